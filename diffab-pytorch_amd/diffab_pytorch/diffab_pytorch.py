"""DiffAb module surface over the HIP engine (libdiffab_hip.so, gfx950).

Mirrors the reference's ``diffab_pytorch/diffab_pytorch.py`` for the diffusion / denoise hot path:
InvariantPointAttentionLayer (:339-465), InvariantPointAttentionModule (:468-498), Denoiser (:501-607),
OrientationLoss (:610-625) and DiffAb (:628-931) keep their constructor signatures, method names,
output dict keys and ``state_dict`` keys/shapes, so a checkpoint of the
reference loads unchanged and callers need no edits.  The ``nn.Module`` objects only own the
parameters; every forward is one C-ABI call into the HIP library - there is no ATen fallback.

The context encoders ResidueEmbedding / PairEmbedding (the step just before the hot path) also run
on HIP, forward and backward (the reference itself cannot back-propagate through PairEmbedding: in-place product at
diffab_pytorch.py:295-301; the backward here is the gradient of the same forward with that product out of place), so
DiffAb.training_step on a reference batch dict trains all 2 538 468 parameters.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Dict, Optional, Tuple

import torch
import torch.nn as nn

from . import _hip
from .diffusion import CoordinateDiffuser, OrientationDiffuser, SequenceDiffuser, cosine_variance_schedule, even_steps, jump_coefficients
from . import so3 as _so3
from . import features as _features
from . import guidance as _guidance
from . import patch as _patch
from . import refine as _refine
from . import steering as _steering
from . import temperature as _temperature

try:  # LightningModule hooks when Lightning is installed; a plain nn.Module otherwise
    import pytorch_lightning as pl

    _ModuleBase = pl.LightningModule
except ImportError:  # pragma: no cover - this image has no pytorch_lightning

    class _ModuleBase(nn.Module):
        def log_dict(self, *args, **kwargs):
            pass

        def log(self, *args, **kwargs):
            pass


CA_IDX = 1  # protstruc.general.ATOM.CA (reference diffab_pytorch.py:9, :820)
# DiffAb.sample(mode=...): (generate_structure, generate_sequence) of encode_context, and the modality the sampler keeps as given
SAMPLE_MODES = {
    "codesign": (True, True, 0),
    "fixed_backbone": (False, True, _hip.FLAG_KEEP_STRUCTURE),
    "structure": (True, False, _hip.FLAG_KEEP_SEQUENCE),
}


# DiffAb.score: evaluated rows per diffab_score_designs chunk when the caller does not choose (tools/score_bench.py, profiles/score.md)
SCORE_ROWS_PER_LAUNCH = 256


def _mode_settings(who: str, mode, generate_structure: bool, generate_sequence: bool):
    """(generate_structure, generate_sequence, DIFFAB_FLAG_KEEP_* bits) of a design mode (sample() and score())."""
    if mode is None:
        return generate_structure, generate_sequence, 0
    if not isinstance(mode, str) or mode not in SAMPLE_MODES:
        raise ValueError(f"{who}: unknown mode {mode!r}; expected None or one of {sorted(SAMPLE_MODES)}")
    if not generate_structure or not generate_sequence:
        raise ValueError(f"{who}: mode={mode!r} sets generate_structure / generate_sequence itself; leave them at their defaults")
    return SAMPLE_MODES[mode]


def _context_map(who: str, context_index, n_rows: int, res_context_emb, pair_context_emb, rows: str) -> torch.Tensor:
    """Host int32 (n_rows,) from `context_index`: the shared contexts must be given, and every entry lie in [0, n_ctx)."""
    if res_context_emb is None or pair_context_emb is None:
        raise ValueError(f"{who}: context_index needs res_context_emb and pair_context_emb (the n_ctx shared contexts)")
    ci = torch.as_tensor(context_index)
    n_ctx = res_context_emb.shape[0]
    if pair_context_emb.shape[0] != n_ctx:
        raise ValueError(f"{who}: res_context_emb has {n_ctx} contexts, pair_context_emb {pair_context_emb.shape[0]}")
    if ci.dim() != 1 or ci.numel() != n_rows or ci.is_floating_point() or ci.is_complex():
        raise ValueError(f"{who}: context_index must be an integer vector of length {n_rows} (the {rows}), "
                         f"got shape {tuple(ci.shape)} {ci.dtype}")
    ci = ci.detach().to("cpu", torch.int64)
    if n_rows and (int(ci.min()) < 0 or int(ci.max()) >= n_ctx):
        raise ValueError(f"{who}: context_index entries must lie in [0, {n_ctx})")
    return ci.to(torch.int32)


def _allowed_aa_host(who: str, allowed_aa, generation_mask, n_rows: int, K: int, V: int, keep: int) -> torch.Tensor:
    """Host bool (n_rows, K, V) of sample()'s `allowed_aa` broadcast to the state rows, after every check made before device work."""
    if keep & _hip.FLAG_KEEP_SEQUENCE:
        raise ValueError(f"{who}: allowed_aa constrains the sequence, which mode='structure' does not diffuse")
    a = torch.as_tensor(allowed_aa)
    if a.dtype != torch.bool:
        raise ValueError(f"{who}: allowed_aa must be a bool tensor (True = class allowed), got {a.dtype}")
    if V > 32:
        raise ValueError(f"{who}: allowed_aa is one 32-bit word per residue on the device; the model's vocabulary V = {V} > 32")
    if a.dim() not in (1, 2, 3) or a.shape[-1] != V:
        raise ValueError(f"{who}: allowed_aa must be (V,), (K, V) or (rows, K, V) with V = {V}, got {tuple(a.shape)}")
    try:
        a = a.detach().cpu().expand(n_rows, K, V)
    except RuntimeError:
        raise ValueError(f"{who}: allowed_aa {tuple(a.shape)} does not broadcast to the state rows ({n_rows}, {K}, {V})") from None
    gm = torch.as_tensor(generation_mask).detach().cpu().bool()
    if tuple(gm.shape) != (n_rows, K):
        raise ValueError(f"{who}: generation_mask is {tuple(gm.shape)}, seq_idx is {(n_rows, K)}")
    empty = (gm & ~a.any(-1)).nonzero()
    if len(empty):
        b, k = (int(v) for v in empty[0])
        raise ValueError(f"{who}: allowed_aa allows no class at {len(empty)} generated residue(s), the first is row {b}, residue {k}")
    return a


def _sample_steps(who: str, steps, t_start: int, t_stop: int, T: int) -> Optional[torch.Tensor]:
    """Host int64 (n,) of sample()'s executed steps, descending, from `steps` (None: every step, the ordinary loop), after every check
    made before device work."""
    if steps is None:
        return None
    if not T >= t_start > t_stop >= 0:
        raise ValueError(f"{who}: steps needs T = {T} >= t_start = {t_start} > t_stop = {t_stop} >= 0")
    if isinstance(steps, bool) or isinstance(steps, float):
        raise ValueError(f"{who}: steps must be an int n or a 1-D list of steps, got {steps!r}")
    if isinstance(steps, int):
        try:
            return even_steps(t_start, t_stop, steps)
        except ValueError as e:
            raise ValueError(f"{who}: {e}") from None
    lt = torch.as_tensor(steps)
    if lt.dim() != 1 or lt.numel() == 0 or lt.dtype == torch.bool or lt.is_floating_point() or lt.is_complex():
        raise ValueError(f"{who}: a step list must be a non-empty 1-D integer list, got shape {tuple(lt.shape)} {lt.dtype}")
    lt = lt.detach().to("cpu", torch.int64)
    if int(lt[0]) != t_start:
        raise ValueError(f"{who}: the step list starts at {int(lt[0])}, the run at t_start = {t_start}")
    if lt.numel() > 1 and not bool((lt[1:] < lt[:-1]).all()):
        raise ValueError(f"{who}: the step list is not strictly descending: {lt.tolist()}")
    if int(lt[-1]) <= t_stop:
        raise ValueError(f"{who}: step {int(lt[-1])} is not above t_stop = {t_stop}")
    return lt


def _trajectory_labels(who: str, trajectory, predictions, t_start: int, t_stop: int, T: int,
                       executed: Optional[torch.Tensor] = None) -> Optional[torch.Tensor]:
    """Host int64 (n,) of sample()'s recorded steps, descending, from `trajectory` (None / False: nothing recorded), after every check
    made before device work.  `executed`: the steps a respaced run executes (labels are among them; a stride k is every k-th of them)."""
    if trajectory is None or trajectory is False:
        if predictions:
            raise ValueError(f"{who}: trajectory_predictions records predictions along a trajectory; give trajectory as well")
        return None
    if not T >= t_start >= t_stop >= 0:
        raise ValueError(f"{who}: a trajectory needs T = {T} >= t_start = {t_start} >= t_stop = {t_stop} >= 0")
    if executed is not None and trajectory is True:
        labels = executed.clone()
    elif executed is not None and isinstance(trajectory, int) and not isinstance(trajectory, bool) and trajectory >= 1:
        labels = executed[::trajectory].clone()
    elif trajectory is True:
        labels = torch.arange(t_start, t_stop, -1, dtype=torch.int64)
    elif isinstance(trajectory, int):
        if trajectory < 1:
            raise ValueError(f"{who}: a trajectory stride must be an int >= 1, got {trajectory}")
        labels = torch.arange(t_start, t_stop, -trajectory, dtype=torch.int64)
    elif isinstance(trajectory, float):
        raise ValueError(f"{who}: trajectory must be True, a stride (int >= 1) or a 1-D list of steps, got the float {trajectory!r}")
    else:
        lt = torch.as_tensor(trajectory)
        if lt.dim() != 1 or lt.numel() == 0 or lt.dtype == torch.bool or lt.is_floating_point() or lt.is_complex():
            raise ValueError(f"{who}: a trajectory list must be a non-empty 1-D integer list of steps, got shape {tuple(lt.shape)} {lt.dtype}")
        lt = lt.detach().to("cpu", torch.int64)
        bad = lt[(lt <= t_stop) | (lt > t_start)]
        if bad.numel():
            raise ValueError(f"{who}: trajectory step {int(bad[0])} outside [t_stop + 1, t_start] = [{t_stop + 1}, {t_start}]")
        if lt.unique().numel() != lt.numel():
            raise ValueError(f"{who}: trajectory lists a step more than once")
        if executed is not None:
            missing = [t for t in lt.tolist() if t not in set(executed.tolist())]
            if missing:
                raise ValueError(f"{who}: trajectory step {missing[0]} is not one of the executed steps {executed.tolist()}")
        labels = lt.sort(descending=True).values
    if labels.numel() == 0:
        raise ValueError(f"{who}: the trajectory records no step (t_start = {t_start}, t_stop = {t_stop})")
    return labels


def _record_c_struct(labels: torch.Tensor, T: int, B: int, K: int, V: int, predictions: bool, device):
    """diffab_sample_record of the recorded steps `labels` (slot j holds step labels[j]) over fresh device tensors: the struct, the
    tensors under their names in sample()'s "trajectory", and the step -> slot table of the device (the caller keeps all three alive
    until the call is enqueued)."""
    n = labels.numel()
    slot_of_step = [-1] * (T + 1)
    for j, t in enumerate(labels.tolist()):
        slot_of_step[t] = j
    slot_dev = torch.empty(T + 1, dtype=torch.int32, device=device)
    traj = {"seq_idx": torch.empty(B, n, K, dtype=torch.int64, device=device),
            "translations": torch.empty(B, n, K, 3, device=device), "orientations": torch.empty(B, n, K, 3, 3, device=device)}
    if predictions:
        traj.update(pred_translations=torch.empty(B, n, K, 3, device=device), pred_orientations=torch.empty(B, n, K, 3, 3, device=device),
                    seq_probs=torch.empty(B, n, K, V, device=device))
    rec = _hip.SampleRecord(n, (C.c_int32 * (T + 1))(*slot_of_step), _hip.ptr(slot_dev),
                            *(_hip.ptr(traj.get(k)) for k in ("seq_idx", "translations", "orientations", "pred_translations",
                                                              "pred_orientations", "seq_probs")))
    return rec, traj, slot_dev


def _steps_c_struct(executed: torch.Tensor, beta_jump: torch.Tensor, alpha_jump: torch.Tensor, plan_dev: torch.Tensor) -> "_hip.SampleSteps":
    """diffab_sample_steps of the executed steps and their jump coefficients ((T + 1,) host tables); plan_dev: 3 (T + 1) int32 words on
    the device (the caller keeps it alive until the call is enqueued)."""
    n = executed.numel()
    return _hip.SampleSteps(n, (C.c_int32 * n)(*executed.tolist()), (C.c_float * beta_jump.numel())(*beta_jump.tolist()),
                            (C.c_float * alpha_jump.numel())(*alpha_jump.tolist()), _hip.ptr(plan_dev))


def _pack_allowed_aa(allowed: torch.Tensor) -> torch.Tensor:
    """(..., V) bool on the device -> (...) int32 words, bit v = class v allowed (the layout of diffab_sample_options.allowed)."""
    bits = torch.ones((), dtype=torch.int64, device=allowed.device) << torch.arange(allowed.shape[-1], device=allowed.device)
    words = (allowed.to(torch.int64) * bits).sum(-1)
    return torch.where(words >= 1 << 31, words - (1 << 32), words).to(torch.int32).contiguous()


def _check_encode_fields(who: str, xyz, atom_mask, chain_idx) -> None:
    need = {"atom_mask": atom_mask, "chain_idx": chain_idx}
    missing = [k for k, v in need.items() if v is None]
    if missing or xyz.dim() != 4:
        raise ValueError(f"{who}: without res_context_emb / pair_context_emb the contexts are computed by encode_context, "
                         f"which needs all-atom xyz (B,K,A,3) and the batch fields {sorted(need)}; missing: "
                         f"{missing if missing else 'xyz is not (B,K,A,3)'}")


def _named(module: nn.Module) -> Dict[str, torch.Tensor]:
    return dict(module.named_parameters())


def _wants_grad(module: Optional[nn.Module], *tensors) -> bool:
    """True when the caller expects a differentiable result: autograd is on and an input or a parameter requires grad."""
    if not torch.is_grad_enabled():
        return False
    if any(torch.is_tensor(t_) and t_.requires_grad for t_ in tensors):
        return True
    return module is not None and any(p.requires_grad for p in module.parameters())


class _AngularEncodingFn(torch.autograd.Function):
    """AngularEncoding on HIP; differentiable in x like the reference's plain torch code (diffab_angular_encoding_bwd)."""

    @staticmethod
    def forward(ctx, x, num_funcs: int):
        lib = _hip.lib()
        xd = _hip.dev_f32(x)
        out = torch.empty(*xd.shape[:-1], xd.shape[-1] * (4 * num_funcs + 1), dtype=torch.float32, device=xd.device)
        _hip.check(lib.diffab_angular_encoding(_hip.ptr(xd), xd.numel(), num_funcs, _hip.ptr(out), _hip.stream_ptr()),
                   "diffab_angular_encoding")
        ctx.save_for_backward(out)
        ctx.num_funcs, ctx.x_shape, ctx.x_device, ctx.x_dtype = num_funcs, tuple(x.shape), x.device, x.dtype
        return out.to(x.device)

    @staticmethod
    def backward(ctx, g):
        (out,) = ctx.saved_tensors
        lib = _hip.lib()
        gd = _hip.dev_f32(g)
        dx = torch.empty(ctx.x_shape, dtype=torch.float32, device=out.device)
        _hip.check(lib.diffab_angular_encoding_bwd(_hip.ptr(out), _hip.ptr(gd), dx.numel(), ctx.num_funcs, _hip.ptr(dx), _hip.stream_ptr()),
                   "diffab_angular_encoding_bwd")
        return dx.to(device=ctx.x_device, dtype=ctx.x_dtype), None


class AngularEncoding(nn.Module):
    """[x, sin(f x), cos(f x)] with f = [1..n, 1/1..1/n] per input value (reference diffab_pytorch.py:20-54); one HIP kernel, and
    differentiable in x as the reference's torch expression is."""

    def __init__(self, num_funcs=3):
        super().__init__()
        self.num_funcs = num_funcs
        self.freq_bands = torch.tensor([i + 1.0 for i in range(num_funcs)] + [1.0 / (i + 1.0) for i in range(num_funcs)]).float()

    def get_output_dimension(self, d_in):
        return d_in * (self.num_funcs * 2 * 2 + 1)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        return _AngularEncodingFn.apply(x, self.num_funcs)


class _FramesFn(torch.autograd.Function):
    """euclidean_transform / inverse_euclidean_transform on HIP; differentiable in the points (the opposite rotation of the cotangent,
    same kernel with t = NULL) and in the frames r, t (diffab_frames_bwd), as the reference's einsums are (:315-336)."""

    @staticmethod
    def forward(ctx, x, r, t, invert: bool):
        lib = _hip.lib()
        xd, rd, td = _hip.dev_f32(x), _hip.dev_f32(r), _hip.dev_f32(t)
        B, N, L, P = xd.shape[:4]
        out = torch.empty_like(xd)
        fn = lib.diffab_frames_invert if invert else lib.diffab_frames_apply
        _hip.check(fn(_hip.ptr(xd), _hip.ptr(rd), _hip.ptr(td), _hip.ptr(out), B, N, L, P, _hip.stream_ptr()), "diffab_frames")
        ctx.invert, ctx.shape, ctx.devs = invert, (B, N, L, P), (x.device, r.device, t.device)
        ctx.save_for_backward(xd, rd, td)
        return out.to(x.device)

    @staticmethod
    def backward(ctx, g):
        lib = _hip.lib()
        xd, rd, td = ctx.saved_tensors
        gd = _hip.dev_f32(g)
        B, N, L, P = ctx.shape
        dx = dr = dt = None
        if ctx.needs_input_grad[0]:
            dx = torch.empty_like(gd)
            fn = lib.diffab_frames_apply if ctx.invert else lib.diffab_frames_invert  # d x = g R^T (apply) | g R (invert)
            _hip.check(fn(_hip.ptr(gd), _hip.ptr(rd), None, _hip.ptr(dx), B, N, L, P, _hip.stream_ptr()), "diffab_frames (backward)")
            dx = dx.to(ctx.devs[0])
        if ctx.needs_input_grad[1] or ctx.needs_input_grad[2]:
            dr = torch.empty_like(rd) if ctx.needs_input_grad[1] else None
            dt = torch.empty_like(td) if ctx.needs_input_grad[2] else None
            _hip.check(lib.diffab_frames_bwd(_hip.ptr(xd), _hip.ptr(rd), _hip.ptr(td), _hip.ptr(gd), int(ctx.invert), _hip.ptr(dr), _hip.ptr(dt),
                                             B, N, L, P, _hip.stream_ptr()), "diffab_frames_bwd")
            dr = dr.to(ctx.devs[1]) if dr is not None else None
            dt = dt.to(ctx.devs[2]) if dt is not None else None
        return dx, dr, dt, None


def euclidean_transform(x, r, t):
    """global = x R + t for points x (b, n heads, l, p, 3), r (b, l, 3, 3), t (b, l, 3) (reference diffab_pytorch.py:315-324)."""
    return _FramesFn.apply(x, r, t, False)


def inverse_euclidean_transform(x, r, t):
    """local = (x - t) R^T (reference diffab_pytorch.py:327-336)."""
    return _FramesFn.apply(x, r, t, True)


class _IpaLayerFn(torch.autograd.Function):
    """InvariantPointAttentionLayer.forward under autograd: taped HIP forward + HIP backward from d y (diffab_ipa_layer_fwd_taped /
    diffab_ipa_layer_bwd): gradients of the layer's ten parameters, of x and of the pair embedding."""

    @staticmethod
    def forward(ctx, layer, flags, x, e, r, t, *params):
        lib = _hip.lib()
        names = [n for n, _ in layer.named_parameters()]
        xd, ed, rd, td = (_hip.dev_f32(a) for a in (x, e, r, t))
        B, K = xd.shape[:2]
        d = layer.dims
        dims = _hip.make_dims(B, K, d["D"], d["C"], d["H"], d["DS"], d["PQ"], d["PV"], 1)
        keep: list = []
        w = _hip.ipa_layer_weights(dict(zip(names, params)), keep)
        tape = _hip.workspace(lib.diffab_ipa_layer_tape_bytes(C.byref(dims)))
        y = torch.empty_like(xd)
        _hip.check(lib.diffab_ipa_layer_fwd_taped(C.byref(dims), C.byref(w), _hip.ptr(xd), _hip.ptr(ed), _hip.ptr(rd), _hip.ptr(td), _hip.ptr(y),
                                                  _hip.ptr(tape), tape.numel(), flags, _hip.stream_ptr()), "diffab_ipa_layer_fwd_taped")
        ctx.layer, ctx.names, ctx.dims = layer, names, dims
        ctx.need_e = ctx.needs_input_grad[3]
        ctx.need_frames = (ctx.needs_input_grad[4], ctx.needs_input_grad[5])  # d r, d t (reference :315-336 is differentiable in them)
        ctx.devs = (x.device, e.device, [p.device for p in params], r.device, t.device)
        ctx.save_for_backward(ed, rd, td, tape, *params)
        return y.to(x.device)

    @staticmethod
    def backward(ctx, dy):
        lib = _hip.lib()
        ed, rd, td, tape = ctx.saved_tensors[:4]
        params = ctx.saved_tensors[4:]
        dims = ctx.dims
        keep: list = []
        w = _hip.ipa_layer_weights(dict(zip(ctx.names, params)), keep)
        grads, ctx.layer._flat_grad = _zero_grads_like(params)
        g = _hip.ipa_layer_weights(dict(zip(ctx.names, grads)), keep)
        dyd = _hip.dev_f32(dy)
        dx = torch.empty_like(dyd)
        de = torch.zeros_like(ed) if ctx.need_e else None
        dr = torch.empty_like(rd) if ctx.need_frames[0] else None
        dt = torch.empty_like(td) if ctx.need_frames[1] else None
        ws = _hip.workspace(lib.diffab_ipa_layer_bwd_workspace_bytes(C.byref(dims)))
        _hip.check(lib.diffab_ipa_layer_bwd(C.byref(dims), C.byref(w), C.byref(g), _hip.ptr(ed), _hip.ptr(rd), _hip.ptr(td), _hip.ptr(dyd),
                                            _hip.ptr(dx), _hip.ptr(de), _hip.ptr(dr), _hip.ptr(dt), _hip.ptr(tape), tape.numel(), _hip.ptr(ws),
                                            ws.numel(), _hip.stream_ptr()), "diffab_ipa_layer_bwd")
        x_dev, e_dev, p_devs, r_dev, t_dev = ctx.devs
        return (None, None, dx.to(x_dev), de.to(e_dev) if ctx.need_e else None, dr.to(r_dev) if dr is not None else None,
                dt.to(t_dev) if dt is not None else None) + tuple(gr.to(dv) for gr, dv in zip(grads, p_devs))


class InvariantPointAttentionLayer(nn.Module):
    """Reference IPA layer: no LayerNorm/residual/transition, raw gamma, unmasked (diffab_pytorch.py:339-465)."""

    def __init__(self, d_residue_emb, d_pair_emb, d_scalar_per_head=16, n_query_point_per_head=4, n_value_point_per_head=4, n_head=8,
                 use_pair_bias=True):
        super().__init__()
        self.n_head = n_head
        self.use_pair_bias = use_pair_bias
        # use_pair_bias=False (reference :348-385, not on the DiffAb path): no to_pair_bias, two independent logits, no pair block in
        # to_out's input; on the HIP side that is C = 0 on the any-dims kernels (forward and backward), e is not read
        self.dims = dict(D=d_residue_emb, C=d_pair_emb if use_pair_bias else 0, H=n_head, DS=d_scalar_per_head, PQ=n_query_point_per_head,
                         PV=n_value_point_per_head)
        d_scalar = d_scalar_per_head * n_head
        # creation order = the reference's, so a seeded construction draws identical initial weights
        self.to_q_scalar = nn.Linear(d_residue_emb, d_scalar, bias=False)
        self.to_k_scalar = nn.Linear(d_residue_emb, d_scalar, bias=False)
        self.to_v_scalar = nn.Linear(d_residue_emb, d_scalar, bias=False)
        if use_pair_bias:
            self.to_pair_bias = nn.Linear(d_pair_emb, n_head, bias=False)
        self.to_q_point = nn.Linear(d_residue_emb, n_query_point_per_head * 3 * n_head, bias=False)
        self.to_k_point = nn.Linear(d_residue_emb, n_query_point_per_head * 3 * n_head, bias=False)
        self.to_v_point = nn.Linear(d_residue_emb, n_value_point_per_head * 3 * n_head, bias=False)
        self.gamma = nn.Parameter(torch.log(torch.exp(torch.ones(n_head)) - 1.0))
        self.to_out = nn.Linear(d_scalar + (d_pair_emb * n_head if use_pair_bias else 0) + n_value_point_per_head * 3 * n_head +
                                n_value_point_per_head * n_head, d_residue_emb)

    def forward(self, x, e, r, t, *, flags: int = 0):
        lib = _hip.lib()
        if x.shape[0] == 0 or x.shape[1] == 0:  # empty batch / empty patch: nothing to launch (the reference's einsums return empty too)
            return torch.zeros(x.shape, dtype=torch.float32, device=x.device)
        if _wants_grad(self, x, e, r, t):  # differentiable like the reference's forward (:389-465): taped HIP forward + HIP backward
            return _IpaLayerFn.apply(self, flags & ~_hip.FLAG_PAIR_PLANES, x, e, r, t, *[p for _, p in self.named_parameters()])
        xd, ed, rd, td = (_hip.dev_f32(a) for a in (x, e, r, t))
        B, K = xd.shape[:2]
        d = self.dims
        dims = _hip.make_dims(B, K, d["D"], d["C"], d["H"], d["DS"], d["PQ"], d["PV"], 1)
        keep: list = []
        w = _hip.ipa_layer_weights(_named(self), keep)
        ws = _hip.workspace(lib.diffab_denoise_workspace_bytes(C.byref(dims)))
        y = torch.empty_like(xd)
        _hip.check(lib.diffab_ipa_layer_fwd(C.byref(dims), C.byref(w), _hip.ptr(xd), _hip.ptr(ed), _hip.ptr(rd), _hip.ptr(td), _hip.ptr(y),
                                            _hip.ptr(ws), ws.numel(), flags, _hip.stream_ptr()), "diffab_ipa_layer_fwd")
        return y.to(x.device)


class InvariantPointAttentionModule(nn.Module):
    """x <- layer(x, e, R, t) for each layer, same e/R/t (diffab_pytorch.py:468-498)."""

    def __init__(self, n_layers, d_residue_emb, d_pair_emb, d_scalar_per_head, n_query_point_per_head, n_value_point_per_head, n_head):
        super().__init__()
        self.layers = nn.ModuleList([
            InvariantPointAttentionLayer(d_residue_emb, d_pair_emb, d_scalar_per_head, n_query_point_per_head, n_value_point_per_head, n_head)
            for _ in range(n_layers)
        ])

    def forward(self, res_emb, pair_emb, orientations, translations, *, flags: int = 0):
        dev = res_emb.device
        x, e, r, t = (_hip.dev_f32(a) for a in (res_emb, pair_emb, orientations, translations))
        for layer in self.layers:
            x = layer(x, e, r, t, flags=flags)
        return x.to(dev)


class Denoiser(nn.Module):
    """eps-hat, O0-hat and the aa posterior from (s_t, x_t, O_t, contexts, beta) (diffab_pytorch.py:501-607)."""

    def __init__(self, d_residue_emb, d_pair_emb, n_ipa_layers, d_scalar_per_head, n_query_point_per_head, n_value_point_per_head, n_head,
                 aa_vocab_size):
        super().__init__()
        D = d_residue_emb
        self.dims = dict(D=D, C=d_pair_emb, H=n_head, DS=d_scalar_per_head, PQ=n_query_point_per_head, PV=n_value_point_per_head,
                         NL=n_ipa_layers, V=aa_vocab_size)
        self.sequence_embedding = nn.Embedding(25, D)
        self.to_res_emb = nn.Sequential(nn.Linear(D * 2, D), nn.ReLU(), nn.Linear(D, D))
        self.ipa = InvariantPointAttentionModule(n_ipa_layers, D, d_pair_emb, d_scalar_per_head, n_query_point_per_head,
                                                 n_value_point_per_head, n_head)

        def head(n_out, softmax=False):
            mods = [nn.Linear(D + 3, D), nn.ReLU(), nn.Linear(D, D), nn.ReLU(), nn.Linear(D, n_out)]
            if softmax:
                mods.append(nn.Softmax(dim=-1))
            return nn.Sequential(*mods)

        self.coordinate_denoising = head(3)
        self.orientation_denoising = head(3)
        self.sequence_denoising = head(aa_vocab_size, softmax=True)

    def hip_weights(self) -> _hip.DenoiserWeightsOnDevice:
        return _hip.DenoiserWeightsOnDevice(_named(self), self.dims["NL"])

    def hip_dims(self, B: int, K: int) -> _hip.Dims:
        d = self.dims
        return _hip.make_dims(B, K, d["D"], d["C"], d["H"], d["DS"], d["PQ"], d["PV"], d["NL"], d["V"])

    def forward(self, seq_idx_t, translations_t, orientations_t, res_context_emb, pair_context_emb, beta, generation_mask=None,
                residue_mask=None, *, return_logits: bool = False, flags: int = 0) -> Dict[str, torch.Tensor]:
        # generation_mask / residue_mask are accepted and ignored, exactly like the reference (:566-567).
        lib = _hip.lib()
        if seq_idx_t.shape[0] == 0 or seq_idx_t.shape[1] == 0:  # empty batch: empty outputs, like the reference
            B0, K0 = seq_idx_t.shape[:2]
            dev0, V0 = translations_t.device, self.dims["V"]
            out0 = {"translations_eps": torch.zeros(B0, K0, 3, device=dev0), "orientations_t0": torch.zeros(B0, K0, 3, 3, device=dev0),
                    "seq_posterior": torch.zeros(B0, K0, V0, device=dev0)}
            if return_logits:
                out0["aa_logits"] = torch.zeros(B0, K0, V0, device=dev0)
                out0["res_emb"] = torch.zeros(B0, K0, self.dims["D"], device=dev0)
            return out0
        if not return_logits and _wants_grad(self, res_context_emb, pair_context_emb, translations_t, orientations_t):
            # differentiable like the reference's forward (:558-607): taped HIP forward + HIP backward from the outputs' cotangents
            # (return_logits=True is an inference-only diagnostic of this package: detached outputs)
            eps, O0, post = _DenoiserFn.apply(self, flags & ~_hip.FLAG_PAIR_PLANES, seq_idx_t, translations_t, orientations_t, beta,
                                              res_context_emb, pair_context_emb, *[p for _, p in self.named_parameters()])
            return {"translations_eps": eps, "orientations_t0": O0, "seq_posterior": post}
        out_dev = translations_t.device
        seq = _hip.dev_i64(seq_idx_t)
        x, O, rc, pc, bt = (_hip.dev_f32(a) for a in (translations_t, orientations_t, res_context_emb, pair_context_emb, beta))
        B, K = seq.shape
        dims = self.hip_dims(B, K)
        w = self.hip_weights()
        ws = _hip.workspace(lib.diffab_denoise_workspace_bytes(C.byref(dims)))
        dev = seq.device
        eps = torch.empty(B, K, 3, dtype=torch.float32, device=dev)
        O0 = torch.empty(B, K, 3, 3, dtype=torch.float32, device=dev)
        post = torch.empty(B, K, dims.V, dtype=torch.float32, device=dev)
        logits = torch.empty(B, K, dims.V, dtype=torch.float32, device=dev) if return_logits else None
        h = torch.empty(B, K, dims.D, dtype=torch.float32, device=dev) if return_logits else None
        _hip.check(lib.diffab_denoise_step_fwd(C.byref(dims), C.byref(w.struct), _hip.ptr(seq), _hip.ptr(x), _hip.ptr(O), _hip.ptr(rc),
                                               _hip.ptr(pc), _hip.ptr(bt), _hip.ptr(eps), _hip.ptr(O0), _hip.ptr(post), _hip.ptr(logits),
                                               _hip.ptr(h), _hip.ptr(ws), ws.numel(), flags, _hip.stream_ptr()), "diffab_denoise_step_fwd")
        out = {"translations_eps": eps.to(out_dev), "orientations_t0": O0.to(out_dev), "seq_posterior": post.to(out_dev)}
        if return_logits:
            out["aa_logits"] = logits.to(out_dev)
            out["res_emb"] = h.to(out_dev)
        return out


class _DenoiserFn(torch.autograd.Function):
    """Denoiser.forward under autograd: diffab_denoise_step_fwd_taped, then diffab_denoise_step_bwd from the cotangents of
    (eps-hat, O0-hat, posterior): gradients of every denoiser parameter and of the two context embeddings."""

    @staticmethod
    def forward(ctx, denoiser, flags, seq_t, x_t, O_t, beta, res_ctx, pair_ctx, *params):
        lib = _hip.lib()
        names = [n for n, _ in denoiser.named_parameters()]
        seq = _hip.dev_i64(seq_t)
        x, O, bt, rc, pc = (_hip.dev_f32(a) for a in (x_t, O_t, beta, res_ctx, pair_ctx))
        B, K = seq.shape
        dims = denoiser.hip_dims(B, K)
        w = _hip.DenoiserWeightsOnDevice(dict(zip(names, params)), denoiser.dims["NL"])
        dev = seq.device
        eps = torch.empty(B, K, 3, dtype=torch.float32, device=dev)
        O0 = torch.empty(B, K, 3, 3, dtype=torch.float32, device=dev)
        post = torch.empty(B, K, dims.V, dtype=torch.float32, device=dev)
        tape = _hip.workspace(lib.diffab_train_tape_bytes(C.byref(dims)))
        _hip.check(lib.diffab_denoise_step_fwd_taped(C.byref(dims), C.byref(w.struct), _hip.ptr(seq), _hip.ptr(x), _hip.ptr(O), _hip.ptr(rc),
                                                     _hip.ptr(pc), _hip.ptr(bt), _hip.ptr(eps), _hip.ptr(O0), _hip.ptr(post), _hip.ptr(tape),
                                                     tape.numel(), flags, _hip.stream_ptr()), "diffab_denoise_step_fwd_taped")
        ctx.denoiser, ctx.names, ctx.dims = denoiser, names, dims
        ctx.need = (ctx.needs_input_grad[6], ctx.needs_input_grad[7])
        ctx.need_frames = (ctx.needs_input_grad[3], ctx.needs_input_grad[4])  # d translations_t, d orientations_t
        ctx.devs = (res_ctx.device, pair_ctx.device, [p.device for p in params], x_t.device, O_t.device)
        ctx.save_for_backward(seq, x, O, pc, post, tape, *params)
        out_dev = x_t.device
        return eps.to(out_dev), O0.to(out_dev), post.to(out_dev)

    @staticmethod
    def backward(ctx, g_eps, g_O0, g_post):
        lib = _hip.lib()
        seq, x, O, pc, post, tape = ctx.saved_tensors[:6]
        params = ctx.saved_tensors[6:]
        dims = ctx.dims
        B, K = seq.shape
        w = _hip.DenoiserWeightsOnDevice(dict(zip(ctx.names, params)), ctx.denoiser.dims["NL"])
        grads, ctx.denoiser._flat_grad = _zero_grads_like(params)
        g = _hip.DenoiserWeightsOnDevice(dict(zip(ctx.names, grads)), ctx.denoiser.dims["NL"])
        ce, cO, cp = (None if t_ is None else _hip.dev_f32(t_) for t_ in (g_eps, g_O0, g_post))
        d_rc = torch.empty(B, K, dims.D, dtype=torch.float32, device=seq.device)
        d_pc = torch.zeros_like(pc) if ctx.need[1] else None
        d_x = torch.empty_like(x) if ctx.need_frames[0] else None
        d_O = torch.empty_like(O) if ctx.need_frames[1] else None
        ws = _hip.workspace(lib.diffab_train_workspace_bytes(C.byref(dims)))
        _hip.check(lib.diffab_denoise_step_bwd(C.byref(dims), C.byref(w.struct), C.byref(g.struct), _hip.ptr(seq), _hip.ptr(x), _hip.ptr(O),
                                               _hip.ptr(pc), _hip.ptr(post), _hip.ptr(ce), _hip.ptr(cO), _hip.ptr(cp), _hip.ptr(d_rc),
                                               _hip.ptr(d_pc), _hip.ptr(d_x), _hip.ptr(d_O), _hip.ptr(tape), tape.numel(), _hip.ptr(ws), ws.numel(),
                                               _hip.stream_ptr()), "diffab_denoise_step_bwd")
        rc_dev, pc_dev, p_devs, x_dev, O_dev = ctx.devs
        return (None, None, None, d_x.to(x_dev) if d_x is not None else None, d_O.to(O_dev) if d_O is not None else None, None,
                d_rc.to(rc_dev) if ctx.need[0] else None, d_pc.to(pc_dev) if ctx.need[1] else None) + \
            tuple(gr.to(dv) for gr, dv in zip(grads, p_devs))


class _OrientationLossFn(torch.autograd.Function):
    """OrientationLoss under autograd: diffab_orientation_loss, then diffab_orientation_loss_bwd."""

    @staticmethod
    def forward(ctx, pred, target, reduction):
        lib = _hip.lib()
        p, t = _hip.dev_f32(pred), _hip.dev_f32(target)
        n = p.numel() // 9
        elems = torch.empty_like(p) if reduction == "none" else None
        total = torch.empty(1, dtype=torch.float32, device=p.device)
        _hip.check(lib.diffab_orientation_loss(_hip.ptr(p), _hip.ptr(t), n, _hip.ptr(elems), _hip.ptr(total), _hip.stream_ptr()),
                   "diffab_orientation_loss")
        ctx.reduction, ctx.n = reduction, n
        ctx.devs = (pred.device, target.device)
        ctx.save_for_backward(p, t)
        out = elems if reduction == "none" else (total[0] / float(9 * n) if reduction == "mean" else total[0])
        return out.to(device=pred.device, dtype=pred.dtype)

    @staticmethod
    def backward(ctx, g):
        lib = _hip.lib()
        p, t = ctx.saved_tensors
        gd = _hip.dev_f32(g)
        ge, gt = (gd, None) if ctx.reduction == "none" else (None, (gd / float(9 * ctx.n) if ctx.reduction == "mean" else gd).reshape(1))
        dp = torch.empty_like(p) if ctx.needs_input_grad[0] else None
        dt = torch.empty_like(t) if ctx.needs_input_grad[1] else None
        _hip.check(lib.diffab_orientation_loss_bwd(_hip.ptr(p), _hip.ptr(t), ctx.n, _hip.ptr(ge), _hip.ptr(gt), _hip.ptr(dp), _hip.ptr(dt),
                                                   _hip.stream_ptr()), "diffab_orientation_loss_bwd")
        return (None if dp is None else dp.to(ctx.devs[0]), None if dt is None else dt.to(ctx.devs[1]), None)


class _HotpathTrainStep(torch.autograd.Function):
    """(seq KL, translation MSE, orientation loss) of one noised batch, differentiable w.r.t. every denoiser parameter and
    the two context embeddings.  Forward = diffab_train_step_fwd (Denoiser forward with a saved-activation tape + the masked
    losses of reference diffab_pytorch.py:856-880), backward = diffab_train_step_bwd.  Both are single C-ABI calls."""

    @staticmethod
    def forward(ctx, denoiser, seq_t, x_t, O_t, beta, true_post, true_eps, true_O0, gen_mask, res_mask, res_ctx, pair_ctx, *params):
        lib = _hip.lib()
        names = [n for n, _ in denoiser.named_parameters()]
        seq = _hip.dev_i64(seq_t)
        x, O, bt, tp, te, tO, rc, pc = (_hip.dev_f32(a) for a in (x_t, O_t, beta, true_post, true_eps, true_O0, res_ctx, pair_ctx))
        gm, rm = _hip.dev_mask(gen_mask), _hip.dev_mask(res_mask)
        B, K = seq.shape
        dims = denoiser.hip_dims(B, K)
        w = _hip.DenoiserWeightsOnDevice(dict(zip(names, params)), denoiser.dims["NL"])
        dev = seq.device
        eps = torch.empty(B, K, 3, dtype=torch.float32, device=dev)
        O0 = torch.empty(B, K, 3, 3, dtype=torch.float32, device=dev)
        post = torch.empty(B, K, dims.V, dtype=torch.float32, device=dev)
        losses = torch.empty(3, dtype=torch.float32, device=dev)
        tape = _hip.workspace(lib.diffab_train_tape_bytes(C.byref(dims)))
        _hip.check(lib.diffab_train_step_fwd(C.byref(dims), C.byref(w.struct), _hip.ptr(seq), _hip.ptr(x), _hip.ptr(O), _hip.ptr(rc),
                                             _hip.ptr(pc), _hip.ptr(bt), _hip.ptr(tp), _hip.ptr(te), _hip.ptr(tO), _hip.ptr(gm), _hip.ptr(rm),
                                             _hip.ptr(eps), _hip.ptr(O0), _hip.ptr(post), _hip.ptr(losses), _hip.ptr(tape), tape.numel(), 0,
                                             _hip.stream_ptr()), "diffab_train_step_fwd")
        ctx.denoiser, ctx.names, ctx.dims = denoiser, names, dims
        ctx.need = (ctx.needs_input_grad[10], ctx.needs_input_grad[11])
        ctx.out_devs = (res_ctx.device, pair_ctx.device, [p.device for p in params])
        ctx.save_for_backward(seq, x, O, pc, eps, O0, post, tp, te, tO, gm, rm, tape, *params)
        ctx.mark_non_differentiable(eps, O0, post)
        return losses, eps, O0, post

    @staticmethod
    def backward(ctx, g_losses, _g_eps, _g_O0, _g_post):
        lib = _hip.lib()
        seq, x, O, pc, eps, O0, post, tp, te, tO, gm, rm, tape = ctx.saved_tensors[:13]
        params = ctx.saved_tensors[13:]
        dims = ctx.dims
        B, K = seq.shape
        w = _hip.DenoiserWeightsOnDevice(dict(zip(ctx.names, params)), ctx.denoiser.dims["NL"])
        # one zero-filled flat buffer, one view per parameter (256-byte aligned): a fill per parameter is 100+ tiny launches per step;
        # kept on the module so that the data-parallel all-reduce can run on the bucket itself (DiffAb.gradient_buckets)
        grads, ctx.denoiser._flat_grad = _zero_grads_like(params)
        g = _hip.DenoiserWeightsOnDevice(dict(zip(ctx.names, grads)), ctx.denoiser.dims["NL"])
        up = _hip.dev_f32(g_losses)
        d_rc = torch.empty(B, K, dims.D, dtype=torch.float32, device=seq.device)
        d_pc = torch.zeros_like(pc) if ctx.need[1] else None
        ws = _hip.workspace(lib.diffab_train_workspace_bytes(C.byref(dims)))
        _hip.check(lib.diffab_train_step_bwd(C.byref(dims), C.byref(w.struct), C.byref(g.struct), _hip.ptr(seq), _hip.ptr(x), _hip.ptr(O),
                                             _hip.ptr(pc), _hip.ptr(eps), _hip.ptr(O0), _hip.ptr(post), _hip.ptr(tp), _hip.ptr(te), _hip.ptr(tO),
                                             _hip.ptr(gm), _hip.ptr(rm), _hip.ptr(up), _hip.ptr(d_rc), _hip.ptr(d_pc), _hip.ptr(tape),
                                             tape.numel(), _hip.ptr(ws), ws.numel(), _hip.stream_ptr()), "diffab_train_step_bwd")
        rc_dev, pc_dev, p_devs = ctx.out_devs
        out_params = tuple(gr.to(dv) for gr, dv in zip(grads, p_devs))
        return (None,) * 10 + (d_rc.to(rc_dev) if ctx.need[0] else None, d_pc.to(pc_dev) if ctx.need[1] else None) + out_params


class OrientationLoss(nn.Module):
    """(pred^T target - I)^2; reduction 'none' | 'mean' | 'sum' (diffab_pytorch.py:610-625)."""

    def __init__(self, reduction="mean"):
        super().__init__()
        self.reduction = reduction

    def forward(self, pred_rotmat: torch.Tensor, target_rotmat: torch.Tensor) -> torch.Tensor:
        lib = _hip.lib()
        if _wants_grad(None, pred_rotmat, target_rotmat):
            return _OrientationLossFn.apply(pred_rotmat, target_rotmat, self.reduction)
        p, t = _hip.dev_f32(pred_rotmat), _hip.dev_f32(target_rotmat)
        n = p.numel() // 9
        elems = torch.empty_like(p) if self.reduction == "none" else None
        total = torch.empty(1, dtype=torch.float32, device=p.device)
        _hip.check(lib.diffab_orientation_loss(_hip.ptr(p), _hip.ptr(t), n, _hip.ptr(elems), _hip.ptr(total), _hip.stream_ptr()),
                   "diffab_orientation_loss")
        if self.reduction == "none":
            out = elems
        elif self.reduction == "mean":
            out = total[0] / float(9 * n)
        else:
            out = total[0]
        return out.to(device=pred_rotmat.device, dtype=pred_rotmat.dtype)


def _opt_mask(m):
    return None if m is None else _hip.dev_mask(m)


_RES_KEYS = ("amino_acid_type_embedding.weight", "chain_embedding.weight", "mlp.0.weight", "mlp.0.bias", "mlp.2.weight", "mlp.2.bias",
             "mlp.4.weight", "mlp.4.bias", "mlp.6.weight", "mlp.6.bias")
_PAIR_KEYS = ("aa_pair_type_embedding.weight", "relpos_embedding.weight", "pair2distcoef.weight", "distance_embedding.0.weight",
              "distance_embedding.0.bias", "distance_embedding.2.weight", "distance_embedding.2.bias", "mlp.0.weight", "mlp.0.bias",
              "mlp.2.weight", "mlp.2.bias", "mlp.4.weight", "mlp.4.bias")


def _zero_grads_like(params):
    """One zero-filled flat buffer with a (256-byte aligned) view per parameter: the HIP backward accumulates into it."""
    offs, total = [], 0
    for p in params:
        offs.append(total)
        total += (p.numel() + 63) // 64 * 64
    flat = torch.zeros(total, dtype=torch.float32, device=_hip.device())
    return [flat[o:o + p.numel()].view(p.shape) for o, p in zip(offs, params)], flat


class _ResidueEmbeddingFn(torch.autograd.Function):
    """ResidueEmbedding forward / backward as two C-ABI calls (the backward recomputes the forward: nothing is taped)."""

    @staticmethod
    def forward(ctx, owner, dims, seq, x, O, dh, ch, am, sm, qm, *params):
        lib = _hip.lib()
        ctx.owner = owner
        ts = [_hip.dev_f32(p) for p in params]
        w = _hip.ResidueEmbWeights(*[_hip.ptr(t_) for t_ in ts])
        ws = _hip.workspace(lib.diffab_residue_embedding_workspace_bytes(C.byref(dims)))
        out = torch.empty(dims.B, dims.K, dims.D, dtype=torch.float32, device=seq.device)
        _hip.check(lib.diffab_residue_embedding_fwd(C.byref(dims), C.byref(w), _hip.ptr(seq), _hip.ptr(x), _hip.ptr(O), _hip.ptr(dh),
                                                    _hip.ptr(ch), _hip.ptr(am), _hip.ptr(sm), _hip.ptr(qm), _hip.ptr(out), _hip.ptr(ws),
                                                    ws.numel(), _hip.stream_ptr()), "diffab_residue_embedding_fwd")
        ctx.dims, ctx.masks = dims, (sm, qm)
        ctx.p_devs = [p.device for p in params]
        ctx.save_for_backward(seq, x, O, dh, ch, am, *ts)
        return out

    @staticmethod
    def backward(ctx, d_out):
        lib = _hip.lib()
        seq, x, O, dh, ch, am = ctx.saved_tensors[:6]
        ts = list(ctx.saved_tensors[6:])
        sm, qm = ctx.masks
        dims = ctx.dims
        grads, ctx.owner._flat_grad = _zero_grads_like(ts)
        w = _hip.ResidueEmbWeights(*[_hip.ptr(t_) for t_ in ts])
        g = _hip.ResidueEmbWeights(*[_hip.ptr(t_) for t_ in grads])
        ws = _hip.workspace(lib.diffab_residue_embedding_bwd_workspace_bytes(C.byref(dims)))
        do = _hip.dev_f32(d_out)
        _hip.check(lib.diffab_residue_embedding_bwd(C.byref(dims), C.byref(w), C.byref(g), _hip.ptr(seq), _hip.ptr(x), _hip.ptr(O),
                                                    _hip.ptr(dh), _hip.ptr(ch), _hip.ptr(am), _hip.ptr(sm), _hip.ptr(qm), _hip.ptr(do),
                                                    _hip.ptr(ws), ws.numel(), _hip.stream_ptr()), "diffab_residue_embedding_bwd")
        return (None,) * 10 + tuple(gr.to(dv) for gr, dv in zip(grads, ctx.p_devs))


class _PairEmbeddingFn(torch.autograd.Function):
    """PairEmbedding forward / backward as two C-ABI calls.  The backward is the gradient of the reference's forward with its
    in-place mask product (diffab_pytorch.py:295-301, which makes the reference's own autograd fail) taken out of place."""

    @staticmethod
    def forward(ctx, owner, dims, from_xyz, seq, dm, dh, ri, ri_stride, ch, am, qm, *params):
        lib = _hip.lib()
        ctx.owner = owner
        ts = [_hip.dev_f32(p) for p in params]
        w = _hip.PairEmbWeights(*[_hip.ptr(t_) for t_ in ts])
        ws = _hip.workspace(lib.diffab_pair_embedding_workspace_bytes(C.byref(dims)))
        out = torch.empty(dims.B, dims.K, dims.K, dims.C, dtype=torch.float32, device=seq.device)
        # Taped form (C ABI "Taped form of the PairEmbedding pair"): when a backward will follow and the device has the room, the forward
        # leaves its four hidden activations (8.6 GB at B = 128, K = 128) and the backward does not recompute it.  DIFFAB_PAIR_TAPE=0: off.
        ctx.tape = None
        tape_bytes = lib.diffab_pair_embedding_tape_bytes(C.byref(dims))
        if (tape_bytes and getattr(owner, "_tape_wanted", False) and any(ctx.needs_input_grad) and os.environ.get("DIFFAB_PAIR_TAPE", "1") != "0"
                and torch.cuda.mem_get_info(seq.device)[0] > 2 * tape_bytes):
            ctx.tape = torch.empty(tape_bytes // 4, dtype=torch.float32, device=seq.device)
            _hip.check(lib.diffab_pair_embedding_fwd_taped(C.byref(dims), C.byref(w), _hip.ptr(seq), _hip.ptr(None if from_xyz else dm),
                                                           _hip.ptr(dm if from_xyz else None), _hip.ptr(dh), _hip.ptr(ri), ri_stride, _hip.ptr(ch),
                                                           _hip.ptr(am), _hip.ptr(qm), _hip.ptr(out), _hip.ptr(ctx.tape), tape_bytes, _hip.ptr(ws),
                                                           ws.numel(), _hip.stream_ptr()), "diffab_pair_embedding_fwd_taped")
        else:
            entry = lib.diffab_pair_embedding_xyz_fwd if from_xyz else lib.diffab_pair_embedding_fwd
            _hip.check(entry(C.byref(dims), C.byref(w), _hip.ptr(seq), _hip.ptr(dm), _hip.ptr(dh), _hip.ptr(ri), ri_stride, _hip.ptr(ch),
                             _hip.ptr(am), _hip.ptr(qm), _hip.ptr(out), _hip.ptr(ws), ws.numel(), _hip.stream_ptr()),
                       "diffab_pair_embedding_xyz_fwd" if from_xyz else "diffab_pair_embedding_fwd")
        ctx.dims, ctx.from_xyz, ctx.ri_stride, ctx.qm = dims, from_xyz, ri_stride, qm
        ctx.p_devs = [p.device for p in params]
        ctx.save_for_backward(seq, dm, dh, ri, ch, am, *ts)
        return out

    @staticmethod
    def backward(ctx, d_out):
        lib = _hip.lib()
        seq, dm, dh, ri, ch, am = ctx.saved_tensors[:6]
        ts = list(ctx.saved_tensors[6:])
        dims = ctx.dims
        grads, ctx.owner._flat_grad = _zero_grads_like(ts)
        w = _hip.PairEmbWeights(*[_hip.ptr(t_) for t_ in ts])
        g = _hip.PairEmbWeights(*[_hip.ptr(t_) for t_ in grads])
        ws = _hip.workspace(lib.diffab_pair_embedding_bwd_workspace_bytes(C.byref(dims)))
        do = _hip.dev_f32(d_out)
        if ctx.tape is not None:
            tape, ctx.tape = ctx.tape, None
            _hip.check(lib.diffab_pair_embedding_bwd_taped(C.byref(dims), C.byref(w), C.byref(g), _hip.ptr(seq),
                                                           _hip.ptr(None if ctx.from_xyz else dm), _hip.ptr(dm if ctx.from_xyz else None),
                                                           _hip.ptr(dh), _hip.ptr(ri), ctx.ri_stride, _hip.ptr(ch), _hip.ptr(am), _hip.ptr(ctx.qm),
                                                           _hip.ptr(do), _hip.ptr(tape), tape.numel() * 4, _hip.ptr(ws), ws.numel(),
                                                           _hip.stream_ptr()), "diffab_pair_embedding_bwd_taped")
            del tape
        else:
            _hip.check(lib.diffab_pair_embedding_bwd(C.byref(dims), C.byref(w), C.byref(g), _hip.ptr(seq),
                                                     _hip.ptr(None if ctx.from_xyz else dm), _hip.ptr(dm if ctx.from_xyz else None), _hip.ptr(dh),
                                                     _hip.ptr(ri), ctx.ri_stride, _hip.ptr(ch), _hip.ptr(am), _hip.ptr(ctx.qm), _hip.ptr(do),
                                                     _hip.ptr(ws), ws.numel(), _hip.stream_ptr()), "diffab_pair_embedding_bwd")
        return (None,) * 11 + tuple(gr.to(dv) for gr, dv in zip(grads, ctx.p_devs))


class ResidueEmbedding(nn.Module):
    """Per-residue context embedding (reference diffab_pytorch.py:57-183): same parameters, creation order and forward
    signature; forward and backward are one C-ABI call each (feature gather kernel + four MFMA linears; the backward recomputes them)."""

    def __init__(self, max_n_atoms_per_residue, d_feat):
        super().__init__()
        self.max_n_aa_types = 21
        self.max_n_atoms_per_residue = max_n_atoms_per_residue
        self.d_feat = d_feat
        self.amino_acid_type_embedding = nn.Embedding(self.max_n_aa_types, d_feat)
        self.chain_embedding = nn.Embedding(10, d_feat, padding_idx=0)
        d_in = d_feat + self.max_n_aa_types * max_n_atoms_per_residue * 3 + 3 * (3 * 2 * 2 + 1) + d_feat
        self.mlp = nn.Sequential(nn.Linear(d_in, d_feat * 2), nn.ReLU(), nn.Linear(d_feat * 2, d_feat), nn.ReLU(),
                                 nn.Linear(d_feat, d_feat), nn.ReLU(), nn.Linear(d_feat, d_feat))

    def forward(self, seq_idx, xyz, orientation, dihedrals, chain_idx, atom_mask, structure_context_mask=None,
                sequence_context_mask=None):
        lib = _hip.lib()
        out_dev = xyz.device
        seq, ch = _hip.dev_i64(seq_idx), _hip.dev_i64(chain_idx)
        x, O, dh, am = (_hip.dev_f32(a) for a in (xyz, orientation, dihedrals, atom_mask))
        sm, qm = _opt_mask(structure_context_mask), _opt_mask(sequence_context_mask)
        B, K = seq.shape
        dims = _hip.CtxDims(B, K, self.max_n_atoms_per_residue, self.d_feat, 1, 32)
        p = _named(self)
        out = _ResidueEmbeddingFn.apply(self, dims, seq, x, O, dh, ch, am, sm, qm, *[p[k] for k in _RES_KEYS])
        return out.to(out_dev)


class PairEmbedding(nn.Module):
    """Residue-pair context embedding (reference diffab_pytorch.py:186-312), forward and backward on HIP.  Reference quirks kept: the
    same-chain mask is a product of chain ids (:279) and the structure-context mask never reaches the output (:292-301)."""

    def __init__(self, max_n_atoms_per_residue, d_feat, max_dist_to_consider=32):
        super().__init__()
        self.d_feat = d_feat
        self.max_dist_to_consider = max_dist_to_consider
        self.max_n_atoms_per_residue = max_n_atoms_per_residue
        self.max_n_aa_types = 21
        self.aa_pair_type_embedding = nn.Embedding(self.max_n_aa_types**2, d_feat)
        self.relpos_embedding = nn.Embedding(2 * max_dist_to_consider + 1, d_feat)
        self.pair2distcoef = nn.Embedding(self.max_n_aa_types**2, max_n_atoms_per_residue**2)
        nn.init.zeros_(self.pair2distcoef.weight)
        self.distance_embedding = nn.Sequential(nn.Linear(max_n_atoms_per_residue**2, d_feat), nn.ReLU(), nn.Linear(d_feat, d_feat),
                                                nn.ReLU())
        self.mlp = nn.Sequential(nn.Linear(3 * d_feat + 2 * (2 * 2 * 2 + 1), d_feat), nn.ReLU(), nn.Linear(d_feat, d_feat), nn.ReLU(),
                                 nn.Linear(d_feat, d_feat))

    def forward(self, seq_idx, distmat, dihedrals, residue_idx, chain_idx, atom_mask, structure_context_mask, sequence_context_mask, *,
                xyz=None):
        """distmat (B,K,K,A,A) as in the reference; or distmat=None and xyz=(B,K,A,3): the atom-atom distances are then computed
        inside the kernel and the 14.7 MB/patch tensor is never built."""
        lib = _hip.lib()
        if distmat is None and xyz is None:
            raise ValueError("PairEmbedding.forward needs distmat or xyz")
        from_xyz = distmat is None
        out_dev = (xyz if from_xyz else distmat).device
        seq, ch, ri = _hip.dev_i64(seq_idx), _hip.dev_i64(chain_idx), _hip.dev_i64(residue_idx)
        dm, dh, am = (_hip.dev_f32(a) for a in (xyz if from_xyz else distmat, dihedrals, atom_mask))
        qm = _opt_mask(sequence_context_mask)
        B, K = seq.shape
        A = self.max_n_atoms_per_residue
        dims = _hip.CtxDims(B, K, A, 1, self.d_feat, self.max_dist_to_consider)
        p = _named(self)
        if ri.shape[0] not in (1, B):
            raise ValueError("residue_idx must be (1, K) or (B, K)")
        # (the grad mode is read HERE: inside an autograd Function's forward it is always off, and needs_input_grad ignores it)
        self._tape_wanted = torch.is_grad_enabled()
        out = _PairEmbeddingFn.apply(self, dims, from_xyz, seq, dm, dh, ri, K if ri.shape[0] == B else 0, ch, am, qm,
                                     *[p[k] for k in _PAIR_KEYS])
        return out.to(out_dev)


class DiffAb(_ModuleBase):
    """Drop-in for ``diffab_pytorch.DiffAb`` on the diffusion hot path (reference diffab_pytorch.py:628-931).

    Any model dims run; the benchmark dims take the MFMA kernels, every other geometry the any-dims kernels.  The forward (denoise,
    sample, score) reaches n_head * K of about 40 000; training (a backward) needs about three times the attention's LDS and stops at
    n_head * K of about 13 500 (at most 16 IPA layers).  Past that the taped forward raises DiffabHipError before anything runs."""

    def __init__(self, d_residue_emb, d_pair_emb, n_ipa_layers, d_scalar_per_head, n_query_point_per_head, n_value_point_per_head, n_head,
                 T=100, s=0.01, beta_max=0.999, n_atoms=15, aa_vocab_size=21, max_dist_to_consider=32, lr=1e-4, weight_decay=0.0,
                 betas=(0.9, 0.999), *, igso3_without_replacement: bool = True):
        """The reference's constructor (diffab_pytorch.py:629-660).  `igso3_without_replacement` (keyword-only, build-defined switch, default =
        the reference's behaviour): the forward orientation noise draws a patch's K histogram bins without replacement, as
        torch.multinomial does at so3.py:78; False selects independent inverse-CDF draws (what the build-defined reverse sampler uses)."""
        super().__init__()
        self.sched = cosine_variance_schedule(T=T, s=s, beta_max=beta_max)
        self.residue_context_embedding = ResidueEmbedding(n_atoms, d_residue_emb)
        self.pair_context_embedding = PairEmbedding(n_atoms, d_pair_emb, max_dist_to_consider)
        self.denoiser = Denoiser(d_residue_emb, d_pair_emb, n_ipa_layers, d_scalar_per_head, n_query_point_per_head, n_value_point_per_head,
                                 n_head, aa_vocab_size)
        self.seq_diffuser = SequenceDiffuser(T, s, beta_max, aa_vocab_size)
        self.coordinate_diffuser = CoordinateDiffuser(T, s, beta_max)
        self.orientation_diffuser = OrientationDiffuser(T, s, beta_max, igso3_without_replacement=igso3_without_replacement)
        self.aa_loss = nn.KLDivLoss(reduction="none")
        self.coordinate_loss = nn.MSELoss(reduction="none")
        self.orientation_loss = OrientationLoss(reduction="none")
        self.T = T
        self.beta_max = beta_max  # the schedule's clip, which the jump coefficients of a respaced sample() reuse
        self.lr = lr
        self.weight_decay = weight_decay
        self.betas = betas
        self._sched_dev: Optional[_hip.SchedOnDevice] = None
        self._rev_so3: Optional[_so3.SO3] = None
        self._rev_so3_steps: Dict[tuple, _so3.SO3] = {}  # (executed steps, t_stop) -> the reverse table over sqrt(beta')
        self._rev_so3_tempered: Dict[tuple, _so3.SO3] = {}  # (rotation scales, step list) -> the stacked reverse table

    # ------------------------------------------------------------------ device-side tables
    def _sched_on_device(self) -> _hip.SchedOnDevice:
        if self._sched_dev is None or self._sched_dev.tensors["beta"].device != _hip.device():
            self._sched_dev = _hip.SchedOnDevice(self.sched)
        return self._sched_dev

    def _reverse_so3(self) -> _so3.SO3:
        """IGSO3 table over sigma_t = sqrt(beta_t) for the reverse step (build-defined)."""
        if self._rev_so3 is None or self._rev_so3.histograms.device != _hip.device():
            # (the device sampler of the reverse loop draws by inverse CDF: one table lookup per residue inside reverse_update)
            self._rev_so3 = _so3.SO3(self.sched["beta"].sqrt(), sigma_threshold=0.1, n_bins=8192, num_iters=1024, without_replacement=False)
        return self._rev_so3

    def _reverse_so3_steps(self, steps: torch.Tensor, t_stop: int, beta_jump: torch.Tensor) -> _so3.SO3:
        """Reverse IGSO3 table of a respaced run: row t over sigma_t = sqrt(beta'_t), built like _reverse_so3 (each row depends on its
        own sigma alone, so the rows at stride-1 steps are bitwise _reverse_so3's; a run that lists every step uses that table)."""
        if torch.equal(beta_jump, self.sched["beta"]):
            return self._reverse_so3()
        key = (tuple(steps.tolist()), int(t_stop))
        tab = self._rev_so3_steps.get(key)
        if tab is None or tab.histograms.device != _hip.device():
            if len(self._rev_so3_steps) >= 8:  # a few step lists in use at once; 64 MiB of tables per list
                self._rev_so3_steps.pop(next(iter(self._rev_so3_steps)))
            tab = _so3.SO3(beta_jump.sqrt(), sigma_threshold=0.1, n_bins=8192, num_iters=1024, without_replacement=False)
            self._rev_so3_steps[key] = tab
        return tab

    def _reverse_so3_tempered(self, scales: Tuple[float, ...], steps: Optional[torch.Tensor], t_stop: int,
                              beta_jump: Optional[torch.Tensor]) -> _so3.SO3:
        """Stacked reverse IGSO3 table of a call with rotation scales: one SO3 over the concatenated sigma lists
        lambda_k sqrt(beta'), T + 1 entries each, row (k, t) at k (T + 1) + t; beta' is the schedule's beta, or the plan's with steps=.
        Each row depends on its own sigma alone, so a row is bitwise the same whatever else is stacked, and the lambda = 1 rows are
        _reverse_so3's (_reverse_so3_steps' in a respaced run).  Cached per (scales, step list): at most 4 stacks, the oldest dropped
        first; a stack is 2 fp32 planes of n_bins = 8192 per row (64 KiB), i.e. 6.3 MiB per scale at T = 100 and 101 MiB at the
        16-scale limit, so the cache holds at most ~404 MiB of device memory."""
        key = (tuple(scales), None if steps is None else (tuple(steps.tolist()), int(t_stop)))
        tab = self._rev_so3_tempered.get(key)
        if tab is None or tab.histograms.device != _hip.device():
            if len(self._rev_so3_tempered) >= 4:
                self._rev_so3_tempered.pop(next(iter(self._rev_so3_tempered)))
            base = (self.sched["beta"] if beta_jump is None else beta_jump).sqrt()
            tab = _so3.SO3(_temperature.stacked_sigmas(base, tuple(scales)), sigma_threshold=0.1, n_bins=8192, num_iters=1024,
                           without_replacement=False)
            self._rev_so3_tempered[key] = tab
        return tab

    # ------------------------------------------------------------------ reference API
    def encode_context(self, seq_idx_t0, xyz_t0, orientations_t0, backbone_dihedrals, distmat, pairwise_dihedrals, atom_mask, chain_idx,
                       residue_idx, generation_mask, residue_mask, generate_structure: bool = True, generate_sequence: bool = True):
        """Residue and pair context embeddings of the non-generated residues (reference diffab_pytorch.py:680-724)."""
        context_mask = residue_mask.bool() & (~generation_mask.bool())
        structure_context_mask = context_mask if generate_structure else None
        sequence_context_mask = context_mask if generate_sequence else None
        res_context_emb = self.residue_context_embedding(seq_idx_t0, xyz_t0, orientations_t0, backbone_dihedrals, chain_idx, atom_mask,
                                                         structure_context_mask, sequence_context_mask)
        # distmat=None: distances come from xyz_t0 inside the kernel (the reference's batches do not carry distmat, data.py:93-94)
        pair_context_emb = self.pair_context_embedding(seq_idx_t0, distmat, pairwise_dihedrals, residue_idx, chain_idx, atom_mask,
                                                       structure_context_mask, sequence_context_mask,
                                                       xyz=xyz_t0 if distmat is None else None)
        return res_context_emb, pair_context_emb

    def denoise(self, seq_idx_t, translations_t, orientations_t, res_context_emb, pair_context_emb, beta, generation_mask, residue_mask
                ) -> Dict[str, torch.Tensor]:
        """seq_posterior, translations_eps, orientations_t0 for a noisy state (diffab_pytorch.py:726-768)."""
        return self.denoiser(seq_idx_t, translations_t, orientations_t, res_context_emb, pair_context_emb, beta, generation_mask,
                             residue_mask)

    def _add_noise(self, seq_idx_t0, translations_t0, orientations_t0, generation_mask, t) -> Dict[str, torch.Tensor]:
        """Forward-noise all three modalities to timestep t (diffab_pytorch.py:778-806)."""
        seq_idx_t, seq_posterior = self.seq_diffuser.diffuse_from_t0(seq_idx_t0, t, generation_mask, return_posterior=True)
        translations_t, translations_eps = self.coordinate_diffuser.diffuse_from_t0(translations_t0, t, generation_mask, return_eps=True)
        orientations_t = self.orientation_diffuser.diffuse_from_t0(orientations_t0, generation_mask, t)
        return {"seq_idx_t": seq_idx_t, "seq_posterior": seq_posterior, "translations_t": translations_t,
                "translations_eps": translations_eps, "orientations_t": orientations_t}

    def hotpath_losses(self, denoised, noised, orientations_t0, generation_mask, residue_mask):
        """(seq KL, translation MSE, orientation) each over masked residues / #masked residues (diffab_pytorch.py:856-880)."""
        lib = _hip.lib()
        pp, tp = _hip.dev_f32(denoised["seq_posterior"]), _hip.dev_f32(noised["seq_posterior"])
        pe, te = _hip.dev_f32(denoised["translations_eps"]), _hip.dev_f32(noised["translations_eps"])
        pO, tO = _hip.dev_f32(denoised["orientations_t0"]), _hip.dev_f32(orientations_t0)
        gm, rm = _hip.dev_mask(generation_mask), _hip.dev_mask(residue_mask)
        B, K, V = pp.shape
        out = torch.empty(3, dtype=torch.float32, device=pp.device)
        _hip.check(lib.diffab_losses_fwd(_hip.ptr(pp), _hip.ptr(tp), _hip.ptr(pe), _hip.ptr(te), _hip.ptr(pO), _hip.ptr(tO), _hip.ptr(gm),
                                         _hip.ptr(rm), B, K, V, _hip.ptr(out), _hip.stream_ptr()), "diffab_losses_fwd")
        return out[0], out[1], out[2]

    def hotpath_train_losses(self, noised, res_context_emb, pair_context_emb, beta, orientations_t0, generation_mask, residue_mask):
        """Differentiable (seq, translation, orientation) losses of a noised batch: denoise + losses in one taped HIP forward,
        gradients for the denoiser parameters and both contexts in one HIP backward (reference :843-880 under autograd)."""
        params = [p for _, p in self.denoiser.named_parameters()]
        losses, *_ = _HotpathTrainStep.apply(self.denoiser, noised["seq_idx_t"], noised["translations_t"], noised["orientations_t"], beta,
                                             noised["seq_posterior"], noised["translations_eps"], orientations_t0, generation_mask,
                                             residue_mask, res_context_emb, pair_context_emb, *params)
        out_dev = noised["translations_t"].device
        return losses[0].to(out_dev), losses[1].to(out_dev), losses[2].to(out_dev)

    def _shared_step(self, batch, batch_idx):
        """t ~ U[1,T]; noise; denoise; three losses (diffab_pytorch.py:808-880).  The contexts come from encode_context on
        the reference's batch dict, or from batch['res_context_emb'] / batch['pair_context_emb'] when a caller
        has them already (the hot-path benchmarks and gradient goldens, where contexts are leaf inputs)."""
        dev_in = batch["generation_mask"].device
        bsz = batch["generation_mask"].size(0)
        t_host = torch.randint(low=1, high=self.T + 1, size=(bsz,))  # CPU generator, as the reference (:813); the schedule lookup stays on
        beta = self.sched["beta"][t_host].to(dev_in)                  # the host: no device -> host copy (a stream drain) per step
        t = t_host.to(dev_in)
        xyz_t0 = batch["xyz"]
        if "orientations" not in batch and xyz_t0.dim() == 4:  # frames from the backbone atoms
            batch = dict(batch, **_features.featurize(xyz_t0, orientations=True, backbone_dihedrals=False, pairwise_dihedrals=False))
        translations_t0 = xyz_t0[:, :, CA_IDX] if xyz_t0.dim() == 4 else xyz_t0
        noised = self._add_noise(batch["seq_idx"], translations_t0, batch["orientations"], batch["generation_mask"], t)
        if "res_context_emb" in batch and "pair_context_emb" in batch:
            res_ctx, pair_ctx = batch["res_context_emb"], batch["pair_context_emb"]
        else:
            if "backbone_dihedrals" not in batch or "pairwise_dihedrals" not in batch:  # from xyz, on the device
                batch = dict(batch, **_features.featurize(xyz_t0, batch["chain_idx"], batch["residue_mask"], orientations=False,
                                                          backbone_dihedrals="backbone_dihedrals" not in batch,
                                                          pairwise_dihedrals="pairwise_dihedrals" not in batch))
            res_ctx, pair_ctx = self.encode_context(batch["seq_idx"], xyz_t0, batch["orientations"], batch["backbone_dihedrals"],
                                                    batch.get("distmat"), batch["pairwise_dihedrals"], batch["atom_mask"], batch["chain_idx"],
                                                    batch["residue_idx"], batch["generation_mask"], batch["residue_mask"])
        if torch.is_grad_enabled():
            return self.hotpath_train_losses(noised, res_ctx, pair_ctx, beta, batch["orientations"], batch["generation_mask"],
                                             batch["residue_mask"])
        denoised = self.denoise(noised["seq_idx_t"], noised["translations_t"], noised["orientations_t"], res_ctx, pair_ctx, beta,
                                batch["generation_mask"], batch["residue_mask"])
        return self.hotpath_losses(denoised, noised, batch["orientations"], batch["generation_mask"], batch["residue_mask"])

    def training_step(self, batch, batch_idx):
        seq_loss, translations_loss, orientations_loss = self._shared_step(batch, batch_idx)
        loss = seq_loss + translations_loss + orientations_loss
        self.log_dict({"train/seq_loss": seq_loss, "train/translations_loss": translations_loss,
                       "train/orientations_loss": orientations_loss, "train/loss": loss}, on_step=True, on_epoch=True, prog_bar=True,
                      logger=True)
        return loss

    @torch.no_grad()
    def validation_step(self, batch, batch_idx):
        seq_loss, translations_loss, orientations_loss = self._shared_step(batch, batch_idx)
        loss = seq_loss + translations_loss + orientations_loss
        self.log_dict({"val/seq_loss": seq_loss, "val/translations_loss": translations_loss, "val/orientations_loss": orientations_loss,
                       "val/loss": loss}, on_step=False, on_epoch=True, prog_bar=False, logger=True)
        return loss

    def gradient_buckets(self):
        """The flat fp32 buffers the last HIP backward wrote the parameter gradients into (denoiser, residue encoder, pair encoder):
        after zero_grad(set_to_none=True) + backward every p.grad is a view of one of them.  distributed.allreduce_gradients
        reduces them in place."""
        return [getattr(m, "_flat_grad", None) for m in (self.denoiser, self.residue_context_embedding, self.pair_context_embedding)]

    def configure_optimizers(self):
        # reference :925-931: Adam with these hyper-parameters.  On the device the update runs as torch's fused kernel (one launch over
        # all parameters instead of ~8 multi-tensor launches per step: 0.17 -> 0.03 ms of a 7.6 ms step); same update rule.
        params = list(self.parameters())
        fused = bool(params) and all(p.is_cuda and p.is_floating_point() for p in params)
        return torch.optim.Adam(params, lr=self.lr, weight_decay=self.weight_decay, betas=self.betas, fused=fused)

    def _contexts_from_batch(self, seq_idx, xyz, orientations, generation_mask, residue_mask, backbone_dihedrals, pairwise_dihedrals,
                             distmat, atom_mask, chain_idx, residue_idx, generate_structure, generate_sequence):
        """encode_context from the reference's batch fields as sample() and score() accept them: residue_idx and
        residue_mask default to arange(K) and all-true; the dihedral features are taken from xyz on the device when absent."""
        Bq, Kq = seq_idx.shape
        if residue_mask is None:
            residue_mask = torch.ones(Bq, Kq, dtype=torch.bool, device=seq_idx.device)
        if backbone_dihedrals is None or pairwise_dihedrals is None:  # dihedral features from the coordinates, on the device
            feats = _features.featurize(xyz, chain_idx, residue_mask, orientations=False, backbone_dihedrals=backbone_dihedrals is None,
                                        pairwise_dihedrals=pairwise_dihedrals is None)
            backbone_dihedrals = feats.get("backbone_dihedrals", backbone_dihedrals)
            pairwise_dihedrals = feats.get("pairwise_dihedrals", pairwise_dihedrals)
        if residue_idx is None:
            residue_idx = torch.arange(Kq, device=seq_idx.device).unsqueeze(0)  # data.py:91
        return self.encode_context(seq_idx, xyz, orientations, backbone_dihedrals, distmat, pairwise_dihedrals, atom_mask, chain_idx,
                                   residue_idx, generation_mask, residue_mask, generate_structure, generate_sequence)

    # ------------------------------------------------------------------ reverse process (the reference has a stub, :770-776)
    @torch.no_grad()
    def sample(self, seq_idx: torch.LongTensor, xyz: torch.FloatTensor, orientations: torch.FloatTensor, *, generation_mask=None,
               res_context_emb=None, pair_context_emb=None, residue_mask=None, backbone_dihedrals=None, pairwise_dihedrals=None,
               distmat=None, atom_mask=None, chain_idx=None, residue_idx=None, generate_structure: bool = True,
               generate_sequence: bool = True, seed: Optional[int] = None, first_patch: int = 0, t_start: Optional[int] = None,
               t_stop: int = 0, init: bool = True, flags: int = 0, graph: Optional[bool] = None,
               skip_unused_rows: bool = True, num_samples: int = 1,
               context_index: Optional[torch.LongTensor] = None, mode: Optional[str] = None,
               optimize_from: Optional[int] = None, allowed_aa: Optional[torch.Tensor] = None, trajectory=None,
               trajectory_predictions: bool = False, steps=None,
               guidance: Optional[_guidance.SampleGuidance] = None,
               temperature: Optional[_temperature.SampleTemperature] = None,
               steering: Optional[_steering.ParticleSteering] = None) -> Dict[str, torch.Tensor]:
        """Reverse diffusion t_start .. t_stop+1 (default T .. 1) on the generated residues (the reference's `sample` is a stub,
        diffab_pytorch.py:770-776; the loop is build-defined).

        seq_idx (B,K), xyz (B,K,3) CA translations or (B,K,A,3) atoms, orientations (B,K,3,3): the ground-truth
        context; generated residues are re-initialised (x ~ N(0,I), O ~ U(SO3), s ~ U{0..19}) when ``init``.
        Contexts: pass ``res_context_emb`` / ``pair_context_emb``, or the remaining fields of the reference's batch dict
        (SURVEY B.2): atom_mask and chain_idx; residue_idx and residue_mask default to arange(K) and all-true; distmat and the two
        dihedral features are taken from xyz on the device when absent (features.featurize) - and `encode_context` runs first, once.
        Noise is Philox keyed by (seed, first_patch + b, residue, t): any sharding of a batch over ranks gives
        the same samples.  All T steps are enqueued on the current stream by ONE C-ABI call, no host sync.
        ``graph=True``: replay one captured step as a hipGraph instead of ~45 launches per step (same kernels, bitwise the same
        result; the call then waits for the trajectory).  Off by default: measured at BASELINE config 1 (B = 1, K = 128, 100 steps)
        it changes nothing - 145 ms eager, 146 ms replayed - because the host already runs ahead of the device there; a step is a
        chain of ~45 dependent kernels on 8-work-group grids (1.45 ms), not 45 launch overheads.
        ``skip_unused_rows`` (default True): a step's outputs are used for generated residues only, so the LAST layer's attention runs only
        for the 16-row tiles that contain one - on both launch forms of the loop, bitwise the same samples, less work when few residues
        are generated (one CDR: 5-7 of the 8 row tiles of the last layer are skipped; a fully generated patch loses nothing).  ``False``
        sets `DIFFAB_FLAG_ALL_ROWS`: every tile runs, the form to time the full layer with.

        Many designs per patch from one shared context:
        ``num_samples=N``: every per-patch input (seq_idx, xyz, orientations, generation_mask; B rows) is replicated N times on the
        device and the result has B*N rows, row b*N + r being design r of patch b.  The contexts stay B rows - given, or computed by ONE
        encode_context call over the B patches - and the sampler reads them through a row -> context map
        (`diffab_sample_loop_ex`, option `ctx_of_row`): no (B*N, K, K, C) copy of the pair context and no per-replica fp16 planes.  Bitwise the result
        of num_samples=1 on the repeat_interleave(N, dim=0) of every per-patch input with the same seed and first_patch (the replicas
        differ by their noise keys, patch id first_patch + b*N + r).
        ``context_index`` (R,) is the general form: res_context_emb / pair_context_emb hold n_ctx contexts (required), the state
        inputs have R rows and row i is denoised against context context_index[i].  A rank that owns output rows [lo, hi) of a
        num_samples run passes the state rows lo..hi-1, context_index = arange(lo, hi) // N and first_patch = lo.
        Both together, num_samples < 1, lengths that do not match and indices outside [0, n_ctx) raise ValueError before any
        device work.

        Design modes (Luo et al.'s three tasks; every mode combines with num_samples, context_index, graph and the launch flags):
        ``mode=None`` is the behaviour above (generate_structure / generate_sequence as given, all three modalities diffused);
        ``"codesign"`` is the same with both flags true (bitwise mode=None); ``"fixed_backbone"`` encodes the context with the generated
        residues' structure visible (encode_context(generate_structure=False)) and diffuses only the sequence - x and O of the generated
        residues are returned exactly as given (`DIFFAB_FLAG_KEEP_STRUCTURE`); ``"structure"`` encodes it with their sequence visible
        and diffuses only x and O - seq is returned as given (`DIFFAB_FLAG_KEEP_SEQUENCE`).  The diffused modality sees the same Philox
        draws as in co-design.  A mode sets generate_structure / generate_sequence itself: giving either as False with a mode raises.
        ``optimize_from=t`` (antibody optimisation): the given state of the generated residues is the native; it is forward-noised to
        step t on the device (`diffab_sample_init_noised`, Philox keyed like the loop, so sharding and num_samples behave as above)
        instead of re-initialised, and the loop runs t .. t_stop+1 (a few steps instead of T).  The kept modality of a mode is not
        noised.  An unknown mode, a mode with generate_structure / generate_sequence False, optimize_from outside [1, T], optimize_from
        with init=False and a t_start other than optimize_from raise ValueError before any device work.

        Sequence constraints: ``allowed_aa`` is a bool tensor (V,), (K, V) or (rows, K, V) - True where class v (io.AA3 order, UNK last)
        may appear - broadcast to the input rows (io.allowed_aa_mask builds one from one-letter codes).  Every sequence draw of a
        generated residue is restricted to its allowed classes on the device (`diffab_sample_loop_ex`, option `allowed`, and `allowed` of the init entries): the
        reverse step draws from the posterior renormalised over them, the initial state uniformly over them (UNK only when it is the
        only one), optimize_from's start from q(s_t | s_0) renormalised over them.  The Philox lanes are the unconstrained ones, so an
        all-True mask is bitwise the unconstrained run and sharding / num_samples / context_index behave as above; with num_samples the
        rows are per patch and replicated like generation_mask, with context_index they are per state row.  Combines with
        "codesign" / "fixed_backbone" (constrained inverse folding), optimize_from, graph and the launch flags.  A dtype other than bool,
        a shape that does not broadcast, a last dimension other than the model's V (or V > 32), a generated residue with no allowed
        class and mode="structure" (the sequence is not diffused) raise ValueError before any device work.

        Trajectory: ``trajectory=True`` records every step, an int k >= 1 the steps t_start, t_start - k, ... down to t_stop + 1, a 1-D
        int list / tensor the distinct steps it names in [t_stop + 1, t_start]; the result gains ``"trajectory"``, a dict on the input's
        device.  Labels are steps: ``t`` (n,) int64 in descending order, and slot j of every field holds label t[j]:
        ``seq_idx`` (rows, n, K), ``translations`` (rows, n, K, 3), ``orientations`` (rows, n, K, 3, 3) - the state that step t denoises,
        bitwise the result of this call with t_stop = t (same seed, first_patch, mode, optimize_from, allowed_aa, num_samples /
        context_index, flags and graph); label t_start is the initial state.  The final state is the ordinary return value and is not
        repeated.  ``trajectory_predictions=True`` adds what the denoiser made of that state: ``pred_translations`` x0_hat = (x_t -
        sqrt(1 - alpha_bar_t) eps_hat) / sqrt(alpha_bar_t), ``pred_orientations`` O0_hat, and ``seq_probs`` (rows, n, K, V), the
        softmax posterior over s_{t-1} - unrestricted: under allowed_aa the draw renormalises it over the allowed set; label 1 is the
        distribution the returned token was drawn from.  Residues that are not generated hold their given state in every slot, and
        their predictions are their x / O and a one-hot of their token; a kept modality of a mode appears in the predictions as its
        given values.  Rows are outermost (row b*N + r under num_samples), so a shard's rows are that slice of the whole call's
        trajectory.  The update kernel writes the record on the device (`diffab_sample_loop_ex`, option `record`); the returned state is bitwise the
        same with and without a trajectory, on every launch form.  Memory: 56 B of state plus 132 B of predictions (V = 21) per
        recorded residue and label - every step of a 100-step run at 256 x 128 is about 590 MiB.  A bool / float / 2-D / empty
        trajectory, a stride < 1, a step outside the range or named twice, and trajectory_predictions without trajectory raise
        ValueError before any device work.

        Fewer-step sampling (DDPM respacing): ``steps=n`` runs n evenly spaced steps tau_j = t_start -
        round_half_up(j (L - 1) / (n - 1)), L = t_start - t_stop (every step when n = L); a 1-D int list / tensor names them itself,
        strictly descending from t_start (optimize_from's step with optimize_from) and above t_stop.  Step tau_j evaluates the denoiser
        at tau_j exactly as the full loop does and moves the state to tau_{j+1} (t_stop after the last) with the jump's coefficients
        beta'_t = clip(1 - abar_t / abar_s, 1e-5, beta_max): translations and orientations by the DDPM update with beta', the sequence
        from sum_u p(s_0 = u | s_t) q(s_s | s_t, u), the x0 mixture recovered from the head posterior on the device in double
        (`diffab_sample_loop_ex`, option `steps`).  Noise stays keyed by (seed, first_patch + b, residue, tau_j), so sharding, num_samples and
        context_index behave as above; it combines with every mode, optimize_from, allowed_aa, graph, skip_unused_rows and the flags.
        Listing every step is bitwise ``steps=None``, and a mixed list is bitwise the full run up to its last stride-1 step.  With a
        trajectory, labels are executed steps: True records every executed step, an int k every k-th of them, and a list must name
        executed steps; ``seq_probs`` is still the head posterior.  None is the ordinary loop.  A bool / float / 2-D / empty list,
        n outside [1, L], a list that does not start at t_start, is not strictly descending or reaches t_stop, and t_start = t_stop
        raise ValueError before any device work.

        Structure guidance: ``guidance=guidance.SampleGuidance(clash=..., bond=...)`` steers the CA translations
        of the generated residues away from clashes and towards chain bonds while they form.  Per state row, over the pairs with
        residue_mask on both and at least one generated residue, at p = x0_hat (the pred_translations of a trajectory record; the given
        x for residues that are not generated): U = clash sum_nonbonded max(0, clash_distance - d)^2 + bond sum_bonded (d -
        bond_length)^2, bonded meaning the same chain_idx and residue_idx one apart.  At every step t <= t_max (None: all) the mean of
        the update loses Delta = beta'_t dU/dp (beta[t], or the jump's beta' with steps=), capped at length max_shift, before the noise
        is added; the last step is guided too.  Orientations, the sequence, the Philox draws and the trajectory record are unchanged.
        The tables are ``chain_idx`` (default one chain), ``residue_idx`` (default arange(K)) and ``residue_mask`` (default all true),
        (K,) or (rows, K), used even when the contexts are given: per patch and replicated like generation_mask under num_samples, per
        state row with context_index.  Both weights 0 (and t_max = 0) still run the guidance kernel and are bitwise the unguided
        sample (`diffab_sample_loop_ex`, option `guidance`).  Combines with every mode except "fixed_backbone" (the structure is kept), with
        optimize_from, allowed_aa, trajectory, steps, graph, skip_unused_rows, num_samples / context_index and the flags.  Anything but
        a SampleGuidance, a negative or non-finite weight, a non-positive distance or max_shift, t_max outside [0, T], tables of a
        non-integer dtype or a shape that does not broadcast to the rows, and mode="fixed_backbone" raise ValueError before any device
        work.  guidance.structure_energy counts clashes and bond deviations of finished designs.

        Noise scales and sequence temperature: ``temperature=temperature.SampleTemperature(translation=...,
        rotation=..., sequence=...)`` sets how greedy every reverse step is.  Each field is a number or a 1-D tensor with one entry per
        output row (B * num_samples rows, row b * N + r; per state row with context_index), finite and >= 0, default 1.  The translation
        noise is lambda_x sqrt(beta'_t) z (0: the mean, exactly); the IGSO3 angle is drawn at sigma = lambda_O sqrt(beta'_t) from a
        table row built over that sigma with the same uniforms, normal and axis (0: O = O0_hat, exactly); s_{t-1} is drawn from
        p^(1/tau) renormalised over the allowed classes, p the head posterior or a respaced step's jump distribution (tau = 0: the
        argmax, lowest index on ties).  All three are applied by the update kernel (`diffab_sample_loop_ex`, option `temperature`), so they combine with
        every mode that samples the modality, optimize_from, allowed_aa, trajectory, steps, guidance, graph, num_samples /
        context_index and the flags; 1 everywhere is bitwise the untempered sample, and with init=False and every value 0 the result
        does not depend on the seed.  Not changed: the posterior, x0_hat / O0_hat and with them the trajectory record, the initial
        state, optimize_from's forward noise, and DiffAb.score.  A rank that owns output rows [lo, hi) passes those rows' values and
        first_patch = lo.  The stacked IGSO3 table of the call's distinct nonzero rotation scales is built once and cached
        (_reverse_so3_tempered).  Anything but a SampleTemperature, a shape that does not broadcast, a negative, NaN or infinite value,
        more than 16 distinct nonzero rotation scales, a structure scale != 1 with mode="fixed_backbone" and a sequence temperature
        != 1 with mode="structure" raise ValueError before any device work.

        Particle steering: ``steering=steering.ParticleSteering(strength=..., ess_threshold=...)`` spends the
        designs of a patch where they pay off.  The state rows are groups of ``group_size`` consecutive rows (default num_samples: the
        designs of one patch).  At every steering step - the executed steps t in [t_min, t_max] with (t_max - t) % every == 0, the last
        executed step excepted; t_max None: the first step of the call - each row is weighed by the guidance potential U (clash, bond,
        clash_distance, bond_length as in SampleGuidance; chain_idx / residue_idx / residue_mask as for guidance) at x0_hat of that step:
        log w += -strength (U - U at the previous steering step).  When the effective sample size (sum w)^2 / sum w^2 of a group falls
        below ess_threshold * group_size the group is resampled systematically with one Philox uniform, keyed by the group's first
        global row, and after the step's ordinary update the generated residues (seq, x, O) of every row are replaced by those of its
        ancestor; the copies separate again at the next step through their own noise.  No gradient, no extra model evaluation, the mean
        of no step moves; weights never reach the host, so it runs under graph replay and on every launch form
        (`diffab_sample_loop_ex`, option `steering`).  The result gains ``"steering"``: ``log_weight`` (rows,) and ``energy`` (rows,) - the energy
        each weight has seen last, its ancestor's after a resampling - ``t`` (n,) the steering steps in descending order, ``ancestors``
        (n, rows) the global row each row was copied from at that step (its own index where nothing moved) and ``lineage`` (rows,), the
        initial row every design descends from.  All rows of a group must share generation_mask, the context and the tables (checked on
        the host before device work, which copies generation_mask to it once per call).
        strength = 0 (ess_threshold <= 1), ess_threshold = 0 and group_size = 1 are bitwise the unsteered sample.  Combines with the
        modes that sample the structure, optimize_from, allowed_aa, trajectory (the record of step t is written before the gather),
        steps, guidance, temperature, graph, num_samples / context_index and the flags.  A rank passes whole groups
        (distributed.shard_range(..., group_size=N)) and first_patch = its first row: bitwise the slice of the whole call.  Anything
        but a ParticleSteering, a negative or non-finite strength or weight, a non-positive distance, ess_threshold outside [0, 2],
        every < 1, t_min / t_max outside [0, T] or t_min > t_max, group_size outside [1, 1024], rows that are no whole groups, a group
        whose rows differ in generation_mask, context or tables, and mode="fixed_backbone" raise ValueError before any device work."""
        if generation_mask is None:
            raise ValueError("sample() needs generation_mask: which residues to generate")
        generate_structure, generate_sequence, keep = _mode_settings("sample()", mode, generate_structure, generate_sequence)
        if optimize_from is not None:
            if isinstance(optimize_from, bool) or not isinstance(optimize_from, int) or not 1 <= optimize_from <= self.T:
                raise ValueError(f"sample(): optimize_from must be an int in [1, T = {self.T}], got {optimize_from!r}")
            if not init:
                raise ValueError("sample(): optimize_from noises the given native state itself; it cannot be combined with init=False")
            if t_start is not None and int(t_start) != optimize_from:
                raise ValueError(f"sample(): t_start = {t_start} disagrees with optimize_from = {optimize_from} (the loop starts at "
                                 "optimize_from; leave t_start out)")
            t_start = optimize_from
        t_start, t_stop = self.T if t_start is None else int(t_start), int(t_stop)
        if isinstance(num_samples, bool) or not isinstance(num_samples, int) or num_samples < 1:
            raise ValueError(f"sample(): num_samples must be an int >= 1, got {num_samples!r}")
        if num_samples > 1 and context_index is not None:
            raise ValueError("sample(): give num_samples or context_index, not both (context_index is the general form)")
        n_rows, K_ = seq_idx.shape
        ctx_map = None  # host int32 (rows,): the context of every state row (None: one context per row)
        if num_samples > 1 or context_index is not None:
            for name, v in (("xyz", xyz), ("orientations", orientations), ("generation_mask", generation_mask)):
                if v.shape[0] != n_rows or v.shape[1] != K_:
                    raise ValueError(f"sample(): {name} is {tuple(v.shape)}, seq_idx is {(n_rows, K_)}")
            dd = self.denoiser.dims
            for name, v, tail in (("res_context_emb", res_context_emb, (K_, dd["D"])), ("pair_context_emb", pair_context_emb, (K_, K_, dd["C"]))):
                if v is not None and tuple(v.shape[1:]) != tail:
                    raise ValueError(f"sample(): {name} is {tuple(v.shape)}, expected (contexts, {', '.join(map(str, tail))})")
        if context_index is not None:
            ctx_map = _context_map("sample()", context_index, n_rows, res_context_emb, pair_context_emb, "state rows")
        elif num_samples > 1:
            for name, v in (("res_context_emb", res_context_emb), ("pair_context_emb", pair_context_emb)):
                if v is not None and v.shape[0] != n_rows:
                    raise ValueError(f"sample(): with num_samples the contexts are per patch: {name} has {v.shape[0]} rows, "
                                     f"seq_idx has {n_rows}")
            ctx_map = torch.arange(n_rows, dtype=torch.int32).repeat_interleave(num_samples)
        if allowed_aa is not None:
            _allowed_aa_host("sample()", allowed_aa, generation_mask, n_rows, K_, self.denoiser.dims["V"], keep)
        res_tabs = None  # host (rows, K) chain / residue_idx / residue_mask of the potential, for guidance and steering alike (None: neither)
        if guidance is not None:
            _guidance.check_guidance("sample()", guidance, self.T)
            if keep & _hip.FLAG_KEEP_STRUCTURE:
                raise ValueError("sample(): guidance moves the structure, which mode='fixed_backbone' keeps as given")
        if steering is not None:
            _steering.check_steering("sample()", steering, self.T)
            if keep & _hip.FLAG_KEEP_STRUCTURE:
                raise ValueError("sample(): steering weighs the sampled structure, which mode='fixed_backbone' keeps as given")
        if guidance is not None or steering is not None:
            res_tabs = _guidance.residue_tables("sample()", chain_idx, residue_idx, residue_mask, n_rows, K_)
        temp_vals = None  # host fp32 (output rows,) lambda_x, lambda_O, tau (None: untempered)
        if temperature is not None:
            temp_vals = _temperature.row_values("sample()", temperature, n_rows * num_samples)
            _temperature.check_mode("sample()", temp_vals, bool(keep & _hip.FLAG_KEEP_STRUCTURE), bool(keep & _hip.FLAG_KEEP_SEQUENCE))
        if steering is not None:  # steer_n: the group size; the groups are checked on the host (one copy of generation_mask to it)
            if steering.t_max is None and steering.t_min > t_start:
                raise ValueError(f"sample(): steering t_min = {steering.t_min} is above the first step of the call (t_max=None steers from it)")
            steer_n = num_samples if steering.group_size is None else steering.group_size
            per_row = lambda v: v.repeat_interleave(num_samples, dim=0) if num_samples > 1 else v
            gm_host = torch.as_tensor(generation_mask).detach().cpu().ne(0)
            _steering.check_groups("sample()", steer_n, n_rows * num_samples,
                                   {"generation_mask": per_row(gm_host), "the context (context_index)": ctx_map,
                                    "chain_idx": per_row(res_tabs[0]), "residue_idx": per_row(res_tabs[1]),
                                    "residue_mask": per_row(res_tabs[2])})
        executed = _sample_steps("sample()", steps, t_start, t_stop, self.T)
        labels = _trajectory_labels("sample()", trajectory, trajectory_predictions, t_start, t_stop, self.T, executed)
        if res_context_emb is None or pair_context_emb is None:
            _check_encode_fields("sample()", xyz, atom_mask, chain_idx)
            res_context_emb, pair_context_emb = self._contexts_from_batch(seq_idx, xyz, orientations, generation_mask, residue_mask,
                                                                          backbone_dihedrals, pairwise_dihedrals, distmat, atom_mask,
                                                                          chain_idx, residue_idx, generate_structure, generate_sequence)
        lib = _hip.lib()
        out_dev = seq_idx.device
        seq = _hip.dev_i64(seq_idx)
        x = _hip.dev_f32(xyz[:, :, CA_IDX] if xyz.dim() == 4 else xyz)
        O = _hip.dev_f32(orientations)
        rc, pc, gm = _hip.dev_f32(res_context_emb), _hip.dev_f32(pair_context_emb), _hip.dev_mask(generation_mask)
        allowed = None  # int32 (rows, K) words of the allowed classes (always passed when allowed_aa is given, an all-True mask too)
        if allowed_aa is not None:
            allowed = _pack_allowed_aa(torch.as_tensor(allowed_aa).detach().to(seq.device).expand(n_rows, K_, self.denoiser.dims["V"]))
        if res_tabs is not None:  # on the device once; guidance and steering read the same three tensors
            res_tabs = tuple(v.to(seq.device) for v in res_tabs)
        if num_samples > 1:  # the state of every design: the patch's rows, replicated on the device (the contexts are not)
            seq, x, O, gm = (v.repeat_interleave(num_samples, dim=0) for v in (seq, x, O, gm))
            if allowed is not None:
                allowed = allowed.repeat_interleave(num_samples, dim=0)
            if res_tabs is not None:
                res_tabs = tuple(v.repeat_interleave(num_samples, dim=0) for v in res_tabs)
        else:
            seq, x, O = seq.clone(), x.clone(), O.clone()
        B, K = seq.shape
        seed = _so3._draw_seed() if seed is None else int(seed)
        dims = self.denoiser.hip_dims(B, K)
        w = self.denoiser.hip_weights()
        sd = self._sched_on_device()
        if executed is None:
            tab = self._reverse_so3().struct()
        else:
            beta_j, alpha_j = jump_coefficients(self.sched, executed, t_stop, self.beta_max)
            rev_tab = self._reverse_so3_steps(executed, t_stop, beta_j)  # (held until the call has been enqueued)
            tab = rev_tab.struct()
        temp = None  # diffab_sample_temperature (None: every field 1 - untempered); its device tensors live in temp_dev
        if temp_vals is not None:
            lx, lo, tau = temp_vals
            temp_dev = [None if bool((v == 1).all()) else v.to(seq.device) for v in (lx, lo, tau)] + [None]
            if temp_dev[1] is not None:
                scales = _temperature.rotation_scales(lo)
                if scales:  # (every lambda_O = 0: the table is never read)
                    rev_tab = self._reverse_so3_tempered(scales, executed, t_stop, None if executed is None else beta_j)
                    tab = rev_tab.struct()
                temp_dev[3] = _temperature.rotation_rows(lo, scales, self.T).to(seq.device)
            if any(v is not None for v in temp_dev):
                temp = _hip.SampleTemperature(*(_hip.ptr(v) for v in temp_dev))
        opt = {}  # the fields of diffab_sample_options that are on (none: the plain loop)
        if ctx_map is None:
            ws = _hip.workspace(lib.diffab_sample_workspace_bytes(C.byref(dims)))
        else:
            n_ctx = rc.shape[0]
            ws = _hip.workspace(lib.diffab_sample_shared_workspace_bytes(C.byref(dims), n_ctx))
            opt.update(n_ctx=n_ctx, ctx_of_row=(C.c_int32 * B)(*ctx_map.tolist()))
        if graph:
            flags |= _hip.FLAG_GRAPH_SAMPLER
        if not skip_unused_rows:
            flags |= _hip.FLAG_ALL_ROWS
        flags |= keep
        state = (_hip.ptr(seq), _hip.ptr(x), _hip.ptr(O), _hip.ptr(gm), seed, first_patch, B, K)
        if init and optimize_from is not None:
            fwd_tab = self.orientation_diffuser.so3.struct()
            _hip.check(lib.diffab_sample_init_noised(C.byref(sd.struct), C.byref(fwd_tab), *state, optimize_from, keep, _hip.ptr(allowed),
                                                     _hip.stream_ptr()), "diffab_sample_init_noised")
        elif init and (keep or allowed is not None):
            _hip.check(lib.diffab_sample_init_ex(*state, self.T, keep, _hip.ptr(allowed), _hip.stream_ptr()), "diffab_sample_init_ex")
        elif init:
            _hip.check(lib.diffab_sample_init(*state, self.T, _hip.stream_ptr()), "diffab_sample_init")
        dev = seq.device
        if allowed is not None:
            opt["allowed"] = _hip.ptr(allowed)
        if labels is not None:
            opt["record"], traj, slot_dev = _record_c_struct(labels, self.T, B, K, self.denoiser.dims["V"], trajectory_predictions, dev)
        if executed is not None:
            plan_dev = torch.empty(3 * (self.T + 1), dtype=torch.int32, device=dev)
            opt["steps"] = _steps_c_struct(executed, beta_j, alpha_j, plan_dev)
        if guidance is not None:
            shift = torch.empty(B, K, 3, device=dev)
            opt["guidance"] = _guidance.c_struct(guidance, self.T if guidance.t_max is None else guidance.t_max, *res_tabs, shift)
        if temp is not None:
            opt["temperature"] = temp
        if steering is not None:
            logw, u_prev, energy = (torch.zeros(B, device=dev) for _ in range(3))
            anc = torch.empty(self.T + 1, B, dtype=torch.int32, device=dev)
            scratch = torch.empty(_steering.scratch_bytes(B, K), dtype=torch.uint8, device=dev)
            st_max = t_start if steering.t_max is None else steering.t_max
            opt["steering"] = _steering.c_struct(steering, st_max, steer_n, *res_tabs, logw, u_prev, energy, anc, scratch)
        options = _hip.SampleOptions(**opt)
        _hip.check(lib.diffab_sample_loop_ex(C.byref(dims), C.byref(w.struct), C.byref(sd.struct), C.byref(tab), _hip.ptr(seq), _hip.ptr(x),
                                             _hip.ptr(O), _hip.ptr(rc), _hip.ptr(pc), _hip.ptr(gm), seed, first_patch, t_start, t_stop,
                                             _hip.ptr(ws), ws.numel(), flags, C.byref(options) if opt else None, _hip.stream_ptr()),
                   "diffab_sample_loop_ex")
        out = {"seq_idx": seq.to(out_dev), "translations": x.to(out_dev), "orientations": O.to(out_dev)}
        if labels is not None:
            out["trajectory"] = {"t": labels.to(out_dev), **{k: v.to(out_dev) for k, v in traj.items()}}
        if steering is not None:
            ran = executed.tolist() if executed is not None else list(range(t_start, t_stop, -1))
            ts = torch.tensor(_steering.steering_steps(ran, t_stop, steering.t_min, st_max, steering.every), dtype=torch.int64)
            first = torch.arange(B, device=dev) // steer_n * steer_n  # group-local -> global row indices
            glob = anc[ts.to(dev)].to(torch.int64) + first
            out["steering"] = {"log_weight": logw.to(out_dev), "energy": u_prev.to(out_dev), "t": ts.to(out_dev),
                               "ancestors": glob.to(out_dev), "lineage": _steering.lineage(glob).to(out_dev)}
        return out

    # ------------------------------------------------------------------ from a whole complex (build-defined; the reference cuts patches in preprocess_pdb.py:44-58)
    @torch.no_grad()
    def design_complex(self, batch: Dict[str, torch.Tensor], *, k: int = 128, k_antigen: Optional[int] = None, pad_to: int = 128,
                       refine: Optional["_refine.Refinement"] = None, **sample_kwargs) -> Dict[str, torch.Tensor]:
        """Designs for whole complexes: ``batch`` holds the reference's batch fields for B complexes
        of N residues each - ``seq_idx``, ``xyz`` (B,N,A,3), ``generation_mask`` and, unless ``sample_kwargs`` brings the contexts,
        ``atom_mask`` and ``chain_idx``; optionally ``orientations`` (taken from xyz with features.featurize on the patch when absent),
        ``residue_mask``, ``residue_idx`` (default arange(N): the complex's numbering), ``antigen_mask``, ``anchor_mask``,
        ``backbone_dihedrals``, ``allowed_aa`` (B,N,V).  ``patch.select`` picks the K residues of each patch (k, k_antigen, pad_to as
        there), ``patch.gather`` brings every per-residue field to patch size, ``sample`` runs on the gathered fields - so the contexts
        are encoded once per complex, and ``num_samples`` and every other sampler option in ``sample_kwargs`` pass through untouched -
        and ``patch.paste`` writes the designs back.  Returns sample()'s dict (patch-sized rows) plus ``"patch"``, the PatchIndex, and
        ``"complex"``: full-length ``seq_idx`` (rows,N), ``translations``, ``orientations`` - the native complex with the generated
        residues replaced by the design.  Bitwise what the four calls give when made by hand.  The fields sample() takes from the
        batch cannot be given again in sample_kwargs (ValueError).  ``refine``: a ``refine.Refinement`` sends the patch designs through
        ``refine.backbone`` with the gathered patch's chain_idx / residue_idx / residue_mask before they are
        pasted - the returned frames and ``"complex"`` are the refined ones, and ``energy_before`` / ``energy_after`` / ``terms`` /
        ``max_shift`` are added; None (the default) leaves the call as it is without the argument."""
        if refine is not None and not isinstance(refine, _refine.Refinement):
            raise ValueError(f"design_complex(): refine must be a refine.Refinement or None, got {type(refine).__name__}")
        taken = ("generation_mask", "residue_mask", "atom_mask", "chain_idx", "residue_idx", "backbone_dihedrals", "pairwise_dihedrals",
                 "distmat")
        clash = [n for n in taken if n in sample_kwargs]
        if clash:
            raise ValueError(f"design_complex(): {clash} come from the batch, not from keyword arguments")
        if not isinstance(batch, dict) or batch.get("xyz") is None or batch.get("generation_mask") is None:
            raise ValueError("design_complex(): batch must be a dict with xyz and generation_mask (the reference's batch fields)")
        sel = _patch.select(batch["xyz"], batch["generation_mask"], k=k, k_antigen=k_antigen, antigen_mask=batch.get("antigen_mask"),
                            anchor_mask=batch.get("anchor_mask"), chain_idx=batch.get("chain_idx"), residue_mask=batch.get("residue_mask"),
                            pad_to=pad_to)
        g = _patch.gather(batch, sel)
        full = batch
        if g.get("orientations") is None:  # the frames of the patch and of the native complex, from the coordinates
            g["orientations"] = _features.featurize(g["xyz"], g.get("chain_idx"), g["residue_mask"], backbone_dihedrals=False,
                                                    pairwise_dihedrals=False)["orientations"]
            full = dict(batch, orientations=_features.featurize(batch["xyz"], batch.get("chain_idx"), batch.get("residue_mask"),
                                                                backbone_dihedrals=False, pairwise_dihedrals=False)["orientations"])
        if "allowed_aa" in g and "allowed_aa" not in sample_kwargs:
            sample_kwargs["allowed_aa"] = g["allowed_aa"]
        out = self.sample(g["seq_idx"], g["xyz"], g["orientations"], generation_mask=g["generation_mask"], residue_mask=g["residue_mask"],
                          atom_mask=g.get("atom_mask"), chain_idx=g.get("chain_idx"), residue_idx=g["residue_idx"],
                          backbone_dihedrals=g.get("backbone_dihedrals"), **sample_kwargs)
        if refine is not None:
            tabs = {n: g.get(n) for n in ("generation_mask", "chain_idx", "residue_idx", "residue_mask")}
            tabs.update({n: tabs[n].ne(0) for n in ("generation_mask", "residue_mask") if tabs[n] is not None})
            ci = sample_kwargs.get("context_index")
            if ci is not None:  # one row per design, each with the fields of its own complex
                tabs = {n: None if v is None else v.index_select(0, torch.as_tensor(ci, device=v.device).long()) for n, v in tabs.items()}
            out.update(_refine.backbone(out, tabs.pop("generation_mask"), group_size=1 if ci is not None else sample_kwargs.get("num_samples", 1),
                                        options=refine, **tabs))
        out["patch"] = sel
        out["complex"] = _patch.paste(full, sel, out, num_samples=sample_kwargs.get("num_samples", 1),
                                      context_index=sample_kwargs.get("context_index"))
        return out

    # ------------------------------------------------------------------ design scoring (build-defined; the training objective per design)
    @torch.no_grad()
    def score(self, seq_idx: torch.LongTensor, xyz: torch.FloatTensor, orientations: torch.FloatTensor, *, generation_mask=None,
              residue_mask=None, res_context_emb=None, pair_context_emb=None, context_index: Optional[torch.LongTensor] = None,
              backbone_dihedrals=None, pairwise_dihedrals=None, distmat=None, atom_mask=None, chain_idx=None, residue_idx=None,
              generate_structure: bool = True, generate_sequence: bool = True, t=None, num_draws: int = 1, seed: Optional[int] = None,
              first_design: int = 0, mode: Optional[str] = None, per_residue: bool = False, return_noised: bool = False,
              rows_per_launch: Optional[int] = None, flags: int = 0) -> Dict[str, torch.Tensor]:
        """Per-design diffusion losses: the reference's training objective (_shared_step, diffab_pytorch.py:808-880; `loss` as
        training_step sums it, :882-887) for each of R designs, averaged over a grid of timesteps and noise draws - a model-side signal to
        rank designs (e.g. many `sample(num_samples=N)` CDRs per antigen) by.

        Designs: seq_idx (R,K), xyz (R,K,3) CA translations or (R,K,A,3) atoms, orientations (R,K,3,3), generation_mask (R,K) - the
        residues that are noised and scored - and residue_mask (R,K, default all true).  Contexts as in sample(): res_context_emb /
        pair_context_emb with one context per design, or n_ctx shared contexts and ``context_index`` (R,) (design r reads context
        context_index[r]), or neither - then encode_context runs first, once, from the batch fields sample() accepts, with the mode's
        visibility.  ``t``: the grid, None = every step 1..T, an int, or a 1-D list / tensor of distinct steps in [1, T].
        ``num_draws`` = M >= 1 noise draws per (design, t).

        Row q = ((r n_t) + j) M + m is design r forward-noised to t_j with draw m and denoised against its context (diffab_score_designs:
        one C-ABI call, chunks of ``rows_per_launch`` rows, no host sync).  Noise: Philox patch first_design + r, step t_j, the
        optimisation-start streams + (m << 16) - draw 0 is exactly sample(optimize_from=t_j, t_stop=t_j, first_patch=first_design + r),
        and scoring designs [lo, hi) with first_design = lo gives that slice of the whole call bitwise.  Per residue with
        generation_mask & residue_mask: seq = KL(q(s_{t-1} | s_t, s_0) || softmax(logits)), translations = sum_c (eps_hat - eps)^2,
        orientations = sum_jk (O0_hat^T O0 - I)^2; each row's terms are summed over its masked residues and divided by their count
        (a design without one gives NaN, as 0/0 does in the reference).
        Modes as sample(): "fixed_backbone" does not noise x and O (their terms are exactly 0 and not part of `loss`), "structure" does
        not noise the sequence (its term is exactly 0 and not part of `loss`).

        Returns seq_loss, translations_loss, orientations_loss (R,) - the mean over the grid and the draws -, loss (R,) - the sum of the
        diffused terms -, per_step (R, n_t, M, 3) and t (n_t,); per_residue (R, n_t, M, K, 3) when asked, and with ``return_noised``
        the noised state of every row (seq_idx_t, translations_t, orientations_t, translations_eps).  Every argument error raises
        ValueError before any library call."""
        who = "score()"
        generate_structure, generate_sequence, keep = _mode_settings(who, mode, generate_structure, generate_sequence)
        if int(flags) & (_hip.FLAG_KEEP_STRUCTURE | _hip.FLAG_KEEP_SEQUENCE):
            raise ValueError(f"{who}: choose the design mode with mode=, not with the DIFFAB_FLAG_KEEP_* bits in flags")
        if generation_mask is None:
            raise ValueError(f"{who} needs generation_mask: which residues to noise and score")
        if not torch.is_tensor(seq_idx) or seq_idx.dim() != 2 or seq_idx.is_floating_point():
            raise ValueError(f"{who}: seq_idx must be an integer tensor (R, K), got {getattr(seq_idx, 'shape', type(seq_idx))}")
        R, K = seq_idx.shape
        if R < 1 or K < 1:
            raise ValueError(f"{who}: no designs to score (seq_idx is {(R, K)})")
        def shape_error(name, v, want):
            return ValueError(f"{who}: {name} is {tuple(v.shape) if torch.is_tensor(v) else type(v).__name__}, expected {want}")

        if not torch.is_tensor(xyz) or not (tuple(xyz.shape) == (R, K, 3) or (xyz.dim() == 4 and tuple(xyz.shape[:2]) == (R, K)
                                                                                and xyz.shape[3] == 3)):
            raise shape_error("xyz", xyz, f"{(R, K, 3)} or {(R, K, 'A', 3)}")
        for name, v, want in (("orientations", orientations, (R, K, 3, 3)), ("generation_mask", generation_mask, (R, K)),
                              ("residue_mask", residue_mask, (R, K))):
            if (v is not None or name != "residue_mask") and (not torch.is_tensor(v) or tuple(v.shape) != want):
                raise shape_error(name, v, want)
        T = int(self.T)
        if t is None:
            grid = list(range(1, T + 1))
        else:
            tt = torch.as_tensor(t)
            if tt.numel() == 0:
                raise ValueError(f"{who}: t is empty")
            if tt.dim() > 1 or tt.is_floating_point() or tt.is_complex() or tt.dtype == torch.bool:
                raise ValueError(f"{who}: t must be None, an int or a 1-D integer list / tensor, got {t!r}")
            grid = [int(v) for v in tt.reshape(-1).tolist()]
            bad = [v for v in grid if not 1 <= v <= T]
            if bad:
                raise ValueError(f"{who}: every t must lie in [1, T = {T}], got {bad}")
            if len(set(grid)) != len(grid):
                raise ValueError(f"{who}: t has duplicate steps {sorted(v for v in set(grid) if grid.count(v) > 1)}")
        if isinstance(num_draws, bool) or not isinstance(num_draws, int) or not 1 <= num_draws <= 65536:
            raise ValueError(f"{who}: num_draws must be an int in [1, 65536], got {num_draws!r}")
        if isinstance(first_design, bool) or not isinstance(first_design, int) or first_design < 0 or first_design + R > 2 ** 32:
            raise ValueError(f"{who}: first_design must be an int >= 0 (first_design + R <= 2^32), got {first_design!r}")
        if rows_per_launch is not None and (isinstance(rows_per_launch, bool) or not isinstance(rows_per_launch, int) or rows_per_launch < 1):
            raise ValueError(f"{who}: rows_per_launch must be an int >= 1, got {rows_per_launch!r}")
        dd = self.denoiser.dims
        for name, v, tail in (("res_context_emb", res_context_emb, (K, dd["D"])), ("pair_context_emb", pair_context_emb, (K, K, dd["C"]))):
            if v is not None and (v.dim() != len(tail) + 1 or tuple(v.shape[1:]) != tail):
                raise ValueError(f"{who}: {name} is {tuple(v.shape)}, expected (contexts, {', '.join(map(str, tail))})")
        ctx_map = None  # host int32 (R,): the context of every design (None: one context per design)
        if context_index is not None:
            ctx_map = _context_map(who, context_index, R, res_context_emb, pair_context_emb, "designs")
        elif res_context_emb is not None or pair_context_emb is not None:
            for name, v in (("res_context_emb", res_context_emb), ("pair_context_emb", pair_context_emb)):
                if v is None or v.shape[0] != R:
                    raise ValueError(f"{who}: without context_index give both contexts with one row per design ({R}); {name} is "
                                     f"{None if v is None else tuple(v.shape)}")
        else:
            _check_encode_fields(who, xyz, atom_mask, chain_idx)
        n_t, M = len(grid), num_draws
        total = R * n_t * M
        rows = min(total, SCORE_ROWS_PER_LAUNCH if rows_per_launch is None else rows_per_launch)

        if res_context_emb is None:
            res_context_emb, pair_context_emb = self._contexts_from_batch(seq_idx, xyz, orientations, generation_mask, residue_mask,
                                                                          backbone_dihedrals, pairwise_dihedrals, distmat, atom_mask,
                                                                          chain_idx, residue_idx, generate_structure, generate_sequence)
        lib = _hip.lib()
        n_ctx = res_context_emb.shape[0]
        dims = self.denoiser.hip_dims(rows, K)
        ws_bytes = lib.diffab_score_workspace_bytes(C.byref(dims), n_ctx)  # (sized by rows and n_ctx only)
        if ws_bytes == 0:
            raise _hip.DiffabHipError(f"diffab_score_workspace_bytes: {lib.diffab_last_error().decode()}")
        out_dev = seq_idx.device
        seq = _hip.dev_i64(seq_idx)
        x = _hip.dev_f32(xyz[:, :, CA_IDX] if xyz.dim() == 4 else xyz)
        O = _hip.dev_f32(orientations)
        gm = _hip.dev_mask(generation_mask)
        rm = None if residue_mask is None else _hip.dev_mask(residue_mask)
        rc, pc = _hip.dev_f32(res_context_emb), _hip.dev_f32(pair_context_emb)
        seed = _so3._draw_seed() if seed is None else int(seed)
        w = self.denoiser.hip_weights()
        sd = self._sched_on_device()
        fwd_tab = self.orientation_diffuser.so3.struct()
        ws = _hip.workspace(ws_bytes)
        dev = seq.device
        terms = torch.empty(R, n_t, M, 3, dtype=torch.float32, device=dev)
        resid = torch.empty(R, n_t, M, K, 3, dtype=torch.float32, device=dev) if per_residue else None
        noised = None
        noised_struct = None
        if return_noised:
            noised = {"seq_idx_t": torch.empty(R, n_t, M, K, dtype=torch.int64, device=dev),
                      "translations_t": torch.empty(R, n_t, M, K, 3, dtype=torch.float32, device=dev),
                      "orientations_t": torch.empty(R, n_t, M, K, 3, 3, dtype=torch.float32, device=dev),
                      "translations_eps": torch.empty(R, n_t, M, K, 3, dtype=torch.float32, device=dev)}
            noised_struct = _hip.ScoreNoised(*[_hip.ptr(noised[k]) for k in ("seq_idx_t", "translations_t", "orientations_t",
                                                                              "translations_eps")])
        ctx_host = None if ctx_map is None else (C.c_int32 * R)(*ctx_map.tolist())
        t_host = (C.c_int32 * n_t)(*grid)
        _hip.check(lib.diffab_score_designs(C.byref(dims), C.byref(w.struct), C.byref(sd.struct), C.byref(fwd_tab), _hip.ptr(seq), _hip.ptr(x),
                                            _hip.ptr(O), _hip.ptr(gm), _hip.ptr(rm), R, _hip.ptr(rc), _hip.ptr(pc), n_ctx, ctx_host, t_host, n_t,
                                            M, seed, first_design, _hip.ptr(terms), _hip.ptr(resid),
                                            None if noised_struct is None else C.byref(noised_struct), _hip.ptr(ws), ws.numel(),
                                            int(flags) | keep, _hip.stream_ptr()), "diffab_score_designs")
        mean = terms.mean(dim=(1, 2))
        diffused = [keep != _hip.FLAG_KEEP_SEQUENCE, keep != _hip.FLAG_KEEP_STRUCTURE, keep != _hip.FLAG_KEEP_STRUCTURE]
        loss = sum(mean[:, i] for i in range(3) if diffused[i])
        out = {"seq_loss": mean[:, 0], "translations_loss": mean[:, 1], "orientations_loss": mean[:, 2], "loss": loss, "per_step": terms,
               "t": torch.tensor(grid, dtype=torch.int64)}
        if per_residue:
            out["per_residue"] = resid
        if return_noised:
            out["noised"] = noised
        return {k: (v.to(out_dev) if torch.is_tensor(v) else {kk: vv.to(out_dev) for kk, vv in v.items()}) for k, v in out.items()}
