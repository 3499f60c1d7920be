"""What the sampler's test files share: the device fixture, models and inputs, the bitwise comparison, the Philox noise of one step and
the oracle's reverse step built on it (GPU side); the stand-in model, the refused library and the zero-state call (host side); and the
padded-patch / gradient helpers of the ragged-K, backward-path and any-dims tests.

Not a test module and not a conftest: test files import what they need by name.  Importing it loads no library and touches no device
(the host tests import it on machines without a GPU) - _hip.lib(), .cuda() and DiffAb are taken inside the functions that need them.
A new sampler feature's test file starts from here and keeps per file only the fixtures whose weight seeds are its own.
"""
import os
import re
import time
import types

import numpy as np
import pytest
import torch

import diffab_oracle as orc
from conftest import REPO, maxrel
from diffab_pytorch import _hip, synthetic as syn
from scratch_poison import GuardDamaged, raw_bytes

STATE = ("seq_idx", "translations", "orientations", "generation_mask")
CTX = ("res_context_emb", "pair_context_emb")
ARGS = ("seq_idx", "translations", "orientations", "res_context_emb", "pair_context_emb")
UNK = 20
TOL = 1e-4   # forward outputs (tests/test_gpu_parity.py)
GTOL = 2e-4  # gradients (the training-step goldens' bar)
PATCH_LENGTH_DIMS = dict(syn.BENCH_DIMS, NL=2)
FLAGS = [0, _hip.FLAG_FORCE_GENERIC, _hip.FLAG_FP32_GEMM, _hip.FLAG_PAIR_PLANES]
FLAG_IDS = ["dispatch", "generic", "fp32gemm", "pairplanes"]
OUTS = ("res_emb", "aa_logits", "translations_eps", "orientations_t0", "seq_posterior")
STREAMS_REVERSE = (orc.STREAM_SEQ, orc.STREAM_TRANS, orc.STREAM_AXIS, orc.STREAM_ANGLE)
STREAMS_OPT = (7, 8, 9, 10)  # STREAM_OPT_SEQ, _TRANS, _AXIS, _ANGLE of csrc/philox.h: the forward-noised start and the scorer's draws


# ====================================================================== GPU side
@pytest.fixture(scope="module")
def hip():
    lib = _hip.lib()  # raises HipUnavailable when there is no gfx950 / no library: never a silent fallback
    assert lib.diffab_device_ok() == 1
    return lib


def make_model(dims, seed, T=100):
    from diffab_pytorch import DiffAb

    torch.manual_seed(0)
    model = DiffAb(dims["D"], dims["C"], dims["NL"], dims["DS"], dims["PQ"], dims["PV"], dims["H"], T=T).cuda()
    model.denoiser.load_state_dict(syn.denoiser_state_dict(dims, seed=seed, prefix=""))
    return model


def bench_model(T_steps, NL=None):
    d = dict(syn.BENCH_DIMS)
    if NL is not None:
        d["NL"] = NL
    return d, make_model(d, 0, T=T_steps)


def unit_model(NL=2, seed=17):
    """(dims, model, oracle state dict) at the unit dims.  The boundary modules keep whatever the global generator gives them: unlike
    make_model this does not reseed it, and the callers' later draws depend on that."""
    from diffab_pytorch import DiffAb

    dims = dict(syn.UNIT_DIMS, NL=NL)
    model = DiffAb(dims["D"], dims["C"], dims["NL"], dims["DS"], dims["PQ"], dims["PV"], dims["H"]).cuda()
    sd = syn.denoiser_state_dict(dims, seed=seed, prefix="")
    model.denoiser.load_state_dict(sd)
    return dims, model, {"denoiser." + k: v for k, v in sd.items()}


def patches(B, K, dims, seed, chains=False, collapse=True, generation_mask=None):
    """syn.patches on the device.  chains=True (the guidance and steering tests) adds two chains with a gap in residue_idx and a few
    padded context residues, and with `collapse` puts the generated residues within ~1 A of one point (clashes and broken bonds for the
    potential to act on).  generation_mask (B, K) replaces the synthetic one (before the collapse)."""
    inp = {k: v.cuda() for k, v in syn.patches(B, K, dims, seed=seed, coord_sigma=6.0).items() if k in STATE + CTX}
    if generation_mask is not None:
        inp["generation_mask"] = generation_mask.cuda()
    return add_chains(inp, seed, collapse) if chains else inp


def add_chains(inp, seed, collapse=True):
    """The chains=True part of `patches`, on device inputs of any origin (in place, and returned)."""
    B, K = inp["seq_idx"].shape
    g = torch.Generator(device="cuda").manual_seed(seed)
    gm = inp["generation_mask"]
    if collapse:
        x = inp["translations"]
        centre = x[torch.arange(B), gm.float().argmax(1)][:, None, :]
        x[:] = torch.where(gm[..., None], centre + torch.randn(x.shape, device="cuda", generator=g), x)
    half = K // 2
    inp["chain_idx"] = (torch.arange(K, device="cuda") >= half).long().expand(B, K).contiguous()
    inp["residue_idx"] = (torch.arange(K, device="cuda") + 7 * (torch.arange(K, device="cuda") >= half)).expand(B, K).contiguous()
    rm = torch.rand(B, K, device="cuda", generator=g) > 0.1
    inp["residue_mask"] = rm | gm
    return inp


def device_patches(B, K, dims, seed):
    """Seeded synthetic patches of SURVEY 8(d)'s shapes, generated on the device (the 8.6 GB pair context of config 5 would take
    minutes through the host generator): N(0,1) contexts, N(0,10^2) A translations, uniform rotations, one CDR-like segment
    of 5..20 generated residues per patch."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    out = {
        "res_context_emb": torch.randn(B, K, dims["D"], device="cuda", generator=g),
        "pair_context_emb": torch.randn(B, K, K, dims["C"], device="cuda", generator=g),
        "translations": 10 * torch.randn(B, K, 3, device="cuda", generator=g),
        "seq_idx": torch.randint(0, 20, (B, K), device="cuda", generator=g),
    }
    q = torch.randn(B, K, 4, device="cuda", generator=g)
    out["orientations"] = orc.uniform_rotation_from_normals(q.cpu()).cuda()
    start = torch.randint(0, K - 20, (B, 1), device="cuda", generator=g)
    length = torch.randint(5, 21, (B, 1), device="cuda", generator=g)
    pos = torch.arange(K, device="cuda")[None]
    out["generation_mask"] = (pos >= start) & (pos < start + length)
    return out


def segment_mask(B, K, spans):
    """(B, K) generation mask with the residues lo .. hi - 1 of every span generated in every patch."""
    gm = torch.zeros(B, K, dtype=torch.bool)
    for lo, hi in spans:
        gm[:, lo:hi] = True
    return gm


def slab_mask(name, B, K, synthetic_mask):
    """The generation masks of the row-plan tests by name, over the 32-row slabs of a K >= 128 patch."""
    if name == "mixed":  # patch 0 nothing, patch 1 everything, the rest the synthetic segments
        gm = synthetic_mask.clone()
        gm[0], gm[1] = False, True
        return gm
    return {"one_slab": segment_mask(B, K, [(12, 21)]),
            "two_adjacent_slabs": segment_mask(B, K, [(31, 33)]),
            "slabs_0_and_3": segment_mask(B, K, [(5, 12), (K - 30, K - 18)]),
            "three_slabs": segment_mask(B, K, [(5, 12), (40, 46), (100, 106)]),  # slabs 0, 1, 3: a two-slab pass, then a one-slab pass
            "row_127": segment_mask(B, K, [(K - 1, K)]),
            "none": torch.zeros(B, K, dtype=torch.bool),
            "all": torch.ones(B, K, dtype=torch.bool)}[name]


def sample(model, inp, **kw):
    tabs = {k: inp[k] for k in ("chain_idx", "residue_idx", "residue_mask") if k in inp}
    return model.sample(inp["seq_idx"], inp["translations"], inp["orientations"], generation_mask=inp["generation_mask"],
                        res_context_emb=inp.get("res_context_emb"), pair_context_emb=inp.get("pair_context_emb"), **tabs, **kw)


def score(model, inp, **kw):
    return model.score(inp["seq_idx"], inp["translations"], inp["orientations"], generation_mask=inp["generation_mask"],
                       residue_mask=inp.get("residue_mask"), res_context_emb=inp.get("res_context_emb"),
                       pair_context_emb=inp.get("pair_context_emb"), **kw)


def rows(inp, index):
    """Every per-patch input at the given rows (a LongTensor on the device): the replicated batch of the shared-context specification."""
    return {k: v.index_select(0, index) for k, v in inp.items()}


def assert_bitwise(got, want, what=""):
    assert set(got) == set(want), (what, set(got) ^ set(want))
    for k in want:
        if isinstance(want[k], dict):  # the "trajectory" / "steering" records
            assert_bitwise(got[k], want[k], (what, k))
            continue
        assert got[k].shape == want[k].shape, (what, k)
        assert torch.equal(got[k], want[k]), (what, k, int((got[k] != want[k]).sum()))


def lanes(first_patch, B, K):
    """(patch, residue) int64 (B, K): the Philox counter words of the rows first_patch .. first_patch + B of the global batch."""
    patch = (first_patch + np.arange(B))[:, None] + np.zeros((B, K), dtype=np.int64)
    res = np.zeros((B, K), dtype=np.int64) + np.arange(K)[None, :]
    return patch, res


def step_noise(seed, first_patch, B, K, t, cdf_row, sigma, streams=STREAMS_REVERSE, draw=0):
    """Which Philox lane feeds which draw of one step, stated once: (z, rotvec, us) on the (first_patch, B, K) grid at counter step t.
    z (B, K, 3): normals 0..2 of the translation stream (the forward process calls it eps); rotvec (B, K, 3): the IGSO3 draw about
    normals 0..2 of the axis stream, its angle from uniforms 0, 1 (bin of the (n_bins,) CDF row, position in the bin) and normal 2 (the
    Gaussian branch) of the angle stream, at the 0-d sigma; us (B, K): uniform 0 of the sequence stream.
    streams = (seq, trans, axis, angle): the reverse loop's by default, STREAMS_OPT with the scorer's draw index m as `draw` (m << 16)."""
    patch, res = lanes(first_patch, B, K)
    s_seq, s_trans, s_axis, s_angle = (s + (draw << 16) for s in streams)
    z = torch.from_numpy(np.stack(orc.philox_normal4(seed, patch, res, t, s_trans)[:3], -1))
    ax = torch.from_numpy(np.stack(orc.philox_normal4(seed, patch, res, t, s_axis)[:3], -1))
    ua = orc.philox_uniform4(seed, patch, res, t, s_angle)
    na = orc.philox_normal4(seed, patch, res, t, s_angle)
    us = torch.from_numpy(orc.philox_uniform4(seed, patch, res, t, s_seq)[0])
    th_h = orc.igso3_theta_from_hist(orc.igso3_bin_from_cdf(cdf_row[None, None, :].expand(B, K, -1), torch.from_numpy(ua[0])),
                                     torch.from_numpy(ua[1]))
    th_g = orc.igso3_theta_from_gaussian(sigma.expand(B, K), torch.from_numpy(na[2]))
    return z, orc.igso3_rotvec(ax, th_h, th_g, sigma.expand(B)), us


def oracle_reverse_step(sd, inp, gm, rev, sched, seed, first_patch, t, NL, H):
    """The oracle's reverse step t -> t-1 on the sampler's Philox lanes, teacher-forced: (s1, x1, O1, den, us, edge) from the host inputs
    `inp`, the oracle state dict `sd` and the model's reverse table `rev`.  edge (B, K) is the distance of every sequence draw's uniform
    from the nearest edge of the oracle posterior's CDF (a draw can flip only on an edge)."""
    B, K = inp["seq_idx"].shape
    z, rotvec, us = step_noise(seed, first_patch, B, K, t, rev._cdf[t].cpu(), sched["beta"].sqrt()[t])
    den = orc.denoiser(sd, *[inp[k] for k in ARGS], sched["beta"][t].expand(B), NL, H)
    s1, x1, O1 = orc.reverse_update(t, inp["seq_idx"], inp["translations"], inp["orientations"], den, gm, sched, z, rotvec, us)
    edge = (den["seq_posterior"].double().cumsum(-1) - us.double()[..., None]).abs().min(dim=-1).values
    return s1, x1, O1, den, us, edge


# ====================================================================== padded patches and gradient checks
def n_real_of(K):
    return K * 201 // 256  # 173 -> 135, 192 -> 150, 196 -> 153, 256 -> 201


def padded(B, K, n_real, seed, zero_orientations=False, dims=PATCH_LENGTH_DIMS):
    """syn.patches with patch 0 real only for its first n_real residues, as collate_fn pads a batch: the tail is outside residue_mask and
    generation_mask, at the origin with the identity frame (or the all-zero matrix: protstruc's fill is not in the reference tree) and
    of the unknown type; its contexts stay random (encode_context gives padded residues non-zero rows too).  The last patch is whole."""
    inp = syn.patches(B, K, dims, seed=seed, coord_sigma=6.0)
    pad = torch.zeros(B, K, dtype=torch.bool)
    pad[0, n_real:] = True
    inp["residue_mask"][pad] = False
    inp["generation_mask"][pad] = False
    inp["translations"][pad] = 0.0
    inp["orientations"][pad] = torch.zeros(3, 3) if zero_orientations else torch.eye(3)
    inp["seq_idx"][pad] = UNK
    return inp


def f64(v):
    return v.detach().cpu().double()


def leaves(sd, prefix):
    return {prefix + k: f64(v).requires_grad_(True) for k, v in sd.items()}


def relu_margin(sd, seq, res_ctx, want, beta):
    """min |pre-activation| over the denoiser's ReLUs (to_res_emb.0 and the heads' first two layers) in the float64 oracle.  An element
    within fp32 rounding of 0 flips its mask between the kernel and the oracle and moves one row of the gradient by O(10 %) (measured:
    a pre-activation of 9e-8 at one residue gave d res_ctx 0.10 off in that row only) - a kink of the function, not an error."""
    s = {k: v.double() for k, v in sd.items()}
    z = [torch.cat([f64(res_ctx), s["sequence_embedding.weight"][seq]], -1) @ s["to_res_emb.0.weight"].T + s["to_res_emb.0.bias"]]
    B, K = seq.shape
    bt = beta.double()
    cat = torch.cat([want["res_emb"].detach(), torch.stack([bt, bt.sin(), bt.cos()], -1)[:, None].expand(B, K, 3)], -1)
    for hd in ("coordinate_denoising", "orientation_denoising", "sequence_denoising"):
        z1 = cat @ s[hd + ".0.weight"].T + s[hd + ".0.bias"]
        z += [z1, z1.relu() @ s[hd + ".2.weight"].T + s[hd + ".2.bias"]]
    return min(float(v.abs().min()) for v in z)


def check_params(named, ref, prefix, what):
    worst = ("", 0.0)
    for n, p in named:
        assert p.grad is not None, (what, n)
        r = maxrel(p.grad, ref[prefix + n].grad)
        worst = max(worst, (n, r), key=lambda v: v[1])
        assert r < GTOL, (what, n, r)
    print(what, "worst parameter gradient:", worst)


# ====================================================================== operands that are only 4-byte aligned
def misaligned(t, nbytes):
    """A contiguous view holding t's values (same shape, dtype and device) with data_ptr() % 16 == nbytes, cut out of a larger buffer of
    its own.  nbytes is a multiple of the element size: 4, 8 or 12 for float32, 8 for int64, any of 1 .. 15 for masks.  What such a view is
    in practice: a parameter behind a 3-wide bias in a flat parameter vector, a batch slice at a ragged patch length."""
    item = t.element_size()
    assert 0 < nbytes < 16 and nbytes % item == 0, (nbytes, t.dtype)
    buf = torch.empty(t.numel() * item + 32, dtype=torch.uint8, device=t.device)
    off = (nbytes - buf.data_ptr()) % 16  # (a fresh allocation is 16-byte aligned, but nothing here relies on it)
    view = buf[off:off + t.numel() * item].view(t.dtype).view(t.shape)
    view.copy_(t)
    return view


def flat_parameters(module, shift_floats=1, grads=None, align_floats=1):
    """Rebind every parameter of `module` to a view of ONE flat float32 vector that starts `shift_floats` floats behind a 16-byte
    boundary and packs the parameters back to back in named_parameters() order, as torch.nn.utils.parameters_to_vector and the
    flat-parameter wrappers lay them out; the values are kept.  Returns (flat, {name: data_ptr() % 16}).
    align_floats: every view starts at a multiple of that many floats from the vector's start (4 with shift_floats = 0: every view on a
    16-byte boundary, which the entries that take weight and gradient tables ask for; a view whose size is a multiple of 4 floats is
    then followed directly by its neighbour, a 3-wide bias by one float of padding).
    grads=<fill>: every .grad becomes a zero-filled view of a second flat vector of the same layout (what a flat-gradient wrapper
    hands the optimiser).  Every byte of both vectors' storage outside the views - the padding, and at least 16 bytes in front of the
    first and behind the last view - holds the float `grads`.  Returns (flat, offsets, flat_grads, outside): outside(flat_vector) is
    the flat uint8 tensor of those bytes."""
    ps = list(module.named_parameters())
    starts, total = [], 0
    for _, p in ps:
        total = (total + align_floats - 1) // align_floats * align_floats
        starts.append(total)
        total += p.numel()
    dev = ps[0][1].device

    def vector():
        if grads is None:
            return misaligned(torch.zeros(total, dtype=torch.float32, device=dev), 4 * shift_floats)
        buf = torch.empty(4 * total + 64, dtype=torch.uint8, device=dev)  # (a multiple of 4 bytes; a fresh allocation is 4-byte aligned)
        buf.view(torch.float32).fill_(grads)
        off = 16 + (4 * shift_floats - buf.data_ptr()) % 16
        return buf[off:off + 4 * total].view(torch.float32)

    flat, gflat = vector(), None if grads is None else vector()
    inside = torch.zeros(total, dtype=torch.bool, device=dev)
    offs = {}
    for at, (n, p) in zip(starts, ps):
        v = flat[at:at + p.numel()].view(p.shape)
        v.copy_(p.data)
        p.data = v
        offs[n] = p.data_ptr() % 16
        if gflat is not None:
            p.grad = gflat[at:at + p.numel()].view(p.shape).zero_()
            inside[at:at + p.numel()] = True
    if grads is None:
        return flat, offs

    def outside(vector):
        raw = raw_bytes(vector)
        keep = torch.ones(raw.numel(), dtype=torch.bool, device=dev)
        lo = 4 * vector.storage_offset()  # (of the float32 view, in floats)
        keep[lo:lo + 4 * total] = ~inside.repeat_interleave(4)
        return raw[keep]

    return flat, offs, gflat, outside


def misalign_parameters(module, select, nbytes=4):
    """Rebind the parameters whose name `select` accepts to misaligned views of their own (values kept); returns their names."""
    hit = []
    for n, p in module.named_parameters():
        if select(n):
            p.data = misaligned(p.data, nbytes)
            hit.append(n)
    return hit


class MisalignedABI:
    """Everything between __enter__ and __exit__ reaches the C ABI through pointers that are only naturally aligned.

    Stands in for the library (_hip.lib(), and as the `hip` argument of a test function): an entry of `entries` is called with every
    device pointer that was made by _hip.ptr - direct arguments and the pointer fields of structs passed by reference - replaced by the
    pointer of a misaligned copy of the tensor (float32 at `f32` bytes behind a 16-byte boundary, 8-byte types at 8, 4-byte integers at
    4, masks at 1), and what the call wrote is copied back into the caller's tensor behind it on the same stream.  `positions`
    ({entry: argument indices}) restricts an entry to some of its arguments (the accepted operands of an entry that refuses others),
    `when` ({entry: predicate of the arguments}) to some of its calls.
    Workspaces (_hip.workspace) and uint8 scratch keep their own alignment rule and are passed as they are.  counts[entry] is the number
    of pointers replaced, so a caller can assert that an entry really ran misaligned.  The Python wrappers, and test functions written
    for aligned tensors, run unchanged on top of it."""

    def __init__(self, entries, f32=4, positions=None, when=None):
        import ctypes

        self.C, self.entries, self.f32, self.positions = ctypes, set(entries), f32, positions or {}
        self.when = when or {}  # {entry: predicate of the argument tuple}: the calls of an entry that are misaligned (default: all)
        self.counts, self.tensors, self.scratch, self.saved = {}, {}, {}, None

    def __enter__(self):
        self.real = _hip.lib()
        self.saved = (_hip.lib, _hip.ptr, _hip.workspace)
        real_ptr, real_ws = _hip.ptr, _hip.workspace

        def ptr(t):
            if t is not None and t.is_cuda and t.numel():
                self.tensors[t.data_ptr()] = t  # (held: the address cannot be given to another tensor meanwhile)
                if self.scratch.get(t.data_ptr()) not in (None, t.numel() if t.dtype == torch.uint8 else -1):
                    del self.scratch[t.data_ptr()]  # a freed workspace's address, given to an operand of a later call
            return real_ptr(t)

        def workspace(nbytes):
            w = real_ws(nbytes)
            self.scratch[w.data_ptr()] = w.numel()
            return w

        _hip.lib, _hip.ptr, _hip.workspace = (lambda: self), ptr, workspace
        return self

    def __exit__(self, *exc):
        _hip.lib, _hip.ptr, _hip.workspace = self.saved
        self.tensors.clear()
        return False

    def _shadow(self, address, made):
        t = self.tensors.get(address)
        if t is None or address in self.scratch or t.dtype == torch.uint8 or not t.is_contiguous():
            return None
        if address not in made:
            off = {8: 8, 4: self.f32 if t.dtype == torch.float32 else 4, 2: 2, 1: 1}[t.element_size()]
            made[address] = (misaligned(t, off), t)
        return made[address][0].data_ptr()

    def __getattr__(self, name):
        fn = getattr(self.real, name)
        if name not in self.entries:
            return fn
        C = self.C

        def call(*args):
            if name in self.when and not self.when[name](args):
                return fn(*args)
            made, restore, out = {}, [], []
            only = self.positions.get(name)
            for i, a in enumerate(args):
                if only is not None and i not in only:
                    out.append(a)
                    continue
                struct = getattr(a, "_obj", None) if not isinstance(a, C.c_void_p) else None
                if struct is None and hasattr(a, "contents") and a:
                    struct = a.contents
                if isinstance(a, C.c_void_p) and a.value:
                    new = self._shadow(a.value, made)
                    out.append(a if new is None else C.c_void_p(new))
                elif isinstance(struct, C.Structure):
                    for field, ftype in struct._fields_:
                        v = getattr(struct, field)
                        if ftype is C.c_void_p and v:
                            new = self._shadow(v, made)
                            if new is not None:
                                restore.append((struct, field, v))
                                setattr(struct, field, new)
                    out.append(a)
                else:
                    out.append(a)
            rc = fn(*out)
            for struct, field, v in restore:
                setattr(struct, field, v)
            for shadow, t in made.values():
                t.copy_(shadow)
            self.counts[name] = self.counts.get(name, 0) + len(made)
            return rc

        return call


# ====================================================================== the operand-alignment table (include/diffab_hip.h, "Operand alignment")
# Mirrored from the header: tests/test_operand_alignment_host.py drives it through the C ABI without a device,
# tests/test_gpu_operand_alignment.py on the device.
NO_DATA, ACCEPTS, REFUSES = "no data operand", "accepts natural alignment", "refuses misaligned float operands"

ENTRIES = {n: NO_DATA for n in (
    "diffab_version", "diffab_last_error", "diffab_device_ok", "diffab_kernel_timer_enable", "diffab_kernel_timer_read",
    "diffab_debug_set_attn_stamps", "diffab_debug_set_attn_variant", "diffab_debug_set_module_stagger", "diffab_debug_set_module_stamps",
    "diffab_set_stream_guard", "diffab_denoise_workspace_bytes", "diffab_sample_workspace_bytes", "diffab_sample_shared_workspace_bytes",
    "diffab_train_tape_bytes", "diffab_train_workspace_bytes", "diffab_ipa_layer_tape_bytes", "diffab_ipa_layer_bwd_workspace_bytes",
    "diffab_residue_embedding_workspace_bytes", "diffab_pair_embedding_workspace_bytes", "diffab_residue_embedding_bwd_workspace_bytes",
    "diffab_pair_embedding_bwd_workspace_bytes", "diffab_pair_embedding_tape_bytes", "diffab_score_workspace_bytes",
    "diffab_debug_dense_forms")}
ENTRIES.update({n: ACCEPTS for n in (
    "diffab_debug_row_tiles", "diffab_debug_row_plan", "diffab_debug_gemm_tn", "diffab_so3_log", "diffab_so3_exp",
    "diffab_so3_matrix_to_rotvec", "diffab_so3_rotvec_to_matrix", "diffab_so3_scale_rot", "diffab_igso3_table_build",
    "diffab_igso3_table_build_accurate", "diffab_igso3_cdf_build", "diffab_igso3_sample", "diffab_igso3_bins_without_replacement",
    "diffab_igso3_sample_bins", "diffab_weighted_multinomial", "diffab_seq_forward_prob", "diffab_seq_posterior",
    "diffab_categorical_sample", "diffab_coord_forward", "diffab_orient_forward", "diffab_philox_fill", "diffab_losses_fwd",
    "diffab_orientation_loss", "diffab_orientation_loss_bwd", "diffab_frames_apply", "diffab_frames_invert", "diffab_frames_bwd",
    "diffab_angular_encoding", "diffab_angular_encoding_bwd", "diffab_featurize_xyz", "diffab_patch_select", "diffab_patch_gather",
    "diffab_patch_scatter", "diffab_metrics_vs_native", "diffab_metrics_pairwise", "diffab_metrics_select_diverse",
    "diffab_metrics_backbone", "diffab_metrics_contacts", "diffab_metrics_ensemble", "diffab_metrics_similarity", "diffab_refine_backbone",
    "diffab_reverse_update", "diffab_reverse_update_jump", "diffab_sample_init", "diffab_sample_init_ex", "diffab_sample_init_noised",
    "diffab_guidance_energy", "diffab_steer_energy", "diffab_steer_resample", "diffab_steer_gather",
    "diffab_metrics_surface")})  # (the last: include/diffab_hip_analysis.h)

# name:kind in prototype order.  f: float operand, refused unless 16-byte aligned; fa: float operand, accepted; i64, m: accepted;
# W / G, LW / LG, RW / RG, PW / PG: denoiser, layer, ResidueEmbedding, PairEmbedding weights / gradients (every buffer refused);
# S, I: schedule and IGSO3 structs (their tables accepted); N: the optional struct of noised copies (accepted; the host test passes
# NULL); ws: workspace / tape / scratch; a number or null: passed as it is.
_DEN_IN = "seq_t:i64 x_t:f O_t:f res_ctx:f pair_ctx:f beta:f"
_PAIR_IN = "pairwise_dihedrals:f residue_idx:i64 stride:0 chain_idx:i64 atom_mask:f sequence_context_mask:m"
_LOOP = ("d:dims w:W s:S rev_tab:I seq:i64 x:f O:f res_ctx:f pair_ctx:f gen_mask:m seed:1 first_patch:0 t_start:5 t_stop:4 "
         "workspace:ws workspace_bytes:0 flags:0")
SIGNATURES = {
    "diffab_ipa_layer_fwd": "d:dims w:LW x:f e:f R:f t:f y:f workspace:ws workspace_bytes:0 flags:0 stream:null",
    "diffab_denoise_step_fwd": f"d:dims w:W {_DEN_IN} out_eps:f out_O0:f out_posterior:f out_logits:f out_res_emb:f workspace:ws "
                               "workspace_bytes:0 flags:0 stream:null",
    "diffab_train_step_fwd": f"d:dims w:W {_DEN_IN} true_post:f true_eps:f true_O0:f gen_mask:m res_mask:m out_eps:f out_O0:f "
                             "out_posterior:f losses3:f tape:ws tape_bytes:0 flags:0 stream:null",
    "diffab_train_step_bwd": "d:dims w:W grads:G seq_t:i64 x_t:f O_t:f pair_ctx:f out_eps:f out_O0:f out_posterior:f true_post:f true_eps:f "
                             "true_O0:f gen_mask:m res_mask:m upstream3:f d_res_ctx:f d_pair_ctx:f tape:ws tape_bytes:0 workspace:ws "
                             "workspace_bytes:0 stream:null",
    "diffab_denoise_step_fwd_taped": f"d:dims w:W {_DEN_IN} out_eps:f out_O0:f out_posterior:f tape:ws tape_bytes:0 flags:0 stream:null",
    "diffab_denoise_step_bwd": "d:dims w:W grads:G seq_t:i64 x_t:f O_t:f pair_ctx:f out_posterior:f d_eps:f d_O0:f d_posterior:f "
                               "d_res_ctx:f d_pair_ctx:f d_x_t:f d_O_t:f tape:ws tape_bytes:0 workspace:ws workspace_bytes:0 stream:null",
    "diffab_ipa_layer_fwd_taped": "d:dims w:LW x:f e:f R:f t:f y:f tape:ws tape_bytes:0 flags:0 stream:null",
    "diffab_ipa_layer_bwd": "d:dims w:LW grads:LG e:f R:f t:f dy:f dx:f d_e:f d_R:f d_t:f tape:ws tape_bytes:0 workspace:ws "
                            "workspace_bytes:0 stream:null",
    "diffab_sample_loop": _LOOP + " stream:null",
    "diffab_sample_loop_ex": _LOOP + " options:null stream:null",
    "diffab_score_designs": "d:dims w:W s:S fwd_tab:I seq:i64 x:fa O:fa gen_mask:m res_mask:m n_designs:1 res_ctx:f pair_ctx:f n_ctx:1 "
                            "ctx_of_design:null t_list:tlist n_t:1 n_draws:1 seed:1 first_design:0 out_terms:fa out_residue:fa noised:N "
                            "workspace:ws workspace_bytes:0 flags:0 stream:null",
    "diffab_residue_embedding_fwd": "d:cdims w:RW seq_idx:i64 xyz:f orientations:f dihedrals:f chain_idx:i64 atom_mask:f "
                                    "structure_context_mask:m sequence_context_mask:m out:f workspace:ws workspace_bytes:0 stream:null",
    "diffab_residue_embedding_bwd": "d:cdims w:RW g:RG seq_idx:i64 xyz:f orientations:f dihedrals:f chain_idx:i64 atom_mask:f "
                                    "structure_context_mask:m sequence_context_mask:m d_out:f workspace:ws workspace_bytes:0 stream:null",
    "diffab_pair_embedding_fwd": f"d:cdims w:PW seq_idx:i64 distmat:f {_PAIR_IN} out:f workspace:ws workspace_bytes:0 stream:null",
    "diffab_pair_embedding_xyz_fwd": f"d:cdims w:PW seq_idx:i64 xyz:f {_PAIR_IN} out:f workspace:ws workspace_bytes:0 stream:null",
    "diffab_pair_embedding_bwd": f"d:cdims w:PW g:PG seq_idx:i64 distmat:f xyz:null {_PAIR_IN} d_out:f workspace:ws workspace_bytes:0 "
                                 "stream:null",
    "diffab_pair_embedding_fwd_taped": f"d:cdims w:PW seq_idx:i64 distmat:f xyz:null {_PAIR_IN} out:f tape:ws tape_bytes:0 workspace:ws "
                                       "workspace_bytes:0 stream:null",
    "diffab_pair_embedding_bwd_taped": f"d:cdims w:PW g:PG seq_idx:i64 distmat:f xyz:null {_PAIR_IN} d_out:f tape:ws tape_bytes:0 "
                                       "workspace:ws workspace_bytes:0 stream:null",
}
ENTRIES.update({n: REFUSES for n in SIGNATURES})
# The two diagnostics that refuse (their own entry comments give the rule; the messages of their scratch checks come first, so the host
# test does not drive them): X, W, bias, Y of diffab_debug_linear128 in modes 1 and 2, X, W, Y of diffab_debug_xstat128.
DEBUG_REFUSES = {"diffab_debug_linear128": ("X", "W", "bias", "Y"), "diffab_debug_xstat128": ("X", "W", "Y")}
ENTRIES.update({n: REFUSES for n in DEBUG_REFUSES})
# the name an entry gives itself in its messages, where it is not its symbol without "diffab_"
MESSAGE_NAME = {"diffab_sample_loop_ex": "sample_loop", "diffab_pair_embedding_xyz_fwd": "pair_embedding_fwd"}

LAYER_FIELDS = tuple(n for n, _ in _hip.IpaLayerWeights._fields_)
MLP3_FIELDS = tuple(n for n, _ in _hip.Mlp3Weights._fields_)
TABLE_FIELDS = {"RW": tuple(n for n, _ in _hip.ResidueEmbWeights._fields_), "PW": tuple(n for n, _ in _hip.PairEmbWeights._fields_)}
TABLE_FIELDS["RG"], TABLE_FIELDS["PG"] = TABLE_FIELDS["RW"], TABLE_FIELDS["PW"]
HOST_NL = 2  # layers of the tables the host test builds


def signature(entry):
    return [tuple(a.split(":")) for a in SIGNATURES[entry].split()]


def table_operands(name, kind, NL=HOST_NL):
    """The buffers of a weight / gradient table as the library names them: w.res_w0, grads.coord.b4, w.layers[1].w_bias, g.mw0."""
    if kind in ("W", "G"):
        base = [f"{name}.{f}" for f in ("seq_emb", "res_w0", "res_b0", "res_w2", "res_b2")]
        heads = [f"{name}.{h}.{f}" for h in ("coord", "orient", "seq") for f in MLP3_FIELDS]
        return base + heads + [f"{name}.layers[{l}].{f}" for l in range(NL) for f in LAYER_FIELDS]
    if kind in ("LW", "LG"):
        return [f"{name}.layers[0].{f}" for f in LAYER_FIELDS]
    return [f"{name}.{f}" for f in TABLE_FIELDS[kind]]


def refused(NL=HOST_NL):
    """{entry: operand names} - every (entry, operand) pair that may be refused, as the header lists them."""
    out = {}
    for entry in SIGNATURES:
        ops = []
        for name, kind in signature(entry):
            if kind == "f":
                ops.append(name)
            elif kind in ("W", "G", "LW", "LG", "RW", "RG", "PW", "PG"):
                ops += table_operands(name, kind, NL)
        out[entry] = ops
    return out


HEADERS = ("diffab_hip.h", "diffab_hip_analysis.h")


def header_source(headers=HEADERS):
    """The headers' declarations as one string: no comments, no preprocessor lines (continued ones included)."""
    src = "\n".join(open(os.path.join(REPO, "include", h)).read() for h in headers)
    src = re.sub(r"/\*.*?\*/", " ", src, flags=re.S).replace("\\\n", " ")
    return re.sub(r"^[ \t]*#.*$", "", src, flags=re.M)


def header_exports(headers=HEADERS):
    return sorted(set(re.findall(r"\b(diffab_[a-z0-9_]+)\s*\(", header_source(headers))))


def _declarators(decl):
    """`const float *w0, *b0` -> [(name, base type, is a pointer, points to const)]; `int32_t B, K` likewise."""
    first, *more = [p.strip() for p in decl.split(",")]
    m = re.fullmatch(r"(const\s+)?([A-Za-z_][A-Za-z0-9_ ]*?)\s*(\*?)\s*([A-Za-z_][A-Za-z0-9_]*)", first)
    assert m, decl
    const, base = bool(m.group(1)), m.group(2).strip()
    out = [(m.group(4), base, bool(m.group(3)), const)]
    for p in more:
        out.append((p.lstrip("* "), base, p.startswith("*"), const))
    return out


def header_prototypes(headers=HEADERS):
    """(structs, prototypes) as the headers declare them.  structs: {typedef name: [(field, base type, pointer, const)]};
    prototypes: {export: [(parameter, base type, pointer, const)]}.  `const` is the pointee's (const float* x); a struct member that
    is a struct by value (diffab_mlp3_weights coord) is a non-pointer field whose base type is in `structs`."""
    src = header_source(headers)
    structs = {}
    for body, name in re.findall(r"typedef\s+struct\s*\{(.*?)\}\s*([a-z0-9_]+)\s*;", src, flags=re.S):
        structs[name] = [f for decl in body.split(";") if decl.strip() for f in _declarators(" ".join(decl.split()))]
    src = re.sub(r"typedef\s+struct\s*\{.*?\}\s*[a-z0-9_]+\s*;", "", src, flags=re.S)
    protos = {}
    for name, params in re.findall(r"\b(diffab_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", src):
        params = " ".join(params.split())
        protos[name] = [] if params in ("", "void") else [_declarators(p)[0] for p in params.split(",")]
    return structs, protos


# ====================================================================== the operand-extent table (include/diffab_hip.h, "Operand extents")
def typed_writes(headers=HEADERS):
    """{export: operands its C types leave writable}: non-const pointer parameters, and the non-const pointer fields of struct
    parameters by path (options.record.seq, noised.x_t, g.shift_dev).  `stream` is a handle, not memory."""
    structs, protos = header_prototypes(headers)

    def fields(path, struct):
        out = []
        for f, base, pointer, const in structs[struct]:
            if base in structs:  # a struct by value or by pointer
                out += fields(f"{path}.{f}", base)
            elif pointer and not const:
                out.append(f"{path}.{f}")
        return out

    out = {}
    for name, params in protos.items():
        ops = []
        for p, base, pointer, const in params:
            if p != "stream":
                ops += fields(p, base) if base in structs else [p] if pointer and not const else []
        out[name] = ops
    return out


# What the C types cannot say: a gradient table is the weights struct again (const float* fields), and every buffer of it is
# accumulated into.  "grads.*" in WRITES.
GRADIENT_TABLES = {"diffab_train_step_bwd": "grads", "diffab_denoise_step_bwd": "grads", "diffab_ipa_layer_bwd": "grads",
                   "diffab_residue_embedding_bwd": "g", "diffab_pair_embedding_bwd": "g", "diffab_pair_embedding_bwd_taped": "g"}
_RECORD = " ".join("opt.record." + f for f in ("slot_dev", "seq", "x", "O", "pred_x", "pred_O", "seq_probs"))
_STEERING = " ".join("{}." + f for f in ("logw", "u_prev", "energy", "ancestors", "scratch"))
_OPTIONS = f"{_RECORD} opt.steps.plan_dev opt.guidance.shift_dev {_STEERING.format(*['opt.steering'] * 5)}"
_SURFACE = ("free_points bound_points design_buried_points free_area bound_area design_buried_area residue_buried bsa_paratope bsa_epitope "
            "bsa_design_epitope n_paratope_buried n_epitope_buried n_hotspot n_hotspot_buried hotspot_buried_area workspace")
# entry -> the operands it may write, by the prototype's names (every export of both headers; "" = none).  Mirrored from the headers:
# tests/test_operand_extents_host.py holds it against typed_writes() + GRADIENT_TABLES, both ways.
WRITES = {n: "" for n in (
    "diffab_version", "diffab_last_error", "diffab_device_ok", "diffab_kernel_timer_enable", "diffab_debug_set_attn_variant",
    "diffab_debug_set_module_stagger", "diffab_set_stream_guard", "diffab_denoise_workspace_bytes", "diffab_sample_workspace_bytes",
    "diffab_sample_shared_workspace_bytes", "diffab_train_tape_bytes", "diffab_train_workspace_bytes", "diffab_ipa_layer_tape_bytes",
    "diffab_ipa_layer_bwd_workspace_bytes", "diffab_residue_embedding_workspace_bytes", "diffab_pair_embedding_workspace_bytes",
    "diffab_residue_embedding_bwd_workspace_bytes", "diffab_pair_embedding_bwd_workspace_bytes", "diffab_pair_embedding_tape_bytes",
    "diffab_score_workspace_bytes")}
WRITES.update({
    "diffab_debug_set_attn_stamps": "device_buffer", "diffab_debug_set_module_stamps": "device_buffer",
    "diffab_kernel_timer_read": "launches total_ms", "diffab_debug_dense_forms": "out5",  # (host pointers)
    "diffab_debug_row_tiles": "tiles", "diffab_debug_row_plan": "plan",
    "diffab_debug_linear128": "Y scratch", "diffab_debug_xstat128": "Y scratch", "diffab_debug_gemm_tn": "C db",
    "diffab_so3_log": "S", "diffab_so3_exp": "R", "diffab_so3_matrix_to_rotvec": "v", "diffab_so3_rotvec_to_matrix": "R",
    "diffab_so3_scale_rot": "out", "diffab_igso3_table_build": "pdf", "diffab_igso3_table_build_accurate": "pdf",
    "diffab_igso3_cdf_build": "cdf", "diffab_igso3_sample": "rotvec", "diffab_igso3_bins_without_replacement": "bins",
    "diffab_igso3_sample_bins": "rotvec", "diffab_weighted_multinomial": "out", "diffab_seq_forward_prob": "prob",
    "diffab_seq_posterior": "post", "diffab_categorical_sample": "out", "diffab_coord_forward": "xt", "diffab_orient_forward": "Ot",
    "diffab_philox_fill": "out", "diffab_losses_fwd": "losses3",
    "diffab_ipa_layer_fwd": "y workspace",
    "diffab_denoise_step_fwd": "out_eps out_O0 out_posterior out_logits out_res_emb workspace",
    "diffab_train_step_fwd": "out_eps out_O0 out_posterior losses3 tape",
    "diffab_train_step_bwd": "grads.* d_res_ctx d_pair_ctx workspace",
    "diffab_orientation_loss": "elems sum1", "diffab_orientation_loss_bwd": "d_pred d_target",
    "diffab_frames_apply": "out", "diffab_frames_invert": "out", "diffab_frames_bwd": "dR dt",
    "diffab_angular_encoding": "out", "diffab_angular_encoding_bwd": "dx",
    "diffab_denoise_step_fwd_taped": "out_eps out_O0 out_posterior tape",
    "diffab_denoise_step_bwd": "grads.* d_res_ctx d_pair_ctx d_x_t d_O_t workspace",
    "diffab_ipa_layer_fwd_taped": "y tape", "diffab_ipa_layer_bwd": "grads.* dx d_e d_R d_t workspace",
    "diffab_residue_embedding_fwd": "out workspace", "diffab_pair_embedding_fwd": "out workspace",
    "diffab_pair_embedding_xyz_fwd": "out workspace",
    "diffab_residue_embedding_bwd": "g.* workspace", "diffab_pair_embedding_bwd": "g.* workspace",
    "diffab_pair_embedding_fwd_taped": "out tape workspace", "diffab_pair_embedding_bwd_taped": "g.* workspace",
    "diffab_featurize_xyz": "orientations backbone_dihedrals backbone_dihedrals_mask pairwise_dihedrals",
    "diffab_patch_select": "index patch_mask count", "diffab_patch_gather": "dst", "diffab_patch_scatter": "dst",
    "diffab_metrics_vs_native": "aar rmsd rmsd_aligned segment_aar segment_rmsd segment_rmsd_aligned",
    "diffab_metrics_pairwise": "rmsd seq_identity workspace", "diffab_metrics_select_diverse": "index min_dist count",
    "diffab_metrics_backbone": "phi psi omega peptide_bond n_bonds max_peptide_deviation n_chain_break n_cis workspace",
    "diffab_metrics_contacts": "n_clash clash_score min_distance n_contact_pairs n_paratope n_epitope n_hotspot_contacted n_hotspot "
                               "residue_clash residue_contact workspace",
    "diffab_metrics_ensemble": "aa_freq entropy consensus mean_points rmsf log_prob consensus_identity rmsd_to_mean n_eff central workspace",
    "diffab_metrics_similarity": "n_pairs n_pairs_interface preserved preserved_interface lddt_residue lddt lddt_thresholds ilddt_residue "
                                 "ilddt lddt_segment n_native native_contacts_residue n_design n_kept fnat fnonnat kept_residue",
    "diffab_metrics_surface": _SURFACE,
    "diffab_refine_backbone": "out_translations out_orientations energy_before energy_after terms_after max_shift workspace",
    "diffab_reverse_update": "seq x O", "diffab_reverse_update_jump": "seq x O r_out",
    "diffab_sample_init": "seq x O", "diffab_sample_init_ex": "seq x O", "diffab_sample_init_noised": "seq x O",
    "diffab_sample_loop": "seq x O workspace", "diffab_sample_loop_ex": f"seq x O workspace {_OPTIONS}",
    "diffab_guidance_energy": "g.shift_dev clash bond n_clash max_bond_deviation grad",
    "diffab_steer_energy": f"{_STEERING.format(*['steering'] * 5)} energy_out",
    "diffab_steer_resample": "logw u_prev ancestors_out ess_out", "diffab_steer_gather": "seq x O scratch",
    "diffab_score_designs": "out_terms out_residue noised.seq_t noised.x_t noised.O_t noised.eps workspace",
})
# A non-null device pointer that resolves to no contiguous tensor the harness knows, and may pass as it is: (entry, operand) -> why.
UNGUARDED = {("diffab_patch_select", "ca"): "ca / ca_stride address a strided view (atom slot 1 of a (B,N,A,3) array): no contiguous extent "
                                            "that a copy could stand in for"}
GUARD_BYTES = 64 * 1024  # one 128 x 128 fp32 tile
GUARD_FILLS = ("nan0", "ones")


def writable(entry, operand):
    ops = WRITES[entry].split()
    return operand in ops or any(o.endswith(".*") and operand.startswith(o[:-1]) for o in ops)


class ConstOperandChanged(AssertionError):
    pass


class UnresolvedPointer(AssertionError):
    pass


def tensors_of(*things, depth=3):
    """Every tensor reachable from `things`: tensors, modules (parameters, their .grad, buffers, and what their attributes cache - the
    schedule and IGSO3 tables of a DiffAb), pointer tables (_hip.SchedOnDevice.tensors, DenoiserWeightsOnDevice.keep), dicts, lists."""
    out, seen = [], set()

    def walk(v, d):
        if id(v) in seen or d < 0:
            return
        seen.add(id(v))
        if isinstance(v, torch.Tensor):
            out.append(v)
            if v.grad is not None:
                out.append(v.grad)
        elif isinstance(v, torch.nn.Module):
            for m in v.modules():
                for t in list(m.parameters(recurse=False)) + list(m.buffers(recurse=False)):
                    walk(t, d)
                for k, a in vars(m).items():
                    if k not in ("_parameters", "_buffers", "_modules"):
                        walk(a, d - 1)
        elif isinstance(v, dict):
            for a in v.values():
                walk(a, d - 1)
        elif isinstance(v, (list, tuple, set)):
            for a in v:
                walk(a, d - 1)
        elif hasattr(v, "__dict__") and not isinstance(v, (type, types.ModuleType, types.FunctionType)):
            for a in vars(v).values():
                walk(a, d - 1)

    for v in things:
        walk(v, depth)
    return out


def bytes_of(t):
    """A contiguous tensor's own bytes as a flat uint8 view (raw_bytes is the whole storage)."""
    return t.detach().reshape(-1).view(torch.uint8)


class GuardedABI:
    """Everything between __enter__ and __exit__ reaches the C ABI through operands that stand between two guards: the harness of the
    operand-extent contract (include/diffab_hip.h, "Operand extents").

    Stands in for the library like MisalignedABI (_hip.lib(), _hip.ptr, _hip.workspace; the same `entries`, `positions`, `when` and
    `counts`).  An entry of `entries` is called with every device pointer - direct arguments, void* fields of structs passed by
    reference, structs nested by value (w.coord), structs behind pointer fields (options.record, noised) and the host array
    w.layers[NL], NL from the dims argument - replaced by a pointer into the interior of a fresh uint8 buffer: the interior holds the
    tensor's bytes and starts at the original's address modulo 256 (every entry picks the kernel it would have picked, nothing is newly
    refused), and GUARD_BYTES of guard lie directly in front of it and directly behind its last byte.  The guards hold `fill`:
    "nan0" = NaN (0xFF bytes) in float operands and 0 in integer and mask operands, "ones" = the value 1 of the type.  Both are valid
    wherever an integer is an index, a stray store cannot equal both, a float read past the end that is used turns the result into NaN
    under "nan0", a mask read past the end flips under "ones" - so every case runs under both.  One address has one shadow: aliased
    operands stay aliased.  Buffers from _hip.workspace pass as they are (tests/scratch_poison.py owns them).

    After the call the device is synchronised, and (a) a guard byte that changed raises GuardDamaged with the entry, the operand, the
    side and the element offset of the first damaged byte; (b) an operand the entry may not write (WRITES) whose interior differs from
    the caller's tensor raises ConstOperandChanged; (c) the others are copied back into the caller's tensor.  Struct fields are put back.

    A pointer is resolved through the tensors _hip.ptr saw inside the context and those of `known` (tensors_of: what was built before -
    cached schedule and IGSO3 structs, weight tables).  A non-null device pointer that resolves to none of them raises UnresolvedPointer
    unless UNGUARDED names it.  `lib` and `argtypes` replace the library and _hip's symbol table (tests/test_operand_extents_host.py
    drives the harness with Python stand-ins on CPU tensors).  Does not mix with an outer torch.cuda.graph capture (the copies, fills
    and checks are launches of their own); DIFFAB_FLAG_GRAPH_SAMPLER captures inside the call and is fine."""

    def __init__(self, entries, fill, known=(), positions=None, when=None, lib=None, argtypes=None):
        import ctypes

        if fill not in GUARD_FILLS:
            raise ValueError(f"fill must be one of {GUARD_FILLS}, not {fill!r}")
        self.C, self.entries, self.fill, self.positions, self.when = ctypes, set(entries), fill, positions or {}, when or {}
        self.real, self.argtypes = lib, argtypes
        self.headers, self.host_operands = HEADERS, ()  # (the gated-stream harness widens both)
        self.counts, self.tensors, self.known, self.scratch, self.saved, self.patterns, self.last = {}, {}, {}, {}, None, {}, {}
        for t in tensors_of(*known):
            self._see(t, self.known)  # (a tensor _hip.ptr sees inside the context goes first: the operand itself, not a buffer it is cut from)

    def _see(self, t, table=None):
        if t is not None and t.numel():
            table, had = self.tensors if table is None else table, None if table is None else table.get(t.data_ptr())
            if had is None or t.numel() * t.element_size() < had.numel() * had.element_size():  # of two known= tensors at one address the
                table[t.data_ptr()] = t  # smaller: a guard too near is reported, one too far is not.  (Held: the address stays its own.)
            if self.scratch.get(t.data_ptr()) not in (None, t.numel() if t.dtype == torch.uint8 else -1):
                del self.scratch[t.data_ptr()]  # a freed workspace's address, given to an operand of a later call

    def __enter__(self):
        if self.real is None:
            self.real = _hip.lib()
        if self.argtypes is None:
            self.argtypes = {n: a for n, (_, a) in list(_hip.SYMBOLS.items()) + list(_hip.ANALYSIS_SYMBOLS.items())}
        self.params = {n: [p[0] for p in ps] for n, ps in header_prototypes(self.headers)[1].items()}
        self.saved = (_hip.lib, _hip.ptr, _hip.workspace)
        real_ptr, real_ws = _hip.ptr, _hip.workspace

        def ptr(t):
            self._see(t)
            return real_ptr(t)

        def workspace(nbytes):
            w = real_ws(nbytes)
            self.scratch[w.data_ptr()] = w.numel()
            return w

        _hip.lib, _hip.ptr, _hip.workspace = (lambda: self), ptr, workspace
        return self

    def __exit__(self, *exc):
        _hip.lib, _hip.ptr, _hip.workspace = self.saved
        self.tensors.clear()
        self.known.clear()
        self.last.clear()
        return False

    # ------------------------------------------------------------------ shadows
    def _guard(self, part, dtype):
        """Fill the guard bytes `part` (a uint8 view) with the fill's value of `dtype`."""
        if dtype.is_floating_point and self.fill == "nan0":
            part.fill_(0xFF)
        elif dtype in (torch.bool, torch.uint8):
            part.fill_(0 if self.fill == "nan0" else 1)
        else:
            part.view(dtype).fill_(0 if self.fill == "nan0" else 1)

    def _pattern(self, dtype, device):
        key = (dtype, device)
        if key not in self.patterns:
            self.patterns[key] = torch.empty(GUARD_BYTES, dtype=torch.uint8, device=device)
            self._guard(self.patterns[key], dtype)
        return self.patterns[key]

    def _new_shadow(self, t, address, owner, operand):
        """A fresh buffer whose interior holds t's bytes at `address` modulo 256, between two guards.  `owner` is the struct the pointer
        was a field of (None for a direct argument)."""
        n = t.numel() * t.element_size()
        buf = torch.empty(n + 2 * GUARD_BYTES + 256, dtype=torch.uint8, device=t.device)
        lo = GUARD_BYTES + (address - buf.data_ptr() - GUARD_BYTES) % 256
        self._guard(buf[lo - GUARD_BYTES:lo], t.dtype)
        self._guard(buf[lo + n:lo + n + GUARD_BYTES], t.dtype)
        buf[lo:lo + n].copy_(bytes_of(t))
        return dict(buf=buf, lo=lo, n=n, t=t, names=[], writable=False)

    def _writable(self, entry, operand):
        return writable(entry, operand)

    def _shadow(self, entry, operand, address, made, owner=None):
        """The shadow pointer of `address`, or None for a pointer that passes as it is."""
        if address in self.scratch:
            return None
        t = self.tensors.get(address, self.known.get(address))
        if t is None or not t.is_contiguous():
            if (entry, operand) in UNGUARDED:
                return None
            raise UnresolvedPointer(f"{entry}: operand {operand} = {address:#x} is not the data pointer of a contiguous tensor the harness "
                                    "has seen (register it with known=, or name it in UNGUARDED with the reason)")
        if address not in made:
            made[address] = self._new_shadow(t, address, owner, operand)
        s = made[address]
        s["names"].append(operand)
        s["writable"] |= self._writable(entry, operand)
        return s["buf"].data_ptr() + s["lo"]

    def _struct_pointers(self, struct, path, NL, visit):
        C = self.C
        for field, ftype in struct._fields_:
            v, p = getattr(struct, field), f"{path}.{field}"
            if ftype is C.c_void_p:
                if v:
                    visit(struct, field, v, p)
            elif isinstance(ftype, type) and issubclass(ftype, C.Structure):  # by value: w.coord
                self._struct_pointers(v, p, NL, visit)
            elif isinstance(getattr(ftype, "_type_", None), type) and issubclass(ftype._type_, C.Structure) and v:  # options.record, w.layers
                if field == "layers":
                    for l in range(NL):
                        self._struct_pointers(v[l], f"{p}[{l}]", NL, visit)
                else:
                    self._struct_pointers(v.contents, p, NL, visit)
            # (everything else is a number or a HOST array: slot_of_step, steps, ctx_of_row)

    def _run(self, entry, fn, args, made):
        return fn(*args)

    def _check(self, entry, made):
        devices = {s["buf"].device for s in made.values()}
        for d in devices:
            if d.type == "cuda":
                torch.cuda.synchronize(d)
        fine = []  # the common case, one synchronisation per call: every guard and every const interior compared on the device
        for s in made.values():
            buf, lo, n, t = s["buf"], s["lo"], s["n"], s["t"]
            want = self._pattern(t.dtype, buf.device)
            fine += [(buf[lo - GUARD_BYTES:lo] == want).all(), (buf[lo + n:lo + n + GUARD_BYTES] == want).all()]
            if not s["writable"]:
                fine.append((buf[lo:lo + n] == bytes_of(t)).all())
        if all(bool(torch.stack([f for f in fine if f.device == d]).all()) for d in devices):
            for s in made.values():
                if s["writable"]:
                    bytes_of(s["t"]).copy_(s["buf"][s["lo"]:s["lo"] + s["n"]])
            return
        for s in made.values():
            buf, lo, n, t = s["buf"], s["lo"], s["n"], s["t"]
            item, name = t.element_size(), " / ".join(dict.fromkeys(s["names"]))
            want = self._pattern(t.dtype, buf.device)
            for side, part in (("in front of", buf[lo - GUARD_BYTES:lo]), ("behind", buf[lo + n:lo + n + GUARD_BYTES])):
                if not torch.equal(part, want):
                    bad = (part != want).nonzero().flatten()
                    first = int(bad[0])
                    if side == "behind":
                        where = f"element {first // item} behind its end (operand of {t.numel()} elements, {tuple(t.shape)})"
                    else:
                        where = f"element {(first - GUARD_BYTES) // item} from its start (negative: in front of it)"
                    raise GuardDamaged(f"{entry}: operand {name} ({t.dtype}) was written out of bounds {side} it: first damaged guard byte at "
                                       f"{where}, {int(bad.numel())} damaged bytes on that side, value 0x{int(part[first]):02x}, "
                                       f'guard fill "{self.fill}"')
            inner, own = buf[lo:lo + n], bytes_of(t)
            if s["writable"]:
                own.copy_(inner)
            elif not torch.equal(inner, own):
                first = int((inner != own).nonzero().flatten()[0])
                raise ConstOperandChanged(f"{entry}: operand {name} is not writable (WRITES) and changed: first changed element {first // item} "
                                          f"of {t.numel()}")

    def __getattr__(self, name):
        fn = getattr(self.real, name)
        if name not in self.entries:
            return fn
        C = self.C

        def call(*args):
            if name in self.when and not self.when[name](args):
                return fn(*args)
            made, restore, out = {}, [], []
            only, types_, names = self.positions.get(name), self.argtypes[name], self.params[name]
            assert len(args) == len(types_) == len(names), (name, len(args), len(types_), len(names))
            dims = [getattr(a, "_obj", None) or (a.contents if hasattr(a, "contents") and a else None) for a in args]
            NL = next((int(v.NL) for v in dims if isinstance(v, _hip.Dims)), 1)

            def visit(struct, field, v, path):
                new = self._shadow(name, path, v, made, struct)
                if new is not None:
                    restore.append((struct, field, v))
                    setattr(struct, field, new)

            try:
                for i, (a, at, pname) in enumerate(zip(args, types_, names)):
                    if (only is not None and i not in only) or pname == "stream" or (name, pname) in self.host_operands:
                        out.append(a)
                    elif at is C.c_void_p:
                        v = a.value if isinstance(a, C.c_void_p) else a
                        new = self._shadow(name, pname, int(v), made) if v else None
                        out.append(a if new is None else C.c_void_p(new))
                    elif isinstance(getattr(at, "_type_", None), type) and issubclass(at._type_, C.Structure):
                        struct = getattr(a, "_obj", None) if a is not None else None
                        if struct is None and a is not None and hasattr(a, "contents") and a:
                            struct = a.contents
                        if struct is not None:
                            self._struct_pointers(struct, pname, NL, visit)
                        out.append(a)
                    else:
                        out.append(a)
                self.last = made  # (for the host tests' stand-ins: the shadows of the call in flight)
                rc = self._run(name, fn, out, made)
            finally:
                for struct, field, v in restore:
                    setattr(struct, field, v)
            self._check(name, made)
            self.counts[name] = self.counts.get(name, 0) + len(made)
            return rc

        return call


# ====================================================================== the stream contract (include/diffab_hip.h, "Streams")
LATER_HEADERS = ("diffab_hip_hbonds.h", "diffab_hip_cluster.h", "diffab_hip_interface.h", "diffab_hip_develop.h", "diffab_hip_energy.h",
                 "diffab_hip_novelty.h", "diffab_hip_conformation.h")
ALL_HEADERS = HEADERS + LATER_HEADERS  # the nine headers of the product ABI
DIAGNOSTIC_HEADERS = ("diffab_hip_debug.h",)  # declared for the launch-form tests alone: no ctypes table in _hip
# (entry, operand by the prototype's name or struct path): HOST arrays, read during the call only.  They pass the harness as they are.
HOST_ARRAYS = (("diffab_sample_loop_ex", "opt.ctx_of_row"), ("diffab_sample_loop_ex", "opt.record.slot_of_step"),
               ("diffab_sample_loop_ex", "opt.steps.steps"), ("diffab_sample_loop_ex", "opt.steps.beta_jump"),
               ("diffab_sample_loop_ex", "opt.steps.alpha_jump"), ("diffab_score_designs", "ctx_of_design"),
               ("diffab_score_designs", "t_list"), ("diffab_metrics_pair_energy", "bin_edges"), ("diffab_metrics_motifs", "motifs"),
               ("diffab_metrics_surface", "point_radius"), ("diffab_patch_gather", "complex_of_row"))
# HOST memory the headers name that is no array operand of a device call: (entry or struct, name) -> why it has no overwrite case
HOST_NOT_ARRAYS = {("diffab_denoiser_weights", "layers"): "a host table of pointer structs: its device pointers are copied into launch "
                                                          "arguments, and every rerun row that takes `w` passes it rebuilt per call",
                   ("diffab_debug_dense_forms", "out5"): "host output of a host-only query: nothing is enqueued",
                   ("diffab_debug_start_classes", "plan"): "on_device = 0 runs on the host alone; diagnostic header"}
# Float operands that keep their true values in the decoy: tables a kernel searches or indexes by
TRUE_VALUE_OPERANDS = ("cdf", "sigmas", "pdf")
# Calls that may hold the host: entry -> (predicate of {parameter: argument}, why).  They are held to the value check only.
GRAPH_SAMPLER_DRAINS = "DIFFAB_FLAG_GRAPH_SAMPLER drains the private replay stream before the call returns (include/diffab_hip.h)"
MAY_WAIT = {"diffab_sample_loop": (lambda a: bool(int(a["flags"]) & _hip.FLAG_GRAPH_SAMPLER), GRAPH_SAMPLER_DRAINS),
            "diffab_sample_loop_ex": (lambda a: bool(int(a["flags"]) & _hip.FLAG_GRAPH_SAMPLER), GRAPH_SAMPLER_DRAINS)}
# Gate length (profiles/stream_contract.md): the longest host time of one entry call at the shapes of tests/test_gpu_stream_contract.py
# was measured ungated; the floor is well above it, and an entry whose own calls have taken longer gets ten times its longest so far.
GATE_FLOOR_MS = 40.0
GATE_MULTIPLE = 10.0
GATE_RETRY = 4.0


class EntryWaited(AssertionError):
    pass


def all_argtypes():
    return {n: a for name in dir(_hip) if name.endswith("SYMBOLS") for n, (_, a) in getattr(_hip, name).items()}


def all_writes():
    """WRITES, and for the later headers what their C types leave writable (they have no gradient tables)."""
    out = dict(WRITES)
    out.update({n: " ".join(ops) for n, ops in typed_writes(LATER_HEADERS).items()})
    return out


_GATED = {}


def hip_runtime():
    """The HIP runtime torch has loaded, through ctypes (dlopen of a loaded library hands back the same library)."""
    import ctypes

    with open("/proc/self/maps") as f:
        paths = sorted({line.split()[-1] for line in f if "libamdhip64" in line})
    assert paths, "torch has not loaded libamdhip64"
    return ctypes.CDLL(paths[0])


def gated_stream():
    """(side stream, sleep cycles per millisecond): one stream for every harness of the process, checked once to be non-blocking (a
    blocking stream synchronises with the legacy default stream: every stray launch on it would look ordered), and the gate kernel's
    length calibrated once with events."""
    import ctypes

    if not _GATED:
        s = torch.cuda.Stream()
        flags = ctypes.c_uint(0)
        rc = hip_runtime().hipStreamGetFlags(ctypes.c_void_p(s.cuda_stream), ctypes.byref(flags))
        assert rc == 0 and flags.value & 1, ("the side stream must be hipStreamNonBlocking", rc, flags.value)
        cycles, best = 20_000_000, None
        with torch.cuda.stream(s):
            for _ in range(3):  # (the first run pays the kernel's load)
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record(s)
                torch.cuda._sleep(cycles)
                b.record(s)
                b.synchronize()
                best = a.elapsed_time(b) if best is None else min(best, a.elapsed_time(b))
        assert best > 0.5, ("the gate kernel did not run for a measurable time", best)
        _GATED.update(stream=s, cycles_per_ms=cycles / best, calibration=(cycles, best))
    return _GATED["stream"], _GATED["cycles_per_ms"]


class GatedStreamABI(GuardedABI):
    """Everything between __enter__ and __exit__ reaches the C ABI on a side stream that is busy: the harness of the stream contract
    (include/diffab_hip.h, "Streams") - every launch and copy of an entry on `stream` or ordered by events after and before it, no host
    wait, HOST arrays dead on return.

    Stands in for the library like GuardedABI and shares its pointer resolution (`known`, `positions`, `when`, `counts`, `lib`,
    `argtypes`; all nine headers).  A call of a listed entry: every operand gets a shadow at the original's address modulo 256
    (workspaces, tapes and scratch pass as they are).  Before anything else a float32 shadow holds a DECOY, the caller's values times
    0.5; integer, mask, schedule and IGSO3 shadows hold the true values (a decoy index or CDF could send a stray kernel out of bounds).
    After one synchronisation the side stream waits for the caller's current stream and gets, in order: the gate (bounded device work,
    torch.cuda._sleep), the event gate_done, a copy of every caller tensor into its shadow (outputs too), the entry with its `stream`
    argument replaced, a copy of the writable shadows back, the event done - for which the caller's current stream then waits, with no
    host synchronisation.

    A kernel or copy that the entry puts on any other stream without an event path from `stream` runs during the gate: it reads
    decoys, or what it writes is overwritten by the copy-in, and the caller's own comparison fails.  A host wait inside the entry
    outlasts the gate: returned_early = not gate_done.query(), taken directly after the entry returns, is False.  Such a call is
    repeated once (its copy-back had not been enqueued) under a gate GATE_RETRY times as long; if it still has not returned early
    EntryWaited names the entry - unless MAY_WAIT lists the call.  calls holds (entry, returned_early, gate ms, host ms, attempts,
    may wait) of every gated call.  on_return ({entry: f({parameter: argument})}) runs directly after returned_early is taken: the
    HOST-array cases overwrite the array there.  gate=False runs everything but the gate (the host times of profiles/stream_contract.md).
    Does not mix with an outer stream capture."""

    def __init__(self, entries, known=(), positions=None, when=None, lib=None, argtypes=None, floor_ms=GATE_FLOOR_MS, multiple=GATE_MULTIPLE,
                 may_wait=MAY_WAIT, on_return=None, gate=True):
        super().__init__(entries, "nan0", known=known, positions=positions, when=when, lib=lib, argtypes=argtypes)
        self.headers, self.host_operands = ALL_HEADERS, set(HOST_ARRAYS)
        self.floor_ms, self.multiple, self.may_wait, self.on_return, self.gate = floor_ms, multiple, may_wait, on_return or {}, gate
        self.calls, self.host_ms, self.held, self.writes = [], {}, [], all_writes()

    def __enter__(self):
        if self.argtypes is None:
            self.argtypes = all_argtypes()
        self.stream, self.cycles_per_ms = gated_stream()
        return super().__enter__()

    def __exit__(self, *exc):
        self.stream.synchronize()  # the shadows stay referenced until everything that uses them has run
        torch.cuda.current_stream().synchronize()
        self.held.clear()
        return super().__exit__(*exc)

    def _writable(self, entry, operand):
        ops = self.writes[entry].split()
        return operand in ops or any(o.endswith(".*") and operand.startswith(o[:-1]) for o in ops)

    def _new_shadow(self, t, address, owner, operand):
        n = t.numel() * t.element_size()
        buf = torch.empty(n + 512, dtype=torch.uint8, device=t.device)
        lo = (address - buf.data_ptr()) % 256
        inner = buf[lo:lo + n]
        inner.copy_(bytes_of(t))
        true_values = isinstance(owner, (_hip.Sched, _hip.Igso3)) or operand.split(".")[-1] in TRUE_VALUE_OPERANDS
        if t.dtype == torch.float32 and not true_values:
            inner.view(torch.float32).mul_(0.5)  # the decoy: finite and valid wherever the true value is
        self.held.append(buf)
        return dict(buf=buf, lo=lo, n=n, t=t, names=[], writable=False)

    def _run(self, entry, fn, args, made):
        names = self.params[entry]
        at = names.index("stream")
        named = dict(zip(names, args))
        args = list(args)
        args[at] = self.C.c_void_p(self.stream.cuda_stream)
        may_wait = entry in self.may_wait and bool(self.may_wait[entry][0](named))
        cur, s = torch.cuda.current_stream(), self.stream
        attempts = 0
        for scale in (1.0, GATE_RETRY):
            attempts += 1
            cur.synchronize()  # allocation and decoy fill are complete: the one synchronisation, of the two streams involved alone
            s.synchronize()  # (a repeated call: the first attempt has drained)
            gate_ms = scale * max(self.floor_ms, self.multiple * self.host_ms.get(entry, 0.0)) if self.gate else 0.0
            s.wait_stream(cur)  # the inputs were produced on the caller's stream
            gate_done = torch.cuda.Event()
            with torch.cuda.stream(s):
                if self.gate:
                    torch.cuda._sleep(int(gate_ms * self.cycles_per_ms))
                gate_done.record(s)
                for sh in made.values():
                    sh["buf"][sh["lo"]:sh["lo"] + sh["n"]].copy_(bytes_of(sh["t"]))
            t0 = time.perf_counter()
            rc = fn(*args)
            returned_early = not gate_done.query()
            host_ms = 1e3 * (time.perf_counter() - t0)
            if entry in self.on_return:
                self.on_return[entry](named)
            if returned_early or not self.gate:
                self.host_ms[entry] = max(self.host_ms.get(entry, 0.0), host_ms)
            if returned_early or may_wait or not self.gate or rc != 0:
                break
        self.calls.append((entry, returned_early, gate_ms, host_ms, attempts, may_wait))
        with torch.cuda.stream(s):
            for sh in made.values():
                if sh["writable"]:
                    bytes_of(sh["t"]).copy_(sh["buf"][sh["lo"]:sh["lo"] + sh["n"]])
        done = torch.cuda.Event()
        done.record(s)
        cur.wait_event(done)
        if self.gate and not returned_early and not may_wait and rc == 0:
            raise EntryWaited(f"{entry} held the host until its stream had drained: it returned after a gate of {gate_ms:.0f} ms "
                              f"had ended, twice (host time of the call {host_ms:.1f} ms)")
        return rc

    def _check(self, entry, made):
        pass  # (values are the caller's own comparison; extents are GuardedABI's)


# ====================================================================== host side: argument checks before the library
class ReachedTheLibrary(Exception):
    pass


def refuse():
    raise ReachedTheLibrary()


def refuse_library(monkeypatch):
    """Every check under test must fire before the call asks for the library: any access raises ReachedTheLibrary."""
    monkeypatch.setattr(_hip, "lib", refuse)
    monkeypatch.setattr(_hip, "load_library", refuse)


def stand_in(methods=("sample",), aa_vocab=21, T=10):
    """DiffAb.<method> bound to a stand-in with the model's dimensions only (a DiffAb builds its IGSO3 tables on the device)."""
    from diffab_pytorch import DiffAb
    from diffab_pytorch.diffab_pytorch import Denoiser

    d = dict(syn.BENCH_DIMS, NL=1)
    den = Denoiser(d["D"], d["C"], d["NL"], d["DS"], d["PQ"], d["PV"], d["H"], aa_vocab)
    stub = types.SimpleNamespace(denoiser=den, T=T)
    for m in methods:
        setattr(stub, m, types.MethodType(getattr(DiffAb, m), stub))
    return stub


def inputs(rows, K=16, n_ctx=None, D=128, Cp=64):
    """A zero state of `rows` designs (residues 3..7 generated) with n_ctx contexts (one per row by default)."""
    n_ctx = rows if n_ctx is None else n_ctx
    gm = torch.zeros(rows, K, dtype=torch.bool)
    gm[:, 3:8] = True
    return dict(seq_idx=torch.zeros(rows, K, dtype=torch.long), xyz=torch.zeros(rows, K, 3),
                orientations=torch.eye(3).expand(rows, K, 3, 3).clone(), generation_mask=gm, res_context_emb=torch.zeros(n_ctx, K, D),
                pair_context_emb=torch.zeros(n_ctx, K, K, Cp))


def call(model, inp, method="sample", **kw):
    inp = dict(inp)
    return getattr(model, method)(inp.pop("seq_idx"), inp.pop("xyz"), inp.pop("orientations"), seed=1, **inp, **kw)
