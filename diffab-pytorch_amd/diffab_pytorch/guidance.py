"""Structure guidance of the reverse sampler: a clash and a chain-bond potential on the CA translations.

``SampleGuidance`` configures ``DiffAb.sample(guidance=...)``: at every guided step the gradient of

    U = clash * sum_nonbonded max(0, clash_distance - d)^2 + bond * sum_bonded (d - bond_length)^2

taken at the model's clean-structure prediction x0_hat, times the step's variance beta'_t and capped at max_shift, is subtracted from the
mean of the translations (`diffab_sample_loop_ex`, option `guidance`).  ``structure_energy`` evaluates the same potential at given coordinates on the
device (`diffab_guidance_energy`): clash and bond statistics of finished designs, and the gradient.
"""
from __future__ import annotations

import ctypes as C
import math
from dataclasses import dataclass
from typing import Dict, Optional, Tuple

import torch

from . import _hip


@dataclass(frozen=True)
class SampleGuidance:
    """Weights and shape of the potential (distances in Angstrom, as the coordinates).  ``clash`` / ``bond``: the weights (>= 0; both 0
    still runs the guidance kernel and is bitwise the unguided sample).  ``clash_distance``: d0 of the clash term, ``bond_length``: L of
    the bond term, ``max_shift``: the largest per-residue shift of one step (math.inf: no cap), ``t_max``: the steps t <= t_max are
    guided (None: every step, T)."""
    clash: float = 0.0
    bond: float = 0.0
    clash_distance: float = 3.8
    bond_length: float = 3.8
    max_shift: float = 1.0
    t_max: Optional[int] = None


def _real(v) -> bool:
    return isinstance(v, (int, float)) and not isinstance(v, bool)


def check_guidance(who: str, guidance, T: Optional[int]) -> SampleGuidance:
    """`guidance` after every check made before device work (ValueError); T None: t_max is not checked (structure_energy)."""
    if not isinstance(guidance, SampleGuidance):
        raise ValueError(f"{who}: guidance must be a guidance.SampleGuidance, got {type(guidance).__name__}")
    g = guidance
    for name in ("clash", "bond"):
        v = getattr(g, name)
        if not _real(v) or not math.isfinite(v) or v < 0:
            raise ValueError(f"{who}: guidance {name} weight must be a finite number >= 0, got {v!r}")
    for name in ("clash_distance", "bond_length"):
        v = getattr(g, name)
        if not _real(v) or not math.isfinite(v) or v <= 0:
            raise ValueError(f"{who}: guidance {name} must be a finite number > 0, got {v!r}")
    if not _real(g.max_shift) or math.isnan(g.max_shift) or g.max_shift <= 0:
        raise ValueError(f"{who}: guidance max_shift must be > 0 (math.inf: no cap), got {g.max_shift!r}")
    if T is not None and g.t_max is not None:
        if isinstance(g.t_max, bool) or not isinstance(g.t_max, int) or not 0 <= g.t_max <= T:
            raise ValueError(f"{who}: guidance t_max must be None or an int in [0, T = {T}], got {g.t_max!r}")
    return g


def residue_tables(who: str, chain_idx, residue_idx, residue_mask, n_rows: int, K: int) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """Host (n_rows, K) int32 chain, int32 residue_idx and bool residue_mask from the optional (K,) / (rows, K) inputs: one chain,
    arange(K) and all true by default; ValueError for a non-integer dtype, a value outside int32 or a shape that does not broadcast."""
    out = []
    for name, v, default in (("chain_idx", chain_idx, lambda: torch.zeros(K, dtype=torch.int64)),
                             ("residue_idx", residue_idx, lambda: torch.arange(K, dtype=torch.int64)),
                             ("residue_mask", residue_mask, lambda: torch.ones(K, dtype=torch.bool))):
        t = default() if v is None else torch.as_tensor(v).detach().cpu()
        if t.is_floating_point() or t.is_complex() or (name != "residue_mask" and t.dtype == torch.bool):
            raise ValueError(f"{who}: needs an integer {name}" + (" (or bool)" if name == "residue_mask" else "") + f", got {t.dtype}")
        if t.dim() not in (1, 2):
            raise ValueError(f"{who}: {name} must be (K,) or (rows, K), got {tuple(t.shape)}")
        try:
            t = t.expand(n_rows, K)
        except RuntimeError:
            raise ValueError(f"{who}: {name} {tuple(t.shape)} does not broadcast to the rows ({n_rows}, {K})") from None
        if name == "residue_mask":
            t = t.ne(0)
        else:
            if t.numel() and (int(t.min()) < -2 ** 31 or int(t.max()) >= 2 ** 31):
                raise ValueError(f"{who}: {name} values must fit in int32")
            t = t.to(torch.int32)
        out.append(t.contiguous())
    return out[0], out[1], out[2]


def c_struct(g: SampleGuidance, t_max: int, chain: torch.Tensor, residue_idx: torch.Tensor, residue_mask: Optional[torch.Tensor],
             shift: Optional[torch.Tensor]) -> "_hip.SampleGuidance":
    """diffab_sample_guidance over device tensors (the caller keeps them alive until the call is enqueued)."""
    return _hip.SampleGuidance(float(g.clash), float(g.clash_distance), float(g.bond), float(g.bond_length), float(g.max_shift), int(t_max),
                               _hip.ptr(chain), _hip.ptr(residue_idx), _hip.ptr(residue_mask), _hip.ptr(shift))


@torch.no_grad()
def structure_energy(translations: torch.Tensor, generation_mask: torch.Tensor, *, chain_idx=None, residue_idx=None, residue_mask=None,
                     guidance: Optional[SampleGuidance] = None, return_grad: bool = False) -> Dict[str, torch.Tensor]:
    """The guidance potential at the given CA translations (B, K, 3) (or (K, 3)), on the device (`diffab_guidance_energy`).

    Pairs {i, j}, i != j, with residue_mask set on both and generation_mask on at least one; bonded when chain_idx is equal and
    residue_idx differs by exactly 1.  chain_idx / residue_idx / residue_mask are (K,) or (B, K) (defaults: one chain, arange(K), all
    true).  Returns, per row (B,): ``clash`` = sum_nonbonded max(0, d0 - d)^2 and ``bond`` = sum_bonded (d - L)^2 (UNWEIGHTED),
    ``n_clash`` (int64) the nonbonded pairs with d < d0, ``max_bond_deviation`` the largest |d - L| over bonded pairs (0 without one);
    with ``return_grad`` also ``grad`` (B, K, 3), the WEIGHTED gradient dU/dx of the generated residues (0 elsewhere; pairs closer than
    1e-6 contribute none).  d0, L and the weights come from ``guidance`` (default SampleGuidance(clash=1.0, bond=1.0)).  Each row is
    reduced in a fixed order: its result does not depend on the other rows.  Results are on the input's device."""
    g = check_guidance("structure_energy()", SampleGuidance(clash=1.0, bond=1.0) if guidance is None else guidance, None)
    x = torch.as_tensor(translations)
    squeeze = x.dim() == 2
    if squeeze:
        x = x.unsqueeze(0)
    if x.dim() != 3 or x.shape[-1] != 3:
        raise ValueError(f"structure_energy(): translations must be (B, K, 3) or (K, 3), got {tuple(translations.shape)}")
    if not x.is_floating_point():
        raise ValueError(f"structure_energy(): translations must be floating point, got {x.dtype}")
    B, K = x.shape[0], x.shape[1]
    if K < 1:
        raise ValueError("structure_energy(): K = 0 residues")
    gm = torch.as_tensor(generation_mask)
    if gm.is_floating_point() or gm.is_complex():
        raise ValueError(f"structure_energy(): generation_mask must be bool, got {gm.dtype}")
    try:
        gm = gm.expand(B, K)
    except RuntimeError:
        raise ValueError(f"structure_energy(): generation_mask {tuple(gm.shape)} does not broadcast to ({B}, {K})") from None
    chain, ridx, rmask = residue_tables("structure_energy()", chain_idx, residue_idx, residue_mask, B, K)
    lib = _hip.lib()
    out_dev = x.device
    xd, gmd = _hip.dev_f32(x), _hip.dev_mask(gm)
    dev = xd.device
    chain, ridx, rmask = chain.to(dev), ridx.to(dev), rmask.to(dev)
    clash, bond, dmax = (torch.empty(B, device=dev) for _ in range(3))
    n_clash = torch.empty(B, dtype=torch.int32, device=dev)
    grad = torch.empty(B, K, 3, device=dev) if return_grad else None
    gs = c_struct(g, 0, chain, ridx, rmask, None)
    _hip.check(lib.diffab_guidance_energy(_hip.ptr(xd), _hip.ptr(gmd), C.byref(gs), B, K, _hip.ptr(clash), _hip.ptr(bond), _hip.ptr(n_clash),
                                          _hip.ptr(dmax), _hip.ptr(grad), _hip.stream_ptr()), "diffab_guidance_energy")
    out = {"clash": clash, "bond": bond, "n_clash": n_clash.to(torch.int64), "max_bond_deviation": dmax}
    if return_grad:
        out["grad"] = grad
    if squeeze:
        out = {k: v[0] for k, v in out.items()}
    return {k: v.to(out_dev) for k, v in out.items()}
