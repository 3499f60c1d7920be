"""Backbone refinement on the device: close the peptide bonds between the residue frames of finished designs.

``sample()`` returns one rigid frame per residue; N, CA, C inside a residue are ideal, between residues they are whatever the diffusion
left, and ``metrics.backbone`` reports the damage.  ``backbone`` mends it: a fixed number of Jacobi steps on a sum of pair-distance
terms - the peptide bond, the two angles at it as 1-3 distances, the trans CA - CA distance, a CA clash term and an optional tether to
the start - moves every generated residue as a rigid body (``diffab_refine_backbone``, ``csrc/refine_kernels.hip``: one launch, a
design resident in LDS for all iterations).  Model-free: nothing here needs a ``DiffAb``, and designs that were loaded, pasted, steered
or filtered are refined like fresh ones.  The rule is the comment of ``diffab_refine_backbone`` in ``include/diffab_hip.h``; there is
no torch fallback.
"""
from __future__ import annotations

import ctypes as C
import math
from dataclasses import dataclass
from typing import Dict, Optional

import torch

from . import _hip
from .guidance import residue_tables
from .metrics import _check_common

MAX_K = 256  # DIFFAB_REFINE_MAX_K
MAX_ITERATIONS = 100000  # DIFFAB_REFINE_MAX_ITERATIONS
MAX_STEP_WEIGHT = 0.1000001  # DIFFAB_REFINE_MAX_STEP_WEIGHT: step x the largest weight
TERMS = ("bond", "angle", "trans", "clash", "tether")  # the columns of ``terms``


def _f32(v: float) -> float:
    return C.c_float(v).value


@dataclass(frozen=True)
class Refinement:
    """The options of ``backbone`` (distances in Angstrom).  ``iterations`` Jacobi steps of size ``step``; ``bond``, ``angle``,
    ``trans``, ``clash``, ``tether``: the weights of the five terms (>= 0; all 0 returns the input's bits); ``clash_distance``: below it
    two CA that are no chain neighbours repel.  ``step`` times the largest weight may not exceed 0.1: beyond it the iteration is not
    stable.  Checked on construction (ValueError)."""
    iterations: int = 200
    step: float = 0.05
    bond: float = 1.0
    angle: float = 1.0
    trans: float = 1.0
    clash: float = 1.0
    tether: float = 0.0
    clash_distance: float = 3.8

    def __post_init__(self):
        who = "refine.Refinement"
        if isinstance(self.iterations, bool) or not isinstance(self.iterations, int) or not 0 <= self.iterations <= MAX_ITERATIONS:
            raise ValueError(f"{who}: iterations must be an int in [0, {MAX_ITERATIONS}], got {self.iterations!r}")
        for name in ("step", "clash_distance"):
            v = getattr(self, name)
            if isinstance(v, bool) or not isinstance(v, (int, float)) or not math.isfinite(v) or v <= 0:
                raise ValueError(f"{who}: {name} must be a finite number > 0, got {v!r}")
        for name in TERMS:
            v = getattr(self, name)
            if isinstance(v, bool) or not isinstance(v, (int, float)) or not math.isfinite(v) or v < 0:
                raise ValueError(f"{who}: {name} weight must be a finite number >= 0, got {v!r}")
        heaviest = max(_f32(getattr(self, name)) for name in TERMS)
        if _f32(self.step) * heaviest > MAX_STEP_WEIGHT:  # (the library's own test: the product in double of the fp32 values)
            raise ValueError(f"{who}: step x largest weight = {self.step!r} x {heaviest!r} is above 0.1: the iteration is not stable there")

    def c_struct(self) -> "_hip.RefineOptions":
        return _hip.RefineOptions(int(self.iterations), float(self.step), float(self.bond), float(self.angle), float(self.trans),
                                  float(self.clash), float(self.tether), float(self.clash_distance))


def workspace_bytes(G: int, K: int) -> int:
    """DIFFAB_REFINE_WORKSPACE_BYTES of include/diffab_hip.h."""
    return G * K * 8 + 1024


@torch.no_grad()
def backbone(designs: Dict[str, torch.Tensor], generation_mask: torch.Tensor, *, chain_idx=None, residue_idx=None,
             residue_mask: Optional[torch.Tensor] = None, group_size: int = 1, options: Optional[Refinement] = None) -> Dict[str, torch.Tensor]:
    """Refine the frames of ``designs`` - the dict ``sample()`` returns, rows = G * ``group_size``, row g * group_size + r = design r of
    patch g - with the masks per patch (G,K) as in ``metrics``.  A residue moves when it is generated and inside ``residue_mask``; every
    other residue comes back bitwise and still exerts forces.  Chain neighbours by ``metrics.backbone``'s rule (``chain_idx`` /
    ``residue_idx`` (K,) or (G,K), default one chain and ``arange(K)``).  ``options``: a ``Refinement`` (default ``Refinement()``).

    Returns ``seq_idx`` (the same tensor), ``translations`` (rows,K,3), ``orientations`` (rows,K,3,3), ``energy_before`` /
    ``energy_after`` (rows,), ``terms`` (rows,5) - bond, angle, trans, clash, tether of the result - and ``max_shift`` (rows,), the
    largest CA displacement; the result feeds ``metrics.*``, ``patch.paste`` and ``io.write_pdb`` as ``sample()``'s dict does.  One
    C-ABI call; K <= 256; results on the device of ``designs['seq_idx']``; ValueError naming the argument before any device work."""
    who = "refine.backbone()"
    rows, G, K = _check_common(who, designs, generation_mask, residue_mask, group_size, "backbone")
    if K > MAX_K:
        raise ValueError(f"{who}: K = {K} residues per patch, at most {MAX_K}")
    if options is None:
        options = Refinement()
    if not isinstance(options, Refinement):
        raise ValueError(f"{who}: options must be a refine.Refinement, got {type(options).__name__}")
    chain, ridx, _ = residue_tables(who, chain_idx, residue_idx, None, G, K)
    lib = _hip.lib()
    dev, out_dev = _hip.device(), designs["seq_idx"].device
    x, O = _hip.dev_f32(designs["translations"]), _hip.dev_f32(designs["orientations"])
    gm = _hip.dev_mask(generation_mask)
    rm = None if residue_mask is None else _hip.dev_mask(residue_mask)
    chain, ridx = chain.to(dev), ridx.to(dev)
    x_out, O_out = torch.empty_like(x), torch.empty_like(O)
    before, after, shift = (torch.empty(rows, dtype=torch.float32, device=dev) for _ in range(3))
    terms = torch.empty(rows, len(TERMS), dtype=torch.float32, device=dev)
    nbytes = workspace_bytes(G, K)
    ws = _hip.workspace(nbytes)
    opt = options.c_struct()
    _hip.check(lib.diffab_refine_backbone(_hip.ptr(x), _hip.ptr(O), _hip.ptr(gm), _hip.ptr(rm), _hip.ptr(chain), _hip.ptr(ridx), rows,
                                          group_size, K, C.byref(opt), _hip.ptr(x_out), _hip.ptr(O_out), _hip.ptr(before), _hip.ptr(after),
                                          _hip.ptr(terms), _hip.ptr(shift), _hip.ptr(ws), nbytes, _hip.stream_ptr()), "diffab_refine_backbone")
    out = {"translations": x_out.to(designs["translations"].dtype), "orientations": O_out.to(designs["orientations"].dtype),
           "energy_before": before, "energy_after": after, "terms": terms, "max_shift": shift}
    out = {k: v.to(out_dev) for k, v in out.items()}
    out["seq_idx"] = designs["seq_idx"]
    return out
