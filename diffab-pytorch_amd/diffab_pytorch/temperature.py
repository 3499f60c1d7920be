"""Noise scales and sequence temperature of the reverse sampler: how greedy the sampling is.

``SampleTemperature`` configures ``DiffAb.sample(temperature=...)``.  Per output row, the translation noise of every step is scaled by
``translation`` (lambda_x), the IGSO3 angle is drawn at sigma = ``rotation`` * sqrt(beta'_t) (lambda_O) and s_{t-1} is drawn from
p^(1/``sequence``) renormalised (tau; 0 is the argmax).  The update kernel applies all three (`diffab_sample_loop_ex`, option `temperature`); 1 is the
ordinary draw, bitwise.  The posterior, x0_hat / O0_hat, the trajectory record, the initial state, optimize_from's forward noise and
``DiffAb.score`` are untouched.
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import List, Optional, Tuple, Union

import torch

Value = Union[float, int, torch.Tensor]

MAX_ROTATION_SCALES = 16  # distinct nonzero lambda_O of one call: one IGSO3 table of T + 1 rows each


@dataclass(frozen=True)
class SampleTemperature:
    """``translation`` (lambda_x), ``rotation`` (lambda_O) and ``sequence`` (tau): each a number or a 1-D tensor with one entry per output
    row (B * num_samples rows, row b * N + r; one per state row with context_index), every value finite and >= 0.  0 removes the noise
    of that modality (tau = 0: the argmax of the distribution drawn from); the defaults, 1, are the untempered sample."""
    translation: Value = 1.0
    rotation: Value = 1.0
    sequence: Value = 1.0


_FIELDS = ("translation", "rotation", "sequence")


def _row_values(who: str, name: str, v, n_rows: int) -> torch.Tensor:
    """One field as a host fp32 (n_rows,) tensor; ValueError for a type, a shape or a value outside the rule."""
    if isinstance(v, torch.Tensor):
        t = v.detach().cpu()
        if t.dtype == torch.bool or t.is_complex():
            raise ValueError(f"{who}: temperature {name} must be real numbers, got {t.dtype}")
        if t.dim() > 1:
            raise ValueError(f"{who}: temperature {name} must be a number or a 1-D tensor (one entry per output row), got "
                             f"{tuple(t.shape)}")
        t = t.double()
    elif isinstance(v, (int, float)) and not isinstance(v, bool):
        t = torch.tensor(float(v), dtype=torch.float64)
    else:
        raise ValueError(f"{who}: temperature {name} must be a number or a 1-D tensor, got {type(v).__name__}")
    try:
        t = t.expand(n_rows)
    except RuntimeError:
        raise ValueError(f"{who}: temperature {name} {tuple(t.shape)} does not broadcast to the {n_rows} output rows") from None
    if t.numel() and not bool(torch.isfinite(t).all()):
        raise ValueError(f"{who}: temperature {name} values must be finite")
    if t.numel() and bool((t < 0).any()):
        raise ValueError(f"{who}: temperature {name} values must be >= 0, got {float(t.min())}")
    f = t.float().contiguous()
    if f.numel() and not bool(torch.isfinite(f).all()):
        raise ValueError(f"{who}: temperature {name} values must be finite in fp32")
    return f


def row_values(who: str, temperature, n_rows: int) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """(lambda_x, lambda_O, tau), each a host fp32 (n_rows,) tensor, after every check made before device work (ValueError): the type,
    broadcasting, finite and >= 0 values, at most MAX_ROTATION_SCALES distinct nonzero rotation scales."""
    if not isinstance(temperature, SampleTemperature):
        raise ValueError(f"{who}: temperature must be a temperature.SampleTemperature, got {type(temperature).__name__}")
    out = tuple(_row_values(who, name, getattr(temperature, name), n_rows) for name in _FIELDS)
    scales = rotation_scales(out[1])
    if len(scales) > MAX_ROTATION_SCALES:
        raise ValueError(f"{who}: {len(scales)} distinct rotation scales; at most {MAX_ROTATION_SCALES} per call (one IGSO3 table each)")
    return out


def check_mode(who: str, values: Tuple[torch.Tensor, torch.Tensor, torch.Tensor], keep_structure: bool, keep_sequence: bool) -> None:
    """A structure scale != 1 with the structure kept (mode="fixed_backbone"), a sequence temperature != 1 with the sequence kept
    (mode="structure"): ValueError."""
    lx, lo, tau = values
    if keep_structure and (bool((lx != 1).any()) or bool((lo != 1).any())):
        raise ValueError(f"{who}: translation / rotation scales act on the structure, which mode='fixed_backbone' keeps as given")
    if keep_sequence and bool((tau != 1).any()):
        raise ValueError(f"{who}: a sequence temperature acts on the sequence, which mode='structure' keeps as given")


def rotation_scales(rot: torch.Tensor) -> Tuple[float, ...]:
    """The distinct nonzero rotation scales (fp32 values as Python floats), increasing: the sigma lists of the stacked reverse table."""
    return tuple(sorted({float(v) for v in rot.tolist() if v != 0.0}))


def rotation_rows(rot: torch.Tensor, scales: Tuple[float, ...], T: int) -> torch.Tensor:
    """int32 (rows,): the stacked-table row of t = 0 for every row, k (T + 1) for the k-th scale of `scales`; 0 for lambda_O = 0 (never read)."""
    where = {s: k for k, s in enumerate(scales)}
    return torch.tensor([where[float(v)] * (T + 1) if v != 0.0 else 0 for v in rot.tolist()], dtype=torch.int32)


def stacked_sigmas(base: torch.Tensor, scales: Tuple[float, ...]) -> torch.Tensor:
    """The sigma lists of the stacked reverse table, concatenated: lambda_k sqrt(beta') (T + 1 entries each), the product in fp32.
    ``base`` is sqrt(beta') (T + 1,) fp32; a row equal to 1 * base is base itself."""
    base = base.float()
    return torch.cat([base * torch.tensor(s, dtype=torch.float32) for s in scales])


def tempered_draw(p, u: float, tau: float, allowed: Optional[List[bool]] = None) -> int:
    """Host float64 restatement of the tempered draw (categorical_draw_tempered): p^(1/tau) over the allowed classes, scanned in
    increasing v against u * total; tau = 0 the argmax (lowest index on ties); every allowed class at 0: unit weights.  -1: none allowed.
    (tau = 1 on the device is categorical_draw / categorical_draw_allowed, which this also describes up to rounding.)"""
    p = [float(v) for v in p]
    ok = [True] * len(p) if allowed is None else [bool(a) for a in allowed]
    idx = [v for v in range(len(p)) if ok[v]]
    if not idx:
        return -1
    pmax = max(p[v] for v in idx)
    if not pmax > 0.0:
        w = {v: 1.0 for v in idx}
    elif tau == 0.0:
        return min(v for v in idx if p[v] == pmax)
    else:
        lm = math.log(pmax)
        w = {v: (math.exp((math.log(p[v]) - lm) / tau) if p[v] > 0.0 else 0.0) for v in idx}
    thr = u * sum(w.values())
    acc = 0.0
    for v in idx:
        acc += w[v]
        if acc > thr:
            return v
    return idx[-1]
