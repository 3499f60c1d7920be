"""Particle steering of the reverse sampler: the designs of a patch resampled by energy while they form.

``ParticleSteering`` configures ``DiffAb.sample(steering=...)``.  The rows of a group (the ``num_samples`` designs of a patch) are the
particles of a sequential Monte Carlo run over the reverse process.  At every steering step each row is weighted by

    U = clash * sum_nonbonded max(0, clash_distance - d)^2 + bond * sum_bonded (d - bond_length)^2

taken at the model's clean-structure prediction x0_hat (the potential of guidance.py), log w += -strength (U - U_previous); when the
effective sample size of a group falls below ess_threshold N the group is resampled systematically and the generated residues of every
row are replaced by those of its ancestor, all on the device (`diffab_sample_loop_ex`, option `steering`).  ``resample_oracle`` restates the weight
and resampling rule in numpy float64 for the tests; it is not a fallback.
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Dict, List, Optional, Sequence

import numpy as np
import torch

from . import _hip

MAX_GROUP = 1024  # DIFFAB_STEER_MAX_GROUP


@dataclass(frozen=True)
class ParticleSteering:
    """``strength``: lambda >= 0 of the weights.  ``clash`` / ``bond`` / ``clash_distance`` / ``bond_length``: the potential, as
    guidance.SampleGuidance.  ``ess_threshold`` in [0, 2]: a group resamples when ESS < ess_threshold N (0: never, above 1: always).
    Steering steps are the executed steps t with t_min <= t <= t_max (None: the first step of the call) and (t_max - t) % every == 0,
    the last executed step excepted.  ``group_size``: rows per group (None: num_samples)."""
    strength: float = 1.0
    clash: float = 1.0
    bond: float = 1.0
    clash_distance: float = 3.8
    bond_length: float = 3.8
    ess_threshold: float = 0.5
    every: int = 1
    t_min: int = 0
    t_max: Optional[int] = None
    group_size: Optional[int] = None


def _real(v) -> bool:
    return isinstance(v, (int, float)) and not isinstance(v, bool)


def _int(v) -> bool:
    return isinstance(v, int) and not isinstance(v, bool)


def check_steering(who: str, steering, T: int) -> ParticleSteering:
    """`steering` after every check made before device work (ValueError)."""
    if not isinstance(steering, ParticleSteering):
        raise ValueError(f"{who}: steering must be a steering.ParticleSteering, got {type(steering).__name__}")
    s = steering
    for name in ("strength", "clash", "bond"):
        v = getattr(s, name)
        if not _real(v) or not math.isfinite(v) or v < 0:
            raise ValueError(f"{who}: steering {name} must be a finite number >= 0, got {v!r}")
    for name in ("clash_distance", "bond_length"):
        v = getattr(s, name)
        if not _real(v) or not math.isfinite(v) or v <= 0:
            raise ValueError(f"{who}: steering {name} must be a finite number > 0, got {v!r}")
    if not _real(s.ess_threshold) or not 0 <= s.ess_threshold <= 2:
        raise ValueError(f"{who}: steering ess_threshold must lie in [0, 2], got {s.ess_threshold!r}")
    if not _int(s.every) or s.every < 1:
        raise ValueError(f"{who}: steering every must be an int >= 1, got {s.every!r}")
    if not _int(s.t_min) or not 0 <= s.t_min <= T:
        raise ValueError(f"{who}: steering t_min must be an int in [0, T = {T}], got {s.t_min!r}")
    if s.t_max is not None and (not _int(s.t_max) or not s.t_min <= s.t_max <= T):
        raise ValueError(f"{who}: steering t_max must be None or an int in [t_min = {s.t_min}, T = {T}], got {s.t_max!r}")
    if s.group_size is not None and (not _int(s.group_size) or not 1 <= s.group_size <= MAX_GROUP):
        raise ValueError(f"{who}: steering group_size must be None or an int in [1, {MAX_GROUP}], got {s.group_size!r}")
    return s


def check_groups(who: str, group_size: int, n_rows: int, fields: Dict[str, Optional[torch.Tensor]]) -> None:
    """The rows are whole groups of `group_size`, and every field (host tensors with the state rows outermost; None: skipped) is the
    same on all rows of a group (ValueError)."""
    if not 1 <= group_size <= MAX_GROUP:
        raise ValueError(f"{who}: steering group_size = {group_size} outside [1, {MAX_GROUP}]")
    if n_rows % group_size:
        raise ValueError(f"{who}: {n_rows} state rows are not a multiple of the steering group_size = {group_size} (a shard must hold "
                         "whole groups)")
    for name, v in fields.items():
        if v is None or group_size == 1:
            continue
        g = v.reshape(n_rows // group_size, group_size, -1)
        if not bool((g == g[:, :1]).all()):
            bad = int((g != g[:, :1]).flatten(1).any(1).nonzero()[0])
            raise ValueError(f"{who}: steering needs {name} to be the same on all rows of a group; group {bad} (rows {bad * group_size} .. "
                             f"{bad * group_size + group_size - 1}) differs")


def steering_steps(executed: Sequence[int], t_stop: int, t_min: int, t_max: int, every: int) -> List[int]:
    """The steering steps of a run over `executed` (descending), descending: the predicate the kernels evaluate."""
    out = []
    for j, t in enumerate(executed):
        succ = executed[j + 1] if j + 1 < len(executed) else t_stop
        if t_min <= t <= t_max and (t_max - t) % every == 0 and succ > t_stop:
            out.append(int(t))
    return out


def c_struct(s: ParticleSteering, t_max: int, group_size: int, chain: torch.Tensor, residue_idx: torch.Tensor,
             residue_mask: Optional[torch.Tensor], logw: Optional[torch.Tensor], u_prev: Optional[torch.Tensor],
             energy: Optional[torch.Tensor], ancestors: Optional[torch.Tensor], scratch: Optional[torch.Tensor]) -> "_hip.SampleSteering":
    """diffab_sample_steering over device tensors (the caller keeps them alive until the call is enqueued)."""
    return _hip.SampleSteering(float(s.clash), float(s.clash_distance), float(s.bond), float(s.bond_length), float(s.strength),
                               float(s.ess_threshold), int(s.t_min), int(t_max), int(s.every), int(group_size), _hip.ptr(chain),
                               _hip.ptr(residue_idx), _hip.ptr(residue_mask), _hip.ptr(logw), _hip.ptr(u_prev), _hip.ptr(energy),
                               _hip.ptr(ancestors), _hip.ptr(scratch))


def scratch_bytes(rows: int, K: int) -> int:
    return rows * K * 56 + rows * 4  # DIFFAB_STEER_SCRATCH_BYTES


def lineage(ancestors: torch.Tensor) -> torch.Tensor:
    """(n, rows) global ancestor maps in execution order -> (rows,) the initial row every final row descends from."""
    n, rows = ancestors.shape
    lin = torch.arange(rows, dtype=torch.int64, device=ancestors.device)
    for j in range(n - 1, -1, -1):  # final row r <- a_n[r] <- a_{n-1}[a_n[r]] ...
        lin = ancestors[j].to(torch.int64)[lin]
    return lin


def resample_oracle(logw, u_prev, energy, u, N: int, strength: float, ess_threshold: float) -> Dict[str, np.ndarray]:
    """The weight and resampling rule of one steering step in numpy, for G groups of N rows.

    logw, u_prev, energy: (G * N,) float32 values; u: (G,) float32 uniforms in [0, 1).  The weight update is fp32 as on the device,
    everything after it float64.  Returns ``logw`` / ``u_prev`` (float32, after the step), ``ancestors`` (G * N,) indices inside the
    group, ``ess`` (G,) float64 (0 for a group without weight), ``resampled`` (G,) bool and ``margin`` (G,), the smallest distance of
    a position (u + j) / N to a cumulative boundary C_i (inf where the group does not resample): a draw decided by less than the
    float64 rounding of C may legitimately differ."""
    f32 = np.float32
    logw, u_prev, energy = (np.asarray(v, dtype=f32).reshape(-1, N) for v in (logw, u_prev, energy))
    u = np.asarray(u, dtype=f32).reshape(-1)
    G = logw.shape[0]
    with np.errstate(invalid="ignore", over="ignore"):
        lw = (logw + (-(f32(strength) * (energy - u_prev)))).astype(f32)
    out_lw, out_up = lw.copy(), energy.copy()
    anc = np.tile(np.arange(N, dtype=np.int32), (G, 1))
    ess = np.zeros(G)
    resampled = np.zeros(G, dtype=bool)
    margin = np.full(G, np.inf)
    thr = float(f32(ess_threshold))
    for g in range(G):
        fin = np.isfinite(lw[g])
        if not fin.any():
            out_lw[g] = 0
            continue
        m = float(lw[g][fin].max())
        w = np.where(fin, np.exp(np.where(fin, lw[g].astype(np.float64), m) - m), 0.0)
        S = float(w.sum())
        if not S > 0:
            out_lw[g] = 0
            continue
        ess[g] = S * S / float((w * w).sum())
        if not ess[g] < thr * N:
            continue
        resampled[g] = True
        C = np.cumsum(w) / S
        pos = (float(u[g]) + np.arange(N)) / N
        a = np.searchsorted(C, pos, side="right")  # the smallest i with C_i > pos
        last = int(np.flatnonzero(w > 0)[-1])
        a = np.minimum(a, last)
        anc[g] = a
        out_lw[g] = 0
        out_up[g] = energy[g][a]
        margin[g] = float(np.abs(pos[:, None] - C[None, :last + 1]).min())
    return {"logw": out_lw.reshape(-1), "u_prev": out_up.reshape(-1), "ancestors": anc.reshape(-1), "ess": ess, "resampled": resampled,
            "margin": margin}
