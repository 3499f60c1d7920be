"""One reverse step t -> s of the sampler with its options combined, restated in float64 (DESIGN sections 4.9 - 4.11 and 4.14).

Not a test module and not a conftest (like sampler_support.py): tests/test_reverse_step_composed_host.py pins `reverse_step_ref` on the
CPU against every single-option restatement the suite already has and against orc.reverse_update, and
tests/test_gpu_reverse_step_composed.py compares the update kernel with it.  It is assembled from those restatements and adds only the
order in which the options meet:

  1. record   - the predictions (x0_hat, O0_hat, the head posterior) are the model's own: no option changes them, so they are inputs;
  2. structure - the steering energy U at x0_hat, then Delta = beta' dU/dp (capped) off the mean, then the noise lambda_x sqrt(beta') z,
                 and the angle from the row's own table over lambda_O sqrt(beta'), about the unscaled axis, both only when s > 0;
  3. sequence - posterior -> jump distribution (s < t - 1; stored as fp32, as the kernel overwrites the posterior in place) -> allowed
                 classes -> temperature -> draw, all against the one STREAM_SEQ uniform of step t;
  4. steering - after the update, the rows of a group take the generated residues of their ancestors.

The denoiser is not evaluated here: eps_hat never appears, because the translations are stated as a difference to the options-off step
(the jump alone), in which the mean cancels.
"""
import numpy as np
import torch

import diffab_oracle as orc
from diffab_pytorch.steering import resample_oracle
from diffab_pytorch.temperature import tempered_draw
from sampler_support import step_noise
from test_guidance_host import guidance_ref, shift_ref
from test_respaced_host import seq_jump_ref

STREAM_STEER = 11  # csrc/philox.h
SIGMA_THRESHOLD = 0.1  # below it the angle comes from the histogram's inverse CDF, from it on from the Gaussian rule (so3.py:118-125)


def draw_edges(p, tau, ok=None):
    """The cumulative edges (float64, increasing, the last one 1) of what tempered_draw(p, u, tau, ok) scans against u, or None where
    the draw does not depend on u (no class allowed, one class allowed, tau = 0 with a positive probability)."""
    p = np.asarray(p, np.float64)
    idx = np.arange(p.size) if ok is None else np.flatnonzero(np.asarray(ok, bool))
    if idx.size <= 1:
        return None
    q = p[idx]
    if not q.max() > 0.0:
        w = np.ones(idx.size)
    elif tau == 0.0:
        return None
    else:
        with np.errstate(divide="ignore"):
            w = np.where(q > 0.0, np.exp((np.log(q) - np.log(q.max())) / tau), 0.0)
    return np.cumsum(w) / w.sum()


def reverse_step_ref(t, s, seq, x0_hat, O0_hat, post, gm, sched, beta_j, alpha_j, seed, first_patch, *, trans_scale=None, rot_scale=None,
                     seq_temp=None, rot_cdf=None, allowed=None, guidance=None, tables=None, steering=None, group_size=1):
    """The step t -> s of B state rows, from the state's tokens `seq` (B, K), the recorded predictions x0_hat (B, K, 3), O0_hat
    (B, K, 3, 3) and post (B, K, V), and the generation mask gm (B, K).

    sched: the model's schedule (fp32 tensors alpha / beta / alpha_bar); beta_j, alpha_j: the jump's beta'_t / alpha'_t (fp32 values;
    the schedule's own beta[t] / alpha[t] at s = t - 1).  trans_scale / rot_scale / seq_temp: (B,) per-row lambda_x, lambda_O, tau
    (None: 1).  rot_cdf: {lambda_O: (n_bins,) fp32 CDF row of a table over lambda_O sqrt(beta'_t)}, one entry per distinct nonzero scale
    (None: scale 1 only, Gaussian branch or s = 0).  allowed: (B, K, V) bool (None: every class).  guidance: a SampleGuidance with
    tables = (chain, residue_idx, residue_mask), each (B, K).  steering: a ParticleSteering (the step is taken to be a steering step;
    log-weights and last energies start at 0) over groups of `group_size` rows, same tables.

    Returns a dict of numpy arrays (float64 unless said):
      seq (B, K) int64   the token after the step: the class drawn, the old token where no class is allowed or nothing is generated
      edge (B, K)        |u - nearest cumulative edge| of what the class was drawn from (inf where the draw does not depend on u)
      drawn (B, K) bool  generated residues with at least one allowed class
      probs (B, K, V)    the distribution the draw starts from: the posterior, or the jump distribution
      dx (B, K, 3)       x_s minus x_s of the step with the jump alone: -Delta + (lambda_x - 1) sqrt(beta') z, -Delta at s = 0
      delta (B, K, 3)    Delta (0 without guidance)
      noise (B, K, 3)    lambda_x sqrt(beta') z, the noise term of x_s itself (0 at s = 0 and on lambda_x = 0 rows)
      theta (B, K), axis (B, K, 3), rotvec (B, K, 3)   the rotation about O0_hat (theta = 0 at s = 0 and on lambda_O = 0 rows)
      hist (B,) bool     rows whose angle is the histogram's (sigma < 0.1); sigma (B,) the row's lambda_O sqrt(beta'_t), fp32 product
      O (B, K, 3, 3)     O0_hat exp(hat(rotvec)) on generated residues, float64
      energy (B,), ancestors (B,) int64 (global rows), resampled / margin (groups,)   with steering only; seq, dx, rotvec, theta, axis
                         and O are then the gathered ones (row r holds the generated residues of row ancestors[r])."""
    seq = np.asarray(seq, np.int64)
    gm = np.asarray(gm, bool)
    B, K = seq.shape
    post = np.asarray(post, np.float64)
    V = post.shape[-1]
    x0 = np.asarray(x0_hat, np.float64)
    ones = np.ones(B, np.float32)
    lx, lo, tau = (ones if v is None else np.asarray(v, np.float32) for v in (trans_scale, rot_scale, seq_temp))
    noisy = s > 0
    sb = torch.tensor(float(beta_j), dtype=torch.float32).sqrt()  # sqrt(beta'_t), fp32 as the table's sigma list is built

    # ---- the Philox lanes of step t; one igso3 draw per distinct rotation scale, each from its own table row
    flat = (torch.arange(1, 9) / 8.0).float()  # (a stand-in row where no table is read)
    z, _, us = step_noise(seed, first_patch, B, K, t, flat, torch.tensor(1.0))
    z, us = z.double().numpy(), us.double().numpy()
    sigma = np.zeros(B, np.float32)
    rotvec = np.zeros((B, K, 3))
    for lam in sorted({float(v) for v in lo if v != 0.0}):
        sg = sb * torch.tensor(lam, dtype=torch.float32)
        hist = bool(sg < SIGMA_THRESHOLD)
        if hist and noisy and (rot_cdf is None or lam not in rot_cdf):
            raise ValueError(f"reverse_step_ref: sigma = {float(sg)} < {SIGMA_THRESHOLD} needs the table row of rotation scale {lam}")
        row = rot_cdf[lam].float().cpu() if hist and noisy else flat
        _, rv, _ = step_noise(seed, first_patch, B, K, t, row, sg)
        rows = np.flatnonzero(lo == np.float32(lam))
        rotvec[rows] = rv.double().numpy()[rows]
        sigma[rows] = float(sg)
    if not noisy:
        rotvec[:] = 0.0
    theta = np.sqrt((rotvec ** 2).sum(-1))
    axis = rotvec / np.where(theta > 0, theta, 1.0)[..., None]

    # ---- structure: Delta at x0_hat with the jump's beta', not scaled by lambda_x; then the scaled noise
    delta = np.zeros((B, K, 3))
    if guidance is not None and t <= (np.inf if guidance.t_max is None else guidance.t_max):
        chain, ridx, rmask = (np.asarray(v) for v in tables)
        g = guidance_ref(x0, gm, chain, ridx, rmask, guidance.clash, guidance.clash_distance, guidance.bond, guidance.bond_length)["grad"]
        delta = shift_ref(g, float(beta_j), guidance.max_shift)
    sbz = float(sb) * z
    noise = lx.astype(np.float64)[:, None, None] * sbz if noisy else np.zeros_like(sbz)
    dx = (-delta + (noise - (sbz if noisy else 0.0))) * gm[..., None]  # (the noise difference first: exactly 0 at lambda_x = 1)
    O0 = np.asarray(O0_hat, np.float64)
    turned = gm & (theta > 0)  # (the oracle's Rodrigues form is NaN at the zero vector: no rotation is O0_hat itself, exactly)
    safe = np.where(turned[..., None], rotvec, [1.0, 0.0, 0.0])
    O = np.where(turned[..., None, None], O0 @ orc.rotvec_to_matrix(torch.from_numpy(safe)).numpy(), O0)

    # ---- sequence: posterior -> jump -> allowed -> temperature -> draw
    probs = post
    if s < t - 1:
        f = lambda name, i: float(sched[name][i])
        r = seq_jump_ref(post, seq, f("alpha", t), f("beta", t), f("alpha_bar", t - 1), float(alpha_j), f("alpha_bar", s), V=V)
        probs = r.astype(np.float32).astype(np.float64)
    new, edge, drawn = seq.copy(), np.full((B, K), np.inf), np.zeros((B, K), bool)
    for b, k in zip(*np.nonzero(gm)):
        ok = None if allowed is None else np.asarray(allowed[b, k], bool).tolist()
        cls = tempered_draw(probs[b, k], float(us[b, k]), float(tau[b]), ok)
        if cls < 0:
            continue
        new[b, k], drawn[b, k] = cls, True
        edges = draw_edges(probs[b, k], float(tau[b]), ok)
        if edges is not None:
            edge[b, k] = np.abs(edges - us[b, k]).min()
    out = {"seq": new, "edge": edge, "drawn": drawn, "probs": probs, "dx": dx, "delta": delta, "noise": noise * gm[..., None],
           "theta": theta * gm, "axis": axis * gm[..., None], "rotvec": rotvec * gm[..., None], "O": O,
           "hist": (sigma < SIGMA_THRESHOLD) & (lo != 0), "sigma": sigma.astype(np.float64)}

    # ---- steering: the energy at x0_hat (before Delta; no temperature), one uniform per group, then the gather
    if steering is not None:
        chain, ridx, rmask = (np.asarray(v) for v in tables)
        e = guidance_ref(x0, gm, chain, ridx, rmask, steering.clash, steering.clash_distance, steering.bond, steering.bond_length)
        U = steering.clash * e["clash"] + steering.bond * e["bond"]
        first = first_patch + np.arange(0, B, group_size)
        u = orc.philox_uniform4(seed, first, np.zeros_like(first), t, STREAM_STEER)[0]
        zero = np.zeros(B, np.float32)
        rs = resample_oracle(zero, zero, U.astype(np.float32), u, group_size, steering.strength, steering.ess_threshold)
        anc = rs["ancestors"].astype(np.int64) + np.arange(B) // group_size * group_size
        m = gm
        for k in ("seq", "dx", "theta", "axis", "rotvec", "O"):
            v = out[k]
            out[k] = np.where(m.reshape(m.shape + (1,) * (v.ndim - 2)), v[anc], v)
        out.update(energy=U, ancestors=anc, resampled=rs["resampled"], margin=rs["margin"], log_weight=rs["logw"], uniform=u)
    return out
