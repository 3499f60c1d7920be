"""The SO(3) kernels at rotation angles near 0 and pi, where every other test masks them out (`well_conditioned` in test_gpu_parity.py and
its copies: |cos theta -+ 1| < 1e-2 is dropped because the reference-made goldens are bad there).

Oracle: tests/so3_ref.py, float64 numpy, angle from atan2 and the axis near pi from the symmetric part (tests/test_so3_edges_host.py
checks it on the host).  Inputs (so3_ref.edge_inputs): 1024 fp32 rotations at each of 15 angles from 1e-8 to pi - 1e-6, once built from
axis-angle in float64 and rounded, once as an fp32 product A B C (off the rotation group by a few 1e-7); the exact identity; 512 exactly
symmetric half-turns.  The entries are called directly through the C ABI.

Bars, the same in every test:
  * nothing non-finite, for any input, the identity, zero vectors and exact half-turns included;
  * matrix outputs: geodesic(got, want) <= 1e-5 rad, the element-wise 1e-5 the suite holds these maps to outside the bands (the oracle
    moves by ~1e-7 under one fp32 rounding of the input in every band, so the bar leaves two decades), and orthogonal to atol 1e-5;
  * rotvec / skew outputs below theta = 3: |v - v_ref| <= 1e-5 |v_ref| + 2^-24 (the floor is one rounding of a matrix entry near 1;
    below theta ~ 1e-7 the floor is all that is left, so there only finiteness and the floor are tested);
  * rotvec / skew outputs at theta >= 3: exp of the output within 1e-5 rad of the input (v and v - 2 pi axis are the same rotation), and
    |v| <= pi + 1e-5;
  * R^k at an exact half-turn, k outside {0, 1}, has two values: either axis sign is accepted, on the rows where the oracle's w is exactly
    0 only (so3_ref.two_valued: the constructed symmetric matrices, under 2 % of the inputs);
  * exact limits: log(I) = 0, exp(0) = rotvec_to_matrix(0) = scale_rot(R, 0) = I, bitwise.
Every test prints its worst error per angle band before it asserts.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import diffab_oracle as orc
import so3_ref as ref
from diffab_pytorch import _hip, synthetic as syn
from sampler_support import STREAMS_OPT, hip, make_model, patches, sample, step_noise

pytestmark = pytest.mark.gpu
BAR = 1e-5          # rad, and the relative bar of the rotvec outputs
FLOOR = 2.0 ** -24  # one rounding of a matrix entry near 1
ORTH = 1e-5
KS = (0.0, 0.3, 0.999, 1.0)
P = _hip.ptr


@pytest.fixture(scope="module")
def case(hip):
    """The inputs and everything of the oracle that more than one test reads, computed once."""
    inp = ref.edge_inputs()
    Q = ref.project(inp["R"])
    v = ref.log(Q)
    # 128 rows for the (B, K) = (2, 64) entries: four of every band (the one identity four times), shuffled over both patches
    pick = np.concatenate([np.resize(np.flatnonzero(inp["band"] == b), 4) for b in range(len(inp["names"]))])
    assert len(pick) == 128
    pick = pick[np.random.default_rng(5).permutation(128)]
    return dict(inp, Q=Q, v=v, theta=np.linalg.norm(v, axis=-1), two=ref.two_valued(inp["R"]), pick=pick, hip=hip)


def dev(a, dtype=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(a)).to(dtype).cuda().contiguous()


def run(hip, name, ins, shape, *extra):
    """One elementwise entry: inputs, the output, `extra`, the stream."""
    out = torch.full(shape, float("nan"), device="cuda")
    held = [dev(a) for a in ins]
    _hip.check(getattr(hip, name)(*[P(t) for t in held], P(out), *extra, _hip.stream_ptr()), name)
    return out.cpu().numpy()


def worst(err):
    """max over a band; a non-finite entry is the worst there is."""
    return float(np.max(np.where(np.isfinite(err), err, np.inf))) if err.size else 0.0


def report(what, err, band, names, bar):
    """Print the worst error per band and return the names of the bands over `bar` (err and bar may be per-row arrays)."""
    bad, cells = [], []
    over = ~(err <= bar)
    for b, name in enumerate(names):
        sel = band == b
        if not sel.any():
            continue
        cells.append("%s %.1e%s" % (name, worst(err[sel]), "*" if over[sel].any() else ""))
        if over[sel].any():
            bad.append(name)
    print("%s: %s" % (what, ", ".join(cells)))
    return bad


def off_orthogonal(M):
    M = M.astype(np.float64)
    return np.abs(ref.T(M) @ M - np.eye(3)).max((-1, -2))


def matrix_errors(got, want, alt=None):
    """geodesic(got, want) per row, NaN where got is not finite; `alt` (or NaN rows of it) is the second value of a two-valued row."""
    got = got.astype(np.float64)
    with np.errstate(invalid="ignore"):
        err = ref.geodesic(got, want)
        if alt is not None:
            err = np.where(np.isnan(alt).any((-1, -2)), err, np.minimum(err, ref.geodesic(got, np.nan_to_num(alt))))
    return np.where(np.isfinite(got).all((-1, -2)), err, np.nan)


def rotvec_errors(v, case):
    """Per row (error, bar) of a rotvec output: |v - v_ref| against 1e-5 |v_ref| + 2^-24 below theta = 3; from theta = 3 the geodesic
    error of exp(v) against the input, and |v| - pi, both against 1e-5."""
    v = v.astype(np.float64)
    low = case["theta"] < 3
    with np.errstate(invalid="ignore"):
        err_low = np.linalg.norm(v - case["v"], axis=-1)
        err_high = np.maximum(ref.geodesic(ref.exp(np.nan_to_num(v)), case["Q"]), np.linalg.norm(v, axis=-1) - np.pi)
    err = np.where(low, err_low, err_high)
    err = np.where(np.isfinite(v).all(-1), err, np.nan)
    return err, np.where(low, BAR * case["theta"] + FLOOR, BAR)


# ------------------------------------------------------------------ the five maps
def test_log_and_matrix_to_rotvec(case):
    """diffab_so3_log and diffab_so3_matrix_to_rotvec on every input.  Below theta ~ 1e-7 (the 1e-8 bands and the product family's
    noise) the bar is its floor: only finiteness and one rounding are tested there."""
    hip, R, n = case["hip"], case["R"], len(case["R"])
    S = run(hip, "diffab_so3_log", [R], (n, 3, 3), n)
    v = run(hip, "diffab_so3_matrix_to_rotvec", [R], (n, 3), n)
    err, bar = rotvec_errors(v, case)
    bad = report("matrix_to_rotvec |dv| (theta < 3) / geodesic of exp(v) (theta >= 3)", err, case["band"], case["names"], bar)
    err_S, _ = rotvec_errors(ref.vee(S), case)
    bad += report("log, its vee likewise", err_S, case["band"], case["names"], bar)
    assert np.isfinite(S).all() and np.isfinite(v).all(), "non-finite log"
    assert not bad, bad
    assert np.array_equal(S, ref.hat(v).astype(np.float32))  # one log behind both entries, and an exactly skew matrix
    one = case["band"] == case["names"].index("identity")
    assert np.array_equal(S[one], np.zeros((1, 3, 3), np.float32)) and np.array_equal(v[one], np.zeros((1, 3), np.float32))


def test_exp_and_rotvec_to_matrix(case):
    """diffab_so3_exp and diffab_so3_rotvec_to_matrix on the fp32 rotation vectors of every input (the zero vector for the identity), and
    on vectors so short that |v|^2 underflows."""
    hip = case["hip"]
    tiny = np.array([1e-12, 1e-20, 1e-30, 1e-38])[:, None, None] * ref.SPECIAL_AXES[None, :4] / np.linalg.norm(ref.SPECIAL_AXES[:4], axis=-1)[:, None]
    v = np.concatenate([case["v"], tiny.reshape(-1, 3)]).astype(np.float32)
    band = np.concatenate([case["band"], np.full(16, len(case["names"]))])
    names = case["names"] + ["|v| <= 1e-12"]
    n = len(v)
    R1 = run(hip, "diffab_so3_exp", [ref.hat(v)], (n, 3, 3), n)
    R2 = run(hip, "diffab_so3_rotvec_to_matrix", [v], (n, 3, 3), n)
    want = ref.exp(v)
    bad = report("exp geodesic", matrix_errors(R1, want), band, names, BAR)
    bad += report("exp |R^T R - I|", off_orthogonal(R1), band, names, ORTH)
    assert np.isfinite(R1).all() and np.isfinite(R2).all(), "non-finite exp"
    assert not bad, bad
    assert np.array_equal(R1, R2)
    zero = ~v.any(-1)  # the identity's, and any product whose fp32 noise left no skew part
    assert zero[band == case["names"].index("identity")].all()
    assert np.array_equal(R1[zero], np.broadcast_to(np.eye(3, dtype=np.float32), R1[zero].shape))


def test_scale_rot(case):
    """diffab_so3_scale_rot at k = 0, 0.3, 0.999 and 1 on every input."""
    hip, R, n = case["hip"], case["R"], len(case["R"])
    out = run(hip, "diffab_so3_scale_rot", [np.tile(R, (len(KS), 1, 1)), np.array(KS)], (len(KS) * n, 3, 3), len(KS) * n, n)
    out = out.reshape(len(KS), n, 3, 3)
    bad = []
    for got, k in zip(out, KS):
        want = ref.scale(R, np.full(n, k))
        alt = np.where(case["two"][:, None, None], ref.T(want), np.nan) if k not in (0.0, 1.0) else None  # the other axis sign
        bad += [(k, b) for b in report("scale_rot k = %g geodesic" % k, matrix_errors(got, want, alt), case["band"], case["names"], BAR)]
        bad += [(k, b) for b in report("scale_rot k = %g |R^T R - I|" % k, off_orthogonal(got), case["band"], case["names"], ORTH)]
    assert np.isfinite(out).all(), "non-finite scale_rot"
    assert not bad, bad
    assert np.array_equal(out[0], np.broadcast_to(np.eye(3, dtype=np.float32), (n, 3, 3)))


# ------------------------------------------------------------------ the entries that apply them to frames
def sched_on_device():
    from diffab_pytorch.diffusion import CoordinateDiffuser

    return CoordinateDiffuser(T=100, s=0.01, beta_max=0.999)._sched_dev()


def short_rotvecs(rng, n):
    """(n, 3) fp32: exactly zero on a quarter of the rows, |v| log-uniform in 1e-6 .. 1e-2 on the others."""
    v = ref.axes(n, rng) * 10.0 ** rng.uniform(-6, -2, (n, 1))
    v[rng.permutation(n)[: n // 4]] = 0.0
    return v.astype(np.float32)


def noised_mean(O0, k, two):
    """(want, alt) of scale(O0, k): alt is the other value on the two-valued rows, NaN elsewhere."""
    mean = ref.scale(O0, k)
    return mean, np.where(two[:, None, None], ref.T(mean), np.nan)


def test_orient_forward(case):
    """diffab_orient_forward at (B, K) = (2, 64), four frames of every band: t at the first and last schedule index (k = 1 and
    k = sqrt(abar_T) ~ 0) and at two inner ones; the noise rotvec exactly zero on a quarter of the rows and 1e-6 .. 1e-2 long on the
    others; masked rows bitwise O0."""
    hip, B, K = case["hip"], 2, 64
    rng = np.random.default_rng(11)
    O0, band, two = case["R"][case["pick"]], case["band"][case["pick"]], case["two"][case["pick"]]
    sd = sched_on_device()
    abs_ = sd.tensors["alpha_bar_sqrt"].cpu().numpy().astype(np.float64)
    rv = short_rotvecs(rng, B * K)
    mask = rng.uniform(size=B * K) < 0.8
    held = [dev(O0), dev(mask, torch.bool), dev(rv)]
    errs, orth, finite = [], [], True
    for ts in ((0, 100), (1, 57)):
        t = torch.tensor(ts, dtype=torch.int64).cuda()
        Ot = torch.full((B * K, 3, 3), float("nan"), device="cuda")
        _hip.check(hip.diffab_orient_forward(C.byref(sd.struct), P(held[0]), P(held[1]), P(t), P(held[2]), B, K, P(Ot), _hip.stream_ptr()),
                   "diffab_orient_forward")
        got = Ot.cpu().numpy()
        assert np.array_equal(got[~mask], O0[~mask]), ts
        mean, alt = noised_mean(O0, np.repeat(abs_[list(ts)], K), two)
        noise = ref.exp(rv)
        errs.append(matrix_errors(got, mean @ noise, alt @ noise)[mask])
        orth.append(off_orthogonal(got)[mask])
        finite &= bool(np.isfinite(got).all())
    bad = report("orient_forward geodesic", np.max(errs, 0), band[mask], case["names"], BAR)
    bad += report("orient_forward |R^T R - I|", np.max(orth, 0), band[mask], case["names"], ORTH)
    assert finite, "non-finite orient_forward"
    assert not bad, bad


def test_reverse_update(case):
    """diffab_reverse_update at (B, K) = (2, 64), t = 33 (rotation noise on), the predicted frames four of every band: where the supplied
    rotvec is exactly zero O is O0_hat bitwise, elsewhere O0_hat exp(rotvec); residues outside the mask keep their frame."""
    hip, B, K, t = case["hip"], 2, 64, 33
    rng = np.random.default_rng(12)
    n = B * K
    Oh, band = case["R"][case["pick"]], case["band"][case["pick"]]
    rv = np.where(rng.uniform(size=(n, 1)) < 0.5, short_rotvecs(rng, n), (0.3 * rng.standard_normal((n, 3))).astype(np.float32))
    zero = ~rv.any(-1)
    gm = rng.uniform(size=n) < 0.8
    assert (zero & gm).sum() >= 8 and (~zero & gm).sum() >= 64
    O_in = ref.exp(rng.standard_normal((n, 3))).astype(np.float32)
    seq, x, O = dev(rng.integers(0, 20, n), torch.int64), dev(5 * rng.standard_normal((n, 3))), dev(O_in)
    post = torch.softmax(torch.as_tensor(rng.standard_normal((n, 21))), -1)
    held = [dev(rng.standard_normal((n, 3))), dev(Oh), dev(post), dev(gm, torch.bool), dev(rng.standard_normal((n, 3))), dev(rv),
            dev(rng.uniform(size=n))]
    sd = sched_on_device()
    _hip.check(hip.diffab_reverse_update(C.byref(sd.struct), t, P(seq), P(x), P(O), *[P(h) for h in held], B, K, 21, _hip.stream_ptr()),
               "diffab_reverse_update")
    got = O.cpu().numpy()
    err = matrix_errors(got, Oh.astype(np.float64) @ ref.exp(rv))
    bad = report("reverse_update geodesic", err[gm], band[gm], case["names"], BAR)
    bad += report("reverse_update |R^T R - I|", off_orthogonal(got)[gm], band[gm], case["names"], ORTH)
    assert np.isfinite(got).all() and bool(torch.isfinite(x).all()), "non-finite reverse_update"
    assert not bad, bad
    assert np.array_equal(got[zero & gm], Oh[zero & gm]) and np.array_equal(got[~gm], O_in[~gm])


def test_sample_init_noised(case):
    """diffab_sample_init_noised through the sampler harness of tests/test_gpu_design_modes.py (sample(optimize_from=t, t_stop=t) runs no
    reverse step) at (B, K) = (2, 64), the native frames four of every band: the mean rotation scale(O, sqrt(abar_t)) from so3_ref, the
    IGSO3 noise replayed on the same Philox lanes by the existing oracle; t on the histogram branch (1, 5) and the Gaussian one (40)."""
    dims = dict(syn.UNIT_DIMS, NL=2)
    model = make_model(dims, 17)
    sched = orc.cosine_variance_schedule(100, s=0.01, beta_max=0.999)
    B, K, seed, fp = 2, 64, 2025, 3
    inp = {k: v.cpu() for k, v in patches(B, K, dims, seed=9).items()}
    O = case["R"][case["pick"]]
    band, two = case["band"][case["pick"]], case["two"][case["pick"]]
    inp["orientations"] = torch.from_numpy(O.reshape(B, K, 3, 3).copy())
    gm = torch.from_numpy(np.random.default_rng(13).uniform(size=(B, K)) < 0.9)
    inp["generation_mask"] = gm
    g = gm.numpy().reshape(-1)
    cdf = model.orientation_diffuser.so3._cdf.cpu()
    errs, orth, finite = [], [], True
    for t in (1, 5, 40):
        got = {k: v.cpu() for k, v in sample(model, inp, optimize_from=t, t_stop=t, seed=seed, first_patch=fp).items()}
        _, rotvec, _ = step_noise(seed, fp, B, K, t, cdf[t], sched["one_minus_alpha_bar_sqrt"][t], streams=STREAMS_OPT)
        mean, alt = noised_mean(O, np.full(B * K, float(sched["alpha_bar_sqrt"][t])), two)
        noise = ref.exp(rotvec.numpy().reshape(-1, 3))
        Og = got["orientations"].numpy().reshape(-1, 3, 3)
        assert np.array_equal(Og[~g], O[~g]), t
        errs.append(matrix_errors(Og, mean @ noise, alt @ noise)[g])
        orth.append(off_orthogonal(Og)[g])
        finite &= all(bool(torch.isfinite(got[k]).all()) for k in ("translations", "orientations"))
    bad = report("sample_init_noised geodesic", np.max(errs, 0), band[g], case["names"], BAR)
    bad += report("sample_init_noised |R^T R - I|", np.max(orth, 0), band[g], case["names"], ORTH)
    assert finite, "non-finite forward-noised start"
    assert not bad, bad
