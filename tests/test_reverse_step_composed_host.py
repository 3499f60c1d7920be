"""CPU: the composed float64 restatement of one reverse step (tests/reverse_step_ref.py) before any kernel is compared with it.

With every option neutral it is orc.reverse_update on the sampler's Philox lanes; with one option on it is that option's own host
restatement (tempered_draw, seq_jump_ref, guidance_ref / shift_ref, the IGSO3 rules of the oracle, resample_oracle); with several on
it is their composition in the kernel's documented order; and the inputs the kernel has branches for - no allowed class, allowed
classes all at probability 0, tau = 0 with a tie, s = 0, lambda_O = 0, lambda_x = 0 - give what DESIGN 4.7 / 4.9 / 4.11 say.
tests/test_gpu_reverse_step_composed.py holds the kernel to this function."""
import numpy as np
import pytest
import torch

import diffab_oracle as orc
from diffab_pytorch.diffusion import cosine_variance_schedule, jump_coefficients
from diffab_pytorch.guidance import SampleGuidance
from diffab_pytorch.steering import ParticleSteering, resample_oracle
from diffab_pytorch.temperature import tempered_draw
from reverse_step_ref import STREAM_STEER, draw_edges, reverse_step_ref
from sampler_support import lanes, step_noise
from test_guidance_host import guidance_ref, shift_ref
from test_respaced_host import seq_jump_ref

V, T, SEED, FIRST = 21, 100, 77, 5
SCHED = cosine_variance_schedule(T, s=0.01, beta_max=0.999)
STEPS = [(57, 20), (30, 29), (8, 0), (2, 1)]
GUIDE = SampleGuidance(clash=2.0, bond=1.0, max_shift=0.5)


def coefficients(t, s):
    b, a = jump_coefficients(SCHED, torch.tensor([t]), s, 0.999)
    return float(b[t]), float(a[t])


def cdf_row(sigma):
    return orc.igso3_cdf_table(orc.igso3_table([torch.tensor(float(sigma))]))[0]


@pytest.fixture(scope="module")
def rows_by_sigma():
    """CDF rows of CPU tables over lambda sqrt(beta'), built once per distinct sigma below the threshold."""
    cache = {}

    def get(lam, beta_j):
        sg = float(torch.tensor(beta_j, dtype=torch.float32).sqrt() * torch.tensor(lam, dtype=torch.float32))
        if sg not in cache:
            cache[sg] = cdf_row(sg)
        return cache[sg]
    return get


def predictions(B, K, seed):
    """Seeded random state and model outputs: two generated segments per row, clashing predictions, a ragged posterior."""
    rng = np.random.default_rng(seed)
    gm = np.zeros((B, K), bool)
    gm[:, 1:K // 3] = True
    gm[:, K // 2 + 1:K - 2] = True
    seq = rng.integers(0, 20, (B, K))
    x = rng.normal(0, 6, (B, K, 3)).astype(np.float32)
    x0 = np.where(gm[..., None], rng.normal(0, 1.5, (B, K, 3)), x).astype(np.float32)
    eps = rng.normal(0, 1, (B, K, 3)).astype(np.float32)
    O = orc.uniform_rotation_from_normals(torch.from_numpy(rng.normal(0, 1, (B, K, 4)).astype(np.float32)))
    O0 = orc.uniform_rotation_from_normals(torch.from_numpy(rng.normal(0, 1, (B, K, 4)).astype(np.float32)))
    post = rng.dirichlet(np.full(V, 0.3), (B, K)).astype(np.float32)
    chain = np.broadcast_to((np.arange(K) >= K // 2).astype(np.int32), (B, K))
    ridx = np.broadcast_to(np.arange(K, dtype=np.int32) + 7 * (np.arange(K) >= K // 2), (B, K))
    rmask = (rng.random((B, K)) > 0.1) | gm
    return dict(gm=gm, seq=seq, x=x, x0=x0, eps=eps, O=O, O0=O0, post=post, tables=(chain, ridx, rmask))


def ref(p, t, s, **kw):
    bj, aj = coefficients(t, s)
    if "rot_cdf" not in kw and "rot_scale" not in kw and s > 0 and bj ** 0.5 < 0.1:  # every row at scale 1, from the histogram
        kw["rot_cdf"] = {1.0: cdf_row(torch.tensor(bj, dtype=torch.float32).sqrt())}
    return reverse_step_ref(t, s, p["seq"], p["x0"], p["O0"].numpy(), p["post"], p["gm"], SCHED, bj, aj, SEED, FIRST, **kw)


# ------------------------------------------------------------------ neutral: the oracle's reverse step
@pytest.mark.parametrize("t", [30, 2, 1])
def test_neutral_is_the_oracle_reverse_update(rows_by_sigma, t):
    B, K = 3, 24
    p = predictions(B, K, seed=t)
    beta = float(SCHED["beta"][t])
    row = rows_by_sigma(1.0, beta)
    z, rotvec, us = step_noise(SEED, FIRST, B, K, t, row, SCHED["beta"].sqrt()[t])
    den = {"translations_eps": torch.from_numpy(p["eps"]), "orientations_t0": p["O0"], "seq_posterior": torch.from_numpy(p["post"])}
    gm = torch.from_numpy(p["gm"])
    s1, x1, O1 = orc.reverse_update(t, torch.from_numpy(p["seq"]), torch.from_numpy(p["x"]), p["O"], den, gm, SCHED, z, rotvec, us)
    got = ref(p, t, t - 1, rot_cdf={1.0: row})
    assert np.array_equal(got["seq"], s1.numpy())
    assert not got["dx"].any() and not got["delta"].any()
    Og = np.where(p["gm"][..., None, None], got["O"], p["O"].double().numpy())
    assert np.abs(Og - O1.double().numpy()).max() < 5e-6  # the oracle multiplies in fp32
    assert np.abs(got["rotvec"] - (rotvec.double().numpy() * p["gm"][..., None] if t > 1 else 0.0)).max() == 0.0
    assert bool(got["hist"].all()) == (beta ** 0.5 < 0.1)
    if t == 1:
        assert not got["theta"].any() and not got["noise"].any()
        assert np.array_equal(got["O"], p["O0"].double().numpy())
    # lambda_x alone: the oracle's step with z scaled, minus the oracle's step
    lam = np.array([0.0, 0.5, 1.5], np.float32)
    zs = z * torch.from_numpy(lam)[:, None, None]
    _, x2, _ = orc.reverse_update(t, torch.from_numpy(p["seq"]), torch.from_numpy(p["x"]), p["O"], den, gm, SCHED, zs, rotvec, us)
    got = ref(p, t, t - 1, rot_cdf={1.0: row}, trans_scale=lam)
    tol = 4 * 2.0 ** -24 * float(x1.abs().max())
    assert np.abs((x2 - x1).double().numpy() - got["dx"]).max() <= tol
    assert np.array_equal(got["seq"], s1.numpy()) and not got["noise"][0].any()


# ------------------------------------------------------------------ one option on: that option's own restatement
@pytest.mark.parametrize("t, s", STEPS)
def test_jump_alone_is_seq_jump_ref_drawn_by_the_oracle(t, s):
    p = predictions(3, 24, seed=100 + t)
    bj, aj = coefficients(t, s)
    got = ref(p, t, s)
    us = torch.from_numpy(orc.philox_uniform4(SEED, *lanes(FIRST, 3, 24), t, orc.STREAM_SEQ)[0])
    r = p["post"]
    if s < t - 1:
        r = seq_jump_ref(p["post"], p["seq"], float(SCHED["alpha"][t]), float(SCHED["beta"][t]), float(SCHED["alpha_bar"][t - 1]), aj,
                         float(SCHED["alpha_bar"][s])).astype(np.float32)
        assert np.abs(r.sum(-1) - 1).max() < 1e-6 and np.abs(r - p["post"]).max() > 1e-3
    want = orc.categorical_from_uniform(torch.from_numpy(r), us).numpy()
    safe = got["edge"] > 1e-6  # (the oracle's running sum is fp32)
    assert safe[p["gm"]].mean() > 0.99
    assert np.array_equal(got["seq"][p["gm"] & safe], want[p["gm"] & safe])
    assert np.array_equal(got["seq"][~p["gm"]], p["seq"][~p["gm"]])
    assert not got["dx"].any()
    assert (got["theta"][p["gm"]] > 0).all() == (s > 0) and got["theta"].any() == (s > 0)


def test_temperature_and_mask_alone_are_tempered_draw_and_the_masked_oracle_draw():
    B, K, t = 4, 24, 30
    p = predictions(B, K, seed=7)
    us = orc.philox_uniform4(SEED, *lanes(FIRST, B, K), t, orc.STREAM_SEQ)[0]
    tau = np.array([0.0, 0.5, 1.0, 2.0], np.float32)
    got = ref(p, t, t - 1, seq_temp=tau)
    for b, k in zip(*np.nonzero(p["gm"])):
        assert got["seq"][b, k] == tempered_draw(p["post"][b, k], float(us[b, k]), float(tau[b])), (b, k)
    assert np.array_equal(got["seq"][0][p["gm"][0]], p["post"][0].argmax(-1)[p["gm"][0]])
    assert np.isinf(got["edge"][0]).all() and np.isfinite(got["edge"][1:][p["gm"][1:]]).all()
    rng = np.random.default_rng(3)
    allowed = rng.random((B, K, V)) < 0.5
    allowed[..., 4] = True
    got = ref(p, t, t - 1, allowed=allowed)
    masked = torch.from_numpy(np.where(allowed, p["post"], np.float32(0)))
    want = orc.categorical_from_uniform(masked, torch.from_numpy(us)).numpy()
    safe = p["gm"] & (got["edge"] > 1e-6)
    assert np.array_equal(got["seq"][safe], want[safe]) and safe.sum() > 0.95 * p["gm"].sum()
    assert np.take_along_axis(allowed, got["seq"][..., None], -1)[..., 0][p["gm"]].all()


@pytest.mark.parametrize("t, s", STEPS)
def test_guidance_alone_is_minus_the_capped_shift_at_the_jumps_beta(t, s):
    p = predictions(3, 24, seed=200 + t)
    bj, _ = coefficients(t, s)
    got = ref(p, t, s, guidance=GUIDE, tables=p["tables"])
    g = guidance_ref(p["x0"], p["gm"], *p["tables"], GUIDE.clash, GUIDE.clash_distance, GUIDE.bond, GUIDE.bond_length)["grad"]
    want = shift_ref(g, bj, GUIDE.max_shift)
    assert np.abs(want).max() > 1e-3 and np.array_equal(got["dx"], -want) and np.array_equal(got["delta"], want)
    assert not got["dx"][~p["gm"]].any()
    off = ref(p, t, s, guidance=SampleGuidance(clash=2.0, bond=1.0, t_max=t - 1), tables=p["tables"])
    assert not off["dx"].any()


@pytest.mark.parametrize("t, s", STEPS)
def test_rotation_scales_alone_are_the_oracles_draw_on_each_rows_own_table(rows_by_sigma, t, s):
    B, K = 4, 24
    p = predictions(B, K, seed=300 + t)
    bj, _ = coefficients(t, s)
    lo = np.array([0.0, 0.06, 0.3, 1.0], np.float32)
    cdf = {float(l): rows_by_sigma(float(l), bj) for l in lo[1:] if float(l) * bj ** 0.5 < 0.1}
    got = ref(p, t, s, rot_scale=lo, rot_cdf=cdf)
    assert np.array_equal(got["O"][0], p["O0"].double().numpy()[0]) and not got["theta"][0].any()
    assert not got["dx"].any()
    if s == 0:
        assert not got["theta"].any() and np.array_equal(got["O"], p["O0"].double().numpy())
        return
    ua = orc.philox_uniform4(SEED, *lanes(FIRST, B, K), t, orc.STREAM_ANGLE)
    na = orc.philox_normal4(SEED, *lanes(FIRST, B, K), t, orc.STREAM_ANGLE)
    ax = torch.nn.functional.normalize(torch.from_numpy(np.stack(orc.philox_normal4(SEED, *lanes(FIRST, B, K), t, orc.STREAM_AXIS)[:3], -1)),
                                       dim=-1).double().numpy()
    for b in range(1, B):
        sg = torch.tensor(bj, dtype=torch.float32).sqrt() * torch.tensor(float(lo[b]), dtype=torch.float32)
        if float(sg) < 0.1:
            th = orc.igso3_theta_from_hist(orc.igso3_bin_from_cdf(cdf[float(lo[b])], torch.from_numpy(ua[0][b])), torch.from_numpy(ua[1][b]))
        else:
            th = orc.igso3_theta_from_gaussian(sg, torch.from_numpy(na[2][b]))
        m = p["gm"][b]
        assert got["hist"][b] == (float(sg) < 0.1) and abs(got["sigma"][b] - float(sg)) == 0
        assert np.abs(got["theta"][b][m] - th.double().numpy()[m]).max() < 1e-6, b
        assert np.abs(got["axis"][b][m] - ax[b][m]).max() < 1e-6, b
    assert not got["hist"][0]


def test_steering_alone_is_the_resampling_oracle_and_a_gather():
    B, N, K, t, s = 6, 3, 24, 57, 20
    p = predictions(2, K, seed=9)
    rep = {k: (tuple(np.repeat(x, N, 0) for x in v) if k == "tables" else
               (v.repeat_interleave(N, 0) if torch.is_tensor(v) else np.repeat(v, N, 0))) for k, v in p.items()}
    rng = np.random.default_rng(1)
    rep["x0"] = np.where(rep["gm"][..., None], rep["x0"] + rng.normal(0, 0.7, rep["x0"].shape), rep["x0"]).astype(np.float32)
    st = ParticleSteering(strength=0.05, clash=1.3, bond=0.7, ess_threshold=2.0)
    lx = np.linspace(0.0, 1.5, B).astype(np.float32)
    plain = ref(rep, t, s, trans_scale=lx)
    got = ref(rep, t, s, trans_scale=lx, steering=st, tables=rep["tables"], group_size=N)
    e = guidance_ref(rep["x0"], rep["gm"], *rep["tables"], 1.3, 3.8, 0.7, 3.8)
    U = 1.3 * e["clash"] + 0.7 * e["bond"]
    assert np.array_equal(got["energy"], U) and (U > 0).all()
    u = orc.philox_uniform4(SEED, FIRST + np.array([0, N]), np.zeros(2, np.int64), t, STREAM_STEER)[0]
    zero = np.zeros(B, np.float32)
    want = resample_oracle(zero, zero, U.astype(np.float32), u, N, 0.05, 2.0)
    anc = want["ancestors"] + np.arange(B) // N * N
    assert want["resampled"].all() and np.array_equal(got["ancestors"], anc) and len(set(anc.tolist())) < B
    gm = rep["gm"]
    for k in ("seq", "dx", "rotvec", "O"):
        assert np.array_equal(got[k][gm], plain[k][anc][gm]) and np.array_equal(got[k][~gm], plain[k][~gm]), k


# ------------------------------------------------------------------ everything on: the composition, and the kernel's edge inputs
def all_options(B, K, rows_by_sigma, t, s, seed):
    p = predictions(B, K, seed=seed)
    bj, _ = coefficients(t, s)
    rng = np.random.default_rng(seed + 1)
    allowed = rng.random((B, K, V)) < 0.5
    allowed[..., 2] = True
    gen = np.argwhere(p["gm"])
    for j, (b, k) in enumerate(gen[:3]):
        allowed[b, k] = np.arange(V) == 5 + j  # single-class residues
    b0, k0 = gen[3]
    allowed[b0, k0] = False                    # no class allowed: the token stays
    lx = np.array([1.5, 0.0, 1.0, 0.5], np.float32)
    lo = np.array([0.0, 0.06, 0.3, 1.0], np.float32)
    tau = np.array([0.5, 1.0, 0.0, 2.0], np.float32)
    cdf = {float(l): rows_by_sigma(float(l), bj) for l in lo[1:] if float(l) * bj ** 0.5 < 0.1 and s > 0}
    kw = dict(trans_scale=lx, rot_scale=lo, seq_temp=tau, rot_cdf=cdf, allowed=allowed, guidance=GUIDE, tables=p["tables"])
    return p, kw, (b0, k0)


@pytest.mark.parametrize("t, s", STEPS)
def test_all_options_are_their_composition_in_the_kernels_order(rows_by_sigma, t, s):
    B, K = 4, 24
    p, kw, (b0, k0) = all_options(B, K, rows_by_sigma, t, s, seed=400 + t)
    got = ref(p, t, s, **kw)
    bj, aj = coefficients(t, s)
    gm, lx, lo, tau, allowed = p["gm"], kw["trans_scale"], kw["rot_scale"], kw["seq_temp"], kw["allowed"]
    # sequence: jump first (from the untempered, unrestricted posterior), then the mask, then the temperature
    r = p["post"].astype(np.float64)
    if s < t - 1:
        r = seq_jump_ref(p["post"], p["seq"], float(SCHED["alpha"][t]), float(SCHED["beta"][t]), float(SCHED["alpha_bar"][t - 1]), aj,
                         float(SCHED["alpha_bar"][s])).astype(np.float32).astype(np.float64)
    us = orc.philox_uniform4(SEED, *lanes(FIRST, B, K), t, orc.STREAM_SEQ)[0]
    for b, k in zip(*np.nonzero(gm)):
        want = tempered_draw(r[b, k], float(us[b, k]), float(tau[b]), allowed[b, k].tolist())
        assert got["seq"][b, k] == (want if want >= 0 else p["seq"][b, k]), (b, k)
        assert got["drawn"][b, k] == (want >= 0)
        if want >= 0:
            assert allowed[b, k, want]
    assert got["seq"][b0, k0] == p["seq"][b0, k0] and not got["drawn"][b0, k0]
    assert np.array_equal(got["seq"][~gm], p["seq"][~gm])
    # translations: Delta with beta', unscaled, then the scaled noise when s > 0
    g = guidance_ref(p["x0"], gm, *p["tables"], GUIDE.clash, GUIDE.clash_distance, GUIDE.bond, GUIDE.bond_length)["grad"]
    delta = shift_ref(g, bj, GUIDE.max_shift)
    z = np.stack(orc.philox_normal4(SEED, *lanes(FIRST, B, K), t, orc.STREAM_TRANS)[:3], -1).astype(np.float64)
    sb = float(torch.tensor(bj, dtype=torch.float32).sqrt())
    want = -delta + ((lx.astype(np.float64) - 1)[:, None, None] * sb * z if s > 0 else 0.0)
    assert np.abs(got["dx"] - want * gm[..., None]).max() < 1e-12
    assert not got["noise"][1].any() and (s > 0) == bool(got["noise"][0].any())
    # orientations: one option's result, untouched by the others
    alone = ref(p, t, s, rot_scale=lo, rot_cdf=kw["rot_cdf"])
    for k in ("theta", "axis", "O", "hist"):
        assert np.array_equal(got[k], alone[k]), k
    assert np.array_equal(got["O"][0], p["O0"].double().numpy()[0])


def test_edge_inputs_the_kernel_has_branches_for():
    B, K, t = 2, 6, 8
    p = predictions(B, K, seed=11)
    p["gm"][:] = True
    p["x0"] = np.random.default_rng(0).normal(0, 1.5, (B, K, 3)).astype(np.float32)
    post = np.zeros((B, K, V), np.float32)
    post[..., 3] = post[..., 9] = 0.4     # a tie at the top
    post[..., 12] = 0.2
    p["post"] = post
    allowed = np.ones((B, K, V), bool)
    allowed[0, 0] = False                  # no allowed class
    allowed[0, 1] = False
    allowed[0, 1, [1, 6, 7, 15]] = True    # allowed classes all at probability 0: unit weights
    allowed[0, 2, 3] = False               # the tie's first class excluded
    us = orc.philox_uniform4(SEED, *lanes(FIRST, B, K), t, orc.STREAM_SEQ)[0]
    for tau in (0.0, 0.5, 1.0):
        got = ref(p, t, t - 1, seq_temp=np.full(B, tau, np.float32), allowed=allowed)
        assert got["seq"][0, 0] == p["seq"][0, 0] and not got["drawn"][0, 0]
        assert got["seq"][0, 1] == [1, 6, 7, 15][min(int(float(us[0, 1]) * 4), 3)], tau
        assert abs(got["edge"][0, 1] - np.abs(np.arange(1, 5) / 4 - us[0, 1]).min()) < 1e-12
        if tau == 0.0:
            assert (got["seq"][1] == 3).all() and got["seq"][0, 2] == 9, "the lowest index on a tie, among the allowed classes"
            assert np.isinf(got["edge"][1]).all()
    # s = 0: no noise of either kind, whatever the scales; the jump to 0 is the recovered x0 distribution, exact zeros included
    lx, lo = np.array([1.5, 0.0], np.float32), np.array([1.0, 0.3], np.float32)
    got = ref(p, t, 0, trans_scale=lx, rot_scale=lo, guidance=GUIDE, tables=p["tables"])
    assert not got["noise"].any() and not got["theta"].any() and np.array_equal(got["O"], p["O0"].double().numpy())
    assert np.array_equal(got["dx"], -got["delta"]) and np.abs(got["delta"]).max() > 1e-3
    assert (got["probs"][..., [0, 1, 2]] == 0).all() and np.abs(got["probs"].sum(-1) - 1).max() < 1e-6
    # lambda_O = 0 and lambda_x = 0 at a noisy step
    bj, _ = coefficients(t, 5)
    got = ref(p, t, 5, trans_scale=np.array([0.0, 1.0], np.float32), rot_scale=np.array([0.0, 1.0], np.float32),
              rot_cdf={1.0: cdf_row(torch.tensor(bj, dtype=torch.float32).sqrt())})
    assert np.array_equal(got["O"][0], p["O0"].double().numpy()[0]) and (got["theta"][1] > 0).all()
    z = np.stack(orc.philox_normal4(SEED, *lanes(FIRST, B, K), t, orc.STREAM_TRANS)[:3], -1).astype(np.float64)
    assert not got["noise"][0].any() and not got["dx"][1].any()
    assert np.array_equal(got["dx"][0], -float(torch.tensor(bj, dtype=torch.float32).sqrt()) * z[0])
    with pytest.raises(ValueError, match="needs the table row"):
        ref(p, 2, 1, rot_scale=np.array([0.5, 1.0], np.float32), rot_cdf={1.0: torch.ones(8)})


def test_draw_edges_are_where_tempered_draw_changes_class():
    rng = np.random.default_rng(5)
    n = 0
    for _ in range(200):
        p = rng.dirichlet(np.full(V, 0.3))
        p[rng.random(V) < 0.1] = 0.0
        ok = (rng.random(V) < 0.6).tolist() if rng.random() < 0.7 else None
        tau = float(rng.choice([0.0, 0.5, 1.0, 2.0]))
        edges = draw_edges(p, tau, ok)
        idx = [v for v in range(V) if ok is None or ok[v]]
        if edges is None:
            draws = {tempered_draw(p, u, tau, ok) for u in (1e-7, 0.3, 0.999999)}
            assert len(draws) == 1
            continue
        assert abs(edges[-1] - 1) < 1e-12 and len(edges) == len(idx)
        for j, e in enumerate(edges[:-1]):
            if e < 1e-9 or e > 1 - 1e-9 or (j and e - edges[j - 1] < 1e-9):
                continue
            nxt = next(idx[i] for i in range(j + 1, len(idx)) if edges[i] > e + 5e-10)
            assert tempered_draw(p, e - 5e-10, tau, ok) == idx[j] and tempered_draw(p, e + 5e-10, tau, ok) == nxt
            n += 1
    assert n > 500
