"""Design ensembles on the MI355X: diffab_metrics_ensemble through diffab_pytorch.metrics.ensemble.

The rule is DESIGN.md section 4.16 / include/diffab_hip.h; the oracle is the float64 numpy restatement of test_ensemble_host.py, run on
the SAME fp32 points the kernels read (the CA, or the backbone the frame kernel builds).  Bounds:
  integers and comparisons (consensus, consensus_identity, the NaN / -1 / -inf patterns) EQUAL the oracle: the weights used here are
      multiples of 2^-3 and at most 8, so every class sum is exact in fp64 in any order;
  floats: within 2 fp32 ulps of the oracle's fp64 rounded to fp32.  Every sum has at most 4096 * P * 3 same-signed fp64 terms, a relative
      error under 2e-12, which can move the one rounding to fp32 by at most one ulp; the second ulp is margin.  rmsf and rmsd_to_mean also
      get an absolute floor of 1e-9 A: identical designs leave |p - m| at the fp64 rounding of the mean, (N + 1) 2^-53 |p|, about 5e-11 A at
      N = 4096 and |p| = 100 A, not exactly 0;
  central: the argmin (lowest index on ties) of the device's own rmsd_to_mean over the designs of positive weight, and the oracle's
      wherever the oracle's best and second best differ by more than that tolerance."""
import numpy as np
import pytest
import torch

from diffab_pytorch import metrics, synthetic as syn
from sampler_support import hip, make_model
from test_ensemble_host import ensemble_ref

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("hip")]  # every test here needs the device, whether it names the fixture or not

FLOATS = ("aa_freq", "entropy", "mean_points", "rmsf", "log_prob", "rmsd_to_mean", "n_eff")
FLOOR = {"rmsf": 1e-9, "rmsd_to_mean": 1e-9}
KEYS = FLOATS + ("consensus", "consensus_identity", "central")


# ------------------------------------------------------------------ inputs
def rotation(rng):
    q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
    return q * np.sign(np.linalg.det(q))


def designs_of(rng, G, N, K, vocab=20):
    """N designs per patch: a native (scattered residues around a centre up to 30 A from the origin) plus 1.5 A noise, fresh frames, and
    about 60 % of the tokens redrawn.  Design N - 1 is a copy of design 0 when N > 1."""
    centre = rng.normal(0.0, 8.0, (G, 1, K, 3)) + rng.uniform(-30.0, 30.0, (G, 1, 1, 3))
    x = (centre + rng.normal(0.0, 1.5, (G, N, K, 3))).astype(np.float32)
    O = np.stack([rotation(rng) for _ in range(G * N * K)]).reshape(G, N, K, 3, 3).astype(np.float32)
    native = rng.integers(0, vocab, (G, 1, K))
    seq = np.where(rng.random((G, N, K)) < 0.6, rng.integers(0, vocab, (G, N, K)), native)
    if N > 1:
        x[:, N - 1], O[:, N - 1], seq[:, N - 1] = x[:, 0], O[:, 0], seq[:, 0]
    d = {"seq_idx": seq.reshape(G * N, K), "translations": x.reshape(G * N, K, 3), "orientations": O.reshape(G * N, K, 3, 3)}
    return {k: torch.from_numpy(v).cuda() for k, v in d.items()}


def masks(rng, G, K, empty=None):
    """Ragged, as test_gpu_metrics.masks: patch 0 has one counted residue, the others 1 to K/2 scattered ones; residue_mask removes a few
    generated and a few other residues; patch `empty` has no counted residue (its generated residues are all outside residue_mask)."""
    gen, rm = np.zeros((G, K), bool), np.ones((G, K), bool)
    for g in range(G):
        n = 1 if g == 0 else int(rng.integers(1, max(2, K // 2) + 1))
        extra = min(3, K - n)
        pick = rng.choice(K, size=n + extra, replace=False)
        gen[g, pick] = True
        rm[g, pick[n:]] = False
        rest = np.flatnonzero(~gen[g])
        rm[g, rng.choice(rest, size=min(5, rest.size // 2), replace=False)] = False
        if g == empty:
            rm[g, gen[g]] = False
    return gen, rm


def weights_of(rng, G, N):
    """Multiples of 2^-3 in [0, 8], about a quarter of them 0; every group keeps a positive one."""
    w = rng.integers(1, 65, (G, N)) / 8.0
    w[rng.random((G, N)) < 0.25] = 0.0
    w[:, N // 2] = 0.375
    return w.astype(np.float32)


def run(des, gen, rm=None, weights=None, N=1, **kw):
    dev = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()
    out = metrics.ensemble(des, dev(gen), group_size=N, residue_mask=dev(rm), weights=dev(weights), **kw)
    assert set(out) == set(KEYS) and out["consensus"].dtype == torch.int64 and out["central"].dtype == torch.int64
    assert all(out[k].dtype == torch.float32 and out[k].is_cuda for k in FLOATS + ("consensus_identity",))
    return {k: v.cpu().numpy() for k, v in out.items()}


def oracle(des, gen, rm=None, weights=None, N=1, atoms="ca", num_classes=21, pseudocount=0.0):
    return ensemble_ref(des["seq_idx"].cpu().numpy(), metrics._points(des, atoms).cpu().numpy(), gen, rm, weights, N, num_classes, pseudocount)


# ------------------------------------------------------------------ comparison
def bits(a):
    a = np.asarray(a)
    return a.view(np.int32) if a.dtype == np.float32 else a


def assert_same_bits(a, b, what):
    for k in KEYS:
        assert a[k].shape == b[k].shape and np.array_equal(bits(a[k]), bits(b[k])), (what, k)


def assert_close(dev, ref, key, what):
    """Same NaN and infinity pattern; finite entries within 2 fp32 ulps of the oracle rounded to fp32 (or the key's absolute floor)."""
    dev, ref32 = np.asarray(dev, np.float32), np.asarray(ref, np.float64).astype(np.float32)
    assert dev.shape == ref32.shape, (what, key)
    assert np.array_equal(np.isnan(dev), np.isnan(ref32)), (what, key, "NaN pattern")
    inf = np.isinf(ref32)
    assert np.array_equal(np.isinf(dev), inf) and np.array_equal(dev[inf], ref32[inf]), (what, key, "infinities")
    ok = np.isfinite(ref32)
    err = np.abs(dev[ok].astype(np.float64) - ref32[ok].astype(np.float64))
    ulp = np.spacing(np.abs(ref32[ok])).astype(np.float64)
    floor = FLOOR.get(key, 0.0)
    worst = np.max(np.where(err <= floor, 0.0, err / ulp), initial=0.0)
    print(f"{what}: {key} max error {worst:.3g} ulp over {int(ok.sum())} finite entries")
    assert ((err <= 2.0 * ulp) | (err <= floor)).all(), (what, key, worst)


def check(out, ref, w, N, what):
    for k in FLOATS:
        assert_close(out[k], ref[k], k, what)
    assert np.array_equal(out["consensus"], ref["consensus"]), (what, "consensus")
    got, want = out["consensus_identity"], ref["consensus_identity"]
    assert np.array_equal(np.isnan(got), np.isnan(want)) and np.array_equal(bits(np.nan_to_num(got, nan=-1.0)), bits(np.nan_to_num(want, nan=-1.0))), what
    G = out["central"].shape[0]
    w = np.ones((G, N), np.float32) if w is None else np.asarray(w).reshape(G, N)
    rd = out["rmsd_to_mean"].reshape(G, N)
    for g in range(G):
        can = np.flatnonzero((w[g] > 0) & ~np.isnan(rd[g]))
        own = can[np.argmin(rd[g, can])] if can.size else -1  # the first minimum: lowest index on ties
        assert out["central"][g] == own, (what, "central of the device's own rmsd_to_mean", g)
        if can.size and ref["central_gap"][g] > max(1e-9, 4.0 * np.spacing(np.float32(rd[g, own]))):
            assert out["central"][g] == ref["central"][g], (what, "central", g)
        elif not can.size:
            assert ref["central"][g] == -1, (what, g)


# ------------------------------------------------------------------ against the oracle
@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("atoms", ["ca", "backbone"])
@pytest.mark.parametrize("shape", [(3, 5, 70), (2, 130, 33), (1, 1, 1)])
def test_ensemble_equals_the_oracle(shape, atoms, weighted):
    """K = 70 crosses a 64-lane chunk raggedly; N = 130 is more than one 128-design slice and more than one row per wave, a multiple of
    neither; one design of one residue.  Patch 0 has one counted residue, and patch 2 of the first shape none."""
    G, N, K = shape
    rng = np.random.default_rng(1000 * G + N)
    des = designs_of(rng, G, N, K)
    gen, rm = (np.ones((1, 1), bool), None) if K == 1 else masks(rng, G, K, empty=2 if G == 3 else None)
    w = weights_of(rng, G, N) if weighted else None
    out = run(des, gen, rm, w, N, atoms=atoms)
    ref = oracle(des, gen, rm, w, N, atoms)
    check(out, ref, w, N, f"{shape} {atoms} {'weighted' if weighted else 'unweighted'}")
    if G == 3:
        assert np.isnan(out["log_prob"][2 * N:]).all() and np.isnan(out["rmsd_to_mean"][2 * N:]).all() and out["central"][2] == -1
        assert not np.isnan(out["log_prob"][:2 * N]).any() and ((gen & rm).sum(1) == [1, (gen & rm)[1].sum(), 0]).all()
    if rm is not None:
        assert np.isnan(out["entropy"][~rm]).all() and (out["consensus"][~rm] == -1).all() and not np.isnan(out["entropy"][rm]).any()
    # weights as (rows,) are the same call
    if weighted:
        assert_same_bits(run(des, gen, rm, w.reshape(-1), N, atoms=atoms), out, "weights (rows,)")


@pytest.mark.parametrize("pseudocount", [0.0, 1.0])
@pytest.mark.parametrize("num_classes", [20, 21])
def test_pseudocount_and_classes(num_classes, pseudocount):
    """The same designs, tokens in [0, 21): with 20 classes token 20 is in no class - its rows have log_prob -inf - and with a pseudocount
    no frequency is 0."""
    rng = np.random.default_rng(5)
    G, N, K = 2, 9, 40
    des = designs_of(rng, G, N, K, vocab=21)
    des["seq_idx"][3, :] = 20
    gen, rm = masks(rng, G, K)
    w = weights_of(rng, G, N)
    w[0, 3] = 1.0
    out = run(des, gen, rm, w, N, atoms="backbone", num_classes=num_classes, pseudocount=pseudocount)
    ref = oracle(des, gen, rm, w, N, "backbone", num_classes, pseudocount)
    check(out, ref, w, N, f"V = {num_classes}, pseudocount {pseudocount}")
    assert out["aa_freq"].shape == (G, K, num_classes)
    assert np.isneginf(out["log_prob"][3]) == (num_classes == 20)
    if pseudocount > 0:
        assert (out["aa_freq"][rm] > 0).all()


@pytest.mark.parametrize("num_classes, atoms", [(32, "ca"), (32, "backbone"), (1, "ca"), (1, "backbone")])
def test_the_largest_and_the_smallest_number_of_classes(num_classes, atoms):
    """V = 32 is the largest class table in LDS (64 KiB); with V = 1 the table is smaller than the 3 P point sums that pass through the
    same memory, and every token but 0 is outside the classes."""
    rng = np.random.default_rng(6)
    G, N, K = 2, 9, 70
    des = designs_of(rng, G, N, K, vocab=num_classes + 1)
    gen, rm = masks(rng, G, K)
    w = weights_of(rng, G, N)
    out = run(des, gen, rm, w, N, atoms=atoms, num_classes=num_classes, pseudocount=0.5)
    check(out, oracle(des, gen, rm, w, N, atoms, num_classes, 0.5), w, N, f"V = {num_classes} {atoms}")
    assert out["aa_freq"].shape == (G, K, num_classes)


# ------------------------------------------------------------------ exact properties
def test_all_ones_weights_are_no_weights():
    rng = np.random.default_rng(11)
    G, N, K = 2, 131, 70
    des = designs_of(rng, G, N, K)
    gen, rm = masks(rng, G, K)
    for atoms in ("ca", "backbone"):
        assert_same_bits(run(des, gen, rm, np.ones((G, N), np.float32), N, atoms=atoms), run(des, gen, rm, None, N, atoms=atoms), atoms)


@pytest.mark.parametrize("atoms", ["ca", "backbone"])
def test_one_hot_weight_returns_that_design(atoms):
    rng = np.random.default_rng(12)
    G, N, K = 2, 130, 33
    des = designs_of(rng, G, N, K)
    gen, rm = masks(rng, G, K)
    pick = [129, 57]  # (the last row of the second slice; a row in the middle of the first)
    w = np.zeros((G, N), np.float32)
    w[np.arange(G), pick] = [2.5, 0.125]
    out = run(des, gen, rm, w, N, atoms=atoms)
    rows = [g * N + j for g, j in enumerate(pick)]
    pts = metrics._points(des, atoms).cpu().numpy()[rows]
    seq = des["seq_idx"].cpu().numpy()[rows]
    assert np.array_equal(bits(out["mean_points"][rm]), bits(pts[rm]))
    one_hot = np.zeros((G, K, 21), np.float32)
    np.put_along_axis(one_hot, seq[..., None], 1.0, 2)
    assert np.array_equal(bits(out["aa_freq"][rm]), bits(one_hot[rm])) and np.array_equal(out["consensus"][rm], seq[rm])
    assert np.array_equal(bits(out["n_eff"]), bits(np.ones(G, np.float32))) and out["central"].tolist() == pick
    assert np.array_equal(bits(out["entropy"][rm]), bits(np.zeros(int(rm.sum()), np.float32)))
    assert np.array_equal(bits(out["rmsf"][rm]), bits(np.zeros(int(rm.sum()), np.float32)))
    assert np.array_equal(bits(out["rmsd_to_mean"][rows]), bits(np.zeros(G, np.float32))) and (out["consensus_identity"][rows] == 1.0).all()
    assert np.array_equal(bits(out["log_prob"][rows]), bits(np.zeros(G, np.float32)))


def test_a_patch_alone_is_the_patch_in_the_batch():
    rng = np.random.default_rng(13)
    G, N, K = 3, 130, 70
    des = designs_of(rng, G, N, K)
    gen, rm = masks(rng, G, K)
    w = weights_of(rng, G, N)
    for atoms in ("ca", "backbone"):
        full = run(des, gen, rm, w, N, atoms=atoms)
        for g in range(G):
            alone = run({k: v[g * N:(g + 1) * N] for k, v in des.items()}, gen[g:g + 1], rm[g:g + 1], w[g:g + 1], N, atoms=atoms)
            part = {k: (full[k][g * N:(g + 1) * N] if full[k].shape[0] == G * N else full[k][g:g + 1]) for k in KEYS}
            assert_same_bits(alone, part, f"patch {g} {atoms}")


@pytest.mark.parametrize("atoms", ["ca", "backbone"])
def test_one_design_per_patch_is_plus_zero(atoms):
    rng = np.random.default_rng(14)
    G, K = 3, 70
    des = designs_of(rng, G, 1, K)
    gen, rm = masks(rng, G, K)
    out = run(des, gen, rm, None, 1, atoms=atoms)
    zero = lambda n: bits(np.zeros(n, np.float32))
    inside = int(rm.sum())
    assert np.array_equal(bits(out["entropy"][rm]), zero(inside)) and np.array_equal(bits(out["rmsf"][rm]), zero(inside))
    assert np.array_equal(bits(out["rmsd_to_mean"]), zero(G)) and np.array_equal(bits(out["log_prob"]), zero(G))
    assert (out["consensus_identity"] == 1.0).all() and (out["n_eff"] == 1.0).all() and out["central"].tolist() == [0] * G
    assert np.array_equal(bits(out["mean_points"][rm]), bits(metrics._points(des, atoms).cpu().numpy()[rm]))


# ------------------------------------------------------------------ edge cases
def test_a_group_of_zero_weights_is_undefined_and_alone():
    rng = np.random.default_rng(15)
    G, N, K = 3, 6, 70
    des = designs_of(rng, G, N, K)
    gen, rm = masks(rng, G, K)
    w = weights_of(rng, G, N)
    w0 = w.copy()
    w0[1] = [0.0, -1.0, np.nan, -np.inf, np.inf, 0.0]  # a negative or non-finite weight is 0
    out, base = run(des, gen, rm, w0, N, atoms="backbone"), run(des, gen, rm, w, N, atoms="backbone")
    for k in ("aa_freq", "entropy", "mean_points", "rmsf"):
        assert np.isnan(out[k][1]).all(), k
    for k in ("log_prob", "rmsd_to_mean"):
        assert np.isnan(out[k][N:2 * N]).all(), k
    assert (out["consensus"][1] == -1).all() and (out["consensus_identity"][N:2 * N] == 0.0).all()
    assert np.isnan(out["n_eff"][1]) and out["central"][1] == -1
    for k in KEYS:  # the neighbours are what they are without the change
        rows = out[k].shape[0] == G * N
        for g in (0, 2):
            sl = slice(g * N, (g + 1) * N) if rows else slice(g, g + 1)
            assert np.array_equal(bits(out[k][sl]), bits(base[k][sl])), (k, g)
    check(out, oracle(des, gen, rm, w0, N, "backbone"), np.where(np.isfinite(w0) & (w0 > 0), w0, 0), N, "a group of zero weights")


def test_tokens_outside_the_classes():
    rng = np.random.default_rng(16)
    G, N, K = 2, 7, 33
    des = designs_of(rng, G, N, K)
    gen, rm = masks(rng, G, K)
    k0 = int(np.flatnonzero(gen[1] & rm[1])[0])  # a counted position of patch 1
    des["seq_idx"][N + 2, k0] = 21
    des["seq_idx"][N + 4, k0] = -1
    out = run(des, gen, rm, None, N)
    assert np.isneginf(out["log_prob"][[N + 2, N + 4]]).all()
    others = np.setdiff1d(np.arange(G * N), [N + 2, N + 4])
    assert np.isfinite(out["log_prob"][others]).all()
    f = out["aa_freq"][1, k0].astype(np.float64)
    assert abs(f.sum() - 1.0) < 1e-6 and (f * (N - 2)).round().sum() == N - 2  # the five other designs share the position
    check(out, oracle(des, gen, rm, None, N), None, N, "tokens 21 and -1")
    des["seq_idx"][N:2 * N, k0] = torch.tensor([21, -1, 22, -5, 21, 1 << 40, -(1 << 40)]).cuda()  # no design has a class there
    out = run(des, gen, rm, None, N)
    assert np.isnan(out["aa_freq"][1, k0]).all() and np.isnan(out["entropy"][1, k0]) and out["consensus"][1, k0] == -1
    assert np.isneginf(out["log_prob"][N:2 * N]).all() and np.isfinite(out["log_prob"][:N]).all()
    check(out, oracle(des, gen, rm, None, N), None, N, "a position without a class")
    smoothed = run(des, gen, rm, None, N, pseudocount=2.0)
    assert np.array_equal(bits(smoothed["aa_freq"][1, k0]), bits(np.full(21, np.float32(1.0 / 21.0))))
    assert abs(float(smoothed["entropy"][1, k0]) - np.log(21.0)) <= 2 * np.spacing(np.float32(np.log(21.0))) and smoothed["consensus"][1, k0] == -1


# ------------------------------------------------------------------ end to end
def test_sampled_designs_share_their_context():
    """sample(num_samples = 4, steps = 2) -> ensemble on the sampler's own tensors: the oracle on them, and +0 entropy and RMSF at the
    positions the sampler does not generate (all designs of a patch share their context)."""
    dims = dict(syn.BENCH_DIMS, NL=2)
    model = make_model(dims, seed=1)
    inp = {k: v.cuda() for k, v in syn.patches(2, 128, dims, seed=3, coord_sigma=8.0).items()}
    N = 4
    res = model.sample(inp["seq_idx"], inp["translations"], inp["orientations"], res_context_emb=inp["res_context_emb"],
                       pair_context_emb=inp["pair_context_emb"], generation_mask=inp["generation_mask"], seed=1, num_samples=N, steps=2)
    gen, rm = inp["generation_mask"].cpu().numpy(), inp["residue_mask"].cpu().numpy()
    for atoms in ("ca", "backbone"):
        got = metrics.ensemble(res, inp["generation_mask"], group_size=N, residue_mask=inp["residue_mask"], atoms=atoms)
        assert got["aa_freq"].is_cuda and got["aa_freq"].shape == (2, 128, 21) and got["mean_points"].shape == (2, 128, 1 if atoms == "ca" else 4, 3)
        out = {k: v.cpu().numpy() for k, v in got.items()}
        check(out, oracle(res, gen, rm, None, N, atoms), None, N, f"sampled {atoms}")
        context = rm & ~gen
        zero = bits(np.zeros(int(context.sum()), np.float32))
        assert context.any() and np.array_equal(bits(out["entropy"][context]), zero) and np.array_equal(bits(out["rmsf"][context]), zero)
        assert (out["rmsf"][gen & rm] > 0).all()
