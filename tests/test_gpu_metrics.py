"""Design metrics on the MI355X: diffab_metrics_vs_native / _pairwise / _select_diverse through diffab_pytorch.metrics.

The rules are DESIGN.md section 4.13 / include/diffab_hip.h; the oracle is the float64 numpy restatement of test_metrics_host.py, run
on the SAME fp32 points the kernels read (the CA, or the backbone the frame kernel builds).  Bounds, from the arithmetic the header fixes:
  in place  |dev - ref| <= 1e-4 * ref   (one rounding per difference, 3nP fp32 terms: (3nP + 2) * 2^-24 on the msd, half on the root;
                                          9.2e-5 for a full K = 256 backbone row, 7e-6 for the 40 residues used here; ref = 0 gives 0)
  aligned   |dev - ref| <= 1e-5 A + 1e-5 * ref   (fp64 sums and solve: about 1e-6 A at ref = 0, the fp32 rounding 6e-8 relative elsewhere)
AAR, sequence identity and the selection are integers and comparisons: they must EQUAL the oracle."""
import numpy as np
import pytest
import torch

from diffab_pytorch import DiffAb, metrics, synthetic as syn
from sampler_support import hip
from test_metrics_host import evaluate_ref, pairwise_ref, rotation, select_ref

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("hip")]  # every test here needs the device, whether it names the fixture or not


def assert_in_place(dev, ref, what):
    dev, ref = np.asarray(dev, np.float64), np.asarray(ref, np.float64)
    assert np.array_equal(np.isnan(dev), np.isnan(ref)), what
    ok = ~np.isnan(ref)
    err = np.abs(dev[ok] - ref[ok])
    print(f"{what}: in-place max |dev - ref| / ref = {np.max(err / np.maximum(ref[ok], 1e-30), initial=0.0):.3g}")
    assert (err <= 1e-4 * ref[ok]).all(), (what, float(err.max()))


def assert_aligned(dev, ref, what):
    dev, ref = np.asarray(dev, np.float64), np.asarray(ref, np.float64)
    assert np.array_equal(np.isnan(dev), np.isnan(ref)), what
    ok = ~np.isnan(ref)
    err = np.abs(dev[ok] - ref[ok])
    print(f"{what}: aligned max |dev - ref| = {np.max(err, initial=0.0):.3g} A, max ratio to the bound {np.max(err / (1e-5 + 1e-5 * ref[ok]), initial=0.0):.3g}")
    assert (err <= 1e-5 + 1e-5 * ref[ok]).all(), (what, float(err.max()))


def same_bits(a, b):
    return np.array_equal(np.asarray(a).view(np.int32), np.asarray(b).view(np.int32))


# ------------------------------------------------------------------ inputs
def natives(rng, G, K):
    x = (rng.normal(0.0, 8.0, (G, K, 3)) + rng.uniform(-30.0, 30.0, (G, 1, 3))).astype(np.float32)
    O = np.stack([[rotation(rng) for _ in range(K)] for _ in range(G)]).astype(np.float32)
    return {"seq_idx": rng.integers(0, 20, (G, K)), "translations": x, "orientations": O}


def design_of(rng, nat, g, kind):
    """One design of patch g: the native plus N(0, 1.5 A) noise, a rigidly moved native, a mirrored native, unrelated coordinates."""
    x, O, seq = nat["translations"][g].astype(np.float64), nat["orientations"][g].astype(np.float64), nat["seq_idx"][g].copy()
    K = x.shape[0]
    if kind == "noise":
        x = x + rng.normal(0.0, 1.5, x.shape)
        O = O @ np.stack([rotation(rng) for _ in range(K)])
        change = rng.random(K) < 0.6
        seq[change] = rng.integers(0, 20, int(change.sum()))
    elif kind == "moved":  # global = local @ O + t, so a motion x -> x R^T + s takes O to O R^T
        R = rotation(rng)
        x, O = x @ R.T + rng.normal(0.0, 5.0, 3), O @ R.T
    elif kind == "mirrored":
        M = np.diag([1.0, 1.0, -1.0])
        x, O = x @ M, O @ M
    elif kind == "unrelated":
        x, seq = rng.normal(0.0, 12.0, x.shape), rng.integers(0, 20, K)
        O = np.stack([rotation(rng) for _ in range(K)])
    return seq, x.astype(np.float32), O.astype(np.float32)


KINDS = ("noise", "moved", "mirrored", "unrelated", "noise")


def masks(rng, G, K, lo=1, hi=40):
    """Ragged: 1-40 counted residues per patch, scattered; a residue_mask that removes a few generated residues as well."""
    gen, rm = np.zeros((G, K), bool), np.ones((G, K), bool)
    for g in range(G):
        n = lo if g == 0 else int(rng.integers(lo, hi + 1))  # patch 0: the smallest selection
        pick = rng.choice(K, size=min(K, n + 3), replace=False)
        gen[g, pick] = True
        rm[g, pick[n:]] = False
        rm[g, rng.choice(np.flatnonzero(~gen[g]), size=5, replace=False)] = False
    return gen, rm


def segments(gen, rm):
    """Labels over 4 segments: the first counted residue alone in segment 1, the others alternate between 0 and 2, segment 3 is empty;
    one counted residue of the larger patches has no label (-1) and uncounted residues carry labels that must not count."""
    seg = np.full(gen.shape, 2, np.int64)
    for g in range(gen.shape[0]):
        c = np.flatnonzero(gen[g] & rm[g])
        seg[g, c] = np.where(np.arange(c.size) % 2 == 0, 0, 2)
        seg[g, c[0]] = 1
        if c.size > 4:
            seg[g, c[-1]] = -1
    return seg


def batch_of(rng, G, N, K, kinds=KINDS):
    nat = natives(rng, G, K)
    rows = [design_of(rng, nat, g, kinds[(g * N + r) % len(kinds)]) for g in range(G) for r in range(N)]
    des = {"seq_idx": np.stack([r[0] for r in rows]), "translations": np.stack([r[1] for r in rows]), "orientations": np.stack([r[2] for r in rows])}
    to = lambda d: {k: torch.from_numpy(v).cuda() for k, v in d.items()}
    return to(des), to(nat)


def points_of(d, atoms):
    return metrics._points(d, atoms).cpu().numpy()


def rows_of(d, lo, hi):
    return {k: v[lo:hi] for k, v in d.items()}


# ------------------------------------------------------------------ evaluate
@pytest.mark.parametrize("with_segments", [False, True])
@pytest.mark.parametrize("N", [1, 5])
@pytest.mark.parametrize("atoms", ["ca", "backbone"])
@pytest.mark.parametrize("K", [128, 256])
def test_evaluate_equals_the_oracle(K, atoms, N, with_segments):
    rng = np.random.default_rng(100 + K + N)
    G = 6
    des, nat = batch_of(rng, G, N, K)
    gen, rm = masks(rng, G, K)
    seg = segments(gen, rm) if with_segments else None
    kw = dict(residue_mask=torch.from_numpy(rm).cuda(), group_size=N, atoms=atoms)
    if with_segments:
        kw.update(segment_idx=torch.from_numpy(seg).cuda(), num_segments=4)
    out = {k: v.cpu().numpy() for k, v in metrics.evaluate(des, nat, torch.from_numpy(gen).cuda(), **kw).items()}
    ref = evaluate_ref(des["seq_idx"].cpu().numpy(), points_of(des, atoms), nat["seq_idx"].cpu().numpy(), points_of(nat, atoms), gen, rm, seg,
                       4 if with_segments else 0, N)
    assert same_bits(out["aar"], ref["aar"])  # an integer count over an integer n, one fp32 division
    assert_in_place(out["rmsd"], ref["rmsd"], "rmsd")
    assert_aligned(out["rmsd_aligned"], ref["rmsd_aligned"], "rmsd_aligned")
    assert set(out) == ({"aar", "rmsd", "rmsd_aligned"} | ({"segment_aar", "segment_rmsd", "segment_rmsd_aligned"} if with_segments else set()))
    if with_segments:
        assert out["segment_aar"].shape == (G * N, 4) and np.isnan(out["segment_rmsd"][:, 3]).all() and np.isnan(out["segment_aar"][:, 3]).all()
        assert not np.isnan(out["segment_rmsd"][:, 1]).any()  # the one-residue segment
        assert np.isnan(out["segment_aar"][:N, 0]).all()  # patch 0 has one counted residue: segments 0 and 2 are empty there
        assert np.array_equal(np.isnan(out["segment_aar"]), np.isnan(ref["segment_aar"]))
        assert same_bits(np.nan_to_num(out["segment_aar"], nan=-1.0), np.nan_to_num(ref["segment_aar"], nan=-1.0))
        assert_in_place(out["segment_rmsd"], ref["segment_rmsd"], "segment_rmsd")
        assert_aligned(out["segment_rmsd_aligned"], ref["segment_rmsd_aligned"], "segment_rmsd_aligned")
        if atoms == "ca":
            assert (out["segment_rmsd_aligned"][:, 1] == 0.0).all()  # one point gives 0
    # the moved native aligns, the mirrored one does not; with one counted residue everything aligns
    kinds = [KINDS[r % len(KINDS)] for r in range(G * N)]
    big = np.repeat((gen & rm).sum(1) >= 4, N)
    for r, kind in enumerate(kinds):
        if kind == "moved":
            assert out["rmsd_aligned"][r] <= 2e-5 and (out["aar"][r] == 1.0)
        if kind == "mirrored" and big[r]:
            assert out["rmsd_aligned"][r] > 0.1
    # a row's result does not depend on how many rows are in the call: patches 2..3 alone give the same bits
    part = dict(kw, residue_mask=kw["residue_mask"][2:4])
    if with_segments:
        part["segment_idx"] = kw["segment_idx"][2:4]
    sub = metrics.evaluate(rows_of(des, 2 * N, 4 * N), rows_of(nat, 2, 4), torch.from_numpy(gen[2:4]).cuda(), **part)
    for k, v in sub.items():
        assert same_bits(np.nan_to_num(v.cpu().numpy(), nan=-1.0), np.nan_to_num(out[k][2 * N:4 * N], nan=-1.0)), k


def test_evaluate_empty_selection_is_nan():
    rng = np.random.default_rng(7)
    des, nat = batch_of(rng, 2, 3, 128)
    gen = np.zeros((2, 128), bool)
    gen[1, 10:20] = True
    out = metrics.evaluate(des, nat, torch.from_numpy(gen).cuda(), group_size=3)
    for k in ("aar", "rmsd", "rmsd_aligned"):
        v = out[k].cpu().numpy()
        assert np.isnan(v[:3]).all() and not np.isnan(v[3:]).any(), k


# ------------------------------------------------------------------ pairwise
def group_batch(rng, G, N, K):
    """Groups of N designs: mostly native + noise, plus an exact copy of design 0, a rigidly moved and a mirrored copy of it when N allows."""
    des, nat = batch_of(rng, G, N, K, kinds=("noise",))
    for g in range(G):
        base = g * N
        x0, O0 = des["translations"][base].double().cpu().numpy(), des["orientations"][base].double().cpu().numpy()
        if N > 1:
            for k in des:
                des[k][base + N - 1] = des[k][base]  # identical rows: the in-place number must be exactly 0
        if N > 3:
            R = rotation(rng)
            des["translations"][base + 1] = torch.from_numpy((x0 @ R.T + 3.0).astype(np.float32)).cuda()
            des["orientations"][base + 1] = torch.from_numpy((O0 @ R.T).astype(np.float32)).cuda()
            des["seq_idx"][base + 1] = des["seq_idx"][base]
            M = np.diag([1.0, 1.0, -1.0])
            des["translations"][base + 2] = torch.from_numpy((x0 @ M).astype(np.float32)).cuda()
            des["orientations"][base + 2] = torch.from_numpy((O0 @ M).astype(np.float32)).cuda()
    return des


def check_pairwise(out, des, gen, rm, N, atoms, aligned, constructed=True):
    """constructed: the designs are group_batch's (design N - 1 a copy of design 0, design 1 a moved and design 2 a mirrored copy)."""
    rmsd, ident = out["rmsd"].cpu().numpy(), out["seq_identity"].cpu().numpy()
    G = gen.shape[0]
    assert rmsd.shape == (G, N, N) and ident.shape == (G, N, N)
    assert same_bits(rmsd, rmsd.transpose(0, 2, 1)) and same_bits(ident, ident.transpose(0, 2, 1))  # entry (i, j) is bitwise entry (j, i)
    d = np.arange(N)
    assert (rmsd[:, d, d] == 0.0).all() and (ident[:, d, d] == 1.0).all()  # the defined diagonal
    ref_r, ref_i = pairwise_ref(des["seq_idx"].cpu().numpy(), points_of(des, atoms), gen, rm, N, aligned)
    assert same_bits(ident, ref_i)
    (assert_aligned if aligned else assert_in_place)(rmsd, ref_r, f"pairwise N = {N} {atoms}")
    if constructed and N > 1 and not aligned:
        assert (rmsd[:, 0, N - 1] == 0.0).all()  # identical rows: exactly 0
    if constructed and N > 3:
        big = (gen & rm).sum(1) >= 4
        if aligned:
            assert (rmsd[:, 0, 1] <= 2e-5).all() and (rmsd[big, 0, 2] > 0.1).all()  # the moved copy aligns, the mirrored one does not
        assert (ident[:, 0, 1] == 1.0).all()
    return rmsd, ident


@pytest.mark.parametrize("aligned", [False, True])
@pytest.mark.parametrize("atoms", ["ca", "backbone"])
@pytest.mark.parametrize("N", [1, 2, 63, 64, 65, 200])
@pytest.mark.parametrize("G", [1, 3])
def test_pairwise_equals_the_oracle(G, N, atoms, aligned):
    rng = np.random.default_rng(1000 * G + N)
    K = 256 if G == 1 else 128
    des = group_batch(rng, G, N, K)
    gen, rm = masks(rng, G, K, lo=2)
    out = metrics.pairwise(des, torch.from_numpy(gen).cuda(), residue_mask=torch.from_numpy(rm).cuda(), group_size=N, atoms=atoms, aligned=aligned)
    check_pairwise(out, des, gen, rm, N, atoms, aligned)


@pytest.mark.parametrize("atoms", ["ca", "backbone"])
def test_pairwise_full_rows_and_empty_patch(atoms):
    """Every residue of a K = 256 patch counted (the longest fp32 sum: 3 072 terms with the backbone), no residue_mask; and a patch
    without a counted residue, which is NaN everywhere, diagonal included."""
    rng = np.random.default_rng(5)
    des = group_batch(rng, 2, 9, 256)
    gen = np.ones((2, 256), bool)
    gen[1] = False
    for aligned in (False, True):
        out = metrics.pairwise(des, torch.from_numpy(gen).cuda(), group_size=9, atoms=atoms, aligned=aligned)
        rmsd, ident = out["rmsd"].cpu().numpy(), out["seq_identity"].cpu().numpy()
        assert np.isnan(rmsd[1]).all() and np.isnan(ident[1]).all()
        ref_r, ref_i = pairwise_ref(des["seq_idx"].cpu().numpy(), points_of(des, atoms), gen, None, 9, aligned)
        assert same_bits(ident[0], ref_i[0])
        (assert_aligned if aligned else assert_in_place)(rmsd[0], ref_r[0], f"full rows {atoms}")


@pytest.mark.parametrize("atoms", ["ca", "backbone"])
def test_pairwise_against_evaluate_and_a_block_of_a_large_call(atoms):
    """pairwise(...)[g, i, j] is evaluate of design i with design j as the native.  The two do NOT share the in-place device function
    (a running fp32 sum per pair there, fp64 sums per row here), so both comparisons are within the bound, not bitwise."""
    rng = np.random.default_rng(11)
    G, N, K = 2, 200, 128
    des = group_batch(rng, G, N, K)
    gen, rm = masks(rng, G, K, lo=3)
    gm_d, rm_d = torch.from_numpy(gen).cuda(), torch.from_numpy(rm).cuda()
    for aligned in (False, True):
        full = metrics.pairwise(des, gm_d, residue_mask=rm_d, group_size=N, atoms=atoms, aligned=aligned)["rmsd"].cpu().numpy()
        for j in (0, 7, 150):
            native = {k: v.view(G, N, *v.shape[1:])[:, j].contiguous() for k, v in des.items()}
            ev = metrics.evaluate(des, native, gm_d, residue_mask=rm_d, group_size=N, atoms=atoms)
            col = ev["rmsd_aligned" if aligned else "rmsd"].cpu().numpy().reshape(G, N)
            keep = np.arange(N) != j  # (the diagonal is defined, not computed)
            (assert_aligned if aligned else assert_in_place)(full[:, keep, j], col[:, keep], f"pairwise vs evaluate, native {j}")
        # designs 10..73 of each group as a group of 64 of their own
        block = {k: v.view(G, N, *v.shape[1:])[:, 10:74].reshape(G * 64, *v.shape[1:]).contiguous() for k, v in des.items()}
        small = metrics.pairwise(block, gm_d, residue_mask=rm_d, group_size=64, atoms=atoms, aligned=aligned)["rmsd"].cpu().numpy()
        (assert_aligned if aligned else assert_in_place)(small, full[:, 10:74, 10:74], "block of a large call")


# ------------------------------------------------------------------ select_diverse
def check_selection(dist, m, score=None, candidates=None):
    out = metrics.select_diverse(dist, m, score=score, candidates=candidates)
    cpu = lambda t: None if t is None else t.cpu().numpy()
    index, min_dist, count, gap = select_ref(cpu(dist), m, cpu(score), cpu(candidates))
    print("smallest gap between the best and the second-best running minimum:", gap)
    assert np.array_equal(out["index"].cpu().numpy(), index), (out["index"].cpu().numpy(), index)
    assert np.array_equal(out["count"].cpu().numpy(), count)
    got = out["min_dist"].cpu().numpy()
    assert np.array_equal(np.isnan(got), np.isnan(min_dist)) and same_bits(np.nan_to_num(got, nan=-1.0), np.nan_to_num(min_dist, nan=-1.0))
    assert out["index"].dtype == torch.int64 and out["min_dist"].dtype == torch.float32 and out["count"].dtype == torch.int32
    return index, count


def test_select_diverse_equals_the_oracle():
    rng = np.random.default_rng(21)
    G, N, K = 3, 200, 128
    des = group_batch(rng, G, N, K)
    gen, rm = masks(rng, G, K, lo=5)
    out = metrics.pairwise(des, torch.from_numpy(gen).cuda(), residue_mask=torch.from_numpy(rm).cuda(), group_size=N)
    check_selection(out["rmsd"], 16)
    check_selection(1.0 - out["seq_identity"], 16)  # few distinct values: ties everywhere
    score = torch.from_numpy(rng.normal(size=(G, N)).astype(np.float32)).cuda()
    score[0, 5] = score[0, 3] = score[0].min() - 1.0  # a tie for the lowest score: design 3 starts
    score[1, 0] = float("nan")
    index, _ = check_selection(out["rmsd"], 8, score=score)
    assert index[0, 0] == 3
    cand = torch.zeros(G, N, dtype=torch.bool).cuda()
    cand[0, [4, 9, 100]] = True
    cand[1, 50:] = True
    index, count = check_selection(out["rmsd"], 6, score=score, candidates=cand)
    assert count.tolist() == [3, 6, 0] and index[0, 3:].tolist() == [-1, -1, -1] and (index[2] == -1).all()
    check_selection(out["rmsd"], 0)


@pytest.mark.parametrize("N", [300, 1500, 4096])
def test_select_diverse_on_a_grid_of_ties(N):
    """Distances on a 0.25 grid: ties in every round, decided by the lower index; N above 1 024 gives every thread several designs."""
    rng = np.random.default_rng(N)
    a = (rng.integers(0, 24, (2, N, N)) * 0.25).astype(np.float32)
    d = np.maximum(a, a.transpose(0, 2, 1))
    d[:, np.arange(N), np.arange(N)] = 0.0
    d[1, 3, 7] = d[1, 7, 3] = np.nan  # counts as 0
    check_selection(torch.from_numpy(d).cuda(), 40)


# ------------------------------------------------------------------ end to end
def test_sample_evaluate_pairwise_select():
    """sample(num_samples = 8) on the synthetic benchmark model -> evaluate -> pairwise -> select_diverse(m = 3) runs on the sampler's own
    tensors and matches the oracle on them (no claim about the values: the weights are untrained)."""
    dims = dict(syn.BENCH_DIMS, NL=2)
    model = DiffAb(dims["D"], dims["C"], dims["NL"], dims["DS"], dims["PQ"], dims["PV"], dims["H"]).cuda()
    model.denoiser.load_state_dict(syn.denoiser_state_dict(dims, seed=1, prefix=""))
    inp = {k: v.cuda() for k, v in syn.patches(2, 128, dims, seed=3, coord_sigma=8.0).items()}
    N = 8
    res = model.sample(inp["seq_idx"], inp["translations"], inp["orientations"], res_context_emb=inp["res_context_emb"],
                       pair_context_emb=inp["pair_context_emb"], generation_mask=inp["generation_mask"], seed=1, t_start=100, t_stop=90,
                       num_samples=N)
    gen = inp["generation_mask"].cpu().numpy()
    for atoms in ("ca", "backbone"):
        ev = metrics.evaluate(res, inp, inp["generation_mask"], residue_mask=inp["residue_mask"], group_size=N, atoms=atoms)
        ref = evaluate_ref(res["seq_idx"].cpu().numpy(), points_of(res, atoms), inp["seq_idx"].cpu().numpy(), points_of(inp, atoms), gen, None, None, 0, N)
        assert same_bits(ev["aar"].cpu().numpy(), ref["aar"])
        assert_in_place(ev["rmsd"].cpu().numpy(), ref["rmsd"], "sampled rmsd")
        assert_aligned(ev["rmsd_aligned"].cpu().numpy(), ref["rmsd_aligned"], "sampled rmsd_aligned")
        assert ev["aar"].is_cuda and ev["aar"].shape == (2 * N,)
        for aligned in (False, True):
            pw = metrics.pairwise(res, inp["generation_mask"], group_size=N, atoms=atoms, aligned=aligned)
            check_pairwise(pw, res, gen, np.ones_like(gen), N, atoms, aligned, constructed=False)
            index, count = check_selection(pw["rmsd"], 3, score=ev["rmsd"].view(2, N))
            assert count.tolist() == [3, 3] and (index >= 0).all()
