"""CPU: the host side of the design metrics (diffab_pytorch.metrics, io.chothia_cdr_index) - the float64 numpy oracle of the three rules
and its self-checks, the C-ABI entries and their host-side refusals, and the argument checks that happen before any library call.

The rules are DESIGN.md section 4.13 / include/diffab_hip.h (diffab_metrics_vs_native, diffab_metrics_pairwise,
diffab_metrics_select_diverse).  test_gpu_metrics.py imports the oracle from here."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from diffab_pytorch import _hip, io as dio, metrics
from sampler_support import ReachedTheLibrary, refuse_library

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------ the oracle (shared with test_gpu_metrics.py)
def kabsch_msd(p, q):
    """The definition: centre both (m,3) sets, H = P^T Q, singular values s1 >= s2 >= s3, d = sign(det H) (+1 at 0),
    msd = max(0, sum |p|^2 + sum |q|^2 - 2 (s1 + s2 + d s3)) / m."""
    p = np.asarray(p, np.float64) - np.mean(np.asarray(p, np.float64), 0)
    q = np.asarray(q, np.float64) - np.mean(np.asarray(q, np.float64), 0)
    h = p.T @ q
    s = np.linalg.svd(h, compute_uv=False)
    d = -1.0 if np.linalg.det(h) < 0 else 1.0
    return max(0.0, (p * p).sum() + (q * q).sum() - 2.0 * (s[0] + s[1] + d * s[2])) / p.shape[0]


def three_numbers(seq, pts, nseq, npts, sel):
    """(aar as the fp32 quotient, rmsd, rmsd_aligned, n, matches) over the residues `sel` (K,) of one design: pts (K,P,3)."""
    n = int(sel.sum())
    if n == 0:
        return np.float32(np.nan), np.nan, np.nan, 0, 0
    p, q = np.asarray(pts, np.float64)[sel].reshape(-1, 3), np.asarray(npts, np.float64)[sel].reshape(-1, 3)
    matches = int((np.asarray(seq)[sel] == np.asarray(nseq)[sel]).sum())
    return np.float32(matches) / np.float32(n), np.sqrt(((p - q) ** 2).sum() / p.shape[0]), np.sqrt(kabsch_msd(p, q)), n, matches


def evaluate_ref(seq, pts, nseq, npts, gen, residue_mask=None, segment_idx=None, S=0, group_size=1):
    """seq (rows,K), pts (rows,K,P,3), nseq (G,K), npts (G,K,P,3), masks (G,K) -> dict of aar (fp32), rmsd, rmsd_aligned (float64),
    (rows,), and segment_* (rows,S)."""
    rows = seq.shape[0]
    out = {"aar": np.zeros(rows, np.float32), "rmsd": np.zeros(rows), "rmsd_aligned": np.zeros(rows),
           "segment_aar": np.zeros((rows, S), np.float32), "segment_rmsd": np.zeros((rows, S)), "segment_rmsd_aligned": np.zeros((rows, S))}
    for r in range(rows):
        g = r // group_size
        counted = np.asarray(gen[g], bool) & (True if residue_mask is None else np.asarray(residue_mask[g], bool))
        out["aar"][r], out["rmsd"][r], out["rmsd_aligned"][r], _, _ = three_numbers(seq[r], pts[r], nseq[g], npts[g], counted)
        for s in range(S):
            sel = counted & (np.asarray(segment_idx[g]) == s)
            out["segment_aar"][r, s], out["segment_rmsd"][r, s], out["segment_rmsd_aligned"][r, s], _, _ = \
                three_numbers(seq[r], pts[r], nseq[g], npts[g], sel)
    return out


def pairwise_ref(seq, pts, gen, residue_mask=None, group_size=1, aligned=False):
    """-> rmsd (G,N,N) float64, seq_identity (G,N,N) fp32 (the fp32 quotient); the diagonal is 0 / 1 by definition."""
    N = group_size
    G = seq.shape[0] // N
    rmsd, ident = np.zeros((G, N, N)), np.zeros((G, N, N), np.float32)
    for g in range(G):
        counted = np.asarray(gen[g], bool) & (True if residue_mask is None else np.asarray(residue_mask[g], bool))
        n = int(counted.sum())
        if n == 0:
            rmsd[g], ident[g] = np.nan, np.nan
            continue
        p = np.asarray(pts[g * N:(g + 1) * N], np.float64)[:, counted].reshape(N, -1, 3)
        s = np.asarray(seq[g * N:(g + 1) * N])[:, counted]
        ident[g] = (s[:, None, :] == s[None, :, :]).sum(-1).astype(np.float32) / np.float32(n)
        if aligned:
            for i in range(N):
                for j in range(i + 1, N):
                    rmsd[g, i, j] = rmsd[g, j, i] = np.sqrt(kabsch_msd(p[i], p[j]))
        else:
            rmsd[g] = np.sqrt(((p[:, None] - p[None, :]) ** 2).sum((-1, -2)) / p.shape[1])
        np.fill_diagonal(rmsd[g], 0.0)
        np.fill_diagonal(ident[g], 1.0)
    return rmsd, ident


def select_ref(dist, m, score=None, candidates=None):
    """dist (G,N,N) fp32 -> index (G,m) int64, min_dist (G,m) fp32, count (G,), gap: the smallest difference between the best and the
    second-best running minimum over all rounds (inf when no round had two candidates) - printed by the tests, never asserted."""
    dist = np.asarray(dist, np.float32)
    G, N = dist.shape[:2]
    index, min_dist, count, gap = np.full((G, m), -1, np.int64), np.full((G, m), np.nan, np.float32), np.zeros(G, np.int32), np.inf
    for g in range(G):
        open_ = np.ones(N, bool) if candidates is None else np.asarray(candidates[g], bool).copy()
        run = np.full(N, np.inf, np.float32)
        for k in range(m):
            where = np.flatnonzero(open_)
            if where.size == 0:
                break
            if k == 0:
                key = np.zeros(N, np.float32) if score is None else -np.where(np.isnan(score[g]), np.inf, score[g]).astype(np.float32)
            else:
                key = run
            best = where[np.argmax(key[where])]  # argmax returns the first maximum: ties to the lower index
            if k > 0 and where.size > 1:
                top = np.sort(key[where])[-2:]
                gap = min(gap, float(top[1] - top[0])) if np.isfinite(top).all() else gap
            index[g, k], min_dist[g, k] = best, (np.inf if k == 0 else run[best])
            open_[best] = False
            run = np.minimum(run, np.where(np.isnan(dist[g, best]), np.float32(0), dist[g, best]))
            count[g] = k + 1
    return index, min_dist, count, gap


# ------------------------------------------------------------------ self-checks of the oracle
def rotation(rng):
    q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
    return q * np.sign(np.linalg.det(q))


def cloud(rng, K=24, P=4):
    return (rng.normal(0.0, 6.0, (K, 1, 3)) + rng.normal(0.0, 1.0, (K, P, 3)) + np.array([30.0, -20.0, 10.0])).astype(np.float32)


def test_oracle_superposition_and_mirror():
    rng = np.random.default_rng(0)
    nat = cloud(rng)
    seq = rng.integers(0, 20, 24)
    sel = np.zeros(24, bool)
    sel[3:17] = True
    moved = nat.astype(np.float64) @ rotation(rng).T + np.array([4.0, -7.0, 2.5])
    aar, rmsd, aligned, n, matches = three_numbers(seq, moved, seq, nat, sel)
    assert aar == 1.0 and n == 14 and matches == 14
    assert aligned <= 1e-6 and rmsd > 1.0  # a rigid motion leaves the aligned number at 0 and changes the in-place one
    mirrored = nat.astype(np.float64) * np.array([1.0, 1.0, -1.0])
    assert three_numbers(seq, mirrored, seq, nat, sel)[2] > 0.5  # a mirror image does NOT align to 0
    same = three_numbers(seq, nat, seq, nat, sel)
    assert same[1] == 0.0 and same[2] <= 1e-6  # (the root of float64's own rounding of an msd of 0)
    one = np.zeros(24, bool)
    one[5] = True
    assert three_numbers(seq, moved[:, :1], seq, nat[:, :1], one)[2] == 0.0  # one point gives 0
    assert np.isnan(three_numbers(seq, moved, seq, nat, np.zeros(24, bool))[1])


def test_oracle_segments_recombine_to_the_row():
    rng = np.random.default_rng(1)
    nat, des = cloud(rng)[None], (cloud(rng) + rng.normal(0, 1.5, (24, 4, 3)).astype(np.float32))[None]
    nseq = rng.integers(0, 20, (1, 24))
    seq = np.where(rng.random((1, 24)) < 0.5, nseq, (nseq + 1) % 20)
    gen = np.zeros((1, 24), bool)
    gen[0, 2:20] = True
    seg = np.full((1, 24), -1)
    seg[0, 2:9], seg[0, 9:10], seg[0, 10:20] = 0, 1, 2  # every counted residue has a label; segment 3 is empty
    out = evaluate_ref(seq, des, nseq, nat, gen, segment_idx=seg, S=4)
    sizes = np.array([7, 1, 10, 0])
    assert np.isnan(out["segment_rmsd"][0, 3]) and np.isnan(out["segment_aar"][0, 3])
    msd = np.nansum(out["segment_rmsd"][0] ** 2 * sizes) / sizes.sum()
    assert abs(np.sqrt(msd) - out["rmsd"][0]) < 1e-12
    assert abs(np.nansum(out["segment_aar"][0].astype(np.float64) * sizes) / sizes.sum() - float(out["aar"][0])) < 1e-6
    assert out["segment_rmsd_aligned"][0, 1] > 0.0  # four points of an unrelated residue do not align exactly; one POINT does:
    ca = evaluate_ref(seq, des[:, :, 1:2], nseq, nat[:, :, 1:2], gen, segment_idx=seg, S=4)
    assert ca["segment_rmsd_aligned"][0, 1] == 0.0 and ca["segment_rmsd"][0, 1] > 0.0


def test_oracle_pairwise_and_selection_on_hand_cases():
    rng = np.random.default_rng(2)
    pts = np.stack([cloud(rng, 16, 1) for _ in range(5)])
    seq = rng.integers(0, 20, (5, 16))
    seq[3] = seq[1]
    gen = np.zeros((1, 16), bool)
    gen[0, 4:12] = True
    rmsd, ident = pairwise_ref(seq, pts, gen, group_size=5)
    assert np.array_equal(rmsd, rmsd.transpose(0, 2, 1)) and ident[0, 1, 3] == 1.0 and (np.diag(rmsd[0]) == 0).all()
    al, _ = pairwise_ref(seq, pts, gen, group_size=5, aligned=True)
    assert (al <= rmsd + 1e-12).all()
    # four designs on a line at 0, 1, 3, 7: from design 0 the farthest is 3 (7), then 2 (min(3, 4) = 3), then 1 (1)
    x = np.array([0.0, 1.0, 3.0, 7.0], np.float32)
    d = np.abs(x[:, None] - x[None, :])[None]
    index, md, count, _ = select_ref(d, 5)
    assert index.tolist() == [[0, 3, 2, 1, -1]] and count.tolist() == [4] and md[0, :4].tolist() == [np.inf, 7.0, 3.0, 1.0] and np.isnan(md[0, 4])
    # the lowest score starts; ties go to the lower index: from 2 the designs 0 and ... 3 (4) beats 0 (3); then 0 (3) ; then 1
    assert select_ref(d, 3, score=np.array([[2.0, 1.0, 0.5, 0.5]], np.float32))[0].tolist() == [[2, 3, 0]]
    tie = np.array([[0, 2, 2], [2, 0, 2], [2, 2, 0]], np.float32)[None]
    assert select_ref(tie, 3)[0].tolist() == [[0, 1, 2]]
    assert select_ref(d, 3, candidates=np.array([[False, True, False, True]]))[0].tolist() == [[1, 3, -1]]


# ------------------------------------------------------------------ C ABI
NAMES = ("diffab_metrics_vs_native", "diffab_metrics_pairwise", "diffab_metrics_select_diverse")


def test_header_and_symbol_table_declare_the_three_entries():
    src = open(os.path.join(REPO, "include", "diffab_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    lib = _hip.load_library()
    for name in NAMES:
        assert re.search(r"\bint\s+" + name + r"\s*\(", code), name
        assert name in _hip.SYMBOLS and hasattr(lib, name), name
        res, args = _hip.SYMBOLS[name]
        assert res is ctypes.c_int and args[-1] is ctypes.c_void_p
    vs, pw, sel = (_hip.SYMBOLS[n][1] for n in NAMES)
    assert len(vs) == 19 and vs[7:12] == [ctypes.c_int32] * 5 and all(a is ctypes.c_void_p for a in vs[:7] + vs[12:])
    assert len(pw) == 14 and pw[4:9] == [ctypes.c_int32] * 5 and pw[12] is ctypes.c_size_t
    assert len(sel) == 10 and sel[3:6] == [ctypes.c_int32] * 3
    limits = {k: int(v) for k, v in re.findall(r"#define\s+DIFFAB_METRICS_(MAX_[A-Z]+)\s+(\d+)", code)}
    assert limits == {"MAX_GROUP": metrics.MAX_GROUP, "MAX_K": metrics.MAX_K, "MAX_POINTS": 5, "MAX_SEGMENTS": metrics.MAX_SEGMENTS}
    assert limits["MAX_GROUP"] == 4096 and limits["MAX_SEGMENTS"] == 8


def test_host_side_refusals_touch_no_gpu():
    """Every refusal is decided from the scalar arguments and whether a pointer is null: the pointers are fake addresses that are never
    dereferenced, nothing is enqueued (no GPU is needed), and diffab_last_error names the problem."""
    l = _hip.load_library()
    p, null = ctypes.c_void_p(4096), ctypes.c_void_p(0)

    def err():
        return l.diffab_last_error().decode()

    def vs(rows=10, group=5, K=128, P=1, S=0, seg=null, seq=p, out=p, seg_out=p):
        return l.diffab_metrics_vs_native(seq, p, p, p, p, null, seg, rows, group, K, P, S, out, p, p, seg_out, p, p, null)

    for kw, word in ((dict(rows=11), "not a multiple"), (dict(P=0), "points per residue"), (dict(P=6), "points per residue"),
                     (dict(S=9, seg=p), "segments outside"), (dict(S=-1), "segments outside"), (dict(S=2), "needs a segment_idx"),
                     (dict(seg=p), "NULL segment_idx"), (dict(group=0), "extent"), (dict(group=4097, rows=4097), "at most 4096 designs"),
                     (dict(K=0), "extent"), (dict(K=4097), "at most 4096"), (dict(rows=-5), "extent"), (dict(seq=null), "null input"),
                     (dict(out=null), "null output"), (dict(S=2, seg=p, seg_out=null), "null segment output")):
        rc = vs(**kw)
        assert rc == -1 and word in err(), (kw, rc, err())

    def pw(G=2, N=8, K=128, P=4, aligned=0, ws=p, ws_bytes=1 << 40, seq=p, out=p):
        return l.diffab_metrics_pairwise(seq, p, p, null, G, N, K, P, aligned, out, p, ws, ws_bytes, null)

    for kw, word in ((dict(N=4097), "at most 4096 designs"), (dict(N=0), "extent"), (dict(G=-1), "extent"), (dict(P=6), "points per residue"),
                     (dict(K=5000), "at most 4096"), (dict(aligned=2), "aligned must be"), (dict(seq=null), "null input"),
                     (dict(out=null), "null output"), (dict(ws=null), "workspace"), (dict(ws=ctypes.c_void_p(4100)), "16-byte aligned")):
        rc = pw(**kw)
        assert rc == -1 and word in err(), (kw, rc, err())
    need = metrics.pairwise_workspace_bytes(2, 8, 128, 4)
    assert pw(ws_bytes=need // 2) == -4 and "needed" in err()  # DIFFAB_ERR_WORKSPACE
    asked = int(re.search(r"(\d+) needed", err()).group(1))
    assert need - 2048 <= asked <= need  # the header's macro covers the carves and no more than their alignment on top

    def sel(G=2, N=8, m=3, dist=p, out=p, count=p):
        return l.diffab_metrics_select_diverse(dist, null, null, G, N, m, out, p, count, null)

    for kw, word in ((dict(N=4097), "at most 4096"), (dict(N=0), "extent"), (dict(G=-1), "extent"), (dict(m=-1), "m must be"),
                     (dict(dist=null), "null dist"), (dict(out=null), "null output"), (dict(count=null), "null output")):
        rc = sel(**kw)
        assert rc == -1 and word in err(), (kw, rc, err())
    # empty problems return 0 before any pointer is looked at
    assert l.diffab_metrics_vs_native(*[null] * 7, 0, 5, 128, 1, 0, *[null] * 7) == 0
    assert l.diffab_metrics_pairwise(*[null] * 4, 0, 8, 128, 1, 0, null, null, null, 0, null) == 0
    assert l.diffab_metrics_select_diverse(null, null, null, 0, 8, 3, null, null, null, null) == 0


# ------------------------------------------------------------------ argument errors before any device work
@pytest.fixture
def no_library(monkeypatch):
    refuse_library(monkeypatch)


def frames(rows=6, K=16):
    return {"seq_idx": torch.zeros(rows, K, dtype=torch.long), "translations": torch.zeros(rows, K, 3),
            "orientations": torch.eye(3).expand(rows, K, 3, 3)}


def mask(G=2, K=16):
    m = torch.zeros(G, K, dtype=torch.bool)
    m[:, 3:9] = True
    return m


def test_good_arguments_reach_the_library(no_library):
    with pytest.raises(ReachedTheLibrary):
        metrics.evaluate(frames(), frames(2), mask(), group_size=3, atoms="backbone", segment_idx=torch.zeros(2, 16, dtype=torch.long))
    with pytest.raises(ReachedTheLibrary):
        metrics.pairwise(frames(), mask(), group_size=3, aligned=True)
    with pytest.raises(ReachedTheLibrary):
        metrics.select_diverse(torch.zeros(2, 5, 5), 3, score=torch.zeros(2, 5), candidates=torch.ones(2, 5, dtype=torch.bool))


@pytest.mark.parametrize("kw, match", [
    (dict(atoms="cb"), "atoms must be 'ca' or 'backbone'"), (dict(group_size=4), "6 design rows are not a multiple of group_size = 4"),
    (dict(group_size=0), "group_size must be"), (dict(group_size=True), "group_size must be"),
    (dict(generation_mask=mask().long()), "generation_mask must be a bool tensor"), (dict(generation_mask=mask(3)), "generation_mask is"),
    (dict(residue_mask=mask(2, 15)), "residue_mask is"), (dict(residue_mask=mask().float()), "residue_mask must be a bool tensor"),
    (dict(designs={"seq_idx": torch.zeros(6, 16, dtype=torch.long)}), "designs must be a dict"),
    (dict(designs=dict(frames(), seq_idx=torch.zeros(6, 16))), r"designs\['seq_idx'\] must be an integer tensor"),
    (dict(designs=dict(frames(), translations=torch.zeros(6, 15, 3))), r"designs\['translations'\] is"),
    (dict(designs=dict(frames(), orientations=torch.zeros(6, 16, 3)), atoms="backbone"), r"designs\['orientations'\] must be"),
])
def test_common_argument_errors(no_library, kw, match):
    args = dict(designs=frames(), generation_mask=mask(), group_size=3)
    args.update(kw)
    designs = args.pop("designs")
    gm = args.pop("generation_mask")
    with pytest.raises(ValueError, match=match):
        metrics.evaluate(designs, frames(2), gm, **args)
    with pytest.raises(ValueError, match=match):
        metrics.pairwise(designs, gm, **args)


def test_evaluate_pairwise_and_select_argument_errors(no_library):
    with pytest.raises(ValueError, match=r"native\['seq_idx'\] is \(3, 16\)"):
        metrics.evaluate(frames(), frames(3), mask(), group_size=3)
    with pytest.raises(ValueError, match="native must be a dict"):
        metrics.evaluate(frames(), None, mask(), group_size=3)
    with pytest.raises(ValueError, match="segment_idx must be an integer tensor"):
        metrics.evaluate(frames(), frames(2), mask(), group_size=3, segment_idx=torch.zeros(2, 16))
    with pytest.raises(ValueError, match="segment_idx is"):
        metrics.evaluate(frames(), frames(2), mask(), group_size=3, segment_idx=torch.zeros(2, 15, dtype=torch.long))
    with pytest.raises(ValueError, match=r"num_segments = 9 .* outside \[1, 8\]"):
        metrics.evaluate(frames(), frames(2), mask(), group_size=3, segment_idx=torch.full((2, 16), 8))
    with pytest.raises(ValueError, match="num_segments without segment_idx"):
        metrics.evaluate(frames(), frames(2), mask(), group_size=3, num_segments=2)
    with pytest.raises(ValueError, match="at most 4096 designs"):
        metrics.pairwise(frames(4097, 4), mask(1, 4), group_size=4097)
    with pytest.raises(ValueError, match="aligned must be a bool"):
        metrics.pairwise(frames(), mask(), group_size=3, aligned=1)
    for dist in (torch.zeros(2, 5, 4), torch.zeros(5, 5), torch.zeros(2, 5, 5, dtype=torch.float64)):
        with pytest.raises(ValueError, match="dist must be a float32 tensor"):
            metrics.select_diverse(dist, 2)
    with pytest.raises(ValueError, match="outside"):
        metrics.select_diverse(torch.zeros(1, 4097, 4097), 2)
    with pytest.raises(ValueError, match="m must be"):
        metrics.select_diverse(torch.zeros(2, 5, 5), -1)
    with pytest.raises(ValueError, match="score must be"):
        metrics.select_diverse(torch.zeros(2, 5, 5), 2, score=torch.zeros(2, 4))
    with pytest.raises(ValueError, match="candidates must be"):
        metrics.select_diverse(torch.zeros(2, 5, 5), 2, candidates=torch.ones(2, 5))


# ------------------------------------------------------------------ io.chothia_cdr_index
def test_chothia_cdr_index_agrees_with_the_mask():
    h = [25, 26, 32, 33, 51, 52, 56, 57, 94, 95, 100, 100, 100, 102, 103]  # range ends, and 100, 100A, 100B by their number
    l = [23, 24, 34, 35, 49, 50, 56, 57, 88, 89, 97, 98]
    chain = torch.tensor([1] * len(h) + [2] * len(l) + [3, 3, 0])
    resseq = torch.tensor(h + l + [96, 30, 27])
    want = [-1, 0, 0, -1, -1, 1, 1, -1, -1, 2, 2, 2, 2, 2, -1] + [-1, 3, 3, -1, -1, 4, 4, -1, -1, 5, 5, -1] + [-1, -1, -1]
    got = dio.chothia_cdr_index(chain, resseq)
    assert got.dtype == torch.int64 and got.tolist() == want
    assert torch.equal(got >= 0, dio.chothia_cdr_mask(chain, resseq))
    g = torch.Generator().manual_seed(0)
    chain, resseq = torch.randint(0, 4, (3, 200), generator=g), torch.randint(1, 120, (3, 200), generator=g)
    index = dio.chothia_cdr_index(chain, resseq)
    assert torch.equal(index >= 0, dio.chothia_cdr_mask(chain, resseq))
    for label, name in enumerate(("H1", "H2", "H3", "L1", "L2", "L3")):
        assert torch.equal(index == label, dio.chothia_cdr_mask(chain, resseq, cdrs=(name,)))
    with pytest.raises(ValueError, match="chain_idx is"):
        dio.chothia_cdr_index(chain, resseq[:, :-1])
