"""Loop conformations on the MI355X: metrics.conformation / diffab_metrics_dihedral_nearest and
metrics.design_dihedrals / diffab_metrics_pack_dihedrals against the numpy restatement of conformation_ref.py, their properties and
their contracts.

EXACT cases: features on the dyadic grid k / 128, |k| <= 128.  Every product is a multiple of 2^-14 and every partial sum of up to 384
of them is below 2^9, so every partial sum is exact in fp32 in any order, and EVERY output must equal the restatement bit for bit,
whatever path the kernel took.  REAL-VALUED cases: cos / sin of uniform random angles; every finite distance must be within

    bound = 2 (n_k + 2) u * sum|q l| / n + 8 u,   u = 2^-24, n_k = 2 A len,

of the float64 restatement (the gamma bound of an n_k-term chain plus one rounding each for the division and the subtraction; DESIGN
4.27 has the derivation), and the index rules of check_real hold.  The restatement's own hand-made cases are in
tests/test_conformation_host.py.  R * M of a case stays at or below about 3 x 10^5."""
import functools

import numpy as np
import pytest
import torch

import sampler_support
from conformation_ref import PER_QUERY, U, bound, clamp, features, nearest_ref, pack_ref, pair_matrix, same_bits
from diffab_pytorch import _hip, metrics
from sampler_support import GuardedABI, header_prototypes, hip, misaligned
from scratch_poison import poisoned

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("hip")]

cuda = lambda v: torch.from_numpy(np.ascontiguousarray(v)).cuda()
numpy_of = lambda out: {k: v.cpu().numpy() for k, v in out.items()}
OUTPUTS = ("distance", "index", "n_terms", "n_within", "matrix")
LENGTHS = (1, 2, 15, 16, 17, 31, 32, 33, 63, 64)  # every bucket boundary of the sort and every k-step boundary of the product
ABSENT = 5                                        # a length no library of these tests holds
GARBAGE = np.float32(3e30)


# ------------------------------------------------------------------ inputs
def behind(feat, lengths):
    """Finite garbage and NaN, alternating, in the slots past each clamped length: never read."""
    n, L = feat.shape[:2]
    past = np.arange(L)[None, :] >= clamp(lengths, L)[:, None]
    fill = np.where(np.arange(feat[0].size).reshape(feat.shape[1:]) % 3 == 0, np.float32(np.nan), GARBAGE)
    feat[past] = np.broadcast_to(fill, feat.shape)[past]
    return feat


def grid_loops(rng, lengths, L, A, holes=0.05):
    """(feat (n, L, A, 2) float32 on the grid k / 128, lengths int32): a share `holes` of the terms undefined - a NaN cos, a NaN sin, an
    infinite cos or both NaN."""
    lengths = np.asarray(lengths, np.int32)
    feat = (rng.integers(-128, 129, (len(lengths), L, A, 2)) / 128.0).astype(np.float32)
    hit = rng.random(feat.shape[:3]) < holes
    kind = rng.integers(0, 4, feat.shape[:3])
    feat[..., 0][hit & (kind == 0)] = np.nan
    feat[..., 1][hit & (kind == 1)] = np.nan
    feat[..., 0][hit & (kind == 2)] = np.inf
    feat[hit & (kind == 3)] = np.nan
    return behind(feat, lengths), lengths


def plant(rng, qf, nq, lf, nl, share=0.2):
    """A share of the library replaced by queries (their first len slots), at random places: ties between the copies of one query, and
    every copied query has a near entry.  Entries narrower than the query's length are left alone, and a query of length ABSENT is not copied."""
    LQ, LM = qf.shape[1], lf.shape[1]
    for k, m in enumerate(rng.choice(len(lf), max(1, int(len(lf) * share)), replace=False)):
        r = k % len(qf)
        n = int(clamp(nq[r:r + 1], LQ)[0])
        if n <= LM and nq[r] != ABSENT:
            lf[m, :n], nl[m] = qf[r, :n], n
    behind(lf, nl)


@functools.lru_cache(maxsize=None)
def exact_case(A, R, M, LQ, LM, seed=0):
    rng = np.random.default_rng(1000 * A + 10 * R + M + seed)
    pick = lambda width, n: rng.choice([v for v in LENGTHS if v <= width], n)
    nq, nl = pick(LQ, R), pick(LM, M)
    if R >= 15:
        nq[1], nq[2], nq[3], nq[4] = ABSENT, LQ + 1000, -7, 0  # a length the library does not hold, lengths outside the row, an empty loop
    if M >= 63:
        nl[0], nl[1], nl[2], nl[3] = 2 ** 31 - 1, -1, 0, 0
    (qf, nq), (lf, nl) = grid_loops(rng, nq, LQ, A), grid_loops(rng, nl, LM, A)
    if M >= 63:  # a loop with an undefined term in every word of the masks, first and last slot, on either side and on both
        wide = int(np.argmax(clamp(nl, LM)))
        lf[wide, [0, clamp(nl, LM)[wide] - 1]] = np.nan
        qf[0, 0, :, 1] = np.nan
    plant(rng, qf, nq, lf, nl)
    if M >= 63:
        lf[M // 2], nl[M // 2] = lf[M // 3], nl[M // 3]  # two entries that are the same loop
    skip = rng.integers(-1, M + 2, R).astype(np.int64)
    skip[0] = 2 ** 31 - 1
    return qf, nq, lf, nl, skip


def raw_nearest(qf, nq, lf, nl, skip=None, radius=2.0, min_terms=1, leave=(), shifted=False):
    """diffab_metrics_dihedral_nearest on device operands, through whatever stands in for _hip.lib(): the features go in unchanged."""
    place = lambda t: misaligned(t, 4) if shifted else t
    (R, LQ, A, _), (M, LM) = qf.shape, lf.shape[:2]
    ops = [cuda(qf), cuda(np.asarray(nq, np.int32)), cuda(lf), cuda(np.asarray(nl, np.int32)),
           None if skip is None else cuda(np.clip(np.asarray(skip, np.int64), -1, 2 ** 31 - 1).astype(np.int32))]
    ops = [None if t is None else place(t) for t in ops]
    shapes = {"distance": (R,), "index": (R,), "n_terms": (R,), "n_within": (R,), "matrix": (R, M)}
    out = {k: place(torch.empty(s, dtype=torch.float32 if k in ("distance", "matrix") else torch.int32, device="cuda")) for k, s in shapes.items() if k not in leave}
    nbytes = metrics.dihedral_nearest_workspace_bytes(R, M, LQ, LM, A)
    ws = _hip.workspace(nbytes)
    lib_ = _hip.lib()
    rc = lib_.diffab_metrics_dihedral_nearest(_hip.ptr(ops[0]), _hip.ptr(ops[1]), R, LQ, _hip.ptr(ops[2]), _hip.ptr(ops[3]), M, LM, A, _hip.ptr(ops[4]),
                                              float(radius), min_terms, *[_hip.ptr(out.get(k)) for k in OUTPUTS], _hip.ptr(ws), nbytes, _hip.stream_ptr())
    assert rc == 0, _hip.load_library().diffab_last_error().decode()
    torch.cuda.synchronize()
    return numpy_of(out)


def restated(qf, nq, lf, nl, skip=None, radius=2.0, min_terms=1):
    d, n, _, d32 = pair_matrix(qf, nq, lf, nl, min_terms)
    return nearest_ref(d32, n, skip=skip, radius=radius)


def check(got, want, what, only=OUTPUTS):
    for k in only:
        if k in got:
            assert same_bits(got[k], want[k]), (what, k, got[k], want[k])


def compare(qf, nq, lf, nl, what, skip=None, radius=2.0, min_terms=1):
    """The device against the restatement, bit for bit, and the per-query outputs against the device's own matrix."""
    want = restated(qf, nq, lf, nl, skip, radius, min_terms)
    got = raw_nearest(qf, nq, lf, nl, skip, radius, min_terms)
    check(got, want, what)
    n = pair_matrix(qf, nq, lf, nl, min_terms)[1]
    check(got, nearest_ref(got["matrix"], n, skip=skip, radius=radius), what + " (from the device matrix)", only=PER_QUERY)
    return got, want


# ------------------------------------------------------------------ (a) exact: bit for bit
EXACT = [(1, 1, 1, 64, 64), (2, 15, 63, 64, 64), (3, 16, 64, 37, 64), (1, 17, 65, 64, 35), (2, 65, 1000, 64, 64), (3, 65, 4097, 64, 64), (2, 1, 4097, 33, 64),
         (3, 17, 1000, 64, 17), (1, 65, 4097, 2, 64)]


@pytest.mark.parametrize("A, R, M, LQ, LM", EXACT)
def test_grid_features_equal_the_restatement_bit_for_bit(A, R, M, LQ, LM):
    qf, nq, lf, nl, skip = exact_case(A, R, M, LQ, LM)
    got, want = compare(qf, nq, lf, nl, f"A={A} R={R} M={M}", skip=skip)
    finite = np.isfinite(want["matrix"])
    if R >= 15 and M >= 63:
        assert finite.any() and not finite.all() and (want["index"] >= 0).any() and np.isinf(want["distance"][[1, 4] if LQ >= ABSENT else [4]]).all()
        assert want["n_within"].any() and (want["n_within"] < M).all()
    if LQ == 64 and LM == 64 and M >= 63:
        assert set(clamp(nl, LM)) >= set(LENGTHS)


def test_radius_and_min_terms():
    qf, nq, lf, nl, skip = exact_case(2, 65, 1000, 64, 64)
    d32 = pair_matrix(qf, nq, lf, nl)[3]
    occurs = float(np.sort(d32[np.isfinite(d32)])[200])
    for radius in (0.0, occurs, float(np.nextafter(np.float32(occurs), np.float32(0))), 1e9, float("inf"), -1.0, -0.0, float("nan")):
        got, want = compare(qf, nq, lf, nl, f"radius {radius}", skip=skip, radius=radius)
        if radius < 0 or radius != radius:
            assert not got["n_within"].any()
    assert raw_nearest(qf, nq, lf, nl, skip, radius=occurs)["n_within"].sum() > raw_nearest(qf, nq, lf, nl, skip, radius=float(np.nextafter(np.float32(occurs), np.float32(0))))["n_within"].sum()
    n = pair_matrix(qf, nq, lf, nl)[1]
    comparable = (clamp(nq, 64)[:, None] == clamp(nl, 64)[None, :]) & (n >= 1)
    for min_terms in (2, 4, 30, 124, 129, 2 ** 31 - 1):
        got, want = compare(qf, nq, lf, nl, f"min_terms {min_terms}", skip=skip, min_terms=min_terms)
        assert (np.isfinite(got["matrix"]) == (comparable & (n >= min_terms))).all()
    assert (n[comparable] < 124).any() and (n[comparable] >= 124).any()  # some pairs of full loops fall below 124 terms, some do not


def test_ties_go_to_the_lower_index_across_lanes_waves_tiles_and_chunks():
    rng = np.random.default_rng(11)
    M, places = 4097, [5, 6, 21, 70, 300, 2047, 2048, 4096]
    (qf, nq), (lf, nl) = grid_loops(rng, [16, 16, 33], 40, 2, holes=0), grid_loops(rng, np.full(M, 16), 16, 2, holes=0)
    nl[1000:1100] = 15  # (the sorted places are no longer the indices)
    qf[0, :16] = rng.choice([-1.0, 1.0], (16, 2, 2)).astype(np.float32)  # with its copies t = 2, so d = 0; nothing random comes near
    behind(lf, nl)
    for m in places:
        lf[m], nl[m] = qf[0, :16], 16
    for k, m in enumerate(places):
        got, want = compare(qf, nq, lf, nl, f"skip {m}", skip=np.array([m, -1, 3]), radius=0.0)
        assert got["index"][0] == (places[0] if k else places[1]) and got["distance"][0] == 0 and got["n_within"][0] == len(places) - 1
        assert got["index"][2] == -1 and got["n_within"][2] == 0
    got, _ = compare(qf, nq, lf, nl, "no skip", radius=0.0)
    assert got["index"][0] == 5 and got["n_within"][0] == len(places) and got["n_terms"][0] == 32


def test_nothing_to_compare():
    qf, nq, lf, nl, skip = exact_case(2, 15, 63, 64, 64)
    R = len(qf)
    got = raw_nearest(qf, nq, lf[:0], nl[:0], radius=5.0)
    assert np.isinf(got["distance"]).all() and (got["distance"] > 0).all() and got["index"].tolist() == [-1] * R
    assert got["n_terms"].tolist() == [0] * R and got["n_within"].tolist() == [0] * R and got["matrix"].shape == (R, 0)
    check(got, restated(qf, nq, lf[:0], nl[:0], radius=5.0), "M = 0")
    none = raw_nearest(qf[:0], nq[:0], lf, nl)
    assert none["distance"].shape == (0,) and none["matrix"].shape == (0, len(lf))
    m = int(np.flatnonzero(clamp(nl, 64) == clamp(nq, 64)[0])[0])  # an entry of query 0's length
    one = np.full(R, -1)
    one[0] = 0
    got, want = compare(qf, nq, lf[m:m + 1], nl[m:m + 1], "one entry, skipped for query 0", skip=one, radius=9.0)
    assert got["index"][0] == -1 and np.isinf(got["distance"][0]) and got["n_within"][0] == 0 and np.isfinite(got["matrix"][0, 0])
    got, want = compare(qf, nq, lf[m:m + 1], nl[m:m + 1], "one entry", radius=9.0)
    assert got["index"][0] == 0 and got["n_within"][0] == 1
    lonely = raw_nearest(qf[1:2], nq[1:2], lf, nl)  # a query of a length the library does not hold
    assert lonely["index"].tolist() == [-1] and np.isinf(lonely["matrix"]).all() and lonely["n_terms"].tolist() == [0]


def test_what_stands_behind_the_lengths_changes_nothing_and_lengths_are_clamped():
    qf, nq, lf, nl, skip = exact_case(3, 16, 64, 37, 64)
    base = raw_nearest(qf, nq, lf, nl, skip)
    q2, l2 = qf.copy(), lf.copy()
    for f, n in ((q2, nq), (l2, nl)):
        past = np.arange(f.shape[1])[None, :] >= clamp(n, f.shape[1])[:, None]
        f[past] = 0.5  # numbers that would count
    filled = raw_nearest(q2, nq, l2, nl, skip)
    for k in OUTPUTS:
        assert same_bits(filled[k], base[k]), k
    assert (nq > 37).any() and (nq < 0).any() and (nl > 64).any() and (nl < 0).any()
    clamped = raw_nearest(qf, clamp(nq, 37), lf, clamp(nl, 64), skip)
    for k in OUTPUTS:
        assert same_bits(clamped[k], base[k]), k


# ------------------------------------------------------------------ (b) properties
def test_the_distance_is_symmetric_with_the_roles_swapped():
    qf, nq, lf, nl, _ = exact_case(2, 65, 1000, 64, 64)
    ab, ba = raw_nearest(qf, nq, lf, nl)["matrix"], raw_nearest(lf, nl, qf, nq)["matrix"]
    assert same_bits(ab, np.ascontiguousarray(ba.T)) and same_bits(ab, pair_matrix(qf, nq, lf, nl)[3])
    qf, nq, lf, nl = real_case(17, 64, 2, 2)[:4]
    ab, ba = raw_nearest(qf, nq, lf, nl)["matrix"], raw_nearest(lf, nl, qf, nq)["matrix"]
    assert same_bits(ab, np.ascontiguousarray(ba.T))  # (the chain is the same chain: the products commute)


def test_a_library_cut_in_two_combines_to_the_whole():
    qf, nq, lf, nl, skip = exact_case(3, 65, 4097, 64, 64)
    cut = 2051
    whole = raw_nearest(qf, nq, lf, nl, skip, radius=2.0)
    lo = raw_nearest(qf, nq, lf[:cut], nl[:cut], skip, radius=2.0)
    hi = raw_nearest(qf, nq, lf[cut:], nl[cut:], np.where(skip >= cut, skip - cut, -1), radius=2.0)
    assert same_bits(whole["matrix"], np.concatenate([lo["matrix"], hi["matrix"]], 1))
    assert np.array_equal(whole["n_within"], lo["n_within"] + hi["n_within"]) and whole["n_within"].any()
    first = (lo["index"] >= 0) & ((hi["index"] < 0) | (lo["distance"] <= hi["distance"]))
    assert same_bits(whole["distance"], np.where(first, lo["distance"], hi["distance"]))
    assert np.array_equal(whole["index"], np.where(first, lo["index"], np.where(hi["index"] >= 0, hi["index"] + cut, -1)))
    assert np.array_equal(whole["n_terms"], np.where(first, lo["n_terms"], hi["n_terms"])) and first.any() and not first.all()


def test_a_query_alone_gives_the_bits_it_gives_among_others():
    for case in (exact_case(3, 65, 4097, 64, 64), real_case(65, 1000, 64, 3)):
        qf, nq, lf, nl, skip = case[:5]
        among = raw_nearest(qf, nq, lf, nl, skip)
        for r in (0, 5, 33, 64):
            alone = raw_nearest(qf[r:r + 1], nq[r:r + 1], lf, nl, skip[r:r + 1])
            for k in OUTPUTS:
                assert same_bits(alone[k], among[k][r:r + 1]), (r, k)
        n = int(clamp(nq, qf.shape[1])[7])
        narrow = raw_nearest(qf[7:8, :max(n, 1)], nq[7:8], lf, nl, skip[7:8])  # the same loop in a row as narrow as it is
        for k in OUTPUTS:
            assert same_bits(narrow[k], among[k][7:8]), k


# ------------------------------------------------------------------ (c) real-valued: within the derived bound
@functools.lru_cache(maxsize=None)
def real_case(R, M, L, A, tiny=False):
    """cos / sin of uniform random angles; both sides mostly of length L, some of L - 1, a few terms undefined.  With `tiny`, a quarter of
    the slots hold features of 1e-20 on both sides: their products are subnormal in fp32, and the restatement keeps them.  (Not all
    slots: every distance would then be 2 to within 1e-39, no query would have a gap of two bounds, and the cap of check_real on the
    queries left out - a tenth - could not hold by the reference alone.)"""
    rng = np.random.default_rng(R + M + L + A + tiny)
    lengths = lambda n: np.where(rng.random(n) < 0.8, L, L - 1).astype(np.int32)
    nq, nl = lengths(R), lengths(M)
    qf, lf = (features(rng.uniform(-np.pi, np.pi, (n, L, 3)), range(A)) for n in (R, M))
    if tiny:
        small = rng.random(L) < 0.25
        qf[:, small], lf[:, small] = np.float32(1e-20) * np.sign(qf[:, small]), np.float32(1e-20) * np.sign(lf[:, small])
    for f in (qf, lf):
        f[rng.random(f.shape[:3]) < 0.01] = np.nan
    plant(rng, qf, nq, lf, nl, share=0.01)  # (fewer copies than queries: no query has two, which would be a tie)
    skip = rng.integers(-1, M, R).astype(np.int64)
    return behind(qf, nq), nq, behind(lf, nl), nl, skip


def well_separated(values, near, limit):
    """A radius near the quantile `near` of the finite values that is farther than `limit` from every one of them."""
    v = np.unique(values[np.isfinite(values)])
    at = int(near * (len(v) - 1))
    lo, hi = max(at - 500, 0), min(at + 500, len(v) - 1)
    gaps = np.diff(v[lo:hi + 1])
    k = int(np.argmax(gaps))
    assert gaps[k] / 2 > limit, "the case has no radius that is clear of every distance"
    return float(np.float32((v[lo + k] + v[lo + k + 1]) / 2))


def check_real(case, what):
    """Every finite distance within the bound; index within 2 bounds of the restated minimum, and equal to the restatement's where the
    restated gap between best and second best exceeds 2 bounds, which may leave out at most 10 % of the queries."""
    qf, nq, lf, nl, skip = case
    A = qf.shape[2]
    d, n, magnitude, _ = pair_matrix(qf, nq, lf, nl)
    b = bound(n, magnitude, A, clamp(nq, qf.shape[1]))
    finite = np.isfinite(d)
    limit = float(b[finite].max())
    radius = well_separated(d, 0.05, limit)
    got = raw_nearest(qf, nq, lf, nl, skip, radius=radius)
    want = nearest_ref(d, n, skip=skip, radius=radius)
    assert np.array_equal(np.isfinite(got["matrix"]), finite) and (got["matrix"][~finite] == np.inf).all()
    multiple = float((np.abs(got["matrix"].astype(np.float64)[finite] - d[finite]) / b[finite]).max())
    print(f"{what}: the largest |device - restatement| is {multiple:.3f} of the bound")
    assert multiple <= 1.0, (what, multiple)
    rows = np.arange(len(qf))
    counted = finite & (np.arange(len(lf))[None, :] != skip[:, None])
    some = counted.any(1)
    assert np.array_equal(got["index"] >= 0, some) and some.mean() > 0.9
    ranked = np.sort(np.where(counted, d, np.inf), 1)
    least, gap = ranked[:, 0], (ranked[:, 1] - ranked[:, 0] if len(lf) > 1 else np.full(len(qf), np.inf))
    at = np.maximum(got["index"], 0)
    b_at = b[rows, at]
    assert (counted[rows, at] & (d[rows, at] <= least + 2 * b_at))[some].all()
    assert (np.abs(got["distance"].astype(np.float64) - d[rows, at]) <= b_at)[some].all()
    clear = some & (gap > 2 * np.maximum(b_at, b[rows, np.maximum(want["index"], 0)]))
    assert clear.sum() >= 0.9 * some.sum(), (what, clear.sum(), some.sum())
    assert np.array_equal(got["index"][clear], want["index"][clear])
    assert np.array_equal(got["n_terms"][some], n[rows, at][some]) and not got["n_terms"][~some].any()
    assert np.array_equal(got["n_within"], want["n_within"]) and got["n_within"].any()
    derived = nearest_ref(got["matrix"], n, skip=skip, radius=radius)
    check(got, derived, what + " (from the device matrix)", only=PER_QUERY)
    return multiple


@pytest.mark.parametrize("R, M, L, A, tiny", [(65, 4097, 16, 2, False), (65, 1000, 64, 3, False), (17, 64, 2, 2, False), (65, 1000, 32, 2, True)])
def test_random_angles_stay_within_the_derived_bound(R, M, L, A, tiny):
    case = real_case(R, M, L, A, tiny)
    if tiny:
        assert (np.abs(case[0][np.isfinite(case[0])]) == np.float32(1e-20)).any()
    check_real(case, f"R={R} M={M} L={L} A={A}" + (" tiny" if tiny else ""))


# ------------------------------------------------------------------ (d) the front end
def test_conformation_front_end_against_the_restatement():
    rng = np.random.default_rng(21)
    R, M, L = 40, 300, 12
    loops = lambda n: (rng.uniform(-np.pi, np.pi, (n, L, 3)).astype(np.float32), rng.choice([7, 11, 12], n).astype(np.int32))
    (qa, nq), (la, nl) = loops(R), loops(M)
    qa[rng.random(qa.shape) < 0.05] = np.nan
    la[5], nl[5] = qa[3], nq[3]
    queries, library = metrics.DihedralSet(cuda(qa), cuda(nq)), metrics.DihedralSet(cuda(la), cuda(nl))
    labels = rng.integers(0, 9, M)
    for angles, which in ((("phi", "psi"), (0, 1)), (("omega", "phi"), (0, 2)), (metrics.DIHEDRALS, (0, 1, 2)), (("psi",), (1,))):
        qf, lf = (metrics.dihedral_features(t, which).cpu().numpy() for t in (queries.angles, library.angles))
        assert qf.shape == (R, L, len(which), 2) and np.isnan(qf).any()
        exclude = rng.integers(-1, M + 3, R)
        out = numpy_of(metrics.conformation(queries, library, angles=angles, radius=1.0, exclude=cuda(exclude), matrix=True, labels=cuda(labels), min_terms=3))
        assert out["index"].dtype == np.int64 and out["label"].dtype == np.int64 and out["n_terms"].dtype == np.int32
        want = restated(qf, nq, lf, nl, skip=exclude, radius=1.0, min_terms=3)
        got = dict(out, index=out["index"].astype(np.int32))
        # (the same features, the same fp32 steps; the sum alone may differ by its order, so the distances are held to the bound)
        d, n, magnitude, _ = pair_matrix(qf, nq, lf, nl, 3)
        b = bound(n, magnitude, len(which), nq)
        fin = np.isfinite(d)
        assert np.array_equal(np.isfinite(got["matrix"]), fin) and (np.abs(got["matrix"][fin] - d[fin]) <= b[fin]).all()
        check(got, nearest_ref(got["matrix"], n, skip=exclude, radius=1.0), str(angles), only=PER_QUERY)
        assert np.array_equal(out["length"], nq) and np.array_equal(out["nearest_length"], np.where(got["index"] >= 0, nl[np.maximum(got["index"], 0)], -1))
        assert np.array_equal(out["label"], np.where(got["index"] >= 0, labels[np.maximum(got["index"], 0)], -1))
        if exclude[3] != 5:
            assert got["index"][3] == 5 and got["distance"][3] <= b[3, 5]
    plain = metrics.conformation(queries, library)
    assert set(plain) == {"distance", "index", "n_terms", "length", "nearest_length"}
    # the set against itself
    own = numpy_of(metrics.conformation(queries, queries, exclude="self", radius=1e-6, matrix=True))
    assert (own["index"] != np.arange(R)).all() and (own["matrix"].diagonal()[nq > 0] <= 1e-6).all() and not own["n_within"].any()
    on_cpu = metrics.conformation(metrics.DihedralSet(torch.from_numpy(qa), torch.from_numpy(nq)), library, matrix=True)
    assert not on_cpu["matrix"].is_cuda and same_bits(on_cpu["matrix"].numpy(), numpy_of(metrics.conformation(queries, library, matrix=True))["matrix"])
    empty = metrics.conformation(queries, metrics.dihedral_set([]), radius=1.0, labels=torch.zeros(0, dtype=torch.long))
    assert torch.isinf(empty["distance"]).all() and (empty["index"] == -1).all() and (empty["label"] == -1).all() and (empty["nearest_length"] == -1).all()


# ------------------------------------------------------------------ (e) design rows as loops
def pack_case(K, N=3, G=2, seed=0):
    rng = np.random.default_rng(K + seed)
    phi, psi, omega = (rng.uniform(-np.pi, np.pi, (G * N, K)).astype(np.float32) for _ in range(3))
    for v in (phi, psi, omega):
        v[rng.random(v.shape) < 0.15] = np.nan
    mask = rng.random((G, K)) < 0.3
    mask[:, [0, K - 1]] = True
    if K > 64:
        mask[:, 62:67] = True  # counted slots on both sides of slot 64
    rm = rng.random((G, K)) < 0.8
    seg = rng.integers(0, 3, (G, K))
    return phi, psi, omega, mask, rm, seg


def raw_pack(phi, psi, omega, mask, rm, seg, segment, group_size, L, shifted=False, skip=()):
    place = lambda t: misaligned(t, 4 if t.element_size() >= 4 else 3) if shifted else t
    rows, K = phi.shape
    ops = [cuda(phi), cuda(psi), cuda(omega), cuda(mask), None if rm is None else cuda(rm), None if seg is None else cuda(seg.astype(np.int32))]
    ops = [None if t is None else place(t) for t in ops]
    out = {"out_angles": place(torch.empty(rows, L, 3, dtype=torch.float32, device="cuda")), "out_len": place(torch.empty(rows, dtype=torch.int32, device="cuda"))}
    out = {k: v for k, v in out.items() if k not in skip}
    lib = _hip.lib()
    rc = lib.diffab_metrics_pack_dihedrals(*[_hip.ptr(t) for t in ops], segment, rows, group_size, K, L, _hip.ptr(out.get("out_angles")),
                                           _hip.ptr(out.get("out_len")), _hip.stream_ptr())
    assert rc == 0, _hip.load_library().diffab_last_error().decode()
    torch.cuda.synchronize()
    return numpy_of(out)


@pytest.mark.parametrize("K", [1, 64, 65, 130])
def test_pack_dihedrals_equals_a_gather(K):
    phi, psi, omega, mask, rm, seg = pack_case(K)
    for rm_, seg_, segment, L in ((None, None, 0, 64), (rm, None, 0, 64), (rm, seg, 2, 33), (None, seg, 1, 7), (None, None, 0, 1)):
        want_a, want_n = pack_ref(phi, psi, omega, mask, rm_, seg_, segment, 3, L)
        got = raw_pack(phi, psi, omega, mask, rm_, seg_, segment, 3, L)
        assert same_bits(got["out_angles"], want_a) and same_bits(got["out_len"], want_n), (K, L, segment)
    if K == 130:
        assert (pack_ref(phi, psi, omega, mask, None, seg, 1, 3, 7)[1] > 7).any()  # a count above L: reported, the slots cut
        inside = pack_ref(phi, psi, omega, mask, None, None, 0, 3, 64)
        assert np.isnan(inside[0][0, :min(inside[1][0], 64)]).any()  # NaN angles are carried through
    only_len = raw_pack(phi, psi, omega, mask, rm, seg, 2, 3, 64, skip=("out_angles",))
    assert set(only_len) == {"out_len"} and same_bits(only_len["out_len"], pack_ref(phi, psi, omega, mask, rm, seg, 2, 3, 64)[1])
    only_angles = raw_pack(phi, psi, omega, mask, rm, seg, 2, 3, 64, skip=("out_len",))
    assert same_bits(only_angles["out_angles"], pack_ref(phi, psi, omega, mask, rm, seg, 2, 3, 64)[0])


# ------------------------------------------------------------------ (f) contracts
@functools.lru_cache(maxsize=None)
def contract_case(A=2, R=33, M=2100, LQ=23, LM=37):
    qf, nq, lf, nl, skip = exact_case(A, R, M, LQ, LM, seed=7)
    return qf, nq, lf, nl, skip, restated(qf, nq, lf, nl, skip)


@pytest.mark.parametrize("leave", [("matrix",), ("distance",), ("index", "n_terms"), ("n_within", "matrix"), OUTPUTS[:4], OUTPUTS])
def test_null_outputs_are_skipped_and_the_others_unchanged(leave):
    qf, nq, lf, nl, skip, want = contract_case()
    got = raw_nearest(qf, nq, lf, nl, skip, leave=leave)
    assert set(got) == set(OUTPUTS) - set(leave)
    check(got, want, f"without {leave}")


@pytest.mark.parametrize("fill", ["ff", "random"])
def test_what_the_workspace_and_the_outputs_held_is_ignored(fill):
    qf, nq, lf, nl, skip, want = contract_case()
    with poisoned(fill, seed=5):
        check(raw_nearest(qf, nq, lf, nl, skip), want, f"under {fill}")
        check(raw_nearest(qf, nq, lf, nl, skip, leave=("matrix",)), want, f"four outputs under {fill}")
        check(raw_nearest(qf, nq, lf, nl, skip, leave=OUTPUTS[:4]), want, f"the matrix under {fill}")
        small = contract_case(3, 5, 3, 64, 64)
        check(raw_nearest(*small[:5]), small[5], f"three entries under {fill}")
        phi, psi, omega, mask, rm, seg = pack_case(130)
        got = raw_pack(phi, psi, omega, mask, rm, None, 0, 3, 50)
        want_a, want_n = pack_ref(phi, psi, omega, mask, rm, None, 0, 3, 50)
        assert same_bits(got["out_angles"], want_a) and same_bits(got["out_len"], want_n)


CONFORMATION_ARGTYPES = {n: a for n, (_, a) in _hip.CONFORMATION_SYMBOLS.items()}
CONFORMATION_WRITES = {"diffab_metrics_dihedral_nearest": " ".join(OUTPUTS) + " workspace", "diffab_metrics_pack_dihedrals": "out_angles out_len"}


@pytest.mark.parametrize("fill", sampler_support.GUARD_FILLS)
def test_outputs_between_guards_with_operands_at_their_natural_alignment(fill, monkeypatch):
    for entry, writes in CONFORMATION_WRITES.items():
        monkeypatch.setitem(sampler_support.WRITES, entry, writes)
    params = {n: [p[0] for p in ps] for n, ps in header_prototypes(("diffab_hip_conformation.h",))[1].items()}
    assert set(params) == set(CONFORMATION_ARGTYPES)
    with GuardedABI(tuple(CONFORMATION_ARGTYPES), fill, argtypes=CONFORMATION_ARGTYPES) as abi:
        abi.params.update(params)
        for shape in ((2, 33, 2100, 23, 37), (3, 5, 3, 64, 64), (1, 17, 65, 1, 1)):
            qf, nq, lf, nl, skip, want = contract_case(*shape)
            check(raw_nearest(qf, nq, lf, nl, skip, shifted=True), want, f"{shape} guarded [{fill}]")
        qf, nq, lf, nl, skip, want = contract_case()
        check(raw_nearest(qf, nq, lf, nl, None, leave=OUTPUTS[:4], shifted=True), restated(qf, nq, lf, nl), "guarded, the matrix alone")
        for K in (1, 65, 130):
            phi, psi, omega, mask, rm, seg = pack_case(K)
            got = raw_pack(phi, psi, omega, mask, rm, seg, 1, 3, 9, shifted=True)
            want_a, want_n = pack_ref(phi, psi, omega, mask, rm, seg, 1, 3, 9)
            assert same_bits(got["out_angles"], want_a) and same_bits(got["out_len"], want_n), K
    assert abi.counts["diffab_metrics_dihedral_nearest"] >= 4 and abi.counts["diffab_metrics_pack_dihedrals"] >= 3


# ------------------------------------------------------------------ (g) end to end
def test_sampled_designs_against_a_library_that_holds_them():
    """sample(num_samples = 4) of the unit model at K = 64 -> design_dihedrals -> conformation against a library that holds every design's
    own loop once among decoys of the same and of other lengths: each design finds its own entry at a distance of rounding size (the sum
    of cos^2 + sin^2 of fp32 features is n only up to the bound), the labels come through, and the self-matrix goes into cluster."""
    dims, model, _ = sampler_support.unit_model()
    G, K, N = 2, 64, 4
    inp = sampler_support.patches(G, K, dims, seed=5)
    res = sampler_support.sample(model, inp, seed=3, num_samples=N, steps=2)
    gm = inp["generation_mask"]
    designs = metrics.design_dihedrals(res, gm, group_size=N)
    rows = G * N
    bb = metrics.backbone(res, gm, group_size=N)
    want_a, want_n = pack_ref(*[bb[k].cpu().numpy() for k in metrics.DIHEDRALS], gm.cpu().numpy(), group_size=N, L=64)
    qa, nq = designs.angles.cpu().numpy(), designs.lengths.cpu().numpy()
    assert same_bits(qa, want_a) and same_bits(nq, want_n) and (nq > 0).all() and qa.shape == (rows, 64, 3)
    assert np.isfinite(qa[np.arange(64)[None, :] < nq[:, None]]).any()
    rng = np.random.default_rng(2)
    M = 300
    nl = np.concatenate([rng.choice(np.unique(nq), M // 2), rng.integers(1, 30, M - M // 2)]).astype(np.int32)
    la = rng.uniform(-np.pi, np.pi, (M, 64, 3)).astype(np.float32)
    own = rng.choice(M, rows, replace=False)  # where each design's own loop goes
    la[own], nl[own] = qa, nq
    la[np.arange(64)[None, :] >= nl[:, None]] = np.nan
    library = metrics.DihedralSet(cuda(la), cuda(nl))
    labels = np.arange(M) * 3 + 1
    out = numpy_of(metrics.conformation(designs, library, angles=metrics.DIHEDRALS, radius=1e-5, labels=cuda(labels)))
    qf, lf = (metrics.dihedral_features(t.cuda(), (0, 1, 2)).cpu().numpy() for t in (designs.angles, library.angles))
    d, n, magnitude, _ = pair_matrix(qf, nq, lf, nl)
    b = bound(n, magnitude, 3, nq)
    at = np.arange(rows)
    assert np.isfinite(d[at, own]).all() and (out["n_terms"] == n[at, own]).all() and (out["n_terms"] > 0).all()
    assert (out["distance"] <= b[at, own]).all() and (out["distance"] >= 0).all()
    assert (d[at, out["index"]] <= d.min(1) + 2 * b[at, out["index"]]).all()
    second = np.sort(d, 1)[:, 1]
    clear = second - d.min(1) > 2 * b.max(1)
    assert clear.any() and np.array_equal(out["index"][clear], own[clear]) and np.array_equal(out["label"], labels[out["index"]])
    assert (out["n_within"] >= 1).all() and np.array_equal(out["nearest_length"], nq)
    assert (metrics.dihedral_angle(torch.from_numpy(out["distance"])) < 0.1).all()
    # the designs of patch 0 against themselves, as a distance matrix for cluster
    mine = metrics.DihedralSet(designs.angles[:N], designs.lengths[:N])
    dist = metrics.conformation(mine, mine, angles=metrics.DIHEDRALS, matrix=True)["matrix"]
    clusters = metrics.cluster(dist.view(1, N, N), 0.5)
    assert tuple(clusters["label"].shape) == (1, N) and (dist.diagonal() <= 1e-5).all() and torch.equal(dist, dist.T)
