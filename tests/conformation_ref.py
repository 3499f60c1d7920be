"""The numpy restatement of diffab_metrics_dihedral_nearest and diffab_metrics_pack_dihedrals (DESIGN.md section 4.27,
include/diffab_hip_conformation.h), shared by tests/test_conformation_host.py (hand-made cases) and tests/test_gpu_conformation.py (the
kernels).

pair_matrix is the rule in float64: the mask of the terms defined in both loops, their sum, 2 - 2 sum / n, and sum |q l| for the error
bound.  Beside it stands the same value taken through the rule's three fp32 roundings (the sum, the quotient, 2 - 2 t): where the
float64 sum is exact in fp32 - features on a dyadic grid - that is what the entry must give bit for bit, in whatever order it adds.
Nothing of the sort by lengths, of the masks as words or of the matrix cores is restated here.  Not a test module."""
import numpy as np

U = 2.0 ** -24  # the unit roundoff of fp32
PER_QUERY = ("distance", "index", "n_terms", "n_within")


def clamp(lengths, width):
    return np.clip(np.asarray(lengths, np.int64), 0, width)


def features(angles, which=(0, 1, 2)):
    """(M, L, A, 2) float32: (cos, sin) of the chosen kinds of angles (M, L, 3), taken in float64 and rounded once."""
    a = np.asarray(angles, np.float64)[..., list(which)]
    with np.errstate(invalid="ignore"):
        return np.stack([np.cos(a), np.sin(a)], -1).astype(np.float32)


def defined(feat, lengths):
    """(n, L, A) bool: the term is below the clamped length and both of its numbers are finite."""
    feat = np.asarray(feat)
    n, L = feat.shape[:2]
    inside = np.arange(L)[None, :] < clamp(lengths, L)[:, None]
    return np.isfinite(feat).all(-1) & inside[:, :, None]


def pair_matrix(q_feat, q_len, lib_feat, lib_len, min_terms=1):
    """d (R, M) float64 (+inf for a pair that is not comparable), n (R, M) int32, sum |q l| (R, M) float64, and d32 (R, M) float32: the
    rule's fp32 steps applied to the float64 sum."""
    q_feat, lib_feat = np.asarray(q_feat, np.float32), np.asarray(lib_feat, np.float32)
    (R, LQ, A, _), (M, LM) = q_feat.shape, lib_feat.shape[:2]
    nq, nl = clamp(q_len, LQ), clamp(lib_len, LM)
    L = max(LQ, LM)

    def side(feat, lengths, n_rows, width):
        ok = defined(feat, lengths)
        v = np.zeros((n_rows, L, A, 2), np.float64)  # (float64 keeps the subnormal products of tiny features)
        v[:, :width] = np.where(ok[..., None], feat.astype(np.float64), 0.0)
        return v.reshape(n_rows, L * A * 2), np.pad(ok, ((0, 0), (0, L - width), (0, 0))).reshape(n_rows, L * A).astype(np.float64)

    (q, q_ok), (l, l_ok) = side(q_feat, nq, R, LQ), side(lib_feat, nl, M, LM)
    total = q @ l.T
    magnitude = np.abs(q) @ np.abs(l).T
    n = np.rint(q_ok @ l_ok.T).astype(np.int32)
    comparable = (nq[:, None] == nl[None, :]) & (n >= min_terms)
    safe = np.maximum(n, 1)
    d = np.where(comparable, 2.0 - 2.0 * total / safe, np.inf)
    with np.errstate(over="ignore", invalid="ignore"):
        t = total.astype(np.float32) / safe.astype(np.float32)
        d32 = np.where(t >= 1, np.float32(0), np.float32(2) - np.float32(2) * t).astype(np.float32)
    d32 = np.where(comparable, d32, np.float32(np.inf)).astype(np.float32)
    return d, n, magnitude, d32


def bound(n, magnitude, A, lengths):
    """The derived error bound of a comparable pair's distance, (R, M): 2 (n_k + 2) u sum|q l| / n + 8 u with n_k = 2 A len (the gamma
    bound of an n_k-term chain, one rounding each for the division and the subtraction)."""
    n_k = 2 * A * np.asarray(lengths, np.float64)[:, None]
    return 2 * (n_k + 2) * U * magnitude / np.maximum(n, 1) + 8 * U


def nearest_ref(d, n, skip=None, radius=-1.0):
    """What the entry writes per query, from a matrix d (R, M) of either precision and the term counts n: distance (the matrix's dtype),
    index, n_terms, n_within int32."""
    d, n = np.asarray(d), np.asarray(n)
    R, M = d.shape
    counted = np.isfinite(d) | np.isnan(d)  # a comparable pair (+inf stands for "not comparable")
    if skip is not None:
        counted &= np.arange(M)[None, :] != np.asarray(skip, np.int64)[:, None]
    distance, index, n_terms = np.full(R, np.inf, d.dtype), np.full(R, -1, np.int32), np.zeros(R, np.int32)
    for r in range(R):
        ms = np.flatnonzero(counted[r])
        if len(ms):
            best = ms[np.argmin(d[r, ms])]  # (argmin: the first of equals, so the lowest m)
            distance[r], index[r], n_terms[r] = d[r, best], best, n[r, best]
    with np.errstate(invalid="ignore"):
        n_within = (counted & (d <= d.dtype.type(radius))).sum(1).astype(np.int32)
    return {"distance": distance, "index": index, "n_terms": n_terms, "n_within": n_within, "matrix": d}


def pack_ref(phi, psi, omega, mask, residue_mask=None, segment_idx=None, segment=0, group_size=1, L=64):
    """out_angles (rows, L, 3) float32 and out_len (rows) int32 of diffab_metrics_pack_dihedrals, by a gather."""
    angles = np.stack([np.asarray(v, np.float32) for v in (phi, psi, omega)], -1)
    rows = angles.shape[0]
    counted = np.asarray(mask) != 0
    if residue_mask is not None:
        counted = counted & (np.asarray(residue_mask) != 0)
    if segment_idx is not None:
        counted = counted & (np.asarray(segment_idx) == segment)
    out, length = np.full((rows, L, 3), np.nan, np.float32), np.zeros(rows, np.int32)
    for r in range(rows):
        t = angles[r, counted[r // group_size]]
        length[r] = len(t)
        out[r, :min(len(t), L)] = t[:L]
    return out, length


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()
