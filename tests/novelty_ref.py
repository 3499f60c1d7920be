"""The numpy restatement of diffab_metrics_edit_nearest and diffab_metrics_pack_sequences (DESIGN.md section 4.26,
include/diffab_hip_novelty.h), shared by tests/test_novelty_host.py (hand-made cases) and tests/test_gpu_novelty.py (the kernels).

The distance is the plain dynamic programme, D[i][j] = min(D[i-1][j] + 1, D[i][j-1] + 1, D[i-1][j-1] + (0 if the tokens match else 1)),
one row of the table at a time and every (query, entry) pair at once: the horizontal term is a running minimum, D[i][j] - j =
min over k <= j of (t[k] - k) with t the minimum of the other two terms, so a row is a handful of array operations.  Nothing of the
bit-vector form the kernels use is restated here.  Not a test module; keep R * M of a case at or below about 20 000."""
import numpy as np

MAX_MATCH = 32  # two tokens match iff they are equal and both below this
PAD = 255
PER_QUERY = ("distance", "index", "n_within", "identity")


def clamp(lengths, width):
    return np.clip(np.asarray(lengths, np.int64), 0, width)


def edit_matrix(q_tokens, q_len, lib_tokens, lib_len):
    """(R, M) int32: d(r, m) of the first clamped-length tokens of the rows."""
    q_tokens, lib_tokens = np.asarray(q_tokens, np.int64), np.asarray(lib_tokens, np.int64)
    (R, LQ), (M, LM) = q_tokens.shape, lib_tokens.shape
    nq, nl = clamp(q_len, LQ), clamp(lib_len, LM)
    out = np.zeros((R, M), np.int16)  # (int16 throughout: no value exceeds LQ + LM, and the arrays are what takes the time)
    if R == 0 or M == 0:
        return out.astype(np.int32)
    j = np.arange(LM + 1, dtype=np.int16)
    row = np.broadcast_to(j, (R, M, LM + 1)).copy()  # D[0][j] = j
    at = np.broadcast_to(nl[None, :, None], (R, M, 1))
    take = lambda: np.take_along_axis(row, at, 2)[:, :, 0]
    out[nq == 0] = take()[nq == 0]
    text_ok = lib_tokens < MAX_MATCH
    for i in range(1, int(nq.max()) + 1):
        a = q_tokens[:, i - 1]
        match = (a[:, None, None] == lib_tokens[None]) & (a < MAX_MATCH)[:, None, None] & text_ok[None]  # (R, M, LM)
        t = np.empty_like(row)
        t[:, :, 0] = i
        t[:, :, 1:] = np.minimum(row[:, :, 1:] + 1, row[:, :, :-1] + np.where(match, 0, 1).astype(np.int16))
        row = np.minimum.accumulate(t - j, axis=2) + j
        out[nq == i] = take()[nq == i]
    return out.astype(np.int32)


def nearest_ref(q_tokens, q_len, lib_tokens, lib_len, skip=None, radius=-1, matrix=None):
    """What the entry writes, from the full matrix: distance, index, n_within int32 (R), identity float32 (R), matrix int32 (R, M)."""
    q_tokens, lib_tokens = np.asarray(q_tokens), np.asarray(lib_tokens)
    (R, LQ), (M, LM) = q_tokens.shape, lib_tokens.shape
    d = edit_matrix(q_tokens, q_len, lib_tokens, lib_len) if matrix is None else np.asarray(matrix, np.int32)
    nq, nl = clamp(q_len, LQ), clamp(lib_len, LM)
    counted = np.ones((R, M), bool)
    if skip is not None:
        counted &= np.arange(M)[None, :] != np.asarray(skip, np.int64)[:, None]
    distance, index = np.full(R, -1, np.int32), np.full(R, -1, np.int32)
    identity = np.full(R, np.nan, np.float32)
    for r in range(R):
        ms = np.flatnonzero(counted[r])
        if len(ms):
            best = ms[np.argmin(d[r, ms])]  # (argmin: the first of equals, so the lowest m)
            distance[r], index[r] = d[r, best], best
            longer = max(int(nq[r]), int(nl[best]))
            identity[r] = np.float32(1.0) if longer == 0 else np.float32(1.0) - np.float32(d[r, best]) / np.float32(longer)
    n_within = (counted & (d <= radius)).sum(1).astype(np.int32) if radius >= 0 else np.zeros(R, np.int32)
    return {"distance": distance, "index": index, "n_within": n_within, "identity": identity, "matrix": d}


def pack_ref(tokens, mask, residue_mask=None, segment_idx=None, segment=0, group_size=1, L=64):
    """out_tokens (rows, L) uint8 and out_len (rows) int32 of diffab_metrics_pack_sequences, by a gather."""
    tokens = np.asarray(tokens, np.int64)
    rows, K = tokens.shape
    counted = np.asarray(mask) != 0
    if residue_mask is not None:
        counted = counted & (np.asarray(residue_mask) != 0)
    if segment_idx is not None:
        counted = counted & (np.asarray(segment_idx) == segment)
    out, length = np.full((rows, L), PAD, np.uint8), np.zeros(rows, np.int32)
    for r in range(rows):
        t = tokens[r, counted[r // group_size]]
        t = np.where((t >= 0) & (t < PAD), t, PAD)
        length[r] = len(t)
        out[r, :min(len(t), L)] = t[:L]
    return out, length


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()
