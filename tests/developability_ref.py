"""The numpy restatements of the two developability entries (include/diffab_hip_develop.h), shared by
test_developability_host.py and test_gpu_developability.py.  Not a test module: importing it loads no library and touches no device.

patches_ref takes the squared distances and every comparison in numpy float32, grouped as the header fixes them
(test_geometry_host.d2_f32), so its integers and states are what the kernel must EQUAL; the pair terms and every sum are float64 (the
product of two float32 values is exact there), rounded to float32 once at the end.  motifs_ref walks the chain slot by slot in Python."""
import numpy as np

from test_geometry_host import d2_f32

f32 = np.float32
PRESENT, SCOPE, EXPOSED = 1, 2, 4


def patches_ref(sites, context_sites, tokens, gen, rm=None, antigen=None, exposed_in=None, *, hydrophobicity, charge, group_size=1,
                neighbour_distance=10.0, max_neighbours=16, vicinity_distance=10.0, patch_distance=7.5, min_distance=3.8):
    """sites (rows,K,3) fp32, context_sites (G,K,3) fp32, tokens (rows,K) int, gen / rm / antigen (G,K) bool, exposed_in (rows,K) bool
    -> dict of the thirteen outputs of diffab_metrics_patches, the float ones as float32 plus their float64 values under '<name>_f64'."""
    sites, context_sites = np.asarray(sites, f32), np.asarray(context_sites, f32)
    rows, K = tokens.shape
    hyd, chg = np.asarray(hydrophobicity, f32), np.asarray(charge, f32)
    V = len(hyd)
    assert len(chg) == V
    sq = lambda c: f32(c) * f32(c)
    nb2, vic2, patch2, min2 = sq(neighbour_distance), sq(vicinity_distance), sq(patch_distance), sq(min_distance)
    out = {k: np.zeros(rows, np.float64) for k in ("psh", "ppc", "pnc", "charge_generated", "charge_scope")}
    out.update({k: np.zeros(rows, np.int32) for k in ("n_scope", "n_exposed", "n_pairs")})
    out.update({k: np.zeros((rows, K), np.float64) for k in ("residue_psh", "residue_ppc", "residue_pnc")})
    out.update(n_neighbours=np.zeros((rows, K), np.int32), state=np.zeros((rows, K), np.uint8))
    for r in range(rows):
        g = r // group_size
        present = np.ones(K, bool) if rm is None else np.asarray(rm[g], bool).copy()
        if antigen is not None:
            present &= ~np.asarray(antigen[g], bool)
        generated = np.asarray(gen[g], bool) & present
        xyz = np.where(generated[:, None], sites[r], context_sites[g])
        known = (tokens[r] >= 0) & (tokens[r] < V)
        h = np.where(known, hyd[np.where(known, tokens[r], 0)], f32(0)).astype(f32)
        q = np.where(known, chg[np.where(known, tokens[r], 0)], f32(0)).astype(f32)
        with np.errstate(invalid="ignore", over="ignore"):
            d2 = d2_f32(xyz, xyz)
            both = present[:, None] & present[None, :] & ~np.eye(K, dtype=bool)
            count = (both & (d2 < nb2)).sum(1).astype(np.int32)
            near = (present[:, None] & generated[None, :] & (d2 < vic2)).any(1)
            scope = present & (generated | near)
            exposed = scope & (count <= max_neighbours if exposed_in is None else np.asarray(exposed_in[r]) != 0)
            pair = exposed[:, None] & exposed[None, :] & ~np.eye(K, dtype=bool) & (d2 < patch2)
            floor = np.maximum(d2, min2).astype(np.float64)  # (the max is taken in float32)
        h64, q64 = h.astype(np.float64), q.astype(np.float64)
        for name, w, ok in (("psh", h64, np.ones(K, bool)), ("ppc", q64, q > 0), ("pnc", q64, q < 0)):
            use = pair & ok[:, None] & ok[None, :]
            with np.errstate(invalid="ignore", divide="ignore"):
                term = np.where(use, w[:, None] * w[None, :] / floor, 0.0)
            per_residue = np.array([sum(term[i, use[i]].tolist()) for i in range(K)])  # ascending j
            out["residue_" + name][r] = per_residue
            out[name][r] = 0.5 * per_residue.sum()
        out["charge_generated"][r] = q64[generated].sum()
        out["charge_scope"][r] = q64[scope].sum()
        out["n_scope"][r], out["n_exposed"][r], out["n_pairs"][r] = scope.sum(), exposed.sum(), pair.sum() // 2
        out["n_neighbours"][r] = count
        out["state"][r] = present * PRESENT + scope * SCOPE + exposed * EXPOSED
    for k in [k for k, v in out.items() if v.dtype == np.float64]:
        out[k + "_f64"] = out[k]
        out[k] = out[k].astype(f32)
    return out


def succ_ref(rm, chain, ridx):
    """(K,) each -> (K,) int: the lowest slot j inside rm with chain[j] == chain[i] and ridx[j] == ridx[i] + 1, -1 without one or for a
    slot outside rm."""
    K = len(chain)
    out = np.full(K, -1, np.int64)
    for i in range(K):
        if rm[i]:
            hit = [j for j in range(K) if rm[j] and chain[j] == chain[i] and int(ridx[j]) == int(ridx[i]) + 1]
            out[i] = hit[0] if hit else -1
    return out


def motifs_ref(tokens, gen, rm, chain, ridx, motifs, group_size=1, counted_only=True):
    """tokens (rows,K) int, gen / rm (G,K) bool (rm may be None), chain / ridx (G,K) int, motifs (M,4) int32 ->
    dict: motif_count (rows,M) int32, n_motifs (rows) int32, motif_start (rows,K) int32.
    counted_only=False counts the matches without a generated residue as well (for a test's own preconditions)."""
    motifs = np.ascontiguousarray(np.asarray(motifs, np.int32).reshape(-1, 4)).view(np.uint32).astype(np.int64)
    rows, K = tokens.shape
    M = len(motifs)
    count = np.zeros((rows, M), np.int32)
    start = np.zeros((rows, K), np.uint32)
    for r in range(rows):
        g = r // group_size
        inside = np.ones(K, bool) if rm is None else np.asarray(rm[g], bool)
        succ = succ_ref(inside, chain[g], ridx[g])
        for m in range(M):
            length = next((p for p in range(4) if motifs[m, p] == 0), 4)
            for i in range(K):
                s, ok, generated = i, True, False
                for p in range(length):
                    if s < 0 or not inside[s] or not 0 <= tokens[r, s] < 32 or not (int(motifs[m, p]) >> int(tokens[r, s])) & 1:
                        ok = False
                        break
                    generated |= bool(gen[g][s])
                    s = succ[s]
                if ok and (generated or not counted_only):
                    count[r, m] += 1
                    start[r, i] |= np.uint32(1 << m)
    return {"motif_count": count, "n_motifs": count.sum(1).astype(np.int32), "motif_start": start.view(np.int32)}


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def ulps_apart(a, b):
    """Elementwise distance of two float32 arrays in units in the last place (both finite and of one sign, or equal)."""
    a, b = np.ascontiguousarray(a, f32), np.ascontiguousarray(b, f32)
    ia, ib = a.view(np.int32).astype(np.int64), b.view(np.int32).astype(np.int64)
    ia, ib = np.where(ia < 0, -(ia & 0x7FFFFFFF), ia), np.where(ib < 0, -(ib & 0x7FFFFFFF), ib)
    return np.abs(ia - ib)
