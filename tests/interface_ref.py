"""The numpy restatements of the two interface entries (include/diffab_hip_interface.h), shared by
test_interface_host.py and test_gpu_interface.py.  Not a test module: importing it loads no library and touches no device.

contact_map_ref takes the squared distances and the comparison in numpy float32, grouped as the header of diffab_metrics_contacts fixes
them (test_geometry_host.d2_f32), so its bits are the bits the kernel must EQUAL.  pairwise_bits_ref counts by unpacking every word into
32 booleans and multiplying the boolean matrices in int64, and divides in numpy float32: one correctly rounded division per quotient."""
import numpy as np

from test_geometry_host import atoms_of, d2_f32

f32 = np.float32


def contact_map_ref(points, valid, ctx_points, ctx_valid, gen, rm, chain, ridx, antigen, group_size=1, contact_distance=5.0,
                    ignore_bonds=False):
    """points (rows,K,P,3) fp32 with validity bits valid (rows,K); ctx_points (G,K,A,3) fp32 with bits ctx_valid (G,K); gen, rm, chain,
    ridx, antigen (G,K).  -> (rows,K,K) bool: [r,i,j] is true iff generated residue i of row r and antigen residue j are in contact.
    ignore_bonds: chain neighbours count like any other pair (for a test's own preconditions, never for a comparison)."""
    rows, K = points.shape[:2]
    contact = f32(contact_distance)
    contact2 = contact * contact
    out = np.zeros((rows, K, K), bool)
    for r in range(rows):
        g = r // group_size
        rows_of = np.flatnonzero(gen[g] & rm[g])
        cols_of = np.flatnonzero(~gen[g] & rm[g] & np.asarray(antigen[g], bool))
        gxyz, gown = atoms_of(np.asarray(points[r], f32), valid[r], rows_of)
        cxyz, cown = atoms_of(np.asarray(ctx_points[g], f32), ctx_valid[g], cols_of)
        if gxyz.shape[0] == 0 or cxyz.shape[0] == 0:
            continue
        bonded = (chain[g][:, None] == chain[g][None, :]) & (np.abs(ridx[g][:, None].astype(np.int64) - ridx[g][None, :]) == 1)
        ok = np.ones((len(gown), len(cown)), bool) if ignore_bonds else ~bonded[gown[:, None], cown[None, :]]
        ia, ib = np.nonzero(ok & (d2_f32(gxyz, cxyz) < contact2))  # strict
        out[r, gown[ia], cown[ib]] = True
    return out


def pack_ref(contact):
    """(rows,K,K) bool -> (rows,K,W) int32, W = ceil(K / 32): bit j & 31 of word j >> 5 of row i = contact[r,i,j]."""
    rows, K = contact.shape[:2]
    W = (K + 31) // 32
    padded = np.zeros((rows, K, W * 32), np.uint64)
    padded[:, :, :K] = contact
    words = (padded.reshape(rows, K, W, 32) << np.arange(32, dtype=np.uint64)).sum(-1)
    return words.astype(np.uint32).view(np.int32)


def unpack_ref(words):
    """(..., L) int32 -> (..., 32 L) bool, bit b of word w at [32 w + b]."""
    u = np.ascontiguousarray(words).view(np.uint32)
    return ((u[..., None] >> np.arange(32, dtype=np.uint32)) & 1).astype(bool).reshape(*u.shape[:-1], u.shape[-1] * 32)


def pairwise_bits_ref(bits, group_size):
    """bits (G*N, ...) int32, L words per design -> dict: n_set (G,N) int32, n_common (G,N,N) int32, fcc, jaccard (G,N,N) float32."""
    bits = np.asarray(bits)
    assert bits.dtype == np.int32
    N = group_size
    G = bits.shape[0] // N
    member = unpack_ref(bits.reshape(G, N, -1)).astype(np.int64)  # (G, N, 32 L)
    n_set = member.sum(-1)
    n_common = member @ member.transpose(0, 2, 1)
    union = n_set[:, :, None] + n_set[:, None, :] - n_common
    with np.errstate(divide="ignore", invalid="ignore"):
        fcc = np.where(n_set[:, :, None] == 0, f32(1), n_common.astype(f32) / np.broadcast_to(n_set[:, :, None], n_common.shape).astype(f32))
        jaccard = np.where(union == 0, f32(1), n_common.astype(f32) / union.astype(f32))
    return {"n_set": n_set.astype(np.int32), "n_common": n_common.astype(np.int32), "fcc": fcc.astype(f32), "jaccard": jaccard.astype(f32)}


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()
