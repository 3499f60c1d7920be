"""CPU: the host side of the design similarities (diffab_pytorch.metrics.similarity) - the float64 numpy oracle of the rule (lddt_ref,
contacts_ref), the fp32 restatement that performs the kernel's operations in the kernel's order (lddt_f32, contacts_f32), their
hand-computed cases, the C-ABI entry and its host-side refusals, and the argument checks that happen before any library call.

The rule is DESIGN.md section 4.17 / the comment of diffab_metrics_similarity in include/diffab_hip.h.  test_gpu_similarity.py imports
the oracle, the restatement and the inputs from here.

Where fp32 and float64 may differ.  Every output is an integer count of comparisons of distances with a threshold, or one fp32 division of
two such counts.  The fp32 distance of two points up to 60 A apart is within 1e-5 A of the exact one (three subtractions, three products,
two sums and a root, each within 2^-24 relative of a value below 3600), so a comparison can come out differently only where the float64
quantity lies within 1e-4 A of its threshold: |d_des - d_nat| of a threshold, d_nat of the inclusion radius, a point distance of the
contact distance.  The oracle counts those BOUNDARY pairs; the two restatements must agree on every other pair."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from diffab_pytorch import _hip, metrics, synthetic as syn
from diffab_pytorch.io import backbone_from_frames
from sampler_support import ReachedTheLibrary, refuse_library

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TAU = (0.5, 1.0, 2.0, 4.0)
EDGE = 1e-4  # Angstrom: the half-width of a boundary
LDDT_KEYS = ("n_pairs", "preserved", "lddt_residue", "lddt", "lddt_thresholds")
INTERFACE_KEYS = ("n_pairs_interface", "preserved_interface", "ilddt_residue", "ilddt")
CONTACT_KEYS = ("n_native", "native_contacts_residue", "n_design", "n_kept", "fnat", "fnonnat", "kept_residue")
INT_KEYS = ("n_pairs", "preserved", "n_pairs_interface", "preserved_interface", "n_native", "native_contacts_residue", "n_design", "n_kept",
            "kept_residue")


# ------------------------------------------------------------------ the rule in numpy (shared with test_gpu_similarity.py)
def ratio(num, den):
    """One fp32 division of two integers, NaN on a zero denominator: the definition of every ratio, for the oracle too."""
    num, den = np.asarray(num, np.int64), np.asarray(den, np.int64)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(den > 0, num.astype(np.float32) / den.astype(np.float32), np.float32(np.nan)).astype(np.float32)


def similarity_np(pts, npts, gen, dtype, group_size=1, residue_mask=None, antigen_mask=None, segment_idx=None, num_segments=0, chain=None,
                  residue_idx=None, inclusion_radius=15.0, contact_distance=8.0, detail=False):
    """pts (rows,K,P,3) and npts (G,K,P,3) fp32 points, masks (G,K) -> every output of the rule.  dtype = np.float32 performs the kernel's
    operations in the kernel's order (one rounded subtraction per difference, d2 = ((dx*dx) + dy*dy) + dz*dz, d = sqrt(d2), comparisons
    on those values); dtype = np.float64 is the oracle on the same points.  Also `boundary` and `contact_boundary` (rows,): the point
    pairs / residue pairs of the row within EDGE of a threshold.  detail=True adds `pairs`, per patch the booleans of every pair."""
    pts, npts = np.asarray(pts, np.float32), np.asarray(npts, np.float32)
    rows, K, P, _ = pts.shape
    N, S, f = group_size, num_segments, dtype
    G = rows // N
    radius, cutoff = f(np.float32(inclusion_radius)), f(np.float32(contact_distance))  # the entry takes them as fp32
    out = {"n_pairs": np.zeros((G, K), np.int32), "preserved": np.zeros((rows, K, 4), np.int32), "n_native": np.zeros(G, np.int32),
           "native_contacts_residue": np.zeros((G, K), np.int32), "n_design": np.zeros(rows, np.int32), "n_kept": np.zeros(rows, np.int32),
           "kept_residue": np.zeros((rows, K), np.int32), "n_pairs_interface": np.zeros((G, K), np.int32),
           "preserved_interface": np.zeros((rows, K, 4), np.int32), "boundary": np.zeros(rows, np.int64),
           "contact_boundary": np.zeros(rows, np.int64), "pairs": []}
    seg_num, seg_den = np.zeros((rows, max(S, 1)), np.int64), np.zeros((rows, max(S, 1)), np.int64)
    counted = np.zeros((rows, K), bool)

    def distances(x, ci):  # (...,K,P,3) -> (...,nc,P,K,P)
        a, b = x[..., ci, :, None, None, :], x[..., None, None, :, :, :]
        dx, dy, dz = a[..., 0] - b[..., 0], a[..., 1] - b[..., 1], a[..., 2] - b[..., 2]
        return np.sqrt(((dx * dx) + dy * dy) + dz * dz)

    for g in range(G):
        present = np.ones(K, bool) if residue_mask is None else np.asarray(residue_mask[g], bool)
        ci = np.flatnonzero(present & np.asarray(gen[g], bool))
        antigen = np.zeros(K, bool) if antigen_mask is None else np.asarray(antigen_mask[g], bool)
        lo = g * N
        counted[lo:lo + N, ci] = True
        dn, dd = distances(npts[g].astype(f), ci), distances(pts[lo:lo + N].astype(f), ci)  # (nc,P,K,P), (N,nc,P,K,P)
        other = present[None, :] & (np.arange(K)[None, :] != ci[:, None])  # (nc,K): j present, j != i
        scored = (dn < radius) & other[:, None, :, None]
        off = np.abs(dd - dn[None])
        pres = np.stack([scored[None] & (off < f(t)) for t in TAU], -1)  # (N,nc,P,K,P,4)
        face = antigen[None, None, :, None]
        out["n_pairs"][g, ci] = scored.sum((1, 2, 3))
        out["n_pairs_interface"][g, ci] = (scored & face).sum((1, 2, 3))
        out["preserved"][lo:lo + N, ci] = pres.sum((2, 3, 4))
        out["preserved_interface"][lo:lo + N, ci] = (pres & face[None, ..., None]).sum((2, 3, 4))
        # contacts
        if antigen_mask is not None:
            partner = other & antigen[None, :]
        elif chain is None:
            partner = other & (np.abs(np.arange(K)[None, :] - ci[:, None]) > 1)
        else:
            c, r = np.asarray(chain[g], np.int64), np.asarray(residue_idx[g], np.int64)
            partner = other & ~((c[None, :] == c[ci][:, None]) & (np.abs(r[None, :] - r[ci][:, None]) == 1))
        cn = (dn < cutoff).any((1, 3)) & partner  # (nc,K)
        cd = (dd < cutoff).any((2, 4)) & partner[None]  # (N,nc,K)
        out["native_contacts_residue"][g, ci] = cn.sum(1)
        out["n_native"][g] = cn.sum()
        out["n_design"][lo:lo + N] = cd.sum((1, 2))
        out["kept_residue"][lo:lo + N, ci] = (cd & cn[None]).sum(2)
        out["n_kept"][lo:lo + N] = (cd & cn[None]).sum((1, 2))
        # boundaries
        near_r = (np.abs(dn - radius) <= EDGE) & other[:, None, :, None]
        near_t = np.zeros(off.shape, bool)
        for t in TAU:
            near_t |= np.abs(off - f(t)) <= EDGE
        near = near_r[None] | (near_t & ((dn < radius + EDGE) & other[:, None, :, None])[None])
        cnear = ((np.abs(dn - cutoff) <= EDGE).any((1, 3))[None] | (np.abs(dd - cutoff) <= EDGE).any((2, 4))) & partner[None]
        out["boundary"][lo:lo + N] = near.sum((1, 2, 3, 4))
        out["contact_boundary"][lo:lo + N] = cnear.sum((1, 2))
        if S:
            labels = np.asarray(segment_idx[g], np.int64)[ci]
            for s in range(S):
                seg_num[lo:lo + N, s] = pres[:, labels == s].sum((1, 2, 3, 4, 5))
                seg_den[lo:lo + N, s] = scored[labels == s].sum()
        if detail:
            out["pairs"].append({"scored": scored, "preserved": pres, "near": near, "native": cn, "design": cd, "contact_near": cnear})

    by_patch = lambda a: np.repeat(a, N, 0)
    n_pairs, n_face = by_patch(out["n_pairs"]).astype(np.int64), by_patch(out["n_pairs_interface"]).astype(np.int64)
    p, q = out["preserved"].astype(np.int64), out["preserved_interface"].astype(np.int64)
    nan = np.float32(np.nan)
    out["lddt_residue"] = np.where(counted, ratio(p.sum(2), 4 * n_pairs), nan)
    out["lddt"] = ratio(p.sum((1, 2)), 4 * n_pairs.sum(1))
    out["lddt_thresholds"] = ratio(p.sum(1), n_pairs.sum(1)[:, None])
    out["ilddt_residue"] = np.where(counted, ratio(q.sum(2), 4 * n_face), nan)
    out["ilddt"] = ratio(q.sum((1, 2)), 4 * n_face.sum(1))
    out["fnat"] = ratio(out["n_kept"], by_patch(out["n_native"]))
    out["fnonnat"] = ratio(out["n_design"] - out["n_kept"], out["n_design"])
    if S:
        out["lddt_segment"] = ratio(seg_num, 4 * seg_den)
    if antigen_mask is None:
        for k in INTERFACE_KEYS:
            del out[k]
    if not detail:
        del out["pairs"]
    return out


def _part(out, keys):
    return {k: v for k, v in out.items() if k in keys}


def lddt_ref(pts, npts, gen, **kw):
    """The float64 oracle of the lDDT outputs (and `boundary`)."""
    return _part(similarity_np(pts, npts, gen, np.float64, **kw), LDDT_KEYS + INTERFACE_KEYS + ("lddt_segment", "boundary"))


def contacts_ref(pts, npts, gen, **kw):
    """The float64 oracle of the native-contact outputs (and `contact_boundary`)."""
    return _part(similarity_np(pts, npts, gen, np.float64, **kw), CONTACT_KEYS + ("contact_boundary",))


def lddt_f32(pts, npts, gen, **kw):
    """The kernel's lDDT arithmetic in numpy float32."""
    return _part(similarity_np(pts, npts, gen, np.float32, **kw), LDDT_KEYS + INTERFACE_KEYS + ("lddt_segment",))


def contacts_f32(pts, npts, gen, **kw):
    """The kernel's contact arithmetic in numpy float32."""
    return _part(similarity_np(pts, npts, gen, np.float32, **kw), CONTACT_KEYS)


# ------------------------------------------------------------------ the inputs of the GPU tests (built on the host, no device needed)
SHAPES = [(2, 3, 16, 1), (2, 5, 130, 4), (1, 1, 64, 4), (3, 70, 128, 1)]  # (G, N, K, P)
VARIANTS = {"plain": (), "antigen": ("antigen",), "masked": ("residue_mask", "segments", "tables"),
            "all": ("antigen", "residue_mask", "segments")}


def case(G, N, K, P, options=(), empty=None, contactless=None, seed=None, copy_native=None):
    """Natives from synthetic.patches - the generator behind sampler_support.patches, coord_sigma = 6 A - and N designs per patch: the
    native with Gaussian displacements of 0.3 to 3 A (one sigma per design) and fresh frames on the generated residues.  At most a third
    of a patch is generated.  The last design of the last patch is a copy of the native (`copy_native`; by default when N > 1).  Options: `antigen` (a third of the non-generated residues), `residue_mask` (removes one
    generated residue and about a tenth of the context), `segments` (labels 0 and 2 on the two halves of the generated residues, label 1
    on nobody that counts, S = 3), `tables` (two chains and a gap in residue_idx).  Patch `empty` has no generated residue; in patch
    `contactless` the native's generated residues stand in a row 12 A apart, 60 A from the rest: scored pairs, but no contact.
    Returns (designs, native, generation_mask, kwargs of metrics.similarity) as host tensors."""
    seed = 100 * K + 10 * N + P if seed is None else seed
    nat = syn.patches(G, K, {"D": 1, "C": 1}, seed=seed, coord_sigma=6.0)
    rng = np.random.default_rng(seed)
    x, O, gm = nat["translations"].numpy().copy(), nat["orientations"].numpy().copy(), nat["generation_mask"].numpy().copy()
    for g in range(G):
        gm[g, np.flatnonzero(gm[g])[K // 3:]] = False
    if empty is not None:
        gm[empty] = False
    if contactless is not None:
        ks = np.flatnonzero(gm[contactless])
        x[contactless, ks] = np.stack([np.full(ks.size, 60.0), 12.0 * np.arange(ks.size), np.zeros(ks.size)], -1).astype(np.float32)
    dx, dO = np.repeat(x, N, 0), np.repeat(O, N, 0)
    gen_rows = np.repeat(gm, N, 0)
    sigma = rng.uniform(0.3, 3.0, (G * N, 1, 1))
    dx = np.where(gen_rows[..., None], dx + sigma * rng.standard_normal(dx.shape), dx).astype(np.float32)
    fresh = syn.random_rotations(rng, G * N * K).reshape(G * N, K, 3, 3).astype(np.float32)
    dO = np.where(gen_rows[..., None, None], fresh, dO)
    if N > 1 if copy_native is None else copy_native:
        dx[-1], dO[-1] = x[-1], O[-1]
    designs = {"seq_idx": torch.zeros(G * N, K, dtype=torch.long), "translations": torch.from_numpy(dx), "orientations": torch.from_numpy(dO)}
    native = {"translations": torch.from_numpy(x), "orientations": torch.from_numpy(O)}
    kw = {"group_size": N, "atoms": "ca" if P == 1 else "backbone"}
    if "antigen" in options:
        kw["antigen_mask"] = torch.from_numpy((rng.random((G, K)) < 1 / 3) & ~gm)
    if "residue_mask" in options:
        rm = rng.random((G, K)) > 0.1
        rm |= gm
        for g in range(G):
            ks = np.flatnonzero(gm[g])
            if ks.size:
                rm[g, ks[ks.size // 2]] = False
        kw["residue_mask"] = torch.from_numpy(rm)
    if "segments" in options:
        seg = np.full((G, K), -1, np.int64)
        for g in range(G):
            ks = np.flatnonzero(gm[g])
            seg[g, ks[:ks.size // 2]], seg[g, ks[ks.size // 2:]] = 0, 2
            seg[g, np.flatnonzero(~gm[g])[:2]] = 1  # (not counted: label 1 stays empty)
        kw.update(segment_idx=torch.from_numpy(seg), num_segments=3)
    if "tables" in options:
        kw["chain_idx"] = torch.from_numpy((np.arange(K) >= K // 2).astype(np.int64))
        kw["residue_idx"] = torch.from_numpy(np.arange(K) + 7 * (np.arange(K) >= K // 3)).expand(G, K).contiguous()
    return designs, native, torch.from_numpy(gm), kw


def host_points(frames, atoms):
    """The points metrics._points takes from the frames, from the host expression of io.backbone_from_frames."""
    x = frames["translations"].float()
    return (x[:, :, None] if atoms == "ca" else backbone_from_frames(x, frames["orientations"].float(), metrics.ATOMS[atoms])).numpy()


def numpy_kwargs(kw, G, K, atoms):
    """metrics.similarity's keywords as similarity_np's (the contact distance's default and the broadcast tables resolved)."""
    out = {"group_size": kw["group_size"], "inclusion_radius": kw.get("inclusion_radius", 15.0),
           "contact_distance": kw.get("contact_distance") or metrics.CONTACT_DISTANCE[atoms], "num_segments": kw.get("num_segments", 0)}
    for name in ("residue_mask", "antigen_mask", "segment_idx"):
        if kw.get(name) is not None:
            out[name] = kw[name].numpy()
    if kw.get("chain_idx") is not None or kw.get("residue_idx") is not None:
        zero, count = torch.zeros(K, dtype=torch.long), torch.arange(K)
        out["chain"] = (zero if kw.get("chain_idx") is None else kw["chain_idx"]).expand(G, K).numpy()
        out["residue_idx"] = (count if kw.get("residue_idx") is None else kw["residue_idx"]).expand(G, K).numpy()
    return out


# ------------------------------------------------------------------ self-checks of the oracle
def ca(x):
    """(rows,K) x coordinates -> CA points (rows,K,1,3) on the x axis."""
    x = np.asarray(x, np.float32)
    return np.stack([x, np.zeros_like(x), np.zeros_like(x)], -1)[:, :, None, :]


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_three_residues_by_hand(dtype):
    """Native x = 0, 3, 7.5; residue 0 is generated and the design puts it at x = -1.  Pair (0,1): d_nat 3, d_des 4, |difference| 1 - not
    below 1, so preserved at 2 and 4 only.  Pair (0,2): 7.5 -> 8.5, the same.  Contacts at 8 A: residue 1 is bonded, residue 2 is in
    contact in the native (7.5) and not in the design (8.5)."""
    nat, des, gen = ca([[0.0, 3.0, 7.5]]), ca([[-1.0, 3.0, 7.5]]), np.array([[True, False, False]])
    out = similarity_np(des, nat, gen, dtype)
    assert out["n_pairs"].tolist() == [[2, 0, 0]] and out["preserved"][0].tolist() == [[0, 0, 2, 2], [0] * 4, [0] * 4]
    assert out["lddt_residue"][0, 0] == 0.5 and np.isnan(out["lddt_residue"][0, 1:]).all() and out["lddt"].tolist() == [0.5]
    assert out["lddt_thresholds"].tolist() == [[0.0, 0.0, 1.0, 1.0]]
    assert out["n_native"].tolist() == [1] and out["native_contacts_residue"].tolist() == [[1, 0, 0]]
    assert out["n_design"].tolist() == [0] and out["n_kept"].tolist() == [0] and out["fnat"].tolist() == [0.0] and np.isnan(out["fnonnat"][0])
    assert out["kept_residue"].tolist() == [[0, 0, 0]] and "ilddt" not in out
    # an inclusion radius of 5 A scores pair (0,1) only; at x = 0.5 it is preserved at 1 A too, and residue 2 stays in contact
    out = similarity_np(ca([[0.5, 3.0, 7.5]]), nat, gen, dtype, inclusion_radius=5.0)
    assert out["n_pairs"].tolist() == [[1, 0, 0]] and out["preserved"][0, 0].tolist() == [0, 1, 1, 1] and out["lddt"].tolist() == [0.75]
    assert out["n_design"].tolist() == [1] and out["n_kept"].tolist() == [1] and out["fnat"].tolist() == [1.0] and out["fnonnat"].tolist() == [0.0]
    assert out["kept_residue"].tolist() == [[1, 0, 0]]
    # residue 1 as the antigen: it is the only partner, bonded or not, and the only interface pair
    out = similarity_np(des, nat, gen, dtype, antigen_mask=np.array([[False, True, False]]))
    assert out["n_pairs_interface"].tolist() == [[1, 0, 0]] and out["preserved_interface"][0, 0].tolist() == [0, 0, 1, 1]
    assert out["ilddt"].tolist() == [0.5] and out["ilddt_residue"][0, 0] == 0.5 and out["n_pairs"].tolist() == [[2, 0, 0]]
    assert out["n_native"].tolist() == [1] and out["n_design"].tolist() == [1] and out["n_kept"].tolist() == [1]
    # residue 2 outside residue_mask: no pair with it; one segment holding residue 0 and an empty one
    out = similarity_np(des, nat, gen, dtype, residue_mask=np.array([[True, True, False]]), segment_idx=np.array([[1, 0, 0]]), num_segments=2)
    assert out["n_pairs"].tolist() == [[1, 0, 0]] and out["n_native"].tolist() == [0] and np.isnan(out["fnat"][0])
    assert np.isnan(out["lddt_segment"][0, 0]) and out["lddt_segment"][0, 1] == 0.5
    # chain tables: residues 0 and 1 on different chains are not bonded, so residue 1 is a partner too
    out = similarity_np(des, nat, gen, dtype, chain=np.array([[0, 1, 1]]), residue_idx=np.array([[0, 1, 2]]))
    assert out["n_native"].tolist() == [2] and out["n_design"].tolist() == [1] and out["n_kept"].tolist() == [1] and out["fnat"].tolist() == [0.5]


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_a_pair_of_two_counted_residues_counts_from_both_sides(dtype):
    nat, gen = ca([[0.0, 3.0, 7.0]]), np.array([[True, True, False]])
    out = similarity_np(nat, nat, gen, dtype)
    assert out["n_pairs"].tolist() == [[2, 2, 0]]  # three unordered pairs, four scored: (0,1) from both sides
    assert out["preserved"][0].sum() == 16 and out["lddt"].tolist() == [1.0]
    # moving residue 0 by 0.75 A changes pair (0,1) on both sides and pair (0,2) once
    out = similarity_np(ca([[-0.75, 3.0, 7.0]]), nat, gen, dtype)
    assert out["preserved"][0].tolist() == [[0, 2, 2, 2], [1, 2, 2, 2], [0] * 4] and out["lddt"][0] == np.float32(13) / np.float32(16)
    # contacts: residue 2 is the partner of residue 0; residue 1 has none, both its neighbours are bonded to it
    assert out["n_native"].tolist() == [1] and out["native_contacts_residue"].tolist() == [[1, 0, 0]]
    both = similarity_np(ca([[0.0, 3.0, 7.0, 4.0]]), ca([[0.0, 3.0, 7.0, 4.0]]), np.array([[True, False, False, True]]), dtype)
    assert both["native_contacts_residue"].tolist() == [[2, 0, 0, 2]] and both["n_native"].tolist() == [4]  # pair (0,3) from both sides


def test_design_equal_to_the_native_and_design_far_away():
    G, N, K, P = 2, 3, 16, 1
    des, nat, gm, kw = case(G, N, K, P)
    npts = host_points(nat, "ca")
    same = similarity_np(np.repeat(npts, N, 0), npts, gm.numpy(), np.float64, group_size=N)
    assert (same["lddt"] == 1.0).all() and (same["fnat"] == 1.0).all() and (same["fnonnat"] == 0.0).all() and (same["n_native"] > 0).all()
    assert (same["lddt_thresholds"] == 1.0).all() and np.array_equal(same["n_kept"], np.repeat(same["n_native"], N))
    far = np.repeat(npts, N, 0)
    ks = np.repeat(gm.numpy(), N, 0)
    far[ks] += (100.0 * (1 + np.arange(int(ks.sum()))))[:, None, None].astype(np.float32)  # every generated residue 100 A from everything
    for dtype in (np.float64, np.float32):
        out = similarity_np(far, npts, gm.numpy(), dtype, group_size=N)
        assert (out["lddt"] == 0.0).all() and (out["n_kept"] == 0).all() and (out["n_design"] == 0).all() and np.isnan(out["fnonnat"]).all()
        assert (out["fnat"] == 0.0).all() and (out["preserved"] == 0).all() and (out["n_pairs"].sum(1) > 0).all()


def test_patch_without_generated_residue_and_native_without_contact():
    des, nat, gm, kw = case(3, 2, 32, 1, empty=1, contactless=2)
    out = similarity_np(host_points(des, "ca"), host_points(nat, "ca"), gm.numpy(), np.float64, group_size=2)
    assert np.isnan(out["lddt"][2:4]).all() and np.isnan(out["fnat"][2:4]).all() and (out["n_pairs"][1] == 0).all()
    assert out["n_native"].tolist()[1:] == [0, 0] and out["n_native"][0] > 0 and np.isnan(out["fnat"][4:]).all()
    assert out["n_pairs"][2].sum() > 0 and not np.isnan(out["lddt"][4:]).any()


# ------------------------------------------------------------------ fp32 against float64 on the GPU tests' inputs
@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_fp32_restatement_disagrees_with_float64_only_at_boundaries(shape, variant):
    G, N, K, P = shape
    des, nat, gm, kw = case(G, N, K, P, VARIANTS[variant], empty=1 if G == 3 else None, contactless=G - 1 if G > 1 else None)
    atoms = kw["atoms"]
    args = (host_points(des, atoms), host_points(nat, atoms), gm.numpy())
    nkw = numpy_kwargs(kw, G, K, atoms)
    lo, hi = similarity_np(*args, np.float32, detail=True, **nkw), similarity_np(*args, np.float64, detail=True, **nkw)
    scored = boundary = differ = 0
    for a, b in zip(lo["pairs"], hi["pairs"]):
        wrong = (a["preserved"] != b["preserved"]).any(-1) | (a["scored"] != b["scored"])[None]
        assert not (wrong & ~b["near"]).any()  # every disagreement is a boundary pair
        cwrong = (a["design"] != b["design"]) | (a["native"] != b["native"])[None]
        assert not (cwrong & ~b["contact_near"]).any()
        scored += int(b["scored"].sum()) * N
        boundary += int(b["near"].sum())
        differ += int(wrong.sum()) + int(cwrong.sum())
    print(f"{shape} {variant}: {scored} scored pairs, {boundary} boundary pairs, {differ} disagreements")
    assert scored > 0 and boundary <= 0.005 * scored
    assert boundary == int(hi["boundary"].sum())
    if differ == 0:
        for k in lo:
            if k not in ("pairs", "boundary", "contact_boundary"):
                assert np.array_equal(lo[k], hi[k], equal_nan=True), k


# ------------------------------------------------------------------ C ABI
NAME = "diffab_metrics_similarity"
N_ARGS = 33


def header_code():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "diffab_hip.h")).read(), flags=re.S)


def test_header_and_symbol_table_declare_the_entry():
    code = header_code()
    lib = _hip.load_library()
    proto = re.search(r"\bint\s+" + NAME + r"\s*\(([^)]*)\)\s*;", code)
    assert proto and len(proto.group(1).split(",")) == N_ARGS
    assert NAME in _hip.SYMBOLS and hasattr(lib, NAME)
    assert not NAME.startswith(("diffab_sample_loop", "diffab_sample_init"))
    res, args = _hip.SYMBOLS[NAME]
    assert res is ctypes.c_int and len(args) == N_ARGS and args[8:13] == [ctypes.c_int32] * 5 and args[13:15] == [ctypes.c_float] * 2
    assert all(a is ctypes.c_void_p for a in args[:8] + args[15:])
    types = [" ".join(a.split()[:-1]) for a in proto.group(1).split(",")]
    assert types[8:15] == ["int32_t"] * 5 + ["float"] * 2 and all(t.endswith("*") for t in types[:8] + types[15:])
    limit = re.search(r"#define\s+DIFFAB_METRICS_SIMILARITY_MAX_POINTS\s+(\d+)", code)
    assert limit and int(limit.group(1)) == metrics.SIMILARITY_MAX_POINTS == 1024
    assert metrics.LDDT_THRESHOLDS == TAU


def test_host_side_refusals_touch_no_gpu():
    """Every refusal is decided from the scalar arguments and whether a pointer is null: the pointers are fake addresses that are never
    dereferenced, nothing is enqueued (no GPU is needed), and diffab_last_error names the problem."""
    l = _hip.load_library()
    p, null = ctypes.c_void_p(4096), ctypes.c_void_p(0)
    INPUTS = ("pts", "npts", "gm", "rm", "ag", "seg", "chain", "ridx")
    OUTPUTS = ("n_pairs", "n_pairs_interface", "preserved", "preserved_interface", "lddt_residue", "lddt", "lddt_thresholds", "ilddt_residue",
               "ilddt", "lddt_segment", "n_native", "native_contacts_residue", "n_design", "n_kept", "fnat", "fnonnat", "kept_residue")

    def err():
        return l.diffab_last_error().decode()

    def call(rows=16, N=8, K=128, P=4, S=0, radius=15.0, cutoff=5.0, **ptrs):
        given = dict(rm=null, ag=null, seg=null, chain=null, ridx=null, n_pairs_interface=null, preserved_interface=null, ilddt_residue=null,
                     ilddt=null, lddt_segment=null)
        given.update(ptrs)
        return l.diffab_metrics_similarity(*[given.get(k, p) for k in INPUTS], rows, N, K, P, S, radius, cutoff,
                                           *[given.get(k, p) for k in OUTPUTS], null)

    cases = [(dict(rows=-8), "extent"), (dict(N=0), "extent"), (dict(K=0), "extent"), (dict(P=0), "points per residue"),
             (dict(P=6), "points per residue"), (dict(rows=4097, N=4097, K=4, P=1), "at most 4096 designs"), (dict(K=4097, P=1), "at most 4096"),
             (dict(K=257), "at most 1024 are staged"), (dict(K=1025, P=1), "at most 1024 are staged"), (dict(K=205, P=5), "at most 1024 are staged"),
             (dict(rows=15), "not a multiple"), (dict(S=9, seg=p), "segments outside"), (dict(S=-1), "segments outside"),
             (dict(S=2), "needs a segment_idx"), (dict(seg=p), "goes with a NULL segment_idx"), (dict(S=2, seg=p), "null segment output"),
             (dict(radius=0.0), "inclusion radius"), (dict(radius=-1.0), "inclusion radius"), (dict(radius=float("nan")), "inclusion radius"),
             (dict(radius=float("inf")), "inclusion radius"), (dict(cutoff=0.0), "contact distance"), (dict(cutoff=float("nan")), "contact distance"),
             (dict(cutoff=float("inf")), "contact distance"), (dict(cutoff=-2.0), "contact distance"),
             (dict(chain=p), "go together"), (dict(ridx=p), "go together"),
             (dict(pts=null), "null input"), (dict(npts=null), "null input"), (dict(gm=null), "null input"), (dict(ag=p), "null interface output")]
    cases += [(dict([(k, null)]), "null lDDT output") for k in ("n_pairs", "preserved", "lddt_residue", "lddt", "lddt_thresholds")]
    cases += [(dict([(k, null)]), "null contact output") for k in CONTACT_KEYS]
    cases += [(dict([("ag", p), ("n_pairs_interface", p), ("preserved_interface", p), ("ilddt_residue", p), ("ilddt", p), (k, null)]),
               "null interface output") for k in INTERFACE_KEYS]
    for kw, word in cases:
        rc = call(**kw)
        assert rc == -1 and word in err(), (kw, rc, err())  # DIFFAB_ERR_ARG
    # the limits themselves pass the checks, and an empty problem returns 0 before any pointer is looked at
    assert l.diffab_metrics_similarity(*[null] * 8, 0, 4096, 256, 4, 0, 15.0, 5.0, *[null] * 17, null) == 0
    assert l.diffab_metrics_similarity(*[null] * 8, 0, 1, 1024, 1, 0, 15.0, 8.0, *[null] * 17, null) == 0
    assert l.diffab_metrics_similarity(*[null] * 5, p, null, null, 0, 1, 204, 5, 8, 15.0, 8.0, *[null] * 17, null) == 0


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
    native = {k: v for k, v in frames(2).items() if k != "seq_idx"}
    with pytest.raises(ReachedTheLibrary):
        metrics.similarity(frames(), native, mask(), group_size=3)
    with pytest.raises(ReachedTheLibrary):
        metrics.similarity(frames(), frames(6), mask(), group_size=3, atoms="backbone", residue_mask=mask(), antigen_mask=~mask(),
                           segment_idx=torch.zeros(2, 16, dtype=torch.long), inclusion_radius=12, contact_distance=4.5)
    with pytest.raises(ReachedTheLibrary):
        metrics.similarity(frames(), native, mask(), group_size=3, segment_idx=torch.full((2, 16), 7), chain_idx=torch.zeros(16, dtype=torch.long),
                           residue_idx=torch.arange(16).expand(2, 16))
    with pytest.raises(ReachedTheLibrary):
        metrics.similarity(frames(4, 256), frames(4, 256), mask(4, 256), atoms="backbone")


@pytest.mark.parametrize("kw, match", [
    (dict(atoms="cb"), "atoms must be 'ca' or 'backbone'"), (dict(group_size=4), "6 design rows are not a multiple of group_size = 4"),
    (dict(group_size=0), "group_size must be"), (dict(group_size=True), "group_size must be"),
    (dict(generation_mask=mask().long()), "generation_mask must be a bool tensor"), (dict(generation_mask=mask(3)), "generation_mask is"),
    (dict(residue_mask=mask(2, 15)), "residue_mask is"), (dict(residue_mask=mask().float()), "residue_mask must be a bool tensor"),
    (dict(designs={"seq_idx": torch.zeros(6, 16, dtype=torch.long)}), "designs must be a dict"),
    (dict(designs=dict(frames(), translations=torch.zeros(6, 15, 3))), r"designs\['translations'\] is"),
    (dict(designs=dict(frames(), orientations=torch.zeros(6, 16, 3)), atoms="backbone"), r"designs\['orientations'\] must be"),
    (dict(designs=frames(4097, 4), native=frames(1, 4), generation_mask=mask(1, 4), group_size=4097), "at most 4096 designs"),
    (dict(native=None), "native must be a dict"), (dict(native={"orientations": torch.eye(3).expand(2, 16, 3, 3)}), "native must be a dict"),
    (dict(native=frames(3)), r"native\['translations'\] is \(3, 16, 3\)"), (dict(native=frames(2, 15)), r"native\['translations'\] is"),
    (dict(native={"translations": torch.zeros(2, 16, 3, dtype=torch.long)}), r"native\['translations'\] is"),
    (dict(native={"translations": torch.zeros(2, 16, 3)}, atoms="backbone"), r"native\['orientations'\] must be"),
    (dict(native=dict(frames(2), orientations=torch.zeros(6, 16, 3, 3)), atoms="backbone"), r"native\['orientations'\] must be"),
    (dict(designs=frames(2, 257), native=frames(2, 257), generation_mask=mask(2, 257), group_size=1, atoms="backbone"), "at most 1024 are staged"),
    (dict(designs=frames(1, 1025), native=frames(1, 1025), generation_mask=mask(1, 1025), group_size=1), "at most 1024 are staged"),
    (dict(antigen_mask=mask().long()), "antigen_mask must be a bool tensor"), (dict(antigen_mask=mask(2, 15)), "antigen_mask is"),
    (dict(segment_idx=torch.zeros(2, 16)), "segment_idx must be an integer tensor"), (dict(segment_idx=mask()), "segment_idx must be an integer"),
    (dict(segment_idx=torch.zeros(3, 16, dtype=torch.long)), "segment_idx is"), (dict(segment_idx=torch.full((2, 16), 8)), "num_segments = 9"),
    (dict(segment_idx=torch.zeros(2, 16, dtype=torch.long), num_segments=9), "num_segments = 9"), (dict(num_segments=2), "num_segments without"),
    (dict(inclusion_radius=0), "inclusion_radius must be a finite number > 0"), (dict(inclusion_radius=float("nan")), "inclusion_radius must be"),
    (dict(inclusion_radius=float("inf")), "inclusion_radius must be"), (dict(inclusion_radius="15"), "inclusion_radius must be"),
    (dict(inclusion_radius=True), "inclusion_radius must be"), (dict(contact_distance=0.0), "contact_distance must be a finite number > 0"),
    (dict(contact_distance=-8.0), "contact_distance must be"), (dict(contact_distance=float("inf")), "contact_distance must be"),
    (dict(chain_idx=torch.zeros(16)), "needs an integer chain_idx"), (dict(residue_idx=torch.arange(15)), "residue_idx .* does not broadcast"),
    (dict(residue_idx=torch.zeros(1, 2, 16, dtype=torch.long)), r"residue_idx must be \(K,\) or \(rows, K\)"),
])
def test_argument_errors(no_library, kw, match):
    args = dict(designs=frames(), native=frames(2), generation_mask=mask(), group_size=3)
    args.update(kw)
    designs, native, gm = args.pop("designs"), args.pop("native"), args.pop("generation_mask")
    with pytest.raises(ValueError, match=r"metrics\.similarity\(\): .*" + match):
        metrics.similarity(designs, native, gm, **args)
