"""CPU: the host side of the design filters (diffab_pytorch.metrics.backbone / .contacts) - the numpy oracle of
the two rules with its self-checks, a NeRF chain builder on the ideal backbone geometry, the C-ABI entries and their host-side refusals,
and the argument checks that happen before any library call.

The rules are the header comments of diffab_metrics_backbone / diffab_metrics_contacts in include/diffab_hip.h.  backbone_ref is float64;
contacts_ref takes the squared distances and every comparison in numpy float32, grouped as the header fixes them, so its counts are the
numbers the kernels must EQUAL, and its scores in float64.  test_gpu_geometry.py imports the oracle and the builder from here."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from diffab_pytorch import _hip, io as dio, metrics
from sampler_support import ReachedTheLibrary, refuse_library

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PEPTIDE = 1.329


# ------------------------------------------------------------------ the oracle (shared with test_gpu_geometry.py)
def dihedral_ref(p0, p1, p2, p3):
    """IUPAC dihedral in (-pi, pi] -> (angle, |b1 x b2|, |b2 x b3|), float64."""
    p0, p1, p2, p3 = (np.asarray(p, np.float64) for p in (p0, p1, p2, p3))
    b1, b2, b3 = p1 - p0, p2 - p1, p3 - p2
    n1, n2 = np.cross(b1, b2), np.cross(b2, b3)
    a = np.arctan2(np.linalg.norm(b2) * np.dot(b1, n2), np.dot(n1, n2))
    return (np.pi if a <= -np.pi else a), np.linalg.norm(n1), np.linalg.norm(n2)


def neighbours(chain, ridx, rm):
    """succ, pred (K,) of one patch: the lowest slot with the same chain and residue_idx + 1 / - 1, both inside rm; -1 without one."""
    K = len(chain)
    succ, pred = np.full(K, -1), np.full(K, -1)
    for i in range(K):
        if not rm[i]:
            continue
        for j in range(K):
            if not rm[j] or chain[j] != chain[i]:
                continue
            gap = int(ridx[j]) - int(ridx[i])
            if gap == 1 and succ[i] < 0:
                succ[i] = j
            if gap == -1 and pred[i] < 0:
                pred[i] = j
    return succ, pred


INT32_MIN, INT32_MAX = -2 ** 31, 2 ** 31 - 1


def tangle_chain_keys(chain, ridx, rm, at, far):
    """Rewrites, in place, the keys of one patch so that each way to get the chain rule wrong gives other links.  Slots at .. at + 12
    must be a run of one chain numbered r, r + 1, ... and inside rm; `far` is a slot of another chain.  Afterwards
      - slot `at` has residue_idx INT32_MIN and `far`, moved into the run's chain, INT32_MAX: no neighbours, a 32-bit gap says they are;
      - slot at + 4 repeats the key of at + 2: the lower slot is the neighbour of at + 1 and at + 3;
      - slot at + 7, outside rm, carries the key of at + 9 ahead of it: it is skipped;
      - slot at + 10, in `far`'s old chain, carries the number of at + 12 ahead of it: another chain is no neighbour.
    Returns {slot: (succ, pred)}, the links the rule gives the rewritten slots (derived by hand, not by a reference)."""
    c, r, other = chain[at], int(ridx[at]), chain[far]
    assert other != c and rm[at:at + 13].all() and (chain[at:at + 13] == c).all() and (ridx[at:at + 13] == r + np.arange(13)).all()
    ridx[at], ridx[far], chain[far] = INT32_MIN, INT32_MAX, c
    ridx[at + 4] = r + 2
    ridx[at + 7], rm[at + 7] = r + 9, False
    ridx[at + 10], chain[at + 10] = r + 12, other
    a = at
    return {a: (-1, -1), far: (-1, -1), a + 1: (a + 2, -1), a + 2: (a + 3, a + 1), a + 3: (-1, a + 2), a + 4: (a + 3, a + 1),
            a + 5: (a + 6, -1), a + 6: (-1, a + 5), a + 7: (-1, -1), a + 8: (a + 9, -1), a + 9: (-1, a + 8), a + 11: (a + 12, -1)}


def dihedrals_ref(p0, p1, p2, p3):
    """dihedral_ref over leading axes: (…,3) float64 points -> angle (…), the smaller of the two cross-product norms (…)."""
    b1, b2, b3 = p1 - p0, p2 - p1, p3 - p2
    n1, n2 = np.cross(b1, b2), np.cross(b2, b3)
    a = np.arctan2(np.linalg.norm(b2, axis=-1) * (b1 * n2).sum(-1), (n1 * n2).sum(-1))
    return np.where(a <= -np.pi, np.pi, a), np.minimum(np.linalg.norm(n1, axis=-1), np.linalg.norm(n2, axis=-1))


def backbone_ref(points, gen, chain, ridx, rm, group_size=1, bond_tolerance=0.25):
    """points (rows,K,3,3) = N, CA, C; gen / chain / ridx / rm (G,K).  -> dict: phi, psi, omega, peptide_bond (rows,K) float64 (NaN
    where undefined), the four row outputs, and for the tests' own preconditions `min_cross` (the smallest cross-product norm of any
    defined dihedral), `tolerance_gap` (the smallest | |d - 1.329| - bond_tolerance | over the counted bonds) and `cis_gap` (the
    smallest | |omega| - pi/2 | over them)."""
    rows, K = points.shape[:2]
    out = {k: np.full((rows, K), np.nan) for k in ("phi", "psi", "omega", "peptide_bond")}
    out.update(n_bonds=np.zeros(rows, np.int32), max_peptide_deviation=np.zeros(rows), n_chain_break=np.zeros(rows, np.int32),
               n_cis=np.zeros(rows, np.int32), min_cross=np.inf, tolerance_gap=np.inf, cis_gap=np.inf)
    tol = float(np.float32(bond_tolerance))
    for g in range(gen.shape[0]):
        succ, pred = neighbours(chain[g], ridx[g], rm[g])
        sl = slice(g * group_size, (g + 1) * group_size)
        p = np.asarray(points[sl], np.float64)
        n, ca, c = p[:, :, 0], p[:, :, 1], p[:, :, 2]
        has_p, has_s = pred >= 0, succ >= 0
        phi, x0 = dihedrals_ref(c[:, pred], n, ca, c)
        psi, x1 = dihedrals_ref(n, ca, c, n[:, succ])
        omega, x2 = dihedrals_ref(ca, c, n[:, succ], ca[:, succ])
        d = np.linalg.norm(c - n[:, succ], axis=-1)
        out["phi"][sl] = np.where(has_p, phi, np.nan)
        out["psi"][sl], out["omega"][sl], out["peptide_bond"][sl] = (np.where(has_s, v, np.nan) for v in (psi, omega, d))
        for x, has in ((x0, has_p), (x1, has_s), (x2, has_s)):
            out["min_cross"] = min(out["min_cross"], x[:, has].min(initial=np.inf))
        counted = has_s & (gen[g] | gen[g][succ])
        dev, w = np.abs(d - PEPTIDE)[:, counted], np.abs(omega)[:, counted]
        out["n_bonds"][sl] = int(counted.sum())
        out["max_peptide_deviation"][sl] = dev.max(axis=1, initial=0.0)
        out["n_chain_break"][sl] = (dev > tol).sum(1)
        out["n_cis"][sl] = (w < np.pi / 2).sum(1)
        out["tolerance_gap"] = min(out["tolerance_gap"], np.abs(dev - tol).min(initial=np.inf))
        out["cis_gap"] = min(out["cis_gap"], np.abs(w - np.pi / 2).min(initial=np.inf))
    return out


def d2_f32(a, b):
    """(n,3), (m,3) float32 -> (n,m) float32: (dx*dx + dy*dy) + dz*dz, every operation rounded to float32."""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    dx, dy, dz = (a[:, None, x] - b[None, :, x] for x in range(3))
    return (dx * dx + dy * dy) + dz * dz


def atoms_of(points, bits, residues):
    """The valid atoms of the listed residues: (n,3) float32 coordinates and (n,) their residue slot."""
    xyz, owner = [], []
    for k in residues:
        for a in range(points.shape[1]):
            if (int(bits[k]) >> a) & 1:
                xyz.append(points[k, a])
                owner.append(k)
    return np.asarray(xyz, np.float32).reshape(-1, 3), np.asarray(owner, np.int64)


def contacts_ref(points, valid, ctx_points, ctx_valid, gen, rm, chain, ridx, antigen=None, hotspot=None, group_size=1, clash_distance=3.0,
                 contact_distance=5.0):
    """points (rows,K,P,3) fp32 with validity bits valid (rows,K); ctx_points (G,K,A,3) fp32 with bits ctx_valid (G,K); gen, rm, chain,
    ridx, antigen, hotspot (G,K).  -> dict of the outputs of diffab_metrics_contacts (clash_score float64, min_distance float32)."""
    rows, K = points.shape[:2]
    G = gen.shape[0]
    clash, contact = np.float32(clash_distance), np.float32(contact_distance)
    clash2, contact2 = clash * clash, contact * contact
    antigen = np.zeros((G, K), bool) if antigen is None else np.asarray(antigen, bool)
    hotspot = np.zeros((G, K), bool) if hotspot is None else np.asarray(hotspot, bool)
    out = {k: np.zeros(rows, np.int32) for k in ("n_clash", "n_contact_pairs", "n_paratope", "n_epitope", "n_hotspot_contacted", "n_hotspot")}
    out.update(clash_score=np.zeros(rows), min_distance=np.full(rows, np.inf, np.float32), residue_clash=np.zeros((rows, K), np.int32),
               residue_contact=np.zeros((rows, K), np.int32))
    context = {}
    for r in range(rows):
        g = r // group_size
        gen_res = np.flatnonzero(gen[g] & rm[g])
        if g not in context:
            context[g] = atoms_of(np.asarray(ctx_points[g], np.float32), ctx_valid[g], np.flatnonzero(~gen[g] & rm[g]))
        cxyz, cown = context[g]
        gxyz, gown = atoms_of(np.asarray(points[r], np.float32), valid[r], gen_res)
        out["n_hotspot"][r] = int((~gen[g] & rm[g] & antigen[g] & hotspot[g]).sum())
        bonded = (chain[g][:, None] == chain[g][None, :]) & (np.abs(ridx[g][:, None].astype(np.int64) - ridx[g][None, :]) == 1)
        contact_pair = np.zeros((K, K), bool)
        for oxyz, oown, same in ((cxyz, cown, False), (gxyz, gown, True)):
            if gxyz.shape[0] == 0 or oxyz.shape[0] == 0:
                continue
            d2 = d2_f32(gxyz, oxyz)
            ok = ~bonded[gown[:, None], oown[None, :]]
            ok &= (gown[:, None] < oown[None, :]) if same else True  # two generated residues: the unordered residue pair once
            if not ok.any():
                continue
            out["min_distance"][r] = min(out["min_distance"][r], np.sqrt(d2[ok].min()))
            hit = ok & (d2 < clash2)
            out["n_clash"][r] += int(hit.sum())
            d = np.sqrt(d2[hit]).astype(np.float64)  # the fp32 root, widened
            out["clash_score"][r] += float(((float(clash) - d) ** 2).sum())
            ia, ib = np.nonzero(hit)
            np.add.at(out["residue_clash"][r], gown[ia], 1)
            np.add.at(out["residue_clash"][r], oown[ib], 1)
            if not same:
                ia, ib = np.nonzero(ok & (d2 < contact2) & antigen[g][oown][None, :])
                contact_pair[gown[ia], oown[ib]] = True
        out["n_contact_pairs"][r] = int(contact_pair.sum())
        out["residue_contact"][r] = contact_pair.sum(1) + contact_pair.sum(0)
        out["n_paratope"][r] = int(contact_pair.any(1).sum())
        out["n_epitope"][r] = int(contact_pair.any(0).sum())
        out["n_hotspot_contacted"][r] = int((contact_pair.any(0) & hotspot[g]).sum())
    return out


# ------------------------------------------------------------------ a NeRF chain on the ideal backbone geometry
_N, _C = np.array(dio.IDEAL_BACKBONE["N"], np.float64), np.array(dio.IDEAL_BACKBONE["C"], np.float64)
L_N_CA, L_CA_C = float(np.linalg.norm(_N)), float(np.linalg.norm(_C))
ANGLE_N_CA_C = float(np.arccos(np.dot(_N, _C) / (L_N_CA * L_CA_C)))
ANGLE_CA_C_N, ANGLE_C_N_CA = np.deg2rad(116.2), np.deg2rad(121.7)


def place(a, b, c, length, angle, torsion):
    """The point d with |c d| = length, angle(b, c, d) = angle and dihedral(a, b, c, d) = torsion."""
    bc = (c - b) / np.linalg.norm(c - b)
    n = np.cross(b - a, bc)
    n /= np.linalg.norm(n)
    m = np.cross(n, bc)
    return c + length * (-np.cos(angle) * bc + np.sin(angle) * np.cos(torsion) * m + np.sin(angle) * np.sin(torsion) * n)


def nerf_chain(phi, psi, omega, peptide=None):
    """len(phi) residues -> (L,3,3) float64 N, CA, C.  phi[0], psi[-1] and omega[-1] are not used; peptide: the C-N bond lengths
    (default 1.329 everywhere).  The first residue lies in the ideal local frame."""
    L = len(phi)
    peptide = [PEPTIDE] * L if peptide is None else peptide
    out = np.zeros((L, 3, 3))
    out[0] = _N, (0.0, 0.0, 0.0), _C
    for i in range(1, L):
        n = place(out[i - 1, 0], out[i - 1, 1], out[i - 1, 2], peptide[i - 1], ANGLE_CA_C_N, psi[i - 1])
        ca = place(out[i - 1, 1], out[i - 1, 2], n, L_N_CA, ANGLE_C_N_CA, omega[i - 1])
        c = place(out[i - 1, 2], n, ca, L_CA_C, ANGLE_N_CA_C, phi[i])
        out[i] = n, ca, c
    return out


def frames_of(backbone):
    """(…,3,3) float64 N, CA, C -> translations (…,3), orientations (…,3,3) float64 (io.frames_from_backbone)."""
    b = torch.from_numpy(np.asarray(backbone, np.float64))
    t, R = dio.frames_from_backbone(b[..., 0, :], b[..., 1, :], b[..., 2, :])
    return t.numpy(), R.numpy()


def wrapped(a, b):
    d = np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64)) % (2 * np.pi)
    return np.minimum(d, 2 * np.pi - d)


# ------------------------------------------------------------------ self-checks of the oracle
def test_dihedral_sign_on_a_hand_case():
    # looking from p1 to p2 (along +z) the front bond (+x) turns clockwise by a quarter onto the rear bond (+y): +90 degrees (IUPAC)
    a, _, _ = dihedral_ref((1, 0, 0), (0, 0, 0), (0, 0, 1), (0, 1, 1))
    assert abs(a - np.pi / 2) < 1e-15
    assert abs(dihedral_ref((1, 0, 0), (0, 0, 0), (0, 0, 1), (0, -1, 1))[0] + np.pi / 2) < 1e-15
    assert dihedral_ref((1, 0, 0), (0, 0, 0), (0, 0, 1), (-1, 0, 1))[0] == np.pi  # trans is +pi, never -pi
    assert dihedral_ref((1, 0, 0), (0, 0, 0), (0, 0, 1), (1, 0, 1))[0] == 0.0


def chain_case(L=12, seed=0):
    rng = np.random.default_rng(seed)
    phi, psi = rng.uniform(-2.8, -0.8, L), rng.uniform(-1.0, 2.8, L)
    omega = np.full(L, np.pi) + rng.normal(0.0, 0.05, L)
    return phi, psi, omega


def one_patch(L):
    return np.zeros((1, L), np.int64), np.arange(L)[None], np.ones((1, L), bool)


def test_the_builder_returns_its_dihedrals_and_round_trips_through_frames():
    phi, psi, omega = chain_case()
    bb = nerf_chain(phi, psi, omega)
    L = len(phi)
    chain, ridx, rm = one_patch(L)
    gen = np.ones((1, L), bool)
    ref = backbone_ref(bb[None], gen, chain, ridx, rm)
    assert np.isnan(ref["phi"][0, 0]) and np.isnan(ref["psi"][0, -1]) and np.isnan(ref["omega"][0, -1]) and np.isnan(ref["peptide_bond"][0, -1])
    assert wrapped(ref["phi"][0, 1:], phi[1:]).max() < 1e-9
    assert wrapped(ref["psi"][0, :-1], psi[:-1]).max() < 1e-9
    assert wrapped(ref["omega"][0, :-1], omega[:-1]).max() < 1e-9
    assert np.abs(ref["peptide_bond"][0, :-1] - PEPTIDE).max() < 1e-12
    assert ref["n_bonds"][0] == L - 1 and ref["n_chain_break"][0] == 0 and ref["n_cis"][0] == 0 and ref["max_peptide_deviation"][0] < 1e-12
    assert ref["min_cross"] > 1.0
    # the frames of the chain give the same N, CA, C back: the builder uses the ideal lengths and the ideal N-CA-C angle
    t, R = frames_of(bb)
    back = dio.backbone_from_frames(torch.from_numpy(t), torch.from_numpy(R), ("N", "CA", "C")).numpy()
    assert np.abs(back - bb).max() < 1e-5  # (IDEAL_BACKBONE goes through float32 inside backbone_from_frames)


def test_cis_stretched_and_deleted_are_counted():
    phi, psi, omega = chain_case(10, seed=1)
    omega[3] = 0.1  # a cis bond 3 -> 4
    peptide = [PEPTIDE] * 10
    peptide[6] = 1.9  # a stretched bond 6 -> 7
    bb = nerf_chain(phi, psi, omega, peptide)
    chain, ridx, rm = one_patch(10)
    gen = np.ones((1, 10), bool)
    ref = backbone_ref(bb[None], gen, chain, ridx, rm)
    assert ref["n_bonds"][0] == 9 and ref["n_cis"][0] == 1 and ref["n_chain_break"][0] == 1
    assert abs(ref["max_peptide_deviation"][0] - (1.9 - PEPTIDE)) < 1e-12
    # a deleted residue: residue_idx jumps by 2 after slot 4 - no bond 4 -> 5, and nothing defined across it
    gap = ridx.copy()
    gap[0, 5:] += 1
    ref = backbone_ref(bb[None], gen, chain, gap, rm)
    assert ref["n_bonds"][0] == 8 and np.isnan(ref["psi"][0, 4]) and np.isnan(ref["phi"][0, 5]) and np.isnan(ref["peptide_bond"][0, 4])
    # only bonds with a generated end are counted: generated 3..4 -> bonds 2-3, 3-4 (cis) and, without the gap, 4-5
    gen = np.zeros((1, 10), bool)
    gen[0, 3:5] = True
    assert backbone_ref(bb[None], gen, chain, ridx, rm)["n_bonds"][0] == 3 and backbone_ref(bb[None], gen, chain, gap, rm)["n_bonds"][0] == 2
    assert backbone_ref(bb[None], gen, chain, ridx, rm)["n_chain_break"][0] == 0
    # a residue outside residue_mask bonds to nothing; another chain bonds to nothing
    rm2 = rm.copy()
    rm2[0, 4] = False
    assert backbone_ref(bb[None], gen, chain, ridx, rm2)["n_bonds"][0] == 1
    chain2 = chain.copy()
    chain2[0, 4:] = 1
    assert backbone_ref(bb[None], gen, chain2, ridx, rm)["n_bonds"][0] == 2


def two_atoms(distance):
    """Residue 0 generated with one atom at the origin, residue 2 context with one atom at `distance` on x (residue 1 is absent)."""
    pts = np.zeros((1, 3, 1, 3), np.float32)
    ctx = np.zeros((1, 3, 1, 3), np.float32)
    ctx[0, 2, 0, 0] = distance
    gen = np.array([[True, False, False]])
    rm = np.array([[True, False, True]])
    chain, ridx, _ = one_patch(3)
    return contacts_ref(pts, np.ones((1, 3), np.uint8), ctx, np.ones((1, 3), np.int64), gen, rm, chain, ridx, antigen=~gen,
                        hotspot=np.array([[False, False, True]]))


def test_two_hand_placed_atoms():
    near, far = two_atoms(2.9), two_atoms(3.1)
    assert near["n_clash"][0] == 1 and far["n_clash"][0] == 0
    assert abs(near["clash_score"][0] - (3.0 - float(np.float32(np.sqrt(np.float32(2.9) ** 2)))) ** 2) < 1e-12 and far["clash_score"][0] == 0.0
    assert near["min_distance"][0] == np.float32(2.9) and far["min_distance"][0] == np.float32(3.1)
    assert near["residue_clash"][0].tolist() == [1, 0, 1] and far["residue_clash"][0].tolist() == [0, 0, 0]
    for out in (near, far):  # both are within the contact distance
        assert out["n_contact_pairs"][0] == 1 and out["n_paratope"][0] == 1 and out["n_epitope"][0] == 1
        assert out["n_hotspot"][0] == 1 and out["n_hotspot_contacted"][0] == 1 and out["residue_contact"][0].tolist() == [1, 0, 1]
    away = two_atoms(5.1)
    assert away["n_contact_pairs"][0] == 0 and away["residue_contact"][0].tolist() == [0, 0, 0] and away["n_hotspot"][0] == 1


def test_chain_neighbours_and_generated_pairs():
    # three generated residues on a line, 1 A apart, one atom each: 0-1 and 1-2 are chain neighbours, 0-2 (2 A) clashes once
    pts = np.zeros((1, 3, 1, 3), np.float32)
    pts[0, :, 0, 0] = [0.0, 1.0, 2.0]
    chain, ridx, rm = one_patch(3)
    gen = np.ones((1, 3), bool)
    bits = np.ones((1, 3), np.uint8)
    out = contacts_ref(pts, bits, pts, np.zeros((1, 3), np.int64), gen, rm, chain, ridx)
    assert out["n_clash"][0] == 1 and out["residue_clash"][0].tolist() == [1, 0, 1] and out["min_distance"][0] == np.float32(2.0)
    assert abs(out["clash_score"][0] - 1.0) < 1e-12
    # on different chains nothing is bonded: three pairs
    out = contacts_ref(pts, bits, pts, np.zeros((1, 3), np.int64), gen, rm, np.array([[0, 1, 2]]), ridx)
    assert out["n_clash"][0] == 3 and out["residue_clash"][0].tolist() == [2, 2, 2] and out["min_distance"][0] == np.float32(1.0)
    # an atom whose bit is clear does not exist; no pair at all gives +inf
    out = contacts_ref(pts, np.array([[1, 1, 0]], np.uint8), pts, np.zeros((1, 3), np.int64), gen, rm, chain, ridx)
    assert out["n_clash"][0] == 0 and out["min_distance"][0] == np.inf


def test_every_reference_of_the_chain_rule_takes_the_gap_in_64_bits_and_the_lowest_slot():
    """The four entries that link chain neighbours share one kernel; their tests share tangle_chain_keys.  What the references (this
    file's, the hydrogen bonds' and the motifs') make of such keys is checked here against links derived by hand."""
    from developability_ref import succ_ref  # (imports this module)
    from test_hbonds_host import links

    K = 40
    chain, rm = np.repeat([1, 2], K // 2).astype(np.int32), np.ones(K, bool)
    ridx = np.arange(K, dtype=np.int32) + 7
    expect = tangle_chain_keys(chain, ridx, rm, 3, K - 1)
    assert ridx.dtype == np.int32 and int(ridx[K - 1]) - int(ridx[3]) == 2 ** 32 - 1  # (the difference is 1 where it wraps)
    for name, (succ, pred) in (("neighbours", neighbours(chain, ridx, rm)), ("links", links(chain, ridx, rm)),
                               ("succ_ref", (succ_ref(rm, chain, ridx), None))):
        for slot, (s, p) in expect.items():
            assert succ[slot] == s and (pred is None or pred[slot] == p), (name, slot, succ[slot], s, None if pred is None else pred[slot], p)
    # bonded pairs in either direction, as contacts_ref and refine_ref ask: the two ends of the int32 range are not bonded
    gap = ridx.astype(np.int64)[:, None] - ridx[None, :]
    assert abs(int(gap[K - 1, 3])) == 2 ** 32 - 1


# ------------------------------------------------------------------ C ABI
NAMES = ("diffab_metrics_backbone", "diffab_metrics_contacts")


def test_header_and_symbol_table_declare_the_two_entries():
    src = open(os.path.join(REPO, "include", "diffab_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    lib = _hip.load_library()
    for name in NAMES:
        assert re.search(r"\bint\s+" + name + r"\s*\(", code), name
        assert name in _hip.SYMBOLS and hasattr(lib, name), name
        res, args = _hip.SYMBOLS[name]
        assert res is ctypes.c_int and args[-1] is ctypes.c_void_p and args[-2] is ctypes.c_size_t
    bb, ct = (_hip.SYMBOLS[n][1] for n in NAMES)
    assert len(bb) == 20 and bb[5:8] == [ctypes.c_int32] * 3 and bb[8] is ctypes.c_float
    assert len(ct) == 30 and ct[10:15] == [ctypes.c_int32] * 5 and ct[15:17] == [ctypes.c_float] * 2
    macro = {k: int(v) for k, v in re.findall(r"#define\s+DIFFAB_METRICS_(MAX_CONTEXT_ATOMS|CONTACTS_CHUNK_ATOMS|CONTACTS_CHUNK_RESIDUES)\s+(\d+)", code)}
    assert macro == {"MAX_CONTEXT_ATOMS": metrics.MAX_CONTEXT_ATOMS, "CONTACTS_CHUNK_ATOMS": metrics.CONTACTS_CHUNK_ATOMS,
                     "CONTACTS_CHUNK_RESIDUES": metrics.CONTACTS_CHUNK_RESIDUES}
    assert metrics.GLY == 7 and dio.AA3[7] == "GLY" and metrics.PEPTIDE_BOND == PEPTIDE


def test_host_side_refusals_touch_no_gpu():
    """Every refusal is decided from the scalar arguments and whether a pointer is null: the pointers are fake addresses that are never
    dereferenced, nothing is enqueued (no GPU is needed), and diffab_last_error names the problem."""
    l = _hip.load_library()
    p, null = ctypes.c_void_p(4096), ctypes.c_void_p(0)

    def err():
        return l.diffab_last_error().decode()

    def bb(rows=10, group=5, K=128, tol=0.25, pts=p, rm=null, chain=p, out=p, last=p, ws=p, ws_bytes=1 << 40):
        return l.diffab_metrics_backbone(pts, p, rm, chain, p, rows, group, K, tol, out, p, p, p, p, p, p, last, ws, ws_bytes, null)

    for kw, word in ((dict(rows=11), "not a multiple"), (dict(rows=-5), "extent"), (dict(group=0), "extent"), (dict(K=0), "extent"),
                     (dict(group=4097, rows=4097), "at most 4096 designs"), (dict(K=4097), "at most 4096"),
                     (dict(tol=-0.1), "bond_tolerance"), (dict(tol=float("nan")), "bond_tolerance"), (dict(tol=float("inf")), "bond_tolerance"),
                     (dict(pts=null), "null input"), (dict(chain=null), "null input"), (dict(out=null), "null output"),
                     (dict(last=null), "null output"), (dict(ws=null), "workspace"), (dict(ws=ctypes.c_void_p(4100)), "16-byte aligned")):
        rc = bb(**kw)
        assert rc == -1 and word in err(), (kw, rc, err())
    need = metrics.backbone_workspace_bytes(2, 128)
    assert bb(ws_bytes=need // 2) == -4 and "needed" in err()  # DIFFAB_ERR_WORKSPACE
    assert need - 1024 <= int(re.search(r"(\d+) needed", err()).group(1)) <= need

    def ct(rows=10, group=5, K=128, P=5, A=15, clash=3.0, contact=5.0, pts=p, valid=p, ctx=p, ag=null, hs=null, out=p, rc_out=p, pairs=p, rct=p,
           hot=p, ws=p, ws_bytes=1 << 40):
        return l.diffab_metrics_contacts(pts, valid, ctx, p, p, null, ag, hs, p, p, rows, group, K, P, A, clash, contact, out, p, p, pairs, p, p,
                                         hot, p, rc_out, rct, ws, ws_bytes, null)

    for kw, word in ((dict(rows=11), "not a multiple"), (dict(rows=-5), "extent"), (dict(group=0), "extent"), (dict(K=0), "extent"),
                     (dict(group=4097, rows=4097), "at most 4096 designs"), (dict(K=4097), "at most 4096"), (dict(P=0), "points per residue"),
                     (dict(P=6), "points per residue"), (dict(A=0), "context atoms per residue"), (dict(A=33), "context atoms per residue"),
                     (dict(clash=-1.0), "clash_distance"), (dict(clash=float("nan")), "clash_distance"), (dict(contact=float("inf")), "contact_distance"),
                     (dict(contact=-2.0), "contact_distance"), (dict(hs=p), "needs an antigen_mask"), (dict(pts=null), "null input"),
                     (dict(valid=null), "null input"), (dict(ctx=null), "null input"), (dict(out=null), "null output"),
                     (dict(rc_out=null), "null output"), (dict(ag=p, pairs=null), "null contact output"), (dict(ag=p, rct=null), "null contact output"),
                     (dict(ag=p, hs=p, hot=null), "null hotspot output"), (dict(ws=null), "workspace"),
                     (dict(ws=ctypes.c_void_p(4100)), "16-byte aligned")):
        rc = ct(**kw)
        assert rc == -1 and word in err(), (kw, rc, err())
    need = metrics.contacts_workspace_bytes(2, 128, 15)
    assert ct(ws_bytes=need // 2) == -4 and "needed" in err()
    assert need - 2048 <= int(re.search(r"(\d+) needed", err()).group(1)) <= need
    # the outputs of a mask that is not given may be null: such a call passes every argument check and is stopped by the workspace size
    assert ct(pairs=null, rct=null, hot=null, ws_bytes=16) == -4 and "needed" in err()
    assert ct(ag=p, hot=null, ws_bytes=16) == -4 and "needed" in err()
    # empty problems return 0 before any pointer is looked at
    assert l.diffab_metrics_backbone(*[null] * 5, 0, 5, 128, 0.25, *[null] * 8, null, 0, null) == 0
    assert l.diffab_metrics_contacts(*[null] * 10, 0, 5, 128, 5, 15, 3.0, 5.0, *[null] * 10, null, 0, null) == 0


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


def context(G=2, K=16, A=15):
    return {"xyz": torch.zeros(G, K, A, 3), "atom_mask": torch.ones(G, K, A, dtype=torch.bool)}


def test_good_arguments_reach_the_library(no_library):
    with pytest.raises(ReachedTheLibrary):
        metrics.backbone(frames(), mask(), group_size=3, chain_idx=torch.zeros(16, dtype=torch.long), residue_idx=torch.arange(16).expand(2, 16),
                         residue_mask=~mask(), bond_tolerance=0.3)
    with pytest.raises(ReachedTheLibrary):
        metrics.contacts(frames(), mask(), group_size=3, context=context(), antigen_mask=~mask(), hotspot_mask=~mask(), residue_mask=mask(),
                         chain_idx=torch.zeros(2, 16, dtype=torch.int32), atoms=("N", "CA", "C", "O"), clash_distance=2.5, contact_distance=6)
    with pytest.raises(ReachedTheLibrary):
        metrics.contacts(frames(), mask(), group_size=3)


@pytest.mark.parametrize("kw, match", [
    (dict(group_size=4), "6 design rows are not a multiple of group_size = 4"), (dict(group_size=0), "group_size must be"),
    (dict(group_size=True), "group_size must be"), (dict(generation_mask=mask().long()), "generation_mask must be a bool tensor"),
    (dict(generation_mask=mask(3)), "generation_mask is"), (dict(residue_mask=mask(2, 15)), "residue_mask is"),
    (dict(residue_mask=mask().float()), "residue_mask must be a bool tensor"),
    (dict(designs={"seq_idx": torch.zeros(6, 16, dtype=torch.long)}), "designs must be a dict"),
    (dict(designs=dict(frames(), seq_idx=torch.zeros(6, 16))), r"designs\['seq_idx'\] must be an integer tensor"),
    (dict(designs=dict(frames(), translations=torch.zeros(6, 15, 3))), r"designs\['translations'\] is"),
    (dict(designs=dict(frames(), orientations=torch.zeros(6, 16, 3))), r"designs\['orientations'\] must be"),
    (dict(designs={k: v for k, v in frames().items() if k != "orientations"}), r"designs\['orientations'\] must be"),
    (dict(chain_idx=torch.zeros(16)), "integer chain_idx"), (dict(chain_idx=torch.zeros(3, 16, dtype=torch.long)), "chain_idx .* does not broadcast"),
    (dict(residue_idx=torch.zeros(15, dtype=torch.long)), "residue_idx .* does not broadcast"),
    (dict(residue_idx=torch.zeros(16, dtype=torch.bool)), "integer residue_idx"),
    (dict(residue_idx=torch.full((16,), 2 ** 40)), "residue_idx values must fit in int32"),
])
def test_common_argument_errors(no_library, kw, match):
    args = dict(designs=frames(), generation_mask=mask(), group_size=3)
    args.update(kw)
    designs = args.pop("designs")
    gm = args.pop("generation_mask")
    with pytest.raises(ValueError, match=match):
        metrics.backbone(designs, gm, **args)
    with pytest.raises(ValueError, match=match):
        metrics.contacts(designs, gm, **args)


def test_backbone_and_contacts_argument_errors(no_library):
    for bad in (-0.1, float("nan"), float("inf"), "0.25", True):
        with pytest.raises(ValueError, match="bond_tolerance must be"):
            metrics.backbone(frames(), mask(), group_size=3, bond_tolerance=bad)
        with pytest.raises(ValueError, match="clash_distance must be"):
            metrics.contacts(frames(), mask(), group_size=3, clash_distance=bad)
        with pytest.raises(ValueError, match="contact_distance must be"):
            metrics.contacts(frames(), mask(), group_size=3, contact_distance=bad)
    for bad in ("CA", ("N", "CG"), (), ("N", "N"), ("N", "CA", "C", "O", "CB", "CB"), 5):
        with pytest.raises(ValueError, match="atoms must be a sequence of distinct names"):
            metrics.contacts(frames(), mask(), group_size=3, atoms=bad)
    with pytest.raises(ValueError, match="antigen_mask must be a bool tensor"):
        metrics.contacts(frames(), mask(), group_size=3, antigen_mask=mask().long())
    with pytest.raises(ValueError, match="antigen_mask is"):
        metrics.contacts(frames(), mask(), group_size=3, antigen_mask=mask(3))
    with pytest.raises(ValueError, match="hotspot_mask needs an antigen_mask"):
        metrics.contacts(frames(), mask(), group_size=3, hotspot_mask=mask())
    with pytest.raises(ValueError, match="hotspot_mask is"):
        metrics.contacts(frames(), mask(), group_size=3, antigen_mask=mask(), hotspot_mask=mask(2, 15))
    for bad in (torch.zeros(2, 16, 15, 3), {"xyz": torch.zeros(2, 16, 15, 3)}, {"atom_mask": torch.ones(2, 16, 15, dtype=torch.bool)}):
        with pytest.raises(ValueError, match="context must be a dict with xyz"):
            metrics.contacts(frames(), mask(), group_size=3, context=bad)
    with pytest.raises(ValueError, match=r"context\['xyz'\] is"):
        metrics.contacts(frames(), mask(), group_size=3, context=context(3))
    with pytest.raises(ValueError, match=r"context\['xyz'\] is"):
        metrics.contacts(frames(), mask(), group_size=3, context=dict(context(), xyz=torch.zeros(2, 16, 15, 3, dtype=torch.long)))
    with pytest.raises(ValueError, match=r"A = 33 atoms per residue"):
        metrics.contacts(frames(), mask(), group_size=3, context=context(A=33))
    with pytest.raises(ValueError, match=r"context\['atom_mask'\] is"):
        metrics.contacts(frames(), mask(), group_size=3, context=dict(context(), atom_mask=torch.ones(2, 16, 14, dtype=torch.bool)))
    with pytest.raises(ReachedTheLibrary):  # the reference batch's float 0 / 1 atom_mask is a mask too
        metrics.contacts(frames(), mask(), group_size=3, context=dict(context(), atom_mask=torch.ones(2, 16, 15)))
    with pytest.raises(ValueError, match="at most 4096 designs"):
        metrics.backbone(frames(4097, 4), mask(1, 4), group_size=4097)
