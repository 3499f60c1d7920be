"""CPU: the hydrogen-bond entry - the numpy oracle of diffab_metrics_hbonds and its hand cases (an ideal
alpha-helix, two antiparallel strands), the third header against the library and the ctypes table, the workspace macro, host-side refusals
through the C ABI, and every Python argument error before any device work.

The oracle restates the rule of include/diffab_hip_hbonds.h in numpy, brute force over all pairs: derived atoms and energies in float64
from the float32 atoms in the written order and rounded once, the CA cull in float32.  float64 + - * / sqrt are correctly rounded in
numpy as on the device, so tests/test_gpu_hbonds.py asks for equality."""
import ctypes
import inspect
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

from conftest import REPO
from diffab_pytorch import _hip, metrics
from sampler_support import ReachedTheLibrary, refuse_library

HEADER = os.path.join(REPO, "include", "diffab_hip_hbonds.h")
f32, f64 = np.float32, np.float64
RESIDUE_OUTPUTS = ("O", "H", "nh_o_partner", "nh_o_energy", "o_hn_partner", "o_hn_energy", "bridge_partner", "bridge_parallel", "ss",
                   "residue_hbonds")
ROW_OUTPUTS = ("n_hbonds", "n_hbonds_internal", "n_hbonds_antigen", "n_hbonds_framework", "n_hotspot_bonded", "n_hotspot", "hbond_energy",
               "ss_count")
OUTPUTS = RESIDUE_OUTPUTS + ROW_OUTPUTS  # the order of the C prototype
H_, B_, E_, G_, I_, T_, S_ = range(1, 8)


# ------------------------------------------------------------------ the oracle
def links(chain, ridx, inside):
    """succ, pred (K,): the lowest slot with the same chain and residue_idx + 1 / - 1, both inside the mask; -1 without one."""
    K = len(chain)
    succ, pred = np.full(K, -1), np.full(K, -1)
    for k in np.flatnonzero(inside):
        same = inside & (chain == chain[k])
        nxt, prv = np.flatnonzero(same & (ridx.astype(np.int64) == int(ridx[k]) + 1)), np.flatnonzero(same & (ridx.astype(np.int64) == int(ridx[k]) - 1))
        succ[k] = nxt[0] if len(nxt) else -1
        pred[k] = prv[0] if len(prv) else -1
    return succ, pred


def dot(u, v):
    return (u[0] * v[0] + u[1] * v[1]) + u[2] * v[2]


def unit(v):
    n = np.sqrt(dot(v, v))
    return v / n if n > 0 else None


def atoms_of_row(pts, off, ctx, cvalid, coff, gen, inside, succ, pred):
    """N, CA, C, O, H (K,3) float32 and complete, has_o, has_h (K,) of one design row."""
    K = len(gen)
    at = {a: np.zeros((K, 3), f32) for a in "N CA C O H".split()}
    complete, has_o, has_h, real_o = (np.zeros(K, bool) for _ in range(4))
    for k in np.flatnonzero(inside):
        if gen[k]:
            at["N"][k], at["CA"][k], at["C"][k] = pts[k]
            complete[k] = True
        elif (int(cvalid[k]) & 7) == 7:
            at["N"][k], at["CA"][k], at["C"][k] = ctx[k, :3]
            complete[k] = True
            if int(cvalid[k]) & 8:
                at["O"][k] = ctx[k, 3]
                has_o[k] = real_o[k] = True
    for k in np.flatnonzero(complete & ~has_o):
        n, ca, c = (at[a][k].astype(f64) for a in ("N", "CA", "C"))
        s, o = succ[k], None
        if s >= 0 and complete[s]:
            u1, u2 = unit(ca - c), unit(at["N"][s].astype(f64) - c)
            ub = unit(u1 + u2) if u1 is not None and u2 is not None else None
            if ub is not None:
                o = c - 1.231 * ub
        else:
            e1, v = unit(c - ca), n - ca
            e2 = unit(v - dot(v, e1) * e1) if e1 is not None else None
            if e2 is not None:
                o = (ca + 2.153 * e1) - 1.062 * e2
        if o is not None:
            at["O"][k], has_o[k] = o.astype(f32), True
    for k in np.flatnonzero(complete):
        p = pred[k]
        donor_off = off[k] if gen[k] else coff[k]
        if donor_off or p < 0 or not complete[p] or not has_o[p]:
            continue
        u = unit(at["C"][p].astype(f64) - at["O"][p].astype(f64))
        if u is not None:
            at["H"][k], has_h[k] = (at["N"][k].astype(f64) + u).astype(f32), True
    return at, complete, has_o, has_h


def energies(at, acceptor, donor, succ):
    """tested (K,K) bool [a,d], E (K,K) float64 and the float32 CA d2 of every pair."""
    K = len(acceptor)
    ca = at["CA"]
    dx, dy, dz = (ca[:, None, x] - ca[None, :, x] for x in range(3))
    d2 = (dx * dx + dy * dy) + dz * dz
    assert d2.dtype == f32

    def r(p, q):
        d = at[p].astype(f64)[:, None, :] - at[q].astype(f64)[None, :, :]
        return np.maximum(np.sqrt((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]), 0.5)

    E = 27.888 * (((1.0 / r("O", "N") + 1.0 / r("C", "H")) - 1.0 / r("O", "H")) - 1.0 / r("C", "N"))
    idx = np.arange(K)
    pair = acceptor[:, None] & donor[None, :] & (idx[:, None] != idx[None, :]) & (succ[:, None] != idx[None, :])
    return pair & (d2 < f32(81.0)), E, d2, pair


def states(HB, succ, pred, inside, complete, ca):
    """ss (K,) and the bridge partners / types of one row from its bond matrix; the two bridge relations over all pairs at once."""
    K = len(succ)
    idx = np.arange(K)

    def s(k, n=1):
        for _ in range(n):
            k = succ[k] if k >= 0 else -1
        return k

    def hb(a, d):
        return a >= 0 and d >= 0 and bool(HB[a, d])

    pad = np.zeros((K + 1, K + 1), bool)  # index -1 (no such residue) reads False
    pad[:K, :K] = HB
    linked = inside & (succ >= 0) & (pred >= 0)
    s2 = np.array([s(k, 2) for k in range(K)])
    near = (idx[None, :] == idx[:, None]) | (idx[None, :] == succ[:, None]) | (idx[None, :] == s2[:, None])  # j in {i, s(i), s^2(i)}: -1 is no slot
    ok = linked[:, None] & linked[None, :] & ~near & ~near.T
    i_, j_ = idx[:, None], idx[None, :]
    pi, si, pj, sj = pred[:, None], succ[:, None], pred[None, :], succ[None, :]
    par = ok & ((pad[pi, j_] & pad[j_, si]) | (pad[pj, i_] & pad[i_, sj]))
    anti = ok & ((pad[i_, j_] & pad[j_, i_]) | (pad[pi, sj] & pad[pj, si]))
    ppar, panti = np.zeros((K + 1, K + 1), bool), np.zeros((K + 1, K + 1), bool)
    ppar[:K, :K], panti[:K, :K] = par, anti
    ladder = (par & (ppar[si, sj] | ppar[pi, pj])) | (anti & (panti[si, pj] | panti[pi, sj]))

    flag = np.zeros((K, 8), bool)
    turn = {n: [inside[i] and hb(i, s(i, n)) for i in range(K)] for n in (3, 4, 5)}
    partner, parallel = np.full((K, 2), -1, np.int32), np.zeros((K, 2), np.uint8)
    for i in np.flatnonzero(inside):
        p = pred[i]
        if p >= 0 and turn[4][p] and turn[4][i]:
            for m in range(4):
                flag[s(i, m), H_] = True
        for n in (3, 4, 5):
            if turn[n][i]:
                for m in range(1, n):
                    flag[s(i, m), T_] = True
        found = np.flatnonzero(par[i] | anti[i])
        for m, j in enumerate(found[:2]):
            partner[i, m], parallel[i, m] = j, par[i, j]
        if len(found):
            flag[i, E_ if ladder[i].any() else B_] = True
        pp, ss_ = (pred[p] if p >= 0 else -1), s(i, 2)
        if complete[i] and pp >= 0 and ss_ >= 0 and complete[pp] and complete[ss_]:
            u, v = ca[i].astype(f64) - ca[pp].astype(f64), ca[ss_].astype(f64) - ca[i].astype(f64)
            flag[i, S_] = dot(u, v) < 0.3420201433256687 * (np.sqrt(dot(u, u)) * np.sqrt(dot(v, v)))
    for n, mark, higher in ((3, G_, (H_, B_, E_)), (5, I_, (H_, B_, E_, G_))):
        for i in np.flatnonzero(inside):
            p = pred[i]
            if p >= 0 and turn[n][p] and turn[n][i]:
                stretch = [s(i, m) for m in range(n)]
                if not flag[stretch][:, list(higher)].any():
                    flag[stretch, mark] = True
    ss = np.zeros(K, np.uint8)
    for k in np.flatnonzero(inside):
        on = np.flatnonzero(flag[k])
        ss[k] = on[0] if len(on) else 0
    return ss, partner, parallel


def hbonds_ref(points, donor_off, ctx_points, ctx_valid, ctx_donor_off, gen, chain, ridx, rm=None, antigen=None, hotspot=None, group_size=1,
               keep_energy=False):
    """Every output of diffab_metrics_hbonds as numpy arrays of the output's dtype, plus `_margin` (the smallest |E + 0.5| over the
    tested pairs), `_on_cull` (a pair whose CA d2 is exactly 81) and `_bonds` (rows, K, K) for the tests' own guards; with keep_energy
    also `_energy` and `_tested` (rows, K, K)."""
    rows, K = points.shape[:2]
    G = rows // group_size
    rm = np.ones((G, K), bool) if rm is None else rm
    ag = np.zeros((G, K), bool) if antigen is None else antigen
    hs = np.zeros((G, K), bool) if hotspot is None else hotspot
    out = {"O": np.full((rows, K, 3), np.nan, f32), "H": np.full((rows, K, 3), np.nan, f32)}
    for k in ("nh_o_partner", "o_hn_partner", "bridge_partner"):
        out[k] = np.full((rows, K, 2), -1, np.int32)
    out.update(nh_o_energy=np.zeros((rows, K, 2), f32), o_hn_energy=np.zeros((rows, K, 2), f32), bridge_parallel=np.zeros((rows, K, 2), np.uint8),
               ss=np.zeros((rows, K), np.uint8), residue_hbonds=np.zeros((rows, K), np.int32), hbond_energy=np.zeros(rows, f32),
               ss_count=np.zeros((rows, 8), np.int32), _bonds=np.zeros((rows, K, K), bool))
    for k in ROW_OUTPUTS[:6]:
        out[k] = np.zeros(rows, np.int32)
    if keep_energy:
        out.update(_energy=np.zeros((rows, K, K)), _tested=np.zeros((rows, K, K), bool))
    margin, on_cull = np.inf, False
    for g in range(G):
        succ, pred = links(chain[g], ridx[g], rm[g])
        hot = rm[g] & ~gen[g] & ag[g] & hs[g]
        for r in range(g * group_size, (g + 1) * group_size):
            at, complete, has_o, has_h = atoms_of_row(points[r], donor_off[r], ctx_points[g], ctx_valid[g], ctx_donor_off[g], gen[g], rm[g], succ, pred)
            tested, E, d2, pair = energies(at, complete & has_o, complete & has_h, succ)
            HB = tested & (E < -0.5)
            if tested.any():
                margin = min(margin, float(np.abs(E[tested] + 0.5).min()))
            on_cull = on_cull or bool((d2[pair] == f32(81.0)).any())
            out["_bonds"][r] = HB
            if keep_energy:
                out["_energy"][r], out["_tested"][r] = E, tested
            out["O"][r][has_o], out["H"][r][has_h] = at["O"][has_o], at["H"][has_h]
            for k in range(K):
                for name, cand, e in (("o_hn", np.flatnonzero(HB[k]), E[k]), ("nh_o", np.flatnonzero(HB[:, k]), E[:, k])):
                    best = sorted(cand, key=lambda j: (e[j], j))[:2]
                    for m, j in enumerate(best):
                        out[name + "_partner"][r, k, m], out[name + "_energy"][r, k, m] = j, f32(e[j])
            out["ss"][r], out["bridge_partner"][r], out["bridge_parallel"][r] = states(HB, succ, pred, rm[g], complete, at["CA"])
            total, bonded = f64(0.0), set()
            for a, d in zip(*np.nonzero(HB)):  # ascending (acceptor, donor)
                if not (gen[g, a] or gen[g, d]):
                    continue
                total = total + E[a, d]
                out["n_hbonds"][r] += 1
                out["residue_hbonds"][r, a] += 1
                out["residue_hbonds"][r, d] += 1
                if gen[g, a] and gen[g, d]:
                    out["n_hbonds_internal"][r] += 1
                else:
                    other = d if gen[g, a] else a
                    out["n_hbonds_antigen" if ag[g, other] else "n_hbonds_framework"][r] += 1
                    if hot[other]:
                        bonded.add(other)
            out["hbond_energy"][r] = f32(total)
            out["n_hotspot"][r], out["n_hotspot_bonded"][r] = hot.sum(), len(bonded)
            out["ss_count"][r] = np.bincount(out["ss"][r][gen[g] & rm[g]], minlength=8)
    out["_margin"], out["_on_cull"] = margin, on_cull
    return out


# ------------------------------------------------------------------ backbones by NeRF
BOND = {"N-CA": 1.458, "CA-C": 1.525, "C-N": 1.329}
ANGLE = {"N-CA-C": 111.0, "CA-C-N": 116.2, "C-N-CA": 121.7}


def place(a, b, c, length, angle, torsion):
    """The point d with |d - c| = length, angle b-c-d and dihedral a-b-c-d (degrees)."""
    angle, torsion = np.radians(angle), np.radians(torsion)
    bc = (c - b) / np.linalg.norm(c - b)
    n = np.cross(b - a, bc)
    n /= np.linalg.norm(n)
    m = np.cross(n, bc)
    d = np.array([-length * np.cos(angle), length * np.sin(angle) * np.cos(torsion), length * np.sin(angle) * np.sin(torsion)])
    return c + d[0] * bc + d[1] * m + d[2] * n


def backbone(n, phi, psi, omega=180.0):
    """(n,3,3) float64 N, CA, C of a chain with the same phi, psi at every residue."""
    N = np.array([0.0, 0.0, 0.0])
    CA = np.array([BOND["N-CA"], 0.0, 0.0])
    a = np.radians(ANGLE["N-CA-C"])
    C = CA + BOND["CA-C"] * np.array([-np.cos(a), np.sin(a), 0.0])
    out = [[N, CA, C]]
    for _ in range(n - 1):
        N2 = place(N, CA, C, BOND["C-N"], ANGLE["CA-C-N"], psi)
        CA2 = place(CA, C, N2, BOND["N-CA"], ANGLE["C-N-CA"], omega)
        C2 = place(C, N2, CA2, BOND["CA-C"], ANGLE["N-CA-C"], phi)
        N, CA, C = N2, CA2, C2
        out.append([N, CA, C])
    return np.array(out)


def helix(n=12):
    return backbone(n, -57.0, -47.0)


def rotation(axis, angle):
    axis = axis / np.linalg.norm(axis)
    Kx = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    return np.eye(3) + np.sin(angle) * Kx + (1 - np.cos(angle)) * Kx @ Kx


STRAND_OFF, STRAND_ALONG = 5.0, -1.5  # chosen with the oracle: test_the_strand_placement_is_clear_of_the_threshold


def strands(n=7, off=STRAND_OFF, along=STRAND_ALONG):
    """(2n,3,3): a beta strand (phi -120, psi 130) and its antiparallel partner: the first turned by pi about the in-sheet axis
    perpendicular to it and by pi about its own axis, moved `off` across and `along` along.  The in-sheet direction is the one the
    carbonyls of the odd residues point along."""
    one = backbone(n, -120.0, 130.0)
    centre = one[:, 1].mean(0)
    one = one - centre
    axis = one[-1, 1] - one[0, 1]
    axis /= np.linalg.norm(axis)
    nxt = one[2, 0]  # C=O of residue 1 is, up to the bisector, opposite to where N of residue 2 and CA of 1 lie
    co = -((one[1, 1] - one[1, 2]) / np.linalg.norm(one[1, 1] - one[1, 2]) + (nxt - one[1, 2]) / np.linalg.norm(nxt - one[1, 2]))
    side = co - (co @ axis) * axis
    side /= np.linalg.norm(side)
    R = rotation(axis, np.pi) @ rotation(side, np.pi)
    two = one.reshape(-1, 3) @ R.T + off * side + along * axis
    return np.concatenate([one, two.reshape(n, 3, 3)])


def single_patch(pts, chain=None, off=None):
    """One patch, one design, every residue generated, no context atoms."""
    K = len(pts)
    chain = np.zeros(K, np.int32) if chain is None else np.asarray(chain, np.int32)
    ridx = np.arange(K, dtype=np.int32)
    off = np.zeros(K, bool) if off is None else off
    return dict(points=pts.astype(f32)[None], donor_off=off[None], ctx_points=np.zeros((1, K, 4, 3), f32), ctx_valid=np.zeros((1, K), np.int64),
                ctx_donor_off=np.zeros((1, K), bool), gen=np.ones((1, K), bool), chain=chain[None], ridx=ridx[None])


def test_the_bisector_oxygen_of_an_ideal_chain():
    """|C - O| = 1.231 and CA-C-O = 121.9 degrees on the NeRF chain (its CA-C-N is 116.2: the two angles at C besides it share 243.8)."""
    ref = hbonds_ref(**single_patch(helix()))
    pts = helix()
    for k in range(11):
        o, ca, c = ref["O"][0, k].astype(f64), pts[k, 1], pts[k, 2]
        assert abs(np.linalg.norm(o - c) - 1.231) < 1e-5
        cos = (o - c) @ (ca - c) / (np.linalg.norm(o - c) * np.linalg.norm(ca - c))
        assert abs(np.degrees(np.arccos(cos)) - 121.9) < 0.01
    # the last residue has no successor: the ideal placement, in the N-CA-C plane at 1.23 A
    o, n, ca, c = ref["O"][0, 11].astype(f64), *pts[11]
    assert abs(np.linalg.norm(o - c) - 1.2335) < 1e-3 and abs(np.linalg.det(np.stack([o - ca, n - ca, c - ca]))) < 1e-4
    assert np.isnan(ref["H"][0, 0]).all() and not np.isnan(ref["H"][0, 1:]).any()
    assert np.allclose(np.linalg.norm(ref["H"][0, 1:].astype(f64) - pts[1:, 0], axis=-1), 1.0, atol=1e-6)


def test_an_ideal_helix_has_its_eight_i_to_i_plus_4_bonds():
    ref = hbonds_ref(**single_patch(helix()))
    assert sorted(zip(*map(list, np.nonzero(ref["_bonds"][0])))) == [(i, i + 4) for i in range(8)]
    e = ref["o_hn_energy"][0, :8, 0]
    print("helix energies", e, "margin", ref["_margin"])
    assert (np.abs(e + 2.3) < 0.4).all() and ref["_margin"] > 0.1
    assert ref["n_hbonds"].tolist() == [8] and ref["n_hbonds_internal"].tolist() == [8] and ref["n_hbonds_framework"].tolist() == [0]
    assert ref["o_hn_partner"][0, :, 0].tolist() == [4, 5, 6, 7, 8, 9, 10, 11, -1, -1, -1, -1] and (ref["o_hn_partner"][0, :, 1] == -1).all()
    assert ref["nh_o_partner"][0, :, 0].tolist() == [-1] * 4 + list(range(8))
    assert metrics.SS_LETTERS[1] == "H" and "".join(metrics.SS_LETTERS[c] for c in ref["ss"][0]) == " HHHHHHHHHH "
    assert ref["residue_hbonds"][0].tolist() == [1] * 4 + [2] * 4 + [1] * 4 and ref["ss_count"][0].tolist() == [2, 10, 0, 0, 0, 0, 0, 0]
    total = f64(0.0)
    for i in range(8):
        total = total + _energy_of(ref, helix(), i, i + 4)
    assert ref["hbond_energy"][0] == f32(total)


def _energy_of(ref, pts, a, d):
    """E of one pair from the oracle's own atoms, written out once more."""
    o, c, n, h = ref["O"][0, a].astype(f64), pts.astype(f32)[a, 2].astype(f64), pts.astype(f32)[d, 0].astype(f64), ref["H"][0, d].astype(f64)
    r = lambda p, q: max(np.sqrt(((p - q)[0] ** 2 + (p - q)[1] ** 2) + (p - q)[2] ** 2), 0.5)
    return 27.888 * (((1.0 / r(o, n) + 1.0 / r(c, h)) - 1.0 / r(o, h)) - 1.0 / r(c, n))


def test_a_proline_removes_exactly_its_own_donor():
    off = np.zeros(12, bool)
    off[6] = True
    ref = hbonds_ref(**single_patch(helix(), off=off))
    assert sorted(zip(*map(list, np.nonzero(ref["_bonds"][0])))) == [(i, i + 4) for i in range(8) if i != 2]
    assert np.isnan(ref["H"][0, 6]).all() and ref["nh_o_partner"][0, 6].tolist() == [-1, -1] and ref["n_hbonds"].tolist() == [7]
    # turn_4(2) is gone and with it the seeds at 2 and 3; the seeds at 1 (H on 1..4) and 4 (H on 4..7) still meet
    assert "".join(metrics.SS_LETTERS[c] for c in ref["ss"][0]) == " HHHHHHHHHH "


def strand_case(off=None, along=None, n=7):
    return single_patch(strands(n, STRAND_OFF if off is None else off, STRAND_ALONG if along is None else along), chain=[0] * n + [1] * n)


def strand_report(ref, n=7):
    """The bonds of the two-strand case, and how far the energies of its tested pairs stay from -0.5: between the strands, and within one."""
    bonds = sorted((int(a), int(d)) for a, d in zip(*np.nonzero(ref["_bonds"][0])))
    idx = np.arange(2 * n)
    across = (idx[:, None] < n) != (idx[None, :] < n)
    gap = np.abs(ref["_energy"][0] + 0.5)
    return bonds, float(gap[ref["_tested"][0] & across].min()), float(gap[ref["_tested"][0] & ~across].min())


LADDER = [(1, 12), (3, 10), (8, 5), (10, 3)]


def test_two_antiparallel_strands_form_a_ladder():
    """phi -120, psi 130, 7 residues each, the second strand 5.0 A across and -1.5 A along.  With this chain geometry the placement
    gives four bonds between the strands - 3 and 10 bonded both ways, C=O of 1 to N-H of 12, C=O of 8 to N-H of 5 (no placement on the
    grid of the next test gives six) - every energy between the strands at least 0.3 from -0.5.  Inside a strand the rule's only
    near miss is C=O(i) to N-H(i+2) at -0.454: it is fixed by phi, psi and the bond angles, not by the placement, and is 0.046 from
    the threshold - 4e7 times the 1e-9 the exactness guard of the GPU tests asks for."""
    n = 7
    ref = hbonds_ref(**strand_case(), keep_energy=True)
    bonds, across, within = strand_report(ref)
    print("strand bonds", bonds, "margins", across, within)
    assert bonds == sorted(LADDER) and across >= 0.1 and abs(within - 0.046) < 0.001
    assert ref["n_hbonds"].tolist() == [4] and ref["residue_hbonds"][0].tolist() == [0, 1, 0, 2, 0, 1, 0, 0, 1, 0, 2, 0, 1, 0]
    ss = metrics.SS_LETTERS
    assert "".join(ss[c] for c in ref["ss"][0]) == "  EEE    EEE  "
    # 3 and 10 by their two bonds; 2 / 11 and 4 / 9 by the bonds of their neighbours (the second antiparallel pattern)
    assert ref["bridge_partner"][0, 2:5].tolist() == [[11, -1], [10, -1], [9, -1]] and ref["bridge_partner"][0, 9:12].tolist() == [[4, -1], [3, -1], [2, -1]]
    assert not ref["bridge_parallel"].any() and ref["ss_count"][0].tolist() == [8, 0, 0, 6, 0, 0, 0, 0]
    assert ref["nh_o_partner"][0, 10].tolist() == [3, -1] and ref["o_hn_partner"][0, 10].tolist() == [3, -1]


def test_the_strand_placement_is_clear_of_the_threshold():
    """How STRAND_OFF / STRAND_ALONG were chosen: among the placements of a grid that give the ladder, one whose energies between
    the strands - bonds and near misses - are all at least 0.1 from -0.5 (the committed one: 0.33)."""
    good = {}
    for off in (4.6, 5.0, 5.4):
        for along in (-2.5, -1.5, 0.0, 1.0):
            bonds, across, _ = strand_report(hbonds_ref(**strand_case(off, along), keep_energy=True))
            print(off, along, len(bonds), round(across, 3))
            assert len([b for b in bonds if (b[0] < 7) != (b[1] < 7)]) < 6
            if bonds == sorted(LADDER):
                good[off, along] = across
    assert good[STRAND_OFF, STRAND_ALONG] >= 0.3


def test_a_lone_bridge_is_B_and_a_bend_is_S():
    """The two one-way bonds of the ladder lose their donors (Pro at 5 and 12): 3 and 10 stay bonded both ways with no bridged neighbour."""
    case = strand_case()
    off = np.zeros(14, bool)
    off[[5, 12]] = True
    case["donor_off"] = off[None]
    ref = hbonds_ref(**case)
    assert sorted(zip(*map(list, np.nonzero(ref["_bonds"][0])))) == [(3, 10), (10, 3)]
    assert "".join(metrics.SS_LETTERS[c] for c in ref["ss"][0]) == "   B      B   "  # (an extended strand does not bend by 70 degrees)
    hel = hbonds_ref(**single_patch(helix(), off=np.ones(12, bool)))  # no H at all: no bonds, only the CA trace
    assert "".join(metrics.SS_LETTERS[c] for c in hel["ss"][0]) == "  SSSSSSSS  "


# ------------------------------------------------------------------ the header, the library and the ctypes table
def header_code():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


def test_header_library_and_symbol_table_agree():
    declared = sorted(set(re.findall(r"\b(diffab_[a-z0-9_]+)\s*\(", header_code())))
    assert declared == ["diffab_metrics_hbonds"]
    assert sorted(_hip.HBOND_SYMBOLS) == declared, "HBOND_SYMBOLS and include/diffab_hip_hbonds.h drifted apart"
    assert not set(_hip.HBOND_SYMBOLS) & (set(_hip.SYMBOLS) | set(_hip.ANALYSIS_SYMBOLS))
    raw = ctypes.CDLL(_hip.LIB_PATH)
    typed = _hip.load_library()
    assert hasattr(raw, "diffab_metrics_hbonds"), "declared in include/diffab_hip_hbonds.h but not exported by libdiffab_hip.so"
    res, args = _hip.HBOND_SYMBOLS["diffab_metrics_hbonds"]
    fn = typed.diffab_metrics_hbonds
    assert fn.restype is res and list(fn.argtypes) == args  # load_library() types the third table onto the same CDLL object
    proto = re.search(r"\bint\s+diffab_metrics_hbonds\s*\((.*?)\)\s*;", header_code(), flags=re.S).group(1)
    params = [p.strip() for p in proto.split(",")]
    assert res is ctypes.c_int and len(args) == len(params) == 36
    for p, a in zip(params, args):
        kind = p.rsplit(" ", 1)[0]
        want = {"int32_t": ctypes.c_int32, "size_t": ctypes.c_size_t}.get(kind)
        if want is None:
            assert "*" in kind and a is ctypes.c_void_p, p
        else:
            assert a is want, p
    names = [p.rsplit(" ", 1)[1].lstrip("*") for p in params]
    assert names[15:33] == list(OUTPUTS)
    text = open(HEADER).read()
    assert '#include "diffab_hip.h"' in text and "Why a header of its own" in text.split("*/")[0] and "No bulge linking" in text
    assert int(re.search(r"#define\s+DIFFAB_HBONDS_MAX_K\s+(\d+)", header_code()).group(1)) == metrics.HBONDS_MAX_K == 512


SHAPES = [(1, 1, 4), (3, 24, 4), (1, 40, 15), (2, 96, 32), (3, 130, 15), (16, 128, 15), (256, 128, 4), (1, 512, 32), (7, 31, 5), (5, 33, 4)]
MACRO_C = r"""
#include <stdio.h>
#include "diffab_hip_hbonds.h"
int main(void) {
%s
  printf("%%d %%d %%d\n", DIFFAB_ERR_ARG, DIFFAB_HBONDS_MAX_K, DIFFAB_METRICS_MAX_CONTEXT_ATOMS);
  return 0;
}
"""


def test_workspace_macro_equals_the_python_mirror(tmp_path):
    """The header compiles as C on its own (it brings diffab_hip.h along) and its macro gives metrics.hbonds_workspace_bytes."""
    cc = shutil.which("cc") or shutil.which("gcc") or next((p for p in ("/opt/rocm/llvm/bin/clang",) if os.path.exists(p)), None)
    assert cc, "no C compiler to read the header's macro with"
    src, exe = tmp_path / "macro.c", tmp_path / "macro"
    lines = "\n".join(f'  printf("%zu\\n", DIFFAB_METRICS_HBONDS_WORKSPACE_BYTES({G}, {K}, {A}));' for G, K, A in SHAPES)
    src.write_text(MACRO_C % lines)
    subprocess.run([cc, "-I", os.path.join(REPO, "include"), str(src), "-o", str(exe)], check=True)
    got = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()
    assert [int(v) for v in got[:len(SHAPES)]] == [metrics.hbonds_workspace_bytes(*s) for s in SHAPES]
    assert got[len(SHAPES):] == ["-1", "512", str(metrics.MAX_CONTEXT_ATOMS)]


def test_host_side_refusals_touch_no_gpu():
    """Every refusal is decided from the scalar arguments and whether a pointer is null: the device pointers are fake addresses that
    are never dereferenced, nothing is enqueued (no GPU is needed), and diffab_last_error names the problem."""
    l = _hip.load_library()
    p, null = ctypes.c_void_p(4096), ctypes.c_void_p(0)
    inputs = ("pts", "off", "ctx", "cvalid", "coff", "gen", "rm", "ag", "hs", "chain", "ridx")

    def err():
        return l.diffab_last_error().decode()

    def call(rows=10, group=5, K=128, A=15, outs=None, ws=p, ws_bytes=1 << 40, **ptrs):
        given = dict(dict.fromkeys(inputs, p), rm=null, ag=null, hs=null)
        given.update(ptrs)
        outs = [p] * 18 if outs is None else outs
        return l.diffab_metrics_hbonds(*[given[k] for k in inputs], rows, group, K, A, *outs, ws, ws_bytes, null)

    for kw, word in ((dict(rows=11), "not a multiple"), (dict(rows=-5), "extent"), (dict(group=0), "extent"), (dict(K=0), "extent"),
                     (dict(group=4097, rows=4097), "at most 4096 designs"), (dict(K=513), "at most 512"), (dict(K=4096), "at most 512"),
                     (dict(A=3), "context atoms per residue outside [4, 32]"), (dict(A=0), "context atoms per residue"),
                     (dict(A=33), "context atoms per residue"), (dict(hs=p), "needs an antigen_mask"), (dict(pts=null), "null input"),
                     (dict(off=null), "null input"), (dict(ctx=null), "null input"), (dict(cvalid=null), "null input"),
                     (dict(coff=null), "null input"), (dict(gen=null), "null input"), (dict(chain=null), "null input"),
                     (dict(ridx=null), "null input"), (dict(ws=null), "workspace"), (dict(ws=ctypes.c_void_p(4096 + 16)), "256-byte aligned")):
        rc = call(**kw)
        assert rc == -1 and word in err() and err().startswith("metrics_hbonds:"), (kw, rc, err())
    need = metrics.hbonds_workspace_bytes(2, 128, 15)
    assert call(ws_bytes=need // 2) == -4 and "needed" in err()  # DIFFAB_ERR_WORKSPACE
    assert need - 1024 <= int(re.search(r"(\d+) needed", err()).group(1)) <= need
    # the limits themselves pass every argument check (the call is stopped by the workspace size, still on the host); so do the
    # optional operands and every output left out
    for kw in (dict(K=512), dict(K=1), dict(A=4), dict(A=32), dict(rm=p, ag=p, hs=p), dict(ag=p), dict(outs=[null] * 18),
               dict(group=4096, rows=4096)):
        assert call(ws_bytes=16, **kw) == -4 and "needed" in err(), kw
    # an empty problem returns 0 before any pointer is looked at
    assert l.diffab_metrics_hbonds(*[null] * 11, 0, 5, 128, 15, *[null] * 18, null, 0, null) == 0


# ------------------------------------------------------------------ Python argument errors before any device work
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
        metrics.hbonds(frames(), mask(), group_size=3)
    with pytest.raises(ReachedTheLibrary):
        metrics.hbonds(frames(), mask(), group_size=3, context=context(A=4), antigen_mask=~mask(), hotspot_mask=~mask(), residue_mask=mask(),
                       chain_idx=torch.zeros(16, dtype=torch.long), residue_idx=torch.arange(16).expand(2, 16))
    with pytest.raises(ReachedTheLibrary):
        metrics.hbonds(frames(2, 512), mask(2, 512), context=context(2, 512, 32))


@pytest.mark.parametrize("kw, match", [
    (dict(group_size=4), "6 design rows are not a multiple of group_size = 4"), (dict(group_size=0), "group_size must be"),
    (dict(group_size=True), "group_size must be"), (dict(generation_mask=mask().long()), "generation_mask must be a bool tensor"),
    (dict(generation_mask=mask(3)), "generation_mask is"), (dict(residue_mask=mask(2, 15)), "residue_mask is"),
    (dict(residue_mask=mask().float()), "residue_mask must be a bool tensor"),
    (dict(designs={"seq_idx": torch.zeros(6, 16, dtype=torch.long)}), "designs must be a dict"),
    (dict(designs=dict(frames(), seq_idx=torch.zeros(6, 16))), r"designs\['seq_idx'\] must be an integer tensor"),
    (dict(designs=dict(frames(), translations=torch.zeros(6, 15, 3))), r"designs\['translations'\] is"),
    (dict(designs={k: v for k, v in frames().items() if k != "orientations"}), r"designs\['orientations'\] must be"),
    (dict(designs=frames(6, 513), generation_mask=mask(2, 513)), "K = 513 residues per patch, at most 512"),
    (dict(antigen_mask=mask().long()), "antigen_mask must be a bool tensor"), (dict(antigen_mask=mask(3)), "antigen_mask is"),
    (dict(hotspot_mask=mask()), "hotspot_mask needs an antigen_mask"), (dict(antigen_mask=mask(), hotspot_mask=mask(2, 15)), "hotspot_mask is"),
    (dict(context=torch.zeros(2, 16, 15, 3)), "context must be a dict with xyz"), (dict(context={"xyz": torch.zeros(2, 16, 15, 3)}), "context must be a dict"),
    (dict(context=context(3)), r"context\['xyz'\] is"), (dict(context=context(A=33)), "A = 33 atoms per residue"),
    (dict(context=context(A=3)), r"A = 3 atoms per residue, N, CA, C, O \(at least 4\) are needed"),
    (dict(context=dict(context(), atom_mask=torch.ones(2, 16, 14, dtype=torch.bool))), r"context\['atom_mask'\] is"),
    (dict(chain_idx=torch.zeros(16)), "needs an integer chain_idx"), (dict(residue_idx=torch.zeros(3, 16, dtype=torch.long)), "residue_idx .* does not broadcast"),
    (dict(residue_idx=torch.zeros(2, 2, 16, dtype=torch.long)), r"residue_idx must be \(K,\) or \(rows, K\)"),
])
def test_argument_errors(no_library, kw, match):
    args = dict(designs=frames(), generation_mask=mask(), group_size=3)
    args.update(kw)
    designs, gm = args.pop("designs"), args.pop("generation_mask")
    with pytest.raises(ValueError, match=match):
        metrics.hbonds(designs, gm, **args)


def test_signature_letters_and_strings():
    sig = inspect.signature(metrics.hbonds)
    assert list(sig.parameters) == ["designs", "generation_mask", "context", "antigen_mask", "hotspot_mask", "chain_idx", "residue_idx",
                                    "residue_mask", "group_size"]
    assert all(sig.parameters[k].kind is inspect.Parameter.KEYWORD_ONLY for k in list(sig.parameters)[2:])
    assert sig.parameters["group_size"].default == 1 and all(sig.parameters[k].default is None for k in list(sig.parameters)[2:8])
    assert metrics.SS_LETTERS == " HBEGITS"
    assert metrics.ss_strings(torch.tensor([[0, 1, 1, 6, 7], [3, 3, 2, 4, 5]], dtype=torch.uint8)) == [" HHTS", "EEBGI"]
    assert metrics.ss_strings(torch.tensor([1, 0, 3])) == ["H E"]
    for bad in (torch.tensor([[8]]), torch.tensor([[-1]]), torch.tensor([[0.0]]), [[0]], torch.zeros(1, 1, 1, dtype=torch.long)):
        with pytest.raises(ValueError, match="ss_strings"):
            metrics.ss_strings(bad)
