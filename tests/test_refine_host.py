"""CPU: the host side of the backbone refinement (diffab_pytorch.refine) - the numpy restatement of the rule,
runnable in float64 (the oracle) and in float32 (the rule's own rounding sensitivity), its hand-checkable cases, the behaviour the issue
rests on (monotone energy, closed bonds), the C-ABI entry with its host-side refusals and the argument checks made before any library
call.

The rule is the header comment of diffab_refine_backbone in include/diffab_hip.h.  refine_ref writes every expression in the order the
header gives, so in float32 each operation rounds as the kernel's does (numpy rounds every elementwise operation once);
test_gpu_refine.py imports it from here."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from diffab_pytorch import _hip, io as dio, refine
from sampler_support import ReachedTheLibrary, refuse_library
from test_cabi_and_host import header_struct
from test_geometry_host import L_N_CA, PEPTIDE, backbone_ref, frames_of, neighbours, nerf_chain

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
L_CA_C = 1.526
BOND = 1.329
CA_N = float(np.sqrt(L_CA_C ** 2 + PEPTIDE ** 2 - 2 * L_CA_C * PEPTIDE * np.cos(np.deg2rad(116.2))))
C_CA = float(np.sqrt(PEPTIDE ** 2 + L_N_CA ** 2 - 2 * PEPTIDE * L_N_CA * np.cos(np.deg2rad(121.7))))
CA_CA = 3.8
INERTIA = 4.45
TINY = 1e-6
LOCAL_N, LOCAL_C = dio.IDEAL_BACKBONE["N"], dio.IDEAL_BACKBONE["C"]


# ------------------------------------------------------------------ the oracle (shared with test_gpu_refine.py)
def norm(v):
    x, y, z = v[..., 0], v[..., 1], v[..., 2]
    return np.sqrt((x * x + y * y) + z * z)


def place(t, O, dt):
    """N and C of frames (…,3), (…,3,3): t + (-0.525 O0 + 1.363 O1) and t + 1.526 O0."""
    return t + (dt(LOCAL_N[0]) * O[..., 0, :] + dt(LOCAL_N[1]) * O[..., 1, :]), t + dt(LOCAL_C[0]) * O[..., 0, :]


def pair_force(a, b, d0, w, valid, dt):
    r = a - b
    d = norm(r)
    with np.errstate(divide="ignore", invalid="ignore"):
        coef = ((dt(-2.0) * w) * (d - d0)) / d
    return np.where(valid & ~(d < dt(TINY)), coef, dt(0.0))[..., None] * r


def pair_energy(a, b, d0, w):
    e = norm(a - b) - d0
    return w * (e * e)


def gram_schmidt(O):
    e1 = O[..., 0, :] / norm(O[..., 0, :])[..., None]
    r1 = O[..., 1, :]
    dot = (e1[..., 0] * r1[..., 0] + e1[..., 1] * r1[..., 1]) + e1[..., 2] * r1[..., 2]
    u2 = r1 - dot[..., None] * e1
    e2 = u2 / norm(u2)[..., None]
    return np.stack([e1, e2, np.cross(e1, e2)], axis=-2)


class Patch:
    """The tables of one patch: masks, links and the clash pairs."""

    def __init__(self, gen, rm, chain, ridx):
        K = len(gen)
        self.K, self.inside, self.moving = K, np.asarray(rm, bool), np.asarray(gen, bool) & np.asarray(rm, bool)
        self.succ, self.pred = neighbours(chain, ridx, self.inside)
        self.has_s, self.has_p = self.succ >= 0, self.pred >= 0
        gap = np.asarray(ridx, np.int64)[:, None] - np.asarray(ridx, np.int64)[None, :]
        bonded = (np.asarray(chain)[:, None] == np.asarray(chain)[None, :]) & (np.abs(gap) == 1)
        self.partner = self.inside[:, None] & self.inside[None, :] & ~bonded & ~np.eye(K, dtype=bool)  # (k, j): j can push k
        self.counted_link = self.has_s & (self.moving | self.moving[self.succ])  # (succ = -1 reads the last slot: masked by has_s)
        upper = np.triu(np.ones((K, K), bool), 1)
        self.counted_pair = self.partner & upper & (self.moving[:, None] | self.moving[None, :])


def energy_terms(p, ca, n, c, start, o, dt):
    """(N,5) float64: bond, angle, trans, clash, tether - every term in dt, the sums in float64."""
    s = p.succ
    link = p.counted_link[None, :]
    f = lambda v: np.asarray(v, np.float64)
    bond = np.where(link, f(pair_energy(c, n[:, s], dt(BOND), dt(o.bond))), 0.0).sum(1)
    angle = np.where(link, f(pair_energy(ca, n[:, s], dt(CA_N), dt(o.angle))), 0.0).sum(1) + \
        np.where(link, f(pair_energy(c, ca[:, s], dt(C_CA), dt(o.angle))), 0.0).sum(1)
    trans = np.where(link, f(pair_energy(ca, ca[:, s], dt(CA_CA), dt(o.trans))), 0.0).sum(1)
    d = norm(ca[:, :, None, :] - ca[:, None, :, :])
    gap = dt(o.clash_distance) - d
    clash = np.where(p.counted_pair[None] & (d < dt(o.clash_distance)), f(dt(o.clash) * (gap * gap)), 0.0).sum((1, 2))
    r = ca - start
    tether = np.where(p.moving[None, :], f(dt(o.tether) * ((r[..., 0] * r[..., 0] + r[..., 1] * r[..., 1]) + r[..., 2] * r[..., 2])), 0.0).sum(1)
    return np.stack([bond, angle, trans, clash, tether], axis=1)


def clash_push(p, ca, o, dt):
    """(N,K,3): the clash force on every moving residue (0 elsewhere), four partial sums over j = l, l + 4, ... ascending, combined
    (0 + 1) + (2 + 3)."""
    N, K = ca.shape[:2]
    own = np.flatnonzero(p.moving)
    r = ca[:, own, None, :] - ca[:, None, :, :]
    d = norm(r)
    with np.errstate(divide="ignore", invalid="ignore"):
        coef = ((dt(2.0) * dt(o.clash)) * (dt(o.clash_distance) - d)) / d
    coef = np.where(p.partner[None, own] & (d < dt(o.clash_distance)) & ~(d < dt(TINY)), coef, dt(0.0))
    f = coef[..., None] * r
    Kp = (K + 3) // 4 * 4
    f = np.concatenate([f, np.zeros((N, len(own), Kp - K, 3), dt)], axis=2).reshape(N, len(own), Kp // 4, 4, 3)
    part = np.zeros((N, len(own), 4, 3), dt)
    for q in range(Kp // 4):
        part = part + f[:, :, q]
    out = np.zeros((N, K, 3), dt)
    out[:, own] = (part[:, :, 0] + part[:, :, 1]) + (part[:, :, 2] + part[:, :, 3])
    return out


def rodrigues(w, dt):
    """(…,3) -> (…,3,3) Exp(w) = I + a hat(w) + b (w w^T - |w|^2 I)."""
    x, y, z = w[..., 0], w[..., 1], w[..., 2]
    n2 = (x * x + y * y) + z * z
    nn = np.sqrt(n2)
    small = nn < dt(TINY)
    with np.errstate(divide="ignore", invalid="ignore"):
        a = np.where(small, dt(1.0), np.sin(nn) / nn)
        b = np.where(small, dt(0.5), (dt(1.0) - np.cos(nn)) / n2)
    one = dt(1.0)
    rows = [[one + b * (x * x - n2), a * -z + b * (x * y), a * y + b * (x * z)],
            [a * z + b * (y * x), one + b * (y * y - n2), a * -x + b * (y * z)],
            [a * -y + b * (z * x), a * x + b * (z * y), one + b * (z * z - n2)]]
    return np.stack([np.stack(r, axis=-1) for r in rows], axis=-2)


def refine_ref(t, R, gen, rm, chain, ridx, options=None, dtype=np.float64, group_size=1, trace=False):
    """The rule of diffab_refine_backbone in numpy, every operation in `dtype`.  t (rows,K,3), R (rows,K,3,3); gen, rm, chain, ridx
    (G,K) with rows = G * group_size.  -> dict: translations, orientations (dtype), energy_before, energy_after, max_shift (rows,),
    terms (rows,5) - energies as float64 sums of the dtype terms - and with `trace` the energy after every iteration (iterations, rows),
    of the state before the final orthonormalisation."""
    o = refine.Refinement() if options is None else options
    dt = np.dtype(dtype).type
    t0, R0 = np.array(t, dtype), np.array(R, dtype)
    rows, K = t0.shape[:2]
    out = dict(translations=t0.copy(), orientations=R0.copy(), energy_before=np.zeros(rows), energy_after=np.zeros(rows),
               terms=np.zeros((rows, 5)), max_shift=np.zeros(rows), trace=np.zeros((o.iterations, rows)))
    step, rot_step = dt(o.step), dt(o.step) / dt(INERTIA)
    for g in range(len(gen)):
        sl = slice(g * group_size, (g + 1) * group_size)
        p = Patch(gen[g], rm[g], chain[g], ridx[g])
        mv, s, q = p.moving, p.succ, p.pred
        hs, hp = p.has_s[None, :], p.has_p[None, :]
        ca, O = t0[sl].copy(), R0[sl].copy()
        start = ca.copy()
        n, c = place(ca, O, dt)
        out["energy_before"][sl] = energy_terms(p, ca, n, c, start, o, dt).sum(1)
        turned = np.zeros(ca.shape[:2], bool)
        for it in range(o.iterations if mv.any() else 0):
            f_c = pair_force(c, n[:, s], dt(BOND), dt(o.bond), hs, dt)
            f_ca = pair_force(ca, n[:, s], dt(CA_N), dt(o.angle), hs, dt)
            f_c = f_c + pair_force(c, ca[:, s], dt(C_CA), dt(o.angle), hs, dt)
            f_ca = f_ca + pair_force(ca, ca[:, s], dt(CA_CA), dt(o.trans), hs, dt)
            f_n = pair_force(n, c[:, q], dt(BOND), dt(o.bond), hp, dt)
            f_n = f_n + pair_force(n, ca[:, q], dt(CA_N), dt(o.angle), hp, dt)
            f_ca = f_ca + pair_force(ca, c[:, q], dt(C_CA), dt(o.angle), hp, dt)
            f_ca = f_ca + pair_force(ca, ca[:, q], dt(CA_CA), dt(o.trans), hp, dt)
            if o.clash != 0:
                f_ca = f_ca + clash_push(p, ca, o, dt)
            if o.tether != 0:
                f_ca = f_ca + (dt(-2.0) * dt(o.tether)) * (ca - start)
            F = (f_n + f_ca) + f_c
            torque = np.cross(n - ca, f_n) + np.cross(c - ca, f_c)
            w = rot_step * torque
            move = mv[None, :] & (F != 0).any(-1)
            turn = mv[None, :] & (w != 0).any(-1)
            ca = np.where(move[..., None], ca + step * F, ca)
            E = rodrigues(w, dt)  # O' = O E^T: O'[i][j] = (O[i][0] E[j][0] + O[i][1] E[j][1]) + O[i][2] E[j][2]
            turned_O = (O[..., :, None, 0] * E[..., None, :, 0] + O[..., :, None, 1] * E[..., None, :, 1]) + O[..., :, None, 2] * E[..., None, :, 2]
            O = np.where(turn[..., None, None], turned_O, O)
            turned |= turn
            n_new, c_new = place(ca, O, dt)
            n, c = np.where(mv[None, :, None], n_new, n), np.where(mv[None, :, None], c_new, c)
            if trace:
                out["trace"][it, sl] = energy_terms(p, ca, n, c, start, o, dt).sum(1)
        if turned.any():
            O = np.where(turned[..., None, None], gram_schmidt(np.where(turned[..., None, None], O, np.eye(3, dtype=dtype))), O)
            n_new, c_new = place(ca, O, dt)
            n, c = np.where(turned[..., None], n_new, n), np.where(turned[..., None], c_new, c)
        terms = energy_terms(p, ca, n, c, start, o, dt)
        out["terms"][sl], out["energy_after"][sl] = terms, terms.sum(1)
        out["max_shift"][sl] = np.where(mv[None, :], norm(ca - start), dt(0.0)).max(1, initial=0.0)
        out["translations"][sl], out["orientations"][sl] = ca, O
    if not trace:
        del out["trace"]
    return out


# ------------------------------------------------------------------ chains to refine
def rotvec_matrix(v):
    return rodrigues(np.asarray(v, np.float64), np.float64)


def noisy(rng, t, R, moving, sigma, angle):
    """Translations + N(0, sigma) and a rotation by N(0, angle) per axis (a rotation vector) on the moving residues."""
    t, R = t.copy(), R.copy()
    m = int(moving.sum())
    t[moving] += rng.normal(0.0, sigma, (m, 3))
    R[moving] = R[moving] @ np.swapaxes(rotvec_matrix(rng.normal(0.0, angle, (m, 3))), -1, -2)
    return t, R


def chain24(seed=0):
    """A 24-residue NeRF chain with trans omega, residues 6..16 moving: frames (float64) and the patch tables (1,24)."""
    rng = np.random.default_rng(seed)
    L = 24
    phi, psi = rng.uniform(-2.6, -0.9, L), rng.uniform(1.8, 2.8, L)
    bb = nerf_chain(phi, psi, np.full(L, np.pi))
    t, R = frames_of(bb)
    gen = np.zeros((1, L), bool)
    gen[0, 6:17] = True
    return t, R, gen, np.ones((1, L), bool), np.zeros((1, L), np.int64), np.arange(L)[None]


# ------------------------------------------------------------------ hand-checkable cases
def test_targets_are_the_third_sides_of_the_two_triangles():
    src = open(os.path.join(REPO, "include", "diffab_hip.h")).read()
    macro = dict(re.findall(r"#define\s+DIFFAB_REFINE_(\w+)\s+([-0-9.e]+)f?\s", src))
    assert float(macro["BOND"]) == BOND == PEPTIDE and float(macro["CA_CA"]) == CA_CA and float(macro["INERTIA"]) == INERTIA
    assert abs(float(macro["CA_N"]) - CA_N) < 1e-12 and abs(CA_N - 2.426) < 1e-3
    assert abs(float(macro["C_CA"]) - C_CA) < 1e-12 and abs(C_CA - 2.437) < 1e-3
    assert int(macro["MAX_K"]) == refine.MAX_K and int(macro["MAX_ITERATIONS"]) == refine.MAX_ITERATIONS
    assert float(macro["MAX_STEP_WEIGHT"]) == refine.MAX_STEP_WEIGHT
    assert abs(INERTIA - (L_N_CA ** 2 + L_CA_C ** 2)) < 0.02
    assert abs(L_N_CA - np.linalg.norm(LOCAL_N)) < 1e-14 and LOCAL_C == (L_CA_C, 0.0, 0.0)
    # the ideal chain has these distances: the targets and the builder agree
    bb = nerf_chain(np.full(3, -1.2), np.full(3, 2.3), np.full(3, np.pi))
    assert abs(np.linalg.norm(bb[0, 1] - bb[1, 0]) - CA_N) < 1e-12 and abs(np.linalg.norm(bb[0, 2] - bb[1, 1]) - C_CA) < 1e-12
    assert abs(np.linalg.norm(bb[0, 1] - bb[1, 1]) - 3.8) < 0.02  # trans: 3.80 A to the precision the number is given with


def test_one_stretched_bond_first_step_by_hand():
    """Residue 0 fixed at the origin in the identity frame, residue 1 moving, its N on the x axis 2.0 A beyond C_0: only w_bond acts.
    d = 2.0, force on N_1 = -2 (2.0 - 1.329) = -1.342 along x; the residue moves by step x force = -0.0671 A along x, and turns by
    step / I x ((N - CA) x f)."""
    t = np.zeros((1, 2, 3))
    R = np.stack([np.eye(3), np.eye(3)])[None]
    t[0, 1] = np.array([L_CA_C + 2.0, 0.0, 0.0]) - np.array(LOCAL_N)  # N_1 = C_0 + (2, 0, 0)
    gen, rm = np.array([[False, True]]), np.ones((1, 2), bool)
    chain, ridx = np.zeros((1, 2), np.int64), np.arange(2)[None]
    o = refine.Refinement(iterations=1, step=0.05, bond=1.0, angle=0.0, trans=0.0, clash=0.0)
    out = refine_ref(t, R, gen, rm, chain, ridx, o)
    assert abs(out["energy_before"][0] - 0.671 ** 2) < 1e-12
    f = np.array([-2.0 * 0.671, 0.0, 0.0])
    assert np.abs(out["translations"][0, 1] - (t[0, 1] + 0.05 * f)).max() < 1e-14
    w = 0.05 / 4.45 * np.cross(np.array(LOCAL_N), f)  # about z: (0, 0, 1.363 x 1.342 x 0.05 / 4.45)
    assert abs(w[2] - 1.363 * 1.342 * 0.05 / 4.45) < 1e-14 and w[0] == 0 and w[1] == 0
    want = gram_schmidt(np.eye(3) @ rotvec_matrix(w).T)
    assert np.abs(out["orientations"][0, 1] - want).max() < 1e-14
    assert abs(out["max_shift"][0] - 0.0671) < 1e-14
    assert np.array_equal(out["translations"][0, 0], t[0, 0]) and np.array_equal(out["orientations"][0, 0], R[0, 0])
    assert out["energy_after"][0] < out["energy_before"][0] and out["terms"][0, 1:].max() == 0.0
    # the turn brings N_1 towards C_0: rotating about +z by a positive angle moves N (at -0.525, 1.363 from CA) to smaller x
    n_after = place(out["translations"], out["orientations"], np.float64)[0][0, 1]
    n_shifted = place(out["translations"], R, np.float64)[0][0, 1]
    assert n_after[0] < n_shifted[0]


def test_an_ideal_chain_has_no_energy_and_does_not_move():
    """The bond and the two angle targets are the chain builder's own numbers: under them an ideal chain is at rest."""
    t, R, gen, rm, chain, ridx = chain24()
    out = refine_ref(t[None], R[None], gen, rm, chain, ridx, refine.Refinement(trans=0.0, clash=0.0))
    assert out["energy_before"][0] < 1e-20 and out["energy_after"][0] < 1e-20
    assert np.abs(out["translations"] - t[None]).max() < 1e-12 and np.abs(out["orientations"] - R[None]).max() < 1e-12
    # the trans target is the round 3.80 A and the ideal geometry gives a CA - CA distance within 0.02 A of it (the test of the
    # targets): with the defaults the 12 counted links hold at most 12 x 0.02^2, and the chain gives way by less than that 0.02 A
    out = refine_ref(t[None], R[None], gen, rm, chain, ridx)
    assert out["energy_before"][0] < 12 * 0.02 ** 2 and out["energy_after"][0] <= out["energy_before"][0] and out["max_shift"][0] < 0.02


def test_zero_iterations_and_zero_weights_touch_nothing():
    rng = np.random.default_rng(3)
    t, R, gen, rm, chain, ridx = chain24()
    tn, Rn = noisy(rng, t, R, gen[0], 0.3, 0.15)
    for o in (refine.Refinement(iterations=0), refine.Refinement(bond=0.0, angle=0.0, trans=0.0, clash=0.0)):
        for dtype in (np.float64, np.float32):
            out = refine_ref(tn[None], Rn[None], gen, rm, chain, ridx, o, dtype)
            assert np.array_equal(out["translations"][0], tn.astype(dtype)) and np.array_equal(out["orientations"][0], Rn.astype(dtype))
            assert out["energy_after"][0] == out["energy_before"][0] and out["max_shift"][0] == 0.0


def test_fixed_residues_pull_but_do_not_move_and_gaps_do_not_bind():
    rng = np.random.default_rng(4)
    t, R, gen, rm, chain, ridx = chain24()
    tn, Rn = noisy(rng, t, R, np.ones(24, bool), 0.3, 0.15)  # the context is off its place too
    out = refine_ref(tn[None], Rn[None], gen, rm, chain, ridx)
    fixed = ~gen[0]
    assert np.array_equal(out["translations"][0, fixed], tn[fixed]) and np.array_equal(out["orientations"][0, fixed], Rn[fixed])
    assert (out["translations"][0, gen[0]] != tn[gen[0]]).any(-1).all()
    # a residue_idx gap after slot 10: the two sides do not feel each other through bonded terms
    gap = ridx.copy()
    gap[0, 11:] += 1
    apart = tn.copy()
    apart[11:] += np.array([0.0, 0.0, 40.0])  # far beyond any clash
    a = refine_ref(apart[None], Rn[None], gen, rm, chain, gap)
    b = refine_ref(tn[None], Rn[None], gen, rm, chain, gap, refine.Refinement(clash=0.0))
    assert np.abs(a["translations"][0, :11] - b["translations"][0, :11]).max() < 1e-12
    assert np.abs(a["translations"][0, 11:] - (b["translations"][0, 11:] + np.array([0.0, 0.0, 40.0]))).max() < 1e-12
    # a residue outside residue_mask neither moves nor pulls
    rm2 = rm.copy()
    rm2[0, 9] = False
    c = refine_ref(tn[None], Rn[None], gen, rm2, chain, ridx)
    assert np.array_equal(c["translations"][0, 9], tn[9]) and np.array_equal(c["orientations"][0, 9], Rn[9])
    far = tn.copy()
    far[9] += 100.0
    d = refine_ref(far[None], Rn[None], gen, rm2, chain, ridx)
    keep = np.arange(24) != 9
    assert np.array_equal(d["translations"][0, keep], c["translations"][0, keep])


def test_clash_pushes_two_residues_apart_once_per_pair():
    # two moving residues on different chains, 3.0 A apart: energy (3.8 - 3.0)^2 once, forces equal and opposite
    t = np.zeros((1, 2, 3))
    t[0, 1, 0] = 3.0
    R = np.stack([np.eye(3), np.eye(3)])[None]
    gen = rm = np.ones((1, 2), bool)
    chain, ridx = np.array([[0, 1]]), np.array([[0, 1]])
    out = refine_ref(t, R, gen, rm, chain, ridx, refine.Refinement(iterations=1))
    assert abs(out["energy_before"][0] - 0.8 ** 2) < 1e-12
    shift = out["translations"][0] - t[0]
    assert abs(shift[0, 0] + 0.05 * 2 * 0.8) < 1e-14 and abs(shift[1, 0] - 0.05 * 2 * 0.8) < 1e-14 and np.abs(shift[:, 1:]).max() == 0
    assert np.array_equal(out["orientations"], R)  # a force on CA turns nothing
    # chain neighbours do not clash; with a tether the pair moves less
    bound = refine_ref(t, R, gen, rm, np.zeros((1, 2), np.int64), ridx, refine.Refinement(iterations=1, bond=0.0, angle=0.0, trans=0.0))
    assert bound["energy_before"][0] == 0.0 and np.array_equal(bound["translations"], t)
    held = refine_ref(t, R, gen, rm, chain, ridx, refine.Refinement(iterations=20, tether=1.0))
    free = refine_ref(t, R, gen, rm, chain, ridx, refine.Refinement(iterations=20))
    assert 0 < held["max_shift"][0] < free["max_shift"][0] and held["terms"][0, 4] > 0 and free["terms"][0, 4] == 0


# ------------------------------------------------------------------ what the defaults rest on
@pytest.fixture(scope="module")
def perturbed():
    rng = np.random.default_rng(11)
    t, R, gen, rm, chain, ridx = chain24(seed=5)
    tn, Rn = noisy(rng, t, R, gen[0], 0.3, 0.15)
    return tn, Rn, gen, rm, chain, ridx


def peptide_deviation(out, gen, chain, ridx, rm):
    n, c = place(out["translations"], out["orientations"], np.float64)
    pts = np.stack([n, out["translations"], c], axis=2)
    return backbone_ref(pts, gen, chain, ridx, rm)["max_peptide_deviation"]


def test_energy_is_non_increasing_and_the_bonds_close(perturbed):
    tn, Rn, gen, rm, chain, ridx = perturbed
    before = peptide_deviation(dict(translations=tn[None], orientations=Rn[None]), gen, chain, ridx, rm)[0]
    out = refine_ref(tn[None], Rn[None], gen, rm, chain, ridx, trace=True)
    e = np.concatenate([[out["energy_before"][0]], out["trace"][:, 0]])
    print(f"energy {e[0]:.4g} -> {e[-1]:.4g} (after orthonormalisation {out['energy_after'][0]:.4g}); worst peptide deviation {before:.3g} -> "
          f"{peptide_deviation(out, gen, chain, ridx, rm)[0]:.3g} A; max_shift {out['max_shift'][0]:.3g} A")
    assert len(e) == 201 and (np.diff(e) <= 0).all()
    assert before > 0.3 and peptide_deviation(out, gen, chain, ridx, rm)[0] < 0.05
    assert out["energy_after"][0] <= e[-1] * (1 + 1e-9) + 1e-12
    O = out["orientations"][0]
    assert np.abs(O @ np.swapaxes(O, -1, -2) - np.eye(3)).max() < 1e-14


def test_float32_run_stays_next_to_the_float64_run(perturbed):
    tn, Rn, gen, rm, chain, ridx = perturbed
    t32, R32 = tn.astype(np.float32), Rn.astype(np.float32)
    a = refine_ref(t32[None], R32[None], gen, rm, chain, ridx, dtype=np.float32)
    b = refine_ref(t32[None], R32[None], gen, rm, chain, ridx, dtype=np.float64)
    assert a["translations"].dtype == np.float32
    dt_, dO = np.abs(a["translations"] - b["translations"]).max(), np.abs(a["orientations"] - b["orientations"]).max()
    print(f"float32 against float64 after 200 iterations: translations {dt_:.3g} A, orientations {dO:.3g}")
    assert dt_ < 2.5e-4 and dO < 2.5e-5  # a quarter of the 1e-3 A and 1e-4 the GPU test asks of its allowance


# ------------------------------------------------------------------ C ABI
def test_header_symbol_table_struct_and_macro():
    src = open(os.path.join(REPO, "include", "diffab_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    lib = _hip.load_library()
    name = "diffab_refine_backbone"
    assert re.search(r"\bint\s+" + name + r"\s*\(", code) and name in _hip.SYMBOLS and hasattr(lib, name)
    assert not name.startswith("diffab_sample_loop") and not name.startswith("diffab_sample_init")
    res, args = _hip.SYMBOLS[name]
    assert res is ctypes.c_int and len(args) == 19 and args[6:9] == [ctypes.c_int32] * 3 and args[9] == ctypes.POINTER(_hip.RefineOptions)
    assert args[-1] is ctypes.c_void_p and args[-2] is ctypes.c_size_t
    want = header_struct("diffab_refine_options")
    mine = _hip.RefineOptions
    assert [f[0] for f in mine._fields_] == [f[0] for f in want._fields_]
    assert ctypes.sizeof(mine) == ctypes.sizeof(want) == 36
    for field, ctype in want._fields_:
        assert getattr(mine, field).offset == getattr(want, field).offset and getattr(mine, field).size == ctypes.sizeof(ctype), field
    assert [f[0] for f in mine._fields_][0] == "struct_bytes"
    o = refine.Refinement(iterations=7, step=0.02, bond=2.0, angle=0.5, trans=0.25, clash=3.0, tether=0.125, clash_distance=4.0).c_struct()
    assert (o.struct_bytes, o.iterations, o.w_bond, o.w_angle, o.w_trans, o.w_clash, o.w_tether, o.clash_distance) == \
        (36, 7, 2.0, 0.5, 0.25, 3.0, 0.125, 4.0) and o.step == np.float32(0.02)
    # the defaults of the header are the defaults of the dataclass
    defaults = re.search(r"#define\s+DIFFAB_REFINE_DEFAULTS\s+\{\(uint32_t\)sizeof\(diffab_refine_options\),([^}]*)\}", code).group(1)
    d = refine.Refinement()
    assert [float(v.strip().rstrip("f")) for v in defaults.split(",")] == \
        [d.iterations, d.step, d.bond, d.angle, d.trans, d.clash, d.tether, d.clash_distance]
    # the workspace macro
    body = re.search(r"#define\s+DIFFAB_REFINE_WORKSPACE_BYTES\(G, K\)\s+(.*)", code).group(1)
    for G, K in ((1, 1), (3, 70), (16, 128), (5, 256)):
        assert eval(body.replace("(size_t)", ""), {"G": G, "K": K}) == refine.workspace_bytes(G, K)
    lds = re.search(r"#define\s+DIFFAB_REFINE_LDS_BYTES\(K\)\s+(.*)", code).group(1)
    assert eval(lds.replace("(size_t)", ""), {"K": 256}) == 37888 < 64 * 1024


def test_host_side_refusals_touch_no_gpu():
    """Every refusal is decided from the scalar arguments, the options and whether a pointer is null: the pointers are fake addresses
    that are never dereferenced, nothing is enqueued (no GPU is needed), and diffab_last_error names the problem."""
    l = _hip.load_library()
    p, q, null = ctypes.c_void_p(4096), ctypes.c_void_p(8192), ctypes.c_void_p(0)

    def err():
        return l.diffab_last_error().decode()

    def call(rows=10, group=5, K=128, opt=None, t=p, O=p, gm=p, rm=null, chain=p, ridx=p, t_out=q, O_out=q, extra=q, ws=p, ws_bytes=1 << 40):
        return l.diffab_refine_backbone(t, O, gm, rm, chain, ridx, rows, group, K, None if opt is None else ctypes.byref(opt), t_out, O_out,
                                        extra, extra, extra, extra, ws, ws_bytes, null)

    def options(**kw):
        o = _hip.RefineOptions(200, 0.05, 1.0, 1.0, 1.0, 1.0, 0.0, 3.8)
        for k, v in kw.items():
            setattr(o, k, v)
        return o

    need = refine.workspace_bytes(2, 128)
    assert call(ws_bytes=need // 2) == -4 and "needed" in err()  # DIFFAB_ERR_WORKSPACE: every argument check passed
    assert need - 1024 <= int(re.search(r"(\d+) needed", err()).group(1)) <= need
    assert call(opt=options(), ws_bytes=16) == -4 and call(extra=null, rm=p, ws_bytes=16) == -4  # the optional outputs may be null
    assert call(opt=options(step=0.05, w_bond=2.0), ws_bytes=16) == -4  # 0.05 x 2 = 0.1 in fp32 is not above the bound
    assert call(opt=options(iterations=0), ws_bytes=16) == -4
    bad = options()
    bad.struct_bytes = 32
    bad.iterations = -5  # not read: the size is refused first
    assert call(opt=bad) == -1 and "struct_bytes" in err()
    for kw, word in ((dict(rows=11), "not a multiple"), (dict(rows=-5), "extent"), (dict(group=0), "extent"), (dict(K=0), "extent"),
                     (dict(K=257), "at most 256"), (dict(t=null), "null input"), (dict(O=null), "null input"), (dict(gm=null), "null input"),
                     (dict(chain=null), "null input"), (dict(ridx=null), "null input"), (dict(t_out=null), "null output"),
                     (dict(O_out=null), "null output"), (dict(t_out=p), "aliases"), (dict(O_out=p), "aliases"), (dict(ws=null), "workspace"),
                     (dict(ws=ctypes.c_void_p(4100)), "16-byte aligned"),
                     (dict(opt=options(iterations=-1)), "iterations"), (dict(opt=options(iterations=100001)), "iterations"),
                     (dict(opt=options(step=0.0)), "step must be"), (dict(opt=options(step=float("nan"))), "step must be"),
                     (dict(opt=options(step=float("inf"))), "step must be"), (dict(opt=options(w_bond=-1.0)), "w_bond"),
                     (dict(opt=options(w_angle=float("nan"))), "w_angle"), (dict(opt=options(w_trans=float("inf"))), "w_trans"),
                     (dict(opt=options(w_clash=-0.5)), "w_clash"), (dict(opt=options(w_tether=-1e-3)), "w_tether"),
                     (dict(opt=options(clash_distance=0.0)), "clash_distance"), (dict(opt=options(clash_distance=float("nan"))), "clash_distance"),
                     (dict(opt=options(step=0.12)), "not stable"), (dict(opt=options(step=0.05, w_tether=2.5)), "not stable"),
                     (dict(opt=options(step=0.01, w_clash=11.0)), "not stable")):
        rc = call(**kw)
        assert rc == -1 and word in err(), (kw, rc, err())
    # an empty problem returns 0 before any pointer is looked at; its options are still checked
    assert l.diffab_refine_backbone(*[null] * 6, 0, 5, 128, None, *[null] * 6, null, 0, null) == 0
    assert l.diffab_refine_backbone(*[null] * 6, 0, 5, 128, ctypes.byref(options(step=0.2)), *[null] * 6, null, 0, null) == -1


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
        refine.backbone(frames(), mask(), group_size=3, chain_idx=torch.zeros(16, dtype=torch.long), residue_idx=torch.arange(16).expand(2, 16),
                        residue_mask=~mask(), options=refine.Refinement(iterations=3, step=0.05, bond=2.0, tether=0.5))
    with pytest.raises(ReachedTheLibrary):
        refine.backbone(frames(), mask(), group_size=3)
    with pytest.raises(ReachedTheLibrary):
        refine.backbone(frames(2, 256), mask(2, 256))


@pytest.mark.parametrize("kw, match", [
    (dict(iterations=-1), "iterations must be"), (dict(iterations=2.0), "iterations must be"), (dict(iterations=True), "iterations must be"),
    (dict(iterations=100001), "iterations must be"), (dict(step=0.0), "step must be"), (dict(step=-0.05), "step must be"),
    (dict(step=float("nan")), "step must be"), (dict(step="0.05"), "step must be"), (dict(bond=-1.0), "bond weight must be"),
    (dict(angle=float("inf")), "angle weight must be"), (dict(trans=None), "trans weight must be"), (dict(clash=-0.1), "clash weight must be"),
    (dict(tether=float("nan")), "tether weight must be"), (dict(tether=True), "tether weight must be"),
    (dict(clash_distance=0.0), "clash_distance must be"), (dict(clash_distance=float("inf")), "clash_distance must be"),
    (dict(step=0.12), "not stable"), (dict(step=0.05, bond=2.5), "not stable"), (dict(step=0.02, tether=6.0), "not stable"),
    (dict(step=0.101, bond=0.0, angle=0.0, trans=0.0, clash=1.0), "not stable"),
])
def test_refinement_is_validated_on_construction(no_library, kw, match):
    with pytest.raises(ValueError, match=match):
        refine.Refinement(**kw)


def test_refinement_at_the_stability_bound_is_accepted(no_library):
    for kw in (dict(step=0.05, bond=2.0), dict(step=0.1), dict(step=0.02, clash=5.0), dict(step=0.08), dict(step=0.3, bond=0.0, angle=0.0,
                                                                                                    trans=0.0, clash=0.0)):
        refine.Refinement(**kw)
    assert refine.Refinement() == refine.Refinement(200, 0.05, 1.0, 1.0, 1.0, 1.0, 0.0, 3.8)


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
    (dict(designs=frames(2, 257), generation_mask=mask(2, 257), group_size=1), "K = 257 residues per patch, at most 256"),
    (dict(chain_idx=torch.zeros(16)), "integer chain_idx"), (dict(chain_idx=torch.zeros(3, 16, dtype=torch.long)), "chain_idx .* does not broadcast"),
    (dict(residue_idx=torch.zeros(15, dtype=torch.long)), "residue_idx .* does not broadcast"),
    (dict(residue_idx=torch.zeros(16, dtype=torch.bool)), "integer residue_idx"),
    (dict(residue_idx=torch.full((16,), 2 ** 40)), "residue_idx values must fit in int32"),
    (dict(options=dict(iterations=3)), "options must be a refine.Refinement"), (dict(options=200), "options must be a refine.Refinement"),
])
def test_argument_errors_come_before_the_library(no_library, kw, match):
    args = dict(designs=frames(), generation_mask=mask(), group_size=3)
    args.update(kw)
    designs, gm = args.pop("designs"), args.pop("generation_mask")
    with pytest.raises(ValueError, match=match):
        refine.backbone(designs, gm, **args)


def test_design_complex_refuses_a_refine_that_is_no_refinement(no_library):
    from sampler_support import stand_in

    model = stand_in(("design_complex",))
    with pytest.raises(ValueError, match="refine must be a refine.Refinement or None"):
        model.design_complex({"xyz": torch.zeros(1, 8, 4, 3), "generation_mask": torch.zeros(1, 8, dtype=torch.bool)}, refine=dict(iterations=3))


def test_the_package_exports_the_module():
    import diffab_pytorch

    assert diffab_pytorch.refine is refine and callable(refine.backbone) and refine.TERMS == ("bond", "angle", "trans", "clash", "tether")
