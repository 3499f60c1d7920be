"""Design filters on the MI355X: diffab_metrics_backbone / _contacts through diffab_pytorch.metrics.

The oracle is test_geometry_host.py's, run on the SAME fp32 points the kernels read (the frame kernel's atoms, the patch's xyz).
Every integer output must EQUAL the oracle: the squared distances and the comparisons are defined fp32 numbers.  The float bounds, from
the arithmetic the header fixes:
  phi, psi, omega   wrapped |dev - ref| <= 5e-7 rad      (half an fp32 ulp at pi, 1.2e-7, plus fp64 noise), on dihedrals whose two cross
                                                          products exceed 1e-3 A^2 - asserted on the oracle for every dihedral compared
  peptide_bond, min_distance   |dev - ref| <= 2e-7 * ref  (one fp32 rounding of an fp64 value; the fp32 root of an fp32 number)
  clash_score       |dev - ref| <= 3e-6 A^2 * n_clash     (a clashing d is below 3 A: one fp32 ulp on d, 2.4e-7, times 2 (clash - d) <= 6 A
                                                          is 1.4e-6 per term, doubled)
Measured on the MI355X (this file, printed by the tests): see DESIGN.md section 4.15."""
import functools

import numpy as np
import pytest
import torch

from diffab_pytorch import DiffAb, io as dio, metrics, patch, synthetic as syn
from sampler_support import hip
from test_geometry_host import backbone_ref, contacts_ref, frames_of, nerf_chain, tangle_chain_keys, wrapped

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("hip")]  # every test here needs the device, whether it names the fixture or not

CHUNK_ATOMS = metrics.CONTACTS_CHUNK_ATOMS  # context atoms the contacts kernel stages in LDS per pass (include/diffab_hip.h)
CHUNK_RESIDUES = metrics.CONTACTS_CHUNK_RESIDUES
ATOMS5 = dio.BACKBONE_ATOMS


def rotation(rng):
    q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
    return q * np.sign(np.linalg.det(q))


# ------------------------------------------------------------------ patches: two antibody chains and an antigen chain, from NeRF chains
def build_chain(rng, L):
    phi, psi = rng.uniform(-2.6, -0.9, L), np.where(rng.random(L) < 0.5, rng.uniform(-1.0, -0.4, L), rng.uniform(1.8, 2.8, L))
    return nerf_chain(phi, psi, np.pi + rng.normal(0.0, 0.06, L))


def build_patch(rng, K, A, role, dense):
    """One patch of K residues: chain 1 (heavy, with the loop), chain 2 (light), chain 3 (the antigen), each a NeRF chain moved rigidly
    to lie next to the others.  role: 'one' generated residue, 'none', or a 'loop' of nine with a residue_idx gap inside.  Returns the
    per-residue fields (numpy) with real atoms xyz (K,A,3): N, CA, C, O, CB from the frames, then side-chain atoms, ragged atom_mask."""
    n1 = K * 2 // 5
    n2 = (K - n1) // 2
    lengths = (n1, n2, K - n1 - n2)
    bb, chain, ridx = [], [], []
    for c, L in enumerate(lengths):
        b = build_chain(rng, L)
        b = (b - b[:, 1].mean(0)) @ rotation(rng).T
        b += np.array([[0.0, 0.0, 0.0], [9.0, 3.0, 0.0], [3.0, 10.0, 4.0]])[c] + rng.normal(0.0, 1.0, 3)
        bb.append(b)
        chain += [c + 1] * L
        r = np.arange(L) + 100 * c
        r[L // 2:] += 1  # a deleted residue in the middle of every chain
        ridx.append(r)
    bb, chain, ridx = np.concatenate(bb), np.array(chain), np.concatenate(ridx)
    gen = np.zeros(K, bool)
    if role == "one":
        gen[5] = True
    elif role == "loop":
        gen[n1 // 2 - 5:n1 // 2 + 4] = True  # spans the gap of chain 1
    t, R = frames_of(bb)
    t, R = t.astype(np.float32), R.astype(np.float32)
    seq = rng.integers(0, 20, K)
    seq[np.flatnonzero(gen)[::3]] = 7  # Gly at generated positions
    seq[2] = 7
    frame_atoms = dio.backbone_from_frames(torch.from_numpy(t), torch.from_numpy(R), ATOMS5).numpy()  # (K,5,3)
    xyz = np.zeros((K, A, 3), np.float32)
    xyz[:, :5] = frame_atoms
    xyz[:, 5:] = frame_atoms[:, 4:5] + rng.normal(0.0, 1.4, (K, A - 5, 3)).astype(np.float32)
    am = np.ones((K, A), bool) if dense else rng.random((K, A)) < 0.75
    am[:, :4] = True
    am[seq == 7, 4:] = False
    am[3] = False  # a context residue without a single atom
    am[3, 1] = dense
    return dict(seq_idx=seq, translations=t, orientations=R, xyz=xyz, atom_mask=am, chain_idx=chain, residue_idx=ridx, generation_mask=gen)


KINDS = ("native", "noisy", "pushed", "pulled")


def design_of(rng, p, antigen, kind):
    """One design of a patch: its native frames; noisy frames (translations + N(0, 1 A), random frame rotations, new tokens) on the
    generated residues; the loop pushed into the antigen; the loop pulled 30 A away from everything."""
    seq, t, R = p["seq_idx"].copy(), p["translations"].astype(np.float64), p["orientations"].astype(np.float64)
    gen = p["generation_mask"]
    n = int(gen.sum())
    if n and kind == "noisy":
        t[gen] += rng.normal(0.0, 1.0, (n, 3))
        R[gen] = R[gen] @ np.stack([rotation(rng) for _ in range(n)])
        seq[gen] = np.where(rng.random(n) < 0.3, 7, rng.integers(0, 20, n))
    elif n and kind == "pushed":
        t[gen] += 0.85 * (p["translations"][antigen].mean(0) - t[gen].mean(0))
    elif n and kind == "pulled":
        rest = p["translations"][~gen].astype(np.float64)
        away = t[gen].mean(0) - rest.mean(0)
        away /= np.linalg.norm(away)
        t[gen] += away * (30.0 + ((rest - rest.mean(0)) @ away).max())  # 30 A beyond the last residue of the patch on that side
    return seq, t.astype(np.float32), R.astype(np.float32)


@functools.lru_cache(maxsize=None)
def case(N, K, A=15, dense=False, kinds=KINDS, seed=0):
    """G = 3 patches x N designs: patch 0 has one generated residue and no antigen flagged, patch 1 no generated residue, patch 2 a
    loop; residue_mask removes a generated and two context residues of patch 2.  Everything the tests need, the oracle inputs as numpy
    and the device inputs as tensors; computed once per shape."""
    rng = np.random.default_rng(1000 * K + 10 * N + A + seed)
    G = 3
    patches = [build_patch(rng, K, A, role, dense) for role in ("one", "none", "loop")]
    stack = lambda k: np.stack([p[k] for p in patches])
    gen, chain, ridx = stack("generation_mask"), stack("chain_idx"), stack("residue_idx")
    antigen = (chain == 3)
    antigen[0] = False
    hotspot = antigen & (rng.random((G, K)) < 0.4)
    rm = np.ones((G, K), bool)
    loop = np.flatnonzero(gen[2])
    rm[2, loop[2]] = False
    rm[2, [1, K - 2]] = False
    rows = [design_of(rng, patches[g], chain[g] == 3, kinds[(g + r) % len(kinds)]) for g in range(G) for r in range(N)]
    kind_of_row = [kinds[(g + r) % len(kinds)] for g in range(G) for r in range(N)]
    des = {"seq_idx": np.stack([r[0] for r in rows]), "translations": np.stack([r[1] for r in rows]), "orientations": np.stack([r[2] for r in rows])}
    cuda = lambda v: torch.from_numpy(np.ascontiguousarray(v)).cuda()
    c = dict(G=G, N=N, K=K, A=A, gen=gen, chain=chain, ridx=ridx, antigen=antigen, hotspot=hotspot, rm=rm, kinds=kind_of_row,
             designs={k: cuda(v) for k, v in des.items()}, context={"xyz": cuda(stack("xyz")), "atom_mask": cuda(stack("atom_mask"))},
             xyz=stack("xyz"), atom_bits=(stack("atom_mask").astype(np.int64) << np.arange(A)).sum(-1))
    c["kw"] = dict(chain_idx=cuda(chain), residue_idx=cuda(ridx), residue_mask=cuda(rm), group_size=N)
    c["gen_d"], c["antigen_d"], c["hotspot_d"] = cuda(gen), cuda(antigen), cuda(hotspot)
    return c


TANGLED = (2, 257)  # (N, K) of tangled_case: the chain rule where one links kernel serves four entries, past its 256 threads


@functools.lru_cache(maxsize=None)
def tangled_case(N, K):
    """G = 2 patches x N designs with the keys of test_geometry_host.tangle_chain_keys in chain 1, at slots 38 .. 50 and 20 .. 32, and
    in the last slot of the patch; those slots are generated, so their bonds are counted.  The fields of case()."""
    rng = np.random.default_rng(1000 * K + 10 * N + 7)
    G = 2
    patches = [build_patch(rng, K, 15, "loop", False) for _ in range(G)]
    rm = np.ones((G, K), bool)
    for g, at in enumerate((38, 20)):
        p = patches[g]
        p["chain_idx"], p["residue_idx"] = p["chain_idx"].astype(np.int32), p["residue_idx"].astype(np.int32)
        tangle_chain_keys(p["chain_idx"], p["residue_idx"], rm[g], at, K - 1)
        p["generation_mask"][at:at + 13] = p["generation_mask"][K - 1] = True
    stack = lambda k: np.stack([p[k] for p in patches])
    gen, chain, ridx = stack("generation_mask"), stack("chain_idx"), stack("residue_idx")
    kinds = [("native", "pushed")[(g + r) % 2] for g in range(G) for r in range(N)]
    rows = [design_of(rng, patches[g], chain[g] == 3, kinds[g * N + r]) for g in range(G) for r in range(N)]
    des = {"seq_idx": np.stack([r[0] for r in rows]), "translations": np.stack([r[1] for r in rows]), "orientations": np.stack([r[2] for r in rows])}
    cuda = lambda v: torch.from_numpy(np.ascontiguousarray(v)).cuda()
    c = dict(G=G, N=N, K=K, gen=gen, chain=chain, ridx=ridx, rm=rm, kinds=kinds, designs={k: cuda(v) for k, v in des.items()})
    c["kw"] = dict(chain_idx=cuda(chain), residue_idx=cuda(ridx), residue_mask=cuda(rm), group_size=N)
    c["gen_d"] = cuda(gen)
    return c


def design_points(designs, atoms):
    """The fp32 atoms the contacts kernel reads, and their validity bits, as numpy."""
    pts = dio.backbone_from_frames(designs["translations"], designs["orientations"], atoms).float().cpu().numpy()
    seq = designs["seq_idx"].cpu().numpy()
    bits = np.full(seq.shape, (1 << len(atoms)) - 1, np.int64)
    if "CB" in atoms:
        bits[seq == 7] &= ~(1 << atoms.index("CB"))
    return pts, bits


def numpy_of(out):
    return {k: v.cpu().numpy() for k, v in out.items()}


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


# ------------------------------------------------------------------ backbone
def check_backbone(c, out, ref, angles, what):
    for k in ("n_bonds", "n_chain_break", "n_cis"):
        assert out[k].dtype == np.int32 and np.array_equal(out[k], ref[k]), (what, k, out[k], ref[k])
    for k in ("phi", "psi", "omega", "peptide_bond"):
        assert out[k].dtype == np.float32 and out[k].shape == ref[k].shape and np.array_equal(np.isnan(out[k]), np.isnan(ref[k])), (what, k)
    ok = ~np.isnan(ref["peptide_bond"])
    rel = np.abs(out["peptide_bond"][ok].astype(np.float64) - ref["peptide_bond"][ok]) / ref["peptide_bond"][ok]
    dev = np.abs(out["max_peptide_deviation"].astype(np.float64) - ref["max_peptide_deviation"])
    print(f"{what}: peptide_bond max rel {rel.max(initial=0.0):.3g}, max_peptide_deviation max abs {dev.max(initial=0.0):.3g}")
    assert (rel <= 2e-7).all()
    assert (dev <= 2e-7 * (ref["max_peptide_deviation"] + 1.329)).all()  # the deviation of a bond length that is itself within 2e-7 relative
    if angles:
        assert ref["min_cross"] > 1e-3, ref["min_cross"]  # every dihedral of these designs is well conditioned: nothing is left out
        worst = 0.0
        for k in ("phi", "psi", "omega"):
            ok = ~np.isnan(ref[k])
            worst = max(worst, wrapped(out[k][ok], ref[k][ok]).max(initial=0.0))
            assert (np.abs(out[k][ok]) <= np.float32(np.pi)).all()
        print(f"{what}: dihedrals max wrapped |dev - ref| = {worst:.3g} rad (min cross product {ref['min_cross']:.3g} A^2)")
        assert worst <= 5e-7


@pytest.mark.parametrize("N, K", [(N, K) for K in (40, 130) for N in (1, 5, 70)] + [(3, 70), (3, 300), TANGLED])
def test_backbone_equals_the_oracle(N, K):
    """The native, the pushed and the pulled loop: dihedrals, bond lengths and counts.  K = 70 and K = 300: the chain neighbours of a patch
    past 64 slots that is no multiple of 64, and of one past the 256 threads of the links kernel.  TANGLED: keys on which a 32-bit gap,
    the highest slot, a masked slot or another chain would give other neighbours."""
    c = tangled_case(N, K) if (N, K) == TANGLED else case(N, K, kinds=("native", "pushed", "pulled"))
    out = numpy_of(metrics.backbone(c["designs"], c["gen_d"], **c["kw"]))
    pts = design_points(c["designs"], ("N", "CA", "C"))[0]
    ref = backbone_ref(pts, c["gen"], c["chain"], c["ridx"], c["rm"], N)
    assert ref["tolerance_gap"] > 1e-4 and ref["cis_gap"] > 1e-4  # the threshold counts are well defined
    check_backbone(c, out, ref, True, f"backbone N={N} K={K}")
    if (N, K) == TANGLED:
        assert (ref["n_bonds"] >= 6).all(), ref["n_bonds"]  # the tangled slots are generated: their links are counted bonds
        return  # (what follows is about the three patches of case())
    rows = np.arange(3 * N)
    assert (out["n_bonds"][rows // N == 1] == 0).all() and (out["max_peptide_deviation"][rows // N == 1] == 0).all()  # no generated residue
    assert (out["n_bonds"][rows // N == 0] == 2).all()  # one generated residue inside a chain
    native = np.array([k == "native" for k in c["kinds"]])
    assert (out["n_chain_break"][native] == 0).all() and (out["n_cis"][native] == 0).all()
    pulled = np.array([k == "pulled" for k in c["kinds"]]) & (rows // N != 1)
    assert (out["n_chain_break"][pulled] >= 1).all() and (out["max_peptide_deviation"][pulled] > 20.0).all()
    # a residue outside residue_mask and the ends of the residue_idx gaps define nothing
    loop = np.flatnonzero(c["gen"][2])
    assert np.isnan(out["phi"][2 * N:, loop[2]]).all() and np.isnan(out["psi"][2 * N:, loop[1]]).all() and np.isnan(out["phi"][2 * N:, loop[3]]).all()


@pytest.mark.parametrize("K", [40, 130])
def test_backbone_counts_on_noisy_frames(K):
    """Noisy frames break bonds and produce cis: counts and bond lengths against the oracle (the dihedrals of noisy frames can be
    ill-conditioned and are not compared)."""
    N = 5
    c = case(N, K, seed=1)
    out = numpy_of(metrics.backbone(c["designs"], c["gen_d"], **c["kw"]))
    ref = backbone_ref(design_points(c["designs"], ("N", "CA", "C"))[0], c["gen"], c["chain"], c["ridx"], c["rm"], N)
    assert ref["tolerance_gap"] > 1e-4 and ref["cis_gap"] > 1e-4
    check_backbone(c, out, ref, False, f"backbone noisy K={K}")
    noisy = np.array([k == "noisy" for k in c["kinds"]]) & (np.arange(3 * N) // N == 2)
    assert (out["n_chain_break"][noisy] >= 1).all() and out["n_cis"][noisy].sum() >= 1
    wide = numpy_of(metrics.backbone(c["designs"], c["gen_d"], bond_tolerance=500.0, **c["kw"]))
    assert (wide["n_chain_break"] == 0).all() and np.array_equal(wide["n_bonds"], out["n_bonds"])


def test_backbone_defaults_and_rows_alone():
    """Without tables: one chain, arange(K), every residue present.  Rows [lo, hi) alone give the bits of the whole call."""
    N, K = 5, 40
    c = case(N, K)
    out = numpy_of(metrics.backbone(c["designs"], c["gen_d"], group_size=N))
    one = np.zeros((3, K), np.int64)
    ref = backbone_ref(design_points(c["designs"], ("N", "CA", "C"))[0], c["gen"], one, np.arange(K) + one, one == 0, N)
    check_backbone(c, out, ref, False, "backbone defaults")
    assert out["n_bonds"][2 * N] == c["gen"][2].sum() + 1
    full = numpy_of(metrics.backbone(c["designs"], c["gen_d"], **c["kw"]))
    part = numpy_of(metrics.backbone({k: v[N:3 * N] for k, v in c["designs"].items()}, c["gen_d"][1:],
                                     **{k: (v if k == "group_size" else v[1:]) for k, v in c["kw"].items()}))
    for k, v in part.items():
        assert same_bits(v, full[k][N:3 * N]), k


# ------------------------------------------------------------------ contacts
def check_contacts(c, out, ref, what, antigen=True, hotspot=True):
    ints = ["n_clash", "residue_clash"] + (["n_contact_pairs", "n_paratope", "n_epitope", "residue_contact"] if antigen else []) \
        + (["n_hotspot_contacted", "n_hotspot"] if hotspot else [])
    assert set(out) == set(ints) | {"clash_score", "min_distance"}, sorted(out)
    for k in ints:
        assert out[k].dtype == np.int32 and np.array_equal(out[k], ref[k]), (what, k, np.flatnonzero((out[k] != ref[k]).reshape(len(ref[k]), -1).any(1)))
    assert out["min_distance"].dtype == np.float32 and np.array_equal(np.isinf(out["min_distance"]), np.isinf(ref["min_distance"]))
    ok = ~np.isinf(ref["min_distance"])
    rel = np.abs(out["min_distance"][ok].astype(np.float64) - ref["min_distance"][ok]) / ref["min_distance"][ok]
    err = np.abs(out["clash_score"].astype(np.float64) - ref["clash_score"])
    per_term = (err / np.maximum(ref["n_clash"], 1)).max(initial=0.0)
    print(f"{what}: min_distance max rel {rel.max(initial=0.0):.3g}; clash_score max |dev - ref| / n_clash = {per_term:.3g} A^2 "
          f"(largest n_clash {ref['n_clash'].max()}, largest n_contact_pairs {ref['n_contact_pairs'].max()})")
    assert (rel <= 2e-7).all()
    assert (err <= 3e-6 * ref["n_clash"]).all()


def reference(c, atoms=ATOMS5, context=True, **kw):
    pts, bits = design_points(c["designs"], atoms)
    if context:
        cpts, cbits = c["xyz"], c["atom_bits"]
    else:
        cpts, cbits = pts[::c["N"]], bits[::c["N"]]
    return contacts_ref(pts, bits, cpts, cbits, c["gen"], c["rm"], c["chain"], c["ridx"], c["antigen"], c["hotspot"], c["N"], **kw)


def by_patch(c, v, g):
    return v[g * c["N"]:(g + 1) * c["N"]]


@pytest.mark.parametrize("K", [40, 130])
@pytest.mark.parametrize("N", [1, 5, 70])
def test_contacts_equal_the_oracle(N, K):
    c = case(N, K)
    out = numpy_of(metrics.contacts(c["designs"], c["gen_d"], context=c["context"], antigen_mask=c["antigen_d"], hotspot_mask=c["hotspot_d"], **c["kw"]))
    ref = reference(c)
    check_contacts(c, out, ref, f"contacts N={N} K={K}")
    # patch 1 has no generated residue: nothing to count; patch 0 has no antigen: no contact
    assert (by_patch(c, out["n_clash"], 1) == 0).all() and np.isinf(by_patch(c, out["min_distance"], 1)).all()
    assert (by_patch(c, out["clash_score"], 1) == 0).all() and (by_patch(c, out["residue_clash"], 1) == 0).all()
    assert (by_patch(c, out["n_contact_pairs"], 0) == 0).all() and (by_patch(c, out["n_hotspot"], 0) == 0).all()
    assert (by_patch(c, out["n_hotspot"], 2) == (c["hotspot"][2] & c["rm"][2]).sum()).all()
    assert (out["residue_clash"].sum(1) == 2 * out["n_clash"]).all() and (out["residue_contact"].sum(1) == 2 * out["n_contact_pairs"]).all()
    kinds = np.array(c["kinds"])
    loop = np.arange(3 * N) // N == 2
    assert (out["n_contact_pairs"][loop & (kinds == "pushed")] > 0).all() and (out["n_clash"][loop & (kinds == "pushed")] > 0).all()
    # the pulled loop touches nothing of the patch (its own residues two apart still count: its min_distance stays small); the one
    # pulled residue of patch 0 has nothing near it at all
    far = loop & (kinds == "pulled")
    assert (out["n_contact_pairs"][far] == 0).all() and (out["residue_clash"][far][:, ~c["gen"][2]] == 0).all()
    alone = (np.arange(3 * N) // N == 0) & (kinds == "pulled")
    assert (ref["min_distance"][alone] > 25.0).all()  # (the construction, on the oracle)
    assert (out["min_distance"][alone] > 25.0).all() and (out["n_clash"][alone] == 0).all()
    # residues outside residue_mask take part in nothing
    assert (by_patch(c, out["residue_clash"], 2)[:, ~c["rm"][2]] == 0).all() and (by_patch(c, out["residue_contact"], 2)[:, ~c["rm"][2]] == 0).all()


def test_contacts_without_masks_and_other_cutoffs():
    N, K = 5, 40
    c = case(N, K)
    out = numpy_of(metrics.contacts(c["designs"], c["gen_d"], context=c["context"], **c["kw"]))
    check_contacts(c, out, reference(c), "contacts, no antigen", antigen=False, hotspot=False)
    out = numpy_of(metrics.contacts(c["designs"], c["gen_d"], context=c["context"], antigen_mask=c["antigen_d"], clash_distance=3.6,
                                    contact_distance=8.0, **c["kw"]))
    ref = reference(c, clash_distance=3.6, contact_distance=8.0)
    assert (np.abs(out["clash_score"] - ref["clash_score"]) <= 3e-6 * 1.2 * ref["n_clash"]).all()  # (2 (clash - d) <= 7.2 A at 3.6 A)
    for k in ("n_clash", "residue_clash", "n_contact_pairs", "n_paratope", "n_epitope", "residue_contact"):
        assert np.array_equal(out[k], ref[k]), k
    four = ("N", "CA", "C", "O")  # no CB anywhere on the designs
    out = numpy_of(metrics.contacts(c["designs"], c["gen_d"], context=c["context"], antigen_mask=c["antigen_d"], hotspot_mask=c["hotspot_d"],
                                    atoms=four, **c["kw"]))
    check_contacts(c, out, reference(c, atoms=four), "contacts, four atoms")


@pytest.mark.parametrize("N", [5, 70])
def test_contacts_context_from_the_frames(N):
    """context=None: the non-generated residues take the frame atoms of the first row of their group - the same call as passing those
    atoms as the context, to the bit."""
    c = case(N, 40)
    kw = dict(antigen_mask=c["antigen_d"], hotspot_mask=c["hotspot_d"], **c["kw"])
    out = numpy_of(metrics.contacts(c["designs"], c["gen_d"], **kw))
    check_contacts(c, out, reference(c, context=False), f"contacts, frame context N={N}")
    pts, bits = design_points(c["designs"], ATOMS5)
    mask = ((bits[::N, :, None] >> np.arange(5)) & 1).astype(bool)
    explicit = {"xyz": torch.from_numpy(pts[::N].copy()).cuda(), "atom_mask": torch.from_numpy(mask).cuda()}
    again = numpy_of(metrics.contacts(c["designs"], c["gen_d"], context=explicit, **kw))
    for k, v in out.items():
        assert same_bits(v, again[k]), k


def test_contacts_more_context_atoms_than_a_chunk():
    """K = 90 residues with all A = 32 atoms present: the valid context atoms of a patch are more than two passes of CHUNK_ATOMS = 1024
    atoms and no multiple of it (a pass ends at the atom limit, after 32 residues), where the A = 15 cases above end a pass at
    CHUNK_RESIDUES = 64 residues."""
    N, K, A = 5, 90, 32
    c = case(N, K, A=A, dense=True)
    n_atoms = [int(sum(bin(int(b)).count("1") for b in c["atom_bits"][g][~c["gen"][g] & c["rm"][g]])) for g in range(3)]
    assert all(n > 2 * CHUNK_ATOMS and n % CHUNK_ATOMS != 0 for n in n_atoms), n_atoms
    assert CHUNK_ATOMS // A < CHUNK_RESIDUES
    out = numpy_of(metrics.contacts(c["designs"], c["gen_d"], context=c["context"], antigen_mask=c["antigen_d"], hotspot_mask=c["hotspot_d"], **c["kw"]))
    check_contacts(c, out, reference(c), f"contacts K={K} A={A}, {n_atoms} context atoms")


def test_contacts_rows_alone_and_swapped():
    N, K = 70, 130
    c = case(N, K)
    kw = dict(antigen_mask=c["antigen_d"], hotspot_mask=c["hotspot_d"])
    full = numpy_of(metrics.contacts(c["designs"], c["gen_d"], context=c["context"], **kw, **c["kw"]))
    # patch 2 alone
    sub = lambda t: t[2:]
    part = numpy_of(metrics.contacts({k: v[2 * N:] for k, v in c["designs"].items()}, sub(c["gen_d"]), context={k: sub(v) for k, v in c["context"].items()},
                                     **{k: sub(v) for k, v in kw.items()}, **{k: (v if k == "group_size" else sub(v)) for k, v in c["kw"].items()}))
    for k, v in part.items():
        assert same_bits(v, full[k][2 * N:]), k
    # designs 3 and 66 of patch 2 change places (another lane, another 64-design block): so do their results, nothing else moves
    perm = np.arange(3 * N)
    perm[[2 * N + 3, 2 * N + 66]] = perm[[2 * N + 66, 2 * N + 3]]
    swapped = numpy_of(metrics.contacts({k: v[torch.from_numpy(perm).cuda()] for k, v in c["designs"].items()}, c["gen_d"], context=c["context"],
                                        **kw, **c["kw"]))
    assert not same_bits(full["residue_clash"][2 * N + 3], full["residue_clash"][2 * N + 66])
    for k, v in swapped.items():
        assert same_bits(v, full[k][perm]), k
    bb = numpy_of(metrics.backbone(c["designs"], c["gen_d"], **c["kw"]))
    bs = numpy_of(metrics.backbone({k: v[torch.from_numpy(perm).cuda()] for k, v in c["designs"].items()}, c["gen_d"], **c["kw"]))
    for k, v in bs.items():
        assert same_bits(v, bb[k][perm]), k


def test_rows_inside_a_group_alone():
    """Rows [lo, hi) from inside a group, across its 64-design block boundary, as groups of one with the patch's masks, tables and
    context repeated per row: the bits of the same rows of the whole call, for both entries."""
    N, K = 70, 130
    c = case(N, K)
    lo, hi = 2 * N + 60, 2 * N + 67  # designs 60..66 of patch 2
    n = hi - lo
    rep = lambda t: t[2:3].expand(n, *t.shape[1:]).contiguous()
    kw = {k: (1 if k == "group_size" else rep(v)) for k, v in c["kw"].items()}
    designs = {k: v[lo:hi] for k, v in c["designs"].items()}
    full = numpy_of(metrics.contacts(c["designs"], c["gen_d"], context=c["context"], antigen_mask=c["antigen_d"], hotspot_mask=c["hotspot_d"], **c["kw"]))
    part = numpy_of(metrics.contacts(designs, rep(c["gen_d"]), context={k: rep(v) for k, v in c["context"].items()},
                                     antigen_mask=rep(c["antigen_d"]), hotspot_mask=rep(c["hotspot_d"]), **kw))
    assert full["n_clash"][lo:hi].max() > 0 and full["n_contact_pairs"][lo:hi].max() > 0
    for k, v in part.items():
        assert same_bits(v, full[k][lo:hi]), k
    full = numpy_of(metrics.backbone(c["designs"], c["gen_d"], **c["kw"]))
    part = numpy_of(metrics.backbone(designs, rep(c["gen_d"]), **kw))
    for k, v in part.items():
        assert same_bits(v, full[k][lo:hi]), k


# ------------------------------------------------------------------ end to end
def test_sampled_designs_feed_both_entries():
    """sample(num_samples = 8) on the synthetic benchmark model (the call of test_gpu_metrics' end-to-end test) -> backbone, contacts
    on the sampler's own tensors, equal to the oracle on them (no claim about the values: the weights are untrained)."""
    dims = dict(syn.BENCH_DIMS, NL=2)
    model = DiffAb(dims["D"], dims["C"], dims["NL"], dims["DS"], dims["PQ"], dims["PV"], dims["H"]).cuda()
    model.denoiser.load_state_dict(syn.denoiser_state_dict(dims, seed=1, prefix=""))
    inp = {k: v.cuda() for k, v in syn.patches(2, 128, dims, seed=3, coord_sigma=8.0).items()}
    N = 8
    res = model.sample(inp["seq_idx"], inp["translations"], inp["orientations"], res_context_emb=inp["res_context_emb"],
                       pair_context_emb=inp["pair_context_emb"], generation_mask=inp["generation_mask"], seed=1, t_start=100, t_stop=90,
                       num_samples=N)
    gen = inp["generation_mask"].cpu().numpy()
    G, K = gen.shape
    one = np.zeros((G, K), np.int64)
    antigen = ~inp["generation_mask"]
    bb = numpy_of(metrics.backbone(res, inp["generation_mask"], group_size=N))
    ref = backbone_ref(design_points(res, ("N", "CA", "C"))[0], gen, one, np.arange(K) + one, one == 0, N)
    c = dict(N=N)
    check_backbone(c, bb, ref, False, "sampled backbone")
    assert bb["phi"].shape == (G * N, K)
    out = metrics.contacts(res, inp["generation_mask"], antigen_mask=antigen, group_size=N)
    assert out["n_clash"].is_cuda and out["residue_contact"].shape == (G * N, K)
    pts, bits = design_points(res, ATOMS5)
    want = contacts_ref(pts, bits, pts[::N], bits[::N], gen, one == 0, one, np.arange(K) + one, antigen.cpu().numpy(), None, N)
    check_contacts(c, numpy_of(out), want, "sampled contacts", hotspot=False)


def test_design_complex_patch_is_a_context():
    """patch.gather's dict of a small design_complex call is the `context` of contacts, its tables the tables of both entries."""
    from test_gpu_patch import complexes, make_model

    dims = dict(syn.BENCH_DIMS, NL=2)
    model = make_model(dims, 9)
    batch = complexes()
    N = 4
    out = model.design_complex(batch, seed=31, num_samples=N, t_start=12, t_stop=10)
    g = patch.gather(batch, out["patch"])
    kw = dict(chain_idx=g["chain_idx"], residue_idx=g["residue_idx"], residue_mask=g["residue_mask"], group_size=N)
    designs = {k: out[k].cuda() for k in ("seq_idx", "translations", "orientations")}
    got = numpy_of(metrics.contacts(designs, g["generation_mask"], context=g, antigen_mask=g["antigen_mask"], **kw))
    np_ = lambda t: t.cpu().numpy()
    A = g["xyz"].shape[2]
    pts, bits = design_points(designs, ATOMS5)
    ctx_bits = (np_(g["atom_mask"]).astype(np.int64) << np.arange(A)).sum(-1)
    want = contacts_ref(pts, bits, np_(g["xyz"]).astype(np.float32), ctx_bits, np_(g["generation_mask"]), np_(g["residue_mask"]), np_(g["chain_idx"]),
                        np_(g["residue_idx"]), np_(g["antigen_mask"]), None, N)
    check_contacts(dict(N=N), got, want, "design_complex contacts", hotspot=False)
    bb = numpy_of(metrics.backbone(designs, g["generation_mask"], **kw))
    ref = backbone_ref(design_points(designs, ("N", "CA", "C"))[0], np_(g["generation_mask"]), np_(g["chain_idx"]), np_(g["residue_idx"]),
                       np_(g["residue_mask"]), N)
    check_backbone(dict(N=N), bb, ref, False, "design_complex backbone")
