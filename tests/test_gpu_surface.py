"""The surface entry on the MI355X: diffab_metrics_surface through diffab_pytorch.metrics.surface.

The oracle is test_surface_host.py's brute-force float32 restatement of the rule, run on the SAME fp32 atoms the kernels read (the frame
kernel's atoms read back from the device, the patch's xyz).  Every int32 output must EQUAL the oracle, no case left out and no
tolerance: a sphere point, its squared distances and the comparisons are defined fp32 numbers, and the kernels' neighbour culling may
not change one of them.  Areas: a per-residue area is the oracle's float64 value rounded once, within 1 fp32 ulp; a per-row area within
2 fp32 ulps (room for the float64 summation order only).  The contracts of the general C ABI that the pinned tables of the older test
files cannot take for a new entry - workspace contents, operand alignment - are held here."""
import functools

import numpy as np
import pytest
import torch

from diffab_pytorch import io as dio, metrics
from sampler_support import MisalignedABI, hip
from scratch_poison import poisoned
from test_gpu_geometry import ATOMS5, KINDS, build_patch, design_of, design_points, numpy_of, same_bits
from test_surface_host import INT_OUTPUTS, R_CA, RESIDUE_AREAS, ROW_AREAS, surface_ref, ulps32

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("hip")]

RADII5 = [metrics.ATOM_RADIUS[a] for a in ATOMS5]
ROLES = ("one", "loop", "none", "loop", "loop")


def cuda(v):
    return torch.from_numpy(np.ascontiguousarray(v)).cuda()


# ------------------------------------------------------------------ analytic cases through the kernel
def ca_frames(centres):
    c = torch.tensor(centres, dtype=torch.float32).reshape(1, -1, 3).cuda()
    K = c.shape[1]
    return {"seq_idx": torch.zeros(1, K, dtype=torch.long).cuda(), "translations": c, "orientations": torch.eye(3).expand(1, K, 3, 3).contiguous().cuda()}


@pytest.mark.parametrize("S", [8, 33, 64, 96, 130, 256])
def test_one_atom_is_a_whole_sphere(S):
    gen = torch.ones(1, 1, dtype=torch.bool).cuda()
    out = numpy_of(metrics.surface(ca_frames([[3.0, -2.0, 7.5]]), gen, atoms=("CA",), n_points=S))
    assert set(out) == {"free_points", "free_area"} and out["free_points"].dtype == np.int32 and out["free_area"].dtype == np.float32
    assert out["free_points"].tolist() == [[S]]
    assert ulps32(out["free_area"], 4.0 * np.pi * float(R_CA) ** 2).max() <= 1.0
    out = numpy_of(metrics.surface(ca_frames([[3.0, -2.0, 7.5]]), gen, atoms=("CA",), n_points=S, antigen_mask=~gen, hotspot_mask=~gen))
    assert out["bound_points"].tolist() == [[S]] and out["design_buried_points"].tolist() == [[0]] and out["bsa_paratope"].tolist() == [0.0]
    assert out["n_hotspot"].tolist() == [0] and out["residue_buried"].tolist() == [[0.0]]


def test_two_equal_spheres_at_distance_R():
    """test_surface_host.py derives it: 24 of 96 points of each sphere have |z_k| > 1/2 on the other's side, none within 0.01 of it."""
    R = float(R_CA)
    des = ca_frames([[0.0, 0.0, 0.0], [0.0, 0.0, R]])
    assert des["translations"][0, 1, 2].item() == R
    both = torch.ones(1, 2, dtype=torch.bool).cuda()
    out = numpy_of(metrics.surface(des, both, atoms=("CA",)))
    assert out["free_points"].tolist() == [[72, 72]]
    assert ulps32(out["free_area"], 72 * 4.0 * np.pi * R * R / 96).max() <= 1.0
    first = torch.tensor([[True, False]]).cuda()
    out = numpy_of(metrics.surface(des, first, atoms=("CA",), antigen_mask=~first, hotspot_mask=~first))
    assert out["free_points"].tolist() == [[96, 96]] and out["bound_points"].tolist() == [[72, 72]] and out["design_buried_points"].tolist() == [[0, 24]]
    area = 24 * 4.0 * np.pi * R * R / 96
    for k in ("bsa_paratope", "bsa_epitope", "bsa_design_epitope", "hotspot_buried_area"):
        assert ulps32(out[k], area).max() <= 1.0, k
    assert ulps32(out["residue_buried"], [[area, area]]).max() <= 1.0
    assert [out[k].tolist() for k in ("n_paratope_buried", "n_epitope_buried", "n_hotspot", "n_hotspot_buried")] == [[1]] * 4


# ------------------------------------------------------------------ patches, designs and the oracle on them
@functools.lru_cache(maxsize=None)
def case(K, A, dense, N, mixed_radii=False, roles=ROLES, seed=0):
    """One patch per role x N designs.  Patch g, design r is of kind KINDS[(g + r) % 4]: with N = 1 the loops are noisy, pulled and
    native, with N = 3 every kind meets a loop.  (At K = 24 build_patch's loop is empty: those patches have no generated residue, and
    the one generated residue of patch 0 is what meets the antigen.)  Chain 3 is the antigen (not flagged on the last patch), a random
    40 % of it hotspots;
    residue_mask is ragged: it removes a generated and two context residues of every loop patch and an antigen residue of all.  Gly
    sits at generated positions, residue 3 has no valid atom (one, when dense).  Oracle inputs as numpy, device inputs as tensors."""
    rng = np.random.default_rng(7000 * K + 100 * A + 10 * N + seed)
    G = len(roles)
    patches = [build_patch(rng, K, A, role, dense) for role in roles]
    stack = lambda k: np.stack([p[k] for p in patches])
    gen, chain = stack("generation_mask"), stack("chain_idx")
    antigen = chain == 3
    antigen[G - 1] = G == 1
    hotspot = antigen & (rng.random((G, K)) < 0.4)
    rm = np.ones((G, K), bool)
    for g in range(G):
        loop = np.flatnonzero(gen[g])
        if len(loop) > 2:
            rm[g, loop[2]] = False
            rm[g, [1, K - 2]] = False
        rm[g, K - 4] = False
    rows = [design_of(rng, patches[g], chain[g] == 3, KINDS[(g + r) % 4]) for g in range(G) for r in range(N)]
    kinds = [KINDS[(g + r) % 4] for g in range(G) for r in range(N)]
    des = {"seq_idx": np.stack([r[0] for r in rows]), "translations": np.stack([r[1] for r in rows]), "orientations": np.stack([r[2] for r in rows])}
    radius = np.full((G, K, A), 1.8, np.float32)
    context = {"xyz": cuda(stack("xyz")), "atom_mask": cuda(stack("atom_mask"))}
    if mixed_radii:
        radius = rng.choice(np.array([1.2, 1.4, 1.65, 1.8, 1.9, 2.3], np.float32), size=(G, K, A))
        context["atom_radius"] = cuda(radius)
    c = dict(G=G, N=N, K=K, A=A, gen=gen, antigen=antigen, hotspot=hotspot, rm=rm, kinds=kinds, radius=radius, context=context,
             designs={k: cuda(v) for k, v in des.items()}, xyz=stack("xyz"), atom_bits=(stack("atom_mask").astype(np.int64) << np.arange(A)).sum(-1))
    c["gen_d"], c["antigen_d"], c["hotspot_d"], c["rm_d"] = cuda(gen), cuda(antigen), cuda(hotspot), cuda(rm)
    return c


def run(c, S=96, **kw):
    args = dict(context=c["context"], antigen_mask=c["antigen_d"], hotspot_mask=c["hotspot_d"], residue_mask=c["rm_d"], group_size=c["N"], n_points=S)
    args.update(kw)
    return numpy_of(metrics.surface(c["designs"], c["gen_d"], **args))


@functools.lru_cache(maxsize=None)
def reference(K, A, dense, N, mixed_radii=False, S=96, probe=1.4, roles=ROLES, seed=0):
    """The oracle on the atoms the kernels read; computed once per case and shared."""
    c = case(K, A, dense, N, mixed_radii, roles, seed)
    pts, bits = design_points(c["designs"], ATOMS5)
    return surface_ref(pts, bits, RADII5, c["xyz"], c["atom_bits"], c["radius"], c["gen"], c["rm"], metrics.sphere_points(S).numpy(),
                       antigen=c["antigen"], hotspot=c["hotspot"], group_size=N, probe=probe)


def check(out, ref, what):
    assert set(out) == set(INT_OUTPUTS) | set(RESIDUE_AREAS) | set(ROW_AREAS), sorted(out)
    for k in INT_OUTPUTS:
        assert out[k].dtype == np.int32 and out[k].shape == ref[k].shape, (what, k)
        wrong = np.flatnonzero((out[k] != ref[k]).reshape(len(ref[k]), -1).any(1))
        assert wrong.size == 0, (what, k, "rows", wrong[:10], out[k][wrong[:2]], ref[k][wrong[:2]])
    worst = {}
    for names, bound in ((RESIDUE_AREAS, 1.0), (ROW_AREAS, 2.0)):
        for k in names:
            assert out[k].dtype == np.float32 and out[k].shape == ref[k].shape, (what, k)
            worst[k] = float(ulps32(out[k], ref[k]).max(initial=0.0))
            assert np.array_equal(out[k] == 0, ref[k] == 0), (what, k)
    print(f"{what}: max fp32 ulps " + ", ".join(f"{k} {v:.2f}" for k, v in worst.items())
          + f"; largest bsa_paratope {ref['bsa_paratope'].max():.1f} A^2, design-buried points {int(ref['design_buried_points'].sum())}")
    for names, bound in ((RESIDUE_AREAS, 1.0), (ROW_AREAS, 2.0)):
        for k in names:
            assert worst[k] <= bound, (what, k, worst[k])


SHAPES = [(24, 8, False), (24, 15, True), (70, 8, False), (70, 15, True)]  # K, A, dense: 70 x 15 = 1050 context atoms


@pytest.mark.parametrize("S", [33, 96, 130])
@pytest.mark.parametrize("N", [1, 3])
@pytest.mark.parametrize("K, A, dense", SHAPES)
def test_surface_equals_the_oracle(K, A, dense, N, S):
    """K in {24, 70} x A in {8 ragged with mixed context radii, 15 dense} x roles one / loop / none x kinds native / noisy / pushed /
    pulled x group_size in {1, 3} x S in {33, 96, 130}: below a wave, the default, more than two passes and no multiple of 32."""
    mixed = not dense
    c = case(K, A, dense, N, mixed)
    out = run(c, S)
    ref = reference(K, A, dense, N, mixed, S)
    check(out, ref, f"surface K={K} A={A} N={N} S={S}")
    rows = np.arange(c["G"] * N)
    g_of = rows // N
    gen_rows = np.stack([c["gen"][g] & c["rm"][g] for g in g_of])
    assert (gen_rows.any(1) == np.isin(g_of, (0, 1, 3, 4) if K >= 70 else (0,))).all()
    # no generated residue: zeros; no antigen flagged: nothing bound away, nothing buried
    assert all((out[k][~gen_rows.any(1)] == 0).all() for k in out)
    assert np.array_equal(out["bound_points"][g_of == 4], out["free_points"][g_of == 4]) and (out["bsa_paratope"][g_of == 4] == 0).all()
    assert (out["free_points"][g_of == 0].sum(1) > 0).all() and (out["free_points"][g_of == 0][:, c["antigen"][0] & c["rm"][0]].sum(1) > 0).all()
    # framework residues and residues outside residue_mask have no numbers
    for g in range(c["G"]):
        silent = ~(c["rm"][g] & (c["gen"][g] | c["antigen"][g]))
        assert all((out[k][g_of == g][:, silent] == 0).all() for k in ("free_points", "bound_points", "design_buried_points", "free_area", "residue_buried"))
    kinds = np.array(c["kinds"])
    loops = np.isin(g_of, (1, 3)) & gen_rows.any(1)
    pushed, pulled = loops & (kinds == "pushed"), loops & (kinds == "pulled")
    assert (out["bsa_paratope"][pushed] > 0).all() and (out["bsa_design_epitope"][pushed] > 0).all() and (out["n_epitope_buried"][pushed] > 0).all()
    # the loop 30 A from everything buries nothing and loses nothing, exactly
    assert np.array_equal(out["bound_points"][pulled][gen_rows[pulled]], out["free_points"][pulled][gen_rows[pulled]])
    assert (out["design_buried_points"][pulled] == 0).all()
    for k in ("bsa_paratope", "bsa_design_epitope", "hotspot_buried_area"):
        assert (out[k][pulled] == 0).all(), k
    assert (out["n_paratope_buried"][pulled] == 0).all() and (out["n_epitope_buried"][pulled] == 0).all() and (out["n_hotspot_buried"][pulled] == 0).all()
    if K >= 70:
        assert pulled.any() and (N == 1 or pushed.any())


def test_more_context_atoms_than_two_chunks():
    """K = 90 residues with all A = 32 atoms present, two rows: about 2 400 context atoms in the patch, S = 64 (one full pass)."""
    K, A, N = 90, 32, 2
    roles = ("loop",)
    c = case(K, A, True, N, roles=roles)
    n_atoms = int(sum(bin(int(b)).count("1") for b in c["atom_bits"][0][~c["gen"][0] & c["rm"][0]]))
    assert n_atoms > 2 * 1024, n_atoms
    check(run(c, S=64), reference(K, A, True, N, S=64, roles=roles), f"surface K={K} A={A}, {n_atoms} context atoms")


def test_more_neighbours_than_a_wave_lists_at_once():
    """A 5 A probe on a dense patch: an atom has several hundred neighbours, more than twice the 256 a wave keeps on chip, so the list
    is emptied and refilled while one atom is scanned."""
    K, A, N = 70, 15, 1
    roles = ("loop",)
    c = case(K, A, True, N, roles=roles)
    xyz = c["xyz"][0][~c["gen"][0] & c["rm"][0]].reshape(-1, 3)
    near = int((np.linalg.norm(xyz[:, None] - xyz[None, :300], axis=-1) < 2 * 6.8).sum(0).max())  # (6.8 A = 1.8 + 5)
    assert near > 2 * 256, near
    check(run(c, S=33, probe=5.0), reference(K, A, True, N, S=33, probe=5.0, roles=roles), f"surface probe 5, up to {near} neighbours")


def test_more_generated_atoms_than_are_kept_on_chip():
    """K = 300 with the two antibody chains generated, 210 residues x 5 frame atoms = 1 050 atoms of the row: more than the 1 024 the
    rows kernel keeps in LDS, so it reads them from the caller's points instead.  One row; the antigen is chain 3."""
    K, A = 300, 8
    rng = np.random.default_rng(5)
    p = build_patch(rng, K, A, "none", False)
    gen = (p["chain_idx"] != 3)[None]
    assert gen.sum() * 5 > 1024
    antigen = ~gen
    seq, t, R = design_of(rng, dict(p, generation_mask=gen[0]), antigen[0], "noisy")
    des = {"seq_idx": cuda(seq[None]), "translations": cuda(t[None]), "orientations": cuda(R[None])}
    ctx = {"xyz": cuda(p["xyz"][None]), "atom_mask": cuda(p["atom_mask"][None])}
    out = numpy_of(metrics.surface(des, cuda(gen), context=ctx, antigen_mask=cuda(antigen), hotspot_mask=cuda(antigen)))
    pts, bits = design_points(des, ATOMS5)
    ref = surface_ref(pts, bits, RADII5, p["xyz"][None], (p["atom_mask"].astype(np.int64) << np.arange(A)).sum(-1)[None],
                      np.full((1, K, A), 1.8, np.float32), gen, np.ones((1, K), bool), metrics.sphere_points(96).numpy(), antigen=antigen, hotspot=antigen)
    check(out, ref, f"surface K={K}, {int(gen.sum()) * 5} atoms of the row")
    assert out["n_hotspot"][0] == antigen.sum() and out["bsa_paratope"][0] > 0


def test_other_atoms_radii_and_context_from_the_frames():
    """Four frame atoms with radii of the caller's, given by name; and context=None: the non-generated residues take the frame atoms of
    the first row of their group with the frame atoms' radii - the same call as passing those atoms as the context, to the bit."""
    K, A, N = 24, 8, 3
    c = case(K, A, False, N, True)
    four = ("N", "CA", "C", "O")
    radii = {"N": 1.5, "CA": 2.0, "C": 1.7, "O": 1.52, "CB": 9.0}
    out = run(c, atoms=four, atom_radius=radii, probe=1.2)
    pts, bits = design_points(c["designs"], four)
    table = metrics.sphere_points(96).numpy()
    ref = surface_ref(pts, bits, [radii[a] for a in four], c["xyz"], c["atom_bits"], c["radius"], c["gen"], c["rm"], table, antigen=c["antigen"],
                      hotspot=c["hotspot"], group_size=N, probe=1.2)
    check(out, ref, "surface, four atoms with other radii")
    out = run(c, context=None)
    pts, bits = design_points(c["designs"], ATOMS5)
    frame_radius = np.broadcast_to(np.asarray(RADII5, np.float32), (c["G"], K, 5))
    ref = surface_ref(pts, bits, RADII5, pts[::N], bits[::N], frame_radius, c["gen"], c["rm"], table, antigen=c["antigen"], hotspot=c["hotspot"],
                      group_size=N)
    check(out, ref, "surface, frame context")
    mask = ((bits[::N, :, None] >> np.arange(5)) & 1).astype(bool)
    explicit = {"xyz": cuda(pts[::N].copy()), "atom_mask": cuda(mask), "atom_radius": cuda(frame_radius)}
    again = run(c, context=explicit)
    for k, v in out.items():
        assert same_bits(v, again[k]), k


# ------------------------------------------------------------------ exact invariants
def test_free_points_without_an_antigen_mask():
    """Without antigen_mask every non-generated residue is framework.  So the call equals, to the bit, the one with a mask that flags
    nothing; its free points are the BOUND points of the flagged call (everything occludes) - and the flagged call's free points where
    the patch has no antigen flagged (the last patch).  (The free points of a generated residue are NOT the same with and without the
    antigen flagged, wherever the design touches the antigen: a flagged antigen does not occlude the antibody alone, an unflagged one
    does.  These are the exact statements the rule makes about the two calls.)"""
    N = 3
    c = case(70, 15, True, N)
    full = run(c)
    free = run(c, antigen_mask=None, hotspot_mask=None)
    assert set(free) == {"free_points", "free_area"}
    nothing = run(c, antigen_mask=torch.zeros_like(c["antigen_d"]), hotspot_mask=None)
    assert same_bits(free["free_points"], nothing["free_points"]) and same_bits(free["free_area"], nothing["free_area"])
    assert same_bits(nothing["bound_points"], nothing["free_points"]) and (nothing["design_buried_points"] == 0).all()
    g_of = np.arange(c["G"] * N) // N
    gen_rows = np.stack([c["gen"][g] & c["rm"][g] for g in g_of])
    assert gen_rows.any() and (free["free_points"][~gen_rows] == 0).all()
    assert same_bits(free["free_points"][gen_rows], full["bound_points"][gen_rows])
    assert same_bits(free["free_area"][gen_rows], full["bound_area"][gen_rows])
    assert not same_bits(full["free_points"][gen_rows], full["bound_points"][gen_rows])
    last = g_of == c["G"] - 1
    assert same_bits(free["free_points"][last], full["free_points"][last]) and free["free_points"][last].sum() > 0


def test_rows_alone_and_shared_contexts():
    """A row alone gives the bits it gives in a batch; N designs on one shared context equal the same designs on N replicated contexts."""
    K, A, N = 70, 8, 3
    c = case(K, A, False, N, True)
    full = run(c)
    assert full["design_buried_points"].sum() > 0
    rep = lambda t: t.repeat_interleave(N, 0).contiguous()
    each = numpy_of(metrics.surface(c["designs"], rep(c["gen_d"]), context={k: rep(v) for k, v in c["context"].items()}, antigen_mask=rep(c["antigen_d"]),
                                    hotspot_mask=rep(c["hotspot_d"]), residue_mask=rep(c["rm_d"]), group_size=1))
    for k, v in each.items():
        assert same_bits(v, full[k]), k
    for r in (4, 3 * N + 1, 4 * N + 2):  # a loop row of patches 1, 3 and 4
        g = r // N
        one = numpy_of(metrics.surface({k: v[r:r + 1] for k, v in c["designs"].items()}, c["gen_d"][g:g + 1], context={k: v[g:g + 1] for k, v in c["context"].items()},
                                       antigen_mask=c["antigen_d"][g:g + 1], hotspot_mask=c["hotspot_d"][g:g + 1], residue_mask=c["rm_d"][g:g + 1]))
        for k, v in one.items():
            assert same_bits(v, full[k][r:r + 1]), (r, k)


# ------------------------------------------------------------------ the contracts of the C ABI, for this entry
@pytest.mark.parametrize("fill", ["zero", "ff", "random"])
def test_workspace_and_output_contents_on_entry_do_not_matter(fill):
    """The workspace poisoned behind guard bytes, and every output buffer poisoned before the call: identical bits, intact guards."""
    K, A, N = 70, 8, 3
    c = case(K, A, False, N, True)
    clean = run(c, S=130)
    with poisoned(fill, seed=3) as p:
        dirty = run(c, S=130)
        assert len(p.bases) == 1 and p.bases[0][1] == metrics.surface_workspace_bytes(c["G"], K, A, 130)
    for k, v in clean.items():
        assert same_bits(v, dirty[k]), (fill, k)
    with poisoned(fill, seed=4):  # without an antigen the second launch is not made: the masks stay as they were filled
        lone = run(c, antigen_mask=None, hotspot_mask=None)
    assert same_bits(lone["free_points"], run(c, antigen_mask=None, hotspot_mask=None)["free_points"])


@pytest.mark.parametrize("off", [4, 12])
def test_operands_need_their_natural_alignment_only(off):
    """Every data operand ACCEPTED: the oracle-equality case again with every device pointer replaced by one that is only 4-byte
    (float32: `off` bytes behind a 16-byte boundary), or 1-byte (masks), aligned."""
    K, A, dense, N, S = 70, 8, False, 3, 96
    c = case(K, A, dense, N, True)
    with MisalignedABI(("diffab_metrics_surface",), f32=off) as abi:
        out = run(c, S)
    assert abi.counts["diffab_metrics_surface"] > 0
    check(out, reference(K, A, dense, N, True, S), f"surface, operands {off} bytes off")
    aligned = run(c, S)
    for k, v in aligned.items():
        assert same_bits(v, out[k]), k
