"""Developability on the MI355X: metrics.patches / diffab_metrics_patches and metrics.liabilities /
diffab_metrics_motifs against the numpy restatements of developability_ref.py, their properties and their contracts.

Integers, states and the two charges are compared for exact equality: every decision is one fp32 comparison of a defined number, and
the charge tables of these tests hold 0 or fp32 values of magnitude in [2^-4, 4], so every fp64 partial sum of at most 512 of them is
exact whatever the order.  psh, ppc, pnc and the three per-residue sums are compared within ONE fp32 ulp of the float64 restatement
rounded to fp32: every term of a sum has the same sign (no cancellation), an fp64 sum of at most 131 072 terms carries a relative
error below 2e-11, far inside half an fp32 ulp, so the two roundings can differ only across a rounding boundary.  The restatement runs
on the SAME fp32 sites the kernel reads (the frame kernel's CA and CB, the patch's xyz)."""
import functools

import numpy as np
import pytest
import torch

import sampler_support
from developability_ref import EXPOSED, PRESENT, SCOPE, motifs_ref, patches_ref, same_bits, ulps_apart
from test_geometry_host import tangle_chain_keys
from diffab_pytorch import _hip, io as dio, metrics
from sampler_support import GuardedABI, header_prototypes, hip, misaligned
from scratch_poison import poisoned

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("hip")]

GLY, UNK = metrics.GLY, 20
f32 = np.float32
cuda = lambda v: torch.from_numpy(np.ascontiguousarray(v)).cuda()
numpy_of = lambda out: {k: v.cpu().numpy() for k, v in out.items()}
A = 7  # atom slots of the patches' real atoms
# 20 classes, so token 20 (UNK) lies outside the tables and weighs nothing.  The charges are 0 or of magnitude in [2^-4, 4].
HYDROPHOBICITY = tuple(metrics.KYTE_DOOLITTLE[:20])
# (Many classes carry a charge here, so that pairs of two positive and of two negative residues are common at every size.)
CHARGE = tuple({"A": 0.5, "R": 1.0, "N": -0.5, "D": -1.0, "C": -4.0, "Q": 0.25, "E": -1.0, "H": 0.125, "L": 2.0, "K": 1.0, "M": -2.0, "P": -0.25,
                "S": 0.0625, "T": -0.125, "W": 4.0, "Y": -0.0625}.get(c, 0.0) for c in dio.AA1[:20])
EXACT = ("n_neighbours", "state", "n_scope", "n_exposed", "n_pairs", "charge_generated", "charge_scope")
WITHIN_ONE_ULP = ("psh", "ppc", "pnc", "residue_psh", "residue_ppc", "residue_pnc")
OUTPUTS = ("psh", "ppc", "pnc", "charge_generated", "charge_scope", "n_scope", "n_exposed", "n_pairs", "residue_psh", "residue_ppc", "residue_pnc",
           "n_neighbours", "state")
SHAPES = [(K, N) for K in (5, 33, 63, 64, 65, 130) for N in (1, 3)] + [(33, 65)]  # (33, 65): one patch, 65 rows in the group


def rotations(rng, n):
    q, _ = np.linalg.qr(rng.normal(size=(n, 3, 3)))
    return q * np.sign(np.linalg.det(q))[:, None, None]


# ------------------------------------------------------------------ inputs
@functools.lru_cache(maxsize=None)
def case(K, N, seed=0):
    """G patches (2; 1 where N = 65) x N designs of K residues, uniform in a cube of edge (135 K)^(1/3) A - about a protein's density.
    A contiguous quarter of the slots is generated (it starts at K // 5), the last third is flagged as antigen.  The generated residues
    of every design are moved by about 1.5 A and redrawn; a fifth of them is Gly, a few tokens are UNK.  One non-generated residue lies
    outside residue_mask, and in the patch's real atoms one non-generated residue has no CA (it is absent), a few have no CB and one is
    Gly (their site is the CA)."""
    rng = np.random.default_rng(1000 * K + N + seed)
    G = 1 if N > 8 else 2
    edge = (135.0 * K) ** (1.0 / 3.0)
    n_gen, n_ag = max(1, K // 4), K // 3
    gen = np.zeros((G, K), bool)
    gen[:, K // 5:K // 5 + n_gen] = True
    antigen = np.zeros((G, K), bool)
    antigen[:, K - n_ag:] = True
    assert not (gen & antigen).any()
    free = np.flatnonzero(~gen[0] & ~antigen[0])
    rm = np.ones((G, K), bool)
    t0 = rng.uniform(0.0, edge, (G, K, 3))
    R0 = rotations(rng, G * K).reshape(G, K, 3, 3)
    seq0 = rng.integers(0, 20, (G, K))
    seq0[seq0 == GLY] = 0
    am = np.ones((G, K, A), bool)
    am[:, :, 4] = rng.random((G, K)) < 0.8
    am[:, :, 5:] = rng.random((G, K, 2)) < 0.5
    if len(free) >= 3:
        rm[:, free[0]] = False
        am[:, free[1], 1] = False  # no CA: absent
        seq0[:, free[2]] = GLY
        am[:, free[2], 4] = True  # (a Gly with a "CB" in the mask still takes its CA)
    seq, tt, RR = [], [], []
    for g in range(G):
        for r in range(N):
            s, x, O = seq0[g].copy(), t0[g].copy(), R0[g].copy()
            n = int(gen[g].sum())
            x[gen[g]] += rng.normal(0.0, 1.5, (n, 3))
            O[gen[g]] = rotations(rng, n)
            s[gen[g]] = np.where(rng.random(n) < 0.2, GLY, rng.integers(0, 20, n))
            s[rng.random(K) < 0.04] = UNK
            s[~gen[g]] = np.where(s[~gen[g]] == UNK, UNK, seq0[g][~gen[g]])  # (the context keeps its tokens, but for the UNKs)
            seq.append(s), tt.append(x.astype(f32)), RR.append(O.astype(f32))
    designs = {"seq_idx": cuda(np.stack(seq)), "translations": cuda(np.stack(tt)), "orientations": cuda(np.stack(RR))}
    frame_atoms = dio.backbone_from_frames(torch.from_numpy(t0.astype(f32)), torch.from_numpy(R0.astype(f32)), dio.BACKBONE_ATOMS).numpy()
    xyz = np.zeros((G, K, A, 3), f32)
    xyz[:, :, :5] = frame_atoms
    xyz[:, :, 5:] = frame_atoms[:, :, 4:5] + rng.normal(0.0, 1.4, (G, K, A - 5, 3)).astype(f32)
    return dict(G=G, N=N, K=K, gen=gen, antigen=antigen, rm=rm, xyz=xyz, am=am, designs=designs, gen_d=cuda(gen), rm_d=cuda(rm),
                antigen_d=cuda(antigen), context={"xyz": cuda(xyz), "atom_mask": cuda(am)})


def sites_of(designs):
    """The fp32 sites the kernel reads, as numpy: CB of every row's frames through the frame kernel, CA where the token is Gly."""
    frame = dio.backbone_from_frames(designs["translations"], designs["orientations"], ("CA", "CB")).float().cpu().numpy()
    gly = designs["seq_idx"].cpu().numpy() == GLY
    return np.where(gly[:, :, None], frame[:, :, 0], frame[:, :, 1])


def inputs_of(c, context, antigen, designs=None, xyz=None):
    """(sites, context_sites, tokens, rm, antigen) as the rule of metrics.patches builds them, restated in numpy."""
    designs = c["designs"] if designs is None else designs
    xyz = c["xyz"] if xyz is None else xyz
    N = c["N"]
    sites, tokens = sites_of(designs), designs["seq_idx"].cpu().numpy()
    rm = c["rm"]
    if context:
        use_cb = c["am"][:, :, 4] & (tokens[::N] != GLY)
        csites = np.where(use_cb[:, :, None], xyz[:, :, 4], xyz[:, :, 1])
        rm = rm & (c["am"][:, :, 1] | c["gen"])
    else:
        csites = sites[::N]
    return sites, csites, tokens, rm, (c["antigen"] if antigen else None)


def defaults(**kw):
    return dict(dict(hydrophobicity=HYDROPHOBICITY, charge=CHARGE, neighbour_distance=10.0, vicinity_distance=10.0, patch_distance=7.5,
                     min_distance=3.8), **kw)


@functools.lru_cache(maxsize=None)
def reference(K, N, context, antigen, vicinity=10.0):
    """The restatement with max_neighbours = the median of its own counts over the residues in scope -> (dict, max_neighbours)."""
    c = case(K, N)
    sites, csites, tokens, rm, ag = inputs_of(c, context, antigen)
    kw = defaults(group_size=N, vicinity_distance=vicinity)
    first = patches_ref(sites, csites, tokens, c["gen"], rm, ag, max_neighbours=10 ** 6, **kw)
    scope = (first["state"] & SCOPE) != 0
    limit = int(np.median(first["n_neighbours"][scope]))
    return patches_ref(sites, csites, tokens, c["gen"], rm, ag, max_neighbours=limit, **kw), limit


def device_call(c, context, antigen, **kw):
    return metrics.patches(c["designs"], c["gen_d"], context=c["context"] if context else None, antigen_mask=c["antigen_d"] if antigen else None,
                           residue_mask=c["rm_d"], group_size=c["N"], **defaults(**kw))


@functools.lru_cache(maxsize=None)
def device_patches(K, N, context, antigen):
    return numpy_of(device_call(case(K, N), context, antigen, max_neighbours=reference(K, N, context, antigen)[1]))


def check_patches(out, want, what, only=OUTPUTS):
    assert set(out) == set(only), (what, set(out) ^ set(only))
    for k in out:
        assert out[k].dtype == want[k].dtype and out[k].shape == want[k].shape, (what, k, out[k].dtype, out[k].shape)
        if k in EXACT:
            bad = np.argwhere(out[k] != want[k])
            assert len(bad) == 0, (what, k, "first differing elements:", bad[:5].tolist())
        else:
            far = ulps_apart(out[k], want[k])
            print(f"{what}: {k} at most {int(far.max()) if far.size else 0} ulp from the restatement")
            assert np.isfinite(out[k]).all() and (far <= 1).all(), (what, k, int(far.max()), np.argwhere(far > 1)[:5].tolist())


# ------------------------------------------------------------------ patches against the restatement
@pytest.mark.parametrize("antigen", [True, False], ids=["antigen", "no_antigen"])
@pytest.mark.parametrize("context", [True, False], ids=["context", "frames"])
@pytest.mark.parametrize("K, N", SHAPES)
def test_patches_equal_the_restatement(K, N, context, antigen):
    c = case(K, N)
    want, limit = reference(K, N, context, antigen)
    state = want["state"]
    # ---- what the inputs must contain
    scope, exposed = (state & SCOPE) != 0, (state & EXPOSED) != 0
    if K >= 33:
        assert want["n_pairs"].max() >= 5 and want["n_pairs"].min() >= 1 and (scope & ~exposed).sum(1).min() >= 5, (
            want["n_pairs"].tolist(), (scope & ~exposed).sum(1).tolist())
        assert (want["psh"] > 0).all() and (want["ppc"] > 0).any() and (want["pnc"] > 0).any()
        tokens = c["designs"]["seq_idx"].cpu().numpy()
        assert (tokens == UNK).any() and (tokens[:, c["gen"][0]] == GLY).any()
        assert ((state & PRESENT) == 0).any() and (exposed & ~np.repeat(c["gen"], N, 0)).any()  # an exposed residue of the framework
        if context:
            assert (~c["am"][:, :, 1]).any() and (~c["am"][:, :, 4] & ~c["gen"]).any()
    if antigen:
        assert (state[:, K - K // 3:] == 0).all()
    # ---- the device
    check_patches(device_patches(K, N, context, antigen), want, f"patches K={K} N={N} context={context} antigen={antigen} max_neighbours={limit}")


def test_a_smaller_vicinity_leaves_present_residues_out_of_scope():
    K, N = 65, 3
    want, limit = reference(K, N, True, True, vicinity=6.0)
    state = want["state"]
    assert (state == PRESENT).sum(1).min() >= 1 and ((state & SCOPE) != 0).sum(1).min() > K // 4  # present, out of scope; the CDR and more
    out = numpy_of(device_call(case(K, N), True, True, max_neighbours=limit, vicinity_distance=6.0))
    check_patches(out, want, "vicinity_distance=6.0")


def test_the_default_tables_and_a_caller_s_threshold():
    """The defaults of metrics.patches (21 classes, H = +0.1: the charges are then within one ulp, not exact) and no residue_mask."""
    K, N = 64, 3
    c = case(K, N)
    sites, csites, tokens, _, ag = inputs_of(c, False, True)
    want = patches_ref(sites, csites, tokens, c["gen"], None, ag, group_size=N, hydrophobicity=np.array(metrics.KYTE_DOOLITTLE, f32),
                       charge=np.array(metrics.RESIDUE_CHARGE, f32), max_neighbours=16)
    out = numpy_of(metrics.patches(c["designs"], c["gen_d"], antigen_mask=c["antigen_d"], group_size=N))
    assert 0 < want["n_exposed"].min() and want["n_pairs"].max() > 0
    for k in OUTPUTS:
        if k in EXACT[:5]:
            assert np.array_equal(out[k], want[k]), k
        else:
            assert (ulps_apart(out[k], want[k]) <= 1).all(), k


# ------------------------------------------------------------------ properties
def test_a_zero_hydrophobicity_table_gives_no_psh_and_the_same_states():
    K, N = 65, 3
    base, limit = device_patches(K, N, True, True), reference(K, N, True, True)[1]
    out = numpy_of(device_call(case(K, N), True, True, max_neighbours=limit, hydrophobicity=(0.0,) * 20))
    assert (out["psh"] == 0).all() and (out["residue_psh"] == 0).all() and base["psh"].min() > 0
    for k in OUTPUTS:
        if not k.endswith("psh"):
            assert same_bits(out[k], base[k]), k


def test_sites_that_are_never_read_may_hold_anything():
    """NaN in the row's sites of non-generated residues, NaN in the patch's sites of generated residues and an antigen moved by 100 A
    change no output bit."""
    K, N = 65, 3
    c = case(K, N)
    base, limit = device_patches(K, N, True, True), reference(K, N, True, True)[1]
    gen_rows = np.repeat(c["gen"], N, 0)
    t = c["designs"]["translations"].cpu().numpy().copy()
    t[~gen_rows] = np.nan
    rows_poisoned = dict(c["designs"], translations=cuda(t))
    xyz = c["xyz"].copy()
    xyz[c["gen"]] = np.nan
    xyz[c["antigen"]] += f32(100.0)
    ctx_poisoned = {"xyz": cuda(xyz), "atom_mask": c["context"]["atom_mask"]}
    kw = dict(antigen_mask=c["antigen_d"], residue_mask=c["rm_d"], group_size=N, **defaults(max_neighbours=limit))
    for what, designs, context in (("row sites", rows_poisoned, c["context"]), ("context sites", c["designs"], ctx_poisoned),
                                   ("both", rows_poisoned, ctx_poisoned)):
        out = numpy_of(metrics.patches(designs, c["gen_d"], context=context, **kw))
        for k in OUTPUTS:
            assert same_bits(out[k], base[k]), (what, k)
    assert np.isnan(sites_of(rows_poisoned)[~gen_rows]).all() and (base["state"] & EXPOSED).any()


def test_exposed_in_equal_to_the_call_s_own_states_reproduces_the_call():
    K, N = 130, 3
    c = case(K, N)
    base, limit = device_patches(K, N, False, True), reference(K, N, False, True)[1]
    own = cuda((base["state"] & EXPOSED) != 0)
    again = numpy_of(device_call(c, False, True, max_neighbours=0, exposed=own))  # (the threshold no longer decides)
    for k in OUTPUTS:
        assert same_bits(again[k], base[k]), k
    # and another choice is taken as given: nobody exposed, everybody in scope exposed
    none = numpy_of(device_call(c, False, True, max_neighbours=limit, exposed=torch.zeros_like(own)))
    assert (none["n_exposed"] == 0).all() and (none["psh"] == 0).all() and same_bits(none["n_neighbours"], base["n_neighbours"])
    every = numpy_of(device_call(c, False, True, max_neighbours=limit, exposed=torch.ones_like(own)))
    assert np.array_equal(every["n_exposed"], base["n_scope"]) and np.array_equal((every["state"] & EXPOSED) != 0, (base["state"] & SCOPE) != 0)
    sites, csites, tokens, rm, ag = inputs_of(c, False, True)
    want = patches_ref(sites, csites, tokens, c["gen"], rm, ag, np.ones_like(base["state"], bool), **defaults(group_size=N, max_neighbours=limit))
    check_patches(every, want, "every residue in scope exposed")


def test_one_residue_and_a_row_without_a_generated_residue_give_zeros():
    one = {"seq_idx": torch.ones(2, 1, dtype=torch.long).cuda(), "translations": torch.zeros(2, 1, 3).cuda(),
           "orientations": torch.eye(3).expand(2, 1, 3, 3).contiguous().cuda()}
    out = numpy_of(metrics.patches(one, torch.ones(2, 1, dtype=torch.bool).cuda(), hydrophobicity=HYDROPHOBICITY, charge=CHARGE))
    assert (out["state"] == PRESENT | SCOPE | EXPOSED).all() and (out["n_exposed"] == 1).all() and (out["charge_generated"] == 1).all()
    for k in ("psh", "ppc", "pnc", "n_pairs", "residue_psh", "residue_ppc", "residue_pnc", "n_neighbours"):
        assert (out[k] == 0).all(), k
    c = case(33, 3)
    gen = c["gen"].copy()
    gen[0] = False  # patch 0 generates nothing: nothing is in scope
    out = numpy_of(metrics.patches(c["designs"], cuda(gen), group_size=3, **defaults(max_neighbours=16)))
    for k in OUTPUTS:
        if k not in ("n_neighbours", "state"):
            assert (out[k][:3] == 0).all() and out[k].dtype == device_patches(33, 3, False, False)[k].dtype, k
    assert (out["state"][:3] == PRESENT).all() and out["n_neighbours"][:3].max() > 0 and (out["n_scope"][3:] > 0).all()


@pytest.mark.parametrize("context", [True, False], ids=["context", "frames"])
def test_a_patch_alone_gives_the_bits_it_gives_in_a_batch(context):
    K, N = 65, 3
    c, both, limit = case(K, N), device_patches(K, N, context, True), reference(K, N, context, True)[1]
    for g in range(2):
        rows = slice(g * N, (g + 1) * N)
        alone = metrics.patches({k: v[rows] for k, v in c["designs"].items()}, c["gen_d"][g:g + 1],
                                context={k: v[g:g + 1] for k, v in c["context"].items()} if context else None,
                                antigen_mask=c["antigen_d"][g:g + 1], residue_mask=c["rm_d"][g:g + 1], group_size=N, **defaults(max_neighbours=limit))
        for k in OUTPUTS:
            assert same_bits(alone[k].cpu().numpy(), both[k][rows]), (g, k)
    m = motif_case(65, 3)
    for g in range(2):
        rows = slice(g * N, (g + 1) * N)
        alone = numpy_of(metrics.liabilities({k: v[rows] for k, v in m["designs"].items()}, m["gen_d"][g:g + 1], chain_idx=m["chain_d"][g:g + 1],
                                             residue_idx=m["ridx_d"][g:g + 1], residue_mask=m["rm_d"][g:g + 1], group_size=N))
        for k, v in device_motifs(65, 3).items():
            assert same_bits(alone[k], v[rows]), (g, k)


# ------------------------------------------------------------------ motifs
# (K, N) -> per patch, the first of 13 slots of the second chain that take the keys of test_geometry_host.tangle_chain_keys, slot 0 with
# them: a 32-bit gap, the highest slot, a masked slot or another chain would give other successors.  The slots are generated and hold
# D P, N A . G, D G and G N A along the right and the wrong successors, so each wrong rule counts another number of motifs.
TANGLED = {(65, 2): (36, 37)}


@functools.lru_cache(maxsize=None)
def motif_case(K, N, seed=0):
    """G = 2 patches x N designs of random tokens 0..20 (and a token of 32 and a negative one where there is room).  Two chains with a gap
    in residue_idx inside the first, and the last two slots of the first chain swapped, so chain neighbours are not always adjacent
    slots; one slot of the second chain lies outside residue_mask.  A contiguous quarter is generated.  With K >= 33 the stretch
    C M N G S D S D P is planted at the start of the generated residues of every row - every default motif once, the last one (D P)
    straddling the segment's end at K = 33 - and the sequon N K T once more wholly outside them."""
    rng = np.random.default_rng(77 * K + N + seed)
    G = 1 if N > 8 else 2
    gen = np.zeros((G, K), bool)
    lo, n_gen = K // 5, max(1, K // 4)
    gen[:, lo:lo + n_gen] = True
    half = (K + 1) // 2
    chain = np.broadcast_to((np.arange(K) >= half).astype(np.int64), (G, K)).copy()
    ridx = np.broadcast_to(np.arange(K) + 5 * (np.arange(K) >= 3) + 100 * (np.arange(K) >= half), (G, K)).copy()
    rm = np.ones((G, K), bool)
    tokens = rng.integers(0, 21, (G * N, K))
    if K >= 33:
        planted = "CMNGSDSDP"
        assert lo >= 6 and n_gen >= len(planted) - 1 and lo + len(planted) <= half - 2 and half + 3 < K - 4
        ridx[:, [half - 1, half - 2]] = ridx[:, [half - 2, half - 1]]  # slots out of chain order (behind the planted stretch)
        rm[:, half + 1] = False
        tokens[:, half + 2], tokens[:, half + 3] = 32, -3
        tokens[:, lo:lo + len(planted)] = [dio.AA1.index(ch) for ch in planted]
        tokens[:, K - 4:K - 1] = [dio.AA1.index(ch) for ch in "NKT"]  # outside the generated residues: matched, not counted
    for g, at in enumerate(TANGLED.get((K, N), ())):
        chain, ridx = chain.astype(np.int32), ridx.astype(np.int32)
        tangle_chain_keys(chain[g], ridx[g], rm[g], at, 0)
        gen[g, at:at + 13] = gen[g, 0] = True
        for slot, ch in zip([0, at, at + 1, at + 2, at + 4, at + 8, at + 9, at + 7, at + 10, at + 11, at + 12], "DPNAGDGGGNA"):
            tokens[g * N:(g + 1) * N, slot] = dio.AA1.index(ch)
    designs = {"seq_idx": cuda(tokens), "translations": cuda(np.zeros((G * N, K, 3), f32))}
    return dict(G=G, N=N, K=K, gen=gen, rm=rm, chain=chain, ridx=ridx, tokens=tokens, designs=designs, gen_d=cuda(gen), rm_d=cuda(rm),
                chain_d=cuda(chain), ridx_d=cuda(ridx))


MOTIF_WORDS = metrics.motif_masks(metrics.LIABILITY_MOTIFS).numpy()


@functools.lru_cache(maxsize=None)
def motif_reference(K, N):
    m = motif_case(K, N)
    return motifs_ref(m["tokens"], m["gen"], m["rm"], m["chain"], m["ridx"], MOTIF_WORDS, N)


@functools.lru_cache(maxsize=None)
def device_motifs(K, N):
    m = motif_case(K, N)
    return numpy_of(metrics.liabilities(m["designs"], m["gen_d"], chain_idx=m["chain_d"], residue_idx=m["ridx_d"], residue_mask=m["rm_d"], group_size=N))


def check_motifs(out, want, names, what):
    """out: metrics.liabilities' dict (names: its motif names in order), or some of the three raw outputs (names: None)."""
    if names is not None:
        assert list(out) == list(names) + ["n_motifs", "motif_start"], (what, list(out))
        out = {"motif_count": np.stack([out[n] for n in names], 1), "n_motifs": out["n_motifs"], "motif_start": out["motif_start"]}
    for k in out:
        assert out[k].dtype == np.int32 and out[k].shape == want[k].shape, (what, k)
        bad = np.argwhere(out[k] != want[k])
        assert len(bad) == 0, (what, k, "first differing elements:", bad[:5].tolist())


@pytest.mark.parametrize("K, N", SHAPES + [(70, 3), (300, 3)] + list(TANGLED))  # (successors past the 64 threads of their kernel, ragged and not)
def test_liabilities_equal_the_restatement(K, N):
    m, want = motif_case(K, N), motif_reference(K, N)
    if K >= 33:  # what the inputs must contain
        assert (want["motif_count"] >= 1).all(), want["motif_count"].min(0)  # every default motif is counted in every row
        every = motifs_ref(m["tokens"], m["gen"], m["rm"], m["chain"], m["ridx"], MOTIF_WORDS, N, counted_only=False)
        assert (every["motif_count"][:, 0] > want["motif_count"][:, 0]).all()  # a sequon outside the generated residues
        assert (m["tokens"] >= 32).any() and (m["tokens"] < 0).any() and not m["rm"].all()
        assert (np.diff(m["ridx"][0]) < 0).any() and (np.diff(m["ridx"][0]) > 1).any() and len(set(m["chain"][0])) == 2
    check_motifs(device_motifs(K, N), want, list(metrics.LIABILITY_MOTIFS), f"liabilities K={K} N={N}")


def test_thirty_two_motifs_and_the_sign_bit():
    K, N = 65, 3
    m = motif_case(K, N)
    patterns = {f"m{i}": dio.AA1[i % 20] + ("" if i % 3 else ".") + ("[^P]" if i % 5 == 0 else "") for i in range(31)}
    patterns["last"] = "."
    words = metrics.motif_masks(patterns).numpy()
    want = motifs_ref(m["tokens"], m["gen"], None, m["chain"], m["ridx"], words, N)
    assert (want["motif_start"] < 0).any() and (want["motif_count"][:, 31] == m["gen"].sum(1)[0]).all()
    assert (want["motif_count"] > 0).any(0).sum() >= 16 and len({len(p) for p in patterns.values()}) >= 3  # many motifs hit, several lengths
    out = numpy_of(metrics.liabilities(m["designs"], m["gen_d"], motifs=patterns, chain_idx=m["chain_d"], residue_idx=m["ridx_d"], group_size=N))
    check_motifs(out, want, list(patterns), "32 motifs")
    # V = 32 classes and the raw words: every class, the sign bit = class 31
    tokens = m["tokens"].copy()
    tokens[:, ::7] = 31
    designs = dict(m["designs"], seq_idx=cuda(tokens))
    want = motifs_ref(tokens, m["gen"], m["rm"], m["chain"], m["ridx"], metrics.motif_masks({"x": "..", "y": "[^A]"}, V=32).numpy(), N)
    out = numpy_of(metrics.liabilities(designs, m["gen_d"], motifs={"x": "..", "y": "[^A]"}, V=32, chain_idx=m["chain_d"], residue_idx=m["ridx_d"],
                                       residue_mask=m["rm_d"], group_size=N))
    check_motifs(out, want, ["x", "y"], "V = 32")
    assert (want["motif_count"] > 0).all()


# ------------------------------------------------------------------ the C ABI directly
DEVELOP_ARGTYPES = {n: a for n, (_, a) in _hip.DEVELOP_SYMBOLS.items()}
DEVELOP_WRITES = {"diffab_metrics_patches": " ".join(OUTPUTS) + " workspace", "diffab_metrics_motifs": "motif_count n_motifs motif_start workspace"}
MOTIFS_HOST_ARGUMENT = 5  # `motifs` is a host array: the guarded ABI passes it as it is


def place(t, shifted):
    """The tensor itself, or a copy that starts 4 bytes (1 byte for masks) behind a 16-byte boundary: the natural alignment only."""
    return misaligned(t, 4 if t.element_size() >= 4 else 1) if shifted else t


def raw_patches(K, N, context, antigen, skip=(), shifted=False):
    """diffab_metrics_patches on the operands metrics.patches would build, through whatever stands in for _hip.lib()."""
    c, limit = case(K, N), reference(K, N, context, antigen)[1]
    sites, csites, tokens, rm, ag = inputs_of(c, context, antigen)
    ops = [cuda(sites.astype(f32)), cuda(csites.astype(f32)), cuda(tokens.astype(np.int32)), cuda(c["gen"]), cuda(rm), None if ag is None else cuda(ag),
           None, cuda(np.array(HYDROPHOBICITY, f32)), cuda(np.array(CHARGE, f32))]
    ops = [None if t is None else place(t, shifted) for t in ops]
    rows = c["G"] * N
    kinds = {k: torch.float32 for k in OUTPUTS}
    kinds.update(n_scope=torch.int32, n_exposed=torch.int32, n_pairs=torch.int32, n_neighbours=torch.int32, state=torch.uint8)
    per_residue = ("residue_psh", "residue_ppc", "residue_pnc", "n_neighbours", "state")
    out = {k: place(torch.empty((rows, K) if k in per_residue else (rows,), dtype=kinds[k], device="cuda"), shifted) for k in OUTPUTS if k not in skip}
    nbytes = metrics.patches_workspace_bytes(c["G"], K)
    ws = _hip.workspace(nbytes)
    lib = _hip.lib()
    rc = lib.diffab_metrics_patches(*[_hip.ptr(t) for t in ops], rows, N, K, 20, 10.0, limit, 10.0, 7.5, 3.8, *[_hip.ptr(out.get(k)) for k in OUTPUTS],
                                    _hip.ptr(ws), nbytes, _hip.stream_ptr())
    assert rc == 0, _hip.load_library().diffab_last_error().decode()
    torch.cuda.synchronize()
    return numpy_of(out)


def raw_motifs(K, N, skip=(), shifted=False):
    import ctypes

    m = motif_case(K, N)
    ops = [cuda(m["tokens"].astype(np.int32)), cuda(m["gen"]), cuda(m["rm"]), cuda(m["chain"].astype(np.int32)), cuda(m["ridx"].astype(np.int32))]
    ops = [place(t, shifted) for t in ops]
    rows, M = m["G"] * N, len(MOTIF_WORDS)
    shapes = {"motif_count": (rows, M), "n_motifs": (rows,), "motif_start": (rows, K)}
    out = {k: place(torch.empty(s, dtype=torch.int32, device="cuda"), shifted) for k, s in shapes.items() if k not in skip}
    host = (ctypes.c_int32 * (M * 4))(*MOTIF_WORDS.flatten().tolist())
    nbytes = metrics.motifs_workspace_bytes(m["G"], K)
    ws = _hip.workspace(nbytes)
    lib = _hip.lib()
    rc = lib.diffab_metrics_motifs(*[_hip.ptr(t) for t in ops], ctypes.cast(host, ctypes.c_void_p), rows, N, K, M, *[_hip.ptr(out.get(k)) for k in shapes],
                                   _hip.ptr(ws), nbytes, _hip.stream_ptr())
    assert rc == 0, _hip.load_library().diffab_last_error().decode()
    torch.cuda.synchronize()
    return numpy_of(out)


@pytest.mark.parametrize("skip", [("psh",), ("state", "n_neighbours"), ("residue_psh", "residue_ppc", "residue_pnc"),
                                  ("ppc", "pnc", "charge_generated", "charge_scope", "n_scope", "n_exposed", "n_pairs"), OUTPUTS])
def test_null_outputs_are_skipped_and_the_others_unchanged(skip):
    K, N = 65, 3
    out = raw_patches(K, N, True, True, skip=skip)
    full = device_patches(K, N, True, True)
    assert set(out) == set(OUTPUTS) - set(skip)
    for k in out:
        assert same_bits(out[k], full[k]), (skip, k)
    for drop in (("motif_count",), ("n_motifs", "motif_start"), ("motif_count", "n_motifs", "motif_start")):
        out = raw_motifs(K, N, skip=drop)
        assert set(out) == {"motif_count", "n_motifs", "motif_start"} - set(drop)
        check_motifs(out, {k: motif_reference(K, N)[k] for k in out}, None, f"motifs without {drop}")


# ------------------------------------------------------------------ contracts
@pytest.mark.parametrize("fill", ["ff", "random"])
def test_what_the_workspace_and_the_outputs_held_is_ignored(fill):
    with poisoned(fill, seed=5):
        for K, N, context, antigen in ((33, 3, True, True), (65, 3, False, True), (130, 1, True, False), (5, 1, True, True)):
            c, (want, limit) = case(K, N), reference(K, N, context, antigen)
            check_patches(numpy_of(device_call(c, context, antigen, max_neighbours=limit)), want, f"patches K={K} under {fill}")
        check_patches(raw_patches(65, 3, True, True, skip=OUTPUTS[5:]), reference(65, 3, True, True)[0], f"five outputs under {fill}", only=OUTPUTS[:5])
        for K, N in ((33, 3), (65, 3), (130, 1), (5, 1)):
            m = motif_case(K, N)
            out = metrics.liabilities(m["designs"], m["gen_d"], chain_idx=m["chain_d"], residue_idx=m["ridx_d"], residue_mask=m["rm_d"], group_size=N)
            check_motifs(numpy_of(out), motif_reference(K, N), list(metrics.LIABILITY_MOTIFS), f"liabilities K={K} under {fill}")


@pytest.mark.parametrize("fill", sampler_support.GUARD_FILLS)
def test_outputs_between_guards_with_operands_at_their_natural_alignment(fill, monkeypatch):
    for entry, writes in DEVELOP_WRITES.items():
        monkeypatch.setitem(sampler_support.WRITES, entry, writes)
    params = {n: [p[0] for p in ps] for n, ps in header_prototypes(("diffab_hip_develop.h",))[1].items()}
    assert set(params) == set(DEVELOP_ARGTYPES) and params["diffab_metrics_motifs"][MOTIFS_HOST_ARGUMENT] == "motifs"
    positions = {"diffab_metrics_motifs": set(range(len(params["diffab_metrics_motifs"]))) - {MOTIFS_HOST_ARGUMENT}}
    with GuardedABI(tuple(DEVELOP_ARGTYPES), fill, argtypes=DEVELOP_ARGTYPES, positions=positions) as abi:
        abi.params.update(params)
        for K, N, context, antigen in ((33, 3, True, True), (65, 3, False, True), (64, 1, True, False), (130, 3, True, True)):
            check_patches(raw_patches(K, N, context, antigen, shifted=True), reference(K, N, context, antigen)[0], f"K={K} N={N} guarded [{fill}]")
        check_patches(raw_patches(65, 3, True, True, skip=OUTPUTS[:8], shifted=True), reference(65, 3, True, True)[0], "guarded, per residue",
                      only=OUTPUTS[8:])
        for K, N in ((33, 3), (65, 3), (64, 1), (130, 3)):
            check_motifs(raw_motifs(K, N, shifted=True), motif_reference(K, N), None, f"motifs K={K} N={N} guarded [{fill}]")
    assert abi.counts["diffab_metrics_patches"] >= 4 * 20 and abi.counts["diffab_metrics_motifs"] >= 4 * 8


# ------------------------------------------------------------------ end to end
def test_sampled_designs_through_patches_and_liabilities_into_pareto():
    """sample(num_samples = 16) of the unit model at K = 64 -> patches and liabilities on the sampler's own tensors, equal to the
    restatements on them, and pareto over (psh, ppc, pnc) with the motif count as the hard limit: front 0 holds no design with a motif
    unless every design of the patch has one (no claim about the values: the weights are untrained)."""
    dims, model, _ = sampler_support.unit_model()
    G, K, N = 2, 64, 16
    inp = sampler_support.patches(G, K, dims, seed=5)
    res = sampler_support.sample(model, inp, seed=3, num_samples=N, steps=2)
    gm = inp["generation_mask"]
    pt = metrics.patches(res, gm, group_size=N)
    lb = metrics.liabilities(res, gm, group_size=N)
    assert pt["psh"].is_cuda and tuple(pt["psh"].shape) == (G * N,) and tuple(lb["n_motifs"].shape) == (G * N,) and tuple(pt["state"].shape) == (G * N, K)
    gen = gm.cpu().numpy()
    sites, tokens = sites_of(res), res["seq_idx"].cpu().numpy()
    want = patches_ref(sites, sites[::N], tokens, gen, group_size=N, hydrophobicity=np.array(metrics.KYTE_DOOLITTLE, f32),
                       charge=np.array(metrics.RESIDUE_CHARGE, f32), max_neighbours=16)
    out = numpy_of(pt)
    for k in OUTPUTS:
        assert np.array_equal(out[k], want[k]) if k in EXACT[:5] else (ulps_apart(out[k], want[k]) <= 1).all(), k
    one = np.zeros((G, K), np.int64)
    check_motifs(numpy_of(lb), motifs_ref(tokens, gen, None, one, np.arange(K) + one, MOTIF_WORDS, N), list(metrics.LIABILITY_MOTIFS), "sampled")
    ranked = metrics.pareto([pt["psh"], pt["ppc"], pt["pnc"]], group_size=N, violation=lb["n_motifs"].float().view(G, N))
    front, n = ranked["front"].cpu().numpy(), lb["n_motifs"].view(G, N).cpu().numpy()
    for g in range(G):
        assert front[g].any() and (n[g][front[g]] == n[g].min()).all()
        assert not (n[g][front[g]] > 0).any() or (n[g] > 0).all()
