"""The binding score on the MI355X: metrics.interface_energy / diffab_metrics_pair_energy against the numpy
restatement of pair_energy_ref.py, its properties and its contracts.

Integers are compared for exact equality: every decision is a float32 comparison of a defined number.  (a) With a DYADIC table - entries
k / 64 in [-4, 4] - every fp64 partial sum of at most 2^18 terms is exact whatever the order, so EVERY output, the energies, the
per-residue sums and the substitution scan, must equal the restatement bit for bit.  (b) With a real-valued table each float output
obeys |got - ref| <= ulp32(ref) + 2^-34 * sum |term| (pair_energy_ref.bound): one rounding and the double-rounding boundary, plus what an
fp64 sum of at most 2^18 terms errs by in another order, n * 2^-53 * sum |t|, with a factor of 2 for the scan's difference of two
sums.  The restatement runs on the SAME fp32 sites the kernel reads (the frame kernel's CA and CB, the patch's xyz)."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import sampler_support
from diffab_pytorch import _hip, io as dio, metrics
from pair_energy_ref import FLOATS, INTS, bound, pair_energy_ref, same_bits, ulp32
from sampler_support import GuardedABI, header_prototypes, hip, misaligned
from scratch_poison import poisoned

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("hip")]

GLY, UNK = metrics.GLY, 20
f32 = np.float32
cuda = lambda v: torch.from_numpy(np.ascontiguousarray(v)).cuda()
numpy_of = lambda out: {k: v.cpu().numpy() for k, v in out.items()}
A = 7  # atom slots of the patches' real atoms
EDGES = {1: (0.0, 9.0), 3: (0.0, 5.0, 7.0, 9.0), 8: (0.0, 4.0, 5.0, 6.0, 7.0, 8.0, 9.0, 10.0, 11.0)}
OUTPUTS = ("e_antigen", "e_framework", "e_internal", "n_pairs", "residue_energy", "residue_antigen_energy", "n_partners", "substitution")
SHAPES = [(K, N) for K in (5, 33, 63, 64, 65, 130) for N in (1, 3)] + [(33, 65)]  # (33, 65): one patch, 65 rows in the group
# the other bin counts and the full table width, where the smaller shapes fill every bin of every class
FORMS = [(65, 3, 1, 20), (65, 3, 8, 20), (130, 3, 8, 32), (64, 1, 1, 32), (33, 65, 8, 20), (63, 3, 3, 32)]
SEED = {(33, 1): 5}  # (at K = 33 with two rows, seeds 0 to 3 leave a bin of the eight generated residues' internal pairs empty)


def rotations(rng, n):
    q, _ = np.linalg.qr(rng.normal(size=(n, 3, 3)))
    return q * np.sign(np.linalg.det(q))[:, None, None]


# ------------------------------------------------------------------ inputs
@functools.lru_cache(maxsize=None)
def case(K, N, V=20):
    """test_gpu_developability.case with chains: G patches (2; 1 where N = 65) x N designs of K residues, uniform in a cube of edge
    (135 K)^(1/3) A - about a protein's density.  A contiguous quarter of the slots is generated (it starts at K // 5), the last third
    is the antigen: chain 1, numbered from 1, the antibody chain 0 numbered by slot.  The generated residues of every design are moved
    by about 1.5 A and redrawn; a fifth of them is Gly, a few tokens are UNK = 20 - outside a table of V = 20 classes; with V = 32 the
    tokens run over 0 .. 31 and a few are 32 or negative.  One non-generated residue lies outside residue_mask, and in the patch's real
    atoms one non-generated residue has no CA (it is absent), a few have no CB and one is Gly (their site is the CA)."""
    rng = np.random.default_rng(1000 * K + N + SEED.get((K, N), 0))
    G = 1 if N > 8 else 2
    edge = (135.0 * K) ** (1.0 / 3.0)
    n_gen, n_ag = max(1, K // 4), K // 3
    gen = np.zeros((G, K), bool)
    gen[:, K // 5:K // 5 + n_gen] = True
    antigen = np.zeros((G, K), bool)
    antigen[:, K - n_ag:] = True
    assert not (gen & antigen).any()
    chain = antigen.astype(np.int64)
    ridx = np.where(antigen, np.arange(K) - (K - n_ag) + 1, np.arange(K))
    free = np.flatnonzero(~gen[0] & ~antigen[0])
    rm = np.ones((G, K), bool)
    t0 = rng.uniform(0.0, edge, (G, K, 3))
    R0 = rotations(rng, G * K).reshape(G, K, 3, 3)
    top = 20 if V == 20 else 32
    seq0 = rng.integers(0, top, (G, K))
    seq0[seq0 == GLY] = 0
    am = np.ones((G, K, A), bool)
    am[:, :, 4] = rng.random((G, K)) < 0.8
    am[:, :, 5:] = rng.random((G, K, 2)) < 0.5
    if len(free) >= 3:
        rm[:, free[0]] = False
        am[:, free[1], 1] = False  # no CA: absent
        seq0[:, free[2]] = GLY
        am[:, free[2], 4] = True  # (a Gly with a "CB" in the mask still takes its CA)
    outside = UNK if V == 20 else 32
    seq, tt, RR = [], [], []
    for g in range(G):
        for r in range(N):
            s, x, O = seq0[g].copy(), t0[g].copy(), R0[g].copy()
            n = int(gen[g].sum())
            x[gen[g]] += rng.normal(0.0, 1.5, (n, 3))
            O[gen[g]] = rotations(rng, n)
            s[gen[g]] = np.where(rng.random(n) < 0.2, GLY, rng.integers(0, top, n))
            s[rng.random(K) < 0.04] = outside
            s[~gen[g]] = np.where(s[~gen[g]] == outside, outside, seq0[g][~gen[g]])  # (the context keeps its tokens, but for the unknown ones)
            if V == 32 and K > 8:
                s[K - 1] = -1
            seq.append(s), tt.append(x.astype(f32)), RR.append(O.astype(f32))
    designs = {"seq_idx": cuda(np.stack(seq)), "translations": cuda(np.stack(tt)), "orientations": cuda(np.stack(RR))}
    frame_atoms = dio.backbone_from_frames(torch.from_numpy(t0.astype(f32)), torch.from_numpy(R0.astype(f32)), dio.BACKBONE_ATOMS).numpy()
    xyz = np.zeros((G, K, A, 3), f32)
    xyz[:, :, :5] = frame_atoms
    xyz[:, :, 5:] = frame_atoms[:, :, 4:5] + rng.normal(0.0, 1.4, (G, K, A - 5, 3)).astype(f32)
    return dict(G=G, N=N, K=K, V=V, gen=gen, antigen=antigen, rm=rm, chain=chain, ridx=ridx, xyz=xyz, am=am, designs=designs, gen_d=cuda(gen),
                rm_d=cuda(rm), antigen_d=cuda(antigen), chain_d=cuda(chain), ridx_d=cuda(ridx), context={"xyz": cuda(xyz), "atom_mask": cuda(am)})


def sites_of(designs):
    """The fp32 sites the kernel reads, as numpy: CB of every row's frames through the frame kernel, CA where the token is Gly."""
    frame = dio.backbone_from_frames(designs["translations"], designs["orientations"], ("CA", "CB")).float().cpu().numpy()
    gly = designs["seq_idx"].cpu().numpy() == GLY
    return np.where(gly[:, :, None], frame[:, :, 0], frame[:, :, 1])


def inputs_of(c, context, antigen=True, designs=None, xyz=None):
    """(sites, context_sites, tokens, gen, rm, antigen, chain, ridx) as the rule of metrics.interface_energy builds them, in numpy."""
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
    return sites, csites, tokens, c["gen"], rm, (c["antigen"] if antigen else None), c["chain"], c["ridx"]


@functools.lru_cache(maxsize=None)
def table_of(kind, NB, V, seed=0):
    rng = np.random.default_rng(31 * NB + V + seed)
    if kind == "dyadic":  # k / 64 in [-4, 4], asymmetric
        return (rng.integers(-256, 257, (NB, V, V)) / 64.0).astype(f32)
    if kind == "symmetric":
        t = rng.integers(-128, 129, (NB, V, V)) / 64.0
        return (t + t.transpose(0, 2, 1)).astype(f32)
    assert kind == "real"
    return rng.normal(0.0, 1.5, (NB, V, V)).astype(f32)


def potential_of(table, NB):
    return metrics.PairPotential(table, EDGES[NB])


@functools.lru_cache(maxsize=None)
def reference(K, N, context, kind="dyadic", NB=3, V=20, antigen=True):
    c = case(K, N, V)
    *ops, chain, ridx = inputs_of(c, context, antigen)
    return pair_energy_ref(*ops, chain, ridx, table=table_of(kind, NB, V), bin_edges=EDGES[NB], group_size=N, min_separation=3)


def device_call(c, context, table, NB, antigen=True, designs=None, ctx=None, **kw):
    args = dict(context=(c["context"] if ctx is None else ctx) if context else None, antigen_mask=c["antigen_d"] if antigen else None,
                residue_mask=c["rm_d"], chain_idx=c["chain_d"], residue_idx=c["ridx_d"], group_size=c["N"], potential=potential_of(table, NB),
                min_separation=3, substitutions=True)
    args.update(kw)
    return metrics.interface_energy(c["designs"] if designs is None else designs, c["gen_d"], **args)


@functools.lru_cache(maxsize=None)
def device_energy(K, N, context, kind="dyadic", NB=3, V=20, antigen=True):
    return numpy_of(device_call(case(K, N, V), context, table_of(kind, NB, V), NB, antigen))


def check(out, want, what, exact, only=OUTPUTS):
    """Integers equal; floats bit for bit (exact) or within pair_energy_ref.bound -> the largest deviation of a float output in ulps."""
    assert set(out) - {"e_binding"} == set(only), (what, set(out) ^ set(only))
    worst = 0.0
    for k in only:
        assert out[k].dtype == want[k].dtype and out[k].shape == want[k].shape, (what, k, out[k].dtype, out[k].shape, want[k].shape)
        if k in INTS or exact:
            bad = np.argwhere(out[k] != want[k])
            assert len(bad) == 0 and same_bits(out[k], want[k]), (what, k, "first differing elements:", bad[:5].tolist())
        else:
            ref64 = want[k + "_f64"]
            off = np.abs(out[k].astype(np.float64) - ref64)
            ulps = float((off / ulp32(ref64)).max()) if off.size else 0.0
            worst = max(worst, ulps)
            print(f"{what}: {k} at most {ulps:.3f} ulp from the restatement")
            assert np.isfinite(out[k]).all() and (off <= bound(ref64, want["sum_abs"][k])).all(), (what, k, ulps)
    if "e_binding" in out:
        assert same_bits(out["e_binding"], out["e_antigen"])
    return worst


def filled(want, what):
    """The condition of the issue, on the restatement: every (class, bin) holds a counted pair in some row of the case."""
    total = want["n_pairs"].sum(0)
    assert (total > 0).all(), (what, total.tolist())


# ------------------------------------------------------------------ (a) dyadic tables: bit for bit
@pytest.mark.parametrize("context", [True, False], ids=["context", "frames"])
@pytest.mark.parametrize("K, N", SHAPES)
def test_a_dyadic_table_equals_the_restatement_bit_for_bit(K, N, context):
    c, want = case(K, N), reference(K, N, context)
    if K >= 33:  # what the inputs must contain
        filled(want, (K, N, context))
        tokens = c["designs"]["seq_idx"].cpu().numpy()
        assert (tokens == UNK).any() and (tokens[:, c["gen"][0]] == GLY).any() and not c["rm"].all()
        assert (want["substitution"] != 0).any() and (want["e_antigen"] != 0).any() and (want["e_internal"] != 0).any()
        if context:
            assert (~c["am"][:, :, 1]).any() and (~c["am"][:, :, 4] & ~c["gen"]).any()
    check(device_energy(K, N, context), want, f"pair energy K={K} N={N} context={context}", exact=True)


@pytest.mark.parametrize("K, N, NB, V", FORMS)
def test_other_bin_counts_and_table_widths(K, N, NB, V):
    c, want = case(K, N, V), reference(K, N, True, "dyadic", NB, V)
    filled(want, (K, N, NB, V))
    tokens = c["designs"]["seq_idx"].cpu().numpy()
    assert (tokens >= V).any() and (V == 20 or ((tokens < 0).any() and (tokens == 31).any()))
    check(device_energy(K, N, True, "dyadic", NB, V), want, f"pair energy K={K} N={N} NB={NB} V={V}", exact=True)


def test_without_an_antigen_mask_every_partner_is_framework():
    K, N = 65, 3
    want = reference(K, N, True, antigen=False)
    assert (want["n_pairs"][:, 0] == 0).all() and (want["substitution"] == 0).all() and (want["n_pairs"][:, 1].sum(0) > 0).all()
    check(device_energy(K, N, True, antigen=False), want, "no antigen_mask", exact=True)


# ------------------------------------------------------------------ (b) a real-valued table: within the bound
@pytest.mark.parametrize("K, N, NB, V", [(33, 3, 3, 20), (65, 3, 3, 20), (130, 3, 8, 32), (33, 65, 3, 20), (64, 1, 1, 32)])
def test_a_real_valued_table_is_within_the_bound(K, N, NB, V):
    want = reference(K, N, True, "real", NB, V)
    filled(want, (K, N, NB, V))
    worst = check(device_energy(K, N, True, "real", NB, V), want, f"real table K={K} N={N} NB={NB} V={V}", exact=False)
    print(f"real table K={K} N={N} NB={NB} V={V}: largest deviation {worst:.3f} ulp")


def test_the_default_potential_and_default_chains():
    """metrics.contact_potential() (21 classes, real-valued), one chain numbered by slot, no residue_mask, no substitutions."""
    K, N = 64, 3
    c = case(K, N)
    sites, csites, tokens, gen, _, ag, _, _ = inputs_of(c, False)
    p = metrics.contact_potential()
    one = np.zeros((c["G"], K), np.int64)
    want = pair_energy_ref(sites, csites, tokens, gen, None, ag, one, np.arange(K) + one, table=p.table.numpy(), bin_edges=p.bin_edges, group_size=N,
                           substitutions=False)
    out = numpy_of(metrics.interface_energy(c["designs"], c["gen_d"], antigen_mask=c["antigen_d"], group_size=N))
    assert (want["n_pairs"].sum(0) > 0).all() and out["n_pairs"].shape == (c["G"] * N, 3, 2)
    check(out, want, "default potential", exact=False, only=OUTPUTS[:7])


# ------------------------------------------------------------------ (c) properties
def test_a_zero_table_gives_zeros_and_the_same_counts():
    K, N = 65, 3
    base = device_energy(K, N, True)
    out = numpy_of(device_call(case(K, N), True, np.zeros((3, 20, 20), f32), 3))
    for k in FLOATS:
        assert (out[k] == 0).all() and not np.signbit(out[k]).any(), k
    for k in INTS:
        assert same_bits(out[k], base[k]) and base[k].any(), k


def test_a_symmetric_table_gives_the_same_result_as_its_transpose_and_an_asymmetric_one_does_not():
    K, N = 65, 3
    c, sym, asym = case(K, N), table_of("symmetric", 3, 20), table_of("dyadic", 3, 20)
    assert np.array_equal(sym, sym.transpose(0, 2, 1)) and not np.array_equal(asym, asym.transpose(0, 2, 1))
    one, other = numpy_of(device_call(c, True, sym, 3)), numpy_of(device_call(c, True, np.ascontiguousarray(sym.transpose(0, 2, 1)), 3))
    for k in OUTPUTS:
        assert same_bits(one[k], other[k]), k
    *ops, chain, ridx = inputs_of(c, True)
    check(one, pair_energy_ref(*ops, chain, ridx, table=sym, bin_edges=EDGES[3], group_size=N), "symmetric table", exact=True)
    flipped = numpy_of(device_call(c, True, np.ascontiguousarray(asym.transpose(0, 2, 1)), 3))
    base = device_energy(K, N, True)
    assert not np.array_equal(flipped["e_antigen"], base["e_antigen"]) and not np.array_equal(flipped["e_internal"], base["e_internal"])
    assert same_bits(flipped["n_pairs"], base["n_pairs"])


def test_sites_that_are_never_read_may_hold_nan():
    """NaN in the row's sites of non-generated residues, in the patch's sites of generated residues and in every site of a residue
    outside residue_mask or without a CA changes no output bit."""
    K, N = 65, 3
    c, base = case(K, N), device_energy(K, N, True)
    gen_rows = np.repeat(c["gen"], N, 0)
    t = c["designs"]["translations"].cpu().numpy().copy()
    t[~gen_rows] = np.nan
    t[np.repeat(~c["rm"], N, 0)] = np.nan
    rows_poisoned = dict(c["designs"], translations=cuda(t))
    xyz = c["xyz"].copy()
    xyz[c["gen"]] = np.nan
    xyz[~c["rm"]] = np.nan
    xyz[~c["am"][:, :, 1] & ~c["gen"]] = np.nan
    ctx_poisoned = {"xyz": cuda(xyz), "atom_mask": c["context"]["atom_mask"]}
    for what, designs, ctx in (("row sites", rows_poisoned, None), ("context sites", None, ctx_poisoned), ("both", rows_poisoned, ctx_poisoned)):
        out = numpy_of(device_call(c, True, table_of("dyadic", 3, 20), 3, designs=designs, ctx=ctx))
        for k in OUTPUTS:
            assert same_bits(out[k], base[k]), (what, k)
    assert np.isnan(sites_of(rows_poisoned)[~gen_rows]).all() and np.isnan(xyz).any() and base["n_partners"].any()


def test_a_moved_antigen_changes_e_antigen_and_nothing_of_the_other_classes():
    K, N = 65, 3
    c, base = case(K, N), device_energy(K, N, True)
    xyz = c["xyz"].copy()
    xyz[c["antigen"]] += f32(2.0)
    out = numpy_of(device_call(c, True, table_of("dyadic", 3, 20), 3, ctx={"xyz": cuda(xyz), "atom_mask": c["context"]["atom_mask"]}))
    assert (out["e_antigen"] != base["e_antigen"]).all() and not same_bits(out["n_pairs"][:, 0], base["n_pairs"][:, 0])
    assert same_bits(out["e_internal"], base["e_internal"]) and same_bits(out["e_framework"], base["e_framework"])
    assert same_bits(out["n_pairs"][:, 1:], base["n_pairs"][:, 1:])
    *ops, chain, ridx = inputs_of(c, True, xyz=xyz)
    check(out, pair_energy_ref(*ops, chain, ridx, table=table_of("dyadic", 3, 20), bin_edges=EDGES[3], group_size=N), "moved antigen", exact=True)


def test_the_scan_is_zero_at_the_own_token_and_equals_a_rerun_with_the_token_replaced():
    K, N = 65, 3
    c, base = case(K, N), device_energy(K, N, True)
    tokens = c["designs"]["seq_idx"].cpu().numpy()
    gen_rows = np.repeat(c["gen"], N, 0)
    sub = base["substitution"]
    assert sub.shape == (c["G"] * N, K, 20) and (sub[~gen_rows] == 0).all() and (sub != 0).any(2)[gen_rows].sum() > gen_rows.sum() // 2
    r, i = np.nonzero(gen_rows & (tokens < 20))
    assert len(r) > 20 and (sub[r, i, tokens[r, i]] == 0).all() and not np.signbit(sub[r, i, tokens[r, i]]).any()
    # e_antigen of the row with the token of slot i replaced by v, minus e_antigen as it is (dyadic: both are exact); the structure is
    # held, so rows where the slot is Gly (whose site is the CA) are left out, and v is not Gly
    first = K // 5
    checked = 0
    for i, v in ((first, 0), (first + 3, 13), (first + K // 4 - 1, 19), (first + 5, 4)):
        assert c["gen"][:, i].all() and v != GLY
        keep = tokens[:, i] != GLY
        replaced = tokens.copy()
        replaced[keep, i] = v
        out = numpy_of(device_call(c, True, table_of("dyadic", 3, 20), 3, designs=dict(c["designs"], seq_idx=cuda(replaced)), substitutions=False))
        assert "substitution" not in out
        assert np.array_equal((out["e_antigen"] - base["e_antigen"])[keep], sub[keep, i, v]), (i, v)
        checked += int((sub[keep, i, v] != 0).sum())
    assert checked >= 6 and (tokens[:, first:first + K // 4] == UNK).any()  # (a row whose own token is unknown: S_cur = 0)


def raw_energy(K, N, context=True, skip=(), shifted=False, chains=True, kind="dyadic", NB=3, V=20):
    """diffab_metrics_pair_energy on the operands metrics.interface_energy would build, through whatever stands in for _hip.lib()."""
    c = case(K, N, V)
    sites, csites, tokens, gen, rm, ag, chain, ridx = inputs_of(c, context)
    place = lambda t: misaligned(t, 4 if t.element_size() >= 4 else 1) if shifted else t
    ops = [cuda(sites.astype(f32)), cuda(csites.astype(f32)), cuda(tokens.astype(np.int32)), cuda(gen), cuda(rm), cuda(ag),
           cuda(chain.astype(np.int32)) if chains else None, cuda(ridx.astype(np.int32)) if chains else None, cuda(table_of(kind, NB, V))]
    ops = [None if t is None else place(t) for t in ops]
    rows = c["G"] * N
    shapes = {"e_antigen": (rows,), "e_framework": (rows,), "e_internal": (rows,), "n_pairs": (rows, 3, NB), "residue_energy": (rows, K),
              "residue_antigen_energy": (rows, K), "n_partners": (rows, K), "substitution": (rows, K, V)}
    out = {k: place(torch.empty(s, dtype=torch.int32 if k in INTS else torch.float32, device="cuda")) for k, s in shapes.items() if k not in skip}
    host = (ctypes.c_float * (NB + 1))(*EDGES[NB])
    nbytes = metrics.pair_energy_workspace_bytes(c["G"], K)
    ws = _hip.workspace(nbytes)
    lib = _hip.lib()
    rc = lib.diffab_metrics_pair_energy(*[_hip.ptr(t) for t in ops], ctypes.cast(host, ctypes.c_void_p), rows, N, K, V, NB, 3,
                                        *[_hip.ptr(out.get(k)) for k in OUTPUTS], _hip.ptr(ws), nbytes, _hip.stream_ptr())
    assert rc == 0, _hip.load_library().diffab_last_error().decode()
    torch.cuda.synchronize()
    return numpy_of(out)


@pytest.mark.parametrize("skip", [("substitution",), ("e_antigen",), ("n_pairs", "n_partners"), ("residue_energy", "residue_antigen_energy"),
                                  ("e_antigen", "e_framework", "e_internal", "n_pairs"), OUTPUTS[:7], OUTPUTS])
def test_null_outputs_are_skipped_and_the_others_unchanged(skip):
    K, N = 65, 3
    out, full = raw_energy(K, N, skip=skip), device_energy(K, N, True)
    assert set(out) == set(OUTPUTS) - set(skip)
    for k in out:
        assert same_bits(out[k], full[k]), (skip, k)


def test_without_chain_and_residue_idx_no_pair_is_skipped():
    K, N = 65, 3
    c = case(K, N)
    *ops, _, _ = inputs_of(c, True)
    want = pair_energy_ref(*ops, None, None, table=table_of("dyadic", 3, 20), bin_edges=EDGES[3], group_size=N)
    assert want["n_pairs"].sum() > reference(K, N, True)["n_pairs"].sum()
    check(raw_energy(K, N, chains=False), want, "chain = residue_idx = NULL", exact=True)


@pytest.mark.parametrize("context", [True, False], ids=["context", "frames"])
def test_a_patch_alone_gives_the_bits_it_gives_in_a_batch(context):
    K, N = 65, 3
    c, both = case(K, N), device_energy(K, N, context, "real")
    for g in range(2):
        rows = slice(g * N, (g + 1) * N)
        alone = metrics.interface_energy({k: v[rows] for k, v in c["designs"].items()}, c["gen_d"][g:g + 1],
                                         context={k: v[g:g + 1] for k, v in c["context"].items()} if context else None,
                                         antigen_mask=c["antigen_d"][g:g + 1], residue_mask=c["rm_d"][g:g + 1], chain_idx=c["chain_d"][g:g + 1],
                                         residue_idx=c["ridx_d"][g:g + 1], group_size=N, potential=potential_of(table_of("real", 3, 20), 3),
                                         substitutions=True)
        for k in OUTPUTS:
            assert same_bits(alone[k].cpu().numpy(), both[k][rows]), (g, k)


def test_one_residue_and_a_row_without_a_generated_residue_give_zeros():
    one = {"seq_idx": torch.ones(2, 1, dtype=torch.long).cuda(), "translations": torch.zeros(2, 1, 3).cuda(),
           "orientations": torch.eye(3).expand(2, 1, 3, 3).contiguous().cuda()}
    out = numpy_of(metrics.interface_energy(one, torch.ones(2, 1, dtype=torch.bool).cuda(), substitutions=True))
    assert out["substitution"].shape == (2, 1, 21) and out["n_pairs"].shape == (2, 3, 2)
    for k in OUTPUTS:
        assert (out[k] == 0).all(), k
    c = case(33, 3)
    gen = c["gen"].copy()
    gen[0] = False  # patch 0 generates nothing: no pair is counted
    out = numpy_of(metrics.interface_energy(c["designs"], cuda(gen), antigen_mask=c["antigen_d"], group_size=3, substitutions=True,
                                            potential=potential_of(table_of("dyadic", 3, 20), 3)))
    for k in OUTPUTS:
        assert (out[k][:3] == 0).all() and out[k][3:].any() and out[k].dtype == device_energy(33, 3, False)[k].dtype, k


def test_native_equal_to_the_designs_improves_nothing():
    K = 65
    c = case(K, 1)
    kw = dict(context=c["context"], antigen_mask=c["antigen_d"], residue_mask=c["rm_d"], chain_idx=c["chain_d"], residue_idx=c["ridx_d"],
              potential=potential_of(table_of("real", 3, 20), 3))
    native = {k: v.clone() for k, v in c["designs"].items()}
    out = numpy_of(metrics.interface_energy(c["designs"], c["gen_d"], native=native, **kw))
    assert same_bits(out["native_e_antigen"], out["e_antigen"]) and same_bits(out["e_antigen"], device_energy(K, 1, True, "real")["e_antigen"])
    assert (out["delta"] == 0).all() and not out["improved"].any() and out["improved"].dtype == bool and (out["imp"] == 0).all()
    assert out["imp"].shape == (2,) and out["delta"].shape == (2,) and out["imp"].dtype == f32
    # three designs per patch against the first of them: IMP is the share of rows below it
    c3 = case(K, 3)
    native = {k: v[::3].clone() for k, v in c3["designs"].items()}
    out = numpy_of(metrics.interface_energy(c3["designs"], c3["gen_d"], native=native, group_size=3, **dict(kw, context=c3["context"])))
    e = device_energy(K, 3, True, "real")["e_antigen"]
    assert same_bits(out["native_e_antigen"], e[::3]) and same_bits(out["delta"], e - np.repeat(e[::3], 3))
    assert np.array_equal(out["improved"], e < np.repeat(e[::3], 3)) and np.array_equal(out["imp"], (e < np.repeat(e[::3], 3)).reshape(2, 3).mean(1).astype(f32))
    assert out["improved"].any() and not out["improved"][::3].any()


# ------------------------------------------------------------------ (d) contracts
@pytest.mark.parametrize("fill", ["ff", "random"])
def test_what_the_workspace_and_the_outputs_held_is_ignored(fill):
    with poisoned(fill, seed=5):
        for K, N, context, NB, V in ((33, 3, True, 3, 20), (65, 3, False, 3, 20), (130, 3, True, 8, 32), (5, 1, True, 3, 20), (64, 1, True, 1, 32)):
            out = numpy_of(device_call(case(K, N, V), context, table_of("dyadic", NB, V), NB))
            check(out, reference(K, N, context, "dyadic", NB, V), f"K={K} N={N} under {fill}", exact=True)
        check(raw_energy(65, 3, skip=OUTPUTS[3:]), reference(65, 3, True), f"three outputs under {fill}", exact=True, only=OUTPUTS[:3])
        check(raw_energy(65, 3, chains=False, skip=OUTPUTS[:3]), pair_energy_ref(*inputs_of(case(65, 3), True)[:6], None, None, table=table_of("dyadic", 3, 20),
                                                                                  bin_edges=EDGES[3], group_size=3), f"no chains under {fill}",
              exact=True, only=OUTPUTS[3:])


ENERGY_ARGTYPES = {n: a for n, (_, a) in _hip.ENERGY_SYMBOLS.items()}
ENERGY_WRITES = {"diffab_metrics_pair_energy": " ".join(OUTPUTS) + " workspace"}
EDGES_HOST_ARGUMENT = 9  # `bin_edges` is a host array: the guarded ABI passes it as it is


@pytest.mark.parametrize("fill", sampler_support.GUARD_FILLS)
def test_outputs_between_guards_with_operands_at_their_natural_alignment(fill, monkeypatch):
    for entry, writes in ENERGY_WRITES.items():
        monkeypatch.setitem(sampler_support.WRITES, entry, writes)
    params = {n: [p[0] for p in ps] for n, ps in header_prototypes(("diffab_hip_energy.h",))[1].items()}
    assert set(params) == set(ENERGY_ARGTYPES) and params["diffab_metrics_pair_energy"][EDGES_HOST_ARGUMENT] == "bin_edges"
    positions = {"diffab_metrics_pair_energy": set(range(len(params["diffab_metrics_pair_energy"]))) - {EDGES_HOST_ARGUMENT}}
    with GuardedABI(tuple(ENERGY_ARGTYPES), fill, argtypes=ENERGY_ARGTYPES, positions=positions) as abi:
        abi.params.update(params)
        for K, N, context, NB, V in ((33, 3, True, 3, 20), (65, 3, False, 3, 20), (64, 1, True, 1, 32), (130, 3, True, 8, 32)):
            check(raw_energy(K, N, context, shifted=True, NB=NB, V=V), reference(K, N, context, "dyadic", NB, V), f"K={K} N={N} guarded [{fill}]",
                  exact=True)
        check(raw_energy(65, 3, skip=OUTPUTS[:4], shifted=True), reference(65, 3, True), "guarded, per residue", exact=True, only=OUTPUTS[4:])
    assert abi.counts["diffab_metrics_pair_energy"] >= 4 * 17


# ------------------------------------------------------------------ (e) end to end
def test_sampled_designs_through_interface_energy_into_pareto():
    """sample(num_samples = 16) of the unit model at K = 64 -> interface_energy(native=...) on the sampler's own tensors, equal to the
    restatement on them, and pareto over (e_antigen, psh): front 0 holds the design of lowest e_antigen (no claim about the values:
    the weights are untrained and the default potential is a placeholder)."""
    dims, model, _ = sampler_support.unit_model()
    G, K, N = 2, 64, 16
    inp = sampler_support.patches(G, K, dims, seed=5)
    res = sampler_support.sample(model, inp, seed=3, num_samples=N, steps=2)
    gm = inp["generation_mask"]
    gen = gm.cpu().numpy()
    antigen = np.zeros((G, K), bool)
    antigen[:, K - K // 3:] = True
    antigen &= ~gen
    native = {k: inp[k] for k in ("seq_idx", "translations", "orientations")}
    out = metrics.interface_energy(res, gm, antigen_mask=cuda(antigen), group_size=N, substitutions=True, native=native)
    assert out["e_antigen"].is_cuda and tuple(out["e_antigen"].shape) == (G * N,) and tuple(out["substitution"].shape) == (G * N, K, 21)
    p = metrics.contact_potential()
    one = np.zeros((G, K), np.int64)
    sites, tokens = sites_of(res), res["seq_idx"].cpu().numpy()
    want = pair_energy_ref(sites, sites[::N], tokens, gen, None, antigen, one, np.arange(K) + one, table=p.table.numpy(), bin_edges=p.bin_edges,
                           group_size=N)
    got = numpy_of(out)
    check({k: got[k] for k in OUTPUTS + ("e_binding",)}, want, "sampled", exact=False)
    nsites = sites_of({k: v.cuda() for k, v in native.items()})
    nwant = pair_energy_ref(nsites, nsites, native["seq_idx"].cpu().numpy(), gen, None, antigen, one, np.arange(K) + one, table=p.table.numpy(),
                            bin_edges=p.bin_edges, substitutions=False)
    assert (np.abs(got["native_e_antigen"] - nwant["e_antigen_f64"]) <= bound(nwant["e_antigen_f64"], nwant["sum_abs"]["e_antigen"])).all()
    per_row = np.repeat(got["native_e_antigen"], N)
    assert same_bits(got["delta"], got["e_antigen"] - per_row) and np.array_equal(got["improved"], got["e_antigen"] < per_row)
    assert np.array_equal(got["imp"], (got["e_antigen"] < per_row).reshape(G, N).mean(1).astype(f32))
    psh = metrics.patches(res, gm, antigen_mask=cuda(antigen), group_size=N)["psh"]
    ranked = metrics.pareto([out["e_antigen"], psh], group_size=N)
    front, e = ranked["front"].cpu().numpy(), got["e_antigen"].reshape(G, N)
    for g in range(G):
        assert front[g].any() and front[g][e[g] == e[g].min()].any()
