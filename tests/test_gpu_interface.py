"""Binding modes on the MI355X: metrics.contact_map / diffab_metrics_contact_bits and metrics.pairwise_bits /
diffab_metrics_pairwise_bits against the numpy restatements of interface_ref.py, against metrics.contacts, and their contracts.

Every comparison is exact equality - integers, and fp32 values by their bit patterns: a contact is one fp32 comparison of a defined
number, the counts are integers, and each quotient is one correctly rounded fp32 division of two integers below 2^24.  The restatement
of the contact map runs on the SAME fp32 points the kernel reads (the frame kernel's atoms, the patch's xyz), as test_gpu_geometry.py
does for metrics.contacts."""
import functools

import numpy as np
import pytest
import torch

import sampler_support
from diffab_pytorch import _hip, io as dio, metrics
from interface_ref import contact_map_ref, pack_ref, pairwise_bits_ref, same_bits, unpack_ref
from sampler_support import GuardedABI, header_prototypes, hip, misaligned
from scratch_poison import poisoned
from test_geometry_host import d2_f32

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("hip")]

ATOMS5 = dio.BACKBONE_ATOMS
GLY = metrics.GLY
f32 = np.float32
cuda = lambda v: torch.from_numpy(np.ascontiguousarray(v)).cuda()
CONTEXT_ATOMS = {5: 7, 33: 32, 64: 15, 70: 32}  # A of the patches' real atoms, per K
I_EXACT, J_BONDED, I_HOLE, J_HOLE, J_EXACT = 0, 1, 2, 3, 4  # the five hand-placed slots of every patch


def rotation(rng):
    q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
    return q * np.sign(np.linalg.det(q))


# ------------------------------------------------------------------ contact-map inputs
@functools.lru_cache(maxsize=None)
def case(K, N, seed=0):
    """G = 2 patches x N designs of K residues scattered in a 14 A box (about a third of the generated / antigen pairs touch), with five
    hand-placed slots per patch.  Slot 0: generated, Gly in the first design, flagged as antigen as well, at (1, 2, 3) with the identity
    frame in every design.  Slot 1: antigen, on slot 0's chain with the next residue_idx, 3 A away: a chain neighbour.  Slot 2: generated,
    never moved, outside residue_mask in patch 0.  Slot 3: antigen, outside residue_mask in patch 1.  Slot 4: antigen on another chain at (1, 2, 8), its frame turned by
    180 degrees about x, and in the patch's real atoms only its CA: CA(0) - CA(4) is exactly 5 A, and no other atom pair of the two is
    nearer.  The last slot is an antigen residue, so the ragged last word has a live bit."""
    rng = np.random.default_rng(100 * K + N + seed)
    G, A = 2, CONTEXT_ATOMS[K]
    gen = rng.random((G, K)) < 0.3
    antigen = ~gen & (rng.random((G, K)) < 0.6)
    chain = np.where(gen, 0, rng.integers(0, 2, (G, K)))
    gen[:, [I_EXACT, I_HOLE]], gen[:, [J_BONDED, J_HOLE, J_EXACT, K - 1]] = True, False
    antigen[:, [I_EXACT, J_BONDED, J_HOLE, J_EXACT, K - 1]] = True
    chain[:, [I_EXACT, J_BONDED]], chain[:, [J_HOLE, J_EXACT]], chain[:, I_HOLE] = 0, 1, 2
    ridx = np.broadcast_to(np.arange(K), (G, K)).copy()
    rm = np.ones((G, K), bool)
    rm[0, I_HOLE] = rm[1, J_HOLE] = False
    t = rng.uniform(0.0, 14.0, (G, K, 3))
    R = np.stack([[rotation(rng) for _ in range(K)] for _ in range(G)])
    t[:, I_EXACT], t[:, J_BONDED], t[:, J_EXACT] = (1.0, 2.0, 3.0), (4.0, 2.0, 3.0), (1.0, 2.0, 8.0)
    t[:, I_HOLE], t[:, J_HOLE] = (4.0, 2.0, 6.0), (1.0, 5.0, 3.0)  # 3 A from slot 1 and 3.6 A from slot 4; 3 A from slot 0
    R[:, I_EXACT], R[:, J_EXACT] = np.eye(3), np.diag([1.0, -1.0, -1.0])
    seq0 = rng.integers(0, 20, (G, K))
    seq0[seq0 == GLY] = 0
    frame_atoms = dio.backbone_from_frames(torch.from_numpy(t.astype(f32)), torch.from_numpy(R.astype(f32)), ATOMS5).numpy()  # (G,K,5,3)
    xyz = np.zeros((G, K, A, 3), f32)
    xyz[:, :, :5] = frame_atoms
    xyz[:, :, 5:] = frame_atoms[:, :, 4:5] + rng.normal(0.0, 1.4, (G, K, A - 5, 3)).astype(f32)
    am = rng.random((G, K, A)) < 0.75
    am[:, :, :4] = True
    if K > 6:
        am[:, 6] = False  # a residue without a single atom
    am[:, J_EXACT] = False
    am[:, J_EXACT, 1] = True
    xyz[:, J_EXACT, 1] = (1.0, 2.0, 8.0)
    seq, tt, RR = [], [], []
    for g in range(G):
        for r in range(N):
            s, x, O = seq0[g].copy(), t[g].copy(), R[g].copy()
            move = gen[g].copy()
            move[[I_EXACT, I_HOLE]] = False
            n = int(move.sum())
            x[move] += rng.normal(0.0, 1.5, (n, 3))
            O[move] = np.stack([rotation(rng) for _ in range(n)]) if n else O[move]
            s[move] = np.where(rng.random(n) < 0.2, GLY, rng.integers(0, 20, n))
            s[I_EXACT] = GLY if r == 0 else 1
            seq.append(s), tt.append(x.astype(f32)), RR.append(O.astype(f32))
    designs = {"seq_idx": cuda(np.stack(seq)), "translations": cuda(np.stack(tt)), "orientations": cuda(np.stack(RR))}
    c = dict(G=G, N=N, K=K, A=A, gen=gen, antigen=antigen, chain=chain, ridx=ridx, rm=rm, xyz=xyz, am=am, designs=designs,
             atom_bits=(am.astype(np.int64) << np.arange(A)).sum(-1), context={"xyz": cuda(xyz), "atom_mask": cuda(am)})
    c["kw"] = dict(antigen_mask=cuda(antigen), chain_idx=cuda(chain), residue_idx=cuda(ridx), residue_mask=cuda(rm), group_size=N)
    c["gen_d"] = cuda(gen)
    return c


def design_points(designs, atoms=ATOMS5):
    """The fp32 atoms the kernel reads and their validity bits, as numpy."""
    pts = dio.backbone_from_frames(designs["translations"], designs["orientations"], atoms).float().cpu().numpy()
    seq = designs["seq_idx"].cpu().numpy()
    bits = np.full(seq.shape, (1 << len(atoms)) - 1, np.int64)
    if "CB" in atoms:
        bits[seq == GLY] &= ~(1 << atoms.index("CB"))
    return pts, bits


def context_of(c, context, pts, bits):
    return (c["xyz"], c["atom_bits"]) if context else (pts[::c["N"]], bits[::c["N"]])


@functools.lru_cache(maxsize=None)
def reference(K, N, context, **kw):
    c = case(K, N)
    pts, bits = design_points(c["designs"])
    cpts, cbits = context_of(c, context, pts, bits)
    return contact_map_ref(pts, bits, cpts, cbits, c["gen"], c["rm"], c["chain"], c["ridx"], c["antigen"], N, **kw)


@functools.lru_cache(maxsize=None)
def device_map(K, N, context):
    c = case(K, N)
    out = metrics.contact_map(c["designs"], c["gen_d"], context=c["context"] if context else None, **c["kw"])
    return {k: v.cpu().numpy() for k, v in out.items()}


def check_map(out, want, K, what):
    rows = want.shape[0]
    assert out["bits"].dtype == np.int32 and out["bits"].shape == (rows, K, (K + 31) // 32) and out["n_contacts"].dtype == np.int32
    got = unpack_ref(out["bits"])
    assert not got[:, :, K:].any(), (what, "bits of j >= K are set")
    bad = np.argwhere(got[:, :, :K] != want)
    assert len(bad) == 0, (what, "first differing (row, i, j):", bad[:5].tolist())
    assert same_bits(out["bits"], pack_ref(want)) and np.array_equal(out["n_contacts"], want.sum((1, 2)).astype(np.int32)), what


@pytest.mark.parametrize("context", [True, False], ids=["context", "frames"])
@pytest.mark.parametrize("N", [1, 3])
@pytest.mark.parametrize("K", [5, 33, 64, 70])
def test_contact_map_equals_the_restatement(K, N, context):
    c = case(K, N)
    gen, antigen, rm, chain, ridx = (c[k] for k in ("gen", "antigen", "rm", "chain", "ridx"))
    want = reference(K, N, context)
    pts, bits = design_points(c["designs"])
    cpts, cbits = context_of(c, context, pts, bits)
    # ---- what the inputs must contain
    assert c["A"] == CONTEXT_ATOMS[K] and max(CONTEXT_ATOMS.values()) == 32 and (~c["am"]).any() and ((c["atom_bits"] == 0).any() or K < 7)
    seq = c["designs"]["seq_idx"].cpu().numpy()
    assert all((seq[g * N:(g + 1) * N][:, gen[g] & rm[g]] == GLY).any() for g in range(2))  # a Gly among the generated residues
    assert (gen & ~rm).any() and (antigen & ~gen & ~rm).any()  # a hole in residue_mask on each side
    assert (gen[:, I_EXACT] & antigen[:, I_EXACT] & rm[:, I_EXACT]).all() and not want[:, :, I_EXACT].any()  # in both masks: no column
    assert (antigen[:, J_BONDED] & ~gen[:, J_BONDED] & rm[:, J_BONDED] & (chain[:, J_BONDED] == chain[:, I_EXACT])).all()
    assert (ridx[:, J_BONDED] - ridx[:, I_EXACT] == 1).all()  # an antigen residue that is a chain neighbour of a generated one ...
    assert reference(K, N, context, ignore_bonds=True)[:, I_EXACT, J_BONDED].all() and not want[:, I_EXACT, J_BONDED].any()  # ... and near it
    for r in range(2 * N):  # one atom pair at exactly the contact distance, none of the two residues nearer: the comparison is strict
        g = r // N
        mine = pts[r, I_EXACT][[a for a in range(5) if (bits[r, I_EXACT] >> a) & 1]]
        theirs = cpts[g, J_EXACT][[a for a in range(cpts.shape[2]) if (int(cbits[g, J_EXACT]) >> a) & 1]]
        d2 = d2_f32(mine, theirs)
        assert d2.min() == f32(5.0) * f32(5.0) and (d2 == f32(25.0)).any() and not want[r, I_EXACT, J_EXACT]
    assert reference(K, N, context, contact_distance=float(np.nextafter(f32(5), f32(6))))[:, I_EXACT, J_EXACT].all()
    assert not want[:, ~(gen & rm)[0]][:N].any() and not want[:N, I_HOLE].any() and not want[N:, :, J_HOLE].any()
    assert want[N:, I_HOLE].any() and want[:N, :, J_HOLE].any()  # (the same slots count in the patch whose residue_mask holds them)
    assert want[:, :, K - 1].any() and 0.05 < want[:, gen[0] & rm[0]][:N][:, :, antigen[0] & ~gen[0] & rm[0]].mean() < 0.95
    # ---- the device
    check_map(device_map(K, N, context), want, K, f"contact_map K={K} N={N} context={context}")


@pytest.mark.parametrize("context", [True, False], ids=["context", "frames"])
@pytest.mark.parametrize("N", [1, 3])
@pytest.mark.parametrize("K", [5, 33, 64, 70])
def test_contact_map_agrees_with_contacts(K, N, context):
    """The code that already exists counts what the map holds: same inputs, metrics.contacts."""
    c = case(K, N)
    out = device_map(K, N, context)
    old = {k: v.cpu().numpy() for k, v in metrics.contacts(c["designs"], c["gen_d"], context=c["context"] if context else None, **c["kw"]).items()}
    m = metrics.unpack_contact_map(torch.from_numpy(out["bits"]), K).numpy()
    assert np.array_equal(out["n_contacts"], old["n_contact_pairs"]) and out["n_contacts"].max() > 0
    by_row, by_col = m.sum(2).astype(np.int32), m.sum(1).astype(np.int32)
    for g in range(2):
        rows = slice(g * N, (g + 1) * N)
        assert np.array_equal(by_row[rows][:, c["gen"][g]], old["residue_contact"][rows][:, c["gen"][g]])
        assert np.array_equal(by_col[rows][:, ~c["gen"][g]], old["residue_contact"][rows][:, ~c["gen"][g]])
        assert not by_row[rows][:, ~c["gen"][g]].any() and not by_col[rows][:, c["gen"][g]].any()
    assert np.array_equal((by_row > 0).sum(1), old["n_paratope"]) and np.array_equal((by_col > 0).sum(1), old["n_epitope"])


def test_contact_map_other_atoms_and_cutoffs():
    K, N = 33, 3
    c = case(K, N)
    for atoms, dist in ((("CA",), 8.0), (("N", "CA", "C", "O"), 4.0), (ATOMS5, 0.0)):
        pts, bits = design_points(c["designs"], atoms)
        want = contact_map_ref(pts, bits, c["xyz"], c["atom_bits"], c["gen"], c["rm"], c["chain"], c["ridx"], c["antigen"], N, contact_distance=dist)
        out = metrics.contact_map(c["designs"], c["gen_d"], context=c["context"], atoms=atoms, contact_distance=dist, **c["kw"])
        check_map({k: v.cpu().numpy() for k, v in out.items()}, want, K, f"atoms={atoms} contact_distance={dist}")
        assert want.any() == (dist > 0)


# ------------------------------------------------------------------ pairwise inputs
PAIR_SHAPES = [(1, 1, 1), (2, 3, 5), (3, 63, 7), (2, 65, 33), (1, 129, 600), (2, 257, 40)]
LIVE = {(2, 3, 5): "all", (1, 129, 600): "all", (2, 257, 40): "three"}  # every column live / at most three; the others: about half


@functools.lru_cache(maxsize=None)
def pair_case(G, N, L):
    """(G*N, L) int32: designs of random words at two densities (1/2 and 1/8), design 1 and design 3 all zero, design 2 a copy of
    design 0, a word with the sign bit set in every patch; dead columns are zero in every design."""
    rng = np.random.default_rng(1000 * N + L)
    words = lambda *shape: rng.integers(0, 2 ** 32, shape, dtype=np.uint64).astype(np.uint32)
    b = words(G, N, L)
    b[:, 1::2] &= words(G, (N + 0) // 2, L) & words(G, N // 2, L)
    kind = LIVE.get((G, N, L), "half")
    live = np.ones((G, L), bool) if kind == "all" else rng.random((G, L)) < 0.5
    if kind == "three":
        live[:] = False
        for g in range(G):
            live[g, rng.choice(np.arange(1, L), 2, replace=False)] = True
    live[:, 0] = True
    b[~np.broadcast_to(live[:, None, :], b.shape)] = 0
    b[:, 0, 0] |= 0x80000000
    if N >= 2:
        b[:, 1] = 0
    if N >= 3:
        b[:, 2] = b[:, 0]
    if N >= 4:
        b[:, 3] = 0
    return np.ascontiguousarray(b.reshape(G * N, L).view(np.int32))


@functools.lru_cache(maxsize=None)
def pair_reference(G, N, L):
    return pairwise_bits_ref(pair_case(G, N, L), N)


def check_pairs(out, want, what):
    assert set(out) <= set(want)
    for k in out:
        assert same_bits(out[k], want[k]), (what, k, np.argwhere(out[k] != want[k])[:5].tolist())


@pytest.mark.parametrize("G, N, L", PAIR_SHAPES)
def test_pairwise_bits_equals_the_restatement(G, N, L):
    bits = pair_case(G, N, L)
    want = pair_reference(G, N, L)
    # ---- what the inputs must contain
    live = (bits.reshape(G, N, L) != 0).any(1).sum(1)
    kind = LIVE.get((G, N, L), "half")
    assert (live == L).all() if kind == "all" else (live <= 3).all() if kind == "three" else (live > 0).all()
    assert (bits < 0).any()
    if N >= 4:
        assert (want["n_set"][:, [1, 3]] == 0).all() and same_bits(bits.reshape(G, N, L)[:, 2], bits.reshape(G, N, L)[:, 0])
        dens = want["n_set"][:, 4:].astype(np.float64) / (32.0 * live[:, None])
        assert dens[:, 0::2].mean() > 0.4 and dens[:, 1::2].mean() < 0.2  # two densities
    # ---- the device
    out = {k: v.cpu().numpy() for k, v in metrics.pairwise_bits(cuda(bits), group_size=N).items()}
    assert set(out) == {"n_set", "n_common", "fcc", "jaccard"}
    check_pairs(out, want, f"pairwise_bits G={G} N={N} L={L}")
    # ---- properties, on the device's own numbers
    nc, ns = out["n_common"], out["n_set"]
    assert np.array_equal(nc, nc.transpose(0, 2, 1)) and np.array_equal(np.diagonal(nc, axis1=1, axis2=2), ns)
    assert same_bits(out["jaccard"], np.ascontiguousarray(out["jaccard"].transpose(0, 2, 1)))
    assert (np.diagonal(out["fcc"], axis1=1, axis2=2) == 1).all() and (np.diagonal(out["jaccard"], axis1=1, axis2=2) == 1).all()
    if N >= 4:  # the empty-set conventions
        assert (out["fcc"][:, [1, 3], :] == 1).all() and (out["fcc"][:, 0, [1, 3]] == 0).all()
        assert (out["jaccard"][:, 1, 3] == 1).all() and (out["jaccard"][:, 3, 1] == 1).all() and (out["jaccard"][:, 0, [1, 3]] == 0).all()
        assert (nc[:, 0, 2] == ns[:, 0]).all() and (out["jaccard"][:, 0, 2] == 1).all() and (out["fcc"][:, 2, 0] == 1).all()  # identical designs


# ------------------------------------------------------------------ the C ABI directly
INTERFACE_ARGTYPES = {n: a for n, (_, a) in _hip.INTERFACE_SYMBOLS.items()}
INTERFACE_WRITES = {"diffab_metrics_contact_bits": "bits n_contacts workspace",
                    "diffab_metrics_pairwise_bits": "n_set n_common fcc jaccard workspace"}


def place(t, shifted):
    """The tensor itself, or a copy that starts 4 bytes (1 byte for masks) behind a 16-byte boundary: the natural alignment only."""
    return misaligned(t, 4 if t.element_size() >= 4 else 1) if shifted else t


def raw_contact_bits(c, context=True, shifted=False):
    """diffab_metrics_contact_bits on the operands metrics.contact_map would build, through whatever stands in for _hip.lib()."""
    G, N, K = c["G"], c["N"], c["K"]
    pts, bits = design_points(c["designs"])
    cpts, cbits = context_of(c, context, pts, bits)
    A = cpts.shape[2]
    word = np.where(cbits >= 2 ** 31, cbits - 2 ** 32, cbits).astype(np.int32)
    ops = [cuda(pts), cuda(bits.astype(np.uint8)), cuda(np.asarray(cpts, f32)), cuda(word), cuda(c["gen"]), cuda(c["rm"]), cuda(c["antigen"]),
           cuda(c["chain"].astype(np.int32)), cuda(c["ridx"].astype(np.int32))]
    ops = [place(t, shifted) for t in ops]
    out = [place(torch.empty(G * N, K, (K + 31) // 32, dtype=torch.int32, device="cuda"), shifted),
           place(torch.empty(G * N, dtype=torch.int32, device="cuda"), shifted)]
    nbytes = metrics.contact_bits_workspace_bytes(G, K, A)
    ws = _hip.workspace(nbytes)
    lib = _hip.lib()
    rc = lib.diffab_metrics_contact_bits(*[_hip.ptr(t) for t in ops], G * N, N, K, 5, A, 5.0, *[_hip.ptr(t) for t in out], _hip.ptr(ws), nbytes,
                                         _hip.stream_ptr())
    assert rc == 0, _hip.load_library().diffab_last_error().decode()
    torch.cuda.synchronize()
    return {"bits": out[0].cpu().numpy(), "n_contacts": out[1].cpu().numpy()}


def raw_pairwise_bits(bits, N, skip=(), shifted=False):
    G, L = bits.shape[0] // N, bits.shape[1]
    b = place(cuda(bits), shifted)
    shapes = {"n_set": ((G, N), torch.int32), "n_common": ((G, N, N), torch.int32), "fcc": ((G, N, N), torch.float32),
              "jaccard": ((G, N, N), torch.float32)}
    out = {k: place(torch.empty(*s, dtype=d, device="cuda"), shifted) for k, (s, d) in shapes.items() if k not in skip}
    nbytes = metrics.pairwise_bits_workspace_bytes(G, N, L)
    ws = _hip.workspace(nbytes)
    lib = _hip.lib()
    rc = lib.diffab_metrics_pairwise_bits(_hip.ptr(b), G, N, L, *[_hip.ptr(out.get(k)) for k in shapes], _hip.ptr(ws), nbytes, _hip.stream_ptr())
    assert rc == 0, _hip.load_library().diffab_last_error().decode()
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


@pytest.mark.parametrize("skip", [("n_set",), ("n_common", "fcc"), ("n_set", "n_common", "fcc"), ("jaccard",), ("n_set", "n_common", "fcc", "jaccard")])
def test_null_outputs_are_skipped_and_the_others_unchanged(skip):
    for shape in ((2, 65, 33), (2, 257, 40)):
        out = raw_pairwise_bits(pair_case(*shape), shape[1], skip=skip)
        assert set(out) == {"n_set", "n_common", "fcc", "jaccard"} - set(skip)
        check_pairs(out, pair_reference(*shape), f"{shape} without {skip}")


# ------------------------------------------------------------------ determinism and contracts
@pytest.mark.parametrize("context", [True, False], ids=["context", "frames"])
def test_a_patch_alone_gives_the_bits_it_gives_in_a_batch(context):
    K, N = 70, 3
    c, both = case(K, N), device_map(K, N, context)
    for g in range(2):
        rows = slice(g * N, (g + 1) * N)
        kw = {k: (v if k == "group_size" else v[g:g + 1]) for k, v in c["kw"].items()}
        alone = metrics.contact_map({k: v[rows] for k, v in c["designs"].items()}, c["gen_d"][g:g + 1],
                                    context={k: v[g:g + 1] for k, v in c["context"].items()} if context else None, **kw)
        assert same_bits(alone["bits"].cpu().numpy(), both["bits"][rows]) and same_bits(alone["n_contacts"].cpu().numpy(), both["n_contacts"][rows])
    for G, N, L in ((3, 63, 7), (2, 257, 40)):
        bits, want = pair_case(G, N, L), pair_reference(G, N, L)
        for g in range(G):
            alone = {k: v.cpu().numpy() for k, v in metrics.pairwise_bits(cuda(bits[g * N:(g + 1) * N]), group_size=N).items()}
            check_pairs(alone, {k: v[g:g + 1] for k, v in want.items()}, f"patch {g} of {(G, N, L)} alone")


@pytest.mark.parametrize("fill", ["ff", "random"])
def test_what_the_workspace_and_the_outputs_held_is_ignored(fill):
    with poisoned(fill, seed=3):
        for K, N, context in ((33, 3, True), (70, 3, False), (5, 1, True)):
            c = case(K, N)
            out = metrics.contact_map(c["designs"], c["gen_d"], context=c["context"] if context else None, **c["kw"])
            check_map({k: v.cpu().numpy() for k, v in out.items()}, reference(K, N, context), K, f"K={K} under {fill}")
        for shape in ((2, 3, 5), (2, 65, 33), (1, 129, 600), (2, 257, 40)):
            out = {k: v.cpu().numpy() for k, v in metrics.pairwise_bits(cuda(pair_case(*shape)), group_size=shape[1]).items()}
            check_pairs(out, pair_reference(*shape), f"{shape} under {fill}")
            check_pairs(raw_pairwise_bits(pair_case(*shape), shape[1], skip=("n_set", "fcc")), pair_reference(*shape), f"{shape} under {fill}, two outputs")


@pytest.mark.parametrize("fill", sampler_support.GUARD_FILLS)
def test_outputs_between_guards_with_operands_at_their_natural_alignment(fill, monkeypatch):
    for entry, writes in INTERFACE_WRITES.items():
        monkeypatch.setitem(sampler_support.WRITES, entry, writes)
    params = {n: [p[0] for p in ps] for n, ps in header_prototypes(("diffab_hip_interface.h",))[1].items()}
    assert set(params) == set(INTERFACE_ARGTYPES)
    with GuardedABI(tuple(INTERFACE_ARGTYPES), fill, argtypes=INTERFACE_ARGTYPES) as abi:
        abi.params.update(params)
        for K, N, context in ((33, 3, True), (70, 3, False), (64, 1, True)):
            check_map(raw_contact_bits(case(K, N), context, shifted=True), reference(K, N, context), K, f"K={K} N={N} guarded [{fill}]")
        for shape in ((2, 3, 5), (3, 63, 7), (2, 65, 33), (2, 257, 40)):
            check_pairs(raw_pairwise_bits(pair_case(*shape), shape[1], shifted=True), pair_reference(*shape), f"{shape} guarded [{fill}]")
        check_pairs(raw_pairwise_bits(pair_case(2, 65, 33), 65, skip=("n_common",), shifted=True), pair_reference(2, 65, 33), "guarded, three outputs")
    assert abi.counts["diffab_metrics_contact_bits"] >= 3 * 11 and abi.counts["diffab_metrics_pairwise_bits"] >= 4 * 5 + 4


# ------------------------------------------------------------------ end to end: two planted binding modes
def test_two_planted_binding_modes_come_back_as_two_clusters():
    """One patch, N = 32 designs: a loop of eight residues, rigid, placed 4.5 A above one of two rows of an antigen lattice (4 A apart,
    CA only), plus a jitter of at most 0.1 A that flips no contact: the nearest lattice point stays within 4.7 A, the next beyond 5.8 A."""
    rng = np.random.default_rng(7)
    N, n_loop, nx, ny = 32, 8, 8, 3
    K = n_loop + nx * ny
    lattice = np.array([(4.0 * i, 4.0 * j, 0.0) for j in range(ny) for i in range(nx)])
    family = rng.permutation(np.array([0] * 20 + [1] * 12))
    t = np.zeros((N, K, 3))
    t[:, n_loop:] = lattice
    for r in range(N):
        y = 0.0 if family[r] == 0 else 8.0
        t[r, :n_loop] = np.array([(4.0 * i, y, 4.5) for i in range(n_loop)]) + rng.uniform(-0.1, 0.1, (n_loop, 3))
    gen = np.zeros((1, K), bool)
    gen[0, :n_loop] = True
    chain = np.where(gen, 0, 1)
    designs = {"seq_idx": torch.zeros(N, K, dtype=torch.long), "translations": torch.from_numpy(t.astype(f32)),
               "orientations": torch.eye(3).expand(N, K, 3, 3).clone()}
    context = {"xyz": torch.from_numpy(t[:1, :, None, :].astype(f32)), "atom_mask": torch.ones(1, K, 1, dtype=torch.bool)}
    # ---- on the CPU restatement first: the families are separated by the cutoff
    pts = t.astype(f32)[:, :, None, :]
    ones = np.ones((N, K), np.int64)
    want = contact_map_ref(pts, ones, pts[:1], ones[:1], gen, np.ones((1, K), bool), chain, np.arange(K)[None], ~gen, N)
    ref = pairwise_bits_ref(pack_ref(want).reshape(N, -1), N)
    cutoff = 0.5
    same = family[:, None] == family[None, :]
    dist = f32(1) - ref["jaccard"][0]
    assert (want.sum((1, 2)) == n_loop).all() and dist[same].max() < cutoff < dist[~same].min()
    # ---- the device, through the three calls
    cm = metrics.contact_map({k: v.cuda() for k, v in designs.items()}, cuda(gen), context={k: v.cuda() for k, v in context.items()},
                             antigen_mask=cuda(~gen), chain_idx=cuda(chain), group_size=N, atoms=("CA",))
    assert same_bits(cm["bits"].cpu().numpy(), pack_ref(want))
    pw = metrics.pairwise_bits(cm["bits"], group_size=N)
    check_pairs({k: v.cpu().numpy() for k, v in pw.items()}, ref, "planted modes")
    cl = metrics.cluster(1 - pw["jaccard"], cutoff)
    assert cl["count"].tolist() == [2] and cl["size"][0, :2].tolist() == [20, 12] and cl["n_unassigned"].tolist() == [0]
    assert np.array_equal(cl["label"][0].cpu().numpy(), family.astype(np.int32))
