"""Patch construction from a whole complex on the MI355X: diffab_patch_select / _gather / _scatter, diffab_pytorch.patch and
DiffAb.design_complex.

The rule is DESIGN.md section 4.12 / include/diffab_hip.h; the oracle is the numpy float64 restatement of test_patch_host.py.  On
coordinates of a 0.25 A grid every squared distance is exact in fp32, so the selection must EQUAL the oracle, ties included; on
unconstrained coordinates the test first checks that its own input has no near-tie at the rank that decides membership, then demands
equality as well.  Gather and scatter are bitwise torch indexing; design_complex is bitwise the four calls made by hand.
"""
import ctypes

import numpy as np
import pytest
import torch

from diffab_pytorch import _hip, patch, synthetic as syn
from diffab_pytorch.guidance import SampleGuidance
from sampler_support import hip, make_model
from test_patch_host import select_ref

pytestmark = pytest.mark.gpu
LIMIT = patch.MAX_RESIDUES
FIELDS = ("residue_mask", "anchor_mask", "chain", "antigen")


# ------------------------------------------------------------------ complexes
def blobs(rng, N, grid=True, segments=((1, 8),), length=None, chain_end=False):
    """One complex of N residues: a heavy, a light and an antigen blob (chains 1, 2, 3 - about 3 : 3 : 4), coordinates on the 0.25 A grid
    within +-64 A (or unconstrained floats), generated segments as (chain, length) pairs placed inside their chain (chain_end: the
    segment ends where its chain ends, so it has one anchor).  length < N: the residues behind it are padding outside residue_mask."""
    L = N if length is None else length
    nh, nl = max(1, (3 * L) // 10), (3 * L) // 10
    chain = np.zeros(N, np.int64)
    chain[:L] = np.array([1] * nh + [2] * nl + [3] * (L - nh - nl))[:L]
    centre = np.array([[0.0, 0, 0], [-12.0, 0, 0], [12.0, 0, 0], [0.0, 26, 0]])
    ca = centre[chain] + rng.normal(0.0, 9.0, (N, 3))
    ca = np.clip(np.round(ca * 4) / 4, -64, 64) if grid else ca + rng.normal(0.0, 1e-3, (N, 3))
    gen = np.zeros(N, bool)
    for c, n in segments:
        where = np.flatnonzero(chain == c)
        if where.size == 0:
            continue
        n = min(n, where.size)
        start = where[-1] - n + 1 if chain_end else where[0] + int(rng.integers(0, where.size - n + 1))
        gen[start:start + n] = True
    rm = np.arange(N) < L
    rm[rng.random(N) < 0.03] = False  # a few missing residues inside the complex as well
    return {"ca": ca.astype(np.float32), "gen": gen, "chain": chain, "antigen": chain == 3, "residue_mask": rm}


def raw_select(hip, cs, k, k_antigen, K, use=("residue_mask", "chain", "antigen")):
    """diffab_patch_select on the stacked complexes `cs` (the C entry itself: a count of -1 comes back as data)."""
    B, N = len(cs), cs[0]["ca"].shape[0]
    dev = lambda name, dt: torch.from_numpy(np.stack([c[name] for c in cs])).to(dt).cuda().contiguous() if name in use or name in ("ca", "gen") else None
    ca, gen = dev("ca", torch.float32), dev("gen", torch.bool)
    rm, am, ag, ch = dev("residue_mask", torch.bool), dev("anchor_mask", torch.bool), dev("antigen", torch.bool), dev("chain", torch.int64)
    index = torch.full((B, K), -7, dtype=torch.int64, device="cuda")
    mask = torch.full((B, K), True, dtype=torch.bool, device="cuda")
    count = torch.full((B,), -7, dtype=torch.int32, device="cuda")
    _hip.check(hip.diffab_patch_select(_hip.ptr(ca), 3, _hip.ptr(rm), _hip.ptr(gen), _hip.ptr(am), _hip.ptr(ch), _hip.ptr(ag), B, N, k,
                                       k_antigen, K, _hip.ptr(index), _hip.ptr(mask), _hip.ptr(count), _hip.stream_ptr()),
               "diffab_patch_select")
    torch.cuda.synchronize()
    return index.cpu().numpy(), mask.cpu().numpy(), count.cpu().numpy()


def oracle(c, k, k_antigen, K, use):
    kw = {name: c[name] for name in FIELDS if name in use}
    return select_ref(c["ca"], c["gen"], k, k_antigen, K, **kw)


def assert_equals_oracle(hip, cs, k, k_antigen, K=None, use=("residue_mask", "chain", "antigen"), min_gap=None):
    K = k + k_antigen if K is None else K
    want = [oracle(c, k, k_antigen, K, use) for c in cs]
    if min_gap is not None:  # a condition on the test's own input: no near-tie at the rank that decides membership, in either pass
        gaps = [g for w in want for g in w[3]]
        print("smallest relative gap at ranks k / k + 1:", min(gaps))
        assert min(gaps) >= min_gap, f"the seed is wrong, not the kernel: relative key gap {min(gaps):.3g} < {min_gap}"
    index, mask, count = raw_select(hip, cs, k, k_antigen, K, use)
    for b, (wi, wm, wc, _) in enumerate(want):
        assert count[b] == wc, (b, count[b], wc)
        assert np.array_equal(index[b], wi), (b, np.flatnonzero(index[b] != wi)[:8], index[b][index[b] != wi][:8], wi[index[b] != wi][:8])
        assert np.array_equal(mask[b], wm), b
    return want


# ------------------------------------------------------------------ exact selection on the grid
@pytest.mark.parametrize("N", [1, 63, 97, 400, 1000, 2500, LIMIT])
def test_grid_selection_equals_the_oracle(hip, N):
    rng = np.random.default_rng(100 + N)
    k, ka = (128, 128) if N >= 400 else (48, 24)
    cs = [blobs(rng, N, segments=((1, 9), (2, 6)) if N >= 63 else ((1, 1),))]
    want = assert_equals_oracle(hip, cs, k, ka, K=256)
    assert want[0][2] == (1 if N == 1 else want[0][2]) and want[0][2] > 0


def test_ragged_batch_of_37(hip):
    rng = np.random.default_rng(7)
    lengths = [int(v) for v in rng.integers(40, 701, 37)]
    lengths[3], lengths[20] = 700, 41
    cs = [blobs(rng, 700, length=L, segments=((1, 7), (2, 5))) for L in lengths]
    cs[11]["gen"][:] = False  # one complex with nothing to design, among the others
    want = assert_equals_oracle(hip, cs, 128, 128)
    counts = [w[2] for w in want]
    assert counts[11] == 0 and min(c for j, c in enumerate(counts) if j != 11) < 128 and max(counts) > 128  # count < k and the full patch both occur


def test_variants_of_the_definition(hip):
    rng = np.random.default_rng(11)
    # no antigen pass (NULL antigen_mask)
    assert_equals_oracle(hip, [blobs(rng, 500)], 96, 0, use=("residue_mask", "chain"))
    # no masks and no chain table at all
    assert_equals_oracle(hip, [blobs(rng, 300)], 64, 0, use=())
    # an antigen smaller than k_antigen
    c = blobs(rng, 400)
    c["antigen"] = c["antigen"] & (np.cumsum(c["antigen"]) <= 10)
    w = assert_equals_oracle(hip, [c], 64, 24)
    assert w[0][2] <= 64 + 10
    # a complex smaller than k: count < k, the rest of the row is padding
    w = assert_equals_oracle(hip, [blobs(rng, 63)], 128, 0, K=128)
    assert 0 < w[0][2] < 64 and (w[0][0][w[0][2]:] == -1).all()
    # an explicit anchor_mask (a few residues of the light chain, one of them absent)
    c = blobs(rng, 600)
    c["anchor_mask"] = np.zeros(600, bool)
    c["anchor_mask"][[200, 201, 230, 231]] = True
    c["residue_mask"][230] = False
    assert_equals_oracle(hip, [c], 128, 64, use=FIELDS)
    # an anchor_mask that marks nothing: the generated residues are the anchors
    c["anchor_mask"][:] = False
    assert_equals_oracle(hip, [c], 128, 64, use=FIELDS)
    # two generated segments on two chains; a segment at a chain end has one anchor
    assert_equals_oracle(hip, [blobs(rng, 800, segments=((1, 12), (2, 9)))], 128, 128)
    c = blobs(rng, 500, segments=((1, 6),), chain_end=True)
    c["residue_mask"][:] = True
    gen = np.flatnonzero(c["gen"])
    assert c["chain"][gen[-1] + 1] == 2  # the next residue is on the light chain: no anchor there
    assert_equals_oracle(hip, [c], 64, 32)
    # without the chain table the same residue IS an anchor, and the patch differs
    assert_equals_oracle(hip, [c], 64, 32, use=("residue_mask", "antigen"))
    # no generated residue: count 0, an empty row
    c = blobs(rng, 200)
    c["gen"][:] = False
    w = assert_equals_oracle(hip, [c], 32, 16)
    assert w[0][2] == 0


def test_more_forced_residues_than_k_is_reported(hip):
    rng = np.random.default_rng(5)
    cs = [blobs(rng, 300, segments=((1, 8),)), blobs(rng, 300, segments=((1, 40),)), blobs(rng, 300, segments=((1, 30),))]
    for c in cs:
        c["residue_mask"][:] = True
    index, mask, count = raw_select(hip, cs, 32, 0, 32)  # 8 + 2, 40 + 2 and 30 + 2 forced residues against k = 32
    assert count.tolist()[1] == -1 and (index[1] == -1).all() and not mask[1].any()
    assert_equals_oracle(hip, cs, 32, 0)
    assert count[0] == 32 and count[2] == 32  # exactly k forced residues still fit
    x = torch.from_numpy(np.stack([c["ca"] for c in cs]))
    gm = torch.from_numpy(np.stack([c["gen"] for c in cs]))
    with pytest.raises(ValueError, match="complex 1 has more generated and anchor residues than k = 32"):
        patch.select(x, gm, k=32, pad_to=32)


def test_tie_exactly_at_rank_k(hip):
    """Two residues mirrored about the single anchor have the same key bit for bit; placed at ranks k and k + 1, the lower index is in."""
    rng = np.random.default_rng(21)
    c = blobs(rng, 300, segments=((1, 1),))
    c["residue_mask"][:] = True
    g = int(np.flatnonzero(c["gen"])[0])
    c["anchor_mask"] = np.zeros(300, bool)
    c["anchor_mask"][g - 1] = True
    c["ca"][g - 1] = [1.25, -0.5, 2.0]  # the anchor, well inside the grid
    k = 20
    d = ((c["ca"].astype(np.float64) - c["ca"][g - 1]) ** 2).sum(1)
    d[[g, g - 1]] = -1
    ranked = np.lexsort((np.arange(300), d))
    lo, hi = sorted((int(ranked[k - 1]), int(ranked[k])))
    c["ca"][hi] = 2 * c["ca"][g - 1] - c["ca"][lo]  # the mirror image: on the grid, within +-64 + 2.5
    want = assert_equals_oracle(hip, [c], k, 0, use=("anchor_mask",))
    assert want[0][3][0] == 0.0, "the constructed tie is not at rank k"
    assert lo in want[0][0] and hi not in want[0][0]


# ------------------------------------------------------------------ unconstrained coordinates
@pytest.mark.parametrize("N, seed", [(97, 0), (400, 1), (1000, 2), (2500, 3), (LIMIT, 4), (700, 5)])
def test_float_selection_equals_the_oracle(hip, N, seed):
    rng = np.random.default_rng(1000 + seed)
    k, ka = (128, 128) if N >= 400 else (48, 24)
    cs = [blobs(rng, N, grid=False, segments=((1, 9), (2, 6))) for _ in range(3)]
    assert_equals_oracle(hip, cs, k, ka, min_gap=1e-5)


# ------------------------------------------------------------------ gather / scatter
@pytest.mark.parametrize("width", [1, 8, 16, 36, 180])
@pytest.mark.parametrize("shift", [0, 1])
def test_gather_and_scatter_are_torch_indexing(hip, width, shift):
    g = torch.Generator().manual_seed(width)
    B, N, rows, K = 5, 77, 9, 24
    buf = torch.randint(0, 256, (B * N * width + shift,), dtype=torch.uint8, generator=g)
    src = buf[shift:].view(B, N, width)  # shift = 1: an odd base address, byte lanes whatever the width
    index = torch.stack([torch.randperm(N, generator=g)[:K].sort().values for _ in range(rows)])
    index[:, K - 5:] = -1
    index[2] = -1
    cor = [0, 4, 4, 1, 3, 2, 0, 1, 4]
    src_d, idx_d = src.cuda(), index.cuda()
    src_d = src_d if shift == 0 else torch.cat([torch.zeros(shift, dtype=torch.uint8, device="cuda"), src_d.flatten()])[shift:].view(B, N, width)
    assert src_d.data_ptr() % 2 == shift
    dst = torch.full((rows, K, width), 0xAB, dtype=torch.uint8, device="cuda")
    _hip.check(hip.diffab_patch_gather(_hip.ptr(src_d), _hip.ptr(idx_d), (ctypes.c_int32 * rows)(*cor), B, N, rows, K, width, _hip.ptr(dst),
                                       _hip.stream_ptr()), "diffab_patch_gather")
    want = src[torch.tensor(cor)[:, None], index.clamp_min(0)] * (index >= 0)[..., None]
    assert torch.equal(dst.cpu(), want)
    # without the row map: row r reads complex r
    dst5 = torch.full((B, K, width), 0xAB, dtype=torch.uint8, device="cuda")
    _hip.check(hip.diffab_patch_gather(_hip.ptr(src_d), _hip.ptr(idx_d), None, B, N, B, K, width, _hip.ptr(dst5), _hip.stream_ptr()),
               "diffab_patch_gather")
    assert torch.equal(dst5.cpu(), src[torch.arange(B)[:, None], index[:B].clamp_min(0)] * (index[:B] >= 0)[..., None])
    # scatter(gather(x)) restores x on the patch and leaves the rest of a sentinel-filled destination untouched
    back = torch.full((rows, N, width), 0xCD, dtype=torch.uint8, device="cuda")
    _hip.check(hip.diffab_patch_scatter(_hip.ptr(dst), _hip.ptr(idx_d), None, rows, N, K, width, _hip.ptr(back), _hip.stream_ptr()),
               "diffab_patch_scatter")
    want_back = torch.full((rows, N, width), 0xCD, dtype=torch.uint8)
    for r in range(rows):
        sel = index[r][index[r] >= 0]
        want_back[r, sel] = src[cor[r], sel]
    assert torch.equal(back.cpu(), want_back)
    # a write mask keeps slots out
    wm = torch.rand(rows, K, generator=g) < 0.5
    back2 = torch.full((rows, N, width), 0xCD, dtype=torch.uint8, device="cuda")
    _hip.check(hip.diffab_patch_scatter(_hip.ptr(dst), _hip.ptr(idx_d), _hip.ptr(wm.cuda()), rows, N, K, width, _hip.ptr(back2),
                                        _hip.stream_ptr()), "diffab_patch_scatter")
    want2 = torch.full((rows, N, width), 0xCD, dtype=torch.uint8)
    for r in range(rows):
        sel = index[r][(index[r] >= 0) & wm[r]]
        want2[r, sel] = src[cor[r], sel]
    assert torch.equal(back2.cpu(), want2)


def test_many_rows_through_the_row_map(hip):
    """More rows than one launch's row map holds (256), 16-byte lanes."""
    g = torch.Generator().manual_seed(2)
    B, N, rows, K = 7, 50, 700, 16
    src = torch.randn(B, N, 12, generator=g)
    index = torch.randint(-1, N, (rows, K), generator=g)
    cor = torch.randint(0, B, (rows,), generator=g)
    got = patch._gather_rows(hip, src.cuda(), index.cuda(), cor.tolist())
    assert torch.equal(got.cpu(), src[cor[:, None], index.clamp_min(0)] * (index >= 0)[..., None])


# ------------------------------------------------------------------ python layer and end to end
def model_with_encoders(dims, seed):
    model = make_model(dims, seed)
    model.load_state_dict(syn.context_state_dict(dims["D"], dims["C"], 15, 32, seed=3), strict=False)
    return model


def complexes(B=2, N=600, seed=5):
    """Complexes built like synthetic.context_batch (its fields at N residues), with a 10-residue generated segment on the first chain
    and the third chain as the antigen; the pair fields are left out."""
    cb = {k: v for k, v in syn.context_batch(B, N, 15, seed=seed, with_distmat=False).items() if k not in ("distmat", "pairwise_dihedrals",
                                                                                                           "residue_idx")}
    gm = torch.zeros(B, N, dtype=torch.bool)
    for b in range(B):
        first = torch.nonzero(cb["chain_idx"][b] == 1).flatten()
        assert first.numel() > 40
        gm[b, int(first[10]) + 3 * b:int(first[10]) + 3 * b + 10] = True
    cb["generation_mask"] = gm
    cb["antigen_mask"] = cb["chain_idx"] == 3
    return cb


def by_hand(model, batch, **kw):
    sel = patch.select(batch["xyz"], batch["generation_mask"], k=128, antigen_mask=batch["antigen_mask"], chain_idx=batch["chain_idx"],
                       residue_mask=batch["residue_mask"])
    g = patch.gather(batch, sel)
    res = model.sample(g["seq_idx"], g["xyz"], g["orientations"], generation_mask=g["generation_mask"], residue_mask=g["residue_mask"],
                       atom_mask=g["atom_mask"], chain_idx=g["chain_idx"], residue_idx=g["residue_idx"],
                       backbone_dihedrals=g["backbone_dihedrals"], **kw)
    return sel, g, res


STATE = ("seq_idx", "translations", "orientations")


def test_python_select_and_gather_match_the_oracle_and_torch(hip):
    batch = complexes()
    sel = patch.select(batch["xyz"], batch["generation_mask"], k=100, k_antigen=60, antigen_mask=batch["antigen_mask"],
                       chain_idx=batch["chain_idx"], residue_mask=batch["residue_mask"])
    assert sel.index.shape == (2, 256) and sel.index.device == batch["xyz"].device  # 160 rounded up to pad_to = 128
    for b in range(2):
        wi, wm, wc, _ = select_ref(batch["xyz"][b, :, 1].numpy(), batch["generation_mask"][b].numpy(), 100, 60, 256,
                                   residue_mask=batch["residue_mask"][b].numpy(), chain=batch["chain_idx"][b].numpy(),
                                   antigen=batch["antigen_mask"][b].numpy(), dtype=np.float32)
        assert int(sel.count[b]) == wc and np.array_equal(sel.index[b].numpy(), wi) and np.array_equal(sel.mask[b].numpy(), wm)
    g = patch.gather(batch, sel)
    rows, safe, live = torch.arange(2)[:, None], sel.index.clamp_min(0), sel.index >= 0
    assert set(g) == set(batch) | {"residue_idx"} and "pairwise_dihedrals" not in g
    for name, v in batch.items():
        want = v[rows, safe] * live.view(2, 256, *([1] * (v.dim() - 2))).to(v.dtype)
        assert g[name].dtype == v.dtype and torch.equal(g[name], want), name
    assert torch.equal(g["residue_idx"], safe * live)  # the complex's numbering: arange(N) before the gather
    assert not bool(g["residue_mask"][~live].any())


def test_design_complex_end_to_end(hip):
    dims = dict(syn.BENCH_DIMS, NL=2)
    model = model_with_encoders(dims, 9)
    batch = complexes()
    kw = dict(seed=31, num_samples=4, t_start=12, t_stop=5)
    out = model.design_complex(batch, **kw)
    sel, g, res = by_hand(model, batch, **kw)
    for name in STATE:
        assert out[name].shape[:2] == (8, 256) and torch.equal(out[name], res[name]), name
    for got, want in zip(out["patch"], sel):
        assert torch.equal(got, want)
    assert 128 < int(sel.count.min()) and int(sel.count.max()) < 256  # the two passes overlap: the rows end in unused slots
    # the pasted complex: the native outside the generated residues, the design inside
    native = {"seq_idx": batch["seq_idx"], "translations": batch["xyz"][:, :, 1], "orientations": batch["orientations"]}
    changed = 0
    for r in range(8):
        c = r // 4
        gen = batch["generation_mask"][c] & batch["residue_mask"][c]
        slot = {int(i): p for p, i in enumerate(sel.index[c].tolist()) if i >= 0}
        assert all(int(i) in slot for i in torch.nonzero(gen).flatten())
        for name in STATE:
            full = out["complex"][name][r]
            assert full.shape[0] == 600 and torch.equal(full[~gen], native[name][c][~gen]), (r, name)
            for i in torch.nonzero(gen).flatten().tolist():
                assert torch.equal(full[i], out[name][r, slot[i]]), (r, name, i)
            changed += int((full[gen] != native[name][c][gen]).any())
    assert changed == 24  # every design row differs from the native in every modality

    # 300 more residues at the END of the arrays, farther from every anchor than anything in the patch: no output bit changes
    def extended(name, v):
        tail = torch.zeros((2, 300) + tuple(v.shape[2:]), dtype=v.dtype)
        if name == "xyz":
            tail = 400.0 + 3.0 * torch.randn(2, 300, 15, 3, generator=torch.Generator().manual_seed(1))
        elif name == "orientations":
            tail = torch.eye(3).expand(2, 300, 3, 3).clone()
        elif name in ("chain_idx",):
            tail += 3
        elif name in ("atom_mask", "residue_mask", "antigen_mask"):
            tail = torch.ones_like(tail)
        return torch.cat([v, tail], 1)

    big = {name: extended(name, v) for name, v in batch.items()}
    out2 = model.design_complex(big, **kw)
    for name in STATE:
        assert torch.equal(out2[name], out[name]), name
        assert torch.equal(out2["complex"][name][:, :600], out["complex"][name]), name
    for got, want in zip(out2["patch"], out["patch"]):
        assert torch.equal(got, want)


def test_the_sampler_sees_the_numbering_of_the_complex(hip):
    """A numbering gap inside the generated segment: under bond guidance the design differs from the same call made with
    residue_idx = arange(K), and is bitwise the hand-made call that passes the gathered numbering."""
    dims = dict(syn.BENCH_DIMS, NL=2)
    model = model_with_encoders(dims, 9)
    batch = complexes()
    ridx = torch.arange(600).repeat(2, 1)
    for b in range(2):
        start = int(torch.nonzero(batch["generation_mask"][b]).flatten()[0])
        ridx[b, start + 5:] += 7
    batch["residue_idx"] = ridx
    kw = dict(seed=4, t_start=20, t_stop=0, guidance=SampleGuidance(bond=1.0))
    out = model.design_complex(batch, **kw)
    sel, g, res = by_hand(model, batch, **kw)
    assert torch.equal(g["residue_idx"], torch.gather(ridx, 1, sel.index.clamp_min(0)) * (sel.index >= 0))
    for name in STATE:
        assert torch.equal(out[name], res[name]), name
    plain = model.sample(g["seq_idx"], g["xyz"], g["orientations"], generation_mask=g["generation_mask"], residue_mask=g["residue_mask"],
                         atom_mask=g["atom_mask"], chain_idx=g["chain_idx"], residue_idx=torch.arange(256).unsqueeze(0),
                         backbone_dihedrals=g["backbone_dihedrals"], **kw)
    assert not torch.equal(plain["translations"], out["translations"])
