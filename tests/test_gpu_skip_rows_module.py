"""The reverse sampler skips the last layer's attention items whose 16 rows hold no generated residue - by default, on the module launch
(ipa_persistent.hip) and on the per-layer launches alike.  Every comparison here is bitwise (torch.equal on seq / x / O after >= 5
reverse steps from diffab_sample_init), three ways: default against DIFFAB_FLAG_ALL_ROWS, module launch against
DIFFAB_FLAG_MULTI_LAUNCH, and both together."""
import ctypes as C

import pytest
import torch

from diffab_pytorch import DiffAb, _hip, synthetic as syn
from sampler_support import hip

pytestmark = pytest.mark.gpu
STATE = ("seq_idx", "translations", "orientations")


@pytest.fixture(scope="module")
def model(hip):
    bd = dict(syn.BENCH_DIMS, NL=3)  # odd NL: the module's result leaves in xb; the last layer is not the first
    torch.manual_seed(0)
    return bd, DiffAb(bd["D"], bd["C"], bd["NL"], bd["DS"], bd["PQ"], bd["PV"], bd["H"]).cuda()


def _segment(B, K, spans):
    gm = torch.zeros(B, K, dtype=torch.bool)
    for lo, hi in spans:
        gm[:, lo:hi] = True
    return gm


def _masks(B, K, synthetic_mask):
    """name -> (B, K) generation mask: the cases the skip has to get right."""
    return {
        "synthetic": synthetic_mask,                              # one CDR-like segment of 5-20 residues per patch
        "none": torch.zeros(B, K, dtype=torch.bool),              # zero items of the last layer run
        "all": torch.ones(B, K, dtype=torch.bool),                # every item runs
        "straddle": _segment(B, K, [(K // 2 - 3, K // 2 + 4)]),   # a segment across a tile boundary (two tiles)
        "two_segments": _segment(B, K, [(5, 12), (K - 30, K - 18)]),
    }


def _same(a, b, what):
    for k in STATE:
        assert torch.equal(a[k], b[k]), (what, k)


def _three_ways(model, bi, gm, what, module_flag=0, **kw):
    """default | all rows | per-layer launches | per-layer launches with all rows: the same state, bit for bit"""
    args = (bi["seq_idx"], bi["translations"], bi["orientations"])
    kw = dict(dict(res_context_emb=bi["res_context_emb"], pair_context_emb=bi["pair_context_emb"], generation_mask=gm.cuda(), seed=11,
                   t_start=60, t_stop=54), **kw)
    base = model.sample(*args, flags=module_flag, **kw)
    _same(base, model.sample(*args, flags=module_flag, skip_unused_rows=False, **kw), (what, "default vs all rows"))
    _same(base, model.sample(*args, flags=_hip.FLAG_MULTI_LAUNCH, **kw), (what, "module vs per-layer launches"))
    _same(base, model.sample(*args, flags=_hip.FLAG_MULTI_LAUNCH, skip_unused_rows=False, **kw), (what, "module, skipping vs per-layer, all rows"))
    for k in ("translations", "orientations"):
        assert torch.isfinite(base[k]).all(), (what, k)
    return base


def test_row_tile_map_is_any_over_16_rows(hip):
    """The map the sampler builds per call from generation_mask, for hand-written masks (the builder is a device kernel)."""
    for B, K in ((3, 128), (2, 256), (5, 16)):
        g = torch.Generator().manual_seed(B * K)
        gm = torch.rand(B, K, generator=g) < 0.03
        gm[0] = False
        gm[-1, K - 1] = True
        if K > 16:
            gm[1, 15:17] = True  # the last row of one tile and the first of the next
        dev, tiles = gm.cuda(), torch.full((B, K // 16), 7, dtype=torch.uint8, device="cuda")
        _hip.check(hip.diffab_debug_row_tiles(_hip.ptr(dev), B, K, _hip.ptr(tiles), _hip.stream_ptr()), "row_tiles")
        assert torch.equal(tiles.cpu().bool(), gm.view(B, K // 16, 16).any(-1)), (B, K)
        assert int(tiles.max()) <= 1


@pytest.mark.parametrize("B", [8, 256, 264])
def test_module_launch_skips_unread_tiles_k128(model, B):
    """K = 128; B = 8 takes the module launch on request, 256 by the loop's own choice, 264 has work-groups that walk two patches."""
    bd, m = model
    bi = {k: v.cuda() for k, v in syn.patches(B, 128, bd, seed=40 + B).items()}
    flag = _hip.FLAG_PERSISTENT_MODULE
    names = ("synthetic", "none", "all", "straddle", "two_segments") if B == 8 else ("synthetic", "two_segments")
    masks = _masks(B, 128, bi["generation_mask"].cpu())
    for name in names:
        gm = masks[name]
        if name == "synthetic":  # mixed in one launch: a patch with nothing to generate, one with everything
            gm = gm.clone()
            gm[0], gm[1] = False, True
            run = gm.view(B, 8, 16).any(-1).float().mean().item()
            assert 0.1 < run < 0.5, run
        out = _three_ways(m, bi, gm, (B, name), module_flag=flag)
        assert torch.equal(out["translations"].cpu()[~gm], bi["translations"].cpu()[~gm]), (B, name)
        assert torch.equal(out["seq_idx"].cpu()[~gm], bi["seq_idx"].cpu()[~gm]), (B, name)
        if name == "none":
            _same(out, bi, (B, "no generated residue: the state is the input"))


def test_module_launch_skips_unread_tiles_k256(model):
    """K = 256 (NTILE = 16, two dense tiles, two-chunk attention items) with DIFFAB_FLAG_PERSISTENT_MODULE"""
    bd, m = model
    B, K = 8, 256
    bi = {k: v.cuda() for k, v in syn.patches(B, K, bd, seed=57).items()}
    for name, gm in _masks(B, K, bi["generation_mask"].cpu()).items():
        out = _three_ways(m, bi, gm, (K, name), module_flag=_hip.FLAG_PERSISTENT_MODULE)
        if name == "none":
            _same(out, bi, (K, "no generated residue: the state is the input"))


def test_shared_contexts_skip_unread_tiles(model):
    """shared contexts (diffab_sample_options.ctx_of_row): N samples per context read the pair rows through ctx_of_row; the tile map is per state row"""
    bd, m = model
    B, N = 4, 2
    bi = {k: v.cuda() for k, v in syn.patches(B, 128, bd, seed=63).items()}
    for name in ("synthetic", "straddle"):
        gm = _masks(B, 128, bi["generation_mask"].cpu())[name]
        out = _three_ways(m, bi, gm, ("shared", name), module_flag=_hip.FLAG_PERSISTENT_MODULE, num_samples=N)
        assert out["translations"].shape[0] == B * N
        assert not torch.equal(out["translations"][0], out["translations"][1])  # two designs of patch 0


@pytest.mark.parametrize("mode", ["codesign", "fixed_backbone", "structure"])
def test_design_modes_skip_unread_tiles(model, mode):
    bd, m = model
    bi = {k: v.cuda() for k, v in syn.patches(8, 128, bd, seed=71).items()}
    gm = bi["generation_mask"].cpu()
    out = _three_ways(m, bi, gm, mode, module_flag=_hip.FLAG_PERSISTENT_MODULE, mode=mode)
    if mode == "fixed_backbone":
        assert torch.equal(out["translations"], bi["translations"])
    if mode == "structure":
        assert torch.equal(out["seq_idx"], bi["seq_idx"])


def test_graph_sampler_skips_unread_tiles(model):
    """DIFFAB_FLAG_GRAPH_SAMPLER: the captured step carries the map's pointer; the map is built once per call, before the capture"""
    bd, m = model
    bi = {k: v.cuda() for k, v in syn.patches(8, 128, bd, seed=83).items()}
    gm = bi["generation_mask"].cpu()
    args = (bi["seq_idx"], bi["translations"], bi["orientations"])
    kw = dict(res_context_emb=bi["res_context_emb"], pair_context_emb=bi["pair_context_emb"], generation_mask=gm.cuda(), seed=11, t_start=60,
              t_stop=52)
    for flag in (_hip.FLAG_PERSISTENT_MODULE, _hip.FLAG_MULTI_LAUNCH):
        eager = m.sample(*args, flags=flag, graph=False, **kw)
        _same(eager, m.sample(*args, flags=flag, graph=True, **kw), (flag, "graph vs eager"))
        _same(eager, m.sample(*args, flags=flag, graph=True, skip_unused_rows=False, **kw), (flag, "graph, all rows vs eager"))
    # a second call with another mask on the same workspace: the map is the call's own
    gm2 = _masks(8, 128, gm)["two_segments"]
    kw2 = dict(kw, generation_mask=gm2.cuda())
    _same(m.sample(*args, flags=_hip.FLAG_PERSISTENT_MODULE, graph=True, **kw2),
          m.sample(*args, flags=_hip.FLAG_MULTI_LAUNCH, skip_unused_rows=False, **kw2), "graph, second mask")


def test_skip_flag_of_old_callers_is_accepted(model):
    """DIFFAB_FLAG_SKIP_UNUSED_ROWS (256) changes nothing any more, and does not force the per-layer launches"""
    bd, m = model
    bi = {k: v.cuda() for k, v in syn.patches(8, 128, bd, seed=91).items()}
    args = (bi["seq_idx"], bi["translations"], bi["orientations"])
    kw = dict(res_context_emb=bi["res_context_emb"], pair_context_emb=bi["pair_context_emb"], generation_mask=bi["generation_mask"], seed=3,
              t_start=30, t_stop=25)
    _same(m.sample(*args, flags=_hip.FLAG_PERSISTENT_MODULE | _hip.FLAG_SKIP_UNUSED_ROWS, **kw),
          m.sample(*args, flags=_hip.FLAG_PERSISTENT_MODULE, skip_unused_rows=False, **kw), "flag 256")
