"""The module launch runs the last layer of a reverse step by the call's row plan: 16-row attention items that start at the first
generated row not yet covered (clamped to K - 16) instead of the aligned row tiles with a generated residue - by default, wherever the
sampler skips unread rows - and the heads of that launch only on the 32-row slabs with a generated residue.  A row's bits depend neither
on the item that carries it nor on the wave that computes it, so every comparison here is bitwise (torch.equal on
seq / x / O, and on every record, after >= 5 reverse steps from diffab_sample_init), as in test_gpu_skip_rows_module.py: default against
skip_unused_rows=False (every item, every row), and the module launch against DIFFAB_FLAG_MULTI_LAUNCH (which keeps the tile map).

The plan itself (diffab_debug_row_plan) is checked against a host greedy.  Its slab word has one bit per 32 rows, (K + 31) / 32 of them:
K = 16 is ONE slab (bit 0), not a refused shape."""
import pytest
import torch

from diffab_pytorch import _hip, synthetic as syn
from diffab_pytorch.guidance import SampleGuidance
from diffab_pytorch.steering import ParticleSteering
from diffab_pytorch.temperature import SampleTemperature
from sampler_support import assert_bitwise, hip, make_model, patches, sample

pytestmark = pytest.mark.gpu
MODULE = _hip.FLAG_PERSISTENT_MODULE
STEPS = dict(t_start=60, t_stop=54)


@pytest.fixture(scope="module")
def models(hip):
    """NL = 2: the module's result leaves in xa; NL = 3: in xb.  The last layer is never the first."""
    out = {}
    for NL in (2, 3):
        dims = dict(syn.BENCH_DIMS, NL=NL)
        out[NL] = (dims, make_model(dims, 31 + NL))
    return out


@pytest.fixture(scope="module")
def inputs8(models):
    return {NL: patches(8, 128, models[NL][0], seed=140 + NL) for NL in models}


def _segment(B, K, spans):
    gm = torch.zeros(B, K, dtype=torch.bool)
    for lo, hi in spans:
        gm[:, lo:hi] = True
    return gm


def _mixed(synthetic_mask):
    gm = synthetic_mask.clone()
    gm[0], gm[1] = False, True  # a patch with nothing to generate and one with everything next to the synthetic segments
    return gm


def _masks(B, K, synthetic_mask):
    """name -> ((B, K) generation mask, the plan's start rows of every patch or None)"""
    return {
        "rows_12_20": (_segment(B, K, [(12, 21)]), [12]),                    # two aligned tiles, one window
        "rows_110_127": (_segment(B, K, [(K - 18, K)]), [K - 18, K - 16]),   # the second start is clamped: the windows overlap
        "row_127": (_segment(B, K, [(K - 1, K)]), [K - 16]),
        "rows_31_32": (_segment(B, K, [(31, 33)]), [31]),                    # two slabs, one window
        "two_segments": (_segment(B, K, [(5, 12), (K - 30, K - 18)]), [5, K - 30]),
        "none": (torch.zeros(B, K, dtype=torch.bool), []),
        "all": (torch.ones(B, K, dtype=torch.bool), list(range(0, K, 16))),  # the aligned tiles
        "mixed": (_mixed(synthetic_mask), None),
    }


def _host_plan(gm):
    """The greedy covering and the slab bits of a (B, K) mask, on the host."""
    B, K = gm.shape
    starts, slabs = [], []
    for b in range(B):
        s_b, covered, bits = [], 0, 0
        for i in torch.nonzero(gm[b]).flatten().tolist():
            bits |= 1 << (i // 32)
            if i >= covered:
                s_b.append(min(i, K - 16))
                covered = s_b[-1] + 16
        starts.append(s_b)
        slabs.append(bits)
    return starts, slabs


def _device_plan(hip, gm):
    B, K = gm.shape
    plan = torch.full((B, 2 + K // 16), 77, dtype=torch.int32, device="cuda")
    _hip.check(hip.diffab_debug_row_plan(_hip.ptr(gm.cuda()), B, K, _hip.ptr(plan), _hip.stream_ptr()), "row_plan")
    plan = plan.cpu()
    n = plan[:, 0].tolist()
    assert all(0 <= v <= K // 16 for v in n), n
    for b in range(B):
        assert bool((plan[b, 2 + n[b]:] == -1).all()), (b, plan[b])
    return [plan[b, 2:2 + n[b]].tolist() for b in range(B)], [v & 0xFFFFFFFF for v in plan[:, 1].tolist()]


def _run(model, inp, gm, flags, **kw):
    inp = dict(inp, generation_mask=gm.cuda())
    if "residue_mask" in inp:  # (the guidance tables: a generated residue is a real one)
        inp["residue_mask"] = inp["residue_mask"] | gm.cuda()
    return sample(model, inp, flags=flags, **kw)


def _three_ways(model, inp, gm, what, **kw):
    """default | all rows | per-layer launches | per-layer launches with all rows: the same result, bit for bit"""
    kw = dict(dict(seed=11, **STEPS), **kw)
    base = _run(model, inp, gm, MODULE, **kw)
    assert_bitwise(base, _run(model, inp, gm, MODULE, skip_unused_rows=False, **kw), (what, "default vs all rows"))
    assert_bitwise(base, _run(model, inp, gm, _hip.FLAG_MULTI_LAUNCH, **kw), (what, "module vs per-layer launches"))
    assert_bitwise(base, _run(model, inp, gm, _hip.FLAG_MULTI_LAUNCH, skip_unused_rows=False, **kw), (what, "module vs per-layer, all rows"))
    for k in ("translations", "orientations"):
        assert torch.isfinite(base[k]).all(), (what, k)
    return base


def test_row_plan_is_the_greedy_covering(hip):
    for B, K in ((3, 128), (2, 256), (5, 16)):
        g = torch.Generator().manual_seed(B * K + 1)
        gm = torch.rand(B, K, generator=g) < 0.04
        gm[0] = False
        gm[-1, K - 1] = True
        if K > 16:
            gm[1, 15:17] = True      # across a tile boundary: one window
            gm[1, K - 18:] = True    # the clamped start
        starts, slabs = _device_plan(hip, gm)
        want_starts, want_slabs = _host_plan(gm)
        assert starts == want_starts, (B, K)
        assert slabs == want_slabs, (B, K)
        tiles = gm.view(B, K // 16, 16).any(-1).sum(1).tolist()
        for b in range(B):
            covered = torch.zeros(K, dtype=torch.bool)
            for s in starts[b]:
                assert 0 <= s <= K - 16
                covered[s:s + 16] = True
            assert bool(covered[gm[b]].all()), (B, K, b)
            assert len(starts[b]) <= tiles[b], (B, K, b)
        if K % 32 == 0:
            bits = gm.view(B, K // 32, 32).any(-1)
            assert [[bool(slabs[b] >> s & 1) for s in range(K // 32)] for b in range(B)] == bits.tolist(), (B, K)
        else:  # K = 16: one slab
            assert slabs == [int(v) for v in gm.any(-1).tolist()], (B, K)


def test_row_plan_of_the_test_masks(hip, models, inputs8):
    K = 128
    for name, (gm, want) in _masks(8, K, inputs8[2]["generation_mask"].cpu()).items():
        starts, slabs = _device_plan(hip, gm)
        if want is not None:
            assert starts == [want] * 8, name
        if name == "all":
            assert slabs == [(1 << (K // 32)) - 1] * 8
        if name == "none":
            assert slabs == [0] * 8
        if name == "rows_31_32":
            assert slabs == [0b11] * 8
        if name == "mixed":
            assert starts[0] == [] and starts[1] == list(range(0, K, 16)) and slabs[0] == 0 and slabs[1] == 15
            assert all(1 <= len(s) <= 2 for s in starts[2:]), starts


@pytest.mark.parametrize("NL", [2, 3])
@pytest.mark.parametrize("name", ["rows_12_20", "rows_110_127", "row_127", "rows_31_32", "two_segments", "none", "all", "mixed"])
def test_last_layer_items_at_their_start_rows_k128(models, inputs8, NL, name):
    _, model = models[NL]
    inp = inputs8[NL]
    gm, _ = _masks(8, 128, inp["generation_mask"].cpu())[name]
    out = _three_ways(model, inp, gm, (NL, name))
    for k in ("translations", "seq_idx", "orientations"):
        assert torch.equal(out[k].cpu()[~gm], inp[k].cpu()[~gm]), (NL, name, k)
    if name == "none":
        for k in ("translations", "seq_idx", "orientations"):
            assert torch.equal(out[k], inp[k]), (NL, k, "no generated residue: the state is the input")


def test_work_groups_that_walk_two_patches(models):
    dims, model = models[3]
    inp = patches(264, 128, dims, seed=304)
    _three_ways(model, inp, inp["generation_mask"].cpu(), "B = 264")


def test_k256(models):
    dims, model = models[3]
    B, K = 8, 256
    inp = patches(B, K, dims, seed=157)
    for name, gm in (("straddle", _segment(B, K, [(K // 2 - 3, K // 2 + 4)])), ("two_segments", _segment(B, K, [(5, 12), (K - 30, K - 18)]))):
        _three_ways(model, inp, gm, (K, name))


def test_shared_contexts(models):
    dims, model = models[3]
    inp = patches(4, 128, dims, seed=163)
    for gm in (inp["generation_mask"].cpu(), _segment(4, 128, [(12, 21)])):
        out = _three_ways(model, inp, gm, "shared contexts", num_samples=2)
        assert out["translations"].shape[0] == 8
        assert not torch.equal(out["translations"][0], out["translations"][1])  # two designs of patch 0


def test_graph_then_another_mask_on_the_same_workspace(models, inputs8):
    _, model = models[3]
    inp = inputs8[3]
    gm = inp["generation_mask"].cpu()
    kw = dict(seed=11, t_start=60, t_stop=52)
    eager = _run(model, inp, gm, MODULE, graph=False, **kw)
    assert_bitwise(eager, _run(model, inp, gm, MODULE, graph=True, **kw), "graph vs eager")
    assert_bitwise(eager, _run(model, inp, gm, MODULE, graph=True, skip_unused_rows=False, **kw), "graph, all rows vs eager")
    gm2 = _segment(8, 128, [(110, 128)])  # the plan is the call's own
    assert_bitwise(_run(model, inp, gm2, MODULE, graph=True, **kw),
                   _run(model, inp, gm2, _hip.FLAG_MULTI_LAUNCH, skip_unused_rows=False, **kw), "graph, second mask")


@pytest.mark.parametrize("option", ["guidance", "trajectory", "allowed_aa", "temperature", "steps", "steering"])
def test_options_that_read_the_step_outputs(models, option):
    """guidance reads x0_hat, the record the predictions, allowed_aa the posterior, temperature O0_hat and the posterior, a jump the
    posterior (rewritten in place) and steering eps_hat for its energy - each behind the generation mask"""
    dims, model = models[3]
    inp = patches(8, 128, dims, seed=171, chains=option in ("guidance", "steering"))
    mix = lambda v: torch.tensor(v * 2)  # per row: lambda_x, lambda_O (two stacked tables and a zero row), tau
    kw = {"guidance": dict(guidance=SampleGuidance(clash=2.0, bond=1.0, max_shift=0.5)),
          "trajectory": dict(trajectory=True, trajectory_predictions=True),
          "allowed_aa": dict(allowed_aa=torch.rand(8, 128, 21, generator=torch.Generator().manual_seed(3)) < 0.6),
          "temperature": dict(temperature=SampleTemperature(mix([1.5, 0.0, 1.0, 0.5]), mix([0.0, 0.3, 0.6, 1.0]), mix([0.5, 1.0, 0.0, 2.0]))),
          "steps": dict(steps=[60, 58, 57, 54], t_stop=53),
          "steering": dict(num_samples=2, steering=ParticleSteering(strength=0.05, ess_threshold=2.0))}[option]
    moved = 0
    for gm in (inp["generation_mask"].cpu(), _segment(8, 128, [(110, 128)])):
        out = _three_ways(model, inp, gm, option, **kw)
        if option == "steering":
            moved += int((out["steering"]["ancestors"].cpu() != torch.arange(16)).sum())
    assert option != "steering" or moved > 0, "some row must move for this case to say anything"
