"""The MLP phases of the module launch under a row plan: the three heads of every 32-row slab with a generated residue run in one pass
of the slab form (csrc/mlp_chain_slab.h: a (head, 64-column half) unit on each of six waves, weight fragments from global memory,
two slabs to a pass) instead of three chain tiles behind one another.  A row's bits depend neither on the wave that computes its unit
nor on how many slabs run, so every comparison is bitwise (torch.equal on seq / x / O after >= 5 reverse steps from diffab_sample_init, so that later steps read what
earlier ones left and the sequences of the live rows have changed): the module launch's default against skip_unused_rows=False (every
row through the chain tile), against DIFFAB_FLAG_MULTI_LAUNCH (the per-layer chain kernels) and against both together."""
import pytest
import torch

from diffab_pytorch import _hip, synthetic as syn
from diffab_pytorch.steering import ParticleSteering
from sampler_support import assert_bitwise, hip, make_model, patches, sample, segment_mask, slab_mask  # noqa: F401 (hip: the device fixture)

pytestmark = pytest.mark.gpu
MODULE = _hip.FLAG_PERSISTENT_MODULE
STEPS = dict(t_start=60, t_stop=54)  # six reverse steps
K = 128


@pytest.fixture(scope="module")
def models(hip):
    """NL = 2: the module's result leaves in xa; NL = 3: in xb."""
    out = {}
    for NL in (2, 3):
        dims = dict(syn.BENCH_DIMS, NL=NL)
        out[NL] = (dims, make_model(dims, 41 + NL))
    return out


@pytest.fixture(scope="module")
def inputs8(models):
    return {NL: patches(8, K, models[NL][0], seed=240 + NL) for NL in models}


def _run(model, inp, gm, flags, **kw):
    inp = dict(inp, generation_mask=gm.cuda())
    if "residue_mask" in inp:  # (the steering tables: a generated residue is a real one)
        inp["residue_mask"] = inp["residue_mask"] | gm.cuda()
    return sample(model, inp, flags=flags, **kw)


def _three_ways(model, inp, gm, what, **kw):
    kw = dict(dict(seed=13, **STEPS), **kw)
    base = _run(model, inp, gm, MODULE, **kw)
    assert_bitwise(base, _run(model, inp, gm, MODULE, skip_unused_rows=False, **kw), (what, "default vs all rows"))
    assert_bitwise(base, _run(model, inp, gm, _hip.FLAG_MULTI_LAUNCH, **kw), (what, "module vs per-layer launches"))
    assert_bitwise(base, _run(model, inp, gm, _hip.FLAG_MULTI_LAUNCH, skip_unused_rows=False, **kw), (what, "module vs per-layer, all rows"))
    for k in ("translations", "orientations"):
        assert torch.isfinite(base[k]).all(), (what, k)
    return base


@pytest.mark.parametrize("NL", [2, 3])
@pytest.mark.parametrize("name", ["one_slab", "two_adjacent_slabs", "slabs_0_and_3", "three_slabs", "row_127", "none", "all", "mixed"])
def test_heads_on_live_slabs(models, inputs8, NL, name):
    _, model = models[NL]
    inp = inputs8[NL]
    gm = slab_mask(name, 8, K, inp["generation_mask"].cpu())
    out = _three_ways(model, inp, gm, (NL, name))
    for k in ("translations", "seq_idx", "orientations"):
        assert torch.equal(out[k].cpu()[~gm], inp[k].cpu()[~gm]), (NL, name, k)
    if name == "none":
        for k in ("translations", "seq_idx", "orientations"):
            assert torch.equal(out[k], inp[k]), (NL, k, "no generated residue: the state is the input")
    elif name != "row_127":  # (one residue may keep its type)
        assert not torch.equal(out["seq_idx"], inp["seq_idx"]), (NL, name, "the live rows' sequences must have changed")


def test_work_groups_that_walk_two_patches(models):
    """B = 264 > the work-groups of the launch: the images of a work-group's second patch must not carry the first's."""
    dims, model = models[3]
    inp = patches(264, K, dims, seed=404)
    _three_ways(model, inp, inp["generation_mask"].cpu(), "B = 264")


@pytest.mark.parametrize("graph", [False, True])
def test_second_call_on_the_same_workspace(models, inputs8, graph):
    """The second call has another mask and another sequence on the rows it keeps fixed: nothing of the first call may survive.  Its
    reference is a fresh model's per-layer, all-rows run."""
    dims, model = models[3]
    inp = inputs8[3]
    kw = dict(seed=13, t_start=60, t_stop=52)
    gm1 = inp["generation_mask"].cpu()
    first = _run(model, inp, gm1, MODULE, graph=graph, **kw)
    fresh = make_model(dims, 41 + 3)
    assert_bitwise(first, _run(fresh, inp, gm1, _hip.FLAG_MULTI_LAUNCH, skip_unused_rows=False, **kw), ("first call", graph))
    gm2 = segment_mask(8, K, [(40, 52), (110, 128)])
    inp2 = dict(inp, seq_idx=(inp["seq_idx"] + 7) % 20)  # every row's type moves, the fixed rows' with it
    second = _run(model, inp2, gm2, MODULE, graph=graph, **kw)
    assert_bitwise(second, _run(fresh, inp2, gm2, _hip.FLAG_MULTI_LAUNCH, skip_unused_rows=False, **kw), ("second call", graph))
    assert torch.equal(second["seq_idx"].cpu()[~gm2], inp2["seq_idx"].cpu()[~gm2])


def test_shared_contexts(models):
    dims, model = models[3]
    inp = patches(4, K, dims, seed=263)
    for gm in (inp["generation_mask"].cpu(), segment_mask(4, K, [(31, 33)])):
        out = _three_ways(model, inp, gm, "shared contexts", num_samples=2)
        assert out["translations"].shape[0] == 8
        assert not torch.equal(out["translations"][0], out["translations"][1])  # two designs of patch 0


def test_steering_moves_whole_rows(models):
    """steer_gather_kernel copies whole state rows between the designs of a patch."""
    dims, model = models[3]
    inp = patches(8, K, dims, seed=271, chains=True)
    kw = dict(num_samples=2, steering=ParticleSteering(strength=0.05, ess_threshold=2.0))
    moved = 0
    for gm in (inp["generation_mask"].cpu(), segment_mask(8, K, [(110, 128)])):
        out = _three_ways(model, inp, gm, "steering", **kw)
        moved += int((out["steering"]["ancestors"].cpu() != torch.arange(16)).sum())
    assert moved > 0, "some ancestor must differ from the identity for this case to say anything"


def test_allowed_aa_reads_the_posterior(models):
    """the seq head's narrow last layer (21 of 32 columns of its only unit) feeds the constrained posterior"""
    dims, model = models[3]
    inp = patches(8, K, dims, seed=277)
    allowed = torch.rand(8, K, 21, generator=torch.Generator().manual_seed(5)) < 0.6
    for gm in (inp["generation_mask"].cpu(), segment_mask(8, K, [(31, 33)])):
        _three_ways(model, inp, gm, "allowed_aa", allowed_aa=allowed)
