"""The end of a reverse step's module launch under a row plan (K = 128): the launch starts its work-groups by last-layer work
(csrc/denoiser_internal.h start_class_of).  Given the row plan, patches are ranked by descending (items, live slabs) and
class = rank * classes / B; a work-group waits class x 10 us before its first phase, so the patches with the most last-layer work
start first and their extra items end inside the launch instead of at its end.

That is timing only.  No result may depend on it: the module launch (which reads the class bytes) is compared bitwise (torch.equal on
seq / x / O after six reverse steps) against skip_unused_rows=False (no plan: the static classes), against DIFFAB_FLAG_MULTI_LAUNCH
(the per-layer launches, no classes at all) and against both, at masks with no live slab, every slab and mixed work, on a second
call on the same workspace (eager and replayed from a graph), on two calls that continue one trajectory, on a poisoned workspace (the
class bytes live in it and are rebuilt per call), in the design modes, with shared contexts, under steering and with more patches
than work-groups.

The assignment itself is checked on the host, without a device: diffab_debug_start_classes (include/diffab_hip_debug.h, a test hook
outside the public C ABI) runs the device kernel's own function on a host plan; on the device the same entry enqueues the sampler's
kernel, whose bytes must equal the host's."""
import ctypes as C

import numpy as np
import pytest
import torch

import scratch_poison
from diffab_pytorch import _hip, synthetic as syn
from diffab_pytorch.steering import ParticleSteering
from sampler_support import assert_bitwise, hip, make_model, patches, sample, segment_mask, slab_mask  # noqa: F401 (hip: the device fixture)

gpu = pytest.mark.gpu  # (per test: the start-class tests at the end of the file run on the host)
MODULE = _hip.FLAG_PERSISTENT_MODULE
STEPS = dict(t_start=60, t_stop=54)  # six reverse steps
K = 128
STATE = ("seq_idx", "translations", "orientations")


@pytest.fixture(scope="module")
def models(hip):
    """NL = 2: the module's result leaves in xa; NL = 3: in xb."""
    out = {}
    for NL in (2, 3):
        dims = dict(syn.BENCH_DIMS, NL=NL)
        out[NL] = (dims, make_model(dims, 51 + NL))
    return out


@pytest.fixture(scope="module")
def inputs8(models):
    return {NL: patches(8, K, models[NL][0], seed=340 + NL) for NL in models}


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


def _mask(name, inp):
    if name == "straddle":  # one generated residue on each side of the boundary between slabs 0 and 1
        return segment_mask(8, K, [(31, 33)])
    return slab_mask(name, 8, K, inp["generation_mask"].cpu())


@gpu
@pytest.mark.parametrize("NL", [2, 3])
@pytest.mark.parametrize("name", ["one_slab", "two_adjacent_slabs", "slabs_0_and_3", "three_slabs", "row_127", "none", "all", "mixed",
                                  "straddle"])
def test_start_classes_do_not_show_in_the_results(models, inputs8, NL, name):
    """equal work in every patch (the static order), no item at all, eight items, and patches of different work (mixed)"""
    _, model = models[NL]
    inp = inputs8[NL]
    gm = _mask(name, inp)
    out = _three_ways(model, inp, gm, (NL, name))
    for k in STATE:
        assert torch.equal(out[k].cpu()[~gm], inp[k].cpu()[~gm]), (NL, name, k)


@gpu
@pytest.mark.parametrize("graph", [False, True])
def test_second_call_on_the_same_workspace(models, inputs8, graph):
    """The second call has another mask, so other classes: it finds the first call's bytes in the workspace and must build its own
    (in front of any graph capture).  Each call's reference is a fresh model's per-layer, all-rows run."""
    dims, model = models[3]
    inp = inputs8[3]
    kw = dict(seed=13, **STEPS)
    gm1 = slab_mask("mixed", 8, K, inp["generation_mask"].cpu())
    first = _run(model, inp, gm1, MODULE, graph=graph, **kw)
    fresh = make_model(dims, 51 + 3)
    assert_bitwise(first, _run(fresh, inp, gm1, _hip.FLAG_MULTI_LAUNCH, skip_unused_rows=False, **kw), ("first call", graph))
    gm2 = segment_mask(8, K, [(40, 52), (110, 128)])
    inp2 = dict(inp, seq_idx=(inp["seq_idx"] + 7) % 20)
    second = _run(model, inp2, gm2, MODULE, graph=graph, **kw)
    assert_bitwise(second, _run(fresh, inp2, gm2, _hip.FLAG_MULTI_LAUNCH, skip_unused_rows=False, **kw), ("second call", graph))


@gpu
@pytest.mark.parametrize("NL", [2, 3])
def test_two_calls_continue_one_trajectory(models, inputs8, NL):
    """60 -> 57 and 57 -> 54 as two calls equal the single call"""
    _, model = models[NL]
    inp = inputs8[NL]
    gm = slab_mask("mixed", 8, K, inp["generation_mask"].cpu())
    whole = _run(model, inp, gm, MODULE, seed=13, **STEPS)
    half = _run(model, inp, gm, MODULE, seed=13, t_start=60, t_stop=57)
    rest = _run(model, dict(inp, **{k: half[k] for k in STATE}), gm, MODULE, seed=13, t_start=57, t_stop=54, init=False)
    assert_bitwise(rest, whole, (NL, "two calls vs one"))
    assert_bitwise(whole, _run(model, inp, gm, _hip.FLAG_MULTI_LAUNCH, seed=13, **STEPS), (NL, "module vs per-layer launches"))


@gpu
@pytest.mark.parametrize("fill", ["ff", "random"])
def test_poisoned_workspace(models, inputs8, fill):
    """what the workspace (the class bytes in it) held before the call does not show; 0xFF bytes would be class 255"""
    _, model = models[2]
    inp = inputs8[2]
    for gm in (slab_mask("mixed", 8, K, inp["generation_mask"].cpu()), slab_mask("none", 8, K, None)):
        want = _run(model, inp, gm, _hip.FLAG_MULTI_LAUNCH, seed=13, **STEPS)
        with scratch_poison.poisoned(fill, seed=3):
            got = _run(model, inp, gm, MODULE, seed=13, **STEPS)
        assert_bitwise(got, want, ("poisoned workspace", fill))


@gpu
@pytest.mark.parametrize("mode", ["structure", "fixed_backbone"])
def test_design_modes(models, inputs8, mode):
    """"structure" keeps the sequence (DIFFAB_FLAG_KEEP_SEQUENCE), "fixed_backbone" the structure (DIFFAB_FLAG_KEEP_STRUCTURE)"""
    _, model = models[3]
    inp = inputs8[3]
    for gm in (slab_mask("mixed", 8, K, inp["generation_mask"].cpu()), segment_mask(8, K, [(31, 33)])):
        out = _three_ways(model, inp, gm, mode, mode=mode)
        if mode == "structure":
            assert torch.equal(out["seq_idx"], inp["seq_idx"])
        else:
            assert torch.equal(out["translations"], inp["translations"]) and torch.equal(out["orientations"], inp["orientations"])


@gpu
def test_shared_contexts(models):
    """num_samples = 3 on 2 contexts: the shared-context workspace (the map and the gathered residue contexts) with the class bytes"""
    dims, model = models[3]
    inp = patches(2, K, dims, seed=363)
    for gm in (inp["generation_mask"].cpu(), segment_mask(2, K, [(31, 33)])):
        out = _three_ways(model, inp, gm, "shared contexts", num_samples=3)
        assert out["translations"].shape[0] == 6
        assert not torch.equal(out["translations"][0], out["translations"][1])  # two designs of patch 0


@gpu
def test_steering(models):
    dims, model = models[3]
    inp = patches(8, K, dims, seed=371, chains=True)
    kw = dict(num_samples=2, steering=ParticleSteering(strength=0.05, ess_threshold=2.0))
    moved = 0
    for gm in (inp["generation_mask"].cpu(), segment_mask(8, K, [(110, 128)])):
        out = _three_ways(model, inp, gm, "steering", **kw)
        moved += int((out["steering"]["ancestors"].cpu() != torch.arange(16)).sum())
    assert moved > 0, "some ancestor must differ from the identity for this case to say anything"


@gpu
@pytest.mark.parametrize("B", [8, 264, 301])
def test_device_start_classes_equal_the_host_function(hip, start_classes, B):
    """the sampler's kernel on the device plan of the same masks writes the bytes the host function gives, and none behind them"""
    dims = dict(syn.BENCH_DIMS, NL=2)
    gm = patches(B, K, dims, seed=600 + B)["generation_mask"].clone()
    gm[0], gm[B - 1] = False, True
    plan = torch.empty(B, NT, dtype=torch.int32, device="cuda")
    _hip.check(hip.diffab_debug_row_plan(_hip.ptr(gm.contiguous()), B, K, _hip.ptr(plan), _hip.stream_ptr()), "row_plan")
    out = torch.full((B + 8,), 0xEE, dtype=torch.uint8, device="cuda")
    for classes in (8, 3):
        _hip.check(_start_classes_entry(hip)(_hip.ptr(plan), B, K, classes, _hip.ptr(out), 1, _hip.stream_ptr()), "start_classes")
        got = out.cpu().numpy()
        assert (got[B:] == 0xEE).all()
        assert (got[:B].astype(int) == start_classes(plan.cpu().numpy(), classes)).all(), (B, classes)


@gpu
def test_work_groups_that_walk_two_patches(models):
    """B = 264 > the work-groups of the launch: a work-group takes the class of its first patch, and the class bytes end in a whole word"""
    dims, model = models[3]
    inp = patches(264, K, dims, seed=504)
    _three_ways(model, inp, inp["generation_mask"].cpu(), "B = 264")


# ====================================================================== start classes (host, no GPU)
NT = 2 + K // 16


def _start_classes_entry(lib):
    """include/diffab_hip_debug.h: (plan, B, K, classes, out, on_device, stream)"""
    fn = lib.diffab_debug_start_classes
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p]
    return fn


@pytest.fixture(scope="module")
def start_classes():
    fn = _start_classes_entry(_hip.load_library())  # dlopen only: needs no GPU

    def run(plan, classes):
        plan = np.ascontiguousarray(plan, dtype=np.int32)
        out = np.full(plan.shape[0] + 8, 0xEE, dtype=np.uint8)  # (bytes behind B stay untouched)
        assert fn(plan.ctypes.data, plan.shape[0], K, classes, out.ctypes.data, 0, None) == 0
        assert (out[plan.shape[0]:] == 0xEE).all()
        return out[:plan.shape[0]].astype(int)

    return run


def _plan(B, seed):
    """a row plan as launch_row_plan writes it: one CDR-like segment of 5 .. 20 rows per patch, a few patches with two segments, one
    with no generated residue and one with all"""
    rng = np.random.default_rng(seed)
    gm = np.zeros((B, K), dtype=bool)
    for b in range(B):
        for _ in range(2 if rng.random() < 0.1 else 1):
            lo = int(rng.integers(0, K - 20))
            gm[b, lo:lo + int(rng.integers(5, 21))] = True
    gm[0] = False
    gm[B - 1] = True
    plan = np.full((B, NT), -1, dtype=np.int32)
    for b in range(B):
        items, covered = [], 0
        for i in np.flatnonzero(gm[b]):
            if i >= covered:
                s = min(int(i), K - 16)
                items.append(s)
                covered = s + 16
        plan[b, 0] = len(items)
        plan[b, 1] = sum(1 << s for s in range(K // 32) if gm[b, 32 * s:32 * s + 32].any())
        plan[b, 2:2 + len(items)] = items
    return plan


@pytest.mark.parametrize("B", [8, 256, 264, 300])
@pytest.mark.parametrize("classes", [8, 16, 3])
def test_start_classes_are_balanced_and_ordered_by_work(start_classes, B, classes):
    plan = _plan(B, seed=B)
    cls = start_classes(plan, classes)
    assert cls.min() >= 0 and cls.max() < classes
    counts = np.bincount(cls, minlength=classes)
    assert set(counts.tolist()) <= {B // classes, -(-B // classes)}, counts
    items = plan[:, 0]
    slabs = np.array([bin(int(w)).count("1") for w in plan[:, 1]])
    assert len(set(items.tolist())) > 1, "the plan must have patches of different work for this case to say anything"
    work = items * 8 + slabs  # (slabs <= 4: ordered as (items, slabs))
    latest = -1  # the latest class of any patch with more work
    for w in sorted(set(work.tolist()), reverse=True):
        mine = cls[work == w]
        assert mine.min() >= latest, (w, "a patch with more last-layer work sits in a later class than one with less")
        latest = mine.max()


def test_equal_work_keeps_the_static_classes_order(start_classes):
    """all patches alike: ranked by the static class (b / 8) % classes, then by b"""
    B, classes = 256, 8
    plan = np.tile(_plan(8, seed=1)[3], (B, 1))
    cls = start_classes(plan, classes)
    static = (np.arange(B) // 8) % classes
    assert (cls == static).all()


def test_one_class(start_classes):
    assert (start_classes(_plan(16, seed=2), 1) == 0).all()
