"""Shared-context sampling on the MI355X: DiffAb.sample(num_samples=N) and DiffAb.sample(context_index=...)
(diffab_sample_options.ctx_of_row).

The specification is an equality: N designs of each patch from ONE copy of its context are bitwise the samples of num_samples=1 on the
repeat_interleave(N, dim=0) of every per-patch input (same seed, same first_patch) - on every launch form of the sampler: the
patch-resident module launch, the per-layer launches, the two-chunk K = 256 items, the fp32 pair stream, the generic kernels, graph
replay and skipped row tiles; plus sharding by output rows, distinct designs per patch, and the memory the shared form does not hold.
"""
import ctypes as C

import pytest
import torch

from diffab_pytorch import _hip, synthetic as syn
from sampler_support import CTX, STATE, assert_bitwise, bench_model, device_patches, hip, rows, sample

pytestmark = pytest.mark.gpu


def shared_vs_replicated(model, inp, N, **kw):
    B = inp["seq_idx"].shape[0]
    got = sample(model, inp, num_samples=N, **kw)
    want = sample(model, rows(inp, torch.arange(B, device="cuda").repeat_interleave(N)), **kw)
    assert_bitwise(got, want, f"num_samples={N} {kw}")
    return got


def test_module_launch_b16_n16_k128_100_steps(hip):
    """B N = 256 rows from 16 contexts, K = 128, the full 100-step trajectory: the batch fills the chip, so the sampler takes the
    patch-resident module launch (one launch per step) - bitwise the replicated batch, and the 16 designs of a patch differ."""
    dims, model = bench_model(100)
    B, N, K = 16, 16, 128
    inp = device_patches(B, K, dims, seed=41)
    got = shared_vs_replicated(model, inp, N, seed=7)
    gm = inp["generation_mask"].repeat_interleave(N, 0)
    assert torch.isfinite(got["translations"]).all() and torch.isfinite(got["orientations"]).all()
    x = got["translations"].view(B, N, K, 3)
    for b in range(B):  # the replicas of a patch have their own noise keys (patch id b N + r): distinct designs
        g = inp["generation_mask"][b]
        assert not all(torch.equal(x[b, 0, g], x[b, r, g]) for r in range(1, N)), b
    x_in = inp["translations"].repeat_interleave(N, 0)
    assert torch.equal(got["translations"][~gm], x_in[~gm])  # context residues are never touched


def test_per_layer_launches_b2_n4(hip):
    """B N = 8 rows (fewer than the CUs): one launch per kernel of an IPA layer, planes of 2 contexts."""
    dims, model = bench_model(100)
    inp = device_patches(2, 128, dims, seed=42)
    shared_vs_replicated(model, inp, 4, seed=3, t_start=30, t_stop=18)


def test_two_chunk_items_k256_b4_n2(hip):
    """K = 256: attention items of two 128-key chunks with the online softmax across them."""
    dims, model = bench_model(100, NL=2)
    inp = device_patches(4, 256, dims, seed=43)
    shared_vs_replicated(model, inp, 2, seed=5, t_start=20, t_stop=14)


@pytest.mark.parametrize("form", ["pair_f32", "force_generic", "graph", "skip_unused_rows", "module_flag"])
def test_launch_forms(hip, form):
    """Every other form of the reverse loop reads the pair context through the map: the fp32 pair stream (no planes), the generic
    kernels, one captured step replayed as a hipGraph, the last layer for generated row tiles only, the module launch at a small batch."""
    dims, model = bench_model(100, NL=3)
    inp = device_patches(3, 128, dims, seed=44)
    inp["generation_mask"][1] = False  # (a patch without generated residues: all its tiles of the last layer skipped)
    kw = {"pair_f32": dict(flags=_hip.FLAG_PAIR_F32), "force_generic": dict(flags=_hip.FLAG_FORCE_GENERIC), "graph": dict(graph=True),
          "skip_unused_rows": dict(skip_unused_rows=True), "module_flag": dict(flags=_hip.FLAG_PERSISTENT_MODULE)}[form]
    shared_vs_replicated(model, inp, 3, seed=11, t_start=12, t_stop=7, **kw)


def test_non_benchmark_dims_generic_path(hip):
    """Unit dims (D = 32, C = 16, K = 24): the generic path by dims, not by flag."""
    from diffab_pytorch import DiffAb

    dims = dict(syn.UNIT_DIMS, NL=2)
    model = DiffAb(dims["D"], dims["C"], dims["NL"], dims["DS"], dims["PQ"], dims["PV"], dims["H"], T=20).cuda()
    model.denoiser.load_state_dict(syn.denoiser_state_dict(dims, seed=5, prefix=""))
    inp = {k: v.cuda() for k, v in syn.patches(3, 24, dims, seed=45, coord_sigma=5.0).items() if k in STATE + CTX}
    shared_vs_replicated(model, inp, 2, seed=13)


def test_sharding_by_output_rows_and_arbitrary_maps(hip):
    """A rank that owns output rows [lo, hi) - ends not multiples of N - passes those state rows, context_index = row // N over all
    contexts, first_patch = lo: exactly those rows of the full run.  And any map (repeats, gaps, any order) is its gathered batch."""
    dims, model = bench_model(100)
    B, N, K = 3, 4, 128
    inp = device_patches(B, K, dims, seed=46)
    kw = dict(seed=17, t_start=25, t_stop=15)
    full = sample(model, inp, num_samples=N, **kw)
    rep = rows(inp, torch.arange(B, device="cuda").repeat_interleave(N))
    for lo, hi in ((3, 10), (0, 5), (7, 12)):
        state = {k: rep[k][lo:hi] for k in STATE}
        part = sample(model, dict(state, **{k: inp[k] for k in CTX}), context_index=torch.arange(lo, hi) // N, first_patch=lo, **kw)
        assert_bitwise(part, {k: v[lo:hi] for k, v in full.items()}, f"rows [{lo}, {hi})")
    idx = torch.tensor([2, 0, 2, 2, 1, 0], device="cuda")  # (state rows of patches 0..5 of a batch whose contexts are the 3 patches)
    state = {k: v for k, v in device_patches(6, K, dims, seed=47).items() if k in STATE}
    got = sample(model, dict(state, **{k: inp[k] for k in CTX}), context_index=idx, **kw)
    want = sample(model, dict(state, **{k: inp[k].index_select(0, idx) for k in CTX}), **kw)
    assert_bitwise(got, want, "map [2, 0, 2, 2, 1, 0]")


def test_raw_batch_encodes_each_patch_once(hip):
    """Without precomputed contexts: ONE encode_context call over the B patches (not B N), then the shared loop - bitwise the raw
    replicated batch, whose encode_context runs over all B N rows."""
    dims, model = bench_model(100, NL=2)
    model.load_state_dict(syn.context_state_dict(dims["D"], dims["C"], 15, 32, seed=3), strict=False)
    B, N, K = 2, 3, 128
    cb = {k: v.cuda() for k, v in syn.context_batch(B, K, 15, seed=3, with_distmat=False).items() if k != "distmat"}
    calls = []
    enc = model.encode_context

    def counting(*a, **k):
        calls.append(a[0].shape[0])
        return enc(*a, **k)

    model.encode_context = counting
    try:
        def run(sel, **kw):
            g = lambda k: cb[k] if sel is None else cb[k].index_select(0, sel)
            return model.sample(g("seq_idx"), g("xyz"), g("orientations"), generation_mask=g("generation_mask"), atom_mask=g("atom_mask"),
                                chain_idx=g("chain_idx"), residue_mask=g("residue_mask"), seed=23, t_start=10, t_stop=4, **kw)

        got = run(None, num_samples=N)
        assert calls == [B]  # once, over the B patches
        want = run(torch.arange(B, device="cuda").repeat_interleave(N))
        assert calls == [B, B * N]
    finally:
        del model.encode_context
    assert_bitwise(got, want, "raw batch")


def test_memory_of_256_designs_from_16_contexts(hip):
    """The in-call peak of the shared form at B N = 256 from 16 contexts is below the replicated call's by >= 0.75 GiB: the replicated
    call's fp16 pair planes alone are 1 GiB (256 x 4 MiB), the shared call's 64 MiB."""
    dims, model = bench_model(100)
    B, N, K = 16, 16, 128
    inp = device_patches(B, K, dims, seed=48)
    rep = rows(inp, torch.arange(B, device="cuda").repeat_interleave(N))
    kw = dict(seed=29, t_start=3, t_stop=1)

    def in_call_peak(fn):
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        out = fn()
        torch.cuda.synchronize()
        return torch.cuda.max_memory_allocated() - base, out

    peak_shared, got = in_call_peak(lambda: sample(model, inp, num_samples=N, **kw))
    peak_rep, want = in_call_peak(lambda: sample(model, rep, **kw))
    assert_bitwise(got, want, "memory run")
    print(f"in-call peak: shared {peak_shared / 2**20:.0f} MiB, replicated {peak_rep / 2**20:.0f} MiB")
    assert peak_rep - peak_shared >= 0.75 * 2**30, (peak_shared, peak_rep)


# ------------------------------------------------------------------ the C ABI
def test_loop_ex_without_options_is_the_plain_loop(hip):
    """diffab_sample_loop, diffab_sample_loop_ex with NULL options and with options that are zero except for struct_bytes: three steps
    from t_start = T = 10 on the same seed give bitwise the same seq, x and O (B = 2, K = 64, unit dims, one layer)."""
    from diffab_pytorch import DiffAb

    dims = dict(syn.UNIT_DIMS, NL=1)
    B, K, T = 2, 64, 10
    model = DiffAb(dims["D"], dims["C"], dims["NL"], dims["DS"], dims["PQ"], dims["PV"], dims["H"], T=T).cuda()
    model.denoiser.load_state_dict(syn.denoiser_state_dict(dims, seed=5, prefix=""))
    inp = {k: v.cuda() for k, v in syn.patches(B, K, dims, seed=46, coord_sigma=5.0).items() if k in STATE + CTX}
    P, st = _hip.ptr, _hip.stream_ptr()
    gm = _hip.dev_mask(inp["generation_mask"])
    dims_c, w, sd = model.denoiser.hip_dims(B, K), model.denoiser.hip_weights(), model._sched_on_device()
    rev = model._reverse_so3().struct()
    ws = _hip.workspace(hip.diffab_sample_workspace_bytes(C.byref(dims_c)))

    def run(entry, *opt):
        seq, x, O = inp["seq_idx"].clone(), inp["translations"].clone(), inp["orientations"].clone()
        _hip.check(hip.diffab_sample_init(P(seq), P(x), P(O), P(gm), 17, 0, B, K, T, st), "init")
        _hip.check(entry(C.byref(dims_c), C.byref(w.struct), C.byref(sd.struct), C.byref(rev), P(seq), P(x), P(O), P(inp["res_context_emb"]),
                         P(inp["pair_context_emb"]), P(gm), 17, 0, T, T - 3, P(ws), ws.numel(), 0, *opt, st), "loop")
        torch.cuda.synchronize()
        return {"seq_idx": seq, "translations": x, "orientations": O}

    want = run(hip.diffab_sample_loop)
    assert not torch.equal(want["translations"], inp["translations"])  # the steps ran
    assert_bitwise(run(hip.diffab_sample_loop_ex, None), want, "NULL options")
    zeroed = _hip.SampleOptions()
    assert zeroed.struct_bytes == 64 and bytes(zeroed)[4:] == bytes(60)
    assert_bitwise(run(hip.diffab_sample_loop_ex, C.byref(zeroed)), want, "zeroed options")
