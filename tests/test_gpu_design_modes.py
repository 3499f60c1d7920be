"""Design modes of the sampler on the MI355X: DiffAb.sample(mode="fixed_backbone" | "structure" | "codesign", optimize_from=t).

The specification is a set of equalities.  A mode diffuses one modality exactly as co-design does (same state in, same Philox draws)
and never writes the other (DIFFAB_FLAG_KEEP_STRUCTURE / _SEQUENCE), on every launch form of the reverse loop.  optimize_from=t starts
from the native forward-noised to step t (diffab_sample_init_noised), which matches the oracle's forward process on the same Philox
lanes, and keeps the sampler's sharding / num_samples / graph-replay equalities.
"""
import ctypes as C

import pytest
import torch

import diffab_oracle as orc
from conftest import maxrel
from diffab_pytorch import _hip, synthetic as syn
from sampler_support import CTX, STREAMS_OPT, assert_bitwise, hip, make_model, patches, rows, sample, step_noise

pytestmark = pytest.mark.gpu
TOL = 1e-4  # as tests/test_gpu_parity.py
STRUCT = ("translations", "orientations")


@pytest.fixture(scope="module")
def unit(hip):
    dims = dict(syn.UNIT_DIMS, NL=2)
    return dims, make_model(dims, 17)


@pytest.fixture(scope="module")
def bench(hip):
    dims = dict(syn.BENCH_DIMS, NL=3)
    return dims, make_model(dims, 19)


def assert_kept(out, inp, mode, what=""):
    """The modality the mode keeps is bitwise the input on every residue; the other one moved on the generated residues."""
    gm = inp["generation_mask"]
    kept, moved = (STRUCT, ("seq_idx",)) if mode == "fixed_backbone" else (("seq_idx",), STRUCT)
    for k in kept:
        assert torch.equal(out[k], inp[k]), (what, mode, k, int((out[k] != inp[k]).sum()))
    for k in moved:
        assert not torch.equal(out[k][gm], inp[k][gm]), (what, mode, k)
        assert torch.equal(out[k][~gm], inp[k][~gm]), (what, mode, k)  # context residues are never written
    assert torch.isfinite(out["translations"]).all() and torch.isfinite(out["orientations"]).all()


# ------------------------------------------------------------------ one step: a mode is co-design restricted to one modality
@pytest.mark.parametrize("geometry", ["unit_k16", "bench_k128"])
def test_one_step_mode_separability(unit, bench, geometry):
    """One step t -> t-1 from the same state and seed (init=False): fixed_backbone's seq is co-design's seq and its x, O are the input;
    structure's x, O are co-design's and its seq is the input.  Generic kernels (unit dims, K = 16) and the MFMA per-layer path at the
    benchmark dims (K = 128); t = 100, 57, 8 (the histogram branch of the reverse table) and 1 (no noise)."""
    dims, model = unit if geometry == "unit_k16" else bench
    K = 16 if geometry == "unit_k16" else 128
    inp = patches(3, K, dims, seed=5)
    inp["generation_mask"][:, : K // 2] = True
    for t in (100, 57, 8, 1):
        kw = dict(init=False, t_start=t, t_stop=t - 1, seed=31, first_patch=4)
        co = sample(model, inp, mode="codesign", **kw)
        fb = sample(model, inp, mode="fixed_backbone", **kw)
        st = sample(model, inp, mode="structure", **kw)
        gm = inp["generation_mask"]
        assert not torch.equal(co["translations"][gm], inp["translations"][gm]), t  # (the comparisons below are not vacuous)
        assert torch.equal(fb["seq_idx"], co["seq_idx"]), t
        for k in STRUCT:
            assert torch.equal(fb[k], inp[k]), (t, k)
            assert torch.equal(st[k], co[k]), (t, k)
        assert torch.equal(st["seq_idx"], inp["seq_idx"]), t


# ------------------------------------------------------------------ full trajectories: the kept modality is never written
@pytest.mark.parametrize("mode", ["fixed_backbone", "structure"])
@pytest.mark.parametrize("form", ["per_layer", "graph", "num_samples", "pair_f32", "force_generic", "skip_unused_rows", "module_flag",
                                  "context_index"])
def test_trajectory_keeps_the_modality(bench, mode, form):
    """Multi-step trajectories from the mode's own initial state (diffab_sample_init_ex): the kept modality is bitwise the input on every
    residue after the run, on each launch form of the loop."""
    dims, model = bench
    inp = patches(3, 128, dims, seed=6)
    inp["generation_mask"][1, :40] = True
    kw = {"per_layer": {}, "graph": dict(graph=True), "num_samples": dict(num_samples=3), "pair_f32": dict(flags=_hip.FLAG_PAIR_F32),
          "force_generic": dict(flags=_hip.FLAG_FORCE_GENERIC), "skip_unused_rows": dict(skip_unused_rows=True),
          "module_flag": dict(flags=_hip.FLAG_PERSISTENT_MODULE), "context_index": dict(context_index=torch.tensor([2, 0, 2]))}[form]
    ref = inp
    if form == "num_samples":
        ref = rows(inp, torch.arange(3, device="cuda").repeat_interleave(3))
    elif form == "context_index":
        ref = dict(inp, **{k: inp[k].index_select(0, torch.tensor([2, 0, 2], device="cuda")) for k in CTX})
    out = sample(model, inp, mode=mode, seed=8, t_start=30, t_stop=22, **kw)
    assert_kept(out, ref, mode, form)
    if form in ("graph", "skip_unused_rows", "module_flag"):  # (these forms are bitwise the per-layer loop)
        assert_bitwise(out, sample(model, inp, mode=mode, seed=8, t_start=30, t_stop=22), form)
    if form in ("num_samples", "context_index"):  # shared contexts: bitwise the replicated batch
        assert_bitwise(out, sample(model, ref, mode=mode, seed=8, t_start=30, t_stop=22), form)


@pytest.mark.parametrize("mode", ["fixed_backbone", "structure"])
def test_module_launch_256_rows_keeps_the_modality(bench, mode):
    """256 rows at K = 128 from 16 contexts (as test_module_launch_b16_n16_k128_100_steps): the batch fills the chip, so the loop takes
    the patch-resident module launch, whose folded heads' O0 epilogue runs in the update kernel - skipped with KEEP_STRUCTURE."""
    dims, model = bench
    B, N, K = 16, 16, 128
    inp = patches(B, K, dims, seed=41)
    out = sample(model, inp, mode=mode, num_samples=N, seed=7, t_start=12, t_stop=4)
    rep = rows(inp, torch.arange(B, device="cuda").repeat_interleave(N))
    assert_kept(out, rep, mode, "module")
    per_layer = sample(model, inp, mode=mode, num_samples=N, seed=7, t_start=12, t_stop=4, flags=_hip.FLAG_MULTI_LAUNCH)
    assert_bitwise(out, per_layer, "module vs per-layer launches")


# ------------------------------------------------------------------ forward-noised start vs the oracle
def test_forward_noised_init_vs_oracle(unit):
    """sample(optimize_from=t, t_stop=t) runs no reverse step: the result is the native forward-noised to t.  Against the oracle's forward
    process driven by the same Philox lanes (streams 7-10, counter step t): x and O within TOL for t on the histogram branch of the
    forward table (sigma_t = sqrt(1 - abar_t) < 0.1: t <= 5) and the Gaussian branch; a sequence draw may differ only on an edge of the
    CDF; context residues are bitwise unchanged."""
    dims, model = unit
    sched = orc.cosine_variance_schedule(100, s=0.01, beta_max=0.999)
    B, K, seed, fp = 8, 16, 2024, 5
    inp = {k: v.cpu() for k, v in patches(B, K, dims, seed=9).items()}
    inp["generation_mask"][:, :12] = True
    gm = inp["generation_mask"]
    cdf = model.orientation_diffuser.so3._cdf.cpu()
    sig = sched["one_minus_alpha_bar_sqrt"]
    cos = (inp["orientations"].diagonal(dim1=-2, dim2=-1).sum(-1) - 1) / 2
    ok = gm & ((cos - 1).abs() >= 1e-2) & ((cos + 1).abs() >= 1e-2)  # scale_rot is defined away from theta in {0, pi}
    assert ok.sum() > 0.8 * gm.sum()
    flips = 0
    for t in (1, 3, 5, 6, 8, 40, 100):
        got = {k: v.cpu() for k, v in sample(model, inp, optimize_from=t, t_stop=t, seed=seed, first_patch=fp).items()}
        tt = torch.full((B,), t, dtype=torch.long)
        eps, rotvec, us = step_noise(seed, fp, B, K, t, cdf[t], sig[t], streams=STREAMS_OPT)
        x1 = orc.coord_diffuse_from_t0(inp["translations"], tt, gm, eps, sched)
        O1 = orc.orient_diffuse_from_t0(inp["orientations"], gm, tt, rotvec, sched)
        p = orc.seq_forward_prob_from_t0(inp["seq_idx"], tt, gm, sched)
        s1 = orc.categorical_from_uniform(p, us)
        assert maxrel(got["translations"], x1) < TOL, (t, maxrel(got["translations"], x1))
        assert maxrel(got["orientations"][ok], O1[ok]) < TOL, (t, maxrel(got["orientations"][ok], O1[ok]))
        diff = (got["seq_idx"] != s1) & gm
        if diff.any():
            edge = (p.double().cumsum(-1) - us.double()[..., None]).abs().min(dim=-1).values
            assert float(edge[diff].max()) < 1e-5, (t, int(diff.sum()), float(edge[diff].max()))
            flips += int(diff.sum())
        for k in ("seq_idx", "translations", "orientations"):
            assert torch.equal(got[k][~gm], inp[k][~gm]), (t, k)
        Og = got["orientations"][gm].double()
        assert torch.allclose(Og.transpose(-1, -2) @ Og, torch.eye(3, dtype=torch.float64).expand_as(Og), atol=1e-4), t
        if t >= 40:  # noised well away from the native
            assert not torch.equal(got["seq_idx"][gm], inp["seq_idx"][gm]), t
    print(f"forward-noised start: {flips} sequence draws on a CDF edge")


# ------------------------------------------------------------------ optimisation trajectories
@pytest.mark.parametrize("mode", [None, "fixed_backbone", "structure"])
def test_optimisation_trajectories(bench, mode):
    """optimize_from=8 (8 reverse steps from the forward-noised native): num_samples=4 is bitwise num_samples=1 on the replicated batch,
    two first_patch shards are bitwise the whole batch, graph replay is bitwise the eager loop; a mode's kept modality is the native."""
    dims, model = bench
    B, N, K = 3, 4, 128
    inp = patches(B, K, dims, seed=12)
    kw = dict(mode=mode, optimize_from=8, seed=55)
    many = sample(model, inp, num_samples=N, **kw)
    rep = rows(inp, torch.arange(B, device="cuda").repeat_interleave(N))
    whole = sample(model, rep, **kw)
    assert_bitwise(many, whole, "num_samples")
    parts = [sample(model, {k: v[lo:hi] for k, v in rep.items()}, first_patch=lo, **kw) for lo, hi in ((0, 5), (5, B * N))]
    assert_bitwise({k: torch.cat([p[k] for p in parts]) for k in whole}, whole, "shards")
    assert_bitwise(sample(model, rep, graph=True, **kw), whole, "graph")
    if mode is None:
        gm = rep["generation_mask"]
        for k in ("seq_idx", "translations", "orientations"):
            assert torch.equal(whole[k][~gm], rep[k][~gm]), k
        x = whole["translations"].view(B, N, K, 3)
        assert not torch.equal(x[0, 0], x[0, 1])  # the replicas of a patch are distinct variants
    else:
        assert_kept(whole, rep, mode, "optimize_from")


# ------------------------------------------------------------------ mode=None / "codesign", and the contexts each mode encodes
def test_codesign_is_mode_none_and_modes_encode_their_context(hip):
    """From the reference's raw batch: mode="codesign" is bitwise mode=None, and each mode calls encode_context with its
    (generate_structure, generate_sequence) - fixed_backbone (False, True), structure (True, False)."""
    dims = dict(syn.BENCH_DIMS, NL=2)
    model = make_model(dims, 0)
    model.load_state_dict(syn.context_state_dict(dims["D"], dims["C"], 15, 32, seed=3), strict=False)
    cb = {k: v.cuda() for k, v in syn.context_batch(3, 128, 15, seed=3, with_distmat=False).items() if k != "distmat"}
    calls = []
    enc = model.encode_context

    def recording(*a, **k):
        calls.append(tuple(a[11:13]))
        return enc(*a, **k)

    model.encode_context = recording
    try:
        def run(**kw):
            return model.sample(cb["seq_idx"], cb["xyz"], cb["orientations"], generation_mask=cb["generation_mask"],
                                atom_mask=cb["atom_mask"], chain_idx=cb["chain_idx"], residue_mask=cb["residue_mask"], seed=23, t_start=12,
                                t_stop=5, **kw)

        base = run()
        assert_bitwise(run(mode="codesign"), base, "codesign")
        fb = run(mode="fixed_backbone")
        st = run(mode="structure")
    finally:
        del model.encode_context
    assert calls == [(True, True), (True, True), (False, True), (True, False)]
    from diffab_pytorch.diffab_pytorch import CA_IDX

    ref = {"seq_idx": cb["seq_idx"], "translations": cb["xyz"][:, :, CA_IDX].contiguous(), "orientations": cb["orientations"],
           "generation_mask": cb["generation_mask"]}
    assert_kept(fb, ref, "fixed_backbone", "raw batch")
    assert_kept(st, ref, "structure", "raw batch")


# ------------------------------------------------------------------ the C ABI
def test_c_abi_keep_bits_and_argument_errors(bench):
    """diffab_sample_init_ex without KEEP bits is bitwise diffab_sample_init (other bits ignored); both KEEP bits, t outside [1, T] and a
    short forward table return DIFFAB_ERR_ARG and enqueue nothing - in the loop as in the two init entries."""
    dims, model = bench
    lib = _hip.lib()
    B, K, T = 2, 128, model.T
    inp = patches(B, K, dims, seed=13)
    seq, x, O = inp["seq_idx"].clone(), inp["translations"].clone(), inp["orientations"].clone()
    gm = _hip.dev_mask(inp["generation_mask"])
    st = _hip.stream_ptr()
    both = _hip.FLAG_KEEP_STRUCTURE | _hip.FLAG_KEEP_SEQUENCE
    P = _hip.ptr
    _hip.check(lib.diffab_sample_init(P(seq), P(x), P(O), P(gm), 3, 1, B, K, T, st), "init")
    for flags in (0, _hip.FLAG_GRAPH_SAMPLER | _hip.FLAG_PAIR_F32):
        s2, x2, O2 = inp["seq_idx"].clone(), inp["translations"].clone(), inp["orientations"].clone()
        _hip.check(lib.diffab_sample_init_ex(P(s2), P(x2), P(O2), P(gm), 3, 1, B, K, T, flags, None, st), "init_ex")
        assert torch.equal(s2, seq) and torch.equal(x2, x) and torch.equal(O2, O), flags
    sd = model._sched_on_device()
    fwd = model.orientation_diffuser.so3.struct()
    short = _hip.Igso3(T, fwd.n_bins, fwd.sigmas, fwd.cdf, fwd.sigma_threshold)
    dims_c = model.denoiser.hip_dims(B, K)
    w = model.denoiser.hip_weights()
    rev = model._reverse_so3().struct()
    ws = _hip.workspace(lib.diffab_sample_workspace_bytes(C.byref(dims_c)))
    rc_, pc_ = inp["res_context_emb"], inp["pair_context_emb"]
    s0, x0, O0 = inp["seq_idx"].clone(), inp["translations"].clone(), inp["orientations"].clone()
    bad = [
        ("init_ex both", lambda: lib.diffab_sample_init_ex(P(s0), P(x0), P(O0), P(gm), 3, 1, B, K, T, both, None, st)),
        ("noised both", lambda: lib.diffab_sample_init_noised(C.byref(sd.struct), C.byref(fwd), P(s0), P(x0), P(O0), P(gm), 3, 1, B, K, 8,
                                                              both, None, st)),
        ("noised t=0", lambda: lib.diffab_sample_init_noised(C.byref(sd.struct), C.byref(fwd), P(s0), P(x0), P(O0), P(gm), 3, 1, B, K, 0,
                                                             0, None, st)),
        ("noised t=T+1", lambda: lib.diffab_sample_init_noised(C.byref(sd.struct), C.byref(fwd), P(s0), P(x0), P(O0), P(gm), 3, 1, B, K,
                                                               T + 1, 0, None, st)),
        ("noised short table", lambda: lib.diffab_sample_init_noised(C.byref(sd.struct), C.byref(short), P(s0), P(x0), P(O0), P(gm), 3, 1, B,
                                                                     K, 8, 0, None, st)),
        ("loop both", lambda: lib.diffab_sample_loop(C.byref(dims_c), C.byref(w.struct), C.byref(sd.struct), C.byref(rev), P(s0), P(x0),
                                                     P(O0), P(rc_), P(pc_), P(gm), 3, 1, 10, 5, P(ws), ws.numel(), both, st)),
        ("loop_ex both", lambda: lib.diffab_sample_loop_ex(C.byref(dims_c), C.byref(w.struct), C.byref(sd.struct), C.byref(rev), P(s0),
                                                           P(x0), P(O0), P(rc_), P(pc_), P(gm), 3, 1, 10, 5, P(ws), ws.numel(), both,
                                                           C.byref(_hip.SampleOptions(n_ctx=B)), st)),
    ]
    for what, fn in bad:
        assert fn() == -1, what  # DIFFAB_ERR_ARG
        assert lib.diffab_last_error(), what
    torch.cuda.synchronize()
    assert torch.equal(s0, inp["seq_idx"]) and torch.equal(x0, inp["translations"]) and torch.equal(O0, inp["orientations"])
    # t = T and t = 1 are inside the schedule
    for t in (1, T):
        _hip.check(lib.diffab_sample_init_noised(C.byref(sd.struct), C.byref(fwd), P(s0), P(x0), P(O0), P(gm), 3, 1, B, K, t, 0, None, st), t)
    torch.cuda.synchronize()
    assert torch.isfinite(x0).all() and torch.isfinite(O0).all()
