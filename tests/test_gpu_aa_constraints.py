"""Sequence constraints of the sampler on the MI355X: DiffAb.sample(allowed_aa=...) and the diffab_*_aa entries.

The specification (include/diffab_hip.h): every sequence draw of a generated residue is restricted to its allowed
classes, on the Philox lane of the unconstrained draw.  Checked here as equalities - an all-True mask is bitwise the unconstrained run
on every launch form; a forbidden class never appears; a single allowed class is always the result; one reverse step, the initial
state and the optimisation start match a host restatement of the rules on the same uniforms; sharding keeps its bitwise equality.
"""
import ctypes as C

import pytest
import torch

from diffab_pytorch import _hip, io, synthetic as syn
from sampler_support import CTX, STATE, assert_bitwise, hip, make_model, patches, rows, sample

pytestmark = pytest.mark.gpu
V, UNK = 21, 20
STREAM_SEQ, STREAM_INIT_S, STREAM_OPT_SEQ = 0, 6, 7  # csrc/philox.h
STRUCT = ("translations", "orientations")
MARGIN = 1e-5  # relative to tot: how far a threshold must lie from a cumulative boundary for the draw to be decided


@pytest.fixture(scope="module")
def unit(hip):
    dims = dict(syn.UNIT_DIMS, NL=2)
    return dims, make_model(dims, 17)


@pytest.fixture(scope="module")
def bench(hip):
    dims = dict(syn.BENCH_DIMS, NL=3)
    return dims, make_model(dims, 19)


def assert_context_untouched(out, inp, what=""):
    gm = inp["generation_mask"]
    for k in ("seq_idx",) + STRUCT:
        assert torch.equal(out[k][~gm], inp[k][~gm]), (what, k)


def random_subsets(shape, seed, lo=1, hi=V):
    """bool (*shape, V): every entry a random subset of lo..hi classes"""
    g = torch.Generator().manual_seed(seed)
    n = int(torch.tensor(shape).prod())
    size = torch.randint(lo, hi + 1, (n, 1), generator=g)
    ranks = torch.rand(n, V, generator=g).argsort(-1).argsort(-1)
    return (ranks < size).view(*shape, V)


def allowed_ok(seq, allowed):
    """per residue: is the token in its allowed set"""
    return allowed.gather(-1, seq.unsqueeze(-1)).squeeze(-1)


def uniforms(lib, seed, first_patch, B, K, step, stream):
    u = torch.empty(B * K * 4, dtype=torch.float32, device="cuda")
    _hip.check(lib.diffab_philox_fill(seed, first_patch, B, K, step, stream, 1, _hip.ptr(u), _hip.stream_ptr()), "philox_fill")
    return u.view(B, K, 4)[..., 0].cpu()


def restricted_draw(p, u, allowed):
    """Rule 1 on the host, fp32 in increasing v: the draw and how far its threshold lies from the nearest cumulative boundary (over tot)."""
    p, u = p.float().cpu(), u.float().cpu()
    a = allowed.cpu()
    tot = torch.zeros_like(u)
    n = torch.zeros_like(u)
    for v in range(V):
        tot = torch.where(a[..., v], tot + p[..., v], tot)
        n = n + a[..., v].float()
    flat = tot == 0
    thr = u * torch.where(flat, n, tot)
    acc = torch.zeros_like(u)
    tok = torch.full(u.shape, -1, dtype=torch.long)
    last = torch.zeros(u.shape, dtype=torch.long)
    margin = torch.full(u.shape, float("inf"), dtype=torch.float64)
    for v in range(V):
        av = a[..., v]
        acc = torch.where(av, acc + torch.where(flat, torch.ones_like(u), p[..., v]), acc)
        tok = torch.where(av & (acc > thr) & (tok < 0), torch.full_like(tok, v), tok)
        last = torch.where(av, torch.full_like(last, v), last)
        margin = torch.where(av, torch.minimum(margin, (acc.double() - thr.double()).abs()), margin)
    tok = torch.where(tok < 0, last, tok)
    return tok, margin / torch.where(flat, n, tot).double()


def check_against_rule(got, want, margin, allowed, gm, what):
    """Every generated token is allowed; it equals the restatement wherever the draw is decided by more than MARGIN, and at least 95 % of
    the generated residues are decided."""
    g = gm.cpu()
    got = got.cpu()
    assert bool(allowed_ok(got, allowed.cpu())[g].all()), what
    decided = (margin > MARGIN) & g
    assert torch.equal(got[decided], want[decided]), (what, int((got != want)[decided].sum()))
    assert float(decided.sum()) >= 0.95 * float(g.sum()), (what, int(decided.sum()), int(g.sum()))
    return int((got != want)[g].sum())


# ------------------------------------------------------------------ 1. an all-True mask is the unconstrained run, bitwise
FORMS = {"per_layer": {}, "graph": dict(graph=True), "num_samples": dict(num_samples=3),
         "context_index": dict(context_index=torch.tensor([2, 0, 2])), "pair_f32": dict(flags=_hip.FLAG_PAIR_F32),
         "force_generic": dict(flags=_hip.FLAG_FORCE_GENERIC),
         "skip_unused_rows": dict(skip_unused_rows=True), "module_flag": dict(flags=_hip.FLAG_PERSISTENT_MODULE),
         "fixed_backbone": dict(mode="fixed_backbone"), "optimize_from": dict(optimize_from=8)}


@pytest.mark.parametrize("form", sorted(FORMS))
def test_all_true_mask_is_bitwise_unconstrained(bench, form):
    """From the initial state (diffab_sample_init_ex / _noised with `allowed`) through the loop (diffab_sample_options.allowed): the masked draws with every
    class allowed are bitwise the unconstrained ones, on each launch form of the loop."""
    dims, model = bench
    inp = patches(3, 128, dims, seed=6)
    inp["generation_mask"][1, :40] = True
    kw = dict(FORMS[form])
    if form != "optimize_from":
        kw.update(t_start=30, t_stop=22)
    free = sample(model, inp, seed=8, **kw)
    for a in (torch.ones(V, dtype=torch.bool), torch.ones(3, 128, V, dtype=torch.bool, device="cuda")):
        assert_bitwise(sample(model, inp, seed=8, allowed_aa=a, **kw), free, form)


def test_all_true_mask_module_launch_256_rows(bench):
    """256 rows at K = 128 from 16 contexts: the patch-resident module launch, whose heads' epilogue runs in the update kernel."""
    dims, model = bench
    inp = patches(16, 128, dims, seed=41)
    kw = dict(num_samples=16, seed=7, t_start=12, t_stop=4)
    assert_bitwise(sample(model, inp, allowed_aa=torch.ones(V, dtype=torch.bool), **kw), sample(model, inp, **kw), "module")


# ------------------------------------------------------------------ 2. exclusion
@pytest.mark.parametrize("layout", ["rows64", "module256"])
def test_excluded_classes_never_appear(bench, layout):
    """C, M and UNK forbidden on every residue, full T = 100 trajectories: no generated residue holds one, while the unconstrained run
    with the same seed does; context residues are bitwise the input."""
    dims, model = bench
    if layout == "rows64":
        inp, kw = patches(64, 128, dims, seed=51), {}
    else:
        inp, kw = patches(16, 128, dims, seed=52), dict(num_samples=16)
    mask = io.allowed_aa_mask(128, exclude="CMX")
    forbidden = torch.tensor([4, 12, UNK], device="cuda")
    out = sample(model, inp, seed=11, allowed_aa=mask, **kw)
    free = sample(model, inp, seed=11, **kw)
    ref = inp if layout == "rows64" else rows(inp, torch.arange(16, device="cuda").repeat_interleave(16))
    gm = ref["generation_mask"]
    assert int(torch.isin(out["seq_idx"][gm], forbidden).sum()) == 0
    assert int(torch.isin(free["seq_idx"][gm], forbidden).sum()) > 0  # the check above is not vacuous
    assert_context_untouched(out, ref, layout)
    assert torch.isfinite(out["translations"]).all() and torch.isfinite(out["orientations"]).all()


# ------------------------------------------------------------------ 3. fixed positions
@pytest.mark.parametrize("mode", ["codesign", "fixed_backbone"])
def test_single_allowed_class_is_always_drawn(bench, mode):
    """Every generated residue allows one random class (UNK included): a full trajectory ends on exactly that sequence; in co-design x and O
    of those residues still move, in fixed_backbone they are bitwise the input."""
    dims, model = bench
    B, K = 8, 128
    inp = patches(B, K, dims, seed=61)
    g = torch.Generator().manual_seed(3)
    cls = torch.randint(0, V, (B, K), generator=g)
    mask = torch.nn.functional.one_hot(cls, V).bool()
    out = sample(model, inp, mode=mode, seed=13, allowed_aa=mask)
    gm = inp["generation_mask"]
    assert torch.equal(out["seq_idx"][gm].cpu(), cls[gm.cpu()])
    assert_context_untouched(out, inp, mode)
    for k in STRUCT:
        if mode == "codesign":
            assert not torch.equal(out[k][gm], inp[k][gm]), k
        else:
            assert torch.equal(out[k], inp[k]), k


# ------------------------------------------------------------------ 4. one reverse step against the host restatement
@pytest.mark.parametrize("geometry", ["unit_k16", "bench_k128", "bench_k128_generic"])
def test_one_step_vs_host_restatement(unit, bench, geometry):
    """init=False, one step t -> t-1 for t in {100, 57, 1} with random allowed subsets of 1..21 classes per residue: each token is rule 1
    applied to model.denoise's posterior and the STREAM_SEQ uniform (diffab_philox_fill), wherever the draw is decided by more than 1e-5
    of tot (the loop's posterior and denoise's need not agree in the last bits) - at least 95 % of the residues."""
    dims, model = unit if geometry == "unit_k16" else bench
    K = 16 if geometry == "unit_k16" else 128
    flags = _hip.FLAG_FORCE_GENERIC if geometry.endswith("generic") else 0
    lib = _hip.lib()
    B, seed, fp = 6, 31, 4
    inp = patches(B, K, dims, seed=5)
    inp["generation_mask"][:, : K // 2] = True
    gm = inp["generation_mask"]
    mask = random_subsets((B, K), seed=K + flags)
    rm = torch.ones_like(gm)
    flips = 0
    for t in (100, 57, 1):
        out = sample(model, inp, init=False, t_start=t, t_stop=t - 1, seed=seed, first_patch=fp, flags=flags, allowed_aa=mask)
        beta = model.sched["beta"][t].expand(B).contiguous().cuda()
        with torch.no_grad():
            post = model.denoise(inp["seq_idx"], inp["translations"], inp["orientations"], inp["res_context_emb"], inp["pair_context_emb"],
                                 beta, gm, rm)["seq_posterior"]
        u = uniforms(lib, seed, fp, B, K, t, STREAM_SEQ)
        want, margin = restricted_draw(post, u, mask)
        flips += check_against_rule(out["seq_idx"], want, margin, mask, gm, (geometry, t))
        assert_context_untouched(out, inp, t)
        free = sample(model, inp, init=False, t_start=t, t_stop=t - 1, seed=seed, first_patch=fp, flags=flags)
        for k in STRUCT:  # the structure draws are untouched
            assert torch.equal(out[k], free[k]), (t, k)
    print(f"{geometry}: {flips} sequence draws differ from the restatement (all within the margin)")


# ------------------------------------------------------------------ 5. initial state and optimisation start, on the entries
def test_init_and_noised_start_vs_rules(unit):
    """diffab_sample_init_ex with `allowed`: rule 2 on the STREAM_INIT_S uniforms, exactly (UNK drawn only where it is the whole set), x and
    O bitwise diffab_sample_init's.  diffab_sample_init_noised with `allowed`: rule 3 (q(s_t | s_0) restricted to the set) on the
    STREAM_OPT_SEQ uniforms with the margin rule.  NULL masks are the unconstrained entries, bitwise."""
    dims, model = unit
    lib = _hip.lib()
    P, st = _hip.ptr, _hip.stream_ptr()
    B, K, T, seed, fp = 64, 16, model.T, 77, 9
    inp = patches(B, K, dims, seed=8)
    inp["generation_mask"][:, 2:14] = True
    gm = _hip.dev_mask(inp["generation_mask"])
    mask = random_subsets((B, K), seed=5)
    mask[:4, :] = False
    mask[:4, :, UNK] = True  # {UNK}: drawn
    mask[4:8] = False
    mask[4:8, :, 0] = True
    mask[4:8, :, UNK] = True  # {A, UNK}: UNK left out of the initial state
    words = _pack_words(mask)
    state = lambda: (inp["seq_idx"].clone(), inp["translations"].clone(), inp["orientations"].clone())  # noqa: E731

    s0, x0, O0 = state()
    _hip.check(lib.diffab_sample_init(P(s0), P(x0), P(O0), P(gm), seed, fp, B, K, T, st), "init")
    s1, x1, O1 = state()
    _hip.check(lib.diffab_sample_init_ex(P(s1), P(x1), P(O1), P(gm), seed, fp, B, K, T, 0, P(words), st), "init_ex allowed")
    s2, x2, O2 = state()
    _hip.check(lib.diffab_sample_init_ex(P(s2), P(x2), P(O2), P(gm), seed, fp, B, K, T, 0, None, st), "init_ex NULL")
    assert torch.equal(s2, s0) and torch.equal(x2, x0) and torch.equal(O2, O0)
    assert torch.equal(x1, x0) and torch.equal(O1, O0)
    u = uniforms(lib, seed, fp, B, K, T + 1, STREAM_INIT_S)
    a = mask.clone()
    only_unk = a[..., UNK] & (a.sum(-1) == 1)
    a[..., UNK] = only_unk
    n = a.sum(-1)
    j = torch.minimum((u * n.float()).floor().long(), n - 1)
    want = (a.long().cumsum(-1) == (j + 1).unsqueeze(-1)).long().argmax(-1)  # the j-th allowed class
    g = inp["generation_mask"].cpu()
    assert torch.equal(s1.cpu()[g], want[g])
    assert torch.equal(s1[~inp["generation_mask"]], inp["seq_idx"][~inp["generation_mask"]])
    assert bool((s1.cpu()[:4][g[:4]] == UNK).all()) and bool((s1.cpu()[4:8][g[4:8]] == 0).all())

    sd = model._sched_on_device()
    fwd = model.orientation_diffuser.so3.struct()
    ab = sd.tensors["alpha_bar"].cpu()
    one, c21 = torch.tensor(1.0), torch.tensor(1.0) / torch.tensor(21.0)
    for t in (1, 8, 40, 100):
        s0, x0, O0 = state()
        _hip.check(lib.diffab_sample_init_noised(C.byref(sd.struct), C.byref(fwd), P(s0), P(x0), P(O0), P(gm), seed, fp, B, K, t, 0, None,
                                                 st), t)
        s1, x1, O1 = state()
        _hip.check(lib.diffab_sample_init_noised(C.byref(sd.struct), C.byref(fwd), P(s1), P(x1), P(O1), P(gm), seed, fp, B, K, t, 0,
                                                 P(words), st), t)
        s2, x2, O2 = state()
        _hip.check(lib.diffab_sample_init_noised(C.byref(sd.struct), C.byref(fwd), P(s2), P(x2), P(O2), P(gm), seed, fp, B, K, t, 0,
                                                 None, st), t)
        assert torch.equal(s2, s0) and torch.equal(x2, x0) and torch.equal(O2, O0), t
        assert torch.equal(x1, x0) and torch.equal(O1, O0), t
        wk = ab[t]
        oh = torch.nn.functional.one_hot(inp["seq_idx"].cpu(), V).float()
        p = wk * oh + (one - wk) * c21
        u = uniforms(lib, seed, fp, B, K, t, STREAM_OPT_SEQ)
        want, margin = restricted_draw(p, u, mask)
        check_against_rule(s1, want, margin, mask, inp["generation_mask"], ("noised", t))
        assert torch.equal(s1[~inp["generation_mask"]], inp["seq_idx"][~inp["generation_mask"]]), t


def _pack_words(mask):
    from diffab_pytorch.diffab_pytorch import _pack_allowed_aa

    return _pack_allowed_aa(mask.cuda())


# ------------------------------------------------------------------ 6. sharding and replicated rows
def test_sharding_and_num_samples_with_constraints(bench):
    """Rows [lo, hi) run with first_patch = lo and the matching mask rows are bitwise that slice of the whole run; num_samples with a
    per-patch mask and context_index with a per-row mask are bitwise the replicated batch with the mask replicated."""
    dims, model = bench
    B, K, N = 4, 128, 2
    inp = patches(B, K, dims, seed=71)
    rep = rows(inp, torch.arange(B, device="cuda").repeat_interleave(N))
    mask = random_subsets((B, K), seed=9)
    mrep = mask.repeat_interleave(N, 0)
    kw = dict(seed=21, t_start=30, t_stop=20)
    whole = sample(model, rep, allowed_aa=mrep, **kw)
    parts = [sample(model, {k: v[lo:hi] for k, v in rep.items()}, allowed_aa=mrep[lo:hi], first_patch=lo, **kw)
             for lo, hi in ((0, 3), (3, B * N))]
    assert_bitwise({k: torch.cat([p[k] for p in parts]) for k in whole}, whole, "shards")
    assert_bitwise(sample(model, inp, num_samples=N, allowed_aa=mask, **kw), whole, "num_samples")
    ci = torch.arange(B).repeat_interleave(N)
    shared = {k: rep[k] for k in STATE}
    shared.update({k: inp[k] for k in CTX})
    assert_bitwise(sample(model, shared, context_index=ci, allowed_aa=mrep, **kw), whole, "context_index")
    assert bool(allowed_ok(whole["seq_idx"].cpu(), mrep)[rep["generation_mask"].cpu()].all())
    assert_bitwise(sample(model, rep, optimize_from=8, seed=21, allowed_aa=mrep, graph=True),
                   sample(model, rep, optimize_from=8, seed=21, allowed_aa=mrep), "graph, optimize_from")


# ------------------------------------------------------------------ the C ABI
def test_c_abi_rejects_a_mask_with_keep_sequence(bench):
    """A non-NULL mask with DIFFAB_FLAG_KEEP_SEQUENCE returns DIFFAB_ERR_ARG from all three entries and enqueues nothing."""
    dims, model = bench
    lib = _hip.lib()
    P, st = _hip.ptr, _hip.stream_ptr()
    B, K, T = 2, 128, model.T
    inp = patches(B, K, dims, seed=13)
    s0, x0, O0 = inp["seq_idx"].clone(), inp["translations"].clone(), inp["orientations"].clone()
    gm = _hip.dev_mask(inp["generation_mask"])
    words = _pack_words(torch.ones(B, K, V, dtype=torch.bool))
    keep = _hip.FLAG_KEEP_SEQUENCE
    sd = model._sched_on_device()
    fwd = model.orientation_diffuser.so3.struct()
    dims_c = model.denoiser.hip_dims(B, K)
    w = model.denoiser.hip_weights()
    rev = model._reverse_so3().struct()
    ws = _hip.workspace(lib.diffab_sample_workspace_bytes(C.byref(dims_c)))
    rc_, pc_ = inp["res_context_emb"], inp["pair_context_emb"]
    bad = [
        ("init_ex", lambda: lib.diffab_sample_init_ex(P(s0), P(x0), P(O0), P(gm), 3, 1, B, K, T, keep, P(words), st)),
        ("noised", lambda: lib.diffab_sample_init_noised(C.byref(sd.struct), C.byref(fwd), P(s0), P(x0), P(O0), P(gm), 3, 1, B, K, 8,
                                                        keep, P(words), st)),
        ("loop_ex", lambda: lib.diffab_sample_loop_ex(C.byref(dims_c), C.byref(w.struct), C.byref(sd.struct), C.byref(rev), P(s0), P(x0),
                                                      P(O0), P(rc_), P(pc_), P(gm), 3, 1, 10, 5, P(ws), ws.numel(), keep,
                                                      C.byref(_hip.SampleOptions(n_ctx=B, allowed=P(words))), st)),
    ]
    for what, fn in bad:
        assert fn() == -1, what  # DIFFAB_ERR_ARG
        assert lib.diffab_last_error(), what
    torch.cuda.synchronize()
    assert torch.equal(s0, inp["seq_idx"]) and torch.equal(x0, inp["translations"]) and torch.equal(O0, inp["orientations"])
