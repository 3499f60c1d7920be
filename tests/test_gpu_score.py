"""Design scoring on the MI355X: DiffAb.score / diffab_score_designs.

The noised state of every evaluated row matches the oracle's forward process on the same Philox lanes and is, for draw 0, exactly the
optimisation start of the sampler; the per-residue and per-row terms match the oracle's denoiser and the reference's element losses on that
state; and the result is bitwise invariant under chunking, launch form, shared contexts, design ranges and grid splits.
"""
import ctypes as C

import pytest
import torch

import diffab_oracle as orc
from conftest import elemrel, maxrel
from diffab_pytorch import _hip, synthetic as syn
from sampler_support import CTX, STATE, STREAMS_OPT, hip, make_model, patches, score, step_noise

pytestmark = pytest.mark.gpu
TOL = 1e-4  # as tests/test_gpu_parity.py
NOISED = ("seq_idx_t", "translations_t", "orientations_t", "translations_eps")


@pytest.fixture(scope="module")
def unit(hip):
    dims = dict(syn.UNIT_DIMS, NL=2)
    return dims, make_model(dims, 17)


@pytest.fixture(scope="module")
def bench(hip):
    dims = dict(syn.BENCH_DIMS, NL=3)
    return dims, make_model(dims, 19)


def assert_bitwise(got, want, what=""):
    for k in ("seq_loss", "translations_loss", "orientations_loss", "loss", "per_step", "t"):
        assert torch.equal(got[k], want[k]) or (torch.equal(got[k].isnan(), want[k].isnan()) and
                                                 torch.equal(got[k].nan_to_num(), want[k].nan_to_num())), (what, k)


def oracle_terms(sd, NL, H, sched, seq0, O0, gm, rm, nz, res_ctx, pair_ctx, t):
    """The reference's element losses (diffab_pytorch.py:856-880 before the reduction, summed over their trailing axes) of the oracle's
    denoiser on a noised state, in float64: (B, K, 3)."""
    B = seq0.shape[0]
    d = lambda v: v.detach().cpu().double()
    beta = sched["beta"].double()[t].expand(B)
    den = orc.denoiser(sd, nz["seq_idx_t"].cpu(), d(nz["translations_t"]), d(nz["orientations_t"]), d(res_ctx), d(pair_ctx), beta, NL, H)
    tt = torch.full((B,), t, dtype=torch.long)
    q = orc.seq_posterior_single_step(nz["seq_idx_t"].cpu(), seq0.cpu(), tt, gm.cpu(), sched, dtype=torch.float64)
    p = den["aa_logits"].softmax(-1)
    kl = (torch.xlogy(q, q) - q * p.log()).sum(-1)
    mse = ((den["translations_eps"] - d(nz["translations_eps"])) ** 2).sum(-1)
    ol = orc.orientation_loss_elems(den["orientations_t0"], d(O0)).sum((-1, -2))
    m = (gm & rm).cpu()
    return torch.stack([kl, mse, ol], -1) * m[..., None]


def row_means(per_res, m):
    return per_res.sum(-2) / m.sum(-1, keepdim=True)


# ------------------------------------------------------------------ 1. noised state vs the oracle's forward process
def test_noised_state_vs_oracle(unit):
    """Every (design, t, draw) row: x_t, O_t and eps within TOL of the oracle's forward process driven by Philox with stream
    STREAM_OPT_* + (m << 16) (t on both branches of the forward IGSO3 table); a sequence draw may differ only on a CDF edge; context
    residues are bitwise the input."""
    dims, model = unit
    sched = orc.cosine_variance_schedule(100, s=0.01, beta_max=0.999)
    R, K, M, seed, fd = 6, 16, 2, 2024, 5
    grid = [1, 3, 5, 6, 8, 40, 100]
    inp = patches(R, K, dims, seed=9)
    inp["generation_mask"][:, :12] = True
    out = score(model, inp, t=grid, num_draws=M, seed=seed, first_design=fd, return_noised=True)
    nz = {k: v.cpu() for k, v in out["noised"].items()}
    assert out["t"].tolist() == grid and out["per_step"].shape == (R, len(grid), M, 3)
    cpu = {k: v.cpu() for k, v in inp.items()}
    gm = cpu["generation_mask"]
    cdf = model.orientation_diffuser.so3._cdf.cpu()
    sig = sched["one_minus_alpha_bar_sqrt"]
    cos = (cpu["orientations"].diagonal(dim1=-2, dim2=-1).sum(-1) - 1) / 2
    ok = gm & ((cos - 1).abs() >= 1e-2) & ((cos + 1).abs() >= 1e-2)  # scale_rot is defined away from theta in {0, pi}
    flips = 0
    for j, t in enumerate(grid):
        for m in range(M):
            tt = torch.full((R,), t, dtype=torch.long)
            eps, rotvec, us = step_noise(seed, fd, R, K, t, cdf[t], sig[t], streams=STREAMS_OPT, draw=m)
            x1 = orc.coord_diffuse_from_t0(cpu["translations"], tt, gm, eps, sched)
            O1 = orc.orient_diffuse_from_t0(cpu["orientations"], gm, tt, rotvec, sched)
            p = orc.seq_forward_prob_from_t0(cpu["seq_idx"], tt, gm, sched)
            s1 = orc.categorical_from_uniform(p, us)
            got = {k: nz[k][:, j, m] for k in NOISED}
            assert maxrel(got["translations_t"], x1) < TOL, (t, m)
            assert maxrel(got["orientations_t"][ok], O1[ok]) < TOL, (t, m)
            assert maxrel(got["translations_eps"][gm], eps[gm]) < TOL, (t, m)
            assert torch.equal(got["translations_eps"][~gm], torch.zeros_like(got["translations_eps"][~gm])), (t, m)
            diff = (got["seq_idx_t"] != s1) & gm
            if diff.any():
                edge = (p.double().cumsum(-1) - us.double()[..., None]).abs().min(dim=-1).values
                assert float(edge[diff].max()) < 1e-5, (t, m, int(diff.sum()))
                flips += int(diff.sum())
            for k, ki in (("seq_idx_t", "seq_idx"), ("translations_t", "translations"), ("orientations_t", "orientations")):
                assert torch.equal(got[k][~gm], cpu[ki][~gm]), (t, m, k)
        assert not torch.equal(nz["translations_t"][:, j, 0], nz["translations_t"][:, j, 1]), t  # the draws differ
    print(f"score noising: {flips} sequence draws on a CDF edge")


# ------------------------------------------------------------------ 2. draw 0 is the sampler's optimisation start
@pytest.mark.parametrize("mode", [None, "fixed_backbone", "structure"])
def test_draw_zero_is_the_optimisation_start(unit, mode):
    dims, model = unit
    R, K, fd, seed = 5, 16, 3, 77
    grid = [2, 9, 50]
    inp = patches(R, K, dims, seed=4)
    out = score(model, inp, t=grid, num_draws=2, seed=seed, first_design=fd, mode=mode, return_noised=True)
    for j, t in enumerate(grid):
        s = model.sample(inp["seq_idx"], inp["translations"], inp["orientations"], generation_mask=inp["generation_mask"],
                         res_context_emb=inp["res_context_emb"], pair_context_emb=inp["pair_context_emb"], mode=mode, optimize_from=t,
                         t_stop=t, seed=seed, first_patch=fd)
        for k, ks in (("seq_idx_t", "seq_idx"), ("translations_t", "translations"), ("orientations_t", "orientations")):
            assert torch.equal(out["noised"][k][:, j, 0], s[ks]), (mode, t, k)


# ------------------------------------------------------------------ 3. terms vs the oracle on the device's own noised state
def check_terms(model, dims, inp, out, designs, steps, M):
    sched = orc.cosine_variance_schedule(100, s=0.01, beta_max=0.999)
    sd = {"denoiser." + k: v.detach().cpu() for k, v in model.denoiser.state_dict().items()}
    rm = inp.get("residue_mask", torch.ones_like(inp["generation_mask"]))
    got_r, want_r, got_s, want_s = [], [], [], []
    for j in steps:
        t = int(out["t"][j])
        for m in range(M):
            nz = {k: v[designs, j, m] for k, v in out["noised"].items()}
            ctx = {k: inp[k][designs] for k in CTX}
            want = oracle_terms(sd, dims["NL"], dims["H"], sched, inp["seq_idx"][designs], inp["orientations"][designs],
                                inp["generation_mask"][designs], rm[designs], nz, ctx["res_context_emb"], ctx["pair_context_emb"], t)
            got_r.append(out["per_residue"][designs, j, m].cpu().double())
            want_r.append(want)
            got_s.append(out["per_step"][designs, j, m].cpu().double())
            want_s.append(row_means(want, (inp["generation_mask"] & rm)[designs].cpu()))
    gr, wr, gs, ws_ = (torch.stack(v) for v in (got_r, want_r, got_s, want_s))
    for c in range(3):
        assert maxrel(gr[..., c], wr[..., c]) < TOL and elemrel(gr[..., c], wr[..., c]) < TOL, ("per_residue", c, maxrel(gr[..., c], wr[..., c]),
                                                                                              elemrel(gr[..., c], wr[..., c]))
        assert maxrel(gs[..., c], ws_[..., c]) < TOL and elemrel(gs[..., c], ws_[..., c]) < TOL, ("per_step", c)
    assert (wr != 0).any(-1).any(), "vacuous"


def test_terms_vs_oracle_unit(unit):
    dims, model = unit
    R, K, M = 6, 16, 2
    inp = patches(R, K, dims, seed=21)
    inp["generation_mask"][:, 2:10] = True
    inp["residue_mask"] = torch.ones_like(inp["generation_mask"])
    inp["residue_mask"][:, 4] = False
    out = score(model, inp, t=[1, 4, 7, 30, 99], num_draws=M, seed=5, per_residue=True, return_noised=True)
    check_terms(model, dims, inp, out, torch.arange(R, device="cuda"), range(5), M)
    # unmasked residues carry zero terms; the means are the per-step means over the grid and the draws
    assert torch.equal(out["per_residue"][:, :, :, 4], torch.zeros_like(out["per_residue"][:, :, :, 4]))
    mean = out["per_step"].mean(dim=(1, 2))
    assert torch.equal(out["seq_loss"], mean[:, 0]) and torch.equal(out["orientations_loss"], mean[:, 2])
    assert torch.equal(out["loss"], mean[:, 0] + mean[:, 1] + mean[:, 2])


def test_terms_vs_oracle_bench_slice_module_launch(bench):
    """256 rows at K = 128 (16 designs from 4 contexts x a 16-step grid, one chunk: the patch-resident module launch); 4 designs x 3 steps
    against the oracle."""
    dims, model = bench
    n_ctx, R, K = 4, 16, 128
    ctx = patches(n_ctx, K, dims, seed=31)
    ci = torch.arange(R) % n_ctx
    inp = {k: ctx[k][ci.cuda()] for k in STATE}
    inp["generation_mask"][:, 40:60] = True
    grid = list(range(3, 100, 6))[:16]
    out = model.score(inp["seq_idx"], inp["translations"], inp["orientations"], generation_mask=inp["generation_mask"],
                      res_context_emb=ctx["res_context_emb"], pair_context_emb=ctx["pair_context_emb"], context_index=ci, t=grid, seed=9,
                      per_residue=True, return_noised=True, rows_per_launch=256)
    full = dict(inp, **{k: ctx[k][ci.cuda()] for k in CTX})
    check_terms(model, dims, full, out, torch.tensor([0, 5, 10, 15], device="cuda"), [0, 7, 15], 1)


# ------------------------------------------------------------------ 4. one column of per_step vs hotpath_losses(denoise(...))
def test_one_column_is_the_training_losses(bench):
    dims, model = bench
    R, K = 4, 128
    inp = patches(R, K, dims, seed=33)
    inp["generation_mask"][:, 10:30] = True
    rm = torch.ones_like(inp["generation_mask"])
    t = 23
    out = score(model, inp, t=[5, t], num_draws=2, seed=3, return_noised=True)
    sched = orc.cosine_variance_schedule(100, s=0.01, beta_max=0.999)
    for m in range(2):
        nz = {k: v[:, 1, m].contiguous() for k, v in out["noised"].items()}
        beta = model.sched["beta"][t].expand(R).cuda().contiguous()
        den = model.denoise(nz["seq_idx_t"], nz["translations_t"], nz["orientations_t"], inp["res_context_emb"], inp["pair_context_emb"], beta,
                            inp["generation_mask"], rm)
        post = orc.seq_posterior_single_step(nz["seq_idx_t"].cpu(), inp["seq_idx"].cpu(), torch.full((R,), t), inp["generation_mask"].cpu(),
                                             sched).cuda()
        for r in range(R):
            sl = slice(r, r + 1)
            want = model.hotpath_losses({k: v[sl] for k, v in den.items()}, {"seq_posterior": post[sl], "translations_eps": nz["translations_eps"][sl]},
                                        inp["orientations"][sl], inp["generation_mask"][sl], rm[sl])
            for c in range(3):
                w = float(want[c])
                assert abs(float(out["per_step"][r, 1, m, c]) - w) <= 1e-5 * abs(w), (m, r, c, float(out["per_step"][r, 1, m, c]), w)


# ------------------------------------------------------------------ 5. bitwise invariances at the benchmark geometry
@pytest.fixture(scope="module")
def workload(bench):
    dims, model = bench
    n_ctx, N, K = 16, 4, 128
    ctx = patches(n_ctx, K, dims, seed=51)
    ci = torch.arange(n_ctx).repeat_interleave(N)
    R = n_ctx * N
    g = torch.Generator().manual_seed(5)
    inp = {k: ctx[k][ci.cuda()].clone() for k in STATE}
    inp["translations"] = inp["translations"] + torch.randn(R, K, 3, generator=g).cuda()  # the designs of a context differ
    inp["seq_idx"] = torch.where(inp["generation_mask"], torch.randint(0, 20, (R, K), generator=g).cuda(), inp["seq_idx"])
    return dims, model, ctx, ci, inp


def test_invariances_bench(workload):
    dims, model, ctx, ci, inp = workload
    grid = [1, 4, 9, 17, 33, 52, 75, 100]
    kw = dict(t=grid, seed=12)

    def run(sub=None, **extra):
        sub = slice(None) if sub is None else sub
        return model.score(inp["seq_idx"][sub], inp["translations"][sub], inp["orientations"][sub], generation_mask=inp["generation_mask"][sub],
                           res_context_emb=ctx["res_context_emb"], pair_context_emb=ctx["pair_context_emb"], context_index=ci[sub],
                           **dict(kw, **extra))

    base = run(rows_per_launch=512)
    assert torch.isfinite(base["per_step"]).all() and (base["per_step"] > 0).all()
    assert_bitwise(run(rows_per_launch=256), base, "rows_per_launch 256")
    assert_bitwise(run(rows_per_launch=100), base, "rows_per_launch 100 (ragged)")
    assert_bitwise(run(rows_per_launch=256, flags=_hip.FLAG_MULTI_LAUNCH), base, "multi-launch")
    rep = model.score(inp["seq_idx"], inp["translations"], inp["orientations"], generation_mask=inp["generation_mask"],
                      res_context_emb=ctx["res_context_emb"][ci.cuda()], pair_context_emb=ctx["pair_context_emb"][ci.cuda()], rows_per_launch=512,
                      **kw)
    assert_bitwise(rep, base, "replicated contexts")
    lo, hi = 13, 41
    part = run(slice(lo, hi), first_design=lo, rows_per_launch=512)
    for k in ("per_step", "loss", "seq_loss"):
        assert torch.equal(part[k], base[k][lo:hi]), ("design range", k)
    a = run(rows_per_launch=256, t=grid[:3])
    b = run(rows_per_launch=256, t=grid[3:])
    assert torch.equal(torch.cat([a["per_step"], b["per_step"]], 1), base["per_step"]), "grid split"


# ------------------------------------------------------------------ 6. modes
@pytest.mark.parametrize("mode", ["fixed_backbone", "structure"])
def test_modes_keep_their_modality(unit, mode):
    dims, model = unit
    R, K, M = 4, 16, 2
    inp = patches(R, K, dims, seed=61)
    grid = [3, 20, 80]
    out = score(model, inp, t=grid, num_draws=M, seed=8, mode=mode, return_noised=True, per_residue=True)
    co = score(model, inp, t=grid, num_draws=M, seed=8, return_noised=True)
    nz = out["noised"]
    shape = (R, len(grid), M, K)
    if mode == "fixed_backbone":
        for k, ki in (("translations_t", "translations"), ("orientations_t", "orientations")):
            assert torch.equal(nz[k], inp[ki][:, None, None].expand(*shape, *inp[ki].shape[2:])), k
        assert torch.equal(nz["translations_eps"], torch.zeros_like(nz["translations_eps"]))
        assert torch.equal(nz["seq_idx_t"], co["noised"]["seq_idx_t"])
        zero, kept = (1, 2), (0,)
    else:
        assert torch.equal(nz["seq_idx_t"], inp["seq_idx"][:, None, None].expand(shape))
        for k in ("translations_t", "orientations_t", "translations_eps"):
            assert torch.equal(nz[k], co["noised"][k]), k
        zero, kept = (0,), (1, 2)
    for c in zero:
        assert torch.equal(out["per_step"][..., c], torch.zeros_like(out["per_step"][..., c])), c
        assert torch.equal(out["per_residue"][..., c], torch.zeros_like(out["per_residue"][..., c])), c
    assert (out["per_step"][..., list(kept)] > 0).all()
    names = ("seq_loss", "translations_loss", "orientations_loss")
    assert torch.equal(out["loss"], sum(out[names[c]] for c in kept))


# ------------------------------------------------------------------ 7. the C ABI refuses bad arguments before any launch
def test_c_abi_argument_errors(unit):
    dims, model = unit
    lib = _hip.lib()
    R, K = 3, 16
    inp = patches(R, K, dims, seed=71)
    d = model.denoiser.hip_dims(8, K)
    w = model.denoiser.hip_weights()
    sd = model._sched_on_device()
    fwd = model.orientation_diffuser.so3.struct()
    ws_bytes = lib.diffab_score_workspace_bytes(C.byref(d), 2)
    ws = _hip.workspace(ws_bytes)
    P = _hip.ptr
    seq, x, O = inp["seq_idx"], inp["translations"], inp["orientations"]
    gm = _hip.dev_mask(inp["generation_mask"])
    rc, pc = inp["res_context_emb"][:2].contiguous(), inp["pair_context_emb"][:2].contiguous()
    terms = torch.full((R, 2, 1, 3), 7.0, device="cuda")
    st = _hip.stream_ptr()

    def call(t=(3, 5), n_draws=1, ctx=(0, 1, 1), out=terms, nbytes=ws_bytes, n_ctx=2):
        th = (C.c_int32 * len(t))(*t)
        ch = (C.c_int32 * len(ctx))(*ctx)
        return lib.diffab_score_designs(C.byref(d), C.byref(w.struct), C.byref(sd.struct), C.byref(fwd), P(seq), P(x), P(O), P(gm), None, R,
                                        P(rc), P(pc), n_ctx, ch, th, len(t), n_draws, 1, 0, P(out), None, None, P(ws), nbytes, 0, st)

    bad = [("t = 0", dict(t=(0, 5))), ("t = T + 1", dict(t=(3, 101))), ("duplicate t", dict(t=(3, 3))), ("n_draws = 0", dict(n_draws=0)),
           ("context index out of range", dict(ctx=(0, 2, 1))), ("negative context index", dict(ctx=(0, -1, 1))),
           ("null out_terms", dict(out=None)), ("workspace too small", dict(nbytes=ws_bytes - 1))]
    for what, kw in bad:
        rc_ = call(**kw)
        assert rc_ in (-1, -4), what  # DIFFAB_ERR_ARG / DIFFAB_ERR_WORKSPACE
        assert rc_ == (-4 if what == "workspace too small" else -1), what
        assert lib.diffab_last_error(), what
    torch.cuda.synchronize()
    assert torch.equal(terms, torch.full_like(terms, 7.0)), "a refused call wrote its output"
    assert call() == 0
    torch.cuda.synchronize()
    assert torch.isfinite(terms).all() and not torch.equal(terms, torch.full_like(terms, 7.0))
