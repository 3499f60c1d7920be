"""Fewer-step reverse sampling on the MI355X: DiffAb.sample(steps=...), diffab_sample_options.steps and diffab_reverse_update_jump.

The rule is DESIGN.md section 4.9 / include/diffab_hip.h.  Listing every step is bitwise the ordinary loop on every launch form; a mixed
list is bitwise the ordinary run up to its last stride-1 step; one jump, teacher-forced, is the oracle denoiser followed by the float64
jump; the jump's sequence distribution and translation mean are the known answers of an exact denoiser; a bad plan is refused before
anything is enqueued.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import diffab_oracle as orc
from conftest import maxrel
from diffab_pytorch import _hip, synthetic as syn
from diffab_pytorch.diffusion import jump_coefficients
from sampler_support import CTX, STATE, assert_bitwise, hip, make_model, patches, rows, sample, step_noise, unit_model
from test_respaced_host import posterior_ref, seq_jump_ref

pytestmark = pytest.mark.gpu
V = 21
REC_STATE = ("seq_idx", "translations", "orientations")
TOL = 1e-4


@pytest.fixture(scope="module")
def bench(hip):
    dims = dict(syn.BENCH_DIMS, NL=3)
    return dims, make_model(dims, 19)


def final(out):
    return {k: v for k, v in out.items() if k != "trajectory"}


# ------------------------------------------------------------------ 1. every step listed is the ordinary loop
FORMS = {"eager": {}, "graph": dict(graph=True), "num_samples": dict(num_samples=3),
         "context_index": dict(context_index=torch.tensor([2, 0, 2])), "pair_f32": dict(flags=_hip.FLAG_PAIR_F32),
         "force_generic": dict(flags=_hip.FLAG_FORCE_GENERIC), "skip_unused_rows": dict(skip_unused_rows=True),
         "module_flag": dict(flags=_hip.FLAG_PERSISTENT_MODULE), "codesign": dict(mode="codesign"),
         "fixed_backbone": dict(mode="fixed_backbone"), "structure": dict(mode="structure"), "optimize_from": dict(optimize_from=8),
         "allowed_aa": dict(allowed_aa=torch.rand(3, 128, V, generator=torch.Generator().manual_seed(3)) < 0.6),
         "recording": dict(trajectory=True, trajectory_predictions=True), "recording_graph": dict(trajectory=2, graph=True)}


@pytest.mark.parametrize("form", sorted(FORMS))
def test_every_step_listed_is_the_ordinary_loop(bench, form):
    """steps = L (and the explicit list of every step) is bitwise steps=None, on each launch form and mode."""
    dims, model = bench
    inp = patches(3, 128, dims, seed=6)
    inp["generation_mask"][1, :40] = True
    kw = dict(FORMS[form])
    if form == "allowed_aa":
        kw["allowed_aa"] = kw["allowed_aa"] | ~kw["allowed_aa"].any(-1, keepdim=True)
    hi, lo = (8, 0) if form == "optimize_from" else (30, 22)
    if form != "optimize_from":
        kw.update(t_start=hi, t_stop=lo)
    plain = sample(model, inp, seed=8, **kw)
    assert_bitwise(sample(model, inp, seed=8, steps=hi - lo, **kw), plain, (form, "n = L"))
    assert_bitwise(sample(model, inp, seed=8, steps=list(range(hi, lo, -1)), **kw), plain, (form, "list"))


def test_every_step_listed_module_launch_256_rows(bench):
    """256 rows at K = 128 from 16 contexts: the patch-resident module launch taken by the chip-filling rule."""
    dims, model = bench
    inp = patches(16, 128, dims, seed=41)
    kw = dict(num_samples=16, seed=7, t_start=12, t_stop=4)
    plain = sample(model, inp, **kw)
    assert_bitwise(sample(model, inp, steps=8, **kw), plain, "module")
    assert_bitwise(sample(model, inp, steps=8, graph=True, **kw), plain, "module graph")


# ------------------------------------------------------------------ 2. a mixed list
MIXED = [100, 99, 98, 70, 40, 3, 2, 1]


@pytest.mark.parametrize("form", ["eager", "graph", "allowed_aa"])
def test_mixed_list_is_the_ordinary_run_until_it_jumps(bench, form):
    """[100, 99, 98, 70, 40, 3, 2, 1]: the states at labels 100, 99 and 98 are bitwise the ordinary run's, the jumps then move the
    state away from it, and the result is finite (and within the allowed classes)."""
    dims, model = bench
    inp = patches(3, 128, dims, seed=12)
    kw = dict(seed=5)
    if form == "graph":
        kw["graph"] = True
    if form == "allowed_aa":
        allowed = torch.rand(128, V, generator=torch.Generator().manual_seed(9)) < 0.3
        allowed[:, 0] = True
        kw["allowed_aa"] = allowed
    full = sample(model, inp, trajectory=True, **kw)
    out = sample(model, inp, trajectory=True, steps=MIXED, **kw)
    tr, ftr = out["trajectory"], full["trajectory"]
    assert tr["t"].tolist() == MIXED
    for j, t in enumerate((100, 99, 98)):
        fj = int((ftr["t"] == t).nonzero())
        assert_bitwise({k: tr[k][:, j] for k in REC_STATE}, {k: ftr[k][:, fj] for k in REC_STATE}, t)
    fj = int((ftr["t"] == 70).nonzero())
    gm = inp["generation_mask"]
    assert not torch.equal(tr["translations"][:, 3][gm], ftr["translations"][:, fj][gm])  # step 98 jumped to 70
    for k in ("translations", "orientations"):
        assert bool(torch.isfinite(out[k]).all()), k
    if form == "allowed_aa":
        got = out["seq_idx"][gm]
        assert bool(kw["allowed_aa"].cuda().expand(3, 128, V)[gm].gather(-1, got[:, None]).all())


def test_graph_equals_eager_and_shards_are_slices(bench):
    """A respaced list on graph replay is bitwise eager, and rows [lo, hi) with first_patch = lo are that slice of the whole call."""
    dims, model = bench
    B, K, N = 4, 128, 3
    inp = patches(B, K, dims, seed=71)
    kw = dict(seed=21, t_start=60, t_stop=2, steps=[60, 45, 44, 20, 9, 5, 3])
    whole = sample(model, inp, num_samples=N, **kw)
    assert_bitwise(sample(model, inp, num_samples=N, graph=True, **kw), whole, "graph")
    rep = rows(inp, torch.arange(B, device="cuda").repeat_interleave(N))
    for lo, hi in ((0, 5), (5, 12), (3, 9)):
        part = {k: rep[k][lo:hi] for k in STATE}
        part.update({k: inp[k] for k in CTX})
        got = sample(model, part, context_index=torch.arange(lo, hi) // N, first_patch=lo, **kw)
        assert_bitwise(got, {k: v[lo:hi] for k, v in whole.items()}, (lo, hi))


@pytest.mark.parametrize("n", [20, 10, 3, 1])
def test_even_steps_run_on_every_mode(bench, n):
    """steps = n on each mode and optimize_from: finite, the kept modality untouched, the recorded labels the executed steps."""
    dims, model = bench
    inp = patches(3, 128, dims, seed=33)
    gm = inp["generation_mask"]
    for kw in (dict(), dict(mode="fixed_backbone"), dict(mode="structure"), dict(optimize_from=30, mode="codesign")):
        out = sample(model, inp, seed=4, steps=n, trajectory=True, **kw)
        assert out["trajectory"]["t"].numel() == n
        for k in ("translations", "orientations"):
            assert bool(torch.isfinite(out[k]).all()), (kw, k)
        if kw.get("mode") == "fixed_backbone":
            assert torch.equal(out["translations"], inp["translations"]) and torch.equal(out["orientations"], inp["orientations"])
        if kw.get("mode") == "structure":
            assert torch.equal(out["seq_idx"], inp["seq_idx"])
        assert torch.equal(out["seq_idx"][~gm], inp["seq_idx"][~gm])
        assert bool(((out["seq_idx"] >= 0) & (out["seq_idx"] < V)).all())


# ------------------------------------------------------------------ 3. one jump, teacher-forced, against the oracle
@pytest.mark.parametrize("t, s", [(100, 80), (57, 20), (8, 0), (30, 1)])
def test_jump_teacher_forced_vs_oracle(hip, t, s):
    """sample(t_start=t, steps=[t], t_stop=s, init=False) against oracle.denoiser at beta_t, the host Philox / IGSO3 draws (row t of the
    jump table over sqrt(beta')) and the float64 jump: x and O within 1e-4; a sequence draw may differ only on an edge of r's CDF."""
    dims, model, sd = unit_model()
    sched = orc.cosine_variance_schedule(100, s=0.01, beta_max=0.999)
    B, K, seed = 3, 16, 991
    inp = syn.patches(B, K, dims, seed=4, coord_sigma=5.0)
    gm = inp["generation_mask"]
    got = model.sample(inp["seq_idx"], inp["translations"], inp["orientations"], res_context_emb=inp["res_context_emb"],
                       pair_context_emb=inp["pair_context_emb"], generation_mask=gm, seed=seed, first_patch=10, t_start=t, t_stop=s,
                       steps=[t], init=False)
    steps = torch.tensor([t])
    bj, aj = jump_coefficients(model.sched, steps, s, 0.999)
    rev = model._reverse_so3_steps(steps, s, bj)
    z, rotvec, us = step_noise(seed, 10, B, K, t, rev._cdf[t].cpu(), bj.sqrt()[t])
    den = orc.denoiser(sd, inp["seq_idx"], inp["translations"], inp["orientations"], inp["res_context_emb"], inp["pair_context_emb"],
                       sched["beta"][t].expand(B), dims["NL"], dims["H"])
    c = bj[t] / sched["one_minus_alpha_bar_sqrt"][t]
    x1 = (inp["translations"] - c * den["translations_eps"]) / aj[t].sqrt()
    O1 = den["orientations_t0"]
    if s > 0:
        x1 = x1 + bj[t].sqrt() * z
        O1 = O1 @ orc.rotvec_to_matrix(rotvec)
    x1 = torch.where(gm[..., None], x1, inp["translations"])
    O1 = torch.where(gm[..., None, None], O1, inp["orientations"])
    assert maxrel(got["translations"], x1) < TOL, t
    assert maxrel(got["orientations"], O1) < TOL, t
    ab = sched["alpha_bar"]
    r = seq_jump_ref(den["seq_posterior"].double().numpy(), inp["seq_idx"].numpy(), float(sched["alpha"][t]), float(sched["beta"][t]),
                     float(ab[t - 1]), float(aj[t]), float(ab[s]))
    cdf = np.cumsum(r, -1)
    u = us.double().numpy()[..., None] * cdf[..., -1:]
    s1 = torch.from_numpy(np.minimum((cdf <= u).sum(-1), V - 1))
    s1 = torch.where(gm, s1, inp["seq_idx"])
    diff = (got["seq_idx"].cpu() != s1).numpy()
    if diff.any():  # a draw can flip only when u sits on an edge of r's CDF
        edge = np.abs(cdf - u).min(-1)
        assert float(edge[diff].max()) < 1e-5, (t, int(diff.sum()), float(edge[diff].max()))
    print(f"t={t} -> s={s}: {int(diff.sum())} of {int(gm.sum())} draws on a CDF edge")
    assert torch.equal(got["translations"].cpu()[~gm], inp["translations"][~gm])
    assert torch.equal(got["seq_idx"].cpu()[~gm], inp["seq_idx"][~gm])


# ------------------------------------------------------------------ 4. known answers through diffab_reverse_update_jump
def _jump(lib, sd, t, s, bj, aj, seq, x, O, eps, O0, post, gm, z, rv, us, r_out):
    B, K = seq.shape
    P = _hip.ptr
    return lib.diffab_reverse_update_jump(C.byref(sd.struct), t, s, C.c_float(bj), C.c_float(aj), P(seq), P(x), P(O), P(eps), P(O0), P(post),
                                          P(gm), P(z), P(rv), P(us), P(r_out), B, K, V, _hip.stream_ptr())


def test_jump_known_answers_of_an_exact_denoiser(bench):
    """Every pair s < t - 1 (t = T included), every (s_t, s_0): with p = q(s_{t-1} | s_t, s_0) rounded to fp32, r is the float64
    restatement fed the same p within 1e-6 and q(s_s | s_t, s_0) within 5e-5 (the fp32 rounding of p alone costs up to 6.2e-6); with
    eps_hat = the true eps and no noise, x_s is the DDPM posterior mean of (x_t, x0) for (t, s) wherever beta' is not clipped."""
    _, model = bench
    lib = _hip.lib()
    sd = model._sched_on_device()
    sch = {k: v.double() for k, v in model.sched.items()}
    ab = sch["alpha_bar"]
    T = model.T
    s_t = torch.arange(V).repeat_interleave(V)  # every (s_t, s_0) pair in one row
    s_0 = torch.arange(V).repeat(V)
    K = V * V
    g = torch.Generator().manual_seed(3)
    x0 = torch.randn(1, K, 3, generator=g, dtype=torch.float64) * 5.0
    eps = torch.randn(1, K, 3, generator=g, dtype=torch.float64)
    gm = torch.ones(1, K, dtype=torch.bool, device="cuda")
    O = torch.eye(3).expand(1, K, 3, 3).contiguous().cuda()
    zeros3 = torch.zeros(1, K, 3, device="cuda")
    us = torch.full((1, K), 0.5, device="cuda")
    worst = {"ref": 0.0, "q": 0.0, "x": 0.0}
    for t in range(2, T + 1):
        p32 = posterior_ref(s_t.numpy(), s_0.numpy(), float(sch["alpha"][t]), float(ab[t - 1])).astype(np.float32)
        post = torch.from_numpy(p32)[None].cuda()
        x_t = (ab[t].sqrt() * x0 + (1 - ab[t]).sqrt() * eps).float()
        eps_d = eps.float().cuda()
        for s in range(0, t - 1):
            steps = torch.tensor([t])
            bj_t, aj_t = jump_coefficients(model.sched, steps, s, 0.999)
            bj, aj = float(bj_t[t]), float(aj_t[t])
            seq = s_t[None].cuda().clone()
            x = x_t.cuda()
            r_out = torch.empty(1, K, V, device="cuda")
            assert _jump(lib, sd, t, s, bj, aj, seq, x, O.clone(), eps_d, O, post, gm, zeros3, zeros3, us, r_out) == 0
            r = r_out[0].double().cpu().numpy()
            ref = seq_jump_ref(p32, s_t.numpy(), float(sch["alpha"][t]), float(sch["beta"][t]), float(ab[t - 1]), aj, float(ab[s]))
            q = posterior_ref(s_t.numpy(), s_0.numpy(), aj, float(ab[s]))
            worst["ref"] = max(worst["ref"], float(np.abs(r - ref).max()))
            worst["q"] = max(worst["q"], float(np.abs(r - q).max()))
            b_true = 1.0 - float(ab[t]) / float(ab[s])
            if 1e-5 < b_true < 0.999:  # the DDPM posterior mean of (x_t, x0) for the pair (t, s)
                xt = x_t.double()
                mu = ab[s].sqrt() * b_true / (1 - ab[t]) * x0 + (1 - b_true) ** 0.5 * (1 - ab[s]) / (1 - ab[t]) * xt
                scale = float((xt.abs() + bj / (1 - ab[t]).sqrt() * eps.abs()).max()) / aj ** 0.5
                err = float((x.double().cpu() - mu).abs().max()) / scale
                worst["x"] = max(worst["x"], err)
    print("worst:", worst)
    assert worst["ref"] < 1e-6, worst
    assert worst["q"] < 5e-5, worst
    assert worst["x"] < 1e-5, worst


def test_stride_one_jump_is_reverse_update(bench):
    """diffab_reverse_update_jump(t, t - 1, beta[t], alpha[t]) is bitwise diffab_reverse_update, and r_out is the posterior."""
    _, model = bench
    lib = _hip.lib()
    sd = model._sched_on_device()
    P, st = _hip.ptr, _hip.stream_ptr()
    B, K = 3, 64
    g = torch.Generator().manual_seed(11)
    seq0 = torch.randint(0, V, (B, K), generator=g).cuda()
    x0 = (torch.randn(B, K, 3, generator=g) * 4).cuda()
    O0 = torch.linalg.qr(torch.randn(B, K, 3, 3, generator=g))[0].cuda()
    eps = torch.randn(B, K, 3, generator=g).cuda()
    Oh = torch.linalg.qr(torch.randn(B, K, 3, 3, generator=g))[0].cuda()
    post = torch.softmax(torch.randn(B, K, V, generator=g) * 3, -1).cuda()
    gm = (torch.rand(B, K, generator=g) < 0.7).cuda()
    z = torch.randn(B, K, 3, generator=g).cuda()
    rv = (torch.randn(B, K, 3, generator=g) * 0.3).cuda()
    us = torch.rand(B, K, generator=g).cuda()
    for t in (100, 57, 2, 1):
        a = [seq0.clone(), x0.clone(), O0.clone()]
        b = [seq0.clone(), x0.clone(), O0.clone()]
        assert lib.diffab_reverse_update(C.byref(sd.struct), t, P(a[0]), P(a[1]), P(a[2]), P(eps), P(Oh), P(post), P(gm), P(z), P(rv), P(us),
                                         B, K, V, st) == 0
        r_out = torch.zeros(B, K, V, device="cuda")
        assert _jump(lib, sd, t, t - 1, float(model.sched["beta"][t]), float(model.sched["alpha"][t]), b[0], b[1], b[2], eps, Oh, post, gm,
                     z, rv, us, r_out) == 0
        for u, v in zip(a, b):
            assert torch.equal(u, v), t
        assert torch.equal(r_out[gm], post[gm])


# ------------------------------------------------------------------ 5. the C ABI refuses bad plans
def test_c_abi_rejects_bad_plans(bench):
    """Each bad plan returns DIFFAB_ERR_ARG; the state and the device plan are untouched afterwards (nothing was enqueued)."""
    dims, model = bench
    lib = _hip.lib()
    P, st = _hip.ptr, _hip.stream_ptr()
    B, K, T = 2, 128, model.T
    inp = patches(B, K, dims, seed=13)
    s0, x0, O0 = inp["seq_idx"].clone(), inp["translations"].clone(), inp["orientations"].clone()
    gm = _hip.dev_mask(inp["generation_mask"])
    sd = model._sched_on_device()
    dims_c = model.denoiser.hip_dims(B, K)
    w = model.denoiser.hip_weights()
    rev = model._reverse_so3().struct()
    ws = _hip.workspace(lib.diffab_sample_workspace_bytes(C.byref(dims_c)))
    rc_, pc_ = inp["res_context_emb"], inp["pair_context_emb"]
    plan_dev = torch.full((3 * (T + 1),), 77, dtype=torch.int32, device="cuda")
    t_start, t_stop = 10, 2
    good = [10, 8, 5, 3]
    bj, aj = jump_coefficients(model.sched, torch.tensor(good), t_stop, 0.999)

    def plan(steps=good, beta=None, alpha=None, n=None, drop=()):
        b = (bj if beta is None else beta).tolist()
        a = (aj if alpha is None else alpha).tolist()
        return _hip.SampleSteps(len(steps) if n is None else n, None if "steps" in drop else (C.c_int32 * max(len(steps), 1))(*steps),
                                None if "beta" in drop else (C.c_float * (T + 1))(*b),
                                None if "alpha" in drop else (C.c_float * (T + 1))(*a), None if "plan" in drop else P(plan_dev))

    def setat(tab, t, v):
        out = tab.clone()
        out[t] = v
        return out

    slot_dev = torch.full((T + 1,), 77, dtype=torch.int32, device="cuda")
    rec_buf = {"seq": torch.zeros(B, 2, K, dtype=torch.int64, device="cuda"), "x": torch.zeros(B, 2, K, 3, device="cuda"),
               "O": torch.zeros(B, 2, K, 3, 3, device="cuda")}

    def record(entries):
        tab = [-1] * (T + 1)
        for t, j in entries.items():
            tab[t] = j
        return _hip.SampleRecord(2, (C.c_int32 * (T + 1))(*tab), P(slot_dev), P(rec_buf["seq"]), P(rec_buf["x"]), P(rec_buf["O"]), None,
                                 None, None)

    bad = {"n_steps 0": (plan(n=0), None), "null steps": (plan(drop=("steps",)), None), "null beta": (plan(drop=("beta",)), None),
           "null alpha": (plan(drop=("alpha",)), None), "null plan": (plan(drop=("plan",)), None),
           "first is not t_start": (plan(steps=[9, 8, 5, 3]), None), "repeated step": (plan(steps=[10, 8, 8, 3]), None),
           "ascending": (plan(steps=[10, 5, 8, 3]), None), "at t_stop": (plan(steps=[10, 8, 5, 2]), None),
           "below t_stop": (plan(steps=[10, 8, 1]), None), "above T": (plan(steps=[10, 101]), None),
           "beta' 0": (plan(beta=setat(bj, 8, 0.0)), None), "beta' 1": (plan(beta=setat(bj, 5, 1.0)), None),
           "beta' nan": (plan(beta=setat(bj, 10, float("nan"))), None), "alpha' 0": (plan(alpha=setat(aj, 3, 0.0)), None),
           "alpha' 1": (plan(alpha=setat(aj, 3, 1.0)), None),
           "record slot off the list": (plan(), record({10: 0, 9: 1}))}
    def loop(pl, rec):
        return lib.diffab_sample_loop_ex(C.byref(dims_c), C.byref(w.struct), C.byref(sd.struct), C.byref(rev), P(s0), P(x0), P(O0), P(rc_),
                                         P(pc_), P(gm), 3, 1, t_start, t_stop, P(ws), ws.numel(), 0,
                                         C.byref(_hip.SampleOptions(n_ctx=B, record=rec, steps=pl)), st)

    for what, (pl, rec) in bad.items():
        assert loop(pl, rec) == -1, what  # DIFFAB_ERR_ARG
    torch.cuda.synchronize()
    assert torch.equal(s0, inp["seq_idx"]) and torch.equal(x0, inp["translations"]) and torch.equal(O0, inp["orientations"])
    assert bool((plan_dev == 77).all()) and bool((slot_dev == 77).all())
    # the good plan runs and fills the device plan: next[] along the list, the coefficients bit for bit
    ok = plan()
    assert loop(ok, record({10: 0, 5: 1})) == 0
    torch.cuda.synchronize()
    pd = plan_dev.cpu()
    assert pd[[10, 8, 5, 3]].tolist() == [8, 5, 3, 2]
    assert torch.equal(pd[T + 1:2 * (T + 1)].view(torch.float32), bj) and torch.equal(pd[2 * (T + 1):].view(torch.float32), aj)
    assert slot_dev[[10, 5]].tolist() == [0, 1]
