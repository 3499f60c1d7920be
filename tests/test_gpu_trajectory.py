"""Trajectory recording of the sampler on the MI355X: DiffAb.sample(trajectory=...) and diffab_sample_options.record.

The specification (include/diffab_hip.h): label t holds the state that step t denoises - bitwise the same call
with t_stop = t - and, with predictions, what the denoiser made of it (x0_hat, O0_hat, the softmax posterior over s_{t-1}).  Recording
does not change the sample, on any launch form; residues that are not generated and a kept modality hold their given values; a shard of
rows records that slice of the whole call's trajectory; a bad record is refused before anything is enqueued.
"""
import ctypes as C

import pytest
import torch

from conftest import maxrel
from diffab_pytorch import _hip, synthetic as syn
from sampler_support import CTX, STATE, assert_bitwise, hip, make_model, patches, rows, sample

pytestmark = pytest.mark.gpu
V = 21
REC_STATE = ("seq_idx", "translations", "orientations")
REC_PRED = ("pred_translations", "pred_orientations", "seq_probs")
DENOISE_TOL = 1e-5  # loop vs model.denoise on the same state: the same kernels up to summation order (test_gpu_aa_constraints' margin)


@pytest.fixture(scope="module")
def bench(hip):
    dims = dict(syn.BENCH_DIMS, NL=3)
    return dims, make_model(dims, 19)


def final(out):
    return {k: v for k, v in out.items() if k != "trajectory"}


def slot(tr, t):
    return int((tr["t"] == t).nonzero())


# ------------------------------------------------------------------ 1. recording is invisible
FORMS = {"per_layer": {}, "graph": dict(graph=True), "num_samples": dict(num_samples=3),
         "context_index": dict(context_index=torch.tensor([2, 0, 2])), "pair_f32": dict(flags=_hip.FLAG_PAIR_F32),
         "force_generic": dict(flags=_hip.FLAG_FORCE_GENERIC),
         "skip_unused_rows": dict(skip_unused_rows=True), "module_flag": dict(flags=_hip.FLAG_PERSISTENT_MODULE),
         "fixed_backbone": dict(mode="fixed_backbone"), "optimize_from": dict(optimize_from=8), "structure": dict(mode="structure"),
         "allowed_aa": dict(allowed_aa=torch.rand(3, 128, V, generator=torch.Generator().manual_seed(3)) < 0.6)}


@pytest.mark.parametrize("form", sorted(FORMS))
def test_recording_is_invisible(bench, form):
    """With every step and its predictions recorded, the returned state is bitwise the run without a trajectory, on each launch form."""
    dims, model = bench
    inp = patches(3, 128, dims, seed=6)
    inp["generation_mask"][1, :40] = True
    kw = dict(FORMS[form])
    if form == "allowed_aa":
        kw["allowed_aa"] = kw["allowed_aa"] | ~kw["allowed_aa"].any(-1, keepdim=True)
    if form != "optimize_from":
        kw.update(t_start=30, t_stop=22)
    plain = sample(model, inp, seed=8, **kw)
    out = sample(model, inp, seed=8, trajectory=True, trajectory_predictions=True, **kw)
    assert_bitwise(final(out), plain, form)
    tr = out["trajectory"]
    n = 8
    assert tr["t"].tolist() == list(range(30 if form != "optimize_from" else 8, 22 if form != "optimize_from" else 0, -1))
    R = plain["seq_idx"].shape[0]
    assert tr["seq_idx"].shape == (R, n, 128) and tr["seq_idx"].dtype == torch.int64
    assert tr["translations"].shape == tr["pred_translations"].shape == (R, n, 128, 3)
    assert tr["orientations"].shape == tr["pred_orientations"].shape == (R, n, 128, 3, 3)
    assert tr["seq_probs"].shape == (R, n, 128, V)
    for k in REC_STATE + REC_PRED:
        assert tr[k].is_cuda and (tr[k].dtype == torch.int64 or bool(torch.isfinite(tr[k]).all())), (form, k)


def test_recording_is_invisible_module_launch_256_rows(bench):
    """256 rows at K = 128 from 16 contexts: the patch-resident module launch taken by the chip-filling rule, not by the flag."""
    dims, model = bench
    inp = patches(16, 128, dims, seed=41)
    kw = dict(num_samples=16, seed=7, t_start=12, t_stop=4)
    out = sample(model, inp, trajectory=3, trajectory_predictions=True, **kw)
    assert_bitwise(final(out), sample(model, inp, **kw), "module")
    assert out["trajectory"]["t"].tolist() == [12, 9, 6]


# ------------------------------------------------------------------ 2. states are the truncated runs
@pytest.mark.parametrize("form", ["eager", "graph", "module_flag", "optimize_from", "num_samples"])
def test_states_are_the_truncated_runs(bench, form):
    """The state at label t is bitwise sample(..., t_stop=t) with the same arguments, for t_start, t_stop + 1 and labels between; the
    final state is the return value and is not repeated."""
    dims, model = bench
    inp = patches(3, 128, dims, seed=12)
    kw = {"eager": dict(t_start=30, t_stop=22), "graph": dict(t_start=30, t_stop=22, graph=True),
          "module_flag": dict(t_start=30, t_stop=22, flags=_hip.FLAG_PERSISTENT_MODULE), "optimize_from": dict(optimize_from=9, t_stop=1),
          "num_samples": dict(t_start=30, t_stop=22, num_samples=2)}[form]
    kw["seed"] = 5
    out = sample(model, inp, trajectory=True, **kw)
    tr = out["trajectory"]
    hi, lo = int(tr["t"][0]), int(tr["t"][-1])
    assert set(tr) == {"t", *REC_STATE} and lo == kw["t_stop"] + 1
    for t in sorted({hi, hi - 1, (hi + lo) // 2, lo + 1, lo}, reverse=True):
        want = sample(model, inp, **dict(kw, t_stop=t))
        got = {k: tr[k][:, slot(tr, t)] for k in REC_STATE}
        assert_bitwise(got, want, (form, t))
    if form == "optimize_from":  # label t_start: the forward-noised native, not the given state
        gm = inp["generation_mask"]
        assert not torch.equal(tr["translations"][:, 0][gm], inp["translations"][gm])
    for k in ("translations", "orientations"):  # the last step moves the structure: the final state is not in the record
        assert not torch.equal(tr[k][:, -1], out[k]), k


# ------------------------------------------------------------------ 3. predictions are the denoiser's
def test_predictions_are_the_denoisers(bench):
    """At labels 90, 50 and 3 of a full run, on the recorded state s_t: O0_hat and seq_probs are model.denoise's at beta_t within
    DENOISE_TOL (max-relative); x0_hat is the formula on denoise's eps_hat.  x0_hat = (x_t - b_t eps_hat) / a_t is linear in eps_hat with
    slope b_t / a_t (6.4 at t = 90), so an eps_hat that agrees to DENOISE_TOL of its largest entry moves x0_hat by up to
    DENOISE_TOL max|eps_hat| b_t / a_t; the fp32 evaluation of the formula itself adds a few ulps of max|x0_hat|."""
    dims, model = bench
    B, K = 3, 128
    inp = patches(B, K, dims, seed=31)
    out = sample(model, inp, seed=4, trajectory=[90, 50, 3], trajectory_predictions=True)
    tr = out["trajectory"]
    gm = inp["generation_mask"]
    rm = torch.ones_like(gm)
    sch = {k: v.cuda() for k, v in model.sched.items()}
    for j, t in enumerate(tr["t"].tolist()):
        beta = sch["beta"][t].expand(B).contiguous()
        with torch.no_grad():
            d = model.denoise(tr["seq_idx"][:, j], tr["translations"][:, j], tr["orientations"][:, j], inp["res_context_emb"],
                              inp["pair_context_emb"], beta, gm, rm)
        e_O = maxrel(tr["pred_orientations"][:, j][gm], d["orientations_t0"][gm])
        e_p = maxrel(tr["seq_probs"][:, j][gm], d["seq_posterior"][gm])
        a, b = sch["alpha_bar_sqrt"][t], sch["one_minus_alpha_bar_sqrt"][t]
        eps = d["translations_eps"][gm]
        want_x = (tr["translations"][:, j][gm] - b * eps) / a
        err_x = float((tr["pred_translations"][:, j][gm] - want_x).abs().max())
        bound = DENOISE_TOL * float(eps.abs().max()) * float(b / a) + 8 * 2.0 ** -23 * float(want_x.abs().max())
        print(f"t={t}: O0 {e_O:.2e}, probs {e_p:.2e}, x0 {err_x:.2e} (bound {bound:.2e})")
        assert e_O < DENOISE_TOL and e_p < DENOISE_TOL, (t, e_O, e_p)
        assert err_x < bound, (t, err_x, bound)


# ------------------------------------------------------------------ 4. fixed entries
def test_residues_not_generated_hold_their_state(bench):
    dims, model = bench
    inp = patches(4, 128, dims, seed=8)
    out = sample(model, inp, seed=2, t_start=20, t_stop=10, trajectory=[20, 15, 11], trajectory_predictions=True,
                 skip_unused_rows=True)
    tr, ctx = out["trajectory"], ~inp["generation_mask"]
    for j in range(3):
        for k, pk in (("translations", "pred_translations"), ("orientations", "pred_orientations")):
            assert torch.equal(tr[k][:, j][ctx], inp[k][ctx]) and torch.equal(tr[pk][:, j][ctx], inp[k][ctx]), (j, k)
        assert torch.equal(tr["seq_idx"][:, j][ctx], inp["seq_idx"][ctx])
        assert torch.equal(tr["seq_probs"][:, j][ctx], torch.nn.functional.one_hot(inp["seq_idx"][ctx], V).float())


@pytest.mark.parametrize("mode", ["fixed_backbone", "structure"])
def test_kept_modality_holds_its_given_values(bench, mode):
    dims, model = bench
    inp = patches(3, 128, dims, seed=9)
    out = sample(model, inp, seed=3, mode=mode, t_start=25, t_stop=18, trajectory=True, trajectory_predictions=True)
    tr, n = out["trajectory"], 7
    rep = lambda v: v.unsqueeze(1).expand(v.shape[0], n, *v.shape[1:])  # noqa: E731
    gm = inp["generation_mask"]
    if mode == "fixed_backbone":
        for k, pk in (("translations", "pred_translations"), ("orientations", "pred_orientations")):
            assert torch.equal(tr[k], rep(inp[k])) and torch.equal(tr[pk], rep(inp[k])), k
        assert not torch.equal(tr["seq_idx"][:, -1][gm], inp["seq_idx"][gm])  # the sequence is diffused
    else:
        assert torch.equal(tr["seq_idx"], rep(inp["seq_idx"]))
        assert torch.equal(tr["seq_probs"], torch.nn.functional.one_hot(rep(inp["seq_idx"]), V).float())
        assert not torch.equal(tr["translations"][:, -1][gm], inp["translations"][gm])


def test_probabilities_of_the_last_step(bench):
    """seq_probs rows sum to 1 within 1e-5, and at label 1 every returned generated token has a nonzero probability."""
    dims, model = bench
    inp = patches(4, 128, dims, seed=10)
    out = sample(model, inp, seed=6, t_start=40, trajectory=[40, 20, 1], trajectory_predictions=True)
    tr, gm = out["trajectory"], inp["generation_mask"]
    assert float((tr["seq_probs"].sum(-1) - 1).abs().max()) < 1e-5
    p1 = tr["seq_probs"][:, slot(tr, 1)]
    drawn = p1.gather(-1, out["seq_idx"].unsqueeze(-1)).squeeze(-1)
    assert bool((drawn[gm] > 0).all())


# ------------------------------------------------------------------ 5. sharding
def test_sharding_num_samples_and_context_index(bench):
    """Rows [lo, hi) run with first_patch = lo give that slice of the whole call's trajectory, bitwise: with num_samples (the shard as
    context_index = arange(lo, hi) // N) and with a general context_index."""
    dims, model = bench
    B, K, N = 4, 128, 3
    inp = patches(B, K, dims, seed=71)
    kw = dict(seed=21, t_start=24, t_stop=14, trajectory=3, trajectory_predictions=True)
    whole = sample(model, inp, num_samples=N, **kw)
    rep = rows(inp, torch.arange(B, device="cuda").repeat_interleave(N))
    for lo, hi in ((0, 5), (5, 12), (3, 9)):
        part = {k: rep[k][lo:hi] for k in STATE}
        part.update({k: inp[k] for k in CTX})
        got = sample(model, part, context_index=torch.arange(lo, hi) // N, first_patch=lo, **kw)
        assert_bitwise(final(got), {k: v[lo:hi] for k, v in final(whole).items()}, (lo, hi))
        want = {k: (v if k == "t" else v[lo:hi]) for k, v in whole["trajectory"].items()}
        assert_bitwise(got["trajectory"], want, ("trajectory", lo, hi))
    ci = torch.tensor([2, 0, 2, 1, 3, 1])
    state = rows(inp, ci.cuda())
    full = {k: state[k] for k in STATE}
    full.update({k: inp[k] for k in CTX})
    whole = sample(model, full, context_index=ci, **kw)
    for lo, hi in ((1, 4), (4, 6)):
        part = {k: full[k][lo:hi] for k in STATE}
        part.update({k: inp[k] for k in CTX})
        got = sample(model, part, context_index=ci[lo:hi], first_patch=lo, **kw)
        want = {k: (v if k == "t" else v[lo:hi]) for k, v in whole["trajectory"].items()}
        assert_bitwise(got["trajectory"], want, ("context_index", lo, hi))


# ------------------------------------------------------------------ 6. the C ABI
def test_c_abi_rejects_bad_records(bench):
    """Each bad record returns DIFFAB_ERR_ARG; the state and the record buffers are untouched afterwards (nothing was enqueued)."""
    dims, model = bench
    lib = _hip.lib()
    P, st = _hip.ptr, _hip.stream_ptr()
    B, K, T, n = 2, 128, model.T, 3
    inp = patches(B, K, dims, seed=13)
    s0, x0, O0 = inp["seq_idx"].clone(), inp["translations"].clone(), inp["orientations"].clone()
    gm = _hip.dev_mask(inp["generation_mask"])
    sd = model._sched_on_device()
    dims_c = model.denoiser.hip_dims(B, K)
    w = model.denoiser.hip_weights()
    rev = model._reverse_so3().struct()
    ws = _hip.workspace(lib.diffab_sample_workspace_bytes(C.byref(dims_c)))
    rc_, pc_ = inp["res_context_emb"], inp["pair_context_emb"]
    slot_dev = torch.full((T + 1,), 77, dtype=torch.int32, device="cuda")
    buf = {"seq": torch.full((B, n, K), 5, dtype=torch.int64, device="cuda"), "x": torch.full((B, n, K, 3), 7.0, device="cuda"),
           "O": torch.full((B, n, K, 3, 3), 7.0, device="cuda"), "pred_x": torch.full((B, n, K, 3), 7.0, device="cuda"),
           "pred_O": torch.full((B, n, K, 3, 3), 7.0, device="cuda"), "seq_probs": torch.full((B, n, K, V), 7.0, device="cuda")}
    before = {k: v.clone() for k, v in buf.items()}
    t_start, t_stop = 10, 5

    def table(entries):
        tab = [-1] * (T + 1)
        for t, j in entries.items():
            tab[t] = j
        return (C.c_int32 * (T + 1))(*tab)

    good = {10: 0, 8: 1, 6: 2}

    def record(n_slots=n, entries=good, drop=(), host=True, dev=True):
        ptrs = {k: (None if k in drop else P(v)) for k, v in buf.items()}
        return _hip.SampleRecord(n_slots, table(entries) if host else None, P(slot_dev) if dev else None,
                                 *(ptrs[k] for k in ("seq", "x", "O", "pred_x", "pred_O", "seq_probs")))

    bad = {"n_slots 0": record(n_slots=0, entries={}), "slot >= n_slots": record(entries={10: 0, 8: 1, 6: 3}),
           "slot < -1": record(entries={10: 0, 8: 1, 6: -2}), "slot used twice": record(entries={10: 0, 8: 1, 6: 1}),
           "slot unused": record(entries={10: 0, 8: 1}), "step past t_start": record(entries={11: 0, 8: 1, 6: 2}),
           "step at t_stop": record(entries={10: 0, 8: 1, 5: 2}), "null seq": record(drop=("seq",)), "null x": record(drop=("x",)),
           "null O": record(drop=("O",)), "partial predictions": record(drop=("seq_probs",)),
           "one prediction": record(drop=("pred_x", "pred_O")), "null host table": record(host=False),
           "null device table": record(dev=False)}
    def loop(rec):
        return lib.diffab_sample_loop_ex(C.byref(dims_c), C.byref(w.struct), C.byref(sd.struct), C.byref(rev), P(s0), P(x0), P(O0), P(rc_),
                                         P(pc_), P(gm), 3, 1, t_start, t_stop, P(ws), ws.numel(), 0,
                                         C.byref(_hip.SampleOptions(n_ctx=B, record=rec)), st)

    for what, rec in bad.items():
        assert loop(rec) == -1, what  # DIFFAB_ERR_ARG
    torch.cuda.synchronize()
    assert torch.equal(s0, inp["seq_idx"]) and torch.equal(x0, inp["translations"]) and torch.equal(O0, inp["orientations"])
    assert_bitwise(buf, before, "record buffers")
    assert bool((slot_dev == 77).all())
    # the good record runs, fills the device table and every slot
    ok = record()
    assert loop(ok) == 0
    torch.cuda.synchronize()
    assert slot_dev[[10, 8, 6]].tolist() == [0, 1, 2] and int((slot_dev == -1).sum()) == T + 1 - 3
    assert bool(torch.isfinite(buf["pred_x"]).all()) and not bool((buf["x"] == 7.0).any())
    assert torch.equal(buf["seq"][:, 0], inp["seq_idx"])  # label t_start: the state the call was given
