"""Particle steering on the MI355X: DiffAb.sample(steering=...), diffab_sample_options.steering and the three teacher-forced entries
diffab_steer_resample, diffab_steer_gather and diffab_steer_energy.

The rule is DESIGN.md section 4.14 / include/diffab_hip.h.  The resampling kernel matches steering.resample_oracle (float64 numpy) on
explicit uniforms; the gather is indexing, cycles included; the energy is the guidance potential at x0_hat; steering that must change
nothing is bitwise the unsteered run on every launch form; one resampling step is the unsteered step indexed by the ancestors; and from
collapsed starts steered designs end with less clash and bond energy than unsteered ones.
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from diffab_pytorch import _hip, synthetic as syn
from diffab_pytorch.guidance import SampleGuidance, structure_energy
from diffab_pytorch.steering import ParticleSteering, c_struct, resample_oracle
from diffab_pytorch.temperature import SampleTemperature
from sampler_support import CTX, assert_bitwise, hip, make_model, patches, rows, sample
from test_guidance_host import guidance_ref, planted_rows

pytestmark = pytest.mark.gpu
F32 = np.float32
patches = functools.partial(patches, chains=True)  # as tests/test_gpu_guidance.py: collapsed generated residues, two chains


@pytest.fixture(scope="module")
def unit(hip):
    dims = dict(syn.UNIT_DIMS, NL=2)
    return dims, make_model(dims, 31)


@pytest.fixture(scope="module")
def bench(hip):
    dims = dict(syn.BENCH_DIMS, NL=2)
    return dims, make_model(dims, 23)


def tabs(inp):
    return dict(chain_idx=inp["chain_idx"], residue_idx=inp["residue_idx"], residue_mask=inp["residue_mask"])


def weighted_energy(x, inp, s: ParticleSteering):
    """fp32 w_clash clash + w_bond bond of diffab_guidance_energy at x (rows, K, 3), the kernel's expression."""
    e = structure_energy(x, inp["generation_mask"], guidance=SampleGuidance(clash=s.clash, bond=s.bond, clash_distance=s.clash_distance,
                                                                            bond_length=s.bond_length), **tabs(inp))
    return F32(s.clash) * e["clash"].cpu().numpy() + F32(s.bond) * e["bond"].cpu().numpy()


# ------------------------------------------------------------------ 1. the resampling kernel against the float64 oracle
PLANTED = 7


def resample_inputs(N, G, seed):
    """G groups of N rows: log-weights drawn wide (sigma = 5), random energies, and in the first groups the planted cases - all equal;
    one -inf; all -inf; one NaN; one row holding all the weight; u = 0; u = the largest float below 1.  Planted groups have energy =
    u_prev, so their log-weights reach the resampling exactly as planted.  `exact`: groups whose cumulative sums are exact in double
    (equal weights, one weight), compared even when a position lies on a boundary."""
    rng = np.random.default_rng(seed)
    lw = rng.normal(0.0, 5.0, (G, N)).astype(F32)
    up = rng.uniform(0.0, 8.0, (G, N)).astype(F32)
    U = rng.uniform(0.0, 8.0, (G, N)).astype(F32)
    u = rng.random(G).astype(F32)
    U[:PLANTED] = up[:PLANTED]
    lw[0] = -1.5
    lw[1, rng.integers(N)] = -np.inf
    lw[2] = -np.inf
    lw[3, rng.integers(N)] = np.nan
    lw[4] = -np.inf
    lw[4, rng.integers(N)] = 2.0
    u[5] = 0.0
    u[6] = np.nextafter(F32(1), F32(0))
    exact = np.zeros(G, bool)
    exact[[0, 4]] = True
    return lw, up, U, u, exact


def run_resample(lib, lw, up, U, u, N, lam, thr):
    G = u.shape[0]
    d = [torch.tensor(v.reshape(-1)).cuda() for v in (lw, up, U, u)]
    anc = torch.full((G * N,), -7, dtype=torch.int32, device="cuda")
    ess = torch.full((G,), -1.0, dtype=torch.float64, device="cuda")
    _hip.check(lib.diffab_steer_resample(_hip.ptr(d[0]), _hip.ptr(d[1]), _hip.ptr(d[2]), _hip.ptr(d[3]), G, N, lam, thr, _hip.ptr(anc),
                                         _hip.ptr(ess), _hip.stream_ptr()), "diffab_steer_resample")
    return {"logw": d[0].cpu().numpy(), "u_prev": d[1].cpu().numpy(), "ancestors": anc.cpu().numpy(), "ess": ess.cpu().numpy()}


@pytest.mark.parametrize("N", [1, 2, 3, 64, 65, 257, 1024])
def test_resample_kernel_against_the_oracle(hip, N):
    """Groups in which a position (u + j) / N lies within 1e-12 of a cumulative boundary may differ legitimately and are left out, at
    most 2 % of them (for these seeds the oracle leaves out none of the 64 groups at any N and either threshold - checked on the CPU)."""
    G, lam = 64, 0.75
    lw, up, U, u, exact = resample_inputs(N, G, seed=1000 + N)
    for thr in (2.0, 0.5):
        ref = resample_oracle(lw, up, U, u, N, lam, thr)
        got = run_resample(hip, lw, up, U, u, N, lam, thr)
        live = ref["ess"] > 0
        err = np.abs(got["ess"] - ref["ess"])[live] / ref["ess"][live]
        print(f"\nN = {N}, threshold {thr}: ESS max rel err {err.max() if err.size else 0.0:.2e}, resampled {int(ref['resampled'].sum())} / {G}, "
              f"smallest margin {ref['margin'][~exact].min():.2e}")
        assert (err <= 1e-12).all(), err.max()
        assert np.array_equal(got["ess"][~live], ref["ess"][~live])
        keep = (ref["margin"] >= 1e-12) | exact
        assert (~keep).sum() <= 0.02 * G, (~keep).sum()
        sel = np.repeat(keep, N)
        assert np.array_equal(got["ancestors"][sel], ref["ancestors"][sel])
        for k in ("logw", "u_prev"):
            assert np.array_equal(got[k][sel], ref[k][sel], equal_nan=True), k
        if thr == 2.0 and N > 1:
            a = got["ancestors"].reshape(G, N)
            assert a[2].tolist() == list(range(N)) and not got["logw"].reshape(G, N)[2].any(), "a group without weight stays, logw = 0"
            assert len(set(a[4])) == 1 and np.isfinite(lw[4, a[4, 0]]), "one row holds all the weight"
            assert (np.diff(a, axis=1) >= 0).all()


def test_resample_result_does_not_depend_on_the_launch(hip):
    N, G = 65, 64
    lw, up, U, u, _ = resample_inputs(N, G, seed=5)
    whole = run_resample(hip, lw, up, U, u, N, 0.75, 2.0)
    part = run_resample(hip, lw[10:13], up[10:13], U[10:13], u[10:13], N, 0.75, 2.0)
    for k in whole:
        per = N if k != "ess" else 1
        assert np.array_equal(part[k], whole[k][10 * per:13 * per], equal_nan=True), k


# ------------------------------------------------------------------ 2. the gather kernel
@pytest.mark.parametrize("K", [5, 64, 130])
def test_gather_is_indexing(hip, K):
    R = 12
    g = torch.Generator().manual_seed(K)
    seq = torch.randint(0, 21, (R, K), generator=g)
    x, O = torch.randn(R, K, 3, generator=g), torch.randn(R, K, 3, 3, generator=g)
    gm = torch.rand(R, K, generator=g) < 0.6  # ragged, a different mask on every row
    gm[1] = False
    maps = {"cycle": (torch.arange(R) + 1) % R, "two cycles": torch.tensor([1, 2, 0, 4, 5, 3, 6, 7, 9, 8, 11, 10]),
            "random": torch.randint(0, R, (R,), generator=g), "one ancestor": torch.full((R,), 7), "identity": torch.arange(R)}
    for name, a in maps.items():
        d = [v.clone().cuda() for v in (seq, x, O)]
        scratch = torch.empty(R * K * 56, dtype=torch.uint8, device="cuda")
        gm_d, a_d = gm.cuda(), a.to(torch.int32).cuda()
        _hip.check(hip.diffab_steer_gather(_hip.ptr(d[0]), _hip.ptr(d[1]), _hip.ptr(d[2]), _hip.ptr(gm_d), _hip.ptr(a_d), R, K,
                                           _hip.ptr(scratch), _hip.stream_ptr()), "diffab_steer_gather")
        for got, old in zip(d, (seq, x, O)):
            m = gm.reshape(R, K, *([1] * (old.dim() - 2)))
            assert torch.equal(got.cpu(), torch.where(m, old[a], old)), (name, tuple(old.shape))


# ------------------------------------------------------------------ 3. the energy kernel
@pytest.mark.parametrize("K", [5, 64, 130])
def test_energy_against_float64_at_x0_hat(hip, unit, K):
    _, model = unit
    B, t = 3, 30
    p, gen, chain, ridx, rmask = planted_rows(B, K, seed=K, n_chains=2)
    rng = np.random.default_rng(K)
    sched = {k: v.cpu().numpy() for k, v in model.sched.items()}
    a, om = sched["alpha_bar_sqrt"][t].astype(np.float64), sched["one_minus_alpha_bar_sqrt"][t].astype(np.float64)
    eps = rng.normal(0.0, 1.0, (B, K, 3)).astype(F32)
    x = (p * a + om * eps).astype(F32)  # so that x0_hat is the planted structure, up to fp32
    x0 = np.where(gen[..., None], (x.astype(np.float64) - om * eps) / a, x.astype(np.float64))
    s = ParticleSteering(clash=1.3, bond=0.7, clash_distance=4.0, bond_length=3.8)
    ref = guidance_ref(x0, gen, chain, ridx, rmask, 1.3, 4.0, 0.7, 3.8)
    want = 1.3 * ref["clash"] + 0.7 * ref["bond"]
    dev = [torch.tensor(v).cuda() for v in (chain, ridx, rmask)]
    ss = c_struct(s, 0, 1, dev[0], dev[1], dev[2], None, None, None, None, None)
    out = torch.full((B,), -1.0, device="cuda")
    sd = model._sched_on_device()
    x_d, eps_d, gen_d = (torch.tensor(v).cuda() for v in (x, eps, gen))
    _hip.check(hip.diffab_steer_energy(_hip.ptr(x_d), _hip.ptr(eps_d), _hip.ptr(gen_d), C.byref(sd.struct), t, C.byref(ss), B, K, _hip.ptr(out),
                                       _hip.stream_ptr()), "diffab_steer_energy")
    got = out.cpu().double().numpy()
    print(f"\nK = {K}: U {got}, float64 {want}")
    assert (want > 0).any()
    # (the tolerance of tests/test_gpu_guidance.py::test_energy_against_float64 for diffab_guidance_energy)
    assert np.abs(got - want).max() <= 1e-5 * np.abs(want).max() + 1e-5, (got, want)


@pytest.mark.parametrize("K", [64, 130])
def test_energy_is_bitwise_the_guidance_energy_at_the_recorded_prediction(unit, K):
    """One steering step, never resampling: log_weight = -(strength U) exactly, U = w_clash clash + w_bond bond of diffab_guidance_energy
    at the recorded pred_translations (the context residues hold their given coordinates there)."""
    dims, model = unit
    inp = patches(2, K, dims, seed=K)
    s = ParticleSteering(strength=0.5, clash=1.3, bond=0.7, ess_threshold=0.0, t_min=30, t_max=30)
    out = sample(model, inp, seed=3, t_start=30, t_stop=28, init=False, num_samples=2, steering=s, trajectory=True, trajectory_predictions=True)
    rep = rows(inp, torch.arange(2, device="cuda").repeat_interleave(2))
    U = weighted_energy(out["trajectory"]["pred_translations"][:, 0], rep, s)
    assert (U > 0).all()
    assert out["steering"]["t"].tolist() == [30]
    assert np.array_equal(out["steering"]["energy"].cpu().numpy(), U)
    assert np.array_equal(out["steering"]["log_weight"].cpu().numpy(), -(F32(0.5) * U))


# ------------------------------------------------------------------ 4. steering that must change nothing, bitwise
FORMS = {"per_layer": dict(flags=_hip.FLAG_MULTI_LAUNCH), "module": dict(flags=_hip.FLAG_PERSISTENT_MODULE), "graph": dict(graph=True)}
STATE_KEYS = ("seq_idx", "translations", "orientations")


def states(out):
    return {k: out[k] for k in STATE_KEYS}


def steer_out(out):
    """samples["steering"] on the host (the entries come back on the inputs' device)."""
    return {k: v.cpu() for k, v in out["steering"].items()}


@pytest.mark.parametrize("form", sorted(FORMS))
def test_zero_strength_is_bitwise_unsteered(bench, form):
    dims, model = bench
    inp = patches(2, 128, dims, seed=3)
    base = dict(seed=4, t_start=12, t_stop=0, init=False, num_samples=2, **FORMS[form])
    extra = dict(steps=6, guidance=SampleGuidance(clash=2.0, bond=1.0, max_shift=0.5),
                 temperature=SampleTemperature(translation=0.8, rotation=0.5, sequence=0.7))
    for kw in (base, dict(base, **extra)):
        plain = sample(model, inp, **kw)
        out = sample(model, inp, steering=ParticleSteering(strength=0.0, ess_threshold=1.0), **kw)
        assert_bitwise(states(out), plain, (form, sorted(kw)))
        st = steer_out(out)
        assert not st["log_weight"].any() and (st["energy"] > 0).all()
        assert torch.equal(st["ancestors"], torch.arange(4).expand(st["t"].numel(), 4)) and st["lineage"].tolist() == [0, 1, 2, 3]


@pytest.mark.parametrize("K", [64, 130])
def test_threshold_zero_keeps_the_states_and_weights_telescope(unit, K):
    dims, model = unit
    N, lam = 3, 0.25
    inp = patches(2, K, dims, seed=7)
    kw = dict(seed=5, t_start=9, t_stop=0, init=False, num_samples=N, trajectory=True, trajectory_predictions=True)
    plain = sample(model, inp, **kw)
    s = ParticleSteering(strength=lam, ess_threshold=0.0, every=2)
    out = sample(model, inp, steering=s, **kw)
    st = steer_out(out)
    del out["steering"]
    assert_bitwise(out, plain, "ess_threshold = 0")
    assert st["t"].tolist() == [9, 7, 5, 3]
    rep = rows(inp, torch.arange(2, device="cuda").repeat_interleave(N))
    label = out["trajectory"]["t"].tolist()
    lw, up, umax = np.zeros(2 * N, F32), np.zeros(2 * N, F32), 0.0
    for t in st["t"].tolist():  # the rule's fp32 recurrence over the recorded predictions
        U = weighted_energy(out["trajectory"]["pred_translations"][:, label.index(t)], rep, s)
        lw, up, umax = lw + (-(F32(lam) * (U - up))), U, max(umax, float(U.max()))
    assert np.array_equal(st["energy"].cpu().numpy(), up)
    assert np.array_equal(st["log_weight"].cpu().numpy(), lw)
    # log_weight = -strength energy up to the fp32 rounding of the telescoping sum: three roundings per step, each at most 2^-24 of a
    # magnitude below 2 strength U_max
    bound = len(st["t"]) * 3 * 2.0 ** -24 * 2 * lam * umax
    assert np.abs(lw.astype(np.float64) + lam * up.astype(np.float64)).max() <= bound
    assert torch.equal(st["ancestors"], torch.arange(2 * N).expand(4, 2 * N))


@pytest.mark.parametrize("K", [5, 64])
def test_groups_of_one_are_bitwise_unsteered(unit, K):
    dims, model = unit
    inp = patches(3, K, dims, seed=9)
    kw = dict(seed=6, t_start=8, t_stop=0, init=False)
    out = sample(model, inp, steering=ParticleSteering(strength=3.0, ess_threshold=2.0), **kw)
    st = steer_out(out)
    del out["steering"]
    assert_bitwise(out, sample(model, inp, **kw), "N = 1")
    assert st["lineage"].tolist() == [0, 1, 2] and (st["log_weight"] == 0).all()


def test_shards_of_whole_groups_are_slices_of_the_whole_call(unit):
    dims, model = unit
    B, N, K = 3, 4, 64
    inp = patches(B, K, dims, seed=13)
    s = ParticleSteering(strength=0.05, ess_threshold=0.9)
    kw = dict(seed=8, t_start=10, t_stop=0, init=False, steering=s)
    whole = sample(model, inp, num_samples=N, **kw)
    ws = steer_out(whole)
    assert (ws["ancestors"] != torch.arange(B * N)).any(), "some group must resample for this test to say anything"
    ci = torch.arange(B * N) // N
    for lo, hi in ((0, N), (N, B * N)):
        part_rows = rows({k: v for k, v in inp.items() if k not in CTX}, ci[lo:hi].cuda())
        part = sample(model, dict(part_rows, res_context_emb=inp["res_context_emb"], pair_context_emb=inp["pair_context_emb"]),
                      context_index=ci[lo:hi], first_patch=lo, **dict(kw, steering=ParticleSteering(strength=0.05, ess_threshold=0.9, group_size=N)))
        assert_bitwise(states(part), {k: whole[k][lo:hi] for k in STATE_KEYS}, ("shard", lo))
        ps = steer_out(part)
        assert torch.equal(ps["t"], ws["t"])
        for k in ("log_weight", "energy"):
            assert torch.equal(ps[k], ws[k][lo:hi]), k
        assert torch.equal(ps["ancestors"] + lo, ws["ancestors"][:, lo:hi]) and torch.equal(ps["lineage"] + lo, ws["lineage"][lo:hi])


# ------------------------------------------------------------------ 5. one resampling step is the unsteered step, indexed by the ancestors
@pytest.mark.parametrize("K, form", [(64, {}), (130, {}), (64, dict(graph=True, steps=[10, 9, 8, 7, 6, 4, 2]))])
def test_one_resampling_step_is_the_rule(unit, K, form):
    dims, model = unit
    B, N, ts = 2, 6, 7
    inp = patches(B, K, dims, seed=17)
    kw = dict(seed=11, t_start=10, t_stop=0, init=False, num_samples=N, trajectory=True, **form)
    a = sample(model, inp, steering=ParticleSteering(strength=0.2, ess_threshold=2.0, t_min=ts, t_max=10), **kw)
    b = sample(model, inp, steering=ParticleSteering(strength=0.2, ess_threshold=2.0, t_min=ts + 1, t_max=10), **kw)
    sa, sb = steer_out(a), steer_out(b)
    assert sa["t"].tolist() == [10, 9, 8, 7] and sb["t"].tolist() == [10, 9, 8]
    assert torch.equal(sa["ancestors"][:3], sb["ancestors"])
    anc = sa["ancestors"][3].cuda()
    assert (anc // N == torch.arange(B * N, device="cuda") // N).all(), "ancestors stay inside the group"
    assert len(set(anc.tolist())) < B * N, "some rows must share an ancestor for this test to say anything"
    label = a["trajectory"]["t"].tolist()
    j, j2 = label.index(6), label.index(6) + 1
    gm = inp["generation_mask"].repeat_interleave(N, dim=0)
    for k in STATE_KEYS:
        ta, tb = a["trajectory"][k], b["trajectory"][k]
        assert torch.equal(ta[:, :j], tb[:, :j]), (k, "identical up to and including the record of step t*")
        assert torch.equal(ta[:, j][gm], tb[:, j][anc][gm]), (k, "the gathered state is B's, indexed by the ancestors")
        assert torch.equal(ta[:, j][~gm], tb[:, j][~gm]), k
    twins = [(r, q) for r in range(B * N) for q in range(r + 1, B * N) if anc[r] == anc[q]]
    xa = a["trajectory"]["translations"]
    for r, q in twins:
        assert torch.equal(xa[r, j][gm[r]], xa[q, j][gm[q]]), "children of one ancestor are equal after the step"
        assert not torch.equal(xa[r, j2][gm[r]], xa[q, j2][gm[q]]), "and separate at the next one (their noise is keyed by the row)"


# ------------------------------------------------------------------ 6. what steering does
def test_steering_lowers_the_final_energy_from_collapsed_starts(unit):
    """Generated residues collapsed onto one point (the starts of profiles/guidance.md), forward-noised to t = 20 (optimize_from), 2
    patches of N = 64 designs, same seed with and without steering.  The mean clash + bond energy (weights 1) of the finished designs
    must be lower with steering: a strict inequality on a deterministic pair of runs.  A statement about the potential, not about design
    quality (the weights are untrained)."""
    dims, model = unit
    B, N, K = 2, 64, 64
    inp = patches(B, K, dims, seed=29)
    kw = dict(seed=12, optimize_from=20, num_samples=N)
    s = ParticleSteering(strength=5.0, ess_threshold=0.5)
    plain = sample(model, inp, **kw)
    steered = sample(model, inp, steering=s, **kw)
    rep = rows(inp, torch.arange(B, device="cuda").repeat_interleave(N))
    e0, e1 = (weighted_energy(o["translations"], rep, ParticleSteering()).astype(np.float64).mean() for o in (plain, steered))
    st = steer_out(steered)
    n_res = int((st["ancestors"] != torch.arange(B * N)).any(1).sum())
    print(f"\nsteering effect: mean clash + bond energy {e0:.2f} -> {e1:.2f} ({e1 / e0:.3f}); {n_res} of {st['t'].numel()} steering steps "
          f"resampled, {len(set(st['lineage'].tolist()))} of {B * N} initial rows survive")
    assert n_res > 0
    assert e1 < e0


# ------------------------------------------------------------------ 7. design_complex passes steering through
def test_design_complex_with_steering_is_the_calls_by_hand(hip):
    import test_gpu_patch as tp

    model = tp.make_model(dict(syn.BENCH_DIMS, NL=2), 9)
    batch = tp.complexes()
    kw = dict(seed=31, num_samples=4, t_start=12, t_stop=5, steering=ParticleSteering(strength=1.0, ess_threshold=2.0))
    out = model.design_complex(batch, **kw)
    sel, _, res = tp.by_hand(model, batch, **kw)
    for name in STATE_KEYS:
        assert torch.equal(out[name], res[name]), name
    for k, v in res["steering"].items():
        assert torch.equal(out["steering"][k], v), k
    st = steer_out(out)
    assert st["t"].tolist() == [12, 11, 10, 9, 8, 7] and (st["ancestors"] != torch.arange(8)).any()
    assert (st["ancestors"] // 4 == torch.arange(8) // 4).all()
    plain = model.design_complex(batch, **{k: v for k, v in kw.items() if k != "steering"})
    native = {"seq_idx": batch["seq_idx"], "translations": batch["xyz"][:, :, 1], "orientations": batch["orientations"]}
    for r in range(8):  # the pasted complex: the native outside the generated residues, the steered design inside
        c = r // 4
        gen = batch["generation_mask"][c] & batch["residue_mask"][c]
        slot = {int(i): p for p, i in enumerate(sel.index[c].tolist()) if i >= 0}
        where = torch.tensor([slot[int(i)] for i in torch.nonzero(gen).flatten()])
        for name in STATE_KEYS:
            full = out["complex"][name][r].cpu()
            assert torch.equal(full[~gen], native[name][c][~gen]), name
            assert torch.equal(full[gen], out[name][r].cpu()[where]), name
    assert not torch.equal(out["translations"], plain["translations"])


# ------------------------------------------------------------------ 8. the C ABI refuses a bad struct before anything is enqueued
@pytest.mark.parametrize("field, value, match", [
    ("group_size", 3, "4 rows are not a multiple of the steering group_size = 3"), ("group_size", 0, "group_size = 0 outside"),
    ("group_size", 2048, "group_size = 2048 outside"), ("strength", -1.0, "strength = -1 must be finite"),
    ("strength", float("inf"), "strength"), ("w_clash", -1.0, "weights must be finite"), ("w_bond", float("nan"), "weights must be finite"),
    ("clash_distance", 0.0, "clash_distance and bond_length"), ("bond_length", -3.8, "clash_distance and bond_length"),
    ("ess_threshold", 2.5, "ess_threshold = 2.5 outside"), ("ess_threshold", -0.5, "ess_threshold"), ("t_min", 9, "t_min <= t_max"),
    ("t_min", -1, "t_min <= t_max"), ("t_max", 101, "t_min <= t_max"), ("every", 0, "every = 0 < 1"), ("logw", None, "needs logw"),
    ("u_prev", None, "needs logw"), ("energy", None, "needs logw"), ("scratch", None, "needs logw"), ("chain", None, "chain and residue_idx"),
    ("residue_idx", None, "chain and residue_idx"),
])
def test_the_entry_refuses_a_bad_struct(unit, monkeypatch, field, value, match):
    from diffab_pytorch import steering as steering_mod

    dims, model = unit
    inp = patches(2, 64, dims, seed=3)
    good = steering_mod.c_struct

    def bad(*a, **k):
        ss = good(*a, **k)
        setattr(ss, field, value)
        return ss

    monkeypatch.setattr(steering_mod, "c_struct", bad)
    before = {k: inp[k].clone() for k in STATE_KEYS}
    with pytest.raises(_hip.DiffabHipError, match=match):
        sample(model, inp, seed=1, t_start=8, init=False, num_samples=2, steering=ParticleSteering(t_max=8))
    torch.cuda.synchronize()
    assert all(torch.equal(inp[k], before[k]) for k in STATE_KEYS)


def test_the_entry_refuses_steering_with_a_kept_structure(unit, hip):
    """DIFFAB_FLAG_KEEP_STRUCTURE with a steering struct: DIFFAB_ERR_ARG from the library itself (Python refuses mode='fixed_backbone'
    earlier, so the flag is passed by hand)."""
    dims, model = unit
    inp = patches(2, 64, dims, seed=3)
    with pytest.raises(_hip.DiffabHipError, match="DIFFAB_FLAG_KEEP_STRUCTURE does not sample"):
        sample(model, inp, seed=1, t_start=8, init=False, num_samples=2, steering=ParticleSteering(), flags=_hip.FLAG_KEEP_STRUCTURE)
