"""One reverse step on the MI355X with the sampler's options on together - a jump (steps=), per-row noise scales and sequence
temperature, a per-residue allowed_aa mask and structure guidance in one call, and particle steering on top - against
tests/reverse_step_ref.py, the float64 composition that tests/test_reverse_step_composed_host.py pins on the CPU first.

Every step is teacher-forced: sample(init=False, t_start=t, t_stop=s, steps=[t]) with the record on, so the model's predictions are
read from the record and the denoiser is never re-evaluated on the host.  Translations are compared by difference with a run that has
only the jump on (the mean, and with it eps_hat, cancels).  The angle is checked against a table built alone over lambda sqrt(beta'_t),
not against the model's stack: a wrong rot_row, a stack over the wrong beta or a stale cache entry fails.

A case is one geometry over the four steps (57 -> 20 a jump with noise, 30 -> 29 a stride-1 step inside a plan, 8 -> 0 a jump to 0,
2 -> 1 the last noisy step); the generation masks are the test's own (two unaligned segments, 24 residues per row; at K = 5 four of the
five residues), so a case has 4 x 96 draws (4 x 16 at K = 5, the only geometry with fewer than 50 per step).  The rotation scales
lambda_a < lambda_b are taken from the schedule so that scaled rows fall on both sides of the 0.1 threshold: sigma < 0.1 draws from
the histogram's inverse CDF, sigma >= 0.1 by the Gaussian rule (csrc igso3_theta, reference so3.py:118-125).

The allowed_aa masks hold one generated residue with no allowed class.  The update kernel leaves such a residue's token as it is
 and DiffAb.sample refuses the mask before device work, so these tests switch that one host check off
(`empty_set_reaches_the_kernel`) and change nothing else of the front end.
"""
import numpy as np
import pytest
import torch

import diffab_oracle as orc
from diffab_pytorch import _hip, so3 as _so3, synthetic as syn
from diffab_pytorch.diffusion import jump_coefficients
from diffab_pytorch.guidance import SampleGuidance
from diffab_pytorch.steering import ParticleSteering, resample_oracle
from diffab_pytorch.temperature import SampleTemperature
from reverse_step_ref import STREAM_STEER, reverse_step_ref
from sampler_support import PATCH_LENGTH_DIMS, add_chains, assert_bitwise, hip, make_model, n_real_of, padded, patches, sample
from test_gpu_temperature import rotation_of
from test_guidance_host import guidance_ref

pytestmark = pytest.mark.gpu
V, B, SEED, FIRST = 21, 4, 23, 3
F32 = np.float32
STEPS = [(57, 20), (30, 29), (8, 0), (2, 1)]
GUIDE = SampleGuidance(clash=2.0, bond=1.0, max_shift=0.5)
LX = [1.5, 0.0, 1.0, 0.5]
TAU = [0.5, 1.0, 0.0, 2.0]
MODULE, PER_LAYER = _hip.FLAG_PERSISTENT_MODULE, _hip.FLAG_MULTI_LAUNCH
GEOMETRIES = {  # name: (dims, K, launch forms; the first is compared with the reference, the others with the first, bitwise)
    "unit_k5": ("unit", 5, {"any_dims": {}}),
    "unit_k130": ("unit", 130, {"any_dims": {}}),
    "bench_k64": ("bench", 64, {"default": {}}),
    "bench_k128": ("bench", 128, {"per_layer": dict(flags=PER_LAYER), "module": dict(flags=MODULE), "graph": dict(graph=True)}),
    "bench_k173_padded": ("bench", 173, {"default": {}}),
    "bench_k256": ("bench", 256, {"default": {}, "module": dict(flags=MODULE)}),
}


@pytest.fixture(scope="module")
def models(hip):
    return {"unit": (dict(syn.UNIT_DIMS, NL=2), make_model(dict(syn.UNIT_DIMS, NL=2), 31)),
            "bench": (dict(PATCH_LENGTH_DIMS), make_model(dict(PATCH_LENGTH_DIMS), 23))}


@pytest.fixture(scope="module")
def steered_models(hip):
    """Models of their own: the steered runs use one more (scales, step list) key, and a model's cache holds four."""
    return {"unit": (dict(syn.UNIT_DIMS, NL=2), make_model(dict(syn.UNIT_DIMS, NL=2), 37)),
            "bench": (dict(PATCH_LENGTH_DIMS), make_model(dict(PATCH_LENGTH_DIMS), 29))}


@pytest.fixture()
def empty_set_reaches_the_kernel(monkeypatch):
    from diffab_pytorch import diffab_pytorch as front_end

    monkeypatch.setattr(front_end, "_allowed_aa_host", lambda *a, **k: None)


def rotation_scales(model):
    """(lambda_a, lambda_b) from the model's own schedule: with s_max the largest sqrt(beta') of the four steps, lambda_a s_max = 0.05
    (the histogram at every step) and lambda_b s_max = 0.2 (the Gaussian rule at the widest step, the histogram at the narrowest)."""
    sig = [float(jump_coefficients(model.sched, torch.tensor([t]), s, model.beta_max)[0][t].sqrt()) for t, s in STEPS]
    la, lb = round(0.05 / max(sig), 3), round(0.2 / max(sig), 3)
    assert 0 < la < lb < 1 and lb * max(sig) >= 0.1 > lb * min(sig) and la * max(sig) < 0.1
    return la, lb


def generation_mask(rows, K):
    gm = torch.zeros(rows, K, dtype=torch.bool)
    for b in range(rows):
        if K < 64:
            gm[b] = True
            gm[b, b % K] = False
        else:  # two segments that start and end inside 16-row tiles, different on every row
            gm[b, 3 + b:16 + b] = True
            gm[b, K // 2 + 5 + 2 * b:K // 2 + 16 + 2 * b] = True
    return gm


def allowed_mask(gm, seed):
    """Random (rows, K, V) mask; of each row's generated residues the first allows one class only, and the second of row 0 none."""
    rows, K = gm.shape
    al = torch.rand(rows, K, V, generator=torch.Generator().manual_seed(seed)) < 0.5
    al[..., 2] = True
    none = None
    for b in range(rows):
        gen = torch.nonzero(gm[b]).flatten().tolist()
        al[b, gen[0]] = torch.arange(V) == 5 + b
        if b == 0:
            none = (0, gen[1])
            al[none] = False
    return al, none


def inputs(name, dims, K, rows=B, gm=None):
    gm = generation_mask(rows, K) if gm is None else gm
    if "padded" in name:  # patch 0 real for its first n_real residues only (the generated segments lie inside them)
        inp = {k: v.cuda() for k, v in padded(rows, K, n_real_of(K), seed=K, dims=dims).items()}
        real = inp["residue_mask"].clone()
        assert bool((real.cpu() | ~gm).all())
        inp["generation_mask"] = gm.cuda()
        add_chains(inp, seed=K)
        inp["residue_mask"] &= real
        return inp
    return patches(rows, K, dims, seed=K, chains=True, generation_mask=gm)


def temperature(rows, la, lb):
    rep = lambda v: torch.tensor((v * rows)[:rows], dtype=torch.float32)
    return rep(LX), rep([0.0, la, lb, 1.0]), rep(TAU)


def table_rows(sigma_of_scale):
    """{lambda: CDF row} of tables built alone, one sigma each, for the scales whose sigma is below the threshold."""
    out = {}
    for lam, sg in sigma_of_scale.items():
        if float(sg) < 0.1:
            alone = _so3.SO3(sg.reshape(1), sigma_threshold=0.1, n_bins=8192, num_iters=1024, without_replacement=False)
            out[lam] = alone._cdf[0].cpu()
    return out


def reference(model, inp, rec, t, s, temp, allowed, rows_gm, slot=0, **kw):
    """reverse_step_ref on the recorded predictions of label t (in `slot`) and on tables built alone."""
    bj, aj = (float(v[t]) for v in jump_coefficients(model.sched, torch.tensor([t]), s, model.beta_max))
    lx, lo, tau = temp
    sb = torch.tensor(bj, dtype=torch.float32).sqrt()
    scales = {float(v) for v in lo.tolist() if v != 0.0}
    cdf = table_rows({lam: sb * torch.tensor(lam, dtype=torch.float32) for lam in scales}) if s > 0 else {}
    tables = tuple(inp[k].cpu().numpy() for k in ("chain_idx", "residue_idx", "residue_mask"))
    return reverse_step_ref(t, s, inp["seq_idx"].cpu().numpy(), rec["pred_translations"][:, slot].cpu().numpy(),
                            rec["pred_orientations"][:, slot].cpu().numpy(), rec["seq_probs"][:, slot].cpu().numpy(), rows_gm, model.sched, bj, aj,
                            SEED, FIRST, trans_scale=lx.numpy(), rot_scale=lo.numpy(), seq_temp=tau.numpy(), rot_cdf=cdf,
                            allowed=allowed.numpy(), guidance=GUIDE, tables=tables, **kw)


# ------------------------------------------------------------------ 1. every option at once, per row, on every launch path
@pytest.mark.parametrize("name", sorted(GEOMETRIES))
def test_all_options_in_one_step_are_the_float64_composition(models, empty_set_reaches_the_kernel, name):
    which, K, forms = GEOMETRIES[name]
    dims, model = models[which]
    la, lb = rotation_scales(model)
    inp = inputs(name, dims, K)
    gm_d = inp["generation_mask"]
    gm = gm_d.cpu().numpy()
    allowed, none = allowed_mask(gm_d.cpu(), seed=K)
    temp = temperature(B, la, lb)
    lx, lo, tau = temp
    n_draws = n_excused = 0
    branches = set()
    for t, s in STEPS:
        kw = dict(seed=SEED, first_patch=FIRST, t_start=t, t_stop=s, steps=[t], init=False, trajectory=True, trajectory_predictions=True)
        on = dict(temperature=SampleTemperature(*temp), allowed_aa=allowed, guidance=GUIDE)
        jump = sample(model, inp, **kw)  # the options-off step: the jump alone, lambda = 1 on every row
        outs = {form: sample(model, inp, **kw, **on, **extra) for form, extra in forms.items()}
        first = next(iter(outs))
        out = outs[first]
        for form, other in outs.items():
            assert_bitwise(other, out, (name, t, form, "against", first))
        # ---- record: the model's own outputs, whatever the options
        assert_bitwise(out["trajectory"], jump["trajectory"], (name, t, "record"))
        ref = reference(model, inp, out["trajectory"], t, s, temp, allowed, gm)
        # ---- sequence
        got = out["seq_idx"].cpu().numpy()
        drawn = ref["drawn"]
        assert np.array_equal(got[~drawn], inp["seq_idx"].cpu().numpy()[~drawn]), (name, t, "no draw: the token stays")
        assert not drawn[none] and gm[none]
        assert np.take_along_axis(allowed.numpy(), got[..., None], -1)[..., 0][drawn].all(), (name, t, "an excluded class was drawn")
        differ = drawn & (got != ref["seq"])
        assert (ref["edge"][differ] < 1e-5).all(), (name, t, np.argwhere(differ).tolist(), ref["edge"][differ])
        n_draws, n_excused = n_draws + int(drawn.sum()), n_excused + int(differ.sum())
        # ---- translations: the difference to the jump alone
        xa, xj = out["translations"].cpu().double().numpy(), jump["translations"].cpu().double().numpy()
        assert np.abs(ref["delta"][gm]).max() > 1e-3, "the state must clash for this case to say anything"
        err_x = np.abs((xa - xj) - ref["dx"]).max()
        bar_x = 1e-5 * max(1.0, np.abs(xj).max())
        assert torch.equal(out["translations"][~gm_d], inp["translations"][~gm_d])
        other_seed = sample(model, inp, **dict(kw, seed=SEED + 1), **on, **forms[first])  # no noise term: the seed cannot matter
        quiet = torch.ones(B, dtype=torch.bool) if s == 0 else lx == 0
        assert torch.equal(other_seed["translations"][quiet.cuda()], out["translations"][quiet.cuda()]), (name, t, "noise at s = 0 / lambda_x = 0")
        assert s == 0 or not torch.equal(other_seed["translations"][~quiet.cuda()], out["translations"][~quiet.cuda()])
        # ---- orientations
        O0 = out["trajectory"]["pred_orientations"][:, 0]
        still = torch.ones(B, dtype=torch.bool) if s == 0 else lo == 0
        m_still = gm_d & still.cuda()[:, None]
        assert torch.equal(out["orientations"][m_still], O0[m_still]), (name, t, "lambda_O = 0 / s = 0: O0_hat exactly")
        assert torch.equal(out["orientations"][~gm_d], inp["orientations"][~gm_d])
        err_th = err_ax = 0.0
        if s > 0:
            m = gm_d & ~still.cuda()[:, None]
            th, ax = rotation_of(O0[m].cpu(), out["orientations"][m].cpu())
            th1, ax1 = rotation_of(O0[m].cpu(), jump["orientations"][m].cpu())
            err_th = float((th - torch.from_numpy(ref["theta"])[m.cpu()]).abs().max())
            big = (th > 0.02) & (th1 > 0.02)
            err_ax = float((ax[big] - ax1[big]).abs().max())
            assert int(big.sum()) > 0
            for b in range(B):
                if lo[b] not in (0.0, 1.0):
                    branches.add((t, s, round(float(lo[b]), 3), "histogram" if ref["hist"][b] else "gaussian"))
        print(f"\n{name} {t} -> {s}: translation error {err_x:.2e} (bar {bar_x:.2e}), angle error {err_th:.2e}, axis error {err_ax:.2e}, "
              f"{int(differ.sum())} of {int(drawn.sum())} draws excused, sigma per row {np.round(ref['sigma'], 4).tolist()}")
        assert err_x <= bar_x, (name, t, err_x)
        assert err_th < 1e-5 and err_ax < 1e-4, (name, t, err_th, err_ax)
    print(f"{name}: {n_excused} of {n_draws} draws excused; scaled rows: {sorted(branches)}")
    assert n_draws >= 50 and n_excused <= 2, (name, n_draws, n_excused)
    assert {b[3] for b in branches} == {"histogram", "gaussian"}, branches


# ------------------------------------------------------------------ 2. steering on top
@pytest.mark.parametrize("which, K, N, extra", [("unit", 64, 2, {}), ("unit", 64, 5, {}), ("unit", 130, 2, {}), ("unit", 130, 5, {}),
                                                ("bench", 128, 2, dict(flags=MODULE)), ("bench", 128, 5, dict(flags=MODULE))])
def test_a_steering_step_with_every_option_on(steered_models, empty_set_reaches_the_kernel, which, K, N, extra):
    """Four executed steps, 60 -> 59 -> 57 -> 20 -> 19: the first two let the designs of a patch drift apart (they start as copies, and
    copies weigh the same), step 57 alone steers and always resamples, and the record's slot of label 20 is the state after the update of
    step 57 and the gather."""
    dims, model = steered_models[which]
    la, lb = rotation_scales(model)
    P, t, s, lam, j = 2, 57, 20, 0.02, 2
    rows = P * N
    inp = inputs(f"steer_{which}", dims, K, rows=P, gm=generation_mask(1, K).expand(P, K).clone())
    allowed, _ = allowed_mask(inp["generation_mask"].cpu(), seed=K + N)
    temp = temperature(rows, la, lb)
    kw = dict(seed=SEED, first_patch=FIRST, t_start=60, t_stop=s - 1, steps=[60, 59, t, s], init=False, num_samples=N, trajectory=True,
              trajectory_predictions=True, temperature=SampleTemperature(*temp), allowed_aa=allowed, guidance=GUIDE, **extra)
    steer = dict(strength=lam, clash=1.3, bond=0.7, t_min=t, t_max=t)
    plain = sample(model, inp, **kw)
    a = sample(model, inp, steering=ParticleSteering(ess_threshold=2.0, **steer), **kw)
    c = sample(model, inp, steering=ParticleSteering(ess_threshold=0.0, **steer), **kw)  # never resamples: the weights of every row
    assert a["steering"]["t"].tolist() == [t] and c["steering"]["t"].tolist() == [t]
    rep = {k: v.repeat_interleave(N, dim=0) for k, v in inp.items() if k in ("generation_mask", "chain_idx", "residue_idx", "residue_mask")}
    gm_d = rep["generation_mask"]
    gm = gm_d.cpu().numpy()
    # ---- the energy: the float64 potential at the recorded x0_hat - no guidance shift, no temperature in it
    assert a["trajectory"]["t"].tolist() == [60, 59, t, s]
    x0 = a["trajectory"]["pred_translations"][:, j].cpu().double().numpy()
    e = guidance_ref(x0, gm, *(rep[k].cpu().numpy() for k in ("chain_idx", "residue_idx", "residue_mask")), 1.3, 3.8, 0.7, 3.8)
    want = 1.3 * e["clash"] + 0.7 * e["bond"]
    U = c["steering"]["energy"].cpu().numpy()
    err_u = np.abs(U.astype(np.float64) - want).max()
    assert (want > 0).all() and err_u <= 1e-5 * np.abs(want).max() + 1e-5, (U, want)
    lw = c["steering"]["log_weight"].cpu().numpy()
    assert np.array_equal(lw, -(F32(lam) * U))
    assert_bitwise({k: c[k] for k in plain}, plain, "ess_threshold = 0 moves nothing")
    # ---- the ancestors: the host rule on the recorded log-weights
    first = FIRST + np.arange(0, rows, N)
    u = orc.philox_uniform4(SEED, first, np.zeros_like(first), t, STREAM_STEER)[0]
    zero = np.zeros(rows, F32)
    rule = resample_oracle(zero, zero, U, u, N, lam, 2.0)
    assert np.array_equal(rule["logw"], np.zeros(rows, F32)) and rule["resampled"].all() and (rule["margin"] >= 1e-12).all(), rule["margin"]
    anc = torch.from_numpy(rule["ancestors"].astype(np.int64) + np.arange(rows) // N * N)
    assert torch.equal(a["steering"]["ancestors"][0].cpu(), anc), (a["steering"]["ancestors"], anc)
    assert np.array_equal(a["steering"]["energy"].cpu().numpy(), U[anc.numpy()]) and not a["steering"]["log_weight"].any()
    moved = int((anc != torch.arange(rows)).sum())
    # ---- the gather: after the tempered, constrained, jumped, guided update
    ta, tp = a["trajectory"], plain["trajectory"]
    for k in ("seq_idx", "translations", "orientations"):
        assert torch.equal(ta[k][:, :j + 1], tp[k][:, :j + 1]), (k, "the record of the steering step is written before the gather")
        assert torch.equal(ta[k][:, j + 1][gm_d], tp[k][:, j + 1][anc.cuda()][gm_d]), (k, "row r holds the generated residues of its ancestor")
        assert torch.equal(ta[k][:, j + 1][~gm_d], tp[k][:, j + 1][~gm_d]), k
    for k in ("pred_translations", "pred_orientations", "seq_probs"):
        assert torch.equal(ta[k][:, :j + 1], tp[k][:, :j + 1]), k
    # the ungathered step itself is the composition (one geometry more for the reference: shared contexts, rows b N + r)
    rep_inp = dict(rep, seq_idx=tp["seq_idx"][:, j])
    ref = reference(model, rep_inp, tp, t, s, temp, allowed.repeat_interleave(N, dim=0), gm, slot=j)
    got = tp["seq_idx"][:, j + 1].cpu().numpy()
    differ = ref["drawn"] & (got != ref["seq"])
    assert (ref["edge"][differ] < 1e-5).all() and int(differ.sum()) <= 2
    spread = float(np.ptp(want.reshape(P, N), axis=1).max())
    print(f"\nsteering {which} K = {K} N = {N}: energy error {err_u:.2e} of {np.abs(want).max():.1f} (spread in a group {spread:.1f}), "
          f"{moved} of {rows} rows moved, "
          f"smallest margin {rule['margin'].min():.2e}, {int(differ.sum())} of {int(ref['drawn'].sum())} draws excused")
    if N == 5:
        assert moved > 0, "some row must move for this case to say anything"
