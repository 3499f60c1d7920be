"""Noise scales and sequence temperature on the MI355X: DiffAb.sample(temperature=...) and diffab_sample_options.temperature.

The rule is DESIGN.md section 4.11 / include/diffab_hip.h.  All-ones values are bitwise the untempered sample; one step is linear in the
translation scale; the rotation angle is the inverse CDF of the scaled row of the stacked table at the Philox uniforms, about the
unscaled axis; tau = 0 is the argmax of what is drawn from and tau = 0.5 the float64 restatement of test_temperature_host.py; zero noise
does not depend on the seed; a per-row sweep is bitwise its rows run alone, on every launch form; and the C entry's NULL struct and its
argument errors behave as documented.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import diffab_oracle as orc
from diffab_pytorch import _hip, so3 as _so3, synthetic as syn
from diffab_pytorch.diffusion import jump_coefficients
from diffab_pytorch.guidance import SampleGuidance
from diffab_pytorch.temperature import SampleTemperature, tempered_draw
from sampler_support import assert_bitwise, hip, lanes, make_model, patches, rows, sample
from test_respaced_host import seq_jump_ref

pytestmark = pytest.mark.gpu
V = 21


@pytest.fixture(scope="module")
def bench(hip):
    dims = dict(syn.BENCH_DIMS, NL=3)
    return dims, make_model(dims, 31)


def rotation_of(O0, O):
    """angle (float64) and unit axis of O0^T O, from the skew part and the trace (well conditioned away from pi)"""
    R = O0.double().transpose(-1, -2) @ O.double()
    w = torch.stack([R[..., 2, 1] - R[..., 1, 2], R[..., 0, 2] - R[..., 2, 0], R[..., 1, 0] - R[..., 0, 1]], -1) / 2
    s = w.norm(dim=-1)
    c = (R.diagonal(dim1=-2, dim2=-1).sum(-1) - 1) / 2
    return torch.atan2(s, c), w / s.clamp_min(1e-30)[..., None]


# ------------------------------------------------------------------ 1. identity
@pytest.mark.parametrize("case", ["plain", "steps", "guidance", "allowed_aa", "num_samples"])
def test_all_ones_is_bitwise_untempered(bench, case):
    dims, model = bench
    B, K, N = 3, 128, 2 if case == "num_samples" else 1
    inp = patches(B, K, dims, seed=5)
    kw = dict(seed=7, t_start=12, t_stop=0, init=False)
    if case == "steps":
        kw.update(steps=5)
    elif case == "guidance":
        kw.update(guidance=SampleGuidance(clash=2.0, bond=1.0, max_shift=0.5))
    elif case == "allowed_aa":
        allowed = torch.rand(K, V, generator=torch.Generator().manual_seed(3)) < 0.5
        allowed[:, 4] = True
        kw.update(allowed_aa=allowed)
    elif case == "num_samples":
        kw.update(num_samples=N)
    plain = sample(model, inp, **kw)
    assert_bitwise(sample(model, inp, temperature=SampleTemperature(), **kw), plain, (case, "defaults"))
    ones = torch.ones(B * N)
    assert_bitwise(sample(model, inp, temperature=SampleTemperature(ones, ones.clone(), ones.clone()), **kw), plain, (case, "per-row ones"))
    hot = sample(model, inp, temperature=SampleTemperature(0.5, 0.5, 0.5), **kw)
    assert not torch.equal(hot["translations"], plain["translations"]), case


# ------------------------------------------------------------------ 2. translations: linear in lambda_x
@pytest.mark.parametrize("t", [40, 1])
def test_one_step_is_linear_in_the_translation_scale(bench, t):
    dims, model = bench
    inp = patches(3, 128, dims, seed=11)
    kw = dict(seed=3, t_start=t, t_stop=t - 1, init=False)
    out = {lam: sample(model, inp, temperature=SampleTemperature(translation=lam), **kw) for lam in (0.0, 0.5, 1.0)}
    for lam in (0.5, 1.0):  # only the translations depend on lambda_x
        assert torch.equal(out[lam]["orientations"], out[0.0]["orientations"]) and torch.equal(out[lam]["seq_idx"], out[0.0]["seq_idx"])
    assert_bitwise(out[1.0], sample(model, inp, **kw), "lambda_x = 1")
    x = {lam: v["translations"].double() for lam, v in out.items()}
    if t == 1:  # the last step adds no noise: x(lambda) = x(0) for every lambda
        assert torch.equal(out[0.5]["translations"], out[0.0]["translations"])
        assert torch.equal(out[1.0]["translations"], out[0.0]["translations"])
        return
    gm = inp["generation_mask"]
    d1, dh = x[1.0] - x[0.0], x[0.5] - x[0.0]
    assert float(d1[gm].abs().max()) > 0.05
    tol = 4 * 2.0 ** -24 * max(1.0, float(x[1.0].abs().max()))  # a few fp32 roundings of x
    assert float((dh - 0.5 * d1).abs().max()) <= tol, float((dh - 0.5 * d1).abs().max())
    assert torch.equal(out[0.5]["translations"][~gm], inp["translations"][~gm])


# ------------------------------------------------------------------ 3. orientations: the scaled row of the stacked table
def test_rotation_draw_at_half_scale(bench):
    dims, model = bench
    B, K, seed = 3, 128, 17
    beta = model.sched["beta"]
    t = next(t for t in range(60, 0, -1) if float(beta[t].sqrt()) * 0.5 < 0.1 < float(beta[t].sqrt()))  # the histogram branch at 0.5
    inp = patches(B, K, dims, seed=19)
    kw = dict(seed=seed, t_start=t, t_stop=t - 1, init=False, trajectory=True, trajectory_predictions=True)
    out = {lam: sample(model, inp, temperature=SampleTemperature(rotation=lam), **kw) for lam in (0.0, 0.5, 1.0)}
    gm = inp["generation_mask"]
    O0 = out[1.0]["trajectory"]["pred_orientations"][:, 0]
    for lam in (0.0, 0.5):  # the record is the model's untempered output; the translations and the sequence do not depend on lambda_O
        assert_bitwise(out[lam]["trajectory"], out[1.0]["trajectory"], ("record", lam))
        assert torch.equal(out[lam]["translations"], out[1.0]["translations"]) and torch.equal(out[lam]["seq_idx"], out[1.0]["seq_idx"])
    assert torch.equal(out[0.0]["orientations"][gm], O0[gm])  # lambda_O = 0: O_s = O0_hat exactly
    th_h, ax_h = rotation_of(O0[gm].cpu(), out[0.5]["orientations"][gm].cpu())
    th_1, ax_1 = rotation_of(O0[gm].cpu(), out[1.0]["orientations"][gm].cpu())
    big = (th_h > 0.02) & (th_1 > 0.02)
    assert int(big.sum()) > 0.8 * int(gm.sum())
    assert float((ax_h[big] - ax_1[big]).abs().max()) < 1e-4  # same axis
    # the angle: host inverse CDF of the device table's lambda = 0.5 row at the Philox uniforms of the step
    stack = model._rev_so3_tempered[((0.5,), None)]
    row = 0 * (model.T + 1) + t
    ua = orc.philox_uniform4(seed, *lanes(0, B, K), t, orc.STREAM_ANGLE)
    cdf = stack._cdf[row].cpu()
    m = gm.cpu()
    th_ref = orc.igso3_theta_from_hist(orc.igso3_bin_from_cdf(cdf, torch.from_numpy(ua[0])[m]), torch.from_numpy(ua[1])[m]).double()
    assert float((th_h - th_ref).abs().max()) < 1e-5, float((th_h - th_ref).abs().max())
    # that row is bitwise a table built alone over 0.5 sqrt(beta), and the scale-1 rows of a stack are the ordinary table's
    alone = _so3.SO3(beta.sqrt() * torch.tensor(0.5), sigma_threshold=0.1, n_bins=8192, num_iters=1024, without_replacement=False)
    assert torch.equal(stack._cdf[: model.T + 1], alone._cdf) and torch.equal(stack.histograms[: model.T + 1], alone.histograms)
    two = model._reverse_so3_tempered((0.5, 1.0), None, 0, None)
    assert torch.equal(two._cdf[model.T + 1:], model._reverse_so3()._cdf)
    assert torch.equal(two._cdf[: model.T + 1], alone._cdf)


# ------------------------------------------------------------------ 4. the sequence
def test_tau_zero_is_the_argmax_of_the_posterior(bench):
    dims, model = bench
    B, K = 3, 128
    inp = patches(B, K, dims, seed=23)
    allowed = torch.rand(K, V, generator=torch.Generator().manual_seed(8)) < 0.4
    allowed[:, 2] = True
    gm = inp["generation_mask"].cpu()
    for al in (None, allowed):
        kw = dict(seed=2, t_start=35, t_stop=34, init=False, trajectory=True, trajectory_predictions=True, allowed_aa=al)
        out = sample(model, inp, temperature=SampleTemperature(sequence=0.0), **kw)
        p = out["trajectory"]["seq_probs"][:, 0].cpu()
        if al is not None:
            p = p.masked_fill(~al, -1.0)
        assert torch.equal(out["seq_idx"].cpu()[gm], p.argmax(-1)[gm]), al is not None
        assert_bitwise(out["trajectory"], sample(model, inp, **kw)["trajectory"], "the record is untempered")


def test_tau_half_is_the_float64_restatement(bench):
    dims, model = bench
    B, K, seed, t = 4, 128, 13, 30
    inp = patches(B, K, dims, seed=29)
    allowed = torch.rand(K, V, generator=torch.Generator().manual_seed(4)) < 0.6
    allowed[:, 0] = True
    gm = inp["generation_mask"].cpu().numpy()
    us = orc.philox_uniform4(seed, *lanes(0, B, K), t, orc.STREAM_SEQ)[0]
    for al in (None, allowed):
        kw = dict(seed=seed, t_start=t, t_stop=t - 1, init=False, trajectory=True, trajectory_predictions=True, allowed_aa=al)
        out = sample(model, inp, temperature=SampleTemperature(sequence=0.5), **kw)
        p = out["trajectory"]["seq_probs"][:, 0].cpu().double().numpy()
        got = out["seq_idx"].cpu().numpy()
        n_bad = n_draw = 0
        for b, k in zip(*np.nonzero(gm)):
            ok = None if al is None else al[k].tolist()
            want = tempered_draw(p[b, k], float(us[b, k]), 0.5, ok)
            n_draw += 1
            if got[b, k] == want:
                continue
            mask = np.ones(V, bool) if ok is None else np.array(ok)
            w = np.where(mask, p[b, k], 0.0) ** 2
            edge = np.abs(np.cumsum(w) / w.sum() - float(us[b, k])).min()
            assert edge < 1e-5, (b, k, got[b, k], want, edge)
            n_bad += 1
        assert n_draw > 50, n_draw
    plain = sample(model, inp, **kw)
    assert not torch.equal(out["seq_idx"], plain["seq_idx"])


def test_respaced_tau_zero_is_the_argmax_of_the_jump_distribution(bench):
    dims, model = bench
    B, K, t, s = 3, 128, 40, 25
    inp = patches(B, K, dims, seed=37)
    kw = dict(seed=4, t_start=t, t_stop=s, steps=[t], init=False, trajectory=True, trajectory_predictions=True)
    out = sample(model, inp, temperature=SampleTemperature(sequence=0.0), **kw)
    sch = model.sched
    aj = float(jump_coefficients(sch, torch.tensor([t]), s, model.beta_max)[1][t])
    p = out["trajectory"]["seq_probs"][:, 0].cpu().double().numpy()
    r = seq_jump_ref(p, inp["seq_idx"].cpu().numpy(), float(sch["alpha"][t]), float(sch["beta"][t]), float(sch["alpha_bar"][t - 1]), aj,
                     float(sch["alpha_bar"][s]))
    gm = inp["generation_mask"].cpu().numpy()
    got = out["seq_idx"].cpu().numpy()[gm]
    want = r.argmax(-1)[gm]
    top2 = np.sort(r[gm], -1)[:, -2:]
    close = (top2[:, 1] - top2[:, 0]) < 1e-5 * top2[:, 1]
    assert np.array_equal(got[~close], want[~close]), int((got != want).sum())


# ------------------------------------------------------------------ 5. zero noise does not depend on the seed
def test_zero_noise_is_seed_independent(bench):
    dims, model = bench
    inp = patches(3, 128, dims, seed=41)
    zero = SampleTemperature(0.0, 0.0, 0.0)
    kw = dict(t_start=15, t_stop=0, init=False, temperature=zero)
    a = sample(model, inp, seed=1, **kw)
    assert_bitwise(sample(model, inp, seed=987654321, **kw), a, "seeds")
    assert_bitwise(sample(model, inp, seed=5, steps=4, **kw), sample(model, inp, seed=6, steps=4, **kw), "respaced")
    assert not torch.equal(sample(model, inp, seed=1, t_start=15, t_stop=0, init=False)["translations"], a["translations"])


# ------------------------------------------------------------------ 6. a per-row sweep is its rows run alone
SWEEP = [(1.0, 1.0, 1.0), (0.5, 0.25, 0.3), (0.0, 2.0, 0.0), (1.5, 0.0, 2.0)]
FORMS = {"per_layer": dict(flags=_hip.FLAG_MULTI_LAUNCH), "module": dict(flags=_hip.FLAG_PERSISTENT_MODULE), "graph": dict(graph=True),
         "k256": dict()}


def sweep_temperature(vals):
    cols = [torch.tensor([v[j] for v in vals]) for j in range(3)]
    return SampleTemperature(*cols)


@pytest.mark.parametrize("form", sorted(FORMS))
def test_per_row_sweep_is_each_row_alone(bench, form):
    dims, model = bench
    K = 256 if form == "k256" else 128
    B = len(SWEEP)
    inp = patches(B, K, dims, seed=43)
    kw = dict(seed=8, t_start=12, t_stop=0, init=False, **FORMS[form])
    whole = sample(model, inp, temperature=sweep_temperature(SWEEP), **kw)
    for b, (lx, lo, tau) in enumerate(SWEEP):
        alone = sample(model, rows(inp, torch.tensor([b], device="cuda")), first_patch=b, temperature=SampleTemperature(lx, lo, tau), **kw)
        assert_bitwise(alone, {k: v[b:b + 1] for k, v in whole.items()}, (form, b))
    assert_bitwise(sample(model, rows(inp, torch.tensor([0], device="cuda")), **kw), {k: v[:1] for k, v in whole.items()}, "row 0 = ones")
    if form == "per_layer":  # two shards, each with its rows' values and first_patch = lo
        for lo, hi in ((0, 2), (2, 4)):
            part = sample(model, rows(inp, torch.arange(lo, hi, device="cuda")), first_patch=lo, temperature=sweep_temperature(SWEEP[lo:hi]),
                          **kw)
            assert_bitwise(part, {k: v[lo:hi] for k, v in whole.items()}, ("shard", lo))
        # eager against graph replay of the same sweep, and the module launch
        assert_bitwise(sample(model, inp, temperature=sweep_temperature(SWEEP), seed=8, t_start=12, t_stop=0, init=False, graph=True),
                       whole, "graph")
        assert_bitwise(sample(model, inp, temperature=sweep_temperature(SWEEP), seed=8, t_start=12, t_stop=0, init=False,
                              flags=_hip.FLAG_PERSISTENT_MODULE), whole, "module")


# ------------------------------------------------------------------ 7. the C entry
class Proxy:
    """The library with the temperature struct of diffab_sample_loop_ex's options rewritten by `edit` (None: passed as NULL); the rc is
    recorded."""

    def __init__(self, lib, edit):
        self._lib, self._edit, self.rc = lib, edit, []

    def __getattr__(self, name):
        return getattr(self._lib, name)

    def diffab_sample_loop_ex(self, *args):
        opt = args[-2]._obj  # the SampleOptions behind byref
        t = self._edit(opt.temperature.contents if opt.temperature else None)  # (contents shares the struct's memory)
        opt.temperature = None if t is None else C.pointer(t)
        self.rc.append(self._lib.diffab_sample_loop_ex(*args))
        return self.rc[-1]


def test_null_struct_is_guided_and_bad_structs_enqueue_nothing(bench, monkeypatch):
    dims, model = bench
    lib = _hip.lib()
    inp = patches(2, 128, dims, seed=47)
    guide = SampleGuidance(clash=1.0, bond=1.0)
    kw = dict(seed=9, t_start=10, t_stop=0, init=False, guidance=guide)
    want = sample(model, inp, **kw)  # guidance alone: options.temperature NULL
    proxy = Proxy(lib, lambda s: None)
    monkeypatch.setattr(_hip, "lib", lambda: proxy)
    # (lambda_O = 1: the call passes the ordinary reverse table, which a NULL struct reads at row t)
    assert_bitwise(sample(model, inp, temperature=SampleTemperature(0.5, 1.0, 0.5), **kw), want, "NULL struct")
    assert proxy.rc == [0]

    def rewrite(**fields):
        def edit(s):
            for k, v in fields.items():
                setattr(s, k, getattr(s, v) if isinstance(v, str) else v)
            return s
        return edit

    cases = [  # (the Python call, the struct it is turned into)
        (dict(temperature=SampleTemperature(rotation=0.5)), rewrite(rot_row=None)),
        (dict(mode="fixed_backbone", temperature=SampleTemperature(sequence=0.5)), rewrite(trans_scale="seq_temp")),
        (dict(mode="fixed_backbone", temperature=SampleTemperature(sequence=0.5)), rewrite(rot_scale="seq_temp", rot_row="seq_temp")),
        (dict(mode="structure", temperature=SampleTemperature(rotation=0.5)), rewrite(seq_temp="rot_scale")),
    ]
    tensors = {}  # every tensor handed to the library, by address: the state buffers the call was given are read back after it returned
    real_ptr = _hip.ptr

    def recording_ptr(t):
        if t is not None:
            tensors[t.data_ptr()] = t
        return real_ptr(t)

    monkeypatch.setattr(_hip, "ptr", recording_ptr)
    for extra, edit in cases:
        proxy = Proxy(lib, edit)
        monkeypatch.setattr(_hip, "lib", lambda: proxy)
        seen = {}
        real = lib.diffab_sample_loop_ex

        def spy(*args, real=real):
            state = [tensors[a.value] for a in args[4:7]]  # seq, x, O
            before = [v.clone() for v in state]
            rc = real(*args)
            torch.cuda.synchronize()
            seen["same"] = all(torch.equal(a, b) for a, b in zip(before, state))
            return rc

        proxy._lib = type("L", (), {"diffab_sample_loop_ex": staticmethod(spy), "__getattr__": lambda s, n: getattr(lib, n)})()
        kw2 = dict(kw, **extra)
        if extra.get("mode") == "fixed_backbone":
            kw2.pop("guidance")
        with pytest.raises(_hip.DiffabHipError, match="code -1"):
            sample(model, inp, **kw2)
        assert proxy.rc == [-1] and seen["same"], (extra, proxy.rc, seen)
