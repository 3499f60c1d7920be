"""CPU: noise scales and sequence temperature of the reverse sampler - argument checks made before any device work,
broadcasting of the per-row values, the float64 restatement of the tempered draw on hand-made posteriors, the stacked-table row mapping
and the C-ABI binding.  The device side is tests/test_gpu_temperature.py."""
import ctypes
import math

import pytest
import torch

import sampler_support as support
from diffab_pytorch import _hip
from diffab_pytorch.temperature import (MAX_ROTATION_SCALES, SampleTemperature, check_mode, row_values, rotation_rows, rotation_scales,
                                        stacked_sigmas, tempered_draw)
from sampler_support import ReachedTheLibrary, inputs, refuse_library, stand_in

V, T = 21, 100


# ------------------------------------------------------------------ the float64 restatement of the draw
def test_tau_zero_is_the_argmax_lowest_index_on_ties():
    assert tempered_draw([0.1, 0.6, 0.3], 0.99, 0.0) == 1
    assert tempered_draw([0.4, 0.2, 0.4], 0.99, 0.0) == 0
    assert tempered_draw([0.4, 0.2, 0.2, 0.2], 0.5, 0.0, allowed=[False, True, True, True]) == 1
    assert tempered_draw([0.5, 0.1, 0.3, 0.1], 0.0, 0.0, allowed=[False, True, False, True]) == 1


def test_tau_half_squares_the_probabilities():
    p = [0.1, 0.6, 0.3]  # weights 0.01, 0.36, 0.09 (total 0.46)
    assert tempered_draw(p, 0.01, 0.5) == 0   # u * 0.46 = 0.0046 < 0.01
    assert tempered_draw(p, 0.5, 0.5) == 1    # 0.23 in (0.01, 0.37]
    assert tempered_draw(p, 0.9, 0.5) == 2    # 0.414 > 0.37
    assert tempered_draw(p, 0.02, 0.5) == 0 and tempered_draw(p, 0.03, 0.5) == 1  # the edge 0.01 / 0.46 = 0.0217...
    # the same draws from the explicit p^2 distribution
    w = [v * v for v in p]
    for u in (0.01, 0.02, 0.03, 0.5, 0.79, 0.81, 0.9, 0.999):
        edge = [sum(w[: k + 1]) / sum(w) for k in range(3)]
        assert tempered_draw(p, u, 0.5) == next(k for k in range(3) if edge[k] > u)


def test_tau_one_is_the_plain_categorical_and_large_tau_flattens():
    p = [0.05, 0.25, 0.0, 0.7]
    for u in (0.01, 0.049, 0.051, 0.29, 0.31, 0.99):
        acc, want = 0.0, None
        for v, q in enumerate(p):
            acc += q
            if acc > u:
                want = v
                break
        assert tempered_draw(p, u, 1.0) == want, u
    # tau -> inf: uniform over the classes of positive probability (a zero stays impossible)
    draws = [tempered_draw(p, u, 1e6) for u in (0.1, 0.4, 0.6, 0.9, 0.9999)]
    assert draws == [0, 1, 1, 3, 3]
    assert 2 not in {tempered_draw(p, u / 100, 1e6) for u in range(100)}


def test_constrained_tempered_draw_and_the_unit_weight_fallback():
    p = [0.5, 0.0, 0.0, 0.5]
    allowed = [False, True, True, False]  # every allowed class at probability 0: unit weights over {1, 2}
    assert [tempered_draw(p, u, tau, allowed) for tau in (0.0, 0.5, 2.0) for u in (0.2, 0.7)] == [1, 2] * 3
    assert tempered_draw(p, 0.3, 0.5, [False] * 4) == -1
    # restricted, then tempered: p over {0, 2, 3} = (0.2, 0.3, 0.1) -> tau = 0.5 weights (0.04, 0.09, 0.01) / 0.14
    q = [0.2, 0.4, 0.3, 0.1]
    al = [True, False, True, True]
    assert tempered_draw(q, 0.28, 0.5, al) == 0 and tempered_draw(q, 0.29, 0.5, al) == 2
    assert tempered_draw(q, 0.92, 0.5, al) == 2 and tempered_draw(q, 0.93, 0.5, al) == 3
    assert tempered_draw(q, 0.5, 0.0, al) == 2


def test_weights_are_relative_to_the_largest_probability():
    """exp((log p_v - log p_max) / tau): no underflow of the whole distribution at small tau, whatever the scale of p."""
    p = [1e-30, 3e-30, 2e-30]
    assert tempered_draw(p, 0.999, 0.01) == 1 and tempered_draw(p, 1e-9, 0.01) == 1  # (1/3)^100 of the mass below class 1
    w = [math.exp((math.log(v) - math.log(3e-30)) / 0.25) for v in p]
    edge0 = w[0] / sum(w)
    assert tempered_draw(p, edge0 * 0.999, 0.25) == 0 and tempered_draw(p, edge0 * 1.001, 0.25) == 1


# ------------------------------------------------------------------ per-row values
def test_row_values_broadcast_scalars_and_per_row_tensors():
    lx, lo, tau = row_values("t", SampleTemperature(), 5)
    assert all(v.dtype == torch.float32 and v.shape == (5,) and bool((v == 1).all()) for v in (lx, lo, tau))
    lx, lo, tau = row_values("t", SampleTemperature(translation=0.5, rotation=torch.tensor(2.0), sequence=torch.tensor([0.25])), 3)
    assert lx.tolist() == [0.5] * 3 and lo.tolist() == [2.0] * 3 and tau.tolist() == [0.25] * 3
    per = torch.tensor([0.0, 0.5, 1.0, 2.0], dtype=torch.float64)
    assert row_values("t", SampleTemperature(sequence=per), 4)[2].tolist() == per.tolist()
    assert row_values("t", SampleTemperature(translation=torch.tensor([1, 0, 2])), 3)[0].tolist() == [1.0, 0.0, 2.0]


@pytest.mark.parametrize("kw, match", [
    (dict(translation=-0.5), ">= 0"), (dict(rotation=float("nan")), "finite"), (dict(sequence=float("inf")), "finite"),
    (dict(sequence=torch.tensor([1.0, -1e-9, 1.0])), ">= 0"), (dict(translation=torch.tensor([1.0, float("nan"), 1.0])), "finite"),
    (dict(rotation=1e39), "finite in fp32"), (dict(translation=torch.ones(2)), "does not broadcast"),
    (dict(sequence=torch.ones(3, 1)), "1-D tensor"), (dict(rotation=True), "number or a 1-D tensor"), (dict(sequence="1"), "number"),
    (dict(translation=torch.tensor([True, False, True])), "real numbers"),
])
def test_bad_values_are_rejected(kw, match):
    with pytest.raises(ValueError, match=match):
        row_values("t", SampleTemperature(**kw), 3)


def test_not_a_sample_temperature_is_rejected():
    with pytest.raises(ValueError, match="temperature.SampleTemperature"):
        row_values("t", {"translation": 1.0}, 3)


def test_at_most_sixteen_distinct_nonzero_rotation_scales():
    ok = torch.cat([torch.zeros(3), torch.arange(1, MAX_ROTATION_SCALES + 1) / 8.0, torch.ones(2)])
    assert len(rotation_scales(row_values("t", SampleTemperature(rotation=ok), ok.numel())[1])) == MAX_ROTATION_SCALES
    bad = torch.arange(1, MAX_ROTATION_SCALES + 2) / 8.0
    with pytest.raises(ValueError, match="17 distinct rotation scales"):
        row_values("t", SampleTemperature(rotation=bad), bad.numel())


def test_mode_checks():
    ones = tuple(torch.ones(2) for _ in range(3))
    check_mode("t", ones, True, False)
    check_mode("t", ones, False, True)
    half = torch.full((2,), 0.5)
    with pytest.raises(ValueError, match="fixed_backbone"):
        check_mode("t", (half, ones[1], ones[2]), True, False)
    with pytest.raises(ValueError, match="fixed_backbone"):
        check_mode("t", (ones[0], torch.tensor([1.0, 0.0]), ones[2]), True, False)
    with pytest.raises(ValueError, match="mode='structure'"):
        check_mode("t", (ones[0], ones[1], half), False, True)
    check_mode("t", (half, half, ones[2]), False, True)
    check_mode("t", (ones[0], ones[1], half), True, False)


# ------------------------------------------------------------------ the stacked table
def test_stacked_table_row_mapping():
    rot = torch.tensor([1.0, 0.5, 0.0, 1.0, 2.0, 0.5])
    scales = rotation_scales(rot)
    assert scales == (0.5, 1.0, 2.0)
    assert rotation_rows(rot, scales, T).tolist() == [1 * (T + 1), 0, 0, 1 * (T + 1), 2 * (T + 1), 0]
    assert rotation_rows(rot, scales, T).dtype == torch.int32
    base = torch.linspace(0.01, 0.9, T + 1).sqrt()
    sig = stacked_sigmas(base, scales)
    assert sig.shape == (3 * (T + 1),) and sig.dtype == torch.float32
    for k, s in enumerate(scales):  # row (k, t) at k (T + 1) + t holds lambda_k sqrt(beta'_t), the fp32 product
        assert torch.equal(sig[k * (T + 1):(k + 1) * (T + 1)], base * torch.tensor(s, dtype=torch.float32))
    assert torch.equal(sig[T + 1:2 * (T + 1)], base)  # the lambda = 1 list is sqrt(beta') itself, bit for bit
    assert rotation_scales(torch.zeros(4)) == () and rotation_rows(torch.zeros(4), (), T).tolist() == [0] * 4


def test_rotation_scales_are_keyed_by_their_fp32_value():
    rot = row_values("t", SampleTemperature(rotation=torch.tensor([0.1, 0.1 + 1e-12, 0.3], dtype=torch.float64)), 3)[1]
    assert rotation_scales(rot) == (float(torch.tensor(0.1)), float(torch.tensor(0.3)))


# ------------------------------------------------------------------ DiffAb.sample: every check before device work
@pytest.fixture(scope="module")
def model():
    return stand_in(T=T)


@pytest.fixture(autouse=True)
def no_library(monkeypatch):
    refuse_library(monkeypatch)


def call(model, B=2, K=16, n_ctx=None, **kw):
    return support.call(model, inputs(B, K, n_ctx), **kw)


@pytest.mark.parametrize("temp, kw, match", [
    (SampleTemperature(translation=-1.0), {}, ">= 0"),
    (SampleTemperature(rotation=float("nan")), {}, "finite"),
    (SampleTemperature(sequence=float("-inf")), {}, "finite"),
    (SampleTemperature(sequence=torch.ones(3)), {}, "does not broadcast to the 2 output rows"),
    (SampleTemperature(rotation=torch.arange(1, 18) / 4.0), dict(B=17), "17 distinct rotation scales"),
    (SampleTemperature(translation=0.5), dict(mode="fixed_backbone"), "fixed_backbone"),
    (SampleTemperature(rotation=torch.tensor([1.0, 0.0])), dict(mode="fixed_backbone"), "fixed_backbone"),
    (SampleTemperature(sequence=0.0), dict(mode="structure"), "mode='structure'"),
    ("hot", {}, "temperature.SampleTemperature"),
])
def test_bad_temperature_is_rejected_before_device_work(model, temp, kw, match):
    with pytest.raises(ValueError, match=match):
        call(model, temperature=temp, **kw)


@pytest.mark.parametrize("temp, kw", [
    (SampleTemperature(), {}),
    (SampleTemperature(translation=0.0, rotation=0.5, sequence=0.1), {}),
    (SampleTemperature(sequence=0.3), dict(mode="fixed_backbone")),  # the kept modality at 1: allowed
    (SampleTemperature(translation=torch.tensor([0.5, 1.0]), rotation=0.0), dict(mode="structure")),
    (SampleTemperature(sequence=torch.tensor([0.1, 0.2, 0.3, 0.4])), dict(num_samples=2)),  # per output row: B N = 4
    (SampleTemperature(rotation=torch.tensor([0.5, 1.0, 2.0])), dict(B=3, n_ctx=2, context_index=torch.tensor([1, 0, 1]))),
])
def test_good_temperature_reaches_the_library(model, temp, kw):
    with pytest.raises(ReachedTheLibrary):
        call(model, temperature=temp, **kw)


def test_per_row_values_follow_the_output_rows(model):
    """num_samples = N: one value per output row (B N), not per patch; context_index: one per state row, not per context."""
    with pytest.raises(ValueError, match="does not broadcast to the 4 output rows"):
        call(model, num_samples=2, temperature=SampleTemperature(sequence=torch.tensor([0.5, 0.5])))
    with pytest.raises(ReachedTheLibrary):
        call(model, num_samples=2, temperature=SampleTemperature(sequence=torch.tensor([0.5])))
    with pytest.raises(ValueError, match="does not broadcast to the 3 output rows"):
        call(model, B=3, n_ctx=2, context_index=torch.tensor([1, 0, 1]), temperature=SampleTemperature(translation=torch.ones(2)))


# ------------------------------------------------------------------ the C ABI
def test_temperature_struct_layout():
    fields = [f[0] for f in _hip.SampleTemperature._fields_]
    assert fields == ["trans_scale", "rot_scale", "seq_temp", "rot_row"]
    assert ctypes.sizeof(_hip.SampleTemperature) == 4 * ctypes.sizeof(ctypes.c_void_p)
