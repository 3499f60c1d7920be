"""CPU: the host side of fewer-step reverse sampling (DiffAb.sample(steps=...)) - the even step list, the jump coefficients, a float64
restatement of the sequence jump against brute force, the argument checks that happen before any library call, and the C-ABI entries.

The rule is DESIGN.md section 4.9 / include/diffab_hip.h (diffab_sample_options.steps)."""
import ctypes

import numpy as np
import pytest
import torch

import sampler_support as support
from diffab_pytorch import _hip
from diffab_pytorch.diffab_pytorch import _trajectory_labels
from diffab_pytorch.diffusion import cosine_variance_schedule, even_steps, jump_coefficients
from sampler_support import ReachedTheLibrary, inputs, refuse_library, stand_in

V, T = 21, 10


# ------------------------------------------------------------------ the float64 restatement (shared with test_gpu_respaced.py)
def seq_jump_ref(p, s_t, at, bt, ab1, aj, abs_, V=V):
    """r (..., V) float64 of the jump t -> s from the head posterior p (..., V) and the token s_t (...), the formulas of DESIGN 4.9 with
    the schedule values given as they are stored (fp32, promoted)."""
    p = np.asarray(p, dtype=np.float64)
    onehot = np.arange(V) == np.asarray(s_t)[..., None]
    at, bt, ab1, aj, abs_ = (np.asarray(v, dtype=np.float64)[..., None] for v in (at, bt, ab1, aj, abs_))
    A = np.where(onehot, at, 0.0) + bt / V
    c = (1.0 - ab1) / V
    S = (p / A).sum(-1, keepdims=True)
    mix = (ab1 * A + c) * np.maximum(0.0, p / A - c * S)
    tot = mix.sum(-1, keepdims=True)
    pi = np.where(tot > 0, mix / np.where(tot > 0, tot, 1.0), p)
    Aj = np.where(onehot, aj, 0.0) + (1.0 - aj) / V
    cj = (1.0 - abs_) / V
    Z = abs_ * Aj + cj
    W = (pi / Z).sum(-1, keepdims=True)
    return Aj * (cj * W + abs_ * pi / Z)


def q_step(a, src, V=V):
    """q(. | src) of a uniform-noise transition keeping src with weight a: (..., V) float64."""
    a = np.asarray(a, dtype=np.float64)[..., None]
    return np.where(np.arange(V) == np.asarray(src)[..., None], a, 0.0) + (1.0 - a) / V


def posterior_ref(s_t, s_0, a_fwd, ab_prev, V=V):
    """q(s_prev | s_t, s_0) proportional to q(s_t | s_prev) q(s_prev | s_0): (..., V) float64 over s_prev (q(s_t | s_prev) as a
    function of s_prev is a_fwd [s_prev = s_t] + (1 - a_fwd) / V)."""
    w = q_step(a_fwd, s_t, V) * q_step(ab_prev, s_0, V)
    return w / w.sum(-1, keepdims=True)


# ------------------------------------------------------------------ the step list
def test_even_steps_endpoints_and_spacing():
    assert even_steps(100, 0, 1).tolist() == [100]
    assert even_steps(100, 0, 100).tolist() == list(range(100, 0, -1))
    assert even_steps(100, 0, 2).tolist() == [100, 1]
    for n in (3, 10, 20, 50, 99):
        st = even_steps(100, 0, n)
        assert st.dtype == torch.int64 and st.numel() == n
        assert int(st[0]) == 100 and int(st[-1]) == 1
        assert bool((st[1:] < st[:-1]).all())
        # round_half_up(j (L - 1) / (n - 1)), in exact rationals
        want = [100 - int(np.floor(j * 99 / (n - 1) + 0.5)) for j in range(n)]
        assert st.tolist() == want
    assert even_steps(100, 0, 3).tolist() == [100, 50, 1]  # 49.5 rounds up


def test_even_steps_optimize_from_and_t_stop():
    assert even_steps(8, 0, 8).tolist() == list(range(8, 0, -1))  # optimize_from = 8: the list starts there
    assert even_steps(8, 0, 3).tolist() == [8, 4, 1]  # 3.5 rounds up
    assert even_steps(30, 10, 20).tolist() == list(range(30, 10, -1))
    assert even_steps(30, 10, 5).tolist() == [30, 25, 20, 16, 11]
    assert even_steps(30, 10, 1).tolist() == [30]
    for bad in (0, 21, -1, True, 2.0):
        with pytest.raises(ValueError, match="need an int in \\[1, t_start - t_stop\\] = \\[1, 20\\]"):
            even_steps(30, 10, bad)


# ------------------------------------------------------------------ jump coefficients
@pytest.mark.parametrize("steps, t_stop", [([100, 99, 98, 70, 40, 3, 2, 1], 0), (list(range(100, 0, -1)), 0), ([100, 60, 20], 0),
                                           ([57, 20], 0), ([30, 29, 5], 1), ([100], 80), ([8], 0)])
def test_jump_coefficients_against_float64(steps, t_stop):
    sched = cosine_variance_schedule(100, s=0.01, beta_max=0.999)
    st = torch.tensor(steps)
    beta, alpha = jump_coefficients(sched, st, t_stop, 0.999)
    assert beta.dtype == alpha.dtype == torch.float32 and beta.shape == alpha.shape == (101,)
    ab = sched["alpha_bar"].double()
    nxt = steps[1:] + [t_stop]
    listed = dict(zip(steps, nxt))
    for t in range(101):
        s = listed.get(t)
        if s is None or s == t - 1:  # the schedule's own values, copied
            assert torch.equal(beta[t], sched["beta"][t]) and torch.equal(alpha[t], sched["alpha"][t]), t
            continue
        b = min(max(1.0 - float(ab[t]) / float(ab[s]), 1e-5), 0.999)
        assert float(beta[t]) == float(torch.tensor(b, dtype=torch.float64).float()), t
        assert float(alpha[t]) == float(torch.tensor(1.0 - b, dtype=torch.float64).float()), t
        assert 0.0 < float(beta[t]) < 1.0 and 0.0 < float(alpha[t]) < 1.0


def test_every_step_listed_is_the_schedule():
    sched = cosine_variance_schedule(100, s=0.01, beta_max=0.999)
    beta, alpha = jump_coefficients(sched, torch.arange(100, 0, -1), 0, 0.999)
    assert torch.equal(beta, sched["beta"]) and torch.equal(alpha, sched["alpha"])


# ------------------------------------------------------------------ the sequence jump, float64, against brute force
@pytest.mark.parametrize("t, s", [(100, 80), (100, 0), (57, 20), (30, 1), (8, 0), (3, 1), (100, 98), (50, 2)])
def test_sequence_jump_against_brute_force(t, s):
    sched = {k: v.double() for k, v in cosine_variance_schedule(100, s=0.01, beta_max=0.999).items()}
    ab = sched["alpha_bar"]
    rng = np.random.default_rng(t * 101 + s)
    n = 64
    s_t = rng.integers(0, V, n)
    pi = rng.dirichlet(np.full(V, 0.3), n)  # a spread of x0 mixtures, some near one-hot
    pi[:8] = np.eye(V)[rng.integers(0, V, 8)]  # exact one-hot x0 (an exact denoiser)
    a_t, b_t, ab1, ab_s = float(sched["alpha"][t]), float(sched["beta"][t]), float(ab[t - 1]), float(ab[s])
    aj = float(ab[t]) / ab_s if s > 0 else float(ab[t])
    aj = 1.0 - min(max(1.0 - aj, 1e-5), 0.999)
    # p = sum_u pi_u q(s_{t-1} | s_t, u), and the brute-force jump sum_u pi_u q(s_s | s_t, u)
    post = np.stack([posterior_ref(s_t, np.full(n, u), a_t, ab1) for u in range(V)], 1)  # (n, u, V)
    p = (pi[:, :, None] * post).sum(1)
    jump = np.stack([posterior_ref(s_t, np.full(n, u), aj, ab_s) for u in range(V)], 1)
    want = (pi[:, :, None] * jump).sum(1)
    r = seq_jump_ref(p, s_t, a_t, b_t, ab1, aj, ab_s)
    assert np.abs(r - want).max() < 1e-9, np.abs(r - want).max()
    assert np.abs(r.sum(-1) - 1.0).max() < 1e-12
    if s == 0:  # the jump to 0 is the recovered x0 distribution
        assert np.abs(r - pi).max() < 1e-9
    # with p rounded to fp32 (what the device sees) the recovery stays close
    r32 = seq_jump_ref(p.astype(np.float32), s_t, a_t, b_t, ab1, aj, ab_s)
    assert np.abs(r32 - want).max() < 5e-5, np.abs(r32 - want).max()


def test_stride_one_jump_is_the_posterior():
    """s = t - 1 with alpha' = alpha_t: the jump distribution is p itself (the loop then draws from p directly)."""
    sched = {k: v.double() for k, v in cosine_variance_schedule(100, s=0.01, beta_max=0.999).items()}
    rng = np.random.default_rng(5)
    for t in (100, 40, 2):
        s_t = rng.integers(0, V, 16)
        pi = rng.dirichlet(np.full(V, 0.5), 16)
        a_t, b_t, ab1 = float(sched["alpha"][t]), float(sched["beta"][t]), float(sched["alpha_bar"][t - 1])
        post = np.stack([posterior_ref(s_t, np.full(16, u), a_t, ab1) for u in range(V)], 1)
        p = (pi[:, :, None] * post).sum(1)
        r = seq_jump_ref(p, s_t, a_t, b_t, ab1, a_t, ab1)
        assert np.abs(r - p).max() < 1e-9


# ------------------------------------------------------------------ argument checks before the library
@pytest.fixture(scope="module")
def model():
    return stand_in(T=T)


@pytest.fixture(autouse=True)
def no_library(monkeypatch):
    refuse_library(monkeypatch)


def call(model, B=2, K=16, **kw):
    return support.call(model, inputs(B, K), **kw)


@pytest.mark.parametrize("bad, match", [
    (0, "need an int in \\[1, t_start - t_stop\\] = \\[1, 10\\]"), (11, "need an int in \\[1, t_start - t_stop\\]"),
    (-2, "need an int in"), (True, "an int n or a 1-D list"), (False, "an int n or a 1-D list"), (2.0, "an int n or a 1-D list"),
    ([], "non-empty 1-D integer list"), (torch.tensor([[10, 5]]), "non-empty 1-D integer list"),
    (torch.tensor([10.0, 5.0]), "non-empty 1-D integer list"), (torch.tensor([True, False]), "non-empty 1-D integer list"),
    ([9, 5], "starts at 9, the run at t_start = 10"), ([10, 5, 5, 1], "not strictly descending"), ([10, 3, 5], "not strictly descending"),
    ([10, 4, 0], "step 0 is not above t_stop = 0"), ([11, 5], "starts at 11"),
])
def test_bad_steps_are_rejected(model, bad, match):
    with pytest.raises(ValueError, match=match):
        call(model, steps=bad)


def test_bad_steps_in_a_truncated_run_are_rejected(model):
    with pytest.raises(ValueError, match="step 3 is not above t_stop = 3"):
        call(model, steps=[8, 5, 3], t_start=8, t_stop=3)
    with pytest.raises(ValueError, match="starts at 10, the run at t_start = 6"):
        call(model, steps=[10, 5], optimize_from=6)
    with pytest.raises(ValueError, match="t_start = 4 > t_stop = 4"):
        call(model, steps=1, t_start=4, t_stop=4)
    with pytest.raises(ValueError, match="steps needs T = 10 >= t_start = 12"):
        call(model, steps=2, t_start=12)


def test_trajectory_labels_must_be_executed_steps(model):
    with pytest.raises(ValueError, match="trajectory step 7 is not one of the executed steps \\[10, 6, 1\\]"):
        call(model, steps=[10, 6, 1], trajectory=[10, 7])


@pytest.mark.parametrize("kw", [dict(steps=5), dict(steps=[10, 9, 2]), dict(steps=torch.tensor([10, 4, 1]), trajectory=True),
                                dict(steps=1, num_samples=2, allowed_aa=torch.ones(V, dtype=torch.bool)),
                                dict(steps=3, mode="structure", optimize_from=5), dict(steps=[6, 2], optimize_from=6, trajectory=[2])])
def test_good_steps_reach_the_library(model, kw):
    with pytest.raises(ReachedTheLibrary):
        call(model, **kw)


def test_trajectory_labels_of_a_respaced_run():
    ex = torch.tensor([10, 8, 5, 3, 1])
    assert _trajectory_labels("x", True, False, 10, 0, T, ex).tolist() == [10, 8, 5, 3, 1]
    assert _trajectory_labels("x", 2, False, 10, 0, T, ex).tolist() == [10, 5, 1]
    assert _trajectory_labels("x", 1, False, 10, 0, T, ex).tolist() == [10, 8, 5, 3, 1]
    assert _trajectory_labels("x", [3, 10], False, 10, 0, T, ex).tolist() == [10, 3]
    # steps=None keeps the ordinary labels
    assert _trajectory_labels("x", 4, False, 10, 0, T).tolist() == [10, 6, 2]


# ------------------------------------------------------------------ the C ABI
def test_library_exports_the_steps_entries():
    lib = ctypes.CDLL(_hip.LIB_PATH)
    assert hasattr(lib, "diffab_reverse_update_jump") and "diffab_reverse_update_jump" in _hip.SYMBOLS
    # the step list travels in diffab_sample_options.steps (the loop's own ABI: test_cabi_and_host.py)
    assert dict(_hip.SampleOptions._fields_)["steps"] == ctypes.POINTER(_hip.SampleSteps)
    jump, upd = _hip.SYMBOLS["diffab_reverse_update_jump"][1], _hip.SYMBOLS["diffab_reverse_update"][1]
    # diffab_reverse_update's arguments with (s, beta', alpha') after t and r_out after u_seq
    assert len(jump) == len(upd) + 4
    assert jump[:2] == upd[:2] and jump[2:5] == [ctypes.c_int32, ctypes.c_float, ctypes.c_float]
    assert jump[5:15] == upd[2:12] and jump[16:] == upd[12:]


def test_steps_struct_layout():
    # int32 n_steps, then four pointers (the host list, the host beta' / alpha' tables, the device plan)
    names = [f[0] for f in _hip.SampleSteps._fields_]
    assert names == ["n_steps", "steps", "beta_jump", "alpha_jump", "plan_dev"]
    assert ctypes.sizeof(_hip.SampleSteps) == 8 + 4 * ctypes.sizeof(ctypes.c_void_p)
