"""tests/so3_ref.py checked on the host: the float64 oracle the edge tests of the SO(3) kernels (tests/test_gpu_so3_edges.py) compare
against must itself be right at theta near 0 and pi, agree with the reference-shaped oracle where that one is well defined, and
differentiate exp correctly down to |v| = 0."""
import numpy as np
import torch

import diffab_oracle as orc
import so3_ref as ref


def inputs():
    if not hasattr(inputs, "cache"):
        inputs.cache = ref.edge_inputs()
    return inputs.cache


def test_exp_log_round_trip_at_every_angle():
    """exp(log R) is R to below 1e-12 rad on every input of the device tests (both families, projected to rotations), the identity and
    the exact half-turns included; log never exceeds pi."""
    inp = inputs()
    R = ref.project(inp["R"])
    v = ref.log(R)
    assert np.isfinite(v).all() and np.linalg.norm(v, axis=-1).max() <= np.pi * (1 + 1e-15)
    err = ref.geodesic(ref.exp(v), R)
    for b, name in enumerate(inp["names"]):
        print("round trip %-12s %.2e rad" % (name, err[inp["band"] == b].max()))
    assert err.max() < 1e-12
    one = inp["band"] == inp["names"].index("identity")
    assert np.array_equal(v[one], np.zeros((1, 3))) and np.array_equal(ref.exp(np.zeros(3)), np.eye(3))
    # the angle that went in comes out: to the input's fp32 rounding for the axis-angle family
    for th, name in zip(ref.ANGLES, ref.ANGLE_NAMES):
        got = np.linalg.norm(v[inp["band"] == inp["names"].index(name)], axis=-1)
        assert np.abs(got - th).max() < 2e-7, (name, np.abs(got - th).max())


def test_inputs_are_what_the_device_tests_assume():
    """fp32, the product family off the rotation group by a few 1e-7 and no more, the exact cases exact, and the two-valued rows (w = 0
    exactly at theta = pi) exactly the constructed half-turns: at most 2 % of the inputs."""
    inp = inputs()
    R, band, names = inp["R"], inp["band"], inp["names"]
    assert R.dtype == np.float32 and len(R) == 2 * len(ref.ANGLES) * ref.PER_ANGLE + 1 + ref.N_EXACT_PI
    off = np.abs(ref.T(R.astype(np.float64)) @ R.astype(np.float64) - np.eye(3)).max((-1, -2))
    product = np.array([n.startswith("ABC") for n in names])[band]
    assert off[~product].max() < 2.5e-7 and 5e-8 < off[product].max() < 1.5e-6
    pi = band == names.index("exact pi")
    assert np.array_equal(R[pi], ref.T(R[pi])) and np.array_equal(R[pi][0], np.diag([1, -1, -1]).astype(np.float32))
    assert np.array_equal(R[band == names.index("identity")][0], np.eye(3, dtype=np.float32))
    two = ref.two_valued(R)
    assert np.array_equal(two, pi) and two.mean() <= 0.02
    # off the exact half-turns w decides the sign with a margin: the closest band keeps |w| above the fp32 noise of the inputs
    _, s, _ = ref.sin_cos_parts(ref.project(R))
    for name in ("pi-1e-6", "ABC pi-1e-6"):
        assert s[band == names.index(name)].min() > 3e-7, (name, s[band == names.index(name)].min())


def test_agrees_with_the_reference_shaped_oracle_where_that_is_defined():
    """log and exp against orc.log_so3 / orc.exp_so3 in float64, to 1e-9, on rotations the existing masks keep (|cos theta -+ 1| >= 1e-2)."""
    rng = np.random.default_rng(1)
    v = ref.axes(4096, rng) * rng.uniform(0.15, np.pi - 0.15, (4096, 1))
    R = ref.exp(v)
    cos = (np.trace(R, axis1=-2, axis2=-1) - 1) / 2
    assert (np.abs(cos - 1) >= 1e-2).all() and (np.abs(cos + 1) >= 1e-2).all() and (cos < ref.NEAR_PI_COS).sum() > 100
    Rt, vt = torch.from_numpy(R), torch.from_numpy(v)
    assert np.abs(ref.hat(ref.log(R)) - orc.log_so3(Rt).numpy()).max() < 1e-9
    assert np.abs(ref.log(R) - v).max() < 1e-9
    assert np.abs(R - orc.exp_so3(orc.hat(vt)).numpy()).max() < 1e-9
    k = rng.uniform(0, 1, 4096)
    assert np.abs(ref.scale(R, k) - orc.scale_rot(Rt, torch.from_numpy(k)).numpy()).max() < 1e-9


def test_exp_head_vjp_against_central_differences():
    """d / d v of <G0, O_t exp(hat(v))> by central differences in float64 (h = 1e-6: truncation 1e-12, rounding 1e-10 of |G0|), at the
    |v| of the device test and across both series thresholds."""
    rng = np.random.default_rng(2)
    n = 64
    O_t = ref.exp(rng.standard_normal((n, 3)))
    G0 = rng.standard_normal((n, 3, 3))
    h = 1e-6
    for mag in (0.0, 1e-6, 1e-4, 3e-4, 1e-3, 0.999e-2, 1.001e-2, 0.1, 1.0, 3.0):
        v = ref.axes(n, rng) * mag
        got = ref.exp_head_vjp(v, O_t, G0)
        fd = np.zeros_like(v)
        for k in range(3):
            d = np.zeros(3)
            d[k] = h
            fd[:, k] = ((G0 * (O_t @ ref.exp(v + d))).sum((-1, -2)) - (G0 * (O_t @ ref.exp(v - d))).sum((-1, -2))) / (2 * h)
        assert np.isfinite(got).all() and np.abs(got - fd).max() < 1e-8 * np.abs(fd).max(), (mag, np.abs(got - fd).max())
    # the limit at v = 0 in closed form: d E / d v_k = hat(e_k)
    G = ref.T(O_t) @ G0
    assert np.allclose(ref.exp_head_vjp(np.zeros((n, 3)), O_t, G0), ref.vee(G - ref.T(G)), rtol=0, atol=1e-14)
