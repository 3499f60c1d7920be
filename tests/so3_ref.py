"""An independent float64 statement of the SO(3) maps, for the rotation angles where the reference's formulation breaks down.

numpy only: no torch, no device, and nothing of oracle/diffab_oracle.py, whose log_so3 / exp_so3 mirror the reference (theta from acos
of the trace, theta / (2 sin theta), sin n / n) and are 0/0 at theta = 0 and lose the axis near theta = pi exactly as it does.  Here

  log   takes the angle from atan2(|w|, c), w = vee(R - R^T) / 2 = sin(theta) axis, c = (tr R - 1) / 2 = cos(theta), which is conditioned
        like one rounding at every angle, and near pi takes the axis from the symmetric part (R + R^T) / 2 - c I = (1 - cos theta) a a^T,
        whose largest column is a multiple of the axis with nothing cancelled; w only gives its sign;
  exp   is Rodrigues with sin n / n and (1 - cos n) / n^2 by their series below |v| = 1e-4 (and 2 sin^2(n / 2) / n^2 above).

Every function takes arrays with any leading dimensions.  Not a test module: tests/test_so3_edges_host.py checks it on the host,
tests/test_gpu_so3_edges.py holds the kernels to it.
"""
import numpy as np

SERIES = 1e-4        # |v| below which exp uses the series coefficients
SERIES_VJP = 1e-2    # |v| below which the derivative coefficients use theirs (they cancel two orders earlier)
NEAR_PI_COS = -0.9   # cos(theta) below which log takes the axis from the symmetric part
ANGLES = (1e-8, 1e-6, 1e-5, 1e-4, 3e-4, 1e-3, 1e-2, 0.1, 1.0, 2.0, np.pi - 0.1, np.pi - 1e-2, np.pi - 1e-3, np.pi - 1e-4, np.pi - 1e-6)
ANGLE_NAMES = ("1e-8", "1e-6", "1e-5", "1e-4", "3e-4", "1e-3", "1e-2", "0.1", "1.0", "2.0", "pi-0.1", "pi-1e-2", "pi-1e-3", "pi-1e-4",
               "pi-1e-6")
PER_ANGLE = 1024
N_EXACT_PI = 512
SPECIAL_AXES = np.array([[1, 0, 0], [0, 1, 0], [0, 0, 1], [1, 1, 1], [1, 1, -1], [1, -1, 1], [-1, 1, 1]], dtype=np.float64)


def T(M):
    return np.swapaxes(M, -1, -2)


def hat(v):
    v = np.asarray(v, dtype=np.float64)
    x, y, z = v[..., 0], v[..., 1], v[..., 2]
    o = np.zeros_like(x)
    return np.stack([np.stack([o, -z, y], -1), np.stack([z, o, -x], -1), np.stack([-y, x, o], -1)], -2)


def vee(S):
    return np.stack([S[..., 2, 1], S[..., 0, 2], S[..., 1, 0]], -1)


def project(R):
    """The nearest proper rotation (Frobenius norm): U diag(1, 1, det(U V^T)) V^T of the SVD.  The polar factor of a symmetric matrix is
    symmetric, so for an exactly symmetric input (the constructed theta = pi matrices, the identity) the SVD's 1e-16 asymmetry is
    removed: log sees w = 0 exactly there, as it does on the input itself."""
    R = np.asarray(R, dtype=np.float64)
    U, _, Vt = np.linalg.svd(R)
    d = np.ones(R.shape[:-1])
    d[..., 2] = np.sign(np.linalg.det(U @ Vt))
    Q = (U * d[..., None, :]) @ Vt
    sym = (R == T(R)).all((-1, -2))[..., None, None]
    return np.where(sym, 0.5 * (Q + T(Q)), Q)


def sin_cos_parts(R):
    """(w, |w|, c): w = vee(R - R^T) / 2 = sin(theta) axis and c = (tr R - 1) / 2 = cos(theta)."""
    R = np.asarray(R, dtype=np.float64)
    w = vee(R - T(R)) / 2
    return w, np.linalg.norm(w, axis=-1), (np.trace(R, axis1=-2, axis2=-1) - 1) / 2


def log(R):
    """The rotation vector theta * axis of a rotation matrix, theta in [0, pi].  At theta = pi exactly (w = 0) the two signs of the axis
    are the same rotation; the one whose largest-column component is positive is returned."""
    R = np.asarray(R, dtype=np.float64)
    w, s, c = sin_cos_parts(R)
    theta = np.arctan2(s, c)
    with np.errstate(divide="ignore", invalid="ignore"):
        away = np.where(s[..., None] > 0, w / s[..., None], 0.0)  # theta = 0: the zero vector
    M = (R + T(R)) / 2 - c[..., None, None] * np.eye(3)
    j = np.argmax(np.linalg.norm(M, axis=-2), axis=-1)
    col = np.take_along_axis(M, j[..., None, None], axis=-1)[..., 0]
    with np.errstate(divide="ignore", invalid="ignore"):
        near = col / np.linalg.norm(col, axis=-1, keepdims=True)
    near = near * np.where((col * w).sum(-1) < 0, -1.0, 1.0)[..., None]
    axis = np.where((c < NEAR_PI_COS)[..., None], near, away)
    return theta[..., None] * axis


def exp_coefficients(n):
    """a = sin n / n and b = (1 - cos n) / n^2."""
    n = np.asarray(n, dtype=np.float64)
    n2 = n * n
    safe = np.where(n < SERIES, 1.0, n)
    a = np.where(n < SERIES, 1 - n2 / 6 + n2 * n2 / 120, np.sin(safe) / safe)
    b = np.where(n < SERIES, 0.5 - n2 / 24 + n2 * n2 / 720, 2 * np.sin(safe / 2) ** 2 / (safe * safe))
    return a, b


def exp(v):
    """Rodrigues: I + a hat(v) + b hat(v)^2."""
    v = np.asarray(v, dtype=np.float64)
    a, b = exp_coefficients(np.linalg.norm(v, axis=-1))
    S = hat(v)
    return np.eye(3) + a[..., None, None] * S + b[..., None, None] * (S @ S)


def scale(R, k):
    """R^k = exp(k log(project R)); k broadcasts against R's leading dimensions."""
    return exp(np.asarray(k, dtype=np.float64)[..., None] * log(project(R)))


def geodesic(A, B):
    """The angle of A^T B, by the same atan2 form."""
    _, s, c = sin_cos_parts(T(np.asarray(A, dtype=np.float64)) @ np.asarray(B, dtype=np.float64))
    return np.arctan2(s, c)


def exp_head_vjp(v, O_t, G0):
    """d L / d v for O0 = O_t exp(hat(v)) and G0 = d L / d O0: what rotvec_head_bwd (csrc/noslp_kernels.hip) computes per row.
    With E = I + a S + b S^2 and G = O_t^T G0,  d E / d v_k = a hat(e_k) + b (hat(e_k) S + S hat(e_k)) + v_k (a'/n S + b'/n S^2);
    a'/n = (n cos n - sin n) / n^3 -> -1/3 and b'/n = (n sin n - 2 (1 - cos n)) / n^4 -> -1/12 by their series at small n."""
    v, O_t, G0 = (np.asarray(x, dtype=np.float64) for x in (v, O_t, G0))
    n = np.linalg.norm(v, axis=-1)
    n2 = n * n
    a, b = exp_coefficients(n)
    small = n < SERIES_VJP
    safe = np.where(small, 1.0, n)
    ca = np.where(small, -1 / 3 + n2 / 30 - n2**2 / 840 + n2**3 / 45360, (safe * np.cos(safe) - np.sin(safe)) / safe**3)
    cb = np.where(small, -1 / 12 + n2 / 180 - n2**2 / 6720 + n2**3 / 453600,
                  (safe * np.sin(safe) - 4 * np.sin(safe / 2) ** 2) / safe**4)
    S = hat(v)
    G = T(O_t) @ G0
    radial = ca[..., None, None] * S + cb[..., None, None] * (S @ S)
    out = []
    for k in range(3):
        Ek = hat(np.eye(3)[k])
        dE = a[..., None, None] * Ek + b[..., None, None] * (Ek @ S + S @ Ek) + v[..., k, None, None] * radial
        out.append((G * dE).sum((-1, -2)))
    return np.stack(out, -1)


# ---------------------------------------------------------------------- the inputs of both edge-test files
def axes(n, rng):
    """n unit axes: the three coordinate axes, the four body diagonals, the rest uniform on the sphere."""
    a = np.concatenate([SPECIAL_AXES, rng.standard_normal((n - len(SPECIAL_AXES), 3))])
    return a / np.linalg.norm(a, axis=-1, keepdims=True)


def axis_angle(a, theta):
    """cos(theta) I + (1 - cos theta) a a^T + sin(theta) hat(a) in float64; at theta = pi exactly 2 a a^T - I, an exactly symmetric
    matrix (a_i a_j commutes) that stays so when rounded to fp32."""
    aa = a[..., :, None] * a[..., None, :]
    if theta == np.pi:
        return 2 * aa - np.eye(3)
    return np.cos(theta) * np.eye(3) + (1 - np.cos(theta)) * aa + np.sin(theta) * hat(a)


def edge_inputs(seed=0):
    """fp32 inputs of the edge tests, as {"R": (N, 3, 3) float32, "band": (N,) int index into "names", "names": [...]}.

    Family "axis-angle": PER_ANGLE rotations per angle of ANGLES, built in float64 and rounded to fp32 (orthogonal to one rounding).
    Family "product": the same angles as A B C multiplied in fp32 from three fp32 rotations (A, B uniform, C = fp32((A B)^T R)), so the
    orthogonality error is a few 1e-7 and the trace can leave [-1, 3].  An fp32 product cannot be the identity or a half-turn exactly, so
    the two exact cases exist in the first family only: one identity, and N_EXACT_PI exactly symmetric half-turns."""
    rng = np.random.default_rng(seed)
    Rs, band, names = [], [], []
    for fam in ("axis-angle", "product"):
        for th, nm in zip(ANGLES, ANGLE_NAMES):
            R = axis_angle(axes(PER_ANGLE, rng), th)
            if fam == "product":
                A, B = (exp(rng.standard_normal((PER_ANGLE, 3))).astype(np.float32) for _ in range(2))
                C = (T(A.astype(np.float64) @ B.astype(np.float64)) @ R).astype(np.float32)
                R = np.matmul(np.matmul(A, B, dtype=np.float32), C, dtype=np.float32)
            Rs.append(R.astype(np.float32))
            band += [len(names)] * PER_ANGLE
            names.append(("" if fam == "axis-angle" else "ABC ") + nm)
    Rs.append(np.eye(3, dtype=np.float32)[None])
    band.append(len(names))
    names.append("identity")
    Rs.append(axis_angle(axes(N_EXACT_PI, rng), np.pi).astype(np.float32))
    band += [len(names)] * N_EXACT_PI
    names.append("exact pi")
    return {"R": np.concatenate(Rs), "band": np.array(band), "names": names}


def two_valued(R):
    """Rows whose R^k has two values for k outside {0, 1}: half-turns with w = 0 exactly (project keeps the constructed ones so)."""
    _, s, c = sin_cos_parts(project(R))
    return (s == 0) & (c < 0)
