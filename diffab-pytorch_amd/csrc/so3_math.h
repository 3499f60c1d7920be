// so3_math.h - 3x3 rotation helpers (row-major float[9]).
// The maps are the reference's (log: so3.py:146-162, exp: so3.py:219-237, hat/vee: so3.py:165-204) in a form that is defined and
// accurate at every rotation angle, which the reference's is not ("SO(3) maps at theta near 0 and pi"):
//   log : theta = atan2(|w|, c) with w = vee(R - R^T) / 2 = sin(theta) axis and c = (tr R - 1) / 2, not acos(c); theta / (2 sin theta) by
//         its series at small |w|; for c < kSo3NearPiCos the axis from the symmetric part, (R + R^T) / 2 - c I = (1 - c) a a^T, and only
//         its sign from w.  log(I) = 0; at theta = pi exactly (w = 0) the axis whose largest component is positive.
//   exp : sin n / n and (1 - cos n) / n^2 by their series for n^2 < kSo3Series; from there on the reference's expression in the
//         reference's operation order, so those results are the same bits as before.  exp(0) = I.
// No input gives a non-finite output unless it holds one.  Everything branches on values in registers; there is no indexed access to
// the matrices, so nothing goes to scratch.
#pragma once
#include <hip/hip_runtime.h>

namespace diffab {

constexpr float kSo3Series = 1e-4f;     // n^2 (or |w|^2) below which the two-term series are exact to fp32 (next term < 1e-9)
constexpr float kSo3NearPiCos = -0.5f;  // cos(theta) below which log takes the axis from the symmetric part

__device__ inline void mat3_mul(const float* a, const float* b, float* c) {
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) c[i * 3 + j] = a[i * 3 + 0] * b[0 * 3 + j] + a[i * 3 + 1] * b[1 * 3 + j] + a[i * 3 + 2] * b[2 * 3 + j];
}

__device__ inline void so3_hat(float x, float y, float z, float* S) {
  S[0] = 0.0f; S[1] = -z;   S[2] = y;
  S[3] = z;    S[4] = 0.0f; S[5] = -x;
  S[6] = -y;   S[7] = x;    S[8] = 0.0f;
}

// a = sin n / n and b = (1 - cos n) / n^2 for n^2 < kSo3Series
__device__ inline void so3_exp_series(float n2, float& a, float& b) {
  a = 1.0f - n2 * (1.0f / 6.0f);
  b = 0.5f - n2 * (1.0f / 24.0f);
}

// S = log R, skew-symmetric; vee(S) = theta axis, theta in [0, pi]
__device__ inline void so3_log(const float* R, float* S) {
  const float tr = (R[0] + R[4]) + R[8];
  const float c = (tr - 1.0f) / 2.0f;
  const float wx = 0.5f * (R[7] - R[5]), wy = 0.5f * (R[2] - R[6]), wz = 0.5f * (R[3] - R[1]);
  const float s2 = wx * wx + wy * wy + wz * wz;
  const float s = sqrtf(s2);
  const float theta = atan2f(s, c);
  if (c >= kSo3NearPiCos) {
    // theta / (2 sin theta) (R - R^T), sin theta = |w|;  theta / sin theta = 1 + s^2 / 6 + ... at small s
    const float f = s2 < kSo3Series ? 0.5f + s2 * (1.0f / 12.0f) : theta / (2.0f * s);
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
      for (int j = 0; j < 3; ++j) S[i * 3 + j] = f * (R[i * 3 + j] - R[j * 3 + i]);
    return;
  }
  // M = (R + R^T) / 2 - c I = (1 - c) a a^T: the column of the largest diagonal entry is (1 - c) a_j a, with |a_j| >= 1 / sqrt(3)
  const float d0 = R[0] - c, d1 = R[4] - c, d2 = R[8] - c;
  const float m01 = 0.5f * (R[1] + R[3]), m02 = 0.5f * (R[2] + R[6]), m12 = 0.5f * (R[5] + R[7]);
  const bool p0 = d0 >= d1 && d0 >= d2, p1 = !p0 && d1 >= d2;
  float ax = p0 ? d0 : (p1 ? m01 : m02);
  float ay = p0 ? m01 : (p1 ? d1 : m12);
  float az = p0 ? m02 : (p1 ? m12 : d2);
  const float len = sqrtf(ax * ax + ay * ay + az * az);
  float g = len > 0.0f ? theta / len : 0.0f;  // (a matrix that is no rotation can have M = 0)
  if (ax * wx + ay * wy + az * wz < 0.0f) g = -g;
  so3_hat(g * ax, g * ay, g * az, S);
}

// R = I + S sin(n)/n + S^2 (1 - cos n)/n^2,  n = |(S21, S02, S10)|
__device__ inline void so3_exp(const float* S, float* R) {
  const float vx = S[7], vy = S[2], vz = S[3];
  const float n2 = vx * vx + vy * vy + vz * vz;
  float S2[9];
  mat3_mul(S, S, S2);
  if (n2 < kSo3Series) {
    float a, b;
    so3_exp_series(n2, a, b);
#pragma unroll
    for (int i = 0; i < 9; ++i) {
      const float eye = (i == 0 || i == 4 || i == 8) ? 1.0f : 0.0f;
      R[i] = (eye + S[i] * a) + S2[i] * b;
    }
    return;
  }
  const float n = sqrtf(n2);
  float sn, cn;
  sincosf(n, &sn, &cn);
  const float nn = n * n;
#pragma unroll
  for (int i = 0; i < 9; ++i) {
    const float eye = (i == 0 || i == 4 || i == 8) ? 1.0f : 0.0f;
    R[i] = (eye + S[i] * sn / n) + S2[i] * (1.0f - cn) / nn;
  }
}

__device__ inline void so3_rotvec_to_matrix(float x, float y, float z, float* R) {
  float S[9];
  so3_hat(x, y, z, S);
  so3_exp(S, R);
}

// exp(k log R)
__device__ inline void so3_scale(const float* R, float k, float* out) {
  float S[9];
  so3_log(R, S);
#pragma unroll
  for (int i = 0; i < 9; ++i) S[i] *= k;
  so3_exp(S, out);
}

}  // namespace diffab
