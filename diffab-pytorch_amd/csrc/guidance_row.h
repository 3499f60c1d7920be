// guidance_row.h - the pass of the clash / chain-bond potential over one state row, shared by the guidance
// kernels (diffusion_kernels.hip) and the steering energy (steering_kernels.hip, section 4.14).  Include it from a translation unit
// built with -ffp-contract=off: the sums are defined numbers.
#pragma once
#include "common.h"
#include "denoiser_internal.h"

namespace diffab {

// ------------------------------------------------------------------ structure guidance
// One work-group of four waves per state row.  The row is staged in LDS tiles of kGuideThreads residues: p (x0_hat of a generated
// residue, x of any other) with a flag word in .w (bit 0 residue_mask, bit 1 generated; 0 past the end of a ragged row) in one float4,
// chain and residue_idx in one int2.  Lane l of every wave owns residue i0 + l of each chunk of 64 residues; wave w scans the w-th
// quarter of every tile's partners in order - all lanes read the same LDS address, a broadcast - and the four partial gradients of a
// residue are added in wave order through LDS.  A wave whose 64 owners have nothing to compute skips the scan.  Sums run in that fixed
// order, then in a fixed tree: no atomics, the result of a row depends on the row alone.  Plain fp32 VALU / LDS code (this file is
// built with -ffp-contract=off).
constexpr int kGuideThreads = 256, kGuideWaves = kGuideThreads / 64;

struct GuideSums {
  float clash = 0.f, bond = 0.f, max_dev = 0.f;
  int n_clash = 0;
};

// p of residue i: x0_hat_i = (x_t,i - sqrt(1 - abar_t) eps_hat_i) / sqrt(abar_t) for a generated residue - record_residue's expression,
// so the recorded pred_x is bitwise the point the potential is taken at - and x_i otherwise (eps_hat == nullptr: x for every residue)
__device__ inline float3 guide_point(const float* x, const float* eps_hat, int64_t i, bool gen, float omabs, float a) {
  if (eps_hat != nullptr && gen)
    return make_float3((x[i * 3 + 0] - omabs * eps_hat[i * 3 + 0]) / a, (x[i * 3 + 1] - omabs * eps_hat[i * 3 + 1]) / a,
                       (x[i * 3 + 2] - omabs * eps_hat[i * 3 + 2]) / a);
  return make_float3(x[i * 3 + 0], x[i * 3 + 1], x[i * 3 + 2]);
}

// The pass over one row: g_i for every residue, handed to emit(i, gx, gy, gz) by wave 0 (0 unless generated and masked).  kEnergy:
// every masked residue also scans, and the unordered pairs {i, j} are counted by their smaller index into `sums`.
template <bool kEnergy, typename Emit>
__device__ inline void guide_row(int64_t row, int K, const float* __restrict__ x, const float* __restrict__ eps_hat, float omabs, float a,
                                 const uint8_t* __restrict__ gm, const GuidanceDev& g, GuideSums& sums, Emit emit) {
  __shared__ float4 tp[kGuideThreads];
  __shared__ int2 tc[kGuideThreads];
  __shared__ float part[kGuideWaves][3][64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t base = row * K;
  // a nonbonded pair whose d^2 is not below d0^2 (with a margin over its rounding) cannot clash: skipped before the square root
  const float d0 = g.clash_distance, L = g.bond_length, wc2 = 2.0f * g.w_clash, wb2 = 2.0f * g.w_bond, far2 = d0 * d0 * 1.0001f;
  for (int i0 = 0; i0 < K; i0 += 64) {
    const int i = i0 + lane;
    int fi = 0, ci = 0, ri = 0;
    float3 pi = make_float3(0.f, 0.f, 0.f);
    if (i < K) {
      const bool gen = gm[base + i] != 0;
      fi = (g.residue_mask == nullptr || g.residue_mask[base + i] ? 1 : 0) | (gen ? 2 : 0);
      pi = guide_point(x, eps_hat, base + i, gen, omabs, a);
      ci = g.chain[base + i];
      ri = g.residue_idx[base + i];
    }
    const bool run = kEnergy ? (fi & 1) != 0 : fi == 3;
    float gx = 0.f, gy = 0.f, gz = 0.f;
    for (int j0 = 0; j0 < K; j0 += kGuideThreads) {
      __syncthreads();  // every wave is done with the previous tile
      const int j = j0 + tid;
      if (j < K) {
        const bool gen = gm[base + j] != 0;
        const int fj = (g.residue_mask == nullptr || g.residue_mask[base + j] ? 1 : 0) | (gen ? 2 : 0);
        const float3 pj = guide_point(x, eps_hat, base + j, gen, omabs, a);
        tp[tid] = make_float4(pj.x, pj.y, pj.z, static_cast<float>(fj));
        tc[tid] = make_int2(g.chain[base + j], g.residue_idx[base + j]);
      } else {
        tp[tid] = make_float4(0.f, 0.f, 0.f, 0.f);
        tc[tid] = make_int2(0, 0);
      }
      __syncthreads();
      if (!run) continue;
      const int n = min(kGuideThreads, K - j0), lo = n * wave / kGuideWaves, hi = n * (wave + 1) / kGuideWaves;
#pragma unroll 4
      for (int jj = lo; jj < hi; ++jj) {
        const float4 q = tp[jj];
        const int fj = static_cast<int>(q.w);
        if (!(fj & 1) || !((fi | fj) & 2) || j0 + jj == i) continue;
        const int2 c = tc[jj];
        const float dx = pi.x - q.x, dy = pi.y - q.y, dz = pi.z - q.z;
        const float d2 = dx * dx + dy * dy + dz * dz;
        const int64_t gap = static_cast<int64_t>(c.y) - ri;
        const bool bonded = c.x == ci && (gap == 1 || gap == -1);
        if (!bonded && !(d2 < far2)) continue;
        const float d = sqrtf(d2);
        const bool counted = kEnergy && j0 + jj > i;
        float coef;
        if (bonded) {
          const float dev = d - L;
          coef = wb2 * dev;
          if (counted) {
            sums.bond += dev * dev;
            sums.max_dev = fmaxf(sums.max_dev, fabsf(dev));
          }
        } else {
          if (!(d < d0)) continue;
          const float h = d0 - d;
          coef = -wc2 * h;
          if (counted) {
            sums.clash += h * h;
            sums.n_clash += 1;
          }
        }
        if ((fi & 2) && d >= 1e-6f) {
          const float sc = coef / d;
          gx += sc * dx;
          gy += sc * dy;
          gz += sc * dz;
        }
      }
    }
    part[wave][0][lane] = gx;
    part[wave][1][lane] = gy;
    part[wave][2][lane] = gz;
    __syncthreads();  // (part is next written after the next chunk's first tile barrier)
    if (wave == 0 && i < K) {
      float sx = part[0][0][lane], sy = part[0][1][lane], sz = part[0][2][lane];
#pragma unroll
      for (int w = 1; w < kGuideWaves; ++w) {
        sx += part[w][0][lane];
        sy += part[w][1][lane];
        sz += part[w][2][lane];
      }
      emit(base + i, sx, sy, sz);
    }
  }
}

// The row's sums over the work-group, in a fixed tree: every thread's partial sums in, the row's totals out (valid in thread 0).
__device__ inline void guide_reduce(GuideSums& sums) {
  __shared__ float red[3][kGuideThreads];
  __shared__ int red_n[kGuideThreads];
  const int tid = threadIdx.x;
  red[0][tid] = sums.clash;
  red[1][tid] = sums.bond;
  red[2][tid] = sums.max_dev;
  red_n[tid] = sums.n_clash;
  __syncthreads();
  for (int s = kGuideThreads / 2; s > 0; s >>= 1) {
    if (tid < s) {
      red[0][tid] += red[0][tid + s];
      red[1][tid] += red[1][tid + s];
      red[2][tid] = fmaxf(red[2][tid], red[2][tid + s]);
      red_n[tid] += red_n[tid + s];
    }
    __syncthreads();
  }
  if (tid == 0) {
    sums.clash = red[0][0];
    sums.bond = red[1][0];
    sums.max_dev = red[2][0];
    sums.n_clash = red_n[0];
  }
}

}  // namespace diffab
