// cluster_kernels.hip - the designs of a patch grouped into families on the device: diffab_metrics_cluster, the
// Daura / GROMOS neighbour-count clustering of a pairwise matrix at a cutoff.  The rule is the header comment of the entry in
// include/diffab_hip_cluster.h.
//
// Built with -ffp-contract=off like the other defined numbers (csrc/Makefile), although nothing here rounds: the only floating-point
// operations are the compare dist <= cutoff and the NaN test of a score (two scores are compared through their order-preserving bit
// patterns, inside the arg-max key).  Everything else is integer work on the adjacency bits: ballots, ANDs, popcounts, adds.  VALU + LDS only; no atomics; every value reaches memory through plain C++ stores.
#include <climits>
#include <cmath>

#include "../../include/diffab_hip_cluster.h"
#include "analysis_common.h"

namespace diffab {
namespace {

constexpr int kMaxGroup = DIFFAB_METRICS_MAX_GROUP;
constexpr int kLdsMaxN = DIFFAB_METRICS_CLUSTER_LDS_MAX_N;
constexpr int kSegCols = 256;                                // columns of one threshold item: four ballots per row
constexpr int kSegChunks = kSegCols / 64;
constexpr int kRowsInFlight = 4;                             // rows of one item whose loads are issued together
constexpr int kMaxThreads = 1024;                            // of the cluster launch
constexpr int kMaxPerThread = kMaxGroup / kMaxThreads;       // designs a thread owns above 1024 designs
constexpr int kMaxWords = kMaxGroup / 32;                    // 32-bit words of one row of the largest patch

constexpr int pad64(int n) { return (n + 63) / 64 * 64; }
// LDS form: word w of design i at [w * (Np + 1) + i].  Designs run along the fastest axis, so "thread i reads word w of its own row" puts
// the lanes of a wave on consecutive banks; the odd stride also spreads the centre's row (word w at bank (w + centre) % 32).
constexpr size_t lds_bits_bytes(int Np) { return static_cast<size_t>(Np / 32) * (Np + 1) * 4; }
static_assert(kLdsMaxN % 64 == 0 && kLdsMaxN <= kMaxThreads, "the LDS form gives every design a thread of its own");
static_assert(lds_bits_bytes(kLdsMaxN) + 2 * kMaxWords * 4 + 1024 <= 160 * 1024, "the bits of the largest on-chip patch fit the LDS of a CU");

// Workspace of diffab_metrics_cluster (DIFFAB_METRICS_CLUSTER_WORKSPACE_BYTES covers the carves and their alignment).
struct ClusterWorkspace {
  uint32_t* bits;  // (G, W, Np): bit j % 32 of [g][j / 32][i] = adj(i, j)
  int32_t* part;   // (G, S, Np): candidate neighbours of row i inside column segment s
  size_t bytes;
};

ClusterWorkspace carve_cluster(void* base, int64_t G, int64_t N) {
  const int64_t Np = (N + 63) / 64 * 64, W = Np / 32, S = (N + kSegCols - 1) / kSegCols;
  Carver c(base);
  ClusterWorkspace ws;
  ws.bits = c.take<uint32_t>(static_cast<size_t>(G * W * Np));
  ws.part = c.take<int32_t>(static_cast<size_t>(G * S * Np));
  ws.bytes = c.bytes();
  return ws;
}

// ------------------------------------------------------------------ 1. threshold: the only pass over dist
// One wave per item = (patch, 64 rows, 256 columns).  Lane l reads column c0 + 64 k + l of a row, k = 0..3 (four coalesced 256-byte
// loads), the ballot of the compare is the 64-bit word of that row, and lane r keeps the words of row i0 + r: after the rows every lane
// stores the eight 32-bit words and the candidate count of its own row, coalesced along the designs.
__global__ void __launch_bounds__(64)
cluster_threshold_kernel(const float* __restrict__ dist, const float* __restrict__ cutoff, const uint8_t* __restrict__ candidates, int N, int Np,
                         int S, ClusterWorkspace ws) {
  const int lane = threadIdx.x;
  const int blocks = Np / 64, W = Np / 32;
  const int per_patch = blocks * S;
  const int64_t g = blockIdx.x / per_patch;
  const int rem = blockIdx.x % per_patch;
  const int i0 = (rem / S) * 64, s = rem % S, c0 = s * kSegCols;
  const float cut = cutoff[g];
  const float* D = dist + g * N * N;
  unsigned long long cand[kSegChunks], mine[kSegChunks];
#pragma unroll
  for (int k = 0; k < kSegChunks; ++k) {
    const int j = c0 + k * 64 + lane;
    cand[k] = __ballot(j < N && (candidates == nullptr || candidates[g * N + j] != 0));
    mine[k] = 0ull;
  }
  for (int r0 = 0; r0 < 64 && i0 + r0 < N; r0 += kRowsInFlight) {  // (uniform)
    float d[kRowsInFlight][kSegChunks];
#pragma unroll
    for (int q = 0; q < kRowsInFlight; ++q) {  // the loads of four rows first: sixteen in flight per lane
      const int i = i0 + r0 + q;
#pragma unroll
      for (int k = 0; k < kSegChunks; ++k) {
        const int j = c0 + k * 64 + lane;
        d[q][k] = i < N && j < N ? D[static_cast<int64_t>(i) * N + j] : NAN;  // (a NaN on either side compares false)
      }
    }
#pragma unroll
    for (int q = 0; q < kRowsInFlight; ++q) {
      const int r = r0 + q;
#pragma unroll
      for (int k = 0; k < kSegChunks; ++k) {
        const int j = c0 + k * 64 + lane;
        const unsigned long long b = __ballot((j == i0 + r && j < N) || d[q][k] <= cut);
        if (lane == r) mine[k] = b;
      }
    }
  }
  const int i = i0 + lane;  // (< Np: rows past N store zero words and a zero count)
  int n = 0;
#pragma unroll
  for (int k = 0; k < kSegChunks; ++k) {
    const int w = (c0 + k * 64) / 32;
    if (w >= W) break;  // (W is even: w + 1 < W too)
    ws.bits[(g * W + w) * Np + i] = static_cast<uint32_t>(mine[k]);
    ws.bits[(g * W + w + 1) * Np + i] = static_cast<uint32_t>(mine[k] >> 32);
    n += __popcll(mine[k] & cand[k]);
  }
  ws.part[(g * S + s) * Np + i] = n;
}

// ------------------------------------------------------------------ 2. cluster: one work-group per patch
// The arg-max key of an open design, one integer whose order IS the rule: the count (13 bits) above the score, above the index.  The score
// enters as the complement of its order-preserving bit pattern (the lower score is the larger key): NaN was made +inf and -0 is made +0
// first, so two scores compare equal as fp32 values exactly when these bits are equal.  The index enters as 4095 - i.  An open design
// counts itself, so its key is at least 2^44 and 0 stands for "none".
constexpr int kKeyIndexBits = 12, kKeyCountShift = 44;
static_assert((1 << kKeyIndexBits) == kMaxGroup, "the index field holds every design");

__device__ inline unsigned long long score_key(float v, int i) {  // the part of the key that never changes
  uint32_t u = __float_as_uint(v);
  if ((u << 1) == 0u) u = 0u;  // (-0 -> +0)
  u = (u & 0x80000000u) ? ~u : (u | 0x80000000u);  // ascending in v
  return (static_cast<unsigned long long>(~u) << kKeyIndexBits) | static_cast<unsigned long long>(kMaxGroup - 1 - i);
}

__device__ inline unsigned long long key_max(unsigned long long a, unsigned long long b) { return a > b ? a : b; }

__device__ inline unsigned long long shfl_xor64(unsigned long long k, int d) {
  const uint32_t lo = __shfl_xor(static_cast<uint32_t>(k), d, 64), hi = __shfl_xor(static_cast<uint32_t>(k >> 32), d, 64);
  return (static_cast<unsigned long long>(hi) << 32) | lo;
}

__device__ inline unsigned long long uniform64(unsigned long long v) {
  const uint32_t lo = __builtin_amdgcn_readfirstlane(static_cast<uint32_t>(v));
  const uint32_t hi = __builtin_amdgcn_readfirstlane(static_cast<uint32_t>(v >> 32));
  return (static_cast<unsigned long long>(hi) << 32) | lo;
}

// PER designs per thread (design tid + r * blockDim.x); kLds: the bit words of the patch live in LDS, else they are read from the workspace.
template <int PER, bool kLds>
__global__ void __launch_bounds__(kMaxThreads)
cluster_kernel(const float* __restrict__ dist, const float* __restrict__ score, const uint8_t* __restrict__ candidates, int N, int Np, int S, int M,
               ClusterWorkspace ws, int32_t* __restrict__ label, float* __restrict__ center_dist, int64_t* __restrict__ center,
               int32_t* __restrict__ size, int32_t* __restrict__ count, int32_t* __restrict__ n_unassigned) {
  extern __shared__ uint32_t s_bits[];  // kLds: (W, Np + 1)
  __shared__ uint32_t s_open[kMaxWords], s_member[kMaxWords];
  __shared__ unsigned long long s_nonzero[kMaxWords / 64];  // which member words are not zero
  __shared__ unsigned long long s_part[kMaxThreads / 64];
  static_assert(kMaxThreads / 64 == 16, "the second butterfly of the arg-max runs over 16 lanes");
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, T = blockDim.x, waves = T >> 6;
  const int W = Np / 32;
  const int64_t g = blockIdx.x;
  const uint32_t* gbits = ws.bits + g * W * Np;
  const int stride = kLds ? Np + 1 : Np;
  const uint32_t* bits = kLds ? s_bits : gbits;

  if (kLds) {
    for (int idx = tid; idx < W * Np; idx += T) s_bits[(idx / Np) * stride + idx % Np] = gbits[idx];
  }
  int n[PER], lab[PER], of[PER];  // running count, cluster, and that cluster's centre
  unsigned long long v[PER];      // score_key
  bool open[PER];
#pragma unroll
  for (int r = 0; r < PER; ++r) {
    const int c = tid + r * T;
    const bool valid = c < N;
    open[r] = valid && (candidates == nullptr || candidates[g * N + c] != 0);
    v[r] = 0ull;
    n[r] = 0;
    lab[r] = of[r] = -1;
    if (valid) {
      float sc = score != nullptr ? score[g * N + c] : 0.f;
      if (sc != sc) sc = INFINITY;  // a NaN score counts as +inf
      v[r] = score_key(sc, c);
      for (int s = 0; s < S; ++s) n[r] += ws.part[(g * S + s) * Np + c];
    }
    const unsigned long long o = __ballot(open[r]);
    const int base = r * T + wave * 64;
    if (lane == 0 && base < Np) {
      s_open[base / 32] = static_cast<uint32_t>(o);
      s_open[base / 32 + 1] = static_cast<uint32_t>(o >> 32);
    }
  }
  if (tid < kMaxWords / 64) s_nonzero[tid] = 0ull;
  __syncthreads();

  int made = 0;
  while (made < M) {
    unsigned long long best = 0ull;
#pragma unroll
    for (int r = 0; r < PER; ++r)
      if (open[r]) best = key_max(best, (static_cast<unsigned long long>(n[r]) << kKeyCountShift) | v[r]);
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) best = key_max(best, shfl_xor64(best, d));
    if (lane == 0) s_part[wave] = best;
    __syncthreads();
    best = (lane & 15) < waves ? s_part[lane & 15] : 0ull;  // (at most 16 partials: a second butterfly over 16 lanes, in every wave alike)
#pragma unroll
    for (int d = 8; d > 0; d >>= 1) best = key_max(best, shfl_xor64(best, d));
    if (best == 0ull) break;  // (uniform: every thread reduced the same partials)
    const int ctr = kMaxGroup - 1 - static_cast<int>(best & (kMaxGroup - 1));
    if (tid < kMaxWords) {  // (whole waves: 128 threads, or all 64 of the smallest group)
      uint32_t m = 0;
      if (tid < W) {
        m = bits[tid * stride + ctr] & s_open[tid];
        s_member[tid] = m;
        s_open[tid] &= ~m;
      }
      const unsigned long long nz = __ballot(m != 0);
      if (lane == 0) s_nonzero[wave] = nz;
    }
    __syncthreads();
    // (nothing goes to global memory inside the loop: a store, or the load of center_dist, would be waited for at the next barrier)
#pragma unroll
    for (int r = 0; r < PER; ++r) {
      const int c = tid + r * T;
      if (open[r] && ((s_member[c >> 5] >> (c & 31)) & 1u)) {
        open[r] = false;
        lab[r] = made;
        of[r] = ctr;  // (n[r] is frozen from here on: a centre keeps the count it was chosen with)
      }
    }
    for (int h = 0; h < kMaxWords / 64; ++h) {
      unsigned long long nz = uniform64(s_nonzero[h]);
      while (nz != 0ull) {  // (uniform)
        const int w = h * 64 + __builtin_ctzll(nz);
        nz &= nz - 1;
        const uint32_t m = s_member[w];
#pragma unroll
        for (int r = 0; r < PER; ++r)
          if (open[r]) n[r] -= __popc(bits[w * stride + tid + r * T] & m);
      }
    }
    ++made;
  }

  __syncthreads();
#pragma unroll
  for (int r = 0; r < PER; ++r) {
    const int c = tid + r * T;
    if (c >= N) continue;
    label[g * N + c] = lab[r];
    if (center_dist != nullptr) center_dist[g * N + c] = lab[r] < 0 ? NAN : of[r] == c ? 0.f : dist[(g * N + of[r]) * N + c];
    if (lab[r] >= 0 && of[r] == c) {
      center[g * M + lab[r]] = c;
      size[g * M + lab[r]] = n[r];  // the centre's own count IS the member count: the centre was open and adj(i, i) holds
    }
  }
  for (int p = made + tid; p < M; p += T) {
    center[g * M + p] = -1;
    size[g * M + p] = 0;
  }
  if (tid == 0) {
    count[g] = made;
    if (n_unassigned != nullptr) {
      int left = 0;
      for (int w = 0; w < W; ++w) left += __popc(s_open[w]);
      n_unassigned[g] = left;
    }
  }
}

}  // namespace
}  // namespace diffab

using namespace diffab;

extern "C" {

int diffab_metrics_cluster(const float* dist, const float* cutoff, const float* score, const uint8_t* candidates, int32_t G, int32_t N,
                           int32_t M, int32_t* label, float* center_dist, int64_t* center, int32_t* size, int32_t* count,
                           int32_t* n_unassigned, void* workspace, size_t workspace_bytes, void* stream) {
  StreamOrder order_(stream);
  const char* who = "metrics_cluster";
  if (!group_shape_ok(who, G, N)) return DIFFAB_ERR_ARG;
  DIFFAB_REQUIRE(M >= 0 && M <= N, DIFFAB_ERR_ARG, "%s: M = %d clusters outside [0, N = %d]", who, M, N);
  if (G == 0) return DIFFAB_OK;
  DIFFAB_REQUIRE(dist != nullptr && cutoff != nullptr, DIFFAB_ERR_ARG, "%s: null input", who);
  DIFFAB_REQUIRE(label != nullptr && count != nullptr && (M == 0 || (center != nullptr && size != nullptr)), DIFFAB_ERR_ARG,
                 "%s: null output", who);
  const ClusterWorkspace ws = carve_cluster(workspace, G, N);
  if (const int e = workspace_ok(who, workspace, 256, workspace_bytes, ws.bytes)) return e;
  const int Np = pad64(N), S = (N + kSegCols - 1) / kSegCols;
  const int64_t items = static_cast<int64_t>(G) * (Np / 64) * S;
  DIFFAB_REQUIRE(items <= INT_MAX, DIFFAB_ERR_UNSUPPORTED, "%s: G = %d groups of N = %d are more tiles than one launch holds", who, G, N);
  hipStream_t st = as_stream(stream);
  hipLaunchKernelGGL(cluster_threshold_kernel, dim3(static_cast<unsigned>(items)), dim3(64), 0, st, dist, cutoff, candidates, N, Np, S, ws);
  const int threads = Np < kMaxThreads ? Np : kMaxThreads;
  if (N <= kLdsMaxN) {  // the one place that selects the form
    const size_t lds = lds_bits_bytes(Np);
    if (lds > 64 * 1024)  // (above the default limit of a launch: 128 KiB at N = 1024, of the 160 KiB a CU has)
      DIFFAB_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(cluster_kernel<1, true>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                           static_cast<int>(lds_bits_bytes(kLdsMaxN))));
    hipLaunchKernelGGL((cluster_kernel<1, true>), dim3(G), dim3(threads), lds, st, dist, score, candidates, N, Np, S, M, ws, label, center_dist,
                       center, size, count, n_unassigned);
  } else {
    hipLaunchKernelGGL((cluster_kernel<kMaxPerThread, false>), dim3(G), dim3(threads), 0, st, dist, score, candidates, N, Np, S, M, ws, label,
                       center_dist, center, size, count, n_unassigned);
  }
  DIFFAB_LAUNCH_CHECK();
  return DIFFAB_OK;
}

}  // extern "C"
