// pareto_kernels.hip - the designs of a patch ranked into non-dominated fronts on the device: diffab_metrics_pareto,
// Pareto ranking of N designs over M objectives with Deb's constrained domination.  The rule is the header comment of the entry in
// include/diffab_hip_cluster.h.
//
// Built with -ffp-contract=off like the other defined numbers (csrc/Makefile), although nothing here rounds: the only floating-point
// operations are fp32 compares of stored values (after a sign-bit flip for a maximised objective and NaN -> +inf); scores are compared
// through their order-preserving bit patterns.  Everything else is integer work: ballots, ANDs, popcounts, adds.  The layouts are those of
// csrc/cluster_kernels.hip, whose measurements chose them.  VALU + LDS only; the one atomic is an LDS integer add of
// wave counts after the loop; every value reaches memory through plain C++ stores.
#include <climits>
#include <cmath>

#include "../../include/diffab_hip_cluster.h"
#include "analysis_common.h"

namespace diffab {
namespace {

constexpr int kMaxGroup = DIFFAB_METRICS_MAX_GROUP;
constexpr int kLdsMaxN = DIFFAB_METRICS_CLUSTER_LDS_MAX_N;
constexpr int kMaxObjectives = DIFFAB_METRICS_PARETO_MAX_OBJECTIVES;
constexpr int kSegCols = 256;                           // designs i of one dominance item: four ballots per design j
constexpr int kSegChunks = kSegCols / 64;
constexpr int kTile = 64 + kSegCols;                    // key rows staged per item: 64 designs j, then 256 designs i
constexpr int kRowsInFlight = 4;                        // designs j compared per pass over the objectives
constexpr int kStageSteps = 4;                          // loads of the key staging issued together
constexpr int kMaxThreads = 1024;                       // of the peel launch
constexpr int kMaxPerThread = kMaxGroup / kMaxThreads;  // designs a thread owns above 1024 designs
constexpr int kMaxWords = kMaxGroup / 32;               // 32-bit words of one row of the largest patch
constexpr int kWordsInFlight = 4;                       // member words of one step of the peel loop's popcount pass
static_assert(64 % kWordsInFlight == 0, "a group of member words lies inside one 64-bit mask of non-zero words");

constexpr int pad64(int n) { return (n + 63) / 64 * 64; }
// LDS form of the bits: word w of design j at [w * (Np + 1) + j], as the cluster launch keeps them (designs on the fastest axis).
constexpr size_t lds_bits_bytes(int Np) { return static_cast<size_t>(Np / 32) * (Np + 1) * 4; }
// The sort keys of `order`, written over the bits after the loop: a 64-bit word per design.
constexpr size_t lds_keys_bytes(int Np) { return static_cast<size_t>(Np) * 8; }
constexpr size_t lds_peel_bytes(int Np, bool lds_form) {
  return lds_form && lds_bits_bytes(Np) > lds_keys_bytes(Np) ? lds_bits_bytes(Np) : lds_keys_bytes(Np);
}
static_assert(kLdsMaxN % 64 == 0 && kLdsMaxN <= kMaxThreads, "the LDS form gives every design a thread of its own");
static_assert(lds_peel_bytes(kLdsMaxN, true) + 2 * kMaxWords * 4 + 1024 <= 160 * 1024, "the bits of the largest on-chip patch fit the LDS of a CU");
static_assert(lds_peel_bytes(kMaxGroup, false) <= 64 * 1024, "the keys of the largest patch fit a launch's default LDS limit");
static_assert((kMaxObjectives + 1) * kTile * 4 <= 64 * 1024, "the key rows of a dominance item fit a launch's default LDS limit");

// Workspace of diffab_metrics_pareto (DIFFAB_METRICS_PARETO_WORKSPACE_BYTES covers the carves and their alignment).
struct ParetoWorkspace {
  uint32_t* bits;  // (G, W, Np): bit i % 32 of [g][i / 32][j] = dom(i, j)
  int32_t* by;     // (G, S, Np): dominators of j among the designs of segment s
  int32_t* of;     // (G, B, Np): designs that i dominates among the 64 designs of row tile b
  size_t bytes;
};

ParetoWorkspace carve_pareto(void* base, int64_t G, int64_t N) {
  const int64_t Np = (N + 63) / 64 * 64, W = Np / 32, S = (N + kSegCols - 1) / kSegCols, B = Np / 64;
  Carver c(base);
  ParetoWorkspace ws;
  ws.bits = c.take<uint32_t>(static_cast<size_t>(G * W * Np));
  ws.by = c.take<int32_t>(static_cast<size_t>(G * S * Np));
  ws.of = c.take<int32_t>(static_cast<size_t>(G * B * Np));
  ws.bytes = c.bytes();
  return ws;
}

// ------------------------------------------------------------------ 1. dominance: the only pass over the objectives
// One wave per item = (patch, 64 designs j, 256 designs i).  The 320 key rows are staged objective-major in LDS with the rule's
// transformations applied once: v = the stored value, its sign bit flipped where the objective is maximised, a NaN made +inf; w = the
// violation, a NaN made +inf and everything <= 0 made +0.  A design that is no candidate (or lies past N) gets w = NaN: every compare
// with it is false, so it neither dominates nor is dominated, and no candidate test is left in the pair loop.  i != j needs no test
// either: a design does not dominate a vector equal to its own.  Lane l owns design i = c0 + 64 k + l, k = 0..3; the ballot of dom(i, j)
// is the 64-bit word of j's dominators and lane r keeps the words of design j0 + r, as the cluster threshold launch does.
__global__ void __launch_bounds__(64)
pareto_dominance_kernel(const float* __restrict__ objectives, const uint8_t* __restrict__ maximize, const float* __restrict__ violation,
                        const uint8_t* __restrict__ candidates, int N, int Np, int S, int M, ParetoWorkspace ws) {
  extern __shared__ float s_key[];  // (M, kTile): objective m of staged design d at [m * kTile + d]
  __shared__ float s_w[kTile];
  const int lane = threadIdx.x;
  const int blocks = Np / 64, W = Np / 32;
  const int per_patch = blocks * S;
  const int64_t g = blockIdx.x / per_patch;
  const int rem = blockIdx.x % per_patch;
  const int b = rem / S, j0 = b * 64, s = rem % S, c0 = s * kSegCols;

  for (int d = lane; d < kTile; d += 64) {
    const int c = d < 64 ? j0 + d : c0 + d - 64;
    float w = NAN;
    if (c < N && (candidates == nullptr || candidates[g * N + c] != 0)) {
      w = violation != nullptr ? violation[g * N + c] : 0.f;
      if (w != w) w = INFINITY;
      if (w <= 0.f) w = 0.f;
    }
    s_w[d] = w;
  }
  // Element idx = d * M + m of the staged rows goes to lane idx % 64: both runs of rows are contiguous in memory, so these are coalesced
  // dword loads.  (d, m) advance by 64 elements per step without a division, and the loads of four steps are issued before their stores.
  const int dq = 64 / M, dr = 64 % M;
  int d = lane / M, m = lane % M;
  for (int idx0 = 0; idx0 < kTile * M; idx0 += 64 * kStageSteps) {  // (uniform)
    uint32_t u[kStageSteps];
    int at[kStageSteps];
#pragma unroll
    for (int t = 0; t < kStageSteps; ++t) {
      const int c = d < 64 ? j0 + d : c0 + d - 64;
      at[t] = d < kTile ? m * kTile + d : -1;
      u[t] = 0x7f800000u;  // +inf
      if (d < kTile && c < N) {
        u[t] = __float_as_uint(objectives[(g * N + c) * M + m]);
        if (maximize != nullptr && maximize[m] != 0) u[t] ^= 0x80000000u;
      }
      d += dq;
      m += dr;
      if (m >= M) {
        m -= M;
        ++d;
      }
    }
#pragma unroll
    for (int t = 0; t < kStageSteps; ++t) {
      float v = __uint_as_float(u[t]);
      if (v != v) v = INFINITY;
      if (at[t] >= 0) s_key[at[t]] = v;
    }
  }
  __syncthreads();

  float wi[kSegChunks];
  unsigned long long mine[kSegChunks];
  int of[kSegChunks];
#pragma unroll
  for (int k = 0; k < kSegChunks; ++k) {
    wi[k] = s_w[64 + k * 64 + lane];
    mine[k] = 0ull;
    of[k] = 0;
  }
  for (int r0 = 0; r0 < 64 && j0 + r0 < N; r0 += kRowsInFlight) {  // (uniform)
    // (per pair the number of objectives with v(i) <= v(j) and with v(i) < v(j): integer counters in vector registers - thirty-two
    // lane masks would not fit the scalar registers)
    int le[kRowsInFlight][kSegChunks], lt[kRowsInFlight][kSegChunks];
#pragma unroll
    for (int q = 0; q < kRowsInFlight; ++q)
#pragma unroll
      for (int k = 0; k < kSegChunks; ++k) le[q][k] = lt[q][k] = 0;
    for (int m = 0; m < M; ++m) {
      const float* km = s_key + m * kTile;
      float vj[kRowsInFlight], vi[kSegChunks];
#pragma unroll
      for (int q = 0; q < kRowsInFlight; ++q) vj[q] = km[r0 + q];  // (a broadcast)
#pragma unroll
      for (int k = 0; k < kSegChunks; ++k) vi[k] = km[64 + k * 64 + lane];
#pragma unroll
      for (int q = 0; q < kRowsInFlight; ++q)
#pragma unroll
        for (int k = 0; k < kSegChunks; ++k) {
          le[q][k] += vi[k] <= vj[q] ? 1 : 0;
          lt[q][k] += vi[k] < vj[q] ? 1 : 0;
        }
    }
#pragma unroll
    for (int q = 0; q < kRowsInFlight; ++q) {
      const float wj = s_w[r0 + q];
#pragma unroll
      for (int k = 0; k < kSegChunks; ++k) {
        const bool dom = wi[k] < wj || (wi[k] == wj && le[q][k] == M && lt[q][k] > 0);
        const unsigned long long bal = __ballot(dom);
        if (lane == r0 + q) mine[k] = bal;
        of[k] += dom ? 1 : 0;
      }
    }
  }
  const int j = j0 + lane;  // (< Np: designs past N store zero words and zero counts)
  int by = 0;
#pragma unroll
  for (int k = 0; k < kSegChunks; ++k) {
    const int i = c0 + k * 64;
    if (i >= Np) break;  // (uniform; W is even: both words of the chunk exist)
    const int w = i / 32;
    ws.bits[(g * W + w) * Np + j] = static_cast<uint32_t>(mine[k]);
    ws.bits[(g * W + w + 1) * Np + j] = static_cast<uint32_t>(mine[k] >> 32);
    by += __popcll(mine[k]);
    ws.of[(g * blocks + b) * Np + i + lane] = of[k];
  }
  ws.by[(g * S + s) * Np + j] = by;
}

// ------------------------------------------------------------------ 2. peel: one work-group per patch
constexpr int kKeyScoreShift = 12, kKeyClassShift = 44;  // n_dominated below the score below the class
static_assert((1 << kKeyScoreShift) == kMaxGroup, "the lowest field holds kMaxGroup - 1 - n_dominated");

__device__ inline uint32_t score_bits(float v) {  // ascending in v as an unsigned integer; equal fp32 values have equal bits
  if (v != v) v = INFINITY;                       // a NaN score counts as +inf
  uint32_t u = __float_as_uint(v);
  if ((u << 1) == 0u) u = 0u;  // (-0 -> +0)
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// PER designs per thread (design tid + r * blockDim.x); kLds: the bit words of the patch live in LDS, else they are read from the workspace.
template <int PER, bool kLds>
__global__ void __launch_bounds__(kMaxThreads)
pareto_peel_kernel(const float* __restrict__ score, const uint8_t* __restrict__ candidates, int N, int Np, int S, int F, ParetoWorkspace ws,
                   int32_t* __restrict__ rank, int32_t* __restrict__ n_dominators, int32_t* __restrict__ n_dominated,
                   int32_t* __restrict__ front_size, int32_t* __restrict__ count, int32_t* __restrict__ n_unranked,
                   int64_t* __restrict__ order) {
  extern __shared__ unsigned long long s_dyn[];  // kLds: the bits (W, Np + 1) during the loop; the keys of `order` after it
  __shared__ uint32_t s_member[2][kMaxWords];    // (two buffers: a fast wave writes the next front's words while a slow one reads this one's)
  __shared__ int s_left;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, T = blockDim.x;
  const int W = Np / 32, B = Np / 64;
  const int64_t g = blockIdx.x;
  const uint32_t* gbits = ws.bits + g * W * Np;
  uint32_t* s_bits = reinterpret_cast<uint32_t*>(s_dyn);
  const int stride = kLds ? Np + 1 : Np;
  const uint32_t* bits = kLds ? s_bits : gbits;

  if (kLds) {
    for (int idx = tid; idx < W * Np; idx += T) s_bits[(idx / Np) * stride + idx % Np] = gbits[idx];
  }
  int n[PER], by[PER], rk[PER], fs[PER];  // open dominators, all dominators, front, and the size of front tid + r * T
  bool open[PER], cand[PER];
#pragma unroll
  for (int r = 0; r < PER; ++r) {
    const int c = tid + r * T;
    cand[r] = c < N && (candidates == nullptr || candidates[g * N + c] != 0);
    open[r] = cand[r];
    n[r] = 0;
    rk[r] = -1;
    fs[r] = 0;
    if (c < N)
      for (int s = 0; s < S; ++s) n[r] += ws.by[(g * S + s) * Np + c];
    by[r] = n[r];
  }
  if (tid == 0) s_left = 0;
  __syncthreads();

  int made = 0;
  while (made < F) {
    uint32_t* member = s_member[made & 1];
#pragma unroll
    for (int r = 0; r < PER; ++r) {
      const bool in = open[r] && n[r] == 0;  // no open design dominates it: a member of this front
      const unsigned long long o = __ballot(in);
      const int base = r * T + wave * 64;
      if (lane == 0 && base < Np) {
        member[base / 32] = static_cast<uint32_t>(o);
        member[base / 32 + 1] = static_cast<uint32_t>(o >> 32);
      }
      if (in) {
        open[r] = false;
        rk[r] = made;
      }
    }
    __syncthreads();
    // (nothing goes to global memory inside the loop)
    unsigned long long nz[kMaxWords / 64];
    bool any = false;
#pragma unroll
    for (int h = 0; h < kMaxWords / 64; ++h) {
      const int w = h * 64 + lane;
      nz[h] = __ballot(w < W && member[w] != 0u);
      any = any || nz[h] != 0ull;
    }
    if (!any) break;  // (uniform: every wave read the same words.  A non-empty open set has a member, so the open set is empty)
    // Groups of four words with a non-zero member word among them: the loads of a group - four per design - are in flight together.
    int size = 0;
#pragma unroll
    for (int h = 0; h < kMaxWords / 64; ++h) {
      unsigned long long left = nz[h];
      while (left != 0ull) {  // (uniform)
        const int first = __builtin_ctzll(left);
        const int b = first & ~(kWordsInFlight - 1);
        const unsigned group = static_cast<unsigned>(left >> b) & ((1u << kWordsInFlight) - 1);
        left &= ~(((1ull << kWordsInFlight) - 1) << b);
        if ((group & (group - 1)) == 0u) {  // (uniform) one non-zero word in the group - a front of few designs: that word alone
          const int w = h * 64 + first;
          const uint32_t m = member[w];
          size += __popc(m);
#pragma unroll
          for (int r = 0; r < PER; ++r)
            if (open[r]) n[r] -= __popc(bits[w * stride + tid + r * T] & m);
          continue;
        }
        const int w0 = h * 64 + b;
        uint32_t m[kWordsInFlight];
        int at[kWordsInFlight];
#pragma unroll
        for (int u = 0; u < kWordsInFlight; ++u) {  // (W is even, not a multiple of four: a word past the row counts as zero)
          at[u] = w0 + u < W ? w0 + u : W - 1;
          m[u] = w0 + u < W ? member[w0 + u] : 0u;
          size += __popc(m[u]);
        }
#pragma unroll
        for (int r = 0; r < PER; ++r)
          if (open[r]) {
            uint32_t x[kWordsInFlight];
#pragma unroll
            for (int u = 0; u < kWordsInFlight; ++u) x[u] = bits[at[u] * stride + tid + r * T];
#pragma unroll
            for (int u = 0; u < kWordsInFlight; ++u) n[r] -= __popc(x[u] & m[u]);
          }
      }
    }
#pragma unroll
    for (int r = 0; r < PER; ++r)
      if (tid + r * T == made) fs[r] = size;
    ++made;
  }

  __syncthreads();  // (the bits in LDS are dead from here on)
  int of[PER];
  unsigned long long key[PER];
#pragma unroll
  for (int r = 0; r < PER; ++r) {
    const int c = tid + r * T;
    const unsigned long long o = __ballot(open[r]);
    if (lane == 0 && o != 0ull) atomicAdd(&s_left, __popcll(o));
    of[r] = -1;
    key[r] = 0ull;
    if (c >= N) continue;
    if (cand[r] && (n_dominated != nullptr || order != nullptr)) {
      of[r] = 0;
      for (int b = 0; b < B; ++b) of[r] += ws.of[(g * B + b) * Np + c];
    }
    rank[g * N + c] = rk[r];
    if (n_dominators != nullptr) n_dominators[g * N + c] = cand[r] ? by[r] : -1;
    if (n_dominated != nullptr) n_dominated[g * N + c] = of[r];
    if (order != nullptr) {  // (class, score, -n_dominated) of the tuple as one unsigned integer: 13 + 32 + 12 bits
      const unsigned long long cls = rk[r] >= 0 ? rk[r] : cand[r] ? N : N + 1;
      key[r] = (cls << kKeyClassShift) | (static_cast<unsigned long long>(score_bits(score != nullptr ? score[g * N + c] : 0.f)) << kKeyScoreShift) |
               static_cast<unsigned long long>(kMaxGroup - 1 - (cand[r] ? of[r] : 0));
      s_dyn[c] = key[r];
    }
  }
  for (int p = tid; p < F; p += T) {
    int v = 0;
#pragma unroll
    for (int r = 0; r < PER; ++r)
      if (p == tid + r * T) v = fs[r];  // (0 past `made`)
    front_size[g * F + p] = v;
  }
  __syncthreads();
  if (tid == 0) {
    count[g] = made;
    if (n_unranked != nullptr) n_unranked[g] = s_left;
  }
  if (order != nullptr) {
    // The position of a design is the number of designs whose tuple is smaller.  The tuple's last component, the index, needs no bits:
    // design j < i comes before i when key(j) <= key(i), design j > i when key(j) < key(i).  The designs of a wave are consecutive, so
    // per block of 64 designs j the wave compares with key + 1 (blocks before its own) or with key (its own and later blocks) - one
    // 64-bit compare per pair - and the ties inside its own block are added afterwards.
    int pos[PER];
#pragma unroll
    for (int r = 0; r < PER; ++r) pos[r] = 0;
    for (int jb = 0; jb < N; jb += 64) {  // (uniform)
      unsigned long long than[PER];
#pragma unroll
      for (int r = 0; r < PER; ++r) than[r] = jb < r * T + wave * 64 ? key[r] + 1 : key[r];
      const int jend = N - jb < 64 ? N - jb : 64;
      for (int t = 0; t < jend; ++t) {
        const unsigned long long kj = s_dyn[jb + t];  // (a broadcast)
#pragma unroll
        for (int r = 0; r < PER; ++r) pos[r] += kj < than[r] ? 1 : 0;
      }
    }
#pragma unroll
    for (int r = 0; r < PER; ++r) {
      const int base = r * T + wave * 64;
      for (int t = 0; t < 64 && base + t < N; ++t) pos[r] += (t < lane && s_dyn[base + t] == key[r]) ? 1 : 0;
    }
#pragma unroll
    for (int r = 0; r < PER; ++r) {
      const int c = tid + r * T;
      if (c < N) order[g * N + pos[r]] = c;
    }
  }
}

}  // namespace
}  // namespace diffab

using namespace diffab;

extern "C" {

int diffab_metrics_pareto(const float* objectives, const uint8_t* maximize, const float* violation, const float* score,
                          const uint8_t* candidates, int32_t G, int32_t N, int32_t M, int32_t F, int32_t* rank, int32_t* n_dominators,
                          int32_t* n_dominated, int32_t* front_size, int32_t* count, int32_t* n_unranked, int64_t* order, void* workspace,
                          size_t workspace_bytes, void* stream) {
  StreamOrder order_(stream);
  const char* who = "metrics_pareto";
  if (!group_shape_ok(who, G, N)) return DIFFAB_ERR_ARG;
  DIFFAB_REQUIRE(M >= 1 && M <= kMaxObjectives, DIFFAB_ERR_ARG, "%s: M = %d objectives outside [1, %d]", who, M, kMaxObjectives);
  DIFFAB_REQUIRE(F >= 0 && F <= N, DIFFAB_ERR_ARG, "%s: F = %d fronts outside [0, N = %d]", who, F, N);
  if (G == 0) return DIFFAB_OK;
  DIFFAB_REQUIRE(objectives != nullptr, DIFFAB_ERR_ARG, "%s: null input", who);
  DIFFAB_REQUIRE(rank != nullptr && count != nullptr && (F == 0 || front_size != nullptr), DIFFAB_ERR_ARG, "%s: null output", who);
  const ParetoWorkspace ws = carve_pareto(workspace, G, N);
  if (const int e = workspace_ok(who, workspace, 256, workspace_bytes, ws.bytes)) return e;
  const int Np = pad64(N), S = (N + kSegCols - 1) / kSegCols;
  const int64_t items = static_cast<int64_t>(G) * (Np / 64) * S;
  DIFFAB_REQUIRE(items <= INT_MAX, DIFFAB_ERR_UNSUPPORTED, "%s: G = %d groups of N = %d are more tiles than one launch holds", who, G, N);
  hipStream_t st = as_stream(stream);
  hipLaunchKernelGGL(pareto_dominance_kernel, dim3(static_cast<unsigned>(items)), dim3(64), static_cast<size_t>(M) * kTile * sizeof(float), st,
                     objectives, maximize, violation, candidates, N, Np, S, M, ws);
  const int threads = Np < kMaxThreads ? Np : kMaxThreads;
  if (N <= kLdsMaxN) {  // the one place that selects the form
    const size_t lds = lds_peel_bytes(Np, true);
    if (lds > 64 * 1024)  // (above the default limit of a launch: 128 KiB at N = 1024, of the 160 KiB a CU has)
      DIFFAB_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(pareto_peel_kernel<1, true>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                           static_cast<int>(lds_peel_bytes(kLdsMaxN, true))));
    hipLaunchKernelGGL((pareto_peel_kernel<1, true>), dim3(G), dim3(threads), lds, st, score, candidates, N, Np, S, F, ws, rank, n_dominators,
                       n_dominated, front_size, count, n_unranked, order);
  } else {
    hipLaunchKernelGGL((pareto_peel_kernel<kMaxPerThread, false>), dim3(G), dim3(threads), lds_peel_bytes(Np, false), st, score, candidates, N, Np,
                       S, F, ws, rank, n_dominators, n_dominated, front_size, count, n_unranked, order);
  }
  DIFFAB_LAUNCH_CHECK();
  return DIFFAB_OK;
}

}  // extern "C"
