// conformation_kernels.hip - the nearest library loop of every design by backbone-dihedral distance, and the dihedrals of the designed
// residues of a row as a loop: diffab_metrics_dihedral_nearest and diffab_metrics_pack_dihedrals.  The rule is the
// header comment of the entries in include/diffab_hip_conformation.h.
//
// Built with -ffp-contract=off like the other defined numbers (csrc/Makefile): the epilogue is __fdiv_rn and one rounded 2 - 2 t.  The
// product of the features runs on v_mfma_f32_16x16x4_f32, whose result is the k-ordered fmaf chain of the rule.  No atomics, no inline
// assembly; every value reaches memory through plain C++ stores.
#include <cmath>

#include "../../include/diffab_hip_conformation.h"
#include "analysis_common.h"

namespace diffab {
namespace {

using f32x4 = __attribute__((ext_vector_type(4))) float;
using u64 = unsigned long long;

constexpr int kMaxLen = DIFFAB_CONFORMATION_MAX_LENGTH;
constexpr int kMaxAngles = DIFFAB_CONFORMATION_MAX_ANGLES;
constexpr int kChunk = DIFFAB_CONFORMATION_CHUNK;
constexpr int kLens = kMaxLen + 1;   // the clamped lengths 0 .. 64
constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kTile = 16;            // places of one tile of features: the 16 rows or columns of the MFMA
constexpr int kQT = 4;               // query tiles of a work-group: 64 sorted queries share every load of a library tile
constexpr int kQueries = kQT * kTile;
constexpr int kPair = 2;             // library tiles a wave takes at a time: two independent accumulators per query tile
constexpr int kAhead = 4;            // k-steps whose library loads are in flight while the MFMAs of the steps before them run
constexpr int kMaxK = 2 * kMaxAngles * kMaxLen;  // 384 numbers per loop
constexpr int kMaxBlocks = 1 << 22;  // work-groups of one launch of the distance kernel
constexpr u64 kNoKey = ~0ull;
static_assert(kMaxLen == 64, "one bit per slot of a 64-bit word of defined-bits");
static_assert(kChunk % (kPair * kTile * kWaves) == 0 && kChunk % kThreads == 0, "whole passes of the waves over a chunk");
static_assert(kMaxK % 4 == 0, "whole k-steps");

__device__ __forceinline__ int clamp_len(int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }
__host__ __device__ __forceinline__ int padded_k(int A, int L) { return (2 * A * L + 3) / 4 * 4; }

struct ConfSlot {
  int32_t len;    // the clamped length of the loop in this place
  int32_t entry;  // which one it is: its row in the caller's arrays
};

// One side (the queries, the library) in the order of its (clamped length, index).
struct ConfSide {
  float* feat;      // (tiles, Kp, 16): number k of the loop in place p at [p / 16][k][p % 16]; 0 for an undefined term and behind the length
  u64* mask;        // (n, A): the defined-bits of the loop in place p, bit i of word a for (slot i, angle a)
  ConfSlot* slot;   // (n): the places
  int32_t* base;    // (chunks, 65): launch 1 the chunk's loops of each length, after launch 2 the place of the first of them
  int32_t* start;   // (66): the place of the first loop of each length; [65] = n
  int32_t* place;   // (n): entry -> place
};

struct ConfWorkspace {
  ConfSide q, l;
  u64* key;         // (chunks of the library, R): (bits(d) << 32) | m of the chunk's nearest entry per query PLACE, ~0 without one
  int32_t* count;   // (chunks of the library, R): the chunk's entries within the radius
  size_t bytes;
};

ConfSide carve_side(Carver& c, int64_t n, int L, int A) {
  const size_t tiles = static_cast<size_t>((n + kTile - 1) / kTile), chunks = static_cast<size_t>((n + kChunk - 1) / kChunk);
  ConfSide s;
  s.feat = c.take<float>(tiles * static_cast<size_t>(padded_k(A, L)) * kTile);
  s.mask = c.take<u64>(static_cast<size_t>(n) * A);
  s.slot = c.take<ConfSlot>(static_cast<size_t>(n));
  s.base = c.take<int32_t>(chunks * kLens);
  s.start = c.take<int32_t>(kLens + 1);
  s.place = c.take<int32_t>(static_cast<size_t>(n));
  return s;
}

ConfWorkspace carve_conformation(void* base, int64_t R, int64_t M, int LQ, int LM, int A) {
  Carver c(base);
  ConfWorkspace w;
  w.q = carve_side(c, R, LQ, A);
  w.l = carve_side(c, M, LM, A);
  const size_t chunks = static_cast<size_t>((M + kChunk - 1) / kChunk);
  w.key = c.take<u64>(chunks * static_cast<size_t>(R));
  w.count = c.take<int32_t>(chunks * static_cast<size_t>(R));
  w.bytes = c.bytes();
  return w;
}

// What the three ordering launches know of a side.
struct ConfInput {
  const float* feat;
  const int32_t* len;
  int n, L, chunks;
};

// ------------------------------------------------------------------ (1) per chunk, the loops of each length
// The work-groups [0, q.chunks) take the queries, the others the library.
__global__ void __launch_bounds__(kThreads)
conformation_histogram_kernel(ConfInput qi, ConfSide qs, ConfInput li, ConfSide ls) {
  __shared__ uint8_t s_len[kChunk];
  const bool lib = static_cast<int>(blockIdx.x) >= qi.chunks;
  const ConfInput in = lib ? li : qi;
  const ConfSide side = lib ? ls : qs;
  const int chunk = static_cast<int>(blockIdx.x) - (lib ? qi.chunks : 0), tid = threadIdx.x;
  const int64_t e0 = static_cast<int64_t>(chunk) * kChunk;
  const int count = static_cast<int>(e0 + kChunk < in.n ? kChunk : in.n - e0);
  for (int e = tid; e < count; e += kThreads) s_len[e] = static_cast<uint8_t>(clamp_len(in.len[e0 + e], in.L));
  __syncthreads();
  if (tid < kLens) {
    int n = 0;
    for (int e = 0; e < count; ++e) n += s_len[e] == tid ? 1 : 0;
    side.base[static_cast<int64_t>(chunk) * kLens + tid] = n;
  }
}

// ------------------------------------------------------------------ (2) the place of the first loop of each (length, chunk)
// One work-group; lanes [0, 65) take the lengths of the queries, lanes [65, 130) those of the library.
__global__ void __launch_bounds__(kThreads)
conformation_scan_kernel(int q_chunks, ConfSide qs, int l_chunks, ConfSide ls) {
  __shared__ int s_total[2][kLens];
  const int tid = threadIdx.x, which = tid / kLens, len = tid % kLens;
  const bool mine = tid < 2 * kLens;
  const ConfSide side = which == 0 ? qs : ls;
  const int chunks = which == 0 ? q_chunks : l_chunks;
  if (mine) {
    int total = 0;
    for (int c = 0; c < chunks; ++c) total += side.base[static_cast<int64_t>(c) * kLens + len];
    s_total[which][len] = total;
  }
  __syncthreads();
  if (mine) {
    int run = 0;
    for (int v = 0; v < len; ++v) run += s_total[which][v];
    side.start[len] = run;
    if (len == kLens - 1) side.start[kLens] = run + s_total[which][len];
    for (int c = 0; c < chunks; ++c) {
      const int64_t at = static_cast<int64_t>(c) * kLens + len;
      const int h = side.base[at];
      side.base[at] = run;
      run += h;
    }
  }
}

// ------------------------------------------------------------------ (3) every loop at its place
// A loop's place is the first place of its (length, chunk) plus the loops of its length before it in its chunk: a count.  Only the slots
// below the clamped length are read.
__global__ void __launch_bounds__(kThreads)
conformation_place_kernel(ConfInput qi, ConfSide qs, ConfInput li, ConfSide ls, int A) {
  __shared__ uint8_t s_len[kChunk];
  const bool lib = static_cast<int>(blockIdx.x) >= qi.chunks;
  const ConfInput in = lib ? li : qi;
  const ConfSide side = lib ? ls : qs;
  const int chunk = static_cast<int>(blockIdx.x) - (lib ? qi.chunks : 0), tid = threadIdx.x;
  const int64_t e0 = static_cast<int64_t>(chunk) * kChunk;
  const int count = static_cast<int>(e0 + kChunk < in.n ? kChunk : in.n - e0);
  const int Kp = padded_k(A, in.L);
  for (int e = tid; e < count; e += kThreads) s_len[e] = static_cast<uint8_t>(clamp_len(in.len[e0 + e], in.L));
  __syncthreads();
  for (int e = tid; e < count; e += kThreads) {
    const int n = s_len[e];
    int rank = 0;
    for (int j = 0; j < e; ++j) rank += s_len[j] == n ? 1 : 0;
    const int64_t entry = e0 + e;
    const int64_t p = static_cast<int64_t>(side.base[static_cast<int64_t>(chunk) * kLens + n]) + rank;
    ConfSlot slot;
    slot.len = n, slot.entry = static_cast<int32_t>(entry);
    side.slot[p] = slot;
    side.place[entry] = static_cast<int32_t>(p);
    const float* __restrict__ row = in.feat + entry * in.L * A * 2;
    float* __restrict__ out = side.feat + (p / kTile) * Kp * kTile + (p % kTile);
    u64 words[kMaxAngles] = {0ull, 0ull, 0ull};
    for (int i = 0; i < n; ++i) {
#pragma unroll
      for (int a = 0; a < kMaxAngles; ++a) {
        if (a < A) {
          const int k = (i * A + a) * 2;
          const float c = row[k], s = row[k + 1];
          const bool defined = isfinite(c) && isfinite(s);
          words[a] |= static_cast<u64>(defined) << i;
          out[static_cast<int64_t>(k) * kTile] = defined ? c : 0.f;
          out[static_cast<int64_t>(k + 1) * kTile] = defined ? s : 0.f;
        }
      }
    }
    for (int k = 2 * A * n; k < Kp; ++k) out[static_cast<int64_t>(k) * kTile] = 0.f;
#pragma unroll
    for (int a = 0; a < kMaxAngles; ++a)
      if (a < A) side.mask[p * A + a] = words[a];
  }
}

// ------------------------------------------------------------------ (4) the distances
struct DistanceArgs {
  const int32_t* skip;
  float* matrix;
  int R, M, LQ, LM, A, min_terms;
  float radius;
  int chunks, group0;  // blockIdx.x = (group - group0) * chunks + chunk
};

__device__ __forceinline__ u64 shuffle_xor(u64 v, int off) {
  const uint32_t lo = static_cast<uint32_t>(__shfl_xor(static_cast<int>(static_cast<uint32_t>(v)), off, 64));
  const uint32_t hi = static_cast<uint32_t>(__shfl_xor(static_cast<int>(static_cast<uint32_t>(v >> 32)), off, 64));
  return (static_cast<u64>(hi) << 32) | lo;
}

// kCap: the numbers per loop the LDS image of a query tile has room for, the padded 2 A LQ of the call rounded up to one of four sizes
// (16, 32, 64 or 96 KB for the four tiles), so that short loops leave room for several work-groups per CU.
template <int kCap>
__global__ void __launch_bounds__(kThreads)
conformation_distance_kernel(DistanceArgs a, ConfSide qs, ConfSide ls, u64* __restrict__ part_key, int32_t* __restrict__ part_count) {
  __shared__ float s_a[kQT][kCap * kTile];  // the query tiles, k-major as in the workspace: k-step s of a lane at [64 s + lane]
  __shared__ u64 s_mask[kQueries][kMaxAngles];
  __shared__ int s_len[kQueries], s_row[kQueries], s_skip[kQueries];  // length -1 and row -1 behind the last query
  __shared__ u64 s_key[kWaves][kQueries];
  __shared__ int s_count[kWaves][kQueries];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, col = lane & 15, quad = lane >> 4;
  const int chunk = static_cast<int>(blockIdx.x % static_cast<unsigned>(a.chunks));
  const int64_t qp0 = (static_cast<int64_t>(a.group0) + blockIdx.x / static_cast<unsigned>(a.chunks)) * kQueries;
  const int A = a.A, KpQ = padded_k(A, a.LQ), KpL = padded_k(A, a.LM);
  const int n_queries = static_cast<int>(a.R - qp0 < kQueries ? a.R - qp0 : kQueries);
  const int n_qt = (n_queries + kTile - 1) / kTile;

  // the lengths of the group's queries (sorted: the first and the last), and the library places that hold them
  const int q_lo = qs.slot[qp0].len, q_hi = qs.slot[qp0 + n_queries - 1].len;
  const int64_t p_lo = ls.start[q_lo], p_hi = ls.start[q_hi + 1];
  const int64_t c_lo = static_cast<int64_t>(chunk) * kChunk, c_hi = c_lo + kChunk < a.M ? c_lo + kChunk : a.M;
  const bool matrix = a.matrix != nullptr;
  // what the waves walk: with a matrix the whole chunk, else its places of the queries' lengths, from a whole pair of tiles on
  int64_t w_lo = c_lo, w_hi = c_hi;
  if (!matrix) {
    w_lo = p_lo > c_lo ? p_lo / (kPair * kTile) * (kPair * kTile) : c_lo;
    w_hi = p_hi < c_hi ? p_hi : c_hi;
  }
  if (w_lo >= w_hi) {  // (uniform) nothing of this chunk is comparable with these queries
    if (tid < n_queries) {
      part_key[static_cast<int64_t>(chunk) * a.R + qp0 + tid] = kNoKey;
      part_count[static_cast<int64_t>(chunk) * a.R + qp0 + tid] = 0;
    }
    return;
  }

  if (tid < kQueries) {
    const bool have = tid < n_queries;
    ConfSlot slot;
    slot.len = -1, slot.entry = -1;
    if (have) slot = qs.slot[qp0 + tid];
    s_len[tid] = slot.len, s_row[tid] = slot.entry;
    s_skip[tid] = (have && a.skip != nullptr) ? a.skip[slot.entry] : -1;
#pragma unroll
    for (int w = 0; w < kMaxAngles; ++w) s_mask[tid][w] = (have && w < A) ? qs.mask[(qp0 + tid) * A + w] : 0ull;
  }
  const int q_steps = (2 * A * q_hi + 3) / 4;  // k-steps of the longest query
  for (int t = 0; t < n_qt; ++t) {
    const float* src = qs.feat + (qp0 / kTile + t) * KpQ * kTile;
    for (int i = tid; i < q_steps * 64; i += kThreads) s_a[t][i] = src[i];
  }
  __syncthreads();

  u64 best[kQT][4];
  int within[kQT][4];
#pragma unroll
  for (int t = 0; t < kQT; ++t)
#pragma unroll
    for (int r = 0; r < 4; ++r) best[t][r] = kNoKey, within[t][r] = 0;

  for (int64_t pp = w_lo + wave * (kPair * kTile); pp < w_hi; pp += kWaves * kPair * kTile) {  // (uniform per wave)
    // the lane's entry of each of the two tiles
    bool have[kPair];
    int l_len[kPair], l_entry[kPair];
    u64 l_mask[kPair][kMaxAngles];
#pragma unroll
    for (int j = 0; j < kPair; ++j) {
      const int64_t p = pp + j * kTile + col;
      have[j] = p < c_hi;
      ConfSlot slot;
      slot.len = -2, slot.entry = -1;
      if (have[j]) slot = ls.slot[p];
      l_len[j] = slot.len, l_entry[j] = slot.entry;
#pragma unroll
      for (int w = 0; w < kMaxAngles; ++w) l_mask[j][w] = (have[j] && w < A) ? ls.mask[p * A + w] : 0ull;
    }
    const int64_t p_last = pp + kPair * kTile - 1 < c_hi - 1 ? pp + kPair * kTile - 1 : c_hi - 1;
    const int l_hi = ls.slot[p_last].len;  // (sorted: the longest of the pair)
    const bool active = pp < p_hi && pp + kPair * kTile > p_lo;  // (uniform) some place of the pair is of a length of the queries
    const int shorter = q_hi < l_hi ? q_hi : l_hi;
    const int steps = active ? (2 * A * shorter + 3) / 4 : 0;
    const bool second = pp + kTile < c_hi;  // (uniform) the pair's second tile exists
    const float* b0 = ls.feat + (pp / kTile) * KpL * kTile + lane;
    const float* b1 = b0 + static_cast<int64_t>(KpL) * kTile;

    f32x4 acc[kQT][kPair];
#pragma unroll
    for (int t = 0; t < kQT; ++t)
#pragma unroll
      for (int j = 0; j < kPair; ++j) acc[t][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    // kAhead k-steps of the two tiles are requested before the MFMAs of the kAhead steps before them are issued
    float cur[kAhead][kPair], nxt[kAhead][kPair];
    auto request = [&](int s0, float (&v)[kAhead][kPair]) {
#pragma unroll
      for (int i = 0; i < kAhead; ++i) {
        const bool in = s0 + i < steps;  // (uniform)
        v[i][0] = in ? b0[(s0 + i) * 64] : 0.f;
        v[i][1] = (in && second) ? b1[(s0 + i) * 64] : 0.f;
      }
    };
    request(0, cur);
    for (int s0 = 0; s0 < steps; s0 += kAhead) {
      request(s0 + kAhead, nxt);
#pragma unroll
      for (int i = 0; i < kAhead; ++i) {
        if (s0 + i < steps) {  // (uniform; behind the last step the LDS image holds nothing)
#pragma unroll
          for (int t = 0; t < kQT; ++t) {
            if (t < n_qt) {  // (uniform)
              const float q = s_a[t][(s0 + i) * 64 + lane];
              acc[t][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(q, cur[i][0], acc[t][0], 0, 0, 0);
              acc[t][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(q, cur[i][1], acc[t][1], 0, 0, 0);
            }
          }
        }
      }
#pragma unroll
      for (int i = 0; i < kAhead; ++i) cur[i][0] = nxt[i][0], cur[i][1] = nxt[i][1];
    }

    // acc[t][j][r] = query 16 t + 4 quad + r of the group . the lane's entry of tile j
#pragma unroll
    for (int t = 0; t < kQT; ++t) {
      if (t >= n_qt) continue;  // (uniform)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int qi = t * kTile + quad * 4 + r;
        const int q_len = s_len[qi], row = s_row[qi], skip = s_skip[qi];
        u64 q_mask[kMaxAngles];
#pragma unroll
        for (int w = 0; w < kMaxAngles; ++w) q_mask[w] = s_mask[qi][w];
#pragma unroll
        for (int j = 0; j < kPair; ++j) {
          int n = 0;
#pragma unroll
          for (int w = 0; w < kMaxAngles; ++w) n += __popcll(q_mask[w] & l_mask[j][w]);
          const bool live = have[j] && row >= 0;
          const bool comparable = live && q_len == l_len[j] && n >= a.min_terms;
          float d = INFINITY;
          if (comparable) {
            const float tq = __fdiv_rn(acc[t][j][r], static_cast<float>(n));
            d = tq >= 1.f ? 0.f : 2.f - 2.f * tq;
          }
          if (matrix && live) a.matrix[static_cast<int64_t>(row) * a.M + l_entry[j]] = d;
          const bool counted = comparable && l_entry[j] != skip;
          const u64 key = counted ? (static_cast<u64>(__float_as_uint(d)) << 32) | static_cast<u64>(static_cast<uint32_t>(l_entry[j])) : kNoKey;
          best[t][r] = key < best[t][r] ? key : best[t][r];
          within[t][r] += (counted && d <= a.radius) ? 1 : 0;
        }
      }
    }
  }

  // over the 16 lanes that hold a query's columns, then over the waves
#pragma unroll
  for (int t = 0; t < kQT; ++t)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      u64 key = best[t][r];
      int count = within[t][r];
#pragma unroll
      for (int off = 8; off >= 1; off >>= 1) {
        const u64 other = shuffle_xor(key, off);
        key = other < key ? other : key;
        count += __shfl_xor(count, off, 64);
      }
      if (col == 0) s_key[wave][t * kTile + quad * 4 + r] = key, s_count[wave][t * kTile + quad * 4 + r] = count;
    }
  __syncthreads();
  if (tid < n_queries) {
    u64 key = s_key[0][tid];
    int count = s_count[0][tid];
#pragma unroll
    for (int w = 1; w < kWaves; ++w) {
      key = s_key[w][tid] < key ? s_key[w][tid] : key;
      count += s_count[w][tid];
    }
    part_key[static_cast<int64_t>(chunk) * a.R + qp0 + tid] = key;
    part_count[static_cast<int64_t>(chunk) * a.R + qp0 + tid] = count;
  }
}

// ------------------------------------------------------------------ (5) per query, over the chunks
__global__ void __launch_bounds__(kThreads)
conformation_finish_kernel(int R, int A, int chunks, ConfSide qs, ConfSide ls, const u64* __restrict__ part_key,
                           const int32_t* __restrict__ part_count, float* distance, int32_t* index, int32_t* n_terms, int32_t* n_within) {
  const int64_t qp = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x;
  if (qp >= R) return;
  u64 best = kNoKey;
  int within = 0;
  for (int c = 0; c < chunks; ++c) {
    const u64 key = part_key[static_cast<int64_t>(c) * R + qp];
    best = key < best ? key : best;
    within += part_count[static_cast<int64_t>(c) * R + qp];
  }
  const bool none = best == kNoKey;
  const int m = none ? -1 : static_cast<int>(static_cast<uint32_t>(best));
  int n = 0;
  if (!none) {
    const int64_t lp = ls.place[m];
    for (int w = 0; w < A; ++w) n += __popcll(qs.mask[qp * A + w] & ls.mask[lp * A + w]);
  }
  const int64_t r = qs.slot[qp].entry;
  if (distance != nullptr) distance[r] = none ? INFINITY : __uint_as_float(static_cast<uint32_t>(best >> 32));
  if (index != nullptr) index[r] = m;
  if (n_terms != nullptr) n_terms[r] = n;
  if (n_within != nullptr) n_within[r] = within;
}

// An empty library: nothing is comparable.
__global__ void __launch_bounds__(kThreads)
conformation_nothing_kernel(int R, float* distance, int32_t* index, int32_t* n_terms, int32_t* n_within) {
  const int64_t r = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x;
  if (r >= R) return;
  if (distance != nullptr) distance[r] = INFINITY;
  if (index != nullptr) index[r] = -1;
  if (n_terms != nullptr) n_terms[r] = 0;
  if (n_within != nullptr) n_within[r] = 0;
}

// ------------------------------------------------------------------ the dihedrals of the counted residues of a row as a loop
// One wave per row: the counted slots of 64 slots at a time, each at its rank among them.
__global__ void __launch_bounds__(64)
conformation_pack_kernel(const float* __restrict__ phi, const float* __restrict__ psi, const float* __restrict__ omega,
                         const uint8_t* __restrict__ mask, const uint8_t* __restrict__ residue_mask, const int32_t* __restrict__ segment_idx,
                         int segment, int group_size, int K, int L, float* out_angles, int32_t* out_len) {
  const int lane = threadIdx.x;
  const int64_t row = blockIdx.x, g = row / group_size, rbase = row * K, gbase = g * K;
  int count = 0;
  for (int k0 = 0; k0 < K; k0 += 64) {
    const int k = k0 + lane;
    bool counted = false;
    if (k < K) {
      counted = mask[gbase + k] != 0;
      if (residue_mask != nullptr) counted = counted && residue_mask[gbase + k] != 0;
      if (segment_idx != nullptr) counted = counted && segment_idx[gbase + k] == segment;
    }
    const BallotRank at = ballot_rank(counted, lane);
    const int pos = count + at.rank;
    if (counted && pos < L && out_angles != nullptr) {
      float* out = out_angles + (row * L + pos) * 3;
      out[0] = phi[rbase + k], out[1] = psi[rbase + k], out[2] = omega[rbase + k];
    }
    count += at.count;
  }
  if (out_angles != nullptr)
    for (int p = count + lane; p < L; p += 64) {
      float* out = out_angles + (row * L + p) * 3;
      out[0] = NAN, out[1] = NAN, out[2] = NAN;
    }
  if (lane == 0 && out_len != nullptr) out_len[row] = count;
}

}  // namespace
}  // namespace diffab

using namespace diffab;

extern "C" {

int diffab_metrics_dihedral_nearest(const float* q_feat, const int32_t* q_len, int32_t R, int32_t LQ, const float* lib_feat,
                                    const int32_t* lib_len, int32_t M, int32_t LM, int32_t A, const int32_t* skip, float radius,
                                    int32_t min_terms, float* distance, int32_t* index, int32_t* n_terms, int32_t* n_within, float* matrix,
                                    void* workspace, size_t workspace_bytes, void* stream) {
  StreamOrder order_(stream);
  const char* who = "metrics_dihedral_nearest";
  DIFFAB_REQUIRE(R >= 0 && M >= 0, DIFFAB_ERR_ARG, "%s: negative extent (R = %d queries, M = %d library entries)", who, R, M);
  DIFFAB_REQUIRE(LQ >= 1 && LQ <= kMaxLen, DIFFAB_ERR_ARG, "%s: LQ = %d slots per query outside [1, %d]", who, LQ, kMaxLen);
  DIFFAB_REQUIRE(LM >= 1 && LM <= kMaxLen, DIFFAB_ERR_ARG, "%s: LM = %d slots per library entry outside [1, %d]", who, LM, kMaxLen);
  DIFFAB_REQUIRE(A >= 1 && A <= kMaxAngles, DIFFAB_ERR_ARG, "%s: A = %d angles per slot outside [1, %d]", who, A, kMaxAngles);
  DIFFAB_REQUIRE(min_terms >= 1, DIFFAB_ERR_ARG, "%s: min_terms = %d, at least 1", who, min_terms);
  if (R == 0) return DIFFAB_OK;
  DIFFAB_REQUIRE(q_feat && q_len, DIFFAB_ERR_ARG, "%s: null input (q_feat, q_len)", who);
  DIFFAB_REQUIRE(M == 0 || (lib_feat && lib_len), DIFFAB_ERR_ARG, "%s: null input (lib_feat, lib_len) with M = %d", who, M);
  DIFFAB_REQUIRE(matrix == nullptr || static_cast<int64_t>(R) * M < (1ll << 31), DIFFAB_ERR_ARG,
                 "%s: matrix of R * M = %d * %d elements, fewer than 2^31 are needed", who, R, M);
  const ConfWorkspace ws = carve_conformation(workspace, R, M, LQ, LM, A);
  if (const int e = workspace_ok(who, workspace, 256, workspace_bytes, ws.bytes)) return e;
  hipStream_t st = as_stream(stream);
  const bool per_query = distance != nullptr || index != nullptr || n_terms != nullptr || n_within != nullptr;
  if (M == 0) {
    if (per_query)
      hipLaunchKernelGGL(conformation_nothing_kernel, dim3((R + kThreads - 1) / kThreads), dim3(kThreads), 0, st, R, distance, index, n_terms, n_within);
    DIFFAB_LAUNCH_CHECK();
    return DIFFAB_OK;
  }
  ConfInput qi, li;
  qi.feat = q_feat, qi.len = q_len, qi.n = R, qi.L = LQ, qi.chunks = (R + kChunk - 1) / kChunk;
  li.feat = lib_feat, li.len = lib_len, li.n = M, li.L = LM, li.chunks = (M + kChunk - 1) / kChunk;
  hipLaunchKernelGGL(conformation_histogram_kernel, dim3(qi.chunks + li.chunks), dim3(kThreads), 0, st, qi, ws.q, li, ws.l);
  hipLaunchKernelGGL(conformation_scan_kernel, dim3(1), dim3(kThreads), 0, st, qi.chunks, ws.q, li.chunks, ws.l);
  hipLaunchKernelGGL(conformation_place_kernel, dim3(qi.chunks + li.chunks), dim3(kThreads), 0, st, qi, ws.q, li, ws.l, A);
  DistanceArgs a;
  a.skip = skip, a.matrix = matrix, a.R = R, a.M = M, a.LQ = LQ, a.LM = LM, a.A = A, a.min_terms = min_terms, a.radius = radius;
  a.chunks = li.chunks;
  const int groups = (R + kQueries - 1) / kQueries, per_launch = kMaxBlocks / a.chunks > 0 ? kMaxBlocks / a.chunks : 1;
  for (int g0 = 0; g0 < groups; g0 += per_launch) {
    const int n = groups - g0 < per_launch ? groups - g0 : per_launch;
    a.group0 = g0;
    const dim3 grid(static_cast<unsigned>(n) * static_cast<unsigned>(a.chunks));
    const int k_q = padded_k(A, LQ);
    if (k_q <= 64) hipLaunchKernelGGL(conformation_distance_kernel<64>, grid, dim3(kThreads), 0, st, a, ws.q, ws.l, ws.key, ws.count);
    else if (k_q <= 128) hipLaunchKernelGGL(conformation_distance_kernel<128>, grid, dim3(kThreads), 0, st, a, ws.q, ws.l, ws.key, ws.count);
    else if (k_q <= 256) hipLaunchKernelGGL(conformation_distance_kernel<256>, grid, dim3(kThreads), 0, st, a, ws.q, ws.l, ws.key, ws.count);
    else hipLaunchKernelGGL(conformation_distance_kernel<kMaxK>, grid, dim3(kThreads), 0, st, a, ws.q, ws.l, ws.key, ws.count);
  }
  if (per_query)
    hipLaunchKernelGGL(conformation_finish_kernel, dim3((R + kThreads - 1) / kThreads), dim3(kThreads), 0, st, R, A, a.chunks, ws.q, ws.l, ws.key,
                       ws.count, distance, index, n_terms, n_within);
  DIFFAB_LAUNCH_CHECK();
  return DIFFAB_OK;
}

int diffab_metrics_pack_dihedrals(const float* phi, const float* psi, const float* omega, const uint8_t* mask, const uint8_t* residue_mask,
                                  const int32_t* segment_idx, int32_t segment, int32_t rows, int32_t group_size, int32_t K, int32_t L,
                                  float* out_angles, int32_t* out_len, void* stream) {
  StreamOrder order_(stream);
  const char* who = "metrics_pack_dihedrals";
  if (!rows_shape_ok(who, rows, group_size, K, DIFFAB_METRICS_MAX_K)) return DIFFAB_ERR_ARG;
  DIFFAB_REQUIRE(L >= 1 && L <= kMaxLen, DIFFAB_ERR_ARG, "%s: L = %d slots per loop outside [1, %d]", who, L, kMaxLen);
  if (rows == 0) return DIFFAB_OK;
  DIFFAB_REQUIRE(phi && psi && omega && mask, DIFFAB_ERR_ARG, "%s: null input (phi, psi, omega, mask)", who);
  if (out_angles == nullptr && out_len == nullptr) return DIFFAB_OK;
  hipLaunchKernelGGL(conformation_pack_kernel, dim3(rows), dim3(64), 0, as_stream(stream), phi, psi, omega, mask, residue_mask, segment_idx,
                     segment, group_size, K, L, out_angles, out_len);
  DIFFAB_LAUNCH_CHECK();
  return DIFFAB_OK;
}

}  // extern "C"
