// novelty_kernels.hip - the nearest library sequence of every design by edit distance, and the designed residues of a row as a sequence
// (DESIGN section 4.26): diffab_metrics_edit_nearest and diffab_metrics_pack_sequences.  The rule is the header comment of the entries
// in include/diffab_hip_novelty.h.
//
// Built with -ffp-contract=off like the other defined numbers (csrc/Makefile): the one fp32 quotient is __fdiv_rn of two integers below
// 2^9.  Everything else is integer work on the VALU: Myers' bit-vector recurrence in Hyyro's global form on 64-bit words, the query's
// match masks in LDS, one library entry per lane.  No atomics; every value reaches memory through plain C++ stores.
#include <cmath>

#include "../../include/diffab_hip_novelty.h"
#include "analysis_common.h"

namespace diffab {
namespace {

constexpr int kMaxQuery = DIFFAB_NOVELTY_MAX_QUERY;
constexpr int kMaxLibrary = DIFFAB_NOVELTY_MAX_LIBRARY;
constexpr int kChunk = DIFFAB_NOVELTY_CHUNK;
constexpr int kClasses = 32;   // tokens that can match: their 32 words of a Peq table cover every 4-byte bank of the LDS once; one
                               // more word, all zeros, stands for every token that matches nothing (it shares its banks with token 0)
constexpr int kThreads = 256;  // lanes of a work-group of the distance kernel, one library entry each per pass over the chunk
constexpr int kWaves = kThreads / 64;
constexpr int kTile = 16;      // queries of a work-group
constexpr int kGroup = 4;      // queries a lane runs side by side along the text: four independent chains of the recurrence
constexpr int kPad = 255;
constexpr int kNone = 1023;    // stands for "not compared" in a wave's key; every distance is at most kMaxLibrary
constexpr int kMaxBlocks = 1 << 22;  // work-groups of one launch of the distance kernel
static_assert(kMaxQuery == 64, "a query is one bit per position of a 64-bit word");
static_assert(kClasses == DIFFAB_METRICS_MAX_CLASSES, "the match rule's limit is the class limit of the other entries");
static_assert(kChunk % kThreads == 0 && kTile % kGroup == 0, "whole passes, whole groups");
constexpr int kChunkBits = 11;
static_assert(kChunk == 1 << kChunkBits && kChunk <= 65536, "a key is (distance << 11) | (m - chunk start); the order of a chunk is 16-bit slots");
static_assert(kNone > kMaxLibrary && kNone > kMaxQuery && kMaxLibrary < 512, "a distance takes nine bits of a key, kNone ten");

__device__ __forceinline__ int clamp_len(int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }

// A chunk's entries stand in the workspace in the order of their lengths (ties by m), so that the 64 entries of a wave are of one or two
// lengths and the wave's walk along the text ends for all its lanes together.
struct NoveltySlot {
  int32_t len;    // the clamped length of the entry in this place
  int32_t entry;  // which one it is: m - chunk start
};

struct NoveltyWorkspace {
  uint32_t* words;            // (LMw, M): word w of the entry in place s, tokens 4w .. 4w + 3, 255 behind the clamped length
  NoveltySlot* slot;          // (M): the places, chunk by chunk
  unsigned long long* key;    // (chunks, R): (distance << 32) | m of the chunk's nearest entry, ~0 without one
  int32_t* count;             // (chunks, R): the chunk's entries within the radius
  size_t bytes;
};

NoveltyWorkspace carve_novelty(void* base, int64_t R, int64_t M, int64_t LM) {
  Carver c(base);
  const size_t LMw = static_cast<size_t>((LM + 3) / 4), chunks = static_cast<size_t>((M + kChunk - 1) / kChunk);
  NoveltyWorkspace w;
  w.words = c.take<uint32_t>(LMw * static_cast<size_t>(M));
  w.slot = c.take<NoveltySlot>(static_cast<size_t>(M));
  w.key = c.take<unsigned long long>(chunks * static_cast<size_t>(R));
  w.count = c.take<int32_t>(chunks * static_cast<size_t>(R));
  w.bytes = c.bytes();
  return w;
}

// ------------------------------------------------------------------ (1) the library, word-major, each chunk in the order of its lengths
// One work-group per chunk.  The place of an entry is the number of entries of the chunk with a smaller (length, m): a count, so no
// order of execution shows in it.  Only the bytes below the clamped length are read; the writes of a wave are consecutive words.
__global__ void __launch_bounds__(kThreads)
novelty_repack_kernel(const uint8_t* __restrict__ lib_tokens, const int32_t* __restrict__ lib_len, int M, int LM, NoveltyWorkspace ws) {
  __shared__ int s_key[kChunk];        // (length << 11) | entry
  __shared__ uint16_t s_at[kChunk];    // place -> entry
  const int tid = threadIdx.x, LMw = (LM + 3) / 4;
  const int64_t m_begin = static_cast<int64_t>(blockIdx.x) * kChunk;
  const int count = static_cast<int>(m_begin + kChunk < M ? kChunk : M - m_begin);
  for (int e = tid; e < count; e += kThreads) s_key[e] = (clamp_len(lib_len[m_begin + e], LM) << kChunkBits) | e;
  __syncthreads();
  for (int e = tid; e < count; e += kThreads) {
    const int mine = s_key[e];
    int place = 0;
    for (int j = 0; j < count; ++j) place += s_key[j] < mine ? 1 : 0;  // (every lane reads the same word)
    s_at[place] = static_cast<uint16_t>(e);
  }
  __syncthreads();
  for (int p = tid; p < count; p += kThreads) {
    const int e = s_at[p], n = s_key[e] >> kChunkBits;
    const uint8_t* row = lib_tokens + (m_begin + e) * LM;
    NoveltySlot slot;
    slot.len = n, slot.entry = e;
    ws.slot[m_begin + p] = slot;
    for (int w = 0; w < LMw; ++w) {
      uint32_t word = 0u;
#pragma unroll
      for (int b = 0; b < 4; ++b) {
        const int j = 4 * w + b;
        const uint32_t c = j < n ? static_cast<uint32_t>(row[j]) : static_cast<uint32_t>(kPad);
        word |= c << (8 * b);
      }
      ws.words[static_cast<int64_t>(w) * M + m_begin + p] = word;
    }
  }
}

// ------------------------------------------------------------------ (2) the distances
struct NearestArgs {
  const uint8_t* q_tokens;
  const int32_t* q_len;
  const int32_t* skip;
  int32_t* matrix;
  int R, LQ, M, radius;
  int chunks, tile0;  // blockIdx.x = (tile - tile0) * chunks + chunk
};

// v << 1 with `low` in bit 0, on the two halves: one funnel shift and one shift-or of the 32-bit VALU, no 64-bit shift.
__device__ __forceinline__ unsigned long long shift_in(unsigned long long v, uint32_t low) {
  const uint32_t lo = static_cast<uint32_t>(v), hi = static_cast<uint32_t>(v >> 32);
  const uint32_t up = __builtin_amdgcn_alignbit(hi, lo, 31), down = (lo << 1) | low;
  return (static_cast<unsigned long long>(up) << 32) | down;
}

// One step of the recurrence for one query: the text token's match mask against the vertical deltas.  The query stands at the TOP of
// the word, its last token in bit 63, so the score's bit is the sign of the high half whatever the query's length.  The bits below the
// query hold no pattern: Eq, Pv and Mv are 0 there and stay 0, Ph is 1 there, and what the shift moves into the query's first bit is the
// +1 of the first row of a global alignment (for a query of 64 tokens the 1 comes from shift_in).
__device__ __forceinline__ void myers_step(unsigned long long Eq, unsigned long long& Pv, unsigned long long& Mv, int& score) {
  const unsigned long long Xv = Eq | Mv;
  const unsigned long long Xh = (((Eq & Pv) + Pv) ^ Pv) | Eq;  // (a 64-bit addition: the carry out of bit 31 goes into bit 32)
  unsigned long long Ph = Mv | ~(Xh | Pv);
  unsigned long long Mh = Pv & Xh;
  score += static_cast<int>(static_cast<uint32_t>(Ph >> 32) >> 31);
  score -= static_cast<int>(static_cast<uint32_t>(Mh >> 32) >> 31);
  Ph = shift_in(Ph, 1u);
  Mh = shift_in(Mh, 0u);
  Pv = Mh | ~(Xv | Ph);
  Mv = Ph & Xv;
}

__global__ void __launch_bounds__(kThreads)
novelty_distance_kernel(NearestArgs a, NoveltyWorkspace ws) {
  __shared__ unsigned long long s_peq[kTile][kClasses + 1];
  __shared__ uint8_t s_tok[kTile][kMaxQuery];
  __shared__ int s_qlen[kTile], s_skip[kTile];
  __shared__ int s_best[kWaves][kTile], s_within[kWaves][kTile];  // per wave: the least (distance << 11) | (m - chunk start) so far, the count

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int chunk = static_cast<int>(blockIdx.x % static_cast<unsigned>(a.chunks));
  const int64_t r0 = (static_cast<int64_t>(a.tile0) + blockIdx.x / static_cast<unsigned>(a.chunks)) * kTile;
  const int64_t m_begin = static_cast<int64_t>(chunk) * kChunk;
  const int64_t m_end = m_begin + kChunk < a.M ? m_begin + kChunk : a.M;

  // the tile's queries: tokens below the clamped length (255 behind it, and for a query behind R), lengths, skips
  if (tid < kTile) {
    const int64_t r = r0 + tid;
    s_qlen[tid] = r < a.R ? clamp_len(a.q_len[r], a.LQ) : 0;
    s_skip[tid] = (r < a.R && a.skip != nullptr) ? a.skip[r] : -1;
  }
  for (int t = tid; t < kWaves * kTile; t += kThreads) (&s_best[0][0])[t] = kNone << kChunkBits, (&s_within[0][0])[t] = 0;
  __syncthreads();
  for (int t = tid; t < kTile * kMaxQuery; t += kThreads) {
    const int q = t / kMaxQuery, i = t % kMaxQuery;
    const int64_t r = r0 + q;
    s_tok[q][i] = i < s_qlen[q] ? a.q_tokens[r * a.LQ + i] : static_cast<uint8_t>(kPad);
  }
  __syncthreads();
  for (int t = tid; t < kTile * (kClasses + 1); t += kThreads) {
    const int q = t / (kClasses + 1), c = t % (kClasses + 1);
    const int n = s_qlen[q];
    unsigned long long bits = 0ull;  // bit 64 - n + i for query token i: the query's last token in bit 63
    for (int i = 0; i < n; ++i) bits |= static_cast<unsigned long long>(s_tok[q][i] == c && c < kClasses) << (kMaxQuery - n + i);
    s_peq[q][c] = bits;
  }
  __syncthreads();

  for (int64_t p0 = m_begin; p0 < m_end; p0 += kThreads) {  // (uniform)
    const int64_t p = p0 + tid;  // the lane's place; the entry that stands there is m
    const bool have = p < m_end;
    NoveltySlot slot;
    slot.len = 0, slot.entry = 0;
    if (have) slot = ws.slot[p];
    const int n = slot.len;
    const int64_t m = m_begin + slot.entry;
    for (int g0 = 0; g0 < kTile; g0 += kGroup) {  // (uniform)
      if (r0 + g0 >= a.R) break;                  // (uniform)
      unsigned long long Pv[kGroup], Mv[kGroup];
      int score[kGroup], d[kGroup], qlen[kGroup];
#pragma unroll
      for (int k = 0; k < kGroup; ++k) {
        qlen[k] = __builtin_amdgcn_readfirstlane(s_qlen[g0 + k]);
        Pv[k] = qlen[k] > 0 ? ~0ull << (kMaxQuery - qlen[k]) : 0ull;  // (an empty query: its answer is the text's length, below)
        Mv[k] = 0ull, score[k] = qlen[k], d[k] = qlen[k];             // d: the score behind the text's last token
      }
      for (int w = 0; 4 * w < n; ++w) {
        uint32_t word = ws.words[static_cast<int64_t>(w) * a.M + p];
#pragma unroll
        for (int b = 0; b < 4; ++b) {
          const int c = static_cast<int>(word & 0xFFu) < kClasses ? static_cast<int>(word & 0xFFu) : kClasses;
          word >>= 8;
          const bool last = 4 * w + b + 1 == n;  // (the tokens behind it in the word are padding: their steps are run and not kept)
#pragma unroll
          for (int k = 0; k < kGroup; ++k) {
            const unsigned long long Eq = s_peq[g0 + k][c];
            myers_step(Eq, Pv[k], Mv[k], score[k]);
            d[k] = last ? score[k] : d[k];
          }
        }
      }
#pragma unroll
      for (int k = 0; k < kGroup; ++k) {
        const int q = g0 + k;
        const int64_t r = r0 + q;
        const int dist = qlen[k] == 0 ? n : d[k];
        const bool live = have && r < a.R;
        if (live && a.matrix != nullptr) a.matrix[r * a.M + m] = dist;
        const bool counted = live && m != static_cast<int64_t>(s_skip[q]);
        int key = ((counted ? dist : kNone) << kChunkBits) | slot.entry;
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) {
          const int other = __shfl_xor(key, off, 64);
          key = other < key ? other : key;
        }
        const int within = __popcll(__ballot(counted && dist <= a.radius));
        if (lane == 0) {  // this wave's word: no other wave touches it
          s_best[wave][q] = key < s_best[wave][q] ? key : s_best[wave][q];
          s_within[wave][q] += within;
        }
      }
    }
  }
  __syncthreads();
  if (tid < kTile && r0 + tid < a.R) {
    int best = s_best[0][tid], within = s_within[0][tid];
#pragma unroll
    for (int w = 1; w < kWaves; ++w) {
      best = s_best[w][tid] < best ? s_best[w][tid] : best;
      within += s_within[w][tid];
    }
    const int64_t slot = static_cast<int64_t>(chunk) * a.R + r0 + tid;
    const int dist = best >> kChunkBits;
    ws.key[slot] = dist >= kNone ? ~0ull
                                 : (static_cast<unsigned long long>(dist) << 32) | static_cast<unsigned long long>(m_begin + (best & (kChunk - 1)));
    ws.count[slot] = within;
  }
}

// ------------------------------------------------------------------ (3) per query, over the chunks
__global__ void __launch_bounds__(kThreads)
novelty_finish_kernel(const int32_t* __restrict__ q_len, const int32_t* __restrict__ lib_len, int R, int LQ, int LM, int chunks,
                      NoveltyWorkspace ws, int32_t* distance,
                      int32_t* index, int32_t* n_within, float* identity) {
  const int64_t r = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x;
  if (r >= R) return;
  unsigned long long best = ~0ull;
  int within = 0;
  for (int c = 0; c < chunks; ++c) {
    const unsigned long long key = ws.key[static_cast<int64_t>(c) * R + r];
    best = key < best ? key : best;
    within += ws.count[static_cast<int64_t>(c) * R + r];
  }
  const bool none = best == ~0ull;
  const int dist = none ? -1 : static_cast<int>(best >> 32), m = none ? -1 : static_cast<int>(best & 0xFFFFFFFFull);
  if (distance != nullptr) distance[r] = dist;
  if (index != nullptr) index[r] = m;
  if (n_within != nullptr) n_within[r] = within;
  if (identity != nullptr) {
    float v = NAN;
    if (!none) {
      const int lq = clamp_len(q_len[r], LQ), lm = clamp_len(lib_len[m], LM), longer = lq > lm ? lq : lm;
      v = longer == 0 ? 1.f : 1.f - __fdiv_rn(static_cast<float>(dist), static_cast<float>(longer));
    }
    identity[r] = v;
  }
}

// ------------------------------------------------------------------ the counted residues of a row as a sequence
// One wave per row: the counted slots of 64 slots at a time, each at its rank among them.
__global__ void __launch_bounds__(64)
novelty_pack_kernel(const int32_t* __restrict__ tokens, const uint8_t* __restrict__ mask, const uint8_t* __restrict__ residue_mask,
                    const int32_t* __restrict__ segment_idx, int segment, int group_size, int K, int L, uint8_t* out_tokens, int32_t* out_len) {
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
    if (counted && pos < L && out_tokens != nullptr) {
      const int tok = tokens[rbase + k];
      out_tokens[row * L + pos] = static_cast<uint8_t>(tok >= 0 && tok < kPad ? tok : kPad);
    }
    count += at.count;
  }
  if (out_tokens != nullptr)
    for (int p = count + lane; p < L; p += 64) out_tokens[row * L + p] = static_cast<uint8_t>(kPad);
  if (lane == 0 && out_len != nullptr) out_len[row] = count;
}

}  // namespace
}  // namespace diffab

using namespace diffab;

extern "C" {

int diffab_metrics_edit_nearest(const uint8_t* q_tokens, const int32_t* q_len, int32_t R, int32_t LQ, const uint8_t* lib_tokens,
                                const int32_t* lib_len, int32_t M, int32_t LM, const int32_t* skip, int32_t radius, int32_t* distance,
                                int32_t* index, int32_t* n_within, float* identity, int32_t* matrix, void* workspace, size_t workspace_bytes,
                                void* stream) {
  StreamOrder order_(stream);
  const char* who = "metrics_edit_nearest";
  DIFFAB_REQUIRE(R >= 0 && M >= 0, DIFFAB_ERR_ARG, "%s: negative extent (R = %d queries, M = %d library entries)", who, R, M);
  DIFFAB_REQUIRE(LQ >= 1 && LQ <= kMaxQuery, DIFFAB_ERR_ARG, "%s: LQ = %d tokens per query outside [1, %d]", who, LQ, kMaxQuery);
  DIFFAB_REQUIRE(LM >= 1 && LM <= kMaxLibrary, DIFFAB_ERR_ARG, "%s: LM = %d tokens per library entry outside [1, %d]", who, LM, kMaxLibrary);
  if (R == 0) return DIFFAB_OK;
  DIFFAB_REQUIRE(q_tokens && q_len, DIFFAB_ERR_ARG, "%s: null input (q_tokens, q_len)", who);
  DIFFAB_REQUIRE(M == 0 || (lib_tokens && lib_len), DIFFAB_ERR_ARG, "%s: null input (lib_tokens, lib_len) with M = %d", who, M);
  DIFFAB_REQUIRE(matrix == nullptr || static_cast<int64_t>(R) * M < (1ll << 31), DIFFAB_ERR_ARG,
                 "%s: matrix of R * M = %d * %d elements, fewer than 2^31 are needed", who, R, M);
  const NoveltyWorkspace ws = carve_novelty(workspace, R, M, LM);
  if (const int e = workspace_ok(who, workspace, 256, workspace_bytes, ws.bytes)) return e;
  hipStream_t st = as_stream(stream);
  const int chunks = (M + kChunk - 1) / kChunk;
  if (M > 0) {
    hipLaunchKernelGGL(novelty_repack_kernel, dim3(chunks), dim3(kThreads), 0, st, lib_tokens, lib_len, M, LM, ws);
    NearestArgs a;
    a.q_tokens = q_tokens, a.q_len = q_len, a.skip = skip, a.matrix = matrix;
    a.R = R, a.LQ = LQ, a.M = M, a.radius = radius, a.chunks = chunks;
    const int tiles = (R + kTile - 1) / kTile, per_launch = kMaxBlocks / chunks > 0 ? kMaxBlocks / chunks : 1;
    for (int t0 = 0; t0 < tiles; t0 += per_launch) {
      const int n = tiles - t0 < per_launch ? tiles - t0 : per_launch;
      a.tile0 = t0;
      hipLaunchKernelGGL(novelty_distance_kernel, dim3(static_cast<unsigned>(n) * static_cast<unsigned>(chunks)), dim3(kThreads), 0, st, a, ws);
    }
  }
  if (distance != nullptr || index != nullptr || n_within != nullptr || identity != nullptr)
    hipLaunchKernelGGL(novelty_finish_kernel, dim3((R + kThreads - 1) / kThreads), dim3(kThreads), 0, st, q_len, lib_len, R, LQ, LM, chunks, ws, distance,
                       index, n_within, identity);
  DIFFAB_LAUNCH_CHECK();
  return DIFFAB_OK;
}

int diffab_metrics_pack_sequences(const int32_t* tokens, const uint8_t* mask, const uint8_t* residue_mask, const int32_t* segment_idx,
                                  int32_t segment, int32_t rows, int32_t group_size, int32_t K, int32_t L, uint8_t* out_tokens,
                                  int32_t* out_len, void* stream) {
  StreamOrder order_(stream);
  const char* who = "metrics_pack_sequences";
  if (!rows_shape_ok(who, rows, group_size, K, DIFFAB_NOVELTY_PACK_MAX_K)) return DIFFAB_ERR_ARG;
  DIFFAB_REQUIRE(L >= 1 && L <= kMaxLibrary, DIFFAB_ERR_ARG, "%s: L = %d tokens per sequence outside [1, %d]", who, L, kMaxLibrary);
  if (rows == 0) return DIFFAB_OK;
  DIFFAB_REQUIRE(tokens && mask, DIFFAB_ERR_ARG, "%s: null input (tokens, mask)", who);
  if (out_tokens == nullptr && out_len == nullptr) return DIFFAB_OK;
  hipLaunchKernelGGL(novelty_pack_kernel, dim3(rows), dim3(64), 0, as_stream(stream), tokens, mask, residue_mask, segment_idx, segment, group_size,
                     K, L, out_tokens, out_len);
  DIFFAB_LAUNCH_CHECK();
  return DIFFAB_OK;
}

}  // extern "C"
