// interface_kernels.hip - the interface of a design as a set, on the device: diffab_metrics_contact_bits, the
// contacts diffab_metrics_contacts counts kept as a bit map per design, and diffab_metrics_pairwise_bits, the overlap of such sets between
// all the designs of a patch (the fraction of common contacts, Jaccard).  The rules are the header comments of the two entries in
// include/diffab_hip_interface.h.
//
// Built with -ffp-contract=off like the other defined numbers (csrc/Makefile): the squared distance is dist2 of analysis_common.h, as
// in diffab_metrics_contacts (csrc/geometry_kernels.hip), and a contact is one strict comparison on it.  The two quotients are plain fp32 divisions of exact integers - the build has no fast-math
// flag, so they are correctly rounded.  Everything else is integer work on bits: ballots, ORs, ANDs, popcounts, adds.  VALU + LDS only;
// no atomics; every value reaches memory through plain C++ stores.
#include <climits>
#include <cmath>

#include "../../include/diffab_hip_interface.h"
#include "analysis_prep.h"

namespace diffab {
namespace {

constexpr int kMaxGroup = DIFFAB_METRICS_MAX_GROUP;
constexpr int kMaxPoints = DIFFAB_METRICS_MAX_POINTS;
constexpr int kMaxContextAtoms = DIFFAB_METRICS_MAX_CONTEXT_ATOMS;
constexpr int kMaxK = DIFFAB_INTERFACE_MAX_K;
constexpr int kMaxWords = DIFFAB_INTERFACE_MAX_WORDS;
constexpr int kColumnAtoms = 32 * kMaxContextAtoms;  // the most atoms the 32 residues of one word column have
constexpr int kTileColumns = DIFFAB_INTERFACE_TILE_COLUMNS;
static_assert(kMaxK % 64 == 0 && kMaxWords == kMaxK * (kMaxK / 32), "a contact map of the largest patch is the longest set");
static_assert(static_cast<long long>(kMaxWords) * 32 < (1 << 24), "every count is exact as an fp32 number");

constexpr int pad64(int n) { return (n + 63) / 64 * 64; }

// ------------------------------------------------------------------ 1. contact bits
// The workspace of diffab_metrics_contact_bits (DIFFAB_METRICS_CONTACT_BITS_WORKSPACE_BYTES covers the carves and their alignment) is the
// ContextWorkspace of analysis_prep.h, then wstart (G, W + 1).  context_pack_kernel<true, kMaxK> fills both: the pack of
// diffab_metrics_contacts, with the antigen mask as part of the listing and the start of every word column noted on the way.
//
// One work-group per (patch, 64 designs): lane = design, the four waves share the staged antigen atoms and split the generated residues.
// The listed residues go through LDS one word column (32 slots) at a time; every lane reads the same antigen atom (an LDS broadcast)
// against the atoms of its own design, held in registers.  The word of (design, generated residue i, column w) is built by one thread in
// one register and stored once; a column without a listed residue stores zero without staging anything.  The rows of the other residues
// are zero: the work-group sweeps the K * W words of each of its designs in address order and stores the zeros of the rows that are not
// in the generated list - the two kinds of store never meet, so nothing is written twice and no order between them is needed.
template <int P>
__global__ void __launch_bounds__(256)
contact_bits_kernel(const float* __restrict__ points, const uint8_t* __restrict__ valid, const int32_t* __restrict__ chain,
                    const int32_t* __restrict__ residue_idx, int N, int K, int A, float contact2, ContextWorkspace ws,
                    const int32_t* __restrict__ wstarts, uint32_t* __restrict__ bits, int32_t* __restrict__ n_contacts) {
  __shared__ float4 s_atom[kColumnAtoms];
  __shared__ int4 s_res[32];  // slot, first atom in s_atom, atoms
  __shared__ int2 s_key[32];
  __shared__ uint8_t s_listed[kMaxK];  // 1: the slot is in the generated list (its words are stored by their owners)
  __shared__ int s_count[4][64];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int blocks = (N + 63) / 64, W = (K + 31) / 32;
  const int64_t g = blockIdx.x / blocks;
  const int d0 = (blockIdx.x % blocks) * 64, d = d0 + lane;
  const bool active = d < N;
  const int64_t row = g * N + (active ? d : N - 1);  // (an idle lane reads the last design and stores nothing)
  const int4 hdr = ws.hdr[g];
  const int ng = hdr.x;
  const int32_t* gen = ws.gen + g * K;
  const int4* res = ws.res + g * K;
  const int2* key = ws.key + g * K;
  const float4* atoms = ws.atoms + g * K * A;
  const int32_t* wstart = wstarts + g * (W + 1);
  const float* pp = points + row * K * P * 3;
  const uint8_t* vv = valid + row * K;
  const int32_t* ch = chain + g * K;
  const int32_t* ri = residue_idx + g * K;

  for (int k = tid; k < K; k += 256) s_listed[k] = 0;
  __syncthreads();
  for (int gi = tid; gi < ng; gi += 256) s_listed[gen[gi]] = 1;
  __syncthreads();
  {  // the zero rows of this work-group's designs: K * W contiguous words per design
    const int nd = N - d0 < 64 ? N - d0 : 64;
    const int per = K * W;
    uint32_t* out = bits + (g * N + d0) * per;
    for (int e = tid; e < nd * per; e += 256)
      if (!s_listed[(e % per) / W]) out[e] = 0u;
  }

  int count = 0;
  for (int w = 0; w < W; ++w) {
    const int r0 = wstart[w], nres = wstart[w + 1] - r0;  // (uniform; at most 32)
    if (nres > 0) {
      const int first = res[r0].y;
      const int4 last = res[r0 + nres - 1];
      const int natoms = last.y + last.z - first;
      __syncthreads();  // the column before is done with
      for (int t = tid; t < natoms; t += 256) s_atom[t] = atoms[first + t];
      if (tid < nres) {
        const int4 r = res[r0 + tid];
        s_res[tid] = make_int4(r.x, r.y - first, r.z, 0);
        s_key[tid] = key[r0 + tid];
      }
      __syncthreads();
    }
    for (int gi = wave; gi < ng; gi += 4) {
      const int i = gen[gi];
      uint32_t word = 0u;
      if (nres > 0) {
        float px[P], py[P], pz[P];
#pragma unroll
        for (int a = 0; a < P; ++a) px[a] = pp[(i * P + a) * 3], py[a] = pp[(i * P + a) * 3 + 1], pz[a] = pp[(i * P + a) * 3 + 2];
        const uint32_t pv = active ? vv[i] : 0u;
        const int ci = ch[i], rri = ri[i];
        for (int rl = 0; rl < nres; ++rl) {
          const int4 r = s_res[rl];
          const int2 kk = s_key[rl];
          if (bonded(ci, rri, kk.x, kk.y)) continue;
          bool near = false;
          for (int b = r.y; b < r.y + r.z; ++b) {
            const float4 q = s_atom[b];
#pragma unroll
            for (int a = 0; a < P; ++a) {
              near |= masked_dist2(px[a], py[a], pz[a], q.x, q.y, q.z, ((pv >> a) & 1u) != 0u) < contact2;
            }
          }
          if (near) word |= 1u << (r.x & 31);
        }
      }
      if (active) bits[(row * K + i) * W + w] = word;  // (this thread alone writes word (row, i, w))
      count += __popc(word);
    }
  }

  s_count[wave][lane] = count;
  __syncthreads();
  if (wave == 0 && active) n_contacts[row] = (s_count[0][lane] + s_count[1][lane]) + (s_count[2][lane] + s_count[3][lane]);
}

// ------------------------------------------------------------------ 2. pairwise bits
// Workspace of diffab_metrics_pairwise_bits (DIFFAB_METRICS_PAIRWISE_BITS_WORKSPACE_BYTES covers the carves and their alignment).
struct PairBitsWorkspace {
  uint32_t* live;   // (G, L, Np): word cols[ci] of design d at [g][ci][d], zero for d >= N; only the first ncols[g] columns are written
  uint32_t* part;   // (G, S, L): the OR of the words of designs 64 s .. 64 s + 63, per column
  int32_t* cols;    // (G, L): the columns that are not zero in every design, ascending
  int32_t* ncols;   // (G)
  size_t bytes;
};

PairBitsWorkspace carve_pair_bits(void* base, int64_t G, int64_t N, int64_t L) {
  const int64_t Np = (N + 63) / 64 * 64, S = Np / 64;
  Carver c(base);
  PairBitsWorkspace w;
  w.live = c.take<uint32_t>(static_cast<size_t>(G * L * Np));
  w.part = c.take<uint32_t>(static_cast<size_t>(G * S * L));
  w.cols = c.take<int32_t>(static_cast<size_t>(G * L));
  w.ncols = c.take<int32_t>(static_cast<size_t>(G));
  w.bytes = c.bytes();
  return w;
}

// (1) One work-group per (patch, 64 designs): thread = column (coalesced along the words of a design), eight designs in flight.
__global__ void __launch_bounds__(256)
pair_bits_or_kernel(const uint32_t* __restrict__ bits, int N, int L, int S, PairBitsWorkspace ws) {
  const int64_t g = blockIdx.x / S;
  const int s = blockIdx.x % S;
  const int d0 = s * 64, nd = N - d0 < 64 ? N - d0 : 64;
  const uint32_t* in = bits + (g * N + d0) * L;
  for (int c = threadIdx.x; c < L; c += 256) {
    uint32_t acc = 0u;
    int d = 0;
    for (; d + 8 <= nd; d += 8) {
      uint32_t v[8];
#pragma unroll
      for (int q = 0; q < 8; ++q) v[q] = in[static_cast<int64_t>(d + q) * L + c];
#pragma unroll
      for (int q = 0; q < 8; ++q) acc |= v[q];
    }
    for (; d < nd; ++d) acc |= in[static_cast<int64_t>(d) * L + c];
    ws.part[(g * S + s) * L + c] = acc;
  }
}

// (2) One work-group per patch: the OR over the parts, then wave 0 lists the live columns in ascending order with ballots.
__global__ void __launch_bounds__(256)
pair_bits_compact_kernel(int L, int S, PairBitsWorkspace ws) {
  __shared__ uint8_t s_live[kMaxWords];
  const int tid = threadIdx.x, lane = tid & 63;
  const int64_t g = blockIdx.x;
  for (int c = tid; c < L; c += 256) {
    uint32_t acc = 0u;
    for (int s = 0; s < S; ++s) acc |= ws.part[(g * S + s) * L + c];
    s_live[c] = acc != 0u;
  }
  __syncthreads();
  if (tid >= 64) return;
  int n = 0;
  const unsigned long long below = (1ull << lane) - 1ull;
  for (int c0 = 0; c0 < L; c0 += 64) {
    const int c = c0 + lane;
    const bool live = c < L && s_live[c] != 0;
    const unsigned long long v = __ballot(live);
    if (live) ws.cols[g * L + n + __popcll(v & below)] = c;
    n += __popcll(v);
  }
  if (lane == 0) ws.ncols[g] = n;
}

// (3) One work-group per (patch, 64 designs of the padded patch): lane = design, so the stores are whole 256-byte rows; a lane walks the
// live words of its own design in ascending order (neighbouring words of a row share a cache line), the four waves take every fourth.
__global__ void __launch_bounds__(256)
pair_bits_gather_kernel(const uint32_t* __restrict__ bits, int N, int Np, int L, PairBitsWorkspace ws) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int S = Np / 64;
  const int64_t g = blockIdx.x / S;
  const int d = (blockIdx.x % S) * 64 + lane;
  const int nc = ws.ncols[g];
  const int32_t* cols = ws.cols + g * L;
  const uint32_t* in = bits + (g * N + (d < N ? d : 0)) * L;
  uint32_t* out = ws.live + g * L * Np;
  for (int ci = wave; ci < nc; ci += 4) {
    const uint32_t v = in[cols[ci]];
    out[static_cast<int64_t>(ci) * Np + d] = d < N ? v : 0u;
  }
}

// (4) One work-group per 64 x 64 block of pairs (a in block bi, b in block bj >= bi).  Thread (ty, tx) = (tid / 16, tid % 16) owns the
// pairs a = 4 ty .. 4 ty + 3, b = 4 tx .. 4 tx + 3.  LDS: word c of design d at [c][d], so a thread's four a words and four b words are
// one 128-bit read each; in a wave the a read has four addresses (a broadcast) and the b read covers 64 consecutive words, every bank
// once.  After the last chunk the counts go to s_out[a][b] (row stride 65: the mirror reads a column without a conflict) and every
// store of the block and of its mirror is a row of 64 consecutive elements.
__global__ void __launch_bounds__(256)
pair_bits_tile_kernel(int N, int Np, int L, PairBitsWorkspace ws, int32_t* __restrict__ n_set, int32_t* __restrict__ n_common,
                      float* __restrict__ fcc, float* __restrict__ jaccard) {
  __shared__ __attribute__((aligned(16))) uint32_t s_a[kTileColumns * 64];
  __shared__ __attribute__((aligned(16))) uint32_t s_b[kTileColumns * 64];
  __shared__ int s_out[64 * 65];
  __shared__ int s_na[64], s_nb[64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int ty = tid >> 4, tx = tid & 15;
  const int T = Np / 64, per_patch = T * (T + 1) / 2;
  const int64_t g = blockIdx.x / per_patch;
  int t = blockIdx.x % per_patch, bi = 0;
  while (t >= T - bi) {  // (uniform) row bi of the upper triangle holds T - bi blocks
    t -= T - bi;
    ++bi;
  }
  const int bj = bi + t;
  const int a0 = bi * 64, b0 = bj * 64;
  const int nc = ws.ncols[g];
  const uint32_t* live = ws.live + g * L * Np;

  int acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = 0;
  int own = 0;  // waves 0 and 1: the popcount of design a0 + lane / b0 + lane

  for (int c0 = 0; c0 < nc; c0 += kTileColumns) {
    const int ch = nc - c0 < kTileColumns ? nc - c0 : kTileColumns;
    __syncthreads();  // the chunk before is done with
    for (int cc = wave; cc < ch; cc += 4) {
      const uint32_t* col = live + static_cast<int64_t>(c0 + cc) * Np;
      s_a[cc * 64 + lane] = col[a0 + lane];
      s_b[cc * 64 + lane] = col[b0 + lane];
    }
    __syncthreads();
    if (wave < 2) {
      const uint32_t* mine = wave == 0 ? s_a : s_b;
      for (int cc = 0; cc < ch; ++cc) own += __popc(mine[cc * 64 + lane]);
    }
    for (int cc = 0; cc < ch; ++cc) {
      const uint4 va = *reinterpret_cast<const uint4*>(&s_a[cc * 64 + 4 * ty]);
      const uint4 vb = *reinterpret_cast<const uint4*>(&s_b[cc * 64 + 4 * tx]);
      const uint32_t a[4] = {va.x, va.y, va.z, va.w}, b[4] = {vb.x, vb.y, vb.z, vb.w};
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] += __popc(a[i] & b[j]);
    }
  }

#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) s_out[(4 * ty + i) * 65 + 4 * tx + j] = acc[i][j];
  if (wave == 0) s_na[lane] = own;
  if (wave == 1) s_nb[lane] = own;
  __syncthreads();

  if (n_set != nullptr && bi == bj && wave == 0 && a0 + lane < N) n_set[g * N + a0 + lane] = s_na[lane];
  const int64_t base = g * N * N;
  // the block itself: row a0 + r, columns b0 + lane
  const int b = b0 + lane;
  if (b < N) {
    const int nb = s_nb[lane];
    for (int r = wave; r < 64 && a0 + r < N; r += 4) {
      const int c = s_out[r * 65 + lane], na = s_na[r];
      const int64_t at = base + static_cast<int64_t>(a0 + r) * N + b;
      if (n_common != nullptr) n_common[at] = c;
      if (fcc != nullptr) fcc[at] = na == 0 ? 1.f : static_cast<float>(c) / static_cast<float>(na);
      if (jaccard != nullptr) {
        const int u = na + nb - c;
        jaccard[at] = u == 0 ? 1.f : static_cast<float>(c) / static_cast<float>(u);
      }
    }
  }
  if (bi == bj) return;  // (uniform) a diagonal block is its own mirror
  // the mirror: row b0 + r, columns a0 + lane, from the same integers
  const int a = a0 + lane;  // (< N: bi < bj, so block bi is a whole block)
  const int na = s_na[lane];
  for (int r = wave; r < 64 && b0 + r < N; r += 4) {
    const int c = s_out[lane * 65 + r], nb = s_nb[r];
    const int64_t at = base + static_cast<int64_t>(b0 + r) * N + a;
    if (n_common != nullptr) n_common[at] = c;
    if (fcc != nullptr) fcc[at] = nb == 0 ? 1.f : static_cast<float>(c) / static_cast<float>(nb);
    if (jaccard != nullptr) {
      const int u = na + nb - c;
      jaccard[at] = u == 0 ? 1.f : static_cast<float>(c) / static_cast<float>(u);
    }
  }
}

}  // namespace
}  // namespace diffab

using namespace diffab;

extern "C" {

int diffab_metrics_contact_bits(const float* points, const uint8_t* valid, const float* context_points, const uint32_t* context_valid,
                                const uint8_t* generation_mask, const uint8_t* residue_mask, const uint8_t* antigen_mask,
                                const int32_t* chain, const int32_t* residue_idx, int32_t rows, int32_t group_size, int32_t K, int32_t P,
                                int32_t A, float contact_distance, int32_t* bits, int32_t* n_contacts, void* workspace,
                                size_t workspace_bytes, void* stream) {
  StreamOrder order_(stream);
  const char* who = "metrics_contact_bits";
  if (!rows_shape_ok(who, rows, group_size, K, kMaxK)) return DIFFAB_ERR_ARG;
  DIFFAB_REQUIRE(P >= 1 && P <= kMaxPoints, DIFFAB_ERR_ARG, "%s: P = %d points per residue outside [1, %d]", who, P, kMaxPoints);
  DIFFAB_REQUIRE(A >= 1 && A <= kMaxContextAtoms, DIFFAB_ERR_ARG, "%s: A = %d context atoms per residue outside [1, %d]", who, A,
                 kMaxContextAtoms);
  DIFFAB_REQUIRE(finite_nonnegative(contact_distance), DIFFAB_ERR_ARG,
                 "%s: contact_distance must be finite and >= 0, got %g", who, static_cast<double>(contact_distance));
  if (rows == 0) return DIFFAB_OK;
  DIFFAB_REQUIRE(points && valid && context_points && context_valid && generation_mask && antigen_mask && chain && residue_idx,
                 DIFFAB_ERR_ARG, "%s: null input", who);
  DIFFAB_REQUIRE(bits != nullptr && n_contacts != nullptr, DIFFAB_ERR_ARG, "%s: null output", who);
  const int32_t G = rows / group_size;
  Carver carver(workspace);
  const ContextWorkspace ws = carve_context(carver, G, K, A);
  int32_t* wstart = carver.take<int32_t>(static_cast<size_t>(G) * ((K + 31) / 32 + 1));
  if (const int e = workspace_ok(who, workspace, 256, workspace_bytes, carver.bytes())) return e;
  const int64_t grid = static_cast<int64_t>(G) * ((group_size + 63) / 64);
  DIFFAB_REQUIRE(grid <= INT_MAX, DIFFAB_ERR_UNSUPPORTED, "%s: %d rows are more work-groups than one launch holds", who, rows);
  hipStream_t st = as_stream(stream);
  hipLaunchKernelGGL((context_pack_kernel<true, kMaxK>), dim3(G), dim3(256), 0, st, context_points, context_valid, generation_mask,
                     residue_mask, antigen_mask, static_cast<const uint8_t*>(nullptr), chain, residue_idx, K, A, ws, wstart);
  const float contact2 = contact_distance * contact_distance;
  uint32_t* out = reinterpret_cast<uint32_t*>(bits);
#define DIFFAB_CONTACT_BITS_LAUNCH(PP)                                                                                                    \
  hipLaunchKernelGGL((contact_bits_kernel<PP>), dim3(static_cast<unsigned>(grid)), dim3(256), 0, st, points, valid, chain, residue_idx, \
                     group_size, K, A, contact2, ws, wstart, out, n_contacts)
  switch (P) {
    case 1: DIFFAB_CONTACT_BITS_LAUNCH(1); break;
    case 2: DIFFAB_CONTACT_BITS_LAUNCH(2); break;
    case 3: DIFFAB_CONTACT_BITS_LAUNCH(3); break;
    case 4: DIFFAB_CONTACT_BITS_LAUNCH(4); break;
    default: DIFFAB_CONTACT_BITS_LAUNCH(5); break;
  }
#undef DIFFAB_CONTACT_BITS_LAUNCH
  DIFFAB_LAUNCH_CHECK();
  return DIFFAB_OK;
}

int diffab_metrics_pairwise_bits(const int32_t* bits, int32_t G, int32_t N, int32_t L, int32_t* n_set, int32_t* n_common, float* fcc,
                                 float* jaccard, void* workspace, size_t workspace_bytes, void* stream) {
  StreamOrder order_(stream);
  const char* who = "metrics_pairwise_bits";
  DIFFAB_REQUIRE(G >= 0 && N >= 1 && L >= 1, DIFFAB_ERR_ARG, "%s: negative or empty extent (G = %d, N = %d, L = %d)", who, G, N, L);
  DIFFAB_REQUIRE(N <= kMaxGroup, DIFFAB_ERR_ARG, "%s: N = %d, at most %d designs per group", who, N, kMaxGroup);
  DIFFAB_REQUIRE(L <= kMaxWords, DIFFAB_ERR_ARG, "%s: L = %d words per design, at most %d", who, L, kMaxWords);
  if (G == 0) return DIFFAB_OK;
  DIFFAB_REQUIRE(bits != nullptr, DIFFAB_ERR_ARG, "%s: null input", who);
  const PairBitsWorkspace ws = carve_pair_bits(workspace, G, N, L);
  if (const int e = workspace_ok(who, workspace, 256, workspace_bytes, ws.bytes)) return e;
  const int Np = pad64(N), S = Np / 64;
  const int64_t tiles = static_cast<int64_t>(G) * (S * (S + 1) / 2);
  DIFFAB_REQUIRE(tiles <= INT_MAX, DIFFAB_ERR_UNSUPPORTED, "%s: G = %d groups of N = %d are more tiles than one launch holds", who, G, N);
  if (n_set == nullptr && n_common == nullptr && fcc == nullptr && jaccard == nullptr) return DIFFAB_OK;  // nothing was asked for
  hipStream_t st = as_stream(stream);
  const uint32_t* in = reinterpret_cast<const uint32_t*>(bits);
  const unsigned segments = static_cast<unsigned>(G) * static_cast<unsigned>(S);
  hipLaunchKernelGGL(pair_bits_or_kernel, dim3(segments), dim3(256), 0, st, in, N, L, S, ws);
  hipLaunchKernelGGL(pair_bits_compact_kernel, dim3(G), dim3(256), 0, st, L, S, ws);
  hipLaunchKernelGGL(pair_bits_gather_kernel, dim3(segments), dim3(256), 0, st, in, N, Np, L, ws);
  hipLaunchKernelGGL(pair_bits_tile_kernel, dim3(static_cast<unsigned>(tiles)), dim3(256), 0, st, N, Np, L, ws, n_set, n_common, fcc, jaccard);
  DIFFAB_LAUNCH_CHECK();
  return DIFFAB_OK;
}

}  // extern "C"
