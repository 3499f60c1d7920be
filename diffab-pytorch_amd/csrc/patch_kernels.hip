// patch_kernels.hip - patch construction from a whole complex on the device: which K residues of an N-residue
// antibody-antigen complex the sampler sees (the reference's preprocess_pdb.py:44-58: the nearest-k residues around the CDR anchors united
// with the nearest-k antigen residues, then residue_masked_select), the gather of every per-residue field to patch size and the scatter
// of the designs back into the complex.  The definition of the selection is the header comment of diffab_patch_select.
//
// Built with -ffp-contract=off (csrc/Makefile): the selection key ((dx*dx + dy*dy) + dz*dz) is then a defined fp32 number, and the patch
// is the same set whatever the compiler would have fused.  VALU + LDS only; every value reaches memory through plain C++ stores.
#include <climits>

#include "common.h"

namespace diffab {
namespace {

constexpr int kSelThreads = 1024;                    // one work-group per complex
constexpr int kSelMaxN = DIFFAB_PATCH_MAX_RESIDUES;  // keys of the whole complex resident in LDS: 4096 x 8 B = 32 KiB
constexpr int kSelPerThread = kSelMaxN / kSelThreads;
constexpr int kAnchorTile = 1024;                    // anchors staged per pass of the min-distance loop (16 KiB as float4)
constexpr int kSelWords = kSelMaxN / 32;
constexpr uint32_t kAbsent = 0xFFFFFFFFu;            // key word of a residue that is not present (and of the sort's padding)

// Exclusive prefix sum of the set bits of `bits` (kSelWords 32-bit words) into off[0 .. kSelWords), the total into off[kSelWords].
// Run by the first wave (64 lanes, two words each); the caller puts barriers around it.
__device__ inline void bit_offsets(const uint32_t* bits, int* off) {
  const int lane = threadIdx.x;
  if (lane >= 64) return;
  static_assert(kSelWords == 128, "two words per lane of one wave");
  const int c0 = __popc(bits[2 * lane]), c1 = __popc(bits[2 * lane + 1]);
  int incl = c0 + c1;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const int up = __shfl_up(incl, d, 64);
    if (lane >= d) incl += up;
  }
  const int excl = incl - (c0 + c1);
  off[2 * lane] = excl;
  off[2 * lane + 1] = excl + c0;
  if (lane == 63) off[kSelWords] = incl;
}

__device__ inline int bit_rank(const uint32_t* bits, const int* off, int i) {
  return off[i >> 5] + __popc(bits[i >> 5] & ((1u << (i & 31)) - 1u));
}

// ca: CA of residue (b, i) at ca[(b * N + i) * ca_stride + 0..2].  P: the sort's extent, a power of two with N <= P <= kSelMaxN.
__global__ void __launch_bounds__(kSelThreads)
patch_select_kernel(const float* __restrict__ ca, int ca_stride, const uint8_t* __restrict__ residue_mask,
                    const uint8_t* __restrict__ generation_mask, const uint8_t* __restrict__ anchor_mask,
                    const int64_t* __restrict__ chain_idx, const uint8_t* __restrict__ antigen_mask, int N, int P, int k, int k_antigen,
                    int K, int64_t* __restrict__ index, uint8_t* __restrict__ patch_mask, int32_t* __restrict__ count) {
  __shared__ uint64_t s_key[kSelMaxN];        // (key word << 32) | residue index, sorted ascending
  __shared__ float4 s_anchor[kAnchorTile];    // anchor coordinates of the current tile
  __shared__ uint16_t s_alist[kSelMaxN];      // residue indices of the anchors (any order: a minimum does not care)
  __shared__ uint32_t s_forced[kSelWords];    // bit i: residue i is an anchor or a present generated residue (key -1)
  __shared__ uint32_t s_bits[kSelWords];      // antigen pass: bit j: sorted slot j holds a present antigen residue
  __shared__ uint32_t s_sel[kSelWords];       // bit i: residue i is in the patch
  __shared__ int s_off[kSelWords + 1];
  __shared__ int s_n[3];                      // anchors, present generated residues, forced residues

  const int tid = threadIdx.x;
  const int b = blockIdx.x;
  const int64_t base = static_cast<int64_t>(b) * N;
  const uint8_t* rm = residue_mask ? residue_mask + base : nullptr;
  const uint8_t* gm = generation_mask + base;
  const uint8_t* am = anchor_mask ? anchor_mask + base : nullptr;
  const uint8_t* ag = antigen_mask ? antigen_mask + base : nullptr;
  const int64_t* ch = chain_idx ? chain_idx + base : nullptr;
  int64_t* out_index = index + static_cast<int64_t>(b) * K;
  uint8_t* out_mask = patch_mask + static_cast<int64_t>(b) * K;

  auto present = [&](int i) { return rm == nullptr || rm[i] != 0; };
  auto generated = [&](int i) { return present(i) && gm[i] != 0; };
  auto flanks = [&](int i, int j) { return j >= 0 && j < N && generated(j) && (ch == nullptr || ch[j] == ch[i]); };

  for (int w = tid; w < kSelWords; w += kSelThreads) s_forced[w] = s_bits[w] = s_sel[w] = 0u;
  if (tid < 3) s_n[tid] = 0;
  __syncthreads();

  // ---- 1. anchors.  use_generated: the fallback of a complex whose generated residues have no anchor.
  auto mark = [&](bool use_generated) {
    for (int i = tid; i < N; i += kSelThreads) {
      const bool gen = generated(i);
      bool anchor;
      if (use_generated)
        anchor = gen;
      else if (am)
        anchor = present(i) && am[i] != 0;
      else
        anchor = present(i) && !gen && (flanks(i, i - 1) || flanks(i, i + 1));
      if (anchor) s_alist[atomicAdd(&s_n[0], 1)] = static_cast<uint16_t>(i);
      if (!use_generated && gen) atomicAdd(&s_n[1], 1);
      if (anchor || gen) atomicOr(&s_forced[i >> 5], 1u << (i & 31));
    }
    __syncthreads();
  };
  mark(false);
  const bool fallback = s_n[0] == 0 && s_n[1] > 0;  // (uniform: read between two barriers)
  __syncthreads();
  if (fallback) mark(true);
  const int n_anchor = s_n[0];
  if (tid < kSelWords / 2) atomicAdd(&s_n[2], __popc(s_forced[2 * tid]) + __popc(s_forced[2 * tid + 1]));
  __syncthreads();
  const int n_generated = s_n[1], n_forced = s_n[2];
  if (n_generated == 0 || n_forced > k) {  // nothing to design / the forced residues alone overflow k: an empty row
    for (int p = tid; p < K; p += kSelThreads) {
      out_index[p] = -1;
      out_mask[p] = 0;
    }
    if (tid == 0) count[b] = n_generated == 0 ? 0 : -1;
    return;
  }

  // ---- 2. key = min over anchors of the squared CA distance, in the header's association
  float px[kSelPerThread], py[kSelPerThread], pz[kSelPerThread], best[kSelPerThread];
#pragma unroll
  for (int r = 0; r < kSelPerThread; ++r) {
    const int i = tid + r * kSelThreads;
    best[r] = INFINITY;
    px[r] = py[r] = pz[r] = 0.f;
    if (i < N) {
      const float* c = ca + (base + i) * ca_stride;
      px[r] = c[0], py[r] = c[1], pz[r] = c[2];
    }
  }
  for (int a0 = 0; a0 < n_anchor; a0 += kAnchorTile) {
    const int na = min(kAnchorTile, n_anchor - a0);
    __syncthreads();
    for (int a = tid; a < na; a += kSelThreads) {
      const float* c = ca + (base + s_alist[a0 + a]) * ca_stride;
      s_anchor[a] = make_float4(c[0], c[1], c[2], 0.f);
    }
    __syncthreads();
    for (int a = 0; a < na; ++a) {
      const float4 q = s_anchor[a];  // one address for the whole wave: an LDS broadcast
#pragma unroll
      for (int r = 0; r < kSelPerThread; ++r) {
        const float dx = px[r] - q.x, dy = py[r] - q.y, dz = pz[r] - q.z;
        best[r] = fminf(best[r], (dx * dx + dy * dy) + dz * dz);
      }
    }
  }

  // ---- 3. order by (key, index): non-negative floats order as their bit patterns; forced residues sort first, absent ones last
#pragma unroll
  for (int r = 0; r < kSelPerThread; ++r) {
    const int i = tid + r * kSelThreads;
    if (i < P) {
      uint32_t word = kAbsent;
      if (i < N && present(i)) word = (s_forced[i >> 5] >> (i & 31)) & 1u ? 0u : __float_as_uint(best[r]) + 1u;
      s_key[i] = (static_cast<uint64_t>(word) << 32) | static_cast<uint32_t>(i);
    }
  }
  __syncthreads();
  for (int span = 2; span <= P; span <<= 1) {  // bitonic sort, ascending
    for (int j = span >> 1; j > 0; j >>= 1) {
      for (int t = tid; t < (P >> 1); t += kSelThreads) {
        const int lo = 2 * t - (t & (j - 1)), hi = lo + j;
        const uint64_t u = s_key[lo], v = s_key[hi];
        if ((u > v) == ((lo & span) == 0)) {
          s_key[lo] = v;
          s_key[hi] = u;
        }
      }
      __syncthreads();
    }
  }

  // S1: the first k present residues.  S2: the first k_antigen present antigen residues, ranked by a prefix count over the sorted slots.
  for (int j = tid; j < min(k, P); j += kSelThreads) {
    const uint64_t w = s_key[j];
    if (static_cast<uint32_t>(w >> 32) != kAbsent) {
      const uint32_t i = static_cast<uint32_t>(w);
      atomicOr(&s_sel[i >> 5], 1u << (i & 31));
    }
  }
  if (k_antigen > 0) {
    for (int j = tid; j < P; j += kSelThreads) {
      const uint64_t w = s_key[j];
      if (static_cast<uint32_t>(w >> 32) != kAbsent && ag[static_cast<uint32_t>(w)] != 0) atomicOr(&s_bits[j >> 5], 1u << (j & 31));
    }
    __syncthreads();
    bit_offsets(s_bits, s_off);
    __syncthreads();
    for (int j = tid; j < P; j += kSelThreads) {
      if (((s_bits[j >> 5] >> (j & 31)) & 1u) && bit_rank(s_bits, s_off, j) < k_antigen) {
        const uint32_t i = static_cast<uint32_t>(s_key[j]);
        atomicOr(&s_sel[i >> 5], 1u << (i & 31));
      }
    }
  }
  __syncthreads();

  // ---- 4. the patch in ascending residue index
  bit_offsets(s_sel, s_off);
  __syncthreads();
  const int n_sel = min(s_off[kSelWords], K);  // (<= k + k_antigen <= K by construction; the clamp keeps every store inside the row)
  for (int i = tid; i < N; i += kSelThreads) {
    if ((s_sel[i >> 5] >> (i & 31)) & 1u) {
      const int p = bit_rank(s_sel, s_off, i);
      if (p < K) out_index[p] = i;
    }
  }
  for (int p = tid; p < K; p += kSelThreads) {
    if (p >= n_sel) out_index[p] = -1;
    out_mask[p] = p < n_sel ? 1 : 0;
  }
  if (tid == 0) count[b] = n_sel;
}

// Rows of a launch read their complex through a map passed by value (a HOST array of the caller: no device copy, no workspace).
constexpr int kMapRows = 256;
struct RowMap {
  int32_t complex_of_row[kMapRows];
};

// Lane: the widest unit (16, 4 or 1 bytes) that divides row_bytes and both base addresses.  lanes = row_bytes / sizeof(Lane).
template <typename Lane, bool kMapped>
__global__ void __launch_bounds__(256)
patch_gather_kernel(const Lane* __restrict__ src, const int64_t* __restrict__ index, RowMap map, int row0, int64_t slots, int N, int K,
                    int64_t lanes, Lane* __restrict__ dst) {
  const int64_t total = slots * lanes;
  for (int64_t e = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x; e < total; e += static_cast<int64_t>(gridDim.x) * blockDim.x) {
    const int64_t slot = e / lanes, l = e - slot * lanes;  // slot = (row - row0) * K + p
    const int64_t r = slot / K;
    const int64_t c = kMapped ? map.complex_of_row[r] : row0 + r;
    const int64_t gslot = static_cast<int64_t>(row0) * K + slot;
    const int64_t i = index[gslot];
    Lane v = Lane();
    if (i >= 0 && i < N) v = src[(c * N + i) * lanes + l];
    dst[gslot * lanes + l] = v;
  }
}

template <typename Lane>
__global__ void __launch_bounds__(256)
patch_scatter_kernel(const Lane* __restrict__ patch, const int64_t* __restrict__ index, const uint8_t* __restrict__ write_mask,
                     int64_t slots, int N, int K, int64_t lanes, Lane* __restrict__ dst) {
  const int64_t total = slots * lanes;
  for (int64_t e = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x; e < total; e += static_cast<int64_t>(gridDim.x) * blockDim.x) {
    const int64_t slot = e / lanes, l = e - slot * lanes;
    const int64_t i = index[slot];
    if (i < 0 || i >= N || (write_mask && write_mask[slot] == 0)) continue;
    dst[((slot / K) * N + i) * lanes + l] = patch[e];
  }
}

using Lane1 = uint8_t;
using Lane4 = uint32_t;
using Lane16 = uint4;

int lane_bytes(int64_t row_bytes, const void* a, const void* b) {
  const uintptr_t bits = static_cast<uintptr_t>(row_bytes) | reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(b);
  return bits % 16 == 0 ? 16 : bits % 4 == 0 ? 4 : 1;
}

unsigned copy_grid(int64_t elements) { return static_cast<unsigned>(std::min<int64_t>((elements + 255) / 256, 1 << 16)); }

template <typename Lane>
void launch_gather(const void* src, const int64_t* index, const int32_t* complex_of_row, int rows, int N, int K, int64_t row_bytes, void* dst,
                   hipStream_t st) {
  const int64_t lanes = row_bytes / static_cast<int64_t>(sizeof(Lane));
  RowMap map{};
  if (complex_of_row == nullptr) {
    const int64_t slots = static_cast<int64_t>(rows) * K;
    hipLaunchKernelGGL((patch_gather_kernel<Lane, false>), dim3(copy_grid(slots * lanes)), dim3(256), 0, st, static_cast<const Lane*>(src),
                       index, map, 0, slots, N, K, lanes, static_cast<Lane*>(dst));
    return;
  }
  for (int row0 = 0; row0 < rows; row0 += kMapRows) {
    const int n = std::min(kMapRows, rows - row0);
    for (int r = 0; r < n; ++r) map.complex_of_row[r] = complex_of_row[row0 + r];
    const int64_t slots = static_cast<int64_t>(n) * K;
    hipLaunchKernelGGL((patch_gather_kernel<Lane, true>), dim3(copy_grid(slots * lanes)), dim3(256), 0, st, static_cast<const Lane*>(src),
                       index, map, row0, slots, N, K, lanes, static_cast<Lane*>(dst));
  }
}

template <typename Lane>
void launch_scatter(const void* patch, const int64_t* index, const uint8_t* write_mask, int rows, int N, int K, int64_t row_bytes, void* dst,
                    hipStream_t st) {
  const int64_t lanes = row_bytes / static_cast<int64_t>(sizeof(Lane));
  const int64_t slots = static_cast<int64_t>(rows) * K;
  hipLaunchKernelGGL((patch_scatter_kernel<Lane>), dim3(copy_grid(slots * lanes)), dim3(256), 0, st, static_cast<const Lane*>(patch), index,
                     write_mask, slots, N, K, lanes, static_cast<Lane*>(dst));
}

}  // namespace
}  // namespace diffab

using namespace diffab;

extern "C" {

int diffab_patch_select(const float* ca, int32_t ca_stride, const uint8_t* residue_mask, const uint8_t* generation_mask,
                        const uint8_t* anchor_mask, const int64_t* chain_idx, const uint8_t* antigen_mask, int32_t B, int32_t N, int32_t k,
                        int32_t k_antigen, int32_t K, int64_t* index, uint8_t* patch_mask, int32_t* count, void* stream) {
  StreamOrder order_(stream);
  DIFFAB_REQUIRE(B >= 0 && N >= 0, DIFFAB_ERR_ARG, "patch_select: negative extent (B = %d, N = %d)", B, N);
  DIFFAB_REQUIRE(k >= 1, DIFFAB_ERR_ARG, "patch_select: k must be >= 1, got %d", k);
  DIFFAB_REQUIRE(k_antigen >= 0, DIFFAB_ERR_ARG, "patch_select: k_antigen must be >= 0, got %d", k_antigen);
  DIFFAB_REQUIRE(static_cast<int64_t>(K) >= static_cast<int64_t>(k) + k_antigen, DIFFAB_ERR_ARG,
                 "patch_select: K = %d rows cannot hold k + k_antigen = %d + %d residues", K, k, k_antigen);
  DIFFAB_REQUIRE(k_antigen == 0 || antigen_mask != nullptr, DIFFAB_ERR_ARG, "patch_select: k_antigen = %d needs an antigen_mask", k_antigen);
  DIFFAB_REQUIRE(N <= kSelMaxN, DIFFAB_ERR_UNSUPPORTED, "patch_select: N = %d residues per complex, the kernel holds at most %d", N, kSelMaxN);
  if (B == 0) return DIFFAB_OK;
  DIFFAB_REQUIRE(index && patch_mask && count, DIFFAB_ERR_ARG, "patch_select: null output");
  DIFFAB_REQUIRE(N == 0 || (ca && generation_mask), DIFFAB_ERR_ARG, "patch_select: null ca / generation_mask");
  DIFFAB_REQUIRE(ca_stride >= 3, DIFFAB_ERR_ARG, "patch_select: ca_stride = %d floats, a residue's CA takes 3", ca_stride);
  int P = 64;
  while (P < N) P <<= 1;
  hipLaunchKernelGGL(patch_select_kernel, dim3(B), dim3(kSelThreads), 0, as_stream(stream), ca, ca_stride, residue_mask, generation_mask,
                     anchor_mask, chain_idx, antigen_mask, N, P, k, k_antigen, K, index, patch_mask, count);
  DIFFAB_LAUNCH_CHECK();
  return DIFFAB_OK;
}

int diffab_patch_gather(const void* src, const int64_t* index, const int32_t* complex_of_row, int32_t B, int32_t N, int32_t rows, int32_t K,
                        int64_t row_bytes, void* dst, void* stream) {
  StreamOrder order_(stream);
  DIFFAB_REQUIRE(B >= 0 && N >= 0 && rows >= 0 && K >= 0, DIFFAB_ERR_ARG, "patch_gather: negative extent (B = %d, N = %d, rows = %d, K = %d)",
                 B, N, rows, K);
  DIFFAB_REQUIRE(row_bytes > 0 && row_bytes <= INT_MAX, DIFFAB_ERR_ARG, "patch_gather: row_bytes = %lld outside [1, 2^31)",
                 static_cast<long long>(row_bytes));
  if (rows == 0 || K == 0) return DIFFAB_OK;
  DIFFAB_REQUIRE(complex_of_row != nullptr || rows == B, DIFFAB_ERR_ARG, "patch_gather: without complex_of_row rows must equal B (%d != %d)",
                 rows, B);
  for (int r = 0; complex_of_row && r < rows; ++r)
    DIFFAB_REQUIRE(complex_of_row[r] >= 0 && complex_of_row[r] < B, DIFFAB_ERR_ARG, "patch_gather: complex_of_row[%d] = %d outside [0, %d)", r,
                   complex_of_row[r], B);
  DIFFAB_REQUIRE(index && dst && (src || N == 0), DIFFAB_ERR_ARG, "patch_gather: null src / index / dst");
  hipStream_t st = as_stream(stream);
  switch (lane_bytes(row_bytes, src, dst)) {
    case 16: launch_gather<Lane16>(src, index, complex_of_row, rows, N, K, row_bytes, dst, st); break;
    case 4: launch_gather<Lane4>(src, index, complex_of_row, rows, N, K, row_bytes, dst, st); break;
    default: launch_gather<Lane1>(src, index, complex_of_row, rows, N, K, row_bytes, dst, st); break;
  }
  DIFFAB_LAUNCH_CHECK();
  return DIFFAB_OK;
}

int diffab_patch_scatter(const void* patch, const int64_t* index, const uint8_t* write_mask, int32_t rows, int32_t N, int32_t K,
                         int64_t row_bytes, void* dst, void* stream) {
  StreamOrder order_(stream);
  DIFFAB_REQUIRE(rows >= 0 && N >= 0 && K >= 0, DIFFAB_ERR_ARG, "patch_scatter: negative extent (rows = %d, N = %d, K = %d)", rows, N, K);
  DIFFAB_REQUIRE(row_bytes > 0 && row_bytes <= INT_MAX, DIFFAB_ERR_ARG, "patch_scatter: row_bytes = %lld outside [1, 2^31)",
                 static_cast<long long>(row_bytes));
  if (rows == 0 || K == 0 || N == 0) return DIFFAB_OK;
  DIFFAB_REQUIRE(patch && index && dst, DIFFAB_ERR_ARG, "patch_scatter: null patch / index / dst");
  hipStream_t st = as_stream(stream);
  switch (lane_bytes(row_bytes, patch, dst)) {
    case 16: launch_scatter<Lane16>(patch, index, write_mask, rows, N, K, row_bytes, dst, st); break;
    case 4: launch_scatter<Lane4>(patch, index, write_mask, rows, N, K, row_bytes, dst, st); break;
    default: launch_scatter<Lane1>(patch, index, write_mask, rows, N, K, row_bytes, dst, st); break;
  }
  DIFFAB_LAUNCH_CHECK();
  return DIFFAB_OK;
}

}  // extern "C"
