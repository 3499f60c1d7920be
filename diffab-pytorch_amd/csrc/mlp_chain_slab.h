// mlp_chain_slab.h - the chains of mlp_chain_tile.h for ONE or TWO 32-row slabs: one or three chains over the same input rows at the
// same time, as a device function (the head phases of the patch-resident module kernel under a row plan, ipa_persistent.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

#include "mlp_chain_tile.h"

namespace diffab {
namespace chainslab {
using b6tile::BK;
using b6tile::b6_off;
using b6tile::split3;
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
// (global address space, said aloud: a pointer that went through sel3's integers would otherwise be loaded from as a flat one, which
// counts against the LDS counter too)
typedef const bf16x8 __attribute__((address_space(1)))* global_bf16x8_p;
typedef const float __attribute__((address_space(1)))* global_float_p;
typedef const f32x4 __attribute__((address_space(1)))* global_f32x4_p;

constexpr int kSlabImage = 4 * 3 * 32 * BK;  // bf16 elements of one [4 chunks][3 planes][32 rows][32 k] image: 24 KiB
template <int NCH>
constexpr int slab_lds_bytes() { return 2 * NCH * kSlabImage * 2; }  // an image per (slab, chain)
static_assert(slab_lds_bytes<3>() <= kChainLdsBytes, "slab form: within the LDS of the chain tile");

// pointer L of three by masks on the scalar unit (written as nested selects the compiler builds a table of the three in scratch memory
// and indexes it per lane)
template <typename T>
__device__ __forceinline__ T* sel3(int L, T* p0, T* p1, T* p2) {
  const uintptr_t m0 = -static_cast<uintptr_t>(L == 0), m1 = -static_cast<uintptr_t>(L == 1), m2 = -static_cast<uintptr_t>(L >= 2);
  return reinterpret_cast<T*>((reinterpret_cast<uintptr_t>(p0) & m0) | (reinterpret_cast<uintptr_t>(p1) & m1) |
                              (reinterpret_cast<uintptr_t>(p2) & m2));
}

// The chain tile runs a chain as 12 chunk steps behind one another, all 512 threads staging every 24 KiB weight chunk through LDS for
// the two waves that own a wanted slab, and three heads are three such calls.  With one or two wanted slabs that phase is latency: no
// weight byte in LDS is read by more than two waves.  Here a UNIT is (chain, 64-column half): the chain tile's wave tile, its two
// 32 x 32 accumulators acc[0], acc[1] per slab.  Wave w < 2 NCH owns unit (chain w % NCH, half w / NCH) in every layer - waves w and
// w + 4 share a SIMD, so the three chains of a slab run side by side on three SIMDs before a SIMD takes a second wave - and the waves
// without a unit only stage rows and take the barriers.
// Weights: a lane's fragments come straight from the wsplit128 planes in global memory ([chunk][plane][128 rows][32 k], unswizzled:
// the 16 bytes at row 64 cw + 32 tt + (lane & 31), slot 2 ks + (lane >> 5)) - no LDS ring, no block barrier per chunk.  Two chunks of
// fragments are in registers; as soon as a chunk's products are issued its registers take the chunk two steps on, across the layers
// (weights do not depend on activations), so that two chunks are in flight all the time.  With TWO slabs a fragment serves both: the
// second slab costs its MFMAs, not a second pass over the weights.
// Activations go through LDS as in the chain tile (split3 planes, the same swizzled rows), one 24 KiB image per (slab, chain).  Layer
// 0's input image of a slab is shared by the chains (image j of slab j); an epilogue writes the next layer's input in place, behind a
// barrier that ends the layer's reads (the accumulators wait in registers), and a second barrier hands the images to the next layer.
// The narrow last layer: a unit whose 64 columns do not exist is skipped, a 32-column group that does not exist is not computed.
// Bitwise the chain tile for every row it computes: the same split3 of the inputs, the same MFMA with the weights as the A operand, per
// accumulator the order chunk 0..3, ks 0..1, the six terms in TA / TB order, the same epilogue and stores.  Which wave computes a unit
// does not enter its arithmetic.
//
// cl: slab_lds_bytes<NCH>() of LDS, 16-byte aligned; 512 threads, ALL of which must call with the same ns (every wave takes every
// barrier, with or without a unit); rows row0a .. + 31 and (ns == 2) row0b .. + 31 of X[M x 128] (ldx floats apart) ->
// cs.Y[c][M x n_out] for c < NCH.  The chains have the same number of layers.  On return the images may be overwritten.
template <int NCH>
__device__ __forceinline__ void mlp_chain_slabs(__bf16* cl, const int tid, const int ns, const int row0a, const int row0b,
                                                const float* __restrict__ X, int ldx, const MlpChainSet& cs, int M) {
  static_assert(NCH == 1 || NCH == 3, "slab form: one chain or three");
  // (selects, not indexed loads: the set is a kernel argument)
#define SLAB_CSEL(k_, f) ((NCH == 1 || (k_) == 0) ? cs.c[0].f : (k_) == 1 ? cs.c[NCH > 1 ? 1 : 0].f : cs.c[NCH - 1].f)
#define SLAB_YSEL(k_, f) ((NCH == 1 || (k_) == 0) ? cs.f[0] : (k_) == 1 ? cs.f[NCH > 1 ? 1 : 0] : cs.f[NCH - 1])
  const int lane = tid & 63, l31 = lane & 31, hk = lane >> 5;
  const int wv_u = __builtin_amdgcn_readfirstlane(tid >> 6);  // (scalar: the unit tests below are scalar branches)
  const int nl = cs.c[0].nlayers;
  const bool has_unit = wv_u < 2 * NCH;
  const int ch = has_unit ? wv_u % NCH : 0, cw = has_unit ? wv_u / NCH : 0;
  // the unit's chain, selected once
  const __bf16 *const pl0 = SLAB_CSEL(ch, planes[0]), *const pl1 = SLAB_CSEL(ch, planes[1]), *const pl2 = SLAB_CSEL(ch, planes[2]);
  const float *const bs0 = SLAB_CSEL(ch, bias[0]), *const bs1 = SLAB_CSEL(ch, bias[1]), *const bs2 = SLAB_CSEL(ch, bias[2]);
  const int64_t* const bias_idx0 = SLAB_CSEL(ch, bias_idx0);
  const int bias_div0 = SLAB_CSEL(ch, bias_div0), n_out = SLAB_CSEL(ch, n_out), ldy = SLAB_YSEL(ch, ldy);
  float* const Y = SLAB_YSEL(ch, Y);
#undef SLAB_CSEL
#undef SLAB_YSEL
  const int ntt_last = n_out - 64 * cw >= 64 ? 2 : n_out - 64 * cw <= 0 ? 0 : (n_out - 64 * cw + 31) >> 5;
  // a step is one chunk of the unit: step s = chunk s % 4 of layer s / 4
  const int n_steps = !has_unit ? 0 : ntt_last > 0 ? 4 * nl : 4 * (nl - 1);
  auto w_of = [&](int s) -> const __bf16* {  // the step's chunk of the unit's planes (uniform: plane 0, row 64 cw)
    s = s < n_steps ? s : n_steps - 1;       // (past the end: the last one again - an unconditional prefetch)
    const int L = s >> 2;
    const __bf16* W = sel3(L, pl0, pl1, pl2);
    return W + (s & 3) * (3 * 128 * BK) + (64 * cw) * BK;
  };
  // (a scalar base and ONE 32-bit lane offset for all twelve loads of a chunk: no 64-bit lane address per plane and column group)
  const unsigned w_lane = static_cast<unsigned>((l31 * BK + 8 * hk) * 2);  // bytes
  bf16x8 wf[2][2][2][3];  // [step % 2][tt][ks][plane]
  auto load_w = [&](int slot, const __bf16* src) {
#pragma unroll
    for (int tt = 0; tt < 2; ++tt)
#pragma unroll
      for (int ks = 0; ks < 2; ++ks)
#pragma unroll
        for (int p = 0; p < 3; ++p)
          wf[slot][tt][ks][p] =
              *(global_bf16x8_p)(reinterpret_cast<uintptr_t>(src + (p * 128 + 32 * tt) * BK + 16 * ks) + w_lane);
  };
  if (n_steps > 0) {  // the weights do not wait for the rows
    load_w(0, w_of(0));
    load_w(1, w_of(1));
  }
  // ---- X -> image j of slab j: 1024 16-byte pieces per slab, two per thread (row q / 32, floats 4 (q % 32) ..)
  {
    f32x4 xr[2][2];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      if (j >= ns) continue;
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        const int q = tid + 512 * i;
        int row = (j ? row0b : row0a) + (q >> 5);
        row = row < M ? row : M - 1;  // clamped (never stored)
        xr[j][i] = *reinterpret_cast<const f32x4*>(X + static_cast<int64_t>(row) * ldx + 4 * (q & 31));
      }
    }
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      if (j >= ns) continue;
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        const int q = tid + 512 * i, lrow = q >> 5, c4 = q & 31;
        bf16x4 h, m, l;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          __bf16 hh, mm, ll;
          split3(xr[j][i][e], hh, mm, ll);
          h[e] = hh; m[e] = mm; l[e] = ll;
        }
        __bf16* dst = cl + j * kSlabImage + (c4 >> 3) * (3 * 32 * BK) + b6_off(lrow, (c4 & 7) >> 1) + 4 * (c4 & 1);
        *reinterpret_cast<bf16x4*>(dst) = h;
        *reinterpret_cast<bf16x4*>(dst + 32 * BK) = m;
        *reinterpret_cast<bf16x4*>(dst + 2 * 32 * BK) = l;
      }
    }
  }
  __syncthreads();
  const int fx = (l31 >> 2) & 3;
  constexpr int TA[6] = {1, 2, 0, 1, 0, 0}, TB[6] = {1, 0, 2, 0, 1, 0};  // (mid,mid) (lo,hi) (hi,lo) (mid,hi) (hi,mid) (hi,hi)
#pragma unroll 1
  for (int L = 0; L < nl; ++L) {
    const bool last = L == nl - 1;
    const int ntt = last ? ntt_last : 2;
    const bool active = has_unit && ntt > 0;
    f32x16 acc[2][2];  // [slab][tt]
    if (active) {
#pragma unroll
      for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int tt = 0; tt < 2; ++tt)
#pragma unroll
          for (int r = 0; r < 16; ++r) acc[j][tt][r] = 0.f;
      // the layer's input images: layer 0 image j (the rows), later image j NCH + ch
      const __bf16* al = cl + (L == 0 ? 0 : ch * kSlabImage) + l31 * BK;
      const int slab_stride = L == 0 ? kSlabImage : NCH * kSlabImage;
#pragma unroll
      for (int c = 0; c < 4; ++c) {
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
          const int so = 8 * ((2 * ks + hk) ^ fx);
#pragma unroll
          for (int j = 0; j < 2; ++j) {
            if (j >= ns) continue;
            bf16x8 a[3];
#pragma unroll
            for (int p = 0; p < 3; ++p)
              a[p] = *reinterpret_cast<const bf16x8*>(al + j * slab_stride + c * (3 * 32 * BK) + (p * 32) * BK + so);
            // (weights as the A operand: D is the TRANSPOSED tile, as in the chain tile; one branch per twelve products)
            if (ntt == 2) {
#pragma unroll
              for (int term = 0; term < 6; ++term)
#pragma unroll
                for (int tt = 0; tt < 2; ++tt)
                  acc[j][tt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wf[c & 1][tt][ks][TB[term]], a[TA[term]], acc[j][tt], 0, 0, 0);
            } else {
#pragma unroll
              for (int term = 0; term < 6; ++term)
                acc[j][0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wf[c & 1][0][ks][TB[term]], a[TA[term]], acc[j][0], 0, 0, 0);
            }
          }
        }
        load_w(c & 1, w_of(4 * L + c + 2));  // the chunk two steps on, of this layer or of the next
        __builtin_amdgcn_sched_barrier(0);   // (requested here, not behind the layer's last product)
      }
    }
    __syncthreads();  // the layer's images are read
    if (active) {
      // ---- epilogue.  D^T 32x32: row = lane & 31, column = (r & 3) + 8 (r >> 2) + 4 hk (+ 32 tt + 64 cw)
      const bool table = L == 0 && (bias_idx0 != nullptr || bias_div0 > 0);
      const float* bl0 = sel3(L, bs0, bs1, bs2);
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        if (j >= ns) continue;
        int row = (j ? row0b : row0a) + l31;
        asm volatile("" : "+v"(row));  // (an opaque copy: the lane addresses of the epilogue must not be computed ahead of the layers and kept)
        global_float_p bl = (global_float_p)reinterpret_cast<uintptr_t>(bl0);
        if (table) {
          const int rc = row < M ? row : M - 1;
          const int64_t bi = bias_idx0 ? bias_idx0[rc] : rc / bias_div0;
          bl += bi * 128;
        }
        __bf16* img_out = cl + (j * NCH + ch) * kSlabImage;
#pragma unroll
        for (int tt = 0; tt < 2; ++tt) {
          if (tt >= ntt) continue;
#pragma unroll
          for (int g4 = 0; g4 < 4; ++g4) {
            const int col = 64 * cw + 32 * tt + 8 * g4 + 4 * hk;  // four consecutive columns col .. col + 3
            f32x4 bv = {0.f, 0.f, 0.f, 0.f};
            if (bl && (table || !last || col + 3 < n_out)) bv = *(global_f32x4_p)(bl + col);
            else if (bl && col < n_out) {  // the narrow last layer: the columns that exist
#pragma unroll
              for (int e = 0; e < 4; ++e)
                if (col + e < n_out) bv[e] = bl[col + e];
            }
            float o[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) o[e] = acc[j][tt][4 * g4 + e] + bv[e];
            if (last) {
              if (row < M) {
#pragma unroll
                for (int e = 0; e < 4; ++e)
                  if (col + e < n_out) Y[static_cast<int64_t>(row) * ldy + col + e] = o[e];
              }
            } else {
              bf16x4 h, m, l;
#pragma unroll
              for (int e = 0; e < 4; ++e) {
                __bf16 hh, mm, ll;
                split3(fmaxf(o[e], 0.f), hh, mm, ll);  // every layer but the last is followed by a ReLU
                h[e] = hh; m[e] = mm; l[e] = ll;
              }
              // elements (row l31, k = col .. col + 3) of the next layer's input: chunk col / 32, slot (col % 32) / 8, elements col % 8 ..
              __bf16* dst = img_out + (col >> 5) * (3 * 32 * BK) + b6_off(l31, (col & 31) >> 3) + (col & 7);
              *reinterpret_cast<bf16x4*>(dst) = h;
              *reinterpret_cast<bf16x4*>(dst + 32 * BK) = m;
              *reinterpret_cast<bf16x4*>(dst + 2 * 32 * BK) = l;
            }
          }
        }
      }
    }
    if (!last) __syncthreads();  // the next layer's images are written (the last layer writes no image)
  }
}
}  // namespace chainslab
}  // namespace diffab
