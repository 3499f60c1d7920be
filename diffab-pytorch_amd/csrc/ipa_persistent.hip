// ipa_persistent.hip - the IPA module (all NL layers) of a batch of K = 128 or K = 256 patches as ONE patch-resident launch.
//
// BASELINE.json's execution model: one 512-thread work-group per CDR patch.  A work-group owns its patch from the first layer's
// projections to the last layer's to_out - per layer: the six projections of its 128 rows (proj_frames_h3_tile.h), the eight 16-row
// attention tiles (ipa_attn_tile.h), to_out (rowgemm_h3_tile.h) - and the next patch of its queue after that.  Patches never exchange
// data on this path (every einsum of diffab_pytorch.py:416-457 carries `b`; the layer loop :494-498 is per sample), so there is NO
// inter-CU synchronisation: a phase hands its rows to the next one through global memory written and read by the SAME work-group
// (one CU, one vector L1: work-group scope; s_waitcnt vmcnt(0) + s_barrier), and the CUs are free to drift apart - which is the point:
// started together by 18 separate launches, all 256 CUs stream their pair rows in the same 13-15 us and leave HBM idle for the next 25
// (profiles/r03_lockstep.md); here the first items are staggered once per launch and nothing ever re-aligns them.
//
// K = 128: to_out hands its 128 x 128 output tile to the next layer's projections through LDS (the tile's fp32 values, read back by the
// projections instead of from global memory); only the last layer writes it to global memory, where the heads and the caller read it.
//
// Same tile bodies, same arithmetic, same summation orders as the multi-launch path: results are bitwise the same (tested), and with
// them the sampler's shard invariance.
#include "common.h"
#include "denoiser_internal.h"
#define AT_STAMP_REALTIME 1  // the diagnostic stamps of this file's kernels use the chip-wide 100 MHz counter (comparable between CUs)
#include "ipa_attn_tile.h"
#include "proj_frames_h3_tile.h"
#include "rowgemm_h3_tile.h"
#include "mlp_chain_tile.h"
#include "mlp_chain_slab.h"

namespace diffab {

namespace {
constexpr size_t cmax(size_t a, size_t b) { return a > b ? a : b; }
constexpr size_t kModuleLdsBytes = cmax(cmax(ipa_attn_lds_bytes(8), static_cast<size_t>(kChainLdsBytes)),
                                        cmax(static_cast<size_t>(pjh3::PJ_LDS_BYTES), static_cast<size_t>(h3tile::lds_bytes<128>())));
// K = 128: to_out's output tile, kept for the next layer's projections, behind the LDS of both dense tiles (floats)
constexpr size_t kXImageOffset = cmax(static_cast<size_t>(pjh3::PJ_LDS_BYTES), static_cast<size_t>(h3tile::lds_bytes<128>())) / 4;
static_assert(kXImageOffset * 4 + h3tile::y_lds_bytes<128>() <= kModuleLdsBytes, "module LDS: no room for the x image of the dense phases");
static_assert(kModuleLdsBytes <= 160 * 1024, "module LDS: one work-group per CU within gfx950's 160 KiB");
static_assert(kXImageOffset % 4 == 0, "x image: 16-byte aligned rows");

struct ModuleArgs {
  float* xa;                 // [B K][128]: the module's input (layer 0 reads it), then every odd layer's output
  float* xb;                 // [B K][128]: every even layer's output; the result is in (NL odd ? xb : xa) (K = 128: the last layer's only)
  float* proj;               // [B K][1344] workspace
  float* feat;               // [B K][1024] workspace
  const float* pair;         // fp16 planes of the pair embedding (launch_pair_split)
  const float* esc;          // {s, 1 / s} per pair row
  const int* ctx_of_row;     // shared contexts: [B] context of each patch's pair rows (null: the identity)
  // reverse sampler: the row plan of the LAST layer (launch_row_plan: per patch {items, slab bits, start row of each item}; null: the
  // K / 16 aligned tiles)
  const int* last_layer_rows;
  const float* R;            // [B K][9]
  const float* t;            // [B K][3]
  const char* planes;        // per layer: ipa_layer_planes_bytes() (w_bias, gamma, b_out | projection planes | to_out planes | 1 / scales)
  size_t layer_stride, pj_off, out_off, wis_off, small_off;  // offsets of the fp16 planes, 1 / scale vectors and small vectors in a layer's block
  // diagnostics (null in production): [item][wave][8] of the attention tiles + [B][NL][4] phase stamps behind them + [B] the end of the heads
  // + [B] the start of the patch
  unsigned long long* stamps;
  // the denoiser's MLPs as phases of the same launch (null emb_X: not fused): the embedding MLP of the patch's rows in front of layer 0
  // (emb_X -> xa), the three heads behind the last layer (module output -> heads.Y[]); mlp_chain_tile.h, bitwise mlp_chain_b6_kernel
  const float* emb_X;
  MlpChainSet emb, heads;
  int B, NL;
  int stagger_ticks, stagger_classes;  // the work-groups of class c = (blockIdx / 8) % classes start c * ticks (10 ns each) late
  // reverse sampler, K = 128 with a row plan: the start class of every patch's work-group by its last-layer work (launch_start_classes),
  // read by the PLANNED_START form of the kernel alone (last: the other arguments keep their places)
  const unsigned char* start_class;
};
}  // namespace

// Word idx of the row plan through a scalar load (as attn_shift_pair_rows: a kernel that also stores to global memory would otherwise
// get a vector load and a readfirstlane): the item count and the start rows stay off the vector pipe, in SGPRs.
__device__ __forceinline__ int module_plan_word(const int* __restrict__ plan, const int idx) {
  int w;
  asm volatile("s_load_dword %0, %1, 0x0\n\ts_waitcnt lgkmcnt(0)" : "=s"(w) : "s"(plan + idx) : "memory");
  return w;
}

// KRES: residues per patch - 128 (one 128-row dense tile per patch, single-chunk attention items) or 256 (BASELINE config 5: two dense
// tiles, sixteen attention items of two 128-key chunks with the online softmax across them - ipa_attn_tile<8, true, ...>)
// PLANNED_START: the start class of a work-group is the byte of its first patch in a.start_class instead of the static one.  Its own
// instantiation: every launch without the bytes (no plan, DIFFAB_FLAG_ALL_ROWS, diffab_denoise_step_fwd, scoring, K = 256) runs the
// code it ran before, instruction for instruction.
template <int KRES, bool PLANNED_START = false>
__global__ __launch_bounds__(512) void ipa_module_persistent_kernel(const ModuleArgs a) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  constexpr int K = KRES, NTILE = K / TI, DT = K / 128;  // DT: dense 128-row tiles per patch
  static_assert(KRES == 128 || KRES == 256, "patch-resident module: K = 128 or 256");
  const int M = a.B * K;
  if (a.stagger_ticks > 0 && a.stagger_classes > 1) {
    // (every wave waits for itself: no barrier needed, the first phase starts with loads only)
    const unsigned long long t0 = __builtin_amdgcn_s_memrealtime();
    // (the class byte through a scalar load of its word, as the plan's words)
    const int cls = PLANNED_START
                        ? (module_plan_word(reinterpret_cast<const int*>(a.start_class), blockIdx.x >> 2) >> (8 * (blockIdx.x & 3))) & 255
                        : static_cast<int>((blockIdx.x >> 3) % a.stagger_classes);
    const unsigned long long wait = static_cast<unsigned long long>(cls) * a.stagger_ticks;
    while (__builtin_amdgcn_s_memrealtime() - t0 < wait) __builtin_amdgcn_s_sleep(32);
  }
  unsigned long long* pstamps = a.stamps ? a.stamps + static_cast<size_t>(a.B) * a.NL * NTILE * 64 : nullptr;
  auto pstamp = [&](int b, int l, int k) {
    if (pstamps != nullptr && threadIdx.x == 0) pstamps[(static_cast<size_t>(b) * a.NL + l) * 4 + k] = __builtin_amdgcn_s_memrealtime();
  };
#pragma unroll 1
  for (int b = blockIdx.x; b < a.B; b += gridDim.x) {
    // (the start of the patch: what lies between it and layer 0's first stamp is the embedding MLP)
    if (pstamps != nullptr && threadIdx.x == 0) pstamps[static_cast<size_t>(a.B) * a.NL * 4 + a.B + b] = __builtin_amdgcn_s_memrealtime();
    if (a.emb_X != nullptr) {  // ---- to_res_emb of the patch's rows (diffab_pytorch.py:519-523, folded concatenation)
#pragma unroll 1
      for (int dt = 0; dt < DT; ++dt) {
        int tid = threadIdx.x;
        asm volatile("" : "+v"(tid));
        chaintile::mlp_chain_tile(reinterpret_cast<__bf16*>(lds), tid, b * DT + dt, a.emb_X, 128, a.emb.c[0].planes[0], a.emb.c[0].planes[1],
                                  nullptr, a.emb.c[0].bias[0], a.emb.c[0].bias[1], nullptr, a.emb.c[0].bias_idx0, a.emb.c[0].bias_div0, 2, 128,
                                  a.xa, 128, M);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
      }
    }
#pragma unroll 1
    for (int l = 0; l < a.NL; ++l) {
      const char* lp = a.planes + static_cast<size_t>(l) * a.layer_stride;
      const float* small = reinterpret_cast<const float*>(lp + a.small_off);  // [w_bias 8 x 64][gamma 8, pad to 64][b_out 128]
      const float* xin = (l & 1) ? a.xb : a.xa;
      float* xout = (l & 1) ? a.xa : a.xb;
      pstamp(b, l, 0);
#pragma unroll 1
      for (int dt = 0; dt < DT; ++dt) {  // ---- the six projections + frames of the patch's rows, 128 at a time
        int tid = threadIdx.x;
        asm volatile("" : "+v"(tid));  // (an opaque copy per phase: lane-constant addresses must not stay live across the phases)
        if (KRES == 128) {  // x: the previous layer's to_out tile, still in LDS; layer 0 stages the module's input rows there first
          if (l == 0) {
            float* xl = lds + kXImageOffset;
            for (int i = tid; i < 128 * 32; i += 512) {
              const int row = i >> 5, c4 = 4 * (i & 31);
              *reinterpret_cast<float4*>(xl + row * h3tile::Y_LDS_LD + c4) =
                  *reinterpret_cast<const float4*>(xin + (static_cast<int64_t>(b) * 128 + row) * 128 + c4);
            }
            __syncthreads();
          }
          pjh3::proj_frames_h3_tile<true, false, true, true>(reinterpret_cast<_Float16*>(lds), tid, b, 0, 1, nullptr,
                                                             reinterpret_cast<const _Float16*>(lp + a.pj_off),
                                                             reinterpret_cast<const float*>(lp + a.wis_off), a.R, a.t, a.proj, M, 0, 0, 0,
                                                             lds + kXImageOffset);
        } else {
          pjh3::proj_frames_h3_tile<true, false>(reinterpret_cast<_Float16*>(lds), tid, b * DT + dt, 0, 1, xin,
                                                 reinterpret_cast<const _Float16*>(lp + a.pj_off), reinterpret_cast<const float*>(lp + a.wis_off),
                                                 a.R, a.t, a.proj, M);
        }
        if (dt + 1 < DT) {  // the next tile's weight stages overwrite this one's LDS
          asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
          __syncthreads();
        }
      }
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __syncthreads();
      pstamp(b, l, 1);
      // ---- attention: the eight row tiles of the patch
      // last_layer_rows (reverse sampler): the step's outputs are read for generated residues only, and the last layer's attention
      // output of a row feeds that row of to_out and of the heads alone - the last layer runs the plan's items instead: 16-row windows
      // that start at the first generated row not yet covered (clamped to K - 16), never more than the aligned tiles with a generated
      // residue and often fewer (a segment of up to 16 rows across a tile boundary is one item).  The rows of no item keep in their
      // feature rows what the previous layer's item wrote (the same work-group, complete since that layer's barriers): finite and
      // deterministic; to_out still runs on all rows of the patch and the heads on the 32-row slabs with a generated residue (below),
      // every product there is row-wise, and nothing reads what they make of those rows.  A row's bits do not depend on the item that
      // carries it (ipa_attn_tile.h).
      const int* rows = l + 1 == a.NL ? a.last_layer_rows : nullptr;
      const int n_items = rows != nullptr ? module_plan_word(rows, b * (2 + NTILE)) : NTILE;
#pragma unroll 1
      for (int item = 0; item < n_items; ++item) {
        const int i0 = rows != nullptr ? module_plan_word(rows, b * (2 + NTILE) + 2 + item) : item * TI;
        ipa_attn_tile<8, (KRES > 128), true>(lds, b, i0, static_cast<unsigned>((b * a.NL + l) * NTILE + item), a.proj, a.pair, a.R, a.t, small,
                                             small + 512, a.feat, K / 128, a.stamps, a.esc, nullptr, nullptr, a.ctx_of_row);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();  // the next tile's phase 1 overwrites the image; the last tile's feature rows are complete
      }
      pstamp(b, l, 2);
#pragma unroll 1
      for (int dt = 0; dt < DT; ++dt) {  // ---- to_out
        int tid = threadIdx.x;
        asm volatile("" : "+v"(tid));
        if (KRES == 128)  // the tile stays in LDS for the next layer; the last layer's goes to global memory only
          h3tile::rowgemm128_h3_tile<false, 128, false, true>(reinterpret_cast<_Float16*>(lds), tid, b, a.feat, AF,
                                                              reinterpret_cast<const _Float16*>(lp + a.out_off),
                                                              reinterpret_cast<const float*>(lp + a.wis_off) + ANP, small + 576, nullptr, 0,
                                                              l + 1 == a.NL ? xout : nullptr, 128, M, AF, 0, nullptr, lds + kXImageOffset);
        else
          h3tile::rowgemm128_h3_tile<false, 128>(reinterpret_cast<_Float16*>(lds), tid, b * DT + dt, a.feat, AF,
                                                 reinterpret_cast<const _Float16*>(lp + a.out_off),
                                                 reinterpret_cast<const float*>(lp + a.wis_off) + ANP, small + 576, nullptr, 0, xout, 128, M, AF);
        if (dt + 1 < DT) {
          asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
          __syncthreads();
        }
      }
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __syncthreads();
      pstamp(b, l, 3);
    }
    if (a.emb_X != nullptr) {  // ---- the three heads on the module's output rows (:525-533, beta columns folded into bias tables)
      const float* xfin = (a.NL & 1) ? a.xb : a.xa;
      if (KRES == 128 && a.last_layer_rows != nullptr) {
        // reverse sampler, K = 128: the three heads of the 32-row slabs with a generated residue (the plan's slab bits), two slabs to a
        // pass of the slab form (mlp_chain_slab.h: the units of the three chains side by side on six waves, weight fragments straight
        // from global memory and shared by the two slabs, two barriers per layer) instead of three chain tiles behind one another.
        // The heads of the other rows are never read and keep what the workspace held.  Bitwise the chain tile's rows.
        unsigned rest = static_cast<unsigned>(module_plan_word(a.last_layer_rows, b * (2 + NTILE) + 1)) & 15u;
#pragma unroll 1
        while (rest != 0) {
          const int s0 = __builtin_ctz(rest);
          rest &= rest - 1;
          const int ns = rest != 0 ? 2 : 1;
          const int s1 = rest != 0 ? __builtin_ctz(rest) : s0;
          rest &= rest - 1;  // (0 stays 0)
          int tid = threadIdx.x;
          asm volatile("" : "+v"(tid));
          chainslab::mlp_chain_slabs<3>(reinterpret_cast<__bf16*>(lds), tid, ns, b * 128 + 32 * s0, b * 128 + 32 * s1, xfin, 128, a.heads, M);
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // (the barrier behind the last layer is the slab form's own)
      } else {
#pragma unroll 1
      for (int hdt = 0; hdt < 3 * DT; ++hdt) {
        const int hd = hdt / DT, dt = hdt % DT;
        // reverse sampler: only the 32-row slabs with a generated residue (the plan's slab bits) - the heads of the other rows are never
        // read and keep what the workspace held.  Waves 2 s and 2 s + 1 own slab s (mlp_chain_tile<true>): the one or two wanted slabs
        // of a CDR then keep all four SIMDs' matrix pipes busy instead of queueing both waves of a slab on one.
        const unsigned hslabs =
            a.last_layer_rows != nullptr ? static_cast<unsigned>(module_plan_word(a.last_layer_rows, b * (2 + NTILE) + 1)) : ~0u;
        const unsigned tslabs = (hslabs >> (4 * dt)) & 15u;
        if (tslabs == 0) continue;
        int tid = threadIdx.x;
        asm volatile("" : "+v"(tid));
#define HSEL(f) (hd == 0 ? a.heads.c[0].f : hd == 1 ? a.heads.c[1].f : a.heads.c[2].f)
        chaintile::mlp_chain_tile<true>(reinterpret_cast<__bf16*>(lds), tid, b * DT + dt, xfin, 128, HSEL(planes[0]), HSEL(planes[1]), HSEL(planes[2]),
                                  HSEL(bias[0]), HSEL(bias[1]), HSEL(bias[2]), HSEL(bias_idx0), HSEL(bias_div0), 3, HSEL(n_out),
                                  hd == 0 ? a.heads.Y[0] : hd == 1 ? a.heads.Y[1] : a.heads.Y[2],
                                  hd == 0 ? a.heads.ldy[0] : hd == 1 ? a.heads.ldy[1] : a.heads.ldy[2], M, tslabs);
#undef HSEL
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();  // the next chain (or the next patch's first phase) overwrites the image
      }
      }
      if (pstamps != nullptr && threadIdx.x == 0) pstamps[static_cast<size_t>(a.B) * a.NL * 4 + b] = __builtin_amdgcn_s_memrealtime();
    }
  }
}

namespace {
int g_stagger_ticks = 1000, g_stagger_classes = 8;  // 8 classes x 10 us = two attention-tile periods (swept in round 5: 0 | 8 x 2.5 | 8 x 5 |
                                                     // 8 x 10 | 8 x 20 | 16 x 10 | 8 x 30 us -> 2.47 2.48 2.47 2.43 2.44 2.46 2.50 ms per step)
unsigned long long* g_module_stamps = nullptr;
}  // namespace
void set_module_stagger(int ticks, int classes) {
  g_stagger_ticks = ticks;
  g_stagger_classes = classes;
}
void set_module_stamps(void* p) { g_module_stamps = static_cast<unsigned long long*>(p); }
int module_stagger_classes() { return g_stagger_ticks > 0 ? g_stagger_classes : 1; }

bool ipa_module_persistent_supported(const diffab_dims* d) {
  return fast_path_supported(d) && (d->K == 128 || d->K == 256) && d->NL >= 1;
}

// planes: d->NL x ipa_layer_planes_bytes() (ipa_layer_split_weights); pair_planes: launch_pair_split() of n_ctx patches (0: d->B), state
// patch b reading those of ctx_of_row[b] (null: b); xa in, result in (NL odd ? xb : xa)
// last_layer_rows (optional, reverse sampler): the row plan of launch_row_plan ([B][2 + K / 16] ints), the last layer's attention runs
// its items only and the heads (when fused) its slabs only
// emb_X (optional, with emb and heads): the embedding MLP's input rows - the launch then also runs the embedding MLP (-> xa) and the three
// heads (module output -> heads->Y[]) of every patch
// start_class (optional, with a row plan): launch_start_classes' byte per patch, the start class of its work-group
int launch_ipa_module_persistent(const diffab_dims* d, float* xa, float* xb, const float* R, const float* t, float* ws, const void* planes,
                                 const float* pair_planes, hipStream_t st, const float* emb_X, const MlpChainSet* emb,
                                 const MlpChainSet* heads, const int* ctx_of_row, int n_ctx, const int* last_layer_rows,
                                 const unsigned char* start_class) {
  DIFFAB_REQUIRE(ipa_module_persistent_supported(d) && xa && xb && R && t && ws && planes && pair_planes, DIFFAB_ERR_ARG,
                 "ipa_module_persistent: unsupported operands");
  DIFFAB_REQUIRE((reinterpret_cast<uintptr_t>(last_layer_rows) & 3) == 0, DIFFAB_ERR_ARG,
                 "ipa_module_persistent: the row plan must be 4-byte aligned");
  const size_t rows = static_cast<size_t>(d->B) * d->K;
  ModuleArgs a{};
  a.xa = xa;
  a.xb = xb;
  a.proj = ws;
  a.feat = ws + rows * ANP;
  a.pair = pair_planes + 64;
  a.esc = pair_row_scales(d, pair_planes, n_ctx);
  a.ctx_of_row = ctx_of_row;
  a.last_layer_rows = last_layer_rows;
  a.R = R;
  a.t = t;
  a.planes = static_cast<const char*>(planes);
  a.layer_stride = ipa_layer_planes_bytes();
  a.pj_off = ipa_layer_h3_pj_offset();
  a.out_off = ipa_layer_h3_out_offset();
  a.wis_off = ipa_layer_h3_wis_offset();
  a.small_off = ipa_layer_small_offset();
  a.stamps = g_module_stamps;
  if (emb_X != nullptr) {
    DIFFAB_REQUIRE(emb && heads && d->D == 128 && (reinterpret_cast<uintptr_t>(emb_X) & 15) == 0, DIFFAB_ERR_ARG,
                   "ipa_module_persistent: the fused MLP phases need both chain sets");
    a.emb_X = emb_X;
    a.emb = *emb;
    a.heads = *heads;
  }
  a.B = d->B;
  a.NL = d->NL;
  a.stagger_ticks = g_stagger_ticks;
  a.stagger_classes = g_stagger_classes;
  DIFFAB_REQUIRE((reinterpret_cast<uintptr_t>(start_class) & 3) == 0, DIFFAB_ERR_ARG,
                 "ipa_module_persistent: the start classes must be 4-byte aligned");
  DIFFAB_REQUIRE(start_class == nullptr || (d->K == 128 && last_layer_rows != nullptr), DIFFAB_ERR_ARG,
                 "ipa_module_persistent: start classes go with K = 128 and a row plan");
  a.start_class = start_class;
  int dev = 0, ncu = 256;
  if (hipGetDevice(&dev) == hipSuccess) (void)hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, dev);
  const int grid = d->B < ncu ? d->B : ncu;  // one work-group per CU (149 KiB of LDS each); more patches than CUs: a work-group walks its queue
#define MODULE_LAUNCH(...)                                                                                                       \
  do {                                                                                                                            \
    DIFFAB_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(ipa_module_persistent_kernel<__VA_ARGS__>),                \
                                         hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int>(kModuleLdsBytes)));        \
    timer_begin(st);                                                                                                              \
    hipLaunchKernelGGL((ipa_module_persistent_kernel<__VA_ARGS__>), dim3(grid), dim3(512), kModuleLdsBytes, st, a);               \
    timer_end(st);                                                                                                                \
  } while (0)
  if (d->K == 128 && a.start_class != nullptr) MODULE_LAUNCH(128, true);
  else if (d->K == 128) MODULE_LAUNCH(128);
  else MODULE_LAUNCH(256);
#undef MODULE_LAUNCH
  DIFFAB_LAUNCH_CHECK();
  return DIFFAB_OK;
}

}  // namespace diffab
