// analysis_prep.h - what an analysis entry prepares once per patch, before its row kernel runs, written once: the chain neighbours of
// every slot (diffab_metrics_backbone, diffab_refine_backbone, diffab_metrics_hbonds, diffab_metrics_motifs), the context of a patch
// compacted (diffab_metrics_contacts, diffab_metrics_contact_bits; the classification of a slot also diffab_metrics_surface), the contact
// decision of those two entries, and the site of a residue (diffab_metrics_patches, diffab_metrics_pair_energy).  Nothing here asks at
// run time which entry it serves: where two entries differ, the difference is a template parameter or stays in the entry's own file.
//
// The kernels are templates in an unnamed namespace, so every translation unit that launches one owns its instance.  The fp32 results
// are defined numbers only in a translation unit built with -ffp-contract=off (analysis_common.h).
#pragma once
#include "analysis_common.h"

namespace diffab {

// ------------------------------------------------------------------ chain neighbours of a patch
// Slots a and b are bonded when they are on the same chain and their residue_idx differ by one, in either direction.  The gap is taken
// in 64 bits: residue_idx INT32_MAX next to INT32_MIN are not neighbours.  (Whether both are inside residue_mask is the caller's to ask.)
__device__ __forceinline__ bool bonded(int chain_a, int idx_a, int chain_b, int idx_b) {
  const int64_t gap = static_cast<int64_t>(idx_b) - idx_a;
  return chain_a == chain_b && (gap == 1 || gap == -1);
}

// The keys of the chain rule of a patch, for LDS: key[k] = (chain, residue_idx), in[k] = inside residue_mask.  A barrier follows.
template <int kThreads>
__device__ __forceinline__ void stage_chain_keys(const int32_t* __restrict__ chain, const int32_t* __restrict__ residue_idx,
                                                 const uint8_t* __restrict__ residue_mask, int64_t base, int K, int2* key, uint8_t* in) {
  for (int k = threadIdx.x; k < K; k += kThreads) {
    key[k] = make_int2(chain[base + k], residue_idx[base + k]);
    in[k] = residue_mask == nullptr || residue_mask[base + k] != 0;
  }
}

// succ / pred of slot k: the lowest slot j of the patch with the same chain, residue_idx[j] = residue_idx[k] + 1 / - 1 and both inside
// residue_mask; -1 without one.
struct ChainLinks {
  int succ, pred;
};
__device__ __forceinline__ ChainLinks chain_links(const int2* key, const uint8_t* in, int K, int k) {
  ChainLinks l{-1, -1};
  if (!in[k]) return l;
  const int2 me = key[k];
  for (int j = 0; j < K; ++j) {
    if (!in[j] || key[j].x != me.x) continue;
    const int64_t gap = static_cast<int64_t>(key[j].y) - me.y;
    if (gap == 1 && l.succ < 0) l.succ = j;
    if (gap == -1 && l.pred < 0) l.pred = j;
  }
  return l;
}

struct LinkWorkspace {
  int32_t* succ;  // (G, K)
  int32_t* pred;  // (G, K)
  size_t bytes;
};

inline LinkWorkspace carve_links(void* base, int64_t G, int64_t K) {
  Carver c(base);
  LinkWorkspace w;
  w.succ = c.take<int32_t>(static_cast<size_t>(G * K));
  w.pred = c.take<int32_t>(static_cast<size_t>(G * K));
  w.bytes = c.bytes();
  return w;
}

// ------------------------------------------------------------------ the context of a patch, compacted
// The inclusive prefix sum of v over the lanes of a wave: lane l ends with v of lanes 0 .. l.
__device__ __forceinline__ int wave_inclusive_scan(int v, int lane) {
  int incl = v;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const int t = __shfl_up(incl, d, 64);
    if (lane >= d) incl += t;
  }
  return incl;
}

// What slot k of a patch is.  Everything is false / zero behind K and outside residue_mask; a generated slot is neither antigen nor
// hotspot and has no context atoms; a hotspot is an antigen slot.
struct SlotClass {
  bool in, gen, antigen, hot;
  uint32_t bits;  // the valid context atoms of a non-generated slot
};
__device__ __forceinline__ SlotClass classify_slot(int k, int K, int64_t base, const uint8_t* __restrict__ residue_mask,
                                                   const uint8_t* __restrict__ generation_mask, const uint8_t* __restrict__ antigen_mask,
                                                   const uint8_t* __restrict__ hotspot_mask, const uint32_t* __restrict__ ctx_valid,
                                                   uint32_t amask) {
  SlotClass c;
  c.in = k < K && (residue_mask == nullptr || residue_mask[base + k] != 0);
  c.gen = c.in && generation_mask[base + k] != 0;
  c.bits = (c.in && !c.gen) ? (ctx_valid[base + k] & amask) : 0u;
  c.antigen = c.in && !c.gen && antigen_mask != nullptr && antigen_mask[base + k] != 0;
  c.hot = c.antigen && hotspot_mask != nullptr && hotspot_mask[base + k] != 0;
  return c;
}

__device__ __forceinline__ uint32_t atom_mask_of(int A) { return A >= 32 ? 0xFFFFFFFFu : ((1u << A) - 1u); }

// Per patch, the context side compacted once for all its designs (the head of an entry's workspace).
struct ContextWorkspace {
  float4* atoms;  // (G, K*A): the valid atoms of the listed context residues, in residue order
  int4* res;      // (G, K): listed context residues (non-generated, inside residue_mask, >= 1 valid atom): slot, first atom, atoms, flags
  int2* key;      // (G, K): chain and residue_idx of the same
  int32_t* gen;   // (G, K): slots of the generated residues inside residue_mask, ascending
  int4* hdr;      // (G): generated residues, listed context residues, context atoms, hotspot residues
};
constexpr int kFlagAntigen = 1, kFlagHotspot = 2;  // ContextWorkspace::res[].w

inline ContextWorkspace carve_context(Carver& c, int64_t G, int64_t K, int64_t A) {
  ContextWorkspace w;
  w.atoms = c.take<float4>(static_cast<size_t>(G * K * A));
  w.res = c.take<int4>(static_cast<size_t>(G * K));
  w.key = c.take<int2>(static_cast<size_t>(G * K));
  w.gen = c.take<int32_t>(static_cast<size_t>(G * K));
  w.hdr = c.take<int4>(static_cast<size_t>(G));
  return w;
}

// ------------------------------------------------------------------ the contact decision
// The squared distance of an own atom and another atom, +inf unless both are valid: a clash and a contact are strict comparisons on it.
__device__ __forceinline__ float masked_dist2(float ax, float ay, float az, float bx, float by, float bz, bool both_valid) {
  const float d2 = dist2(ax, ay, az, bx, by, bz);
  return both_valid ? d2 : INFINITY;
}

// ------------------------------------------------------------------ one site per residue
// The record of a slot from what the patch knows (SiteRecord of analysis_common.h); the entry decides what present, generated and antigen
// mean.  `site` is the context's site of the slot.
__device__ __forceinline__ SiteRecord pack_site(const float* __restrict__ site, bool present, bool gen, bool antigen) {
  SiteRecord r;
  r.x = r.y = r.z = present ? 0.f : NAN;
  r.flags = (present ? kSitePresent : 0u) | (gen ? kSiteGenerated : 0u) | (antigen ? kSiteAntigen : 0u);
  if (present && !gen) r.x = site[0], r.y = site[1], r.z = site[2];
  return r;
}

// The record of a slot in a design row: the patch's record, with the row's own site where the residue is generated.
__device__ __forceinline__ SiteRecord overlay_site(SiteRecord r, const float* __restrict__ row_site) {
  if ((r.flags & kSiteGenerated) != 0u) r.x = row_site[0], r.y = row_site[1], r.z = row_site[2];
  return r;
}

namespace {

// One work-group per patch, the keys in LDS: succ and, unless it is null, pred of every slot.
template <int kThreads, int kMaxK>
__global__ void __launch_bounds__(kThreads)
chain_links_kernel(const int32_t* __restrict__ chain, const int32_t* __restrict__ residue_idx, const uint8_t* __restrict__ residue_mask,
                   int K, int32_t* __restrict__ succ, int32_t* __restrict__ pred) {
  __shared__ int2 s_key[kMaxK];
  __shared__ uint8_t s_in[kMaxK];
  const int64_t base = static_cast<int64_t>(blockIdx.x) * K;
  stage_chain_keys<kThreads>(chain, residue_idx, residue_mask, base, K, s_key, s_in);
  __syncthreads();
  for (int k = threadIdx.x; k < K; k += kThreads) {
    const ChainLinks l = chain_links(s_key, s_in, K, k);
    succ[base + k] = l.succ;
    if (pred != nullptr) pred[base + k] = l.pred;
  }
}

// One work-group of 256 threads per patch.  Wave 0 lists the residues in ascending order (ballots and a wave prefix sum over the atom
// counts), then all threads copy the valid atoms behind each other.  kAntigenOnly: only antigen residues are listed, and wstart
// (G, W + 1) takes the first listed residue whose slot is >= 32 w, [W] = the number of listed residues (W = ceil(K / 32) word columns).
template <bool kAntigenOnly, int kMaxK>
__global__ void __launch_bounds__(256)
context_pack_kernel(const float* __restrict__ ctx_points, const uint32_t* __restrict__ ctx_valid, const uint8_t* __restrict__ generation_mask,
                    const uint8_t* __restrict__ residue_mask, const uint8_t* __restrict__ antigen_mask, const uint8_t* __restrict__ hotspot_mask,
                    const int32_t* __restrict__ chain, const int32_t* __restrict__ residue_idx, int K, int A, ContextWorkspace ws,
                    int32_t* __restrict__ wstart) {
  __shared__ int s_begin[kMaxK];  // first atom of a listed context residue, -1 for every other slot
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int W = (K + 31) / 32;
  const int64_t g = blockIdx.x, base = g * K;
  const uint32_t amask = atom_mask_of(A);
  if (wave == 0) {
    int ng = 0, nr = 0, na = 0, nh = 0;
    for (int k0 = 0; k0 < K; k0 += 64) {
      const int k = k0 + lane;
      const SlotClass c = classify_slot(k, K, base, residue_mask, generation_mask, antigen_mask, hotspot_mask, ctx_valid, amask);
      const int cnt = __popc((kAntigenOnly && !c.antigen) ? 0u : c.bits);
      const BallotRank rg = ballot_rank(c.gen, lane);
      if (c.gen) ws.gen[base + ng + rg.rank] = k;
      ng += rg.count;
      const bool listed = cnt > 0;
      const unsigned long long vr = __ballot(listed);
      const int incl = wave_inclusive_scan(cnt, lane);
      const int begin = na + incl - cnt;
      if (listed) {
        const int r = nr + __popcll(vr & ((1ull << lane) - 1ull));
        ws.res[base + r] = make_int4(k, begin, cnt, (c.antigen ? kFlagAntigen : 0) | (c.hot ? kFlagHotspot : 0));
        ws.key[base + r] = make_int2(chain[base + k], residue_idx[base + k]);
      }
      if (k < K) s_begin[k] = listed ? begin : -1;
      if (kAntigenOnly && lane == 0) {
        wstart[g * (W + 1) + k0 / 32] = nr;
        if (k0 / 32 + 1 < W) wstart[g * (W + 1) + k0 / 32 + 1] = nr + __popcll(vr & 0xFFFFFFFFull);
      }
      nr += __popcll(vr);
      na += __shfl(incl, 63, 64);
      nh += __popcll(__ballot(c.hot));
    }
    if (lane == 0) {
      if (kAntigenOnly) wstart[g * (W + 1) + W] = nr;
      ws.hdr[g] = make_int4(ng, nr, na, nh);
    }
  }
  __syncthreads();
  float4* out = ws.atoms + base * A;
  for (int t = tid; t < K * A; t += 256) {
    const int k = t / A, a = t - k * A;
    const int b = s_begin[k];
    if (b < 0) continue;
    const uint32_t bits = ctx_valid[base + k] & amask;
    if (((bits >> a) & 1u) == 0u) continue;
    const float* p = ctx_points + ((base + k) * A + a) * 3;
    out[b + __popc(bits & ((1u << a) - 1u))] = make_float4(p[0], p[1], p[2], 0.f);
  }
}

}  // namespace
}  // namespace diffab
