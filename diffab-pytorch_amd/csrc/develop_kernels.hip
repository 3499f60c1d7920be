// develop_kernels.hip - developability of a design on the device: diffab_metrics_patches, hydrophobic and charged
// surface patches on one site per residue, and diffab_metrics_motifs, sequence motifs along the chain.  The rules are the header
// comments of the two entries in include/diffab_hip_develop.h.
//
// Built with -ffp-contract=off like the other defined numbers (csrc/Makefile): the squared distance is the fp32 value
// (dx*dx + dy*dy) + dz*dz (dist2 of analysis_common.h, written out here) and every decision is one strict comparison on it.  A pair term is
// w_i * w_j / max(d2, min^2) in fp64 - the product of two fp32 values is exact in fp64 and the build has no fast-math flag, so the
// quotient is correctly rounded - and the sums are fp64 in a fixed order, rounded to fp32 once.  The motifs are integer work on bits.
// VALU + LDS only; no atomics; every value reaches memory through plain C++ stores.
#include <climits>
#include <cmath>

#include "../../include/diffab_hip_develop.h"
#include "analysis_prep.h"

namespace diffab {
namespace {

constexpr int kMaxK = DIFFAB_DEVELOP_MAX_K;
constexpr int kMaxClasses = DIFFAB_DEVELOP_MAX_CLASSES;
constexpr int kMaxMotifs = DIFFAB_DEVELOP_MAX_MOTIFS;
constexpr int kMotifWords = DIFFAB_DEVELOP_MOTIF_WORDS;
static_assert(kMaxK % 64 == 0 && kMaxK <= 65535, "lane l owns residues l, l + 64, ...; the list of exposed residues holds 16-bit slots");
static_assert(kMaxMotifs <= 32 && kMaxClasses <= 32, "one bit per motif in motif_start, one bit per class in a motif word");

constexpr uint8_t kStatePresent = 1, kStateScope = 2, kStateExposed = 4;  // the bits of the state output

// ------------------------------------------------------------------ 1. surface patches
struct PatchesWorkspace {
  SiteRecord* site;  // (G, K): the antigen is not present here, so flags are kSitePresent | kSiteGenerated
  size_t bytes;
};

PatchesWorkspace carve_patches(void* base, int64_t G, int64_t K) {
  Carver c(base);
  PatchesWorkspace w;
  w.site = c.take<SiteRecord>(static_cast<size_t>(G * K));
  w.bytes = c.bytes();
  return w;
}

__global__ void __launch_bounds__(64)
patches_pack_kernel(const float* __restrict__ context_sites, const uint8_t* __restrict__ generation_mask, const uint8_t* __restrict__ residue_mask,
                    const uint8_t* __restrict__ antigen_mask, int K, PatchesWorkspace ws) {
  const int64_t base = static_cast<int64_t>(blockIdx.x) * K;
  for (int k = threadIdx.x; k < K; k += 64) {
    const bool in = residue_mask == nullptr || residue_mask[base + k] != 0;
    const bool antigen = antigen_mask != nullptr && antigen_mask[base + k] != 0;
    const bool present = in && !antigen;
    const bool gen = present && generation_mask[base + k] != 0;
    ws.site[base + k] = pack_site(context_sites + (base + k) * 3, present, gen, false);
  }
}

struct PatchesArgs {
  const float* sites;
  const int32_t* tokens;
  const uint8_t* exposed_in;
  const float* hydrophobicity;
  const float* charge;
  int N, K, V, max_neighbours;
  float neighbour2, vicinity2, patch2, min2;
  float *psh, *ppc, *pnc, *charge_generated, *charge_scope;
  int32_t *n_scope, *n_exposed, *n_pairs;
  float *residue_psh, *residue_ppc, *residue_pnc;
  int32_t* n_neighbours;
  uint8_t* state;
};

// One wave per design row; lane l owns residues l, l + 64, ...  Every lane reads the same s_site[j] in the inner loops (an LDS
// broadcast) against its own residue, held in registers.  LDS is sized by K (kPatchesLdsPerResidue bytes per residue), so that the
// patches of the sampler (K = 128, 3.4 KiB) run eight waves per SIMD where K = 512 (13.5 KiB) runs three.
constexpr int kPatchesLdsPerResidue = sizeof(SiteRecord) + 2 * sizeof(float) + sizeof(uint16_t) + sizeof(uint8_t);

__global__ void __launch_bounds__(64)
patches_row_kernel(PatchesArgs a, PatchesWorkspace ws) {
  extern __shared__ __attribute__((aligned(16))) unsigned char s_raw[];
  const int lane = threadIdx.x, K = a.K;
  SiteRecord* s_site = reinterpret_cast<SiteRecord*>(s_raw);
  float* s_h = reinterpret_cast<float*>(s_site + K);
  float* s_q = s_h + K;
  uint16_t* s_list = reinterpret_cast<uint16_t*>(s_q + K);  // the exposed residues, ascending
  uint8_t* s_state = reinterpret_cast<uint8_t*>(s_list + K);

  const int64_t row = blockIdx.x, g = row / a.N;
  const int64_t rbase = row * K, gbase = g * K;
  const unsigned long long below = (1ull << lane) - 1ull;

  for (int k = lane; k < K; k += 64) {
    const SiteRecord r = overlay_site(ws.site[gbase + k], a.sites + (rbase + k) * 3);
    const int tok = a.tokens[rbase + k];
    const bool known = tok >= 0 && tok < a.V;
    const float h = a.hydrophobicity[known ? tok : 0], q = a.charge[known ? tok : 0];
    s_site[k] = r;
    s_h[k] = known ? h : 0.f;
    s_q[k] = known ? q : 0.f;
  }
  __syncthreads();

  // ---- pass 1: neighbour counts, scope, exposure, the two charges
  double sum_qgen = 0.0, sum_qscope = 0.0;
  int n_scope = 0, n_exposed = 0;
  for (int i0 = 0; i0 < K; i0 += 64) {
    const int i = i0 + lane;
    const bool mine = i < K;
    SiteRecord me;
    me.x = me.y = me.z = NAN, me.flags = 0u;
    if (mine) me = s_site[i];
    int count = 0;
    bool near = false;
#pragma unroll 4
    for (int j = 0; j < K; ++j) {
      const SiteRecord o = s_site[j];
      const float dx = me.x - o.x, dy = me.y - o.y, dz = me.z - o.z;
      const float d2 = (dx * dx + dy * dy) + dz * dz;
      count += (d2 < a.neighbour2 && j != i) ? 1 : 0;
      near |= d2 < a.vicinity2 && (o.flags & kSiteGenerated) != 0u;
    }
    const bool present = (me.flags & kSitePresent) != 0u, gen = (me.flags & kSiteGenerated) != 0u;
    const bool scope = present && (gen || near);
    bool exposed = scope && count <= a.max_neighbours;
    if (a.exposed_in != nullptr) exposed = scope && mine && a.exposed_in[rbase + (mine ? i : 0)] != 0;
    const unsigned long long vs = __ballot(scope), ve = __ballot(exposed);
    if (exposed) s_list[n_exposed + __popcll(ve & below)] = static_cast<uint16_t>(i);
    n_scope += __popcll(vs);
    n_exposed += __popcll(ve);
    if (mine) {
      const double q = static_cast<double>(s_q[i]);
      sum_qgen += gen ? q : 0.0;
      sum_qscope += scope ? q : 0.0;
      const uint8_t st = (present ? kStatePresent : 0) | (scope ? kStateScope : 0) | (exposed ? kStateExposed : 0);
      s_state[i] = st;
      if (a.n_neighbours != nullptr) a.n_neighbours[rbase + i] = count;
      if (a.state != nullptr) a.state[rbase + i] = st;
    }
  }
  __syncthreads();

  // ---- pass 2: the pair terms of every exposed residue, partners in ascending order
  double sum_h = 0.0, sum_p = 0.0, sum_n = 0.0;
  int pairs = 0;
  for (int i0 = 0; i0 < K; i0 += 64) {
    const int i = i0 + lane;
    const bool mine = i < K;
    const bool exposed = mine && (s_state[mine ? i : 0] & kStateExposed) != 0;
    double rh = 0.0, rp = 0.0, rn = 0.0;
    if (__ballot(exposed) != 0ull) {  // (uniform)
      const SiteRecord me = s_site[mine ? i : 0];
      const float qi = s_q[mine ? i : 0];
      const double hi = static_cast<double>(s_h[mine ? i : 0]);
      for (int e = 0; e < n_exposed; ++e) {
        const int j = s_list[e];
        const SiteRecord o = s_site[j];
        const float dx = me.x - o.x, dy = me.y - o.y, dz = me.z - o.z;
        const float d2 = (dx * dx + dy * dy) + dz * dz;
        if (exposed && j != i && d2 < a.patch2) {
          const double m = static_cast<double>(fmaxf(d2, a.min2));
          const float qj = s_q[j];
          ++pairs;
          rh += hi * static_cast<double>(s_h[j]) / m;
          if (qi > 0.f && qj > 0.f) rp += static_cast<double>(qi) * static_cast<double>(qj) / m;
          if (qi < 0.f && qj < 0.f) rn += static_cast<double>(qi) * static_cast<double>(qj) / m;
        }
      }
    }
    if (mine) {
      if (a.residue_psh != nullptr) a.residue_psh[rbase + i] = static_cast<float>(rh);
      if (a.residue_ppc != nullptr) a.residue_ppc[rbase + i] = static_cast<float>(rp);
      if (a.residue_pnc != nullptr) a.residue_pnc[rbase + i] = static_cast<float>(rn);
    }
    sum_h += rh, sum_p += rp, sum_n += rn;
  }

  sum_h = wave_sum(sum_h), sum_p = wave_sum(sum_p), sum_n = wave_sum(sum_n);
  sum_qgen = wave_sum(sum_qgen), sum_qscope = wave_sum(sum_qscope);
  pairs = wave_sum(pairs);
  if (lane == 0) {  // every pair is in the sums of both its residues; halving is exact
    if (a.psh != nullptr) a.psh[row] = static_cast<float>(0.5 * sum_h);
    if (a.ppc != nullptr) a.ppc[row] = static_cast<float>(0.5 * sum_p);
    if (a.pnc != nullptr) a.pnc[row] = static_cast<float>(0.5 * sum_n);
    if (a.charge_generated != nullptr) a.charge_generated[row] = static_cast<float>(sum_qgen);
    if (a.charge_scope != nullptr) a.charge_scope[row] = static_cast<float>(sum_qscope);
    if (a.n_scope != nullptr) a.n_scope[row] = n_scope;
    if (a.n_exposed != nullptr) a.n_exposed[row] = n_exposed;
    if (a.n_pairs != nullptr) a.n_pairs[row] = pairs / 2;
  }
}

// ------------------------------------------------------------------ 2. sequence motifs
struct MotifsWorkspace {
  int32_t* succ;  // (G, K): the chain successor of every slot, -1 without one (chain_links_kernel of analysis_prep.h, no pred)
  size_t bytes;
};

MotifsWorkspace carve_motifs(void* base, int64_t G, int64_t K) {
  Carver c(base);
  MotifsWorkspace w;
  w.succ = c.take<int32_t>(static_cast<size_t>(G * K));
  w.bytes = c.bytes();
  return w;
}

struct MotifTable {
  int32_t word[kMaxMotifs * kMotifWords];
};

// One wave per design row; lane l owns slots l, l + 64, ...  A slot outside residue_mask has no class bit, so it matches nothing.
__global__ void __launch_bounds__(64)
motifs_row_kernel(const int32_t* __restrict__ tokens, const uint8_t* __restrict__ generation_mask, const uint8_t* __restrict__ residue_mask,
                  int N, int K, int M, MotifTable table, MotifsWorkspace ws, int32_t* __restrict__ motif_count, int32_t* __restrict__ n_motifs,
                  int32_t* __restrict__ motif_start) {
  __shared__ uint32_t s_bit[kMaxK];
  __shared__ int32_t s_succ[kMaxK];
  __shared__ uint8_t s_gen[kMaxK];
  __shared__ uint32_t s_word[kMaxMotifs * kMotifWords];
  const int lane = threadIdx.x;
  const int64_t row = blockIdx.x, g = row / N;
  const int64_t rbase = row * K, gbase = g * K;
  for (int t = lane; t < M * kMotifWords; t += 64) s_word[t] = static_cast<uint32_t>(table.word[t]);
  for (int k = lane; k < K; k += 64) {
    const int tok = tokens[rbase + k];
    const bool in = residue_mask == nullptr || residue_mask[gbase + k] != 0;
    s_bit[k] = (in && tok >= 0 && tok < 32) ? (1u << tok) : 0u;
    s_succ[k] = ws.succ[gbase + k];
    s_gen[k] = generation_mask[gbase + k] != 0;
  }
  __syncthreads();

  int count = 0;  // lane m: the counted matches of motif m
  for (int i0 = 0; i0 < K; i0 += 64) {
    const int i = i0 + lane;
    uint32_t start = 0u;
    for (int m = 0; m < M; ++m) {
      bool ok = i < K, generated = false;
      int s = i;
      for (int p = 0; p < kMotifWords; ++p) {
        const uint32_t w = s_word[m * kMotifWords + p];
        if (w == 0u) break;  // (uniform)
        if (ok) {
          if (s < 0) {
            ok = false;
          } else {
            ok = (s_bit[s] & w) != 0u;
            generated |= s_gen[s] != 0;
            s = s_succ[s];
          }
        }
      }
      const bool hit = ok && generated;
      const unsigned long long v = __ballot(hit);
      if (lane == m) count += __popcll(v);
      if (hit) start |= 1u << m;
    }
    if (i < K && motif_start != nullptr) motif_start[rbase + i] = static_cast<int32_t>(start);
  }
  if (lane < M && motif_count != nullptr) motif_count[row * M + lane] = count;
  const int total = wave_sum(lane < M ? count : 0);
  if (lane == 0 && n_motifs != nullptr) n_motifs[row] = total;
}

}  // namespace
}  // namespace diffab

using namespace diffab;

extern "C" {

int diffab_metrics_patches(const float* sites, const float* context_sites, const int32_t* tokens, const uint8_t* generation_mask,
                           const uint8_t* residue_mask, const uint8_t* antigen_mask, const uint8_t* exposed_in, const float* hydrophobicity,
                           const float* charge, int32_t rows, int32_t group_size, int32_t K, int32_t V, float neighbour_distance,
                           int32_t max_neighbours, float vicinity_distance, float patch_distance, float min_distance, float* psh, float* ppc,
                           float* pnc, float* charge_generated, float* charge_scope, int32_t* n_scope, int32_t* n_exposed, int32_t* n_pairs,
                           float* residue_psh, float* residue_ppc, float* residue_pnc, int32_t* n_neighbours, uint8_t* state,
                           void* workspace, size_t workspace_bytes, void* stream) {
  StreamOrder order_(stream);
  const char* who = "metrics_patches";
  if (!rows_shape_ok(who, rows, group_size, K, kMaxK)) return DIFFAB_ERR_ARG;
  DIFFAB_REQUIRE(V >= 1 && V <= kMaxClasses, DIFFAB_ERR_ARG, "%s: V = %d classes outside [1, %d]", who, V, kMaxClasses);
  DIFFAB_REQUIRE(finite_nonnegative(neighbour_distance), DIFFAB_ERR_ARG, "%s: neighbour_distance must be finite and >= 0, got %g", who,
                 static_cast<double>(neighbour_distance));
  DIFFAB_REQUIRE(max_neighbours >= 0, DIFFAB_ERR_ARG, "%s: max_neighbours must be >= 0, got %d", who, max_neighbours);
  DIFFAB_REQUIRE(finite_nonnegative(vicinity_distance), DIFFAB_ERR_ARG, "%s: vicinity_distance must be finite and >= 0, got %g", who,
                 static_cast<double>(vicinity_distance));
  DIFFAB_REQUIRE(finite_nonnegative(patch_distance), DIFFAB_ERR_ARG, "%s: patch_distance must be finite and >= 0, got %g", who,
                 static_cast<double>(patch_distance));
  DIFFAB_REQUIRE(min_distance > 0.f && min_distance < INFINITY, DIFFAB_ERR_ARG, "%s: min_distance must be finite and > 0, got %g", who,
                 static_cast<double>(min_distance));
  const float min2 = min_distance * min_distance;
  DIFFAB_REQUIRE(min2 > 0.f && min2 < INFINITY, DIFFAB_ERR_ARG, "%s: min_distance = %g has no fp32 square to divide by", who,
                 static_cast<double>(min_distance));
  if (rows == 0) return DIFFAB_OK;
  DIFFAB_REQUIRE(sites && context_sites && tokens && generation_mask && hydrophobicity && charge, DIFFAB_ERR_ARG, "%s: null input", who);
  const int32_t G = rows / group_size;
  const PatchesWorkspace ws = carve_patches(workspace, G, K);
  if (const int e = workspace_ok(who, workspace, 256, workspace_bytes, ws.bytes)) return e;
  hipStream_t st = as_stream(stream);
  hipLaunchKernelGGL(patches_pack_kernel, dim3(G), dim3(64), 0, st, context_sites, generation_mask, residue_mask, antigen_mask, K, ws);
  PatchesArgs a;
  a.sites = sites, a.tokens = tokens, a.exposed_in = exposed_in, a.hydrophobicity = hydrophobicity, a.charge = charge;
  a.N = group_size, a.K = K, a.V = V, a.max_neighbours = max_neighbours;
  a.neighbour2 = neighbour_distance * neighbour_distance, a.vicinity2 = vicinity_distance * vicinity_distance;
  a.patch2 = patch_distance * patch_distance, a.min2 = min2;
  a.psh = psh, a.ppc = ppc, a.pnc = pnc, a.charge_generated = charge_generated, a.charge_scope = charge_scope;
  a.n_scope = n_scope, a.n_exposed = n_exposed, a.n_pairs = n_pairs;
  a.residue_psh = residue_psh, a.residue_ppc = residue_ppc, a.residue_pnc = residue_pnc, a.n_neighbours = n_neighbours, a.state = state;
  hipLaunchKernelGGL(patches_row_kernel, dim3(rows), dim3(64), static_cast<size_t>(K) * kPatchesLdsPerResidue, st, a, ws);
  DIFFAB_LAUNCH_CHECK();
  return DIFFAB_OK;
}

int diffab_metrics_motifs(const int32_t* tokens, const uint8_t* generation_mask, const uint8_t* residue_mask, const int32_t* chain,
                          const int32_t* residue_idx, const int32_t* motifs, int32_t rows, int32_t group_size, int32_t K, int32_t M,
                          int32_t* motif_count, int32_t* n_motifs, int32_t* motif_start, void* workspace, size_t workspace_bytes,
                          void* stream) {
  StreamOrder order_(stream);
  const char* who = "metrics_motifs";
  if (!rows_shape_ok(who, rows, group_size, K, kMaxK)) return DIFFAB_ERR_ARG;
  DIFFAB_REQUIRE(M >= 1 && M <= kMaxMotifs, DIFFAB_ERR_ARG, "%s: M = %d motifs outside [1, %d]", who, M, kMaxMotifs);
  if (rows == 0) return DIFFAB_OK;
  DIFFAB_REQUIRE(tokens && generation_mask && chain && residue_idx, DIFFAB_ERR_ARG, "%s: null input", who);
  DIFFAB_REQUIRE(motifs != nullptr, DIFFAB_ERR_ARG, "%s: null motifs (a host array of %d words per motif)", who, kMotifWords);
  MotifTable table;
  for (int t = 0; t < kMaxMotifs * kMotifWords; ++t) table.word[t] = 0;
  for (int m = 0; m < M; ++m) {
    DIFFAB_REQUIRE(motifs[m * kMotifWords] != 0, DIFFAB_ERR_ARG, "%s: motifs: word 0 of motif %d is zero (an empty motif)", who, m);
    for (int p = 0; p < kMotifWords; ++p) {
      DIFFAB_REQUIRE(p == 0 || motifs[m * kMotifWords + p] == 0 || motifs[m * kMotifWords + p - 1] != 0, DIFFAB_ERR_ARG,
                     "%s: motifs: word %d of motif %d is non-zero after a zero word", who, p, m);
      table.word[m * kMotifWords + p] = motifs[m * kMotifWords + p];
    }
  }
  const int32_t G = rows / group_size;
  const MotifsWorkspace ws = carve_motifs(workspace, G, K);
  if (const int e = workspace_ok(who, workspace, 256, workspace_bytes, ws.bytes)) return e;
  if (motif_count == nullptr && n_motifs == nullptr && motif_start == nullptr) return DIFFAB_OK;  // nothing was asked for
  hipStream_t st = as_stream(stream);
  hipLaunchKernelGGL((chain_links_kernel<64, kMaxK>), dim3(G), dim3(64), 0, st, chain, residue_idx, residue_mask, K, ws.succ,
                     static_cast<int32_t*>(nullptr));
  hipLaunchKernelGGL(motifs_row_kernel, dim3(rows), dim3(64), 0, st, tokens, generation_mask, residue_mask, group_size, K, M, table, ws,
                     motif_count, n_motifs, motif_start);
  DIFFAB_LAUNCH_CHECK();
  return DIFFAB_OK;
}

}  // extern "C"
