// energy_kernels.hip - a distance-binned residue pair potential over the pairs a design takes part in:
// diffab_metrics_pair_energy.  The rule is the header comment of the entry in include/diffab_hip_energy.h.
//
// Built with -ffp-contract=off like the other defined numbers (csrc/Makefile): the squared distance is dist2 of
// analysis_common.h and a pair's bin is decided by comparisons on it.  A term is one fp32 table
// entry, exact in fp64, and the sums are fp64 in a fixed order, rounded to fp32 once.  VALU + LDS only; no atomics; every value reaches
// memory through plain C++ stores.
#include <cmath>

#include "../../include/diffab_hip_energy.h"
#include "analysis_prep.h"

namespace diffab {
namespace {

constexpr int kMaxK = DIFFAB_ENERGY_MAX_K;
constexpr int kMaxClasses = DIFFAB_ENERGY_MAX_CLASSES;
constexpr int kMaxBins = DIFFAB_ENERGY_MAX_BINS;
constexpr int kMaxWaves = 4;            // design rows (one wave each) of a work-group: they share one copy of the table
constexpr int kLdsBudget = 64 * 1024;   // dynamic LDS of one work-group
static_assert(kMaxK % 64 == 0 && kMaxK <= 65535, "lane l owns residues l, l + 64, ...; the lists hold 16-bit slots");
static_assert(kMaxClasses == 32, "the scan gives every class one lane of a half wave; a token takes five bits of a record's flags");
static_assert(kMaxK / 64 * kMaxK < 65536, "a lane's pairs of one class and bin are counted in 16 bits");

// SiteRecord::flags beside the shared ones: kKnown and the token (bits 8..12) are the row kernel's, a token inside [0, V).
constexpr uint32_t kKnown = 8u;
constexpr int kTokenShift = 8;
enum { kClassAntigen = 0, kClassFramework = 1, kClassInternal = 2 };

struct EnergyWorkspace {
  SiteRecord* site;  // (G, K)
  int32_t* chain;    // (G, K), zeros without chain / residue_idx
  int32_t* ridx;     // (G, K)
  size_t bytes;
};

EnergyWorkspace carve_energy(void* base, int64_t G, int64_t K) {
  Carver c(base);
  EnergyWorkspace w;
  w.site = c.take<SiteRecord>(static_cast<size_t>(G * K));
  w.chain = c.take<int32_t>(static_cast<size_t>(G * K));
  w.ridx = c.take<int32_t>(static_cast<size_t>(G * K));
  w.bytes = c.bytes();
  return w;
}

__global__ void __launch_bounds__(64)
energy_pack_kernel(const float* __restrict__ context_sites, const uint8_t* __restrict__ generation_mask, const uint8_t* __restrict__ residue_mask,
                   const uint8_t* __restrict__ antigen_mask, const int32_t* __restrict__ chain, const int32_t* __restrict__ residue_idx, int K,
                   EnergyWorkspace ws) {
  const int64_t base = static_cast<int64_t>(blockIdx.x) * K;
  for (int k = threadIdx.x; k < K; k += 64) {
    const bool present = residue_mask == nullptr || residue_mask[base + k] != 0;
    const bool gen = present && generation_mask[base + k] != 0;
    const bool antigen = present && !gen && antigen_mask != nullptr && antigen_mask[base + k] != 0;
    ws.site[base + k] = pack_site(context_sites + (base + k) * 3, present, gen, antigen);
    ws.chain[base + k] = chain != nullptr ? chain[base + k] : 0;
    ws.ridx[base + k] = residue_idx != nullptr ? residue_idx[base + k] : 0;
  }
}

struct EnergyArgs {
  const float* sites;
  const int32_t* tokens;
  const float* table;
  int rows, N, K, V, Vp, NB, waves;  // Vp: the LDS length of a table row, V made odd
  int min_sep;                       // 0 without chain / residue_idx: no pair is skipped
  int table_bytes, wave_bytes;       // LDS: the table, then one block of wave_bytes per wave
  float e2[kMaxBins + 1];            // the fp32 squares of the edges, +inf behind e2[NB]
  float *e_antigen, *e_framework, *e_internal;
  int32_t* n_pairs;
  float *residue_energy, *residue_antigen_energy;
  int32_t* n_partners;
  float* substitution;
};

// The bin of the pair, -1 without one: the number of edges at or below d2 is 1 ... NB for a pair with a bin, 0 below e2[0] or for a
// NaN, and more than NB at or beyond e2[NB] (the edges behind NB are +inf, which only an infinite d2 reaches).
__device__ __forceinline__ int bin_of(const SiteRecord& me, const SiteRecord& o, const EnergyArgs& a) {
  const float d2 = dist2(me.x, me.y, me.z, o.x, o.y, o.z);
  int n = 0;
#pragma unroll
  for (int b = 0; b <= kMaxBins; ++b) n += d2 >= a.e2[b] ? 1 : 0;
  return (n >= 1 && n <= a.NB) ? n - 1 : -1;
}

__device__ __forceinline__ bool too_near(int ci, int64_t ri, int cj, int64_t rj, int min_sep) {
  const int64_t d = ri - rj;
  return ci == cj && (d < 0 ? -d : d) < static_cast<int64_t>(min_sep);
}

// One wave per design row, a.waves rows per work-group; lane l owns residues l, l + 64, ...  Every lane reads the same record in the
// inner loops (an LDS broadcast) against its own residue, held in registers.  A wave behind the last row runs the last row again and
// stores nothing, so that every wave meets the same barriers.
__global__ void __launch_bounds__(64 * kMaxWaves)
energy_row_kernel(EnergyArgs a, EnergyWorkspace ws) {
  extern __shared__ __attribute__((aligned(16))) unsigned char s_raw[];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, K = a.K, V = a.V, Vp = a.Vp;
  float* s_table = reinterpret_cast<float*>(s_raw);  // [b][first][second], rows of Vp
  unsigned char* s_mine = s_raw + a.table_bytes + static_cast<size_t>(wave) * a.wave_bytes;
  SiteRecord* s_site = reinterpret_cast<SiteRecord*>(s_mine);
  int32_t* s_chain = reinterpret_cast<int32_t*>(s_site + K);
  int32_t* s_ridx = s_chain + K;
  uint16_t* s_gen = reinterpret_cast<uint16_t*>(s_ridx + K);  // the generated residues, ascending
  uint16_t* s_ag = s_gen + K;                                 // the antigen residues with a token of the table, ascending

  int64_t row = static_cast<int64_t>(blockIdx.x) * a.waves + wave;
  const bool live = row < a.rows;
  row = live ? row : a.rows - 1;
  const int64_t g = row / a.N, rbase = row * K, gbase = g * K;
  const unsigned long long below = (1ull << lane) - 1ull;

  for (int t = threadIdx.x; t < a.NB * V * V; t += blockDim.x) s_table[(t / V) * Vp + t % V] = a.table[t];
  int n_gen = 0, n_ag = 0;
  for (int i0 = 0; i0 < K; i0 += 64) {
    const int i = i0 + lane;
    const bool mine = i < K;
    SiteRecord r;
    r.x = r.y = r.z = NAN, r.flags = 0u;
    if (mine) {
      r = overlay_site(ws.site[gbase + i], a.sites + (rbase + i) * 3);
      const int tok = a.tokens[rbase + i];
      if (tok >= 0 && tok < V) r.flags |= kKnown | (static_cast<uint32_t>(tok) << kTokenShift);
      s_site[i] = r;
      s_chain[i] = ws.chain[gbase + i];
      s_ridx[i] = ws.ridx[gbase + i];
    }
    const bool gen = (r.flags & kSiteGenerated) != 0u;
    const bool ag = (r.flags & (kSiteAntigen | kKnown)) == (kSiteAntigen | kKnown);
    const unsigned long long vg = __ballot(gen), va = __ballot(ag);
    if (gen) s_gen[n_gen + __popcll(vg & below)] = static_cast<uint16_t>(i);
    if (ag) s_ag[n_ag + __popcll(va & below)] = static_cast<uint16_t>(i);
    n_gen += __popcll(vg);
    n_ag += __popcll(va);
  }
  __syncthreads();

  // ---- the pairs: a generated residue walks all slots, any other the list of generated residues
  double sum_ag = 0.0, sum_fw = 0.0, sum_in = 0.0;
  unsigned long long count[3][2] = {{0ull, 0ull}, {0ull, 0ull}, {0ull, 0ull}};  // [class][bin / 4]: four 16-bit counters each
  for (int i0 = 0; i0 < K; i0 += 64) {
    const int i = i0 + lane;
    const bool mine = i < K;
    SiteRecord me;
    me.x = me.y = me.z = NAN, me.flags = 0u;
    if (mine) me = s_site[i];
    const int ci = mine ? s_chain[i] : 0;
    const int64_t ri = mine ? s_ridx[i] : 0;
    const int ti = static_cast<int>(me.flags >> kTokenShift);
    const bool known = (me.flags & kKnown) != 0u;
    const bool walks_all = known && (me.flags & kSiteGenerated) != 0u;
    const bool walks_gen = known && (me.flags & (kSitePresent | kSiteGenerated)) == kSitePresent;
    const bool i_antigen = (me.flags & kSiteAntigen) != 0u;
    double r_all = 0.0, r_ag = 0.0, r_fw = 0.0, r_in = 0.0;
    int partners = 0;
    if (__ballot(walks_all) != 0ull) {  // (uniform)
      for (int j = 0; j < K; ++j) {
        const SiteRecord o = s_site[j];
        const int b = bin_of(me, o, a);
        if (walks_all && j != i && b >= 0 && (o.flags & kKnown) != 0u && !too_near(ci, ri, s_chain[j], s_ridx[j], a.min_sep)) {
          const int tj = static_cast<int>(o.flags >> kTokenShift);
          const bool internal = (o.flags & kSiteGenerated) != 0u;
          const bool swap = internal && j < i;  // an internal pair: the lower slot first
          const double term = static_cast<double>(s_table[(b * V + (swap ? tj : ti)) * Vp + (swap ? ti : tj)]);
          const int cls = internal ? kClassInternal : (o.flags & kSiteAntigen) != 0u ? kClassAntigen : kClassFramework;
          const unsigned long long inc = 1ull << ((b & 3) * 16);
          const int hi = b >> 2;
          ++partners;
          r_all += term;
          r_ag += cls == kClassAntigen ? term : 0.0;
          r_fw += cls == kClassFramework ? term : 0.0;
          r_in += cls == kClassInternal ? term : 0.0;
#pragma unroll
          for (int c = 0; c < 3; ++c) {
            count[c][0] += (cls == c && hi == 0) ? inc : 0ull;
            count[c][1] += (cls == c && hi == 1) ? inc : 0ull;
          }
        }
      }
    }
    if (__ballot(walks_gen) != 0ull) {  // (uniform)
      for (int e = 0; e < n_gen; ++e) {
        const int j = s_gen[e];
        const SiteRecord o = s_site[j];
        const int b = bin_of(me, o, a);
        if (walks_gen && b >= 0 && (o.flags & kKnown) != 0u && !too_near(ci, ri, s_chain[j], s_ridx[j], a.min_sep)) {
          const int tj = static_cast<int>(o.flags >> kTokenShift);
          const double term = static_cast<double>(s_table[(b * V + tj) * Vp + ti]);  // the generated residue first
          ++partners;
          r_all += term;
          r_ag += i_antigen ? term : 0.0;
        }
      }
    }
    if (mine && live) {
      if (a.residue_energy != nullptr) a.residue_energy[rbase + i] = static_cast<float>(r_all);
      if (a.residue_antigen_energy != nullptr) a.residue_antigen_energy[rbase + i] = static_cast<float>(r_ag);
      if (a.n_partners != nullptr) a.n_partners[rbase + i] = partners;
    }
    if (walks_all) sum_ag += r_ag, sum_fw += r_fw, sum_in += r_in;
  }

  sum_ag = wave_sum(sum_ag), sum_fw = wave_sum(sum_fw), sum_in = wave_sum(sum_in);
  if (lane == 0 && live) {  // an internal pair is in the sums of both its residues; halving is exact
    if (a.e_antigen != nullptr) a.e_antigen[row] = static_cast<float>(sum_ag);
    if (a.e_framework != nullptr) a.e_framework[row] = static_cast<float>(sum_fw);
    if (a.e_internal != nullptr) a.e_internal[row] = static_cast<float>(0.5 * sum_in);
  }
  if (a.n_pairs != nullptr) {  // (uniform)
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      for (int b = 0; b < a.NB; ++b) {
        const unsigned long long word = (b >> 2) != 0 ? count[c][1] : count[c][0];
        const int total = wave_sum(static_cast<int>((word >> ((b & 3) * 16)) & 0xFFFFull));
        if (lane == 0 && live) a.n_pairs[(row * 3 + c) * a.NB + b] = c == kClassInternal ? total / 2 : total;
      }
    }
  }

  // ---- the substitution scan: the two half waves take the generated residues in turn, lane v of a half holds S_v
  if (a.substitution != nullptr) {  // (uniform)
    float* out = a.substitution + rbase * V;
    if (live) {
      for (int t = lane; t < K * V; t += 64)
        if ((s_site[t / V].flags & kSiteGenerated) == 0u) out[t] = 0.f;
    }
    const int half = lane >> 5, v = lane & 31;
    for (int e0 = 0; e0 < n_gen; e0 += 2) {
      const bool has = e0 + half < n_gen;
      const int i = s_gen[has ? e0 + half : e0];
      const SiteRecord me = s_site[i];
      const int ci = s_chain[i];
      const int64_t ri = s_ridx[i];
      double S = 0.0;
      for (int q = 0; q < n_ag; ++q) {
        const int j = s_ag[q];
        const SiteRecord o = s_site[j];
        const int b = bin_of(me, o, a);
        if (v < V && b >= 0 && !too_near(ci, ri, s_chain[j], s_ridx[j], a.min_sep))
          S += static_cast<double>(s_table[(b * V + v) * Vp + static_cast<int>(o.flags >> kTokenShift)]);
      }
      const bool known = (me.flags & kKnown) != 0u;
      const double at_token = __shfl(S, half * 32 + (known ? static_cast<int>(me.flags >> kTokenShift) : 0), 64);
      const double cur = known ? at_token : 0.0;
      if (has && v < V && live) out[static_cast<int64_t>(i) * V + v] = static_cast<float>(S - cur);
    }
  }
}

}  // namespace
}  // namespace diffab

using namespace diffab;

extern "C" {

int diffab_metrics_pair_energy(const float* sites, const float* context_sites, const int32_t* tokens, const uint8_t* generation_mask,
                               const uint8_t* residue_mask, const uint8_t* antigen_mask, const int32_t* chain, const int32_t* residue_idx,
                               const float* table, const float* bin_edges, int32_t rows, int32_t group_size, int32_t K, int32_t V, int32_t NB,
                               int32_t min_separation, float* e_antigen, float* e_framework, float* e_internal, int32_t* n_pairs,
                               float* residue_energy, float* residue_antigen_energy, int32_t* n_partners, float* substitution,
                               void* workspace, size_t workspace_bytes, void* stream) {
  StreamOrder order_(stream);
  const char* who = "metrics_pair_energy";
  if (!rows_shape_ok(who, rows, group_size, K, kMaxK)) return DIFFAB_ERR_ARG;
  DIFFAB_REQUIRE(V >= 1 && V <= kMaxClasses, DIFFAB_ERR_ARG, "%s: V = %d classes outside [1, %d]", who, V, kMaxClasses);
  DIFFAB_REQUIRE(NB >= 1 && NB <= kMaxBins, DIFFAB_ERR_ARG, "%s: NB = %d bins outside [1, %d]", who, NB, kMaxBins);
  DIFFAB_REQUIRE(min_separation >= 0, DIFFAB_ERR_ARG, "%s: min_separation must be >= 0, got %d", who, min_separation);
  if (rows == 0) return DIFFAB_OK;
  DIFFAB_REQUIRE(sites && context_sites && tokens && generation_mask && table, DIFFAB_ERR_ARG, "%s: null input", who);
  DIFFAB_REQUIRE((chain == nullptr) == (residue_idx == nullptr), DIFFAB_ERR_ARG,
                 "%s: chain and residue_idx go together: both given, or both null (no pair is skipped)", who);
  DIFFAB_REQUIRE(bin_edges != nullptr, DIFFAB_ERR_ARG, "%s: null bin_edges (a host array of NB + 1 = %d edges)", who, NB + 1);
  EnergyArgs a;
  for (int b = 0; b <= kMaxBins; ++b) a.e2[b] = INFINITY;
  for (int b = 0; b <= NB; ++b) {
    const float e = bin_edges[b];
    DIFFAB_REQUIRE(finite_nonnegative(e), DIFFAB_ERR_ARG, "%s: bin_edges[%d] must be finite and >= 0, got %g", who, b, static_cast<double>(e));
    DIFFAB_REQUIRE(b == 0 || e > bin_edges[b - 1], DIFFAB_ERR_ARG, "%s: bin_edges must be strictly ascending, bin_edges[%d] = %g after %g", who, b,
                   static_cast<double>(e), static_cast<double>(bin_edges[b > 0 ? b - 1 : 0]));
    a.e2[b] = e * e;
    DIFFAB_REQUIRE(a.e2[b] < INFINITY && (b == 0 || a.e2[b] > a.e2[b - 1]), DIFFAB_ERR_ARG,
                   "%s: the fp32 squares of bin_edges must be finite and strictly ascending, bin_edges[%d] = %g has the square %g", who, b,
                   static_cast<double>(e), static_cast<double>(a.e2[b]));
  }
  const int32_t G = rows / group_size;
  const EnergyWorkspace ws = carve_energy(workspace, G, K);
  if (const int e = workspace_ok(who, workspace, 256, workspace_bytes, ws.bytes)) return e;
  hipStream_t st = as_stream(stream);
  hipLaunchKernelGGL(energy_pack_kernel, dim3(G), dim3(64), 0, st, context_sites, generation_mask, residue_mask, antigen_mask, chain, residue_idx,
                     K, ws);
  a.sites = sites, a.tokens = tokens, a.table = table;
  a.rows = rows, a.N = group_size, a.K = K, a.V = V, a.Vp = V | 1, a.NB = NB;
  a.min_sep = chain != nullptr ? min_separation : 0;
  a.table_bytes = static_cast<int>(align_up(static_cast<size_t>(NB) * V * a.Vp * sizeof(float), 16));
  a.wave_bytes = static_cast<int>(align_up(static_cast<size_t>(K) * (sizeof(SiteRecord) + 2 * sizeof(int32_t) + 2 * sizeof(uint16_t)), 16));
  a.waves = (kLdsBudget - a.table_bytes) / a.wave_bytes;  // (at least 2: 33 KiB of table and 14 KiB per wave at the limits)
  a.waves = a.waves > kMaxWaves ? kMaxWaves : a.waves;
  a.waves = a.waves > rows ? rows : a.waves;
  a.e_antigen = e_antigen, a.e_framework = e_framework, a.e_internal = e_internal, a.n_pairs = n_pairs;
  a.residue_energy = residue_energy, a.residue_antigen_energy = residue_antigen_energy, a.n_partners = n_partners, a.substitution = substitution;
  const int blocks = (rows + a.waves - 1) / a.waves;
  hipLaunchKernelGGL(energy_row_kernel, dim3(blocks), dim3(64 * a.waves), static_cast<size_t>(a.table_bytes) + static_cast<size_t>(a.waves) * a.wave_bytes,
                     st, a, ws);
  DIFFAB_LAUNCH_CHECK();
  return DIFFAB_OK;
}

}  // extern "C"
