// geometry_kernels.hip - design filters on the device: backbone dihedrals and peptide bonds of every design row
// (diffab_metrics_backbone) and atom clashes / antigen contacts of the generated residues against the rest of the patch
// (diffab_metrics_contacts).  The definitions are the header comments of the two entries.
//
// Built with -ffp-contract=off (csrc/Makefile): the squared distance is dist2 of analysis_common.h and every count is a
// comparison on it, so the integer outputs are defined numbers.  The dihedrals and bond lengths are fp64 from the fp32 points, rounded once.
// VALU + LDS only; the only atomics are integer adds on LDS; every value reaches memory through plain C++ stores.
#include <climits>

#include "analysis_prep.h"

namespace diffab {
namespace {

constexpr int kMaxK = DIFFAB_METRICS_MAX_K;
constexpr int kMaxPoints = DIFFAB_METRICS_MAX_POINTS;
constexpr int kMaxContextAtoms = DIFFAB_METRICS_MAX_CONTEXT_ATOMS;
constexpr int kChunkAtoms = DIFFAB_METRICS_CONTACTS_CHUNK_ATOMS;
constexpr int kChunkResidues = DIFFAB_METRICS_CONTACTS_CHUNK_RESIDUES;
constexpr double kPeptideBond = 1.329;
constexpr double kPi = 3.14159265358979323846;
static_assert(kChunkResidues == 64, "a wave finds the extent of a chunk: one lane per residue");
static_assert(kChunkAtoms >= kMaxContextAtoms, "a chunk holds at least one whole residue");

// ------------------------------------------------------------------ 1. backbone dihedrals and peptide bonds
__device__ inline void load3(const float* p, double (&v)[3]) {
  v[0] = static_cast<double>(p[0]), v[1] = static_cast<double>(p[1]), v[2] = static_cast<double>(p[2]);
}

// IUPAC dihedral of p0-p1-p2-p3 in (-pi, pi]: atan2(|b2| b1.(b2 x b3), (b1 x b2).(b2 x b3)).
__device__ inline double dihedral(const double (&p0)[3], const double (&p1)[3], const double (&p2)[3], const double (&p3)[3]) {
  double b1[3], b2[3], b3[3];
#pragma unroll
  for (int x = 0; x < 3; ++x) b1[x] = p1[x] - p0[x], b2[x] = p2[x] - p1[x], b3[x] = p3[x] - p2[x];
  const double n1[3] = {b1[1] * b2[2] - b1[2] * b2[1], b1[2] * b2[0] - b1[0] * b2[2], b1[0] * b2[1] - b1[1] * b2[0]};
  const double n2[3] = {b2[1] * b3[2] - b2[2] * b3[1], b2[2] * b3[0] - b2[0] * b3[2], b2[0] * b3[1] - b2[1] * b3[0]};
  const double len = sqrt(b2[0] * b2[0] + b2[1] * b2[1] + b2[2] * b2[2]);
  const double y = len * (b1[0] * n2[0] + b1[1] * n2[1] + b1[2] * n2[2]);
  const double x = n1[0] * n2[0] + n1[1] * n2[1] + n1[2] * n2[2];
  const double a = atan2(y, x);
  return a <= -kPi ? kPi : a;
}

// One wave per design row; points (rows, K, 3, 3) = N, CA, C of every residue.
__global__ void __launch_bounds__(64)
metrics_backbone_kernel(const float* __restrict__ points, const uint8_t* __restrict__ generation_mask, const int32_t* __restrict__ succ,
                        const int32_t* __restrict__ pred, int group_size, int K, float bond_tolerance, float* __restrict__ phi,
                        float* __restrict__ psi, float* __restrict__ omega, float* __restrict__ peptide_bond, int32_t* __restrict__ n_bonds,
                        float* __restrict__ max_deviation, int32_t* __restrict__ n_chain_break, int32_t* __restrict__ n_cis) {
  const int lane = threadIdx.x;
  const int64_t row = blockIdx.x;
  const int64_t g = row / group_size;
  const float* pp = points + row * K * 9;
  const uint8_t* gm = generation_mask + g * K;
  int bonds = 0, breaks = 0, cis = 0;
  double worst = 0.0;
  for (int k = lane; k < K; k += 64) {
    const int s = succ[g * K + k], p = pred[g * K + k];
    float o_phi = NAN, o_psi = NAN, o_omega = NAN, o_bond = NAN;
    double n[3], ca[3], c[3];
    load3(pp + k * 9, n);
    load3(pp + k * 9 + 3, ca);
    load3(pp + k * 9 + 6, c);
    if (p >= 0) {
      double cp[3];
      load3(pp + p * 9 + 6, cp);
      o_phi = static_cast<float>(dihedral(cp, n, ca, c));
    }
    if (s >= 0) {
      double ns[3], cas[3];
      load3(pp + s * 9, ns);
      load3(pp + s * 9 + 3, cas);
      const double w = dihedral(ca, c, ns, cas);
      const double dx = c[0] - ns[0], dy = c[1] - ns[1], dz = c[2] - ns[2];
      const double d = sqrt(dx * dx + dy * dy + dz * dz);
      o_psi = static_cast<float>(dihedral(n, ca, c, ns));
      o_omega = static_cast<float>(w);
      o_bond = static_cast<float>(d);
      if (gm[k] != 0 || gm[s] != 0) {
        const double dev = fabs(d - kPeptideBond);
        ++bonds;
        worst = fmax(worst, dev);
        if (dev > static_cast<double>(bond_tolerance)) ++breaks;
        if (fabs(w) < 0.5 * kPi) ++cis;
      }
    }
    phi[row * K + k] = o_phi;
    psi[row * K + k] = o_psi;
    omega[row * K + k] = o_omega;
    peptide_bond[row * K + k] = o_bond;
  }
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) {  // integer sums and a maximum: the order does not matter
    bonds += __shfl_xor(bonds, d, 64);
    breaks += __shfl_xor(breaks, d, 64);
    cis += __shfl_xor(cis, d, 64);
    worst = fmax(worst, __shfl_xor(worst, d, 64));
  }
  if (lane == 0) {
    n_bonds[row] = bonds;
    max_deviation[row] = static_cast<float>(worst);
    n_chain_break[row] = breaks;
    n_cis[row] = cis;
  }
}

// ------------------------------------------------------------------ 2. clashes and contacts
// The workspace of diffab_metrics_contacts is the ContextWorkspace of analysis_prep.h (DIFFAB_METRICS_CONTACTS_WORKSPACE_BYTES covers
// its carves and their alignment), filled by context_pack_kernel<false, kMaxK>: every context residue is listed.
//
// One work-group per (patch, 64 designs): lane = design, the four waves share the staged context and split the generated residues.
// The context residues of the patch go through LDS in chunks of whole residues (at most kChunkResidues residues and kChunkAtoms atoms);
// every lane reads the same context atom (an LDS broadcast) against the atoms of its own design, held in registers.  A generated
// residue's counts are owned by one thread (its wave, the design's lane) and live in registers; a context residue's counts are collected
// from the four waves by integer adds on LDS and stored by one thread when its chunk is done.
template <int P>
__global__ void __launch_bounds__(256)
metrics_contacts_kernel(const float* __restrict__ points, const uint8_t* __restrict__ valid, const int32_t* __restrict__ chain,
                        const int32_t* __restrict__ residue_idx, int N, int K, int A, float clash, float clash2, float contact2, int with_antigen,
                        ContextWorkspace ws, int32_t* __restrict__ n_clash, float* __restrict__ clash_score, float* __restrict__ min_distance,
                        int32_t* __restrict__ n_contact_pairs, int32_t* __restrict__ n_paratope, int32_t* __restrict__ n_epitope,
                        int32_t* __restrict__ n_hotspot_contacted, int32_t* __restrict__ n_hotspot, int32_t* __restrict__ residue_clash,
                        int32_t* __restrict__ residue_contact) {
  __shared__ float4 s_atom[kChunkAtoms];
  __shared__ int4 s_res[kChunkResidues];  // slot, first atom in s_atom, atoms, flags
  __shared__ int2 s_key[kChunkResidues];
  __shared__ int s_clash[kChunkResidues][64];
  __shared__ int s_contact[kChunkResidues][64];
  __shared__ int s_int[5][4][64];
  __shared__ double s_score[4][64];
  __shared__ float s_min[4][64];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int blocks = (N + 63) / 64;
  const int64_t g = blockIdx.x / blocks;
  const int d = (blockIdx.x % blocks) * 64 + lane;
  const bool active = d < N;
  const int64_t row = g * N + (active ? d : N - 1);  // (an idle lane reads the last design and counts nothing)
  const int4 hdr = ws.hdr[g];
  const int ng = hdr.x, nr = hdr.y;
  const int32_t* gen = ws.gen + g * K;
  const int4* res = ws.res + g * K;
  const int2* key = ws.key + g * K;
  const float4* atoms = ws.atoms + g * K * A;
  const float* pp = points + row * K * P * 3;
  const uint8_t* vv = valid + row * K;
  const int32_t* ch = chain + g * K;
  const int32_t* ri = residue_idx + g * K;

  for (int e = tid; e < kChunkResidues * 64; e += 256) {
    (&s_clash[0][0])[e] = 0;
    (&s_contact[0][0])[e] = 0;
  }
  int clashes = 0, pairs = 0, paratope = 0, epitope = 0, hot = 0;
  double score = 0.0;
  float least = INFINITY;

  // the atoms of generated residue i of this lane's design
  float px[P], py[P], pz[P];
  uint32_t pv = 0;
  auto load_own = [&](int i) {
#pragma unroll
    for (int a = 0; a < P; ++a) px[a] = pp[(i * P + a) * 3], py[a] = pp[(i * P + a) * 3 + 1], pz[a] = pp[(i * P + a) * 3 + 2];
    pv = active ? vv[i] : 0u;
  };
  // one other atom q against them: its clashes (and their score, when counted), whether it is within the contact distance
  auto against = [&](float qx, float qy, float qz, bool q_valid, bool counted, int& c, bool& near) {
#pragma unroll
    for (int a = 0; a < P; ++a) {
      const float d2 = masked_dist2(px[a], py[a], pz[a], qx, qy, qz, q_valid && ((pv >> a) & 1u) != 0u);
      least = fminf(least, d2);
      near |= d2 < contact2;
      if (d2 < clash2) {
        ++c;
        if (counted) {
          const double t = static_cast<double>(clash) - static_cast<double>(sqrtf(d2));
          score += t * t;
        }
      }
    }
  };

  // ---- generated residues against the context, chunk by chunk
  for (int r0 = 0; r0 < nr;) {
    // the extent of the chunk, found by every wave alike: one lane per residue
    const int e = r0 + lane;
    const int4 mine = e < nr ? res[e] : make_int4(0, 0, 0, 0);
    const int first = __shfl(mine.y, 0, 64);
    const bool fits = e < nr && mine.y + mine.z - first <= kChunkAtoms;  // (monotone; lane 0 always fits: a residue has at most 32 atoms)
    const int nres = __popcll(__ballot(fits));
    const int natoms = __shfl(mine.y + mine.z, nres - 1, 64) - first;
    __syncthreads();  // the chunk before is flushed
    for (int t = tid; t < natoms; t += 256) s_atom[t] = atoms[first + t];
    if (tid < nres) {
      const int4 r = res[r0 + tid];
      s_res[tid] = make_int4(r.x, r.y - first, r.z, r.w);
      s_key[tid] = key[r0 + tid];
    }
    __syncthreads();
    for (int gi = wave; gi < ng; gi += 4) {
      const int i = gen[gi];
      load_own(i);
      const int ci = ch[i], rri = ri[i];
      int own_clash = 0, own_contact = 0;
      for (int rl = 0; rl < nres; ++rl) {
        const int4 r = s_res[rl];
        const int2 kk = s_key[rl];
        if (bonded(ci, rri, kk.x, kk.y)) continue;
        int c = 0;
        bool near = false;
        for (int b = r.y; b < r.y + r.z; ++b) {
          const float4 q = s_atom[b];
          against(q.x, q.y, q.z, true, true, c, near);
        }
        if (c != 0) {
          clashes += c;
          own_clash += c;
          atomicAdd(&s_clash[rl][lane], c);
        }
        if (with_antigen && (r.w & kFlagAntigen) != 0 && near) {
          ++pairs;
          ++own_contact;
          atomicAdd(&s_contact[rl][lane], 1);
        }
      }
      if (active && own_clash != 0) residue_clash[row * K + i] += own_clash;  // (this thread alone writes entry (row, i))
      if (active && own_contact != 0) {
        const int before = residue_contact[row * K + i];
        if (before == 0) ++paratope;
        residue_contact[row * K + i] = before + own_contact;
      }
    }
    __syncthreads();
    for (int rl = wave; rl < nres; rl += 4) {  // a context residue is in one chunk: its counts are complete
      const int4 r = s_res[rl];
      const int c = s_clash[rl][lane], t = s_contact[rl][lane];
      if (c != 0) {
        if (active) residue_clash[row * K + r.x] = c;
        s_clash[rl][lane] = 0;
      }
      if (t != 0) {
        if (active) residue_contact[row * K + r.x] = t;
        ++epitope;
        if ((r.w & kFlagHotspot) != 0) ++hot;
        s_contact[rl][lane] = 0;
      }
    }
    r0 += nres;
  }

  // ---- generated residues against each other, inside the design: residue i takes its counts from every other one, the row counts the
  // unordered pair once (the squared distance is the same number from both sides)
  for (int gi = wave; gi < ng; gi += 4) {
    const int i = gen[gi];
    load_own(i);
    const int ci = ch[i], rri = ri[i];
    int own_clash = 0;
    for (int gj = 0; gj < ng; ++gj) {
      const int j = gen[gj];
      if (gj == gi || bonded(ci, rri, ch[j], ri[j])) continue;
      const uint32_t qv = active ? vv[j] : 0u;
      int c = 0;
      bool near = false;
#pragma unroll
      for (int b = 0; b < P; ++b)
        against(pp[(j * P + b) * 3], pp[(j * P + b) * 3 + 1], pp[(j * P + b) * 3 + 2], ((qv >> b) & 1u) != 0u, gi < gj, c, near);
      own_clash += c;
      if (gi < gj) clashes += c;
    }
    if (active && own_clash != 0) residue_clash[row * K + i] += own_clash;
  }

  // ---- the row: the four waves' parts, in wave order
  s_int[0][wave][lane] = clashes, s_int[1][wave][lane] = pairs, s_int[2][wave][lane] = paratope, s_int[3][wave][lane] = epitope;
  s_int[4][wave][lane] = hot;
  s_score[wave][lane] = score;
  s_min[wave][lane] = least;
  __syncthreads();
  if (wave != 0 || !active) return;
  int sum[5] = {0, 0, 0, 0, 0};
  double total = 0.0;
  float lowest = INFINITY;
  for (int w = 0; w < 4; ++w) {
#pragma unroll
    for (int v = 0; v < 5; ++v) sum[v] += s_int[v][w][lane];
    total += s_score[w][lane];
    lowest = fminf(lowest, s_min[w][lane]);
  }
  n_clash[row] = sum[0];
  clash_score[row] = static_cast<float>(total);
  min_distance[row] = sqrtf(lowest);
  if (with_antigen) {
    n_contact_pairs[row] = sum[1];
    n_paratope[row] = sum[2];
    n_epitope[row] = sum[3];
  }
  if (n_hotspot != nullptr) {
    n_hotspot_contacted[row] = sum[4];
    n_hotspot[row] = hdr.w;
  }
}

}  // namespace
}  // namespace diffab

using namespace diffab;

extern "C" {

int diffab_metrics_backbone(const float* points, const uint8_t* generation_mask, const uint8_t* residue_mask, const int32_t* chain,
                            const int32_t* residue_idx, int32_t rows, int32_t group_size, int32_t K, float bond_tolerance, float* phi,
                            float* psi, float* omega, float* peptide_bond, int32_t* n_bonds, float* max_peptide_deviation,
                            int32_t* n_chain_break, int32_t* n_cis, void* workspace, size_t workspace_bytes, void* stream) {
  StreamOrder order_(stream);
  if (!rows_shape_ok("metrics_backbone", rows, group_size, K, kMaxK)) return DIFFAB_ERR_ARG;
  DIFFAB_REQUIRE(finite_nonnegative(bond_tolerance), DIFFAB_ERR_ARG,
                 "metrics_backbone: bond_tolerance must be finite and >= 0, got %g", static_cast<double>(bond_tolerance));
  if (rows == 0) return DIFFAB_OK;
  DIFFAB_REQUIRE(points && generation_mask && chain && residue_idx, DIFFAB_ERR_ARG, "metrics_backbone: null input");
  DIFFAB_REQUIRE(phi && psi && omega && peptide_bond && n_bonds && max_peptide_deviation && n_chain_break && n_cis, DIFFAB_ERR_ARG,
                 "metrics_backbone: null output");
  const int32_t G = rows / group_size;
  const LinkWorkspace ws = carve_links(workspace, G, K);
  if (const int e = workspace_ok("metrics_backbone", workspace, 16, workspace_bytes, ws.bytes)) return e;
  hipStream_t st = as_stream(stream);
  hipLaunchKernelGGL((chain_links_kernel<256, kMaxK>), dim3(G), dim3(256), 0, st, chain, residue_idx, residue_mask, K, ws.succ, ws.pred);
  hipLaunchKernelGGL(metrics_backbone_kernel, dim3(rows), dim3(64), 0, st, points, generation_mask, ws.succ, ws.pred, group_size, K,
                     bond_tolerance, phi, psi, omega, peptide_bond, n_bonds, max_peptide_deviation, n_chain_break, n_cis);
  DIFFAB_LAUNCH_CHECK();
  return DIFFAB_OK;
}

int diffab_metrics_contacts(const float* points, const uint8_t* valid, const float* context_points, const uint32_t* context_valid,
                            const uint8_t* generation_mask, const uint8_t* residue_mask, const uint8_t* antigen_mask,
                            const uint8_t* hotspot_mask, const int32_t* chain, const int32_t* residue_idx, int32_t rows, int32_t group_size,
                            int32_t K, int32_t P, int32_t A, float clash_distance, float contact_distance, int32_t* n_clash,
                            float* clash_score, float* min_distance, int32_t* n_contact_pairs, int32_t* n_paratope, int32_t* n_epitope,
                            int32_t* n_hotspot_contacted, int32_t* n_hotspot, int32_t* residue_clash, int32_t* residue_contact,
                            void* workspace, size_t workspace_bytes, void* stream) {
  StreamOrder order_(stream);
  if (!rows_shape_ok("metrics_contacts", rows, group_size, K, kMaxK)) return DIFFAB_ERR_ARG;
  DIFFAB_REQUIRE(P >= 1 && P <= kMaxPoints, DIFFAB_ERR_ARG, "metrics_contacts: P = %d points per residue outside [1, %d]", P, kMaxPoints);
  DIFFAB_REQUIRE(A >= 1 && A <= kMaxContextAtoms, DIFFAB_ERR_ARG, "metrics_contacts: A = %d context atoms per residue outside [1, %d]", A,
                 kMaxContextAtoms);
  DIFFAB_REQUIRE(finite_nonnegative(clash_distance), DIFFAB_ERR_ARG,
                 "metrics_contacts: clash_distance must be finite and >= 0, got %g", static_cast<double>(clash_distance));
  DIFFAB_REQUIRE(finite_nonnegative(contact_distance), DIFFAB_ERR_ARG,
                 "metrics_contacts: contact_distance must be finite and >= 0, got %g", static_cast<double>(contact_distance));
  DIFFAB_REQUIRE(hotspot_mask == nullptr || antigen_mask != nullptr, DIFFAB_ERR_ARG, "metrics_contacts: a hotspot_mask needs an antigen_mask");
  if (rows == 0) return DIFFAB_OK;
  DIFFAB_REQUIRE(points && valid && context_points && context_valid && generation_mask && chain && residue_idx, DIFFAB_ERR_ARG,
                 "metrics_contacts: null input");
  DIFFAB_REQUIRE(n_clash && clash_score && min_distance && residue_clash, DIFFAB_ERR_ARG, "metrics_contacts: null output");
  DIFFAB_REQUIRE(antigen_mask == nullptr || (n_contact_pairs && n_paratope && n_epitope && residue_contact), DIFFAB_ERR_ARG,
                 "metrics_contacts: null contact output with an antigen_mask");
  DIFFAB_REQUIRE(hotspot_mask == nullptr || (n_hotspot_contacted && n_hotspot), DIFFAB_ERR_ARG,
                 "metrics_contacts: null hotspot output with a hotspot_mask");
  const int32_t G = rows / group_size;
  Carver carver(workspace);
  const ContextWorkspace ws = carve_context(carver, G, K, A);
  if (const int e = workspace_ok("metrics_contacts", workspace, 16, workspace_bytes, carver.bytes())) return e;
  const int64_t grid = static_cast<int64_t>(G) * ((group_size + 63) / 64);
  DIFFAB_REQUIRE(grid <= INT_MAX, DIFFAB_ERR_UNSUPPORTED, "metrics_contacts: %d rows are more work-groups than one launch holds", rows);
  hipStream_t st = as_stream(stream);
  const size_t per_residue = static_cast<size_t>(rows) * static_cast<size_t>(K) * sizeof(int32_t);
  DIFFAB_HIP_CHECK(hipMemsetAsync(residue_clash, 0, per_residue, st));
  const int with_antigen = antigen_mask != nullptr;
  if (with_antigen) DIFFAB_HIP_CHECK(hipMemsetAsync(residue_contact, 0, per_residue, st));
  hipLaunchKernelGGL((context_pack_kernel<false, kMaxK>), dim3(G), dim3(256), 0, st, context_points, context_valid, generation_mask,
                     residue_mask, antigen_mask, hotspot_mask, chain, residue_idx, K, A, ws, static_cast<int32_t*>(nullptr));
  const float clash2 = clash_distance * clash_distance, contact2 = contact_distance * contact_distance;
  int32_t* hot_out = hotspot_mask != nullptr ? n_hotspot : nullptr;
#define DIFFAB_CONTACTS_LAUNCH(PP)                                                                                                       \
  hipLaunchKernelGGL((metrics_contacts_kernel<PP>), dim3(static_cast<unsigned>(grid)), dim3(256), 0, st, points, valid, chain, residue_idx, \
                     group_size, K, A, clash_distance, clash2, contact2, with_antigen, ws, n_clash, clash_score, min_distance,          \
                     n_contact_pairs, n_paratope, n_epitope, n_hotspot_contacted, hot_out, residue_clash, residue_contact)
  switch (P) {
    case 1: DIFFAB_CONTACTS_LAUNCH(1); break;
    case 2: DIFFAB_CONTACTS_LAUNCH(2); break;
    case 3: DIFFAB_CONTACTS_LAUNCH(3); break;
    case 4: DIFFAB_CONTACTS_LAUNCH(4); break;
    default: DIFFAB_CONTACTS_LAUNCH(5); break;
  }
#undef DIFFAB_CONTACTS_LAUNCH
  DIFFAB_LAUNCH_CHECK();
  return DIFFAB_OK;
}

}  // extern "C"
