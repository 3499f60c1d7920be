// similarity_kernels.hip - the two superposition-free comparisons of a design with the native of its patch: lDDT per
// residue, per design and per segment, and the recovery of the native residue contacts (Fnat).  The definition is the header comment of
// diffab_metrics_similarity.
//
// Built with -ffp-contract=off (csrc/Makefile): every distance is d = sqrtf(((dx*dx) + dy*dy) + dz*dz) of three rounded subtractions, every
// comparison is made in fp32 on those values, and every accumulator is an integer - so a row's numbers depend on neither the reduction order
// nor the rows around it, and they equal an fp32 numpy restatement exactly.  VALU + LDS only, no atomics; every value reaches memory through
// plain C++ stores.  One launch.
#include "analysis_common.h"

namespace diffab {
namespace {

constexpr int kMaxK = DIFFAB_METRICS_MAX_K;
constexpr int kMaxGroup = DIFFAB_METRICS_MAX_GROUP;
constexpr int kMaxPoints = DIFFAB_METRICS_MAX_POINTS;
constexpr int kMaxSegments = DIFFAB_METRICS_MAX_SEGMENTS;
constexpr int kMaxStaged = DIFFAB_METRICS_SIMILARITY_MAX_POINTS;  // K * P of one patch
constexpr int kWaves = 4;                                         // designs per work-group: one wave each
constexpr int kCounters = 13;
constexpr unsigned kPresent = 1u, kAntigen = 2u, kCounted = 4u;

struct SimilarityOut {
  int32_t* n_pairs;            // (G,K)
  int32_t* n_pairs_interface;  // (G,K), with an antigen_mask
  int32_t* preserved;          // (rows,K,4)
  int32_t* preserved_interface;
  float* lddt_residue;  // (rows,K)
  float* lddt;          // (rows)
  float* lddt_thresholds;  // (rows,4)
  float* ilddt_residue;
  float* ilddt;
  float* lddt_segment;  // (rows,S)
  int32_t* n_native;    // (G)
  int32_t* native_contacts_residue;  // (G,K)
  int32_t* n_design;                 // (rows)
  int32_t* n_kept;
  float* fnat;
  float* fnonnat;
  int32_t* kept_residue;  // (rows,K)
};

// The plane stride of the staged points: odd, so that the staging stores (consecutive lanes = consecutive planes) spread over the banks.
__host__ __device__ inline int plane_stride(int K) { return K | 1; }

size_t similarity_lds_bytes(int K, int P) {
  return static_cast<size_t>(1 + kWaves) * 3 * P * plane_stride(K) * sizeof(float) + static_cast<size_t>(K) * (sizeof(uint16_t) + 1);
}

__device__ inline float ratio(int num, int den) { return den > 0 ? static_cast<float>(num) / static_cast<float>(den) : NAN; }

// One work-group per (patch, kWaves designs), one wave per design.  LDS (dynamic): the native points of the patch and each wave's design row
// as planes [point * 3 + xyz][residue] (stride K | 1), the counted residues of the patch in ascending order (a ballot prefix) and one flag
// byte per residue.  A wave takes the counted residues i in turn; its lanes are the partner residues j = lane, lane + 64, ...: residue i's
// points are LDS broadcasts, residue j's points are conflict-free plane reads, the P x P native and design distances of the residue pair
// stay in the lane - so the contact of a residue pair is decided by one lane - and the thirteen integers of residue i are summed over the
// wave once per i.  d_nat is recomputed by every wave rather than kept as a pair list.  The wave of the patch's first design also writes
// the per-patch integers.  A patch without a counted residue stages nothing.
template <int P>
__global__ void __launch_bounds__(64 * kWaves)
similarity_kernel(const float* __restrict__ points, const float* __restrict__ native_points, const uint8_t* __restrict__ generation_mask,
                  const uint8_t* __restrict__ residue_mask, const uint8_t* __restrict__ antigen_mask, const int64_t* __restrict__ segment_idx,
                  const int32_t* __restrict__ chain, const int32_t* __restrict__ residue_idx, int N, int K, int S, float radius, float cutoff,
                  SimilarityOut o) {
  extern __shared__ __align__(16) unsigned char s_raw[];
  __shared__ int s_n;
  const int Kp = plane_stride(K);
  float* s_nat = reinterpret_cast<float*>(s_raw);
  float* s_rows = s_nat + 3 * P * Kp;
  uint16_t* s_list = reinterpret_cast<uint16_t*>(s_rows + kWaves * 3 * P * Kp);
  uint8_t* s_flag = reinterpret_cast<uint8_t*>(s_list + K);

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int blocks = (N + kWaves - 1) / kWaves;
  const int64_t g = blockIdx.x / blocks;
  const int d = (blockIdx.x % blocks) * kWaves + wave;  // design of this wave
  const uint8_t* gm = generation_mask + g * K;
  const uint8_t* rm = residue_mask ? residue_mask + g * K : nullptr;
  const uint8_t* ag = antigen_mask ? antigen_mask + g * K : nullptr;

  for (int k = tid; k < K; k += 64 * kWaves) {
    const bool present = rm == nullptr || rm[k] != 0;
    s_flag[k] = static_cast<uint8_t>((present ? kPresent : 0u) | ((ag != nullptr && ag[k] != 0) ? kAntigen : 0u) |
                                     ((present && gm[k] != 0) ? kCounted : 0u));
  }
  if (wave == 0) {
    int n = 0;
    for (int k0 = 0; k0 < K; k0 += 64) {
      const int k = k0 + lane;
      const bool in = k < K && gm[k] != 0 && (rm == nullptr || rm[k] != 0);
      const BallotRank r = ballot_rank(in, lane);
      if (in) s_list[n + r.rank] = static_cast<uint16_t>(k);
      n += r.count;
    }
    if (lane == 0) s_n = n;
  }
  __syncthreads();
  const int n = s_n;
  const int64_t row = g * N + d;
  float* s_des = s_rows + wave * 3 * P * Kp;
  if (n > 0) {  // (uniform over the work-group)
    const float* np = native_points + g * K * (3 * P);
    for (int e = tid; e < K * 3 * P; e += 64 * kWaves) {
      const int k = e / (3 * P), c = e - k * (3 * P);
      s_nat[c * Kp + k] = np[e];
    }
    if (d < N) {
      const float* pp = points + row * K * (3 * P);
      for (int e = lane; e < K * 3 * P; e += 64) {
        const int k = e / (3 * P), c = e - k * (3 * P);
        s_des[c * Kp + k] = pp[e];
      }
    }
    __syncthreads();
  }
  if (d >= N) return;
  const bool patch_writer = d == 0;  // the per-patch integers: written by the wave of the patch's first design

  // the residues that are not counted: zero counts, NaN ratios
  for (int k = lane; k < K; k += 64) {
    if (s_flag[k] & kCounted) continue;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      o.preserved[(row * K + k) * 4 + t] = 0;
      if (ag) o.preserved_interface[(row * K + k) * 4 + t] = 0;
    }
    o.lddt_residue[row * K + k] = NAN;
    if (ag) o.ilddt_residue[row * K + k] = NAN;
    o.kept_residue[row * K + k] = 0;
    if (patch_writer) {
      o.n_pairs[g * K + k] = 0;
      if (ag) o.n_pairs_interface[g * K + k] = 0;
      o.native_contacts_residue[g * K + k] = 0;
    }
  }

  const int64_t* sg = segment_idx ? segment_idx + g * K : nullptr;
  const int32_t* ch = chain ? chain + g * K : nullptr;
  const int32_t* ri = chain ? residue_idx + g * K : nullptr;
  // row totals (the same on every lane); the sums of segment s live on lane s
  int row_pairs = 0, row_ipairs = 0, row_native = 0, row_design = 0, row_kept = 0, seg_num = 0, seg_den = 0;
  int row_pres[4] = {0, 0, 0, 0}, row_ipres[4] = {0, 0, 0, 0};

  for (int c = 0; c < n; ++c) {
    const int i = s_list[c];
    float ni[P][3], di[P][3];
#pragma unroll
    for (int a = 0; a < P; ++a)
#pragma unroll
      for (int x = 0; x < 3; ++x) {
        ni[a][x] = s_nat[(a * 3 + x) * Kp + i];
        di[a][x] = s_des[(a * 3 + x) * Kp + i];
      }
    const int chain_i = ch ? ch[i] : 0;
    const int64_t ridx_i = ri ? ri[i] : 0;
    // 0: scored pairs, 1..4: preserved, 5: scored interface pairs, 6..9: preserved interface, 10: native contacts, 11: design, 12: kept
    int v[kCounters];
#pragma unroll
    for (int t = 0; t < kCounters; ++t) v[t] = 0;
    for (int j = lane; j < K; j += 64) {
      const unsigned flag = s_flag[j];
      if (!(flag & kPresent) || j == i) continue;
      const bool antigen = (flag & kAntigen) != 0;
      bool partner;  // of the contacts
      if (ag) {
        partner = antigen;
      } else if (ch) {
        const int64_t step = static_cast<int64_t>(ri[j]) - ridx_i;
        partner = !(ch[j] == chain_i && (step == 1 || step == -1));
      } else {
        partner = j - i > 1 || i - j > 1;
      }
      float nj[P][3], dj[P][3];
#pragma unroll
      for (int b = 0; b < P; ++b)
#pragma unroll
        for (int x = 0; x < 3; ++x) {
          nj[b][x] = s_nat[(b * 3 + x) * Kp + j];
          dj[b][x] = s_des[(b * 3 + x) * Kp + j];
        }
      bool near_nat = false, near_des = false;
#pragma unroll
      for (int a = 0; a < P; ++a)
#pragma unroll
        for (int b = 0; b < P; ++b) {
          float dx = ni[a][0] - nj[b][0], dy = ni[a][1] - nj[b][1], dz = ni[a][2] - nj[b][2];
          const float d_nat = sqrtf(((dx * dx) + dy * dy) + dz * dz);
          dx = di[a][0] - dj[b][0], dy = di[a][1] - dj[b][1], dz = di[a][2] - dj[b][2];
          const float d_des = sqrtf(((dx * dx) + dy * dy) + dz * dz);
          near_nat |= d_nat < cutoff;
          near_des |= d_des < cutoff;
          const bool scored = d_nat < radius;
          const float off = fabsf(d_des - d_nat);
          const int p0 = (scored && off < 0.5f) ? 1 : 0, p1 = (scored && off < 1.0f) ? 1 : 0;
          const int p2 = (scored && off < 2.0f) ? 1 : 0, p3 = (scored && off < 4.0f) ? 1 : 0;
          const int sc = scored ? 1 : 0, in = antigen ? 1 : 0;
          v[0] += sc, v[1] += p0, v[2] += p1, v[3] += p2, v[4] += p3;
          v[5] += sc & in, v[6] += p0 & in, v[7] += p1 & in, v[8] += p2 & in, v[9] += p3 & in;
        }
      if (partner) {
        v[10] += near_nat ? 1 : 0;
        v[11] += near_des ? 1 : 0;
        v[12] += (near_nat && near_des) ? 1 : 0;
      }
    }
    wave_sum(v);

    const int sum = (v[1] + v[2]) + (v[3] + v[4]), isum = (v[6] + v[7]) + (v[8] + v[9]);
    if (lane < 4) {
      o.preserved[(row * K + i) * 4 + lane] = lane == 0 ? v[1] : lane == 1 ? v[2] : lane == 2 ? v[3] : v[4];
      if (ag) o.preserved_interface[(row * K + i) * 4 + lane] = lane == 0 ? v[6] : lane == 1 ? v[7] : lane == 2 ? v[8] : v[9];
    }
    if (lane == 0) {
      o.lddt_residue[row * K + i] = ratio(sum, 4 * v[0]);
      if (ag) o.ilddt_residue[row * K + i] = ratio(isum, 4 * v[5]);
      o.kept_residue[row * K + i] = v[12];
      if (patch_writer) {
        o.n_pairs[g * K + i] = v[0];
        if (ag) o.n_pairs_interface[g * K + i] = v[5];
        o.native_contacts_residue[g * K + i] = v[10];
      }
    }
    row_pairs += v[0], row_ipairs += v[5], row_native += v[10], row_design += v[11], row_kept += v[12];
#pragma unroll
    for (int t = 0; t < 4; ++t) row_pres[t] += v[1 + t], row_ipres[t] += v[6 + t];
    if (sg) {
      const int64_t label = sg[i];
      if (label >= 0 && label < S && lane == static_cast<int>(label)) seg_num += sum, seg_den += v[0];
    }
  }

  if (lane < 4) {
    o.lddt_thresholds[row * 4 + lane] = ratio(lane == 0 ? row_pres[0] : lane == 1 ? row_pres[1] : lane == 2 ? row_pres[2] : row_pres[3], row_pairs);
  }
  if (sg && lane < S) o.lddt_segment[row * S + lane] = ratio(seg_num, 4 * seg_den);
  if (lane == 0) {
    o.lddt[row] = ratio((row_pres[0] + row_pres[1]) + (row_pres[2] + row_pres[3]), 4 * row_pairs);
    if (ag) o.ilddt[row] = ratio((row_ipres[0] + row_ipres[1]) + (row_ipres[2] + row_ipres[3]), 4 * row_ipairs);
    o.n_design[row] = row_design;
    o.n_kept[row] = row_kept;
    o.fnat[row] = ratio(row_kept, row_native);
    o.fnonnat[row] = ratio(row_design - row_kept, row_design);
    if (patch_writer) o.n_native[g] = row_native;
  }
}

using SimilarityKernel = decltype(&similarity_kernel<1>);
constexpr SimilarityKernel kKernels[kMaxPoints] = {similarity_kernel<1>, similarity_kernel<2>, similarity_kernel<3>, similarity_kernel<4>,
                                                   similarity_kernel<5>};

}  // namespace
}  // namespace diffab

using namespace diffab;

extern "C" {

int diffab_metrics_similarity(const float* points, const float* native_points, const uint8_t* generation_mask, const uint8_t* residue_mask,
                              const uint8_t* antigen_mask, const int64_t* segment_idx, const int32_t* chain, const int32_t* residue_idx,
                              int32_t rows, int32_t group_size, int32_t K, int32_t P, int32_t S, float inclusion_radius, float contact_distance,
                              int32_t* n_pairs, int32_t* n_pairs_interface, int32_t* preserved, int32_t* preserved_interface,
                              float* lddt_residue, float* lddt, float* lddt_thresholds, float* ilddt_residue, float* ilddt, float* lddt_segment,
                              int32_t* n_native, int32_t* native_contacts_residue, int32_t* n_design, int32_t* n_kept, float* fnat,
                              float* fnonnat, int32_t* kept_residue, void* stream) {
  StreamOrder order_(stream);
  static_assert(kMaxPoints == 5, "kKernels holds P = 1..5");
  static_assert(kMaxSegments <= 64, "the sums of segment s live on lane s");
  const int N = group_size;
  DIFFAB_REQUIRE(rows >= 0 && N >= 1 && K >= 1, DIFFAB_ERR_ARG, "metrics_similarity: negative or empty extent (%d rows, group size %d, K = %d)",
                 rows, N, K);
  DIFFAB_REQUIRE(P >= 1 && P <= kMaxPoints, DIFFAB_ERR_ARG, "metrics_similarity: P = %d points per residue outside [1, %d]", P, kMaxPoints);
  DIFFAB_REQUIRE(N <= kMaxGroup, DIFFAB_ERR_ARG, "metrics_similarity: group size N = %d, at most %d designs per group", N, kMaxGroup);
  DIFFAB_REQUIRE(K <= kMaxK, DIFFAB_ERR_ARG, "metrics_similarity: K = %d residues per patch, at most %d", K, kMaxK);
  DIFFAB_REQUIRE(static_cast<int64_t>(K) * P <= kMaxStaged, DIFFAB_ERR_ARG,
                 "metrics_similarity: K * P = %d * %d points per patch, at most %d are staged on chip", K, P, kMaxStaged);
  DIFFAB_REQUIRE(rows % N == 0, DIFFAB_ERR_ARG, "metrics_similarity: %d rows are not a multiple of group_size = %d", rows, N);
  DIFFAB_REQUIRE(S >= 0 && S <= kMaxSegments, DIFFAB_ERR_ARG, "metrics_similarity: S = %d segments outside [0, %d]", S, kMaxSegments);
  DIFFAB_REQUIRE((S > 0) == (segment_idx != nullptr), DIFFAB_ERR_ARG, "metrics_similarity: S = %d %s segment_idx", S,
                 S > 0 ? "needs a" : "goes with a NULL");
  DIFFAB_REQUIRE(inclusion_radius > 0.f && inclusion_radius < INFINITY, DIFFAB_ERR_ARG,
                 "metrics_similarity: the inclusion radius must be finite and > 0, got %g", static_cast<double>(inclusion_radius));
  DIFFAB_REQUIRE(contact_distance > 0.f && contact_distance < INFINITY, DIFFAB_ERR_ARG,
                 "metrics_similarity: the contact distance must be finite and > 0, got %g", static_cast<double>(contact_distance));
  DIFFAB_REQUIRE((chain != nullptr) == (residue_idx != nullptr), DIFFAB_ERR_ARG, "metrics_similarity: chain and residue_idx go together");
  if (rows == 0) return DIFFAB_OK;
  DIFFAB_REQUIRE(points && native_points && generation_mask, DIFFAB_ERR_ARG, "metrics_similarity: null input");
  DIFFAB_REQUIRE(n_pairs && preserved && lddt_residue && lddt && lddt_thresholds, DIFFAB_ERR_ARG, "metrics_similarity: null lDDT output");
  DIFFAB_REQUIRE(n_native && native_contacts_residue && n_design && n_kept && fnat && fnonnat && kept_residue, DIFFAB_ERR_ARG,
                 "metrics_similarity: null contact output");
  DIFFAB_REQUIRE(antigen_mask == nullptr || (n_pairs_interface && preserved_interface && ilddt_residue && ilddt), DIFFAB_ERR_ARG,
                 "metrics_similarity: null interface output with an antigen_mask");
  DIFFAB_REQUIRE(S == 0 || lddt_segment, DIFFAB_ERR_ARG, "metrics_similarity: null segment output");
  const size_t lds = similarity_lds_bytes(K, P);
  DIFFAB_REQUIRE(lds <= 65536, DIFFAB_ERR_UNSUPPORTED, "metrics_similarity: %zu bytes of LDS for K = %d, P = %d", lds, K, P);
  const SimilarityOut o{n_pairs, n_pairs_interface, preserved, preserved_interface, lddt_residue, lddt, lddt_thresholds, ilddt_residue, ilddt,
                        lddt_segment, n_native, native_contacts_residue, n_design, n_kept, fnat, fnonnat, kept_residue};
  const int64_t grid = static_cast<int64_t>(rows / N) * ((N + kWaves - 1) / kWaves);  // at most rows work-groups
  hipStream_t st = as_stream(stream);
  hipLaunchKernelGGL(kKernels[P - 1], dim3(static_cast<unsigned>(grid)), dim3(64 * kWaves), lds, st, points, native_points, generation_mask,
                     residue_mask, antigen_mask, segment_idx, chain, residue_idx, N, K, S, inclusion_radius, contact_distance, o);
  DIFFAB_LAUNCH_CHECK();
  return DIFFAB_OK;
}

}  // extern "C"
