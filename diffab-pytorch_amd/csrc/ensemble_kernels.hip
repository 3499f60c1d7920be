// ensemble_kernels.hip - the N designs of a patch as a distribution: per-position amino-acid frequencies, entropy and
// consensus, the weighted mean structure and per-residue RMSF, how typical each design is of its siblings (mean log-frequency of its own
// tokens, identity to the consensus, RMSD to the mean), the effective number of designs and the central design.  The definition is the
// header comment of diffab_metrics_ensemble.
//
// Built with -ffp-contract=off (csrc/Makefile): every result is a defined number.  Every sum is fp64 from the fp32 / int64 inputs, in a
// fixed order: a wave's rows of a slice in ascending order, the four waves of a work-group in wave order, the slices of N in slice order,
// the 64-residue chunks of K in chunk order, the lanes of a wave through one fixed butterfly.  VALU + LDS only, no atomics; every value
// reaches memory through plain C++ stores.  Four launches: accumulate, finish, deviations, rows.
#include <climits>

#include "analysis_common.h"

namespace diffab {
namespace {

constexpr int kMaxK = DIFFAB_METRICS_MAX_K;
constexpr int kMaxGroup = DIFFAB_METRICS_MAX_GROUP;
constexpr int kMaxPoints = DIFFAB_METRICS_MAX_POINTS;
constexpr int kMaxClasses = DIFFAB_METRICS_MAX_CLASSES;
constexpr int kSlice = 128;  // design rows of a group per work-group of the two streaming kernels (a function of nothing: results do not depend on G)
constexpr int kChunk = 64;   // residues per work-group: lane = residue
constexpr int kWaves = 4;
constexpr int kNone = INT_MAX;

// Workspace of diffab_metrics_ensemble (DIFFAB_METRICS_ENSEMBLE_WORKSPACE_BYTES covers the carves and their alignment).
// S = slices of N, KC = chunks of K; the residue is the fastest axis of every per-residue carve, so a wave's accesses are whole lines.
struct EnsembleWorkspace {
  double* part_c;    // (G, S, V, K): class sums of a slice
  double* part_p;    // (G, S, 3P, K): weighted point sums of a slice
  double* lnf;       // (G, V, K): the class sums, then ln f
  double* mean;      // (G, 3P, K): the mean before rounding
  double* part_dev;  // (G, S, K): sum of w |p - m|^2 of a slice
  double* part_row;  // (G*N, KC, 3): per design and chunk: sum ln f, token matches, sum |p - m|^2 over the counted residues
  double* wsum;      // (G): W
  int32_t* cons;     // (G, K): consensus
  int32_t* cnt;      // (G): counted residues
  size_t bytes;
};

EnsembleWorkspace carve_ensemble(void* base, int64_t G, int64_t N, int64_t K, int64_t P, int64_t V) {
  const int64_t S = (N + kSlice - 1) / kSlice, KC = (K + kChunk - 1) / kChunk;
  Carver c(base);
  EnsembleWorkspace w;
  w.part_c = c.take<double>(static_cast<size_t>(G * S * V * K));
  w.part_p = c.take<double>(static_cast<size_t>(G * S * 3 * P * K));
  w.lnf = c.take<double>(static_cast<size_t>(G * V * K));
  w.mean = c.take<double>(static_cast<size_t>(G * 3 * P * K));
  w.part_dev = c.take<double>(static_cast<size_t>(G * S * K));
  w.part_row = c.take<double>(static_cast<size_t>(G * N * KC * 3));
  w.wsum = c.take<double>(static_cast<size_t>(G));
  w.cons = c.take<int32_t>(static_cast<size_t>(G * K));
  w.cnt = c.take<int32_t>(static_cast<size_t>(G));
  w.bytes = c.bytes();
  return w;
}

// The weight of a design row: 1 without weights; a negative or non-finite weight is 0.
__device__ inline double weight_of(const float* __restrict__ weights, int64_t row) {
  if (weights == nullptr) return 1.0;
  const float w = weights[row];
  return (w > 0.f && w < INFINITY) ? static_cast<double>(w) : 0.0;
}

// The four waves' columns [wave][line][lane] of `lines` lines, added in wave order and stored to out[line * K + k].
__device__ inline void combine_waves(const double* s, int lines, int tid, int k0, int K, double* __restrict__ out) {
  for (int i = tid; i < lines * kChunk; i += kWaves * 64) {
    const int line = i >> 6, l = i & 63;
    double sum = s[line * kChunk + l];
#pragma unroll
    for (int w = 1; w < kWaves; ++w) sum += s[(w * lines + line) * kChunk + l];
    if (k0 + l < K) out[static_cast<int64_t>(line) * K + k0 + l] = sum;
  }
}

// ------------------------------------------------------------------ 1. accumulate
// Grid (G, S, KC), 256 threads: lane = residue, wave w takes rows w, w + 4, ... of the slice.  The class sums of a wave live in LDS as
// [wave][class][lane] doubles - the column of a lane is its own, so plain read-modify-writes - the 3P point sums in registers.  A row of
// weight 0 is not read; a residue outside residue_mask is not read.  Dynamic LDS: 4 * max(V, 3P) * 64 doubles.
template <int P>
__global__ void __launch_bounds__(256)
ensemble_accumulate_kernel(const int64_t* __restrict__ seq, const float* __restrict__ points, const uint8_t* __restrict__ residue_mask,
                           const float* __restrict__ weights, int N, int K, int V, EnsembleWorkspace ws) {
  extern __shared__ __align__(16) double s_cols[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t g = blockIdx.x;
  const int s = blockIdx.y, S = gridDim.y, k0 = blockIdx.z * kChunk, k = k0 + lane;
  const bool inside = k < K && (residue_mask == nullptr || residue_mask[g * K + k] != 0);
  for (int i = tid; i < kWaves * V * kChunk; i += 256) s_cols[i] = 0.0;
  __syncthreads();
  double* col = s_cols + wave * V * kChunk + lane;
  double acc[3 * P];
#pragma unroll
  for (int e = 0; e < 3 * P; ++e) acc[e] = 0.0;
  const int r1 = min(N, (s + 1) * kSlice);
  for (int r = s * kSlice + wave; r < r1; r += kWaves) {
    const int64_t row = g * N + r;
    const double w = weight_of(weights, row);  // (uniform over the wave)
    if (!(w > 0.0) || !inside) continue;
    const int64_t tok = seq[row * K + k];
    const float* p = points + (row * K + k) * (3 * P);
    if (tok >= 0 && tok < V) col[tok * kChunk] += w;
#pragma unroll
    for (int e = 0; e < 3 * P; ++e) acc[e] += w * static_cast<double>(p[e]);
  }
  __syncthreads();
  combine_waves(s_cols, V, tid, k0, K, ws.part_c + ((g * S + s) * V) * K);
  __syncthreads();
#pragma unroll
  for (int e = 0; e < 3 * P; ++e) s_cols[(wave * 3 * P + e) * kChunk + lane] = acc[e];
  __syncthreads();
  combine_waves(s_cols, 3 * P, tid, k0, K, ws.part_p + ((g * S + s) * 3 * P) * K);
}

// ------------------------------------------------------------------ 2. finish the positions
// Grid (G, KC), one wave: lane = residue.  Every work-group of a patch takes W and the sum of w^2 the same way (so they agree to the bit);
// chunk 0 stores them, the number of counted residues and n_eff.
__global__ void __launch_bounds__(64)
ensemble_finish_kernel(const uint8_t* __restrict__ generation_mask, const uint8_t* __restrict__ residue_mask, const float* __restrict__ weights,
                       int N, int K, int P, int V, int S, double alpha, EnsembleWorkspace ws, float* __restrict__ aa_freq,
                       float* __restrict__ entropy, int64_t* __restrict__ consensus, float* __restrict__ mean_points, float* __restrict__ n_eff) {
  const int lane = threadIdx.x;
  const int64_t g = blockIdx.x;
  const int k = blockIdx.y * kChunk + lane;
  double a[2] = {0.0, 0.0};
  for (int r = lane; r < N; r += 64) {
    const double w = weight_of(weights, g * N + r);
    a[0] += w;
    a[1] += w * w;
  }
  wave_sum(a);
  const double W = a[0];
  if (blockIdx.y == 0) {
    int n = 0;
    for (int j0 = 0; j0 < K; j0 += 64) {
      const int j = j0 + lane;
      const bool in = j < K && generation_mask[g * K + j] != 0 && (residue_mask == nullptr || residue_mask[g * K + j] != 0);
      n += __popcll(__ballot(in));
    }
    if (lane == 0) {
      ws.wsum[g] = W;
      ws.cnt[g] = n;
      if (n_eff) n_eff[g] = W > 0.0 ? static_cast<float>(W * W / a[1]) : NAN;
    }
  }
  if (k >= K) return;
  const bool inside = residue_mask == nullptr || residue_mask[g * K + k] != 0;

  // class sums: slices in slice order, classes in ascending order
  double* fcol = ws.lnf + (g * V) * K + k;
  double Wk = 0.0, best = -1.0;
  int cons = -1;
  for (int v = 0; v < V; ++v) {
    double c = 0.0;
    for (int s = 0; s < S; ++s) c += ws.part_c[((g * S + s) * V + v) * K + k];
    fcol[static_cast<int64_t>(v) * K] = c;
    Wk += c;
    if (c > best) {
      best = c;
      cons = v;
    }
  }
  if (!(Wk > 0.0)) cons = -1;
  const double denom = Wk + alpha, share = alpha / static_cast<double>(V);
  double ent = 0.0;
  for (int v = 0; v < V; ++v) {
    const double f = denom > 0.0 ? (fcol[static_cast<int64_t>(v) * K] + share) / denom : NAN;
    const double l = log(f);
    fcol[static_cast<int64_t>(v) * K] = l;
    if (f > 0.0)
      ent += -(f * l);
    else if (f != f)
      ent = NAN;
    if (aa_freq) aa_freq[(g * K + k) * V + v] = inside ? static_cast<float>(f) : NAN;
  }
  if (entropy) entropy[g * K + k] = inside ? static_cast<float>(ent) : NAN;
  if (consensus) consensus[g * K + k] = inside ? cons : -1;
  ws.cons[g * K + k] = cons;

  for (int e = 0; e < 3 * P; ++e) {
    double sum = 0.0;
    for (int s = 0; s < S; ++s) sum += ws.part_p[((g * S + s) * 3 * P + e) * K + k];
    const double m = W > 0.0 ? sum / W : NAN;
    ws.mean[(g * 3 * P + e) * K + k] = m;
    if (mean_points) mean_points[(g * K + k) * 3 * P + e] = inside ? static_cast<float>(m) : NAN;
  }
}

// ------------------------------------------------------------------ 3. deviations from the mean
// The grid of the accumulation.  Per residue the slice's sum of w |p - m|^2 (registers, the waves combined in wave order); per design row
// the chunk's sums over the counted residues of ln f(token), token == consensus and |p - m|^2 (one butterfly per row).
template <int P>
__global__ void __launch_bounds__(256)
ensemble_deviation_kernel(const int64_t* __restrict__ seq, const float* __restrict__ points, const uint8_t* __restrict__ generation_mask,
                          const uint8_t* __restrict__ residue_mask, const float* __restrict__ weights, int N, int K, int V,
                          EnsembleWorkspace ws) {
  __shared__ double s_dev[kWaves * kChunk];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t g = blockIdx.x;
  const int s = blockIdx.y, S = gridDim.y, KC = gridDim.z, kc = blockIdx.z, k0 = kc * kChunk, k = k0 + lane;
  const bool inside = k < K && (residue_mask == nullptr || residue_mask[g * K + k] != 0);
  const bool counted = inside && generation_mask[g * K + k] != 0;
  double m[3 * P];
#pragma unroll
  for (int e = 0; e < 3 * P; ++e) m[e] = inside ? ws.mean[(g * 3 * P + e) * K + k] : 0.0;
  const int cons = counted ? ws.cons[g * K + k] : -1;
  const double* lnf = ws.lnf + (g * V) * K + (k < K ? k : 0);
  double dev = 0.0;
  const int r1 = min(N, (s + 1) * kSlice);
  for (int r = s * kSlice + wave; r < r1; r += kWaves) {
    const int64_t row = g * N + r;
    const double w = weight_of(weights, row);  // (uniform over the wave)
    double t[3] = {0.0, 0.0, 0.0};
    if (inside) {
      const float* p = points + (row * K + k) * (3 * P);
      double d2 = 0.0;
#pragma unroll
      for (int e = 0; e < 3 * P; ++e) {
        const double d = static_cast<double>(p[e]) - m[e];
        d2 += d * d;
      }
      if (w > 0.0) dev += w * d2;
      if (counted) {
        const int64_t tok = seq[row * K + k];
        t[0] = (tok >= 0 && tok < V) ? lnf[tok * K] : -INFINITY;
        t[1] = (cons >= 0 && tok == cons) ? 1.0 : 0.0;
        t[2] = d2;
      }
    }
    wave_sum(t);
    if (lane == 0) {
      double* out = ws.part_row + (row * KC + kc) * 3;
      out[0] = t[0], out[1] = t[1], out[2] = t[2];
    }
  }
  s_dev[wave * kChunk + lane] = dev;
  __syncthreads();
  combine_waves(s_dev, 1, tid, k0, K, ws.part_dev + (g * S + s) * K);
}

// ------------------------------------------------------------------ 4. rows and patches
struct Least {
  float v;
  int i;
};

__device__ inline Least lesser(Least a, Least b) {  // the smaller value; ties to the lower index; kNone loses to anything
  if (b.i == kNone) return a;
  if (a.i == kNone) return b;
  if (b.v < a.v || (b.v == a.v && b.i < a.i)) return b;
  return a;
}

// One work-group per patch: the three numbers of every design (chunks in chunk order), the central design, the RMSF of every residue.
__global__ void __launch_bounds__(256)
ensemble_rows_kernel(const uint8_t* __restrict__ residue_mask, const float* __restrict__ weights, int N, int K, int P, int S, int KC,
                     EnsembleWorkspace ws, float* __restrict__ rmsf, float* __restrict__ log_prob, float* __restrict__ consensus_identity,
                     float* __restrict__ rmsd_to_mean, int64_t* __restrict__ central) {
  __shared__ Least s_part[kWaves];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t g = blockIdx.x;
  const int n = ws.cnt[g];
  const double W = ws.wsum[g];
  Least mine{0.f, kNone};
  for (int r = tid; r < N; r += 256) {
    const int64_t row = g * N + r;
    double t[3] = {0.0, 0.0, 0.0};
    for (int c = 0; c < KC; ++c) {
#pragma unroll
      for (int i = 0; i < 3; ++i) t[i] += ws.part_row[(row * KC + c) * 3 + i];
    }
    float lp = NAN, ci = NAN, rd = NAN;
    if (n > 0) {
      lp = static_cast<float>(t[0] / static_cast<double>(n));
      ci = static_cast<float>(t[1]) / static_cast<float>(n);
      rd = static_cast<float>(sqrt(t[2] / (static_cast<double>(n) * static_cast<double>(P))));
    }
    if (log_prob) log_prob[row] = lp;
    if (consensus_identity) consensus_identity[row] = ci;
    if (rmsd_to_mean) rmsd_to_mean[row] = rd;
    if (weight_of(weights, row) > 0.0 && rd == rd) mine = lesser(mine, Least{rd, r});
  }
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) mine = lesser(mine, Least{__shfl_xor(mine.v, d, 64), __shfl_xor(mine.i, d, 64)});
  if (lane == 0) s_part[wave] = mine;
  __syncthreads();
  if (tid == 0 && central) {
    Least b = s_part[0];
    for (int w = 1; w < kWaves; ++w) b = lesser(b, s_part[w]);
    central[g] = b.i == kNone ? -1 : b.i;
  }
  if (rmsf) {
    for (int k = tid; k < K; k += 256) {
      double sum = 0.0;
      for (int s = 0; s < S; ++s) sum += ws.part_dev[(g * S + s) * K + k];
      const bool inside = residue_mask == nullptr || residue_mask[g * K + k] != 0;
      rmsf[g * K + k] = inside ? static_cast<float>(sqrt(sum / (W * static_cast<double>(P)))) : NAN;
    }
  }
}

template <int P>
void launch_streams(dim3 grid, size_t lds, hipStream_t st, bool first, const int64_t* seq, const float* points, const uint8_t* gm,
                    const uint8_t* rm, const float* weights, int N, int K, int V, const EnsembleWorkspace& ws) {
  if (first)
    hipLaunchKernelGGL(ensemble_accumulate_kernel<P>, grid, dim3(256), lds, st, seq, points, rm, weights, N, K, V, ws);
  else
    hipLaunchKernelGGL(ensemble_deviation_kernel<P>, grid, dim3(256), 0, st, seq, points, gm, rm, weights, N, K, V, ws);
}

void launch_streams(int P, dim3 grid, size_t lds, hipStream_t st, bool first, const int64_t* seq, const float* points, const uint8_t* gm,
                    const uint8_t* rm, const float* weights, int N, int K, int V, const EnsembleWorkspace& ws) {
  switch (P) {
    case 1: return launch_streams<1>(grid, lds, st, first, seq, points, gm, rm, weights, N, K, V, ws);
    case 2: return launch_streams<2>(grid, lds, st, first, seq, points, gm, rm, weights, N, K, V, ws);
    case 3: return launch_streams<3>(grid, lds, st, first, seq, points, gm, rm, weights, N, K, V, ws);
    case 4: return launch_streams<4>(grid, lds, st, first, seq, points, gm, rm, weights, N, K, V, ws);
    default: return launch_streams<5>(grid, lds, st, first, seq, points, gm, rm, weights, N, K, V, ws);
  }
}

}  // namespace
}  // namespace diffab

using namespace diffab;

extern "C" {

int diffab_metrics_ensemble(const int64_t* seq_idx, const float* points, const uint8_t* generation_mask, const uint8_t* residue_mask,
                            const float* weights, int32_t G, int32_t N, int32_t K, int32_t P, int32_t V, double pseudocount, float* aa_freq,
                            float* entropy, int64_t* consensus, float* mean_points, float* rmsf, float* log_prob, float* consensus_identity,
                            float* rmsd_to_mean, float* n_eff, int64_t* central, void* workspace, size_t workspace_bytes, void* stream) {
  StreamOrder order_(stream);
  static_assert(kMaxPoints == 5, "launch_streams dispatches P = 1..5");
  DIFFAB_REQUIRE(G >= 0 && N >= 1 && K >= 1, DIFFAB_ERR_ARG, "metrics_ensemble: negative or empty extent (%d groups, group size %d, K = %d)", G, N,
                 K);
  DIFFAB_REQUIRE(P >= 1 && P <= kMaxPoints, DIFFAB_ERR_ARG, "metrics_ensemble: P = %d points per residue outside [1, %d]", P, kMaxPoints);
  DIFFAB_REQUIRE(N <= kMaxGroup, DIFFAB_ERR_ARG, "metrics_ensemble: group size N = %d, at most %d designs per group", N, kMaxGroup);
  DIFFAB_REQUIRE(K <= kMaxK, DIFFAB_ERR_ARG, "metrics_ensemble: K = %d residues per patch, at most %d", K, kMaxK);
  DIFFAB_REQUIRE(V >= 1 && V <= kMaxClasses, DIFFAB_ERR_ARG, "metrics_ensemble: V = %d classes outside [1, %d]", V, kMaxClasses);
  DIFFAB_REQUIRE(pseudocount >= 0.0 && pseudocount < static_cast<double>(INFINITY), DIFFAB_ERR_ARG,
                 "metrics_ensemble: the pseudocount must be finite and >= 0, got %g", pseudocount);
  if (G == 0) return DIFFAB_OK;
  DIFFAB_REQUIRE(seq_idx && points && generation_mask, DIFFAB_ERR_ARG, "metrics_ensemble: null input");
  const EnsembleWorkspace ws = carve_ensemble(workspace, G, N, K, P, V);
  if (const int e = workspace_ok("metrics_ensemble", workspace, 16, workspace_bytes, ws.bytes)) return e;
  const int S = (N + kSlice - 1) / kSlice, KC = (K + kChunk - 1) / kChunk;
  const dim3 grid(static_cast<unsigned>(G), static_cast<unsigned>(S), static_cast<unsigned>(KC));
  const size_t lds = static_cast<size_t>(kWaves) * static_cast<size_t>(V > 3 * P ? V : 3 * P) * kChunk * sizeof(double);
  hipStream_t st = as_stream(stream);
  launch_streams(P, grid, lds, st, true, seq_idx, points, generation_mask, residue_mask, weights, N, K, V, ws);
  hipLaunchKernelGGL(ensemble_finish_kernel, dim3(static_cast<unsigned>(G), static_cast<unsigned>(KC)), dim3(64), 0, st, generation_mask,
                     residue_mask, weights, N, K, P, V, S, pseudocount, ws, aa_freq, entropy, consensus, mean_points, n_eff);
  if (rmsf || log_prob || consensus_identity || rmsd_to_mean || central) {
    launch_streams(P, grid, 0, st, false, seq_idx, points, generation_mask, residue_mask, weights, N, K, V, ws);
    hipLaunchKernelGGL(ensemble_rows_kernel, dim3(static_cast<unsigned>(G)), dim3(256), 0, st, residue_mask, weights, N, K, P, S, KC, ws, rmsf,
                       log_prob, consensus_identity, rmsd_to_mean, central);
  }
  DIFFAB_LAUNCH_CHECK();
  return DIFFAB_OK;
}

}  // extern "C"
