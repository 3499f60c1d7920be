// steering_kernels.hip - particle steering of the reverse sampler: sequential Monte Carlo over the rows of a group.
// Three kernels around the update of a steering step, all launched from launch_reverse_update_philox:
//   steer_energy_kernel    before the update (and before the guidance shift): U_r of every row at x0_hat, the pass of guidance_row.h
//   steer_resample_kernel  after it: weights, ESS, systematic resampling - one work-group per group, doubles in LDS, fixed order
//   steer_gather_kernel    twice: the generated residues of the rows with a_j != j out of their ancestors into scratch, then into the state
// Each of them evaluates the steering-step predicate itself from by-value fields (t from t_dev under graph replay) and leaves a step that
// is not a steering step untouched; the eager loop, which knows t on the host, does not launch them at such a step.  Plain C++ loads and
// stores, no atomics; built with -ffp-contract=off like the sampler's arithmetic.
#include <cmath>

#include "common.h"
#include "denoiser_internal.h"
#include "guidance_row.h"
#include "philox.h"

namespace diffab {

constexpr int kSteerThreads = 256, kSteerPer = DIFFAB_STEER_MAX_GROUP / kSteerThreads;
static_assert(DIFFAB_STEER_MAX_GROUP % kSteerThreads == 0, "every thread holds the same number of rows of the largest group");

__device__ inline bool steer_runs(const SteeringDev& sd, const int32_t* plan_next, int t, bool force) {
  return force || steer_is_step(sd, t, plan_next != nullptr ? plan_next[t] : t - 1);
}

// U_r = w_clash sum_nonbonded max(0, d0 - d)^2 + w_bond sum_bonded (d - L)^2 at p = x0_hat (generated) / x (others): guidance_energy_kernel's
// pass and tree, so the two sums are bitwise diffab_guidance_energy's at the recorded pred_translations.
__global__ __launch_bounds__(kGuideThreads) void steer_energy_kernel(SteeringDev sd, GuidanceDev g, const float* __restrict__ x,
                                                                     const float* __restrict__ eps_hat, const uint8_t* __restrict__ gm,
                                                                     const float* __restrict__ omabs, const float* __restrict__ abs_,
                                                                     const int32_t* __restrict__ plan_next, int t,
                                                                     const int* __restrict__ t_dev, int K, float* __restrict__ out,
                                                                     bool force) {
  if (t_dev != nullptr) t = *t_dev;
  if (!steer_runs(sd, plan_next, t, force)) return;  // uniform over the launch
  const int64_t row = blockIdx.x;
  GuideSums sums;
  guide_row<true>(row, K, x, eps_hat, omabs[t], abs_[t], gm, g, sums, [](int64_t, float, float, float) {});
  guide_reduce(sums);
  if (threadIdx.x == 0) out[row] = sd.w_clash * sums.clash + sd.w_bond * sums.bond;
}

// One work-group per group of N <= DIFFAB_STEER_MAX_GROUP rows; thread `tid` holds the rows tid per .. tid per + per - 1, per = ceil(N /
// 256), so sums run in row order inside a thread and in a fixed tree / scan across threads: the result of a group depends on the group alone.
//   logw_r += -(lambda (U_r - u_prev_r)) (fp32);  w_r = exp(logw_r - max finite logw) in double, 0 for a non-finite logw;
//   ESS = S^2 / sum w^2, S = sum w;  resample iff S > 0 and ESS < ess_threshold N;  all w = 0: no resampling, logw = 0;
//   C_i = (sum_{k <= i} w_k) / S;  a_j = the smallest i with C_i > (u + j) / N, at most the last row with w > 0;
//   resampled: logw_j = 0, u_prev_j = U_{a_j};  otherwise a_j = j, u_prev_j = U_j.
// u: u_explicit[group] (the teacher-forced entry), or lane .x of Philox (seed, first_patch + first row of the group, residue 0, t, STREAM_STEER).
__global__ __launch_bounds__(kSteerThreads) void steer_resample_kernel(SteeringDev sd, const int32_t* __restrict__ plan_next, int t,
                                                                       const int* __restrict__ t_dev, const float* __restrict__ u_explicit,
                                                                       uint64_t seed, int64_t first_patch, int32_t* __restrict__ record,
                                                                       int64_t rows, double* __restrict__ ess_out, bool force) {
  if (t_dev != nullptr) t = *t_dev;
  if (!steer_runs(sd, plan_next, t, force)) return;
  __shared__ double sC[DIFFAB_STEER_MAX_GROUP];
  __shared__ float sU[DIFFAB_STEER_MAX_GROUP];
  __shared__ double red[2][kSteerThreads];
  __shared__ double scan[kSteerThreads];
  __shared__ int red_i[kSteerThreads];
  const int tid = threadIdx.x, N = sd.group_size, per = (N + kSteerThreads - 1) / kSteerThreads;
  const int64_t base = static_cast<int64_t>(blockIdx.x) * N;
  const int lo = tid * per;
  float lw[kSteerPer];
  double mx = -INFINITY;
#pragma unroll
  for (int k = 0; k < kSteerPer; ++k) {
    const int r = lo + k;
    lw[k] = 0.f;
    if (k < per && r < N) {
      const float U = sd.energy[base + r];
      lw[k] = sd.logw[base + r] + (-(sd.strength * (U - sd.u_prev[base + r])));
      sU[r] = U;
      if (isfinite(lw[k])) mx = fmax(mx, static_cast<double>(lw[k]));
    }
  }
  red[0][tid] = mx;
  __syncthreads();
  for (int s = kSteerThreads / 2; s > 0; s >>= 1) {
    if (tid < s) red[0][tid] = fmax(red[0][tid], red[0][tid + s]);
    __syncthreads();
  }
  mx = red[0][0];
  __syncthreads();
  double pre[kSteerPer], s1 = 0.0, s2 = 0.0;
  int last = -1;
#pragma unroll
  for (int k = 0; k < kSteerPer; ++k) {
    const int r = lo + k;
    double w = 0.0;
    if (k < per && r < N && isfinite(lw[k])) w = exp(static_cast<double>(lw[k]) - mx);
    s1 += w;
    s2 += w * w;
    pre[k] = s1;
    if (w > 0.0) last = r;
  }
  red[0][tid] = s1;
  red[1][tid] = s2;
  red_i[tid] = last;
  scan[tid] = s1;
  __syncthreads();
  for (int s = kSteerThreads / 2; s > 0; s >>= 1) {
    if (tid < s) {
      red[0][tid] += red[0][tid + s];
      red[1][tid] += red[1][tid + s];
      red_i[tid] = max(red_i[tid], red_i[tid + s]);
    }
    __syncthreads();
  }
  for (int off = 1; off < kSteerThreads; off <<= 1) {  // inclusive scan of the threads' sums
    const double v = tid >= off ? scan[tid - off] : 0.0;
    __syncthreads();
    scan[tid] += v;
    __syncthreads();
  }
  const double S = red[0][0], S2 = red[1][0], excl = tid > 0 ? scan[tid - 1] : 0.0;
  const int last_nz = red_i[0];
  const bool none = !(S > 0.0);
  const double ess = none ? 0.0 : S * S / S2;
  const bool resample = !none && ess < static_cast<double>(sd.ess_threshold) * N;
#pragma unroll
  for (int k = 0; k < kSteerPer; ++k) {
    const int r = lo + k;
    if (k < per && r < N) sC[r] = none ? 0.0 : (excl + pre[k]) / S;
  }
  __syncthreads();
  float u = 0.f;
  if (resample)
    u = u_explicit != nullptr ? u_explicit[blockIdx.x] : philox_uniform4(seed, static_cast<uint32_t>(first_patch + base), 0u,
                                                                         static_cast<uint32_t>(t), STREAM_STEER).x;
#pragma unroll
  for (int k = 0; k < kSteerPer; ++k) {
    const int j = lo + k;
    if (!(k < per && j < N)) continue;
    int a = j;
    float lw_out = none ? 0.f : lw[k], up_out = sU[j];
    if (resample) {
      const double pos = (static_cast<double>(u) + j) / N;
      int l = 0, h = N;
      while (l < h) {
        const int mid = (l + h) >> 1;
        if (sC[mid] > pos) h = mid;
        else l = mid + 1;
      }
      a = min(l, last_nz);
      lw_out = 0.f;
      up_out = sU[a];
    }
    sd.logw[base + j] = lw_out;
    sd.u_prev[base + j] = up_out;
    sd.step_anc[base + j] = a;
    if (record != nullptr) record[static_cast<int64_t>(t) * rows + base + j] = a;
  }
  if (tid == 0 && ess_out != nullptr) ess_out[blockIdx.x] = ess;
}

// One thread per (row, residue), neighbouring residues in neighbouring lanes - the update kernel's access pattern; the state is 2 + 3 + 9
// dwords per residue at 8-, 12- and 36-byte strides, and the generation mask is ragged, so a residue's own dwords are the widest unit
// that is always aligned.  kOut: the generated residues of every row j with a_j != j are read from row a_j of the same group into
// scratch (seq | x | O, at the residue's own index); !kOut: scratch into the state.  Two launches: the map is no permutation in place.
// A residue of a row with a_j = j costs one read (the row's ancestor), a residue of a moved row that is not generated two (and its
// mask).  The destination's mask decides; the source residue is read whatever its own mask says.  anc holds indices local to groups of
// `group` rows.
template <bool kOut>
__global__ void steer_gather_kernel(SteeringDev sd, const int32_t* __restrict__ plan_next, int t, const int* __restrict__ t_dev,
                                    const int32_t* __restrict__ anc, int group, int64_t* __restrict__ seq, float* __restrict__ x,
                                    float* __restrict__ O, const uint8_t* __restrict__ gm, int64_t n, int K, void* __restrict__ scratch,
                                    bool copy_seq, bool force) {
  if (t_dev != nullptr) t = *t_dev;
  if (!steer_runs(sd, plan_next, t, force)) return;
  const int64_t i = blockIdx.x * static_cast<int64_t>(blockDim.x) + threadIdx.x;
  if (i >= n) return;
  const int64_t row = i / K;
  const int a = anc[row], self = static_cast<int>(row % group);
  if (a == self || a < 0 || a >= group) return;  // an unmoved row: one read (the same word for all its residues)
  if (!gm[i]) return;
  int64_t* s_seq = static_cast<int64_t*>(scratch);
  float* s_x = reinterpret_cast<float*>(s_seq + n);
  float* s_O = s_x + 3 * n;
  if (kOut) {
    const int64_t src = (row - self + a) * K + i % K;
    if (copy_seq) s_seq[i] = seq[src];
#pragma unroll
    for (int c = 0; c < 3; ++c) s_x[i * 3 + c] = x[src * 3 + c];
#pragma unroll
    for (int c = 0; c < 9; ++c) s_O[i * 9 + c] = O[src * 9 + c];
  } else {
    if (copy_seq) seq[i] = s_seq[i];
#pragma unroll
    for (int c = 0; c < 3; ++c) x[i * 3 + c] = s_x[i * 3 + c];
#pragma unroll
    for (int c = 0; c < 9; ++c) O[i * 9 + c] = s_O[i * 9 + c];
  }
}

static GuidanceDev potential_of(const SteeringDev& sd) {
  GuidanceDev g;
  g.chain = sd.chain;
  g.residue_idx = sd.residue_idx;
  g.residue_mask = sd.residue_mask;
  g.w_clash = sd.w_clash;
  g.clash_distance = sd.clash_distance;
  g.w_bond = sd.w_bond;
  g.bond_length = sd.bond_length;
  return g;
}

static unsigned residue_blocks(int64_t n) { return static_cast<unsigned>((n + 255) / 256); }

// The eager loop knows t on the host: a step that is not a steering step launches nothing.  Under graph replay (t_dev) one captured
// step serves every t, so the kernels are always launched and decide themselves.
static bool host_skips(const SteeringDev& sd, int t, const int* t_dev) {
  return t_dev == nullptr && !steer_is_step(sd, t, sd.next_host != nullptr ? sd.next_host[t] : t - 1);
}

int launch_steer_energy(const SteeringDev& sd, const diffab_sched* s, const StepPlanDev& plan, int t, const int* t_dev, const float* x,
                        const float* eps_hat, const uint8_t* gm, int B, int K, hipStream_t st) {
  if (host_skips(sd, t, t_dev)) return DIFFAB_OK;
  hipLaunchKernelGGL(steer_energy_kernel, dim3(B), dim3(kGuideThreads), 0, st, sd, potential_of(sd), x, eps_hat, gm, s->one_minus_alpha_bar_sqrt,
                     s->alpha_bar_sqrt, plan.next, t, t_dev, K, sd.energy, false);
  DIFFAB_LAUNCH_CHECK();
  return DIFFAB_OK;
}

static int launch_steer_gather(const SteeringDev& sd, const int32_t* plan_next, int t, const int* t_dev, const int32_t* anc, int group,
                               int64_t* seq, float* x, float* O, const uint8_t* gm, int64_t n, int K, void* scratch, bool copy_seq, bool force,
                               hipStream_t st) {
  hipLaunchKernelGGL(steer_gather_kernel<true>, dim3(residue_blocks(n)), dim3(256), 0, st, sd, plan_next, t, t_dev, anc, group, seq, x, O, gm, n,
                     K, scratch, copy_seq, force);
  DIFFAB_LAUNCH_CHECK();
  hipLaunchKernelGGL(steer_gather_kernel<false>, dim3(residue_blocks(n)), dim3(256), 0, st, sd, plan_next, t, t_dev, anc, group, seq, x, O, gm, n,
                     K, scratch, copy_seq, force);
  DIFFAB_LAUNCH_CHECK();
  return DIFFAB_OK;
}

int launch_steer_resample_gather(const SteeringDev& sd, const StepPlanDev& plan, int t, const int* t_dev, int64_t* seq, float* x, float* O,
                                 const uint8_t* gm, uint64_t seed, int64_t first_patch, int B, int K, bool copy_seq, hipStream_t st) {
  if (host_skips(sd, t, t_dev)) return DIFFAB_OK;
  hipLaunchKernelGGL(steer_resample_kernel, dim3(B / sd.group_size), dim3(kSteerThreads), 0, st, sd, plan.next, t, t_dev, nullptr, seed,
                     first_patch, sd.ancestors, static_cast<int64_t>(B), nullptr, false);
  DIFFAB_LAUNCH_CHECK();
  // (a group of one row, and a threshold of 0, never resample: every a_j = j, nothing to move - a by-value decision, the same for every step)
  if (sd.group_size == 1 || !(sd.ess_threshold > 0.0f)) return DIFFAB_OK;
  return launch_steer_gather(sd, plan.next, t, t_dev, sd.step_anc, sd.group_size, seq, x, O, gm, static_cast<int64_t>(B) * K, K, sd.scratch,
                             copy_seq, false, st);
}

}  // namespace diffab

using namespace diffab;

extern "C" {

int diffab_steer_energy(const float* x, const float* eps_hat, const uint8_t* gen_mask, const diffab_sched* s, int32_t t,
                        const diffab_sample_steering* steering, int32_t rows, int32_t K, float* energy_out, void* stream) {
  StreamOrder order_(stream);
  DIFFAB_REQUIRE(steering != nullptr, DIFFAB_ERR_ARG, "steer_energy: steering is null");
  diffab_sample_guidance terms{};
  terms.w_clash = steering->w_clash;
  terms.clash_distance = steering->clash_distance;
  terms.w_bond = steering->w_bond;
  terms.bond_length = steering->bond_length;
  terms.chain = steering->chain;
  terms.residue_idx = steering->residue_idx;
  if (int rc = check_guidance_terms(&terms, "steer_energy")) return rc;
  DIFFAB_REQUIRE(s && s->T > 0 && s->alpha_bar_sqrt && s->one_minus_alpha_bar_sqrt, DIFFAB_ERR_ARG, "steer_energy: bad schedule");
  DIFFAB_REQUIRE(t >= 1 && t <= s->T, DIFFAB_ERR_ARG, "steer_energy: t = %d outside [1, T = %d]", t, s->T);
  DIFFAB_REQUIRE(rows >= 0 && K >= 1 && static_cast<int64_t>(rows) * K < (1ll << 31), DIFFAB_ERR_ARG,
                 "steer_energy: need rows >= 0, K >= 1, rows*K < 2^31");
  DIFFAB_REQUIRE(x && eps_hat && gen_mask && energy_out, DIFFAB_ERR_ARG, "steer_energy: null pointer (x, eps_hat, gen_mask, energy_out)");
  if (rows == 0) return DIFFAB_OK;
  SteeringDev sd;
  sd.chain = steering->chain;
  sd.residue_idx = steering->residue_idx;
  sd.residue_mask = steering->residue_mask;
  sd.w_clash = steering->w_clash;
  sd.clash_distance = steering->clash_distance;
  sd.w_bond = steering->w_bond;
  sd.bond_length = steering->bond_length;
  hipLaunchKernelGGL(steer_energy_kernel, dim3(rows), dim3(kGuideThreads), 0, as_stream(stream), sd, potential_of(sd), x, eps_hat, gen_mask,
                     s->one_minus_alpha_bar_sqrt, s->alpha_bar_sqrt, nullptr, t, nullptr, K, energy_out, true);
  DIFFAB_LAUNCH_CHECK();
  return DIFFAB_OK;
}

int diffab_steer_resample(float* logw, float* u_prev, const float* energy, const float* u, int32_t G, int32_t N, float strength,
                          float ess_threshold, int32_t* ancestors_out, double* ess_out, void* stream) {
  StreamOrder order_(stream);
  DIFFAB_REQUIRE(G >= 0 && N >= 1 && N <= DIFFAB_STEER_MAX_GROUP && static_cast<int64_t>(G) * N < (1ll << 31), DIFFAB_ERR_ARG,
                 "steer_resample: need G >= 0, 1 <= N <= %d, G*N < 2^31 (G = %d, N = %d)", DIFFAB_STEER_MAX_GROUP, G, N);
  DIFFAB_REQUIRE(std::isfinite(strength) && strength >= 0.0f, DIFFAB_ERR_ARG, "steer_resample: strength = %g must be finite and >= 0", strength);
  DIFFAB_REQUIRE(ess_threshold >= 0.0f && ess_threshold <= 2.0f, DIFFAB_ERR_ARG, "steer_resample: ess_threshold = %g outside [0, 2]",
                 ess_threshold);
  DIFFAB_REQUIRE(logw && u_prev && energy && u && ancestors_out, DIFFAB_ERR_ARG,
                 "steer_resample: null pointer (logw, u_prev, energy, u and ancestors_out are required)");
  if (G == 0) return DIFFAB_OK;
  SteeringDev sd;
  sd.logw = logw;
  sd.u_prev = u_prev;
  sd.energy = const_cast<float*>(energy);
  sd.step_anc = ancestors_out;
  sd.strength = strength;
  sd.ess_threshold = ess_threshold;
  sd.group_size = N;
  hipLaunchKernelGGL(steer_resample_kernel, dim3(G), dim3(kSteerThreads), 0, as_stream(stream), sd, nullptr, 0, nullptr, u, 0ull, 0ll, nullptr,
                     static_cast<int64_t>(G) * N, ess_out, true);
  DIFFAB_LAUNCH_CHECK();
  return DIFFAB_OK;
}

int diffab_steer_gather(int64_t* seq, float* x, float* O, const uint8_t* gen_mask, const int32_t* ancestors, int32_t rows, int32_t K,
                        void* scratch, void* stream) {
  StreamOrder order_(stream);
  DIFFAB_REQUIRE(rows >= 0 && K >= 1 && static_cast<int64_t>(rows) * K < (1ll << 31), DIFFAB_ERR_ARG,
                 "steer_gather: need rows >= 0, K >= 1, rows*K < 2^31");
  DIFFAB_REQUIRE(seq && x && O && gen_mask && ancestors && scratch, DIFFAB_ERR_ARG, "steer_gather: null pointer");
  DIFFAB_REQUIRE(reinterpret_cast<uintptr_t>(scratch) % 8 == 0, DIFFAB_ERR_ARG, "steer_gather: scratch must be 8-byte aligned");
  if (rows == 0) return DIFFAB_OK;
  // (ancestors are row indices of the call here: one group of `rows` rows; an index outside [0, rows) leaves its row as it is)
  return launch_steer_gather(SteeringDev{}, nullptr, 0, nullptr, ancestors, rows, seq, x, O, gen_mask, static_cast<int64_t>(rows) * K, K, scratch,
                             true, true, as_stream(stream));
}

}  // extern "C"
