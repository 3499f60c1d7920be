// refine_kernels.hip - backbone refinement on the device: diffab_refine_backbone closes the peptide bonds between
// the rigid residue frames of finished designs by a fixed number of Jacobi steps on a sum of pair-distance terms.  The definition is the
// header comment of the entry in include/diffab_hip.h; the float64 restatement is tests/test_refine_host.py::refine_ref.
//
// Built with -ffp-contract=off (csrc/Makefile): every force, step and energy term is the fp32 expression written here, one rounding per
// operation, so a design's result is a function of its own row and of K.  One work-group per design row for the whole run: the atoms of
// the row live in LDS in two buffers (a step reads one and writes the other), the frames of the moving residues in a third array that
// only their owner reads.  VALU + LDS only, no atomics, no per-thread arrays with a run-time index; every value reaches memory through
// plain C++ stores.
#include <climits>

#include "analysis_prep.h"

namespace diffab {
namespace {

constexpr int kMaxK = DIFFAB_REFINE_MAX_K;
constexpr int kThreads = 256;
constexpr int kLanes = 4;                    // lanes that share the clash partners of one moving residue
constexpr int kPerPass = kThreads / kLanes;  // moving residues per pass of the work-group
static_assert(kMaxK <= kThreads, "the energy pass and the staging give one thread to every slot");
static_assert(kMaxK <= SHRT_MAX, "slots travel as 16-bit numbers");

// local coordinates of N and C in the residue frame (io.IDEAL_BACKBONE; CA is the origin), and the targets of the four bonded terms
constexpr float kNx = -0.525f, kNy = 1.363f, kCx = 1.526f;
constexpr float kBond = DIFFAB_REFINE_BOND, kAngleCaN = DIFFAB_REFINE_CA_N, kAngleCCa = DIFFAB_REFINE_C_CA, kTrans = DIFFAB_REFINE_CA_CA;
constexpr float kInertia = DIFFAB_REFINE_INERTIA;
constexpr float kTiny = 1e-6f;  // a pair closer than this exerts no force (guidance's guard); below it Exp uses its limit values
constexpr unsigned kIn = 1u, kMoving = 2u;

// ------------------------------------------------------------------ the refinement
struct RefineParams {
  int iterations;
  float step, rot_step;  // rot_step = step / kInertia, one fp32 division on the host
  float w_bond, w_angle, w_trans, w_clash, w_tether, clash;
};

struct Vec3 {
  float x, y, z;
};
__device__ inline Vec3 v3(float x, float y, float z) { return Vec3{x, y, z}; }
__device__ inline Vec3 v3(const float4& a) { return Vec3{a.x, a.y, a.z}; }
__device__ inline Vec3 operator+(Vec3 a, Vec3 b) { return Vec3{a.x + b.x, a.y + b.y, a.z + b.z}; }
__device__ inline Vec3 operator-(Vec3 a, Vec3 b) { return Vec3{a.x - b.x, a.y - b.y, a.z - b.z}; }
__device__ inline Vec3 operator*(float s, Vec3 a) { return Vec3{s * a.x, s * a.y, s * a.z}; }
__device__ inline Vec3 cross(Vec3 a, Vec3 b) { return Vec3{a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }
__device__ inline float norm2(Vec3 a) { return (a.x * a.x + a.y * a.y) + a.z * a.z; }
__device__ inline float4 f4(Vec3 a) { return make_float4(a.x, a.y, a.z, 0.f); }

// force on a of the term w (|a - b| - d0)^2: ((-2 w) (d - d0) / d) (a - b); none below kTiny
__device__ inline Vec3 pair_force(Vec3 a, Vec3 b, float d0, float w) {
  const Vec3 r = a - b;
  const float d = sqrtf(norm2(r));
  const float coef = d < kTiny ? 0.f : ((-2.f * w) * (d - d0)) / d;
  return coef * r;
}

__device__ inline float pair_energy(Vec3 a, Vec3 b, float d0, float w) {
  const float e = sqrtf(norm2(a - b)) - d0;
  return w * (e * e);
}

// The LDS of one work-group, carved from the dynamic allocation: 148 K bytes (DIFFAB_REFINE_LDS_BYTES).
struct RowLds {
  float4* ca;  // [2][K]
  float4* n;   // [2][K]
  float4* c;   // [2][K]
  int2* key;   // [K] chain, residue_idx
  float* O;    // [K][9], rows = local axes; read and written by the owner of the slot only
  short2* link;  // [K] successor, predecessor
  short* moving;  // [K] the moving slots in ascending order
  uint8_t* flag;  // [K] kIn | kMoving
  uint8_t* turned;  // [K] the frame was rotated at least once
};

__device__ inline RowLds carve_row(unsigned char* base, int K) {
  RowLds s;
  s.ca = reinterpret_cast<float4*>(base);
  s.n = s.ca + 2 * K;
  s.c = s.n + 2 * K;
  s.key = reinterpret_cast<int2*>(s.c + 2 * K);  // (every array starts at a multiple of its element size for any K)
  s.O = reinterpret_cast<float*>(s.key + K);
  s.link = reinterpret_cast<short2*>(s.O + 9 * K);
  s.moving = reinterpret_cast<short*>(s.link + K);
  s.flag = reinterpret_cast<uint8_t*>(s.moving + K);
  s.turned = s.flag + K;
  return s;
}

// N and C of a frame: t + (kNx O0 + kNy O1) and t + kCx O0
__device__ inline void place_atoms(Vec3 t, const float* O, Vec3& n, Vec3& c) {
  const Vec3 e0 = v3(O[0], O[1], O[2]), e1 = v3(O[3], O[4], O[5]);
  n = t + (kNx * e0 + kNy * e1);
  c = t + kCx * e0;
}

// The five energy terms of the state in buffer b, reduced over the work-group in a fixed order; thread 0 returns with the totals.
// A link i -> succ(i) counts when one of its ends moves, an unordered clash pair once, the tether on the moving residues.
__device__ inline void row_energy(const RowLds& s, int b, int K, const RefineParams& p, const float* __restrict__ start, double (*s_red)[5],
                                  double (&total)[5]) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  double e0 = 0.0, e1 = 0.0, e2 = 0.0, e3 = 0.0, e4 = 0.0;
  if (tid < K && (s.flag[tid] & kIn) != 0u) {
    const int k = tid;
    const bool mine = (s.flag[k] & kMoving) != 0u;
    const Vec3 ca = v3(s.ca[b * K + k]), c = v3(s.c[b * K + k]);
    const int nx = s.link[k].x;
    if (nx >= 0 && (mine || (s.flag[nx] & kMoving) != 0u)) {
      const Vec3 n2 = v3(s.n[b * K + nx]), ca2 = v3(s.ca[b * K + nx]);
      e0 = static_cast<double>(pair_energy(c, n2, kBond, p.w_bond));
      e1 = static_cast<double>(pair_energy(ca, n2, kAngleCaN, p.w_angle));
      e1 += static_cast<double>(pair_energy(c, ca2, kAngleCCa, p.w_angle));
      e2 = static_cast<double>(pair_energy(ca, ca2, kTrans, p.w_trans));
    }
    const int2 me = s.key[k];
    for (int j = k + 1; j < K; ++j) {
      const unsigned fj = s.flag[j];
      if ((fj & kIn) == 0u || !(mine || (fj & kMoving) != 0u) || bonded(me.x, me.y, s.key[j].x, s.key[j].y)) continue;
      const float d = sqrtf(norm2(ca - v3(s.ca[b * K + j])));
      if (d < p.clash) {
        const float t = p.clash - d;
        e3 += static_cast<double>(p.w_clash * (t * t));
      }
    }
    if (mine) e4 = static_cast<double>(p.w_tether * norm2(ca - v3(start[k * 3], start[k * 3 + 1], start[k * 3 + 2])));
  }
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) {
    e0 += __shfl_xor(e0, d, 64);
    e1 += __shfl_xor(e1, d, 64);
    e2 += __shfl_xor(e2, d, 64);
    e3 += __shfl_xor(e3, d, 64);
    e4 += __shfl_xor(e4, d, 64);
  }
  __syncthreads();  // the totals of the pass before have been read
  if (lane == 0) s_red[wave][0] = e0, s_red[wave][1] = e1, s_red[wave][2] = e2, s_red[wave][3] = e3, s_red[wave][4] = e4;
  __syncthreads();
  if (tid == 0) {
#pragma unroll
    for (int v = 0; v < 5; ++v) total[v] = ((s_red[0][v] + s_red[1][v]) + s_red[2][v]) + s_red[3][v];
  }
}

__global__ void __launch_bounds__(kThreads)
refine_backbone_kernel(const float* __restrict__ translations, const float* __restrict__ orientations,
                       const uint8_t* __restrict__ generation_mask, const uint8_t* __restrict__ residue_mask, const int32_t* __restrict__ chain,
                       const int32_t* __restrict__ residue_idx, const int32_t* __restrict__ succ, const int32_t* __restrict__ pred,
                       int group_size, int K, RefineParams p, float* __restrict__ out_translations, float* __restrict__ out_orientations,
                       float* __restrict__ energy_before, float* __restrict__ energy_after, float* __restrict__ terms_after,
                       float* __restrict__ max_shift) {
  extern __shared__ __attribute__((aligned(16))) unsigned char s_raw[];
  __shared__ double s_red[4][5];
  __shared__ float s_shift[4];
  __shared__ int s_count;
  const RowLds s = carve_row(s_raw, K);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t row = blockIdx.x;
  const int64_t g = row / group_size;
  const float* t_in = translations + row * K * 3;
  const float* O_in = orientations + row * K * 9;

  // ---- stage the row: keys, links, flags, frames, and the atoms into both buffers
  if (tid < K) {
    const int k = tid;
    const bool in = residue_mask == nullptr || residue_mask[g * K + k] != 0;
    const bool mv = in && generation_mask[g * K + k] != 0;
    s.flag[k] = (in ? kIn : 0u) | (mv ? kMoving : 0u);
    s.turned[k] = 0;
    s.key[k] = make_int2(chain[g * K + k], residue_idx[g * K + k]);
    s.link[k] = make_short2(static_cast<short>(succ[g * K + k]), static_cast<short>(pred[g * K + k]));
#pragma unroll
    for (int e = 0; e < 9; ++e) s.O[k * 9 + e] = O_in[k * 9 + e];
    const Vec3 t = v3(t_in[k * 3], t_in[k * 3 + 1], t_in[k * 3 + 2]);
    Vec3 n, c;
    place_atoms(t, s.O + k * 9, n, c);
    s.ca[k] = s.ca[K + k] = f4(t);
    s.n[k] = s.n[K + k] = f4(n);
    s.c[k] = s.c[K + k] = f4(c);
  }
  __syncthreads();
  if (wave == 0) {  // the moving slots in ascending order
    int count = 0;
    const unsigned long long below = (1ull << lane) - 1ull;
    for (int k0 = 0; k0 < K; k0 += 64) {
      const int k = k0 + lane;
      const bool mv = k < K && (s.flag[k] & kMoving) != 0u;
      const unsigned long long votes = __ballot(mv);
      if (mv) s.moving[count + __popcll(votes & below)] = static_cast<short>(k);
      count += __popcll(votes);
    }
    if (lane == 0) s_count = count;
  }
  __syncthreads();
  const int M = s_count;

  double total[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
  if (energy_before != nullptr) {
    row_energy(s, 0, K, p, t_in, s_red, total);
    if (tid == 0) energy_before[row] = static_cast<float>((((total[0] + total[1]) + total[2]) + total[3]) + total[4]);
  }

  // ---- the steps: a group of kLanes lanes per moving residue, kPerPass residues per pass; state b is read, state b ^ 1 written
  int b = 0;
  const int grp = tid / kLanes, sub = tid % kLanes;
  if (M > 0) {
    for (int it = 0; it < p.iterations; ++it) {
      for (int m0 = 0; m0 < M; m0 += kPerPass) {
        const int m = m0 + grp;
        if (m >= M) continue;  // (whole groups: the lanes of a group stay together)
        const int k = s.moving[m];
        const Vec3 ca = v3(s.ca[b * K + k]);
        // clash partners j = sub, sub + kLanes, ... in ascending order, then (lane 0 + lane 1) + (lane 2 + lane 3)
        Vec3 push = v3(0.f, 0.f, 0.f);
        if (p.w_clash != 0.f) {
          const int2 me = s.key[k];
          for (int j = sub; j < K; j += kLanes) {
            if (j == k || (s.flag[j] & kIn) == 0u || bonded(me.x, me.y, s.key[j].x, s.key[j].y)) continue;
            const Vec3 r = ca - v3(s.ca[b * K + j]);
            const float d = sqrtf(norm2(r));
            if (d < p.clash && !(d < kTiny)) push = push + (((2.f * p.w_clash) * (p.clash - d)) / d) * r;
          }
          push.x += __shfl_xor(push.x, 1, 64), push.y += __shfl_xor(push.y, 1, 64), push.z += __shfl_xor(push.z, 1, 64);
          push.x += __shfl_xor(push.x, 2, 64), push.y += __shfl_xor(push.y, 2, 64), push.z += __shfl_xor(push.z, 2, 64);
        }
        if (sub != 0) continue;
        const Vec3 n = v3(s.n[b * K + k]), c = v3(s.c[b * K + k]);
        const short2 link = s.link[k];
        Vec3 f_n = v3(0.f, 0.f, 0.f), f_ca = f_n, f_c = f_n;
        if (link.x >= 0) {  // the link to the successor: this residue's CA and C
          const Vec3 n2 = v3(s.n[b * K + link.x]), ca2 = v3(s.ca[b * K + link.x]);
          f_c = f_c + pair_force(c, n2, kBond, p.w_bond);
          f_ca = f_ca + pair_force(ca, n2, kAngleCaN, p.w_angle);
          f_c = f_c + pair_force(c, ca2, kAngleCCa, p.w_angle);
          f_ca = f_ca + pair_force(ca, ca2, kTrans, p.w_trans);
        }
        if (link.y >= 0) {  // the link from the predecessor: this residue's N and CA
          const Vec3 c0 = v3(s.c[b * K + link.y]), ca0 = v3(s.ca[b * K + link.y]);
          f_n = f_n + pair_force(n, c0, kBond, p.w_bond);
          f_n = f_n + pair_force(n, ca0, kAngleCaN, p.w_angle);
          f_ca = f_ca + pair_force(ca, c0, kAngleCCa, p.w_angle);
          f_ca = f_ca + pair_force(ca, ca0, kTrans, p.w_trans);
        }
        f_ca = f_ca + push;
        if (p.w_tether != 0.f) f_ca = f_ca + (-2.f * p.w_tether) * (ca - v3(t_in[k * 3], t_in[k * 3 + 1], t_in[k * 3 + 2]));
        const Vec3 F = (f_n + f_ca) + f_c;
        const Vec3 torque = cross(n - ca, f_n) + cross(c - ca, f_c);
        Vec3 t = ca;
        if (F.x != 0.f || F.y != 0.f || F.z != 0.f) t = ca + p.step * F;
        float* O = s.O + k * 9;
        const Vec3 w = p.rot_step * torque;
        if (w.x != 0.f || w.y != 0.f || w.z != 0.f) {  // O <- O Exp(w)^T, Exp(w) = I + a S + b S^2 with S = hat(w), S^2 = w w^T - |w|^2 I
          const float n2 = norm2(w), nn = sqrtf(n2);
          const float sn = sinf(nn), cn = cosf(nn);
          const float a = nn < kTiny ? 1.f : sn / nn, bb = nn < kTiny ? 0.5f : (1.f - cn) / n2;
          const float R00 = 1.f + bb * (w.x * w.x - n2), R01 = a * -w.z + bb * (w.x * w.y), R02 = a * w.y + bb * (w.x * w.z);
          const float R10 = a * w.z + bb * (w.y * w.x), R11 = 1.f + bb * (w.y * w.y - n2), R12 = a * -w.x + bb * (w.y * w.z);
          const float R20 = a * -w.y + bb * (w.z * w.x), R21 = a * w.x + bb * (w.z * w.y), R22 = 1.f + bb * (w.z * w.z - n2);
#pragma unroll
          for (int i = 0; i < 3; ++i) {
            const float o0 = O[i * 3], o1 = O[i * 3 + 1], o2 = O[i * 3 + 2];
            O[i * 3] = (o0 * R00 + o1 * R01) + o2 * R02;
            O[i * 3 + 1] = (o0 * R10 + o1 * R11) + o2 * R12;
            O[i * 3 + 2] = (o0 * R20 + o1 * R21) + o2 * R22;
          }
          s.turned[k] = 1;
        }
        Vec3 n_new, c_new;
        place_atoms(t, O, n_new, c_new);
        s.ca[(b ^ 1) * K + k] = f4(t);
        s.n[(b ^ 1) * K + k] = f4(n_new);
        s.c[(b ^ 1) * K + k] = f4(c_new);
      }
      __syncthreads();
      b ^= 1;
    }
  }

  // ---- the rows of every frame that was rotated, orthonormalised in the order of io.frames_from_backbone
  if (tid < K && s.turned[tid] != 0) {
    float* O = s.O + tid * 9;
    Vec3 e1 = v3(O[0], O[1], O[2]);
    const float len1 = sqrtf(norm2(e1));
    e1 = v3(e1.x / len1, e1.y / len1, e1.z / len1);
    const Vec3 r1 = v3(O[3], O[4], O[5]);
    const float dot = (e1.x * r1.x + e1.y * r1.y) + e1.z * r1.z;
    Vec3 e2 = r1 - dot * e1;
    const float len2 = sqrtf(norm2(e2));
    e2 = v3(e2.x / len2, e2.y / len2, e2.z / len2);
    const Vec3 e3 = cross(e1, e2);
    O[0] = e1.x, O[1] = e1.y, O[2] = e1.z, O[3] = e2.x, O[4] = e2.y, O[5] = e2.z, O[6] = e3.x, O[7] = e3.y, O[8] = e3.z;
    Vec3 n_new, c_new;
    place_atoms(v3(s.ca[b * K + tid]), O, n_new, c_new);
    s.n[b * K + tid] = f4(n_new);
    s.c[b * K + tid] = f4(c_new);
  }
  __syncthreads();

  if (energy_after != nullptr || terms_after != nullptr) {
    row_energy(s, b, K, p, t_in, s_red, total);
    if (tid == 0) {
      if (energy_after != nullptr) energy_after[row] = static_cast<float>((((total[0] + total[1]) + total[2]) + total[3]) + total[4]);
      if (terms_after != nullptr) {
#pragma unroll
        for (int v = 0; v < 5; ++v) terms_after[row * 5 + v] = static_cast<float>(total[v]);
      }
    }
  }

  // ---- results: a moving residue from LDS, every other one the input's bits
  float shift = 0.f;
  if (tid < K) {
    const int k = tid;
    const bool mv = (s.flag[k] & kMoving) != 0u;
    const float4 t = s.ca[b * K + k];
    const float x0 = t_in[k * 3], y0 = t_in[k * 3 + 1], z0 = t_in[k * 3 + 2];
    float* t_out = out_translations + (row * K + k) * 3;
    float* O_out = out_orientations + (row * K + k) * 9;
    t_out[0] = mv ? t.x : x0, t_out[1] = mv ? t.y : y0, t_out[2] = mv ? t.z : z0;
#pragma unroll
    for (int e = 0; e < 9; ++e) {
      const float given = O_in[k * 9 + e], mine = s.O[k * 9 + e];
      O_out[e] = mv ? mine : given;
    }
    if (mv) shift = sqrtf(norm2(v3(t) - v3(x0, y0, z0)));
  }
  if (max_shift != nullptr) {
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) shift = fmaxf(shift, __shfl_xor(shift, d, 64));  // a maximum: the order does not matter
    if (lane == 0) s_shift[wave] = shift;
    __syncthreads();
    if (tid == 0) max_shift[row] = fmaxf(fmaxf(s_shift[0], s_shift[1]), fmaxf(s_shift[2], s_shift[3]));
  }
}

bool finite_at_least(float v, float lowest) { return v >= lowest && v < INFINITY; }

}  // namespace
}  // namespace diffab

using namespace diffab;

extern "C" {

int diffab_refine_backbone(const float* translations, const float* orientations, const uint8_t* generation_mask, const uint8_t* residue_mask,
                           const int32_t* chain, const int32_t* residue_idx, int32_t rows, int32_t group_size, int32_t K,
                           const diffab_refine_options* opt, float* out_translations, float* out_orientations, float* energy_before,
                           float* energy_after, float* terms_after, float* max_shift, void* workspace, size_t workspace_bytes, void* stream) {
  StreamOrder order_(stream);
  diffab_refine_options o = DIFFAB_REFINE_DEFAULTS;
  if (opt != nullptr) {
    DIFFAB_REQUIRE(opt->struct_bytes == sizeof(diffab_refine_options), DIFFAB_ERR_ARG,
                   "refine_backbone: options struct_bytes = %u, this library's diffab_refine_options has %zu", opt->struct_bytes,
                   sizeof(diffab_refine_options));
    o = *opt;
  }
  DIFFAB_REQUIRE(rows >= 0 && group_size >= 1 && K >= 1, DIFFAB_ERR_ARG, "refine_backbone: negative or empty extent (%d rows, group size %d, K = %d)",
                 rows, group_size, K);
  DIFFAB_REQUIRE(K <= kMaxK, DIFFAB_ERR_ARG, "refine_backbone: K = %d residues per patch, at most %d", K, kMaxK);
  DIFFAB_REQUIRE(rows % group_size == 0, DIFFAB_ERR_ARG, "refine_backbone: %d rows are not a multiple of group_size = %d", rows, group_size);
  DIFFAB_REQUIRE(o.iterations >= 0 && o.iterations <= DIFFAB_REFINE_MAX_ITERATIONS, DIFFAB_ERR_ARG,
                 "refine_backbone: iterations = %d outside [0, %d]", o.iterations, DIFFAB_REFINE_MAX_ITERATIONS);
  DIFFAB_REQUIRE(o.step > 0.f && o.step < INFINITY, DIFFAB_ERR_ARG, "refine_backbone: step must be finite and > 0, got %g",
                 static_cast<double>(o.step));
  const float weights[5] = {o.w_bond, o.w_angle, o.w_trans, o.w_clash, o.w_tether};
  const char* const names[5] = {"w_bond", "w_angle", "w_trans", "w_clash", "w_tether"};
  float heaviest = 0.f;
  for (int v = 0; v < 5; ++v) {
    DIFFAB_REQUIRE(finite_at_least(weights[v], 0.f), DIFFAB_ERR_ARG, "refine_backbone: %s must be finite and >= 0, got %g", names[v],
                   static_cast<double>(weights[v]));
    heaviest = weights[v] > heaviest ? weights[v] : heaviest;
  }
  DIFFAB_REQUIRE(o.clash_distance > 0.f && o.clash_distance < INFINITY, DIFFAB_ERR_ARG,
                 "refine_backbone: clash_distance must be finite and > 0, got %g", static_cast<double>(o.clash_distance));
  DIFFAB_REQUIRE(!(static_cast<double>(o.step) * static_cast<double>(heaviest) > DIFFAB_REFINE_MAX_STEP_WEIGHT), DIFFAB_ERR_ARG,
                 "refine_backbone: step x largest weight = %g x %g is above %g: the iteration is not stable there",
                 static_cast<double>(o.step), static_cast<double>(heaviest), DIFFAB_REFINE_MAX_STEP_WEIGHT);
  if (rows == 0) return DIFFAB_OK;
  DIFFAB_REQUIRE(translations && orientations && generation_mask && chain && residue_idx, DIFFAB_ERR_ARG, "refine_backbone: null input");
  DIFFAB_REQUIRE(out_translations && out_orientations, DIFFAB_ERR_ARG, "refine_backbone: null output");
  DIFFAB_REQUIRE(out_translations != translations && out_orientations != orientations, DIFFAB_ERR_ARG,
                 "refine_backbone: an output aliases its input");
  DIFFAB_REQUIRE(workspace != nullptr && reinterpret_cast<uintptr_t>(workspace) % 16 == 0, DIFFAB_ERR_ARG,
                 "refine_backbone: the workspace must be a 16-byte aligned device buffer");
  const int32_t G = rows / group_size;
  const LinkWorkspace ws = carve_links(workspace, G, K);
  DIFFAB_REQUIRE(workspace_bytes >= ws.bytes, DIFFAB_ERR_WORKSPACE, "refine_backbone: workspace of %zu bytes, %zu needed", workspace_bytes,
                 ws.bytes);
  RefineParams p;
  p.iterations = o.iterations;
  p.step = o.step;
  p.rot_step = o.step / kInertia;
  p.w_bond = o.w_bond, p.w_angle = o.w_angle, p.w_trans = o.w_trans, p.w_clash = o.w_clash, p.w_tether = o.w_tether;
  p.clash = o.clash_distance;
  hipStream_t st = as_stream(stream);
  hipLaunchKernelGGL((chain_links_kernel<kThreads, kMaxK>), dim3(G), dim3(kThreads), 0, st, chain, residue_idx, residue_mask, K, ws.succ, ws.pred);
  hipLaunchKernelGGL(refine_backbone_kernel, dim3(rows), dim3(kThreads), DIFFAB_REFINE_LDS_BYTES(K), st, translations, orientations,
                     generation_mask, residue_mask, chain, residue_idx, ws.succ, ws.pred, group_size, K, p, out_translations,
                     out_orientations, energy_before, energy_after, terms_after, max_shift);
  DIFFAB_LAUNCH_CHECK();
  return DIFFAB_OK;
}

}  // extern "C"
