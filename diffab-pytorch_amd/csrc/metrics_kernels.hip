// metrics_kernels.hip - design metrics on the device: RMSD and amino-acid recovery of each design against the native
// (diffab_metrics_vs_native), the all-pairs RMSD / sequence-identity matrices of the designs of one patch (diffab_metrics_pairwise) and the
// greedy farthest-point choice of m designs from such a matrix (diffab_metrics_select_diverse).  The definitions are the header comments of the
// three entries.
//
// Built with -ffp-contract=off (csrc/Makefile): every result is a defined number.  The in-place squared distance is the fp32 sum
// ((acc + dx*dx) + dy*dy) + dz*dz over the counted points in ascending order; the superposed (Kabsch) numbers take their sums in fp64 (the
// products enter through explicit fma) and solve in fp64.  VALU + LDS only, no atomics; every value reaches memory through plain C++ stores.
#include <climits>

#include "analysis_common.h"

namespace diffab {
namespace {

constexpr int kMaxK = DIFFAB_METRICS_MAX_K;
constexpr int kMaxGroup = DIFFAB_METRICS_MAX_GROUP;
constexpr int kMaxPoints = DIFFAB_METRICS_MAX_POINTS;
constexpr int kMaxSegments = DIFFAB_METRICS_MAX_SEGMENTS;

// ------------------------------------------------------------------ the superposition solve
// One Hestenes rotation of the columns (a, b) of a 3 x 3 matrix: afterwards they are orthogonal.  Returns whether it turned anything.
__device__ inline bool orthogonalise(double (&a)[3], double (&b)[3]) {
  const double alpha = a[0] * a[0] + a[1] * a[1] + a[2] * a[2];
  const double beta = b[0] * b[0] + b[1] * b[1] + b[2] * b[2];
  const double gamma = a[0] * b[0] + a[1] * b[1] + a[2] * b[2];
  if (!(gamma * gamma > 1e-32 * alpha * beta)) return false;  // orthogonal to fp64 (or a zero column)
  const double zeta = (beta - alpha) / (2.0 * gamma);
  const double t = (zeta < 0.0 ? -1.0 : 1.0) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
  const double c = 1.0 / sqrt(1.0 + t * t), s = c * t;
#pragma unroll
  for (int x = 0; x < 3; ++x) {
    const double u = a[x], v = b[x];
    a[x] = c * u - s * v;
    b[x] = s * u + c * v;
  }
  return true;
}

// The least mean squared distance over proper rotations, from the centred sums: h = sum (p - cp)(q - cq)^T (row-major 3 x 3),
// spread = sum |p - cp|^2 + sum |q - cq|^2, over m points.  The singular values of h are the column norms after one-sided Jacobi sweeps
// (Hestenes): they come out to fp64 relative accuracy without forming h^T h, and the mirror case is the sign of det h on the smallest one.
__device__ inline double kabsch_msd(const double (&h)[9], double spread, double m) {
  double c0[3] = {h[0], h[3], h[6]}, c1[3] = {h[1], h[4], h[7]}, c2[3] = {h[2], h[5], h[8]};
  const double det = h[0] * (h[4] * h[8] - h[5] * h[7]) - h[1] * (h[3] * h[8] - h[5] * h[6]) + h[2] * (h[3] * h[7] - h[4] * h[6]);
  for (int sweep = 0; sweep < 30; ++sweep) {
    bool turned = orthogonalise(c0, c1);
    turned |= orthogonalise(c0, c2);
    turned |= orthogonalise(c1, c2);
    if (!turned) break;
  }
  const double s0 = sqrt(c0[0] * c0[0] + c0[1] * c0[1] + c0[2] * c0[2]);
  const double s1 = sqrt(c1[0] * c1[0] + c1[1] * c1[1] + c1[2] * c1[2]);
  const double s2 = sqrt(c2[0] * c2[0] + c2[1] * c2[1] + c2[2] * c2[2]);
  double trace = s0 + s1 + s2;
  if (det < 0.0) trace -= 2.0 * fmin(s0, fmin(s1, s2));
  return fmax(0.0, spread - 2.0 * trace) / m;
}

// ------------------------------------------------------------------ 1. designs against the native
// One wave per design row; the sets are the S segments, then the whole row (set S).
__global__ void __launch_bounds__(64)
metrics_vs_native_kernel(const int64_t* __restrict__ seq, const float* __restrict__ points, const int64_t* __restrict__ native_seq,
                         const float* __restrict__ native_points, const uint8_t* __restrict__ generation_mask,
                         const uint8_t* __restrict__ residue_mask, const int64_t* __restrict__ segment_idx, int group_size, int K, int P, int S,
                         float* __restrict__ aar, float* __restrict__ rmsd, float* __restrict__ rmsd_aligned, float* __restrict__ seg_aar,
                         float* __restrict__ seg_rmsd, float* __restrict__ seg_rmsd_aligned) {
  const int lane = threadIdx.x;
  const int64_t row = blockIdx.x;
  const int64_t g = row / group_size;
  const int64_t* sq = seq + row * K;
  const int64_t* nq = native_seq + g * K;
  const float* pp = points + row * K * P * 3;
  const float* np = native_points + g * K * P * 3;
  const uint8_t* gm = generation_mask + g * K;
  const uint8_t* rm = residue_mask ? residue_mask + g * K : nullptr;
  const int64_t* sg = segment_idx ? segment_idx + g * K : nullptr;

  for (int set = 0; set <= S; ++set) {
    auto inside = [&](int k) { return gm[k] != 0 && (rm == nullptr || rm[k] != 0) && (set == S || sg[k] == set); };
    double a[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};  // residues, matches, sum |p - q|^2, sum p, sum q
    for (int k = lane; k < K; k += 64) {
      if (!inside(k)) continue;
      a[0] += 1.0;
      if (sq[k] == nq[k]) a[1] += 1.0;
      for (int e = 0; e < P * 3; ++e) {
        const double p = pp[k * P * 3 + e], q = np[k * P * 3 + e], d = p - q;
        a[2] += d * d;
      }
      for (int e = 0; e < P; ++e) {
#pragma unroll
        for (int x = 0; x < 3; ++x) {
          a[3 + x] += static_cast<double>(pp[(k * P + e) * 3 + x]);
          a[6 + x] += static_cast<double>(np[(k * P + e) * 3 + x]);
        }
      }
    }
    wave_sum(a);
    const double n = a[0], m = a[0] * P;
    float out_aar = NAN, out_rmsd = NAN, out_aligned = NAN;
    if (n > 0.0) {  // (uniform: every lane holds the same sums)
      const double cp[3] = {a[3] / m, a[4] / m, a[5] / m}, cq[3] = {a[6] / m, a[7] / m, a[8] / m};
      double b[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};  // h, spread
      for (int k = lane; k < K; k += 64) {
        if (!inside(k)) continue;
        for (int e = 0; e < P; ++e) {
          double p[3], q[3];
#pragma unroll
          for (int x = 0; x < 3; ++x) {
            p[x] = static_cast<double>(pp[(k * P + e) * 3 + x]) - cp[x];
            q[x] = static_cast<double>(np[(k * P + e) * 3 + x]) - cq[x];
            b[9] += p[x] * p[x] + q[x] * q[x];
          }
#pragma unroll
          for (int x = 0; x < 3; ++x)
#pragma unroll
            for (int y = 0; y < 3; ++y) b[3 * x + y] = fma(p[x], q[y], b[3 * x + y]);
        }
      }
      wave_sum(b);
      const double h[9] = {b[0], b[1], b[2], b[3], b[4], b[5], b[6], b[7], b[8]};
      out_aar = static_cast<float>(a[1]) / static_cast<float>(n);
      out_rmsd = static_cast<float>(sqrt(a[2] / m));
      out_aligned = static_cast<float>(sqrt(kabsch_msd(h, b[9], m)));
    }
    if (lane == 0) {
      if (set == S) {
        aar[row] = out_aar;
        rmsd[row] = out_rmsd;
        rmsd_aligned[row] = out_aligned;
      } else {
        seg_aar[row * S + set] = out_aar;
        seg_rmsd[row * S + set] = out_rmsd;
        seg_rmsd_aligned[row * S + set] = out_aligned;
      }
    }
  }
}

// ------------------------------------------------------------------ 2. all pairs of a group
// Workspace of diffab_metrics_pairwise (DIFFAB_METRICS_PAIRWISE_WORKSPACE_BYTES covers the carves and their alignment).
struct PairWorkspace {
  float* pts;     // (G, K*P*3, N): counted points of every design, compacted, the designs of a group along the fastest axis
  uint32_t* tok;  // (G, ceil(K/4), N): counted tokens, four to a word (low 8 bits each), zero behind the last
  double* cen;    // (G*N, 4): centroid of the counted points and the sum of squared distances to it
  int32_t* cnt;   // (G): counted residues
  size_t bytes;
};

PairWorkspace carve_pairs(void* base, int64_t G, int64_t N, int64_t K, int64_t P) {
  Carver c(base);
  PairWorkspace w;
  w.pts = c.take<float>(static_cast<size_t>(G * N * K * P * 3));
  w.tok = c.take<uint32_t>(static_cast<size_t>(G * N * ((K + 3) / 4)));
  w.cen = c.take<double>(static_cast<size_t>(G * N * 4));
  w.cnt = c.take<int32_t>(static_cast<size_t>(G));
  w.bytes = c.bytes();
  return w;
}

// One work-group per (group, 64 designs): lane = design, the four waves share the points.  The counted residues of the group are listed
// in ascending order in LDS first (the same list for all its designs).
__global__ void __launch_bounds__(256)
metrics_pack_kernel(const int64_t* __restrict__ seq, const float* __restrict__ points, const uint8_t* __restrict__ generation_mask,
                    const uint8_t* __restrict__ residue_mask, int N, int K, int P, int aligned, PairWorkspace ws) {
  __shared__ uint16_t s_list[kMaxK];
  __shared__ int s_n;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int blocks = (N + 63) / 64;
  const int64_t g = blockIdx.x / blocks;
  const int d = (blockIdx.x % blocks) * 64 + lane;  // design of this lane
  const uint8_t* gm = generation_mask + g * K;
  const uint8_t* rm = residue_mask ? residue_mask + g * K : nullptr;
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
  const int n = s_n, m = n * P;
  if (blockIdx.x % blocks == 0 && tid == 0) ws.cnt[g] = n;
  if (d >= N) return;
  const int64_t row = g * N + d;
  const float* src = points + row * K * P * 3;
  float* pts = ws.pts + g * (static_cast<int64_t>(K) * P * 3) * N + d;
  for (int pt = wave; pt < m; pt += 4) {
    const float* p = src + (static_cast<int64_t>(s_list[pt / P]) * P + pt % P) * 3;
#pragma unroll
    for (int x = 0; x < 3; ++x) pts[static_cast<int64_t>(pt * 3 + x) * N] = p[x];
  }
  const int64_t* sq = seq + row * K;
  uint32_t* tok = ws.tok + g * ((K + 3) / 4) * N + d;
  for (int w = wave; w < (n + 3) / 4; w += 4) {
    uint32_t word = 0;
#pragma unroll
    for (int b = 0; b < 4; ++b)
      if (4 * w + b < n) word |= (static_cast<uint32_t>(sq[s_list[4 * w + b]]) & 0xFFu) << (8 * b);
    tok[static_cast<int64_t>(w) * N] = word;
  }
  if (aligned && wave == 0) {
    double c[3] = {0, 0, 0}, spread = 0;
    for (int pt = 0; pt < m; ++pt) {
      const float* p = src + (static_cast<int64_t>(s_list[pt / P]) * P + pt % P) * 3;
#pragma unroll
      for (int x = 0; x < 3; ++x) c[x] += static_cast<double>(p[x]);
    }
    if (m > 0) {
#pragma unroll
      for (int x = 0; x < 3; ++x) c[x] /= static_cast<double>(m);
    }
    for (int pt = 0; pt < m; ++pt) {
      const float* p = src + (static_cast<int64_t>(s_list[pt / P]) * P + pt % P) * 3;
#pragma unroll
      for (int x = 0; x < 3; ++x) {
        const double e = static_cast<double>(p[x]) - c[x];
        spread += e * e;
      }
    }
    double* out = ws.cen + row * 4;
    out[0] = c[0], out[1] = c[1], out[2] = c[2], out[3] = spread;
  }
}

constexpr int kPointChunk = 16;  // points of the two panels staged per pass
constexpr int kWordChunk = 32;   // token words of the two panels staged per pass

template <int TB>
struct Lanes;  // TB consecutive designs of a panel row as one LDS read
template <>
struct Lanes<4> {
  using F = float4;
  using U = uint4;
};
template <>
struct Lanes<2> {
  using F = float2;
  using U = uint2;
};

__device__ inline uint32_t differing_bytes(uint32_t x) {  // number of non-zero bytes
  x |= x >> 4;
  x |= x >> 2;
  x |= x >> 1;
  return __popc(x & 0x01010101u);
}

// One work-group per (group, T x T tile of pairs with tile column >= tile row), T = 16 * TB; thread (ty, tx) owns the TB x TB pairs
// (I0 + ty*TB + a, J0 + tx*TB + b).  Panels in LDS as [point][xyz][design]: the I read is one address per ty (a broadcast over the 16 tx
// lanes), the J read is 16 consecutive TB-vectors - both conflict-free.  The finished tile goes through LDS so that the tile and its
// mirror are both written as whole rows.  A pair (i, j) is computed once, by the thread with j > i, and stored twice.
template <int TB, bool kAligned>
__global__ void __launch_bounds__(256)
metrics_pair_tile_kernel(PairWorkspace ws, int N, int K, int P, int tiles, float* __restrict__ rmsd, float* __restrict__ identity) {
  constexpr int T = 16 * TB;
  constexpr int kPanel = kPointChunk * 3 * T, kTokens = kWordChunk * T, kOut = T * (T + 1);
  constexpr int kWords = 2 * (kPanel > kTokens ? (kPanel > kOut ? kPanel : kOut) : (kTokens > kOut ? kTokens : kOut));
  __shared__ __align__(16) uint32_t s_buf[kWords];
  using VF = typename Lanes<TB>::F;
  using VU = typename Lanes<TB>::U;

  const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
  const int per_group = tiles * (tiles + 1) / 2;
  const int64_t g = blockIdx.x / per_group;
  int t = blockIdx.x % per_group, ti = 0;
  while (t >= tiles - ti) {
    t -= tiles - ti;
    ++ti;
  }
  const int tj = ti + t;
  const int I0 = ti * T, J0 = tj * T;
  const int n = ws.cnt[g], m = n * P;
  const float* pts = ws.pts + g * (static_cast<int64_t>(K) * P * 3) * N;
  const uint32_t* tok = ws.tok + g * ((K + 3) / 4) * N;

  float acc[TB][TB];
  double h[kAligned ? TB : 1][kAligned ? TB : 1][9];
  double ci[TB][3], cj[TB][3];
  uint32_t differ[TB][TB];
#pragma unroll
  for (int a = 0; a < TB; ++a)
#pragma unroll
    for (int b = 0; b < TB; ++b) {
      acc[a][b] = 0.f;
      differ[a][b] = 0u;
      if constexpr (kAligned) {
#pragma unroll
        for (int e = 0; e < 9; ++e) h[a][b][e] = 0.0;
      }
    }
  if constexpr (kAligned) {
#pragma unroll
    for (int a = 0; a < TB; ++a) {
      const int i = I0 + ty * TB + a, j = J0 + tx * TB + a;
#pragma unroll
      for (int x = 0; x < 3; ++x) {
        ci[a][x] = i < N ? ws.cen[(g * N + i) * 4 + x] : 0.0;
        cj[a][x] = j < N ? ws.cen[(g * N + j) * 4 + x] : 0.0;
      }
    }
  }

  // ---- coordinates
  float* sI = reinterpret_cast<float*>(s_buf);
  float* sJ = sI + kPanel;
  for (int p0 = 0; p0 < m; p0 += kPointChunk) {
    const int np = min(kPointChunk, m - p0);
    __syncthreads();
    for (int e = tid; e < 2 * np * 3 * T; e += 256) {
      const int panel = e / (np * 3 * T), rem = e - panel * (np * 3 * T);
      const int line = rem / T, d = rem - line * T;  // line = point * 3 + xyz
      const int design = (panel ? J0 : I0) + d;
      (panel ? sJ : sI)[line * T + d] = design < N ? pts[static_cast<int64_t>(p0 * 3 + line) * N + design] : 0.f;
    }
    __syncthreads();
    for (int c = 0; c < np; ++c) {
      float pi[3][TB], pj[3][TB];
#pragma unroll
      for (int x = 0; x < 3; ++x) {
        *reinterpret_cast<VF*>(pi[x]) = *reinterpret_cast<const VF*>(sI + (c * 3 + x) * T + ty * TB);
        *reinterpret_cast<VF*>(pj[x]) = *reinterpret_cast<const VF*>(sJ + (c * 3 + x) * T + tx * TB);
      }
      if constexpr (kAligned) {
        double di[TB][3], dj[TB][3];
#pragma unroll
        for (int a = 0; a < TB; ++a)
#pragma unroll
          for (int x = 0; x < 3; ++x) {
            di[a][x] = static_cast<double>(pi[x][a]) - ci[a][x];
            dj[a][x] = static_cast<double>(pj[x][a]) - cj[a][x];
          }
#pragma unroll
        for (int a = 0; a < TB; ++a)
#pragma unroll
          for (int b = 0; b < TB; ++b)
#pragma unroll
            for (int x = 0; x < 3; ++x)
#pragma unroll
              for (int y = 0; y < 3; ++y) h[a][b][3 * x + y] = fma(di[a][x], dj[b][y], h[a][b][3 * x + y]);
      } else {
#pragma unroll
        for (int a = 0; a < TB; ++a)
#pragma unroll
          for (int b = 0; b < TB; ++b) {
            const float dx = pi[0][a] - pj[0][b], dy = pi[1][a] - pj[1][b], dz = pi[2][a] - pj[2][b];
            acc[a][b] = ((acc[a][b] + dx * dx) + dy * dy) + dz * dz;
          }
      }
    }
  }

  // ---- tokens
  uint32_t* wI = s_buf;
  uint32_t* wJ = wI + kTokens;
  const int words = (n + 3) / 4;
  for (int w0 = 0; w0 < words; w0 += kWordChunk) {
    const int nw = min(kWordChunk, words - w0);
    __syncthreads();
    for (int e = tid; e < 2 * nw * T; e += 256) {
      const int panel = e / (nw * T), rem = e - panel * (nw * T);
      const int line = rem / T, d = rem - line * T;
      const int design = (panel ? J0 : I0) + d;
      (panel ? wJ : wI)[line * T + d] = design < N ? tok[static_cast<int64_t>(w0 + line) * N + design] : 0u;
    }
    __syncthreads();
    for (int w = 0; w < nw; ++w) {
      uint32_t ui[TB], uj[TB];
      *reinterpret_cast<VU*>(ui) = *reinterpret_cast<const VU*>(wI + w * T + ty * TB);
      *reinterpret_cast<VU*>(uj) = *reinterpret_cast<const VU*>(wJ + w * T + tx * TB);
#pragma unroll
      for (int a = 0; a < TB; ++a)
#pragma unroll
        for (int b = 0; b < TB; ++b) differ[a][b] += differing_bytes(ui[a] ^ uj[b]);
    }
  }

  // ---- the tile, through LDS
  float* sD = reinterpret_cast<float*>(s_buf);
  float* sQ = sD + kOut;
  __syncthreads();
#pragma unroll
  for (int a = 0; a < TB; ++a)
#pragma unroll
    for (int b = 0; b < TB; ++b) {
      const int i = I0 + ty * TB + a, j = J0 + tx * TB + b;
      float r = NAN, q = NAN;
      if (n > 0 && i < N && j < N) {
        if constexpr (kAligned) {
          const double spread = ws.cen[(g * N + i) * 4 + 3] + ws.cen[(g * N + j) * 4 + 3];
          r = static_cast<float>(sqrt(kabsch_msd(h[a][b], spread, static_cast<double>(m))));
        } else {
          r = sqrtf(acc[a][b] / static_cast<float>(m));
        }
        q = static_cast<float>(n - static_cast<int>(differ[a][b])) / static_cast<float>(n);
      }
      sD[(ty * TB + a) * (T + 1) + tx * TB + b] = r;
      sQ[(ty * TB + a) * (T + 1) + tx * TB + b] = q;
    }
  __syncthreads();
  float* out_r = rmsd + g * N * N;
  float* out_q = identity + g * N * N;
  const float diag_r = n > 0 ? 0.f : NAN, diag_q = n > 0 ? 1.f : NAN;
  for (int e = tid; e < T * T; e += 256) {
    const int r = e / T, c = e - r * T;
    const int i = I0 + r, j = J0 + c;
    if (i >= N || j >= N) continue;
    float vr, vq;
    if (ti != tj || r != c) {
      const int lo = (ti != tj || r < c) ? r : c, hi = (ti != tj || r < c) ? c : r;  // a diagonal tile reads its upper half for both
      vr = sD[lo * (T + 1) + hi];
      vq = sQ[lo * (T + 1) + hi];
    } else {
      vr = diag_r;
      vq = diag_q;
    }
    out_r[static_cast<int64_t>(i) * N + j] = vr;
    out_q[static_cast<int64_t>(i) * N + j] = vq;
  }
  if (ti != tj) {
    for (int e = tid; e < T * T; e += 256) {
      const int c = e / T, r = e - c * T;  // lanes along i: the mirror's rows are whole lines too
      const int i = I0 + r, j = J0 + c;
      if (i >= N || j >= N) continue;
      out_r[static_cast<int64_t>(j) * N + i] = sD[r * (T + 1) + c];
      out_q[static_cast<int64_t>(j) * N + i] = sQ[r * (T + 1) + c];
    }
  }
}

// ------------------------------------------------------------------ 3. greedy farthest-point selection
constexpr int kPickThreads = 1024;
constexpr int kPickPerThread = kMaxGroup / kPickThreads;
constexpr int kNone = INT_MAX;

struct Best {
  float v;
  int i;
};

__device__ inline Best better(Best a, Best b) {  // the larger value; ties to the lower index; kNone loses to anything
  if (b.i == kNone) return a;
  if (a.i == kNone) return b;
  if (b.v > a.v || (b.v == a.v && b.i < a.i)) return b;
  return a;
}

__device__ inline float nan_to(float v, float r) { return v != v ? r : v; }

__global__ void __launch_bounds__(kPickThreads)
metrics_select_kernel(const float* __restrict__ dist, const float* __restrict__ score, const uint8_t* __restrict__ candidates, int N, int m,
                      int64_t* __restrict__ index, float* __restrict__ min_dist, int32_t* __restrict__ count) {
  __shared__ Best s_part[kPickThreads / 64];
  __shared__ Best s_pick;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t g = blockIdx.x;
  const float* D = dist + g * N * N;
  float run[kPickPerThread];
  bool open[kPickPerThread];
#pragma unroll
  for (int r = 0; r < kPickPerThread; ++r) {
    const int c = tid + r * kPickThreads;
    run[r] = INFINITY;
    open[r] = c < N && (candidates == nullptr || candidates[g * N + c] != 0);
  }
  int picked = 0;
  for (; picked < m; ++picked) {
    Best mine{0.f, kNone};
#pragma unroll
    for (int r = 0; r < kPickPerThread; ++r) {
      const int c = tid + r * kPickThreads;
      if (!open[r]) continue;
      // the first pick: the lowest score (a NaN score counts as +inf), or the first candidate
      const float key = picked > 0 ? run[r] : (score ? -nan_to(score[g * N + c], INFINITY) : 0.f);
      mine = better(mine, Best{key, c});
    }
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) mine = better(mine, Best{__shfl_xor(mine.v, d, 64), __shfl_xor(mine.i, d, 64)});
    if (lane == 0) s_part[wave] = mine;
    __syncthreads();
    if (tid == 0) {
      Best b = s_part[0];
      for (int w = 1; w < kPickThreads / 64; ++w) b = better(b, s_part[w]);
      s_pick = b;
    }
    __syncthreads();
    const Best pick = s_pick;
    if (pick.i == kNone) break;  // (uniform)
    if (tid == 0) {
      index[g * m + picked] = pick.i;
      min_dist[g * m + picked] = picked > 0 ? pick.v : INFINITY;
    }
#pragma unroll
    for (int r = 0; r < kPickPerThread; ++r) {
      const int c = tid + r * kPickThreads;
      if (c == pick.i) open[r] = false;
      if (open[r]) run[r] = fminf(run[r], nan_to(D[static_cast<int64_t>(pick.i) * N + c], 0.f));
    }
  }
  for (int p = picked + tid; p < m; p += kPickThreads) {
    index[g * m + p] = -1;
    min_dist[g * m + p] = NAN;
  }
  if (tid == 0) count[g] = picked;
}

bool shape_ok(const char* who, int64_t rows_or_G, int32_t N, int32_t K, int32_t P) {
  if (rows_or_G < 0 || N < 1 || K < 1) {
    set_error("%s: negative or empty extent (%lld rows or groups, group size %d, K = %d)", who, static_cast<long long>(rows_or_G), N, K);
    return false;
  }
  if (P < 1 || P > kMaxPoints) {
    set_error("%s: P = %d points per residue outside [1, %d]", who, P, kMaxPoints);
    return false;
  }
  if (N > kMaxGroup) {
    set_error("%s: group size N = %d, at most %d designs per group", who, N, kMaxGroup);
    return false;
  }
  if (K > kMaxK) {
    set_error("%s: K = %d residues per patch, at most %d", who, K, kMaxK);
    return false;
  }
  return true;
}

}  // namespace
}  // namespace diffab

using namespace diffab;

extern "C" {

int diffab_metrics_vs_native(const int64_t* seq_idx, const float* points, const int64_t* native_seq_idx, const float* native_points,
                             const uint8_t* generation_mask, const uint8_t* residue_mask, const int64_t* segment_idx, int32_t rows,
                             int32_t group_size, int32_t K, int32_t P, int32_t S, float* aar, float* rmsd, float* rmsd_aligned, float* segment_aar,
                             float* segment_rmsd, float* segment_rmsd_aligned, void* stream) {
  StreamOrder order_(stream);
  if (!shape_ok("metrics_vs_native", rows, group_size, K, P)) return DIFFAB_ERR_ARG;
  DIFFAB_REQUIRE(rows % group_size == 0, DIFFAB_ERR_ARG, "metrics_vs_native: %d rows are not a multiple of group_size = %d", rows, group_size);
  DIFFAB_REQUIRE(S >= 0 && S <= kMaxSegments, DIFFAB_ERR_ARG, "metrics_vs_native: S = %d segments outside [0, %d]", S, kMaxSegments);
  DIFFAB_REQUIRE((S > 0) == (segment_idx != nullptr), DIFFAB_ERR_ARG, "metrics_vs_native: S = %d %s segment_idx", S,
                 S > 0 ? "needs a" : "goes with a NULL");
  if (rows == 0) return DIFFAB_OK;
  DIFFAB_REQUIRE(seq_idx && points && native_seq_idx && native_points && generation_mask, DIFFAB_ERR_ARG, "metrics_vs_native: null input");
  DIFFAB_REQUIRE(aar && rmsd && rmsd_aligned, DIFFAB_ERR_ARG, "metrics_vs_native: null output");
  DIFFAB_REQUIRE(S == 0 || (segment_aar && segment_rmsd && segment_rmsd_aligned), DIFFAB_ERR_ARG, "metrics_vs_native: null segment output");
  hipLaunchKernelGGL(metrics_vs_native_kernel, dim3(rows), dim3(64), 0, as_stream(stream), seq_idx, points, native_seq_idx, native_points,
                     generation_mask, residue_mask, segment_idx, group_size, K, P, S, aar, rmsd, rmsd_aligned, segment_aar, segment_rmsd,
                     segment_rmsd_aligned);
  DIFFAB_LAUNCH_CHECK();
  return DIFFAB_OK;
}

int diffab_metrics_pairwise(const int64_t* seq_idx, const float* points, const uint8_t* generation_mask, const uint8_t* residue_mask, int32_t G,
                            int32_t N, int32_t K, int32_t P, int32_t aligned, float* rmsd, float* seq_identity, void* workspace,
                            size_t workspace_bytes, void* stream) {
  StreamOrder order_(stream);
  if (!shape_ok("metrics_pairwise", G, N, K, P)) return DIFFAB_ERR_ARG;
  DIFFAB_REQUIRE(aligned == 0 || aligned == 1, DIFFAB_ERR_ARG, "metrics_pairwise: aligned must be 0 or 1, got %d", aligned);
  if (G == 0) return DIFFAB_OK;
  DIFFAB_REQUIRE(seq_idx && points && generation_mask, DIFFAB_ERR_ARG, "metrics_pairwise: null input");
  DIFFAB_REQUIRE(rmsd && seq_identity, DIFFAB_ERR_ARG, "metrics_pairwise: null output");
  const PairWorkspace ws = carve_pairs(workspace, G, N, K, P);
  if (const int e = workspace_ok("metrics_pairwise", workspace, 16, workspace_bytes, ws.bytes)) return e;
  const int T = aligned ? 32 : 64;
  const int64_t tiles = (N + T - 1) / T;
  const int64_t grid = static_cast<int64_t>(G) * (tiles * (tiles + 1) / 2), pack_grid = static_cast<int64_t>(G) * ((N + 63) / 64);
  DIFFAB_REQUIRE(grid <= INT_MAX && pack_grid <= INT_MAX, DIFFAB_ERR_UNSUPPORTED, "metrics_pairwise: G = %d groups of N = %d are more tiles than one launch holds", G, N);
  hipStream_t st = as_stream(stream);
  hipLaunchKernelGGL(metrics_pack_kernel, dim3(static_cast<unsigned>(pack_grid)), dim3(256), 0, st, seq_idx, points, generation_mask, residue_mask,
                     N, K, P, aligned, ws);
  if (aligned)
    hipLaunchKernelGGL((metrics_pair_tile_kernel<2, true>), dim3(static_cast<unsigned>(grid)), dim3(256), 0, st, ws, N, K, P,
                       static_cast<int>(tiles), rmsd, seq_identity);
  else
    hipLaunchKernelGGL((metrics_pair_tile_kernel<4, false>), dim3(static_cast<unsigned>(grid)), dim3(256), 0, st, ws, N, K, P,
                       static_cast<int>(tiles), rmsd, seq_identity);
  DIFFAB_LAUNCH_CHECK();
  return DIFFAB_OK;
}

int diffab_metrics_select_diverse(const float* dist, const float* score, const uint8_t* candidates, int32_t G, int32_t N, int32_t m,
                                  int64_t* index, float* min_dist, int32_t* count, void* stream) {
  StreamOrder order_(stream);
  DIFFAB_REQUIRE(G >= 0 && N >= 1, DIFFAB_ERR_ARG, "metrics_select_diverse: negative or empty extent (G = %d, N = %d)", G, N);
  DIFFAB_REQUIRE(m >= 0, DIFFAB_ERR_ARG, "metrics_select_diverse: m must be >= 0, got %d", m);
  DIFFAB_REQUIRE(N <= kMaxGroup, DIFFAB_ERR_ARG, "metrics_select_diverse: N = %d, at most %d designs per group", N, kMaxGroup);
  if (G == 0) return DIFFAB_OK;
  DIFFAB_REQUIRE(dist != nullptr, DIFFAB_ERR_ARG, "metrics_select_diverse: null dist");
  DIFFAB_REQUIRE(count && (m == 0 || (index && min_dist)), DIFFAB_ERR_ARG, "metrics_select_diverse: null output");
  hipLaunchKernelGGL(metrics_select_kernel, dim3(G), dim3(kPickThreads), 0, as_stream(stream), dist, score, candidates, N, m, index, min_dist,
                     count);
  DIFFAB_LAUNCH_CHECK();
  return DIFFAB_OK;
}

}  // extern "C"
