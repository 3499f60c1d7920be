// hbond_kernels.hip - backbone hydrogen bonds and secondary structure of every design row on the device:
// diffab_metrics_hbonds, the Kabsch-Sander electrostatic bond and the states built on it.  The rule is the header comment of the entry in
// include/diffab_hip_hbonds.h.
//
// Built with -ffp-contract=off (csrc/Makefile): the derived atoms (O, H) are fp64 expressions of the fp32 inputs in a written order,
// rounded once; the CA cull is dist2 of analysis_common.h; the bond energy is fp64 from the fp32 atoms and "bonded" is a strict
// comparison on it.  fp64 + - * / sqrt are correctly rounded, so every bit of the K x K bond matrix is a defined number, and everything
// after it is integer work on that matrix in LDS.  VALU + LDS only; the only atomics are integer ones on LDS; every value reaches memory
// through plain C++ stores.
#include <climits>
#include <cmath>

#include "../../include/diffab_hip_hbonds.h"
#include "analysis_prep.h"

namespace diffab {
namespace {

constexpr int kMaxK = DIFFAB_HBONDS_MAX_K;
constexpr int kMaxGroup = DIFFAB_METRICS_MAX_GROUP;
constexpr int kMaxContextAtoms = DIFFAB_METRICS_MAX_CONTEXT_ATOMS;
constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr double kCoupling = 27.888;     // 0.42 e * 0.20 e * 332 kcal A / mol
constexpr double kBonded = -0.5;         // kcal / mol
constexpr double kMinDistance = 0.5;     // Angstrom
constexpr double kCarbonyl = 1.231;      // |C - O|
constexpr double kCos70 = 0.3420201433256687;
constexpr float kCull2 = 81.0f;          // CA - CA, 9 Angstrom

// what is known of residue k (s_flags)
enum : uint32_t {
  fIn = 1u,         // inside residue_mask
  fGen = 2u,        // generated
  fBackbone = 4u,   // complete: N, CA, C
  fO = 8u,
  fH = 16u,
  fRealO = 32u,     // O is the context's own atom
  fDonorOff = 64u,
  fDepO = 128u,     // the acceptor side of the residue depends on the design row
  fDepD = 256u,     // the donor side does
  fAntigen = 512u,
  fHotspot = 1024u,
  fLinked = 2048u,  // has a predecessor and a successor
};
// what the secondary-structure passes find (s_state): the seven states in priority order, then the turns and the hotspot mark
enum : uint32_t { sH = 1u, sB = 2u, sE = 4u, sG = 8u, sI = 16u, sT = 32u, sS = 64u, sTurn3 = 256u, sTurn4 = 512u, sTurn5 = 1024u, sBonded = 2048u };
enum { aN = 0, aCA = 1, aC = 2, aO = 3, aH = 4 };
enum { rBonds = 0, rInternal, rAntigen, rFramework, rHotBonded, rHot, rCount, rEnd = rCount + 8 };

// Workspace of diffab_metrics_hbonds (DIFFAB_METRICS_HBONDS_WORKSPACE_BYTES covers the carves and their alignment).
struct HbondWorkspace {
  int32_t* succ;   // (G, K)
  int32_t* pred;   // (G, K)
  uint32_t* bits;  // (G, K, W): the bonds of the pairs that do not depend on the row
  size_t bytes;
};

HbondWorkspace carve_hbonds(void* base, int64_t G, int64_t K) {
  Carver c(base);
  HbondWorkspace w;
  const int64_t W = (K + 31) / 32;
  w.succ = c.take<int32_t>(static_cast<size_t>(G * K));
  w.pred = c.take<int32_t>(static_cast<size_t>(G * K));
  w.bits = c.take<uint32_t>(static_cast<size_t>(G * K * W));
  w.bytes = c.bytes();
  return w;
}

struct HbondIn {
  const float* points;              // (rows, K, 3, 3)
  const uint8_t* donor_off;         // (rows, K)
  const float* ctx_points;          // (G, K, A, 3)
  const uint32_t* ctx_valid;        // (G, K)
  const uint8_t* ctx_donor_off;     // (G, K)
  const uint8_t *generation_mask, *residue_mask, *antigen_mask, *hotspot_mask;
  const int32_t *chain, *residue_idx;
};

struct HbondOut {
  float *O, *H;                                 // (rows, K, 3)
  int32_t* nh_o_partner;                        // (rows, K, 2)
  float* nh_o_energy;
  int32_t* o_hn_partner;
  float* o_hn_energy;
  int32_t* bridge_partner;
  uint8_t* bridge_parallel;
  uint8_t* ss;                                  // (rows, K)
  int32_t* residue_hbonds;
  int32_t *n_hbonds, *n_internal, *n_antigen, *n_framework, *n_hotspot_bonded, *n_hotspot;  // (rows)
  float* energy;
  int32_t* ss_count;                            // (rows, 8)
};

// The dynamic LDS of both kernels: 4-byte words throughout.
struct Lds {
  float* xyz;        // [5][K][3]: N, CA, C, O, H
  uint32_t* flags;   // [K]
  int* succ;         // [K]
  int* pred;         // [K]
  uint32_t* state;   // [K]
  int* red;          // [rEnd]
  uint32_t* bits;    // [K][W]
};
constexpr size_t lds_words(int K, int W, bool with_bits) {
  return static_cast<size_t>(K) * 19 + 32 + (with_bits ? static_cast<size_t>(K) * W : 0);
}
__device__ inline Lds carve_lds(unsigned char* smem, int K) {
  Lds l;
  l.xyz = reinterpret_cast<float*>(smem);
  l.flags = reinterpret_cast<uint32_t*>(l.xyz + 15 * K);
  l.succ = reinterpret_cast<int*>(l.flags + K);
  l.pred = l.succ + K;
  l.state = reinterpret_cast<uint32_t*>(l.pred + K);
  l.red = reinterpret_cast<int*>(l.state + K);
  l.bits = reinterpret_cast<uint32_t*>(l.red + 32);
  return l;
}

__device__ inline float* atom(const Lds& l, int K, int which, int k) { return l.xyz + (which * K + k) * 3; }

__device__ inline void load3(const float* p, double (&v)[3]) {
  v[0] = static_cast<double>(p[0]), v[1] = static_cast<double>(p[1]), v[2] = static_cast<double>(p[2]);
}
__device__ inline double dot3(const double (&u)[3], const double (&v)[3]) { return (u[0] * v[0] + u[1] * v[1]) + u[2] * v[2]; }
// v / |v| component by component; false where |v| = 0
__device__ inline bool unit3(const double (&v)[3], double (&u)[3]) {
  const double len = sqrt(dot3(v, v));
  if (!(len > 0.0)) return false;
  u[0] = v[0] / len, u[1] = v[1] / len, u[2] = v[2] / len;
  return true;
}
__device__ inline double distance(const float* p, const float* q) {
  const double dx = static_cast<double>(p[0]) - static_cast<double>(q[0]);
  const double dy = static_cast<double>(p[1]) - static_cast<double>(q[1]);
  const double dz = static_cast<double>(p[2]) - static_cast<double>(q[2]);
  return fmax(sqrt((dx * dx + dy * dy) + dz * dz), kMinDistance);
}

// The atoms of every residue into LDS.  `pp` / `don` are the design row's points and donor_off, or null for the patch alone: then a
// generated residue has no atoms, and what is derived next to one is wrong and marked as depending on the row.  succ / pred are in LDS.
__device__ void stage_atoms(const Lds& l, const HbondIn& in, const float* pp, const uint8_t* don, int64_t g, int K, int A, int tid) {
  const int64_t base = g * K;
  for (int k = tid; k < K; k += kThreads) {
    uint32_t f = 0;
    const bool inside = in.residue_mask == nullptr || in.residue_mask[base + k] != 0;
    if (inside) {
      f |= fIn;
      const float* src = nullptr;
      if (in.generation_mask[base + k] != 0) {
        f |= fGen;
        if (pp != nullptr) {
          src = pp + k * 9;
          if (don[k] != 0) f |= fDonorOff;
        }
      } else {
        const uint32_t bits = in.ctx_valid[base + k];
        if (in.ctx_donor_off[base + k] != 0) f |= fDonorOff;
        if ((bits & 7u) == 7u) {
          src = in.ctx_points + (base + k) * A * 3;
          if ((bits & 8u) != 0u) {
            f |= fO | fRealO;
            float* o = atom(l, K, aO, k);
            o[0] = src[9], o[1] = src[10], o[2] = src[11];
          }
        }
        if (in.antigen_mask != nullptr && in.antigen_mask[base + k] != 0) {
          f |= fAntigen;
          if (in.hotspot_mask != nullptr && in.hotspot_mask[base + k] != 0) f |= fHotspot;
        }
      }
      if (src != nullptr) {
        f |= fBackbone;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
          float* d = atom(l, K, a, k);
          d[0] = src[a * 3], d[1] = src[a * 3 + 1], d[2] = src[a * 3 + 2];
        }
      }
      if (l.succ[k] >= 0 && l.pred[k] >= 0) f |= fLinked;
    }
    l.flags[k] = f;
    l.state[k] = 0;
  }
  __syncthreads();
  // O where the context has none
  for (int k = tid; k < K; k += kThreads) {
    uint32_t f = l.flags[k];
    const int s = l.succ[k];
    const uint32_t fs = s >= 0 ? l.flags[s] : 0u;
    if ((f & fGen) != 0u || ((f & fRealO) == 0u && (fs & fGen) != 0u)) f |= fDepO;
    if ((f & fBackbone) != 0u && (f & fO) == 0u) {
      double n[3], ca[3], c[3], o[3];
      load3(atom(l, K, aN, k), n);
      load3(atom(l, K, aCA, k), ca);
      load3(atom(l, K, aC, k), c);
      bool ok;
      if ((fs & fBackbone) != 0u) {
        double ns[3], u1[3], u2[3], ub[3];
        load3(atom(l, K, aN, s), ns);
        const double v1[3] = {ca[0] - c[0], ca[1] - c[1], ca[2] - c[2]};
        const double v2[3] = {ns[0] - c[0], ns[1] - c[1], ns[2] - c[2]};
        ok = unit3(v1, u1) && unit3(v2, u2);
        if (ok) {
          const double b[3] = {u1[0] + u2[0], u1[1] + u2[1], u1[2] + u2[2]};
          ok = unit3(b, ub);
          if (ok) o[0] = c[0] - kCarbonyl * ub[0], o[1] = c[1] - kCarbonyl * ub[1], o[2] = c[2] - kCarbonyl * ub[2];
        }
      } else {
        double e1[3], e2[3];
        const double v1[3] = {c[0] - ca[0], c[1] - ca[1], c[2] - ca[2]};
        const double v[3] = {n[0] - ca[0], n[1] - ca[1], n[2] - ca[2]};
        ok = unit3(v1, e1);
        if (ok) {
          const double t = dot3(v, e1);
          const double w[3] = {v[0] - t * e1[0], v[1] - t * e1[1], v[2] - t * e1[2]};
          ok = unit3(w, e2);
          if (ok) {
#pragma unroll
            for (int x = 0; x < 3; ++x) o[x] = (ca[x] + 2.153 * e1[x]) - 1.062 * e2[x];
          }
        }
      }
      if (ok) {
        float* d = atom(l, K, aO, k);
        d[0] = static_cast<float>(o[0]), d[1] = static_cast<float>(o[1]), d[2] = static_cast<float>(o[2]);
        f |= fO;
      }
    }
    l.flags[k] = f;
  }
  __syncthreads();
  // H from the predecessor's C and O
  for (int k = tid; k < K; k += kThreads) {
    uint32_t f = l.flags[k];
    const int p = l.pred[k];
    const uint32_t fp = p >= 0 ? l.flags[p] : 0u;
    if ((f & fGen) != 0u || (fp & fDepO) != 0u) f |= fDepD;
    if ((f & fBackbone) != 0u && (f & fDonorOff) == 0u && (fp & (fBackbone | fO)) == (fBackbone | fO)) {
      double n[3], cp[3], op[3], u[3];
      load3(atom(l, K, aN, k), n);
      load3(atom(l, K, aC, p), cp);
      load3(atom(l, K, aO, p), op);
      const double v[3] = {cp[0] - op[0], cp[1] - op[1], cp[2] - op[2]};
      if (unit3(v, u)) {
        float* d = atom(l, K, aH, k);
        d[0] = static_cast<float>(n[0] + u[0]), d[1] = static_cast<float>(n[1] + u[1]), d[2] = static_cast<float>(n[2] + u[2]);
        f |= fH;
      }
    }
    l.flags[k] = f;  // (fDepD and fH of k are read by nobody in this loop)
  }
  __syncthreads();
}

// The Kabsch-Sander energy of acceptor a (C, O) and donor d (N, H), both with their atoms; false when the CA cull removes the pair.
__device__ inline bool pair_energy(const Lds& l, int K, int a, int d, double& E) {
  const float* ca = atom(l, K, aCA, a);
  const float* cd = atom(l, K, aCA, d);
  if (!(dist2(ca[0], ca[1], ca[2], cd[0], cd[1], cd[2]) < kCull2)) return false;
  const float *o = atom(l, K, aO, a), *c = atom(l, K, aC, a), *n = atom(l, K, aN, d), *h = atom(l, K, aH, d);
  const double r_on = distance(o, n), r_ch = distance(c, h), r_oh = distance(o, h), r_cn = distance(c, n);
  E = kCoupling * (((1.0 / r_on + 1.0 / r_ch) - 1.0 / r_oh) - 1.0 / r_cn);
  return true;
}

__device__ inline bool bonded(const Lds& l, int K, int a, int d, uint32_t fa, uint32_t fd) {
  if ((fa & (fBackbone | fO)) != (fBackbone | fO) || (fd & (fBackbone | fH)) != (fBackbone | fH)) return false;
  if (d == a || d == l.succ[a]) return false;
  double E;
  return pair_energy(l, K, a, d, E) && E < kBonded;
}

// One wave per acceptor, lane = donor in passes of 64.  kRow = false: the pairs neither end of which depends on the row, to `out`
// (the workspace).  kRow = true: the pairs of which one does, OR-ed into `out` (LDS, holding the patch's bits).
template <bool kRow>
__device__ void fill_bits(const Lds& l, int K, int W, uint32_t* out, int tid) {
  const int lane = tid & 63, wave = tid >> 6;
  for (int a = wave; a < K; a += kWaves) {
    const uint32_t fa = l.flags[a];
    const bool dep_a = (fa & fDepO) != 0u;
    const bool a_ok = (fa & (fBackbone | fO)) == (fBackbone | fO);
    for (int d0 = 0; d0 < K; d0 += 64) {
      const int d = d0 + lane;
      const uint32_t fd = d < K ? l.flags[d] : 0u;
      const bool dep = dep_a || (fd & fDepD) != 0u;
      const bool mine = d < K && dep == kRow;
      if (kRow && (!a_ok || __ballot(mine) == 0ull)) continue;  // (uniform)
      const bool bit = mine && a_ok && bonded(l, K, a, d, fa, fd);
      const unsigned long long m = __ballot(bit);
      if (lane == 0) {
        const int w = d0 >> 5;
        const uint32_t lo = static_cast<uint32_t>(m), hi = static_cast<uint32_t>(m >> 32);
        if (kRow) {
          if (lo != 0u) out[a * W + w] |= lo;
          if (hi != 0u) out[a * W + w + 1] |= hi;  // (a set bit of hi is a donor below K: the word exists)
        } else {
          out[a * W + w] = lo;
          if (w + 1 < W) out[a * W + w + 1] = hi;
        }
      }
    }
  }
}

// ------------------------------------------------------------------ 1. per patch
__global__ void __launch_bounds__(kThreads)
hbonds_patch_kernel(HbondIn in, int K, int A, HbondWorkspace ws) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const Lds l = carve_lds(smem, K);
  const int tid = threadIdx.x;
  const int64_t g = blockIdx.x, base = g * K;
  const int W = (K + 31) / 32;
  // the keys of the chain rule, borrowed from the atoms' space
  int2* key = reinterpret_cast<int2*>(l.xyz);
  uint8_t* key_in = reinterpret_cast<uint8_t*>(key + K);
  stage_chain_keys<kThreads>(in.chain, in.residue_idx, in.residue_mask, base, K, key, key_in);
  __syncthreads();
  for (int k = tid; k < K; k += kThreads) {
    const ChainLinks links = chain_links(key, key_in, K, k);
    l.succ[k] = links.succ, l.pred[k] = links.pred;
    ws.succ[base + k] = links.succ, ws.pred[base + k] = links.pred;
  }
  __syncthreads();
  stage_atoms(l, in, nullptr, nullptr, g, K, A, tid);
  fill_bits<false>(l, K, W, ws.bits + base * W, tid);
}

// ------------------------------------------------------------------ 2. per design row
struct Best2 {
  int j0 = -1, j1 = -1;
  double e0 = 0.0, e1 = 0.0;
  __device__ void add(int j, double e) {  // candidates arrive in ascending slot order: a tie keeps the earlier one
    if (j0 < 0 || e < e0) {
      j1 = j0, e1 = e0, j0 = j, e0 = e;
    } else if (j1 < 0 || e < e1) {
      j1 = j, e1 = e;
    }
  }
};

__device__ inline bool hb(const Lds& l, int W, int a, int d) {
  return a >= 0 && d >= 0 && ((l.bits[a * W + (d >> 5)] >> (d & 31)) & 1u) != 0u;
}
__device__ inline int step(const Lds& l, int k, int n) {  // s^n(k), -1 where a step is missing
  for (int i = 0; i < n && k >= 0; ++i) k = l.succ[k];
  return k;
}
__device__ inline bool apart(const Lds& l, int i, int j) {
  const int si = l.succ[i], sj = l.succ[j];
  return j != i && j != si && j != l.succ[si] && i != sj && i != l.succ[sj];
}
// bit 0: parallel(i, j), bit 1: antiparallel(i, j); i, j any slots or -1
__device__ inline int bridge(const Lds& l, int W, int i, int j) {
  if (i < 0 || j < 0 || (l.flags[i] & fLinked) == 0u || (l.flags[j] & fLinked) == 0u || !apart(l, i, j)) return 0;
  const int pi = l.pred[i], si = l.succ[i], pj = l.pred[j], sj = l.succ[j];
  const bool par = (hb(l, W, pi, j) && hb(l, W, j, si)) || (hb(l, W, pj, i) && hb(l, W, i, sj));
  const bool anti = (hb(l, W, i, j) && hb(l, W, j, i)) || (hb(l, W, pi, sj) && hb(l, W, pj, si));
  return (par ? 1 : 0) | (anti ? 2 : 0);
}

__global__ void __launch_bounds__(kThreads)
hbonds_rows_kernel(HbondIn in, int group_size, int K, int A, HbondWorkspace ws, HbondOut out) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const Lds l = carve_lds(smem, K);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t row = blockIdx.x;
  const int64_t g = row / group_size, base = g * K;
  const int W = (K + 31) / 32;

  for (int k = tid; k < K; k += kThreads) l.succ[k] = ws.succ[base + k], l.pred[k] = ws.pred[base + k];
  for (int i = tid; i < K * W; i += kThreads) l.bits[i] = ws.bits[base * W + i];
  if (tid < rEnd) l.red[tid] = 0;
  __syncthreads();
  stage_atoms(l, in, in.points + row * K * 9, in.donor_off + row * K, g, K, A, tid);
  fill_bits<true>(l, K, W, l.bits, tid);
  __syncthreads();

  // ---- wave 0: the energy of the row in (acceptor, donor) order.  The other waves: partners, energies and bond counts per residue.
  if (wave == 0) {
    double sum = 0.0;
    for (int a = 0; a < K; ++a) {
      const bool gen_a = (l.flags[a] & fGen) != 0u;
      for (int d0 = 0; d0 < K; d0 += 64) {
        const int d = d0 + lane;
        double E = 0.0;
        bool take = d < K && hb(l, W, a, d) && (gen_a || (l.flags[d] & fGen) != 0u);
        if (take) pair_energy(l, K, a, d, E);
        unsigned long long m = __ballot(take);
        while (m != 0ull) {
          const int src = __ffsll(static_cast<long long>(m)) - 1;
          m &= m - 1ull;
          sum += __shfl(E, src, 64);
        }
      }
    }
    if (lane == 0 && out.energy != nullptr) out.energy[row] = static_cast<float>(sum);
  } else {
    int n_bonds = 0, n_internal = 0, n_antigen = 0, n_framework = 0;
    for (int k = tid - 64; k < K; k += kThreads - 64) {
      const uint32_t fk = l.flags[k];
      const bool gen_k = (fk & fGen) != 0u;
      Best2 as_acceptor, as_donor;
      int mine = 0;
      for (int w = 0; w < W; ++w) {  // the donors of k's C=O
        uint32_t word = l.bits[k * W + w];
        while (word != 0u) {
          const int d = w * 32 + __ffs(static_cast<int>(word)) - 1;
          word &= word - 1u;
          double E = 0.0;
          pair_energy(l, K, k, d, E);
          as_acceptor.add(d, E);
          const uint32_t fd = l.flags[d];
          const bool gen_d = (fd & fGen) != 0u;
          if (gen_k || gen_d) {  // every bond has one acceptor: counted here
            ++mine, ++n_bonds;
            if (gen_k && gen_d) {
              ++n_internal;
            } else {
              const int other = gen_k ? d : k;
              const uint32_t fo = gen_k ? fd : fk;
              if ((fo & fAntigen) != 0u) ++n_antigen; else ++n_framework;
              if ((fo & fHotspot) != 0u) atomicOr(&l.state[other], sBonded);
            }
          }
        }
      }
      if ((fk & fH) != 0u) {  // the acceptors of k's N-H
        const int w = k >> 5, b = k & 31;
        for (int a = 0; a < K; ++a) {
          if (((l.bits[a * W + w] >> b) & 1u) == 0u) continue;
          double E = 0.0;
          pair_energy(l, K, a, k, E);
          as_donor.add(a, E);
          if (gen_k || (l.flags[a] & fGen) != 0u) ++mine;
        }
      }
      const int64_t e = row * K + k;
      if (out.nh_o_partner) out.nh_o_partner[e * 2] = as_donor.j0, out.nh_o_partner[e * 2 + 1] = as_donor.j1;
      if (out.nh_o_energy) out.nh_o_energy[e * 2] = static_cast<float>(as_donor.e0), out.nh_o_energy[e * 2 + 1] = static_cast<float>(as_donor.e1);
      if (out.o_hn_partner) out.o_hn_partner[e * 2] = as_acceptor.j0, out.o_hn_partner[e * 2 + 1] = as_acceptor.j1;
      if (out.o_hn_energy)
        out.o_hn_energy[e * 2] = static_cast<float>(as_acceptor.e0), out.o_hn_energy[e * 2 + 1] = static_cast<float>(as_acceptor.e1);
      if (out.residue_hbonds) out.residue_hbonds[e] = mine;
#pragma unroll
      for (int x = 0; x < 3; ++x) {
        if (out.O) out.O[e * 3 + x] = (fk & fO) != 0u ? atom(l, K, aO, k)[x] : NAN;
        if (out.H) out.H[e * 3 + x] = (fk & fH) != 0u ? atom(l, K, aH, k)[x] : NAN;
      }
    }
    if (n_bonds != 0) {
      atomicAdd(&l.red[rBonds], n_bonds);
      atomicAdd(&l.red[rInternal], n_internal);
      atomicAdd(&l.red[rAntigen], n_antigen);
      atomicAdd(&l.red[rFramework], n_framework);
    }
  }

  // ---- turns and bends: every residue writes its own word
  for (int k = tid; k < K; k += kThreads) {
    const uint32_t fk = l.flags[k];
    if ((fk & fIn) == 0u) continue;
    uint32_t st = 0;
    if (hb(l, W, k, step(l, k, 3))) st |= sTurn3;
    if (hb(l, W, k, step(l, k, 4))) st |= sTurn4;
    if (hb(l, W, k, step(l, k, 5))) st |= sTurn5;
    const int p = l.pred[k], s = l.succ[k];
    const int pp = p >= 0 ? l.pred[p] : -1, ss = s >= 0 ? l.succ[s] : -1;
    if ((fk & fBackbone) != 0u && pp >= 0 && ss >= 0 && (l.flags[pp] & fBackbone) != 0u && (l.flags[ss] & fBackbone) != 0u) {
      double a[3], b[3], c[3];
      load3(atom(l, K, aCA, pp), a);
      load3(atom(l, K, aCA, k), b);
      load3(atom(l, K, aCA, ss), c);
      const double u[3] = {b[0] - a[0], b[1] - a[1], b[2] - a[2]};
      const double v[3] = {c[0] - b[0], c[1] - b[1], c[2] - b[2]};
      if (dot3(u, v) < kCos70 * (sqrt(dot3(u, u)) * sqrt(dot3(v, v)))) st |= sS;
    }
    if (st != 0u) atomicOr(&l.state[k], st);  // (the hotspot mark above may land at the same time)
  }
  __syncthreads();

  // ---- helices (H), turns (T), bridges (B, E)
  for (int i = tid; i < K; i += kThreads) {
    const uint32_t fi = l.flags[i];
    const bool inside = (fi & fIn) != 0u;
    int j0 = -1, j1 = -1, t0 = 0, t1 = 0;
    if (inside) {
      const uint32_t st = l.state[i];
      const int p = l.pred[i];
      if ((st & sTurn4) != 0u && p >= 0 && (l.state[p] & sTurn4) != 0u) {
        int k = i;
        for (int m = 0; m < 4; ++m, k = l.succ[k]) atomicOr(&l.state[k], sH);
      }
#pragma unroll
      for (int n = 3; n <= 5; ++n) {
        if ((st & (sTurn3 << (n - 3))) == 0u) continue;
        int k = l.succ[i];
        for (int m = 1; m < n; ++m, k = l.succ[k]) atomicOr(&l.state[k], sT);
      }
      if ((fi & fLinked) != 0u) {
        const int si = l.succ[i];
        bool ladder = false;
        for (int j = 0; j < K; ++j) {
          const int t = bridge(l, W, i, j);
          if (t == 0) continue;
          if (j0 < 0) j0 = j, t0 = t & 1; else if (j1 < 0) j1 = j, t1 = t & 1;
          const int pj = l.pred[j], sj = l.succ[j];
          if ((t & 1) != 0 && (((bridge(l, W, si, sj) | bridge(l, W, p, pj)) & 1) != 0)) ladder = true;
          if ((t & 2) != 0 && (((bridge(l, W, si, pj) | bridge(l, W, p, sj)) & 2) != 0)) ladder = true;
        }
        if (j0 >= 0) atomicOr(&l.state[i], ladder ? sE : sB);
      }
    }
    const int64_t e = row * K + i;
    if (out.bridge_partner) out.bridge_partner[e * 2] = j0, out.bridge_partner[e * 2 + 1] = j1;
    if (out.bridge_parallel) out.bridge_parallel[e * 2] = static_cast<uint8_t>(t0), out.bridge_parallel[e * 2 + 1] = static_cast<uint8_t>(t1);
  }
  __syncthreads();

  // ---- G, then I: a stretch whole or not at all
#pragma unroll
  for (int n = 3; n <= 5; n += 2) {
    const uint32_t turn = n == 3 ? sTurn3 : sTurn5, mark = n == 3 ? sG : sI;
    const uint32_t higher = n == 3 ? (sH | sB | sE) : (sH | sB | sE | sG);
    for (int i = tid; i < K; i += kThreads) {
      const int p = l.pred[i];
      if ((l.flags[i] & fIn) == 0u || p < 0 || (l.state[i] & turn) == 0u || (l.state[p] & turn) == 0u) continue;
      bool is_free = true;
      int k = i;
      for (int m = 0; m < n; ++m, k = l.succ[k]) is_free = is_free && (l.state[k] & higher) == 0u;
      if (!is_free) continue;
      k = i;
      for (int m = 0; m < n; ++m, k = l.succ[k]) atomicOr(&l.state[k], mark);
    }
    __syncthreads();
  }

  // ---- the state of every residue and the counts of the row
  for (int k = tid; k < K; k += kThreads) {
    const uint32_t fk = l.flags[k], st = l.state[k];
    int code = 0;
    if ((fk & fIn) != 0u && (st & 127u) != 0u) code = __ffs(static_cast<int>(st & 127u));
    if (out.ss) out.ss[row * K + k] = static_cast<uint8_t>(code);
    if ((fk & fGen) != 0u) atomicAdd(&l.red[rCount + code], 1);
    if ((fk & fHotspot) != 0u) {
      atomicAdd(&l.red[rHot], 1);
      if ((st & sBonded) != 0u) atomicAdd(&l.red[rHotBonded], 1);
    }
  }
  __syncthreads();
  if (tid == 0) {
    if (out.n_hbonds) out.n_hbonds[row] = l.red[rBonds];
    if (out.n_internal) out.n_internal[row] = l.red[rInternal];
    if (out.n_antigen) out.n_antigen[row] = l.red[rAntigen];
    if (out.n_framework) out.n_framework[row] = l.red[rFramework];
    if (out.n_hotspot_bonded) out.n_hotspot_bonded[row] = l.red[rHotBonded];
    if (out.n_hotspot) out.n_hotspot[row] = l.red[rHot];
  }
  if (tid < 8 && out.ss_count != nullptr) out.ss_count[row * 8 + tid] = l.red[rCount + tid];
}

}  // namespace
}  // namespace diffab

using namespace diffab;

extern "C" {

int diffab_metrics_hbonds(const float* points, const uint8_t* donor_off, const float* context_points, const uint32_t* context_valid,
                          const uint8_t* context_donor_off, const uint8_t* generation_mask, const uint8_t* residue_mask,
                          const uint8_t* antigen_mask, const uint8_t* hotspot_mask, const int32_t* chain, const int32_t* residue_idx,
                          int32_t rows, int32_t group_size, int32_t K, int32_t A, float* O, float* H, int32_t* nh_o_partner,
                          float* nh_o_energy, int32_t* o_hn_partner, float* o_hn_energy, int32_t* bridge_partner,
                          uint8_t* bridge_parallel, uint8_t* ss, int32_t* residue_hbonds, int32_t* n_hbonds, int32_t* n_hbonds_internal,
                          int32_t* n_hbonds_antigen, int32_t* n_hbonds_framework, int32_t* n_hotspot_bonded, int32_t* n_hotspot,
                          float* hbond_energy, int32_t* ss_count, void* workspace, size_t workspace_bytes, void* stream) {
  StreamOrder order_(stream);
  const char* who = "metrics_hbonds";
  DIFFAB_REQUIRE(rows >= 0 && group_size >= 1 && K >= 1, DIFFAB_ERR_ARG, "%s: negative or empty extent (%d rows, group size %d, K = %d)", who,
                 rows, group_size, K);
  DIFFAB_REQUIRE(group_size <= kMaxGroup, DIFFAB_ERR_ARG, "%s: group size %d, at most %d designs per group", who, group_size, kMaxGroup);
  DIFFAB_REQUIRE(K <= kMaxK, DIFFAB_ERR_ARG, "%s: K = %d residues per patch, at most %d (the bond matrix of a row stays on chip)", who, K,
                 kMaxK);
  DIFFAB_REQUIRE(rows % group_size == 0, DIFFAB_ERR_ARG, "%s: %d rows are not a multiple of group_size = %d", who, rows, group_size);
  DIFFAB_REQUIRE(A >= 4 && A <= kMaxContextAtoms, DIFFAB_ERR_ARG, "%s: A = %d context atoms per residue outside [4, %d] (N, CA, C, O first)",
                 who, A, kMaxContextAtoms);
  DIFFAB_REQUIRE(hotspot_mask == nullptr || antigen_mask != nullptr, DIFFAB_ERR_ARG, "%s: a hotspot_mask needs an antigen_mask", who);
  if (rows == 0) return DIFFAB_OK;
  DIFFAB_REQUIRE(points && donor_off && context_points && context_valid && context_donor_off && generation_mask && chain && residue_idx,
                 DIFFAB_ERR_ARG, "%s: null input", who);
  const int32_t G = rows / group_size;
  const HbondWorkspace ws = carve_hbonds(workspace, G, K);
  if (const int e = workspace_ok(who, workspace, 256, workspace_bytes, ws.bytes)) return e;
  hipStream_t st = as_stream(stream);
  const int W = (K + 31) / 32;
  const size_t patch_lds = lds_words(K, W, false) * 4, rows_lds = lds_words(K, W, true) * 4;
  if (rows_lds > 64 * 1024) {  // (above the default limit of a launch: 73 KiB at K = 512, of the 160 KiB a CU has)
    static_assert(lds_words(kMaxK, (kMaxK + 31) / 32, true) * 4 <= 160 * 1024, "the row of the largest patch fits the LDS of a CU");
    DIFFAB_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(hbonds_rows_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                         static_cast<int>(rows_lds)));
  }
  const HbondIn in = {points, donor_off, context_points, context_valid, context_donor_off, generation_mask, residue_mask, antigen_mask,
                      hotspot_mask, chain, residue_idx};
  const HbondOut out = {O, H, nh_o_partner, nh_o_energy, o_hn_partner, o_hn_energy, bridge_partner, bridge_parallel, ss, residue_hbonds,
                        n_hbonds, n_hbonds_internal, n_hbonds_antigen, n_hbonds_framework, n_hotspot_bonded, n_hotspot, hbond_energy,
                        ss_count};
  hipLaunchKernelGGL(hbonds_patch_kernel, dim3(G), dim3(kThreads), patch_lds, st, in, K, A, ws);
  hipLaunchKernelGGL(hbonds_rows_kernel, dim3(static_cast<unsigned>(rows)), dim3(kThreads), rows_lds, st, in, group_size, K, A, ws, out);
  DIFFAB_LAUNCH_CHECK();
  return DIFFAB_OK;
}

}  // extern "C"
