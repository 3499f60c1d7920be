// surface_kernels.hip - solvent-accessible and buried surface of every design row on the device:
// diffab_metrics_surface, Shrake-Rupley sphere points of the generated residues and of the antigen.  The rule is the header comment of
// the entry in include/diffab_hip_analysis.h.
//
// Built with -ffp-contract=off (csrc/Makefile): a sphere point is fl(c + fl(R * u)) per component, the squared distance is the fp32 value
// (dx*dx + dy*dy) + dz*dz (dist2 of analysis_common.h, written out here) and "covered" is a strict comparison on it, so every point count is a defined number.  The areas are fp64 from
// the integer counts and the fp32 radii, summed in a fixed order of the row and rounded once.  VALU + LDS only, no atomics at all; every
// value reaches memory through plain C++ stores.
#include <climits>
#include <cmath>

#include "../../include/diffab_hip_analysis.h"
#include "analysis_prep.h"

namespace diffab {
namespace {

constexpr int kMaxK = DIFFAB_METRICS_MAX_K;
constexpr int kMaxPoints = DIFFAB_METRICS_MAX_POINTS;
constexpr int kMaxContextAtoms = DIFFAB_METRICS_MAX_CONTEXT_ATOMS;
constexpr int kMinSphere = DIFFAB_METRICS_SURFACE_MIN_POINTS;
constexpr int kMaxSphere = DIFFAB_METRICS_SURFACE_MAX_POINTS;
constexpr int kPasses = kMaxSphere / 64;  // a wave holds the sphere of one atom: lane = point, up to four passes of 64
constexpr int kList = 256;                // neighbours of one atom a wave keeps in LDS before it tests its points against them
constexpr int kStage = 1024;              // atoms of the generated residues of a row kept in LDS (more are read from the caller's points)
constexpr int kBatch = 64;                // target residues between two ordered additions to the row's sums
constexpr double kPi = 3.14159265358979323846;
static_assert(kMaxSphere % 64 == 0 && kPasses == 4, "the point loops are unrolled four times");
static_assert(kMaxContextAtoms <= 64 && kMaxPoints <= 8, "one lane per atom of a context residue; valid is a byte");
static_assert(kList >= 128, "a scan appends up to 64 neighbours before it looks at the fill");

constexpr int kAntigen = 1, kHotspot = 2, kGenerated = 4;

// Workspace of diffab_metrics_surface (DIFFAB_METRICS_SURFACE_WORKSPACE_BYTES covers the carves and their alignment): per patch, the
// context compacted once for all its designs - the antigen's atoms first, then the framework's - and the antigen's own point masks.
struct SurfaceWorkspace {
  float4* atoms;     // (G, K*A): x, y, z, R = radius + probe of the valid atoms of the listed context residues; [0, hdr.x) antigen
  uint64_t* masks;   // (G, K*A, 2, W): per antigen atom, the points no antigen atom covers, and those no context atom covers
  int4* targets;     // (G, K): residues with outputs, ascending: slot, first atom (antigen) or index among the generated, atoms, flags
  int32_t* gen;      // (G, K): slots of the generated residues inside residue_mask, ascending
  int4* hdr;         // (G, 2): antigen atoms, context atoms, generated residues, targets; hotspot residues, 0, 0, 0
  size_t bytes;
};

SurfaceWorkspace carve_surface(void* base, int64_t G, int64_t K, int64_t A, int64_t S) {
  Carver c(base);
  SurfaceWorkspace w;
  const int64_t W = (S + 63) / 64;
  w.atoms = c.take<float4>(static_cast<size_t>(G * K * A));
  w.masks = c.take<uint64_t>(static_cast<size_t>(G * K * A * 2 * W));
  w.targets = c.take<int4>(static_cast<size_t>(G * K));
  w.gen = c.take<int32_t>(static_cast<size_t>(G * K));
  w.hdr = c.take<int4>(static_cast<size_t>(G * 2));
  w.bytes = c.bytes();
  return w;
}

struct Radii {
  float r[kMaxPoints];
};

struct SurfaceOut {
  int32_t *free_points, *bound_points, *design_buried_points;             // (rows, K)
  float *free_area, *bound_area, *design_buried_area, *residue_buried;    // (rows, K)
  float *bsa_paratope, *bsa_epitope, *bsa_design_epitope;                 // (rows)
  int32_t *n_paratope_buried, *n_epitope_buried, *n_hotspot, *n_hotspot_buried;
  float* hotspot_buried_area;
};

// ------------------------------------------------------------------ 1. the context of a patch, compacted
// One work-group per patch.  Wave 0 lists the residues in ascending order (ballots and wave prefix sums over the atom counts of the two
// sides), then all threads copy the valid atoms behind each other: the antigen's, then the framework's.
__global__ void __launch_bounds__(256)
surface_pack_kernel(const float* __restrict__ ctx_points, const uint32_t* __restrict__ ctx_valid, const float* __restrict__ ctx_radius,
                    const uint8_t* __restrict__ generation_mask, const uint8_t* __restrict__ residue_mask,
                    const uint8_t* __restrict__ antigen_mask, const uint8_t* __restrict__ hotspot_mask, int K, int A, int P, float probe,
                    float radius_default, SurfaceWorkspace ws) {
  __shared__ int s_begin[kMaxK];  // first atom of a listed context residue on its side, -1 for every other slot
  __shared__ uint8_t s_antigen[kMaxK];
  __shared__ int s_n_antigen;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t g = blockIdx.x, base = g * K;
  const uint32_t amask = atom_mask_of(A);
  if (wave == 0) {
    int ng = 0, nt = 0, na = 0, nf = 0, nh = 0;
    const unsigned long long below = (1ull << lane) - 1ull;
    for (int k0 = 0; k0 < K; k0 += 64) {
      const int k = k0 + lane;
      const SlotClass c = classify_slot(k, K, base, residue_mask, generation_mask, antigen_mask, hotspot_mask, ctx_valid, amask);
      const bool gen = c.gen, antigen = c.antigen, hot = c.hot;
      const int cnt = __popc(c.bits);
      const unsigned long long vg = __ballot(gen);
      const int gi = ng + __popcll(vg & below);
      if (gen) ws.gen[base + gi] = k;
      int incl_a = antigen ? cnt : 0, incl_f = antigen ? 0 : cnt;
#pragma unroll
      for (int d = 1; d < 64; d <<= 1) {
        const int ta = __shfl_up(incl_a, d, 64), tf = __shfl_up(incl_f, d, 64);
        if (lane >= d) incl_a += ta, incl_f += tf;
      }
      const int begin = antigen ? na + incl_a - cnt : nf + incl_f - cnt;
      const bool target = gen || (antigen && cnt > 0);
      const unsigned long long vt = __ballot(target);
      if (target) {
        const int flags = gen ? kGenerated : (kAntigen | (hot ? kHotspot : 0));
        ws.targets[base + nt + __popcll(vt & below)] = make_int4(k, gen ? gi : begin, gen ? P : cnt, flags);
      }
      if (k < K) {
        s_begin[k] = cnt > 0 ? begin : -1;
        s_antigen[k] = antigen;
      }
      ng += __popcll(vg);
      nt += __popcll(vt);
      na += __shfl(incl_a, 63, 64);
      nf += __shfl(incl_f, 63, 64);
      nh += __popcll(__ballot(hot));
    }
    if (lane == 0) {
      ws.hdr[2 * g] = make_int4(na, na + nf, ng, nt);
      ws.hdr[2 * g + 1] = make_int4(nh, 0, 0, 0);
      s_n_antigen = na;
    }
  }
  __syncthreads();
  const int n_antigen = s_n_antigen;
  float4* out = ws.atoms + base * A;
  for (int t = tid; t < K * A; t += 256) {
    const int k = t / A, a = t - k * A;
    const int b = s_begin[k];
    if (b < 0) continue;
    const uint32_t bits = ctx_valid[base + k] & amask;
    if (((bits >> a) & 1u) == 0u) continue;
    const int64_t at = (base + k) * A + a;
    const float* p = ctx_points + at * 3;
    const float radius = ctx_radius != nullptr ? ctx_radius[at] : radius_default;
    out[(s_antigen[k] ? 0 : n_antigen) + b + __popc(bits & ((1u << a) - 1u))] = make_float4(p[0], p[1], p[2], radius + probe);
  }
}

// ------------------------------------------------------------------ a wave, the sphere of one atom and the atoms around it
// The points of the wave's atom: lane = point, pass p holds point 64 p + lane (idle beyond S).
struct Sphere {
  float qx[kPasses], qy[kPasses], qz[kPasses];
  float cx, cy, cz, R, slack;
};

// The lane's unit vectors of the caller's table, read once per wave.
struct Directions {
  float ux[kPasses], uy[kPasses], uz[kPasses];
};

__device__ inline void directions_of(Directions& u, const float* __restrict__ table, int S, int lane) {
#pragma unroll
  for (int p = 0; p < kPasses; ++p) {
    const int i = p * 64 + lane;
    u.ux[p] = u.uy[p] = u.uz[p] = 0.f;
    if (i < S) u.ux[p] = table[i * 3], u.uy[p] = table[i * 3 + 1], u.uz[p] = table[i * 3 + 2];
  }
}

__device__ inline void sphere_of(Sphere& s, float cx, float cy, float cz, float R, const Directions& u) {
  s.cx = cx, s.cy = cy, s.cz = cz, s.R = R;
  // what the rounding of a point can add to its distance from the centre, for the cull below: a few ulps of the largest number involved
  s.slack = 1e-6f * (((fabsf(cx) + fabsf(cy)) + fabsf(cz)) + R);
#pragma unroll
  for (int p = 0; p < kPasses; ++p) {
    const float ox = R * u.ux[p], oy = R * u.uy[p], oz = R * u.uz[p];
    s.qx[p] = cx + ox, s.qy[p] = cy + oy, s.qz[p] = cz + oz;
  }
}

// The wave's points against the `count` atoms (x, y, z, R^2) of its list: bit p of cov is set when an atom covers point 64 p + lane.
__device__ inline void cover_list(const Sphere& s, const float4* list, int count, int passes, uint32_t& cov) {
  for (int j = 0; j < count; ++j) {
    const float4 b = list[j];  // (every lane reads the same atom: an LDS broadcast)
#pragma unroll
    for (int p = 0; p < kPasses; ++p) {
      if (p < passes) {
        const float dx = s.qx[p] - b.x, dy = s.qy[p] - b.y, dz = s.qz[p] - b.z;
        const float d2 = (dx * dx + dy * dy) + dz * dz;
        if (d2 < b.w) cov |= 1u << p;
      }
    }
  }
}

// Atoms [begin, end) of `load` (x, y, z, R; R < 0 = no atom) other than `self`, 64 at a time, lane = candidate.  A candidate stays when
// its centre is no farther than R_a + R_b, widened above every rounding that enters (a point lies R_a from the centre up to `slack`, a
// covering atom R_b from the point): the cull never removes an atom that covers a point, so it never changes a count.  The kept atoms
// go into the wave's list in LDS by ballot compaction and the points are tested against the list whenever it may overflow, so neither
// the number of atoms nor of neighbours is limited.
template <class Load>
__device__ inline void cover_scan(const Sphere& s, Load load, int begin, int end, int self, float4* list, int passes, int lane,
                                  uint32_t& cov) {
  constexpr int kAhead = 4;  // batches of 64 candidates whose loads are in flight together (a scan is a chain of load latencies otherwise)
  int count = 0;
  const unsigned long long below = (1ull << lane) - 1ull;
  for (int b0 = begin; b0 < end; b0 += 64 * kAhead) {
    float4 v[kAhead];
#pragma unroll
    for (int u = 0; u < kAhead; ++u) {
      const int b = b0 + u * 64 + lane;
      v[u] = make_float4(0.f, 0.f, 0.f, -1.f);
      if (b < end && b != self) v[u] = load(b);
    }
#pragma unroll
    for (int u = 0; u < kAhead; ++u) {
      if (b0 + u * 64 < end) {
        const float dx = s.cx - v[u].x, dy = s.cy - v[u].y, dz = s.cz - v[u].z;
        const float d2 = (dx * dx + dy * dy) + dz * dz;
        const float reach = (s.R + v[u].w) * 1.00001f + s.slack;
        const bool keep = v[u].w >= 0.f && !(d2 > reach * reach * 1.00001f);
        const unsigned long long m = __ballot(keep);
        if (keep) list[count + __popcll(m & below)] = make_float4(v[u].x, v[u].y, v[u].z, v[u].w * v[u].w);
        count += __popcll(m);
        if (count > kList - 64) {
          __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
          __builtin_amdgcn_wave_barrier();
          cover_list(s, list, count, passes, cov);
          __builtin_amdgcn_wave_barrier();
          count = 0;
        }
      }
    }
  }
  if (count > 0) {
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
    cover_list(s, list, count, passes, cov);
    __builtin_amdgcn_wave_barrier();
  }
}

__device__ inline unsigned long long valid_lanes(int p, int S) {  // the lanes of pass p that hold a point
  const int n = S - p * 64;
  return n >= 64 ? ~0ull : (n <= 0 ? 0ull : ((1ull << n) - 1ull));
}

__device__ inline double area_weight(float R, int S) {
  const double r = static_cast<double>(R);
  return 4.0 * kPi * r * r / static_cast<double>(S);
}

// ------------------------------------------------------------------ 2. the antigen alone and in its patch: once per patch
// One wave per antigen atom.  Writes, per pass of 64 points, the points no other antigen atom covers and those no context atom covers.
__global__ void __launch_bounds__(256)
surface_antigen_kernel(const float* __restrict__ table, int S, int K, int A, int blocks_per_patch, SurfaceWorkspace ws) {
  __shared__ float4 s_list[4][kList];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t g = blockIdx.x / blocks_per_patch;
  const int t = (blockIdx.x % blocks_per_patch) * 4 + wave;
  const int4 hdr = ws.hdr[2 * g];
  if (t >= hdr.x) return;  // (no barrier below: a wave leaves alone)
  const int passes = (S + 63) / 64;
  const float4* atoms = ws.atoms + g * K * A;
  const float4 me = atoms[t];
  Directions dirs;
  directions_of(dirs, table, S, lane);
  Sphere s;
  sphere_of(s, me.x, me.y, me.z, me.w, dirs);
  auto load = [&](int b) { return atoms[b]; };
  uint32_t cov_antigen = 0;
  cover_scan(s, load, 0, hdr.x, t, s_list[wave], passes, lane, cov_antigen);
  uint32_t cov_all = cov_antigen;
  cover_scan(s, load, hdr.x, hdr.y, -1, s_list[wave], passes, lane, cov_all);
  uint64_t* out = ws.masks + (g * K * A + t) * 2 * passes;
#pragma unroll
  for (int p = 0; p < kPasses; ++p) {
    if (p < passes) {
      const unsigned long long open_antigen = __ballot(((cov_antigen >> p) & 1u) == 0u) & valid_lanes(p, S);
      const unsigned long long open_all = __ballot(((cov_all >> p) & 1u) == 0u) & valid_lanes(p, S);
      if (lane == 0) out[p] = open_antigen, out[passes + p] = open_all;
    }
  }
}

// ------------------------------------------------------------------ 3. the design rows
// What a target residue adds to its row, handed from the wave that computed it to the thread that adds the row up in residue order.
struct Contribution {
  double interface;  // free - bound area
  double buried;     // design-buried area (antigen)
  int flags;         // kGenerated / kAntigen / kHotspot, | 8 when the residue counts as buried
  int pad;
};

// One work-group per design row; a wave per target residue (ascending, kBatch residues between two ordered additions), lane = point.
template <int P>
__global__ void __launch_bounds__(256)
surface_rows_kernel(const float* __restrict__ points, const uint8_t* __restrict__ valid, const float* __restrict__ table, int S,
                    int group_size, int K, int A, Radii radii, float probe, SurfaceWorkspace ws, SurfaceOut out) {
  __shared__ float4 s_d[kStage];
  __shared__ float4 s_list[4][kList];
  __shared__ Contribution s_batch[kBatch];
  __shared__ float s_box[4][7];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t row = blockIdx.x;
  const int64_t g = row / group_size;
  const int4 hdr = ws.hdr[2 * g];
  const int n_antigen = hdr.x, n_context = hdr.y, ng = hdr.z;
  const int nt = ng > 0 ? hdr.w : 0;  // a row without a generated residue has nothing to evaluate: zeros
  const int nd = ng * P;
  const bool staged = nd <= kStage;
  const int passes = (S + 63) / 64;
  const int32_t* gen = ws.gen + g * K;
  const float4* atoms = ws.atoms + g * K * A;
  const float* pp = points + row * K * P * 3;
  const uint8_t* vv = valid + row * K;

  // atom i = (generated residue i / P, frame atom i % P) of this row: x, y, z, R, with R = -1 where the atom does not exist
  auto load_row = [&](int i) {
    const int gi = i / P, a = i - gi * P;
    const int k = gen[gi];
    const float* p = pp + (k * P + a) * 3;
    const bool there = ((vv[k] >> a) & 1u) != 0u;
    return make_float4(p[0], p[1], p[2], there ? radii.r[a] + probe : -1.f);
  };
  auto load_d = [&](int i) { return staged ? s_d[i] : load_row(i); };
  auto load_context = [&](int b) { return atoms[b]; };

  // ---- the row's own atoms into LDS (when they fit), and the box around them
  float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY}, widest = -1.f;
  for (int i = tid; i < nd; i += 256) {
    const float4 v = load_row(i);
    if (staged) s_d[i] = v;
    if (v.w >= 0.f) {
      lo[0] = fminf(lo[0], v.x), lo[1] = fminf(lo[1], v.y), lo[2] = fminf(lo[2], v.z);
      hi[0] = fmaxf(hi[0], v.x), hi[1] = fmaxf(hi[1], v.y), hi[2] = fmaxf(hi[2], v.z);
      widest = fmaxf(widest, v.w);
    }
  }
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) {
#pragma unroll
    for (int x = 0; x < 3; ++x) lo[x] = fminf(lo[x], __shfl_xor(lo[x], d, 64)), hi[x] = fmaxf(hi[x], __shfl_xor(hi[x], d, 64));
    widest = fmaxf(widest, __shfl_xor(widest, d, 64));
  }
  if (lane == 0) {
#pragma unroll
    for (int x = 0; x < 3; ++x) s_box[wave][x] = lo[x], s_box[wave][3 + x] = hi[x];
    s_box[wave][6] = widest;
  }
  __syncthreads();
#pragma unroll
  for (int w = 0; w < 4; ++w) {
#pragma unroll
    for (int x = 0; x < 3; ++x) lo[x] = fminf(lo[x], s_box[w][x]), hi[x] = fmaxf(hi[x], s_box[w][3 + x]);
    widest = fmaxf(widest, s_box[w][6]);
  }

  Directions dirs;
  directions_of(dirs, table, S, lane);

  // the row's sums, kept by thread 0
  double sum_paratope = 0.0, sum_epitope = 0.0, sum_design = 0.0, sum_hot = 0.0;
  int n_par = 0, n_epi = 0, n_hot = 0;

  for (int j0 = 0; j0 < nt; j0 += kBatch) {
    const int j1 = min(nt, j0 + kBatch);
    for (int j = j0 + wave; j < j1; j += 4) {
      const int4 tg = ws.targets[g * K + j];
      const int k = tg.x;
      int n_free = 0, n_bound = 0, n_buried = 0;
      double a_free = 0.0, a_bound = 0.0, a_buried = 0.0;
      if ((tg.w & kGenerated) != 0) {
        // a generated residue: its frame atoms one after the other.  Free = not covered by the row's own atoms or the framework;
        // bound = free and not covered by the antigen.
        for (int a = 0; a < P; ++a) {
          const int i = tg.y * P + a;
          const float4 me = load_d(i);
          if (!(me.w >= 0.f)) continue;  // (uniform: every lane read the same atom)
          Sphere s;
          sphere_of(s, me.x, me.y, me.z, me.w, dirs);
          uint32_t cov = 0;
          cover_scan(s, load_d, 0, nd, i, s_list[wave], passes, lane, cov);
          cover_scan(s, load_context, n_antigen, n_context, -1, s_list[wave], passes, lane, cov);
          const uint32_t cov_alone = cov;
          cover_scan(s, load_context, 0, n_antigen, -1, s_list[wave], passes, lane, cov);
          int nf = 0, nb = 0;
#pragma unroll
          for (int p = 0; p < kPasses; ++p) {
            if (p < passes) {
              nf += __popcll(__ballot(((cov_alone >> p) & 1u) == 0u) & valid_lanes(p, S));
              nb += __popcll(__ballot(((cov >> p) & 1u) == 0u) & valid_lanes(p, S));
            }
          }
          const double w = area_weight(me.w, S);
          n_free += nf, n_bound += nb;
          a_free += static_cast<double>(nf) * w, a_bound += static_cast<double>(nb) * w;
        }
      } else {
        // an antigen residue: lane = atom.  Its free points are the patch's (kernel 2); of the points nothing of the context covers,
        // those an atom of the row covers are design-buried, the others bound.  Only an atom within reach of the row's box is tested.
        const bool mine = lane < tg.z;
        const int t = tg.y + (mine ? lane : 0);
        const float4 me = atoms[t];
        const uint64_t* mk = ws.masks + (g * K * A + t) * 2 * passes;
        unsigned long long open[kPasses] = {0ull, 0ull, 0ull, 0ull};
        int nf = 0, no = 0, nbur = 0;
#pragma unroll
        for (int p = 0; p < kPasses; ++p) {
          if (p < passes && mine) {
            nf += __popcll(mk[p]);
            open[p] = mk[passes + p];
            no += __popcll(open[p]);
          }
        }
        float gap2 = 0.f;
        {
          const float c[3] = {me.x, me.y, me.z};
#pragma unroll
          for (int x = 0; x < 3; ++x) {
            const float d = fmaxf(fmaxf(lo[x] - c[x], c[x] - hi[x]), 0.f);
            gap2 += d * d;
          }
        }
        const float slack = 1e-6f * (((fabsf(me.x) + fabsf(me.y)) + fabsf(me.z)) + me.w);
        const float reach = (me.w + widest) * 1.00001f + slack;
        const bool near = mine && no > 0 && widest >= 0.f && !(gap2 > reach * reach * 1.00001f);
        unsigned long long todo = __ballot(near);
        while (todo != 0ull) {
          const int a = __ffsll(static_cast<long long>(todo)) - 1;
          todo &= todo - 1ull;
          Sphere s;
          sphere_of(s, __shfl(me.x, a, 64), __shfl(me.y, a, 64), __shfl(me.z, a, 64), __shfl(me.w, a, 64), dirs);
          uint32_t cov = 0;
          cover_scan(s, load_d, 0, nd, -1, s_list[wave], passes, lane, cov);
          int nb = 0;
#pragma unroll
          for (int p = 0; p < kPasses; ++p) {
            if (p < passes) {
              const unsigned long long op = __shfl(open[p], a, 64);
              nb += __popcll(__ballot(((cov >> p) & 1u) != 0u) & op);
            }
          }
          if (lane == a) nbur = nb;
        }
        for (int a = 0; a < tg.z; ++a) {  // the atoms in slot order
          const int f = __shfl(nf, a, 64), o = __shfl(no, a, 64), b = __shfl(nbur, a, 64);
          const double w = area_weight(__shfl(me.w, a, 64), S);
          n_free += f, n_bound += o - b, n_buried += b;
          a_free += static_cast<double>(f) * w, a_bound += static_cast<double>(o - b) * w, a_buried += static_cast<double>(b) * w;
        }
      }
      if (lane == 0) {
        const bool generated = (tg.w & kGenerated) != 0;
        const int64_t e = row * K + k;
        if (out.free_points) out.free_points[e] = n_free;
        if (out.bound_points) out.bound_points[e] = n_bound;
        if (out.design_buried_points) out.design_buried_points[e] = n_buried;
        if (out.free_area) out.free_area[e] = static_cast<float>(a_free);
        if (out.bound_area) out.bound_area[e] = static_cast<float>(a_bound);
        if (out.design_buried_area) out.design_buried_area[e] = static_cast<float>(a_buried);
        if (out.residue_buried) out.residue_buried[e] = static_cast<float>(generated ? a_free - a_bound : a_buried);
        Contribution c;
        c.interface = a_free - a_bound;
        c.buried = a_buried;
        c.flags = tg.w | ((generated ? n_free > n_bound : n_buried > 0) ? 8 : 0);
        c.pad = 0;
        s_batch[j - j0] = c;
      }
    }
    __syncthreads();
    if (tid == 0) {
      for (int j = 0; j < j1 - j0; ++j) {  // residue order
        const Contribution c = s_batch[j];
        const bool is_buried = (c.flags & 8) != 0;
        if ((c.flags & kGenerated) != 0) {
          sum_paratope += c.interface;
          n_par += is_buried;
        } else {
          sum_epitope += c.interface;
          sum_design += c.buried;
          n_epi += is_buried;
          if ((c.flags & kHotspot) != 0) {
            sum_hot += c.buried;
            n_hot += is_buried;
          }
        }
      }
    }
    __syncthreads();
  }
  if (tid != 0) return;
  if (out.bsa_paratope) out.bsa_paratope[row] = static_cast<float>(sum_paratope);
  if (out.bsa_epitope) out.bsa_epitope[row] = static_cast<float>(sum_epitope);
  if (out.bsa_design_epitope) out.bsa_design_epitope[row] = static_cast<float>(sum_design);
  if (out.n_paratope_buried) out.n_paratope_buried[row] = n_par;
  if (out.n_epitope_buried) out.n_epitope_buried[row] = n_epi;
  if (out.n_hotspot) out.n_hotspot[row] = ng > 0 ? ws.hdr[2 * g + 1].x : 0;
  if (out.n_hotspot_buried) out.n_hotspot_buried[row] = n_hot;
  if (out.hotspot_buried_area) out.hotspot_buried_area[row] = static_cast<float>(sum_hot);
}

}  // namespace
}  // namespace diffab

using namespace diffab;

extern "C" {

int diffab_metrics_surface(const float* points, const uint8_t* valid, const float* point_radius, const float* context_points,
                           const uint32_t* context_valid, const float* context_radius, const uint8_t* generation_mask,
                           const uint8_t* residue_mask, const uint8_t* antigen_mask, const uint8_t* hotspot_mask, const float* sphere,
                           int32_t rows, int32_t group_size, int32_t K, int32_t P, int32_t A, int32_t S, float probe,
                           float context_radius_default, int32_t* free_points, int32_t* bound_points, int32_t* design_buried_points,
                           float* free_area, float* bound_area, float* design_buried_area, float* residue_buried, float* bsa_paratope,
                           float* bsa_epitope, float* bsa_design_epitope, int32_t* n_paratope_buried, int32_t* n_epitope_buried,
                           int32_t* n_hotspot, int32_t* n_hotspot_buried, float* hotspot_buried_area, void* workspace,
                           size_t workspace_bytes, void* stream) {
  StreamOrder order_(stream);
  const char* who = "metrics_surface";
  if (!rows_shape_ok(who, rows, group_size, K, kMaxK)) return DIFFAB_ERR_ARG;
  DIFFAB_REQUIRE(P >= 1 && P <= kMaxPoints, DIFFAB_ERR_ARG, "%s: P = %d points per residue outside [1, %d]", who, P, kMaxPoints);
  DIFFAB_REQUIRE(A >= 1 && A <= kMaxContextAtoms, DIFFAB_ERR_ARG, "%s: A = %d context atoms per residue outside [1, %d]", who, A,
                 kMaxContextAtoms);
  DIFFAB_REQUIRE(S >= kMinSphere && S <= kMaxSphere, DIFFAB_ERR_ARG, "%s: S = %d sphere points outside [%d, %d]", who, S, kMinSphere,
                 kMaxSphere);
  DIFFAB_REQUIRE(finite_nonnegative(probe), DIFFAB_ERR_ARG, "%s: probe must be finite and >= 0, got %g", who, static_cast<double>(probe));
  DIFFAB_REQUIRE(finite_nonnegative(context_radius_default), DIFFAB_ERR_ARG, "%s: context_radius_default must be finite and >= 0, got %g", who,
                 static_cast<double>(context_radius_default));
  DIFFAB_REQUIRE(hotspot_mask == nullptr || antigen_mask != nullptr, DIFFAB_ERR_ARG, "%s: a hotspot_mask needs an antigen_mask", who);
  if (rows == 0) return DIFFAB_OK;
  DIFFAB_REQUIRE(points && valid && point_radius && context_points && context_valid && generation_mask && sphere, DIFFAB_ERR_ARG,
                 "%s: null input", who);
  Radii radii = {};
  for (int a = 0; a < P; ++a) {
    DIFFAB_REQUIRE(finite_nonnegative(point_radius[a]), DIFFAB_ERR_ARG, "%s: point_radius[%d] must be finite and >= 0, got %g", who, a,
                   static_cast<double>(point_radius[a]));
    radii.r[a] = point_radius[a];
  }
  const int32_t G = rows / group_size;
  const SurfaceWorkspace ws = carve_surface(workspace, G, K, A, S);
  if (const int e = workspace_ok(who, workspace, 256, workspace_bytes, ws.bytes)) return e;
  const int blocks_per_patch = (K * A + 3) / 4;
  const int64_t antigen_grid = static_cast<int64_t>(G) * blocks_per_patch;
  DIFFAB_REQUIRE(antigen_grid <= INT_MAX, DIFFAB_ERR_UNSUPPORTED, "%s: %d patches of %d atom slots are more work-groups than one launch holds",
                 who, G, K * A);
  hipStream_t st = as_stream(stream);
  // every element of a per-residue output is written: zero, then the target residues by the rows kernel
  const size_t per_residue = static_cast<size_t>(rows) * static_cast<size_t>(K) * 4;
  for (void* p : {static_cast<void*>(free_points), static_cast<void*>(bound_points), static_cast<void*>(design_buried_points),
                  static_cast<void*>(free_area), static_cast<void*>(bound_area), static_cast<void*>(design_buried_area),
                  static_cast<void*>(residue_buried)})
    if (p != nullptr) DIFFAB_HIP_CHECK(hipMemsetAsync(p, 0, per_residue, st));
  hipLaunchKernelGGL(surface_pack_kernel, dim3(G), dim3(256), 0, st, context_points, context_valid, context_radius, generation_mask,
                     residue_mask, antigen_mask, hotspot_mask, K, A, P, probe, context_radius_default, ws);
  if (antigen_mask != nullptr)
    hipLaunchKernelGGL(surface_antigen_kernel, dim3(static_cast<unsigned>(antigen_grid)), dim3(256), 0, st, sphere, S, K, A,
                       blocks_per_patch, ws);
  SurfaceOut out = {free_points, bound_points, design_buried_points, free_area,        bound_area,       design_buried_area,
                    residue_buried, bsa_paratope, bsa_epitope,        bsa_design_epitope, n_paratope_buried, n_epitope_buried,
                    n_hotspot,   n_hotspot_buried, hotspot_buried_area};
#define DIFFAB_SURFACE_LAUNCH(PP)                                                                                                  \
  hipLaunchKernelGGL((surface_rows_kernel<PP>), dim3(static_cast<unsigned>(rows)), dim3(256), 0, st, points, valid, sphere, S, group_size, \
                     K, A, radii, probe, ws, out)
  switch (P) {
    case 1: DIFFAB_SURFACE_LAUNCH(1); break;
    case 2: DIFFAB_SURFACE_LAUNCH(2); break;
    case 3: DIFFAB_SURFACE_LAUNCH(3); break;
    case 4: DIFFAB_SURFACE_LAUNCH(4); break;
    default: DIFFAB_SURFACE_LAUNCH(5); break;
  }
#undef DIFFAB_SURFACE_LAUNCH
  DIFFAB_LAUNCH_CHECK();
  return DIFFAB_OK;
}

}  // extern "C"
