// analysis_common.h - what the analysis translation units (the metrics, geometry, ensemble, similarity, hbond, cluster, pareto,
// interface, develop, energy, novelty and conformation kernels: DESIGN sections 4.13 - 4.27) share: wave reductions and ranks, the defined squared distance,
// the site record of a residue, and the host checks every such entry makes on its extents and its workspace.
// Only what at least two of those files use lives here, and only what leaves the device code the compiler makes of them as it was.
//
// The fp32 results are defined numbers only in a translation unit built with -ffp-contract=off (the DEFINED_OBJS of csrc/Makefile):
// dist2 below is (dx*dx + dy*dy) + dz*dz with every product and sum rounded, and a contracted build would fuse them.
#pragma once
#include <cmath>

#include "common.h"

namespace diffab {

// ------------------------------------------------------------------ a wave of 64 lanes
// The sum of v over the 64 lanes in a fixed tree (lane ^ 32, ^ 16, ..., ^ 1): every lane ends with the same bits.
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}
__device__ __forceinline__ int wave_sum(int v) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}
template <typename T, int V>
__device__ inline void wave_sum(T (&v)[V]) {
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) {
#pragma unroll
    for (int i = 0; i < V; ++i) v[i] += __shfl_xor(v[i], d, 64);
  }
}

// Where a lane stands among the lanes of its wave for which `pred` holds (the set lanes below it), and how many there are.
struct BallotRank {
  int rank, count;
};
__device__ __forceinline__ BallotRank ballot_rank(bool pred, int lane) {
  const unsigned long long v = __ballot(pred);
  BallotRank r;
  r.rank = __popcll(v & ((1ull << lane) - 1ull)), r.count = __popcll(v);
  return r;
}

// ------------------------------------------------------------------ the defined squared distance
__device__ __forceinline__ float dist2(float ax, float ay, float az, float bx, float by, float bz) {
  const float dx = ax - bx, dy = ay - by, dz = az - bz;
  return (dx * dx + dy * dy) + dz * dz;
}

// ------------------------------------------------------------------ one site per residue
// What depends on the patch alone, one record per slot (diffab_metrics_patches, diffab_metrics_pair_energy): the patch's site of a
// present non-generated residue, zeros for a present generated one (the row kernel puts the row's site there) and NaN for a residue
// that is not present, which then fails every comparison.
struct alignas(16) SiteRecord {
  float x, y, z;
  uint32_t flags;
};
// SiteRecord::flags.  kSiteGenerated and kSiteAntigen are set for present residues only and exclude each other.
constexpr uint32_t kSitePresent = 1u, kSiteGenerated = 2u, kSiteAntigen = 4u;

// ------------------------------------------------------------------ the host checks of an entry
// Each sets the error text and says no; an entry makes them in this order.
inline bool rows_shape_ok(const char* who, int32_t rows, int32_t group_size, int32_t K, int32_t max_K) {
  if (rows < 0 || group_size < 1 || K < 1) {
    set_error("%s: negative or empty extent (%d rows, group size %d, K = %d)", who, rows, group_size, K);
    return false;
  }
  if (group_size > DIFFAB_METRICS_MAX_GROUP) {
    set_error("%s: group size %d, at most %d designs per group", who, group_size, DIFFAB_METRICS_MAX_GROUP);
    return false;
  }
  if (K > max_K) {
    set_error("%s: K = %d residues per patch, at most %d", who, K, max_K);
    return false;
  }
  if (rows % group_size != 0) {
    set_error("%s: %d rows are not a multiple of group_size = %d", who, rows, group_size);
    return false;
  }
  return true;
}

inline bool group_shape_ok(const char* who, int32_t G, int32_t N) {
  if (G < 0 || N < 1) {
    set_error("%s: negative or empty extent (G = %d, N = %d)", who, G, N);
    return false;
  }
  if (N > DIFFAB_METRICS_MAX_GROUP) {
    set_error("%s: N = %d, at most %d designs per group", who, N, DIFFAB_METRICS_MAX_GROUP);
    return false;
  }
  return true;
}

// DIFFAB_OK, or the code of what is wrong with the workspace: not a device buffer of the entry's alignment, or shorter than its carves.
inline int workspace_ok(const char* who, const void* workspace, int align, size_t have, size_t need) {
  DIFFAB_REQUIRE(workspace != nullptr && reinterpret_cast<uintptr_t>(workspace) % static_cast<uintptr_t>(align) == 0, DIFFAB_ERR_ARG,
                 "%s: the workspace must be a %d-byte aligned device buffer", who, align);
  DIFFAB_REQUIRE(have >= need, DIFFAB_ERR_WORKSPACE, "%s: workspace of %zu bytes, %zu needed", who, have, need);
  return DIFFAB_OK;
}

inline bool finite_nonnegative(float v) { return v >= 0.f && v < INFINITY; }

}  // namespace diffab
