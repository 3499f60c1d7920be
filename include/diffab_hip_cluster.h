/* diffab_hip_cluster.h - set-level analysis of the designs of a patch from their pairwise matrix: the fourth header of libdiffab_hip.so.
 *
 * Why a header of its own: the export lists of include/diffab_hip.h, include/diffab_hip_analysis.h and include/diffab_hip_hbonds.h are
 * each pinned, name by name, by tests that are the record of finished audits (symbols, operand alignment, operand extents); the hbonds
 * header is pinned to exactly one name.  The entries that take a (G,N,N) matrix of one patch's designs and answer a question about the
 * SET are declared here, typed in _hip.CLUSTER_SYMBOLS onto the same library, and bring their contract tests (workspace contents, operand
 * alignment, guard bands, host-side refusals) in test files of their own.  This header's test asserts that table and header agree, not
 * how many names there are: the next set-level entry joins it here.
 *
 * Same library, same conventions, same contracts as include/diffab_hip.h - its "General contract" applies word for word: every check is
 * made on the host before anything is enqueued; a refusal returns a negative DIFFAB_ERR_* and leaves its message in diffab_last_error();
 * an empty problem (G = 0) returns 0 before any pointer is looked at; what the workspace holds on entry is ignored and nothing outside
 * [workspace, workspace + bytes) is written; every element of every non-NULL output is written and a NULL output is skipped; every DATA
 * operand is ACCEPTED at its natural alignment (4 bytes float / int32, 8 bytes int64, 1 byte masks); the workspace is 256-byte aligned.
 */
#ifndef DIFFAB_HIP_CLUSTER_H
#define DIFFAB_HIP_CLUSTER_H

#include "diffab_hip.h" /* DIFFAB_OK, DIFFAB_ERR_*, DIFFAB_METRICS_MAX_GROUP */

#ifdef __cplusplus
extern "C" {
#endif

/* diffab_metrics_cluster: the Daura / GROMOS neighbour-count clustering of the N designs of every patch at a distance cutoff, from the
 * matrix diffab_metrics_pairwise returns (rmsd, or 1 - seq_identity).  Integer-exact: loads, compares, popcounts and
 * integer adds only, so every output is a function of the fp32 inputs, and a patch alone gives the bits it gives in a batch.
 *
 * Inputs.  dist (G,N,N) fp32; cutoff (G) fp32, on the device; score (G,N) fp32 or NULL (none); candidates (G,N) uint8 or NULL (all).
 * 1 <= N <= DIFFAB_METRICS_MAX_GROUP, 0 <= M <= N.
 *
 * The rule, per patch g.
 *   adj(i,j) is true when i == j, or when dist[g,i,j] <= cutoff[g] as one fp32 compare of the stored values.  The row used is the row of
 *     i, as diffab_metrics_select_diverse reads the row of the pick.  A NaN distance or a NaN cutoff means not a neighbour.  The value on
 *     the diagonal does not enter.  Nothing assumes symmetry.
 *   The open set starts as the candidates.  n(i) is the number of open j with adj(i,j).
 *   Repeat while the open set is not empty and fewer than M clusters have been made:
 *     the centre is the open i with the largest n(i); ties go to the lower score (a NaN score counts as +inf, compared as fp32 values);
 *     remaining ties go to the lower index.  The centre's open neighbours become cluster c, the centre included.  For each member j:
 *     label[j] = c and center_dist[j] = dist[g,centre,j] as stored (0 for the centre itself, by definition).  center[g,c] = centre and
 *     size[g,c] is the member count.  The members leave the open set.
 *   count[g] is the number of clusters made; center and size are padded with -1 / 0 up to M.  Designs still open when M is reached, and
 *     non-candidates, get label = -1 and center_dist = NaN.  n_unassigned[g] counts only the designs still open.
 * Two properties follow: sizes are non-increasing in c, and a later centre is never within the cutoff of an earlier centre's row.
 *
 * Outputs.  label (G,N) int32; center_dist (G,N) fp32, nullable; center (G,M) int64 and size (G,M) int32, which may be NULL when M = 0;
 * count (G) int32; n_unassigned (G) int32, nullable.
 *
 * Limits, DIFFAB_ERR_ARG, decided from the scalars and from which pointers are NULL before anything is enqueued: G >= 0, N and M as
 * above, a NULL dist, cutoff, label or count, a NULL center or size with M > 0, a workspace that is NULL or not 256-byte aligned (too
 * small: DIFFAB_ERR_WORKSPACE).
 *
 * Two launches.  (1) Threshold, over the whole device: one wave per 64 rows x 256 columns of a patch's matrix reads dist ONCE and writes
 * the adjacency as 32-bit words into the workspace, the lanes of a wave packed with a ballot - word-major, (G, W, Np) with Np = N rounded
 * up to 64 and W = Np / 32: bit j % 32 of word [j / 32][i] = adj(i,j), zero for i or j >= N - and, per 256-column segment, the number of
 * candidate neighbours of every row, (G, S, Np) int32 with S = ceil(N / 256); their sum over S is the initial n(i).  (2) Cluster, one
 * work-group per patch of 64 to 1024 threads: each thread owns the running count of one design (of up to four above 1024 designs); per
 * cluster a block arg-max on (count, -score, -index), the centre's row ANDed with the open words gives the member words, and every open
 * design subtracts popcount(own row & member words).  The adjacency is never thresholded again and no count is recomputed.  With
 * N <= DIFFAB_METRICS_CLUSTER_LDS_MAX_N the patch's bit matrix is copied into LDS (N * N / 8 bytes, sized by N: small patches share a
 * CU) and stays there; above it the words are read from the workspace (2 MiB per patch at N = 4096).
 * workspace: DIFFAB_METRICS_CLUSTER_WORKSPACE_BYTES(G, N) bytes. */
#define DIFFAB_METRICS_CLUSTER_LDS_MAX_N 1024
#define DIFFAB_METRICS_CLUSTER_PAD64(N) ((((size_t)(N) + 63) / 64) * 64)
#define DIFFAB_METRICS_CLUSTER_WORKSPACE_BYTES(G, N)                                                                     \
  ((size_t)(G) * (DIFFAB_METRICS_CLUSTER_PAD64(N) * DIFFAB_METRICS_CLUSTER_PAD64(N) / 8 +                                \
                  (((size_t)(N) + 255) / 256) * DIFFAB_METRICS_CLUSTER_PAD64(N) * 4) + 1024)
int diffab_metrics_cluster(const float* dist, const float* cutoff, const float* score, const uint8_t* candidates, int32_t G, int32_t N,
                           int32_t M, int32_t* label, float* center_dist, int64_t* center, int32_t* size, int32_t* count,
                           int32_t* n_unassigned, void* workspace, size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* DIFFAB_HIP_CLUSTER_H */
