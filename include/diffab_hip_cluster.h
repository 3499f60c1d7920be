/* diffab_hip_cluster.h - set-level analysis of the designs of a patch from a table of them - their pairwise matrix, or their objectives:
 * the fourth header of libdiffab_hip.so.
 *
 * Why a header of its own: the export lists of include/diffab_hip.h, include/diffab_hip_analysis.h and include/diffab_hip_hbonds.h are
 * each pinned, name by name, by tests that are the record of finished audits (symbols, operand alignment, operand extents); the hbonds
 * header is pinned to exactly one name.  The entries that take a table of one patch's designs - the (G,N,N) pairwise matrix, or the
 * (G,N,M) objectives - and answer a question about the SET are declared here, typed in _hip.CLUSTER_SYMBOLS onto the same library, and bring their contract tests (workspace contents, operand
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

/* diffab_metrics_pareto: Pareto ranking of the N designs of every patch over M objectives - the non-dominated fronts, with hard limits
 * handled by Deb's constrained domination.  Integer-exact: loads, fp32 compares, popcounts and integer adds only, so
 * every output is a function of the fp32 inputs, and a patch alone gives the bits it gives in a batch.
 *
 * Inputs.  objectives (G,N,M) fp32; maximize (M) uint8, on the device, or NULL (every objective is minimised); violation (G,N) fp32 or
 * NULL (every design is feasible); score (G,N) fp32 or NULL (none); candidates (G,N) uint8 or NULL (all).
 * 1 <= N <= DIFFAB_METRICS_MAX_GROUP, 1 <= M <= DIFFAB_METRICS_PARETO_MAX_OBJECTIVES, 0 <= F <= N (F = max_fronts).
 *
 * The rule, per patch g.
 *   v(i,m) is objectives[g,i,m] as stored, with its sign bit flipped where maximize[m] is set; a NaN of either sign then counts as +inf
 *     (a missing number is the worst value).  All compares are fp32 compares, so -0 equals +0.
 *   w(i) is violation[g,i]: a NaN counts as +inf, every value <= 0 (-0 included) counts as 0; without the operand every w(i) is 0.
 *   dom(i,j), "i dominates j", requires that i and j are both candidates and i != j, and holds when w(i) < w(j), or when w(i) == w(j),
 *     v(i,m) <= v(j,m) for every m and v(i,m) < v(j,m) for at least one m.  Equal vectors do not dominate each other and share a front.
 *   The open set starts as the candidates.  While it is not empty and fewer than F fronts have been made: front r is every open design
 *     that no open design dominates; its designs get rank = r and leave the open set, and front_size[g,r] is their number.
 *   rank is -1 for non-candidates and for designs still open when F fronts have been made.  n_dominators[g,j] counts the candidates that
 *     dominate j and n_dominated[g,i] the candidates that i dominates, both over ALL candidates, not only the open ones, and both -1
 *     for a non-candidate.  front_size is 0 past count[g], the number of fronts made; n_unranked[g] counts the candidates still open.
 *   order[g] is a full permutation of 0..N-1, best first: the designs sorted by the tuple (class, score, -n_dominated, index), where the
 *     class is the rank of a ranked design, N for an unranked candidate and N + 1 for a non-candidate; a NaN score counts as +inf,
 *     -0 equals +0, and without the operand all scores are equal.  Front r is therefore a contiguous slice of order whose length
 *     front_size gives.
 * Properties that follow: dom is irreflexive and never holds both ways; rank[j] > rank[i] wherever dom(i,j) and both are ranked; every
 * design of front r > 0 has a dominator in front r - 1; with F >= 1, rank == 0 exactly where n_dominators == 0.
 *
 * Outputs.  rank (G,N) int32; n_dominators (G,N) int32, nullable; n_dominated (G,N) int32, nullable; front_size (G,F) int32, which may be
 * NULL when F = 0; count (G) int32; n_unranked (G) int32, nullable; order (G,N) int64, nullable.
 *
 * Limits, DIFFAB_ERR_ARG, decided from the scalars and from which pointers are NULL before anything is enqueued: G >= 0, N, M and F as
 * above, a NULL objectives, rank or count, a NULL front_size with F > 0, a workspace that is NULL or not 256-byte aligned (too small:
 * DIFFAB_ERR_WORKSPACE).
 *
 * Two launches, in the shape and the layouts of diffab_metrics_cluster.  (1) Dominance, over the whole device: one wave per 64 designs j
 * x 256 designs i of a patch stages the 320 key rows objective-major in LDS - sign flip, NaN -> +inf and the violation clamp applied
 * once, a non-candidate's w made NaN so that no compare with it holds - and writes dom as 32-bit words into the workspace, the lanes of a
 * wave packed with a ballot: word-major, (G, W, Np) with Np = N rounded up to 64 and W = Np / 32, bit i % 32 of word [i / 32][j] =
 * dom(i,j), zero for i or j >= N; with them, per 256-design segment the dominators of every j, (G, S, Np) int32 with S = ceil(N / 256),
 * and per tile of 64 designs j the designs every i dominates, (G, Np / 64, Np) int32 - partial sums, no atomics.  (2) Peel, one work-group
 * per patch of 64 to 1024 threads: each thread owns the count of OPEN dominators of one design (of up to four above 1024 designs); per
 * front the open designs whose count is 0 are the members, the waves' ballots are the member words, and after one barrier every design
 * still open subtracts popcount(own row & member words) over the non-zero member words.  After the loop the position of every design in
 * order is the number of designs whose tuple is smaller, counted from the keys in LDS - (class, score, -n_dominated) as one 64-bit
 * integer, the index settled by which side of the design the other one lies - and one pass writes every output.  With
 * N <= DIFFAB_METRICS_CLUSTER_LDS_MAX_N the patch's bit matrix is copied into LDS and stays there; above it the words are read from the
 * workspace.
 * workspace: DIFFAB_METRICS_PARETO_WORKSPACE_BYTES(G, N) bytes. */
#define DIFFAB_METRICS_PARETO_MAX_OBJECTIVES 16
#define DIFFAB_METRICS_PARETO_WORKSPACE_BYTES(G, N)                                                                      \
  ((size_t)(G) * (DIFFAB_METRICS_CLUSTER_PAD64(N) * DIFFAB_METRICS_CLUSTER_PAD64(N) / 8 +                                \
                  (((size_t)(N) + 255) / 256) * DIFFAB_METRICS_CLUSTER_PAD64(N) * 4 +                                    \
                  (DIFFAB_METRICS_CLUSTER_PAD64(N) / 64) * DIFFAB_METRICS_CLUSTER_PAD64(N) * 4) + 1024)
int diffab_metrics_pareto(const float* objectives, const uint8_t* maximize, const float* violation, const float* score,
                          const uint8_t* candidates, int32_t G, int32_t N, int32_t M, int32_t F, int32_t* rank, int32_t* n_dominators,
                          int32_t* n_dominated, int32_t* front_size, int32_t* count, int32_t* n_unranked, int64_t* order, void* workspace,
                          size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* DIFFAB_HIP_CLUSTER_H */
