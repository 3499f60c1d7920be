/* diffab_hip_interface.h - the interface of a design as a SET: which generated residue touches which antigen residue, as bits, and the
 * overlap of such sets between all the designs of a patch (the fraction of common contacts): the fifth header of libdiffab_hip.so.
 *
 * Why a header of its own: the export lists of include/diffab_hip.h, include/diffab_hip_analysis.h, include/diffab_hip_hbonds.h and
 * include/diffab_hip_cluster.h are each pinned by tests that are the record of finished audits, and the cluster header's test allows its
 * entries pointer, int32_t and size_t parameters only - diffab_metrics_contact_bits takes a distance.  The entries that produce or compare
 * PACKED BIT SETS per design are declared here, typed in _hip.INTERFACE_SYMBOLS onto the same library, and bring their contract tests
 * (workspace contents, operand alignment, guard bands, host-side refusals) in test files of their own.  This header's test asserts that
 * table and header agree, not how many names there are.
 *
 * Same library, same conventions, same contracts as include/diffab_hip.h - its "General contract" applies word for word: every check is
 * made on the host before anything is enqueued; a refusal returns a negative DIFFAB_ERR_* and leaves its message in diffab_last_error();
 * an empty problem (rows = 0, G = 0) returns 0 before any pointer is looked at; what the workspace holds on entry is ignored and nothing
 * outside [workspace, workspace + bytes) is written; every element of every non-NULL output is written, zeros included, whatever it held,
 * and a NULL output is skipped; every DATA operand is ACCEPTED at its natural alignment (4 bytes float / int32 / uint32, 1 byte masks);
 * the workspace is 256-byte aligned.  Integer work only - compares, ORs, ANDs, popcounts, integer adds, and one correctly rounded fp32
 * division per quotient - and no atomics, so every output is a function of the inputs and a patch alone gives the bits it gives in a batch.
 */
#ifndef DIFFAB_HIP_INTERFACE_H
#define DIFFAB_HIP_INTERFACE_H

#include "diffab_hip.h" /* DIFFAB_OK, DIFFAB_ERR_*, DIFFAB_METRICS_MAX_GROUP, DIFFAB_METRICS_MAX_POINTS, DIFFAB_METRICS_MAX_CONTEXT_ATOMS */

#ifdef __cplusplus
extern "C" {
#endif

/* diffab_metrics_contact_bits: the contacts diffab_metrics_contacts COUNTS as n_contact_pairs, kept as data.
 *
 * Inputs, as diffab_metrics_contacts names and lays them out (include/diffab_hip.h, whose header comment is the rule): points
 * (rows,K,P,3) fp32 and valid (rows,K) uint8, the atoms of every design row and their validity bits, 1 <= P <= DIFFAB_METRICS_MAX_POINTS;
 * context_points (G,K,A,3) fp32 and context_valid (G,K) uint32, the patch's own atoms, 1 <= A <= DIFFAB_METRICS_MAX_CONTEXT_ATOMS;
 * generation_mask, antigen_mask (G,K) uint8 and residue_mask (G,K) uint8 or NULL (all present); chain, residue_idx (G,K) int32.
 * rows = G * group_size, 1 <= group_size <= DIFFAB_METRICS_MAX_GROUP, 1 <= K <= DIFFAB_INTERFACE_MAX_K, contact_distance finite and >= 0.
 *
 * The rule.  Generated residue i of row r (generation_mask and residue_mask) and residue j of its patch are IN CONTACT when j is not
 * generated, is inside residue_mask and antigen_mask, is no chain neighbour of i in either direction (chain equal and residue_idx one
 * apart), and one atom pair (valid atom a of i in the row's points, valid atom b of j in context_points) has d2 < contact^2, with
 * d2 = (dx*dx + dy*dy) + dz*dz in fp32, dx, dy, dz one rounded subtraction each, no contraction, and contact^2 the fp32 product
 * contact_distance * contact_distance; the comparison is strict.  This is diffab_metrics_contacts' arithmetic and eligibility, so the
 * number of set bits of a row is its n_contact_pairs, the set bits of row i of the map its residue_contact, and so on.
 *
 * Outputs.  bits (rows,K,W) int32 with W = (K + 31) / 32: bit j % 32 of word [r][i][j / 32] is set iff i and j are in contact in row r;
 * every other bit is 0 - all words of the rows of non-generated residues, and the bits of j >= K in the last word.  n_contacts (rows)
 * int32 = the number of set bits of the row.  Both are written in full.
 *
 * Limits, DIFFAB_ERR_ARG, decided from the scalars and from which pointers are NULL before anything is enqueued: rows >= 0 a multiple
 * of group_size, group_size, K, P, A and contact_distance as above, a NULL input other than residue_mask, a NULL output, a workspace
 * that is NULL or not 256-byte aligned (too small: DIFFAB_ERR_WORKSPACE).
 *
 * Two launches.  (1) Pack, one work-group per patch: the valid atoms of the antigen residues a contact may have (non-generated, inside
 * both masks, at least one valid atom) compacted in ascending residue order, with the slots of the generated residues and, per word
 * column of 32 slots, where its residues start in the list.  (2) Bits, one work-group per (patch, 64 designs), lane = design: the
 * antigen atoms go through LDS one word column at a time (at most 32 residues and 32 * DIFFAB_METRICS_MAX_CONTEXT_ATOMS atoms, so
 * neither K nor A needs a second chunk size), shared by the 64 designs; the four waves split the generated residues; every lane builds
 * the word of (its design, its generated residue, this column) in a register and stores it once, and the work-group stores the zero
 * words of every other row of its designs in one coalesced sweep.
 * workspace: DIFFAB_METRICS_CONTACT_BITS_WORKSPACE_BYTES(G, K, A) bytes. */
#define DIFFAB_INTERFACE_MAX_K 512
#define DIFFAB_METRICS_CONTACT_BITS_WORKSPACE_BYTES(G, K, A) \
  ((size_t)(G) * (size_t)(K) * ((size_t)(A) * 16 + 28) + (size_t)(G) * (((size_t)(K) + 31) / 32 * 4 + 24) + 2048)
int diffab_metrics_contact_bits(const float* points, const uint8_t* valid, const float* context_points, const uint32_t* context_valid,
                                const uint8_t* generation_mask, const uint8_t* residue_mask, const uint8_t* antigen_mask,
                                const int32_t* chain, const int32_t* residue_idx, int32_t rows, int32_t group_size, int32_t K, int32_t P,
                                int32_t A, float contact_distance, int32_t* bits, int32_t* n_contacts, void* workspace,
                                size_t workspace_bytes, void* stream);

/* diffab_metrics_pairwise_bits: the overlap of the bit sets of the N designs of every patch, all pairs.
 *
 * Input.  bits (G*N, L) int32: design r of patch g is the L words of row g * N + r - a contact map of diffab_metrics_contact_bits goes
 * in as it came out, with L = K * W.  All 32 bits of a word are data, the sign bit included.  1 <= N <= DIFFAB_METRICS_MAX_GROUP,
 * 1 <= L <= DIFFAB_INTERFACE_MAX_WORDS (so every count is below 2^24 and exact as an fp32 number).
 *
 * The rule, per patch, with A and B the sets of designs a and b.
 *   n_set[g,a]      = |A|, the popcount of the L words (int32).
 *   n_common[g,a,b] = |A & B| (int32): symmetric, and the diagonal is n_set.
 *   fcc[g,a,b]      = (float)n_common[a,b] / (float)n_set[a], one correctly rounded fp32 division: the fraction of a's set that b
 *                     shares (the fraction of common contacts; NOT symmetric); 1 where n_set[a] == 0.
 *   jaccard[g,a,b]  = (float)n_common[a,b] / (float)(n_set[a] + n_set[b] - n_common[a,b]), likewise: symmetric to the bit; 1 where both
 *                     sets are empty.
 *
 * Outputs.  n_set (G,N) int32, n_common (G,N,N) int32, fcc (G,N,N) fp32, jaccard (G,N,N) fp32: each may be NULL and is then neither
 * computed for nor written, so one matrix of the largest patch costs one matrix.
 *
 * Limits, DIFFAB_ERR_ARG, decided from the scalars and from which pointers are NULL before anything is enqueued: G >= 0, N and L as
 * above, a NULL bits, a workspace that is NULL or not 256-byte aligned (too small: DIFFAB_ERR_WORKSPACE).
 *
 * Four launches.  A contact map is almost empty by construction - only the rows of generated residues and the words that hold antigen
 * slots can be non-zero - so the pairs are compared over the LIVE word columns only.  (1) Or, one work-group per (patch, 64 designs):
 * the OR of their words, per column, into the workspace.  (2) Compact, one work-group per patch: the OR over those parts, and the
 * columns that are not zero as a list in ascending order (ballots), so the list does not depend on scheduling.  (3) Gather, one
 * work-group per (patch, 64 designs): the live words, column-major with the designs along the fastest axis and padded with zero designs
 * up to a multiple of 64.  (4) Tiles, one work-group of 256 threads per 64 x 64 block of pairs on or above the diagonal, 4 x 4 pairs per
 * thread: the live words of its 64 + 64 designs go through LDS in chunks of DIFFAB_INTERFACE_TILE_COLUMNS columns (a dense input takes
 * more chunks, never more LDS), word c of design d at [c][d], so the sixteen lanes that differ in the b designs read all 64 banks once
 * (128-bit reads) and the a designs are a broadcast; popcount(a & b) adds up in integer registers; the block's counts pass through LDS
 * once more so that both the (a,b) block and its mirror (b,a) leave as whole 256-byte rows.  The mirror is stored from the same integer,
 * so symmetry is by construction.
 * workspace: DIFFAB_METRICS_PAIRWISE_BITS_WORKSPACE_BYTES(G, N, L) bytes. */
#define DIFFAB_INTERFACE_MAX_WORDS 8192
#define DIFFAB_INTERFACE_TILE_COLUMNS 64
#define DIFFAB_INTERFACE_PAD64(N) ((((size_t)(N) + 63) / 64) * 64)
#define DIFFAB_METRICS_PAIRWISE_BITS_WORKSPACE_BYTES(G, N, L)                                                             \
  ((size_t)(G) * ((size_t)(L) * DIFFAB_INTERFACE_PAD64(N) * 4 + (DIFFAB_INTERFACE_PAD64(N) / 64) * (size_t)(L) * 4 +      \
                  (size_t)(L) * 4 + 4) + 2048)
int diffab_metrics_pairwise_bits(const int32_t* bits, int32_t G, int32_t N, int32_t L, int32_t* n_set, int32_t* n_common, float* fcc,
                                 float* jaccard, void* workspace, size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* DIFFAB_HIP_INTERFACE_H */
