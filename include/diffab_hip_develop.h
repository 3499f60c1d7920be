/* diffab_hip_develop.h - can this design be made: hydrophobic and charged surface patches of the unbound antibody, and sequence motifs
 * along the chain that do not survive production: the sixth header of libdiffab_hip.so.
 *
 * Why a header of its own: the export lists of include/diffab_hip.h, include/diffab_hip_analysis.h, include/diffab_hip_hbonds.h,
 * include/diffab_hip_cluster.h and include/diffab_hip_interface.h are each pinned by tests that are the record of finished audits.  The
 * entries that read a design's coordinates and its designed SEQUENCE together are declared here, typed in _hip.DEVELOP_SYMBOLS onto the
 * same library, and bring their contract tests (workspace contents, operand alignment, guard bands, host-side refusals) in test files of
 * their own.  This header's test asserts that table and header agree, not how many names there are.
 *
 * Same library, same conventions, same contracts as include/diffab_hip.h - its "General contract" applies word for word: every check is
 * made on the host before anything is enqueued; a refusal returns a negative DIFFAB_ERR_* and leaves its message in diffab_last_error();
 * an empty problem (rows = 0) returns 0 before any pointer is looked at; what the workspace holds on entry is ignored and nothing outside
 * [workspace, workspace + bytes) is written; every element of every non-NULL output is written, zeros included, whatever it held, and a
 * NULL output is skipped; every DATA operand is ACCEPTED at its natural alignment (4 bytes float / int32, 1 byte masks); the workspace is
 * 256-byte aligned.  No atomics: a row's result depends on the row and its patch alone, so a patch alone gives the bits it gives in a
 * batch.
 */
#ifndef DIFFAB_HIP_DEVELOP_H
#define DIFFAB_HIP_DEVELOP_H

#include "diffab_hip.h" /* DIFFAB_OK, DIFFAB_ERR_*, DIFFAB_METRICS_MAX_GROUP */

#ifdef __cplusplus
extern "C" {
#endif

#define DIFFAB_DEVELOP_MAX_K 512      /* residues per patch: a row's sites, weights and state stay in LDS */
#define DIFFAB_DEVELOP_MAX_CLASSES 32 /* V of the two weight tables; the classes a motif word has a bit for */
#define DIFFAB_DEVELOP_MAX_MOTIFS 32  /* M: one bit of motif_start per motif */
#define DIFFAB_DEVELOP_MOTIF_WORDS 4  /* words per motif: a motif is at most four residues long */

/* diffab_metrics_patches: hydrophobic and charged surface patches on one site per residue.  The project's own
 * restatement of the Therapeutic Antibody Profiler's PSH / PPC / PNC (Raybould et al.); no parity with that tool is claimed - it uses
 * closest heavy-atom distances and side-chain relative accessibility, and backbone frames give neither.
 *
 * Inputs.  sites (rows,K,3) fp32, one point per residue of every design row; context_sites (G,K,3) fp32, one point per residue of the
 * patch; tokens (rows,K) int32; generation_mask (G,K) uint8; residue_mask, antigen_mask (G,K) uint8 or NULL (all present / no antigen);
 * exposed_in (rows,K) uint8 or NULL; hydrophobicity (V) and charge (V) fp32, device tables, 1 <= V <= DIFFAB_DEVELOP_MAX_CLASSES.
 * rows = G * group_size, 1 <= group_size <= DIFFAB_METRICS_MAX_GROUP, 1 <= K <= DIFFAB_DEVELOP_MAX_K.  neighbour_distance,
 * vicinity_distance and patch_distance finite and >= 0, min_distance finite and > 0, max_neighbours >= 0.
 *
 * The rule, per design row r of patch g.
 *   Present.  A residue is present when it is inside residue_mask and not inside antigen_mask.  The antigen is ignored entirely -
 *     developability is a property of the unbound antibody - and so is everything outside residue_mask: their sites are never read.
 *   Site.  The site of a present residue is sites[r] if it is generated (generation_mask), else context_sites[g].  The row's sites of
 *     non-generated residues and the patch's sites of generated residues are never read.
 *   Distance.  d2(i,j) = (dx*dx + dy*dy) + dz*dz in fp32, dx, dy, dz one rounded subtraction each, no contraction.  Every comparison
 *     is strict, d2 < c*c, with c*c the fp32 product of the distance with itself: the arithmetic of diffab_metrics_contacts.
 *   Neighbour count.  n_neighbours[i] = the number of present j != i with d2 < neighbour_distance^2; 0 for a residue that is not present.
 *   Scope.  i is in scope when it is present and either generated or with d2 < vicinity_distance^2 to a generated present residue: the
 *     CDR and what it sits on.
 *   Exposure.  i is exposed when it is in scope and n_neighbours[i] <= max_neighbours; with exposed_in, when it is in scope and
 *     exposed_in[r][i] != 0 (the count is still reported).
 *   Weights.  h_i = hydrophobicity[tokens[r][i]], q_i = charge[tokens[r][i]]; a token outside [0, V) gives 0 for both.
 *   Pair term.  Over unordered pairs {i,j} of exposed residues with d2 < patch_distance^2: w_i * w_j / max(d2, min_distance^2) in fp64,
 *     from the fp32 d2, the fp32 product min_distance * min_distance (the max is taken in fp32) and the fp32 table values.
 *     psh: w = h.  ppc: the pairs with q_i > 0 and q_j > 0, w = q.  pnc: the pairs with q_i < 0 and q_j < 0, w = q.
 *   Accumulation.  fp64 in a fixed order, rounded to fp32 once: a residue's sum over its partners j in ascending j; a row's sum is half
 *     the sum of its residues' fp64 sums (every pair is in two of them), added per lane over residues lane, lane + 64, ... in ascending
 *     order and then over a fixed tree of the 64 lanes.
 *
 * Outputs, each may be NULL.  Per row: psh, ppc, pnc (rows) fp32; charge_generated, charge_scope (rows) fp32, the sum of q over the
 * present generated residues and over the residues in scope; n_scope, n_exposed (rows) int32; n_pairs (rows) int32, the unordered pairs
 * of exposed residues with d2 < patch_distance^2.  Per residue: residue_psh, residue_ppc, residue_pnc (rows,K) fp32, the sum of the
 * terms the residue is part of (0 for a residue that is not exposed); n_neighbours (rows,K) int32; state (rows,K) uint8, bit 0 present,
 * bit 1 in scope, bit 2 exposed.
 *
 * Limits, DIFFAB_ERR_ARG, decided from the scalars and from which pointers are NULL before anything is enqueued: rows >= 0 a multiple
 * of group_size; group_size, K, V and the five scalars as above; a NULL sites, context_sites, tokens, generation_mask, hydrophobicity
 * or charge; a workspace that is NULL or not 256-byte aligned (too small: DIFFAB_ERR_WORKSPACE).
 *
 * Two launches.  (1) Pack, one wave per patch: what depends on the patch alone - per slot one 16-byte record of the patch's site and
 * the present and generated bits (the site of a residue that is not present is NaN: it fails every comparison), shared by the designs.
 * (2) Rows, one wave per design row: the records, the row's sites of its generated residues and the weights of its tokens go to LDS;
 * lane l owns residues l, l + 64, ...; a first pass over all j counts neighbours and decides scope and exposure, the exposed residues
 * are listed in ascending order with ballots, and a second pass over that list adds the pair terms of every exposed residue.
 * workspace: DIFFAB_METRICS_PATCHES_WORKSPACE_BYTES(G, K) bytes. */
#define DIFFAB_METRICS_PATCHES_WORKSPACE_BYTES(G, K) ((size_t)(G) * (size_t)(K) * 16 + 1024)
int diffab_metrics_patches(const float* sites, const float* context_sites, const int32_t* tokens, const uint8_t* generation_mask,
                           const uint8_t* residue_mask, const uint8_t* antigen_mask, const uint8_t* exposed_in, const float* hydrophobicity,
                           const float* charge, int32_t rows, int32_t group_size, int32_t K, int32_t V, float neighbour_distance,
                           int32_t max_neighbours, float vicinity_distance, float patch_distance, float min_distance, float* psh, float* ppc,
                           float* pnc, float* charge_generated, float* charge_scope, int32_t* n_scope, int32_t* n_exposed, int32_t* n_pairs,
                           float* residue_psh, float* residue_ppc, float* residue_pnc, int32_t* n_neighbours, uint8_t* state,
                           void* workspace, size_t workspace_bytes, void* stream);

/* diffab_metrics_motifs: sequence motifs along the chain, counted where they touch the design.
 *
 * Inputs.  tokens (rows,K) int32; generation_mask (G,K) uint8; residue_mask (G,K) uint8 or NULL (all present); chain, residue_idx (G,K)
 * int32; motifs, a HOST array int32[M * DIFFAB_DEVELOP_MOTIF_WORDS], 1 <= M <= DIFFAB_DEVELOP_MAX_MOTIFS, read during the call only.
 * Word p of motif m has bit v set iff class v matches at position p (all 32 bits are classes, the sign bit is class 31); a zero word
 * ends the motif, so a motif is one to four residues long.  rows = G * group_size, 1 <= group_size <= DIFFAB_METRICS_MAX_GROUP,
 * 1 <= K <= DIFFAB_DEVELOP_MAX_K.
 *
 * The rule.  A slot exists when it is inside residue_mask.  succ(i), for a slot i that exists, is the lowest slot j that exists with
 * chain[j] == chain[i] and residue_idx[j] == residue_idx[i] + 1 (as integers, no wrap-around) - diffab_metrics_backbone's chain
 * neighbour; j need not be i + 1, and there may be none.  Motif m of length L matches at slot i, for row r, when the L slots i, succ(i),
 * succ(succ(i)), ... all exist, every one's token is in [0, 32), and every token's bit is set in its word.  A match is COUNTED iff at
 * least one of its slots is generated.
 *
 * Outputs, each may be NULL.  motif_count (rows,M) int32, the counted matches of every motif; n_motifs (rows) int32, their sum;
 * motif_start (rows,K) int32, bit m set iff a counted match of motif m starts at slot i - the sign bit is data.
 *
 * Limits, DIFFAB_ERR_ARG, decided on the host before anything is enqueued: rows >= 0 a multiple of group_size; group_size, K and M as
 * above; a NULL tokens, generation_mask, chain, residue_idx or motifs; a motif whose word 0 is zero, or with a non-zero word after a
 * zero word; a workspace that is NULL or not 256-byte aligned (too small: DIFFAB_ERR_WORKSPACE).
 *
 * Two launches.  (1) Successors, one wave per patch: succ (G,K) into the workspace, -1 where there is none, shared by the designs.
 * (2) Rows, one wave per design row: the class bit of every token, succ and the generated bits in LDS, the motif words from the
 * kernel's arguments; lane l owns slots l, l + 64, ... and walks every motif from each of them; the counts are ballots.
 * workspace: DIFFAB_METRICS_MOTIFS_WORKSPACE_BYTES(G, K) bytes. */
#define DIFFAB_METRICS_MOTIFS_WORKSPACE_BYTES(G, K) ((size_t)(G) * (size_t)(K) * 4 + 1024)
int diffab_metrics_motifs(const int32_t* tokens, const uint8_t* generation_mask, const uint8_t* residue_mask, const int32_t* chain,
                          const int32_t* residue_idx, const int32_t* motifs, int32_t rows, int32_t group_size, int32_t K, int32_t M,
                          int32_t* motif_count, int32_t* n_motifs, int32_t* motif_start, void* workspace, size_t workspace_bytes,
                          void* stream);

#ifdef __cplusplus
}
#endif
#endif /* DIFFAB_HIP_DEVELOP_H */
