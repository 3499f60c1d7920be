/* diffab_hip_energy.h - does this design bind: a residue-level, distance-binned pair potential between the designed residues and what
 * they touch, per class of partner (antigen, framework, each other), and what every single substitution at a designed position would do
 * to the antigen term: the seventh header of libdiffab_hip.so.
 *
 * Why a header of its own: the export lists of include/diffab_hip.h, include/diffab_hip_analysis.h, include/diffab_hip_hbonds.h,
 * include/diffab_hip_cluster.h, include/diffab_hip_interface.h and include/diffab_hip_develop.h are each pinned by tests that are the
 * record of finished audits.  The entry that scores a designed residue against the residue it touches BY WHAT THE TWO RESIDUES ARE - the
 * first to read the antigen's sequence together with the design's - is declared here, typed in _hip.ENERGY_SYMBOLS onto the same
 * library, and brings its contract tests (workspace contents, operand alignment, guard bands, host-side refusals) in test files of its
 * own.  This header's test asserts that table and header agree, not how many names there are.
 *
 * Same library, same conventions, same contracts as include/diffab_hip.h - its "General contract" applies word for word: every check is
 * made on the host before anything is enqueued; a refusal returns a negative DIFFAB_ERR_* and leaves its message in diffab_last_error();
 * an empty problem (rows = 0) returns 0 before any pointer is looked at; what the workspace holds on entry is ignored and nothing outside
 * [workspace, workspace + bytes) is written; every element of every non-NULL output is written, zeros included, whatever it held, and a
 * NULL output is skipped; every DATA operand is ACCEPTED at its natural alignment (4 bytes float / int32, 1 byte masks); the workspace is
 * 256-byte aligned.  No atomics: a row's result depends on the row and its patch alone, so a patch alone gives the bits it gives in a
 * batch.
 */
#ifndef DIFFAB_HIP_ENERGY_H
#define DIFFAB_HIP_ENERGY_H

#include "diffab_hip.h" /* DIFFAB_OK, DIFFAB_ERR_*, DIFFAB_METRICS_MAX_GROUP */

#ifdef __cplusplus
extern "C" {
#endif

#define DIFFAB_ENERGY_MAX_K 512      /* residues per patch: a row's sites, tokens and chain tables stay in LDS */
#define DIFFAB_ENERGY_MAX_CLASSES 32 /* V: token classes of the table; the substitution scan gives every class a lane of a half wave */
#define DIFFAB_ENERGY_MAX_BINS 8     /* NB: distance bins of the table; the whole table stays in LDS (8 * 32 * 33 * 4 bytes at most) */

/* diffab_metrics_pair_energy: a distance-binned residue pair potential over the pairs a design takes part in.
 * The stand-in of docking and design triage for a binding energy on backbone frames - Miyazawa-Jernigan-style contact energies or
 * paratope-epitope propensities, whatever table the caller brings; no parity with Rosetta's ddG is claimed, which needs side chains.
 *
 * Inputs.  sites (rows,K,3) fp32, one point per residue of every design row; context_sites (G,K,3) fp32, one point per residue of the
 * patch; tokens (rows,K) int32; generation_mask (G,K) uint8; residue_mask, antigen_mask (G,K) uint8 or NULL (all present / no antigen);
 * chain, residue_idx (G,K) int32, both given or both NULL (NULL: the separation rule is off); table (NB,V,V) fp32 on the device;
 * bin_edges, a HOST array float[NB + 1], read during the call only.  rows = G * group_size, 1 <= group_size <= DIFFAB_METRICS_MAX_GROUP,
 * 1 <= K <= DIFFAB_ENERGY_MAX_K, 1 <= V <= DIFFAB_ENERGY_MAX_CLASSES, 1 <= NB <= DIFFAB_ENERGY_MAX_BINS, min_separation >= 0.
 *
 * The rule, per design row r of patch g.
 *   Present.  A residue is present when it is inside residue_mask.  It is generated when it is present and inside generation_mask.
 *   Site.  The site of a present residue is sites[r] if it is generated, else context_sites[g].  The row's sites of non-generated
 *     residues, the patch's sites of generated residues and everything outside residue_mask are never read: they may hold NaN.
 *   Distance.  d2(i,j) = (dx*dx + dy*dy) + dz*dz in fp32, dx, dy, dz one rounded subtraction each, no contraction: the arithmetic of
 *     diffab_metrics_contacts.
 *   Bins.  e2[b] = the fp32 product bin_edges[b] * bin_edges[b].  The pair falls in bin b iff e2[b] <= d2 < e2[b + 1]; a pair below
 *     e2[0] or at or beyond e2[NB] (or with a d2 that is NaN) has no bin.
 *   Separation.  With chain and residue_idx, a pair with chain[i] == chain[j] and |residue_idx[i] - residue_idx[j]| < min_separation,
 *     the difference taken in 64-bit integers, is skipped: chain neighbours are always in contact and say nothing.
 *   Counted pair.  An unordered pair {i,j}, i != j, is counted when both residues are present, at least one is generated, both tokens
 *     lie in [0, V), the pair has a bin and it is not skipped.
 *   Class.  INTERNAL (class 2): both are generated.  ANTIGEN (class 0): the non-generated one is inside antigen_mask.  FRAMEWORK
 *     (class 1): everything else.  A generated residue inside antigen_mask counts as generated.
 *   Term.  table[b][first][second] with the generated residue's token first; for an INTERNAL pair the lower slot's token first.
 *   Sums.  fp64 in a fixed order, rounded to fp32 once.  A residue's sums run over its partners j in ascending j.  A row's sum of a
 *     class adds, per lane, the class sums of the GENERATED residues lane, lane + 64, ... in ascending order, then the 64 lanes over
 *     the fixed tree lane ^ 32, ^ 16, ..., ^ 1; the INTERNAL sum is half of that (every such pair is in the sums of both its ends;
 *     halving is exact).
 *
 * Outputs, each may be NULL.  Per row: e_antigen, e_framework, e_internal (rows) fp32, every pair once; n_pairs (rows,3,NB) int32, the
 * counted pairs per class (0 antigen, 1 framework, 2 internal) and bin.  Per residue: residue_energy (rows,K) fp32, the terms of every
 * counted pair the residue is part of (for an antigen or framework residue: its pairs with generated residues); residue_antigen_energy
 * (rows,K) fp32, those of the ANTIGEN class only; n_partners (rows,K) int32, the counted pairs of the residue.
 * substitution (rows,K,V) fp32: for a generated residue i and class v, S_v - S_cur, where S_v is the fp64 sum over the geometric
 * antigen partners j of i in ascending j of table[b][v][tokens[j]] - j present, not generated, inside antigen_mask, its token in
 * [0, V), the pair with a bin and not skipped - and S_cur = S_{tokens[i]}, or 0 when tokens[i] is outside [0, V); the difference is
 * taken in fp64 and rounded once; 0 for every other residue.  It is what each single substitution at a designed position would do to
 * e_antigen with the structure held.  A NULL substitution skips that work entirely.
 *
 * Limits, DIFFAB_ERR_ARG, decided on the host before anything is enqueued: rows >= 0 a multiple of group_size; group_size, K, V, NB
 * and min_separation as above; a NULL sites, context_sites, tokens, generation_mask, table or bin_edges; exactly one of chain and
 * residue_idx NULL; bin_edges not finite, negative or not strictly ascending, or whose fp32 squares are not finite or not strictly
 * ascending; a workspace that is NULL or not 256-byte aligned (too small: DIFFAB_ERR_WORKSPACE).
 *
 * Two launches.  (1) Pack, one wave per patch: what depends on the patch alone - per slot one 16-byte record of the patch's site and
 * the present, generated and antigen bits (the site of a residue that is not present is NaN: it fails every comparison), and chain and
 * residue_idx (zeros without them) - shared by the designs.  (2) Rows, one wave per design row, up to four waves in a work-group that
 * share one copy of the table in LDS, rows of V padded to an odd length: lane l owns residues l, l + 64, ...; a generated residue walks
 * all slots, any other the ascending list of generated residues, built with ballots.  For the scan the two half waves take the
 * generated residues in turn, lane v of a half holds S_v, and both walk the ascending list of antigen residues.
 * workspace: DIFFAB_METRICS_PAIR_ENERGY_WORKSPACE_BYTES(G, K) bytes. */
#define DIFFAB_METRICS_PAIR_ENERGY_WORKSPACE_BYTES(G, K) ((size_t)(G) * (size_t)(K) * 24 + 1024)
int diffab_metrics_pair_energy(const float* sites, const float* context_sites, const int32_t* tokens, const uint8_t* generation_mask,
                               const uint8_t* residue_mask, const uint8_t* antigen_mask, const int32_t* chain, const int32_t* residue_idx,
                               const float* table, const float* bin_edges, int32_t rows, int32_t group_size, int32_t K, int32_t V, int32_t NB,
                               int32_t min_separation, float* e_antigen, float* e_framework, float* e_internal, int32_t* n_pairs,
                               float* residue_energy, float* residue_antigen_energy, int32_t* n_partners, float* substitution,
                               void* workspace, size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* DIFFAB_HIP_ENERGY_H */
