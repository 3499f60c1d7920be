/* diffab_hip_hbonds.h - backbone hydrogen bonds and secondary structure of sampled designs: the third header of libdiffab_hip.so.
 *
 * Why a header of its own: the export lists of include/diffab_hip.h and include/diffab_hip_analysis.h are both pinned, name by name, by
 * tests that are the record of finished audits (symbols, operand alignment, operand extents).  The entry below is declared here, typed
 * in _hip.HBOND_SYMBOLS onto the same library, and brings its contract tests (workspace contents, operand alignment, guard bands,
 * host-side refusals) in test files of its own.
 *
 * Same library, same conventions, same contracts as include/diffab_hip.h - its "General contract" applies word for word: every check is
 * made on the host before anything is enqueued; a refusal returns a negative DIFFAB_ERR_* and leaves its message in diffab_last_error();
 * an empty problem (rows = 0) returns 0 before any pointer is looked at; what the workspace holds on entry is ignored and nothing outside
 * [workspace, workspace + bytes) is written; every element of every non-NULL output is written and a NULL output is skipped; every DATA
 * operand is ACCEPTED at its natural alignment (4 bytes float / int32 / uint32, 1 byte masks); the workspace is 256-byte aligned.
 */
#ifndef DIFFAB_HIP_HBONDS_H
#define DIFFAB_HIP_HBONDS_H

#include "diffab_hip.h" /* DIFFAB_OK, DIFFAB_ERR_*, DIFFAB_METRICS_MAX_* */

#ifdef __cplusplus
extern "C" {
#endif

/* diffab_metrics_hbonds: Kabsch-Sander (DSSP, 1983) backbone hydrogen bonds and secondary structure of every design row (DESIGN section
 * 4.20).  A defined number like the other filters: every count, partner and state is an exact function of the fp32 inputs.  No parity
 * with the mkdssp program is claimed; the two simplifications are marked (*) below.
 *
 * Rows, groups and masks as in "Common layout" of diffab_hip.h: rows = G * group_size, row r belongs to patch g = r / group_size, masks
 * are (G,K), residue_mask NULL = all present.  chain, residue_idx (G,K) int32 give the CHAIN NEIGHBOURS exactly as for
 * diffab_metrics_backbone: the successor s(k) / predecessor p(k) of slot k is the lowest slot j with chain[j] == chain[k],
 * residue_idx[j] == residue_idx[k] + 1 / - 1, both inside residue_mask; s^n(k) is n successor steps, and a rule that needs a step that
 * does not exist is false.
 *
 * Inputs.  points (rows,K,3,3) fp32: N, CA, C of every residue of every row.  donor_off (rows,K) uint8: the design's token has no amide
 * hydrogen (Pro).  context_points (G,K,A,3) fp32 with context_valid (G,K) uint32, 4 <= A <= DIFFAB_METRICS_MAX_CONTEXT_ATOMS, slots
 * 0..3 = N, CA, C, O; context_donor_off (G,K) uint8.  generation_mask (G,K); residue_mask, antigen_mask, hotspot_mask (G,K) or NULL
 * (hotspot_mask needs antigen_mask).  1 <= K <= DIFFAB_HBONDS_MAX_K: this limit is this entry's own, so that the atoms of a row and its
 * K x K bond bits stay in LDS.
 *
 * Atoms of residue k of row r, k inside residue_mask.  Derived atoms are computed in fp64 from the fp32 atoms in the order written, no
 * contraction, and rounded once per component to fp32; from there on they are fp32 points like the others.  dot(u, v) = (u0*v0 + u1*v1)
 * + u2*v2, |v| = sqrt(dot(v, v)), unit(v) = v / |v| component by component; where |v| = 0 the atom built from it is absent.
 *   N, CA, C: a generated residue takes points[r,k]; any other residue takes context slots 0, 1, 2 and is COMPLETE only if bits 0..2 of
 *     context_valid are all set (a generated residue is always complete).  An incomplete residue has no atoms at all; it keeps its place
 *     in the chain, and nothing is derived from it.
 *   O, the first case that applies: (1) a non-generated complete residue with bit 3 set takes context slot 3;  (2) with a complete
 *     successor s: O = C - 1.231 * unit(unit(CA - C) + unit(N_s - C)), the negative bisector in the peptide plane;  (3) otherwise
 *     O = (CA + 2.153 * e1) - 1.062 * e2, e1 = unit(C - CA), e2 = unit(v - dot(v, e1) * e1), v = N - CA (the ideal placement of the
 *     frame kernel, from the points alone).
 *   H: absent where donor_off (context_donor_off on a non-generated residue) is set, or without a complete predecessor p that has O_p;
 *     otherwise H = N + unit(C_p - O_p) (Kabsch-Sander's placement, 1.0 A).
 *
 * Bond HB(a, d), acceptor a with C and O, donor d with N and H.  Never for d = a or d = s(a).  The pair is tested only when the fp32
 * d2(CA_a, CA_d) < 81.0f, d2 = (dx*dx + dy*dy) + dz*dz with one rounded subtraction per component (the arithmetic of
 * diffab_metrics_contacts): the 9 A cull is part of the rule, as in DSSP.  In fp64 from the fp32 atoms, with r(X, Y) = max(|X - Y|, 0.5):
 *   E = 27.888 * (((1 / r(O,N) + 1 / r(C,H)) - 1 / r(O,H)) - 1 / r(C,N));   HB(a, d) iff E < -0.5.
 *
 * Secondary structure of every residue inside residue_mask, code 0..7 for " HBEGITS" (0 outside it):
 *   turn_n(i) = HB(i, s^n(i)), n = 3, 4, 5.
 *   Helix seeds, p(i) existing: turn_4(p(i)) and turn_4(i) mark H on i..s^3(i); n = 3 gives a G stretch i..s^2(i); n = 5 an I stretch
 *     i..s^4(i).
 *   Bridges between i and j, each with a predecessor and a successor, j not in {i, s(i), s^2(i)} and i not in {j, s(j), s^2(j)}:
 *     parallel(i, j) = [HB(p(i), j) and HB(j, s(i))] or [HB(p(j), i) and HB(i, s(j))];
 *     antiparallel(i, j) = [HB(i, j) and HB(j, i)] or [HB(p(i), s(j)) and HB(p(j), s(i))].
 *   A bridged residue i is E when, for a partner j and a type it has with j, a chain neighbour of i has a bridge of that type with the
 *     matching neighbour of j: parallel s(i) with s(j) or p(i) with p(j); antiparallel s(i) with p(j) or p(i) with s(j).  Otherwise it is
 *     B.  (*) No bulge linking: two ladders separated by a bulge stay two ladders, and a lone bridge next to one stays B.
 *   Bend S: k, p(p(k)) and s(s(k)) complete and, in fp64, dot(u, v) < 0.3420201433256687 * (|u| * |v|) with u = CA_k - CA_pp,
 *     v = CA_ss - CA_k (more than 70 degrees).
 *   Priority H, B, E, G, I, T, S.  A G stretch is taken whole or not at all - every residue of it free of H, B and E - and an I stretch
 *     likewise, free of H, B, E and G (*) (per seed; DSSP's later revisions prefer I over H).  T goes to the residues s^m(i), 0 < m < n,
 *     of a turn_n(i) that have no higher state.
 *
 * Outputs, each nullable.  Per residue, inside residue_mask (outside: NaN, -1, 0):
 *   O, H (rows,K,3) fp32, NaN where absent.
 *   nh_o_partner (rows,K,2) int32: the acceptors of the two lowest-energy bonds of the residue's N-H; o_hn_partner: the donors of the two
 *     lowest-energy bonds of its C=O.  Ties go to the lower slot; -1 where there are fewer.  nh_o_energy, o_hn_energy (rows,K,2) fp32:
 *     E rounded once, 0 where there is none.
 *   bridge_partner (rows,K,2) int32: the two lowest slots j with a bridge of either type, -1 where none; bridge_parallel (rows,K,2)
 *     uint8: parallel(i, j) of that partner (a pair that satisfies both types reads parallel), 0 where none.
 *   ss (rows,K) uint8.
 *   residue_hbonds (rows,K) int32: the bonds the residue takes part in, as acceptor or donor, that have at least one generated end.
 * Per row, over the bonds with at least one generated end (int32 unless noted): n_hbonds; n_hbonds_internal (both ends generated);
 *   n_hbonds_antigen (the other end is not generated and inside antigen_mask; 0 without one); n_hbonds_framework (the rest);
 *   n_hotspot = non-generated residues inside residue_mask, antigen_mask and hotspot_mask, n_hotspot_bonded = those of them in such a
 *   bond (both 0 without a hotspot_mask); hbond_energy fp32 = the fp64 sum of E in ascending (acceptor, donor) order, rounded once;
 *   ss_count (rows,8) int32 = the generated residues inside residue_mask by state.
 * A row's numbers do not depend on the other rows.  No float atomics (integer atomics on LDS only); every value reaches memory through
 * plain stores.
 *
 * Limits, DIFFAB_ERR_ARG with the null-pointer checks before anything is enqueued: rows >= 0 a multiple of group_size, 1 <= group_size <=
 * DIFFAB_METRICS_MAX_GROUP, K and A as above, a hotspot_mask without an antigen_mask, a NULL input other than residue_mask, antigen_mask
 * and hotspot_mask, a workspace that is NULL or not 256-byte aligned (too small: DIFFAB_ERR_WORKSPACE).
 *
 * Two launches.  (1) One work-group per patch: the neighbour table, the patch's own atoms, and the bond bits of every pair of which
 * neither end depends on the row, written once to the workspace as (G, K, ceil(K/32)) words, bit d % 32 of word [a][d / 32] = HB(a, d).
 * An acceptor depends on the row when it is generated, or has no real O and a generated successor; a donor when it is generated or its
 * predecessor is such an acceptor.  (2) One work-group per design row: N, CA, C, O, H of the K residues in LDS, the patch's bits loaded
 * and the row-dependent rows and columns computed, the secondary-structure passes on the bit matrix in LDS, counts reduced on chip.
 * workspace: DIFFAB_METRICS_HBONDS_WORKSPACE_BYTES(G, K, A) bytes (A does not enter today: the context atoms are read in place). */
#define DIFFAB_HBONDS_MAX_K 512
#define DIFFAB_METRICS_HBONDS_WORKSPACE_BYTES(G, K, A) \
  ((size_t)(G) * (size_t)(K) * (8 + 4 * (((size_t)(K) + 31) / 32)) + 0 * (size_t)(A) + 1024)
int diffab_metrics_hbonds(const float* points, const uint8_t* donor_off, const float* context_points, const uint32_t* context_valid,
                          const uint8_t* context_donor_off, const uint8_t* generation_mask, const uint8_t* residue_mask,
                          const uint8_t* antigen_mask, const uint8_t* hotspot_mask, const int32_t* chain, const int32_t* residue_idx,
                          int32_t rows, int32_t group_size, int32_t K, int32_t A, float* O, float* H, int32_t* nh_o_partner,
                          float* nh_o_energy, int32_t* o_hn_partner, float* o_hn_energy, int32_t* bridge_partner,
                          uint8_t* bridge_parallel, uint8_t* ss, int32_t* residue_hbonds, int32_t* n_hbonds, int32_t* n_hbonds_internal,
                          int32_t* n_hbonds_antigen, int32_t* n_hbonds_framework, int32_t* n_hotspot_bonded, int32_t* n_hotspot,
                          float* hbond_energy, int32_t* ss_count, void* workspace, size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* DIFFAB_HIP_HBONDS_H */
