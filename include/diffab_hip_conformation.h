/* diffab_hip_conformation.h - is this shape known: the nearest loop of a library of known loops by backbone-dihedral distance, for every
 * design, and the entry that turns the dihedrals of the designed residues of a row into such a loop: the ninth header of libdiffab_hip.so.
 *
 * Why a header of its own: the export lists of include/diffab_hip.h, include/diffab_hip_analysis.h, include/diffab_hip_hbonds.h,
 * include/diffab_hip_cluster.h, include/diffab_hip_interface.h, include/diffab_hip_develop.h, include/diffab_hip_energy.h and
 * include/diffab_hip_novelty.h are each pinned by tests that are the record of finished audits.  The entries that compare the SHAPE of a
 * design with loops that are not in its patch - frame-free, by dihedral angles - are declared here, typed in _hip.CONFORMATION_SYMBOLS
 * onto the same library, and bring their contract tests (workspace contents, operand alignment, guard bands, host-side refusals) in test
 * files of their own.  This header's test asserts that table and header agree, not how many names there are.
 *
 * Same library, same conventions, same contracts as include/diffab_hip.h - its "General contract" applies word for word: every check is
 * made on the host before anything is enqueued; a refusal returns a negative DIFFAB_ERR_* and leaves its message in diffab_last_error();
 * an empty problem (R = 0, rows = 0) returns 0 before any pointer is looked at; what the workspace holds on entry is ignored and nothing
 * outside [workspace, workspace + bytes) is written; every element of every non-NULL output is written, whatever it held, and a NULL
 * output is skipped; every DATA operand is ACCEPTED at its natural alignment (4 bytes int32 / float, 1 byte masks); the workspace is
 * 256-byte aligned.  No atomics: a query's result depends on that query and the library alone, so a query alone gives the bits it gives
 * among others, and a library cut in two gives two results whose combination (least distance, lower index on a tie, summed counts) is
 * the result of the whole.
 */
#ifndef DIFFAB_HIP_CONFORMATION_H
#define DIFFAB_HIP_CONFORMATION_H

#include "diffab_hip.h" /* DIFFAB_OK, DIFFAB_ERR_*, DIFFAB_METRICS_MAX_GROUP, DIFFAB_METRICS_MAX_K */

#ifdef __cplusplus
extern "C" {
#endif

#define DIFFAB_CONFORMATION_MAX_LENGTH 64 /* LQ, LM: slots of a loop row; one bit of a 64-bit word of defined-bits per slot and angle kind */
#define DIFFAB_CONFORMATION_MAX_ANGLES 3  /* A: angle kinds per residue (a subset of phi, psi, omega) */
#define DIFFAB_CONFORMATION_CHUNK 2048    /* loops of one work-group of the ordering, and sorted library places per partial result */

/* diffab_metrics_dihedral_nearest: for every query loop the nearest loop of a library, among those of its own length, by the mean of
 * 2 (1 - cos(difference)) over the backbone dihedrals both have.
 *
 * Inputs.  q_feat (R,LQ,A,2) fp32, q_len (R) int32: the queries; lib_feat (M,LM,A,2) fp32, lib_len (M) int32: the library; skip (R)
 * int32 or NULL; radius fp32; min_terms int32 >= 1.  1 <= LQ, LM <= DIFFAB_CONFORMATION_MAX_LENGTH, 1 <= A <=
 * DIFFAB_CONFORMATION_MAX_ANGLES, R, M >= 0.
 *
 * The rule.
 *   Loops.  A loop is the first len slots of its row, A angles per slot, each held as its features (cos, sin); slots past len are never
 *     read.  A len outside [0, L] is read as clamped into the range: lengths are device data, the host cannot refuse them, the clamp is
 *     the defined behaviour.  A term (slot i, angle a) of a loop is DEFINED when both of its numbers are finite.  The entry never takes
 *     a cosine: every output is a function of the fp32 features as given.  Features outside [-1, 1] are the caller's business: the
 *     result is whatever the IEEE chain below gives, and nothing but the outputs is affected.
 *   Pair (query r, library entry m).  The pair is COMPARABLE iff the clamped lengths are equal and n >= min_terms, n being the number of
 *     terms defined in both.  For a comparable pair
 *       acc = the fp32 fmaf chain over the terms defined in both, from +0, slots ascending, angles ascending within a slot, the cos
 *             product before the sin product: acc = fmaf(q, l, acc); a term undefined on either side takes no part (it is held as 0);
 *       t   = acc / n, one correctly rounded fp32 division;
 *       d   = (t >= 1) ? +0 : 2 - 2 * t, one more rounding.
 *     For unit vectors d is the mean of 2 (1 - cos(difference)) over the compared angles and lies in [0, 4]; North, Lehmann and
 *     Dunbrack's D over phi and psi is 2 * d.  A pair that is not comparable has d = +inf.
 *   Per query r, over the library entries m in [0, M) except m == skip[r] when skip is given (a skip[r] outside [0, M) skips nothing):
 *     distance[r] = the least d; index[r] = the lowest m that attains it; n_terms[r] = n of that pair;
 *     n_within[r] = the number of those entries with d <= radius, one fp32 compare; 0 for a negative or NaN radius.
 *     With nothing comparable: distance = +inf, index = -1, n_terms = 0.
 *   Matrix.  With a non-NULL matrix (R,M) fp32 every d(r, m) is stored, the skipped entry's too.
 *
 * Outputs, each may be NULL: distance (R) fp32; index, n_terms, n_within (R) int32; matrix (R,M) fp32.
 *
 * Limits, DIFFAB_ERR_ARG, decided on the host before anything is enqueued: R < 0 or M < 0; LQ, LM or A outside the ranges above;
 * min_terms < 1; with R > 0: a NULL q_feat or q_len; with R > 0 and M > 0: a NULL lib_feat or lib_len; R * M >= 2^31 when matrix is
 * given; a workspace that is NULL or not 256-byte aligned (too small: DIFFAB_ERR_WORKSPACE).
 *
 * The arithmetic.  2 (1 - cos(a - b)) = 2 - 2 (cos a cos b + sin a sin b): the comparison is a dot product of the features, k = 2 A len
 * long, with a per-pair epilogue.  The product runs on v_mfma_f32_16x16x4_f32, whose result is bit for bit the k-ordered fmaf chain of
 * the rule; an undefined term is stored as 0 on its side, and a chain is padded with zeros, which add nothing.  n is the popcount of
 * mask_q & mask_l over the A words of defined-bits.  For d >= 0 the fp32 bits order as integers, so (bits(d) << 32) | m is one 64-bit
 * minimum that also settles ties to the lower index.
 *
 * Five launches.  Only loops of equal length are compared, so both sides are brought into the order of their (clamped length, index)
 * once per call: (1) a histogram over the 65 lengths per chunk of DIFFAB_CONFORMATION_CHUNK loops; (2) a scan, one lane per length; (3) the
 * placement: a loop's place is the number of loops with a smaller (length, index) - a count, never the outcome of a race - and at its
 * place go its length and index, its A mask words and its features, undefined terms zeroed, in tiles of 16 places, k-major, so that one
 * k-step of the product is one contiguous load of 64 floats.  (4) Distances: a work-group of 256 lanes takes 64 sorted queries and one
 * chunk of sorted library places; it walks only the places whose lengths occur among its queries, each wave two tiles of 16 entries at
 * a time against the four query tiles, and runs the epilogue per accumulator element - n, the division, the clamp, the matrix store,
 * the compare with the radius, the running least key; key and count go over the wave by shuffles into LDS and from there as one
 * partial per query and chunk into the workspace.  (5) Finish: one lane per query takes the minimum and the integer sum over the chunks
 * - neither depends on an order - and writes the four per-query outputs.  With M = 0 one launch writes them.
 * workspace: DIFFAB_METRICS_DIHEDRAL_NEAREST_WORKSPACE_BYTES(R, M, LQ, LM, A) bytes. */
#define DIFFAB_CONFORMATION_SIDE_BYTES(n, L, A)                                                                    \
  ((((size_t)(n) + 15) / 16) * (((size_t)2 * (size_t)(A) * (size_t)(L) + 3) / 4) * 256 +                           \
   (size_t)(n) * (8 * (size_t)(A) + 12) + (((size_t)(n) + DIFFAB_CONFORMATION_CHUNK - 1) / DIFFAB_CONFORMATION_CHUNK) * 260)
#define DIFFAB_METRICS_DIHEDRAL_NEAREST_WORKSPACE_BYTES(R, M, LQ, LM, A)                                           \
  (DIFFAB_CONFORMATION_SIDE_BYTES(R, LQ, A) + DIFFAB_CONFORMATION_SIDE_BYTES(M, LM, A) +                           \
   (((size_t)(M) + DIFFAB_CONFORMATION_CHUNK - 1) / DIFFAB_CONFORMATION_CHUNK) * (size_t)(R) * 12 + 8192)
int diffab_metrics_dihedral_nearest(const float* q_feat, const int32_t* q_len, int32_t R, int32_t LQ, const float* lib_feat,
                                    const int32_t* lib_len, int32_t M, int32_t LM, int32_t A, const int32_t* skip, float radius,
                                    int32_t min_terms, float* distance, int32_t* index, int32_t* n_terms, int32_t* n_within, float* matrix,
                                    void* workspace, size_t workspace_bytes, void* stream);

/* diffab_metrics_pack_dihedrals: the dihedrals of the counted residues of every design row as one loop, the form metrics.conformation
 * turns into features.
 *
 * Inputs.  phi, psi, omega (rows,K) fp32, as diffab_metrics_backbone wrote them; mask (G,K) uint8; residue_mask (G,K) uint8 or NULL (all
 * inside); segment_idx (G,K) int32 or NULL (no segment filter, `segment` is ignored); rows = G * group_size,
 * 1 <= group_size <= DIFFAB_METRICS_MAX_GROUP, 1 <= K <= DIFFAB_METRICS_MAX_K, 1 <= L <= DIFFAB_CONFORMATION_MAX_LENGTH.
 *
 * The rule, per row r of patch g = r / group_size, is the slot rule of diffab_metrics_pack_sequences.  A slot is counted when it is inside
 * mask[g], inside residue_mask[g], and segment_idx[g] == segment when segment_idx is given.  The three angles of the counted slots are
 * copied in slot order into out_angles[r] as (phi, psi, omega), bit for bit, NaNs included; the row is padded with NaN up to L.
 * out_len[r] is the full count, even when it exceeds L: the surplus slots are dropped.
 *
 * Outputs, each may be NULL: out_angles (rows,L,3) fp32; out_len (rows) int32.
 *
 * Limits, DIFFAB_ERR_ARG, decided on the host before anything is enqueued: the extents above (rows >= 0 a multiple of group_size); L
 * outside its range; a NULL phi, psi, omega or mask.  One launch, one wave per row, ranks by ballot; no workspace. */
int diffab_metrics_pack_dihedrals(const float* phi, const float* psi, const float* omega, const uint8_t* mask, const uint8_t* residue_mask,
                                  const int32_t* segment_idx, int32_t segment, int32_t rows, int32_t group_size, int32_t K, int32_t L,
                                  float* out_angles, int32_t* out_len, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* DIFFAB_HIP_CONFORMATION_H */
