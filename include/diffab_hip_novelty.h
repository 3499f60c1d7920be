/* diffab_hip_novelty.h - is this design new: the nearest sequence of a library of known loops by edit distance, for every design, and the
 * entry that turns the designed residues of a row into such a sequence: the eighth header of libdiffab_hip.so.
 *
 * Why a header of its own: the export lists of include/diffab_hip.h, include/diffab_hip_analysis.h, include/diffab_hip_hbonds.h,
 * include/diffab_hip_cluster.h, include/diffab_hip_interface.h, include/diffab_hip_develop.h and include/diffab_hip_energy.h are each
 * pinned by tests that are the record of finished audits.  The entries that compare a design with sequences that are NOT in its patch -
 * of other lengths, so by alignment - are declared here, typed in _hip.NOVELTY_SYMBOLS onto the same library, and bring their contract
 * tests (workspace contents, operand alignment, guard bands, host-side refusals) in test files of their own.  This header's test asserts
 * that table and header agree, not how many names there are.
 *
 * Same library, same conventions, same contracts as include/diffab_hip.h - its "General contract" applies word for word: every check is
 * made on the host before anything is enqueued; a refusal returns a negative DIFFAB_ERR_* and leaves its message in diffab_last_error();
 * an empty problem (R = 0, rows = 0) returns 0 before any pointer is looked at; what the workspace holds on entry is ignored and nothing
 * outside [workspace, workspace + bytes) is written; every element of every non-NULL output is written, whatever it held, and a NULL
 * output is skipped; every DATA operand is ACCEPTED at its natural alignment (4 bytes int32 / float, 1 byte tokens and masks); the
 * workspace is 256-byte aligned.  No atomics: a query's result depends on that query and the library alone, so a query alone gives the
 * bits it gives among others, and a library cut in two gives two results whose combination is the result of the whole.
 */
#ifndef DIFFAB_HIP_NOVELTY_H
#define DIFFAB_HIP_NOVELTY_H

#include "diffab_hip.h" /* DIFFAB_OK, DIFFAB_ERR_*, DIFFAB_METRICS_MAX_GROUP */

#ifdef __cplusplus
extern "C" {
#endif

#define DIFFAB_NOVELTY_MAX_QUERY 64    /* LQ: tokens of a query row; a query is one bit per position of a 64-bit word */
#define DIFFAB_NOVELTY_MAX_LIBRARY 256 /* LM: tokens of a library row */
#define DIFFAB_NOVELTY_CHUNK 2048      /* library entries of one work-group: the workspace holds one partial result per query and chunk */
#define DIFFAB_NOVELTY_PACK_MAX_K 4096 /* K of diffab_metrics_pack_sequences (DIFFAB_METRICS_MAX_K) */

/* diffab_metrics_edit_nearest: for every query the nearest entry of a library by Levenshtein distance.
 *
 * Inputs.  q_tokens (R,LQ) uint8, q_len (R) int32: the queries; lib_tokens (M,LM) uint8, lib_len (M) int32: the library; skip (R)
 * int32 or NULL; radius int32.  1 <= LQ <= DIFFAB_NOVELTY_MAX_QUERY, 1 <= LM <= DIFFAB_NOVELTY_MAX_LIBRARY, R, M >= 0.
 *
 * The rule.
 *   Sequences.  A sequence is the first len bytes of its row; bytes past len are never read.  Two tokens MATCH iff they are equal and
 *     both are below 32 (DIFFAB_METRICS_MAX_CLASSES, the limit every other entry has): a token of 32 or more matches nothing, itself
 *     included.  Padding is written as 255.
 *   Distance.  d(a, b) is the Levenshtein distance over matches: the least number of single-token insertions, deletions and
 *     substitutions that turns a into b, each at cost 1.  d of two empty sequences is 0; d is symmetric.
 *   Per query r, over the library entries m in [0, M) except m == skip[r] when skip is given (a skip[r] outside [0, M) skips nothing):
 *     distance[r] = the minimum of d(r, m); index[r] = the lowest m that attains it;
 *     identity[r] = 1 - distance / max(len_q, len_lib[index]), both integers exact in fp32, one correctly rounded fp32 division and one
 *       fp32 subtraction; 1 when both lengths are 0;
 *     n_within[r] = the number of those entries with d <= radius; 0 when radius < 0.
 *     With nothing to compare (M = 0, or the only entry skipped): distance = index = -1, identity is NaN, n_within is 0.
 *   Matrix.  With a non-NULL matrix (R,M) int32 every d(r, m) is stored, the skipped entry too.
 *   Bad lengths.  A q_len[r] outside [0, LQ], or a lib_len[m] outside [0, LM], is read as clamped into the range: lengths are device
 *     data, the host cannot refuse them, the clamp is the defined behaviour, and nothing outside the rows is read.
 *
 * Outputs, each may be NULL: distance, index, n_within (R) int32; identity (R) fp32; matrix (R,M) int32.
 *
 * Limits, DIFFAB_ERR_ARG, decided on the host before anything is enqueued: R < 0 or M < 0; LQ or LM outside the ranges above; with
 * R > 0: a NULL q_tokens or q_len; with R > 0 and M > 0: a NULL lib_tokens or lib_len; R * M >= 2^31 when matrix is given; a workspace
 * that is NULL or not 256-byte aligned (too small: DIFFAB_ERR_WORKSPACE).
 *
 * The arithmetic: Myers' bit-vector algorithm in Hyyro's global form, the query as the pattern and a library entry as the text, in
 * 64-bit words of which the addition carries from bit 31 into bit 32.  The query stands at the TOP of the word: with s = 64 - len_q,
 * bit s + i of Peq[c] is set iff query token i is c, c < 32, so that the score is read from bit 63 whatever the length:
 *   Pv = ~0 << s, Mv = 0, score = len_q                   (len_q = 0: the answer is the text's length)
 *   per text token c:  Eq = Peq[c]  (0 when c >= 32)
 *     Xv = Eq | Mv;  Xh = (((Eq & Pv) + Pv) ^ Pv) | Eq;  Ph = Mv | ~(Xh | Pv);  Mh = Pv & Xh
 *     score += Ph >> 63;  score -= Mh >> 63
 *     Ph = (Ph << 1) | 1;  Mh <<= 1;  Pv = Mh | ~(Xv | Ph);  Mv = Ph & Xv
 * The s bits below the query hold no pattern: Eq, Pv and Mv are 0 there and stay 0, Ph is 1 there, and what the shift moves into the
 * query's first bit is the +1 of the first row of a global alignment.  It is the recurrence with the query in the low bits and the
 * score read from bit len_q - 1, moved up by s bits.  All integers: every output is the same on every run and whatever the library
 * is cut into.
 *
 * Three launches.  (1) Repack, one work-group per chunk of DIFFAB_NOVELTY_CHUNK entries: the chunk in the order of its clamped lengths
 * (ties by m; an entry's place is a count of the entries before it, not the outcome of a race), word-major - word w of the entry in
 * place p at [w][p], four tokens each, 255 behind the length - so that the lanes of a wave, one entry each, read consecutive words and
 * finish their texts together.  (2) Distances: a work-group of 256 lanes takes 16 queries and one chunk; it builds the queries' Peq
 * tables in LDS (32 words of 8 bytes each: lanes with different tokens read different banks, lanes with the same token one address;
 * a 33rd word of zeros serves every token that matches nothing); each lane walks the chunk's entries, one per pass, and runs four
 * queries at a time along the entry's words to the entry's own length (the steps of a last word's padding are run and not kept); the
 * matrix is stored from here; per query the wave's minimum key (d, m) and its count within the radius go over the chunk into LDS and
 * from there as one partial per query and chunk into the workspace.  (3) Finish: one lane per query takes the minimum and the integer
 * sum over the chunks - neither depends on an order - and writes the four per-query outputs.
 * workspace: DIFFAB_METRICS_EDIT_NEAREST_WORKSPACE_BYTES(R, M, LM) bytes. */
#define DIFFAB_METRICS_EDIT_NEAREST_WORKSPACE_BYTES(R, M, LM)                                               \
  ((size_t)(M) * ((((size_t)(LM) + 3) / 4) * 4 + 8) +                                                       \
   (((size_t)(M) + DIFFAB_NOVELTY_CHUNK - 1) / DIFFAB_NOVELTY_CHUNK) * (size_t)(R) * 12 + 1024)
int diffab_metrics_edit_nearest(const uint8_t* q_tokens, const int32_t* q_len, int32_t R, int32_t LQ, const uint8_t* lib_tokens,
                                const int32_t* lib_len, int32_t M, int32_t LM, const int32_t* skip, int32_t radius, int32_t* distance,
                                int32_t* index, int32_t* n_within, float* identity, int32_t* matrix, void* workspace, size_t workspace_bytes,
                                void* stream);

/* diffab_metrics_pack_sequences: the counted residues of every design row as one sequence, the form diffab_metrics_edit_nearest reads.
 *
 * Inputs.  tokens (rows,K) int32; mask (G,K) uint8; residue_mask (G,K) uint8 or NULL (all inside); segment_idx (G,K) int32 or NULL (no
 * segment filter, `segment` is ignored); rows = G * group_size, 1 <= group_size <= DIFFAB_METRICS_MAX_GROUP,
 * 1 <= K <= DIFFAB_NOVELTY_PACK_MAX_K, 1 <= L <= DIFFAB_NOVELTY_MAX_LIBRARY.
 *
 * The rule, per row r of patch g = r / group_size.  A slot is counted when it is inside mask[g], inside residue_mask[g], and
 * segment_idx[g] == segment when segment_idx is given.  The tokens of the counted slots are written in slot order into out_tokens[r]; a
 * token outside [0, 255) becomes 255; the row is padded with 255 up to L.  out_len[r] is the full count, even when it exceeds L: the
 * surplus tokens are dropped.
 *
 * Outputs, each may be NULL: out_tokens (rows,L) uint8; out_len (rows) int32.
 *
 * Limits, DIFFAB_ERR_ARG, decided on the host before anything is enqueued: the extents above (rows >= 0 a multiple of group_size); L
 * outside its range; a NULL tokens or mask.  One launch, one wave per row; no workspace. */
int diffab_metrics_pack_sequences(const int32_t* tokens, const uint8_t* mask, const uint8_t* residue_mask, const int32_t* segment_idx,
                                  int32_t segment, int32_t rows, int32_t group_size, int32_t K, int32_t L, uint8_t* out_tokens,
                                  int32_t* out_len, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* DIFFAB_HIP_NOVELTY_H */
