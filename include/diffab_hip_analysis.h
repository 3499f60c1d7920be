/* diffab_hip_analysis.h - model-free analysis of sampled designs: the second header of libdiffab_hip.so.
 *
 * Same library, same conventions, same contracts as include/diffab_hip.h - its "General contract" applies word for word: every check is
 * made on the host before anything is enqueued; a refusal returns a negative DIFFAB_ERR_* and leaves its message in diffab_last_error();
 * an empty problem (rows = 0) returns 0 before any pointer is looked at; what a workspace holds on entry is ignored and nothing outside
 * [workspace, workspace + bytes) is written; every element of an output tensor is written; every DATA operand is ACCEPTED at its natural
 * alignment (4 bytes float / int32 / uint32, 1 byte masks: the kernels address caller memory element by element); the workspace is
 * 256-byte aligned, as torch allocates.  A NULL output pointer skips that output.
 *
 * Why a header of its own: the export list of diffab_hip.h is pinned, name by name, by the tables behind the operand-alignment and
 * symbol tests of the sampler's C ABI, and those tables are the record of a finished audit.  Model-free analysis entries added from now
 * on are declared here, typed in _hip.ANALYSIS_SYMBOLS, and bring their contract tests (workspace contents, operand alignment, host-side
 * refusals) in test files of their own.
 */
#ifndef DIFFAB_HIP_ANALYSIS_H
#define DIFFAB_HIP_ANALYSIS_H

#include "diffab_hip.h" /* DIFFAB_OK, DIFFAB_ERR_*, DIFFAB_METRICS_MAX_* */

#ifdef __cplusplus
extern "C" {
#endif

/* diffab_metrics_surface: solvent-accessible surface of the generated residues and of the antigen, and what the two bury on each other
 * (Shrake-Rupley sphere points).  Rows, groups and masks as in "Common layout" of diffab_hip.h: rows = G *
 * group_size, row r belongs to patch g = r / group_size, masks are (G,K), residue_mask NULL = all present.
 *
 * Atoms of row r, for every residue k inside residue_mask:
 *   generated (generation_mask[g,k]): the frame atoms points[r,k,a] (rows,K,P,3), a < P <= DIFFAB_METRICS_MAX_POINTS, whose bit a is set
 *     in valid[r,k] (rows,K) uint8; radius point_radius[a].  point_radius is a HOST array of P floats (it travels as launch arguments
 *     and may be freed on return).  These atoms are the set D.
 *   not generated: the patch's atoms context_points[g,k,a] (G,K,A,3), a < A <= DIFFAB_METRICS_MAX_CONTEXT_ATOMS, whose bit a is set in
 *     context_valid[g,k] (G,K) uint32, shared by the designs of the patch; radius context_radius[g,k,a] (G,K,A) fp32, or the scalar
 *     context_radius_default where that pointer is NULL.  They form the set G (antigen) where antigen_mask[g,k] is set, the set F
 *     (framework) otherwise.  A generated residue is never antigen.  Bits at or above P / A are ignored.
 * With R = radius + probe (one fp32 addition) and the caller's table sphere (S,3) fp32 of S unit vectors u_s,
 * DIFFAB_METRICS_SURFACE_MIN_POINTS <= S <= DIFFAB_METRICS_SURFACE_MAX_POINTS:
 *   sphere point s of atom a with centre c is q = fl(c + fl(R_a * u_s)), component by component;
 *   atom b != a COVERS q iff d2 < fl(R_b * R_b), d2 = (dx*dx + dy*dy) + dz*dz in fp32, dx, dy, dz one rounded subtraction each, no
 *   contraction, the comparison strict (the arithmetic of diffab_metrics_contacts).  Chain neighbours and the other atoms of the same
 *   residue cover like any other atom.
 * Points of a target atom in D:  FREE iff no atom of D or F covers it (the antibody alone);  BOUND iff free and no atom of G covers it.
 * Points of a target atom in G:  FREE iff no atom of G covers it (the antigen alone);  BOUND iff no atom at all covers it;
 *   DESIGN-BURIED iff no atom of G or F covers it but an atom of D does (what the designed residues bury beyond the framework).
 * Atoms of F are occluders only: they have no points and no outputs.
 *
 * Per residue (rows,K) int32: free_points, bound_points (summed over the residue's atoms; 0 on a framework residue or one outside
 * residue_mask), design_buried_points (antigen residues; 0 elsewhere).  Per residue (rows,K) fp32: free_area, bound_area,
 * design_buried_area = sum over the residue's atoms, ascending slot, of n_a * (4 pi R_a^2 / S) in fp64 from the fp32 R_a, rounded once;
 * residue_buried = free - bound area on a generated residue, the design-buried area on an antigen residue (in fp64, rounded once).
 * Per row (rows), fp64 sums over k ascending of the fp64 residue values, rounded once:
 *   bsa_paratope = sum over generated residues of (free - bound);  bsa_epitope = the same over antigen residues;
 *   bsa_design_epitope = sum over antigen residues of the design-buried area;  hotspot_buried_area = the same over the hotspot residues.
 * Per row (rows) int32: n_paratope_buried = generated residues with free_points > bound_points;  n_epitope_buried = antigen residues
 * with design_buried_points > 0;  n_hotspot = non-generated residues inside residue_mask, antigen_mask and hotspot_mask (hotspot_mask
 * needs antigen_mask);  n_hotspot_buried = those of them with design_buried_points > 0.
 * Without antigen_mask the set G is empty: bound = free on the generated residues and every antigen number is 0.  A row whose patch has
 * no generated residue inside residue_mask has nothing to evaluate: every output of the row is 0.  A row's numbers do not depend on the
 * other rows.  No float atomics (no atomics at all); every value reaches memory through plain stores.
 *
 * Limits, DIFFAB_ERR_ARG with the shape and null-pointer checks before anything is enqueued: rows >= 0 a multiple of group_size,
 * 1 <= group_size <= DIFFAB_METRICS_MAX_GROUP, 1 <= K <= DIFFAB_METRICS_MAX_K, P, A and S as above, probe, context_radius_default and
 * every point_radius[a] finite and >= 0, a hotspot_mask without an antigen_mask, a NULL input other than the optional ones
 * (context_radius, residue_mask, antigen_mask, hotspot_mask), a workspace that is NULL or not 256-byte aligned (too small:
 * DIFFAB_ERR_WORKSPACE).  The values of context_radius live on the device and are the caller's to keep finite and >= 0 (an atom whose
 * R is negative or NaN neither covers nor counts).  There is no limit on K * A, on the atoms of a row or on the neighbours of an atom.
 *
 * Up to seven memsets (the per-residue outputs) and three launches: (1) per patch, the valid context atoms are compacted once into the
 * workspace as (x, y, z, R), the antigen's first; (2) per patch, one wave per antigen atom, lane = sphere point in passes of 64, writes
 * two S-bit masks - the points no antigen atom covers, and those no context atom covers - which every design of the patch shares;
 * (3) one work-group per design row, one wave per target residue: a generated atom's points against the row's atoms and the context, an
 * antigen atom's surviving points against the row's atoms only.  A wave collects the neighbours of its atom by centre distance (a cull
 * widened above every fp32 rounding involved, so it cannot change a count) into a list in LDS by ballot compaction and tests its points
 * against the list.  workspace: DIFFAB_METRICS_SURFACE_WORKSPACE_BYTES(G, K, A, S) bytes. */
#define DIFFAB_METRICS_SURFACE_MIN_POINTS 8
#define DIFFAB_METRICS_SURFACE_MAX_POINTS 256
#define DIFFAB_METRICS_SURFACE_WORKSPACE_BYTES(G, K, A, S) \
  ((size_t)(G) * (size_t)(K) * ((size_t)(A) * (16 + 16 * (((size_t)(S) + 63) / 64)) + 20) + (size_t)(G) * 32 + 2048)
int diffab_metrics_surface(const float* points, const uint8_t* valid, const float* point_radius, const float* context_points,
                           const uint32_t* context_valid, const float* context_radius, const uint8_t* generation_mask,
                           const uint8_t* residue_mask, const uint8_t* antigen_mask, const uint8_t* hotspot_mask, const float* sphere,
                           int32_t rows, int32_t group_size, int32_t K, int32_t P, int32_t A, int32_t S, float probe,
                           float context_radius_default, int32_t* free_points, int32_t* bound_points, int32_t* design_buried_points,
                           float* free_area, float* bound_area, float* design_buried_area, float* residue_buried, float* bsa_paratope,
                           float* bsa_epitope, float* bsa_design_epitope, int32_t* n_paratope_buried, int32_t* n_epitope_buried,
                           int32_t* n_hotspot, int32_t* n_hotspot_buried, float* hotspot_buried_area, void* workspace,
                           size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* DIFFAB_HIP_ANALYSIS_H */
