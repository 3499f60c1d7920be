// denoiser_internal.h - launchers shared between denoiser_generic.hip, denoiser_fast.hip and api.hip.
#pragma once
#include "common.h"

namespace diffab {

// generic (any dims)
int launch_linear_generic(const float* X, int ldx, const float* W, const float* bias, float* Y, int ldy, int M, int N, int Kd, bool relu,
                          hipStream_t st);
size_t ipa_generic_workspace_floats(const diffab_dims* d);
// ctx_of_row (here and in ipa_layer_fast / launch_ipa_module_persistent): shared contexts - device [B] map, the pair rows of state row b
// are those of context ctx_of_row[b] of the n_ctx patches in e / pair_planes; nullptr: the identity (n_ctx = B)
int ipa_layer_generic(const diffab_dims* d, const diffab_ipa_layer_weights* w, const float* x, const float* e, const float* R, const float* t,
                      float* y, float* ws, hipStream_t st, const int* ctx_of_row = nullptr);
int launch_embed_concat(const float* res_ctx, const float* emb, const int64_t* seq, int D, int64_t rows, float* out, hipStream_t st);
int launch_beta_concat(const float* h, const float* beta, int D, int K, int64_t rows, float* out, hipStream_t st);
int launch_heads_finish(const float* v, const float* O_t, const float* logits, int V, int64_t rows, float* O0, float* post, hipStream_t st);
// noslp_kernels.hip (compiled without the SLP vectoriser: no packed fp32 arithmetic from scalar code)
int launch_proj_frames_f32(const float* x, const float* const* W6, const float* R, const float* t, float* proj, int rows, hipStream_t st);
int launch_losses_bwd(const float* post, const float* tpost, const float* eps, const float* teps, const float* O0, const float* tO,
                      const float* O_t, const float* v, const uint8_t* gm, const uint8_t* rm, const float* count, const float* up, int V,
                      int64_t rows, float* d_logits, float* d_eps, float* d_v, hipStream_t st);
int launch_heads_cotangent(const float* post, const float* c_post, const float* c_eps, const float* c_O0, const float* O_t, const float* v,
                           int V, int64_t rows, float* d_logits, float* d_eps, float* d_v, float* d_Ot, hipStream_t st);
int launch_ipa_frames_bwd(const float* proj, const float* dproj, int NP, int pt_col0, int n_pts, const float* feat, const float* dfeat, int F,
                          int ol_col0, int on_col0, int n_vpts, const float* R, const float* t, float* dR, float* dt, int rows,
                          hipStream_t st);

// The launch forms of the dense tiles of the MFMA path.  Each launcher picks its kernel instantiation from the row count rows = B K
// alone, through these functions (host arithmetic; diffab_debug_dense_forms reports them, tests/test_launch_forms_host.py pins both
// sides of every threshold and DESIGN 4.3 has the table).  kDenseFillGroups is a constant of this code, not the device's CU count.
constexpr int kDenseTileRows = 128;    // rows of a projection / x-stationary tile and of an MLP-chain group
constexpr int kDenseFillGroups = 256;  // "the groups fill the chip"
constexpr int kPartsTilesMax = 64;     // 64-row tiles up to which the row GEMM takes its (row tile, k part) form
// launch_rowgemm128_h3p / _b6p: rows per work-group - 0: the (row tile, k part) form (parts_usable: the caller gave 16-byte aligned
// parts scratch and the contraction has more than one part), 128 when 128-row groups fill the chip, else 64
inline int rowgemm128_rows_per_group(int M, bool parts_usable) {
  if (parts_usable && (M + 63) / 64 <= kPartsTilesMax) return 0;
  return (M + kDenseTileRows - 1) / kDenseTileRows >= kDenseFillGroups ? 128 : 64;
}
// the FULL instantiations (no row guards): launch_proj_frames_h3p / _f32, launch_xstat_h3, launch_xstat (b6)
inline bool dense_tile_full(int rows) { return rows % kDenseTileRows == 0; }
// launch_proj_frames_h3p, launch_xstat_h3, launch_xstat (b6): work-groups per row tile, each with its share of the nblocks column
// blocks - half the chip or less: several (the SPLIT instantiations are nsplit > 1)
inline int dense_tile_nsplit(int rows, int nblocks) {
  const int ntiles = (rows + kDenseTileRows - 1) / kDenseTileRows, nsplit = kDenseFillGroups / ntiles;
  return nsplit < 1 ? 1 : (nsplit > nblocks ? nblocks : nsplit);
}

// MFMA path for the benchmark geometry (D=128, C=64, H=8, DS=32, PQ=PV=8, K % 16 == 0)
bool fast_path_supported(const diffab_dims* d);
size_t ipa_fast_workspace_floats(const diffab_dims* d);
int ipa_layer_fast(const diffab_dims* d, const diffab_ipa_layer_weights* w, const float* x, const float* e, const float* R, const float* t,
                   float* y, float* ws, hipStream_t st,
                   float* sp_keep = nullptr, float* d2_keep = nullptr,  // training tape: three launches, P and d2 kept in these buffers
                   const void* planes = nullptr,  // ipa_layer_split_weights() output; nullptr: split per call into the workspace tail
                   const float* pair_planes = nullptr,  // launch_pair_split() output: attention's pair-tile products on f16 MFMA
                   bool fp32_gemm = false,
                   bool taped = false,   // ws is a slot of the training tape: proj and feat are read by the backward (no scratch use)
                   const unsigned char* tile_needed = nullptr,  // [B][K / 16]: row tiles whose outputs are read (nullptr: all)  // DIFFAB_FLAG_FP32_GEMM: dense products on the f32-input MFMA kernels
                   const int* ctx_of_row = nullptr, int n_ctx = 0);  // shared contexts (inference only; n_ctx 0: d->B)
// fp16 planes of the pair embedding for the fused attention kernel (K = 64 / 128): pair_planes_floats(d) floats, 256-byte aligned.
// n_pair: patches of the pair embedding, 0 = d->B (shared contexts: n_ctx - the planes are built once per context, not per state row)
bool pair_planes_supported(const diffab_dims* d);
size_t pair_planes_floats(const diffab_dims* d, int n_pair = 0);
int launch_pair_split(const diffab_dims* d, const float* e, float* planes, hipStream_t st, int n_pair = 0);
const float* pair_row_scales(const diffab_dims* d, const float* planes, int n_pair = 0);  // {s_i, 1 / s_i} per pair row (b, i) of a launch_pair_split() buffer
// Y = act(X W^T + b) on MFMA; requires Kd % 4 == 0 (falls back to the generic kernel otherwise)
int launch_linear(const float* X, int ldx, const float* W, const float* bias, float* Y, int ldy, int M, int N, int Kd, bool relu,
                  hipStream_t st);

// Y[M x 128] = act(X[:, 0:Kd] W[:, 0:Kd]^T + bias row), W rows ldw floats apart (4-byte aligned), bias row = bias (vector) or
// bias[128 * bias_idx[row]] or bias[128 * (row / bias_div)]; requires rowgemm128_ok()
bool rowgemm128_ok(const float* X, int ldx, const float* Y, int ldy, int M, int Kd);
int launch_rowgemm128(const float* X, int ldx, const float* W, int ldw, const float* bias, const int64_t* bias_idx, int bias_div, float* Y,
                      int ldy, int M, int Kd, bool relu, hipStream_t st);
// gemm_bf16x6.hip: the same products on the bf16 matrix cores, fp32-accurate (three-way bf16 split of both operands, six partial
// products, fp32 accumulation).  The weights are split once into bf16 planes (launch_wsplit128: per call, or once per trajectory by
// the reverse sampler) and the ...p launchers take the planes.
size_t rowgemm128_b6_scratch_bytes(int Kd);
bool rowgemm128_b6_ok(const float* X, int ldx, const float* Y, int ldy, int M, int Kd);
int launch_wsplit128(const float* W, int ldw, int Kd, void* planes, hipStream_t st, int nrows = 128);  // rows >= nrows: zero planes
// X[M x 128] through 2 or 3 dense 128-wide layers in ONE kernel (ReLU between them, the last layer n_out <= 128 columns wide,
// activations stay in LDS); layer 0's bias may be a table indexed per row like launch_rowgemm128's
int launch_mlp_chains_b6(const float* X, int ldx, int nchains, const void* const* planes, const float* const* bias, const int64_t* bias_idx0,
                         int bias_div0, int nlayers, const int* n_out, float* const* Y, const int* ldy, int M, hipStream_t st);
struct MlpChainSet;  // mlp_chain_tile.h
// the descriptors of up to three chains (the by-value kernel argument of mlp_chain_b6_kernel; also handed to the module kernel)
int make_mlp_chain_set(MlpChainSet* out, int nchains, const void* const* planes, const float* const* bias, const int64_t* bias_idx0,
                       int bias_div0, int nlayers, const int* n_out, float* const* Y, const int* ldy);
int launch_mlp_chain_b6(const float* X, int ldx, const void* const* planes, const float* const* bias, const int64_t* bias_idx0, int bias_div0,
                        int nlayers, int n_out, float* Y, int ldy, int M, hipStream_t st);
int launch_wsplit128_strided(const float* W, int64_t sn, int64_t sk, int kseg, int k0, void* planes, hipStream_t st);  // (n, k) = W[n sn + k sk]
int launch_wsplit128_segs(const float* const* W, const int* k_end, int nseg, void* planes, hipStream_t st);  // W_q[k][n] stacked along k
int launch_rowgemm128_b6p(const float* X, int ldx, const void* planes, const float* bias, const int64_t* bias_idx, int bias_div, float* Y,
                          int ldy, int M, int Kd, bool relu, hipStream_t st, float* parts = nullptr);
size_t rowgemm128_b6_parts_floats(int M, int Kd);  // scratch of the k-parts form (few row tiles)
size_t rowgemm128_h3_parts_floats(int M, int Kd);
int launch_rowgemm128_b6(const float* X, int ldx, const float* W, int ldw, const float* bias, const int64_t* bias_idx, int bias_div, float* Y,
                         int ldy, int M, int Kd, bool relu, void* scratch, hipStream_t st);
bool use_b6_gemm(uint32_t flags = 0);  // false with DIFFAB_FLAG_FP32_GEMM (experimental builds: or DIFFAB_FP32_GEMM=1 in the environment)
// the x-stationary product Y[rows x N] = X[rows x 128] W'^T, (n, k) of W' = W[n sn + k sk] (to_out input gradient; a test reference of
// launch_xstat_h3)
size_t xstat_b6_scratch_bytes(int N);
// gemm_f16x3.hip: C[N1 x N2] += A^T B as three fp16 terms (launch_gemm_tn_b6's contract)
int launch_gemm_tn_h3(const float* A, int lda, const float* B, int ldb, float* C, int ldc, int M, int N1, int N2, float* db,
                      float* const* seg_ptrs, const int* seg_ends, int nseg, hipStream_t st);
size_t xstat_h3_scratch_bytes(int N);  // gemm_f16x3.hip: the same product as three fp16 terms
int launch_xstat_h3(const float* X, const float* W, int64_t sn, int64_t sk, float* Y, int ldy, int rows, int N, void* scratch, hipStream_t st);
int launch_xstat_b6(const float* X, const float* W, int64_t sn, int64_t sk, float* Y, int ldy, int rows, int N, void* scratch, hipStream_t st);
// weight-gradient product C[N1 x N2] += A[M x N1]^T B[M x N2] (transposing LDS reads), any widths / row strides; rows of C optionally
// spread over nseg matrices (a test reference of launch_gemm_tn_h3; gemm_tn_b6_ok is the contract of both)
bool gemm_tn_b6_ok(const float* A, int lda, const float* B, int ldb, int M, int N1, int N2);
int launch_gemm_tn_b6(const float* A, int lda, const float* B, int ldb, float* C, int ldc, int M, int N1, int N2, float* db,
                      float* const* seg_ptrs, const int* seg_ends, int nseg, hipStream_t st);  // db (nullable): += column sums of A
// split planes of one IPA layer's projection and to_out weights: ipa_layer_planes_bytes() bytes, 256-byte aligned
size_t ipa_layer_planes_bytes();
size_t ipa_layer_small_offset();       // fp32 copies of w_bias [8][64], gamma [8] (padded to 64), b_out [128] in front of the planes
size_t ipa_layer_h3_pj_offset();       // gemm_f16x3.hip: the projections' two-piece fp16 planes,
size_t ipa_layer_h3_out_offset();      //   to_out's,
size_t ipa_layer_h3_wis_offset();      //   and 1 / scale per output column: [1344 | 128] floats
// gemm_f16x3.hip: the two big dense products of a layer as three-term fp16 split products (half the matrix-pipe work of bf16x6)
size_t rowgemm128_h3_planes_bytes(int Kd);
size_t proj_frames_h3_planes_bytes();
int launch_wsplit128_h3(const float* W, int ldw, int Kd, void* planes, float* wis, hipStream_t st, int nrows = 128);
int launch_pjsplit_h3(const float* const* W6, void* planes, float* wis, hipStream_t st);
int launch_rowgemm128_h3p(const float* X, int ldx, const void* planes, const float* wis, const float* bias, const int64_t* bias_idx, int bias_div,
                          float* Y, int ldy, int M, int Kd, bool relu, hipStream_t st, float* parts = nullptr);
int launch_proj_frames_h3p(const float* x, const void* planes, const float* wis, const float* R, const float* t, float* proj, int rows,
                           hipStream_t st);
int ipa_layer_split_weights(const diffab_ipa_layer_weights* w, void* planes, hipStream_t st);
// ipa_persistent.hip: all NL layers of the IPA module for K = 128 patches as ONE patch-resident launch (one work-group owns a patch
// through projections -> 8 attention row tiles -> to_out, layer after layer; no inter-CU synchronisation).  xa: input, the result is in
// (NL odd ? xb : xa).  planes: NL x ipa_layer_planes_bytes(); pair_planes: launch_pair_split(); ws: proj | feat (ipa_fast_workspace_floats)
bool ipa_module_persistent_supported(const diffab_dims* d);
int launch_ipa_module_persistent(const diffab_dims* d, float* xa, float* xb, const float* R, const float* t, float* ws, const void* planes,
                                 const float* pair_planes, hipStream_t st, const float* emb_X = nullptr, const MlpChainSet* emb = nullptr,
                                 const MlpChainSet* heads = nullptr, const int* ctx_of_row = nullptr, int n_ctx = 0,
                                 const int* last_layer_rows = nullptr,  // launch_row_plan's [B][2 + K / 16] ints
                                 const unsigned char* start_class = nullptr);  // launch_start_classes (null: the static classes)
int module_stagger_classes();  // the classes the module launch spreads its work-groups' starts over (<= 1: no stagger)
void set_module_stagger(int ticks, int classes);  // diagnostics: start-up stagger of the persistent module kernel (10 ns ticks)
void set_module_stamps(void* device_buffer);      // diagnostics: phase stamps of the persistent module kernel
// bias tables of the folded concatenations (see denoiser_fast.hip): emb_tab[25][D] depends on the weights only; beta_tab[3 heads][B][D]
// takes beta[b] per patch, or sched_beta[t] (t = *t_dev when t_dev is given) for every patch
int launch_fold_embed_table(const diffab_dims* d, const diffab_denoiser_weights* w, float* emb_tab, hipStream_t st);
int launch_fold_beta_table(const diffab_dims* d, const diffab_denoiser_weights* w, const float* beta, float* beta_tab, hipStream_t st,
                           const float* sched_beta = nullptr, int t = 0, const int* t_dev = nullptr);

// pair_embed_fused.hip: PairEmbedding forward as one kernel (C = 64, K % 128 == 0, A <= 16); context_kernels.hip falls back to its
// unfused launches elsewhere.  prep: pair_embed_fused_prep_floats(d) floats (prepared planes and tables, rebuilt per call); tapes
// (all or none): the four hidden activations [nrows][64] of rows [row0, row0 + nrows) for the backward; out == nullptr: tapes only
bool pair_embed_fused_supported(const diffab_ctx_dims* d);
size_t pair_embed_fused_prep_floats(const diffab_ctx_dims* d);
int launch_pair_embed_fused(const diffab_ctx_dims* d, const diffab_pair_emb_weights* w, const int64_t* seq_idx, const float* distmat,
                            const float* xyz, const float* pairwise_dihedrals, const int64_t* residue_idx, int32_t residue_idx_batch_stride,
                            const int64_t* chain_idx, const float* atom_mask, const uint8_t* sequence_context_mask, float* out, float* prep,
                            float* tape_h1, float* tape_df, float* tape_m1, float* tape_m2, int64_t row0, int64_t nrows, hipStream_t st,
                            const float** coef_sp_out = nullptr);
int launch_softplus_table(const float* coefw, int n, float* out, hipStream_t st);  // softplus(pair2distcoef) (context_kernels.hip)

// attention_split.hip: the attention of one IPA layer as three launches (logits | pair stream | P x V) exchanging the
// (B, 8, K, K) logits / probabilities through SP - the form the training tape keeps; single key chunk only (K = 64, 128)
bool attention_split_supported(const diffab_dims* d);
size_t attention_split_workspace_floats(const diffab_dims* d);
int launch_ipa_logits(const diffab_dims* d, const float* proj, const float* gamma, float* SP, hipStream_t st);  // S[b][h][i][j] only
int launch_attention_probs(const diffab_dims* d, const float* proj, const float* e, const float* Wb, const float* gamma, float* P,
                           float* D2, hipStream_t st);  // training backward: normalised probabilities + squared point distances
// d pair_ctx of all layers in one pass (attention_split.hip): P / G [B][8][K][K], doe [B K][512], Wb [8][64] per layer
constexpr int kDeLayersMax = 6;
int launch_pair_de_layers(const diffab_dims* d, int nl, const float* const* P, const float* const* G, const float* const* doe,
                          const float* const* Wb, float* de, hipStream_t st);
int launch_pair_stream_bwd(const diffab_dims* d, const float* e, const float* P, float* G /* in dA_kv, out g */, const float* D2,
                           const float* dfeat, float* wb_part, const float* Wb, float* de /* nullable: += d pair_ctx */,
                           hipStream_t st);  // training backward: g, d gamma / d w_bias partials, d e
int launch_attention_split(const diffab_dims* d, const float* proj, const float* e, const float* R, const float* t, const float* Wb,
                           const float* gamma, float* feat, float* SP, hipStream_t st, float* D2 = nullptr);

void set_stream_order(bool on);  // api.hip: the cross-stream ordering guard (common.h StreamOrder)
int set_attn_variant(int v);  // reference paths for tests: 4 = unfused PairEmbedding launches, 64 = separate PairEmbedding backward launches
void set_attn_stamps(void* device_buffer);  // diagnostics: per-wave s_memtime stamps of the attention kernel's phases

// api.hip: opt-in hipEvent bracket around the dominant (attention) kernel
void timer_begin(hipStream_t st);
void timer_end(hipStream_t st);
bool kernel_timer_enabled();

// Derived widths of a call's dims, host side (the kernels keep their own copies): rows = B K, NP = the columns of a projection row
// [q_s | k_s | v_s | q_pts | k_pts | v_pts], F = the columns of a feature row [o_s | o_e | o_l | o_n], HKK = one [B][H][K][K] image
struct Geometry {
  int rows, NP, F;
  size_t HKK;
  explicit Geometry(const diffab_dims* d)
      : rows(d->B * d->K), NP(3 * d->H * d->DS + 2 * d->H * d->PQ * 3 + d->H * d->PV * 3),
        F(d->H * d->DS + d->H * d->C + d->H * d->PV * 3 + d->H * d->PV), HKK(static_cast<size_t>(d->B) * d->H * d->K * d->K) {}
  size_t per_row(size_t n) const { return static_cast<size_t>(rows) * n; }  // floats of a [rows][n] buffer
};

// denoiser_backward.hip: what a taped forward and its backward do, decided once per call by plan_backward.  The tape layout, the
// backward's workspace layout, the taped forwards (api.hip) and run_backward all read it.
constexpr int kMaxLayers = 16;
struct BackwardPlan {
  bool fast;           // benchmark geometry (fast_path_supported): the taped layers run the MFMA kernels, the tape ends in their weight planes
  bool probs_on_tape;  // ... and K = 64 / 128: the three-launch attention leaves P and d2 of every layer on the tape, the backward reads them
  bool de_slots;       // ... and NL <= kDeLayersMax: g and d o_e of every layer have workspace slots - d pair_ctx can be one pass (C = 64, H = 8)
  bool split_planes;   // D = 128: the input-gradient products of to_out and of the projections read the weights as split bf16 planes
};
BackwardPlan plan_backward(const diffab_dims* d);
// saved activations of one training forward (every buffer written by the forward kernels themselves)
struct TrainTape {
  float *cat2, *h1, *x[kMaxLayers + 1], *ipa_ws[kMaxLayers], *cat3, *t1[3], *t2[3], *vbuf, *logits;
  float* scratch;  // 1024 floats: partial sums of the loss reduction
  void* planes;    // ipa_layer_planes_bytes(): the current layer's split weights for the bf16x6 forward GEMMs (null off the MFMA path)
  // per layer with BackwardPlan::probs_on_tape (else null): the attention probabilities and the squared point distances [b][h][i][j]
  float *sp[kMaxLayers], *d2[kMaxLayers];
  size_t floats;   // of the whole tape
};
// base == nullptr: null pointers and the size, as Carver does.  d->NL <= kMaxLayers (the entry points refuse more before they call)
TrainTape carve_tape(const diffab_dims* d, float* base);
inline size_t train_tape_floats(const diffab_dims* d) { return carve_tape(d, nullptr).floats; }
// Dynamic LDS of the attention backward's row pass (ipa_attn_bwd_rows_kernel: 3 H K + the row's vectors, in bytes) and its limit.  The
// one predicate of which dims the backward runs: run_backward refuses past it, and so do the taped forwards, before anything is launched.
constexpr size_t kAttnBwdLdsMax = 160 * 1024;
size_t attn_bwd_lds_bytes(const diffab_dims* d);
inline bool attn_bwd_lds_ok(const diffab_dims* d) { return attn_bwd_lds_bytes(d) <= kAttnBwdLdsMax; }
size_t train_bwd_workspace_floats(const diffab_dims* d);
// One backward driver, three roots:
//   BWD_LOSSES      the three masked losses of diffab_pytorch.py:856-880 with upstream gradients upstream3 (the training step)
//   BWD_COTANGENTS  arbitrary cotangents of the Denoiser outputs (cot_eps, cot_O0, cot_post; null = zero): Denoiser.forward under autograd
//   BWD_LAYER       one IPA layer from d y (layer_dy) to d x (layer_dx): InvariantPointAttentionLayer.forward under autograd; `w` / `g`
//                   then carry only layers[0] and `tp` is a one-layer tape
enum BwdRoot { BWD_LOSSES, BWD_COTANGENTS, BWD_LAYER };
struct BackwardArgs {  // fields a root does not name stay null
  BwdRoot root;
  const diffab_dims* d;
  const diffab_denoiser_weights *w, *g;  // weights; gradients (+=)
  TrainTape tp;
  float* ws;  // train_bwd_workspace_floats(d)
  hipStream_t st;
  // inputs of the forward.  The frames: x_t / O_t of the denoiser entries, t / R of the layer entry
  const int64_t* seq_t;
  const float *trans, *rot, *pair_ctx;
  // BWD_LOSSES: the forward's outputs, the targets, the masks and the three upstream gradients
  const float *eps_hat, *O0_hat, *true_post, *true_eps, *true_O0, *upstream3;
  const uint8_t *gm, *rm;
  const float* post_hat;                      // BWD_LOSSES, BWD_COTANGENTS
  const float *cot_eps, *cot_O0, *cot_post;  // BWD_COTANGENTS (each nullable = zero)
  const float* layer_dy;                      // BWD_LAYER
  // outputs.  d_trans (rows x 3) / d_rot (rows x 9), nullable: gradients with respect to the frames, which the reference's forward is
  // differentiable in (:315-336, :594-596) - d_x_t / d_O_t of the denoiser, d_t / d_R of the layer; the training step never asks
  float *layer_dx, *d_res_ctx, *d_pair_ctx, *d_trans, *d_rot;
};
int run_backward(const BackwardArgs& a);
// Y = act(X W^T + b) backward: dW += dY^T X (W is N x Kd, row-major), db += colsum dY (nullable), dX (+)= dY W (nullable).
// dY must already carry the activation mask (bwd_relu_mask: dY *= act > 0, in place).  bwd_gemm_nn: C (+)= A[M,K] B[K,N].
int bwd_linear(const float* dY, int ldy, const float* X, int ldx, const float* W, float* dW, float* db, float* dX, int lddx, int M, int N,
               int Kd, bool acc_dx, hipStream_t st);
int bwd_relu_mask(float* dY, const float* act, int64_t n, hipStream_t st);
// bwd_linear whose input gradient is masked by relu_act > 0 (rows lddx apart) in the product's epilogue; C = (A B) masked likewise
int bwd_linear_masked(const float* dY, int ldy, const float* X, int ldx, const float* W, float* dW, float* db, float* dX, int lddx, int M,
                      int N, int Kd, const float* relu_act, hipStream_t st);
// pair_chain_bwd.hip: the four 64-wide layers at the end of the PairEmbedding backward as one launch per chunk of pair rows
size_t pair_chain_bwd_prep_floats();
size_t pair_chain_bwd_part_floats();
int launch_pair_dist_bwd_fused(const int64_t* seq, const uint8_t* seq_m, const float* distmat, const float* xyz, const float* din, const float* dh1,
                               const float* W, int ld_w, int K, int A, int n_aa, int unk, int64_t row0, int64_t nrows, int ld, float* g_sp,
                               float* prep, hipStream_t st);
bool pair_dist_bwd_mfma_supported(int K, int A, int64_t row0, int64_t nrows, int ld, int n_aa);
int launch_pair_dist_bwd_mfma(const int64_t* seq, const uint8_t* seq_m, const float* distmat, const float* xyz, const float* din, const float* ddin,
                              int K, int A, int n_aa, int unk, int64_t row0, int64_t nrows, int ld, float* g_sp, hipStream_t st);
bool pair_table_mfma_supported(int C, int K, int64_t row0, int64_t nrows, int n_aa, int max_dist);
int launch_pair_table_mfma(const float* g, const int64_t* seq, const uint8_t* seq_m, const int64_t* resid, int resid_bstride, const int64_t* chain,
                           int K, int max_dist, int n_aa, int unk, int64_t row0, int64_t nrows, float* G1, float* part, hipStream_t st);
// per-work-group partial sums -> their destinations: out[q][(i / cols[q]) ld[q] + i % cols[q]] += sum_p parts[p stride + off[q] + i], i < n[q]
struct PartsSegs { int nseg; int off[8]; int n[8]; int cols[8]; int ld[8]; float* out[8]; };
int launch_parts_reduce(const float* parts, int nparts, int64_t stride, const PartsSegs& sg, hipStream_t st);
bool pair_chain_bwd_supported(int C, int K, int64_t row0, int64_t nrows);
bool pair_chain_bwd_enabled();  // false: diffab_debug_set_attn_variant bit 6 (64): the separate launches (A/B, tests)
int launch_pair_chain_bwd(const float* d_out, const float* amask, int K, int A, int ca, int64_t row0, int64_t nrows, const float* const* X,
                          const float* const* W, const int* ldw, float* dC, float* dh1, float* const* gW, const int* ldg, float* const* gb,
                          float* prep, float* part, hipStream_t st);
int bwd_gemm_nn_masked(const float* A, int lda, const float* B, int ldb, float* C, int ldc, int M, int N, int K, const float* relu_act,
                       hipStream_t st);
// n <= 4 products C_p[64 x 64] (rows ldc_p apart) += A_p^T B_p of dense [M x 64] operands in one launch; db_p (nullable) += colsum A_p
int bwd_tn64_set(int n, const float* const* A, const float* const* B, float* const* C, const int* ldc, float* const* db, int64_t M,
                 hipStream_t st);
// C[N1 x N2] (rows ldc apart) += A[M x N1]^T B[M x N2]; db (nullable) += column sums of A
int bwd_gemm_tn(const float* A, int lda, const float* B, int ldb, float* C, int ldc, int M, int N1, int N2, float* db, hipStream_t st);
int bwd_gemm_nn(const float* A, int lda, const float* B, int ldb, float* C, int ldc, int M, int N, int K, bool acc, hipStream_t st);
int launch_losses_fwd(const float* pp, const float* tp, const float* pe, const float* te, const float* pO, const float* tO, const uint8_t* gm,
                      const uint8_t* rm, int B, int K, int V, float* out3, hipStream_t st,
                      float* scratch = nullptr);  // scratch: 1024 floats -> the multi-work-group two-stage reduction

// diffusion_kernels.hip
// Trajectory recording (diffab_sample_options.record), a by-value launch argument of the update kernel: constant for a whole call, so the
// captured step of graph replay carries it unchanged.  slot == nullptr: nothing is recorded (one uniform branch).  Entry (b, j, k) of
// every field is (b n_slots + j) K + k; pred_x == nullptr: the state alone.
struct SampleRecordDev {
  const int32_t* slot = nullptr;  // device [T + 1]: step t -> slot, -1 = not recorded
  int32_t n_slots = 0;
  int64_t* seq = nullptr;
  float* x = nullptr;
  float* O = nullptr;
  float* pred_x = nullptr;
  float* pred_O = nullptr;
  float* seq_probs = nullptr;
  const float* alpha_bar_sqrt = nullptr;  // the schedule's, for x0_hat (read with predictions only)
};
// Fewer-step sampling (diffab_sample_options.steps), a by-value launch argument of the update kernel like the record: next == nullptr is the
// ordinary step t -> t - 1.  The three tables (T + 1 entries, device) are the call's plan; alpha_bar is the schedule's.
struct StepPlanDev {
  const int32_t* next = nullptr;  // step t -> the step s the update moves the state to
  const float* beta = nullptr;    // beta'_t
  const float* alpha = nullptr;   // alpha'_t
  const float* alpha_bar = nullptr;
};
// Structure guidance (diffab_sample_options.guidance), a by-value launch argument of the update kernel like the plan: shift == nullptr is
// off.  launch_reverse_update_philox runs the guidance kernel first (Delta into shift), and the update subtracts Delta from the mean of
// the translations at the steps t <= t_max.
struct GuidanceDev {
  float* shift = nullptr;                  // (B, K, 3) Delta of the step
  const int32_t* chain = nullptr;          // (B, K)
  const int32_t* residue_idx = nullptr;    // (B, K)
  const uint8_t* residue_mask = nullptr;   // (B, K), nullable = all
  float w_clash = 0.f, clash_distance = 0.f, w_bond = 0.f, bond_length = 0.f, max_shift = 0.f;
  int32_t t_max = -1;
};
// Noise scales and sequence temperature (diffab_sample_options.temperature), a by-value launch argument of the update kernel like the plan:
// one entry per state row of the launch (i / K), each pointer nullable (null = 1 for that quantity; all null is today's update).  rot_row
// is the row of the state row's sigma list in the stacked reverse table: step t reads table row rot_row + t.
struct TemperatureDev {
  const float* trans_scale = nullptr;  // lambda_x >= 0
  const float* rot_scale = nullptr;    // lambda_O >= 0 (needs rot_row)
  const float* seq_temp = nullptr;     // tau >= 0
  const int32_t* rot_row = nullptr;
};
// Particle steering (diffab_sample_options.steering), by value like the guidance: logw == nullptr is off and today's
// launch sequence.  Every steering kernel evaluates the steering-step predicate itself (steer_is_step), so a replayed graph needs no
// host decision.  step_anc is the step's ancestor map (rows, group-local indices) the gather reads; ancestors the nullable record.
struct SteeringDev {
  float* logw = nullptr;     // (rows) accumulated log-weight
  float* u_prev = nullptr;   // (rows) the energy the weight has seen last
  float* energy = nullptr;   // (rows) U of the last steering step
  int32_t* ancestors = nullptr;  // (T + 1, rows), nullable: row t is written at steering step t
  int32_t* step_anc = nullptr;   // (rows)
  void* scratch = nullptr;       // rows K 56 B: seq (int64) | x (3 fp32) | O (9 fp32) of the gathered residues
  const int32_t* chain = nullptr;
  const int32_t* residue_idx = nullptr;
  const uint8_t* residue_mask = nullptr;
  float w_clash = 0.f, clash_distance = 0.f, w_bond = 0.f, bond_length = 0.f, strength = 0.f, ess_threshold = 0.f;
  int32_t t_min = 0, t_max = -1, every = 1, group_size = 1, t_stop = 0;
  const int32_t* next_host = nullptr;  // HOST copy of a step plan's next[] (nullptr: t - 1): lets the eager loop skip the launches of a step that does not steer
};
// t is a steering step: t_min <= t <= t_max, (t_max - t) % every == 0 and the step's successor (t - 1, or next[t] of a step plan) above t_stop
__host__ __device__ inline bool steer_is_step(const SteeringDev& sd, int t, int succ) {
  return t >= sd.t_min && t <= sd.t_max && (sd.t_max - t) % sd.every == 0 && succ > sd.t_stop;
}
// steering_kernels.hip: U of every row at x0_hat into sd.energy (before the update); weights, resampling and the gather (after it)
int launch_steer_energy(const SteeringDev& sd, const diffab_sched* s, const StepPlanDev& plan, int t, const int* t_dev, const float* x,
                        const float* eps_hat, const uint8_t* gm, int B, int K, hipStream_t st);
int launch_steer_resample_gather(const SteeringDev& sd, const StepPlanDev& plan, int t, const int* t_dev, int64_t* seq, float* x, float* O,
                                 const uint8_t* gm, uint64_t seed, int64_t first_patch, int B, int K, bool copy_seq, hipStream_t st);
// The options of a reverse update, constant for a whole diffab_sample_loop_ex call (host side: the launcher unpacks it into the update
// kernel's launch arguments).  A default-constructed one is the plain update.
struct UpdateOptions {
  uint32_t keep = 0;                  // DIFFAB_FLAG_KEEP_STRUCTURE / _SEQUENCE: the modality left unwritten
  const uint32_t* allowed = nullptr;  // per-residue allowed-class words of the sequence draw (nullable)
  SampleRecordDev rec;                // trajectory recording (rec.slot nullable)
  StepPlanDev plan;                   // fewer-step sampling (plan.next nullable)
  GuidanceDev guide;                  // structure guidance (guide.shift nullable)
  TemperatureDev temp;                // noise scales / sequence temperature (all nullable)
  SteeringDev steer;                  // particle steering (steer.logw nullable)
};
// t_dev: read the timestep from device memory (graph replay); head_v / head_logits: the heads' epilogue done in the kernel
int launch_reverse_update_philox(const diffab_sched* s, const diffab_igso3* tab, int t, int64_t* seq, float* x, float* O,
                                 const float* eps_hat, float* O0_hat, float* post, const uint8_t* gm, uint64_t seed,
                                 int64_t first_patch, int B, int K, int V, hipStream_t st, const int* t_dev, const float* head_v,
                                 const float* head_logits, const UpdateOptions& o);
int check_guidance_terms(const diffab_sample_guidance* g, const char* who);  // weights, distances, chain / residue_idx (DIFFAB_ERR_ARG)
// the residues that are not generated: their (constant) state in every slot of the record, and their predictions - the given x / O and a
// one-hot of the token - once per call
int launch_record_fixed(const SampleRecordDev& rec, const int64_t* seq, const float* x, const float* O, const uint8_t* gm, int B, int K, int V,
                        hipStream_t st);
int launch_fill_beta(const diffab_sched* s, int t, int B, float* out, hipStream_t st, const int* t_dev = nullptr);
int launch_tiles_needed(const uint8_t* gm, int B, int K, unsigned char* out, hipStream_t st);  // [B][K / 16]: any generated residue in the tile
// The last layer's row plan of the module launch, per patch 2 + K / 16 ints: {n_items, slab bits, start row of item 0 .. n_items - 1 (-1
// behind them)}.  Items are 16-row windows chosen greedily - s = min(first generated row not yet covered, K - 16) covers [s, s + 16) - so
// there are never more than aligned tiles with a generated residue; bit j of the slab word: a generated residue in rows 32 j .. 32 j + 31
// ((K + 31) / 32 slabs, the last one short when K % 32 != 0: K = 16 is one slab).  K % 16 == 0, 16 <= K <= 1024.
constexpr int row_plan_ints(int K) { return 2 + K / 16; }
int launch_row_plan(const uint8_t* gm, int B, int K, int* out, hipStream_t st);
// The start class of patch b's work-group in the module launch, from the row plan: the launch staggers its work-groups' starts over
// `classes` classes (ipa_persistent.hip), and what a patch's LAST layer costs is known from its plan (items first, then live slabs) -
// the patches with the most start first, so that the extra items end inside the launch instead of at its end.  Patches ranked by
// descending (items, slabs), ties by the static class (b / 8) % classes and then by b; class = rank * classes / B: every class keeps
// B / classes patches (floor or ceiling), the spread of the starts is what it was.  Timing only: no result depends on it.
__host__ __device__ inline int start_class_of(const int* plan, int B, int K, int classes, int b) {
  const int n = row_plan_ints(K);
  auto key = [&](int i) {  // larger: more work in the last layer; then the earlier static class
    const int* p = plan + static_cast<int64_t>(i) * n;
    return ((p[0] * 64 + __builtin_popcount(static_cast<unsigned>(p[1]))) * classes) + (classes - 1 - (i >> 3) % classes);
  };
  const int kb = key(b);
  int64_t rank = 0;
  for (int i = 0; i < B; ++i) {
    const int ki = key(i);
    rank += ki > kb || (ki == kb && i < b);
  }
  return static_cast<int>(rank * classes / B);
}
// out[b] = start_class_of(plan, ..., b), one byte per patch (classes <= 256); out holds B bytes rounded up to a multiple of 4
int launch_start_classes(const int* plan, int B, int K, int classes, unsigned char* out, hipStream_t st);
// shared contexts: out[b] = src[ctx_of_row[b]] for the B rows of `row_floats` floats each (16-byte aligned rows)
int launch_gather_rows(const float* src, const int* ctx_of_row, int B, int64_t row_floats, float* out, hipStream_t st);
// design scoring (diffab_score_designs): a chunk of evaluated rows q = ((r n_t) + j) n_draws + m, q0 .. q0 + valid - 1, in buffers of
// `rows` (d->B) rows; the noising kernel fills rows past `valid` with copies of the last valid row, the loss kernel reads the valid ones
struct ScoreChunk {
  const int* t_list;  // device [n_t]
  int n_t, n_draws, K;
  int64_t q0;
  int rows, valid;
  uint32_t keep;  // DIFFAB_FLAG_KEEP_STRUCTURE / _SEQUENCE
};
constexpr int kScoreCtxMax = 256;  // designs per noising launch (their context indices are a by-value kernel argument)
struct ScoreCtxTable {
  int64_t r0;  // ctx[r - r0] = context of design r
  int ctx[kScoreCtxMax];
};
// s_t / x_t / O_t / eps (rows, K, ...), beta_row / ctx_row (rows); ctx_of_design: HOST map, nullptr = the identity
int launch_score_noise(const diffab_sched* s, const diffab_igso3* fwd, const ScoreChunk& c, const int64_t* seq0, const float* x0,
                       const float* O0, const uint8_t* gm, const int32_t* ctx_of_design, uint64_t seed, int64_t first_design, int64_t* s_t,
                       float* x_t, float* O_t, float* eps, float* beta_row, int* ctx_row, const diffab_score_noised& out, hipStream_t st);
// out_terms (n_designs n_t n_draws, 3) and out_residue (nullable, (..., K, 3)) at rows q0 .. q0 + valid - 1; rm nullable (all true)
int launch_score_losses(const diffab_sched* s, const ScoreChunk& c, const int64_t* seq0, const float* O0, const uint8_t* gm, const uint8_t* rm,
                        const int64_t* s_t, const float* O_t, const float* eps, const float* eps_hat, const float* v_hat, const float* logits,
                        float* out_terms, float* out_residue, hipStream_t st);
int launch_set_int(int* p, int v, hipStream_t st);
int launch_dec_int(int* p, hipStream_t st);
int launch_advance_step(int* p, const int* next, hipStream_t st);  // *p = next[*p] (graph replay of a step plan)

}  // namespace diffab
