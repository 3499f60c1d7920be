// api.hip - C-ABI entry points for the denoise step, the IPA layer and the reverse sampling loop,
// plus library plumbing (version, last error, device probe).
#include <atomic>
#include <cstring>
#include <mutex>
#include <vector>

#include "common.h"
#include "denoiser_internal.h"
#include "mlp_chain_tile.h"
#include "../../include/diffab_hip_debug.h"

namespace diffab {

static thread_local char g_err[512] = "";

void set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}

// ---- cross-stream ordering guard (common.h StreamOrder), OFF by default since round 6 ---------------------------------------------
// History (profiles/r04_two_queue.md, r05_two_queue.md): with two library pipelines on two streams of one process, heads_finish_kernel and
// reverse_update_philox_kernel - small VALU-only kernels - computed wrong values in lanes 48-63 while bf16 x 6 GEMM work-groups of the OTHER
// stream were resident.  Round 6 found the cause (profiles/r06_lanes_48_63.md, tools/hwtests/pkmul_two_streams.hip): hipcc's SLP vectoriser
// had packed their scalar code into v_pk_{mul,fma}_f32 ... op_sel:[0,1], a form gfx950 miscomputes in lanes 48-63 while f16 / bf16 MFMAs of
// ANY wave - another kernel's included - are in flight on the SIMD.  The form is gone from every kernel of the library (Makefile NOSLP,
// tools/isa_hazard_lint.py), two pipelines on two streams measure bitwise the sequential runs with the guard off, so the guard is now an
// opt-in (diffab_set_stream_guard(1)): one state per device = {last stream, event}.
namespace {
struct OrderState {
  std::recursive_mutex mu;
  hipStream_t last = nullptr;
  bool have = false;
  hipEvent_t ev = nullptr;
  int depth = 0;
};
OrderState g_order[32];
std::atomic<bool> g_order_on{false};
}  // namespace

StreamOrder::StreamOrder(void* stream) : dev_(-1) {
  if (!g_order_on.load(std::memory_order_relaxed)) return;  // guard off (default): nothing is held, calls of host threads do not serialise
  if (hipGetDevice(&dev_) != hipSuccess) dev_ = 0;
  OrderState& o = g_order[dev_ & 31];
  o.mu.lock();
  if (o.depth++ > 0) return;  // an entry point called from another entry point: already ordered
  hipStream_t st = as_stream(stream);
  if (o.have && o.last != st) {
    // everything enqueued on the previous stream so far (the library's last call, and whatever the caller put behind it) comes first
    if (o.ev == nullptr && hipEventCreateWithFlags(&o.ev, hipEventDisableTiming) != hipSuccess) o.ev = nullptr;
    if (o.ev != nullptr && hipEventRecord(o.ev, o.last) == hipSuccess) (void)hipStreamWaitEvent(st, o.ev, 0);
    (void)hipGetLastError();  // a stream the caller destroyed meanwhile: nothing left to order against
  }
  o.last = st;
  o.have = true;
}
StreamOrder::~StreamOrder() {
  if (dev_ < 0) return;
  OrderState& o = g_order[dev_ & 31];
  --o.depth;
  o.mu.unlock();
}
void set_stream_order(bool on) { g_order_on.store(on); }

// ---- opt-in launch timer for the dominant kernel (bench.py's roofline leg) ---------------------------------
// When enabled, the attention-kernel launchers bracket each launch with a hipEvent pair recorded on the launch
// stream; diffab_kernel_timer_read() synchronises the events and returns the launch count and the summed time.
struct KernelTimer {
  bool on = false;
  std::vector<hipEvent_t> ev;  // start/stop pairs
  size_t used = 0;
};
static KernelTimer g_timer;

void timer_begin(hipStream_t st) {
  if (!g_timer.on) return;
  if (g_timer.used + 2 > g_timer.ev.size()) {
    for (int i = 0; i < 2; ++i) {
      hipEvent_t e;
      if (hipEventCreate(&e) != hipSuccess) return;
      g_timer.ev.push_back(e);
    }
  }
  (void)hipEventRecord(g_timer.ev[g_timer.used], st);
}
bool kernel_timer_enabled() { return g_timer.on; }
void timer_end(hipStream_t st) {
  if (!g_timer.on || g_timer.used + 2 > g_timer.ev.size()) return;
  (void)hipEventRecord(g_timer.ev[g_timer.used + 1], st);
  g_timer.used += 2;
}

static int check_dims(const diffab_dims* d, const char* who) {
  DIFFAB_REQUIRE(d != nullptr, DIFFAB_ERR_ARG, "%s: dims is null", who);
  // C == 0: an IPA layer built with use_pair_bias = False (reference :348-385) - no pair bias, two independent logits, no o_pair block
  // in the feature row; the layer entries take it on the any-dims path (e and w_bias may be NULL), the Denoiser always has C > 0
  DIFFAB_REQUIRE(d->B > 0 && d->K > 0 && d->D > 0 && d->C >= 0 && d->H > 0 && d->DS > 0 && d->PQ > 0 && d->PV > 0 && d->NL >= 0 && d->V > 0,
                 DIFFAB_ERR_ARG, "%s: non-positive dimension (B=%d K=%d D=%d C=%d H=%d DS=%d PQ=%d PV=%d NL=%d V=%d)", who, d->B, d->K, d->D,
                 d->C, d->H, d->DS, d->PQ, d->PV, d->NL, d->V);
  DIFFAB_REQUIRE(static_cast<int64_t>(d->B) * d->K < (1ll << 31), DIFFAB_ERR_UNSUPPORTED, "%s: B*K must be < 2^31", who);
  return DIFFAB_OK;
}

struct StepBuffers {
  float *cat2, *h1, *hA, *hB, *cat3, *t1, *t2, *vbuf, *logits, *ipa, *emb_tab, *beta_tab;
  char* planes;  // split bf16 planes of the dense weights (MFMA path): NL x ipa_layer_planes_bytes(), then 11 MLP matrices
  float* pair;   // fp16 planes of the pair embedding (launch_pair_split), null when the fused kernel cannot take them
  size_t bytes;
};
static size_t mlp_planes_bytes() { return (rowgemm128_b6_scratch_bytes(128) + 255) & ~static_cast<size_t>(255); }

// n_pair: patches of the pair embedding whose fp16 planes the buffers hold (0: d->B; shared contexts: n_ctx)
static StepBuffers carve_step(const diffab_dims* d, void* ws, int n_pair = 0) {
  Carver c(ws);
  const size_t rows = static_cast<size_t>(d->B) * d->K;
  StepBuffers b;
  b.cat2 = c.take<float>(rows * 2 * d->D);
  b.h1 = c.take<float>(rows * d->D);
  b.hA = c.take<float>(rows * d->D);
  b.hB = c.take<float>(rows * d->D);
  b.cat3 = c.take<float>(rows * (d->D + 3));
  b.t1 = c.take<float>(rows * d->D);
  b.t2 = c.take<float>(rows * d->D);
  b.vbuf = c.take<float>(rows * 3);
  b.logits = c.take<float>(rows * d->V);
  b.emb_tab = c.take<float>(static_cast<size_t>(25) * d->D);
  b.beta_tab = c.take<float>(static_cast<size_t>(3) * d->B * d->D);
  size_t ipa_floats = ipa_generic_workspace_floats(d);
  if (fast_path_supported(d)) ipa_floats = ipa_floats > ipa_fast_workspace_floats(d) ? ipa_floats : ipa_fast_workspace_floats(d);
  b.ipa = c.take<float>(ipa_floats);
  b.planes = fast_path_supported(d) ? c.take<char>(d->NL * ipa_layer_planes_bytes() + 11 * mlp_planes_bytes()) : nullptr;
  b.pair = pair_planes_supported(d) ? c.take<float>(pair_planes_floats(d, n_pair)) : nullptr;  // (last: n_pair moves no other buffer)
  b.bytes = c.bytes();
  return b;
}

static bool ipa_layer_weights_ok(const diffab_dims* d, const diffab_ipa_layer_weights* w) {
  return w && w->gamma && w->wq_s && w->wk_s && w->wv_s && (w->w_bias || d->C == 0) && w->wq_p && w->wk_p && w->wv_p && w->w_out && w->b_out;
}

static int ipa_layer_dispatch(const diffab_dims* d, const diffab_ipa_layer_weights* w, const float* x, const float* e, const float* R,
                              const float* t, float* y, float* ws, uint32_t flags, hipStream_t st, float* sp_keep = nullptr,
                              float* d2_keep = nullptr, const void* planes = nullptr, const float* pair_planes = nullptr,
                              bool taped = false,  // taped: ws is a slot of the training tape (the backward reads proj and feat)
                              const unsigned char* tile_needed = nullptr, const int* ctx_of_row = nullptr, int n_ctx = 0) {
  DIFFAB_REQUIRE(ipa_layer_weights_ok(d, w), DIFFAB_ERR_ARG, "ipa layer: null weight pointer");
  if (!(flags & DIFFAB_FLAG_FORCE_GENERIC) && fast_path_supported(d))
    return ipa_layer_fast(d, w, x, e, R, t, y, ws, st, sp_keep, d2_keep, planes, pair_planes, (flags & DIFFAB_FLAG_FP32_GEMM) != 0,
                          taped, tile_needed, ctx_of_row, n_ctx);
  return ipa_layer_generic(d, w, x, e, R, t, y, ws, st, ctx_of_row);
}

// Every weight pointer the denoiser forward reads, checked on the host before anything is enqueued.
static int check_denoiser_weights(const diffab_dims* d, const diffab_denoiser_weights* w) {
  DIFFAB_REQUIRE(w && w->seq_emb && w->res_w0 && w->res_b0 && w->res_w2 && w->res_b2 && (d->NL == 0 || w->layers), DIFFAB_ERR_ARG,
                 "denoiser: null weight pointer");
  DIFFAB_REQUIRE(d->C > 0, DIFFAB_ERR_ARG, "denoiser: C must be positive (the Denoiser's IPA layers use the pair bias, :478-492)");
  for (const diffab_mlp3_weights* h : {&w->coord, &w->orient, &w->seq})
    DIFFAB_REQUIRE(h->w0 && h->b0 && h->w2 && h->b2 && h->w4 && h->b4, DIFFAB_ERR_ARG, "denoiser head: null weight pointer");
  for (int l = 0; l < d->NL; ++l)
    DIFFAB_REQUIRE(ipa_layer_weights_ok(d, &w->layers[l]), DIFFAB_ERR_ARG, "denoiser: null weight pointer in IPA layer %d", l);
  return DIFFAB_OK;
}

// Operand alignment of a weight (or gradient) table: every float buffer of it, named `group.field` in the message.  The denoiser, layer,
// training, sampler and scoring entries refuse a float operand that is not 16-byte aligned (their tiles load and store float4), on the
// host and before anything is enqueued; int64 indices and masks are read element by element and need their natural alignment only.
static int check_layer_aligned(const char* who, const char* group, int l, const diffab_ipa_layer_weights* w) {
  const Operand fs[] = {{"gamma", w->gamma}, {"wq_s", w->wq_s}, {"wk_s", w->wk_s}, {"wv_s", w->wv_s}, {"w_bias", w->w_bias},
                        {"wq_p", w->wq_p},   {"wk_p", w->wk_p}, {"wv_p", w->wv_p}, {"w_out", w->w_out}, {"b_out", w->b_out}};
  for (const Operand& f : fs)
    DIFFAB_REQUIRE(aligned16(f.p), DIFFAB_ERR_ARG, "%s: operand %s.layers[%d].%s must be 16-byte aligned (see \"Operand alignment\" in diffab_hip.h)",
                   who, group, l, f.name);
  return DIFFAB_OK;
}
static int check_denoiser_aligned(const char* who, const char* group, const diffab_dims* d, const diffab_denoiser_weights* w) {
  const Operand fs[] = {{"seq_emb", w->seq_emb}, {"res_w0", w->res_w0}, {"res_b0", w->res_b0}, {"res_w2", w->res_w2}, {"res_b2", w->res_b2}};
  for (const Operand& f : fs)
    DIFFAB_REQUIRE(aligned16(f.p), DIFFAB_ERR_ARG, "%s: operand %s.%s must be 16-byte aligned (see \"Operand alignment\" in diffab_hip.h)", who,
                   group, f.name);
  const diffab_mlp3_weights* hw[3] = {&w->coord, &w->orient, &w->seq};
  const char* hn[3] = {"coord", "orient", "seq"};
  for (int hd = 0; hd < 3; ++hd) {
    const Operand hs[] = {{"w0", hw[hd]->w0}, {"b0", hw[hd]->b0}, {"w2", hw[hd]->w2}, {"b2", hw[hd]->b2}, {"w4", hw[hd]->w4}, {"b4", hw[hd]->b4}};
    for (const Operand& f : hs)
      DIFFAB_REQUIRE(aligned16(f.p), DIFFAB_ERR_ARG, "%s: operand %s.%s.%s must be 16-byte aligned (see \"Operand alignment\" in diffab_hip.h)",
                     who, group, hn[hd], f.name);
  }
  for (int l = 0; l < d->NL; ++l)
    if (int rc = check_layer_aligned(who, group, l, &w->layers[l])) return rc;
  return DIFFAB_OK;
}

static bool use_pair_planes(const diffab_dims* d, uint32_t flags, const float* pair_ctx, const StepBuffers& b) {
  const uint32_t other = DIFFAB_FLAG_FORCE_GENERIC | DIFFAB_FLAG_PAIR_F32;
  return (flags & DIFFAB_FLAG_PAIR_PLANES) && !(flags & other) && b.pair != nullptr && pair_planes_supported(d) &&
         (reinterpret_cast<uintptr_t>(pair_ctx) & 15) == 0;
}

// The rule by which the reverse loop and design scoring choose the patch-resident module launch (given its other preconditions): K = 128
// and a batch that fills the chip with one work-group per patch, without a mostly idle last round.
static bool module_launch_fills_chip(const diffab_dims* d) {
  if (!ipa_module_persistent_supported(d)) return false;
  int dev = 0, ncu = 256;
  if (hipGetDevice(&dev) == hipSuccess) (void)hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, dev);
  const int rounds = (d->B + ncu - 1) / ncu;
  // (K = 256 - two dense tiles and sixteen two-chunk attention items per patch in the same launch, round 6 - measures SLOWER than its
  // per-layer launches at B = 512: 19.5 against 18.6 ms per step; it is bitwise the same and stays behind the explicit flag)
  return d->K == 128 && d->B >= ncu && static_cast<double>(d->B) >= 0.85 * rounds * ncu;
}

// The launch path of every denoiser forward of one call, decided once by plan_forward: prepare_forward does the call's weights-only
// work for it, denoise_step runs it once per step.
struct ForwardPlan {
  uint32_t flags;  // as the IPA layers read them (DIFFAB_FLAG_FORCE_GENERIC, DIFFAB_FLAG_FP32_GEMM)
  // Folded concatenations (MFMA path): the sequence-embedding half of to_res_emb[0] and the beta-embedding columns of the three head
  // MLPs become bias tables, so neither cat[res_ctx, E[s]] nor cat[h, tau] is written or re-read.
  bool fold;
  bool b6;     // dense products of the folded path from split weight planes prepared once per call (bf16x6; the layers' f16x3)
  bool chain;  // each MLP as one row-resident kernel (mlp_chain_b6_kernel) instead of one launch per dense layer
  // the NL layers as one patch-resident launch (ipa_persistent.hip) - the same tile bodies, bitwise the same result; fused_mlps: the
  // embedding MLP and the three heads run as phases of that launch, one launch per step in front of the state update
  bool persistent, fused_mlps;
  const float* pair_planes;               // fp16 planes of the pair embedding (launch_pair_split), or null: attention reads fp32
  const int* ctx_of_row;                  // shared contexts: device [B] map, state row b reads context ctx_of_row[b] (null: the identity)
  int n_ctx;                              // patches of pair_ctx and of its planes (0: d->B)
  const unsigned char* last_layer_tiles;  // [B][K / 16] row tiles of the LAST layer whose outputs are read (null: all)
  const int* last_layer_rows;             // the module launch's form of the same: launch_row_plan (null with last_layer_tiles)
  float* res_emb;                         // the residue embedding after the IPA module is copied here (null: not wanted)
  // reverse sampler, module launch with a row plan: [B] the start class of every patch by its last-layer work (launch_start_classes;
  // null: the static classes)
  const unsigned char* start_class;
};

// loop: the call runs many forwards (reverse sampler, design scoring).  There the pair embedding is the same tensor in every attention
// launch, so its fp16 planes are on unless DIFFAB_FLAG_PAIR_F32, and the module launch is chosen by module_launch_fills_chip unless
// DIFFAB_FLAG_MULTI_LAUNCH; a single forward takes both from its flags.  tiles, row_plan: the reverse sampler's buffers of the row-tile
// map and of the row plan; start_class: its buffer of the work-groups' start classes.
static ForwardPlan plan_forward(const diffab_dims* d, uint32_t flags, const StepBuffers& b, const float* res_ctx, const float* pair_ctx,
                                float* res_emb, bool loop, const int* ctx_of_row = nullptr, int n_ctx = 0, unsigned char* tiles = nullptr,
                                int* row_plan = nullptr, unsigned char* start_class = nullptr) {
  const int rows = d->B * d->K, D = d->D;
  if (loop && !(flags & DIFFAB_FLAG_PAIR_F32)) flags |= DIFFAB_FLAG_PAIR_PLANES;
  ForwardPlan p{};
  p.flags = flags;
  // The split-precision MLPs take any row count; only the fp32 kernel of the folded path needs a whole 128-row group (rowgemm128_ok).
  // That M >= 128 must not gate the split-precision path: one patch of 64 residues would run its embedding MLP and heads on other kernels
  // than the same patch in a larger batch, and its bits would depend on the batch (tests/test_gpu_launch_forms.py, K = 64, B = 1).
  const bool mfma = !(flags & DIFFAB_FLAG_FORCE_GENERIC) && fast_path_supported(d);
  p.b6 = mfma && use_b6_gemm(flags) && rowgemm128_b6_ok(res_ctx, D, b.h1, D, rows, D);
  p.fold = mfma && (p.b6 || rowgemm128_ok(res_ctx, D, b.h1, D, rows, D));
  p.chain = p.b6 && d->V <= 128;
  p.pair_planes = use_pair_planes(d, flags, pair_ctx, b) ? b.pair : nullptr;
  p.ctx_of_row = ctx_of_row;
  p.n_ctx = n_ctx;
  // Reverse sampler (tiles != nullptr): the step's outputs (eps, O0, posterior) are read for GENERATED residues only (reverse_update,
  // its heads epilogue, guidance and the record leave the others alone), so the last layer's attention is needed only for row tiles
  // that contain one; every other layer feeds keys and values of all rows to the next.  Same trajectory, bit for bit, on both launch
  // forms; DIFFAB_FLAG_ALL_ROWS keeps every tile.  (NL >= 2: a skipped tile's feature rows then hold the previous layer's values of
  // this very forward - never an unwritten workspace.)
  p.last_layer_tiles = tiles != nullptr && !(flags & DIFFAB_FLAG_ALL_ROWS) && p.fold && d->K % 16 == 0 && d->NL >= 2 ? tiles : nullptr;
  p.res_emb = res_emb;
  // The module launch of a loop: bitwise the 3 NL launches it replaces, so the choice never shows in the results.  When the batch fills
  // the chip with one work-group per patch it wins (B = 256: 2.60 ms per step against 2.70); fewer patches than CUs leave CUs idle for
  // the whole module (B = 8: 2.07 ms against 0.47), a ragged last round of patches costs a module time for a few of them.
  p.persistent = p.b6 && p.pair_planes != nullptr && ipa_module_persistent_supported(d) &&
                 ((flags & DIFFAB_FLAG_PERSISTENT_MODULE) || (loop && !(flags & DIFFAB_FLAG_MULTI_LAUNCH) && module_launch_fills_chip(d)));
  p.fused_mlps = p.persistent && p.chain && D == 128 && res_emb == nullptr;
  // The module launch walks the last layer's rows by the row plan (16-row windows from the generated rows: fewer items than aligned
  // tiles); the per-layer launches keep the tile map.
  p.last_layer_rows = p.persistent && p.last_layer_tiles != nullptr ? row_plan : nullptr;
  // The plan says what a patch's last layer costs: the launch starts the heaviest patches first (timing only).  K = 128 only, where
  // it was measured; K = 256 keeps the static classes.
  p.start_class = p.last_layer_rows != nullptr && d->K == 128 && module_stagger_classes() > 1 && module_stagger_classes() <= 256
                      ? start_class
                      : nullptr;
  return p;
}

// The per-step head bias: beta of every patch, or (reverse sampler: every patch is at step t, or *t_dev under graph replay) the
// schedule's sched_beta[t], which the folded head tables read themselves; `beta` is then read by the unfolded path only.
struct StepBias {
  const float* beta;
  const float* sched_beta;
  int t;
  const int* t_dev;
  // chain path of the eager reverse loop: [3 heads][traj_rows steps][D] the heads' folded beta columns of EVERY step (row t this
  // step's), built once per call by prepare_forward instead of a table per step
  float* beta_traj;
  int traj_rows;
};

// Everything of a call's forwards that depends on the weights and contexts only, once per call: on the folded path the
// sequence-embedding bias table and the split planes of every dense weight matrix, the fp16 planes of the n_ctx pair embeddings, and
// the table of every step's head columns when `bias` names one.
static int prepare_forward(const diffab_dims* d, const diffab_denoiser_weights* w, const ForwardPlan& p, const StepBuffers& b,
                           const float* pair_ctx, const StepBias& bias, hipStream_t st) {
  if (p.fold)
    if (int rc = launch_fold_embed_table(d, w, b.emb_tab, st)) return rc;
  if (p.b6) {
    const int D = d->D;
    for (int l = 0; l < d->NL; ++l)
      if (int rc = ipa_layer_split_weights(&w->layers[l], b.planes + l * ipa_layer_planes_bytes(), st)) return rc;
    char* mlp = b.planes + d->NL * ipa_layer_planes_bytes();
    const diffab_mlp3_weights* hw[3] = {&w->coord, &w->orient, &w->seq};
    if (int rc = launch_wsplit128(w->res_w0, 2 * D, D, mlp, st)) return rc;                        // slot 0: res_ctx half of to_res_emb[0]
    if (int rc = launch_wsplit128(w->res_w2, D, D, mlp + mlp_planes_bytes(), st)) return rc;      // slot 1
    for (int hd = 0; hd < 3; ++hd) {                                                              // slots 2 + 2 hd, 3 + 2 hd
      if (int rc = launch_wsplit128(hw[hd]->w0, D + 3, D, mlp + (2 + 2 * hd) * mlp_planes_bytes(), st)) return rc;
      if (int rc = launch_wsplit128(hw[hd]->w2, D, D, mlp + (3 + 2 * hd) * mlp_planes_bytes(), st)) return rc;
      const int nout = hd == 2 ? d->V : 3;                                                          // slot 8 + hd: the narrow last layer
      if (int rc = launch_wsplit128(hw[hd]->w4, D, D, mlp + (8 + hd) * mlp_planes_bytes(), st, nout)) return rc;
    }
  }
  if (p.pair_planes)
    if (int rc = launch_pair_split(d, pair_ctx, b.pair, st, p.n_ctx)) return rc;
  if (bias.beta_traj) {  // the same kernel and formula as the per-step table, "patch" = step
    diffab_dims dt = *d;
    dt.B = bias.traj_rows;
    if (int rc = launch_fold_beta_table(&dt, w, bias.sched_beta, bias.beta_traj, st)) return rc;
  }
  return DIFFAB_OK;
}

// One denoiser forward along a prepared plan.  out_O0 == nullptr: the caller finishes the heads itself from b.vbuf / b.logits.
static int denoise_step(const diffab_dims* d, const diffab_denoiser_weights* w, const ForwardPlan& p, const StepBias& bias,
                        const int64_t* seq_t, const float* x_t, const float* O_t, const float* res_ctx, const float* pair_ctx, float* out_eps,
                        float* out_O0, float* out_post, float* out_logits, const StepBuffers& b, hipStream_t st) {
  const int rows = d->B * d->K, D = d->D;
  if (p.fold && bias.beta_traj == nullptr)
    if (int rc = launch_fold_beta_table(d, w, bias.beta, b.beta_tab, st, bias.sched_beta, bias.t, bias.t_dev)) return rc;
  const char* mlp = p.b6 ? b.planes + d->NL * ipa_layer_planes_bytes() : nullptr;
  auto dense128 = [&](int slot, const float* X, const float* W, int ldw, const float* bvec, const int64_t* bias_idx, int bias_div, float* Y,
                      bool relu) -> int {
    if (p.b6) return launch_rowgemm128_b6p(X, D, mlp + slot * mlp_planes_bytes(), bvec, bias_idx, bias_div, Y, D, rows, D, relu, st);
    return launch_rowgemm128(X, D, W, ldw, bvec, bias_idx, bias_div, Y, D, rows, D, relu, st);
  };
  float* logits = out_logits ? out_logits : b.logits;
  MlpChainSet emb_set{}, head_set{};
  if (p.chain) {
    const void* pl[3] = {mlp, mlp + mlp_planes_bytes(), nullptr};
    const float* bs[3] = {b.emb_tab, w->res_b2, nullptr};
    float* ys[1] = {b.hA};
    const int nout1[1] = {D};
    if (int rc = make_mlp_chain_set(&emb_set, 1, pl, bs, seq_t, 0, 2, nout1, ys, nout1)) return rc;
    if (!p.fused_mlps)
      if (int rc = launch_mlp_chain_b6(res_ctx, D, pl, bs, seq_t, 0, 2, D, b.hA, D, rows, st)) return rc;
  } else if (p.fold) {
    if (int rc = dense128(0, res_ctx, w->res_w0, 2 * D, b.emb_tab, seq_t, 0, b.h1, true)) return rc;
    if (int rc = dense128(1, b.h1, w->res_w2, D, w->res_b2, nullptr, 0, b.hA, false)) return rc;
  } else {
    if (int rc = launch_embed_concat(res_ctx, w->seq_emb, seq_t, D, rows, b.cat2, st)) return rc;
    if (int rc = launch_linear(b.cat2, 2 * D, w->res_w0, w->res_b0, b.h1, D, rows, D, 2 * D, true, st)) return rc;
    if (int rc = launch_linear(b.h1, D, w->res_w2, w->res_b2, b.hA, D, rows, D, D, false, st)) return rc;
  }
  float *cur = b.hA, *nxt = b.hB;
  const diffab_mlp3_weights* hw[3] = {&w->coord, &w->orient, &w->seq};
  float* outs[3] = {out_eps, b.vbuf, logits};
  const int nout[3] = {3, 3, d->V};
  const void* hpl[9];
  const float* hbs[9];
  // (beta_traj: one table row for every patch - "row / rows" is 0 for all of them)
  const int head_div = bias.beta_traj ? rows : d->K;
  if (p.chain) {  // the three heads read the same rows: one launch (blockIdx.y = head), or three phases of the module launch
    for (int hd = 0; hd < 3; ++hd) {
      hpl[3 * hd] = mlp + (2 + 2 * hd) * mlp_planes_bytes();
      hpl[3 * hd + 1] = mlp + (3 + 2 * hd) * mlp_planes_bytes();
      hpl[3 * hd + 2] = mlp + (8 + hd) * mlp_planes_bytes();
      hbs[3 * hd] = bias.beta_traj ? bias.beta_traj + (static_cast<size_t>(hd) * bias.traj_rows + bias.t) * D
                                   : b.beta_tab + static_cast<size_t>(hd) * d->B * D;
      hbs[3 * hd + 1] = hw[hd]->b2;
      hbs[3 * hd + 2] = hw[hd]->b4;
    }
    if (int rc = make_mlp_chain_set(&head_set, 3, hpl, hbs, nullptr, head_div, 3, nout, outs, nout)) return rc;
  }
  if (p.persistent) {
    if (int rc = launch_ipa_module_persistent(d, b.hA, b.hB, O_t, x_t, b.ipa, b.planes, p.pair_planes, st, p.fused_mlps ? res_ctx : nullptr,
                                              &emb_set, &head_set, p.ctx_of_row, p.n_ctx, p.last_layer_rows, p.start_class))
      return rc;
    cur = (d->NL & 1) ? b.hB : b.hA;
  }
  for (int l = 0; l < d->NL && !p.persistent; ++l) {
    const void* planes = p.b6 ? b.planes + l * ipa_layer_planes_bytes() : nullptr;
    if (int rc = ipa_layer_dispatch(d, &w->layers[l], cur, pair_ctx, O_t, x_t, nxt, b.ipa, p.flags, st, nullptr, nullptr, planes, p.pair_planes,
                                    false, l == d->NL - 1 ? p.last_layer_tiles : nullptr, p.ctx_of_row, p.n_ctx))
      return rc;
    float* tmp = cur; cur = nxt; nxt = tmp;
  }
  if (p.res_emb) DIFFAB_HIP_CHECK(hipMemcpyAsync(p.res_emb, cur, sizeof(float) * rows * D, hipMemcpyDeviceToDevice, st));
  if (p.chain) {
    if (!p.fused_mlps)
      if (int rc = launch_mlp_chains_b6(cur, D, 3, hpl, hbs, nullptr, head_div, 3, nout, outs, nout, rows, st)) return rc;
  } else if (p.fold) {
    for (int hd = 0; hd < 3; ++hd) {
      if (int rc = dense128(2 + 2 * hd, cur, hw[hd]->w0, D + 3, b.beta_tab + static_cast<size_t>(hd) * d->B * D, nullptr, d->K, b.t1, true))
        return rc;
      if (int rc = dense128(3 + 2 * hd, b.t1, hw[hd]->w2, D, hw[hd]->b2, nullptr, 0, b.t2, true)) return rc;
      if (int rc = launch_linear(b.t2, D, hw[hd]->w4, hw[hd]->b4, outs[hd], nout[hd], rows, nout[hd], D, false, st)) return rc;
    }
  } else {
    if (int rc = launch_beta_concat(cur, bias.beta, D, d->K, rows, b.cat3, st)) return rc;
    for (int hd = 0; hd < 3; ++hd) {
      if (int rc = launch_linear(b.cat3, D + 3, hw[hd]->w0, hw[hd]->b0, b.t1, D, rows, D, D + 3, true, st)) return rc;
      if (int rc = launch_linear(b.t1, D, hw[hd]->w2, hw[hd]->b2, b.t2, D, rows, D, D, true, st)) return rc;
      if (int rc = launch_linear(b.t2, D, hw[hd]->w4, hw[hd]->b4, outs[hd], nout[hd], rows, nout[hd], D, false, st)) return rc;
    }
  }
  if (out_O0 == nullptr) return DIFFAB_OK;
  return launch_heads_finish(b.vbuf, O_t, logits, d->V, rows, out_O0, out_post, st);
}

// The taped forwards and their backwards are one unit: where the MFMA path applies the backward reads the probabilities and squared
// distances the three-launch attention left on the tape, so a taped forward must not be diverted to the generic kernels (which do not
// write them) - DIFFAB_FLAG_FORCE_GENERIC is ignored by diffab_train_step_fwd / diffab_denoise_step_fwd_taped /
// diffab_ipa_layer_fwd_taped (unit dims take the generic kernels on both sides anyway); the arithmetic selectors (FP32_GEMM) pass.
static uint32_t taped_flags(uint32_t flags) { return flags & ~(DIFFAB_FLAG_FORCE_GENERIC | DIFFAB_FLAG_PAIR_PLANES); }

// Training forward: the same launches as denoise_step, but every intermediate lands in its own slot of the tape.
static int denoise_step_taped(const diffab_dims* d, const diffab_denoiser_weights* w, const int64_t* seq_t, const float* x_t,
                              const float* O_t, const float* res_ctx, const float* pair_ctx, const float* beta, float* out_eps,
                              float* out_O0, float* out_post, const TrainTape& tp, uint32_t flags, hipStream_t st) {
  const int rows = d->B * d->K, D = d->D;
  if (int rc = launch_embed_concat(res_ctx, w->seq_emb, seq_t, D, rows, tp.cat2, st)) return rc;
  if (int rc = launch_linear(tp.cat2, 2 * D, w->res_w0, w->res_b0, tp.h1, D, rows, D, 2 * D, true, st)) return rc;
  if (int rc = launch_linear(tp.h1, D, w->res_w2, w->res_b2, tp.x[0], D, rows, D, D, false, st)) return rc;
  const bool b6 = plan_backward(d).fast && use_b6_gemm(flags);  // the layers' dense products from the tape's weight planes
  for (int l = 0; l < d->NL; ++l) {
    if (b6)
      if (int rc = ipa_layer_split_weights(&w->layers[l], tp.planes, st)) return rc;
    if (int rc = ipa_layer_dispatch(d, &w->layers[l], tp.x[l], pair_ctx, O_t, x_t, tp.x[l + 1], tp.ipa_ws[l], flags, st, tp.sp[l], tp.d2[l],
                                    b6 ? tp.planes : nullptr, nullptr, true))
      return rc;
  }
  if (int rc = launch_beta_concat(tp.x[d->NL], beta, D, d->K, rows, tp.cat3, st)) return rc;
  const diffab_mlp3_weights* hw[3] = {&w->coord, &w->orient, &w->seq};
  float* outs[3] = {out_eps, tp.vbuf, tp.logits};
  const int nout[3] = {3, 3, d->V};
  for (int hd = 0; hd < 3; ++hd) {
    if (int rc = launch_linear(tp.cat3, D + 3, hw[hd]->w0, hw[hd]->b0, tp.t1[hd], D, rows, D, D + 3, true, st)) return rc;
    if (int rc = launch_linear(tp.t1[hd], D, hw[hd]->w2, hw[hd]->b2, tp.t2[hd], D, rows, D, D, true, st)) return rc;
    if (int rc = launch_linear(tp.t2[hd], D, hw[hd]->w4, hw[hd]->b4, outs[hd], nout[hd], rows, nout[hd], D, false, st)) return rc;
  }
  return launch_heads_finish(tp.vbuf, O_t, tp.logits, d->V, rows, out_O0, out_post, st);
}

constexpr int kTrajRows = 1025;  // schedules up to T = 1024 get their per-step head tables built once per call
struct SampleBuffers {
  float *beta, *eps, *O0, *post;
  int* t_dev;  // the current timestep in device memory (graph replay)
  unsigned char* tiles;  // [B][K / 16]: row tiles with a generated residue (the last layer's attention runs for these only)
  int* row_plan;         // [B][2 + K / 16]: the module launch's items of the last layer (launch_row_plan)
  unsigned char* start_class;  // [B] (whole words): the module launch's start class of every patch (launch_start_classes)
  float* beta_traj;      // [3 heads][kTrajRows][D]: the heads' folded beta columns of every step of a schedule with T < kTrajRows
  int* ctx_of_row;       // shared contexts: [B] the context of every state row (device copy of the caller's map)
  float* res_ctx;        // shared contexts: [B][K][D] the residue context of every state row (gathered once per call)
  void* step;
  size_t bytes;
};

// n_pair: patches of the pair embedding (0: d->B); mapped: diffab_sample_loop_ex with a context map (its two buffers)
static SampleBuffers carve_sample(const diffab_dims* d, void* ws, int n_pair = 0, bool mapped = false) {
  Carver c(ws);
  const size_t rows = static_cast<size_t>(d->B) * d->K;
  SampleBuffers s;
  s.beta = c.take<float>(d->B);
  s.eps = c.take<float>(rows * 3);
  s.O0 = c.take<float>(rows * 9);
  s.post = c.take<float>(rows * d->V);
  s.t_dev = c.take<int>(64);
  s.tiles = c.take<unsigned char>(static_cast<size_t>(d->B) * ((d->K + 15) / 16));
  s.row_plan = c.take<int>(static_cast<size_t>(d->B) * (2 + (d->K + 15) / 16));
  s.beta_traj = c.take<float>(static_cast<size_t>(3) * kTrajRows * d->D);
  s.ctx_of_row = mapped ? c.take<int>(d->B) : nullptr;
  s.res_ctx = mapped ? c.take<float>(rows * d->D) : nullptr;  // 256-byte aligned: the folded embedding MLP takes it as it takes the caller's
  const size_t step_bytes = carve_step(d, nullptr, n_pair).bytes;
  s.step = c.take<char>(step_bytes);
  // (behind everything else: no other buffer of the workspace moves for it - the pair planes keep their place relative to the base)
  s.start_class = c.take<unsigned char>((static_cast<size_t>(d->B) + 3) & ~static_cast<size_t>(3));
  s.bytes = c.bytes();
  return s;
}

// diffab_score_designs: the state of one chunk of d->B evaluated rows, and the step buffers of its denoiser call
struct ScoreBuffers {
  int* t_list;    // [kTrajRows] the caller's timestep grid (device copy)
  float* beta;    // [B] beta[t_j] of every row
  int* ctx_of_row;  // [B] the context of every row
  int64_t* seq_t;
  float *x_t, *O_t, *eps, *eps_hat;  // (B,K,3), (B,K,3,3), (B,K,3), (B,K,3)
  float* res_ctx;  // (B,K,D) the residue context of every row (gathered per chunk)
  void* step;
  size_t bytes;
};
static ScoreBuffers carve_score(const diffab_dims* d, void* ws, int n_ctx) {
  Carver c(ws);
  const size_t rows = static_cast<size_t>(d->B) * d->K;
  ScoreBuffers s;
  s.t_list = c.take<int>(kTrajRows);
  s.beta = c.take<float>(d->B);
  s.ctx_of_row = c.take<int>(d->B);
  s.seq_t = c.take<int64_t>(rows);
  s.x_t = c.take<float>(rows * 3);
  s.O_t = c.take<float>(rows * 9);
  s.eps = c.take<float>(rows * 3);
  s.eps_hat = c.take<float>(rows * 3);
  s.res_ctx = c.take<float>(rows * d->D);
  s.step = c.take<char>(carve_step(d, nullptr, n_ctx).bytes);
  s.bytes = c.bytes();
  return s;
}

}  // namespace diffab

using namespace diffab;

extern "C" {

const char* diffab_version(void) { return "diffab_hip 0.1.0 (gfx950)"; }
const char* diffab_last_error(void) { return g_err; }

int diffab_device_ok(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return 0;
  hipDeviceProp_t p;
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || hipGetDeviceProperties(&p, dev) != hipSuccess) return 0;
  return std::strncmp(p.gcnArchName, "gfx950", 6) == 0 ? 1 : 0;
}

int diffab_debug_linear128(const float* X, const float* W, const float* bias, float* Y, int64_t M, int32_t Kd, int32_t mode, void* scratch,
                           size_t scratch_bytes, void* stream) {
  StreamOrder order_(stream);
  DIFFAB_REQUIRE(X && W && Y && M >= 1 && M < (1LL << 31) && Kd >= 32 && Kd % 32 == 0, DIFFAB_ERR_ARG, "debug_linear128: bad operands");
  hipStream_t st = as_stream(stream);
  if (mode == 0) return launch_linear(X, Kd, W, bias, Y, 128, static_cast<int>(M), 128, Kd, false, st);  // rowgemm128 / tiled f32 MFMA
  if (int rc = require_aligned16("debug_linear128", {{"X", X}, {"W", W}, {"bias", bias}, {"Y", Y}})) return rc;  // (modes 1 and 2)
  if (mode == 2) {  // fp16 x 3 (gemm_f16x3.hip): planes | 1 / scale of the 128 weight rows
    const size_t pb = (rowgemm128_h3_planes_bytes(Kd) + 255) & ~static_cast<size_t>(255);
    DIFFAB_REQUIRE(Kd % 64 == 0, DIFFAB_ERR_ARG, "debug_linear128: mode 2 (fp16 x 3) needs Kd %% 64 == 0 (its chunks of 32 k are joined in pairs)");
    DIFFAB_REQUIRE(scratch && scratch_bytes >= pb + 512 && rowgemm128_b6_ok(X, Kd, Y, 128, static_cast<int>(M), Kd) &&
                       (reinterpret_cast<uintptr_t>(scratch) & 15) == 0,
                   DIFFAB_ERR_ARG, "debug_linear128: mode 2 needs 16-byte aligned operands and %zu bytes of scratch", pb + 512);
    float* wis = reinterpret_cast<float*>(static_cast<char*>(scratch) + pb);
    if (int rc = launch_wsplit128_h3(W, Kd, Kd, scratch, wis, st)) return rc;
    return launch_rowgemm128_h3p(X, Kd, scratch, wis, bias, nullptr, 0, Y, 128, static_cast<int>(M), Kd, false, st, nullptr);
  }
  DIFFAB_REQUIRE(mode == 1 && scratch && scratch_bytes >= rowgemm128_b6_scratch_bytes(Kd) && rowgemm128_b6_ok(X, Kd, Y, 128, static_cast<int>(M), Kd),
                 DIFFAB_ERR_ARG, "debug_linear128: mode 1 needs 16-byte aligned operands and %zu bytes of scratch", rowgemm128_b6_scratch_bytes(Kd));
  return launch_rowgemm128_b6(X, Kd, W, Kd, bias, nullptr, 0, Y, 128, static_cast<int>(M), Kd, false, scratch, st);
}

int diffab_debug_xstat128(const float* X, const float* W, float* Y, int64_t M, int32_t N, int32_t mode, void* scratch, size_t scratch_bytes,
                          void* stream) {
  StreamOrder order_(stream);
  DIFFAB_REQUIRE(X && W && Y && scratch && M >= 1 && M < (1LL << 31) && N >= 1 && (mode == 1 || mode == 2), DIFFAB_ERR_ARG,
                 "debug_xstat128: bad operands");
  const size_t need = mode == 1 ? xstat_b6_scratch_bytes(N) : xstat_h3_scratch_bytes(N);
  if (int rc = require_aligned16("debug_xstat128", {{"X", X}, {"W", W}, {"Y", Y}})) return rc;
  DIFFAB_REQUIRE(scratch_bytes >= need && (reinterpret_cast<uintptr_t>(scratch) & 15) == 0 && (reinterpret_cast<uintptr_t>(X) & 15) == 0,
                 DIFFAB_ERR_ARG, "debug_xstat128: needs 16-byte aligned X / scratch and %zu bytes of scratch", need);
  hipStream_t st = as_stream(stream);
  if (mode == 1) return launch_xstat_b6(X, W, 1, N, Y, N, static_cast<int>(M), N, scratch, st);
  return launch_xstat_h3(X, W, 1, N, Y, N, static_cast<int>(M), N, scratch, st);
}

int diffab_debug_dense_forms(int64_t rows, int32_t nblocks, int32_t has_parts, int32_t* out5) {
  DIFFAB_REQUIRE(out5 && rows >= 1 && rows < (1LL << 31) && nblocks >= 1, DIFFAB_ERR_ARG, "debug_dense_forms: bad operands");
  const int M = static_cast<int>(rows);
  const int group = rowgemm128_rows_per_group(M, has_parts != 0);
  out5[0] = group;
  out5[1] = M % (group == 0 ? 64 : group) != 0;
  out5[2] = dense_tile_full(M);
  out5[3] = dense_tile_nsplit(M, nblocks);
  out5[4] = M - (M - 1) / kDenseTileRows * kDenseTileRows;
  return DIFFAB_OK;
}

int diffab_debug_gemm_tn(const float* A, const float* B, float* C, float* db, int64_t M, int32_t N1, int32_t N2, int32_t mode, void* stream) {
  StreamOrder order_(stream);
  DIFFAB_REQUIRE(A && B && C && M >= 1 && M < (1LL << 31) && N1 >= 1 && N2 >= 1 && (mode == 1 || mode == 2), DIFFAB_ERR_ARG,
                 "debug_gemm_tn: bad operands");
  hipStream_t st = as_stream(stream);
  if (mode == 1) return launch_gemm_tn_b6(A, N1, B, N2, C, N2, static_cast<int>(M), N1, N2, db, nullptr, nullptr, 0, st);
  return launch_gemm_tn_h3(A, N1, B, N2, C, N2, static_cast<int>(M), N1, N2, db, nullptr, nullptr, 0, st);
}

int diffab_set_stream_guard(int on) {
  set_stream_order(on != 0);
  return DIFFAB_OK;
}

int diffab_debug_set_module_stagger(int32_t ticks_10ns, int32_t classes) {
  set_module_stagger(ticks_10ns, classes);
  return DIFFAB_OK;
}

int diffab_debug_set_module_stamps(void* device_buffer) {
  set_module_stamps(device_buffer);
  return DIFFAB_OK;
}

int diffab_debug_row_tiles(const uint8_t* gen_mask, int32_t B, int32_t K, uint8_t* tiles, void* stream) {
  StreamOrder order_(stream);
  DIFFAB_REQUIRE(gen_mask && tiles && B >= 1 && K >= 16 && K % 16 == 0, DIFFAB_ERR_ARG, "debug_row_tiles: need B >= 1 and K a multiple of 16");
  return launch_tiles_needed(gen_mask, B, K, tiles, as_stream(stream));
}

int diffab_debug_row_plan(const uint8_t* gen_mask, int32_t B, int32_t K, int32_t* plan, void* stream) {
  StreamOrder order_(stream);
  DIFFAB_REQUIRE(gen_mask && plan && B >= 1 && K >= 16 && K <= 1024 && K % 16 == 0, DIFFAB_ERR_ARG,
                 "debug_row_plan: need B >= 1 and K a multiple of 16 in 16 .. 1024");
  return launch_row_plan(gen_mask, B, K, plan, as_stream(stream));
}

int diffab_debug_start_classes(const int32_t* plan, int32_t B, int32_t K, int32_t classes, uint8_t* out, int32_t on_device, void* stream) {
  DIFFAB_REQUIRE(plan && out && B >= 1 && K >= 16 && K <= 1024 && K % 16 == 0 && classes >= 1 && classes <= 256, DIFFAB_ERR_ARG,
                 "debug_start_classes: need B >= 1, K a multiple of 16 in 16 .. 1024 and 1 .. 256 classes");
  if (on_device) {  // the sampler's own launch, on device buffers
    StreamOrder order_(stream);
    return launch_start_classes(plan, B, K, classes, out, as_stream(stream));
  }
  for (int b = 0; b < B; ++b) out[b] = static_cast<uint8_t>(start_class_of(plan, B, K, classes, b));  // (the device kernel's function, on the host)
  return DIFFAB_OK;
}

int diffab_debug_set_attn_variant(int32_t v) { return set_attn_variant(v); }

int diffab_debug_set_attn_stamps(void* device_buffer) {
  set_attn_stamps(device_buffer);
  return DIFFAB_OK;
}

int diffab_kernel_timer_enable(int on) {
  g_timer.on = on != 0;
  g_timer.used = 0;
  return DIFFAB_OK;
}

int diffab_kernel_timer_read(int64_t* launches, double* total_ms) {
  DIFFAB_REQUIRE(launches && total_ms, DIFFAB_ERR_ARG, "kernel_timer_read: null pointer");
  double tot = 0.0;
  for (size_t i = 0; i + 1 < g_timer.used; i += 2) {
    DIFFAB_HIP_CHECK(hipEventSynchronize(g_timer.ev[i + 1]));
    float ms = 0.f;
    DIFFAB_HIP_CHECK(hipEventElapsedTime(&ms, g_timer.ev[i], g_timer.ev[i + 1]));
    tot += ms;
  }
  *launches = static_cast<int64_t>(g_timer.used / 2);
  *total_ms = tot;
  g_timer.used = 0;
  return DIFFAB_OK;
}

size_t diffab_denoise_workspace_bytes(const diffab_dims* d) {
  if (check_dims(d, "denoise_workspace_bytes")) return 0;
  return carve_step(d, nullptr).bytes;
}

size_t diffab_sample_workspace_bytes(const diffab_dims* d) {
  if (check_dims(d, "sample_workspace_bytes")) return 0;
  return carve_sample(d, nullptr).bytes;
}

size_t diffab_sample_shared_workspace_bytes(const diffab_dims* d, int32_t n_ctx) {
  if (check_dims(d, "sample_shared_workspace_bytes")) return 0;
  if (n_ctx < 1 || static_cast<int64_t>(n_ctx) * d->K >= (1ll << 31)) {
    set_error("sample_shared_workspace_bytes: need 1 <= n_ctx and n_ctx*K < 2^31 (n_ctx=%d)", n_ctx);
    return 0;
  }
  return carve_sample(d, nullptr, n_ctx, true).bytes;
}

int diffab_ipa_layer_fwd(const diffab_dims* d, const diffab_ipa_layer_weights* w, const float* x, const float* e, const float* R,
                         const float* t, float* y, void* workspace, size_t workspace_bytes, uint32_t flags, void* stream) {
  StreamOrder order_(stream);
  if (int rc = check_dims(d, "ipa_layer_fwd")) return rc;
  DIFFAB_REQUIRE(x && (e || d->C == 0) && R && t && y && workspace, DIFFAB_ERR_ARG, "ipa_layer_fwd: null pointer");
  if (int rc = require_aligned16("ipa_layer_fwd", {{"x", x}, {"e", e}, {"R", R}, {"t", t}, {"y", y}})) return rc;
  if (w != nullptr)  // (a null table or field is the dispatch's refusal, behind the workspace check as before)
    if (int rc = check_layer_aligned("ipa_layer_fwd", "w", 0, w)) return rc;
  const StepBuffers b = carve_step(d, workspace);
  DIFFAB_REQUIRE(workspace_bytes >= b.bytes, DIFFAB_ERR_WORKSPACE, "ipa_layer_fwd: workspace %zu < %zu bytes", workspace_bytes, b.bytes);
  const float* pair_planes = nullptr;
  if (use_pair_planes(d, flags, e, b)) {
    if (int rc = launch_pair_split(d, e, b.pair, as_stream(stream))) return rc;
    pair_planes = b.pair;
  }
  return ipa_layer_dispatch(d, w, x, e, R, t, y, b.ipa, flags, as_stream(stream), nullptr, nullptr, nullptr, pair_planes);
}

int diffab_denoise_step_fwd(const diffab_dims* d, const diffab_denoiser_weights* w, const int64_t* seq_t, const float* x_t, const float* O_t,
                            const float* res_ctx, const float* pair_ctx, const float* beta, float* out_eps, float* out_O0,
                            float* out_posterior, float* out_logits, float* out_res_emb, void* workspace, size_t workspace_bytes,
                            uint32_t flags, void* stream) {
  StreamOrder order_(stream);
  if (int rc = check_dims(d, "denoise_step_fwd")) return rc;
  if (int rc = check_denoiser_weights(d, w)) return rc;
  DIFFAB_REQUIRE(seq_t && x_t && O_t && res_ctx && pair_ctx && beta && out_eps && out_O0 && out_posterior && workspace, DIFFAB_ERR_ARG,
                 "denoise_step_fwd: null pointer");
  if (int rc = require_aligned16("denoise_step_fwd", {{"x_t", x_t}, {"O_t", O_t}, {"res_ctx", res_ctx}, {"pair_ctx", pair_ctx}, {"beta", beta},
                                                      {"out_eps", out_eps}, {"out_O0", out_O0}, {"out_posterior", out_posterior},
                                                      {"out_logits", out_logits}, {"out_res_emb", out_res_emb}}))
    return rc;
  if (int rc = check_denoiser_aligned("denoise_step_fwd", "w", d, w)) return rc;
  const StepBuffers b = carve_step(d, workspace);
  DIFFAB_REQUIRE(workspace_bytes >= b.bytes, DIFFAB_ERR_WORKSPACE, "denoise_step_fwd: workspace %zu < %zu bytes", workspace_bytes, b.bytes);
  hipStream_t st = as_stream(stream);
  const ForwardPlan p = plan_forward(d, flags, b, res_ctx, pair_ctx, out_res_emb, false);
  const StepBias bias{beta};
  if (int rc = prepare_forward(d, w, p, b, pair_ctx, bias, st)) return rc;
  return denoise_step(d, w, p, bias, seq_t, x_t, O_t, res_ctx, pair_ctx, out_eps, out_O0, out_posterior, out_logits, b, st);
}

// The taped forwards refuse dims whose backward cannot run (attn_bwd_lds_ok, the predicate run_backward checks), so that a training step
// fails before anything is launched rather than inside the layer loop, after the heads' backward has been enqueued.
static int check_attn_bwd_lds(const diffab_dims* d, const char* who) {
  DIFFAB_REQUIRE(attn_bwd_lds_ok(d), DIFFAB_ERR_UNSUPPORTED,
                 "%s: H*K = %d too large for the attention backward's LDS (%zu > %zu bytes; the forward alone reaches further)", who,
                 d->H * d->K, attn_bwd_lds_bytes(d), kAttnBwdLdsMax);
  return DIFFAB_OK;
}

size_t diffab_train_tape_bytes(const diffab_dims* d) {
  if (check_dims(d, "train_tape_bytes") || d->NL > kMaxLayers) return 0;
  return train_tape_floats(d) * sizeof(float);
}

size_t diffab_train_workspace_bytes(const diffab_dims* d) {
  if (check_dims(d, "train_workspace_bytes")) return 0;
  return train_bwd_workspace_floats(d) * sizeof(float);
}

int diffab_train_step_fwd(const diffab_dims* d, const diffab_denoiser_weights* w, const int64_t* seq_t, const float* x_t, const float* O_t,
                          const float* res_ctx, const float* pair_ctx, const float* beta, const float* true_post, const float* true_eps,
                          const float* true_O0, const uint8_t* gen_mask, const uint8_t* res_mask, float* out_eps, float* out_O0,
                          float* out_posterior, float* losses3, void* tape, size_t tape_bytes, uint32_t flags, void* stream) {
  StreamOrder order_(stream);
  if (int rc = check_dims(d, "train_step_fwd")) return rc;
  if (int rc = check_denoiser_weights(d, w)) return rc;
  DIFFAB_REQUIRE(d->NL <= kMaxLayers, DIFFAB_ERR_UNSUPPORTED, "train_step_fwd: at most %d IPA layers", kMaxLayers);
  if (int rc = check_attn_bwd_lds(d, "train_step_fwd")) return rc;
  DIFFAB_REQUIRE(seq_t && x_t && O_t && res_ctx && pair_ctx && beta && true_post && true_eps && true_O0 && gen_mask && res_mask && out_eps &&
                     out_O0 && out_posterior && losses3 && tape,
                 DIFFAB_ERR_ARG, "train_step_fwd: null pointer");
  if (int rc = require_aligned16("train_step_fwd", {{"x_t", x_t}, {"O_t", O_t}, {"res_ctx", res_ctx}, {"pair_ctx", pair_ctx}, {"beta", beta},
                                                    {"true_post", true_post}, {"true_eps", true_eps}, {"true_O0", true_O0}, {"out_eps", out_eps},
                                                    {"out_O0", out_O0}, {"out_posterior", out_posterior}, {"losses3", losses3}}))
    return rc;
  if (int rc = check_denoiser_aligned("train_step_fwd", "w", d, w)) return rc;
  DIFFAB_REQUIRE(tape_bytes >= train_tape_floats(d) * sizeof(float), DIFFAB_ERR_WORKSPACE, "train_step_fwd: tape %zu < %zu bytes", tape_bytes,
                 train_tape_floats(d) * sizeof(float));
  const TrainTape tp = carve_tape(d, static_cast<float*>(tape));
  hipStream_t st = as_stream(stream);
  flags = taped_flags(flags);
  if (int rc = denoise_step_taped(d, w, seq_t, x_t, O_t, res_ctx, pair_ctx, beta, out_eps, out_O0, out_posterior, tp, flags, st)) return rc;
  return launch_losses_fwd(out_posterior, true_post, out_eps, true_eps, out_O0, true_O0, gen_mask, res_mask, d->B, d->K, d->V, losses3, st,
                           tp.scratch);
}

int diffab_train_step_bwd(const diffab_dims* d, const diffab_denoiser_weights* w, const diffab_denoiser_weights* grads,
                          const int64_t* seq_t, const float* x_t, const float* O_t, const float* pair_ctx, const float* out_eps,
                          const float* out_O0, const float* out_posterior, const float* true_post, const float* true_eps,
                          const float* true_O0, const uint8_t* gen_mask, const uint8_t* res_mask, const float* upstream3, float* d_res_ctx,
                          float* d_pair_ctx, const void* tape, size_t tape_bytes, void* workspace, size_t workspace_bytes, void* stream) {
  StreamOrder order_(stream);
  if (int rc = check_dims(d, "train_step_bwd")) return rc;
  if (int rc = check_denoiser_weights(d, w)) return rc;
  if (int rc = check_denoiser_weights(d, grads)) return rc;
  DIFFAB_REQUIRE(d->NL <= kMaxLayers, DIFFAB_ERR_UNSUPPORTED, "train_step_bwd: at most %d IPA layers", kMaxLayers);
  if (int rc = check_attn_bwd_lds(d, "train_step_bwd")) return rc;
  DIFFAB_REQUIRE(seq_t && x_t && O_t && pair_ctx && out_eps && out_O0 && out_posterior && true_post && true_eps && true_O0 && gen_mask &&
                     res_mask && upstream3 && tape && workspace,
                 DIFFAB_ERR_ARG, "train_step_bwd: null pointer");
  if (int rc = require_aligned16("train_step_bwd", {{"x_t", x_t}, {"O_t", O_t}, {"pair_ctx", pair_ctx}, {"out_eps", out_eps}, {"out_O0", out_O0},
                                                    {"out_posterior", out_posterior}, {"true_post", true_post}, {"true_eps", true_eps},
                                                    {"true_O0", true_O0}, {"upstream3", upstream3}, {"d_res_ctx", d_res_ctx},
                                                    {"d_pair_ctx", d_pair_ctx}}))
    return rc;
  if (int rc = check_denoiser_aligned("train_step_bwd", "w", d, w)) return rc;
  if (int rc = check_denoiser_aligned("train_step_bwd", "grads", d, grads)) return rc;
  DIFFAB_REQUIRE(tape_bytes >= train_tape_floats(d) * sizeof(float), DIFFAB_ERR_WORKSPACE, "train_step_bwd: tape too small");
  DIFFAB_REQUIRE(workspace_bytes >= train_bwd_workspace_floats(d) * sizeof(float), DIFFAB_ERR_WORKSPACE, "train_step_bwd: workspace %zu < %zu",
                 workspace_bytes, train_bwd_workspace_floats(d) * sizeof(float));
  BackwardArgs a{};
  a.root = BWD_LOSSES;
  a.d = d; a.w = w; a.g = grads;
  a.tp = carve_tape(d, static_cast<float*>(const_cast<void*>(tape)));
  a.ws = static_cast<float*>(workspace); a.st = as_stream(stream);
  a.seq_t = seq_t; a.trans = x_t; a.rot = O_t; a.pair_ctx = pair_ctx;
  a.eps_hat = out_eps; a.O0_hat = out_O0; a.post_hat = out_posterior;
  a.true_post = true_post; a.true_eps = true_eps; a.true_O0 = true_O0;
  a.gm = gen_mask; a.rm = res_mask; a.upstream3 = upstream3;
  a.d_res_ctx = d_res_ctx; a.d_pair_ctx = d_pair_ctx;
  return run_backward(a);
}

/* ---- Denoiser.forward / InvariantPointAttentionLayer.forward under autograd: taped forward + backward from arbitrary cotangents ---- */
int diffab_denoise_step_fwd_taped(const diffab_dims* d, const diffab_denoiser_weights* w, const int64_t* seq_t, const float* x_t,
                                  const float* O_t, const float* res_ctx, const float* pair_ctx, const float* beta, float* out_eps,
                                  float* out_O0, float* out_posterior, void* tape, size_t tape_bytes, uint32_t flags, void* stream) {
  StreamOrder order_(stream);
  if (int rc = check_dims(d, "denoise_step_fwd_taped")) return rc;
  if (int rc = check_denoiser_weights(d, w)) return rc;
  DIFFAB_REQUIRE(d->NL <= kMaxLayers, DIFFAB_ERR_UNSUPPORTED, "denoise_step_fwd_taped: at most %d IPA layers", kMaxLayers);
  if (int rc = check_attn_bwd_lds(d, "denoise_step_fwd_taped")) return rc;
  DIFFAB_REQUIRE(seq_t && x_t && O_t && res_ctx && pair_ctx && beta && out_eps && out_O0 && out_posterior && tape, DIFFAB_ERR_ARG,
                 "denoise_step_fwd_taped: null pointer");
  if (int rc = require_aligned16("denoise_step_fwd_taped", {{"x_t", x_t}, {"O_t", O_t}, {"res_ctx", res_ctx}, {"pair_ctx", pair_ctx},
                                                            {"beta", beta}, {"out_eps", out_eps}, {"out_O0", out_O0},
                                                            {"out_posterior", out_posterior}}))
    return rc;
  if (int rc = check_denoiser_aligned("denoise_step_fwd_taped", "w", d, w)) return rc;
  DIFFAB_REQUIRE(tape_bytes >= train_tape_floats(d) * sizeof(float), DIFFAB_ERR_WORKSPACE, "denoise_step_fwd_taped: tape %zu < %zu bytes",
                 tape_bytes, train_tape_floats(d) * sizeof(float));
  const TrainTape tp = carve_tape(d, static_cast<float*>(tape));
  return denoise_step_taped(d, w, seq_t, x_t, O_t, res_ctx, pair_ctx, beta, out_eps, out_O0, out_posterior, tp, taped_flags(flags), as_stream(stream));
}

int diffab_denoise_step_bwd(const diffab_dims* d, const diffab_denoiser_weights* w, const diffab_denoiser_weights* grads,
                            const int64_t* seq_t, const float* x_t, const float* O_t, const float* pair_ctx, const float* out_posterior,
                            const float* d_eps, const float* d_O0, const float* d_posterior, float* d_res_ctx, float* d_pair_ctx,
                            float* d_x_t, float* d_O_t, const void* tape, size_t tape_bytes, void* workspace, size_t workspace_bytes,
                            void* stream) {
  StreamOrder order_(stream);
  if (int rc = check_dims(d, "denoise_step_bwd")) return rc;
  if (int rc = check_denoiser_weights(d, w)) return rc;
  if (int rc = check_denoiser_weights(d, grads)) return rc;
  DIFFAB_REQUIRE(d->NL <= kMaxLayers, DIFFAB_ERR_UNSUPPORTED, "denoise_step_bwd: at most %d IPA layers", kMaxLayers);
  if (int rc = check_attn_bwd_lds(d, "denoise_step_bwd")) return rc;
  DIFFAB_REQUIRE(seq_t && x_t && O_t && pair_ctx && out_posterior && d_res_ctx && tape && workspace, DIFFAB_ERR_ARG,
                 "denoise_step_bwd: null pointer");
  if (int rc = require_aligned16("denoise_step_bwd", {{"x_t", x_t}, {"O_t", O_t}, {"pair_ctx", pair_ctx}, {"out_posterior", out_posterior},
                                                      {"d_eps", d_eps}, {"d_O0", d_O0}, {"d_posterior", d_posterior}, {"d_res_ctx", d_res_ctx},
                                                      {"d_pair_ctx", d_pair_ctx}, {"d_x_t", d_x_t}, {"d_O_t", d_O_t}}))
    return rc;
  if (int rc = check_denoiser_aligned("denoise_step_bwd", "w", d, w)) return rc;
  if (int rc = check_denoiser_aligned("denoise_step_bwd", "grads", d, grads)) return rc;
  DIFFAB_REQUIRE(tape_bytes >= train_tape_floats(d) * sizeof(float), DIFFAB_ERR_WORKSPACE, "denoise_step_bwd: tape too small");
  DIFFAB_REQUIRE(workspace_bytes >= train_bwd_workspace_floats(d) * sizeof(float), DIFFAB_ERR_WORKSPACE, "denoise_step_bwd: workspace %zu < %zu",
                 workspace_bytes, train_bwd_workspace_floats(d) * sizeof(float));
  BackwardArgs a{};
  a.root = BWD_COTANGENTS;
  a.d = d; a.w = w; a.g = grads;
  a.tp = carve_tape(d, static_cast<float*>(const_cast<void*>(tape)));
  a.ws = static_cast<float*>(workspace); a.st = as_stream(stream);
  a.seq_t = seq_t; a.trans = x_t; a.rot = O_t; a.pair_ctx = pair_ctx;
  a.post_hat = out_posterior;
  a.cot_eps = d_eps; a.cot_O0 = d_O0; a.cot_post = d_posterior;
  a.d_res_ctx = d_res_ctx; a.d_pair_ctx = d_pair_ctx; a.d_trans = d_x_t; a.d_rot = d_O_t;
  return run_backward(a);
}

static diffab_dims one_layer(const diffab_dims* d) {
  diffab_dims d1 = *d;
  d1.NL = 1;
  return d1;
}
size_t diffab_ipa_layer_tape_bytes(const diffab_dims* d) {
  if (check_dims(d, "ipa_layer_tape_bytes")) return 0;
  const diffab_dims d1 = one_layer(d);
  return train_tape_floats(&d1) * sizeof(float);
}
size_t diffab_ipa_layer_bwd_workspace_bytes(const diffab_dims* d) {
  if (check_dims(d, "ipa_layer_bwd_workspace_bytes")) return 0;
  const diffab_dims d1 = one_layer(d);
  return train_bwd_workspace_floats(&d1) * sizeof(float);
}

int diffab_ipa_layer_fwd_taped(const diffab_dims* d, const diffab_ipa_layer_weights* w, const float* x, const float* e, const float* R,
                               const float* t, float* y, void* tape, size_t tape_bytes, uint32_t flags, void* stream) {
  StreamOrder order_(stream);
  if (int rc = check_dims(d, "ipa_layer_fwd_taped")) return rc;
  DIFFAB_REQUIRE(x && (e || d->C == 0) && R && t && y && tape, DIFFAB_ERR_ARG, "ipa_layer_fwd_taped: null pointer");
  if (int rc = require_aligned16("ipa_layer_fwd_taped", {{"x", x}, {"e", e}, {"R", R}, {"t", t}, {"y", y}})) return rc;
  if (w != nullptr)  // (a null table or field is the dispatch's refusal, behind the workspace check as before)
    if (int rc = check_layer_aligned("ipa_layer_fwd_taped", "w", 0, w)) return rc;
  const diffab_dims d1 = one_layer(d);
  if (int rc = check_attn_bwd_lds(&d1, "ipa_layer_fwd_taped")) return rc;
  DIFFAB_REQUIRE(tape_bytes >= train_tape_floats(&d1) * sizeof(float), DIFFAB_ERR_WORKSPACE, "ipa_layer_fwd_taped: tape %zu < %zu bytes", tape_bytes,
                 train_tape_floats(&d1) * sizeof(float));
  const TrainTape tp = carve_tape(&d1, static_cast<float*>(tape));
  hipStream_t st = as_stream(stream);
  const size_t nb = sizeof(float) * static_cast<size_t>(d->B) * d->K * d->D;
  DIFFAB_HIP_CHECK(hipMemcpyAsync(tp.x[0], x, nb, hipMemcpyDeviceToDevice, st));
  flags = taped_flags(flags);
  const bool b6 = plan_backward(&d1).fast && use_b6_gemm(flags);
  if (b6)
    if (int rc = ipa_layer_split_weights(w, tp.planes, st)) return rc;
  if (int rc = ipa_layer_dispatch(&d1, w, tp.x[0], e, R, t, tp.x[1], tp.ipa_ws[0], flags, st, tp.sp[0], tp.d2[0], b6 ? tp.planes : nullptr,
                                  nullptr, true))
    return rc;
  DIFFAB_HIP_CHECK(hipMemcpyAsync(y, tp.x[1], nb, hipMemcpyDeviceToDevice, st));
  return DIFFAB_OK;
}

int diffab_ipa_layer_bwd(const diffab_dims* d, const diffab_ipa_layer_weights* w, const diffab_ipa_layer_weights* grads, const float* e,
                         const float* R, const float* t, const float* dy, float* dx, float* d_e, float* d_R, float* d_t, const void* tape,
                         size_t tape_bytes, void* workspace, size_t workspace_bytes, void* stream) {
  StreamOrder order_(stream);
  if (int rc = check_dims(d, "ipa_layer_bwd")) return rc;
  DIFFAB_REQUIRE(w && grads && (e || d->C == 0) && R && t && dy && dx && tape && workspace, DIFFAB_ERR_ARG, "ipa_layer_bwd: null pointer");
  if (int rc = require_aligned16("ipa_layer_bwd", {{"e", e}, {"R", R}, {"t", t}, {"dy", dy}, {"dx", dx}, {"d_e", d_e}, {"d_R", d_R}, {"d_t", d_t}}))
    return rc;
  if (int rc = check_layer_aligned("ipa_layer_bwd", "w", 0, w)) return rc;
  if (int rc = check_layer_aligned("ipa_layer_bwd", "grads", 0, grads)) return rc;
  const diffab_dims d1 = one_layer(d);
  if (int rc = check_attn_bwd_lds(&d1, "ipa_layer_bwd")) return rc;
  DIFFAB_REQUIRE(tape_bytes >= train_tape_floats(&d1) * sizeof(float), DIFFAB_ERR_WORKSPACE, "ipa_layer_bwd: tape too small");
  DIFFAB_REQUIRE(workspace_bytes >= train_bwd_workspace_floats(&d1) * sizeof(float), DIFFAB_ERR_WORKSPACE, "ipa_layer_bwd: workspace %zu < %zu",
                 workspace_bytes, train_bwd_workspace_floats(&d1) * sizeof(float));
  // One IPA layer backward: the one-layer tape of the taped layer forward (x[0] = the layer input), dy -> dx, d_e += ..
  diffab_denoiser_weights w1{}, g1{};
  w1.layers = w;
  g1.layers = grads;
  BackwardArgs a{};
  a.root = BWD_LAYER;
  a.d = &d1; a.w = &w1; a.g = &g1;
  a.tp = carve_tape(&d1, static_cast<float*>(const_cast<void*>(tape)));
  a.ws = static_cast<float*>(workspace); a.st = as_stream(stream);
  a.trans = t; a.rot = R; a.pair_ctx = e;
  a.layer_dy = dy; a.layer_dx = dx;
  a.d_pair_ctx = d_e; a.d_trans = d_t; a.d_rot = d_R;
  return run_backward(a);
}

// ---- the options of diffab_sample_loop_ex: one helper per option checks the caller's struct (everything on the host, before the first
// HIP call) and fills the by-value device struct the update kernel takes.  A NULL option leaves `out` default-constructed: off.

// trajectory recording: every slot is written by exactly one step of this call, so the record holds no stale entry
static int record_option(const diffab_sample_record* rec, const diffab_sched* s, int t_start, int t_stop, SampleRecordDev* out) {
  if (rec == nullptr) return DIFFAB_OK;
  DIFFAB_REQUIRE(rec->n_slots >= 1, DIFFAB_ERR_ARG, "sample_loop: record n_slots = %d < 1", rec->n_slots);
  DIFFAB_REQUIRE(rec->slot_of_step && rec->slot_dev && rec->seq && rec->x && rec->O, DIFFAB_ERR_ARG,
                 "sample_loop: record needs slot_of_step, slot_dev, seq, x and O");
  const int n_pred = (rec->pred_x != nullptr) + (rec->pred_O != nullptr) + (rec->seq_probs != nullptr);
  DIFFAB_REQUIRE(n_pred == 0 || n_pred == 3, DIFFAB_ERR_ARG, "sample_loop: record predictions are pred_x, pred_O and seq_probs, all or none");
  DIFFAB_REQUIRE(n_pred == 0 || s->alpha_bar_sqrt, DIFFAB_ERR_ARG, "sample_loop: record predictions need the schedule's alpha_bar_sqrt");
  std::vector<int> used(rec->n_slots, 0);
  for (int t = 0; t <= s->T; ++t) {
    const int j = rec->slot_of_step[t];
    if (j == -1) continue;
    DIFFAB_REQUIRE(j >= 0 && j < rec->n_slots, DIFFAB_ERR_ARG, "sample_loop: record slot_of_step[%d] = %d outside -1, [0, %d)", t, j,
                   rec->n_slots);
    DIFFAB_REQUIRE(t > t_stop && t <= t_start, DIFFAB_ERR_ARG,
                   "sample_loop: record slot_of_step[%d] = %d, but the call runs steps [%d, %d] only (the slot would never be written)", t, j,
                   t_stop + 1, t_start);
    DIFFAB_REQUIRE(used[j]++ == 0, DIFFAB_ERR_ARG, "sample_loop: record slot %d is given to two steps", j);
  }
  for (int j = 0; j < rec->n_slots; ++j)
    DIFFAB_REQUIRE(used[j] == 1, DIFFAB_ERR_ARG, "sample_loop: record slot %d is given to no step", j);
  *out = SampleRecordDev{rec->slot_dev, rec->n_slots, rec->seq, rec->x, rec->O, rec->pred_x, rec->pred_O, rec->seq_probs,
                         n_pred ? s->alpha_bar_sqrt : nullptr};
  return DIFFAB_OK;
}

// fewer-step sampling: the list, its jump coefficients and the record are checked, and the device plan - next[], beta'[], alpha'[] - is
// packed into plan_host (the loop copies it to plan_dev once, after every check)
static int steps_option(const diffab_sample_steps* steps, const diffab_sample_record* rec, const diffab_sched* s, int t_start, int t_stop,
                        std::vector<int32_t>* plan_host, StepPlanDev* out) {
  if (steps == nullptr) return DIFFAB_OK;
  const int T = s->T;
  DIFFAB_REQUIRE(steps->n_steps >= 1, DIFFAB_ERR_ARG, "sample_loop: steps n_steps = %d < 1", steps->n_steps);
  DIFFAB_REQUIRE(steps->steps && steps->beta_jump && steps->alpha_jump && steps->plan_dev, DIFFAB_ERR_ARG,
                 "sample_loop: steps needs steps, beta_jump, alpha_jump and plan_dev");
  DIFFAB_REQUIRE(s->alpha_bar, DIFFAB_ERR_ARG, "sample_loop: steps need the schedule's alpha_bar");
  DIFFAB_REQUIRE(steps->steps[0] == t_start, DIFFAB_ERR_ARG, "sample_loop: steps[0] = %d, t_start = %d", steps->steps[0], t_start);
  std::vector<char> listed(T + 1, 0);
  for (int j = 0; j < steps->n_steps; ++j) {
    const int t = steps->steps[j];
    DIFFAB_REQUIRE(t > t_stop && t <= T, DIFFAB_ERR_ARG, "sample_loop: steps[%d] = %d outside [t_stop + 1, T] = [%d, %d]", j, t, t_stop + 1, T);
    DIFFAB_REQUIRE(j == 0 || t < steps->steps[j - 1], DIFFAB_ERR_ARG, "sample_loop: steps are not strictly descending at %d (%d after %d)", j,
                   t, steps->steps[j - 1]);
    const float bj = steps->beta_jump[t], aj = steps->alpha_jump[t];
    DIFFAB_REQUIRE(bj > 0.0f && bj < 1.0f && aj > 0.0f && aj < 1.0f, DIFFAB_ERR_ARG,
                   "sample_loop: jump coefficients at step %d outside (0, 1): beta' = %g, alpha' = %g", t, bj, aj);
    listed[t] = 1;
  }
  if (rec != nullptr)
    for (int t = 0; t <= T; ++t)
      DIFFAB_REQUIRE(rec->slot_of_step[t] == -1 || listed[t], DIFFAB_ERR_ARG,
                     "sample_loop: record slot_of_step[%d] = %d, but the step list does not run step %d", t, rec->slot_of_step[t], t);
  plan_host->resize(3 * static_cast<size_t>(T + 1));
  int32_t* ph = plan_host->data();
  for (int t = 0; t <= T; ++t) ph[t] = t > 0 ? t - 1 : 0;
  for (int j = 0; j < steps->n_steps; ++j) ph[steps->steps[j]] = j + 1 < steps->n_steps ? steps->steps[j + 1] : t_stop;
  std::memcpy(ph + (T + 1), steps->beta_jump, sizeof(float) * (T + 1));
  std::memcpy(ph + 2 * (T + 1), steps->alpha_jump, sizeof(float) * (T + 1));
  const int32_t* pd = static_cast<const int32_t*>(steps->plan_dev);
  *out = StepPlanDev{pd, reinterpret_cast<const float*>(pd + (T + 1)), reinterpret_cast<const float*>(pd + 2 * (T + 1)), s->alpha_bar};
  return DIFFAB_OK;
}

// structure guidance: the potential's terms and per-residue tables; its kernel runs before every update
static int guidance_option(const diffab_sample_guidance* guidance, const diffab_sched* s, uint32_t keep, GuidanceDev* out) {
  if (guidance == nullptr) return DIFFAB_OK;
  if (int rc = check_guidance_terms(guidance, "sample_loop")) return rc;
  DIFFAB_REQUIRE(guidance->max_shift > 0.0f, DIFFAB_ERR_ARG, "sample_loop: guidance max_shift = %g must be > 0 (INFINITY: no cap)",
                 guidance->max_shift);
  DIFFAB_REQUIRE(guidance->t_max >= 0 && guidance->t_max <= s->T, DIFFAB_ERR_ARG, "sample_loop: guidance t_max = %d outside [0, T = %d]",
                 guidance->t_max, s->T);
  DIFFAB_REQUIRE(guidance->shift_dev != nullptr, DIFFAB_ERR_ARG, "sample_loop: guidance needs shift_dev");
  DIFFAB_REQUIRE(!(keep & DIFFAB_FLAG_KEEP_STRUCTURE), DIFFAB_ERR_ARG,
                 "sample_loop: guidance moves the structure, which DIFFAB_FLAG_KEEP_STRUCTURE does not sample");
  DIFFAB_REQUIRE(s->alpha_bar_sqrt, DIFFAB_ERR_ARG, "sample_loop: guidance needs the schedule's alpha_bar_sqrt");
  out->shift = guidance->shift_dev;
  out->chain = guidance->chain;
  out->residue_idx = guidance->residue_idx;
  out->residue_mask = guidance->residue_mask;
  out->w_clash = guidance->w_clash;
  out->clash_distance = guidance->clash_distance;
  out->w_bond = guidance->w_bond;
  out->bond_length = guidance->bond_length;
  out->max_shift = guidance->max_shift;
  out->t_max = guidance->t_max;
  return DIFFAB_OK;
}

// noise scales and sequence temperature: the pointers are checked (the per-row values are the caller's contract, like `allowed`)
static int temperature_option(const diffab_sample_temperature* temperature, uint32_t keep, TemperatureDev* out) {
  if (temperature == nullptr) return DIFFAB_OK;
  DIFFAB_REQUIRE(!temperature->rot_scale || temperature->rot_row, DIFFAB_ERR_ARG,
                 "sample_loop: temperature rot_scale needs rot_row (its rows of the stacked reverse table)");
  DIFFAB_REQUIRE(!((temperature->trans_scale || temperature->rot_scale) && (keep & DIFFAB_FLAG_KEEP_STRUCTURE)), DIFFAB_ERR_ARG,
                 "sample_loop: noise scales act on the structure, which DIFFAB_FLAG_KEEP_STRUCTURE does not sample");
  DIFFAB_REQUIRE(!(temperature->seq_temp && (keep & DIFFAB_FLAG_KEEP_SEQUENCE)), DIFFAB_ERR_ARG,
                 "sample_loop: a sequence temperature acts on the sequence, which DIFFAB_FLAG_KEEP_SEQUENCE does not sample");
  *out = TemperatureDev{temperature->trans_scale, temperature->rot_scale, temperature->seq_temp, temperature->rot_row};
  return DIFFAB_OK;
}

// particle steering: terms, tables and buffers; its kernels run around every update (the energy before it, weights, resampling and the
// gather after it) and decide themselves which steps steer.  next_host: the packed step plan's next[] (nullptr: t - 1)
static int steering_option(const diffab_sample_steering* q, const diffab_dims* d, const diffab_sched* s, uint32_t keep, int t_stop,
                           const int32_t* next_host, SteeringDev* out) {
  if (q == nullptr) return DIFFAB_OK;
  diffab_sample_guidance terms{};
  terms.w_clash = q->w_clash;
  terms.clash_distance = q->clash_distance;
  terms.w_bond = q->w_bond;
  terms.bond_length = q->bond_length;
  terms.chain = q->chain;
  terms.residue_idx = q->residue_idx;
  if (int rc = check_guidance_terms(&terms, "sample_loop (steering)")) return rc;
  DIFFAB_REQUIRE(q->group_size >= 1 && q->group_size <= DIFFAB_STEER_MAX_GROUP, DIFFAB_ERR_ARG,
                 "sample_loop: steering group_size = %d outside [1, %d]", q->group_size, DIFFAB_STEER_MAX_GROUP);
  DIFFAB_REQUIRE(d->B % q->group_size == 0, DIFFAB_ERR_ARG, "sample_loop: %d rows are not a multiple of the steering group_size = %d", d->B,
                 q->group_size);
  DIFFAB_REQUIRE(std::isfinite(q->strength) && q->strength >= 0.0f, DIFFAB_ERR_ARG,
                 "sample_loop: steering strength = %g must be finite and >= 0", q->strength);
  DIFFAB_REQUIRE(q->ess_threshold >= 0.0f && q->ess_threshold <= 2.0f, DIFFAB_ERR_ARG, "sample_loop: steering ess_threshold = %g outside [0, 2]",
                 q->ess_threshold);
  DIFFAB_REQUIRE(q->t_min >= 0 && q->t_min <= q->t_max && q->t_max <= s->T, DIFFAB_ERR_ARG,
                 "sample_loop: steering needs 0 <= t_min <= t_max <= T (t_min = %d, t_max = %d, T = %d)", q->t_min, q->t_max, s->T);
  DIFFAB_REQUIRE(q->every >= 1, DIFFAB_ERR_ARG, "sample_loop: steering every = %d < 1", q->every);
  DIFFAB_REQUIRE(q->logw && q->u_prev && q->energy && q->scratch, DIFFAB_ERR_ARG, "sample_loop: steering needs logw, u_prev, energy and scratch");
  DIFFAB_REQUIRE(reinterpret_cast<uintptr_t>(q->scratch) % 8 == 0, DIFFAB_ERR_ARG, "sample_loop: steering scratch must be 8-byte aligned");
  DIFFAB_REQUIRE(!(keep & DIFFAB_FLAG_KEEP_STRUCTURE), DIFFAB_ERR_ARG,
                 "sample_loop: steering weighs the sampled structure, which DIFFAB_FLAG_KEEP_STRUCTURE does not sample");
  DIFFAB_REQUIRE(s->alpha_bar_sqrt, DIFFAB_ERR_ARG, "sample_loop: steering needs the schedule's alpha_bar_sqrt");
  out->logw = q->logw;
  out->u_prev = q->u_prev;
  out->energy = q->energy;
  out->ancestors = q->ancestors;
  out->scratch = q->scratch;
  out->step_anc = reinterpret_cast<int32_t*>(static_cast<char*>(q->scratch) + static_cast<size_t>(d->B) * d->K * 56u);
  out->chain = q->chain;
  out->residue_idx = q->residue_idx;
  out->residue_mask = q->residue_mask;
  out->w_clash = q->w_clash;
  out->clash_distance = q->clash_distance;
  out->w_bond = q->w_bond;
  out->bond_length = q->bond_length;
  out->strength = q->strength;
  out->ess_threshold = q->ess_threshold;
  out->t_min = q->t_min;
  out->t_max = q->t_max;
  out->every = q->every;
  out->group_size = q->group_size;
  out->t_stop = t_stop;
  out->next_host = next_host;
  return DIFFAB_OK;
}

// Shared contexts: state row b reads context ctx_of_row[b] of n_ctx (0: d->B).  The map is checked here, on the host, so that no kernel
// can index outside the caller's contexts; a map that is the identity launches exactly the one-context-per-row form.
static int context_map_option(const diffab_dims* d, const int32_t* ctx_of_row, int* n_ctx, bool* identity) {
  if (*n_ctx == 0) *n_ctx = d->B;
  DIFFAB_REQUIRE(ctx_of_row != nullptr || *n_ctx == d->B, DIFFAB_ERR_ARG, "sample_loop: without ctx_of_row n_ctx must equal B (%d != %d)",
                 *n_ctx, d->B);
  DIFFAB_REQUIRE(*n_ctx >= 1 && static_cast<int64_t>(*n_ctx) * d->K < (1ll << 31), DIFFAB_ERR_ARG, "sample_loop: need 1 <= n_ctx, n_ctx*K < 2^31");
  *identity = *n_ctx == d->B;
  for (int b = 0; ctx_of_row != nullptr && b < d->B; ++b) {
    DIFFAB_REQUIRE(ctx_of_row[b] >= 0 && ctx_of_row[b] < *n_ctx, DIFFAB_ERR_ARG, "sample_loop: ctx_of_row[%d] = %d outside [0, %d)", b,
                   ctx_of_row[b], *n_ctx);
    *identity = *identity && ctx_of_row[b] == b;
  }
  return DIFFAB_OK;
}

int diffab_sample_loop(const diffab_dims* d, const diffab_denoiser_weights* w, const diffab_sched* s, const diffab_igso3* rev_tab,
                       int64_t* seq, float* x, float* O, const float* res_ctx, const float* pair_ctx, const uint8_t* gen_mask, uint64_t seed,
                       int64_t first_patch, int32_t t_start, int32_t t_stop, void* workspace, size_t workspace_bytes, uint32_t flags,
                       void* stream) {
  return diffab_sample_loop_ex(d, w, s, rev_tab, seq, x, O, res_ctx, pair_ctx, gen_mask, seed, first_patch, t_start, t_stop, workspace,
                               workspace_bytes, flags, nullptr, stream);
}

int diffab_sample_loop_ex(const diffab_dims* d, const diffab_denoiser_weights* w, const diffab_sched* s, const diffab_igso3* rev_tab,
                          int64_t* seq, float* x, float* O, const float* res_ctx, const float* pair_ctx, const uint8_t* gen_mask, uint64_t seed,
                          int64_t first_patch, int32_t t_start, int32_t t_stop, void* workspace, size_t workspace_bytes, uint32_t flags,
                          const diffab_sample_options* opt_in, void* stream) {
  StreamOrder order_(stream);
  DIFFAB_REQUIRE(!opt_in || opt_in->struct_bytes == sizeof(diffab_sample_options), DIFFAB_ERR_ARG,
                 "sample_loop: options struct_bytes = %u, this library's diffab_sample_options has %zu", opt_in->struct_bytes,
                 sizeof(diffab_sample_options));
  diffab_sample_options none{};  // NULL options: every option off, exactly the zeroed struct
  const diffab_sample_options* opt = opt_in ? opt_in : &none;
  if (int rc = check_dims(d, "sample_loop")) return rc;
  if (int rc = check_denoiser_weights(d, w)) return rc;
  DIFFAB_REQUIRE(s && s->T > 0 && s->alpha && s->beta && s->one_minus_alpha_bar_sqrt, DIFFAB_ERR_ARG, "sample_loop: bad schedule");
  DIFFAB_REQUIRE(rev_tab && rev_tab->sigmas && rev_tab->cdf && rev_tab->n_sigmas >= s->T + 1 && rev_tab->n_bins > 0, DIFFAB_ERR_ARG,
                 "sample_loop: reverse IGSO3 table must have T+1 rows");
  DIFFAB_REQUIRE(seq && x && O && res_ctx && pair_ctx && gen_mask && workspace, DIFFAB_ERR_ARG, "sample_loop: null pointer");
  if (int rc = require_aligned16("sample_loop", {{"x", x}, {"O", O}, {"res_ctx", res_ctx}, {"pair_ctx", pair_ctx}})) return rc;
  if (int rc = check_denoiser_aligned("sample_loop", "w", d, w)) return rc;
  DIFFAB_REQUIRE(t_start <= s->T && t_stop >= 0 && t_stop <= t_start, DIFFAB_ERR_ARG, "sample_loop: need T >= t_start >= t_stop >= 0");
  // design modes: the modality a KEEP bit names is never written by the update kernel (the only writer of the state in the loop); the
  // bits mean nothing to the denoiser, which sees the state as it is
  const uint32_t keep = flags & (DIFFAB_FLAG_KEEP_STRUCTURE | DIFFAB_FLAG_KEEP_SEQUENCE);
  DIFFAB_REQUIRE(keep != (DIFFAB_FLAG_KEEP_STRUCTURE | DIFFAB_FLAG_KEEP_SEQUENCE), DIFFAB_ERR_ARG,
                 "sample_loop: DIFFAB_FLAG_KEEP_STRUCTURE and DIFFAB_FLAG_KEEP_SEQUENCE together leave nothing to sample");
  flags &= ~keep;
  // sequence constraints: one word of allowed classes per (state row, residue), read by the update kernel's draw of s_{t-1} alone
  const uint32_t* allowed = opt->allowed;
  DIFFAB_REQUIRE(!(allowed && (keep & DIFFAB_FLAG_KEEP_SEQUENCE)), DIFFAB_ERR_ARG,
                 "sample_loop: allowed classes constrain a sequence that DIFFAB_FLAG_KEEP_SEQUENCE does not sample");
  DIFFAB_REQUIRE(!allowed || d->V <= 32, DIFFAB_ERR_ARG, "sample_loop: allowed classes are one 32-bit word per residue; V = %d > 32", d->V);
  const diffab_sample_record* rec = opt->record;
  const diffab_sample_steps* steps = opt->steps;
  const diffab_sample_steering* steering = opt->steering;
  UpdateOptions uo;
  uo.keep = keep;
  uo.allowed = allowed;
  std::vector<int32_t> plan_host;  // the step plan as the device reads it (empty without steps)
  if (int rc = record_option(rec, s, t_start, t_stop, &uo.rec)) return rc;
  if (int rc = steps_option(steps, rec, s, t_start, t_stop, &plan_host, &uo.plan)) return rc;
  if (int rc = guidance_option(opt->guidance, s, keep, &uo.guide)) return rc;
  if (int rc = temperature_option(opt->temperature, keep, &uo.temp)) return rc;
  if (int rc = steering_option(steering, d, s, keep, t_stop, steps != nullptr ? plan_host.data() : nullptr, &uo.steer)) return rc;
  const int32_t* ctx_of_row = opt->ctx_of_row;
  const bool mapped = ctx_of_row != nullptr;
  int n_ctx = opt->n_ctx;
  bool identity = false;
  if (int rc = context_map_option(d, ctx_of_row, &n_ctx, &identity)) return rc;
  const SampleBuffers sb = carve_sample(d, workspace, n_ctx, mapped);
  DIFFAB_REQUIRE(workspace_bytes >= sb.bytes, DIFFAB_ERR_WORKSPACE, "sample_loop: workspace %zu < %zu bytes", workspace_bytes, sb.bytes);
  hipStream_t st = as_stream(stream);
  const int* ctx_dev = nullptr;  // device map of the kernels (nullptr: the identity)
  if (!identity) {
    // once per call: the map, and the residue context of every state row (64 KiB per row at K = 128 - the per-row MLPs read it as
    // before; only the pair stream is read through the map)
    DIFFAB_HIP_CHECK(hipMemcpyAsync(sb.ctx_of_row, ctx_of_row, sizeof(int32_t) * d->B, hipMemcpyHostToDevice, st));
    if (int rc = launch_gather_rows(res_ctx, sb.ctx_of_row, d->B, static_cast<int64_t>(d->K) * d->D, sb.res_ctx, st)) return rc;
    ctx_dev = sb.ctx_of_row;
    res_ctx = sb.res_ctx;
  }
  const StepBuffers b0 = carve_step(d, sb.step, n_ctx);
  const ForwardPlan plan = plan_forward(d, flags, b0, res_ctx, pair_ctx, nullptr, true, ctx_dev, n_ctx, sb.tiles, sb.row_plan,
                                        sb.start_class);
  // The heads' folded beta columns depend on (step, head, column) only - every patch of a reverse step has the same beta - so the table
  // of ALL steps is built once per call instead of once per step.  Eager loop only: under graph replay the step index lives in device
  // memory and the chain's bias pointer is a launch argument.
  StepBias bias{sb.beta, plan.fold ? s->beta : nullptr, 0, nullptr, nullptr, s->T + 1};
  if (plan.chain && s->T + 1 <= kTrajRows && !(flags & DIFFAB_FLAG_GRAPH_SAMPLER)) bias.beta_traj = sb.beta_traj;
  if (int rc = prepare_forward(d, w, plan, b0, pair_ctx, bias, st)) return rc;
  if (plan.last_layer_tiles)
    if (int rc = launch_tiles_needed(gen_mask, d->B, d->K, sb.tiles, st)) return rc;
  if (plan.last_layer_rows)
    if (int rc = launch_row_plan(gen_mask, d->B, d->K, sb.row_plan, st)) return rc;
  if (plan.start_class)
    if (int rc = launch_start_classes(sb.row_plan, d->B, d->K, module_stagger_classes(), sb.start_class, st)) return rc;
  if (rec != nullptr) {  // the step -> slot table, and the residues the loop never writes, once per call
    DIFFAB_HIP_CHECK(hipMemcpyAsync(rec->slot_dev, rec->slot_of_step, sizeof(int32_t) * (s->T + 1), hipMemcpyHostToDevice, st));
    if (int rc = launch_record_fixed(uo.rec, seq, x, O, gen_mask, d->B, d->K, d->V, st)) return rc;
  }
  if (steps != nullptr)  // the step plan, once per call
    DIFFAB_HIP_CHECK(hipMemcpyAsync(steps->plan_dev, plan_host.data(), sizeof(int32_t) * plan_host.size(), hipMemcpyHostToDevice, st));
  if (steering != nullptr && steering->ancestors != nullptr)  // the ancestor record: -1 wherever no steering step writes
    DIFFAB_HIP_CHECK(hipMemsetAsync(steering->ancestors, 0xFF, sizeof(int32_t) * static_cast<size_t>(s->T + 1) * d->B, st));
  auto one_step = [&](int t, const int* t_dev) -> int {
    if (!plan.fold)  // (the folded head tables read the schedule themselves: one launch less per step)
      if (int rc = launch_fill_beta(s, t, d->B, sb.beta, st, t_dev)) return rc;
    StepBias step = bias;
    step.t = t;
    step.t_dev = t_dev;
    if (int rc = denoise_step(d, w, plan, step, seq, x, O, res_ctx, pair_ctx, sb.eps, nullptr, nullptr, nullptr, b0, st)) return rc;
    // (the heads' epilogue - O0 = O_t exp(hat(v)), the posterior's softmax - runs inside the update kernel, for the generated rows)
    return launch_reverse_update_philox(s, rev_tab, t, seq, x, O, sb.eps, sb.O0, sb.post, gen_mask, seed, first_patch, d->B, d->K, d->V, st,
                                        t_dev, b0.vbuf, b0.logits, uo);
  };
  // DIFFAB_FLAG_GRAPH_SAMPLER: a step is ~45 launches; at B = 1 (BASELINE config 1) their host cost (3-4 us each) is several times
  // the kernels' own time.  The first step runs eagerly (it also performs the one-time function-attribute calls), the second is
  // captured into a hipGraph that takes its timestep from device memory, and the graph is replayed for every remaining step: one host
  // call per step instead of 45.  Same kernels, same order, same arguments: bitwise the same trajectory (tested).
  // (a step list: the eager loop runs over it, and graph replay advances the device timestep through the plan's next[] table)
  const int n_steps = steps != nullptr ? steps->n_steps : t_start - t_stop;
  const bool graph = (flags & DIFFAB_FLAG_GRAPH_SAMPLER) && n_steps >= 3 && !kernel_timer_enabled();
  if (!graph) {
    if (steps != nullptr) {
      for (int j = 0; j < n_steps; ++j)
        if (int rc = one_step(steps->steps[j], nullptr)) return rc;
      return DIFFAB_OK;
    }
    for (int t = t_start; t > t_stop; --t)
      if (int rc = one_step(t, nullptr)) return rc;
    return DIFFAB_OK;
  }
  const int t_second = steps != nullptr ? steps->steps[1] : t_start - 1;
  if (int rc = one_step(t_start, nullptr)) return rc;
  if (int rc = launch_set_int(sb.t_dev, t_second, st)) return rc;
  // Capture and replay run on a private stream (the caller's may be the legacy default stream, which cannot be captured), ordered
  // behind the caller's stream by an event; the private stream is drained before the call returns, so later work on the caller's
  // stream sees the finished trajectory, and the executable graph outlives its launches (the only synchronisation in this library;
  // the eager path stays fully asynchronous).
  hipStream_t side = nullptr;
  hipEvent_t ev = nullptr;
  hipGraph_t g = nullptr;
  hipGraphExec_t ge = nullptr;
  DIFFAB_HIP_CHECK(hipStreamCreateWithFlags(&side, hipStreamNonBlocking));
  hipError_t ei = hipEventCreateWithFlags(&ev, hipEventDisableTiming);
  if (ei == hipSuccess) ei = hipEventRecord(ev, st);
  if (ei == hipSuccess) ei = hipStreamWaitEvent(side, ev, 0);
  int rc = DIFFAB_OK;
  if (ei == hipSuccess) {
    hipStream_t caller = st;
    st = side;  // one_step enqueues on `st`
    ei = hipStreamBeginCapture(side, hipStreamCaptureModeThreadLocal);
    if (ei == hipSuccess) {
      rc = one_step(t_second, sb.t_dev);
      if (rc == DIFFAB_OK) rc = steps != nullptr ? launch_advance_step(sb.t_dev, uo.plan.next, side) : launch_dec_int(sb.t_dev, side);
      ei = hipStreamEndCapture(side, &g);
    }
    st = caller;
  }
  if (ei == hipSuccess && rc == DIFFAB_OK) ei = hipGraphInstantiate(&ge, g, nullptr, nullptr, 0);
  if (ei == hipSuccess && rc == DIFFAB_OK)
    for (int j = 1; j < n_steps && ei == hipSuccess; ++j) ei = hipGraphLaunch(ge, side);
  if (ei == hipSuccess) ei = hipStreamSynchronize(side);
  if (ge) (void)hipGraphExecDestroy(ge);
  if (g) (void)hipGraphDestroy(g);
  if (ev) (void)hipEventDestroy(ev);
  (void)hipStreamDestroy(side);
  if (rc != DIFFAB_OK) return rc;
  if (ei != hipSuccess) {
    set_error("sample_loop: graph capture / replay failed: %s", hipGetErrorString(ei));
    return DIFFAB_ERR_HIP;
  }
  return DIFFAB_OK;
}

size_t diffab_score_workspace_bytes(const diffab_dims* d, int32_t n_ctx) {
  if (check_dims(d, "score_workspace_bytes")) return 0;
  if (n_ctx < 1 || static_cast<int64_t>(n_ctx) * d->K >= (1ll << 31)) {
    set_error("score_workspace_bytes: need 1 <= n_ctx and n_ctx*K < 2^31 (n_ctx=%d)", n_ctx);
    return 0;
  }
  return carve_score(d, nullptr, n_ctx).bytes;
}

int diffab_score_designs(const diffab_dims* d, const diffab_denoiser_weights* w, const diffab_sched* s, const diffab_igso3* fwd_tab,
                         const int64_t* seq, const float* x, const float* O, const uint8_t* gen_mask, const uint8_t* res_mask,
                         int32_t n_designs, const float* res_ctx, const float* pair_ctx, int32_t n_ctx, const int32_t* ctx_of_design,
                         const int32_t* t_list, int32_t n_t, int32_t n_draws, uint64_t seed, int64_t first_design, float* out_terms,
                         float* out_residue, const diffab_score_noised* noised, void* workspace, size_t workspace_bytes, uint32_t flags,
                         void* stream) {
  StreamOrder order_(stream);
  // every check on the host, before anything is enqueued
  if (int rc = check_dims(d, "score_designs")) return rc;
  if (int rc = check_denoiser_weights(d, w)) return rc;
  DIFFAB_REQUIRE(d->V == 21, DIFFAB_ERR_ARG, "score_designs: the sequence diffusion has 21 classes (V = %d)", d->V);
  DIFFAB_REQUIRE(s && s->T > 0 && s->T < kTrajRows && s->alpha_bar && s->alpha_bar_sqrt && s->one_minus_alpha_bar_sqrt && s->beta,
                 DIFFAB_ERR_ARG, "score_designs: bad schedule (need 1 <= T < %d)", kTrajRows);
  DIFFAB_REQUIRE(fwd_tab && fwd_tab->sigmas && fwd_tab->cdf && fwd_tab->n_bins > 0 && fwd_tab->n_sigmas >= s->T + 1, DIFFAB_ERR_ARG,
                 "score_designs: forward IGSO3 table must have T+1 rows");
  DIFFAB_REQUIRE(seq && x && O && gen_mask && res_ctx && pair_ctx && t_list && out_terms && workspace, DIFFAB_ERR_ARG,
                 "score_designs: null pointer (seq, x, O, gen_mask, res_ctx, pair_ctx, t_list, out_terms and workspace are required)");
  if (int rc = require_aligned16("score_designs", {{"res_ctx", res_ctx}, {"pair_ctx", pair_ctx}})) return rc;
  if (int rc = check_denoiser_aligned("score_designs", "w", d, w)) return rc;
  DIFFAB_REQUIRE(n_designs >= 1, DIFFAB_ERR_ARG, "score_designs: n_designs = %d < 1", n_designs);
  DIFFAB_REQUIRE(first_design >= 0 && first_design + n_designs <= (1ll << 32), DIFFAB_ERR_ARG,
                 "score_designs: first_design + n_designs must lie in [0, 2^32] (Philox patch ids)");
  DIFFAB_REQUIRE(n_t >= 1 && n_t <= s->T, DIFFAB_ERR_ARG, "score_designs: n_t = %d outside [1, T = %d]", n_t, s->T);
  for (int j = 0; j < n_t; ++j) {
    DIFFAB_REQUIRE(t_list[j] >= 1 && t_list[j] <= s->T, DIFFAB_ERR_ARG, "score_designs: t_list[%d] = %d outside [1, T = %d]", j, t_list[j], s->T);
    for (int i = 0; i < j; ++i)
      DIFFAB_REQUIRE(t_list[i] != t_list[j], DIFFAB_ERR_ARG, "score_designs: t_list[%d] = t_list[%d] = %d (duplicate step)", i, j, t_list[j]);
  }
  DIFFAB_REQUIRE(n_draws >= 1 && n_draws <= 65536, DIFFAB_ERR_ARG, "score_designs: n_draws = %d outside [1, 65536]", n_draws);
  DIFFAB_REQUIRE(n_ctx >= 1 && static_cast<int64_t>(n_ctx) * d->K < (1ll << 31), DIFFAB_ERR_ARG, "score_designs: need 1 <= n_ctx, n_ctx*K < 2^31");
  DIFFAB_REQUIRE(ctx_of_design != nullptr || n_ctx == n_designs, DIFFAB_ERR_ARG,
                 "score_designs: without ctx_of_design n_ctx must equal n_designs (%d != %d)", n_ctx, n_designs);
  for (int r = 0; ctx_of_design != nullptr && r < n_designs; ++r)
    DIFFAB_REQUIRE(ctx_of_design[r] >= 0 && ctx_of_design[r] < n_ctx, DIFFAB_ERR_ARG, "score_designs: ctx_of_design[%d] = %d outside [0, %d)", r,
                   ctx_of_design[r], n_ctx);
  const uint32_t keep = flags & (DIFFAB_FLAG_KEEP_STRUCTURE | DIFFAB_FLAG_KEEP_SEQUENCE);
  DIFFAB_REQUIRE(keep != (DIFFAB_FLAG_KEEP_STRUCTURE | DIFFAB_FLAG_KEEP_SEQUENCE), DIFFAB_ERR_ARG,
                 "score_designs: DIFFAB_FLAG_KEEP_STRUCTURE and DIFFAB_FLAG_KEEP_SEQUENCE together leave nothing to score");
  const ScoreBuffers sb = carve_score(d, workspace, n_ctx);
  DIFFAB_REQUIRE(workspace_bytes >= sb.bytes, DIFFAB_ERR_WORKSPACE, "score_designs: workspace %zu < %zu bytes", workspace_bytes, sb.bytes);
  // (the reverse loop's graph replay and skipped row tiles have no meaning here; the design-mode bits steer the noising and the terms)
  flags &= ~(keep | DIFFAB_FLAG_GRAPH_SAMPLER | DIFFAB_FLAG_SKIP_UNUSED_ROWS | DIFFAB_FLAG_ALL_ROWS);
  hipStream_t st = as_stream(stream);
  DIFFAB_HIP_CHECK(hipMemcpyAsync(sb.t_list, t_list, sizeof(int32_t) * n_t, hipMemcpyHostToDevice, st));
  const StepBuffers b0 = carve_step(d, sb.step, n_ctx);
  const ForwardPlan plan = plan_forward(d, flags, b0, sb.res_ctx, pair_ctx, nullptr, true, sb.ctx_of_row, n_ctx);
  const StepBias bias{sb.beta};  // per-row beta: the heads' folded beta columns come from the per-chunk table
  if (int rc = prepare_forward(d, w, plan, b0, pair_ctx, bias, st)) return rc;
  const diffab_score_noised out = noised ? *noised : diffab_score_noised{nullptr, nullptr, nullptr, nullptr};
  const int64_t total = static_cast<int64_t>(n_designs) * n_t * n_draws;
  for (int64_t q0 = 0; q0 < total; q0 += d->B) {
    const ScoreChunk c{sb.t_list, n_t, n_draws, d->K, q0, d->B, static_cast<int>(total - q0 < d->B ? total - q0 : d->B), keep};
    if (int rc = launch_score_noise(s, fwd_tab, c, seq, x, O, gen_mask, ctx_of_design, seed, first_design, sb.seq_t, sb.x_t, sb.O_t, sb.eps,
                                    sb.beta, sb.ctx_of_row, out, st))
      return rc;
    if (int rc = launch_gather_rows(res_ctx, sb.ctx_of_row, d->B, static_cast<int64_t>(d->K) * d->D, sb.res_ctx, st)) return rc;
    if (int rc = denoise_step(d, w, plan, bias, sb.seq_t, sb.x_t, sb.O_t, sb.res_ctx, pair_ctx, sb.eps_hat, nullptr, nullptr, nullptr, b0, st))
      return rc;
    if (int rc = launch_score_losses(s, c, seq, O, gen_mask, res_mask, sb.seq_t, sb.O_t, sb.eps, sb.eps_hat, b0.vbuf, b0.logits, out_terms,
                                     out_residue, st))
      return rc;
  }
  return DIFFAB_OK;
}

}  // extern "C"
