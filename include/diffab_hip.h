/*
 * diffab_hip.h - C ABI of libdiffab_hip.so: the MI355X (gfx950) engine under the
 * DiffAb diffusion / denoise hot path.
 *
 * The reference (dohlee/diffab-pytorch) is pure Python on stock ATen ops and has
 * no FFI of its own; its boundary for this path is the
 * Python class surface of diffab_pytorch.DiffAb.  This header is the C ABI a
 * maintainer binds underneath that surface (ctypes stub: INTEGRATION.md).  Each
 * entry point cites the reference code it replaces, file:line relative to the
 * reference repository root.
 *
 * Conventions (all entry points):
 *   - plain device pointers and sizes; no torch / HIP types in signatures
 *     (`stream` is a hipStream_t passed as void*, NULL = default stream);
 *   - row-major, contiguous, float32 unless stated; residue/aa indices and
 *     timesteps are int64 (torch.LongTensor), masks are 1 byte per element
 *     (torch.bool);
 *   - the caller owns every buffer including the workspace (size from the
 *     matching *_workspace_bytes query); kernels are enqueued on `stream` and
 *     never synchronise on the host; no hidden global state beyond the opt-in stream guard below; the
 *     library never reads the environment.  Two DIAGNOSTIC entry points keep
 *     process-global state and are off by default: diffab_kernel_timer_enable/read
 *     (an event list) and diffab_debug_set_attn_stamps / diffab_debug_set_module_stamps / _stagger (stamp-buffer pointers, two ints);
 *     they are not thread-safe and must not be left enabled in production.
 *     DIFFAB_FLAG_GRAPH_SAMPLER makes diffab_sample_loop drain a private stream
 *     before it returns.  (Kernel variants that were measured and not adopted, the environment
 *     switches used to A/B them and the timing-ablation hooks are patches under experiments/.)
 *   - Streams: calls on ONE stream are ordered by the stream, as usual; calls on DIFFERENT streams are independent and may overlap on
 *     the device (no state of the library is shared between two calls).  History: rounds 3-5 saw a small elementwise kernel compute wrong
 *     values in lanes 48-63 while kernels of a second library pipeline ran on another stream, and serialised the library's calls across
 *     streams by default.  Round 6 found the cause (profiles/r06_lanes_48_63.md; reproducer tools/hwtests/pkmul_two_streams.hip): gfx950
 *     returns a wrong low result in lanes 48-63 for v_pk_{mul,add,fma}_f32 ... op_sel:[0,1] while f16 / bf16 MFMAs of ANY wave on the
 *     SIMD - another kernel's included - are in flight, and hipcc's SLP vectoriser had formed that instruction in 14 VALU-only kernels.
 *     No kernel of the library contains the form any more (enforced at build time and by tests/test_isa_lint.py), two pipelines on two
 *     streams are bitwise the sequential runs, and the ordering guard is OFF by default.  diffab_set_stream_guard(1) switches it on:
 *     before a call enqueues on stream B, everything enqueued so far on the stream of the library's previous call (same device) is
 *     ordered in front of it (hipEventRecord + hipStreamWaitEvent; no host synchronisation; one mutex per device).  With the guard on,
 *     a stream handed to the library must stay alive until the library's next call on that device has been made, and library calls must
 *     not be captured into a hipGraph from a stream other than the last one used.  NOTE for callers: the hardware behaviour applies to
 *     YOUR kernels too - a caller's own VALU kernel holding that packed form can miscompute beside this library's f16 / bf16 MFMA
 *     kernels on another stream (tools/isa_hazard_lint.py checks any gfx950 object file or shared library).
 *     What is tested (tests/test_gpu_stream_contract.py, every export of every header in the table of
 *     tests/test_stream_contract_host.py): behind other work on a side stream, every launch, memset and copy of an entry is on `stream`
 *     or on an internal stream ordered after and before it by events; the call returns without waiting for the stream; and an array
 *     in host memory (ctx_of_row, slot_of_step, steps, beta_jump, alpha_jump, ctx_of_design, t_list, bin_edges, motifs, point_radius,
 *     complex_of_row) may be overwritten or freed the moment the call has returned.  Outside that: the queries, setters and host-only
 *     diagnostics enqueue nothing; diffab_kernel_timer_read waits for its events by design; a call with DIFFAB_FLAG_GRAPH_SAMPLER
 *     drains its private stream, so it is held to its values only; diffab_debug_start_classes (diffab_hip_debug.h) is not driven.
 *   - Workspaces and tapes: what a workspace or a tape holds ON ENTRY is ignored - it may be zeros, NaN bit patterns or the leftover of a
 *     call at another shape, mask or flag selection, and the result is the same to the bit (for the gradients below: to their stated
 *     accuracy).  What a workspace holds ON EXIT is unspecified.  Nothing outside [p, p + bytes) of the stated *_workspace_bytes /
 *     *_tape_bytes is written.  A tape is fully defined by its forward call: the backward reads nothing of it that the forward of the
 *     same dims and flags did not write.  Every element of an OUTPUT tensor is written, unless its entry says otherwise (the record of
 *     diffab_sample_record is written in every slot; the steering ancestors table is filled with -1 by the call, then written in the
 *     rows of the steered steps; row 0 of the chain embedding's gradient - padding_idx = 0 - stays the caller's zero).  Buffers the
 *     library ACCUMULATES into (float atomics, order-dependent in the last bits) are the only ones the caller must zero-fill first:
 *     every buffer of a `grads` / `g` weight struct (diffab_train_step_bwd, diffab_denoise_step_bwd, diffab_ipa_layer_bwd,
 *     diffab_residue_embedding_bwd, diffab_pair_embedding_bwd / _bwd_taped), d_pair_ctx of the two denoiser backwards and d_e of
 *     diffab_ipa_layer_bwd (each NULL to skip); and the steering state logw / u_prev, 0 at the start of a run.  d_res_ctx, d_x_t,
 *     d_O_t, d x, d R, d t are written, not accumulated.  tests/test_gpu_scratch_contract.py holds every hot-path entry to this with
 *     zero, 0xFF and random fills behind guard bytes, and with the previous call's leftover.
 *   - Operand alignment.  A contiguous tensor can start anywhere: a parameter that is a view of one flat parameter vector behind a 3-wide
 *     bias, a batch slice x[1:3] at a ragged patch length (K = 173: +12 bytes).  DATA operands - state, contexts, masks, schedule and
 *     IGSO3 tables, option tables, weights, cotangents, gradient buffers, outputs - need their NATURAL alignment only (4 bytes float /
 *     int32 / uint32, 8 bytes int64 / double, 1 byte masks).  Workspaces, tapes and scratch keep the 16- or 256-byte rule stated at
 *     their entry (a *_workspace_bytes workspace and a tape: 256 bytes, as torch allocates; the debug GEMM scratch, the PairEmbedding
 *     tape: 16 bytes; the steering scratch: 8).  For every entry, every data operand that meets its natural alignment has exactly one of
 *     two outcomes:
 *       ACCEPTED - the result contract of the entry, as with 16-byte aligned operands (possibly on a slower kernel);
 *       REFUSED  - DIFFAB_ERR_ARG, diffab_last_error() = "<entry>: operand <name> must be 16-byte aligned ...", decided on the host among
 *                  the argument checks, before anything is enqueued: outputs, in-place state and accumulating gradient buffers are
 *                  untouched to the bit, and the next call on the same workspace is as correct as any.
 *     Nothing else happens: no kernel makes a vector access through a caller's pointer that the entry has not checked, and no refusal
 *     comes after the first launch.  Which is which:
 *       REFUSED unless 16-byte aligned - every FLOAT operand, and every buffer of a weights / grads table (`w`, `grads`, `g`), of the
 *         entries whose kernels read and write float4: diffab_ipa_layer_fwd, diffab_denoise_step_fwd, diffab_train_step_fwd / _bwd,
 *         diffab_denoise_step_fwd_taped / diffab_denoise_step_bwd, diffab_ipa_layer_fwd_taped / diffab_ipa_layer_bwd,
 *         diffab_residue_embedding_fwd / _bwd, diffab_pair_embedding_fwd / _xyz_fwd / _bwd / _fwd_taped / _bwd_taped (operand names as in
 *         the prototypes; a table's buffer is named w.res_w0, w.coord.b4, grads.layers[1].w_bias, g.mw0, ...); of
 *         diffab_sample_loop / _ex: x, O, res_ctx, pair_ctx and the weights; of diffab_score_designs: res_ctx, pair_ctx and the weights;
 *         of the diagnostics diffab_debug_linear128 (modes 1 and 2): X, W, bias, Y, and of diffab_debug_xstat128: X, W, Y.
 *         (The kernel launchers behind these entries keep alignment preconditions of their own - "rowgemm128: unsupported operands",
 *         "ipa_layer_fast: x and the projection weights must be 16-byte aligned", "gemm_nn: ... needs the aligned path" and the like.
 *         They are internal invariants: every pointer they look at is either an operand the entry has already refused unless aligned, or
 *         a buffer carved from a workspace or tape at offsets that keep 16 bytes.  No caller pointer reaches one of them misaligned, so
 *         none can fire behind a launch because of an operand's alignment; one that fires is a defect of the library.)
 *       ACCEPTED at natural alignment - everything else: the int64 and mask operands of the entries above; of diffab_sample_loop / _ex
 *         also seq, the schedule, the IGSO3 table and every table of the options struct; of diffab_score_designs also seq, x, O, the
 *         schedule, the table, out_terms, out_residue and the `noised` copies; and every operand of every other entry (SO(3) maps,
 *         IGSO3 tables and draws, the three forward diffusers, diffab_philox_fill, the losses, frames, the angular encoding,
 *         diffab_featurize_xyz, the reverse updates, the sampler's initialisers, guidance and steering, patch selection / gather /
 *         scatter, the metrics, the refinement, diffab_debug_linear128 mode 0, diffab_debug_gemm_tn, diffab_debug_row_tiles / _plan).
 *         Their kernels address caller memory element by element; three of them pick a vector form from the pointer itself
 *         (diffab_philox_fill's float4 store, diffab_featurize_xyz's float2 store of the pairwise dihedrals, the 16- / 4- / 1-byte lanes
 *         of diffab_patch_gather / _scatter) and write the same values either way.
 *     The Python front end never refuses: _hip.dev_f32 hands the library a 16-byte aligned copy of a misaligned tensor, and everything
 *     the library writes goes to tensors the front end allocates.  tests/test_gpu_operand_alignment.py pins this table.
 *   - Operand extents.  An operand's EXTENT is the shape its prototype comment gives, at the dims of the call (x_t: B K 3 floats; a
 *     table's buffer: its parameter's shape; out_terms: n_designs n_t n_draws 3), from the pointer, contiguous.  Behind it may lie a
 *     neighbour - the next gradient of a flat vector, the next rows of the batch an operand is a slice of, the rest of a larger result -
 *     so an entry writes NOTHING outside the extents of the operands it declares writable.  Writable are: the non-const pointer
 *     parameters; the non-const pointer fields of the option and record structs (diffab_sample_record, diffab_sample_steps.plan_dev,
 *     diffab_sample_guidance.shift_dev, the steering state and scratch, diffab_score_noised); every buffer of a `grads` / `g` table (the
 *     weights struct again, so its fields read const float*: accumulated into all the same); and the in-place state (seq, x, O of the
 *     samplers, the updates, the initialisers and diffab_steer_gather; logw / u_prev of diffab_steer_resample).  Every const operand is
 *     bit-for-bit unchanged on return: the inputs, the buffers of `w`, the schedule and IGSO3 tables, the option tables (allowed, chain,
 *     residue_idx, residue_mask, the temperature tables), a tape in its backward.  An entry may ISSUE a load past the end of an operand
 *     only where the address is clamped inside it (a ragged last tile reads its last valid row again); no result depends on memory
 *     outside an operand, whatever it holds.  Two operands may alias only where an entry says so (diffab_reverse_update_jump:
 *     posterior / r_out).  tests/test_gpu_operand_extents.py holds every entry with a data operand to this: its own reference test
 *     again with every operand between two 64 KiB guards, under two guard fills (NaN / 0, and 1), the guards and the const operands
 *     compared to the byte afterwards; tests/sampler_support.py WRITES is the table of writable operands, checked against this header
 *     and include/diffab_hip_analysis.h by tests/test_operand_extents_host.py.
 *   - empty problems (a count or extent of 0) return 0 before any pointer is looked at: an empty tensor's data pointer is NULL;
 *   - return 0 on success, a negative DIFFAB_ERR_* otherwise (never throws);
 *     diffab_last_error() gives the thread's last message.
 */
#ifndef DIFFAB_HIP_H
#define DIFFAB_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DIFFAB_OK 0
#define DIFFAB_ERR_ARG (-1)         /* null pointer / non-positive size / inconsistent dims */
#define DIFFAB_ERR_UNSUPPORTED (-2) /* dims outside what the kernels cover */
#define DIFFAB_ERR_HIP (-3)         /* a HIP runtime call failed */
#define DIFFAB_ERR_WORKSPACE (-4)   /* workspace too small */

/* flags */
#define DIFFAB_FLAG_FORCE_GENERIC 1u /* skip the MFMA kernels specialised for D=128,C=64,H=8,DS=32,P=8 */
/* (bits 2u, 4u, 8u selected attention variants that were measured slower than the fused kernel and are no longer part of this
   library: experiments/README.md; the three-launch attention survives as the form the training tape keeps) */

#define DIFFAB_FLAG_PAIR_PLANES 32u /* K = 64 / 128, default attention kernel: the pair embedding is first rewritten as two fp16 planes (e s =
                                      h1 + h2 to 2^-23 of the tensor maximum, same bytes, in the workspace) and the two products on
                                      the pair tile run on the f16 matrix cores as three exact partial products each, fp32
                                      accumulation.  diffab_sample_loop always does this (once per trajectory); for single calls
                                      the flag adds the rewrite (2x the pair embedding in HBM traffic) to every call. */

#define DIFFAB_FLAG_PAIR_F32 64u /* diffab_sample_loop: keep the fp32 pair stream (do not build the fp16 planes); for single calls simply
                                    do not pass DIFFAB_FLAG_PAIR_PLANES.  The plain-fp32 reference form of the attention kernel. */
#define DIFFAB_FLAG_FP32_GEMM 128u /* forward paths: the dense products (projections, to_out, MLPs) on the f32-input MFMA kernels instead
                                      of the split-precision products (projections, to_out: three-term fp16 under power-of-two
                                      scales; MLPs: six-term bf16); same results to fp32 rounding (the plain-fp32 reference form) */

#define DIFFAB_FLAG_GRAPH_SAMPLER 16u /* diffab_sample_loop: capture one reverse step into a hipGraph (timestep read from device memory)
                                         and replay it for the remaining steps - one host call per step instead of ~45.  Bitwise the
                                         eager trajectory.  The call drains its private replay stream before it returns (the graph
                                         must outlive its launches).  Measured at B = 1, K = 128: no gain (the host already runs
                                         ahead of the device; a step is 45 dependent small-grid kernels), hence opt-in. */
#define DIFFAB_FLAG_PERSISTENT_MODULE 512u /* MFMA path with pair planes, K = 128 or 256 (diffab_sample_loop, or a single call with
                                         DIFFAB_FLAG_PAIR_PLANES): the NL layers of the IPA module (reference diffab_pytorch.py:494-498)
                                         run as ONE patch-resident launch - a 512-thread work-group owns a patch through projections,
                                         eight attention row tiles and to_out, layer after layer, with no inter-CU synchronisation
                                         (patches never exchange data) - instead of 3 NL chip-wide launches.  Same tile bodies:
                                         bitwise the multi-launch result.  Where the MLP chains apply (D == 128, V <= 128, no
                                         out_res_emb) the launch also runs the embedding MLP of the patch's rows in front of layer 0
                                         and the three heads behind the last layer: one launch per denoiser forward.  Ignored where
                                         it does not apply.  diffab_sample_loop
                                         chooses it by itself at K = 128 when the batch fills the chip (B >= number of CUs), see
                                         DIFFAB_FLAG_MULTI_LAUNCH.  K = 256
                                         (two dense tiles, sixteen two-chunk attention items per patch; round 6) only on request:
                                         it measures 4 % slower than its per-layer launches at B = 512. */
#define DIFFAB_FLAG_MULTI_LAUNCH 1024u /* diffab_sample_loop: keep one launch per kernel of an IPA layer even where the patch-resident module
                                          launch would be chosen (B >= number of CUs, K = 128); the two forms are bitwise equal */
#define DIFFAB_FLAG_ALL_ROWS 8192u /* diffab_sample_loop / _ex: a step's outputs are read for GENERATED residues only (the reverse
                                     update, its heads epilogue, guidance and the trajectory record leave the others alone), so on the
                                     MFMA path with K % 16 == 0 and NL >= 2 the loop runs the LAST layer's attention only for the 16-row
                                     tiles that contain one (every other layer feeds all rows' keys and values to the next) - on the
                                     module launch and on the per-layer launches alike, bitwise the same trajectory.  The work skipped
                                     depends on the mask: with one CDR-like segment per patch 5-7 of the 8 row tiles of the last layer;
                                     a fully generated patch skips nothing.  This bit keeps every tile: the all-rows time of a step.
                                     The single forwards, the taped entries and diffab_score_designs always run every row. */
#define DIFFAB_FLAG_SKIP_UNUSED_ROWS 256u /* accepted, no effect: what it asked for is what diffab_sample_loop does unless
                                             DIFFAB_FLAG_ALL_ROWS is set */
/* Design modes of the reverse loop (diffab_sample_loop / _ex, diffab_sample_init_ex, diffab_sample_init_noised).  With one of these
   bits set the sampler never writes that modality of the state; the other is updated exactly as without the bit, from the same Philox
   draws.  The branch is uniform per launch, on every launch form of the loop.  Both bits together: DIFFAB_ERR_ARG, nothing enqueued. */
#define DIFFAB_FLAG_KEEP_STRUCTURE 2048u /* fixed-backbone sequence design: x and O of the generated residues stay as given (the
                                            heads' O0 epilogue is skipped); only seq is diffused */
#define DIFFAB_FLAG_KEEP_SEQUENCE 4096u /* structure prediction: seq of the generated residues stays as given; only x and O are diffused */

/* Model and batch geometry.  Reference ctor: diffab_pytorch.py:629-647. */
typedef struct {
  int32_t B;  /* patches in this call */
  int32_t K;  /* residues per patch */
  int32_t D;  /* d_residue_emb */
  int32_t C;  /* d_pair_emb */
  int32_t H;  /* n_head */
  int32_t DS; /* d_scalar_per_head */
  int32_t PQ; /* n_query_point_per_head */
  int32_t PV; /* n_value_point_per_head */
  int32_t NL; /* n_ipa_layers */
  int32_t V;  /* aa vocabulary (21; reference diffusion.py:47) */
} diffab_dims;

/* One InvariantPointAttentionLayer's parameters in nn.Linear layout (out x in),
 * i.e. pointers straight into the reference's state_dict tensors
 * (diffab_pytorch.py:354-379; keys: SURVEY Appendix B.3). */
typedef struct {
  const float* gamma;  /* (H)                     raw, no softplus (:373) */
  const float* wq_s;   /* (H*DS, D)  to_q_scalar.weight */
  const float* wk_s;   /* (H*DS, D)  to_k_scalar.weight */
  const float* wv_s;   /* (H*DS, D)  to_v_scalar.weight */
  const float* w_bias; /* (H, C)     to_pair_bias.weight */
  const float* wq_p;   /* (H*PQ*3, D) to_q_point.weight */
  const float* wk_p;   /* (H*PQ*3, D) to_k_point.weight */
  const float* wv_p;   /* (H*PV*3, D) to_v_point.weight */
  const float* w_out;  /* (D, H*DS + H*C + H*PV*3 + H*PV) to_out.weight */
  const float* b_out;  /* (D) to_out.bias */
} diffab_ipa_layer_weights;

/* Linear-ReLU-Linear-ReLU-Linear head (diffab_pytorch.py:533-556). */
typedef struct {
  const float *w0, *b0; /* (D, D+3), (D) */
  const float *w2, *b2; /* (D, D), (D) */
  const float *w4, *b4; /* (n_out, D), (n_out) */
} diffab_mlp3_weights;

/* Denoiser parameters (diffab_pytorch.py:501-556). `layers` is a HOST array of NL. */
typedef struct {
  const float* seq_emb;           /* (25, D) sequence_embedding.weight (:514) */
  const float *res_w0, *res_b0;   /* (D, 2D), (D)  to_res_emb.0 */
  const float *res_w2, *res_b2;   /* (D, D), (D)   to_res_emb.2 */
  const diffab_ipa_layer_weights* layers;
  diffab_mlp3_weights coord;      /* coordinate_denoising  -> 3 */
  diffab_mlp3_weights orient;     /* orientation_denoising -> 3 */
  diffab_mlp3_weights seq;        /* sequence_denoising    -> V (softmax applied by the kernel) */
} diffab_denoiser_weights;

/* Variance schedule on the device: five (T+1) float arrays
 * (diffusion.py:11-35; keys alpha, alpha_bar, alpha_bar_sqrt,
 * one_minus_alpha_bar_sqrt, beta). */
typedef struct {
  int32_t T;
  const float* alpha;
  const float* alpha_bar;
  const float* alpha_bar_sqrt;
  const float* one_minus_alpha_bar_sqrt;
  const float* beta;
} diffab_sched;

/* IGSO3 tables on the device (so3.py:9-72): one row per sigma. */
typedef struct {
  int32_t n_sigmas;
  int32_t n_bins;
  const float* sigmas;   /* (n_sigmas) */
  const float* cdf;      /* (n_sigmas, n_bins) normalised inclusive prefix sums of the pdf rows */
  float sigma_threshold; /* histogram branch iff sigma < threshold (so3.py:122-125) */
} diffab_igso3;

const char* diffab_version(void);
const char* diffab_last_error(void);
/* 1 if a gfx950 device is visible to this process, else 0 (no error). */
int diffab_device_ok(void);

/* Opt-in diagnostics for bench.py's roofline leg: while enabled, every launch of the dominant kernel (the IPA
 * attention kernel) is bracketed by a hipEvent pair recorded on its launch stream.  read() waits for the events,
 * returns the number of launches and their summed duration, and resets the counter.  Not thread-safe; off by default. */
int diffab_kernel_timer_enable(int on);
/* Diagnostics only: while a device buffer of (work-groups x 8 waves x 8) uint64 is registered, the fused attention kernel
 * writes s_memtime stamps at its phase boundaries into it (tools/attn_phase_profile.py).  NULL (default) disables it. */
int diffab_debug_set_attn_stamps(void* device_buffer);
/* Diagnostics of the patch-resident module kernel (DIFFAB_FLAG_PERSISTENT_MODULE): its start-up stagger (work-groups of class
 * (index / 8) % classes start class x ticks late, ticks of 10 ns; default 8 x 1000: eight classes 10 us apart),
 * and a stamp buffer of (B NL 8 tiles x 8 waves x 8) + (B NL 4) + (2 B) uint64 filled with 100 MHz s_memrealtime stamps (NULL: off; of
 * the last 2 B the first B: the end of each patch's heads, the second B: the start of each patch, in front of the embedding MLP).  The
 * kernel writes ALL of it: a buffer sized for an earlier library (which ended with one B) is B uint64 too short for this one. */
int diffab_debug_set_attn_variant(int32_t v); /* Reference paths for tests and tools (process-global): bit 2 (4) = the PairEmbedding
                                                 forward / backward as their unfused launches where the fused kernel would apply, bit 6
                                                 (64) = the PairEmbedding backward's matrix-core kernels (csrc/pair_chain_bwd.hip: 64-wide
                                                 chain, one-hot table / coefficient sums) as the separate launches they replaced.  0 =
                                                 defaults.  Any other bit: DIFFAB_ERR_ARG, the switch is left as it was. */
int diffab_debug_set_module_stagger(int32_t ticks_10ns, int32_t classes);
int diffab_debug_set_module_stamps(void* device_buffer);
/* Tests: the row-tile map diffab_sample_loop builds per call - tiles[b][j] (B x K / 16 bytes, device) = 1 when one of the residues
 * 16 j .. 16 j + 15 of patch b is generated, else 0; the last layer's attention runs for the tiles with a 1 (DIFFAB_FLAG_ALL_ROWS). */
int diffab_debug_row_tiles(const uint8_t* gen_mask, int32_t B, int32_t K, uint8_t* tiles, void* stream);
/* Tests: the row plan diffab_sample_loop builds per call for the module launch - plan[b] (B x (2 + K / 16) int32, device) =
 * {n_items, slab bits, start rows}: the last layer's attention runs n_items 16-row items, item j on rows start[j] .. start[j] + 15
 * (start = min(first generated row not yet covered, K - 16); entries behind n_items are -1); bit s of the slab word is set when one of
 * the residues 32 s .. 32 s + 31 is generated ((K + 31) / 32 slabs: K = 16 is one slab).  K a multiple of 16 in 16 .. 1024. */
int diffab_debug_row_plan(const uint8_t* gen_mask, int32_t B, int32_t K, int32_t* plan, void* stream);
/* The cross-stream ordering guard described under "Streams" above: on / off (default since round 6), process-wide. */
int diffab_set_stream_guard(int on);
/* Diagnostics / accuracy tests: Y[M x 128] = X[M x Kd] W[128 x Kd]^T + bias through ONE of the two dense kernels of the MFMA path -
 * mode 0: f32-input MFMA (rowgemm128_kernel), mode 1: bf16 matrix cores, six-term split (rowgemm128_b6_kernel; scratch >=
 * 3 * 128 * Kd * 2 bytes, 16-byte aligned operands), mode 2: f16 matrix cores, three-term split under power-of-two scales
 * (rowgemm128_h3_kernel; scratch >= 2 * 128 * Kd * 2 + 768 bytes; Kd a multiple of 64).  Modes 0 and 1: Kd a multiple of 32.  Lets a test measure them against float64. */
int diffab_debug_linear128(const float* X, const float* W, const float* bias, float* Y, int64_t M, int32_t Kd, int32_t mode, void* scratch,
                           size_t scratch_bytes, void* stream);
/* Diagnostics / accuracy tests: Y[M x N] = X[M x 128] W[128 x N] (row-major, 16-byte aligned X) through one of the two x-stationary kernels
 * the training backward uses for d feat = d y W_out (reference: autograd of diffab_pytorch.py:459-464) - mode 1: bf16 matrix cores, six-term
 * split (proj_frames_b6_kernel without frames), mode 2: f16 matrix cores, three-term split under power-of-two scales (xstat_h3_kernel).
 * Any N >= 1, any M >= 1; scratch: 16-byte aligned, >= 3 * 2 * ceil(N / 96) * 96 * 128 * 2 + ceil(N / 96) * 96 * 4 bytes. */
int diffab_debug_xstat128(const float* X, const float* W, float* Y, int64_t M, int32_t N, int32_t mode, void* scratch, size_t scratch_bytes,
                          void* stream);
/* Diagnostics / accuracy tests: C[N1 x N2] += A[M x N1]^T B[M x N2] (row-major, contraction over the rows) through one of the two
 * weight-gradient kernels of the training backward (reference: autograd of every nn.Linear, e.g. diffab_pytorch.py:375-379, :459-464) -
 * mode 1: bf16 matrix cores, six-term split (gemm_tn_b6_kernel), mode 2: f16 matrix cores, three-term split with one power-of-two
 * scale per (32-row slab, operand) (gemm_tn_h3_kernel).  db (nullable): db[N1] += column sums of A.  Any M, N1, N2 >= 1. */
int diffab_debug_gemm_tn(const float* A, const float* B, float* C, float* db, int64_t M, int32_t N1, int32_t N2, int32_t mode, void* stream);
/* Tests: the launch forms the dense tiles of the MFMA path pick at a row count rows = B K (the launchers call the same host functions,
 * csrc/denoiser_internal.h).  Host only, enqueues nothing, out5 is a HOST array of 5: out5[0] = rows per work-group of the row GEMM
 * (to_out, the MLP layers, diffab_debug_linear128 modes 1 and 2) - 0: the (row tile, k part) form, taken with has_parts (the launcher
 * was given parts scratch and the contraction has more than one part) up to 64 tiles of 64 rows; else 128 when ceil(rows / 128) >= 256,
 * else 64; out5[1] = 1 if the last group of that form is ragged; out5[2] = FULL (rows a multiple of 128: the projection and
 * x-stationary tiles, also the fp32 projection tile, run without row guards); out5[3] = nsplit of the x-stationary / projection tile
 * with nblocks column blocks = clamp(256 / ceil(rows / 128), 1, nblocks) (work-groups per row tile; SPLIT = nsplit > 1); out5[4] = rows
 * of its last tile (1 .. 128; also of the last group of the MLP chains). */
int diffab_debug_dense_forms(int64_t rows, int32_t nblocks, int32_t has_parts, int32_t* out5);
int diffab_kernel_timer_read(int64_t* launches, double* total_ms);
/* ---- SO(3) maps, n matrices/vectors each --------------------------------- */
/* so3.py:146-162  log R = theta/(2 sin theta) (R - R^T), theta in [0, pi], defined at every angle (unlike the reference: DESIGN.md,
 * "SO(3) maps at theta near 0 and pi"): log I = 0; at theta = pi exactly the axis whose largest component is positive */
int diffab_so3_log(const float* R, float* S, int64_t n, void* stream);
/* so3.py:219-237  exp of a skew-symmetric matrix (Rodrigues); exp(0) = I (NaN in the reference) */
int diffab_so3_exp(const float* S, float* R, int64_t n, void* stream);
/* so3.py:173-182 */
int diffab_so3_matrix_to_rotvec(const float* R, float* v, int64_t n, void* stream);
/* so3.py:207-216 */
int diffab_so3_rotvec_to_matrix(const float* v, float* R, int64_t n, void* stream);
/* so3.py:240-259  exp(k log R); k has n/per_k entries, k[i / per_k] scales matrix i */
int diffab_so3_scale_rot(const float* R, const float* k, float* out, int64_t n, int64_t per_k, void* stream);

/* ---- IGSO3 ---------------------------------------------------------------- */
/* so3.py:52-72  pdf[n_sigmas][n_bins] at the bin centres, series of num_iters terms, NaN->0, <0 -> 0.  The reference's table:
 * every term formed with the reference's own fp32 roundings (its rounding noise, rectified by the clamp, is part of the
 * distribution it samples from); the terms are added in fp32 in the order of torch's CPU cascade sum for this reduction (ATen
 * SumKernel multi_row_sum: four levels), csrc/diffusion_kernels.hip igso3_pdf_kernel<true>. */
int diffab_igso3_table_build(const float* sigmas, int32_t n_sigmas, int32_t n_bins, int32_t num_iters, float* pdf, void* stream);
/* opt-in variant: the whole series in float64, rounded once - the exact density, NOT what the reference samples from */
int diffab_igso3_table_build_accurate(const float* sigmas, int32_t n_sigmas, int32_t n_bins, int32_t num_iters, float* pdf,
                                      void* stream);
/* build-defined: cdf rows = normalised inclusive prefix sums (float64 accumulate) of the pdf rows */
int diffab_igso3_cdf_build(const float* pdf, int32_t n_sigmas, int32_t n_bins, float* cdf, void* stream);
/* so3.py:98-126  rot-vectors (B,K,3) = normalize(axis_raw) * theta, theta from the histogram row
 * sigma_idx[b] (inverse CDF on u_bin, uniform in the bin by u_in) if sigma < threshold, else
 * (2 sigma + sigma z) mod pi.  axis_raw (B,K,3), u_bin/u_in/z (B,K). */
int diffab_igso3_sample(const diffab_igso3* tab, const int64_t* sigma_idx, int32_t B, int32_t K, const float* axis_raw,
                        const float* u_bin, const float* u_in, const float* z, float* rotvec, void* stream);

/* so3.py:78  `torch.multinomial(probs, num_samples)` draws the K bins of a patch WITHOUT replacement.  bins (B,K) int32 = the K
 * bins of histogram row sigma_idx[b] with the largest pdf[bin] / race[b][bin], largest first, ties by lower bin: with race (B, n_bins)
 * ~ Exp(1) this is a draw without replacement in draw order (the exponential race torch itself uses on a GPU).  n_bins <= 16384.
 * sigmas (n_sigmas, nullable) + sigma_threshold: rows with sigma >= threshold use the Gaussian angle and never read their bins
 * (so3.py:122-125) - they are skipped (bins 0) instead of sorted; NULL sorts every row.  Cost of a sorted row: one 1024-thread
 * work-group, a bitonic network over the 8192 keys in LDS. */
int diffab_igso3_bins_without_replacement(const float* pdf, int32_t n_sigmas, int32_t n_bins, const int64_t* sigma_idx, int32_t B,
                                          int32_t K, const float* race, int32_t* bins, const float* sigmas, float sigma_threshold,
                                          void* stream);
/* diffab_igso3_sample with the histogram bins given (bins (B,K) from diffab_igso3_bins_without_replacement) instead of u_bin */
int diffab_igso3_sample_bins(const diffab_igso3* tab, const int64_t* sigma_idx, int32_t B, int32_t K, const float* axis_raw,
                             const int32_t* bins, const float* u_in, const float* z, float* rotvec, void* stream);

/* ---- forward (noising) process, explicit noise ----------------------------- */
/* diffusion.py:38-41  out[b, ...] = w1[b] p1[b, ...] + w2[b] p2[b, ...]; n elements in all, per_b of them per patch */
int diffab_weighted_multinomial(const float* p1, const float* p2, const float* w1, const float* w2, int64_t n, int64_t per_b,
                                float* out, void* stream);
/* diffusion.py:49-79 (mode 0: q(s_t|s_{t-1}), beta_t), :105-135 (mode 1: q(s_t|s_0), alpha_bar_t) */
int diffab_seq_forward_prob(const diffab_sched* s, int mode, const int64_t* seq, const int64_t* t, const uint8_t* mask,
                            int32_t B, int32_t K, float* prob /* (B,K,21) */, void* stream);
/* diffusion.py:168-192 */
int diffab_seq_posterior(const diffab_sched* s, const int64_t* seq_t, const int64_t* seq_0, const int64_t* t,
                         const uint8_t* mask, int32_t B, int32_t K, float* post /* (B,K,21) */, void* stream);
/* diffusion.py:156-158 (torch.multinomial replaced by inverse CDF on the given uniforms) */
int diffab_categorical_sample(const float* prob, const float* u, int64_t n_rows, int32_t V, int64_t* out, void* stream);
/* diffusion.py:199-236 */
int diffab_coord_forward(const diffab_sched* s, const float* x0, const int64_t* t, const uint8_t* mask, const float* eps,
                         int32_t B, int32_t K, float* xt, void* stream);
/* diffusion.py:262-294 */
int diffab_orient_forward(const diffab_sched* s, const float* O0, const uint8_t* mask, const int64_t* t,
                          const float* rotvec, int32_t B, int32_t K, float* Ot, void* stream);

/* ---- counter-based noise (Philox4x32-10) ------------------------------------ */
/* out[(b*K + k)*4 + c], c = 0..3: normals (kind 0) or uniforms in (0,1) (kind 1) for
 * counter (residue k, patch first_patch + b, step, stream_id), key = seed. */
int diffab_philox_fill(uint64_t seed, int64_t first_patch, int32_t B, int32_t K, int32_t step, int32_t stream_id, int kind,
                       float* out, void* stream);

/* ---- IPA / denoiser --------------------------------------------------------- */
size_t diffab_denoise_workspace_bytes(const diffab_dims* d);
size_t diffab_sample_workspace_bytes(const diffab_dims* d); /* for diffab_sample_loop */
/* for diffab_sample_loop_ex with a context map (diffab_sample_options.ctx_of_row): the fp16 pair planes and their row scales are
 * sized by n_ctx, not d->B, plus the device copy of the map and a (B,K,D) residue-context buffer.  0 (and diffab_last_error) for bad dims or n_ctx < 1. */
size_t diffab_sample_shared_workspace_bytes(const diffab_dims* d, int32_t n_ctx);
/* diffab_pytorch.py:389-465  one InvariantPointAttentionLayer.forward */
int diffab_ipa_layer_fwd(const diffab_dims* d, const diffab_ipa_layer_weights* w, const float* x /* (B,K,D) */,
                         const float* e /* (B,K,K,C) */, const float* R /* (B,K,3,3) */, const float* t /* (B,K,3) */,
                         float* y /* (B,K,D) */, void* workspace, size_t workspace_bytes, uint32_t flags, void* stream);
/* diffab_pytorch.py:558-607  Denoiser.forward == DiffAb.denoise (:726-768).
 * out_logits (B,K,V) pre-softmax and out_res_emb (B,K,D) post-IPA are optional (NULL to skip). */
int diffab_denoise_step_fwd(const diffab_dims* d, const diffab_denoiser_weights* w, const int64_t* seq_t, const float* x_t,
                            const float* O_t, const float* res_ctx, const float* pair_ctx, const float* beta /* (B) */,
                            float* out_eps, float* out_O0, float* out_posterior, float* out_logits, float* out_res_emb,
                            void* workspace, size_t workspace_bytes, uint32_t flags, void* stream);

/* ---- losses (diffab_pytorch.py:610-625, 856-880) ----------------------------- */
/* losses[3] = (seq KL, translation MSE, orientation) each summed over masked residues / #masked residues.
 * One work-group, fixed-order tree reduction: bitwise reproducible. */
int diffab_losses_fwd(const float* pred_post, const float* true_post, const float* pred_eps, const float* true_eps,
                      const float* pred_O0, const float* true_O0, const uint8_t* gen_mask, const uint8_t* res_mask,
                      int32_t B, int32_t K, int32_t V, float* losses3, void* stream);

/* ---- training step of the hot path (diffab_pytorch.py:808-880 minus encode_context; BASELINE config 4) -------------------
 * fwd: Denoiser.forward with every intermediate saved in `tape` (size: diffab_train_tape_bytes) + the three masked losses.
 * bwd: gradients of  upstream3 . (seq KL, translation MSE, orientation loss)  w.r.t. every denoiser parameter, the residue
 *      context and (optionally) the pair context.  `grads` is the weights struct again, pointing at ZERO-INITIALISED buffers
 *      of the parameters' shapes; they, and d_pair_ctx (NULL to skip, else zero-initialised (B,K,K,C)), are accumulated into
 *      (float atomics: sums over residues are order-dependent in the last bits).  d_res_ctx (B,K,D) may be NULL.
 *      upstream3 is a DEVICE pointer to 3 floats (autograd's incoming gradient; no host sync). */
size_t diffab_train_tape_bytes(const diffab_dims* d);
size_t diffab_train_workspace_bytes(const diffab_dims* d);
int diffab_train_step_fwd(const diffab_dims* d, const diffab_denoiser_weights* w, const int64_t* seq_t, const float* x_t,
                          const float* O_t, const float* res_ctx, const float* pair_ctx, const float* beta, const float* true_post,
                          const float* true_eps, const float* true_O0, const uint8_t* gen_mask, const uint8_t* res_mask,
                          float* out_eps, float* out_O0, float* out_posterior, float* losses3, void* tape, size_t tape_bytes,
                          uint32_t flags, void* stream);
int diffab_train_step_bwd(const diffab_dims* d, const diffab_denoiser_weights* w, const diffab_denoiser_weights* grads,
                          const int64_t* seq_t, const float* x_t, const float* O_t, const float* pair_ctx, const float* out_eps,
                          const float* out_O0, const float* out_posterior, const float* true_post, const float* true_eps,
                          const float* true_O0, const uint8_t* gen_mask, const uint8_t* res_mask, const float* upstream3,
                          float* d_res_ctx, float* d_pair_ctx, const void* tape, size_t tape_bytes, void* workspace,
                          size_t workspace_bytes, void* stream);

/* diffab_pytorch.py:610-625  OrientationLoss: elems (n,3,3) = (pred^T target - I)^2 and/or their total (either may be NULL) */
int diffab_orientation_loss(const float* pred, const float* target, int64_t n, float* elems, float* sum1, void* stream);
/* its backward (autograd of :620-625): cotangent per element (g_elems, (n,3,3)) or one device scalar applied to every element
 * (g_total: upstream / (9 n) for reduction "mean", upstream for "sum"); d_pred / d_target (n,3,3), either may be NULL */
int diffab_orientation_loss_bwd(const float* pred, const float* target, int64_t n, const float* g_elems, const float* g_total,
                                float* d_pred, float* d_target, void* stream);

/* diffab_pytorch.py:315-324 euclidean_transform: out = x R + t, and :327-336 inverse_euclidean_transform: out = (x - t) R^T, for
 * points x (B, N heads, L, P, 3), frames R (B, L, 3, 3), t (B, L, 3) broadcast over the heads (row-vector convention).  t may be
 * NULL (rotation only: the x-gradient of the opposite direction). */
int diffab_frames_apply(const float* x, const float* R, const float* t, float* out, int32_t B, int32_t N, int32_t L, int32_t P, void* stream);
int diffab_frames_invert(const float* x, const float* R, const float* t, float* out, int32_t B, int32_t N, int32_t L, int32_t P, void* stream);
/* d R (B, L, 3, 3) and d t (B, L, 3) of the same two maps from the cotangent g_out of their output (each nullable; written, not accumulated):
 * invert = 0: euclidean_transform, 1: inverse_euclidean_transform.  The x-gradient is the other map with t = NULL. */
int diffab_frames_bwd(const float* x, const float* R, const float* t, const float* g_out, int32_t invert, float* dR, float* dt, int32_t B,
                      int32_t N, int32_t L, int32_t P, void* stream);
/* diffab_pytorch.py:20-54 AngularEncoding.forward: n input values -> n x (4 num_funcs + 1) outputs [x, sin(f x), cos(f x)],
 * f = [1 .. num_funcs, 1/1 .. 1/num_funcs] */
int diffab_angular_encoding(const float* x, int64_t n, int32_t num_funcs, float* out, void* stream);
/* its backward (the reference module is plain differentiable torch code): enc = the forward's output, g_out its cotangent, both
 * n x (4 num_funcs + 1); dx[n] = g[0] + sum_k f_k (cos(f_k x) g_sin[k] - sin(f_k x) g_cos[k]) */
int diffab_angular_encoding_bwd(const float* enc, const float* g_out, int64_t n, int32_t num_funcs, float* dx, void* stream);

/* ---- Denoiser.forward / InvariantPointAttentionLayer.forward under autograd (reference :558-607, :389-465 are differentiable) ----
 * Taped forwards (same outputs as diffab_denoise_step_fwd / diffab_ipa_layer_fwd, activations kept in `tape`) and backwards from
 * ARBITRARY cotangents.  Gradient buffers in `grads` and d_pair_ctx / d_e must be zero-filled by the caller (they are accumulated
 * into); NULL cotangents mean zero.  Tape: diffab_train_tape_bytes(d) / diffab_ipa_layer_tape_bytes(d); workspace:
 * diffab_train_workspace_bytes(d) / diffab_ipa_layer_bwd_workspace_bytes(d).  d_x_t (B,K,3) / d_O_t (B,K,3,3) and d_R / d_t: the
 * gradients with respect to the frames (reference: euclidean_transform / inverse_euclidean_transform :315-336 and O_t @ exp(v) :594-596
 * are differentiable in them), WRITTEN by the call, each nullable (the training step never needs them).  They are the gradients of
 * the formulas with R^T = R^-1, i.e. for rotation frames, as on the whole path.  DIFFAB_FLAG_FORCE_GENERIC is ignored by the taped
 * forwards (their backward reads the tape the MFMA path writes). */
int diffab_denoise_step_fwd_taped(const diffab_dims* d, const diffab_denoiser_weights* w, const int64_t* seq_t, const float* x_t,
                                  const float* O_t, const float* res_ctx, const float* pair_ctx, const float* beta, float* out_eps,
                                  float* out_O0, float* out_posterior, void* tape, size_t tape_bytes, uint32_t flags, void* stream);
int diffab_denoise_step_bwd(const diffab_dims* d, const diffab_denoiser_weights* w, const diffab_denoiser_weights* grads,
                            const int64_t* seq_t, const float* x_t, const float* O_t, const float* pair_ctx, const float* out_posterior,
                            const float* d_eps, const float* d_O0, const float* d_posterior, float* d_res_ctx, float* d_pair_ctx,
                            float* d_x_t, float* d_O_t, const void* tape, size_t tape_bytes, void* workspace, size_t workspace_bytes,
                            void* stream);
size_t diffab_ipa_layer_tape_bytes(const diffab_dims* d);
size_t diffab_ipa_layer_bwd_workspace_bytes(const diffab_dims* d);
int diffab_ipa_layer_fwd_taped(const diffab_dims* d, const diffab_ipa_layer_weights* w, const float* x, const float* e, const float* R,
                               const float* t, float* y, void* tape, size_t tape_bytes, uint32_t flags, void* stream);
int diffab_ipa_layer_bwd(const diffab_dims* d, const diffab_ipa_layer_weights* w, const diffab_ipa_layer_weights* grads, const float* e,
                         const float* R, const float* t, const float* dy, float* dx, float* d_e, float* d_R, float* d_t, const void* tape,
                         size_t tape_bytes, void* workspace, size_t workspace_bytes, void* stream);

/* ---- encode_context (reference diffab_pytorch.py:57-312, 680-724) -----------------------------------------
 * Runs once per sample.  atom_mask is float32 (B,K,A) (1 = atom present); context masks are 1 byte per residue, NULL = "not
 * given" (the reference passes None when generate_structure / generate_sequence is False). */
typedef struct {
  int32_t B, K;
  int32_t A;        /* atoms per residue (n_atoms, 15) */
  int32_t D;        /* d_residue_emb */
  int32_t C;        /* d_pair_emb */
  int32_t max_dist; /* max_dist_to_consider (32) */
} diffab_ctx_dims;

typedef struct { /* ResidueEmbedding parameters (:57-79), nn.Linear layout */
  const float *aa_emb, *chain_emb;        /* (21, D), (10, D) */
  const float *w0, *b0, *w2, *b2, *w4, *b4, *w6, *b6; /* mlp: (2D, 2D+21*A*3+39) (D,2D) (D,D) (D,D) */
} diffab_residue_emb_weights;

typedef struct { /* PairEmbedding parameters (:186-218) */
  const float *aa_pair_emb, *relpos_emb, *pair2distcoef; /* (441, C), (2*max_dist+1, C), (441, A*A) */
  const float *dw0, *db0, *dw2, *db2;                    /* distance_embedding: (C, A*A), (C, C) */
  const float *mw0, *mb0, *mw2, *mb2, *mw4, *mb4;        /* mlp: (C, 3C+18), (C, C), (C, C) */
} diffab_pair_emb_weights;

size_t diffab_residue_embedding_workspace_bytes(const diffab_ctx_dims* d);
/* ResidueEmbedding.forward (:81-183) -> out (B,K,D) */
int diffab_residue_embedding_fwd(const diffab_ctx_dims* d, const diffab_residue_emb_weights* w, const int64_t* seq_idx,
                                 const float* xyz /* (B,K,A,3) */, const float* orientations, const float* dihedrals /* (B,K,3) */,
                                 const int64_t* chain_idx, const float* atom_mask, const uint8_t* structure_context_mask,
                                 const uint8_t* sequence_context_mask, float* out, void* workspace, size_t workspace_bytes,
                                 void* stream);
size_t diffab_pair_embedding_workspace_bytes(const diffab_ctx_dims* d);
/* PairEmbedding.forward (:220-312) -> out (B,K,K,C).  residue_idx is (B,K) with batch stride K, or (1,K) with batch stride 0.
 * The structure-context mask has no effect on this module's output in the reference (:292-301) and is not a parameter. */
int diffab_pair_embedding_fwd(const diffab_ctx_dims* d, const diffab_pair_emb_weights* w, const int64_t* seq_idx,
                              const float* distmat /* (B,K,K,A,A) */, const float* pairwise_dihedrals /* (B,K,K,2) */,
                              const int64_t* residue_idx, int32_t residue_idx_batch_stride, const int64_t* chain_idx,
                              const float* atom_mask, const uint8_t* sequence_context_mask, float* out, void* workspace,
                              size_t workspace_bytes, void* stream);
/* Same, with the atom-atom distances taken from the coordinates xyz (B,K,A,3) inside the kernel instead of a materialised
 * distmat (K*K*A*A*4 = 14.7 MB per K=128 patch).  The reference's data layer computes that tensor with protstruc
 * (data.py:76, preprocess_pdb.py:61) and then leaves it out of its batches; d = |xyz[b,i,a] - xyz[b,j,a']|. */
int diffab_pair_embedding_xyz_fwd(const diffab_ctx_dims* d, const diffab_pair_emb_weights* w, const int64_t* seq_idx,
                                  const float* xyz /* (B,K,A,3) */, const float* pairwise_dihedrals /* (B,K,K,2) */,
                                  const int64_t* residue_idx, int32_t residue_idx_batch_stride, const int64_t* chain_idx,
                                  const float* atom_mask, const uint8_t* sequence_context_mask, float* out, void* workspace,
                                  size_t workspace_bytes, void* stream);

/* Featurisation from coordinates (what the reference's data layer computes with protstruc: data.py:75-82, preprocess_pdb.py:60-65):
 * backbone orientations (B,K,3,3) (rows = the residue's local axes: x along CA->C, y in the N-CA-C plane towards N; `global = local @ R
 * + t`), backbone dihedrals (B,K,3) = (phi, psi, omega) with their validity mask (B,K,3), and pairwise dihedrals (B,K,K,2):
 * phi_ij = (C_i, N_j, CA_j, C_j), psi_ij = (N_i, CA_i, C_i, N_j), IUPAC sign.  Any output may be NULL; chain_idx / residue_mask
 * may be NULL (one chain, every residue present).  xyz is (B,K,A,3) with atoms N, CA, C in slots 0, 1, 2.
 * protstruc is not part of the reference tree: these are the geometric definitions, parity with protstruc is unpinned. */
int diffab_featurize_xyz(const float* xyz, const int64_t* chain_idx, const uint8_t* residue_mask, int32_t B, int32_t K, int32_t A,
                         float* orientations, float* backbone_dihedrals, uint8_t* backbone_dihedrals_mask,
                         float* pairwise_dihedrals, void* stream);

/* Patch construction from a whole complex (what the reference's data layer does with protstruc before a batch exists:
 * preprocess_pdb.py:44-58 - the nearest-k residues around the CDR anchor residues, united with the nearest-k antigen residues, then
 * residue_masked_select).  protstruc is not part of the reference tree: the selection below is this library's own definition, and parity
 * with protstruc's get_cdr_anchor_mask / get_topk_nearest_residue_mask is UNPINNED (as for diffab_featurize_xyz).
 *
 * diffab_patch_select: B complexes padded to N residues each (N <= DIFFAB_PATCH_MAX_RESIDUES).  ca: the CA of residue (b, i) is the three
 * floats at ca[(b * N + i) * ca_stride] (ca_stride = 3 for a packed (B,N,3) array; A * 3 with ca pointing at atom slot 1 of an (B,N,A,3)
 * array).  residue_mask (B,N) (NULL: all present), generation_mask (B,N), anchor_mask (B,N) or NULL, chain_idx (B,N) or NULL (one chain),
 * antigen_mask (B,N) or NULL.  Outputs: index (B,K) int64, patch_mask (B,K), count (B) int32.  Per complex:
 *   1. Anchors.  With anchor_mask NULL, residue i is an anchor when it is present, not generated, and residue i-1 or i+1 is present,
 *      generated and has the same chain_idx (the residues flanking each generated segment); with an anchor_mask, when it is present and
 *      marked.  "Generated" always means present and marked in generation_mask.  A complex with a generated residue and no anchor uses
 *      the generated residues themselves as anchors.  A complex with no generated residue: count = 0.
 *   2. Key.  key_i = min over anchors a of ((x_i-x_a)^2 + (y_i-y_a)^2) + (z_i-z_a)^2, in fp32, in exactly this association and without
 *      contraction (the translation unit is built with -ffp-contract=off), so the value is a defined fp32 number.  Generated residues
 *      and anchors get key -1: they are always in the patch.
 *   3. Order.  Residues are ranked by (key, index) ascending: ties go to the lower index.  S1 = the first k present residues; S2 = the
 *      first k_antigen present residues with antigen_mask; the patch is the union of S1 and S2.
 *   4. Output.  index[b, :count] = the patch in ascending residue index (chain order is kept), index[b, count:] = -1, patch_mask true on
 *      the first count slots.  count <= k + k_antigen.
 * Refused before anything is enqueued: K < k + k_antigen, k < 1, k_antigen < 0, k_antigen > 0 with a NULL antigen_mask (DIFFAB_ERR_ARG);
 * N > DIFFAB_PATCH_MAX_RESIDUES (DIFFAB_ERR_UNSUPPORTED).  More generated-plus-anchor residues than k cannot be known on the host: that
 * complex gets count[b] = -1, an all-(-1) index row and an all-false patch_mask row.
 * One work-group per complex: the packed (key, index) words of the whole complex are sorted in LDS, hence the limit on N. */
#define DIFFAB_PATCH_MAX_RESIDUES 4096
int diffab_patch_select(const float* ca, int32_t ca_stride, const uint8_t* residue_mask, const uint8_t* generation_mask,
                        const uint8_t* anchor_mask, const int64_t* chain_idx, const uint8_t* antigen_mask, int32_t B, int32_t N, int32_t k,
                        int32_t k_antigen, int32_t K, int64_t* index, uint8_t* patch_mask, int32_t* count, void* stream);
/* diffab_patch_gather (preprocess_pdb.py:44-58, the residue_masked_select): dst (rows,K,row_bytes) = src (B,N,row_bytes) at index (rows,K);
 * slots whose index is outside [0, N) (the -1 padding) are zero-filled.  Row r reads complex complex_of_row[r], a HOST array of rows
 * entries in [0, B) (an entry outside: DIFFAB_ERR_ARG, nothing enqueued; it travels as launch arguments, so it may be freed on return);
 * NULL: row r reads complex r and rows must equal B.  row_bytes is any positive size - the bytes of one residue of the field, so one
 * entry serves every per-residue field (seq_idx 8, xyz A * 12, orientations 36, masks 1, ...); copies move 16, 4 or 1 bytes per lane,
 * whichever the size and the two addresses allow. */
int diffab_patch_gather(const void* src, const int64_t* index, const int32_t* complex_of_row, int32_t B, int32_t N, int32_t rows, int32_t K,
                        int64_t row_bytes, void* dst, void* stream);
/* diffab_patch_scatter, the inverse for results (the reference never pastes a patch back; preprocess_pdb.py:44-58 is the cut it undoes):
 * dst[r, index[r, p]] = patch[r, p] for patch (rows,K,row_bytes), index (rows,K), into dst (rows,N,row_bytes) that the caller has
 * pre-filled (with the native complex, one copy per design row).  Slots with an index outside [0, N) or a false write_mask (rows,K;
 * NULL: all true) write nothing.  An index row must not name a residue twice (diffab_patch_select's rows never do). */
int diffab_patch_scatter(const void* patch, const int64_t* index, const uint8_t* write_mask, int32_t rows, int32_t N, int32_t K,
                         int64_t row_bytes, void* dst, void* stream);

/* Design metrics: what a batch of designs looks like next to the native and next to each other.  The reference has
 * no evaluation code; these are the numbers DiffAb-style evaluations report (RMSD of the designed residues in the fixed framework, amino-acid
 * recovery) plus the Kabsch minimum and the all-pairs matrices of the designs of one patch.
 *
 * Common layout.  Designs are rows = G * N rows of K residues, row g * N + r = design r of group g (sample(num_samples = N)'s layout).
 * points (rows,K,P,3) fp32: P points per residue, 1 <= P <= DIFFAB_METRICS_MAX_POINTS (P = 1: the CA; P = 4: N, CA, C, O).  Per group:
 * generation_mask (G,K), residue_mask (G,K) or NULL (all present).  A residue COUNTS when it is generated and inside residue_mask; a row
 * with n counted residues has m = n * P counted points, taken in ascending residue order.  A mean over an empty selection is NaN.
 * Limits (DIFFAB_ERR_ARG, with the shape and null-pointer checks, before anything is enqueued): 1 <= N <= DIFFAB_METRICS_MAX_GROUP,
 * 1 <= K <= DIFFAB_METRICS_MAX_K, P as above.  rows = 0 / G = 0 succeeds without looking at a pointer.
 *
 * diffab_metrics_vs_native: per design row against its group's native_seq_idx (G,K) and native_points (G,K,P,3):
 *   aar          = (counted residues whose token equals the native's) / n, one fp32 division of the two integers;
 *   rmsd         = sqrt(sum |p - q|^2 / m), no superposition (the framework is fixed: the patch frame is the alignment);
 *   rmsd_aligned = sqrt(msd), msd = the minimum of the same over proper rotations and translations of the design: both sets centred,
 *                  H = sum p q^T, singular values s1 >= s2 >= s3, d = sign(det H) (+1 at 0),
 *                  msd = max(0, sum |p|^2 + sum |q|^2 - 2 (s1 + s2 + d s3)) / m.  One point gives 0; a mirror image does not align.
 * All sums, the centroids and the solve are fp64 (one wave per row: per-lane partial sums in ascending residue order, one fixed butterfly);
 * the singular values are the column norms of H after one-sided Jacobi (Hestenes) sweeps.  A row's numbers do not depend on the other
 * rows of the call.  segment_idx (G,K) int64 or NULL with S = 0: labels in [0, S), S <= DIFFAB_METRICS_MAX_SEGMENTS, anything else = no
 * segment; the same three numbers over the counted residues of each segment go to segment_* (rows,S). */
#define DIFFAB_METRICS_MAX_GROUP 4096
#define DIFFAB_METRICS_MAX_K 4096
#define DIFFAB_METRICS_MAX_POINTS 5
#define DIFFAB_METRICS_MAX_SEGMENTS 8
int diffab_metrics_vs_native(const int64_t* seq_idx, const float* points, const int64_t* native_seq_idx, const float* native_points,
                             const uint8_t* generation_mask, const uint8_t* residue_mask, const int64_t* segment_idx, int32_t rows,
                             int32_t group_size, int32_t K, int32_t P, int32_t S, float* aar, float* rmsd, float* rmsd_aligned,
                             float* segment_aar, float* segment_rmsd, float* segment_rmsd_aligned, void* stream);
/* diffab_metrics_pairwise: for every group the symmetric matrices rmsd (G,N,N) and seq_identity (G,N,N) over the group's counted residues.
 *   rmsd[g,i,j], aligned = 0: sqrt(acc / m) in fp32, acc = the fp32 sum over the counted points, in ascending order, of
 *                ((acc + dx*dx) + dy*dy) + dz*dz with dx = x_i - x_j one rounded subtraction of the inputs (no |a|^2 + |b|^2 - 2ab form,
 *                no contraction: the translation unit is built with -ffp-contract=off).
 *   rmsd[g,i,j], aligned = 1: rmsd_aligned of diffab_metrics_vs_native with design j as the native: centroids, H (through fma) and the
 *                spreads in fp64 from the fp32 inputs, the same fp64 solve, one rounding to fp32 at the end.
 *   seq_identity[g,i,j] = (counted residues with equal tokens) / n in fp32.  Tokens are compared by their low 8 bits.
 * The diagonal is defined, not computed: rmsd 0, identity 1 (NaN for an empty selection).  A pair is computed once (by j > i) and stored
 * twice, so entry (i,j) is bitwise entry (j,i).  The in-place number is NOT bitwise diffab_metrics_vs_native's rmsd (fp32 running sum
 * here, fp64 sums there); both are within 1e-4 relative of the exact value.
 * workspace: DIFFAB_METRICS_PAIRWISE_WORKSPACE_BYTES(G, N, K, P) bytes of device memory, 16-byte aligned (too small: DIFFAB_ERR_WORKSPACE):
 * the counted points and tokens of each group, compacted and with the designs along the fastest axis, and the fp64 centroids.
 * Two launches: the packing, then one work-group per 64 x 64 (aligned: 32 x 32) tile of pairs on or above the diagonal. */
#define DIFFAB_METRICS_PAIRWISE_WORKSPACE_BYTES(G, N, K, P) \
  ((size_t)(G) * (size_t)(N) * ((size_t)(K) * (size_t)(P) * 12 + ((size_t)(K) + 3) / 4 * 4 + 32) + (size_t)(G) * 4 + 1024)
int diffab_metrics_pairwise(const int64_t* seq_idx, const float* points, const uint8_t* generation_mask, const uint8_t* residue_mask,
                            int32_t G, int32_t N, int32_t K, int32_t P, int32_t aligned, float* rmsd, float* seq_identity, void* workspace,
                            size_t workspace_bytes, void* stream);
/* diffab_metrics_select_diverse: greedy farthest-point choice of m designs per group from dist (G,N,N) fp32 (either matrix above, or
 * 1 - identity).  candidates (G,N) or NULL (all); score (G,N) fp32 or NULL.
 *   first pick: the candidate with the lowest score (a NaN score counts as +inf; ties to the lower index); without score the first one;
 *   then:       among the candidates not picked, the one whose minimum over the picked p of dist[g,p,c] (row of the pick; a NaN distance
 *               counts as 0) is largest, ties to the lower index.
 * index (G,m) int64, min_dist (G,m) fp32 = that minimum at the moment of the pick (+inf for the first), count (G) int32 = picks made;
 * with fewer than m candidates the tail is -1 / NaN.  Loads, min, max and compares only: the result is a function of the fp32 matrix.
 * One work-group per group; N <= DIFFAB_METRICS_MAX_GROUP, m >= 0 (DIFFAB_ERR_ARG). */
int diffab_metrics_select_diverse(const float* dist, const float* score, const uint8_t* candidates, int32_t G, int32_t N, int32_t m,
                                  int64_t* index, float* min_dist, int32_t* count, void* stream);

/* Design filters: is a design a possible protein, and does it touch the antigen.  Rows, groups and masks as in
 * "Common layout" above (rows = G * group_size, masks (G,K), residue_mask NULL = all present).  Both entries also take the patch's
 * chain (G,K) int32 and residue_idx (G,K) int32.  Slots i and j of a patch are CHAIN NEIGHBOURS, j after i, when chain[i] == chain[j],
 * residue_idx[j] == residue_idx[i] + 1 and both are inside residue_mask (the bonded rule of diffab_sample_guidance; j need not be i + 1,
 * and a gap in residue_idx is a deleted residue: no bond).  Where several slots qualify, the successor (predecessor) of a slot is the
 * lowest one.  Limits, DIFFAB_ERR_ARG with the shape and null-pointer checks before anything is enqueued: rows >= 0 a multiple of
 * group_size, 1 <= group_size <= DIFFAB_METRICS_MAX_GROUP, 1 <= K <= DIFFAB_METRICS_MAX_K, finite distances >= 0, a workspace that is
 * NULL or not 16-byte aligned (too small: DIFFAB_ERR_WORKSPACE).  rows = 0 succeeds without looking at a pointer.  The entries see
 * points and validity bits only, never orientations or tokens.
 *
 * diffab_metrics_backbone: points (rows,K,3,3) fp32 = N, CA, C of every residue of every row.  With p / s the predecessor / successor of
 * slot i, per residue (rows,K) fp32, NaN where the neighbour does not exist (or i is outside residue_mask):
 *   phi   = dihedral(C_p, N_i, CA_i, C_i)      psi = dihedral(N_i, CA_i, C_i, N_s)      omega = dihedral(CA_i, C_i, N_s, CA_s)
 *   peptide_bond = |C_i - N_s| in Angstrom, stored at i.
 * dihedral(p0,p1,p2,p3) = atan2(|b2| b1.(b2 x b3), (b1 x b2).(b2 x b3)), b1 = p1 - p0, b2 = p2 - p1, b3 = p3 - p2: radians in (-pi, pi],
 * IUPAC sign (-pi is returned as pi).  Everything in fp64 from the fp32 points (differences, cross products, atan2, the root), rounded
 * once to fp32.  Per row (rows), over the bonds i -> s with generation_mask set on at least one end:
 *   n_bonds (int32); max_peptide_deviation = max |d - 1.329| (0 without a bond); n_chain_break = bonds with |d - 1.329| > bond_tolerance;
 *   n_cis = bonds with |omega| < pi/2 - the comparisons on the fp64 values, bond_tolerance widened to fp64.
 * One wave per row: integer sums and a maximum, so a row's numbers do not depend on the other rows.  Two launches (the neighbour table
 * of every patch, then the rows).  workspace: DIFFAB_METRICS_BACKBONE_WORKSPACE_BYTES(G, K) bytes. */
#define DIFFAB_METRICS_BACKBONE_WORKSPACE_BYTES(G, K) ((size_t)(G) * (size_t)(K) * 8 + 1024)
int diffab_metrics_backbone(const float* points, const uint8_t* generation_mask, const uint8_t* residue_mask, const int32_t* chain,
                            const int32_t* residue_idx, int32_t rows, int32_t group_size, int32_t K, float bond_tolerance, float* phi,
                            float* psi, float* omega, float* peptide_bond, int32_t* n_bonds, float* max_peptide_deviation,
                            int32_t* n_chain_break, int32_t* n_cis, void* workspace, size_t workspace_bytes, void* stream);
/* diffab_metrics_contacts: atom clashes of the generated residues and their contacts with the antigen.
 * Atoms.  A generated residue (generation_mask and residue_mask) of row r has the atoms points[r,k,a] (rows,K,P,3), 1 <= P <=
 * DIFFAB_METRICS_MAX_POINTS, whose bit a is set in valid[r,k] (rows,K) uint8.  A non-generated residue inside residue_mask has the atoms
 * context_points[g,k,a] (G,K,A,3), 1 <= A <= DIFFAB_METRICS_MAX_CONTEXT_ATOMS, whose bit a is set in context_valid[g,k] (G,K) uint32:
 * they belong to the patch and are shared by its designs.  Bits at or above P / A are ignored.
 * Eligible pairs: (atom a of generated residue i, atom b of residue j != i) with both residues inside residue_mask and j no chain
 * neighbour of i in either direction; when both residues are generated the unordered residue pair counts once.
 * d2 = (dx*dx + dy*dy) + dz*dz in fp32 with dx, dy, dz one rounded subtraction each, no contraction; every comparison is d2 against the
 * fp32 product clash_distance * clash_distance (contact_distance likewise).  Per row (rows):
 *   n_clash (int32) = eligible pairs with d2 < clash^2;  clash_score (fp32) = sum over them of (clash - d)^2, d = the fp32 root of d2,
 *   the terms and the sum in fp64 in a fixed order of the row, rounded once;  min_distance = the fp32 root of the smallest eligible d2,
 *   +inf without a pair.
 * With antigen_mask (G,K): generated residue i and a non-generated residue j inside antigen_mask are IN CONTACT when one of their
 * eligible atom pairs has d2 < contact^2.  n_contact_pairs = residue pairs in contact, n_paratope = generated residues with a contact,
 * n_epitope = antigen residues with one (each (rows) int32).  With hotspot_mask (G,K; needs antigen_mask): n_hotspot = non-generated
 * residues inside residue_mask, antigen_mask and hotspot_mask, n_hotspot_contacted = those of them with a contact.
 * Per residue (rows,K) int32: residue_clash = clashing atom pairs the residue takes part in (both ends count, context residues too),
 * residue_contact = its contact partners (both sides; only written with an antigen_mask).  Outputs that go with a NULL mask may be NULL.
 * Two launches and up to two memsets: the patch's valid context atoms are compacted once into the workspace; then one work-group per
 * (patch, 64 designs), lane = design, stages them through LDS in chunks of whole residues - at most
 * DIFFAB_METRICS_CONTACTS_CHUNK_RESIDUES residues and DIFFAB_METRICS_CONTACTS_CHUNK_ATOMS atoms, neither a limit on K * A - and keeps
 * every count on chip (registers, integer adds on LDS).  No float atomics.  A row's numbers do not depend on the other rows.
 * workspace: DIFFAB_METRICS_CONTACTS_WORKSPACE_BYTES(G, K, A) bytes. */
#define DIFFAB_METRICS_MAX_CONTEXT_ATOMS 32
#define DIFFAB_METRICS_CONTACTS_CHUNK_ATOMS 1024
#define DIFFAB_METRICS_CONTACTS_CHUNK_RESIDUES 64
#define DIFFAB_METRICS_CONTACTS_WORKSPACE_BYTES(G, K, A) \
  ((size_t)(G) * (size_t)(K) * ((size_t)(A) * 16 + 28) + (size_t)(G) * 16 + 2048)
int diffab_metrics_contacts(const float* points, const uint8_t* valid, const float* context_points, const uint32_t* context_valid,
                            const uint8_t* generation_mask, const uint8_t* residue_mask, const uint8_t* antigen_mask,
                            const uint8_t* hotspot_mask, const int32_t* chain, const int32_t* residue_idx, int32_t rows, int32_t group_size,
                            int32_t K, int32_t P, int32_t A, float clash_distance, float contact_distance, int32_t* n_clash,
                            float* clash_score, float* min_distance, int32_t* n_contact_pairs, int32_t* n_paratope, int32_t* n_epitope,
                            int32_t* n_hotspot_contacted, int32_t* n_hotspot, int32_t* residue_clash, int32_t* residue_contact,
                            void* workspace, size_t workspace_bytes, void* stream);

/* Design ensembles: the N designs of a patch as a distribution.  Rows, groups, points and masks as in "Common
 * layout" above (rows = G * N, row g * N + r = design r of group g, points (rows,K,P,3), masks (G,K)).
 * diffab_metrics_ensemble: weights (rows) fp32 or NULL (all 1): one weight w_r per design, the caller's contract like other per-row device
 * data (softmax of steering's log_weight, or a 0 / 1 mask of the designs that passed a filter); a negative or non-finite weight is 0, and a
 * design of weight 0 is not read for the sums over designs.  V classes, 1 <= V <= DIFFAB_METRICS_MAX_CLASSES; a = pseudocount, finite, >= 0.
 * A position (g,k) is INSIDE when residue_mask[g,k] holds (NULL: every position) and COUNTED when it is inside and generated.  Every sum
 * over designs, residues or atoms is taken in fp64 from the fp32 / int64 inputs; every float output is that fp64 rounded once to fp32.
 *
 * Per position, defined at inside positions (elsewhere the float outputs are NaN and consensus is -1):
 *   c_v = sum_r w_r [s_rk = v] for v in [0, V) - a token outside [0, V) is in no class - and W_k = sum_v c_v;
 *   aa_freq (G,K,V) fp32: f_v = (c_v + a / V) / (W_k + a); all V entries NaN where W_k + a = 0;
 *   entropy (G,K) fp32:   - sum_v f_v ln f_v in nats with 0 ln 0 = 0; NaN where f is NaN;
 *   consensus (G,K) int64: the smallest v with the largest c_v; -1 where W_k = 0;
 *   mean_points (G,K,P,3) fp32: m = sum_r w_r p_r / W with W = sum_r w_r over the group's designs; NaN where W = 0;
 *   rmsf (G,K) fp32: sqrt(sum_r w_r sum_a |p_rka - m_ka|^2 / (W P)) with m the fp64 mean before rounding and the sum taken in a second
 *                    pass over the designs (never sum p^2 - (sum p)^2, which cancels).
 * Per design (rows) fp32, over the n counted positions of the design's patch; NaN for a patch without a counted position:
 *   log_prob           = the mean of ln f_k(s_rk) with the fp64 f; a term is -inf where the token is outside [0, V) or f is 0, and NaN
 *                        where the token is a class and f is NaN;
 *   consensus_identity = (float)count / (float)n, count = counted positions with s_rk = consensus_k (a position without a consensus,
 *                        W_k = 0, matches no token);
 *   rmsd_to_mean       = sqrt(sum_k sum_a |p - m|^2 / (n P)); NaN where W = 0.
 * Per patch:
 *   n_eff (G) fp32:    W^2 / sum_r w_r^2; NaN where W = 0;
 *   central (G) int64: the design r in [0, N) with w_r > 0 whose fp32 rmsd_to_mean is smallest, ties to the lower r, a NaN never wins;
 *                      -1 if there is none.
 * Nothing is superposed before the average (the framework is fixed: the in-place number is the meaningful one, as for rmsd above).
 * residue_mask and weights may be NULL; any output pointer may be NULL (that output is not wanted; without rmsf, the three per-design
 * outputs and central the second pass is not run).  Limits, DIFFAB_ERR_ARG before anything is enqueued: N, K, P as in "Common layout",
 * V and a as above, null seq_idx / points / generation_mask, a workspace that is NULL or not 16-byte aligned (too small:
 * DIFFAB_ERR_WORKSPACE).  G = 0 succeeds without looking at a pointer.
 * Fixed reduction order, no atomics: N is cut into slices of 128 designs and K into chunks of 64 residues; a work-group of four waves
 * takes one (group, slice, chunk), lane = residue, wave w the designs w, w + 4, ... of the slice; the waves are added in wave order, the
 * slices in slice order, the chunks in chunk order, the lanes of a wave through one fixed butterfly.  A group's results depend on that
 * group alone.  Four launches: accumulate, finish, deviations, rows.
 * workspace: DIFFAB_METRICS_ENSEMBLE_WORKSPACE_BYTES(G, N, K, P, V) bytes: the slices' partial sums, ln f and the mean in fp64, and the
 * per-design partial sums of every chunk. */
#define DIFFAB_METRICS_MAX_CLASSES (32)
#define DIFFAB_METRICS_ENSEMBLE_WORKSPACE_BYTES(G, N, K, P, V)                                                                    \
  ((size_t)(G) * 8 * ((((size_t)(N) + 127) / 128) * (size_t)(K) * ((size_t)(V) + 3 * (size_t)(P) + 1) +                          \
                      (size_t)(K) * ((size_t)(V) + 3 * (size_t)(P)) + (size_t)(N) * (((size_t)(K) + 63) / 64) * 3 + 1) +          \
   (size_t)(G) * 4 * ((size_t)(K) + 1) + 4096)
int diffab_metrics_ensemble(const int64_t* seq_idx, const float* points, const uint8_t* generation_mask, const uint8_t* residue_mask,
                            const float* weights, int32_t G, int32_t N, int32_t K, int32_t P, int32_t V, double pseudocount, float* aa_freq,
                            float* entropy, int64_t* consensus, float* mean_points, float* rmsf, float* log_prob, float* consensus_identity,
                            float* rmsd_to_mean, float* n_eff, int64_t* central, void* workspace, size_t workspace_bytes, void* stream);

/* Design similarity: the two superposition-free comparisons of a design with the native of its patch, lDDT and the
 * recovery of the native residue contacts (Fnat).  Rows, groups, points and masks as in "Common layout" above (rows = G * group_size,
 * points (rows,K,P,3), masks (G,K), residue_mask NULL = all present); native_points (G,K,P,3) are the same points of the patch's native.
 * A residue is PRESENT when it is inside residue_mask and COUNTED when it is present and generated.  This is the project's own statement of
 * the published definitions (lDDT: Mariani et al. 2013, thresholds 0.5, 1, 2, 4 A; Fnat as in CAPRI / DockQ, on residue pairs).
 *
 * Arithmetic.  The distance of two points is d = sqrtf(((dx*dx) + dy*dy) + dz*dz) in fp32, dx, dy, dz one rounded subtraction each, no
 * contraction; d_nat(a,b) is taken between two native points and d_des(a,b) between the same two points of the design row - the context
 * residues of the design are whatever the row holds.  Every comparison is made in fp32 on those values, against inclusion_radius,
 * contact_distance and the thresholds as fp32.  Every accumulator is an integer: a row's numbers depend on neither the order of the sums
 * nor the other rows of the call, and the per-patch integers are the same whichever design they are computed beside.  Every ratio is ONE
 * fp32 division of two integers converted to fp32, NaN where the denominator is 0.
 *
 * lDDT.  For a point a of a counted residue i and every point b of a present residue j != i: the pair is SCORED when d_nat < inclusion_radius
 * and PRESERVED AT tau when it is scored and |d_des - d_nat| < tau (one rounded subtraction), tau = 0.5, 1, 2, 4.
 *   n_pairs (G,K) int32:        the scored pairs of residue i - a property of the native; 0 where i is not counted;
 *   preserved (rows,K,4) int32: the pairs of residue i preserved at each tau; 0 where i is not counted;
 *   lddt_residue (rows,K):      (sum_tau preserved) / (4 n_pairs); NaN where n_pairs = 0 or i is not counted;
 *   lddt (rows):                (sum_i sum_tau preserved) / (4 sum_i n_pairs) over the counted residues - a pair of two counted residues is
 *                               counted from both sides;
 *   lddt_thresholds (rows,4):   (sum_i preserved_tau) / (sum_i n_pairs);
 *   lddt_segment (rows,S):      lddt over the counted residues with segment_idx = s.  segment_idx (G,K) int64 or NULL with S = 0: labels in
 *                               [0, S), S <= DIFFAB_METRICS_MAX_SEGMENTS, anything else = no segment.
 * With antigen_mask (G,K) a second set of integer counters takes the scored pairs whose j is inside antigen_mask: n_pairs_interface (G,K),
 * preserved_interface (rows,K,4), ilddt_residue (rows,K), ilddt (rows), the same ratios.  Without antigen_mask those four may be NULL.
 *
 * Native contacts.  A residue pair is a counted residue i and a PARTNER j != i: a present residue that, with antigen_mask, is inside
 * antigen_mask, and without it is not bonded to i.  Bonded: chain[i] == chain[j] and |residue_idx[i] - residue_idx[j]| = 1 (chain,
 * residue_idx (G,K) int32, the rule of diffab_sample_guidance); with chain = residue_idx = NULL, |i - j| = 1 by position in the patch.
 * The pair is IN CONTACT in a structure when one of its P x P point distances is < contact_distance (the smallest one is).
 *   native_contacts_residue (G,K) int32: the partners of residue i in contact in the native; 0 where i is not counted;
 *   n_native (G) int32:         their sum over the counted residues (a pair of two counted residues is counted from both sides);
 *   n_design (rows) int32:      the same sum in the design row;
 *   n_kept (rows) int32:        pairs in contact in both;  kept_residue (rows,K) int32: those of residue i, 0 where i is not counted;
 *   fnat (rows) = n_kept / n_native;  fnonnat (rows) = (n_design - n_kept) / n_design.
 *
 * One launch: one work-group of four waves per (patch, four designs), one wave per design.  The native points of the patch and the four
 * design rows are staged in LDS, 15 (K | 1) P floats and 3 K bytes, which has to fit 64 KiB: K * P <= DIFFAB_METRICS_SIMILARITY_MAX_POINTS
 * = 1024 (K <= 256 for the backbone, K <= 1024 for the CA).  A patch without a counted residue stages nothing.
 * Limits, DIFFAB_ERR_ARG before anything is enqueued: rows >= 0 a multiple of group_size, 1 <= group_size <= DIFFAB_METRICS_MAX_GROUP,
 * 1 <= K <= DIFFAB_METRICS_MAX_K, 1 <= P <= DIFFAB_METRICS_MAX_POINTS, K * P as above, 0 <= S <= DIFFAB_METRICS_MAX_SEGMENTS with
 * segment_idx and lddt_segment exactly when S > 0, inclusion_radius and contact_distance finite and > 0, chain without residue_idx or the
 * reverse, a null points, native_points, generation_mask or output (the interface outputs: with antigen_mask).  rows = 0 succeeds without
 * looking at a pointer. */
#define DIFFAB_METRICS_SIMILARITY_MAX_POINTS 1024
int diffab_metrics_similarity(const float* points, const float* native_points, const uint8_t* generation_mask, const uint8_t* residue_mask,
                              const uint8_t* antigen_mask, const int64_t* segment_idx, const int32_t* chain, const int32_t* residue_idx,
                              int32_t rows, int32_t group_size, int32_t K, int32_t P, int32_t S, float inclusion_radius,
                              float contact_distance, int32_t* n_pairs, int32_t* n_pairs_interface, int32_t* preserved,
                              int32_t* preserved_interface, float* lddt_residue, float* lddt, float* lddt_thresholds, float* ilddt_residue,
                              float* ilddt, float* lddt_segment, int32_t* n_native, int32_t* native_contacts_residue, int32_t* n_design,
                              int32_t* n_kept, float* fnat, float* fnonnat, int32_t* kept_residue, void* stream);

/* Backbone refinement: close the peptide bonds between the rigid frames of finished designs.  Model-free; rows,
 * groups and masks as in "Common layout" above (rows = G * group_size, masks, chain and residue_idx (G,K), residue_mask NULL = all
 * present).  translations (rows,K,3) and orientations (rows,K,3,3) fp32 are the frames sample() returns: rows of O are the local axes.
 *
 * Atoms.  N = t + (-0.525 O0 + 1.363 O1), CA = t, C = t + 1.526 O0 (O0, O1 the first two rows of O): io.IDEAL_BACKBONE.
 * Moving residues.  A residue MOVES when generation_mask is set and it is inside residue_mask.  Every other residue is fixed: its
 * output is its input's bits.  A fixed residue inside residue_mask still exerts forces.
 * Chain neighbours.  succ(i) / pred(i) as for diffab_metrics_backbone: the lowest slot with the same chain and residue_idx + 1 / - 1,
 * both inside residue_mask.  (With two slots of one (chain, residue_idx) key a residue feels its own two links only.)
 * Energy of a design: a sum of terms w (|a - b| - d0)^2,
 *   bond   w_bond  (|C_i  - N_s|  - DIFFAB_REFINE_BOND)^2                                 s = succ(i), for every link i -> s of which
 *   angle  w_angle (|CA_i - N_s|  - DIFFAB_REFINE_CA_N)^2 + w_angle (|C_i - CA_s| - DIFFAB_REFINE_C_CA)^2      at least one end moves
 *   trans  w_trans (|CA_i - CA_s| - DIFFAB_REFINE_CA_CA)^2
 *   clash  w_clash (clash_distance - |CA_i - CA_j|)^2 where the distance is below clash_distance, once per unordered pair {i, j} inside
 *          residue_mask of which at least one moves, not chain neighbours (equal chain and residue_idx differing by exactly 1)
 *   tether w_tether |CA_i - CA_i of the input|^2 over the moving residues.
 * DIFFAB_REFINE_CA_N / _C_CA are the third sides of the triangles (1.526, 1.329, 116.2 degrees) and (1.329, |N - CA| = 1.46061...,
 * 121.7 degrees), computed in double.  A cis peptide is pulled to trans by the CA - CA term.
 * One iteration is a Jacobi step: every moving residue k reads the state before the step.
 *   force on a of a term with partner b: ((-2 w) (d - d0) / d) (a - b), d = |a - b| = sqrt((dx dx + dy dy) + dz dz); none where d < 1e-6.
 *   f_C  = bond(C_k, N_s) + angle(C_k, CA_s);        f_N = bond(N_k, C_p) + angle(N_k, CA_p)                 p = pred(k), s = succ(k)
 *   f_CA = angle(CA_k, N_s) + trans(CA_k, CA_s) + angle(CA_k, C_p) + trans(CA_k, CA_p) + clash + tether, added in this order;
 *          clash = sum over the partners j of ((2 w_clash) (clash_distance - d) / d) (CA_k - CA_j), 1e-6 <= d < clash_distance: four
 *          partial sums over j = l, l + 4, l + 8, ... (l = 0..3, ascending), combined as (0 + 1) + (2 + 3);
 *          tether = (-2 w_tether) (CA_k - CA_k of the input).
 *   F = (f_N + f_CA) + f_C;    torque = (N_k - CA_k) x f_N + (C_k - CA_k) x f_C
 *   t <- t + step F  (kept as it is where F is exactly zero)
 *   O <- O Exp(w)^T, w = (step / DIFFAB_REFINE_INERTIA) torque  (kept where w is exactly zero); Exp(w) = I + a hat(w) + b (w w^T - |w|^2 I),
 *        a = sin|w| / |w|, b = (1 - cos|w|) / |w|^2 (Rodrigues; a = 1, b = 1/2 where |w| < 1e-6); then N and C are placed again.
 * After the last step the rows of every O that was rotated at least once are orthonormalised: e1 = O0 / |O0|, e2 = the normalised
 * O1 - (e1 . O1) e1, e3 = e1 x e2 (the order of io.frames_from_backbone), and N and C are placed once more.  With iterations = 0, or all
 * weights 0, every output bit is the input's.  All of this is fp32, one rounding per operation as written (no contraction), in an order
 * that depends on K alone: a design alone gives the bits it gives in a batch, and group_size changes no bits.
 * Outputs.  out_translations / out_orientations: the refined frames.  Each of the following may be NULL: energy_before / energy_after
 * (rows): the energy of the input and of the output frames; terms_after (rows,5): bond, angle, trans, clash, tether of the output;
 * each term in fp32, summed in fp64 in a fixed order of the row and rounded once.  max_shift (rows): the largest |CA - CA of the
 * input| over the moving residues, 0 without one.
 * One work-group of 256 threads per row for all iterations, the row's atoms in DIFFAB_REFINE_LDS_BYTES(K) bytes of LDS; a launch before
 * it finds the chain neighbours of every patch.  A row without a moving residue is copied and its energies (0) reported.
 * opt: NULL means DIFFAB_REFINE_DEFAULTS.  Refused before anything is enqueued, DIFFAB_ERR_ARG with a message: struct_bytes other than
 * sizeof(diffab_refine_options) (checked before any other field); rows < 0, group_size < 1, rows no multiple of group_size, K outside
 * [1, DIFFAB_REFINE_MAX_K]; iterations outside [0, DIFFAB_REFINE_MAX_ITERATIONS]; a step or clash_distance that is not finite and > 0; a
 * weight that is not finite and >= 0; step x the largest weight (the product in double of the fp32 values) above
 * DIFFAB_REFINE_MAX_STEP_WEIGHT (0.1 and a float rounding: the energy fell monotonically at 0.08 and not at 0.12); a null input or frame
 * output; an output that is its input; a workspace that is NULL or not 16-byte aligned (smaller than
 * DIFFAB_REFINE_WORKSPACE_BYTES(G, K): DIFFAB_ERR_WORKSPACE).  rows = 0 succeeds without looking at a pointer. */
#define DIFFAB_REFINE_MAX_K 256
#define DIFFAB_REFINE_MAX_ITERATIONS 100000
#define DIFFAB_REFINE_BOND 1.329f
#define DIFFAB_REFINE_CA_N 2.4260487261296753f
#define DIFFAB_REFINE_C_CA 2.437145924677046f
#define DIFFAB_REFINE_CA_CA 3.8f
#define DIFFAB_REFINE_INERTIA 4.45f
#define DIFFAB_REFINE_MAX_STEP_WEIGHT 0.1000001
#define DIFFAB_REFINE_WORKSPACE_BYTES(G, K) ((size_t)(G) * (size_t)(K) * 8 + 1024)
#define DIFFAB_REFINE_LDS_BYTES(K) ((size_t)(K) * 148)
typedef struct {
  uint32_t struct_bytes; /* sizeof(diffab_refine_options); anything else: DIFFAB_ERR_ARG, before any other field is read */
  int32_t iterations;
  float step;
  float w_bond, w_angle, w_trans, w_clash, w_tether;
  float clash_distance;
} diffab_refine_options;
#define DIFFAB_REFINE_DEFAULTS {(uint32_t)sizeof(diffab_refine_options), 200, 0.05f, 1.0f, 1.0f, 1.0f, 1.0f, 0.0f, 3.8f}
int diffab_refine_backbone(const float* translations, const float* orientations, const uint8_t* generation_mask, const uint8_t* residue_mask,
                           const int32_t* chain, const int32_t* residue_idx, int32_t rows, int32_t group_size, int32_t K,
                           const diffab_refine_options* opt, float* out_translations, float* out_orientations, float* energy_before,
                           float* energy_after, float* terms_after, float* max_shift, void* workspace, size_t workspace_bytes, void* stream);

/* Backward of the two context encoders (training through encode_context, diffab_pytorch.py:843-854 under autograd).
 * d_out is the gradient w.r.t. the module output; parameter gradients ACCUMULATE (+=) into the buffers of `g`, which has the
 * layout of the weight struct (the caller zero-fills them).  Inputs other than parameters take no gradient.  Nothing is taped:
 * the backward recomputes the forward of each chunk.  PairEmbedding: the reference's own autograd fails on an in-place product
 * (:295-301); this is the gradient of the same forward with that product out of place (it does not reach the output). */
size_t diffab_residue_embedding_bwd_workspace_bytes(const diffab_ctx_dims* d);
int diffab_residue_embedding_bwd(const diffab_ctx_dims* d, const diffab_residue_emb_weights* w, const diffab_residue_emb_weights* g,
                                 const int64_t* seq_idx, const float* xyz, const float* orientations, const float* dihedrals,
                                 const int64_t* chain_idx, const float* atom_mask, const uint8_t* structure_context_mask,
                                 const uint8_t* sequence_context_mask, const float* d_out /* (B,K,D) */, void* workspace,
                                 size_t workspace_bytes, void* stream);
size_t diffab_pair_embedding_bwd_workspace_bytes(const diffab_ctx_dims* d);
/* exactly one of distmat (B,K,K,A,A) / xyz (B,K,A,3) is non-null, as in the two forward entries */
int diffab_pair_embedding_bwd(const diffab_ctx_dims* d, const diffab_pair_emb_weights* w, const diffab_pair_emb_weights* g,
                              const int64_t* seq_idx, const float* distmat, const float* xyz, const float* pairwise_dihedrals,
                              const int64_t* residue_idx, int32_t residue_idx_batch_stride, const int64_t* chain_idx,
                              const float* atom_mask, const uint8_t* sequence_context_mask, const float* d_out /* (B,K,K,C) */,
                              void* workspace, size_t workspace_bytes, void* stream);
/* Taped form of the PairEmbedding pair (round 6; where diffab_pair_embedding_tape_bytes(d) > 0: C = 64, K a multiple of 128, A <= 16):
 * the forward also leaves the four hidden activations of every pair row on `tape` (4 x B K K C floats: 8.6 GB at B = 128, K = 128 - the
 * 288 GB of an MI355X hold it), and the backward reads them instead of recomputing the forward chunk by chunk (-2 ms of 12 at B = 128).
 * Same arguments and results as diffab_pair_embedding_fwd / _xyz_fwd (exactly one of distmat / xyz non-null) and diffab_pair_embedding_bwd;
 * the tape must be 16-byte aligned and stay untouched between the two calls.  Reference: autograd's saved tensors of
 * PairEmbedding.forward, diffab_pytorch.py:186-312. */
size_t diffab_pair_embedding_tape_bytes(const diffab_ctx_dims* d);
int diffab_pair_embedding_fwd_taped(const diffab_ctx_dims* d, const diffab_pair_emb_weights* w, const int64_t* seq_idx, const float* distmat,
                                    const float* xyz, const float* pairwise_dihedrals, const int64_t* residue_idx,
                                    int32_t residue_idx_batch_stride, const int64_t* chain_idx, const float* atom_mask,
                                    const uint8_t* sequence_context_mask, float* out, float* tape, size_t tape_bytes, void* workspace,
                                    size_t workspace_bytes, void* stream);
int diffab_pair_embedding_bwd_taped(const diffab_ctx_dims* d, const diffab_pair_emb_weights* w, const diffab_pair_emb_weights* g,
                                    const int64_t* seq_idx, const float* distmat, const float* xyz, const float* pairwise_dihedrals,
                                    const int64_t* residue_idx, int32_t residue_idx_batch_stride, const int64_t* chain_idx,
                                    const float* atom_mask, const uint8_t* sequence_context_mask, const float* d_out, const float* tape,
                                    size_t tape_bytes, void* workspace, size_t workspace_bytes, void* stream);

/* ---- reverse process (build-defined; reference stub diffab_pytorch.py:770-776) -- */
/* One update t -> t-1 from denoiser outputs with explicit noise (z (B,K,3), rotvec (B,K,3), u_seq (B,K)),
 * in place on (seq, x, O), only where gen_mask is set. */
int diffab_reverse_update(const diffab_sched* s, int32_t t, int64_t* seq, float* x, float* O, const float* eps_hat,
                          const float* O0_hat, const float* posterior, const uint8_t* gen_mask, const float* z,
                          const float* rotvec, const float* u_seq, int32_t B, int32_t K, int32_t V, void* stream);
/* The whole reverse trajectory t = t_start .. t_stop+1 (normally T .. 1) for B patches, all launches
 * enqueued on `stream` with no host synchronisation: denoise step + Philox noise + IGSO3 draw (table
 * over sqrt(beta)) + update.  State (seq, x, O) is updated in place.  Noise is keyed by
 * (seed, first_patch + b, residue, t), so any sharding of a batch over ranks gives identical samples.  The design-mode bits
 * DIFFAB_FLAG_KEEP_STRUCTURE / _SEQUENCE restrict the update to the other modality (fixed-backbone sequence design, structure
 * prediction); antibody optimisation starts the loop at t_start = t from diffab_sample_init_noised. */
int diffab_sample_loop(const diffab_dims* d, const diffab_denoiser_weights* w, const diffab_sched* s,
                       const diffab_igso3* rev_tab, int64_t* seq, float* x, float* O, const float* res_ctx,
                       const float* pair_ctx, const uint8_t* gen_mask, uint64_t seed, int64_t first_patch, int32_t t_start,
                       int32_t t_stop, void* workspace, size_t workspace_bytes, uint32_t flags, void* stream);
/* Initial state at t = T on generated residues: x ~ N(0,I), O ~ uniform SO(3), s ~ U{0..19} (Philox, step = T+1). */
int diffab_sample_init(int64_t* seq, float* x, float* O, const uint8_t* gen_mask, uint64_t seed, int64_t first_patch,
                       int32_t B, int32_t K, int32_t T, void* stream);
/* diffab_sample_init with the design-mode bits of `flags`: DIFFAB_FLAG_KEEP_STRUCTURE leaves x and O, DIFFAB_FLAG_KEEP_SEQUENCE leaves
 * seq as given (other bits are ignored).  flags without either bit: bitwise diffab_sample_init.  allowed (nullable): the sequence
 * constraints of "Sampler options" below; NULL with flags = 0 is exactly diffab_sample_init (which is this call with both). */
int diffab_sample_init_ex(int64_t* seq, float* x, float* O, const uint8_t* gen_mask, uint64_t seed, int64_t first_patch,
                          int32_t B, int32_t K, int32_t T, uint32_t flags, const uint32_t* allowed, void* stream);
/* Starting state of antibody optimisation: the given (native) state of the generated residues is forward-noised to step t, in place
 * (reference forward process, diffusion.py:105-135, 199-236, 262-294), with Philox noise keyed by (seed, first_patch + b, residue, t) on
 * its own streams (philox.h STREAM_OPT_*), so sharding and replicated rows behave as in the reverse loop:
 *   x_t = sqrt(abar_t) x_0 + sqrt(1 - abar_t) eps,
 *   O_t = scale(O_0, sqrt(abar_t)) exp(w), w drawn from row t of fwd_tab (the IGSO3 table over sigma_t = sqrt(1 - abar_t),
 *         T+1 rows) by the reverse loop's rule: inverse CDF of the histogram below the table's threshold, the Gaussian angle above,
 *   s_t ~ q(s_t | s_0) = abar_t onehot(s_0) + (1 - abar_t) / 21, by inverse CDF.
 * Build-defined: every residue's angle is an independent inverse-CDF draw (the reference's forward noise draws a patch's histogram
 * bins without replacement, so3.py:78), as in the reverse loop.  Context residues are never written; DIFFAB_FLAG_KEEP_STRUCTURE /
 * _SEQUENCE leave that modality un-noised.  allowed (nullable): the sequence constraints of "Sampler options" below.  DIFFAB_ERR_ARG
 * for t outside [1, T], a fwd_tab with fewer than T+1 rows, or both bits. */
int diffab_sample_init_noised(const diffab_sched* s, const diffab_igso3* fwd_tab, int64_t* seq, float* x, float* O,
                              const uint8_t* gen_mask, uint64_t seed, int64_t first_patch, int32_t B, int32_t K, int32_t t,
                              uint32_t flags, const uint32_t* allowed, void* stream);

/* ==== Sampler options (build-defined) ===================================================================================================
 * Everything the reverse loop can do beyond diffab_sample_loop travels in ONE struct, diffab_sample_options (defined after the option
 * structs below), given to diffab_sample_loop_ex.  Every field is nullable / zero = off, and the options combine freely; each block below
 * describes one option and names the field of diffab_sample_options that carries it.
 *
 * ---- shared contexts: diffab_sample_options.n_ctx and .ctx_of_row -------------------------------------------------------------------
 * Contexts shared between state rows (many designs of one patch from one context): res_ctx (n_ctx,K,D) and
 * pair_ctx (n_ctx,K,K,C) hold n_ctx contexts, and state row b (seq/x/O/gen_mask are (d->B,K,...)) is denoised against context
 * ctx_of_row[b].  ctx_of_row is a HOST array of d->B entries, each in [0, n_ctx) (else DIFFAB_ERR_ARG, nothing enqueued); it is copied
 * to the workspace once per call (the call returns with the host array no longer needed).  The pair context is read through the map by
 * every attention form (planes, DIFFAB_FLAG_PAIR_F32, DIFFAB_FLAG_FORCE_GENERIC, the patch-resident module, graph replay, skipped row
 * tiles) and never expanded to B rows; its fp16 planes are built once per context.  Noise stays keyed by (seed, first_patch + b,
 * residue, t): the result is bitwise that of diffab_sample_loop on the contexts replicated row by row.  workspace:
 * diffab_sample_shared_workspace_bytes(d, n_ctx).  ctx_of_row NULL: the identity (n_ctx must be 0 or d->B; diffab_sample_workspace_bytes(d)
 * suffices) - diffab_sample_loop is exactly that call. */
/* ---- sequence constraints: diffab_sample_options.allowed (and `allowed` of diffab_sample_init_ex / _noised) --------------------------
 * Per-residue allowed amino-acid classes.
 * `allowed` is a caller-owned DEVICE buffer of B*K uint32 words, one per (state row, residue) in the layout of gen_mask; bit v of a
 * word allows class v (io.AA3 order: the 20 amino acids, then UNK = 20).  Bits at and above the vocabulary size are ignored.  Only
 * GENERATED residues read their word, and only where the sequence is diffused; context residues are never written.  Every draw uses
 * the Philox lane of the unconstrained entry, so noise keys, sharding and replicated rows behave exactly as there.  With A the
 * residue's allowed set:
 *   reverse step (STREAM_SEQ): tot = sum of p_v over v in A in increasing v, thr = u tot; the first v in A whose running sum exceeds
 *     thr, else the largest v in A; tot == 0: the floor(u |A|)-th element of A.  On both posterior paths (the folded heads' softmax
 *     in the update kernel, and the heads kernel's posterior).  A = all V classes: bitwise the unconstrained draw;
 *   initial state (STREAM_INIT_S): uniform over A \ {UNK} (over A when A = {UNK}): its floor(u n)-th element, clamped to n - 1.
 *     All classes: bitwise the unconstrained min(int(u 20), 19);
 *   optimisation start (STREAM_OPT_SEQ): q(s_t | s_0) restricted to A and renormalised, drawn by the reverse-step rule (a native
 *     token outside A is not reachable).
 * Structure draws (x, O) and the denoiser are untouched.  A generated residue with an empty A is the caller's error (DiffAb.sample
 * rejects it): its token is then left as it is.  allowed == NULL: unconstrained.
 * A non-NULL allowed with DIFFAB_FLAG_KEEP_SEQUENCE, or (loop) with d->V > 32: DIFFAB_ERR_ARG, nothing enqueued. */
/* ---- trajectory recording: diffab_sample_options.record ----------------------------------------------------------------------------
 * The reverse process, step by step; record == NULL: no trajectory.
 * Labels are steps: slot j = slot_of_step[t] (a HOST table of T + 1 int32, -1 = not recorded) holds, for step t,
 *   the state that step t denoises: s_t, x_t, O_t (label t_start: the state the call was given - diffab_sample_init*'s, or the
 *     forward-noised native of optimize_from).  Bitwise the output of this call with t_stop = t, same seed, first_patch, flags, map and
 *     allowed.  The final state is the call's own output and has no slot;
 *   with pred_x / pred_O / seq_probs, what the denoiser made of that state: x0_hat = (x_t - one_minus_alpha_bar_sqrt[t] eps_hat) /
 *     alpha_bar_sqrt[t], O0_hat = O_t exp(hat(v)), and the softmax posterior over s_{t-1} - the UNRESTRICTED one: an `allowed` draw
 *     renormalises it over the residue's set.  Slot of step 1: the distribution the returned token was drawn from.
 * Residues that are not generated hold their given state in every slot; their predictions are their x / O and a one-hot of their
 * token.  A kept modality (DIFFAB_FLAG_KEEP_STRUCTURE / _SEQUENCE) appears in the predictions as its given values (x_t, O_t; a one-hot
 * of s_t).  Layout, B state rows outermost so a shard's rows are one contiguous slice: seq (B, n_slots, K) int64, x / pred_x
 * (B, n_slots, K, 3), O / pred_O (B, n_slots, K, 3, 3), seq_probs (B, n_slots, K, V), all caller-owned DEVICE buffers.  Rows [lo, hi)
 * run with first_patch = lo record that slice of the whole call's record, bitwise.  Recording does not change the sample: the state the
 * call returns is bitwise the same with and without `rec`, on every launch form (graph replay included: the update kernel reads
 * slot_dev[t] with t from device memory).  Cost: one uniform branch per step without a slot; with one, 56 B of state plus 12 + 36 + 4 V
 * B of predictions per generated residue, written by the update kernel.
 * slot_dev: a caller-owned DEVICE array of T + 1 int32 the call fills from slot_of_step with one hipMemcpyAsync (not workspace: the
 * workspace size is unchanged).  Checked before anything is enqueued, DIFFAB_ERR_ARG: n_slots >= 1; every entry -1 or in [0, n_slots);
 * every slot given to exactly one step; no slot for a step outside [t_stop + 1, t_start] (it would never be written); null
 * slot_of_step, slot_dev, seq, x or O; some but not all of pred_x, pred_O, seq_probs (and predictions need s->alpha_bar_sqrt). */
typedef struct {
  int32_t n_slots;
  const int32_t* slot_of_step; /* HOST (T + 1): step t -> slot, -1 = not recorded */
  int32_t* slot_dev;           /* DEVICE (T + 1), filled by the call */
  int64_t* seq;                /* (B, n_slots, K) */
  float* x;                    /* (B, n_slots, K, 3) */
  float* O;                    /* (B, n_slots, K, 3, 3) */
  float* pred_x;               /* (B, n_slots, K, 3), nullable (all three predictions or none) */
  float* pred_O;               /* (B, n_slots, K, 3, 3) */
  float* seq_probs;            /* (B, n_slots, K, V) */
} diffab_sample_record;
/* ---- fewer-step reverse sampling: diffab_sample_options.steps ----------------------------------------------------------------------
 * The reverse process on a subsequence of the steps; steps == NULL: every step.
 * A run names the steps it executes, tau_0 = t_start > tau_1 > ... > tau_{n-1} > t_stop.  Step tau_j denoises the state at tau_j (the
 * denoiser's time input is beta[tau_j], as always) and moves it to s = tau_{j+1}; the last step moves it to s = t_stop.  Philox noise
 * stays keyed by (seed, first_patch + b, residue, t = tau_j) on the same streams.  With abar = alpha_bar and V the vocabulary size:
 *   jump coefficients (HOST tables, the caller's): beta'_t = clip(1 - abar_t / abar_s, 1e-5, beta_max), alpha'_t = 1 - beta'_t,
 *     computed in float64 and stored as fp32; when s = t - 1 they are the schedule's own beta[t] / alpha[t], copied;
 *   translations: x_s = (x_t - beta'_t / sqrt(1 - abar_t) eps_hat) / sqrt(alpha'_t) + [s > 0] sqrt(beta'_t) z;
 *   orientations: O_s = O0_hat exp(hat(w)) when s > 0, else O0_hat; w is drawn as always from row t of rev_tab, which for a respaced
 *     run is the IGSO3 table over sigma_t = sqrt(beta'_t) (the caller builds it; stride-1 rows are the ordinary table's rows);
 *   sequence: s = t - 1 draws from the head posterior p exactly as diffab_sample_loop.  s < t - 1 first recovers p(s_0 | s_t) from p,
 *     in double: A_v = alpha_t [v = s_t] + beta_t / V, c = (1 - abar_{t-1}) / V, S = sum_v p_v / A_v,
 *     pi~_v = (abar_{t-1} A_v + c) max(0, p_v / A_v - c S), pi = pi~ / sum pi~ (pi = p when sum pi~ = 0) - the exact inverse of
 *     p = sum_u pi_u q(s_{t-1} | s_t, u).  Then A'_v = alpha'_t [v = s_t] + (1 - alpha'_t) / V, c' = (1 - abar_s) / V,
 *     Z'_u = abar_s A'_u + c', W = sum_u pi_u / Z'_u and r_v = A'_v (c' W + abar_s pi_v / Z'_v) = sum_u pi_u q(s_s | s_t, u) (r = pi at
 *     s = 0).  s_s is drawn from r (rounded to fp32) with the STREAM_SEQ uniform of step t by the reverse-step rule (restricted to the
 *     residue's `allowed` classes when given).
 * Listing every step t_start .. t_stop + 1 with the schedule's own beta / alpha is bitwise the call with steps == NULL.
 * The eager loop runs over the list; graph replay advances the device timestep through the plan's next[] table, n - 1
 * replays after the first step.  plan_dev: a caller-owned DEVICE buffer of 3 (T + 1) 32-bit words - next[T + 1] int32 (next[tau_j] =
 * tau_{j+1}, t_stop after the last; t - 1 elsewhere), beta'[T + 1] and alpha'[T + 1] fp32 - the call fills it from the host fields with
 * one hipMemcpyAsync (not workspace: the workspace size is unchanged).  Needs s->alpha_bar.  Checked before anything is
 * enqueued, DIFFAB_ERR_ARG: n_steps < 1; a null field; steps[0] != t_start; a list that is not strictly descending; an entry <= t_stop
 * or > T; beta'_t or alpha'_t outside (0, 1) at a listed step; a record slot for a step the list does not run. */
typedef struct {
  int32_t n_steps;
  const int32_t* steps;     /* HOST (n_steps): tau_0 = t_start > ... > tau_{n-1} > t_stop */
  const float* beta_jump;   /* HOST (T + 1): beta'_t at every listed step t (other entries unread) */
  const float* alpha_jump;  /* HOST (T + 1): alpha'_t = 1 - beta'_t */
  void* plan_dev;           /* DEVICE 3 (T + 1) 32-bit words, filled by the call */
} diffab_sample_steps;
/* Teacher-forced jump t -> s (the analogue of diffab_reverse_update): explicit z (B,K,3), rotvec (B,K,3), u_seq (B,K) and jump
 * coefficients beta_jump / alpha_jump; the rule above, in place on (seq, x, O) where gen_mask is set.  r_out (B,K,V, nullable): the
 * distribution s_s is drawn from, for the generated residues (p itself when s = t - 1).  s = t - 1 with the schedule's beta[t] / alpha[t]
 * is bitwise diffab_reverse_update.  DIFFAB_ERR_ARG: t outside [1, T], s outside [0, t), beta_jump / alpha_jump outside (0, 1), V > 32,
 * a null pointer, or a schedule without alpha_bar. */
int diffab_reverse_update_jump(const diffab_sched* s, int32_t t, int32_t s_next, float beta_jump, float alpha_jump, int64_t* seq, float* x,
                               float* O, const float* eps_hat, const float* O0_hat, const float* posterior, const uint8_t* gen_mask,
                               const float* z, const float* rotvec, const float* u_seq, float* r_out, int32_t B, int32_t K, int32_t V,
                               void* stream);
/* ---- structure guidance: diffab_sample_options.guidance --------------------------------------------------------
 * Clash and chain-bond potentials on the translations; guidance == NULL: unguided.
 * Per state row, over the unordered pairs {i, j}, i != j, with residue_mask set on both and at least one of them generated:
 *   p_i = x0_hat_i = (x_t,i - one_minus_alpha_bar_sqrt[t] eps_hat_i) / alpha_bar_sqrt[t] for a generated residue - the expression, and
 *     so bitwise the value, of the record's pred_x - and the given x_i for one that is not generated;
 *   bonded: chain_i == chain_j and |residue_idx_i - residue_idx_j| == 1;  d = |p_i - p_j| (Angstrom: coordinates are not scaled);
 *   U = w_clash sum_nonbonded max(0, clash_distance - d)^2 + w_bond sum_bonded (d - bond_length)^2;
 *   g_i = dU / dp_i for generated i (0 elsewhere); a pair with d < 1e-6 contributes no gradient (it still counts in U);
 *   at a guided step t <= t_max: Delta_i = beta'_t g_i, beta'_t = beta[t] (the step plan's beta' in a respaced run) - the variance of the
 *     step's Gaussian, so the guidance fades with the noise; |Delta_i| > max_shift scales Delta_i to length max_shift (INFINITY: no cap);
 *   x_s = mu - Delta_i + [s > 0] sqrt(beta'_t) z: Delta is subtracted from the ordinary mean mu before the noise is added.  The last step
 *     (s = 0) is guided too.  Orientations, sequence draws, Philox lanes, the record (pred_x included) are untouched.
 * One work-group per state row stages p, chain, residue_idx and the masks in LDS tiles of 256 residues (every K); its four waves scan
 * a quarter of the partners each for the same owners, summed in a fixed order, no atomics.  Launched right before the update of every
 * step, on every launch form (graph replay reads t from device memory).  shift_dev: a caller-owned DEVICE (B, K, 3) fp32 buffer the
 * call writes every step - Delta of the last step after the call (0 where not generated, and all 0 when that step had t > t_max); not
 * workspace: the workspace size is unchanged.
 * chain / residue_idx: DEVICE (B, K) int32 per state row; residue_mask: DEVICE (B, K) uint8, NULL = all set.
 * Both weights 0 still runs the kernel and gives Delta = +0: bitwise the unguided run; so does t_max = 0 (no step is guided). */
typedef struct {
  float w_clash;              /* >= 0, finite */
  float clash_distance;       /* d0 > 0 (3.8) */
  float w_bond;               /* >= 0, finite */
  float bond_length;          /* L > 0 (3.8) */
  float max_shift;            /* > 0; INFINITY = no cap */
  int32_t t_max;              /* steps t <= t_max are guided, in [0, T] */
  const int32_t* chain;       /* DEVICE (B, K) */
  const int32_t* residue_idx; /* DEVICE (B, K) */
  const uint8_t* residue_mask;/* DEVICE (B, K), nullable = all */
  float* shift_dev;           /* DEVICE (B, K, 3), written by the call */
} diffab_sample_guidance;
/* Needs s->alpha_bar_sqrt.  Checked before anything is enqueued, DIFFAB_ERR_ARG: a negative or non-finite weight;
 * clash_distance or bond_length <= 0 or not finite; max_shift <= 0 or NaN; t_max outside [0, T]; null chain, residue_idx or shift_dev;
 * DIFFAB_FLAG_KEEP_STRUCTURE (the structure is not sampled). */
/* The potential of the rule above at given coordinates (p = x for every residue), for B rows of K residues: per row, UNWEIGHTED,
 * clash = sum_nonbonded max(0, d0 - d)^2, bond = sum_bonded (d - L)^2, n_clash = the number of nonbonded pairs with d < d0, and
 * max_bond_deviation = the largest |d - L| over bonded pairs (0 without one); grad (nullable, (B, K, 3)) = the WEIGHTED gradient g
 * (w_clash, w_bond applied; 0 where not generated; neither scaled by beta nor capped).  Pairs as above (mask on both, at least one
 * generated).  Each row is one work-group with a fixed reduction order and no atomics: the result of a row does not depend on B.  Reads
 * w_clash, clash_distance, w_bond, bond_length, chain, residue_idx and residue_mask of `g` (max_shift, t_max, shift_dev are ignored).
 * DIFFAB_ERR_ARG: the weight / distance checks of diffab_sample_options.guidance, B < 0, K < 1, a null x, gen_mask, g, chain, residue_idx,
 * clash, bond, n_clash or max_bond_deviation. */
int diffab_guidance_energy(const float* x, const uint8_t* gen_mask, const diffab_sample_guidance* g, int32_t B, int32_t K, float* clash,
                           float* bond, int32_t* n_clash, float* max_bond_deviation, float* grad, void* stream);
/* ---- noise scales and sequence temperature: diffab_sample_options.temperature --------------------------------
 * How greedy the reverse sampler is; temperature == NULL: untempered.
 * Three values per state row b: lambda_x = trans_scale[b], lambda_O = rot_scale[b], tau = seq_temp[b]; a NULL pointer is 1 for every row.
 *   translations: x_s = mu - Delta + [s > 0] lambda_x sqrt(beta'_t) z (mu the ordinary mean, Delta the guidance shift, z the usual Philox
 *     normal); lambda_x = 0 adds no noise term at all (x_s = mu - Delta exactly);
 *   orientations: theta is drawn by the usual inverse CDF / Gaussian rule at sigma = lambda_O sqrt(beta'_t) from row rot_row[b] + t of
 *     rev_tab, with the same uniforms, normal and axis (lambda_O = 1 over a row built at sqrt(beta'_t) is the ordinary draw); lambda_O = 0
 *     skips the perturbation: O_s = O0_hat exactly;
 *   sequence: s_{t-1} ~ p_v^(1/tau) / sum_u p_u^(1/tau), p the distribution drawn from otherwise (the head posterior, or a respaced step's
 *     jump distribution), restricted to the allowed classes when `allowed` is given; in fp32 as w_v = exp((log p_v - log p_max) / tau),
 *     p_v = 0 weight 0, scanned in increasing v against the usual STREAM_SEQ uniform.  tau = 0: the argmax (lowest index on ties) of the
 *     allowed classes; every allowed class at probability 0: the unit-weight draw of the constrained sampler; tau = 1: the ordinary draw.
 * The posterior, O0_hat and the trajectory record (predictions included) stay the model's untempered outputs; the initial state and
 * optimize_from's forward noise are not scaled.  lambda_x = lambda_O = tau = 1 is bitwise the untempered run.
 * Caller's contract (not checked: the values live on the device): every value finite and >= 0; with rot_scale, rot_row[b] + T is a row of
 * rev_tab for every row b with lambda_O != 0 and rev_tab->sigmas[rot_row[b] + t] = lambda_O sqrt(beta'_t) (fp32).  The tables are
 * read by the update kernel alone, once per generated residue and step. */
typedef struct {
  const float* trans_scale; /* DEVICE (B,) fp32 lambda_x, nullable */
  const float* rot_scale;   /* DEVICE (B,) fp32 lambda_O, nullable (needs rot_row) */
  const float* seq_temp;    /* DEVICE (B,) fp32 tau, nullable */
  const int32_t* rot_row;   /* DEVICE (B,) int32: the row of rev_tab that holds t = 0 of the state row's sigma list */
} diffab_sample_temperature;
/* Checked before anything is enqueued, DIFFAB_ERR_ARG: rot_scale without rot_row; trans_scale or rot_scale with
 * DIFFAB_FLAG_KEEP_STRUCTURE; seq_temp with DIFFAB_FLAG_KEEP_SEQUENCE. */
/* ---- particle steering: diffab_sample_options.steering ---------------------------------------------------------
 * The rows of a group resampled by energy while they form; steering == NULL: unsteered.
 * Sequential Monte Carlo over the reverse process (Feynman-Kac steering / the twisted diffusion sampler).  The state rows are grouped
 * as consecutive runs of group_size = N rows (rows b N .. b N + N - 1 under num_samples = N); all rows of a group share gen_mask, the
 * context and the residue tables (the caller's contract).  Per row two fp32 values live in caller-owned device memory across the steps
 * (and across calls): the accumulated log-weight logw and the last seen energy u_prev, both 0 at the start of a run.
 *   Steering step: an executed step t with t_min <= t <= t_max, (t_max - t) % every == 0 and its successor s (t - 1, or the step plan's
 *     next step) above t_stop - the last executed step never resamples, the finished designs come back with their weights.
 *   Energy: U_r = w_clash sum_nonbonded max(0, clash_distance - d)^2 + w_bond sum_bonded (d - bond_length)^2 of the guidance rule above,
 *     at p = x0_hat (bitwise the record's pred_x) for generated residues and x otherwise, on the state the step denoises, from that
 *     step's eps_hat: before the update and before any guidance shift.  The two sums are bitwise diffab_guidance_energy's at those points.
 *   Weights: logw_r += -(strength (U_r - u_prev_r)) in fp32, then u_prev_r = U_r: over a run the increments telescope to -strength U.
 *   ESS, per group in double: w_r = exp(logw_r - max finite logw) (a non-finite logw: w_r = 0), S = sum w, ESS = S^2 / sum w^2.  The
 *     group resamples iff S > 0 and ESS < ess_threshold N (0: never; above 1: always).  A group with every w_r = 0 does not resample
 *     and its logw is set to 0.
 *   Systematic resampling: one uniform u per group and step, lane x of Philox (seed, first_patch + first row of the group, residue 0,
 *     t, STREAM_STEER = 11); C_i = (sum_{k <= i} w_k) / S in row order; a_j = the smallest i with C_i > (u + j) / N, at most the last
 *     row with w > 0.  Then logw_j = 0 and u_prev_j = U_{a_j} for every row of the group.  A group that does not resample: a_j = j.
 *   What moves: the update of step t runs first, on every row, with its usual noise; then seq, x and O of the generated residues of row
 *     j become those of row a_j (propagate, then select, with the weights of x_t).  Children of one ancestor are equal after step t and
 *     separate at the next step: the Philox noise is keyed by the row, not by the lineage.  Per-row options (temperature, allowed
 *     classes, guidance tables) belong to the row.  The record of step t is written before the gather; the next step records the
 *     gathered state.  DIFFAB_FLAG_KEEP_SEQUENCE leaves seq alone.
 * strength = 0 with ess_threshold <= 1, ess_threshold = 0 and group_size = 1 are bitwise the unsteered states.
 * Three kernels around the update of every step, on every launch form; each evaluates the steering-step predicate itself (graph replay
 * reads t from device memory).  Buffers, all DEVICE and caller-owned (the workspace size is unchanged):
 *   logw, u_prev (rows) fp32: read and written; energy (rows) fp32: U of the last steering step, as computed before its resampling;
 *   ancestors ((T + 1) rows) int32, nullable: filled with -1 by the call, row t = the a_j (indices inside the group) of steering step t;
 *   scratch: DIFFAB_STEER_SCRATCH_BYTES(rows, K) bytes, 8-byte aligned - 56 B per residue (seq 8, x 12, O 36) of the rows being
 *     replaced, because the map is no permutation in place, and the step's ancestor map (4 B per row). */
#define DIFFAB_STEER_MAX_GROUP 1024
#define DIFFAB_STEER_SCRATCH_BYTES(rows, K) ((size_t)(rows) * (size_t)(K) * 56u + (size_t)(rows) * 4u)
typedef struct {
  float w_clash;              /* >= 0, finite */
  float clash_distance;       /* d0 > 0 */
  float w_bond;               /* >= 0, finite */
  float bond_length;          /* L > 0 */
  float strength;             /* lambda >= 0, finite */
  float ess_threshold;        /* in [0, 2] */
  int32_t t_min, t_max;       /* 0 <= t_min <= t_max <= T */
  int32_t every;              /* >= 1 */
  int32_t group_size;         /* N in [1, DIFFAB_STEER_MAX_GROUP], divides the rows */
  const int32_t* chain;       /* DEVICE (rows, K) */
  const int32_t* residue_idx; /* DEVICE (rows, K) */
  const uint8_t* residue_mask;/* DEVICE (rows, K), nullable = all */
  float* logw;                /* DEVICE (rows) */
  float* u_prev;              /* DEVICE (rows) */
  float* energy;              /* DEVICE (rows) */
  int32_t* ancestors;         /* DEVICE (T + 1, rows), nullable */
  void* scratch;              /* DEVICE DIFFAB_STEER_SCRATCH_BYTES(rows, K) */
} diffab_sample_steering;
/* Needs s->alpha_bar_sqrt.  Checked before anything is enqueued, DIFFAB_ERR_ARG: rows (d->B) not a multiple of
 * group_size; group_size < 1 or > DIFFAB_STEER_MAX_GROUP; a negative or non-finite weight or strength; a distance <= 0; ess_threshold
 * outside [0, 2]; t_min > t_max or either outside [0, T]; every < 1; null logw, u_prev, energy, scratch, chain or residue_idx; scratch
 * not 8-byte aligned; DIFFAB_FLAG_KEEP_STRUCTURE (the structure is not sampled). */
/* The options of one diffab_sample_loop_ex call.  struct_bytes lets the library refuse a caller built against another layout instead of
 * reading pointers from the wrong offsets. */
typedef struct {
  uint32_t struct_bytes;   /* sizeof(diffab_sample_options); anything else: DIFFAB_ERR_ARG, before any other field is read */
  int32_t n_ctx;           /* contexts in res_ctx / pair_ctx; 0 means B; read through ctx_of_row */
  const int32_t* ctx_of_row;                       /* host int32[B], NULL: one context per row */
  const uint32_t* allowed;                         /* device uint32[B*K], NULL: unconstrained */
  const diffab_sample_record* record;              /* NULL: no trajectory */
  const diffab_sample_steps* steps;                /* NULL: every step */
  const diffab_sample_guidance* guidance;          /* NULL: unguided */
  const diffab_sample_temperature* temperature;    /* NULL: untempered */
  const diffab_sample_steering* steering;          /* NULL: unsteered */
} diffab_sample_options;
#ifdef __cplusplus
static_assert(sizeof(diffab_sample_options) == 64, "diffab_sample_options: 2 x 32 bits and 7 pointers");
#else
_Static_assert(sizeof(diffab_sample_options) == 64, "diffab_sample_options: 2 x 32 bits and 7 pointers");
#endif
/* diffab_sample_loop with options: its 18 arguments, and `opt` before the stream.  opt == NULL and an opt that is zero except for
 * struct_bytes are exactly diffab_sample_loop (which is this call with NULL).  Every option is checked before anything is enqueued. */
int diffab_sample_loop_ex(const diffab_dims* d, const diffab_denoiser_weights* w, const diffab_sched* s, const diffab_igso3* rev_tab,
                          int64_t* seq, float* x, float* O, const float* res_ctx, const float* pair_ctx, const uint8_t* gen_mask,
                          uint64_t seed, int64_t first_patch, int32_t t_start, int32_t t_stop, void* workspace, size_t workspace_bytes,
                          uint32_t flags, const diffab_sample_options* opt, void* stream);
/* Teacher-forced pieces of the rule above, one launch each (the analogues of diffab_reverse_update_jump):
 * diffab_steer_energy: U (rows) fp32 at step t in [1, T] from x (rows, K, 3) and eps_hat; reads the potential's terms and tables of
 *   `steering` only.
 * diffab_steer_resample: the weight update, ESS and resampling of G groups of N rows with explicit uniforms u (G) fp32 in [0, 1): logw
 *   and u_prev (G N) are updated in place from energy (G N); ancestors_out (G N) int32, indices inside the group; ess_out (G) double,
 *   nullable (0 for a group with no weight).
 * diffab_steer_gather: seq / x / O of the generated residues of row j become those of row ancestors[j] (row indices of the call; an
 *   index outside [0, rows) leaves its row alone).  gen_mask of the DESTINATION row decides which residues are replaced; the residue of
 *   the source row is read whatever its own mask says.  scratch: rows K 56 B, 8-byte aligned.
 * DIFFAB_ERR_ARG: a null pointer (ess_out excepted), negative extents, N outside [1, DIFFAB_STEER_MAX_GROUP], the checks of
 * diffab_sample_options.steering on the values given. */
int diffab_steer_energy(const float* x, const float* eps_hat, const uint8_t* gen_mask, const diffab_sched* s, int32_t t,
                        const diffab_sample_steering* steering, int32_t rows, int32_t K, float* energy_out, void* stream);
int diffab_steer_resample(float* logw, float* u_prev, const float* energy, const float* u, int32_t G, int32_t N, float strength,
                          float ess_threshold, int32_t* ancestors_out, double* ess_out, void* stream);
int diffab_steer_gather(int64_t* seq, float* x, float* O, const uint8_t* gen_mask, const int32_t* ancestors, int32_t rows, int32_t K,
                        void* scratch, void* stream);

/* ---- design scoring (build-defined evaluator; reference objective diffab_pytorch.py:808-887) ----------------------------------------
 * Per-design diffusion losses over a timestep grid: the reference's training objective (_shared_step, :808-880, summed as `loss` at
 * :882-887) evaluated per design instead of as one batch mean at one random t per row.  Evaluated row q = ((r n_t) + j) n_draws + m is
 * design r (of n_designs; seq (n,K), x (n,K,3), O (n,K,3,3), gen_mask / res_mask (n,K), res_mask NULL = all true) forward-noised to
 * t_j = t_list[j] with draw m, then denoised against context ctx_of_design[r] of the n_ctx contexts in res_ctx (n_ctx,K,D) / pair_ctx
 * (n_ctx,K,K,C) (ctx_of_design: a HOST array of n_designs entries in [0, n_ctx); NULL = the identity, n_ctx must be n_designs).
 *   Noise: diffab_sample_init_noised's forward process (diffusion.py:105-135, 199-236, 262-294) and Philox lanes, patch first_design + r,
 *          counter step t_j, stream word STREAM_OPT_* + (m << 16): draw 0 is bitwise sample_init_noised(t_j, first_patch = first_design +
 *          r), and designs [lo, hi) scored with first_design = lo are bitwise that slice of the whole call.  Only generated residues are
 *          noised; DIFFAB_FLAG_KEEP_STRUCTURE / _SEQUENCE leave that modality un-noised.
 *   Denoiser: Denoiser.forward (:558-607) at beta = beta[t_j] per row, on every launch form the sampler has (the shared-context pair
 *          stream, fp16 pair planes built once per call for the n_ctx contexts, the patch-resident module launch where
 *          diffab_sample_loop_ex with a context map would take it).
 *   Terms, per residue with gen_mask & res_mask (0 elsewhere), the reference's element losses (:856-880 before reduction) summed over
 *          their trailing axes:  seq  sum_v q_v (log q_v - log p_v), q = q(s_{t-1} | s_t, s_0) (diffusion.py:168-192), p = softmax(logits);
 *          translations  sum_c (eps_hat - eps)^2;  orientations  sum_jk ((O0_hat^T O0) - I)^2_jk, O0_hat = O_t exp(hat(v_hat)) (:594-596,
 *          :610-625).  A kept modality's terms are exactly 0.
 *   out_terms (n_designs, n_t, n_draws, 3): each term summed over the row's masked residues / their count (0/0 = NaN for a row without
 *          one, as :868-878), reduced in a fixed order per row: independent of chunking, sharding and launch form.
 *   out_residue (nullable, (n_designs, n_t, n_draws, K, 3)): the per-residue terms.  noised (nullable, and each member nullable): the
 *          noised state of every row, for tests and debugging.
 * The rows run in chunks of d->B consecutive rows (d->B: rows per launch, not the total), all enqueued on `stream` with no host sync.
 * t_list is a HOST array of n_t distinct steps in [1, T] (n_t <= 1024); 1 <= n_draws <= 65536; d->V must be 21.  Every argument is
 * checked before anything is enqueued (DIFFAB_ERR_ARG / DIFFAB_ERR_WORKSPACE with a message).  workspace: diffab_score_workspace_bytes(d,
 * n_ctx) - sized by d->B and n_ctx, never by the number of designs, steps or draws. */
typedef struct {
  int64_t* seq_t; /* (n_designs, n_t, n_draws, K) */
  float* x_t;     /* (..., K, 3) */
  float* O_t;     /* (..., K, 3, 3) */
  float* eps;     /* (..., K, 3) the translation noise (0 where not noised) */
} diffab_score_noised;
size_t diffab_score_workspace_bytes(const diffab_dims* d, int32_t n_ctx);
int diffab_score_designs(const diffab_dims* d, const diffab_denoiser_weights* w, const diffab_sched* s, const diffab_igso3* fwd_tab,
                         const int64_t* seq, const float* x, const float* O, const uint8_t* gen_mask, const uint8_t* res_mask,
                         int32_t n_designs, const float* res_ctx, const float* pair_ctx, int32_t n_ctx, const int32_t* ctx_of_design,
                         const int32_t* t_list, int32_t n_t, int32_t n_draws, uint64_t seed, int64_t first_design, float* out_terms,
                         float* out_residue, const diffab_score_noised* noised, void* workspace, size_t workspace_bytes, uint32_t flags,
                         void* stream);

#ifdef __cplusplus
}
#endif
#endif /* DIFFAB_HIP_H */
