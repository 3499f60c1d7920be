"""ctypes binding of libdiffab_hip.so (C ABI: include/diffab_hip.h and include/diffab_hip_analysis.h).

torch is used here only as the owner of device memory and streams: every call
passes raw device pointers, sizes and the current HIP stream handle.  There is
no CPU or ATen fallback: if the library or a gfx950 device is missing, calls
raise ``HipUnavailable`` loudly.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Dict, Optional, Sequence

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
# DIFFAB_HIP_LIB: developer override used by tools/ and experiments/ to load another build of the same C ABI (ablations, variants)
LIB_PATH = os.environ.get("DIFFAB_HIP_LIB") or os.path.join(os.path.dirname(_HERE), "lib", "libdiffab_hip.so")

FLAG_FORCE_GENERIC = 1
FLAG_PAIR_F32 = 64  # sample_loop: keep the fp32 pair stream (no fp16 planes)
FLAG_FP32_GEMM = 128  # forward paths: dense products on the f32-input MFMA kernels instead of the bf16 split
FLAG_PAIR_PLANES = 32  # K = 64 / 128: pair embedding as two fp16 planes, pair-tile products on the f16 matrix cores (always on in sample_loop)
FLAG_GRAPH_SAMPLER = 16  # sample_loop: one captured step replayed as a hipGraph (launch-bound small batches)
FLAG_PERSISTENT_MODULE = 512  # MFMA path, K = 128 / 256, pair planes: the IPA module as one patch-resident launch (bitwise the multi-launch result)
FLAG_MULTI_LAUNCH = 1024  # sample_loop: never choose the patch-resident module launch (bitwise the same samples either way)
FLAG_SKIP_UNUSED_ROWS = 256  # sample_loop: accepted, no effect - the loop skips the last layer's unread row tiles by itself (same trajectory)
FLAG_ALL_ROWS = 8192  # sample_loop: run the last layer's attention for every row tile, also those without a generated residue (same trajectory)
FLAG_KEEP_STRUCTURE = 2048  # design mode: the sampler never writes x and O (fixed-backbone sequence design)
FLAG_KEEP_SEQUENCE = 4096  # design mode: the sampler never writes seq (structure prediction)


class HipUnavailable(RuntimeError):
    pass


class DiffabHipError(RuntimeError):
    pass


class Dims(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("B", "K", "D", "C", "H", "DS", "PQ", "PV", "NL", "V")]


_fp = C.c_void_p  # device pointers travel as void*


class IpaLayerWeights(C.Structure):
    _fields_ = [(n, _fp) for n in ("gamma", "wq_s", "wk_s", "wv_s", "w_bias", "wq_p", "wk_p", "wv_p", "w_out", "b_out")]


class Mlp3Weights(C.Structure):
    _fields_ = [(n, _fp) for n in ("w0", "b0", "w2", "b2", "w4", "b4")]


class DenoiserWeights(C.Structure):
    _fields_ = [
        ("seq_emb", _fp), ("res_w0", _fp), ("res_b0", _fp), ("res_w2", _fp), ("res_b2", _fp),
        ("layers", C.POINTER(IpaLayerWeights)),
        ("coord", Mlp3Weights), ("orient", Mlp3Weights), ("seq", Mlp3Weights),
    ]


class CtxDims(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("B", "K", "A", "D", "C", "max_dist")]


class ResidueEmbWeights(C.Structure):
    _fields_ = [(n, _fp) for n in ("aa_emb", "chain_emb", "w0", "b0", "w2", "b2", "w4", "b4", "w6", "b6")]


class PairEmbWeights(C.Structure):
    _fields_ = [(n, _fp) for n in ("aa_pair_emb", "relpos_emb", "pair2distcoef", "dw0", "db0", "dw2", "db2", "mw0", "mb0", "mw2", "mb2",
                                   "mw4", "mb4")]


class Sched(C.Structure):
    _fields_ = [("T", C.c_int32), ("alpha", _fp), ("alpha_bar", _fp), ("alpha_bar_sqrt", _fp),
                ("one_minus_alpha_bar_sqrt", _fp), ("beta", _fp)]


class Igso3(C.Structure):
    _fields_ = [("n_sigmas", C.c_int32), ("n_bins", C.c_int32), ("sigmas", _fp), ("cdf", _fp), ("sigma_threshold", C.c_float)]


class ScoreNoised(C.Structure):  # diffab_score_noised: optional copies of the noised state of every evaluated row
    _fields_ = [(n, _fp) for n in ("seq_t", "x_t", "O_t", "eps")]


class SampleRecord(C.Structure):  # diffab_sample_record: the recorded reverse trajectory (SampleOptions.record)
    _fields_ = [("n_slots", C.c_int32), ("slot_of_step", C.POINTER(C.c_int32)), ("slot_dev", _fp)] + \
        [(n, _fp) for n in ("seq", "x", "O", "pred_x", "pred_O", "seq_probs")]


class SampleSteps(C.Structure):  # diffab_sample_steps: the executed step list and its jump coefficients (SampleOptions.steps)
    _fields_ = [("n_steps", C.c_int32), ("steps", C.POINTER(C.c_int32)), ("beta_jump", C.POINTER(C.c_float)),
                ("alpha_jump", C.POINTER(C.c_float)), ("plan_dev", _fp)]


class SampleGuidance(C.Structure):  # diffab_sample_guidance: the clash / chain-bond potential (SampleOptions.guidance)
    _fields_ = [(n, C.c_float) for n in ("w_clash", "clash_distance", "w_bond", "bond_length", "max_shift")] + \
        [("t_max", C.c_int32)] + [(n, _fp) for n in ("chain", "residue_idx", "residue_mask", "shift_dev")]


class SampleTemperature(C.Structure):  # diffab_sample_temperature: per-row noise scales and sequence temperature (SampleOptions.temperature)
    _fields_ = [(n, _fp) for n in ("trans_scale", "rot_scale", "seq_temp", "rot_row")]


class SampleSteering(C.Structure):  # diffab_sample_steering: particle steering (SampleOptions.steering)
    _fields_ = [(n, C.c_float) for n in ("w_clash", "clash_distance", "w_bond", "bond_length", "strength", "ess_threshold")] + \
        [(n, C.c_int32) for n in ("t_min", "t_max", "every", "group_size")] + \
        [(n, _fp) for n in ("chain", "residue_idx", "residue_mask", "logw", "u_prev", "energy", "ancestors", "scratch")]


class SampleOptions(C.Structure):
    """diffab_sample_options: the options of one diffab_sample_loop_ex call, by keyword (what is left out is off); struct_bytes is
    filled in here.  The structure keeps the Python objects its pointer fields were given alive, not the device memory behind them."""
    _fields_ = [("struct_bytes", C.c_uint32), ("n_ctx", C.c_int32), ("ctx_of_row", C.POINTER(C.c_int32)), ("allowed", _fp),
                ("record", C.POINTER(SampleRecord)), ("steps", C.POINTER(SampleSteps)), ("guidance", C.POINTER(SampleGuidance)),
                ("temperature", C.POINTER(SampleTemperature)), ("steering", C.POINTER(SampleSteering))]

    def __init__(self, **options):
        for name in ("record", "steps", "guidance", "temperature", "steering"):  # a structure (or None) where the field is a pointer
            if isinstance(options.get(name), C.Structure):
                options[name] = C.pointer(options[name])
        super().__init__(struct_bytes=C.sizeof(type(self)), **{k: v for k, v in options.items() if v is not None})


class RefineOptions(C.Structure):
    """diffab_refine_options: iterations, step, the five weights and the clash distance of diffab_refine_backbone; struct_bytes is filled
    in here."""
    _fields_ = [("struct_bytes", C.c_uint32), ("iterations", C.c_int32)] + \
        [(n, C.c_float) for n in ("step", "w_bond", "w_angle", "w_trans", "w_clash", "w_tether", "clash_distance")]

    def __init__(self, *args, **kw):
        super().__init__(C.sizeof(type(self)), *args, **kw)


# every symbol include/diffab_hip.h declares: name -> (restype, argtypes)
_i32, _i64, _u32, _u64, _sz = C.c_int32, C.c_int64, C.c_uint32, C.c_uint64, C.c_size_t
_PD, _PS, _PI = C.POINTER(Dims), C.POINTER(Sched), C.POINTER(Igso3)
SYMBOLS = {
    "diffab_version": (C.c_char_p, []),
    "diffab_last_error": (C.c_char_p, []),
    "diffab_device_ok": (C.c_int, []),
    "diffab_kernel_timer_enable": (C.c_int, [C.c_int]),
    "diffab_debug_set_attn_stamps": (C.c_int, [_fp]),
    "diffab_debug_set_attn_variant": (C.c_int, [_i32]),
    "diffab_debug_set_module_stagger": (C.c_int, [_i32, _i32]),
    "diffab_debug_set_module_stamps": (C.c_int, [_fp]),
    "diffab_debug_row_tiles": (C.c_int, [_fp, _i32, _i32, _fp, _fp]),
    "diffab_debug_row_plan": (C.c_int, [_fp, _i32, _i32, _fp, _fp]),
    "diffab_set_stream_guard": (C.c_int, [C.c_int]),
    "diffab_debug_linear128": (C.c_int, [_fp, _fp, _fp, _fp, C.c_int64, C.c_int32, C.c_int32, _fp, C.c_size_t, _fp]),
    "diffab_debug_gemm_tn": (C.c_int, [_fp, _fp, _fp, _fp, C.c_int64, C.c_int32, C.c_int32, C.c_int32, _fp]),
    "diffab_debug_xstat128": (C.c_int, [_fp, _fp, _fp, C.c_int64, C.c_int32, C.c_int32, _fp, C.c_size_t, _fp]),
    "diffab_debug_dense_forms": (C.c_int, [C.c_int64, C.c_int32, C.c_int32, C.POINTER(C.c_int32)]),
    "diffab_kernel_timer_read": (C.c_int, [C.POINTER(C.c_int64), C.POINTER(C.c_double)]),
    "diffab_so3_log": (C.c_int, [_fp, _fp, _i64, _fp]),
    "diffab_so3_exp": (C.c_int, [_fp, _fp, _i64, _fp]),
    "diffab_so3_matrix_to_rotvec": (C.c_int, [_fp, _fp, _i64, _fp]),
    "diffab_so3_rotvec_to_matrix": (C.c_int, [_fp, _fp, _i64, _fp]),
    "diffab_so3_scale_rot": (C.c_int, [_fp, _fp, _fp, _i64, _i64, _fp]),
    "diffab_igso3_table_build": (C.c_int, [_fp, _i32, _i32, _i32, _fp, _fp]),
    "diffab_igso3_table_build_accurate": (C.c_int, [_fp, _i32, _i32, _i32, _fp, _fp]),
    "diffab_igso3_cdf_build": (C.c_int, [_fp, _i32, _i32, _fp, _fp]),
    "diffab_igso3_sample": (C.c_int, [_PI, _fp, _i32, _i32, _fp, _fp, _fp, _fp, _fp, _fp]),
    "diffab_igso3_bins_without_replacement": (C.c_int, [_fp, _i32, _i32, _fp, _i32, _i32, _fp, _fp, _fp, C.c_float, _fp]),
    "diffab_igso3_sample_bins": (C.c_int, [_PI, _fp, _i32, _i32, _fp, _fp, _fp, _fp, _fp, _fp]),
    "diffab_weighted_multinomial": (C.c_int, [_fp, _fp, _fp, _fp, _i64, _i64, _fp, _fp]),
    "diffab_seq_forward_prob": (C.c_int, [_PS, C.c_int, _fp, _fp, _fp, _i32, _i32, _fp, _fp]),
    "diffab_seq_posterior": (C.c_int, [_PS, _fp, _fp, _fp, _fp, _i32, _i32, _fp, _fp]),
    "diffab_categorical_sample": (C.c_int, [_fp, _fp, _i64, _i32, _fp, _fp]),
    "diffab_coord_forward": (C.c_int, [_PS, _fp, _fp, _fp, _fp, _i32, _i32, _fp, _fp]),
    "diffab_orient_forward": (C.c_int, [_PS, _fp, _fp, _fp, _fp, _i32, _i32, _fp, _fp]),
    "diffab_philox_fill": (C.c_int, [_u64, _i64, _i32, _i32, _i32, _i32, C.c_int, _fp, _fp]),
    "diffab_denoise_workspace_bytes": (_sz, [_PD]),
    "diffab_sample_workspace_bytes": (_sz, [_PD]),
    "diffab_sample_shared_workspace_bytes": (_sz, [_PD, _i32]),
    "diffab_ipa_layer_fwd": (C.c_int, [_PD, C.POINTER(IpaLayerWeights), _fp, _fp, _fp, _fp, _fp, _fp, _sz, _u32, _fp]),
    "diffab_denoise_step_fwd": (C.c_int, [_PD, C.POINTER(DenoiserWeights), _fp, _fp, _fp, _fp, _fp, _fp, _fp, _fp, _fp, _fp, _fp,
                                          _fp, _sz, _u32, _fp]),
    "diffab_losses_fwd": (C.c_int, [_fp, _fp, _fp, _fp, _fp, _fp, _fp, _fp, _i32, _i32, _i32, _fp, _fp]),
    "diffab_train_tape_bytes": (_sz, [_PD]),
    "diffab_train_workspace_bytes": (_sz, [_PD]),
    "diffab_train_step_fwd": (C.c_int, [_PD, C.POINTER(DenoiserWeights)] + [_fp] * 16 + [_sz, _u32, _fp]),
    "diffab_train_step_bwd": (C.c_int, [_PD, C.POINTER(DenoiserWeights), C.POINTER(DenoiserWeights)] + [_fp] * 16 + [_sz, _fp, _sz, _fp]),
    "diffab_residue_embedding_workspace_bytes": (_sz, [C.POINTER(CtxDims)]),
    "diffab_residue_embedding_fwd": (C.c_int, [C.POINTER(CtxDims), C.POINTER(ResidueEmbWeights)] + [_fp] * 10 + [_sz, _fp]),
    "diffab_pair_embedding_workspace_bytes": (_sz, [C.POINTER(CtxDims)]),
    "diffab_pair_embedding_fwd": (C.c_int, [C.POINTER(CtxDims), C.POINTER(PairEmbWeights), _fp, _fp, _fp, _fp, _i32, _fp, _fp, _fp, _fp,
                                            _fp, _sz, _fp]),
    "diffab_pair_embedding_xyz_fwd": (C.c_int, [C.POINTER(CtxDims), C.POINTER(PairEmbWeights), _fp, _fp, _fp, _fp, _i32, _fp, _fp, _fp, _fp,
                                                _fp, _sz, _fp]),
    "diffab_residue_embedding_bwd_workspace_bytes": (_sz, [C.POINTER(CtxDims)]),
    "diffab_residue_embedding_bwd": (C.c_int, [C.POINTER(CtxDims), C.POINTER(ResidueEmbWeights), C.POINTER(ResidueEmbWeights)] + [_fp] * 10
                                     + [_sz, _fp]),
    "diffab_pair_embedding_bwd_workspace_bytes": (_sz, [C.POINTER(CtxDims)]),
    "diffab_pair_embedding_bwd": (C.c_int, [C.POINTER(CtxDims), C.POINTER(PairEmbWeights), C.POINTER(PairEmbWeights), _fp, _fp, _fp, _fp, _fp,
                                            _i32, _fp, _fp, _fp, _fp, _fp, _sz, _fp]),
    "diffab_pair_embedding_tape_bytes": (_sz, [C.POINTER(CtxDims)]),
    # (d, w, seq, distmat, xyz, pdih, resid, stride, chain, amask, mask, out, tape, tape_bytes, ws, ws_bytes, stream)
    "diffab_pair_embedding_fwd_taped": (C.c_int, [C.POINTER(CtxDims), C.POINTER(PairEmbWeights), _fp, _fp, _fp, _fp, _fp, _i32, _fp, _fp, _fp,
                                                  _fp, _fp, _sz, _fp, _sz, _fp]),
    # (d, w, g, seq, distmat, xyz, pdih, resid, stride, chain, amask, mask, d_out, tape, tape_bytes, ws, ws_bytes, stream)
    "diffab_pair_embedding_bwd_taped": (C.c_int, [C.POINTER(CtxDims), C.POINTER(PairEmbWeights), C.POINTER(PairEmbWeights), _fp, _fp, _fp, _fp,
                                                  _fp, _i32, _fp, _fp, _fp, _fp, _fp, _sz, _fp, _sz, _fp]),
    "diffab_featurize_xyz": (C.c_int, [_fp, _fp, _fp, _i32, _i32, _i32, _fp, _fp, _fp, _fp, _fp]),
    # (ca, ca_stride, residue_mask, generation_mask, anchor_mask, chain_idx, antigen_mask, B, N, k, k_antigen, K, index, patch_mask, count, stream)
    "diffab_patch_select": (C.c_int, [_fp, _i32, _fp, _fp, _fp, _fp, _fp, _i32, _i32, _i32, _i32, _i32, _fp, _fp, _fp, _fp]),
    # (src, index, complex_of_row (host int32[rows], nullable), B, N, rows, K, row_bytes, dst, stream)
    "diffab_patch_gather": (C.c_int, [_fp, _fp, C.POINTER(_i32), _i32, _i32, _i32, _i32, _i64, _fp, _fp]),
    # (patch, index, write_mask (nullable), rows, N, K, row_bytes, dst, stream)
    "diffab_patch_scatter": (C.c_int, [_fp, _fp, _fp, _i32, _i32, _i32, _i64, _fp, _fp]),
    # (seq_idx, points, native_seq_idx, native_points, generation_mask, residue_mask (nullable), segment_idx (nullable), rows, group_size, K, P, S,
    #  aar, rmsd, rmsd_aligned, segment_aar, segment_rmsd, segment_rmsd_aligned, stream)
    "diffab_metrics_vs_native": (C.c_int, [_fp] * 7 + [_i32] * 5 + [_fp] * 7),
    # (seq_idx, points, generation_mask, residue_mask (nullable), G, N, K, P, aligned, rmsd, seq_identity, workspace, workspace_bytes, stream)
    "diffab_metrics_pairwise": (C.c_int, [_fp] * 4 + [_i32] * 5 + [_fp, _fp, _fp, _sz, _fp]),
    # (dist, score (nullable), candidates (nullable), G, N, m, index, min_dist, count, stream)
    "diffab_metrics_select_diverse": (C.c_int, [_fp, _fp, _fp, _i32, _i32, _i32, _fp, _fp, _fp, _fp]),
    # (points, generation_mask, residue_mask (nullable), chain, residue_idx, rows, group_size, K, bond_tolerance, phi, psi, omega, peptide_bond,
    #  n_bonds, max_peptide_deviation, n_chain_break, n_cis, workspace, workspace_bytes, stream)
    "diffab_metrics_backbone": (C.c_int, [_fp] * 5 + [_i32] * 3 + [C.c_float] + [_fp] * 9 + [_sz, _fp]),
    # (points, valid, context_points, context_valid, generation_mask, residue_mask (nullable), antigen_mask (nullable), hotspot_mask (nullable),
    #  chain, residue_idx, rows, group_size, K, P, A, clash_distance, contact_distance, n_clash, clash_score, min_distance, n_contact_pairs,
    #  n_paratope, n_epitope, n_hotspot_contacted, n_hotspot, residue_clash, residue_contact, workspace, workspace_bytes, stream)
    "diffab_metrics_contacts": (C.c_int, [_fp] * 10 + [_i32] * 5 + [C.c_float] * 2 + [_fp] * 11 + [_sz, _fp]),
    # (seq_idx, points, generation_mask, residue_mask (nullable), weights (nullable), G, N, K, P, V, pseudocount, aa_freq, entropy, consensus,
    #  mean_points, rmsf, log_prob, consensus_identity, rmsd_to_mean, n_eff, central (each nullable), workspace, workspace_bytes, stream)
    "diffab_metrics_ensemble": (C.c_int, [_fp] * 5 + [_i32] * 5 + [C.c_double] + [_fp] * 11 + [_sz, _fp]),
    # (points, native_points, generation_mask, residue_mask (nullable), antigen_mask (nullable), segment_idx (nullable), chain (nullable),
    #  residue_idx (nullable), rows, group_size, K, P, S, inclusion_radius, contact_distance, n_pairs, n_pairs_interface, preserved,
    #  preserved_interface, lddt_residue, lddt, lddt_thresholds, ilddt_residue, ilddt, lddt_segment, n_native, native_contacts_residue, n_design,
    #  n_kept, fnat, fnonnat, kept_residue, stream)
    "diffab_metrics_similarity": (C.c_int, [_fp] * 8 + [_i32] * 5 + [C.c_float] * 2 + [_fp] * 18),
    # (translations, orientations, generation_mask, residue_mask (nullable), chain, residue_idx, rows, group_size, K, options (nullable),
    #  out_translations, out_orientations, energy_before, energy_after, terms_after, max_shift (the last four nullable), workspace,
    #  workspace_bytes, stream)
    "diffab_refine_backbone": (C.c_int, [_fp] * 6 + [_i32] * 3 + [C.POINTER(RefineOptions)] + [_fp] * 6 + [_fp, _sz, _fp]),
    "diffab_orientation_loss": (C.c_int, [_fp, _fp, _i64, _fp, _fp, _fp]),
    "diffab_orientation_loss_bwd": (C.c_int, [_fp, _fp, _i64, _fp, _fp, _fp, _fp, _fp]),
    "diffab_frames_apply": (C.c_int, [_fp, _fp, _fp, _fp, _i32, _i32, _i32, _i32, _fp]),
    "diffab_frames_invert": (C.c_int, [_fp, _fp, _fp, _fp, _i32, _i32, _i32, _i32, _fp]),
    "diffab_frames_bwd": (C.c_int, [_fp, _fp, _fp, _fp, _i32, _fp, _fp, _i32, _i32, _i32, _i32, _fp]),
    "diffab_angular_encoding": (C.c_int, [_fp, _i64, _i32, _fp, _fp]),
    "diffab_angular_encoding_bwd": (C.c_int, [_fp, _fp, _i64, _i32, _fp, _fp]),
    "diffab_denoise_step_fwd_taped": (C.c_int, [_PD, C.POINTER(DenoiserWeights)] + [_fp] * 10 + [_sz, _u32, _fp]),
    "diffab_denoise_step_bwd": (C.c_int, [_PD, C.POINTER(DenoiserWeights), C.POINTER(DenoiserWeights)] + [_fp] * 13 + [_sz, _fp, _sz, _fp]),
    "diffab_ipa_layer_tape_bytes": (_sz, [_PD]),
    "diffab_ipa_layer_bwd_workspace_bytes": (_sz, [_PD]),
    "diffab_ipa_layer_fwd_taped": (C.c_int, [_PD, C.POINTER(IpaLayerWeights), _fp, _fp, _fp, _fp, _fp, _fp, _sz, _u32, _fp]),
    "diffab_ipa_layer_bwd": (C.c_int, [_PD, C.POINTER(IpaLayerWeights), C.POINTER(IpaLayerWeights), _fp, _fp, _fp, _fp, _fp, _fp, _fp, _fp, _fp,
                                       _sz, _fp, _sz, _fp]),
    "diffab_reverse_update": (C.c_int, [_PS, _i32, _fp, _fp, _fp, _fp, _fp, _fp, _fp, _fp, _fp, _fp, _i32, _i32, _i32, _fp]),
    "diffab_sample_loop": (C.c_int, [_PD, C.POINTER(DenoiserWeights), _PS, _PI, _fp, _fp, _fp, _fp, _fp, _fp, _u64, _i64, _i32,
                                     _i32, _fp, _sz, _u32, _fp]),
    # diffab_sample_loop's arguments plus the options (nullable) before the stream
    "diffab_sample_loop_ex": (C.c_int, [_PD, C.POINTER(DenoiserWeights), _PS, _PI, _fp, _fp, _fp, _fp, _fp, _fp, _u64, _i64, _i32,
                                        _i32, _fp, _sz, _u32, C.POINTER(SampleOptions), _fp]),
    "diffab_sample_init": (C.c_int, [_fp, _fp, _fp, _fp, _u64, _i64, _i32, _i32, _i32, _fp]),
    # (seq, x, O, gen_mask, seed, first_patch, B, K, T, flags, allowed (device uint32[B*K], nullable), stream)
    "diffab_sample_init_ex": (C.c_int, [_fp, _fp, _fp, _fp, _u64, _i64, _i32, _i32, _i32, _u32, _fp, _fp]),
    # (sched, fwd_tab, seq, x, O, gen_mask, seed, first_patch, B, K, t, flags, allowed (nullable), stream)
    "diffab_sample_init_noised": (C.c_int, [_PS, _PI, _fp, _fp, _fp, _fp, _u64, _i64, _i32, _i32, _i32, _u32, _fp, _fp]),
    # (x, eps_hat, gen_mask, sched, t, steering, rows, K, energy_out, stream)
    "diffab_steer_energy": (C.c_int, [_fp, _fp, _fp, _PS, _i32, C.POINTER(SampleSteering), _i32, _i32, _fp, _fp]),
    # (logw, u_prev, energy, u, G, N, strength, ess_threshold, ancestors_out, ess_out (double, nullable), stream)
    "diffab_steer_resample": (C.c_int, [_fp, _fp, _fp, _fp, _i32, _i32, C.c_float, C.c_float, _fp, _fp, _fp]),
    # (seq, x, O, gen_mask, ancestors, rows, K, scratch, stream)
    "diffab_steer_gather": (C.c_int, [_fp, _fp, _fp, _fp, _fp, _i32, _i32, _fp, _fp]),
    # (x, gen_mask, guidance, B, K, clash, bond, n_clash, max_bond_deviation, grad (nullable), stream)
    "diffab_guidance_energy": (C.c_int, [_fp, _fp, C.POINTER(SampleGuidance), _i32, _i32, _fp, _fp, _fp, _fp, _fp, _fp]),
    # (sched, t, s, beta', alpha', seq, x, O, eps_hat, O0_hat, posterior, gen_mask, z, rotvec, u_seq, r_out (nullable), B, K, V, stream)
    "diffab_reverse_update_jump": (C.c_int, [_PS, _i32, _i32, C.c_float, C.c_float, _fp, _fp, _fp, _fp, _fp, _fp, _fp, _fp, _fp, _fp, _fp,
                                             _i32, _i32, _i32, _fp]),
    "diffab_score_workspace_bytes": (_sz, [_PD, _i32]),
    # (d, w, sched, fwd_tab, seq, x, O, gen_mask, res_mask, n_designs, res_ctx, pair_ctx, n_ctx, ctx_of_design (host int32[n_designs]),
    #  t_list (host int32[n_t]), n_t, n_draws, seed, first_design, out_terms, out_residue, noised, ws, ws_bytes, flags, stream)
    "diffab_score_designs": (C.c_int, [_PD, C.POINTER(DenoiserWeights), _PS, _PI, _fp, _fp, _fp, _fp, _fp, _i32, _fp, _fp, _i32,
                                       C.POINTER(_i32), C.POINTER(_i32), _i32, _i32, _u64, _i64, _fp, _fp, C.POINTER(ScoreNoised), _fp, _sz,
                                       _u32, _fp]),
}

# every symbol include/diffab_hip_analysis.h declares (the model-free analysis entries added after the export list of diffab_hip.h was
# pinned): same library, same conventions, a table of its own
ANALYSIS_SYMBOLS = {
    # (points, valid, point_radius (HOST float[P]), context_points, context_valid, context_radius (nullable), generation_mask,
    #  residue_mask (nullable), antigen_mask (nullable), hotspot_mask (nullable), sphere, rows, group_size, K, P, A, S, probe,
    #  context_radius_default, free_points, bound_points, design_buried_points, free_area, bound_area, design_buried_area, residue_buried,
    #  bsa_paratope, bsa_epitope, bsa_design_epitope, n_paratope_buried, n_epitope_buried, n_hotspot, n_hotspot_buried,
    #  hotspot_buried_area (each output nullable), workspace, workspace_bytes, stream)
    "diffab_metrics_surface": (C.c_int, [_fp, _fp, C.POINTER(C.c_float)] + [_fp] * 8 + [_i32] * 6 + [C.c_float] * 2 + [_fp] * 15
                               + [_fp, _sz, _fp]),
}

# every symbol include/diffab_hip_hbonds.h declares (both export lists above are pinned by their tests): same library, a third table
HBOND_SYMBOLS = {
    # (points, donor_off, context_points, context_valid, context_donor_off, generation_mask, residue_mask (nullable), antigen_mask
    #  (nullable), hotspot_mask (nullable), chain, residue_idx, rows, group_size, K, A, O, H, nh_o_partner, nh_o_energy, o_hn_partner,
    #  o_hn_energy, bridge_partner, bridge_parallel, ss, residue_hbonds, n_hbonds, n_hbonds_internal, n_hbonds_antigen, n_hbonds_framework,
    #  n_hotspot_bonded, n_hotspot, hbond_energy, ss_count (each output nullable), workspace, workspace_bytes, stream)
    "diffab_metrics_hbonds": (C.c_int, [_fp] * 11 + [_i32] * 4 + [_fp] * 18 + [_fp, _sz, _fp]),
}

# every symbol include/diffab_hip_cluster.h declares (the three export lists above are pinned by their tests): same library, a fourth
# table, open to the next entry that reads a patch's pairwise matrix
CLUSTER_SYMBOLS = {
    # (dist, cutoff (G) device, score (nullable), candidates (nullable), G, N, M, label, center_dist (nullable), center, size, count,
    #  n_unassigned (nullable), workspace, workspace_bytes, stream)
    "diffab_metrics_cluster": (C.c_int, [_fp] * 4 + [_i32] * 3 + [_fp] * 6 + [_fp, _sz, _fp]),
    # (objectives, maximize (M) device (nullable), violation (nullable), score (nullable), candidates (nullable), G, N, M, F, rank,
    #  n_dominators (nullable), n_dominated (nullable), front_size, count, n_unranked (nullable), order (nullable), workspace,
    #  workspace_bytes, stream)
    "diffab_metrics_pareto": (C.c_int, [_fp] * 5 + [_i32] * 4 + [_fp] * 7 + [_fp, _sz, _fp]),
}

# every symbol include/diffab_hip_interface.h declares (the four export lists above are pinned by their tests, and the cluster header's
# test allows no float parameter): same library, a fifth table, for the entries that produce or compare packed bit sets per design
INTERFACE_SYMBOLS = {
    # (points, valid, context_points, context_valid, generation_mask, residue_mask (nullable), antigen_mask, chain, residue_idx, rows,
    #  group_size, K, P, A, contact_distance, bits, n_contacts, workspace, workspace_bytes, stream)
    "diffab_metrics_contact_bits": (C.c_int, [_fp] * 9 + [_i32] * 5 + [C.c_float] + [_fp] * 2 + [_fp, _sz, _fp]),
    # (bits, G, N, L, n_set, n_common, fcc, jaccard (each output nullable), workspace, workspace_bytes, stream)
    "diffab_metrics_pairwise_bits": (C.c_int, [_fp] + [_i32] * 3 + [_fp] * 4 + [_fp, _sz, _fp]),
}

# every symbol include/diffab_hip_develop.h declares (the five export lists above are pinned by their tests): same library, a sixth
# table, for the entries that read a design's coordinates and its sequence together
DEVELOP_SYMBOLS = {
    # (sites, context_sites, tokens, generation_mask, residue_mask (nullable), antigen_mask (nullable), exposed_in (nullable),
    #  hydrophobicity, charge, rows, group_size, K, V, neighbour_distance, max_neighbours, vicinity_distance, patch_distance, min_distance,
    #  psh, ppc, pnc, charge_generated, charge_scope, n_scope, n_exposed, n_pairs, residue_psh, residue_ppc, residue_pnc, n_neighbours,
    #  state (each output nullable), workspace, workspace_bytes, stream)
    "diffab_metrics_patches": (C.c_int, [_fp] * 9 + [_i32] * 4 + [C.c_float, _i32] + [C.c_float] * 3 + [_fp] * 13 + [_fp, _sz, _fp]),
    # (tokens, generation_mask, residue_mask (nullable), chain, residue_idx, motifs (HOST int32[M * 4]), rows, group_size, K, M,
    #  motif_count, n_motifs, motif_start (each output nullable), workspace, workspace_bytes, stream)
    "diffab_metrics_motifs": (C.c_int, [_fp] * 6 + [_i32] * 4 + [_fp] * 3 + [_fp, _sz, _fp]),
}

# every symbol include/diffab_hip_energy.h declares (the six export lists above are pinned by their tests): same library, a seventh
# table, for the entry that scores a designed residue against the residue it touches by what the two residues are
ENERGY_SYMBOLS = {
    # (sites, context_sites, tokens, generation_mask, residue_mask (nullable), antigen_mask (nullable), chain, residue_idx (both or
    #  neither), table, bin_edges (HOST float[NB + 1]), rows, group_size, K, V, NB, min_separation, e_antigen, e_framework, e_internal,
    #  n_pairs, residue_energy, residue_antigen_energy, n_partners, substitution (each output nullable), workspace, workspace_bytes, stream)
    "diffab_metrics_pair_energy": (C.c_int, [_fp] * 10 + [_i32] * 6 + [_fp] * 8 + [_fp, _sz, _fp]),
}

# every symbol include/diffab_hip_novelty.h declares (the seven export lists above are pinned by their tests): same library, an eighth
# table, for the entries that compare a design with sequences outside its patch
NOVELTY_SYMBOLS = {
    # (q_tokens, q_len, R, LQ, lib_tokens, lib_len, M, LM, skip (nullable), radius, distance, index, n_within, identity, matrix (each
    #  output nullable), workspace, workspace_bytes, stream)
    "diffab_metrics_edit_nearest": (C.c_int, [_fp, _fp, _i32, _i32, _fp, _fp, _i32, _i32, _fp, _i32] + [_fp] * 5 + [_fp, _sz, _fp]),
    # (tokens, mask, residue_mask (nullable), segment_idx (nullable), segment, rows, group_size, K, L, out_tokens, out_len, stream)
    "diffab_metrics_pack_sequences": (C.c_int, [_fp] * 4 + [_i32] * 5 + [_fp] * 2 + [_fp]),
}

# every symbol include/diffab_hip_conformation.h declares (the eight export lists above are pinned by their tests): same library, a ninth
# table, for the entries that compare the shape of a design with loops outside its patch
CONFORMATION_SYMBOLS = {
    # (q_feat, q_len, R, LQ, lib_feat, lib_len, M, LM, A, skip (nullable), radius, min_terms, distance, index, n_terms, n_within, matrix
    #  (each output nullable), workspace, workspace_bytes, stream)
    "diffab_metrics_dihedral_nearest": (C.c_int, [_fp, _fp, _i32, _i32, _fp, _fp, _i32, _i32, _i32, _fp, C.c_float, _i32] + [_fp] * 5
                                        + [_fp, _sz, _fp]),
    # (phi, psi, omega, mask, residue_mask (nullable), segment_idx (nullable), segment, rows, group_size, K, L, out_angles, out_len, stream)
    "diffab_metrics_pack_dihedrals": (C.c_int, [_fp] * 6 + [_i32] * 5 + [_fp] * 2 + [_fp]),
}

_lib: Optional[C.CDLL] = None


def load_library() -> C.CDLL:
    """dlopen libdiffab_hip.so and type every declared symbol.  Needs no GPU."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise HipUnavailable(
                f"{LIB_PATH} is missing - build it with `make -C diffab-pytorch_amd/csrc` "
                "(or __graft_entry__.build()); there is no CPU fallback for this path")
        lib = C.CDLL(LIB_PATH)
        for name, (res, args) in (list(SYMBOLS.items()) + list(ANALYSIS_SYMBOLS.items()) + list(HBOND_SYMBOLS.items())
                                   + list(CLUSTER_SYMBOLS.items()) + list(INTERFACE_SYMBOLS.items()) + list(DEVELOP_SYMBOLS.items())
                                   + list(ENERGY_SYMBOLS.items()) + list(NOVELTY_SYMBOLS.items()) + list(CONFORMATION_SYMBOLS.items())):
            fn = getattr(lib, name)  # AttributeError if a header and the library drift apart
            fn.restype, fn.argtypes = res, args
        _lib = lib
    return _lib


_device_checked = False


def lib() -> C.CDLL:
    """The library, after checking that a gfx950 device is usable (compute calls only)."""
    global _device_checked
    l = load_library()
    if not _device_checked:
        if not torch.cuda.is_available() or not l.diffab_device_ok():
            raise HipUnavailable("no gfx950 (MI355X) device visible: the DiffAb hot path runs on HIP only")
        _device_checked = True
    return l


def check(rc: int, what: str) -> None:
    if rc != 0:
        raise DiffabHipError(f"{what} failed (code {rc}): {load_library().diffab_last_error().decode()}")


def stream_ptr() -> C.c_void_p:
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def device() -> torch.device:
    return torch.device("cuda", torch.cuda.current_device())


def ptr(t: Optional[torch.Tensor]) -> C.c_void_p:
    return C.c_void_p(0 if t is None else t.data_ptr())


def aligned16(t: torch.Tensor) -> torch.Tensor:
    """`t` itself when its storage starts on a 16-byte boundary, else a copy in an allocation of its own (which does).  A contiguous view
    can start anywhere - a parameter inside a flat parameter vector, a batch slice at a ragged patch length - and the library's vector
    kernels refuse such a float operand (include/diffab_hip.h, "Operand alignment"); the front end never does."""
    return t if t.data_ptr() % 16 == 0 else t.clone(memory_format=torch.contiguous_format)


def dev_f32(t: torch.Tensor) -> torch.Tensor:
    """float32, contiguous, 16-byte aligned, on the current HIP device (copying only if needed).  Read-only use: what the library writes
    goes to tensors the front end allocates itself."""
    return aligned16(t.detach().to(device=device(), dtype=torch.float32).contiguous())


def dev_i64(t: torch.Tensor) -> torch.Tensor:
    return t.detach().to(device=device(), dtype=torch.int64).contiguous()


def dev_mask(t: torch.Tensor) -> torch.Tensor:
    return t.detach().to(device=device()).ne(0).contiguous()  # torch.bool, 1 byte per element


def make_dims(B, K, D, C_, H, DS, PQ, PV, NL, V=21) -> Dims:
    return Dims(int(B), int(K), int(D), int(C_), int(H), int(DS), int(PQ), int(PV), int(NL), int(V))


def workspace(nbytes: int) -> torch.Tensor:
    # torch's caching allocator owns the buffer; it is stream-ordered with the launches that use it.
    return torch.empty(max(int(nbytes), 256), dtype=torch.uint8, device=device())


class SchedOnDevice:
    """The five schedule tables (host-computed, see diffusion.cosine_variance_schedule) uploaded once per device."""

    def __init__(self, sched: Dict[str, torch.Tensor]):
        self.T = int(sched["beta"].numel() - 1)
        self.tensors = {k: dev_f32(v) for k, v in sched.items()}
        t = self.tensors
        self.struct = Sched(self.T, ptr(t["alpha"]), ptr(t["alpha_bar"]), ptr(t["alpha_bar_sqrt"]),
                            ptr(t["one_minus_alpha_bar_sqrt"]), ptr(t["beta"]))


def ipa_layer_weights(params: Dict[str, torch.Tensor], keep: list) -> IpaLayerWeights:
    """params: the layer's own named parameters (reference names, diffab_pytorch.py:354-379)."""
    order = ("gamma", "to_q_scalar.weight", "to_k_scalar.weight", "to_v_scalar.weight", "to_pair_bias.weight",
             "to_q_point.weight", "to_k_point.weight", "to_v_point.weight", "to_out.weight", "to_out.bias")
    # (a layer built with use_pair_bias=False has no to_pair_bias: NULL in the struct, C = 0 in its dims)
    ts = [dev_f32(params[k]) if k in params else None for k in order]
    keep.extend(t for t in ts if t is not None)
    return IpaLayerWeights(*[ptr(t) for t in ts])


def mlp3_weights(params: Dict[str, torch.Tensor], prefix: str, keep: list) -> Mlp3Weights:
    ts = [dev_f32(params[prefix + k]) for k in ("0.weight", "0.bias", "2.weight", "2.bias", "4.weight", "4.bias")]
    keep.extend(ts)
    return Mlp3Weights(*[ptr(t) for t in ts])


class DenoiserWeightsOnDevice:
    """Pointer table over a Denoiser's parameters.  No copies when they live on the device and start on 16-byte boundaries (every
    parameter with an allocation of its own); a parameter that is a misaligned view - behind the 3-wide coordinate_denoising.4.bias of
    a flat parameter vector, 12 of the 43 - is copied for the call (dev_f32), on every call."""

    def __init__(self, params: Dict[str, torch.Tensor], n_layers: int):
        self.keep: list = []
        g = lambda k: dev_f32(params[k])
        base = [g(k) for k in ("sequence_embedding.weight", "to_res_emb.0.weight", "to_res_emb.0.bias", "to_res_emb.2.weight",
                               "to_res_emb.2.bias")]
        self.keep.extend(base)
        self.layers = (IpaLayerWeights * max(n_layers, 1))()
        for l in range(n_layers):
            pre = f"ipa.layers.{l}."
            sub = {k[len(pre):]: v for k, v in params.items() if k.startswith(pre)}
            self.layers[l] = ipa_layer_weights(sub, self.keep)
        self.struct = DenoiserWeights(
            *[ptr(t) for t in base], C.cast(self.layers, C.POINTER(IpaLayerWeights)),
            mlp3_weights(params, "coordinate_denoising.", self.keep),
            mlp3_weights(params, "orientation_denoising.", self.keep),
            mlp3_weights(params, "sequence_denoising.", self.keep),
        )
