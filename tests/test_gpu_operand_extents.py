"""What an entry may do to its data operands (include/diffab_hip.h, "Operand extents"): it writes only the operands its prototype marks
as written, only inside their extent, leaves const operands unchanged to the bit, and no value read past the end of an operand reaches a
result.

Every other test hands the library allocations of their own, which the caching allocator rounds to 512 bytes: a store that runs one row,
one float4 or one partial tile past an output lands in slack nobody looks at.  Behind a gradient that is a view of a flat vector, a
state that is the batch slice x[1:3], an output that is a slice of a larger result, the same store lands in a neighbour.

No new numerical reference.  Every case of CASES is an existing test function - its float64 oracle, its bounds - rerun on top of
GuardedABI (tests/sampler_support.py), which hands the listed entries every operand between two 64 KiB guards, once per guard fill
("nan0": NaN / 0, "ones": 1 / true), and checks the guards, the const operands and that the entries really ran on shadows.  The rows:
the RERUNS and SWEEPS of tests/test_gpu_operand_alignment.py (every entry that accepts natural alignment, at shapes that are ragged
already), and the hot-path entries at the smallest shapes where their kernels still take the ragged branches - K = 37 and 173 (generic),
192 and 256 (MFMA, three / two key chunks), B = 3 on the module launch, N = 100 = 96 + 4 and 1344 columns of the x-stationary product.
K = 37 is the forward's alone: gradient cases stay at the patch lengths and seeds whose ReLU margins their own tests pin.

One case no rerun gives: diffab_train_step_fwd / _bwd through ctypes with the weight and gradient tables pointing at views of one flat
vector each, without any harness (test_training_step_into_flat_gradient_views).
"""
import ctypes as C
import importlib
import time

import pytest
import torch

import diffab_oracle as orc
from conftest import maxrel
from diffab_pytorch import _hip
from sampler_support import GTOL, GUARD_FILLS, TOL, GuardedABI, check_params, f64, flat_parameters, hip, make_model, relu_margin, tensors_of  # noqa: F401
from scratch_poison import raw_bytes
from test_gpu_aa_constraints import unit as aa_unit  # noqa: F401  (fixtures of the rerun tests, under names of their own)
from test_gpu_operand_alignment import DIMS, RERUNS, SWEEPS, new_denoiser, step_case, train_case
from test_gpu_respaced import bench as respaced_bench  # noqa: F401
from test_gpu_reverse_step_composed import empty_set_reaches_the_kernel, models as composed_models  # noqa: F401
from test_gpu_reverse_step_composed import steered_models  # noqa: F401
from test_gpu_score import unit as score_unit  # noqa: F401
from test_gpu_steering import unit as steering_unit  # noqa: F401

pytestmark = pytest.mark.gpu
PLANES = _hip.FLAG_PAIR_PLANES
ME = "test_gpu_operand_extents"
FWD, LAYER = ("diffab_denoise_step_fwd",), ("diffab_ipa_layer_fwd_taped", "diffab_ipa_layer_bwd")
TRAIN, COT = ("diffab_train_step_fwd", "diffab_train_step_bwd"), ("diffab_denoise_step_fwd_taped", "diffab_denoise_step_bwd")
LOOP, SCORE = ("diffab_sample_loop_ex",), ("diffab_score_designs",)
RES = ("diffab_residue_embedding_fwd", "diffab_residue_embedding_bwd")
FUSED = RES + ("diffab_pair_embedding_fwd_taped", "diffab_pair_embedding_bwd_taped")
UNFUSED = RES + ("diffab_pair_embedding_xyz_fwd", "diffab_pair_embedding_bwd")


def loop_without_options_is_bitwise_loop_ex(hip, K):
    """diffab_sample_loop is diffab_sample_loop_ex without options: two reverse steps at B = 2 through ctypes (K = 128: the MFMA path;
    K = 173, padded: the generic forward and the ragged last tiles), the in-place state of the two calls equal to the bit.  The _ex form
    is held to the oracle by the reverse-step cases; no test with a reference calls the plain form."""
    _, _, _, inp4, gm4 = step_case(K)
    model = make_model(DIMS, 30 + K)  # (its own: every table it caches is built under the harness)
    B = 2
    order = ("seq_idx", "translations", "orientations", "res_context_emb", "pair_context_emb")
    d = model.denoiser.hip_dims(B, K)
    w = model.denoiser.hip_weights()
    sdev, tab = model._sched_on_device(), model._reverse_so3().struct()
    ws = _hip.workspace(hip.diffab_sample_workspace_bytes(C.byref(d)))
    gm = gm4[:B].cuda().contiguous()
    got = []
    for ex in (True, False):
        a = {k: inp4[k][:B].cuda().contiguous() for k in order}
        head = (C.byref(d), C.byref(w.struct), C.byref(sdev.struct), C.byref(tab), *[_hip.ptr(a[k]) for k in order], _hip.ptr(gm), 911, 4, 57,
                55, _hip.ptr(ws), ws.numel(), 0)
        rc = hip.diffab_sample_loop_ex(*head, None, _hip.stream_ptr()) if ex else hip.diffab_sample_loop(*head, _hip.stream_ptr())
        _hip.check(rc, "diffab_sample_loop" + ("_ex" if ex else ""))
        torch.cuda.synchronize()
        got.append(a)
    assert not torch.equal(got[0]["translations"].cpu(), inp4["translations"][:B])  # two steps were taken
    for k in order[:3]:
        assert torch.equal(got[0][k], got[1][k]), k


def layer_forward_without_autograd_at_ragged_k(hip, K):
    """The untaped diffab_ipa_layer_fwd (a layer called under no_grad) on the layer, the inputs and the oracle of
    tests/test_gpu_patch_lengths.py test_ipa_layer_gradients_vs_float64_oracle, at that test's forward bound: the gradient tests reach
    the taped forward only."""
    import test_gpu_patch_lengths as pl

    den, _ = pl.denoiser(seed=K + 3)
    layer = den.ipa.layers[1]
    inp = pl.gradient_inputs(K)
    names = ("res_context_emb", "pair_context_emb", "orientations", "translations")
    with torch.no_grad():
        y = layer(*[inp[k].cuda() for k in names])
    want = orc.ipa_layer(*[f64(inp[k]) for k in names], {"L." + n: f64(p) for n, p in layer.named_parameters()}, "L.", DIMS["H"])
    assert y.grad_fn is None and torch.isfinite(y).all() and maxrel(y, want) < TOL, (K, maxrel(y, want))


# id: (entries that must have run on shadows, test module, test function, fixtures, arguments or module -> arguments)
CASES = {}
for _K in (37, 173, 192, 256):
    for _f, _n in ((0, "dispatch"), (PLANES, "pairplanes")):
        CASES[f"forward_k{_K}_{_n}"] = (FWD, "test_gpu_patch_lengths", "test_forward_vs_float64_oracle", ("hip",), (_K, _f))
CASES.update({
    "forward_groups_k64": (FWD, "test_gpu_operand_alignment", "test_denoiser_forward_with_misaligned_groups_vs_float64_oracle", ("hip",),
                           (2, 64, 0, "bench")),
    "forward_groups_k64_pairplanes": (FWD, "test_gpu_operand_alignment", "test_denoiser_forward_with_misaligned_groups_vs_float64_oracle",
                                      ("hip",), (2, 64, PLANES, "bench")),
    "forward_groups_k128_b3_module": (FWD, "test_gpu_operand_alignment", "test_denoiser_forward_with_misaligned_groups_vs_float64_oracle",
                                      ("hip",), (3, 128, PLANES | _hip.FLAG_PERSISTENT_MODULE, "bench")),
    "forward_groups_unit_dims": (FWD, "test_gpu_operand_alignment", "test_denoiser_forward_with_misaligned_groups_vs_float64_oracle", ("hip",),
                                 (2, 16, 0, "unit")),
    "layer_k173": (LAYER, "test_gpu_patch_lengths", "test_ipa_layer_gradients_vs_float64_oracle", ("hip",), (173,)),
    "layer_k192": (LAYER, "test_gpu_patch_lengths", "test_ipa_layer_gradients_vs_float64_oracle", ("hip",), (192,)),
    "layer_k64": (LAYER, "test_gpu_backward_paths", "test_ipa_layer_gradients_at_k64_vs_float64_oracle", ("hip",), ()),
    "layer_no_pair_bias_h12": (LAYER, "test_gpu_generic_dims", "test_ipa_layer_gradients_vs_float64_oracle", ("hip",), ("af2", False)),
    # the untaped layer forward runs under no_grad only: the reference goldens' test calls it (and the taped pair, and the denoiser's)
    "layer_forward_goldens": (("diffab_ipa_layer_fwd",) + LAYER + COT, "test_gpu_autograd",
                              "test_denoiser_and_ipa_layer_autograd_vs_reference_goldens", ("hip", "golden"), ("bench",)),
    "train_k173": (TRAIN, "test_gpu_patch_lengths", "test_training_loss_gradients_vs_float64_oracle", ("hip",), (173,)),
    "train_k192": (TRAIN, "test_gpu_patch_lengths", "test_training_loss_gradients_vs_float64_oracle", ("hip",), (192,)),
    "train_k64_b3": (TRAIN, "test_gpu_backward_paths", "test_training_loss_gradients_vs_float64_oracle", ("hip",), (64, 3, 2, 11)),
    "train_k64_nl7": (TRAIN, "test_gpu_backward_paths", "test_training_loss_gradients_vs_float64_oracle", ("hip",), (64, 2, 7, 13)),
    "train_frozen_pair_ctx": (TRAIN, "test_gpu_backward_paths", "test_frozen_pair_context_gradients_vs_float64_oracle", ("hip",),
                              (64, 2, 2, 17)),
    "cotangents_k173": (COT, "test_gpu_patch_lengths", "test_denoiser_cotangent_gradients_vs_float64_oracle", ("hip",), (173,)),
    "cotangents_k196": (COT, "test_gpu_patch_lengths", "test_denoiser_cotangent_gradients_vs_float64_oracle", ("hip",), (196,)),
    "reverse_step_k173": (LOOP, "test_gpu_patch_lengths", "test_reverse_step_teacher_forced_at_ragged_k", ("hip",), (173,)),
    "reverse_step_all_options": (LOOP, "test_gpu_reverse_step_composed", "test_all_options_in_one_step_are_the_float64_composition",
                                 ("composed_models", "empty_set_reaches_the_kernel"), ("unit_k5",)),
    "reverse_step_steering": (LOOP, "test_gpu_reverse_step_composed", "test_a_steering_step_with_every_option_on",
                              ("steered_models", "empty_set_reaches_the_kernel"), ("unit", 64, 2, {})),
    # (the teacher-forced parity step, the noised scorer state and diffab_debug_linear128 at Kd = 128 - all three modes: no `when` here -
    # are rows of RERUNS below: accepts_sample_loop, accepts_score_designs_noised, accepts_debug_linear128_mode0)
    "sample_loop_plain_k128": (("diffab_sample_loop", "diffab_sample_loop_ex"), ME, "loop_without_options_is_bitwise_loop_ex", ("hip",), (128,)),
    "sample_loop_plain_k173": (("diffab_sample_loop", "diffab_sample_loop_ex"), ME, "loop_without_options_is_bitwise_loop_ex", ("hip",), (173,)),
    "layer_forward_k173": (("diffab_ipa_layer_fwd",), ME, "layer_forward_without_autograd_at_ragged_k", ("hip",), (173,)),
    "layer_forward_k192": (("diffab_ipa_layer_fwd",), ME, "layer_forward_without_autograd_at_ragged_k", ("hip",), (192,)),
    "score_k173": (SCORE, "test_gpu_patch_lengths", "test_score_terms_at_ragged_k_vs_oracle", ("hip",), ()),
    "xstat128_300x100": (("diffab_debug_xstat128",), "test_gpu_parity", "test_x_stationary_backward_product_is_fp32_accurate", ("hip",),
                         (300, 100)),
    "xstat128_129x1344": (("diffab_debug_xstat128",), "test_gpu_parity", "test_x_stationary_backward_product_is_fp32_accurate", ("hip",),
                          (129, 1344)),
    "row_tiles": (("diffab_debug_row_tiles",), "test_gpu_skip_rows_module", "test_row_tile_map_is_any_over_16_rows", ("hip",), ()),
    "row_plan": (("diffab_debug_row_plan",), "test_gpu_last_layer_rows", "test_row_plan_is_the_greedy_covering", ("hip",), ()),
    "encoders_distmat": (RES + ("diffab_pair_embedding_fwd", "diffab_pair_embedding_bwd"), "test_gpu_context_encoders",
                         "test_encode_context_vs_float64_oracle", ("hip",), ("unfused_A17", True, True, "distmat", 0)),
    "encoder_chunks_fused_taped": (FUSED, "test_gpu_context_encoders", "test_backward_chunks_vs_float64_oracle", ("hip",), (True, True)),
    "encoder_chunks_fused_recompute": (RES + ("diffab_pair_embedding_xyz_fwd", "diffab_pair_embedding_bwd"), "test_gpu_context_encoders",
                                       "test_backward_chunks_vs_float64_oracle", ("hip",), (True, False)),
    "encoder_chunks_unfused": (UNFUSED, "test_gpu_context_encoders", "test_backward_chunks_vs_float64_oracle", ("hip",), (False, True)),
})
for _name in importlib.import_module("test_gpu_context_encoders").CASES:  # the smallest run of every case: both masks generated, xyz
    CASES["encoders_" + _name] = (FUSED if _name.startswith("fused") else UNFUSED, "test_gpu_context_encoders",
                                  "test_encode_context_vs_float64_oracle", ("hip",), (_name, True, True, "xyz", 0))
for _id, (_entries, _mod, _fn, _fix, _args, _) in RERUNS.items():  # every entry that accepts natural alignment: its own test again
    CASES["accepts_" + _id] = (_entries, _mod, _fn, _fix, _args)
for _sweep in sorted(set(SWEEPS.values()), key=lambda f: f.__name__):  # ... or its sweep, which holds it to the oracle on views
    CASES["accepts_" + _sweep.__name__] = (tuple(sorted(n for n, f in SWEEPS.items() if f is _sweep)), "test_gpu_operand_alignment",
                                           _sweep.__name__, ("hip",), ())
COVERED = {e for row in CASES.values() for e in row[0]}
_SECONDS = {}


@pytest.mark.parametrize("fill", GUARD_FILLS)
@pytest.mark.parametrize("case", sorted(CASES))
def test_entries_rerun_their_own_reference_test_between_guards(request, case, fill):
    """The test an entry's own file holds, rerun with every operand of the entry between two guards: intact guards, const operands
    unchanged, the test's own comparison (a float read past the end is NaN under "nan0", a mask read past the end flips under "ones"),
    and every listed entry called on shadows."""
    entries, module, function, fixtures, args = CASES[case]
    mod = importlib.import_module(module)
    args = args(mod) if callable(args) else args
    values = {f: request.getfixturevalue(f) for f in fixtures}  # (models are built on the real library, before the stand-in)
    known = tensors_of([v for f, v in values.items() if f != "hip"], vars(mod), depth=6)  # tables cached before the harness stands in
    t0 = time.perf_counter()
    with GuardedABI(entries, fill, known=known) as abi:
        if "hip" in values:
            values["hip"] = abi
        getattr(mod, function)(*[values[f] for f in fixtures], *args)
    torch.cuda.synchronize()
    _SECONDS[(case, fill)] = time.perf_counter() - t0
    for e in entries:
        assert abi.counts.get(e, 0) > 0, (case, e, fill, "was not called on guarded operands", abi.counts)
    print(f"{case} [{fill}]: {_SECONDS[(case, fill)]:.1f} s, operands replaced {abi.counts}")


# ---------------------------------------------------------------------------------------------------------------- flat vectors
FILL = 7.25


def test_training_step_into_flat_gradient_views(hip):
    """The caller the contract is for, without any harness in between: diffab_train_step_fwd / _bwd through ctypes at K = 173 with `w`
    a pointer table over views of one flat parameter vector and `grads` a table over views of one flat gradient vector - every view on
    a 16-byte boundary, as the two entries ask of table buffers, so a view whose size is a multiple of 4 floats is followed directly by
    its neighbour and a 3-wide bias by one float of fill.  The library's own accumulating stores land in those views: every gradient,
    d res_ctx and d pair_ctx against the float64 oracle (GTOL, the case of tests/test_gpu_operand_alignment.py section 4); every byte
    of the gradient vector's storage between and around the views still holds its fill; the parameter vector's storage is unchanged to
    the bit."""
    K, B = 173, 2
    c = train_case(K)
    den64 = orc.denoiser({"denoiser." + k: v.double() for k, v in c["sd"].items()}, c["nz"]["seq_idx_t"], f64(c["nz"]["translations_t"]),
                         f64(c["nz"]["orientations_t"]), f64(c["inp"]["res_context_emb"]), f64(c["inp"]["pair_context_emb"]),
                         c["beta"].double(), DIMS["NL"], DIMS["H"])
    margin = relu_margin(c["sd"], c["nz"]["seq_idx_t"], c["inp"]["res_context_emb"], den64, c["beta"])
    assert margin > 5e-7, (margin, "inputs on a ReLU kink: pick another weight seed")  # (the margin the ragged-K gradient tests ask for)
    den, _ = new_denoiser(DIMS, 40 + K)
    den.requires_grad_(True)
    flat, offs, gflat, outside = flat_parameters(den, shift_floats=0, grads=FILL, align_floats=4)
    names = [n for n, _ in den.named_parameters()]
    params, grads = [p.data for _, p in den.named_parameters()], [p.grad for _, p in den.named_parameters()]
    assert not any(offs.values()) and not any(g.data_ptr() % 16 for g in grads)
    w = _hip.DenoiserWeightsOnDevice(dict(zip(names, params)), DIMS["NL"])
    g = _hip.DenoiserWeightsOnDevice(dict(zip(names, grads)), DIMS["NL"])
    # the tables point into the flat vectors themselves: nothing was copied on the way
    assert {t.data_ptr() for t in w.keep} == {t.data_ptr() for t in params} and {t.data_ptr() for t in g.keep} == {t.data_ptr() for t in grads}
    assert all(t.untyped_storage().data_ptr() == gflat.untyped_storage().data_ptr() for t in g.keep)
    neighbours = sum(a.data_ptr() + 4 * a.numel() == b.data_ptr() for a, b in zip(grads, grads[1:]))
    assert neighbours >= len(grads) // 2 and neighbours < len(grads) - 1, neighbours  # both: a neighbour directly behind, and fill
    before = {"parameters": raw_bytes(flat).clone(), "outside": outside(gflat).clone()}
    assert before["outside"].numel() >= 32 + 4 * (len(grads) - 1 - neighbours)
    assert bool((before["outside"].view(torch.float32) == FILL).all())
    d = den.hip_dims(B, K)
    cu = lambda v: v.cuda().contiguous()  # noqa: E731
    t = {"seq_t": cu(c["nz"]["seq_idx_t"]), "x_t": cu(c["nz"]["translations_t"]), "O_t": cu(c["nz"]["orientations_t"]),
         "res_ctx": cu(c["inp"]["res_context_emb"]), "pair_ctx": cu(c["inp"]["pair_context_emb"]), "beta": cu(c["beta"]),
         "true_post": cu(c["nz"]["seq_posterior"]), "true_eps": cu(c["nz"]["translations_eps"]), "true_O0": cu(c["inp"]["orientations"]),
         "gen_mask": cu(c["inp"]["generation_mask"]), "res_mask": cu(c["inp"]["residue_mask"]),
         "out_eps": torch.empty(B, K, 3, device="cuda"), "out_O0": torch.empty(B, K, 3, 3, device="cuda"),
         "out_posterior": torch.empty(B, K, 21, device="cuda"), "losses3": torch.empty(3, device="cuda"),
         "upstream3": torch.ones(3, device="cuda"), "d_res_ctx": torch.empty(B, K, DIMS["D"], device="cuda"),
         "d_pair_ctx": torch.zeros(B, K, K, DIMS["C"], device="cuda")}
    tape = _hip.workspace(hip.diffab_train_tape_bytes(C.byref(d)))
    ws = _hip.workspace(hip.diffab_train_workspace_bytes(C.byref(d)))
    fwd = ("seq_t", "x_t", "O_t", "res_ctx", "pair_ctx", "beta", "true_post", "true_eps", "true_O0", "gen_mask", "res_mask", "out_eps", "out_O0",
           "out_posterior", "losses3")
    bwd = ("seq_t", "x_t", "O_t", "pair_ctx", "out_eps", "out_O0", "out_posterior", "true_post", "true_eps", "true_O0", "gen_mask", "res_mask",
           "upstream3", "d_res_ctx", "d_pair_ctx")
    _hip.check(hip.diffab_train_step_fwd(C.byref(d), C.byref(w.struct), *[_hip.ptr(t[k]) for k in fwd], _hip.ptr(tape), tape.numel(), 0,
                                         _hip.stream_ptr()), "train_step_fwd")
    _hip.check(hip.diffab_train_step_bwd(C.byref(d), C.byref(w.struct), C.byref(g.struct), *[_hip.ptr(t[k]) for k in bwd], _hip.ptr(tape),
                                         tape.numel(), _hip.ptr(ws), ws.numel(), _hip.stream_ptr()), "train_step_bwd")
    torch.cuda.synchronize()
    torch.testing.assert_close(t["losses3"].cpu().double(), torch.tensor(c["losses"]).double(), rtol=5e-5, atol=0)
    assert maxrel(t["d_res_ctx"], c["d_rc"]) < GTOL and maxrel(t["d_pair_ctx"], c["d_pc"]) < GTOL
    check_params(den.named_parameters(), c["sdo"], "denoiser.", f"K={K} training step through ctypes, flat parameters and flat gradients")
    assert torch.equal(raw_bytes(flat), before["parameters"]), "a parameter (or the fill around one) changed"
    assert torch.equal(outside(gflat), before["outside"]), "a byte between or around the gradient views changed"
