"""Operands that are only 4-byte aligned (include/diffab_hip.h, "Operand alignment").

Every other test hands the library fresh torch allocations: 512-byte aligned.  A parameter that is a view of one flat parameter vector, or
a batch slice at a ragged patch length, is contiguous and starts 4, 8 or 12 bytes behind a 16-byte boundary.  The header gives every data
operand of every entry one of two outcomes - ACCEPTED (the entry's result contract) or REFUSED (DIFFAB_ERR_ARG naming the operand, decided
on the host before anything is enqueued) - and tests/sampler_support.py holds the table of both, mirrored from the header:

  ENTRIES     every exported diffab_* function -> NO_DATA (queries, switches), ACCEPTS (every data operand at its natural alignment) or
              REFUSES (its float operands and weight / gradient tables need 16 bytes; SIGNATURES says which argument is which)
  SIGNATURES  the argument list of every REFUSES entry: name:kind, kind = f (float operand, refused unless 16-byte aligned), fa (float,
              accepted), i64 / m (int64 / mask: accepted), a weight table, a struct, or a literal
  refused()   the (entry, operand) pairs allowed to refuse - nothing else may; through the Python front end the set is empty

tests/test_operand_alignment_host.py drives every pair of refused() through the C ABI with pointers that are never dereferenced (the
refusal comes before the workspace-size check, so before any launch).  Here, on the device:

  1. Denoiser forward through the front end with one operand group misaligned at a time, then all, against the float64 oracle (TOL,
     maxrel and elemrel as tests/test_gpu_parity.py); the front end copies what the C entry would refuse, so nothing is refused, and
     whether the result is bitwise the aligned call's is printed.
  2. diffab_denoise_step_fwd through ctypes: the accepted operand (seq_t at +8) against the oracle, every refused operand - inputs,
     outputs, a field of every weight group - with the code, the message, outputs unchanged as raw bytes, and a correct aligned call
     on the same workspace afterwards.
  3. One teacher-forced reverse step (diffab_sample_loop_ex) at t in {57, 2, 1}: in-place state, contexts, mask, flat-vector weights,
     schedule and IGSO3 tables misaligned, and the natural case - rows [1:3] of a B = 4 batch at K = 173 - against oracle_reverse_step.
  4. The training step through the front end with flat-vector weights and misaligned inputs against the oracle's autograd, and
     diffab_train_step_bwd through ctypes: refused operands leave pattern-filled gradient buffers unchanged to the byte, and the
     aligned call that follows accumulates (+=) into the pattern.
  5. The accepted entries that pick a vector form from the pointer (diffab_philox_fill, diffab_featurize_xyz, diffab_patch_gather /
     _scatter) and the elementwise entries with a host reference in the oracle, through ctypes with every pointer misaligned.
  6. Every other accepted entry - frames, IGSO3, the jump update, patch selection, the metrics, the refinement, guidance, steering,
     the initialisers, the two pointer-dispatched diagnostics (diffab_debug_gemm_tn, diffab_debug_linear128 mode 0) - and the accepted
     operands of diffab_score_designs and diffab_sample_loop_ex: the test of the entry's own file, with its host reference and its
     bounds, rerun on top of MisalignedABI (tests/sampler_support.py), which hands the entry misaligned copies of every tensor.
  7. diffab_sample_loop_ex through ctypes: refused operands leave the in-place state unchanged as raw bytes.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import diffab_oracle as orc
from conftest import elemrel, maxrel
from diffab_pytorch import _hip, synthetic as syn
from sampler_support import (ACCEPTS, ARGS, DEBUG_REFUSES, ENTRIES, GTOL, OUTS, REFUSES, SIGNATURES, TOL, MisalignedABI, check_params, header_exports, signature, f64, flat_parameters, hip, leaves, make_model, misalign_parameters,
                             misaligned, n_real_of, oracle_reverse_step, padded)
from scratch_poison import raw_bytes
from test_gpu_aa_constraints import unit as aa_unit  # noqa: F401  (fixtures of the rerun tests, under names of their own)
from test_gpu_respaced import bench as respaced_bench  # noqa: F401
from test_gpu_score import unit as score_unit  # noqa: F401
from test_gpu_steering import unit as steering_unit  # noqa: F401

# ---------------------------------------------------------------------------------------------------------------- GPU tests
gpu = pytest.mark.gpu
DIMS = dict(syn.BENCH_DIMS, NL=2)
PLANES, PERSISTENT, FP32 = _hip.FLAG_PAIR_PLANES, _hip.FLAG_PERSISTENT_MODULE, _hip.FLAG_FP32_GEMM
F32_OFFSETS = (4, 8, 12)


def new_denoiser(dims, seed):
    from diffab_pytorch.diffab_pytorch import Denoiser

    den = Denoiser(dims["D"], dims["C"], dims["NL"], dims["DS"], dims["PQ"], dims["PV"], dims["H"], 21)
    sd = syn.denoiser_state_dict(dims, seed=seed, prefix="")
    den.load_state_dict(sd, strict=True)
    return den.cuda().requires_grad_(False), sd


def check_outputs(out, want, what):
    for k in OUTS:
        got = out[k].cpu()
        assert torch.isfinite(got).all(), (what, k)
        r, e = maxrel(got, want[k]), elemrel(got, want[k])
        assert r < TOL and e < TOL, (what, k, r, e)


_FWD = {}


def forward_case(K, dims_name="bench"):
    """(dims, state dict, host inputs of 2 patches, beta, float64 oracle outputs), once per patch length."""
    key = (K, dims_name)
    if key not in _FWD:
        dims = DIMS if dims_name == "bench" else dict(syn.UNIT_DIMS, NL=2)
        sd = syn.denoiser_state_dict(dims, seed=900 + K, prefix="")
        inp = syn.patches(2, K, dims, seed=700 + K, coord_sigma=6.0)
        beta = torch.tensor([0.03, 0.7])
        want = orc.denoiser({"denoiser." + k: v.double() for k, v in sd.items()}, inp["seq_idx"], *[inp[k].double() for k in ARGS[1:]],
                            beta.double(), dims["NL"], dims["H"])
        _FWD[key] = (dims, sd, inp, beta, {k: want[k].detach() for k in OUTS})
    return _FWD[key]


INPUT_GROUPS = {  # group -> (names of the forward's inputs, byte offsets tried)
    "seq_t": (("seq_idx",), (8,)), "x_t": (("translations",), F32_OFFSETS), "O_t": (("orientations",), F32_OFFSETS),
    "res_ctx": (("res_context_emb",), F32_OFFSETS), "pair_ctx": (("pair_context_emb",), F32_OFFSETS), "beta": (("beta",), F32_OFFSETS),
    "masks": (("generation_mask", "residue_mask"), (1, 3))}
WEIGHT_GROUPS = {
    "projections": lambda n: ".to_q_" in n or ".to_k_" in n or ".to_v_" in n, "w_bias": lambda n: "to_pair_bias" in n,
    "gamma": lambda n: n.endswith("gamma"), "to_out": lambda n: ".to_out." in n,
    "embedding_mlp": lambda n: n.startswith("to_res_emb") or n.startswith("sequence_embedding"),
    "coord_head": lambda n: n.startswith("coordinate_denoising"), "orient_head": lambda n: n.startswith("orientation_denoising"),
    "seq_head": lambda n: n.startswith("sequence_denoising")}

FORWARD_CASES = [  # id, B, K, flags, dims
    ("k64", 2, 64, 0, "bench"), ("k64_fp32gemm", 2, 64, FP32, "bench"), ("k64_pairplanes", 2, 64, PLANES, "bench"),
    ("k128", 2, 128, 0, "bench"), ("k128_fp32gemm", 2, 128, FP32, "bench"), ("k128_pairplanes", 2, 128, PLANES, "bench"),
    ("k128_b8_module", 8, 128, PLANES | PERSISTENT, "bench"), ("k256_chunked", 2, 256, PLANES, "bench"), ("unit_dims", 2, 16, 0, "unit")]


@gpu
@pytest.mark.parametrize("B,K,flags,dims_name", [c[1:] for c in FORWARD_CASES], ids=[c[0] for c in FORWARD_CASES])
def test_denoiser_forward_with_misaligned_groups_vs_float64_oracle(hip, B, K, flags, dims_name):
    """Denoiser.forward with each operand group misaligned in turn (every offset of its type), then everything at once with the weights
    as views of one flat vector: all five outputs against the float64 oracle.  The outputs are the front end's own allocations; a
    misaligned OUTPUT exists at the C ABI only (test_denoise_step_fwd_refusals_and_accepted_operand).  B = 8 repeats the two patches
    (row b is patch b % 2; tests/test_gpu_operand_extents.py also asks for B = 3)."""
    dims, sd, inp2, beta2, want2 = forward_case(K, dims_name)
    idx = torch.arange(B) % 2
    host = {k: v[idx].contiguous() for k, v in inp2.items()}
    host["beta"] = beta2[idx].contiguous()
    want = {k: v[idx] for k, v in want2.items()}
    dev = {k: v.cuda() for k, v in host.items()}
    names = ARGS + ("beta", "generation_mask", "residue_mask")

    def run(den, over=()):
        a = dict(dev)
        a.update(over)
        return den(*[a[k] for k in names], return_logits=True, flags=flags)

    den, _ = new_denoiser(dims, 900 + K)
    base = run(den)
    check_outputs(base, want, "aligned")
    same = {}

    def compare(out, what):
        check_outputs(out, want, what)
        same[what] = all(torch.equal(out[k], base[k]) for k in OUTS)

    for group, (keys, offsets) in INPUT_GROUPS.items():
        for off in offsets:
            over = {k: misaligned(dev[k], off) for k in keys}
            assert all(v.data_ptr() % 16 == off and v.is_contiguous() for v in over.values())
            compare(run(den, over), f"{group}+{off}")
    for group, select in WEIGHT_GROUPS.items():
        den_g, _ = new_denoiser(dims, 900 + K)
        hit = misalign_parameters(den_g, select, 4 if group != "to_out" else 12)
        assert hit, group
        compare(run(den_g), group)
    den_f, _ = new_denoiser(dims, 900 + K)
    _, offs = flat_parameters(den_f)
    assert sum(o != 0 for o in offs.values()) >= len(offs) // 2, offs  # shifted by one float: most views are off the boundary
    over = {k: misaligned(dev[k], 8 if dev[k].dtype == torch.int64 else 3 if dev[k].dtype == torch.bool else 12) for k in names}
    compare(run(den_f, over), "everything")
    differ = [k for k, v in same.items() if not v]
    print(f"B={B} K={K} flags={flags} {dims_name}: {len(same)} misaligned calls, not bitwise equal to the aligned call: {differ or 'none'}")


def denoiser_call(hip, dims_struct, w, t, ws, flags=0):
    """diffab_denoise_step_fwd on the tensors of `t` (by the prototype's names)."""
    return hip.diffab_denoise_step_fwd(C.byref(dims_struct), C.byref(w.struct), *[_hip.ptr(t[k]) for k in (
        "seq_t", "x_t", "O_t", "res_ctx", "pair_ctx", "beta", "out_eps", "out_O0", "out_posterior", "out_logits", "out_res_emb")],
        _hip.ptr(ws), ws.numel(), flags, _hip.stream_ptr())


OUT_OF = {"out_eps": "translations_eps", "out_O0": "orientations_t0", "out_posterior": "seq_posterior", "out_logits": "aa_logits",
          "out_res_emb": "res_emb"}


@gpu
def test_denoise_step_fwd_refusals_and_accepted_operand(hip):
    """diffab_denoise_step_fwd at B = 2, K = 64 through ctypes.  seq_t at +8 is accepted: the oracle's outputs (and, printed, whether
    bitwise the aligned call's).  Every float input, every output and one buffer of every weight group at +4 / +8 / +12 is refused:
    DIFFAB_ERR_ARG, a message naming the operand and `16-byte`, the pattern-filled outputs unchanged as raw bytes; then an aligned call
    on the same workspace gives bitwise the first call's outputs."""
    dims, sd, inp, beta, want = forward_case(64)
    den, _ = new_denoiser(dims, 900 + 64)
    B, K = inp["seq_idx"].shape
    d = den.hip_dims(B, K)
    w = den.hip_weights()
    ws = _hip.workspace(hip.diffab_denoise_workspace_bytes(C.byref(d)))
    t = {"seq_t": inp["seq_idx"].cuda(), "x_t": inp["translations"].cuda(), "O_t": inp["orientations"].cuda(),
         "res_ctx": inp["res_context_emb"].cuda(), "pair_ctx": inp["pair_context_emb"].cuda(), "beta": beta.cuda()}
    shapes = {"out_eps": (B, K, 3), "out_O0": (B, K, 3, 3), "out_posterior": (B, K, 21), "out_logits": (B, K, 21), "out_res_emb": (B, K, dims["D"])}

    def outputs():
        return {k: torch.full(s, 7.25, device="cuda") for k, s in shapes.items()}

    first = dict(t, **outputs())
    _hip.check(denoiser_call(hip, d, w, first, ws), "aligned call")
    check_outputs({OUT_OF[k]: first[k] for k in shapes}, want, "aligned")
    acc = dict(t, **outputs(), seq_t=misaligned(t["seq_t"], 8))
    _hip.check(denoiser_call(hip, d, w, acc, ws), "seq_t at +8")
    check_outputs({OUT_OF[k]: acc[k] for k in shapes}, want, "seq_t+8")
    print("seq_t at +8 bitwise the aligned call:", all(torch.equal(acc[k], first[k]) for k in shapes))

    def expect_refusal(args, wtab, operand):
        before = {k: raw_bytes(args[k]).clone() for k in shapes}
        rc = denoiser_call(hip, d, wtab, args, ws)
        msg = hip.diffab_last_error().decode()
        assert rc == -1, (operand, rc, msg)
        assert f"denoise_step_fwd: operand {operand} " in msg and "16-byte" in msg, (operand, msg)
        torch.cuda.synchronize()
        for k in shapes:
            assert torch.equal(raw_bytes(args[k]), before[k]), (operand, k)

    n = 0
    for name in list(t)[1:] + list(shapes):
        for off in F32_OFFSETS:
            args = dict(t, **outputs())
            args[name] = misaligned(args[name], off)
            expect_refusal(args, w, name)
            n += 1
    fields = [("w.res_w0", lambda s: s, "res_w0"), ("w.seq_emb", lambda s: s, "seq_emb"), ("w.coord.b4", lambda s: s.coord, "b4"),
              ("w.orient.w0", lambda s: s.orient, "w0"), ("w.seq.w4", lambda s: s.seq, "w4"), ("w.layers[0].w_bias", lambda s: w.layers[0], "w_bias"),
              ("w.layers[1].gamma", lambda s: w.layers[1], "gamma"), ("w.layers[1].wq_p", lambda s: w.layers[1], "wq_p"),
              ("w.layers[0].w_out", lambda s: w.layers[0], "w_out"), ("w.layers[1].b_out", lambda s: w.layers[1], "b_out")]
    for operand, owner, field in fields:
        obj = owner(w.struct)
        good = getattr(obj, field)
        setattr(obj, field, good + 4)  # (never dereferenced: the refusal comes first)
        expect_refusal(dict(t, **outputs()), w, operand)
        setattr(obj, field, good)
        n += 1
    again = dict(t, **outputs())
    _hip.check(denoiser_call(hip, d, w, again, ws), "aligned call after the refusals")
    for k in shapes:
        assert torch.equal(again[k], first[k]), k
    print(n, "refusals, each with untouched outputs; the aligned call on the same workspace is bitwise the first")


# ---------------------------------------------------------------------------------------------------------------- one reverse step
STEP_T = (57, 2, 1)
_STEP = {}


def step_case(K):
    """(model, oracle state dict, schedule, 4 host patches, generation mask) at patch length K, once."""
    if K not in _STEP:
        model = make_model(DIMS, 30 + K)
        sd = {"denoiser." + k: v for k, v in syn.denoiser_state_dict(DIMS, seed=30 + K, prefix="").items()}
        sched = orc.cosine_variance_schedule(100, s=0.01, beta_max=0.999)
        inp = padded(4, K, n_real_of(K), seed=500 + K) if K % 64 else syn.patches(4, K, DIMS, seed=500 + K, coord_sigma=6.0)
        gm = inp["generation_mask"].clone()
        gm[:, 8:40] = True
        if "residue_mask" in inp:
            gm &= inp["residue_mask"]
        _STEP[K] = (model, sd, sched, inp, gm)
    return _STEP[K]


def check_step(got, model, sd, sched, inp, gm, seed, first, t, what):
    s1, x1, O1, den, us, edge = oracle_reverse_step(sd, inp, gm, model._reverse_so3(), sched, seed, first, t, DIMS["NL"], DIMS["H"])
    rx, rO = maxrel(got["translations"], x1), maxrel(got["orientations"], O1)
    assert rx < TOL and rO < TOL, (what, t, rx, rO)
    diff = got["seq_idx"].cpu() != s1
    if diff.any():  # the existing CDF-edge rule for a flipped draw
        assert float(edge[diff].max()) < 1e-5, (what, t, float(edge[diff].max()))
    for k in ("seq_idx", "translations", "orientations"):
        assert torch.equal(got[k].cpu()[~gm], inp[k][~gm]), (what, t, k)
    return int(diff.sum())


def step(model, a, gm, seed, first, t, flags=0):
    return model.sample(a["seq_idx"], a["translations"], a["orientations"], res_context_emb=a["res_context_emb"],
                        pair_context_emb=a["pair_context_emb"], generation_mask=gm, seed=seed, first_patch=first, t_start=t, t_stop=t - 1,
                        init=False, flags=flags)


@gpu
@pytest.mark.parametrize("B,K", [(2, 128), (8, 128), (2, 173)], ids=["b2_k128", "b8_k128_module", "b2_k173"])
def test_reverse_step_with_misaligned_operands_vs_oracle(hip, B, K):
    """One teacher-forced reverse step at t in {57, 2, 1} with the state, the contexts and the mask misaligned, the denoiser's weights
    as views of one flat vector, and the schedule and reverse IGSO3 tables (operands the C entry accepts) rebound to misaligned views:
    x and O within TOL of the oracle, a flipped draw only on a CDF edge, the rest of the state bitwise untouched.  B = 8 repeats two
    patches and asks for the module launch (every patch of a reverse step shares t, and the lanes differ per row, so every row is
    compared with its own oracle row)."""
    model, sd, sched, inp4, gm4 = step_case(K)
    idx = torch.arange(B) % 2
    inp = {k: v[idx].contiguous() for k, v in inp4.items()}
    gm = gm4[idx].contiguous()
    dev = {k: v.cuda() for k, v in inp.items()}
    flat, offs = flat_parameters(model.denoiser)
    sdev = model._sched_on_device()
    sdev.tensors = {k: misaligned(v, 4 * (1 + i % 3)) for i, (k, v) in enumerate(sdev.tensors.items())}
    ts = sdev.tensors
    sdev.struct = _hip.Sched(sdev.T, *[_hip.ptr(ts[k]) for k in ("alpha", "alpha_bar", "alpha_bar_sqrt", "one_minus_alpha_bar_sqrt", "beta")])
    rev = model._reverse_so3()
    rev._sigmas, rev._cdf = misaligned(rev._sigmas, 4), misaligned(rev._cdf, 12)
    flags = PERSISTENT if B == 8 else 0  # the loop takes the module launch by itself only when the batch fills the chip: ask for it
    a = {k: misaligned(v, 8 if v.dtype == torch.int64 else 12) for k, v in dev.items() if k in ARGS}
    gmd = misaligned(gm.cuda(), 3)
    seed, first, flips = 777, 6, 0
    for t in STEP_T:
        flips += check_step(step(model, a, gmd, seed, first, t, flags), model, sd, sched, inp, gm, seed, first, t, f"B={B} K={K}")
    print(f"B={B} K={K}: {flips} draws on a CDF edge; parameter offsets in the flat vector {sorted(set(offs.values()))}")


@gpu
def test_reverse_step_on_a_batch_slice_at_ragged_k_vs_oracle(hip):
    """The natural case: rows [1:3] of a B = 4 device batch at K = 173.  The slices are contiguous; x[1:3] starts 12 bytes and O[1:3]
    4 bytes behind a 16-byte boundary, the contexts 4 and 0."""
    K = 173
    model, sd, sched, inp4, gm4 = step_case(K)
    dev4 = {k: v.cuda() for k, v in inp4.items()}
    a = {k: dev4[k][1:3] for k in ARGS}
    assert all(v.is_contiguous() for v in a.values())
    assert a["translations"].data_ptr() % 16 == 12 and a["orientations"].data_ptr() % 16 == 4
    inp = {k: v[1:3] for k, v in inp4.items()}
    seed, first = 778, 2
    for t in STEP_T:
        check_step(step(model, a, gm4.cuda()[1:3], seed, first, t), model, sd, sched, inp, gm4[1:3], seed, first, t, "slice [1:3] K=173")


@gpu
def test_sample_loop_refusal_leaves_the_in_place_state_untouched(hip):
    """diffab_sample_loop_ex at B = 2, K = 128 through ctypes (DiffAb.sample clones the state, so the in-place contract shows at the C
    ABI only).  x, O, res_ctx, pair_ctx at +4 / +8 / +12 and a buffer of the weight table are refused by name; seq, x and O - the state
    the loop updates in place - are unchanged as raw bytes, the misaligned view's whole buffer included; the aligned call that follows
    on the same workspace is bitwise the call made before the refusals."""
    model, sd, sched, inp4, gm4 = step_case(128)
    B, K = 2, 128
    host = {k: inp4[k][:B].contiguous() for k in ARGS}
    d = model.denoiser.hip_dims(B, K)
    w = model.denoiser.hip_weights()
    sdev, tab = model._sched_on_device(), model._reverse_so3().struct()
    ws = _hip.workspace(hip.diffab_sample_workspace_bytes(C.byref(d)))
    gm = gm4[:B].cuda().contiguous()
    order = ("seq_idx", "translations", "orientations", "res_context_emb", "pair_context_emb")
    operand = dict(zip(order, ("seq", "x", "O", "res_ctx", "pair_ctx")))

    def fresh():
        return {k: host[k].cuda().contiguous() for k in order}

    def call(a):
        return hip.diffab_sample_loop_ex(C.byref(d), C.byref(w.struct), C.byref(sdev.struct), C.byref(tab), *[_hip.ptr(a[k]) for k in order],
                                         _hip.ptr(gm), 911, 4, 57, 55, _hip.ptr(ws), ws.numel(), 0, None, _hip.stream_ptr())

    first = fresh()
    _hip.check(call(first), "aligned call")
    torch.cuda.synchronize()
    assert not torch.equal(first["translations"].cpu(), host["translations"])  # two steps were taken
    n = 0

    def expect_refusal(a, name):
        before = {k: raw_bytes(a[k]).clone() for k in order[:3]}
        rc = call(a)
        msg = hip.diffab_last_error().decode()
        assert rc == -1 and f"sample_loop: operand {name} " in msg and "16-byte" in msg, (name, rc, msg)
        torch.cuda.synchronize()
        for k in order[:3]:
            assert torch.equal(raw_bytes(a[k]), before[k]), (name, k)

    for k in order[1:]:
        for off in F32_OFFSETS:
            a = fresh()
            a[k] = misaligned(a[k], off)
            expect_refusal(a, operand[k])
            n += 1
    for name, obj, field in (("w.res_w2", w.struct, "res_w2"), ("w.orient.b2", w.struct.orient, "b2"), ("w.layers[1].wv_p", w.layers[1], "wv_p")):
        good = getattr(obj, field)
        setattr(obj, field, good + 4)  # (never dereferenced: the refusal comes first)
        expect_refusal(fresh(), name)
        setattr(obj, field, good)
        n += 1
    again = fresh()
    _hip.check(call(again), "aligned call after the refusals")
    for k in order[:3]:
        assert torch.equal(again[k], first[k]), k
    print(n, "refusals with the in-place state untouched; the aligned call on the same workspace is bitwise the first")


# ---------------------------------------------------------------------------------------------------------------- training
def train_inputs(B, K, seed):
    inp = syn.patches(B, K, DIMS, seed=seed, coord_sigma=6.0)
    gm = inp["generation_mask"].clone()
    gm[:, 10:34] = True
    inp["generation_mask"], inp["residue_mask"] = gm, torch.ones_like(gm)
    g = torch.Generator().manual_seed(seed)
    eps = torch.randn(B, K, 3, generator=g)
    other = syn.patches(B, K, DIMS, seed=seed + 7)["orientations"]
    nz = {"seq_idx_t": torch.where(gm, torch.randint(0, 20, (B, K), generator=g), inp["seq_idx"]),
          "translations_t": inp["translations"] + 2.0 * gm[..., None] * eps,
          "orientations_t": torch.where(gm[..., None, None], other, inp["orientations"]),
          "seq_posterior": torch.softmax(2.0 * torch.randn(B, K, 21, generator=g), -1), "translations_eps": eps}
    return inp, nz, torch.tensor([0.03, 0.7])[:B]


_TRAIN = {}


def train_case(K):
    """The float64 oracle of one training step (losses, d res_ctx, d pair_ctx, parameter gradients as leaves), once per K."""
    if K not in _TRAIN:
        sd = syn.denoiser_state_dict(DIMS, seed=40 + K, prefix="")
        inp, nz, beta = train_inputs(2, K, 600 + K)
        rco, pco = f64(inp["res_context_emb"]).requires_grad_(True), f64(inp["pair_context_emb"]).requires_grad_(True)
        sdo = leaves(sd, "denoiser.")
        den = orc.denoiser(sdo, nz["seq_idx_t"], f64(nz["translations_t"]), f64(nz["orientations_t"]), rco, pco, beta.double(), DIMS["NL"],
                           DIMS["H"])
        lo = orc.hotpath_losses(den, f64(nz["seq_posterior"]), f64(nz["translations_eps"]), f64(inp["orientations"]), inp["generation_mask"],
                                inp["residue_mask"])
        (lo[0] + lo[1] + lo[2]).backward()
        _TRAIN[K] = dict(sd=sd, inp=inp, nz=nz, beta=beta, losses=[float(v.detach()) for v in lo], d_rc=rco.grad, d_pc=pco.grad, sdo=sdo)
    return _TRAIN[K]


@gpu
@pytest.mark.parametrize("K", [64, 128])
def test_training_step_with_misaligned_operands_vs_float64_oracle(hip, K):
    """hotpath_train_losses + backward (diffab_train_step_fwd / _bwd) with the denoiser's parameters as views of one flat vector and
    every input tensor misaligned: the losses (rtol 5e-5), d res_ctx, d pair_ctx and every parameter gradient (GTOL) against the
    oracle's autograd - the bounds of tests/test_gpu_backward_paths.py.  The gradients come back in the parameters' own (misaligned)
    .grad layout."""
    from diffab_pytorch import DiffAb

    c = train_case(K)
    torch.manual_seed(0)
    model = DiffAb(DIMS["D"], DIMS["C"], DIMS["NL"], DIMS["DS"], DIMS["PQ"], DIMS["PV"], DIMS["H"]).cuda()
    model.denoiser.load_state_dict(c["sd"])
    _, offs = flat_parameters(model.denoiser)
    assert any(offs.values())
    mis = lambda v: misaligned(v.cuda(), 8 if v.dtype == torch.int64 else 1 if v.dtype == torch.bool else 4)  # noqa: E731
    inp = {k: mis(v) for k, v in c["inp"].items()}
    nz = {k: mis(v) for k, v in c["nz"].items()}
    rc = mis(c["inp"]["res_context_emb"]).requires_grad_(True)
    pc = mis(c["inp"]["pair_context_emb"]).requires_grad_(True)
    ls = model.hotpath_train_losses(nz, rc, pc, mis(c["beta"]), inp["orientations"], inp["generation_mask"], inp["residue_mask"])
    (ls[0] + ls[1] + ls[2]).backward()
    np.testing.assert_allclose([float(v) for v in ls], c["losses"], rtol=5e-5)
    r_rc, r_pc = maxrel(rc.grad, c["d_rc"]), maxrel(pc.grad, c["d_pc"])
    assert r_rc < GTOL and r_pc < GTOL, (K, r_rc, r_pc)
    check_params(model.denoiser.named_parameters(), c["sdo"], "denoiser.", f"K={K} training step, flat misaligned parameters")


@gpu
def test_train_step_bwd_refusal_leaves_gradients_untouched_and_accumulates(hip):
    """diffab_train_step_fwd / _bwd at B = 2, K = 64 through ctypes.  A misaligned cotangent (upstream3), input, gradient buffer or
    d_pair_ctx is refused with the operand's name, and every gradient buffer - pre-filled with a pattern - is unchanged as raw bytes.
    The aligned call that follows ACCUMULATES: (buffer - pattern) equals the gradients of a call into zero-filled buffers to the
    rounding of the pattern's magnitude, and those equal the oracle's (GTOL)."""
    from diffab_pytorch.diffab_pytorch import _zero_grads_like

    K = 64
    c = train_case(K)
    den, _ = new_denoiser(DIMS, 40 + K)
    den.load_state_dict(c["sd"])
    B = 2
    d = den.hip_dims(B, K)
    names = [n for n, _ in den.named_parameters()]
    params = [p.data for _, p in den.named_parameters()]
    w = _hip.DenoiserWeightsOnDevice(dict(zip(names, params)), DIMS["NL"])
    cu = lambda v: v.cuda().contiguous()  # noqa: E731
    t = {"seq_t": cu(c["nz"]["seq_idx_t"]), "x_t": cu(c["nz"]["translations_t"]), "O_t": cu(c["nz"]["orientations_t"]),
         "res_ctx": cu(c["inp"]["res_context_emb"]), "pair_ctx": cu(c["inp"]["pair_context_emb"]), "beta": cu(c["beta"]),
         "true_post": cu(c["nz"]["seq_posterior"]), "true_eps": cu(c["nz"]["translations_eps"]), "true_O0": cu(c["inp"]["orientations"]),
         "gen_mask": cu(c["inp"]["generation_mask"]), "res_mask": cu(c["inp"]["residue_mask"]),
         "out_eps": torch.empty(B, K, 3, device="cuda"), "out_O0": torch.empty(B, K, 3, 3, device="cuda"),
         "out_posterior": torch.empty(B, K, 21, device="cuda"), "losses3": torch.empty(3, device="cuda"),
         "upstream3": torch.ones(3, device="cuda")}
    tape = _hip.workspace(hip.diffab_train_tape_bytes(C.byref(d)))
    ws = _hip.workspace(hip.diffab_train_workspace_bytes(C.byref(d)))
    fwd = ("seq_t", "x_t", "O_t", "res_ctx", "pair_ctx", "beta", "true_post", "true_eps", "true_O0", "gen_mask", "res_mask", "out_eps", "out_O0",
           "out_posterior", "losses3")
    _hip.check(hip.diffab_train_step_fwd(C.byref(d), C.byref(w.struct), *[_hip.ptr(t[k]) for k in fwd], _hip.ptr(tape), tape.numel(), 0,
                                         _hip.stream_ptr()), "train_step_fwd")
    np.testing.assert_allclose(t["losses3"].cpu().numpy(), c["losses"], rtol=5e-5)
    bwd = ("seq_t", "x_t", "O_t", "pair_ctx", "out_eps", "out_O0", "out_posterior", "true_post", "true_eps", "true_O0", "gen_mask", "res_mask",
           "upstream3", "d_res_ctx", "d_pair_ctx")

    def backward(args, g):
        return hip.diffab_train_step_bwd(C.byref(d), C.byref(w.struct), C.byref(g.struct), *[_hip.ptr(args[k]) for k in bwd], _hip.ptr(tape),
                                         tape.numel(), _hip.ptr(ws), ws.numel(), _hip.stream_ptr())

    def buffers(fill):
        grads, flat = _zero_grads_like(params)
        flat.fill_(fill)
        g = _hip.DenoiserWeightsOnDevice(dict(zip(names, grads)), DIMS["NL"])
        return grads, flat, g, dict(t, d_res_ctx=torch.full((B, K, DIMS["D"]), fill, device="cuda"),
                                    d_pair_ctx=torch.full((B, K, K, DIMS["C"]), fill, device="cuda"))

    PATTERN = 0.5
    grads, flat, g, args = buffers(PATTERN)
    before = {"flat": raw_bytes(flat).clone(), "d_res_ctx": raw_bytes(args["d_res_ctx"]).clone(),
              "d_pair_ctx": raw_bytes(args["d_pair_ctx"]).clone()}

    def expect_refusal(a, gtab, operand):
        rc = backward(a, gtab)
        msg = hip.diffab_last_error().decode()
        assert rc == -1 and f"train_step_bwd: operand {operand} " in msg and "16-byte" in msg, (operand, rc, msg)
        torch.cuda.synchronize()
        assert torch.equal(raw_bytes(flat), before["flat"]), operand
        for k in ("d_res_ctx", "d_pair_ctx"):
            assert torch.equal(raw_bytes(args[k]), before[k]), (operand, k)

    for name in ("upstream3", "x_t", "O_t", "pair_ctx", "out_eps", "out_O0", "out_posterior", "true_post", "true_eps", "true_O0"):
        for off in F32_OFFSETS:
            expect_refusal(dict(args, **{name: misaligned(args[name], off)}), g, name)
    for name in ("d_res_ctx", "d_pair_ctx"):  # a misaligned OUTPUT: a view into a larger pattern-filled buffer, which must stay the pattern
        view = misaligned(args[name], 4)
        whole = raw_bytes(view).clone()
        expect_refusal(dict(args, **{name: view}), g, name)
        assert torch.equal(raw_bytes(view), whole), name
    for operand, obj, field in (("grads.res_w0", g.struct, "res_w0"), ("grads.seq.b4", g.struct.seq, "b4"),
                                ("grads.layers[1].w_bias", g.layers[1], "w_bias"), ("grads.layers[0].wq_s", g.layers[0], "wq_s")):
        good = getattr(obj, field)
        setattr(obj, field, good + 4)
        expect_refusal(args, g, operand)
        setattr(obj, field, good)
    # the aligned call on the same tape and workspace: += into the pattern
    _hip.check(backward(args, g), "train_step_bwd into pattern-filled buffers")
    grads0, flat0, g0, args0 = buffers(0.0)
    args0["d_res_ctx"].fill_(3.0)  # written, not accumulated: what it held does not matter
    _hip.check(backward(args0, g0), "train_step_bwd into zero-filled buffers")
    torch.cuda.synchronize()
    # d_res_ctx is written, not accumulated: the same product twice, equal up to the order of its fp32 sums
    assert maxrel(args["d_res_ctx"], args0["d_res_ctx"]) < 1e-6
    # An accumulated element is pattern + (a sum of at most B K = 128 atomic addends, one per residue row at the worst); every addition
    # rounds to half an ulp of the running value, at most 2^-24 of max(pattern, |g|) each: 128 * 2^-24 = 7.6e-6 of that magnitude when
    # every rounding goes the same way.  2e-5 of it is the bound.
    for what, got, ref in [("parameters", flat - PATTERN, flat0), ("d_pair_ctx", args["d_pair_ctx"] - PATTERN, args0["d_pair_ctx"])]:
        err, scale = float((got - ref).abs().max()), max(PATTERN, float(ref.abs().max()))
        print(f"accumulate into the pattern, {what}: max |(buffer - pattern) - g| = {err:.3g}, max |g| = {float(ref.abs().max()):.3g}")
        assert err < 2e-5 * scale, (what, err, scale)
    assert maxrel(args0["d_res_ctx"], c["d_rc"]) < GTOL and maxrel(args0["d_pair_ctx"], c["d_pc"]) < GTOL
    for n, gr in zip(names, grads0):
        r = maxrel(gr, c["sdo"]["denoiser." + n].grad)
        assert r < GTOL, (n, r)


def by_width(v, f32=4):
    """`v` on the device, misaligned by its element size (float32: by `f32` bytes)."""
    return misaligned(v.cuda().contiguous(), {8: 8, 4: f32, 1: 1}[v.element_size()])


@gpu
@pytest.mark.parametrize("K", [64, 128])
def test_denoiser_autograd_with_misaligned_operands_vs_float64_oracle(hip, K):
    """Denoiser under autograd (diffab_denoise_step_fwd_taped / diffab_denoise_step_bwd) at NL = 2 with flat-vector parameters,
    misaligned inputs and misaligned cotangents: outputs (TOL), d x_t, d O_t, both context gradients and every parameter (GTOL) against
    the oracle case of tests/test_gpu_backward_paths.py."""
    import test_gpu_backward_paths as bp

    c = bp.cotangent_case(K, 2, 2, 21)
    assert c["margin"] > bp.MARGIN, (K, c["margin"], "inputs on a ReLU kink: pick another weight seed")
    den, _ = new_denoiser(DIMS, 21)
    den.load_state_dict(c["sd"], strict=True)
    den = den.requires_grad_(True).train()
    _, offs = flat_parameters(den)
    assert any(offs.values())
    inp = c["inp"]
    lv = {k: by_width(inp[k], 12).requires_grad_(True) for k in ARGS[1:]}
    out = den(by_width(inp["seq_idx"]), lv["translations"], lv["orientations"], lv["res_context_emb"], lv["pair_context_emb"],
              by_width(c["beta"]), None, None)
    for k, ref in c["outs"].items():
        assert maxrel(out[k], ref) < TOL, (K, k, maxrel(out[k], ref))
    torch.autograd.backward([out[k] for k in c["cot"]], [by_width(v, 8) for v in c["cot"].values()])
    for k in ARGS[1:]:
        r = maxrel(lv[k].grad, c["grads"][k])
        assert torch.isfinite(lv[k].grad).all() and r < GTOL, (K, k, r)
    check_params(den.named_parameters(), c["sdo"], "denoiser.", f"K={K} denoiser autograd, misaligned operands")


@gpu
@pytest.mark.parametrize("K", [64, 128])
def test_ipa_layer_autograd_with_misaligned_operands_vs_float64_oracle(hip, K):
    """One InvariantPointAttentionLayer under autograd (diffab_ipa_layer_fwd_taped / diffab_ipa_layer_bwd) with flat-vector parameters,
    misaligned x, e, R, t and a misaligned d y: y (TOL), d x, d e, d R, d t and the layer's parameters (GTOL) against the oracle."""
    import test_gpu_backward_paths as bp

    den, _ = new_denoiser(DIMS, 31)
    den.requires_grad_(True)
    layer = den.ipa.layers[1]
    _, offs = flat_parameters(layer)
    assert any(offs.values())
    inp = bp.gradient_inputs(2, K, seed=531 + K)
    cy = torch.randn(2, K, DIMS["D"], generator=torch.Generator().manual_seed(K + 1))
    names = ("res_context_emb", "pair_context_emb", "orientations", "translations")
    lv = {k: by_width(inp[k], 4 + 4 * (i % 3)).requires_grad_(True) for i, k in enumerate(names)}
    y = layer(*[lv[k] for k in names])
    y.backward(by_width(cy, 12))
    lo = {k: f64(inp[k]).requires_grad_(True) for k in names}
    sdo = leaves({n: p for n, p in layer.named_parameters()}, "L.")
    want = orc.ipa_layer(*[lo[k] for k in names], sdo, "L.", DIMS["H"])
    assert maxrel(y, want) < TOL, maxrel(y, want)
    (want * cy.double()).sum().backward()
    for k in names:
        r = maxrel(lv[k].grad, lo[k].grad)
        assert r < GTOL, (K, k, r)
    check_params(layer.named_parameters(), sdo, "L.", f"K={K} layer autograd, misaligned operands")


@gpu
@pytest.mark.parametrize("name", ["unfused_k64", "fused_A4"])
def test_context_encoders_with_misaligned_operands_vs_float64_oracle(hip, name):
    """encode_context forward and backward (ResidueEmbedding, PairEmbedding: the unfused launches at K = 64, the fused kernel with its
    tape at K = 128) with every parameter a view of one flat vector, every batch tensor and both cotangents misaligned: the two context
    embeddings and the 23 parameter gradients at the bars, cases and oracle of tests/test_gpu_context_encoders.py."""
    import test_gpu_context_encoders as ce

    K, A, md, ex = ce.CASES[name]
    seed, (cb, G1, G2, want) = ce.case_data(name, True, True)
    model, _ = ce.model_for(A, md, seed)
    _, offs = flat_parameters(model)
    assert any(offs.values())
    dev = {k: by_width(v, 12) for k, v in cb.items()}
    model.zero_grad(set_to_none=True)
    res, pair = model.encode_context(dev["seq_idx"], dev["xyz"], dev["orientations"], dev["backbone_dihedrals"], None,
                                     dev["pairwise_dihedrals"], dev["atom_mask"], dev["chain_idx"], dev["residue_idx"],
                                     dev["generation_mask"], dev["residue_mask"], generate_structure=True, generate_sequence=True)
    torch.autograd.backward([res, pair], [by_width(G1), by_width(G2, 8)])
    torch.cuda.synchronize()
    grads = {n: p.grad.detach().cpu() for n, p in model.named_parameters() if n.startswith((ce.RES, ce.PAIR))}
    tag = f"{name}, misaligned operands"
    ce.check_forward(tag, (res.detach().cpu(), pair.detach().cpu()), want[:2])
    ce.check_grads(tag, grads, want[2], chain0=bool((cb["chain_idx"] == 0).any()))


# ---------------------------------------------------------------------------------------------------------------- accepted entries
def _f(t):  # device float32 copy at +4
    return misaligned(t.float().cuda().contiguous(), 4)


class Held:
    """ptr(t) of tensors that stay alive as long as this object.  A temporary built inside an argument list is freed as soon as its
    pointer has been taken, and the caching allocator hands its block to the next temporary of the same call: the kernel would then read
    another operand's bytes (a timestep that is a mask byte pattern indexes the schedule far out of bounds)."""

    def __init__(self):
        self.keep = []

    def __call__(self, t):
        self.keep.append(t)
        return _hip.ptr(t)


def sweep_philox_fill(hip):
    """the float4 store of diffab_philox_fill through a pointer at every float offset: the oracle's Philox values, bitwise for the
    uniforms (tests/test_gpu_parity.py), and nothing written outside the view"""
    P = Held()
    seed, B, K = 0x1234ABCD5678, 3, 17
    patch = (7 + np.arange(B))[:, None] + np.zeros((B, K), dtype=np.int64)
    res = np.zeros((B, K), dtype=np.int64) + np.arange(K)[None]
    want_u = np.stack(orc.philox_uniform4(seed, patch, res, 42, 2), -1)
    want_n = np.stack(orc.philox_normal4(seed, patch, res, 42, 2), -1)
    for off in (0,) + F32_OFFSETS:
        for kind, want in ((1, want_u), (0, want_n)):
            big = torch.full((B * K * 4 + 16,), -3.0, device="cuda")
            lo = ((off - big.data_ptr()) % 16) // 4 + 4
            out = big[lo:lo + B * K * 4].view(B, K, 4)
            assert out.data_ptr() % 16 == off
            _hip.check(hip.diffab_philox_fill(seed, 7, B, K, 42, 2, kind, P(out), _hip.stream_ptr()), "philox_fill")
            got = out.cpu().numpy()
            assert np.array_equal(got, want.astype(np.float32)) if kind == 1 else np.abs(got - want).max() < 2e-6, (off, kind)
            assert bool((big[:lo] == -3.0).all()) and bool((big[lo + B * K * 4:] == -3.0).all()), (off, kind)


def sweep_featurize_xyz(hip):
    """diffab_featurize_xyz with xyz, the masks and all four outputs misaligned (the pairwise dihedrals' float2 store at +4 and +12)
    against orc.featurize_xyz"""
    P = Held()
    B, K, A = 2, 9, 4
    g = torch.Generator().manual_seed(5)
    xyz = torch.randn(B, K, A, 3, generator=g) * 3
    chain = (torch.arange(K) >= 5).long().expand(B, K).contiguous()
    rmask = torch.rand(B, K, generator=g) > 0.2
    want = orc.featurize_xyz(xyz, chain, rmask)
    for off in F32_OFFSETS:
        O, dih, pd = (misaligned(torch.zeros(s, device="cuda"), off) for s in ((B, K, 3, 3), (B, K, 3), (B, K, K, 2)))
        dm = misaligned(torch.zeros(B, K, 3, dtype=torch.bool, device="cuda"), 3)
        _hip.check(hip.diffab_featurize_xyz(P(misaligned(xyz.cuda(), off)), P(misaligned(chain.cuda(), 8)),
                                            P(misaligned(rmask.cuda(), 1)), B, K, A, P(O), P(dih), P(dm),
                                            P(pd), _hip.stream_ptr()), "featurize_xyz")
        # the bounds of test_featurize_xyz_vs_oracle_and_minimal_batch (tests/test_gpu_parity.py); angles compared on the circle
        assert maxrel(O, want["orientations"]) < 5e-5, off
        assert torch.equal(dm.cpu(), want["backbone_dihedrals_mask"]), off
        for gv, k in ((dih, "backbone_dihedrals"), (pd, "pairwise_dihedrals")):
            dd = (gv.cpu().double() - want[k]).abs()
            dd = torch.minimum(dd, 2 * np.pi - dd)
            assert float(dd.max()) < 2e-4 and float(dd.median()) < 1e-6, (off, k, float(dd.max()), float(dd.median()))


def sweep_patch_gather_scatter(hip):
    """diffab_patch_gather / _scatter choose 16-, 4- or 1-byte lanes from the pointers: float rows with src and dst at every offset,
    byte rows at odd offsets, against torch indexing (exact)"""
    P = Held()
    B, N, K = 2, 11, 5
    g = torch.Generator().manual_seed(6)
    index = torch.stack([torch.randperm(N, generator=g)[:K] for _ in range(B)])
    idx = misaligned(index.cuda(), 8)
    for dtype, width, offs in ((torch.float32, 8, (0, 4, 8, 12)), (torch.uint8, 3, (1, 3, 0))):
        src = (torch.randn(B, N, width, generator=g) * 50).to(dtype)
        want = torch.stack([src[b, index[b]] for b in range(B)])
        row_bytes = width * src.element_size()
        for off in offs:
            s = misaligned(src.cuda(), off) if off else src.cuda()
            dst = misaligned(torch.zeros(B, K, width, dtype=dtype, device="cuda"), off) if off else torch.zeros(B, K, width, dtype=dtype,
                                                                                                               device="cuda")
            _hip.check(hip.diffab_patch_gather(P(s), P(idx), None, B, N, B, K, row_bytes, P(dst), _hip.stream_ptr()),
                       "patch_gather")
            assert torch.equal(dst.cpu(), want), (dtype, off)
            back = misaligned(torch.zeros(B, N, width, dtype=dtype, device="cuda"), off) if off else torch.zeros(B, N, width, dtype=dtype,
                                                                                                                 device="cuda")
            _hip.check(hip.diffab_patch_scatter(P(dst), P(idx), None, B, N, K, row_bytes, P(back), _hip.stream_ptr()),
                       "patch_scatter")
            ref = torch.zeros(B, N, width, dtype=dtype)
            for b in range(B):
                ref[b, index[b]] = want[b]
            assert torch.equal(back.cpu(), ref), (dtype, off)


def sweep_so3(hip):
    """the five SO(3) maps on misaligned matrices / vectors against the oracle (1e-5 / 2e-6, the bounds of the golden test)"""
    P = Held()
    g = torch.Generator().manual_seed(7)
    n = 37
    v = torch.nn.functional.normalize(torch.randn(n, 3, generator=g), dim=-1) * (0.2 + 2.3 * torch.rand(n, 1, generator=g))  # away from 0, pi
    R = orc.rotvec_to_matrix(v.double()).float()
    k = torch.rand(n, generator=g)

    def call(fn, ins, shape, *extra):
        out = misaligned(torch.zeros(shape, device="cuda"), 12)
        _hip.check(fn(*[P(_f(t)) for t in ins], P(out), *extra, _hip.stream_ptr()), fn.__name__)
        return out.cpu()

    assert maxrel(call(hip.diffab_so3_log, [R], (n, 3, 3), n), orc.log_so3(R.double())) < 1e-5
    assert maxrel(call(hip.diffab_so3_exp, [orc.hat(v)], (n, 3, 3), n), orc.exp_so3(orc.hat(v.double()))) < 2e-6
    assert maxrel(call(hip.diffab_so3_matrix_to_rotvec, [R], (n, 3), n), orc.matrix_to_rotvec(R.double())) < 1e-5
    assert maxrel(call(hip.diffab_so3_rotvec_to_matrix, [v], (n, 3, 3), n), orc.rotvec_to_matrix(v.double())) < 2e-6
    assert maxrel(call(hip.diffab_so3_scale_rot, [R, k], (n, 3, 3), n, 1), orc.scale_rot(R.double(), k.double())) < 1e-5


def sweep_angular_encoding(hip):
    """diffab_angular_encoding and its backward on misaligned buffers against the oracle and its autograd (1e-5)"""
    P = Held()
    g = torch.Generator().manual_seed(8)
    n, nf = 29, 3
    x = torch.randn(n, generator=g)
    enc = misaligned(torch.zeros(n, 4 * nf + 1, device="cuda"), 4)
    _hip.check(hip.diffab_angular_encoding(P(_f(x)), n, nf, P(enc), _hip.stream_ptr()), "angular_encoding")
    xo = x.double().requires_grad_(True)
    want = orc.angular_encoding(xo, nf)
    assert maxrel(enc, want.detach().reshape(n, -1)) < 1e-5
    go = torch.randn(n, 4 * nf + 1, generator=g)
    (want.reshape(n, -1) * go.double()).sum().backward()
    dx = misaligned(torch.zeros(n, device="cuda"), 8)
    _hip.check(hip.diffab_angular_encoding_bwd(P(enc), P(_f(go)), n, nf, P(dx), _hip.stream_ptr()), "angular_encoding_bwd")
    assert maxrel(dx, xo.grad) < 1e-5


def sweep_losses(hip):
    """diffab_orientation_loss and diffab_losses_fwd on misaligned operands against the oracle (1e-5 / TOL)"""
    P = Held()
    g = torch.Generator().manual_seed(9)
    B, K = 2, 13
    Pm, Tm = (orc.rotvec_to_matrix(torch.randn(B, K, 3, generator=g).double()).float() for _ in range(2))
    el = misaligned(torch.zeros(B * K, 3, 3, device="cuda"), 4)
    _hip.check(hip.diffab_orientation_loss(P(_f(Pm)), P(_f(Tm)), B * K, P(el), None, _hip.stream_ptr()), "orientation_loss")
    assert maxrel(el.view(B, K, 3, 3), orc.orientation_loss_elems(Pm.double(), Tm.double())) < 1e-5
    post, tpost = (torch.softmax(torch.randn(B, K, 21, generator=g), -1) for _ in range(2))
    eps, teps = torch.randn(B, K, 3, generator=g), torch.randn(B, K, 3, generator=g)
    gm, rm = torch.rand(B, K, generator=g) > 0.4, torch.rand(B, K, generator=g) > 0.1
    out = misaligned(torch.zeros(3, device="cuda"), 12)
    _hip.check(hip.diffab_losses_fwd(P(_f(post)), P(_f(tpost)), P(_f(eps)), P(_f(teps)), P(_f(Pm)),
                                     P(_f(Tm)), P(misaligned(gm.cuda(), 1)), P(misaligned(rm.cuda(), 3)), B, K, 21,
                                     P(out), _hip.stream_ptr()), "losses_fwd")
    den = {"seq_posterior": post.double(), "translations_eps": eps.double(), "orientations_t0": Pm.double()}
    want = orc.hotpath_losses(den, tpost.double(), teps.double(), Tm.double(), gm, rm)
    np.testing.assert_allclose(out.cpu().numpy(), [float(v) for v in want], rtol=TOL)


def sweep_diffusers_and_update(hip):
    """the coordinate diffuser, the sequence's forward probabilities, draw and posterior, the weighted mix, the CDF build and the explicit-noise reverse update with every
    pointer (the schedule's tables included) misaligned, against the oracle at the bounds of tests/test_gpu_parity.py"""
    P = Held()
    g = torch.Generator().manual_seed(10)
    B, K, t = 2, 16, 33
    sched = orc.cosine_variance_schedule(100, s=0.01, beta_max=0.999)
    tabs = {k: _f(v) for k, v in sched.items()}
    sc = _hip.Sched(100, *[P(tabs[k]) for k in ("alpha", "alpha_bar", "alpha_bar_sqrt", "one_minus_alpha_bar_sqrt", "beta")])
    x0, eps = torch.randn(B, K, 3, generator=g) * 5, torch.randn(B, K, 3, generator=g)
    tt = torch.tensor([33, 90])
    gm = torch.rand(B, K, generator=g) < 0.5
    i8, m1 = (lambda v: misaligned(v.cuda(), 8)), (lambda v: misaligned(v.cuda(), 1))
    xt = misaligned(torch.zeros(B, K, 3, device="cuda"), 8)
    _hip.check(hip.diffab_coord_forward(C.byref(sc), P(_f(x0)), P(i8(tt)), P(m1(gm)), P(_f(eps)), B, K, P(xt),
                                        _hip.stream_ptr()), "coord_forward")
    assert maxrel(xt, orc.coord_diffuse_from_t0(x0, tt, gm, eps, sched)) < 1e-6
    s0 = torch.randint(0, 20, (B, K), generator=g)
    st = torch.where(gm, torch.randint(0, 20, (B, K), generator=g), s0)  # (a residue that is not generated keeps its type: one-hot posterior)
    post = misaligned(torch.zeros(B, K, 21, device="cuda"), 4)
    _hip.check(hip.diffab_seq_posterior(C.byref(sc), P(i8(st)), P(i8(s0)), P(i8(tt)), P(m1(gm)), B, K, P(post),
                                        _hip.stream_ptr()), "seq_posterior")
    assert maxrel(post, orc.seq_posterior_single_step(st, s0, tt, gm, sched)) < 2e-6
    for mode, ref in ((0, orc.seq_forward_prob_single_step), (1, orc.seq_forward_prob_from_t0)):
        prob = misaligned(torch.zeros(B, K, 21, device="cuda"), 8)
        _hip.check(hip.diffab_seq_forward_prob(C.byref(sc), mode, P(i8(s0)), P(i8(tt)), P(m1(gm)), B, K, P(prob), _hip.stream_ptr()),
                   "seq_forward_prob")
        want_p = ref(s0, tt, gm, sched)
        assert maxrel(prob, want_p) < 3e-7, mode
    u = torch.rand(B, K, generator=g)
    draw = misaligned(torch.zeros(B, K, dtype=torch.int64, device="cuda"), 8)
    _hip.check(hip.diffab_categorical_sample(P(_f(want_p)), P(_f(u)), B * K, 21, P(draw), _hip.stream_ptr()), "categorical_sample")
    assert torch.equal(draw.cpu(), orc.categorical_from_uniform(want_p, u))  # (the same fp32 prefix sums in the same order: exact)
    p1, p2 = torch.rand(B, K, 21, generator=g), torch.rand(B, K, 21, generator=g)
    w1, w2 = torch.rand(B, generator=g), torch.rand(B, generator=g)
    mix = misaligned(torch.zeros(B, K, 21, device="cuda"), 12)
    _hip.check(hip.diffab_weighted_multinomial(P(_f(p1)), P(_f(p2)), P(_f(w1)), P(_f(w2)), B * K * 21, K * 21,
                                               P(mix), _hip.stream_ptr()), "weighted_multinomial")
    assert maxrel(mix, orc.weighted_multinomial(p1, p2, w1, w2)) < 3e-7
    pdf = torch.rand(5, 64, generator=g)
    cdf = misaligned(torch.zeros(5, 64, device="cuda"), 4)
    _hip.check(hip.diffab_igso3_cdf_build(P(_f(pdf)), 5, 64, P(cdf), _hip.stream_ptr()), "igso3_cdf_build")
    assert maxrel(cdf, orc.igso3_cdf_table(pdf)) < 5e-6
    x, O = torch.randn(B, K, 3, generator=g) * 5, orc.rotvec_to_matrix(torch.randn(B, K, 3, generator=g))
    seq = torch.randint(0, 20, (B, K), generator=g)
    den = {"translations_eps": torch.randn(B, K, 3, generator=g), "orientations_t0": orc.rotvec_to_matrix(torch.randn(B, K, 3, generator=g)),
           "seq_posterior": torch.rand(B, K, 21, generator=g).softmax(-1)}
    z, rv, u = torch.randn(B, K, 3, generator=g), torch.randn(B, K, 3, generator=g) * 0.3, torch.rand(B, K, generator=g)
    s1, x1, O1 = orc.reverse_update(t, seq, x, O, den, gm, sched, z, rv, u)
    sq, xq, Oq = i8(seq), _f(x), _f(O)
    keep = [_f(den["translations_eps"]), _f(den["orientations_t0"]), _f(den["seq_posterior"]), misaligned(gm.cuda(), 3), _f(z), _f(rv), _f(u)]
    _hip.check(hip.diffab_reverse_update(C.byref(sc), t, P(sq), P(xq), P(Oq), *[P(v) for v in keep], B, K, 21,
                                         _hip.stream_ptr()), "reverse_update")
    assert maxrel(xq, x1) < 1e-6 and maxrel(Oq, O1) < 1e-6 and torch.equal(sq.cpu(), s1)


# Every ACCEPTS export runs on the device with misaligned pointers: through one of the sweeps above, or (RERUNS) through the test of its
# own file - the host reference that file already uses - rerun on top of MisalignedABI, which hands the entry a misaligned copy of
# every tensor and copies back what the entry wrote.
SWEEPS = {"diffab_philox_fill": sweep_philox_fill, "diffab_featurize_xyz": sweep_featurize_xyz,
          "diffab_patch_gather": sweep_patch_gather_scatter, "diffab_patch_scatter": sweep_patch_gather_scatter,
          "diffab_so3_log": sweep_so3, "diffab_so3_exp": sweep_so3, "diffab_so3_matrix_to_rotvec": sweep_so3,
          "diffab_so3_rotvec_to_matrix": sweep_so3, "diffab_so3_scale_rot": sweep_so3,
          "diffab_angular_encoding": sweep_angular_encoding, "diffab_angular_encoding_bwd": sweep_angular_encoding,
          "diffab_orientation_loss": sweep_losses, "diffab_losses_fwd": sweep_losses,
          "diffab_coord_forward": sweep_diffusers_and_update, "diffab_seq_posterior": sweep_diffusers_and_update,
          "diffab_seq_forward_prob": sweep_diffusers_and_update, "diffab_categorical_sample": sweep_diffusers_and_update,
          "diffab_weighted_multinomial": sweep_diffusers_and_update, "diffab_igso3_cdf_build": sweep_diffusers_and_update,
          "diffab_reverse_update": sweep_diffusers_and_update}

# id: (entries that must have run misaligned, test module, test function, fixtures, arguments or module -> arguments, float offsets)
RERUNS = {
    "frames": (("diffab_frames_apply", "diffab_frames_invert", "diffab_frames_bwd"), "test_gpu_autograd",
               "test_frames_and_angular_encoding_vs_reference_goldens", ("hip", "golden"), (), (4, 12)),
    "orientation_loss_bwd": (("diffab_orientation_loss_bwd",), "test_gpu_autograd", "test_orientation_loss_autograd_vs_reference_goldens",
                             ("hip", "golden"), (), (4, 12)),
    "igso3_tables": (("diffab_igso3_table_build", "diffab_igso3_table_build_accurate"), "test_gpu_parity", "test_igso3_table_vs_golden",
                     ("hip", "golden"), (), (4,)),
    "igso3_sample_orient_forward": (("diffab_igso3_sample", "diffab_orient_forward"), "test_gpu_parity",
                                    "test_igso3_sampler_and_orientation_diffuser_vs_golden", ("hip", "golden"), (), (4, 12)),
    "igso3_bins": (("diffab_igso3_bins_without_replacement", "diffab_igso3_sample_bins"), "test_gpu_parity",
                   "test_igso3_bins_without_replacement", ("hip",), (), (12,)),
    "reverse_update_jump": (("diffab_reverse_update_jump",), "test_gpu_respaced", "test_jump_known_answers_of_an_exact_denoiser",
                            ("respaced_bench",), (), (12,)),
    "patch_select": (("diffab_patch_select",), "test_gpu_patch", "test_float_selection_equals_the_oracle", ("hip",), (97, 0), (4, 12)),
    "metrics_vs_native": (("diffab_metrics_vs_native",), "test_gpu_metrics", "test_evaluate_equals_the_oracle", (),
                          (128, "backbone", 5, True), (4, 12)),
    "metrics_pairwise": (("diffab_metrics_pairwise",), "test_gpu_metrics", "test_pairwise_equals_the_oracle", (), (3, 65, "backbone", True),
                         (4, 12)),
    "metrics_select_diverse": (("diffab_metrics_select_diverse",), "test_gpu_metrics", "test_select_diverse_equals_the_oracle", (), (), (4, 12)),
    "metrics_backbone": (("diffab_metrics_backbone",), "test_gpu_geometry", "test_backbone_equals_the_oracle", (), (5, 40), (4, 12)),
    "metrics_contacts": (("diffab_metrics_contacts",), "test_gpu_geometry", "test_contacts_equal_the_oracle", (), (5, 40), (4, 12)),
    "metrics_ensemble": (("diffab_metrics_ensemble",), "test_gpu_ensemble", "test_ensemble_equals_the_oracle", (),
                         ((3, 5, 70), "backbone", True), (4, 12)),
    "metrics_similarity": (("diffab_metrics_similarity",), "test_gpu_similarity", "test_similarity_equals_the_restatement_and_the_oracle", (),
                           lambda m: (m.SHAPES[0], list(m.VARIANTS)[0]), (4, 12)),
    "refine_backbone": (("diffab_refine_backbone",), "test_gpu_refine", "test_refinement_against_the_oracle", (),
                        lambda m: (m.SHAPES[0], 7), (4, 12)),
    "guidance_energy": (("diffab_guidance_energy",), "test_gpu_guidance", "test_energy_against_float64", ("hip",), (77,), (4, 12)),
    "steer_resample": (("diffab_steer_resample",), "test_gpu_steering", "test_resample_kernel_against_the_oracle", ("hip",), (65,), (4, 12)),
    "steer_gather": (("diffab_steer_gather",), "test_gpu_steering", "test_gather_is_indexing", ("hip",), (5,), (4, 12)),
    "steer_energy": (("diffab_steer_energy",), "test_gpu_steering", "test_energy_against_float64_at_x0_hat", ("hip", "steering_unit"), (5,),
                     (4, 12)),
    "sample_init": (("diffab_sample_init", "diffab_sample_init_ex", "diffab_sample_init_noised"), "test_gpu_aa_constraints",
                    "test_init_and_noised_start_vs_rules", ("aa_unit",), (), (4, 12)),
    # the two diagnostics whose kernels are picked from the pointers: A, B, C and db of the weight-gradient product (a_vec / b_vec of
    # gemm_tn_b6 / _h3) at a vector-wide and at a narrow shape, X, W, bias and Y of the f32 dense product (launch_linear: rowgemm128,
    # the tiled kernel's vector loads, or its scalar loads) - mode 0 only, modes 1 and 2 refuse misaligned operands
    "debug_gemm_tn": (("diffab_debug_gemm_tn",), "test_gpu_parity", "test_weight_gradient_product_is_fp32_accurate", ("hip",),
                      (16384, 128, 1024), (4, 8, 12)),
    "debug_gemm_tn_narrow": (("diffab_debug_gemm_tn",), "test_gpu_parity", "test_weight_gradient_product_is_fp32_accurate", ("hip",),
                             (128, 3, 128), (4,)),
    "debug_linear128_mode0": (("diffab_debug_linear128",), "test_gpu_parity", "test_split_precision_gemm_is_fp32_accurate", ("hip",), (128,),
                              (4, 8, 12)),
    # the accepted operands of two entries that refuse others: seq, x, O, the masks, the schedule, the IGSO3 table, out_terms,
    # out_residue and the noised copies of diffab_score_designs; seq, the mask, the schedule and the table of diffab_sample_loop_ex
    "score_designs_noised": (("diffab_score_designs",), "test_gpu_score", "test_noised_state_vs_oracle", ("score_unit",), (), (4, 12)),
    "score_designs_terms": (("diffab_score_designs",), "test_gpu_score", "test_terms_vs_oracle_unit", ("score_unit",), (), (4, 12)),
    "sample_loop": (("diffab_sample_loop_ex",), "test_gpu_parity", "test_reverse_step_teacher_forced_vs_oracle", ("hip",), (), (4, 12)),
    # the analysis header's entry (include/diffab_hip_analysis.h), at the smallest parametrisation of its oracle test
    "metrics_surface": (("diffab_metrics_surface",), "test_gpu_surface", "test_surface_equals_the_oracle", (), (24, 8, False, 1, 33), (4, 12)),
}
# diffab_debug_row_tiles / _row_plan read a mask byte by byte and write bytes / int32 (diffusion_kernels.hip tiles_needed_kernel, row_plan):
# the sample loop's own calls of the same launchers run in every reverse-step case; the debug exports have no misaligned case
UNSWEPT = {"diffab_debug_row_tiles", "diffab_debug_row_plan"}
RERUN_WHEN = {"diffab_debug_linear128": lambda args: args[6] == 0}
COVERED = {n for row in RERUNS.values() for n in row[0]}


def accepted_positions(entry):
    """Argument indices of a REFUSES entry's accepted operands (SIGNATURES)."""
    return {i for i, (_, kind) in enumerate(signature(entry)) if kind in ("fa", "i64", "m", "S", "I", "N")}


@gpu
@pytest.mark.parametrize("case", sorted(RERUNS))
def test_entries_rerun_their_own_reference_test_with_misaligned_pointers(request, case):
    """The test an entry's own file holds (its host reference, its bounds), rerun with every pointer of the entry misaligned at the C
    ABI, once per float offset; the entry must have been called with replaced pointers."""
    import importlib

    entries, module, function, fixtures, args, offsets = RERUNS[case]
    mod = importlib.import_module(module)
    args = args(mod) if callable(args) else args
    values = {f: request.getfixturevalue(f) for f in fixtures}  # (models are built on the real library, before the stand-in)
    positions = {e: accepted_positions(e) for e in entries if e in SIGNATURES}
    for off in offsets:
        with MisalignedABI(entries, f32=off, positions=positions, when=RERUN_WHEN) as abi:
            if "hip" in values:
                values["hip"] = abi
            getattr(mod, function)(*[values[f] for f in fixtures], *args)
        torch.cuda.synchronize()
        for e in entries:
            assert abi.counts.get(e, 0) > 0, (case, e, off, "was not called with a misaligned pointer")
        print(f"{case} at +{off}: pointers replaced {abi.counts}")


def test_every_export_is_in_the_table():
    """The table is the two headers' list of exports: one missing from it, or one it names that the headers no longer have, fails here
    (no GPU needed).  Every ACCEPTS entry runs misaligned on the device, in a sweep or a rerun; UNSWEPT names the two that do not."""
    exports = header_exports()
    assert sorted(ENTRIES) == exports, (sorted(set(exports) - set(ENTRIES)), sorted(set(ENTRIES) - set(exports)))
    assert set(SWEEPS) | (COVERED - set(SIGNATURES) - set(DEBUG_REFUSES)) == {n for n, c in ENTRIES.items() if c == ACCEPTS} - UNSWEPT, \
        sorted({n for n, c in ENTRIES.items() if c == ACCEPTS} - UNSWEPT - set(SWEEPS) - COVERED)
    assert {n for n, c in ENTRIES.items() if c == REFUSES} == set(SIGNATURES) | set(DEBUG_REFUSES)


@gpu
@pytest.mark.parametrize("sweep", sorted(set(SWEEPS.values()), key=lambda f: f.__name__), ids=lambda f: f.__name__[6:])
def test_accepted_entries_with_misaligned_pointers_vs_host_reference(hip, sweep):
    sweep(hip)
    print(sweep.__name__, "covers", sorted(n for n, f in SWEEPS.items() if f is sweep), "-", " ".join(sweep.__doc__.split()))
