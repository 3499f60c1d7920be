"""The dense tiles of the MFMA path at the row counts where they change their launch form (tests/launch_forms.py has the cases,
tests/test_launch_forms_host.py what each selects; DESIGN 4.3 the selector table).

The launchers pick a kernel instantiation from rows = B K alone.  Until this file the suite ran large batches at K = 128 only, where
rows % 128 == 0, and K = 64 / 192 at B <= 3, so the ragged forms of large batches and the unsplit x-stationary forms were compiled and
never run.  What each group below reaches, at the benchmark dims (D = 128, C = 64, H = 8, DS = 32, P = 8), NL = 2:

  1. diffab_debug_linear128 (no parts scratch): mode 0 rowgemm128_kernel (one instantiation, M guarded), mode 1 rowgemm128_b6_kernel<.,G>,
     mode 2 rowgemm128_h3_kernel<.,G>; G = 64 at M = 32640 (510 groups), G = 128 at M = 32641 (last group 1 row), 32704 (64 rows),
     32768 (exact); Kd = 1344 (21 k pairs, the backward's d x of the projections) at M = 32704.
  2. diffab_debug_xstat128: mode 1 proj_frames_b6_kernel<FULL, SPLIT> without frames, mode 2 xstat_h3_kernel<FULL, SPLIT>; M = 16384
     <true, true> with two groups per row tile (the last split batch), 16512 <true, false>, 16385 and 16448 <false, false> (1 and 64 rows in
     tile 129); N = 1024: 11 column blocks (12 in the bf16 form) walked by one group, N = 100: a partial last block.
  3. Denoiser.forward -> diffab_denoise_step_fwd (denoise_step, one launch per kernel: the module launch is K = 128 / 256 only).
       flags 0 and PAIR_PLANES: embedding MLP launch_mlp_chain_b6 and the three heads launch_mlp_chains_b6 (ceil(rows / 128) groups, the
       last one guarded by row < M: 64 rows at every odd B); per layer (ipa_layer_fast) launch_proj_frames_h3p ->
       proj_frames_h3_kernel<FULL, SPLIT>, ipa_attn_fast_kernel<4, MULTI, PLANES> (K = 64: one chunk of 4 key tiles; K = 192: three
       chunks, MULTI), launch_rowgemm128_h3p with parts scratch (Kd = 1024: 16 k parts).
         K = 64:  B = 1, 3 rowgemm128_h3_parts_kernel<64> + proj<false, true> (nsplit 14); B = 64 the last batch of the parts form (64
                  tiles), proj<true, true> (nsplit 8); B = 65 rowgemm128_h3_kernel<false, 64>, proj<false, true> (nsplit 7); B = 257
                  <false, 64>, proj<false, false>; B = 511 rowgemm128_h3_kernel<false, 128> with a 64-row last group, proj<false, false>.
         K = 192: B = 1, 3 parts; B = 23 <false, 64>, nsplit 7; B = 87 <false, 64>, proj<false, false>; B = 171 <false, 128> ragged,
                  proj<false, false>.
       FP32_GEMM: embedding and heads launch_rowgemm128 (rowgemm128_kernel; below 128 rows launch_linear_bn) and launch_linear; per layer
       launch_proj_frames_f32 -> proj_frames_kernel<FULL> (<false> at every B above but K = 64, B = 64), the fp32 attention kernel,
       launch_linear -> rowgemm128_kernel for to_out.
  4. Denoiser under autograd (_DenoiserFn), K = 64, B = 257 and 511: diffab_denoise_step_fwd_taped (denoise_step_taped: embedding and
     heads launch_linear; per layer launch_proj_frames_h3p<false, false> from the tape's planes, the three-launch attention,
     launch_rowgemm128_h3p WITHOUT parts: <false, 64> / <false, 128> ragged), then diffab_denoise_step_bwd (run_backward): per layer d feat
     = d y W_out through launch_xstat_h3 -> xstat_h3_kernel<false, false> (N = 1024), d x of the six projections through
     launch_rowgemm128_b6p (Kd = 1344, no parts) -> rowgemm128_b6_kernel<false, 64> / <false, 128> ragged; the weight gradients through
     launch_gemm_tn_h3 (M moves its chunking only: tests/test_gpu_parity.py).

Oracle: float64 products on the device (1, 2), oracle/diffab_oracle.py in float64 on the host for the compared patches only (3, 4) -
patches are independent in the denoiser, so a patch's outputs and input gradients are those of a batch that holds it alone.
"""
import pytest
import torch

import diffab_oracle as orc
from conftest import elemrel, maxrel
from diffab_pytorch import _hip, synthetic as syn
from launch_forms import BACKWARD_B, FORWARD_B, LINEAR_CASES, LINEAR_M, PJ_NB, XSTAT_BWD_NB, XSTAT_M, XSTAT_N, dense_forms, xstat_blocks
from sampler_support import ARGS, GTOL, OUTS, PATCH_LENGTH_DIMS, TOL, device_patches, f64, hip, leaves, n_real_of, padded, relu_margin

pytestmark = pytest.mark.gpu
DIMS = PATCH_LENGTH_DIMS
BAR = 2e-6  # |error| / sum |x w| of a split-precision product (tests/test_gpu_parity.py)


# ------------------------------------------------------------------ 1. the row GEMM at the 64- / 128-row threshold
@pytest.mark.parametrize("M,Kd", LINEAR_CASES)
def test_row_gemm_at_the_group_size_threshold_is_fp32_accurate(hip, M, Kd):
    """test_split_precision_gemm_is_fp32_accurate's operands and bars at the row counts around ceil(M / 128) = 256, where the bf16 x 6 and
    fp16 x 3 kernels change from 64- to 128-row groups; two sentinel rows behind Y come back untouched."""
    group, ragged = LINEAR_M[M]
    got = dense_forms(hip, M, 1, 0)
    print(f"M={M} Kd={Kd}: dense forms {got}")
    assert got[:2] == (group, ragged)
    g = torch.Generator(device="cuda").manual_seed(M + Kd)
    X = torch.randn(M, Kd, device="cuda", generator=g) * torch.exp(3 * torch.randn(M, 1, device="cuda", generator=g))
    W = torch.randn(128, Kd, device="cuda", generator=g) * 0.1 * torch.exp(2 * torch.randn(128, 1, device="cuda", generator=g))
    b = torch.randn(128, device="cuda", generator=g)
    want = X.double() @ W.double().T + b.double()
    scale = (X.double().abs() @ W.double().abs().T) + b.double().abs()
    scratch = torch.empty(3 * 128 * Kd * 2 + 256, dtype=torch.uint8, device="cuda")
    errs = {}
    for mode in (0, 1, 2):
        Y = torch.full((M + 2, 128), 7.0, device="cuda")
        rc = hip.diffab_debug_linear128(_hip.ptr(X), _hip.ptr(W), _hip.ptr(b), _hip.ptr(Y), M, Kd, mode, _hip.ptr(scratch), scratch.numel(),
                                        _hip.stream_ptr())
        assert rc == 0, hip.diffab_last_error()
        assert torch.isfinite(Y).all() and bool((Y[M:] == 7.0).all()), mode
        errs[mode] = float(((Y[:M].double() - want).abs() / scale).max())
    print(f"M={M} Kd={Kd}: max |err| / sum|x w|: f32 MFMA {errs[0]:.2e}, bf16x6 {errs[1]:.2e}, fp16x3 {errs[2]:.2e}")
    assert errs[0] < BAR and errs[1] < BAR and errs[2] < BAR, errs
    assert errs[1] < 4 * errs[0] + 1e-7, errs
    assert errs[2] < 4 * errs[0] + 4e-7, errs


# ------------------------------------------------------------------ 2. the x-stationary product past 128 row tiles
@pytest.mark.parametrize("N", XSTAT_N)
@pytest.mark.parametrize("M", sorted(XSTAT_M))
def test_x_stationary_product_unsplit_forms_are_fp32_accurate(hip, M, N):
    """test_x_stationary_backward_product_is_fp32_accurate's operands and bars where a row tile has ONE work-group that walks every column
    block (rows > 16384: the training backward at more than 128 patches of 128 residues per GPU), full and ragged, beside the last split
    row count; two sentinel rows behind Y."""
    full, nsplit, last = XSTAT_M[M]
    for mode in (1, 2):
        got = dense_forms(hip, M, xstat_blocks(N, mode), 0)
        print(f"M={M} N={N} mode {mode}: dense forms {got}")
        assert got[2:] == (full, nsplit, last)
    g = torch.Generator(device="cuda").manual_seed(M + N)
    X = torch.randn(M, 128, device="cuda", generator=g) * 1e-4 * torch.exp(3 * torch.randn(M, 1, device="cuda", generator=g))
    X[7] = 0.0
    W = torch.randn(128, N, device="cuda", generator=g) * 0.1 * torch.exp(2 * torch.randn(1, N, device="cuda", generator=g))
    want = X.double() @ W.double()
    scale = X.double().abs() @ W.double().abs() + 1e-300
    nb = (N + 95) // 96
    scratch = torch.empty(3 * 2 * nb * 96 * 128 * 2 + nb * 96 * 4 + 256, dtype=torch.uint8, device="cuda")
    errs = {}
    for mode in (1, 2):
        Y = torch.full((M + 2, N), 7.0, device="cuda")
        rc = hip.diffab_debug_xstat128(_hip.ptr(X), _hip.ptr(W), _hip.ptr(Y), M, N, mode, _hip.ptr(scratch), scratch.numel(), _hip.stream_ptr())
        assert rc == 0, hip.diffab_last_error()
        assert torch.isfinite(Y).all() and bool((Y[M:] == 7.0).all()) and bool((Y[7] == 0.0).all()), mode
        errs[mode] = float(((Y[:M].double() - want).abs() / scale).max())
    print(f"M={M} N={N}: max |err| / sum|x w|: bf16x6 {errs[1]:.2e}, fp16x3 {errs[2]:.2e}")
    assert errs[1] < BAR and errs[2] < BAR, errs
    assert errs[2] < 4 * errs[1] + 4e-7, errs


# ------------------------------------------------------------------ 3. the real forward at every form
def denoiser(seed):
    from diffab_pytorch.diffab_pytorch import Denoiser

    d = DIMS
    den = Denoiser(d["D"], d["C"], d["NL"], d["DS"], d["PQ"], d["PV"], d["H"], 21)
    sd = syn.denoiser_state_dict(d, seed=seed, prefix="")
    den.load_state_dict(sd, strict=True)
    return den.cuda(), sd


_FWD = {}  # the inputs of ONE K at a time (K = 192: a 1.6 GB pair tensor)


def forward_case(K):
    if _FWD.get("K") != K:
        _FWD.clear()
        torch.cuda.empty_cache()
        den, sd = denoiser(seed=K + 40)
        den.requires_grad_(False)
        Bmax = max(FORWARD_B[K])
        inp = device_patches(Bmax, K, DIMS, seed=800 + K)
        beta = torch.linspace(0.02, 0.9, Bmax, device="cuda")
        tail = {k: inp[k][-3:].cpu() for k in ARGS}
        want = orc.denoiser({"denoiser." + k: v.double() for k, v in sd.items()}, tail["seq_idx"], *[tail[k].double() for k in ARGS[1:]],
                            beta[-3:].cpu().double(), DIMS["NL"], DIMS["H"])
        _FWD.update(K=K, den=den, inp=inp, beta=beta, want=want, Bmax=Bmax)
    return _FWD


def run_forward(case, lo, hi, flags):
    """The patches lo .. hi - 1 of the case's inputs as a batch of their own."""
    out = case["den"](*[case["inp"][k][lo:hi] for k in ARGS], case["beta"][lo:hi], None, None, return_logits=True, flags=flags)
    return {k: out[k] for k in OUTS}


@pytest.mark.parametrize("flags", [0, _hip.FLAG_PAIR_PLANES, _hip.FLAG_FP32_GEMM], ids=["dispatch", "pairplanes", "fp32gemm"])
@pytest.mark.parametrize("K", sorted(FORWARD_B))
def test_forward_at_every_launch_form(hip, K, flags):
    """The batch is the LAST B patches of one set of inputs, so the last patch always ends in the ragged tile.  (a) the last min(B, 3)
    patches against the float64 oracle at TOL, as test_gpu_patch_lengths.check_forward does; (b) the same bits as the B = 3 run at every
    B (a patch's bits do not depend on its batch); (c) at the largest B the first two patches - interior tiles - are
    bit-equal to a run of those two alone.  DESIGN 4.3 makes its statement for the split-precision tiles (same operations in every launch
    shape); the fp32 kernels of FLAG_FP32_GEMM change kernel below 128 rows (launch_linear_bn) and carry no such statement: there (b)
    and (c) print the number of differing elements and (a) holds.
    Regression: K = 64, B = 1 (64 rows) used to fail (b) in all five outputs (res_emb: 7306 of 8192 elements) - plan_forward gated the
    bf16 x 6 MLP chains on the fp32 row GEMM's M >= 128, so a single 64-residue patch ran its embedding MLP and heads on the unfolded fp32
    kernels and its bits differed from the same patch in any larger batch."""
    case = forward_case(K)
    Bmax, want = case["Bmax"], case["want"]
    bitwise = flags != _hip.FLAG_FP32_GEMM
    ref3 = run_forward(case, Bmax - 3, Bmax, flags)
    worst, unequal = {"maxrel": 0.0, "elemrel": 0.0}, []
    for B in sorted(FORWARD_B[K]):
        got = dense_forms(hip, B * K, PJ_NB, 1)
        print(f"K={K} B={B} flags={flags}: dense forms {got}")
        assert got == FORWARD_B[K][B]
        out = ref3 if B == 3 else run_forward(case, Bmax - B, Bmax, flags)
        n = min(B, 3)
        for k in OUTS:
            o, ref = out[k][-n:].cpu(), want[k][-n:]
            assert o.shape == ref.shape and torch.isfinite(o).all(), (K, B, flags, k)
            mr, er = maxrel(o, ref), elemrel(o, ref)
            worst = {"maxrel": max(worst["maxrel"], mr), "elemrel": max(worst["elemrel"], er)}
            assert mr < TOL and er < TOL, (K, B, flags, k, mr, er)
            differ = int((out[k][-n:] != ref3[k][-n:]).sum())
            if differ:
                print(f"K={K} B={B} flags={flags}: {k} differs from the B = 3 run in {differ} of {o.numel()} elements")
                unequal.append((B, k, differ))
    print(f"K={K} flags={flags}: worst vs the float64 oracle over every B and output: maxrel {worst['maxrel']:.2e}, "
          f"elemrel {worst['elemrel']:.2e} (bar {TOL:.0e})")
    full, two = out, run_forward(case, 0, 2, flags)  # (the loop's last run is the whole set of inputs)
    assert B == Bmax
    for k in OUTS:
        differ = int((full[k][:2] != two[k]).sum())
        if differ:
            print(f"K={K} flags={flags}: {k} of the first two patches differs between B = {Bmax} and B = 2 in {differ} elements")
            unequal.append(("interior", k, differ))
    assert not (bitwise and unequal), (K, flags, unequal)


# ------------------------------------------------------------------ 4. the backward's input-gradient products at the large forms
# Weight seeds whose float64 ReLU pre-activations on the two compared patches all lie more than 5e-7 from 0 (`relu_margin`, a property
# of the oracle alone: chosen on the host, asserted below).
BWD_WEIGHT_SEED = {257: 328, 511: 583}  # margins 2.0e-5 and 1.5e-5 (of ten seeds tried each, the widest)


@pytest.mark.parametrize("B", sorted(BACKWARD_B))
def test_input_gradients_of_a_large_batch_vs_float64_oracle(hip, B):
    """BWD_COTANGENTS at K = 64 with 257 and 511 patches: x-stationary d feat without column split in its ragged form, d x of the
    projections on 64- and on ragged 128-row groups.  The last two patches are test_denoiser_cotangent_gradients_vs_float64_oracle's
    (patch 0 padded, seeded random cotangents, the contexts and frames as leaves); their input gradients against the float64 oracle on
    those two patches alone at GTOL.  Parameter gradients of the whole batch: finite and non-zero."""
    K = 64
    got = dense_forms(hip, B * K, XSTAT_BWD_NB, 0)
    print(f"backward K={K} B={B}: dense forms {got}")
    assert got == BACKWARD_B[B]
    den, sd = denoiser(seed=BWD_WEIGHT_SEED[B])
    den.train()
    inp = device_patches(B, K, DIMS, seed=900 + B)
    tail = padded(2, K, n_real_of(K), seed=200 + K + B)
    for k in ARGS:
        inp[k][-2:] = tail[k].cuda()
    beta_tail = torch.tensor([0.05, 0.4])
    beta = torch.linspace(0.02, 0.9, B, device="cuda")
    beta[-2:] = beta_tail.cuda()
    g = torch.Generator().manual_seed(K + B)
    cot_tail = {"translations_eps": torch.randn(2, K, 3, generator=g), "orientations_t0": torch.randn(2, K, 3, 3, generator=g),
                "seq_posterior": torch.randn(2, K, 21, generator=g)}
    gd = torch.Generator(device="cuda").manual_seed(K + B)
    cot = {k: torch.randn(B, *c.shape[1:], device="cuda", generator=gd) for k, c in cot_tail.items()}
    for k, c in cot_tail.items():
        cot[k][-2:] = c.cuda()
    lo = {k: f64(tail[k]).requires_grad_(True) for k in ARGS[1:]}
    sdo = leaves(sd, "denoiser.")
    want = orc.denoiser(sdo, tail["seq_idx"], lo["translations"], lo["orientations"], lo["res_context_emb"], lo["pair_context_emb"],
                        beta_tail.double(), DIMS["NL"], DIMS["H"])
    sum((want[k] * c.double()).sum() for k, c in cot_tail.items()).backward()
    assert relu_margin(sd, tail["seq_idx"], tail["res_context_emb"], want, beta_tail) > 5e-7, "inputs on a ReLU kink: pick another weight seed"
    lv = {k: inp[k].requires_grad_(True) for k in ARGS[1:]}
    out = den(inp["seq_idx"], lv["translations"], lv["orientations"], lv["res_context_emb"], lv["pair_context_emb"], beta, None, None)
    for k in cot_tail:
        assert maxrel(out[k][-2:].detach(), want[k].detach()) < TOL, (B, k)
    sum((out[k] * cot[k]).sum() for k in cot).backward()
    worst = 0.0
    for k in ARGS[1:]:
        assert torch.isfinite(lv[k].grad).all(), (B, k)
        r = maxrel(lv[k].grad[-2:], lo[k].grad)
        worst = max(worst, r)
        print(f"backward K={K} B={B}: d {k} of the last two patches vs the oracle {r:.2e}")
        assert r < GTOL, (B, k, r)
    print(f"backward K={K} B={B}: worst input gradient {worst:.2e} (bar {GTOL:.0e})")
    for n, p in den.named_parameters():
        assert p.grad is not None and torch.isfinite(p.grad).all() and float(p.grad.abs().max()) > 0, (B, n)
