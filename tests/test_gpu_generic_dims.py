"""The any-dims denoiser, its backward and the sampler step at model dims other than the unit and benchmark ones, against the float64 oracle.

Every geometry that is not the benchmark one (fast_path_supported: D = 128, C = 64, H = 8, DS = 32, PQ = PV = 8, K % 64 == 0) runs on
denoiser_generic.hip, the launch_linear MLP kernels and the generic half of run_backward (csrc/denoiser_backward.hip: the VALU row and
key passes of choose_attn_bwd).  Those branch on
H, on PQ against PV, on DS / C / 3 PQ / 3 PV modulo 4 and on the attention's LDS need; the cases below pick each branch (confirmed by a
kernel trace, profiles/generic_dims.md):

  id         B    K    D   C   H  DS PQ PV NL  reaches
  odd        3   37   35   6   3   7  3  5  2  linear_mfma_kernel<64, *, false>; generic attention at H = 3, PQ != PV; backward
                                               ipa_attn_bwd_rows_kernel with vec = 0, ipa_attn_bwd_keys_kernel (K % 4 != 0), per-projection
                                               linear_bwd, the VALU gemm_nn / gemm_tn fallbacks
  odd_k5     2    5   (as odd)             2  K far below a wave: softmax and key loops with idle lanes
  af2        2  128  128  64  12  16  4  8  2  AlphaFold 2's IPA head shape.  rowgemm128 embedding, linear_mfma_kernel<128, *, false> head
                                               (Kd = 131); backward rows kernel at H = 12 (vec = 1), keys_mr<4>, to_out through xstat_h3,
                                               per-projection linear_bwd (H PQ 3 = 144 is not a multiple of 64)
  h4         2   96   96  32   4  16  4  4  3  linear_mfma_kernel<128, *, true> and <128, *, false>; rows_mr<4, 0> at H = 4, keys_mr<4>
  segs64     2   64   64  16   8   8  8  8  2  the segmented projection backward at D = 64 (one gemm_tn over the six weight segments,
                                               a segmented gemm_nn for d x)
  d128_ds24  2  100  128  64   8  24  8  8  2  generic attention (DS != 32) under the split-plane dense products: segmented gemm_tn,
                                               wsplit128_segs + rowgemm128_b6p for d x
  lds_rows   1  384   32   8  16   8  4  4  1  the backward row kernel above 64 KiB of dynamic LDS; the one-key kernel at 48 KiB
  lds_keys   1  136   32   8  64   8  4  4  1  the row kernel at 118 KiB, the one-key kernel at 68 KiB (its LDS attribute)
  refused    1  256   32   4  64   8  4  4  1  the forward's generic attention at 72 KiB (attribute branch); the backward would need
                                               207 KiB: the taped forward refuses it before anything is launched

The two largest LDS cases reach their bytes with many heads rather than long patches: at H = 16, K = 544 / 1024 the fp32 sums over the
keys alone put res_emb's element-wise error at 1.5e-4 (max-rel 3e-6; the host's fp32 restatement of the same step is at 6e-5), past
TOL for rounding, not for a wrong kernel.

Oracle: oracle/diffab_oracle.py in float64 on the host under torch autograd, computed once per case.  Patch 0 is padded as collate does
(`padded`) and every patch has a CDR-sized generated block.  Weight seeds keep every ReLU pre-activation at least 5e-7 away from 0
(`relu_margin`).  Bars: TOL (1e-4) for forward values, max-rel and element-wise; GTOL (2e-4) for gradients; rtol 5e-5 for the losses.
"""
import numpy as np
import pytest
import torch

import diffab_oracle as orc
from conftest import elemrel, maxrel
from diffab_pytorch import _hip, synthetic as syn
from sampler_support import ARGS, FLAGS, FLAG_IDS, GTOL, OUTS, TOL, check_params, f64, hip, leaves, oracle_reverse_step, padded, relu_margin

pytestmark = pytest.mark.gpu
MARGIN = 5e-7
# id: B, K, D, C, H, DS, PQ, PV, NL, weight seed (a seed whose ReLU margin is > MARGIN in every mode that uses it)
GEOMS = {
    "odd": (3, 37, 35, 6, 3, 7, 3, 5, 2, 1),
    "odd_k5": (2, 5, 35, 6, 3, 7, 3, 5, 2, 2),
    "af2": (2, 128, 128, 64, 12, 16, 4, 8, 2, 13),
    "h4": (2, 96, 96, 32, 4, 16, 4, 4, 3, 10),
    "segs64": (2, 64, 64, 16, 8, 8, 8, 8, 2, 5),
    "d128_ds24": (2, 100, 128, 64, 8, 24, 8, 8, 2, 6),
    "lds_rows": (1, 384, 32, 8, 16, 8, 4, 4, 1, 7),
    "lds_keys": (1, 136, 32, 8, 64, 8, 4, 4, 1, 8),
    "refused": (1, 256, 32, 4, 64, 8, 4, 4, 1, 9),
}
LOSS_IDS = ["odd", "odd_k5", "af2", "h4", "segs64", "d128_ds24", "lds_rows", "lds_keys"]


def geom(gid):
    B, K, D, C, H, DS, PQ, PV, NL, seed = GEOMS[gid]
    return B, K, dict(D=D, C=C, H=H, DS=DS, PQ=PQ, PV=PV, NL=NL, V=21), seed


def n_real_of(K):
    return max(2, K * 201 // 256)  # 37 -> 29, 128 -> 100, 544 -> 427; K = 5 -> 3


def cdr_of(K):
    """A CDR-H3-sized generated block (up to 24 residues) inside patch 0's real residues."""
    start = K // 8
    return slice(start, start + min(24, max(1, (n_real_of(K) - start) // 2)))


def inputs(gid, seed):
    B, K, d, _ = geom(gid)
    inp = padded(B, K, n_real_of(K), seed=seed, dims=d)
    gm = inp["generation_mask"].clone()
    gm[:, cdr_of(K)] = True
    inp["generation_mask"] = gm & inp["residue_mask"]
    return inp


def betas(B):
    return torch.tensor([0.03, 0.7, 0.25])[:B]


def diffab(d, sd):
    from diffab_pytorch import DiffAb

    torch.manual_seed(0)
    model = DiffAb(d["D"], d["C"], d["NL"], d["DS"], d["PQ"], d["PV"], d["H"]).cuda()
    model.denoiser.load_state_dict(sd)
    return model


def denoiser(d, sd):
    from diffab_pytorch.diffab_pytorch import Denoiser

    den = Denoiser(d["D"], d["C"], d["NL"], d["DS"], d["PQ"], d["PV"], d["H"], 21)
    den.load_state_dict(sd, strict=True)
    return den.cuda()


_ORACLE = {}


# ------------------------------------------------------------------ 1. forward, every geometry, every flag selection
def forward_case(gid):
    key = ("forward", gid)
    if key not in _ORACLE:
        B, K, d, seed = geom(gid)
        sd = syn.denoiser_state_dict(d, seed=seed, prefix="")
        inp = inputs(gid, seed=100 + seed)
        beta = betas(B)
        want = orc.denoiser({"denoiser." + k: v.double() for k, v in sd.items()}, inp["seq_idx"], *[f64(inp[k]) for k in ARGS[1:]],
                            beta.double(), d["NL"], d["H"])
        _ORACLE[key] = dict(sd=sd, inp=inp, beta=beta, want=want)
    return _ORACLE[key]


@pytest.mark.parametrize("gid", list(GEOMS))
def test_forward_vs_float64_oracle(hip, gid):
    """res_emb, aa_logits, eps, O0 and the posterior under each flag selection (dispatch, FORCE_GENERIC, FP32_GEMM, PAIR_PLANES) against
    the oracle, max-rel and element-wise.  Each flag only chooses among fast-path kernels, none of which these dims are eligible for,
    so the four runs must also be bitwise equal."""
    c = forward_case(gid)
    B, K, d, _ = geom(gid)
    den = denoiser(d, c["sd"]).requires_grad_(False)
    inp, want = c["inp"], c["want"]
    outs = []
    for flags, fid in zip(FLAGS, FLAG_IDS):
        with torch.no_grad():
            out = den(*[inp[k].cuda() for k in ARGS], c["beta"].cuda(), inp["generation_mask"].cuda(), inp["residue_mask"].cuda(),
                      return_logits=True, flags=flags)
        for k in OUTS:
            got, ref = out[k].cpu(), want[k].detach()
            assert torch.isfinite(got).all(), (gid, fid, k)
            assert maxrel(got, ref) < TOL and elemrel(got, ref) < TOL, (gid, fid, k, maxrel(got, ref), elemrel(got, ref))
        outs.append(out)
    worst = {k: f"{maxrel(outs[0][k].cpu(), want[k].detach()):.1e}" for k in OUTS}
    print(gid, "forward max-rel:", worst)
    for out, fid in zip(outs[1:], FLAG_IDS[1:]):
        for k in OUTS:
            assert torch.equal(out[k], outs[0][k]), (gid, fid, k)


# ------------------------------------------------------------------ 2. BWD_LOSSES (DiffAb.hotpath_train_losses)
def noised_inputs(inp, d, seed):
    """Host-drawn noised state (tests/test_gpu_backward_paths.py): generated residues get a random type, a displaced position and a random
    frame; a random posterior; eps standard normal everywhere (the losses mask it)."""
    B, K = inp["seq_idx"].shape
    gm = inp["generation_mask"]
    g = torch.Generator().manual_seed(seed)
    eps = torch.randn(B, K, 3, generator=g)
    other = syn.patches(B, K, dict(d, C=1), seed=seed + 7)["orientations"]
    return {"seq_idx_t": torch.where(gm, torch.randint(0, 20, (B, K), generator=g), inp["seq_idx"]),
            "translations_t": inp["translations"] + 2.0 * gm[..., None] * eps,
            "orientations_t": torch.where(gm[..., None, None], other, inp["orientations"]),
            "seq_posterior": torch.softmax(2.0 * torch.randn(B, K, 21, generator=g), -1),
            "translations_eps": eps}


def losses_case(gid):
    key = ("losses", gid)
    if key not in _ORACLE:
        B, K, d, seed = geom(gid)
        sd = syn.denoiser_state_dict(d, seed=seed, prefix="")
        inp = inputs(gid, seed=200 + seed)
        nz = noised_inputs(inp, d, seed=300 + seed)
        beta = betas(B)
        rco, pco = f64(inp["res_context_emb"]).requires_grad_(True), f64(inp["pair_context_emb"]).requires_grad_(True)
        sdo = leaves(sd, "denoiser.")
        den = orc.denoiser(sdo, nz["seq_idx_t"], f64(nz["translations_t"]), f64(nz["orientations_t"]), rco, pco, beta.double(), d["NL"],
                           d["H"])
        lo = orc.hotpath_losses(den, f64(nz["seq_posterior"]), f64(nz["translations_eps"]), f64(inp["orientations"]), inp["generation_mask"],
                                inp["residue_mask"])
        (lo[0] + lo[1] + lo[2]).backward()
        _ORACLE[key] = dict(sd=sd, inp=inp, nz=nz, beta=beta, losses=[float(v.detach()) for v in lo], d_rc=rco.grad, d_pc=pco.grad, sdo=sdo,
                            margin=relu_margin(sd, nz["seq_idx_t"], inp["res_context_emb"], den, beta))
    return _ORACLE[key]


def run_losses(gid):
    c = losses_case(gid)
    what = f"{gid} losses"
    assert c["margin"] > MARGIN, (what, c["margin"], "inputs on a ReLU kink: pick another weight seed")
    _, _, d, _ = geom(gid)
    model = diffab(d, c["sd"])
    inp = {k: v.cuda() for k, v in c["inp"].items()}
    nz = {k: v.cuda() for k, v in c["nz"].items()}
    rc = inp["res_context_emb"].clone().requires_grad_(True)
    pc = inp["pair_context_emb"].clone().requires_grad_(True)
    ls = model.hotpath_train_losses(nz, rc, pc, c["beta"].cuda(), inp["orientations"], inp["generation_mask"], inp["residue_mask"])
    (ls[0] + ls[1] + ls[2]).backward()
    np.testing.assert_allclose([float(v) for v in ls], c["losses"], rtol=5e-5, err_msg=what)
    r_rc, r_pc = maxrel(rc.grad, c["d_rc"]), maxrel(pc.grad, c["d_pc"])
    assert r_rc < GTOL, (what, "res_ctx", r_rc)
    assert r_pc < GTOL, (what, "pair_ctx", r_pc)
    print(what, f"d res_ctx {r_rc:.1e}, d pair_ctx {r_pc:.1e}")
    check_params(model.denoiser.named_parameters(), c["sdo"], "denoiser.", f"{what} (ReLU margin {c['margin']:.1e})")


@pytest.mark.parametrize("gid", LOSS_IDS)
def test_training_loss_gradients_vs_float64_oracle(hip, gid):
    """The three losses, d res_ctx, d pair_ctx and every denoiser parameter (the six projection weights of every layer included)."""
    run_losses(gid)


# ------------------------------------------------------------------ 3. BWD_COTANGENTS (Denoiser under autograd)
def cotangent_case(gid):
    key = ("cotangents", gid)
    if key not in _ORACLE:
        B, K, d, seed = geom(gid)
        sd = syn.denoiser_state_dict(d, seed=seed, prefix="")
        inp = inputs(gid, seed=400 + seed)
        beta = betas(B)
        g = torch.Generator().manual_seed(seed)
        cot = {"translations_eps": torch.randn(B, K, 3, generator=g), "orientations_t0": torch.randn(B, K, 3, 3, generator=g),
               "seq_posterior": torch.randn(B, K, 21, generator=g)}
        lo = {k: f64(inp[k]).requires_grad_(True) for k in ARGS[1:]}
        sdo = leaves(sd, "denoiser.")
        want = orc.denoiser(sdo, inp["seq_idx"], lo["translations"], lo["orientations"], lo["res_context_emb"], lo["pair_context_emb"],
                            beta.double(), d["NL"], d["H"])
        sum((want[k] * c.double()).sum() for k, c in cot.items()).backward()
        _ORACLE[key] = dict(sd=sd, inp=inp, beta=beta, cot=cot, outs={k: want[k].detach() for k in cot}, grads={k: v.grad for k, v in lo.items()},
                            sdo=sdo, margin=relu_margin(sd, inp["seq_idx"], inp["res_context_emb"], want, beta))
    return _ORACLE[key]


@pytest.mark.parametrize("gid", ["odd", "af2"])
def test_denoiser_cotangent_gradients_vs_float64_oracle(hip, gid):
    """Seeded random cotangents on eps, O0 and the posterior: the outputs, d x_t and d O_t (launch_ipa_frames_bwd at these dims), both
    contexts and every parameter."""
    c = cotangent_case(gid)
    what = f"{gid} cotangents"
    assert c["margin"] > MARGIN, (what, c["margin"], "inputs on a ReLU kink: pick another weight seed")
    _, _, d, _ = geom(gid)
    den = denoiser(d, c["sd"]).train()
    inp = c["inp"]
    lv = {k: inp[k].cuda().requires_grad_(True) for k in ARGS[1:]}
    out = den(inp["seq_idx"].cuda(), lv["translations"], lv["orientations"], lv["res_context_emb"], lv["pair_context_emb"], c["beta"].cuda(),
              None, None)
    for k, ref in c["outs"].items():
        assert maxrel(out[k], ref) < TOL, (what, k, maxrel(out[k], ref))
    sum((out[k] * v.cuda()).sum() for k, v in c["cot"].items()).backward()
    worst = {}
    for k in ARGS[1:]:
        assert torch.isfinite(lv[k].grad).all(), (what, k)
        worst[k] = maxrel(lv[k].grad, c["grads"][k])
        assert worst[k] < GTOL, (what, k, worst[k])
    print(what, "input gradients:", {k: f"{v:.1e}" for k, v in worst.items()})
    check_params(den.named_parameters(), c["sdo"], "denoiser.", f"{what} (ReLU margin {c['margin']:.1e})")


# ------------------------------------------------------------------ 4. BWD_LAYER (one InvariantPointAttentionLayer under autograd)
@pytest.mark.parametrize("gid,pair_bias", [("odd", True), ("af2", True), ("af2", False)], ids=["odd", "af2", "af2_no_pair_bias"])
def test_ipa_layer_gradients_vs_float64_oracle(hip, gid, pair_bias):
    """y, d x, d e (with the pair bias), d R, d t and the layer's parameters from a random d y.  Without the pair bias the layer is C = 0
    through the H = 12 row kernel (no to_pair_bias, two logits); its weights are the seeded construction, gamma drawn as the goldens'."""
    from diffab_pytorch.diffab_pytorch import InvariantPointAttentionLayer

    B, K, d, seed = geom(gid)
    if pair_bias:
        layer = denoiser(d, syn.denoiser_state_dict(d, seed=seed + 30, prefix="")).ipa.layers[d["NL"] - 1]
    else:
        torch.manual_seed(seed + 30)
        layer = InvariantPointAttentionLayer(d["D"], d["C"], d["DS"], d["PQ"], d["PV"], d["H"], use_pair_bias=False)
        with torch.no_grad():
            layer.gamma.copy_(torch.rand(d["H"]) + 0.2)
        layer = layer.cuda()
    inp = inputs(gid, seed=500 + seed)
    g = torch.Generator().manual_seed(seed)
    cy = torch.randn(B, K, d["D"], generator=g)
    names = ("res_context_emb", "pair_context_emb", "orientations", "translations")
    grads_of = [k for k in names if pair_bias or k != "pair_context_emb"]
    lv = {k: inp[k].cuda().requires_grad_(k in grads_of) for k in names}
    y = layer(*[lv[k] for k in names])
    (y * cy.cuda()).sum().backward()
    lo = {k: f64(inp[k]).requires_grad_(k in grads_of) for k in names}
    sdo = leaves({n: p for n, p in layer.named_parameters()}, "L.")
    want = orc.ipa_layer(*[lo[k] for k in names], sdo, "L.", d["H"], use_pair_bias=pair_bias)
    what = f"{gid} layer{'' if pair_bias else ' without pair bias'}"
    assert maxrel(y, want) < TOL and elemrel(y, want) < TOL, (what, maxrel(y, want), elemrel(y, want))
    (want * cy.double()).sum().backward()
    worst = {}
    for k in grads_of:
        worst[k] = maxrel(lv[k].grad, lo[k].grad)
        assert worst[k] < GTOL, (what, k, worst[k])
    print(what, "input gradients:", {k: f"{v:.1e}" for k, v in worst.items()})
    check_params(layer.named_parameters(), sdo, "L.", what)


# ------------------------------------------------------------------ 5. teacher-forced reverse step through the C ABI
@pytest.mark.parametrize("gid", ["odd", "af2"])
def test_reverse_step_teacher_forced_vs_oracle(hip, gid):
    """One reverse step at t in {100, 57, 8, 1} (diffab_sample_loop on the generic forward) against orc.reverse_update on the same noise:
    x and O within TOL, a differing sequence draw only within 1e-5 of an edge of the posterior's CDF, everything not generated bitwise
    unchanged."""
    B, K, d, seed = geom(gid)
    sd0 = syn.denoiser_state_dict(d, seed=seed + 40, prefix="")
    model = diffab(d, sd0)
    sd = {"denoiser." + k: v for k, v in sd0.items()}
    sched = orc.cosine_variance_schedule(100, s=0.01, beta_max=0.999)
    inp = inputs(gid, seed=600 + seed)
    gm = inp["generation_mask"]
    keep = ~gm
    rev = model._reverse_so3()
    rseed, first, flips = 977, 3, 0
    for t in (100, 57, 8, 1):
        got = model.sample(inp["seq_idx"], inp["translations"], inp["orientations"], res_context_emb=inp["res_context_emb"],
                           pair_context_emb=inp["pair_context_emb"], generation_mask=gm, seed=rseed, first_patch=first, t_start=t,
                           t_stop=t - 1, init=False)
        s1, x1, O1, den, us, edge = oracle_reverse_step(sd, inp, gm, rev, sched, rseed, first, t, d["NL"], d["H"])
        assert maxrel(got["translations"], x1) < TOL, (gid, t, maxrel(got["translations"], x1))
        assert maxrel(got["orientations"], O1) < TOL, (gid, t, maxrel(got["orientations"], O1))
        diff = got["seq_idx"].cpu() != s1
        if diff.any():
            assert float(edge[diff].max()) < 1e-5, (gid, t, float(edge[diff].max()))
            flips += int(diff.sum())
        for k in ("seq_idx", "translations", "orientations"):
            assert torch.equal(got[k].cpu()[keep], inp[k][keep]), (gid, t, k)
    print(f"teacher-forced reverse steps, {gid}: {flips} of {4 * int(gm.sum())} sequence draws on a CDF edge")


# ------------------------------------------------------------------ 6. past the backward's LDS: refused before anything runs
def test_backward_lds_limit_is_refused_before_launch(hip):
    """`refused` (H K = 16384): the forward runs (test_forward_vs_float64_oracle above, no grad), the backward's row kernel would need
    207 KiB of LDS.  hotpath_train_losses raises DiffabHipError naming the LDS limit from the taped forward, before anything is launched,
    leaves every .grad None, and an in-range case run right after it still matches the oracle."""
    B, K, d, seed = geom("refused")
    model = diffab(d, syn.denoiser_state_dict(d, seed=seed, prefix=""))
    inp = {k: v.cuda() for k, v in inputs("refused", seed=700).items()}
    nz = {k: v.cuda() for k, v in noised_inputs({k: v.cpu() for k, v in inp.items()}, d, seed=701).items()}
    rc = inp["res_context_emb"].clone().requires_grad_(True)
    pc = inp["pair_context_emb"].clone().requires_grad_(True)
    with pytest.raises(_hip.DiffabHipError, match=r"too large for the attention backward's LDS \(\d+ > 163840 bytes"):
        model.hotpath_train_losses(nz, rc, pc, betas(B).cuda(), inp["orientations"], inp["generation_mask"], inp["residue_mask"])
    torch.cuda.synchronize()
    assert rc.grad is None and pc.grad is None
    assert all(p.grad is None for p in model.parameters())
    run_losses("odd")


# ------------------------------------------------------------------ 7. the rotation head's gradient at small |v|
@pytest.mark.parametrize("mag", [0.0, 1e-6, 1e-4, 3e-4, 1e-3, 1e-2, 0.1], ids=lambda m: f"v{m:g}")
def test_rotation_head_gradient_at_small_rotvec(hip, mag):
    """O0 = O_t exp(hat(v)) differentiated where sin n / n, (1 - cos n) / n^2 and their derivatives are 0/0 or cancel (rotvec_head_bwd,
    csrc/noslp_kernels.hip).  `odd_k5`, the smallest geometry; the rotation head's last layer has zero weight and the bias v, so every
    row's rotvec is exactly v, |v| = mag; seeded cotangents on O0 alone.  Then d bias = sum over the rows of so3_ref.exp_head_vjp (float64,
    the series limits at small |v|) and d O_t = G0 exp(hat(v))^T: both finite at |v| = 0 and within GTOL at every |v|, 0 included."""
    import so3_ref as ref

    gid = "odd_k5"
    B, K, d, seed = geom(gid)
    sd = syn.denoiser_state_dict(d, seed=seed, prefix="")
    v = (mag * np.array([0.6, -0.48, 0.64])).astype(np.float32)
    sd["orientation_denoising.4.weight"] = torch.zeros_like(sd["orientation_denoising.4.weight"])
    sd["orientation_denoising.4.bias"] = torch.from_numpy(v.copy())
    den = denoiser(d, sd).train()
    inp = inputs(gid, seed=800 + seed)
    G0 = torch.randn(B, K, 3, 3, generator=torch.Generator().manual_seed(seed))
    lv = {k: inp[k].cuda().requires_grad_(True) for k in ARGS[1:]}
    out = den(inp["seq_idx"].cuda(), lv["translations"], lv["orientations"], lv["res_context_emb"], lv["pair_context_emb"], betas(B).cuda(),
              None, None)
    (out["orientations_t0"] * G0.cuda()).sum().backward()
    O_t = inp["orientations"].double().numpy().reshape(-1, 3, 3)
    G = G0.double().numpy().reshape(-1, 3, 3)
    vs = np.broadcast_to(v.astype(np.float64), (B * K, 3))
    want_v = ref.exp_head_vjp(vs, O_t, G).sum(0)
    want_O = G @ ref.T(ref.exp(vs))
    got_v, got_O = den.orientation_denoising[4].bias.grad.cpu(), lv["orientations"].grad.cpu().reshape(-1, 3, 3)
    r_O0 = maxrel(out["orientations_t0"].detach().reshape(-1, 3, 3), O_t @ ref.exp(vs))
    r_v, r_O = maxrel(got_v, want_v), maxrel(got_O, want_O)
    print(f"rotation head at |v| = {mag:g}: O0 {r_O0:.1e}, d bias {r_v:.1e}, d O_t {r_O:.1e}")
    assert torch.isfinite(got_v).all() and torch.isfinite(got_O).all() and torch.isfinite(out["orientations_t0"]).all(), mag
    assert r_O0 < TOL and r_v < GTOL and r_O < GTOL, (mag, r_O0, r_v, r_O)
