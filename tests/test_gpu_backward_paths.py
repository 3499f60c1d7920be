"""The training backward (csrc/denoiser_backward.hip, run_backward) at the K, depth and frozen-context branches no other test compares.

run_backward picks its kernels (plan_backward once per call, choose_attn_bwd once per layer) from K, the layer count NL, which gradients
were asked for and the buffers of its workspace (BwdWorkspace) it reuses across layers.  At the
benchmark dims (D = 128, C = 64, H = 8, DS = 32, PQ = PV = 8) every case below is compared with the float64 oracle
(oracle/diffab_oracle.py under torch autograd on the host): the losses (rtol 5e-5), the forward outputs where the mode returns them (TOL),
every input gradient and every denoiser parameter (GTOL, max-rel).

  case          K    B  NL  mode                              reaches
  k64_losses    64   3   2  hotpath_train_losses (LOSSES)     ipa_attn_bwd_keys_mfma_kernel<0,false> / <1,false> / <2,true> (d q: scales
                                                              hard-coded in the kernel), ipa_pair_stream_bwd_kernel<4,4>,
                                                              ipa_pair_de_layers_kernel<4,2> (nl = 2), the split attention's taped
                                                              forward at K = 64
  k64_cot       64   2   2  Denoiser under autograd, random   the above, plus launch_ipa_frames_bwd at K = 64 (d x_t, d O_t)
                            cotangents (COTANGENTS)
  k64_layer     64   2   -  one IPA layer (LAYER)             defer_de off: d pair_ctx read-modified-written by the pair-stream kernel
  k64_nl6       64   2   6  losses                            ipa_pair_de_layers_kernel<4,2> with a full layer table (kDeLayersMax)
  k64_nl7       64   2   7  losses                            NL > kDeLayersMax at K = 64: d pair_ctx per layer, g in the single dAkv slot
  k128_nl3     128   2   3  losses                            the first depth at which dprojs[l & 1] / dxa / dxb are reused while the
                                                              side stream's weight gradients may still read them; every projection
                                                              weight of every layer
  k128_nl7     128   2   7  losses and cotangents             NL > 6 at K = 128 (keys_tn_b6 / keys_nn_b6, d pair_ctx per layer)
  frozen_pair  64,  2   2,  losses, pair_ctx without grad    d_pair_ctx == nullptr: defer_de off, the pair-stream kernel gets de = null,
               128      7                                     d to_pair_bias.weight and d gamma still come out of wb_part; pair_ctx.grad
                                                              stays None
  deepest       64   1  16  losses                            kMaxLayers, the deepest tape the library carves

and NL = 17 (one past kMaxLayers) must be refused with DiffabHipError before anything runs.

Every case pads patch 0 as collate does (`padded`) and marks a CDR-sized generated block.  The noised inputs of the loss cases are drawn on
the host (any seq_idx_t / x_t / O_t / posterior / eps is a valid input of the losses), so the oracle side is deterministic and is computed
once per case (`_ORACLE`).  Weight seeds keep every ReLU pre-activation at least 5e-7 away from 0 (`relu_margin`).
"""
import numpy as np
import pytest
import torch

import diffab_oracle as orc
from conftest import maxrel
from diffab_pytorch import _hip, synthetic as syn
from sampler_support import GTOL, TOL, check_params, f64, hip, leaves, n_real_of, padded, relu_margin

pytestmark = pytest.mark.gpu
ARGS = ("seq_idx", "translations", "orientations", "res_context_emb", "pair_context_emb")
CDR = slice(10, 34)  # a CDR-H3-sized generated block (24 residues), inside patch 0's real residues at K = 64 (50 real)
MARGIN = 5e-7


def dims_of(NL):
    return dict(syn.BENCH_DIMS, NL=NL)


def gradient_inputs(B, K, seed):
    """`padded` patches (patch 0 padded after ~4/5 of its residues) with the CDR block generated in every patch, within residue_mask."""
    inp = padded(B, K, n_real_of(K), seed=seed, dims=dims_of(2))
    gm = inp["generation_mask"].clone()
    gm[:, CDR] = True
    inp["generation_mask"] = gm & inp["residue_mask"]
    return inp


def betas(B):
    return torch.tensor([0.03, 0.7, 0.25])[:B]


def noised_inputs(inp, seed):
    """Host-drawn noised state: generated residues get a random type, a displaced position and a random frame; the posterior is a
    random distribution over the 21 types; eps is standard normal everywhere (the losses mask it)."""
    B, K = inp["seq_idx"].shape
    gm = inp["generation_mask"]
    g = torch.Generator().manual_seed(seed)
    eps = torch.randn(B, K, 3, generator=g)
    other = syn.patches(B, K, dims_of(2), seed=seed + 7)["orientations"]
    return {"seq_idx_t": torch.where(gm, torch.randint(0, 20, (B, K), generator=g), inp["seq_idx"]),
            "translations_t": inp["translations"] + 2.0 * gm[..., None] * eps,
            "orientations_t": torch.where(gm[..., None, None], other, inp["orientations"]),
            "seq_posterior": torch.softmax(2.0 * torch.randn(B, K, 21, generator=g), -1),
            "translations_eps": eps}


_ORACLE = {}


def losses_case(K, B, NL, seed):
    """The float64 oracle of one loss case: losses, d res_ctx, d pair_ctx, every parameter gradient (as leaves), the ReLU margin."""
    key = ("losses", K, B, NL, seed)
    if key not in _ORACLE:
        sd = syn.denoiser_state_dict(dims_of(NL), seed=seed, prefix="")
        inp = gradient_inputs(B, K, seed=200 + seed)
        nz = noised_inputs(inp, seed=300 + seed)
        beta = betas(B)
        rco, pco = f64(inp["res_context_emb"]).requires_grad_(True), f64(inp["pair_context_emb"]).requires_grad_(True)
        sdo = leaves(sd, "denoiser.")
        den = orc.denoiser(sdo, nz["seq_idx_t"], f64(nz["translations_t"]), f64(nz["orientations_t"]), rco, pco, beta.double(), NL,
                           syn.BENCH_DIMS["H"])
        lo = orc.hotpath_losses(den, f64(nz["seq_posterior"]), f64(nz["translations_eps"]), f64(inp["orientations"]), inp["generation_mask"],
                                inp["residue_mask"])
        (lo[0] + lo[1] + lo[2]).backward()
        _ORACLE[key] = dict(sd=sd, inp=inp, nz=nz, beta=beta, losses=[float(v.detach()) for v in lo], d_rc=rco.grad, d_pc=pco.grad, sdo=sdo,
                            margin=relu_margin(sd, nz["seq_idx_t"], inp["res_context_emb"], den, beta))
    return _ORACLE[key]


def run_losses(K, B, NL, seed, what, frozen_pair=False):
    """DiffAb.hotpath_train_losses + backward on the device against losses_case; pair_ctx without grad when frozen_pair."""
    from diffab_pytorch import DiffAb

    c = losses_case(K, B, NL, seed)
    assert c["margin"] > MARGIN, (what, c["margin"], "inputs on a ReLU kink: pick another weight seed")
    d = dims_of(NL)
    torch.manual_seed(0)
    model = DiffAb(d["D"], d["C"], d["NL"], d["DS"], d["PQ"], d["PV"], d["H"]).cuda()
    model.denoiser.load_state_dict(c["sd"])
    inp = {k: v.cuda() for k, v in c["inp"].items()}
    nz = {k: v.cuda() for k, v in c["nz"].items()}
    rc = inp["res_context_emb"].clone().requires_grad_(True)
    pc = inp["pair_context_emb"].clone().requires_grad_(not frozen_pair)
    ls = model.hotpath_train_losses(nz, rc, pc, c["beta"].cuda(), inp["orientations"], inp["generation_mask"], inp["residue_mask"])
    (ls[0] + ls[1] + ls[2]).backward()
    np.testing.assert_allclose([float(v) for v in ls], c["losses"], rtol=5e-5, err_msg=what)
    r_rc = maxrel(rc.grad, c["d_rc"])
    assert r_rc < GTOL, (what, "res_ctx", r_rc)
    if frozen_pair:
        assert pc.grad is None, what
        r_pc = None
    else:
        r_pc = maxrel(pc.grad, c["d_pc"])
        assert r_pc < GTOL, (what, "pair_ctx", r_pc)
    print(what, f"d res_ctx {r_rc:.1e}, d pair_ctx", "frozen" if r_pc is None else f"{r_pc:.1e}")
    check_params(model.denoiser.named_parameters(), c["sdo"], "denoiser.", f"{what} (ReLU margin {c['margin']:.1e})")
    return model, c


# ------------------------------------------------------------------ 1. BWD_LOSSES at K = 64, at depth, at the deepest tape
LOSS_CASES = [  # id, K, B, NL, weight seed
    ("k64_losses", 64, 3, 2, 11),
    ("k64_nl6", 64, 2, 6, 12),
    ("k64_nl7", 64, 2, 7, 13),
    ("k128_nl3", 128, 2, 3, 14),
    ("k128_nl7", 128, 2, 7, 15),
    ("deepest", 64, 1, 16, 16),
]


@pytest.mark.parametrize("K,B,NL,seed", [c[1:] for c in LOSS_CASES], ids=[c[0] for c in LOSS_CASES])
def test_training_loss_gradients_vs_float64_oracle(hip, K, B, NL, seed):
    """The three losses, d res_ctx, d pair_ctx and every parameter of every layer (the six projection weights of layers 0 .. NL-1
    included) against the oracle."""
    run_losses(K, B, NL, seed, f"K={K} B={B} NL={NL} losses")


# ------------------------------------------------------------------ 2. frozen pair context: d_pair_ctx == nullptr
@pytest.mark.parametrize("K,B,NL,seed", [(64, 2, 2, 17), (128, 2, 7, 15)], ids=["k64_nl2", "k128_nl7"])
def test_frozen_pair_context_gradients_vs_float64_oracle(hip, K, B, NL, seed):
    """pair_context_emb without grad (frozen encoder, contexts under no_grad): no d pair_ctx is asked for, pair_ctx.grad stays None, and
    d to_pair_bias.weight / d gamma of every layer (reduced from the per-row partials) still equal the oracle's, as does everything else.
    The K = 128 case shares k128_nl7's oracle."""
    model, c = run_losses(K, B, NL, seed, f"K={K} B={B} NL={NL} frozen pair_ctx", frozen_pair=True)
    params = dict(model.denoiser.named_parameters())
    for l in range(NL):
        for n in ("to_pair_bias.weight", "gamma"):
            name = f"ipa.layers.{l}.{n}"
            assert float(params[name].grad.abs().max()) > 0, name
            assert maxrel(params[name].grad, c["sdo"]["denoiser." + name].grad) < GTOL, name


# ------------------------------------------------------------------ 3. BWD_COTANGENTS at K = 64 and at NL = 7
def cotangent_case(K, B, NL, seed):
    key = ("cotangents", K, B, NL, seed)
    if key not in _ORACLE:
        sd = syn.denoiser_state_dict(dims_of(NL), seed=seed, prefix="")
        inp = gradient_inputs(B, K, seed=400 + seed)
        beta = betas(B)
        g = torch.Generator().manual_seed(seed)
        cot = {"translations_eps": torch.randn(B, K, 3, generator=g), "orientations_t0": torch.randn(B, K, 3, 3, generator=g),
               "seq_posterior": torch.randn(B, K, 21, generator=g)}
        lo = {k: f64(inp[k]).requires_grad_(True) for k in ARGS[1:]}
        sdo = leaves(sd, "denoiser.")
        want = orc.denoiser(sdo, inp["seq_idx"], lo["translations"], lo["orientations"], lo["res_context_emb"], lo["pair_context_emb"],
                            beta.double(), NL, syn.BENCH_DIMS["H"])
        sum((want[k] * c.double()).sum() for k, c in cot.items()).backward()
        _ORACLE[key] = dict(sd=sd, inp=inp, beta=beta, cot=cot, outs={k: want[k].detach() for k in cot}, grads={k: v.grad for k, v in lo.items()},
                            sdo=sdo, margin=relu_margin(sd, inp["seq_idx"], inp["res_context_emb"], want, beta))
    return _ORACLE[key]


@pytest.mark.parametrize("K,B,NL,seed", [(64, 2, 2, 21), (128, 2, 7, 22)], ids=["k64_cot", "k128_nl7_cot"])
def test_denoiser_cotangent_gradients_vs_float64_oracle(hip, K, B, NL, seed):
    """Denoiser under autograd with seeded random cotangents on eps, O0 and the posterior: the outputs, d x_t, d O_t (the frame
    gradients of every layer), both contexts and every parameter."""
    from diffab_pytorch.diffab_pytorch import Denoiser

    c = cotangent_case(K, B, NL, seed)
    what = f"K={K} B={B} NL={NL} cotangents"
    assert c["margin"] > MARGIN, (what, c["margin"], "inputs on a ReLU kink: pick another weight seed")
    d = dims_of(NL)
    den = Denoiser(d["D"], d["C"], d["NL"], d["DS"], d["PQ"], d["PV"], d["H"], 21)
    den.load_state_dict(c["sd"], strict=True)
    den = den.cuda().train()
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


# ------------------------------------------------------------------ 4. BWD_LAYER at K = 64
def test_ipa_layer_gradients_at_k64_vs_float64_oracle(hip):
    """One InvariantPointAttentionLayer under autograd at K = 64 (defer_de is off in this mode): y, d x, d e, d R, d t and the layer's
    parameters from a random d y."""
    from diffab_pytorch.diffab_pytorch import Denoiser

    K, B = 64, 2
    d = dims_of(2)
    den = Denoiser(d["D"], d["C"], d["NL"], d["DS"], d["PQ"], d["PV"], d["H"], 21)
    den.load_state_dict(syn.denoiser_state_dict(d, seed=31, prefix=""), strict=True)
    layer = den.cuda().ipa.layers[1]
    inp = gradient_inputs(B, K, seed=531)
    g = torch.Generator().manual_seed(K + 1)
    cy = torch.randn(B, K, d["D"], generator=g)
    names = ("res_context_emb", "pair_context_emb", "orientations", "translations")
    lv = {k: inp[k].cuda().requires_grad_(True) for k in names}
    y = layer(*[lv[k] for k in names])
    (y * cy.cuda()).sum().backward()
    lo = {k: f64(inp[k]).requires_grad_(True) for k in names}
    sdo = leaves({n: p for n, p in layer.named_parameters()}, "L.")
    want = orc.ipa_layer(*[lo[k] for k in names], sdo, "L.", d["H"])
    assert maxrel(y, want) < TOL, maxrel(y, want)
    (want * cy.double()).sum().backward()
    worst = {}
    for k in names:
        worst[k] = maxrel(lv[k].grad, lo[k].grad)
        assert worst[k] < GTOL, (k, worst[k])
    print(f"K={K} layer input gradients:", {k: f"{v:.1e}" for k, v in worst.items()})
    check_params(layer.named_parameters(), sdo, "L.", f"K={K} layer")


# ------------------------------------------------------------------ 5. one past the deepest tape
def test_layer_limit_is_an_error(hip):
    """NL = 17 > kMaxLayers under hotpath_train_losses: DiffabHipError naming the limit, raised by the taped forward before anything
    is launched, and no gradient anywhere."""
    from diffab_pytorch import DiffAb

    d = dims_of(17)
    torch.manual_seed(0)
    model = DiffAb(d["D"], d["C"], d["NL"], d["DS"], d["PQ"], d["PV"], d["H"]).cuda()
    inp = {k: v.cuda() for k, v in gradient_inputs(1, 64, seed=617).items()}
    nz = {k: v.cuda() for k, v in noised_inputs({k: v.cpu() for k, v in inp.items()}, seed=617).items()}
    rc = inp["res_context_emb"].clone().requires_grad_(True)
    pc = inp["pair_context_emb"].clone().requires_grad_(True)
    with pytest.raises(_hip.DiffabHipError, match="at most 16 IPA layers"):
        model.hotpath_train_losses(nz, rc, pc, betas(1).cuda(), inp["orientations"], inp["generation_mask"], inp["residue_mask"])
    torch.cuda.synchronize()
    assert rc.grad is None and pc.grad is None
    assert all(p.grad is None for p in model.parameters())
