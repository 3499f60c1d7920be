"""The benchmark-geometry (MFMA) kernels at patch lengths above 256, against a float64 restatement.

fast_path_supported (csrc/denoiser_fast.hip) takes D = 128, C = 64, H = 8, DS = 32, P = 8 at every K % 64 == 0 from 64 to 1024;
tests/test_gpu_patch_lengths.py stops at K = 256.  This file continues its kernel-per-K table (profiles/long_patches.md has the trace):

  K     forward ipa_attn_fast_kernel<NT, MULTI, *>    attention backward (plan.fast), row pass -> key pass
  192   <4, true>, 3 chunks of  64 keys               ipa_attn_bwd_rows_mr_kernel<4, 0> -> ipa_attn_bwd_keys_mfma_kernel<0/1>
  256   <8, true>, 2 chunks of 128 keys               ipa_attn_bwd_rows_mr_kernel<4, 0> -> ipa_attn_bwd_keys_mr_kernel<4> (64 KiB of LDS)
  320   <4, true>, 5 chunks of  64 keys               ipa_attn_bwd_rows_mr_kernel<4, 0> -> ipa_attn_bwd_keys_kernel (4 * 256 K > 64 KiB)
  384   <8, true>, 3 chunks of 128 keys               ipa_attn_bwd_rows_kernel (16 (24 K + 1672) > 160 KiB from K = 358) -> ipa_attn_bwd_keys_kernel
  512   <8, true>, 4 chunks of 128 keys               (forward only here)
  640   <8, true>, 5 chunks of 128 keys               ipa_attn_bwd_rows_kernel with 4 (24 K + 1672) = 68 128 bytes > 64 KiB of dynamic LDS
                                                      -> ipa_attn_bwd_keys_kernel
  1024  <8, true>, 8 chunks of 128 keys               (forward and sampler only here; the documented limit)

K = 384 is the first length at which the 128-key form rescales sums that were already rescaled and parked, K = 320 the first with more
than three 64-key chunks.  Above K = 256 the sampler leaves the patch-resident module launch (ipa_module_persistent_supported) for
per-layer launches with the last-layer tile map (K / 16 tiles per patch) and pair planes.

Inputs: `padded` patches (patch 0 padded after ~4/5 of its residues, the last patch whole) at B = 2, B = 1 from K = 640 up.  Oracle:
oracle/diffab_oracle.py in float64 on the host.

Bars.  TOL = 1e-4 (forward) and GTOL = 2e-4 (gradients) hold for `maxrel` at every K.  Element-wise (`elemrel`) and for gradients a
kernel is held to max(bar, 2 x the error of the SAME oracle evaluated in fp32 on the host against float64, on the same tensor): fp32
sums over this many keys are themselves above 1e-4 element-wise (tests/test_gpu_generic_dims.py records it for long K), and the
factor 2 covers a different but equally valid fp32 summation order.  Every test prints both numbers per tensor.

fp32 oracle against float64 on the host, worst of the five forward outputs (8 threads / 16 threads: the order of the host's fp32
sums, and with it the bar, depends on the thread count):
  K = 320   maxrel 2.1e-6 / 1.3e-6, elemrel 9.5e-5 (translations_eps) / 6.9e-5
  K = 384   maxrel 1.6e-6 / 1.6e-6, elemrel 8.6e-5 (res_emb) / 1.07e-4 (orientations_t0)
  K = 1024  maxrel 1.8e-6 / 1.1e-6, elemrel 1.16e-4 (res_emb) / 6.0e-5
  one layer at K = 512: maxrel 6e-7, elemrel 3.3e-5; the shaped softmax cases: maxrel 3e-7 .. 1.2e-6, elemrel 1.4e-5 .. 6.8e-5 per row group
  gradients (fp32 autograd, the three roots at K = 320 / 384, the layer at 640): inputs 5e-7 .. 3.5e-6, parameters <= 4.4e-6: far below
  GTOL, so every gradient bar is GTOL itself
The kernels on an MI355X:
  forward, MFMA (dispatch / fp32gemm / pairplanes), worst output: K = 320 maxrel 1.2e-6, elemrel 9.0e-5; K = 384 1.5e-6, 6.6e-5;
    K = 1024 2.3e-6, 8.2e-5.  Generic: K = 320 1.2e-6, 5.6e-5; K = 384 1.3e-6, 6.8e-5; K = 1024 2.0e-6, 6.5e-5
  one layer at K = 512: maxrel 5.6e-7, elemrel 2.9e-5; shaped softmax cases, worst row group: maxrel 8.1e-7, elemrel 3.7e-5
  gradients: inputs <= 3.0e-6, parameters <= 3.5e-6; the teacher-forced reverse step: x 5e-8, O 1.6e-6, no sequence draw on a CDF edge

What this file found.  The generic forward (FLAG_FORCE_GENERIC) at K = 1024 had res_emb at elemrel 3.4e-4 (maxrel 5.2e-6) against a bar
of 1.2e-4: ipa_attn_generic_kernel summed the weighted values of a query row over the keys in one fp32 accumulator.  A host
restatement of its operation order gives the same 5.2e-6, and 7.6e-7 with only those sums in float64, so the kernel now runs them in
fp64 (the dense products, logits and softmax were not the cause).  The MFMA kernels passed every case as they were.
"""
import math

import pytest
import torch

import diffab_oracle as orc
from conftest import elemrel, maxrel
from diffab_pytorch import _hip, synthetic as syn
from sampler_support import (ARGS, FLAGS, FLAG_IDS, GTOL, OUTS, PATCH_LENGTH_DIMS, TOL, check_params, f64, hip, make_model,
                             n_real_of, oracle_reverse_step, padded, relu_margin)

pytestmark = pytest.mark.gpu
DIMS = PATCH_LENGTH_DIMS
LAYER_IN = ("res_context_emb", "pair_context_emb", "orientations", "translations")


def batch_of(K):
    return 2 if K < 640 else 1


def denoiser(seed, dims=DIMS):
    from diffab_pytorch.diffab_pytorch import Denoiser

    den = Denoiser(dims["D"], dims["C"], dims["NL"], dims["DS"], dims["PQ"], dims["PV"], dims["H"], 21)
    sd = syn.denoiser_state_dict(dims, seed=seed, prefix="")
    den.load_state_dict(sd, strict=True)
    return den.cuda(), sd


def diffab(seed):
    return make_model(DIMS, seed), syn.denoiser_state_dict(DIMS, seed=seed, prefix="")


def as_type(v, dtype):
    v = v.detach().cpu()
    return v.to(dtype) if v.is_floating_point() else v


def leaves_as(sd, prefix, dtype):
    """`leaves` at a chosen precision: the oracle's parameters as autograd leaves."""
    return {prefix + k: as_type(v, dtype).requires_grad_(True) for k, v in sd.items()}


def hold(what, got, own, ref, base, metric=maxrel):
    """got (the kernel) within max(base, 2 x the fp32 oracle's own error) of ref (float64), by `metric`; prints both."""
    err, err32 = metric(got, ref), metric(own, ref)
    bar = max(base, 2.0 * err32)
    print(f"{what}: {metric.__name__} kernel {err:.2e}, fp32 oracle {err32:.2e}, bar {bar:.2e}")
    assert err < bar, (what, metric.__name__, err, err32, bar)
    return err


def hold_forward(what, got, own, ref):
    """A forward tensor: finite, maxrel at TOL flat, elemrel at max(TOL, 2 x fp32 oracle)."""
    got = got.detach().cpu()
    assert torch.isfinite(got).all(), what
    mr, mr32 = maxrel(got, ref), maxrel(own, ref)
    print(f"{what}: maxrel kernel {mr:.2e}, fp32 oracle {mr32:.2e}")
    assert mr < TOL, (what, mr)
    hold(what, got, own, ref, TOL, elemrel)


def worst_param(sdo, own, prefix=""):
    """(name, maxrel) of the fp32 oracle's worst parameter gradient against float64."""
    return max(((n, maxrel(own[n].grad, sdo[n].grad)) for n in sdo if sdo[n].grad is not None), key=lambda v: v[1])


# ------------------------------------------------------------------ 1. forward parity
_FWD = {}


def forward_case(K):
    if K not in _FWD:
        den, sd = denoiser(seed=K)
        den.requires_grad_(False)
        inp = padded(batch_of(K), K, n_real_of(K), seed=100 + K)
        beta = torch.tensor([0.03, 0.7])[: batch_of(K)]
        want = {}
        with torch.no_grad():
            for dtype in (torch.float64, torch.float32):
                want[dtype] = orc.denoiser({"denoiser." + k: v.to(dtype) for k, v in sd.items()}, inp["seq_idx"],
                                           *[inp[k].to(dtype) for k in ARGS[1:]], beta.to(dtype), DIMS["NL"], DIMS["H"])
        _FWD[K] = (den, inp, beta, want[torch.float64], want[torch.float32])
    return _FWD[K]


@pytest.mark.parametrize("flags", FLAGS, ids=FLAG_IDS)
@pytest.mark.parametrize("K", [320, 384, 1024])
def test_forward_vs_float64_oracle(hip, K, flags):
    """res_emb, aa_logits, eps, O0 and the posterior at nc = 5 (64-key chunks), nc = 3 and nc = 8 (128-key chunks), every flag."""
    den, inp, beta, want, own = forward_case(K)
    out = den(*[inp[k].cuda() for k in ARGS], beta.cuda(), inp["generation_mask"].cuda(), inp["residue_mask"].cuda(), return_logits=True,
              flags=flags)
    for k in OUTS:
        hold_forward(f"K={K} flags={flags} {k}", out[k], own[k], want[k])


_LAYER = {}


def layer_case(K, seed, shaped=False):
    """(layer on the device, host inputs by LAYER_IN name, float64 oracle (y, attn), fp32 oracle y) of one IPA layer at B = 1."""
    key = (K, seed, shaped)
    if key not in _LAYER:
        den, _ = denoiser(seed=seed)
        layer = den.ipa.layers[0].requires_grad_(False)
        inp = padded(1, K, n_real_of(K), seed=600 + K)
        sdo = {"L." + n: f64(p) for n, p in layer.named_parameters()}
        groups = None
        if shaped:
            inp["pair_context_emb"], groups = shape_pair_bias(inp, sdo, K)
        with torch.no_grad():
            y, attn, _ = orc.ipa_layer(*[f64(inp[k]) for k in LAYER_IN], sdo, "L.", DIMS["H"], return_attn=True)
            own = orc.ipa_layer(*[inp[k] for k in LAYER_IN], {n: p.float() for n, p in sdo.items()}, "L.", DIMS["H"])
        _LAYER[key] = (layer, inp, y, attn[0], own, groups)
    return _LAYER[key]


PAIR_FORMS = [0, _hip.FLAG_PAIR_PLANES]
PAIR_IDS = ["pair_f32", "pairplanes"]


@pytest.mark.parametrize("flags", PAIR_FORMS, ids=PAIR_IDS)
def test_ipa_layer_forward_at_k512(hip, flags):
    """diffab_ipa_layer_fwd at K = 512 (four 128-key chunks), from the fp32 pair stream and from pair planes."""
    layer, inp, want, _, own, _ = layer_case(512, seed=512 + 3)
    with torch.no_grad():
        y = layer(*[inp[k].cuda() for k in LAYER_IN], flags=flags)
    hold_forward(f"layer K=512 flags={flags}", y, own, want)


# ------------------------------------------------------------------ 2. the online softmax with chosen maxima
# Logits below are the oracle's: 3^-1/2 (q.k / sqrt(DS) + pair bias + point term), the argument of its softmax.  The pair bias of head h at
# (i, j) is pair[i, j] . to_pair_bias[h]; adding pinv(to_pair_bias) @ v to pair[i, j] adds exactly v[h] to the bias of every head h.
BLOCK = 64         # the cases are laid out on 64-key blocks: a 128-key chunk is two of them, so they hold for both chunk sizes
DOMINANT = 120.0   # (a) the dominant key's logit above the row's largest random logit; fp32 exp underflows to 0 below -103.98
LIFT, STEP = 4.0, 3.0  # (b), (c) one key per block at LIFT + STEP * rank above the row's largest random logit
HEAD_SETS = ((0, 2, 5, 7), (1, 3, 4, 6))  # the heads shaped in a row (alternating); the row's other heads stay random


def row_roles(K):
    """role of query row i: 0 .. nb - 1 = (a) dominant key in 64-key block `role`; nb = (b) climbing; nb + 1 = (c) falling; nb + 2 = (d)
    control.  Consecutive rows take consecutive roles, so every 16-row tile of the kernel mixes all of them."""
    nb = K // BLOCK
    return torch.arange(K) % (nb + 3), nb


def row_heads(K):
    """(K, H) bool: the heads shaped in each row."""
    _, nb = row_roles(K)
    which = (torch.arange(K) // (nb + 3)) % 2
    sets = torch.zeros(2, DIMS["H"], dtype=torch.bool)
    for s, hs in enumerate(HEAD_SETS):
        sets[s, list(hs)] = True
    return sets[which]


def shape_pair_bias(inp, sdo, K):
    """The pair tensor with the cases (a) - (c) written into it along to_pair_bias's rows, and the row groups {name: LongTensor}."""
    H = DIMS["H"]
    with torch.no_grad():
        _, attn, _ = orc.ipa_layer(*[f64(inp[k]) for k in LAYER_IN], sdo, "L.", H, return_attn=True)
    logit = attn[0].log()  # (H, K, K) up to a constant per row; -inf where float64 underflows (never a block's maximum here)
    role, nb = row_roles(K)
    heads = row_heads(K).T  # (H, K)
    top = logit.max(-1).values  # (H, K)
    bmax, barg = logit.view(H, K, nb, BLOCK).max(-1)  # (H, K, nb): every block's largest random logit and its key
    assert torch.isfinite(bmax).all()
    key = barg + BLOCK * torch.arange(nb)
    delta = torch.zeros(H, K, K, dtype=torch.float64)
    rank = torch.arange(nb, dtype=torch.float64)
    for c in range(nb):
        level = {"dominant": torch.full((K,), DOMINANT, dtype=torch.float64), "climb": LIFT + STEP * rank[c].expand(K),
                 "fall": LIFT + STEP * (nb - 1 - rank[c]).expand(K)}
        for name, rows in (("dominant", role == c), ("climb", role == nb), ("fall", role == nb + 1)):
            sel = heads & rows[None, :]  # (H, K)
            h, i = sel.nonzero(as_tuple=True)
            j = key[h, i, c]
            delta[h, i, j] = top[h, i] + level[name][i] - logit[h, i, j]
    pinv = torch.linalg.pinv(sdo["L.to_pair_bias.weight"])  # (C, H)
    e = f64(inp["pair_context_emb"])
    e[0] += torch.einsum("ch,hij->ijc", pinv, math.sqrt(3.0) * delta)
    groups = {f"dominant_block_{c}": (role == c).nonzero().flatten() for c in range(nb)}
    groups.update(climb=(role == nb).nonzero().flatten(), fall=(role == nb + 1).nonzero().flatten(),
                  control=(role == nb + 2).nonzero().flatten())
    return e.float(), groups


def chunk_keys(K):
    return 128 if K % 128 == 0 else 64  # 16 nt keys per chunk of ipa_attn_fast_kernel, nt = 8 when K % 128 == 0


def check_shaped_preconditions(K, attn, groups):
    """The cases as the float64 oracle's attention on the shaped inputs has them - asserted before any kernel is judged."""
    H = DIMS["H"]
    logit = attn.log()  # (H, K, K)
    heads = row_heads(K).T
    _, nb = row_roles(K)
    ck = chunk_keys(K)
    for c in range(nb):
        rows = groups[f"dominant_block_{c}"]
        assert len(rows) >= 16
        for h in range(H):
            r = rows[heads[h, rows]]
            two = logit[h, r].topk(2, dim=-1)
            assert bool((two.indices[:, 0] // BLOCK == c).all()), (K, c, h)
            gap = two.values[:, 0] - two.values[:, 1]
            assert float(gap.min()) > 104.0 and bool((torch.exp(-gap.float()) == 0).all()), (K, c, h, float(gap.min()))
    for name, sign in (("climb", 1.0), ("fall", -1.0)):
        rows = groups[name]
        assert len(rows) >= 16
        for h in range(H):
            r = rows[heads[h, rows]]
            for width in {BLOCK, ck}:
                m = logit[h, r].view(len(r), K // width, width).max(-1).values
                step = sign * (m[:, 1:] - m[:, :-1])
                lo, hi = STEP * width / BLOCK - 1.0, STEP * width / BLOCK + 1.0
                assert float(step.min()) > lo and float(step.max()) < hi, (K, name, h, width, float(step.min()), float(step.max()))
    assert len(groups["control"]) >= 16
    # the shaped rows' other heads and the control rows keep spread-out random maxima: nothing there is one-hot by construction
    return True


@pytest.mark.parametrize("flags", PAIR_FORMS, ids=PAIR_IDS)
@pytest.mark.parametrize("K", [192, 256, 320, 384])
def test_online_softmax_with_chosen_maxima(hip, K, flags):
    """One IPA layer whose pair bias places, per query row and for half of the heads: (a) a dominant key in a chosen 64-key block, far
    enough above everything else that exp(M_old - M_new) is 0 in fp32 - once per block, so every chunk is once the one that wipes the
    parked sums and once one that is wiped; (b) one key per block whose logit climbs by 3 per block, so every chunk rescales what is
    parked (by e^-3 at 64-key chunks, e^-6 at 128-key chunks); (c) the same falling, so every later chunk enters with cf < 1; (d) control
    rows.  Each group of rows is compared on its own, normalised by its own maximum (the dominant rows' outputs are larger)."""
    layer, inp, want, attn, own, groups = layer_case(K, seed=K + 9, shaped=True)
    assert check_shaped_preconditions(K, attn, groups)
    with torch.no_grad():
        y = layer(*[inp[k].cuda() for k in LAYER_IN], flags=flags)
    assert torch.isfinite(y).all()
    for name, rows in groups.items():
        hold_forward(f"K={K} flags={flags} rows {name}", y[0, rows.cuda()], own[0, rows], want[0, rows])


# ------------------------------------------------------------------ 3. gradient parity: the three roots of the backward
def gradient_inputs(K):
    B = batch_of(K)
    inp = padded(B, K, n_real_of(K), seed=200 + K)
    gm = torch.zeros(B, K, dtype=torch.bool)
    gm[:, 10:70] = True  # a CDR-sized generated block in every patch, plus the generator's own segment where it is real
    gm |= inp["generation_mask"]
    inp["generation_mask"] = gm & inp["residue_mask"]
    return inp


# weight seeds: every ReLU pre-activation of the oracle >= 5e-7 from 0 (`relu_margin`).  The loss root's noise is drawn on the device:
# its margins are 2.5e-6 and 2.7e-6 as measured there (K + 201 gives 3.7e-8 at K = 320 and 1.4e-7 at K = 384)
LOSS_SEED = {320: 321, 384: 385}
COTANGENT_SEED = {320: 343, 384: 406}  # margins 1.4e-6 and 2.2e-6 (344 gives 5.1e-7 at K = 320, 407 gives 6e-8 at K = 384)


@pytest.mark.parametrize("K", [320, 384])
def test_training_loss_gradients_vs_float64_oracle(hip, K):
    """BWD_LOSSES (DiffAb.hotpath_train_losses): the three losses, both contexts and every denoiser parameter."""
    model, sd = diffab(seed=LOSS_SEED[K])
    inp = gradient_inputs(K)
    dev = {k: v.cuda() for k, v in inp.items()}
    t = torch.tensor([37, 6])
    torch.manual_seed(K)
    nz = model._add_noise(dev["seq_idx"], dev["translations"], dev["orientations"], dev["generation_mask"], t.cuda())
    beta = model.sched["beta"][t]
    rc = dev["res_context_emb"].clone().requires_grad_(True)
    pc = dev["pair_context_emb"].clone().requires_grad_(True)
    ls = model.hotpath_train_losses(nz, rc, pc, beta.cuda(), dev["orientations"], dev["generation_mask"], dev["residue_mask"])
    (ls[0] + ls[1] + ls[2]).backward()

    def oracle(dtype):
        c = lambda v: as_type(v, dtype)
        rco, pco = c(inp["res_context_emb"]).requires_grad_(True), c(inp["pair_context_emb"]).requires_grad_(True)
        sdo = leaves_as(sd, "denoiser.", dtype)
        den = orc.denoiser(sdo, nz["seq_idx_t"].cpu(), c(nz["translations_t"]), c(nz["orientations_t"]), rco, pco, c(beta), DIMS["NL"],
                           DIMS["H"])
        lo = orc.hotpath_losses(den, c(nz["seq_posterior"]), c(nz["translations_eps"]), c(inp["orientations"]), inp["generation_mask"],
                                inp["residue_mask"])
        (lo[0] + lo[1] + lo[2]).backward()
        return den, lo, rco.grad, pco.grad, sdo

    den, lo, rg, pg, sdo = oracle(torch.float64)
    _, lo32, rg32, pg32, sdo32 = oracle(torch.float32)
    margin = relu_margin(sd, nz["seq_idx_t"].cpu(), inp["res_context_emb"], den, beta)
    assert margin > 5e-7, ("inputs on a ReLU kink: pick another weight seed", margin)
    for i, name in enumerate(("seq", "eps", "orientation")):
        rel, rel32 = abs(float(ls[i]) - float(lo[i])) / abs(float(lo[i])), abs(float(lo32[i]) - float(lo[i])) / abs(float(lo[i]))
        print(f"K={K} {name} loss: kernel {rel:.2e}, fp32 oracle {rel32:.2e}")
        assert rel < max(5e-5, 2.0 * rel32), (K, name, rel, rel32)
    hold(f"K={K} losses d res_ctx", rc.grad, rg32, rg, GTOL)
    hold(f"K={K} losses d pair_ctx", pc.grad, pg32, pg, GTOL)
    print(f"K={K} losses, fp32 oracle's worst parameter gradient:", worst_param(sdo, sdo32))
    check_params(model.denoiser.named_parameters(), sdo, "denoiser.", f"K={K} losses (ReLU margin {margin:.1e})")


@pytest.mark.parametrize("K", [320, 384])
def test_denoiser_cotangent_gradients_vs_float64_oracle(hip, K):
    """BWD_COTANGENTS (Denoiser under autograd): seeded random cotangents on eps, O0 and the posterior; the contexts, x_t and O_t as leaves."""
    den, sd = denoiser(seed=COTANGENT_SEED[K])
    den.train()
    inp = gradient_inputs(K)
    beta = torch.tensor([0.05, 0.4])
    g = torch.Generator().manual_seed(K)
    cot = {"translations_eps": torch.randn(2, K, 3, generator=g), "orientations_t0": torch.randn(2, K, 3, 3, generator=g),
           "seq_posterior": torch.randn(2, K, 21, generator=g)}
    lv = {k: inp[k].cuda().requires_grad_(True) for k in ARGS[1:]}
    out = den(inp["seq_idx"].cuda(), lv["translations"], lv["orientations"], lv["res_context_emb"], lv["pair_context_emb"], beta.cuda(),
              None, None)
    sum((out[k] * c.cuda()).sum() for k, c in cot.items()).backward()

    def oracle(dtype):
        lo = {k: as_type(inp[k], dtype).requires_grad_(True) for k in ARGS[1:]}
        sdo = leaves_as(sd, "denoiser.", dtype)
        want = orc.denoiser(sdo, inp["seq_idx"], lo["translations"], lo["orientations"], lo["res_context_emb"], lo["pair_context_emb"],
                            beta.to(dtype), DIMS["NL"], DIMS["H"])
        sum((want[k] * c.to(dtype)).sum() for k, c in cot.items()).backward()
        return want, lo, sdo

    want, lo, sdo = oracle(torch.float64)
    _, lo32, sdo32 = oracle(torch.float32)
    assert relu_margin(sd, inp["seq_idx"], inp["res_context_emb"], want, beta) > 5e-7, "inputs on a ReLU kink: pick another weight seed"
    for k in ARGS[1:]:
        assert torch.isfinite(lv[k].grad).all(), (K, k)
        hold(f"K={K} cotangents d {k}", lv[k].grad, lo32[k].grad, lo[k].grad, GTOL)
    print(f"K={K} cotangents, fp32 oracle's worst parameter gradient:", worst_param(sdo, sdo32))
    check_params(den.named_parameters(), sdo, "denoiser.", f"K={K} cotangents")


@pytest.mark.parametrize("K", [320, 384, 640])
def test_ipa_layer_gradients_vs_float64_oracle(hip, K):
    """BWD_LAYER (one InvariantPointAttentionLayer under autograd): d x, d e, d R, d t and the layer's parameters from a random d y.
    K = 640 (B = 1, NL = 1) is the one-row kernel above 64 KiB of dynamic LDS."""
    B = batch_of(K)
    den, _ = denoiser(seed=K + 3, dims=dict(DIMS, NL=1) if K >= 640 else DIMS)
    layer = den.ipa.layers[-1]
    inp = gradient_inputs(K)
    g = torch.Generator().manual_seed(K + 1)
    cy = torch.randn(B, K, DIMS["D"], generator=g)
    lv = {k: inp[k].cuda().requires_grad_(True) for k in LAYER_IN}
    y = layer(*[lv[k] for k in LAYER_IN])
    (y * cy.cuda()).sum().backward()

    def oracle(dtype):
        lo = {k: as_type(inp[k], dtype).requires_grad_(True) for k in LAYER_IN}
        sdo = leaves_as({n: p for n, p in layer.named_parameters()}, "L.", dtype)
        want = orc.ipa_layer(*[lo[k] for k in LAYER_IN], sdo, "L.", DIMS["H"])
        (want * cy.to(dtype)).sum().backward()
        return want.detach(), lo, sdo

    want, lo, sdo = oracle(torch.float64)
    want32, lo32, sdo32 = oracle(torch.float32)
    hold_forward(f"K={K} layer y", y, want32, want)
    for k in LAYER_IN:
        assert torch.isfinite(lv[k].grad).all(), (K, k)
        hold(f"K={K} layer d {k}", lv[k].grad, lo32[k].grad, lo[k].grad, GTOL)
    print(f"K={K} layer, fp32 oracle's worst parameter gradient:", worst_param(sdo, sdo32))
    check_params(layer.named_parameters(), sdo, "L.", f"K={K} layer")


# ------------------------------------------------------------------ 4. sampler and scorer above the patch-resident module launch
@pytest.mark.parametrize("K", [320, 384])
def test_reverse_step_teacher_forced(hip, K):
    """One reverse step (per-layer launches, last-layer tile map, pair planes) against the oracle: x and O within 1e-4, a differing
    sequence draw only within 1e-5 of an edge of the posterior's CDF, padded and non-generated residues bitwise unchanged."""
    model, sd0 = diffab(seed=K + 4)
    sd = {"denoiser." + k: v for k, v in sd0.items()}
    sched = orc.cosine_variance_schedule(100, s=0.01, beta_max=0.999)
    inp = padded(2, K, n_real_of(K), seed=300 + K)
    gm = inp["generation_mask"].clone()
    gm[:, : K // 2] = True
    gm &= inp["residue_mask"]
    keep = ~gm
    rev = model._reverse_so3()
    seed, first, t = 4243, 5, 57
    got = model.sample(inp["seq_idx"], inp["translations"], inp["orientations"], res_context_emb=inp["res_context_emb"],
                       pair_context_emb=inp["pair_context_emb"], generation_mask=gm, seed=seed, first_patch=first, t_start=t, t_stop=t - 1,
                       init=False)
    s1, x1, O1, den, us, edge = oracle_reverse_step(sd, inp, gm, rev, sched, seed, first, t, DIMS["NL"], DIMS["H"])
    assert maxrel(got["translations"], x1) < TOL, (K, t, maxrel(got["translations"], x1))
    assert maxrel(got["orientations"], O1) < TOL, (K, t, maxrel(got["orientations"], O1))
    diff = got["seq_idx"].cpu() != s1
    if diff.any():
        assert float(edge[diff].max()) < 1e-5, (K, t, float(edge[diff].max()))
    for k in ("seq_idx", "translations", "orientations"):
        assert torch.equal(got[k].cpu()[keep], inp[k][keep]), (K, t, k)
    print(f"teacher-forced reverse step, K={K}: x {maxrel(got['translations'], x1):.2e}, O {maxrel(got['orientations'], O1):.2e}, "
          f"{int(diff.sum())} of {int(gm.sum())} sequence draws on a CDF edge")


def sampler_inputs(B, K):
    """Patch 0 padded with a generated block in its real part, patch 1 whole with generated residues ONLY in its last 16-row tile, a
    third patch (if any) with nothing generated."""
    inp = {k: v.cuda() for k, v in padded(B, K, n_real_of(K), seed=400 + K).items()}
    gm = torch.zeros(B, K, dtype=torch.bool, device="cuda")
    gm[0, 30:50] = True
    gm[1, K - 16:] = True
    inp["generation_mask"] = gm
    return inp


@pytest.mark.parametrize("K", [320, 384, 1024])
def test_skipped_last_layer_rows_are_bitwise_the_all_rows_sampler(hip, K):
    """The default sampler (the last layer's attention only on the K / 16-tile map's live tiles) = DIFFAB_FLAG_ALL_ROWS, eager and graph
    replay.  The only generated residues of patch 1 lie in its last tile (tile 63 at K = 1024): a misplaced tile changes its trajectory."""
    model, _ = diffab(seed=K + 5)
    inp = sampler_inputs(2, K)
    gm = inp["generation_mask"]
    kw = dict(res_context_emb=inp["res_context_emb"], pair_context_emb=inp["pair_context_emb"], generation_mask=gm, seed=19, t_start=40,
              t_stop=37)
    full = model.sample(inp["seq_idx"], inp["translations"], inp["orientations"], skip_unused_rows=False, **kw)
    assert torch.isfinite(full["translations"]).all() and torch.isfinite(full["orientations"]).all()
    assert not torch.equal(full["translations"][1, -1], inp["translations"][1, -1])  # the last-tile residues did move
    for graph in (False, True):
        lean = model.sample(inp["seq_idx"], inp["translations"], inp["orientations"], skip_unused_rows=True, graph=graph, **kw)
        for k in full:
            assert torch.equal(full[k], lean[k]), (K, graph, k)
    for k in ("seq_idx", "translations", "orientations"):
        assert torch.equal(full[k][~gm], inp[k][~gm]), (K, k)


def test_sampler_shards_and_num_samples_are_bitwise_at_k384(hip):
    """Shards of the batch (noise keyed by the global patch id) and num_samples = 2 (shared contexts through the row map) are bitwise the
    full batch and the replicated batch."""
    K = 384
    model, _ = diffab(seed=K + 6)
    inp = sampler_inputs(3, K)
    st = ("seq_idx", "translations", "orientations")
    ctx = ("res_context_emb", "pair_context_emb")
    kw = dict(seed=23, t_start=30, t_stop=27)
    full = model.sample(*[inp[k] for k in st], generation_mask=inp["generation_mask"], **{k: inp[k] for k in ctx}, **kw)
    parts = [model.sample(*[inp[k][lo:hi] for k in st], generation_mask=inp["generation_mask"][lo:hi], first_patch=lo,
                          **{k: inp[k][lo:hi] for k in ctx}, **kw) for lo, hi in ((0, 1), (1, 3))]
    for k in full:
        assert torch.equal(torch.cat([p[k] for p in parts]), full[k]), (K, k)
    many = model.sample(*[inp[k] for k in st], generation_mask=inp["generation_mask"], num_samples=2, **{k: inp[k] for k in ctx}, **kw)
    rep = {k: v.repeat_interleave(2, dim=0) for k, v in inp.items()}
    want = model.sample(*[rep[k] for k in st], generation_mask=rep["generation_mask"], **{k: rep[k] for k in ctx}, **kw)
    for k in want:
        assert torch.equal(many[k], want[k]), (K, k)
    assert not torch.equal(many["translations"][2], many["translations"][3])  # the two designs of patch 1 differ


def test_score_terms_at_k384_vs_oracle(hip):
    """DiffAb.score per-residue and per-step terms of two designs at K = 384 (patch 0 padded) against the oracle, as
    tests/test_gpu_score.py checks them at K = 16 / 128."""
    from test_gpu_score import check_terms

    K = 384
    model, _ = diffab(seed=K + 7)
    inp = {k: v.cuda() for k, v in padded(2, K, n_real_of(K), seed=500 + K).items()}
    inp["generation_mask"][:, 40:70] = True
    inp["generation_mask"] &= inp["residue_mask"]
    out = model.score(inp["seq_idx"], inp["translations"], inp["orientations"], generation_mask=inp["generation_mask"],
                      residue_mask=inp["residue_mask"], res_context_emb=inp["res_context_emb"], pair_context_emb=inp["pair_context_emb"],
                      t=[1, 50], seed=11, per_residue=True, return_noised=True)
    check_terms(model, DIMS, inp, out, torch.arange(2, device="cuda"), range(2), 1)
    pad = ~inp["residue_mask"]
    assert torch.equal(out["per_residue"][0, :, :, pad[0]], torch.zeros_like(out["per_residue"][0, :, :, pad[0]]))
