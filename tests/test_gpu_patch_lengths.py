"""The denoiser, its backward, the sampler and the scorer at the patch lengths training really sees, against a float64 restatement.

The reference builds a patch from the 128 residues nearest the CDR anchors unioned with the 128 nearest antigen residues (129..256
residues, mostly not a multiple of 64) and its collate function pads every batch to its longest complex, marking the padding in
residue_mask.  The HIP code picks different kernels as K changes; at the benchmark dims (D = 128, C = 64, H = 8, DS = 32, P = 8):

  K = 173  generic forward (K % 64 != 0); attention backward ipa_attn_bwd_rows_kernel -> ipa_attn_bwd_keys_kernel (K % 4 != 0: one
           query row / one key per work-group)
  K = 192  MFMA forward, three 64-key chunks; attention backward ipa_attn_bwd_rows_mr_kernel -> ipa_attn_bwd_keys_mfma_kernel<0/1> with
           TSRC = true (key side from the transposed At / Gt images; no taped probabilities at this K)
  K = 196  generic forward; attention backward ipa_attn_bwd_rows_mr_kernel -> ipa_attn_bwd_keys_mr_kernel<4> (K % 4 == 0)
  K = 256  MFMA forward, two 128-key chunks; attention backward ipa_attn_bwd_rows_mr_kernel -> ipa_attn_bwd_keys_mr_kernel<4> (its LDS
           is exactly 64 KiB; keys_mfma would need 68 KiB)
  K > 256  tests/test_gpu_long_patches.py continues this table (K = 320, 384, 512, 640, 1024: more and rescaled key chunks in the
           forward, the one-key and one-row attention backward kernels, the sampler past the patch-resident module launch)

Every case is B = 2 with patch 0 padded after ~4/5 of its residues (`padded`) and patch 1 whole.  The reference denoiser ignores the
masks (diffab_pytorch.py:566-567), so padded residues are keys like any other: their values and gradients are compared too.  Oracle:
oracle/diffab_oracle.py evaluated in float64 on the host.
"""
import numpy as np
import pytest
import torch

import diffab_oracle as orc
from conftest import elemrel, maxrel
from diffab_pytorch import synthetic as syn
from sampler_support import (ARGS, FLAGS, FLAG_IDS, GTOL, OUTS, PATCH_LENGTH_DIMS, TOL, UNK, check_params, f64, hip, leaves, make_model,
                             n_real_of, oracle_reverse_step, padded, relu_margin)

pytestmark = pytest.mark.gpu
DIMS = PATCH_LENGTH_DIMS
KS = [173, 192, 196, 256]


def denoiser(seed):
    from diffab_pytorch.diffab_pytorch import Denoiser

    d = DIMS
    den = Denoiser(d["D"], d["C"], d["NL"], d["DS"], d["PQ"], d["PV"], d["H"], 21)
    sd = syn.denoiser_state_dict(d, seed=seed, prefix="")
    den.load_state_dict(sd, strict=True)
    return den.cuda(), sd


def diffab(seed):
    return make_model(DIMS, seed), syn.denoiser_state_dict(DIMS, seed=seed, prefix="")


# ------------------------------------------------------------------ 1. forward parity
_FWD = {}


def forward_case(K, zero_orientations=False):
    key = (K, zero_orientations)
    if key not in _FWD:
        den, sd = denoiser(seed=K)
        den.requires_grad_(False)
        inp = padded(2, K, n_real_of(K), seed=100 + K, zero_orientations=zero_orientations)
        beta = torch.tensor([0.03, 0.7])
        want = orc.denoiser({"denoiser." + k: v.double() for k, v in sd.items()}, inp["seq_idx"], *[inp[k].double() for k in ARGS[1:]],
                            beta.double(), DIMS["NL"], DIMS["H"])
        _FWD[key] = (den, inp, beta, want)
    return _FWD[key]


def check_forward(K, flags, zero_orientations):
    den, inp, beta, want = forward_case(K, zero_orientations)
    out = den(*[inp[k].cuda() for k in ARGS], beta.cuda(), inp["generation_mask"].cuda(), inp["residue_mask"].cuda(), return_logits=True,
              flags=flags)
    for k in OUTS:
        fin = torch.isfinite(want[k])
        assert torch.isfinite(out[k].cpu()[fin]).all(), (K, flags, k)
        got, ref = out[k].cpu()[fin], want[k][fin]
        assert maxrel(got, ref) < TOL and elemrel(got, ref) < TOL, (K, flags, k, maxrel(got, ref), elemrel(got, ref))
    return out


@pytest.mark.parametrize("flags", FLAGS, ids=FLAG_IDS)
@pytest.mark.parametrize("K", KS)
def test_forward_vs_float64_oracle(hip, K, flags):
    """res_emb, aa_logits, eps, O0 and the posterior of a padded batch at every K, every flag (the three selectors are accepted where they
    do not apply and must agree there too)."""
    check_forward(K, flags, False)


@pytest.mark.parametrize("flags", FLAGS, ids=FLAG_IDS)
@pytest.mark.parametrize("K", [173, 192])
def test_forward_with_zero_padded_orientations(hip, K, flags):
    """The padded frames as the all-zero matrix (generic and MFMA forward): every output the oracle gives finite is finite and at the bar;
    the padded residues' O0 = 0 @ exp(hat v) is exactly zero."""
    out = check_forward(K, flags, True)
    n = n_real_of(K)
    assert float(out["orientations_t0"][0, n:].abs().max()) == 0.0


# ------------------------------------------------------------------ 2. gradient parity: the three roots of the backward
def gradient_inputs(K):
    inp = padded(2, K, n_real_of(K), seed=200 + K)
    gm = torch.zeros(2, K, dtype=torch.bool)
    gm[:, 10:70] = True  # a CDR-sized generated block in both patches, plus the generator's own segment where it is real
    gm |= inp["generation_mask"]
    inp["generation_mask"] = gm & inp["residue_mask"]
    return inp


@pytest.mark.parametrize("K", KS)
def test_training_loss_gradients_vs_float64_oracle(hip, K):
    """BWD_LOSSES (DiffAb.hotpath_train_losses): the three losses, both contexts and every denoiser parameter."""
    model, sd = diffab(seed=K + 1)
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
    rco, pco = f64(inp["res_context_emb"]).requires_grad_(True), f64(inp["pair_context_emb"]).requires_grad_(True)
    sdo = leaves(sd, "denoiser.")
    den = orc.denoiser(sdo, nz["seq_idx_t"].cpu(), f64(nz["translations_t"]), f64(nz["orientations_t"]), rco, pco, beta.double(),
                       DIMS["NL"], DIMS["H"])
    lo = orc.hotpath_losses(den, f64(nz["seq_posterior"]), f64(nz["translations_eps"]), f64(inp["orientations"]), inp["generation_mask"],
                            inp["residue_mask"])
    (lo[0] + lo[1] + lo[2]).backward()
    margin = relu_margin(sd, nz["seq_idx_t"].cpu(), inp["res_context_emb"], den, beta)
    np.testing.assert_allclose([float(v) for v in ls], [float(v) for v in lo], rtol=5e-5)
    assert maxrel(rc.grad, rco.grad) < GTOL, (K, maxrel(rc.grad, rco.grad), margin)
    assert maxrel(pc.grad, pco.grad) < GTOL, (K, maxrel(pc.grad, pco.grad), margin)
    check_params(model.denoiser.named_parameters(), sdo, "denoiser.", f"K={K} losses (ReLU margin {margin:.1e})")


@pytest.mark.parametrize("K", KS)
def test_denoiser_cotangent_gradients_vs_float64_oracle(hip, K):
    """BWD_COTANGENTS (Denoiser under autograd): seeded random cotangents on eps, O0 and the posterior; the contexts, x_t and O_t as leaves.
    The weight seed keeps every ReLU pre-activation >= 1e-6 away from 0 at all four K (`relu_margin`; seed K + 2 put one at 9e-8 at
    K = 196)."""
    den, sd = denoiser(seed=K + 22)
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
    lo = {k: f64(inp[k]).requires_grad_(True) for k in ARGS[1:]}
    sdo = leaves(sd, "denoiser.")
    want = orc.denoiser(sdo, inp["seq_idx"], lo["translations"], lo["orientations"], lo["res_context_emb"], lo["pair_context_emb"],
                        beta.double(), DIMS["NL"], DIMS["H"])
    sum((want[k] * c.double()).sum() for k, c in cot.items()).backward()
    assert relu_margin(sd, inp["seq_idx"], inp["res_context_emb"], want, beta) > 5e-7, "inputs on a ReLU kink: pick another weight seed"
    for k in ARGS[1:]:
        assert torch.isfinite(lv[k].grad).all(), (K, k)
        assert maxrel(lv[k].grad, lo[k].grad) < GTOL, (K, k, maxrel(lv[k].grad, lo[k].grad))
    check_params(den.named_parameters(), sdo, "denoiser.", f"K={K} cotangents")


@pytest.mark.parametrize("K", KS)
def test_ipa_layer_gradients_vs_float64_oracle(hip, K):
    """BWD_LAYER (one InvariantPointAttentionLayer under autograd): d x, d e, d R, d t and the layer's parameters from a random d y."""
    den, sd = denoiser(seed=K + 3)
    layer = den.ipa.layers[1]
    inp = gradient_inputs(K)
    g = torch.Generator().manual_seed(K + 1)
    cy = torch.randn(2, K, DIMS["D"], generator=g)
    names = ("res_context_emb", "pair_context_emb", "orientations", "translations")
    lv = {k: inp[k].cuda().requires_grad_(True) for k in names}
    y = layer(*[lv[k] for k in names])
    (y * cy.cuda()).sum().backward()
    lo = {k: f64(inp[k]).requires_grad_(True) for k in names}
    sdo = leaves({n: p for n, p in layer.named_parameters()}, "L.")
    want = orc.ipa_layer(*[lo[k] for k in names], sdo, "L.", DIMS["H"])
    assert maxrel(y, want) < TOL, (K, maxrel(y, want))
    (want * cy.double()).sum().backward()
    for k in names:
        assert maxrel(lv[k].grad, lo[k].grad) < GTOL, (K, k, maxrel(lv[k].grad, lo[k].grad))
    check_params(layer.named_parameters(), sdo, "L.", f"K={K} layer")


# ------------------------------------------------------------------ 3. sampler and scorer at ragged K
@pytest.mark.parametrize("K", [173, 196])
def test_reverse_step_teacher_forced_at_ragged_k(hip, K):
    """One reverse step at t in {100, 57, 8, 1} (the generic forward inside diffab_sample_loop) against the oracle: x and O within 1e-4, a
    differing sequence draw only within 1e-5 of an edge of the posterior's CDF, padded and non-generated residues bitwise unchanged."""
    model, sd0 = diffab(seed=K + 4)
    sd = {"denoiser." + k: v for k, v in sd0.items()}
    sched = orc.cosine_variance_schedule(100, s=0.01, beta_max=0.999)
    inp = padded(2, K, n_real_of(K), seed=300 + K)
    gm = inp["generation_mask"].clone()
    gm[:, : K // 2] = True
    gm &= inp["residue_mask"]
    keep = ~gm
    rev = model._reverse_so3()
    seed, first, flips = 4243, 5, 0
    for t in (100, 57, 8, 1):
        got = model.sample(inp["seq_idx"], inp["translations"], inp["orientations"], res_context_emb=inp["res_context_emb"],
                           pair_context_emb=inp["pair_context_emb"], generation_mask=gm, seed=seed, first_patch=first, t_start=t,
                           t_stop=t - 1, init=False)
        s1, x1, O1, den, us, edge = oracle_reverse_step(sd, inp, gm, rev, sched, seed, first, t, DIMS["NL"], DIMS["H"])
        assert maxrel(got["translations"], x1) < TOL, (K, t, maxrel(got["translations"], x1))
        assert maxrel(got["orientations"], O1) < TOL, (K, t, maxrel(got["orientations"], O1))
        diff = got["seq_idx"].cpu() != s1
        if diff.any():
            assert float(edge[diff].max()) < 1e-5, (K, t, float(edge[diff].max()))
            flips += int(diff.sum())
        for k in ("seq_idx", "translations", "orientations"):
            assert torch.equal(got[k].cpu()[keep], inp[k][keep]), (K, t, k)
    print(f"teacher-forced reverse steps, K={K}: {flips} of {4 * int(gm.sum())} sequence draws on a CDF edge")


def sampler_inputs(K):
    """3 patches: 0 padded with a generated block in its real part, 1 whole with generated residues ONLY in the last 16-row tile (partial
    when K % 16 != 0), 2 with nothing generated."""
    inp = {k: v.cuda() for k, v in padded(3, K, n_real_of(K), seed=400 + K).items()}
    gm = torch.zeros(3, K, dtype=torch.bool, device="cuda")
    gm[0, 30:50] = True
    last = (K - 1) // 16 * 16
    gm[1, last:] = True
    inp["generation_mask"] = gm
    return inp


@pytest.mark.parametrize("K", [173, 196, 192])
def test_skip_unused_rows_is_bitwise_the_full_sampler(hip, K):
    """skip_unused_rows=True = the full sampler, eager and graph replay.  At 173 / 196 the plan keeps every row (the tile map needs the
    MFMA path and K % 16 == 0: a partial last tile never reaches it); at 192 the tile map is live and the only generated residues of
    patch 1 lie in its last tile, so a misplaced last tile changes that patch's trajectory."""
    model, _ = diffab(seed=K + 5)
    inp = sampler_inputs(K)
    gm = inp["generation_mask"]
    kw = dict(res_context_emb=inp["res_context_emb"], pair_context_emb=inp["pair_context_emb"], generation_mask=gm, seed=19, t_start=40,
              t_stop=33)
    full = model.sample(inp["seq_idx"], inp["translations"], inp["orientations"], **kw)
    assert torch.isfinite(full["translations"]).all() and torch.isfinite(full["orientations"]).all()
    assert not torch.equal(full["translations"][1, -1], inp["translations"][1, -1])  # the last-tile residues did move
    for graph in (False, True):
        lean = model.sample(inp["seq_idx"], inp["translations"], inp["orientations"], skip_unused_rows=True, graph=graph, **kw)
        for k in full:
            assert torch.equal(full[k], lean[k]), (K, graph, k)
    for k in ("seq_idx", "translations", "orientations"):
        assert torch.equal(full[k][~gm], inp[k][~gm]), (K, k)


@pytest.mark.parametrize("K", [173, 196])
def test_sampler_shards_and_num_samples_are_bitwise(hip, K):
    """Shards of the batch (noise keyed by the global patch id) and num_samples = 2 (shared contexts through the row map) are bitwise the
    full batch and the replicated batch."""
    model, _ = diffab(seed=K + 6)
    inp = sampler_inputs(K)
    st = ("seq_idx", "translations", "orientations")
    ctx = ("res_context_emb", "pair_context_emb")
    kw = dict(seed=23, t_start=30, t_stop=24)
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


def test_score_terms_at_ragged_k_vs_oracle(hip):
    """DiffAb.score per-residue and per-step terms of two designs at K = 173 (patch 0 padded) against the oracle, as
    tests/test_gpu_score.py checks them at K = 16 / 128."""
    from test_gpu_score import check_terms

    K = 173
    model, _ = diffab(seed=K + 7)
    inp = {k: v.cuda() for k, v in padded(2, K, n_real_of(K), seed=500 + K).items()}
    inp["generation_mask"][:, 40:70] = True
    inp["generation_mask"] &= inp["residue_mask"]
    out = model.score(inp["seq_idx"], inp["translations"], inp["orientations"], generation_mask=inp["generation_mask"],
                      residue_mask=inp["residue_mask"], res_context_emb=inp["res_context_emb"], pair_context_emb=inp["pair_context_emb"],
                      t=[1, 9, 50], seed=11, per_residue=True, return_noised=True)
    check_terms(model, DIMS, inp, out, torch.arange(2, device="cuda"), range(3), 1)
    pad = ~inp["residue_mask"]
    assert torch.equal(out["per_residue"][0, :, :, pad[0]], torch.zeros_like(out["per_residue"][0, :, :, pad[0]]))


# ------------------------------------------------------------------ 4. the whole training step from a raw padded batch
def test_training_step_from_raw_padded_batch_vs_float64_oracle(hip):
    """DiffAb.training_step on a raw batch (15 atoms, chain ids, no contexts, no distances) at K = 173 with a padded tail (atom mask 0,
    chain 0 = the embedding's padding index, xyz 0, identity frames, residue_mask False): encode_context (the unfused pair embedding: the
    fused kernel takes K % 64 == 0 only) + noise + denoiser + losses + the HIP backward.  The loss masks are restricted to patch 0, so the
    losses and every gradient are that patch's alone: against the oracle's float64 autograd on it, distances built on the host."""
    from diffab_pytorch import features

    K, n = 173, n_real_of(173)
    model, sd = diffab(seed=K + 8)
    csd = syn.context_state_dict(DIMS["D"], DIMS["C"], 15, 32, seed=8)
    model.load_state_dict(csd, strict=False)
    cb = syn.context_batch(2, K, 15, seed=8, with_distmat=False)
    for k in ("distmat", "backbone_dihedrals", "pairwise_dihedrals"):  # raw: the step takes the dihedrals from xyz on the device
        del cb[k]
    cb["atom_mask"][0, n:] = 0.0
    cb["chain_idx"][0, n:] = 0
    cb["xyz"][0, n:] = 0.0
    cb["orientations"][0, n:] = torch.eye(3)
    cb["residue_mask"][0, n:] = False
    cb["seq_idx"][0, n:] = UNK
    cb["generation_mask"][0] = False
    cb["generation_mask"][0, 60:75] = True  # patch 0's CDR; patch 1 generates nothing: the losses are patch 0's
    cb["generation_mask"][1] = False
    batch = {k: v.cuda() for k, v in cb.items()}
    model.zero_grad(set_to_none=True)
    torch.manual_seed(31)
    loss = model.training_step(batch, 0)
    loss.backward()
    # the same t and noise again, and the device's own dihedral features (inputs, not differentiated)
    torch.manual_seed(31)
    t = torch.randint(low=1, high=model.T + 1, size=(2,))
    nz = model._add_noise(batch["seq_idx"], batch["xyz"][:, :, 1], batch["orientations"], batch["generation_mask"], t.cuda())
    feats = features.featurize(batch["xyz"], batch["chain_idx"], batch["residue_mask"], orientations=False)
    sl = slice(0, 1)
    c = lambda v: v[sl].detach().cpu()
    xyz = c(batch["xyz"]).double()
    b1 = {"seq_idx": c(batch["seq_idx"]), "xyz": xyz, "orientations": c(batch["orientations"]).double(),
          "backbone_dihedrals": c(feats["backbone_dihedrals"]).double(), "pairwise_dihedrals": c(feats["pairwise_dihedrals"]).double(),
          "atom_mask": c(batch["atom_mask"]).double(), "chain_idx": c(batch["chain_idx"]), "residue_idx": cb["residue_idx"],
          "generation_mask": c(batch["generation_mask"]), "residue_mask": c(batch["residue_mask"]),
          "distmat": (xyz[:, :, None, :, None, :] - xyz[:, None, :, None, :, :]).norm(dim=-1)}
    csdo = {k: f64(v).requires_grad_(True) for k, v in csd.items()}
    sdo = leaves(sd, "denoiser.")
    res, pair = orc.encode_context(csdo, b1, True, True)
    den = orc.denoiser(sdo, c(nz["seq_idx_t"]), f64(nz["translations_t"][sl]), f64(nz["orientations_t"][sl]), res, pair,
                       model.sched["beta"][t[sl]].double(), DIMS["NL"], DIMS["H"])
    lo = orc.hotpath_losses(den, f64(nz["seq_posterior"][sl]), f64(nz["translations_eps"][sl]), b1["orientations"], b1["generation_mask"],
                            b1["residue_mask"])
    want = lo[0] + lo[1] + lo[2]
    want.backward()
    assert abs(float(loss) - float(want)) < 5e-5 * abs(float(want)), (float(loss), float(want))
    params = dict(model.named_parameters())
    ref = dict(csdo, **sdo)
    names = ["residue_context_embedding.mlp.0.weight", "residue_context_embedding.mlp.6.bias",
             "residue_context_embedding.amino_acid_type_embedding.weight", "pair_context_embedding.mlp.0.weight",
             "pair_context_embedding.mlp.4.weight", "pair_context_embedding.distance_embedding.0.weight",
             "pair_context_embedding.pair2distcoef.weight", "pair_context_embedding.relpos_embedding.weight",
             "pair_context_embedding.aa_pair_type_embedding.weight", "denoiser.to_res_emb.0.weight", "denoiser.ipa.layers.0.to_pair_bias.weight",
             "denoiser.ipa.layers.1.to_out.weight", "denoiser.ipa.layers.0.gamma", "denoiser.sequence_denoising.4.weight"]
    worst = {n_: maxrel(params[n_].grad, ref[n_].grad) for n_ in names}
    # chain_embedding has padding_idx = 0 (reference :65): row 0 takes no gradient there; the oracle's plain lookup gives it one
    ce = "residue_context_embedding.chain_embedding.weight"
    assert float(params[ce].grad[0].abs().max()) == 0.0
    worst[ce] = maxrel(params[ce].grad[1:], ref[ce].grad[1:])
    print("raw padded training step, K=173, gradients vs the oracle:", {k: f"{v:.1e}" for k, v in worst.items()})
    assert max(worst.values()) < GTOL, worst
