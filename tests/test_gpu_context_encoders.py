"""The two context encoders (DiffAb.encode_context: ResidueEmbedding + PairEmbedding) forward and every parameter gradient against a
float64 restatement, at the shapes where the HIP code changes kernels.

PairEmbedding picks its launches from C, K, n_atoms (A), max_dist_to_consider (md), the backward chunk and two diagnostic bits of
diffab_debug_set_attn_variant (4: unfused, 64: the fused backward's separate launches).  At C = 64 (the benchmark model, D = 128):

  case                 K    A   md   forward                         backward (beyond the shared launches)
  fused_A4             128   4  32   pair_embed_fused_kernel         pair_chain_bwd_kernel, pair_enc_tn_kernel<20>, pair_table_mfma_kernel,
                                                                     pair_dist_bwd_fused64_kernel (A A = 16)
  fused_A15            128  15  32   pair_embed_fused_kernel         as fused_A4; all four generate_structure / generate_sequence flags
                                                                     (generate_sequence=False: a null sequence mask); distances from xyz and
                                                                     from the materialised tensor
  fused_A16            128  16  32   pair_embed_fused_kernel         as fused_A4 at the last fused A and the last A A <= 256
  fused_md8 / md37     128  15  8/37 pair_embed_fused_kernel         as fused_A4; 37 is the last max_dist whose tables fit the fused kernel
  fused_k256           256  15  32   pair_embed_fused_kernel         as fused_A4, two 128-row tiles per (patch, i)
  variant 4 (A15, k256)         unfused launches (below)        pair_cat_bwd_lds_kernel, pair_dist_bwd_mfma_kernel
  variant 64 (A15, k256)        pair_embed_fused_kernel         pair_mask_bwd_kernel, gemm_nn_mfma_kernel<true> (bwd_gemm_nn_masked), tn64_kernel
                                                                     (bwd_tn64_set), pair_table_scatter_kernel, bwd_linear + pair_dist_bwd_group_kernel
  unfused_A17          128  17  32   pair_dist_kernel, pair_cat_kernel pair_cat_bwd_lds_kernel, pair_dist_bwd_mfma_kernel at A A = 289; from xyz
                                                                     and from the materialised tensor
  unfused_A17_k64       64  17  32   unfused                         pair_cat_bwd_lds_kernel, pair_dist_bwd_group_kernel (21 A^2 floats: 24 KiB)
  unfused_A28_k64       64  28  32   unfused                         pair_dist_bwd_group_kernel with its LDS raised past 64 KiB (64.3 KiB)
  unfused_md38         128  15  38   unfused (tables too large)      pair_cat_bwd_lds_kernel, pair_dist_bwd_mfma_kernel
  unfused_md80         128  15  80   unfused                         pair_cat_bwd_kernel (tables past 150 KiB); residue_idx = arange(K) shared,
                                                                     |i - j| up to 127 clamped to 80
  unfused_k64          64   15  32   unfused                         pair_cat_bwd_lds_kernel, pair_dist_bwd_group_kernel; all four flags
  unfused_k192/k173   192/173 15 32  unfused (173: K % 4 != 0)       pair_cat_bwd_lds_kernel, pair_dist_bwd_group_kernel
  chunks fused         128  15  32   fused, B = 40                   two backward chunks (31 + 9 patches), taped and recomputing
                                                                     (DIFFAB_PAIR_TAPE=0: pair_embed_fused_kernel<true> inside the backward)
  chunks unfused       173  15  32   unfused, B = 8                  two forward and two backward chunks (6 + 2 patches)

The unfused forward is pair_dist_kernel, pair_cat_kernel, the row linears and pair_mask_kernel; every case also runs residue_feat_kernel
and residue_embed_bwd_kernel (input width 2 D + 63 A + 39).  pair_dist_bwd_kernel (per-row atomics) needs 21 A^2 floats past 160 KiB
(A >= 45) and is not reached; every other kernel named here shows in a rocprofv3 --kernel-trace run of this file.  Cases are B = 2 with
patch 0's tail padded as collate_fn pads it (atom mask 0, xyz 0, chain 0 = the chain embedding's padding index, UNK,
outside residue_mask); chain ids 1..9 in several contiguous chains per patch (chain products up to 81); a (B, K) residue_idx whose rows differ per patch, with gaps that clamp both ways (except unfused_md80).  Distances come from xyz on the device
(distmat=None) unless a case says otherwise.  Oracle: oracle/diffab_oracle.py in float64 on the host (distances from xyz in float64), its
autograd from random cotangents on both outputs; the chunk cases put the cotangents on one patch of the second chunk only, so every gradient
is that patch's alone and the oracle runs on it.  Cotangents are zero on the few rows with a ReLU pre-activation within fp32 rounding of
its kink (run_oracle), so no draw can put a kink between the kernel and the oracle.
"""
import os

import pytest
import torch

import diffab_oracle as orc
from conftest import elemrel, elemrel_by_decade, maxrel
from diffab_pytorch import synthetic as syn
from sampler_support import hip

pytestmark = pytest.mark.gpu
FMAX, FELEM = 2e-5, 1e-4  # forward: max-rel and element-wise bars (tests/conftest.py)
GTOL = 2e-4               # gradients, per parameter
DIMS = syn.BENCH_DIMS
RES, PAIR = "residue_context_embedding.", "pair_context_embedding."
CE = RES + "chain_embedding.weight"
RES_RELU = [RES + "mlp.0", RES + "mlp.2", RES + "mlp.4"]
PAIR_RELU = [PAIR + "distance_embedding.0", PAIR + "distance_embedding.2", PAIR + "mlp.0", PAIR + "mlp.2"]
KINK = 1e-5  # of the magnitude a pre-activation's rounding scales with, |x| |W|^T + |b| (run_oracle)
ALL_FLAGS = [(True, True), (True, False), (False, True), (False, False)]

# name: (K, A, max_dist, extra); extra: flags = the (generate_structure, generate_sequence) pairs, distmat = also from the materialised
# tensor, variants = the diagnostic variants also run, shared_ri = residue_idx arange(K) shared by the patches
CASES = {
    "fused_A4": (128, 4, 32, {}),
    "fused_A15": (128, 15, 32, dict(flags=ALL_FLAGS, distmat=True, variants=(4, 64))),
    "fused_A16": (128, 16, 32, {}),
    "fused_md8": (128, 15, 8, {}),
    "fused_md37": (128, 15, 37, {}),
    "fused_k256": (256, 15, 32, dict(variants=(4, 64))),
    "unfused_A17": (128, 17, 32, dict(distmat=True)),
    "unfused_A17_k64": (64, 17, 32, {}),
    "unfused_A28_k64": (64, 28, 32, {}),
    "unfused_md38": (128, 15, 38, {}),
    "unfused_md80": (128, 15, 80, dict(shared_ri=True)),
    "unfused_k64": (64, 15, 32, dict(flags=ALL_FLAGS)),
    "unfused_k192": (192, 15, 32, {}),
    "unfused_k173": (173, 15, 32, {}),
}


def _runs():
    out = []
    for name, (K, A, md, ex) in CASES.items():
        for gs, gq in ex.get("flags", [(True, True)]):
            out.append(pytest.param(name, gs, gq, "xyz", 0, id=f"{name}-gs{int(gs)}gq{int(gq)}-xyz"))
        if ex.get("distmat"):
            out.append(pytest.param(name, True, True, "distmat", 0, id=f"{name}-gs1gq1-distmat"))
        for v in ex.get("variants", ()):
            out.append(pytest.param(name, True, True, "xyz", v, id=f"{name}-gs1gq1-xyz-variant{v}"))
    return out


def model_for(A, md, seed):
    from diffab_pytorch import DiffAb

    d = DIMS
    model = DiffAb(d["D"], d["C"], 1, d["DS"], d["PQ"], d["PV"], d["H"], n_atoms=A, max_dist_to_consider=md).cuda()
    sd = syn.context_state_dict(d["D"], d["C"], A, md, seed=seed)  # pair2distcoef random (zero upstream): the distance feature depends on it
    missing = model.load_state_dict(sd, strict=False)
    assert not missing.unexpected_keys and len(sd) == 23
    return model, sd


def batch_for(B, K, A, seed, shared_ri=False):
    cb = syn.context_batch(B, K, A, seed=seed, with_distmat=False, max_chain=9, per_patch_residue_idx=not shared_ri, n_pad=K // 5)
    del cb["distmat"]
    return cb


def host_distmat(xyz):
    x = xyz.double()
    return (x[:, :, None, :, None, :] - x[:, None, :, None, :, :]).norm(dim=-1)


def cotangents(B, K, seed, only=None):
    g = torch.Generator().manual_seed(seed)
    G1 = torch.randn(B, K, DIMS["D"], generator=g)
    G2 = torch.randn(B, K, K, DIMS["C"], generator=g)
    if only is not None:
        keep = torch.zeros(B, dtype=torch.bool)
        keep[only] = True
        G1[~keep] = 0.0
        G2[~keep] = 0.0
    return G1, G2


def run_hip(hip, model, cb, gs, gq, G1, G2, distmat=None, variant=0, tape=True):
    dev = {k: v.cuda() for k, v in cb.items()}
    hip.diffab_debug_set_attn_variant(variant)
    if not tape:
        os.environ["DIFFAB_PAIR_TAPE"] = "0"
    try:
        model.zero_grad(set_to_none=True)
        res, pair = model.encode_context(dev["seq_idx"], dev["xyz"], dev["orientations"], dev["backbone_dihedrals"], distmat,
                                         dev["pairwise_dihedrals"], dev["atom_mask"], dev["chain_idx"], dev["residue_idx"],
                                         dev["generation_mask"], dev["residue_mask"], generate_structure=gs, generate_sequence=gq)
        ((res * G1.cuda()).sum() + (pair * G2.cuda()).sum()).backward()
        torch.cuda.synchronize()
    finally:
        hip.diffab_debug_set_attn_variant(0)
        os.environ.pop("DIFFAB_PAIR_TAPE", None)
    grads = {n: p.grad.detach().cpu() for n, p in model.named_parameters() if n.startswith((RES, PAIR))}
    return res.detach().cpu(), pair.detach().cpu(), grads


def run_oracle(sd, cb, gs, gq, md, G1, G2, patch=None):
    """encode_context in float64 and its autograd; patch: that patch alone (the cotangents of the others are zero).

    A ReLU pre-activation within fp32 rounding of 0 can take the other side of the kink in the kernel: the forward barely moves (the
    function is continuous there), but that unit's gradient is dropped or kept whole, and one such row moves a row of a table gradient
    (aa_pair_type_embedding, pair2distcoef) by ~1e-3 of its maximum - the float32 oracle on the host misses the 2e-4 bar by as much at
    K = 192 (1.1e-3) and K = 256 (4.3e-4).  With 2 K^2 x 64 x 4 pair pre-activations some always lie that close, whatever the seed.  So
    the cotangents are zeroed on the residue rows and pair rows (every row is its own MLP) that hold a pre-activation z with
    |z| < KINK (|x| |W|^T + |b|), 1e-5 of the magnitude its rounding scales with: no kink can reach a gradient, for any draw, and the rows
    left out are counted (~0.5 % of the pair rows; 2 - 12 % of the residue rows, whose first layer sums ~1200 products)."""
    sl = slice(None) if patch is None else slice(patch, patch + 1)
    B = cb["seq_idx"].shape[0]
    b = {k: v[sl] if v.shape[0] == B else v for k, v in cb.items()}
    b = {k: v.double() if v.is_floating_point() else v for k, v in b.items()}
    b["distmat"] = host_distmat(b["xyz"])
    sdo = {k: v.double().requires_grad_(True) for k, v in sd.items()}
    z = {}
    res, pair = orc.encode_context(sdo, b, gs, gq, max_dist=md, preacts=z)
    assert sorted(z) == sorted(RES_RELU + PAIR_RELU), sorted(z)
    near = lambda names: torch.stack([(z[n][0].abs() < KINK * z[n][1]).any(-1) for n in names]).any(0)
    kink_res, kink_pair = near(RES_RELU), near(PAIR_RELU)
    G1, G2 = G1.clone(), G2.clone()
    G1[sl][kink_res] = 0.0
    G2[sl][kink_pair] = 0.0
    frac = (float(kink_res.double().mean()), float(kink_pair.double().mean()))
    assert frac[0] < 0.25 and frac[1] < 0.02, frac  # the check still covers most residue rows and nearly every pair row
    ((res * G1[sl].double()).sum() + (pair * G2[sl].double()).sum()).backward()
    print(f"rows with a pre-activation within {KINK:.0e} of a kink (cotangent 0): residue {frac[0]:.2%}, pair {frac[1]:.2%}")
    return res.detach(), pair.detach(), {k: v.grad for k, v in sdo.items()}, G1, G2


def check_forward(tag, got, want):
    for k, g_, w_ in (("res", got[0], want[0]), ("pair", got[1], want[1])):
        assert torch.isfinite(g_).all(), (tag, k)
        m, e = maxrel(g_, w_), elemrel(g_, w_)
        assert m < FMAX and e < FELEM, (tag, k, m, e, elemrel_by_decade(g_, w_))


def check_grads(tag, grads, want, chain0):
    assert len(grads) == 23, sorted(grads)
    worst = ("", 0.0)
    for n, g_ in grads.items():
        w_ = want[n]
        assert float(w_.abs().max()) > 0.0, (tag, n)  # every parameter takes part
        if n == CE:
            # padding_idx = 0 (reference :65): row 0 takes no gradient; the oracle's plain lookup gives it one
            if chain0:
                assert float(g_[0].abs().max()) == 0.0, tag
            g_, w_ = g_[1:], w_[1:]
        r = maxrel(g_, w_)
        worst = max(worst, (n, r), key=lambda t_: t_[1])
        assert r < GTOL, (tag, n, r, elemrel_by_decade(g_, w_))
    print(tag, "worst parameter gradient max-rel:", worst)


_ORACLE = {}


def case_data(name, gs, gq):
    K, A, md, ex = CASES[name]
    seed = sum(map(ord, name)) % 1000
    key = (name, gs, gq)
    if key not in _ORACLE:
        cb = batch_for(2, K, A, seed, shared_ri=ex.get("shared_ri", False))
        G1, G2 = cotangents(2, K, seed)
        sd = syn.context_state_dict(DIMS["D"], DIMS["C"], A, md, seed=seed)
        _ORACLE.clear()  # one case's float64 activations at a time
        *want, G1, G2 = run_oracle(sd, cb, gs, gq, md, G1, G2)
        _ORACLE[key] = (cb, G1, G2, want)
    return seed, _ORACLE[key]


@pytest.mark.parametrize("name,gs,gq,src,variant", _runs())
def test_encode_context_vs_float64_oracle(hip, name, gs, gq, src, variant):
    K, A, md, ex = CASES[name]
    seed, (cb, G1, G2, want) = case_data(name, gs, gq)
    rel = cb["residue_idx"][:, :, None] - cb["residue_idx"][:, None, :]
    assert int(rel.max()) > md and int(rel.min()) < -md  # the window clamps both ways
    assert int((cb["chain_idx"][:, :, None] * cb["chain_idx"][:, None, :]).max()) == 81
    model, _ = model_for(A, md, seed)
    distmat = host_distmat(cb["xyz"]).float().cuda() if src == "distmat" else None
    got = run_hip(hip, model, cb, gs, gq, G1, G2, distmat=distmat, variant=variant)
    tag = f"{name} gs={gs} gq={gq} {src} variant={variant}"
    check_forward(tag, got[:2], want[:2])
    check_grads(tag, got[2], want[2], chain0=bool((cb["chain_idx"] == 0).any()))


@pytest.mark.parametrize("fused,tape", [(True, True), (True, False), (False, True)], ids=["fused-taped", "fused-recompute", "unfused"])
def test_backward_chunks_vs_float64_oracle(hip, fused, tape):
    """Several backward chunks: B = 40 at K = 128 (fused: 31 + 9 patches; the taped form keeps the whole batch's activations, the
    recomputing form reruns the fused forward per chunk) and B = 8 at K = 173 (unfused: 6 + 2 patches in the forward and in the backward,
    which has no taped form).  The cotangents are non-zero on one patch inside the second chunk (not its first), so a tile origin or
    per-patch stride that is wrong past the first chunk moves the gradients."""
    B, K, patch, seed = (40, 128, 33, 828) if fused else (8, 173, 7, 873)
    A, md = 15, 32
    cb = batch_for(B, K, A, seed)
    G1, G2 = cotangents(B, K, seed, only=patch)
    model, sd = model_for(A, md, seed)
    *want, G1, G2 = run_oracle(sd, cb, True, True, md, G1, G2, patch=patch)
    res, pair, grads = run_hip(hip, model, cb, True, True, G1, G2, tape=tape)
    tag = f"chunks B={B} K={K} patch {patch} {('fused taped' if tape else 'fused recomputing') if fused else 'unfused'}"
    check_forward(tag, (res[patch:patch + 1], pair[patch:patch + 1]), want[:2])
    check_grads(tag, grads, want[2], chain0=True)


def test_wide_fixture_vs_hip(hip, golden):
    """The reference's own encode_context at n_atoms / max_dist_to_consider = 4 / 8 and 17 / 40 (tests/golden/encode_context_wide.npz:
    D = 32, C = 16, K = 24, chain ids up to 9, a (B, K) residue_idx, patch 0 padded): the generic kernels, distances from xyz and from the
    materialised tensor, four flag combinations."""
    from diffab_pytorch import DiffAb

    g = golden("encode_context_wide")
    Bw, Kw, Dw, Cw, npad = [int(v) for v in g["meta"]]
    for si in range(2):
        A, md, seed = [int(v) for v in g[f"setting{si}"]]
        model = DiffAb(Dw, Cw, 1, 12, 4, 4, 8, n_atoms=A, max_dist_to_consider=md).cuda()
        sd = syn.context_state_dict(Dw, Cw, A, md, seed=seed)
        missing = model.load_state_dict(sd, strict=False)
        assert not missing.unexpected_keys and len(sd) == 23 and all(k.startswith("denoiser.") for k in missing.missing_keys)
        cb = {k: v.cuda() for k, v in syn.context_batch(Bw, Kw, A, seed=seed, max_chain=9, per_patch_residue_idx=True, n_pad=npad).items()}
        for gs, gq in ALL_FLAGS:
            for dm in (None, cb["distmat"]):
                with torch.no_grad():
                    res, pair = model.encode_context(cb["seq_idx"], cb["xyz"], cb["orientations"], cb["backbone_dihedrals"], dm,
                                                     cb["pairwise_dihedrals"], cb["atom_mask"], cb["chain_idx"], cb["residue_idx"],
                                                     cb["generation_mask"], cb["residue_mask"], generate_structure=gs, generate_sequence=gq)
                check_forward(f"wide A={A} md={md} gs={gs} gq={gq} {'xyz' if dm is None else 'distmat'}",
                              (res.cpu(), pair.cpu()), (torch.from_numpy(g[f"res_{si}_{int(gs)}{int(gq)}"]),
                                                        torch.from_numpy(g[f"pair_{si}_{int(gq)}"])))
