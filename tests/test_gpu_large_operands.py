"""Late patches of a batch whose pair operands pass 4 GiB and 2^31 elements equal the same patches run alone.

At the benchmark dims (C = 64) a patch of K = 256 holds 2^22 fp32 pair elements = 2^24 bytes, and its two fp16 planes take the same
2^24 bytes.  In a batch of 520 patches a pair address therefore passes 4 GiB at patch 256 and element 2^31 at patch 512; the attention
images (B, H, K, K) pass element 2^31 at patch 4096 only and their byte offset 4 GiB at patch 2048, so they stay below both here.
include/diffab_hip.h asks for B K < 2^31 only: such batches are inside the contract.  A pair-row offset computed in 32 bits gives
finite, plausible numbers - patch 256 + n reads the rows of patch n (a byte offset that wraps at 2^32), patch 512 + n those of patch n
(an element index that wraps at 2^32 after its sign), or a negative offset in front of the operand - so the checks here are equalities:

  BIG   = device_patches(520, 256, PATCH_LENGTH_DIMS): every operand of every patch drawn independently on the device
  R     = [0, 255, 256, 511, 512, 519]: the first patch, the last one below and the first one past each border, the last patch
  SMALL = rows(BIG, R): the same six patches as a batch of their own (pair operand 100 MB)

and every entry gives on rows R of BIG what it gives on SMALL: bitwise where the suite already asserts that a shard is bitwise the
whole (the sampler, the scorer), otherwise at TOL / GTOL.  520 is the smallest multiple of 8 above 512; it is no multiple of the 256
CUs, so the module launch's walk of two patches per work-group ends ragged (8 work-groups take a third patch).  The fixture asserts
that no checked patch is a copy of the patch 256 or 512 rows before it: a wrapped address cannot read equal data.

profiles/large_operands.md has, per check, the operand that passes which border at which row, the measured time and the peak memory.
"""
import math
import time

import pytest
import torch

import diffab_oracle as orc
from diffab_pytorch import _hip, synthetic as syn
from sampler_support import (CTX, FLAG_IDS, FLAGS, GTOL, OUTS, PATCH_LENGTH_DIMS, STATE, TOL, assert_bitwise, bench_model, device_patches,
                             hip, make_model, oracle_reverse_step, rows, sample, score)

pytestmark = pytest.mark.gpu
DIMS = PATCH_LENGTH_DIMS
B_BIG, K_BIG = 520, 256
R = [0, 255, 256, 511, 512, 519]
LAYER_IN = ("res_context_emb", "pair_context_emb", "orientations", "translations")
# What the largest check holds at once: check 6 with the fixture's 8.7 GB pair operand, d e of the same size, the layer's tape and the
# backward's workspace - 25.33 GB allocated at its peak as measured (profiles/large_operands.md; the sampler's forms peak at 19.5 GB).
# The fixture skips only when less than this is free: the measured peak plus room for the caching allocator's rounding.
NEED_BYTES = 30 * 10**9


def rel(got, want):
    """conftest.maxrel on the device: max |got - want| / max |want|."""
    got, want = got.detach().double(), want.detach().double()
    return float((got - want).abs().max() / want.abs().max().clamp_min(1e-30))


@pytest.fixture(scope="module")
def big(hip):
    free = torch.cuda.mem_get_info()[0]
    if free < NEED_BYTES:
        pytest.skip(f"{free / 1e9:.1f} GB of device memory free, these checks hold up to {NEED_BYTES / 1e9:.0f} GB")
    model = make_model(DIMS, 23)
    model.load_state_dict(syn.context_state_dict(DIMS["D"], DIMS["C"], 15, 32, seed=7), strict=False)
    model.requires_grad_(False)
    inp = device_patches(B_BIG, K_BIG, DIMS, seed=520)
    at = torch.tensor(R, device="cuda")
    pair = inp["pair_context_emb"]
    assert pair.numel() > 2**31 and pair.numel() * 4 > 2**32
    for r in R:  # a wrapped address would have to read different data
        for back in (256, 512):
            if r >= back:
                assert not torch.equal(pair[r], pair[r - back]), (r, back)
                assert not torch.equal(inp["res_context_emb"][r], inp["res_context_emb"][r - back]), (r, back)
    # the sampler's masks: nothing generated in patch 512, only the last 16-row tile in patch 519 (the row plans differ at the border)
    gm = inp["generation_mask"].clone()
    gm[512] = False
    gm[519] = False
    gm[519, K_BIG - 16:] = True
    case = {"model": model, "big": inp, "small": rows(inp, at), "at": at, "sampler_mask": gm}
    yield case
    case.clear()
    inp.clear()
    del pair, gm
    torch.cuda.empty_cache()


@pytest.fixture(autouse=True)
def peak_memory():
    """Prints the test's wall time and peak device memory (what profiles/large_operands.md records)."""
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    t0 = time.perf_counter()
    yield
    torch.cuda.synchronize()
    print(f"\n[large operands] {time.perf_counter() - t0:.2f} s, peak {torch.cuda.max_memory_allocated() / 1e9:.2f} GB allocated")
    torch.cuda.empty_cache()


def at_rows(out, at):
    return {k: v.index_select(0, at) for k, v in out.items()}


# ------------------------------------------------------------------ 1. the sampler, every launch form
STEPS = dict(seed=31, t_start=40, t_stop=38, init=False)
FORMS = {"default": {}, "module": dict(flags=_hip.FLAG_PERSISTENT_MODULE), "multi_launch": dict(flags=_hip.FLAG_MULTI_LAUNCH),
         "pair_f32": dict(flags=_hip.FLAG_PAIR_F32), "generic": dict(flags=_hip.FLAG_FORCE_GENERIC), "all_rows": dict(flags=_hip.FLAG_ALL_ROWS),
         "graph": dict(graph=True)}


@pytest.mark.parametrize("form", list(FORMS))
def test_sampler_rows_past_the_borders_are_the_rows_alone(big, form):
    """Two reverse steps of all 520 patches: rows R are bitwise the six patches sampled one at a time under their global ids."""
    model, at = big["model"], big["at"]
    inp = dict(big["big"], generation_mask=big["sampler_mask"])
    got = at_rows(sample(model, inp, **STEPS, **FORMS[form]), at)
    assert torch.isfinite(got["translations"]).all() and torch.isfinite(got["orientations"]).all()
    alone = [sample(model, rows(inp, at[i:i + 1]), first_patch=r, **STEPS, **FORMS[form]) for i, r in enumerate(R)]
    want = {k: torch.cat([a[k] for a in alone]) for k in got}
    assert_bitwise(got, want, form)
    last = R.index(519)
    assert not torch.equal(want["translations"][last, -16:], inp["translations"][519, -16:])  # the last tile of the last patch moved
    for k in got:
        assert torch.equal(got[k][R.index(512)], inp[k][512]), k  # nothing generated in patch 512: untouched


def test_the_last_patch_alone_is_the_float64_oracle(big):
    """What anchors the `alone` side: one teacher-forced reverse step of patch 519 on its own (default form, global id 519) against the
    oracle in float64, at the bounds of test_reverse_step_teacher_forced_at_benchmark_geometry."""
    from conftest import maxrel

    model, at = big["model"], big["at"]
    inp = rows(dict(big["big"], generation_mask=big["sampler_mask"]), at[-1:])
    seed, t = 31, 40
    got = sample(model, inp, seed=seed, first_patch=519, t_start=t, t_stop=t - 1, init=False)
    sd = {"denoiser." + k: v for k, v in syn.denoiser_state_dict(DIMS, seed=23, prefix="").items()}
    sched = orc.cosine_variance_schedule(model.T, s=0.01, beta_max=0.999)
    host = {k: v.cpu() for k, v in inp.items()}
    gm = host["generation_mask"]
    s1, x1, O1, _, _, edge = oracle_reverse_step(sd, host, gm, model._reverse_so3(), sched, seed, 519, t, DIMS["NL"], DIMS["H"])
    ex, eO = maxrel(got["translations"], x1), maxrel(got["orientations"], O1)
    diff = got["seq_idx"].cpu() != s1
    print(f"patch 519 alone against the oracle: x {ex:.2e}, O {eO:.2e}, {int(diff.sum())} of {int(gm.sum())} sequence draws differ")
    assert ex < 1e-4 and eO < 1e-4, (ex, eO)
    if diff.any():
        assert float(edge[diff].max()) < 1e-5, float(edge[diff].max())
    assert not torch.equal(got["translations"].cpu()[gm], host["translations"][gm])


# ------------------------------------------------------------------ 2. shared contexts past the borders
@pytest.mark.parametrize("form", ["default", "module"])
def test_six_rows_from_520_shared_contexts(big, form):
    """context_index = R over the 520 contexts of BIG: the pair-plane split runs over all of them, the attention shifts its pair rows
    by up to 519 K rows, and six rows are denoised - bitwise the six patches with their own contexts."""
    model, at = big["model"], big["at"]
    inp = dict(big["big"], generation_mask=big["sampler_mask"])
    small = rows(inp, at)
    kw = dict(STEPS, **FORMS[form])
    got = sample(model, dict({k: small[k] for k in STATE}, **{k: inp[k] for k in CTX}), context_index=at, **kw)
    want = sample(model, small, **kw)
    assert_bitwise(got, want, form)
    assert not torch.equal(got["translations"][-1], small["translations"][-1])


# ------------------------------------------------------------------ 3. the denoiser's forward
@pytest.mark.parametrize("flags", FLAGS, ids=FLAG_IDS)
def test_denoiser_forward_rows(big, flags):
    """Denoiser.forward (eval) over the 520 patches, every flag: all five outputs at rows R against the six patches alone at TOL (no
    test of the suite holds this entry bitwise across batch sizes: the dense products pick their form by the row count)."""
    model, at, inp, small = big["model"], big["at"], big["big"], big["small"]
    g = torch.Generator(device="cuda").manual_seed(3)
    beta = 0.01 + 0.9 * torch.rand(B_BIG, device="cuda", generator=g)
    args = lambda d, bt: ([d[k] for k in ("seq_idx", "translations", "orientations", "res_context_emb", "pair_context_emb")] +
                          [bt, d["generation_mask"], torch.ones_like(d["generation_mask"])])
    with torch.no_grad():
        got = at_rows(model.denoiser(*args(inp, beta), return_logits=True, flags=flags), at)
        want = model.denoiser(*args(small, beta.index_select(0, at)), return_logits=True, flags=flags)
    for k in OUTS:
        assert torch.isfinite(got[k]).all(), k
        for i, r in enumerate(R):
            e = rel(got[k][i], want[k][i])
            assert e < TOL, (flags, k, r, e)
    print(f"flags={flags}:", {k: f"{rel(got[k], want[k]):.1e}" for k in OUTS})


# ------------------------------------------------------------------ 4. the scorer
def test_score_rows(big):
    """DiffAb.score over 520 designs (three launches of 256, 256 and 8 rows): every term at rows R is bitwise the design scored alone
    with first_design = r, as test_gpu_score.py asserts for its design ranges."""
    model, at, inp = big["model"], big["at"], big["big"]
    kw = dict(t=[9], num_draws=1, seed=17, per_residue=True)
    got = score(model, inp, **kw)
    keys = ("seq_loss", "translations_loss", "orientations_loss", "loss", "per_step", "per_residue")
    assert torch.isfinite(got["per_step"]).all() and (got["per_step"] > 0).all()
    for i, r in enumerate(R):
        one = score(model, rows(inp, at[i:i + 1]), first_design=r, **kw)
        for k in keys:
            assert torch.equal(got[k][r:r + 1], one[k]), (r, k)


# ------------------------------------------------------------------ 5. the pair embedding's forward
def raw_batch(B, K, seed, A=15):
    """A syn.context_batch-shaped raw batch drawn on the device (no distance tensor: it would be 7.6 GB)."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    rn = lambda *s: torch.randn(*s, device="cuda", generator=g)
    ru = lambda *s: torch.rand(*s, device="cuda", generator=g)
    ca = 8.0 * rn(B, K, 1, 3)
    xyz = ca + 1.5 * rn(B, K, A, 3)
    xyz[:, :, 1] = ca[:, :, 0]
    am = (ru(B, K, A) < 0.8).float()
    am[:, :, :4] = 1.0
    am[:, K - 1, 1] = 0.0  # one residue without CA
    start = torch.randint(0, K - 20, (B, 1), device="cuda", generator=g)
    length = torch.randint(5, 21, (B, 1), device="cuda", generator=g)
    pos = torch.arange(K, device="cuda")[None]
    rm = torch.ones(B, K, dtype=torch.bool, device="cuda")
    rm[:, 0] = False
    return {"seq_idx": torch.randint(0, 20, (B, K), device="cuda", generator=g), "xyz": xyz,
            "orientations": orc.uniform_rotation_from_normals(rn(B, K, 4).cpu()).cuda(),
            "backbone_dihedrals": (2 * ru(B, K, 3) - 1) * math.pi, "pairwise_dihedrals": (2 * ru(B, K, K, 2) - 1) * math.pi,
            "atom_mask": am, "chain_idx": torch.randint(1, 4, (B, K), device="cuda", generator=g).sort(dim=1).values,
            "generation_mask": (pos >= start) & (pos < start + length), "residue_mask": rm}


def test_encode_context_rows(big):
    """encode_context from a raw batch of 520 x 256 (distances from xyz inside the kernel): the pair embedding (520, 256, 256, 64) is
    written past element 2^31; rows R of both embeddings against the six patches encoded alone, at TOL."""
    model, at = big["model"], big["at"]
    cb = raw_batch(B_BIG, K_BIG, seed=77)
    ri = torch.arange(K_BIG, device="cuda")[None]

    def encode(d):
        with torch.no_grad():
            return model.encode_context(d["seq_idx"], d["xyz"], d["orientations"], d["backbone_dihedrals"], None, d["pairwise_dihedrals"],
                                        d["atom_mask"], d["chain_idx"], ri, d["generation_mask"], d["residue_mask"])

    res, pair = encode(cb)
    assert pair.shape == (B_BIG, K_BIG, K_BIG, DIMS["C"]) and pair.numel() > 2**31
    res, pair = res.index_select(0, at), pair.index_select(0, at)
    want_res, want_pair = encode(rows(cb, at))
    assert torch.isfinite(res).all() and torch.isfinite(pair).all()
    for i, r in enumerate(R):
        e_res, e_pair = rel(res[i], want_res[i]), rel(pair[i], want_pair[i])
        assert e_res < TOL and e_pair < TOL, (r, e_res, e_pair)
        for j in range(i):
            assert not torch.equal(want_pair[i], want_pair[j]), (r, R[j])  # the encoded patches differ from each other
    print(f"encode_context rows R: res {rel(res, want_res):.1e}, pair {rel(pair, want_pair):.1e}")


# ------------------------------------------------------------------ 6. one IPA layer's backward
def test_ipa_layer_backward_rows(big):
    """One InvariantPointAttentionLayer under autograd on the 520 patches with a seeded cotangent: y at TOL and d x, d e, d R, d t at
    GTOL at rows R against the six patches alone with the same cotangent rows.  d e is an 8.7 GB output written past element 2^31."""
    model, at, inp, small = big["model"], big["at"], big["big"], big["small"]
    layer = model.denoiser.ipa.layers[0]
    g = torch.Generator(device="cuda").manual_seed(6)
    cy = torch.randn(B_BIG, K_BIG, DIMS["D"], device="cuda", generator=g)

    def run(d, cot):
        lv = {k: d[k].detach().requires_grad_(True) for k in LAYER_IN}
        y = layer(*[lv[k] for k in LAYER_IN])
        (y * cot).sum().backward()
        return y.detach(), {k: lv[k].grad for k in LAYER_IN}

    y, grads = run(inp, cy)
    y, grads = y.index_select(0, at), at_rows(grads, at)
    want_y, want = run(small, cy.index_select(0, at))
    worst = {}
    for i, r in enumerate(R):
        e = rel(y[i], want_y[i])
        assert e < TOL, ("y", r, e)
        for k in LAYER_IN:
            assert torch.isfinite(grads[k][i]).all(), (k, r)
            e = rel(grads[k][i], want[k][i])
            worst[k] = max(worst.get(k, 0.0), e)
            assert e < GTOL, (k, r, e)
    print("layer backward rows R:", {k: f"{v:.1e}" for k, v in worst.items()})


# ------------------------------------------------------------------ 7. the training step at config 4's size
def test_training_step_is_the_sum_of_its_chunks(hip):
    """hotpath_train_losses at B = 128, K = 128, NL = 6 (the pair tape is 8.6 GB) whole, then in 16 chunks of 8 patches - the forms the
    oracle tests verify.  The losses are normalised by the batch's masked-residue count, so chunk c is weighted by count_c / count_all:
    the whole losses are the weighted sum of the chunks', d res_ctx and d pair_ctx rows are their chunk's rows, every parameter
    gradient is the sum of the chunks', all at GTOL of the tensor's maximum (the two sides differ in fp32 summation order only)."""
    dims, model = bench_model(100)
    B, K, step = 128, 128, 8
    inp = device_patches(B, K, dims, seed=704)
    gm, rm = inp["generation_mask"], torch.ones_like(inp["generation_mask"])
    t = 1 + (torch.arange(B) * 37) % 100
    torch.manual_seed(7)
    nz = model._add_noise(inp["seq_idx"], inp["translations"], inp["orientations"], gm, t.cuda())
    beta = model.sched["beta"][t].cuda()
    names = [n for n, _ in model.denoiser.named_parameters()]

    def run(sl, weight):
        rc = inp["res_context_emb"][sl].clone().requires_grad_(True)
        pc = inp["pair_context_emb"][sl].clone().requires_grad_(True)
        ls = model.hotpath_train_losses({k: v[sl] for k, v in nz.items()}, rc, pc, beta[sl], inp["orientations"][sl], gm[sl], rm[sl])
        ((ls[0] + ls[1] + ls[2]) * weight).backward()
        return torch.stack([l.detach() for l in ls]).double() * weight, rc.grad, pc.grad

    model.zero_grad(set_to_none=True)
    whole, d_rc, d_pc = run(slice(None), 1.0)
    whole_params = {n: p.grad.clone() for n, p in model.denoiser.named_parameters()}
    count = (gm & rm).sum(1).double()
    model.zero_grad(set_to_none=True)
    parts = torch.zeros(3, dtype=torch.float64, device="cuda")
    worst = {"res_ctx": 0.0, "pair_ctx": 0.0}
    scale_rc, scale_pc = d_rc.abs().max().double(), d_pc.abs().max().double()
    for lo in range(0, B, step):
        sl = slice(lo, lo + step)
        ls, g_rc, g_pc = run(sl, float(count[sl].sum() / count.sum()))  # p.grad accumulates over the chunks
        parts += ls
        worst["res_ctx"] = max(worst["res_ctx"], float((g_rc.double() - d_rc[sl].double()).abs().max() / scale_rc))
        worst["pair_ctx"] = max(worst["pair_ctx"], float((g_pc.double() - d_pc[sl].double()).abs().max() / scale_pc))
    loss_err = ((parts - whole).abs() / whole.abs()).tolist()
    print("whole against 16 chunks: losses", [f"{e:.1e}" for e in loss_err], {k: f"{v:.1e}" for k, v in worst.items()})
    assert torch.isfinite(whole).all() and max(loss_err) < GTOL, loss_err
    assert float(scale_rc) > 0 and float(scale_pc) > 0 and max(worst.values()) < GTOL, worst
    worst_param = ("", 0.0)
    for n, p in model.denoiser.named_parameters():
        e = rel(p.grad, whole_params[n])
        worst_param = max(worst_param, (n, e), key=lambda v: v[1])
        assert e < GTOL, (n, e)
    print("worst parameter gradient:", worst_param, "of", len(names))
    del inp, nz, d_rc, d_pc, whole_params
    model.zero_grad(set_to_none=True)
    torch.cuda.empty_cache()
