"""The workspace contract on the MI355X (include/diffab_hip.h, "Workspaces and tapes"): a result does not depend on what scratch memory
held before the call, and no kernel writes outside the bytes it was given.

Every hot-path entry works in memory it does not initialise itself (workspaces and tapes from _hip.workspace, outputs from torch.empty),
and the sampler, the module launch and the backward write ever less of it (skipped last-layer rows, the row plan, heads on live slabs,
one layout per backward buffer).  The bitwise tests of those paths run two variants back to back at one shape, where the allocator very
likely hands the second run the first run's block: a read of an unwritten row finds the right value there, or zeros on a fresh block.

Protocol (`four_runs` / `assert_contract`; the harness is tests/scratch_poison.py, pinned on the host by test_scratch_poison_host.py).
Each scenario computes its result plain and under each of the fills "zero", "ff" (NaN as a float, -1 as an integer, true as a mask
byte) and "random" (seeded random bytes).  Then
  (a) the guards around every workspace and tape are intact (checked when the fill's context exits);
  (b) every returned float tensor is finite wherever the plain run is;
  (c) paths stated to be deterministic: the four results are torch.equal (or equal bit for bit where the result holds NaN by
      definition, as metrics.backbone's dihedrals without a neighbour do);
  (c') paths the header documents as order-dependent in the last bits (parameter gradients and d pair_ctx: float atomics): each of the
      four is held to GTOL = 2e-4 max-rel against the float64 oracle, every element included.  Input gradients that no float atomic
      feeds are (c) when two plain runs agree bit for bit and (c') otherwise.
"keep" (scenario 6) hands each call the workspace the previous call of another shape, mask or mode left behind, as the caching
allocator does in production, and compares with the plain run of the same call.

Nothing returned is meant to be unspecified: the trajectory record and the steering record are defined in every slot (header,
diffab_sample_record), so everything `sample` and `score` return is compared whole; the ancestors table (T + 1 rows, torch.empty) is
filled with -1 by the call and written in the rows of the steered steps, which are the rows DiffAb.sample returns.  One row of one
gradient is never written by design and is asserted to be the caller's zero under every fill: row 0 of the chain embedding's gradient
(padding_idx = 0; the oracle's plain lookup gives it a gradient, so that row alone has no oracle value - test_encode_context).  No other
exclusion is made anywhere in this file.

The particle-steering entries (energy, resample, gather) are called on their own (scenario 8: caller-owned energy_out, ancestors_out,
ess_out and gather scratch) and run inside the composed sampler case; the patch, metrics, ensemble, similarity and refinement entries
are called once each on small inputs of this file (K = 128).  Graph capture is out of scope (the allocator hooks
are launches of their own).  The encode_context scenario borrows its cases, the oracle with its kink handling and the gradient check
from test_gpu_context_encoders.py, and the training-step scenarios their oracle cases from test_gpu_backward_paths.py and
test_gpu_generic_dims.py: the float64 sides are theirs, computed once per process.

`test_protocol_flags_a_stand_in_that_reads_its_scratch` proves the protocol can fail without running a faulty kernel: a torch-only
stand-in "entry" that sums a torch.empty buffer it wrote half of, and one that writes one byte behind its workspace.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import diffab_oracle as orc
from conftest import maxrel
from diffab_pytorch import _hip, metrics, patch, refine, synthetic as syn
from diffab_pytorch.guidance import SampleGuidance
from diffab_pytorch.steering import ParticleSteering, c_struct as steering_c_struct
from diffab_pytorch.temperature import SampleTemperature
from sampler_support import (ARGS, CTX, FLAG_IDS, FLAGS, GTOL, OUTS, PATCH_LENGTH_DIMS, STATE, TOL, assert_bitwise, check_params, f64, hip,  # noqa: F401
                             leaves, make_model, patches, sample, score, segment_mask, slab_mask, unit_model)
from scratch_poison import GUARD, GuardDamaged, poisoned, raw_bytes

pytestmark = pytest.mark.gpu
FILLS = ("zero", "ff", "random")
MODULE, PER_LAYER = _hip.FLAG_PERSISTENT_MODULE, _hip.FLAG_MULTI_LAUNCH


@pytest.fixture(autouse=True)
def _a_device_fault_ends_the_session():
    """A kernel that trusts a poisoned plan word may fault: nothing more is started on the device then."""
    yield
    try:
        torch.cuda.synchronize()
    except RuntimeError as err:
        pytest.exit(f"device error after a scratch-contract case, the session ends here: {err}", returncode=3)


# ====================================================================== the protocol
def flat(out, prefix=""):
    """A call's result as {name: tensor}: nested dicts ("trajectory", "steering", "noised") by dotted names, tuples by index."""
    if torch.is_tensor(out):
        return {prefix or "out": out}
    items = out.items() if isinstance(out, dict) else enumerate(out)
    res = {}
    for k, v in items:
        if v is not None:
            res.update(flat(v, f"{prefix}.{k}" if prefix else str(k)))
    return res


def four_runs(call, seed=0, workspace=True):
    """{"plain": ..., "zero": ..., "ff": ..., "random": ...} of call(); (a) is asserted as each fill's context exits.  workspace: the
    call takes one - then the "ff" run must have left some byte of a handed-out interior changed, or the poison never reached the library
    (an entry that stopped going through _hip.workspace would make every case here pass for nothing)."""
    runs = {"plain": flat(call())}
    for fill in FILLS:
        with poisoned(fill, seed=seed) as p:
            runs[fill] = flat(call())
            if fill == "ff":
                written = [bool((base[GUARD:GUARD + n] != 0xFF).any()) for base, n, _ in p.bases]
                assert any(written) == workspace and bool(p.bases) == workspace, ("workspaces handed out and written:", written)
    return runs


def same(a, b):
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if torch.equal(a, b):
        return True
    if a.is_floating_point() and a.element_size() == 4:  # NaN by definition: the same NaN in the same place
        return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))
    return False


def assert_contract(runs, what, close=None):
    """(b) and (c) over every tensor of the runs; the names in `close` = {name: check(tensor, run)} go by (c') instead."""
    plain = runs["plain"]
    close = close or {}
    for fill, got in runs.items():
        assert set(got) == set(plain), (what, fill, set(got) ^ set(plain))
        for k, want in plain.items():
            if want.is_floating_point():
                bad = torch.isfinite(want) & ~torch.isfinite(got[k])
                assert not bool(bad.any()), (what, fill, k, "not finite where the plain run is", int(bad.sum()), bad.nonzero()[:4].tolist())
            if k in close:
                close[k](got[k], (what, fill, k))
            else:
                assert same(got[k], want), (what, fill, k, "elements that differ:", int((got[k] != want).sum()),
                                            (got[k] != want).nonzero()[:4].tolist())


def within_gtol(ref):
    def check(got, tag):
        r = maxrel(got, ref)
        assert r < GTOL, (tag, r)
    return check


# ====================================================================== 0. the protocol can fail
def test_protocol_flags_a_stand_in_that_reads_its_scratch(hip):
    """Torch only, no call into the library: an "entry" that writes half of a torch.empty buffer and sums all of it, one that leaves the
    tail of its output unwritten, and one that writes a byte behind its workspace."""
    x = torch.arange(64.0, device="cuda").reshape(2, 32)
    names = (_hip.workspace, torch.empty, torch.empty_like)

    def reads_unwritten():
        scratch = torch.empty(2, 64, device="cuda")
        scratch[:, :32] = x
        return {"y": scratch.sum(1)}

    def output_not_fully_written():
        y = torch.empty_like(x)
        y[:, :31] = x[:, :31]
        return {"y": y}

    def honest():
        scratch = torch.empty(2, 64, device="cuda")
        scratch[:, :32] = x
        scratch[:, 32:] = 1.0
        ws = _hip.workspace(1000)
        ws[:] = 3
        return {"y": scratch.sum(1) + ws.sum()}

    assert_contract(four_runs(honest), "honest stand-in")
    for entry in (reads_unwritten, output_not_fully_written):
        runs = four_runs(entry, workspace=False)
        with pytest.raises(AssertionError, match="not finite where the plain run is|elements that differ"):
            assert_contract(runs, entry.__name__)

    for offset in (1000, -1):
        with pytest.raises(GuardDamaged, match=f"1000 bytes.*offset {offset} "):
            with poisoned("random"):
                ws = _hip.workspace(1000)
                raw_bytes(ws)[GUARD + offset] = 0  # inside the helper's base buffer, outside the 1000 bytes handed out
    assert all(a is b for a, b in zip((_hip.workspace, torch.empty, torch.empty_like), names)), "the three names are back"


# ====================================================================== 1. denoiser forward
def denoise(model, inp, beta, flags):
    with torch.no_grad():
        return model.denoiser(*[inp[k] for k in ARGS], beta, inp["generation_mask"], None, return_logits=True, flags=flags)


DENOISE_SHAPES = [("unit_b3_k24", "unit", 3, 24), ("bench_k64", "bench", 2, 64), ("bench_k128", "bench", 2, 128), ("bench_k192", "bench", 2, 192),
                  ("bench_k256", "bench", 1, 256)]


@pytest.fixture(scope="module")
def denoise_models(hip):
    dims, model, sd = unit_model(NL=2, seed=17)
    return {"unit": (dims, model, sd), "bench": (dict(PATCH_LENGTH_DIMS), make_model(dict(PATCH_LENGTH_DIMS), 23), None)}


@pytest.mark.parametrize("name,which,B,K", DENOISE_SHAPES, ids=[s[0] for s in DENOISE_SHAPES])
def test_denoiser_forward(denoise_models, name, which, B, K):
    """All five outputs under each flag selection.  At the unit dims the "ff" run is also held to TOL against the float64 oracle."""
    dims, model, sd = denoise_models[which]
    inp = patches(B, K, dims, seed=300 + K)
    beta = torch.tensor([0.03, 0.7, 0.25])[:B].cuda()
    for flags, fid in zip(FLAGS, FLAG_IDS):
        runs = four_runs(lambda: denoise(model, inp, beta, flags), seed=K)
        assert set(runs["plain"]) == set(OUTS)
        assert_contract(runs, (name, fid))
        if which == "unit" and flags == 0:
            want = orc.denoiser(sd, inp["seq_idx"].cpu(), *[f64(inp[k]) for k in ARGS[1:]], beta.cpu().double(), dims["NL"], dims["H"])
            for k in OUTS:
                assert maxrel(runs["ff"][k], want[k]) < TOL, (name, k, maxrel(runs["ff"][k], want[k]))


# ====================================================================== 2. one IPA layer
@pytest.mark.parametrize("pair_bias", [True, False], ids=["pair_bias", "no_pair_bias"])
def test_ipa_layer_forward_and_backward(hip, pair_bias):
    """Bench dims, B = 2, K = 128.  Inference forward: (c).  Taped forward + backward from a random d y (the tape is poisoned before the
    forward writes it): y (c); d x, d R, d t (c) if two plain runs agree, else (c'); d e and the parameters (c')."""
    from diffab_pytorch.diffab_pytorch import InvariantPointAttentionLayer

    d, B, K = dict(syn.BENCH_DIMS), 2, 128
    torch.manual_seed(71)
    layer = InvariantPointAttentionLayer(d["D"], d["C"], d["DS"], d["PQ"], d["PV"], d["H"], use_pair_bias=pair_bias)
    with torch.no_grad():
        layer.gamma.copy_(torch.rand(d["H"]) + 0.2)
    layer = layer.cuda()
    host = syn.patches(B, K, d, seed=571, coord_sigma=6.0)
    names = ("res_context_emb", "pair_context_emb", "orientations", "translations")
    grads_of = [k for k in names if pair_bias or k != "pair_context_emb"]
    cy = torch.randn(B, K, d["D"], generator=torch.Generator().manual_seed(5))

    def inference():
        with torch.no_grad():
            return {"y": layer(*[host[k].cuda() for k in names])}

    assert_contract(four_runs(inference), ("layer inference", pair_bias))

    def taped():
        layer.zero_grad(set_to_none=True)
        lv = {k: host[k].cuda().requires_grad_(k in grads_of) for k in names}
        y = layer(*[lv[k] for k in names])
        (y * cy.cuda()).sum().backward()
        out = {"y": y.detach()}
        out.update({"d_" + k: lv[k].grad for k in grads_of})
        out.update({"p_" + n: p.grad.clone() for n, p in layer.named_parameters()})
        return out

    lo = {k: f64(host[k]).requires_grad_(k in grads_of) for k in names}
    sdo = leaves({n: p for n, p in layer.named_parameters()}, "L.")
    want = orc.ipa_layer(*[lo[k] for k in names], sdo, "L.", d["H"], use_pair_bias=pair_bias)
    (want * cy.double()).sum().backward()
    runs = four_runs(taped)
    again = flat(taped())
    close = {"p_" + n: within_gtol(sdo["L." + n].grad) for n, _ in layer.named_parameters()}
    for k in grads_of:
        if k == "pair_context_emb" or not torch.equal(again["d_" + k], runs["plain"]["d_" + k]):
            close["d_" + k] = within_gtol(lo[k].grad)
    print("layer backward, by the oracle bar:", sorted(close))
    assert maxrel(runs["plain"]["y"], want.detach()) < TOL
    assert_contract(runs, ("layer taped", pair_bias), close)


# ====================================================================== 3. training step
@pytest.fixture(scope="module")
def train_cases(hip):
    from test_gpu_backward_paths import losses_case  # noqa: the float64 side of the same (K, B, NL, seed) cases, computed once per process

    return losses_case


@pytest.mark.parametrize("frozen", [False, True], ids=["d_pair_ctx", "frozen_pair"])
@pytest.mark.parametrize("K,seed", [(64, 17), (128, 14)])
def test_training_step(train_cases, K, seed, frozen):
    """hotpath_train_losses + backward (what _shared_step runs under grad), NL = 2, B = 2.  The three losses (c); d res_ctx (c) if two
    plain runs agree, else (c'); d pair_ctx and every parameter gradient (c')."""
    runs, close, _ = training_runs(train_cases, K, seed, frozen, FILLS)
    assert_contract(runs, ("training step", K, frozen), close)


def training_call(model, c, frozen):
    inp = {k: v.cuda() for k, v in c["inp"].items()}
    nz = {k: v.cuda() for k, v in c["nz"].items()}
    beta = c["beta"].cuda()

    def call():
        model.zero_grad(set_to_none=True)
        rc = inp["res_context_emb"].clone().requires_grad_(True)
        pc = inp["pair_context_emb"].clone().requires_grad_(not frozen)
        ls = model.hotpath_train_losses(nz, rc, pc, beta, inp["orientations"], inp["generation_mask"], inp["residue_mask"])
        (ls[0] + ls[1] + ls[2]).backward()
        assert frozen == (pc.grad is None)
        out = {"losses": torch.stack([v.detach() for v in ls]), "d_res_ctx": rc.grad}
        if not frozen:
            out["d_pair_ctx"] = pc.grad
        out.update({"p_" + n: p.grad.clone() for n, p in model.denoiser.named_parameters()})
        return out
    return call


def training_runs(losses_case, K, seed, frozen, fills):
    from diffab_pytorch import DiffAb

    NL, B = 2, 2
    c = losses_case(K, B, NL, seed)
    assert c["margin"] > 5e-7, (c["margin"], "inputs on a ReLU kink: pick another weight seed")
    d = dict(syn.BENCH_DIMS, NL=NL)
    torch.manual_seed(0)
    model = DiffAb(d["D"], d["C"], d["NL"], d["DS"], d["PQ"], d["PV"], d["H"]).cuda()
    model.denoiser.load_state_dict(c["sd"])
    call = training_call(model, c, frozen)
    runs = {"plain": flat(call())}
    for fill in fills:
        with poisoned(fill, seed=K):
            runs[fill] = flat(call())
    again = flat(call())
    close = {"p_" + n: within_gtol(c["sdo"]["denoiser." + n].grad) for n, _ in model.denoiser.named_parameters()}
    if not frozen:
        close["d_pair_ctx"] = within_gtol(c["d_pc"])
    if not torch.equal(again["d_res_ctx"], runs["plain"]["d_res_ctx"]):
        close["d_res_ctx"] = within_gtol(c["d_rc"])
    assert maxrel(runs["plain"]["d_res_ctx"], c["d_rc"]) < GTOL
    print(f"training step K={K} frozen={frozen}: d res_ctx by", "the oracle bar" if "d_res_ctx" in close else "bits")
    return runs, close, (model, c)


@pytest.mark.parametrize("gid", ["odd", "af2"])
def test_training_step_any_dims(hip, gid):
    """The same step on the any-dims kernels (B = 3, K = 37 with H = 3, PQ != PV; AlphaFold 2's head shape at K = 128): the generic
    attention backward, per-projection linear_bwd and the VALU gemm fallbacks carve the workspace their own way."""
    from test_gpu_generic_dims import diffab, geom, losses_case  # noqa: the float64 side of the any-dims cases

    c = losses_case(gid)
    assert c["margin"] > 5e-7
    model = diffab(geom(gid)[2], c["sd"])
    call = training_call(model, c, frozen=False)
    runs = four_runs(call, seed=3)
    again = flat(call())
    close = {"p_" + n: within_gtol(c["sdo"]["denoiser." + n].grad) for n, _ in model.denoiser.named_parameters()}
    close["d_pair_ctx"] = within_gtol(c["d_pc"])
    if not torch.equal(again["d_res_ctx"], runs["plain"]["d_res_ctx"]):
        close["d_res_ctx"] = within_gtol(c["d_rc"])
    assert maxrel(runs["plain"]["d_res_ctx"], c["d_rc"]) < GTOL
    assert_contract(runs, ("training step", gid), close)


def test_denoiser_cotangent_backward(hip):
    """Denoiser under autograd with random cotangents at K = 64, NL = 2, B = 2 (d x_t and d O_t exist on this path only): the outputs
    (c); d x_t, d O_t, d res_ctx (c) if two plain runs agree, else (c'); d pair_ctx and the parameters (c')."""
    from diffab_pytorch.diffab_pytorch import Denoiser
    from test_gpu_backward_paths import cotangent_case

    K, B, NL, seed = 64, 2, 2, 21
    c = cotangent_case(K, B, NL, seed)
    assert c["margin"] > 5e-7
    d = dict(syn.BENCH_DIMS, NL=NL)
    den = Denoiser(d["D"], d["C"], d["NL"], d["DS"], d["PQ"], d["PV"], d["H"], 21)
    den.load_state_dict(c["sd"], strict=True)
    den = den.cuda().train()
    inp = c["inp"]

    def call():
        den.zero_grad(set_to_none=True)
        lv = {k: inp[k].cuda().requires_grad_(True) for k in ARGS[1:]}
        out = den(inp["seq_idx"].cuda(), lv["translations"], lv["orientations"], lv["res_context_emb"], lv["pair_context_emb"], c["beta"].cuda(),
                  None, None)
        sum((out[k] * v.cuda()).sum() for k, v in c["cot"].items()).backward()
        res = {k: v.detach() for k, v in out.items()}
        res.update({"d_" + k: lv[k].grad for k in ARGS[1:]})
        res.update({"p_" + n: p.grad.clone() for n, p in den.named_parameters()})
        return res

    runs = four_runs(call)
    again = flat(call())
    close = {"p_" + n: within_gtol(c["sdo"]["denoiser." + n].grad) for n, _ in den.named_parameters()}
    for k in ARGS[1:]:
        if k == "pair_context_emb" or not torch.equal(again["d_" + k], runs["plain"]["d_" + k]):
            close["d_" + k] = within_gtol(c["grads"][k])
    print("cotangent backward, by the oracle bar:", sorted(k for k in close if k.startswith("d_")))
    assert_contract(runs, "denoiser cotangents K = 64", close)


# ====================================================================== 4. encode_context
@pytest.mark.parametrize("name", ["fused_A15", "unfused_k64"])
def test_encode_context(hip, name):
    """Residue and pair embeddings forward and backward, B = 2: K = 128 (the taped pair path) and K = 64 (diffab_pair_embedding_tape_bytes
    = 0: chunked recompute).  Forward (c); the 23 parameter gradients (c') by the encoders' own check_grads.  That check leaves row 0 of
    the chain embedding's gradient out of the oracle comparison (padding_idx = 0: the kernel never writes the row, the oracle's plain
    lookup does): here the row must be exactly the caller's zero under every fill, whether chain 0 occurs or not."""
    from test_gpu_context_encoders import CASES, DIMS, case_data, check_grads, model_for, run_hip

    K, A, md, _ = CASES[name]
    cd = _hip.CtxDims(2, K, A, DIMS["D"], DIMS["C"], md)
    taped = hip.diffab_pair_embedding_tape_bytes(C.byref(cd)) > 0
    assert taped == (name == "fused_A15"), (name, "the case must reach the path it stands for")
    seed, (cb, G1, G2, want) = case_data(name, True, True)
    model, _ = model_for(A, md, seed)

    def call():
        res, pair, grads = run_hip(hip, model, cb, True, True, G1, G2)
        return {"res": res, "pair": pair, "grads": grads}

    runs = four_runs(call)
    chain0 = bool((cb["chain_idx"] == 0).any())
    for fill, got in runs.items():  # (c'): check_grads is the existing per-parameter GTOL bar of the encoders' own test
        check_grads((name, fill), {k[len("grads."):]: v for k, v in got.items() if k.startswith("grads.")}, want[2], chain0)
        row0 = got["grads.residue_context_embedding.chain_embedding.weight"][0]
        assert not bool(row0.any()), (name, fill, "the padding row of the chain embedding's gradient was written", row0.abs().max())
    close = {k: (lambda got, tag: None) for k in runs["plain"] if k.startswith("grads.")}
    assert_contract(runs, ("encode_context", name), close)  # res, pair: (c); (b) for everything


# ====================================================================== 5. sampler
STEPS = dict(t_start=60, t_stop=54)  # six reverse steps from diffab_sample_init


@pytest.fixture(scope="module")
def sampler_models(hip):
    out = {}
    for NL in (2, 3):
        dims = dict(syn.BENCH_DIMS, NL=NL)
        out[NL] = (dims, make_model(dims, 41 + NL), patches(8, 128, dims, seed=240 + NL))
    return out


SAMPLER_FORMS = [("default", {}), ("module", dict(flags=MODULE)), ("module_all_rows", dict(flags=MODULE, skip_unused_rows=False)),
                 ("per_layer", dict(flags=PER_LAYER))]


def with_mask(inp, gm):
    inp = dict(inp, generation_mask=gm.cuda())
    if "residue_mask" in inp:
        inp["residue_mask"] = inp["residue_mask"] | gm.cuda()
    return inp


@pytest.mark.parametrize("NL", [2, 3])
@pytest.mark.parametrize("mask", ["one_slab", "slabs_0_and_3", "row_127", "none", "mixed"])
def test_sampler_masks_and_launch_forms(sampler_models, NL, mask):
    """Six reverse steps at B = 8, K = 128 under each launch form: seq, x, O after the loop, (c); the forms agree bitwise as well."""
    dims, model, inp8 = sampler_models[NL]
    inp = with_mask(inp8, slab_mask(mask, 8, 128, inp8["generation_mask"].cpu()))
    first = None
    for form, extra in SAMPLER_FORMS:
        runs = four_runs(lambda: sample(model, inp, seed=13, **STEPS, **extra), seed=NL)
        assert_contract(runs, (NL, mask, form))
        first = runs["plain"] if first is None else first
        assert_bitwise(runs["plain"], first, (NL, mask, form, "against the default form"))


def test_sampler_shared_contexts(sampler_models):
    """num_samples = 2 on four contexts (n_ctx < B): the shared-context workspace."""
    dims, model, inp8 = sampler_models[3]
    inp = {k: v[:4] for k, v in inp8.items()}
    for gm in (inp["generation_mask"].cpu(), segment_mask(4, 128, [(31, 33)])):
        for form, extra in SAMPLER_FORMS[:2]:
            runs = four_runs(lambda: sample(model, with_mask(inp, gm), seed=13, num_samples=2, **STEPS, **extra))
            assert runs["plain"]["translations"].shape[0] == 8
            assert_contract(runs, ("shared contexts", form))


@pytest.mark.parametrize("extra", [dict(mode="fixed_backbone"), dict(mode="structure"), dict(optimize_from=60, t_stop=54)],
                         ids=["fixed_backbone", "structure", "optimize_from"])
def test_sampler_design_modes(sampler_models, extra):
    """The KEEP bits (the update kernel never writes x and O, or seq) and the forward-noised start, module and per-layer forms."""
    dims, model, inp8 = sampler_models[2]
    inp = with_mask(inp8, slab_mask("slabs_0_and_3", 8, 128, inp8["generation_mask"].cpu()))
    kw = dict(seed=13, **(extra if "optimize_from" in extra else dict(STEPS, **extra)))
    for form, flags in (("module", MODULE), ("per_layer", PER_LAYER)):
        assert_contract(four_runs(lambda: sample(model, inp, flags=flags, **kw)), (sorted(extra), form))


def composed_kw(rows, K, N):
    """Guidance, steering, temperature, allowed_aa, steps= and trajectory= in one call (as tests/test_gpu_reverse_step_composed.py)."""
    rep = lambda v: torch.tensor((v * rows)[:rows], dtype=torch.float32)
    allowed = torch.rand(rows // N, K, 21, generator=torch.Generator().manual_seed(K)) < 0.5
    allowed[..., 2] = True
    return dict(seed=23, first_patch=3, t_start=60, t_stop=19, steps=[60, 59, 57, 20], init=False, num_samples=N, trajectory=True,
                trajectory_predictions=True, temperature=SampleTemperature(rep([1.5, 0.0, 1.0, 0.5]), rep([0.0, 0.3, 0.6, 1.0]),
                                                                           rep([0.5, 1.0, 0.0, 2.0])),
                allowed_aa=allowed, guidance=SampleGuidance(clash=2.0, bond=1.0, max_shift=0.5),
                steering=ParticleSteering(strength=0.5, clash=1.3, bond=0.7, t_min=20, t_max=59, ess_threshold=2.0))


@pytest.mark.parametrize("form", ["module", "per_layer"])
def test_sampler_options_combined(hip, form):
    """Everything sample returns, the trajectory record (predictions included) and the steering record among it, (c)."""
    dims = dict(PATCH_LENGTH_DIMS)
    model = make_model(dims, 29)
    P, N, K = 2, 5, 128
    gm = torch.zeros(1, K, dtype=torch.bool)
    gm[0, 3:16] = True
    gm[0, K // 2 + 5:K // 2 + 16] = True
    inp = patches(P, K, dims, seed=K, chains=True, generation_mask=gm.expand(P, K).clone())
    kw = composed_kw(P * N, K, N)
    runs = four_runs(lambda: sample(model, inp, flags=MODULE if form == "module" else PER_LAYER, **kw))
    assert {"trajectory.seq_probs", "trajectory.pred_translations", "steering.ancestors", "steering.log_weight"} <= set(runs["plain"])
    assert runs["plain"]["steering.t"].numel() >= 2
    moved = int((runs["plain"]["steering.ancestors"].cpu() != torch.arange(P * N)).sum())
    assert moved > 0, "some ancestor must differ from the identity for the gather to have moved a row"
    assert_contract(runs, ("options combined", form))


@pytest.mark.parametrize("K", [64, 173, 192, 256])
def test_sampler_other_patch_lengths(denoise_models, K):
    """B = 2 at K = 256 (the module launch's other length), and at the lengths whose loop carves other buffers: 64, 192 (per-layer
    launches) and 173 (no multiple of 64: the any-dims kernels)."""
    dims, model, _ = denoise_models["bench"]
    inp = patches(2, K, dims, seed=K)
    for form, extra in SAMPLER_FORMS[:2] if K == 256 else SAMPLER_FORMS[:1]:
        assert_contract(four_runs(lambda: sample(model, inp, seed=13, **STEPS, **extra), seed=K), (K, form))


# ====================================================================== 6. "keep": the leftover of one call handed to the next
def test_keep_across_masks_and_shapes(sampler_models, denoise_models):
    """Within one poisoned("keep"): the sampler with the `all` mask, then `one_slab`, then `none`, in both launch forms; denoise at
    K = 192, then K = 128 (served from the front of the K = 192 workspace).  Each result is bitwise the plain run of the same call."""
    dims, model, inp8 = sampler_models[3]
    gms = {name: slab_mask(name, 8, 128, inp8["generation_mask"].cpu()) for name in ("all", "one_slab", "none")}
    ddims, dmodel, _ = denoise_models["bench"]
    dinp = {K: patches(2, K, ddims, seed=300 + K) for K in (192, 128)}
    beta = torch.tensor([0.03, 0.7]).cuda()
    for form, extra in SAMPLER_FORMS[1:4:2]:  # module, per_layer
        calls = [((form, name), (lambda gm=gm: sample(model, with_mask(inp8, gm), seed=13, **STEPS, **extra))) for name, gm in gms.items()]
        calls += [(("denoise", K), (lambda K=K: denoise(dmodel, dinp[K], beta, 0))) for K in (192, 128)]
        plain = [flat(call()) for _, call in calls]
        with poisoned("keep") as p:
            for (what, call), want in zip(calls, plain):
                got = flat(call())
                assert_contract({"plain": want, "keep": got}, what)
            assert len(p.bases) <= 2, [b[1] for b in p.bases]  # the three sampler calls share one buffer, the two denoise calls one


def test_keep_across_batch_sizes_and_depths(sampler_models):
    """One kept workspace serves B = 8 at NL = 3, then the first three patches alone (every carved buffer starts elsewhere), then the
    NL = 2 model (the module's result leaves in the other activation buffer), then K = 128 rows of the NL = 3 model again."""
    (_, m3, inp3), (_, m2, inp2) = sampler_models[3], sampler_models[2]
    sub = lambda inp, n: {k: v[:n] for k, v in inp.items()}
    calls = [("NL3 B8", lambda: sample(m3, inp3, seed=13, flags=MODULE, **STEPS)),
             ("NL3 B3", lambda: sample(m3, sub(inp3, 3), seed=13, flags=MODULE, **STEPS)),
             ("NL2 B8", lambda: sample(m2, with_mask(inp2, slab_mask("one_slab", 8, 128, None)), seed=13, flags=MODULE, **STEPS)),
             ("NL2 B5 per layer", lambda: sample(m2, sub(inp2, 5), seed=13, flags=PER_LAYER, **STEPS)),
             ("NL3 B8 again", lambda: sample(m3, with_mask(inp3, slab_mask("row_127", 8, 128, None)), seed=13, flags=MODULE, **STEPS))]
    plain = [flat(call()) for _, call in calls]
    with poisoned("keep") as p:
        for (what, call), want in zip(calls, plain):
            assert_contract({"plain": want, "keep": flat(call())}, what)
        assert len(p.bases) <= 2, [b[1] for b in p.bases]  # (two only if NL = 2 asks for more bytes than NL = 3)


@pytest.mark.parametrize("K,seed", [(64, 17), (128, 14)])
def test_keep_training_step_then_frozen_pair(train_cases, K, seed):
    """d pair_ctx wanted, then the frozen-pair form on the same tape and workspace (the backward's buffers have one layout per call:
    the second call's layout differs from the first's)."""
    from diffab_pytorch import DiffAb

    c = train_cases(K, 2, 2, seed)
    d = dict(syn.BENCH_DIMS, NL=2)
    torch.manual_seed(0)
    model = DiffAb(d["D"], d["C"], d["NL"], d["DS"], d["PQ"], d["PV"], d["H"]).cuda()
    model.denoiser.load_state_dict(c["sd"])
    calls = [training_call(model, c, frozen) for frozen in (False, True, False)]
    plain = [flat(call()) for call in calls]
    again = flat(calls[0]())
    with poisoned("keep") as p:
        for i, (call, want) in enumerate(zip(calls, plain)):
            got = flat(call())
            close = {"p_" + n: within_gtol(c["sdo"]["denoiser." + n].grad) for n, _ in model.denoiser.named_parameters()}
            close["d_pair_ctx"] = within_gtol(c["d_pc"])
            if not torch.equal(again["d_res_ctx"], plain[0]["d_res_ctx"]):
                close["d_res_ctx"] = within_gtol(c["d_rc"])
            assert_contract({"plain": want, "keep": got}, ("training step under keep", K, i), {k: v for k, v in close.items() if k in want})
        assert len(p.bases) == 2, [b[1] for b in p.bases]  # one tape, one workspace


# ====================================================================== 7. score
def test_score(hip):
    """R = 2 designs of one shared context, n_t = 2, M = 2, K = 128, per_residue and return_noised on: everything returned, (c)."""
    dims = dict(PATCH_LENGTH_DIMS)
    model = make_model(dims, 23)
    ctx = patches(1, 128, dims, seed=51)
    ci = torch.zeros(2, dtype=torch.long)
    inp = {k: ctx[k][ci.cuda()].clone() for k in STATE}
    inp["translations"][1] += 0.5
    for flags in (0, PER_LAYER):
        runs = four_runs(lambda: model.score(inp["seq_idx"], inp["translations"], inp["orientations"], generation_mask=inp["generation_mask"],
                                             res_context_emb=ctx["res_context_emb"], pair_context_emb=ctx["pair_context_emb"],
                                             context_index=ci, t=[7, 60], num_draws=2, seed=12, per_residue=True, return_noised=True,
                                             flags=flags))
        assert {"per_step", "per_residue", "noised.translations_t", "noised.seq_idx_t"} <= set(runs["plain"])
        assert_contract(runs, ("score", flags))


# ====================================================================== 8. post-processing entries
@pytest.fixture(scope="module")
def designs(hip):
    """G = 2 patches of K = 128 with N = 3 designs each: the native frames, the generated residues displaced and retyped per design."""
    G, N, K = 2, 3, 128
    nat = patches(G, K, dict(syn.BENCH_DIMS), seed=88, chains=True, collapse=False)
    g = torch.Generator().manual_seed(8)
    rows = torch.arange(G).repeat_interleave(N).cuda()
    gm = nat["generation_mask"]
    des = {k: nat[k][rows].clone() for k in ("seq_idx", "translations", "orientations")}
    des["translations"] += (0.7 * torch.randn(G * N, K, 3, generator=g)).cuda() * gm[rows][..., None]
    des["seq_idx"] = torch.where(gm[rows], torch.randint(0, 20, (G * N, K), generator=g).cuda(), des["seq_idx"])
    other = patches(G * N, K, dict(syn.BENCH_DIMS), seed=89)["orientations"]
    des["orientations"] = torch.where(gm[rows][..., None, None], other, des["orientations"])
    return G, N, K, nat, des


POST = {
    "pairwise": lambda G, N, K, nat, des: metrics.pairwise(des, nat["generation_mask"], residue_mask=nat["residue_mask"], group_size=N,
                                                           atoms="backbone", aligned=True),
    "pick_m": lambda G, N, K, nat, des: metrics.select_diverse(
        metrics.pairwise(des, nat["generation_mask"], group_size=N)["rmsd"], 2),
    "contacts": lambda G, N, K, nat, des: metrics.contacts(des, nat["generation_mask"], antigen_mask=nat["chain_idx"] == 1,
                                                           chain_idx=nat["chain_idx"], residue_idx=nat["residue_idx"],
                                                           residue_mask=nat["residue_mask"], group_size=N),
    "backbone_filters": lambda G, N, K, nat, des: metrics.backbone(des, nat["generation_mask"], chain_idx=nat["chain_idx"],
                                                                   residue_idx=nat["residue_idx"], residue_mask=nat["residue_mask"], group_size=N),
    "similarity": lambda G, N, K, nat, des: metrics.similarity(des, nat, nat["generation_mask"], group_size=N, atoms="backbone",
                                                               residue_mask=nat["residue_mask"], antigen_mask=nat["chain_idx"] == 1,
                                                               chain_idx=nat["chain_idx"], residue_idx=nat["residue_idx"]),
    "ensemble": lambda G, N, K, nat, des: metrics.ensemble(des, nat["generation_mask"], group_size=N, residue_mask=nat["residue_mask"]),
    "evaluate": lambda G, N, K, nat, des: metrics.evaluate(des, nat, nat["generation_mask"], residue_mask=nat["residue_mask"], group_size=N),
    "refine": lambda G, N, K, nat, des: refine.backbone(des, nat["generation_mask"], chain_idx=nat["chain_idx"], residue_idx=nat["residue_idx"],
                                                        residue_mask=nat["residue_mask"], group_size=N, options=refine.Refinement(iterations=5)),
}


@pytest.mark.parametrize("entry", sorted(POST))
def test_post_processing_entry(designs, entry):
    assert_contract(four_runs(lambda: POST[entry](*designs), workspace=entry not in ("similarity", "evaluate")), entry)


# ---- the three steering entries on their own: caller-owned outputs and scratch (inside sample() ess_out is NULL, the gather runs per
# group with the loop's own scratch and the uniforms are Philox's)
@pytest.mark.parametrize("N", [3, 65, 257])
def test_steer_resample_entry(hip, N):
    """G = 64 groups of N rows, wide log-weights with a group of -inf and one NaN, explicit uniforms, always resampling and at threshold
    0.5: logw and u_prev (read and written), ancestors_out and ess_out (torch.empty: every element must be written), (c)."""
    G = 64
    rng = np.random.default_rng(1000 + N)
    lw = rng.normal(0.0, 5.0, (G, N)).astype(np.float32)
    lw[2] = -np.inf
    lw[3, N // 2] = np.nan
    up, U = (rng.uniform(0.0, 8.0, (G, N)).astype(np.float32) for _ in range(2))
    u = rng.random(G).astype(np.float32)
    host = [torch.tensor(v.reshape(-1)) for v in (lw, up, U, u)]
    for thr in (2.0, 0.5):
        def call():
            d = [v.cuda() for v in host]
            anc = torch.empty(G * N, dtype=torch.int32, device="cuda")
            ess = torch.empty(G, dtype=torch.float64, device="cuda")
            _hip.check(hip.diffab_steer_resample(_hip.ptr(d[0]), _hip.ptr(d[1]), _hip.ptr(d[2]), _hip.ptr(d[3]), G, N, 0.75, thr, _hip.ptr(anc),
                                                 _hip.ptr(ess), _hip.stream_ptr()), "diffab_steer_resample")
            return {"logw": d[0], "u_prev": d[1], "ancestors": anc, "ess": ess}

        runs = four_runs(call, seed=N, workspace=False)
        anc = runs["plain"]["ancestors"].view(G, N)
        assert int(anc.min()) >= 0 and int(anc.max()) < N
        if thr == 2.0 and N > 1:
            assert bool((anc != torch.arange(N, device="cuda")).any()), "some group must resample for this case to say anything"
        assert_contract(runs, ("steer_resample", N, thr))


@pytest.mark.parametrize("K", [5, 64, 128])
def test_steer_gather_entry(hip, K):
    """One group of R = 12 rows with a ragged mask, under a cycle, two cycles and a many-to-one map (no permutation in place: the rows
    being replaced go through the scratch).  The scratch is R K 56 bytes from _hip.workspace, so it is poisoned AND guarded; seq, x, O
    (c), and equal to plain indexing."""
    R = 12
    g = torch.Generator().manual_seed(K)
    seq = torch.randint(0, 21, (R, K), generator=g)
    x, O = torch.randn(R, K, 3, generator=g), torch.randn(R, K, 3, 3, generator=g)
    gm = torch.rand(R, K, generator=g) < 0.6
    gm[1] = False
    maps = {"cycle": (torch.arange(R) + 1) % R, "two cycles": torch.tensor([1, 2, 0, 4, 5, 3, 6, 7, 9, 8, 11, 10]),
            "one ancestor": torch.full((R,), 7)}
    for name, a in maps.items():
        def call():
            d = [v.clone().cuda() for v in (seq, x, O)]
            scratch = _hip.workspace(R * K * 56)
            gm_d, a_d = gm.cuda(), a.to(torch.int32).cuda()
            _hip.check(hip.diffab_steer_gather(_hip.ptr(d[0]), _hip.ptr(d[1]), _hip.ptr(d[2]), _hip.ptr(gm_d), _hip.ptr(a_d), R, K,
                                               _hip.ptr(scratch), _hip.stream_ptr()), "diffab_steer_gather")
            return {"seq": d[0], "x": d[1], "O": d[2]}

        runs = four_runs(call, seed=K)
        for k, old in (("seq", seq), ("x", x), ("O", O)):
            m = gm.reshape(R, K, *([1] * (old.dim() - 2)))
            assert torch.equal(runs["plain"][k].cpu(), torch.where(m, old[a], old)), (name, k)
        assert_contract(runs, ("steer_gather", K, name))


@pytest.mark.parametrize("K", [5, 64, 128])
def test_steer_energy_entry(denoise_models, K):
    """B = 3 rows of two chains with collapsed generated residues at t = 30: energy_out (torch.empty, one value per row), (c)."""
    dims, model, _ = denoise_models["unit"]
    B, t = 3, 30
    gen = torch.zeros(B, K, dtype=torch.bool)
    gen[:, K // 4:K // 4 + max(2, K // 3)] = True
    inp = patches(B, K, dims, seed=K, chains=True, generation_mask=gen)
    eps = torch.randn(B, K, 3, generator=torch.Generator().manual_seed(K)).cuda()
    tabs = [inp[k].to(torch.int32).contiguous() for k in ("chain_idx", "residue_idx")] + [inp["residue_mask"].contiguous()]
    ss = steering_c_struct(ParticleSteering(clash=1.3, bond=0.7, clash_distance=4.0, bond_length=3.8), 0, 1, *tabs, None, None, None, None, None)
    sd = model._sched_on_device()
    x, gm = inp["translations"].contiguous(), inp["generation_mask"].contiguous()

    def call():
        out = torch.empty(B, device="cuda")
        _hip.check(_hip.lib().diffab_steer_energy(_hip.ptr(x), _hip.ptr(eps), _hip.ptr(gm), C.byref(sd.struct), t, C.byref(ss), B, K,
                                                  _hip.ptr(out), _hip.stream_ptr()), "diffab_steer_energy")
        return {"energy": out}

    runs = four_runs(call, seed=K, workspace=False)
    assert bool((runs["plain"]["energy"] > 0).all()), runs["plain"]["energy"]
    assert_contract(runs, ("steer_energy", K))


def test_patch_select_gather_paste(hip):
    """B = 2 complexes of N = 300 residues, k = 128: the patch index, every gathered field and the pasted designs, (c)."""
    B, N = 2, 300
    cb = {k: v.cuda() for k, v in syn.context_batch(B, N, 15, seed=7, with_distmat=False).items()
          if k not in ("distmat", "pairwise_dihedrals", "residue_idx")}
    gm = torch.zeros(B, N, dtype=torch.bool)
    for b in range(B):
        first = torch.nonzero(cb["chain_idx"][b].cpu() == 1).flatten()
        gm[b, first[5 + b:15 + b]] = True
    cb["generation_mask"] = gm.cuda()
    cb["antigen_mask"] = cb["chain_idx"] == 3

    def call():
        sel = patch.select(cb["xyz"], cb["generation_mask"], k=128, antigen_mask=cb["antigen_mask"], chain_idx=cb["chain_idx"],
                           residue_mask=cb["residue_mask"])
        g = patch.gather(cb, sel)
        samples = {"seq_idx": (g["seq_idx"] + 1) % 20, "translations": g["xyz"][:, :, 1] + 1.0, "orientations": g["orientations"].transpose(-1, -2)}
        samples = {k: v.repeat_interleave(2, dim=0).contiguous() for k, v in samples.items()}
        return {"index": sel.index, "mask": sel.mask, "count": sel.count, "gathered": g, "pasted": patch.paste(cb, sel, samples, num_samples=2)}

    runs = four_runs(call, workspace=False)
    assert int(runs["plain"]["count"].min()) > 0
    assert_contract(runs, "patch select / gather / paste")
