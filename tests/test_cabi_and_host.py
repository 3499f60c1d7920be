"""CPU: the C-ABI library loads and exports every symbol include/diffab_hip.h declares (no compute calls),
plus the host logic of the boundary package: schedule, state_dict layout, seeded-init parity with the
reference's creation order, loud failure without a GPU."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from conftest import REPO
from diffab_pytorch import _hip, synthetic as syn


def header_symbols():
    src = open(os.path.join(REPO, "include", "diffab_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(diffab_[a-z0-9_]+)\s*\(", src)))


def test_library_exports_every_declared_symbol():
    names = header_symbols()
    assert len(names) >= 25
    lib = ctypes.CDLL(_hip.LIB_PATH)
    for n in names:
        assert hasattr(lib, n), f"{n} declared in include/diffab_hip.h but not exported by libdiffab_hip.so"
    assert sorted(_hip.SYMBOLS) == names, "ctypes table and header drifted apart"
    l = _hip.load_library()
    assert b"gfx950" in l.diffab_version()


def test_attn_variant_switch_takes_only_the_reference_path_bits():
    """diffab_debug_set_attn_variant keeps bits 4 (unfused PairEmbedding launches) and 64 (separate PairEmbedding backward launches);
    any other bit is refused with DIFFAB_ERR_ARG and a message, and leaves the switch as it was (host state only: no GPU needed)."""
    l = _hip.load_library()
    try:
        for v in (0, 4, 64, 68):
            assert l.diffab_debug_set_attn_variant(v) == 0, v
        for v in (1, 8, 16, 32):
            assert l.diffab_debug_set_attn_variant(v) == -1, v  # DIFFAB_ERR_ARG
            assert b"debug_set_attn_variant" in l.diffab_last_error(), v
    finally:
        assert l.diffab_debug_set_attn_variant(0) == 0


def test_struct_layouts_match_header():
    assert ctypes.sizeof(_hip.Dims) == 40
    assert ctypes.sizeof(_hip.IpaLayerWeights) == 80
    assert ctypes.sizeof(_hip.Mlp3Weights) == 48
    assert ctypes.sizeof(_hip.DenoiserWeights) == 5 * 8 + 8 + 3 * 48
    assert ctypes.sizeof(_hip.Sched) == 48 and ctypes.sizeof(_hip.Igso3) == 32


def test_null_denoiser_weight_is_refused_on_the_host():
    """Every weight pointer the denoiser forward reads (embedding MLP, every IPA layer, the three heads) is checked before anything is
    enqueued: DIFFAB_ERR_ARG with a weight message.  The workspace is given as 0 bytes, so a call whose weight check missed would stop
    at the workspace check (DIFFAB_ERR_WORKSPACE), still on the host; no GPU is touched either way."""
    l = _hip.load_library()
    dims = syn.BENCH_DIMS
    d = _hip.Dims(2, 128, dims["D"], dims["C"], dims["H"], dims["DS"], dims["PQ"], dims["PV"], 2, 21)
    fake = 256  # never dereferenced: every call below returns before it enqueues work
    layers = (_hip.IpaLayerWeights * 2)(*[_hip.IpaLayerWeights(*[fake] * 10) for _ in range(2)])
    heads = [_hip.Mlp3Weights(*[fake] * 6) for _ in range(3)]
    w = _hip.DenoiserWeights(*[fake] * 5, ctypes.cast(layers, ctypes.POINTER(_hip.IpaLayerWeights)), *heads)

    def call():
        return l.diffab_denoise_step_fwd(ctypes.byref(d), ctypes.byref(w), *[fake] * 12, 0, 0, None)  # 11 tensors + workspace

    assert call() == -4  # DIFFAB_ERR_WORKSPACE: all weights present, the next check refuses the call
    for obj, field in [(w.coord, "w0"), (w.orient, "b2"), (w.seq, "w4"), (w.seq, "b4"), (layers[1], "gamma"), (layers[0], "w_bias"),
                       (layers[1], "b_out")]:
        setattr(obj, field, None)
        assert call() == -1, field  # DIFFAB_ERR_ARG
        assert b"null weight pointer" in l.diffab_last_error(), field
        setattr(obj, field, fake)
    assert call() == -4


# (B, K, D, C, H, DS, PQ, PV, NL, V) -> train_tape_bytes, train_workspace_bytes, ipa_layer_tape_bytes, ipa_layer_bwd_workspace_bytes
TRAIN_LAYOUT_BYTES = [
    ((2, 128, 128, 64, 8, 32, 8, 8, 3, 21), (16654080, 16997632, 7347968, 13851904)),  # fast path, split attention (K = 128)
    ((3, 64, 128, 64, 8, 32, 8, 8, 2, 21), (7734272, 9074432, 5030912, 8288000)),  # ... K = 64
    ((1, 64, 128, 64, 8, 32, 8, 8, 16, 21), (16010752, 3189248, 2493952, 3451648)),  # the deepest tape, NL > kDeLayersMax
    ((2, 128, 128, 64, 8, 32, 8, 8, 7, 21), (35266304, 12278784, 7347968, 13851904)),  # NL just past kDeLayersMax
    ((2, 192, 128, 64, 8, 32, 8, 8, 2, 21), (11097344, 14755840, 7263488, 14755840)),  # fast path without the split attention
    ((2, 7, 20, 6, 3, 5, 2, 3, 2, 21), (39992, 35512, 28960, 35512)),  # generic dims
    ((1, 5, 12, 0, 2, 4, 3, 2, 1, 21), (9436, 7792, 9436, 7792)),  # C = 0
]


def test_training_tape_and_workspace_sizes_are_pinned():
    """The training tape and the backward's workspace are each described once, by the function that carves them; the sizing entries are
    that function with a null base.  Their totals are the ones callers have always allocated (host arithmetic only: no GPU needed), and
    a tape of more than 16 layers is still refused."""
    l = _hip.load_library()
    entries = [l.diffab_train_tape_bytes, l.diffab_train_workspace_bytes, l.diffab_ipa_layer_tape_bytes,
               l.diffab_ipa_layer_bwd_workspace_bytes]
    for dims, want in TRAIN_LAYOUT_BYTES:
        d = _hip.Dims(*dims)
        assert tuple(int(f(ctypes.byref(d))) for f in entries) == want, dims
    assert l.diffab_train_tape_bytes(ctypes.byref(_hip.Dims(1, 64, 128, 64, 8, 32, 8, 8, 17, 21))) == 0


def test_schedule_is_bit_identical_to_reference(golden):
    from diffab_pytorch.diffusion import cosine_variance_schedule

    g = golden("schedule")
    for T, s in ((100, 0.01), (200, 0.01), (100, 8e-3)):
        mine = cosine_variance_schedule(T, s=s, beta_max=0.999)
        assert set(mine) == {"alpha", "alpha_bar", "alpha_bar_sqrt", "one_minus_alpha_bar_sqrt", "beta"}
        for k, v in mine.items():
            # bit-identical on the CPU that generated the goldens; torch.cos may differ by an ulp on another CPU model
            np.testing.assert_allclose(v.numpy(), g[f"T{T}_s{s}_{k}"], rtol=4e-7, atol=1e-30, err_msg=f"{T} {s} {k}")


@pytest.mark.skipif(torch.cuda.is_available(), reason="CPU-box behaviour")
def test_compute_fails_loudly_without_gpu():
    from diffab_pytorch import so3

    with pytest.raises(_hip.HipUnavailable):
        so3.log_rotmat(torch.eye(3).expand(2, 2, 3, 3))


def test_denoiser_state_dict_layout_and_seeded_init():
    """Keys/shapes of SURVEY.md Appendix B.3 and the reference's parameter creation order."""
    from diffab_pytorch.diffab_pytorch import Denoiser

    d = syn.BENCH_DIMS
    torch.manual_seed(0)
    den = Denoiser(d["D"], d["C"], d["NL"], d["DS"], d["PQ"], d["PV"], d["H"], 21)
    sd = den.state_dict()
    want = syn.denoiser_state_dict(d, prefix="")
    assert list(sd) == list(want) or set(sd) == set(want)
    for k, v in want.items():
        assert tuple(sd[k].shape) == tuple(v.shape), k
    assert sum(p.numel() for p in den.parameters()) == 1_978_827
    assert len(list(den.buffers())) == 0
    den.load_state_dict(want, strict=True)
    # gamma init = log(e - 1), raw (reference diffab_pytorch.py:373)
    torch.manual_seed(0)
    den2 = Denoiser(d["D"], d["C"], 1, d["DS"], d["PQ"], d["PV"], d["H"], 21)
    assert torch.allclose(den2.ipa.layers[0].gamma, torch.full((8,), float(np.log(np.e - 1.0))))


def test_diffab_constructor_surface(monkeypatch):
    """DiffAb() needs the GPU for its IGSO3 table; on a CPU box check the class surface only."""
    import inspect

    from diffab_pytorch import DiffAb

    sig = inspect.signature(DiffAb.__init__)
    extra = [n for n, q in sig.parameters.items() if q.kind is inspect.Parameter.KEYWORD_ONLY]
    # build-defined keyword; its default is the reference's behaviour (torch.multinomial without replacement, so3.py:78)
    assert extra == ["igso3_without_replacement"] and sig.parameters["igso3_without_replacement"].default is True
    assert [n for n in list(sig.parameters)[1:] if n not in extra] == ["d_residue_emb", "d_pair_emb", "n_ipa_layers", "d_scalar_per_head", "n_query_point_per_head",
                                        "n_value_point_per_head", "n_head", "T", "s", "beta_max", "n_atoms", "aa_vocab_size",
                                        "max_dist_to_consider", "lr", "weight_decay", "betas"]
    for m in ("encode_context", "denoise", "sample", "_add_noise", "_shared_step", "training_step", "validation_step",
              "configure_optimizers"):
        assert callable(getattr(DiffAb, m))
    assert list(inspect.signature(DiffAb.denoise).parameters)[1:] == [
        "seq_idx_t", "translations_t", "orientations_t", "res_context_emb", "pair_context_emb", "beta", "generation_mask", "residue_mask"]
    assert list(inspect.signature(DiffAb.sample).parameters)[1:4] == ["seq_idx", "xyz", "orientations"]


def test_synthetic_patches_are_shard_invariant():
    d = syn.UNIT_DIMS
    full = syn.patches(4, 16, d, seed=3)
    lo = syn.patches(2, 16, d, seed=3, first_patch=0)
    hi = syn.patches(2, 16, d, seed=3, first_patch=2)
    for k in full:
        assert torch.equal(full[k], torch.cat([lo[k], hi[k]])), k
    R = full["orientations"]
    eye = torch.eye(3).expand_as(R)
    assert torch.allclose(R.transpose(-1, -2) @ R, eye, atol=1e-5)
    assert (full["generation_mask"].sum(-1) >= 5).all() and (full["generation_mask"].sum(-1) <= 20).all()



# ------------------------------------------------------------------ the sampler's C ABI: two loop entries, three init entries, one options struct
REMOVED_SAMPLER_ENTRIES = ("diffab_sample_loop_shared", "diffab_sample_loop_aa", "diffab_sample_loop_rec", "diffab_sample_loop_steps",
                           "diffab_sample_loop_guided", "diffab_sample_loop_tempered", "diffab_sample_loop_steered", "diffab_sample_init_aa",
                           "diffab_sample_init_noised_aa")
OPTION_STRUCTS = {"diffab_sample_options": _hip.SampleOptions, "diffab_sample_record": _hip.SampleRecord,
                  "diffab_sample_steps": _hip.SampleSteps, "diffab_sample_guidance": _hip.SampleGuidance,
                  "diffab_sample_temperature": _hip.SampleTemperature, "diffab_sample_steering": _hip.SampleSteering}
C_SCALARS = {"int32_t": ctypes.c_int32, "uint32_t": ctypes.c_uint32, "float": ctypes.c_float}


def header_struct(name):
    """ctypes restatement of `typedef struct { ... } name;` as include/diffab_hip.h declares it: fields in the header's order, every
    pointer a void*, the scalars by their C type."""
    src = open(os.path.join(REPO, "include", "diffab_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    body = re.search(r"typedef struct \{([^}]*)\}\s*" + name + r"\s*;", src).group(1)
    fields = []
    for decl in filter(None, (d.strip() for d in body.split(";"))):
        ctype, names = re.fullmatch(r"(?:const\s+)?(\w+)\s*(.*)", decl).groups()
        for n in names.split(","):
            n = n.strip()
            fields.append((n.lstrip("* "), ctypes.c_void_p if n.startswith("*") else C_SCALARS[ctype]))
    return type(name, (ctypes.Structure,), {"_fields_": fields})


def test_sample_option_structs_match_the_header():
    sizes = {"diffab_sample_options": 64, "diffab_sample_record": 72, "diffab_sample_steps": 40, "diffab_sample_guidance": 56,
             "diffab_sample_temperature": 32, "diffab_sample_steering": 104}
    for name, mine in OPTION_STRUCTS.items():
        want = header_struct(name)
        assert [f[0] for f in mine._fields_] == [f[0] for f in want._fields_], name  # the header's field order
        assert ctypes.sizeof(mine) == ctypes.sizeof(want) == sizes[name], name
        for field, ctype in want._fields_:
            assert getattr(mine, field).offset == getattr(want, field).offset, (name, field)
            assert getattr(mine, field).size == ctypes.sizeof(ctype), (name, field)
    opt = _hip.SampleOptions(n_ctx=3, temperature=_hip.SampleTemperature())  # by keyword; struct_bytes filled in
    assert (opt.struct_bytes, opt.n_ctx) == (64, 3) and opt.temperature and not opt.record and not opt.ctx_of_row


def test_sampler_entries_are_two_loops_and_three_inits():
    lib = ctypes.CDLL(_hip.LIB_PATH)
    for name in REMOVED_SAMPLER_ENTRIES:
        assert name not in _hip.SYMBOLS and not hasattr(lib, name), name
    names = header_symbols()
    assert [n for n in names if n.startswith("diffab_sample_loop")] == ["diffab_sample_loop", "diffab_sample_loop_ex"]
    assert [n for n in names if n.startswith("diffab_sample_init")] == ["diffab_sample_init", "diffab_sample_init_ex",
                                                                        "diffab_sample_init_noised"]
    counts = {"diffab_sample_loop": 18, "diffab_sample_loop_ex": 19, "diffab_sample_init": 10, "diffab_sample_init_ex": 12,
              "diffab_sample_init_noised": 14}
    for name, n in counts.items():
        assert len(_hip.SYMBOLS[name][1]) == n, name
    # diffab_sample_loop's arguments plus the options (a pointer) just before the stream
    loop, ex = _hip.SYMBOLS["diffab_sample_loop"][1], _hip.SYMBOLS["diffab_sample_loop_ex"][1]
    assert ex[:-2] == loop[:-1] and ex[-1] == loop[-1] and ex[-2] == ctypes.POINTER(_hip.SampleOptions)


def fake_loop_call(l, B=2):
    """diffab_sample_loop_ex(opt) on pointers that are never dereferenced and a workspace of 0 bytes: a call that passes every argument
    check stops at the workspace check (DIFFAB_ERR_WORKSPACE), still on the host; no GPU is touched."""
    dims = syn.BENCH_DIMS
    d = _hip.Dims(B, 128, dims["D"], dims["C"], dims["H"], dims["DS"], dims["PQ"], dims["PV"], 2, 21)
    fake = 256
    layers = (_hip.IpaLayerWeights * 2)(*[_hip.IpaLayerWeights(*[fake] * 10) for _ in range(2)])
    w = _hip.DenoiserWeights(*[fake] * 5, ctypes.cast(layers, ctypes.POINTER(_hip.IpaLayerWeights)),
                             *[_hip.Mlp3Weights(*[fake] * 6) for _ in range(3)])
    sched = _hip.Sched(10, *[fake] * 5)
    tab = _hip.Igso3(11, 64, fake, fake, 0.1)
    head = (ctypes.byref(d), ctypes.byref(w), ctypes.byref(sched), ctypes.byref(tab), *[fake] * 6, 1, 0, 10, 7, fake, 0, 0)

    def call(opt):
        return l.diffab_sample_loop_ex(*head, None if opt is None else ctypes.byref(opt), None)

    call.plain = lambda: l.diffab_sample_loop(*head, None)
    return call


def test_sample_options_struct_bytes_is_checked_first():
    l = _hip.load_library()
    call = fake_loop_call(l)
    for n in (0, 56):
        opt = _hip.SampleOptions()
        opt.struct_bytes = n
        opt.allowed = 256  # not read: the size is refused before any other field
        assert call(opt) == -1, n  # DIFFAB_ERR_ARG
        assert b"struct_bytes" in l.diffab_last_error(), n


def test_sample_options_n_ctx_without_a_map_is_zero_or_b():
    l = _hip.load_library()
    call = fake_loop_call(l, B=2)
    for n_ctx in (1, 3, -1):
        assert call(_hip.SampleOptions(n_ctx=n_ctx)) == -1, n_ctx  # DIFFAB_ERR_ARG
        assert b"without ctx_of_row n_ctx must equal B" in l.diffab_last_error(), n_ctx
    for n_ctx in (0, 2):
        assert call(_hip.SampleOptions(n_ctx=n_ctx)) == -4, n_ctx  # DIFFAB_ERR_WORKSPACE: the next check


def test_null_and_zeroed_sample_options_reach_the_same_check():
    l = _hip.load_library()
    call = fake_loop_call(l)
    errors = []
    for rc in (call.plain(), call(None), call(_hip.SampleOptions())):
        assert rc == -4  # DIFFAB_ERR_WORKSPACE at 0 bytes
        errors.append(l.diffab_last_error())
    assert errors[0] == errors[1] == errors[2] and b"sample_loop: workspace 0 <" in errors[0]
