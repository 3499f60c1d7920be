"""CPU: the host side of design scoring (DiffAb.score, diffab_score_designs) - the C-ABI entries and their ctypes registration, the argument
validation that happens before any library call, and the workspace sizing (host-only C-ABI calls)."""
import ctypes as C
import os
import re

import pytest
import torch

import sampler_support as support
from conftest import REPO
from diffab_pytorch import _hip, synthetic as syn
from sampler_support import ReachedTheLibrary, inputs, refuse_library, stand_in


@pytest.fixture(scope="module")
def model():
    return stand_in(("score",))


@pytest.fixture
def no_library(monkeypatch):
    refuse_library(monkeypatch)


def call(model, inp, **kw):
    return support.call(model, inp, method="score", **kw)


def test_score_entries_are_exported_and_registered():
    src = open(os.path.join(REPO, "include", "diffab_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    lib = C.CDLL(_hip.LIB_PATH)
    for name, n_args in (("diffab_score_workspace_bytes", 2), ("diffab_score_designs", 26)):
        assert hasattr(lib, name), name
        proto = re.search(name + r"\s*\(([^)]*)\)", src).group(1)
        assert len(proto.split(",")) == n_args, name
        assert len(_hip.SYMBOLS[name][1]) == n_args, name
    assert C.sizeof(_hip.ScoreNoised) == 32


@pytest.mark.parametrize("kw,match", [
    (dict(mode="sequence"), "unknown mode"),
    (dict(mode="fixed_backbone", generate_structure=False), "sets generate_structure"),
    (dict(mode="structure", generate_sequence=False), "sets generate_structure"),
    (dict(flags=_hip.FLAG_KEEP_STRUCTURE), "mode="),
    (dict(t=0), r"\[1, T = 10\]"),
    (dict(t=11), r"\[1, T = 10\]"),
    (dict(t=[1, 5, 11]), r"\[1, T = 10\]"),
    (dict(t=[3, 4, 3]), "duplicate"),
    (dict(t=[]), "empty"),
    (dict(t=[[1, 2]]), "1-D"),
    (dict(t=torch.tensor([1.0, 2.0])), "integer"),
    (dict(num_draws=0), "num_draws"),
    (dict(num_draws=True), "num_draws"),
    (dict(first_design=-1), "first_design"),
    (dict(rows_per_launch=0), "rows_per_launch"),
])
def test_invalid_arguments_raise_before_the_library(model, no_library, kw, match):
    with pytest.raises(ValueError, match=match):
        call(model, inputs(2), **kw)


def test_context_index_rules(model, no_library):
    with pytest.raises(ValueError, match="context_index must be an integer vector of length 4"):
        call(model, inputs(4, n_ctx=2), context_index=torch.tensor([0, 1, 1]))
    with pytest.raises(ValueError, match=r"\[0, 2\)"):
        call(model, inputs(4, n_ctx=2), context_index=torch.tensor([0, 1, 2, 1]))
    with pytest.raises(ValueError, match=r"\[0, 2\)"):
        call(model, inputs(4, n_ctx=2), context_index=torch.tensor([0, -1, 1, 1]))
    inp = inputs(4, n_ctx=2)
    del inp["pair_context_emb"], inp["res_context_emb"]
    with pytest.raises(ValueError, match="context_index needs"):
        call(model, inp, context_index=torch.tensor([0, 0, 1, 1]))
    # without context_index the contexts are one per design
    with pytest.raises(ValueError, match="one row per design"):
        call(model, inputs(4, n_ctx=2))


def test_wrongly_shaped_inputs_are_rejected(model, no_library):
    for name, bad in (("xyz", torch.zeros(2, 16, 4)), ("xyz", torch.zeros(3, 16, 3)), ("orientations", torch.zeros(2, 16, 3)),
                      ("generation_mask", torch.zeros(2, 15, dtype=torch.bool)), ("residue_mask", torch.ones(2, 17, dtype=torch.bool)),
                      ("res_context_emb", torch.zeros(2, 16, 64)), ("pair_context_emb", torch.zeros(2, 16, 8, 64))):
        inp = dict(inputs(2), **{name: bad})
        with pytest.raises(ValueError, match=name):
            call(model, inp)
    with pytest.raises(ValueError, match="seq_idx"):
        call(model, dict(inputs(2), seq_idx=torch.zeros(2, 16)))
    with pytest.raises(ValueError, match="generation_mask"):
        call(model, dict(inputs(2), generation_mask=None))
    inp = inputs(2)
    del inp["res_context_emb"], inp["pair_context_emb"]  # encode_context needs all-atom xyz, atom_mask and chain_idx
    with pytest.raises(ValueError, match="encode_context"):
        call(model, inp)


def test_workspace_grows_with_rows_per_launch_and_contexts_only():
    lib = _hip.load_library()
    d = syn.BENCH_DIMS

    def ws(B, n_ctx, K=128):
        dims = _hip.make_dims(B, K, d["D"], d["C"], d["H"], d["DS"], d["PQ"], d["PV"], d["NL"], d["V"])
        return lib.diffab_score_workspace_bytes(C.byref(dims), n_ctx)

    assert ws(256, 16) < ws(512, 16)
    assert ws(256, 16) < ws(256, 64)
    # the denoiser's step buffers of B rows are part of it (their fp16 pair planes: n_ctx contexts instead of B patches)
    dims = _hip.make_dims(256, 128, d["D"], d["C"], d["H"], d["DS"], d["PQ"], d["PV"], d["NL"], d["V"])
    assert ws(256, 256) > lib.diffab_denoise_workspace_bytes(C.byref(dims)) > ws(256, 16)
    assert ws(256, 0) == 0 and lib.diffab_last_error()


def test_score_asks_for_a_workspace_independent_of_designs_and_steps(model, monkeypatch):
    """What score() asks diffab_score_workspace_bytes for: rows_per_launch (capped by the rows of the call) and n_ctx - never R n_t M."""
    seen = []

    class Fake:
        def diffab_score_workspace_bytes(self, dims, n_ctx):
            seen.append((dims._obj.B, dims._obj.K, n_ctx))
            raise ReachedTheLibrary()

    monkeypatch.setattr(_hip, "lib", lambda: Fake())
    for R, n_ctx, t, M, rows in ((8, 2, None, 4, None), (64, 2, None, 4, None), (64, 2, [1, 2], 1, None), (64, 4, None, 4, 100),
                                 (3, 3, [4], 1, 512)):
        inp = inputs(R, n_ctx=n_ctx)
        with pytest.raises(ReachedTheLibrary):
            call(model, inp, context_index=torch.arange(R) % n_ctx, t=t, num_draws=M, rows_per_launch=rows)
    assert seen == [(256, 16, 2), (256, 16, 2), (128, 16, 2), (100, 16, 4), (3, 16, 3)]
