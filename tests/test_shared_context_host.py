"""CPU: the host side of shared-context sampling (DiffAb.sample(num_samples=N) / context_index, diffab_sample_options.ctx_of_row) - argument
validation that happens before any library call, and the workspace sizing of the shared form (host-only C-ABI calls)."""
import ctypes as C

import pytest
import torch

from diffab_pytorch import _hip, synthetic as syn
from sampler_support import call, inputs, stand_in


@pytest.fixture(scope="module")
def model():
    return stand_in()


@pytest.mark.parametrize("n", [0, -3])
def test_num_samples_below_one_is_rejected(model, n):
    with pytest.raises(ValueError, match="num_samples"):
        call(model, inputs(2), num_samples=n)


def test_num_samples_and_context_index_together_are_rejected(model):
    with pytest.raises(ValueError, match="not both"):
        call(model, inputs(4, n_ctx=2), num_samples=2, context_index=torch.tensor([0, 0, 1, 1]))


@pytest.mark.parametrize("ci", [[0, 1, 1], [0, 1, 1, 0, 1], [[0, 1], [1, 0]]])
def test_context_index_of_the_wrong_length_is_rejected(model, ci):
    with pytest.raises(ValueError, match="context_index"):
        call(model, inputs(4, n_ctx=2), context_index=torch.tensor(ci))


@pytest.mark.parametrize("ci", [[0, 1, 2, 0], [0, -1, 1, 0]])
def test_context_index_out_of_range_is_rejected(model, ci):
    with pytest.raises(ValueError, match=r"\[0, 2\)"):
        call(model, inputs(4, n_ctx=2), context_index=torch.tensor(ci))


def test_context_index_needs_the_contexts(model):
    inp = inputs(4, n_ctx=2)
    del inp["pair_context_emb"]
    with pytest.raises(ValueError, match="context_index needs"):
        call(model, inp, context_index=torch.tensor([0, 0, 1, 1]))


def test_num_samples_contexts_are_per_patch(model):
    # with num_samples the contexts have one row per patch (B), not one per design (B N)
    with pytest.raises(ValueError, match="per patch"):
        call(model, inputs(2, n_ctx=4), num_samples=2)
    inp = inputs(2)
    inp["pair_context_emb"] = torch.zeros(2, 16, 8, 64)
    with pytest.raises(ValueError, match="pair_context_emb"):
        call(model, inp, num_samples=2)


def test_shared_workspace_is_sized_by_the_contexts():
    lib = _hip.load_library()
    d = syn.BENCH_DIMS
    K, Cp = 128, d["C"]
    dims = _hip.make_dims(256, K, d["D"], Cp, d["H"], d["DS"], d["PQ"], d["PV"], d["NL"])
    full = lib.diffab_sample_workspace_bytes(C.byref(dims))
    shared = lib.diffab_sample_shared_workspace_bytes(C.byref(dims), 16)
    assert full > 0 and shared > 0
    # 240 fewer (K, K, C) fp32-sized pair-plane rows; the map and the (B, K, D) residue-context buffer are small against them
    assert full - shared >= 0.9 * 240 * K * K * Cp * 4, (full, shared)
    # one context per state row: the same planes as the unshared loop, plus the map and the residue-context buffer
    same = lib.diffab_sample_shared_workspace_bytes(C.byref(dims), 256)
    assert full < same <= full + 256 * K * d["D"] * 4 + 256 * 4 + 1024
    # the planes grow with the contexts
    assert lib.diffab_sample_shared_workspace_bytes(C.byref(dims), 17) > shared
    assert lib.diffab_sample_shared_workspace_bytes(C.byref(dims), 0) == 0
