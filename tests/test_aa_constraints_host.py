"""CPU: the host side of the sampler's sequence constraints (DiffAb.sample(allowed_aa=...)) - the C-ABI entries, the argument checks
that happen before any library call, and the io.allowed_aa_mask builder."""
import ctypes

import pytest
import torch

import sampler_support as support
from diffab_pytorch import io
from diffab_pytorch.diffab_pytorch import _pack_allowed_aa
from sampler_support import ReachedTheLibrary, inputs, refuse_library, stand_in

V = 21


@pytest.fixture(scope="module")
def model():
    return stand_in()


@pytest.fixture(autouse=True)
def no_library(monkeypatch):
    refuse_library(monkeypatch)


def call(model, **kw):
    return support.call(model, inputs(2), **kw)


@pytest.mark.parametrize("dtype", [torch.uint8, torch.int32, torch.float32, torch.int64])
def test_non_bool_mask_is_rejected(model, dtype):
    with pytest.raises(ValueError, match="must be a bool tensor"):
        call(model, allowed_aa=torch.ones(V, dtype=dtype))


@pytest.mark.parametrize("shape", [(V - 1,), (V + 1,), (16, 20), (2, 16, 22), (), (1, 2, 16, V)])
def test_wrong_last_dimension_or_rank_is_rejected(model, shape):
    with pytest.raises(ValueError, match="must be \\(V,\\), \\(K, V\\) or \\(rows, K, V\\) with V = 21"):
        call(model, allowed_aa=torch.ones(shape, dtype=torch.bool))


@pytest.mark.parametrize("shape", [(15, V), (3, 16, V), (2, 8, V), (17, V)])
def test_shape_that_does_not_broadcast_is_rejected(model, shape):
    with pytest.raises(ValueError, match="does not broadcast"):
        call(model, allowed_aa=torch.ones(shape, dtype=torch.bool))


def test_rows_of_a_num_samples_mask_are_patches(model):
    # with num_samples the mask is per patch (2 rows), not per design (6)
    with pytest.raises(ValueError, match="does not broadcast"):
        call(model, num_samples=3, allowed_aa=torch.ones(6, 16, V, dtype=torch.bool))


def test_vocabulary_above_32_is_rejected():
    big = stand_in(aa_vocab=33)
    with pytest.raises(ValueError, match="V = 33 > 32"):
        call(big, allowed_aa=torch.ones(33, dtype=torch.bool))


def test_generated_residue_without_a_class_is_rejected(model):
    a = torch.ones(2, 16, V, dtype=torch.bool)
    a[1, 5] = False  # residue 5 is generated
    with pytest.raises(ValueError, match="allows no class at 1 generated residue\\(s\\), the first is row 1, residue 5"):
        call(model, allowed_aa=a)


def test_context_residue_without_a_class_is_accepted_by_the_checks(model):
    # an empty set on a context residue is never read; the call gets past every check to the library
    a = torch.ones(16, V, dtype=torch.bool)
    a[0] = False
    with pytest.raises(ReachedTheLibrary):
        call(model, allowed_aa=a)


def test_structure_mode_is_rejected(model):
    with pytest.raises(ValueError, match="mode='structure' does not diffuse"):
        call(model, mode="structure", allowed_aa=torch.ones(V, dtype=torch.bool))


@pytest.mark.parametrize("kw", [dict(), dict(mode="codesign"), dict(mode="fixed_backbone"), dict(optimize_from=4), dict(num_samples=2),
                                dict(context_index=torch.tensor([1, 0, 1]))])
def test_valid_masks_reach_the_library(model, kw):
    # the accepted combinations pass every check (and stop where sample() asks for the library)
    inp = inputs(2)
    if "context_index" in kw:
        for k in ("seq_idx", "xyz", "orientations", "generation_mask"):
            inp[k] = inp[k][[0, 1, 1]]
    for a in (torch.ones(V, dtype=torch.bool), io.allowed_aa_mask(16, exclude="CMX")):
        with pytest.raises(ReachedTheLibrary):
            model.sample(inp["seq_idx"], inp["xyz"], inp["orientations"], generation_mask=inp["generation_mask"],
                         res_context_emb=inp["res_context_emb"], pair_context_emb=inp["pair_context_emb"], seed=1, allowed_aa=a, **kw)


def test_other_checks_keep_their_order(model):
    # the mode check fires before the mask's
    with pytest.raises(ValueError, match="unknown mode"):
        call(model, mode="bogus", allowed_aa=torch.ones(V, dtype=torch.int32))


# ------------------------------------------------------------------ the bit packing
def test_pack_allowed_aa_bits():
    a = torch.zeros(2, 3, V, dtype=torch.bool)
    a[0, 0, 0] = True
    a[0, 1, 20] = True
    a[0, 2] = True
    a[1, 0, [1, 4, 12]] = True
    w = _pack_allowed_aa(a)
    assert w.dtype == torch.int32 and w.shape == (2, 3)
    assert w.tolist() == [[1, 1 << 20, (1 << 21) - 1], [(1 << 1) | (1 << 4) | (1 << 12), 0, 0]]
    full32 = _pack_allowed_aa(torch.ones(32, dtype=torch.bool))
    assert int(full32) == -1  # bit 31 set: the uint32 word 0xffffffff


# ------------------------------------------------------------------ io.allowed_aa_mask
def test_letters_are_in_aa3_order():
    three_to_one = {"ALA": "A", "ARG": "R", "ASN": "N", "ASP": "D", "CYS": "C", "GLN": "Q", "GLU": "E", "GLY": "G", "HIS": "H", "ILE": "I",
                    "LEU": "L", "LYS": "K", "MET": "M", "PHE": "F", "PRO": "P", "SER": "S", "THR": "T", "TRP": "W", "TYR": "Y", "VAL": "V",
                    "UNK": "X"}
    assert io.AA1 == "".join(three_to_one[a] for a in io.AA3)


def test_mask_default_and_exclusion_list():
    assert torch.equal(io.allowed_aa_mask(4), torch.ones(4, V, dtype=torch.bool))
    m = io.allowed_aa_mask(5, exclude="CMX")
    assert m.shape == (5, V) and m.dtype == torch.bool
    want = torch.ones(V, dtype=torch.bool)
    want[[4, 12, 20]] = False
    assert torch.equal(m, want.expand(5, V))


def test_mask_fixed_positions_and_sets():
    m = io.allowed_aa_mask(6, exclude="C", fixed={2: "Y", 4: "FWY", 5: "c"})
    assert m[2].nonzero().flatten().tolist() == [18]
    assert m[4].nonzero().flatten().tolist() == [13, 17, 18]
    assert m[5].nonzero().flatten().tolist() == [4]  # a fixed position allows exactly its letters, an excluded one too
    for k in (0, 1, 3):
        assert m[k].sum() == V - 1 and not m[k, 4]
    x = io.allowed_aa_mask(2, fixed={0: "X"})
    assert x[0].nonzero().flatten().tolist() == [20] and bool(x[1].all())


@pytest.mark.parametrize("kw", [dict(exclude="CB"), dict(exclude="*"), dict(fixed={1: "Z"}), dict(fixed={0: "A-"})])
def test_mask_unknown_letters_are_rejected(kw):
    with pytest.raises(ValueError, match="unknown amino-acid letter"):
        io.allowed_aa_mask(4, **kw)


@pytest.mark.parametrize("fixed", [{4: "A"}, {-1: "A"}, {"1": "A"}])
def test_mask_positions_outside_the_patch_are_rejected(fixed):
    with pytest.raises(ValueError, match="outside"):
        io.allowed_aa_mask(4, fixed=fixed)


def test_mask_empty_fixed_set_is_rejected():
    with pytest.raises(ValueError, match="allows no class"):
        io.allowed_aa_mask(4, fixed={1: ""})


def test_mask_smaller_vocabulary():
    # V = 20 (no UNK class): X is then unknown
    assert io.allowed_aa_mask(3, exclude="C", V=20).shape == (3, 20)
    with pytest.raises(ValueError, match="unknown amino-acid letter 'X'"):
        io.allowed_aa_mask(3, exclude="X", V=20)
