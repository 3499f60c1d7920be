"""CPU: the host side of the sampler's design modes (DiffAb.sample(mode=..., optimize_from=...)) - the C-ABI flags and entries, and the
argument checks that happen before any library call."""
import ctypes
import os
import re

import pytest

import sampler_support as support
from conftest import REPO
from diffab_pytorch import _hip
from diffab_pytorch.diffab_pytorch import SAMPLE_MODES
from sampler_support import inputs, stand_in


def header_defines():
    src = open(os.path.join(REPO, "include", "diffab_hip.h")).read()
    return {k: int(v) for k, v in re.findall(r"#define\s+(DIFFAB_FLAG_\w+)\s+(\d+)u", src)}


def test_flags_match_the_header():
    h = header_defines()
    assert h["DIFFAB_FLAG_KEEP_STRUCTURE"] == _hip.FLAG_KEEP_STRUCTURE == 2048
    assert h["DIFFAB_FLAG_KEEP_SEQUENCE"] == _hip.FLAG_KEEP_SEQUENCE == 4096
    # bits 2, 4 and 8 are retired; every flag is its own bit
    values = list(h.values())
    assert len(set(values)) == len(values) and all(v & (v - 1) == 0 for v in values)
    assert not {2, 4, 8} & set(values)


def test_mode_table():
    assert SAMPLE_MODES["codesign"] == (True, True, 0)
    assert SAMPLE_MODES["fixed_backbone"] == (False, True, _hip.FLAG_KEEP_STRUCTURE)
    assert SAMPLE_MODES["structure"] == (True, False, _hip.FLAG_KEEP_SEQUENCE)


@pytest.fixture(scope="module")
def model():
    return stand_in()


def call(model, **kw):
    return support.call(model, inputs(2), **kw)


@pytest.mark.parametrize("mode", ["co-design", "Structure", "", 3])
def test_unknown_mode_is_rejected(model, mode):
    with pytest.raises(ValueError, match="unknown mode"):
        call(model, mode=mode)


@pytest.mark.parametrize("mode", sorted(SAMPLE_MODES))
@pytest.mark.parametrize("kw", [dict(generate_structure=False), dict(generate_sequence=False),
                                dict(generate_structure=False, generate_sequence=False)])
def test_mode_with_generate_flags_is_rejected(model, mode, kw):
    with pytest.raises(ValueError, match="sets generate_structure"):
        call(model, mode=mode, **kw)


@pytest.mark.parametrize("t", [0, -1, 11, 100, True, 2.0])
def test_optimize_from_outside_the_schedule_is_rejected(model, t):
    with pytest.raises(ValueError, match=r"optimize_from must be an int in \[1, T = 10\]"):
        call(model, optimize_from=t)


@pytest.mark.parametrize("mode", [None, "fixed_backbone"])
def test_optimize_from_with_init_false_is_rejected(model, mode):
    with pytest.raises(ValueError, match="init=False"):
        call(model, optimize_from=4, init=False, mode=mode)


@pytest.mark.parametrize("t_start", [10, 3, 0])
def test_t_start_that_disagrees_with_optimize_from_is_rejected(model, t_start):
    with pytest.raises(ValueError, match="disagrees with optimize_from"):
        call(model, optimize_from=4, t_start=t_start)


def test_mode_checks_come_before_the_shared_context_checks(model):
    # the design-mode checks fire first, whatever else is wrong with the call
    with pytest.raises(ValueError, match="unknown mode"):
        call(model, mode="bogus", num_samples=0)
