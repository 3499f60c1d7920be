"""CPU: which kernel instantiation the dense tiles of the MFMA path pick at the row counts of tests/launch_forms.py, asked of the
library's own selectors through diffab_debug_dense_forms (host arithmetic: no device, nothing enqueued).

  1. Every case selects the form its row of the table names.
  2. The cases together reach every instantiation that no test ran before them, and both sides of every threshold of the selectors -
     whoever moves a threshold is told which form has lost its case.
"""
import ctypes as C

from diffab_pytorch import _hip
from launch_forms import FORWARD_B, LINEAR_CASES, NEVER_RUN_BEFORE, THRESHOLDS, XSTAT_M, cases, dense_forms, forms_of


def test_every_case_selects_the_form_its_table_names():
    lib = _hip.load_library()
    table = cases()
    assert len({c.name for c in table}) == len(table)
    for c in table:
        assert dense_forms(lib, c.rows, c.nblocks, c.has_parts) == c.want, c.name
    # the row counts the issue names, as the table holds them
    assert [m for m, _ in LINEAR_CASES] == [32640, 32641, 32704, 32768, 32704] and set(XSTAT_M) == {16384, 16512, 16385, 16448}
    assert set(FORWARD_B[64]) >= {1, 3, 65, 257, 511} and set(FORWARD_B[192]) == {1, 3, 23, 87, 171}


def test_cases_cover_every_new_instantiation_and_both_sides_of_each_threshold():
    lib = _hip.load_library()
    table = cases()
    reached = set()
    for c in table:
        reached |= forms_of(c.kind, dense_forms(lib, c.rows, c.nblocks, c.has_parts))
    missing = sorted(NEVER_RUN_BEFORE - reached)
    assert not missing, f"no case of tests/launch_forms.py reaches {missing}"
    in_table = {(c.rows, c.has_parts) for c in table}
    for what, below, above, index, v_below, v_above in THRESHOLDS:
        for side, v in ((below, v_below), (above, v_above)):
            assert (side[0], side[2]) in in_table, f"{what}: no case at rows = {side[0]}"
            assert dense_forms(lib, *side)[index] == v, f"{what}: rows = {side[0]} no longer selects {v}"
    # one row either way of each threshold, whatever the table holds
    assert dense_forms(lib, 255 * 128, 1, 0)[0] == 64 and dense_forms(lib, 255 * 128 + 1, 1, 0)[0] == 128
    assert dense_forms(lib, 128 * 128, 14, 0)[3] == 2 and dense_forms(lib, 128 * 128 + 1, 14, 0)[3] == 1
    assert dense_forms(lib, 64 * 64, 14, 1)[0] == 0 and dense_forms(lib, 64 * 64 + 1, 14, 1)[0] == 64
    assert dense_forms(lib, 64, 14, 0)[0] == 64  # without parts scratch never the parts form


def test_dense_forms_refuses_bad_arguments_on_the_host():
    lib = _hip.load_library()
    out = (C.c_int32 * 5)(*[7] * 5)
    for rows, nblocks, ptr in ((0, 1, out), (1 << 31, 1, out), (128, 0, out), (128, 1, None)):
        assert lib.diffab_debug_dense_forms(rows, nblocks, 0, ptr) == -1  # DIFFAB_ERR_ARG
        assert b"debug_dense_forms" in lib.diffab_last_error()
    assert list(out) == [7] * 5
