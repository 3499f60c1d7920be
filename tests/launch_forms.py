"""The batch-size-selected launch forms of the dense tiles of the MFMA path, and the cases that reach them (DESIGN 4.3 has the table).

The launchers pick a kernel instantiation from the row count rows = B K alone (csrc/denoiser_internal.h: rowgemm128_rows_per_group,
dense_tile_full, dense_tile_nsplit); diffab_debug_dense_forms reports what they pick.  This module is the one place the cases of
tests/test_launch_forms_host.py (what every case selects, without a device) and tests/test_gpu_launch_forms.py (what the selected
kernels compute) are kept.  Not a test module and not a conftest; importing it loads no library and touches no device.

A form is named by what the diagnostic reports:
  rowgemm128<parts | 64 | 128>[,ragged]   launch_rowgemm128_h3p / _b6p (one selector for both)
  proj_frames_h3<full | ragged, split | unsplit>, proj_frames_f32<full | ragged>, xstat<full | ragged, split | unsplit> (h3 and b6)
  mlp_chain<full | ragged>                 launch_mlp_chain(s)_b6: the last 128-row group
"""
import ctypes as C
from collections import namedtuple

PJ_NB = 14  # column blocks of the six projections (1344 / 96)
# what a case launches -> the launchers whose selectors it exercises
LINEAR, XSTAT, FORWARD, BACKWARD = "linear128", "xstat128", "forward", "backward"
# want = (rows per group of the row GEMM, its last group ragged, FULL, nsplit, rows of the last tile) as diffab_debug_dense_forms reports
Case = namedtuple("Case", "name kind rows nblocks has_parts want")


def xstat_blocks(N, mode):
    """Column blocks of diffab_debug_xstat128: ceil(N / 96), rounded up to an even count by the bf16 x 6 form (mode 1)."""
    nb = (N + 95) // 96
    return (nb + 1) // 2 * 2 if mode == 1 else nb


# diffab_debug_linear128 modes 1 and 2 (the entry passes no parts scratch): M -> (group, ragged)
LINEAR_M = {32640: (64, 0), 32641: (128, 1), 32704: (128, 1), 32768: (128, 0)}
LINEAR_CASES = [(32640, 128), (32641, 128), (32704, 128), (32768, 128), (32704, 1344)]  # (M, Kd)
# diffab_debug_xstat128 modes 1 and 2: M -> (FULL, nsplit, rows of the last tile); 16384 is the far side of the nsplit threshold
XSTAT_M = {16384: (1, 2, 128), 16512: (1, 1, 128), 16385: (0, 1, 1), 16448: (0, 1, 64)}
XSTAT_N = (1024, 100)
# Denoiser forward at BENCH_DIMS, NL = 2: K -> {B: (group of to_out, ragged, FULL, nsplit of the projections, last tile)}.  to_out is
# launched with parts scratch (16 k parts); K = 64, B = 64 is 64 tiles of 64 rows, the last batch of the parts form.
FORWARD_B = {
    64: {1: (0, 0, 0, 14, 64), 3: (0, 0, 0, 14, 64), 64: (0, 0, 1, 8, 128), 65: (64, 0, 0, 7, 64), 257: (64, 0, 0, 1, 64),
         511: (128, 1, 0, 1, 64)},
    192: {1: (0, 0, 0, 14, 64), 3: (0, 0, 0, 14, 64), 23: (64, 0, 0, 7, 64), 87: (64, 0, 0, 1, 64), 171: (128, 1, 0, 1, 64)},
}
# Denoiser under autograd, K = 64: the taped forward and the backward launch their row GEMMs without parts scratch
BACKWARD_B = {257: (64, 0, 0, 1, 64), 511: (128, 1, 0, 1, 64)}
XSTAT_BWD_NB = 11  # d feat = d y W_out: ceil(1024 / 96) blocks of the fp16 x 3 form


def cases():
    out = []
    for M, Kd in LINEAR_CASES:
        g, ragged = LINEAR_M[M]
        out.append(Case(f"linear128_M{M}_Kd{Kd}", LINEAR, M, 1, 0, (g, ragged, int(M % 128 == 0), 1, M - (M - 1) // 128 * 128)))
    for M, (full, nsplit, last) in XSTAT_M.items():
        for N in XSTAT_N:
            for mode in (1, 2):
                g = 128 if -(-M // 128) >= 256 else 64
                out.append(Case(f"xstat128_M{M}_N{N}_mode{mode}", XSTAT, M, xstat_blocks(N, mode), 0,
                                (g, int(M % g != 0), full, min(nsplit, xstat_blocks(N, mode)), last)))
    for K, table in FORWARD_B.items():
        for B, want in table.items():
            out.append(Case(f"forward_K{K}_B{B}", FORWARD, B * K, PJ_NB, 1, want))
    for B, want in BACKWARD_B.items():
        out.append(Case(f"backward_K64_B{B}", BACKWARD, B * 64, XSTAT_BWD_NB, 0, want))
    return out


def dense_forms(lib, rows, nblocks, has_parts):
    """diffab_debug_dense_forms as a 5-tuple (host arithmetic: `lib` may be a library loaded without a device)."""
    out = (C.c_int32 * 5)()
    rc = lib.diffab_debug_dense_forms(rows, nblocks, has_parts, out)
    assert rc == 0, lib.diffab_last_error()
    return tuple(out)


def forms_of(kind, got):
    """The instantiations a case of `kind` runs when the diagnostic reports `got`."""
    group, ragged, full, nsplit, last = got
    rowgemm = "rowgemm128<%s>" % ("parts" if group == 0 else group) + (",ragged" if ragged else "")
    tile = "%s,%s" % ("full" if full else "ragged", "split" if nsplit > 1 else "unsplit")
    if kind == LINEAR:
        return {rowgemm}
    if kind == XSTAT:
        return {f"xstat<{tile}>"}
    chain = "mlp_chain<%s>" % ("full" if last == 128 else "ragged")
    if kind == FORWARD:  # flags 0 / PAIR_PLANES: the fp16 x 3 tiles and the chains; FP32_GEMM: the fp32 projection tile
        return {rowgemm, f"proj_frames_h3<{tile}>", "proj_frames_f32<%s>" % ("full" if full else "ragged"), chain}
    assert kind == BACKWARD
    return {rowgemm, f"proj_frames_h3<{tile}>", f"xstat<{tile}>"}


# The instantiations no test ran before these cases: every one of them has to be reached by a case, whatever the thresholds become.
NEVER_RUN_BEFORE = {
    "rowgemm128<128>,ragged",
    "xstat<full,unsplit>", "xstat<ragged,unsplit>",
    "proj_frames_h3<ragged,split>", "proj_frames_h3<ragged,unsplit>", "proj_frames_f32<ragged>",
    "mlp_chain<ragged>",
}
# Both sides of every threshold: (what, (rows, nblocks, has_parts) below, (...) above, index into the report, value below, value above)
THRESHOLDS = [
    ("128-row groups of the row GEMM from ceil(M / 128) = 256", (32640, 1, 0), (32641, 1, 0), 0, 64, 128),
    ("one work-group per row tile past 128 tiles", (16384, 11, 0), (16385, 11, 0), 3, 2, 1),
    ("(row tile, k part) form of the row GEMM up to 64 tiles of 64 rows", (64 * 64, PJ_NB, 1), (65 * 64, PJ_NB, 1), 0, 0, 64),
]
