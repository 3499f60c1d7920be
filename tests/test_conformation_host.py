"""Loop conformations without a GPU: the restatement of conformation_ref.py on hand-made cases with the answers
written out, dihedral_set / DihedralSet, the header / library / ctypes table of include/diffab_hip_conformation.h, its workspace macro
against the Python mirror, every host-side refusal of the two entries, and the argument errors of metrics.conformation /
metrics.design_dihedrals."""
import ctypes
import inspect
import math
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

from conftest import REPO
from conformation_ref import bound, features, nearest_ref, pack_ref, pair_matrix
from diffab_pytorch import _hip, metrics
from sampler_support import ReachedTheLibrary, refuse_library

HEADER = os.path.join(REPO, "include", "diffab_hip_conformation.h")
PI = math.pi
NAN = float("nan")


def loops_of(loops):
    """(angles (n, L, 3) float64 with NaN behind the lengths, lengths (n)) of lists of (phi, psi, omega) rows."""
    L = max([len(x) for x in loops] + [1])
    out = np.full((len(loops), L, 3), np.nan)
    for m, x in enumerate(loops):
        out[m, :len(x)] = np.asarray(x, np.float64).reshape(len(x), 3)
    return out, np.array([len(x) for x in loops])


def dist(a, b, which=(0, 1), na=None, nb=None, min_terms=1):
    """d, n of one loop against one loop, the float64 value and the fp32 steps."""
    (qa, la), (qb, lb) = loops_of([a]), loops_of([b])
    d, n, _, d32 = pair_matrix(features(qa, which), la if na is None else [na], features(qb, which), lb if nb is None else [nb], min_terms)
    return float(d[0, 0]), int(n[0, 0]), float(d32[0, 0])


# ------------------------------------------------------------------ the restatement, by hand
def test_hand_made_distances():
    a = [(-1.0, 2.0, 3.0), (0.5, -0.5, 3.1)]
    assert dist(a, a)[:2] == (pytest.approx(0, abs=1e-7), 4) and dist(a, a)[2] <= 2 ** -22
    off = [(p + PI, q + PI, w) for p, q, w in a]
    assert dist(a, off)[0] == pytest.approx(4, abs=1e-6) and dist(a, off, which=(2,))[0] == pytest.approx(0, abs=1e-7)
    quarter = [(a[0][0] + PI / 2, a[0][1], a[0][2]), a[1]]
    assert dist(a, quarter)[0] == pytest.approx(0.5, abs=1e-6)  # one of four angles off by pi/2: (2 + 0 + 0 + 0) / 4
    assert dist(a, quarter, which=(0, 1, 2))[0] == pytest.approx(2 / 6, abs=1e-6) and dist(a, quarter, which=(0, 1, 2))[1] == 6
    assert dist(a, a + [(0.0, 0.0, 0.0)])[0] == math.inf and dist(a, a[:1])[0] == math.inf  # unequal lengths


def test_a_missing_angle_drops_its_term_and_min_terms_is_a_boundary():
    a = [(NAN, 2.0, 3.0), (0.5, -0.5, NAN)]
    b = [(1.0, 2.0, 3.0), (0.5, -0.5 + PI, 3.0)]
    d, n, _ = dist(a, b)
    assert n == 3 and d == pytest.approx(4 / 3, abs=1e-6)  # psi_0 equal, phi_1 equal, psi_1 off by pi: (0 + 0 + 4) / 3
    assert dist(b, a)[:2] == (d, n)
    assert dist(a, b, min_terms=3)[0] == d and dist(a, b, min_terms=4)[0] == math.inf
    assert dist(a, b, which=(2,))[1] == 1 and dist(a, b, which=(0,))[1] == 1
    both = [(NAN, NAN, NAN), (NAN, NAN, NAN)]
    assert dist(both, b) == (math.inf, 0, math.inf)
    assert dist([], []) == (math.inf, 0, math.inf)  # two empty loops: equal lengths, no term, and min_terms >= 1


def test_lengths_are_clamped_and_slots_behind_them_are_not_read():
    a = [(1.0, 2.0, 3.0), (0.5, -0.5, 3.0), (0.1, 0.2, 0.3)]
    b = [(1.0, 2.0, 3.0), (0.5, -0.5, 3.0), (2.0, 2.0, 2.0)]
    assert dist(a, b, na=2, nb=2)[:2] == (pytest.approx(0, abs=1e-7), 4)
    assert dist(a, b, na=9, nb=3)[1] == 6 and dist(a, b, na=1000, nb=2 ** 31 - 1)[1] == 6 and dist(a, b, na=-4, nb=0) == (math.inf, 0, math.inf)
    assert dist(a, b, na=2, nb=3)[0] == math.inf


def test_per_query_outputs_of_the_restatement():
    base = [(0.3, -1.0, 3.0), (-2.0, 2.5, 3.1)]
    turn = lambda x, by: [(p + by, q, w) for p, q, w in x]
    queries, nq = loops_of([base, turn(base, 0.5), [(0.0, 0.0, 0.0)]])
    library, nl = loops_of([turn(base, 1.25), base, base, turn(base, 0.5), [(1.0, 1.0, 1.0)] * 3])
    d, n, mag, d32 = pair_matrix(features(queries, (0, 1)), nq, features(library, (0, 1)), nl)
    assert np.isinf(d[:, 4]).all() and np.isinf(d[2]).all() and (n[:2, :4] == 4).all()
    half = 2 * (1 - math.cos(0.5)) / 2  # two of four angles off by 0.5
    assert d[0, 3] == pytest.approx(half, abs=1e-6) and d[1, 3] == pytest.approx(0, abs=1e-6)
    out = nearest_ref(d32, n, radius=float(d32[0, 3]))
    assert out["index"].tolist() == [1, 3, -1] and out["n_terms"].tolist() == [4, 4, 0]  # ties go to the lower index: entries 1 and 2
    assert out["distance"][2] == np.inf and out["distance"].dtype == np.float32
    assert out["n_within"][[0, 2]].tolist() == [3, 0]  # the radius is exactly d(0, 3): counted
    below = nearest_ref(d32, n, radius=float(np.nextafter(d32[0, 3], np.float32(0))))
    assert below["n_within"][0] == 2
    skipped = nearest_ref(d32, n, skip=[1, 3, 0], radius=-1.0)
    assert skipped["index"].tolist() == [2, 1, -1] and skipped["n_within"].tolist() == [0, 0, 0]
    assert nearest_ref(d32, n, radius=float("nan"))["n_within"].tolist() == [0, 0, 0]
    one = nearest_ref(d32[:, :1], n[:, :1], skip=[0, 5, -1], radius=9.0)
    assert one["index"].tolist() == [-1, 0, -1] and one["n_within"].tolist() == [0, 1, 0] and one["n_terms"].tolist() == [0, 4, 0]
    none = nearest_ref(d32[:, :0], n[:, :0], radius=3.0)
    assert none["index"].tolist() == [-1] * 3 and np.isinf(none["distance"]).all() and none["matrix"].shape == (3, 0)
    b = bound(n, mag, 2, nq)
    assert (np.abs(d32[:2, :4] - d[:2, :4]) <= b[:2, :4]).all() and b.max() < 1e-5


def test_pack_restatement():
    phi = np.array([[0.1, 0.2, 0.3, 0.4], [1.1, 1.2, 1.3, 1.4]], np.float32)
    psi, omega = phi + 10, phi + 20
    phi[0, 1] = np.nan
    mask = np.array([[1, 1, 0, 1]])
    out, n = pack_ref(phi, psi, omega, mask, group_size=2, L=2)
    assert n.tolist() == [3, 3] and np.isnan(out[0, 1, 0]) and out[1].tolist() == [[np.float32(1.1), np.float32(11.1), np.float32(21.1)],
                                                                                    [np.float32(1.2), np.float32(11.2), np.float32(21.2)]]
    out, n = pack_ref(phi, psi, omega, mask, residue_mask=np.array([[0, 1, 1, 1]]), segment_idx=np.array([[2, 2, 2, 1]]), segment=2, group_size=2, L=3)
    assert n.tolist() == [1, 1] and out[1, 0].tolist() == [np.float32(1.2), np.float32(11.2), np.float32(21.2)] and np.isnan(out[:, 1:]).all()


# ------------------------------------------------------------------ tables of loops
def test_dihedral_set_round_trip_and_refusals():
    loops = [[(-60, -45, 180), (None, 120, 175.5)], [], np.array([[NAN, 0.0, 90.0]] * 3), torch.tensor([[10.0, 20.0, 30.0]])]
    s = metrics.dihedral_set(loops, degrees=True)
    assert s.angles.dtype == torch.float32 and tuple(s.angles.shape) == (4, 3, 3) and s.lengths.dtype == torch.int32 and len(s) == 4
    assert s.lengths.tolist() == [2, 0, 3, 1]
    assert s.angles[0, 0].tolist() == [np.float32(math.radians(v)) for v in (-60, -45, 180)]
    assert math.isnan(s.angles[0, 1, 0]) and s.angles[0, 1, 1].item() == np.float32(math.radians(120))
    assert torch.isnan(s.angles[0, 2:]).all() and torch.isnan(s.angles[1]).all() and torch.isnan(s.angles[2, :, 0]).all() and torch.isnan(s.angles[3, 1:]).all()
    radians = metrics.dihedral_set([[(1.0, -2.0, 3.0)]])
    assert radians.angles[0, 0].tolist() == [1.0, -2.0, 3.0] and tuple(radians.angles.shape) == (1, 1, 3)
    empty = metrics.dihedral_set([])
    assert tuple(empty.angles.shape) == (0, 1, 3) and len(empty) == 0
    assert tuple(metrics.dihedral_set([[], []]).angles.shape) == (2, 1, 3)
    assert tuple(metrics.dihedral_set([[(0.0, 0.0, 0.0)] * 64]).angles.shape) == (1, 64, 3)
    with pytest.raises(ValueError, match="loop 0 has 65 residues, at most 64"):
        metrics.dihedral_set([[(0.0, 0.0, 0.0)] * 65])
    with pytest.raises(ValueError, match=r"loop 1 is \(2, 2\), expected \(n, 3\)"):
        metrics.dihedral_set([[(0.0, 0.0, 0.0)], [(0.0, 0.0), (1.0, 1.0)]])
    with pytest.raises(ValueError, match="loop 0 is not an"):
        metrics.dihedral_set([[("a", 0.0, 0.0)]])
    for bad in ("loops", None, 5, torch.zeros(2, 3, 3)):
        with pytest.raises(ValueError, match="loops must be a list"):
            metrics.dihedral_set(bad)
    with pytest.raises(ValueError, match="degrees must be a bool"):
        metrics.dihedral_set([], degrees=1)


@pytest.mark.parametrize("angles, lengths, match", [
    (torch.zeros(2, 3, 3, dtype=torch.float64), torch.zeros(2, dtype=torch.int32), "angles must be a float32 tensor"),
    (torch.zeros(2, 3), torch.zeros(2, dtype=torch.int32), "angles must be a float32 tensor"),
    (torch.zeros(2, 3, 2), torch.zeros(2, dtype=torch.int32), "angles must be a float32 tensor"),
    (np.zeros((2, 3, 3), np.float32), torch.zeros(2, dtype=torch.int32), "angles must be a float32 tensor"),
    (torch.zeros(2, 3, 3), torch.zeros(2, dtype=torch.int64), "lengths must be an int32 tensor"),
    (torch.zeros(2, 3, 3), torch.zeros(3, dtype=torch.int32), r"lengths must be an int32 tensor \(2,\)"),
    (torch.zeros(2, 65, 3), torch.zeros(2, dtype=torch.int32), r"L outside \[1, 64\]"),
    (torch.zeros(2, 0, 3), torch.zeros(2, dtype=torch.int32), r"L outside \[1, 64\]"),
])
def test_dihedral_set_class_refuses(angles, lengths, match):
    with pytest.raises(ValueError, match=r"metrics\.DihedralSet\(\): .*" + match):
        metrics.DihedralSet(angles, lengths)


def test_dihedral_angle_reads_a_distance_as_degrees():
    got = metrics.dihedral_angle(torch.tensor([0.0, 2.0, 4.0, 1.0, 2 * (1 - math.cos(math.radians(25.0)))]))
    assert got.tolist() == pytest.approx([0.0, 90.0, 180.0, 60.0, 25.0], abs=1e-3)
    assert torch.isnan(metrics.dihedral_angle(torch.tensor([5.0, float("inf")]))).all()
    with pytest.raises(ValueError, match="distance must be a float tensor"):
        metrics.dihedral_angle([0.0])


# ------------------------------------------------------------------ the header, the library and the ctypes table
def header_code():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


NEAREST = ["q_feat", "q_len", "R", "LQ", "lib_feat", "lib_len", "M", "LM", "A", "skip", "radius", "min_terms", "distance", "index", "n_terms",
           "n_within", "matrix", "workspace", "workspace_bytes", "stream"]
PACK = ["phi", "psi", "omega", "mask", "residue_mask", "segment_idx", "segment", "rows", "group_size", "K", "L", "out_angles", "out_len", "stream"]


def test_header_library_and_symbol_table_agree():
    """Every entry the header declares is in _hip.CONFORMATION_SYMBOLS with the same arity and kinds, is exported, and is typed by
    load_library(); nothing else is in the table, and the table shares no name with the eight older ones."""
    code = header_code()
    protos = dict(re.findall(r"\bint\s+(diffab_[a-z0-9_]+)\s*\((.*?)\)\s*;", code, flags=re.S))
    declared = sorted(set(re.findall(r"\b(diffab_[a-z0-9_]+)\s*\(", code)))
    assert declared == sorted(protos) == ["diffab_metrics_dihedral_nearest", "diffab_metrics_pack_dihedrals"]
    assert sorted(_hip.CONFORMATION_SYMBOLS) == declared, "CONFORMATION_SYMBOLS and include/diffab_hip_conformation.h drifted apart"
    older = (set(_hip.SYMBOLS) | set(_hip.ANALYSIS_SYMBOLS) | set(_hip.HBOND_SYMBOLS) | set(_hip.CLUSTER_SYMBOLS) | set(_hip.INTERFACE_SYMBOLS)
             | set(_hip.DEVELOP_SYMBOLS) | set(_hip.ENERGY_SYMBOLS) | set(_hip.NOVELTY_SYMBOLS))
    assert not set(_hip.CONFORMATION_SYMBOLS) & older
    raw = ctypes.CDLL(_hip.LIB_PATH)
    typed = _hip.load_library()
    kinds = {"int32_t": ctypes.c_int32, "size_t": ctypes.c_size_t, "float": ctypes.c_float}
    for name, proto in protos.items():
        assert hasattr(raw, name), f"{name} is declared in include/diffab_hip_conformation.h but not exported by libdiffab_hip.so"
        res, args = _hip.CONFORMATION_SYMBOLS[name]
        fn = getattr(typed, name)
        assert fn.restype is res and list(fn.argtypes) == args  # load_library() types the ninth table onto the same CDLL object
        params = [" ".join(p.split()) for p in proto.split(",")]
        assert res is ctypes.c_int and len(args) == len(params), name
        for p, a in zip(params, args):
            kind = p.rsplit(" ", 1)[0]
            if kind in kinds:
                assert a is kinds[kind], (name, p)
            else:
                assert "*" in kind and a is ctypes.c_void_p, (name, p)
    names = lambda entry: [" ".join(p.split()).rsplit(" ", 1)[1].lstrip("*") for p in protos[entry].split(",")]
    assert names("diffab_metrics_dihedral_nearest") == NEAREST and names("diffab_metrics_pack_dihedrals") == PACK
    text = open(HEADER).read()
    assert '#include "diffab_hip.h"' in text and "Why a header of its own" in text.split("*/")[0] and "applies word for word" in text.split("*/")[0]
    for macro, value in (("DIFFAB_CONFORMATION_MAX_LENGTH", metrics.CONFORMATION_MAX_LENGTH), ("DIFFAB_CONFORMATION_MAX_ANGLES", len(metrics.DIHEDRALS)),
                         ("DIFFAB_CONFORMATION_CHUNK", metrics.CONFORMATION_CHUNK)):
        assert int(re.search(rf"#define\s+{macro}\s+(\d+)", code).group(1)) == value
    assert metrics.CONFORMATION_MAX_LENGTH == 64 and metrics.DIHEDRALS == ("phi", "psi", "omega")


SHAPES = [(1, 1, 1, 1, 1), (1, 1, 64, 64, 3), (16, 17, 5, 7, 2), (65, 4097, 33, 64, 3), (3, 2049, 30, 16, 1), (16384, 100000, 16, 30, 2),
          (16384, 1000000, 16, 30, 2), (5, 40000000, 64, 64, 3), (7, 0, 9, 9, 2)]
MACRO_C = r"""
#include <stdio.h>
#include "diffab_hip_conformation.h"
int main(void) {
%s
  printf("%%d %%d %%d %%d %%d\n", DIFFAB_ERR_ARG, DIFFAB_ERR_WORKSPACE, DIFFAB_CONFORMATION_MAX_LENGTH, DIFFAB_CONFORMATION_MAX_ANGLES, DIFFAB_CONFORMATION_CHUNK);
  return 0;
}
"""


def test_workspace_macro_equals_the_python_mirror(tmp_path):
    """The header compiles as C on its own (it brings diffab_hip.h along) and its macro gives metrics.dihedral_nearest_workspace_bytes."""
    cc = shutil.which("cc") or shutil.which("gcc") or next((p for p in ("/opt/rocm/llvm/bin/clang",) if os.path.exists(p)), None)
    assert cc, "no C compiler to read the header's macros with"
    src, exe = tmp_path / "macro.c", tmp_path / "macro"
    src.write_text(MACRO_C % "\n".join(f'  printf("%zu\\n", DIFFAB_METRICS_DIHEDRAL_NEAREST_WORKSPACE_BYTES({R}, {M}, {LQ}, {LM}, {A}));' for R, M, LQ, LM, A in SHAPES))
    subprocess.run([cc, "-std=c99", "-Wall", "-Werror", "-I", os.path.join(REPO, "include"), str(src), "-o", str(exe)], check=True)
    got = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()
    want = [metrics.dihedral_nearest_workspace_bytes(*s) for s in SHAPES]
    assert [int(v) for v in got[:len(want)]] == want
    assert got[len(want):] == ["-1", "-4", "64", "3", "2048"]
    side = lambda n, L, A: (n + 15) // 16 * ((2 * A * L + 3) // 4 * 4) * 16 * 4 + n * A * 8 + n * 8 + n * 4 + (n + 2047) // 2048 * 65 * 4
    assert metrics.dihedral_nearest_workspace_bytes(65, 4097, 33, 64, 3) == side(65, 33, 3) + side(4097, 64, 3) + 3 * 65 * 12 + 8192
    assert metrics.dihedral_nearest_workspace_bytes(1, 1, 1, 1, 1) == 2 * (256 + 20 + 260) + 12 + 8192
    assert metrics.dihedral_nearest_workspace_bytes(5, 40000000, 64, 64, 3) > 1 << 32


def test_host_side_refusals_touch_no_gpu():
    """Every refusal is decided from the scalar arguments and whether a pointer is null: the device pointers are fake addresses that
    are never dereferenced, nothing is enqueued (no GPU is needed), and diffab_last_error names the problem."""
    l = _hip.load_library()
    p, null = ctypes.c_void_p(4096), ctypes.c_void_p(0)
    err = lambda: l.diffab_last_error().decode()
    ins, outs = ("q_feat", "q_len", "lib_feat", "lib_len", "skip"), ("distance", "index", "n_terms", "n_within", "matrix")

    def nearest(R=6, LQ=20, M=40, LM=30, A=2, radius=0.5, min_terms=1, ws=p, ws_bytes=1 << 40, **ptrs):
        a = dict.fromkeys(ins + outs, p)
        a.update(ptrs)
        return l.diffab_metrics_dihedral_nearest(a["q_feat"], a["q_len"], R, LQ, a["lib_feat"], a["lib_len"], M, LM, A, a["skip"], radius, min_terms,
                                                 *[a[k] for k in outs], ws, ws_bytes, null)

    for kw, word in ((dict(R=-1), "negative extent"), (dict(M=-1), "negative extent"), (dict(LQ=0), "LQ = 0"), (dict(LQ=65), "LQ = 65 slots per query outside [1, 64]"),
                     (dict(LM=0), "LM = 0"), (dict(LM=65), "LM = 65 slots per library entry outside [1, 64]"), (dict(A=0), "A = 0 angles per slot outside [1, 3]"),
                     (dict(A=4), "A = 4"), (dict(min_terms=0), "min_terms = 0, at least 1"), (dict(min_terms=-3), "min_terms = -3"),
                     (dict(q_feat=null), "null input (q_feat, q_len)"), (dict(q_len=null), "null input (q_feat, q_len)"),
                     (dict(lib_feat=null), "null input (lib_feat, lib_len)"), (dict(lib_len=null), "null input (lib_feat, lib_len)"),
                     (dict(R=1 << 16, M=1 << 15), "fewer than 2^31"), (dict(R=2 ** 31 - 1, M=2 ** 31 - 1), "fewer than 2^31"), (dict(ws=null), "workspace"),
                     (dict(ws=ctypes.c_void_p(4096 + 16)), "256-byte aligned")):
        rc = nearest(**kw)
        assert rc == -1 and word in err() and err().startswith("metrics_dihedral_nearest:"), (kw, rc, err())
    need = metrics.dihedral_nearest_workspace_bytes(6, 40, 20, 30, 2)
    assert nearest(ws_bytes=need // 2) == -4 and "needed" in err() and err().startswith("metrics_dihedral_nearest:")  # DIFFAB_ERR_WORKSPACE
    assert need - 8192 <= int(re.search(r"(\d+) needed", err()).group(1)) <= need
    big = (65, 4097, 33, 64, 3)
    assert nearest(R=65, M=4097, LQ=33, LM=64, A=3, ws_bytes=16) == -4
    assert metrics.dihedral_nearest_workspace_bytes(*big) - 8192 <= int(re.search(r"(\d+) needed", err()).group(1)) <= metrics.dihedral_nearest_workspace_bytes(*big)
    ok = [dict(LQ=1), dict(LQ=64), dict(LM=1), dict(LM=64), dict(A=1), dict(A=3), dict(radius=-5.0), dict(radius=float("nan")), dict(min_terms=2 ** 31 - 1),
          dict(skip=null), dict.fromkeys(outs, null), dict(R=1 << 16, M=1 << 15, matrix=null), dict(R=(1 << 16) - 1, M=1 << 15), dict(R=1, M=1)]
    for kw in ok:  # accepted as far as the workspace check, the last one before the launches (M = 0 would go on to launch: the GPU tests have it)
        assert nearest(ws_bytes=16, **kw) == -4 and "needed" in err(), kw
    assert l.diffab_metrics_dihedral_nearest(null, null, 0, 20, null, null, 40, 30, 2, null, 0.5, 1, *[null] * 5, null, 0, null) == 0  # R = 0: no pointer is read

    def pack(segment=1, rows=6, group=3, K=40, L=16, **ptrs):
        a = dict.fromkeys(("phi", "psi", "omega", "mask", "residue_mask", "segment_idx", "out_angles", "out_len"), p)
        a.update(ptrs)
        return l.diffab_metrics_pack_dihedrals(a["phi"], a["psi"], a["omega"], a["mask"], a["residue_mask"], a["segment_idx"], segment, rows, group, K, L,
                                               a["out_angles"], a["out_len"], null)

    for kw, word in ((dict(rows=-1), "extent"), (dict(group=0), "extent"), (dict(K=0), "extent"), (dict(group=4097, rows=4097), "at most 4096 designs"),
                     (dict(K=4097), "K = 4097 residues per patch, at most 4096"), (dict(rows=7), "not a multiple"), (dict(L=0), "L = 0"),
                     (dict(L=65), "L = 65 slots per loop outside [1, 64]"), (dict(phi=null), "null input (phi, psi, omega, mask)"),
                     (dict(psi=null), "null input"), (dict(omega=null), "null input"), (dict(mask=null), "null input (phi, psi, omega, mask)")):
        rc = pack(**kw)
        assert rc == -1 and word in err() and err().startswith("metrics_pack_dihedrals:"), (kw, rc, err())
    assert pack(rows=0, phi=null, psi=null, omega=null, mask=null, out_angles=null, out_len=null) == 0  # an empty problem: no pointer is read
    assert pack(out_angles=null, out_len=null) == 0  # nothing to write: nothing is enqueued


# ------------------------------------------------------------------ Python argument errors before any device work
@pytest.fixture
def no_library(monkeypatch):
    refuse_library(monkeypatch)


def sets():
    return (metrics.dihedral_set([[(1.0, 2.0, 3.0)] * 4, [(0.0, 0.0, 0.0)] * 2]),
            metrics.dihedral_set([[(1.0, 2.0, 3.0)] * 4, [], [(0.5, 0.5, 0.5)] * 7]))


def designs_of(rows=4, K=8):
    return {"seq_idx": torch.zeros(rows, K, dtype=torch.long), "translations": torch.zeros(rows, K, 3),
            "orientations": torch.eye(3).expand(rows, K, 3, 3).contiguous()}


def gen_of(G=2, K=8):
    gm = torch.zeros(G, K, dtype=torch.bool)
    gm[:, 2:6] = True
    return gm


def test_good_arguments_reach_the_library(no_library):
    q, lib = sets()
    for kw in ({}, dict(radius=0.0), dict(radius=-1), dict(radius=float("nan")), dict(matrix=True), dict(exclude=torch.tensor([0, 7])),
               dict(exclude=torch.tensor([-1, 2], dtype=torch.int32)), dict(angles=("omega",)), dict(angles=["psi", "phi"]), dict(angles=metrics.DIHEDRALS),
               dict(labels=torch.tensor([3, 1, 2])), dict(min_terms=5)):
        with pytest.raises(ReachedTheLibrary):
            metrics.conformation(q, lib, **kw)
    with pytest.raises(ReachedTheLibrary):
        metrics.conformation(q, q, exclude="self", radius=0.5)
    with pytest.raises(ReachedTheLibrary):
        metrics.conformation(q, metrics.dihedral_set([]))
    seg = torch.zeros(2, 8, dtype=torch.long)
    for kw in ({}, dict(group_size=2), dict(group_size=1, generation_mask=gen_of(4)), dict(residue_mask=torch.ones(2, 8, dtype=torch.bool)),
               dict(segment_idx=seg, segment=0), dict(max_length=4), dict(max_length=64), dict(chain_idx=torch.zeros(8, dtype=torch.long)),
               dict(residue_idx=torch.arange(8))):
        with pytest.raises(ReachedTheLibrary):
            metrics.design_dihedrals(**{**dict(designs=designs_of(), generation_mask=gen_of(), group_size=2), **kw})


@pytest.mark.parametrize("kw, match", [
    (dict(queries=torch.zeros(2, 3, 3)), "queries must be a metrics.DihedralSet"),
    (dict(library=[[(0.0, 0.0, 0.0)]]), "library must be a metrics.DihedralSet"),
    (dict(angles=()), "angles must be a non-empty subset"), (dict(angles="phi"), "angles must be a non-empty subset"),
    (dict(angles=("phi", "chi")), "angles must be a non-empty subset"), (dict(angles=("phi", "phi")), "without repeats"),
    (dict(radius="1"), "radius must be a float or None"), (dict(radius=True), "radius must be a float or None"),
    (dict(matrix=1), "matrix must be a bool"), (dict(min_terms=0), "min_terms must be an int >= 1"), (dict(min_terms=1.0), "min_terms must be an int"),
    (dict(exclude="others"), "exclude must be an integer tensor"),
    (dict(exclude="self"), "exclude='self' needs as many queries as library entries, got R = 2 and M = 3"),
    (dict(exclude=torch.zeros(3, dtype=torch.long)), r"exclude must be an integer tensor \(2,\)"), (dict(exclude=torch.zeros(2)), "exclude must be an integer tensor"),
    (dict(exclude=[0, 1]), "exclude must be an integer tensor"),
    (dict(labels=torch.zeros(2, dtype=torch.long)), r"labels must be an integer tensor \(3,\)"), (dict(labels=torch.zeros(3)), "labels must be an integer tensor"),
    (dict(labels=[1, 2, 3]), "labels must be an integer tensor"),
])
def test_conformation_argument_errors(no_library, kw, match):
    q, lib = sets()
    args = dict(queries=q, library=lib)
    args.update(kw)
    with pytest.raises(ValueError, match=r"metrics\.conformation\(\): .*" + match):
        metrics.conformation(args.pop("queries"), args.pop("library"), **args)


@pytest.mark.parametrize("kw, match", [
    (dict(designs={"seq_idx": torch.zeros(4, 8, dtype=torch.long)}), "designs must be a dict with seq_idx and translations"),
    (dict(designs={"seq_idx": torch.zeros(4, 8, dtype=torch.long), "translations": torch.zeros(4, 8, 3)}), r"designs\['orientations'\] must be a float tensor"),
    (dict(group_size=3), "4 design rows are not a multiple of group_size = 3"), (dict(group_size=0), "group_size must be an int >= 1"),
    (dict(generation_mask=torch.ones(2, 8)), "generation_mask must be a bool tensor"), (dict(generation_mask=gen_of(4)), "generation_mask is"),
    (dict(residue_mask=torch.ones(2, 7, dtype=torch.bool)), "residue_mask is"),
    (dict(chain_idx=torch.zeros(8)), "needs an integer chain_idx"), (dict(residue_idx=torch.arange(7)), "residue_idx"),
    (dict(segment=1), "segment_idx and segment go together, segment_idx is missing"),
    (dict(segment_idx=torch.zeros(2, 8, dtype=torch.long)), "segment_idx and segment go together, segment is missing"),
    (dict(segment_idx=torch.zeros(2, 8), segment=0), "segment_idx must be an integer tensor"),
    (dict(segment_idx=torch.zeros(4, 8, dtype=torch.long), segment=0), r"segment_idx must be an integer tensor \(2, 8\)"),
    (dict(segment_idx=torch.zeros(2, 8, dtype=torch.long), segment=0.0), "segment must be an int"),
    (dict(max_length=0), r"max_length must be an int in \[1, 64\]"), (dict(max_length=65), "max_length must be an int"), (dict(max_length=8.0), "max_length must be an int"),
    (dict(max_length=3), "patch 0 has 4 counted residues, more than max_length = 3"),
    (dict(max_length=4, generation_mask=torch.cat([gen_of(1), torch.ones(1, 8, dtype=torch.bool)])), "patch 1 has 8 counted residues, more than max_length = 4"),
])
def test_design_dihedrals_argument_errors(no_library, kw, match):
    args = dict(designs=designs_of(), generation_mask=gen_of(), group_size=2)
    args.update(kw)
    with pytest.raises(ValueError, match=r"metrics\.design_dihedrals\(\): .*" + match):
        metrics.design_dihedrals(**args)


def test_signatures_constants_and_documents():
    sig = inspect.signature(metrics.conformation)
    assert list(sig.parameters) == ["queries", "library", "angles", "radius", "exclude", "matrix", "labels", "min_terms"]
    assert all(sig.parameters[k].kind is inspect.Parameter.KEYWORD_ONLY for k in list(sig.parameters)[2:])
    assert [sig.parameters[k].default for k in list(sig.parameters)[2:]] == [("phi", "psi"), None, None, False, None, 1]
    sig = inspect.signature(metrics.design_dihedrals)
    assert list(sig.parameters) == ["designs", "generation_mask", "group_size", "chain_idx", "residue_idx", "residue_mask", "segment_idx", "segment", "max_length"]
    assert all(sig.parameters[k].kind is inspect.Parameter.KEYWORD_ONLY for k in list(sig.parameters)[2:])
    assert [sig.parameters[k].default for k in list(sig.parameters)[2:]] == [1, None, None, None, None, None, 64]
    assert list(inspect.signature(metrics.DihedralSet).parameters) == ["angles", "lengths"]
    assert list(inspect.signature(metrics.dihedral_set).parameters) == ["loops", "degrees"]
    for word in ("``conformation``", "``DihedralSet``", "``dihedral_set``", "``design_dihedrals``", "``dihedral_angle``", "conformation_kernels.hip",
                 "include/diffab_hip_conformation.h"):
        assert word in metrics.__doc__, word
    doc = " ".join(metrics.conformation.__doc__.split())
    for word in ("``label`` where ``distance <= cutoff``", "``distance > cutoff``", ".view(1, N, N)", "cluster", "``2 * d``"):
        assert word in doc, word
    readme, design, integration = (open(os.path.join(REPO, f)).read() for f in ("README.md", "DESIGN.md", "INTEGRATION.md"))
    assert "Which ones have a known shape" in readme and "### 4.27" in design
    for word in ("metrics.conformation", "metrics.design_dihedrals", "metrics.dihedral_set", "diffab_metrics_dihedral_nearest", "diffab_metrics_pack_dihedrals"):
        assert word in readme and word in design, word
    for word in ("`conformation_ref.py`", "`test_conformation_host.py`", "`test_gpu_conformation.py`", "`conformation_bench.py`", "`profiles/conformation.md`",
                 "`include/diffab_hip_conformation.h`"):
        assert word in readme, word
    for word in ("Suggested and not adopted", "VGPR", "no scratch", "2 (n_k + 2) u"):
        assert word in design.split("### 4.27")[1], word
    assert "diffab_hip_conformation.h" in integration and "conformation_kernels.hip" in design
    makefile = open(os.path.join(REPO, "diffab-pytorch_amd", "csrc", "Makefile")).read()
    assert "$(OBJ)/conformation_kernels.o" in re.search(r"DEFINED_OBJS := (.*)", makefile).group(1) and "the loop conformations" in makefile
