"""Design novelty without a GPU: the restatement of novelty_ref.py on hand-made cases with the answers written
out, sequence_set / sequence_strings, the header / library / ctypes table of include/diffab_hip_novelty.h, its workspace macro against
the Python mirror, every host-side refusal of the two entries, and metrics.novelty / metrics.design_sequences argument errors."""
import ctypes
import inspect
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

from conftest import REPO
from diffab_pytorch import _hip, io as dio, metrics
from novelty_ref import PAD, edit_matrix, nearest_ref, pack_ref
from sampler_support import ReachedTheLibrary, refuse_library

HEADER = os.path.join(REPO, "include", "diffab_hip_novelty.h")
enc = lambda s: [dio.AA1.index(c) for c in s]


def rows_of(seqs):
    """(tokens (n, L), lengths (n)) of token lists, padded with 255."""
    L = max([len(s) for s in seqs] + [1])
    return np.array([list(s) + [PAD] * (L - len(s)) for s in seqs], np.int64).reshape(len(seqs), L), np.array([len(s) for s in seqs])


def d(a, b):
    (qa, na), (lb, nb) = rows_of([a]), rows_of([b])
    return int(edit_matrix(qa, na, lb, nb)[0, 0])


# ------------------------------------------------------------------ the restatement, by hand
def test_hand_made_distances():
    assert d(enc("ARND"), enc("ARD")) == 1  # one deletion
    assert d([], enc("ARN")) == 3 and d(enc("ARN"), []) == 3 and d([], []) == 0
    assert d(enc("CARDYW"), enc("CARDYW")) == 0
    assert d([40], [40]) == 1 and d([32], [32]) == 1 and d([31], [31]) == 0  # a token of 32 or more matches nothing, itself included
    assert d([3, 40, 5], [3, 40, 5]) == 1 and d([255], []) == 1
    assert d(enc("ARDYW"), enc("GARDY")) == 2  # a motif one register on: one insertion in front, one deletion behind, where
    assert sum(a != b for a, b in zip("ARDYW", "GARDY")) == 5  # identity by position sees nothing in common
    assert d(enc("CARDYW"), enc("CARGDYW")) == 1 and d(enc("KITTEN"), enc("SITTING")) == 3
    assert d(enc("A" * 64), enc("A" * 65)) == 1 and d(enc("A" * 64), enc("A" * 33)) == 31 and d(enc("A" * 64), enc("R" * 256)) == 256


def test_lengths_are_clamped_and_bytes_behind_them_are_not_read():
    q, _ = rows_of([enc("ARND")])
    lib, _ = rows_of([enc("ARNDAR")])
    assert edit_matrix(q, [9], lib, [4])[0, 0] == 0 and edit_matrix(q, [4], lib, [100])[0, 0] == 2 and edit_matrix(q, [-2], lib, [-1])[0, 0] == 0
    assert edit_matrix(q, [2], lib, [6])[0, 0] == 4 and edit_matrix(q, [3], lib, [3])[0, 0] == 0


def test_per_query_outputs_of_the_restatement():
    q, nq = rows_of([enc("ARND"), enc("WW"), []])
    lib, nl = rows_of([enc("ARD"), enc("ARNDC"), enc("ARN"), enc("W")])
    out = nearest_ref(q, nq, lib, nl, radius=1)
    assert out["matrix"].tolist() == [[1, 1, 1, 4], [3, 5, 3, 1], [3, 5, 3, 1]]
    assert out["distance"].tolist() == [1, 1, 1] and out["index"].tolist() == [0, 3, 3]  # ties go to the lower index
    assert out["n_within"].tolist() == [3, 1, 1]
    assert out["identity"].tolist() == [np.float32(1) - np.float32(1) / np.float32(4), np.float32(0.5), np.float32(0.0)]
    out = nearest_ref(q, nq, lib, nl, skip=[0, 3, 9], radius=-1)
    assert out["distance"].tolist() == [1, 3, 1] and out["index"].tolist() == [1, 0, 3] and out["n_within"].tolist() == [0, 0, 0]
    assert out["identity"].dtype == np.float32 and out["identity"][0] == np.float32(1) - np.float32(1) / np.float32(5)
    one = nearest_ref(q, nq, lib[:1], nl[:1], skip=[0, 0, 5], radius=9)
    assert one["distance"].tolist() == [-1, -1, 3] and one["index"].tolist() == [-1, -1, 0] and one["n_within"].tolist() == [0, 0, 1]
    assert np.isnan(one["identity"][:2]).all() and one["identity"][2] == 0 and one["matrix"].tolist() == [[1], [3], [3]]
    none = nearest_ref(q, nq, np.zeros((0, 5), np.int64), [], radius=3)
    assert none["distance"].tolist() == [-1] * 3 and np.isnan(none["identity"]).all() and none["matrix"].shape == (3, 0)
    both_empty = nearest_ref(*rows_of([[]]), *rows_of([[]]))
    assert both_empty["distance"].tolist() == [0] and both_empty["identity"].tolist() == [1.0]


def test_pack_restatement():
    tokens = np.array([[5, -1, 7, 300, 254, 255], [1, 2, 3, 4, 5, 6]])
    mask = np.array([[1, 1, 0, 1, 1, 1]])
    out, n = pack_ref(tokens, mask, group_size=2, L=4)
    assert out.tolist() == [[5, 255, 255, 254], [1, 2, 4, 5]] and n.tolist() == [5, 5]
    out, n = pack_ref(tokens, mask, residue_mask=np.array([[0, 1, 1, 1, 1, 1]]), segment_idx=np.array([[2, 2, 2, 1, 2, 1]]), segment=2, group_size=2, L=3)
    assert out.tolist() == [[255, 254, 255], [2, 5, 255]] and n.tolist() == [2, 2]


# ------------------------------------------------------------------ strings
def test_sequence_set_round_trip_and_refusals():
    strings = ["ARDYW", "", "CARDYWGQGTLVTVSS", "X", dio.AA1]
    s = metrics.sequence_set(strings)
    assert s.tokens.dtype == torch.uint8 and tuple(s.tokens.shape) == (5, 21) and s.lengths.dtype == torch.int32 and len(s) == 5
    assert s.lengths.tolist() == [5, 0, 16, 1, 21] and s.tokens[0].tolist() == enc("ARDYW") + [255] * 16 and s.tokens[4].tolist() == list(range(21))
    assert metrics.sequence_strings(s) == strings
    t = s.tokens.clone()
    t[0, 1], t[0, 2] = 21, 255
    assert metrics.sequence_strings(metrics.SequenceSet(t, torch.tensor([5, -3, 400, 1, 21], dtype=torch.int32)))[:3] == ["A??YW", "", "CARDYWGQGTLVTVSS?????"]
    empty = metrics.sequence_set([])
    assert tuple(empty.tokens.shape) == (0, 1) and len(empty) == 0 and metrics.sequence_strings(empty) == []
    assert tuple(metrics.sequence_set(["", ""]).tokens.shape) == (2, 1)
    assert tuple(metrics.sequence_set(["A" * 256]).tokens.shape) == (1, 256)
    with pytest.raises(ValueError, match=r"string 1 \('ARBD'\) has the letter 'B'"):
        metrics.sequence_set(["ARD", "ARBD"])
    with pytest.raises(ValueError, match="letter 'a'"):
        metrics.sequence_set(["a"])
    with pytest.raises(ValueError, match="string 0 has 257 letters, at most 256"):
        metrics.sequence_set(["A" * 257])
    for bad in ("ARD", [1, 2], None, ["A", b"R"]):
        with pytest.raises(ValueError, match="strings must be a list of str"):
            metrics.sequence_set(bad)
    with pytest.raises(ValueError, match="must be a metrics.SequenceSet"):
        metrics.sequence_strings(["ARD"])


@pytest.mark.parametrize("tokens, lengths, match", [
    (torch.zeros(2, 3, dtype=torch.int32), torch.zeros(2, dtype=torch.int32), "tokens must be a uint8 tensor"),
    (torch.zeros(6, dtype=torch.uint8), torch.zeros(6, dtype=torch.int32), "tokens must be a uint8 tensor"),
    (np.zeros((2, 3), np.uint8), torch.zeros(2, dtype=torch.int32), "tokens must be a uint8 tensor"),
    (torch.zeros(2, 3, dtype=torch.uint8), torch.zeros(2, dtype=torch.int64), "lengths must be an int32 tensor"),
    (torch.zeros(2, 3, dtype=torch.uint8), torch.zeros(3, dtype=torch.int32), r"lengths must be an int32 tensor \(2,\)"),
    (torch.zeros(2, 257, dtype=torch.uint8), torch.zeros(2, dtype=torch.int32), r"L outside \[1, 256\]"),
    (torch.zeros(2, 0, dtype=torch.uint8), torch.zeros(2, dtype=torch.int32), r"L outside \[1, 256\]"),
])
def test_sequence_set_refuses(tokens, lengths, match):
    with pytest.raises(ValueError, match=r"metrics\.SequenceSet\(\): .*" + match):
        metrics.SequenceSet(tokens, lengths)


# ------------------------------------------------------------------ the header, the library and the ctypes table
def header_code():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


NEAREST = ["q_tokens", "q_len", "R", "LQ", "lib_tokens", "lib_len", "M", "LM", "skip", "radius", "distance", "index", "n_within", "identity",
           "matrix", "workspace", "workspace_bytes", "stream"]
PACK = ["tokens", "mask", "residue_mask", "segment_idx", "segment", "rows", "group_size", "K", "L", "out_tokens", "out_len", "stream"]


def test_header_library_and_symbol_table_agree():
    """Every entry the header declares is in _hip.NOVELTY_SYMBOLS with the same arity and kinds, is exported, and is typed by
    load_library(); nothing else is in the table, and the table shares no name with the seven older ones."""
    code = header_code()
    protos = dict(re.findall(r"\bint\s+(diffab_[a-z0-9_]+)\s*\((.*?)\)\s*;", code, flags=re.S))
    declared = sorted(set(re.findall(r"\b(diffab_[a-z0-9_]+)\s*\(", code)))
    assert declared == sorted(protos) == ["diffab_metrics_edit_nearest", "diffab_metrics_pack_sequences"]
    assert sorted(_hip.NOVELTY_SYMBOLS) == declared, "NOVELTY_SYMBOLS and include/diffab_hip_novelty.h drifted apart"
    older = (set(_hip.SYMBOLS) | set(_hip.ANALYSIS_SYMBOLS) | set(_hip.HBOND_SYMBOLS) | set(_hip.CLUSTER_SYMBOLS) | set(_hip.INTERFACE_SYMBOLS)
             | set(_hip.DEVELOP_SYMBOLS) | set(_hip.ENERGY_SYMBOLS))
    assert not set(_hip.NOVELTY_SYMBOLS) & older
    raw = ctypes.CDLL(_hip.LIB_PATH)
    typed = _hip.load_library()
    kinds = {"int32_t": ctypes.c_int32, "size_t": ctypes.c_size_t}
    for name, proto in protos.items():
        assert hasattr(raw, name), f"{name} is declared in include/diffab_hip_novelty.h but not exported by libdiffab_hip.so"
        res, args = _hip.NOVELTY_SYMBOLS[name]
        fn = getattr(typed, name)
        assert fn.restype is res and list(fn.argtypes) == args  # load_library() types the eighth table onto the same CDLL object
        params = [" ".join(p.split()) for p in proto.split(",")]
        assert res is ctypes.c_int and len(args) == len(params), name
        for p, a in zip(params, args):
            kind = p.rsplit(" ", 1)[0]
            if kind in kinds:
                assert a is kinds[kind], (name, p)
            else:
                assert "*" in kind and a is ctypes.c_void_p, (name, p)
    names = lambda entry: [" ".join(p.split()).rsplit(" ", 1)[1].lstrip("*") for p in protos[entry].split(",")]
    assert names("diffab_metrics_edit_nearest") == NEAREST and names("diffab_metrics_pack_sequences") == PACK
    text = open(HEADER).read()
    assert '#include "diffab_hip.h"' in text and "Why a header of its own" in text.split("*/")[0] and "applies word for word" in text.split("*/")[0]
    for macro, value in (("DIFFAB_NOVELTY_MAX_QUERY", metrics.NOVELTY_MAX_QUERY), ("DIFFAB_NOVELTY_MAX_LIBRARY", metrics.NOVELTY_MAX_LIBRARY),
                         ("DIFFAB_NOVELTY_CHUNK", metrics.NOVELTY_CHUNK), ("DIFFAB_NOVELTY_PACK_MAX_K", metrics.MAX_K)):
        assert int(re.search(rf"#define\s+{macro}\s+(\d+)", code).group(1)) == value
    assert (metrics.NOVELTY_MAX_QUERY, metrics.NOVELTY_MAX_LIBRARY, metrics.NOVELTY_PAD) == (64, 256, 255)


SHAPES = [(1, 1, 1), (1, 1, 4), (1, 2048, 5), (3, 2049, 30), (65, 4097, 256), (16384, 100000, 30), (16384, 1000000, 30), (5, 40000000, 130)]
MACRO_C = r"""
#include <stdio.h>
#include "diffab_hip_novelty.h"
int main(void) {
%s
  printf("%%d %%d %%d %%d %%d\n", DIFFAB_ERR_ARG, DIFFAB_ERR_WORKSPACE, DIFFAB_NOVELTY_MAX_QUERY, DIFFAB_NOVELTY_MAX_LIBRARY, DIFFAB_NOVELTY_CHUNK);
  return 0;
}
"""


def test_workspace_macro_equals_the_python_mirror(tmp_path):
    """The header compiles as C on its own (it brings diffab_hip.h along) and its macro gives metrics.edit_nearest_workspace_bytes."""
    cc = shutil.which("cc") or shutil.which("gcc") or next((p for p in ("/opt/rocm/llvm/bin/clang",) if os.path.exists(p)), None)
    assert cc, "no C compiler to read the header's macros with"
    src, exe = tmp_path / "macro.c", tmp_path / "macro"
    src.write_text(MACRO_C % "\n".join(f'  printf("%zu\\n", DIFFAB_METRICS_EDIT_NEAREST_WORKSPACE_BYTES({R}, {M}, {LM}));' for R, M, LM in SHAPES))
    subprocess.run([cc, "-std=c99", "-Wall", "-Werror", "-I", os.path.join(REPO, "include"), str(src), "-o", str(exe)], check=True)
    got = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()
    want = [metrics.edit_nearest_workspace_bytes(*s) for s in SHAPES]
    assert [int(v) for v in got[:len(want)]] == want
    assert got[len(want):] == ["-1", "-4", "64", "256", "2048"]
    assert metrics.edit_nearest_workspace_bytes(1, 1, 1) == 12 + 12 + 1024 and metrics.edit_nearest_workspace_bytes(65, 4097, 256) == 4097 * 264 + 3 * 65 * 12 + 1024
    assert metrics.edit_nearest_workspace_bytes(5, 40000000, 130) > 1 << 32 and metrics.edit_nearest_workspace_bytes(7, 0, 30) == 1024


def test_host_side_refusals_touch_no_gpu():
    """Every refusal is decided from the scalar arguments and whether a pointer is null: the device pointers are fake addresses that
    are never dereferenced, nothing is enqueued (no GPU is needed), and diffab_last_error names the problem."""
    l = _hip.load_library()
    p, null = ctypes.c_void_p(4096), ctypes.c_void_p(0)
    err = lambda: l.diffab_last_error().decode()
    ins, outs = ("q_tokens", "q_len", "lib_tokens", "lib_len", "skip"), ("distance", "index", "n_within", "identity", "matrix")

    def nearest(R=6, LQ=20, M=40, LM=30, radius=2, ws=p, ws_bytes=1 << 40, **ptrs):
        a = dict.fromkeys(ins + outs, p)
        a.update(ptrs)
        return l.diffab_metrics_edit_nearest(a["q_tokens"], a["q_len"], R, LQ, a["lib_tokens"], a["lib_len"], M, LM, a["skip"], radius,
                                             *[a[k] for k in outs], ws, ws_bytes, null)

    for kw, word in ((dict(R=-1), "negative extent"), (dict(M=-1), "negative extent"), (dict(LQ=0), "LQ = 0"), (dict(LQ=65), "LQ = 65 tokens per query outside [1, 64]"),
                     (dict(LM=0), "LM = 0"), (dict(LM=257), "LM = 257 tokens per library entry outside [1, 256]"), (dict(q_tokens=null), "null input (q_tokens, q_len)"),
                     (dict(q_len=null), "null input (q_tokens, q_len)"), (dict(lib_tokens=null), "null input (lib_tokens, lib_len)"),
                     (dict(lib_len=null), "null input (lib_tokens, lib_len)"), (dict(R=1 << 16, M=1 << 15), "fewer than 2^31"),
                     (dict(R=2 ** 31 - 1, M=2 ** 31 - 1), "fewer than 2^31"), (dict(ws=null), "workspace"), (dict(ws=ctypes.c_void_p(4096 + 16)), "256-byte aligned")):
        rc = nearest(**kw)
        assert rc == -1 and word in err() and err().startswith("metrics_edit_nearest:"), (kw, rc, err())
    need = metrics.edit_nearest_workspace_bytes(6, 40, 30)
    assert nearest(ws_bytes=need // 2) == -4 and "needed" in err() and err().startswith("metrics_edit_nearest:")  # DIFFAB_ERR_WORKSPACE
    assert need - 1024 <= int(re.search(r"(\d+) needed", err()).group(1)) <= need
    big = (3, 2049, 30)
    assert nearest(R=3, M=2049, ws_bytes=16) == -4 and metrics.edit_nearest_workspace_bytes(*big) - 1024 <= int(re.search(r"(\d+) needed", err()).group(1)) <= metrics.edit_nearest_workspace_bytes(*big)
    ok = [dict(LQ=1), dict(LQ=64), dict(LM=1), dict(LM=256), dict(radius=-5), dict(radius=2 ** 31 - 1), dict(skip=null), dict.fromkeys(outs, null),
          dict(R=1 << 16, M=1 << 15, matrix=null), dict(R=(1 << 16) - 1, M=1 << 15), dict(R=1, M=1)]  # (M = 0 needs no workspace and would go on to launch: the GPU tests have it)
    for kw in ok:  # accepted as far as the workspace check, the last one before the launches
        assert nearest(ws_bytes=16, **kw) == -4 and "needed" in err(), kw
    assert l.diffab_metrics_edit_nearest(null, null, 0, 20, null, null, 40, 30, null, 2, *[null] * 5, null, 0, null) == 0  # R = 0: no pointer is read

    def pack(segment=1, rows=6, group=3, K=40, L=16, **ptrs):
        a = dict.fromkeys(("tokens", "mask", "residue_mask", "segment_idx", "out_tokens", "out_len"), p)
        a.update(ptrs)
        return l.diffab_metrics_pack_sequences(a["tokens"], a["mask"], a["residue_mask"], a["segment_idx"], segment, rows, group, K, L,
                                               a["out_tokens"], a["out_len"], null)

    for kw, word in ((dict(rows=-1), "extent"), (dict(group=0), "extent"), (dict(K=0), "extent"), (dict(group=4097, rows=4097), "at most 4096 designs"),
                     (dict(K=4097), "K = 4097 residues per patch, at most 4096"), (dict(rows=7), "not a multiple"), (dict(L=0), "L = 0"),
                     (dict(L=257), "L = 257 tokens per sequence outside [1, 256]"), (dict(tokens=null), "null input (tokens, mask)"),
                     (dict(mask=null), "null input (tokens, mask)")):
        rc = pack(**kw)
        assert rc == -1 and word in err() and err().startswith("metrics_pack_sequences:"), (kw, rc, err())
    assert pack(rows=0, tokens=null, mask=null, out_tokens=null, out_len=null) == 0  # an empty problem: no pointer is read
    assert pack(out_tokens=null, out_len=null) == 0  # nothing to write: nothing is enqueued


# ------------------------------------------------------------------ Python argument errors before any device work
@pytest.fixture
def no_library(monkeypatch):
    refuse_library(monkeypatch)


def designs_of(rows=4, K=8):
    return {"seq_idx": torch.zeros(rows, K, dtype=torch.long)}


def gen_of(G=2, K=8):
    gm = torch.zeros(G, K, dtype=torch.bool)
    gm[:, 2:6] = True
    return gm


def test_good_arguments_reach_the_library(no_library):
    q, lib = metrics.sequence_set(["ARD", "ARDYW"]), metrics.sequence_set(["ARDY", "", "W"])
    for kw in ({}, dict(radius=0), dict(radius=-1), dict(matrix=True), dict(exclude=torch.tensor([0, 7])), dict(exclude=torch.tensor([-1, 2], dtype=torch.int32))):
        with pytest.raises(ReachedTheLibrary):
            metrics.novelty(q, lib, **kw)
    with pytest.raises(ReachedTheLibrary):
        metrics.novelty(q, q, exclude="self", radius=0)
    with pytest.raises(ReachedTheLibrary):
        metrics.novelty(q, metrics.sequence_set([]))
    with pytest.raises(ReachedTheLibrary):
        metrics.novelty(metrics.sequence_set(["A" * 64]), metrics.sequence_set(["A" * 256]))
    seg = torch.zeros(2, 8, dtype=torch.long)
    for kw in ({}, dict(group_size=2), dict(group_size=1, generation_mask=gen_of(4)), dict(residue_mask=torch.ones(2, 8, dtype=torch.bool)),
               dict(segment_idx=seg, segment=0), dict(max_length=4), dict(max_length=256)):
        with pytest.raises(ReachedTheLibrary):
            metrics.design_sequences(**{**dict(designs=designs_of(), generation_mask=gen_of(), group_size=2), **kw})


@pytest.mark.parametrize("kw, match", [
    (dict(queries=torch.zeros(2, 3, dtype=torch.uint8)), "queries must be a metrics.SequenceSet"),
    (dict(library=["ARD"]), "library must be a metrics.SequenceSet"),
    (dict(queries=metrics.sequence_set(["A" * 65])), "queries is 65 tokens wide, at most 64"),
    (dict(radius=1.0), "radius must be an int or None"), (dict(radius=True), "radius must be an int or None"), (dict(radius=2 ** 31), "radius must be an int"),
    (dict(matrix=1), "matrix must be a bool"), (dict(exclude="others"), "exclude must be an integer tensor"),
    (dict(exclude="self"), "exclude='self' needs as many queries as library entries, got R = 2 and M = 3"),
    (dict(exclude=torch.zeros(3, dtype=torch.long)), r"exclude must be an integer tensor \(2,\)"), (dict(exclude=torch.zeros(2)), "exclude must be an integer tensor"),
    (dict(exclude=[0, 1]), "exclude must be an integer tensor"),
])
def test_novelty_argument_errors(no_library, kw, match):
    args = dict(queries=metrics.sequence_set(["ARD", "ARDYW"]), library=metrics.sequence_set(["ARDY", "", "W"]))
    args.update(kw)
    with pytest.raises(ValueError, match=r"metrics\.novelty\(\): .*" + match):
        metrics.novelty(args.pop("queries"), args.pop("library"), **args)


@pytest.mark.parametrize("kw, match", [
    (dict(designs={"translations": torch.zeros(4, 8, 3)}), "designs must be a dict with seq_idx"),
    (dict(designs={"seq_idx": torch.zeros(4, 8)}), r"designs\['seq_idx'\] must be an integer tensor"),
    (dict(group_size=3), "4 design rows are not a multiple of group_size = 3"), (dict(group_size=0), "group_size must be an int >= 1"),
    (dict(generation_mask=torch.ones(2, 8)), "generation_mask must be a bool tensor"), (dict(generation_mask=gen_of(4)), "generation_mask is"),
    (dict(residue_mask=torch.ones(2, 7, dtype=torch.bool)), "residue_mask is"),
    (dict(segment=1), "segment_idx and segment go together, segment_idx is missing"),
    (dict(segment_idx=torch.zeros(2, 8, dtype=torch.long)), "segment_idx and segment go together, segment is missing"),
    (dict(segment_idx=torch.zeros(2, 8), segment=0), "segment_idx must be an integer tensor"),
    (dict(segment_idx=torch.zeros(4, 8, dtype=torch.long), segment=0), r"segment_idx must be an integer tensor \(2, 8\)"),
    (dict(segment_idx=torch.zeros(2, 8, dtype=torch.long), segment=0.0), "segment must be an int"),
    (dict(max_length=0), r"max_length must be an int in \[1, 256\]"), (dict(max_length=257), "max_length must be an int"), (dict(max_length=8.0), "max_length must be an int"),
    (dict(max_length=3), "patch 0 has 4 counted residues, more than max_length = 3"),
    (dict(max_length=4, generation_mask=torch.cat([gen_of(1), torch.ones(1, 8, dtype=torch.bool)])), "patch 1 has 8 counted residues, more than max_length = 4"),
])
def test_design_sequences_argument_errors(no_library, kw, match):
    args = dict(designs=designs_of(), generation_mask=gen_of(), group_size=2)
    args.update(kw)
    with pytest.raises(ValueError, match=r"metrics\.design_sequences\(\): .*" + match):
        metrics.design_sequences(**args)


def test_signatures_constants_and_documents():
    sig = inspect.signature(metrics.novelty)
    assert list(sig.parameters) == ["queries", "library", "radius", "exclude", "matrix"]
    assert all(sig.parameters[k].kind is inspect.Parameter.KEYWORD_ONLY for k in list(sig.parameters)[2:])
    assert [sig.parameters[k].default for k in ("radius", "exclude", "matrix")] == [None, None, False]
    sig = inspect.signature(metrics.design_sequences)
    assert list(sig.parameters) == ["designs", "generation_mask", "group_size", "residue_mask", "segment_idx", "segment", "max_length"]
    assert all(sig.parameters[k].kind is inspect.Parameter.KEYWORD_ONLY for k in list(sig.parameters)[2:])
    assert [sig.parameters[k].default for k in list(sig.parameters)[2:]] == [1, None, None, None, 64]
    assert list(inspect.signature(metrics.SequenceSet).parameters) == ["tokens", "lengths"]
    for word in ("``novelty``", "``SequenceSet``", "``sequence_set``", "``design_sequences``", "novelty_kernels.hip", "include/diffab_hip_novelty.h"):
        assert word in metrics.__doc__, word
    doc = " ".join(metrics.novelty.__doc__.split())
    for word in ("distance > 0", 'novelty(q, q, exclude="self", radius=0)["n_within"] == 0', ".float().view(1, N, N)", "cluster"):
        assert word in doc, word
    readme, design, integration = (open(os.path.join(REPO, f)).read() for f in ("README.md", "DESIGN.md", "INTEGRATION.md"))
    assert "Which ones are new:" in readme and "4.26" in design
    for word in ("metrics.novelty", "metrics.design_sequences", "metrics.sequence_set", "diffab_metrics_edit_nearest", "diffab_metrics_pack_sequences"):
        assert word in readme and word in design, word
    for word in ("`novelty_ref.py`", "`test_novelty_host.py`", "`test_gpu_novelty.py`", "`novelty_bench.py`", "`profiles/novelty.md`", "`include/diffab_hip_novelty.h`"):
        assert word in readme, word
    assert "diffab_hip_novelty.h" in integration and "novelty_kernels.hip" in design
    makefile = open(os.path.join(REPO, "diffab-pytorch_amd", "csrc", "Makefile")).read()
    assert "$(OBJ)/novelty_kernels.o" in re.search(r"DEFINED_OBJS := (.*)", makefile).group(1)
