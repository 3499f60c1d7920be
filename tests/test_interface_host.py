"""Binding modes without a GPU: the numpy restatements of interface_ref.py on hand-made cases with the answer
written out, unpack_contact_map, the header / library / ctypes table of include/diffab_hip_interface.h, the two workspace macros, the
host-side refusals of the two entries and the Python argument errors, raised before the library is loaded."""
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
from diffab_pytorch import _hip, metrics
from interface_ref import contact_map_ref, pack_ref, pairwise_bits_ref, same_bits, unpack_ref
from sampler_support import ReachedTheLibrary, refuse_library

HEADER = os.path.join(REPO, "include", "diffab_hip_interface.h")
f32 = np.float32


# ------------------------------------------------------------------ the restatements on hand-made cases
def hand_case():
    """One patch, K = 6, one atom per residue, on a line.  Slots 0, 1 generated (x = 0 and 3); slots 2..5 flagged as antigen: slot 2 at
    x = 4 is the chain neighbour of slot 1; slot 3 at x = 5 (exactly the contact distance from slot 0); slot 4 at x = 7.5; slot 5 at
    x = 6 lies outside residue_mask.  Slot 1 is flagged as antigen too, and is generated: no column."""
    x = np.array([0.0, 3.0, 4.0, 5.0, 7.5, 6.0], f32)
    pts = np.zeros((1, 6, 1, 3), f32)
    pts[0, :, 0, 0] = x
    gen = np.array([[1, 1, 0, 0, 0, 0]], bool)
    rm = np.array([[1, 1, 1, 1, 1, 0]], bool)
    antigen = np.array([[0, 1, 1, 1, 1, 1]], bool)
    chain = np.array([[0, 0, 0, 1, 1, 1]])
    ridx = np.array([[0, 1, 2, 3, 4, 5]])
    ones = np.ones((1, 6), np.int64)
    return dict(points=pts, valid=ones, ctx_points=pts, ctx_valid=ones, gen=gen, rm=rm, chain=chain, ridx=ridx, antigen=antigen)


def test_contact_map_ref_on_a_hand_case():
    c = hand_case()
    m = contact_map_ref(**c)
    want = np.zeros((1, 6, 6), bool)
    want[0, 0, 2] = True  # 4 A
    want[0, 1, 3] = True  # 2 A; (1, 2) is 1 A apart but a chain neighbour; (0, 3) is exactly 5 A: not below it
    want[0, 1, 4] = True  # 4.5 A; (0, 4) is 7.5 A; slot 5 is outside residue_mask; slot 1 is generated: no column
    assert np.array_equal(m, want)
    assert contact_map_ref(**c, ignore_bonds=True)[0, 1, 2] and not contact_map_ref(**c, ignore_bonds=True)[0, 0, 3]
    assert contact_map_ref(**c, contact_distance=np.nextafter(f32(5), f32(6)))[0, 0, 3]  # one ulp further: a contact
    bits = pack_ref(m)
    assert bits.dtype == np.int32 and bits.shape == (1, 6, 1) and bits[0, :, 0].tolist() == [4, 24, 0, 0, 0, 0]
    # an atom whose validity bit is clear does not exist, on either side
    c2 = dict(c, valid=np.array([[0, 1, 1, 1, 1, 1]]))
    assert not contact_map_ref(**c2)[0, 0].any() and contact_map_ref(**c2)[0, 1].sum() == 2
    c3 = dict(c, ctx_valid=np.array([[1, 1, 1, 0, 1, 1]]))
    assert contact_map_ref(**c3)[0, :, 3].sum() == 0 and contact_map_ref(**c3).sum() == 2


def test_pack_and_unpack_at_the_sign_bit_and_a_ragged_word():
    m = np.zeros((1, 33, 33), bool)
    m[0, 0, 31] = m[0, 0, 32] = m[0, 2, 0] = m[0, 32, 5] = True
    bits = pack_ref(m)
    assert bits.shape == (1, 33, 2) and bits[0, 0].tolist() == [-2 ** 31, 1] and bits[0, 2].tolist() == [1, 0] and bits[0, 32].tolist() == [32, 0]
    assert np.array_equal(unpack_ref(bits)[:, :, :33], m) and not unpack_ref(bits)[:, :, 33:].any()


def test_unpack_contact_map_on_a_hand_written_example():
    K = 33
    bits = torch.zeros(2, K, 2, dtype=torch.int32)
    bits[0, 0, 0] = -2 ** 31  # column 31: the sign bit is data
    bits[0, 0, 1] = 1  # column 32
    bits[0, 4, 0] = 0b101  # columns 0 and 2
    bits[1, 32, 1] = 3  # column 32, and bit 33, which is no column
    m = metrics.unpack_contact_map(bits, K)
    assert m.dtype == torch.bool and tuple(m.shape) == (2, K, K)
    assert sorted(map(tuple, m.nonzero().tolist())) == [(0, 0, 31), (0, 0, 32), (0, 4, 0), (0, 4, 2), (1, 32, 32)]
    want = np.zeros((2, K, K), bool)
    for r, i, j in [(0, 0, 31), (0, 0, 32), (0, 4, 0), (0, 4, 2), (1, 32, 32)]:
        want[r, i, j] = True
    assert np.array_equal(pack_ref(want)[0], bits[0].numpy()) and np.array_equal(unpack_ref(bits.numpy())[:, :, :K], m.numpy())
    for bad, match in ((dict(bits=bits.float()), "int32 tensor"), (dict(bits=bits[:, :, :1]), "int32 tensor"), (dict(bits=bits[0]), "int32 tensor"),
                       (dict(K=0), "K must be an int"), (dict(K=32), "int32 tensor"), (dict(K=True), "K must be an int")):
        args = dict(bits=bits, K=K)
        args.update(bad)
        with pytest.raises(ValueError, match=r"metrics\.unpack_contact_map\(\): .*" + match):
            metrics.unpack_contact_map(args["bits"], args["K"])


def test_pairwise_bits_ref_on_a_hand_case():
    # designs of two words: A = {0, 1, 31}, B = {1, 31, 32}, C = {}, D = A
    bits = np.array([[3 - 2 ** 31, 0], [2 - 2 ** 31, 1], [0, 0], [3 - 2 ** 31, 0]], np.int32)
    r = pairwise_bits_ref(bits, 4)
    assert r["n_set"].tolist() == [[3, 3, 0, 3]]
    assert r["n_common"].tolist() == [[[3, 2, 0, 3], [2, 3, 0, 2], [0, 0, 0, 0], [3, 2, 0, 3]]]
    third = f32(2) / f32(3)
    assert same_bits(r["fcc"], np.array([[[1, third, 0, 1], [third, 1, 0, third], [1, 1, 1, 1], [1, third, 0, 1]]], f32))
    assert same_bits(r["jaccard"], np.array([[[1, 0.5, 0, 1], [0.5, 1, 0, 0.5], [0, 0, 1, 0], [1, 0.5, 0, 1]]], f32))
    assert all(r[k].dtype == (np.int32 if k.startswith("n_") else f32) for k in r)
    # fcc is not symmetric: a set inside a larger one
    r = pairwise_bits_ref(np.array([[1], [7]], np.int32), 2)
    assert r["fcc"].tolist() == [[[1, 1], [float(f32(1) / f32(3)), 1]]] and r["jaccard"][0, 0, 1] == r["jaccard"][0, 1, 0] == f32(1) / f32(3)
    # two patches of two designs, any trailing shape: the words of a design are its row, flattened
    r2 = pairwise_bits_ref(np.array([[[1], [2]], [[1], [3]], [[4], [0]], [[4], [0]]], np.int32), 2)
    assert r2["n_common"].tolist() == [[[2, 2], [2, 3]], [[1, 1], [1, 1]]]


# ------------------------------------------------------------------ the header, the library and the ctypes table
def header_code():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


def test_header_library_and_symbol_table_agree():
    """Every entry the header declares is in _hip.INTERFACE_SYMBOLS with the same arity and kinds, is exported, and is typed by
    load_library(); nothing else is in the table, and the table shares no name with the four older ones."""
    code = header_code()
    protos = dict(re.findall(r"\bint\s+(diffab_[a-z0-9_]+)\s*\((.*?)\)\s*;", code, flags=re.S))
    declared = sorted(set(re.findall(r"\b(diffab_[a-z0-9_]+)\s*\(", code)))
    assert declared == sorted(protos) and {"diffab_metrics_contact_bits", "diffab_metrics_pairwise_bits"} <= set(declared)
    assert sorted(_hip.INTERFACE_SYMBOLS) == declared, "INTERFACE_SYMBOLS and include/diffab_hip_interface.h drifted apart"
    older = set(_hip.SYMBOLS) | set(_hip.ANALYSIS_SYMBOLS) | set(_hip.HBOND_SYMBOLS) | set(_hip.CLUSTER_SYMBOLS)
    assert not set(_hip.INTERFACE_SYMBOLS) & older
    raw = ctypes.CDLL(_hip.LIB_PATH)
    typed = _hip.load_library()
    kinds = {"int32_t": ctypes.c_int32, "size_t": ctypes.c_size_t, "float": ctypes.c_float}
    for name, proto in protos.items():
        assert hasattr(raw, name), f"{name} is declared in include/diffab_hip_interface.h but not exported by libdiffab_hip.so"
        res, args = _hip.INTERFACE_SYMBOLS[name]
        fn = getattr(typed, name)
        assert fn.restype is res and list(fn.argtypes) == args  # load_library() types the fifth table onto the same CDLL object
        params = [p.strip() for p in proto.split(",")]
        assert res is ctypes.c_int and len(args) == len(params), name
        for p, a in zip(params, args):
            kind = p.rsplit(" ", 1)[0]
            if kind in kinds:
                assert a is kinds[kind], (name, p)
            else:
                assert "*" in kind and a is ctypes.c_void_p, (name, p)
    names = lambda n: [p.strip().rsplit(" ", 1)[1].lstrip("*") for p in protos[n].split(",")]
    assert names("diffab_metrics_contact_bits") == [
        "points", "valid", "context_points", "context_valid", "generation_mask", "residue_mask", "antigen_mask", "chain", "residue_idx", "rows",
        "group_size", "K", "P", "A", "contact_distance", "bits", "n_contacts", "workspace", "workspace_bytes", "stream"]
    assert names("diffab_metrics_pairwise_bits") == ["bits", "G", "N", "L", "n_set", "n_common", "fcc", "jaccard", "workspace", "workspace_bytes",
                                                      "stream"]
    text = open(HEADER).read()
    assert '#include "diffab_hip.h"' in text and "Why a header of its own" in text.split("*/")[0]
    for macro, value in (("DIFFAB_INTERFACE_MAX_K", metrics.INTERFACE_MAX_K), ("DIFFAB_INTERFACE_MAX_WORDS", metrics.INTERFACE_MAX_WORDS)):
        assert int(re.search(rf"#define\s+{macro}\s+(\d+)", code).group(1)) == value
    assert metrics.INTERFACE_MAX_K >= 512 and metrics.INTERFACE_MAX_WORDS == metrics.INTERFACE_MAX_K * (metrics.INTERFACE_MAX_K // 32)


CONTACT_SHAPES = [(1, 1, 1), (1, 5, 5), (2, 33, 32), (3, 64, 15), (2, 70, 32), (16, 128, 5), (256, 128, 15), (7, 511, 3), (4, 512, 32),
                  (300000, 512, 32)]
PAIR_SHAPES = [(1, 1, 1), (2, 3, 5), (3, 63, 7), (2, 65, 33), (1, 129, 600), (2, 257, 40), (16, 1024, 512), (256, 64, 512), (4, 4096, 512),
               (1, 4096, 8192), (3, 4033, 8191), (40, 4096, 8192)]
MACRO_C = r"""
#include <stdio.h>
#include "diffab_hip_interface.h"
int main(void) {
%s
  printf("%%d %%d %%d %%d\n", DIFFAB_ERR_ARG, DIFFAB_INTERFACE_MAX_K, DIFFAB_INTERFACE_MAX_WORDS, DIFFAB_INTERFACE_TILE_COLUMNS);
  return 0;
}
"""


def test_workspace_macros_equal_the_python_mirrors(tmp_path):
    """The header compiles as C on its own (it brings diffab_hip.h along) and its macros give metrics.*_workspace_bytes."""
    cc = shutil.which("cc") or shutil.which("gcc") or next((p for p in ("/opt/rocm/llvm/bin/clang",) if os.path.exists(p)), None)
    assert cc, "no C compiler to read the header's macros with"
    src, exe = tmp_path / "macro.c", tmp_path / "macro"
    lines = [f'  printf("%zu\\n", DIFFAB_METRICS_CONTACT_BITS_WORKSPACE_BYTES({G}, {K}, {A}));' for G, K, A in CONTACT_SHAPES]
    lines += [f'  printf("%zu\\n", DIFFAB_METRICS_PAIRWISE_BITS_WORKSPACE_BYTES({G}, {N}, {L}));' for G, N, L in PAIR_SHAPES]
    src.write_text(MACRO_C % "\n".join(lines))
    subprocess.run([cc, "-I", os.path.join(REPO, "include"), str(src), "-o", str(exe)], check=True)
    got = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()
    want = [metrics.contact_bits_workspace_bytes(*s) for s in CONTACT_SHAPES] + [metrics.pairwise_bits_workspace_bytes(*s) for s in PAIR_SHAPES]
    assert [int(v) for v in got[:len(want)]] == want
    assert got[len(want):] == ["-1", str(metrics.INTERFACE_MAX_K), str(metrics.INTERFACE_MAX_WORDS), "64"]
    assert metrics.contact_bits_workspace_bytes(300000, 512, 32) > 1 << 32 and metrics.pairwise_bits_workspace_bytes(40, 4096, 8192) > 1 << 32
    assert metrics.pairwise_bits_workspace_bytes(1, 65, 3) == 3 * 128 * 4 + 2 * 3 * 4 + 3 * 4 + 4 + 2048


def test_host_side_refusals_touch_no_gpu():
    """Every refusal is decided from the scalar arguments and whether a pointer is null: the device pointers are fake addresses that
    are never dereferenced, nothing is enqueued (no GPU is needed), and diffab_last_error names the problem."""
    l = _hip.load_library()
    p, null = ctypes.c_void_p(4096), ctypes.c_void_p(0)
    err = lambda: l.diffab_last_error().decode()
    inputs = ("points", "valid", "context_points", "context_valid", "generation_mask", "residue_mask", "antigen_mask", "chain", "residue_idx")

    def contact(rows=6, group=3, K=40, P=5, A=15, dist=5.0, ws=p, ws_bytes=1 << 40, **ptrs):
        a = dict.fromkeys(inputs + ("bits", "n_contacts"), p)
        a.update(ptrs)
        return l.diffab_metrics_contact_bits(*[a[k] for k in inputs], rows, group, K, P, A, dist, a["bits"], a["n_contacts"], ws, ws_bytes, null)

    for kw, word in ((dict(rows=-1), "extent"), (dict(group=0), "extent"), (dict(K=0), "extent"), (dict(group=4097, rows=4097), "at most 4096 designs"),
                     (dict(K=513), "K = 513 residues per patch, at most 512"), (dict(rows=7), "not a multiple"), (dict(P=0), "P = 0"),
                     (dict(P=6), "P = 6"), (dict(A=0), "A = 0"), (dict(A=33), "A = 33"), (dict(dist=-1.0), "contact_distance"),
                     (dict(dist=float("inf")), "contact_distance"), (dict(dist=float("nan")), "contact_distance"),
                     (dict(points=null), "null input"), (dict(valid=null), "null input"), (dict(context_points=null), "null input"),
                     (dict(context_valid=null), "null input"), (dict(generation_mask=null), "null input"), (dict(antigen_mask=null), "null input"),
                     (dict(chain=null), "null input"), (dict(residue_idx=null), "null input"), (dict(bits=null), "null output"),
                     (dict(n_contacts=null), "null output"), (dict(ws=null), "workspace"), (dict(ws=ctypes.c_void_p(4096 + 16)), "256-byte aligned")):
        rc = contact(**kw)
        assert rc == -1 and word in err() and err().startswith("metrics_contact_bits:"), (kw, rc, err())
    need = metrics.contact_bits_workspace_bytes(2, 40, 15)
    assert contact(ws_bytes=need // 2) == -4 and "needed" in err() and err().startswith("metrics_contact_bits:")  # DIFFAB_ERR_WORKSPACE
    assert need - 2048 <= int(re.search(r"(\d+) needed", err()).group(1)) <= need
    for kw in (dict(K=512), dict(K=1), dict(group=1), dict(rows=4096, group=4096), dict(P=1, A=1), dict(A=32), dict(dist=0.0), dict(residue_mask=null)):
        assert contact(ws_bytes=16, **kw) == -4 and "needed" in err(), kw
    assert l.diffab_metrics_contact_bits(*[null] * 9, 0, 5, 128, 5, 15, 5.0, null, null, null, 0, null) == 0  # an empty problem

    def pair(G=2, N=100, L=7, ws=p, ws_bytes=1 << 40, **ptrs):
        a = dict.fromkeys(("bits", "n_set", "n_common", "fcc", "jaccard"), p)
        a.update(ptrs)
        return l.diffab_metrics_pairwise_bits(a["bits"], G, N, L, a["n_set"], a["n_common"], a["fcc"], a["jaccard"], ws, ws_bytes, null)

    for kw, word in ((dict(G=-1), "extent"), (dict(N=0), "extent"), (dict(L=0), "extent"), (dict(N=4097), "at most 4096 designs"),
                     (dict(L=8193), "L = 8193 words per design, at most 8192"), (dict(bits=null), "null input"), (dict(ws=null), "workspace"),
                     (dict(ws=ctypes.c_void_p(4096 + 128)), "256-byte aligned")):
        rc = pair(**kw)
        assert rc == -1 and word in err() and err().startswith("metrics_pairwise_bits:"), (kw, rc, err())
    need = metrics.pairwise_bits_workspace_bytes(2, 100, 7)
    assert pair(ws_bytes=need // 2) == -4 and "needed" in err() and err().startswith("metrics_pairwise_bits:")
    assert need - 2048 <= int(re.search(r"(\d+) needed", err()).group(1)) <= need
    for kw in (dict(N=4096, L=8192), dict(N=1, L=1), dict(n_set=null), dict(n_common=null, fcc=null), dict(n_set=null, n_common=null, fcc=null)):
        assert pair(ws_bytes=16, **kw) == -4 and "needed" in err(), kw
    assert l.diffab_metrics_pairwise_bits(null, 0, 8, 3, null, null, null, null, null, 0, null) == 0  # an empty problem


# ------------------------------------------------------------------ Python argument errors before any device work
@pytest.fixture
def no_library(monkeypatch):
    refuse_library(monkeypatch)


def good(rows=4, K=8, N=2):
    G = rows // N
    designs = dict(seq_idx=torch.zeros(rows, K, dtype=torch.long), translations=torch.zeros(rows, K, 3),
                   orientations=torch.eye(3).expand(rows, K, 3, 3).clone())
    gm = torch.zeros(G, K, dtype=torch.bool)
    gm[:, 2:4] = True
    return dict(designs=designs, generation_mask=gm, antigen_mask=~gm, group_size=N)


def test_good_arguments_reach_the_library(no_library):
    a = good()
    context = {"xyz": torch.zeros(2, 8, 15, 3), "atom_mask": torch.ones(2, 8, 15)}
    for kw in ({}, dict(context=context), dict(residue_mask=torch.ones(2, 8, dtype=torch.bool)), dict(chain_idx=torch.zeros(8, dtype=torch.long)),
               dict(residue_idx=torch.arange(8).expand(2, 8)), dict(contact_distance=8), dict(atoms=("CA",)), dict(contact_distance=0.0)):
        with pytest.raises(ReachedTheLibrary):
            metrics.contact_map(**{**a, **kw})
    with pytest.raises(ReachedTheLibrary):
        metrics.contact_map(**good(rows=1, K=512, N=1))
    for bits, N in ((torch.zeros(4, 8, 1, dtype=torch.int32), 2), (torch.zeros(4, 3, dtype=torch.int32), 4), (torch.zeros(6, 2, 2, 2, dtype=torch.int32), 3),
                    (torch.zeros(1, 8192, dtype=torch.int32), 1)):
        with pytest.raises(ReachedTheLibrary):
            metrics.pairwise_bits(bits, group_size=N)


@pytest.mark.parametrize("kw, match", [
    (dict(antigen_mask=None), "antigen_mask is required"), (dict(antigen_mask=torch.ones(2, 8)), "antigen_mask must be a bool tensor"),
    (dict(antigen_mask=torch.ones(2, 7, dtype=torch.bool)), r"antigen_mask is \(2, 7\), expected \(2, 8\)"),
    (dict(generation_mask=torch.ones(2, 8)), "generation_mask must be a bool tensor"),
    (dict(generation_mask=torch.ones(4, 8, dtype=torch.bool)), "generation_mask is"),
    (dict(residue_mask=torch.ones(2, 8)), "residue_mask must be a bool tensor"), (dict(residue_mask=torch.ones(8, dtype=torch.bool)), "residue_mask is"),
    (dict(group_size=3), "4 design rows are not a multiple of group_size = 3"), (dict(group_size=0), "group_size must be an int >= 1"),
    (dict(group_size=2.0), "group_size must be an int"), (dict(designs={"seq_idx": torch.zeros(4, 8)}), "designs must be a dict"),
    (dict(designs=dict(seq_idx=torch.zeros(4, 8), translations=torch.zeros(4, 8, 3), orientations=torch.zeros(4, 8, 3, 3))), "seq_idx.* must be an integer"),
    (dict(designs=dict(seq_idx=torch.zeros(4, 8, dtype=torch.long), translations=torch.zeros(4, 8, 3, dtype=torch.long),
                       orientations=torch.zeros(4, 8, 3, 3))), "translations"),
    (dict(designs=dict(seq_idx=torch.zeros(4, 8, dtype=torch.long), translations=torch.zeros(4, 8, 3))), "orientations"),
    (dict(contact_distance=-1.0), "contact_distance must be a finite number >= 0"), (dict(contact_distance=float("inf")), "contact_distance"),
    (dict(contact_distance="5"), "contact_distance"), (dict(atoms="CA"), "atoms must be a sequence"), (dict(atoms=("CA", "CG")), "atoms must be"),
    (dict(atoms=()), "atoms must be"), (dict(context={"xyz": torch.zeros(2, 8, 15, 3)}), "context must be a dict"),
    (dict(context={"xyz": torch.zeros(2, 8, 33, 3), "atom_mask": torch.ones(2, 8, 33)}), r"A = 33 atoms per residue, outside \[1, 32\]"),
    (dict(context={"xyz": torch.zeros(2, 7, 15, 3), "atom_mask": torch.ones(2, 7, 15)}), r"context\['xyz'\] is"),
    (dict(context={"xyz": torch.zeros(2, 8, 15, 3), "atom_mask": torch.ones(2, 8, 14)}), r"context\['atom_mask'\] is"),
    (dict(chain_idx=torch.zeros(8)), "needs an integer chain_idx"), (dict(chain_idx=torch.zeros(3, 8, dtype=torch.long)), "chain_idx .* does not broadcast"),
    (dict(residue_idx=torch.zeros(7, dtype=torch.long)), "residue_idx .* does not broadcast"),
])
def test_contact_map_argument_errors(no_library, kw, match):
    args = good()
    args.update(kw)
    with pytest.raises(ValueError, match=r"metrics\.contact_map\(\): .*" + match):
        metrics.contact_map(**args)


def test_contact_map_refuses_k_over_the_limit(no_library):
    with pytest.raises(ValueError, match=r"metrics\.contact_map\(\): K = 513 residues per patch, at most 512"):
        metrics.contact_map(**good(rows=1, K=513, N=1))


@pytest.mark.parametrize("bits, N, match", [
    (torch.zeros(4, 8, 1), 2, "bits must be an int32 tensor"), (torch.zeros(4, 8, 1, dtype=torch.int64), 2, "bits must be an int32 tensor"),
    (torch.zeros(4, 8, dtype=torch.bool), 2, "bits must be an int32"), (torch.zeros(4, dtype=torch.int32), 2, "bits must be an int32"),
    ([[0]], 1, "bits must be an int32"), (torch.zeros(4, 8, 1, dtype=torch.int32), 3, "4 design rows are not a multiple of group_size = 3"),
    (torch.zeros(4, 8, 1, dtype=torch.int32), 0, "group_size must be an int >= 1"), (torch.zeros(4, 8, 1, dtype=torch.int32), 2.0, "group_size must be"),
    (torch.zeros(4, 8, 1, dtype=torch.int32), True, "group_size must be"), (torch.zeros(4097, 1, dtype=torch.int32), 4097, "at most 4096 designs"),
    (torch.zeros(2, 8193, dtype=torch.int32), 1, r"L = 8193 words per design, outside \[1, 8192\]"),
    (torch.zeros(2, 513, 17, dtype=torch.int32), 1, "words per design, outside"), (torch.zeros(2, 0, dtype=torch.int32), 1, "L = 0 words"),
])
def test_pairwise_bits_argument_errors(no_library, bits, N, match):
    with pytest.raises(ValueError, match=r"metrics\.pairwise_bits\(\): .*" + match):
        metrics.pairwise_bits(bits, group_size=N)


def test_signatures_and_constants():
    sig = inspect.signature(metrics.contact_map)
    assert list(sig.parameters) == ["designs", "generation_mask", "context", "antigen_mask", "chain_idx", "residue_idx", "residue_mask", "group_size",
                                    "contact_distance", "atoms"]
    assert all(sig.parameters[k].kind is inspect.Parameter.KEYWORD_ONLY for k in list(sig.parameters)[2:])
    assert sig.parameters["contact_distance"].default == 5.0 and sig.parameters["group_size"].default == 1
    assert sig.parameters["atoms"].default == inspect.signature(metrics.contacts).parameters["atoms"].default
    sig = inspect.signature(metrics.pairwise_bits)
    assert list(sig.parameters) == ["bits", "group_size"] and sig.parameters["group_size"].kind is inspect.Parameter.KEYWORD_ONLY
    assert list(inspect.signature(metrics.unpack_contact_map).parameters) == ["bits", "K"]
    for word in ("``contact_map``", "``pairwise_bits``", "interface_kernels.hip", "include/diffab_hip_interface.h"):
        assert word in metrics.__doc__, word
