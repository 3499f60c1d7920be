"""Developability without a GPU: the numpy restatements of developability_ref.py on hand-made cases with the
answers written out, motif_masks, the default tables, the header / library / ctypes table of include/diffab_hip_develop.h, the two
workspace macros, the host-side refusals of the two entries and the Python argument errors, raised before the library is loaded."""
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
from developability_ref import EXPOSED, PRESENT, SCOPE, motifs_ref, patches_ref, succ_ref
from diffab_pytorch import _hip, io as dio, metrics
from sampler_support import ReachedTheLibrary, refuse_library

HEADER = os.path.join(REPO, "include", "diffab_hip_develop.h")
f32 = np.float32
AA = {c: i for i, c in enumerate(dio.AA1)}
ALL = PRESENT | SCOPE | EXPOSED


# ------------------------------------------------------------------ patches: hand-made cases with the answers written out
def line(xs, tokens, gen, **kw):
    """One row, residues on the x axis; the row's sites and the patch's sites are the same points."""
    xs = np.asarray(xs, f32)
    sites = np.zeros((1, len(xs), 3), f32)
    sites[0, :, 0] = xs
    args = dict(hydrophobicity=[1.0, 2.0, 0.5], charge=[0.0, 1.0, -2.0], neighbour_distance=100.0, max_neighbours=100, vicinity_distance=100.0,
                patch_distance=7.5, min_distance=3.8)
    args.update(kw)
    return patches_ref(sites, sites, np.asarray([tokens]), np.asarray([gen], bool), **args)


def test_a_pair_at_the_patch_distance_is_no_pair_and_one_ulp_inside_is():
    inside = float(np.nextafter(f32(7.5), f32(0)))
    # slots 0 and 1 are exactly 7.5 apart, slots 0 and 2 one ulp less, slots 1 and 2 far apart
    r = line([0.0, 7.5, -inside], [1, 0, 1], [1, 1, 1])
    assert f32(0.0) - f32(-inside) < f32(7.5)  # (the subtraction the rule makes gives a distance below the cut-off)
    assert r["n_pairs"].tolist() == [1] and r["state"].tolist() == [[ALL] * 3]
    d2 = float(f32(inside) * f32(inside))
    assert d2 < float(f32(7.5) * f32(7.5))
    assert r["psh_f64"][0] == 2.0 * 2.0 / d2 and r["ppc_f64"][0] == 1.0 / d2 and r["pnc"][0] == 0
    assert r["residue_psh_f64"][0].tolist() == [4.0 / d2, 0, 4.0 / d2] and r["residue_ppc_f64"][0].tolist() == [1.0 / d2, 0, 1.0 / d2]
    assert r["psh"].dtype == f32 and r["psh"][0] == f32(4.0 / d2)


def test_exactly_max_neighbours_is_exposed_and_one_more_is_not():
    # neighbour_distance 5: slot 0 at x = 0 has neighbours at 3 and 4 (two); slot 1 at x = 3 has 0, 4 and 7 (three); 5 apart is no neighbour
    r = line([0.0, 3.0, 4.0, 7.0, 9.0], [0] * 5, [1] * 5, neighbour_distance=5.0, max_neighbours=2)
    assert r["n_neighbours"].tolist() == [[2, 3, 3, 3, 1]]
    assert r["state"].tolist() == [[ALL, PRESENT | SCOPE, PRESENT | SCOPE, PRESENT | SCOPE, ALL]]
    assert r["n_scope"].tolist() == [5] and r["n_exposed"].tolist() == [2] and r["n_pairs"].tolist() == [0]  # 0 and 9: too far apart
    # exposed_in decides instead, the count is still reported, and a residue outside the scope stays unexposed
    ex = np.array([[0, 1, 1, 0, 0]], bool)
    r2 = line([0.0, 3.0, 4.0, 7.0, 9.0], [0] * 5, [1, 1, 0, 0, 0], neighbour_distance=5.0, max_neighbours=2, vicinity_distance=3.5, exposed_in=ex)
    assert r2["n_neighbours"].tolist() == [[2, 3, 3, 3, 1]]
    assert r2["state"].tolist() == [[PRESENT | SCOPE, ALL, ALL, PRESENT, PRESENT]]  # slot 2 is 1 A from generated slot 1; slot 3 is 4 A from it
    assert r2["n_pairs"].tolist() == [1] and r2["psh_f64"][0] == 1.0 / float(f32(3.8) * f32(3.8))


def test_a_pair_closer_than_min_distance_is_clamped():
    r = line([0.0, 1.0], [1, 1], [1, 1])
    floor = float(f32(3.8) * f32(3.8))
    assert r["psh_f64"][0] == 4.0 / floor and r["ppc_f64"][0] == 1.0 / floor and r["n_pairs"].tolist() == [1]
    r = line([0.0, 5.0], [2, 2], [1, 1])
    assert r["psh_f64"][0] == 0.25 / 25.0 and r["pnc_f64"][0] == 4.0 / 25.0 and r["ppc"][0] == 0  # two negative charges: pnc, positive
    assert r["charge_generated"].tolist() == [-4.0] and r["charge_scope"].tolist() == [-4.0]
    r = line([0.0, 5.0], [1, 2], [1, 0])  # opposite charges: neither ppc nor pnc
    assert r["ppc"][0] == 0 and r["pnc"][0] == 0 and r["psh_f64"][0] == 1.0 / 25.0
    assert r["charge_generated"].tolist() == [1.0] and r["charge_scope"].tolist() == [-1.0]


def test_an_antigen_residue_in_the_middle_changes_nothing():
    xs, tokens, gen = [0.0, 2.0, 4.0], [1, 1, 1], [1, 0, 1]
    with_antigen = line(xs, tokens, gen, antigen=np.array([[0, 1, 0]], bool), neighbour_distance=5.0, max_neighbours=1)
    assert with_antigen["state"].tolist() == [[ALL, 0, ALL]] and with_antigen["n_neighbours"].tolist() == [[1, 0, 1]]
    assert with_antigen["n_pairs"].tolist() == [1] and with_antigen["psh_f64"][0] == 4.0 / 16.0
    moved = line([0.0, 1e6, 4.0], tokens, gen, antigen=np.array([[0, 1, 0]], bool), neighbour_distance=5.0, max_neighbours=1)
    outside = line(xs, tokens, gen, rm=np.array([[1, 0, 1]], bool), neighbour_distance=5.0, max_neighbours=1)
    for k in with_antigen:
        assert np.array_equal(with_antigen[k], moved[k]) and np.array_equal(with_antigen[k], outside[k]), k
    # without the mask the middle residue is a third neighbour: nobody is exposed any more
    assert line(xs, tokens, gen, neighbour_distance=5.0, max_neighbours=1)["n_exposed"].tolist() == [0]


def test_an_unknown_token_weighs_nothing():
    for tok in (3, -1, 1000):
        r = line([0.0, 5.0, 10.0], [1, tok, 1], [1, 1, 1])
        assert r["n_pairs"].tolist() == [2] and r["psh"][0] == 0 and r["ppc"][0] == 0 and r["state"].tolist() == [[ALL] * 3]
        assert r["charge_generated"].tolist() == [2.0]


def test_a_gly_site_is_its_ca():
    """The front end's site: CB of the frame, CA where the token is Gly."""
    t = torch.tensor([[[1.0, 2.0, 3.0], [4.0, 5.0, 6.0]]])
    O = torch.eye(3).expand(1, 2, 3, 3).clone()
    frame = dio.backbone_from_frames(t, O, ("CA", "CB"))
    seq = torch.tensor([[metrics.GLY, 0]])
    sites = torch.where((seq == metrics.GLY).unsqueeze(-1), frame[:, :, 0], frame[:, :, 1])
    assert torch.equal(sites[0, 0], t[0, 0]) and torch.equal(sites[0, 1], frame[0, 1, 1]) and not torch.equal(sites[0, 1], t[0, 1])
    assert abs(float((sites[0, 1] - t[0, 1]).norm()) - 1.53) < 0.02  # a CA - CB bond


# ------------------------------------------------------------------ motifs: hand-made cases
SEQUON = metrics.motif_masks({"n_glycosylation": "N[^P][ST]"}).numpy()


def run_motifs(letters, gen, ridx=None, chain=None, rm=None, motifs=SEQUON, tokens=None):
    K = len(letters)
    tokens = np.array([[AA[c] for c in letters]]) if tokens is None else tokens
    ridx = np.arange(K)[None] if ridx is None else np.asarray([ridx])
    chain = np.zeros((1, K), int) if chain is None else np.asarray([chain])
    return motifs_ref(tokens, np.asarray([gen], bool), rm, chain, ridx, motifs)


def test_the_sequon_along_the_chain():
    gen = [1, 1, 1, 0]
    assert run_motifs("NASA", gen)["motif_count"].tolist() == [[1]] and run_motifs("NASA", gen)["motif_start"].tolist() == [[1, 0, 0, 0]]
    assert run_motifs("NPSA", gen)["n_motifs"].tolist() == [0]  # N-P-S
    assert run_motifs("NASA", gen, ridx=[0, 1, 3, 4])["n_motifs"].tolist() == [0]  # a numbering gap between A and S
    assert run_motifs("NASA", gen, chain=[0, 0, 1, 1])["n_motifs"].tolist() == [0]  # a chain boundary
    # chain neighbours that are not adjacent slots: N (slot 0) -> A (slot 3) -> S (slot 1)
    r = run_motifs("NSCA", [1, 0, 0, 0], ridx=[10, 12, 50, 11])
    assert r["n_motifs"].tolist() == [1] and r["motif_start"].tolist() == [[1, 0, 0, 0]]
    assert succ_ref(np.ones(4, bool), np.zeros(4, int), np.array([10, 12, 50, 11])).tolist() == [3, -1, -1, 1]
    # the lowest slot wins where two slots carry the next number, and a slot outside residue_mask is nobody's neighbour
    assert succ_ref(np.ones(3, bool), np.zeros(3, int), np.array([1, 2, 2])).tolist() == [1, -1, -1]
    assert succ_ref(np.array([1, 0, 1], bool), np.zeros(3, int), np.array([1, 2, 2])).tolist() == [2, -1, -1]
    assert run_motifs("NASA", gen, rm=np.array([[1, 0, 1, 1]], bool))["n_motifs"].tolist() == [0]
    assert run_motifs("NASA", gen, rm=np.array([[0, 1, 1, 1]], bool))["n_motifs"].tolist() == [0]


def test_a_motif_is_counted_where_it_touches_the_design():
    assert run_motifs("ANASA", [1, 0, 0, 0, 0])["n_motifs"].tolist() == [0]  # wholly outside the generated residues
    assert motifs_ref(np.array([[AA[c] for c in "ANASA"]]), np.array([[1, 0, 0, 0, 0]], bool), None, np.zeros((1, 5), int), np.arange(5)[None],
                      SEQUON, counted_only=False)["n_motifs"].tolist() == [1]
    r = run_motifs("ANASA", [0, 0, 0, 1, 1])  # straddling the edge: only the S is generated
    assert r["n_motifs"].tolist() == [1] and r["motif_start"].tolist() == [[0, 1, 0, 0, 0]]
    both = metrics.motif_masks(["C", "N[GS]"]).numpy()
    r = run_motifs("CNGC", [0, 0, 1, 1], motifs=both)
    assert r["motif_count"].tolist() == [[1, 1]] and r["n_motifs"].tolist() == [2] and r["motif_start"].tolist() == [[0, 2, 0, 1]]


def test_the_sign_bit_at_32_motifs_and_a_token_of_32_or_more():
    many = metrics.motif_masks(["A"] * 31 + ["C"]).numpy()
    r = run_motifs("CA", [1, 1], motifs=many)
    assert r["motif_start"].dtype == np.int32 and r["motif_start"].tolist() == [[-2 ** 31, 2 ** 31 - 1]]
    assert r["motif_count"][0].tolist() == [1] * 32 and r["n_motifs"].tolist() == [32]
    everything = np.array([[-1, 0, 0, 0]], np.int32)  # every class, the sign bit = class 31
    r = run_motifs("AAAA", [1, 1, 1, 1], motifs=everything, tokens=np.array([[31, 32, -1, 0]]))
    assert r["motif_start"].tolist() == [[1, 0, 0, 1]] and r["n_motifs"].tolist() == [2]
    only31 = np.array([[-2 ** 31, 0, 0, 0]], np.int32)
    assert run_motifs("AAAA", [1, 1, 1, 1], motifs=only31, tokens=np.array([[31, 32, -1, 0]]))["motif_start"].tolist() == [[1, 0, 0, 0]]


# ------------------------------------------------------------------ motif_masks and the default tables
def test_motif_masks_every_syntax_form():
    bit = lambda letters: sum(1 << AA[c] for c in letters)
    m = metrics.motif_masks({"a": "N[^P][ST]", "b": "DP", "c": "C", "d": "A.[^AX]X"})
    assert m.dtype == torch.int32 and tuple(m.shape) == (4, 4) and m.device.type == "cpu"
    every = (1 << 21) - 1
    assert m.tolist() == [[bit("N"), every & ~bit("P"), bit("ST"), 0], [bit("D"), bit("P"), 0, 0], [bit("C"), 0, 0, 0],
                          [bit("A"), every, every & ~bit("AX"), bit("X")]]
    assert metrics.motif_masks("M").tolist() == [[bit("M"), 0, 0, 0]] and metrics.motif_masks(["M", "C"]).shape == (2, 4)
    assert metrics.motif_masks(".", V=32).tolist() == [[-1, 0, 0, 0]]  # 32 classes: the sign bit is class 31
    assert metrics.motif_masks("[^A]", V=20).tolist() == [[(1 << 20) - 2, 0, 0, 0]]
    assert metrics.motif_masks(metrics.LIABILITY_MOTIFS).tolist() == [
        [bit("N"), every & ~bit("P"), bit("ST"), 0], [bit("N"), bit("GS"), 0, 0], [bit("D"), bit("GS"), 0, 0], [bit("D"), bit("P"), 0, 0],
        [bit("C"), 0, 0, 0], [bit("M"), 0, 0, 0]]
    assert list(metrics.LIABILITY_MOTIFS) == ["n_glycosylation", "deamidation", "isomerisation", "fragmentation", "cysteine", "methionine"]


@pytest.mark.parametrize("patterns, kw, match", [
    ("", {}, "has 0 positions"), ("NASTA", {}, "has 5 positions"), ("n", {}, "no one-letter code"), ("B", {}, "no one-letter code"),
    ("N[ST", {}, r"a class is \[letters\]"), ("N[]", {}, r"a class is \[letters\]"), ("N[^]", {}, r"a class is \[letters\]"),
    ("N]", {}, "no one-letter code"), ("N[S.]", {}, "no one-letter code"), ("X", dict(V=20), "outside the V = 20 classes"),
    ("[^A]", dict(V=1), "matches no token class"), (5, {}, "patterns must be"), ([], {}, "patterns must be"), (["N", 5], {}, "must be a str"),
    (["A"] * 33, {}, "1 to 32 patterns"), ("N", dict(V=0), "V must be an int"), ("N", dict(V=33), "V must be an int"),
    ("N", dict(V=21.0), "V must be an int"),
])
def test_motif_masks_refuses_a_malformed_pattern(patterns, kw, match):
    with pytest.raises(ValueError, match=r"metrics\.motif_masks\(\): .*" + match):
        metrics.motif_masks(patterns, **kw)


def test_the_default_tables_are_the_numbers_of_the_issue():
    kd = dict(zip("ARNDCQEGHILKMFPSTWYV", (1.8, -4.5, -3.5, -3.5, 2.5, -3.5, -3.5, -0.4, -3.2, 4.5, 3.8, -3.9, 1.9, 2.8, -1.6, -0.8, -0.7, -0.9,
                                           -1.3, 4.2)))
    assert len(metrics.KYTE_DOOLITTLE) == len(metrics.RESIDUE_CHARGE) == len(dio.AA1) == 21 and dio.AA1[:20] == "ARNDCQEGHILKMFPSTWYV"
    for i, c in enumerate(dio.AA1[:20]):
        assert metrics.KYTE_DOOLITTLE[i] == 1 + (kd[c] + 4.5) / 9, c
    assert metrics.KYTE_DOOLITTLE[20] == 0 and min(metrics.KYTE_DOOLITTLE[:20]) == 1.0 and max(metrics.KYTE_DOOLITTLE) == 2.0
    assert metrics.KYTE_DOOLITTLE[AA["I"]] == 2.0 and metrics.KYTE_DOOLITTLE[AA["R"]] == 1.0
    want = {"D": -1.0, "E": -1.0, "K": 1.0, "R": 1.0, "H": 0.1}
    assert [metrics.RESIDUE_CHARGE[i] for i in range(21)] == [want.get(c, 0.0) for c in dio.AA1]
    sig = inspect.signature(metrics.patches).parameters
    assert sig["hydrophobicity"].default is metrics.KYTE_DOOLITTLE and sig["charge"].default is metrics.RESIDUE_CHARGE
    assert [sig[k].default for k in ("neighbour_distance", "vicinity_distance", "patch_distance", "min_distance")] == [10.0, 10.0, 7.5, 3.8]
    assert inspect.signature(metrics.liabilities).parameters["motifs"].default is metrics.LIABILITY_MOTIFS


# ------------------------------------------------------------------ the header, the library and the ctypes table
def header_code():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


def test_header_library_and_symbol_table_agree():
    """Every entry the header declares is in _hip.DEVELOP_SYMBOLS with the same arity and kinds, is exported, and is typed by
    load_library(); nothing else is in the table, and the table shares no name with the five older ones."""
    code = header_code()
    protos = dict(re.findall(r"\bint\s+(diffab_[a-z0-9_]+)\s*\((.*?)\)\s*;", code, flags=re.S))
    declared = sorted(set(re.findall(r"\b(diffab_[a-z0-9_]+)\s*\(", code)))
    assert declared == sorted(protos) == ["diffab_metrics_motifs", "diffab_metrics_patches"]
    assert sorted(_hip.DEVELOP_SYMBOLS) == declared, "DEVELOP_SYMBOLS and include/diffab_hip_develop.h drifted apart"
    older = set(_hip.SYMBOLS) | set(_hip.ANALYSIS_SYMBOLS) | set(_hip.HBOND_SYMBOLS) | set(_hip.CLUSTER_SYMBOLS) | set(_hip.INTERFACE_SYMBOLS)
    assert not set(_hip.DEVELOP_SYMBOLS) & older
    raw = ctypes.CDLL(_hip.LIB_PATH)
    typed = _hip.load_library()
    kinds = {"int32_t": ctypes.c_int32, "size_t": ctypes.c_size_t, "float": ctypes.c_float}
    for name, proto in protos.items():
        assert hasattr(raw, name), f"{name} is declared in include/diffab_hip_develop.h but not exported by libdiffab_hip.so"
        res, args = _hip.DEVELOP_SYMBOLS[name]
        fn = getattr(typed, name)
        assert fn.restype is res and list(fn.argtypes) == args  # load_library() types the sixth table onto the same CDLL object
        params = [p.strip() for p in proto.split(",")]
        assert res is ctypes.c_int and len(args) == len(params), name
        for p, a in zip(params, args):
            kind = p.rsplit(" ", 1)[0]
            if kind in kinds:
                assert a is kinds[kind], (name, p)
            else:
                assert "*" in kind and a is ctypes.c_void_p, (name, p)
    names = lambda n: [p.strip().rsplit(" ", 1)[1].lstrip("*") for p in protos[n].split(",")]
    assert names("diffab_metrics_patches") == [
        "sites", "context_sites", "tokens", "generation_mask", "residue_mask", "antigen_mask", "exposed_in", "hydrophobicity", "charge", "rows",
        "group_size", "K", "V", "neighbour_distance", "max_neighbours", "vicinity_distance", "patch_distance", "min_distance", "psh", "ppc", "pnc",
        "charge_generated", "charge_scope", "n_scope", "n_exposed", "n_pairs", "residue_psh", "residue_ppc", "residue_pnc", "n_neighbours",
        "state", "workspace", "workspace_bytes", "stream"]
    assert names("diffab_metrics_motifs") == ["tokens", "generation_mask", "residue_mask", "chain", "residue_idx", "motifs", "rows", "group_size",
                                               "K", "M", "motif_count", "n_motifs", "motif_start", "workspace", "workspace_bytes", "stream"]
    text = open(HEADER).read()
    assert '#include "diffab_hip.h"' in text and "Why a header of its own" in text.split("*/")[0]
    for macro, value in (("DIFFAB_DEVELOP_MAX_K", metrics.DEVELOP_MAX_K), ("DIFFAB_DEVELOP_MAX_CLASSES", metrics.DEVELOP_MAX_CLASSES),
                         ("DIFFAB_DEVELOP_MAX_MOTIFS", metrics.DEVELOP_MAX_MOTIFS), ("DIFFAB_DEVELOP_MOTIF_WORDS", metrics.DEVELOP_MOTIF_WORDS)):
        assert int(re.search(rf"#define\s+{macro}\s+(\d+)", code).group(1)) == value
    assert (metrics.DEVELOP_MAX_K, metrics.DEVELOP_MAX_CLASSES, metrics.DEVELOP_MAX_MOTIFS, metrics.DEVELOP_MOTIF_WORDS) == (512, 32, 32, 4)


SHAPES = [(1, 1), (1, 5), (2, 33), (3, 64), (16, 128), (256, 128), (7, 511), (4, 512), (3000000, 512)]
MACRO_C = r"""
#include <stdio.h>
#include "diffab_hip_develop.h"
int main(void) {
%s
  printf("%%d %%d %%d %%d %%d\n", DIFFAB_ERR_ARG, DIFFAB_DEVELOP_MAX_K, DIFFAB_DEVELOP_MAX_CLASSES, DIFFAB_DEVELOP_MAX_MOTIFS,
         DIFFAB_DEVELOP_MOTIF_WORDS);
  return 0;
}
"""


def test_workspace_macros_equal_the_python_mirrors(tmp_path):
    """The header compiles as C on its own (it brings diffab_hip.h along) and its macros give metrics.*_workspace_bytes."""
    cc = shutil.which("cc") or shutil.which("gcc") or next((p for p in ("/opt/rocm/llvm/bin/clang",) if os.path.exists(p)), None)
    assert cc, "no C compiler to read the header's macros with"
    src, exe = tmp_path / "macro.c", tmp_path / "macro"
    lines = [f'  printf("%zu\\n", DIFFAB_METRICS_PATCHES_WORKSPACE_BYTES({G}, {K}));' for G, K in SHAPES]
    lines += [f'  printf("%zu\\n", DIFFAB_METRICS_MOTIFS_WORKSPACE_BYTES({G}, {K}));' for G, K in SHAPES]
    src.write_text(MACRO_C % "\n".join(lines))
    subprocess.run([cc, "-I", os.path.join(REPO, "include"), str(src), "-o", str(exe)], check=True)
    got = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()
    want = [metrics.patches_workspace_bytes(*s) for s in SHAPES] + [metrics.motifs_workspace_bytes(*s) for s in SHAPES]
    assert [int(v) for v in got[:len(want)]] == want
    assert got[len(want):] == ["-1", "512", "32", "32", "4"]
    assert metrics.patches_workspace_bytes(3000000, 512) > 1 << 32 and metrics.motifs_workspace_bytes(3000000, 512) > 1 << 32
    assert metrics.patches_workspace_bytes(2, 33) == 2 * 33 * 16 + 1024 and metrics.motifs_workspace_bytes(2, 33) == 2 * 33 * 4 + 1024


PATCH_INPUTS = ("sites", "context_sites", "tokens", "generation_mask", "residue_mask", "antigen_mask", "exposed_in", "hydrophobicity", "charge")
PATCH_OUTPUTS = ("psh", "ppc", "pnc", "charge_generated", "charge_scope", "n_scope", "n_exposed", "n_pairs", "residue_psh", "residue_ppc",
                 "residue_pnc", "n_neighbours", "state")
MOTIF_INPUTS = ("tokens", "generation_mask", "residue_mask", "chain", "residue_idx")
MOTIF_OUTPUTS = ("motif_count", "n_motifs", "motif_start")


def test_host_side_refusals_touch_no_gpu():
    """Every refusal is decided from the scalar arguments, the host array of motif words and whether a pointer is null: the device
    pointers are fake addresses that are never dereferenced, nothing is enqueued (no GPU is needed), and diffab_last_error names the
    problem."""
    l = _hip.load_library()
    p, null = ctypes.c_void_p(4096), ctypes.c_void_p(0)
    err = lambda: l.diffab_last_error().decode()
    inf, nan = float("inf"), float("nan")

    def patches(rows=6, group=3, K=40, V=21, near=10.0, maxn=16, vic=10.0, patch=7.5, floor=3.8, ws=p, ws_bytes=1 << 40, **ptrs):
        a = dict.fromkeys(PATCH_INPUTS + PATCH_OUTPUTS, p)
        a.update(ptrs)
        return l.diffab_metrics_patches(*[a[k] for k in PATCH_INPUTS], rows, group, K, V, near, maxn, vic, patch, floor,
                                        *[a[k] for k in PATCH_OUTPUTS], ws, ws_bytes, null)

    for kw, word in ((dict(rows=-1), "extent"), (dict(group=0), "extent"), (dict(K=0), "extent"), (dict(group=4097, rows=4097), "at most 4096 designs"),
                     (dict(K=513), "K = 513 residues per patch, at most 512"), (dict(rows=7), "not a multiple"), (dict(V=0), "V = 0"),
                     (dict(V=33), "V = 33"), (dict(near=-1.0), "neighbour_distance"), (dict(near=inf), "neighbour_distance"),
                     (dict(near=nan), "neighbour_distance"), (dict(maxn=-1), "max_neighbours"), (dict(vic=-0.5), "vicinity_distance"),
                     (dict(vic=nan), "vicinity_distance"), (dict(patch=-7.5), "patch_distance"), (dict(patch=inf), "patch_distance"),
                     (dict(floor=0.0), "min_distance"), (dict(floor=-1.0), "min_distance"), (dict(floor=inf), "min_distance"),
                     (dict(floor=nan), "min_distance"), (dict(floor=1e-30), "min_distance"), (dict(floor=1e30), "min_distance"),
                     (dict(sites=null), "null input"), (dict(context_sites=null), "null input"), (dict(tokens=null), "null input"),
                     (dict(generation_mask=null), "null input"), (dict(hydrophobicity=null), "null input"), (dict(charge=null), "null input"),
                     (dict(ws=null), "workspace"), (dict(ws=ctypes.c_void_p(4096 + 16)), "256-byte aligned")):
        rc = patches(**kw)
        assert rc == -1 and word in err() and err().startswith("metrics_patches:"), (kw, rc, err())
    need = metrics.patches_workspace_bytes(2, 40)
    assert patches(ws_bytes=need // 2) == -4 and "needed" in err() and err().startswith("metrics_patches:")  # DIFFAB_ERR_WORKSPACE
    assert need - 1024 <= int(re.search(r"(\d+) needed", err()).group(1)) <= need
    ok = [dict(K=512), dict(K=1), dict(group=1), dict(rows=4096, group=4096), dict(V=1), dict(V=32), dict(near=0.0, vic=0.0, patch=0.0),
          dict(maxn=0), dict(maxn=2 ** 31 - 1), dict(residue_mask=null, antigen_mask=null, exposed_in=null), dict.fromkeys(PATCH_OUTPUTS, null)]
    for kw in ok:  # accepted as far as the workspace check, the last one before the launches
        assert patches(ws_bytes=16, **kw) == -4 and "needed" in err(), kw
    assert l.diffab_metrics_patches(*[null] * 9, 0, 5, 128, 21, 10.0, 16, 10.0, 7.5, 3.8, *[null] * 13, null, 0, null) == 0  # an empty problem

    words = lambda *w: (ctypes.c_int32 * len(w))(*w)
    good = words(4, 0, 0, 0, 1, 2, 3, 4, -1, 8, 0, 0)

    def motifs(rows=6, group=3, K=40, M=3, table=good, ws=p, ws_bytes=1 << 40, **ptrs):
        a = dict.fromkeys(MOTIF_INPUTS + MOTIF_OUTPUTS, p)
        a.update(ptrs)
        host = null if table is None else ctypes.cast(table, ctypes.c_void_p)
        return l.diffab_metrics_motifs(*[a[k] for k in MOTIF_INPUTS], host, rows, group, K, M, *[a[k] for k in MOTIF_OUTPUTS], ws, ws_bytes, null)

    for kw, word in ((dict(rows=-1), "extent"), (dict(group=0), "extent"), (dict(K=0), "extent"), (dict(group=4097, rows=4097), "at most 4096 designs"),
                     (dict(K=513), "K = 513 residues per patch, at most 512"), (dict(rows=7), "not a multiple"), (dict(M=0), "M = 0"),
                     (dict(M=33), "M = 33"), (dict(tokens=null), "null input"), (dict(generation_mask=null), "null input"),
                     (dict(chain=null), "null input"), (dict(residue_idx=null), "null input"), (dict(table=None), "null motifs"),
                     (dict(table=words(4, 0, 0, 0, 0, 2, 0, 0), M=2), "word 0 of motif 1 is zero"),
                     (dict(table=words(0, 0, 0, 0), M=1), "word 0 of motif 0 is zero"),
                     (dict(table=words(4, 0, 8, 0), M=1), "word 2 of motif 0 is non-zero after a zero word"),
                     (dict(table=words(4, 1, 0, 0, 4, 1, 0, -1), M=2), "word 3 of motif 1 is non-zero after a zero word"),
                     (dict(ws=null), "workspace"), (dict(ws=ctypes.c_void_p(4096 + 128)), "256-byte aligned")):
        rc = motifs(**kw)
        assert rc == -1 and word in err() and err().startswith("metrics_motifs:"), (kw, rc, err())
    need = metrics.motifs_workspace_bytes(2, 40)
    assert motifs(ws_bytes=2 * 40 * 4 - 1) == -4 and "needed" in err() and err().startswith("metrics_motifs:")
    assert need - 1024 <= int(re.search(r"(\d+) needed", err()).group(1)) <= need
    for kw in (dict(K=512), dict(K=1), dict(group=1), dict(rows=4096, group=4096), dict(M=1), dict(M=2), dict(residue_mask=null),
               dict(table=words(*[1] * 128), M=32), dict.fromkeys(MOTIF_OUTPUTS, null)):
        assert motifs(ws_bytes=16, **kw) == -4 and "needed" in err(), kw
    assert l.diffab_metrics_motifs(*[null] * 6, 0, 5, 128, 3, null, null, null, null, 0, null) == 0  # an empty problem: motifs is not read


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
    return dict(designs=designs, generation_mask=gm, group_size=N)


def test_good_arguments_reach_the_library(no_library):
    a = good()
    context = {"xyz": torch.zeros(2, 8, 15, 3), "atom_mask": torch.ones(2, 8, 15)}
    for kw in ({}, dict(context=context), dict(residue_mask=torch.ones(2, 8, dtype=torch.bool)), dict(antigen_mask=torch.zeros(2, 8, dtype=torch.bool)),
               dict(exposed=torch.ones(4, 8, dtype=torch.bool)), dict(hydrophobicity=[1.0] * 5, charge=torch.zeros(5)), dict(max_neighbours=0),
               dict(neighbour_distance=8, vicinity_distance=0, patch_distance=0.0, min_distance=1e-3),
               dict(context={"xyz": torch.zeros(2, 8, 2, 3), "atom_mask": torch.ones(2, 8, 2, dtype=torch.bool)})):
        with pytest.raises(ReachedTheLibrary):
            metrics.patches(**{**a, **kw})
    for kw in ({}, dict(motifs={"x": "C"}), dict(chain_idx=torch.zeros(8, dtype=torch.long)), dict(residue_idx=torch.arange(8).expand(2, 8)),
               dict(residue_mask=torch.ones(2, 8, dtype=torch.bool)), dict(V=20, motifs={"x": "[^C]"}), dict(motifs={str(i): "A" for i in range(32)})):
        with pytest.raises(ReachedTheLibrary):
            metrics.liabilities(**{**a, **kw})
    with pytest.raises(ReachedTheLibrary):
        metrics.patches(**good(rows=1, K=512, N=1))
    with pytest.raises(ReachedTheLibrary):
        metrics.liabilities(**good(rows=1, K=512, N=1))
    d = good()
    del d["designs"]["orientations"]  # liabilities reads the sequence only
    with pytest.raises(ReachedTheLibrary):
        metrics.liabilities(**d)


@pytest.mark.parametrize("kw, match", [
    (dict(antigen_mask=torch.ones(2, 8)), "antigen_mask must be a bool tensor"),
    (dict(antigen_mask=torch.ones(2, 7, dtype=torch.bool)), r"antigen_mask is \(2, 7\), expected \(2, 8\)"),
    (dict(generation_mask=torch.ones(2, 8)), "generation_mask must be a bool tensor"),
    (dict(generation_mask=torch.ones(4, 8, dtype=torch.bool)), "generation_mask is"),
    (dict(residue_mask=torch.ones(2, 8)), "residue_mask must be a bool tensor"), (dict(residue_mask=torch.ones(8, dtype=torch.bool)), "residue_mask is"),
    (dict(group_size=3), "4 design rows are not a multiple of group_size = 3"), (dict(group_size=0), "group_size must be an int >= 1"),
    (dict(group_size=2.0), "group_size must be an int"), (dict(designs={"seq_idx": torch.zeros(4, 8)}), "designs must be a dict"),
    (dict(designs=dict(seq_idx=torch.zeros(4, 8), translations=torch.zeros(4, 8, 3), orientations=torch.zeros(4, 8, 3, 3))), "seq_idx.* must be an integer"),
    (dict(designs=dict(seq_idx=torch.zeros(4, 8, dtype=torch.long), translations=torch.zeros(4, 8, 3))), "orientations"),
    (dict(exposed=torch.ones(4, 8)), "exposed must be a bool tensor"), (dict(exposed=torch.ones(2, 8, dtype=torch.bool)), r"exposed must be a bool tensor \(4, 8\)"),
    (dict(hydrophobicity=[]), "hydrophobicity must be a sequence"), (dict(hydrophobicity=[1.0] * 33, charge=[0.0] * 33), "hydrophobicity must be"),
    (dict(hydrophobicity="kd"), "hydrophobicity must be"), (dict(hydrophobicity=torch.ones(3, 7)), "hydrophobicity must be"),
    (dict(hydrophobicity=[1.0, float("nan")], charge=[0.0, 0.0]), "hydrophobicity must hold finite numbers"),
    (dict(charge=[0.0] * 20), "hydrophobicity has 21 classes and charge 20"), (dict(charge=[float("inf")] * 21), "charge must hold finite"),
    (dict(charge=None), "charge must be"), (dict(neighbour_distance=-1.0), "neighbour_distance must be a finite number >= 0"),
    (dict(neighbour_distance="10"), "neighbour_distance"), (dict(vicinity_distance=float("inf")), "vicinity_distance"),
    (dict(patch_distance=float("nan")), "patch_distance"), (dict(min_distance=0.0), "min_distance must be a finite number > 0"),
    (dict(min_distance=-3.8), "min_distance"), (dict(max_neighbours=-1), "max_neighbours must be an int >= 0"),
    (dict(max_neighbours=16.0), "max_neighbours must be an int"), (dict(max_neighbours=True), "max_neighbours must be an int"),
    (dict(context={"xyz": torch.zeros(2, 8, 15, 3)}), "context must be a dict"),
    (dict(context={"xyz": torch.zeros(2, 8, 1, 3), "atom_mask": torch.ones(2, 8, 1)}), r"A = 1 atoms per residue: slot 1 \(CA\) is needed"),
    (dict(context={"xyz": torch.zeros(2, 8, 33, 3), "atom_mask": torch.ones(2, 8, 33)}), r"A = 33 atoms per residue, outside \[1, 32\]"),
    (dict(context={"xyz": torch.zeros(2, 7, 15, 3), "atom_mask": torch.ones(2, 7, 15)}), r"context\['xyz'\] is"),
    (dict(context={"xyz": torch.zeros(2, 8, 15, 3), "atom_mask": torch.ones(2, 8, 14)}), r"context\['atom_mask'\] is"),
])
def test_patches_argument_errors(no_library, kw, match):
    args = good()
    args.update(kw)
    with pytest.raises(ValueError, match=r"metrics\.patches\(\): .*" + match):
        metrics.patches(**args)


@pytest.mark.parametrize("kw, match", [
    (dict(generation_mask=torch.ones(2, 8)), "generation_mask must be a bool tensor"), (dict(residue_mask=torch.ones(8, dtype=torch.bool)), "residue_mask is"),
    (dict(group_size=3), "4 design rows are not a multiple of group_size = 3"), (dict(group_size=True), "group_size must be an int"),
    (dict(designs={"seq_idx": torch.zeros(4, 8)}), "designs must be a dict"), (dict(motifs="N[GS]"), "motifs must be a dict"),
    (dict(motifs={}), "motifs must be a dict of 1 to 32"), (dict(motifs={str(i): "A" for i in range(33)}), "motifs must be a dict of 1 to 32"),
    (dict(motifs={1: "A"}), "motifs must be a dict"), (dict(motifs={"n_motifs": "A"}), "'n_motifs' names an output"),
    (dict(motifs={"motif_start": "A"}), "'motif_start' names an output"), (dict(motifs={"x": "NASTA"}), r"motifs: metrics\.motif_masks\(\): .*5 positions"),
    (dict(motifs={"x": "N[S"}), "motifs: .*a class is"), (dict(motifs={"x": "X"}, V=20), "motifs: .*outside the V = 20 classes"),
    (dict(V=33), "motifs: .*V must be an int"), (dict(chain_idx=torch.zeros(8)), "needs an integer chain_idx"),
    (dict(chain_idx=torch.zeros(3, 8, dtype=torch.long)), "chain_idx .* does not broadcast"),
    (dict(residue_idx=torch.zeros(7, dtype=torch.long)), "residue_idx .* does not broadcast"),
])
def test_liabilities_argument_errors(no_library, kw, match):
    args = good()
    args.update(kw)
    with pytest.raises(ValueError, match=r"metrics\.liabilities\(\): .*" + match):
        metrics.liabilities(**args)


def test_k_over_the_limit_is_refused(no_library):
    with pytest.raises(ValueError, match=r"metrics\.patches\(\): K = 513 residues per patch, at most 512"):
        metrics.patches(**good(rows=1, K=513, N=1))
    with pytest.raises(ValueError, match=r"metrics\.liabilities\(\): K = 513 residues per patch, at most 512"):
        metrics.liabilities(**good(rows=1, K=513, N=1))


def test_signatures_and_constants():
    sig = inspect.signature(metrics.patches)
    assert list(sig.parameters) == ["designs", "generation_mask", "context", "antigen_mask", "residue_mask", "group_size", "exposed", "hydrophobicity",
                                    "charge", "neighbour_distance", "max_neighbours", "vicinity_distance", "patch_distance", "min_distance"]
    assert all(sig.parameters[k].kind is inspect.Parameter.KEYWORD_ONLY for k in list(sig.parameters)[2:])
    sig = inspect.signature(metrics.liabilities)
    assert list(sig.parameters) == ["designs", "generation_mask", "motifs", "chain_idx", "residue_idx", "residue_mask", "group_size", "V"]
    assert all(sig.parameters[k].kind is inspect.Parameter.KEYWORD_ONLY for k in list(sig.parameters)[2:])
    assert list(inspect.signature(metrics.motif_masks).parameters) == ["patterns", "V"] and inspect.signature(metrics.motif_masks).parameters["V"].default == 21
    for word in ("``patches``", "``liabilities``", "develop_kernels.hip", "include/diffab_hip_develop.h"):
        assert word in metrics.__doc__, word
