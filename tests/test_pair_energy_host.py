"""The binding score without a GPU: the numpy restatement of pair_energy_ref.py on hand-made cases with the
answers written out, contact_potential and PairPotential, the header / library / ctypes table of include/diffab_hip_energy.h, the
workspace macro, the host-side refusals of the entry and the Python argument errors, raised before the library is loaded."""
import ctypes
import dataclasses
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
from pair_energy_ref import ANTIGEN, FRAMEWORK, INTERNAL, bound, pair_energy_ref, ulp32
from sampler_support import ReachedTheLibrary, refuse_library

HEADER = os.path.join(REPO, "include", "diffab_hip_energy.h")
f32 = np.float32
EDGES = (0.0, 5.0, 7.0, 9.0)
# asymmetric, and another power of ten per bin: table[b][a][c] = 100^b * (10 a + c + 1), V = 4
TABLE = np.array([[[100.0 ** b * (10 * a + c + 1) for c in range(4)] for a in range(4)] for b in range(3)], f32)


def line(xs, tokens, gen, antigen=None, rm=None, chain=None, ridx=None, **kw):
    """One row, residues on the x axis; the row's sites and the patch's sites are the same points."""
    xs = np.asarray(xs, f32)
    sites = np.zeros((1, len(xs), 3), f32)
    sites[0, :, 0] = xs
    one = lambda v, kind: None if v is None else np.asarray([v], kind)
    args = dict(table=TABLE, bin_edges=EDGES, min_separation=3)
    args.update(kw)
    return pair_energy_ref(sites, sites, np.asarray([tokens]), np.asarray([gen], bool), one(rm, bool), one(antigen, bool), one(chain, int),
                           one(ridx, int), **args)


def pairs(r):
    """{(class, bin): count} of the one row, the zero counts left out."""
    return {(c, b): int(n) for (c, b), n in np.ndenumerate(r["n_pairs"][0]) if n}


# ------------------------------------------------------------------ hand-made cases with the answers written out
def test_a_pair_at_an_edge_is_in_the_upper_bin_and_one_ulp_inside_in_the_lower():
    inside = float(np.nextafter(f32(5.0), f32(0)))
    assert f32(inside) * f32(inside) < f32(25.0)
    at = line([0.0, 5.0], [1, 2], [1, 0], antigen=[0, 1])
    assert pairs(at) == {(ANTIGEN, 1): 1} and at["e_antigen_f64"][0] == 100.0 * 13 and at["e_antigen"].dtype == f32
    below = line([0.0, inside], [1, 2], [1, 0], antigen=[0, 1])
    assert pairs(below) == {(ANTIGEN, 0): 1} and below["e_antigen_f64"][0] == 13.0
    # at the last edge the pair is out; one ulp inside it is in the last bin
    assert pairs(line([0.0, 9.0], [1, 2], [1, 0], antigen=[0, 1])) == {}
    last = line([0.0, float(np.nextafter(f32(9.0), f32(0)))], [1, 2], [1, 0], antigen=[0, 1])
    assert pairs(last) == {(ANTIGEN, 2): 1} and last["e_antigen_f64"][0] == 10000.0 * 13
    # coincident sites with bin_edges[0] = 0 are counted; with a first edge above 0 they are below every bin
    same = line([3.0, 3.0], [1, 2], [1, 0])
    assert pairs(same) == {(FRAMEWORK, 0): 1} and same["e_framework_f64"][0] == 13.0 and same["n_partners"].tolist() == [[1, 1]]
    assert pairs(line([3.0, 3.0], [1, 2], [1, 0], bin_edges=(1.0, 5.0, 7.0, 9.0))) == {}
    assert pairs(line([3.0, 4.0], [1, 2], [1, 0], bin_edges=(1.0, 5.0, 7.0, 9.0))) == {(FRAMEWORK, 0): 1}  # d = 1 = the first edge


def test_min_separation_at_the_boundary_across_chains_absent_and_out_of_order():
    xs, tokens, gen = [0.0, 1.0], [1, 2], [1, 0]
    near = lambda **kw: pairs(line(xs, tokens, gen, **kw))
    assert near(chain=[0, 0], ridx=[10, 12]) == {}  # |10 - 12| = 2 < 3
    assert near(chain=[0, 0], ridx=[10, 13]) == {(FRAMEWORK, 0): 1}  # 3 is not below 3
    assert near(chain=[0, 0], ridx=[13, 10]) == {(FRAMEWORK, 0): 1} and near(chain=[0, 0], ridx=[12, 10]) == {}
    assert near(chain=[0, 0], ridx=[10, 12], min_separation=2) == {(FRAMEWORK, 0): 1} and near(chain=[0, 0], ridx=[10, 10], min_separation=0) != {}
    assert near(chain=[0, 1], ridx=[10, 10]) == {(FRAMEWORK, 0): 1}  # two chains with equal numbering
    assert near() == {(FRAMEWORK, 0): 1}  # without chain / residue_idx nothing is skipped
    assert near(chain=[0, 0], ridx=[-2 ** 31, 2 ** 31 - 1]) == {(FRAMEWORK, 0): 1}  # the difference is taken in 64 bits
    # slots out of order: slots 0 and 2 are chain neighbours, slots 0 and 1 are not
    r = line([0.0, 1.0, 2.0], [1, 2, 3], [1, 0, 0], chain=[0, 0, 0], ridx=[10, 50, 11])
    assert r["n_partners"].tolist() == [[1, 1, 0]] and r["e_framework_f64"][0] == 13.0


def test_an_asymmetric_table_puts_the_generated_residue_first_and_the_lower_slot_for_internal_pairs():
    for xs, tokens, gen, antigen in (([0.0, 1.0], [1, 2], [1, 0], [0, 1]), ([0.0, 1.0], [2, 1], [0, 1], [1, 0])):
        r = line(xs, tokens, gen, antigen=antigen)  # generated token 1, antigen token 2, in either slot order
        assert r["e_antigen_f64"][0] == 13.0 and pairs(r) == {(ANTIGEN, 0): 1}
        assert r["residue_energy_f64"][0].tolist() == [13.0, 13.0] and r["residue_antigen_energy_f64"][0].tolist() == [13.0, 13.0]
    r = line([0.0, 1.0], [1, 2], [1, 0])  # the same against the framework
    assert r["e_framework_f64"][0] == 13.0 and r["e_antigen"][0] == 0 and r["residue_antigen_energy"][0].tolist() == [0, 0]
    r = line([0.0, 1.0], [2, 1], [1, 1])  # internal: the lower slot (token 2) first
    assert r["e_internal_f64"][0] == 22.0 and pairs(r) == {(INTERNAL, 0): 1} and r["residue_energy_f64"][0].tolist() == [22.0, 22.0]
    assert line([0.0, 1.0], [1, 2], [1, 1])["e_internal_f64"][0] == 13.0
    # three classes at once, every pair once: g(1) - a(2) at 1 A, g(1) - f(3) at 6 A, g(1) - g(0) at 8 A, g(0) - a(2) at 7 A
    r = line([0.0, 1.0, -6.0, 8.0], [1, 2, 3, 0], [1, 0, 0, 1], antigen=[0, 1, 0, 0])
    assert pairs(r) == {(ANTIGEN, 0): 1, (ANTIGEN, 2): 1, (FRAMEWORK, 1): 1, (INTERNAL, 2): 1}
    assert r["e_antigen_f64"][0] == 13.0 + 10000.0 * 3 and r["e_framework_f64"][0] == 100.0 * 14 and r["e_internal_f64"][0] == 10000.0 * 11
    assert r["n_partners"].tolist() == [[3, 2, 1, 2]]
    assert r["residue_energy_f64"][0].tolist() == [13.0 + 1400.0 + 110000.0, 13.0 + 30000.0, 1400.0, 110000.0 + 30000.0]
    assert r["residue_antigen_energy_f64"][0].tolist() == [13.0, 13.0 + 30000.0, 0.0, 30000.0]
    assert r["sum_abs"]["e_antigen"][0] == 30013.0 and r["sum_abs"]["residue_energy"][0, 2] == 1400.0


def test_a_generated_residue_inside_antigen_mask_counts_as_generated():
    r = line([0.0, 1.0, 2.0], [1, 2, 3], [1, 1, 0], antigen=[0, 1, 1])
    assert pairs(r) == {(INTERNAL, 0): 1, (ANTIGEN, 0): 2} and r["e_internal_f64"][0] == 13.0 and r["e_antigen_f64"][0] == 14.0 + 24.0
    assert r["substitution"][0, 1].tolist() == [4.0 - 24.0, 14.0 - 24.0, 0.0, 34.0 - 24.0]  # slot 1 is scanned like any generated residue


def test_a_token_outside_the_table_on_either_end_drops_the_pair():
    for bad in (4, -1, 1000):
        assert pairs(line([0.0, 1.0], [bad, 2], [1, 0], antigen=[0, 1])) == {} and pairs(line([0.0, 1.0], [1, bad], [1, 0], antigen=[0, 1])) == {}
        r = line([0.0, 1.0, 2.0], [1, bad, 2], [1, 1, 0])
        assert pairs(r) == {(FRAMEWORK, 0): 1} and r["n_partners"].tolist() == [[1, 0, 1]]


def test_the_substitution_scan():
    # generated slot 0 (token 1) with antigen partners of token 2 at 1 A (bin 0) and token 3 at 6 A (bin 1); a framework residue nearby
    r = line([0.0, 1.0, 6.0, -1.0], [1, 2, 3, 0], [1, 0, 0, 0], antigen=[0, 1, 1, 0])
    S = [(10 * v + 2 + 1) + 100.0 * (10 * v + 3 + 1) for v in range(4)]
    assert r["substitution_f64"][0, 0].tolist() == [s - S[1] for s in S] and r["substitution"][0, 0, 1] == 0
    assert (r["substitution"][0, 1:] == 0).all() and r["substitution"].shape == (1, 4, 4) and r["substitution"].dtype == f32
    assert r["e_antigen_f64"][0] == S[1]
    assert r["sum_abs"]["substitution"][0, 0].tolist() == [s + S[1] for s in S]
    # the residue's own token outside the table: no pair is counted, S_cur = 0, the scan says what a known token would add
    r = line([0.0, 1.0, 6.0, -1.0], [7, 2, 3, 0], [1, 0, 0, 0], antigen=[0, 1, 1, 0])
    assert r["e_antigen"][0] == 0 and pairs(r) == {} and r["substitution_f64"][0, 0].tolist() == S
    # an antigen partner with a token outside the table, one nearer than min_separation and one without a bin are no partners
    r = line([0.0, 1.0, 6.0, 20.0], [1, 9, 3, 2], [1, 0, 0, 0], antigen=[0, 1, 1, 1], chain=[0, 1, 0, 1], ridx=[5, 5, 6, 5])
    assert (r["substitution"] == 0).all() and pairs(r) == {}
    assert "substitution" not in line([0.0, 1.0], [1, 2], [1, 0], substitutions=False)


def test_absent_residues_are_ignored_whatever_their_sites_hold():
    xs, tokens, gen, antigen = [0.0, 1.0, 2.0, 3.0], [1, 2, 3, 0], [1, 0, 1, 0], [0, 1, 0, 1]
    rm = [1, 1, 0, 0]
    with_nan = line([0.0, 1.0, np.nan, np.nan], tokens, gen, antigen=antigen, rm=rm)
    plain = line(xs, tokens, gen, antigen=antigen, rm=rm)
    two = line(xs[:2], tokens[:2], gen[:2], antigen=antigen[:2])
    for k in ("e_antigen", "e_framework", "e_internal", "n_pairs"):
        assert np.array_equal(with_nan[k], plain[k]) and np.array_equal(plain[k], two[k]), k
    assert plain["n_partners"].tolist() == [[1, 1, 0, 0]] and (plain["substitution"][0, 2:] == 0).all() and pairs(plain) == {(ANTIGEN, 0): 1}
    # the row's sites of non-generated residues and the patch's sites of generated ones are not read
    sites = np.zeros((1, 2, 3), f32)
    sites[0, 1] = np.nan
    csites = np.full((1, 2, 3), np.nan, f32)
    csites[0, 1] = (1.0, 0.0, 0.0)
    r = pair_energy_ref(sites, csites, np.array([[1, 2]]), np.array([[1, 0]], bool), table=TABLE, bin_edges=EDGES)
    assert r["e_framework_f64"][0] == 13.0


def test_the_bound_of_the_real_valued_comparison():
    assert ulp32(1.0) == 2.0 ** -23 and ulp32(-3.0) == 2.0 ** -22 and ulp32(0.0) == float(np.spacing(np.finfo(f32).tiny))
    assert bound(np.array([1.0]), np.array([2.0 ** 10]))[0] == 2.0 ** -23 + 2.0 ** -24


# ------------------------------------------------------------------ contact_potential and PairPotential
def test_contact_potential_against_its_formula():
    p = metrics.contact_potential()
    assert isinstance(p, metrics.PairPotential) and p.bin_edges == (0.0, 6.5, 9.0)
    assert p.table.dtype == torch.float32 and tuple(p.table.shape) == (2, 21, 21) and p.table.device.type == "cpu"
    h, q = np.array(metrics.KYTE_DOOLITTLE, f32).astype(np.float64), np.array(metrics.RESIDUE_CHARGE, f32).astype(np.float64)
    for b, scale in enumerate((1.0, 0.5)):
        for a in range(21):
            for c in range(21):
                want = 0.0 if a == 20 or c == 20 else scale * (-(h[a] - 1) * (h[c] - 1) + q[a] * q[c])
                assert float(p.table[b, a, c]) == float(f32(want)), (b, a, c)
    t = p.table.numpy()
    AA = {c: i for i, c in enumerate(dio.AA1)}
    assert np.array_equal(t, t.transpose(0, 2, 1)) and (t[:, 20] == 0).all() and (t[:, :, 20] == 0).all()
    assert t[0, AA["I"], AA["I"]] == -1.0 and t[0, AA["D"], AA["K"]] < 0 < t[0, AA["D"], AA["E"]] and t[0, AA["R"], AA["R"]] == 1.0
    # a caller's own numbers
    p = metrics.contact_potential([1.0, 2.0, 0.0], [0.0, 1.0, -1.0], bin_edges=(2.0, 4.0), bin_scale=(3.0,), hydrophobic=2.0, electrostatic=0.5)
    assert p.table.tolist() == [[[0.0, 0.0, 0.0], [0.0, 3.0 * (-2.0 + 0.5), 0.0], [0.0, 0.0, 0.0]]] and p.bin_edges == (2.0, 4.0)
    sig = inspect.signature(metrics.contact_potential).parameters
    assert sig["hydrophobicity"].default is metrics.KYTE_DOOLITTLE and sig["charge"].default is metrics.RESIDUE_CHARGE
    assert [sig[k].default for k in ("bin_edges", "bin_scale", "hydrophobic", "electrostatic")] == [(0.0, 6.5, 9.0), (1.0, 0.5), 1.0, 1.0]
    doc = " ".join(metrics.contact_potential.__doc__.split())
    for word in ("PROJECT'S OWN CHOICE", "placeholder", "not a fitted potential", "no predictive value", "Miyazawa-Jernigan", "propensity"):
        assert word in doc, word


@pytest.mark.parametrize("kw, match", [
    (dict(hydrophobicity=[]), "hydrophobicity must be"), (dict(charge=[0.0] * 20), "hydrophobicity has 21 classes and charge 20"),
    (dict(charge=[float("nan")] * 21), "charge must hold finite"), (dict(bin_scale=(1.0,)), r"bin_edges must be NB \+ 1 = 2 numbers"),
    (dict(bin_scale=()), "bin_scale must be 1 to 8"), (dict(bin_scale=(1.0, float("inf"))), "bin_scale must be"),
    (dict(bin_scale="ab"), "bin_scale must be"), (dict(bin_scale=(1.0,) * 9, bin_edges=tuple(range(10))), "bin_scale must be 1 to 8"),
    (dict(bin_edges=(0.0, 9.0, 6.5)), "strictly ascending"), (dict(hydrophobic=float("nan")), "hydrophobic must be a finite number"),
    (dict(electrostatic="1"), "electrostatic must be a finite number"), (dict(hydrophobic=True), "hydrophobic must be"),
])
def test_contact_potential_argument_errors(kw, match):
    with pytest.raises(ValueError, match=r"metrics\.contact_potential\(\): .*" + match):
        metrics.contact_potential(**kw)


def test_pair_potential_takes_what_as_tensor_takes():
    p = metrics.PairPotential([[1, 2], [3, 4]], [0, 5])
    assert p.table.dtype == torch.float32 and p.table.tolist() == [[[1.0, 2.0], [3.0, 4.0]]] and p.bin_edges == (0.0, 5.0)
    p = metrics.PairPotential(np.zeros((8, 32, 32)), torch.arange(9.0))
    assert tuple(p.table.shape) == (8, 32, 32) and p.bin_edges == tuple(float(i) for i in range(9))
    assert tuple(metrics.PairPotential(torch.ones(3, 1, 1, dtype=torch.float64), (1, 2, 3, 4.5)).table.shape) == (3, 1, 1)
    with pytest.raises(dataclasses.FrozenInstanceError):
        p.table = None


@pytest.mark.parametrize("table, edges, match", [
    ("mj", (0, 5), "table must be numbers"), (np.zeros(4), (0, 5), "table must be numbers"), (np.zeros((1, 1, 2, 2)), (0, 5), "table must be numbers"),
    (np.zeros((2, 3)), (0, 5), r"table is \(1, 2, 3\)"), (np.zeros((33, 33)), (0, 5), "1 <= V <= 32"), (np.zeros((9, 2, 2)), range(10), "1 <= NB <= 8"),
    (np.zeros((0, 2, 2)), (0,), "1 <= NB <= 8"), (np.ones((2, 2), bool), (0, 5), "table must be numbers"),
    ([[1.0, float("nan")], [0.0, 0.0]], (0, 5), "finite in float32"), ([[1e39, 0.0], [0.0, 0.0]], (0, 5), "finite in float32"),
    (np.zeros((2, 2)), (0, 5, 7), r"bin_edges must be NB \+ 1 = 2 numbers"), (np.zeros((2, 2)), 5.0, "bin_edges must be"),
    (np.zeros((2, 2)), "05", "bin_edges must be"), (np.zeros((2, 2)), (0, "5"), "bin_edges must be"), (np.zeros((2, 2)), (False, 5), "bin_edges must be"),
    (np.zeros((2, 2)), torch.zeros(2, 1), "bin_edges must be"), (np.zeros((2, 2)), (-1.0, 5.0), "finite, >= 0 and strictly ascending"),
    (np.zeros((2, 2)), (0.0, float("inf")), "finite, >= 0"), (np.zeros((2, 2)), (0.0, float("nan")), "finite, >= 0"),
    (np.zeros((2, 2)), (5.0, 5.0), "strictly ascending"), (np.zeros((2, 2)), (5.0, 5.0 + 1e-9), r"strictly ascending \(in float32\)"),
    (np.zeros((2, 2)), (0.0, 1e30), "float32 squares of bin_edges must be finite"),
    (np.zeros((2, 2)), (1e-30, 2e-30), "float32 squares of bin_edges must be finite and strictly ascending"),
])
def test_pair_potential_refuses(table, edges, match):
    with pytest.raises(ValueError, match=r"metrics\.PairPotential\(\): .*" + match):
        metrics.PairPotential(table, edges)


# ------------------------------------------------------------------ the header, the library and the ctypes table
def header_code():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


NAMES = ["sites", "context_sites", "tokens", "generation_mask", "residue_mask", "antigen_mask", "chain", "residue_idx", "table", "bin_edges", "rows",
         "group_size", "K", "V", "NB", "min_separation", "e_antigen", "e_framework", "e_internal", "n_pairs", "residue_energy",
         "residue_antigen_energy", "n_partners", "substitution", "workspace", "workspace_bytes", "stream"]


def test_header_library_and_symbol_table_agree():
    """Every entry the header declares is in _hip.ENERGY_SYMBOLS with the same arity and kinds, is exported, and is typed by
    load_library(); nothing else is in the table, and the table shares no name with the six older ones."""
    code = header_code()
    protos = dict(re.findall(r"\bint\s+(diffab_[a-z0-9_]+)\s*\((.*?)\)\s*;", code, flags=re.S))
    declared = sorted(set(re.findall(r"\b(diffab_[a-z0-9_]+)\s*\(", code)))
    assert declared == sorted(protos) == ["diffab_metrics_pair_energy"]
    assert sorted(_hip.ENERGY_SYMBOLS) == declared, "ENERGY_SYMBOLS and include/diffab_hip_energy.h drifted apart"
    older = (set(_hip.SYMBOLS) | set(_hip.ANALYSIS_SYMBOLS) | set(_hip.HBOND_SYMBOLS) | set(_hip.CLUSTER_SYMBOLS) | set(_hip.INTERFACE_SYMBOLS)
             | set(_hip.DEVELOP_SYMBOLS))
    assert not set(_hip.ENERGY_SYMBOLS) & older
    raw = ctypes.CDLL(_hip.LIB_PATH)
    typed = _hip.load_library()
    kinds = {"int32_t": ctypes.c_int32, "size_t": ctypes.c_size_t, "float": ctypes.c_float}
    for name, proto in protos.items():
        assert hasattr(raw, name), f"{name} is declared in include/diffab_hip_energy.h but not exported by libdiffab_hip.so"
        res, args = _hip.ENERGY_SYMBOLS[name]
        fn = getattr(typed, name)
        assert fn.restype is res and list(fn.argtypes) == args  # load_library() types the seventh table onto the same CDLL object
        params = [p.strip() for p in proto.split(",")]
        assert res is ctypes.c_int and len(args) == len(params), name
        for p, a in zip(params, args):
            kind = p.rsplit(" ", 1)[0]
            if kind in kinds:
                assert a is kinds[kind], (name, p)
            else:
                assert "*" in kind and a is ctypes.c_void_p, (name, p)
    assert [p.strip().rsplit(" ", 1)[1].lstrip("*") for p in protos["diffab_metrics_pair_energy"].split(",")] == NAMES
    text = open(HEADER).read()
    assert '#include "diffab_hip.h"' in text and "Why a header of its own" in text.split("*/")[0] and "applies word for word" in text.split("*/")[0]
    for macro, value in (("DIFFAB_ENERGY_MAX_K", metrics.ENERGY_MAX_K), ("DIFFAB_ENERGY_MAX_CLASSES", metrics.ENERGY_MAX_CLASSES),
                         ("DIFFAB_ENERGY_MAX_BINS", metrics.ENERGY_MAX_BINS)):
        assert int(re.search(rf"#define\s+{macro}\s+(\d+)", code).group(1)) == value
    assert (metrics.ENERGY_MAX_K, metrics.ENERGY_MAX_CLASSES, metrics.ENERGY_MAX_BINS) == (512, 32, 8)


SHAPES = [(1, 1), (1, 5), (2, 33), (3, 64), (16, 128), (256, 128), (7, 511), (4, 512), (3000000, 512)]  # test_developability_host.SHAPES
MACRO_C = r"""
#include <stdio.h>
#include "diffab_hip_energy.h"
int main(void) {
%s
  printf("%%d %%d %%d %%d %%d\n", DIFFAB_ERR_ARG, DIFFAB_ERR_WORKSPACE, DIFFAB_ENERGY_MAX_K, DIFFAB_ENERGY_MAX_CLASSES, DIFFAB_ENERGY_MAX_BINS);
  return 0;
}
"""


def test_workspace_macro_equals_the_python_mirror(tmp_path):
    """The header compiles as C on its own (it brings diffab_hip.h along) and its macro gives metrics.pair_energy_workspace_bytes."""
    cc = shutil.which("cc") or shutil.which("gcc") or next((p for p in ("/opt/rocm/llvm/bin/clang",) if os.path.exists(p)), None)
    assert cc, "no C compiler to read the header's macros with"
    src, exe = tmp_path / "macro.c", tmp_path / "macro"
    src.write_text(MACRO_C % "\n".join(f'  printf("%zu\\n", DIFFAB_METRICS_PAIR_ENERGY_WORKSPACE_BYTES({G}, {K}));' for G, K in SHAPES))
    subprocess.run([cc, "-std=c99", "-Wall", "-Werror", "-I", os.path.join(REPO, "include"), str(src), "-o", str(exe)], check=True)
    got = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()
    want = [metrics.pair_energy_workspace_bytes(*s) for s in SHAPES]
    assert [int(v) for v in got[:len(want)]] == want
    assert got[len(want):] == ["-1", "-4", "512", "32", "8"]
    assert metrics.pair_energy_workspace_bytes(3000000, 512) > 1 << 32 and metrics.pair_energy_workspace_bytes(2, 33) == 2 * 33 * 24 + 1024


INPUTS = tuple(NAMES[:9])
OUTPUTS = tuple(NAMES[16:24])


def test_host_side_refusals_touch_no_gpu():
    """Every refusal is decided from the scalar arguments, the host array of bin edges and whether a pointer is null: the device
    pointers are fake addresses that are never dereferenced, nothing is enqueued (no GPU is needed), and diffab_last_error names the
    problem."""
    l = _hip.load_library()
    p, null = ctypes.c_void_p(4096), ctypes.c_void_p(0)
    err = lambda: l.diffab_last_error().decode()
    inf, nan = float("inf"), float("nan")
    floats = lambda *v: (ctypes.c_float * len(v))(*v)

    def call(rows=6, group=3, K=40, V=21, NB=3, sep=3, edges=floats(0.0, 5.0, 7.0, 9.0), ws=p, ws_bytes=1 << 40, **ptrs):
        a = dict.fromkeys(INPUTS + OUTPUTS, p)
        a.update(ptrs)
        host = null if edges is None else ctypes.cast(edges, ctypes.c_void_p)
        return l.diffab_metrics_pair_energy(*[a[k] for k in INPUTS], host, rows, group, K, V, NB, sep, *[a[k] for k in OUTPUTS], ws, ws_bytes, null)

    for kw, word in ((dict(rows=-1), "extent"), (dict(group=0), "extent"), (dict(K=0), "extent"), (dict(group=4097, rows=4097), "at most 4096 designs"),
                     (dict(K=513), "K = 513 residues per patch, at most 512"), (dict(rows=7), "not a multiple"), (dict(V=0), "V = 0"),
                     (dict(V=33), "V = 33"), (dict(NB=0), "NB = 0"), (dict(NB=9), "NB = 9"), (dict(sep=-1), "min_separation"),
                     (dict(sites=null), "null input"), (dict(context_sites=null), "null input"), (dict(tokens=null), "null input"),
                     (dict(generation_mask=null), "null input"), (dict(table=null), "null input"), (dict(edges=None), "null bin_edges"),
                     (dict(chain=null), "chain and residue_idx go together"), (dict(residue_idx=null), "chain and residue_idx go together"),
                     (dict(edges=floats(0.0, 5.0, nan, 9.0)), "bin_edges[2] must be finite"), (dict(edges=floats(0.0, 5.0, 7.0, inf)), "bin_edges[3] must be finite"),
                     (dict(edges=floats(-1.0, 5.0, 7.0, 9.0)), "bin_edges[0] must be finite and >= 0"),
                     (dict(edges=floats(0.0, 5.0, 5.0, 9.0)), "strictly ascending"), (dict(edges=floats(0.0, 7.0, 5.0, 9.0)), "strictly ascending"),
                     (dict(edges=floats(0.0, 5.0, 7.0, 1e30)), "fp32 squares"), (dict(edges=floats(1e-30, 2e-30, 7.0, 9.0)), "fp32 squares"),
                     (dict(NB=1, edges=floats(9.0, 5.0)), "strictly ascending"),
                     (dict(ws=null), "workspace"), (dict(ws=ctypes.c_void_p(4096 + 16)), "256-byte aligned")):
        rc = call(**kw)
        assert rc == -1 and word in err() and err().startswith("metrics_pair_energy:"), (kw, rc, err())
    need = metrics.pair_energy_workspace_bytes(2, 40)
    assert call(ws_bytes=need // 2) == -4 and "needed" in err() and err().startswith("metrics_pair_energy:")  # DIFFAB_ERR_WORKSPACE
    assert need - 1024 <= int(re.search(r"(\d+) needed", err()).group(1)) <= need
    ok = [dict(K=512), dict(K=1), dict(group=1), dict(rows=4096, group=4096), dict(V=1), dict(V=32), dict(NB=1), dict(sep=0), dict(sep=2 ** 31 - 1),
          dict(NB=8, edges=floats(*range(9))), dict(edges=floats(3.0, 5.0, 7.0, 9.0)), dict(residue_mask=null, antigen_mask=null),
          dict(chain=null, residue_idx=null), dict.fromkeys(OUTPUTS, null)]
    for kw in ok:  # accepted as far as the workspace check, the last one before the launches
        assert call(ws_bytes=16, **kw) == -4 and "needed" in err(), kw
    assert l.diffab_metrics_pair_energy(*[null] * 10, 0, 5, 128, 21, 3, 3, *[null] * 8, null, 0, null) == 0  # an empty problem: no pointer is read


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


def native_of(G=2, K=8):
    return dict(seq_idx=torch.zeros(G, K, dtype=torch.long), translations=torch.zeros(G, K, 3), orientations=torch.eye(3).expand(G, K, 3, 3).clone())


def test_good_arguments_reach_the_library(no_library):
    a = good()
    context = {"xyz": torch.zeros(2, 8, 15, 3), "atom_mask": torch.ones(2, 8, 15)}
    for kw in ({}, dict(context=context), dict(residue_mask=torch.ones(2, 8, dtype=torch.bool)), dict(antigen_mask=torch.zeros(2, 8, dtype=torch.bool)),
               dict(potential=metrics.PairPotential(np.zeros((3, 3)), (0, 4))), dict(potential=metrics.contact_potential(bin_scale=(1.0, 0.5))),
               dict(min_separation=0), dict(substitutions=True), dict(native=native_of()),
               dict(chain_idx=torch.zeros(8, dtype=torch.long), residue_idx=torch.arange(8).expand(2, 8)),
               dict(context={"xyz": torch.zeros(2, 8, 2, 3), "atom_mask": torch.ones(2, 8, 2, dtype=torch.bool)})):
        with pytest.raises(ReachedTheLibrary):
            metrics.interface_energy(**{**a, **kw})
    with pytest.raises(ReachedTheLibrary):
        metrics.interface_energy(**good(rows=1, K=512, N=1))


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
    (dict(potential=np.zeros((2, 3, 3))), "potential must be a metrics.PairPotential"), (dict(potential="mj"), "potential must be a metrics.PairPotential"),
    (dict(min_separation=-1), "min_separation must be an int >= 0"), (dict(min_separation=3.0), "min_separation must be an int"),
    (dict(min_separation=True), "min_separation must be an int"), (dict(min_separation=2 ** 31), "min_separation must be an int"),
    (dict(substitutions=1), "substitutions must be a bool"), (dict(substitutions=None), "substitutions must be a bool"),
    (dict(chain_idx=torch.zeros(8, dtype=torch.long)), "chain_idx and residue_idx go together, residue_idx is missing"),
    (dict(residue_idx=torch.arange(8)), "chain_idx and residue_idx go together, chain_idx is missing"),
    (dict(chain_idx=torch.zeros(8), residue_idx=torch.arange(8)), "needs an integer chain_idx"),
    (dict(chain_idx=torch.zeros(3, 8, dtype=torch.long), residue_idx=torch.arange(8)), "chain_idx .* does not broadcast"),
    (dict(chain_idx=torch.zeros(8, dtype=torch.long), residue_idx=torch.zeros(7, dtype=torch.long)), "residue_idx .* does not broadcast"),
    (dict(native={"seq_idx": torch.zeros(2, 8)}), "native must be a dict"),
    (dict(native=dict(native_of(), seq_idx=torch.zeros(2, 8))), r"native\['seq_idx'\] must be an integer"),
    (dict(native=native_of(G=4)), r"native\['seq_idx'\] is \(4, 8\), expected \(2, 8\)"),
    (dict(native={k: v for k, v in native_of().items() if k != "orientations"}), r"native\['orientations'\]"),
    (dict(context={"xyz": torch.zeros(2, 8, 15, 3)}), "context must be a dict"),
    (dict(context={"xyz": torch.zeros(2, 8, 1, 3), "atom_mask": torch.ones(2, 8, 1)}), r"A = 1 atoms per residue: slot 1 \(CA\) is needed"),
    (dict(context={"xyz": torch.zeros(2, 8, 33, 3), "atom_mask": torch.ones(2, 8, 33)}), r"A = 33 atoms per residue, outside \[1, 32\]"),
    (dict(context={"xyz": torch.zeros(2, 7, 15, 3), "atom_mask": torch.ones(2, 7, 15)}), r"context\['xyz'\] is"),
    (dict(context={"xyz": torch.zeros(2, 8, 15, 3), "atom_mask": torch.ones(2, 8, 14)}), r"context\['atom_mask'\] is"),
])
def test_interface_energy_argument_errors(no_library, kw, match):
    args = good()
    args.update(kw)
    with pytest.raises(ValueError, match=r"metrics\.interface_energy\(\): .*" + match):
        metrics.interface_energy(**args)


def test_k_over_the_limit_is_refused(no_library):
    with pytest.raises(ValueError, match=r"metrics\.interface_energy\(\): K = 513 residues per patch, at most 512"):
        metrics.interface_energy(**good(rows=1, K=513, N=1))


def test_signatures_and_constants():
    sig = inspect.signature(metrics.interface_energy)
    assert list(sig.parameters) == ["designs", "generation_mask", "context", "antigen_mask", "residue_mask", "chain_idx", "residue_idx", "group_size",
                                    "potential", "min_separation", "substitutions", "native"]
    assert all(sig.parameters[k].kind is inspect.Parameter.KEYWORD_ONLY for k in list(sig.parameters)[2:])
    assert [sig.parameters[k].default for k in ("group_size", "potential", "min_separation", "substitutions", "native")] == [1, None, 3, False, None]
    assert list(inspect.signature(metrics.PairPotential).parameters) == ["table", "bin_edges"]
    for word in ("``interface_energy``", "``PairPotential``", "``contact_potential``", "energy_kernels.hip", "include/diffab_hip_energy.h"):
        assert word in metrics.__doc__, word
    doc = " ".join(metrics.interface_energy.__doc__.split())
    assert "SAME site model" in doc and "not its real CB" in doc
