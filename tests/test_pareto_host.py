"""Pareto ranking without a GPU: the numpy oracles of diffab_metrics_pareto, hand cases with the answer written out, the properties of
the rule, the header / library / ctypes table, the workspace macro, the host-side refusals and the Python argument errors.

The rule is DESIGN.md section 4.22 / the header comment of the entry in include/diffab_hip_cluster.h.  `pareto_ref` restates it by brute
force: a boolean dominance matrix from the definition, peeled by recounting the open dominators of every design at every front.
`pareto_ref_chain` is the longest-chain recursion - rank[j] = 1 + the largest rank among j's dominators, visiting the designs by
increasing dominator count (a dominator always has strictly fewer dominators, so that is a topological order) - and serves large N;
`ref` runs both and asserts them equal, and every host case goes through it, so test_gpu_pareto.py may use the recursion above 1000
designs.  test_gpu_pareto.py imports the oracles and the data from here."""
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
from sampler_support import ReachedTheLibrary, refuse_library

HEADER = os.path.join(REPO, "include", "diffab_hip_cluster.h")
f32 = np.float32
INPUTS = ("objectives", "maximize", "violation", "score", "candidates")  # the order of the C prototype
OUTPUTS = ("rank", "n_dominators", "n_dominated", "front_size", "count", "n_unranked", "order")
nan, inf = np.nan, np.inf


# ------------------------------------------------------------------ the oracles
def keys(objectives, maximize=None, violation=None):
    """v (N,M) and w (N): the stored values with the sign bit flipped where maximised and NaN -> +inf; the violation with NaN -> +inf
    and everything <= 0 -> 0."""
    v = np.array(objectives, dtype=f32)
    N, M = v.shape
    if maximize is not None:
        flip = np.where(np.asarray(maximize).astype(bool), np.uint32(0x80000000), np.uint32(0)).astype(np.uint32)
        v = (v.view(np.uint32) ^ flip[None, :]).view(f32)
    v = np.where(np.isnan(v), f32(inf), v)
    w = np.zeros(N, f32) if violation is None else np.array(violation, dtype=f32)
    w = np.where(np.isnan(w), f32(inf), w)
    w = np.where(w <= 0, f32(0), w)
    return v, w


def dominance(objectives, maximize=None, violation=None, candidates=None):
    """(N,N) bool: dom[i,j] = i dominates j (Deb's constrained domination among the candidates)."""
    v, w = keys(objectives, maximize, violation)
    N, M = v.shape
    le, lt = np.ones((N, N), bool), np.zeros((N, N), bool)
    for m in range(M):
        a = v[:, m]
        le &= a[:, None] <= a[None, :]
        lt |= a[:, None] < a[None, :]
    dom = (w[:, None] < w[None, :]) | ((w[:, None] == w[None, :]) & le & lt)
    cand = np.ones(N, bool) if candidates is None else np.asarray(candidates).astype(bool)
    dom &= cand[:, None] & cand[None, :]
    dom[np.arange(N), np.arange(N)] = False
    return dom, cand


def _finish(dom, cand, rank, score, F):
    N = len(cand)
    by = np.where(cand, dom.sum(0), -1).astype(np.int32)
    of = np.where(cand, dom.sum(1), -1).astype(np.int32)
    made = int(rank.max()) + 1
    front_size = np.zeros(F, np.int32)
    front_size[:made] = np.bincount(rank[rank >= 0], minlength=made)[:made] if made else []
    sc = np.zeros(N, f32) if score is None else np.array(score, dtype=f32)
    sc = np.where(np.isnan(sc), f32(inf), sc)
    cls = np.where(rank >= 0, rank, np.where(cand, N, N + 1))
    order = np.lexsort((np.arange(N), -of.astype(np.int64), sc, cls)).astype(np.int64)  # (the last key is the first compared)
    return rank.astype(np.int32), by, of, front_size, np.int32(made), np.int32((cand & (rank < 0)).sum()), order


def _brute_one(objectives, maximize, violation, score, candidates, F):
    dom, cand = dominance(objectives, maximize, violation, candidates)
    open_ = cand.copy()
    rank = np.full(len(cand), -1, np.int64)
    made = 0
    while made < F and open_.any():
        n = (dom & open_[:, None]).sum(0)  # recounted from scratch
        members = open_ & (n == 0)
        rank[members] = made
        open_ &= ~members
        made += 1
    return _finish(dom, cand, rank, score, F)


def _chain_one(objectives, maximize, violation, score, candidates, F):
    dom, cand = dominance(objectives, maximize, violation, candidates)
    by = dom.sum(0)
    dominators = np.ascontiguousarray(dom.T)
    rank = np.full(len(cand), -1, np.int64)
    for j in np.argsort(by, kind="stable"):
        if cand[j]:
            rank[j] = rank[dominators[j]].max() + 1 if by[j] else 0
    rank[rank >= F] = -1
    return _finish(dom, cand, rank, score, F)


def _pareto(one, objectives, maximize, violation, score, candidates, max_fronts):
    objectives = np.asarray(objectives, dtype=f32)
    G, N, M = objectives.shape
    F = N if max_fronts is None else max_fronts
    per = [one(objectives[g], maximize, None if violation is None else violation[g], None if score is None else score[g],
               None if candidates is None else candidates[g], F) for g in range(G)]
    out = {k: np.stack([p[i] for p in per]) if G else None for i, k in enumerate(OUTPUTS)}
    out["front_size"] = out["front_size"].reshape(G, F)
    return out


def pareto_ref(objectives, maximize=None, violation=None, score=None, candidates=None, max_fronts=None):
    return _pareto(_brute_one, objectives, maximize, violation, score, candidates, max_fronts)


def pareto_ref_chain(objectives, maximize=None, violation=None, score=None, candidates=None, max_fronts=None):
    return _pareto(_chain_one, objectives, maximize, violation, score, candidates, max_fronts)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def ref(objectives, **kw):
    a, b = pareto_ref(objectives, **kw), pareto_ref_chain(objectives, **kw)
    for k in OUTPUTS:
        assert same_bits(a[k], b[k]), f"the two oracles differ in {k}"
    return a


# ------------------------------------------------------------------ data (shared with test_gpu_pareto.py)
def quarters(seed, G, N, M):
    """(G,N,M) fp32: independent normal objectives rounded to quarters - ties, and tens of fronts at M <= 4."""
    return (np.round(np.random.default_rng(seed).normal(0, 1, (G, N, M)) * 4) / 4).astype(f32)


def correlated(seed, G, N, M):
    """(G,N,M) fp32: one integer in [0, 12) per design plus an integer in [0, 3) per objective - many fronts even at M = 16, where
    independent objectives give one."""
    rng = np.random.default_rng(seed)
    return (rng.integers(0, 12, (G, N, 1)) + rng.integers(0, 3, (G, N, M))).astype(f32)


def table(rows):
    return np.array([rows], f32)


STAIRS = [(1, 4), (2, 3), (3, 2), (4, 1), (2, 4), (3, 3), (4, 2), (4, 4)]  # three steps of 4, 3 and 1 designs


# ------------------------------------------------------------------ hand cases
def test_a_staircase_of_two_objectives():
    r = ref(table(STAIRS))
    assert r["rank"].tolist() == [[0, 0, 0, 0, 1, 1, 1, 2]]
    assert r["front_size"].tolist() == [[4, 3, 1, 0, 0, 0, 0, 0]] and r["count"].tolist() == [3] and r["n_unranked"].tolist() == [0]
    assert r["n_dominators"].tolist() == [[0, 0, 0, 0, 2, 2, 2, 7]]
    assert r["n_dominated"].tolist() == [[2, 3, 3, 2, 1, 1, 1, 0]]
    assert r["order"].tolist() == [[1, 2, 0, 3, 4, 5, 6, 7]]  # inside a front: the design that dominates more comes first, then the index
    assert r["rank"].dtype == np.int32 and r["order"].dtype == np.int64 and r["front_size"].dtype == np.int32 and r["count"].dtype == np.int32


def test_duplicates_share_a_front():
    r = ref(table([(1, 1), (1, 1), (2, 2), (2, 2), (1, 1)]))
    assert r["rank"].tolist() == [[0, 0, 1, 1, 0]] and r["front_size"].tolist() == [[3, 2, 0, 0, 0]]
    assert r["n_dominators"].tolist() == [[0, 0, 3, 3, 0]] and r["n_dominated"].tolist() == [[2, 2, 0, 0, 2]]


def test_nan_is_the_worst_value_and_the_zeros_and_infinities():
    r = ref(table([(nan, 0), (5, 0), (inf, 0), (-nan, 0)]))  # a NaN of either sign is +inf: 0, 2 and 3 are equal vectors
    assert r["rank"].tolist() == [[1, 0, 1, 1]] and r["n_dominated"].tolist() == [[0, 3, 0, 0]]
    r = ref(table([(-0.0, 1), (0.0, 1), (0.0, 2)]))  # -0 equals +0
    assert r["rank"].tolist() == [[0, 0, 1]]
    r = ref(table([(-inf, 3), (0, 3), (inf, 3), (-inf, 2)]))
    assert r["rank"].tolist() == [[1, 2, 3, 0]]
    r = ref(table([(nan, nan), (nan, nan), (1, nan)]))  # a design of nothing but NaNs is dominated by anything with a number
    assert r["rank"].tolist() == [[1, 1, 0]]


def test_maximize():
    t = table(STAIRS)
    r = ref(t, maximize=[True, True])
    assert r["rank"].tolist() == [[2, 2, 2, 2, 1, 1, 1, 0]]  # the staircase upside down: (4,4) alone, then the middle step
    r = ref(t, maximize=[False, True])  # small first, large second: (1,4) beats everything, a chain of seven; (4,4) is behind (2,4) only
    assert r["rank"].tolist() == [[0, 2, 4, 6, 1, 3, 5, 2]]
    flipped = t * np.array([1, -1], f32)
    assert same_bits(ref(flipped)["rank"], r["rank"])
    r = ref(table([(nan,), (1,), (2,), (-0.0,), (0.0,)]), maximize=[True])  # NaN stays the worst when the sign is flipped
    assert r["rank"].tolist() == [[3, 1, 0, 2, 2]]
    assert same_bits(ref(t, maximize=[False, False])["rank"], ref(t)["rank"])


def test_violation_negative_zero_positive_and_nan():
    t = table([(5, 5), (1, 1), (2, 2), (0, 0), (0, 0), (9, 9)])
    r = ref(t, violation=np.array([[-3.0, 0.5, -0.0, nan, 0.5, 0.0]], f32))
    # feasible: 0, 2, 5 (w = 0: -3, -0 and 0 alike) ranked by their objectives; then w = 0.5: 4 dominates 1; then the NaN
    assert r["rank"].tolist() == [[1, 4, 0, 5, 3, 2]]
    assert r["n_dominators"].tolist() == [[1, 4, 0, 5, 3, 2]] and r["n_dominated"].tolist() == [[4, 1, 5, 0, 2, 3]]
    r = ref(t, violation=np.array([[inf, inf, nan, 1, 2, 1]], f32))  # NaN ties with +inf
    assert r["rank"].tolist() == [[5, 3, 4, 0, 2, 1]]  # w = 1: 3 before 5; w = 2: 4; w = +inf: 1, 2, 0 by their objectives


def test_candidates_with_an_empty_patch():
    t = np.concatenate([table(STAIRS), table(STAIRS)])
    cand = np.array([[0, 1, 1, 0, 1, 0, 1, 1], [0] * 8], bool)
    r = ref(t, candidates=cand)
    # left: (2,3), (3,2) | (2,4) behind (2,3), (4,2) behind (3,2) | (4,4)
    assert r["rank"].tolist() == [[-1, 0, 0, -1, 1, -1, 1, 2], [-1] * 8]
    assert r["n_dominators"].tolist() == [[-1, 0, 0, -1, 1, -1, 1, 4], [-1] * 8]
    assert r["n_dominated"].tolist() == [[-1, 2, 2, -1, 1, -1, 1, 0], [-1] * 8]
    assert r["count"].tolist() == [3, 0] and r["n_unranked"].tolist() == [0, 0] and r["front_size"].tolist() == [[2, 2, 1] + [0] * 5, [0] * 8]
    assert r["order"].tolist() == [[1, 2, 4, 6, 7, 0, 3, 5], list(range(8))]


def test_max_fronts_0_1_and_a_value_reached_mid_way():
    t = table(STAIRS)
    r = ref(t, max_fronts=0)
    assert (r["rank"] == -1).all() and r["count"].tolist() == [0] and r["n_unranked"].tolist() == [8] and r["front_size"].shape == (1, 0)
    assert r["n_dominators"].tolist() == [[0, 0, 0, 0, 2, 2, 2, 7]] and r["order"].tolist() == [[1, 2, 0, 3, 4, 5, 6, 7]]
    r = ref(t, max_fronts=1)
    assert r["rank"].tolist() == [[0, 0, 0, 0, -1, -1, -1, -1]] and r["front_size"].tolist() == [[4]] and r["n_unranked"].tolist() == [4]
    r = ref(t, max_fronts=2)
    assert r["rank"].tolist() == [[0, 0, 0, 0, 1, 1, 1, -1]] and r["front_size"].tolist() == [[4, 3]]
    assert r["count"].tolist() == [2] and r["n_unranked"].tolist() == [1]
    cand = np.array([[1, 1, 1, 1, 1, 1, 0, 1]], bool)
    r = ref(t, max_fronts=2, candidates=cand)  # the unranked candidate comes before the non-candidate
    assert r["order"].tolist() == [[1, 0, 2, 3, 4, 5, 7, 6]] and r["n_dominated"].tolist() == [[2, 3, 2, 1, 1, 1, -1, 0]]


def test_order_with_and_without_score():
    t = table(STAIRS)
    r = ref(t, score=np.array([[3, 1, 1, nan, 0.0, -0.0, -1, 7]], f32))
    # front 0: scores 1, 1 (1 and 2 dominate three designs each: the index decides), 3, NaN; front 1: -1, then 0.0 == -0.0 by index
    assert r["order"].tolist() == [[1, 2, 0, 3, 6, 4, 5, 7]]
    r = ref(t, score=np.array([[inf, nan, 2, 2, 0, 0, 0, 0]], f32))  # NaN ties with +inf; 2 dominates more than 3
    assert r["order"].tolist() == [[2, 3, 1, 0, 4, 5, 6, 7]]
    r = ref(t, score=np.array([[0, 5, 5, 0, 0, 0, 0, 0]], f32))
    assert r["order"].tolist() == [[0, 3, 1, 2, 4, 5, 6, 7]]
    for g in range(1):  # front r is a contiguous slice of order
        at = np.concatenate([[0], np.cumsum(r["front_size"][g])])
        assert all((r["rank"][g][r["order"][g][at[k]:at[k + 1]]] == k).all() for k in range(int(r["count"][g])))


# ------------------------------------------------------------------ the properties, apart from the oracle
def check_properties(r, objectives, maximize=None, violation=None, candidates=None, max_fronts=None):
    G, N = r["rank"].shape
    F = N if max_fronts is None else max_fronts
    for g in range(G):
        dom, cand = dominance(objectives[g], maximize, None if violation is None else violation[g], None if candidates is None else candidates[g])
        rank, by, of = r["rank"][g], r["n_dominators"][g], r["n_dominated"][g]
        assert not dom.diagonal().any() and not (dom & dom.T).any()
        ranked = rank >= 0
        both = dom & ranked[:, None] & ranked[None, :]
        assert (rank[None, :] > rank[:, None])[both].all()
        for j in np.flatnonzero(rank > 0):
            assert (dom[:, j] & (rank == rank[j] - 1)).any()
        if F >= 1:
            assert ((rank == 0) == (by == 0)).all()
        assert (rank[~cand] == -1).all() and (by[~cand] == -1).all() and (of[~cand] == -1).all()
        assert (by[cand] == dom.sum(0)[cand]).all() and (of[cand] == dom.sum(1)[cand]).all()
        c = int(r["count"][g])
        assert c <= F and rank.max() == c - 1 and (r["front_size"][g, :c] == np.bincount(rank[ranked], minlength=c)).all()
        assert (r["front_size"][g, :c] >= 1).all() and (r["front_size"][g, c:] == 0).all()
        assert int(r["n_unranked"][g]) == int((cand & ~ranked).sum())
        order = r["order"][g]
        assert sorted(order.tolist()) == list(range(N))
        cls = np.where(ranked, rank, np.where(cand, N, N + 1))[order]
        assert (np.diff(cls) >= 0).all()


@pytest.mark.parametrize("seed, N, M, F", [(0, 40, 2, None), (1, 97, 3, None), (2, 130, 4, None), (3, 64, 2, 3), (4, 33, 1, None), (5, 70, 16, None)])
def test_the_properties_on_integer_valued_tables(seed, N, M, F):
    rng = np.random.default_rng(seed + 100)
    t = correlated(seed, 3, N, M) if M == 16 else rng.integers(0, 6, (3, N, M)).astype(f32)
    cand = rng.random((3, N)) < 0.8
    vio = rng.integers(-2, 2, (3, N)).astype(f32)
    mx = [bool(b) for b in rng.integers(0, 2, M)]
    score = rng.integers(0, 3, (3, N)).astype(f32)
    r = ref(t, maximize=mx, violation=vio, candidates=cand, score=score, max_fronts=F)
    check_properties(r, t, mx, vio, cand, F)
    assert (r["count"] > 1).all() and (r["front_size"].max(1) > 1).all()
    assert all(same_bits(pareto_ref(t[1:2], maximize=mx, violation=vio[1:2], candidates=cand[1:2], score=score[1:2], max_fronts=F)[k], r[k][1:2])
               for k in OUTPUTS)  # a patch alone


# ------------------------------------------------------------------ the header, the library and the ctypes table
def header_code():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


def test_header_library_and_symbol_table_agree():
    code = header_code()
    protos = dict(re.findall(r"\bint\s+(diffab_[a-z0-9_]+)\s*\((.*?)\)\s*;", code, flags=re.S))
    assert "diffab_metrics_pareto" in protos and "diffab_metrics_pareto" in _hip.CLUSTER_SYMBOLS
    names = [p.strip().rsplit(" ", 1)[1].lstrip("*") for p in protos["diffab_metrics_pareto"].split(",")]
    assert names == [*INPUTS, "G", "N", "M", "F", *OUTPUTS, "workspace", "workspace_bytes", "stream"]
    res, args = _hip.CLUSTER_SYMBOLS["diffab_metrics_pareto"]
    assert res is ctypes.c_int and len(args) == len(names)
    for p, a in zip(protos["diffab_metrics_pareto"].split(","), args):  # pointers, int32_t and size_t only
        kind = p.strip().rsplit(" ", 1)[0]
        want = {"int32_t": ctypes.c_int32, "size_t": ctypes.c_size_t}.get(kind)
        assert (a is want) if want is not None else ("*" in kind and a is ctypes.c_void_p), p
    assert hasattr(ctypes.CDLL(_hip.LIB_PATH), "diffab_metrics_pareto")
    fn = _hip.load_library().diffab_metrics_pareto
    assert fn.restype is res and list(fn.argtypes) == args
    opening = open(HEADER).read().split("*/")[0]
    assert "a table of one patch's designs" in opening and "Why a header of its own" in opening
    assert int(re.search(r"#define\s+DIFFAB_METRICS_PARETO_MAX_OBJECTIVES\s+(\d+)", code).group(1)) == metrics.PARETO_MAX_OBJECTIVES == 16


SHAPES = [(1, 1), (1, 63), (3, 64), (2, 65), (5, 127), (3, 129), (256, 64), (7, 255), (7, 256), (7, 257), (16, 1024), (2, 1023), (2, 1025), (4, 4096),
          (1, 4033), (600, 4096)]
MACRO_C = r"""
#include <stdio.h>
#include "diffab_hip_cluster.h"
int main(void) {
%s
  printf("%%d %%d\n", DIFFAB_METRICS_PARETO_MAX_OBJECTIVES, DIFFAB_METRICS_MAX_GROUP);
  return 0;
}
"""


def test_workspace_macro_equals_the_python_mirror(tmp_path):
    """The header compiles as C on its own and its macro gives metrics.pareto_workspace_bytes."""
    cc = shutil.which("cc") or shutil.which("gcc") or next((p for p in ("/opt/rocm/llvm/bin/clang",) if os.path.exists(p)), None)
    assert cc, "no C compiler to read the header's macro with"
    src, exe = tmp_path / "macro.c", tmp_path / "macro"
    src.write_text(MACRO_C % "\n".join(f'  printf("%zu\\n", DIFFAB_METRICS_PARETO_WORKSPACE_BYTES({G}, {N}));' for G, N in SHAPES))
    subprocess.run([cc, "-I", os.path.join(REPO, "include"), str(src), "-o", str(exe)], check=True)
    got = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()
    assert [int(v) for v in got[:len(SHAPES)]] == [metrics.pareto_workspace_bytes(*s) for s in SHAPES]
    assert got[len(SHAPES):] == [str(metrics.PARETO_MAX_OBJECTIVES), str(metrics.MAX_GROUP)]
    assert metrics.pareto_workspace_bytes(600, 4096) > 1 << 30  # (size_t arithmetic: past 32 bits)
    assert metrics.pareto_workspace_bytes(1, 4096) == 4096 * 4096 // 8 + 16 * 4096 * 4 + 64 * 4096 * 4 + 1024
    assert metrics.pareto_workspace_bytes(3, 65) == 3 * (128 * 128 // 8 + 128 * 4 + 2 * 128 * 4) + 1024


def test_host_side_refusals_touch_no_gpu():
    """Every refusal is decided from the scalar arguments and whether a pointer is null: the device pointers are fake addresses that
    are never dereferenced, nothing is enqueued (no GPU is needed), and diffab_last_error names the problem."""
    l = _hip.load_library()
    p, null = ctypes.c_void_p(4096), ctypes.c_void_p(0)

    def err():
        return l.diffab_last_error().decode()

    def call(G=2, N=100, M=3, F=10, ws=p, ws_bytes=1 << 40, **ptrs):
        a = dict(dict.fromkeys((*INPUTS, *OUTPUTS), p), maximize=null, violation=null, score=null, candidates=null)
        a.update(ptrs)
        return l.diffab_metrics_pareto(*[a[k] for k in INPUTS], G, N, M, F, *[a[k] for k in OUTPUTS], ws, ws_bytes, null)

    for kw, word in ((dict(G=-1), "extent"), (dict(N=0, F=0), "extent"), (dict(N=-3, F=0), "extent"), (dict(N=4097), "at most 4096 designs"),
                     (dict(M=0), "M = 0 objectives outside [1, 16]"), (dict(M=17), "M = 17 objectives outside [1, 16]"), (dict(M=-1), "objectives outside"),
                     (dict(F=-1), "F = -1 fronts outside [0, N = 100]"), (dict(F=101), "F = 101 fronts outside"),
                     (dict(objectives=null), "null input"), (dict(rank=null), "null output"), (dict(count=null), "null output"),
                     (dict(front_size=null), "null output"), (dict(ws=null), "workspace"), (dict(ws=ctypes.c_void_p(4096 + 16)), "256-byte aligned"),
                     (dict(ws=ctypes.c_void_p(4096 + 128)), "256-byte aligned")):
        rc = call(**kw)
        assert rc == -1 and word in err() and err().startswith("metrics_pareto:"), (kw, rc, err())
    need = metrics.pareto_workspace_bytes(2, 100)
    assert call(ws_bytes=need // 2) == -4 and "needed" in err() and err().startswith("metrics_pareto:")  # DIFFAB_ERR_WORKSPACE
    assert need - 1024 <= int(re.search(r"(\d+) needed", err()).group(1)) <= need
    # the limits themselves pass every argument check (the call is stopped by the workspace size, still on the host); so do the
    # optional operands, the nullable outputs, and front_size left out with F = 0
    for kw in (dict(N=4096, F=4096), dict(N=1, F=1), dict(N=1, F=0), dict(F=0), dict(F=100), dict(M=1), dict(M=16),
               dict(maximize=p, violation=p, score=p, candidates=p), dict(n_dominators=null, n_dominated=null, n_unranked=null, order=null),
               dict(F=0, front_size=null)):
        assert call(ws_bytes=16, **kw) == -4 and "needed" in err(), kw
    # an empty problem returns 0 before any pointer is looked at
    assert l.diffab_metrics_pareto(*[null] * 5, 0, 8, 3, 2, *[null] * 7, null, 0, null) == 0


# ------------------------------------------------------------------ Python argument errors before any device work
@pytest.fixture
def no_library(monkeypatch):
    refuse_library(monkeypatch)


def test_good_arguments_reach_the_library(no_library):
    t = torch.zeros(2, 8, 3)
    flat = [torch.zeros(16), torch.zeros(16, dtype=torch.int32), torch.zeros(16, dtype=torch.float64)]
    for args, kw in (((t,), {}), ((t,), dict(group_size=8, maximize=True)), ((t,), dict(maximize=[True, False, True], max_fronts=0)),
                     ((t,), dict(violation=torch.zeros(2, 8), score=torch.zeros(2, 8, dtype=torch.float64), candidates=torch.ones(2, 8, dtype=torch.bool),
                                 max_fronts=8)),
                     ((flat,), dict(group_size=8)), ((tuple(flat),), dict(group_size=4, maximize=(False, True, False))),
                     (([torch.zeros(2, 8), torch.zeros(2, 8, dtype=torch.long)],), {}), (([torch.zeros(2, 8)] * 16,), dict(group_size=8)),
                     ((torch.zeros(1, 4096, 16),), {})):
        with pytest.raises(ReachedTheLibrary):
            metrics.pareto(*args, **kw)


@pytest.mark.parametrize("kw, match", [
    (dict(objectives=torch.zeros(2, 8)), "objectives must be a float32 tensor"),
    (dict(objectives=torch.zeros(2, 8, 3, dtype=torch.float64)), "objectives must be a float32 tensor"),
    (dict(objectives=torch.zeros(2, 8, 3, dtype=torch.long)), "objectives must be a float32 tensor"),
    (dict(objectives=[]), "objectives must be"), (dict(objectives=[[1.0, 2.0]]), "objectives must be"), (dict(objectives="x"), "objectives must be"),
    (dict(objectives=torch.zeros(2, 0, 3)), r"N = 0 designs per patch, outside \[1, 4096\]"),
    (dict(objectives=torch.zeros(1, 4097, 1)), "N = 4097 designs per patch"),
    (dict(objectives=torch.zeros(2, 8, 0)), r"M = 0 objectives, outside \[1, 16\]"),
    (dict(objectives=torch.zeros(2, 8, 17)), "M = 17 objectives"),
    (dict(objectives=[torch.zeros(16)] * 17, group_size=8), "M = 17 objectives"),
    (dict(objectives=torch.zeros(2, 8, 3), group_size=4), "group_size = 4 does not match"),
    (dict(objectives=[torch.zeros(16), torch.zeros(16)]), "group_size must be an int >= 1 for flat"),
    (dict(objectives=[torch.zeros(16)], group_size=0), "group_size must be an int >= 1"),
    (dict(objectives=[torch.zeros(16)], group_size=True), "group_size must be"),
    (dict(objectives=[torch.zeros(16)], group_size=5), "16 design rows are not a multiple of group_size = 5"),
    (dict(objectives=[torch.zeros(16), torch.zeros(15)], group_size=8), r"objectives\[1\] is \(15,\)"),
    (dict(objectives=[torch.zeros(16), torch.zeros(16, dtype=torch.bool)], group_size=8), r"objectives\[1\] must be a float or integer tensor"),
    (dict(objectives=[torch.zeros(2, 2, 4)], group_size=8), r"objectives\[0\] must be"),
    (dict(objectives=[torch.zeros(2, 8)], group_size=4), "group_size = 4 does not match"),
    (dict(maximize=[True, False]), "maximize must be a bool or a sequence of M = 3 bools"), (dict(maximize=1), "maximize must be"),
    (dict(maximize=[1, 0, 1]), "maximize must be"), (dict(maximize=torch.ones(3, dtype=torch.bool)), "maximize must be"),
    (dict(violation=torch.zeros(2, 8, dtype=torch.long)), "violation must be a float tensor"), (dict(violation=torch.zeros(8)), "violation must be"),
    (dict(violation=[0.0] * 8), "violation must be"), (dict(score=torch.zeros(2, 8, dtype=torch.long)), "score must be a float tensor"),
    (dict(score=torch.zeros(2, 7)), "score must be"), (dict(candidates=torch.ones(2, 8)), "candidates must be a bool tensor"),
    (dict(candidates=torch.ones(2, 7, dtype=torch.bool)), "candidates must be"), (dict(max_fronts=-1), "max_fronts must be an int in"),
    (dict(max_fronts=9), r"max_fronts must be an int in \[0, N = 8\]"), (dict(max_fronts=2.0), "max_fronts must be"),
    (dict(max_fronts=True), "max_fronts must be"),
])
def test_argument_errors(no_library, kw, match):
    args = dict(objectives=torch.zeros(2, 8, 3))
    args.update(kw)
    objectives = args.pop("objectives")
    with pytest.raises(ValueError, match=r"metrics\.pareto\(\): .*" + match):
        metrics.pareto(objectives, **args)


def test_signature_and_constants():
    sig = inspect.signature(metrics.pareto)
    assert list(sig.parameters) == ["objectives", "group_size", "maximize", "violation", "score", "candidates", "max_fronts"]
    assert all(sig.parameters[k].kind is inspect.Parameter.KEYWORD_ONLY and sig.parameters[k].default is None for k in list(sig.parameters)[1:])
    assert metrics.PARETO_MAX_OBJECTIVES == 16
    assert "``pareto``" in metrics.__doc__ and "pareto_kernels.hip" in metrics.__doc__
