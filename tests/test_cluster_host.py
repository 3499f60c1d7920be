"""Design clustering without a GPU: the numpy oracles of diffab_metrics_cluster, hand cases with the answer written out, the two
invariants of the rule, the header / library / ctypes table, the workspace macro, the host-side refusals and the Python argument errors.

The rule is DESIGN.md section 4.21 / the header comment of include/diffab_hip_cluster.h.  `cluster_ref` restates it by brute force: it
recounts n(i) from the full boolean matrix at every iteration.  `cluster_ref_incremental` subtracts the removed columns instead and
serves large N; `ref` runs both and asserts them equal, and every host case goes through it, so test_gpu_cluster.py may use the
incremental one above 1000 designs.  test_gpu_cluster.py imports the oracles and the data from here."""
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
OUTPUTS = ("label", "center_dist", "center", "size", "count", "n_unassigned")  # the order of the C prototype


# ------------------------------------------------------------------ the oracles
def adjacency(dist, cutoff):
    """(N,N) bool: adj(i,j) = i == j or dist[i,j] <= cutoff as one fp32 compare (a NaN on either side: False); the diagonal is not read."""
    d = np.array(dist, dtype=f32)
    np.fill_diagonal(d, 0)
    with np.errstate(invalid="ignore"):
        a = d <= f32(cutoff)
    np.fill_diagonal(a, True)
    return a


def centre_of(n, score, open_):
    """The open design with the largest count; ties to the lower score (fp32 values, NaN = +inf); then to the lower index."""
    idx = np.flatnonzero(open_)
    idx = idx[n[idx] == n[idx].max()]
    idx = idx[score[idx] == score[idx].min()]
    return int(idx[0])


def _cluster_one(dist, cutoff, candidates, score, M, incremental):
    dist = np.asarray(dist, dtype=f32)
    N = dist.shape[0]
    adj = adjacency(dist, cutoff)
    open_ = np.ones(N, bool) if candidates is None else np.asarray(candidates).astype(bool).copy()
    sc = np.zeros(N, f32) if score is None else np.asarray(score, dtype=f32).copy()
    sc[np.isnan(sc)] = np.inf
    label = np.full(N, -1, np.int32)
    cdist = np.full(N, np.nan, f32)
    center, size = np.full(M, -1, np.int64), np.zeros(M, np.int32)
    n = (adj & open_[None, :]).sum(1) if incremental else None
    made = 0
    while made < M and open_.any():
        if not incremental:
            n = (adj & open_[None, :]).sum(1)  # recounted from scratch
        c = centre_of(n, sc, open_)
        members = np.flatnonzero(adj[c] & open_)
        label[members] = made
        cdist[members] = dist[c, members]
        cdist[c] = 0
        center[made], size[made] = c, len(members)
        open_[members] = False
        if incremental:
            n = n - adj[:, members].sum(1)
        made += 1
    return label, cdist, center, size, np.int32(made), np.int32(open_.sum())


def _cluster(dist, cutoff, candidates, score, max_clusters, incremental):
    dist = np.asarray(dist, dtype=f32)
    G, N = dist.shape[:2]
    M = N if max_clusters is None else max_clusters
    cut = np.broadcast_to(np.asarray(cutoff, dtype=f32), (G,))
    per = [_cluster_one(dist[g], cut[g], None if candidates is None else candidates[g], None if score is None else score[g], M, incremental)
           for g in range(G)]
    out = {k: np.stack([p[i] for p in per]) for i, k in enumerate(OUTPUTS)}
    out["center"], out["size"] = out["center"].reshape(G, M), out["size"].reshape(G, M)
    return out


def cluster_ref(dist, cutoff, candidates=None, score=None, max_clusters=None):
    return _cluster(dist, cutoff, candidates, score, max_clusters, incremental=False)


def cluster_ref_incremental(dist, cutoff, candidates=None, score=None, max_clusters=None):
    return _cluster(dist, cutoff, candidates, score, max_clusters, incremental=True)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def ref(dist, cutoff, **kw):
    a, b = cluster_ref(dist, cutoff, **kw), cluster_ref_incremental(dist, cutoff, **kw)
    for k in OUTPUTS:
        assert same_bits(a[k], b[k]), f"the two oracles differ in {k}"
    return a


# ------------------------------------------------------------------ data (shared with test_gpu_cluster.py)
def line(x):
    """(1,N,N) fp32: |x_i - x_j| of points on a line."""
    x = np.asarray(x, dtype=f32)
    return np.abs(x[:, None] - x[None, :])[None]


def planted(seed, G, N, families, spread=1.0, apart=12.0, dim=3):
    """(G,N,N) fp32 Euclidean distances of N points around `families` centres, family sizes uneven, designs in random order."""
    rng = np.random.default_rng(seed)
    out = np.empty((G, N, N), f32)
    for g in range(G):
        centres = rng.normal(0, apart, (families, dim))
        p = rng.dirichlet(np.full(families, 2.0))
        which = rng.choice(families, N, p=p)
        x = (centres[which] + rng.normal(0, spread, (N, dim))).astype(f32)
        for i0 in range(0, N, 512):
            d = x[i0:i0 + 512, None, :] - x[None, :, :]
            out[g, i0:i0 + 512] = np.sqrt((d * d).sum(-1, dtype=f32))
    return out


def integer_valued(seed, G, N, high=6):
    """(G,N,N) fp32 of small integers, not symmetric: many count ties."""
    return np.random.default_rng(seed).integers(0, high, (G, N, N)).astype(f32)


BLOBS = [0.0, 10.0, 0.1, 20.0, 0.2, 10.1, 0.3, 0.4, 10.2]  # sizes 5, 3, 1; every pair of a blob within 0.5


# ------------------------------------------------------------------ hand cases
def test_three_blobs_of_5_3_1():
    d = line(BLOBS)
    r = ref(d, 0.5)
    assert r["label"].tolist() == [[0, 1, 0, 2, 0, 1, 0, 0, 1]]
    assert r["center"].tolist() == [[0, 1, 3] + [-1] * 6] and r["size"].tolist() == [[5, 3, 1] + [0] * 6]
    assert r["count"].tolist() == [3] and r["n_unassigned"].tolist() == [0]
    want = [d[0, 0, j] if lab == 0 else d[0, 1, j] if lab == 1 else 0 for j, lab in enumerate(r["label"][0])]
    assert same_bits(r["center_dist"], np.array([want], f32)) and r["center_dist"][0, [0, 1, 3]].tolist() == [0, 0, 0]
    assert r["label"].dtype == np.int32 and r["center"].dtype == np.int64 and r["size"].dtype == np.int32 and r["center_dist"].dtype == f32


def test_a_count_tie_goes_to_the_lower_score_then_to_the_lower_index():
    d = line([0.0, 0.1, 5.0, 5.1])
    r = ref(d, 0.5, score=np.array([[3.0, 2.0, 1.0, 0.5]], f32))
    assert r["center"].tolist() == [[3, 1, -1, -1]] and r["label"].tolist() == [[1, 1, 0, 0]] and r["size"].tolist() == [[2, 2, 0, 0]]
    r = ref(d, 0.5, score=np.array([[1.0, 1.0, 1.0, 1.0]], f32))
    assert r["center"].tolist() == [[0, 2, -1, -1]] and r["label"].tolist() == [[0, 0, 1, 1]]
    r = ref(d, 0.5, score=np.array([[np.nan, np.inf, -0.0, 0.0]], f32))  # NaN = +inf ties with +inf; -0 == +0
    assert r["center"].tolist() == [[2, 0, -1, -1]]
    r = ref(d, 0.5)
    assert r["center"].tolist() == [[0, 2, -1, -1]]


def test_the_row_of_i_is_read_not_the_column():
    d = np.array([[[0, 0.5, 0.5], [5, 0, 5], [5, 5, 0]]], f32)
    r = ref(d, 1.0)
    assert r["label"].tolist() == [[0, 0, 0]] and r["center"].tolist() == [[0, -1, -1]] and r["size"].tolist() == [[3, 0, 0]]
    assert r["center_dist"].tolist() == [[0, 0.5, 0.5]]
    t = ref(np.ascontiguousarray(d.transpose(0, 2, 1)), 1.0)  # read by columns, design 0 has no neighbour and 1 and 2 have one each
    assert t["center"].tolist() == [[1, 2, -1]] and t["label"].tolist() == [[0, 0, 1]] and t["size"].tolist() == [[2, 1, 0]]


def test_a_nan_distance_is_no_neighbour_and_the_diagonal_is_not_read():
    nan = np.nan
    d = np.array([[[0, nan, 0.1], [nan, 0, 0.1], [0.1, nan, 0]]], f32)
    r = ref(d, 1.0)
    assert r["label"].tolist() == [[0, 1, 0]] and r["center"].tolist() == [[0, 1, -1]] and r["size"].tolist() == [[2, 1, 0]]
    blobs = line(BLOBS)
    for diag in (nan, np.inf, 7.0):
        e = blobs.copy()
        e[0][np.diag_indices(9)] = diag
        a, b = ref(e, 0.5), ref(blobs, 0.5)
        assert all(same_bits(a[k], b[k]) for k in OUTPUTS)


def test_the_extreme_cutoffs():
    d = line(BLOBS)
    r = ref(d, np.inf)
    assert r["count"].tolist() == [1] and r["size"][0, 0] == 9 and r["center"][0, 0] == 0 and (r["label"] == 0).all()
    assert same_bits(r["center_dist"][0], d[0, 0])
    for cut in (-1.0, np.nan):
        r = ref(d, cut)
        assert r["count"].tolist() == [9] and r["center"].tolist() == [list(range(9))] and r["label"].tolist() == [list(range(9))]
        assert (r["size"] == 1).all() and (r["center_dist"] == 0).all()


def test_max_clusters_and_candidates():
    d = line(BLOBS)
    r = ref(d, 0.5, max_clusters=0)
    assert r["count"].tolist() == [0] and r["n_unassigned"].tolist() == [9] and (r["label"] == -1).all() and np.isnan(r["center_dist"]).all()
    assert r["center"].shape == (1, 0) and r["size"].shape == (1, 0)
    r = ref(d, 0.5, max_clusters=2)
    assert r["count"].tolist() == [2] and r["n_unassigned"].tolist() == [1] and r["label"].tolist() == [[0, 1, 0, -1, 0, 1, 0, 0, 1]]
    assert np.isnan(r["center_dist"][0, 3]) and r["center"].tolist() == [[0, 1]] and r["size"].tolist() == [[5, 3]]
    r = ref(d, 0.5, candidates=np.zeros((1, 9), bool))
    assert r["count"].tolist() == [0] and r["n_unassigned"].tolist() == [0] and (r["label"] == -1).all() and (r["center"] == -1).all()
    cand = np.array([[0, 1, 1, 1, 0, 1, 0, 0, 1]], bool)  # the first blob keeps one of its five: the second is now the largest
    r = ref(d, 0.5, candidates=cand, max_clusters=2)
    assert r["label"].tolist() == [[-1, 0, 1, -1, -1, 0, -1, -1, 0]] and r["center"].tolist() == [[1, 2]] and r["size"].tolist() == [[3, 1]]
    assert r["n_unassigned"].tolist() == [1]  # design 3 only: the non-candidates are not counted


@pytest.mark.parametrize("seed, N, cutoff, M", [(0, 40, 1.0, None), (1, 97, 2.0, None), (2, 130, 0.0, None), (3, 64, 1.0, 5), (4, 33, 3.0, None)])
def test_the_two_invariants_on_integer_valued_matrices(seed, N, cutoff, M):
    d = integer_valued(seed, 3, N)
    rng = np.random.default_rng(seed + 100)
    cand = rng.random((3, N)) < 0.8
    score = rng.integers(0, 3, (3, N)).astype(f32)
    r = ref(d, cutoff, candidates=cand, score=score, max_clusters=M)
    check_invariants(r, d, np.full(3, cutoff, f32), cand)
    assert (r["count"] > 1).all() and (r["size"][:, 0] > 1).all()


def check_invariants(r, dist, cutoff, candidates=None):
    """Independent of the oracle: sizes never grow, no later centre within the cutoff of an earlier centre's row, and the book-keeping."""
    G, N = r["label"].shape
    for g in range(G):
        c = int(r["count"][g])
        size, center, label = r["size"][g], r["center"][g], r["label"][g]
        assert (np.diff(size[:c]) <= 0).all() and (size[:c] >= 1).all() and (size[c:] == 0).all() and (center[c:] == -1).all()
        adj = adjacency(dist[g], cutoff[g])
        for a in range(c):
            assert not adj[center[a], center[a + 1:c]].any()
            assert label[center[a]] == a and (label == a).sum() == size[a] and adj[center[a], label == a].all()
        cand = np.ones(N, bool) if candidates is None else candidates[g]
        assert (label[~cand] == -1).all() and (label >= -1).all() and (label < c).all()
        assert int(r["n_unassigned"][g]) == int(((label == -1) & cand).sum())
        assert (np.isnan(r["center_dist"][g]) == (label == -1)).all()


# ------------------------------------------------------------------ the header, the library and the ctypes table
def header_code():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


def test_header_library_and_symbol_table_agree():
    """Every entry the header declares is in _hip.CLUSTER_SYMBOLS with the same arity and kinds, is exported, and is typed by
    load_library(); nothing else is in the table.  How many entries there are is not asserted: the next set-level entry joins them."""
    code = header_code()
    protos = dict(re.findall(r"\bint\s+(diffab_[a-z0-9_]+)\s*\((.*?)\)\s*;", code, flags=re.S))
    declared = sorted(set(re.findall(r"\b(diffab_[a-z0-9_]+)\s*\(", code)))
    assert declared == sorted(protos) and "diffab_metrics_cluster" in declared
    assert sorted(_hip.CLUSTER_SYMBOLS) == declared, "CLUSTER_SYMBOLS and include/diffab_hip_cluster.h drifted apart"
    assert not set(_hip.CLUSTER_SYMBOLS) & (set(_hip.SYMBOLS) | set(_hip.ANALYSIS_SYMBOLS) | set(_hip.HBOND_SYMBOLS))
    raw = ctypes.CDLL(_hip.LIB_PATH)
    typed = _hip.load_library()
    for name, proto in protos.items():
        assert hasattr(raw, name), f"{name} is declared in include/diffab_hip_cluster.h but not exported by libdiffab_hip.so"
        res, args = _hip.CLUSTER_SYMBOLS[name]
        fn = getattr(typed, name)
        assert fn.restype is res and list(fn.argtypes) == args  # load_library() types the fourth table onto the same CDLL object
        params = [p.strip() for p in proto.split(",")]
        assert res is ctypes.c_int and len(args) == len(params), name
        for p, a in zip(params, args):
            kind = p.rsplit(" ", 1)[0]
            want = {"int32_t": ctypes.c_int32, "size_t": ctypes.c_size_t}.get(kind)
            if want is None:
                assert "*" in kind and a is ctypes.c_void_p, (name, p)
            else:
                assert a is want, (name, p)
    names = [p.strip().rsplit(" ", 1)[1].lstrip("*") for p in protos["diffab_metrics_cluster"].split(",")]
    assert names == ["dist", "cutoff", "score", "candidates", "G", "N", "M", *OUTPUTS, "workspace", "workspace_bytes", "stream"]
    text = open(HEADER).read()
    assert '#include "diffab_hip.h"' in text and "Why a header of its own" in text.split("*/")[0]
    assert int(re.search(r"#define\s+DIFFAB_METRICS_CLUSTER_LDS_MAX_N\s+(\d+)", code).group(1)) == metrics.CLUSTER_LDS_MAX_N
    assert metrics.CLUSTER_LDS_MAX_N % 64 == 0 and 64 <= metrics.CLUSTER_LDS_MAX_N <= 1024


SHAPES = [(1, 1), (1, 63), (3, 64), (2, 65), (5, 127), (3, 129), (256, 64), (7, 255), (7, 256), (7, 257), (16, 1024), (2, 1023), (2, 1025), (4, 4096),
          (1, 4033), (600, 4096)]
MACRO_C = r"""
#include <stdio.h>
#include "diffab_hip_cluster.h"
int main(void) {
%s
  printf("%%d %%d %%d\n", DIFFAB_ERR_ARG, DIFFAB_METRICS_CLUSTER_LDS_MAX_N, DIFFAB_METRICS_MAX_GROUP);
  return 0;
}
"""


def test_workspace_macro_equals_the_python_mirror(tmp_path):
    """The header compiles as C on its own (it brings diffab_hip.h along) and its macro gives metrics.cluster_workspace_bytes."""
    cc = shutil.which("cc") or shutil.which("gcc") or next((p for p in ("/opt/rocm/llvm/bin/clang",) if os.path.exists(p)), None)
    assert cc, "no C compiler to read the header's macro with"
    src, exe = tmp_path / "macro.c", tmp_path / "macro"
    src.write_text(MACRO_C % "\n".join(f'  printf("%zu\\n", DIFFAB_METRICS_CLUSTER_WORKSPACE_BYTES({G}, {N}));' for G, N in SHAPES))
    subprocess.run([cc, "-I", os.path.join(REPO, "include"), str(src), "-o", str(exe)], check=True)
    got = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()
    assert [int(v) for v in got[:len(SHAPES)]] == [metrics.cluster_workspace_bytes(*s) for s in SHAPES]
    assert got[len(SHAPES):] == ["-1", str(metrics.CLUSTER_LDS_MAX_N), str(metrics.MAX_GROUP)]
    assert metrics.cluster_workspace_bytes(600, 4096) > 1 << 30  # (size_t arithmetic: past 32 bits)
    assert metrics.cluster_workspace_bytes(1, 4096) == 4096 * 4096 // 8 + 16 * 4096 * 4 + 1024


def test_host_side_refusals_touch_no_gpu():
    """Every refusal is decided from the scalar arguments and whether a pointer is null: the device pointers are fake addresses that
    are never dereferenced, nothing is enqueued (no GPU is needed), and diffab_last_error names the problem."""
    l = _hip.load_library()
    p, null = ctypes.c_void_p(4096), ctypes.c_void_p(0)

    def err():
        return l.diffab_last_error().decode()

    def call(G=2, N=100, M=10, ws=p, ws_bytes=1 << 40, **ptrs):
        a = dict(dict.fromkeys(("dist", "cutoff", "score", "candidates", *OUTPUTS), p), score=null, candidates=null)
        a.update(ptrs)
        return l.diffab_metrics_cluster(a["dist"], a["cutoff"], a["score"], a["candidates"], G, N, M, *[a[k] for k in OUTPUTS], ws, ws_bytes, null)

    for kw, word in ((dict(G=-1), "extent"), (dict(N=0), "extent"), (dict(N=-3), "extent"), (dict(N=4097, M=1), "at most 4096 designs"),
                     (dict(M=-1), "M = -1 clusters outside [0, N = 100]"), (dict(M=101), "M = 101 clusters outside"),
                     (dict(dist=null), "null input"), (dict(cutoff=null), "null input"), (dict(label=null), "null output"),
                     (dict(count=null), "null output"), (dict(center=null), "null output"), (dict(size=null), "null output"),
                     (dict(ws=null), "workspace"), (dict(ws=ctypes.c_void_p(4096 + 16)), "256-byte aligned"),
                     (dict(ws=ctypes.c_void_p(4096 + 128)), "256-byte aligned")):
        rc = call(**kw)
        assert rc == -1 and word in err() and err().startswith("metrics_cluster:"), (kw, rc, err())
    need = metrics.cluster_workspace_bytes(2, 100)
    assert call(ws_bytes=need // 2) == -4 and "needed" in err() and err().startswith("metrics_cluster:")  # DIFFAB_ERR_WORKSPACE
    assert need - 1024 <= int(re.search(r"(\d+) needed", err()).group(1)) <= need
    # the limits themselves pass every argument check (the call is stopped by the workspace size, still on the host); so do the
    # optional operands, the nullable outputs, and center and size left out with M = 0
    for kw in (dict(N=4096, M=4096), dict(N=1, M=1), dict(N=1, M=0), dict(M=0), dict(M=100), dict(score=p, candidates=p),
               dict(center_dist=null, n_unassigned=null), dict(M=0, center=null, size=null)):
        assert call(ws_bytes=16, **kw) == -4 and "needed" in err(), kw
    # an empty problem returns 0 before any pointer is looked at
    assert l.diffab_metrics_cluster(null, null, null, null, 0, 8, 3, *[null] * 6, null, 0, null) == 0


# ------------------------------------------------------------------ Python argument errors before any device work
@pytest.fixture
def no_library(monkeypatch):
    refuse_library(monkeypatch)


def test_good_arguments_reach_the_library(no_library):
    d = torch.zeros(2, 8, 8)
    for kw in (dict(cutoff=1.0), dict(cutoff=2), dict(cutoff=torch.ones(2)), dict(cutoff=torch.ones(2, dtype=torch.float64)),
               dict(cutoff=1.0, candidates=torch.ones(2, 8, dtype=torch.bool), score=torch.zeros(2, 8), max_clusters=0),
               dict(cutoff=float("inf"), max_clusters=8), dict(cutoff=float("nan"), score=torch.zeros(2, 8, dtype=torch.float64))):
        with pytest.raises(ReachedTheLibrary):
            metrics.cluster(d, **kw)
    with pytest.raises(ReachedTheLibrary):
        metrics.cluster(torch.zeros(1, 4096, 4096), 1.0)


@pytest.mark.parametrize("kw, match", [
    (dict(dist=torch.zeros(2, 8, 7)), "dist must be a float32 tensor"), (dict(dist=torch.zeros(8, 8)), "dist must be a float32 tensor"),
    (dict(dist=torch.zeros(2, 8, 8, dtype=torch.float64)), "dist must be a float32 tensor"), (dict(dist=[[[0.0]]]), "dist must be a float32 tensor"),
    (dict(dist=torch.zeros(2, 0, 0)), r"N = 0 designs per patch, outside \[1, 4096\]"),
    (dict(dist=torch.zeros(1, 4097, 4097)), "N = 4097 designs per patch"),
    (dict(cutoff="1"), "cutoff must be a number or a float tensor"), (dict(cutoff=True), "cutoff must be a number"),
    (dict(cutoff=None), "cutoff must be a number"), (dict(cutoff=torch.ones(3)), r"cutoff must be a number or a float tensor \(2,\)"),
    (dict(cutoff=torch.ones(2, dtype=torch.long)), "cutoff must be"), (dict(cutoff=torch.ones(2, 1)), "cutoff must be"),
    (dict(candidates=torch.ones(2, 8)), "candidates must be a bool tensor"), (dict(candidates=torch.ones(2, 7, dtype=torch.bool)), "candidates must be"),
    (dict(candidates=[True] * 8), "candidates must be"), (dict(score=torch.zeros(2, 8, dtype=torch.long)), "score must be a float tensor"),
    (dict(score=torch.zeros(8)), "score must be"), (dict(max_clusters=-1), "max_clusters must be an int in"),
    (dict(max_clusters=9), r"max_clusters must be an int in \[0, N = 8\]"), (dict(max_clusters=2.0), "max_clusters must be"),
    (dict(max_clusters=True), "max_clusters must be"),
])
def test_argument_errors(no_library, kw, match):
    args = dict(dist=torch.zeros(2, 8, 8), cutoff=1.0)
    args.update(kw)
    dist, cutoff = args.pop("dist"), args.pop("cutoff")
    with pytest.raises(ValueError, match=r"metrics\.cluster\(\): .*" + match):
        metrics.cluster(dist, cutoff, **args)


def test_cluster_weights(no_library):
    label = torch.tensor([[0, 1, 0, -1], [2, -1, 0, 1]], dtype=torch.int32)
    clusters = {"label": label}
    assert metrics.cluster_weights(clusters).tolist() == [[1, 0, 1, 0], [0, 0, 1, 0]]
    assert metrics.cluster_weights(clusters, 1).tolist() == [[0, 1, 0, 0], [0, 0, 0, 1]]
    assert metrics.cluster_weights(clusters, 5).tolist() == [[0] * 4] * 2
    w = metrics.cluster_weights(clusters, torch.tensor([1, 2]))
    assert w.tolist() == [[0, 1, 0, 0], [1, 0, 0, 0]] and w.dtype == torch.float32 and tuple(w.shape) == (2, 4)
    for bad, match in ((dict(clusters=label), "clusters must be the dict"), (dict(clusters={}), "clusters must be the dict"),
                       (dict(clusters={"label": label.float()}), "integer label"), (dict(clusters={"label": label[0]}), "integer label"),
                       (dict(cluster=-1), "cluster must be an int >= 0"), (dict(cluster=0.0), "cluster must be"), (dict(cluster=True), "cluster must be"),
                       (dict(cluster=torch.tensor([0, 1, 2])), "cluster must be"), (dict(cluster=torch.tensor([0.0, 1.0])), "cluster must be"),
                       (dict(cluster=torch.tensor([0, -1])), "negative index")):
        args = dict(clusters=clusters, cluster=0)
        args.update(bad)
        with pytest.raises(ValueError, match=r"metrics\.cluster_weights\(\): .*" + match):
            metrics.cluster_weights(args["clusters"], args["cluster"])


def test_signatures_and_constants():
    sig = inspect.signature(metrics.cluster)
    assert list(sig.parameters) == ["dist", "cutoff", "candidates", "score", "max_clusters"]
    assert all(sig.parameters[k].kind is inspect.Parameter.KEYWORD_ONLY and sig.parameters[k].default is None for k in list(sig.parameters)[2:])
    sig = inspect.signature(metrics.cluster_weights)
    assert list(sig.parameters) == ["clusters", "cluster"] and sig.parameters["cluster"].default == 0
    assert "``cluster``" in metrics.__doc__ and "cluster_kernels.hip" in metrics.__doc__
