"""The clustering entry on the MI355X: diffab_metrics_cluster through the C ABI and through diffab_pytorch.metrics.cluster (DESIGN.md
section 4.21).

The oracle is test_cluster_host.py's numpy restatement of the rule, run on the SAME fp32 matrix the kernels read.  Every output must
EQUAL it - labels, centres, sizes, counts, and the bits of center_dist with its NaN positions: the rule is compares, popcounts and
integer adds.  No case is left out and there is no tolerance.  Every case asserts that it is not vacuous - more than one cluster, and one
larger than a single design - unless it is a named extreme.  The brute-force oracle serves up to 1000 designs, the incremental one (which
test_cluster_host.py holds equal to it) above.

The contracts of the general C ABI that the pinned tables of the older test files cannot take for a new entry - guard bands, operand
alignment, workspace contents, NULL outputs, G = 0 - are held here, on a harness of this file's own: EVERY oracle case below runs with
each operand between guard bands."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from diffab_pytorch import _hip, metrics
from sampler_support import hip  # noqa: F401
from test_cluster_host import (BLOBS, OUTPUTS, check_invariants, cluster_ref, cluster_ref_incremental, f32, integer_valued, line, planted,
                               same_bits)

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("hip")]

GUARD = 256  # bytes on either side of every operand
FILL = 0xA5
LDS_MAX = metrics.CLUSTER_LDS_MAX_N
INPUTS = (("dist", f32), ("cutoff", f32), ("score", f32), ("candidates", np.uint8))
OUT_DTYPE = {"label": np.int32, "center_dist": f32, "center": np.int64, "size": np.int32, "count": np.int32, "n_unassigned": np.int32}


def out_shape(name, G, N, M):
    return {"label": (G, N), "center_dist": (G, N), "center": (G, M), "size": (G, M), "count": (G,), "n_unassigned": (G,)}[name]


# ------------------------------------------------------------------ the C ABI, operand by operand
class Operand:
    """`nbytes` of device memory at `offset` bytes behind a 256-byte boundary, between two guard bands."""

    def __init__(self, nbytes, offset=0, data=None, fill=FILL):
        self.nbytes, self.start, self.fill = nbytes, GUARD + offset, fill
        self.buf = torch.full((GUARD + offset + nbytes + GUARD,), fill, dtype=torch.uint8, device="cuda")
        assert self.buf.data_ptr() % 256 == 0
        if data is not None:
            self.buf[self.start:self.start + nbytes] = torch.from_numpy(np.ascontiguousarray(data).reshape(-1).view(np.uint8)).cuda()

    @property
    def ptr(self):
        return ctypes.c_void_p(self.buf.data_ptr() + self.start)

    def guards_intact(self):
        lo, hi = self.buf[:self.start].cpu().numpy(), self.buf[self.start + self.nbytes:].cpu().numpy()
        return bool((lo == self.fill).all() and (hi == self.fill).all())

    def read(self, dtype, shape):
        return self.buf[self.start:self.start + self.nbytes].cpu().numpy().view(dtype).reshape(shape).copy()


def call_abi(case, misaligned=False, skip=(), workspace_fill=0x00):
    """diffab_metrics_cluster on the numpy inputs of `case`.  Every data operand sits between guard bands; with `misaligned`, one element
    (4 bytes floats and int32, 8 bytes the int64 centres, 1 byte the mask: the natural alignment) behind a 256-byte boundary.  Outputs
    named in `skip` are passed as NULL.  The workspace is exactly the documented size, filled with `workspace_fill`, between guard bands
    of its own.  Returns the outputs as numpy arrays."""
    lib = _hip.lib()
    G, N = case["dist"].shape[:2]
    M = case["M"]
    ops = []
    for name, dtype in INPUTS:
        v = case.get(name)
        if v is None:
            ops.append(None)
            continue
        v = np.ascontiguousarray(np.asarray(v).astype(dtype))
        ops.append(Operand(v.nbytes, np.dtype(dtype).itemsize if misaligned else 0, v))
    outs = {}
    for name in OUTPUTS:
        if name not in skip:
            item = np.dtype(OUT_DTYPE[name]).itemsize
            outs[name] = Operand(int(np.prod(out_shape(name, G, N, M))) * item, item if misaligned else 0)
    nbytes = metrics.cluster_workspace_bytes(G, N)
    ws = Operand(nbytes, 0, fill=workspace_fill)
    null = ctypes.c_void_p(0)
    rc = lib.diffab_metrics_cluster(*[null if o is None else o.ptr for o in ops], G, N, M, *[outs[n].ptr if n in outs else null for n in OUTPUTS],
                                    ws.ptr, nbytes, _hip.stream_ptr())
    assert rc == 0, lib.diffab_last_error().decode()
    torch.cuda.synchronize()
    for name, o in list(outs.items()) + [("workspace", ws)] + [(n, o) for (n, _), o in zip(INPUTS, ops) if o is not None]:
        assert o.guards_intact(), f"bytes around {name} were written"
    return {name: o.read(OUT_DTYPE[name], out_shape(name, G, N, M)) for name, o in outs.items()}


def check(out, want, what, names=OUTPUTS):
    for k in names:
        if k in out and not same_bits(out[k], want[k]):
            assert out[k].shape == want[k].shape and out[k].dtype == want[k].dtype, (what, k, out[k].shape, want[k].shape)
            a, b = out[k].reshape(-1), want[k].reshape(-1)
            bad = np.flatnonzero((a.view(np.uint8).reshape(a.size, -1) != b.view(np.uint8).reshape(b.size, -1)).any(1))
            raise AssertionError(f"{what}: {k} differs at {len(bad)} of {a.size} places, first {bad[:4].tolist()}: got {a[bad[:4]]!r}, oracle {b[bad[:4]]!r}")


# ------------------------------------------------------------------ cases
def case_of(dist, cutoff, candidates=None, score=None, M=None, extreme=None):
    G, N = dist.shape[:2]
    return {"dist": np.ascontiguousarray(dist, dtype=f32), "cutoff": np.broadcast_to(np.asarray(cutoff, f32), (G,)).copy(), "candidates": candidates,
            "score": score, "M": N if M is None else M, "extreme": extreme}


@functools.lru_cache(maxsize=None)
def straddle_data():
    return planted(11, 2, LDS_MAX + 1, 24)


def build(name):
    rng = np.random.default_rng(sum(map(ord, name)))
    if name == "N4096 planted":
        return case_of(planted(5, 1, 4096, 24), 3.5)
    if name.startswith("N"):  # "N63": planted families at a ballot / word boundary
        N = int(name[1:])
        if N <= 2:
            return case_of(line(BLOBS[:N]), 0.5, extreme="fewer than three designs")
        return case_of(planted(N, 1, N, 5), 3.0)
    if name.startswith("G3 N"):  # three patches, a cutoff each
        N = int(name[4:])
        return case_of(planted(N, 3, N, 6), [2.0, 3.0, 4.5])
    if name.startswith("straddle"):  # the same planted data cut to size, on both sides of the form change
        N = LDS_MAX + int(name.split()[1])
        return case_of(straddle_data()[:, :N, :N], [3.0, 3.5])
    if name.startswith("singletons"):  # a cutoff below every distance: the longest loop of either form
        N = LDS_MAX + int(name.split()[1])
        return case_of(straddle_data()[:1, :N, :N], -1.0, extreme="all singletons")
    if name == "one cluster":
        return case_of(planted(3, 2, 200, 4), np.inf, extreme="one cluster")
    if name == "nan cutoff":
        return case_of(planted(3, 1, 70, 4), np.nan, extreme="all singletons")
    if name == "candidates":  # random candidates; patch 1 has none
        cand = rng.random((3, 150)) < 0.6
        cand[1] = False
        return case_of(planted(7, 3, 150, 5), 3.0, candidates=cand)
    if name == "scores":  # ties among the scores - both zeros, both infinities, NaNs - and integer distances for the count ties they break
        score = rng.choice(np.array([-np.inf, -1.5, -0.0, 0.0, 1e-30, 2.0, np.inf, np.nan], f32), (2, 140))
        return case_of(integer_valued(8, 2, 140), 0.0, score=score, candidates=rng.random((2, 140)) < 0.9)
    if name == "integer distances":
        return case_of(integer_valued(9, 2, 200), 1.0)
    if name == "asymmetric":
        d = planted(10, 2, 100, 5)
        d = d + np.triu(np.full((100, 100), 2.0, f32), 1)[None]  # the upper triangle is farther than the lower
        return case_of(d, 3.0)
    if name == "nan entries":
        d = planted(12, 2, 131, 5)
        d[rng.random(d.shape) < 0.3] = np.nan
        d[:, np.arange(131), np.arange(131)] = np.nan  # the diagonal too: it does not enter
        return case_of(d, 3.0)
    if name == "max_clusters with candidates and scores past 1024":
        N = LDS_MAX + 70
        return case_of(planted(14, 1, N, 12), 3.0, M=7, candidates=rng.random((1, N)) < 0.7, score=rng.integers(0, 2, (1, N)).astype(f32))
    if name.startswith("max_clusters"):  # 0, 1, and a value hit mid-way (the planted patches have 5 families and more clusters)
        M = int(name.split()[1])
        return case_of(planted(13, 2, 90, 5), 3.0, M=M, extreme=None if M > 1 else f"max_clusters = {M}")
    raise KeyError(name)


CASES = (["N1", "N2", "N63", "N64", "N65", "G3 N127", "G3 N129", "straddle -1", "straddle 0", "straddle +1", "N4096 planted", "singletons 0",
          "singletons +1", "one cluster", "nan cutoff", "candidates", "scores", "integer distances", "asymmetric", "nan entries", "max_clusters 0",
          "max_clusters 1", "max_clusters 3", "max_clusters with candidates and scores past 1024"])


@functools.lru_cache(maxsize=None)
def get(name):
    """(case, oracle): built and solved once, shared by the tests below and left unchanged."""
    c = build(name)
    oracle = cluster_ref_incremental if c["dist"].shape[1] > 1000 else cluster_ref
    want = oracle(c["dist"], c["cutoff"], candidates=c["candidates"], score=c["score"], max_clusters=c["M"])
    if c["extreme"] is None:
        busy = [g for g in range(len(want["count"])) if c["candidates"] is None or c["candidates"][g].any()]
        assert all(want["count"][g] > 1 and want["size"][g, 0] > 1 for g in busy), f"{name} is vacuous: {want['count']}, {want['size'][:, :3]}"
    return c, want


@pytest.mark.parametrize("name", CASES)
def test_every_output_equals_the_oracle(name):
    c, want = get(name)
    out = call_abi(c)
    check(out, want, name)
    check_invariants(out, c["dist"], c["cutoff"], c["candidates"])


def test_the_cases_reach_what_they_are_named_for():
    assert get("singletons 0")[1]["count"].tolist() == [LDS_MAX] and get("singletons +1")[1]["count"].tolist() == [LDS_MAX + 1]
    assert get("one cluster")[1]["count"].tolist() == [1, 1] and get("nan cutoff")[1]["count"].tolist() == [70]
    assert get("candidates")[1]["count"][1] == 0 and get("candidates")[1]["n_unassigned"].tolist() == [0, 0, 0]
    assert get("max_clusters 0")[1]["n_unassigned"].tolist() == [90, 90] and (get("max_clusters 3")[1]["n_unassigned"] > 0).all()
    assert (get("max_clusters with candidates and scores past 1024")[1]["n_unassigned"] > 0).all()
    assert 10 < get("N4096 planted")[1]["count"][0] < 100  # tens of iterations
    c, want = get("scores")  # the score decides: without it another centre comes first
    plain = cluster_ref(c["dist"], c["cutoff"], candidates=c["candidates"])
    assert not same_bits(plain["center"], want["center"])
    c, want = get("asymmetric")  # the row decides: the transposed matrix clusters differently
    assert not same_bits(cluster_ref(np.ascontiguousarray(c["dist"].transpose(0, 2, 1)), c["cutoff"])["label"], want["label"])
    for a, b in (("straddle -1", "straddle 0"), ("straddle 0", "straddle +1")):  # the cut changes the data, not only the form
        assert get(a)[1]["count"].tolist() != [0, 0] and get(b)[1]["count"].tolist() != [0, 0]


@pytest.mark.parametrize("name", ["G3 N129", "straddle 0", "straddle +1", "candidates"])
def test_a_patch_alone_gives_what_it_gives_in_its_batch(name):
    c, want = get(name)
    g = c["dist"].shape[0] - 1
    alone = dict(c, dist=c["dist"][g:g + 1], cutoff=c["cutoff"][g:g + 1], candidates=None if c["candidates"] is None else c["candidates"][g:g + 1],
                 score=None if c["score"] is None else c["score"][g:g + 1])
    check(call_abi(alone), {k: v[g:g + 1] for k, v in want.items()}, name + ", last patch alone")


@pytest.mark.parametrize("name", ["G3 N129", "straddle 0", "straddle +1", "max_clusters with candidates and scores past 1024"])
def test_what_the_workspace_held_is_ignored(name):
    c, want = get(name)
    for fill in (0x00, 0xFF):
        check(call_abi(c, workspace_fill=fill), want, f"{name}, workspace full of {fill:#x}")


@pytest.mark.parametrize("name", ["N65", "G3 N127", "scores", "candidates", "straddle +1"])
def test_operands_at_their_natural_alignment(name):
    c, want = get(name)
    check(call_abi(c, misaligned=True), want, name + ", misaligned")


def test_null_outputs_are_skipped():
    c, want = get("candidates")
    for skip in (("center_dist",), ("n_unassigned",), ("center_dist", "n_unassigned")):
        out = call_abi(c, skip=skip)
        assert not set(skip) & set(out)
        check(out, want, f"candidates without {skip}")
    c, want = get("max_clusters 0")  # with M = 0 center and size may be NULL too
    check(call_abi(c, skip=("center", "size", "center_dist")), want, "max_clusters 0 without center and size")


def test_an_empty_problem_returns_before_any_pointer_is_read(hip):
    null = ctypes.c_void_p(0)
    assert hip.diffab_metrics_cluster(null, null, null, null, 0, 8, 3, *[null] * 6, null, 0, _hip.stream_ptr()) == 0
    out = metrics.cluster(torch.zeros(0, 8, 8, device="cuda"), 1.0, max_clusters=3)
    assert tuple(out["label"].shape) == (0, 8) and tuple(out["center"].shape) == (0, 3) and tuple(out["representative"].shape) == (0, 8)


# ------------------------------------------------------------------ through the package
def t(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.mark.parametrize("name", ["G3 N129", "candidates", "scores", "max_clusters 3", "straddle +1"])
def test_the_python_entry(name):
    c, want = get(name)
    G, N = c["dist"].shape[:2]
    cand = None if c["candidates"] is None else t(c["candidates"].astype(bool))
    out = metrics.cluster(t(c["dist"]), t(c["cutoff"]), candidates=cand, score=t(c["score"]), max_clusters=None if c["M"] == N else c["M"])
    assert list(out) == [*OUTPUTS, "representative"] and all(v.is_cuda for v in out.values())
    check({k: out[k].cpu().numpy() for k in OUTPUTS}, want, name + " through metrics.cluster")
    rep = np.zeros((G, N), bool)
    for g in range(G):
        rep[g, want["center"][g, :want["count"][g]]] = True
    assert out["representative"].dtype == torch.bool and (out["representative"].cpu().numpy() == rep).all()
    if len(set(c["cutoff"].tolist())) == 1:  # a plain number does what the tensor of it does
        again = metrics.cluster(t(c["dist"]), float(c["cutoff"][0]), candidates=cand, score=t(c["score"]), max_clusters=c["M"])
        assert all(same_bits(again[k].cpu().numpy(), out[k].cpu().numpy()) for k in out)
    host = metrics.cluster(torch.from_numpy(c["dist"]), torch.from_numpy(c["cutoff"]), max_clusters=c["M"])  # results on dist's device
    assert all(not v.is_cuda for v in host.values())


@functools.lru_cache(maxsize=None)
def designs(G=2, N=96, K=24, families=4, seed=21):
    """Synthetic designs: every patch's designs are perturbations of `families` conformations, generated residues 4..19."""
    g = torch.Generator().manual_seed(seed)
    base = 6.0 * torch.randn(G, families, K, 3, generator=g)
    which = torch.randint(0, families, (G, N), generator=g)
    x = base[torch.arange(G)[:, None], which] + 0.3 * torch.randn(G, N, K, 3, generator=g)
    seq = torch.randint(0, 20, (G, families, K), generator=g)[torch.arange(G)[:, None], which]
    gm = torch.zeros(G, K, dtype=torch.bool)
    gm[:, 4:20] = True
    d = {"seq_idx": seq.reshape(G * N, K).cuda(), "translations": x.reshape(G * N, K, 3).cuda(),
         "orientations": torch.eye(3).expand(G * N, K, 3, 3).contiguous().cuda()}
    return d, gm.cuda(), which


def test_pairwise_into_cluster_into_ensemble_and_select_diverse():
    d, gm, which = designs()
    G, N = which.shape
    pw = metrics.pairwise(d, gm, group_size=N)
    out = metrics.cluster(pw["rmsd"], 2.0)
    want = cluster_ref(pw["rmsd"].cpu().numpy(), 2.0)
    check({k: out[k].cpu().numpy() for k in OUTPUTS}, want, "pairwise rmsd")
    assert (want["count"] > 1).all() and (want["size"][:, 0] > 1).all()
    for g in range(G):  # the planted conformations come back as the families
        lab = out["label"][g].cpu()
        assert all(len(set(which[g][lab == c].tolist())) == 1 for c in range(int(out["count"][g])))
    seq = metrics.cluster(1 - pw["seq_identity"], 0.5)
    check({k: seq[k].cpu().numpy() for k in OUTPUTS}, cluster_ref((1 - pw["seq_identity"]).cpu().numpy(), 0.5), "1 - seq_identity")
    # cluster_weights -> ensemble: exactly the labelled designs are weighted
    for idx in (0, torch.tensor([1, 0])):
        w = metrics.cluster_weights(out, idx)
        sel = torch.as_tensor(idx).expand(G) if isinstance(idx, int) else idx
        assert (w.cpu() == (out["label"].cpu() == sel[:, None]).float()).all() and w.is_cuda and w.dtype == torch.float32
        ens = metrics.ensemble(d, gm, group_size=N, weights=w)
        for g in range(G):
            n = float(w[g].sum())
            assert n == float(out["size"][g, int(sel[g])]) and abs(float(ens["n_eff"][g]) - n) < 1e-3 * n
            assert w[g, int(ens["central"][g])] == 1
    # representative -> select_diverse: only centres are picked
    pick = metrics.select_diverse(pw["rmsd"], 3, candidates=out["representative"])
    for g in range(G):
        got = pick["index"][g, :int(pick["count"][g])].tolist()
        assert len(got) == min(3, int(out["count"][g])) and set(got) <= set(out["center"][g, :int(out["count"][g])].tolist())
