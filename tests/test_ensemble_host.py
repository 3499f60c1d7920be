"""CPU: the host side of the design ensembles (diffab_pytorch.metrics.ensemble) - the float64 numpy oracle of the rule and its hand-computed
cases, the C-ABI entry and its host-side refusals, and the argument checks that happen before any library call.

The rule is DESIGN.md section 4.16 / the comment of diffab_metrics_ensemble in include/diffab_hip.h.  test_gpu_ensemble.py imports the
oracle from here."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

from diffab_pytorch import _hip, metrics
from sampler_support import ReachedTheLibrary, refuse_library

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------ the oracle (shared with test_gpu_ensemble.py)
def ensemble_ref(seq, pts, gen, residue_mask=None, weights=None, group_size=1, num_classes=21, pseudocount=0.0):
    """seq (rows,K) integers, pts (rows,K,P,3), masks (G,K), weights (rows,) or (G,N) or None -> the ten outputs of the rule as float64
    (consensus_identity as the fp32 quotient, consensus / central int64), plus central_gap (G,): the difference between the smallest
    and the second smallest rmsd_to_mean among the designs that can win (inf with fewer than two)."""
    seq, pts = np.asarray(seq), np.asarray(pts, np.float64)
    rows, K = seq.shape
    N, V, P, a = group_size, num_classes, pts.shape[2], float(pseudocount)
    G = rows // N
    w_all = np.ones(rows) if weights is None else np.asarray(weights, np.float64).reshape(rows)
    w_all = np.where(np.isfinite(w_all) & (w_all > 0), w_all, 0.0)  # a negative or non-finite weight is 0
    out = {"aa_freq": np.full((G, K, V), np.nan), "entropy": np.full((G, K), np.nan), "consensus": np.full((G, K), -1, np.int64),
           "mean_points": np.full((G, K, P, 3), np.nan), "rmsf": np.full((G, K), np.nan), "log_prob": np.full(rows, np.nan),
           "consensus_identity": np.full(rows, np.nan, np.float32), "rmsd_to_mean": np.full(rows, np.nan), "n_eff": np.full(G, np.nan),
           "central": np.full(G, -1, np.int64), "central_gap": np.full(G, np.inf)}
    with np.errstate(divide="ignore", invalid="ignore"):
        for g in range(G):
            inside = np.ones(K, bool) if residue_mask is None else np.asarray(residue_mask[g], bool)
            counted = inside & np.asarray(gen[g], bool)
            s, p, w = seq[g * N:(g + 1) * N], pts[g * N:(g + 1) * N], w_all[g * N:(g + 1) * N]
            use = w > 0  # a design of weight 0 takes no part in a sum over designs
            c = np.stack([(w[use, None] * (s[use] == v)).sum(0) for v in range(V)], 1)  # (K,V)
            Wk = c.sum(1)
            f = np.where((Wk + a > 0)[:, None], (c + a / V) / (Wk + a)[:, None], np.nan)
            lnf = np.log(f)
            ent = 0.0 + np.where(f > 0, -(f * lnf), 0.0).sum(1)
            ent[np.isnan(f).any(1)] = np.nan
            cons = np.where(Wk > 0, np.argmax(c, 1), -1)  # argmax returns the first maximum: the smallest class
            W = w.sum()
            mean = (w[use, None, None, None] * p[use]).sum(0) / W if W > 0 else np.full((K, P, 3), np.nan)
            d2 = ((p - mean[None]) ** 2).sum((-1, -2))  # (N,K)
            rmsf = np.sqrt((w[use, None] * d2[use]).sum(0) / (W * P))
            out["aa_freq"][g, inside], out["entropy"][g, inside], out["consensus"][g, inside] = f[inside], ent[inside], cons[inside]
            out["mean_points"][g, inside], out["rmsf"][g, inside] = mean[inside], rmsf[inside]
            out["n_eff"][g] = W * W / (w * w).sum() if W > 0 else np.nan
            n = int(counted.sum())
            if n == 0:
                continue
            ks = np.flatnonzero(counted)
            tok = s[:, ks]
            known = (tok >= 0) & (tok < V)
            terms = np.where(known, lnf[ks[None, :], np.clip(tok, 0, V - 1)], -np.inf)
            rd = np.sqrt(d2[:, ks].sum(1) / (n * P))
            lo = g * N
            out["log_prob"][lo:lo + N] = terms.sum(1) / n
            out["consensus_identity"][lo:lo + N] = ((cons[ks][None] >= 0) & (tok == cons[ks][None])).sum(1).astype(np.float32) / np.float32(n)
            out["rmsd_to_mean"][lo:lo + N] = rd
            can = np.flatnonzero(use & ~np.isnan(rd.astype(np.float32)))
            if can.size:
                key = rd.astype(np.float32)[can]
                out["central"][g] = can[np.argmin(key)]  # argmin returns the first minimum: ties to the lower index
                if can.size > 1:
                    two = np.sort(rd[can])[:2]
                    out["central_gap"][g] = two[1] - two[0]
    return out


# ------------------------------------------------------------------ hand-computed cases
def ca(x):
    """(rows,K) x coordinates -> CA points (rows,K,1,3) on the x axis."""
    x = np.asarray(x, np.float64)
    return np.stack([x, np.zeros_like(x), np.zeros_like(x)], -1)[:, :, None, :]


def test_oracle_single_design():
    seq = np.array([[4, 0, 20]])
    pts = ca([[1.5, -2.0, 7.0]])
    gen = np.array([[True, True, False]])
    out = ensemble_ref(seq, pts, gen, group_size=1)
    want = np.zeros((1, 3, 21))
    want[0, [0, 1, 2], [4, 0, 20]] = 1.0
    assert np.array_equal(out["aa_freq"], want) and (out["entropy"] == 0).all() and not np.signbit(out["entropy"]).any()
    assert out["consensus"].tolist() == [[4, 0, 20]] and np.array_equal(out["mean_points"], pts[:1].reshape(1, 3, 1, 3))
    assert (out["rmsf"] == 0).all() and out["log_prob"].tolist() == [0.0] and out["consensus_identity"].tolist() == [1.0]
    assert out["rmsd_to_mean"].tolist() == [0.0] and out["n_eff"].tolist() == [1.0] and out["central"].tolist() == [0]
    # no counted position: the per-design numbers are NaN, central is -1; the per-position ones stay
    none = ensemble_ref(seq, pts, np.zeros((1, 3), bool), group_size=1)
    assert np.isnan(none["log_prob"]).all() and np.isnan(none["consensus_identity"]).all() and np.isnan(none["rmsd_to_mean"]).all()
    assert none["central"].tolist() == [-1] and np.array_equal(none["aa_freq"], want)
    # outside residue_mask: NaN and -1
    rm = np.array([[True, False, True]])
    part = ensemble_ref(seq, pts, gen, residue_mask=rm, group_size=1)
    assert np.isnan(part["aa_freq"][0, 1]).all() and np.isnan(part["entropy"][0, 1]) and part["consensus"][0, 1] == -1
    assert np.isnan(part["mean_points"][0, 1]).all() and np.isnan(part["rmsf"][0, 1]) and part["entropy"][0, 0] == 0


def test_oracle_two_designs_that_differ_at_one_position():
    seq = np.array([[3, 7], [3, 9]])
    pts = ca([[0.0, 1.0], [0.0, 3.0]])
    out = ensemble_ref(seq, pts, np.ones((1, 2), bool), group_size=2)
    assert out["aa_freq"][0, 0, 3] == 1.0 and out["aa_freq"][0, 1, 7] == 0.5 and out["aa_freq"][0, 1, 9] == 0.5
    assert out["aa_freq"].sum() == 2.0 and out["entropy"][0, 0] == 0 and abs(out["entropy"][0, 1] - math.log(2)) < 1e-15
    assert out["consensus"].tolist() == [[3, 7]]  # a tie goes to the smaller class
    assert out["mean_points"][0, :, 0, 0].tolist() == [0.0, 2.0] and out["rmsf"][0].tolist() == [0.0, 1.0]
    assert np.allclose(out["log_prob"], [math.log(0.5) / 2] * 2, rtol=0, atol=1e-15)
    assert out["consensus_identity"].tolist() == [1.0, 0.5] and np.allclose(out["rmsd_to_mean"], [math.sqrt(0.5)] * 2, rtol=0, atol=1e-15)
    assert out["n_eff"].tolist() == [2.0] and out["central"].tolist() == [0] and out["central_gap"].tolist() == [0.0]


def test_oracle_three_weighted_designs():
    """Weights 1, 2, 1 (W = 4).  Position 0: tokens 3, 3, 5 -> c_3 = 3, c_5 = 1; x = 0, 2, 4 -> mean (0 + 4 + 4) / 4 = 2,
    rmsf sqrt((4 + 0 + 4) / 4).  Position 1: tokens 0, 1, 2 -> f = 1/4, 1/2, 1/4; every design at x = 1."""
    seq = np.array([[3, 0], [3, 1], [5, 2]])
    pts = ca([[0.0, 1.0], [2.0, 1.0], [4.0, 1.0]])
    out = ensemble_ref(seq, pts, np.ones((1, 2), bool), weights=np.array([1.0, 2.0, 1.0]), group_size=3)
    f = out["aa_freq"][0]
    assert f[0, 3] == 0.75 and f[0, 5] == 0.25 and f[1, :3].tolist() == [0.25, 0.5, 0.25] and f.sum() == 2.0
    assert abs(out["entropy"][0, 0] + 0.75 * math.log(0.75) + 0.25 * math.log(0.25)) < 1e-15
    assert abs(out["entropy"][0, 1] - 1.5 * math.log(2)) < 1e-15
    assert out["consensus"].tolist() == [[3, 1]]
    assert out["mean_points"][0, :, 0, 0].tolist() == [2.0, 1.0] and np.allclose(out["rmsf"][0], [math.sqrt(2.0), 0.0], rtol=0, atol=1e-15)
    want = [(math.log(0.75) + math.log(0.25)) / 2, (math.log(0.75) + math.log(0.5)) / 2, math.log(0.25)]
    assert np.allclose(out["log_prob"], want, rtol=0, atol=1e-15)
    assert out["consensus_identity"].tolist() == [0.5, 1.0, 0.0]
    assert np.allclose(out["rmsd_to_mean"], [math.sqrt(2.0), 0.0, math.sqrt(2.0)], rtol=0, atol=1e-15)
    assert abs(out["n_eff"][0] - 16.0 / 6.0) < 1e-15 and out["central"].tolist() == [1]
    # the same weights as (G, N); a negative, an infinite and a NaN weight are 0: only design 1 is left
    again = ensemble_ref(seq, pts, np.ones((1, 2), bool), weights=np.array([[1.0, 2.0, 1.0]]), group_size=3)
    assert all(np.array_equal(out[k], again[k], equal_nan=True) for k in out)
    alone = ensemble_ref(seq, pts, np.ones((1, 2), bool), weights=np.array([-1.0, 2.0, np.inf]), group_size=3)
    assert alone["aa_freq"][0, 0, 3] == 1.0 and alone["n_eff"].tolist() == [1.0] and alone["central"].tolist() == [1]
    assert alone["mean_points"][0, :, 0, 0].tolist() == [2.0, 1.0] and alone["log_prob"].tolist() == [-np.inf, 0.0, -np.inf]
    # all weights 0: nothing is defined but the shapes
    zero = ensemble_ref(seq, pts, np.ones((1, 2), bool), weights=np.zeros(3), group_size=3)
    assert np.isnan(zero["aa_freq"]).all() and np.isnan(zero["entropy"]).all() and (zero["consensus"] == -1).all()
    assert np.isnan(zero["mean_points"]).all() and np.isnan(zero["rmsf"]).all() and np.isnan(zero["n_eff"]).all()
    assert np.isnan(zero["log_prob"]).all() and np.isnan(zero["rmsd_to_mean"]).all() and zero["central"].tolist() == [-1]
    assert zero["consensus_identity"].tolist() == [0.0, 0.0, 0.0]  # (no position has a consensus: nothing matches)


def test_oracle_pseudocount_where_no_token_is_in_a_class():
    seq = np.array([[-1, 2], [21, 2]])  # position 0: no token in [0, 21)
    pts = ca([[0.0, 0.0], [0.0, 0.0]])
    bare = ensemble_ref(seq, pts, np.ones((1, 2), bool), group_size=2)
    assert np.isnan(bare["aa_freq"][0, 0]).all() and np.isnan(bare["entropy"][0, 0]) and bare["consensus"][0, 0] == -1
    assert bare["log_prob"].tolist() == [-np.inf, -np.inf]  # a token outside the classes is -inf whatever the frequencies are
    inside = ensemble_ref(np.array([[-1, 2], [21, 2], [4, 2]]), ca(np.zeros((3, 2))), np.ones((1, 2), bool), weights=np.array([1.0, 1.0, 0.0]),
                          group_size=3)
    assert np.isnan(inside["log_prob"][2]) and inside["log_prob"][:2].tolist() == [-np.inf, -np.inf]  # token 4 meets a NaN frequency
    out = ensemble_ref(seq, pts, np.ones((1, 2), bool), group_size=2, pseudocount=0.5)
    assert np.allclose(out["aa_freq"][0, 0], 1.0 / 21.0, rtol=0, atol=1e-17) and abs(out["entropy"][0, 0] - math.log(21)) < 1e-14
    assert out["consensus"][0, 0] == -1 and out["consensus"][0, 1] == 2
    assert abs(out["aa_freq"][0, 1, 2] - (2 + 0.5 / 21) / 2.5) < 1e-16 and abs(out["aa_freq"][0, 1, 0] - (0.5 / 21) / 2.5) < 1e-17
    assert out["log_prob"].tolist() == [-np.inf, -np.inf] and out["consensus_identity"].tolist() == [0.5, 0.5]
    # V = 2: token 2 is outside as well; the pseudocount alone gives the uniform distribution and ln V
    small = ensemble_ref(seq, pts, np.ones((1, 2), bool), group_size=2, num_classes=2, pseudocount=1.0)
    assert (small["aa_freq"] == 0.5).all() and np.allclose(small["entropy"], math.log(2), rtol=0, atol=1e-15)


# ------------------------------------------------------------------ C ABI
NAME = "diffab_metrics_ensemble"


def header_code():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "diffab_hip.h")).read(), flags=re.S)


def test_header_and_symbol_table_declare_the_entry():
    code = header_code()
    lib = _hip.load_library()
    assert re.search(r"\bint\s+" + NAME + r"\s*\(", code)
    assert NAME in _hip.SYMBOLS and hasattr(lib, NAME)
    res, args = _hip.SYMBOLS[NAME]
    assert res is ctypes.c_int and len(args) == 24 and args[5:10] == [ctypes.c_int32] * 5 and args[10] is ctypes.c_double
    assert args[22] is ctypes.c_size_t and all(a is ctypes.c_void_p for a in args[:5] + args[11:22] + args[23:])
    limit = re.search(r"#define\s+DIFFAB_METRICS_MAX_CLASSES\s+\(?(\d+)\)?", code)
    assert limit and int(limit.group(1)) == metrics.MAX_CLASSES == 32


def test_workspace_bytes_equals_the_macro():
    """The macro of the header, evaluated from its text, is ensemble_workspace_bytes; the entry asks for no more than it and for no
    less than it minus the alignment allowance."""
    code = header_code().replace("\\\n", " ")
    m = re.search(r"#define\s+DIFFAB_METRICS_ENSEMBLE_WORKSPACE_BYTES\(G, N, K, P, V\)\s+(.*)", code)
    assert m
    expr = m.group(1).replace("(size_t)", "").replace("/", "//")
    l = _hip.load_library()
    p, null = ctypes.c_void_p(4096), ctypes.c_void_p(0)
    for G, N, K, P, V in ((1, 1, 1, 1, 1), (3, 5, 70, 4, 21), (2, 130, 33, 1, 20), (16, 1024, 128, 4, 21), (7, 4096, 4096, 5, 32)):
        need = eval(expr, {"G": G, "N": N, "K": K, "P": P, "V": V})
        assert need == metrics.ensemble_workspace_bytes(G, N, K, P, V), (G, N, K, P, V)
        rc = l.diffab_metrics_ensemble(p, p, p, null, null, G, N, K, P, V, 0.0, *[p] * 10, p, 16, null)
        assert rc == -4 and "needed" in l.diffab_last_error().decode()  # DIFFAB_ERR_WORKSPACE
        asked = int(re.search(r"(\d+) needed", l.diffab_last_error().decode()).group(1))
        assert need - 4096 <= asked <= need, (G, N, K, P, V, asked, need)


def test_host_side_refusals_touch_no_gpu():
    """Every refusal is decided from the scalar arguments and whether a pointer is null: the pointers are fake addresses that are never
    dereferenced, nothing is enqueued (no GPU is needed), and diffab_last_error names the problem."""
    l = _hip.load_library()
    p, null = ctypes.c_void_p(4096), ctypes.c_void_p(0)

    def err():
        return l.diffab_last_error().decode()

    def call(G=2, N=8, K=128, P=4, V=21, a=0.0, seq=p, pts=p, gm=p, ws=p, ws_bytes=1 << 40):
        return l.diffab_metrics_ensemble(seq, pts, gm, null, null, G, N, K, P, V, a, *[p] * 10, ws, ws_bytes, null)

    for kw, word in ((dict(V=0), "classes outside"), (dict(V=33), "classes outside"), (dict(V=-1), "classes outside"),
                     (dict(N=4097), "at most 4096 designs"), (dict(N=0), "extent"), (dict(G=-1), "extent"), (dict(K=0), "extent"),
                     (dict(K=4097), "at most 4096"), (dict(P=0), "points per residue"), (dict(P=6), "points per residue"),
                     (dict(a=-0.5), "pseudocount"), (dict(a=float("nan")), "pseudocount"), (dict(a=float("inf")), "pseudocount"),
                     (dict(seq=null), "null input"), (dict(pts=null), "null input"), (dict(gm=null), "null input"),
                     (dict(ws=null), "workspace"), (dict(ws=ctypes.c_void_p(4100)), "16-byte aligned")):
        rc = call(**kw)
        assert rc == -1 and word in err(), (kw, rc, err())  # DIFFAB_ERR_ARG
    need = metrics.ensemble_workspace_bytes(2, 8, 128, 4, 21)
    assert call(ws_bytes=need // 2) == -4 and "needed" in err()  # DIFFAB_ERR_WORKSPACE
    # an empty problem returns 0 before any pointer is looked at
    assert l.diffab_metrics_ensemble(*[null] * 5, 0, 8, 128, 1, 21, 0.0, *[null] * 10, null, 0, null) == 0


# ------------------------------------------------------------------ argument errors before any device work
@pytest.fixture
def no_library(monkeypatch):
    refuse_library(monkeypatch)


def frames(rows=6, K=16):
    return {"seq_idx": torch.zeros(rows, K, dtype=torch.long), "translations": torch.zeros(rows, K, 3),
            "orientations": torch.eye(3).expand(rows, K, 3, 3)}


def mask(G=2, K=16):
    m = torch.zeros(G, K, dtype=torch.bool)
    m[:, 3:9] = True
    return m


def test_good_arguments_reach_the_library(no_library):
    with pytest.raises(ReachedTheLibrary):
        metrics.ensemble(frames(), mask(), group_size=3)
    with pytest.raises(ReachedTheLibrary):
        metrics.ensemble(frames(), mask(), group_size=3, residue_mask=mask(), weights=torch.ones(2, 3), atoms="backbone", num_classes=32,
                         pseudocount=1)
    with pytest.raises(ReachedTheLibrary):
        metrics.ensemble(frames(), mask(), group_size=3, weights=torch.ones(6, dtype=torch.float64), num_classes=1, pseudocount=0.5)


@pytest.mark.parametrize("kw, match", [
    (dict(atoms="cb"), "atoms must be 'ca' or 'backbone'"), (dict(group_size=4), "6 design rows are not a multiple of group_size = 4"),
    (dict(group_size=0), "group_size must be"), (dict(group_size=True), "group_size must be"),
    (dict(generation_mask=mask().long()), "generation_mask must be a bool tensor"), (dict(generation_mask=mask(3)), "generation_mask is"),
    (dict(residue_mask=mask(2, 15)), "residue_mask is"), (dict(residue_mask=mask().float()), "residue_mask must be a bool tensor"),
    (dict(designs={"seq_idx": torch.zeros(6, 16, dtype=torch.long)}), "designs must be a dict"),
    (dict(designs=dict(frames(), seq_idx=torch.zeros(6, 16))), r"designs\['seq_idx'\] must be an integer tensor"),
    (dict(designs=dict(frames(), translations=torch.zeros(6, 15, 3))), r"designs\['translations'\] is"),
    (dict(designs=dict(frames(), orientations=torch.zeros(6, 16, 3)), atoms="backbone"), r"designs\['orientations'\] must be"),
    (dict(designs=frames(4097, 4), generation_mask=mask(1, 4), group_size=4097), "at most 4096 designs"),
    (dict(weights=torch.ones(3, 2)), r"weights is \(3, 2\)"), (dict(weights=torch.ones(5)), r"weights is \(5,\)"),
    (dict(weights=torch.ones(2, 3, 1)), "weights is"), (dict(weights=torch.ones(2, 3, dtype=torch.long)), "weights must be a float tensor"),
    (dict(weights=torch.ones(2, 3, dtype=torch.bool)), "weights must be a float tensor"), (dict(weights=[1.0] * 6), "weights must be a float tensor"),
    (dict(num_classes=0), r"num_classes = 0 outside \[1, 32\]"), (dict(num_classes=33), r"num_classes = 33 outside \[1, 32\]"),
    (dict(num_classes=21.0), "num_classes = 21.0 outside"), (dict(num_classes=True), "num_classes = True outside"),
    (dict(pseudocount=-1e-3), "pseudocount must be a finite number >= 0"), (dict(pseudocount=float("nan")), "pseudocount must be"),
    (dict(pseudocount=float("inf")), "pseudocount must be"), (dict(pseudocount="1"), "pseudocount must be"),
    (dict(pseudocount=True), "pseudocount must be"),
])
def test_argument_errors(no_library, kw, match):
    args = dict(designs=frames(), generation_mask=mask(), group_size=3)
    args.update(kw)
    designs, gm = args.pop("designs"), args.pop("generation_mask")
    with pytest.raises(ValueError, match=r"metrics\.ensemble\(\): .*" + match):
        metrics.ensemble(designs, gm, **args)
