"""The Pareto ranking entry on the MI355X: diffab_metrics_pareto through the C ABI and through diffab_pytorch.metrics.pareto (DESIGN.md
section 4.22).

The oracle is test_pareto_host.py's numpy restatement of the rule, run on the SAME fp32 tables the kernels read.  Every output must EQUAL
it - ranks, both domination counts, front sizes, counts and the whole order: the rule is compares, popcounts and integer adds.  No case
is left out and there is no tolerance.  Every case asserts that it is not vacuous - more than one front, and a front of more than one
design - unless it is a named extreme.  The brute-force oracle serves up to 1000 designs, the longest-chain recursion (which
test_pareto_host.py holds equal to it) above.

The contracts of the general C ABI - guard bands, operand alignment, workspace contents, NULL outputs, G = 0 - are held here, on a
harness of this file's own: EVERY oracle case below runs with each operand between guard bands."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from diffab_pytorch import _hip, metrics
from sampler_support import hip  # noqa: F401
from test_pareto_host import INPUTS, OUTPUTS, check_properties, correlated, f32, pareto_ref, pareto_ref_chain, quarters, same_bits

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("hip")]

GUARD = 256  # bytes on either side of every operand
FILL = 0xA5
LDS_MAX = metrics.CLUSTER_LDS_MAX_N
IN_DTYPE = {"objectives": f32, "maximize": np.uint8, "violation": f32, "score": f32, "candidates": np.uint8}
OUT_DTYPE = {k: np.int64 if k == "order" else np.int32 for k in OUTPUTS}
nan, inf = np.nan, np.inf


def out_shape(name, G, N, F):
    return {"front_size": (G, F), "count": (G,), "n_unranked": (G,)}.get(name, (G, N))


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
    """diffab_metrics_pareto on the numpy inputs of `case`.  Every data operand sits between guard bands; with `misaligned`, one element
    (4 bytes floats and int32, 8 bytes the int64 order, 1 byte the masks: the natural alignment) behind a 256-byte boundary.  Outputs
    named in `skip` are passed as NULL.  The workspace is exactly the documented size, filled with `workspace_fill`, between guard bands
    of its own.  Returns the outputs as numpy arrays."""
    lib = _hip.lib()
    G, N, M = case["objectives"].shape
    F = case["F"]
    ops = []
    for name in INPUTS:
        v = case.get(name)
        if v is None:
            ops.append(None)
            continue
        v = np.ascontiguousarray(np.asarray(v).astype(IN_DTYPE[name]))
        ops.append(Operand(v.nbytes, np.dtype(IN_DTYPE[name]).itemsize if misaligned else 0, v))
    outs = {}
    for name in OUTPUTS:
        if name not in skip:
            item = np.dtype(OUT_DTYPE[name]).itemsize
            outs[name] = Operand(int(np.prod(out_shape(name, G, N, F))) * item, item if misaligned else 0)
    nbytes = metrics.pareto_workspace_bytes(G, N)
    ws = Operand(nbytes, 0, fill=workspace_fill)
    null = ctypes.c_void_p(0)
    rc = lib.diffab_metrics_pareto(*[null if o is None else o.ptr for o in ops], G, N, M, F, *[outs[n].ptr if n in outs else null for n in OUTPUTS],
                                   ws.ptr, nbytes, _hip.stream_ptr())
    assert rc == 0, lib.diffab_last_error().decode()
    torch.cuda.synchronize()
    for name, o in list(outs.items()) + [("workspace", ws)] + [(n, o) for n, o in zip(INPUTS, ops) if o is not None]:
        assert o.guards_intact(), f"bytes around {name} were written"
    return {name: o.read(OUT_DTYPE[name], out_shape(name, G, N, F)) for name, o in outs.items()}


def check(out, want, what, names=OUTPUTS):
    for k in names:
        if k in out and not same_bits(out[k], want[k]):
            assert out[k].shape == want[k].shape and out[k].dtype == want[k].dtype, (what, k, out[k].shape, want[k].shape)
            a, b = out[k].reshape(-1), want[k].reshape(-1)
            bad = np.flatnonzero(a != b)
            raise AssertionError(f"{what}: {k} differs at {len(bad)} of {a.size} places, first {bad[:4].tolist()}: got {a[bad[:4]]!r}, oracle {b[bad[:4]]!r}")


# ------------------------------------------------------------------ cases
def case_of(objectives, maximize=None, violation=None, score=None, candidates=None, F=None, extreme=None):
    G, N, M = objectives.shape
    return {"objectives": np.ascontiguousarray(objectives, dtype=f32), "maximize": maximize, "violation": violation, "score": score,
            "candidates": candidates, "F": N if F is None else F, "extreme": extreme}


@functools.lru_cache(maxsize=None)
def straddle_data():
    return quarters(11, 2, LDS_MAX + 1, 3)


def build(name):
    rng = np.random.default_rng(sum(map(ord, name)))
    if name == "N4096":
        return case_of(quarters(5, 1, 4096, 3))
    if name.startswith("N"):  # "N63 M3": three patches with their own data, at a ballot / word / segment boundary
        N, M = int(name.split()[0][1:]), int(name.split()[1][1:])
        return case_of(quarters(N + M, 3, N, M), extreme="fewer than three designs" if N <= 2 else None)
    if name.startswith("correlated"):  # sixteen objectives that still make many fronts
        N = int(name.split()[1])
        return case_of(correlated(N, 2, N, 16))
    if name.startswith("straddle"):  # the same table cut to size, on both sides of the form change
        N = LDS_MAX + int(name.split()[1])
        return case_of(straddle_data()[:, :N])
    if name.startswith("chain"):  # one objective with distinct values: N fronts of one design, the longest loop of either form
        N = LDS_MAX + int(name.split()[1])
        return case_of(rng.permutation(N).astype(f32).reshape(1, N, 1), extreme="N fronts of one design")
    if name == "all equal":
        return case_of(np.full((2, 200, 3), 1.5, f32), extreme="one front")
    if name == "single candidate":
        cand = np.zeros((2, 130), bool)
        cand[0, 77] = cand[1, 129] = True
        return case_of(quarters(3, 2, 130, 3), candidates=cand, extreme="a single candidate")
    if name == "candidates":  # random candidates; patch 1 has none
        cand = rng.random((3, 150)) < 0.6
        cand[1] = False
        return case_of(quarters(7, 3, 150, 3), candidates=cand)
    if name == "nan entries":  # NaNs of both signs, infinities and both zeros among the values
        t = quarters(12, 2, 131, 3)
        t[rng.random(t.shape) < 0.2] = nan
        t[rng.random(t.shape) < 0.05] = -nan
        t[rng.random(t.shape) < 0.05] = inf
        t[rng.random(t.shape) < 0.05] = -inf
        t[rng.random(t.shape) < 0.05] = -0.0
        return case_of(t, maximize=[False, True, False])
    if name == "maximize all":
        return case_of(quarters(13, 2, 140, 3), maximize=[True] * 3)
    if name == "maximize mixed":
        return case_of(quarters(13, 2, 140, 4), maximize=[False, True, True, False])
    if name == "violation":  # ties at 0 among negative, -0, +0, then positive values, infinities and NaNs
        vio = rng.choice(np.array([-inf, -2.0, -0.0, 0.0, 0.0, 1e-30, 0.5, 0.5, 3.0, inf, nan], f32), (2, 300))
        return case_of(quarters(14, 2, 300, 2), violation=vio, candidates=rng.random((2, 300)) < 0.9)
    if name == "scores":  # ties among the scores - both zeros, both infinities, NaNs
        score = rng.choice(np.array([-inf, -1.5, -0.0, 0.0, 1e-30, 2.0, inf, nan], f32), (2, 140))
        return case_of(quarters(8, 2, 140, 2), score=score, candidates=rng.random((2, 140)) < 0.9)
    if name == "everything past 1024":
        N = LDS_MAX + 70
        return case_of(quarters(15, 1, N, 3), maximize=[True, False, False], violation=rng.integers(-2, 3, (1, N)).astype(f32),
                       score=rng.integers(0, 2, (1, N)).astype(f32), candidates=rng.random((1, N)) < 0.7, F=5)
    if name.startswith("max_fronts"):  # 0, 1, and a value hit mid-way (the tables have ten fronts and more)
        F = int(name.split()[1])
        return case_of(quarters(16, 2, 90, 2), F=F, extreme=None if F > 1 else f"max_fronts = {F}")
    raise KeyError(name)


CASES = (["N1 M3", "N2 M3", "N63 M3", "N64 M3", "N65 M3", "N127 M3", "N129 M3", "N129 M1", "N129 M2", "N255 M2", "N256 M2", "N257 M2",
          "correlated 129", "correlated 1024", "straddle -1", "straddle 0", "straddle +1", "N4096", "chain 0", "chain +1", "all equal",
          "single candidate", "candidates", "nan entries", "maximize all", "maximize mixed", "violation", "scores", "everything past 1024",
          "max_fronts 0", "max_fronts 1", "max_fronts 4"])


@functools.lru_cache(maxsize=None)
def get(name):
    """(case, oracle): built and solved once, shared by the tests below and left unchanged."""
    c = build(name)
    oracle = pareto_ref_chain if c["objectives"].shape[1] > 1000 else pareto_ref
    want = oracle(c["objectives"], maximize=c["maximize"], violation=c["violation"], score=c["score"], candidates=c["candidates"], max_fronts=c["F"])
    if c["extreme"] is None:
        busy = [g for g in range(len(want["count"])) if c["candidates"] is None or c["candidates"][g].any()]
        assert all(want["count"][g] > 1 and want["front_size"][g].max() > 1 for g in busy), f"{name} is vacuous: {want['count']}, {want['front_size'][:, :3]}"
    return c, want


@pytest.mark.parametrize("name", CASES)
def test_every_output_equals_the_oracle(name):
    c, want = get(name)
    out = call_abi(c)
    check(out, want, name)
    if c["objectives"].shape[1] <= 300:
        check_properties(out, c["objectives"], c["maximize"], c["violation"], c["candidates"], c["F"])


def test_the_cases_reach_what_they_are_named_for():
    assert get("chain 0")[1]["count"].tolist() == [LDS_MAX] and get("chain +1")[1]["count"].tolist() == [LDS_MAX + 1]
    assert (get("chain +1")[1]["front_size"] == 1).all()
    assert get("all equal")[1]["count"].tolist() == [1, 1] and get("all equal")[1]["front_size"][:, 0].tolist() == [200, 200]
    assert get("single candidate")[1]["count"].tolist() == [1, 1] and get("single candidate")[1]["rank"][1, 129] == 0
    assert get("candidates")[1]["count"][1] == 0 and get("candidates")[1]["n_unranked"].tolist() == [0, 0, 0]
    assert get("max_fronts 0")[1]["n_unranked"].tolist() == [90, 90] and (get("max_fronts 4")[1]["n_unranked"] > 0).all()
    assert (get("max_fronts 4")[1]["count"] == 4).all() and (get("everything past 1024")[1]["n_unranked"] > 0).all()
    assert (get("correlated 129")[1]["count"] > 5).all() and (get("correlated 1024")[1]["count"] > 5).all()  # not the one front of independent objectives
    assert 20 < get("N4096")[1]["count"][0] < 200  # tens of fronts
    for name, key in (("scores", "score"), ("violation", "violation"), ("maximize all", "maximize"), ("maximize mixed", "maximize"),
                      ("nan entries", "maximize")):  # the operand decides: without it the answer is another
        c, want = get(name)
        kw = {k: c[k] for k in ("maximize", "violation", "score", "candidates") if k != key}
        plain = pareto_ref(c["objectives"], max_fronts=c["F"], **kw)
        assert not same_bits(plain["order"], want["order"]), name
    for a, b in (("straddle -1", "straddle 0"), ("straddle 0", "straddle +1")):  # the cut changes the data, not only the form
        assert not same_bits(get(a)[1]["front_size"][:, :8], get(b)[1]["front_size"][:, :8])


def alone(c, g):
    return dict(c, objectives=c["objectives"][g:g + 1], **{k: None if c[k] is None else c[k][g:g + 1] for k in ("violation", "score", "candidates")})


@pytest.mark.parametrize("name", ["N129 M3", "straddle 0", "straddle +1", "candidates", "violation"])
def test_a_patch_alone_gives_what_it_gives_in_its_batch(name):
    c, want = get(name)
    g = c["objectives"].shape[0] - 1
    check(call_abi(alone(c, g)), {k: v[g:g + 1] for k, v in want.items()}, name + ", last patch alone")


@pytest.mark.parametrize("name", ["N129 M3", "straddle 0", "straddle +1", "everything past 1024"])
def test_what_the_workspace_held_is_ignored(name):
    c, want = get(name)
    for fill in (0x00, 0xFF):
        check(call_abi(c, workspace_fill=fill), want, f"{name}, workspace full of {fill:#x}")


@pytest.mark.parametrize("name", ["N65 M3", "N127 M3", "scores", "violation", "maximize mixed", "straddle +1"])
def test_operands_at_their_natural_alignment(name):
    c, want = get(name)
    check(call_abi(c, misaligned=True), want, name + ", misaligned")


def test_null_outputs_are_skipped():
    c, want = get("candidates")
    nullable = ("n_dominators", "n_dominated", "n_unranked", "order")
    for skip in [(k,) for k in nullable] + [nullable]:
        out = call_abi(c, skip=skip)
        assert not set(skip) & set(out)
        check(out, want, f"candidates without {skip}")
    c, want = get("max_fronts 0")  # with F = 0 front_size may be NULL too
    check(call_abi(c, skip=("front_size", "order")), want, "max_fronts 0 without front_size")


def test_an_empty_problem_returns_before_any_pointer_is_read(hip):
    null = ctypes.c_void_p(0)
    assert hip.diffab_metrics_pareto(*[null] * 5, 0, 8, 3, 2, *[null] * 7, null, 0, _hip.stream_ptr()) == 0
    out = metrics.pareto(torch.zeros(0, 8, 3, device="cuda"), max_fronts=3)
    assert tuple(out["rank"].shape) == (0, 8) and tuple(out["front_size"].shape) == (0, 3) and tuple(out["front"].shape) == (0, 8)


# ------------------------------------------------------------------ through the package
def t(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.mark.parametrize("name", ["N129 M3", "candidates", "scores", "violation", "maximize mixed", "max_fronts 4", "straddle +1"])
def test_the_python_entry(name):
    c, want = get(name)
    G, N, M = c["objectives"].shape
    kw = dict(maximize=c["maximize"], violation=t(c["violation"]), score=t(c["score"]),
              candidates=None if c["candidates"] is None else t(c["candidates"].astype(bool)), max_fronts=None if c["F"] == N else c["F"])
    out = metrics.pareto(t(c["objectives"]), **kw)
    assert list(out) == [*OUTPUTS, "front"] and all(v.is_cuda for v in out.values())
    check({k: out[k].cpu().numpy() for k in OUTPUTS}, want, name + " through metrics.pareto")
    assert out["front"].dtype == torch.bool and (out["front"].cpu().numpy() == (want["rank"] == 0)).all()
    # the per-design form the filters return: M flat tensors of G * N elements, one of them integer where the values allow it
    flat = [t(c["objectives"][:, :, m].reshape(-1)) for m in range(M)]
    if np.isfinite(c["objectives"][:, :, 0]).all():
        flat[0] = (flat[0] * 4).to(torch.int32)  # (quarters: a positive scale keeps every compare)
    again = metrics.pareto(flat, group_size=N, **kw)
    assert all(same_bits(again[k].cpu().numpy(), out[k].cpu().numpy()) for k in out)
    host = metrics.pareto(torch.from_numpy(c["objectives"]), maximize=c["maximize"], max_fronts=c["F"])  # results on the objectives' device
    assert all(not v.is_cuda for v in host.values())


@functools.lru_cache(maxsize=None)
def designs(G=2, N=64, K=24, families=4, seed=21):
    """Synthetic designs: every patch's designs are perturbations of `families` conformations, generated residues 4..19; the native is
    the first conformation, and residues 0..3 stand for the antigen."""
    g = torch.Generator().manual_seed(seed)
    base = 6.0 * torch.randn(G, families, K, 3, generator=g)
    which = torch.randint(0, families, (G, N), generator=g)
    x = base[torch.arange(G)[:, None], which] + 1.0 * torch.randn(G, N, K, 3, generator=g)
    fam_seq = torch.randint(0, 20, (G, families, K), generator=g)
    seq = fam_seq[torch.arange(G)[:, None], which].clone()
    mutate = torch.rand(G, N, K, generator=g) < 0.3
    seq[mutate] = torch.randint(0, 20, (int(mutate.sum()),), generator=g)
    gm = torch.zeros(G, K, dtype=torch.bool)
    gm[:, 4:20] = True
    ag = torch.zeros(G, K, dtype=torch.bool)
    ag[:, :4] = True
    eye = torch.eye(3)
    d = {"seq_idx": seq.reshape(G * N, K).cuda(), "translations": x.reshape(G * N, K, 3).cuda(),
         "orientations": eye.expand(G * N, K, 3, 3).contiguous().cuda()}
    native = {"seq_idx": fam_seq[:, 0].cuda(), "translations": base[:, 0].contiguous().cuda(), "orientations": eye.expand(G, K, 3, 3).contiguous().cuda()}
    return d, native, gm.cuda(), ag.cuda()


def test_evaluate_and_contacts_into_pareto_into_select_diverse_and_ensemble():
    d, native, gm, ag = designs()
    G, N = 2, 64
    ev = metrics.evaluate(d, native, gm, group_size=N)
    ct = metrics.contacts(d, gm, antigen_mask=ag, group_size=N)
    cols = [ev["rmsd"], ev["aar"], ct["n_contact_pairs"]]  # (rows,) each, as the filters return them; the last is int32
    mx = [False, True, True]
    limit = ct["clash_score"].median()
    out = metrics.pareto(cols, group_size=N, maximize=mx, violation=ct["clash_score"] .view(G, N) - limit, score=ev["rmsd"].view(G, N))
    table = np.stack([c.float().view(G, N).cpu().numpy() for c in cols], -1)
    want = pareto_ref(table, maximize=mx, violation=(ct["clash_score"].view(G, N) - limit).cpu().numpy(), score=ev["rmsd"].view(G, N).cpu().numpy())
    check({k: out[k].cpu().numpy() for k in OUTPUTS}, want, "evaluate and contacts")
    assert (want["count"] > 1).all() and (want["front_size"][:, 0] > 1).all() and (want["front_size"][:, 0] < N).all()
    front = out["front"]
    pw = metrics.pairwise(d, gm, group_size=N)
    pick = metrics.select_diverse(pw["rmsd"], 3, candidates=front)
    ens = metrics.ensemble(d, gm, group_size=N, weights=front.float())
    for g in range(G):
        on = set(np.flatnonzero(want["rank"][g] == 0).tolist())
        got = pick["index"][g, :int(pick["count"][g])].tolist()
        assert len(got) == min(3, len(on)) and set(got) <= on  # every pick lies on front 0
        assert set(out["order"][g, :len(on)].tolist()) == on
        assert abs(float(ens["n_eff"][g]) - len(on)) < 1e-3 * len(on) and int(ens["central"][g]) in on
