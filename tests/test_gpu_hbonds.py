"""The hydrogen-bond entry on the MI355X: diffab_metrics_hbonds through the C ABI and through diffab_pytorch.metrics.hbonds (DESIGN.md
section 4.20).

The oracle is test_hbonds_host.py's numpy restatement of the rule, run on the SAME fp32 atoms the kernels read.  Every output must EQUAL
it - integers, states, the bits of O and H, and the bits of every energy: the derived atoms and the energies are float64 expressions of
float32 numbers in a written order, rounded once, and float64 + - * / sqrt are correctly rounded on both sides.  No case is left out and
there is no tolerance.  A case whose oracle has an energy within 1e-9 of -0.5 or a CA d2 of exactly 81 would not be a fair one: the
cases below are chosen (on the CPU) so that none has, and assert it rather than skip.  Every case also asserts that its oracle finds
bonds with a generated end: none passes vacuously.

The contracts of the general C ABI that the pinned tables of the older test files cannot take for a new entry - workspace contents,
operand alignment, output extents, NULL outputs, rows = 0 - are held here, on a harness of this file's own."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from diffab_pytorch import _hip, io as dio, metrics
from sampler_support import hip  # noqa: F401
from test_geometry_host import tangle_chain_keys
from test_hbonds_host import OUTPUTS, RESIDUE_OUTPUTS, backbone, f32, f64, hbonds_ref, helix, links, place, rotation, strands

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("hip")]

GUARD = 256  # bytes on either side of every operand
FILL = 0xA5
OUT_SPEC = {"O": (f32, 3), "H": (f32, 3), "nh_o_partner": (np.int32, 2), "nh_o_energy": (f32, 2), "o_hn_partner": (np.int32, 2),
            "o_hn_energy": (f32, 2), "bridge_partner": (np.int32, 2), "bridge_parallel": (np.uint8, 2), "ss": (np.uint8, 1),
            "residue_hbonds": (np.int32, 1), "n_hbonds": (np.int32, 0), "n_hbonds_internal": (np.int32, 0), "n_hbonds_antigen": (np.int32, 0),
            "n_hbonds_framework": (np.int32, 0), "n_hotspot_bonded": (np.int32, 0), "n_hotspot": (np.int32, 0), "hbond_energy": (f32, 0),
            "ss_count": (np.int32, 8)}
INPUTS = (("points", f32), ("donor_off", np.uint8), ("ctx_points", f32), ("ctx_valid", np.uint32), ("ctx_donor_off", np.uint8), ("gen", np.uint8),
          ("rm", np.uint8), ("antigen", np.uint8), ("hotspot", np.uint8), ("chain", np.int32), ("ridx", np.int32))


def out_shape(name, rows, K):
    per = OUT_SPEC[name][1]
    if name in RESIDUE_OUTPUTS:
        return (rows, K) if per == 1 else (rows, K, per)
    return (rows,) if per == 0 else (rows, per)


# ------------------------------------------------------------------ the C ABI, operand by operand
class Operand:
    """`nbytes` of device memory at `offset` bytes behind a 256-byte boundary, between two guard bands."""

    def __init__(self, nbytes, offset=0, data=None, fill=FILL):
        self.nbytes, self.start = nbytes, GUARD + offset
        self.buf = torch.full((GUARD + offset + nbytes + GUARD,), fill, dtype=torch.uint8, device="cuda")
        assert self.buf.data_ptr() % 256 == 0
        if data is not None:
            self.buf[self.start:self.start + nbytes] = torch.from_numpy(np.frombuffer(np.ascontiguousarray(data).tobytes(), np.uint8).copy()).cuda()
        self.fill = fill

    @property
    def ptr(self):
        return ctypes.c_void_p(self.buf.data_ptr() + self.start)

    def guards_intact(self):
        host = self.buf.cpu().numpy()
        return bool((host[:self.start] == self.fill).all() and (host[self.start + self.nbytes:] == self.fill).all())

    def read(self, dtype, shape):
        return self.buf[self.start:self.start + self.nbytes].cpu().numpy().view(dtype).reshape(shape).copy()


def call_abi(case, misaligned=False, skip=(), workspace_fill=0x00, lib=None):
    """diffab_metrics_hbonds on the numpy inputs of `case`.  Every data operand sits between guard bands; with `misaligned`, 4 bytes
    (floats, integers) or 1 byte (masks) behind a 256-byte boundary.  Outputs named in `skip` are passed as NULL.  The workspace is
    exactly the documented size, filled with `workspace_fill`, between guard bands of its own.  Returns the outputs as numpy arrays."""
    lib = lib or _hip.lib()
    rows, K = case["points"].shape[:2]
    A, gs = case["ctx_points"].shape[2], case["group_size"]
    ops = []
    for name, dtype in INPUTS:
        v = case.get(name)
        if v is None:
            ops.append(None)
            continue
        v = np.ascontiguousarray(np.asarray(v).astype(dtype))
        ops.append(Operand(v.nbytes, (np.dtype(dtype).itemsize if misaligned else 0), v))
    outs = {}
    for name in OUTPUTS:
        if name in skip:
            continue
        dtype = OUT_SPEC[name][0]
        outs[name] = Operand(int(np.prod(out_shape(name, rows, K))) * np.dtype(dtype).itemsize, (np.dtype(dtype).itemsize if misaligned else 0))
    nbytes = metrics.hbonds_workspace_bytes(rows // gs, K, A)
    ws = Operand(nbytes, 0, fill=workspace_fill)
    null = ctypes.c_void_p(0)
    rc = lib.diffab_metrics_hbonds(*[null if o is None else o.ptr for o in ops], rows, gs, K, A,
                                   *[outs[n].ptr if n in outs else null for n in OUTPUTS], ws.ptr, nbytes, _hip.stream_ptr())
    assert rc == 0, lib.diffab_last_error().decode()
    torch.cuda.synchronize()
    for name, o in list(outs.items()) + [("workspace", ws)] + [(n, o) for (n, _), o in zip(INPUTS, ops) if o is not None]:
        assert o.guards_intact(), f"bytes around {name} were written"
    return {name: o.read(OUT_SPEC[name][0], out_shape(name, rows, K)) for name, o in outs.items()}


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def check(out, ref, what, names=OUTPUTS):
    for k in names:
        if k not in out:
            continue
        if not same_bits(out[k], ref[k]):
            bad = np.argwhere(out[k].view(np.uint8 if out[k].dtype.itemsize == 1 else np.uint32) != ref[k].view(np.uint8 if ref[k].dtype.itemsize == 1 else np.uint32))
            raise AssertionError(f"{what}: {k} differs at {len(bad)} places, first {bad[:4].tolist()}: got {out[k][tuple(bad[0])]!r}, oracle {ref[k][tuple(bad[0])]!r}")


# ------------------------------------------------------------------ patches and designs
def segment_chain(rng, n):
    """A NeRF chain of n residues whose phi, psi come in segments: alpha, 3-10, pi, strand, and anything."""
    kinds = [(-57.0, -47.0), (-49.0, -26.0), (-57.0, -70.0), (-120.0, 130.0), None]
    N, CA, C = backbone(1, 0, 0)[0]
    out, left, kind = [[N, CA, C]], 0, None
    for _ in range(n - 1):
        if left == 0:
            kind, left = kinds[rng.integers(len(kinds))], int(rng.integers(4, 10))
        phi, psi = (rng.uniform(-180, 180, 2) if kind is None else np.array(kind) + rng.normal(0, 6.0, 2))
        left -= 1
        N2 = place(N, CA, C, 1.329, 116.2, psi)
        CA2 = place(CA, C, N2, 1.458, 121.7, 180.0)
        C2 = place(C, N2, CA2, 1.525, 111.0, phi)
        N, CA, C = N2, CA2, C2
        out.append([N, CA, C])
    return np.array(out)


def cloud(rng, n):
    """n residues thrown into a ball at protein density: N-CA-C triangles of the right size, in no chain geometry at all."""
    radius = 3.0 * n ** (1.0 / 3.0)
    d = rng.normal(size=(n, 3))
    ca = d / np.linalg.norm(d, axis=1, keepdims=True) * radius * rng.random((n, 1)) ** (1.0 / 3.0)
    u = rng.normal(size=(n, 3))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    w = np.cross(u, rng.normal(size=(n, 3)))
    w /= np.linalg.norm(w, axis=1, keepdims=True)
    a = np.radians(111.0)
    return np.stack([ca + 1.458 * u, ca, ca + 1.525 * (np.cos(a) * u + np.sin(a) * w)], axis=1)


def moved(rng, pts, spread):
    R = rotation(rng.normal(size=3), rng.uniform(0, 2 * np.pi))
    return (pts.reshape(-1, 3) - pts[:, 1].mean(0)) @ R.T + rng.normal(0, spread, 3)


def ideal_oxygen(pts, nxt):
    """A real carbonyl O for a context residue: in the peptide plane where the next residue is known, else the frame's ideal one."""
    n, ca, c = pts
    if nxt is not None:
        b = (ca - c) / np.linalg.norm(ca - c) + (nxt - c) / np.linalg.norm(nxt - c)
        return c - 1.231 * b / np.linalg.norm(b)
    e1 = (c - ca) / np.linalg.norm(c - ca)
    v = n - ca
    e2 = v - (v @ e1) * e1
    return ca + 2.153 * e1 - 1.062 * e2 / np.linalg.norm(e2)


@functools.lru_cache(maxsize=None)
def case(kind, K, G, N, A, seed=0, context=True, antigen=True, hotspot=True, ragged=False, tangled=False):
    """G patches of K residues x N designs, as numpy inputs of the C ABI, with the oracle's outputs under 'ref'.

    kind 'helix': the 12-residue ideal helix first, 'strands': the 14 residues of the two-strand ladder first (two chains), then
    segment chains of up to 40 residues placed around them; 'cloud': K residues in a ball.  The generated residues are a stretch in the
    middle of the first chain (so both of its ends meet context residues) and, for 'strands', one whole strand end.  Design 0 of every
    patch is the native; the others add N(0, 0.25 A) to the atoms of the generated residues.  Context residues have their real O in two
    slots out of three, and about one residue in twelve outside the two hand cases is Pro.  ragged: a numbering gap, a residue outside residue_mask, a context residue without its CA, another with only
    its O missing, duplicate numbers in a chain.  tangled: the keys of test_geometry_host.tangle_chain_keys in the first chain of 14 or more
    residues behind the first and in the last slot - a 32-bit gap, the highest slot, a masked slot or another chain would link others."""
    rng = np.random.default_rng(1000 * K + 100 * G + 10 * N + seed)
    rows = G * N
    pts = np.zeros((G, K, 3, 3))
    chain, ridx = np.zeros((G, K), np.int32), np.zeros((G, K), np.int32)
    gen = np.zeros((G, K), bool)
    inside = np.ones((G, K), bool)
    for g in range(G):
        pieces = []
        if kind == "helix":
            pieces = [helix()]
        elif kind == "strands":
            two = strands()
            pieces = [two[:7], two[7:]]
        if kind == "cloud":
            pieces = [cloud(rng, K)]
        first = sum(len(p) for p in pieces)
        left = K - first
        while left > 0:
            n = min(left, int(rng.integers(12, 41)))
            if left - n < 4:
                n = left
            pieces.append(moved(rng, segment_chain(rng, n), 9.0).reshape(n, 3, 3) + (0.0 if first == 0 else np.array([14.0, 0.0, 0.0])))
            left -= n
        at = 0
        for c, piece in enumerate(pieces):
            n = len(piece)
            pts[g, at:at + n], chain[g, at:at + n], ridx[g, at:at + n] = piece, c, np.arange(n) + 5 * c
            at += n
        if tangled:
            c = next(c for c in range(1, len(pieces) - 1) if len(pieces[c]) >= 14)
            tangle_chain_keys(chain[g], ridx[g], inside[g], sum(len(p) for p in pieces[:c]) + g, K - 1)
        n0 = len(pieces[0])
        lo, hi = (2, 2 + max(1, n0 // 3)) if kind == "strands" else (n0 // 3, n0 // 3 + max(2, n0 // 3) - (kind == "helix"))
        gen[g, lo:hi] = True  # (the helix: 4, 5, 6, so that C=O of 3 - its O built from the design's N of 4 - meets N-H of the context's 7)
        if kind == "strands":
            gen[g, 11:14] = True  # the end of the second strand: a generated residue without a successor
        if len(pieces) > 2:
            start = sum(len(p) for p in pieces[:2])
            gen[g, start + 3:start + 3 + min(6, len(pieces[2]) - 4)] = True
        if g == 2:
            gen[g] = False  # a patch with nothing generated
    rm = inside if tangled else None
    if ragged:
        rm = inside
        for g in range(G):
            last = K - 1
            ridx[g, last - 6:] += 3  # a numbering gap inside the last chain
            rm[g, last - 3] = False
            if K >= 30:
                ridx[g, last - 10] = ridx[g, last - 9]  # two slots with one number: the lower one is the neighbour
    bits = np.zeros((G, K), np.int64)
    ctx = np.zeros((G, K, A, 3), f32)
    for g in range(G):
        for k in range(K):
            nxt = pts[g, k + 1, 0] if k + 1 < K and chain[g, k + 1] == chain[g, k] else None
            ctx[g, k, :3] = pts[g, k]
            ctx[g, k, 3] = ideal_oxygen(pts[g, k], nxt)
            ctx[g, k, 4:] = rng.normal(0, 3.0, (A - 4, 3)) + pts[g, k, 1]
            before_design = k + 1 < K and gen[g, k + 1] and not gen[g, k]  # (always without a real O: its O depends on the row)
            bits[g, k] = (7 | (8 if (k + g) % 3 and not before_design else 0) | (int(rng.integers(0, 1 << 28)) << 4)) & ((1 << A) - 1)
        if ragged:
            free = np.flatnonzero(~gen[g])
            bits[g, free[1]] &= ~2  # no CA: incomplete, between two complete neighbours
            bits[g, free[-2]] &= ~8
    if not context:  # what metrics.hbonds() builds without one: N, CA, C of the first row, no real O, four slots
        bits[:] = 7
    ag = hs = None
    if antigen:
        ag = rng.random((G, K)) < 0.5 if kind == "cloud" else (chain == chain.max(axis=1, keepdims=True)) | (chain == 1)
    if antigen and hotspot:
        hs = ag & (rng.random((G, K)) < 0.5)
    points = np.repeat(pts, N, axis=0)
    noise = rng.normal(0, 0.25, points.shape)
    noise[::N] = 0.0
    points = (points + noise * np.repeat(gen, N, axis=0)[:, :, None, None]).astype(f32)
    donor_off, ctx_donor_off = rng.random((rows, K)) < 0.08, rng.random((G, K)) < 0.08
    embedded = {"helix": 12, "strands": 14}.get(kind, 0)  # no Pro in the two hand cases: their bonds are known
    donor_off[:, :embedded], ctx_donor_off[:, :embedded] = False, False
    c = dict(points=points, donor_off=donor_off, ctx_points=ctx, ctx_valid=bits, ctx_donor_off=ctx_donor_off, gen=gen, chain=chain,
             ridx=ridx, rm=rm, antigen=ag, hotspot=hs, group_size=N)
    c["ref"] = hbonds_ref(**c)
    return c


def fair(c, what):
    """The exactness guard and the no-vacuous-pass guard of one case."""
    ref = c["ref"]
    assert ref["_margin"] > 1e-9 and not ref["_on_cull"], (what, ref["_margin"], ref["_on_cull"])
    G = c["gen"].shape[0]
    n = ref["n_hbonds"].reshape(G, -1)
    assert all(n[g].min() > 0 for g in range(G) if c["gen"][g].any()), (what, n.tolist())
    return ref


CASES = {  # kind, K, G, N, A, then keywords
    "K24 one chain": ("helix", 24, 1, 1, 4),
    "K70 ragged": ("helix", 70, 2, 3, 4, dict(ragged=True)),  # past 64 slots and no multiple of it; K300: past the 256 threads
    "K300": ("helix", 300, 2, 3, 4),
    "K40 three chains, ragged": ("strands", 40, 2, 5, 15, dict(ragged=True)),
    "K96 three patches": ("helix", 96, 3, 1, 32),
    "K96 cloud": ("cloud", 96, 1, 5, 4),
    "K130 65 designs": ("strands", 130, 1, 65, 15, dict(ragged=True)),
    "K130 two patches": ("helix", 130, 2, 5, 4, dict(antigen=False, hotspot=False)),
    "K512": ("strands", 512, 1, 1, 4),
    "K40 no hotspots": ("strands", 40, 2, 5, 32, dict(hotspot=False)),
    "K64": ("helix", 64, 3, 5, 15, dict(ragged=True)),
    "K257 tangled keys": ("helix", 257, 2, 2, 4, dict(tangled=True)),
}


def get(name):
    spec = CASES[name]
    return case(*spec[:5], **(spec[5] if len(spec) > 5 else {}))


@pytest.mark.parametrize("name", list(CASES))
def test_every_output_equals_the_oracle(name):
    c = get(name)
    ref = fair(c, name)
    out = call_abi(c)
    assert set(out) == set(OUTPUTS)
    check(out, ref, name)
    counts = np.bincount(ref["ss"].ravel(), minlength=8)
    print(name, "bonds", int(ref["_bonds"].sum()), "with a generated end", ref["n_hbonds"].tolist()[:8], "states", dict(zip(" HBEGITS", counts.tolist())))


def test_the_cases_together_reach_every_state_and_every_kind_of_bond():
    """What the shapes above are for: all eight states, both bridge types, second partners, bonds to antigen, framework and hotspots,
    donors whose H comes from a generated predecessor, and acceptors whose O comes from a generated successor."""
    seen, second, kinds = set(), 0, np.zeros(4, np.int64)
    parallel = boundary_h = boundary_o = 0
    for name in CASES:
        c = get(name)
        ref = c["ref"]
        seen |= set(np.unique(ref["ss"]).tolist())
        second += int((ref["nh_o_partner"][..., 1] >= 0).sum() + (ref["o_hn_partner"][..., 1] >= 0).sum() + (ref["bridge_partner"][..., 1] >= 0).sum())
        parallel += int(ref["bridge_parallel"].sum())
        kinds += [ref[k].sum() for k in ("n_hbonds_internal", "n_hbonds_antigen", "n_hbonds_framework", "n_hotspot_bonded")]
        N = c["group_size"]
        for r in range(len(ref["ss"])):
            g = r // N
            gen, real_o = c["gen"][g], (c["ctx_valid"][g] & 15) == 15
            succ, pred = links(c["chain"][g], c["ridx"][g], np.ones(len(gen), bool) if c["rm"] is None else c["rm"][g])
            for a, d in zip(*np.nonzero(ref["_bonds"][r])):
                boundary_h += (not gen[d]) and pred[d] >= 0 and gen[pred[d]] and not gen[a]
                boundary_o += (not gen[a]) and not real_o[a] and succ[a] >= 0 and gen[succ[a]] and not gen[d]
    print(sorted(seen), second, parallel, kinds.tolist(), boundary_h, boundary_o)
    assert seen == set(range(8)) and second > 0 and parallel > 0 and (kinds > 0).all()
    # a context residue behind / before a generated one takes its H / its O from the design: such bonds exist, between context residues
    assert boundary_h > 0 and boundary_o > 0


def test_the_helix_and_the_ladder_come_out_of_the_kernel():
    out = call_abi(get("K24 one chain"))
    assert metrics.ss_strings(torch.from_numpy(out["ss"][:, :12])) == [" HHHHHHHHHH "]
    assert out["o_hn_partner"][0, :8, 0].tolist() == list(range(4, 12)) and np.allclose(out["o_hn_energy"][0, :8, 0], -2.2563, atol=1e-3)
    c = get("K512")
    out = call_abi(c)
    assert metrics.ss_strings(torch.from_numpy(out["ss"][:, :14])) == ["  EEE    EEE  "]
    assert out["bridge_partner"][0, 3].tolist() == [10, -1] and out["bridge_parallel"][0, 3].tolist() == [0, 0]


# ------------------------------------------------------------------ rows do not depend on each other
def rows_of(c, rows):
    """The case cut down to some rows of ONE patch."""
    N = c["group_size"]
    g = rows[0] // N
    assert all(r // N == g for r in rows)
    sub = {k: (None if c[k] is None else c[k][g:g + 1]) for k in ("ctx_points", "ctx_valid", "ctx_donor_off", "gen", "chain", "ridx", "rm", "antigen", "hotspot")}
    sub.update(points=c["points"][rows], donor_off=c["donor_off"][rows], group_size=len(rows))
    return sub


@pytest.mark.parametrize("name", ["K40 three chains, ragged", "K130 65 designs"])
def test_a_row_alone_gives_what_it_gives_in_its_batch(name):
    c = get(name)
    whole = call_abi(c)
    N = c["group_size"]
    for r in (0, N - 1, len(c["points"]) - 2):
        alone = call_abi(rows_of(c, [r]))
        for k in OUTPUTS:
            assert same_bits(alone[k][0], whole[k][r]), (name, r, k)


def test_identical_designs_give_identical_rows():
    c = get("K64")
    N = c["group_size"]
    sub = rows_of(c, [N + 1] * 7)  # design 1 of patch 1, seven times
    out = call_abi(sub)
    assert int(out["n_hbonds"][0]) > 0
    for k in OUTPUTS:
        assert all(same_bits(out[k][0], out[k][r]) for r in range(1, 7)), k
        assert same_bits(out[k][0], c["ref"][k][N + 1]), k


def test_a_patch_with_nothing_generated_gives_zeros_and_the_context_states():
    c = get("K96 three patches")
    assert not c["gen"][2].any() and c["gen"][0].any()
    out, ref = call_abi(c), c["ref"]
    for k in ("n_hbonds", "n_hbonds_internal", "n_hbonds_antigen", "n_hbonds_framework", "n_hotspot_bonded", "hbond_energy"):
        assert out[k][2] == 0, k
    assert not out["ss_count"][2].any() and not out["residue_hbonds"][2].any()
    assert ref["_bonds"][2].any() and out["ss"][2].any() and same_bits(out["ss"][2], ref["ss"][2])  # the context has bonds and states of its own
    assert (out["o_hn_partner"][2] >= 0).any()


# ------------------------------------------------------------------ the contracts of the C ABI, held locally
@pytest.mark.parametrize("name", ["K40 three chains, ragged", "K130 65 designs", "K512"])
def test_what_the_workspace_held_is_ignored(name):
    c = get(name)
    a, b = call_abi(c, workspace_fill=0xFF), call_abi(c, workspace_fill=0x3C)
    for k in OUTPUTS:
        assert same_bits(a[k], b[k]), k
    check(a, c["ref"], name)


@pytest.mark.parametrize("name", ["K40 three chains, ragged", "K96 cloud", "K130 two patches"])
def test_operands_at_their_natural_alignment(name):
    """Every float / integer operand 4 bytes, every mask 1 byte behind a 256-byte boundary (the workspace keeps its own rule)."""
    c = get(name)
    check(call_abi(c, misaligned=True), c["ref"], name)


def test_null_outputs_are_skipped():
    c = get("K40 three chains, ragged")
    for keep in (("ss",), ("hbond_energy", "n_hbonds"), ("O", "bridge_partner", "ss_count"), ()):
        out = call_abi(c, skip=[k for k in OUTPUTS if k not in keep])
        assert set(out) == set(keep)
        check(out, c["ref"], str(keep))
    for leave in OUTPUTS:  # each one alone left out
        out = call_abi(c, skip=[leave])
        check(out, c["ref"], "without " + leave)


def test_an_empty_problem_returns_before_any_pointer_is_read(hip):
    null = ctypes.c_void_p(0)
    assert hip.diffab_metrics_hbonds(*[null] * 11, 0, 5, 128, 15, *[null] * 18, null, 0, _hip.stream_ptr()) == 0
    out = metrics.hbonds({"seq_idx": torch.zeros(0, 16, dtype=torch.long).cuda(), "translations": torch.zeros(0, 16, 3).cuda(),
                          "orientations": torch.zeros(0, 16, 3, 3).cuda()}, torch.zeros(0, 16, dtype=torch.bool).cuda(), group_size=4)
    assert out["ss"].shape == (0, 16) and out["ss_count"].shape == (0, 8)


# ------------------------------------------------------------------ metrics.hbonds
def frames_of(c, seed=3):
    """Designs as sample() returns them whose frame atoms are near the case's atoms: CA and an orthonormal frame from N, CA, C."""
    pts = c["points"].astype(f64)
    n, ca, cc = pts[:, :, 0], pts[:, :, 1], pts[:, :, 2]
    e1 = (cc - ca) / np.linalg.norm(cc - ca, axis=-1, keepdims=True)
    v = n - ca
    e2 = v - (v * e1).sum(-1, keepdims=True) * e1
    e2 /= np.linalg.norm(e2, axis=-1, keepdims=True)
    O = np.stack([e1, e2, np.cross(e1, e2)], axis=-2)  # rows are the local axes
    rng = np.random.default_rng(seed)
    seq = rng.integers(0, 20, pts.shape[:2])
    seq[rng.random(seq.shape) < 0.1] = metrics.PRO
    return {"seq_idx": torch.from_numpy(seq).cuda(), "translations": torch.from_numpy(ca.astype(f32)).cuda(), "orientations": torch.from_numpy(O.astype(f32)).cuda()}


@pytest.mark.parametrize("with_context, with_antigen, with_hotspot", [(True, True, True), (True, True, False), (True, False, False),
                                                                     (False, True, True), (False, False, False)])
def test_the_python_entry(with_context, with_antigen, with_hotspot):
    """metrics.hbonds against the oracle on the atoms the frame kernel gives: with and without context, antigen_mask and hotspot_mask."""
    c = get("K40 three chains, ragged")
    N, A = c["group_size"], c["ctx_points"].shape[2]
    des = frames_of(c)
    atoms = dio.backbone_from_frames(des["translations"], des["orientations"], ("N", "CA", "C")).cpu().numpy()
    pro = des["seq_idx"].cpu().numpy() == metrics.PRO
    cuda = lambda v: None if v is None else torch.from_numpy(np.ascontiguousarray(v)).cuda()
    kw = dict(chain_idx=cuda(c["chain"].astype(np.int64)), residue_idx=cuda(c["ridx"].astype(np.int64)), residue_mask=cuda(c["rm"]), group_size=N)
    oracle = dict(points=atoms, donor_off=pro, ctx_donor_off=pro[::N], gen=c["gen"], chain=c["chain"], ridx=c["ridx"], rm=c["rm"], group_size=N)
    if with_context:
        mask = (c["ctx_valid"][..., None] >> np.arange(A)) & 1
        kw["context"] = {"xyz": cuda(c["ctx_points"]), "atom_mask": cuda(mask.astype(bool))}
        oracle.update(ctx_points=c["ctx_points"], ctx_valid=c["ctx_valid"])
    else:
        first = np.zeros((len(c["gen"]), atoms.shape[1], 4, 3), f32)
        first[:, :, :3] = atoms[::N]
        oracle.update(ctx_points=first, ctx_valid=np.full(c["gen"].shape, 7, np.int64))
    if with_antigen:
        kw["antigen_mask"] = cuda(c["antigen"])
        oracle["antigen"] = c["antigen"]
    if with_hotspot:
        kw["hotspot_mask"] = cuda(c["hotspot"])
        oracle["hotspot"] = c["hotspot"]
    out = metrics.hbonds(des, cuda(c["gen"]), **kw)
    want = set(OUTPUTS) - (set() if with_antigen else {"n_hbonds_antigen"}) - (set() if with_hotspot else {"n_hotspot_bonded", "n_hotspot"})
    assert set(out) == want and all(v.is_cuda for v in out.values()) and out["bridge_parallel"].dtype == torch.bool
    ref = hbonds_ref(**oracle)
    assert ref["_margin"] > 1e-9 and not ref["_on_cull"] and ref["n_hbonds"].min() > 0
    got = {k: v.cpu().numpy() for k, v in out.items()}
    got["bridge_parallel"] = got["bridge_parallel"].astype(np.uint8)
    check(got, ref, f"python {with_context} {with_antigen} {with_hotspot}")
    to_host = lambda v: {k: to_host(x) for k, x in v.items()} if isinstance(v, dict) else (v.cpu() if isinstance(v, torch.Tensor) else v)
    host = metrics.hbonds(to_host(des), torch.from_numpy(c["gen"]), **to_host(kw))  # host tensors in, host tensors out, the same numbers
    assert all(not v.is_cuda and np.array_equal(v.numpy(), out[k].cpu().numpy(), equal_nan=True) for k, v in host.items())
