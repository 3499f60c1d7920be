"""CPU: the surface entry - the float32 oracle of diffab_metrics_surface and its hand cases, sphere_points,
the new header against the library and the ctypes table, host-side refusals through the C ABI, and every Python argument error before
any device work.

The oracle restates the rule of include/diffab_hip_analysis.h in numpy float32, brute force: every sphere point of every target atom
against every other atom, no neighbour lists and no culling.  tests/test_gpu_surface.py runs it on the fp32 atoms the kernels read."""
import ctypes
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

HEADER = os.path.join(REPO, "include", "diffab_hip_analysis.h")
INT_OUTPUTS = ("free_points", "bound_points", "design_buried_points", "n_paratope_buried", "n_epitope_buried", "n_hotspot", "n_hotspot_buried")
RESIDUE_AREAS = ("free_area", "bound_area", "design_buried_area", "residue_buried")
ROW_AREAS = ("bsa_paratope", "bsa_epitope", "bsa_design_epitope", "hotspot_buried_area")


# ------------------------------------------------------------------ the oracle
def covered(q, atoms, R2, own=None, chunk=48):
    """q (n,S,3) float32 sphere points of n target atoms; atoms (m,3) float32 with squared radii R2 (m,) float32; own (n,) the index of
    each target in `atoms` (or None) -> (n,S) bool: some atom other than the target's own has d2 < R2, d2 = (dx*dx + dy*dy) + dz*dz with
    every operation rounded to float32."""
    n, S = q.shape[:2]
    out = np.zeros((n, S), bool)
    if atoms.shape[0] == 0:
        return out
    for lo in range(0, n, chunk):
        part = q[lo:lo + chunk]
        dx, dy, dz = (part[:, :, None, x] - atoms[None, None, :, x] for x in range(3))
        hit = ((dx * dx + dy * dy) + dz * dz) < R2[None, None, :]
        if own is not None:
            idx = np.arange(part.shape[0])
            hit[idx, :, own[lo:lo + chunk]] = False
        out[lo:lo + chunk] = hit.any(-1)
    return out


def atoms_of(points, bits, radius, residues):
    """The valid atoms of the listed residues in residue and slot order: xyz (n,3) float32, radius (n,) float32, residue slot (n,)."""
    xyz, rad, owner = [], [], []
    for k in residues:
        for a in range(points.shape[1]):
            if (int(bits[k]) >> a) & 1:
                xyz.append(points[k, a])
                rad.append(radius[k, a])
                owner.append(k)
    return np.asarray(xyz, np.float32).reshape(-1, 3), np.asarray(rad, np.float32), np.asarray(owner, np.int64)


def sphere_of(xyz, R, table):
    """q = fl(c + fl(R * u)), component by component: (n,S,3) float32."""
    return xyz[:, None, :] + R[:, None, None] * table[None, :, :]


def per_residue(owner, count, R, S, K):
    """Counts and float64 areas per residue: sum over its atoms, ascending slot, of n_a * (4 pi R_a^2 / S) from the float32 R_a."""
    n, area = np.zeros(K, np.int64), np.zeros(K, np.float64)
    for k, c, r in zip(owner, count, R):
        r = float(r)
        n[k] += int(c)
        area[k] += float(c) * (4.0 * np.pi * r * r / float(S))
    return n, area


def surface_ref(points, valid, point_radius, ctx_points, ctx_valid, ctx_radius, gen, rm, sphere, antigen=None, hotspot=None, group_size=1,
                probe=1.4):
    """points (rows,K,P,3) fp32 with validity bits valid (rows,K) and radii point_radius (P,); ctx_points (G,K,A,3) fp32 with bits
    ctx_valid (G,K) and radii ctx_radius (G,K,A); gen, rm, antigen, hotspot (G,K); sphere (S,3) fp32.  -> every output of
    diffab_metrics_surface: the counts as int32, the areas as float64 (unrounded)."""
    rows, K, P = points.shape[:3]
    G, S = gen.shape[0], sphere.shape[0]
    sphere = np.asarray(sphere, np.float32)
    probe = np.float32(probe)
    antigen = np.zeros((G, K), bool) if antigen is None else np.asarray(antigen, bool)
    hotspot = np.zeros((G, K), bool) if hotspot is None else np.asarray(hotspot, bool)
    out = {k: np.zeros((rows, K), np.int32) for k in INT_OUTPUTS[:3]}
    out.update({k: np.zeros(rows, np.int32) for k in INT_OUTPUTS[3:]})
    out.update({k: np.zeros((rows, K)) for k in RESIDUE_AREAS})
    out.update({k: np.zeros(rows) for k in ROW_AREAS})
    prad = np.broadcast_to(np.asarray(point_radius, np.float32), (K, P))
    patch = {}
    for r in range(rows):
        g = r // group_size
        gen_res = np.flatnonzero(gen[g] & rm[g])
        if gen_res.size == 0:
            continue  # nothing to evaluate: zeros
        if g not in patch:
            # the antigen alone and in its patch: the same for every design of the patch
            cp, cr = np.asarray(ctx_points[g], np.float32), np.asarray(ctx_radius[g], np.float32)
            ag_res = np.flatnonzero(~gen[g] & rm[g] & antigen[g])
            fw_res = np.flatnonzero(~gen[g] & rm[g] & ~antigen[g])
            gx, gr, gown = atoms_of(cp, ctx_valid[g], cr, ag_res)
            fx, fr, _ = atoms_of(cp, ctx_valid[g], cr, fw_res)
            gR, fR = gr + probe, fr + probe
            gq = sphere_of(gx, gR, sphere)
            by_antigen = covered(gq, gx, gR * gR, np.arange(len(gx)))
            by_framework = covered(gq, fx, fR * fR)
            patch[g] = (gx, gR, gown, fx, fR, gq, ~by_antigen, ~by_antigen & ~by_framework)
        gx, gR, gown, fx, fR, gq, g_free, g_open = patch[g]
        dx, dr, down = atoms_of(np.asarray(points[r], np.float32), valid[r], prad, gen_res)
        dR = dr + probe
        dq = sphere_of(dx, dR, sphere)
        d_free = ~covered(dq, dx, dR * dR, np.arange(len(dx))) & ~covered(dq, fx, fR * fR)
        d_bound = d_free & ~covered(dq, gx, gR * gR)
        g_buried = g_open & covered(gq, dx, dR * dR)
        g_bound = g_open & ~g_buried
        n_free, a_free = per_residue(down, d_free.sum(1), dR, S, K)
        n_bound, a_bound = per_residue(down, d_bound.sum(1), dR, S, K)
        ag_free, aa_free = per_residue(gown, g_free.sum(1), gR, S, K)
        ag_bound, aa_bound = per_residue(gown, g_bound.sum(1), gR, S, K)
        ag_buried, aa_buried = per_residue(gown, g_buried.sum(1), gR, S, K)
        out["free_points"][r] = n_free + ag_free
        out["bound_points"][r] = n_bound + ag_bound
        out["design_buried_points"][r] = ag_buried
        out["free_area"][r] = a_free + aa_free
        out["bound_area"][r] = a_bound + aa_bound
        out["design_buried_area"][r] = aa_buried
        is_gen, is_ag = gen[g] & rm[g], ~gen[g] & rm[g] & antigen[g]
        out["residue_buried"][r] = np.where(is_gen, a_free - a_bound, aa_buried)
        hot = is_ag & hotspot[g]
        for k in range(K):  # float64 sums over k ascending
            if is_gen[k]:
                out["bsa_paratope"][r] += a_free[k] - a_bound[k]
            if is_ag[k]:
                out["bsa_epitope"][r] += aa_free[k] - aa_bound[k]
                out["bsa_design_epitope"][r] += aa_buried[k]
            if hot[k]:
                out["hotspot_buried_area"][r] += aa_buried[k]
        out["n_paratope_buried"][r] = int((is_gen & (n_free > n_bound)).sum())
        out["n_epitope_buried"][r] = int((is_ag & (ag_buried > 0)).sum())
        out["n_hotspot"][r] = int(hot.sum())
        out["n_hotspot_buried"][r] = int((hot & (ag_buried > 0)).sum())
    return out


def ulps32(got, want):
    """|got - want| in units of the fp32 spacing at want (got float32, want float64)."""
    want = np.asarray(want, np.float64)
    spacing = np.spacing(np.maximum(np.abs(want), np.finfo(np.float32).tiny).astype(np.float32)).astype(np.float64)
    return np.abs(np.asarray(got, np.float64) - want) / spacing


# ------------------------------------------------------------------ the oracle against geometry
R_CA = np.float32(1.87) + np.float32(1.4)


def spheres(centres, S=96, generated=None, antigen=None):
    """Residues of one CA atom each (radius 1.87, probe 1.4) at `centres`, one patch and one row."""
    c = np.asarray(centres, np.float32)
    K = len(c)
    gen = np.ones((1, K), bool) if generated is None else np.asarray(generated, bool)[None]
    table = metrics.sphere_points(S).numpy()
    return surface_ref(c[None, :, None, :], np.ones((1, K), np.int64), [1.87], c[None, :, None, :], np.ones((1, K), np.int64),
                       np.full((1, K, 1), 1.87, np.float32), gen, np.ones((1, K), bool), table,
                       antigen=None if antigen is None else np.asarray(antigen, bool)[None])


def test_an_isolated_atom_has_every_point_free():
    for S in (8, 33, 96, 256):
        out = spheres([[3.0, -2.0, 7.5]], S)
        assert out["free_points"][0, 0] == S and out["bound_points"][0, 0] == S
        assert out["free_area"][0, 0] == pytest.approx(4.0 * np.pi * float(R_CA) ** 2, rel=1e-12)


def test_two_equal_spheres_at_distance_R_keep_72_of_96_points():
    """A point of the sphere at the origin is covered by the one at (0, 0, R) iff z_k > 1/2 (|R u - R z|^2 < R^2 <=> 2 (1 - z) < 1), on
    the other sphere iff z_k < -1/2; z_k = 1 - (2k+1)/96 never comes within 0.01 of +-1/2, so float32 rounding cannot move a point
    across: 24 points are covered on each sphere, 72 stay."""
    z = 1.0 - (2 * np.arange(96) + 1) / 96.0
    assert np.abs(np.abs(z) - 0.5).min() > 0.01 and (z > 0.5).sum() == 24 and (z < -0.5).sum() == 24
    out = spheres([[0.0, 0.0, 0.0], [0.0, 0.0, float(R_CA)]])
    assert out["free_points"][0].tolist() == [72, 72] and out["bound_points"][0].tolist() == [72, 72]
    area = 72 * 4.0 * np.pi * float(R_CA) ** 2 / 96
    assert out["free_area"][0] == pytest.approx([area, area], rel=1e-12)
    assert out["bsa_paratope"][0] == 0.0 and out["n_paratope_buried"][0] == 0
    # the second sphere as the antigen: each is whole alone, 24 points of each are buried by the other
    out = spheres([[0.0, 0.0, 0.0], [0.0, 0.0, float(R_CA)]], generated=[True, False], antigen=[False, True])
    assert out["free_points"][0].tolist() == [96, 96] and out["bound_points"][0].tolist() == [72, 72]
    assert out["design_buried_points"][0].tolist() == [0, 24]
    assert out["bsa_paratope"][0] == pytest.approx(area / 3, rel=1e-12) and out["bsa_epitope"][0] == pytest.approx(area / 3, rel=1e-12)
    assert out["bsa_design_epitope"][0] == pytest.approx(area / 3, rel=1e-12) and out["residue_buried"][0] == pytest.approx([area / 3, area / 3], rel=1e-12)
    assert out["n_paratope_buried"][0] == 1 and out["n_epitope_buried"][0] == 1


def test_the_framework_only_occludes():
    """Three spheres in a row, generated - framework - antigen, R apart: the framework sphere takes 24 points of each neighbour's free
    surface and has no numbers of its own; nothing of the antigen is design-buried (the generated sphere is 2 R away: it touches no point)."""
    R = float(R_CA)
    out = spheres([[0.0, 0.0, 0.0], [0.0, 0.0, R], [0.0, 0.0, 2 * R]], generated=[True, False, False], antigen=[False, False, True])
    assert out["free_points"][0].tolist() == [72, 0, 96] and out["bound_points"][0].tolist() == [72, 0, 72]
    assert out["design_buried_points"][0].tolist() == [0, 0, 0] and out["bsa_paratope"][0] == 0.0 and out["bsa_design_epitope"][0] == 0.0
    assert out["bsa_epitope"][0] > 0.0 and out["n_epitope_buried"][0] == 0


# ------------------------------------------------------------------ sphere_points
@pytest.mark.parametrize("n", [8, 33, 96, 130, 256])
def test_sphere_points_are_the_golden_spiral(n):
    t = metrics.sphere_points(n)
    assert t.dtype == torch.float32 and tuple(t.shape) == (n, 3) and t.device.type == "cpu"
    u = t.numpy().astype(np.float64)
    assert np.abs(np.linalg.norm(u, axis=1) - 1.0).max() <= 1e-7
    k = np.arange(n, dtype=np.float64)
    z = 1.0 - (2.0 * k + 1.0) / n
    phi = k * np.pi * (3.0 - np.sqrt(5.0))
    want = np.stack([np.sqrt(1.0 - z * z) * np.cos(phi), np.sqrt(1.0 - z * z) * np.sin(phi), z], 1)
    assert np.abs(u - want).max() <= 2.0 ** -24  # half an fp32 ulp below 1: the float64 table rounded once
    assert np.array_equal(t.numpy()[:, 2], z.astype(np.float32))
    t[0, 0] = 5.0  # a copy: the next caller gets the table
    assert metrics.sphere_points(n)[0, 0] != 5.0


def test_sphere_points_argument_errors():
    for bad in (7, 257, 0, -96, 96.0, "96", True, None):
        with pytest.raises(ValueError, match="n must be an int in"):
            metrics.sphere_points(bad)


# ------------------------------------------------------------------ the header, the library and the ctypes table
def header_code():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


def test_header_library_and_symbol_table_agree():
    declared = sorted(set(re.findall(r"\b(diffab_[a-z0-9_]+)\s*\(", header_code())))
    assert declared == ["diffab_metrics_surface"]
    assert sorted(_hip.ANALYSIS_SYMBOLS) == declared, "ANALYSIS_SYMBOLS and include/diffab_hip_analysis.h drifted apart"
    assert not set(_hip.ANALYSIS_SYMBOLS) & set(_hip.SYMBOLS)
    raw = ctypes.CDLL(_hip.LIB_PATH)
    typed = _hip.load_library()
    for name in declared:
        assert hasattr(raw, name), f"{name} declared in include/diffab_hip_analysis.h but not exported by libdiffab_hip.so"
        res, args = _hip.ANALYSIS_SYMBOLS[name]
        fn = getattr(typed, name)
        assert fn.restype is res and list(fn.argtypes) == args  # load_library() types the second table onto the same CDLL object
    res, args = _hip.ANALYSIS_SYMBOLS["diffab_metrics_surface"]
    proto = re.search(r"\bint\s+diffab_metrics_surface\s*\((.*?)\)\s*;", header_code(), flags=re.S).group(1)
    params = [p.strip() for p in proto.split(",")]
    assert res is ctypes.c_int and len(args) == len(params) == 37
    for p, a in zip(params, args):
        kind = p.rsplit(" ", 1)[0]
        want = {"int32_t": ctypes.c_int32, "float": ctypes.c_float, "size_t": ctypes.c_size_t}.get(kind)
        if want is None:
            assert "*" in kind and a in (ctypes.c_void_p, ctypes.POINTER(ctypes.c_float)), p
        else:
            assert a is want, p
    assert '#include "diffab_hip.h"' in open(HEADER).read()
    macro = {k: int(v) for k, v in re.findall(r"#define\s+DIFFAB_METRICS_SURFACE_(MIN_POINTS|MAX_POINTS)\s+(\d+)", header_code())}
    assert macro == {"MIN_POINTS": metrics.SURFACE_MIN_POINTS, "MAX_POINTS": metrics.SURFACE_MAX_POINTS}


SHAPES = [(1, 1, 1, 8), (3, 70, 15, 96), (16, 128, 15, 96), (2, 90, 32, 130), (5, 24, 8, 33), (1, 4096, 32, 256), (256, 128, 15, 64),
          (7, 173, 14, 65)]
MACRO_C = r"""
#include <stdio.h>
#include "diffab_hip_analysis.h"
int main(void) {
%s
  printf("%%d %%d %%d\n", DIFFAB_ERR_ARG, DIFFAB_METRICS_MAX_K, DIFFAB_METRICS_SURFACE_MAX_POINTS);
  return 0;
}
"""


def test_workspace_macro_equals_the_python_mirror(tmp_path):
    """The header compiles as C on its own (it brings diffab_hip.h along) and its macro gives metrics.surface_workspace_bytes."""
    cc = shutil.which("cc") or shutil.which("gcc") or next((p for p in ("/opt/rocm/llvm/bin/clang",) if os.path.exists(p)), None)
    assert cc, "no C compiler to read the header's macro with"
    src, exe = tmp_path / "macro.c", tmp_path / "macro"
    lines = "\n".join(f'  printf("%zu\\n", DIFFAB_METRICS_SURFACE_WORKSPACE_BYTES({G}, {K}, {A}, {S}));' for G, K, A, S in SHAPES)
    src.write_text(MACRO_C % lines)
    subprocess.run([cc, "-I", os.path.join(REPO, "include"), str(src), "-o", str(exe)], check=True)
    got = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()
    assert [int(v) for v in got[:len(SHAPES)]] == [metrics.surface_workspace_bytes(*s) for s in SHAPES]
    assert got[len(SHAPES):] == ["-1", str(metrics.MAX_K), "256"]


def test_host_side_refusals_touch_no_gpu():
    """Every refusal is decided from the scalar arguments, the host radii and whether a pointer is null: the device pointers are fake
    addresses that are never dereferenced, nothing is enqueued (no GPU is needed), and diffab_last_error names the problem."""
    l = _hip.load_library()
    p, null = ctypes.c_void_p(4096), ctypes.c_void_p(0)

    def err():
        return l.diffab_last_error().decode()

    def call(rows=10, group=5, K=128, P=5, A=15, S=96, probe=1.4, default=1.8, radii=(1.65, 1.87, 1.76, 1.4, 1.87), pts=p, valid=p, ctx=p,
             cvalid=p, crad=null, gen=p, rm=null, ag=null, hs=null, table=p, outs=None, ws=p, ws_bytes=1 << 40):
        host = None if radii is None else (ctypes.c_float * len(radii))(*radii)
        outs = [p] * 15 if outs is None else outs
        return l.diffab_metrics_surface(pts, valid, host, ctx, cvalid, crad, gen, rm, ag, hs, table, rows, group, K, P, A, S, probe, default,
                                        *outs, ws, ws_bytes, null)

    nan, inf = float("nan"), float("inf")
    for kw, word in ((dict(rows=11), "not a multiple"), (dict(rows=-5), "extent"), (dict(group=0), "extent"), (dict(K=0), "extent"),
                     (dict(group=4097, rows=4097), "at most 4096 designs"), (dict(K=4097), "at most 4096"), (dict(P=0), "points per residue"),
                     (dict(P=6), "points per residue"), (dict(A=0), "context atoms per residue"), (dict(A=33), "context atoms per residue"),
                     (dict(S=7), "sphere points outside [8, 256]"), (dict(S=257), "sphere points outside [8, 256]"), (dict(S=0), "sphere points"),
                     (dict(S=-96), "sphere points"), (dict(probe=-0.1), "probe must be finite"), (dict(probe=nan), "probe must be finite"),
                     (dict(probe=inf), "probe must be finite"), (dict(default=-1.0), "context_radius_default"), (dict(default=nan), "context_radius_default"),
                     (dict(default=inf), "context_radius_default"), (dict(radii=(1.65, nan, 1.76, 1.4, 1.87)), "point_radius[1]"),
                     (dict(radii=(1.65, 1.87, 1.76, 1.4, inf)), "point_radius[4]"), (dict(radii=(-1.0, 1.87, 1.76, 1.4, 1.87)), "point_radius[0]"),
                     (dict(hs=p), "needs an antigen_mask"), (dict(pts=null), "null input"), (dict(valid=null), "null input"),
                     (dict(radii=None), "null input"), (dict(ctx=null), "null input"), (dict(cvalid=null), "null input"), (dict(gen=null), "null input"),
                     (dict(table=null), "null input"), (dict(ws=null), "workspace"), (dict(ws=ctypes.c_void_p(4096 + 16)), "256-byte aligned")):
        rc = call(**kw)
        assert rc == -1 and word in err() and err().startswith("metrics_surface:"), (kw, rc, err())
    need = metrics.surface_workspace_bytes(2, 128, 15, 96)
    assert call(ws_bytes=need // 2) == -4 and "needed" in err()  # DIFFAB_ERR_WORKSPACE
    assert need - 2048 <= int(re.search(r"(\d+) needed", err()).group(1)) <= need
    # the limits themselves pass every argument check (the call is stopped by the workspace size, still on the host); so do optional
    # operands, every output left out, and K * A as large as the two limits allow
    for kw in (dict(S=8), dict(S=256), dict(probe=0.0), dict(P=1, radii=(0.0,)), dict(crad=p, rm=p, ag=p, hs=p), dict(outs=[null] * 15),
               dict(K=4096, A=32, rows=4096, group=4096)):
        assert call(ws_bytes=16, **kw) == -4 and "needed" in err(), kw
    # an empty problem returns 0 before any pointer is looked at
    assert l.diffab_metrics_surface(*[null] * 2, None, *[null] * 8, 0, 5, 128, 5, 15, 96, 1.4, 1.8, *[null] * 15, null, 0, null) == 0


# ------------------------------------------------------------------ Python argument errors before any device work
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


def context(G=2, K=16, A=15, **more):
    return dict({"xyz": torch.zeros(G, K, A, 3), "atom_mask": torch.ones(G, K, A, dtype=torch.bool)}, **more)


def test_good_arguments_reach_the_library(no_library):
    with pytest.raises(ReachedTheLibrary):
        metrics.surface(frames(), mask(), group_size=3)
    with pytest.raises(ReachedTheLibrary):
        metrics.surface(frames(), mask(), group_size=3, context=context(atom_radius=torch.full((2, 16, 15), 1.7)), antigen_mask=~mask(),
                        hotspot_mask=~mask(), residue_mask=mask(), probe=0, n_points=8, atoms=("N", "CA", "C", "O"), atom_radius=(1.6, 1.9, 1.7, 1.4),
                        context_radius=2)
    with pytest.raises(ReachedTheLibrary):
        metrics.surface(frames(), mask(), group_size=3, n_points=256, atoms=("CA", "CB"), atom_radius={"CA": 2.0, "CB": 2.0, "N": 1.0})


@pytest.mark.parametrize("kw, match", [
    (dict(group_size=4), "6 design rows are not a multiple of group_size = 4"), (dict(group_size=0), "group_size must be"),
    (dict(group_size=True), "group_size must be"), (dict(generation_mask=mask().long()), "generation_mask must be a bool tensor"),
    (dict(generation_mask=mask(3)), "generation_mask is"), (dict(residue_mask=mask(2, 15)), "residue_mask is"),
    (dict(residue_mask=mask().float()), "residue_mask must be a bool tensor"),
    (dict(designs={"seq_idx": torch.zeros(6, 16, dtype=torch.long)}), "designs must be a dict"),
    (dict(designs=dict(frames(), seq_idx=torch.zeros(6, 16))), r"designs\['seq_idx'\] must be an integer tensor"),
    (dict(designs=dict(frames(), translations=torch.zeros(6, 15, 3))), r"designs\['translations'\] is"),
    (dict(designs={k: v for k, v in frames().items() if k != "orientations"}), r"designs\['orientations'\] must be"),
    (dict(probe=-0.1), "probe must be a finite number >= 0"), (dict(probe=float("nan")), "probe must be"), (dict(probe="1.4"), "probe must be"),
    (dict(probe=True), "probe must be"), (dict(context_radius=float("inf")), "context_radius must be"), (dict(context_radius=-1), "context_radius must be"),
    (dict(n_points=7), r"n_points must be an int in \[8, 256\]"), (dict(n_points=257), "n_points must be"), (dict(n_points=96.0), "n_points must be"),
    (dict(n_points=True), "n_points must be"), (dict(atoms="CA"), "atoms must be a sequence of distinct names"),
    (dict(atoms=("N", "CG")), "atoms must be a sequence"), (dict(atoms=()), "atoms must be a sequence"), (dict(atoms=("N", "N")), "atoms must be a sequence"),
    (dict(atom_radius=(1.0, 2.0)), "atom_radius must be a dict or a sequence of 5 numbers"), (dict(atom_radius=1.8), "atom_radius must be a dict or"),
    (dict(atom_radius="12345"), "atom_radius must be a dict or"), (dict(atom_radius={"N": 1.6}), "atom_radius must give a radius for every name"),
    (dict(atom_radius=(1.0, 2.0, -1.0, 1.0, 1.0)), "atom_radius of C must be a finite number >= 0"),
    (dict(atom_radius=dict(metrics.ATOM_RADIUS, O=float("nan"))), "atom_radius of O must be"),
    (dict(antigen_mask=mask().long()), "antigen_mask must be a bool tensor"), (dict(antigen_mask=mask(3)), "antigen_mask is"),
    (dict(hotspot_mask=mask()), "hotspot_mask needs an antigen_mask"), (dict(antigen_mask=mask(), hotspot_mask=mask(2, 15)), "hotspot_mask is"),
    (dict(context=torch.zeros(2, 16, 15, 3)), "context must be a dict with xyz"), (dict(context={"xyz": torch.zeros(2, 16, 15, 3)}), "context must be a dict"),
    (dict(context=context(3)), r"context\['xyz'\] is"), (dict(context=context(A=33)), "A = 33 atoms per residue"),
    (dict(context=dict(context(), atom_mask=torch.ones(2, 16, 14, dtype=torch.bool))), r"context\['atom_mask'\] is"),
    (dict(context=context(atom_radius=torch.ones(2, 16, 14))), r"context\['atom_radius'\] must be a float tensor"),
    (dict(context=context(atom_radius=torch.ones(2, 16, 15, dtype=torch.long))), r"context\['atom_radius'\] must be a float tensor"),
    (dict(context=context(atom_radius=[1.8])), r"context\['atom_radius'\] must be a float tensor"),
    (dict(context=context(atom_radius=torch.full((2, 16, 15), float("nan")))), r"context\['atom_radius'\] must be finite and >= 0"),
    (dict(context=context(atom_radius=torch.full((2, 16, 15), -1.0))), r"context\['atom_radius'\] must be finite and >= 0"),
])
def test_argument_errors(no_library, kw, match):
    args = dict(designs=frames(), generation_mask=mask(), group_size=3)
    args.update(kw)
    designs, gm = args.pop("designs"), args.pop("generation_mask")
    with pytest.raises(ValueError, match=match):
        metrics.surface(designs, gm, **args)


def test_defaults_and_mirrors():
    assert metrics.ATOM_RADIUS == {"N": 1.65, "CA": 1.87, "C": 1.76, "O": 1.40, "CB": 1.87}
    import inspect

    sig = inspect.signature(metrics.surface)
    assert [p for p in sig.parameters] == ["designs", "generation_mask", "context", "antigen_mask", "hotspot_mask", "residue_mask", "group_size",
                                          "probe", "n_points", "atoms", "atom_radius", "context_radius"]
    d = {k: v.default for k, v in sig.parameters.items()}
    assert (d["group_size"], d["probe"], d["n_points"], d["atom_radius"], d["context_radius"]) == (1, 1.4, 96, None, 1.8)
    assert d["atoms"] == ("N", "CA", "C", "O", "CB") and all(sig.parameters[k].kind is inspect.Parameter.KEYWORD_ONLY for k in list(d)[2:])
