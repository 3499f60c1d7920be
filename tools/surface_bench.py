#!/usr/bin/env python3
"""Cost of the surface filter (diffab_pytorch.metrics.surface) on synthetic designs: tools/geometry_bench.py's designs and context
(synthetic.py patches, N Gaussian perturbations of each, one generated segment of --counted residues per patch, A context atoms per
residue under a ragged atom_mask, the far half of the other residues flagged as the antigen), S sphere points per atom.

Two shapes: G x N designs of K residues (16 x 1024 x 128 by default) and the sampler's 256 x 128 batch (256 patches, one design each).
The whole Python call is timed beside a chunked torch broadcast formulation of the SAME rule on the same device - sphere points
fl(c + fl(R u)), d2 = (dx*dx + dy*dy) + dz*dz against every other atom, strict comparison with R_b^2 - the two ALTERNATING in one
process, after a warm-up, with device events around the call after a device synchronise.  The torch form has a part per patch (the
antigen's points against the context) and a part per row (the generated atoms' points against the row and the context, the antigen's
open points against the row); each is timed on --torch-patches patches / --torch-rows rows and scaled to all of them, and the result
says so.  It returns point totals per row only (no per-residue outputs, no areas); the rows where they differ from the kernel's are
counted.
--step-ms takes bench.py's ms_per_step of the same session (256 x 128 batch) and adds every call's ratio to one sampler step; without
it the ratio is reported as not measured.  --hip-only runs nothing but the kernel calls (for a kernel trace taken in a run of its own).
Prints one JSON document (--json OUT) and writes the table of profiles/surface.md (--md OUT).

    python tools/surface_bench.py [--g 16 --n 1024 --k 128 --a 15 --s 96 --counted 20 --repeats 10 --warmup 2 --step-ms MS] [--json OUT] [--md OUT]
"""
import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "diffab-pytorch_amd"))
sys.path.insert(0, os.path.join(REPO, "tools"))

import torch  # noqa: E402

from geometry_bench import ATOMS, GLY, alternate, context_of  # noqa: E402
from metrics_bench import designs_of  # noqa: E402
from sampler_bench_common import stats_ms, timed  # noqa: E402


def covered(q, atoms, R2, skip_self=False):
    """q (..., n, S, 3) points of n atoms, atoms (..., m, 3) with squared radii R2 (..., m) (-1: no atom) -> (..., n, S) bool."""
    dx, dy, dz = (q[..., :, :, None, x] - atoms[..., None, None, :, x] for x in range(3))
    hit = ((dx * dx + dy * dy) + dz * dz) < R2[..., None, None, :]
    if skip_self:
        n = q.shape[-3]
        hit = hit & ~torch.eye(n, dtype=torch.bool, device=q.device)[:, None, :]
    return hit.any(-1)


class TorchSurface:
    """The rule in torch: the context of every patch split into antigen and framework once (host-side bookkeeping, not timed)."""

    def __init__(self, designs, gm, ctx, antigen, N, S, probe=1.4, context_radius=1.8):
        from diffab_pytorch import metrics

        self.designs, self.gm, self.N, self.S = designs, gm, N, S
        self.table = metrics.sphere_points(S).cuda()
        self.radii = torch.tensor([metrics.ATOM_RADIUS[a] for a in ATOMS], device="cuda") + probe
        G, K = gm.shape
        A = ctx["xyz"].shape[2]
        self.n = int(gm[0].sum())
        self.idx = gm.nonzero()[:, 1].view(G, self.n)
        there = ctx["atom_mask"] & ~gm[..., None]
        R = torch.tensor(context_radius, device="cuda") + probe
        self.xyz = ctx["xyz"].reshape(G, K * A, 3)
        self.R2_antigen = torch.where((there & antigen[..., None]).reshape(G, K * A), R * R, -1.0)
        self.R2_framework = torch.where((there & ~antigen[..., None]).reshape(G, K * A), R * R, -1.0)
        self.R = R
        self.open = None

    def patches(self, lo, hi, chunk=256):
        """Per patch: the antigen points no antigen atom covers, and of those the ones no framework atom covers.  (G', KA, S) bool."""
        free, opened = [], []
        for g in range(lo, hi):
            mine = (self.R2_antigen[g] >= 0).nonzero()[:, 0]
            f = torch.zeros(self.xyz.shape[1], self.S, dtype=torch.bool, device="cuda")
            o = torch.zeros_like(f)
            for c in range(0, len(mine), chunk):
                at = mine[c:c + chunk]
                q = self.xyz[g, at, None, :] + self.R * self.table[None]
                R2 = self.R2_antigen[g].repeat(len(at), 1)
                R2[torch.arange(len(at)), at] = -1.0  # an atom does not cover its own points
                dx, dy, dz = (q[:, :, None, x] - self.xyz[g, None, None, :, x] for x in range(3))
                d2 = (dx * dx + dy * dy) + dz * dz
                alone = ~(d2 < R2[:, None, :]).any(-1)
                f[at] = alone
                o[at] = alone & ~(d2 < self.R2_framework[g][None, None, :]).any(-1)
            free.append(f)
            opened.append(o)
        return torch.stack(free), torch.stack(opened)

    def rows(self, lo, hi, opened, first_patch, chunk=8):
        """Per row: free and bound points of the generated atoms, design-buried points of the antigen.  3 x (rows',) int64."""
        from diffab_pytorch import io as dio

        out = []
        for r0 in range(lo, hi, chunk):
            r1 = min(hi, r0 + chunk)
            sub = {k: v[r0:r1] for k, v in self.designs.items()}
            n, rows = self.n, r1 - r0
            g_of = torch.arange(r0, r1, device="cuda") // self.N
            pick = self.idx[g_of]
            pts = dio.backbone_from_frames(sub["translations"], sub["orientations"], ATOMS)
            gp = pts.gather(1, pick[:, :, None, None].expand(rows, n, 5, 3)).reshape(rows, n * 5, 3)
            bits = torch.where(sub["seq_idx"] == GLY, 15, 31).gather(1, pick)
            gv = ((bits[:, :, None] >> torch.arange(5, device="cuda")) & 1).bool().reshape(rows, n * 5)
            R = self.radii.repeat(n)[None].expand(rows, n * 5)
            R2 = torch.where(gv, R * R, -1.0)
            q = gp[:, :, None, :] + R[:, :, None, None] * self.table[None, None]
            free = gv[:, :, None] & ~covered(q, gp, R2, skip_self=True) & ~covered(q, self.xyz[g_of], self.R2_framework[g_of])
            bound = free & ~covered(q, self.xyz[g_of], self.R2_antigen[g_of])
            op = opened[g_of - first_patch]  # (rows, KA, S)
            aq = self.xyz[g_of][:, :, None, :] + self.R * self.table[None, None]
            buried = op & covered(aq, gp, R2)
            out.append(torch.stack([free.sum((1, 2)), bound.sum((1, 2)), buried.sum((1, 2))]))
        return torch.cat(out, 1)


def main():
    ap = argparse.ArgumentParser()
    for name, default in (("g", 16), ("n", 1024), ("k", 128), ("a", 15), ("s", 96), ("counted", 20), ("repeats", 10), ("warmup", 2),
                          ("torch-rows", 32), ("torch-patches", 2)):
        ap.add_argument("--" + name, type=int, default=default)
    ap.add_argument("--step-ms", type=float)
    ap.add_argument("--hip-only", action="store_true")
    ap.add_argument("--json")
    ap.add_argument("--md")
    args = ap.parse_args()
    from diffab_pytorch import _hip, metrics

    _hip.lib()
    res = {"device": torch.cuda.get_device_name(0), "A": args.a, "S": args.s, "counted_residues": args.counted, "sampler_step_ms": args.step_ms,
           "cases": {}}
    for G, N in ((args.g, args.n), (256, 1)):
        K = args.k
        designs, native, gm = designs_of(G, N, K, args.counted, seed=1)
        ctx, antigen = context_of(native, gm, args.a, seed=2)
        rows = G * N
        name = f"G = {G}, N = {N}, K = {K}"
        hip = lambda: metrics.surface(designs, gm, context=ctx, antigen_mask=antigen, group_size=N, n_points=args.s)
        if args.hip_only:
            for _ in range(args.warmup + args.repeats):
                hip()
            torch.cuda.synchronize()
            continue
        tp = min(args.torch_patches, G)
        tr = min(args.torch_rows, tp * N)
        ref = TorchSurface(designs, gm, ctx, antigen, N, args.s)
        opened = ref.patches(0, tp)[1]
        t_hip, t_patch = alternate(hip, lambda: ref.patches(0, tp), args.warmup, args.repeats)
        t_rows = [timed(lambda: ref.rows(0, tr, opened, 0)) for _ in range(args.warmup + args.repeats)][args.warmup:]
        out = hip()
        want = ref.rows(0, tr, opened, 0)
        gen_rows = gm.repeat_interleave(N, 0)[:tr]
        got = torch.stack([(out["free_points"][:tr] * gen_rows).sum(1), (out["bound_points"][:tr] * gen_rows).sum(1),
                           out["design_buried_points"][:tr].sum(1)])
        n_ctx = int((ctx["atom_mask"] & ~gm[..., None]).sum())
        c = {"hip": stats_ms(t_hip), "torch_per_patch": dict(stats_ms(t_patch, G / tp), measured_on_patches=tp),
             "torch_per_row": dict(stats_ms(t_rows, rows / tr), measured_on_rows=tr), "context_atoms_per_patch": round(n_ctx / G, 1),
             "antigen_atoms_per_patch": round(float((ctx["atom_mask"] & ~gm[..., None] & antigen[..., None]).sum()) / G, 1)}
        c["torch_ms"] = round(c["torch_per_patch"]["median_ms"] + c["torch_per_row"]["median_ms"], 4)
        c["torch_over_hip"] = round(c["torch_ms"] / c["hip"]["median_ms"], 2)
        c["rows_where_torch_point_totals_differ"] = int((want != got).any(0).sum())
        c["hip_over_sampler_step"] = round(c["hip"]["median_ms"] / args.step_ms, 3) if args.step_ms else "not measured"
        c["mean_bsa_paratope_A2"] = round(float(out["bsa_paratope"].mean()), 2)
        res["cases"][name] = c
    if args.hip_only:
        return
    print(json.dumps(res, indent=1))
    if args.json:
        with open(args.json, "w") as f:
            json.dump(res, f, indent=1)
    if args.md:
        with open(args.md, "w") as f:
            f.write("| shape | HIP ms (median, min - max) | torch ms (per patch + per row, scaled) | torch / HIP | HIP / one sampler step"
                    + (f" ({args.step_ms:.3f} ms)" if args.step_ms else "") + " |\n|---|---|---|---|---|\n")
            for name, c in res["cases"].items():
                f.write(f"| {name} | {c['hip']['median_ms']} ({c['hip']['min_ms']} - {c['hip']['max_ms']}) | {c['torch_ms']} = "
                        f"{c['torch_per_patch']['median_ms']} (on {c['torch_per_patch']['measured_on_patches']} patches) + "
                        f"{c['torch_per_row']['median_ms']} (on {c['torch_per_row']['measured_on_rows']} rows) | {c['torch_over_hip']} | "
                        f"{c['hip_over_sampler_step']} |\n")
            f.write("\nRows where the torch form's point totals differ from the kernel's: "
                    + ", ".join(f"{c['rows_where_torch_point_totals_differ']} of {c['torch_per_row']['measured_on_rows']} ({name})"
                                for name, c in res["cases"].items()) + ".\n")


if __name__ == "__main__":
    main()
