#!/usr/bin/env python3
"""Cost of the backbone refinement (diffab_pytorch.refine.backbone) on synthetic designs: tools/metrics_bench.py's designs (synthetic.py
patches, N Gaussian perturbations of each with random frames, one generated segment of --counted residues per patch, one chain).

Two shapes: G x N designs of K residues (16 x 1024 x 128 by default) and the sampler's 256 x 128 batch (256 patches, one design each).
Each whole Python call (default options: 200 iterations) is timed beside a batched torch restatement of the same iteration on the same
device - the moving residues of all rows at once, the bonded terms by shifted slices (one chain, residue_idx = arange(K)), the clash
term as a (rows, moving, K) broadcast, Rodrigues and the re-placing of N and C as elementwise torch - the two ALTERNATING in one
process, after a warm-up, with device events around the call after a device synchronise; median of --repeats.  The torch form leaves
out the energies, max_shift and the final orthonormalisation, so it does less; its largest difference from the kernel's translations
after ONE iteration is reported (a check that the two do the same step).  --torch-rows R runs the torch form on the first R rows and
scales its time to all rows (0: all rows); the result says so.
Prints one JSON document (--json OUT) and writes the table of profiles/refine.md (--md OUT).

    python tools/refine_bench.py [--g 16 --n 1024 --k 128 --counted 20 --repeats 20 --warmup 2 --torch-rows 0] [--json OUT] [--md OUT]
"""
import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "diffab-pytorch_amd"))
sys.path.insert(0, os.path.join(REPO, "tools"))

import torch  # noqa: E402

from geometry_bench import alternate  # noqa: E402
from metrics_bench import designs_of  # noqa: E402
from sampler_bench_common import stats_ms  # noqa: E402

BOND, CA_N, C_CA, CA_CA, INERTIA = 1.329, 2.4260487261296753, 2.437145924677046, 3.8, 4.45
LOCAL_N, LOCAL_C = (-0.525, 1.363), 1.526


def torch_refine(designs, gm, rows, o):
    """The iteration of diffab_refine_backbone for one chain with residue_idx = arange(K), every residue inside the mask."""
    t, O = designs["translations"][:rows].clone(), designs["orientations"][:rows].clone()
    G, K = gm.shape
    N = designs["translations"].shape[0] // G
    mv = gm.repeat_interleave(N, 0)[:rows]  # (rows, K)
    n_mov = int(gm[0].sum())
    idx = mv.nonzero()[:, 1].view(rows, n_mov)  # the moving slots of every row
    pick3 = idx[:, :, None].expand(rows, n_mov, 3)
    start = t.clone()
    ar = torch.arange(K, device=t.device)
    partner = ((idx[:, :, None] - ar).abs() > 1)  # (rows, moving, K): neither the residue itself nor a chain neighbour
    zero = torch.zeros(rows, 1, 3, device=t.device)

    def place(t, O):
        return t + (LOCAL_N[0] * O[:, :, 0] + LOCAL_N[1] * O[:, :, 1]), t + LOCAL_C * O[:, :, 0]

    def force(a, b, d0, w):  # on a, (rows, K - 1, 3)
        r = a - b
        d = r.norm(dim=-1, keepdim=True)
        return torch.where(d < 1e-6, torch.zeros_like(r), (-2.0 * w) * (d - d0) / d * r)

    n, c = place(t, O)
    for _ in range(o.iterations):
        lo, hi = slice(0, K - 1), slice(1, K)  # the link i -> i + 1: i in lo, its successor in hi
        f_c = torch.cat([force(c[:, lo], n[:, hi], BOND, o.bond) + force(c[:, lo], t[:, hi], C_CA, o.angle), zero], 1)
        f_n = torch.cat([zero, force(n[:, hi], c[:, lo], BOND, o.bond) + force(n[:, hi], t[:, lo], CA_N, o.angle)], 1)
        f_ca = torch.cat([force(t[:, lo], n[:, hi], CA_N, o.angle) + force(t[:, lo], t[:, hi], CA_CA, o.trans), zero], 1) \
            + torch.cat([zero, force(t[:, hi], c[:, lo], C_CA, o.angle) + force(t[:, hi], t[:, lo], CA_CA, o.trans)], 1)
        r = t.gather(1, pick3)[:, :, None, :] - t[:, None, :, :]  # (rows, moving, K, 3)
        d = r.norm(dim=-1, keepdim=True)
        push = torch.where(partner[..., None] & (d < o.clash_distance) & (d >= 1e-6), (2.0 * o.clash) * (o.clash_distance - d) / d * r,
                           torch.zeros_like(r)).sum(2)
        f_ca = f_ca.scatter_add(1, pick3, push)
        if o.tether:
            f_ca = f_ca - 2.0 * o.tether * (t - start)
        F = f_n + f_ca + f_c
        w = (o.step / INERTIA) * (torch.cross(n - t, f_n, dim=-1) + torch.cross(c - t, f_c, dim=-1))
        m3 = mv[..., None]
        t = torch.where(m3, t + o.step * F, t)
        ang = w.norm(dim=-1)
        small = ang < 1e-6
        safe = ang.clamp_min(1e-6)
        a = torch.where(small, torch.ones_like(ang), safe.sin() / safe)[..., None, None]
        b = torch.where(small, torch.full_like(ang, 0.5), (1.0 - safe.cos()) / (safe * safe))[..., None, None]
        S = torch.zeros(rows, K, 3, 3, device=t.device)
        S[..., 0, 1], S[..., 0, 2], S[..., 1, 0] = -w[..., 2], w[..., 1], w[..., 2]
        S[..., 1, 2], S[..., 2, 0], S[..., 2, 1] = -w[..., 0], -w[..., 1], w[..., 0]
        E = torch.eye(3, device=t.device) + a * S + b * (S @ S)
        O = torch.where(m3[..., None], O @ E.transpose(-1, -2), O)
        n, c = place(t, O)
    return t, O


def main():
    ap = argparse.ArgumentParser()
    for name, default in (("g", 16), ("n", 1024), ("k", 128), ("counted", 20), ("repeats", 20), ("warmup", 2), ("torch-rows", 0)):
        ap.add_argument("--" + name, type=int, default=default)
    ap.add_argument("--json")
    ap.add_argument("--md")
    args = ap.parse_args()
    from diffab_pytorch import _hip, refine

    _hip.lib()
    o = refine.Refinement()
    res = {"device": torch.cuda.get_device_name(0), "counted_residues": args.counted, "iterations": o.iterations, "cases": {}}
    for G, N in ((args.g, args.n), (256, 1)):
        K = args.k
        designs, _, gm = designs_of(G, N, K, args.counted, seed=1)
        rows = G * N
        tr = rows if args.torch_rows <= 0 else (min(args.torch_rows, rows) // N * N or N)
        name = f"G = {G}, N = {N}, K = {K}"
        hip = lambda: refine.backbone(designs, gm, group_size=N, options=o)
        with torch.no_grad():
            t_hip, t_torch = alternate(hip, lambda: torch_refine(designs, gm, tr, o), args.warmup, args.repeats)
            once = refine.Refinement(iterations=1)  # (the synthetic frames are far from a chain: 200 steps amplify rounding, one does not)
            diff = float((refine.backbone(designs, gm, group_size=N, options=once)["translations"][:tr]
                          - torch_refine(designs, gm, tr, once)[0]).abs().max())
        r = {"hip": stats_ms(t_hip), "torch": dict(stats_ms(t_torch, rows / tr), measured_on_rows=tr), "max_abs_translation_difference": diff}
        r["torch_over_hip"] = round(r["torch"]["median_ms"] / r["hip"]["median_ms"], 2)
        r["residue_steps_per_s"] = round(rows * args.counted * o.iterations / (r["hip"]["median_ms"] * 1e-3), 0)
        res["cases"][name] = r
    print(json.dumps(res, indent=1))
    if args.json:
        with open(args.json, "w") as f:
            json.dump(res, f, indent=1)
    if args.md:
        with open(args.md, "w") as f:
            f.write(f"| shape | HIP ms (median of {args.repeats}, min - max) | torch ms (median) | torch / HIP | largest difference of the translations after one iteration (A) |\n"
                    "|---|---|---|---|---|\n")
            for name, r in res["cases"].items():
                note = f" (on {r['torch']['measured_on_rows']} rows, scaled)" if r["torch"]["measured_on_rows"] != int(name.split(",")[0].split("=")[1]) * \
                    int(name.split(",")[1].split("=")[1]) else ""
                f.write(f"| {name} | {r['hip']['median_ms']} ({r['hip']['min_ms']} - {r['hip']['max_ms']}) | {r['torch']['median_ms']}{note} | "
                        f"{r['torch_over_hip']} | {r['max_abs_translation_difference']:.3g} |\n")


if __name__ == "__main__":
    main()
