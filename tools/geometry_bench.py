#!/usr/bin/env python3
"""Cost of the design filters (diffab_pytorch.metrics.backbone / .contacts) on synthetic designs: tools/metrics_bench.py's designs
(synthetic.py patches, N Gaussian perturbations of each, one generated segment of --counted residues per patch) with a synthetic
all-atom context of A atoms per residue (ragged atom_mask) and the far half of the other residues flagged as the antigen.

Two shapes: G x N designs of K residues (16 x 1024 x 128 by default) and the sampler's 256 x 128 batch (256 patches, one design each).
Each whole Python call is timed beside a plain torch formulation of the same numbers on the same device - torch.cdist of the generated
atoms against the context atoms per design row with broadcast comparisons and an amax over the atom axes for the residue contacts;
dihedrals by torch.cross / atan2 over all residues - the two ALTERNATING in one process, after a warm-up, with device events around the
call after a device synchronise.  The torch form of contacts runs on --torch-rows rows and is scaled to all rows; the result says so.
It leaves out the pairs between generated residues, the chain-neighbour exclusion of the clash numbers and the per-residue outputs, so
it does less, and cdist's distances are not the defined fp32 number: the rows where its contact-pair count differs from the kernel's are
counted.
--step-ms takes bench.py's ms_per_step of the same session (256 x 128 batch) and adds every call's ratio to one sampler step; without
it the ratio is reported as not measured.  Prints one JSON document (--json OUT) and writes the table of profiles/geometry.md (--md OUT).

    python tools/geometry_bench.py [--g 16 --n 1024 --k 128 --a 15 --counted 20 --repeats 10 --warmup 2 --step-ms MS] [--json OUT] [--md OUT]
"""
import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "diffab-pytorch_amd"))
sys.path.insert(0, os.path.join(REPO, "tools"))

import torch  # noqa: E402

from metrics_bench import designs_of  # noqa: E402
from sampler_bench_common import stats_ms, timed  # noqa: E402

ATOMS = ("N", "CA", "C", "O", "CB")
GLY = 7  # index of GLY in io.AA3


def context_of(native, gm, A, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    G, K = gm.shape
    xyz = native["translations"][:, :, None] + 1.5 * torch.randn(G, K, A, 3, device="cuda", generator=g)
    am = torch.rand(G, K, A, device="cuda", generator=g) < 0.8
    am[:, :, :4] = True
    centre = (native["translations"] * gm[..., None]).sum(1, keepdim=True) / gm.sum(1)[:, None, None]
    dist = (native["translations"] - centre).norm(dim=-1).masked_fill(gm, -1.0)
    antigen = dist > dist.median(dim=1, keepdim=True).values
    return {"xyz": xyz.contiguous(), "atom_mask": am}, antigen


def torch_contacts(designs, gm, ctx, antigen, N, rows, clash=3.0, contact=5.0):
    from diffab_pytorch import io as dio

    G, K = gm.shape
    n = int(gm[0].sum())
    idx = gm.nonzero()[:, 1].view(G, n)
    sub = {k: v[:rows] for k, v in designs.items()}
    pts = dio.backbone_from_frames(sub["translations"], sub["orientations"], ATOMS)
    bits = torch.where(sub["seq_idx"] == GLY, 15, 31)  # no CB on Gly
    g_of = torch.arange(rows, device="cuda") // N
    pick = idx[g_of]  # (rows, n)
    gp = pts.gather(1, pick[:, :, None, None].expand(rows, n, 5, 3)).reshape(rows, n * 5, 3)
    gv = ((bits.gather(1, pick)[:, :, None] >> torch.arange(5, device="cuda")) & 1).bool().reshape(rows, n * 5)
    A = ctx["xyz"].shape[2]
    cv = (ctx["atom_mask"] & ~gm[..., None]).reshape(G, K * A)[g_of]
    # (rows, n*5, K*A) by plain torch.cdist, which at these sizes takes its matrix-product form.  Its difference form
    # (compute_mode="donot_use_mm_for_euclid_dist") is not used: called on 256 or 1024 of these rows at once it returned distances
    # that moved the contact-pair count of most rows (64 rows at a time it agreed), and it took two to six times as long.
    d = torch.cdist(gp, ctx["xyz"].reshape(G, K * A, 3)[g_of])
    d = d.masked_fill(~(gv[:, :, None] & cv[:, None, :]), float("inf"))
    n_clash = (d < clash).sum((1, 2))
    score = (clash - d).clamp_min(0).square().sum((1, 2))
    near = (d.view(rows, n, 5, K, A) < contact).any(4).any(2) & antigen[g_of][:, None, :]
    near &= (pick[:, :, None] - torch.arange(K, device="cuda")).abs() != 1  # chain neighbours (one chain, residue_idx = arange(K))
    return n_clash, score, d.amin((1, 2)), near.sum((1, 2)), near.any(2).sum(1), near.any(1).sum(1)


def torch_backbone(designs):
    from diffab_pytorch import io as dio

    p = dio.backbone_from_frames(designs["translations"], designs["orientations"], ("N", "CA", "C")).double()
    n, ca, c = p[:, :, 0], p[:, :, 1], p[:, :, 2]

    def dih(p0, p1, p2, p3):
        b1, b2, b3 = p1 - p0, p2 - p1, p3 - p2
        n1, n2 = torch.cross(b1, b2, dim=-1), torch.cross(b2, b3, dim=-1)
        return torch.atan2(b2.norm(dim=-1) * (b1 * n2).sum(-1), (n1 * n2).sum(-1)).float()

    return (dih(c[:, :-1], n[:, 1:], ca[:, 1:], c[:, 1:]), dih(n[:, :-1], ca[:, :-1], c[:, :-1], n[:, 1:]),
            dih(ca[:, :-1], c[:, :-1], n[:, 1:], ca[:, 1:]), (c[:, :-1] - n[:, 1:]).norm(dim=-1).float())


def alternate(hip, other, warmup, repeats):
    for _ in range(warmup):
        hip()
        other()
    runs = [(timed(hip), timed(other)) for _ in range(repeats)]
    return [r[0] for r in runs], [r[1] for r in runs]


def main():
    ap = argparse.ArgumentParser()
    for name, default in (("g", 16), ("n", 1024), ("k", 128), ("a", 15), ("counted", 20), ("repeats", 10), ("warmup", 2), ("torch-rows", 256)):
        ap.add_argument("--" + name, type=int, default=default)
    ap.add_argument("--step-ms", type=float)
    ap.add_argument("--json")
    ap.add_argument("--md")
    args = ap.parse_args()
    from diffab_pytorch import _hip, metrics

    _hip.lib()
    res = {"device": torch.cuda.get_device_name(0), "A": args.a, "counted_residues": args.counted, "sampler_step_ms": args.step_ms, "cases": {}}
    for G, N in ((args.g, args.n), (256, 1)):
        K = args.k
        designs, native, gm = designs_of(G, N, K, args.counted, seed=1)
        ctx, antigen = context_of(native, gm, args.a, seed=2)
        rows = G * N
        tr = min(args.torch_rows, rows) // N * N or N
        name = f"G = {G}, N = {N}, K = {K}"
        hip_c = lambda: metrics.contacts(designs, gm, context=ctx, antigen_mask=antigen, group_size=N)
        hip_b = lambda: metrics.backbone(designs, gm, group_size=N)
        c_hip, c_torch = alternate(hip_c, lambda: torch_contacts(designs, gm, ctx, antigen, N, tr), args.warmup, args.repeats)
        b_hip, b_torch = alternate(hip_b, lambda: torch_backbone(designs), args.warmup, args.repeats)
        out = hip_c()
        ref = torch_contacts(designs, gm, ctx, antigen, N, tr)
        pairs = float(args.counted * 5 * int((ctx["atom_mask"] & ~gm[..., None]).sum()) / G) * rows
        c = {"hip": stats_ms(c_hip), "torch": dict(stats_ms(c_torch, rows / tr), measured_on_rows=tr), "context_distances": pairs}
        c["torch_over_hip"] = round(c["torch"]["median_ms"] / c["hip"]["median_ms"], 2)
        c["context_distances_per_s"] = round(pairs / (c["hip"]["median_ms"] * 1e-3), 0)
        c["rows_where_torch_contact_pairs_differ"] = int((ref[3] != out["n_contact_pairs"][:tr]).sum())
        b = {"hip": stats_ms(b_hip), "torch": stats_ms(b_torch)}
        b["torch_over_hip"] = round(b["torch"]["median_ms"] / b["hip"]["median_ms"], 2)
        for r in (c, b):
            r["hip_over_sampler_step"] = round(r["hip"]["median_ms"] / args.step_ms, 3) if args.step_ms else "not measured"
        res["cases"][name] = {"contacts": c, "backbone": b}
    print(json.dumps(res, indent=1))
    if args.json:
        with open(args.json, "w") as f:
            json.dump(res, f, indent=1)
    if args.md:
        with open(args.md, "w") as f:
            f.write("| call | shape | HIP ms (median, min - max) | torch ms (median) | torch / HIP | HIP / one sampler step"
                    + (f" ({args.step_ms:.3f} ms)" if args.step_ms else "") + " |\n|---|---|---|---|---|---|\n")
            for name, case in res["cases"].items():
                for call in ("contacts", "backbone"):
                    r = case[call]
                    note = f" (on {r['torch']['measured_on_rows']} rows, scaled)" if "measured_on_rows" in r["torch"] else ""
                    f.write(f"| {call} | {name} | {r['hip']['median_ms']} ({r['hip']['min_ms']} - {r['hip']['max_ms']}) | "
                            f"{r['torch']['median_ms']}{note} | {r['torch_over_hip']} | {r['hip_over_sampler_step']} |\n")
            f.write("\nRows where the torch form's contact-pair count differs from the kernel's: "
                    + ", ".join(f"{case['contacts']['rows_where_torch_contact_pairs_differ']} of {case['contacts']['torch']['measured_on_rows']} ({name})"
                                for name, case in res["cases"].items()) + ".\n")


if __name__ == "__main__":
    main()
