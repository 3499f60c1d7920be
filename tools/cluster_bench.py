#!/usr/bin/env python3
"""Cost of the design clustering (diffab_pytorch.metrics.cluster) on synthetic distance matrices.

Three shapes, G patches x N designs: 16 x 1024, 256 x 64 and 4 x 4096.  At each, two matrices: PLANTED - Euclidean distances of N points
drawn around --families centres (uneven family sizes, random order), clustered at a cutoff of three spreads, which gives tens of
clusters - and WORST - the same matrix at a cutoff below every distance, so every design is a cluster of its own and the loop runs N
times.  The whole Python call is timed beside a torch formulation of the same rule on the same device (torch_cluster below: one batched
step per cluster over all patches - recount, arg-max on count * N + (N - 1 - index), mask out the members - whose loop ends when
`open.any()` read back on the host is false, one synchronisation per cluster).  The two ALTERNATE in one process after a warm-up, with
device events around the call after a device synchronise; the torch form gets --torch-repeats rounds.  Its labels are compared with
the kernel's.  metrics.pairwise on synthetic designs of the same G x N (K = --k residues, CA, in place) is timed for scale.
--hip-only --case NAME runs nothing but the kernel calls of one case (for a kernel trace taken in a run of its own: the two launches apart).
Prints one JSON document (--json OUT) and writes the table of profiles/cluster.md (--md OUT).

    python tools/cluster_bench.py [--families 32 --k 128 --repeats 10 --warmup 2 --torch-repeats 2] [--json OUT] [--md OUT]
"""
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "diffab-pytorch_amd"))
sys.path.insert(0, os.path.join(REPO, "tools"))

import torch  # noqa: E402

from sampler_bench_common import parser, stats_ms, timed  # noqa: E402

SHAPES = ((16, 1024), (256, 64), (4, 4096))
SPREAD, APART = 1.0, 12.0


def planted(G, N, families, seed):
    """(G,N,N) fp32 on the device: distances of N points around `families` centres per patch."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    centres = APART * torch.randn(G, families, 3, device="cuda", generator=g)
    p = torch.rand(G, families, device="cuda", generator=g) + 0.2
    which = torch.multinomial(p, N, replacement=True, generator=g)
    x = centres[torch.arange(G, device="cuda")[:, None], which] + SPREAD * torch.randn(G, N, 3, device="cuda", generator=g)
    d = x[:, :, None, :] - x[:, None, :, :]
    return d.square().sum(-1).sqrt().contiguous()


def torch_cluster(dist, cutoff):
    """The rule of metrics.cluster without score and candidates, batched over the patches: (label (G,N) int32, iterations)."""
    G, N, _ = dist.shape
    idx = torch.arange(N, device=dist.device)
    adj = (dist <= cutoff) | torch.eye(N, dtype=torch.bool, device=dist.device)
    open_ = torch.ones(G, N, dtype=torch.bool, device=dist.device)
    label = torch.full((G, N), -1, dtype=torch.int32, device=dist.device)
    made = torch.zeros(G, dtype=torch.int32, device=dist.device)
    it = 0
    while bool(open_.any()):  # one host synchronisation per cluster
        n = (adj & open_[:, None, :]).sum(-1)
        centre = torch.where(open_, n * N + (N - 1 - idx), -1).argmax(1)
        busy = open_.any(1)
        members = adj[torch.arange(G, device=dist.device), centre] & open_ & busy[:, None]
        label = torch.where(members, made[:, None], label)
        made += busy.int()
        open_ &= ~members
        it += 1
    return label, it


def designs_of(G, N, K, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    gm = torch.zeros(G, K, dtype=torch.bool, device="cuda")
    gm[:, K // 2:K // 2 + 20] = True
    return {"seq_idx": torch.randint(0, 20, (G * N, K), device="cuda", generator=g),
            "translations": 8.0 * torch.randn(G * N, K, 3, device="cuda", generator=g)}, gm


def main():
    ap = parser(steps=False)
    ap.set_defaults(repeats=10, warmup=2)
    ap.add_argument("--families", type=int, default=32)
    ap.add_argument("--torch-repeats", type=int, default=2)
    ap.add_argument("--hip-only", action="store_true")
    ap.add_argument("--case", help="with --hip-only: one of the case names, e.g. '16 x 1024, planted'")
    ap.add_argument("--md")
    args = ap.parse_args()
    from diffab_pytorch import _hip, metrics

    _hip.lib()
    res = {"device": torch.cuda.get_device_name(0), "families": args.families, "spread": SPREAD, "cases": {}, "pairwise": {}}
    for G, N in SHAPES:
        dist = planted(G, N, args.families, seed=G + N)
        below = float(dist[dist > 0].min()) * 0.5
        for kind, cutoff in (("planted", 3.0 * SPREAD), ("worst", below)):
            name = f"{G} x {N}, {kind}"
            hip = lambda: metrics.cluster(dist, cutoff)
            if args.hip_only:
                if name == args.case:
                    for _ in range(args.warmup + args.repeats):
                        hip()
                    torch.cuda.synchronize()
                continue
            for _ in range(args.warmup):
                hip()
            torch_cluster(dist, cutoff)
            t_hip, t_torch = [], []
            for r in range(args.repeats):
                t_hip.append(timed(hip))
                if r < args.torch_repeats:
                    t_torch.append(timed(lambda: torch_cluster(dist, cutoff)))
            out = hip()
            label, iterations = torch_cluster(dist, cutoff)
            c = {"cutoff": cutoff, "hip": stats_ms(t_hip), "torch": stats_ms(t_torch), "torch_loop_iterations": iterations,
                 "clusters_per_patch_min_max": [int(out["count"].min()), int(out["count"].max())], "largest_cluster": int(out["size"].max()),
                 "patches_where_torch_labels_differ": int((label != out["label"]).any(1).sum())}
            c["torch_over_hip"] = round(c["torch"]["median_ms"] / c["hip"]["median_ms"], 1)
            res["cases"][name] = c
        if not args.hip_only:
            d, gm = designs_of(G, N, args.k, seed=3)
            pw = lambda: metrics.pairwise(d, gm, group_size=N)
            for _ in range(args.warmup):
                pw()
            res["pairwise"][f"{G} x {N}"] = stats_ms([timed(pw) for _ in range(args.repeats)])
        del dist
    if args.hip_only:
        return
    print(json.dumps(res, indent=1))
    if args.json:
        with open(args.json, "w") as f:
            json.dump(res, f, indent=1)
    if args.md:
        with open(args.md, "w") as f:
            f.write("| shape, matrix | clusters per patch | HIP ms (median, min - max) | torch ms (median; loop iterations) | torch / HIP | "
                    f"pairwise ms, K = {args.k} |\n|---|---|---|---|---|---|\n")
            for name, c in res["cases"].items():
                lo, hi = c["clusters_per_patch_min_max"]
                f.write(f"| {name} | {lo} - {hi} | {c['hip']['median_ms']} ({c['hip']['min_ms']} - {c['hip']['max_ms']}) | "
                        f"{c['torch']['median_ms']} ({c['torch_loop_iterations']}) | {c['torch_over_hip']} | "
                        f"{res['pairwise'][name.split(',')[0]]['median_ms']} |\n")
            f.write("\nPatches where the torch form's labels differ from the kernel's: "
                    + ", ".join(f"{c['patches_where_torch_labels_differ']} ({name})" for name, c in res["cases"].items()) + ".\n")


if __name__ == "__main__":
    main()
