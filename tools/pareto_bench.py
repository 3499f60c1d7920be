#!/usr/bin/env python3
"""Cost of the Pareto ranking (diffab_pytorch.metrics.pareto) on synthetic objective tables.

Three shapes, G patches x N designs: 16 x 1024, 256 x 64 and 4 x 4096.  At each, three tables: M = 3 and M = 8 independent standard
normal objectives (all minimised, no violation, no score, no candidate mask, max_fronts = N), and WORST - M = 1 with distinct values, a
random permutation of 0..N-1 per patch, so every design is a front of its own and the loop runs N times.  The whole Python call is timed
beside a torch formulation of the same rule on the same device (torch_pareto below: the boolean dominance matrix by broadcast compares,
one objective at a time, then one batched step per front over all patches - recount the open dominators, take the open designs with
none - whose loop ends when `open.any()` read back on the host is false, one synchronisation per front).  The two ALTERNATE in one
process after a warm-up, with device events around the call after a device synchronise; the torch form gets --torch-repeats rounds.
EVERY run asserts that torch's ranks equal the kernel's.
--hip-only --case NAME runs nothing but the kernel calls of one case (for a kernel trace taken in a run of its own: the two launches apart).
Prints one JSON document (--json OUT) and writes the table of profiles/pareto.md (--md OUT).

    python tools/pareto_bench.py [--repeats 10 --warmup 2 --torch-repeats 2] [--json OUT] [--md OUT]
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
KINDS = (("M = 3", 3), ("M = 8", 8), ("worst, M = 1", 1))


def table(G, N, M, worst, seed):
    """(G,N,M) fp32 on the device."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    if worst:
        return torch.rand(G, N, device="cuda", generator=g).argsort(1).float().unsqueeze(-1).contiguous()
    return torch.randn(G, N, M, device="cuda", generator=g)


def torch_pareto(obj):
    """The rule of metrics.pareto for minimised objectives without NaNs, violation, score and candidates, batched over the patches:
    (rank (G,N) int32, iterations)."""
    G, N, M = obj.shape
    le = torch.ones(G, N, N, dtype=torch.bool, device=obj.device)
    lt = torch.zeros(G, N, N, dtype=torch.bool, device=obj.device)
    for m in range(M):  # (one objective at a time: the (G,N,N,M) broadcast would be M times the matrix)
        a = obj[:, :, m]
        le &= a[:, :, None] <= a[:, None, :]
        lt |= a[:, :, None] < a[:, None, :]
    dom = le & lt  # dom[g,i,j]: i dominates j
    open_ = torch.ones(G, N, dtype=torch.bool, device=obj.device)
    rank = torch.full((G, N), -1, dtype=torch.int32, device=obj.device)
    it = 0
    while bool(open_.any()):  # one host synchronisation per front
        n = (dom & open_[:, :, None]).sum(1)
        members = open_ & (n == 0)
        rank = torch.where(members, it, rank)
        open_ &= ~members
        it += 1
    return rank, it


def main():
    ap = parser(steps=False)
    ap.set_defaults(repeats=10, warmup=2)
    ap.add_argument("--torch-repeats", type=int, default=2)
    ap.add_argument("--hip-only", action="store_true")
    ap.add_argument("--case", help="with --hip-only: one of the case names, e.g. '16 x 1024, M = 3'")
    ap.add_argument("--md")
    args = ap.parse_args()
    from diffab_pytorch import _hip, metrics

    _hip.lib()
    res = {"device": torch.cuda.get_device_name(0), "cases": {}}
    for G, N in SHAPES:
        for kind, M in KINDS:
            name = f"{G} x {N}, {kind}"
            obj = table(G, N, M, kind.startswith("worst"), seed=G + N + M)
            hip = lambda: metrics.pareto(obj)
            if args.hip_only:
                if name == args.case:
                    for _ in range(args.warmup + args.repeats):
                        hip()
                    torch.cuda.synchronize()
                continue
            for _ in range(args.warmup):
                hip()
            torch_pareto(obj)
            t_hip, t_torch = [], []
            for r in range(args.repeats):
                t_hip.append(timed(hip))
                if r < args.torch_repeats:
                    t_torch.append(timed(lambda: torch_pareto(obj)))
            out = hip()
            rank, iterations = torch_pareto(obj)
            assert bool((rank == out["rank"]).all()), f"{name}: the torch form's ranks differ from the kernel's"
            c = {"hip": stats_ms(t_hip), "torch": stats_ms(t_torch), "torch_loop_iterations": iterations,
                 "fronts_per_patch_min_max": [int(out["count"].min()), int(out["count"].max())], "largest_front": int(out["front_size"].max())}
            c["torch_over_hip"] = round(c["torch"]["median_ms"] / c["hip"]["median_ms"], 1)
            res["cases"][name] = c
            del obj
    if args.hip_only:
        return
    print(json.dumps(res, indent=1))
    if args.json:
        with open(args.json, "w") as f:
            json.dump(res, f, indent=1)
    if args.md:
        with open(args.md, "w") as f:
            f.write("| shape, table | fronts per patch | largest front | HIP ms (median, min - max) | torch ms (median; loop iterations) | torch / HIP |\n"
                    "|---|---|---|---|---|---|\n")
            for name, c in res["cases"].items():
                lo, hi = c["fronts_per_patch_min_max"]
                f.write(f"| {name} | {lo} - {hi} | {c['largest_front']} | {c['hip']['median_ms']} ({c['hip']['min_ms']} - {c['hip']['max_ms']}) | "
                        f"{c['torch']['median_ms']} ({c['torch_loop_iterations']}) | {c['torch_over_hip']} |\n")
            f.write("\nThe torch form's ranks equal the kernel's in every patch of every case (asserted in every run).\n")


if __name__ == "__main__":
    main()
