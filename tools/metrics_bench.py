#!/usr/bin/env python3
"""Cost of the design metrics (diffab_pytorch.metrics) on synthetic designs: synthetic.py patches, N Gaussian perturbations of each as the
designs (no model run), one generated segment of --counted residues per patch.

  pairwise   G = 16, N = 1024, K = 128, for (ca, backbone) x (in place, aligned): the metrics.pairwise call (packing + tile kernel, and
             the backbone through the frame kernel) beside a plain torch formulation on the same device - broadcast differences for the
             in-place number and the token compare, batched torch.linalg.svd of the 3 x 3 covariances for the aligned one.  The torch
             svd is run on --torch-groups of the G groups and scaled to G (it is slow); the result says so.
  evaluate   256 design rows of K = 128 (the sampler's batch) and all G * N rows against their natives, ca and backbone, six segments.
  select     select_diverse on one of the matrices, N = 1024, m = 32.

Each case is warmed up, then timed --repeats times with device events around the whole call after a device synchronise.  Prints one
JSON document (--json OUT) and writes the table of profiles/metrics.md (--md OUT).

    python tools/metrics_bench.py [--g 16 --n 1024 --k 128 --counted 20 --repeats 20 --warmup 3] [--json OUT] [--md OUT]
"""
import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "diffab-pytorch_amd"))

import torch  # noqa: E402

from sampler_bench_common import stats_ms, timed_repeats  # noqa: E402

HBM_PEAK = 8.0e12  # B/s, the figure the output-write floor is set against


def designs_of(G, N, K, counted, seed):
    from diffab_pytorch import synthetic as syn

    p = {k: v.cuda() for k, v in syn.patches(G, K, syn.BENCH_DIMS, seed=seed).items()}
    g = torch.Generator(device="cuda").manual_seed(seed)
    gm = torch.zeros(G, K, dtype=torch.bool, device="cuda")
    start = torch.randint(0, K - counted + 1, (G,), device="cuda", generator=g)
    gm[torch.arange(G, device="cuda")[:, None], start[:, None] + torch.arange(counted, device="cuda")] = True
    rep = lambda t: t.repeat_interleave(N, 0)
    x = rep(p["translations"]) + 1.5 * torch.randn(G * N, K, 3, device="cuda", generator=g)
    seq = torch.where(torch.rand(G * N, K, device="cuda", generator=g) < 0.5, rep(p["seq_idx"]),
                      torch.randint(0, 20, (G * N, K), device="cuda", generator=g))
    q, _ = torch.linalg.qr(torch.randn(G * N, K, 3, 3, device="cuda", generator=g))
    O = q * torch.sign(torch.linalg.det(q))[..., None, None]
    return {"seq_idx": seq, "translations": x, "orientations": O.contiguous()}, p, gm


def counted_points(designs, gm, N, atoms):
    from diffab_pytorch import metrics

    pts = metrics._points(designs, atoms)  # (rows, K, P, 3)
    G, K = gm.shape
    n = int(gm[0].sum())
    idx = gm.nonzero()[:, 1].view(G, n)
    pts = pts.view(G, N, K, -1, 3).gather(2, idx[:, None, :, None, None].expand(G, N, n, pts.shape[2], 3))
    seq = designs["seq_idx"].view(G, N, K).gather(2, idx[:, None, :].expand(G, N, n))
    return pts.reshape(G, N, -1, 3), seq


def torch_in_place(designs, gm, N, atoms, chunk=32):
    p, s = counted_points(designs, gm, N, atoms)
    G = p.shape[0]
    rmsd = torch.empty(G, N, N, device="cuda")
    ident = torch.empty(G, N, N, device="cuda")
    for i0 in range(0, N, chunk):
        d = p[:, i0:i0 + chunk, None] - p[:, None]
        rmsd[:, i0:i0 + chunk] = d.square().sum((-1, -2)).div(p.shape[2]).sqrt()
        ident[:, i0:i0 + chunk] = (s[:, i0:i0 + chunk, None] == s[:, None]).float().mean(-1)
    return rmsd, ident


def torch_aligned(designs, gm, N, atoms, groups, chunk=128):
    p, _ = counted_points(designs, gm, N, atoms)
    p = p[:groups].double()
    p = p - p.mean(2, keepdim=True)
    e = p.square().sum((-1, -2))
    rmsd = torch.empty(groups, N, N, device="cuda")
    for i0 in range(0, N, chunk):
        h = torch.einsum("gimx,gjmy->gijxy", p[:, i0:i0 + chunk], p)
        sv = torch.linalg.svdvals(h)
        sign = torch.where(torch.linalg.det(h) < 0, -1.0, 1.0)
        msd = (e[:, i0:i0 + chunk, None] + e[:, None] - 2 * (sv[..., 0] + sv[..., 1] + sign * sv[..., 2])).clamp_min(0) / p.shape[2]
        rmsd[:, i0:i0 + chunk] = msd.sqrt().float()
    return rmsd


def measure(fn, warmup, repeats, scale=1.0):
    for _ in range(warmup):
        fn()
    return stats_ms(timed_repeats(fn, repeats), scale)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--g", type=int, default=16)
    ap.add_argument("--n", type=int, default=1024)
    ap.add_argument("--k", type=int, default=128)
    ap.add_argument("--counted", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--torch-groups", type=int, default=1)
    ap.add_argument("--torch-repeats", type=int, default=3)
    ap.add_argument("--json")
    ap.add_argument("--md")
    args = ap.parse_args()
    from diffab_pytorch import _hip, metrics

    _hip.lib()
    G, N, K = args.g, args.n, args.k
    designs, native, gm = designs_of(G, N, K, args.counted, seed=1)
    floor_ms = G * N * N * 8 / HBM_PEAK * 1e3
    res = {"device": torch.cuda.get_device_name(0), "G": G, "N": N, "K": K, "counted_residues": args.counted,
           "output_write_floor_ms": round(floor_ms, 4), "pairwise": {}, "evaluate": {}, "select_diverse": {}}
    tg = min(args.torch_groups, G)
    out = None
    for atoms in ("ca", "backbone"):
        for aligned in (False, True):
            name = f"{atoms}, {'aligned' if aligned else 'in place'}"
            hip = measure(lambda: metrics.pairwise(designs, gm, group_size=N, atoms=atoms, aligned=aligned), args.warmup, args.repeats)
            out = metrics.pairwise(designs, gm, group_size=N, atoms=atoms, aligned=aligned)
            if aligned:
                th = measure(lambda: torch_aligned(designs, gm, N, atoms, tg), 1, args.torch_repeats, scale=G / tg)
                th["measured_on_groups"] = tg
                diff = float((torch_aligned(designs, gm, N, atoms, tg) - out["rmsd"][:tg]).abs().max())
            else:
                th = measure(lambda: torch_in_place(designs, gm, N, atoms), 1, args.torch_repeats)
                diff = float((torch_in_place(designs, gm, N, atoms)[0] - out["rmsd"]).abs().max())
            res["pairwise"][name] = {"hip": hip, "torch": th, "torch_over_hip": round(th["median_ms"] / hip["median_ms"], 2),
                                     "pairs_per_s": round(G * N * N / (hip["median_ms"] * 1e-3), 0),
                                     "share_of_output_write_floor": round(floor_ms / hip["median_ms"], 4),
                                     "max_abs_difference_to_torch_A": diff}
    nat = {k: native[k] for k in ("seq_idx", "translations", "orientations")}
    seg = torch.where(gm, torch.arange(K, device="cuda")[None] % 6, -1)
    for n_rows in (256, G * N):  # the sampler's batch (256 x 128), and every design of the pairwise case
        rows = {k: v[:n_rows] for k, v in designs.items()}
        group = min(n_rows, N)
        Gr = n_rows // group
        for atoms in ("ca", "backbone"):
            fn = lambda: metrics.evaluate(rows, {k: v[:Gr] for k, v in nat.items()}, gm[:Gr], segment_idx=seg[:Gr], num_segments=6,
                                          group_size=group, atoms=atoms)
            res["evaluate"][f"{n_rows} rows x K = {K}, {atoms}, 6 segments"] = measure(fn, args.warmup, args.repeats)
    dist = out["rmsd"]
    res["select_diverse"][f"G = {G}, N = {N}, m = 32"] = measure(lambda: metrics.select_diverse(dist, 32), args.warmup, args.repeats)
    print(json.dumps(res, indent=1))
    if args.json:
        with open(args.json, "w") as f:
            json.dump(res, f, indent=1)
    if args.md:
        with open(args.md, "w") as f:
            f.write(f"| pairwise, G = {G}, N = {N}, K = {K}, {args.counted} counted residues | HIP ms (median) | pairs/s | share of the "
                    f"output-write floor ({floor_ms:.4f} ms) | torch ms | torch / HIP | max difference to torch, A |\n|---|---|---|---|---|---|---|\n")
            for name, r in res["pairwise"].items():
                note = f" (on {r['torch']['measured_on_groups']} of {G} groups, scaled)" if "measured_on_groups" in r["torch"] else ""
                f.write(f"| {name} | {r['hip']['median_ms']} | {r['pairs_per_s']:.3g} | {r['share_of_output_write_floor']} | "
                        f"{r['torch']['median_ms']}{note} | {r['torch_over_hip']} | {r['max_abs_difference_to_torch_A']:.2g} |\n")
            f.write("\n| call | ms (median) | min | max |\n|---|---|---|---|\n")
            for kind in ("evaluate", "select_diverse"):
                for name, r in res[kind].items():
                    f.write(f"| {kind}: {name} | {r['median_ms']} | {r['min_ms']} | {r['max_ms']} |\n")


if __name__ == "__main__":
    main()
