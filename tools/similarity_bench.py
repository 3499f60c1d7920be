#!/usr/bin/env python3
"""Cost of metrics.similarity on synthetic designs: tools/metrics_bench.py's designs - synthetic.py patches as the
natives, N Gaussian perturbations of each (no model run), one generated segment of --counted residues per patch.

  similarity   G = 16, N = 1024, K = 128, for ca and backbone, without an antigen_mask (every output but the interface ones).  Each case
               beside a chunked torch broadcast formulation on the same device and the same points: the native distances of the counted
               points to all points once per patch, the designs' distances --chunk designs at a time, boolean masks and sums, fp32.

Each case is warmed up, then timed --repeats times with device events around the whole Python call after a device synchronise; the two
forms alternate in one process.  --step-ms takes bench.py's ms_per_step of the same session (256 x 128 batch) and adds the call's ratio to
one sampler step; without it the ratio is left out.  Prints one JSON document (--json OUT) and writes the table of profiles/similarity.md
(--md OUT).

    python tools/similarity_bench.py [--g 16 --n 1024 --k 128 --counted 20 --repeats 20 --warmup 3 --chunk 64] [--step-ms MS] [--json OUT] [--md OUT]
"""
import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "diffab-pytorch_amd"))

import torch  # noqa: E402

from metrics_bench import designs_of  # noqa: E402
from sampler_bench_common import rounds, stats_ms, timed  # noqa: E402

TAU = (0.5, 1.0, 2.0, 4.0)


def torch_similarity(designs, native, gm, N, atoms, radius, cutoff, chunk):
    """The broadcast formulation of lddt, lddt_residue, n_native, n_kept, n_design and fnat (no masks but generation_mask; the partners
    are the residues with |i - j| > 1), `chunk` designs of every patch at a time."""
    from diffab_pytorch import metrics

    pts, npts = metrics._points(designs, atoms), metrics._points(native, atoms)
    rows, K, P = pts.shape[:3]
    G = rows // N
    n = int(gm[0].sum())
    idx = gm.nonzero()[:, 1].view(G, n)
    pts = pts.view(G, N, K, P, 3)
    own = lambda t, lead: t.gather(lead, idx.view(G, *[1] * (lead - 1), n, 1, 1).expand(*t.shape[:lead], n, P, 3))
    dist = lambda a, b: (a[..., :, :, None, None, :] - b[..., None, None, :, :, :]).square().sum(-1).sqrt()  # (...,n,P,K,P)
    dn = dist(own(npts, 1), npts)
    sep = (torch.arange(K, device=pts.device)[None, None] - idx[:, :, None]).abs()  # (G,n,K)
    scored = (dn < radius) & (sep > 0)[:, :, None, :, None]
    partner = sep > 1
    near_n = (dn < cutoff).any(4).any(2) & partner
    n_pairs = scored.sum((2, 3, 4))  # (G,n)
    n_native = near_n.sum((1, 2))
    lddt, lddt_res, kept, made = [], [], [], []
    for r0 in range(0, N, chunk):
        p = pts[:, r0:r0 + chunk]
        dd = dist(own(p, 2), p)  # (G,c,n,P,K,P)
        off = (dd - dn[:, None]).abs()
        pres = sum((scored[:, None] & (off < t)).sum((3, 4, 5)) for t in TAU)  # (G,c,n)
        near_d = (dd < cutoff).any(5).any(3) & partner[:, None]
        lddt_res.append(pres / (4 * n_pairs[:, None]))
        lddt.append(pres.sum(2) / (4 * n_pairs.sum(1))[:, None])
        kept.append((near_d & near_n[:, None]).sum((2, 3)))
        made.append(near_d.sum((2, 3)))
    n_kept = torch.cat(kept, 1).reshape(rows)
    return {"lddt": torch.cat(lddt, 1).reshape(rows), "lddt_residue_counted": torch.cat(lddt_res, 1).reshape(rows, n), "n_native": n_native,
            "n_kept": n_kept, "n_design": torch.cat(made, 1).reshape(rows), "fnat": n_kept / n_native.repeat_interleave(N)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--g", type=int, default=16)
    ap.add_argument("--n", type=int, default=1024)
    ap.add_argument("--k", type=int, default=128)
    ap.add_argument("--counted", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--chunk", type=int, default=64, help="designs per patch the torch form takes at a time")
    ap.add_argument("--step-ms", type=float, help="bench.py's ms_per_step of the same session")
    ap.add_argument("--json")
    ap.add_argument("--md")
    args = ap.parse_args()
    from diffab_pytorch import _hip, metrics

    _hip.lib()
    G, N, K = args.g, args.n, args.k
    designs, native, gm = designs_of(G, N, K, args.counted, seed=1)
    res = {"device": torch.cuda.get_device_name(0), "counted_residues": args.counted, "torch_chunk": args.chunk, "step_ms": args.step_ms,
           "similarity": {}}
    for atoms in ("ca", "backbone"):
        radius, cutoff = 15.0, metrics.CONTACT_DISTANCE[atoms]
        fns = {"hip": lambda: metrics.similarity(designs, native, gm, group_size=N, atoms=atoms),
               "torch": lambda: torch_similarity(designs, native, gm, N, atoms, radius, cutoff, args.chunk)}
        for fn in fns.values():
            for _ in range(args.warmup):
                fn()
        runs = {k: [] for k in fns}
        for _, k in rounds(list(fns), args.repeats):
            runs[k].append(timed(fns[k]))
        hip, th = stats_ms(runs["hip"]), stats_ms(runs["torch"])
        out, ref = fns["hip"](), fns["torch"]()
        P = 1 if atoms == "ca" else 4
        pairs = int(out["n_pairs"].sum()) * N
        r = {"hip": hip, "torch": th, "torch_over_hip": round(th["median_ms"] / hip["median_ms"], 2), "scored_pairs": pairs,
             "point_pairs_examined": G * N * args.counted * P * (K - 1) * P,
             "max_abs_lddt_difference_to_torch": float((out["lddt"] - ref["lddt"]).abs().nan_to_num(0.0).max()),
             "rows_with_other_contact_counts": int(((out["n_kept"] != ref["n_kept"]) | (out["n_design"] != ref["n_design"])).sum()),
             "mean_lddt": float(out["lddt"].mean()), "mean_fnat": float(out["fnat"].nanmean())}
        if args.step_ms:
            r["hip_over_sampler_step"] = round(hip["median_ms"] / args.step_ms, 3)
        res["similarity"][f"G = {G}, N = {N}, K = {K}, {atoms}"] = r
    print(json.dumps(res, indent=1))
    if args.json:
        with open(args.json, "w") as f:
            json.dump(res, f, indent=1)
    if args.md:
        with open(args.md, "w") as f:
            f.write(f"| similarity, {args.counted} counted residues | HIP ms (median) | min | max | torch ms (median, {args.chunk} designs a chunk) "
                    "| torch / HIP | HIP / one sampler step | point pairs examined | max lddt difference to torch | rows with other contact counts |\n"
                    "|---|---|---|---|---|---|---|---|---|---|\n")
            for name, r in res["similarity"].items():
                f.write(f"| {name} | {r['hip']['median_ms']} | {r['hip']['min_ms']} | {r['hip']['max_ms']} | {r['torch']['median_ms']} | "
                        f"{r['torch_over_hip']} | {r.get('hip_over_sampler_step', 'not measured')} | {r['point_pairs_examined']:.3g} | "
                        f"{r['max_abs_lddt_difference_to_torch']:.2g} | {r['rows_with_other_contact_counts']} |\n")


if __name__ == "__main__":
    main()
