#!/usr/bin/env python3
"""Cost of metrics.ensemble on synthetic designs: tools/metrics_bench.py's designs - synthetic.py patches, N Gaussian
perturbations of each (no model run), one generated segment of --counted residues per patch.

  ensemble   G = 16, N = 1024, K = 128, for (ca, backbone) x (unweighted, weighted: a softmax over the designs of each patch), and one
             batch of 256 rows x K = 128 as 16 patches of N = 16 (ca, unweighted).  Each case beside a plain torch formulation on the
             same device and the same points: one_hot sums for the frequencies, weighted means, broadcast deviations, fp32 throughout.

Each case is warmed up, then timed --repeats times with device events around the whole call after a device synchronise; the two forms
alternate in one process.  The bytes the call must read are the tokens and the points of every design once (8 + 12 P bytes per design
residue; the kernels stream them twice); their rate is given as a share of the 8 TB/s the other profiles use.  Prints one JSON document
(--json OUT) and writes the table of profiles/ensemble.md (--md OUT).

    python tools/ensemble_bench.py [--g 16 --n 1024 --k 128 --counted 20 --repeats 20 --warmup 3] [--json OUT] [--md OUT]
"""
import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "diffab-pytorch_amd"))

import torch  # noqa: E402

from metrics_bench import HBM_PEAK, designs_of  # noqa: E402
from sampler_bench_common import rounds, stats_ms, timed  # noqa: E402


def torch_ensemble(designs, gm, N, atoms, weights, V=21):
    """The plain formulation: every output of metrics.ensemble (no residue_mask, no pseudocount), fp32."""
    from diffab_pytorch import metrics

    pts = metrics._points(designs, atoms)
    rows, K, P = pts.shape[:3]
    G = rows // N
    pts, seq = pts.view(G, N, K, P, 3), designs["seq_idx"].view(G, N, K)
    w = torch.ones(G, N, device=pts.device) if weights is None else weights.view(G, N).float()
    W = w.sum(1)
    c = (torch.nn.functional.one_hot(seq, V) * w[:, :, None, None]).sum(1)  # (G,K,V)
    f = c / c.sum(-1, keepdim=True)
    entropy = -torch.xlogy(f, f).sum(-1)
    consensus = c.argmax(-1)
    mean = (pts * w[:, :, None, None, None]).sum(1) / W[:, None, None, None]
    d2 = (pts - mean[:, None]).square().sum((-1, -2))  # (G,N,K)
    rmsf = ((d2 * w[:, :, None]).sum(1) / (W[:, None] * P)).sqrt()
    n = gm.sum(1).float()[:, None]
    lnf = torch.gather(f.log()[:, None].expand(G, N, K, V), 3, seq[..., None]).squeeze(-1)
    log_prob = torch.where(gm[:, None], lnf, torch.zeros_like(lnf)).sum(-1) / n
    identity = ((seq == consensus[:, None]) & gm[:, None]).sum(-1) / n
    rmsd = ((d2 * gm[:, None]).sum(-1) / (n * P)).sqrt()
    central = torch.where(w > 0, rmsd, torch.full_like(rmsd, float("inf"))).argmin(1)
    return {"aa_freq": f, "entropy": entropy, "consensus": consensus, "mean_points": mean, "rmsf": rmsf, "log_prob": log_prob.reshape(rows),
            "consensus_identity": identity.reshape(rows), "rmsd_to_mean": rmsd.reshape(rows), "n_eff": W * W / (w * w).sum(1), "central": central}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--g", type=int, default=16)
    ap.add_argument("--n", type=int, default=1024)
    ap.add_argument("--k", type=int, default=128)
    ap.add_argument("--counted", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--json")
    ap.add_argument("--md")
    args = ap.parse_args()
    from diffab_pytorch import _hip, metrics

    _hip.lib()
    G, N, K = args.g, args.n, args.k
    designs, _, gm = designs_of(G, N, K, args.counted, seed=1)
    g = torch.Generator(device="cuda").manual_seed(2)
    weights = torch.softmax(2.0 * torch.randn(G, N, device="cuda", generator=g), 1)
    small_n = 16
    small = {k: v[:16 * small_n].contiguous() for k, v in designs.items()}
    cases = [(f"G = {G}, N = {N}, K = {K}, {atoms}, {'weighted' if w is not None else 'unweighted'}", designs, gm, N, atoms, w)
             for atoms in ("ca", "backbone") for w in (None, weights)]
    cases.append((f"256 rows x K = {K} as G = 16, N = {small_n}, ca, unweighted", small, gm[:16], small_n, "ca", None))
    res = {"device": torch.cuda.get_device_name(0), "counted_residues": args.counted, "hbm_peak_bytes_per_s": HBM_PEAK, "ensemble": {}}
    for name, des, mask, n, atoms, w in cases:
        fns = {"hip": lambda: metrics.ensemble(des, mask, group_size=n, atoms=atoms, weights=w),
               "torch": lambda: torch_ensemble(des, mask, n, atoms, w)}
        for fn in fns.values():
            for _ in range(args.warmup):
                fn()
        runs = {k: [] for k in fns}
        for _, k in rounds(list(fns), args.repeats):
            runs[k].append(timed(fns[k]))
        hip, th = stats_ms(runs["hip"]), stats_ms(runs["torch"])
        out, ref = fns["hip"](), fns["torch"]()
        rows, P = des["seq_idx"].shape[0], 1 if atoms == "ca" else 4
        must_read = rows * K * (8 + 12 * P)
        res["ensemble"][name] = {
            "hip": hip, "torch": th, "torch_over_hip": round(th["median_ms"] / hip["median_ms"], 2), "must_read_bytes": must_read,
            "share_of_hbm_peak": round(must_read / (hip["median_ms"] * 1e-3) / HBM_PEAK, 4),
            "max_abs_difference_to_torch": {k: float((out[k].float() - ref[k].float()).abs().nan_to_num(0.0).max())
                                            for k in ("aa_freq", "entropy", "rmsf", "rmsd_to_mean", "log_prob")},
            "consensus_equal": bool(torch.equal(out["consensus"], ref["consensus"])),
            "central_equal": bool(torch.equal(out["central"], ref["central"]))}
    print(json.dumps(res, indent=1))
    if args.json:
        with open(args.json, "w") as f:
            json.dump(res, f, indent=1)
    if args.md:
        with open(args.md, "w") as f:
            f.write(f"| ensemble, {args.counted} counted residues | HIP ms (median) | min | max | must-read MB | share of 8 TB/s | torch ms | torch / HIP "
                    "| max difference to torch: rmsf, A | aa_freq |\n|---|---|---|---|---|---|---|---|---|---|\n")
            for name, r in res["ensemble"].items():
                d = r["max_abs_difference_to_torch"]
                f.write(f"| {name} | {r['hip']['median_ms']} | {r['hip']['min_ms']} | {r['hip']['max_ms']} | {r['must_read_bytes'] / 1e6:.1f} | "
                        f"{r['share_of_hbm_peak']} | {r['torch']['median_ms']} | {r['torch_over_hip']} | {d['rmsf']:.2g} | {d['aa_freq']:.2g} |\n")


if __name__ == "__main__":
    main()
