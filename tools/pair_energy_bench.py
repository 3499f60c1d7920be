#!/usr/bin/env python3
"""Cost of the binding score (diffab_pytorch.metrics.interface_energy) on synthetic designs: tools/developability_bench.py's designs and
context (synthetic.py patches, N Gaussian perturbations of each, one generated segment of --counted residues per patch, an all-atom
context of A atoms per residue with a ragged atom_mask, the far half of the other residues flagged as the antigen), the default
potential (metrics.contact_potential(): 21 classes, two bins), one chain numbered by slot, min_separation = 3.

Three shapes, G patches x N designs of K = --k residues: 16 x 1024, the sampler's own 256 x 1, and 4 x 4096.  At each, the whole Python
call is timed with and without substitutions=True, each beside a torch formulation of the same rule on the same device, the two
ALTERNATING in one process after a warm-up, with device events around the call after a device synchronise; metrics.patches on the same
inputs is timed in the same run.  The torch form is a broadcast: the (rows, K, K) squared distances of a chunk of --torch-rows design
rows at once, the bin of every pair by bucketize, the terms gathered from the table, the class sums as masked float64 reductions (and
for the scan a (rows, K, K, V) gather); it runs on one chunk and is scaled to all rows.  Its distances are a sum over the last axis,
not the defined fp32 number: the rows whose n_pairs differ from the kernel's are counted, and the largest difference of e_antigen
relative to the sum of |term| is reported.
--step-ms takes bench.py's ms_per_step of the same session (256 x 128 batch) and adds every call's ratio to one sampler step; without
it the ratio is reported as not measured.  --hip-only runs nothing but the kernel calls, of every case or of --case NAME alone (for a
kernel trace taken in a run of its own).  Prints one JSON document (--json OUT) and writes the table of profiles/pair_energy.md (--md OUT).

    python tools/pair_energy_bench.py [--k 128 --a 15 --counted 20 --repeats 10 --warmup 2 --step-ms MS] [--json OUT] [--md OUT]
"""
import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "diffab-pytorch_amd"))
sys.path.insert(0, os.path.join(REPO, "tools"))

import torch  # noqa: E402

from developability_bench import SHAPES, alternate  # noqa: E402
from geometry_bench import GLY, context_of  # noqa: E402
from metrics_bench import designs_of  # noqa: E402
from sampler_bench_common import stats_ms, timed  # noqa: E402


def torch_energy(designs, gm, ctx, antigen, N, rows, table, edges, min_separation=3, substitutions=False):
    """metrics.interface_energy's rule on the first `rows` design rows as broadcasts over (rows, K, K)."""
    from diffab_pytorch import io as dio

    G, K = gm.shape
    NB, V = table.shape[:2]
    sub = {k: v[:rows] for k, v in designs.items()}
    frame = dio.backbone_from_frames(sub["translations"], sub["orientations"], ("CA", "CB"))
    seq = sub["seq_idx"]
    sites = torch.where((seq == GLY)[..., None], frame[:, :, 0], frame[:, :, 1])
    first = torch.arange(G, device="cuda") * N
    use_cb = ctx["atom_mask"][:, :, 4] & (designs["seq_idx"][first] != GLY)
    csites = torch.where(use_cb[..., None], ctx["xyz"][:, :, 4], ctx["xyz"][:, :, 1])
    present = ctx["atom_mask"][:, :, 1] | gm
    g_of = torch.arange(rows, device="cuda") // N
    pres, gen = present[g_of], (gm & present)[g_of]
    ag = (antigen & present & ~gm)[g_of]
    xyz = torch.where(gen[..., None], sites, csites[g_of])
    d2 = (xyz[:, :, None] - xyz[:, None]).square().sum(-1)
    e2 = torch.tensor(edges, device="cuda", dtype=torch.float32).square()
    bins = torch.bucketize(d2, e2, right=True) - 1  # e2[b] <= d2 < e2[b + 1]
    slot = torch.arange(K, device="cuda")
    known = (seq >= 0) & (seq < V)
    tok = seq.clamp(0, V - 1)
    geometric = (pres[:, :, None] & pres[:, None, :] & known[:, None, :] & (bins >= 0) & (bins < NB)
                 & ((slot[:, None] - slot[None, :]).abs() >= min_separation)[None])
    counted = geometric & known[:, :, None] & (gen[:, :, None] | gen[:, None, :])
    internal = counted & gen[:, :, None] & gen[:, None, :]
    to_ag = counted & ~internal & (ag[:, :, None] | ag[:, None, :])
    i_first = gen[:, :, None] & (~gen[:, None, :] | (slot[:, None] < slot[None, :])[None])
    ti, tj = tok[:, :, None].expand(rows, K, K), tok[:, None, :].expand(rows, K, K)
    b0 = bins.clamp(0, NB - 1)
    term = torch.where(counted, table[b0, torch.where(i_first, ti, tj), torch.where(i_first, tj, ti)].double(), 0.0)
    upper = (slot[:, None] < slot[None, :])[None]
    out = {"e_antigen": (term * (to_ag & upper)).sum((1, 2)).float(), "e_framework": (term * (counted & ~internal & ~to_ag & upper)).sum((1, 2)).float(),
           "e_internal": (term * (internal & upper)).sum((1, 2)).float(), "residue_energy": term.sum(2).float(),
           "residue_antigen_energy": (term * to_ag).sum(2).float(), "n_partners": counted.sum(2), "n_pairs_total": (counted & upper).sum((1, 2)),
           "sum_abs_antigen": (term.abs() * (to_ag & upper)).sum((1, 2))}
    if substitutions:
        partner = geometric & gen[:, :, None] & ag[:, None, :]  # (rows, K, K): j is a geometric antigen partner of generated i
        S = torch.zeros(rows, K, V, dtype=torch.float64, device="cuda")
        for b in range(NB):  # table[b][v][tok_j] summed over the partners in bin b
            S += torch.einsum("rij,rjv->riv", (partner & (bins == b)).double(), table[b].double().T[tok])
        cur = torch.where(known, S.gather(2, tok[..., None])[..., 0], 0.0)
        out["substitution"] = ((S - cur[..., None]) * gen[..., None]).float()
    return out


def main():
    ap = argparse.ArgumentParser()
    for name, default in (("k", 128), ("a", 15), ("counted", 20), ("repeats", 10), ("warmup", 2), ("torch-rows", 256)):
        ap.add_argument("--" + name, type=int, default=default)
    ap.add_argument("--step-ms", type=float)
    ap.add_argument("--hip-only", action="store_true")
    ap.add_argument("--case", help="with --hip-only: one of the case names, e.g. '16 x 1024' (default: every case, one after the other)")
    ap.add_argument("--json")
    ap.add_argument("--md")
    args = ap.parse_args()
    from diffab_pytorch import _hip, metrics

    _hip.lib()
    K = args.k
    potential = metrics.contact_potential()
    table = potential.table.cuda()
    ratio = lambda r: round(r["hip"]["median_ms"] / args.step_ms, 3) if args.step_ms else "not measured"
    res = {"device": torch.cuda.get_device_name(0), "K": K, "A": args.a, "counted_residues": args.counted, "sampler_step_ms": args.step_ms,
           "potential": "metrics.contact_potential()", "cases": {}}
    for G, N in SHAPES:
        name = f"{G} x {N}"
        if args.hip_only and args.case not in (None, name):
            continue
        designs, native, gm = designs_of(G, N, K, args.counted, seed=1)
        ctx, antigen = context_of(native, gm, args.a, seed=2)
        rows = G * N
        hip = {scan: (lambda scan=scan: metrics.interface_energy(designs, gm, context=ctx, antigen_mask=antigen, group_size=N, potential=potential,
                                                                  substitutions=scan)) for scan in (False, True)}
        hip_p = lambda: metrics.patches(designs, gm, context=ctx, antigen_mask=antigen, group_size=N)
        if args.hip_only:
            for _ in range(args.warmup + args.repeats):
                hip[False]()
                hip[True]()
                hip_p()
            torch.cuda.synchronize()
            continue
        tr = min(args.torch_rows, rows) // N * N or N
        case = {}
        for scan, label in ((False, "energies"), (True, "energies + scan")):
            form = lambda: torch_energy(designs, gm, ctx, antigen, N, tr, table, potential.bin_edges, substitutions=scan)
            t_hip, t_torch = alternate(hip[scan], form, args.warmup, args.repeats)
            got, ref = hip[scan](), form()
            r = {"hip": stats_ms(t_hip), "torch": dict(stats_ms(t_torch, rows / tr), measured_on_rows=tr),
                 "pairs_per_design_min_max": [int(got["n_pairs"].sum((1, 2)).min()), int(got["n_pairs"].sum((1, 2)).max())],
                 "rows_where_torch_counts_differ": int((ref["n_pairs_total"] != got["n_pairs"][:tr].sum((1, 2))).sum()),
                 "largest_e_antigen_difference_over_sum_abs": float(((ref["e_antigen"] - got["e_antigen"][:tr]).abs().double()
                                                                     / ref["sum_abs_antigen"].clamp_min(1e-30)).max())}
            if scan:
                r["largest_substitution_difference"] = float((ref["substitution"] - got["substitution"][:tr]).abs().max())
            r["torch_over_hip"] = round(r["torch"]["median_ms"] / r["hip"]["median_ms"], 2)
            r["hip_over_sampler_step"] = ratio(r)
            case[label] = r
            del got, ref
        p_ms = [timed(hip_p) for _ in range(args.warmup + args.repeats)][args.warmup:]
        case["patches"] = stats_ms(p_ms)
        for label in ("energies", "energies + scan"):
            case[label]["patches_over_hip"] = round(case["patches"]["median_ms"] / case[label]["hip"]["median_ms"], 2)
        res["cases"][name] = case
        del designs, ctx
        torch.cuda.empty_cache()
    if args.hip_only:
        return
    print(json.dumps(res, indent=1))
    if args.json:
        with open(args.json, "w") as f:
            json.dump(res, f, indent=1)
    if args.md:
        with open(args.md, "w") as f:
            f.write("| call | shape | HIP ms (median, min - max) | torch ms (median) | torch / HIP | patches ms (median) | patches / HIP | "
                    "HIP / one sampler step" + (f" ({args.step_ms:.3f} ms)" if args.step_ms else "") + " |\n|---|---|---|---|---|---|---|---|\n")
            for name, case in res["cases"].items():
                for call in ("energies", "energies + scan"):
                    r = case[call]
                    f.write(f"| {call} | {name} | {r['hip']['median_ms']} ({r['hip']['min_ms']} - {r['hip']['max_ms']}) | "
                            f"{r['torch']['median_ms']} (on {r['torch']['measured_on_rows']} rows, scaled) | {r['torch_over_hip']} | "
                            f"{case['patches']['median_ms']} | {r['patches_over_hip']} | {r['hip_over_sampler_step']} |\n")
            f.write("\nRows where the broadcast form's count of pairs differs from the kernel's: "
                    + ", ".join(f"{c['energies']['rows_where_torch_counts_differ']} of {c['energies']['torch']['measured_on_rows']} ({n})"
                                for n, c in res["cases"].items())
                    + "; largest difference of e_antigen relative to the sum of |term|: "
                    + ", ".join(f"{c['energies']['largest_e_antigen_difference_over_sum_abs']:.1e} ({n})" for n, c in res["cases"].items())
                    + "; largest difference of a substitution entry: "
                    + ", ".join(f"{c['energies + scan']['largest_substitution_difference']:.1e} ({n})" for n, c in res["cases"].items()) + ".\n")


if __name__ == "__main__":
    main()
