#!/usr/bin/env python3
"""Cost of the developability calls (diffab_pytorch.metrics.patches / .liabilities) on synthetic designs: tools/geometry_bench.py's
designs and context (synthetic.py patches, N Gaussian perturbations of each, one generated segment of --counted residues per patch, an
all-atom context of A atoms per residue with a ragged atom_mask, the far half of the other residues flagged as the antigen).

Three shapes, G patches x N designs of K = --k residues: 16 x 1024, the sampler's own 256 x 1, and 4 x 4096.  At each, both whole Python
calls are timed beside a torch formulation of the same rules on the same device, the two ALTERNATING in one process after a warm-up,
with device events around the call after a device synchronise; metrics.contacts on the same inputs is timed in the same run:
  patches      against a broadcast form: the (rows, K, K) squared distances of a chunk of --torch-rows design rows at once, the counts,
               scope and exposure as masked reductions, the three pair sums in float64; it runs on one chunk and is scaled to all rows.
               Its distances are a sum over the last axis, not the defined fp32 number: the rows whose n_exposed or n_pairs differ from
               the kernel's are counted, and the largest relative difference of psh is reported;
  liabilities  against a gather form on all rows: succ from a (G, K, K) comparison, the tokens of the next one to three chain
               neighbours gathered, one shift-and-mask per motif position.  Its counts are compared with the kernel's.
--step-ms takes bench.py's ms_per_step of the same session (256 x 128 batch) and adds every call's ratio to one sampler step; without
it the ratio is reported as not measured.  --hip-only runs nothing but the kernel calls (and metrics.contacts), of every case or of
--case NAME alone (for a kernel trace taken in a run of its own).  Prints one JSON document (--json OUT) and writes the table of profiles/developability.md (--md OUT).

    python tools/developability_bench.py [--k 128 --a 15 --counted 20 --repeats 10 --warmup 2 --step-ms MS] [--json OUT] [--md OUT]
"""
import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "diffab-pytorch_amd"))
sys.path.insert(0, os.path.join(REPO, "tools"))

import torch  # noqa: E402

from geometry_bench import GLY, context_of  # noqa: E402
from metrics_bench import designs_of  # noqa: E402
from sampler_bench_common import stats_ms, timed  # noqa: E402

SHAPES = ((16, 1024), (256, 1), (4, 4096))


def torch_patches(designs, gm, ctx, antigen, N, rows, hyd, chg, near=10.0, max_neighbours=16, vicinity=10.0, patch=7.5, floor=3.8):
    """metrics.patches' rule on the first `rows` design rows as broadcasts over (rows, K, K)."""
    from diffab_pytorch import io as dio

    G, K = gm.shape
    sub = {k: v[:rows] for k, v in designs.items()}
    frame = dio.backbone_from_frames(sub["translations"], sub["orientations"], ("CA", "CB"))
    seq = sub["seq_idx"]
    sites = torch.where((seq == GLY)[..., None], frame[:, :, 0], frame[:, :, 1])
    first = torch.arange(G, device="cuda") * N
    use_cb = ctx["atom_mask"][:, :, 4] & (designs["seq_idx"][first] != GLY)
    csites = torch.where(use_cb[..., None], ctx["xyz"][:, :, 4], ctx["xyz"][:, :, 1])
    present = (ctx["atom_mask"][:, :, 1] | gm) & ~antigen
    g_of = torch.arange(rows, device="cuda") // N
    pres, gen = present[g_of], (gm & present)[g_of]
    xyz = torch.where(gen[..., None], sites, csites[g_of])
    d2 = (xyz[:, :, None] - xyz[:, None]).square().sum(-1)
    off = ~torch.eye(K, dtype=torch.bool, device="cuda")
    count = (pres[:, :, None] & pres[:, None, :] & off & (d2 < near * near)).sum(2)
    scope = pres & (gen | (pres[:, :, None] & gen[:, None, :] & (d2 < vicinity * vicinity)).any(2))
    exposed = scope & (count <= max_neighbours)
    pair = exposed[:, :, None] & exposed[:, None, :] & off & (d2 < patch * patch)
    inv = pair / d2.clamp_min(floor * floor).double()
    h, q = hyd[seq].double(), chg[seq].double()
    pos, neg = q.clamp_min(0), q.clamp_max(0)
    out = {"n_exposed": exposed.sum(1), "n_pairs": pair.sum((1, 2)) // 2, "n_neighbours": count}
    for name, w in (("psh", h), ("ppc", pos), ("pnc", neg)):
        per = (inv * w[:, :, None] * w[:, None, :]).sum(2)
        out["residue_" + name], out[name] = per.float(), (0.5 * per.sum(1)).float()
    out["charge_generated"], out["charge_scope"] = (q * gen).sum(1).float(), (q * scope).sum(1).float()
    return out


def torch_motifs(designs, gm, words, N):
    """metrics.liabilities' rule on all rows (one chain, residue_idx = arange(K), everything inside residue_mask) -> (rows, M) counts."""
    G, K = gm.shape
    tokens = designs["seq_idx"]
    rows = tokens.shape[0]
    ridx = torch.arange(K, device="cuda")
    match = ridx[None, :] == ridx[:, None] + 1  # (K, K): j follows i
    succ = torch.where(match.any(1), match.float().argmax(1), -1).expand(G, K)
    g_of = torch.arange(rows, device="cuda") // N
    counts = []
    for m in range(words.shape[0]):
        ok, touched = torch.ones(rows, K, dtype=torch.bool, device="cuda"), torch.zeros(rows, K, dtype=torch.bool, device="cuda")
        slot = torch.arange(K, device="cuda").expand(rows, K)
        for p in range(4):
            if int(words[m, p]) == 0:
                break
            w = torch.tensor(int(words[m, p]) & 0xFFFFFFFF, dtype=torch.int64, device="cuda")
            here = slot.clamp_min(0)
            tok = tokens.gather(1, here)
            ok &= (slot >= 0) & (tok >= 0) & (tok < 32) & (((w >> tok.clamp(0, 31)) & 1) != 0)
            touched |= gm[g_of].gather(1, here) & (slot >= 0)
            slot = torch.where(slot >= 0, succ[g_of].gather(1, here), slot)
        counts.append((ok & touched).sum(1))
    return torch.stack(counts, 1)


def alternate(hip, other, warmup, repeats):
    for _ in range(warmup):
        hip()
        other()
    runs = [(timed(hip), timed(other)) for _ in range(repeats)]
    return [r[0] for r in runs], [r[1] for r in runs]


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
    hyd = torch.tensor(metrics.KYTE_DOOLITTLE, device="cuda")
    chg = torch.tensor(metrics.RESIDUE_CHARGE, device="cuda")
    words = metrics.motif_masks(metrics.LIABILITY_MOTIFS)
    ratio = lambda r: round(r["hip"]["median_ms"] / args.step_ms, 3) if args.step_ms else "not measured"
    res = {"device": torch.cuda.get_device_name(0), "K": K, "A": args.a, "counted_residues": args.counted, "sampler_step_ms": args.step_ms,
           "cases": {}}
    for G, N in SHAPES:
        name = f"{G} x {N}"
        if args.hip_only and args.case not in (None, name):
            continue
        designs, native, gm = designs_of(G, N, K, args.counted, seed=1)
        ctx, antigen = context_of(native, gm, args.a, seed=2)
        rows = G * N
        hip_p = lambda: metrics.patches(designs, gm, context=ctx, antigen_mask=antigen, group_size=N)
        hip_l = lambda: metrics.liabilities(designs, gm, group_size=N)
        hip_c = lambda: metrics.contacts(designs, gm, context=ctx, antigen_mask=antigen, group_size=N)
        if args.hip_only:
            for _ in range(args.warmup + args.repeats):
                hip_p()
                hip_l()
                hip_c()
            torch.cuda.synchronize()
            continue
        tr = min(args.torch_rows, rows) // N * N or N
        form_p = lambda: torch_patches(designs, gm, ctx, antigen, N, tr, hyd, chg)
        p_hip, p_torch = alternate(hip_p, form_p, args.warmup, args.repeats)
        c_hip = [timed(hip_c) for _ in range(args.warmup + args.repeats)][args.warmup:]
        got, ref = hip_p(), form_p()
        scale = ref["psh"].abs().clamp_min(1e-30)
        p = {"hip": stats_ms(p_hip), "torch": dict(stats_ms(p_torch, rows / tr), measured_on_rows=tr), "contacts": stats_ms(c_hip),
             "exposed_per_design_min_max": [int(got["n_exposed"].min()), int(got["n_exposed"].max())],
             "pairs_per_design_min_max": [int(got["n_pairs"].min()), int(got["n_pairs"].max())],
             "rows_where_torch_counts_differ": int(((ref["n_exposed"] != got["n_exposed"][:tr]) | (ref["n_pairs"] != got["n_pairs"][:tr])).sum()),
             "largest_relative_psh_difference": float(((ref["psh"] - got["psh"][:tr]).abs() / scale).max())}
        p["torch_over_hip"] = round(p["torch"]["median_ms"] / p["hip"]["median_ms"], 2)
        p["contacts_over_hip"] = round(p["contacts"]["median_ms"] / p["hip"]["median_ms"], 2)
        p["hip_over_sampler_step"] = ratio(p)
        form_l = lambda: torch_motifs(designs, gm, words, N)
        l_hip, l_torch = alternate(hip_l, form_l, args.warmup, args.repeats)
        got, ref = hip_l(), form_l()
        mine = torch.stack([got[n] for n in metrics.LIABILITY_MOTIFS], 1)
        l = {"hip": stats_ms(l_hip), "torch": stats_ms(l_torch), "motifs_per_design_min_max": [int(got["n_motifs"].min()), int(got["n_motifs"].max())],
             "rows_where_torch_counts_differ": int((ref != mine).any(1).sum())}
        l["torch_over_hip"] = round(l["torch"]["median_ms"] / l["hip"]["median_ms"], 2)
        l["hip_over_sampler_step"] = ratio(l)
        res["cases"][name] = {"patches": p, "liabilities": l}
        del designs, ctx, got, ref
        torch.cuda.empty_cache()
    if args.hip_only:
        return
    print(json.dumps(res, indent=1))
    if args.json:
        with open(args.json, "w") as f:
            json.dump(res, f, indent=1)
    if args.md:
        with open(args.md, "w") as f:
            f.write("| call | shape | HIP ms (median, min - max) | torch ms (median) | torch / HIP | contacts ms (median) | contacts / HIP | "
                    "HIP / one sampler step" + (f" ({args.step_ms:.3f} ms)" if args.step_ms else "") + " |\n|---|---|---|---|---|---|---|---|\n")
            for name, case in res["cases"].items():
                for call in ("patches", "liabilities"):
                    r = case[call]
                    note = f" (on {r['torch']['measured_on_rows']} rows, scaled)" if "measured_on_rows" in r["torch"] else ""
                    other = f"{r['contacts']['median_ms']} | {r['contacts_over_hip']}" if "contacts" in r else "- | -"
                    f.write(f"| {call} | {name} | {r['hip']['median_ms']} ({r['hip']['min_ms']} - {r['hip']['max_ms']}) | "
                            f"{r['torch']['median_ms']}{note} | {r['torch_over_hip']} | {other} | {r['hip_over_sampler_step']} |\n")
            f.write("\nRows where the broadcast form's n_exposed or n_pairs differ from the kernel's: "
                    + ", ".join(f"{c['patches']['rows_where_torch_counts_differ']} of {c['patches']['torch']['measured_on_rows']} ({n})"
                                for n, c in res["cases"].items())
                    + "; largest relative difference of psh: "
                    + ", ".join(f"{c['patches']['largest_relative_psh_difference']:.1e} ({n})" for n, c in res["cases"].items())
                    + ".  Rows where the gather form's motif counts differ from the kernel's: "
                    + ", ".join(f"{c['liabilities']['rows_where_torch_counts_differ']} ({n})" for n, c in res["cases"].items()) + ".\n")


if __name__ == "__main__":
    main()
