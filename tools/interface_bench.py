#!/usr/bin/env python3
"""Cost of the binding-mode calls (diffab_pytorch.metrics.contact_map / .pairwise_bits) on synthetic designs: tools/geometry_bench.py's
designs and context (synthetic.py patches, N Gaussian perturbations of each, one generated segment of --counted residues per patch, an
all-atom context of A atoms per residue with a ragged atom_mask, the far half of the other residues flagged as the antigen).

Three shapes, G patches x N designs of K = --k residues: 16 x 1024, 256 x 64 and 4 x 4096.  At each, both whole Python calls are timed
beside a torch formulation on the same device, the two ALTERNATING in one process after a warm-up, with device events around the call
after a device synchronise:
  contact_map    against torch.cdist of the generated atoms against the context atoms, in chunks of --torch-rows design rows, with an
                 any() over the atom axes - the map as booleans, not packed; it runs on --torch-rows rows and is scaled to all rows, and
                 cdist's distances are not the defined fp32 number: the rows whose contact count differs from the kernel's are counted;
  pairwise_bits  against the strong torch form: the words unpacked to fp16 zeros and ones over ALL 32 L columns, B @ B^T on the matrix
                 cores, the diagonal as n_set, the two quotients elementwise.  Timed whole (from the words) and as the product alone.
                 Its n_common is compared with the kernel's.
A fourth case feeds pairwise_bits random DENSE words (every column live) at 16 x 1024: the input the compaction cannot help.
The live word columns of every input are counted and printed beside its times.
--step-ms takes bench.py's ms_per_step of the same session (256 x 128 batch) and adds every call's ratio to one sampler step; without
it the ratio is reported as not measured.  --hip-only --case NAME runs nothing but the kernel calls of one case (for a kernel trace
taken in a run of its own).  Prints one JSON document (--json OUT) and writes the table of profiles/interface.md (--md OUT).

    python tools/interface_bench.py [--k 128 --a 15 --counted 20 --repeats 10 --warmup 2 --step-ms MS] [--json OUT] [--md OUT]
"""
import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "diffab-pytorch_amd"))
sys.path.insert(0, os.path.join(REPO, "tools"))

import torch  # noqa: E402

from geometry_bench import ATOMS, GLY, context_of  # noqa: E402
from metrics_bench import designs_of  # noqa: E402
from sampler_bench_common import stats_ms, timed  # noqa: E402

SHAPES = ((16, 1024), (256, 64), (4, 4096))


def torch_contact_map(designs, gm, ctx, antigen, N, rows, contact=5.0):
    """(rows, n, K) bool: generated residue x residue of the patch, by torch.cdist on `rows` design rows at once."""
    from diffab_pytorch import io as dio

    G, K = gm.shape
    n = int(gm[0].sum())
    idx = gm.nonzero()[:, 1].view(G, n)
    sub = {k: v[:rows] for k, v in designs.items()}
    pts = dio.backbone_from_frames(sub["translations"], sub["orientations"], ATOMS)
    bits = torch.where(sub["seq_idx"] == GLY, 15, 31)  # no CB on Gly
    g_of = torch.arange(rows, device="cuda") // N
    pick = idx[g_of]
    gp = pts.gather(1, pick[:, :, None, None].expand(rows, n, 5, 3)).reshape(rows, n * 5, 3)
    gv = ((bits.gather(1, pick)[:, :, None] >> torch.arange(5, device="cuda")) & 1).bool().reshape(rows, n * 5)
    A = ctx["xyz"].shape[2]
    cv = (ctx["atom_mask"] & ~gm[..., None]).reshape(G, K * A)[g_of]
    d = torch.cdist(gp, ctx["xyz"].reshape(G, K * A, 3)[g_of])
    d = d.masked_fill(~(gv[:, :, None] & cv[:, None, :]), float("inf"))
    near = (d.view(rows, n, 5, K, A) < contact).any(4).any(2) & antigen[g_of][:, None, :]
    near &= (pick[:, :, None] - torch.arange(K, device="cuda")).abs() != 1  # chain neighbours (one chain, residue_idx = arange(K))
    return near


def torch_unpack(bits, G, N):
    """(G, N, 32 L) fp16 zeros and ones."""
    w = bits.view(G, N, -1)
    return ((w[..., None] >> torch.arange(32, device="cuda", dtype=torch.int32)) & 1).to(torch.float16).view(G, N, -1)


def torch_product(B):
    return torch.bmm(B, B.transpose(1, 2))


def torch_pairwise(bits, G, N):
    c = torch_product(torch_unpack(bits, G, N)).float()
    n = c.diagonal(dim1=1, dim2=2)
    fcc = torch.where(n[:, :, None] == 0, 1.0, c / n[:, :, None])
    union = n[:, :, None] + n[:, None, :] - c
    return c, fcc, torch.where(union == 0, 1.0, c / union)


def alternate(hip, other, warmup, repeats):
    for _ in range(warmup):
        hip()
        other()
    runs = [(timed(hip), timed(other)) for _ in range(repeats)]
    return [r[0] for r in runs], [r[1] for r in runs]


def live_columns(bits, G, N):
    live = (bits.view(G, N, -1) != 0).any(1).sum(1)
    return [int(live.min()), int(live.max())]


def main():
    ap = argparse.ArgumentParser()
    for name, default in (("k", 128), ("a", 15), ("counted", 20), ("repeats", 10), ("warmup", 2), ("torch-rows", 256)):
        ap.add_argument("--" + name, type=int, default=default)
    ap.add_argument("--step-ms", type=float)
    ap.add_argument("--hip-only", action="store_true")
    ap.add_argument("--case", help="with --hip-only: one of the case names, e.g. '16 x 1024' or '16 x 1024, dense'")
    ap.add_argument("--json")
    ap.add_argument("--md")
    args = ap.parse_args()
    from diffab_pytorch import _hip, metrics

    _hip.lib()
    K = args.k
    ratio = lambda r: round(r["hip"]["median_ms"] / args.step_ms, 3) if args.step_ms else "not measured"
    res = {"device": torch.cuda.get_device_name(0), "K": K, "A": args.a, "counted_residues": args.counted, "sampler_step_ms": args.step_ms,
           "cases": {}}
    for G, N in SHAPES:
        name = f"{G} x {N}"
        if args.hip_only and args.case not in (name, name + ", dense"):
            continue
        designs, native, gm = designs_of(G, N, K, args.counted, seed=1)
        ctx, antigen = context_of(native, gm, args.a, seed=2)
        rows = G * N
        hip_c = lambda: metrics.contact_map(designs, gm, context=ctx, antigen_mask=antigen, group_size=N)
        out = hip_c()
        bits = out["bits"]
        inputs = [(name, bits)]
        if (G, N) == SHAPES[0]:
            g = torch.Generator(device="cuda").manual_seed(5)
            inputs.append((name + ", dense", torch.randint(-2 ** 31, 2 ** 31, tuple(bits.shape), device="cuda", generator=g).to(torch.int32)))
        if args.hip_only:
            for case, b in inputs:
                if case == args.case:
                    for _ in range(args.warmup + args.repeats):
                        if case == name:
                            hip_c()
                        metrics.pairwise_bits(b, group_size=N)
                    torch.cuda.synchronize()
            continue
        tr = min(args.torch_rows, rows) // N * N or N
        c_hip, c_torch = alternate(hip_c, lambda: torch_contact_map(designs, gm, ctx, antigen, N, tr), args.warmup, args.repeats)
        near = torch_contact_map(designs, gm, ctx, antigen, N, tr)
        c = {"hip": stats_ms(c_hip), "torch": dict(stats_ms(c_torch, rows / tr), measured_on_rows=tr),
             "contacts_per_design_min_max": [int(out["n_contacts"].min()), int(out["n_contacts"].max())],
             "rows_where_torch_contact_count_differs": int((near.sum((1, 2)) != out["n_contacts"][:tr]).sum())}
        c["torch_over_hip"] = round(c["torch"]["median_ms"] / c["hip"]["median_ms"], 2)
        c["hip_over_sampler_step"] = ratio(c)
        res["cases"][name] = {"contact_map": c}
        for case, b in inputs:
            hip_p = lambda: metrics.pairwise_bits(b, group_size=N)
            p_hip, p_torch = alternate(hip_p, lambda: torch_pairwise(b, G, N), args.warmup, args.repeats)
            B = torch_unpack(b, G, N)
            p_gemm = [timed(lambda: torch_product(B)) for _ in range(args.repeats)]
            del B
            got, ref = hip_p(), torch_pairwise(b, G, N)
            p = {"hip": stats_ms(p_hip), "torch": stats_ms(p_torch), "torch_product_alone": stats_ms(p_gemm), "words_per_design": int(b[0].numel()),
                 "live_columns_min_max": live_columns(b, G, N), "largest_n_common": int(got["n_common"].max()),
                 "pairs_where_torch_n_common_differs": int((ref[0] != got["n_common"].float()).sum())}
            p["torch_over_hip"] = round(p["torch"]["median_ms"] / p["hip"]["median_ms"], 2)
            p["torch_product_alone_over_hip"] = round(p["torch_product_alone"]["median_ms"] / p["hip"]["median_ms"], 2)
            p["hip_over_sampler_step"] = ratio(p)
            res["cases"].setdefault(case, {})["pairwise_bits"] = p
            del got, ref
        del designs, ctx, bits, out, inputs
        torch.cuda.empty_cache()
    if args.hip_only:
        return
    print(json.dumps(res, indent=1))
    if args.json:
        with open(args.json, "w") as f:
            json.dump(res, f, indent=1)
    if args.md:
        with open(args.md, "w") as f:
            f.write("| call | shape | live columns of L | HIP ms (median, min - max) | torch ms (median) | torch / HIP | HIP / one sampler step"
                    + (f" ({args.step_ms:.3f} ms)" if args.step_ms else "") + " |\n|---|---|---|---|---|---|---|\n")
            for name, case in res["cases"].items():
                for call in ("contact_map", "pairwise_bits"):
                    if call not in case:
                        continue
                    r = case[call]
                    note = f" (on {r['torch']['measured_on_rows']} rows, scaled)" if "measured_on_rows" in r["torch"] else \
                        f"; product alone {r['torch_product_alone']['median_ms']}"
                    live = "-" if call == "contact_map" else "{} - {} of {}".format(*r["live_columns_min_max"], r["words_per_design"])
                    f.write(f"| {call} | {name} | {live} | {r['hip']['median_ms']} ({r['hip']['min_ms']} - {r['hip']['max_ms']}) | "
                            f"{r['torch']['median_ms']}{note} | {r['torch_over_hip']} | {r['hip_over_sampler_step']} |\n")
            f.write("\nRows where the cdist form's contact count differs from the kernel's: "
                    + ", ".join(f"{c['contact_map']['rows_where_torch_contact_count_differs']} of {c['contact_map']['torch']['measured_on_rows']} ({n})"
                                for n, c in res["cases"].items() if "contact_map" in c)
                    + ".  Pairs where the product form's n_common differs from the kernel's: "
                    + ", ".join(f"{c['pairwise_bits']['pairs_where_torch_n_common_differs']} ({n})" for n, c in res["cases"].items()) + ".\n")


if __name__ == "__main__":
    main()
