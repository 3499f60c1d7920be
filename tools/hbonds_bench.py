#!/usr/bin/env python3
"""Cost of the hydrogen-bond filter (diffab_pytorch.metrics.hbonds) on synthetic designs: tools/geometry_bench.py's designs and context
(synthetic.py patches, N Gaussian perturbations of each, one generated segment of --counted residues per patch, A context atoms per
residue of which the first four stand for N, CA, C, O, the far half of the other residues flagged as the antigen).

Two shapes: G x N designs of K residues (16 x 1024 x 128 by default) and the sampler's 256 x 128 batch (256 patches, one design each).
The whole Python call is timed beside a chunked torch broadcast formulation of the BOND ENERGIES ALONE on the same device: given the
atoms the kernel built (its O and H outputs, N, CA, C of the rows and of the context), the float32 CA cull and the float64
Kabsch-Sander energy of all K x K pairs of a row, E < -0.5 - no derived atoms, no partners, no secondary structure, no counts.  The two
ALTERNATE in one process, after a warm-up, with device events around the call after a device synchronise; the torch form is timed on
--torch-rows rows and scaled to all of them, and the result says so.  The rows where its number of bonded acceptors differs from the
kernel's are counted.
--step-ms takes bench.py's ms_per_step of the same session (256 x 128 batch) and adds every call's ratio to one sampler step; without
it the ratio is reported as not measured.  --hip-only runs nothing but the kernel calls (for a kernel trace taken in a run of its own).
Prints one JSON document (--json OUT) and writes the table of profiles/hbonds.md (--md OUT).

    python tools/hbonds_bench.py [--g 16 --n 1024 --k 128 --a 15 --counted 20 --repeats 10 --warmup 2 --step-ms MS] [--json OUT] [--md OUT]
"""
import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "diffab-pytorch_amd"))
sys.path.insert(0, os.path.join(REPO, "tools"))

import torch  # noqa: E402

from geometry_bench import alternate, context_of  # noqa: E402
from metrics_bench import designs_of  # noqa: E402
from sampler_bench_common import stats_ms  # noqa: E402


def row_atoms(designs, gm, ctx, N, out):
    """N, CA, C, O, H (rows,K,3) fp32 and has_o, has_h (rows,K) of every row, from the kernel's own derived atoms."""
    from diffab_pytorch import io as dio

    own = dio.backbone_from_frames(designs["translations"], designs["orientations"], ("N", "CA", "C"))
    gen = gm.repeat_interleave(N, 0)[..., None, None]
    nca = torch.where(gen, own, ctx["xyz"][:, :, :3].repeat_interleave(N, 0))
    has_o, has_h = ~torch.isnan(out["O"][..., 0]), ~torch.isnan(out["H"][..., 0])
    return nca[:, :, 0], nca[:, :, 1], nca[:, :, 2], torch.nan_to_num(out["O"]), torch.nan_to_num(out["H"]), has_o, has_h


def torch_bonds(atoms, lo, hi, chunk=64):
    """(rows', K) bool: the acceptors with at least one bond.  Pairs d = a and d = a + 1 (the patches are one chain) are excluded."""
    n, ca, c, o, h, has_o, has_h = (t[lo:hi] for t in atoms)
    K = n.shape[1]
    idx = torch.arange(K, device=n.device)
    allowed = (idx[None, :] != idx[:, None]) & (idx[None, :] != idx[:, None] + 1)
    out = []
    for r0 in range(0, hi - lo, chunk):
        s = slice(r0, r0 + chunk)
        d = ca[s, :, None] - ca[s, None, :]
        near = ((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]) < 81.0

        def inv(p, q):
            v = p[s].double()[:, :, None] - q[s].double()[:, None, :]
            return 1.0 / torch.sqrt((v[..., 0] * v[..., 0] + v[..., 1] * v[..., 1]) + v[..., 2] * v[..., 2]).clamp_min(0.5)

        E = 27.888 * (((inv(o, n) + inv(c, h)) - inv(o, h)) - inv(c, n))
        hb = near & allowed & has_o[s, :, None] & has_h[s, None, :] & (E < -0.5)
        out.append(hb.any(-1))
    return torch.cat(out)


def main():
    ap = argparse.ArgumentParser()
    for name, default in (("g", 16), ("n", 1024), ("k", 128), ("a", 15), ("counted", 20), ("repeats", 10), ("warmup", 2), ("torch-rows", 1024)):
        ap.add_argument("--" + name, type=int, default=default)
    ap.add_argument("--step-ms", type=float)
    ap.add_argument("--hip-only", action="store_true")
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
        name = f"G = {G}, N = {N}, K = {K}"
        hip = lambda: metrics.hbonds(designs, gm, context=ctx, antigen_mask=antigen, group_size=N)
        if args.hip_only:
            for _ in range(args.warmup + args.repeats):
                hip()
            torch.cuda.synchronize()
            continue
        out = hip()
        atoms = row_atoms(designs, gm, ctx, N, out)
        tr = min(args.torch_rows, rows)
        t_hip, t_torch = alternate(hip, lambda: torch_bonds(atoms, 0, tr), args.warmup, args.repeats)
        want = torch_bonds(atoms, 0, tr)
        got = out["o_hn_partner"][:tr, :, 0] >= 0
        c = {"hip": stats_ms(t_hip), "torch_energies_only": dict(stats_ms(t_torch, rows / tr), measured_on_rows=tr)}
        c["torch_over_hip"] = round(c["torch_energies_only"]["median_ms"] / c["hip"]["median_ms"], 2)
        c["rows_where_torch_bonded_acceptors_differ"] = int((want != got).any(1).sum())
        c["hip_over_sampler_step"] = round(c["hip"]["median_ms"] / args.step_ms, 3) if args.step_ms else "not measured"
        c["mean_bonded_acceptors_per_row"] = round(float(got.sum(1).float().mean()), 2)
        c["mean_hbonds_with_a_generated_end"] = round(float(out["n_hbonds"].float().mean()), 2)
        res["cases"][name] = c
    if args.hip_only:
        return
    print(json.dumps(res, indent=1))
    if args.json:
        with open(args.json, "w") as f:
            json.dump(res, f, indent=1)
    if args.md:
        with open(args.md, "w") as f:
            f.write("| shape | HIP ms (median, min - max) | torch ms, bond energies only (scaled) | torch / HIP | HIP / one sampler step"
                    + (f" ({args.step_ms:.3f} ms)" if args.step_ms else "") + " |\n|---|---|---|---|---|\n")
            for name, c in res["cases"].items():
                t = c["torch_energies_only"]
                f.write(f"| {name} | {c['hip']['median_ms']} ({c['hip']['min_ms']} - {c['hip']['max_ms']}) | {t['median_ms']} "
                        f"(on {t['measured_on_rows']} rows) | {c['torch_over_hip']} | {c['hip_over_sampler_step']} |\n")
            f.write("\nRows where the torch form's bonded acceptors differ from the kernel's: "
                    + ", ".join(f"{c['rows_where_torch_bonded_acceptors_differ']} of {c['torch_energies_only']['measured_on_rows']} ({name})"
                                for name, c in res["cases"].items()) + ".\n")


if __name__ == "__main__":
    main()
