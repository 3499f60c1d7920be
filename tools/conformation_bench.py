#!/usr/bin/env python3
"""Cost of loop conformations (diffab_pytorch.metrics.conformation) on synthetic loops: queries of ONE length (16 residues, a long
CDR-H3) in rows of 16, library loops of lengths 5 - 30 in rows of 32, phi / psi / omega uniform in (-pi, pi], one angle in a hundred
missing, every hundredth library entry of the queries' length a query turned by up to 0.2 rad per angle; angles=("phi", "psi").

Cases: 16 x 1024 = 16 384 queries against libraries of 10^4, 10^5 and 10^6 loops; 256 x 1 queries against 10^5; the 16 384 queries
against themselves with the full matrix (exclude="self").  At each the whole Python call is timed after a warm-up, with device events
around the call after a device synchronise - features (cos, sin in float64) included.  The work of a case is counted in COMPARED
pairs, those of equal length, at 2 * 2 A len flop each (one multiply and one add per feature), and the rate is set against the
157 TF fp32 matrix peak.

Beside it a torch form of the same rule on the same device, measured at the case's own size: the same features, then per length
bucket d = 2 - 2 * (q @ l.T) / n with n = mask_q @ mask_l.T, +inf below min_terms, min and argmin per query, the library in blocks of
--torch-block loops so that the (R, block) matrices fit.  It keeps no matrix, so the matrix case has no torch column.
--hip-only runs nothing but the kernel calls, of every case or of --case NAME alone (for a kernel trace taken in a run of its own).
Prints one JSON document (--json OUT) and writes the table of profiles/conformation.md (--md OUT).

    python tools/conformation_bench.py [--repeats 7 --warmup 2 --torch-block 65536] [--json OUT] [--md OUT]
"""
import argparse
import json
import math
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "diffab-pytorch_amd"))
sys.path.insert(0, os.path.join(REPO, "tools"))

import torch  # noqa: E402

from sampler_bench_common import stats_ms, timed  # noqa: E402

CASES = (("16 x 1024 vs 10^4", 16384, 10 ** 4, False), ("16 x 1024 vs 10^5", 16384, 10 ** 5, False), ("16 x 1024 vs 10^6", 16384, 10 ** 6, False),
         ("256 x 1 vs 10^5", 256, 10 ** 5, False), ("16 x 1024 vs themselves, matrix", 16384, 16384, True))
QUERY_LENGTH, ANGLES, WHICH = 16, ("phi", "psi"), (0, 1)
PEAK_F32_MATRIX = 157e12


def random_set(n, lo, hi, width, seed):
    """n loops of lengths lo .. hi in rows of `width`, NaN behind them and for one angle in a hundred, on the device."""
    from diffab_pytorch import metrics

    gen = torch.Generator(device="cuda").manual_seed(seed)
    lengths = torch.randint(lo, hi + 1, (n,), device="cuda", generator=gen, dtype=torch.int32)
    angles = (torch.rand(n, width, 3, device="cuda", generator=gen) * 2 - 1) * math.pi
    angles[torch.rand(n, width, 3, device="cuda", generator=gen) < 0.01] = math.nan
    angles[torch.arange(width, device="cuda")[None, :] >= lengths[:, None]] = math.nan
    return metrics.DihedralSet(angles, lengths)


def plant(library, queries, seed):
    """Every hundredth library entry becomes a query turned by up to 0.2 rad per angle."""
    gen = torch.Generator(device="cuda").manual_seed(seed)
    M, R, LQ = len(library), len(queries), queries.angles.shape[1]
    at = torch.arange(0, M, 100, device="cuda")
    src = torch.randint(0, R, (len(at),), device="cuda", generator=gen)
    library.angles[at] = math.nan
    library.angles[at, :LQ] = queries.angles[src] + (torch.rand(len(at), LQ, 3, device="cuda", generator=gen) - 0.5) * 0.4
    library.lengths[at] = queries.lengths[src]


def torch_nearest(queries, library, block, min_terms=1):
    """The rule per length bucket as dense products: (distance (R,), index (R,)) - no matrix, no n_within."""
    from diffab_pytorch import metrics

    qf, lf = metrics.dihedral_features(queries.angles, WHICH), metrics.dihedral_features(library.angles, WHICH)
    (R, LQ), (M, LM) = qf.shape[:2], lf.shape[:2]
    nq, nl = queries.lengths.clamp(0, LQ), library.lengths.clamp(0, LM)
    best = torch.full((R,), math.inf, device=qf.device)
    index = torch.full((R,), -1, dtype=torch.long, device=qf.device)
    for n in torch.unique(nq).tolist():
        rows, cols = (nq == n).nonzero()[:, 0], (nl == n).nonzero()[:, 0]
        if n == 0 or len(cols) == 0:
            continue
        q = qf[rows, :n]
        q_ok = torch.isfinite(q).all(-1)
        q = torch.where(q_ok[..., None], q, torch.zeros_like(q)).reshape(len(rows), -1)
        q_ok = q_ok.reshape(len(rows), -1).float()
        for c0 in range(0, len(cols), block):
            c = cols[c0:c0 + block]
            l = lf[c, :n]
            l_ok = torch.isfinite(l).all(-1)
            l = torch.where(l_ok[..., None], l, torch.zeros_like(l)).reshape(len(c), -1)
            terms = q_ok @ l_ok.reshape(len(c), -1).float().T
            d = 2 - 2 * (q @ l.T) / terms.clamp(min=1)
            d = torch.where(terms >= min_terms, d.clamp(min=0), torch.full_like(d, math.inf))
            low, arg = d.min(1)
            better = low < best[rows]
            best[rows] = torch.where(better, low, best[rows])
            index[rows] = torch.where(better, c[arg], index[rows])
    return best, index


def main():
    ap = argparse.ArgumentParser()
    for name, default in (("repeats", 7), ("warmup", 2), ("torch-block", 65536)):
        ap.add_argument("--" + name, type=int, default=default)
    ap.add_argument("--hip-only", action="store_true")
    ap.add_argument("--case", help="one of the case names, e.g. '16 x 1024 vs 10^5' (default: every case, one after the other)")
    ap.add_argument("--json")
    ap.add_argument("--md")
    args = ap.parse_args()
    from diffab_pytorch import _hip, metrics

    _hip.lib()
    res = {"device": torch.cuda.get_device_name(0), "query_length": QUERY_LENGTH, "library_lengths": [5, 30], "angles": list(ANGLES), "cases": {}}
    queries = {R: random_set(R, QUERY_LENGTH, QUERY_LENGTH, QUERY_LENGTH, seed=1) for R in {c[1] for c in CASES}}
    for name, R, M, against_self in CASES:
        if args.case not in (None, name):
            continue
        q = queries[R]
        if against_self:
            lib = q
            call = lambda: metrics.conformation(q, lib, angles=ANGLES, exclude="self", radius=0.5, matrix=True)
        else:
            lib = random_set(M, 5, 30, 32, seed=2)
            plant(lib, q, seed=5)
            call = lambda: metrics.conformation(q, lib, angles=ANGLES, radius=0.5)
        for _ in range(args.warmup):
            call()
        runs = [timed(call) for _ in range(args.repeats)]
        if args.hip_only:
            continue
        out = call()
        compared = R * int((lib.lengths == QUERY_LENGTH).sum())
        flop = compared * 2 * 2 * len(WHICH) * QUERY_LENGTH
        r = {"hip": stats_ms(runs), "pairs": R * M, "compared_pairs": compared, "flop": flop}
        seconds = r["hip"]["median_ms"] * 1e-3
        r["compared_pairs_per_s"] = float(f"{compared / seconds:.4g}")
        r["tflops"] = round(flop / seconds / 1e12, 2)
        r["share_of_f32_matrix_peak"] = round(flop / seconds / PEAK_F32_MATRIX, 4)
        r["queries_within_0.5"] = int((out["n_within"] > 0).sum())
        r["mean_distance"] = round(float(out["distance"][torch.isfinite(out["distance"])].mean()), 4)
        if not against_self:
            form = lambda: torch_nearest(q, lib, args.torch_block)
            try:
                for _ in range(args.warmup):
                    form()
                r["torch"] = stats_ms([timed(form) for _ in range(args.repeats)])
                r["torch_over_hip"] = round(r["torch"]["median_ms"] / r["hip"]["median_ms"], 2)
                d, index = form()
                r["torch_index_agrees"] = round(float((index == out["index"]).float().mean()), 4)
                r["torch_max_abs_distance_difference"] = float(f"{float((d - out['distance']).abs().nan_to_num(0, 0, 0).max()):.3g}")
            except RuntimeError as e:  # (out of memory at a size: reported, not hidden)
                r["torch_error"] = str(e).splitlines()[0][:200]
        res["cases"][name] = r
        del out, lib
        torch.cuda.empty_cache()
    if args.hip_only:
        return
    print(json.dumps(res, indent=1))
    if args.json:
        with open(args.json, "w") as f:
            json.dump(res, f, indent=1)
    if args.md:
        with open(args.md, "w") as f:
            f.write("| case | pairs | compared pairs | HIP ms (median, min - max) | compared pairs / s | TF (share of 157) | torch ms (median, min - max) | "
                    "torch / HIP |\n|---|---|---|---|---|---|---|---|\n")
            for name, r in res["cases"].items():
                t = r.get("torch")
                torch_ms = f"{t['median_ms']} ({t['min_ms']} - {t['max_ms']})" if t else r.get("torch_error", "-")
                f.write(f"| {name} | {r['pairs']:.3g} | {r['compared_pairs']:.3g} | {r['hip']['median_ms']} ({r['hip']['min_ms']} - {r['hip']['max_ms']}) | "
                        f"{r['compared_pairs_per_s']:.3g} | {r['tflops']} ({r['share_of_f32_matrix_peak']}) | {torch_ms} | {r.get('torch_over_hip', '-')} |\n")


if __name__ == "__main__":
    main()
