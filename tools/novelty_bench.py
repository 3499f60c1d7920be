#!/usr/bin/env python3
"""Cost of design novelty (diffab_pytorch.metrics.novelty) on synthetic sequences: queries of lengths 8 - 22 (a CDR-H3) in rows of 64,
library entries of lengths 5 - 30 in rows of 32, tokens uniform over the 20 amino acids, a tenth of the library planted as queries after
0 - 3 substitutions.

Cases: 16 x 1024 = 16 384 queries against libraries of 10^4, 10^5 and 10^6 entries; 256 x 1 queries against 10^5; the 16 384 queries
against themselves with the full matrix (exclude="self", radius=0: uniqueness).  At each the whole Python call is timed after a
warm-up, with device events around the call after a device synchronise.  The work of a case is counted in character-steps: one step
of the recurrence per query and library token, R * sum(len_lib) - what the rule needs, not the padding steps the kernel also runs -
and the rate is that over the median time.

Beside it a torch formulation of the same rule on the same device: the plain dynamic programme one row of the table at a time for a
batch of pairs, the horizontal term as a running minimum (cummin), about a dozen launches per row.  It runs at --torch-queries x
--torch-entries pairs, where it is checked against the kernel's matrix, and its time PER PAIR is scaled to each case's pair count:
labelled as scaled, it is not a measurement at that size.
--hip-only runs nothing but the kernel calls, of every case or of --case NAME alone (for a kernel trace taken in a run of its own).
Prints one JSON document (--json OUT) and writes the table of profiles/novelty.md (--md OUT).

    python tools/novelty_bench.py [--repeats 5 --warmup 1 --torch-queries 64 --torch-entries 4096] [--json OUT] [--md OUT]
"""
import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "diffab-pytorch_amd"))
sys.path.insert(0, os.path.join(REPO, "tools"))

import torch  # noqa: E402

from sampler_bench_common import stats_ms, timed  # noqa: E402

CASES = (("16 x 1024 vs 10^4", 16384, 10 ** 4, False), ("16 x 1024 vs 10^5", 16384, 10 ** 5, False), ("16 x 1024 vs 10^6", 16384, 10 ** 6, False),
         ("256 x 1 vs 10^5", 256, 10 ** 5, False), ("16 x 1024 vs themselves, matrix", 16384, 16384, True))


def random_set(n, lo, hi, width, seed):
    """n sequences of lengths lo .. hi in rows of `width`, 255 behind them, on the device."""
    from diffab_pytorch import metrics

    gen = torch.Generator(device="cuda").manual_seed(seed)
    lengths = torch.randint(lo, hi + 1, (n,), device="cuda", generator=gen, dtype=torch.int32)
    tokens = torch.randint(0, 20, (n, width), device="cuda", generator=gen, dtype=torch.uint8)
    tokens[torch.arange(width, device="cuda")[None, :] >= lengths[:, None]] = 255
    return metrics.SequenceSet(tokens, lengths)


def plant(library, queries, seed):
    """Every tenth library entry becomes a query with up to three tokens replaced."""
    gen = torch.Generator(device="cuda").manual_seed(seed)
    M, R, LQ = len(library), len(queries), queries.tokens.shape[1]
    at = torch.arange(0, M, 10, device="cuda")
    src = torch.randint(0, R, (len(at),), device="cuda", generator=gen)
    rows = queries.tokens[src].clone()
    n = queries.lengths[src]
    for _ in range(3):
        pos = (torch.rand(len(at), device="cuda", generator=gen) * n).long().clamp(max=LQ - 1)
        rows[torch.arange(len(at), device="cuda"), pos] = torch.randint(0, 20, (len(at),), device="cuda", generator=gen, dtype=torch.uint8)
    rows[torch.arange(LQ, device="cuda")[None, :] >= n[:, None]] = 255
    library.tokens[at] = 255
    library.tokens[at, :min(LQ, library.tokens.shape[1])] = rows[:, :library.tokens.shape[1]]
    library.lengths[at] = n.clamp(max=library.tokens.shape[1])


def torch_matrix(queries, library):
    """The rule as a batched row dynamic programme on the device: (R, M) int32."""
    q, nq, lib, nl = queries.tokens.long(), queries.lengths.long(), library.tokens.long(), library.lengths.long()
    (R, LQ), (M, LM) = q.shape, lib.shape
    nq, nl = nq.clamp(0, LQ), nl.clamp(0, LM)
    j = torch.arange(LM + 1, device=q.device, dtype=torch.int32)
    row = j.expand(R, M, LM + 1).contiguous()
    at = nl[None, :, None].expand(R, M, 1)
    out = torch.zeros(R, M, dtype=torch.int32, device=q.device)
    take = lambda: row.gather(2, at)[:, :, 0]
    out = torch.where((nq == 0)[:, None], take(), out)
    text_ok = lib < 32
    for i in range(1, int(nq.max()) + 1):
        a = q[:, i - 1]
        cost = (~((a[:, None, None] == lib[None]) & (a < 32)[:, None, None] & text_ok[None])).to(torch.int32)
        t = torch.empty_like(row)
        t[:, :, 0] = i
        t[:, :, 1:] = torch.minimum(row[:, :, 1:] + 1, row[:, :, :-1] + cost)
        row = torch.cummin(t - j, 2).values + j
        out = torch.where((nq == i)[:, None], take(), out)
    return out.int()


def main():
    ap = argparse.ArgumentParser()
    for name, default in (("repeats", 5), ("warmup", 1), ("torch-queries", 64), ("torch-entries", 4096)):
        ap.add_argument("--" + name, type=int, default=default)
    ap.add_argument("--hip-only", action="store_true")
    ap.add_argument("--case", help="one of the case names, e.g. '16 x 1024 vs 10^5' (default: every case, one after the other)")
    ap.add_argument("--json")
    ap.add_argument("--md")
    args = ap.parse_args()
    from diffab_pytorch import _hip, metrics

    _hip.lib()
    res = {"device": torch.cuda.get_device_name(0), "query_lengths": [8, 22], "library_lengths": [5, 30], "cases": {}}
    queries = {R: random_set(R, 8, 22, 64, seed=1) for R in {c[1] for c in CASES}}

    # the torch form, once, at a size it manages; checked against the kernel there
    if not args.hip_only:
        tq = metrics.SequenceSet(queries[16384].tokens[:args.torch_queries].contiguous(), queries[16384].lengths[:args.torch_queries].contiguous())
        tl = random_set(args.torch_entries, 5, 30, 32, seed=3)
        plant(tl, tq, seed=4)
        form = lambda: torch_matrix(tq, tl)
        for _ in range(args.warmup):
            form()
        t_torch = stats_ms([timed(form) for _ in range(args.repeats)])
        same = bool(torch.equal(form(), metrics.novelty(tq, tl, matrix=True)["matrix"]))
        pairs = args.torch_queries * args.torch_entries
        res["torch"] = dict(t_torch, queries=args.torch_queries, entries=args.torch_entries, pairs=pairs, equals_the_kernel_matrix=same,
                            ns_per_pair=round(t_torch["median_ms"] * 1e6 / pairs, 2))

    for name, R, M, against_self in CASES:
        if args.case not in (None, name):
            continue
        q = queries[R]
        if against_self:
            lib = q
            call = lambda: metrics.novelty(q, lib, exclude="self", radius=0, matrix=True)
        else:
            lib = random_set(M, 5, 30, 32, seed=2)
            plant(lib, q, seed=5)
            call = lambda: metrics.novelty(q, lib, radius=3)
        for _ in range(args.warmup):
            call()
        runs = [timed(call) for _ in range(args.repeats)]
        if args.hip_only:
            continue
        out = call()
        steps = R * int(lib.lengths.clamp(0, lib.tokens.shape[1]).long().sum())
        r = {"hip": stats_ms(runs), "pairs": R * M, "character_steps": steps}
        r["character_steps_per_s"] = float(f"{steps / (r['hip']['median_ms'] * 1e-3):.4g}")
        r["pairs_per_s"] = float(f"{R * M / (r['hip']['median_ms'] * 1e-3):.4g}")
        r["queries_at_distance_0"] = int((out["distance"] == 0).sum())
        r["mean_distance"] = round(float(out["distance"].float().mean()), 3)
        if "torch" in res:
            r["torch_scaled_ms"] = round(res["torch"]["ns_per_pair"] * R * M * 1e-6, 1)
            r["torch_scaled_over_hip"] = round(r["torch_scaled_ms"] / r["hip"]["median_ms"], 1)
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
            f.write("| case | pairs | character-steps | HIP ms (median, min - max) | character-steps / s | pairs / s | torch ms (SCALED from "
                    f"{res['torch']['queries']} x {res['torch']['entries']} pairs) | torch / HIP |\n|---|---|---|---|---|---|---|---|\n")
            for name, r in res["cases"].items():
                f.write(f"| {name} | {r['pairs']:.3g} | {r['character_steps']:.3g} | {r['hip']['median_ms']} ({r['hip']['min_ms']} - {r['hip']['max_ms']}) | "
                        f"{r['character_steps_per_s']:.3g} | {r['pairs_per_s']:.3g} | {r['torch_scaled_ms']} | {r['torch_scaled_over_hip']} |\n")
            t = res["torch"]
            f.write(f"\nThe torch row dynamic programme, measured: {t['median_ms']} ms ({t['min_ms']} - {t['max_ms']}) for {t['queries']} x {t['entries']} "
                    f"pairs = {t['ns_per_pair']} ns per pair; its matrix equals the kernel's: {t['equals_the_kernel_matrix']}.\n")


if __name__ == "__main__":
    main()
