#!/usr/bin/env python3
"""Reverse-sampler cost and effect of structure guidance (diffab_sample_options.guidance), ROWS patches, K = 128, benchmark model, one context
per row (256 rows fill the chip: the patch-resident module launch, what bench.py times).

Cases, alternating inside one process (the order reversed every other round), each a --warmup-step untimed call and then ONE call of
--steps steps from t = T on the re-initialised state, bracketed by hipEvents after a device synchronise (bench.py's timed block):
  free     diffab_sample_loop_ex without options
  zero     diffab_sample_loop_ex, option `guidance`, with both weights 0 (the guidance kernel runs every step; bitwise the free result - checked)
  guided   the same with clash = bond = 1 (d0 = L = 3.8 A, max_shift 1 A, every step)
Reported per case: median / min / max ms per step over --repeats rounds, and for the final designs of the last round (same seeds for
every case) the clash / bond statistics of diffab_guidance_energy over the pairs with a generated residue.  Prints one JSON document
(and writes it with --json).  --cases runs a subset (a kernel trace per case:
rocprofv3 --kernel-trace --stats -- python tools/guidance_bench.py --cases guided --repeats 1).

    python tools/guidance_bench.py [--steps 100 --warmup 5 --repeats 5 --rows 256 --k 128] [--cases free,zero,guided] [--json OUT]
"""
import torch

from sampler_bench_common import SamplerRun, bench_model, case_names, emit, parser, rounds, stats

CASES = ("free", "zero", "guided")


def main():
    args = parser(CASES).parse_args()
    R, K = args.rows, args.k
    names = case_names(args, CASES)

    from diffab_pytorch.guidance import SampleGuidance, c_struct, structure_energy

    dims, model = bench_model()
    T = model.T
    if not (1 <= args.steps <= T and 0 <= args.warmup <= T and args.repeats >= 1):
        raise SystemExit(f"need 1 <= --steps <= T = {T}, 0 <= --warmup <= T and --repeats >= 1")
    run = SamplerRun(model, dims, R, K)
    gm = run.gm
    chain = torch.zeros(R, K, dtype=torch.int32, device="cuda")
    ridx = torch.arange(K, dtype=torch.int32, device="cuda").expand(R, K).contiguous()
    shift = torch.empty(R, K, 3, device="cuda")
    guides = {"free": None, "zero": SampleGuidance(), "guided": SampleGuidance(clash=1.0, bond=1.0)}
    options = {n: None if gd is None else dict(guidance=c_struct(gd, T, chain, ridx, None, shift)) for n, gd in guides.items()}

    runs = {n: [] for n in names}
    final = {}
    for _, n in rounds(names, args.repeats):
        run.init()
        if args.warmup:
            run.loop(T, T - args.warmup, options[n])
        run.init()
        runs[n].append(run.timed(lambda: run.loop(T, T - args.steps, options[n])) / args.steps)
        final[n] = run.final()
    out = {"what": "reverse sampler with structure guidance: ms per step unguided / zero weights / clash + bond, and the final designs' "
                   "clash and bond statistics (diffab_guidance_energy, pairs with a generated residue, d0 = L = 3.8 A)",
           "rows": R, "k": K, "T": T, "steps": args.steps, "warmup": args.warmup, "repeats": args.repeats,
           "device": torch.cuda.get_device_name(), "cases": []}
    if "free" in final and "zero" in final:
        out["zero_bitwise_free"] = all(torch.equal(final["free"][k], final["zero"][k]) for k in final["free"])
    if "free" in final and "guided" in final:
        out["guided_seq_orient_bitwise_free"] = all(torch.equal(final["free"][k], final["guided"][k]) for k in ("seq_idx", "orientations"))
    ref = stats(runs[names[0]])[0]
    for n in names:
        med, st = stats(runs[n])
        e = structure_energy(final[n]["translations"], gm, chain_idx=chain, residue_idx=ridx)
        design = {"clash_sum": round(float(e["clash"].sum()), 3), "clash_pairs": int(e["n_clash"].sum()),
                  "rows_with_clash": int((e["n_clash"] > 0).sum()), "bond_sum": round(float(e["bond"].sum()), 3),
                  "max_bond_deviation": round(float(e["max_bond_deviation"].max()), 3),
                  "median_row_max_bond_deviation": round(float(e["max_bond_deviation"].median()), 3)}
        out["cases"].append({"case": n, "ms_per_step": st, f"vs_{names[0]}_pct": round(100 * (med - ref) / ref, 2), "final_designs": design})
    emit(out, args.json)


if __name__ == "__main__":
    main()
