#!/usr/bin/env python3
"""Reverse-sampler cost of noise scales and sequence temperature (diffab_sample_options.temperature), ROWS patches, K = 128, benchmark model, one
context per row (256 rows fill the chip: the patch-resident module launch, what bench.py times).

Cases, alternating inside one process (the order reversed every other round), each a --warmup-step untimed call and then ONE call of
--steps steps from t = T on the re-initialised state, bracketed by hipEvents after a device synchronise (bench.py's timed block):
  free     diffab_sample_loop_ex without options, untempered
  ones     diffab_sample_loop_ex, option `temperature`, with every pointer set and every value 1 (rot_row k (T + 1) over a one-scale stack: the kernel
           reads the values; bitwise the free result - checked)
  sweep    the same with a mixed per-row sweep: lambda_x in {0.5, 0.75, 1, 1.25}, lambda_O over 8 values (an 8-scale
           stacked table) and 0, tau in {0, 0.1, 0.3, 0.5, 1, 2}, cycled over the rows
Reported per case: median / min / max ms per step over --repeats rounds; and, once, the build time of the stacked IGSO3 tables (outside
the timed steps): 1, 8 and 16 scales at T = 100.  Prints one JSON document (and writes it with --json).  --cases runs a subset (a kernel
trace per case: rocprofv3 --kernel-trace --stats -- python tools/temperature_bench.py --cases sweep --repeats 1).

    python tools/temperature_bench.py [--steps 100 --warmup 5 --repeats 5 --rows 256 --k 128] [--cases free,ones,sweep] [--json OUT]
"""
import time

import torch

from sampler_bench_common import SamplerRun, bench_model, case_names, emit, parser, rounds, stats

CASES = ("free", "ones", "sweep")


def main():
    args = parser(CASES).parse_args()
    R, K = args.rows, args.k
    names = case_names(args, CASES)

    from diffab_pytorch import _hip, temperature as tp

    dims, model = bench_model()
    T = model.T
    if not (1 <= args.steps <= T and 0 <= args.warmup <= T and args.repeats >= 1):
        raise SystemExit(f"need 1 <= --steps <= T = {T}, 0 <= --warmup <= T and --repeats >= 1")
    run = SamplerRun(model, dims, R, K)

    # the stacked tables: build time once (a fresh table each, synchronised), outside every timed step
    build_ms = {}
    for n in (1, 8, 16):
        scales = tuple(float(torch.tensor(0.125 * (k + 1))) for k in range(n))
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        model._rev_so3_tempered.clear()
        model._reverse_so3_tempered(scales, None, 0, None)
        torch.cuda.synchronize()
        build_ms[str(n)] = round(1e3 * (time.perf_counter() - t0), 2)
    model._rev_so3_tempered.clear()

    cyc = lambda vals: torch.tensor([vals[r % len(vals)] for r in range(R)], dtype=torch.float32)  # noqa: E731
    setups = {"ones": (torch.ones(R), torch.ones(R), torch.ones(R)),
              "sweep": (cyc([0.5, 0.75, 1.0, 1.25]), cyc([0.25, 0.5, 0.75, 1.0, 0.0, 1.25, 1.5, 2.0, 0.1]),
                        cyc([0.0, 0.1, 0.3, 0.5, 1.0, 2.0]))}
    options, keep_alive, tabs = {"free": None}, [], {"free": model._reverse_so3()}
    for n, (lx, lo, tau) in setups.items():
        scales = tp.rotation_scales(lo)
        tabs[n] = model._reverse_so3_tempered(scales, None, 0, None)
        dev = [lx.cuda(), lo.cuda(), tau.cuda(), tp.rotation_rows(lo, scales, T).cuda()]
        keep_alive.append(dev)
        options[n] = dict(temperature=_hip.SampleTemperature(*(_hip.ptr(v) for v in dev)))

    def loop(n, t_start, t_stop):
        run.loop(t_start, t_stop, options[n], tab=tabs[n].struct())

    runs = {n: [] for n in names}
    final = {}
    for _, n in rounds(names, args.repeats):
        run.init()
        if args.warmup:
            loop(n, T, T - args.warmup)
        run.init()
        runs[n].append(run.timed(lambda: loop(n, T, T - args.steps)) / args.steps)
        final[n] = run.final()
    out = {"what": "reverse sampler with noise scales and sequence temperature: ms per step untempered / all ones through the tempered "
                   "entry / a mixed per-row sweep; stacked IGSO3 table build time (ms) by number of rotation scales",
           "rows": R, "k": K, "T": T, "steps": args.steps, "warmup": args.warmup, "repeats": args.repeats,
           "device": torch.cuda.get_device_name(), "table_build_ms": build_ms, "cases": []}
    if "free" in final and "ones" in final:
        out["ones_bitwise_free"] = all(torch.equal(final["free"][k], final["ones"][k]) for k in final["free"])
    ref = stats(runs[names[0]])[0]
    for n in names:
        med, st = stats(runs[n])
        out["cases"].append({"case": n, "ms_per_step": st, f"vs_{names[0]}_pct": round(100 * (med - ref) / ref, 2)})
    emit(out, args.json)


if __name__ == "__main__":
    main()
