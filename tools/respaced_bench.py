#!/usr/bin/env python3
"""Design throughput of fewer-step reverse sampling (diffab_sample_options.steps), ROWS patches, K = 128, benchmark model, one context per
row (256 rows fill the chip: the patch-resident module launch, what bench.py times).

Cases, alternating inside one process (the order reversed every other round), each a --warmup-step untimed call of the ordinary loop
and then ONE call of the whole reverse run from t = T on the initial state, bracketed by hipEvents after a device synchronise (bench.py's
timed block):
  off    diffab_sample_loop, every step T .. 1
  n100   diffab_sample_loop_ex, option `steps`, listing every step (bitwise "off")
  n50, n20, n10   the same with steps = n (DiffAb.sample(steps=n)'s even list and jump coefficients)
The step plans, jump coefficients and reverse IGSO3 tables are built once, outside the timed block.  Reported per case: median / min /
max ms per call and per executed step over --repeats rounds, designs per second (rows / call time), the speed-up over "off", and
whether n100 ended on the state of "off", bitwise.  Prints one JSON document (and writes it with --json).  --cases runs a subset (a
kernel trace per case: rocprofv3 --kernel-trace --stats -- python tools/respaced_bench.py --cases n20 --repeats 1).

    python tools/respaced_bench.py [--warmup 5 --repeats 5 --rows 256 --k 128] [--cases off,n100,...] [--json OUT]
"""
import ctypes as C

import torch

from sampler_bench_common import SamplerRun, bench_model, case_names, emit, parser, rounds, stats

CASES = ("off", "n100", "n50", "n20", "n10")


def main():
    args = parser(CASES, steps=False).parse_args()
    R, K = args.rows, args.k
    names = case_names(args, CASES)

    from diffab_pytorch import _hip
    from diffab_pytorch.diffusion import even_steps, jump_coefficients

    dims, model = bench_model()
    T = model.T
    if not (0 <= args.warmup <= T and args.repeats >= 1):
        raise SystemExit(f"need 0 <= --warmup <= T = {T} and --repeats >= 1")
    run = SamplerRun(model, dims, R, K)
    plans = {}
    for n in names:
        if n == "off":
            continue
        steps = even_steps(T, 0, int(n[1:]))
        bj, aj = jump_coefficients(model.sched, steps, 0, model.beta_max)
        so3 = model._reverse_so3_steps(steps, 0, bj)
        plan_dev = torch.empty(3 * (T + 1), dtype=torch.int32, device="cuda")
        host = ((C.c_int32 * steps.numel())(*steps.tolist()), (C.c_float * (T + 1))(*bj.tolist()), (C.c_float * (T + 1))(*aj.tolist()))
        plans[n] = (_hip.SampleSteps(steps.numel(), *host, _hip.ptr(plan_dev)), so3.struct(), steps.numel(), (host, plan_dev, so3))

    def loop(n, t_stop=0):
        if n == "off":
            run.loop(T, t_stop)
        else:
            st, tab = plans[n][:2]
            run.loop(T, 0, dict(steps=st), tab=tab)

    runs = {n: [] for n in names}
    final = {}
    for _, n in rounds(names, args.repeats):
        if args.warmup:
            run.init()
            loop("off", T - args.warmup)
        run.init()
        runs[n].append(run.timed(lambda: loop(n)))
        final[n] = run.final()
    out = {"what": "fewer-step reverse sampling: ms per call of a whole reverse run from t = T, ms per executed step, designs per second",
           "rows": R, "k": K, "T": T, "warmup": args.warmup, "repeats": args.repeats, "generated_residues": int(run.gm.sum()),
           "device": torch.cuda.get_device_name(), "cases": []}
    if "off" in final and "n100" in final:
        out["n100_final_state_bitwise_off"] = all(torch.equal(final["n100"][k], final["off"][k]) for k in final["off"])
    ref = stats(runs[names[0]])[0]
    for n in names:
        med, st_call = stats(runs[n], 3)
        n_exec = T if n == "off" else plans[n][2]
        _, st_step = stats([r / n_exec for r in runs[n]])
        out["cases"].append({"case": n, "executed_steps": n_exec, "ms_per_call": st_call, "ms_per_step": st_step,
                             "designs_per_s": round(R / (med / 1e3), 1), f"speedup_vs_{names[0]}": round(ref / med, 3)})
    emit(out, args.json)


if __name__ == "__main__":
    main()
