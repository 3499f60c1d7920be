#!/usr/bin/env python3
"""Reverse-sampler cost of particle steering (diffab_sample_options.steering), ROWS state rows in groups of --group, K = 128, benchmark
model, one context per row (256 rows fill the chip: the patch-resident module launch, what bench.py times; the rows of a group share
their generation mask and tables, which is all the kernels read).

Cases, alternating inside one process (the order reversed every other round), each a --warmup-step untimed call and then ONE call of
--steps steps from t = T on the re-initialised state, bracketed by hipEvents after a device synchronise (bench.py's timed block):
  free     diffab_sample_loop_ex without options, unsteered
  zero     diffab_sample_loop_ex, option `steering`, with strength 0, ess_threshold 1 (the kernels run every step, nothing resamples; bitwise the free
           result - checked)
  steered  the same with strength 1, ess_threshold 2: every group resamples at every step but the last
Reported per case: median / min / max ms per step over --repeats rounds; for `steered` the number of resampling steps and of surviving
initial rows.  Prints one JSON document (and writes it with --json).  --cases runs a subset (a kernel trace per case:
rocprofv3 --kernel-trace --stats -- python tools/steering_bench.py --cases steered --repeats 1).

    python tools/steering_bench.py [--steps 100 --warmup 5 --repeats 5 --rows 256 --group 16 --k 128] [--cases free,zero,steered] [--json OUT]
"""
import torch

from sampler_bench_common import SamplerRun, bench_model, case_names, emit, parser, rounds, stats

CASES = ("free", "zero", "steered")


def main():
    ap = parser(CASES)
    ap.add_argument("--group", type=int, default=16, help="rows per steering group")
    args = ap.parse_args()
    R, K, N = args.rows, args.k, args.group
    if N < 1 or R % N:
        raise SystemExit("--rows must be a multiple of --group")
    names = case_names(args, CASES)

    from diffab_pytorch.steering import ParticleSteering, c_struct, lineage, scratch_bytes

    dims, model = bench_model()
    T = model.T
    if not (1 <= args.steps <= T and 0 <= args.warmup <= T and args.repeats >= 1):
        raise SystemExit(f"need 1 <= --steps <= T = {T}, 0 <= --warmup <= T and --repeats >= 1")
    run = SamplerRun(model, dims, R, K, group=N)
    chain = torch.zeros(R, K, dtype=torch.int32, device="cuda")
    ridx = torch.arange(K, dtype=torch.int32, device="cuda").expand(R, K).contiguous()
    logw, u_prev, energy = (torch.zeros(R, device="cuda") for _ in range(3))
    anc = torch.empty(T + 1, R, dtype=torch.int32, device="cuda")
    scratch = torch.empty(scratch_bytes(R, K), dtype=torch.uint8, device="cuda")
    steers = {"free": None, "zero": ParticleSteering(strength=0.0, ess_threshold=1.0), "steered": ParticleSteering(strength=1.0, ess_threshold=2.0)}
    options = {n: None if sp is None else dict(steering=c_struct(sp, T, N, chain, ridx, None, logw, u_prev, energy, anc, scratch))
               for n, sp in steers.items()}

    def init():
        logw.zero_(), u_prev.zero_()
        run.init()

    runs = {n: [] for n in names}
    final = {}
    for _, n in rounds(names, args.repeats):
        init()
        if args.warmup:
            run.loop(T, T - args.warmup, options[n])
        init()
        runs[n].append(run.timed(lambda: run.loop(T, T - args.steps, options[n])) / args.steps)
        final[n] = run.final()
        if n == "steered":
            final_anc = anc.clone()
    out = {"what": "reverse sampler with particle steering: ms per step unsteered / strength 0 / resampling at every step",
           "rows": R, "group": N, "k": K, "T": T, "steps": args.steps, "warmup": args.warmup, "repeats": args.repeats,
           "device": torch.cuda.get_device_name(), "cases": []}
    if "free" in final and "zero" in final:
        out["zero_bitwise_free"] = all(torch.equal(final["free"][k], final["zero"][k]) for k in final["free"])
    ref = stats(runs[names[0]])[0]
    for n in names:
        med, st = stats(runs[n])
        case = {"case": n, "ms_per_step": st, f"vs_{names[0]}_pct": round(100 * (med - ref) / ref, 2)}
        if n == "steered":
            ts = [t for t in range(T, T - args.steps, -1) if t - 1 > T - args.steps]
            glob = final_anc[torch.tensor(ts, device="cuda")].to(torch.int64) + torch.arange(R, device="cuda") // N * N
            case["steering_steps"] = len(ts)
            case["steps_that_moved_rows"] = int((glob != torch.arange(R, device="cuda")).any(1).sum())
            case["surviving_initial_rows"] = int(lineage(glob).unique().numel())
        out["cases"].append(case)
    emit(out, args.json)


if __name__ == "__main__":
    main()
