#!/usr/bin/env python3
"""Reverse-sampler cost of trajectory recording (diffab_sample_options.record), ROWS patches, K = 128, benchmark model, one context per row
(256 rows fill the chip: the patch-resident module launch, what bench.py times).

Cases, alternating inside one process (the order reversed every other round), each a --warmup-step untimed call and then ONE call of
--steps steps from t = T on the initial state, bracketed by hipEvents after a device synchronise (bench.py's timed block):
  off         diffab_sample_loop (no record)
  state       diffab_sample_loop_ex, option `record`: the state at every step
  state_pred  the same, the state and the predictions at every step
  pred_10     the same, the state and the predictions at every 10th step
The record buffers are allocated once, outside the timed block.  Reported per case: median / min / max ms per step over --repeats
rounds, and whether every case ended on the state of "off", bitwise.  Prints one JSON document (and writes it with --json).
--cases runs a subset (a kernel trace per case: rocprofv3 --kernel-trace --stats -- python tools/trajectory_bench.py --cases off).

    python tools/trajectory_bench.py [--steps 100 --warmup 5 --repeats 5 --rows 256 --k 128] [--cases off,state,...] [--json OUT]
"""
import ctypes as C

import torch

from sampler_bench_common import SamplerRun, bench_model, case_names, emit, parser, rounds, stats

CASES = ("off", "state", "state_pred", "pred_10")


def main():
    args = parser(CASES).parse_args()
    R, K = args.rows, args.k
    names = case_names(args, CASES)

    from diffab_pytorch import _hip

    dims, model = bench_model()
    T = model.T
    if not (1 <= args.steps <= T and 0 <= args.warmup <= T and args.repeats >= 1):
        raise SystemExit(f"need 1 <= --steps <= T = {T}, 0 <= --warmup <= T and --repeats >= 1")
    run = SamplerRun(model, dims, R, K)
    V = model.denoiser.dims["V"]
    slot_dev = torch.empty(T + 1, dtype=torch.int32, device="cuda")

    def record(stride, predictions, t_start, t_stop):
        steps = list(range(t_start, t_stop, -stride))
        n = len(steps)
        table = [-1] * (T + 1)
        for j, t in enumerate(steps):
            table[t] = j
        buf = {"seq": torch.empty(R, n, K, dtype=torch.int64, device="cuda"), "x": torch.empty(R, n, K, 3, device="cuda"),
               "O": torch.empty(R, n, K, 3, 3, device="cuda")}
        if predictions:
            buf.update(pred_x=torch.empty(R, n, K, 3, device="cuda"), pred_O=torch.empty(R, n, K, 3, 3, device="cuda"),
                       seq_probs=torch.empty(R, n, K, V, device="cuda"))
        rec = _hip.SampleRecord(n, (C.c_int32 * (T + 1))(*table), _hip.ptr(slot_dev),
                                *(_hip.ptr(buf.get(k)) for k in ("seq", "x", "O", "pred_x", "pred_O", "seq_probs")))
        return rec, buf

    shape = {"off": None, "state": (1, False), "state_pred": (1, True), "pred_10": (10, True)}
    recs = {n: None if shape[n] is None else record(*shape[n], T, T - args.steps) for n in names}
    warm = {n: None if shape[n] is None else record(*shape[n], T, T - args.warmup) for n in names if args.warmup}
    record_mib = {n: round(sum(b.numel() * b.element_size() for b in recs[n][1].values()) / 2**20, 1) for n in names if recs[n]}

    def loop(rec, t_start, t_stop):
        run.loop(t_start, t_stop, None if rec is None else dict(record=rec[0]))

    runs = {n: [] for n in names}
    final = {}
    for _, n in rounds(names, args.repeats):
        run.init()
        if args.warmup:
            loop(warm[n], T, T - args.warmup)
        run.init()
        runs[n].append(run.timed(lambda: loop(recs[n], T, T - args.steps)) / args.steps)
        final[n] = run.final()
    out = {"what": "reverse sampler with trajectory recording: ms per step, no record / state every step / state + predictions every "
                   "step / state + predictions every 10th step",
           "rows": R, "k": K, "T": T, "steps": args.steps, "warmup": args.warmup, "repeats": args.repeats,
           "generated_residues": int(run.gm.sum()), "record_mib": record_mib, "device": torch.cuda.get_device_name(), "cases": []}
    ref_final = final[names[0]]
    out[f"final_state_bitwise_{names[0]}"] = {n: all(torch.equal(final[n][k], ref_final[k]) for k in ref_final) for n in names}
    ref = stats(runs[names[0]])[0]
    for n in names:
        med, st = stats(runs[n])
        out["cases"].append({"case": n, "ms_per_step": st, f"vs_{names[0]}_pct": round(100 * (med - ref) / ref, 2)})
    emit(out, args.json)


if __name__ == "__main__":
    main()
