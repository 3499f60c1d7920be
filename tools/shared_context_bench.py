#!/usr/bin/env python3
"""Reverse-sampler ms/step for ROWS = B N designs drawn from B shared contexts (diffab_sample_options.ctx_of_row), K = 128, benchmark model.

The variants alternate inside one process: for each of --repeats rounds, every N of --ns runs a --warmup-step untimed call, then ONE
call of --steps steps from t = T on the re-initialised state, bracketed by hipEvents after a device synchronise (bench.py's warm-up and
timed block).  Every variant has the same seeded state and generation masks; only the number of distinct contexts (ROWS / N) changes.  N = 1 is diffab_sample_loop
itself (one context per row, what bench.py times).  Reported per variant: the median / min / max ms per step over the rounds,
residue-steps/s at the median, the workspace bytes and the context bytes held.  Prints one JSON document (and writes it with --json).

    python tools/shared_context_bench.py [--steps 100 --warmup 5 --repeats 5 --rows 256 --k 128 --ns 1,16,64,256] [--json OUT]
"""
import argparse
import ctypes as C
import json

import torch

from sampler_bench_common import bench_model, device_inputs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--rows", type=int, default=256, help="designs (state rows) per call: B N")
    ap.add_argument("--k", type=int, default=128)
    ap.add_argument("--ns", default="1,16,64,256", help="designs per context N (each must divide --rows)")
    ap.add_argument("--json", help="also write the result here")
    args = ap.parse_args()
    ns = [int(v) for v in args.ns.split(",")]
    R, K = args.rows, args.k
    if any(R % n for n in ns) or args.steps < 1 or args.warmup < 0:
        raise SystemExit(f"every N of --ns must divide --rows {R}; --steps >= 1")

    from diffab_pytorch import _hip

    lib = _hip.lib()
    dims, model = bench_model()
    if args.steps > model.T or args.warmup > model.T:
        raise SystemExit(f"--steps and --warmup must be <= T = {model.T}")
    # R contexts (variant N uses the first R / N) and one seeded state of R rows, shared by every variant
    res_all, pair_all, seq0, x0, O0, gm = device_inputs(dims, R, K).values()

    hd = model.denoiser.hip_dims(R, K)
    w = model.denoiser.hip_weights()
    sd = model._sched_on_device()
    tab = model._reverse_so3().struct()
    seed = 2024
    seq, x, O = seq0.clone(), x0.clone(), O0.clone()
    var = {}
    for n in ns:
        n_ctx = R // n
        ws_bytes = (lib.diffab_sample_workspace_bytes(C.byref(hd)) if n == 1 else
                    lib.diffab_sample_shared_workspace_bytes(C.byref(hd), n_ctx))
        var[n] = dict(n_ctx=n_ctx, ws=_hip.workspace(ws_bytes), ws_bytes=int(ws_bytes), res=res_all[:n_ctx], pair=pair_all[:n_ctx],
                      map=(C.c_int32 * R)(*[r // n for r in range(R)]), runs=[])

    def call(v, n, t_start, t_stop):
        common = (_hip.ptr(seq), _hip.ptr(x), _hip.ptr(O), _hip.ptr(v["res"]), _hip.ptr(v["pair"]))
        opt = None if n == 1 else C.byref(_hip.SampleOptions(n_ctx=v["n_ctx"], ctx_of_row=v["map"]))
        _hip.check(lib.diffab_sample_loop_ex(C.byref(hd), C.byref(w.struct), C.byref(sd.struct), C.byref(tab), *common, _hip.ptr(gm), seed, 0,
                                             t_start, t_stop, _hip.ptr(v["ws"]), v["ws"].numel(), 0, opt, _hip.stream_ptr()),
                   "diffab_sample_loop_ex")

    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for rep in range(args.repeats):
        for n in (ns if rep % 2 == 0 else ns[::-1]):  # alternate the order between rounds as well
            v = var[n]
            for timed in (False, True):  # warm-up steps from t = T, then the timed steps from t = T on the re-initialised state
                seq.copy_(seq0), x.copy_(x0), O.copy_(O0)
                _hip.check(lib.diffab_sample_init(_hip.ptr(seq), _hip.ptr(x), _hip.ptr(O), _hip.ptr(gm), seed, 0, R, K, model.T,
                                                  _hip.stream_ptr()), "sample_init")
                if not timed and args.warmup:
                    call(v, n, model.T, model.T - args.warmup)
            torch.cuda.synchronize()
            ev0.record()
            call(v, n, model.T, model.T - args.steps)
            ev1.record()
            torch.cuda.synchronize()
            v["runs"].append(ev0.elapsed_time(ev1) / args.steps)
            if not (torch.isfinite(x).all() and torch.isfinite(O).all()):
                raise SystemExit(f"N = {n}: non-finite state")
    out = {"what": "reverse-sampler ms per step, ROWS designs from ROWS / N shared contexts (diffab_sample_options.ctx_of_row; N = 1: "
                   "diffab_sample_loop)", "rows": R, "k": K, "steps": args.steps, "warmup": args.warmup, "repeats": args.repeats,
           "device": torch.cuda.get_device_name(), "variants": []}
    ctx_row_bytes = K * dims["D"] * 4 + K * K * dims["C"] * 4
    for n in ns:
        v = var[n]
        runs = sorted(v["runs"])
        med = runs[len(runs) // 2]
        out["variants"].append({"n": n, "n_ctx": v["n_ctx"], "ms_per_step_median": round(med, 4), "ms_per_step_min": round(runs[0], 4),
                                "ms_per_step_max": round(runs[-1], 4), "spread_pct": round(100 * (runs[-1] - runs[0]) / med, 2),
                                "ms_per_step_runs": [round(r, 4) for r in v["runs"]],
                                "residue_steps_per_s": round(R * K / (med * 1e-3)), "workspace_bytes": v["ws_bytes"],
                                "context_bytes": v["n_ctx"] * ctx_row_bytes})
    print(json.dumps(out))
    if args.json:
        with open(args.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
