#!/usr/bin/env python3
"""Reverse-sampler cost of the design modes (DIFFAB_FLAG_KEEP_STRUCTURE / _SEQUENCE) and of antibody optimisation, ROWS patches, K = 128,
benchmark model, one context per row (diffab_sample_loop, what bench.py times).

Two measurements, the variants alternating inside one process (the order reversed every other round):
  * ms per step of each mode: a --warmup-step untimed call, then ONE call of --steps steps from t = T on the mode's initial state
    (diffab_sample_init_ex with the mode's KEEP bit), bracketed by hipEvents after a device synchronise (bench.py's timed block);
  * designs/s of a whole trajectory: the initial state plus the loop, for a full run (uniform init, T steps) and for optimisation
    (the native forward-noised to --t-opt by diffab_sample_init_noised, then --t-opt steps), ROWS designs per call.
Reported per variant: median / min / max over --repeats rounds.  Prints one JSON document (and writes it with --json).

    python tools/design_modes_bench.py [--steps 100 --warmup 5 --repeats 5 --rows 256 --k 128 --t-opt 8] [--json OUT]
"""
import ctypes as C

import torch

from sampler_bench_common import SamplerRun, bench_model, emit, parser, rounds, stats


def main():
    ap = parser()
    ap.add_argument("--t-opt", type=int, default=8, help="optimisation: forward-noise the native to this step, then denoise")
    args = ap.parse_args()
    R, K = args.rows, args.k

    from diffab_pytorch import _hip

    dims, model = bench_model()
    T = model.T
    if not (1 <= args.steps <= T and 0 <= args.warmup <= T and 1 <= args.t_opt <= T):
        raise SystemExit(f"need 1 <= --steps, --t-opt <= T = {T} and 0 <= --warmup <= T")
    run = SamplerRun(model, dims, R, K)
    lib, seed = run.lib, run.seed
    fwd = model.orientation_diffuser.so3.struct()
    modes = {"codesign": 0, "fixed_backbone": _hip.FLAG_KEEP_STRUCTURE, "structure": _hip.FLAG_KEEP_SEQUENCE}

    def init(keep, t_opt=None):
        run.reset()
        if t_opt is None:
            _hip.check(lib.diffab_sample_init_ex(*run.state_ptrs(), seed, 0, R, K, T, keep, None, _hip.stream_ptr()), "sample_init_ex")
        else:
            _hip.check(lib.diffab_sample_init_noised(C.byref(run.sd.struct), C.byref(fwd), *run.state_ptrs(), seed, 0, R, K, t_opt, keep, None,
                                                     _hip.stream_ptr()),
                       "sample_init_noised")

    def loop(keep, t_start, t_stop):  # the entry without options, the mode's KEEP bit in its flags
        _hip.check(lib.diffab_sample_loop(C.byref(run.hd), C.byref(run.w.struct), C.byref(run.sd.struct), C.byref(run.tab), _hip.ptr(run.seq),
                                          _hip.ptr(run.x), _hip.ptr(run.O), _hip.ptr(run.res), _hip.ptr(run.pair), _hip.ptr(run.gm), seed, 0,
                                          t_start, t_stop, _hip.ptr(run.ws), run.ws.numel(), keep, _hip.stream_ptr()), "diffab_sample_loop")

    step_runs = {m: [] for m in modes}
    traj_runs = {(m, kind): [] for m in modes for kind in ("full", "opt")}
    names = list(modes)
    for _, m in rounds(names, args.repeats):
        keep = modes[m]
        # per-step cost: warm-up steps, then the timed steps from t = T on the re-initialised state
        init(keep)
        if args.warmup:
            loop(keep, T, T - args.warmup)
        init(keep)
        step_runs[m].append(run.timed(lambda: loop(keep, T, T - args.steps)) / args.steps)
        # whole trajectories: initial state + loop, full (T steps) and optimisation (t_opt steps from the noised native)
        traj_runs[(m, "full")].append(run.timed(lambda: (init(keep), loop(keep, T, 0))))
        traj_runs[(m, "opt")].append(run.timed(lambda: (init(keep, args.t_opt), loop(keep, args.t_opt, 0))))
    out = {"what": "reverse-sampler design modes: ms per step, and designs/s of a full T-step trajectory against optimisation from t_opt",
           "rows": R, "k": K, "T": T, "steps": args.steps, "warmup": args.warmup, "repeats": args.repeats, "t_opt": args.t_opt,
           "device": torch.cuda.get_device_name(), "modes": []}
    co_med, _ = stats(step_runs["codesign"])
    for m in names:
        med, st = stats(step_runs[m])
        full_med, full = stats(traj_runs[(m, "full")])
        opt_med, opt = stats(traj_runs[(m, "opt")])
        out["modes"].append({"mode": m, "ms_per_step": st, "vs_codesign_pct": round(100 * (med - co_med) / co_med, 2),
                             "full_trajectory_ms": full, "optimisation_trajectory_ms": opt,
                             "designs_per_s_full": round(R / (full_med * 1e-3), 1), "designs_per_s_opt": round(R / (opt_med * 1e-3), 1),
                             "opt_speedup": round(full_med / opt_med, 2)})
    emit(out, args.json)


if __name__ == "__main__":
    main()
