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
import argparse
import ctypes as C
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "diffab-pytorch_amd"))

import torch  # noqa: E402


def random_rotations(n, g):
    q = torch.randn(n, 4, device="cuda", generator=g)
    w, x, y, z = (q / q.norm(dim=-1, keepdim=True)).unbind(-1)
    return torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w),
                        2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w),
                        2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)], -1).view(n, 3, 3)


def stats(runs):
    s = sorted(runs)
    med = s[len(s) // 2]
    return med, {"median": round(med, 4), "min": round(s[0], 4), "max": round(s[-1], 4), "spread_pct": round(100 * (s[-1] - s[0]) / med, 2),
                 "runs": [round(r, 4) for r in runs]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--rows", type=int, default=256, help="patches (state rows) per call")
    ap.add_argument("--k", type=int, default=128)
    ap.add_argument("--t-opt", type=int, default=8, help="optimisation: forward-noise the native to this step, then denoise")
    ap.add_argument("--json", help="also write the result here")
    args = ap.parse_args()
    R, K = args.rows, args.k

    from diffab_pytorch import DiffAb, _hip, synthetic as syn

    lib = _hip.lib()
    dims = dict(syn.BENCH_DIMS)
    torch.manual_seed(0)  # bench.py's model: default init of the boundary module
    model = DiffAb(dims["D"], dims["C"], dims["NL"], dims["DS"], dims["PQ"], dims["PV"], dims["H"]).cuda()
    T = model.T
    if not (1 <= args.steps <= T and 0 <= args.warmup <= T and 1 <= args.t_opt <= T):
        raise SystemExit(f"need 1 <= --steps, --t-opt <= T = {T} and 0 <= --warmup <= T")
    g = torch.Generator(device="cuda").manual_seed(0)
    res = torch.randn(R, K, dims["D"], device="cuda", generator=g)
    pair = torch.randn(R, K, K, dims["C"], device="cuda", generator=g)
    seq0 = torch.randint(0, 20, (R, K), device="cuda", generator=g)
    x0 = 10 * torch.randn(R, K, 3, device="cuda", generator=g)
    O0 = random_rotations(R * K, g).view(R, K, 3, 3).contiguous()
    start = torch.randint(0, K - 20, (R, 1), device="cuda", generator=g)
    length = torch.randint(5, 21, (R, 1), device="cuda", generator=g)
    pos = torch.arange(K, device="cuda")[None]
    gm = ((pos >= start) & (pos < start + length)).contiguous()

    hd = model.denoiser.hip_dims(R, K)
    w = model.denoiser.hip_weights()
    sd = model._sched_on_device()
    tab = model._reverse_so3().struct()
    fwd = model.orientation_diffuser.so3.struct()
    ws = _hip.workspace(lib.diffab_sample_workspace_bytes(C.byref(hd)))
    seed = 2024
    seq, x, O = seq0.clone(), x0.clone(), O0.clone()
    modes = {"codesign": 0, "fixed_backbone": _hip.FLAG_KEEP_STRUCTURE, "structure": _hip.FLAG_KEEP_SEQUENCE}

    def init(keep, t_opt=None):
        seq.copy_(seq0), x.copy_(x0), O.copy_(O0)
        p = (_hip.ptr(seq), _hip.ptr(x), _hip.ptr(O), _hip.ptr(gm))
        if t_opt is None:
            _hip.check(lib.diffab_sample_init_ex(*p, seed, 0, R, K, T, keep, None, _hip.stream_ptr()), "sample_init_ex")
        else:
            _hip.check(lib.diffab_sample_init_noised(C.byref(sd.struct), C.byref(fwd), *p, seed, 0, R, K, t_opt, keep, None,
                                                     _hip.stream_ptr()),
                       "sample_init_noised")

    def loop(keep, t_start, t_stop):
        _hip.check(lib.diffab_sample_loop(C.byref(hd), C.byref(w.struct), C.byref(sd.struct), C.byref(tab), _hip.ptr(seq), _hip.ptr(x),
                                          _hip.ptr(O), _hip.ptr(res), _hip.ptr(pair), _hip.ptr(gm), seed, 0, t_start, t_stop, _hip.ptr(ws),
                                          ws.numel(), keep, _hip.stream_ptr()), "diffab_sample_loop")

    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def timed(fn):
        torch.cuda.synchronize()
        ev0.record()
        fn()
        ev1.record()
        torch.cuda.synchronize()
        if not (torch.isfinite(x).all() and torch.isfinite(O).all()):
            raise SystemExit("non-finite state")
        return ev0.elapsed_time(ev1)

    step_runs = {m: [] for m in modes}
    traj_runs = {(m, kind): [] for m in modes for kind in ("full", "opt")}
    names = list(modes)
    for rep in range(args.repeats):
        for m in (names if rep % 2 == 0 else names[::-1]):
            keep = modes[m]
            # per-step cost: warm-up steps, then the timed steps from t = T on the re-initialised state
            init(keep)
            if args.warmup:
                loop(keep, T, T - args.warmup)
            init(keep)
            step_runs[m].append(timed(lambda: loop(keep, T, T - args.steps)) / args.steps)
            # whole trajectories: initial state + loop, full (T steps) and optimisation (t_opt steps from the noised native)
            traj_runs[(m, "full")].append(timed(lambda: (init(keep), loop(keep, T, 0))))
            traj_runs[(m, "opt")].append(timed(lambda: (init(keep, args.t_opt), loop(keep, args.t_opt, 0))))
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
    print(json.dumps(out))
    if args.json:
        with open(args.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
