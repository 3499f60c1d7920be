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
import argparse
import ctypes as C
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "diffab-pytorch_amd"))

import torch  # noqa: E402

CASES = ("free", "zero", "steered")


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
    ap.add_argument("--group", type=int, default=16, help="rows per steering group")
    ap.add_argument("--k", type=int, default=128)
    ap.add_argument("--cases", default=",".join(CASES), help=f"comma-separated subset of {','.join(CASES)}")
    ap.add_argument("--json", help="also write the result here")
    args = ap.parse_args()
    R, K, N = args.rows, args.k, args.group
    if N < 1 or R % N:
        raise SystemExit("--rows must be a multiple of --group")
    names = args.cases.split(",")
    if not names or any(n not in CASES for n in names):
        raise SystemExit(f"--cases: expected a comma-separated subset of {','.join(CASES)}")

    from diffab_pytorch import DiffAb, _hip, synthetic as syn
    from diffab_pytorch.steering import ParticleSteering, c_struct, lineage, scratch_bytes

    lib = _hip.lib()
    dims = dict(syn.BENCH_DIMS)
    torch.manual_seed(0)  # bench.py's model: default init of the boundary module
    model = DiffAb(dims["D"], dims["C"], dims["NL"], dims["DS"], dims["PQ"], dims["PV"], dims["H"]).cuda()
    T = model.T
    if not (1 <= args.steps <= T and 0 <= args.warmup <= T and args.repeats >= 1):
        raise SystemExit(f"need 1 <= --steps <= T = {T}, 0 <= --warmup <= T and --repeats >= 1")
    g = torch.Generator(device="cuda").manual_seed(0)
    res = torch.randn(R, K, dims["D"], device="cuda", generator=g)
    pair = torch.randn(R, K, K, dims["C"], device="cuda", generator=g)
    seq0 = torch.randint(0, 20, (R, K), device="cuda", generator=g)
    x0 = 10 * torch.randn(R, K, 3, device="cuda", generator=g)
    O0 = random_rotations(R * K, g).view(R, K, 3, 3).contiguous()
    start = torch.randint(0, K - 20, (R // N, 1), device="cuda", generator=g).repeat_interleave(N, dim=0)
    length = torch.randint(5, 21, (R // N, 1), device="cuda", generator=g).repeat_interleave(N, dim=0)
    pos = torch.arange(K, device="cuda")[None]
    gm = ((pos >= start) & (pos < start + length)).contiguous()
    chain = torch.zeros(R, K, dtype=torch.int32, device="cuda")
    ridx = torch.arange(K, dtype=torch.int32, device="cuda").expand(R, K).contiguous()
    logw, u_prev, energy = (torch.zeros(R, device="cuda") for _ in range(3))
    anc = torch.empty(T + 1, R, dtype=torch.int32, device="cuda")
    scratch = torch.empty(scratch_bytes(R, K), dtype=torch.uint8, device="cuda")
    steers = {"free": None, "zero": ParticleSteering(strength=0.0, ess_threshold=1.0), "steered": ParticleSteering(strength=1.0, ess_threshold=2.0)}
    structs = {n: None if sp is None else c_struct(sp, T, N, chain, ridx, None, logw, u_prev, energy, anc, scratch) for n, sp in steers.items()}

    hd = model.denoiser.hip_dims(R, K)
    w = model.denoiser.hip_weights()
    sd = model._sched_on_device()
    tab = model._reverse_so3().struct()
    ws = _hip.workspace(lib.diffab_sample_workspace_bytes(C.byref(hd)))
    seed = 2024
    seq, x, O = seq0.clone(), x0.clone(), O0.clone()

    def init():
        seq.copy_(seq0), x.copy_(x0), O.copy_(O0)
        logw.zero_(), u_prev.zero_()
        _hip.check(lib.diffab_sample_init(_hip.ptr(seq), _hip.ptr(x), _hip.ptr(O), _hip.ptr(gm), seed, 0, R, K, T, _hip.stream_ptr()),
                   "sample_init")

    def loop(gs, t_start, t_stop):
        opt = None if gs is None else C.byref(_hip.SampleOptions(steering=gs))
        _hip.check(lib.diffab_sample_loop_ex(C.byref(hd), C.byref(w.struct), C.byref(sd.struct), C.byref(tab), _hip.ptr(seq), _hip.ptr(x),
                                             _hip.ptr(O), _hip.ptr(res), _hip.ptr(pair), _hip.ptr(gm), seed, 0, t_start, t_stop, _hip.ptr(ws),
                                             ws.numel(), 0, opt, _hip.stream_ptr()), "diffab_sample_loop_ex")

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

    runs = {n: [] for n in names}
    final = {}
    for rep in range(args.repeats):
        for n in (names if rep % 2 == 0 else names[::-1]):
            gs = structs[n]
            init()
            if args.warmup:
                loop(gs, T, T - args.warmup)
            init()
            runs[n].append(timed(lambda: loop(gs, T, T - args.steps)) / args.steps)
            final[n] = {"seq_idx": seq.clone(), "translations": x.clone(), "orientations": O.clone()}
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
    print(json.dumps(out))
    if args.json:
        with open(args.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
