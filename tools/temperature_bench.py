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
import argparse
import ctypes as C
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "diffab-pytorch_amd"))

import torch  # noqa: E402

CASES = ("free", "ones", "sweep")


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
    ap.add_argument("--cases", default=",".join(CASES), help=f"comma-separated subset of {','.join(CASES)}")
    ap.add_argument("--json", help="also write the result here")
    args = ap.parse_args()
    R, K = args.rows, args.k
    names = args.cases.split(",")
    if not names or any(n not in CASES for n in names):
        raise SystemExit(f"--cases: expected a comma-separated subset of {','.join(CASES)}")

    from diffab_pytorch import DiffAb, _hip, synthetic as syn
    from diffab_pytorch import temperature as tp

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
    start = torch.randint(0, K - 20, (R, 1), device="cuda", generator=g)
    length = torch.randint(5, 21, (R, 1), device="cuda", generator=g)
    pos = torch.arange(K, device="cuda")[None]
    gm = ((pos >= start) & (pos < start + length)).contiguous()

    # the stacked tables: build time once (a fresh table each, synchronised), outside every timed step
    build_ms = {}
    base = model.sched["beta"].sqrt()
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
    structs, keep_alive, tabs = {"free": None}, [], {"free": model._reverse_so3()}
    for n, (lx, lo, tau) in setups.items():
        scales = tp.rotation_scales(lo)
        tabs[n] = model._reverse_so3_tempered(scales, None, 0, None)
        dev = [lx.cuda(), lo.cuda(), tau.cuda(), tp.rotation_rows(lo, scales, T).cuda()]
        keep_alive.append(dev)
        structs[n] = _hip.SampleTemperature(*(_hip.ptr(v) for v in dev))

    hd = model.denoiser.hip_dims(R, K)
    w = model.denoiser.hip_weights()
    sd = model._sched_on_device()
    ws = _hip.workspace(lib.diffab_sample_workspace_bytes(C.byref(hd)))
    seed = 2024
    seq, x, O = seq0.clone(), x0.clone(), O0.clone()

    def init():
        seq.copy_(seq0), x.copy_(x0), O.copy_(O0)
        _hip.check(lib.diffab_sample_init(_hip.ptr(seq), _hip.ptr(x), _hip.ptr(O), _hip.ptr(gm), seed, 0, R, K, T, _hip.stream_ptr()),
                   "sample_init")

    def loop(n, t_start, t_stop):
        tab = tabs[n].struct()
        opt = None if structs[n] is None else C.byref(_hip.SampleOptions(temperature=structs[n]))
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
            init()
            if args.warmup:
                loop(n, T, T - args.warmup)
            init()
            runs[n].append(timed(lambda: loop(n, T, T - args.steps)) / args.steps)
            final[n] = {"seq_idx": seq.clone(), "translations": x.clone(), "orientations": O.clone()}
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
    print(json.dumps(out))
    if args.json:
        with open(args.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
