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
import argparse
import ctypes as C
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "diffab-pytorch_amd"))

import torch  # noqa: E402

CASES = ("off", "state", "state_pred", "pred_10")


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
    V = model.denoiser.dims["V"]

    hd = model.denoiser.hip_dims(R, K)
    w = model.denoiser.hip_weights()
    sd = model._sched_on_device()
    tab = model._reverse_so3().struct()
    ws = _hip.workspace(lib.diffab_sample_workspace_bytes(C.byref(hd)))
    seed = 2024
    seq, x, O = seq0.clone(), x0.clone(), O0.clone()
    slot_dev = torch.empty(T + 1, dtype=torch.int32, device="cuda")

    def record(stride, predictions, t_start, t_stop):
        """(diffab_sample_record, its buffers) for the steps t_start, t_start - stride, ... > t_stop"""
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

    def init():
        seq.copy_(seq0), x.copy_(x0), O.copy_(O0)
        _hip.check(lib.diffab_sample_init(_hip.ptr(seq), _hip.ptr(x), _hip.ptr(O), _hip.ptr(gm), seed, 0, R, K, T, _hip.stream_ptr()),
                   "sample_init")

    def loop(rec, t_start, t_stop):
        opt = None if rec is None else C.byref(_hip.SampleOptions(record=rec[0]))
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
                loop(warm[n], T, T - args.warmup)
            init()
            runs[n].append(timed(lambda: loop(recs[n], T, T - args.steps)) / args.steps)
            final[n] = (seq.clone(), x.clone(), O.clone())
    out = {"what": "reverse sampler with trajectory recording: ms per step, no record / state every step / state + predictions every "
                   "step / state + predictions every 10th step",
           "rows": R, "k": K, "T": T, "steps": args.steps, "warmup": args.warmup, "repeats": args.repeats,
           "generated_residues": int(gm.sum()), "record_mib": record_mib, "device": torch.cuda.get_device_name(), "cases": []}
    ref_final = final[names[0]]
    out[f"final_state_bitwise_{names[0]}"] = {n: all(torch.equal(a, b) for a, b in zip(final[n], ref_final)) for n in names}
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
