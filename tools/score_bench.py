#!/usr/bin/env python3
"""Cost of design scoring (DiffAb.score / diffab_score_designs) against the reverse sampler, benchmark model, K = 128.

Workload: --contexts contexts x --designs designs each (context_index), a --grid-step grid of timesteps 1..T (25 steps by default), M = 1
draw: contexts x designs x steps evaluated rows.  Three measurements, alternating inside one process (the order reversed every other
round), each bracketed by hipEvents after a device synchronise:
  * score, shared contexts, for each --rows-per-launch value: designs/s and ms per chunk of that many rows;
  * the same rows with one context per design (the contexts replicated: the pair stream is no longer shared between rows);
  * diffab_sample_loop's ms per step at the same B (B = rows per launch, one context per row, --sampler-steps steps from t = T).
Reported per variant: median / min / max over --repeats rounds.  Prints one JSON document (and writes it with --json).

    python tools/score_bench.py [--contexts 16 --designs 64 --grid-step 4 --rows-per-launch 256 512 --repeats 5] [--json OUT]
"""
import argparse
import ctypes as C
import json

import torch

from sampler_bench_common import bench_model, device_inputs, stats, timed


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--contexts", type=int, default=16)
    ap.add_argument("--designs", type=int, default=64, help="designs per context")
    ap.add_argument("--grid-step", type=int, default=4, help="timestep grid 1, 1 + s, ... <= T (T = 100, s = 4: 25 steps)")
    ap.add_argument("--rows-per-launch", type=int, nargs="+", default=[256, 512])
    ap.add_argument("--sampler-steps", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--k", type=int, default=128)
    ap.add_argument("--once", action="store_true", help="one score call at the first --rows-per-launch, nothing else (for a profiler)")
    ap.add_argument("--json", help="also write the result here")
    args = ap.parse_args()
    K, n_ctx, N = args.k, args.contexts, args.designs
    R = n_ctx * N

    from diffab_pytorch import _hip

    lib = _hip.lib()
    dims, model = bench_model()
    T = model.T
    grid = list(range(1, T + 1, args.grid_step))
    res, pair, seq0, x0, O0, gm = device_inputs(dims, R, K, n_ctx=n_ctx).values()
    ci = torch.arange(n_ctx).repeat_interleave(N)
    rows_total = R * len(grid)

    def score(rows, shared=True):
        if shared:
            return model.score(seq0, x0, O0, generation_mask=gm, res_context_emb=res, pair_context_emb=pair, context_index=ci, t=grid, seed=7,
                               rows_per_launch=rows)
        return model.score(seq0, x0, O0, generation_mask=gm, res_context_emb=res_rep, pair_context_emb=pair_rep, t=grid, seed=7,
                           rows_per_launch=rows)

    if args.once:
        score(args.rows_per_launch[0])
        torch.cuda.synchronize()
        print(json.dumps({"rows": rows_total, "rows_per_launch": args.rows_per_launch[0]}))
        return
    res_rep, pair_rep = res[ci.cuda()], pair[ci.cuda()]
    ref = score(args.rows_per_launch[0])["per_step"]  # (warm-up; every variant must give these bits)

    sd = model._sched_on_device()
    tab = model._reverse_so3().struct()
    w = model.denoiser.hip_weights()
    samplers = {}
    for B in args.rows_per_launch:
        hd = model.denoiser.hip_dims(B, K)
        ws = _hip.workspace(lib.diffab_sample_workspace_bytes(C.byref(hd)))
        idx = torch.arange(B, device="cuda") % R
        st = (seq0[idx].clone(), x0[idx].clone(), O0[idx].clone(), gm[idx].contiguous(), res[ci.cuda()[idx]].contiguous(),
              pair[ci.cuda()[idx]].contiguous())
        samplers[B] = (hd, ws, st)

    def sample_steps(B):
        hd, ws, (s, x, O, m, rc, pc) = samplers[B]
        _hip.check(lib.diffab_sample_loop(C.byref(hd), C.byref(w.struct), C.byref(sd.struct), C.byref(tab), _hip.ptr(s), _hip.ptr(x), _hip.ptr(O),
                                          _hip.ptr(rc), _hip.ptr(pc), _hip.ptr(m), 11, 0, T, T - args.sampler_steps, _hip.ptr(ws), ws.numel(), 0,
                                          _hip.stream_ptr()), "diffab_sample_loop")

    variants = []
    for B in args.rows_per_launch:
        variants += [(f"score_shared_rows{B}", lambda B=B: score(B)), (f"score_per_design_ctx_rows{B}", lambda B=B: score(B, False)),
                     (f"sample_loop_B{B}", lambda B=B: sample_steps(B))]
    def same(a, b):  # bitwise, NaN where NaN (a residue frame at theta = pi has no defined scale_rot, as in the reference)
        return torch.equal(a.isnan(), b.isnan()) and torch.equal(a.nan_to_num(), b.nan_to_num())

    for name, fn in variants:  # warm-up (and the bits of every scoring form)
        out = fn()
        if name.startswith("score"):
            assert same(out["per_step"], ref), name
    runs = {name: [] for name, _ in variants}
    for rep in range(args.repeats):
        order = variants if rep % 2 == 0 else variants[::-1]
        for name, fn in order:
            runs[name].append(timed(fn))
    result = {"workload": {"contexts": n_ctx, "designs_per_context": N, "K": K, "grid_steps": len(grid), "draws": 1, "rows": rows_total,
                           "model": {k: dims[k] for k in ("D", "C", "NL", "H")}, "sampler_steps": args.sampler_steps,
                           "rows_not_finite": int((~torch.isfinite(ref)).any(-1).sum())},
              "variants": {}}
    for name, _ in variants:
        med, st = stats(runs[name])
        if name.startswith("score"):
            B = int(name.rsplit("rows", 1)[1])
            chunks = -(-rows_total // B)
            st.update(ms_per_chunk=round(med / chunks, 4), designs_per_s=round(R / (med / 1e3), 1), chunks=chunks)
        else:
            st.update(ms_per_step=round(med / args.sampler_steps, 4))
        result["variants"][name] = st
    txt = json.dumps(result, indent=1)
    print(txt)
    if args.json:
        with open(args.json, "w") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()
