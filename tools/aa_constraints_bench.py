#!/usr/bin/env python3
"""Reverse-sampler cost of the sequence constraints (diffab_sample_options.allowed), ROWS patches, K = 128, benchmark model, one context per row
(256 rows fill the chip: the patch-resident module launch, what bench.py times).

Cases, alternating inside one process (the order reversed every other round), each a --warmup-step untimed call and then ONE call of
--steps steps from t = T on the re-initialised state, bracketed by hipEvents after a device synchronise (bench.py's timed block):
  free     diffab_sample_loop (no mask)
  all      diffab_sample_loop_ex, option `allowed`, with every class allowed (the masked code, bitwise the free result - checked)
  no_cmx   the same with Cys, Met and UNK forbidden on every residue
Reported per case: median / min / max ms per step over --repeats rounds.  Prints one JSON document (and writes it with --json).
--cases runs a subset (a kernel trace per case: rocprofv3 --kernel-trace --stats -- python tools/aa_constraints_bench.py --cases free).

    python tools/aa_constraints_bench.py [--steps 100 --warmup 5 --repeats 5 --rows 256 --k 128] [--cases free,all,no_cmx] [--json OUT]
"""
import torch

from sampler_bench_common import SamplerRun, bench_model, case_names, emit, parser, rounds, stats

CASES = ("free", "all", "no_cmx")


def main():
    args = parser(CASES).parse_args()
    R, K = args.rows, args.k
    names = case_names(args, CASES)

    from diffab_pytorch import _hip, io
    from diffab_pytorch.diffab_pytorch import _pack_allowed_aa

    dims, model = bench_model()
    T = model.T
    if not (1 <= args.steps <= T and 0 <= args.warmup <= T and args.repeats >= 1):
        raise SystemExit(f"need 1 <= --steps <= T = {T}, 0 <= --warmup <= T and --repeats >= 1")
    run = SamplerRun(model, dims, R, K)
    gm = run.gm
    V = model.denoiser.dims["V"]
    masks = {"free": None, "all": _pack_allowed_aa(torch.ones(R, K, V, dtype=torch.bool, device="cuda")),
             "no_cmx": _pack_allowed_aa(io.allowed_aa_mask(K, exclude="CMX", V=V).cuda().expand(R, K, V))}

    def init(words):
        run.reset()
        _hip.check(run.lib.diffab_sample_init_ex(*run.state_ptrs(), run.seed, 0, R, K, T, 0, _hip.ptr(words), _hip.stream_ptr()),
                   "sample_init_ex")

    def loop(words, t_start, t_stop):
        run.loop(t_start, t_stop, None if words is None else dict(allowed=_hip.ptr(words)))

    runs = {n: [] for n in names}
    final = {}
    for _, n in rounds(names, args.repeats):
        words = masks[n]
        init(words)
        if args.warmup:
            loop(words, T, T - args.warmup)
        init(words)
        runs[n].append(run.timed(lambda: loop(words, T, T - args.steps)) / args.steps)
        final[n] = run.seq.clone()
    out = {"what": "reverse sampler with sequence constraints: ms per step, unconstrained / all-true mask / C, M, UNK excluded",
           "rows": R, "k": K, "T": T, "steps": args.steps, "warmup": args.warmup, "repeats": args.repeats,
           "device": torch.cuda.get_device_name(), "cases": []}
    if "free" in final and "all" in final:
        out["all_true_bitwise_free"] = bool(torch.equal(final["free"], final["all"]))
    if "no_cmx" in final:
        out["no_cmx_forbidden_tokens"] = int(torch.isin(final["no_cmx"][gm], torch.tensor([4, 12, 20], device="cuda")).sum())
    ref = stats(runs[names[0]])[0]
    for n in names:
        med, st = stats(runs[n])
        out["cases"].append({"case": n, "ms_per_step": st, f"vs_{names[0]}_pct": round(100 * (med - ref) / ref, 2)})
    emit(out, args.json)


if __name__ == "__main__":
    main()
