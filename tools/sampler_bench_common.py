"""What the sampler's bench tools share: the command line, the benchmark model and its seeded device inputs, a runner that owns the state, the
workspace, diffab_sample_init and the diffab_sample_loop_ex call, the hipEvent timing, the alternating rounds, the statistics and the
JSON result.  A tool is run as `python tools/x_bench.py`, so this directory is on sys.path: `from sampler_bench_common import ...`.

A new sampler feature's bench starts from here: its docstring, its cases (an options struct and a table per case) and its own result keys.
"""
import argparse
import ctypes as C
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "diffab-pytorch_amd"))

import torch  # noqa: E402


def parser(cases=None, steps=True):
    """--steps --warmup --repeats --rows --k [--cases] --json; a tool adds its own flags before parse_args()"""
    ap = argparse.ArgumentParser()
    if steps:
        ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--rows", type=int, default=256, help="patches (state rows) per call")
    ap.add_argument("--k", type=int, default=128)
    if cases:
        ap.add_argument("--cases", default=",".join(cases), help=f"comma-separated subset of {','.join(cases)}")
    ap.add_argument("--json", help="also write the result here")
    return ap


def case_names(args, cases):
    names = args.cases.split(",")
    if not names or any(n not in cases for n in names):
        raise SystemExit(f"--cases: expected a comma-separated subset of {','.join(cases)}")
    return names


def random_rotations(n, g):
    q = torch.randn(n, 4, device="cuda", generator=g)
    w, x, y, z = (q / q.norm(dim=-1, keepdim=True)).unbind(-1)
    return torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w),
                        2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w),
                        2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)], -1).view(n, 3, 3)


def stats(runs, nd=4):
    """(median, {"median", "min", "max", "spread_pct", "runs"}) of per-round figures, rounded to nd digits"""
    s = sorted(runs)
    med = s[len(s) // 2]
    return med, {"median": round(med, nd), "min": round(s[0], nd), "max": round(s[-1], nd),
                 "spread_pct": round(100 * (s[-1] - s[0]) / med, 2), "runs": [round(r, nd) for r in runs]}


def stats_ms(runs, scale=1.0):
    """{"median_ms", "min_ms", "max_ms", "repeats"} of event times in ms, each multiplied by scale"""
    s = sorted(r * scale for r in runs)
    return {"median_ms": round(s[len(s) // 2], 4), "min_ms": round(s[0], 4), "max_ms": round(s[-1], 4), "repeats": len(s)}


def timed(fn):
    """ms of fn() between two hipEvents, after a device synchronise (bench.py's timed block)"""
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def timed_repeats(fn, repeats):
    return [timed(fn) for _ in range(repeats)]


def rounds(names, repeats):
    """(round, name): every name once per round, the order reversed every other round"""
    for rep in range(repeats):
        for n in (names if rep % 2 == 0 else names[::-1]):
            yield rep, n


def emit(out, path=None):
    print(json.dumps(out))
    if path:
        with open(path, "w") as f:
            json.dump(out, f, indent=1)


def bench_model():
    """(dims, model): bench.py's model - the benchmark dims, default init of the boundary module under torch.manual_seed(0)"""
    from diffab_pytorch import DiffAb, synthetic as syn

    dims = dict(syn.BENCH_DIMS)
    torch.manual_seed(0)
    return dims, DiffAb(dims["D"], dims["C"], dims["NL"], dims["DS"], dims["PQ"], dims["PV"], dims["H"]).cuda()


def device_inputs(dims, R, K, n_ctx=None, group=1):
    """Seeded inputs on the device, drawn in this order from Generator("cuda").manual_seed(0): res, pair (n_ctx contexts, one per row by
    default), seq0, x0, O0 (R rows), then start and length of one generated segment of 5..20 residues per group of `group` rows."""
    n_ctx = R if n_ctx is None else n_ctx
    g = torch.Generator(device="cuda").manual_seed(0)
    res = torch.randn(n_ctx, K, dims["D"], device="cuda", generator=g)
    pair = torch.randn(n_ctx, K, K, dims["C"], device="cuda", generator=g)
    seq0 = torch.randint(0, 20, (R, K), device="cuda", generator=g)
    x0 = 10 * torch.randn(R, K, 3, device="cuda", generator=g)
    O0 = random_rotations(R * K, g).view(R, K, 3, 3).contiguous()
    start = torch.randint(0, K - 20, (R // group, 1), device="cuda", generator=g)
    length = torch.randint(5, 21, (R // group, 1), device="cuda", generator=g)
    if group > 1:
        start, length = start.repeat_interleave(group, dim=0), length.repeat_interleave(group, dim=0)
    pos = torch.arange(K, device="cuda")[None]
    gm = ((pos >= start) & (pos < start + length)).contiguous()
    return dict(res=res, pair=pair, seq0=seq0, x0=x0, O0=O0, gm=gm)


class SamplerRun:
    """R rows at length K of the benchmark model, one context per row: the inputs, the live state seq / x / O, the workspace, the
    re-initialisation and the diffab_sample_loop_ex call, with the options and the reverse table chosen per call."""
    seed = 2024

    def __init__(self, model, dims, R, K, group=1):
        from diffab_pytorch import _hip

        self._hip, self.lib, self.model, self.R, self.K, self.T = _hip, _hip.lib(), model, R, K, model.T
        for k, v in device_inputs(dims, R, K, group=group).items():
            setattr(self, k, v)
        self.hd = model.denoiser.hip_dims(R, K)
        self.w = model.denoiser.hip_weights()
        self.sd = model._sched_on_device()
        self.tab = model._reverse_so3().struct()
        self.ws = _hip.workspace(self.lib.diffab_sample_workspace_bytes(C.byref(self.hd)))
        self.seq, self.x, self.O = self.seq0.clone(), self.x0.clone(), self.O0.clone()

    def state_ptrs(self):
        P = self._hip.ptr
        return P(self.seq), P(self.x), P(self.O), P(self.gm)

    def reset(self):
        self.seq.copy_(self.seq0), self.x.copy_(self.x0), self.O.copy_(self.O0)

    def init(self):
        _hip = self._hip
        self.reset()
        _hip.check(self.lib.diffab_sample_init(*self.state_ptrs(), self.seed, 0, self.R, self.K, self.T, _hip.stream_ptr()), "sample_init")

    def loop(self, t_start, t_stop, options=None, tab=None, flags=0):
        """diffab_sample_loop_ex from t_start to t_stop; options: the keywords of _hip.SampleOptions (None: no options struct); tab: the
        reverse table's struct (None: the model's)"""
        _hip = self._hip
        opt = None if options is None else C.byref(_hip.SampleOptions(**options))
        _hip.check(self.lib.diffab_sample_loop_ex(C.byref(self.hd), C.byref(self.w.struct), C.byref(self.sd.struct),
                                                  C.byref(self.tab if tab is None else tab), _hip.ptr(self.seq), _hip.ptr(self.x),
                                                  _hip.ptr(self.O), _hip.ptr(self.res), _hip.ptr(self.pair), _hip.ptr(self.gm), self.seed, 0,
                                                  t_start, t_stop, _hip.ptr(self.ws), self.ws.numel(), flags, opt, _hip.stream_ptr()),
                   "diffab_sample_loop_ex")

    def timed(self, fn):
        """timed(fn), then the check that the state is finite (outside the events)"""
        ms = timed(fn)
        if not (torch.isfinite(self.x).all() and torch.isfinite(self.O).all()):
            raise SystemExit("non-finite state")
        return ms

    def final(self):
        return {"seq_idx": self.seq.clone(), "translations": self.x.clone(), "orientations": self.O.clone()}
