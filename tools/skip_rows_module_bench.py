"""The reverse step at the benchmark geometry (B = 256, K = 128, six layers) against the last-layer row tiles the masks leave to run:
the sampler skips the last layer's attention items without a generated residue (DIFFAB_FLAG_ALL_ROWS: it does not).  One JSON line per
case, ms per step as the median of `repeats` blocks timed like bench.py's (wall clock around synchronised blocks of one C-ABI call):
  bench_masks            the benchmark's masks (one segment of 5-20 residues per patch), default flags
  bench_masks_all_rows   the same masks with DIFFAB_FLAG_ALL_ROWS (a build from before the flag ignores the bit: its only behaviour)
  full_mask              every residue generated, default flags (nothing to skip)
  tiles_N                N = 1, 2, 3, 4, 8 row tiles of EVERY patch hold one generated residue
usage: skip_rows_module_bench.py [steps] [warmup] [repeats] [json_out] ; DIFFAB_HIP_LIB selects the build (run once per build)"""
import ctypes as C
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "diffab-pytorch_amd"))
import torch  # noqa: E402

from diffab_pytorch import DiffAb, _hip, synthetic as syn  # noqa: E402

STEPS = int(sys.argv[1]) if len(sys.argv) > 1 else 100
WARMUP = int(sys.argv[2]) if len(sys.argv) > 2 else 5
REPEATS = int(sys.argv[3]) if len(sys.argv) > 3 else 5
OUT = sys.argv[4] if len(sys.argv) > 4 else None
B, K, NTILE = 256, 128, 8
lib = _hip.lib()
dims = dict(syn.BENCH_DIMS)
torch.manual_seed(0)
model = DiffAb(dims["D"], dims["C"], dims["NL"], dims["DS"], dims["PQ"], dims["PV"], dims["H"]).cuda()
inp = {k: v.cuda() for k, v in syn.patches(B, K, dims, seed=0, coord_sigma=10.0).items()}
hd, w = model.denoiser.hip_dims(B, K), model.denoiser.hip_weights()
sd_dev, tab = model._sched_on_device(), model._reverse_so3().struct()
ws = _hip.workspace(lib.diffab_sample_workspace_bytes(C.byref(hd)))
rc, pc = inp["res_context_emb"], inp["pair_context_emb"]


def ms_per_step(gm, flags):
    seq, x, O = inp["seq_idx"].clone(), inp["translations"].clone(), inp["orientations"].clone()
    _hip.check(lib.diffab_sample_init(_hip.ptr(seq), _hip.ptr(x), _hip.ptr(O), _hip.ptr(gm), 2024, 0, B, K, model.T, _hip.stream_ptr()), "init")

    def run(n, t_hi):
        _hip.check(lib.diffab_sample_loop(C.byref(hd), C.byref(w.struct), C.byref(sd_dev.struct), C.byref(tab), _hip.ptr(seq), _hip.ptr(x),
                                          _hip.ptr(O), _hip.ptr(rc), _hip.ptr(pc), _hip.ptr(gm), 2024, 0, t_hi, t_hi - n, _hip.ptr(ws),
                                          ws.numel(), flags, _hip.stream_ptr()), "sample_loop")
        return t_hi - n

    t = run(WARMUP, model.T)
    n = STEPS // REPEATS
    blocks = []
    for _ in range(REPEATS):
        if t < n:
            t = model.T
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        t = run(n, t)
        torch.cuda.synchronize()
        blocks.append(1e3 * (time.perf_counter() - t0) / n)
    assert bool(torch.isfinite(x).all())
    return sorted(blocks)[len(blocks) // 2], blocks


def tiles_mask(n):
    gm = torch.zeros(B, K, dtype=torch.bool)
    gm[:, [16 * j + 5 for j in range(n)]] = True
    return gm.cuda()


all_rows = getattr(_hip, "FLAG_ALL_ROWS", 8192)
cases = [("bench_masks", inp["generation_mask"], 0), ("bench_masks_all_rows", inp["generation_mask"], all_rows),
         ("full_mask", torch.ones(B, K, dtype=torch.bool, device="cuda"), 0)]
cases += [(f"tiles_{n}", tiles_mask(n), 0) for n in (1, 2, 3, 4, 8)]
lines = []
for name, gm, flags in cases:
    t = gm.view(B, NTILE, 16).any(-1).sum(1)
    med, blocks = ms_per_step(gm, flags)
    lines.append({"lib": _hip.LIB_PATH, "case": name, "flags": flags, "ms_per_step": round(med, 4), "blocks_ms": [round(b, 4) for b in blocks],
                  "tiles_with_generated_mean": round(float(t.float().mean()), 3), "tiles_with_generated_max": int(t.max()),
                  "steps": STEPS, "warmup": WARMUP})
    print(json.dumps(lines[-1]), flush=True)
if OUT:
    with open(OUT, "a") as fh:
        for ln in lines:
            fh.write(json.dumps(ln) + "\n")
