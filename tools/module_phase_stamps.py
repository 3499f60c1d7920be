"""Diagnostic: the phases of the patch-resident module launch (ipa_persistent.hip) per patch and layer, from its phase stamps
(diffab_debug_set_module_stamps: four chip-clock stamps per (patch, layer) - projections start, attention start, to_out start, to_out
end - one per patch at the end of its heads and one at its start, in front of the embedding MLP; never enabled in production).  Runs reverse steps of the benchmark model (bench.py's geometry: B = 256, K = 128, six layers) and
prints the per-phase times of the last step's launch in microseconds.
usage: module_phase_stamps.py [steps] [json_out] ; DIFFAB_HIP_LIB selects the build (A/B of two builds: run this once per build)"""
import ctypes as C
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "diffab-pytorch_amd"))
import torch  # noqa: E402

from diffab_pytorch import DiffAb, _hip, synthetic as syn  # noqa: E402

STEPS = int(sys.argv[1]) if len(sys.argv) > 1 else 5
OUT = sys.argv[2] if len(sys.argv) > 2 else None
B, K, NTILE = 256, 128, 128 // 16
TICK_US = 0.01  # s_memrealtime: 100 MHz
lib = _hip.lib()
dims = dict(syn.BENCH_DIMS)
NL = dims["NL"]
torch.manual_seed(0)
model = DiffAb(dims["D"], dims["C"], NL, dims["DS"], dims["PQ"], dims["PV"], dims["H"]).cuda()
inp = {k: v.cuda() for k, v in syn.patches(B, K, dims, seed=0, coord_sigma=10.0).items()}
hd, w = model.denoiser.hip_dims(B, K), model.denoiser.hip_weights()
sd_dev, tab = model._sched_on_device(), model._reverse_so3().struct()
ws = _hip.workspace(lib.diffab_sample_workspace_bytes(C.byref(hd)))
gm, rc, pc = inp["generation_mask"], inp["res_context_emb"], inp["pair_context_emb"]
# [B NL NTILE items][8 waves][8] attention-item stamps, then [B][NL][4] phase stamps, then [B] the end of the heads and [B] the start of
# the patch (a build from before one of these stamps leaves it at zero: its heads / its embedding are then not reported)
stamps = torch.zeros(B * NL * NTILE * 64 + B * NL * 4 + 2 * B, dtype=torch.int64, device="cuda")
seq, x, O = inp["seq_idx"].clone(), inp["translations"].clone(), inp["orientations"].clone()
_hip.check(lib.diffab_sample_init(_hip.ptr(seq), _hip.ptr(x), _hip.ptr(O), _hip.ptr(gm), 2024, 0, B, K, model.T, _hip.stream_ptr()), "init")
lib.diffab_debug_set_module_stamps(_hip.ptr(stamps))
try:
    # flags 0: the sampler's own choice, the module launch at this batch (checked below: a per-layer path leaves the stamps at zero)
    _hip.check(lib.diffab_sample_loop(C.byref(hd), C.byref(w.struct), C.byref(sd_dev.struct), C.byref(tab), _hip.ptr(seq), _hip.ptr(x),
                                      _hip.ptr(O), _hip.ptr(rc), _hip.ptr(pc), _hip.ptr(gm), 2024, 0, model.T, model.T - STEPS, _hip.ptr(ws),
                                      ws.numel(), 0, _hip.stream_ptr()), "sample_loop")
    torch.cuda.synchronize()
finally:
    lib.diffab_debug_set_module_stamps(None)
ph = stamps[B * NL * NTILE * 64:B * NL * NTILE * 64 + B * NL * 4].view(B, NL, 4).cpu().double()
heads_end = stamps[B * NL * NTILE * 64 + B * NL * 4:B * NL * NTILE * 64 + B * NL * 4 + B].cpu().double()
patch_start = stamps[B * NL * NTILE * 64 + B * NL * 4 + B:].cpu().double()
if not bool((ph > 0).all()):
    sys.exit("module phase stamps missing: the module launch did not run for every (patch, layer)")
proj = (ph[:, :, 1] - ph[:, :, 0]) * TICK_US
attn = (ph[:, :, 2] - ph[:, :, 1]) * TICK_US
to_out = (ph[:, :, 3] - ph[:, :, 2]) * TICK_US
layer = (ph[:, :, 3] - ph[:, :, 0]) * TICK_US
res = {"lib": _hip.LIB_PATH, "B": B, "K": K, "NL": NL, "steps": STEPS}
print(f"{_hip.LIB_PATH}: last of {STEPS} steps, {B} patches x {NL} layers (us per patch-layer: mean | median | p10 - p90)")
for name, v in (("projections", proj), ("attention (8 items)", attn), ("to_out", to_out), ("dense (proj + to_out)", proj + to_out),
                ("layer", layer)):
    f = v.flatten()
    q = torch.quantile(f, torch.tensor([0.1, 0.5, 0.9], dtype=f.dtype))
    print(f"  {name:22s} {float(f.mean()):8.2f} | {float(q[1]):8.2f} | {float(q[0]):8.2f} - {float(q[2]):8.2f}")
    res[name] = {"mean": float(f.mean()), "median": float(q[1]), "p10": float(q[0]), "p90": float(q[2]),
                 "mean_by_layer": [float(m) for m in v.mean(0)]}
for name in ("projections", "to_out"):
    print(f"  {name} by layer: " + " ".join(f"{m:.2f}" for m in res[name]["mean_by_layer"]))
# the last layer's attention runs only for the row tiles with a generated residue (DIFFAB_FLAG_ALL_ROWS: for all): its time by tiles run
tiles_run = gm.view(B, NTILE, 16).any(-1).sum(1).cpu()
res["last_layer_attention_by_tiles_run"] = {}
for n in sorted(set(tiles_run.tolist())):
    sel = attn[:, -1][tiles_run == n]
    res["last_layer_attention_by_tiles_run"][str(n)] = {"patches": int(sel.numel()), "mean_us": float(sel.mean())}
    print(f"  last layer, {n} tiles with a generated residue: {int(sel.numel()):4d} patches, attention {float(sel.mean()):8.2f} us")
# the last layer, where the reverse sampler runs only what the update reads, per patch: mean and the slowest work-group
last = {"attention": attn[:, -1], "to_out": to_out[:, -1]}
if bool((heads_end > 0).all()):
    last["heads (end of to_out -> end of the work-group)"] = (heads_end - ph[:, -1, 3]) * TICK_US
if bool((patch_start > 0).all()):
    last["embedding (start of the patch -> layer 0's projections)"] = (ph[:, 0, 0] - patch_start) * TICK_US
res["last_layer"] = {}
for name, v in last.items():
    res["last_layer"][name] = {"mean_us": float(v.mean()), "max_us": float(v.max())}
    print(f"  {'' if name.startswith('embedding') else 'last layer '}{name}: mean {float(v.mean()):.2f} us, slowest {float(v.max()):.2f}")
own = (ph[:, -1, 3] - ph[:, 0, 0]) * TICK_US  # a work-group's module time (B <= #CUs: one patch each)
res["work_group_us"] = {"mean": float(own.mean()), "max": float(own.max()), "min": float(own.min())}
print(f"  work-group first stamp -> its last: mean {float(own.mean()):.1f} us, slowest {float(own.max()):.1f}, fastest {float(own.min()):.1f}")
launch = float(ph[:, -1, 3].max() - ph[:, 0, 0].min()) * TICK_US
res["first_stamp_to_last_us"] = launch
print(f"  first projections start -> last to_out end: {launch:.1f} us")
if bool((heads_end > 0).all()) and bool((patch_start > 0).all()):
    # the whole launch as its work-groups see it: the start of a patch (behind its start delay) to the end of its heads
    whole = (heads_end - patch_start) * TICK_US
    end = float(heads_end.max() - patch_start.min()) * TICK_US
    res["launch_us"] = {"own_mean": float(whole.mean()), "own_max": float(whole.max()), "end": end,
                        "last_start": float(patch_start.max() - patch_start.min()) * TICK_US}
    print(f"  patch start -> end of its heads: mean {float(whole.mean()):.1f} us, slowest {float(whole.max()):.1f}; "
          f"first start -> last finish (the launch's end): {end:.1f} us; last start {res['launch_us']['last_start']:.1f} us behind the first")
    # the launch's end by last-layer work: when the patches of each (items, live slabs) finish, behind the first start
    plan_items = []
    for b in range(B):
        rows_b = gm[b].nonzero().flatten().tolist()
        n, covered = 0, 0
        for i in rows_b:
            if i >= covered:
                covered = min(i, K - 16) + 16
                n += 1
        plan_items.append(n)
    items = torch.tensor(plan_items)
    fin = (heads_end - patch_start.min()) * TICK_US
    res["finish_by_items"] = {}
    for n in sorted(set(plan_items)):
        sel = fin[items == n]
        res["finish_by_items"][str(n)] = {"patches": int(sel.numel()), "mean_us": float(sel.mean()), "max_us": float(sel.max())}
        print(f"  {n} items in the last layer: {int(sel.numel()):4d} patches finish at mean {float(sel.mean()):8.1f} us, last {float(sel.max()):8.1f}")
if OUT:
    with open(OUT, "w") as fh:
        json.dump(res, fh, indent=1)
