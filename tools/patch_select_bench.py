#!/usr/bin/env python3
"""Cost of patch construction from whole complexes: patch.select + patch.gather of the reference batch fields (diffab_patch_select,
diffab_patch_gather), beside the same selection written with torch device ops (cdist, sort, cumsum, gather) in the same process, and one
encode_context call at the resulting K for scale.

B complexes of N residues (three blobs: heavy, light, antigen; one generated segment on the heavy chain), k = k_antigen = 128, K = 256.
Each case is warmed up, then timed --repeats times with device events around the whole case after a device synchronise; the cases
alternate inside each round.  The torch expression follows the four-step definition (forced residues by a -1 key, (key, index) order by
a stable sort); the share of index slots on which it agrees with the kernel is reported (torch.cdist's matrix-product form rounds
the keys differently).  Prints one JSON document (and writes it with --json).

    python tools/patch_select_bench.py [--b 256 --n 1024,4096 --repeats 20 --warmup 3] [--json OUT]
"""
import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "diffab-pytorch_amd"))

import torch  # noqa: E402

from sampler_bench_common import stats_ms, timed_repeats  # noqa: E402

FIELDS = ("seq_idx", "xyz", "orientations", "backbone_dihedrals", "atom_mask", "chain_idx", "residue_mask", "generation_mask", "antigen_mask")


def complexes(B, N, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    nh = nl = (3 * N) // 10
    chain = torch.tensor([1] * nh + [2] * nl + [3] * (N - nh - nl), device="cuda").repeat(B, 1)
    centre = torch.tensor([[0.0, 0, 0], [-12.0, 0, 0], [12.0, 0, 0], [0.0, 26, 0]], device="cuda")
    ca = centre[chain] + 9.0 * torch.randn(B, N, 3, device="cuda", generator=g)
    xyz = ca[:, :, None, :] + 1.5 * torch.randn(B, N, 15, 3, device="cuda", generator=g)
    xyz[:, :, 1] = ca
    gm = torch.zeros(B, N, dtype=torch.bool, device="cuda")
    start = torch.randint(5, nh - 20, (B,), device="cuda", generator=g)
    gm[torch.arange(B, device="cuda")[:, None], start[:, None] + torch.arange(10, device="cuda")] = True
    rm = torch.rand(B, N, device="cuda", generator=g) > 0.02
    return {"seq_idx": torch.randint(0, 20, (B, N), device="cuda", generator=g), "xyz": xyz,
            "orientations": torch.eye(3, device="cuda").expand(B, N, 3, 3).contiguous(),
            "backbone_dihedrals": torch.randn(B, N, 3, device="cuda", generator=g), "atom_mask": torch.ones(B, N, 15, device="cuda"),
            "chain_idx": chain, "residue_mask": rm, "generation_mask": gm, "antigen_mask": chain == 3}


def torch_select(batch, k, k_antigen):
    """The four-step definition with torch device ops.  Returns (index (B, k + k_antigen) ascending with -1 padding, count)."""
    ca, rm, ch = batch["xyz"][:, :, 1], batch["residue_mask"], batch["chain_idx"]
    gen = batch["generation_mask"] & rm
    B, N = gen.shape
    left = torch.zeros_like(gen)
    right = torch.zeros_like(gen)
    left[:, 1:] = gen[:, :-1] & (ch[:, :-1] == ch[:, 1:])
    right[:, :-1] = gen[:, 1:] & (ch[:, 1:] == ch[:, :-1])
    anchors = rm & ~gen & (left | right)
    anchors = torch.where(anchors.any(1, keepdim=True), anchors, gen)
    d = torch.cdist(ca, ca).square()  # (torch's matrix-product form: its keys differ from the definition's in the last bits)
    key = d.masked_fill(~anchors[:, None, :], float("inf")).amin(2)
    key = key.masked_fill(gen | anchors, -1.0).masked_fill(~rm, float("inf"))
    order = key.sort(dim=1, stable=True).indices  # (key, index) ascending
    live = rm.gather(1, order)
    sel = torch.zeros_like(gen)
    sel.scatter_(1, order[:, :k], live[:, :k])
    ag = batch["antigen_mask"].gather(1, order) & live
    sel.scatter_(1, order, sel.gather(1, order) | (ag & (ag.cumsum(1) <= k_antigen)))
    count = sel.sum(1)
    pos = torch.where(sel, torch.arange(N, device=sel.device).expand(B, N), torch.full_like(order, N)).sort(1).values[:, :k + k_antigen]
    return torch.where(pos < N, pos, torch.full_like(pos, -1)), count


def torch_gather(batch, index):
    rows = torch.arange(index.shape[0], device=index.device)[:, None]
    safe, live = index.clamp_min(0), index >= 0
    return {n: batch[n][rows, safe] * live.view(*live.shape, *([1] * (batch[n].dim() - 2))).to(batch[n].dtype) for n in FIELDS}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--b", type=int, default=256)
    ap.add_argument("--n", default="1024,4096")
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--json")
    args = ap.parse_args()
    from diffab_pytorch import DiffAb, _hip, patch, synthetic as syn

    _hip.lib()
    k = ka = 128
    res = {"device": torch.cuda.get_device_name(0), "B": args.b, "k": k, "k_antigen": ka, "cases": {}}
    g = None
    for N in (int(v) for v in args.n.split(",")):
        batch = complexes(args.b, N, seed=N)
        kw = dict(k=k, k_antigen=ka, antigen_mask=batch["antigen_mask"], chain_idx=batch["chain_idx"], residue_mask=batch["residue_mask"])
        sel = patch.select(batch["xyz"], batch["generation_mask"], **kw)
        want, count = torch_select(batch, k, ka)
        same = float((sel.index == want).float().mean())  # (not 1.0 where cdist's rounding reorders a near-tie at rank k)
        hip_select = lambda: patch.select(batch["xyz"], batch["generation_mask"], **kw)
        hip_both = lambda: patch.gather(batch, patch.select(batch["xyz"], batch["generation_mask"], **kw))
        th_select = lambda: torch_select(batch, k, ka)
        th_both = lambda: torch_gather(batch, torch_select(batch, k, ka)[0])
        cases = {"hip_select": hip_select, "hip_select_gather": hip_both, "torch_select": th_select, "torch_select_gather": th_both}
        runs = {n: [] for n in cases}
        for fn in cases.values():
            for _ in range(args.warmup):
                fn()
        for r in range(args.repeats):  # alternate the cases, the order reversed every other round
            for n in (list(cases) if r % 2 == 0 else list(cases)[::-1]):
                runs[n] += timed_repeats(cases[n], 1)
        res["cases"][f"N={N}"] = {"index_slots_equal_to_torch_expression": round(same, 6), **{n: stats_ms(v) for n, v in runs.items()}}
        g = patch.gather({n: v[:16] for n, v in batch.items()}, patch.PatchIndex(sel.index[:16], sel.mask[:16], sel.count[:16]))
    # for scale: one encode_context call on 16 of the gathered patches (K = 256), benchmark dimensions
    d = syn.BENCH_DIMS
    torch.manual_seed(0)
    model = DiffAb(d["D"], d["C"], d["NL"], d["DS"], d["PQ"], d["PV"], d["H"]).cuda()
    model.load_state_dict(syn.context_state_dict(d["D"], d["C"], 15, 32, seed=3), strict=False)
    enc = lambda: model._contexts_from_batch(g["seq_idx"], g["xyz"], g["orientations"], g["generation_mask"], g["residue_mask"],
                                             g["backbone_dihedrals"], None, None, g["atom_mask"], g["chain_idx"], g["residue_idx"], True, True)
    with torch.no_grad():
        for _ in range(args.warmup):
            enc()
        res["encode_context_16_patches_K256"] = stats_ms(timed_repeats(enc, args.repeats))
    print(json.dumps(res, indent=1))
    if args.json:
        with open(args.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
