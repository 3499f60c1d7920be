"""Backbone refinement on the MI355X: diffab_refine_backbone through diffab_pytorch.refine.

The oracle is test_refine_host.py's refine_ref in float64, run on the SAME fp32 frames the kernel reads.  The allowance of every output
is 4 x the largest difference between refine_ref in float32 and in float64 on that same case - the rule's own rounding sensitivity; the
factor covers the kernel's different sine and cosine and the order of its float64 energy sums - with a floor of 2 fp32 ulps of the
largest |coordinate| of the case (2 ulps of 1 for O, 2 ulps relative for the energies).  The condition that this allowance stays below
1e-3 A and 1e-4 (O) is asserted on the oracle, not on the device.  Everything else here is exact: bits.
Measured on the MI355X (printed by test_refinement_against_the_oracle): see DESIGN.md section 4.18."""
import functools

import numpy as np
import pytest
import torch

from diffab_pytorch import metrics, refine, synthetic as syn
from sampler_support import hip, make_model, sample
from test_geometry_host import backbone_ref, tangle_chain_keys
from test_gpu_geometry import build_patch, same_bits
from test_refine_host import noisy, place, refine_ref

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("hip")]

EPS = float(np.finfo(np.float32).eps)
KINDS = ("native", "noisy03", "noisy1", "pushed")
SHAPES = [(3, 5, 70), (2, 3, 33), (1, 1, 1), (1, 2, 256), (2, 2, 256)]  # (G, N, K)
ROLES = {(3, 5, 70): ("one", "none", "loop"), (2, 3, 33): ("loop+ends", "one"), (1, 1, 1): ("single",), (1, 2, 256): ("loop+ends",),
         (2, 2, 256): ("loop", "loop")}
FIRST_KIND = {(3, 5, 70): 0, (2, 3, 33): 0, (1, 1, 1): 1, (1, 2, 256): 1, (2, 2, 256): 1}
# per patch, the first of 13 slots behind the loop that take the keys of test_geometry_host.tangle_chain_keys (and slot K - 1 with them):
# keys on which a 32-bit gap, the highest slot, a masked slot or another chain would link other residues.  These slots move.
TANGLED = {(2, 2, 256): (60, 75)}
OUTPUTS = ("translations", "orientations", "energy_before", "energy_after", "terms", "max_shift")


# ------------------------------------------------------------------ cases
def make_patch(rng, K, role):
    """Three NeRF chains with a residue_idx gap in each (test_gpu_geometry.build_patch); 'loop+ends' also generates slots 0 and K - 1."""
    if role == "single":
        return dict(translations=rng.normal(0.0, 3.0, (1, 3)).astype(np.float32), orientations=np.eye(3, dtype=np.float32)[None],
                    chain_idx=np.array([1]), residue_idx=np.array([5]), generation_mask=np.array([True]))
    p = build_patch(rng, K, 6, "loop" if role.startswith("loop") else role, True)
    if role == "loop+ends":
        p["generation_mask"][[0, K - 1]] = True
    return p


def design_of(rng, p, kind):
    t, R = p["translations"].astype(np.float64), p["orientations"].astype(np.float64)
    gen = p["generation_mask"]
    if gen.any() and kind == "noisy03":
        t, R = noisy(rng, t, R, gen, 0.3, 0.15)
    elif gen.any() and kind == "noisy1":
        t, R = noisy(rng, t, R, gen, 1.0, 0.5)
    elif gen.any() and kind == "pushed" and (p["chain_idx"] == 3).any():
        t = t.copy()
        t[gen] += 0.85 * (t[p["chain_idx"] == 3].mean(0) - t[gen].mean(0))  # into the antigen: the clash term acts
    return t.astype(np.float32), R.astype(np.float32)


@functools.lru_cache(maxsize=None)
def case(shape):
    G, N, K = shape
    rng = np.random.default_rng(7000 + 10 * K + N)
    patches = [make_patch(rng, K, role) for role in ROLES[shape]]
    rm = np.ones((G, K), bool)
    for g, at in enumerate(TANGLED.get(shape, ())):
        tangle_chain_keys(patches[g]["chain_idx"], patches[g]["residue_idx"], rm[g], at, K - 1)
        patches[g]["generation_mask"][at:at + 13] = patches[g]["generation_mask"][K - 1] = True
    stack = lambda k: np.stack([p[k] for p in patches])
    gen, chain, ridx = stack("generation_mask"), stack("chain_idx"), stack("residue_idx")
    if K > 1:  # the patch with the loop loses a generated and two context residues
        g = int(gen.sum(1).argmax())
        loop, ctx = np.flatnonzero(gen[g]), np.flatnonzero(~gen[g])
        rm[g, [loop[2], ctx[1], ctx[-2]]] = False
    kinds = [KINDS[(FIRST_KIND[shape] + g + r) % 4] for g in range(G) for r in range(N)]
    rows = [design_of(rng, patches[g], kinds[g * N + r]) for g in range(G) for r in range(N)]
    t, R = np.stack([r[0] for r in rows]), np.stack([r[1] for r in rows])
    cuda = lambda v: torch.from_numpy(np.ascontiguousarray(v)).cuda()
    designs = {"seq_idx": cuda(np.zeros((G * N, K), np.int64)), "translations": cuda(t), "orientations": cuda(R)}
    return dict(G=G, N=N, K=K, t=t, R=R, gen=gen, rm=rm, chain=chain, ridx=ridx, kinds=kinds, designs=designs, gen_d=cuda(gen),
                kw=dict(chain_idx=cuda(chain), residue_idx=cuda(ridx), residue_mask=cuda(rm), group_size=N))


@functools.lru_cache(maxsize=None)
def reference(shape, iterations, dtype):
    c = case(shape)
    return refine_ref(c["t"], c["R"], c["gen"], c["rm"], c["chain"], c["ridx"], refine.Refinement(iterations=iterations), dtype, c["N"])


@functools.lru_cache(maxsize=None)
def allowance(shape, iterations):
    """Per output: 4 x max |float32 run - float64 run|, and the floor: an array for the energies (relative), a number for the rest."""
    a, b = reference(shape, iterations, np.float32), reference(shape, iterations, np.float64)
    coord = float(np.abs(case(shape)["t"]).max())
    floor = {"translations": 2 * EPS * coord, "orientations": 2 * EPS, "max_shift": 2 * EPS * coord}
    out = {}
    for k in OUTPUTS:
        spread = 4.0 * float(np.abs(np.asarray(a[k], np.float64) - b[k]).max(initial=0.0))
        out[k] = np.maximum(spread, floor[k] if k in floor else 2 * EPS * np.abs(b[k]))
    return out


def run(c, options=None, designs=None, gen=None, **kw):
    out = refine.backbone(c["designs"] if designs is None else designs, c["gen_d"] if gen is None else gen, **dict(c["kw"], **kw), options=options)
    return {k: v.cpu().numpy() for k, v in out.items()}


# ------------------------------------------------------------------ 1. against the oracle
@pytest.mark.parametrize("iterations", [1, 7, 200])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_refinement_against_the_oracle(shape, iterations):
    c = case(shape)
    ref, allow = reference(shape, iterations, np.float64), allowance(shape, iterations)
    assert float(np.max(allow["translations"])) < 1e-3 and float(np.max(allow["orientations"])) < 1e-4, allow  # the oracle's own condition
    out = run(c, refine.Refinement(iterations=iterations))
    assert set(out) == set(OUTPUTS) | {"seq_idx"}
    worst = {}
    for k in OUTPUTS:
        assert out[k].dtype == np.float32 and out[k].shape == ref[k].shape, k
        err = np.abs(out[k].astype(np.float64) - ref[k])
        worst[k] = float(err.max(initial=0.0))
        print(f"refine {shape} iterations={iterations} {k}: max |dev - ref| = {worst[k]:.3g} (allowance {float(np.max(allow[k])):.3g})")
    for k in OUTPUTS:
        err = np.abs(out[k].astype(np.float64) - ref[k])
        assert (err <= allow[k]).all(), (k, worst[k], float(np.max(allow[k])))
    # fixed and masked-out residues: the input's bits, at every iteration count
    moving = np.repeat(c["gen"] & c["rm"], c["N"], axis=0)
    assert same_bits(out["translations"][~moving], c["t"][~moving]) and same_bits(out["orientations"][~moving], c["R"][~moving])
    if iterations == 200:
        O = out["orientations"].astype(np.float64)
        assert np.abs(O @ np.swapaxes(O, -1, -2) - np.eye(3)).max() < 1e-5
        noisy_rows = np.array([k != "native" for k in c["kinds"]]) & moving.any(1)
        assert (out["energy_after"][noisy_rows] <= out["energy_before"][noisy_rows]).all()
        if shape == (3, 5, 70):  # something happened: the shaken loops lost most of their energy, the pushed loop was in a clash
            kinds = np.array(c["kinds"])
            loop = np.arange(15) // 5 == 2
            shaken = loop & ((kinds == "noisy03") | (kinds == "noisy1"))
            assert (out["energy_before"][shaken] > 1.0).all() and (out["energy_after"][shaken] < 0.5 * out["energy_before"][shaken]).all()
            assert (reference(shape, 0, np.float64)["terms"][loop & (kinds == "pushed"), 3] > 0).all() and (out["max_shift"][loop] > 0.1).all()


# ------------------------------------------------------------------ 2. exact statements
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_zero_iterations_and_zero_weights_leave_every_bit(shape):
    c = case(shape)
    for options in (refine.Refinement(iterations=0), refine.Refinement(bond=0.0, angle=0.0, trans=0.0, clash=0.0),
                    refine.Refinement(iterations=3, bond=0.0, angle=0.0, trans=0.0, clash=0.0, tether=0.0, step=0.3)):
        out = run(c, options)
        assert same_bits(out["translations"], c["t"]) and same_bits(out["orientations"], c["R"]), options
        assert same_bits(out["energy_after"], out["energy_before"]) and (out["max_shift"] == 0).all(), options
    assert same_bits(run(c, refine.Refinement(iterations=0))["energy_before"], run(c)["energy_before"])


def test_a_row_a_patch_and_another_group_layout_are_bitwise_the_batch():
    c = case((3, 5, 70))
    N, full = c["N"], run(c)
    sub = lambda lo, hi: {k: v[lo:hi].contiguous() for k, v in c["designs"].items()}
    tabs = lambda g, n: dict(chain_idx=c["kw"]["chain_idx"][g:g + 1].repeat(n, 1), residue_idx=c["kw"]["residue_idx"][g:g + 1].repeat(n, 1),
                             residue_mask=c["kw"]["residue_mask"][g:g + 1].repeat(n, 1))
    part = run(c, designs=sub(2 * N, 3 * N), gen=c["gen_d"][2:3], **tabs(2, 1))  # the loop patch alone
    for k in OUTPUTS:
        assert same_bits(part[k], full[k][2 * N:3 * N]), k
    one = run(c, designs=sub(2 * N + 1, 2 * N + 2), gen=c["gen_d"][2:3], **tabs(2, 1), group_size=1)  # a noisy row alone
    for k in OUTPUTS:
        assert same_bits(one[k], full[k][2 * N + 1:2 * N + 2]), k
    # every row its own group: the masks and tables repeated per row
    rep = lambda v: v.repeat_interleave(N, dim=0)
    flat = run(c, gen=rep(c["gen_d"]), chain_idx=rep(c["kw"]["chain_idx"]), residue_idx=rep(c["kw"]["residue_idx"]),
               residue_mask=rep(c["kw"]["residue_mask"]), group_size=1)
    for k in OUTPUTS:
        assert same_bits(flat[k], full[k]), k
    assert (full["max_shift"][2 * N:] > 0).any()


def test_no_bonded_pull_across_the_gap_or_between_chains():
    """The loop of patch 2 spans the residue_idx gap of chain 1.  The slots on both sides of it follow the oracle (which links nothing
    there); with the gap closed in residue_idx they are pulled together and the result differs.  The loop ends in the middle of chain
    1: its neighbours on chains 2 and 3 are never linked, in the oracle and on the device alike."""
    shape = (3, 5, 70)
    c = case(shape)
    ref, allow = reference(shape, 200, np.float64), allowance(shape, 200)
    out = run(c)
    g, N, K = 2, c["N"], c["K"]
    n1 = K * 2 // 5
    left, right = n1 // 2 - 1, n1 // 2  # the gap of chain 1 lies between these slots (build_patch)
    assert c["ridx"][g, right] - c["ridx"][g, left] == 2 and c["gen"][g, left] and c["gen"][g, right] and c["rm"][g, [left, right]].all()
    rows = slice(g * N, (g + 1) * N)
    for k in ("translations", "orientations"):
        err = np.abs(out[k][rows][:, [left, right]].astype(np.float64) - ref[k][rows][:, [left, right]])
        assert (err <= allow[k]).all(), k
    closed = c["ridx"].copy()
    closed[g, right:n1] -= 1
    linked = run(c, residue_idx=torch.from_numpy(closed).cuda())
    moved = np.abs(linked["translations"][rows][:, [left, right]] - out["translations"][rows][:, [left, right]]).max(-1)
    shaken = np.array([k.startswith("noisy") for k in c["kinds"][rows]])  # (the native and the rigidly pushed loop are whole across the gap)
    assert shaken.sum() >= 2 and (moved[shaken] > 1e-3).all(), moved  # on both sides
    other = np.arange(3 * N) // N != g
    assert same_bits(linked["translations"][other], out["translations"][other])
    # between chains: numbering chain 2 so that it would continue chain 1 changes nothing while the chain labels differ
    cont = c["ridx"].copy()
    cont[g, n1:] += c["ridx"][g, n1 - 1] + 1 - c["ridx"][g, n1]
    assert cont[g, n1] == cont[g, n1 - 1] + 1 and c["chain"][g, n1] != c["chain"][g, n1 - 1]
    same = run(c, residue_idx=torch.from_numpy(cont).cuda())
    for k in OUTPUTS:
        assert same_bits(same[k], out[k]), k


# ------------------------------------------------------------------ 3. end to end
def test_sampled_designs_are_refined_and_scored():
    dims = dict(syn.BENCH_DIMS, NL=2)
    model = make_model(dims, 1)
    inp = {k: v.cuda() for k, v in syn.patches(2, 128, dims, seed=3, coord_sigma=8.0).items()}
    N = 4
    res = sample(model, {k: inp[k] for k in ("seq_idx", "translations", "orientations", "generation_mask", "res_context_emb", "pair_context_emb")},
                 seed=1, num_samples=N, steps=2)
    gm = inp["generation_mask"]
    out = refine.backbone(res, gm, group_size=N)
    assert out["seq_idx"] is res["seq_idx"] and out["translations"].is_cuda
    for k in OUTPUTS:
        assert torch.isfinite(out[k]).all(), k
    fixed = ~gm.repeat_interleave(N, dim=0)
    assert torch.equal(out["translations"][fixed], res["translations"][fixed]) and torch.equal(out["orientations"][fixed], res["orientations"][fixed])
    bb = metrics.backbone(out, gm, group_size=N)
    assert torch.isfinite(bb["max_peptide_deviation"]).all() and bb["phi"].shape == (2 * N, 128)
    assert (out["energy_after"] <= out["energy_before"]).all()


@pytest.mark.parametrize("shape", SHAPES[:2], ids=lambda s: "x".join(map(str, s)))
def test_refined_noisy_designs_have_the_oracles_bonds(shape):
    c = case(shape)
    ref, allow = reference(shape, 200, np.float64), allowance(shape, 200)
    out = refine.backbone(c["designs"], c["gen_d"], **c["kw"])
    got = metrics.backbone(out, c["gen_d"], **c["kw"])["max_peptide_deviation"].cpu().numpy().astype(np.float64)
    n, cc = place(ref["translations"], ref["orientations"], np.float64)
    want = backbone_ref(np.stack([n, ref["translations"], cc], axis=2), c["gen"], c["chain"], c["ridx"], c["rm"], c["N"])["max_peptide_deviation"]
    rows = np.array([k == "noisy03" for k in c["kinds"]])
    # |C - N| moves by at most the two atoms' errors: each a translation error plus a lever of at most 1.53 A times the error of a row of O
    slack = 2 * (float(np.max(allow["translations"])) + 1.53 * 3 * float(np.max(allow["orientations"])))
    print("max_peptide_deviation of the refined noisy-0.3 designs:", got[rows], "oracle:", want[rows], "slack:", slack)
    assert rows.any() and (got[rows] <= want[rows] + slack).all()
    if shape == (2, 3, 33):  # chains that do not run into each other: the bonds close (in the 70-residue patch the clash term holds them open)
        assert (want[rows] < 0.05).all()


def test_design_complex_refine_changes_only_the_generated_segment():
    from test_gpu_patch import complexes, make_model as complex_model

    model = complex_model(dict(syn.BENCH_DIMS, NL=2), 9)
    batch = complexes()
    kw = dict(seed=31, num_samples=4, t_start=12, t_stop=10)
    plain, none = model.design_complex(batch, **kw), model.design_complex(batch, refine=None, **kw)
    assert set(plain) == set(none)
    for k in ("seq_idx", "translations", "orientations"):
        assert torch.equal(plain[k], none[k]) and torch.equal(plain["complex"][k], none["complex"][k]), k
    done = model.design_complex(batch, refine=refine.Refinement(iterations=50), **kw)
    assert set(done) == set(plain) | {"energy_before", "energy_after", "terms", "max_shift"}
    assert torch.equal(done["seq_idx"], plain["seq_idx"]) and torch.equal(done["complex"]["seq_idx"], plain["complex"]["seq_idx"])
    assert (done["max_shift"] > 0).any() and (done["energy_after"] <= done["energy_before"]).all()
    for r in range(8):
        gen = (batch["generation_mask"][r // 4] & batch["residue_mask"][r // 4]).to(plain["complex"]["translations"].device)
        for k in ("translations", "orientations"):
            a, b = done["complex"][k][r], plain["complex"][k][r]
            assert torch.equal(a[~gen], b[~gen]), (r, k)
        assert not torch.equal(done["complex"]["translations"][r][gen], plain["complex"]["translations"][r][gen]), r
