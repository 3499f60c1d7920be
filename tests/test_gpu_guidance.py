"""Structure guidance on the MI355X: DiffAb.sample(guidance=...), guidance.structure_energy, diffab_sample_options.guidance and
diffab_guidance_energy.

The rule is DESIGN.md section 4.10 / include/diffab_hip.h.  The energy entry matches the float64 restatement of test_guidance_host.py at
K = 128, 256 and an odd K; one guided step is the unguided step minus the float64 Delta taken at the recorded x0_hat; guidance that must
change nothing is bitwise the unguided run; a guided run is bitwise the same on every launch form; and the potential does what it says
on designs whose generated residues start collapsed onto one point.
"""
import functools

import numpy as np
import pytest
import torch

from diffab_pytorch import _hip, synthetic as syn
from diffab_pytorch.diffusion import jump_coefficients
from diffab_pytorch.guidance import SampleGuidance, structure_energy
from sampler_support import CTX, assert_bitwise, hip, make_model, patches, rows, sample
from test_guidance_host import guidance_ref, planted_rows, shift_ref

pytestmark = pytest.mark.gpu
V = 21
GUIDE = SampleGuidance(clash=2.0, bond=1.0, max_shift=0.5)
patches = functools.partial(patches, chains=True)  # two chains, padded context residues, the generated residues collapsed onto one point


@pytest.fixture(scope="module")
def bench(hip):
    dims = dict(syn.BENCH_DIMS, NL=3)
    return dims, make_model(dims, 23)


# ------------------------------------------------------------------ 1. the energy entry against the float64 oracle
@pytest.mark.parametrize("K", [128, 256, 77])
def test_energy_against_float64(hip, K):
    B = 3
    p, gen, chain, ridx, rmask = planted_rows(B, K, seed=K, n_chains=3)
    gd = SampleGuidance(clash=1.3, bond=0.7, clash_distance=4.0, bond_length=3.8)
    out = structure_energy(torch.tensor(p, dtype=torch.float32).cuda(), torch.tensor(gen).cuda(), chain_idx=torch.tensor(chain),
                           residue_idx=torch.tensor(ridx), residue_mask=torch.tensor(rmask), guidance=gd, return_grad=True)
    ref = guidance_ref(p.astype(np.float32), gen, chain, ridx, rmask, 1.3, 4.0, 0.7, 3.8)
    assert (ref["n_clash"] > 0).all() and (ref["bond"] > 0).all()
    assert out["n_clash"].cpu().numpy().tolist() == ref["n_clash"].tolist()
    for k in ("clash", "bond", "max_bond_deviation"):
        got = out[k].cpu().double().numpy()
        assert np.abs(got - ref[k]).max() <= 1e-5 * np.abs(ref[k]).max() + 1e-5, (k, got, ref[k])
    g = out["grad"].cpu().double().numpy()
    assert np.abs(g - ref["grad"]).max() <= 1e-5 * np.abs(ref["grad"]).max(), np.abs(g - ref["grad"]).max()
    assert not g[~gen].any()


def test_energy_padded_residue_changes_nothing_and_rows_are_independent(hip):
    B, K = 4, 128
    p, gen, chain, ridx, rmask = planted_rows(B, K, seed=5)
    kw = dict(chain_idx=torch.tensor(chain), residue_idx=torch.tensor(ridx), residue_mask=torch.tensor(rmask),
              guidance=SampleGuidance(clash=1.0, bond=2.0), return_grad=True)
    x, gm = torch.tensor(p, dtype=torch.float32).cuda(), torch.tensor(gen).cuda()
    base = structure_energy(x, gm, **kw)
    moved = x.clone()
    for b in range(B):  # every padded residue onto a generated one
        pad, g0 = np.flatnonzero(~rmask[b]), np.flatnonzero(gen[b])[0]
        moved[b, pad] = x[b, g0]
    assert_bitwise(structure_energy(moved, gm, **kw), base, "padded")
    halves = [structure_energy(x[s], gm[s], **{k: (v[s] if torch.is_tensor(v) else v) for k, v in kw.items()})
              for s in (slice(0, 1), slice(1, B))]
    assert_bitwise({k: torch.cat([h[k] for h in halves]) for k in base}, base, "split")


# ------------------------------------------------------------------ 2. one guided step against the float64 Delta
def one_step_delta(model, inp, out_u, out_g, guide, beta):
    """Delta (B, K, 3) in float64 from the recorded x0_hat of the step, and the checks that only translations moved."""
    assert torch.equal(out_g["seq_idx"], out_u["seq_idx"]) and torch.equal(out_g["orientations"], out_u["orientations"])
    tr = out_g["trajectory"]
    assert_bitwise(tr, out_u["trajectory"], "the record is untouched")
    p = tr["pred_translations"][:, 0].cpu().double().numpy()
    ref = guidance_ref(p, inp["generation_mask"].cpu().numpy(), inp["chain_idx"].cpu().numpy(), inp["residue_idx"].cpu().numpy(),
                       inp["residue_mask"].cpu().numpy(), guide.clash, guide.clash_distance, guide.bond, guide.bond_length)
    return shift_ref(ref["grad"], beta, guide.max_shift)


@pytest.mark.parametrize("t, respaced", [(30, False), (1, False), (30, True), (6, True)])
def test_one_guided_step_is_the_update_minus_delta(bench, t, respaced):
    dims, model = bench
    inp = patches(3, 128, dims, seed=t)
    kw = dict(seed=9, t_start=t, init=False, trajectory=True, trajectory_predictions=True)
    if respaced:  # one jump t -> s with the plan's beta': to s = 20 (noise), or to 0 (the last step)
        s = 20 if t == 30 else 0
        kw.update(t_stop=s, steps=[t])
        beta = float(jump_coefficients(model.sched, torch.tensor([t]), s, model.beta_max)[0][t])
    else:
        kw.update(t_stop=t - 1)
        beta = float(model.sched["beta"][t])
    out_u = sample(model, inp, **kw)
    out_g = sample(model, inp, guidance=GUIDE, **kw)
    delta = one_step_delta(model, inp, out_u, out_g, GUIDE, beta)
    gm = inp["generation_mask"].cpu().numpy()
    assert np.abs(delta[gm]).max() > 1e-3, "the state must clash for this test to say anything"
    assert (np.sqrt((delta ** 2).sum(-1)) <= GUIDE.max_shift * (1 + 1e-9)).all()
    xu, xg = out_u["translations"].cpu().double().numpy(), out_g["translations"].cpu().double().numpy()
    err = np.abs((xg - xu) + delta).max()
    assert err <= 1e-5 * max(1.0, np.abs(xu).max()), err
    assert np.array_equal(xg[~gm], xu[~gm])


# ------------------------------------------------------------------ 3. guidance that must change nothing
FORMS = {"per_layer": dict(flags=_hip.FLAG_MULTI_LAUNCH), "module": dict(flags=_hip.FLAG_PERSISTENT_MODULE), "graph": dict(graph=True)}


@pytest.mark.parametrize("form", sorted(FORMS))
def test_neutral_guidance_is_bitwise_unguided(bench, form):
    dims, model = bench
    inp = patches(3, 128, dims, seed=3)
    kw = dict(seed=4, t_start=14, t_stop=0, init=False, **FORMS[form])
    plain = sample(model, inp, **kw)
    assert_bitwise(sample(model, inp, guidance=SampleGuidance(), **kw), plain, (form, "zero weights"))
    assert_bitwise(sample(model, inp, guidance=SampleGuidance(clash=5.0, bond=5.0, t_max=0), **kw), plain, (form, "t_max = 0"))
    guided = sample(model, inp, guidance=GUIDE, **kw)
    assert not torch.equal(guided["translations"], plain["translations"])


# ------------------------------------------------------------------ 4. a guided run on every launch form
def test_guided_run_per_layer_module_graph(bench):
    dims, model = bench
    inp = patches(3, 128, dims, seed=11)
    kw = dict(seed=2, t_start=16, t_stop=0, init=False, guidance=GUIDE, trajectory=3, trajectory_predictions=True)
    ref = sample(model, inp, flags=_hip.FLAG_MULTI_LAUNCH, **kw)
    assert_bitwise(sample(model, inp, flags=_hip.FLAG_PERSISTENT_MODULE, **kw), ref, "module")
    assert_bitwise(sample(model, inp, graph=True, **kw), ref, "graph")
    assert_bitwise(sample(model, inp, graph=True, flags=_hip.FLAG_PERSISTENT_MODULE, **kw), ref, "module graph")
    assert_bitwise(sample(model, inp, steps=16, graph=True, **kw), ref, "every step listed")


def test_guided_shards_samples_and_context_index(bench):
    dims, model = bench
    B, N = 3, 2
    inp = patches(B, 128, dims, seed=13)
    kw = dict(seed=6, t_start=12, t_stop=0, init=False, guidance=GUIDE)
    whole = sample(model, inp, **kw)
    for lo, hi in ((0, 1), (1, 3)):
        part = sample(model, rows(inp, torch.arange(lo, hi, device="cuda")), first_patch=lo, **kw)
        assert_bitwise(part, {k: v[lo:hi] for k, v in whole.items()}, ("shard", lo))
    many = sample(model, inp, num_samples=N, **kw)
    rep = rows(inp, torch.arange(B, device="cuda").repeat_interleave(N))
    assert_bitwise(many, sample(model, rep, **kw), "num_samples")
    ci = torch.tensor([2, 0, 2, 1])
    st = {k: v for k, v in rows(inp, ci.cuda()).items() if k not in CTX}
    got = sample(model, dict(st, res_context_emb=inp["res_context_emb"], pair_context_emb=inp["pair_context_emb"]), context_index=ci, **kw)
    assert_bitwise(got, sample(model, rows(inp, ci.cuda()), **kw), "context_index")


@pytest.mark.parametrize("case", ["structure", "optimize_from", "allowed_aa", "k256"])
def test_guided_modes_bitwise_across_forms(bench, case):
    dims, model = bench
    K = 256 if case == "k256" else 128
    inp = patches(2, K, dims, seed=17, collapse=case != "optimize_from")
    kw = dict(seed=3, guidance=GUIDE)
    if case == "structure":
        kw.update(mode="structure", t_start=10, init=False)
    elif case == "optimize_from":
        kw.update(optimize_from=8)
    elif case == "allowed_aa":
        allowed = torch.rand(K, V, generator=torch.Generator().manual_seed(1)) < 0.5
        allowed[:, 3] = True
        kw.update(allowed_aa=allowed, t_start=10, init=False)
    else:
        kw.update(t_start=10, init=False)
    ref = sample(model, inp, flags=_hip.FLAG_MULTI_LAUNCH, **kw)
    assert_bitwise(sample(model, inp, flags=_hip.FLAG_PERSISTENT_MODULE, **kw), ref, (case, "module"))
    assert_bitwise(sample(model, inp, graph=True, **kw), ref, (case, "graph"))
    plain = sample(model, inp, flags=_hip.FLAG_MULTI_LAUNCH, **{k: v for k, v in kw.items() if k != "guidance"})
    gm = inp["generation_mask"]
    assert torch.equal(ref["translations"][~gm], plain["translations"][~gm])
    assert not torch.equal(ref["translations"][gm], plain["translations"][gm])
    if case == "structure":
        assert torch.equal(ref["seq_idx"], inp["seq_idx"])


# ------------------------------------------------------------------ 5. what the potential does
def test_guidance_removes_clashes_and_restores_bonds(bench):
    """Generated residues start collapsed onto one point at t = 20 (init=False), same seeds with and without clash + bond guidance.
    Measured on the MI355X with these inputs: clash sum 1768 -> 205 (0.12), bond sum 3308 -> 725 (0.22), clashing pairs 790 -> 360.
    The bound is "at most half" for both sums.  (Over many steps the moved translations feed back into the denoiser, so the sequence and
    orientations of the two runs differ too; one step leaves them bitwise, section 2.)  A statement about the potential, not about
    design quality (the weights are untrained)."""
    dims, model = bench
    inp = patches(8, 128, dims, seed=29)
    kw = dict(seed=12, t_start=20, t_stop=0, init=False)
    guide = SampleGuidance(clash=10.0, bond=10.0, max_shift=1.0)
    plain = sample(model, inp, **kw)
    guided = sample(model, inp, guidance=guide, **kw)
    tabs = dict(chain_idx=inp["chain_idx"], residue_idx=inp["residue_idx"], residue_mask=inp["residue_mask"])
    e0 = structure_energy(plain["translations"], inp["generation_mask"], **tabs)
    e1 = structure_energy(guided["translations"], inp["generation_mask"], **tabs)
    c0, c1, b0, b1 = (float(e[k].sum()) for e, k in ((e0, "clash"), (e1, "clash"), (e0, "bond"), (e1, "bond")))
    print(f"\nguidance effect: clash sum {c0:.1f} -> {c1:.1f} ({c1 / c0:.3f}), n_clash {int(e0['n_clash'].sum())} -> "
          f"{int(e1['n_clash'].sum())}, bond sum {b0:.1f} -> {b1:.1f} ({b1 / b0:.3f}), max bond deviation "
          f"{float(e0['max_bond_deviation'].max()):.2f} -> {float(e1['max_bond_deviation'].max()):.2f}")
    assert c0 > 0 and c1 <= 0.5 * c0
    assert b0 > 0 and b1 <= 0.5 * b0
