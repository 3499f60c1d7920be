"""CPU: the host side of structure guidance (DiffAb.sample(guidance=...), guidance.structure_energy) - a float64 restatement of the
potential and its gradient checked against torch autograd and central differences, the argument checks that happen before any library
call, and the C-ABI entries and struct layout.

The rule is DESIGN.md section 4.10 / include/diffab_hip.h (diffab_sample_options.guidance, diffab_guidance_energy)."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

import sampler_support as support
from diffab_pytorch import _hip
from diffab_pytorch.guidance import SampleGuidance, structure_energy
from sampler_support import ReachedTheLibrary, inputs, refuse_library, stand_in

V, T = 21, 10
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------ the float64 restatement (shared with test_gpu_guidance.py)
def pair_masks(gen, chain, ridx, rmask):
    """(B, K, K) active pairs (mask on both, at least one generated, i != j) and bonded pairs (same chain, residue_idx one apart)."""
    gen, rmask = np.asarray(gen, bool), np.asarray(rmask, bool)
    chain, ridx = np.asarray(chain, np.int64), np.asarray(ridx, np.int64)
    K = gen.shape[-1]
    act = rmask[:, :, None] & rmask[:, None, :] & (gen[:, :, None] | gen[:, None, :]) & ~np.eye(K, dtype=bool)[None]
    bonded = (chain[:, :, None] == chain[:, None, :]) & (np.abs(ridx[:, :, None] - ridx[:, None, :]) == 1)
    return act, bonded


def guidance_ref(p, gen, chain, ridx, rmask, w_clash=1.0, d0=3.8, w_bond=1.0, L=3.8):
    """float64 terms of the potential at p (B, K, 3): per row the unweighted clash and bond sums over unordered pairs, the clash count,
    the largest |d - L| over bonded pairs (0 without one), and the weighted gradient (B, K, 3) of the generated residues (a pair with
    d < 1e-6 contributes none)."""
    p = np.asarray(p, np.float64)
    act, bonded = pair_masks(gen, chain, ridx, rmask)
    diff = p[:, :, None, :] - p[:, None, :, :]
    d = np.sqrt((diff ** 2).sum(-1))
    clash_on = act & ~bonded & (d < d0)
    bond_on = act & bonded
    upper = np.triu(np.ones(d.shape[-2:], dtype=bool), 1)[None]
    clash = np.where(clash_on & upper, (d0 - d) ** 2, 0.0).sum((1, 2))
    bond = np.where(bond_on & upper, (d - L) ** 2, 0.0).sum((1, 2))
    n_clash = (clash_on & upper).sum((1, 2))
    max_dev = np.where(bond_on & upper, np.abs(d - L), 0.0).max((1, 2))
    coef = np.where(clash_on, -2.0 * w_clash * (d0 - d), 0.0) + np.where(bond_on, 2.0 * w_bond * (d - L), 0.0)
    coef = np.where(d >= 1e-6, coef / np.where(d > 0, d, 1.0), 0.0)
    grad = (coef[..., None] * diff).sum(2) * np.asarray(gen, bool)[..., None]
    return {"clash": clash, "bond": bond, "n_clash": n_clash, "max_bond_deviation": max_dev, "grad": grad}


def shift_ref(grad, beta, max_shift):
    """Delta = beta g, scaled to length max_shift where longer (float64)."""
    s = float(beta) * np.asarray(grad, np.float64)
    if np.isinf(max_shift):
        return s
    n = np.sqrt((s ** 2).sum(-1, keepdims=True))
    return np.where(n > max_shift, s * (max_shift / np.where(n > 0, n, 1.0)), s)


def planted_rows(B, K, seed, n_chains=2):
    """Random rows with planted clashes and bonds: two or more chains, gaps in residue_idx, padded residues (residue_mask False) and a
    generated stretch per row.  Chain-consecutive residues sit near 3.8 A apart, a few generated residues are pulled onto others."""
    rng = np.random.default_rng(seed)
    chain = np.sort(rng.integers(0, n_chains, (B, K)), axis=1)
    ridx = np.cumsum(rng.choice([1, 1, 1, 1, 2, 5], (B, K)), axis=1)  # gaps
    p = np.zeros((B, K, 3))
    for b in range(B):
        pos = rng.normal(0.0, 12.0, 3)
        for k in range(K):
            if k and chain[b, k] != chain[b, k - 1]:
                pos = rng.normal(0.0, 12.0, 3)
            step = rng.normal(0.0, 1.0, 3)
            pos = pos + step / np.linalg.norm(step) * rng.uniform(3.0, 4.6)
            p[b, k] = pos
    gen = np.zeros((B, K), bool)
    for b in range(B):
        s0 = rng.integers(0, K - K // 4)
        gen[b, s0:s0 + K // 4] = True
    for b in range(B):  # planted clashes: generated residues onto random partners, a little off
        for k in rng.choice(np.flatnonzero(gen[b]), min(4, int(gen[b].sum())), replace=False):
            p[b, k] = p[b, rng.integers(0, K)] + rng.normal(0.0, 1.0, 3)
    rmask = rng.random((B, K)) > 0.1
    rmask[:, -3:] = False  # a padded tail
    return p, gen, chain.astype(np.int32), ridx.astype(np.int32), rmask


def torch_energy(p, gen, chain, ridx, rmask, w_clash, d0, w_bond, L):
    act, bonded = (torch.as_tensor(m) for m in pair_masks(gen, chain, ridx, rmask))
    diff = p[:, :, None, :] - p[:, None, :, :]
    d = (diff.square().sum(-1) + torch.eye(p.shape[1], dtype=p.dtype)[None]).sqrt()  # (the diagonal is masked out; keeps sqrt smooth)
    clash = torch.where(act & ~bonded, (d0 - d).clamp_min(0.0).square(), torch.zeros_like(d))
    bond = torch.where(act & bonded, (d - L).square(), torch.zeros_like(d))
    return 0.5 * (w_clash * clash.sum() + w_bond * bond.sum())  # both orders of every pair


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_oracle_against_autograd(seed):
    p, gen, chain, ridx, rmask = planted_rows(3, 40, seed, n_chains=2 + seed)
    wc, d0, wb, L = 1.7, 3.8, 0.6, 3.8
    ref = guidance_ref(p, gen, chain, ridx, rmask, wc, d0, wb, L)
    assert ref["n_clash"].min() > 0 and ref["bond"].min() > 0  # the planted terms are there
    pt = torch.tensor(p, dtype=torch.float64, requires_grad=True)
    U = torch_energy(pt, gen, chain, ridx, rmask, wc, d0, wb, L)
    u = U.item()
    assert abs(u - float((wc * ref["clash"] + wb * ref["bond"]).sum())) < 1e-9 * max(1.0, u)
    (g,) = torch.autograd.grad(U, pt)
    g = g.numpy() * gen[..., None]
    assert np.abs(g - ref["grad"]).max() < 1e-9 * max(1.0, np.abs(g).max())


def test_oracle_against_central_differences():
    p, gen, chain, ridx, rmask = planted_rows(2, 32, 7)
    wc, d0, wb, L = 1.0, 3.8, 2.0, 3.8
    ref = guidance_ref(p, gen, chain, ridx, rmask, wc, d0, wb, L)

    def U(q):
        r = guidance_ref(q, gen, chain, ridx, rmask, wc, d0, wb, L)
        return wc * r["clash"] + wb * r["bond"]

    h = 1e-6
    for b, k in zip(*np.nonzero(gen)):
        for c in range(3):
            qp, qm = p.copy(), p.copy()
            qp[b, k, c] += h
            qm[b, k, c] -= h
            num = (U(qp)[b] - U(qm)[b]) / (2 * h)
            assert abs(num - ref["grad"][b, k, c]) < 1e-5 * max(1.0, abs(num)), (b, k, c, num, ref["grad"][b, k, c])


def test_oracle_pair_rules():
    """Two residues: bonded only on the same chain one index apart; a padded or an all-context pair counts nothing; d < 1e-6 no gradient."""
    p = np.array([[[0.0, 0.0, 0.0], [2.0, 0.0, 0.0]]])
    one = lambda **kw: guidance_ref(p, kw.get("gen", [[True, False]]), kw.get("chain", [[0, 0]]), kw.get("ridx", [[5, 6]]),
                                    kw.get("rmask", [[True, True]]))
    r = one()
    assert r["bond"][0] == pytest.approx(1.8 ** 2) and r["clash"][0] == 0 and r["max_bond_deviation"][0] == pytest.approx(1.8)
    assert r["grad"][0, 0, 0] == pytest.approx(2 * (2.0 - 3.8) * -1.0) and r["grad"][0, 1].tolist() == [0, 0, 0]
    r = one(chain=[[0, 1]])
    assert r["clash"][0] == pytest.approx(1.8 ** 2) and r["n_clash"][0] == 1 and r["bond"][0] == 0
    r = one(ridx=[[5, 7]])
    assert r["clash"][0] == pytest.approx(1.8 ** 2) and r["bond"][0] == 0
    for kw in (dict(rmask=[[True, False]]), dict(gen=[[False, False]])):
        r = one(**kw)
        assert r["clash"][0] == r["bond"][0] == 0 and not r["grad"].any()
    r = guidance_ref(np.zeros((1, 2, 3)), [[True, True]], [[0, 1]], [[0, 0]], [[True, True]])
    assert r["clash"][0] == pytest.approx(3.8 ** 2) and not r["grad"].any()


def test_shift_cap():
    g = np.array([[[3.0, 4.0, 0.0], [0.3, 0.4, 0.0]]])
    s = shift_ref(g, 0.5, 1.0)
    assert np.allclose(s[0, 0], [0.6, 0.8, 0.0]) and np.allclose(s[0, 1], [0.15, 0.2, 0.0])
    assert np.allclose(shift_ref(g, 0.5, np.inf), 0.5 * g)


# ------------------------------------------------------------------ argument checks before the library
@pytest.fixture(scope="module")
def model():
    return stand_in(T=T)


@pytest.fixture(autouse=True)
def no_library(monkeypatch):
    refuse_library(monkeypatch)


def call(model, B=2, K=16, **kw):
    return support.call(model, inputs(B, K), **kw)


@pytest.mark.parametrize("bad, match", [
    ({"clash": 1.0}, "must be a guidance.SampleGuidance"), (1.0, "must be a guidance.SampleGuidance"),
    (SampleGuidance(clash=-1.0), "clash weight must be a finite number >= 0"), (SampleGuidance(bond=float("nan")), "bond weight"),
    (SampleGuidance(clash=float("inf")), "clash weight"), (SampleGuidance(bond=True), "bond weight"),
    (SampleGuidance(clash="1"), "clash weight"), (SampleGuidance(clash_distance=0.0), "clash_distance must be a finite number > 0"),
    (SampleGuidance(bond_length=-3.8), "bond_length must be"), (SampleGuidance(bond_length=float("inf")), "bond_length must be"),
    (SampleGuidance(max_shift=0.0), "max_shift must be > 0"), (SampleGuidance(max_shift=float("nan")), "max_shift must be > 0"),
    (SampleGuidance(t_max=-1), "t_max must be None or an int in \\[0, T = 10\\]"), (SampleGuidance(t_max=11), "t_max must be"),
    (SampleGuidance(t_max=2.0), "t_max must be"), (SampleGuidance(t_max=True), "t_max must be"),
])
def test_bad_guidance_is_rejected(model, bad, match):
    with pytest.raises(ValueError, match=match):
        call(model, guidance=bad)


@pytest.mark.parametrize("kw, match", [
    (dict(chain_idx=torch.zeros(3, 16, dtype=torch.long)), "chain_idx \\(3, 16\\) does not broadcast to the rows \\(2, 16\\)"),
    (dict(chain_idx=torch.zeros(17, dtype=torch.long)), "chain_idx \\(17,\\) does not broadcast"),
    (dict(residue_idx=torch.arange(16).float()), "integer residue_idx"), (dict(chain_idx=torch.zeros(16, dtype=torch.bool)), "integer chain_idx"),
    (dict(residue_mask=torch.ones(2, 15, dtype=torch.bool)), "residue_mask \\(2, 15\\) does not broadcast"),
    (dict(residue_mask=torch.ones(16)), "integer residue_mask"), (dict(residue_idx=torch.zeros(1, 2, 16, dtype=torch.long)), "\\(K,\\) or \\(rows, K\\)"),
    (dict(residue_idx=torch.full((16,), 2 ** 31)), "fit in int32"),
    (dict(mode="fixed_backbone"), "mode='fixed_backbone' keeps as given"),
    (dict(num_samples=3, chain_idx=torch.zeros(6, 16, dtype=torch.long)), "chain_idx \\(6, 16\\) does not broadcast to the rows \\(2, 16\\)"),
])
def test_bad_tables_and_modes_are_rejected(model, kw, match):
    with pytest.raises(ValueError, match=match):
        call(model, guidance=SampleGuidance(clash=1.0), **kw)


@pytest.mark.parametrize("kw", [
    dict(), dict(guidance=SampleGuidance()), dict(guidance=SampleGuidance(clash=1.0, bond=1.0, max_shift=float("inf"), t_max=0)),
    dict(guidance=SampleGuidance(clash=2, bond=0, t_max=10)), dict(mode="structure"), dict(mode="codesign"), dict(optimize_from=5),
    dict(allowed_aa=torch.ones(V, dtype=torch.bool)), dict(trajectory=True, trajectory_predictions=True), dict(steps=4),
    dict(graph=True, skip_unused_rows=True), dict(num_samples=3, chain_idx=torch.zeros(2, 16, dtype=torch.long)),
    dict(context_index=torch.tensor([1, 0, 1]), B=3, residue_idx=torch.arange(16).expand(3, 16)),
    dict(chain_idx=torch.tensor([0] * 8 + [1] * 8), residue_idx=torch.arange(16, dtype=torch.int32), residue_mask=torch.ones(2, 16, dtype=torch.uint8)),
    dict(flags=_hip.FLAG_PAIR_F32),
])
def test_good_guidance_reaches_the_library(model, kw):
    kw = dict(kw)
    kw.setdefault("guidance", SampleGuidance(clash=1.0, bond=0.5))
    if "context_index" in kw:
        B = kw.pop("B")
        gm = torch.zeros(B, 16, dtype=torch.bool)
        gm[:, 2:9] = True
        with pytest.raises(ReachedTheLibrary):
            model.sample(torch.zeros(B, 16, dtype=torch.long), torch.zeros(B, 16, 3), torch.eye(3).expand(B, 16, 3, 3).clone(), seed=1,
                         generation_mask=gm, res_context_emb=torch.zeros(2, 16, 128), pair_context_emb=torch.zeros(2, 16, 16, 64), **kw)
        return
    with pytest.raises(ReachedTheLibrary):
        call(model, **kw)


@pytest.mark.parametrize("args, kw, match", [
    ((torch.zeros(2, 8, 2), torch.ones(2, 8, dtype=torch.bool)), {}, "\\(B, K, 3\\) or \\(K, 3\\)"),
    ((torch.zeros(2, 8, 3, dtype=torch.long), torch.ones(2, 8, dtype=torch.bool)), {}, "floating point"),
    ((torch.zeros(2, 8, 3), torch.ones(3, 8, dtype=torch.bool)), {}, "generation_mask \\(3, 8\\) does not broadcast"),
    ((torch.zeros(2, 8, 3), torch.ones(2, 8)), {}, "generation_mask must be bool"),
    ((torch.zeros(2, 8, 3), torch.ones(2, 8, dtype=torch.bool)), dict(chain_idx=torch.zeros(7, dtype=torch.long)), "does not broadcast"),
    ((torch.zeros(2, 8, 3), torch.ones(2, 8, dtype=torch.bool)), dict(guidance=SampleGuidance(clash_distance=-1.0)), "clash_distance"),
    ((torch.zeros(2, 8, 3), torch.ones(2, 8, dtype=torch.bool)), dict(guidance="x"), "SampleGuidance"),
])
def test_structure_energy_arguments(args, kw, match):
    with pytest.raises(ValueError, match=match):
        structure_energy(*args, **kw)


def test_structure_energy_reaches_the_library():
    with pytest.raises(ReachedTheLibrary):
        structure_energy(torch.zeros(8, 3), torch.ones(8, dtype=torch.bool), return_grad=True)


def test_sample_guidance_is_frozen():
    g = SampleGuidance()
    assert (g.clash, g.bond, g.clash_distance, g.bond_length, g.max_shift, g.t_max) == (0.0, 0.0, 3.8, 3.8, 1.0, None)
    with pytest.raises(Exception):
        g.clash = 1.0


# ------------------------------------------------------------------ the C ABI
def test_library_exports_the_guidance_entries():
    lib = ctypes.CDLL(_hip.LIB_PATH)
    assert hasattr(lib, "diffab_guidance_energy") and "diffab_guidance_energy" in _hip.SYMBOLS
    # the guidance travels in diffab_sample_options.guidance (the loop's own ABI: test_cabi_and_host.py)
    assert dict(_hip.SampleOptions._fields_)["guidance"] == ctypes.POINTER(_hip.SampleGuidance)
    assert _hip.SYMBOLS["diffab_guidance_energy"][1][2] == ctypes.POINTER(_hip.SampleGuidance)


LAYOUT_C = r"""
#include <stddef.h>
#include <stdio.h>
#include "diffab_hip.h"
#define F(m) printf("%s %zu\n", #m, offsetof(diffab_sample_guidance, m));
int main(void) {
  F(w_clash) F(clash_distance) F(w_bond) F(bond_length) F(max_shift) F(t_max) F(chain) F(residue_idx) F(residue_mask) F(shift_dev)
  printf("size %zu\n", sizeof(diffab_sample_guidance));
  return 0;
}
"""


def test_guidance_struct_layout_matches_the_header(tmp_path):
    """Offsets and size of the ctypes struct against a C compile of include/diffab_hip.h."""
    cc = shutil.which("cc") or shutil.which("gcc") or next((p for p in ("/opt/rocm/llvm/bin/clang",) if os.path.exists(p)), None)
    assert cc, "no C compiler to read the header's layout with"
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text(LAYOUT_C)
    subprocess.run([cc, "-I", os.path.join(REPO, "include"), str(src), "-o", str(exe)], check=True)
    got = dict(line.split() for line in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    S = _hip.SampleGuidance
    for name, _ in S._fields_:
        assert int(got[name]) == getattr(S, name).offset, name
    assert int(got["size"]) == ctypes.sizeof(S) == 56
