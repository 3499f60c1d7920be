"""CPU: the host side of particle steering (DiffAb.sample(steering=...)) - the argument checks made before any library call, the group
homogeneity and shard alignment errors, the C-ABI entries and struct layout, and the properties of the float64 restatement of the
resampling rule (steering.resample_oracle), which tests/test_gpu_steering.py checks the kernel against.

The rule is DESIGN.md section 4.14 / include/diffab_hip.h (diffab_sample_options.steering, diffab_steer_resample)."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

import sampler_support as support
from diffab_pytorch import _hip, distributed
from diffab_pytorch.steering import ParticleSteering, check_groups, check_steering, lineage, resample_oracle, steering_steps
from sampler_support import ReachedTheLibrary, inputs, refuse_library, stand_in

V, T = 21, 10
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------ the oracle's properties
def oracle(lw, u, N, thr=2.0, lam=0.0):
    lw = np.asarray(lw, np.float32)
    z = np.zeros_like(lw)
    return resample_oracle(lw, z, z, u, N, lam, thr)


@pytest.mark.parametrize("N", [1, 2, 3, 64, 65, 257, 1024])
def test_equal_weights_are_the_identity_at_threshold_up_to_one(N):
    G = 3
    for thr in (0.0, 0.5, 1.0):
        out = oracle(np.full(G * N, -3.25), np.array([0.0, 0.4, 0.99]), N, thr)
        assert not out["resampled"].any()
        assert np.array_equal(out["ancestors"].reshape(G, N), np.tile(np.arange(N), (G, 1)))
        assert np.array_equal(out["ess"], np.full(G, float(N)))
        assert np.array_equal(out["logw"], np.full(G * N, -3.25, np.float32))
    # above 1 the group always resamples; equal weights then give every row once
    out = oracle(np.full(G * N, -3.25), np.array([0.0, 0.4, 0.99]), N, 1.5)
    assert out["resampled"].all() and not out["logw"].any()
    assert np.array_equal(out["ancestors"].reshape(G, N), np.tile(np.arange(N), (G, 1)))


@pytest.mark.parametrize("N", [2, 3, 64, 65, 257, 1024])
def test_one_dominant_weight_gives_all_same_ancestors(N):
    rng = np.random.default_rng(N)
    lw = rng.normal(0.0, 1.0, (4, N))
    who = rng.integers(0, N, 4)
    lw[np.arange(4), who] += 2000.0  # every other weight underflows to 0
    out = oracle(lw.reshape(-1), rng.random(4), N, 0.75)  # ESS = 1 < 0.75 N for every N >= 2
    assert out["resampled"].all()
    assert np.array_equal(out["ancestors"].reshape(4, N), np.repeat(who[:, None], N, 1))
    assert np.allclose(out["ess"], 1.0)


@pytest.mark.parametrize("N", [2, 3, 64, 65, 257, 1024])
def test_ancestors_are_sorted_and_counts_are_within_one_of_the_expectation(N):
    rng = np.random.default_rng(100 + N)
    G = 16
    lw = rng.normal(0.0, 5.0, (G, N)).astype(np.float32)
    out = oracle(lw.reshape(-1), rng.random(G).astype(np.float32), N, 2.0)
    anc = out["ancestors"].reshape(G, N)
    assert out["resampled"].all()
    assert (np.diff(anc, axis=1) >= 0).all()
    w = np.exp(lw.astype(np.float64) - lw.max(1, keepdims=True))
    w /= w.sum(1, keepdims=True)
    for g in range(G):
        counts = np.bincount(anc[g], minlength=N)
        assert (np.abs(counts - N * w[g]) < 1.0 + 1e-9).all(), g
    ess = 1.0 / (w * w).sum(1)
    assert np.allclose(out["ess"], ess, rtol=1e-12)


def test_zero_and_nonfinite_weights():
    N = 5
    inf, nan = np.inf, np.nan
    lw = np.array([[0, -inf, 0, 0, 0], [-inf] * 5, [0, nan, 0, 0, -inf], [inf, 0, 0, 0, 0], [-inf, -inf, 1.0, -inf, -inf]], np.float32)
    out = oracle(lw.reshape(-1), np.full(5, 0.999), N, 2.0)
    anc = out["ancestors"].reshape(5, N)
    assert out["resampled"].tolist() == [True, False, True, True, True]
    assert 1 not in anc[0] and set(anc[0]) == {0, 2, 3, 4}
    assert anc[1].tolist() == list(range(N)) and not out["logw"].reshape(5, N)[1].any() and out["ess"][1] == 0.0
    assert set(anc[2]) == {0, 2, 3}
    assert 0 not in anc[3], "a +inf log-weight counts as weight 0"
    assert anc[4].tolist() == [2] * N, "clamped to the last row with weight"
    # u = 0 and the largest float below 1
    for u in (0.0, np.nextafter(np.float32(1), np.float32(0))):
        o = oracle(np.zeros(N), np.array([u]), N, 2.0)
        assert o["ancestors"].tolist() == list(range(N))


def test_weight_update_telescopes_and_resampling_hands_the_energy_down():
    N = 4
    U1, U2 = np.array([3.0, 1.0, 2.0, 50.0], np.float32), np.array([2.5, 0.5, 4.0, 1.0], np.float32)
    z = np.zeros(N, np.float32)
    a = resample_oracle(z, z, U1, [0.3], N, 0.5, 0.0)  # never resamples
    assert np.array_equal(a["logw"], -(np.float32(0.5) * U1)) and np.array_equal(a["u_prev"], U1)
    b = resample_oracle(a["logw"], a["u_prev"], U2, [0.3], N, 0.5, 0.0)
    assert np.allclose(b["logw"], -0.5 * U2, atol=1e-6) and np.array_equal(b["u_prev"], U2)
    c = resample_oracle(z, z, U1, [0.3], N, 0.5, 2.0)
    assert c["resampled"][0] and not c["logw"].any()
    assert np.array_equal(c["u_prev"], U1[c["ancestors"]]) and 3 not in c["ancestors"]


def test_steering_steps_and_lineage():
    assert steering_steps(list(range(10, 0, -1)), 0, 0, 10, 1) == list(range(10, 1, -1)), "the last executed step never steers"
    assert steering_steps(list(range(10, 0, -1)), 0, 3, 9, 3) == [9, 6, 3]
    assert steering_steps(list(range(10, 4, -1)), 4, 0, 10, 1) == [10, 9, 8, 7, 6]
    assert steering_steps([10, 7, 4, 1], 0, 0, 10, 3) == [10, 7, 4]
    assert steering_steps([10, 7, 4, 1], 0, 0, 10, 2) == [10, 4]
    anc = torch.tensor([[0, 0, 2, 3], [1, 1, 3, 3], [0, 1, 2, 2]])
    assert lineage(anc).tolist() == [0, 0, 3, 3]
    assert lineage(torch.empty(0, 3, dtype=torch.int64)).tolist() == [0, 1, 2]


# ------------------------------------------------------------------ argument checks before the library
@pytest.fixture(scope="module")
def model():
    return stand_in(T=T)


@pytest.fixture()
def no_library(monkeypatch):
    refuse_library(monkeypatch)


def call(model, B=2, K=16, gm=None, **kw):
    inp = inputs(B, K)
    return support.call(model, inp if gm is None else dict(inp, generation_mask=gm), **kw)


BAD = [
    ({"strength": 1.0}, "must be a steering.ParticleSteering"), (1.0, "must be a steering.ParticleSteering"),
    (ParticleSteering(strength=-1.0), "strength must be a finite number >= 0"), (ParticleSteering(strength=float("inf")), "strength"),
    (ParticleSteering(strength=True), "strength"), (ParticleSteering(clash=float("nan")), "clash must be"),
    (ParticleSteering(bond=-0.5), "bond must be"), (ParticleSteering(clash_distance=0.0), "clash_distance must be a finite number > 0"),
    (ParticleSteering(bond_length=float("inf")), "bond_length must be"), (ParticleSteering(ess_threshold=-0.1), "ess_threshold must lie in \\[0, 2\\]"),
    (ParticleSteering(ess_threshold=2.5), "ess_threshold"), (ParticleSteering(ess_threshold=float("nan")), "ess_threshold"),
    (ParticleSteering(every=0), "every must be an int >= 1"), (ParticleSteering(every=1.0), "every must be"),
    (ParticleSteering(t_min=-1), "t_min must be an int in \\[0, T = 10\\]"), (ParticleSteering(t_min=11), "t_min must be"),
    (ParticleSteering(t_max=11), "t_max must be None or an int"), (ParticleSteering(t_min=5, t_max=4), "t_max must be"),
    (ParticleSteering(t_max=2.0), "t_max must be"), (ParticleSteering(group_size=0), "group_size must be None or an int in \\[1, 1024\\]"),
    (ParticleSteering(group_size=1025), "group_size must be"), (ParticleSteering(group_size=True), "group_size must be"),
]


@pytest.mark.parametrize("bad, match", BAD)
def test_bad_steering_is_rejected(model, no_library, bad, match):
    with pytest.raises(ValueError, match=match):
        call(model, steering=bad, num_samples=2)
    if isinstance(bad, ParticleSteering):
        with pytest.raises(ValueError, match=match):
            check_steering("x", bad, T)


def test_groups_must_be_whole_and_homogeneous(model, no_library):
    S = ParticleSteering()
    with pytest.raises(ValueError, match="mode='fixed_backbone' keeps as given"):
        call(model, steering=S, num_samples=2, mode="fixed_backbone")
    with pytest.raises(ValueError, match="t_min = 6 is above the first step of the call"):
        call(model, steering=ParticleSteering(t_min=6), num_samples=2, optimize_from=5)
    with pytest.raises(ValueError, match="4 state rows are not a multiple of the steering group_size = 3"):
        call(model, steering=ParticleSteering(group_size=3), num_samples=2)
    with pytest.raises(ValueError, match="3 state rows are not a multiple of the steering group_size = 2"):
        call(model, B=3, steering=ParticleSteering(group_size=2))
    gm = torch.zeros(4, 16, dtype=torch.bool)
    gm[:, 3:8] = True
    gm[3, 9] = True
    with pytest.raises(ValueError, match="generation_mask to be the same on all rows of a group; group 1 \\(rows 2 .. 3\\)"):
        call(model, B=4, gm=gm, steering=ParticleSteering(group_size=2))
    with pytest.raises(ValueError, match="generation_mask"):  # two patches in one group of four designs
        call(model, B=2, gm=gm[2:], steering=ParticleSteering(group_size=4), num_samples=2)
    chain = torch.zeros(4, 16, dtype=torch.long)
    chain[1, 5] = 1
    with pytest.raises(ValueError, match="chain_idx to be the same on all rows of a group; group 0"):
        call(model, B=4, steering=ParticleSteering(group_size=2), chain_idx=chain)
    with pytest.raises(ValueError, match="residue_idx to be the same"):
        call(model, B=4, steering=ParticleSteering(group_size=4), residue_idx=torch.arange(16).expand(4, 16) + torch.arange(4)[:, None])
    gm3 = torch.zeros(3, 16, dtype=torch.bool)
    gm3[:, 2:9] = True
    with pytest.raises(ValueError, match="context \\(context_index\\) to be the same on all rows of a group"):
        model.sample(torch.zeros(3, 16, dtype=torch.long), torch.zeros(3, 16, 3), torch.eye(3).expand(3, 16, 3, 3).clone(), seed=1,
                     generation_mask=gm3, res_context_emb=torch.zeros(2, 16, 128), pair_context_emb=torch.zeros(2, 16, 16, 64),
                     context_index=torch.tensor([1, 0, 1]), steering=ParticleSteering(group_size=3))
    with pytest.raises(ValueError, match="same on all rows"):
        check_groups("x", 2, 4, {"f": torch.tensor([[1], [1], [2], [3]])})
    check_groups("x", 2, 4, {"f": torch.tensor([[1], [1], [2], [2]]), "g": None})


@pytest.mark.parametrize("kw", [
    dict(num_samples=3), dict(), dict(steering=ParticleSteering(strength=0.0, ess_threshold=0.0, group_size=2)),
    dict(steering=ParticleSteering(group_size=1)), dict(num_samples=4, steering=ParticleSteering(group_size=2, every=3, t_min=2, t_max=9)),
    dict(num_samples=2, mode="structure"), dict(num_samples=2, optimize_from=5), dict(num_samples=2, allowed_aa=torch.ones(V, dtype=torch.bool)),
    dict(num_samples=2, trajectory=True, trajectory_predictions=True), dict(num_samples=2, steps=4), dict(num_samples=2, graph=True),
    dict(num_samples=2, chain_idx=torch.tensor([0] * 8 + [1] * 8), residue_mask=torch.ones(2, 16, dtype=torch.uint8)),
])
def test_good_steering_reaches_the_library(model, no_library, kw):
    kw = dict(kw)
    kw.setdefault("steering", ParticleSteering(strength=2.0, ess_threshold=0.5))
    with pytest.raises(ReachedTheLibrary):
        call(model, **kw)


def test_shard_range_is_group_aligned():
    assert distributed.shard_range(10, 1, 3) == (4, 7), "the default split is unchanged"
    rows, N = 7 * 4, 4
    got = [distributed.shard_range(rows, r, 3, group_size=N) for r in range(3)]
    assert got == [(0, 12), (12, 20), (20, 28)]
    assert all(lo % N == 0 and hi % N == 0 for lo, hi in got)
    assert distributed.shard_range(8, 2, 3, group_size=4) == (8, 8), "more ranks than groups: an empty shard"
    with pytest.raises(ValueError, match="10 rows are not a multiple of group_size = 4"):
        distributed.shard_range(10, 0, 2, group_size=4)
    with pytest.raises(ValueError, match="group_size must be an int >= 1"):
        distributed.shard_range(8, 0, 2, group_size=0)


def test_particle_steering_is_frozen():
    s = ParticleSteering()
    assert (s.strength, s.clash, s.bond, s.clash_distance, s.bond_length, s.ess_threshold, s.every, s.t_min, s.t_max, s.group_size) == \
        (1.0, 1.0, 1.0, 3.8, 3.8, 0.5, 1, 0, None, None)
    with pytest.raises(Exception):
        s.strength = 2.0


# ------------------------------------------------------------------ the C ABI
def test_library_exports_the_steering_entries():
    lib = ctypes.CDLL(_hip.LIB_PATH)
    for name in ("diffab_steer_energy", "diffab_steer_resample", "diffab_steer_gather"):
        assert hasattr(lib, name) and name in _hip.SYMBOLS, name
    # the steering travels in diffab_sample_options.steering (the loop's own ABI: test_cabi_and_host.py)
    assert dict(_hip.SampleOptions._fields_)["steering"] == ctypes.POINTER(_hip.SampleSteering)
    assert len(_hip.SYMBOLS["diffab_steer_resample"][1]) == 11 and len(_hip.SYMBOLS["diffab_steer_gather"][1]) == 9
    assert _hip.SYMBOLS["diffab_steer_energy"][1][5] == ctypes.POINTER(_hip.SampleSteering)
    src = open(os.path.join(REPO, "diffab-pytorch_amd", "csrc", "philox.h")).read()
    assert "STREAM_STEER = 11" in src


LAYOUT_C = r"""
#include <stddef.h>
#include <stdio.h>
#include "diffab_hip.h"
#define F(m) printf("%s %zu\n", #m, offsetof(diffab_sample_steering, m));
int main(void) {
  F(w_clash) F(clash_distance) F(w_bond) F(bond_length) F(strength) F(ess_threshold) F(t_min) F(t_max) F(every) F(group_size) F(chain)
  F(residue_idx) F(residue_mask) F(logw) F(u_prev) F(energy) F(ancestors) F(scratch)
  printf("size %zu\n", sizeof(diffab_sample_steering));
  printf("max_group %d\n", DIFFAB_STEER_MAX_GROUP);
  printf("scratch_bytes %zu\n", DIFFAB_STEER_SCRATCH_BYTES(6, 130));
  return 0;
}
"""


def test_steering_struct_layout_matches_the_header(tmp_path):
    """Offsets and size of the ctypes struct, and the two macros, against a C compile of include/diffab_hip.h."""
    from diffab_pytorch import steering

    cc = shutil.which("cc") or shutil.which("gcc") or next((p for p in ("/opt/rocm/llvm/bin/clang",) if os.path.exists(p)), None)
    assert cc, "no C compiler to read the header's layout with"
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text(LAYOUT_C)
    subprocess.run([cc, "-I", os.path.join(REPO, "include"), str(src), "-o", str(exe)], check=True)
    got = dict(line.split() for line in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    S = _hip.SampleSteering
    for name, _ in S._fields_:
        assert int(got[name]) == getattr(S, name).offset, name
    assert int(got["size"]) == ctypes.sizeof(S) == 104
    assert int(got["max_group"]) == steering.MAX_GROUP
    assert int(got["scratch_bytes"]) == steering.scratch_bytes(6, 130)
