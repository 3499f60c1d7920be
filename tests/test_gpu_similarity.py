"""Design similarities on the MI355X: diffab_metrics_similarity through diffab_pytorch.metrics.similarity.

The rule is DESIGN.md section 4.17 / include/diffab_hip.h.  Both numpy statements of test_similarity_host.py run on the SAME fp32 points the
kernel reads (the CA, or the backbone the frame kernel builds).  Bounds:
  against the fp32 restatement (the kernel's operations in the kernel's order): every integer output EQUAL, every ratio equal to the bit
      (a ratio is one fp32 division of two of the integers, NaN on a zero denominator);
  against the float64 oracle: |lddt - ref| <= (boundary pairs of the row) / (4 sum n_pairs), the boundary pairs being the oracle's count of
      the pairs within 1e-4 A of a threshold or of the inclusion radius (the reasoning is the docstring of test_similarity_host.py); a row
      without one equals the oracle exactly."""
import numpy as np
import pytest
import torch

from diffab_pytorch import metrics
from sampler_support import hip
from test_similarity_host import (CONTACT_KEYS, INT_KEYS, INTERFACE_KEYS, LDDT_KEYS, SHAPES, VARIANTS, case, contacts_f32, lddt_f32, lddt_ref,
                                  numpy_kwargs)

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("hip")]  # every test here needs the device, whether it names the fixture or not

shape_ids = lambda s: "x".join(map(str, s))


def cuda(d):
    return {k: v.cuda() if isinstance(v, torch.Tensor) else v for k, v in d.items()}


def run(des, nat, gm, kw):
    out = metrics.similarity(des, nat, gm, **kw)
    want = set(LDDT_KEYS + CONTACT_KEYS) | (set(INTERFACE_KEYS) if "antigen_mask" in kw else set()) | ({"lddt_segment"} if "segment_idx" in kw else set())
    assert set(out) == want
    assert all(v.dtype == (torch.int32 if k in INT_KEYS else torch.float32) and v.device == des["seq_idx"].device for k, v in out.items())
    return {k: v.cpu().numpy() for k, v in out.items()}


def restatement(des, nat, gm, kw):
    """(points, native points, the fp32 restatement of every output) from the points the kernel reads."""
    G, K = gm.shape
    pts, npts = metrics._points(cuda(des), kw["atoms"]).cpu().numpy(), metrics._points(cuda(nat), kw["atoms"]).cpu().numpy()
    nkw = numpy_kwargs(kw, G, K, kw["atoms"])
    return pts, npts, nkw, {**lddt_f32(pts, npts, gm.numpy(), **nkw), **contacts_f32(pts, npts, gm.numpy(), **nkw)}


def bits(a):
    a = np.asarray(a)
    return a.view(np.int32) if a.dtype == np.float32 else a


def assert_same_bits(got, want, what):
    assert set(got) == set(want), (what, set(got) ^ set(want))
    for k in want:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, (what, k, got[k].dtype, want[k].dtype)
        assert np.array_equal(bits(got[k]), bits(want[k])), (what, k, int((bits(got[k]) != bits(want[k])).sum()))


@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("shape", SHAPES, ids=shape_ids)
def test_similarity_equals_the_restatement_and_the_oracle(shape, variant):
    """K = 16 is a quarter of a wave; K = 130 crosses two 64-lane sweeps raggedly and N = 5 leaves three of the second work-group's four
    waves without a design; one design of one patch; N = 70 is eighteen work-groups per patch.  With more than one patch the last one
    has a native without a contact, and the middle one of three has no generated residue."""
    G, N, K, P = shape
    empty, contactless = (1 if G == 3 else None), (G - 1 if G > 1 else None)
    des, nat, gm, kw = case(G, N, K, P, VARIANTS[variant], empty=empty, contactless=contactless)
    got = run(cuda(des), cuda(nat), gm.cuda(), cuda(kw))
    pts, npts, nkw, want = restatement(des, nat, gm, kw)
    assert_same_bits(got, want, (shape, variant))
    assert got["n_pairs"].sum() > 0 and got["preserved"].sum() > 0 and (G > 1 or got["n_native"].sum() > 0)
    if empty is not None:
        r = slice(empty * N, (empty + 1) * N)
        assert all(np.isnan(got[k][r]).all() for k in ("lddt", "lddt_residue", "lddt_thresholds", "fnat", "fnonnat"))
        assert all((got[k][r] == 0).all() for k in ("preserved", "n_design", "n_kept", "kept_residue"))
        assert (got["n_pairs"][empty] == 0).all() and got["n_native"][empty] == 0
    if contactless is not None:
        r = slice(contactless * N, (contactless + 1) * N)
        assert got["n_native"][contactless] == 0 and np.isnan(got["fnat"][r]).all() and (got["n_kept"][r] == 0).all()
        assert got["n_pairs"][contactless].sum() > 0 and not np.isnan(got["lddt"][r]).any()
    ref = lddt_ref(pts, npts, gm.numpy(), **nkw)
    den = 4.0 * np.repeat(ref["n_pairs"].astype(np.float64).sum(1), N)
    err = np.abs(got["lddt"].astype(np.float64) - ref["lddt"].astype(np.float64))
    ok = den > 0
    assert np.array_equal(np.isnan(got["lddt"]), ~ok)
    print(f"{shape} {variant}: {int(ref['boundary'].sum())} boundary pairs, largest |lddt - oracle| {err[ok].max(initial=0.0):.3g}")
    assert (err[ok] <= ref["boundary"][ok] / den[ok]).all()


@pytest.mark.parametrize("shape", SHAPES, ids=shape_ids)
def test_a_copy_of_the_native_scores_one(shape):
    G, N, K, P = shape
    des, nat, gm, kw = case(G, N, K, P, VARIANTS["antigen"], copy_native=True)
    got = run(cuda(des), cuda(nat), gm.cuda(), cuda(kw))
    assert got["lddt"][-1] == 1.0 and (got["lddt_thresholds"][-1] == 1.0).all() and got["ilddt"][-1] == 1.0
    counted = gm.numpy()[-1]
    assert (got["lddt_residue"][-1][counted] == 1.0).all() and np.isnan(got["lddt_residue"][-1][~counted]).all()
    assert got["n_native"][-1] > 0 and got["fnat"][-1] == 1.0 and got["fnonnat"][-1] == 0.0 and got["n_kept"][-1] == got["n_native"][-1]
    assert np.array_equal(got["kept_residue"][-1], got["native_contacts_residue"][-1])
    kw.pop("antigen_mask")  # and with the non-bonded residues as the partners
    got = run(cuda(des), cuda(nat), gm.cuda(), cuda(kw))
    assert got["n_native"][-1] > 0 and got["fnat"][-1] == 1.0 and got["fnonnat"][-1] == 0.0 and got["lddt"][-1] == 1.0


@pytest.mark.parametrize("shape", [(2, 5, 130, 4), (3, 70, 128, 1)], ids=shape_ids)
def test_a_patch_alone_and_permuted_designs(shape):
    G, N, K, P = shape
    des, nat, gm, kw = case(G, N, K, P, VARIANTS["all"], contactless=0)
    batch = run(cuda(des), cuda(nat), gm.cuda(), cuda(kw))
    per_patch = ("n_pairs", "n_pairs_interface", "n_native", "native_contacts_residue")
    g = G - 1
    rows = slice(g * N, (g + 1) * N)
    one = {k: (v[g:g + 1] if k in ("antigen_mask", "residue_mask", "segment_idx") else v) for k, v in kw.items()}
    alone = run(cuda({k: v[rows] for k, v in des.items()}), cuda({k: v[g:g + 1] for k, v in nat.items()}), gm[g:g + 1].cuda(), cuda(one))
    assert_same_bits(alone, {k: (v[g:g + 1] if k in per_patch else v[rows]) for k, v in batch.items()}, "a patch alone")
    perm = torch.cat([g * N + torch.randperm(N, generator=torch.Generator().manual_seed(g)) for g in range(G)])
    moved = run(cuda({k: v[perm] for k, v in des.items()}), cuda(nat), gm.cuda(), cuda(kw))
    assert_same_bits(moved, {k: (v if k in per_patch else v[perm.numpy()]) for k, v in batch.items()}, "permuted designs")


def test_inputs_as_evaluate_accepts_them():
    """Host tensors (the results come back on the host), float64 and non-contiguous inputs, and a native given per design row."""
    G, N, K, P = 2, 5, 130, 4
    des, nat, gm, kw = case(G, N, K, P, VARIANTS["all"])
    want = run(cuda(des), cuda(nat), gm.cuda(), cuda(kw))
    assert_same_bits(run(des, nat, gm, kw), want, "host inputs")
    wide = torch.zeros(G * N, K, 5, dtype=torch.float64)
    wide[..., 1:4] = des["translations"].double()
    odd = {"seq_idx": des["seq_idx"].cuda(), "translations": wide.cuda()[..., 1:4],
           "orientations": des["orientations"].double().cuda().transpose(-1, -2).contiguous().transpose(-1, -2)}
    assert not odd["translations"].is_contiguous() and not odd["orientations"].is_contiguous()
    per_row = {k: v.repeat_interleave(N, 0).cuda() for k, v in nat.items()}
    assert_same_bits(run(odd, per_row, gm.cuda(), cuda(kw)), want, "float64, non-contiguous, native per row")
