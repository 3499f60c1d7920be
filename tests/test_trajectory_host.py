"""CPU: the host side of trajectory recording (DiffAb.sample(trajectory=...)) - the C-ABI entry, the argument checks that happen before
any library call, the recorded labels, io.write_trajectory_pdb and the nested sample files."""
import ctypes

import pytest
import torch

import sampler_support as support
from diffab_pytorch import _hip, io
from diffab_pytorch.diffab_pytorch import _trajectory_labels
from sampler_support import ReachedTheLibrary, inputs, refuse_library, stand_in

V, T = 21, 10


def test_record_struct_layout():
    # int32 n_slots, then eight pointers (the host table, the device table, three state and three prediction fields)
    names = [f[0] for f in _hip.SampleRecord._fields_]
    assert names == ["n_slots", "slot_of_step", "slot_dev", "seq", "x", "O", "pred_x", "pred_O", "seq_probs"]
    assert ctypes.sizeof(_hip.SampleRecord) == 8 + 8 * ctypes.sizeof(ctypes.c_void_p)


@pytest.fixture(scope="module")
def model():
    return stand_in(T=T)


@pytest.fixture(autouse=True)
def no_library(monkeypatch):
    refuse_library(monkeypatch)


def call(model, B=2, K=16, **kw):
    return support.call(model, inputs(B, K), **kw)


@pytest.mark.parametrize("bad, match", [
    (1.0, "got the float"), (2.5, "got the float"), (0, "stride must be an int >= 1"), (-3, "stride must be an int >= 1"),
    (torch.tensor([[5, 4]]), "non-empty 1-D integer list"), ([], "non-empty 1-D integer list"),
    (torch.tensor([True, False]), "non-empty 1-D integer list"), (torch.tensor([5.0, 4.0]), "non-empty 1-D integer list"),
    ([11], "step 11 outside \\[t_stop \\+ 1, t_start\\] = \\[1, 10\\]"), ([0], "step 0 outside"), ([5, 3, 5], "more than once"),
])
def test_bad_trajectory_is_rejected(model, bad, match):
    with pytest.raises(ValueError, match=match):
        call(model, trajectory=bad)


def test_step_outside_a_truncated_run_is_rejected(model):
    with pytest.raises(ValueError, match="step 3 outside \\[t_stop \\+ 1, t_start\\] = \\[4, 8\\]"):
        call(model, trajectory=[8, 3], t_start=8, t_stop=3)
    with pytest.raises(ValueError, match="step 9 outside"):
        call(model, trajectory=[9], optimize_from=6)


def test_predictions_without_trajectory_are_rejected(model):
    for off in (None, False):
        with pytest.raises(ValueError, match="give trajectory as well"):
            call(model, trajectory=off, trajectory_predictions=True)


def test_empty_run_is_rejected(model):
    with pytest.raises(ValueError, match="records no step"):
        call(model, trajectory=True, t_start=4, t_stop=4)


def test_bad_range_is_rejected(model):
    with pytest.raises(ValueError, match="a trajectory needs T = 10 >= t_start = 12"):
        call(model, trajectory=True, t_start=12)


@pytest.mark.parametrize("kw", [dict(trajectory=True), dict(trajectory=2, trajectory_predictions=True), dict(trajectory=[10, 1]),
                                dict(trajectory=torch.tensor([3, 7]), num_samples=2, allowed_aa=torch.ones(V, dtype=torch.bool)),
                                dict(trajectory=True, mode="structure", optimize_from=5)])
def test_good_trajectory_reaches_the_library(model, kw):
    with pytest.raises(ReachedTheLibrary):
        call(model, **kw)


def test_no_trajectory_is_todays_call(model):
    with pytest.raises(ReachedTheLibrary):
        call(model, trajectory=None)
    with pytest.raises(ReachedTheLibrary):
        call(model, trajectory=False)


# ------------------------------------------------------------------ labels
def labels(tr, t_start=T, t_stop=0, T_=T):
    out = _trajectory_labels("x", tr, False, t_start, t_stop, T_)
    return None if out is None else out.tolist()


def test_labels_every_step_and_stride():
    assert labels(True) == list(range(10, 0, -1))
    assert labels(1) == list(range(10, 0, -1))
    assert labels(3) == [10, 7, 4, 1]
    assert labels(4) == [10, 6, 2]
    assert labels(100) == [10]
    assert labels(10, t_start=8, t_stop=2) == [8]
    assert labels(2, t_start=8, t_stop=2) == [8, 6, 4]
    assert labels(True, t_start=5, t_stop=2) == [5, 4, 3]


def test_labels_list_form_is_sorted_descending():
    assert labels([1, 10, 4]) == [10, 4, 1]
    assert labels(torch.tensor([2, 9], dtype=torch.int32)) == [9, 2]
    assert labels((5,)) == [5]
    assert labels([7, 3], t_start=7, t_stop=2) == [7, 3]
    assert labels(None) is None and labels(False) is None


# ------------------------------------------------------------------ PDB writer
def synthetic_trajectory(B=2, n=3, K=6, predictions=True, seed=0):
    g = torch.Generator().manual_seed(seed)
    tr = {"t": torch.tensor([9, 5, 1])[:n], "seq_idx": torch.randint(0, 20, (B, n, K), generator=g),
          "translations": torch.randn(B, n, K, 3, generator=g) * 5,
          "orientations": torch.linalg.qr(torch.randn(B, n, K, 3, 3, generator=g)).Q}
    tr["orientations"] = tr["orientations"] * torch.linalg.det(tr["orientations"]).sign()[..., None, None]
    if predictions:
        tr["pred_translations"] = torch.randn(B, n, K, 3, generator=g) * 5
        q = torch.linalg.qr(torch.randn(B, n, K, 3, 3, generator=g)).Q
        tr["pred_orientations"] = q * torch.linalg.det(q).sign()[..., None, None]
        tr["seq_probs"] = torch.softmax(torch.randn(B, n, K, V, generator=g) * 3, -1)
    return tr


def parse_models(path):
    models, cur = [], None
    for line in open(path).read().splitlines():
        if line.startswith("MODEL"):
            cur = {"label": int(line[6:].strip()), "atoms": []}
        elif line.startswith("ATOM"):
            cur["atoms"].append((line[12:16].strip(), line[17:20], float(line[30:38]), float(line[38:46]), float(line[46:54]),
                                 float(line[60:66])))
        elif line.startswith("ENDMDL"):
            models.append(cur)
            cur = None
    return models


@pytest.mark.parametrize("predictions", [False, True])
def test_trajectory_pdb_models_and_frames(tmp_path, predictions):
    tr = synthetic_trajectory()
    row, K = 1, 6
    path = tmp_path / "traj.pdb"
    n_atoms = io.write_trajectory_pdb(str(path), tr, row, predictions=predictions)
    models = parse_models(path)
    assert [m["label"] for m in models] == [9, 5, 1]
    assert all(len(m["atoms"]) == 4 * K for m in models) and n_atoms == 3 * 4 * K
    assert open(path).read().rstrip().endswith("END")
    x, O = (tr["pred_translations"], tr["pred_orientations"]) if predictions else (tr["translations"], tr["orientations"])
    seq = tr["seq_probs"].argmax(-1) if predictions else tr["seq_idx"]
    for j, m in enumerate(models):
        xyz = torch.tensor([a[2:5] for a in m["atoms"]], dtype=torch.float64).view(K, 4, 3)
        ca, R = io.frames_from_backbone(xyz[:, 0], xyz[:, 1], xyz[:, 2])
        assert torch.allclose(ca, x[row, j].double(), atol=2e-3)  # %8.3f
        assert torch.allclose(R, O[row, j].double(), atol=1e-2)
        names = [a[1] for a in m["atoms"][::4]]
        assert names == [io.AA3[int(s)] for s in seq[row, j]]
        # the b-factor is the probability of the written residue
        p = tr["seq_probs"][row, j].gather(-1, seq[row, j].unsqueeze(-1)).squeeze(-1)
        assert torch.allclose(torch.tensor([a[5] for a in m["atoms"][::4]]), p, atol=6e-3)


def test_trajectory_pdb_without_probabilities_and_masks(tmp_path):
    tr = synthetic_trajectory(predictions=False)
    path = tmp_path / "t.pdb"
    mask = torch.tensor([True, False, True, True, False, True])
    assert io.write_trajectory_pdb(str(path), tr, 0, residue_mask=mask, chain_idx=torch.full((6,), 2)) == 3 * 4 * 4
    models = parse_models(path)
    assert all(a[5] == 0.0 for m in models for a in m["atoms"])
    assert all(line[21] == "B" for line in open(path) if line.startswith("ATOM"))
    with pytest.raises(ValueError, match="trajectory_predictions=True"):
        io.write_trajectory_pdb(str(path), tr, 0, predictions=True)


def test_write_pdb_output_is_unchanged(tmp_path):
    """write_pdb's records, serials, END line and return value, pinned on a fixed input."""
    tr = synthetic_trajectory(predictions=False)
    path = tmp_path / "one.pdb"
    seq = torch.tensor([7, 0, 20, 3, 7, 19])
    n = io.write_pdb(str(path), seq, tr["translations"][0, 0], tr["orientations"][0, 0], b_factor=torch.arange(6) / 10,
                     atoms=io.BACKBONE_ATOMS)
    lines = open(path).read().split("\n")
    assert n == 5 * 6 - 2 and lines[-2:] == ["END", ""] and len(lines) == n + 2
    assert lines[0].startswith("ATOM      1 N    GLY A   1 ") and lines[0].endswith("  1.00  0.00           N")
    assert [int(line[6:11]) for line in lines[:n]] == list(range(1, n + 1))


# ------------------------------------------------------------------ sample files
def test_nested_samples_round_trip_bitwise(tmp_path):
    tr = synthetic_trajectory()
    out = {"seq_idx": tr["seq_idx"][:, -1], "translations": tr["translations"][:, -1], "orientations": tr["orientations"][:, -1],
           "trajectory": tr, "noised": {"seq_t": torch.zeros(2, 3, dtype=torch.long), "x_t": torch.randn(2, 3, 3).requires_grad_()}}
    path = tmp_path / "s.pt"
    io.save_samples(str(path), out, seed=3, note="traj")
    got, meta = io.load_samples(str(path))
    assert meta == {"seed": 3, "note": "traj"}

    def check(a, b):
        assert set(a) == set(b)
        for k in b:
            if isinstance(b[k], dict):
                check(a[k], b[k])
            else:
                assert a[k].dtype == b[k].dtype and torch.equal(a[k], b[k].detach()), k
                assert not a[k].requires_grad
    check(got, out)
