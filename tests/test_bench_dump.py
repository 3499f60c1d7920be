"""bench.py --dump-outputs on the host: the size bound, the arrays that fit written whole, a fixed seeded sample of the others."""
import os

import numpy as np
import torch

import bench


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in os.listdir(d)}


def test_dump_outputs_bound_whole_small_arrays_and_seeded_sample(tmp_path, monkeypatch):
    assert bench.DUMP_LIMIT_BYTES == 64 << 20
    limit = 1 << 20
    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", limit)
    g = torch.Generator().manual_seed(0)
    arrays = {
        "loss": torch.tensor([1.5], dtype=torch.float64),
        "seq_idx": torch.randint(0, 21, (64, 16), generator=g),
        "grads": torch.randn(20000, generator=g),  # 80 KB: fits, written whole
        "pair": torch.randn(128, 32, 64, generator=g),  # 1 MB in rows of 8 KB: sampled by row
        "wide": torch.randn(2, 1024, 256, generator=g),  # 2 MB in rows of 1 MB, each over its share: sampled by element
    }
    for run in ("a", "b"):
        bench.dump_outputs(str(tmp_path / run), arrays)
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a")) <= limit
    a, b = _load(tmp_path / "a"), _load(tmp_path / "b")
    assert sorted(a) == sorted(arrays)
    assert a["loss"].dtype == np.float64 and a["loss"].tolist() == [1.5]
    assert all(a[k].dtype == np.float32 for k in ("seq_idx", "grads", "pair", "wide"))
    assert np.array_equal(a["seq_idx"], arrays["seq_idx"].numpy()) and np.array_equal(a["grads"], arrays["grads"].numpy())
    pair = arrays["pair"].numpy()
    assert a["pair"].shape[1:] == pair.shape[1:] and 0 < a["pair"].shape[0] < pair.shape[0]
    rows = [int(np.flatnonzero((pair == r).all(axis=(1, 2)))[0]) for r in a["pair"]]  # every kept row is a row of the tensor, in order
    assert rows == sorted(set(rows))
    assert a["wide"].ndim == 1 and 0 < a["wide"].size < arrays["wide"].numel()
    assert np.isin(a["wide"], arrays["wide"].numpy()).all()
    for k in a:  # the sample is fixed: the same arrays give the same files
        assert np.array_equal(a[k], b[k]), k
