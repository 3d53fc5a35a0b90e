"""bench.py --dump-outputs (bench.dump_outputs) on host tensors: every row as float64 beside its read number while the rows fit the
budget, and past it a fixed, seeded sample in read order that stays within the budget."""
import os

import numpy as np
import torch

import bench


def _rows(bounds):
    """int32 [n, 4] per launch, every column a function of the read number (so a row says which read it belongs to)."""
    out = []
    for lo, hi in bounds:
        r = torch.arange(lo, hi, dtype=torch.int32)
        out.append(torch.stack([r, 2 * r + 1, r % 7, -r], dim=1))
    return out


def _want(idx):
    return np.stack([idx, 2 * idx + 1, idx % 7, -idx], axis=1)


def test_dump_outputs_writes_every_row(tmp_path):
    bounds = [(3000, 5000)]
    bench.dump_outputs(str(tmp_path), _rows(bounds), bounds, 0, 1)
    assert sorted(os.listdir(tmp_path)) == ["read_index.npy", "rows.npy"]
    rows, idx = np.load(tmp_path / "rows.npy"), np.load(tmp_path / "read_index.npy")
    assert rows.dtype == np.float64 and idx.dtype == np.float64
    assert (idx == np.arange(3000, 5000)).all() and (rows == _want(idx)).all()


def test_dump_outputs_samples_past_the_budget(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_BYTES", 4096 + 2 * 40 * 500)      # 500 rows for each of two ranks
    bounds = [(10000, 10700), (10700, 11300)]                          # one step = two launches of this rank
    for run in ("a", "b"):
        bench.dump_outputs(str(tmp_path / run), _rows(bounds), bounds, 1, 2)
    rows, idx = np.load(tmp_path / "a" / "rows_rank1.npy"), np.load(tmp_path / "a" / "read_index_rank1.npy")
    assert rows.shape == (500, 4) and idx.shape == (500,)
    assert (np.diff(idx) > 0).all() and idx[0] >= 10000 and idx[-1] < 11300 and (idx >= 10700).any()
    assert (rows == _want(idx)).all()
    assert (np.load(tmp_path / "b" / "rows_rank1.npy") == rows).all() and (np.load(tmp_path / "b" / "read_index_rank1.npy") == idx).all()
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a")) <= bench.DUMP_BYTES // 2
