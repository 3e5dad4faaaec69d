"""bench.py --dump-outputs writer: dtypes, size budget, reproducible
sampling (pure host logic, no GPU)."""
import os

import numpy as np
import torch

import bench


def _dir_bytes(d):
    return sum(os.path.getsize(os.path.join(d, f)) for f in os.listdir(d))


def test_dump_small_outputs_written_whole(tmp_path):
    g = torch.Generator().manual_seed(0)
    n_id = torch.randint(0, 1 << 40, (257,), generator=g)
    x = torch.randn(257, 7, generator=g).to(torch.bfloat16)
    ei = torch.randint(0, 257, (2, 1001), generator=g)
    loss = torch.tensor(1.25)
    bench.dump_outputs(str(tmp_path), [("n_id", n_id, 0), ("x", x, 0),
                                       ("edge_index_0", ei, 1),
                                       ("loss", loss.reshape(1), 0)])
    got = {f[:-4]: np.load(tmp_path / f) for f in os.listdir(tmp_path)}
    assert sorted(got) == ["edge_index_0", "loss", "n_id", "x"]
    # integers -> float64 (exact), floating -> float32
    assert got["n_id"].dtype == np.float64
    assert np.array_equal(got["n_id"].astype(np.int64), n_id.numpy())
    assert got["edge_index_0"].dtype == np.float64
    assert got["edge_index_0"].shape == (2, 1001)
    assert got["x"].dtype == np.float32
    assert np.array_equal(got["x"], x.float().numpy())
    assert got["loss"].dtype == np.float32 and got["loss"][0] == 1.25


def test_dump_large_outputs_sampled_within_budget(tmp_path, monkeypatch):
    # scaled-down budget: same code path as a frontier too big for 64 MB
    monkeypatch.setattr(bench, "DUMP_BUDGET_BYTES", 100_000)
    x = torch.arange(5000 * 16, dtype=torch.float32).view(5000, 16)
    ei = torch.arange(2 * 30_000).view(2, 30_000)
    small = torch.ones(10)
    arrays = [("x", x, 0), ("edge_index_0", ei, 1), ("small", small, 0)]
    a, b = tmp_path / "a", tmp_path / "b"
    bench.dump_outputs(str(a), arrays)
    bench.dump_outputs(str(b), arrays)
    assert _dir_bytes(a) <= 100_000 + 3 * 128  # + .npy headers
    xa, ea = np.load(a / "x.npy"), np.load(a / "edge_index_0.npy")
    assert np.load(a / "small.npy").shape == (10,)
    # whole rows / whole edges, in their original order
    assert xa.shape[1] == 16 and 0 < xa.shape[0] < 5000
    assert np.all(np.diff(xa[:, 0]) > 0)
    assert np.all(xa[:, 1] == xa[:, 0] + 1)
    assert ea.shape[0] == 2 and 0 < ea.shape[1] < 30_000
    assert np.all(ea[1] == ea[0] + 30_000)
    # the sample is fixed: equal outputs give equal files
    assert np.array_equal(xa, np.load(b / "x.npy"))
    assert np.array_equal(ea, np.load(b / "edge_index_0.npy"))
