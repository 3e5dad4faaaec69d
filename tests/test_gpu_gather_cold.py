"""Feature gather over an HBM shard plus a pinned-host (cold) shard: every
row-width path, list lengths around the block and grid boundaries, the
device-side row count, the feature_order translation folded into the
kernel, and the side-stream plumbing, all against plain-torch CPU
indexing."""
import functools
import os
import subprocess
import sys

import pytest
import torch

import quiver
from quiver.shard_tensor import ShardTensor, ShardTensorConfig

pytestmark = pytest.mark.gpu

N_HOT, N_COLD = 3000, 5000
N_ROWS = N_HOT + N_COLD

ROW_TYPES = [
    (torch.float32, 100),   # 400 B, 16 B vectors, 25 of 32 lanes
    (torch.float16, 602),   # 1204 B, 4 B vectors, longer than one pass
    (torch.bfloat16, 7),    # 14 B, byte path
    (torch.float32, 1),     # 4 B
    (torch.int64, 16),      # 128 B
]


ROWS_PER_SUBGROUP = 1  # rows a sub-group has in flight per iteration


def _rows_per_block_iter(dtype, dim):
    """Rows one 256-thread block of the gather kernel takes per iteration
    (mirrors the launcher: widest vector, sub-group covering the row)."""
    row_bytes = dim * torch.empty(0, dtype=dtype).element_size()
    vec = next(v for v in (16, 8, 4, 1) if row_bytes % v == 0)
    nvec = row_bytes // vec
    sub = 4
    while sub < 64 and sub < nvec:
        sub *= 2
    return 256 // sub * ROWS_PER_SUBGROUP


@functools.lru_cache(maxsize=None)
def _table(dtype, dim):
    """(cpu reference, mixed-tier ShardTensor); built once, never written."""
    g = torch.Generator().manual_seed(11)
    if dtype.is_floating_point:
        t = torch.randn(N_ROWS, dim, generator=g).to(dtype)
    else:
        t = torch.randint(0, 1 << 40, (N_ROWS, dim), dtype=dtype, generator=g)
    st = ShardTensor(0, ShardTensorConfig({}))
    st.append(t[:N_HOT], 0)
    st.append(t[N_HOT:], -1)
    return t, st


def _index_sets(dtype, dim):
    g = torch.Generator().manual_seed(5)
    R = ROWS_PER_SUBGROUP
    rpb = _rows_per_block_iter(dtype, dim)
    sets = {}
    # all-cold sets around one sub-group's and one block's share
    for L in sorted({0, 1, R - 1, R, R + 1, rpb - 1, rpb, rpb + 1}):
        sets[f"cold_len{L}"] = torch.randint(N_HOT, N_ROWS, (L,), generator=g)
    # more than one sweep of the capped host-tier grid: grid-stride wrap
    sets["mixed_20000"] = torch.randint(0, N_ROWS, (20000,), generator=g)
    sets["all_hot"] = torch.randint(0, N_HOT, (700,), generator=g)
    sets["all_cold"] = torch.randint(N_HOT, N_ROWS, (20000,), generator=g)
    alt = torch.empty(1001, dtype=torch.int64)
    alt[0::2] = torch.randint(0, N_HOT, (501,), generator=g)
    alt[1::2] = torch.randint(N_HOT, N_ROWS, (500,), generator=g)
    sets["alternating"] = alt
    sets["same_cold_x64"] = torch.full((64,), N_HOT + 1234, dtype=torch.int64)
    return sets


@pytest.mark.parametrize("dtype,dim", ROW_TYPES)
def test_index_sets(dtype, dim):
    t, st = _table(dtype, dim)
    for name, idx in _index_sets(dtype, dim).items():
        got = st[idx.cuda()].cpu()
        assert got.shape == (idx.numel(), dim), name
        assert torch.equal(got, t[idx]), name


@pytest.mark.parametrize("dtype,dim", ROW_TYPES)
def test_out_of_range_index_skipped(dtype, dim):
    t, st = _table(dtype, dim)
    g = torch.Generator().manual_seed(6)
    idx = torch.randint(0, N_ROWS, (301,), generator=g)
    bad = 150
    idx[bad] = N_ROWS + 7
    got = st[idx.cuda()].cpu()
    keep = torch.arange(301) != bad
    assert torch.equal(got[keep], t[idx[keep]])


@pytest.mark.parametrize("dtype,dim", ROW_TYPES)
@pytest.mark.parametrize("k", [0, 1, 1000, 4096])
def test_gather_n_device_count(dtype, dim, k):
    """Upper-bound frontier with the exact count on the device and zeroed
    slack, as the sampler emits it: the first k rows are exact."""
    t, st = _table(dtype, dim)
    g = torch.Generator().manual_seed(8)
    idx = torch.zeros(4096, dtype=torch.int64)
    idx[:k] = torch.randint(0, N_ROWS, (k,), generator=g)
    n_dev = torch.tensor([k], dtype=torch.int64, device="cuda")
    got = st.gather_n(idx.cuda(), n_dev)
    assert got.shape[0] == 4096
    assert torch.equal(got[:k].cpu(), t[idx[:k]])


def test_host_only_and_hbm_only_tables():
    g = torch.Generator().manual_seed(9)
    t = torch.randn(4000, 100, generator=g)
    idx = torch.randint(0, 4000, (5000,), generator=g)
    n_dev = torch.tensor([3000], dtype=torch.int64, device="cuda")

    host = ShardTensor(0, ShardTensorConfig({}))
    host.append(t, -1)
    assert torch.equal(host[idx.cuda()].cpu(), t[idx])
    assert torch.equal(host.gather_n(idx.cuda(), n_dev)[:3000].cpu(),
                       t[idx[:3000]])

    hbm = ShardTensor(0, ShardTensorConfig({}))
    hbm.append(t, 0)
    assert torch.equal(hbm[idx.cuda()].cpu(), t[idx])
    assert torch.equal(hbm.gather_n(idx.cuda(), n_dev)[:3000].cpu(),
                       t[idx[:3000]])


def test_feature_order_fold(small_graph):
    indptr, indices = small_graph
    topo = quiver.CSRTopo(indptr=indptr, indices=indices)
    n = topo.node_count
    g = torch.Generator().manual_seed(10)
    feat_cpu = torch.randn(n, 100, generator=g)
    feature = quiver.Feature(0, device_list=[0], device_cache_size="40K",
                             cache_policy="device_replicate", csr_topo=topo)
    feature.from_cpu_tensor(feat_cpu.clone())
    assert feature.feature_order is not None
    st = feature._shard_tensor().shard_tensor
    assert sorted(st.shard_devices()) == [-1, 0]  # both tiers present

    idx = torch.randint(0, n, (1500,), generator=g)
    k = 1200
    n_dev = torch.tensor([k], dtype=torch.int64, device="cuda")
    raw = feature.gather_raw(idx.cuda(), n_dev)
    direct = feature[idx.cuda()]
    assert torch.equal(direct.cpu(), feat_cpu[idx])
    assert torch.equal(raw[:k].cpu(), feat_cpu[idx[:k]])
    assert torch.equal(raw[:k], direct[:k])


def test_feature_without_order():
    g = torch.Generator().manual_seed(12)
    feat_cpu = torch.randn(2000, 100, generator=g)
    feature = quiver.Feature(0, device_list=[0], device_cache_size="200K")
    feature.from_cpu_tensor(feat_cpu.clone())
    assert feature.feature_order is None
    idx = torch.randint(0, 2000, (3000,), generator=g)
    n_dev = torch.tensor([2500], dtype=torch.int64, device="cuda")
    raw = feature.gather_raw(idx.cuda(), n_dev)
    assert torch.equal(feature[idx.cuda()].cpu(), feat_cpu[idx])
    assert torch.equal(raw[:2500].cpu(), feat_cpu[idx[:2500]])


def test_feature_out_of_range_ids_skipped(small_graph):
    """With an order table, ids outside [0, len(order)) and negative ids
    are skipped (no table read out of bounds); their neighbours are
    exact.  Without one, a negative id is skipped too."""
    indptr, indices = small_graph
    topo = quiver.CSRTopo(indptr=indptr, indices=indices)
    n = topo.node_count
    g = torch.Generator().manual_seed(14)
    feat_cpu = torch.randn(n, 100, generator=g)
    feature = quiver.Feature(0, device_list=[0], device_cache_size="40K",
                             cache_policy="device_replicate", csr_topo=topo)
    feature.from_cpu_tensor(feat_cpu.clone())
    idx = torch.randint(0, n, (400,), generator=g)
    bad = [7, 200, 399]
    idx[7], idx[200], idx[399] = n, -1, n + 12345
    keep = torch.ones(400, dtype=torch.bool)
    keep[bad] = False
    got = feature[idx.cuda()].cpu()
    assert torch.equal(got[keep], feat_cpu[idx[keep]])
    n_dev = torch.tensor([400], dtype=torch.int64, device="cuda")
    raw = feature.gather_raw(idx.cuda(), n_dev).cpu()
    assert torch.equal(raw[keep], feat_cpu[idx[keep]])

    t, st = _table(torch.float32, 100)
    idx2 = torch.randint(0, N_ROWS, (300,), generator=g)
    idx2[100] = -5
    keep2 = torch.arange(300) != 100
    assert torch.equal(st[idx2.cuda()].cpu()[keep2], t[idx2[keep2]])


STAGED_ORDER_SCRIPT = r"""
import numpy as np
import torch
import quiver

rng = np.random.default_rng(0)
n = 20000
degs = np.minimum((rng.pareto(1.5, n) * 4).astype(int) + 1, 64)
indptr = np.zeros(n + 1, dtype=np.int64)
indptr[1:] = np.cumsum(degs)
indices = rng.integers(0, n, indptr[-1], dtype=np.int64)
topo = quiver.CSRTopo(indptr=torch.from_numpy(indptr),
                      indices=torch.from_numpy(indices))
g = torch.Generator().manual_seed(2)
feat_cpu = torch.randn(n, 100, generator=g)
feature = quiver.Feature(0, device_list=[0], device_cache_size="2M",
                         cache_policy="device_replicate", csr_topo=topo)
feature.from_cpu_tensor(feat_cpu.clone())
assert feature.feature_order is not None
assert sorted(feature._shard_tensor().shard_tensor.shard_devices()) == [-1, 0]
idx = torch.randint(0, n, (9000,), generator=g)
got = feature[idx.cuda()].cpu()
assert torch.equal(got, feat_cpu[idx])
print("STAGED-ORDER-OK")
"""


def test_staged_gather_with_order_table():
    """CPU-staged host tier (QUIVER_STAGED_GATHER=1, read once per process)
    behind a Feature with a feature_order table."""
    env = dict(os.environ)
    env["QUIVER_STAGED_GATHER"] = "1"
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    res = subprocess.run([sys.executable, "-c", STAGED_ORDER_SCRIPT],
                         env=env, capture_output=True, text=True,
                         timeout=300, cwd=root)
    assert res.returncode == 0, res.stdout + res.stderr
    assert "STAGED-ORDER-OK" in res.stdout


def test_two_streams_back_to_back(small_graph):
    """Two gather_raw calls on two streams, no sync in between: they share
    the cached side stream and its split/join events."""
    indptr, indices = small_graph
    topo = quiver.CSRTopo(indptr=indptr, indices=indices)
    n = topo.node_count
    g = torch.Generator().manual_seed(13)
    feat_cpu = torch.randn(n, 100, generator=g)
    feature = quiver.Feature(0, device_list=[0], device_cache_size="40K",
                             cache_policy="device_replicate", csr_topo=topo)
    feature.from_cpu_tensor(feat_cpu.clone())
    idx_a = torch.randint(0, n, (20000,), generator=g)
    idx_b = torch.randint(0, n, (20000,), generator=g)
    dev_a, dev_b = idx_a.cuda(), idx_b.cuda()
    n_a = torch.tensor([20000], dtype=torch.int64, device="cuda")
    n_b = torch.tensor([17000], dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    with torch.cuda.stream(s1):
        out_a = feature.gather_raw(dev_a, n_a)
    with torch.cuda.stream(s2):
        out_b = feature.gather_raw(dev_b, n_b)
    torch.cuda.synchronize()
    assert torch.equal(out_a.cpu(), feat_cpu[idx_a])
    assert torch.equal(out_b[:17000].cpu(), feat_cpu[idx_b[:17000]])


HIPGRAPH_SCRIPT = r"""
import os, sys, warnings
import numpy as np
import torch
import quiver

rng = np.random.default_rng(0)
n = 500
degs = np.minimum((rng.pareto(1.5, n) * 4).astype(int) + 1, 64)
indptr = np.zeros(n + 1, dtype=np.int64)
indptr[1:] = np.cumsum(degs)
indices = rng.integers(0, n, indptr[-1], dtype=np.int64)
topo = quiver.CSRTopo(indptr=torch.from_numpy(indptr),
                      indices=torch.from_numpy(indices))
g = torch.Generator().manual_seed(1)
feat_cpu = torch.randn(n, 100, generator=g)
feature = quiver.Feature(0, device_list=[0], device_cache_size="40K",
                         cache_policy="device_replicate", csr_topo=topo)
feature.from_cpu_tensor(feat_cpu.clone())
batches = [torch.randint(0, n, (64,), generator=g) for _ in range(3)]


def run(graphed):
    os.environ["QUIVER_HIPGRAPH"] = "1" if graphed else "0"
    sampler = quiver.GraphSageSampler(topo, [5, 3], device=0, mode="GPU")
    sampler.lazy_init_quiver()
    sampler.quiver.set_seed(1234)
    out = []
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        for n_id, bs, adjs, x in quiver.TrainingPrefetcher(
                sampler, feature, batches, depth=1, device=0, num_streams=1):
            torch.cuda.synchronize()
            out.append((n_id.cpu().clone(), x.cpu().clone()))
    refused = any("capture failed" in str(m.message)
                  or "replay failed" in str(m.message) for m in w)
    return out, refused


plain, _ = run(False)
graphed, refused = run(True)
if refused:
    print("HIPGRAPH-REFUSED")
    sys.exit(0)
assert len(plain) == len(graphed) == 3
for (n0, x0), (n1, x1) in zip(plain, graphed):
    assert torch.equal(n0, n1)
    assert torch.equal(x0, x1)
    assert torch.equal(x1, feat_cpu[n1])
print("HIPGRAPH-OK")
"""


def test_hipgraph_prefetcher_matches_uncaptured():
    env = dict(os.environ)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    res = subprocess.run([sys.executable, "-c", HIPGRAPH_SCRIPT], env=env,
                         capture_output=True, text=True, timeout=300,
                         cwd=root)
    assert res.returncode == 0, res.stdout + res.stderr
    if "HIPGRAPH-REFUSED" in res.stdout:
        pytest.skip("hipGraph capture refused on this runtime")
    assert "HIPGRAPH-OK" in res.stdout
