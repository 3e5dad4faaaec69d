"""Row reuse in the host-tier gather (`gather_n(reuse=True)`): cold rows
that one of the last two reusing gathers also fetched are copied from that
gather's output in HBM.  Every result is compared with `torch.equal`
against plain CPU indexing of the store's contents."""
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
# the capped host-tier grid takes 112 blocks x 8 rows = 896 rows per sweep
# at 400 B, so ~2000 ids cover the grid-stride wrap
BATCH = 2000

ROW_TYPES = [
    (torch.float32, 100),   # 400 B, 16 B vectors, 25 of 32 lanes
    (torch.bfloat16, 100),  # 200 B, 8 B vectors
    (torch.float32, 128),   # 512 B
    (torch.bfloat16, 7),    # 14 B, byte path
]
ROW_IDS = ["f32x100", "bf16x100", "f32x128", "bf16x7"]
row_types = pytest.mark.parametrize("dtype,dim", ROW_TYPES, ids=ROW_IDS)


class Store:
    """3000 hot rows in HBM + 5000 rows in a pinned-host shard, addressed
    through a random id -> row permutation.  `rows` mirrors the contents."""

    def __init__(self, dtype=torch.float32, dim=100, seed=21):
        g = torch.Generator().manual_seed(seed)
        self.rows = torch.randn(N_ROWS, dim, generator=g).to(dtype)
        self.order = torch.randperm(N_ROWS, generator=g)
        # id 0 is what zeroed frontier slack points at: keep it cold
        if self.order[0] < N_HOT:
            j = int((self.order >= N_HOT).nonzero()[0])
            self.order[[0, j]] = self.order[[j, 0]]
        self.order_dev = self.order.cuda()
        self.st = ShardTensor(0, ShardTensorConfig({}))
        self.st.append(self.rows[:N_HOT].clone(), 0)
        self.st.append(self.rows[N_HOT:].clone(), -1)
        self.cold_ids = (self.order >= N_HOT).nonzero().flatten()
        self.hot_ids = (self.order < N_HOT).nonzero().flatten()

    def expect(self, ids):
        return self.rows[self.order[ids]]

    def gather(self, ids_dev, n=None, reuse=True):
        n = ids_dev.numel() if n is None else n
        n_dev = torch.tensor([n], dtype=torch.int64, device="cuda")
        return self.st.gather_n(ids_dev, n_dev, self.order_dev, reuse=reuse)


def _pick(pool, k, g):
    return pool[torch.randperm(pool.numel(), generator=g)[:k]]


def _chained_batches(store, n_batches=8, seed=3):
    """Id lists as consecutive mini-batches produce them: about a third of
    the previous batch's ids, a sixth of the batch before, some ids last
    seen three batches ago, fresh cold ids and hot ids."""
    g = torch.Generator().manual_seed(seed)
    batches = []
    for b in range(n_batches):
        parts = []
        if b >= 1:
            parts.append(_pick(batches[b - 1], BATCH // 3, g))
        if b >= 2:
            parts.append(_pick(batches[b - 2], BATCH // 6, g))
        if b >= 3:
            parts.append(_pick(batches[b - 3], BATCH // 12, g))
        parts.append(_pick(store.hot_ids, BATCH // 5, g))
        have = sum(p.numel() for p in parts)
        parts.append(_pick(store.cold_ids, BATCH + 37 - have, g))
        ids = torch.cat(parts)
        batches.append(ids[torch.randperm(ids.numel(), generator=g)])
    return batches


@row_types
def test_chain_on_one_stream(dtype, dim):
    store = Store(dtype, dim)
    for b, ids in enumerate(_chained_batches(store)):
        out = store.gather(ids.cuda())
        assert torch.equal(out.cpu(), store.expect(ids)), f"batch {b}"


@row_types
def test_chain_on_two_alternating_streams(dtype, dim):
    """No synchronisation between the calls, as the prefetcher issues them."""
    store = Store(dtype, dim)
    batches = _chained_batches(store)
    ids_dev = [ids.cuda() for ids in batches]
    n_dev = [torch.tensor([ids.numel()], dtype=torch.int64, device="cuda")
             for ids in batches]
    torch.cuda.synchronize()
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    outs = []
    for b in range(len(batches)):
        with torch.cuda.stream(streams[b % 2]):
            outs.append(store.st.gather_n(ids_dev[b], n_dev[b],
                                          store.order_dev, reuse=True))
    torch.cuda.synchronize()
    for b, ids in enumerate(batches):
        assert torch.equal(outs[b].cpu(), store.expect(ids)), f"batch {b}"


def _window_scenario(reuse, expect_reuse):
    """Batches B-3, B-2, B-1 with disjoint cold sets, each output then
    changed in place (+4, +2, +1), then batch B over all of them.  Returns
    nothing; asserts what batch B reads."""
    store = Store()
    g = torch.Generator().manual_seed(4)
    cold = _pick(store.cold_ids, 4 * 600, g)
    c3, c2, c1, fresh = cold.split(600)
    hot = _pick(store.hot_ids, 400, g)
    outs = []
    for part, bump in ((c3, 4), (c2, 2), (c1, 1)):
        ids = torch.cat([part, _pick(store.hot_ids, 300, g)])
        out = store.gather(ids.cuda(), reuse=reuse)
        assert torch.equal(out.cpu(), store.expect(ids))
        out += bump  # same stream as the gather, ordered before batch B
        outs.append(out)
    ids_b = torch.cat([c1, c2, c3, fresh, hot])
    got = store.gather(ids_b.cuda(), reuse=reuse).cpu()
    g1, g2, g3, gf, gh = got.split([600, 600, 600, 600, 400])
    if expect_reuse:
        # the source really is the previous output: its modified rows
        assert torch.equal(g1, outs[2][:600].cpu())
        assert torch.equal(g2, outs[1][:600].cpu())
        assert not torch.equal(g1, store.expect(c1))
    else:
        assert torch.equal(g1, store.expect(c1))
        assert torch.equal(g2, store.expect(c2))
    # the window is two: three batches ago comes from the store again
    assert torch.equal(g3, store.expect(c3))
    assert torch.equal(gf, store.expect(fresh))
    assert torch.equal(gh, store.expect(hot))


def test_source_is_previous_output_and_window_is_two():
    _window_scenario(reuse=True, expect_reuse=True)


def test_reuse_false_reads_the_store():
    _window_scenario(reuse=False, expect_reuse=False)


def test_env_switch_forces_reuse_off():
    """QUIVER_GATHER_REUSE=0 is read once per process: child process."""
    env = dict(os.environ)
    env["QUIVER_GATHER_REUSE"] = "0"
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env["PYTHONPATH"] = root + os.pathsep + env.get("PYTHONPATH", "")
    res = subprocess.run([sys.executable, os.path.abspath(__file__)],
                         env=env, capture_output=True, text=True,
                         timeout=300, cwd=root)
    assert res.returncode == 0, res.stdout + res.stderr
    assert "REUSE-OFF-OK" in res.stdout


@row_types
def test_sources_outlive_python_references(dtype, dim):
    """Drop every reference to the outputs a gather will read, hand the
    allocator same-sized requests on both streams, then gather."""
    store = Store(dtype, dim)
    batches = _chained_batches(store, n_batches=6)
    ids_dev = [ids.cuda() for ids in batches]
    torch.cuda.synchronize()
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    got = [torch.empty(ids.numel(), dim, dtype=dtype).pin_memory()
           for ids in batches]
    for b in range(len(batches)):  # nothing in here waits for the GPU
        with torch.cuda.stream(streams[b % 2]):
            out = store.gather(ids_dev[b])
            got[b].copy_(out, non_blocking=True)
        shape = out.shape
        del out
        junk = []
        for s in streams:
            with torch.cuda.stream(s):
                junk.append(torch.full(shape, 7.0, dtype=dtype,
                                       device="cuda"))
        del junk
    torch.cuda.synchronize()
    for b, ids in enumerate(batches):
        assert torch.equal(got[b], store.expect(ids)), f"batch {b}"


@row_types
def test_duplicate_ids(dtype, dim):
    store = Store(dtype, dim)
    g = torch.Generator().manual_seed(6)
    same = store.cold_ids[1234].repeat(64)
    for _ in range(2):
        assert torch.equal(store.gather(same.cuda()).cpu(),
                           store.expect(same))
    dup = _pick(store.cold_ids, 10, g).repeat_interleave(30)
    ids = torch.cat([dup, _pick(store.cold_ids, 1500, g),
                     _pick(store.hot_ids, 200, g), same])
    ids = ids[torch.randperm(ids.numel(), generator=g)]
    for _ in range(3):
        assert torch.equal(store.gather(ids.cuda()).cpu(), store.expect(ids))


@row_types
def test_scatter_update_retires_sources(dtype, dim):
    store = Store(dtype, dim)
    g = torch.Generator().manual_seed(7)
    shared = _pick(store.cold_ids, 700, g)
    ids_a = torch.cat([shared, _pick(store.hot_ids, 300, g)])
    out_a = store.gather(ids_a.cuda())
    assert torch.equal(out_a.cpu(), store.expect(ids_a))
    changed = shared[:250]
    rows = store.order[changed]
    new = torch.randn(250, dim, generator=g).to(dtype)
    store.st.shard_tensor.scatter_update(rows.cuda(), new.cuda())
    store.rows[rows] = new
    ids_b = torch.cat([_pick(store.cold_ids, 800, g), shared])
    out_b = store.gather(ids_b.cuda())
    assert torch.equal(out_b.cpu(), store.expect(ids_b))
    # and reuse resumes from batch B on
    out_c = store.gather(ids_b.cuda())
    assert torch.equal(out_c.cpu(), store.expect(ids_b))


@row_types
def test_device_side_count(dtype, dim):
    """B-1 has 1000 of 4096 slots valid and zeroed slack; its slack rows
    are never written, so they must not become sources for batch B, which
    asks for the slack's id (0) and more."""
    store = Store(dtype, dim)
    g = torch.Generator().manual_seed(8)
    pool = store.cold_ids[store.cold_ids != 0]
    ids_a = torch.zeros(4096, dtype=torch.int64)
    ids_a[:1000] = _pick(pool, 1000, g)
    out_a = store.gather(ids_a.cuda(), n=1000)
    assert out_a.shape[0] == 4096
    assert torch.equal(out_a[:1000].cpu(), store.expect(ids_a[:1000]))
    out_a[1000:] = 3.0  # what a wrongly created entry would hand on
    ids_b = torch.cat([ids_a[:500], torch.zeros(96, dtype=torch.int64),
                       _pick(pool, 3000, g), _pick(store.hot_ids, 500, g)])
    assert ids_b.numel() == 4096
    out_b = store.gather(ids_b.cuda())
    assert torch.equal(out_b.cpu(), store.expect(ids_b))


@pytest.mark.parametrize("reuse_rows", [True, False])
def test_prefetcher(small_graph, reuse_rows):
    indptr, indices = small_graph
    topo = quiver.CSRTopo(indptr=indptr, indices=indices)
    n = topo.node_count
    g = torch.Generator().manual_seed(9)
    feat_cpu = torch.randn(n, 100, generator=g)
    feature = quiver.Feature(0, device_list=[0], device_cache_size="40K",
                             cache_policy="device_replicate", csr_topo=topo)
    feature.from_cpu_tensor(feat_cpu.clone())
    assert sorted(
        feature._shard_tensor().shard_tensor.shard_devices()) == [-1, 0]
    sampler = quiver.GraphSageSampler(topo, [5, 3], device=0, mode="GPU")
    batches = [torch.randint(0, n, (64,), generator=g) for _ in range(6)]
    seen = 0
    for n_id, bs, adjs, x in quiver.TrainingPrefetcher(
            sampler, feature, batches, depth=2, device=0, num_streams=2,
            reuse_rows=reuse_rows):
        torch.cuda.synchronize()
        assert torch.equal(x.cpu(), feat_cpu[n_id.cpu()]), f"batch {seen}"
        seen += 1
    assert seen == 6


if __name__ == "__main__":
    # child of test_env_switch_forces_reuse_off
    _window_scenario(reuse=True, expect_reuse=False)
    print("REUSE-OFF-OK")
