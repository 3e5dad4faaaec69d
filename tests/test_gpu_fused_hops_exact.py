"""The fused multi-hop chain (GpuSampler::sample_hops_raw and everything
built on it) against the exact model of _frontier_model.py.

On the `det` graph no row is longer than a fanout, so the draw copies rows
in CSR order and the whole batch is determined: frontier order, every local
id, the dst pointers, the edge ids, the device-side sizes and the zeroed
slack of the upper-bound buffers are compared with torch.equal.  On the
`mixed` graph (rows of 60 next to the short ones) check_hop_structure pins
everything but the random choice itself."""
import os
import subprocess
import sys

import pytest
import torch

import quiver
from quiver.pyg.sage_sampler import DST_PTR_ATTR

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _frontier_model as fm  # noqa: E402  (shared with the CPU file)

pytestmark = pytest.mark.gpu

MODES = ["GPU", "UVA"]
FANOUTS = [4, 3]


@pytest.fixture(scope="module")
def det():
    indptr, indices = fm.det_graph()
    return quiver.CSRTopo(indptr=indptr, indices=indices)


@pytest.fixture(scope="module")
def mixed():
    indptr, indices = fm.mixed_graph()
    return quiver.CSRTopo(indptr=indptr, indices=indices)


@pytest.fixture(scope="module")
def seeds257(det):
    g = torch.Generator().manual_seed(1)
    return torch.randint(0, det.node_count, (257,), generator=g)


@pytest.fixture(scope="module")
def model257(det, seeds257):
    return fm.hops_model(det.indptr, det.indices, seeds257, FANOUTS)


def _check_batch(model, n_id, adjs, seeds, with_eid=False):
    assert len(adjs) == len(model.hops)
    assert n_id.is_cuda and torch.equal(n_id.cpu(), model.hops[-1].frontier)
    n_dst = seeds.numel()
    for adj, hop in zip(adjs[::-1], model.hops):
        assert torch.equal(adj.edge_index.cpu(), hop.edge_index)
        assert adj.size.tolist() == [hop.frontier.numel(), n_dst]
        ptr = getattr(adj.edge_index, DST_PTR_ATTR, None)
        assert ptr is not None, "no dst_ptr attached"
        assert torch.equal(ptr.cpu(), hop.dst_ptr)
        if with_eid:
            assert torch.equal(adj.e_id.cpu(), hop.e_id)
        n_dst = hop.frontier.numel()


def _check_raw(model, token, seeds, fanouts):
    """The upper-bound buffers of a sample_async token: true sizes on the
    device, frontier slack zero, pointer slack constant at m_h."""
    _, raw, sizes_dev, _, ptrs = token
    assert torch.equal(sizes_dev.cpu(), model.sizes)
    n_dst = n_ub = seeds.numel()
    for h, ((f_ub, e_ub), hop, k) in enumerate(zip(raw, model.hops, fanouts)):
        m, u = int(model.sizes[2 * h]), int(model.sizes[2 * h + 1])
        assert f_ub.numel() == n_ub * (k + 1)
        assert e_ub.shape[1] == n_ub * k
        assert ptrs[h].numel() == n_ub + 1
        f_ub, p_ub = f_ub.cpu(), ptrs[h].cpu()
        assert torch.equal(f_ub[:u], hop.frontier)
        assert not f_ub[u:].any(), "frontier slack is not zero"
        assert torch.equal(p_ub[:n_dst + 1], hop.dst_ptr)
        assert bool((p_ub[n_dst:] == m).all()), "a slack dst counted edges"
        n_dst, n_ub = u, n_ub * (k + 1)


def _async(sampler, seeds):
    token = sampler.sample_async(seeds)
    torch.cuda.synchronize()
    return token, sampler.sample_finalize(token)


def _check_structure(topo, seeds, n_id, adjs, fanouts):
    prev = seeds
    for adj, k in zip(adjs[::-1], fanouts):
        assert int(adj.size[1]) == prev.numel()
        frontier = n_id[:int(adj.size[0])].cpu()
        ptr = getattr(adj.edge_index, DST_PTR_ATTR, None)
        assert ptr is not None, "no dst_ptr attached"
        fm.check_hop_structure(prev, frontier, adj.edge_index, ptr,
                               topo.indptr, topo.indices, k)
        prev = frontier


@pytest.mark.parametrize("mode", MODES)
def test_sample_det(det, seeds257, model257, mode):
    s = quiver.GraphSageSampler(det, FANOUTS, device=0, mode=mode)
    n_id, bs, adjs = s.sample(seeds257)
    assert bs == 257
    _check_batch(model257, n_id, adjs, seeds257)


@pytest.mark.parametrize("mode", MODES)
def test_sample_det_csr_slot_ids(det, seeds257, model257, mode):
    """return_eid on a topo without an id map: ids are CSR slots."""
    s = quiver.GraphSageSampler(det, FANOUTS, device=0, mode=mode,
                                return_eid=True)
    n_id, _, adjs = s.sample(seeds257)
    _check_batch(model257, n_id, adjs, seeds257, with_eid=True)


@pytest.mark.parametrize("mode", MODES)
def test_sample_det_coo_ids(det, seeds257, mode):
    """return_eid on a topo built from a shuffled COO edge_index: ids are
    positions in that edge_index."""
    coo = fm.shuffled_coo(det.indptr, det.indices)
    topo = quiver.CSRTopo(coo, node_count=det.node_count)
    assert topo.eid is not None
    s = quiver.GraphSageSampler(topo, FANOUTS, device=0, mode=mode,
                                return_eid=True)
    n_id, _, adjs = s.sample(seeds257)
    model = fm.hops_model(topo.indptr, topo.indices, seeds257, FANOUTS,
                          eid=topo.eid)
    _check_batch(model, n_id, adjs, seeds257, with_eid=True)
    n_id = n_id.cpu()
    prev = seeds257      # repeats: the seed hop's dsts are seed positions
    for adj in adjs[::-1]:
        src, dst = adj.edge_index.cpu()
        e_id = adj.e_id.cpu()
        assert torch.equal(coo[0, e_id], prev[dst])
        assert torch.equal(coo[1, e_id], n_id[src])
        prev = n_id[:int(adj.size[0])]


@pytest.mark.parametrize("mode", MODES)
def test_async_finalize_det_and_raw_token(det, seeds257, model257, mode):
    s = quiver.GraphSageSampler(det, FANOUTS, device=0, mode=mode)
    token, (n_id, bs, adjs) = _async(s, seeds257)
    assert bs == 257
    _check_batch(model257, n_id, adjs, seeds257)
    assert torch.equal(token[3], model257.sizes)     # the pinned copy
    _check_raw(model257, token, seeds257, FANOUTS)


def test_grid_stride_under_device_counts(det):
    """3 000 seeds under fanouts [12, 3, 4]: the bounds grow to 3 000 /
    39 000 / 156 000 dsts and 780 000 reindex items at the last hop while
    the true counts stay far below, so the row kernels and the reindex
    kernels run second stride iterations that are mostly slack."""
    fanouts = [12, 3, 4]
    g = torch.Generator().manual_seed(4)
    seeds = torch.randperm(det.node_count, generator=g)[:3000]
    model = fm.hops_model(det.indptr, det.indices, seeds, fanouts)
    s = quiver.GraphSageSampler(det, fanouts, device=0, mode="GPU")
    token, (n_id, _, adjs) = _async(s, seeds)
    assert [f.numel() for f, _ in token[1]] == [39000, 156000, 780000]
    assert token[1][2][0].numel() > 2048 * 256
    assert token[4][2].numel() - 1 > 2048 * 16
    _check_batch(model, n_id, adjs, seeds)
    _check_raw(model, token, seeds, fanouts)
    n_id, _, adjs = s.sample(seeds)
    _check_batch(model, n_id, adjs, seeds)


@pytest.mark.parametrize("mode", MODES)
def test_mixed_structure(mixed, mode):
    fanouts = [3, 2]
    s = quiver.GraphSageSampler(mixed, fanouts, device=0, mode=mode)
    for seeds in fm.mixed_seed_batches(mixed.indptr):
        n_id, _, adjs = s.sample(seeds)
        _check_structure(mixed, seeds, n_id, adjs, fanouts)
        _, (n_id, _, adjs) = _async(s, seeds)
        _check_structure(mixed, seeds, n_id, adjs, fanouts)


@pytest.mark.parametrize("mode", MODES)
def test_all_seeds_isolated(det, mode):
    """Every hop has m = 0 and the frontier stays the seeds."""
    seeds = fm.nodes_of_degree(det.indptr, 0)[:257]
    model = fm.hops_model(det.indptr, det.indices, seeds, FANOUTS)
    assert model.sizes.tolist() == [0, 257, 0, 257]
    s = quiver.GraphSageSampler(det, FANOUTS, device=0, mode=mode)
    n_id, _, adjs = s.sample(seeds)
    _check_batch(model, n_id, adjs, seeds)
    assert torch.equal(n_id.cpu(), seeds)
    token, (n_id, _, adjs) = _async(s, seeds)
    _check_batch(model, n_id, adjs, seeds)
    _check_raw(model, token, seeds, FANOUTS)


@pytest.mark.parametrize("mode", MODES)
def test_edgeless_graph(mode):
    """Five nodes and no edge: every per-edge column the engine places
    (indices, id map, times) is empty, and a batch is its seeds."""
    indptr = torch.zeros(6, dtype=torch.int64)
    none = torch.zeros(0, dtype=torch.int64)
    topo = quiver.CSRTopo(indptr=indptr, indices=none)
    seeds = torch.tensor([3, 0, 4])
    model = fm.hops_model(indptr, none, seeds, FANOUTS)
    assert model.sizes.tolist() == [0, 3, 0, 3]
    s = quiver.GraphSageSampler(topo, FANOUTS, device=0, mode=mode,
                                return_eid=True, edge_time=none)
    n_id, _, adjs = s.sample(seeds)
    _check_batch(model, n_id, adjs, seeds, with_eid=True)
    token, (n_id, _, adjs) = _async(s, seeds)
    _check_batch(model, n_id, adjs, seeds, with_eid=True)
    _check_raw(model, token, seeds, FANOUTS)
    bound = torch.zeros(3, dtype=torch.int64, device="cuda")
    out, cnt, ids = s.quiver.sample_neighbor_temporal(seeds.cuda(), bound, 3)
    assert out.numel() == 0 and ids.numel() == 0 and cnt.tolist() == [0, 0, 0]


@pytest.mark.parametrize("mode", MODES)
def test_duplicate_seeds(det, mode):
    """Repeated seeds: the first hop's dst ids are seed POSITIONS, its
    frontier holds each seed once."""
    g = torch.Generator().manual_seed(2)
    seeds = torch.randint(0, 40, (100,), generator=g)
    model = fm.hops_model(det.indptr, det.indices, seeds, FANOUTS)
    s = quiver.GraphSageSampler(det, FANOUTS, device=0, mode=mode)
    n_id, _, adjs = s.sample(seeds)
    _check_batch(model, n_id, adjs, seeds)
    assert int(adjs[-1].edge_index[1].max()) >= 40
    token, (n_id, _, adjs) = _async(s, seeds)
    _check_batch(model, n_id, adjs, seeds)
    _check_raw(model, token, seeds, FANOUTS)


@pytest.mark.parametrize("mode", MODES)
def test_per_hop_path_equals_fused_path(det, seeds257, model257, mode):
    s = quiver.GraphSageSampler(det, FANOUTS, device=0, mode=mode)
    n_id, _, adjs = s.sample(seeds257)
    nodes = seeds257.cuda()
    for adj, hop, k in zip(adjs[::-1], model257.hops, FANOUTS):
        out, cnt = s.sample_layer(nodes, k)
        frontier, row, col = s.reindex(nodes, out, cnt)
        edge_index = torch.stack([col, row])
        assert torch.equal(frontier.cpu(), hop.frontier)
        assert torch.equal(edge_index.cpu(), hop.edge_index)
        assert torch.equal(frontier, n_id[:frontier.numel()])
        assert torch.equal(edge_index, adj.edge_index)
        nodes = frontier
    assert torch.equal(nodes, n_id)


REPLAY_SCRIPT = r"""
import os, sys, warnings
import torch
import quiver
from quiver.pyg.sage_sampler import DST_PTR_ATTR
sys.path.insert(0, os.path.join(os.getcwd(), "tests"))
import _frontier_model as fm

os.environ["QUIVER_HIPGRAPH"] = "1"
FANOUTS = [4, 3]
B = 257
indptr, indices = fm.det_graph()
topo = quiver.CSRTopo(indptr=indptr, indices=indices)
s = quiver.GraphSageSampler(topo, FANOUTS, device=0, mode="GPU")
g = torch.Generator().manual_seed(6)
n = topo.node_count


def rand():
    return torch.randint(0, n, (B,), generator=g)


def of_degree(d):
    pool = fm.nodes_of_degree(indptr, d)
    return pool[torch.randperm(pool.numel(), generator=g)[:B]]


# batch 0 runs eagerly, then the three slots take batches 1 / 2 / 3 and
# again 4 / 5: the isolated batch 4 directly follows a dense one and
# replays the slot that last held the dense batch 1
batches = [rand(), of_degree(3), rand(), of_degree(3), of_degree(0), rand()]
assert all(b.numel() == B for b in batches)
seen = 0
with warnings.catch_warnings(record=True) as caught:
    warnings.simplefilter("always")
    for (n_id, bs, adjs, x), seeds in zip(
            quiver.TrainingPrefetcher(s, None, batches, depth=2, device=0,
                                      num_streams=1), batches):
        torch.cuda.synchronize()
        model = fm.hops_model(indptr, indices, seeds, FANOUTS)
        assert bs == B and x is None
        assert torch.equal(n_id.cpu(), model.hops[-1].frontier), seen
        n_dst = B
        for adj, hop in zip(adjs[::-1], model.hops):
            assert torch.equal(adj.edge_index.cpu(), hop.edge_index), seen
            assert adj.size.tolist() == [hop.frontier.numel(), n_dst], seen
            ptr = getattr(adj.edge_index, DST_PTR_ATTR)
            assert torch.equal(ptr.cpu(), hop.dst_ptr), seen
            n_dst = hop.frontier.numel()
        seen += 1
assert seen == 6
refused = any("capture failed" in str(m.message)
              or "replay failed" in str(m.message) for m in caught)
print("HIPGRAPH-REFUSED" if refused else "HIPGRAPH-OK")
"""


def test_captured_replay_equals_model():
    """Six equal-length batches through the prefetcher's captured slots:
    every yielded batch must be the model's batch of its own seeds, so no
    size, pointer, frontier tail or table state may survive from one
    replay into the next.  In a process of its own, like the other capture
    tests; where the runtime refuses the capture the prefetcher runs
    uncaptured and the same assertions hold."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    res = subprocess.run([sys.executable, "-c", REPLAY_SCRIPT],
                         env=dict(os.environ), capture_output=True,
                         text=True, timeout=300, cwd=root)
    print(res.stdout)
    assert res.returncode == 0, res.stdout + res.stderr
    assert "HIPGRAPH-" in res.stdout
