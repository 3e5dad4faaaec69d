"""The sampler's own count scan, attached to each hop's edge_index as the
dst segment pointer, must be exactly what searchsorted rebuilds from the
dst-sorted edge list — for every way a batch can be produced."""
import numpy as np
import pytest
import torch

import quiver
from quiver.nn import GATConv, SAGEConv
from quiver.pyg.sage_sampler import DST_PTR_ATTR

pytestmark = pytest.mark.gpu

FANOUTS = [3, 2]
N_NODES = 2000


@pytest.fixture(scope="module")
def topo():
    """~2000 nodes whose degrees cycle through 0, below / equal to / far
    above both fanouts."""
    rng = np.random.default_rng(7)
    pattern = np.array([0, 1, 2, 3, 0, 5, 2, 60, 3, 1], dtype=np.int64)
    degs = pattern[np.arange(N_NODES) % pattern.size]
    indptr = np.zeros(N_NODES + 1, dtype=np.int64)
    indptr[1:] = np.cumsum(degs)
    indices = rng.integers(0, N_NODES, indptr[-1], dtype=np.int64)
    return quiver.CSRTopo(indptr=torch.from_numpy(indptr),
                          indices=torch.from_numpy(indices))


def _seed_batches():
    g = torch.Generator().manual_seed(3)
    # hop 0 has no device-side count: its upper bound IS the seed count,
    # so every batch reads the scan's extra slot at index n_seeds.  The
    # batches differ in what sits last: a zero-degree seed, a seed far
    # above the fanout, a single seed.
    return [
        torch.randint(0, N_NODES, (257,), generator=g),
        torch.cat([torch.randint(0, N_NODES, (63,), generator=g),
                   torch.tensor([0])]),          # degree 0 last
        torch.cat([torch.randint(0, N_NODES, (100,), generator=g),
                   torch.tensor([7])]),          # degree 60 last
        torch.tensor([4]),                       # one zero-degree seed
    ]


def _check_adjs(adjs, batch_size):
    assert int(adjs[-1].size[1]) == batch_size
    for adj in adjs:
        ei = adj.edge_index
        n_dst = int(adj.size[1])
        ptr = getattr(ei, DST_PTR_ATTR, None)
        assert ptr is not None, "no dst_ptr attached"
        assert ptr.dtype == torch.int64 and ptr.device == ei.device
        assert ptr.numel() == n_dst + 1
        ref = torch.searchsorted(
            ei[1].contiguous(), torch.arange(n_dst + 1, device=ei.device))
        assert torch.equal(ptr, ref)
        assert int(ptr[-1]) == ei.size(1)
        assert int(ptr[0]) == 0


@pytest.mark.parametrize("mode", ["GPU", "UVA"])
def test_sample_attaches_exact_dst_ptr(topo, mode):
    sampler = quiver.GraphSageSampler(topo, FANOUTS, device=0, mode=mode)
    for seeds in _seed_batches():
        n_id, bs, adjs = sampler.sample(seeds)
        assert len(adjs) == len(FANOUTS)
        _check_adjs(adjs, seeds.numel())


def test_sample_async_finalize_attaches_exact_dst_ptr(topo):
    sampler = quiver.GraphSageSampler(topo, FANOUTS, device=0, mode="GPU")
    for seeds in _seed_batches():
        tok = sampler.sample_async(seeds)
        torch.cuda.synchronize()
        n_id, bs, adjs = sampler.sample_finalize(tok)
        _check_adjs(adjs, seeds.numel())


@pytest.mark.parametrize("num_streams", [1, 2])
def test_prefetcher_batches_carry_exact_dst_ptr(topo, num_streams):
    sampler = quiver.GraphSageSampler(topo, FANOUTS, device=0, mode="GPU")
    batches = _seed_batches()[:3]
    pf = quiver.TrainingPrefetcher(sampler, None, batches, depth=2,
                                   device=0, num_streams=num_streams)
    seen = 0
    for (n_id, bs, adjs, x), seeds in zip(pf, batches):
        torch.cuda.synchronize()
        assert bs == seeds.numel()
        _check_adjs(adjs, seeds.numel())
        seen += 1
    assert seen == 3


def test_layers_agree_without_the_attribute(topo):
    """edge_index.clone() drops the attribute; the layers then rebuild the
    pointer from the edge list and must produce the same output."""
    sampler = quiver.GraphSageSampler(topo, FANOUTS, device=0, mode="GPU")
    seeds = _seed_batches()[0]
    n_id, bs, adjs = sampler.sample(seeds)
    ei, _, size = adjs[0]
    bare = ei.clone()
    assert getattr(bare, DST_PTR_ATTR, None) is None
    torch.manual_seed(0)
    x = torch.randn(n_id.numel(), 32, device="cuda")
    x_dst = x[:int(size[1])]
    sage = SAGEConv(32, 16, sorted_dst=True).cuda()
    gat = GATConv(32, 8, heads=2, sorted_dst=True).cuda()
    with torch.no_grad():
        for conv in (sage, gat):
            a = conv((x, x_dst), ei, size)
            b = conv((x, x_dst), bare, size)
            assert torch.equal(a, b)
