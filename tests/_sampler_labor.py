"""Shared by test_cpu_sampler_labor.py and test_gpu_sampler_labor.py: the
graphs, the model and the checks of GraphSageSampler.sample_labor, the same
in every mode.  The keep rule is integer arithmetic on a documented variate,
so every comparison with the model is exact."""
import functools

import numpy as np
import pytest
import torch

import quiver
from quiver import _ext
from quiver.pyg.sage_sampler import DST_PTR_ATTR
from _sampler_walks import topo_from_rows

M64 = 2 ** 64 - 1
G = 0x9e3779b97f4a7c15
HOP = 0x632be59bd9b4e019
SEED = 1234
N_S = 3000
EID_MODES = [(False, False), (True, False), (True, True)]  # return_eid, eid
# (fanouts, layer_dependency)
DRAWS = [((3,), False), ((16,), False), ((-1,), False), ((4, 3), False),
         ((4, 3), True)]
long = functools.partial(torch.tensor, dtype=torch.long)


def splitmix64(x):
    x = (x + G) & M64
    x = ((x ^ (x >> 30)) * 0xbf58476d1ce4e5b9) & M64
    x = ((x ^ (x >> 27)) * 0x94d049bb133111eb) & M64
    return x ^ (x >> 31)


def model(topo, nodes, sizes, word, layer_dependency, with_ids):
    """[(frontier, edge_index, dst_ptr, e_id)] per hop, hop 0 first."""
    indptr, indices = topo.indptr.tolist(), topo.indices.tolist()
    eid = None if topo.eid is None else topo.eid.tolist()
    cur, hops = list(nodes), []
    for h, k in enumerate(sizes):
        key = splitmix64(
            word if layer_dependency else (word + (h + 1) * HOP) & M64)
        local = {}
        for v in cur:
            local.setdefault(v, len(local))
        src, dst, ids, ptr = [], [], [], [0]
        for i, s in enumerate(cur):
            d = indptr[s + 1] - indptr[s]
            for j in range(indptr[s], indptr[s + 1]):
                r = splitmix64((key + indices[j] * G) & M64)
                if k < 0 or d <= k or (r * d) >> 64 < k:
                    src.append(local.setdefault(indices[j], len(local)))
                    dst.append(i)
                    ids.append(j if eid is None else eid[j])
            ptr.append(len(src))
        cur = list(local)
        hops.append((long(cur), long([src, dst]), long(ptr),
                     long(ids if with_ids else [])))
    return hops


@functools.lru_cache(None)
def structure_graph(eid):
    """(graph, seed batch).  Nodes 0..17 have the degrees below: 0, 1, one
    below, at and above every fanout of DRAWS, a 16-lane step, a mask word
    and one and two chunks, and two hubs.  Neighbours are drawn with repeats
    from few nodes, so rows share sources and hold edges twice."""
    c = _ext.labor_chunk_slots()
    degrees = [0, 1, 2, 3, 4, 5, 15, 16, 17, 63, 64, 65, c - 1, c, c + 1,
               2 * c + 1, 1000, 5000]
    rng = np.random.default_rng(31)
    degrees += list(rng.integers(0, 9, N_S - len(degrees)))
    return topo_from_rows([rng.integers(0, N_S, d) for d in degrees], eid), \
        list(range(18)) + [7, 2500]                 # a seed given twice


@functools.lru_cache(None)
def shared_graph():
    """Rows 0..7 hold the same 200 neighbours, row 8 the first 100."""
    row = np.random.default_rng(32).permutation(N_S)[:200]
    rows = [row] * 8 + [row[:100]] + [[]] * (N_S - 9)
    return topo_from_rows(rows)


@functools.lru_cache(None)
def rate_graph():
    """4096 rows of 64 pairwise distinct neighbours."""
    n = 4096 + 4096 * 64
    indptr = torch.clamp(torch.arange(n + 1) * 64, max=4096 * 64)
    return quiver.CSRTopo(indptr=indptr, indices=4096 + torch.arange(4096 * 64))


@functools.lru_cache(None)
def expected(sizes, layer_dependency, return_eid, eid):
    topo, seeds = structure_graph(eid)
    return model(topo, seeds, sizes, SEED + G, layer_dependency, return_eid)


def make_sampler(topo, mode, sizes, seed=SEED, **kw):
    s = quiver.GraphSageSampler(topo, list(sizes), device=0, mode=mode, **kw)
    s.lazy_init_quiver()
    s.quiver.set_seed(seed)
    return s


def check_batch(sampler, batch, seeds, want):
    """`batch` against the model's hops, exactly, in sample()'s layout."""
    n_id, batch_size, adjs = batch
    device = "cpu" if sampler.mode == "CPU" else "cuda"
    assert batch_size == len(seeds) and len(adjs) == len(want)
    assert torch.equal(n_id.cpu(), want[-1][0] if want else long(seeds))
    prev = len(seeds)
    for adj, (frontier, edge_index, dst_ptr, e_id) in zip(adjs[::-1], want):
        got = (adj.edge_index, getattr(adj.edge_index, DST_PTR_ATTR))
        got += (adj.e_id,) if sampler.return_eid else ()
        for g, w in zip(got, (edge_index, dst_ptr, e_id)):
            assert g.device.type == device and g.dtype == torch.int64
            assert torch.equal(g.cpu(), w)
        assert sampler.return_eid or adj.e_id.numel() == 0
        assert adj.size.tolist() == [len(frontier), prev]
        prev = len(frontier)


def check_model(mode, sizes, layer_dependency, return_eid, eid):
    topo, seeds = structure_graph(eid)
    s = make_sampler(topo, mode, sizes, return_eid=return_eid)
    want = expected(sizes, layer_dependency, return_eid, eid)
    check_batch(s, s.sample_labor(seeds, layer_dependency), seeds, want)
    kept = torch.diff(want[0][2])       # of hop 0; row 17 is the hub
    assert int(kept.sum()) > 0 and (int(kept[17]) == 5000) == (sizes[0] < 0)


def check_shared(mode):
    """What no per-row independent draw does: equal rows keep equal slots,
    and a prefix row keeps at least what they keep of the prefix."""
    topo = shared_graph()
    s = make_sampler(topo, mode, [10], return_eid=True)
    adj = s.sample_labor(list(range(9)))[2][0]
    ptr = getattr(adj.edge_index, DST_PTR_ATTR).tolist()
    at = [(adj.e_id[ptr[i]:ptr[i + 1]].cpu() - topo.indptr[i]).tolist()
          for i in range(9)]
    assert 0 < len(at[0]) < 200 and all(a == at[0] for a in at[1:8])
    assert {j for j in at[0] if j < 100} <= set(at[8])


def rate_batches(mode):
    """Two calls after one set_seed, twice; returns the first batch."""
    runs = []
    for _ in range(2):
        s = make_sampler(rate_graph(), mode, [16])
        runs.append([s.sample_labor(torch.arange(4096)) for _ in range(2)])
    (a, b), (c, _) = runs
    # 6 sd of Binomial(262144, 1/4), sd = 221.7
    assert abs(a[2][0].edge_index.size(1) - 65536) <= 1331
    assert same_batch(a, c) and not same_batch(a, b)
    return a


def same_batch(a, b):
    return torch.equal(a[0], b[0]) and all(
        torch.equal(x.edge_index, y.edge_index) for x, y in zip(a[2], b[2]))


def check_edges(mode, return_eid):
    """An empty batch and one of zero-degree seeds only."""
    topo, _ = structure_graph(False)
    zero = [i for i in range(N_S) if topo.degree[i] == 0][:3]
    for seeds in ([], zero):
        s = make_sampler(topo, mode, (4, 3), return_eid=return_eid)
        want = model(topo, seeds, (4, 3), SEED + G, False, return_eid)
        batch = s.sample_labor(long(seeds))
        check_batch(s, batch, seeds, want)
        assert tuple(batch[2][0].edge_index.shape) == (2, 0)


def check_refused(mode):
    topo, _ = structure_graph(False)
    w = torch.ones(topo.edge_count)
    with pytest.raises(ValueError):
        make_sampler(topo, mode, [3], edge_weight=w).sample_labor([1, 2])
    s = make_sampler(topo, mode, [3])
    with pytest.raises(ValueError):
        s.sample_labor(torch.tensor([3, N_S]))
    s.sample_labor([3])                 # the sampler works on afterwards


CASES = (
    [(check_model, d + e) for d in DRAWS for e in EID_MODES]
    + [(check_shared, ())]
    + [(check_edges, (r,)) for r in (False, True)]
    + [(check_refused, ())])


def case_id(case):
    return "-".join([case[0].__name__[6:]] + [str(a) for a in case[1]])
