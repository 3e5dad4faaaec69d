"""Shared by test_cpu_sampler_edges.py and test_gpu_sampler_edges.py: the
graphs, the exact edge-id checks and the exact successive-sampling model
that the edge-id / edge-weight sampler tests use in every mode."""
import itertools

import numpy as np
import torch

import quiver

FANOUTS = [4, 3]
T = 20000          # repeated seeds per distribution case


def coo_graph(seed=0, nodes=300, edges=6000):
    """Random COO graph from torch.randint: multi-edges and self-loops.
    The mean degree is 20, so a plain draw leaves almost no row at or
    under the fanouts 4 and 3; nodes 0..5 (all among the tests' seeds) are
    therefore cut down to 0..5 out-edges, the surplus moved to nodes
    6..11, which puts degrees on both sides of the fanout for certain."""
    g = torch.Generator().manual_seed(seed)
    coo = torch.randint(0, nodes, (2, edges), generator=g)
    src = coo[0]
    for v in range(6):
        at = (src == v).nonzero().flatten()
        src[at[v:]] = 6 + v
    return coo


def hop_pairs(adjs, sizes):
    """(adj, fanout) from the seeds' hop outward."""
    return list(zip(adjs[::-1], sizes))


def check_coo_ids(coo, topo, n_id, adjs, sizes):
    """The issue's exact checks for a topo whose ids are COO positions."""
    n_id = n_id.cpu()
    deg = topo.degree
    E = coo.shape[1]
    assert len(adjs) == len(sizes)
    for adj, k in hop_pairs(adjs, sizes):
        ei, e_id = adj.edge_index.cpu(), adj.e_id.cpu()
        assert adj.e_id.device == adj.edge_index.device
        m = ei.shape[1]
        assert ei.shape[0] == 2
        assert e_id.dtype == torch.int64 and tuple(e_id.shape) == (m,)
        assert m > 0
        assert int(e_id.min()) >= 0 and int(e_id.max()) < E
        assert torch.equal(coo[0, e_id], n_id[ei[1]])
        assert torch.equal(coo[1, e_id], n_id[ei[0]])
        # distinct ids inside each dst segment, although neighbours repeat
        assert torch.unique(ei[1] * E + e_id).numel() == m
        n_dst = int(adj.size[1])
        want = torch.clamp(deg[n_id[:n_dst]], max=k)
        assert torch.equal(torch.bincount(ei[1], minlength=n_dst), want)


def check_csr_ids(topo, n_id, adjs, sizes):
    """Same, for a topo without an eid: ids are CSR slots."""
    n_id = n_id.cpu()
    indptr, indices = topo.indptr, topo.indices
    E = indices.numel()
    for adj, k in hop_pairs(adjs, sizes):
        ei, e_id = adj.edge_index.cpu(), adj.e_id.cpu()
        m = ei.shape[1]
        assert e_id.dtype == torch.int64 and tuple(e_id.shape) == (m,)
        assert m > 0
        assert int(e_id.min()) >= 0 and int(e_id.max()) < E
        v = n_id[ei[1]]
        assert torch.equal(indices[e_id], n_id[ei[0]])
        assert bool((indptr[v] <= e_id).all())
        assert bool((e_id < indptr[v + 1]).all())
        assert torch.unique(ei[1] * E + e_id).numel() == m
        n_dst = int(adj.size[1])
        want = torch.clamp(topo.degree[n_id[:n_dst]], max=k)
        assert torch.equal(torch.bincount(ei[1], minlength=n_dst), want)


def shuffled_csr_graph(seed=3, nodes=200):
    """COO graph whose edge order is a random shuffle of CSR order, every
    node of degree 5..20, plus one chosen COO edge per node."""
    g = torch.Generator().manual_seed(seed)
    deg = torch.randint(5, 21, (nodes,), generator=g)
    src = torch.repeat_interleave(torch.arange(nodes), deg)
    dst = torch.randint(0, nodes, (src.numel(),), generator=g)
    perm = torch.randperm(src.numel(), generator=g)
    coo = torch.stack([src[perm], dst[perm]])
    chosen = torch.empty(nodes, dtype=torch.long)
    for v in range(nodes):
        own = (coo[0] == v).nonzero().flatten()
        chosen[v] = own[int(torch.randint(0, own.numel(), (1,),
                                          generator=g))]
    return coo, chosen


def star_topo(n_nbrs):
    """Node 0 with neighbours 1..n_nbrs, nothing else; ids = CSR slots =
    neighbour - 1."""
    indptr = torch.tensor([0] + [n_nbrs] * (n_nbrs + 1), dtype=torch.long)
    indices = torch.arange(1, n_nbrs + 1, dtype=torch.long)
    return quiver.CSRTopo(indptr=indptr, indices=indices)


def inclusion_probs(w, k):
    """Exact inclusion probabilities of successive sampling without
    replacement: enumerate every ordered k-tuple."""
    w = [float(x) for x in w]
    pi = np.zeros(len(w))
    for tup in itertools.permutations(range(len(w)), k):
        p, rest = 1.0, sum(w)
        for i in tup:
            p *= w[i] / rest
            rest -= w[i]
        for i in tup:
            pi[i] += p
    return pi


def assert_within_6_sigma(count, trials, pi):
    """The rule of tests/test_gpu_sampler.py: |freq/T - pi| < 6 sigma."""
    pi = np.asarray(pi, dtype=np.float64)
    p = np.asarray(count, dtype=np.float64) / trials
    sigma = np.sqrt(pi * (1 - pi) / trials)
    z = np.abs(p - pi) / sigma
    print("freq", p, "pi", pi, "z", z)
    assert np.all(z < 6), (p, pi, z)


def star_draw_counts(mode, weights, k, seed=4321):
    """Draw k of the star's edges T times (node 0 repeated as seeds) and
    count how often each edge id came out.  Also checks every row holds k
    distinct ids."""
    n = len(weights)
    topo = star_topo(n)
    s = quiver.GraphSageSampler(topo, [k], device=0, mode=mode,
                                return_eid=True,
                                edge_weight=torch.as_tensor(
                                    weights, dtype=torch.float32))
    s.lazy_init_quiver()
    if mode != "CPU":
        s.quiver.set_seed(seed)
    n_id, bs, adjs = s.sample(torch.zeros(T, dtype=torch.long))
    ei, e_id = adjs[0].edge_index.cpu(), adjs[0].e_id.cpu()
    assert tuple(e_id.shape) == (T * k,)
    assert torch.equal(torch.bincount(ei[1], minlength=T),
                       torch.full((T,), k))
    assert torch.unique(ei[1] * n + e_id).numel() == T * k
    assert torch.equal(n_id.cpu()[ei[0]], e_id + 1)
    return np.bincount(e_id.numpy(), minlength=n)


HUB_CLASSES, HUB_PER_CLASS = 6, 500


def hub_weights():
    c = torch.arange(HUB_CLASSES * HUB_PER_CLASS) // HUB_PER_CLASS
    return (2.0 ** c).float()


def distribution_case(mode, case):
    """The four distribution cases of the issue, by name."""
    if case == "w1to8_k1":
        w = np.arange(1, 9, dtype=np.float64)
        assert_within_6_sigma(star_draw_counts(mode, w, 1), T, w / 36)
    elif case == "w1to8_k3":
        w = np.arange(1, 9, dtype=np.float64)
        pi = inclusion_probs(w, 3)
        assert abs(pi.sum() - 3) < 1e-9
        assert_within_6_sigma(star_draw_counts(mode, w, 3), T, pi)
    elif case == "ones64_k8":
        assert_within_6_sigma(star_draw_counts(mode, np.ones(64), 8), T,
                              np.full(64, 1 / 8))
    elif case == "hub3000_k1":
        cnt = star_draw_counts(mode, hub_weights().numpy(), 1)
        per_class = cnt.reshape(HUB_CLASSES, HUB_PER_CLASS).sum(1)
        share = 2.0 ** np.arange(HUB_CLASSES) / 63
        assert_within_6_sigma(per_class, T, share)
    else:
        raise AssertionError(case)


DISTRIBUTION_CASES = ["w1to8_k1", "w1to8_k3", "ones64_k8", "hub3000_k1"]


def check_hub_k16(mode):
    topo = star_topo(3000)
    s = quiver.GraphSageSampler(topo, [16], device=0, mode=mode,
                                return_eid=True, edge_weight=hub_weights())
    rows = 64
    n_id, bs, adjs = s.sample(torch.zeros(rows, dtype=torch.long))
    ei, e_id = adjs[0].edge_index.cpu(), adjs[0].e_id.cpu()
    assert tuple(e_id.shape) == (rows * 16,)
    assert int(e_id.min()) >= 0 and int(e_id.max()) < 3000
    assert torch.unique(ei[1] * 3000 + e_id).numel() == rows * 16
    assert torch.equal(torch.bincount(ei[1], minlength=rows),
                       torch.full((rows,), 16))
    assert torch.equal(n_id.cpu()[ei[0]], topo.indices[e_id])


def check_short_rows_unweighted(mode, small_graph):
    """deg <= k: all neighbours in CSR order, equal to the unweighted
    result."""
    indptr, indices = small_graph
    topo = quiver.CSRTopo(indptr=indptr, indices=indices)
    k = int(topo.degree.max())
    g = torch.Generator().manual_seed(5)
    w = torch.rand(topo.edge_count, generator=g) + 0.5
    seeds = torch.arange(topo.node_count)
    a = quiver.GraphSageSampler(topo, [k], device=0, mode=mode,
                                edge_weight=w)
    b = quiver.GraphSageSampler(topo, [k], device=0, mode=mode)
    out_a, cnt_a = a.sample_layer(seeds, k)
    out_b, cnt_b = b.sample_layer(seeds, k)
    assert torch.equal(cnt_a.cpu(), topo.degree)
    assert torch.equal(out_a.cpu(), indices)
    assert torch.equal(out_a.cpu(), out_b.cpu())
    assert torch.equal(cnt_a.cpu(), cnt_b.cpu())


def check_permutation(mode):
    coo, chosen = shuffled_csr_graph()
    nodes = chosen.numel()
    topo = quiver.CSRTopo(coo, node_count=nodes)
    # the shuffle must actually disagree with CSR order
    assert not torch.equal(topo.eid, torch.arange(coo.shape[1]))
    w = torch.ones(coo.shape[1])
    w[chosen] = 1e9
    s = quiver.GraphSageSampler(topo, [1], device=0, mode=mode,
                                return_eid=True, edge_weight=w)
    n_id, bs, adjs = s.sample(torch.arange(nodes))
    ei, e_id = adjs[0].edge_index.cpu(), adjs[0].e_id.cpu()
    assert torch.equal(ei[1], torch.arange(nodes))
    assert torch.equal(e_id, chosen)


def check_two_hop_weighted(mode):
    coo = coo_graph()
    topo = quiver.CSRTopo(coo, node_count=300)
    g = torch.Generator().manual_seed(11)
    w = torch.rand(coo.shape[1], generator=g) * 1.5 + 0.5
    s = quiver.GraphSageSampler(topo, FANOUTS, device=0, mode=mode,
                                return_eid=True, edge_weight=w)
    n_id, bs, adjs = s.sample(torch.arange(64))
    assert bs == 64
    check_coo_ids(coo, topo, n_id, adjs, FANOUTS)
