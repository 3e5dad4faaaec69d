"""The frontier model of _frontier_model.py against the CPU engine, on small
versions of the cases the GPU files run: a mismatch on the GPU then points
at a kernel, not at the model.  Every assertion is exact."""
import os
import sys

import numpy as np
import pytest
import torch

import quiver

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _frontier_model as fm  # noqa: E402  (shared with the GPU files)

N_SMALL = 600


@pytest.fixture(scope="module")
def det():
    indptr, indices = fm.det_graph(N_SMALL)
    return quiver.CSRTopo(indptr=indptr, indices=indices)


@pytest.fixture(scope="module")
def mixed():
    indptr, indices = fm.mixed_graph(N_SMALL)
    return quiver.CSRTopo(indptr=indptr, indices=indices)


@pytest.fixture(scope="module")
def engine(det):
    s = quiver.GraphSageSampler(det, [3], mode="CPU")
    s.lazy_init_quiver()
    return s


def _check_reindex(engine, seeds, nbrs, counts):
    want = fm.reindex_model(seeds, nbrs, counts)
    got = engine.reindex(seeds, nbrs, counts)
    for g, w in zip(got, want):
        assert g.dtype == torch.int64 and torch.equal(g, w)
    return want


def _check_batch(model, n_id, adjs, seeds, with_eid):
    assert len(adjs) == len(model.hops)
    assert torch.equal(n_id, model.hops[-1].frontier)
    n_dst = seeds.numel()
    for adj, hop in zip(adjs[::-1], model.hops):
        assert torch.equal(adj.edge_index, hop.edge_index)
        assert adj.size.tolist() == [hop.frontier.numel(), n_dst]
        if with_eid:
            assert torch.equal(adj.e_id, hop.e_id)
        n_dst = hop.frontier.numel()


# ---- the model against itself ----------------------------------------------

def test_model_on_a_hand_worked_input():
    frontier, row, col = fm.reindex_model([5, 9, 5], [9, 2, 5, 2, 7],
                                          [2, 0, 3])
    assert frontier.tolist() == [5, 9, 2, 7]
    assert row.tolist() == [0, 0, 2, 2, 2]
    assert col.tolist() == [1, 2, 0, 2, 3]


def test_hops_model_on_a_hand_worked_graph():
    # 0 -> 2, 1;  1 -> 2;  2 -> (none);  3 -> 0
    indptr, indices = [0, 2, 3, 3, 4], [2, 1, 2, 0]
    model = fm.hops_model(indptr, indices, [3, 1], [2, 2],
                          eid=[40, 41, 42, 43])
    h0, h1 = model.hops
    assert h0.frontier.tolist() == [3, 1, 0, 2]
    assert h0.edge_index.tolist() == [[2, 3], [0, 1]]
    assert h0.dst_ptr.tolist() == [0, 1, 2]
    assert h0.e_id.tolist() == [43, 42]
    assert h1.frontier.tolist() == [3, 1, 0, 2]
    assert h1.edge_index.tolist() == [[2, 3, 3, 1], [0, 1, 2, 2]]
    assert h1.dst_ptr.tolist() == [0, 1, 2, 4, 4]
    assert h1.e_id.tolist() == [43, 42, 40, 41]
    assert model.sizes.tolist() == [2, 4, 4, 4]
    with pytest.raises(ValueError):
        fm.hops_model(indptr, indices, [0], [1])


def test_check_hop_structure_rejects_what_the_invariants_let_through():
    """A frontier in the wrong order, a source id pointing at another
    existing node and a pointer off by one all keep ids in range and edges
    real; the structural check must refuse each."""
    indptr, indices = fm.mixed_graph(N_SMALL)
    seeds = fm.mixed_seed_batches(indptr)[0]
    s = quiver.GraphSageSampler(
        quiver.CSRTopo(indptr=indptr, indices=indices), [3], mode="CPU")
    n_id, _, (adj,) = s.sample(seeds)
    ptr = torch.searchsorted(adj.edge_index[1].contiguous(),
                             torch.arange(seeds.numel() + 1))
    args = (indptr, indices, 3)
    fm.check_hop_structure(seeds, n_id, adj.edge_index, ptr, *args)

    swapped = n_id.clone()
    swapped[[-1, -2]] = swapped[[-2, -1]]
    with pytest.raises(AssertionError):
        fm.check_hop_structure(seeds, swapped, adj.edge_index, ptr, *args)
    wrong_src = adj.edge_index.clone()
    wrong_src[0, 0] = (wrong_src[0, 0] + 1) % n_id.numel()
    with pytest.raises(AssertionError):
        fm.check_hop_structure(seeds, n_id, wrong_src, ptr, *args)
    bad_ptr = ptr.clone()
    bad_ptr[1] += 1
    with pytest.raises(AssertionError):
        fm.check_hop_structure(seeds, n_id, adj.edge_index, bad_ptr, *args)


# ---- reindex_model against CpuSampler.reindex_single -----------------------

def test_reindex_strided_small(engine):
    seeds, nbrs, counts = fm.case_strided(small=True)
    frontier, _, _ = _check_reindex(engine, seeds, nbrs, counts)
    assert torch.equal(frontier[:seeds.numel()], seeds)


@pytest.mark.parametrize("key_is_seed", [False, True])
def test_reindex_one_hot_key_small(engine, key_is_seed):
    frontier, _, col = _check_reindex(
        engine, *fm.case_one_hot(small=True, key_is_seed=key_is_seed))
    assert frontier.numel() == (1 if key_is_seed else 2)
    assert col.unique().tolist() == [frontier.numel() - 1]


def test_reindex_wide_keys(engine):
    seeds, nbrs, counts = fm.case_wide_keys()
    frontier, _, col = _check_reindex(engine, seeds, nbrs, counts)
    assert torch.equal(frontier[col], nbrs)
    # per seed: the key itself (twice), and six keys one bit pattern away
    assert frontier.numel() == 7 * seeds.numel()


def test_reindex_duplicate_seeds(engine):
    """With repeated seeds the frontier is shorter than the seed list,
    while row still indexes seed POSITIONS (0..63)."""
    seeds, nbrs, counts = fm.case_duplicate_seeds()
    frontier, row, _ = _check_reindex(engine, seeds, nbrs, counts)
    assert frontier.numel() < seeds.numel()
    assert int(row.max()) > frontier.numel()


@pytest.mark.parametrize("n", [50, 0])
def test_reindex_zero_rows(engine, n):
    frontier, row, col = _check_reindex(engine, *fm.case_zero_rows(n))
    assert frontier.numel() == n and row.numel() == 0 and col.numel() == 0


def test_reindex_around_a_power_of_two(engine):
    for seeds, nbrs, counts in fm.cases_around_pow2():
        _check_reindex(engine, seeds, nbrs, counts)


# ---- hops_model / check_hop_structure against the CPU sampler ---------------

@pytest.mark.parametrize("return_eid", [False, True])
def test_sample_det(det, return_eid):
    g = torch.Generator().manual_seed(1)
    seeds = torch.randint(0, N_SMALL, (257,), generator=g)
    s = quiver.GraphSageSampler(det, [4, 3], mode="CPU",
                                return_eid=return_eid)
    n_id, bs, adjs = s.sample(seeds)
    assert bs == 257
    model = fm.hops_model(det.indptr, det.indices, seeds, [4, 3])
    _check_batch(model, n_id, adjs, seeds, return_eid)


def test_sample_det_coo_ids(det):
    coo = fm.shuffled_coo(det.indptr, det.indices)
    topo = quiver.CSRTopo(coo, node_count=N_SMALL)
    assert topo.eid is not None
    seeds = torch.arange(0, N_SMALL, 3)
    s = quiver.GraphSageSampler(topo, [4, 3], mode="CPU", return_eid=True)
    n_id, _, adjs = s.sample(seeds)
    model = fm.hops_model(topo.indptr, topo.indices, seeds, [4, 3],
                          eid=topo.eid)
    _check_batch(model, n_id, adjs, seeds, True)
    prev = seeds
    for adj in adjs[::-1]:
        src, dst = adj.edge_index
        assert torch.equal(coo[0, adj.e_id], prev[dst])
        assert torch.equal(coo[1, adj.e_id], n_id[src])
        prev = n_id[:int(adj.size[0])]


def test_sample_det_three_hops(det):
    seeds = torch.arange(300)
    s = quiver.GraphSageSampler(det, [12, 3, 4], mode="CPU")
    n_id, _, adjs = s.sample(seeds)
    model = fm.hops_model(det.indptr, det.indices, seeds, [12, 3, 4])
    _check_batch(model, n_id, adjs, seeds, False)


def test_sample_det_legal_edge_batches(det):
    s = quiver.GraphSageSampler(det, [4, 3], mode="CPU")
    isolated = fm.nodes_of_degree(det.indptr, 0)[:64]
    n_id, _, adjs = s.sample(isolated)
    model = fm.hops_model(det.indptr, det.indices, isolated, [4, 3])
    assert model.sizes.tolist() == [0, 64, 0, 64]
    _check_batch(model, n_id, adjs, isolated, False)
    assert torch.equal(n_id, isolated)

    g = torch.Generator().manual_seed(2)
    dup = torch.randint(0, 40, (100,), generator=g)
    n_id, _, adjs = s.sample(dup)
    model = fm.hops_model(det.indptr, det.indices, dup, [4, 3])
    _check_batch(model, n_id, adjs, dup, False)
    # dst ids are seed positions, past the 40 distinct seeds there can be
    assert int(adjs[-1].edge_index[1].max()) >= 40


def test_sample_mixed_structure(mixed):
    fanouts = [3, 2]
    s = quiver.GraphSageSampler(mixed, fanouts, mode="CPU")
    for seeds in fm.mixed_seed_batches(mixed.indptr):
        n_id, _, adjs = s.sample(seeds)
        prev = seeds
        for adj, k in zip(adjs[::-1], fanouts):
            assert int(adj.size[1]) == prev.numel()
            frontier = n_id[:int(adj.size[0])]
            fm.check_hop_structure(prev, frontier, adj.edge_index, None,
                                   mixed.indptr, mixed.indices, k)
            prev = frontier


def test_mixed_graph_is_det_plus_hubs():
    d_ptr, d_idx = (x.numpy() for x in fm.det_graph(N_SMALL))
    m_ptr, m_idx = (x.numpy() for x in fm.mixed_graph(N_SMALL))
    assert np.diff(d_ptr).max() == 3
    for v in range(N_SMALL):
        row = m_idx[m_ptr[v]:m_ptr[v + 1]]
        if v % fm.HUB_EVERY == 0:
            assert row.size == fm.HUB_DEGREE
        else:
            assert np.array_equal(row, d_idx[d_ptr[v]:d_ptr[v + 1]])
