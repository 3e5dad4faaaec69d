"""Edge ids (return_eid) and edge-weighted draws (edge_weight) of the
sampler, on the CPU engine: exact id checks, weight validation, the draw
distribution against the exact successive-sampling model, IPC handles."""
import os
import pickle
import sys

import pytest
import torch

import quiver

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _sampler_edges as se  # noqa: E402  (shared with the GPU file)


@pytest.fixture(scope="module")
def coo_topo():
    coo = se.coo_graph()
    return coo, quiver.CSRTopo(coo, node_count=300)


def test_graph_has_rows_on_both_sides_of_the_fanout(coo_topo):
    coo, topo = coo_topo
    deg = topo.degree[:64]
    assert torch.equal(deg[:6], torch.arange(6))
    assert int((deg > 4).sum()) > 0
    # multi-edges and self-loops
    assert torch.unique(coo[0] * 300 + coo[1]).numel() < coo.shape[1]
    assert int((coo[0] == coo[1]).sum()) > 0


def test_coo_ids_cpu(coo_topo):
    coo, topo = coo_topo
    s = quiver.GraphSageSampler(topo, se.FANOUTS, mode="CPU",
                                return_eid=True)
    n_id, bs, adjs = s.sample(torch.arange(64))
    assert bs == 64
    se.check_coo_ids(coo, topo, n_id, adjs, se.FANOUTS)


def test_coo_ids_cpu_sort_frontier(coo_topo):
    coo, topo = coo_topo
    s = quiver.GraphSageSampler(topo, se.FANOUTS, mode="CPU",
                                return_eid=True)
    s.sort_frontier = True
    n_id, bs, adjs = s.sample(torch.arange(64))
    se.check_coo_ids(coo, topo, n_id, adjs, se.FANOUTS)


def test_csr_slot_ids_cpu(coo_topo):
    _, topo = coo_topo
    plain = quiver.CSRTopo(indptr=topo.indptr, indices=topo.indices)
    assert plain.eid is None
    s = quiver.GraphSageSampler(plain, se.FANOUTS, mode="CPU",
                                return_eid=True)
    n_id, bs, adjs = s.sample(torch.arange(64))
    se.check_csr_ids(plain, n_id, adjs, se.FANOUTS)


def test_defaults_unchanged_cpu(coo_topo):
    _, topo = coo_topo
    s = quiver.GraphSageSampler(topo, se.FANOUTS, mode="CPU")
    n_id, bs, adjs = s.sample(torch.arange(64))
    for adj in adjs:
        assert adj.e_id.numel() == 0
        assert adj.edge_index.shape[0] == 2
    assert s.share_ipc() == (topo, se.FANOUTS, "CPU")


@pytest.mark.parametrize("bad", ["length", "zero", "negative", "nan", "inf"])
def test_weight_validation(coo_topo, bad):
    _, topo = coo_topo
    w = torch.ones(topo.edge_count)
    if bad == "length":
        w = torch.ones(topo.edge_count - 1)
    elif bad == "zero":
        w[17] = 0.0
    elif bad == "negative":
        w[17] = -1.0
    elif bad == "nan":
        w[17] = float("nan")
    else:
        w[17] = float("inf")
    with pytest.raises(ValueError) as err:
        quiver.GraphSageSampler(topo, se.FANOUTS, mode="CPU", edge_weight=w)
    if bad == "zero":
        assert "remove" in str(err.value)
    with pytest.raises(ValueError):
        quiver.MixedGraphSageSampler(None, 1, topo, se.FANOUTS,
                                     mode="GPU_ONLY", edge_weight=w)


def test_weights_are_permuted_to_csr_order(coo_topo):
    coo, topo = coo_topo
    w = torch.arange(1, coo.shape[1] + 1, dtype=torch.float64)
    s = quiver.GraphSageSampler(topo, se.FANOUTS, mode="CPU", edge_weight=w)
    assert s.w_csr_.dtype == torch.float32
    assert torch.equal(s.w_csr_, w[topo.eid].float())


@pytest.mark.parametrize("case", se.DISTRIBUTION_CASES)
def test_weighted_distribution_cpu(case):
    se.distribution_case("CPU", case)


def test_uniform_draw_misses_the_weighted_model():
    """The yardstick has teeth: unweighted draws of the 1..8 star are tens
    of sigma off the weighted inclusion probabilities."""
    import numpy as np
    topo = se.star_topo(8)
    s = quiver.GraphSageSampler(topo, [1], mode="CPU", return_eid=True)
    _, _, adjs = s.sample(torch.zeros(se.T, dtype=torch.long))
    cnt = np.bincount(adjs[0].e_id.numpy(), minlength=8)
    with pytest.raises(AssertionError):
        se.assert_within_6_sigma(cnt, se.T, np.arange(1, 9) / 36)


def test_hub_k16_cpu():
    se.check_hub_k16("CPU")


def test_short_rows_equal_unweighted_cpu(small_graph):
    se.check_short_rows_unweighted("CPU", small_graph)


def test_permutation_cpu():
    se.check_permutation("CPU")


def test_two_hop_weighted_ids_cpu():
    se.check_two_hop_weighted("CPU")


def test_ipc_round_trip_keeps_options(coo_topo):
    coo, topo = coo_topo
    g = torch.Generator().manual_seed(2)
    w = torch.rand(coo.shape[1], generator=g) + 0.5
    s = quiver.GraphSageSampler(topo, se.FANOUTS, mode="CPU",
                                return_eid=True, edge_weight=w)
    handle = s.share_ipc()
    assert s.w_csr_.is_shared()
    t = quiver.GraphSageSampler.lazy_from_ipc_handle(handle)
    assert t.return_eid is True
    assert torch.equal(t.w_csr_, w[topo.eid])
    assert t.mode == "CPU" and t.sizes == se.FANOUTS
    n_id, bs, adjs = t.sample(torch.arange(64))
    se.check_coo_ids(coo, topo, n_id, adjs, se.FANOUTS)
    # ids only, weights only
    only_ids = quiver.GraphSageSampler.lazy_from_ipc_handle(
        quiver.GraphSageSampler(topo, se.FANOUTS, mode="CPU",
                                return_eid=True).share_ipc())
    assert only_ids.return_eid and only_ids.w_csr_ is None
    only_w = quiver.GraphSageSampler.lazy_from_ipc_handle(
        quiver.GraphSageSampler(topo, se.FANOUTS, mode="CPU",
                                edge_weight=w).share_ipc())
    assert not only_w.return_eid
    assert torch.equal(only_w.w_csr_, w[topo.eid])


def test_ipc_plain_three_tuple_still_loads(coo_topo):
    _, topo = coo_topo
    t = quiver.GraphSageSampler.lazy_from_ipc_handle(
        (topo, se.FANOUTS, "CPU"))
    assert t.return_eid is False and t.w_csr_ is None
    n_id, bs, adjs = t.sample(torch.arange(64))
    assert all(adj.e_id.numel() == 0 for adj in adjs)


def test_sampler_pickles_through_the_reducers(coo_topo):
    coo, topo = coo_topo
    w = torch.ones(coo.shape[1]) * 2
    s = quiver.GraphSageSampler(topo, se.FANOUTS, mode="CPU",
                                return_eid=True, edge_weight=w)
    from multiprocessing.reduction import ForkingPickler
    t = pickle.loads(bytes(ForkingPickler.dumps(s)))
    assert t.return_eid and torch.equal(t.w_csr_, s.w_csr_)


def test_mixed_sampler_carries_the_options(coo_topo):
    coo, topo = coo_topo
    w = torch.ones(coo.shape[1]) * 3
    m = quiver.MixedGraphSageSampler(None, 2, topo, se.FANOUTS, device=0,
                                     mode="UVA_CPU_MIXED", return_eid=True,
                                     edge_weight=w)
    handle = m.share_ipc()
    assert len(handle) == 8
    r = quiver.MixedGraphSageSampler.lazy_from_ipc_handle(handle)
    assert r.return_eid is True and torch.equal(r.w_csr_, m.w_csr_)
    assert r.mode == "UVA_CPU_MIXED" and r.num_workers == 2
    plain = quiver.MixedGraphSageSampler(None, 2, topo, se.FANOUTS)
    assert len(plain.share_ipc()) == 6
    assert plain.return_eid is False and plain.w_csr_ is None
