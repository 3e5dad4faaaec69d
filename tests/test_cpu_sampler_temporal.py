"""Temporal neighbour sampling (edge_time, sample_temporal, temporal
sample_links) on the CPU engine.  The CPU engine seeds itself (no
set_seed), so every statistical bound here is one that an exact draw misses
with negligible probability."""
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest
import torch

import quiver

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _sampler_edges as se  # noqa: E402
import _sampler_temporal as st  # noqa: E402  (shared with the GPU file)

MODE = "CPU"
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def graph_t():
    return st.graph_t()


def test_graph_is_as_described(graph_t):
    coo, time, topo, model = graph_t
    deg = topo.degree
    assert deg[:10].tolist() == [0, 1, 5, 6, 10, 11, 40, 12, 6, st.HUB_DEG]
    assert int(deg[10:].min()) >= 3 and int(deg[10:].max()) <= 8
    assert topo.node_count == st.N_T > 2048 and topo.eid is not None
    hub = model.eligible(st.R_HUB, st.I64_MAX)
    assert np.array_equal(model.time[hub], np.arange(st.HUB_DEG))
    assert sorted(model.time[model.eligible(st.R_TIES, 9)]) == \
        [1, 1, 1, 2, 2, 3]
    # no sorted rows to pass through: the sampler has to permute
    s = st.make_sampler(topo, MODE, [3], time)
    assert s.temporal_[0].data_ptr() != topo.indices.data_ptr()
    row = s.temporal_[1][topo.indptr[st.R_HUB]:topo.indptr[st.R_HUB + 1]]
    assert torch.equal(row, torch.arange(st.HUB_DEG))


def test_structure(graph_t):
    st.case_structure(MODE, graph_t)


def test_search_edges(graph_t):
    st.case_search(MODE, graph_t)


def test_every_draw_branch(graph_t):
    st.case_branches(MODE, graph_t)


def test_coverage(graph_t):
    st.case_coverage(MODE, graph_t)


def test_past_2048(graph_t):
    st.case_past_2048(MODE, graph_t)


def test_uniform(graph_t):
    assert st.uniformity_stat(MODE, graph_t) < st.CHI2_BOUND


def test_disjoint_trees(graph_t):
    st.case_disjoint(MODE, graph_t)


def test_successive_calls_differ(graph_t):
    _, time, topo, _ = graph_t
    s = st.make_sampler(topo, MODE, [5], time)
    seeds, bounds = [st.R_DEG40] * 200, [st.I64_MAX] * 200
    a = st.drawn_ids(st.sample(s, seeds, bounds))
    b = st.drawn_ids(st.sample(s, seeds, bounds))
    assert not np.array_equal(a, b)
    # the copies of one seed draw independently
    assert len(np.unique(np.sort(a.reshape(200, 5), axis=1), axis=0)) > 1


def test_many_rows(graph_t):
    st.case_many_rows(MODE, graph_t)


def test_links(graph_t):
    st.case_links(MODE, graph_t)


def test_links_without_negatives_and_ids(graph_t):
    coo, time, topo, _ = graph_t
    s = st.make_sampler(topo, MODE, [4, 3], time, return_eid=False)
    b = s.sample_links(coo[:, :9], num_neg=0, edge_label_time=time[:9])
    assert b.batch_size == 18 and b.neg_ok.numel() == 0
    assert torch.equal(b.n_id[b.edge_label_index], coo[:, :9])
    assert all(adj.e_id.numel() == 0 for adj in b.adjs)
    # without edge_label_time the batch is the merged one, as before
    b = s.sample_links(coo[:, :9], num_neg=0)
    assert b.batch_size == torch.unique(coo[:, :9]).numel()


def test_python_errors(graph_t):
    st.case_python_errors(MODE, graph_t)


def test_engine_checks_its_input(graph_t):
    _, time, topo, _ = graph_t
    s = st.make_sampler(topo, MODE, [3], time)
    keys = torch.arange(8)
    bound = torch.zeros(8, dtype=torch.long)
    out, cnt, ids = s.quiver.sample_neighbor_temporal(keys, bound, 3)
    assert len(cnt) == 8 and len(ids) == len(out) == int(cnt.sum())
    for bad in (keys.to(torch.int32), torch.arange(16)[::2],
                keys.view(2, 4)):
        with pytest.raises(RuntimeError):
            s.quiver.sample_neighbor_temporal(bad, bound, 3)
        with pytest.raises(RuntimeError):
            s.quiver.sample_neighbor_temporal(keys, bad, 3)
    for k in (0, -2):
        with pytest.raises(RuntimeError):
            s.quiver.sample_neighbor_temporal(keys, bound, k)
    with pytest.raises(RuntimeError):
        s.quiver.set_edge_time(time[:-1], True)
    with pytest.raises(RuntimeError):
        s.quiver.set_edge_time(time.float(), True)
    plain = quiver.GraphSageSampler(topo, [3], mode=MODE)
    plain.lazy_init_quiver()
    with pytest.raises(RuntimeError):
        plain.quiver.sample_neighbor_temporal(keys, bound, 3)


def test_ipc_round_trip(graph_t):
    _, time, topo, model = graph_t
    s = quiver.GraphSageSampler(topo, [5, 3], mode=MODE, return_eid=True,
                                edge_time=time)
    handle = s.share_ipc()
    t = quiver.GraphSageSampler.lazy_from_ipc_handle(
        pickle.loads(pickle.dumps(handle)))
    assert t.return_eid and t.sizes == [5, 3] and t.mode == MODE
    # the sorted rows travel: the worker's copy equals the parent's
    for mine, theirs in zip(s.temporal_, t.temporal_):
        assert torch.equal(mine, theirs)
    seeds, bounds = st.structure_seeds()
    st.run_case(model, t, seeds, bounds)
    # samplers without edge_time keep the handles they had
    plain = quiver.GraphSageSampler(topo, [5, 3], mode=MODE)
    assert plain.share_ipc() == (topo, [5, 3], MODE)
    ids = quiver.GraphSageSampler(topo, [5, 3], mode=MODE, return_eid=True)
    h = ids.share_ipc()
    assert len(h) == 5 and h[:4] == (topo, [5, 3], MODE, True) \
        and h[4] is None
    w = quiver.GraphSageSampler(topo, [5, 3], mode=MODE,
                                edge_weight=torch.ones(topo.edge_count))
    h = w.share_ipc()
    assert len(h) == 5 and h[3] is False and h[4] is w.w_csr_


def test_sorted_rows_pass_through():
    st.case_t0(MODE)


def test_unsorted_rows_without_eid(graph_t):
    st.case_unsorted_without_eid(MODE, graph_t)


def test_plain_sample_draws_the_same_graph(graph_t):
    st.case_plain_sample_same_graph(MODE, graph_t, se.check_coo_ids)


def test_example_runs_temporal():
    out = subprocess.run(
        [sys.executable, os.path.join(REPO, "examples", "link_prediction.py"),
         "--mode", "CPU", "--steps", "3", "--temporal"],
        capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [line for line in out.stdout.splitlines() if "loss=" in line]
    assert len(lines) == 3
    for line in lines:
        assert np.isfinite(float(line.split("loss=")[1].split()[0]))
        # every endpoint and negative roots its own tree: 256 * (2 + 2)
        assert "seeds=1024" in line
