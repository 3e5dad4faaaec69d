"""Temporal neighbour sampling (temporal_degree_kernel,
temporal_sample_kernel) of the GPU sampler, UVA and GPU modes.  Shapes are
the smallest that reach every branch: rows whose eligible prefix is 0, 1,
5, 6, 10, 11 and 40 edges long at fanout 5 (copy, reservoir, Floyd), tied
times, a hub row of 5000 edges drawn at fanouts 5 and 130 (positions past
2048, the reservoir past k = 128), more rows than one block of 16, and more
rows than one grid of 32 768."""
import os
import sys

import numpy as np
import pytest
import torch

import quiver

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _sampler_edges as se  # noqa: E402
import _sampler_temporal as st  # noqa: E402  (shared with the CPU file)

pytestmark = pytest.mark.gpu

MODES = ["UVA", "GPU"]


@pytest.fixture(scope="module")
def graph_t():
    return st.graph_t()


@pytest.mark.parametrize("mode", MODES)
def test_structure(graph_t, mode):
    st.case_structure(mode, graph_t)


@pytest.mark.parametrize("mode", MODES)
def test_search_edges(graph_t, mode):
    st.case_search(mode, graph_t)


@pytest.mark.parametrize("mode", MODES)
def test_every_draw_branch(graph_t, mode):
    st.case_branches(mode, graph_t)


@pytest.mark.parametrize("mode", MODES)
def test_coverage(graph_t, mode):
    st.case_coverage(mode, graph_t)


@pytest.mark.parametrize("mode", MODES)
def test_past_2048(graph_t, mode):
    st.case_past_2048(mode, graph_t)


@pytest.mark.parametrize("mode", MODES)
def test_uniform(graph_t, mode):
    assert st.uniformity_stat(mode, graph_t) < st.CHI2_BOUND


@pytest.mark.parametrize("mode", MODES)
def test_disjoint_trees(graph_t, mode):
    st.case_disjoint(mode, graph_t)


@pytest.mark.parametrize("mode", MODES)
def test_seeding(graph_t, mode):
    _, time, topo, _ = graph_t
    s = st.make_sampler(topo, mode, [5], time)
    seeds, bounds = [st.R_DEG40] * 200, [st.I64_MAX] * 200
    a = st.drawn_ids(st.sample(s, seeds, bounds))
    b = st.drawn_ids(st.sample(s, seeds, bounds))
    assert not np.array_equal(a, b)
    s.quiver.set_seed(st.SEED)
    c = st.drawn_ids(st.sample(s, seeds, bounds))
    assert np.array_equal(a, c)
    # the copies of one seed draw independently
    assert len(np.unique(np.sort(a.reshape(200, 5), axis=1), axis=0)) > 1


@pytest.mark.parametrize("mode", MODES)
def test_many_rows(graph_t, mode):
    st.case_many_rows(mode, graph_t)


@pytest.mark.parametrize("mode", MODES)
def test_links(graph_t, mode):
    b = st.case_links(mode, graph_t)
    assert b.edge_label_index.is_cuda and b.neg_ok.is_cuda


@pytest.mark.parametrize("mode", MODES)
def test_device_inputs(graph_t, mode):
    _, time, topo, model = graph_t
    s = st.make_sampler(topo, mode, [5, 3], time)
    seeds, bounds = st.structure_seeds()
    tb = s.sample_temporal(torch.tensor(seeds).cuda(),
                           torch.tensor(bounds).cuda())
    st.check_structure(model, seeds, bounds, tb, [5, 3])
    st.check_counts(model, bounds, tb, [5, 3])


@pytest.mark.parametrize("mode", MODES)
def test_python_errors(graph_t, mode):
    st.case_python_errors(mode, graph_t)


@pytest.mark.parametrize("mode", MODES)
def test_engine_checks_its_input(graph_t, mode):
    _, time, topo, _ = graph_t
    s = st.make_sampler(topo, mode, [3], time)
    keys = torch.arange(8, device="cuda")
    bound = torch.zeros(8, dtype=torch.long, device="cuda")
    out, cnt, ids = s.quiver.sample_neighbor_temporal(keys, bound, 3)
    assert len(cnt) == 8 and len(ids) == len(out) == int(cnt.sum())
    for bad in (keys.cpu(), keys.to(torch.int32),
                torch.arange(16, device="cuda")[::2], keys.view(2, 4)):
        with pytest.raises(RuntimeError):
            s.quiver.sample_neighbor_temporal(bad, bound, 3)
        with pytest.raises(RuntimeError):
            s.quiver.sample_neighbor_temporal(keys, bad, 3)
    for k in (0, -2):
        with pytest.raises(RuntimeError):
            s.quiver.sample_neighbor_temporal(keys, bound, k)
    # a key that names no seed or no node draws nothing
    wild = torch.tensor([-1, 8 * st.N_T, 2 ** 62], device="cuda")
    out, cnt, _ = s.quiver.sample_neighbor_temporal(wild, bound, 3)
    assert out.numel() == 0 and cnt.tolist() == [0, 0, 0]
    with pytest.raises(RuntimeError):
        s.quiver.set_edge_time(time[:-1])
    with pytest.raises(RuntimeError):
        s.quiver.set_edge_time(time.float())
    plain = quiver.GraphSageSampler(topo, [3], mode=mode)
    plain.lazy_init_quiver()
    with pytest.raises(RuntimeError):
        plain.quiver.sample_neighbor_temporal(keys, bound, 3)


@pytest.mark.parametrize("mode", MODES)
def test_sorted_rows_pass_through(mode):
    st.case_t0(mode)


@pytest.mark.parametrize("mode", MODES)
def test_unsorted_rows_without_eid(graph_t, mode):
    st.case_unsorted_without_eid(mode, graph_t)


@pytest.mark.parametrize("mode", MODES)
def test_plain_sample_draws_the_same_graph(graph_t, mode):
    st.case_plain_sample_same_graph(mode, graph_t, se.check_coo_ids)
