"""Negative-tail draws (sample_negative) and link-prediction batches
(sample_links) on the CPU engine.  The CPU engine seeds itself like its
sample_neighbor (no set_seed), so every statistical bound here is one that
an exact draw misses with negligible probability."""
import os
import pickle
import subprocess
import sys

import pytest
import torch

import quiver

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _sampler_edges as se  # noqa: E402
import _sampler_links as sl  # noqa: E402  (shared with the GPU file)

MODE = "CPU"
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def graph_a():
    topo = sl.graph_a()
    return topo, sl.edge_keys(topo)


@pytest.fixture(scope="module")
def graph_b():
    topo = sl.graph_b()
    return topo, sl.edge_keys(topo)


@pytest.fixture(scope="module")
def uniform_draw():
    return sl.uniformity_draw(MODE, sl.graph_u())


@pytest.fixture(scope="module")
def coo_topo():
    coo = se.coo_graph()
    return coo, quiver.CSRTopo(coo, node_count=300)


def test_graphs_are_as_described(graph_a, graph_b):
    topo, _ = graph_a
    assert topo.degree[:8].tolist() == sl.A_DEGREES + [sl.N_A - 2,
                                                       sl.N_A - 1]
    assert int(topo.degree[8:].max()) <= 8
    row = topo.indices[topo.indptr[6]:topo.indptr[7]]
    assert sl.A_VALID_TAIL not in row.tolist()
    # rows are not sorted
    assert not torch.equal(row, torch.sort(row).values)
    topo, keys = graph_b
    assert bool((topo.degree == sl.B_DEGREE).all())
    assert len(keys) == sl.N_B * sl.B_DEGREE


@pytest.mark.parametrize("num_neg", sl.NUM_NEGS)
def test_validity_a(graph_a, num_neg):
    sl.check_validity_case(MODE, *graph_a, num_neg)


@pytest.mark.parametrize("num_neg", sl.NUM_NEGS)
def test_validity_b(graph_b, num_neg):
    sl.check_validity_case(MODE, *graph_b, num_neg)


def test_ok_flags_a(graph_a):
    sl.check_ok_flags_a(MODE, *graph_a)


def test_not_ok_share_b(graph_b):
    # expected (49/64)**16 = 1.4 %; ten runs of this engine gave 1.0 % to
    # 2.5 %
    assert sl.not_ok_share_b(MODE, *graph_b) <= 0.05


def test_uniform(uniform_draw):
    _, stat = uniform_draw
    assert stat < sl.CHI2_BOUND


def test_repeated_source_draws_independently(uniform_draw):
    neg, _ = uniform_draw
    assert torch.unique(neg, dim=0).shape[0] > 1


def test_successive_calls_differ(graph_a):
    topo, _ = graph_a
    s = sl.make_sampler(topo, MODE)
    src = torch.arange(sl.A_SOURCES)
    a, _ = sl.draw(s, src, 5)
    b, _ = sl.draw(s, src, 5)
    assert not torch.equal(a, b)


@pytest.mark.parametrize("p", [0, 1, 17])
def test_sizes(graph_a, p):
    topo, keys = graph_a
    s = sl.make_sampler(topo, MODE)
    src = torch.arange(8, 8 + p)
    neg, ok = sl.draw(s, src, 5)
    sl.check_valid(topo, keys, src, neg, ok)
    assert bool(ok.all())


def test_many_rows(graph_a):
    topo, keys = graph_a
    g = torch.Generator().manual_seed(9)
    src = torch.randint(0, sl.N_A, (40_000,), generator=g)
    s = sl.make_sampler(topo, MODE)
    neg, ok = sl.draw(s, src, 2)
    sl.check_valid(topo, keys, src, neg, ok)
    plain = (src != sl.A_ONE_LEFT) & (src != sl.A_NONE_LEFT)
    assert bool(ok[plain].all())


def test_bad_arguments(graph_b):
    topo, _ = graph_b
    s = sl.make_sampler(topo, MODE)
    src = torch.arange(4)
    with pytest.raises(ValueError):
        s.sample_negative(src, 0)
    with pytest.raises(ValueError):
        s.sample_negative(src, 1, 0)
    with pytest.raises(ValueError):
        s.sample_negative(src.float())
    with pytest.raises(ValueError):
        s.sample_negative(src.view(2, 2))
    with pytest.raises(ValueError):
        s.sample_negative(torch.tensor([0, sl.N_B]))
    with pytest.raises(ValueError):
        s.sample_negative(torch.tensor([-1, 3]))
    # the engine itself refuses what it cannot read
    with pytest.raises(RuntimeError):
        s.quiver.sample_negative(src.to(torch.int32), 1, 16)
    with pytest.raises(RuntimeError):
        s.quiver.sample_negative(torch.arange(8)[::2], 1, 16)
    with pytest.raises(RuntimeError):
        s.quiver.sample_negative(src, 0, 16)
    with pytest.raises(RuntimeError):
        s.quiver.sample_negative(src, 1, 0)


@pytest.mark.parametrize("num_neg", [0, 1, 3])
def test_links(coo_topo, num_neg):
    sl.check_links(MODE, *coo_topo, num_neg)


def test_links_pair_input_and_eid(coo_topo):
    coo, topo = coo_topo
    b = sl.check_links(MODE, coo, topo, 2, return_eid=True)
    s = sl.make_sampler(topo, MODE)
    pair = s.sample_links((coo[0, :9], coo[1, :9]), num_neg=1)
    assert tuple(pair.edge_label_index.shape) == (2, 18)
    assert torch.equal(pair.n_id[pair.edge_label_index[:, :9]], coo[:, :9])
    assert all(adj.e_id.numel() == 0 for adj in pair.adjs)
    assert all(adj.e_id.numel() > 0 for adj in b.adjs)


def test_links_bad_input(coo_topo):
    coo, topo = coo_topo
    s = sl.make_sampler(topo, MODE)
    for bad in (coo[0, :8], coo[:, :8].t().contiguous(),
                coo[:, :8].float(), coo[:, :0],
                torch.tensor([[0, 300], [1, 2]]),
                torch.tensor([[0, 1], [-1, 2]]),
                (coo[0, :8], coo[1, :8], coo[1, :8])):
        with pytest.raises(ValueError):
            s.sample_links(bad)
    with pytest.raises(ValueError):
        s.sample_links(coo[:, :8], num_neg=-1)
    with pytest.raises(ValueError):
        s.sample_links(coo[:, :8], neg_tries=0)


def test_share_ipc_unchanged(coo_topo):
    _, topo = coo_topo
    s = quiver.GraphSageSampler(topo, se.FANOUTS, mode=MODE)
    handle = s.share_ipc()
    assert len(handle) == 3
    assert handle[0] is topo and handle[1] == se.FANOUTS and \
        handle[2] == MODE
    t = quiver.GraphSageSampler.lazy_from_ipc_handle(
        pickle.loads(pickle.dumps(handle)))
    b = t.sample_links(torch.tensor([[0, 7], [1, 2]]).t().contiguous())
    assert b.batch_size <= 6       # four endpoints and two negatives
    # drawing links leaves the handle as it was
    assert t.share_ipc()[1:] == handle[1:] and len(t.share_ipc()) == 3


def test_example_runs():
    out = subprocess.run(
        [sys.executable, os.path.join(REPO, "examples", "link_prediction.py"),
         "--mode", "CPU", "--steps", "4"],
        capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr[-2000:]
    losses = [float(line.split("loss=")[1].split()[0])
              for line in out.stdout.splitlines() if "loss=" in line]
    assert len(losses) == 4
    assert all(torch.isfinite(torch.tensor(losses)))
