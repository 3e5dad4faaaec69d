"""Negative-tail draws (negative_sample_kernel) and link-prediction batches
(sample_links) of the GPU sampler, UVA and GPU modes.  Shapes are the
smallest that reach every branch of the kernel: rows of degree 0, 1, 15,
16, 17 and 40 (the 16-wide step boundary), a node count above 2048, rows
with one and with no valid tail, num_neg under, at and over the 16 lanes
of a row's subgroup, more rows than one block of 16, and more rows than
one grid of 32 768."""
import os
import sys

import pytest
import torch

import quiver

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _sampler_edges as se  # noqa: E402
import _sampler_links as sl  # noqa: E402  (shared with the CPU file)

pytestmark = pytest.mark.gpu

MODES = ["UVA", "GPU"]


@pytest.fixture(scope="module")
def graph_a():
    topo = sl.graph_a()
    return topo, sl.edge_keys(topo)


@pytest.fixture(scope="module")
def graph_b():
    topo = sl.graph_b()
    return topo, sl.edge_keys(topo)


@pytest.fixture(scope="module")
def graph_u():
    return sl.graph_u()


@pytest.fixture(scope="module")
def coo_topo():
    coo = se.coo_graph()
    return coo, quiver.CSRTopo(coo, node_count=300)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("num_neg", sl.NUM_NEGS)
def test_validity_a(graph_a, mode, num_neg):
    sl.check_validity_case(mode, *graph_a, num_neg)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("num_neg", sl.NUM_NEGS)
def test_validity_b(graph_b, mode, num_neg):
    sl.check_validity_case(mode, *graph_b, num_neg)


@pytest.mark.parametrize("mode", MODES)
def test_ok_flags_a(graph_a, mode):
    sl.check_ok_flags_a(mode, *graph_a)


@pytest.mark.parametrize("mode", MODES)
def test_not_ok_share_b(graph_b, mode):
    # expected (49/64)**16 = 1.4 %.  Ten runs of the CPU engine gave 1.0 %
    # to 2.5 %; the seed of make_sampler gives the GPU engine 1.07 %.
    assert sl.not_ok_share_b(mode, *graph_b) <= 0.05


@pytest.mark.parametrize("mode", MODES)
def test_uniform_and_row_keyed(graph_u, mode):
    neg, stat = sl.uniformity_draw(mode, graph_u)
    assert stat < sl.CHI2_BOUND
    # the 1000 copies of the source draw independently
    assert torch.unique(neg, dim=0).shape[0] > 1


@pytest.mark.parametrize("mode", MODES)
def test_seeding(graph_a, mode):
    topo, _ = graph_a
    s = sl.make_sampler(topo, mode)
    src = torch.arange(sl.A_SOURCES)
    a, a_ok = sl.draw(s, src, 17)
    b, _ = sl.draw(s, src, 17)
    assert not torch.equal(a, b)
    s.quiver.set_seed(sl.SEED)
    c, c_ok = sl.draw(s, src, 17)
    assert torch.equal(a, c) and torch.equal(a_ok, c_ok)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("p", [0, 1, 17])
def test_sizes(graph_a, mode, p):
    topo, keys = graph_a
    s = sl.make_sampler(topo, mode)
    src = torch.arange(8, 8 + p)
    neg, ok = sl.draw(s, src, 5)
    sl.check_valid(topo, keys, src, neg, ok)
    assert bool(ok.all())


@pytest.mark.parametrize("mode", MODES)
def test_many_rows(graph_a, mode):
    topo, keys = graph_a
    g = torch.Generator().manual_seed(9)
    src = torch.randint(0, sl.N_A, (40_000,), generator=g)
    s = sl.make_sampler(topo, mode)
    neg, ok = sl.draw(s, src, 2)
    sl.check_valid(topo, keys, src, neg, ok)
    plain = (src != sl.A_ONE_LEFT) & (src != sl.A_NONE_LEFT)
    assert bool(ok[plain].all())
    # the rows past the first grid are drawn too, not left as allocated
    assert int(neg[32_768:].max()) >= 0.9 * sl.N_A


@pytest.mark.parametrize("mode", MODES)
def test_engine_checks_its_input(graph_b, mode):
    topo, _ = graph_b
    s = sl.make_sampler(topo, mode)
    src = torch.arange(8, device="cuda")
    with pytest.raises(RuntimeError):
        s.quiver.sample_negative(src.cpu(), 1, 16)
    with pytest.raises(RuntimeError):
        s.quiver.sample_negative(src.to(torch.int32), 1, 16)
    with pytest.raises(RuntimeError):
        s.quiver.sample_negative(src[::2], 1, 16)
    with pytest.raises(RuntimeError):
        s.quiver.sample_negative(src, 0, 16)
    with pytest.raises(RuntimeError):
        s.quiver.sample_negative(src, 1, 0)
    with pytest.raises(ValueError):
        s.sample_negative(torch.tensor([0, sl.N_B]))


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("num_neg", [0, 3])
def test_links(coo_topo, mode, num_neg):
    sl.check_links(mode, *coo_topo, num_neg)


@pytest.mark.parametrize("mode", MODES)
def test_links_eid_and_device_input(coo_topo, mode):
    coo, topo = coo_topo
    sl.check_links(mode, coo, topo, 2, return_eid=True)
    s = sl.make_sampler(topo, mode)
    b = s.sample_links(coo[:, :9].cuda(), num_neg=1)
    assert b.edge_label_index.is_cuda and b.neg_ok.is_cuda
    assert torch.equal(b.n_id[b.edge_label_index[:, :9]].cpu(), coo[:, :9])


@pytest.mark.parametrize("mode", MODES)
def test_links_bad_input(coo_topo, mode):
    coo, topo = coo_topo
    s = sl.make_sampler(topo, mode)
    for bad in (coo[0, :8], coo[:, :8].t().contiguous(),
                coo[:, :8].float(), coo[:, :8].float().cuda(),
                torch.tensor([[0, 300], [1, 2]])):
        with pytest.raises(ValueError):
            s.sample_links(bad)
