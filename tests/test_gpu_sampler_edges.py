"""Edge ids (return_eid) and edge-weighted draws (edge_weight) of the GPU
sampler, UVA and GPU modes: exact id checks on every sampling path, the
weighted draw kernel against the exact successive-sampling model, and the
structural cases.  Shapes are the smallest that still reach every branch
of weighted_sample_kernel: rows under and over the fanout, fanouts under
and over the 16 lanes of a row's subgroup, rows of many 16-wide steps with
positions past 2048, more rows than one block of 16, and a fanout whose
slots need more than 64 KB of LDS per block."""
import os
import subprocess
import sys

import pytest
import torch

import quiver

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _sampler_edges as se  # noqa: E402  (shared with the CPU file)

pytestmark = pytest.mark.gpu

MODES = ["UVA", "GPU"]


@pytest.fixture(scope="module")
def coo_topo():
    coo = se.coo_graph()
    return coo, quiver.CSRTopo(coo, node_count=300)


def _sampler(topo, mode, **kw):
    s = quiver.GraphSageSampler(topo, se.FANOUTS, device=0, mode=mode, **kw)
    s.lazy_init_quiver()
    s.quiver.set_seed(99)
    return s


@pytest.mark.parametrize("mode", MODES)
def test_coo_ids_fused(coo_topo, mode):
    coo, topo = coo_topo
    s = _sampler(topo, mode, return_eid=True)
    n_id, bs, adjs = s.sample(torch.arange(64))
    assert bs == 64
    for adj in adjs:
        assert adj.edge_index.is_cuda and adj.e_id.is_cuda
        # views of the chain's one edge buffer, not copies
        assert adj.e_id.untyped_storage().data_ptr() == \
            adj.edge_index.untyped_storage().data_ptr()
        assert getattr(adj.edge_index, "_quiver_dst_ptr", None) is not None
    se.check_coo_ids(coo, topo, n_id, adjs, se.FANOUTS)
    moved = [adj.to("cpu") for adj in adjs]
    assert all(a.e_id.device.type == "cpu" for a in moved)
    se.check_coo_ids(coo, topo, n_id, moved, se.FANOUTS)


@pytest.mark.parametrize("mode", MODES)
def test_coo_ids_sort_frontier(coo_topo, mode):
    coo, topo = coo_topo
    s = _sampler(topo, mode, return_eid=True)
    s.sort_frontier = True
    n_id, bs, adjs = s.sample(torch.arange(64))
    se.check_coo_ids(coo, topo, n_id, adjs, se.FANOUTS)


@pytest.mark.parametrize("mode", MODES)
def test_coo_ids_async_finalize(coo_topo, mode):
    coo, topo = coo_topo
    s = _sampler(topo, mode, return_eid=True)
    tok = s.sample_async(torch.arange(64))
    torch.cuda.synchronize()
    n_id, bs, adjs = s.sample_finalize(tok)
    assert bs == 64
    se.check_coo_ids(coo, topo, n_id, adjs, se.FANOUTS)


@pytest.mark.parametrize("mode", MODES)
def test_coo_ids_training_prefetcher(coo_topo, mode):
    coo, topo = coo_topo
    s = _sampler(topo, mode, return_eid=True)
    batches = [torch.arange(64), torch.arange(64)]
    got = 0
    for n_id, bs, adjs, x in quiver.TrainingPrefetcher(
            s, None, batches, depth=2, device=0):
        torch.cuda.synchronize()
        assert x is None and bs == 64
        se.check_coo_ids(coo, topo, n_id, adjs, se.FANOUTS)
        got += 1
    assert got == 2


@pytest.mark.parametrize("mode", MODES)
def test_csr_slot_ids(coo_topo, mode):
    _, topo = coo_topo
    plain = quiver.CSRTopo(indptr=topo.indptr, indices=topo.indices)
    s = _sampler(plain, mode, return_eid=True)
    n_id, bs, adjs = s.sample(torch.arange(64))
    se.check_csr_ids(plain, n_id, adjs, se.FANOUTS)
    s.sort_frontier = True
    n_id, bs, adjs = s.sample(torch.arange(64))
    se.check_csr_ids(plain, n_id, adjs, se.FANOUTS)


@pytest.mark.parametrize("mode", MODES)
def test_defaults_unchanged(coo_topo, mode):
    _, topo = coo_topo
    s = _sampler(topo, mode)
    n_id, bs, adjs = s.sample(torch.arange(64))
    tok = s.sample_async(torch.arange(64))
    torch.cuda.synchronize()
    _, _, adjs_async = s.sample_finalize(tok)
    s.sort_frontier = True
    _, _, adjs_hop = s.sample(torch.arange(64))
    for adj in adjs + adjs_async + adjs_hop:
        assert adj.e_id.numel() == 0
        assert adj.edge_index.shape[0] == 2
    assert tok[1][0][1].shape[0] == 2
    assert s.share_ipc() == (topo, se.FANOUTS, mode)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("case", se.DISTRIBUTION_CASES)
def test_weighted_distribution(case, mode):
    se.distribution_case(mode, case)


def test_weighted_draw_is_reproducible_and_rows_independent():
    """set_seed fixes the draw; duplicate seeds of one batch still draw
    independently (the stream is keyed by row)."""
    w = torch.arange(1, 65, dtype=torch.float32)
    topo = se.star_topo(64)
    s = quiver.GraphSageSampler(topo, [8], device=0, mode="GPU",
                                return_eid=True, edge_weight=w)
    s.lazy_init_quiver()
    seeds = torch.zeros(256, dtype=torch.long)
    s.quiver.set_seed(7)
    a = s.sample(seeds)[2][0].e_id.cpu()
    s.quiver.set_seed(7)
    b = s.sample(seeds)[2][0].e_id.cpu()
    assert torch.equal(a, b)
    rows = a.view(256, 8).sort(dim=1).values
    assert torch.unique(rows, dim=0).shape[0] > 200


@pytest.mark.parametrize("mode", MODES)
def test_hub_k16(mode):
    se.check_hub_k16(mode)


def test_hub_fanout_past_64k_of_lds():
    """k = 600: 16 rows x 600 slots x 8 B = 75 KB of LDS per block."""
    k, rows = 600, 20
    topo = se.star_topo(3000)
    s = quiver.GraphSageSampler(topo, [k], device=0, mode="GPU",
                                return_eid=True,
                                edge_weight=se.hub_weights())
    n_id, bs, adjs = s.sample(torch.zeros(rows, dtype=torch.long))
    ei, e_id = adjs[0].edge_index.cpu(), adjs[0].e_id.cpu()
    assert tuple(e_id.shape) == (rows * k,)
    assert int(e_id.min()) >= 0 and int(e_id.max()) < 3000
    assert torch.unique(ei[1] * 3000 + e_id).numel() == rows * k
    assert torch.equal(n_id.cpu()[ei[0]], topo.indices[e_id])
    # inclusion grows with the weight: class c (weight 2^c) holds about
    # 500 (1 - exp(-2^c t)) of a row's 600 with t near 0.024, i.e. about
    # 12, 23, 46, 87, 159, 268 -- far apart next to their spread over 20
    # rows, so the class totals must come out strictly increasing
    per_class = torch.bincount(e_id // se.HUB_PER_CLASS,
                               minlength=se.HUB_CLASSES)
    assert bool((per_class[1:] > per_class[:-1]).all()), per_class


def test_fanout_too_large_for_lds_is_refused():
    topo = se.star_topo(64)
    k = 160 * 1024 // (16 * 8) + 1
    s = quiver.GraphSageSampler(topo, [k], device=0, mode="GPU",
                                edge_weight=torch.ones(64))
    with pytest.raises(RuntimeError, match="too large"):
        s.sample_layer(torch.zeros(4, dtype=torch.long), k)


@pytest.mark.parametrize("mode", MODES)
def test_short_rows_equal_unweighted(small_graph, mode):
    se.check_short_rows_unweighted(mode, small_graph)


@pytest.mark.parametrize("mode", MODES)
def test_permutation(mode):
    se.check_permutation(mode)


@pytest.mark.parametrize("mode", MODES)
def test_two_hop_weighted_ids(mode):
    se.check_two_hop_weighted(mode)


def test_weights_without_ids_keep_two_row_edges(coo_topo):
    coo, topo = coo_topo
    s = _sampler(topo, "GPU", edge_weight=torch.ones(coo.shape[1]))
    n_id, bs, adjs = s.sample(torch.arange(64))
    for adj, k in se.hop_pairs(adjs, se.FANOUTS):
        assert adj.e_id.numel() == 0 and adj.edge_index.shape[0] == 2
        n_dst = int(adj.size[1])
        want = torch.clamp(topo.degree[n_id.cpu()[:n_dst]], max=k)
        assert torch.equal(
            torch.bincount(adj.edge_index[1].cpu(), minlength=n_dst), want)


GRAPH_SCRIPT = r"""
import os, sys, warnings
import torch
import quiver
sys.path.insert(0, os.path.join(os.getcwd(), "tests"))
import _sampler_edges as se

os.environ["QUIVER_HIPGRAPH"] = "1"
coo = se.coo_graph()
topo = quiver.CSRTopo(coo, node_count=300)
g = torch.Generator().manual_seed(11)
w = torch.rand(coo.shape[1], generator=g) * 1.5 + 0.5
s = quiver.GraphSageSampler(topo, se.FANOUTS, device=0, mode="GPU",
                            return_eid=True, edge_weight=w)
s.lazy_init_quiver()
s.quiver.set_seed(5)
batches = [torch.arange(64) for _ in range(4)]
seen = []
with warnings.catch_warnings(record=True) as caught:
    warnings.simplefilter("always")
    for n_id, bs, adjs, x in quiver.TrainingPrefetcher(
            s, None, batches, depth=1, device=0, num_streams=1):
        torch.cuda.synchronize()
        se.check_coo_ids(coo, topo, n_id, adjs, se.FANOUTS)
        seen.append(torch.cat([a.e_id.cpu() for a in adjs]))
assert len(seen) == 4
# replays advance the device seed: batches differ
assert not all(torch.equal(seen[0], t) for t in seen[1:])
refused = any("capture failed" in str(m.message)
              or "replay failed" in str(m.message) for m in caught)
print("HIPGRAPH-REFUSED" if refused else "HIPGRAPH-OK")
"""


def test_ids_from_captured_graph_slots():
    """The prefetcher's hipGraph slots call sample_hops_raw directly; ids
    and weighted draws must come out of the replays too.  Run in a process
    of its own, like the other capture test: a refused capture must not
    leave this process's stream in capture state.  Where the runtime
    refuses the capture the prefetcher runs uncaptured and the same checks
    hold."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    res = subprocess.run([sys.executable, "-c", GRAPH_SCRIPT],
                         env=dict(os.environ), capture_output=True,
                         text=True, timeout=300, cwd=root)
    assert res.returncode == 0, res.stdout + res.stderr
    assert "HIPGRAPH-" in res.stdout
