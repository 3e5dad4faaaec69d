"""Feature(quantize="int8") end to end: placement in packed bytes, lookups
under the hot-order permutation, the prefetcher, and IPC handles.  Rows
are compared with quiver.dequantize_rows of the same packed rows, within
one unit in the last place (see test_gpu_gather_quant.py)."""
import pytest
import torch
import torch.multiprocessing as mp

import quiver

pytestmark = pytest.mark.gpu

DIM = 100


def _ordinal(t):
    if t.dtype == torch.float32:
        bits = t.contiguous().view(torch.int32).to(torch.int64)
        mag = bits & 0x7FFFFFFF
    else:
        bits = t.contiguous().view(torch.int16).to(torch.int64)
        mag = bits & 0x7FFF
    return torch.where(bits < 0, -mag, mag)


def _within_one_ulp(got, want):
    got = got.cpu()
    return (got.dtype == want.dtype and got.shape == want.shape
            and int((_ordinal(got) - _ordinal(want)).abs().max()) <= 1)


def _reference(x, out_dtype):
    """Rows are quantized one by one, so the reference does not depend on
    the permutation the store applies first."""
    return quiver.dequantize_rows(quiver.quantize_rows(x), x.size(1),
                                  out_dtype)


def _feature(small_graph, x, **kw):
    indptr, indices = small_graph
    topo = quiver.CSRTopo(indptr=indptr, indices=indices)
    feature = quiver.Feature(0, device_list=[0], device_cache_size="16K",
                             cache_policy="device_replicate", csr_topo=topo)
    feature.from_cpu_tensor(x.clone(), **kw)
    return topo, feature


@pytest.mark.parametrize("in_dtype,out_dtype,want_dtype", [
    (torch.float32, None, torch.float32),
    (torch.bfloat16, None, torch.bfloat16),
    (torch.float16, None, torch.float16),
    (torch.float32, torch.bfloat16, torch.bfloat16),
])
def test_lookups_and_shape(small_graph, in_dtype, out_dtype, want_dtype):
    g = torch.Generator().manual_seed(31)
    x = torch.randn(500, DIM, generator=g).to(in_dtype)
    topo, feature = _feature(small_graph, x, quantize="int8",
                             out_dtype=out_dtype)
    ref = _reference(x, want_dtype)
    assert feature.feature_order is not None
    assert feature.shape == x.shape
    assert feature.size(0) == 500 and feature.size(1) == DIM
    st = feature._shard_tensor().shard_tensor
    assert st.shard_devices() == [0, -1]  # the budget splits the rows

    idx = torch.randint(0, 500, (1500,), generator=g)
    got = feature[idx.cuda()]
    assert got.dtype == want_dtype and got.shape == (1500, DIM)
    assert _within_one_ulp(got, ref[idx])
    n_dev = torch.tensor([1200], dtype=torch.int64, device="cuda")
    raw = feature.gather_raw(idx.cuda(), n_dev)
    assert raw.shape == (1500, DIM)
    assert _within_one_ulp(raw[:1200], ref[idx[:1200]])
    assert torch.equal(raw[:1200], got[:1200])


def test_cache_budget_counts_packed_bytes(small_graph):
    g = torch.Generator().manual_seed(32)
    x = torch.randn(500, DIM, generator=g)
    _, plain = _feature(small_graph, x)
    _, packed = _feature(small_graph, x, quantize="int8")
    hot_plain = plain._shard_tensor().shard_tensor.shard_rows()[0]
    hot_packed = packed._shard_tensor().shard_tensor.shard_rows()[0]
    assert hot_plain == 16 * 1024 // 400
    assert hot_packed == 16 * 1024 // 112
    assert hot_packed > hot_plain


def test_prefetcher_yields_dequantized_rows(small_graph):
    g = torch.Generator().manual_seed(33)
    x = torch.randn(500, DIM, generator=g)
    topo, feature = _feature(small_graph, x, quantize="int8")
    ref = _reference(x, torch.float32)
    sampler = quiver.GraphSageSampler(topo, [5, 3], device=0, mode="GPU")
    batches = [torch.randint(0, 500, (64,), generator=g) for _ in range(4)]
    seen = 0
    for n_id, bs, adjs, feats in quiver.TrainingPrefetcher(
            sampler, feature, batches, depth=2, device=0):
        torch.cuda.synchronize()
        assert bs == 64
        assert feats.shape == (n_id.numel(), DIM)
        assert _within_one_ulp(feats, ref[n_id.cpu()])
        seen += 1
    assert seen == 4


def test_dist_feature_over_quantized_store(small_graph):
    """DistFeature sizes its result by feature.size(1): the dequantized
    width, not the packed one."""
    g = torch.Generator().manual_seed(36)
    x = torch.randn(500, DIM, generator=g)
    _, feature = _feature(small_graph, x, quantize="int8")
    comm = quiver.NcclComm(0, 1, quiver.getNcclId(), hosts=1,
                           rank_per_host=1)
    info = quiver.PartitionInfo(0, 0, 1, torch.zeros(500, dtype=torch.int64))
    dist_feature = quiver.DistFeature(feature, info, comm)
    ids = torch.randint(0, 500, (700,), generator=g)
    got = dist_feature[ids]
    assert got.shape == (700, DIM)
    assert _within_one_ulp(got, _reference(x, torch.float32)[ids])


def _ipc_child(handle, ref, idx, q):
    try:
        torch.cuda.set_device(0)
        feature = quiver.Feature.lazy_from_ipc_handle(handle)
        got = feature[idx.cuda()]
        q.put(bool(_within_one_ulp(got, ref[idx])
                   and tuple(feature.shape) == tuple(ref.shape)))
    except Exception as e:  # reported to the parent, which fails the test
        q.put(repr(e))
        raise


def _run_ipc_child(handle, ref, idx):
    ctx = mp.get_context("spawn")
    q = ctx.SimpleQueue()
    p = ctx.Process(target=_ipc_child, args=(handle, ref, idx, q))
    p.start()
    p.join(timeout=120)
    if p.is_alive():
        p.kill()
        p.join()
        pytest.fail("ipc child did not finish")
    result = None if q.empty() else q.get()
    assert p.exitcode == 0 and result is True, (p.exitcode, result)


def test_ipc_handle_of_quantized_store(small_graph):
    g = torch.Generator().manual_seed(34)
    x = torch.randn(500, DIM, generator=g)
    _, feature = _feature(small_graph, x, quantize="int8",
                          out_dtype=torch.bfloat16)
    handle = feature.share_ipc()
    assert len(handle) == 7 and handle[6] == (DIM, torch.bfloat16)
    for items in handle[0].values():
        assert all(len(item) == 7 for item in items)
    idx = torch.randint(0, 500, (300,), generator=g)
    _run_ipc_child(handle, _reference(x, torch.bfloat16), idx)


def test_six_field_handle_of_plain_store_still_loads(small_graph):
    g = torch.Generator().manual_seed(35)
    x = torch.randn(500, DIM, generator=g)
    _, feature = _feature(small_graph, x)
    handle = feature.share_ipc()
    assert len(handle) == 6
    for items in handle[0].values():
        assert all(len(item) == 5 for item in items)
    idx = torch.randint(0, 500, (300,), generator=g)
    _run_ipc_child(handle, x, idx)  # equal rows are zero ulps apart
