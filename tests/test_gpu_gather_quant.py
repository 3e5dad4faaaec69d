"""Gather of int8 rows dequantized in the kernel, over an HBM shard plus a
pinned-host shard: every packed row shape and output dtype, the index sets
of test_gpu_gather_cold.py, the device-side count, the order fold, skipped
ids, the ignored reuse flag, single-tier stores and the native guards.

Reference: quiver.dequantize_rows (fp64, rounded once to the output
dtype).  The kernel rounds the exact q * scale + lo once to fp32 (fmaf)
and, for a 16-bit output, once more; the reference rounds it to fp64 and
then to the output dtype.  The two can differ by one unit in the last
place of the output dtype and no more, which is the tolerance here."""
import functools

import pytest
import torch

import quiver
from quiver.shard_tensor import ShardTensor, ShardTensorConfig

pytestmark = pytest.mark.gpu

N_HOT, N_COLD = 3000, 5000
N_ROWS = N_HOT + N_COLD

DIMS = [
    8,     # 16 B: one chunk, no padding
    1,     # 16 B: the tail and the single code in one chunk
    9,     # 32 B: partial last chunk, output rows not 16-byte aligned
    7,     # 16 B: likewise; bf16/fp16 rows not 4-byte aligned
    100,   # 112 B: 7 chunks, the products shape
    128,   # 144 B: the papers100M shape
    602,   # 624 B: 39 chunks, the widest sub-group
    1100,  # 1120 B: 70 chunks, a second pass of the sub-group
]
OUT_DTYPES = [torch.float32, torch.bfloat16, torch.float16]

shapes = pytest.mark.parametrize("dim", DIMS)
out_dtypes = pytest.mark.parametrize(
    "out_dtype", OUT_DTYPES, ids=["fp32", "bf16", "fp16"])


def _ordinal(t):
    """Floats as integers whose difference is the distance in units in
    the last place (+0 and -0 coincide)."""
    if t.dtype == torch.float32:
        bits = t.contiguous().view(torch.int32).to(torch.int64)
        mag = bits & 0x7FFFFFFF
    else:
        bits = t.contiguous().view(torch.int16).to(torch.int64)
        mag = bits & 0x7FFF
    return torch.where(bits < 0, -mag, mag)


def _assert_one_ulp(got, want, what):
    got = got.cpu()
    assert got.dtype == want.dtype, what
    assert got.shape == want.shape, what
    if got.numel() == 0:
        return
    assert bool(torch.isfinite(got.float()).all()), what
    dist = int((_ordinal(got) - _ordinal(want)).abs().max())
    assert dist <= 1, f"{what}: {dist} ulp"


@functools.lru_cache(maxsize=None)
def _packed(dim):
    g = torch.Generator().manual_seed(11)
    return quiver.quantize_rows(torch.randn(N_ROWS, dim, generator=g))


@functools.lru_cache(maxsize=None)
def _table(dim, out_dtype):
    """(cpu reference rows, mixed-tier store); built once, never written."""
    packed = _packed(dim)
    st = ShardTensor(0, ShardTensorConfig({}), dequant=(dim, out_dtype))
    st.append(packed[:N_HOT], 0)
    st.append(packed[N_HOT:], -1)
    return quiver.dequantize_rows(packed, dim, out_dtype), st


def _rows_per_block_iter(dim):
    """Rows one 256-thread block takes per iteration (mirrors the
    launcher: a sub-group covers the row's 16-byte code chunks)."""
    nchunk = (dim + 15) // 16
    sub = 4
    while sub < 64 and sub < nchunk:
        sub *= 2
    return 256 // sub


def _index_sets(dim):
    g = torch.Generator().manual_seed(5)
    rpb = _rows_per_block_iter(dim)
    sets = {}
    for L in sorted({0, 1, 2, rpb - 1, rpb, rpb + 1}):
        sets[f"cold_len{L}"] = torch.randint(N_HOT, N_ROWS, (L,), generator=g)
    sets["mixed_20000"] = torch.randint(0, N_ROWS, (20000,), generator=g)
    sets["all_hot"] = torch.randint(0, N_HOT, (700,), generator=g)
    sets["all_cold"] = torch.randint(N_HOT, N_ROWS, (20000,), generator=g)
    alt = torch.empty(1001, dtype=torch.int64)
    alt[0::2] = torch.randint(0, N_HOT, (501,), generator=g)
    alt[1::2] = torch.randint(N_HOT, N_ROWS, (500,), generator=g)
    sets["alternating"] = alt
    sets["same_cold_x64"] = torch.full((64,), N_HOT + 1234, dtype=torch.int64)
    return sets


@shapes
@out_dtypes
def test_index_sets(dim, out_dtype):
    ref, st = _table(dim, out_dtype)
    assert st.shape == (N_ROWS, dim)
    assert st.size(0) == N_ROWS and st.size(1) == dim
    for name, idx in _index_sets(dim).items():
        got = st[idx.cuda()]
        assert got.shape == (idx.numel(), dim), name
        assert got.dtype == out_dtype, name
        _assert_one_ulp(got, ref[idx], name)


@shapes
@out_dtypes
def test_neighbouring_rows_untouched(dim, out_dtype):
    """A skipped row between two gathered ones keeps what it held: no
    store of a partial last chunk reaches past its row."""
    ref, st = _table(dim, out_dtype)
    g = torch.Generator().manual_seed(15)
    idx = torch.randint(0, N_ROWS, (600,), generator=g)
    skipped = torch.arange(1, 600, 2)
    idx[skipped] = -1
    idx_dev = idx.cuda()
    # With no allocation in between, the caching allocator hands a freed
    # block to the next request of the same size: the gather's output
    # starts out holding the marker.
    for _ in range(3):
        marker = torch.full((600, dim), 3.0, dtype=out_dtype, device="cuda")
        ptr = marker.data_ptr()
        del marker
        got = st[idx_dev]
        if got.data_ptr() == ptr:
            break
    assert got.data_ptr() == ptr, "the marked block was not reused"
    kept = torch.arange(0, 600, 2)
    _assert_one_ulp(got[kept], ref[idx[kept]], "gathered rows")
    assert bool((got[skipped].cpu() == 3.0).all())


@shapes
@out_dtypes
@pytest.mark.parametrize("k", [0, 1000])
def test_gather_n_device_count(dim, out_dtype, k):
    """Upper-bound frontier, exact count on the device: only the counted
    rows are compared."""
    ref, st = _table(dim, out_dtype)
    g = torch.Generator().manual_seed(8)
    idx = torch.zeros(4096, dtype=torch.int64)
    idx[:k] = torch.randint(0, N_ROWS, (k,), generator=g)
    n_dev = torch.tensor([k], dtype=torch.int64, device="cuda")
    got = st.gather_n(idx.cuda(), n_dev)
    assert got.shape == (4096, dim) and got.dtype == out_dtype
    _assert_one_ulp(got[:k], ref[idx[:k]], f"k={k}")


@shapes
@out_dtypes
def test_order_fold(dim, out_dtype):
    ref, st = _table(dim, out_dtype)
    g = torch.Generator().manual_seed(9)
    order = torch.randperm(N_ROWS, generator=g)
    idx = torch.randint(0, N_ROWS, (3000,), generator=g)
    want = ref[order[idx]]
    _assert_one_ulp(st.gather(idx.cuda(), order.cuda()), want, "gather")
    n_dev = torch.tensor([2500], dtype=torch.int64, device="cuda")
    got = st.gather_n(idx.cuda(), n_dev, order.cuda())
    _assert_one_ulp(got[:2500], want[:2500], "gather_n")


@pytest.mark.parametrize("dim", [7, 100, 1100])
@out_dtypes
def test_out_of_range_and_negative_ids_skipped(dim, out_dtype):
    ref, st = _table(dim, out_dtype)
    g = torch.Generator().manual_seed(6)
    idx = torch.randint(0, N_ROWS, (301,), generator=g)
    idx[150], idx[7], idx[300] = N_ROWS + 7, -5, N_ROWS
    keep = torch.ones(301, dtype=torch.bool)
    keep[[150, 7, 300]] = False
    got = st[idx.cuda()]
    _assert_one_ulp(got[keep], ref[idx[keep]], "no order")
    # with an order table: ids outside [0, len(order)) are skipped too
    order = torch.randperm(N_ROWS, generator=g)[:N_ROWS - 100]
    idx[20] = N_ROWS - 100
    keep[20] = False
    idx[keep] = idx[keep].clamp(max=N_ROWS - 101)
    got = st.gather(idx.cuda(), order.cuda())
    _assert_one_ulp(got[keep], ref[order[idx[keep]]], "order")


@pytest.mark.parametrize("dim", [9, 100])
@out_dtypes
def test_reuse_flag_has_no_effect(dim, out_dtype):
    """gather_n(reuse=True) is accepted by a dequantizing store and gives
    the rows reuse=False gives, over overlapping consecutive batches."""
    ref, st = _table(dim, out_dtype)
    g = torch.Generator().manual_seed(16)
    shared = torch.randint(N_HOT, N_ROWS, (1500,), generator=g)
    for b in range(4):
        idx = torch.cat([shared,
                         torch.randint(0, N_ROWS, (1500,), generator=g)])
        idx = idx[torch.randperm(idx.numel(), generator=g)]
        n_dev = torch.tensor([2800], dtype=torch.int64, device="cuda")
        with_flag = st.gather_n(idx.cuda(), n_dev, None, True)
        without = st.gather_n(idx.cuda(), n_dev, None, False)
        assert torch.equal(with_flag[:2800], without[:2800]), b
        _assert_one_ulp(with_flag[:2800], ref[idx[:2800]], f"batch {b}")


@pytest.mark.parametrize("dim", [9, 100])
@out_dtypes
def test_hot_only_and_cold_only_stores(dim, out_dtype):
    packed = _packed(dim)[:4000]
    ref = quiver.dequantize_rows(packed, dim, out_dtype)
    g = torch.Generator().manual_seed(17)
    idx = torch.randint(0, 4000, (5000,), generator=g)
    n_dev = torch.tensor([3000], dtype=torch.int64, device="cuda")
    for device in (0, -1):
        st = ShardTensor(0, ShardTensorConfig({}), dequant=(dim, out_dtype))
        st.append(packed, device)
        _assert_one_ulp(st[idx.cuda()], ref[idx], f"device {device}")
        _assert_one_ulp(st.gather_n(idx.cuda(), n_dev)[:3000],
                        ref[idx[:3000]], f"device {device}, gather_n")


def test_native_guards():
    packed = _packed(100)
    st = ShardTensor(0, ShardTensorConfig({}), dequant=(100, torch.float32))
    with pytest.raises(RuntimeError, match="uint8 rows of 112"):
        st.shard_tensor.append(packed[:10, :96].contiguous(), 0)
    with pytest.raises(RuntimeError, match="uint8 rows of 112"):
        st.shard_tensor.append(torch.zeros(10, 112), 0)
    with pytest.raises(RuntimeError, match="contiguous"):
        st.shard_tensor.append(
            torch.zeros(10, 224, dtype=torch.uint8)[:, ::2], 0)
    assert st.shard_tensor.shard_count() == 0
    st.append(packed[:100], 0)
    with pytest.raises(RuntimeError, match="already has shards"):
        st.shard_tensor.set_dequant(100, torch.float32)
    with pytest.raises(RuntimeError, match="uint8 rows of 112"):
        st.shard_tensor.scatter_update(
            torch.arange(4).cuda(), torch.zeros(4, 100, device="cuda"))

    plain = ShardTensor(0, ShardTensorConfig({}))
    plain.append(torch.zeros(10, 4), 0)
    with pytest.raises(RuntimeError, match="already has shards"):
        plain.shard_tensor.set_dequant(4, torch.float32)
    empty = ShardTensor(0, ShardTensorConfig({}))
    with pytest.raises(RuntimeError, match="out_dtype"):
        empty.shard_tensor.set_dequant(4, torch.float64)
    with pytest.raises(RuntimeError, match="dim"):
        empty.shard_tensor.set_dequant(0, torch.float32)


@out_dtypes
def test_scatter_update_with_packed_rows(out_dtype):
    dim = 100
    packed = _packed(dim).clone()
    st = ShardTensor(0, ShardTensorConfig({}), dequant=(dim, out_dtype))
    st.append(packed[:N_HOT], 0)
    st.append(packed[N_HOT:], -1)
    g = torch.Generator().manual_seed(18)
    rows = torch.randperm(N_ROWS, generator=g)[:500]  # both tiers
    new = quiver.quantize_rows(torch.randn(500, dim, generator=g) * 3 + 1)
    st.shard_tensor.scatter_update(rows.cuda(), new.cuda())
    want = quiver.dequantize_rows(packed, dim, out_dtype)
    want[rows] = quiver.dequantize_rows(new, dim, out_dtype)
    idx = torch.cat([rows, torch.randint(0, N_ROWS, (2000,), generator=g)])
    _assert_one_ulp(st[idx.cuda()], want[idx], "after scatter_update")
