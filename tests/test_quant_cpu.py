"""Packed int8 row format (quiver/quant.py) on the CPU: layout, the error
bound that follows from the format, and the argument checks of the
Feature front end."""
import pytest
import torch

import quiver
from quiver.quant import packed_row_bytes


def _tail(packed):
    """[N, 2] fp32: scale, lo."""
    return packed[:, -8:].contiguous().view(torch.float32)


@pytest.mark.parametrize("dim", [1, 7, 8, 9, 100, 128])
def test_layout(dim):
    g = torch.Generator().manual_seed(dim)
    x = torch.randn(50, dim, generator=g)
    packed = quiver.quantize_rows(x)
    row_bytes = (dim + 8 + 15) // 16 * 16
    assert packed_row_bytes(dim) == row_bytes
    assert packed.dtype == torch.uint8
    assert packed.shape == (50, row_bytes)
    assert packed.is_contiguous()

    tail = _tail(packed)
    scale, lo = tail[:, 0], tail[:, 1]
    xmin, xmax = x.min(dim=1).values, x.max(dim=1).values
    assert torch.equal(lo, xmin)
    want_scale = ((xmax.double() - xmin.double()) / 255).float()
    assert torch.equal(scale, want_scale)

    # codes start at byte 0, computed in fp64, ties to even
    if dim > 1:
        q = torch.round((x.double() - lo.double()[:, None])
                        / scale.double()[:, None]).clamp(0, 255)
        assert torch.equal(packed[:, :dim], q.to(torch.uint8))
    else:
        assert torch.equal(packed[:, :dim], torch.zeros(50, 1,
                                                        dtype=torch.uint8))
    # padding between the codes and the tail is zero
    assert int(packed[:, dim:row_bytes - 8].sum()) == 0


def _bound_cases():
    g = torch.Generator().manual_seed(21)
    x = torch.randn(4000, 100, generator=g)
    return {
        "randn": x,
        "logspace_cols": x * torch.logspace(-6, 6, 100),
        "x1e30": x * 1e30,
        "x1e-30": x * 1e-30,
    }


@pytest.mark.parametrize("name", ["randn", "logspace_cols", "x1e30",
                                  "x1e-30"])
def test_error_bound(name):
    """|dequantize(quantize(x)) - x| <= scale/2 + 2**-22 * max|row|."""
    x = _bound_cases()[name]
    packed = quiver.quantize_rows(x)
    back = quiver.dequantize_rows(packed, 100, torch.float64)
    scale = _tail(packed)[:, 0].double()[:, None]
    bound = scale / 2 + 2.0 ** -22 * x.double().abs().max(dim=1,
                                                           keepdim=True).values
    err = (back - x.double()).abs()
    worst = float((err / bound).max())
    print(f"{name}: max err / bound = {worst:.6f}, "
          f"max err / (scale/2) = {float((err / (scale / 2)).max()):.6f}")
    assert bool((err <= bound).all()), worst
    # codes reach both ends of the range on every (non-constant) row
    codes = packed[:, :100]
    assert bool((codes.min(dim=1).values == 0).all())
    assert bool((codes.max(dim=1).values == 255).all())


def test_constant_rows_round_trip_exactly():
    x = torch.tensor([[3.25] * 9, [0.0] * 9, [-1e-20] * 9, [7e20] * 9])
    packed = quiver.quantize_rows(x)
    assert int(packed[:, :9].sum()) == 0
    assert torch.equal(_tail(packed)[:, 0], torch.zeros(4))
    for dtype in (torch.float32, torch.float64):
        assert torch.equal(quiver.dequantize_rows(packed, 9, dtype),
                           x.to(dtype))


def test_chunking_gives_the_same_bytes():
    g = torch.Generator().manual_seed(22)
    x = torch.randn(20, 37, generator=g)
    assert torch.equal(quiver.quantize_rows(x, chunk_rows=3),
                       quiver.quantize_rows(x))


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_dequantize_rounds_once(dtype):
    """The reference rounds fp64 to a 16-bit dtype once: it is the nearest
    value of that dtype to the fp64 result (ties aside)."""
    g = torch.Generator().manual_seed(23)
    x = torch.randn(300, 100, generator=g)
    packed = quiver.quantize_rows(x)
    exact = quiver.dequantize_rows(packed, 100, torch.float64)
    got = quiver.dequantize_rows(packed, 100, dtype)
    assert got.dtype == dtype
    info = torch.finfo(dtype)
    # spacing of dtype at got: eps * 2**floor(log2 |got|)
    e = torch.floor(torch.log2(got.double().abs().clamp_min(info.tiny)))
    ulp = info.eps * torch.pow(torch.tensor(2.0, dtype=torch.float64), e)
    assert bool(((got.double() - exact).abs() <= ulp / 2).all())


@pytest.mark.parametrize("bad", [float("nan"), float("inf"), -float("inf")])
def test_non_finite_input_names_the_row(bad):
    x = torch.zeros(10, 5)
    x[6, 2] = bad
    x[8, 0] = bad
    with pytest.raises(ValueError, match="row 6"):
        quiver.quantize_rows(x, chunk_rows=4)


def test_quantize_rows_rejects_other_inputs():
    with pytest.raises(ValueError):
        quiver.quantize_rows(torch.zeros(4, 4, dtype=torch.int32))
    with pytest.raises(ValueError):
        quiver.quantize_rows(torch.zeros(4))
    with pytest.raises(ValueError):
        quiver.dequantize_rows(torch.zeros(4, 16, dtype=torch.uint8), 100)


def test_bad_quantize_value_raises():
    feature = quiver.Feature(0, device_list=[0], device_cache_size=0)
    x = torch.zeros(10, 4)
    with pytest.raises(ValueError, match="quantize"):
        feature.from_cpu_tensor(x, quantize="int4")
    with pytest.raises(ValueError, match="out_dtype"):
        feature.from_cpu_tensor(x, quantize="int8", out_dtype=torch.int32)
    with pytest.raises(ValueError, match="out_dtype"):
        feature.from_cpu_tensor(x, out_dtype=torch.float16)


def test_quantize_with_mmap_raises():
    feature = quiver.Feature(0, device_list=[0], device_cache_size=0)
    cfg = quiver.DeviceConfig([torch.zeros(0, 4)], torch.zeros(0, 4))
    with pytest.raises(NotImplementedError):
        feature.from_mmap(None, cfg, quantize="int8")
    # a quantized store arriving as an IPC handle (seven fields)
    handle = ({}, None, [0], 0, "device_replicate", None,
              (4, torch.float32))
    lazy = quiver.Feature.lazy_from_ipc_handle(handle)
    with pytest.raises(NotImplementedError):
        lazy.set_mmap_file("unused.npy", torch.zeros(4, dtype=torch.int64))
