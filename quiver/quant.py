"""8-bit feature rows: one code byte per channel plus a per-row fp32 scale
and offset, dequantized inside the gather kernel
(csrc/gather_kernels.hip, gather_dequant_kernel).

Packed row, ``row_bytes = round_up(dim + 8, 16)`` bytes:

    [0, dim)                      codes q, uint8
    [dim, row_bytes - 8)          zero padding
    [row_bytes - 8, row_bytes)    scale (fp32), lo (fp32), little-endian

and a channel's value is ``lo + scale * q``.  With the codes at offset 0
the 16-byte code chunk j holds output channels 16j .. 16j+15.

Per row ``lo = min(x)``, ``scale = float32((max - min) / 255)`` and
``q = clamp(round_half_even((x - lo) / scale), 0, 255)``, all in fp64, so
every element comes back within ``scale / 2`` (plus the fp32 rounding of
``scale``, below 2**-22 * max|row|).
"""
import torch

__all__ = ["packed_row_bytes", "quantize_rows", "dequantize_rows"]

TAIL_BYTES = 8  # scale, lo


def packed_row_bytes(dim: int) -> int:
    return (dim + TAIL_BYTES + 15) // 16 * 16


def quantize_rows(x: torch.Tensor, chunk_rows: int = 1 << 20) -> torch.Tensor:
    """Pack a CPU float tensor [N, dim] into uint8 [N, row_bytes].

    Works ``chunk_rows`` rows at a time: the fp64 temporaries are the size
    of a chunk, never of the input."""
    if x.device.type != "cpu" or x.dim() != 2 or not x.is_floating_point():
        raise ValueError("quantize_rows needs a 2-D floating-point CPU "
                         "tensor")
    if chunk_rows < 1:
        raise ValueError("chunk_rows must be positive")
    n, dim = x.shape
    row_bytes = packed_row_bytes(dim)
    out = torch.zeros((n, row_bytes), dtype=torch.uint8)
    for beg in range(0, n, chunk_rows):
        xc = x[beg:beg + chunk_rows].double()
        finite = torch.isfinite(xc).all(dim=1)
        if not bool(finite.all()):
            bad = beg + int((~finite).nonzero()[0])
            raise ValueError(f"quantize_rows: non-finite value in row {bad}")
        if dim == 0:
            continue
        lo = xc.min(dim=1, keepdim=True).values.float()
        hi = xc.max(dim=1, keepdim=True).values
        scale = ((hi - lo.double()) / 255).float()
        # scale == 0: a constant row (or a range below fp32's smallest
        # subnormal * 255); every code is 0 and the row decodes to lo
        safe = torch.where(scale > 0, scale, torch.ones_like(scale)).double()
        q = torch.round((xc - lo.double()) / safe).clamp_(0, 255)
        q = torch.where(scale > 0, q, torch.zeros_like(q))
        rows = out[beg:beg + chunk_rows]
        rows[:, :dim] = q.to(torch.uint8)
        rows[:, row_bytes - TAIL_BYTES:] = \
            torch.cat([scale, lo], dim=1).contiguous().view(torch.uint8)
    return out


def _round_once(v: torch.Tensor, dtype: torch.dtype) -> torch.Tensor:
    """fp64 -> dtype with a single rounding.  torch converts fp64 to a
    16-bit float by way of fp32, which rounds twice; going through fp32
    rounded to odd instead makes the final round-to-nearest-even see the
    exact value's sticky bit."""
    if dtype in (torch.float32, torch.float64):
        return v.to(dtype)
    f = v.float()
    fd = f.double()
    bits = f.view(torch.int32)
    # truncate toward zero where the fp32 rounding went away from zero ...
    bits = torch.where(fd.abs() > v.abs(), bits - 1, bits)
    # ... and make the last bit odd wherever fp32 was inexact
    bits = torch.where(fd != v, bits | 1, bits)
    return bits.view(torch.float32).to(dtype)


def dequantize_rows(packed: torch.Tensor, dim: int,
                    dtype: torch.dtype = torch.float32) -> torch.Tensor:
    """CPU reference of the gather kernel's dequantization:
    ``lo + scale * q`` in fp64, rounded once to ``dtype``."""
    if packed.dtype != torch.uint8 or packed.dim() != 2 or \
            packed.size(1) != packed_row_bytes(dim):
        raise ValueError(f"dequantize_rows: expected uint8 "
                         f"[N, {packed_row_bytes(dim)}] for dim {dim}")
    packed = packed.cpu()
    tail = packed[:, -TAIL_BYTES:].contiguous().view(torch.float32).double()
    q = packed[:, :dim].double()
    return _round_once(tail[:, 1:2] + tail[:, 0:1] * q, dtype)
