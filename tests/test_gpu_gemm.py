"""_ext.tall_gemm (csrc/gemm_kernels.hip) against float64, computed on the
GPU from the same fp32 inputs.

Three kinds of input, because they catch different faults:
- integer-valued operands: every partial sum is an integer below 2^24, so
  any fp32 summation order is exact and the result must EQUAL the fp64 one
  (a dropped, duplicated or misplaced element fails at every shape);
- a selection matrix B: C[:, n] must be bit-equal to A[:, sel[n]], which
  catches any narrowing of the operands;
- random floats: the kernel is a k-ordered fp32 fmaf chain plus one add for
  the bias, so |c - ref| <= (K + 1) * 2^-24 * (|A| @ |B| + |bias|)
  elementwise — the standard bound, not a measured one.

The shapes live in _gemm_cases.py with the constants of the kernel and of
launch_tall_gemm that they are computed from.
"""
import os
import sys

import pytest
import torch

import quiver  # noqa: F401
from quiver import _ext

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _gemm_cases as gc  # noqa: E402  (shared case lists, same folder)

pytestmark = pytest.mark.gpu

DEV = "cuda"
ALL_SHAPES = gc.GEMM_SMALL + gc.GEMM_WALK


def _gen(seed):
    return torch.Generator(device=DEV).manual_seed(seed)


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same_bits(x, y):
    return x.shape == y.shape and torch.equal(_bits(x), _bits(y))


def _int_inputs(m, k, n, bias, seed=0, device=DEV):
    g = torch.Generator(device=device).manual_seed(seed)
    a = gc.rand_ints((m, k), 8, g, device)
    b = gc.rand_ints((k, n), 8, g, device)
    bv = gc.rand_ints((n,), 8, g, device) if bias else None
    return a, b, bv


def _ref64(a, b, bias):
    ref = a.double() @ b.double()
    return ref if bias is None else ref + bias.double()


# ---------------------------------------------------------------------------
# a. integer-valued inputs: exact equality
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("bias", [False, True], ids=["nobias", "bias"])
@pytest.mark.parametrize("m,k,n", ALL_SHAPES)
def test_tall_gemm_integer_exact(m, k, n, bias):
    assert 64 * k + 8 < gc.EXACT_LIMIT
    a, b, bv = _int_inputs(m, k, n, bias)
    c = _ext.tall_gemm(a, b, bv)
    assert c.shape == (m, n) and c.dtype == torch.float32
    assert torch.equal(c.double(), _ref64(a, b, bv))


# ---------------------------------------------------------------------------
# b. selection matrix: the mantissa survives
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("m,k,n", ALL_SHAPES)
def test_tall_gemm_selection_is_bit_exact(m, k, n):
    g = _gen(1)
    a = torch.randn(m, k, device=DEV, generator=g)
    sel = torch.randint(0, k, (n,), device=DEV, generator=g)
    b = torch.zeros(k, n, device=DEV)
    b[sel, torch.arange(n, device=DEV)] = 1.0
    c = _ext.tall_gemm(a, b, None)
    # fma(a, 1, 0) == a and every other term adds an exact zero
    assert torch.equal(c, a[:, sel])


# ---------------------------------------------------------------------------
# c. random floats: the derived bound
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("bias", [False, True], ids=["nobias", "bias"])
@pytest.mark.parametrize("m,k,n", ALL_SHAPES)
def test_tall_gemm_random_within_fma_chain_bound(m, k, n, bias):
    g = _gen(2)
    a = torch.randn(m, k, device=DEV, generator=g)
    b = torch.randn(k, n, device=DEV, generator=g)
    bv = torch.randn(n, device=DEV, generator=g) if bias else None
    c = _ext.tall_gemm(a, b, bv)
    err = (c.double() - _ref64(a, b, bv)).abs()
    bound = gc.gemm_bound(a, b, bv, k)
    worst = float((err / bound.clamp_min(1e-300)).max())
    print(f"tall_gemm {m}x{k}x{n} bias={bias}: max err/bound = {worst:.3g}")
    assert bool((err <= bound).all()), worst


# ---------------------------------------------------------------------------
# isolation
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("row", [70, 129], ids=["second_tile", "last_row"])
def test_tall_gemm_nan_stays_in_its_row(row):
    m, k, n = 130, 47, 100
    g = _gen(3)
    a = torch.randn(m, k, device=DEV, generator=g)
    b = torch.randn(k, n, device=DEV, generator=g)
    bv = torch.randn(n, device=DEV, generator=g)
    clean = _ext.tall_gemm(a, b, bv)
    a_nan = a.clone()
    a_nan[row, 13] = float("nan")
    c = _ext.tall_gemm(a_nan, b, bv)
    assert bool(c[row].isnan().all())
    keep = torch.arange(m, device=DEV) != row
    assert not bool(clean.isnan().any())
    assert _same_bits(c[keep], clean[keep])


def _in_nan_moat(t):
    """The same values as a contiguous view into the middle of a larger
    NaN-filled buffer: 64 floats in, so 16-byte alignment is kept and the
    binding's .contiguous() makes no copy."""
    buf = torch.full((t.numel() + 128,), float("nan"), device=t.device)
    view = buf[64:64 + t.numel()].view(t.shape)
    view.copy_(t)
    assert view.is_contiguous() and view.data_ptr() % 16 == 0
    return view


@pytest.mark.parametrize("m,k,n", [(130, 47, 100), (65, 32, 64),
                                   (63, 100, 130), (200, 64, 128),
                                   (1, 1, 1)])
def test_tall_gemm_reads_nothing_past_its_operands(m, k, n):
    g = _gen(4)
    a = torch.randn(m, k, device=DEV, generator=g)
    b = torch.randn(k, n, device=DEV, generator=g)
    bv = torch.randn(n, device=DEV, generator=g)
    want = _ext.tall_gemm(a, b, bv)
    got = _ext.tall_gemm(_in_nan_moat(a), _in_nan_moat(b), _in_nan_moat(bv))
    assert not bool(want.isnan().any())
    assert _same_bits(got, want)


# ---------------------------------------------------------------------------
# the binding
# ---------------------------------------------------------------------------
def _gemm_args():
    a, b, bv = _int_inputs(70, 12, 9, True)
    return {"a": a, "b": b, "bias": bv}


def _call(args):
    return _ext.tall_gemm(args["a"], args["b"], args["bias"])


_BREAK = {
    "weight_on_cpu": lambda d: d.update(b=d["b"].cpu()),
    "bias_on_cpu": lambda d: d.update(bias=d["bias"].cpu()),
    "a_on_cpu": lambda d: d.update(a=d["a"].cpu()),
    "weight_1d": lambda d: d.update(b=d["b"].reshape(-1)),
    "a_1d": lambda d: d.update(a=d["a"].reshape(-1)),
    "bias_2d": lambda d: d.update(bias=d["bias"].reshape(1, -1)),
    "inner_mismatch": lambda d: d.update(b=d["b"][:-1]),
    "bias_too_short": lambda d: d.update(bias=d["bias"][:-1]),
    "bias_too_long": lambda d: d.update(bias=torch.cat([d["bias"]] * 2)),
    "a_fp64": lambda d: d.update(a=d["a"].double()),
    "weight_fp64": lambda d: d.update(b=d["b"].double()),
    "bias_fp64": lambda d: d.update(bias=d["bias"].double()),
}


@pytest.mark.parametrize("fault", sorted(_BREAK))
def test_tall_gemm_bad_arguments_raise(fault):
    args = _gemm_args()
    c = _call(args)  # the well-formed call goes through
    assert torch.equal(c.double(), _ref64(args["a"], args["b"], args["bias"]))
    _BREAK[fault](args)
    with pytest.raises(RuntimeError):
        _call(args)


@pytest.mark.parametrize("bias", [False, True], ids=["nobias", "bias"])
def test_tall_gemm_empty_dimensions(bias):
    def run(m, k, n):
        a, b, bv = _int_inputs(m, k, n, bias)
        return _ext.tall_gemm(a, b, bv), bv

    c, _ = run(0, 12, 9)
    assert c.shape == (0, 9)
    c, _ = run(70, 12, 0)
    assert c.shape == (70, 0)
    c, _ = run(0, 0, 0)
    assert c.shape == (0, 0)
    # K == 0: an empty sum, so the bias broadcast (or zeros)
    for m in (1, 70, 200):
        c, bv = run(m, 0, 9)
        want = bv.expand(m, 9) if bias else torch.zeros(m, 9, device=DEV)
        assert c.shape == (m, 9) and torch.equal(c, want)


@pytest.mark.skipif(torch.cuda.device_count() < 2, reason="needs two GPUs")
def test_tall_gemm_on_a_device_that_is_not_current():
    torch.cuda.set_device(0)
    a, b, bv = _int_inputs(200, 47, 100, True, device="cuda:1")
    c = _ext.tall_gemm(a, b, bv)
    assert torch.cuda.current_device() == 0
    assert c.device == a.device
    assert torch.equal(c.double(), _ref64(a, b, bv))
