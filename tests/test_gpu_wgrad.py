"""Numerics of the split-K weight-grad kernel (csrc/wgrad_kernels.hip)
against float64, and of QLinear end-to-end autograd: values, routing and
the argument checks of the binding."""
import os
import sys

import pytest
import torch
import torch.nn.functional as F

import quiver  # noqa: F401
import quiver.nn as qnn
from quiver import _ext
from quiver.nn import QLinear, _WGRAD_MIN_K

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _gemm_cases as gc  # noqa: E402  (shared case lists, same folder)

pytestmark = pytest.mark.gpu

DEV = "cuda"


def _gen(seed, device=DEV):
    return torch.Generator(device=device).manual_seed(seed)


def _same_bits(x, y):
    return x.shape == y.shape and torch.equal(
        x.contiguous().view(torch.int32), y.contiguous().view(torch.int32))


@pytest.mark.parametrize("k,m,n", [(1000, 100, 256), (200_000, 100, 256),
                                   (50_000, 256, 256), (33_000, 47, 256),
                                   (70_000, 64, 64), (16, 3, 5)])
def test_wgrad_matches_torch(k, m, n):
    g = torch.Generator(device="cuda").manual_seed(0)
    a = torch.randn(k, m, device="cuda", generator=g)
    b = torch.randn(k, n, device="cuda", generator=g)
    c, bias = _ext.wgrad(a, b, True)
    # fp64 ground truth; fp32 split-K accumulation error grows ~sqrt(K),
    # so judge by relative error against the fp64 result
    want_c = (a.double().t() @ b.double())
    want_bias = a.double().sum(0)
    rel_c = (c.double() - want_c).norm() / want_c.norm()
    rel_b = (bias.double() - want_bias).norm() / max(want_bias.norm(), 1e-30)
    assert rel_c < 1e-5, float(rel_c)
    assert rel_b < 1e-4, float(rel_b)  # bias sums can cancel toward 0


def test_wgrad_no_bias():
    a = torch.randn(5000, 32, device="cuda")
    b = torch.randn(5000, 16, device="cuda")
    c, bias = _ext.wgrad(a, b, False)
    assert bias is None
    assert torch.allclose(c, a.t() @ b, atol=1e-2, rtol=1e-4)


def test_qlinear_autograd_matches_nn_linear():
    k = _WGRAD_MIN_K + 100
    torch.manual_seed(0)
    x = torch.randn(k, 100, device="cuda", requires_grad=True)
    ql = QLinear(100, 256).cuda()
    ref = torch.nn.Linear(100, 256).cuda()
    with torch.no_grad():
        ref.weight.copy_(ql.weight)
        ref.bias.copy_(ql.bias)
    x2 = x.detach().clone().requires_grad_(True)

    out = ql(x)
    out.pow(2).mean().backward()
    out2 = ref(x2)
    out2.pow(2).mean().backward()

    assert torch.allclose(out, out2, atol=1e-5)
    assert torch.allclose(x.grad, x2.grad, atol=1e-5, rtol=1e-4)
    assert torch.allclose(ql.weight.grad, ref.weight.grad,
                          atol=1e-3, rtol=1e-3)
    assert torch.allclose(ql.bias.grad, ref.bias.grad, atol=1e-3, rtol=1e-3)


def test_wgrad_deterministic():
    """Split-K partials are reduced in fixed order (workspace + reduce
    kernel), so repeated calls on identical inputs are bitwise equal —
    unlike rocBLAS GSU."""
    g = torch.Generator(device="cuda").manual_seed(3)
    a = torch.randn(120_000, 256, device="cuda", generator=g)
    b = torch.randn(120_000, 100, device="cuda", generator=g)
    c0, bias0 = _ext.wgrad(a, b, True)
    for _ in range(3):
        c, bias = _ext.wgrad(a, b, True)
        assert torch.equal(c, c0)
        assert torch.equal(bias, bias0)


# ---------------------------------------------------------------------------
# integer-valued operands: exact equality with float64
# ---------------------------------------------------------------------------
def _int_operands(k, m, n, bound=8, seed=0, device=DEV):
    g = _gen(seed, device)
    return (gc.rand_ints((k, m), bound, g, device),
            gc.rand_ints((k, n), bound, g, device))


@pytest.mark.parametrize("bias", [False, True], ids=["nobias", "bias"])
@pytest.mark.parametrize("k,m,n", gc.WGRAD_SMALL + [gc.WGRAD_FRONTIER])
def test_wgrad_integer_exact(k, m, n, bias):
    # |C| <= 64*K and |bias| <= 8*K are exact integers in fp32, and so is
    # every partial sum of any split
    assert 64 * k < gc.EXACT_LIMIT
    a, b = _int_operands(k, m, n)
    c, bg = _ext.wgrad(a, b, bias)
    assert c.shape == (m, n)
    assert torch.equal(c.double(), a.double().t() @ b.double())
    if bias:
        assert bg.shape == (m,)
        assert torch.equal(bg.double(), a.double().sum(0))
    else:
        assert bg is None


# ---------------------------------------------------------------------------
# random floats at small K: the elementwise bound of K fp32 operations
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("k,m,n", gc.WGRAD_SMALL)
def test_wgrad_random_within_bound(k, m, n):
    g = _gen(5)
    a = torch.randn(k, m, device=DEV, generator=g)
    b = torch.randn(k, n, device=DEV, generator=g)
    c, bg = _ext.wgrad(a, b, True)
    a64, b64 = a.double(), b.double()
    err_c = (c.double() - a64.t() @ b64).abs()
    bound_c = k * gc.U * (a64.abs().t() @ b64.abs())
    err_b = (bg.double() - a64.sum(0)).abs()
    bound_b = k * gc.U * a64.abs().sum(0)
    print(f"wgrad {k}x{m}x{n}: max err/bound C = "
          f"{float((err_c / bound_c.clamp_min(1e-300)).max()):.3g}, bias = "
          f"{float((err_b / bound_b.clamp_min(1e-300)).max()):.3g}")
    assert bool((err_c <= bound_c).all())
    assert bool((err_b <= bound_b).all())


def test_wgrad_nan_stays_in_its_row():
    k, m, n = 1000, 100, 47
    row = 70  # in the second m-tile
    g = _gen(6)
    a = torch.randn(k, m, device=DEV, generator=g)
    b = torch.randn(k, n, device=DEV, generator=g)
    clean_c, clean_b = _ext.wgrad(a, b, True)
    a_nan = a.clone()
    a_nan[500, row] = float("nan")
    c, bg = _ext.wgrad(a_nan, b, True)
    assert bool(c[row].isnan().all()) and bool(bg[row].isnan())
    keep = torch.arange(m, device=DEV) != row
    assert not bool(clean_c.isnan().any() | clean_b.isnan().any())
    assert _same_bits(c[keep], clean_c[keep])
    assert _same_bits(bg[keep], clean_b[keep])


# ---------------------------------------------------------------------------
# QLinear autograd with an O(1) upstream gradient
# ---------------------------------------------------------------------------
_QL_M = _WGRAD_MIN_K + 100


def _rel(got, want):
    return float((got.double() - want).norm() / want.norm().clamp_min(1e-30))


@pytest.mark.parametrize("bias", [False, True], ids=["nobias", "bias"])
@pytest.mark.parametrize("fin,fout", [(100, 256), (256, 47), (128, 128)])
def test_qlinear_autograd_matches_fp64(fin, fout, bias):
    """Data-grad through tall_gemm (100), through rocBLAS (256) and at the
    routing boundary (128), with gradients large enough that zeros fail."""
    torch.manual_seed(0)
    g = _gen(7)
    ql = QLinear(fin, fout, bias=bias).cuda()
    x = torch.randn(_QL_M, fin, device=DEV, generator=g, requires_grad=True)
    up = torch.randn(_QL_M, fout, device=DEV, generator=g)
    ql(x).backward(up)

    x64 = x.detach().double().requires_grad_(True)
    w64 = ql.weight.detach().double().requires_grad_(True)
    b64 = ql.bias.detach().double().requires_grad_(True) if bias else None
    F.linear(x64, w64, b64).backward(up.double())

    # x.grad = up @ W: fout fused multiply-adds per element
    err = (x.grad.double() - x64.grad).abs()
    bound = gc.gemm_bound(up, ql.weight.detach(), None, fout)
    print(f"qlinear {fin}->{fout}: x.grad max err/bound = "
          f"{float((err / bound.clamp_min(1e-300)).max()):.3g}, "
          f"|x.grad| max = {float(x64.grad.abs().max()):.3g}")
    assert bool((err <= bound).all())
    # the weight-grad kernel's own criterion (test_wgrad_matches_torch)
    assert _rel(ql.weight.grad, w64.grad) < 1e-5
    if bias:
        assert _rel(ql.bias.grad, b64.grad) < 1e-4
    else:
        assert ql.bias is None


def test_qlinear_autograd_integer_exact():
    """Integers in [-4, 4] everywhere: the largest possible sum is
    16 * 16484 < 2^24, so all three gradients equal float64."""
    fin, fout = 100, 256
    assert 16 * _QL_M < gc.EXACT_LIMIT
    g = _gen(8)
    ql = QLinear(fin, fout).cuda()
    with torch.no_grad():
        ql.weight.copy_(gc.rand_ints((fout, fin), 4, g, DEV))
        ql.bias.copy_(gc.rand_ints((fout,), 4, g, DEV))
    x = gc.rand_ints((_QL_M, fin), 4, g, DEV).requires_grad_(True)
    up = gc.rand_ints((_QL_M, fout), 4, g, DEV)
    ql(x).backward(up)
    up64 = up.double()
    assert torch.equal(x.grad.double(), up64 @ ql.weight.detach().double())
    assert torch.equal(ql.weight.grad.double(),
                       up64.t() @ x.detach().double())
    assert torch.equal(ql.bias.grad.double(), up64.sum(0))


# ---------------------------------------------------------------------------
# routing: which calls reach the two kernels
# ---------------------------------------------------------------------------
@pytest.fixture
def calls(monkeypatch):
    """Counting pass-throughs around the two native entry points."""
    count = {"tall_gemm": 0, "wgrad": 0}

    def counted(name):
        real = getattr(qnn._ext, name)

        def wrapper(*args):
            count[name] += 1
            return real(*args)
        return wrapper

    for name in count:
        monkeypatch.setattr(qnn._ext, name, counted(name), raising=False)
    return count


def _step(fin, rows=_QL_M, x_grad=True, dtype=torch.float32, lead=()):
    ql = QLinear(fin, 64).cuda().to(dtype)
    x = torch.randn(*lead, rows, fin, device=DEV, dtype=dtype,
                    requires_grad=x_grad)
    out = ql(x)
    out.backward(torch.ones_like(out))
    return ql


@pytest.mark.parametrize("fin,n_tall", [(100, 1), (128, 1), (129, 0),
                                        (256, 0)])
def test_routing_by_in_features(calls, fin, n_tall):
    _step(fin)
    assert calls == {"tall_gemm": n_tall, "wgrad": 1}
    _step(fin)  # once per backward, every backward
    assert calls == {"tall_gemm": 2 * n_tall, "wgrad": 2}


def test_routing_input_without_grad(calls):
    ql = _step(100, x_grad=False)
    assert calls == {"tall_gemm": 0, "wgrad": 1}
    assert ql.weight.grad is not None


def test_routing_plain_linear_cases(calls):
    _step(100, rows=_WGRAD_MIN_K - 1)            # too few rows
    _step(100, lead=(2,))                        # 3-D input
    _step(100, dtype=torch.float64)              # not fp32
    with torch.no_grad():
        QLinear(100, 64).cuda()(torch.randn(_QL_M, 100, device=DEV))
    assert calls == {"tall_gemm": 0, "wgrad": 0}


# ---------------------------------------------------------------------------
# the binding
# ---------------------------------------------------------------------------
_BREAK = {
    "row_mismatch": lambda d: d.update(b=d["b"][:-1]),
    "b_on_cpu": lambda d: d.update(b=d["b"].cpu()),
    "a_on_cpu": lambda d: d.update(a=d["a"].cpu()),
    "a_fp64": lambda d: d.update(a=d["a"].double()),
    "b_fp64": lambda d: d.update(b=d["b"].double()),
    "a_1d": lambda d: d.update(a=d["a"].reshape(-1)),
    "b_3d": lambda d: d.update(b=d["b"].unsqueeze(0)),
}


@pytest.mark.parametrize("fault", sorted(_BREAK))
def test_wgrad_bad_arguments_raise(fault):
    a, b = _int_operands(40, 7, 9)
    args = {"a": a, "b": b}
    c, bg = _ext.wgrad(args["a"], args["b"], True)  # well-formed: goes through
    assert torch.equal(c.double(), a.double().t() @ b.double())
    _BREAK[fault](args)
    with pytest.raises(RuntimeError):
        _ext.wgrad(args["a"], args["b"], True)


def test_wgrad_empty_dimensions():
    a, b = _int_operands(0, 7, 9)
    c, bg = _ext.wgrad(a, b, True)        # K == 0: empty sums
    assert torch.equal(c, torch.zeros(7, 9, device=DEV))
    assert torch.equal(bg, torch.zeros(7, device=DEV))
    c, bg = _ext.wgrad(a, b, False)
    assert torch.equal(c, torch.zeros(7, 9, device=DEV)) and bg is None

    a, b = _int_operands(40, 0, 9)
    c, bg = _ext.wgrad(a, b, True)        # M == 0
    assert c.shape == (0, 9) and bg.shape == (0,)

    a, b = _int_operands(40, 7, 0)
    c, bg = _ext.wgrad(a, b, True)        # N == 0: C is empty, bias is not
    assert c.shape == (7, 0)
    assert torch.equal(bg.double(), a.double().sum(0))


@pytest.mark.skipif(torch.cuda.device_count() < 2, reason="needs two GPUs")
def test_wgrad_on_a_device_that_is_not_current():
    torch.cuda.set_device(0)
    a, b = _int_operands(4099, 100, 47, device="cuda:1")
    c, bg = _ext.wgrad(a, b, True)
    assert torch.cuda.current_device() == 0
    assert c.device == a.device and bg.device == a.device
    assert torch.equal(c.double(), a.double().t() @ b.double())
    assert torch.equal(bg.double(), a.double().sum(0))
