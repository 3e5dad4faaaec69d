"""What the GPU GEMM tests take for granted, checked without a GPU: the
case lists cover what they claim, the integer cases stay exact in fp32, and
the random-float bound holds for a known-good fp32 matmul while a single
dropped term breaks it."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _gemm_cases as gc  # noqa: E402  (shared case lists, same folder)


def _partners(cases, axis, value):
    """Distinct values on the other two axes that `value` appears with."""
    others = [i for i in range(3) if i != axis]
    rows = [c for c in cases if c[axis] == value]
    return [len({c[o] for c in rows}) for o in others]


def test_small_gemm_cases_cover_the_lists():
    for axis, values in enumerate((gc.GEMM_MS, gc.GEMM_KS, gc.GEMM_NS)):
        assert {c[axis] for c in gc.GEMM_SMALL} == set(values)
        for v in values:
            assert min(_partners(gc.GEMM_SMALL, axis, v)) >= 2, (axis, v)
    assert (65, 47, 47) in gc.GEMM_SMALL
    assert (200, 256, 100) in gc.GEMM_SMALL
    ks = {k for _, k, _ in gc.GEMM_SMALL}
    ns = {n for _, _, n in gc.GEMM_SMALL}
    assert any(k < gc.BK for k in ks) and gc.BK in ks
    assert any(k > gc.BK and k % gc.BK for k in ks)    # ragged last stage
    assert any(k % 4 for k in ks) and any(n % 4 for n in ns)  # scalar paths
    assert {gc.n_tiles(n) for n in ns} == {1, 2, 3}
    assert any(n % gc.BN for n in ns if n > gc.BN)     # partial last n-tile


def test_walk_cases_walk_and_small_ones_do_not():
    """launch_tall_gemm gives a block a second m-tile only above
    m_stride_max(N) rows; the walk cases are past it, end on a ragged tile,
    and for N=512 some block takes three tiles."""
    assert gc.m_stride_max(512) == 32768 and gc.m_stride_max(100) == 131072
    for m, k, n in gc.GEMM_WALK:
        assert m > gc.m_stride_max(n) and gc.tiles_walked(m, n) >= 2
        assert m % gc.BM != 0
    assert {gc.tiles_walked(m, n) for m, _, n in gc.GEMM_WALK
            if n == 512} == {3}
    assert {k for _, k, n in gc.GEMM_WALK if n == 512} == {8, 40, 64}
    assert (131072 + 64 + 37, 72, 100) in gc.GEMM_WALK
    assert all(gc.tiles_walked(m, n) == 1 for m, _, n in gc.GEMM_SMALL)


def test_wgrad_cases_cover_the_lists():
    assert {k for k, _, _ in gc.WGRAD_SMALL} == set(gc.WGRAD_KS)
    assert {(m, n) for _, m, n in gc.WGRAD_SMALL} == set(gc.WGRAD_MNS)
    assert gc.WGRAD_FRONTIER == (200_001, 100, 256)


def test_integer_cases_stay_exact_in_fp32():
    for m, k, n in gc.GEMM_SMALL + gc.GEMM_WALK:
        assert 64 * k + 8 < gc.EXACT_LIMIT
    for k, m, n in gc.WGRAD_SMALL + [gc.WGRAD_FRONTIER]:
        assert 64 * k < gc.EXACT_LIMIT
    # the worst case itself: all operands at the bound
    k = max(k for _, k, _ in gc.GEMM_SMALL)
    a = torch.full((3, k), 8.0)
    b = torch.full((k, 2), -8.0)
    assert torch.equal((a @ b).double(), a.double() @ b.double())


@pytest.mark.parametrize("k", [1, 4, 33, 47, 100, 256, 1000])
def test_fp32_matmul_is_within_the_bound_and_a_dropped_term_is_not(k):
    g = torch.Generator().manual_seed(k)
    a = torch.randn(70, k, generator=g)
    b = torch.randn(k, 50, generator=g)
    bias = torch.randn(50, generator=g)
    ref = a.double() @ b.double() + bias.double()
    bound = gc.gemm_bound(a, b, bias, k)
    assert bool((((a @ b + bias).double() - ref).abs() <= bound).all())
    # the same product without its last k term: the bound is tight enough
    # to notice that in most elements (only a term that happens to be tiny
    # can hide), so it is no rubber stamp
    dropped = (a[:, :-1] @ b[:-1] + bias).double()
    outside = ((dropped - ref).abs() > bound).double().mean()
    assert float(outside) > 0.5
