"""GpuSampler.reindex_single against the exact model of _frontier_model.py:
torch.equal on frontier, row and col, at sizes chosen against the caps of
csrc/reindex_kernels.hip (a grid is at most 2048 blocks: 524 288 items for
the 256-wide kernels, 32 768 rows for expand_rows_kernel).  Every case also
goes through the CPU engine, so both engines are pinned to one model."""
import os
import sys

import pytest
import torch

import quiver

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _frontier_model as fm  # noqa: E402  (shared with the CPU file)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def engines():
    """reindex_single reads nothing of the graph: any topo will do."""
    topo = quiver.CSRTopo(indptr=torch.tensor([0, 1, 2]),
                          indices=torch.tensor([1, 0]))
    gpu = quiver.GraphSageSampler(topo, [2], device=0, mode="GPU")
    cpu = quiver.GraphSageSampler(topo, [2], mode="CPU")
    gpu.lazy_init_quiver()
    cpu.lazy_init_quiver()
    return gpu, cpu


def _check(engines, seeds, nbrs, counts):
    gpu, cpu = engines
    want = fm.reindex_model(seeds, nbrs, counts)
    got = gpu.reindex(seeds.cuda(), nbrs.cuda(), counts.cuda())
    torch.cuda.synchronize()
    for g, w in zip(got, want):
        assert g.is_cuda and g.dtype == torch.int64
        assert torch.equal(g.cpu(), w)
    for g, w in zip(cpu.reindex(seeds, nbrs, counts), want):
        assert torch.equal(g, w)
    return want


def test_strided(engines):
    """40 000 unique seeds and 560 000 neighbours: insert, mark_first,
    compact, lookup and expand_rows all take a second grid-stride
    iteration."""
    seeds, nbrs, counts = fm.case_strided()
    assert seeds.numel() > 2048 * 16 and nbrs.numel() > 2048 * 256
    frontier, _, _ = _check(engines, seeds, nbrs, counts)
    assert torch.equal(frontier[:seeds.numel()], seeds)


@pytest.mark.parametrize("key_is_seed", [False, True])
def test_one_hot_key(engines, key_is_seed):
    """100 000 copies of one id: the first occurrence must win the
    atomicMin on the one slot they all hit."""
    frontier, _, col = _check(
        engines, *fm.case_one_hot(key_is_seed=key_is_seed))
    assert frontier.numel() == (1 if key_is_seed else 2)
    assert col.unique().tolist() == [frontier.numel() - 1]


def test_wide_keys(engines):
    """Keys up to just below 2^62, some apart only above bit 31."""
    seeds, nbrs, counts = fm.case_wide_keys()
    frontier, _, col = _check(engines, seeds, nbrs, counts)
    assert torch.equal(frontier[col], nbrs)
    assert frontier.numel() == 7 * seeds.numel()


def test_duplicate_seeds(engines):
    """With repeated seeds the frontier is shorter than the seed list,
    while row still indexes seed POSITIONS; both engines must agree with
    the model on that."""
    seeds, nbrs, counts = fm.case_duplicate_seeds()
    frontier, row, _ = _check(engines, seeds, nbrs, counts)
    assert frontier.numel() < seeds.numel()
    assert int(row.max()) > frontier.numel()


@pytest.mark.parametrize("n", [50, 0])
def test_zero_rows(engines, n):
    """A batch of isolated nodes, and an empty batch."""
    frontier, row, col = _check(engines, *fm.case_zero_rows(n))
    assert frontier.numel() == n and row.numel() == 0 and col.numel() == 0


def test_around_a_power_of_two(engines):
    """2 * (n + m) + 64 just under, at and just over 4096: the capacity
    and mask that next_pow2 gives."""
    for seeds, nbrs, counts in fm.cases_around_pow2():
        _check(engines, seeds, nbrs, counts)
