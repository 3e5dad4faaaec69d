"""GraphSageSampler.sample_labor on the GPU: the chunk kernels of
labor_kernels.hip against the model of _sampler_labor.py, exactly, in GPU
and in UVA mode.  One seed batch holds rows of degree 0, 1, one below, at
and above every fanout, a 16-lane step, a word of the hit mask, one and two
chunks, hubs of 1000 and 5000 slots and a seed given twice."""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _sampler_labor as sl  # noqa: E402  (shared with the CPU file)

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("mode", ["GPU", "UVA"])
@pytest.mark.parametrize("case", sl.CASES, ids=sl.case_id)
def test_labor(case, mode):
    check, args = case
    check(mode, *args)


@pytest.mark.parametrize("mask_fill", [0, 1])
@pytest.mark.parametrize("chunk", [64, 256, 1024])
@pytest.mark.parametrize("mode", ["GPU", "UVA"])
def test_every_built_variant(mode, chunk, mask_fill):
    """The fill pass that reads the hit mask and the one that hashes again,
    at every chunk size built, give the same hop, whichever the engine runs
    by default."""
    topo, seeds = sl.structure_graph(True)
    s = sl.make_sampler(topo, mode, [3], return_eid=True)
    hops = s.quiver.sample_labor_hops(
        sl.long(seeds).cuda(), [3], False, chunk, mask_fill)
    frontier, edges, dst_ptr = (x.cpu() for x in hops[0])
    want = sl.expected((3,), False, True, True)[0]
    got = (frontier, edges[:2], dst_ptr, edges[2])
    assert all(map(sl.torch.equal, got, want))


def test_keep_rate_and_reproducibility():
    a, b = sl.rate_batches("GPU"), sl.rate_batches("UVA")
    assert sl.same_batch(a, b)
