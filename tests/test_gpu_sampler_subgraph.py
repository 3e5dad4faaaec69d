"""GraphSageSampler.subgraph and sample_saint_rw on the GPU: the chunk
kernels of subgraph_kernels.hip against the model of _sampler_subgraph.py,
exactly.  Shapes are the smallest that reach every branch: rows of degree
0, 1, 15..17, 63..65 and one below, at and above one and two chunks, a hub
of twenty chunks, members on both sides of every chunk boundary and of a
bitmap word's edge, sets of 1, 17 and 300 nodes, and one set with more
chunks than the capped grid has subgroups.  UVA mode repeats the cases
that read rows through the spare-address loads."""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _sampler_subgraph as ss  # noqa: E402  (shared with the CPU file)

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("case", ss.CASES, ids=ss.case_id)
def test_subgraph_gpu(case):
    check, args, _ = case
    check("GPU", *args)


@pytest.mark.parametrize("case", [c for c in ss.CASES if c[2]],
                         ids=ss.case_id)
def test_subgraph_uva(case):
    check, args, _ = case
    check("UVA", *args)


@pytest.mark.parametrize("bad", (0, 1))
def test_bad_id_on_gpu(bad):
    """The bad-id count comes back with the sizes, in the call's one sync."""
    ss.check_bad_id("GPU", bad, device="cuda")
