"""GraphSageSampler.random_walk on the GPU: uniform_walk_kernel and
node2vec_walk_kernel, the cases of _sampler_walks.py.  Shapes are the
smallest that reach every branch: rows of degree 0, 1, 15, 16, 17, 64 and
65 (the exact/rejection boundary and the 64-wide scan group), a hub row
longer than 2048, the adjacent node at every boundary position of the
scanned row, and more walks than one block.  UVA mode repeats the cases
whose row reads go through the spare-address loads."""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _sampler_walks as sw  # noqa: E402  (shared with the CPU file)

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("case", sw.CASES, ids=sw.case_id)
def test_walk_gpu(case):
    check, args, _ = case
    check("GPU", *args)


@pytest.mark.parametrize("case", [c for c in sw.CASES if c[2]],
                         ids=sw.case_id)
def test_walk_uva(case):
    check, args, _ = case
    check("UVA", *args)
