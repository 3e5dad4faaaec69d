"""GraphSageSampler.subgraph and sample_saint_rw on the CPU engine: the
cases of _sampler_subgraph.py against its model, exactly."""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _sampler_subgraph as ss  # noqa: E402  (shared with the GPU file)


@pytest.mark.parametrize("case", ss.CASES, ids=ss.case_id)
def test_subgraph(case):
    check, args, _ = case
    check("CPU", *args)
