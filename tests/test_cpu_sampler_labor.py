"""GraphSageSampler.sample_labor on the CPU engine: the cases of
_sampler_labor.py against its model, exactly."""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _sampler_labor as sl  # noqa: E402  (shared with the GPU file)


@pytest.mark.parametrize("case", sl.CASES, ids=sl.case_id)
def test_labor(case):
    check, args = case
    check("CPU", *args)


def test_keep_rate_and_reproducibility():
    sl.rate_batches("CPU")
