"""GraphSageSampler.random_walk on the CPU engine, which draws every step
from its exact distribution: the cases of _sampler_walks.py."""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _sampler_walks as sw  # noqa: E402  (shared with the GPU file)


@pytest.mark.parametrize("case", sw.CASES, ids=sw.case_id)
def test_walk(case):
    check, args, _ = case
    check("CPU", *args)
