"""GPU tier of the MMVD limits list (tests/mmvd_extremes.py): vvhip_merge_mmvd_costs_batch on two-level planes at 12 bits, with both BCW clip ends, base vectors at the ends
of the 18-bit range and the 128 x 128 CU nearest the 32-bit cost bound, against the model — tolerance 0, every requested candidate compared."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import mmvd_cases as MC  # noqa: E402
import mmvd_extremes as MX  # noqa: E402
from test_gpu_mmvd import hp, records, run  # noqa: E402,F401


def test_limits_list(hp, oracle):  # noqa: F811
    n = 0
    for group, cl in MC.groups(MX.cases()).items():
        got = run(hp, group, records(hp, group, cl, "two_level"), "two_level")
        want = MC.expected_group(oracle, group, cl)
        assert np.array_equal(got, want), (group, [c["name"] for c in cl], np.argwhere(got != want).tolist()[:8])
        n += int((want != MC.SENTINEL).sum())
    assert n > 300
