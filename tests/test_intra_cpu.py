"""CPU tier of the intra luma mode pre-selection: the numpy model (tests/intra_ref.py) against the reference's own results recorded in tests/golden/intra.npz, the coverage
the fixture must have, and the model's cost against the oracle's existing HAD_2SAD."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import intra_cases as IC  # noqa: E402
import intra_ref as IR  # noqa: E402


@pytest.fixture(scope="module")
def golden():
    return IC.load_golden()


@pytest.fixture(scope="module")
def model(golden):
    """the model on every golden case, once: { name: ( costs, predictions ) } and the branch counters"""
    cnt, out = {}, {}
    for name, (c, _, _) in golden.items():
        out[name] = IC.expected(c, cnt)
    return out, cnt


def test_fixture_is_the_case_list(golden):
    cases = IC.cases()
    assert list(golden) == list(cases)
    for name, c in cases.items():
        g = golden[name][0]
        assert (g.w, g.h, g.bit_depth, g.mri, g.modes, g.pred_modes) == (c.w, c.h, c.bit_depth, c.mri, c.modes, c.pred_modes), name
        assert np.array_equal(g.lines, c.lines) and np.array_equal(g.org, c.org), name


def test_model_equals_golden(golden, model):
    for name, (c, cost, pred) in golden.items():
        mc, mp = model[0][name]
        assert np.array_equal(mc, cost), (name, np.argwhere(mc != cost).reshape(-1).tolist())
        assert np.array_equal(mp, pred), name


def test_fixture_covers_every_branch(golden, model):
    cnt = model[1]
    missing = [k for k in IC.REQUIRED if not cnt.get(k)]
    assert not missing, missing
    shapes = {(c.w, c.h) for c, _, _ in golden.values()}
    assert shapes == set(IC.SHAPES)
    assert {c.bit_depth for c, _, _ in golden.values()} == {8, 10, 12} and {c.mri for c, _, _ in golden.values()} == {0, 1, 2}
    assert any(c.mri and c.w != c.h for c, _, _ in golden.values())
    assert os.path.getsize(IR.GOLDEN) < 400 * 1024


def test_parameters_at_known_points():
    # wide angles replace modes at the low end of wide blocks and at the high end of tall blocks (getWideAngle)
    assert IR.wide_angle(16, 4, 2) == 67 and IR.wide_angle(16, 4, 11) == 76 and IR.wide_angle(16, 4, 12) == 12
    assert IR.wide_angle(4, 64, 66) == 1 and IR.wide_angle(4, 64, 53) == -12 and IR.wide_angle(4, 64, 52) == 52
    # no reference filter for blocks of at most 32 samples; multi_ref_idx switches PDPC and both filter selections off
    assert all(not IR.params(8, 4, m, 0)["ref_filter"] and not IR.params(8, 4, m, 0)["interp"] for m in range(67))
    assert all(not IR.params(16, 16, m, 1)["pdpc"] and not IR.params(16, 16, m, 1)["ref_filter"] and not IR.params(16, 16, m, 1)["interp"] for m in range(1, 67))
    assert IR.params(16, 16, 34, 0)["ref_filter"] and IR.params(16, 16, 35, 0)["interp"] and not IR.params(16, 16, 50, 0)["ref_filter"]


def test_cost_equals_the_oracle(golden, model):
    from oracle.oracle import Oracle
    orc = Oracle()
    picked = 0
    for name, (c, cost, _) in golden.items():
        for m in c.modes[::7]:
            p = IR.predict(c.lines, c.w, c.h, m, c.mri, c.bit_depth)
            want = orc.dist("HAD_2SAD", np.ascontiguousarray(c.org), np.ascontiguousarray(p), c.w, c.h, c.bit_depth)
            assert int(cost[m]) == int(model[0][name][0][m]) == int(want), (name, m)
            picked += 1
    assert picked > 400
