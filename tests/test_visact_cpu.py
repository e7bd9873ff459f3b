"""CPU tier of the visual-activity entry: the model (tests/visact_ref.py) against the reference's own results recorded in tests/golden/visact.npz (tests/visact_golden_gen.*
called calcSpatialVisAct, calcTemporalVisAct, updateVisAct, filterAndCalculateAverageActivity, getAvg and the six g_pelBufOP entries themselves; the scalar row is recorded),
on the pictures and area lists of tests/visact_cases.py."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import visact_cases as VC  # noqa: E402
import visact_ref as VR  # noqa: E402


@pytest.fixture(scope="module")
def golden():
    return np.load(VR.GOLDEN)


@pytest.fixture(scope="module")
def modelled():
    """name -> ( records, double bit patterns, integers, means ) of the model, computed once"""
    return {n: VC.expected(c) for n, c in VC.cases().items()}


def test_the_case_builder_gives_the_recorded_inputs(golden):
    pics, cases = VC.pictures(), VC.cases()
    assert list(golden["pictures"]) == list(pics) and list(golden["cases"]) == list(cases)
    for name, p in pics.items():
        hdr = list(golden[name + "_hdr"])
        assert hdr[:2] == [p.bit_depth, len(p.rows)], name
        for r, (cur, p1, p2) in enumerate(p.rows):
            assert hdr[2 + r] == (1 if p1 is not None else 0) | (2 if p2 is not None else 0) | (4 if p.same(r) else 0), (name, r)
            assert np.array_equal(golden["%s_c%d" % (name, r)], cur), (name, r)
            if not p.same(r):
                assert np.array_equal(cur + golden["%s_d1%d" % (name, r)], p1), (name, r)
            assert np.array_equal(p1 + golden["%s_d2%d" % (name, r)], p2), (name, r)
            assert cur.min() >= 0 and max(cur.max(), p1.max(), p2.max()) < 1 << p.bit_depth
    for name, c in cases.items():
        assert list(golden["pictures"])[int(golden[name + "_pic"])] == c.picture.name, name
        assert golden[name + "_areas"].tobytes() == np.ascontiguousarray(c.areas).tobytes(), name
    # what the cases are there for
    assert {8, 10, 12} == {p.bit_depth for p in pics.values()}
    p72 = cases["p72_10_hd1"].areas
    assert len(p72) == 6 + 3 and (int(p72[0]["x"]), int(p72[0]["w"]), int(p72[0]["y"]), int(p72[0]["h"])) == (0, 33, 0, 33)      # no guard in the first row and column
    assert (int(p72[5]["x"]), int(p72[5]["w"]), int(p72[5]["mw"]), int(p72[5]["y"]), int(p72[5]["h"]), int(p72[5]["mh"])) == (63, 9, 8, 31, 9, 8)
    big = cases["p264_10_ds2"].areas
    assert (int(big[5]["x"]), int(big[5]["w"]), int(big[5]["mw"]), int(big[5]["y"]), int(big[5]["h"]), int(big[5]["mh"])) == (254, 10, 8, 126, 10, 8) and int(big[4]["w"]) == 132
    assert [int(a["ds"]) for a in cases["p72_10_ds1"].areas[-3:]] == [1, 0, 0] and [int(a["ds"]) for a in cases["p72x_10_ds1"].areas[-3:]] == [1, 1, 1]
    mix = cases["mix10"].areas
    assert any(a["ds"] and a["x"] & 1 for a in mix) and any(a["ds"] and a["y"] & 1 for a in mix) and any(VC.pictures()["mix10"].same(int(a["plane"])) for a in mix)
    pos = [((int(a["w"]) - 4) // 2, (int(a["h"]) - 4) // 2) if a["ds"] else (int(a["w"]) - 2, int(a["h"]) - 2) for a in mix]
    assert any(w % VR.TILE_W and h % VR.TILE_H and w % 64 and w > VR.TILE_W and h > VR.TILE_H for w, h in pos), "no area crosses the tile in both directions with a remainder"
    assert not np.array_equal(mix, np.sort(mix, order=["plane", "y", "x"])), "the list is not shuffled"


def test_model_equals_the_fixture(golden, modelled):
    seen = set()
    for name, c in VC.cases().items():
        rec, hp, ints, avg = modelled[name]
        assert np.array_equal(rec, golden[name + "_rec"]), (name, "sums", np.argwhere(rec != golden[name + "_rec"])[:4].tolist())
        assert np.array_equal(hp, golden[name + "_hp"]), (name, "double bit patterns", np.argwhere(hp != golden[name + "_hp"])[:4].tolist())
        assert np.array_equal(ints, golden[name + "_int"]), (name, "spatAct, tempAct, minAct, visAct")
        assert np.array_equal(avg, golden[name + "_avg"]), (name, "getAvg")
        seen |= {(int(a["ds"]), int(a["order"])) for a, r in zip(c.areas, rec) if r[0] > 0 and (a["order"] == 0 or r[1] > 0)}
    assert seen == {(f, o) for f in (0, 1) for o in (0, 1, 2)}, "a form x order without a non-zero sum"


def test_the_extreme_planes_pass_32_bits(golden):
    """in the model's Python integers, on a plane no larger than 1024 x 1024"""
    c = VC.cases()["ext12"]
    assert all(r[0].shape[0] <= 1024 and r[0].shape[1] <= 1024 for r in c.picture.rows)
    recs = [VR.record(c.picture.rows, a) for a in c.areas]
    assert max(r[0] for r in recs) > 1 << 32 and max(r[1] for r in recs) > 1 << 32
    for f in (0, 1):
        assert any(r[0] > 1 << 32 and r[1] > 1 << 32 for a, r in zip(c.areas, recs) if a["ds"] == f and a["order"] == 2), ("form", f)
    assert golden["ext12_rec"][:, :2].max() > 1 << 32


def test_the_tiles_of_an_area_add_up_to_the_area(modelled):
    for name in ("p264_10_hd2", "p264_10_ds1", "mix10", "one10", "ext8"):
        c = VC.cases()[name]
        for a, want in zip(c.areas, modelled[name][0]):
            parts = VR.tiles(a)
            assert len(parts) == -(-((int(a["w"]) - 4) // 2 if a["ds"] else int(a["w"]) - 2) // VR.TILE_W) * -(-((int(a["h"]) - 4) // 2 if a["ds"] else int(a["h"]) - 2) // VR.TILE_H)
            tot = [0, 0, 0]
            for (x, y, w, h) in parts:
                t = VR.area(int(a["plane"]), int(a["ds"]), int(a["order"]), x, y, w, h)
                r = VR.record(c.picture.rows, t)
                tot = [tot[0] + r[0], tot[1] + r[1], tot[2] + r[3]]
            assert tot == [int(want[0]), int(want[1]), int(want[3])], (name, a)


def test_the_bypass_and_the_frame_rate_factor():
    """the double expressions as the reference writes them: 1.15625 only for the first order, hpTempAct = 0 where prev1 is cur"""
    va = VR.vis_act([1000, 300, 0, 100], 12, 12, 10, 0, 1)
    assert va.hpTempAct == 3.0 and va.tempAct == int(0.5 + 3.0 * 4.0 * 1.15625)
    assert VR.vis_act([1000, 300, 0, 100], 12, 12, 10, 0, 2).tempAct == int(0.5 + 3.0 * 4.0)
    same = VR.vis_act([1000, 300, 0, 100], 12, 12, 10, 0, 1, same=True)
    assert same.hpTempAct == 0.0 and same.tempAct == 0 and same.minAct == 0 and same.hpVisAct == max(16.0, 10.0)
    assert VR.vis_act([1000, 300, 0, 100], 12, 12, 10, 0, 2, same=True).hpTempAct == 3.0      # (the bypass is the first order's alone)
