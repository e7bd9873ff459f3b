"""CPU tier of the SAO entries: tests/sao_ref.py — the model the GPU tier is checked against — equals every statistics record and every filtered plane that
tests/golden/sao.npz holds from the reference's own getBlkStats / offsetBlock, tolerance 0; the case lists of tests/sao_cases.py are the fixture's; and the fixture is not
vacuous (the generator driver's own coverage assertions, repeated on the recorded results)."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import sao_cases as SC  # noqa: E402
import sao_golden_gen as GEN  # noqa: E402
import sao_ref as SR  # noqa: E402


@pytest.fixture(scope="module")
def golden():
    return np.load(SR.GOLDEN)


def test_cases_are_the_fixtures(golden):
    P = SC.pictures()
    assert list(golden["pic_names"]) == list(P)
    for name, pic in P.items():
        assert golden["pic_%s_hdr" % name].tolist() == [pic.width, pic.height, pic.ctu, pic.bit_depth]
        for c in range(3):
            assert np.array_equal(golden["pic_%s_org%d" % (name, c)], pic.org[c]) and np.array_equal(golden["pic_%s_src%d" % (name, c)], pic.src[c]), (name, c)
            assert pic.src[c].min() >= 0 and pic.src[c].max() < (1 << pic.bit_depth), "the operand contract: 0 <= src < 2^bitDepth"
    sc, oc = SC.stats_cases(), SC.offset_cases()
    assert list(golden["stats_names"]) == [n for n, _, _ in sc] and list(golden["offset_names"]) == [n for n, _, _, _ in oc]
    for k, (name, pic, flags) in enumerate(sc):
        assert bool(golden["s%03d_borders" % k]) == (flags is None)
        assert np.array_equal(golden["s%03d_flags" % k], SR.border_flags(*pic.grid) if flags is None else flags), name
    for k, (name, pic, prm, clip) in enumerate(oc):
        assert np.array_equal(golden["o%03d_prm" % k], prm) and golden["o%03d_clip" % k].tolist() == [list(c) for c in clip], name


def test_model_equals_recorded_statistics(golden):
    for k, (name, pic, flags) in enumerate(SC.stats_cases()):
        rec = golden["s%03d_rec" % k]
        assert rec.shape == (pic.n_ctus, 3, 5, 2, 32)
        for c in range(3):
            got = SR.stats_picture(pic.org[c], pic.src[c], pic.ctus[c][0], pic.ctus[c][1], pic.bit_depth, c == 0, flags)
            assert np.array_equal(got, rec[:, c]), (name, c)


def test_model_equals_recorded_planes(golden):
    for k, (name, pic, prm, clip) in enumerate(SC.offset_cases()):
        for c in range(3):
            got = SR.offset_picture(pic.src[c], prm[:, c], pic.ctus[c][0], pic.ctus[c][1], pic.bit_depth, clip[c])
            assert np.array_equal(got, pic.src[c] + golden["o%03d_delta%d" % (k, c)]), (name, c)


def test_band_rows_of_the_model_add_up(golden):
    pic = SC.pictures()["geo72"]
    whole = SR.stats_picture(pic.org[0], pic.src[0], 32, 32, 10, True)
    parts = SR.stats_picture(pic.org[0], pic.src[0], 32, 32, 10, True, rows=(0, 1)) + SR.stats_picture(pic.org[0], pic.src[0], 32, 32, 10, True, rows=(1, 1))
    assert np.array_equal(whole, parts)


def test_fixture_is_not_vacuous(golden):
    st = [(name, golden["s%03d_flags" % k], golden["s%03d_rec" % k]) for k, (name, _, _) in enumerate(SC.stats_cases())]
    of = [(name, pic, golden["o%03d_prm" % k], golden["o%03d_clip" % k].tolist(), [golden["o%03d_delta%d" % (k, c)] for c in range(3)]) for k, (name, pic, _, _) in enumerate(SC.offset_cases())]
    seen = GEN.coverage(st, of)
    assert seen["clipped_low"] > 0 and seen["clipped_high"] > 0 and seen["ctus_with_unfiltered_samples"] > 0
    # every flag bit occurs set and cleared; an off CTU lies between filtered ones; a plane is off with the others on
    flags = np.concatenate([f for _, f, _ in st])
    assert all((flags & f).any() and (~flags & f).any() for f in SR.STAT_FLAGS)
    mixed = dict((n, p) for n, _, p, _, _ in of)["geo72/mixed"]
    assert (mixed["type"][:, 0] < 0).any() and (mixed["type"][:, 0] >= 0).sum() >= 2
    off_plane = dict((n, p) for n, _, p, _, _ in of)["geo136/mixed"]
    assert (off_plane["type"][:, 1] < 0).all() and (off_plane["type"][:, 0] >= 0).any() and (off_plane["type"][:, 2] >= 0).any()
    assert os.path.getsize(SR.GOLDEN) <= max(os.path.getsize(os.path.join(HERE, "golden", f)) for f in os.listdir(os.path.join(HERE, "golden")) if f != "sao.npz")
