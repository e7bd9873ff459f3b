"""CPU tier of the deblocking filter: the model (tests/deblock_ref.py) against the reference's own results recorded in tests/golden/deblock.npz
(tests/deblock_golden_gen.* called LoopFilter::xDeblockArea<EDGE_VER> / <EDGE_HOR> themselves, scalar and x86 row), on the pictures and maps of tests/deblock_cases.py."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import deblock_cases as DC  # noqa: E402
import deblock_ref as DR  # noqa: E402


@pytest.fixture(scope="module")
def golden():
    return np.load(DR.GOLDEN)


@pytest.fixture(scope="module")
def modelled():
    """name -> ( planes after VER, planes after VER + HOR ), and the branch counters of all cases together"""
    cnt, out = DR.Counter(), {}
    for name, c in DC.cases().items():
        ver = DR.deblock(c.planes, c.lfp_ver, c.lfp_hor, c.ctu, c.bit_depth, c.clip, c.beta_offsets, c.tc_offsets, dirs=DR.VER)
        out[name] = (ver, DR.deblock(c.planes, c.lfp_ver, c.lfp_hor, c.ctu, c.bit_depth, c.clip, c.beta_offsets, c.tc_offsets, counters=cnt))
    return out, cnt


def test_the_case_builder_gives_the_recorded_inputs(golden):
    assert list(golden["names"]) == list(DC.cases())
    for name, c in DC.cases().items():
        assert list(golden[name + "_hdr"]) == [c.width, c.height, c.ctu, c.bit_depth, len(c.planes), c.clip[0][1], *c.beta_offsets, *c.tc_offsets], name
        assert golden[name + "_ver"].tobytes() == np.ascontiguousarray(c.lfp_ver).tobytes() and golden[name + "_hor"].tobytes() == np.ascontiguousarray(c.lfp_hor).tobytes(), name
        assert all(np.array_equal(golden["%s_p%d" % (name, k)], p) for k, p in enumerate(c.planes)), name
    geo = {(c.width, c.height, c.ctu, c.bit_depth) for c in DC.cases().values()}
    assert {(72, 40, 32, 10), (136, 72, 64, 8), (264, 136, 128, 12)} <= geo and any(len(c.planes) == 1 for c in DC.cases().values())


def test_model_equals_the_fixture_and_every_branch_is_taken(golden, modelled):
    out, cnt = modelled
    for name, c in DC.cases().items():
        for k, p in enumerate(c.planes):
            assert np.array_equal(out[name][0][k], p + golden["%s_v%d" % (name, k)]), (name, k, "after VER")
            assert np.array_equal(out[name][1][k], p + golden["%s_d%d" % (name, k)]), (name, k, "after VER + HOR")
            assert golden["%s_v%d" % (name, k)].any() and not np.array_equal(golden["%s_v%d" % (name, k)], golden["%s_d%d" % (name, k)]), (name, k, "a pass changes nothing")
    # only now do the model's counters say something about the fixture
    assert not DR.coverage(cnt), "branches the cases never take: %s" % DR.coverage(cnt)


def test_the_order_of_the_edges_of_a_direction_is_free(modelled):
    """the legality of the maps: no edge of a direction writes a sample another edge of that direction reads or writes"""
    for seed, (name, c) in enumerate(DC.cases().items()):
        got = DR.deblock(c.planes, c.lfp_ver, c.lfp_hor, c.ctu, c.bit_depth, c.clip, c.beta_offsets, c.tc_offsets, shuffle=np.random.default_rng(31 + seed))
        assert all(np.array_equal(g, w) for g, w in zip(got, modelled[0][name][1])), name


def test_bands_of_the_model_give_the_whole(modelled):
    for name in ("g136", "g64"):
        c = DC.cases()[name]
        planes = c.planes
        for r in range(c.ctu_rows):
            planes = DR.deblock(planes, c.lfp_ver, c.lfp_hor, c.ctu, c.bit_depth, c.clip, c.beta_offsets, c.tc_offsets, rows=(r, 1))
        assert all(np.array_equal(g, w) for g, w in zip(planes, modelled[0][name][1])), name
