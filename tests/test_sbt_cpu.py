"""CPU tier of the SBT entries (vvhip_sbt_parts_batch / vvhip_sbt_tiles / vvhip_sbt_place_batch): the model of tests/sbt_ref.py against the reference's own results recorded in
tests/golden/sbt.npz, the library's host arithmetic (vvhip_sbt_tiles needs no device) and its Python mirror against the same fixture, what the fixture and the lists of
tests/sbt_cases.py cover, the records' layout against the header, and the model of the full chain through the oracle's TU pipeline.  No GPU."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import sbt_cases as SC  # noqa: E402
import sbt_ref as SR  # noqa: E402


@pytest.fixture(scope="module")
def gold():
    return SR.golden()


def test_sbt_symbols_prototypes_and_header():
    """fails on a library without the entries"""
    from vvenc_amd.lib import LIB_PATH, PROTOTYPES
    lib = C.CDLL(LIB_PATH)
    hdr = open(os.path.join(ROOT, "include", "vvenc_hip.h")).read()
    for name, nargs in (("vvhip_sbt_parts_batch", 8), ("vvhip_sbt_tiles", 3), ("vvhip_sbt_place_batch", 8)):
        assert getattr(lib, name) is not None and len(PROTOTYPES[name][1]) == nargs and name in hdr
    assert all(t in hdr for t in ("vvhip_sbt_item", "vvhip_sbt_tile", "vvhip_sbt_place_item"))


def test_sbt_record_layouts(tmp_path):
    """the three records as the C compiler lays them out == the numpy records the Python layer fills"""
    from vvenc_amd import hotpath as HP
    recs = (("vvhip_sbt_item", HP.SBT_ITEM_DTYPE, 28), ("vvhip_sbt_tile", HP.SBT_TILE_DTYPE, 20), ("vvhip_sbt_place_item", HP.SBT_PLACE_DTYPE, 52))
    body = "".join('printf("%%zu ", sizeof(%s));\n' % n + "".join('printf("%%zu ", offsetof(%s, %s));\n' % (n, f) for f in dt.names) for n, dt, _ in recs)
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "vvenc_hip.h"\nint main(void){\n' + body + "return 0; }\n")
    exe = tmp_path / "layout"
    subprocess.check_call(["g++", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    for n, dt, size in recs:
        want = [dt.itemsize] + [dt.fields[f][1] for f in dt.names]
        assert got[:len(want)] == want and dt.itemsize == size, n
        got = got[len(want):]
    assert HP.SBT_ITEM_DTYPE == SR.SBT_ITEM_DTYPE and HP.SBT_PLACE_DTYPE == SR.SBT_PLACE_DTYPE
    assert (HP.DCT2, HP.DCT8, HP.DST7) == (SR.DCT2, SR.DCT8, SR.DST7) and HP.SBT_MAX_DIST == SR.MAX_DISTORTION
    assert all(HP.sbt_allowed_of(w, h) == SR.allowed_of(w, h) for (w, h) in SR.ALL_SIZES)


def test_golden_covers_what_it_must(gold):
    """arrays only and below the largest fixture; the named sizes; every subset of sbt_allowed of the small sizes; the contents; the weights; every mode first of its kind;
    ties; a quad below the other direction's halves; truncation pinned; fast algorithm 1 both ways"""
    z = np.load(SR.GOLDEN)
    assert all(z[k].dtype.kind in "iuf" for k in z.files) and os.path.getsize(SR.GOLDEN) < 500 * 1024
    cus = gold["cus"]
    assert {(c["w"], c["h"]) for c in cus if c["kind"] == 0} == set(SR.SIZES)
    for (w, h) in ((8, 4), (4, 8), (8, 8), (16, 8), (8, 16), (16, 16)):
        assert {c["allowed"] for c in cus if (c["w"], c["h"]) == (w, h)} >= set(SR.subsets_of(SR.allowed_of(w, h)))
    for c in cus:
        assert c["y"].shape == (c["h"], c["w"]) and c["cb"].shape == c["cr"].shape == (c["h"] // 2, c["w"] // 2) and c["y"].dtype == np.int16
        assert c["allowed"] and not c["allowed"] & ~SR.allowed_of(c["w"], c["h"])
    content = [c for c in cus if c["kind"] == 2]
    assert any(not c["y"].any() and not c["cb"].any() for c in content)
    for v in (1023, -1023, 255, -255, 32767, -32768):
        assert any((c["y"] == v).all() and (c["cr"] == v).all() for c in content), v
    assert any(np.array_equal(c["y"], c["y"][:, ::-1]) and c["y"].any() for c in content) and any(np.array_equal(c["y"], c["y"][::-1, :]) and c["y"].any() for c in content)
    weights = {c["cw"] for c in cus}
    assert 1.0 in weights and len([w for w in weights if w != 1.0 and np.log2(w) % 1.0 != 0.0]) >= 3 and weights == set(SC.WEIGHTS)
    first, ties, quad_low, trunc, cross = set(), 0, 0, 0, 0
    for c in cus:
        n_half = min(2 * (((c["allowed"] >> 1) & 1) + ((c["allowed"] >> 2) & 1)), 2)
        first |= {c["order"][0], c["order"][n_half]}
        live = [v for v in c["est"][:8] if v != SR.MAX_DISTORTION]
        ties += len(set(live)) < len(live)
        e = c["est"]
        quad_low += any(e[q] < min(e[a], e[b]) for q, a, b in ((4, 2, 3), (5, 2, 3), (6, 0, 1), (7, 0, 1)) if SR.MAX_DISTORTION not in (e[q], e[a], e[b]))
        prods = [float(v) * c["cw"] for v in c["parts"][1] + c["parts"][2] if v]
        trunc += any(p % 1.0 != 0.0 for p in prods)
        cross += any(p % 1.0 > 0.5 for p in prods)      # rounding to nearest would cross to the next integer
        if c["cw"] != 1.0 and any(c["parts"][1]):
            assert e[8] != sum(sum(row) for row in c["parts"])
    assert first >= set(range(8)) and ties and quad_low and trunc and cross
    assert {c["skip"] for c in cus} == {False, True}
    assert {(w, h) for (w, h, _, _, _) in gold["tilings"]} == set(SR.ALL_SIZES) and len(gold["tilings"]) == sum(len(SR.modes_of(SR.allowed_of(w, h))) for (w, h) in SR.ALL_SIZES)
    assert {t for (_, _, _, _, t) in gold["tilings"]} == {(SR.DCT2, SR.DCT2), (SR.DCT8, SR.DST7), (SR.DST7, SR.DCT8), (SR.DST7, SR.DST7)}


def test_model_parts_estimates_order_against_the_reference(gold):
    """part sums == the reference's SSE table entry on every part; est and order == what InterSearch::xCalcMinDistSbt itself left in m_estMinDistSbt / m_sbtRdoOrder;
    m_skipSbtAll == one comparison on est[8]"""
    for i, c in enumerate(gold["cus"]):
        parts = SR.part_sums(c["y"], c["cb"], c["cr"])
        assert parts == c["parts"], (i, c["w"], c["h"])
        est, order = SR.estimate(parts, c["w"], c["h"], c["allowed"], c["cw"])
        assert est == c["est"], (i, c["w"], c["h"], c["allowed"], c["cw"])
        assert order == c["order"], (i, c["w"], c["h"], c["allowed"], est)
        assert SR.skip_all(est[8], c["dist_scale"]) == c["skip"], (i, est[8], c["dist_scale"])


def test_model_and_library_tilings_and_types_against_the_reference(gold):
    """getSbtTuTiling's rectangles of both tiles and every component and xSetTrTypes' luma types == the model, the Python mirror and vvhip_sbt_tiles (host arithmetic of the
    library: runs without a device)"""
    from vvenc_amd import hotpath as HP
    from vvenc_amd.lib import LIB_PATH
    lib = C.CDLL(LIB_PATH)
    for (w, h, mode, rects, types) in gold["tilings"]:
        for c in range(3):
            cw_, ch_ = w >> (c > 0), h >> (c > 0)
            assert [tuple(int(v) for v in rects[t][c]) for t in range(2)] == SR.tiling(cw_, ch_, mode), (w, h, mode, c)
        assert SR.tr_types(w, h, mode) == types, (w, h, mode)
        item = HP.make_sbt_items([(1000, 9001, 20002, w + 3, w // 2 + 5, w, h, SR.allowed_of(w, h))])[0]
        mirror = HP.sbt_tiles(item, mode)
        out = np.zeros(3, HP.SBT_TILE_DTYPE)
        assert lib.vvhip_sbt_tiles(item.tobytes(), mode, out.ctypes.data_as(C.c_void_p)) == 0
        assert out.tobytes() == mirror.tobytes(), (w, h, mode)
        for c in range(3):
            x, y, tw, th = (int(v) for v in rects[mode & 1][c])
            stride = int(item["stride_c" if c else "stride_y"])
            assert (int(out[c]["x"]), int(out[c]["y"]), int(out[c]["width"]), int(out[c]["height"])) == (x, y, tw, th)
            assert int(out[c]["resi_off"]) == int(item[("y_off", "cb_off", "cr_off")[c]]) + y * stride + x and int(out[c]["stride"]) == stride
            assert (int(out[c]["tr_hor"]), int(out[c]["tr_ver"])) == (types if c == 0 else (SR.DCT2, SR.DCT2))
    item = HP.make_sbt_items([(0, 0, 0, 8, 4, 8, 8, 6)])[0]
    out = np.zeros(3, HP.SBT_TILE_DTYPE)
    for bad_mode in (-1, 8, 4, 6):      # outside 0..7; quad modes on a side of 8
        assert lib.vvhip_sbt_tiles(item.tobytes(), bad_mode, out.ctypes.data_as(C.c_void_p)) != 0
        with pytest.raises(ValueError):
            HP.sbt_tiles(item, bad_mode)


def test_model_placement_against_the_reference(gold):
    """the whole block's SSE of a placed reconstruction == the reference's SSE table entry on it"""
    assert len(gold["placed"]) >= 12
    for p in gold["placed"]:
        placed = SR.place(p["tile"], p["w"], p["h"], p["mode"])
        x, y, tw, th = SR.coded_tile(p["w"], p["h"], p["mode"])
        outside = np.ones((p["h"], p["w"]), bool)
        outside[y:y + th, x:x + tw] = False
        assert not placed[outside].any() and np.array_equal(placed[y:y + th, x:x + tw], p["tile"])
        assert SR.sse(placed, p["org"]) == p["sse"] == SR.sse(p["tile"], p["org"][y:y + th, x:x + tw]) + SR.sse(0, p["org"][outside])


def test_lists_cover_what_the_gpu_tier_relies_on():
    """mixed_specs: every size, several CUs per wave, int16-range and all-zero CUs, proper subsets of sbt_allowed; the layouts: odd offsets and pitches (2-byte accesses),
    4-byte and 16-byte aligned ones; blocks never overlap"""
    specs = SC.mixed_specs(41)
    assert {b[0].shape[::-1] for (_, b) in specs} == {s for s in SR.ALL_SIZES}
    assert any(a != SR.allowed_of(*b[0].shape[::-1]) for (a, b) in specs) and any(not b[0].any() for (_, b) in specs) and any(int(np.abs(b[0].astype(np.int32)).max()) > 30000 for (_, b) in specs)
    for L in (SC.compact(specs), SC.compact(specs, odd_gaps=True), SC.planes(specs), SC.planes(specs, odd=True)):
        taken = np.zeros(L.resi.size, np.int32)
        for i in range(len(L.items)):
            taken += L.block_mask([i])
            for c in range(3):
                assert np.array_equal(L.view(L.resi, i, c), L.blocks[i][c])
        assert taken.max() == 1 and (L.resi[taken == 0] == SC.SENTINEL).all()
    odd = SC.compact(specs, odd_gaps=True)
    assert {int(v) & 7 for v in odd.items["y_off"]} >= {0, 1, 2, 4} and any(int(v) & 1 for v in odd.items["cb_off"])
    assert all(int(v) & 1 for v in SC.planes(specs).items["stride_c"])


def test_chain_model_through_the_oracle(oracle):
    """the model of the full chain: every candidate's coded tile through the oracle's TU pipeline with the tile's types, placed, scored.  At the low QPs the textured CUs
    keep levels, at the high ones the flat CUs' tiles quantise to nothing: then the placed block is zero and the CU's SSE is its residual's energy; a coded tile's SSE is
    the TU's own plus the energy of the zeroed part"""
    world = SC.chain_world()
    L = world["listed"]
    assert len(world["candidates"]) == 2 * len(SC.CHAIN_SIZES) and {m for (_, m) in world["candidates"]} == set(range(8))
    for qps in SC.CHAIN_QPS:
        exp = SC.chain_expected(oracle, world, qps)
        zero = coded = 0
        for (cu, mode), comps in zip(world["candidates"], exp):
            for c, e in enumerate(comps):
                blk = L.blocks[cu][c]
                x, y, tw, th = e["tile"]
                if e["stats"]["abs_sum"] == 0:
                    zero += 1
                    assert not e["placed"].any() and e["sse"] == SR.sse(blk, 0)
                else:
                    coded += 1
                    assert e["sse"] == e["stats"]["sse"] + SR.sse(blk, 0) - SR.sse(blk[y:y + th, x:x + tw], 0)
        assert zero and coded, qps
    assert any(e["types"] == (SR.DCT2, SR.DCT2) for comps in exp for e in comps[:1]) and any(e["types"] == (SR.DCT8, SR.DST7) for comps in exp for e in comps[:1])
