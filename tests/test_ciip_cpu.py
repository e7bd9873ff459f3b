"""CPU tier of the CIIP form of the prediction list (vvhip_pred_inter_batch_ciip): the numpy model of tests/ciip_ref.py against what the reference's own functions
returned (tests/golden/ciip.npz, made by tests/ciip_golden_gen.cpp), the sensitivity of that check, the ABI, and the lists the GPU tier runs."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import blend_cases as BLC  # noqa: E402
import blend_ref as BL  # noqa: E402
import ciip_cases as CC  # noqa: E402
import ciip_ref as CR  # noqa: E402


@pytest.fixture(scope="module")
def cases():
    return CR.golden_cases()


def test_ciip_symbol_prototype_and_header():
    """fails on a library without the entry"""
    from vvenc_amd.lib import LIB_PATH, PROTOTYPES
    lib = C.CDLL(LIB_PATH)
    assert hasattr(lib, "vvhip_pred_inter_batch_ciip"), "missing export vvhip_pred_inter_batch_ciip"
    assert len(PROTOTYPES["vvhip_pred_inter_batch_ciip"][1]) == 15 and len(PROTOTYPES["vvhip_pred_inter_batch_blend"][1]) == 13
    hdr = open(os.path.join(ROOT, "include", "vvenc_hip.h")).read()
    for word in ("vvhip_pred_inter_batch_ciip", "vvhip_pred_ciip", "VVHIP_PRED_CIIP_OFF", "VVHIP_PRED_CIIP_ON"):
        assert word in hdr


def test_pred_ciip_layout(tmp_path):
    """vvhip_pred_ciip as the C compiler lays it out == the numpy record the Python layer fills: 8 bytes"""
    from vvenc_amd.hotpath import PRED_CIIP_DTYPE, PRED_CIIP_OFF, PRED_CIIP_ON
    fields = ["ref_off", "mode", "num_intra", "rsv"]
    src = tmp_path / "layout.cpp"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "vvenc_hip.h"\nint main(void){ printf("%zu %d %d", sizeof(vvhip_pred_ciip), VVHIP_PRED_CIIP_OFF, VVHIP_PRED_CIIP_ON);\n'
                   + "".join('printf(" %%zu", offsetof(vvhip_pred_ciip, %s));\n' % f for f in fields) + "return 0; }\n")
    exe = tmp_path / "layout"
    subprocess.check_call(["g++", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    assert got == [8, 0, 1, 0, 4, 5, 6], got
    assert PRED_CIIP_DTYPE.itemsize == 8 and (PRED_CIIP_OFF, PRED_CIIP_ON) == (0, 1) == (CR.CIIP_OFF, CR.CIIP_ON)
    assert [PRED_CIIP_DTYPE.fields[f][1] for f in fields] == got[3:] and PRED_CIIP_DTYPE == CR.PRED_CIIP_DTYPE


def test_golden_covers_what_it_must(cases):
    """every luma and chroma size, the three num_intra values, both bit depths; samples inside the bit depth; the extremes; arrays only"""
    z = np.load(CR.GOLDEN)
    assert all(z[k].dtype.kind in "iu" for k in z.files) and os.path.getsize(CR.GOLDEN) < 300 * 1024
    seen = {(c["w"], c["h"], c["chroma"]) for c in cases}
    assert seen == set(CC.ALL_SIZES)
    assert {c["num_intra"] for c in cases} == {0, 1, 2} and {c["bd"] for c in cases} == {8, 10}
    for chroma in (0, 1):
        assert {(c["bd"], c["num_intra"]) for c in cases if c["chroma"] == chroma} == {(bd, ni) for bd in (8, 10) for ni in range(3)}
    for c in cases:
        top = (1 << c["bd"]) - 1
        assert c["line"].size == CR.line_len(c["w"], c["h"]) and c["inter"].shape == c["intra"].shape == c["result"].shape == (c["h"], c["w"])
        assert c["line"][0] == c["line"][c["w"] + 3]
        for a in (c["line"], c["inter"], c["intra"], c["result"]):
            assert a.min() >= 0 and a.max() <= top
    for bd in (8, 10):
        top = (1 << bd) - 1
        mine = [c for c in cases if c["bd"] == bd]
        assert any(c["line"].max() == 0 and c["inter"].max() == 0 for c in mine) and any(c["line"].min() == top and c["inter"].min() == top for c in mine)
        assert any(set(np.unique(c["line"])) == {0, top} and c["inter"].min() == top for c in mine) and any(set(np.unique(c["line"])) == {0, top} and c["inter"].max() == 0 for c in mine)
        assert any(c["result"].max() == top for c in mine) and any(c["result"].min() == 0 for c in mine)


def test_model_equals_golden(cases):
    """the four steps of the model == the reference's intra block and result, on every case"""
    for i, c in enumerate(cases):
        intra = CR.planar_intra(c["line"], c["w"], c["h"], c["chroma"])
        assert np.array_equal(intra, c["intra"]), ("intra", i, c["w"], c["h"], c["chroma"], np.argwhere(intra != c["intra"])[:3].tolist())
        assert np.array_equal(CR.weight(c["inter"], intra, c["num_intra"]), c["result"]), ("result", i)
        assert np.array_equal(CR.ciip(c["inter"], c["line"], c["chroma"], c["num_intra"]), c["result"]), i


def test_closed_form_equals_golden(cases):
    """the per-sample form the kernel evaluates — horPred = ( left << log2W ) + ( x + 1 ) ( topRight - left ), vertPred = ( top << log2H ) + ( y + 1 ) ( bottomLeft - top ) —
    gives the reference's intra block on every case (the PDPC-free ones directly, the others after the model's PDPC)"""
    for i, c in enumerate(cases):
        w, h = c["w"], c["h"]
        top, left = CR.split_line(c["line"], w, h)
        if not c["chroma"]:
            top, left = CR.smooth(top), CR.smooth(left)
        l2w, l2h = w.bit_length() - 1, h.bit_length() - 1
        xs, ys = np.arange(w)[None, :], np.arange(h)[:, None]
        lf, t = left[1:h + 1][:, None], top[1:w + 1][None, :]
        hor, ver = (lf << l2w) + (xs + 1) * (top[w + 1] - lf), (t << l2h) + (ys + 1) * (left[h + 1] - t)
        p = ((hor << l2h) + (ver << l2w) + (1 << (l2w + l2h))) >> (1 + l2w + l2h)
        assert np.array_equal(p.astype(np.int16), CR.planar_intra(c["line"], w, h, c["chroma"], pdpc=False)), i
        assert max(abs(int(hor.max())) << l2h, abs(int(ver.max())) << l2w) < 1 << 30


def test_sensitivity(cases):
    """the result differs from the inter block on every case that is not one flat value; dropping the smoothing changes a luma case, and so does dropping PDPC;
    a wrong num_intra changes a case"""
    for i, c in enumerate(cases):
        flat = c["line"].min() == c["line"].max() == c["inter"].min() == c["inter"].max()
        assert np.array_equal(c["result"], c["inter"]) == bool(flat), i
    luma = [c for c in cases if not c["chroma"]]
    assert any(not np.array_equal(CR.ciip(c["inter"], c["line"], 0, c["num_intra"], smoothing=False), c["result"]) for c in luma)
    assert any(not np.array_equal(CR.ciip(c["inter"], c["line"], 0, c["num_intra"], pdpc=False), c["result"]) for c in luma)
    assert any(not np.array_equal(CR.ciip(c["inter"], c["line"], c["chroma"], (c["num_intra"] + 1) % 3), c["result"]) for c in cases)
    # chroma takes no smoothing, and a chroma block of height 2 no PDPC: the model with the step forced equals the fixture there only because the step is skipped
    assert any(not np.array_equal(CR.planar_intra(c["line"], c["w"], c["h"], 0), c["intra"]) for c in cases if c["chroma"])
    assert any(c["chroma"] and c["h"] == 2 for c in cases)


@pytest.mark.parametrize("bd", [10, 8])
def test_gpu_lists_meet_the_margins_and_cover_what_they_must(bd):
    pl, _ = BLC.planes(bd, 100 + bd)
    items, ext, blend, ciip, lines, pos = CC.model_list(pl, 600 + bd)
    BLC.check_margins(pl, items, ext, pos)
    assert {(int(i["width"]), int(i["height"]), int(i["chroma"])) for i in items} == set(CC.ALL_SIZES)
    assert all((w, h, 0) in CC.ALL_SIZES and w * h > 512 for (w, h) in CC.TILED)          # a tile is at most 64 lanes x 8 samples: these are cut
    kinds = set()
    for it, bl, ci in zip(items, blend, ciip):
        assert int(ci["mode"]) == CR.CIIP_ON and 0 <= int(ci["ref_off"]) <= lines.size - CR.line_len(int(it["width"]), int(it["height"]))
        used = [l for l in (0, 1) if int(it["ref_plane"][l]) >= 0]
        assert all(int(it["frac"][l][0]) and int(it["frac"][l][1]) for l in used)
        kinds.add((len(used), int(bl["mode"]), int(bl["param"]), int(ci["num_intra"])))
        o = int(ci["ref_off"])
        assert lines[o] == lines[o + int(it["width"]) + 3]
    assert {k[:3] for k in kinds} == {(1, 0, 0), (2, 0, 0), (2, BL.BLEND_BCW, 0), (2, BL.BLEND_BCW, 4)} and {k[3] for k in kinds} == {0, 1, 2}
    assert any(int(c["ref_off"]) & 1 for c in ciip) and any(not int(c["ref_off"]) & 1 for c in ciip)
    top = (1 << bd) - 1
    assert lines[lines >= 0].max() <= top


def test_mixed_list_has_on_and_off_records():
    pl, _ = BLC.planes(10, 110)
    items, ext, blend, ciip, lines, pos = CC.mixed_on_off(pl, 510)
    on = ciip["mode"] == CR.CIIP_ON
    assert on.sum() >= 8 and (~on).sum() >= 8
    assert all(CC.eligible(items[i], ext[i], blend[i]) for i in np.flatnonzero(on))
    assert any(int(blend[i]["mode"]) == BL.BLEND_BCW for i in np.flatnonzero(on)) and any(int(items[i]["chroma"]) for i in np.flatnonzero(on))
    assert any(int(blend[i]["mode"]) == BL.BLEND_GEO for i in np.flatnonzero(~on)) and any(int(ext[i]["flags"]) for i in np.flatnonzero(~on))


def test_guard_ciip_changes_the_model_list(oracle):
    """ignoring the CIIP record gives other values on every item of the 10-bit list (the GPU tier compares against the model with it)"""
    pl, _ = BLC.planes(10, 110)
    items, ext, blend, ciip, lines, pos = CC.model_list(pl, 610)
    for i in range(0, len(items), 7):
        e = CC.expected(oracle, pl, pos[i], items[i], ext[i], blend[i], ciip[i], lines, 10)
        assert not np.array_equal(e, BLC.expected(oracle, pl, pos[i], items[i], ext[i], blend[i], 10)), i


def test_golden_replay_list_is_the_inter_block(cases):
    plane, items, ciip, lines = CC.golden_replay_list(cases)
    assert plane.shape[0] * plane.shape[1] * 2 < 4 << 20 and len(items) == len(cases)
    for c, it, ci in zip(cases, items, ciip):
        y, x = divmod(int(it["ref_off"][0]), plane.shape[1])
        assert np.array_equal(plane[y:y + c["h"], x:x + c["w"]], c["inter"]) and x >= 4 and y >= 4
        o = int(ci["ref_off"])
        assert np.array_equal(lines[o:o + c["line"].size], c["line"])
    BLC.check_no_overlap(items, int(BLC.compact_offsets(items)[1]))
