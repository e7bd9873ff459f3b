"""CPU tier of the extension forms of the prediction list (vvhip_pred_inter_batch_ex: BDOF, DMVR's padded reference): the ABI, and the expected values the GPU tier
uses (tests/bdof_ref.py), pinned before any GPU is involved.

tests/golden/bdof.npz holds what the reference's own xApplyBDOF returned on recorded frames, on its scalar row and on its x86 row (tests/bdof_golden_gen.cpp);
bdof_ref's numpy restatement must reproduce every case.  The guard conditions at the end are asserted on the model alone: the lists the GPU tier runs are lists on
which ignoring a flag gives other values, so a kernel that ignores the flags cannot pass there."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import bdof_cases as BC  # noqa: E402
import bdof_ref as BR  # noqa: E402
import pred_ref as PR  # noqa: E402

SHAPES = [(16, 16), (16, 8), (8, 16)]


def _golden():
    z = np.load(os.path.join(ROOT, "tests", "golden", "bdof.npz"))
    return [dict(bd=int(z["c%03d_hdr" % i][0]), w=int(z["c%03d_hdr" % i][1]), h=int(z["c%03d_hdr" % i][2]), f0=z["c%03d_f0" % i], f1=z["c%03d_f1" % i],
                 scalar=z["c%03d_scalar" % i], simd=z["c%03d_simd" % i]) for i in range(int(z["n"]))]


def _rows():
    from oracle.oracle import RefLib
    if not RefLib.available():
        pytest.skip("oracle/_ref/libvvenc_ref.so not built (needs the reference sources)")
    return RefLib(0), RefLib(1)


def test_ex_symbol_prototype_and_header():
    from vvenc_amd.lib import LIB_PATH, PROTOTYPES
    lib = C.CDLL(LIB_PATH)
    assert hasattr(lib, "vvhip_pred_inter_batch_ex"), "missing export vvhip_pred_inter_batch_ex"
    assert len(PROTOTYPES["vvhip_pred_inter_batch_ex"][1]) == 12 and len(PROTOTYPES["vvhip_pred_inter_batch"][1]) == 11
    hdr = open(os.path.join(ROOT, "include", "vvenc_hip.h")).read()
    assert "vvhip_pred_inter_batch_ex" in hdr and "VVHIP_PRED_EXT_BDOF" in hdr and "VVHIP_PRED_EXT_DMVR_PAD" in hdr


def test_pred_ext_layout(tmp_path):
    """vvhip_pred_ext as the C compiler lays it out == the numpy record the Python layer fills: 8 bytes; vvhip_pred_item is still 32"""
    from vvenc_amd.hotpath import PRED_EXT_DTYPE, PRED_ITEM_DTYPE, PRED_EXT_BDOF, PRED_EXT_DMVR_PAD
    fields = ["flags", "pad_dx", "pad_dy", "rsv"]
    src = tmp_path / "layout.cpp"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "vvenc_hip.h"\nint main(void){ printf("%zu %zu %d %d", sizeof(vvhip_pred_item), sizeof(vvhip_pred_ext), '
                   'VVHIP_PRED_EXT_BDOF, VVHIP_PRED_EXT_DMVR_PAD);\n' + "".join('printf(" %%zu", offsetof(vvhip_pred_ext, %s));\n' % f for f in fields) + "return 0; }\n")
    exe = tmp_path / "layout"
    subprocess.check_call(["g++", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    assert got == [32, 8, 1, 2, 0, 1, 3, 5], got
    assert PRED_EXT_DTYPE.itemsize == 8 and PRED_ITEM_DTYPE.itemsize == 32 and (PRED_EXT_BDOF, PRED_EXT_DMVR_PAD) == (1, 2)
    assert [PRED_EXT_DTYPE.fields[f][1] for f in fields] == got[4:]
    assert PRED_EXT_DTYPE == BC.PRED_EXT_DTYPE and PRED_ITEM_DTYPE == BC.PRED_ITEM_DTYPE and (BR.EXT_BDOF, BR.EXT_DMVR_PAD) == (1, 2)


def test_golden_covers_what_it_must():
    """all three unit shapes at bit depths 8 and 10; flat blocks (both sums zero); tmpx or tmpy at +15 and at -15; the extreme sample values 0 and max"""
    cases = _golden()
    assert {(c["bd"], c["w"], c["h"]) for c in cases} == {(bd, w, h) for bd in (8, 10) for (w, h) in SHAPES}
    for bd in (8, 10):
        hr, top = max(2, 14 - bd), (1 << bd) - 1
        for (w, h) in SHAPES:
            mine = [c for c in cases if (c["bd"], c["w"], c["h"]) == (bd, w, h)]
            det = [BR.bdof_from_frames(c["f0"], c["f1"], bd, detail=True) for c in mine]
            assert any(not d[3][0].any() and not d[3][1].any() for d in det), "no flat case"
            assert any((d[1] == 15).any() or (d[2] == 15).any() for d in det) and any((d[1] == -15).any() or (d[2] == -15).any() for d in det), "offsets never reach +-15"
            assert any((d[1] == 15).any() for d in det) and any((d[1] == -15).any() for d in det) and any((d[2] == 15).any() for d in det) and any((d[2] == -15).any() for d in det)
            lo, hi = -8192, (top << hr) - 8192
            assert any(set(np.unique(c["f0"])) == {lo, hi} for c in mine), "no case made of the extreme sample values"
            assert any((d[0] == 0).any() for d in det) and any((d[0] == top).any() for d in det)


def test_golden_rows_agree():
    for i, c in enumerate(_golden()):
        assert np.array_equal(c["scalar"], c["simd"]), "case %d: the reference's scalar row and x86 row differ" % i


def test_bdof_ref_equals_golden():
    for i, c in enumerate(_golden()):
        got = BR.bdof_from_frames(c["f0"], c["f1"], c["bd"])
        assert got.dtype == np.int16 and np.array_equal(got, c["scalar"]), "case %d (%dx%d, %d bit)" % (i, c["w"], c["h"], c["bd"])


@pytest.mark.parametrize("bd", [8, 10])
def test_dmvr_window_zero_delta_is_the_plain_block(bd):
    """a DMVR item whose integer delta is zero reads the true plane: bdof_ref on its padded window == pred_ref.expected_block; so does the padded window itself
    at the START position, where the clamp is a no-op"""
    lib = _rows()[0]
    pl, _ = BC.planes(bd, 5)
    b = BC.ListBuilder(pl, 6)
    for (w, h) in BC.DMVR_SHAPES:
        for k in range(6):
            fr = tuple((int(b.rng.integers(0, 16)), int(b.rng.integers(0, 16))) for _ in (0, 1))
            b.add(w, h, 0, 0, fr, (0, 1), BR.EXT_DMVR_PAD, ((0, 0), (0, 0)))
            fr = tuple((int(b.rng.integers(0, 32)), int(b.rng.integers(0, 32))) for _ in (0, 1))
            b.add(w // 2, h // 2, 1, 0, fr, (2, 3), BR.EXT_DMVR_PAD, ((0, 0), (0, 0)))
    items, ext, pos = b.done()
    for it, e, p in zip(items, ext, pos):
        want = PR.expected_block(lib, pl, p, it, bd)
        assert np.array_equal(BR.expected_block_ex(lib, pl, p, it, e, bd), want)
        w, h, chroma = int(it["width"]), int(it["height"]), int(it["chroma"])
        taps, pad = (4, 1) if chroma else (8, 2)
        out = []
        for l in (0, 1):
            win, y, x = BR.padded_window(pl[int(it["ref_plane"][l])], p[l][1], p[l][0], w, h, taps, pad)
            out.append(BR._list_pred(lib, win, y, x, w, h, int(it["frac"][l][0]), int(it["frac"][l][1]), False, bd, chroma, 0))
        assert np.array_equal(PR.bi_average(out[0], out[1], bd), want)


def test_padded_window_is_the_clamped_plane():
    """reading the replication-padded copy == reading the true plane with every coordinate clamped to the prefetched window (what the kernel does)"""
    pl, _ = BC.planes(10, 9)
    for (w, h, chroma, x, y) in ((16, 16, 0, 40, 50), (8, 16, 0, 6, 5), (4, 8, 1, 30, 2), (8, 8, 1, 2, 60)):
        taps, pad = (4, 1) if chroma else (8, 2)
        arr = pl[2 if chroma else 0]
        win, wy, wx = BR.padded_window(arr, y, x, w, h, taps, pad)
        cl = BR.clamped_plane(arr, y, x, w, h, taps)
        r = taps // 2 - 1 + pad
        assert np.array_equal(win[wy - r:wy + h + taps // 2 + pad, wx - r:wx + w + taps // 2 + pad], cl[y - r:y + h + taps // 2 + pad, x - r:x + w + taps // 2 + pad])


@pytest.mark.parametrize("bd", [8, 10])
def test_split_of_a_32x64_item_is_eight_16x16_items(bd):
    lib = _rows()[0]
    pl, _ = BC.planes(bd, 11)
    b = BC.ListBuilder(pl, 12)
    b.add(32, 64, 0, 0, ((5, 11), (14, 2)), (0, 1), BR.EXT_BDOF)
    items, ext, pos = b.done()
    whole = BR.expected_block_ex(lib, pl, pos[0], items[0], ext[0], bd)
    assert len(BR.bdof_units(32, 64)) == 8
    for (x0, y0, uw, uh) in BR.bdof_units(32, 64):
        assert (uw, uh) == (16, 16)
        it = items[0].copy()
        it["width"], it["height"] = 16, 16
        p = [(pos[0][l][0] + x0, pos[0][l][1] + y0) for l in (0, 1)]
        assert np.array_equal(BR.expected_block_ex(lib, pl, p, it, ext[0], bd), whole[y0:y0 + 16, x0:x0 + 16])


def test_rows_agree_on_the_extension_lists():
    """the expected values of the DMVR list and of a part of the BDOF list on the reference's scalar row and on its x86 row"""
    r0, r1 = _rows()
    pl, _ = BC.planes(10, 21)
    for (items, ext, pos) in (BC.dmvr_list(pl, 22), BC.mixed_list(pl, 23)):
        for it, e, p in zip(items, ext, pos):
            assert np.array_equal(BR.expected_block_ex(r0, pl, p, it, e, 10), BR.expected_block_ex(r1, pl, p, it, e, 10))


@pytest.mark.parametrize("bd", [8, 10])
def test_guard_bdof_list_differs_from_the_plain_average(bd):
    """over the BDOF list of the GPU tier the expected block differs from the plain bi_average in more than half of the items, and in at least one item of every
    unit shape: a kernel that ignores the BDOF flag fails there"""
    lib = _rows()[0]
    pl, _ = BC.planes(bd, 100 + bd)
    items, ext, pos = BC.bdof_list(pl, 200 + bd)
    differs = np.array([not np.array_equal(BR.expected_block_ex(lib, pl, p, it, e, bd), BR.expected_block_ex(lib, pl, p, it, e, bd, bdof=False))
                        for it, e, p in zip(items, ext, pos)])
    print("BDOF list, %d bit: %d of %d items differ from the plain average" % (bd, differs.sum(), differs.size))
    assert differs.sum() * 2 > differs.size
    for shape in SHAPES:
        assert any(d for d, it in zip(differs, items) if BC.unit_shape(it) == shape), shape


@pytest.mark.parametrize("bd", [8, 10])
def test_guard_dmvr_list_differs_from_the_unclamped_read(bd):
    """over the DMVR list of the GPU tier the clamped expectation differs from the unclamped one in more than half of the items with a non-zero delta"""
    lib = _rows()[0]
    pl, _ = BC.planes(bd, 100 + bd)
    items, ext, pos = BC.dmvr_list(pl, 300 + bd)
    moved = [k for k in range(len(items)) if any(ext[k]["pad_dx"]) or any(ext[k]["pad_dy"])]
    differs = [k for k in moved if not np.array_equal(BR.expected_block_ex(lib, pl, pos[k], items[k], ext[k], bd), BR.expected_block_ex(lib, pl, pos[k], items[k], ext[k], bd, clamp=False))]
    print("DMVR list, %d bit: %d of %d moved items differ from the unclamped read" % (bd, len(differs), len(moved)))
    assert len(differs) * 2 > len(moved)
    for chroma in (0, 1):
        assert any(int(items[k]["chroma"]) == chroma for k in differs)
    with_bdof = [k for k in range(len(items)) if int(ext[k]["flags"]) & BR.EXT_BDOF]
    d2 = [k for k in with_bdof if not np.array_equal(BR.expected_block_ex(lib, pl, pos[k], items[k], ext[k], bd), BR.expected_block_ex(lib, pl, pos[k], items[k], ext[k], bd, bdof=False))]
    assert len(d2) * 2 > len(with_bdof)


def test_dmvr_helper_mirrors_and_switches():
    """dmvr_pred_items: list 0 moves by +mvd, list 1 by -mvd; integer deltas per component scale; BDOF only where min_cost >= 2 * dx * dy"""
    from vvenc_amd.hotpath import DMVR_RESULT_DTYPE, dmvr_pred_items
    res = np.zeros(3, DMVR_RESULT_DTYPE)
    res[0] = (0, 0, 0, 1000)
    res[1] = (-20, 35, 0, 511)
    res[2] = (32, -32, 0, 512)
    start = [((5, -7), (-5, 7)), ((3, 14), (-3, -14)), ((-9, 0), (8, 31))]
    pos = [(16, 16), (32, 48), (64, 16)]
    items, ext = dmvr_pred_items(res, start, pos, (0, 1), (160, 160), 16, 16, bdof=True, chroma_planes=((2, 3),), chroma_strides=(96, 96))
    assert len(items) == 6 and list(ext["flags"][:3]) == [1, 2, 3] and list(ext["flags"][3:]) == [0, 2, 2]
    for i in range(3):
        for l, sgn in ((0, 1), (1, -1)):
            rx, ry = start[i][l][0] + sgn * int(res[i]["mvd_x"]), start[i][l][1] + sgn * int(res[i]["mvd_y"])
            assert tuple(items[i]["frac"][l]) == (rx & 15, ry & 15)
            assert int(items[i]["ref_off"][l]) == (pos[i][1] + (ry >> 4)) * 160 + pos[i][0] + (rx >> 4)
            assert (int(ext[i]["pad_dx"][l]), int(ext[i]["pad_dy"][l])) == ((rx >> 4) - (start[i][l][0] >> 4), (ry >> 4) - (start[i][l][1] >> 4))
            assert tuple(items[3 + i]["frac"][l]) == (rx & 31, ry & 31)
            assert int(items[3 + i]["ref_off"][l]) == (pos[i][1] // 2 + (ry >> 5)) * 96 + pos[i][0] // 2 + (rx >> 5)
            if i:
                assert (int(ext[3 + i]["pad_dx"][l]), int(ext[3 + i]["pad_dy"][l])) == ((rx >> 5) - (start[i][l][0] >> 5), (ry >> 5) - (start[i][l][1] >> 5))
    assert tuple(items[3]["ref_plane"]) == (2, 3) and int(items[3]["width"]) == 8 and int(items[3]["chroma"]) == 1
