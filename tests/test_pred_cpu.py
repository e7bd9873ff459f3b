"""CPU tier of the inter-prediction list entry (vvhip_pred_inter_batch, vvhip_interp_chroma_batch): the ABI, and the expected values the GPU tier uses
(tests/pred_ref.py), pinned before any GPU is involved."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import pred_ref as PR  # noqa: E402


def test_pred_symbols_and_prototypes():
    from vvenc_amd.lib import LIB_PATH, PROTOTYPES
    lib = C.CDLL(LIB_PATH)
    for name, nargs in (("vvhip_pred_inter_batch", 11), ("vvhip_interp_chroma_batch", 10)):
        assert hasattr(lib, name), "missing export " + name
        assert name in PROTOTYPES and len(PROTOTYPES[name][1]) == nargs, name
    hdr = open(os.path.join(ROOT, "include", "vvenc_hip.h")).read()
    assert "vvhip_pred_inter_batch" in hdr and "vvhip_interp_chroma_batch" in hdr and "xFinalPaddedMCForDMVR" in hdr      # the out-of-scope list is in the header


def test_pred_item_layout(tmp_path):
    """vvhip_pred_item as the C compiler lays it out == the numpy record the Python layer fills: 32 bytes, documented offsets"""
    from vvenc_amd.hotpath import PRED_ITEM_DTYPE
    fields = ["dst_off", "org_off", "ref_off", "frac", "width", "height", "ref_plane", "chroma", "alt_hpel"]
    src = tmp_path / "layout.cpp"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "vvenc_hip.h"\nint main(void){ printf("%zu", sizeof(vvhip_pred_item));\n' +
                   "".join('printf(" %%zu", offsetof(vvhip_pred_item, %s));\n' % f for f in fields) + "return 0; }\n")
    exe = tmp_path / "layout"
    subprocess.check_call(["g++", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    assert got == [32, 0, 4, 8, 16, 24, 26, 28, 30, 31], got
    assert PRED_ITEM_DTYPE.itemsize == got[0]
    assert [PRED_ITEM_DTYPE.fields[f][1] for f in fields] == got[1:]


def _rows():
    from oracle.oracle import RefLib
    if not RefLib.available():
        pytest.skip("oracle/_ref/libvvenc_ref.so not built (needs the reference sources)")
    return RefLib(0), RefLib(1)


def _picture(rng, h, w, bd):
    yy, xx = np.mgrid[0:h, 0:w]
    top = (1 << bd) - 1
    a = np.clip(top / 2 + top / 5 * np.sin(xx / 5.0) * np.cos(yy / 4.0) + rng.normal(0, top / 30, (h, w)), 0, top).astype(np.int16)
    a[:8, :8] = 0          # saturated corners: the clip of the last pass
    a[-8:, -8:] = top
    return a


@pytest.mark.parametrize("bd", [8, 10])
def test_chroma_composition_scalar_row_equals_x86_row(bd):
    """the chroma expected values (pred_ref.chroma_pred: the two table passes of xPredInterBlk, :860-865) on the reference's scalar row and on its x86 row, every one
    of the 32 x 32 phases for every chroma block size 2..64 x 2..64, rndRes alternating: identical samples"""
    scalar, simd = _rows()
    rng = np.random.default_rng(500 + bd)
    arr = _picture(rng, 64 + 24, 64 + 48, bd)
    for (w, h) in PR.CHROMA_SIZES:
        for yf in range(32):
            for xf in range(32):
                rnd = (xf + yf + w) & 1
                x, y = 4 + (xf * 3 + yf) % 8, 4 + (yf * 5 + xf) % 8
                a = PR.chroma_pred(scalar, arr, y, x, w, h, xf, yf, rnd, bd)
                b = PR.chroma_pred(simd, arr, y, x, w, h, xf, yf, rnd, bd)
                assert np.array_equal(a, b), (w, h, xf, yf, rnd, bd)


@pytest.mark.parametrize("bd", [8, 10, 12])
def test_two_pass_form_of_the_kernel_equals_the_reference_dispatch(oracle, bd):
    """pred.hip runs EVERY fraction pair as horizontal (isFirst, !isLast) then vertical (!isFirst) with the one-tap set { 64 } for a zero fraction.  The reference dispatches
    a single pass for one zero fraction and a copy for two; this checks on the CPU (numpy model pred_ref.kernel_form against the C restatement of the reference) that the forms agree
    sample for sample — chroma and luma, rndRes 0 and 1, including all-zero and all-max neighbourhoods"""
    rng = np.random.default_rng(900 + bd)
    arr = _picture(rng, 56, 72, bd)
    for chroma in (1, 0):
        sizes = ((2, 2), (4, 8), (8, 4), (16, 16)) if chroma else ((4, 4), (8, 8), (16, 4), (32, 16))
        nph = 32 if chroma else 16
        for (w, h) in sizes:
            for yf in list(range(0, nph, 3)) + [nph // 2]:
                for xf in list(range(0, nph, 5)) + [nph // 2]:
                    for rnd in (0, 1):
                        for (x, y) in ((4, 4), (72 - w - 5, 56 - h - 5), (20, 17)):
                            if chroma:
                                exp = PR.chroma_pred(oracle, arr, y, x, w, h, xf, yf, rnd, bd)
                                th = (list(oracle.if_coeff(2, xf)[1][:4]), 1) if xf else ([64], 0)
                                tv = (list(oracle.if_coeff(2, yf)[1][:4]), 1) if yf else ([64], 0)
                            else:
                                exp = PR.luma_pred(oracle, arr, y, x, w, h, xf, yf, rnd, bd, 0)
                                s = 1 if (w, h) == (4, 4) else 0
                                th = (list(oracle.if_coeff(s, xf)[1]), 3) if xf else ([64], 0)
                                tv = (list(oracle.if_coeff(s, yf)[1]), 3) if yf else ([64], 0)
                            got = PR.kernel_form([int(c) for c in th[0]], th[1], [int(c) for c in tv[0]], tv[1], arr, y, x, w, h, rnd, bd)
                            assert np.array_equal(got, exp), (chroma, w, h, xf, yf, rnd, bd, x, y)


def test_oracle_and_reference_agree_on_the_chroma_composition(oracle):
    """smoke() checks its chroma case against the C restatement: it gives the reference's samples"""
    scalar, _ = _rows()
    rng = np.random.default_rng(77)
    arr = _picture(rng, 48, 64, 10)
    for (w, h) in ((2, 2), (4, 4), (8, 16), (32, 8)):
        for (xf, yf) in ((0, 0), (5, 0), (0, 29), (17, 3), (16, 16), (31, 31)):
            for rnd in (0, 1):
                assert np.array_equal(PR.chroma_pred(oracle, arr, 6, 9, w, h, xf, yf, rnd, 10), PR.chroma_pred(scalar, arr, 6, 9, w, h, xf, yf, rnd, 10)), (w, h, xf, yf, rnd)


def test_schedule_helpers():
    sizes = [(64, 64), (128, 4), (8, 8), (2, 2), (32, 128)]
    pos, rows = PR.shelf_pack(sizes, 160)
    seen = np.zeros((rows, 160), np.int32)
    for (w, h), (x, y) in zip(sizes, pos):
        seen[y:y + h, x:x + w] += 1
    assert seen.max() == 1
    a, b = np.array([[-8192, 8191]], np.int16), np.array([[-8192, 8191]], np.int16)
    assert PR.bi_average(a, b, 10).tolist() == [[0, 1023]]
