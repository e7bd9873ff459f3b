"""CPU tier of the affine prediction entry (vvhip_pred_affine_batch): the ABI, the numpy model the GPU tier uses (tests/affine_ref.py) against what the reference's own
xPredAffineBlk recorded (tests/golden/affine.npz), and guards that the GPU tier's lists (tests/affine_cases.py) exercise what they are meant to exercise."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import affine_cases as AC  # noqa: E402
import affine_ref as AR  # noqa: E402
import pred_ref as PR  # noqa: E402



def test_affine_symbol_prototype_and_header():
    from vvenc_amd.lib import LIB_PATH, PROTOTYPES
    lib = C.CDLL(LIB_PATH)
    assert hasattr(lib, "vvhip_pred_affine_batch"), "missing export vvhip_pred_affine_batch"
    assert "vvhip_pred_affine_batch" in PROTOTYPES and len(PROTOTYPES["vvhip_pred_affine_batch"][1]) == 14
    hdr = open(os.path.join(ROOT, "include", "vvenc_hip.h")).read()
    assert "xPredAffineBlk" in hdr and "ctu_size + 8 + 3" in hdr          # the semantics and the read bound are in the header
    out_of_scope = hdr[hdr.index("NOT done here"):][:300]
    assert "affine" not in out_of_scope and "PROF" not in out_of_scope


def test_affine_item_layout(tmp_path):
    """vvhip_pred_affine_item as the C compiler lays it out == the numpy record the Python layer fills == the record of the test lists: 80 bytes"""
    from vvenc_amd.hotpath import PRED_AFFINE_ITEM_DTYPE
    fields = ["dst_off", "org_off", "ref_off", "cpmv", "cu_x", "cu_y", "cu_w", "cu_h", "ref_plane", "chroma", "six_param", "prof", "rsv"]
    src = tmp_path / "layout.cpp"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "vvenc_hip.h"\nint main(void){ printf("%zu", sizeof(vvhip_pred_affine_item));\n' +
                   "".join('printf(" %%zu", offsetof(vvhip_pred_affine_item, %s));\n' % f for f in fields) + "return 0; }\n")
    exe = tmp_path / "layout"
    subprocess.check_call(["g++", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    assert got == [80, 0, 4, 8, 16, 64, 66, 68, 70, 72, 74, 75, 76, 77], got
    assert PRED_AFFINE_ITEM_DTYPE.itemsize == got[0] and PRED_AFFINE_ITEM_DTYPE == AC.ITEM_DTYPE
    assert [PRED_AFFINE_ITEM_DTYPE.fields[f][1] for f in fields] == got[1:]


def _rows():
    from oracle.oracle import RefLib
    if not RefLib.available():
        pytest.skip("oracle/_ref/libvvenc_ref.so not built (needs the reference sources)")
    return RefLib(0), RefLib(1)


def test_golden_rows_are_equal_and_cover_the_family():
    (pic_w, pic_h, ctu, _), _, cases = AC.golden_cases()
    n_prof = n_spread = n_clip = 0
    for (bd, lu, ch, pos, rec) in cases:
        for key in rec["scalar"]:
            assert np.array_equal(rec["scalar"][key], rec["simd"][key]), (lu, key)
        for l in (0, 1):
            if lu["ref_plane"][l] >= 0:
                m = AR.ListModel(lu, l)
                n_prof += m.prof
                n_spread += m.spread
                n_clip += not np.array_equal(AR.sub_vectors(lu, m, pic_w, pic_h, ctu), AR.sub_vectors(lu, m, pic_w, pic_h, ctu, clip=False))
    assert n_prof >= 15 and n_spread >= 5 and n_clip >= 5, (n_prof, n_spread, n_clip)
    assert os.path.getsize(AC.GOLDEN) < 512 * 1024


@pytest.mark.parametrize("row", [0, 1], ids=["ref-scalar", "ref-simd"])
def test_model_equals_golden(row):
    """the numpy model around the interpolation passes of row `row` == what xPredAffineBlk of that row recorded, per list, luma and Cb: tolerance 0"""
    lib = _rows()[row]
    (pic_w, pic_h, ctu, _), planes, cases = AC.golden_cases()
    for k, (bd, lu, ch, pos, rec) in enumerate(cases):
        for it, cc in ((lu, 0), (ch, 1)):
            for l in (0, 1):
                if it["ref_plane"][l] < 0:
                    continue
                got = AR.list_block(lib, planes[bd], pos[cc], it, l, bd, pic_w, pic_h, ctu)
                exp = rec["simd" if row else "scalar"][(l, cc)]
                assert np.array_equal(got, exp), (k, bd, cc, l, lu, int(np.abs(got.astype(int) - exp).max()))


def test_prof_off_equals_the_expanded_4x4_items(oracle):
    """with prof = 0 an affine item is its 4x4 items of vvhip_pred_inter_batch: the model == pred_ref.expected_block on the host-expanded list, luma and chroma"""
    from vvenc_amd.hotpath import PRED_ITEM_DTYPE
    world = AC.World(10, 64, seed=5)
    items, pos = AC.size_list(world, 32, 3, reps=1)
    strides = [a.shape[1] for a in world.np]
    for k in range(0, len(items), 3):          # a third of the list: luma and chroma alternate
        it = items[k].copy()
        it["prof"] = 0
        if int(it["cu_w"]) * int(it["cu_h"]) > 64 * 64:
            continue
        exp = AR.expected_block(oracle, world.np, pos[k], it, 10, world.pic_w, world.pic_h, world.ctu)
        ex, where, vec = AR.expand_items(it, strides, world.pic_w, world.pic_h, world.ctu, PRED_ITEM_DTYPE)
        c = int(it["chroma"])
        bw, bh = int(it["cu_w"]) >> c, int(it["cu_h"]) >> c
        flat = np.zeros(bw * bh, np.int16)
        for j, (sx, sy) in enumerate(where):
            p = [None, None]
            for l in vec:
                p[l] = (pos[k][l][0] + 4 * sx + int(vec[l][sy, sx][0]), pos[k][l][1] + 4 * sy + int(vec[l][sy, sx][1]))
            flat[16 * j:16 * j + 16] = PR.expected_block(oracle, world.np, p, ex[j], 10).reshape(-1)
        assert np.array_equal(AR.blocks_to_block(flat, bw, bh), exp), (k, it)


# ---- guards on the lists of the GPU tier -------------------------------------------------------------------------------------------------------------------

def test_guard_prof_changes_most_luma_items_that_ask_for_it(oracle):
    for (bd, D, seed) in AC.TIER_LISTS:
        world = AC.World(bd, 128, seed=seed)
        items, pos = AC.size_list(world, D, seed)
        asked = changed = 0
        for k in range(len(items)):
            it = items[k]
            if int(it["chroma"]) or not int(it["prof"]) or int(it["cu_w"]) * int(it["cu_h"]) > 32 * 32:          # (the small sizes: the guard stays quick)
                continue
            on = [AR.ListModel(it, l).prof for l in (0, 1) if it["ref_plane"][l] >= 0]
            asked += 1
            if any(on):
                a = AR.expected_block(oracle, world.np, pos[k], it, bd, world.pic_w, world.pic_h, world.ctu)
                b = AR.expected_block(oracle, world.np, pos[k], it, bd, world.pic_w, world.pic_h, world.ctu, force_prof=False)
                changed += not np.array_equal(a, b)
        print("PROF guard: bit depth %d D %d: %d of %d luma items that ask for PROF are changed by it" % (bd, D, changed, asked))
        assert asked >= 8 and 2 * changed > asked, (bd, D, asked, changed)


def test_guard_spread_limit_and_search_threshold():
    for (bd, D, seed) in AC.TIER_LISTS:
        world = AC.World(bd, 128, seed=seed)
        items, _ = AC.size_list(world, D, seed)
        lum = [items[k] for k in range(len(items)) if not int(items[k]["chroma"])]
        models = [[AR.ListModel(it, l) for l in (0, 1) if it["ref_plane"][l] >= 0] for it in lum]
        over = sum(any(m.spread for m in ms) for ms in models)
        if D == 256:
            assert over >= 0.10 * len(lum) and len(lum) - over >= 0.50 * len(lum), (bd, over, len(lum))
        else:
            two = [(it, ms) for it, ms in zip(lum, models) if int(it["prof"]) >= 2]
            above = sum(any(m.over_threshold[7 if int(it["prof"]) == 2 else 8] for m in ms) for it, ms in two)
            assert above >= 0.20 * len(two) and len(two) - above >= 0.20 * len(two), (bd, above, len(two))


def test_guard_every_edge_case_is_moved_by_the_picture_clip(oracle):
    for ctu in (32, 64, 128):
        world = AC.World(10, ctu, seed=ctu)
        items, pos = AC.edge_list(world, ctu)
        ext = 64 + 48          # the unclipped vectors point ctu + 40 samples (and their spread) outward: a wider copy of the planes for the comparison only
        wide = [np.pad(a, ext, mode="symmetric") for a in world.np]
        for k in range(len(items)):
            it = items[k]
            wpos = [None if p is None else (p[0] + ext, p[1] + ext) for p in pos[k]]
            for l in (0, 1):
                if it["ref_plane"][l] >= 0:
                    m = AR.ListModel(it, l)
                    assert not np.array_equal(AR.sub_vectors(it, m, world.pic_w, world.pic_h, ctu), AR.sub_vectors(it, m, world.pic_w, world.pic_h, ctu, clip=False)), (ctu, k, l)
            a = AR.expected_block(oracle, wide, wpos, it, 10, world.pic_w, world.pic_h, ctu)
            b = AR.expected_block(oracle, wide, wpos, it, 10, world.pic_w, world.pic_h, ctu, clip=False)
            assert not np.array_equal(a, b), (ctu, k)
            assert np.array_equal(a, AR.expected_block(oracle, world.np, pos[k], it, 10, world.pic_w, world.pic_h, ctu)), (ctu, k)
            m = world.m >> int(it["chroma"])
            assert max(AR.read_extent(it, world.pic_w, world.pic_h, ctu)) <= m, (ctu, k)          # the clipped reads stay inside the margin of ctu + 16


def test_guard_extremes_reach_the_dmv_and_the_di_clip(oracle):
    world = AC.World(10, 128, "checker", seed=9)
    items, pos = AC.extreme_list(world, 9)
    hit_dmv = hit_di = 0
    for k in range(len(items)):
        it = items[k]
        if int(it["chroma"]):
            continue
        for l in (0, 1):
            if it["ref_plane"][l] < 0:
                continue
            m = AR.ListModel(it, l)
            if not m.prof:
                continue
            hit_dmv += int(np.abs(m.dmx).max() == 31 or np.abs(m.dmy).max() == 31)
            vec = AR.sub_vectors(it, m, world.pic_w, world.pic_h, world.ctu)
            arr, (x0, y0) = world.np[int(it["ref_plane"][l])], pos[k][l]
            hit = False
            for sy in range(vec.shape[0]):
                for sx in range(vec.shape[1]):
                    xi, yi, xf, yf = (int(v) for v in vec[sy, sx])
                    x, y = x0 + 4 * sx + xi, y0 + 4 * sy + yi
                    fr = (arr[y + (yf >> 3) - 1:y + (yf >> 3) + 5, x + (xf >> 3) - 1:x + (xf >> 3) + 5].astype(np.int64) << 4) - 8192
                    fr[1:5, 1:5] = PR.luma_pred(oracle, arr, y, x, 4, 4, xf, yf, False, 10, 0)
                    raw = m.dmx * ((fr[1:5, 2:6] >> 6) - (fr[1:5, 0:4] >> 6)) + m.dmy * ((fr[2:6, 1:5] >> 6) - (fr[0:4, 1:5] >> 6))
                    hit = hit or raw.max() > 8191 or raw.min() < -8192
            hit_di += int(hit)
    assert hit_dmv >= 10 and hit_di >= 3, (hit_dmv, hit_di)
