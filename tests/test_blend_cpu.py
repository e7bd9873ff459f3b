"""CPU tier of the blend forms of the prediction list (vvhip_pred_inter_batch_blend: BCW weights, GEO partitions): the ABI, the ROM accessor, and the expected values
the GPU tier uses (tests/blend_ref.py), pinned before any GPU is involved.

tests/golden/blend.npz holds what the reference's own xWeightedGeoBlk and addWeightedAvg returned, on their scalar row and on their x86 row (tests/blend_golden_gen.cpp):
all 2048 GEO weight blocks and 60 blend cases on real 14-bit intermediates.  The model must reproduce every sample, and so must the library's weight accessor — which
evaluates the clamped line the kernel evaluates, not the masks the model reads.  The lists the GPU tier runs are checked here for the entry's margins and for
disjoint outputs, and for being lists on which ignoring the blend record gives other values."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import blend_cases as BLC  # noqa: E402
import blend_golden_gen as GEN  # noqa: E402
import blend_ref as BL  # noqa: E402
import pred_ref as PR  # noqa: E402


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(ROOT, "tests", "golden", "blend.npz"))


def _cases(z):
    return [dict(hdr=[int(v) for v in z["c%03d_hdr" % i]], s0=z["c%03d_s0" % i], s1=z["c%03d_s1" % i], scalar=z["c%03d_scalar" % i], simd=z["c%03d_simd" % i])
            for i in range(int(z["n"]))]


def _lib():
    from vvenc_amd.lib import LIB_PATH
    return C.CDLL(LIB_PATH)


def test_blend_symbols_prototypes_and_header():
    from vvenc_amd.lib import PROTOTYPES
    lib = _lib()
    for name in ("vvhip_pred_inter_batch_blend", "vvhip_get_geo_weights_host"):
        assert hasattr(lib, name), "missing export " + name
    assert len(PROTOTYPES["vvhip_pred_inter_batch_blend"][1]) == 13 and len(PROTOTYPES["vvhip_pred_inter_batch_ex"][1]) == 12 and len(PROTOTYPES["vvhip_get_geo_weights_host"][1]) == 5
    hdr = open(os.path.join(ROOT, "include", "vvenc_hip.h")).read()
    for word in ("vvhip_pred_inter_batch_blend", "vvhip_get_geo_weights_host", "VVHIP_PRED_BLEND_DEFAULT", "VVHIP_PRED_BLEND_BCW", "VVHIP_PRED_BLEND_GEO"):
        assert word in hdr


def test_pred_blend_layout(tmp_path):
    """vvhip_pred_blend as the C compiler lays it out == the numpy record the Python layer fills: 4 bytes; the item and the extension keep their sizes"""
    from vvenc_amd.hotpath import PRED_BLEND_BCW, PRED_BLEND_DEFAULT, PRED_BLEND_DTYPE, PRED_BLEND_GEO, PRED_EXT_DTYPE, PRED_ITEM_DTYPE
    fields = ["mode", "param", "rsv"]
    src = tmp_path / "layout.cpp"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "vvenc_hip.h"\nint main(void){ printf("%zu %zu %zu %d %d %d", sizeof(vvhip_pred_item), sizeof(vvhip_pred_ext), '
                   'sizeof(vvhip_pred_blend), VVHIP_PRED_BLEND_DEFAULT, VVHIP_PRED_BLEND_BCW, VVHIP_PRED_BLEND_GEO);\n'
                   + "".join('printf(" %%zu", offsetof(vvhip_pred_blend, %s));\n' % f for f in fields) + "return 0; }\n")
    exe = tmp_path / "layout"
    subprocess.check_call(["g++", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    assert got == [32, 8, 4, 0, 1, 2, 0, 1, 2], got
    assert PRED_BLEND_DTYPE.itemsize == 4 and PRED_ITEM_DTYPE.itemsize == 32 and PRED_EXT_DTYPE.itemsize == 8
    assert (PRED_BLEND_DEFAULT, PRED_BLEND_BCW, PRED_BLEND_GEO) == (0, 1, 2) == (BL.BLEND_DEFAULT, BL.BLEND_BCW, BL.BLEND_GEO)
    assert [PRED_BLEND_DTYPE.fields[f][1] for f in fields] == got[6:] and PRED_BLEND_DTYPE == BL.PRED_BLEND_DTYPE


def test_golden_covers_what_it_must(golden):
    """both tools, bit depths 8 and 10, luma and chroma; BCW -2 / 10 on inputs beyond the sample range; outputs at both clip ends; all 2048 weight blocks"""
    cases = _cases(golden)
    assert len(cases) >= 56
    assert {(c["hdr"][0], c["hdr"][1], c["hdr"][4]) for c in cases} == {(k, bd, ch) for k in (1, 2) for bd in (8, 10) for ch in (0, 1)}
    assert golden["weights_scalar"].size == 1152000 == sum((w >> c) * (h >> c) for (_, w, h, c) in GEN.weight_blocks()) and len(GEN.weight_blocks()) == 2048
    for bd in (8, 10):
        hr, top = max(2, 14 - bd), (1 << bd) - 1
        mine = [c for c in cases if c["hdr"][1] == bd]
        over = [c for c in mine if c["hdr"][0] == 1 and c["hdr"][5] in (0, 4) and (min(c["s0"].min(), c["s1"].min()) < -8192 or max(c["s0"].max(), c["s1"].max()) > (top << hr) - 8192)]
        assert over, "no BCW -2 / 10 case on an overshooting intermediate"
        assert any((c["scalar"] == 0).any() for c in mine) and any((c["scalar"] == top).any() for c in mine)
        assert all(c["scalar"].min() >= 0 and c["scalar"].max() <= top for c in mine)


def test_golden_rows_agree(golden):
    assert np.array_equal(golden["weights_scalar"], golden["weights_simd"])
    for i, c in enumerate(_cases(golden)):
        assert np.array_equal(c["scalar"], c["simd"]), "case %d: the reference's scalar row and x86 row differ" % i


def test_model_weights_equal_golden(golden):
    """blend_ref.geo_weights == the weight block the reference function returned, all 64 x 16 x 2, on both rows"""
    for row in ("weights_scalar", "weights_simd"):
        at, ref = 0, golden[row]
        for (sd, w, h, c) in GEN.weight_blocks():
            m = BL.geo_weights(sd, w, h, c)
            assert m.shape == (h >> c, w >> c) and np.array_equal(m.reshape(-1), ref[at:at + m.size]), (row, sd, w, h, c)
            at += m.size
        assert at == ref.size


def test_model_blend_equals_golden(golden):
    for i, c in enumerate(_cases(golden)):
        kind, bd, w, h, ch, param = c["hdr"]
        got = BL.blend(c["s0"], c["s1"], kind, param, bd, ch)
        assert got.dtype == np.int16 and got.shape == (h, w)
        assert np.array_equal(got, c["scalar"]) and np.array_equal(got, c["simd"]), "case %d %s" % (i, c["hdr"])


def test_library_geo_weights_equal_golden(golden):
    """vvhip_get_geo_weights_host — the clamped line of the kernel — == the reference's weight block for all 2048 combinations"""
    lib = _lib()
    assert hasattr(lib, "vvhip_get_geo_weights_host"), "missing export vvhip_get_geo_weights_host"
    at, ref = 0, golden["weights_scalar"]
    for (sd, w, h, c) in GEN.weight_blocks():
        out = np.full((h >> c) * (w >> c) + 8, 99, np.int8)
        assert lib.vvhip_get_geo_weights_host(sd, w.bit_length() - 1, h.bit_length() - 1, c, out.ctypes.data_as(C.c_void_p)) == 0
        n = out.size - 8
        assert np.array_equal(out[:n], ref[at:at + n]), (sd, w, h, c)
        assert np.all(out[n:] == 99)
        at += n
    assert at == ref.size


def test_library_geo_weights_argument_errors():
    lib = _lib()
    out = np.full(64 * 64, 99, np.int8)
    p = out.ctypes.data_as(C.c_void_p)
    for args in ((64, 3, 3, 0), (-1, 3, 3, 0), (0, 2, 3, 0), (0, 3, 2, 0), (0, 7, 3, 0), (0, 3, 7, 0), (0, 3, 3, 2), (0, 3, 3, -1)):
        assert lib.vvhip_get_geo_weights_host(*args, p) == -1, args
    assert lib.vvhip_get_geo_weights_host(0, 3, 3, 0, None) == -1
    assert np.all(out == 99)
    assert lib.vvhip_get_geo_weights_host(63, 6, 6, 0, p) == 0 and out.min() == 0 and out.max() == 8


def test_hotpath_wrapper_is_the_accessor():
    """HotPath.geo_weights needs no device: called unbound on an object that only carries the library"""
    from vvenc_amd.hotpath import HotPath
    holder = type("H", (), dict(L=_lib()))()
    for (sd, w, h, c) in ((0, 8, 8, 0), (17, 64, 16, 1), (63, 32, 64, 0)):
        assert np.array_equal(HotPath.geo_weights(holder, sd, w, h, c), BL.geo_weights(sd, w, h, c))
    with pytest.raises(ValueError):
        HotPath.geo_weights(holder, 64, 8, 8, 0)


def test_bcw_default_index_is_the_default_average():
    """bcw_idx 2 (4 : 4) == addAvg for every pair of 14-bit values the interpolation can produce at the block's corners of the range, and on random ones"""
    rng = np.random.default_rng(3)
    for bd in (8, 10, 12):
        a = rng.integers(-12000, 24000, (64, 64)).astype(np.int16)
        b = rng.integers(-12000, 24000, (64, 64)).astype(np.int16)
        assert np.array_equal(BL.blend(a, b, BL.BLEND_BCW, 2, bd), PR.bi_average(a, b, bd))


def test_share_of_samples_with_a_full_weight(golden):
    """over all luma and chroma blocks: 42.9 % of the samples have weight 8 and 46.8 % weight 0 — 89.7 % together, the share the GPU tier compares with the
    uni-prediction of one hypothesis (its assertion asks for 80 %)"""
    w = golden["weights_scalar"]
    s8, s0 = float((w == 8).mean()), float((w == 0).mean())
    print("weight 8: %.4f, weight 0: %.4f, together %.4f" % (s8, s0, s8 + s0))
    assert abs(s8 - 0.4287) < 1e-3 and abs(s0 - 0.4680) < 1e-3 and s8 + s0 >= 0.8


@pytest.mark.parametrize("bd", [8, 10])
def test_gpu_lists_meet_the_margins_and_do_not_overlap(bd):
    """the lists tests/test_gpu_pred_blend.py runs: margins of every hypothesis, disjoint compact outputs, disjoint outputs in the plane layout of the mixed list"""
    pl, _ = BLC.planes(bd, 100 + bd)
    assert all(p.shape[0] <= 192 and p.shape[1] <= 256 for p in pl)
    lists = [BLC.geo_list(pl, 200 + bd, BL.GEO_SIZES if bd == 10 else BLC.GEO_8BIT), BLC.bcw_list(pl, 300 + bd), BLC.extremes_list(pl, 400 + bd), BLC.mixed_list(pl, 500 + bd)]
    for (items, ext, blend, pos) in lists:
        assert len(items) == len(ext) == len(blend) == len(pos)
        BLC.check_margins(pl, items, ext, pos)
        items = items.copy()
        off, total = BLC.compact_offsets(items)
        items["dst_off"] = off
        assert BLC.check_no_overlap(items, total) == total
    items = lists[3][0].copy()
    where, rows = PR.shelf_pack([(int(i["width"]), int(i["height"])) for i in items], 512)
    items["dst_off"] = [y * 512 + x for (x, y) in where]
    BLC.check_no_overlap(items, rows * 512, 512)


def test_gpu_lists_cover_what_they_must():
    pl, _ = BLC.planes(10, 110)
    items, _, blend, _ = BLC.geo_list(pl, 210)
    assert len(items) == 2048 and np.all(blend["mode"] == BL.BLEND_GEO)
    assert {(int(b["param"]), int(i["width"]) << int(i["chroma"]), int(i["height"]) << int(i["chroma"]), int(i["chroma"])) for i, b in zip(items, blend)} == set(GEN.weight_blocks())
    fr = items["frac"]
    assert (fr[:, 0] == 0).all(axis=1).any() and ((fr[:, 0, 0] == 0) & (fr[:, 0, 1] != 0)).any() and ((fr[:, 0, 0] != 0) & (fr[:, 0, 1] == 0)).any()
    assert ((items["alt_hpel"] == 1) & (fr[:, 0, 0] == 8)).any()
    items, _, blend, _ = BLC.bcw_list(pl, 310)
    got = {(int(i["width"]), int(i["height"]), int(i["chroma"]), int(b["param"])) for i, b in zip(items, blend)}
    assert got == {(w, h, c, k) for c, sizes in ((0, BLC.BCW_LUMA), (1, BLC.BCW_CHROMA)) for (w, h) in sizes for k in range(5)}
    assert {tuple(int(v) for v in i["ref_plane"]) for i in items} == {(0, 1), (1, 1), (2, 3), (3, 3)}
    items, ext, blend, _ = BLC.mixed_list(pl, 510)
    kinds = {(int(b["mode"]), int(e["flags"])) for e, b in zip(ext, blend)}
    assert {(0, 0), (0, 1), (0, 2), (0, 3), (1, 0), (2, 0)} <= kinds and any(int(i["ref_plane"][1]) < 0 for i in items)


@pytest.mark.parametrize("bd", [8, 10])
def test_guard_blend_lists_differ_from_the_default_average(oracle, bd):
    """on the lists of the GPU tier the expected block differs from the default average for every BCW item whose index is not 2, and for most GEO items:
    a kernel that ignores the blend record cannot pass there; the extremes reach both clip ends"""
    pl, _ = BLC.planes(bd, 100 + bd)
    top = (1 << bd) - 1
    items, _, blend, pos = BLC.bcw_list(pl, 300 + bd)
    small = [k for k in range(len(items)) if int(items[k]["width"]) * int(items[k]["height"]) <= 1024 and int(items[k]["width"]) >= 4]
    for k in small:
        same = np.array_equal(BL.expected_block_blend(oracle, pl, pos[k], items[k], blend[k], bd), PR.expected_block(oracle, pl, pos[k], items[k], bd))
        assert same == (int(blend[k]["param"]) == 2), (k, items[k], blend[k])
    items, _, blend, pos = BLC.geo_list(pl, 200 + bd, BLC.GEO_8BIT[:2])
    differs = [not np.array_equal(BL.expected_block_blend(oracle, pl, pos[k], items[k], blend[k], bd), PR.expected_block(oracle, pl, pos[k], items[k], bd)) for k in range(len(items))]
    assert sum(differs) * 10 >= 9 * len(differs), (sum(differs), len(differs))
    items, _, blend, pos = BLC.extremes_list(pl, 400 + bd)
    outs = [BL.expected_block_blend(oracle, pl, pos[k], items[k], blend[k], bd) for k in range(len(items))]
    for mode in (BL.BLEND_BCW, BL.BLEND_GEO):
        for chroma in (0, 1):
            mine = [o for o, i, b in zip(outs, items, blend) if int(b["mode"]) == mode and int(i["chroma"]) == chroma]
            assert any((o == 0).any() for o in mine) and any((o == top).any() for o in mine), (mode, chroma)
    for sd in (0, 10, 23, 36, 52):          # the GEO directions of the extremes: the edge runs through every block size used there
        for (w, h) in ((8, 8), (32, 32), (64, 64)):
            wt = BL.geo_weights(sd, w, h, 0)
            assert (wt == 0).any() and (wt == 8).any() and ((wt > 0) & (wt < 8)).any(), (sd, w, h)
