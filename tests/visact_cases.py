"""Seeded pictures and area lists for the visual-activity entry, shared by the fixture generator (tests/visact_golden_gen.py), the CPU tier (tests/test_visact_cpu.py), the
GPU tier (tests/test_gpu_visact.py, tests/test_gpu_visact_shim.py), smoke() and tools/visact_time.py.

A Picture is a plane table: per row ( cur, prev1, prev2 ) — prev1 may BE cur (the first picture of a sequence: the reference's pS0 == pSM1 bypass).  A Case is an area list on
a picture.  The cases are the smallest at which the kernel can still go wrong:
  one<bd>            the one-position areas, 3 x 3 (HD) and 6 x 6 (ds, at even and odd origins), orders 0, 1, 2
  p72_<bd>_<f><o>    a 72 x 40 4:2:0 picture, CTU 32, through the picture list: the last CTU column 8 wide, the last row 8 high, the first row and column without guard
  p72x_10_ds<o>      the same 4:4:4, where the chroma planes take the ds form too
  p264_10_<f><o>     a 264 x 136 4:2:0 picture, CTU 128: filter areas of 130 / 132 samples — more than one tile across and down, the last tile a sliver
  mix10              one call, shuffled: whole planes next to CTU-sized areas, overlapping; ds areas at odd x and odd y origins; sizes that are no multiple of the tile (64 x 32
                     positions) or of the wave; a table row whose prev1 is cur
  ext<bd>            two-level planes at 0 and 2^bd - 1: a checkerboard with prev1 in antiphase and prev2 in phase, and a checkerboard of 2 x 2 blocks (what the ds form sees)
                     with prev1 in antiphase and prev2 in vertical stripes; at 12 bits 1024 x 1024, where the whole-plane totals exceed 2^32
LAYOUTS    per pointer ( base offset in samples, extra pitch ) the GPU tier hands the planes over with: stride > width, another stride per pointer."""
import numpy as np

import visact_ref as VR

LAYOUTS = (((0, 0), (0, 0), (0, 0)), ((1, 3), (2, 9), (0, 1)), ((3, 5), (0, 0), (5, 14)))


class Picture:
    def __init__(self, name, bit_depth, rows):
        self.name, self.bit_depth, self.rows = name, bit_depth, rows      # rows: [ ( cur, prev1, prev2 ) ], int16 arrays or None; prev1 may be the cur object

    def same(self, r):
        return self.rows[r][1] is self.rows[r][0]


class Case:
    def __init__(self, name, picture, areas):
        self.name, self.picture, self.areas = name, picture, areas


def natural(rng, w, h, bd):
    """a smooth level with light noise, flat regions at both ends of the range, and two previous originals a little apart"""
    top = (1 << bd) - 1
    yy, xx = np.mgrid[0:h, 0:w]
    lvl = top * (0.5 + 0.45 * np.sin(xx / 17.0 + 0.3) * np.cos(yy / 11.0))
    cur = np.clip(lvl + rng.integers(-(top >> 6) - 1, (top >> 6) + 2, (h, w)), 0, top)
    cur[: h // 5, : w // 4] = 0
    cur[h - h // 6:, w - w // 3:] = top
    cur = cur.astype(np.int16)
    p1 = np.clip(np.roll(cur, 1, 1).astype(np.int32) + rng.integers(-2, 3, (h, w)), 0, top).astype(np.int16)
    p2 = np.clip(np.roll(p1, 1, 0).astype(np.int32) + rng.integers(-3, 4, (h, w)), 0, top).astype(np.int16)
    return cur, p1, p2


def _two_level(w, h, bd, blocks):
    top = (1 << bd) - 1
    yy, xx = np.mgrid[0:h, 0:w]
    s = 1 if blocks else 0
    chk = ((((xx >> s) + (yy >> s)) & 1) * top).astype(np.int16)
    anti = (top - chk).astype(np.int16)
    third = ((((xx >> 1) & 1) * top).astype(np.int16)) if blocks else chk.copy()
    return chk, anti, third


_cache = {}


def pictures():
    if "p" in _cache:
        return _cache["p"]
    out = {}
    for bd in (8, 10, 12):
        rng = np.random.default_rng(7300 + bd)
        out["one%d" % bd] = Picture("one%d" % bd, bd, [tuple(rng.integers(0, 1 << bd, (11, 12)).astype(np.int16) for _ in range(3))])
        out["p72_%d" % bd] = Picture("p72_%d" % bd, bd, [natural(rng, 72 >> s, 40 >> s, bd) for s in (0, 1, 1)])
        n = 1024 if bd == 12 else 256
        out["ext%d" % bd] = Picture("ext%d" % bd, bd, [_two_level(n, n, bd, False), _two_level(n, n, bd, True)])
    rng = np.random.default_rng(7399)
    out["p72x_10"] = Picture("p72x_10", 10, [natural(rng, 72, 40, 10) for _ in range(3)])
    out["p264_10"] = Picture("p264_10", 10, [natural(rng, 264 >> s, 136 >> s, 10) for s in (0, 1, 1)])
    cur, p1, p2 = natural(rng, 150, 84, 10)
    out["mix10"] = Picture("mix10", 10, [(cur, p1, p2), (cur, cur, p2)])
    _cache["p"] = out
    return out


def sizes(pic):
    return [(r[0].shape[1], r[0].shape[0]) for r in pic.rows]


def cases():
    if "c" in _cache:
        return _cache["c"]
    P, out = pictures(), {}

    def add(name, pic, areas):
        out[name] = Case(name, P[pic], np.array(areas, VR.AREA_DTYPE))

    for bd in (8, 10, 12):
        a = []
        for o in (0, 1, 2):
            a += [VR.area(0, 0, o, 4, 5, 3, 3, (5, 6, 1, 1)), VR.area(0, 1, o, 2, 4, 6, 6, (2, 4, 6, 6)), VR.area(0, 1, o, 1, 1, 6, 6), VR.area(0, 1, o, 5, 2, 6, 6), VR.area(0, 1, o, 6, 5, 6, 6)]
        add("one%d" % bd, "one%d" % bd, a)
        for f in (0, 1):
            for o in (0, 1, 2):
                add("p72_%d_%s%d" % (bd, "ds" if f else "hd", o), "p72_%d" % bd, VR.picture_areas(sizes(P["p72_%d" % bd]), 32, bool(f), o, "420"))
        n = 1024 if bd == 12 else 256
        a = [VR.area(r, f, o, 0, 0, n, n, (0, 0, n, n)) for r in (0, 1) for f in (0, 1) for o in (1, 2)]
        a += [VR.area(1, 1, 2, 121, 61, 132, 70, (122, 64, 128, 64)), VR.area(0, 0, 1, 63, 0, 130, 129, (64, 0, 128, 128))]
        add("ext%d" % bd, "ext%d" % bd, a)
    for o in (1, 2):
        add("p72x_10_ds%d" % o, "p72x_10", VR.picture_areas(sizes(P["p72x_10"]), 32, True, o, "444"))
    for f in (0, 1):
        for o in (0, 1, 2):
            add("p264_10_%s%d" % ("ds" if f else "hd", o), "p264_10", VR.picture_areas(sizes(P["p264_10"]), 128, bool(f), o, "420"))
    a = [VR.area(0, 0, 1, 0, 0, 150, 84, (0, 0, 150, 84)), VR.area(0, 1, 2, 0, 0, 150, 84, (3, 1, 147, 83)), VR.area(0, 0, 2, 3, 2, 67, 35, (4, 3, 64, 32)),
         VR.area(0, 0, 1, 10, 7, 131, 70), VR.area(0, 1, 1, 1, 3, 134, 70, (1, 3, 65, 33)), VR.area(0, 1, 2, 4, 1, 140, 78, (70, 40, 1, 44)), VR.area(0, 1, 0, 7, 9, 136, 72),
         VR.area(0, 0, 0, 80, 40, 66, 34, (81, 41, 64, 32)), VR.area(0, 0, 1, 80, 40, 67, 35), VR.area(0, 1, 1, 16, 14, 36, 36, (18, 16, 32, 32)), VR.area(0, 1, 1, 15, 14, 36, 36, (18, 16, 32, 32)),
         VR.area(1, 0, 1, 0, 0, 150, 84), VR.area(1, 0, 2, 5, 5, 100, 50, (0, 0, 150, 84)), VR.area(1, 1, 1, 3, 3, 70, 40), VR.area(1, 1, 2, 2, 1, 148, 82, (2, 1, 148, 82))]
    order = np.random.default_rng(7311).permutation(len(a))
    add("mix10", "mix10", [a[i] for i in order])
    _cache["c"] = out
    return out


def expected(case):
    """-> ( records uint64 [n][4], double bit patterns uint64 [n][3], uint32 [n][4] = spatAct, tempAct, minAct, visAct, int64 [n] = getAvg of the mean rectangle, -1: none ) of the model"""
    pic = case.picture
    rec = VR.records(pic.rows, case.areas)
    bits, ints, avg = [], [], []
    for a, r in zip(case.areas, rec):
        va = VR.vis_act(r, int(a["w"]), int(a["h"]), pic.bit_depth, int(a["ds"]), int(a["order"]), pic.same(int(a["plane"])))
        bits.append(va.bits()); ints.append(va.ints())
        avg.append(VR.get_avg(int(r[2]), int(a["mw"]), int(a["mh"])) if a["mw"] > 0 else -1)
    return rec, np.array(bits, np.uint64), np.array(ints, np.uint32), np.array(avg, np.int64)
