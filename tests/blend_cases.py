"""Inputs shared by the CPU and GPU tiers of the blend forms of the prediction list (BCW, GEO): reference planes and the lists of items.
Everything here is numpy; the GPU tier uploads the planes.  Expected values: tests/blend_ref.py (and tests/bdof_ref.py for the extension items of the mixed list)."""
import numpy as np

import bdof_cases as BC
import bdof_ref as BR
import blend_ref as BL

PRED_ITEM_DTYPE, PRED_EXT_DTYPE, PRED_BLEND_DTYPE = BC.PRED_ITEM_DTYPE, BC.PRED_EXT_DTYPE, BL.PRED_BLEND_DTYPE
LW, LH = 192, 160          # luma planes (+ one spare row: the 16-byte rule of the window fetch); margins as bdof_cases: 4 luma, 2 chroma
CW, CH = 96, 96            # chroma planes
BCW_LUMA = [(4, 4), (4, 64), (8, 8), (16, 16), (64, 16), (128, 128)]          # one size from each kernel form and tile rule
BCW_CHROMA = [(2, 2), (2, 8), (4, 4), (8, 4), (64, 64)]
GEO_8BIT = [(8, 8), (8, 32), (32, 8), (64, 64)]


def checker(h, w, bd, phase):
    """0 / max in 2 x 2 cells: at a half-sample fraction the taps overshoot on both sides of every edge"""
    yy, xx = np.mgrid[0:h, 0:w]
    return ((((xx >> 1) + (yy >> 1) + phase) & 1) * ((1 << bd) - 1)).astype(np.int16)


def planes(bd, seed):
    """0, 1 luma pictures; 2, 3 chroma pictures; 4, 5 luma checkerboards 0 / max and max / 0; 6, 7 the same for chroma; then the original plane (luma size)"""
    rng = np.random.default_rng(seed)
    top = (1 << bd) - 1
    p = [BC._picture(rng, LH + 1, LW, bd, 0.0), BC._picture(rng, LH + 1, LW, bd, 2.3), BC._picture(rng, CH + 1, CW, bd, 1.0), BC._picture(rng, CH + 1, CW, bd, 3.1),
         checker(LH + 1, LW, bd, 0), checker(LH + 1, LW, bd, 1), checker(CH + 1, CW, bd, 0), checker(CH + 1, CW, bd, 1)]
    org = np.clip(p[0].astype(np.int32) + rng.integers(-12, 13, p[0].shape), 0, top).astype(np.int16)
    return p, org


class Builder(BC.ListBuilder):
    """bdof_cases.ListBuilder with a blend record per item"""

    def __init__(self, pl, seed):
        super().__init__(pl, seed)
        self.blend = []

    def add(self, w, h, chroma, alt, fr, rp, mode=0, param=0, flags=0, delta=None, xy=None):
        super().add(w, h, chroma, alt, fr, rp, flags, delta, xy)
        b = np.zeros((), PRED_BLEND_DTYPE)
        b["mode"], b["param"] = mode, param
        self.blend.append(b)

    def frac(self, chroma, k):
        """seeded fractions of both hypotheses -> ( fr, alt_hpel ); every eighth item: no fraction at all in hypothesis 0, a zero x, a zero y, phase 8 with alt_hpel (luma)"""
        n = 32 if chroma else 16
        r = lambda: (int(self.rng.integers(0, n)), int(self.rng.integers(0, n)))
        f0, f1, alt = r(), r(), 0
        if k % 8 == 0:
            f0 = (0, 0)
        elif k % 8 == 1:
            f0, f1 = (0, f0[1] | 1), (f1[0] | 1, 0)
        elif k % 8 == 2:
            f0, f1 = (f0[0] | 1, 0), (0, 0)
        elif k % 8 == 3 and not chroma:
            f0, f1, alt = (8, 8), (8, f1[1]), 1
        return (f0, f1), alt

    def done(self):
        items, ext, pos = super().done()
        return items, ext, np.array(self.blend, PRED_BLEND_DTYPE), pos


def geo_list(pl, seed, sizes=BL.GEO_SIZES):
    """every split direction x the given CU sizes, each CU as its luma block and its chroma block; hypotheses from two planes, swapped, or one plane twice"""
    b = Builder(pl, seed)
    k = 0
    for (w, h) in sizes:
        for sd in range(64):
            rp = ((0, 1), (1, 0), (0, 0))[k % 3]
            fr, alt = b.frac(0, k)
            b.add(w, h, 0, alt, fr, rp, BL.BLEND_GEO, sd)
            fr, _ = b.frac(1, k + 5)
            b.add(w // 2, h // 2, 1, 0, fr, tuple(2 + r for r in rp), BL.BLEND_GEO, sd)
            k += 1
    return b.done()


def bcw_list(pl, seed):
    """the five indices on one size from each kernel form and tile rule, luma and chroma; hypotheses alternate between two planes and one plane twice"""
    b = Builder(pl, seed)
    k = 0
    for chroma, sizes in ((0, BCW_LUMA), (1, BCW_CHROMA)):
        for (w, h) in sizes:
            for idx in range(5):
                for rp in ((0, 1), (1, 1)):
                    fr, alt = b.frac(chroma, k)
                    b.add(w, h, chroma, alt, fr, tuple(2 * chroma + r for r in rp), BL.BLEND_BCW, idx)
                    k += 1
    return b.done()


def extremes_list(pl, seed):
    """the checkerboard planes (0 / max against max / 0) at half-sample and other fractions: BCW 0 and 4 (weights -2 / 10) and GEO directions whose edge runs through the block"""
    b = Builder(pl, seed)
    for chroma in (0, 1):
        half = 16 if chroma else 8
        rp = (6, 7) if chroma else (4, 5)
        sizes = ((4, 4), (16, 16), (32, 32)) if chroma else ((8, 8), (32, 32), (64, 64))
        for (w, h) in sizes:
            for fr in (((half, half), (half, half)), ((half, 0), (0, half)), ((half, half), (0, 0)), ((3, half), (half, 5))):
                for idx in (0, 4):
                    b.add(w, h, chroma, 0, fr, rp, BL.BLEND_BCW, idx)
                    b.add(w, h, chroma, 0, fr, rp[::-1], BL.BLEND_BCW, idx)
                for sd in (0, 10, 23, 36, 52):
                    b.add(w, h, chroma, 0, fr, rp, BL.BLEND_GEO, sd)
    return b.done()


def mixed_list(pl, seed):
    """one launch of everything: plain uni / bi, BDOF, DMVR's padded reference, BCW and GEO items, luma and chroma"""
    b = Builder(pl, seed)
    rng = b.rng
    f = lambda n: (int(rng.integers(0, n)), int(rng.integers(0, n)))
    for (w, h) in ((8, 8), (16, 8), (16, 16), (32, 16), (64, 64), (8, 64)):
        b.add(w, h, 0, 0, (f(16), f(16)), (0, 1))
        b.add(w, h, 0, 0, (f(16), f(16)), (0, -1))
        b.add(w // 2, h // 2, 1, 0, (f(32), f(32)), (2, 3))
        if BR.bdof_applies(w, h):
            b.add(w, h, 0, 0, (f(16), f(16)), (0, 1), flags=BR.EXT_BDOF)
        b.add(w, h, 0, 0, (f(16), f(16)), (1, 0), BL.BLEND_BCW, int(rng.integers(0, 5)))
        b.add(w // 2, h // 2, 1, 0, (f(32), f(32)), (3, 2), BL.BLEND_BCW, int(rng.integers(0, 5)))
        sd = int(rng.integers(0, 64))
        b.add(w, h, 0, 0, (f(16), f(16)), (0, 1), BL.BLEND_GEO, sd)
        b.add(w // 2, h // 2, 1, 0, (f(32), f(32)), (2, 3), BL.BLEND_GEO, sd)
    for (w, h) in BC.DMVR_SHAPES:
        b.add(w, h, 0, 0, (f(16), f(16)), (0, 1), flags=BR.EXT_DMVR_PAD | (BR.EXT_BDOF if BR.bdof_applies(w, h) else 0), delta=((1, -2), (-1, 2)))
        b.add(w // 2, h // 2, 1, 0, (f(32), f(32)), (2, 3), flags=BR.EXT_DMVR_PAD, delta=((1, 0), (-1, 0)))
    for (w, h) in ((4, 4), (4, 16), (128, 32)):          # BCW on sizes GEO never has
        b.add(w, h, 0, 0, (f(16), f(16)), (0, 1), BL.BLEND_BCW, 4 * int(rng.integers(0, 2)))
    return b.done()


def expected(lib, pl, pos, it, e, bl, bd):
    """one item of a list with extension and blend records"""
    if int(bl["mode"]) != BL.BLEND_DEFAULT:
        return BL.expected_block_blend(lib, pl, pos, it, bl, bd)
    return BR.expected_block_ex(lib, pl, pos, it, e, bd)


def check_margins(pl, items, ext, pos):
    """every hypothesis keeps the entry's margins: 4 (luma) / 2 (chroma) samples round the block — for a DMVR item round its START position — and the spare last row"""
    for it, e, p in zip(items, ext, pos):
        w, h, chroma = int(it["width"]), int(it["height"]), int(it["chroma"])
        for l in (0, 1):
            if int(it["ref_plane"][l]) < 0:
                continue
            plane = pl[int(it["ref_plane"][l])]
            x0, x1, y0, y1 = BC.limits(plane, w, h, chroma)
            x, y = p[l][0] - int(e["pad_dx"][l]), p[l][1] - int(e["pad_dy"][l])
            assert x0 <= x <= x1 and y0 <= y <= y1, (it, l, (x, y))
            assert int(it["ref_off"][l]) == p[l][1] * plane.shape[1] + p[l][0]
            assert plane.shape[0] * plane.shape[1] <= 256 * 192


def check_no_overlap(items, total, pitch=0):
    """the items' outputs are disjoint inside a buffer of `total` samples (compact blocks, or blocks in a plane of row pitch `pitch`)"""
    used = np.zeros(total, np.int32)
    for it in items:
        w, h, o = int(it["width"]), int(it["height"]), int(it["dst_off"])
        rows = o + np.arange(h)[:, None] * (pitch if pitch else w) + np.arange(w)[None, :]
        assert rows.min() >= 0 and rows.max() < total
        used[rows.reshape(-1)] += 1
    assert used.max() <= 1
    return int(used.sum())


compact_offsets = BC.compact_offsets
