"""Inputs shared by the CPU and GPU tiers of the extension forms of the prediction list (BDOF, DMVR's padded reference): reference planes and the lists of items.
Everything here is numpy; the GPU tier uploads the planes.  Expected values: tests/bdof_ref.py."""
import numpy as np

import bdof_ref as BR

LW, LH, LM = 160, 160, 4          # luma planes: visible size incl. margin LM on every side (+ one spare row: the 16-byte rule of the window fetch)
CW, CH, CM = 96, 96, 2            # chroma planes
BDOF_SIZES = [(w, h) for w in (8, 16, 32, 64, 128) for h in (8, 16, 32, 64, 128) if BR.bdof_applies(w, h)]
DMVR_SHAPES = [(8, 8), (16, 8), (8, 16), (16, 16)]

PRED_ITEM_DTYPE = np.dtype([("dst_off", "<i4"), ("org_off", "<i4"), ("ref_off", "<i4", (2,)), ("frac", "<i2", (2, 2)), ("width", "<i2"), ("height", "<i2"),
                            ("ref_plane", "i1", (2,)), ("chroma", "u1"), ("alt_hpel", "u1")])
PRED_EXT_DTYPE = np.dtype([("flags", "u1"), ("pad_dx", "i1", (2,)), ("pad_dy", "i1", (2,)), ("rsv", "u1", (3,))])


def _picture(rng, h, w, bd, shift=0.0):
    yy, xx = np.mgrid[0:h, 0:w]
    top = (1 << bd) - 1
    return np.clip(top / 2 + top / 4 * np.sin((xx + shift) / 6.0) * np.cos((yy - shift) / 5.0) + rng.normal(0, top / 25, (h, w)), 0, top).astype(np.int16)


def planes(bd, seed):
    """0, 1 luma (1 = the content of 0 displaced by a fraction of a sample plus its own noise: an optical flow for BDOF to find); 2, 3 chroma; 4 all zero; 5 all max;
    then the original plane"""
    rng = np.random.default_rng(seed)
    top = (1 << bd) - 1
    p = [_picture(rng, LH + 1, LW, bd, 0.0), _picture(rng, LH + 1, LW, bd, 0.7), _picture(rng, CH + 1, CW, bd, 1.0), _picture(rng, CH + 1, CW, bd, 1.4),
         np.zeros((LH + 1, LW), np.int16), np.full((LH + 1, LW), top, np.int16)]
    org = np.clip(p[0].astype(np.int32) + rng.integers(-12, 13, p[0].shape), 0, top).astype(np.int16)
    return p, org


def limits(plane, w, h, chroma):
    """inclusive range of integer block positions that keep the taps inside the plane's margin"""
    H, W = plane.shape
    m = CM if chroma else LM
    return m, W - w - m, m, H - 1 - h - m


def _place(rng, plane, w, h, chroma, k):
    x0, x1, y0, y1 = limits(plane, w, h, chroma)
    if k % 4 == 0:          # every fourth position touches the margin: one of the four corners of the allowed range
        c = (k // 4) % 4
        return (x0 if c & 1 == 0 else x1), (y0 if c & 2 == 0 else y1)
    return int(rng.integers(x0, x1 + 1)), int(rng.integers(y0, y1 + 1))


class ListBuilder:
    def __init__(self, pl, seed):
        self.pl, self.rng, self.items, self.ext, self.pos = pl, np.random.default_rng(seed), [], [], []

    def add(self, w, h, chroma, alt, fr, rp, flags=0, delta=None, xy=None):
        """xy[l]: the START position (the refined one is start + delta); None: placed inside the margins, every fourth at their limit"""
        it, e = np.zeros((), PRED_ITEM_DTYPE), np.zeros((), PRED_EXT_DTYPE)
        it["width"], it["height"], it["chroma"], it["alt_hpel"], e["flags"] = w, h, chroma, alt, flags
        p = [None, None]
        for l in (0, 1):
            it["ref_plane"][l] = rp[l]
            if rp[l] < 0:
                continue
            x, y = xy[l] if xy is not None else _place(self.rng, self.pl[rp[l]], w, h, chroma, len(self.items) + l)
            if delta is not None:
                e["pad_dx"][l], e["pad_dy"][l] = delta[l]
                x, y = x + delta[l][0], y + delta[l][1]
            p[l] = (x, y)
            it["ref_off"][l] = y * self.pl[rp[l]].shape[1] + x
            it["frac"][l] = fr[l]
        self.items.append(it); self.ext.append(e); self.pos.append(p)

    def done(self):
        return np.array(self.items, PRED_ITEM_DTYPE), np.array(self.ext, PRED_EXT_DTYPE), self.pos


def bdof_list(pl, seed, flags=BR.EXT_BDOF):
    """BDOF items: every luma size 8..128 x 8..128 that passes the size rule, all 16 x 16 phases of list 0 across the list, the alternative half-sample filter,
    every fourth position at the margin limit, the all-zero and all-max planes, identical references in both lists"""
    b = ListBuilder(pl, seed)
    rng, phase = b.rng, 0
    for (w, h) in BDOF_SIZES:
        for k in range(11):
            f0 = (phase % 16, phase // 16 % 16)
            phase += 1
            a = int(rng.integers(0, 2))
            b.add(w, h, 0, 0, (f0, (int(rng.integers(0, 16)), int(rng.integers(0, 16)))), (a, 1 - a), flags)
        for k in range(2):          # IMV_HPEL
            b.add(w, h, 0, 1, ((8 * (k & 1), 8), (8, 8 * ((k + 1) & 1))), (k, 1 - k), flags)
        x, y = _place(rng, pl[0], w, h, 0, 1)
        fr = (int(rng.integers(0, 16)), int(rng.integers(0, 16)))
        b.add(w, h, 0, 0, (fr, fr), (0, 0), flags, xy=[(x, y), (x, y)])          # identical references: every difference is zero
        b.add(w, h, 0, 0, ((0, 0), (0, 0)), (0, 1), flags)                      # no fraction at all: the copy path under the ring
    assert phase >= 256
    for (w, h) in ((16, 16), (16, 8), (8, 16), (64, 32)):
        for rp in ((4, 4), (5, 5), (4, 5), (5, 0), (1, 4)):                     # saturated planes: the clip and the int16 cast of the output
            b.add(w, h, 0, 0, ((int(rng.integers(0, 16)), int(rng.integers(0, 16))), (int(rng.integers(0, 16)), int(rng.integers(0, 16)))), rp, flags)
    return b.done()


def dmvr_list(pl, seed):
    """DMVR sub-blocks: all 25 integer deltas x the four sub-block shapes, luma with and without BDOF, and their 4:2:0 chroma blocks (9 deltas); list 1 mirrors list 0
    or moves on its own (8x8 fails BDOF's size rule, so both of its items go without: with the flag it is an argument error); every fourth START position at the margin limit (the clamp window touches the plane margin)"""
    b = ListBuilder(pl, seed)
    rng = b.rng
    for (w, h) in DMVR_SHAPES:
        for dy in range(-2, 3):
            for dx in range(-2, 3):
                for bdof in (0, 1):
                    d1 = (-dx, -dy) if (dx + dy + bdof) % 2 == 0 else (int(rng.integers(-2, 3)), int(rng.integers(-2, 3)))
                    fr = tuple((int(rng.integers(0, 16)), int(rng.integers(0, 16))) for _ in (0, 1))
                    if (dx, dy) == (2, 2):
                        fr = ((0, 5), (9, 0))          # a zero fraction beside a non-zero one
                    b.add(w, h, 0, int(dx == 1 and dy == 0), fr if not (dx == 1 and dy == 0) else ((8, 8), (8, 0)), (0, 1),
                          BR.EXT_DMVR_PAD | (BR.EXT_BDOF if bdof and BR.bdof_applies(w, h) else 0), ((dx, dy), d1))
        for dy in range(-1, 2):
            for dx in range(-1, 2):
                for k in range(2):
                    d1 = (-dx, -dy) if k == 0 else (int(rng.integers(-1, 2)), int(rng.integers(-1, 2)))
                    fr = tuple((int(rng.integers(0, 32)), int(rng.integers(0, 32))) for _ in (0, 1))
                    b.add(w // 2, h // 2, 1, 0, fr, (2, 3), BR.EXT_DMVR_PAD, ((dx, dy), d1))
    b.add(16, 16, 0, 0, ((3, 7), (0, 0)), (0, -1), BR.EXT_DMVR_PAD, ((2, -1), (0, 0)))          # one list only through the clamp window
    b.add(8, 8, 1, 0, ((0, 0), (30, 1)), (-1, 3), BR.EXT_DMVR_PAD, ((0, 0), (-1, 1)))
    return b.done()


def mixed_list(pl, seed):
    """one launch of everything: BDOF items, DMVR items, plain bi-predicted, uni-predicted and chroma items"""
    b = ListBuilder(pl, seed)
    rng = b.rng
    f = lambda n: (int(rng.integers(0, n)), int(rng.integers(0, n)))
    for (w, h) in ((8, 16), (16, 8), (16, 16), (32, 16), (64, 64), (128, 8)):
        b.add(w, h, 0, 0, (f(16), f(16)), (0, 1), BR.EXT_BDOF)
        b.add(w, h, 0, 0, (f(16), f(16)), (1, 0), 0)
        b.add(w, h, 0, 0, (f(16), f(16)), (0, -1), 0)
        b.add(w // 2, h // 2, 1, 0, (f(32), f(32)), (2, 3), 0)
        b.add(w // 2, h // 2, 1, 0, (f(32), f(32)), (-1, 3), 0)
    for (w, h) in ((4, 4), (4, 8), (8, 4), (8, 8)):          # sizes BDOF never applies to, in the same launch
        b.add(w, h, 0, 0, (f(16), f(16)), (0, 1), 0)
    for (w, h) in DMVR_SHAPES:
        b.add(w, h, 0, 0, (f(16), f(16)), (0, 1), BR.EXT_DMVR_PAD | (BR.EXT_BDOF if BR.bdof_applies(w, h) else 0), ((1, -2), (-1, 2)))
        b.add(w, h, 0, 0, (f(16), f(16)), (0, 1), BR.EXT_DMVR_PAD, ((-2, 1), (2, -1)))
        b.add(w // 2, h // 2, 1, 0, (f(32), f(32)), (2, 3), BR.EXT_DMVR_PAD, ((1, 0), (-1, 0)))
    return b.done()


def unit_shape(it):
    return min(int(it["width"]), 16), min(int(it["height"]), 16)


def compact_offsets(items):
    sizes = items["width"].astype(np.int64) * items["height"]
    off = np.concatenate([[0], np.cumsum(sizes)[:-1]])
    return off.astype(np.int32), int(sizes.sum())
