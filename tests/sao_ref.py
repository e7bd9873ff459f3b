"""numpy restatement of the two data-parallel parts of SAO, per CTU and for a picture:

stats    EncSampleAdaptiveOffset::getBlkStats (EncoderLib/EncSampleAdaptiveOffset.cpp:810-929) with the five calcSaoStatistics*_Core routines
         (CommonLib/SampleAdaptiveOffset.cpp:281-399), driven like getStatistics (:294-344)
offset   offsetBlock_core (CommonLib/SampleAdaptiveOffset.cpp:64-280), driven like offsetCTU (:605-652)

The reference's sign-line buffers are a cache: every counted / filtered sample has edgeType = sgn( c - a ) + sgn( c - b ) for its two neighbours along the type's
direction.  What differs between the types, the two functions and the rows of a CTU is WHICH samples take part; that is written here as boolean masks over the CTU.
Records: int64 [5][2][32] = SAOStatData[5] ({ diff[32], count[32] }), order EO_0, EO_90, EO_135, EO_45, BO, edge classes at edgeType + 2.
tests/golden/sao.npz pins both functions to the reference's own code (tests/sao_golden_gen.*)."""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sao.npz")

# statistics flags of a CTU (VVHIP_SAO_*)
LEFT, ABOVE, ABOVE_LEFT, RIGHT, BELOW, ABOVE_RIGHT = 1, 2, 4, 8, 16, 32
STAT_FLAGS = (LEFT, ABOVE, ABOVE_LEFT, RIGHT, BELOW, ABOVE_RIGHT)
# availability mask of the filter (SampleAdaptiveOffset.h:75-85)
A_LEFT, A_RIGHT, A_ABOVE, A_BELOW, A_ABOVE_LEFT, A_ABOVE_RIGHT, A_BELOW_LEFT, A_BELOW_RIGHT = 1, 2, 4, 8, 16, 32, 64, 128
AVAIL_BITS = (A_LEFT, A_RIGHT, A_ABOVE, A_BELOW, A_ABOVE_LEFT, A_ABOVE_RIGHT, A_BELOW_LEFT, A_BELOW_RIGHT)
# neighbour pairs ( dx, dy ) of EO_0, EO_90, EO_135, EO_45
DIRS = (((-1, 0), (1, 0)), ((0, -1), (0, 1)), ((-1, -1), (1, 1)), ((1, -1), (-1, 1)))
PARAM_DTYPE = np.dtype([("type", "i1"), ("avail", "u1"), ("band", "u1"), ("rsv", "u1"), ("offs", "<i2", (5,))])      # vvhip_sao_param


def max_offset_qval(bit_depth):
    """SampleAdaptiveOffset::getMaxOffsetQVal"""
    return (1 << (min(bit_depth, 10) - 5)) - 1


def grid(width, height, ctu_w, ctu_h):
    return -(-width // ctu_w), -(-height // ctu_h)


def border_flags(gx, gy):
    """what getStatistics derives from the picture's borders alone -> uint8 [gy * gx]"""
    f = np.zeros((gy, gx), np.uint8)
    for cy in range(gy):
        for cx in range(gx):
            L, A, R, B = cx > 0, cy > 0, cx < gx - 1, cy < gy - 1
            f[cy, cx] = LEFT * L | ABOVE * A | ABOVE_LEFT * (L and A) | RIGHT * R | BELOW * B | ABOVE_RIGHT * (A and R)
    return f.reshape(-1)


def border_avail(gx, gy):
    """deriveLoopFilterBoundaryAvailibility with filtering across slices and tiles on: the picture's borders alone -> uint8 [gy * gx]"""
    f = np.zeros((gy, gx), np.uint8)
    for cy in range(gy):
        for cx in range(gx):
            L, A, R, B = cx > 0, cy > 0, cx < gx - 1, cy < gy - 1
            f[cy, cx] = (A_LEFT * L | A_RIGHT * R | A_ABOVE * A | A_BELOW * B | A_ABOVE_LEFT * (L and A) | A_ABOVE_RIGHT * (R and A) | A_BELOW_LEFT * (L and B) | A_BELOW_RIGHT * (R and B))
    return f.reshape(-1)


def _neigh(padded, x0, y0, w, h, dx, dy):
    return padded[y0 + 1 + dy:y0 + 1 + dy + h, x0 + 1 + dx:x0 + 1 + dx + w]


def _edge_types(padded, x0, y0, w, h):
    """-> c ( h x w ) and the four edge-class planes ( edgeType + 2 ); neighbours outside the picture read 0 — no mask below ever selects such a sample"""
    c = _neigh(padded, x0, y0, w, h, 0, 0)
    return c, [np.sign(c - _neigh(padded, x0, y0, w, h, *a)) + np.sign(c - _neigh(padded, x0, y0, w, h, *b)) + 2 for (a, b) in DIRS]


def _span(n, lo, hi):
    k = np.arange(n)
    return (k >= lo) & (k < hi)


def stats_masks(w, h, is_luma, flags):
    """the samples of a w x h CTU that getBlkStats counts, per type -> five boolean h x w masks"""
    L, A, AL, R, B, AR = (bool(flags & f) for f in STAT_FLAGS)
    skip_r, skip_b = (5, 4) if is_luma else (3, 2)
    start_x, end_x, end_x_full = (0 if L else 1), (w - skip_r if R else w - 1), (w - skip_r if R else w)
    end_y_full, end_y = (h - skip_b if B else h), (h - skip_b if B else h - 1)
    xin, xfull = _span(w, start_x, end_x), _span(w, 0, end_x_full)
    m0 = np.outer(_span(h, 0, end_y_full), xin)
    m90 = np.outer(_span(h, 0 if A else 1, end_y), xfull)
    mid = np.outer(_span(h, 1, end_y), xin)
    m135, m45 = mid.copy(), mid.copy()
    m135[0] = _span(w, 0 if AL else 1, end_x if A else 1)
    m45[0] = _span(w, start_x if A else end_x, w if (not R and AR) else end_x)
    return [m0, m90, m135, m45, np.outer(_span(h, 0, end_y_full), xfull)]


def stats_ctu(org, padded_src, x0, y0, w, h, bit_depth, is_luma, flags):
    rec = np.zeros((5, 2, 32), np.int64)
    c, et = _edge_types(padded_src, x0, y0, w, h)
    d = org[y0:y0 + h, x0:x0 + w].astype(np.int64) - c
    masks = stats_masks(w, h, is_luma, flags)
    cls = et + [c >> (bit_depth - 5)]
    for t in range(5):
        sel = masks[t]
        np.add.at(rec[t, 0], cls[t][sel], d[sel])
        np.add.at(rec[t, 1], cls[t][sel], 1)
    return rec


def stats_picture(org, src, ctu_w, ctu_h, bit_depth, is_luma, flags=None, rows=None):
    """-> int64 [ctus][5][2][32] of one plane; flags: uint8 per CTU or None = borders; rows = ( first, count ): the other CTUs' records stay zero"""
    h, w = src.shape
    gx, gy = grid(w, h, ctu_w, ctu_h)
    flags = border_flags(gx, gy) if flags is None else np.asarray(flags, np.uint8).reshape(-1)
    padded = np.pad(src.astype(np.int64), 1)
    out = np.zeros((gx * gy, 5, 2, 32), np.int64)
    r0, rn = (0, gy) if rows is None else rows
    for cy in range(r0, r0 + rn):
        for cx in range(gx):
            x0, y0 = cx * ctu_w, cy * ctu_h
            out[cy * gx + cx] = stats_ctu(org, padded, x0, y0, min(ctu_w, w - x0), min(ctu_h, h - y0), bit_depth, is_luma, int(flags[cy * gx + cx]))
    return out


def offset_masks(w, h, typ, avail):
    """the samples of a w x h CTU that offsetBlock filters with edge type `typ` -> boolean h x w mask"""
    L, R, A, B, AL, AR, BL, BR = (bool(avail & f) for f in AVAIL_BITS)
    start_x, end_x = (0 if L else 1), (w if R else w - 1)
    if typ == 0:
        return np.outer(np.ones(h, bool), _span(w, start_x, end_x))
    if typ == 1:
        return np.outer(_span(h, 0 if A else 1, h if B else h - 1), np.ones(w, bool))
    m = np.outer(_span(h, 1, h - 1), _span(w, start_x, end_x))
    if typ == 2:
        m[0] = _span(w, 0 if AL else 1, end_x if A else 1)
        m[h - 1] = _span(w, start_x if B else w - 1, w if BR else w - 1)
    else:
        m[0] = _span(w, start_x if A else w - 1, w if AR else w - 1)
        m[h - 1] = _span(w, 0 if BL else 1, end_x if B else 1)
    return m


def offset_ctu(dst, padded_src, x0, y0, w, h, bit_depth, prm, clip):
    typ = int(prm["type"])
    if typ < 0:
        return
    c, et = _edge_types(padded_src, x0, y0, w, h)
    offs = prm["offs"].astype(np.int64)
    if typ == 4:
        table = np.zeros(32, np.int64)
        for i in range(4):
            table[(int(prm["band"]) + i) & 31] = offs[i]
        v, m = c + table[c >> (bit_depth - 5)], np.ones((h, w), bool)
    else:
        v, m = c + offs[et[typ]], offset_masks(w, h, typ, int(prm["avail"]))
    blk = dst[y0:y0 + h, x0:x0 + w]
    blk[m] = np.clip(v, clip[0], clip[1])[m]


def offset_picture(src, params, ctu_w, ctu_h, bit_depth, clip=None, rows=None):
    """-> the SAO'd plane: res starts as a copy of src; params: PARAM_DTYPE per CTU of this plane"""
    h, w = src.shape
    gx, gy = grid(w, h, ctu_w, ctu_h)
    clip = (0, (1 << bit_depth) - 1) if clip is None else clip
    padded = np.pad(src.astype(np.int64), 1)
    dst = src.astype(np.int64).copy()
    r0, rn = (0, gy) if rows is None else rows
    for cy in range(r0, r0 + rn):
        for cx in range(gx):
            x0, y0 = cx * ctu_w, cy * ctu_h
            offset_ctu(dst, padded, x0, y0, min(ctu_w, w - x0), min(ctu_h, h - y0), bit_depth, params[cy * gx + cx], clip)
    return dst.astype(np.int16)
