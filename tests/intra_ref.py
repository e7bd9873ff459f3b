"""Plain numpy restatement of the intra luma mode pre-selection arithmetic (vvhip_intra_luma_modes_batch, include/vvenc_hip.h): per block one set of reference lines, per mode
the parameters of IntraPrediction::initPredIntraParams (CommonLib/IntraPrediction.cpp:409-496) for a non-ISP, non-MIP, non-BDPCM luma block, the [1 2 1] reference filter
(xFilterReferenceSamples, :994-1030), the dispatch of predIntraAng (:353-383) with xPredIntraPlanar_Core, xGetPredValDc, IntraPredSampleFilter_Core and all of xPredIntraAng
(:518-681), and the cost of RdCost::xGetHAD2SADs (RdCost.cpp:1768-1816).  The angular part builds the extended main reference as an array, the way the reference does; the device
kernel evaluates it per sample — two routes to the same numbers.

Every function takes a `cnt` dictionary and counts the branches it takes (the fixture's driver and tests/test_intra_cpu.py assert from them that the cases are not vacuous).

lines: the unfiltered reference lines of a block as ONE int16 array: the top row, 2w + 1 + multi_ref_idx samples from the corner, then the left row, 2h + 1 + multi_ref_idx samples
from the corner (the left row starts at predStride = 2w + 1 + multi_ref_idx)."""
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "intra.npz")

NUM_MODES = 67
PLANAR, DC, HOR, DIA, VER, VDIA = 0, 1, 18, 34, 50, 66
SIZES = (4, 8, 16, 32, 64)
ANG_TABLE = (0, 1, 2, 3, 4, 6, 8, 10, 12, 14, 16, 18, 20, 23, 26, 29, 32, 35, 39, 45, 51, 57, 64, 73, 86, 102, 128, 171, 256, 341, 512, 1024)
INV_ANG_TABLE = (0, 16384, 8192, 5461, 4096, 2731, 2048, 1638, 1365, 1170, 1024, 910, 819, 712, 630, 565, 512, 468, 420, 364, 321, 287, 256, 224, 191, 161, 128, 96, 64, 48, 32, 16)
INTRA_FILTER = (24, 24, 24, 14, 2, 0, 0, 0)          # m_aucIntraFilter, by log2( w * h ) >> 1
MODE_SHIFT = (0, 6, 10, 12, 14, 15)
# the 4-tap cubic filter by 1/32 fraction (InterpolationFilter::getChromaFilterTable; the standard's fC table)
CUBIC = np.array([(0, 64, 0, 0), (-1, 63, 2, 0), (-2, 62, 4, 0), (-2, 60, 7, -1), (-2, 58, 10, -2), (-3, 57, 12, -2), (-4, 56, 14, -2), (-4, 55, 15, -2), (-4, 54, 16, -2),
                  (-5, 53, 18, -2), (-6, 52, 20, -2), (-6, 49, 24, -3), (-6, 46, 28, -4), (-5, 44, 29, -4), (-4, 42, 30, -4), (-4, 39, 33, -4), (-4, 36, 36, -4), (-4, 33, 39, -4),
                  (-4, 30, 42, -4), (-4, 29, 44, -5), (-4, 28, 46, -6), (-3, 24, 49, -6), (-2, 20, 52, -6), (-2, 18, 53, -5), (-2, 16, 54, -4), (-2, 15, 55, -4), (-2, 14, 56, -4),
                  (-2, 12, 57, -3), (-2, 10, 58, -2), (-1, 7, 60, -2), (0, 4, 62, -2), (0, 2, 63, -1)], np.int64)

ITEM_DTYPE = np.dtype([("w", "u1"), ("h", "u1"), ("bit_depth", "u1"), ("multi_ref_idx", "u1"), ("ref_off", "<i4"), ("org_off", "<i4"), ("pred_off", "<i4"), ("cost_off", "<i4"),
                       ("mode_mask", "<u4", 3), ("pred_mask", "<u4", 3), ("rsv", "<u4")])      # vvhip_intra_item (48 bytes)
assert ITEM_DTYPE.itemsize == 48


def log2i(v):
    return int(v).bit_length() - 1


def bump(cnt, key):
    if cnt is not None:
        cnt[key] = cnt.get(key, 0) + 1


def line_len(w, h, mri):
    return (2 * w + 1 + mri) + (2 * h + 1 + mri)


def wide_angle(w, h, mode):
    if DC < mode <= VDIA:
        d = abs(log2i(w) - log2i(h))
        if w > h and mode < 2 + MODE_SHIFT[d]:
            return mode + (VDIA - 1)
        if h > w and mode > VDIA - MODE_SHIFT[d]:
            return mode - (VDIA - 1)
    return mode


def params(w, h, mode, mri):
    """initPredIntraParams -> dict( ver, angle, inv, pdpc, scale, ref_filter, interp, pred_mode )"""
    pm = wide_angle(w, h, mode)
    p = dict(pred_mode=pm, ver=pm >= DIA, angle=0, inv=0, pdpc=mri == 0, scale=-1, ref_filter=False, interp=False)
    am = pm - VER if p["ver"] else -(pm - HOR)
    abs_ang = 0
    if mode > DC:
        abs_ang = ANG_TABLE[abs(am)]
        p["inv"] = INV_ANG_TABLE[abs(am)]
        p["angle"] = -abs_ang if am < 0 else abs_ang
        if am < 0:
            p["pdpc"] = False
        elif am > 0:
            side = h if p["ver"] else w
            p["scale"] = min(2, log2i(side) - (log2i(3 * p["inv"] - 2) - 8))
            p["pdpc"] = p["pdpc"] and p["scale"] >= 0
    if mri or mode == DC:
        pass
    elif mode == PLANAR:
        p["ref_filter"] = w * h > 32
    else:
        diff = min(abs(pm - HOR), abs(pm - VER))
        if diff > INTRA_FILTER[log2i(w * h) >> 1]:
            assert w * h > 32
            integer = (abs_ang & 31) == 0
            p["ref_filter"], p["interp"] = integer, not integer
    return p


def filter_lines(lines, w, h):
    """xFilterReferenceSamples for multi_ref_idx 0 (the only index it is used with) -> the filtered lines in the same layout"""
    s = 2 * w + 1
    u = lines.astype(np.int64)
    f = u.copy()
    tl = (u[0] + u[1] + u[s] + u[s + 1] + 2) >> 2
    for base, n in ((0, 2 * w), (s, 2 * h)):
        f[base] = tl
        f[base + 1:base + n] = (u[base:base + n - 1] + 2 * u[base + 1:base + n] + u[base + 2:base + n + 1] + 2) >> 2
        f[base + n] = u[base + n]
    return f.astype(np.int16)


def _sample_filter(pred, top, left, w, h):
    """IntraPredSampleFilter_Core: top / left as pSrc.at( x + 1, 0 ) / pSrc.at( y + 1, 1 )"""
    scale = (log2i(w * h) - 2) >> 2
    y, x = np.mgrid[0:h, 0:w]
    wt = 32 >> np.minimum(31, (y << 1) >> scale)
    wl = 32 >> np.minimum(31, (x << 1) >> scale)
    return pred + ((wl * (left[1 + y] - pred) + wt * (top[1 + x] - pred) + 32) >> 6)


def predict(lines, w, h, mode, mri, bit_depth, cnt=None):
    """-> the prediction block of one mode, int16 ( h, w )"""
    assert w in SIZES and h in SIZES and 0 <= mode < NUM_MODES and 0 <= mri <= 2 and not (mode == PLANAR and mri)
    lines = np.asarray(lines)
    assert lines.size == line_len(w, h, mri)
    p = params(w, h, mode, mri)
    stride = 2 * w + 1 + mri
    src = lines
    if p["ref_filter"]:
        src = filter_lines(lines, w, h)
        bump(cnt, "ref_filter")
    src = src.astype(np.int64)
    top, left = src[:stride], src[stride:]
    vmax = (1 << bit_depth) - 1
    lw, lh = log2i(w), log2i(h)
    if mode == PLANAR:
        bump(cnt, "planar")
        y, x = np.mgrid[0:h, 0:w]
        tr, bl = top[w + 1], left[h + 1]
        hor = (left[1 + y] << lw) + (x + 1) * (tr - left[1 + y])
        ver = (top[1 + x] << lh) + (y + 1) * (bl - top[1 + x])
        pred = ((hor << lh) + (ver << lw) + (1 << (lw + lh))) >> (1 + lw + lh)
        pred = _sample_filter(pred, top, left, w, h)
        return pred.astype(np.int16)
    if mode == DC:
        bump(cnt, "dc")
        off, s = mri + 1, 0
        if w >= h:
            s += int(top[off:off + w].sum())
        if w <= h:
            s += int(left[off:off + h].sum())
        den = 2 * w if w == h else max(w, h)
        pred = np.full((h, w), (s + (den >> 1)) >> log2i(den), np.int64)
        if p["pdpc"]:
            bump(cnt, "dc_pdpc")
            pred = _sample_filter(pred, top, left, w, h)
        return pred.astype(np.int16)
    # ---- xPredIntraAng ----
    ver, angle, inv = p["ver"], p["angle"], p["inv"]
    if p["pred_mode"] < 2:
        bump(cnt, "wide_below")
    elif p["pred_mode"] > VDIA:
        bump(cnt, "wide_above")
    mline, sline = (top, left) if ver else (left, top)
    W, H = (w, h) if ver else (h, w)          # the block as the main direction sees it
    if angle < 0:
        bump(cnt, "neg_ver" if ver else "neg_hor")
        side = sline[:H + 2 + mri]
        k = np.arange(-H, 0)
        ext = side[np.minimum((-k * inv + 256) >> 9, H)]
        main, base = np.concatenate([ext, mline[:W + 2 + mri]]), H          # main[base + i] is refMain[i]
    else:
        ref_len = 2 * W
        s = max(0, log2i(W) - log2i(H))
        max_index = (mri << s) + 2
        main, base = np.concatenate([mline[:ref_len + mri + 1], np.full(max_index, mline[ref_len + mri])]), 0
        side = sline
    base += mri
    soff = mri
    yy, xx = np.mgrid[0:H, 0:W]

    def at(arr, idx, b):
        idx = idx + b
        assert idx.min() >= 0 and idx.max() < arr.size, "the reference would read outside its arrays"
        return arr[idx]

    if angle == 0:
        pred = at(main, 1 + xx, base)
        if p["pdpc"]:
            bump(cnt, "hv_pdpc")
            scale = (log2i(W * H) - 2) >> 2
            m = xx < min(3 << scale, W)
            wl = 32 >> np.minimum(31, (2 * xx) >> scale)
            adj = np.clip(pred + ((wl * (at(side, 1 + yy, soff) - main[base]) + 32) >> 6), 0, vmax)
            if (pred + ((wl * (at(side, 1 + yy, soff) - main[base]) + 32) >> 6))[m].min() < 0:
                bump(cnt, "clip_low")
            if (pred + ((wl * (at(side, 1 + yy, soff) - main[base]) + 32) >> 6))[m].max() > vmax:
                bump(cnt, "clip_high")
            pred = np.where(m, adj, pred)
        else:
            bump(cnt, "hv_copy")
    else:
        dpos = angle * (1 + mri) + angle * yy
        dint, frac = dpos >> 5, dpos & 31
        if (abs(angle) & 31) == 0:
            bump(cnt, "integer_slope")
            pred = at(main, dint + 1 + xx, base)
        else:
            taps = [at(main, dint + xx + t, base) for t in range(4)]
            if not p["interp"]:
                bump(cnt, "cubic")
                f = CUBIC[frac]
                raw = (f[..., 0] * taps[0] + f[..., 1] * taps[1] + f[..., 2] * taps[2] + f[..., 3] * taps[3] + 32) >> 6
                if raw.min() < 0:
                    bump(cnt, "clip_low")
                if raw.max() > vmax:
                    bump(cnt, "clip_high")
                pred = np.clip(raw, 0, vmax)
            else:
                bump(cnt, "smoothing")
                hf = frac >> 1
                pred = ((16 - hf) * taps[0] + (32 - hf) * taps[1] + (16 + hf) * taps[2] + hf * taps[3] + 32) >> 6
        if p["pdpc"]:
            bump(cnt, "ang_pdpc_scale%d" % p["scale"])
            m = xx < min(3 << p["scale"], W)
            wl = 32 >> np.minimum(31, (2 * xx) >> p["scale"])
            sidx = np.where(m, yy + ((256 + inv * (xx + 1)) >> 9) + 1, 0)
            lft = at(side, sidx, soff)
            pred = np.where(m, pred + ((wl * (lft - pred) + 32) >> 6), pred)
        elif mri == 0 and angle > 0:
            bump(cnt, "ang_pdpc_off_negative_scale")
    if not ver:
        bump(cnt, "transposed")
        pred = pred.T
    return np.ascontiguousarray(pred).astype(np.int16)


# ---- the cost: min( xGetHADs<false>, 2 * SAD ) ------------------------------------------------------------------------------------------------------------
def _hmat(n):
    m = np.array([[1]], np.int64)
    while m.shape[0] < n:
        m = np.block([[m, m], [m, -m]])
    return m


def tile_shape(w, h):
    """the tile ladder of xGetHADs (RdCost.cpp:1818-1938), first match wins, for the block sizes of this entry"""
    if w > h and h % 8 == 0 and w % 16 == 0:
        return 16, 8
    if w < h and w % 8 == 0 and h % 16 == 0:
        return 8, 16
    if w > h and h % 4 == 0 and w % 8 == 0:
        return 8, 4
    if w < h and w % 4 == 0 and h % 8 == 0:
        return 4, 8
    if w % 8 == 0 and h % 8 == 0:
        return 8, 8
    return 4, 4


def had(org, pred):
    h, w = org.shape
    tw, th = tile_shape(w, h)
    d = org.astype(np.int64) - pred.astype(np.int64)
    hw, hh = _hmat(tw), _hmat(th)
    total = 0
    for y in range(0, h, th):
        for x in range(0, w, tw):
            c = np.abs(hh @ d[y:y + th, x:x + tw] @ hw)
            s = int(c.sum()) - int(c[0, 0]) + (int(c[0, 0]) >> 2)
            if (tw, th) == (8, 8):
                s = (s + 2) >> 2
            elif (tw, th) == (4, 4):
                s = (s + 1) >> 1
            else:
                s = int(s / np.sqrt(float(tw * th)) * 2)
            total += s
    return total


def cost(org, pred, cnt=None):
    d_had = had(org, pred)
    d_sad = 2 * int(np.abs(org.astype(np.int64) - pred.astype(np.int64)).sum())
    if d_had != d_sad:
        bump(cnt, "cost_had" if d_had < d_sad else "cost_2sad")
    return min(d_had, d_sad)


def mask_bits(mask):
    """the set bits of a 3 x uint32 mask, ascending"""
    return [m for m in range(96) if (int(mask[m >> 5]) >> (m & 31)) & 1]


def make_mask(modes):
    out = np.zeros(3, np.uint32)
    for m in modes:
        out[m >> 5] |= np.uint32(1 << (m & 31))
    return out


def run_items(items, ref, org, cnt=None):
    """the entry on a list -> ( costs uint32 [n][67], 0 where not requested; per item the list of ( mode, prediction ) of its pred_mask )"""
    costs, preds = np.zeros((len(items), NUM_MODES), np.uint32), []
    for i, it in enumerate(items):
        w, h, mri, bd = int(it["w"]), int(it["h"]), int(it["multi_ref_idx"]), int(it["bit_depth"])
        lines = ref[int(it["ref_off"]):int(it["ref_off"]) + line_len(w, h, mri)]
        o = org[int(it["org_off"]):int(it["org_off"]) + w * h].reshape(h, w)
        want, mine = set(mask_bits(it["pred_mask"])), []
        for m in mask_bits(it["mode_mask"]):
            p = predict(lines, w, h, m, mri, bd, cnt)
            costs[i, m] = cost(o, p, cnt)
            if m in want:
                mine.append((m, p))
        preds.append(mine)
    return costs, preds
