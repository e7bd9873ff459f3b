"""Expected values for the affine prediction entry (vvhip_pred_affine_batch): a numpy model of what InterPredInterpolation::xPredAffineBlk
(CommonLib/InterPrediction.cpp:1497-1839) does AROUND the interpolation passes, shared by the CPU and GPU tests.

Every interpolation pass is EXECUTED from the library handed in (`RefLib(0)` scalar row, `RefLib(1)` x86 row of the compiled reference, or `Oracle()`), through
pred_ref.luma_pred / pred_ref.chroma_pred at 4x4 — the passes a 4x4 item of vvhip_pred_inter_batch takes.  Restated here in numpy, with the reference's lines:
  model deltas, base                      :1528-1542          sub-block vector, roundAffineMv, 18-bit clip     :1697-1722, Mv.cpp:61-66
  isSubblockVectorSpreadOverLimit         :1457-1495          picture clip                                     :1545-1550, :1725-1726
  chroma vector from two luma vectors     :1729-1765          PROF conditions that depend on the vectors       :1557-1560
  dMv table                               :1583-1630          ring, gradFilterCore<false>, applyPROFCore       :1797-1835, :113-131, :88-111
tests/golden/affine.npz (recorded from the reference's own xPredAffineBlk, see tests/affine_golden_gen.py) is the anchor of this model where it is present."""
import numpy as np

import pred_ref as PR

SIZES = [(w, h) for w in (8, 16, 32, 64, 128) for h in (8, 16, 32, 64, 128)]


def round_affine(v, shift):
    return (v + (1 << (shift - 1)) - (1 if v >= 0 else 0)) >> shift


def spread_over_limit(a, b, c, d, pred_type):
    s4, tap = 4 << 11, 6
    if pred_type == 3:
        rw = max(0, 4 * a + s4, 4 * c, 4 * a + 4 * c + s4) - min(0, 4 * a + s4, 4 * c, 4 * a + 4 * c + s4)
        rh = max(0, 4 * b, 4 * d + s4, 4 * b + 4 * d + s4) - min(0, 4 * b, 4 * d + s4, 4 * b + 4 * d + s4)
        return ((rw >> 11) + tap + 3) * ((rh >> 11) + tap + 3) > (tap + 9) * (tap + 9)
    rw, rh = max(0, 4 * a + s4) - min(0, 4 * a + s4), max(0, 4 * b) - min(0, 4 * b)
    if ((rw >> 11) + tap + 3) * ((rh >> 11) + tap + 3) > (tap + 9) * (tap + 5):
        return True
    rw, rh = max(0, 4 * c) - min(0, 4 * c), max(0, 4 * d + s4) - min(0, 4 * d + s4)
    return ((rw >> 11) + tap + 3) * ((rh >> 11) + tap + 3) > (tap + 5) * (tap + 9)


class ListModel:
    """what one reference list of one CU needs besides the samples: deltas, spread, the PROF decision, the stored luma vectors, the dMv table"""

    def __init__(self, it, l):
        w, h = int(it["cu_w"]), int(it["cu_h"])
        cp = [[int(v) for v in it["cpmv"][l][k]] for k in range(3)]
        lw, lh = w.bit_length() - 1, h.bit_length() - 1
        self.hx, self.hy = (cp[1][0] - cp[0][0]) * (1 << (7 - lw)), (cp[1][1] - cp[0][1]) * (1 << (7 - lw))
        if int(it["six_param"]):
            self.vx, self.vy = (cp[2][0] - cp[0][0]) * (1 << (7 - lh)), (cp[2][1] - cp[0][1]) * (1 << (7 - lh))
        else:
            self.vx, self.vy = -self.hy, self.hx
        used = [k for k in (0, 1) if int(it["ref_plane"][k]) >= 0]
        self.bi = len(used) == 2
        self.spread = spread_over_limit(self.hx, self.hy, self.vx, self.vy, 3 if self.bi else 1 + l)
        bx, by = cp[0][0] * 128, cp[0][1] * 128
        self.stored = np.zeros((h // 4, w // 4, 2), np.int64)
        for sy in range(h // 4):
            for sx in range(w // 4):
                px, py = (w >> 1, h >> 1) if self.spread else (2 + 4 * sx, 2 + 4 * sy)
                mx = round_affine(bx + self.hx * px + self.vx * py, 7)
                my = round_affine(by + self.hy * px + self.vy * py, 7)
                self.stored[sy, sx] = (min(max(mx, -(1 << 17)), (1 << 17) - 1), min(max(my, -(1 << 17)), (1 << 17) - 1))
        same = cp[0] == cp[1] and (not int(it["six_param"]) or cp[0] == cp[2])
        p = int(it["prof"])
        self.prof = p != 0 and not int(it["chroma"]) and not same and not self.spread
        self.over_threshold = {t: any(abs(v) > (1 << t) for v in (self.hx, self.hy, self.vx, self.vy)) for t in (7, 8)}
        if p >= 2:
            self.prof = self.prof and self.over_threshold[7 if p == 2 else 8]
        dmx, dmy = np.zeros((4, 4), np.int64), np.zeros((4, 4), np.int64)
        for r in range(4):
            for c in range(4):
                dmx[r, c] = min(max(round_affine(-6 * (self.hx + self.vx) + 4 * c * self.hx + 4 * r * self.vx, 8), -31), 31)
                dmy[r, c] = min(max(round_affine(-6 * (self.hy + self.vy) + 4 * c * self.hy + 4 * r * self.vy, 8), -31), 31)
        self.dmx, self.dmy = dmx, dmy


def sub_vectors(it, m, pic_w, pic_h, ctu, clip=True):
    """-> int array [rows][cols][4] = (xInt, yInt, xFrac, yFrac) of every 4x4 sub-block of the item's component block"""
    chroma = int(it["chroma"])
    bw, bh = int(it["cu_w"]) >> chroma, int(it["cu_h"]) >> chroma
    cx, cy = int(it["cu_x"]), int(it["cu_y"])
    hmax, hmin = (pic_w + 8 - cx - 1) << 4, (-ctu - 8 - cx + 1) * 16
    vmax, vmin = (pic_h + 8 - cy - 1) << 4, (-ctu - 8 - cy + 1) * 16
    out = np.zeros((bh // 4, bw // 4, 4), np.int64)
    for sy in range(bh // 4):
        for sx in range(bw // 4):
            if chroma:
                a, b = m.stored[2 * sy, 2 * sx], m.stored[2 * sy + 1, 2 * sx + 1]
                mx, my = round_affine(int(a[0] + b[0]), 1), round_affine(int(a[1] + b[1]), 1)
            else:
                mx, my = int(m.stored[sy, sx][0]), int(m.stored[sy, sx][1])
            if clip:
                mx, my = min(hmax, max(hmin, mx)), min(vmax, max(vmin, my))
            s = 5 if chroma else 4
            out[sy, sx] = (mx >> s, my >> s, mx & ((1 << s) - 1), my & ((1 << s) - 1))
    return out


def prof_refine(blk14, arr, y, x, xf, yf, m, bi, bd):
    """blk14: the sub-block's 14-bit block; (x, y): its integer position in arr -> the refined block (14-bit when bi, final samples otherwise)"""
    hr = max(2, 14 - bd)
    yo, xo = y + (yf >> 3), x + (xf >> 3)
    fr = ((arr[yo - 1:yo + 5, xo - 1:xo + 5].astype(np.int64) << hr) - 8192).astype(np.int16).astype(np.int64)
    fr[1:5, 1:5] = blk14
    gx = (fr[1:5, 2:6] >> 6) - (fr[1:5, 0:4] >> 6)
    gy = (fr[2:6, 1:5] >> 6) - (fr[0:4, 1:5] >> 6)
    lim = 1 << max(bd + 1, 13)
    di = np.clip(m.dmx * gx + m.dmy * gy, -lim, lim - 1)
    v = (blk14.astype(np.int64) + di).astype(np.int16)          # the Pel store before the rounding
    if bi:
        return v
    v = ((v.astype(np.int64) + (1 << (hr - 1)) + 8192) >> hr).astype(np.int16)
    return np.clip(v, 0, (1 << bd) - 1).astype(np.int16)


def list_block(lib, planes, pos, it, l, bd, pic_w, pic_h, ctu, clip=True, force_prof=None):
    """what xPredAffineBlk leaves for list l of the item: final samples when the list is alone, the 14-bit block (after PROF) when both lists are used"""
    chroma = int(it["chroma"])
    bw, bh = int(it["cu_w"]) >> chroma, int(it["cu_h"]) >> chroma
    bi = int(it["ref_plane"][0]) >= 0 and int(it["ref_plane"][1]) >= 0
    m = ListModel(it, l)
    prof = m.prof if force_prof is None else (force_prof and not chroma)
    last = not bi and not prof
    arr, (x0, y0) = planes[int(it["ref_plane"][l])], pos[l]
    vec = sub_vectors(it, m, pic_w, pic_h, ctu, clip)
    blk = np.zeros((bh, bw), np.int16)
    for sy in range(bh // 4):
        for sx in range(bw // 4):
            xi, yi, xf, yf = (int(v) for v in vec[sy, sx])
            x, y = x0 + 4 * sx + xi, y0 + 4 * sy + yi
            if chroma:
                b = PR.chroma_pred(lib, arr, y, x, 4, 4, xf, yf, last, bd)
            else:
                b = PR.luma_pred(lib, arr, y, x, 4, 4, xf, yf, last, bd, 0)
                if prof:
                    b = prof_refine(b, arr, y, x, xf, yf, m, bi, bd)
            blk[4 * sy:4 * sy + 4, 4 * sx:4 * sx + 4] = b
    return blk


def expected_block(lib, planes, pos, it, bd, pic_w, pic_h, ctu, clip=True, force_prof=None):
    """planes[k]: 2-D int16 array (margins included); pos[l] = (x, y) of the block's own position in planes[it.ref_plane[l]]; it: a PRED_AFFINE_ITEM_DTYPE record.
    force_prof: overrides the PROF decision of every list (the guards use it to see what PROF changes)"""
    out = [list_block(lib, planes, pos, it, l, bd, pic_w, pic_h, ctu, clip, force_prof) for l in (0, 1) if int(it["ref_plane"][l]) >= 0]
    return out[0] if len(out) == 1 else PR.bi_average(out[0], out[1], bd)


def read_extent(it, pic_w, pic_h, ctu):
    """how far the item's sub-blocks read beyond the picture, in samples of its component: (left, above, right, below), taps, PROF ring and the aligned dword included"""
    chroma = int(it["chroma"])
    bw, bh = int(it["cu_w"]) >> chroma, int(it["cu_h"]) >> chroma
    cx, cy, pw, ph = int(it["cu_x"]) >> chroma, int(it["cu_y"]) >> chroma, pic_w >> chroma, pic_h >> chroma
    lo, hi = (1, 2) if chroma else (3, 4)
    ext = [0, 0, 0, 0]
    for l in (0, 1):
        if int(it["ref_plane"][l]) < 0:
            continue
        vec = sub_vectors(it, ListModel(it, l), pic_w, pic_h, ctu)
        for sy in range(bh // 4):
            for sx in range(bw // 4):
                xi, yi = int(vec[sy, sx][0]), int(vec[sy, sx][1])
                x, y = cx + 4 * sx + xi, cy + 4 * sy + yi
                ext = [max(ext[0], lo + 1 - x), max(ext[1], lo - y), max(ext[2], x + 3 + hi + 1 - (pw - 1)), max(ext[3], y + 3 + hi - (ph - 1))]
    return ext


def expand_items(it, strides, pic_w, pic_h, ctu, item_dtype):
    """the CU's component block as 4x4 items of vvhip_pred_inter_batch (what a host has to do without the affine entry; PROF cannot be expressed): -> (items, (sx, sy) per item,
    vectors per list).  ref_off relative to the affine item's own ref_off; dst_off = 16 * index (compact 4x4 blocks)"""
    chroma = int(it["chroma"])
    bw, bh = int(it["cu_w"]) >> chroma, int(it["cu_h"]) >> chroma
    n = (bw // 4) * (bh // 4)
    out = np.zeros(n, item_dtype)
    vec = {l: sub_vectors(it, ListModel(it, l), pic_w, pic_h, ctu) for l in (0, 1) if int(it["ref_plane"][l]) >= 0}
    where = []
    for sy in range(bh // 4):
        for sx in range(bw // 4):
            k = sy * (bw // 4) + sx
            out[k]["width"], out[k]["height"], out[k]["chroma"], out[k]["dst_off"] = 4, 4, chroma, 16 * k
            out[k]["ref_plane"] = it["ref_plane"]
            for l, v in vec.items():
                xi, yi, xf, yf = (int(t) for t in v[sy, sx])
                out[k]["ref_off"][l] = int(it["ref_off"][l]) + (4 * sy + yi) * strides[int(it["ref_plane"][l])] + 4 * sx + xi
                out[k]["frac"][l] = (xf, yf)
            where.append((sx, sy))
    return out, where, vec


def blocks_to_block(flat, bw, bh):
    """compact 4x4 blocks in raster order of sub-blocks -> the bh x bw block"""
    return flat.reshape(bh // 4, bw // 4, 4, 4).transpose(0, 2, 1, 3).reshape(bh, bw)
