"""Plain numpy restatement of the intra chroma mode pre-selection arithmetic (vvhip_intra_chroma_modes_batch, include/vvenc_hip.h): per 4:2:0 chroma block the Cb and the Cr
prediction of up to eight candidate modes and the cost min( 2 * SAD, HAD ) of Cb plus the same of Cr, as IntraSearch::estIntraPredChromaQT forms satdSortedCost
(EncoderLib/IntraSearch.cpp:778-862).
  regular modes 0..66   initPredIntraParams for a chroma block (CommonLib/IntraPrediction.cpp:409-496: no reference filter, no interpolation flag), predIntraAng's planar / DC /
                        IntraPredSampleFilter, xPredIntraAng with IntraPredAngleChroma_Core (:225-245: two-tap linear interpolation), the HOR / VER PDPC and IntraAnglePDPC
  modes 67..69          the 4:2:0 branches of loadLMLumaRecPels (:1165-1406), xGetLMParameters (:1408-1605) and linearTransform( a, iShift, b, clip )
The down-sampled template is formed sample by sample, only where xGetLMParameters picks; the device kernel does the same.

Every function takes a `cnt` dictionary and counts the branches it takes (the fixture's driver and tests/test_intra_chroma_cpu.py assert from them that the cases are not vacuous).

luma: a plane of reconstructed luma as ONE int16 array; an item names the top-left sample of its collocated 2w x 2h area with luma_off and the plane's pitch with luma_stride.
lines: the unfiltered reference lines of one component in the luma entry's layout with multi_ref_idx 0: corner, 2w samples above, corner again, 2h samples to the left."""
import os

import numpy as np

import intra_ref as IR
from intra_ref import bump, log2i

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "intra_chroma.npz")

SIZES = (4, 8, 16, 32)
NUM_SLOTS = 8
LM, MDLM_L, MDLM_T = 67, 68, 69
F_ABOVE, F_LEFT, F_FIRST_ROW, F_VER_COLLOCATED = 1, 2, 4, 8
DIV_SIG_TABLE = (0, 7, 6, 5, 5, 4, 4, 3, 3, 2, 2, 1, 1, 1, 1, 0)

ITEM_DTYPE = np.dtype([("w", "u1"), ("h", "u1"), ("bit_depth", "u1"), ("flags", "u1"), ("n_above_right", "u1"), ("n_left_below", "u1"), ("mode_mask", "u1"), ("pred_mask", "u1"),
                       ("cand", "u1", 8), ("luma_off", "<i4"), ("luma_stride", "<i4"), ("ref_off", "<i4", 2), ("org_off", "<i4", 2), ("pred_off", "<i4", 2), ("cost_off", "<i4"),
                       ("rsv", "u1", 12)])      # vvhip_intra_chroma_item (64 bytes)
assert ITEM_DTYPE.itemsize == 64


def line_len(w, h):
    return IR.line_len(w, h, 0)


# ---- regular modes ---------------------------------------------------------------------------------------------------------------------------------------------
def predict_regular(lines, w, h, mode, bit_depth, cnt=None):
    """-> the prediction of a regular mode 0..66 on a chroma block, int16 ( h, w )"""
    assert w in SIZES and h in SIZES and 0 <= mode < IR.NUM_MODES
    lines = np.asarray(lines).astype(np.int64)
    assert lines.size == line_len(w, h)
    p = IR.params(w, h, mode, 0)          # (the luma-only fields ref_filter / interp are not read here: a chroma block has neither, :461-468)
    stride = 2 * w + 1
    top, left = lines[:stride], lines[stride:]
    vmax = (1 << bit_depth) - 1
    lw, lh = log2i(w), log2i(h)
    if mode == IR.PLANAR:
        bump(cnt, "planar")
        y, x = np.mgrid[0:h, 0:w]
        tr, bl = top[w + 1], left[h + 1]
        hor = (left[1 + y] << lw) + (x + 1) * (tr - left[1 + y])
        ver = (top[1 + x] << lh) + (y + 1) * (bl - top[1 + x])
        pred = ((hor << lh) + (ver << lw) + (1 << (lw + lh))) >> (1 + lw + lh)
        return IR._sample_filter(pred, top, left, w, h).astype(np.int16)
    if mode == IR.DC:
        bump(cnt, "dc" if w == h else "dc_nonsquare")
        s = 0
        if w >= h:
            s += int(top[1:1 + w].sum())
        if w <= h:
            s += int(left[1:1 + h].sum())
        den = 2 * w if w == h else max(w, h)
        pred = np.full((h, w), (s + (den >> 1)) >> log2i(den), np.int64)
        return IR._sample_filter(pred, top, left, w, h).astype(np.int16)
    ver, angle, inv = p["ver"], p["angle"], p["inv"]
    if p["pred_mode"] < 2:
        bump(cnt, "wide_below")
    elif p["pred_mode"] > IR.VDIA:
        bump(cnt, "wide_above")
    mline, sline = (top, left) if ver else (left, top)
    W, H = (w, h) if ver else (h, w)
    if angle < 0:
        bump(cnt, "neg_ver" if ver else "neg_hor")
        side = sline[:H + 2]
        k = np.arange(-H, 0)
        ext = side[np.minimum((-k * inv + 256) >> 9, H)]
        main, base = np.concatenate([ext, mline[:W + 2]]), H
    else:
        main, base = np.concatenate([mline[:2 * W + 1], np.full(2, mline[2 * W])]), 0
        side = sline
    yy, xx = np.mgrid[0:H, 0:W]

    def at(arr, idx, b=0):
        idx = idx + b
        assert idx.min() >= 0 and idx.max() < arr.size, "the reference would read outside its arrays"
        return arr[idx]

    if angle == 0:
        pred = at(main, 1 + xx, base)
        bump(cnt, "hv_pdpc")          # (a chroma block of this entry has sides >= 4: applyPDPC holds for the pure directions)
        scale = (log2i(W * H) - 2) >> 2
        m = xx < min(3 << scale, W)
        wl = 32 >> np.minimum(31, (2 * xx) >> scale)
        raw = pred + ((wl * (at(side, 1 + yy) - main[base]) + 32) >> 6)
        if raw[m].min() < 0:
            bump(cnt, "hv_clip_low")
        if raw[m].max() > vmax:
            bump(cnt, "hv_clip_high")
        pred = np.where(m, np.clip(raw, 0, vmax), pred)
    else:
        dpos = angle * (1 + yy)
        dint, frac = dpos >> 5, dpos & 31
        if (abs(angle) & 31) == 0:
            bump(cnt, "integer_slope")
            pred = at(main, dint + 1 + xx, base)
        else:
            bump(cnt, "two_tap")
            pred = ((32 - frac) * at(main, dint + 1 + xx, base) + frac * at(main, dint + 2 + xx, base) + 16) >> 5
        if p["pdpc"]:
            bump(cnt, "ang_pdpc_scale%d" % p["scale"])
            m = xx < min(3 << p["scale"], W)
            wl = 32 >> np.minimum(31, (2 * xx) >> p["scale"])
            sidx = np.where(m, yy + ((256 + inv * (xx + 1)) >> 9) + 1, 0)
            lft = at(side, sidx)
            pred = np.where(m, pred + ((wl * (lft - pred) + 32) >> 6), pred)
        elif angle > 0:
            bump(cnt, "ang_pdpc_off_negative_scale")
    if not ver:
        pred = pred.T
    return np.ascontiguousarray(pred).astype(np.int16)


# ---- CCLM / MDLM -----------------------------------------------------------------------------------------------------------------------------------------------
class Luma(object):
    """the collocated luma area of an item: P( x, y ) is the sample at ( x, y ) from the area's top-left; every read is recorded in `touched` (offsets into the plane)"""

    def __init__(self, luma, off, stride, touched=None):
        self.luma, self.off, self.stride, self.touched = luma, int(off), int(stride), touched

    def P(self, x, y):
        i = self.off + y * self.stride + x
        assert 0 <= i < self.luma.size, "the reference would read outside the plane"
        if self.touched is not None:
            self.touched.add(i)
        return int(self.luma[i])


def ds_inner(L, flags, i, j, cnt=None):
    """loadLMLumaRecPels :1355-1405, 4:2:0: the down-sampled sample ( i, j ) of the block"""
    lp = 0 if (i == 0 and not flags & F_LEFT) else 1
    if lp == 0:
        bump(cnt, "left_padding")
    if flags & F_VER_COLLOCATED:
        ap = 0 if (j == 0 and not flags & F_ABOVE) else 1
        if ap == 0:
            bump(cnt, "above_padding")
        return (L.P(2 * i, 2 * j - ap) + 4 * L.P(2 * i, 2 * j) + L.P(2 * i - lp, 2 * j) + L.P(2 * i + 1, 2 * j) + L.P(2 * i, 2 * j + 1) + 4) >> 3
    return (2 * L.P(2 * i, 2 * j) + L.P(2 * i + 1, 2 * j) + L.P(2 * i - lp, 2 * j) + 2 * L.P(2 * i, 2 * j + 1) + L.P(2 * i + 1, 2 * j + 1) + L.P(2 * i - lp, 2 * j + 1) + 4) >> 3


def ds_above(L, flags, i, cnt=None):
    """:1243-1299: position i of the down-sampled row above the block (the above-right extension continues it)"""
    lp = 0 if (i == 0 and not flags & F_LEFT) else 1
    if lp == 0:
        bump(cnt, "left_padding")
    if flags & F_FIRST_ROW:
        bump(cnt, "first_row")
        return (2 * L.P(2 * i, -1) + L.P(2 * i - lp, -1) + L.P(2 * i + 1, -1) + 2) >> 2
    if flags & F_VER_COLLOCATED:
        return (L.P(2 * i, -3) + 4 * L.P(2 * i, -2) + L.P(2 * i - lp, -2) + L.P(2 * i + 1, -2) + L.P(2 * i, -1) + 4) >> 3
    return (2 * L.P(2 * i, -2) + L.P(2 * i + 1, -2) + L.P(2 * i - lp, -2) + 2 * L.P(2 * i, -1) + L.P(2 * i + 1, -1) + L.P(2 * i - lp, -1) + 4) >> 3


def ds_left(L, flags, j, cnt=None):
    """:1301-1353: position j of the down-sampled column left of the block (the left-below extension continues it)"""
    if flags & F_VER_COLLOCATED:
        ap = 0 if (j == 0 and not flags & F_ABOVE) else 1
        if ap == 0:
            bump(cnt, "above_padding")
        return (L.P(-2, 2 * j - ap) + 4 * L.P(-2, 2 * j) + L.P(-3, 2 * j) + L.P(-1, 2 * j) + L.P(-2, 2 * j + 1) + 4) >> 3
    return (2 * L.P(-2, 2 * j) + L.P(-1, 2 * j) + L.P(-3, 2 * j) + 2 * L.P(-2, 2 * j + 1) + L.P(-1, 2 * j + 1) + L.P(-3, 2 * j + 1) + 4) >> 3


def lm_params(L, lines, w, h, bit_depth, flags, n_ar, n_lb, mode, cnt=None):
    """xGetLMParameters -> ( a, b, shift )"""
    above, left = bool(flags & F_ABOVE), bool(flags & F_LEFT)
    top_n = left_n = 0
    if mode == MDLM_T:
        left = False
        ar = min(n_ar, h)          # :1487, in samples
        bump(cnt, "clamp_above_right_bites" if n_ar > h else "clamp_above_right_free")
        top_n = (w + ar) if above else 0
        if not above:
            bump(cnt, "mdlm_t_default")
    elif mode == MDLM_L:
        above = False
        lb = min(n_lb, w)          # :1493
        bump(cnt, "clamp_left_below_bites" if n_lb > w else "clamp_left_below_free")
        left_n = (h + lb) if left else 0
        if not left:
            bump(cnt, "mdlm_l_default")
    else:
        top_n, left_n = w, h
    above_is4, left_is4 = (0 if left else 1), (0 if above else 1)
    start = (top_n >> (2 + above_is4), left_n >> (2 + left_is4))
    step = (max(1, top_n >> (1 + above_is4)), max(1, left_n >> (1 + left_is4)))
    sel_l, sel_c = [], []
    stride = 2 * w + 1
    if above:
        for k in range(min(top_n, (1 + above_is4) << 1)):
            pos = start[0] + k * step[0]
            sel_l.append(ds_above(L, flags, pos, cnt))
            sel_c.append(int(lines[1 + pos]))
    if left:
        for k in range(min(left_n, (1 + left_is4) << 1)):
            pos = start[1] + k * step[1]
            sel_l.append(ds_left(L, flags, pos, cnt))
            sel_c.append(int(lines[stride + 1 + pos]))
    if not (above or left):
        bump(cnt, "lm_nothing_available")
        return 0, 1 << (bit_depth - 1), 0
    assert len(sel_l) == 4, "with sides >= 4 the cnt == 2 branch (:1544) cannot be reached"
    mn, mx = [0, 2], [1, 3]
    if sel_l[mn[0]] > sel_l[mn[1]]:
        mn[0], mn[1] = mn[1], mn[0]
    if sel_l[mx[0]] > sel_l[mx[1]]:
        mx[0], mx[1] = mx[1], mx[0]
    if sel_l[mn[0]] > sel_l[mx[1]]:
        mn, mx = mx, mn
    if sel_l[mn[1]] > sel_l[mx[0]]:
        mn[1], mx[0] = mx[0], mn[1]
    min_l, min_c = (sel_l[mn[0]] + sel_l[mn[1]] + 1) >> 1, (sel_c[mn[0]] + sel_c[mn[1]] + 1) >> 1
    max_l, max_c = (sel_l[mx[0]] + sel_l[mx[1]] + 1) >> 1, (sel_c[mx[0]] + sel_c[mx[1]] + 1) >> 1
    diff = max_l - min_l
    if diff <= 0:
        bump(cnt, "diff_zero")
        return 0, min_c, 0
    diff_c = max_c - min_c
    x = log2i(diff)
    norm = ((diff << 4) >> x) & 15
    v = DIV_SIG_TABLE[norm] | 8
    x += 1 if norm else 0
    if diff_c == 0:
        bump(cnt, "diffc_zero")
    y = 0 if diff_c == 0 else log2i(abs(diff_c)) + 1
    add = (1 << y) >> 1
    a = (diff_c * v + add) >> y
    shift = 3 + x - y
    if shift < 1:
        shift = 1
        if a:
            bump(cnt, "shift_clamp_negative" if a < 0 else "shift_clamp_positive")
        a = 0 if a == 0 else (-15 if a < 0 else 15)
    if a < 0:
        bump(cnt, "a_negative")
    b = min_c - ((a * min_l) >> shift)
    return a, b, shift


def ds_block(L, w, h, flags, cnt=None):
    return np.array([[ds_inner(L, flags, i, j, cnt) for i in range(w)] for j in range(h)], np.int64)


def predict_lm(ds, a, b, shift, bit_depth, cnt=None):
    raw = ((a * ds) >> shift) + b
    vmax = (1 << bit_depth) - 1
    if raw.min() < 0:
        bump(cnt, "lm_clip_low")
    if raw.max() > vmax:
        bump(cnt, "lm_clip_high")
    return np.clip(raw, 0, vmax).astype(np.int16)


def chroma_cost(org, pred):
    """min( 2 * SAD, HAD ) of one component (:827-829)"""
    return min(IR.had(org, pred), 2 * int(np.abs(org.astype(np.int64) - pred.astype(np.int64)).sum()))


def mask_bits(mask):
    return [s for s in range(NUM_SLOTS) if (int(mask) >> s) & 1]


def run_item(it, luma, ref, org, cnt=None, touched=None):
    """one item -> ( costs uint32 [8], 0 where not requested; { slot: ( a, b, shift ) [2] } of its LM slots; { slot: predictions int16 [2][h][w] } of every requested slot )"""
    w, h, bd, flags = int(it["w"]), int(it["h"]), int(it["bit_depth"]), int(it["flags"])
    n_ar, n_lb = int(it["n_above_right"]), int(it["n_left_below"])
    bump(cnt, {0: "avail_none", F_ABOVE: "avail_above", F_LEFT: "avail_left", F_ABOVE | F_LEFT: "avail_both"}[flags & 3])
    bump(cnt, "ver_collocated_on" if flags & F_VER_COLLOCATED else "ver_collocated_off")
    lines = [ref[int(it["ref_off"][c]):int(it["ref_off"][c]) + line_len(w, h)] for c in (0, 1)]
    orgs = [org[int(it["org_off"][c]):int(it["org_off"][c]) + w * h].reshape(h, w) for c in (0, 1)]
    costs, prm, preds, ds = np.zeros(NUM_SLOTS, np.uint32), {}, {}, None
    for s in mask_bits(it["mode_mask"]):
        m = int(it["cand"][s])
        pp = []
        if m >= LM:
            L = Luma(luma, it["luma_off"], it["luma_stride"], touched)
            if ds is None:
                ds = ds_block(L, w, h, flags, cnt)
            prm[s] = [lm_params(L, lines[c], w, h, bd, flags, n_ar, n_lb, m, cnt) for c in (0, 1)]
            pp = [predict_lm(ds, *prm[s][c], bd, cnt) for c in (0, 1)]
        else:
            pp = [predict_regular(lines[c], w, h, m, bd, cnt if c == 0 else None) for c in (0, 1)]
        costs[s] = chroma_cost(orgs[0], pp[0]) + chroma_cost(orgs[1], pp[1])
        preds[s] = np.stack(pp)
    return costs, prm, preds


def run_items(items, luma, ref, org, cnt=None):
    """the entry on a list -> ( costs uint32 [n][8]; per item the concatenated predictions of its pred_mask per component, as the entry lays them out: ( Cb, Cr ) )"""
    costs, out = np.zeros((len(items), NUM_SLOTS), np.uint32), []
    for i, it in enumerate(items):
        c, _, preds = run_item(it, luma, ref, org, cnt)
        costs[i] = c
        want = mask_bits(it["pred_mask"])
        out.append(tuple(np.concatenate([preds[s][comp].reshape(-1) for s in want]) if want else np.zeros(0, np.int16) for comp in (0, 1)))
    return costs, out


def select(costs, cand, mode_mask, reduce_full_rd):
    """the reference's selection from the costs: the stable exchange sort of IntraSearch.cpp:847-857 over all eight slots (unscored slots keep cost 0, as in the reference) and
    the disable list of :859-862 -> ( the sorted mode list, the set of disabled modes )"""
    modes = [int(m) for m in cand]
    c = [int(costs[s]) if (int(mode_mask) >> s) & 1 else 0 for s in range(NUM_SLOTS)]
    for i in range(NUM_SLOTS):
        for j in range(i + 1, NUM_SLOTS):
            if c[j] < c[i]:
                modes[i], modes[j] = modes[j], modes[i]
                c[i], c[j] = c[j], c[i]
    n = NUM_SLOTS >> (1 if reduce_full_rd else 2)
    return modes, {modes[NUM_SLOTS - 1 - i] for i in range(n)}
