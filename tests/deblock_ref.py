"""numpy / Python restatement of the deblocking filter of a picture as the reference runs it once the boundary strengths are known:

area walk   LoopFilter::xDeblockArea<dir> (CommonLib/LoopFilter.cpp:405-462) over every CTU of the picture, EDGE_VER first, then EDGE_HOR (EncSlice.cpp:1020 / :1052)
luma        xEdgeFilterLuma (:1372-1520) with xUseStrongFiltering (:1318-1370), xFilteringPandQCore / xBilinearFilter (:100-201) and xPelFilterLumaCorePel (:217-264)
chroma      xEdgeFilterChroma (:1522-1635), 4:2:0, with xPelFilterChroma (:284-342)

It filters strictly in the reference's order — CTU by CTU, record by record, in place — unless it is handed a shuffled order (which, on legal maps, changes nothing:
tests/test_deblock_cpu.py), and it counts which branch every segment took.  The maps are arrays of LF_PARAM_DTYPE records, one per 4 x 4 luma unit:
[ height / 4 ][ width / 4 ], byte-compatible with LoopFilterParam (CommonLib/TypeDef.h:546-559).  tests/golden/deblock.npz pins it to the reference's own code
(tests/deblock_golden_gen.*)."""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "deblock.npz")

LF_PARAM_DTYPE = np.dtype([("qp", "i1", (3,)), ("bs", "u1"), ("side_max_filt_length", "u1"), ("flags", "u1")])      # vvhip_lf_param, 6 bytes
VER, HOR = 1, 2
FLAG_CMFL = 32

TC_TABLE = (0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 3, 4, 4, 4, 4, 5, 5, 5, 5, 7, 7, 8, 9, 10, 10, 11, 13, 14, 15, 17, 19, 21, 24, 25, 29, 33, 36, 41, 45, 51, 57, 64, 71, 80, 89,
            100, 112, 125, 141, 157, 177, 198, 222, 250, 280, 314, 352, 395)
BETA_TABLE = (0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 17, 18, 20, 22, 24, 26, 28, 30, 32, 34, 36, 38, 40, 42, 44, 46, 48, 50, 52, 54, 56, 58,
              60, 62, 64, 66, 68, 70, 72, 74, 76, 78, 80, 82, 84, 86, 88)
DB7, DB5, DB3 = (59, 50, 41, 32, 23, 14, 5), (58, 45, 32, 19, 6), (53, 32, 11)
TC7, TC3 = (6, 5, 4, 3, 2, 1, 1), (6, 4, 2)

LONG_PAIRS = ((7, 7), (7, 5), (5, 7), (7, 3), (3, 7), (5, 5), (5, 3), (3, 5))
LUMA_BRANCHES = ("none_beta", "weak_pq", "weak_p", "weak_q", "weak_0", "weak_refused", "strong") + tuple("long_%d_%d" % pq for pq in LONG_PAIRS)
CHROMA_BRANCHES = ("c_weak", "c_strong", "c_skip_bs1")
EITHER_DIR = LUMA_BRANCHES + CHROMA_BRANCHES + ("clip_lo", "clip_hi")
HOR_ONLY = ("c_strong_ctb", "ctu_p_rule")


def clip3(lo, hi, v):
    return lo if v < lo else hi if v > hi else v


def tc_of(qp, bs, tc_off, bd):
    t = TC_TABLE[clip3(0, 65, qp + 2 * (bs - 1) + 2 * tc_off)]
    return (t + (1 << (9 - bd))) >> (10 - bd) if bd < 10 else t << (bd - 10)


def beta_of(qp, beta_off, bd):
    return BETA_TABLE[clip3(0, 63, qp + 2 * beta_off)] << (bd - 8)


class _Line:
    """one line of samples across an edge: self[k] is the sample at offset k from the edge (k < 0: the P side); stores go to self.out"""

    def __init__(self, plane, x, y, ver, i):
        if ver:
            self.row, self.c = plane[y + i], x
        else:
            self.row, self.c = plane[:, x + i], y
        self.out = {}

    def __getitem__(self, k):
        assert 0 <= self.c + k < self.row.shape[0], "the filter reads outside the picture"
        return int(self.row[self.c + k])

    def flush(self):
        for k, v in self.out.items():
            self.row[self.c + k] = v


def _dp(s, at=0, ctb=False):
    return abs(s[at - 2] - 2 * s[at - 2] + s[at - 1]) if ctb else abs(s[at - 3] - 2 * s[at - 2] + s[at - 1])


def _dq(s, at=0):
    return abs(s[at] - 2 * s[at + 1] + s[at + 2])


def use_strong(s, d, beta, tc, p_large=False, q_large=False, lp=7, lq=7, ctb=False):
    m3, m4 = s[-1], s[0]
    shift = 4 if (p_large or q_large) else 2
    if not (d < (beta >> shift) and abs(m3 - m4) < ((tc * 5 + 1) >> 1)):
        return False
    sp3 = abs(s[-2] - m3) if ctb else abs(s[-4] - m3)
    sq3 = abs(s[3] - m4)
    if p_large or q_large:
        if p_large:
            mp4 = s[-lp - 1]
            if lp == 7:
                sp3 += abs(s[-5] - s[-6] - s[-7] + mp4)
            sp3 = (sp3 + abs(s[-4] - mp4) + 1) >> 1
        if q_large:
            m11 = s[lq]
            if lq == 7:
                sq3 += abs(s[4] - s[5] - s[6] + m11)
            sq3 = (sq3 + abs(m11 - s[3]) + 1) >> 1
        return sp3 + sq3 < (beta * 3 >> 5)
    return sp3 + sq3 < (beta >> 3)


def long_filter_line(s, n_p, n_q, tc):
    """xFilteringPandQCore for one line"""
    P = [s[-1 - j] for j in range(n_p + 1)]
    Q = [s[j] for j in range(n_q + 1)]
    cp = {7: DB7, 5: DB5, 3: DB3}[n_p]
    cq = {7: DB7, 5: DB5, 3: DB3}[n_q]
    ref_p, ref_q = (P[n_p - 1] + P[n_p] + 1) >> 1, (Q[n_q - 1] + Q[n_q] + 1) >> 1
    if n_p == n_q:
        if n_p == 5:
            mid = (2 * (P[0] + Q[0] + P[1] + Q[1] + P[2] + Q[2]) + P[3] + Q[3] + P[4] + Q[4] + 8) >> 4
        else:
            mid = (2 * (P[0] + Q[0]) + sum(P[1:7]) + sum(Q[1:7]) + 8) >> 4
    else:
        big, small = (P, Q) if n_p > n_q else (Q, P)      # the reference's srcPt / srcQt after the swap
        nb, ns = max(n_p, n_q), min(n_p, n_q)
        if nb == 7 and ns == 5:
            mid = (2 * (P[0] + Q[0] + P[1] + Q[1]) + P[2] + Q[2] + P[3] + Q[3] + P[4] + Q[4] + P[5] + Q[5] + 8) >> 4
        elif nb == 7 and ns == 3:
            mid = (2 * (big[0] + small[0]) + small[0] + 2 * (small[1] + small[2]) + big[1] + small[1] + big[2] + big[3] + big[4] + big[5] + big[6] + 8) >> 4
        else:
            mid = (P[0] + Q[0] + P[1] + Q[1] + P[2] + Q[2] + P[3] + Q[3] + 4) >> 3
    tp, tq = (TC3 if n_p == 3 else TC7), (TC3 if n_q == 3 else TC7)
    for j in range(n_p):
        cv = (tc * tp[j]) >> 1
        s.out[-1 - j] = clip3(P[j] - cv, P[j] + cv, (mid * cp[j] + ref_p * (64 - cp[j]) + 32) >> 6)
    for j in range(n_q):
        cv = (tc * tq[j]) >> 1
        s.out[j] = clip3(Q[j] - cv, Q[j] + cv, (mid * cq[j] + ref_q * (64 - cq[j]) + 32) >> 6)


class Counter(dict):
    def hit(self, key, n=1):
        self[key] = self.get(key, 0) + n


def _clip_pel(v, clip, cnt, tag):
    if v < clip[0]:
        cnt.hit(tag + "clip_lo")
        return clip[0]
    if v > clip[1]:
        cnt.hit(tag + "clip_hi")
        return clip[1]
    return v


def luma_line(s, tc, sw, thr, second_p, second_q, clip, cnt, tag):
    """xPelFilterLumaCorePel; -> False where the weak filter was refused by the threshold"""
    m1, m2, m3, m4, m5, m6 = s[-3], s[-2], s[-1], s[0], s[1], s[2]
    if sw:
        m0, m7 = s[-4], s[3]
        s.out[-3] = clip3(m1 - tc, m1 + tc, (2 * m0 + 3 * m1 + m2 + m3 + m4 + 4) >> 3)
        s.out[-2] = clip3(m2 - 2 * tc, m2 + 2 * tc, (m1 + m2 + m3 + m4 + 2) >> 2)
        s.out[-1] = clip3(m3 - 3 * tc, m3 + 3 * tc, (m1 + 2 * m2 + 2 * m3 + 2 * m4 + m5 + 4) >> 3)
        s.out[0] = clip3(m4 - 3 * tc, m4 + 3 * tc, (m2 + 2 * m3 + 2 * m4 + 2 * m5 + m6 + 4) >> 3)
        s.out[1] = clip3(m5 - 2 * tc, m5 + 2 * tc, (m3 + m4 + m5 + m6 + 2) >> 2)
        s.out[2] = clip3(m6 - tc, m6 + tc, (m3 + m4 + m5 + 3 * m6 + 2 * m7 + 4) >> 3)
        return True
    delta = (9 * (m4 - m3) - 3 * (m5 - m2) + 8) >> 4
    if abs(delta) >= thr:
        return False
    delta = clip3(-tc, tc, delta)
    tc2 = tc >> 1
    s.out[-1] = _clip_pel(m3 + delta, clip, cnt, tag)
    if second_p:
        s.out[-2] = _clip_pel(m2 + clip3(-tc2, tc2, (((m1 + m3 + 1) >> 1) - m2 + delta) >> 1), clip, cnt, tag)
    s.out[0] = _clip_pel(m4 - delta, clip, cnt, tag)
    if second_q:
        s.out[1] = _clip_pel(m5 + clip3(-tc2, tc2, (((m6 + m4 + 1) >> 1) - m5 - delta) >> 1), clip, cnt, tag)
    return True


def luma_segment(plane, x, y, ver, rec, ctu, bd, clip, beta_off, tc_off, cnt):
    """xEdgeFilterLuma: the four lines of the edge segment at luma ( x, y )"""
    tag = "V:" if ver else "H:"
    bs = int(rec["bs"]) & 3
    assert bs <= 2
    if not bs:
        return
    qp, ln = int(rec["qp"][0]), int(rec["side_max_filt_length"])
    lp, lq = (ln >> 4) & 7, ln & 7
    p_large, q_large = lp > 3, lq > 3
    if not ver and y % ctu == 0:
        if p_large:
            cnt.hit(tag + "ctu_p_rule")
        p_large = False
    tc, beta = tc_of(qp, bs, tc_off, bd), beta_of(qp, beta_off, bd)
    side, thr = (beta + (beta >> 1)) >> 3, tc * 10
    L = [_Line(plane, x, y, ver, i) for i in range(4)]
    dp0, dq0, dp3, dq3 = _dp(L[0]), _dq(L[0]), _dp(L[3]), _dq(L[3])
    d0, d3 = dp0 + dq0, dp3 + dq3
    if p_large or q_large:
        dp0l = (dp0 + _dp(L[0], -3) + 1) >> 1 if p_large else dp0
        dq0l = (dq0 + _dq(L[0], 3) + 1) >> 1 if q_large else dq0
        dp3l = (dp3 + _dp(L[3], -3) + 1) >> 1 if p_large else dp3
        dq3l = (dq3 + _dq(L[3], 3) + 1) >> 1 if q_large else dq3
        d0l, d3l = dp0l + dq0l, dp3l + dq3l
        if d0l + d3l < beta:
            if use_strong(L[0], 2 * d0l, beta, tc, p_large, q_large, lp, lq) and use_strong(L[3], 2 * d3l, beta, tc, p_large, q_large, lp, lq):
                n_p, n_q = (lp if p_large else 3), (lq if q_large else 3)
                for s in L:
                    long_filter_line(s, n_p, n_q, tc)
                    s.flush()
                cnt.hit(tag + "long_%d_%d" % (n_p, n_q))
                return
    if d0 + d3 >= beta:
        cnt.hit(tag + "none_beta")
        return
    second_p = second_q = False
    if lp > 1 and lq > 1:
        second_p, second_q = dp0 + dp3 < side, dq0 + dq3 < side
    sw = lp > 2 and lq > 2 and use_strong(L[0], 2 * d0, beta, tc) and use_strong(L[3], 2 * d3, beta, tc)
    done = 0
    for s in L:
        ok = luma_line(s, tc, sw, thr, second_p, second_q, clip, cnt, tag)
        done += ok
        if not ok:
            cnt.hit(tag + "weak_refused")
    for s in L:
        s.flush()
    if sw:
        cnt.hit(tag + "strong")
    elif done:
        cnt.hit(tag + ("weak_pq" if second_p and second_q else "weak_p" if second_p else "weak_q" if second_q else "weak_0"))


def chroma_line(s, tc, sw, clip, ctb, cnt, tag):
    """xPelFilterChroma"""
    m2, m3, m4, m5 = s[-2], s[-1], s[0], s[1]
    if sw:
        m6, m7 = s[2], s[3]
        if ctb:
            s.out[-1] = clip3(m3 - tc, m3 + tc, (3 * m2 + 2 * m3 + m4 + m5 + m6 + 4) >> 3)
            s.out[0] = clip3(m4 - tc, m4 + tc, (2 * m2 + m3 + 2 * m4 + m5 + m6 + m7 + 4) >> 3)
        else:
            m0, m1 = s[-4], s[-3]
            s.out[-3] = clip3(m1 - tc, m1 + tc, (3 * m0 + 2 * m1 + m2 + m3 + m4 + 4) >> 3)
            s.out[-2] = clip3(m2 - tc, m2 + tc, (2 * m0 + m1 + 2 * m2 + m3 + m4 + m5 + 4) >> 3)
            s.out[-1] = clip3(m3 - tc, m3 + tc, (m0 + m1 + m2 + 2 * m3 + m4 + m5 + m6 + 4) >> 3)
            s.out[0] = clip3(m4 - tc, m4 + tc, (m1 + m2 + m3 + 2 * m4 + m5 + m6 + m7 + 4) >> 3)
        s.out[1] = clip3(m5 - tc, m5 + tc, (m2 + m3 + m4 + 2 * m5 + m6 + 2 * m7 + 4) >> 3)
        s.out[2] = clip3(m6 - tc, m6 + tc, (m3 + m4 + m5 + 2 * m6 + 3 * m7 + 4) >> 3)
    else:
        delta = clip3(-tc, tc, (4 * (m4 - m3) + m2 - m5 + 4) >> 3)
        s.out[-1] = _clip_pel(m3 + delta, clip, cnt, tag)
        s.out[0] = _clip_pel(m4 - delta, clip, cnt, tag)


def chroma_segment(planes, cx, cy, ver, rec, ctu_c, bd, clips, beta_offs, tc_offs, cnt):
    """xEdgeFilterChroma, 4:2:0: the two lines of both chroma planes at chroma ( cx, cy ); planes / clips / offsets are those of Cb and Cr"""
    tag = "V:" if ver else "H:"
    large = bool(int(rec["flags"]) & FLAG_CMFL)
    ctb = (not ver) and (cy & (ctu_c - 1)) == 0
    for ci in (0, 1):
        bs = (int(rec["bs"]) >> (2 * (ci + 1))) & 3
        assert bs <= 2
        if not (bs == 2 or (large and bs == 1)):
            if bs == 1:
                cnt.hit(tag + "c_skip_bs1")
            continue
        qp = int(rec["qp"][ci + 1])
        tc = tc_of(qp, bs, tc_offs[ci], bd)
        L = [_Line(planes[ci], cx, cy, ver, i) for i in range(2)]
        sw = False
        if large:
            beta = beta_of(qp, beta_offs[ci], bd)
            d0, d3 = _dp(L[0], 0, ctb) + _dq(L[0]), _dp(L[1], 0, ctb) + _dq(L[1])
            if d0 + d3 < beta:
                sw = use_strong(L[0], 2 * d0, beta, tc, ctb=ctb) and use_strong(L[1], 2 * d3, beta, tc, ctb=ctb)
        for s in L:
            chroma_line(s, tc, sw, clips[ci], ctb, cnt, tag)
        for s in L:
            s.flush()
        cnt.hit(tag + ("c_strong_ctb" if sw and ctb else "c_strong" if sw else "c_weak"))


def segments(width, height, ctu, lfp, ver, chroma, rows=None):
    """the area walk of xDeblockArea<dir> over the CTUs of CTU rows `rows` = ( first, count ) (None: the picture), in the reference's order
    -> list of ( 'L' or 'C', luma x, luma y, record )"""
    gx, gy = -(-width // ctu), -(-height // ctu)
    r0, n = (0, gy) if rows is None else rows
    ctu_c, out = ctu >> 1, []
    for cy in range(r0, r0 + n):
        for cx in range(gx):
            x0, y0 = cx * ctu, cy * ctu
            w, h = min(ctu, width - x0), min(ctu, height - y0)
            for dy in range(0, h, 4):
                dy_in = ((y0 >> 1) + (dy >> 1)) & (ctu_c - 1)
                for dx in range(0, w, 4):
                    rec = lfp[(y0 + dy) >> 2, (x0 + dx) >> 2]
                    bs = int(rec["bs"])
                    if bs & 3:
                        out.append(("L", x0 + dx, y0 + dy, rec))
                    dx_in = ((x0 >> 1) + (dx >> 1)) & (ctu_c - 1)
                    if chroma and ((dx_in & 7) == 0 if ver else (dy_in & 7) == 0) and (bs >> 2) & 15:
                        out.append(("C", x0 + dx, y0 + dy, rec))
    return out


def deblock(planes, lfp_ver, lfp_hor, ctu, bit_depth, clip=None, beta_offsets=(0, 0, 0), tc_offsets=(0, 0, 0), dirs=3, rows=None, counters=None, shuffle=None):
    """-> the filtered planes (new arrays, int16).  planes: [ luma ] or [ luma, cb, cr ] (4:2:0).  shuffle: a numpy Generator that permutes the segments of each direction"""
    out = [np.array(p, np.int16) for p in planes]
    H, W = out[0].shape
    clip = [(0, (1 << bit_depth) - 1)] * len(out) if clip is None else clip
    cnt = Counter() if counters is None else counters
    for bit, lfp in ((VER, lfp_ver), (HOR, lfp_hor)):
        if not dirs & bit:
            continue
        ver = bit == VER
        segs = segments(W, H, ctu, lfp, ver, len(out) == 3, rows)
        if shuffle is not None:
            segs = [segs[i] for i in shuffle.permutation(len(segs))]
        for kind, x, y, rec in segs:
            if kind == "L":
                luma_segment(out[0], x, y, ver, rec, ctu, bit_depth, clip[0], beta_offsets[0], tc_offsets[0], cnt)
            else:
                chroma_segment(out[1:], x >> 1, y >> 1, ver, rec, ctu >> 1, bit_depth, clip[1:], beta_offsets[1:], tc_offsets[1:], cnt)
    return out


def coverage(cnt):
    """what the counters of all cases together must show; -> the missing keys"""
    want = ["%s:%s" % (d, k) for d in "VH" for k in EITHER_DIR] + ["H:" + k for k in HOR_ONLY]
    return [k for k in want if not cnt.get(k)]
