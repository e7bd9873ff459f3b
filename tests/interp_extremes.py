"""Deterministic extreme inputs of the sub-pel interpolation entries (table-slot passes, copy forms, batched luma / chroma prediction blocks, sub-pel candidate
distortion, pattern refinement, the plain prediction list), shared by the CPU tier (tests/test_oracle_interp_extremes.py: oracle against the compiled reference)
and the GPU tier (tests/test_gpu_interp_extremes.py: every kernel form against the oracle).

The pictures of the parity suites (sinusoids with noise, one uniform-random 10-bit plane) never drive a filter into its clips.  These do: a two-level plane of
(0, 2^bd - 1) whose 8-periodic column pattern puts the maximum under a tap row's positive taps and 0 under its negative ones gives the largest sum that row can
produce (the complement the smallest), so a single last pass overshoots both clips, a first pass reaches both ends of its 14-bit range, and on the separable 2-D
version (rows under a positive vertical tap carry the pattern, rows under a negative one its complement) the second pass reaches its largest and smallest sum.
A pattern depends on the SIGNS of a tap row only, so there is one plane per sign signature (four for the 8-tap set, one for the 6-tap set, three for chroma)
and not one per phase.  A sample meets the bound where its column (and row) is 3 modulo 8: one in 64 samples of a block.

The int64 model below restates one pass (sum, offset, shift, a switchable truncation to int16, a switchable clip) and the two-pass compositions.  It computes
the guards of the CPU tier and the mutations of its sensitivity test; expected values of the tests come from the oracle or the compiled reference, never from
it.  Numpy only: no GPU, no oracle, no reference.  The tap tables are restated from InterpolationFilter.cpp:64-163 (the CPU tier compares them with
oracle.if_coeff and the reference's own rows for every set and phase).
"""
from functools import lru_cache

import numpy as np

BITDEPTHS = (8, 10, 12)
PLANE_H, PLANE_W = 88, 152              # multiples of 8 (stacked planes keep their row residues); a 128x64 block with a margin of 11 fits
ORIGIN = (11, 11)                       # (x, y): block origin 3 modulo 8 — sample (0, 0) of the block meets the bound
OFF_ORIGIN = (14, 9)                    # an origin off that residue
SLOT_H, SLOT_W = 32, 48                 # planes of the one-pass entries (blocks up to 24x9 at ORIGIN)
SLOT_SIZES = ((1, 9), (5, 9), (24, 9))

# ---- tap tables (InterpolationFilter.cpp): phases 0 .. P/2, row P - p is row p reversed ---------------------------------------
LUMA8, LUMA6, CHROMA4, ALT, BILINEAR = 0, 1, 2, 3, 4            # the set numbers of oracle.if_coeff
SET_NAMES = ("luma8", "luma6", "chroma4", "alt", "bilinear")
_LUMA8_HALF = ((0, 0, 0, 64, 0, 0, 0, 0), (0, 1, -3, 63, 4, -2, 1, 0), (-1, 2, -5, 62, 8, -3, 1, 0), (-1, 3, -8, 60, 13, -4, 1, 0), (-1, 4, -10, 58, 17, -5, 1, 0),
               (-1, 4, -11, 52, 26, -8, 3, -1), (-1, 3, -9, 47, 31, -10, 4, -1), (-1, 4, -11, 45, 34, -10, 4, -1), (-1, 4, -11, 40, 40, -11, 4, -1))      # m_lumaFilter :85-104
_LUMA6_HALF = ((0, 0, 0, 64, 0, 0, 0, 0), (0, 1, -3, 63, 4, -2, 1, 0), (0, 1, -5, 62, 8, -3, 1, 0), (0, 2, -8, 60, 13, -4, 1, 0), (0, 3, -10, 58, 17, -5, 1, 0),
               (0, 3, -11, 52, 26, -8, 2, 0), (0, 2, -9, 47, 31, -10, 3, 0), (0, 3, -11, 45, 34, -10, 3, 0), (0, 3, -11, 40, 40, -11, 3, 0))                # m_lumaFilter4x4 :64-83
_ALT_HPEL = (0, 3, 9, 20, 20, 9, 3, 0)                                                                                                                     # m_lumaAltHpelIFilter :106
_CHROMA_HALF = ((0, 64, 0, 0), (-1, 63, 2, 0), (-2, 62, 4, 0), (-2, 60, 7, -1), (-2, 58, 10, -2), (-3, 57, 12, -2), (-4, 56, 14, -2), (-4, 55, 15, -2), (-4, 54, 16, -2),
                (-5, 53, 18, -2), (-6, 52, 20, -2), (-6, 49, 24, -3), (-6, 46, 28, -4), (-5, 44, 29, -4), (-4, 42, 30, -4), (-4, 39, 33, -4), (-4, 36, 36, -4))  # m_chromaFilter :107-142


def table_row(set_, phase, mirror=True):
    """the table row as the reference passes it: 8 entries for the luma sets and the alternative half-sample row, 4 for chroma (phase in 1/32), 2 for the bilinear
    pair (m_bilinearFilterPrec4 :144-163: { 16 - p, p }).  mirror=False is a mutation: the stored row of the mirrored phase, not reversed"""
    if set_ in (LUMA8, LUMA6):
        t = _LUMA8_HALF if set_ == LUMA8 else _LUMA6_HALF
        return tuple(t[phase]) if phase <= 8 else (tuple(t[16 - phase][::-1]) if mirror else tuple(t[16 - phase]))
    if set_ == CHROMA4:
        return tuple(_CHROMA_HALF[phase]) if phase <= 16 else (tuple(_CHROMA_HALF[32 - phase][::-1]) if mirror else tuple(_CHROMA_HALF[32 - phase]))
    if set_ == ALT:
        return _ALT_HPEL
    if set_ == BILINEAR:
        return (16 - phase, phase)
    raise ValueError(set_)


def ntaps(set_):
    """the tap count the reference filters with (6-tap cores skip the row's first entry, :361-364)"""
    return (8, 6, 4, 6, 2)[set_]


def phases(set_):
    """the non-zero phases of a set"""
    return {LUMA8: range(1, 16), LUMA6: range(1, 16), CHROMA4: range(1, 32), ALT: (8,), BILINEAR: range(1, 16)}[set_]


def window(set_, phase, mirror=True):
    """(c, lo): c[k] multiplies sample[pos - lo + k]"""
    row, n = table_row(set_, phase, mirror), ntaps(set_)
    return (row[1:7], 2) if n == 6 else (row, n // 2 - 1)


def sig8(set_, phase):
    """the signs of a tap row on the 8-entry window pos - 3 .. pos + 4, continued with the row's own period for the 4- and 2-tap sets (so that every fourth / second
    column matches them)"""
    c, lo = window(set_, phase)
    n = len(c)
    if n >= 6:
        s = [0] * 8
        for k, v in enumerate(c):
            s[3 - lo + k] = (v > 0) - (v < 0)
        return tuple(s)
    return tuple((c[(j - (3 - lo)) % n] > 0) - (c[(j - (3 - lo)) % n] < 0) for j in range(8))


SIG_ZERO = (0, 0, 0, 1, 0, 0, 0, 0)            # phase 0: the one-tap set { 64 }
FULL_SIG = (-1, 1, -1, 1, 1, -1, 1, -1)         # the 8-tap rows of phases 5 .. 11: no zero tap, so the complement plane is the exact complement


def signatures(set_):
    """{signature: [phases]} of the non-zero phases"""
    out = {}
    for p in phases(set_):
        out.setdefault(sig8(set_, p), []).append(p)
    return out


def tap_sums(set_, phase):
    """(S+, S-): the sums of the row's positive and negative taps"""
    c = window(set_, phase)[0]
    return sum(v for v in c if v > 0), sum(v for v in c if v < 0)


# ---- planes ------------------------------------------------------------------------------------------------------------------
def _ro(v):
    """planes are cached and shared between the tests: nobody writes to them"""
    return np.ascontiguousarray(v, np.int16)


def _levels(m01, hi, lo):
    return np.where(m01, hi, lo)


@lru_cache(maxsize=None)
def matched(sig, hi, lo, complement=False, vertical=False, h=SLOT_H, w=SLOT_W):
    """the matched two-level plane of a signature: `hi` in the columns (rows when vertical: the transpose) under a positive tap, `lo` elsewhere; complement: `hi` under
    the negative taps.  A sample whose column (row) is 3 modulo 8 sees the full match"""
    s = np.array(sig)
    p = (s < 0) if complement else (s > 0)
    yy, xx = np.mgrid[0:h, 0:w]
    return _ro(_levels(p[(yy if vertical else xx) % 8], hi, lo))


@lru_cache(maxsize=None)
def separable(sig_h, sig_v, mx, complement=False, h=PLANE_H, w=PLANE_W):
    """rows under a positive vertical tap carry the horizontally matched pattern, rows under a negative one its complement (rows under a zero tap: 0): the sample at
    column and row 3 modulo 8 has the largest second-pass sum; complement: the smallest"""
    yy, xx = np.mgrid[0:h, 0:w]
    prod = np.array(sig_h)[xx % 8] * np.array(sig_v)[yy % 8]
    return _ro(_levels((prod < 0) if complement else (prod > 0), mx, 0))


FILLERS = ("checker", "col_stripe", "row_stripe", "blocks4", "random", "const_0", "const_max")


@lru_cache(maxsize=None)
def filler(kind, hi, lo, h=PLANE_H, w=PLANE_W, seed=0):
    """the usual two-level fillers: checkerboard, one column / one row in eight, 4x4 blocks of alternating extremes, random of the two levels, the constants"""
    yy, xx = np.mgrid[0:h, 0:w]
    if kind == "checker":
        m = (xx + yy) & 1
    elif kind == "col_stripe":
        m = xx % 8 == 3
    elif kind == "row_stripe":
        m = yy % 8 == 3
    elif kind == "blocks4":
        m = ((xx >> 2) + (yy >> 2)) & 1
    elif kind == "random":
        m = np.random.default_rng(4100 + seed).integers(0, 2, (h, w))
    elif kind == "const_0":
        m = np.zeros((h, w), bool)
    elif kind == "const_max":
        m = np.ones((h, w), bool)
    else:
        raise ValueError(kind)
    return _ro(_levels(m.astype(bool), hi, lo))


class Atlas:
    """planes of one size stacked vertically (PLANE_H is a multiple of 8: every plane keeps its row residues), so that one launch reads blocks of many planes"""

    def __init__(self, planes):
        self.keys = [k for k, _ in planes]
        self.arr = _ro(np.concatenate([p for _, p in planes], axis=0))
        self._row = {k: i * PLANE_H for i, k in enumerate(self.keys)}

    def row(self, key):
        return self._row[key]


def family_sigs(family):
    """the signatures a block of a family can meet: the set's own, the one-tap set of phase 0 and, for luma, the alternative half-sample row"""
    sets = {"luma8": (LUMA8, ALT), "luma6": (LUMA6, ALT), "chroma4": (CHROMA4,)}[family]
    out = [SIG_ZERO]
    for s in sets:
        out += [g for g in signatures(s) if g not in out]
    return out


@lru_cache(maxsize=None)
def atlas(bd, family):
    """every separable plane (pair of signatures, matched and complement) of a family plus the fillers; keys ("sep", sig_h, sig_v, complement) and ("fill", kind)"""
    mx = (1 << bd) - 1
    sigs = family_sigs(family)
    planes = [(("sep", a, b, c), separable(a, b, mx, c)) for a in sigs for b in sigs for c in (False, True)]
    planes += [(("fill", k), filler(k, mx, 0)) for k in FILLERS]
    return Atlas(planes)


@lru_cache(maxsize=None)
def org_atlas(bd):
    """original planes of the distortion entries: the same two-level kinds"""
    mx = (1 << bd) - 1
    planes = [(("fill", k), filler(k, mx, 0, seed=5)) for k in FILLERS]
    planes += [(("sep", c), separable(FULL_SIG, FULL_SIG, mx, c)) for c in (False, True)]
    return Atlas(planes)


# ---- the int64 model ---------------------------------------------------------------------------------------------------------
MUTATIONS = ("no_round", "no_upper_clip", "no_lower_clip", "no_mirror", "8tap_4x4", "6tap_4x8", "alt_both", "no_alt_me", "chroma_not_doubled", "copy_no_bias")


def headroom(bd):
    return max(2, 14 - bd)


def pass_geom(n, first, last, bd, mut=()):
    """(shift, offset) of one pass (InterpolationFilter.cpp:388-423)"""
    hr = headroom(bd)
    if n == 2:                                   # IF_FILTER_PREC_BILINEAR 4, IF_INTERNAL_PREC_BILINEAR 10
        shift = 4 - (10 - bd) if first else 4
        return shift, 1 << (shift - 1)
    shift = 6
    if last:
        shift += 0 if first else hr
        return shift, (0 if "no_round" in mut else 1 << (shift - 1)) + (0 if first else 8192 << 6)
    shift -= hr if first else 0
    return shift, -(8192 << shift) if first else 0


def wrap16(v):
    return ((v + 32768) & 0xffff) - 32768


def finish(raw, clip_max, mut=(), trunc=True):
    v = wrap16(raw) if trunc else raw
    if clip_max is not None:
        if "no_lower_clip" not in mut:
            v = np.maximum(v, 0)
        if "no_upper_clip" not in mut:
            v = np.minimum(v, clip_max)
    return v


def one_pass(a, y, x, w, h, c, lo, vertical, first, last, bd, mut=(), trunc=True, n=None, tr=None, tag="raw"):
    """one pass over the w x h block at (x, y) of the int64 array a -> int64 block; tr[tag] receives the value before truncation and clip"""
    acc = np.zeros((h, w), np.int64)
    for k, v in enumerate(c):
        dy, dx = (k - lo, 0) if vertical else (0, k - lo)
        acc += v * a[y + dy:y + dy + h, x + dx:x + dx + w]
    shift, offset = pass_geom(len(c) if n is None else n, first, last, bd, mut)
    raw = (acc + offset) >> shift
    if tr is not None:
        tr[tag] = raw
    return finish(raw, (1 << bd) - 1 if last else None, mut, trunc)


def copy_form(a, y, x, w, h, first, last, bd, bi_mc=False, mut=(), tr=None, tag="raw"):
    """filterCopy<isFirst, isLast> (:255-333)"""
    s = a[y:y + h, x:x + w].astype(np.int64)
    sh = headroom(bd)
    if bool(first) == bool(last):
        return s
    if first:
        if bi_mc:
            return wrap16(s << (10 - bd))
        return wrap16(wrap16(s << sh) - (0 if "copy_no_bias" in mut else 8192))
    raw = (s + wrap16(np.int64((1 << (sh - 1)) + 8192))) >> sh
    if tr is not None:
        tr[tag] = raw
    return finish(raw, (1 << bd) - 1, mut)


def _two_pass(a, y, x, w, h, wh, wv, rnd, bd, mut, tr, trunc=True):
    """horizontal (isFirst, !isLast) over the rows the vertical taps reach, then vertical (!isFirst, isLast = rnd)"""
    (ch, loh), (cv, lov) = wh, wv
    rows = h + len(cv) - 1
    tmp = one_pass(a, y - lov, x, w, rows, ch, loh, False, True, False, bd, mut, trunc, tr=tr, tag="raw1")
    return one_pass(tmp, lov, 0, w, h, cv, lov, True, False, rnd, bd, mut, trunc, tr=tr, tag="raw2")


def luma_set_pred(w, h, frac, both, alt, mut=()):
    """the tap set xPredInterBlk reaches: filter4x4 swaps the alternative row in for BOTH directions whatever the phase (:692-693); the other fused entries and the
    1-D dispatch only at phase 8 (:719-720, :570-580)"""
    is4 = w == 4 and h == 4
    six = (is4 and "8tap_4x4" not in mut) or ("6tap_4x8" in mut and w == 4 and h == 8)
    if alt and ((is4 or "alt_both" in mut) and both or frac == 8):
        return ALT
    return LUMA6 if six else LUMA8


def pred_luma(a, y, x, w, h, xf, yf, rnd, bd, alt=False, mut=(), tr=None, trunc=True):
    """xPredInterBlk for luma (InterPrediction.cpp:832-865): copy, one pass, or two passes"""
    a = a.astype(np.int64) if a.dtype != np.int64 else a
    mirror = "no_mirror" not in mut
    both = xf != 0 and yf != 0
    if not xf and not yf:
        return copy_form(a, y, x, w, h, True, rnd, bd, False, mut)
    if not both:
        f = xf or yf
        c, lo = window(luma_set_pred(w, h, f, False, alt, mut), f, mirror)
        return one_pass(a, y, x, w, h, c, lo, not xf, True, rnd, bd, mut, trunc, tr=tr, tag="raw2")
    return _two_pass(a, y, x, w, h, window(luma_set_pred(w, h, xf, True, alt, mut), xf, mirror), window(luma_set_pred(w, h, yf, True, alt, mut), yf, mirror), rnd, bd, mut, tr, trunc)


def luma_set_me(w, h, frac, vertical, alt, reduce_tap, mut=()):
    """filterHor / filterVer for luma with m_meReduceTap (:557-601, :617-661) -> (set, phase in that set's units)"""
    if reduce_tap == 0 or (alt and frac == 8 and "no_alt_me" not in mut):
        if alt and frac == 8:
            return ALT, frac
        if (w == 4 and h == 4) or (not vertical and w == 4 and h == 4 + 7):
            return LUMA6, frac
        return LUMA8, frac
    if reduce_tap == 1:
        return LUMA6, frac
    return CHROMA4, frac if "chroma_not_doubled" in mut else frac << 1


def pred_luma_me(a, y, x, w, h, xf, yf, bd, alt=False, reduce_tap=0, mut=(), tr=None):
    """the ME form (InterSearch.cpp:818-848): horizontal with isLast = false over h + 7 rows, then vertical isFirst = false, isLast = true; copy forms at phase 0"""
    a = a.astype(np.int64) if a.dtype != np.int64 else a
    mirror = "no_mirror" not in mut
    rows = h + 7
    if xf:
        c, lo = window(*luma_set_me(w, rows, xf, False, alt, reduce_tap, mut), mirror)
        tmp = one_pass(a, y - 3, x, w, rows, c, lo, False, True, False, bd, mut, tr=tr, tag="raw1")
    else:
        tmp = copy_form(a, y - 3, x, w, rows, True, False, bd, False, mut)
    if yf:
        c, lo = window(*luma_set_me(w, h, yf, True, alt, reduce_tap, mut), mirror)
        return one_pass(tmp, 3, 0, w, h, c, lo, True, False, True, bd, mut, tr=tr, tag="raw2")
    return copy_form(tmp, 3, 0, w, h, False, True, bd, False, mut, tr=tr, tag="raw2")


def pred_chroma(a, y, x, w, h, xf, yf, rnd, bd, mut=(), tr=None):
    """the chroma composition of tests/pred_ref.py (xPredInterBlk with the 4-tap set, fractions in 1/32)"""
    a = a.astype(np.int64) if a.dtype != np.int64 else a
    mirror = "no_mirror" not in mut
    if not xf and not yf:
        return copy_form(a, y, x, w, h, True, rnd, bd, False, mut)
    if xf and yf:
        return _two_pass(a, y, x, w, h, window(CHROMA4, xf, mirror), window(CHROMA4, yf, mirror), rnd, bd, mut, tr)
    c, lo = window(CHROMA4, xf or yf, mirror)
    return one_pass(a, y, x, w, h, c, lo, not xf, True, rnd, bd, mut, tr=tr, tag="raw2")


def add_avg(p0, p1, bd, tr=None):
    """AreaBuf<Pel>::addAvg of two 14-bit blocks (Buffer.cpp:129-141)"""
    sh = headroom(bd) + 1
    raw = (p0.astype(np.int64) + p1.astype(np.int64) + (1 << (sh - 1)) + 2 * 8192) >> sh
    if tr is not None:
        tr["avg"] = raw
    return np.clip(raw, 0, (1 << bd) - 1)


def first_pass_bounds(set_, phase, bd):
    """the two reachable extremes of a first (not last) pass on samples 0 .. 2^bd - 1: (max S+ >> s1) - 8192 and (max S- >> s1) - 8192 for the 8 / 6 / 4-tap sets"""
    mx = (1 << min(bd, 10) if set_ == BILINEAR else 1 << bd) - 1
    sp, sn = tap_sums(set_, phase)
    shift, offset = pass_geom(ntaps(set_), True, False, min(bd, 10) if set_ == BILINEAR else bd)
    return (mx * sp + offset) >> shift, (mx * sn + offset) >> shift


def second_pass_bounds(wh, wv, rnd, bd):
    """the largest and the smallest value of the second pass (before truncation and clip) over all in-range inputs, for the tap rows wh then wv"""
    mx = (1 << bd) - 1
    s1, o1 = pass_geom(8, True, False, bd)
    fp, fn = (mx * sum(v for v in wh if v > 0) + o1) >> s1, (mx * sum(v for v in wh if v < 0) + o1) >> s1
    vp, vn = sum(v for v in wv if v > 0), sum(v for v in wv if v < 0)
    s2, o2 = pass_geom(8, False, rnd, bd)
    return (vp * fp + vn * fn + o2) >> s2, (vp * fn + vn * fp + o2) >> s2


def inter_levels(set_, bd):
    """(hi, lo): the largest and smallest first-pass output any phase of the set reaches: the two levels of the not-first inputs"""
    b = [first_pass_bounds(set_, p, bd) for p in phases(set_)]
    return max(v[0] for v in b), min(v[1] for v in b)


def assert_no_wrap():
    """for in-range samples no pass wraps int16: S+ <= 88 and S- >= -24 for luma, S+ <= 74 and S- >= -10 for chroma; first-pass values within +-14 335 and the second
    pass with rnd 0 within +-25 080 at every bit depth.  Returns the extremes found"""
    f_hi = f_lo = s_hi = s_lo = 0
    for set_ in (LUMA8, LUMA6, CHROMA4, ALT):
        for p in phases(set_):
            sp, sn = tap_sums(set_, p)
            assert sp + sn == 64, (set_, p)
            assert (sp <= 74 and sn >= -10) if set_ == CHROMA4 else (sp <= 88 and sn >= -24), (set_, p, sp, sn)
            for bd in BITDEPTHS:
                hi, lo = first_pass_bounds(set_, p, bd)
                f_hi, f_lo = max(f_hi, hi), min(f_lo, lo)
                assert -14335 <= lo <= hi <= 14335, (set_, p, bd, hi, lo)
                for set_v in ((CHROMA4,) if set_ == CHROMA4 else (LUMA8, LUMA6, CHROMA4, ALT)):      # the ME form pairs any luma row with any other
                    for q in phases(set_v):
                        for rnd in (0, 1):
                            hi2, lo2 = second_pass_bounds(window(set_, p)[0], window(set_v, q)[0], rnd, bd)
                            assert -32768 <= lo2 <= hi2 <= 32767, (set_, p, set_v, q, rnd, bd, hi2, lo2)
                            if not rnd:
                                s_hi, s_lo = max(s_hi, hi2), min(s_lo, lo2)
    assert -25100 <= s_lo <= s_hi <= 25100, (s_hi, s_lo)          # 25 079 and -25 085, both at 12 bits with the half-sample row in both directions
    return f_hi, f_lo, s_hi, s_lo


# ---- cases shared by the two tiers -------------------------------------------------------------------------------------------
def slot_cases(bd):
    """the one-pass table-slot entry: (set, phase, vertical, first, last, name, plane, w, h, in_range) at ORIGIN.  First passes read sample planes (matched to the row's
    signature, its complement, two fillers); not-first passes read two-level planes of the reachable first-pass extremes and, as the set beyond the contract
    (in_range False), of 32767 / -32768.  Width 24 on every plane, widths 1 and 5 on the matched ones"""
    mx = (1 << bd) - 1
    for set_ in (LUMA8, LUMA6, CHROMA4, ALT, BILINEAR):
        hi, lo = inter_levels(set_, bd)
        for p in phases(set_):
            sig = sig8(set_, p)
            for vertical in (0, 1):
                for first, last in ((1, 1), (1, 0), (0, 1), (0, 0)):
                    if set_ == BILINEAR and first and bd > 10:
                        continue                          # documented rejection: the bilinear first pass exists up to 10 bits (IF_INTERNAL_PREC_BILINEAR)
                    a, b = (mx, 0) if first else (hi, lo)
                    planes = [("matched", matched(sig, a, b, False, bool(vertical)), True), ("complement", matched(sig, a, b, True, bool(vertical)), True),
                              ("random", filler("random", a, b, SLOT_H, SLOT_W, p), True), ("blocks4", filler("blocks4", a, b, SLOT_H, SLOT_W), True)]
                    if not first:
                        planes += [("int16", matched(sig, 32767, -32768, False, bool(vertical)), False), ("int16_c", matched(sig, 32767, -32768, True, bool(vertical)), False)]
                    for name, pl, ok in planes:
                        for (w, h) in (SLOT_SIZES if name in ("matched", "complement") else SLOT_SIZES[2:]):
                            yield set_, p, vertical, first, last, name, pl, w, h, ok


def copy_cases(bd):
    """filterCopy: (first, last, bi_mc, name, plane, w, h, in_range) at ORIGIN; the four modes are copy, first-not-last, last-not-first and DMVR's first pass"""
    mx = (1 << bd) - 1
    hi, lo = inter_levels(LUMA8, bd)
    for first, last, bi in ((1, 1, 0), (0, 0, 0), (1, 0, 0), (0, 1, 0), (1, 0, 1)):
        if bi and bd > 10:
            continue                                      # a left shift by 10 - bitDepth: DMVR's search exists up to 10 bits
        a, b = (mx, 0) if first or not last else (hi, lo)          # the plain copy (first == last) reads samples
        planes = [("random", filler("random", a, b, SLOT_H, SLOT_W, 1), True), ("checker", filler("checker", a, b, SLOT_H, SLOT_W), True), ("const_hi", filler("const_max", a, b, SLOT_H, SLOT_W), True)]
        if not first:
            planes.append(("int16", filler("random", 32767, -32768, SLOT_H, SLOT_W, 2), False))
        if not first and not last:
            planes.append(("inter", filler("random", hi, lo, SLOT_H, SLOT_W, 3), False))          # 14-bit values through the plain copy: beyond what a copy of samples is asked for
        for name, pl, ok in planes:
            for (w, h) in SLOT_SIZES:
                yield first, last, bi, name, pl, w, h, ok


ALL16 = tuple((xf, yf) for yf in range(16) for xf in range(16))
ALL32 = tuple((xf, yf) for yf in range(32) for xf in range(32))
SOME16 = ((0, 0), (8, 8), (8, 0), (0, 8), (5, 11), (15, 13), (1, 15), (12, 4), (4, 8), (13, 0), (0, 2), (9, 9), (14, 1))
SOME32 = tuple((p, (7 * p + 3) % 32) for p in range(32)) + ((0, 0), (16, 16), (0, 16), (16, 0), (31, 31), (1, 0), (0, 31))      # every phase once in each direction


def _sig_of(set_phase):
    set_, p = set_phase
    return sig8(set_, p) if p else SIG_ZERO


def luma_block_sigs(w, h, xf, yf, alt, mode):
    """the signatures of the rows a luma block meets in the two directions (mode 0: xPredInterBlk; 1 / 2: the ME form with that m_meReduceTap)"""
    both = xf != 0 and yf != 0
    if mode == 0:
        return _sig_of((luma_set_pred(w, h, xf, both, alt), xf)), _sig_of((luma_set_pred(w, h, yf, both, alt), yf))
    return _sig_of(luma_set_me(w, h + 7, xf, False, alt, mode) if xf else (0, 0)), _sig_of(luma_set_me(w, h, yf, True, alt, mode) if yf else (0, 0))


LUMA_FAMILY = {0: "luma8", 1: "luma6", 2: "chroma4"}


def luma_family(w, h, mode):
    return "luma6" if mode == 0 and w == 4 and h == 4 else LUMA_FAMILY[mode]


def _family_key(fam, sh, sv, comp):
    """the separable plane of a pair of signatures; a signature the family does not hold (the alternative row in the 4-tap family) falls back to a filler"""
    sigs = family_sigs(fam)
    return ("sep", sh, sv, comp) if sh in sigs and sv in sigs else ("fill", "blocks4" if comp else "random")


def luma_groups(bd):
    """batched luma prediction blocks: groups (w, h, mode, alt, rnd, family, blocks) with blocks = [(plane key, x, y, xf, yf)] — one launch each.  16x16 and 4x4 run all
    256 phases on the separable planes of their signatures (matched and complement); the other sizes a phase list on matched, complement and a filler, at an origin
    on the residue that meets the bounds and at one off it; the alternative half-sample filter where a phase is 8.  rnd 0 exists for mode 0 only (the ME form always
    ends with a last pass).  Block counts are odd: not a multiple of the blocks a workgroup takes"""
    for (w, h) in ((4, 4), (4, 8), (4, 16), (8, 4), (8, 8), (16, 16), (64, 64), (128, 8)):
        for mode in (0, 1, 2):
            if mode and (w, h) not in ((4, 4), (8, 8), (16, 16)):
                continue
            fam = luma_family(w, h, mode)
            full = (w, h) in ((4, 4), (16, 16)) if mode == 0 else (w, h) == (8, 8)
            for alt in (0, 1):
                for rnd in ((1, 0) if mode == 0 else (1,)):
                    blocks = []
                    for xf, yf in (ALL16 if full else SOME16):
                        if alt and 8 not in (xf, yf) and not (full and (w, h) == (4, 4) and xf and yf and (xf + yf) % 5 == 0):
                            continue                      # alt changes nothing off phase 8 — except in filter4x4, where a fifth of the phase pairs checks it
                        sh, sv = luma_block_sigs(w, h, xf, yf, alt, mode)
                        for comp in (False, True):
                            blocks.append((_family_key(fam, sh, sv, comp), ORIGIN[0], ORIGIN[1], xf, yf))
                        if not full:
                            blocks.append((_family_key(fam, sh, sv, False), OFF_ORIGIN[0], OFF_ORIGIN[1], xf, yf))
                            blocks.append((("fill", "random"), ORIGIN[0], ORIGIN[1], xf, yf))
                    blocks.append((("fill", "checker"), OFF_ORIGIN[0], OFF_ORIGIN[1], 8, 8))
                    assert len(blocks) % 2 == 1
                    yield w, h, mode, alt, rnd, fam, blocks


def chroma_groups(bd):
    """batched chroma prediction blocks (w, h, rnd, blocks): 8x8 runs all 32x32 phases on the separable planes, the other sizes a list that holds every phase once in each
    direction"""
    sz = lambda p: sig8(CHROMA4, p) if p else SIG_ZERO
    for (w, h) in ((2, 2), (4, 2), (2, 8), (8, 8), (64, 4)):
        for rnd in (1, 0):
            blocks = []
            for xf, yf in (ALL32 if (w, h) == (8, 8) else SOME32):
                for comp in (False, True):
                    blocks.append((("sep", sz(xf), sz(yf), comp), ORIGIN[0], ORIGIN[1], xf, yf))
                if (w, h) != (8, 8):
                    blocks.append((("sep", sz(xf), sz(yf), False), OFF_ORIGIN[0], OFF_ORIGIN[1], xf, yf))
                    blocks.append((("fill", "random"), ORIGIN[0], ORIGIN[1], xf, yf))
            blocks.append((("fill", "checker"), OFF_ORIGIN[0], OFF_ORIGIN[1], 16, 16))
            yield w, h, rnd, blocks


DIST_FUNCS = ("SAD", "SSE", "HAD", "HAD_fast")


def dist_groups(bd):
    """sub-pel candidate distortion (w, h, mode, alt, items) with items = [(org key, ref key, xf, yf)], both blocks at ORIGIN: clipped predictions against two-level
    originals.  The zero-phase item of a plane against its complement has every difference at the maximum: with 64x64 at 12 bits and 128x64 at 10 bits its SSE is
    beyond 2^32"""
    sizes = [(8, 8), (16, 16), (32, 16)] + ([(64, 64)] if bd == 12 else []) + ([(128, 64)] if bd == 10 else [])
    for (w, h) in sizes:
        for mode, alt in ((0, 0), (0, 1), (1, 0), (2, 1)):
            if (w, h) in ((64, 64), (128, 64)) and mode:
                continue
            items = []
            for xf, yf in ((0, 0), (8, 8), (8, 0), (5, 11), (0, 12), (15, 3)):
                sh, sv = luma_block_sigs(w, h, xf, yf, alt, mode)
                fam = LUMA_FAMILY[mode]
                items.append((("fill", "blocks4"), _family_key(fam, sh, sv, False), xf, yf))
                items.append((("fill", "random"), _family_key(fam, sh, sv, True), xf, yf))
                items.append((("fill", "const_0" if xf else "const_max"), ("fill", "blocks4"), xf, yf))
            if fam == "luma8":
                items.append((("sep", True), ("sep", FULL_SIG, FULL_SIG, False), 0, 0))          # a plane against its complement: |difference| = max everywhere
            items.append((("fill", "checker"), ("fill", "checker"), 0, 8))
            yield w, h, mode, alt, items


HALF = ((-8, 0), (8, 0), (0, -8), (0, 8), (-8, -8), (8, -8), (-8, 8), (8, 8))
QUARTER = ((-4, 0), (4, 0), (0, -4), (0, 4), (-4, -4), (4, -4), (-4, 4), (4, 4), (0, 0))
# 16 offsets with 16 distinct dx spanning -16 .. 16 and dy at both ends
SPREAD16 = ((-16, -16), (-14, 16), (-12, 0), (-9, 5), (-7, -16), (-4, 16), (-2, -3), (-1, 8), (0, -16), (1, 16), (3, 0), (5, -8), (8, 16), (11, -16), (13, 1), (16, 16))
BASE_FRACS = ((0, 0), (13, 14), (15, 0), (0, 15), (14, 13), (8, 8), (15, 15))


def refine_groups(bd):
    """pattern refinement (w, h, mode, alt, func, offsets, bases) with bases = [(org key, ref key, fx, fy)], both at ORIGIN: the wave-barrier form (8x8, 16x8, 16x16), the
    workgroup-barrier form (32x16, 32x32) and the expand path (64x32); half- and quarter-sample neighbourhoods and the 16-offset list; base fractions 0, 8 and
    13 .. 15 — with the offsets a zero phase in one direction, in both, and only after the offset is added"""
    assert len({dx for dx, _ in SPREAD16}) == 16 and {dy for _, dy in SPREAD16} >= {-16, 16}
    for k, (w, h) in enumerate(((8, 8), (16, 8), (16, 16), (32, 16), (32, 32), (64, 32))):
        for j, (mode, alt, offs) in enumerate(((0, 0, HALF), (0, 1, QUARTER), (1, 0, QUARTER), (2, 1, HALF), (0, 0, SPREAD16), (2, 0, SPREAD16), (1, 1, SPREAD16))):
            func = DIST_FUNCS[(k + j) % 4]
            fam = LUMA_FAMILY[mode]
            sigs = family_sigs(fam)
            bases = []
            for i, (fx, fy) in enumerate(BASE_FRACS):
                sh, sv = sigs[1 + i % (len(sigs) - 1)], sigs[1 + (i // 2) % (len(sigs) - 1)]
                bases.append((("fill", FILLERS[i % 5]), ("sep", sh, sv, bool(i & 1)), fx, fy))
            bases.append((("fill", "blocks4"), ("fill", "random"), 13, 15))
            yield w, h, mode, alt, func, offs, bases


def refine_preds(lib, ref_arr, w, h, mode, alt, offs, bases_xy, bd):
    """the prediction blocks xPatternRefinement scores, from `lib` directly: bases_xy = [(ox, oy, rx, ry, fx, fy)]; base-major, then the offsets in order"""
    out = []
    for (_, _, rx, ry, fx, fy) in bases_xy:
        for dx, dy in offs:
            tx, ty = fx + dx, fy + dy
            out.append(np.ascontiguousarray(lib.if_pred_luma_me((ref_arr, ry + (ty >> 4), rx + (tx >> 4)), w, h, tx & 15, ty & 15, bd, bool(alt), mode)))
    return out


def refine_costs(lib, org, preds, w, h, func, n_offs, bases_xy, bd):
    return [lib.dist(func, (org, bases_xy[k // n_offs][1], bases_xy[k // n_offs][0]), p, w, h, bd, 0) for k, p in enumerate(preds)]


def refine_expected(lib, org, ref_arr, w, h, mode, alt, func, offs, bases_xy, bd):
    """the costs xPatternRefinement would see"""
    return refine_costs(lib, org, refine_preds(lib, ref_arr, w, h, mode, alt, offs, bases_xy, bd), w, h, func, len(offs), bases_xy, bd)


def luma_expected(lib, arr, y, x, w, h, xf, yf, rnd, bd, alt, mode):
    if mode == 0:
        return lib.if_pred_luma((arr, y, x), w, h, xf, yf, bool(rnd), bd, bool(alt))
    assert rnd
    return lib.if_pred_luma_me((arr, y, x), w, h, xf, yf, bd, bool(alt), mode)


PRED_LUMA_SIZES = ((4, 4), (8, 8), (16, 4), (32, 32), (128, 16))
PRED_CHROMA_SIZES = ((2, 2), (4, 4), (8, 2), (32, 8))


def pred_list_items(bd):
    """the plain prediction list: [(w, h, chroma, (key0, key1 or None), ((xf0, yf0), (xf1, yf1)), alt)], every block at ORIGIN of its plane.  Every size class uni- and
    bi-predicted; a bi item pairs a matched plane with itself (both averages' inputs at the top: the upper clip), with its complement, and with a constant"""
    out = []
    for chroma, sizes in ((0, PRED_LUMA_SIZES), (1, PRED_CHROMA_SIZES)):
        fr = ((8, 8), (5, 11), (0, 13), (12, 0), (0, 0)) if not chroma else ((16, 16), (11, 21), (0, 27), (24, 0), (0, 0))
        for (w, h) in sizes:
            for i, (xf, yf) in enumerate(fr):
                alt = int(not chroma and i == 0)
                if chroma:
                    sh, sv = (sig8(CHROMA4, xf) if xf else SIG_ZERO), (sig8(CHROMA4, yf) if yf else SIG_ZERO)
                else:
                    sh, sv = luma_block_sigs(w, h, xf, yf, alt, 0)
                m, c = ("sep", sh, sv, False), ("sep", sh, sv, True)
                out.append((w, h, chroma, (m, None), ((xf, yf), (0, 0)), alt))
                out.append((w, h, chroma, (None, c), ((0, 0), (xf, yf)), alt))
                out.append((w, h, chroma, (m, m), ((xf, yf), (xf, yf)), alt))
                out.append((w, h, chroma, (c, c), ((xf, yf), (xf, yf)), alt))
                out.append((w, h, chroma, (m, c), ((xf, yf), (xf, yf)), alt))
                out.append((w, h, chroma, (m, ("fill", "const_max" if i & 1 else "const_0")), ((xf, yf), (yf, xf)), alt))
            out.append((w, h, chroma, (("fill", "random"), ("fill", "checker")), (fr[1], fr[0]), 0))
    return out


def pred_family(w, h, chroma):
    return "chroma4" if chroma else ("luma6" if (w, h) == (4, 4) else "luma8")


# the layout of vvhip_pred_item (vvenc_amd.hotpath.PRED_ITEM_DTYPE; restated so that the CPU tier imports nothing of the device package)
PRED_ITEM = np.dtype([("dst_off", "<i4"), ("org_off", "<i4"), ("ref_off", "<i4", (2,)), ("frac", "<i2", (2, 2)), ("width", "<i2"), ("height", "<i2"), ("ref_plane", "i1", (2,)),
                      ("chroma", "u1"), ("alt_hpel", "u1")])


def pred_planes(bd):
    fams = ("luma8", "luma6", "chroma4")
    return fams, [atlas(bd, f) for f in fams]


def pred_list_records(bd, strides):
    """vvhip_pred_item records (compact output: dst_off in list order) and positions of pred_list_items; strides[k] = row pitch of plane k"""
    fams, ats = pred_planes(bd)
    spec = pred_list_items(bd)
    it, pos, at_off = np.zeros(len(spec), PRED_ITEM), [], 0
    for k, (w, h, chroma, keys, fr, alt) in enumerate(spec):
        p = fams.index(pred_family(w, h, chroma))
        it[k]["width"], it[k]["height"], it[k]["chroma"], it[k]["alt_hpel"], it[k]["dst_off"] = w, h, chroma, alt, at_off
        where = []
        for l in (0, 1):
            if keys[l] is None:
                it[k]["ref_plane"][l] = -1
                where.append(None)
                continue
            x, y = ORIGIN[0], ats[p].row(keys[l]) + ORIGIN[1]
            it[k]["ref_plane"][l], it[k]["ref_off"][l], it[k]["frac"][l] = p, y * strides[p] + x, fr[l]
            where.append((x, y))
        pos.append(where)
        at_off += w * h
    return it, pos, at_off
