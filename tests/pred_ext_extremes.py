"""Deterministic extreme inputs of the picture-level prediction entries behind the interpolation — vvhip_pred_inter_batch_ex (BDOF, DMVR's padded reference), _blend (BCW,
GEO), _ciip and vvhip_pred_affine_batch (PROF) — at 8, 10 and 12 bits, shared by the CPU tier (tests/test_oracle_pred_ext_extremes.py: the numpy models against the
reference's own functions on tests/golden/*_limits.npz, guards, mutations) and the GPU tier (tests/test_gpu_pred_ext_extremes.py: the device against the models).

BDOF runs fused behind the interpolation, so its frames can only come from planes.  The planes here are the two-level planes of tests/interp_extremes.py: on the
separable FULL_SIG plane and its complement the 14-bit block of a list reaches the largest and smallest value the two passes can produce (+25 079 / -25 085 at 12 bits),
far outside the range ( sample << headroom ) - 8192 of the ring around it, so gradients, the difference of the lists and the correction term b are an order of magnitude
beyond what pictures give, both ends of the final clip act, and every (int16_t) store of the BDOF body carries a value that a narrower store would wrap.

The int64 model below restates the BDOF steps with switchable truncations and shift semantics (MUTATIONS).  It computes the guards of the CPU tier and the mutations of
its sensitivity test; expected values of the tests come from tests/bdof_ref.py, blend_ref.py, ciip_ref.py and affine_ref.py around the interpolation of the oracle or the
compiled reference, never from it.  Numpy only: no GPU, no oracle, no reference.
"""
import os
from functools import lru_cache

import numpy as np

import affine_cases as AC
import bdof_cases as BC
import bdof_ref as BR
import blend_cases as BLC
import blend_ref as BL
import ciip_cases as CC
import ciip_ref as CR
import interp_extremes as X

BITDEPTHS = X.BITDEPTHS
PH, PW, MARGIN = X.PLANE_H + 1, X.PLANE_W, 4          # bdof_cases.limits: a margin of 4 luma samples round every block and one spare last row
SEP, CMP, CHK, RAMP0, RAMP1, COLP, ROWP = range(7)     # plane numbers of planes( bd )
ORIGINS = (X.ORIGIN, X.OFF_ORIGIN, (12, 11), (11, 13))   # on the 3-mod-8 residue, off it in both directions, off it in x only, in y only
PHASES = (((8, 8), (8, 8)), ((8, 8), (5, 11)), ((8, 0), (0, 8)), ((7, 9), (9, 7)), ((8, 8), (0, 0)), ((4, 12), (12, 4)))
UNIT_SHAPES = ((16, 16), (16, 8), (8, 16))


def _ro(a):
    """planes are cached and shared between the tests: nobody writes to them"""
    return np.ascontiguousarray(a, np.int16)


@lru_cache(maxsize=None)
def planes(bd):
    """SEP the separable FULL_SIG plane, CMP its complement, CHK the checkerboard filler; RAMP0 / RAMP1 a smooth low-noise picture and the same picture displaced by a
    flow that grows from -2 to +2 samples across the plane (the interior of the tmpx / tmpy range); COLP / ROWP two-level planes in column / row runs of two for
    DMVR's padded reference (see dmvr_list).  All ( PLANE_H + 1 ) x PLANE_W: one spare row"""
    mx = (1 << bd) - 1
    yy, xx = np.mgrid[0:PH, 0:PW].astype(np.float64)
    rng = np.random.default_rng(7700 + bd)

    def pic(dx, dy):
        return mx / 2 + mx / 3 * np.sin((xx + dx) / 9.0) * np.cos((yy + dy) / 11.0)
    flow_x, flow_y = 2.0 * (xx - PW / 2) / (PW / 2), 2.0 * (yy - PH / 2) / (PH / 2)
    noise = lambda: rng.integers(-1, 2, (PH, PW)) * (mx / 1023.0)
    ramp0 = np.clip(np.round(pic(0, 0) + noise()), 0, mx)
    ramp1 = np.clip(np.round(pic(flow_x, flow_y) + noise()), 0, mx)
    ix, iy = np.mgrid[0:PH, 0:PW][1], np.mgrid[0:PH, 0:PW][0]
    return [_ro(X.separable(X.FULL_SIG, X.FULL_SIG, mx, False, PH, PW)), _ro(X.separable(X.FULL_SIG, X.FULL_SIG, mx, True, PH, PW)), _ro(X.filler("checker", mx, 0, PH, PW)),
            _ro(ramp0), _ro(ramp1), _ro(((ix >> 1) & 1) * mx), _ro(((iy >> 1) & 1) * mx)]


# ---- lists of the extension entry -----------------------------------------------------------------------------------------------
def _add(b, w, h, fr, rp, xy, alt=0, flags=BR.EXT_BDOF, chroma=0, delta=None):
    b.add(w, h, chroma, alt, fr, rp, flags, delta, xy=[tuple(xy[0]), tuple(xy[1])])


def bdof_list(bd):
    """BDOF units on the two-level planes: the three unit shapes, one 32x16 and one 64x64 item (the cut into units); matched (a plane against itself), complement and
    against the checkerboard, both plane orders; the phase pairs of PHASES and alt_hpel at phase 8; origins on and off the 3-mod-8 residue.  -> items, ext, pos"""
    b = BC.ListBuilder(planes(bd), 0)
    pairs = ((SEP, SEP), (SEP, CMP), (CMP, SEP), (SEP, CHK), (CHK, SEP))
    for (w, h) in UNIT_SHAPES:
        for rp in (pairs if (w, h) == (16, 16) else pairs[:2] + pairs[3:4]):
            for fr in PHASES:
                _add(b, w, h, fr, rp, (X.ORIGIN, X.ORIGIN))
            _add(b, w, h, PHASES[0], rp, (X.ORIGIN, X.ORIGIN), alt=1)
        for k, o in enumerate(ORIGINS[1:]):
            for fr in (PHASES if (w, h) == (16, 16) else PHASES[k::3]):
                _add(b, w, h, fr, (SEP, CMP), (o, X.ORIGIN if k == 2 else o))          # the last origin: the two lists on different residues
    for fr in PHASES:
        _add(b, 32, 16, fr, (CMP, SEP), (X.ORIGIN, X.ORIGIN))
    _add(b, 32, 16, PHASES[0], (SEP, CHK), (X.OFF_ORIGIN, X.ORIGIN), alt=1)
    _add(b, 64, 64, PHASES[0], (SEP, CMP), (X.ORIGIN, X.ORIGIN))
    _add(b, 64, 64, PHASES[1], (CHK, SEP), (X.OFF_ORIGIN, X.ORIGIN))
    return b.done()


# found by a search over a denser grid: units in which a negative odd sSign * tmpx is halved and a truncation toward zero would give another tmpy (at 8 bits the grid
# of ramp_list has none; the CPU tier asserts that every bit depth has one)
RAMP_EXTRA = ((70, 20, ((1, 8), (15, 12)), (RAMP1, RAMP0)), (45, 25, ((0, 1), (2, 3)), (RAMP0, RAMP1)), (90, 25, ((11, 14), (1, 6)), (RAMP1, RAMP0)),
              (35, 35, ((6, 11), (0, 9)), (RAMP0, RAMP1)), (55, 35, ((2, 15), (12, 5)), (RAMP0, RAMP1)), (25, 40, ((14, 3), (8, 1)), (RAMP0, RAMP1)))


def ramp_list(bd):
    """16x16, 16x8 and 8x16 units on the low-noise pictures, spread over the flow field: the interior of the tmpx / tmpy range"""
    b = BC.ListBuilder(planes(bd), 0)
    k = 0
    for y in range(6, PH - 1 - 16 - MARGIN, 12):
        for x in range(6, PW - 16 - MARGIN, 14):
            w, h = UNIT_SHAPES[k % 7 % 3] if k % 7 >= 4 else (16, 16)
            fr = (((3 * k) % 16, (5 * k + 1) % 16), ((7 * k + 2) % 16, (11 * k + 3) % 16))
            _add(b, w, h, fr, (RAMP0, RAMP1) if k % 2 == 0 else (RAMP1, RAMP0), ((x, y), (x, y)))
            k += 1
    for (x, y, fr, rp) in RAMP_EXTRA:
        _add(b, 16, 16, fr, rp, ((x, y), (x, y)))
    return b.done()


def _pad_xy(x, y, w, h, d, reach):
    """a START position near ( x, y ) for a list that moves by d = ( dx, dy ) on COLP / ROWP (runs of two): the last column ( row ) of the prefetched window
    start - reach .. start + size + reach on the side the list moves to is the LAST sample of its run, so that the one or two samples beyond it, which the clamp replaces
    by it, carry the opposite level"""
    dx, dy = d
    if dx > 0:
        x += (x + w + reach + 1) & 1          # window's last column odd: the run ends there
    elif dx < 0:
        x += (x - reach) & 1                  # window's first column even: the run starts there
    if dy > 0:
        y += (y + h + reach + 1) & 1
    elif dy < 0:
        y += (y - reach) & 1
    return x, y


def dmvr_list(bd):
    """DMVR's padded reference on COLP ( deltas in x ) and ROWP ( deltas in y ): luma deltas +-2 and +-1 with and without BDOF on 16x16, 16x8 and 8x16 and without it on
    8x8; 4:2:0 chroma deltas +-1 on 8x8, 4x8, 8x4 and 4x4; list 1 mirrors list 0.  Fractions are non-zero in the direction of the delta: the taps read past the window"""
    b = BC.ListBuilder(planes(bd), 0)
    for (w, h) in ((16, 16), (16, 8), (8, 16), (8, 8)):
        for bdof in ((1, 0) if BR.bdof_applies(w, h) else (0,)):
            for k, d in enumerate(((2, 0), (-2, 0), (0, 2), (0, -2), (1, 0), (0, -1))):
                for fr in (((8, 8), (8, 8)), ((5, 11), (11, 5)), ((13, 3), (2, 14))):
                    p = COLP if d[0] else ROWP
                    xy = [_pad_xy(20 + 3 * k, 18 + k, w, h, dd, 3) for dd in (d, (-d[0], -d[1]))]
                    _add(b, w, h, fr, (p, p), xy, flags=BR.EXT_DMVR_PAD | (BR.EXT_BDOF if bdof else 0), delta=(d, (-d[0], -d[1])))
    for (w, h) in ((8, 8), (4, 8), (8, 4), (4, 4)):
        for k, d in enumerate(((1, 0), (-1, 0), (0, 1), (0, -1))):
            for fr in (((16, 16), (16, 16)), ((11, 21), (21, 11))):
                p = COLP if d[0] else ROWP
                xy = [_pad_xy(30 + 5 * k, 40 + k, w, h, dd, 1) for dd in (d, (-d[0], -d[1]))]
                _add(b, w, h, fr, (p, p), xy, flags=BR.EXT_DMVR_PAD, chroma=1, delta=(d, (-d[0], -d[1])))
    return b.done()


def check_margins(pl, items, ext, pos):
    BLC.check_margins(pl, items, ext, pos)


# ---- the int64 model of BDOF ----------------------------------------------------------------------------------------------------
MUTATIONS = ("trunc_x", "trunc_y", "no_half", "wrap12", "no_cast", "cast_after_clip", "sn_hr1", "ring_pos", "ring_unclamped", "clip14", "clip16")


def _wrap(v, bits):
    return ((v + (1 << (bits - 1))) & ((1 << bits) - 1)) - (1 << (bits - 1))


def _shr(v, k, trunc):
    """arithmetic shift right (floor); trunc: the division toward zero a sign-magnitude form would give"""
    return np.sign(v) * (np.abs(v) >> k) if trunc else v >> k


def bdof_model(f0, f1, bd, mut=()):
    """xApplyBDOF on the two ( h + 2 ) x ( w + 2 ) frames -> dict: out, raw (the value in front of the int16 cast and the clip), gx, gy (both lists stacked), di, b, tmpx,
    tmpy, the five sums"""
    f0, f1 = f0.astype(np.int64), f1.astype(np.int64)
    g = lambda f: ((f[1:-1, 2:] >> 6) - (f[1:-1, :-2] >> 6), (f[2:, 1:-1] >> 6) - (f[:-2, 1:-1] >> 6))
    (gx0, gy0), (gx1, gy1) = g(f0), g(f1)
    s0, s1 = f0[1:-1, 1:-1], f1[1:-1, 1:-1]
    tgx, tgy, tdi = (gx0 + gx1) >> 1, (gy0 + gy1) >> 1, (s1 >> 4) - (s0 >> 4)
    store = (lambda v: _wrap(v, 12)) if "wrap12" in mut else (lambda v: _wrap(v, 16))
    tgx, tgy, tdi = store(tgx), store(tgy), store(tdi)
    pad = lambda a: np.pad(a, 1, mode="edge")
    G, V, D = pad(tgx), pad(tgy), pad(tdi)
    win = np.lib.stride_tricks.sliding_window_view
    sums = [win(t, (6, 6))[::4, ::4].sum(axis=(2, 3)) for t in (np.abs(G), np.abs(V), np.sign(G) * D, np.sign(V) * D, np.sign(V) * G)]
    s_agx, s_agy, s_dix, s_diy, s_sign = sums
    lim = 14 if "clip14" in mut else 16 if "clip16" in mut else 15
    lx, ly = BR._floor_log2(s_agx), BR._floor_log2(s_agy)
    tmpx = np.where(s_agx == 0, 0, np.clip(_shr(4 * s_dix, lx, "trunc_x" in mut), -lim, lim))
    cross = s_sign * tmpx
    half = cross if "no_half" in mut else cross >> 1
    tmpy = np.where(s_agy == 0, 0, np.clip(_shr(4 * s_diy - half, ly, "trunc_y" in mut), -lim, lim))
    hr = X.headroom(bd)
    sn = hr + 1 if "sn_hr1" in mut else 15 - bd
    off = (1 << (sn - 1)) + 2 * 8192
    tx, ty = np.kron(tmpx, np.ones((4, 4), np.int64)), np.kron(tmpy, np.ones((4, 4), np.int64))
    bb = tx * (gx0 - gx1) + ty * (gy0 - gy1)
    raw = (s0 + s1 + bb + off) >> sn
    v = raw if ("no_cast" in mut or "cast_after_clip" in mut) else _wrap(raw, 16)
    out = np.clip(v, 0, (1 << bd) - 1)
    if "cast_after_clip" in mut:
        out = _wrap(out, 16)
    return dict(out=out.astype(np.int16), raw=raw, gx=np.stack([gx0, gx1]), gy=np.stack([gy0, gy1]), di=(s1 >> 4) - (s0 >> 4), b=bb, tmpx=tmpx, tmpy=tmpy, sums=sums,
                neg_inexact_x=bool(np.any((s_agx != 0) & (4 * s_dix < 0) & ((4 * s_dix) & ((1 << lx) - 1) != 0))), neg_odd_cross=bool(np.any((s_agy != 0) & (cross < 0) & (cross & 1 == 1))),
                trunc_changes_x=bool(np.any((s_agx != 0) & (np.clip(_shr(4 * s_dix, lx, True), -15, 15) != np.clip(4 * s_dix >> lx, -15, 15)))),
                trunc_changes_half=bool(np.any((s_agy != 0) & (np.clip((4 * s_diy - _shr(cross, 1, True)) >> ly, -15, 15) != np.clip((4 * s_diy - (cross >> 1)) >> ly, -15, 15)))))


def unit_frames(pl, pos, it, e, bd, mut=(), clamp=True):
    """the frames of every BDOF unit of an item, from the int64 interpolation model of tests/interp_extremes.py: [( x0, y0, uw, uh, f0, f1 )]"""
    w, h, alt, flags = int(it["width"]), int(it["height"]), int(it["alt_hpel"]), int(e["flags"])
    hr = X.headroom(bd)
    out = []
    for (x0, y0, uw, uh) in BR.bdof_units(w, h):
        fr = []
        for l in (0, 1):
            arr = pl[int(it["ref_plane"][l])]
            delta = (int(e["pad_dx"][l]), int(e["pad_dy"][l])) if flags & BR.EXT_DMVR_PAD and clamp else None
            src, y, x = BR.source(arr, pos[l][1], pos[l][0], w, h, 0, delta)
            xf, yf = int(it["frac"][l][0]), int(it["frac"][l][1])
            inner = X.pred_luma(src, y + y0, x + x0, uw, uh, xf, yf, False, bd, bool(alt))
            xo, yo = (1, 1) if "ring_pos" in mut else ((1 if xf < 8 else 0), (1 if yf < 8 else 0))
            rs, ry, rx = (arr, pos[l][1], pos[l][0]) if "ring_unclamped" in mut else (src, y, x)
            near = rs[ry + y0 - yo:ry + y0 - yo + uh + 2, rx + x0 - xo:rx + x0 - xo + uw + 2].astype(np.int64)
            f = X.wrap16((near << hr) - 8192)
            f[1:-1, 1:-1] = inner
            fr.append(f)
        out.append((x0, y0, uw, uh, fr[0], fr[1]))
    return out


def model_block(pl, pos, it, e, bd, mut=(), clamp=True, detail=None):
    """an item with the BDOF flag through the int64 model; detail: a list that receives ( unit, model dict, f0, f1 )"""
    res = np.zeros((int(it["height"]), int(it["width"])), np.int16)
    for (x0, y0, uw, uh, f0, f1) in unit_frames(pl, pos, it, e, bd, mut, clamp):
        m = bdof_model(f0, f1, bd, mut)
        res[y0:y0 + uh, x0:x0 + uw] = m["out"]
        if detail is not None:
            detail.append(((x0, y0, uw, uh), m, f0, f1))
    return res


def model_plain(pl, pos, it, e, bd, clamp=True, tr=None):
    """an item without BDOF (uni or the default average, luma or chroma, through the padded window when its record says so) from the int64 interpolation model"""
    w, h, chroma, alt, flags = int(it["width"]), int(it["height"]), int(it["chroma"]), int(it["alt_hpel"]), int(e["flags"])
    used = [l for l in (0, 1) if int(it["ref_plane"][l]) >= 0]
    out = []
    for l in used:
        delta = (int(e["pad_dx"][l]), int(e["pad_dy"][l])) if flags & BR.EXT_DMVR_PAD and clamp else None
        src, y, x = BR.source(pl[int(it["ref_plane"][l])], pos[l][1], pos[l][0], w, h, chroma, delta)
        xf, yf = int(it["frac"][l][0]), int(it["frac"][l][1])
        out.append(X.pred_chroma(src, y, x, w, h, xf, yf, len(used) == 1, bd) if chroma else X.pred_luma(src, y, x, w, h, xf, yf, len(used) == 1, bd, bool(alt)))
    return out[0] if len(out) == 1 else X.add_avg(out[0], out[1], bd, tr)


def model_item(pl, pos, it, e, bd, mut=(), clamp=True):
    return model_block(pl, pos, it, e, bd, mut, clamp) if int(e["flags"]) & BR.EXT_BDOF else model_plain(pl, pos, it, e, bd, clamp).astype(np.int16)


def clamp_swing(pl, pos, it, e):
    """largest |difference| between a sample the taps of a DMVR item fetch through the clamp window and the sample the unclamped read would fetch, over both lists"""
    w, h, chroma = int(it["width"]), int(it["height"]), int(it["chroma"])
    taps, pad = (4, 1) if chroma else (8, 2)
    r, worst = taps // 2 - 1, 0
    for l in (0, 1):
        arr = pl[int(it["ref_plane"][l])]
        dx, dy = int(e["pad_dx"][l]), int(e["pad_dy"][l])
        x, y = pos[l]
        cl = BR.clamped_plane(arr, y - dy, x - dx, w, h, taps)
        a, c = arr[y - r:y + h + taps // 2, x - r:x + w + taps // 2].astype(np.int64), cl[y - r:y + h + taps // 2, x - r:x + w + taps // 2].astype(np.int64)
        worst = max(worst, int(np.abs(a - c).max()))
    return worst


# ---- BCW, GEO, CIIP -------------------------------------------------------------------------------------------------------------
def blend_list(bd):
    """blend_cases.extremes_list on the planes of blend_cases at this bit depth -> planes, items, ext, blend, pos"""
    pl, _ = BLC.planes(bd, 100 + bd)
    return (pl,) + BLC.extremes_list(pl, 500 + bd)


CIIP_SIZES = ((8, 8, 0), (4, 16, 0), (64, 64, 0), (4, 4, 1), (8, 2, 1), (32, 32, 1))          # the smallest luma sizes (w * h >= 64), the largest, the smallest and largest chroma sizes


def ciip_lines(w, h, bd):
    """reference lines all 0, all max, and alternating 0 / max starting with either (top[0] == left[0])"""
    top = (1 << bd) - 1
    n = CR.line_len(w, h)
    alt = np.concatenate([(np.arange(w + 3) & 1) * top, (np.arange(h + 3) & 1) * top]).astype(np.int16)
    return [np.zeros(n, np.int16), np.full(n, top, np.int16), alt, (top - alt).astype(np.int16)]


def ciip_list(bd):
    """CIIP items whose inter part comes from the 0 / max checkerboards of blend_cases at fractional phases (uni, bi, BCW 0 and BCW 4) and whose reference lines are
    all 0, all max and alternating; num_intra cycles 0..2 against the kinds -> planes, items, ext, blend, ciip, lines, pos"""
    pl, _ = BLC.planes(bd, 100 + bd)
    b = CC.Builder(pl, 700 + bd)
    k = 0
    for (w, h, c) in CIIP_SIZES:
        half = 16 if c else 8
        frs = (((half, half), (half, half)), ((half, 3), (5, half)), ((half - 3, half + 3), (half + 3, half - 3)), ((half, half), (1, half)))
        for j, line in enumerate(ciip_lines(w, h, bd)):
            for kind in range(4):
                rp = ((4, -1) if (j + k) % 2 == 0 else (-1, 5)) if kind == 0 else ((4, 5), (5, 4), (4, 5))[kind - 1]
                rp = tuple(r + 2 * c if r >= 0 else -1 for r in rp)
                mode, param = ((BL.BLEND_DEFAULT, 0), (BL.BLEND_DEFAULT, 0), (BL.BLEND_BCW, 0), (BL.BLEND_BCW, 4))[kind]
                b.add(w, h, c, 0, frs[(j + kind) % 4], rp, mode, param, num_intra=k % 3, line=line)
                k += 1
    return (pl,) + b.done()


def blend_mut(s0, s1, mode, param, bd, chroma=0, shift_less=0):
    """blend_ref.blend with BCW's / GEO's shift as headroom + 3 - shift_less (the mutation of the sensitivity test)"""
    w0 = BL.weights_of(s0.shape, mode, param, chroma).astype(np.int64)
    shift = X.headroom(bd) + 3 - shift_less
    v = (w0 * s0.astype(np.int64) + (8 - w0) * s1.astype(np.int64) + (1 << (shift - 1)) + (8192 << 3)) >> shift
    return v, np.clip(v, 0, (1 << bd) - 1).astype(np.int16)


def hypotheses14(pl, pos, it, bd):
    """the 14-bit blocks of both hypotheses of a bi-predicted item from the int64 interpolation model"""
    out = []
    for l in (0, 1):
        arr, (x, y) = pl[int(it["ref_plane"][l])], pos[l]
        xf, yf, w, h = int(it["frac"][l][0]), int(it["frac"][l][1]), int(it["width"]), int(it["height"])
        out.append(X.pred_chroma(arr, y, x, w, h, xf, yf, False, bd) if int(it["chroma"]) else X.pred_luma(arr, y, x, w, h, xf, yf, False, bd, bool(it["alt_hpel"])))
    return out


def ciip_inter(pl, pos, it, bl, bd, tr=None):
    """the inter part of a CIIP item from the int64 models -> clipped block; tr["raw"]: the value in front of the final clip"""
    tr = {} if tr is None else tr
    if int(it["ref_plane"][0]) < 0 or int(it["ref_plane"][1]) < 0:
        e = np.zeros((), BC.PRED_EXT_DTYPE)
        l = 0 if int(it["ref_plane"][0]) >= 0 else 1
        arr, (x, y) = pl[int(it["ref_plane"][l])], pos[l]
        xf, yf, w, h = int(it["frac"][l][0]), int(it["frac"][l][1]), int(it["width"]), int(it["height"])
        t = {}
        out = X.pred_chroma(arr, y, x, w, h, xf, yf, True, bd, tr=t) if int(it["chroma"]) else X.pred_luma(arr, y, x, w, h, xf, yf, True, bd, False, tr=t)
        tr["raw"] = t.get("raw2")
        return out.astype(np.int16)
    s0, s1 = hypotheses14(pl, pos, it, bd)
    if int(bl["mode"]) == BL.BLEND_BCW:
        tr["raw"], out = blend_mut(s0, s1, BL.BLEND_BCW, int(bl["param"]), bd, int(it["chroma"]))
        return out
    t = {}
    out = X.add_avg(s0, s1, bd, t)
    tr["raw"] = t["avg"]
    return out.astype(np.int16)


def ciip_weight_mut(inter, intra, num_intra, plus_one=True):
    wi = int(num_intra) + (1 if plus_one else 0)
    return ((wi * intra.astype(np.int64) + (4 - wi) * inter.astype(np.int64) + 2) >> 2).astype(np.int16)


# ---- affine with PROF -----------------------------------------------------------------------------------------------------------
AFFINE_WORLDS = tuple((ctu, kind) for ctu in (32, 128) for kind in ("texture", "checker", "zero", "max"))


@lru_cache(maxsize=None)
def affine_world(bd, ctu, kind):
    return AC.World(bd, ctu, kind, seed=9)


def affine_lists(bd, ctu, kind):
    """the existing extreme_list and edge_list on World( bd, ctu, kind ) -> world, [( name, items, pos )]"""
    world = affine_world(bd, ctu, kind)
    out = []
    for name, (items, pos) in (("extreme", AC.extreme_list(world, 9)), ("edge", AC.edge_list(world, ctu))):
        items = items.copy()
        items["dst_off"] = AC.compact_offsets(items)[0]
        out.append((name, items, pos))
    return world, out


def prof_limit(bd, mutated=False):
    """the clip of PROF's dI: 1 << max( bitDepth + 1, 13 ) — 1 << 13 at every bit depth of 8..12, so a kernel that hard-codes 13 cannot be told apart there"""
    return 1 << (13 if mutated else max(bd + 1, 13))


AFFINE_LIMITS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "affine_limits.npz")


def affine_limits_cases():
    """tests/golden/affine_limits.npz as affine_cases.golden_cases returns affine.npz, but with planes of one bit depth, `plane_bd` (12), taken as they are
    -> (hdr, {plane_bd: [y0, y1, c0, c1]}, list of (bd, luma item, chroma item, pos per component, {row: {(l, chroma): block}}))"""
    g = np.load(AFFINE_LIMITS)
    pic_w, pic_h, ctu, margin = (int(v) for v in g["hdr"])
    bdp = int(g["plane_bd"])
    spare = lambda a: np.concatenate([a, a[-1:]]).astype(np.int16)          # one spare row: the aligned-dword rule of the device planes
    pl = [spare(g["y0"]), spare(g["y1"]), spare(g["c0"]), spare(g["c1"])]
    out, at = [], 0
    for c in g["cases"]:
        bd, x, y, w, h, six, inter_dir, prof = (int(v) for v in c[:8])
        lu = np.zeros((), AC.ITEM_DTYPE)
        lu["cu_x"], lu["cu_y"], lu["cu_w"], lu["cu_h"], lu["six_param"], lu["prof"] = x, y, w, h, six, prof
        lu["cpmv"] = c[10:22].reshape(2, 3, 2)
        lu["ref_plane"] = [int(c[8 + l]) if inter_dir & (1 << l) else -1 for l in (0, 1)]
        ch = lu.copy()
        ch["chroma"] = 1
        ch["ref_plane"] = [p + 2 if p >= 0 else -1 for p in lu["ref_plane"]]
        pos = {0: [(margin + x, margin + y)] * 2, 1: [(margin // 2 + x // 2, margin // 2 + y // 2)] * 2}
        for it, cc in ((lu, 0), (ch, 1)):
            for l in (0, 1):
                if it["ref_plane"][l] >= 0:
                    it["ref_off"][l] = pos[cc][l][1] * pl[int(it["ref_plane"][l])].shape[1] + pos[cc][l][0]
        rec = {"scalar": {}, "simd": {}}
        for row in ("scalar", "simd"):
            a = at
            for l in (0, 1):
                if inter_dir & (1 << l):
                    rec[row][(l, 0)] = g[row][a:a + w * h].reshape(h, w); a += w * h
                    rec[row][(l, 1)] = g[row][a:a + w * h // 4].reshape(h // 2, w // 2); a += w * h // 4
        at += (w * h + w * h // 4) * (2 if inter_dir == 3 else 1)
        out.append((bd, lu, ch, pos, rec))
    assert at == g["scalar"].size == g["simd"].size
    return (pic_w, pic_h, ctu, margin), {bdp: pl}, out
