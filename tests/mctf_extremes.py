"""Deterministic extreme inputs of the MCTF device code — the search (vvhip_mctf_motion_estimation and the per-level route), the four small entries
(vvhip_mctf_error_batch, vvhip_mctf_calc_var_batch, vvhip_mctf_subsample, vvhip_extend_border) and the apply side (vvhip_mctf_apply_plane) — shared by the CPU tier
(tests/test_oracle_mctf_extremes.py: oracle against the compiled reference, the models, the guards, the sensitivity test) and the GPU tier
(tests/test_gpu_mctf_extremes.py: every entry against the oracle, tolerance 0).  Bit depths 8 and 10 only (MCTF.cpp:1313 refuses more).

The parity suites run MCTF on mid-range texture centred on 512 at 10 bits.  The families here:
  error       every (w, h) of 8 .. 64 x 8 .. 64, integer displacement and all 255 fractional phases of either tap set, on pairs of two-level pages (checkers and stripes
              of period 1 .. 16 and their complements, an impulse and its inverse, constants, samples within 3 of either end) and a mid-range control; odd sample
              offsets; row pitches 104 and 120.  Per size a saturated pair whose sum is min(w h max^2, 2^31 - 1): beyond 2052 full-range differences at 10 bits a
              reference `int` cannot hold the sum, so the pair is built to land on 2^31 - 1 exactly
  variance    flat, half 0 / half max, checker, near-end and texture blocks at every size of 8 .. 64 x 8 .. 64, at 1x1 and at 128x128 (the entry's limits)
  planes      subsample and extend_border on max-valued, checker, near-end and odd-sized planes, pads 0, 1, 16, 128, inside sentinel-filled storage
  search      pictures of 64x64 .. 208x136 x units 8, 16 x speeds 0, 2, 4 x add_level: (a) flat equal planes, (b) 0 against max, (c) periodic stripes and checkers,
              (d) a texture (a ramp under seeded noise) displaced to the far end of the schedule's reach in the four diagonal directions, (e) the same at 8 bits,
              (f) flat planes with steps of +-1 on half of the samples, where a neighbour's vector ties with a block's own best or beats it by one
  apply       4:2:0 pictures up to 96x64 with hand-built motion fields (all 256 phases, negative vectors, the corner blocks' vectors deepest into the margins), block
              errors 49 / 50 / 100 / 101, QP 0 / 32 / 33 / 63, rmsme 0 and not, 1 .. 12 references

Inputs the reference does not define are kept out by construction; the models return the float64 / int64 value of each such intermediate (the items' exact sums, the
traces of me_level_model, ApplyCase.intermediates) so that the CPU tier can assert it finite and inside `int`:
  MCTF.cpp:134, :194, :248   the `int` accumulators of the three error functions (the saturated pairs stop at 2^31 - 1; a fractional item takes the first page pair of its
                             rotation whose exact sum fits)
  MCTF.cpp:1318              (int)( 20 * ( ( error * bdScale + 5 ) / ( dvar + 5 ) ) + mse / 50 ): a flat block with the largest error of a 16x16 final block is 1.07e9;
                             the final blocks here are at most 16x16
  MCTF.cpp:474               (int) round( ( 15 cntD / cntV * variance + 5 ) / ( diffsum + 5 ) ): a constant offset makes diffsum 0; the apply family uses checkers against
                             complements and offsets of a few levels at unit 32, never a full-range flat offset
  MCTF.cpp:396, :399         xSum * ySum of the plane fit is an `int` product: 15872 * ySum at 32x32, beyond `int` from a mean difference of 133 (found while
                             building this tier); the cases of unit 32 have QP 33 and 63, where the plane fit is off
  MCTF.cpp:359-367, :508     fastExp( -diffSq, 2 sigmaSq sw ): 1 - diffSq / ( 1024 d ) must stay positive, or the 1024th power, the weight sum and the (Pel) cast of :513
                             leave the defined range; `fast_exp_base` is its smallest value per case
  MCTF.cpp:1313              bit depths above 10
  MCTF.h:77                  MotionVector() leaves `overlap` uninitialised: in the blocks of the last level that no task writes (a remainder of 4) the reference returns
                             what the allocation held; the oracle and the device define 0 there, and the CPU tier compares the reference's field in the written blocks only

The int64 models below restate motionErrorLumaInt / Frac6 / Frac4 (MCTF.cpp:122-257), calcVarCore (:520-546), subsampleLuma (:1072-1097), estimateLumaLn and the hierarchy
around it (:666-707, :1099-1327), applyFrac8Core (:259-357) and applyPlanarCorrectionCore (:372-417).  They serve the guards and the mutations of the sensitivity test only:
expected values of both tiers come from the oracle, never from them.  Numpy only: no GPU, no oracle, no reference.
"""
from functools import lru_cache

import numpy as np

BITDEPTHS = (8, 10)
INT_MAX = 2 ** 31 - 1
PAD = 128                                     # MCTF_PADDING
SENT16 = -21846                               # 0xAAAA: no sample of 8 or 10 bits

# the search and apply filters (MCTF.cpp:72-110; of the 6-tap rows the taps [1 .. 6] are used); the CPU tier asserts them equal to the oracle's tables
F6 = np.array([[0, 0, 0, 64, 0, 0, 0, 0], [0, 1, -3, 64, 4, -2, 0, 0], [0, 1, -6, 62, 9, -3, 1, 0], [0, 2, -8, 60, 14, -5, 1, 0], [0, 2, -9, 57, 19, -7, 2, 0],
               [0, 3, -10, 53, 24, -8, 2, 0], [0, 3, -11, 50, 29, -9, 2, 0], [0, 3, -11, 44, 35, -10, 3, 0], [0, 1, -7, 38, 38, -7, 1, 0], [0, 3, -10, 35, 44, -11, 3, 0],
               [0, 2, -9, 29, 50, -11, 3, 0], [0, 2, -8, 24, 53, -10, 3, 0], [0, 2, -7, 19, 57, -9, 2, 0], [0, 1, -5, 14, 60, -8, 2, 0], [0, 1, -3, 9, 62, -6, 1, 0],
               [0, 0, -2, 4, 64, -3, 1, 0]], np.int64)
F4 = np.array([[0, 64, 0, 0], [-2, 62, 4, 0], [-2, 58, 10, -2], [-4, 56, 14, -2], [-4, 54, 16, -2], [-6, 52, 20, -2], [-6, 46, 28, -4], [-4, 42, 30, -4], [-4, 36, 36, -4],
               [-4, 30, 42, -4], [-4, 28, 46, -6], [-2, 20, 52, -6], [-2, 16, 54, -4], [-2, 14, 56, -4], [-2, 10, 58, -2], [0, 4, 62, -2]], np.int64)

MV_DTYPE = np.dtype([("x", "<i4"), ("y", "<i4"), ("error", "<i4"), ("rmsme", "<i4"), ("overlap", "<f8")])      # vvhip_mv (vvenc_amd.hotpath.MV_DTYPE, restated)
ERR_ITEM = np.dtype([("o", "<i4"), ("b", "<i4"), ("fx", "<i2"), ("fy", "<i2")])                                  # vvhip_mctf_item

MUTATIONS = ("scan_le", "col_major", "clip_second_only", "no_round", "no_bdscale", "no_and7", "planar_lt32", "neighbour_le", "var_no_shift", "sub_no_round")


def _ro(v):
    return np.ascontiguousarray(v, np.int16)


def wrap16(v):
    return ((v + 32768) & 0xffff) - 32768


# ---- sample fillers -------------------------------------------------------------------------------------------------------------------------------------------
def fill(kind, mx, h, w, seed=0):
    """`kind`: zero, max, checkerP / vstripeP / hstripeP (two levels 0 / max with period P; a leading `~` gives the complement), impulse (one max on 0), hole (its
    inverse), near_lo / near_hi (within 3 of either end), texture (seeded, mid-range: the control)"""
    yy, xx = np.mgrid[0:h, 0:w]
    inv = kind.startswith("~")
    k = kind[1:] if inv else kind
    if k == "zero":
        a = np.zeros((h, w), np.int64)
    elif k == "max":
        a = np.full((h, w), mx, np.int64)
    elif k.startswith("checker"):
        p = int(k[7:])
        a = (((xx // p) + (yy // p)) & 1) * mx
    elif k.startswith("vstripe"):
        a = ((xx // int(k[7:])) & 1) * mx
    elif k.startswith("hstripe"):
        a = ((yy // int(k[7:])) & 1) * mx
    elif k == "impulse":
        a = np.zeros((h, w), np.int64)
        a[h // 2 - 3, w // 2 + 1] = mx
    elif k == "hole":
        a = np.full((h, w), mx, np.int64)
        a[h // 2 - 3, w // 2 + 1] = 0
    elif k == "near_lo":
        a = np.random.default_rng(5100 + seed).integers(0, 4, (h, w))
    elif k == "near_hi":
        a = mx - np.random.default_rng(5200 + seed).integers(0, 4, (h, w))
    elif k == "texture":
        rng = np.random.default_rng(5300 + seed)
        t = 0.5 + 0.29 * np.sin(xx / 3.7) * np.cos(yy / 2.9) + 0.09 * np.sin((xx - yy) / 2.3) + rng.normal(0, 0.03, (h, w))
        a = np.clip(t * (mx + 1), 0, mx).astype(np.int64)
    else:
        raise ValueError(kind)
    return _ro(mx - a if inv else a)


# ---- the error functions --------------------------------------------------------------------------------------------------------------------------------------
def _taps(tap4, f):
    return (F4[f], 1) if tap4 else (F6[f][1:7], 2)


def frac_block(a, y, x, w, h, fx, fy, tap4, bd, mut=(), apply=False, clip=True):
    """the w x h block at (x, y) of the int64 array a, displaced by (fx, fy) sixteenths: horizontal pass, vertical pass.  The error functions clip after each pass
    (MCTF.cpp:172, :192); the apply functions keep the first pass as a Pel without clipping (:285) and clip the second (:305)"""
    mx = (1 << bd) - 1
    (xf, off), (yf, _) = _taps(tap4, fx), _taps(tap4, fy)
    nt = len(xf)
    rnd = 0 if "no_round" in mut else 32
    s = a[y - off:y - off + h + nt - 1, x - off:x - off + w + nt - 1]
    t = sum(int(xf[k]) * s[:, k:k + w] for k in range(nt))
    t = (t + rnd) >> 6
    t = wrap16(t) if (apply or "clip_second_only" in mut) else np.clip(t, 0, mx)
    v = sum(int(yf[k]) * t[k:k + h] for k in range(nt))
    return np.clip((v + rnd) >> 6, 0, mx) if clip else (v + rnd) >> 6


def err_model(org, oy, ox, buf, by, bx, w, h, fx, fy, tap4, bd, mut=()):
    """motionErrorLumaInt (fx == fy == 0) / Frac6 / Frac4 as an exact integer (no `int` wrap-around: the caller compares it with INT_MAX)"""
    o = org[oy:oy + h, ox:ox + w]
    p = buf[by:by + h, bx:bx + w] if (fx | fy) == 0 else frac_block(buf, by, bx, w, h, fx, fy, tap4, bd, mut)
    d = p - o
    return int((d * d).sum())


def err_footprint(w, h):
    """rows and columns relative to the buf position that either side may read, inclusive: the reference's 6-tap form computes the rows -2 .. h + 3 (the last one unused)
    of columns -2 .. w + 2; waveErrorFrac<false> loads eight samples from column x - 2 for x up to w - 2, so column w + 3 too"""
    return -2, h + 3, -2, w + 3


PAGE_H, ORG_W, BUF_W = 80, 104, 120           # a 64x64 block with its footprint at a few offsets; row pitches that are multiples of 8 and no powers of two
ORG_KINDS = ("checker1", "checker2", "checker4", "checker8", "checker16", "vstripe1", "hstripe2", "impulse", "hole", "zero", "max", "near_lo", "near_hi", "texture")
BUF_KINDS = ORG_KINDS + ("~checker1", "~checker2", "~checker4", "~checker8", "~checker16", "~vstripe1", "~hstripe2")
# (org page, buf page): complements (every difference the range where the offsets agree), equal pages at other offsets, the impulses, the constants, the ends, the control
PAIRS = (("checker1", "~checker1"), ("checker2", "~checker2"), ("checker4", "~checker4"), ("checker8", "~checker8"), ("checker16", "~checker16"), ("vstripe1", "~vstripe1"),
         ("hstripe2", "~hstripe2"), ("impulse", "hole"), ("hole", "impulse"), ("zero", "max"), ("max", "zero"), ("checker1", "checker1"), ("checker2", "checker4"),
         ("impulse", "impulse"), ("hole", "hole"), ("zero", "checker1"), ("max", "checker2"), ("near_lo", "near_hi"), ("near_hi", "near_lo"), ("near_lo", "checker1"),
         ("zero", "impulse"), ("max", "hole"), ("texture", "texture"), ("texture", "checker8"))
ERR_SIZES = tuple((w, h) for w in range(8, 65, 8) for h in range(8, 65, 8))
LIST_NS = (0, 1, 63, 64, 65, 300)


@lru_cache(maxsize=None)
def err_planes(bd):
    """(org, buf): the pages stacked; four rows of slack in front of and behind them for the host rows' wider loads"""
    mx = (1 << bd) - 1
    slack = lambda w: np.zeros((4, w), np.int16)
    org = np.concatenate([slack(ORG_W)] + [fill(k, mx, PAGE_H, ORG_W, 1) for k in ORG_KINDS] + [slack(ORG_W)])
    buf = np.concatenate([slack(BUF_W)] + [fill(k, mx, PAGE_H, BUF_W, 2) for k in BUF_KINDS] + [slack(BUF_W)])
    return _ro(org), _ro(buf)


def _page_row(kinds, k):
    return 4 + kinds.index(k) * PAGE_H


def _place(pair, n, w, h):
    """the n-th placement of a page pair: (ox, oy, bx, by) in the stacked planes; org and buf columns take every pair of parities, the footprint stays in the page"""
    r_lo, r_hi, c_lo, c_hi = err_footprint(w, h)
    ox = n % (ORG_W - w + 1)
    oy = (n // 3) % (PAGE_H - h + 1)
    bx = -c_lo + (n * 5 + n // 2) % (BUF_W - c_hi + c_lo)
    by = -r_lo + (n * 3) % (PAGE_H - r_hi + r_lo)
    return ox, _page_row(ORG_KINDS, pair[0]) + oy, bx, _page_row(BUF_KINDS, pair[1]) + by


@lru_cache(maxsize=None)
def err_items(bd, w, h, tap4):
    """[(ox, oy, bx, by, fx, fy, pair, exact sum)]: every pair at integer displacement, then the 255 phases, each on the first pair of its rotation whose exact sum an `int`
    holds (at 10 bits a complement pair of more than 2052 samples does not fit) — `skipped` counts the pairs passed over"""
    org, buf = err_planes(bd)
    o64, b64 = org.astype(np.int64), buf.astype(np.int64)
    out, skipped, n = [], 0, w * 7 + h
    for pair in PAIRS:
        ox, oy, bx, by = _place(pair, n, w, h)
        e = err_model(o64, oy, ox, b64, by, bx, w, h, 0, 0, tap4, bd)
        n += 1
        if e <= INT_MAX:
            out.append((ox, oy, bx, by, 0, 0, pair, e))
        else:
            skipped += 1
    for ph in range(1, 256):
        fx, fy = ph % 16, ph // 16
        for k in range(len(PAIRS)):
            pair = PAIRS[(ph + k) % len(PAIRS)]
            ox, oy, bx, by = _place(pair, n, w, h)
            e = err_model(o64, oy, ox, b64, by, bx, w, h, fx, fy, tap4, bd)
            n += 1
            if e <= INT_MAX:
                out.append((ox, oy, bx, by, fx, fy, pair, e))
                break
            skipped += 1
        else:
            raise AssertionError("no pair fits", bd, w, h, ph)
    return out, skipped


def err_records(items):
    r = np.zeros(len(items), ERR_ITEM)
    for k, it in enumerate(items):
        r[k] = (it[1] * ORG_W + it[0], it[3] * BUF_W + it[2], it[4], it[5])
    return r


def sat_bound(bd, w, h):
    """the largest sum of w x h squared differences that a reference `int` holds"""
    mx = (1 << bd) - 1
    return min(w * h * mx * mx, INT_MAX)


@lru_cache(maxsize=None)
def saturated(bd):
    """(org, buf, [(ox, oy, bx, by, w, h)]): per size one page pair at integer displacement whose sum is sat_bound exactly — buf is max against org 0 on the leading samples
    of the block in raster order, then the greedy squares of the remainder, then 0.  Both planes at pitch BUF_W, odd columns"""
    mx = (1 << bd) - 1
    ph = 68
    org = np.zeros((4 + ph * len(ERR_SIZES) + 4, BUF_W), np.int64)
    buf = np.zeros_like(org)
    items = []
    for k, (w, h) in enumerate(ERR_SIZES):
        left, vals = sat_bound(bd, w, h), []
        while left and len(vals) < w * h:
            v = min(mx, int(np.sqrt(left)))
            while v * v > left:
                v -= 1
            vals.append(v)
            left -= v * v
        assert left == 0, (bd, w, h, left)
        blk = np.zeros(w * h, np.int64)
        blk[:len(vals)] = vals
        ox, oy, bx, by = 1 + 2 * (k % 8), 4 + k * ph + k % 3, 3 + 2 * (k % 5), 4 + k * ph + (k + 1) % 3
        if k % 2:                                                      # every second size the other way round: org holds the large values (negative differences)
            org[oy:oy + h, ox:ox + w] = blk.reshape(h, w)
        else:
            buf[by:by + h, bx:bx + w] = blk.reshape(h, w)
        items.append((ox, oy, bx, by, w, h))
    return _ro(org), _ro(buf), items


# ---- variance, subsample, border ------------------------------------------------------------------------------------------------------------------------------
def var_model(a, y, x, w, h, mut=()):
    """calcVarCore: (returns variance * 256 as an integer; the reference returns it / 256.0)"""
    blk = a[y:y + h, x:x + w]
    sh = 0 if "var_no_shift" in mut else 4
    avg = (int(blk.sum()) << sh) // (w * h)
    d = (blk << sh) - avg
    return int((d * d).sum())


VAR_SIZES = ERR_SIZES + ((1, 1), (4, 4), (12, 4), (3, 5), (1, 128), (128, 1), (128, 64), (128, 128))      # every size of the search and the error entry, the smallest and the largest
VAR_KINDS = ("zero", "max", "half_h", "half_v", "checker1", "near_hi", "texture")


@lru_cache(maxsize=None)
def var_plane(bd):
    """the kinds stacked, 136 rows x 136 columns each (a 128x128 block at offsets 0 .. 8)"""
    mx = (1 << bd) - 1
    pages = []
    for k in VAR_KINDS:
        if k == "half_h":
            p = np.zeros((136, 136), np.int16); p[:, 1::2] = mx          # half 0 / half max whatever the (even-sized) block: alternate columns
        elif k == "half_v":
            p = np.zeros((136, 136), np.int16); p[0::2, :] = mx
        else:
            p = fill(k, mx, 136, 136, 3)
        pages.append(p)
    return _ro(np.concatenate(pages))


def var_items(w, h):
    """[(x, y, kind)]"""
    return [((3 * i + w) % 8 + (1 if i % 2 else 0), i * 136 + (5 * i + h) % 8, k) for i, k in enumerate(VAR_KINDS)]


def subsample_model(a, mut=()):
    a = a.astype(np.int64)
    h, w = a.shape[0] // 2 * 2, a.shape[1] // 2 * 2
    r = 0 if "sub_no_round" in mut else 2
    return (a[0:h:2, 0:w:2] + a[1:h:2, 0:w:2] + a[0:h:2, 1:w:2] + a[1:h:2, 1:w:2] + r) >> 2


def border_model(a, pad):
    return np.pad(a, pad, mode="edge")


PLANE_PADS = (0, 1, 16, 128)


@lru_cache(maxsize=None)
def plane_cases(bd):
    """[(name, plane)]: max-valued, checkers (the sums 2 max and max: (a + b + c + d + 2) >> 2 with every remainder comes from near_hi), the smallest sizes, odd sizes"""
    mx = (1 << bd) - 1
    out = []
    for kind, h, w in (("max", 6, 10), ("checker1", 8, 16), ("vstripe1", 9, 21), ("near_hi", 23, 37), ("near_lo", 16, 8), ("texture", 34, 50), ("hole", 12, 14), ("near_hi", 2, 2),
                       ("max", 3, 2), ("near_hi", 2, 3), ("checker1", 5, 301), ("near_hi", 1, 1), ("near_lo", 1, 7)):
        out.append(("%s %dx%d" % (kind, w, h), fill(kind, mx, h, w, 4)))
    return out


# ---- the search ------------------------------------------------------------------------------------------------------------------------------------------------
def search_params(speed):
    """(m_searchPttrn, m_lowResFltSearch), MCTF.cpp:598-599"""
    return (2 if speed >= 3 else (1 if speed > 0 else 0)), speed > 0


def reach(speed, add_level):
    """the largest integer displacement (full-resolution samples, either axis) that the schedule of estimateLumaLn can reach: range 8 at the coarsest level (:1185), the
    vector doubled from level to level plus the range of :1178 at each of the integer levels, nothing at the final level but fractions below one sample"""
    r = 3 if search_params(speed)[0] == 2 else 5
    v = 8
    for _ in range(3 if add_level else 2):
        v = 2 * v + r
    return v


def level_dims(w, h, unit):
    return [(w // (unit * 16) + 1, h // (unit * 16) + 1), (w // (unit * 8) + 1, h // (unit * 8) + 1), (w // (unit * 4) + 1, h // (unit * 4) + 1),
            (w // (unit * 2) + 1, h // (unit * 2) + 1), ((w + unit - 1) // unit, (h + unit - 1) // unit)]


def _new_field(dims):
    f = np.zeros((dims[1], dims[0]), MV_DTYPE)
    f["error"], f["rmsme"] = INT_MAX, 65535                            # MotionVector(), MCTF.h:79
    return f


def me_level_model(O, B, W, H, bs, prev, factor, dbl, pt, low, bd, unit, dims, mut=(), tr=None):
    """motionEstimationLuma on the padded int64 planes O, B (sample (0, 0) at [PAD, PAD]) -> field.  tr (a dict) collects per block: `n_min` the distinct vectors scored
    with the winning error, `nb` the neighbour tests as (error of the neighbour's vector - best so far) where the vector differs, `raw` the error before :1318, `norm` the
    double of :1318, `sizes` (w, h)"""
    mvs = _new_field(dims)
    le = "scan_le" in mut
    for by in range(0, H - 8 + 1, bs):
        for bx in range(0, W - 8 + 1, bs):
            w, h = min(bs, W - bx), min(bs, H - by)
            if "no_and7" not in mut:
                w, h = w & ~7, h & ~7
            o = O[PAD + by:PAD + by + h, PAD + bx:PAD + bx + w]
            memo = {}

            def err(dx, dy):
                if (dx, dy) not in memo:
                    fx, fy = dx & 15, dy & 15
                    if (fx | fy) == 0:
                        p = B[PAD + by + dy // 16:PAD + by + dy // 16 + h, PAD + bx + dx // 16:PAD + bx + dx // 16 + w]
                    else:
                        p = frac_block(B, PAD + by + (dy >> 4), PAD + bx + (dx >> 4), w, h, fx, fy, low, bd, mut)
                    d = p - o
                    memo[(dx, dy)] = int((d * d).sum())
                return memo[(dx, dy)]

            best = [0, 0, INT_MAX]

            def test(dx, dy):
                e = err(dx, dy)
                if (e <= best[2]) if le else (e < best[2]):
                    best[:] = [dx, dy, e]

            rng_ = 0 if dbl else (3 if pt == 2 else 5)
            if prev is None:
                rng_ = 8
            else:
                for py in (-1, 0, 1):
                    ty = by // (2 * bs) + py
                    if 0 <= ty < prev.shape[0]:
                        for px in (-1, 0, 1):
                            tx = bx // (2 * bs) + px
                            if 0 <= tx < prev.shape[1]:
                                test(int(prev[ty, tx]["x"]) * factor, int(prev[ty, tx]["y"]) * factor)
                test(0, 0)
            pbx, pby = best[0], best[1]
            d = 2 if (prev is None and pt == 2) else 1
            cy, cx = int(pby / 16), int(pbx / 16)                      # C division: towards zero
            grid = [(x2, y2) for y2 in range(cy - rng_, cy + rng_ + 1, d) for x2 in range(cx - rng_, cx + rng_ + 1, d)]
            if "col_major" in mut:
                grid = [(x2, y2) for x2 in range(cx - rng_, cx + rng_ + 1, d) for y2 in range(cy - rng_, cy + rng_ + 1, d)]
            for x2, y2 in grid:
                test(x2 * 16, y2 * 16)
            if dbl:
                for rr, st in ((6 if pt else 12, 6 if pt == 2 else 4), (2, 2), (1, 1)):
                    pbx, pby = best[0], best[1]
                    ring = [(x2, y2) for y2 in range(-rr, rr + 1, st) for x2 in range(-rr, rr + 1, st)]
                    if "col_major" in mut:
                        ring = [(x2, y2) for x2 in range(-rr, rr + 1, st) for y2 in range(-rr, rr + 1, st)]
                    for x2, y2 in ring:
                        if x2 or y2:
                            test(pbx + x2, pby + y2)
            nb = []
            for has, ny, nx in ((by > 0, by // bs - 1, bx // bs), (bx > 0, by // bs, bx // bs - 1)):
                if has:
                    vx, vy = int(mvs[ny, nx]["x"]), int(mvs[ny, nx]["y"])
                    e = err(vx, vy)
                    if (vx, vy) != (best[0], best[1]):
                        nb.append(e - best[2])
                    if (e <= best[2]) if ("neighbour_le" in mut or le) else (e < best[2]):
                        best[:] = [vx, vy, e]
            m = mvs[by // bs, bx // bs]
            m["x"], m["y"], m["error"] = best
            if tr is not None:
                tr.setdefault("n_min", []).append(sum(1 for v in memo.values() if v == best[2]))
                tr.setdefault("nb", []).extend(nb)
                tr.setdefault("acc", []).append(max(memo.values()))
            if dbl:
                scale = 1.0 if "no_bdscale" in mut else float(1 << (2 * (10 - bd)))
                dvar = var_model(O, PAD + by, PAD + bx, w, h) / 256.0 * scale
                mse = best[2] * scale / float(w * h)
                norm = 20 * ((best[2] * scale + 5.0) / (dvar + 5.0)) + mse / 50.0
                if tr is not None:
                    tr.setdefault("raw", []).append(best[2])
                    tr.setdefault("norm", []).append(norm)
                    tr.setdefault("sizes", []).append((w, h))
                m["error"] = int(norm)
                m["rmsme"] = int(0.5 + np.sqrt(mse)) & 0xffff
                m["overlap"] = float(w * h) / (unit * unit)
    return mvs


def me_model(org, ref, bd, unit, speed, add_level, mut=(), traces=None):
    """motionEstimationMCTF -> the five fields (the first None without add_level); traces: a list that receives one dict per level run"""
    pt, low = search_params(speed)
    o, r = [np.asarray(org, np.int64)], [np.asarray(ref, np.int64)]
    for _ in range(3):
        o.append(subsample_model(o[-1]))
        r.append(subsample_model(r[-1]))
    size = [(p.shape[1], p.shape[0]) for p in o]
    o = [border_model(p, PAD) for p in o]
    r = [border_model(p, PAD) for p in r]
    dims = level_dims(size[0][0], size[0][1], unit)
    res, prev = [None] * 5, None
    for k, l, bs, factor, dbl in ((0, 3, 2 * unit, 1, False), (1, 2, 2 * unit, 2, False), (2, 1, 2 * unit, 2, False), (3, 0, 2 * unit, 2, False), (4, 0, unit, 1, True)):
        if k == 0 and not add_level:
            continue
        tr = {} if traces is not None else None
        res[k] = me_level_model(o[l], r[l], size[l][0], size[l][1], bs, prev, factor, dbl, pt, low, bd, unit, dims[k], mut, tr)
        prev = res[k]
        if traces is not None:
            tr["level"] = k
            traces.append(tr)
    return res


class SearchCase:
    def __init__(self, name, family, org, ref, bd, unit, speed, add_level, tag=None):
        self.name, self.family, self.org, self.ref, self.bd, self.unit, self.speed, self.add_level, self.tag = name, family, _ro(org), _ro(ref), bd, unit, speed, bool(add_level), tag
        h, w = self.org.shape
        assert self.ref.shape == (h, w) and 64 <= w <= 208 and 64 <= h <= 136
        assert reach(speed, add_level) + 1 + 3 + 8 <= PAD          # the vector, a fraction, the taps, a vector load: inside the margin

    def expected(self, lib):
        return lib.mctf_me(self.org, self.ref, self.bd, self.unit, self.speed, self.add_level)

    def model(self, mut=(), traces=None):
        return me_model(self.org, self.ref, self.bd, self.unit, self.speed, self.add_level, mut, traces)


CONFIGS = tuple((unit, speed, add) for unit in (8, 16) for speed in (0, 2, 4) for add in (False, True))
# both dimensions multiples of 32; a remainder of 8; a remainder of 4 (the last column and row keep the default vector); one block row at the coarse levels; one block column
GEOMETRIES = ((64, 64), (72, 72), (68, 68), (208, 64), (64, 136))


# per (configuration, case) a seed of _unit_steps at which the model meets both neighbour events (found by trying the seeds in order; the CPU tier asserts the events per configuration)
F_SEEDS = (0, 0, 5, 4, 0, 0, 7, 0, 0, 0, 0, 0, 1, 35, 36, 0, 7, 0, 4, 0, 0, 2, 13, 0)


def _unit_steps(h, w, bd, seed):
    """(org, ref) of family (f): both flat at a level near the top of the range, ref with steps of +-1 on half of the samples: the errors are small integers, so a
    neighbour's vector now and then ties with a block's own best or beats it by one"""
    rng = np.random.default_rng(6100 + seed)
    v = (1 << bd) - 5
    org = np.full((h, w), v, np.int64)
    amp = rng.choice([-1, 1], (h, w))
    return org, org + np.where(rng.random((h, w)) < 0.5, amp, 0)


def _small_contents(bd, h, w, seed):
    """[(family, name, org, ref)] of the families a, b, c, f on one geometry"""
    mx = (1 << bd) - 1
    f = lambda k: fill(k, mx, h, w, seed).astype(np.int64)
    roll = lambda a, dy, dx: np.roll(a, (dy, dx), (0, 1))
    out = [("a", "flat equal", np.full((h, w), mx // 3), np.full((h, w), mx // 3)), ("b", "0 against max", f("zero"), f("max")), ("b", "max against 0", f("max"), f("zero")),
           ("c", "vstripe1 equal", f("vstripe1"), f("vstripe1")), ("c", "checker2 rolled", f("checker2"), roll(f("checker2"), 1, 1)),
           ("c", "checker4 rolled", f("checker4"), roll(f("checker4"), 2, 1)), ("c", "hstripe8 complement", f("hstripe8"), f("~hstripe8")),
           ("c", "checker16 rolled", f("checker16"), roll(f("checker16"), 3, 5)), ("c", "checker1 against vstripe1", f("checker1"), f("vstripe1"))]
    out += [("f", "unit steps %d" % k, *_unit_steps(h, w, bd, F_SEEDS[seed * 2 + k])) for k in (0, 1)]
    return out


@lru_cache(maxsize=None)
def search_small(cfg):
    """the families a, b, c, f of one (unit, speed, add_level): geometry and bit depth rotate over the contents, so that over the twelve configurations every content meets
    every geometry and both bit depths"""
    unit, speed, add = CONFIGS[cfg]
    out = []
    for i in range(11):
        (w, h), bd = GEOMETRIES[(i + cfg) % 5], BITDEPTHS[(i + cfg // 5) % 2]
        fam, name, org, ref = _small_contents(bd, h, w, cfg)[i]
        out.append(SearchCase("%s / %dx%d / %d bits / unit %d speed %d add %d" % (name, w, h, bd, unit, speed, add), fam, org, ref, bd, unit, speed, add))
    return out


DIRECTIONS = ((1, 1), (-1, 1), (1, -1), (-1, -1))
D_W, D_H = 208, 136


@lru_cache(maxsize=None)
def _canvas(bd, sx, sy):
    """a texture without repetition on a canvas of D_H + 200 rows: a ramp that rises along (sx, sy) over the whole canvas — against a reference displaced beyond a
    level's range every candidate's error is N (a ux + b uy)^2 plus a constant, with ux, uy the distances to the true vector, which all have one sign: the corner of the
    range nearest to the truth is the only minimum, at every level and whatever the margins replicate — under seeded noise of a few levels, which makes the match at
    the true vector the only exact one"""
    mx, amp = (1 << bd) - 1, 3 if bd == 10 else 1
    h, w = D_H + 200, D_W + 200
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    t = (xx if sx > 0 else w - 1 - xx) + (yy if sy > 0 else h - 1 - yy)
    t = amp + t * (mx - 2 * amp) / (h + w - 2)
    return np.floor(t).astype(np.int64) + np.random.default_rng(77 + bd).integers(-amp, amp + 1, (h, w))


@lru_cache(maxsize=None)
def search_displaced(cfg, bd):
    """family (d) at 10 bits / (e) at 8: ref is org displaced by the reach of the configuration in each diagonal direction"""
    unit, speed, add = CONFIGS[cfg]
    n = reach(speed, add)
    out = []
    for sx, sy in DIRECTIONS:
        t = _canvas(bd, sx, sy)
        assert t.min() >= 0 and t.max() <= (1 << bd) - 1
        org = t[100:100 + D_H, 100:100 + D_W]
        ref = t[100 - sy * n:100 - sy * n + D_H, 100 - sx * n:100 - sx * n + D_W]          # ref[y + sy n][x + sx n] == org[y][x]: the vector of a block is (sx n, sy n)
        out.append(SearchCase("displaced (%+d, %+d) x %d / %d bits / unit %d speed %d add %d" % (sx, sy, n, bd, unit, speed, add), "d" if bd == 10 else "e", org, ref, bd, unit, speed, add, (sx, sy, n)))
    return out


def search_cases(cfg):
    """every search case of one configuration: a, b, c, f on the small geometries, (d) in four directions at 10 bits, (e) in one direction at 8"""
    return search_small(cfg) + search_displaced(cfg, 10) + [search_displaced(cfg, 8)[cfg % 4]]


FALLBACK = ((3, 3), (3, 5), (8, 7), (8, 4))   # (configuration, index into search_small) of family (c) for the wavefront fallback; (d) joins with search_displaced(3, 10)[0] and (8, 10)[3]


def fallback_cases():
    return [search_small(c)[i] for c, i in FALLBACK] + [search_displaced(3, 10)[0], search_displaced(8, 10)[3]]


# ---- the apply side ----------------------------------------------------------------------------------------------------------------------------------------------
XSZM = (0, 1, 20, 336, 5440, 87296)
REF_STRENGTHS = (0.84375, 0.6, 0.4286, 0.3333, 0.2727, 0.2308)      # MCTF.cpp:112-117, the row of m_picReordering


def filter_params(qp, bd, chroma, overall=0.95):
    """(sigmaSq, weightScaling), MCTF.cpp:1491-1501 and :1417"""
    bdw = 1024.0 / (1 << bd)
    return (900.0 if chroma else 9.0 * (128.0 + 3.0 / 256.0 * qp * qp * qp)) / (bdw * bdw), overall * (0.55 if chroma else 0.4)


def planar_model(org, comp, bd, rmsme, tr=None):
    """applyPlanarCorrectionCore on the compensated block `comp` against the original block `org` (both int64, square)"""
    h, w = comp.shape
    mx, bs, l2 = (1 << bd) - 1, w * h, w.bit_length() - 1
    mw = min(512, rmsme * rmsme)
    yy, xx = np.mgrid[0:h, 0:w]
    z = comp - org
    x1, x2, ys = int((xx * z).sum()), int((yy * z).sum()), int(z.sum())
    xsum = (bs * (w - 1)) >> 1
    if tr is not None:
        tr.append(xsum * ys)                                           # an `int` product in the reference (:396, :399)
    den = bs * XSZM[l2]

    def div(n):
        n = n - (den >> 1) if n < 0 else n + (den >> 1)
        return -((-n) // den) if n < 0 else n // den                   # C division: towards zero

    b1 = min(max(div(mw * (x1 * bs - xsum * ys)), -32768), 32767)
    b2 = min(max(div(mw * (x2 * bs - xsum * ys)), -32768), 32767)
    b0 = (mw * ys - (b1 + b2) * xsum + (bs >> 1)) >> (l2 << 1)
    if b0 == 0 and b1 == 0 and b2 == 0:
        return comp
    return np.clip(comp - ((b0 + b1 * xx + b2 * yy + 256) >> 9), 0, mx)


class ApplyCase:
    """org: (Y, U, V); refs: [(Y, U, V)]; mvs: [MV_DTYPE field of ceil(w / unit) x ceil(h / unit), flat]; ref_index: rows of REF_STRENGTHS"""

    def __init__(self, name, org, refs, mvs, ref_index, bd, qp, unit, low_res):
        self.name, self.org, self.refs, self.mvs, self.ref_index, self.bd, self.qp, self.unit, self.low_res = name, org, refs, mvs, ref_index, bd, qp, unit, low_res
        h, w = org[0].shape
        assert w <= 96 and h <= 64 and w % 2 == 0 and h % 2 == 0
        self.wb, self.hb = (w + unit - 1) // unit, (h + unit - 1) // unit
        assert all(m.size == self.wb * self.hb for m in mvs) and len(refs) == len(mvs) == len(ref_index)
        for m in mvs:                                                  # the vector, the taps and a vector load stay inside the margins (128 luma, 64 chroma)
            assert max(int(np.abs(m["x"]).max()), int(np.abs(m["y"]).max())) <= 99 * 16 + 15

    def expected(self, lib):
        return lib.mctf_bilateral(self.org, self.refs, self.mvs, self.ref_index, self.bd, self.qp, self.unit, self.low_res, True, 0.95)

    def blocks(self, c):
        """(bx, by, w, h, index into the motion field) of component c"""
        cs = 1 if c else 0
        H, W = self.org[c].shape
        blk = self.unit >> cs
        return [(bx, by, min(blk, W - bx), min(blk, H - by), (by // blk) * self.wb + bx // blk) for by in range(0, H, blk) for bx in range(0, W, blk)]

    def intermediates(self, mut=()):
        """per (component, block, reference), from the model of the two filter passes and the plane fit: dict(comp = the compensated block, noise = the double of
        MCTF.cpp:474, base = the smallest 1 - diffSq / (1024 vsw) of :362, planar = whether the plane fit ran, prod = its `int` product, first = the first pass's extremes,
        second = the second pass's value before the clip)"""
        out = []
        for c in range(3):
            cs = 1 if c else 0
            pad = PAD >> cs
            O = self.org[c].astype(np.int64)
            sigma, _ = filter_params(self.qp, self.bd, c > 0)
            for i, (r, m) in enumerate(zip(self.refs, self.mvs)):
                R = border_model(r[c].astype(np.int64), pad)
                for (bx, by, w, h, k) in self.blocks(c):
                    mv = m[k]
                    dx, dy = int(mv["x"]) >> cs, int(mv["y"]) >> cs
                    comp = frac_block(R, pad + by + (dy >> 4), pad + bx + (dx >> 4), w, h, dx & 15, dy & 15, self.low_res, self.bd, mut, apply=True)
                    raw = frac_block(R, pad + by + (dy >> 4), pad + bx + (dx >> 4), w, h, dx & 15, dy & 15, self.low_res, self.bd, mut, apply=True, clip=False)
                    o = O[by:by + h, bx:bx + w]
                    prod = []
                    gate = self.qp < 32 if "planar_lt32" in mut else self.qp <= 32
                    planar = int(mv["rmsme"]) > 0 and gate and w == h and w <= 32
                    if planar:
                        comp = planar_model(o, comp, self.bd, int(mv["rmsme"]) & 0xffff, prod)
                    d = o - comp
                    sc = 1 << (2 * (10 - self.bd))
                    var = int((d * d).sum()) * sc
                    ds = (int(((d[:, 1:] - d[:, :-1]) ** 2).sum()) + int(((d[1:] - d[:-1]) ** 2).sum())) * sc
                    cv, cd = w * h, 2 * w * h - w - h
                    noise = (15.0 * cd / cv * var + 5.0) / (ds + 5.0)
                    err = int(mv["error"])
                    sw = (1.0 if round(noise) < 25 else 0.8) * (1.0 if err < 50 else 0.8)
                    base = 1.0 - float((d * d).max()) / (np.float32(sw * 2 * sigma) * 1024.0)
                    out.append(dict(c=c, ref=i, block=k, size=(w, h), comp=comp, noise=noise, base=base, planar=planar, prod=prod[0] if prod else 0, error=err,
                                    lo=int(raw.min()), hi=int(raw.max()), phase=(int(mv["x"]) & 15, int(mv["y"]) & 15), cphase=(dx & 15, dy & 15)))
        return out


APPLY_SIZES = ((96, 64), (92, 60), (88, 56), (84, 52))      # the last luma block of unit 16: full, 12, 8 and 4 wide / high; the last chroma block of unit 16: 8, 6, 4, 2
APPLY_QPS = (0, 32, 33, 63)
APPLY_NREFS = (1, 2, 8, 12)
APPLY_ERRS = (0, 49, 50, 100, 101, 7, 1000, 1 << 20)
APPLY_RMSME = (0, 1, 5, 22, 23, 300, 0, 1023)
APPLY_INTS = (0, 1, -1, 2, -3, 7, -8)
APPLY_ORG = ("checker1", "near_hi", "checker2", "near_lo", "vstripe1", "hole", "hstripe2", "impulse", "texture", "max", "checker4", "zero")
_HI, _LO = ("near_hi", "hole", "checker1", "texture", "~checker2", "max"), ("near_lo", "impulse", "checker1", "texture", "checker2", "zero")
FAR = 99 * 16 + 15                                            # reach(0, True) samples and the largest fraction


def _ref_kinds(org_kind):
    if org_kind in ("max", "near_hi", "hole"):
        return _HI
    if org_kind in ("zero", "near_lo", "impulse"):
        return _LO
    if org_kind == "texture":
        return ("texture", "near_hi", "near_lo", "checker8", "texture", "~checker1")
    return ("~" + org_kind, org_kind, "texture", "near_hi", "near_lo", "~checker4")


def _yuv(kind, mx, w, h, seed):
    return tuple(fill(kind, mx, h >> (1 if c else 0), w >> (1 if c else 0), seed + c) for c in range(3))


@lru_cache(maxsize=None)
def apply_cases():
    """units 8, 16, 32 x low_res x bit depth, twice: QP, the number of references, the picture size and the original's kind rotate.  The motion fields walk through all 256
    phases (the counter runs on over the cases), integer parts of both signs and parities, the errors and rmsme values above; the four corner blocks of reference 0 point
    outwards by FAR"""
    out, cnt = [], 0
    combos = [(u, lr, bd) for u in (8, 16, 32) for lr in (False, True) for bd in BITDEPTHS]
    for k in range(2 * len(combos)):
        unit, low_res, bd = combos[k % len(combos)]
        mx = (1 << bd) - 1
        qp, nrefs = APPLY_QPS[(k + k // 12) % 4], APPLY_NREFS[(k // 2 + k // 12) % 4]
        w, h = APPLY_SIZES[(k + k // 4) % 4]
        ok = APPLY_ORG[k % len(APPLY_ORG)]
        kinds = _ref_kinds(ok)
        if unit == 32:                                         # 32x32 luma blocks: two-level pages only — no flat offset (MCTF.cpp:474) and a plane fit without a mean (:396)
            ok = ("checker1", "checker2", "vstripe1", "hstripe2")[k % 4]
            kinds = ("~" + ok, ok, "~checker4", "checker8")
            qp = 33 + 30 * (k // 12)                          # and no plane fit at all: a far vector lands in the flat margin, where the mean difference is half the range
        org = _yuv(ok, mx, w, h, 10 * k)
        refs = [_yuv(kinds[(i + k) % len(kinds)], mx, w, h, 10 * k + 3 * i + 1) for i in range(nrefs)]
        wb, hb = (w + unit - 1) // unit, (h + unit - 1) // unit
        mvs = []
        for i in range(nrefs):
            m = np.zeros(wb * hb, MV_DTYPE)
            for b in range(wb * hb):
                ix, iy = APPLY_INTS[(cnt + b) % 7], APPLY_INTS[(cnt // 3 + 2 * b) % 7]
                m[b] = (ix * 16 + cnt % 16, iy * 16 + (cnt // 16) % 16, APPLY_ERRS[(cnt + i) % 8], APPLY_RMSME[(cnt // 2 + b) % 8], 1.0)
                cnt += 1
            if i == 0:
                for b, sx, sy in ((0, -1, -1), (wb - 1, 1, -1), ((hb - 1) * wb, -1, 1), (hb * wb - 1, 1, 1)):
                    m[b]["x"], m[b]["y"] = sx * FAR, sy * FAR
            mvs.append(m)
        name = "%s %dx%d / unit %d / %s / %d bits / QP %d / %d refs" % (ok, w, h, unit, "4-tap" if low_res else "6-tap", bd, qp, nrefs)
        out.append(ApplyCase(name, org, refs, mvs, [(i + k) % 6 for i in range(nrefs)], bd, qp, unit, low_res))
    return out


@lru_cache(maxsize=None)
def noise_cases():
    """vnoise on both sides of 25: zero vectors and rmsme 0, so the compensated block is the reference block; per 16x16 luma block the reference is the original plus an
    offset c and a seeded disturbance of +-3, with c the first (block even) / the last (block odd) offset whose noise value rounds to 24 / to 25 — searched here with the
    formula of MCTF.cpp:474 on the block, asserted by the CPU tier through ApplyCase.intermediates"""
    out = []
    for bd, low_res in ((10, False), (8, True)):
        mx, sc = (1 << bd) - 1, 1 << (2 * (10 - bd))
        w, h, unit = 96, 64, 16
        org = _yuv("texture", mx, w, h, 900 + bd)
        rng = np.random.default_rng(910 + bd)
        ref = [org[0].astype(np.int64), org[1].astype(np.int64) + 2, org[2].astype(np.int64) - 2]
        want = 24
        for by in range(0, h, unit):
            for bx in range(0, w, unit):
                o = org[0][by:by + unit, bx:bx + unit].astype(np.int64)
                for tries in range(400):
                    e = rng.integers(-3, 4, (unit, unit))
                    hit = None
                    for c in range(0, 12):
                        d = -(c + e)
                        var = int((d * d).sum()) * sc
                        ds = (int(((d[:, 1:] - d[:, :-1]) ** 2).sum()) + int(((d[1:] - d[:-1]) ** 2).sum())) * sc
                        if round((15.0 * (2 * 256 - 32) / 256 * var + 5.0) / (ds + 5.0)) == want and o.min() + c - 3 >= 0 and o.max() + c + 3 <= mx:
                            hit = c
                            break
                    if hit is not None:
                        break
                assert hit is not None, (bd, bx, by)
                ref[0][by:by + unit, bx:bx + unit] = o + hit + e
                want = 49 - want
        m = np.zeros(24, MV_DTYPE)
        m["error"], m["overlap"] = [APPLY_ERRS[b % 5] for b in range(24)], 1.0
        out.append(ApplyCase("noise 24 / 25 / %d bits" % bd, org, [tuple(_ro(p) for p in ref)], [m], [0], bd, 33, unit, low_res))
    return out
