"""Deterministic extreme inputs of the decoder-side refinement search (vvhip_dmvr_refine_batch) and the two search-side SAD entries next to it (vvhip_sad_x5_batch,
vvhip_sad_surface), shared by the CPU tier (tests/test_oracle_dmvr_extremes.py: oracle against the compiled reference, the guards, the sensitivity test) and the GPU
tier (tests/test_gpu_dmvr_extremes.py: the three entries against the oracle, tolerance 0).

The parity suites run the search on a smooth sinusoid with noise at interior positions: costs stay below 2^16, the early exit is never met at equality, few of the
fifteen quotients of div_for_maxq7 and few of the 25 positions occur, both planes share one row pitch, and nothing lies next to the blocks that the kernel's wider
loads could pick up.  The families here:
  saturated   two-level planes of (0, 2^bd - 1) in both lists: the largest cost a size allows (all 25 costs of 16x16 are beyond 2^16), every bilinear path on extremes
  threshold   flat planes at 10 bits whose reduced centre cost is dx * dy - 1, dx * dy and dx * dy + 1: the early exit `centre < dx * dy` on both sides of equality
  surface     list 0 flat, list 1 = c0 + g(column) + f(row) with g, f >= 0: cost(hor, ver) = A(hor) + B(ver) with A(hor) = dy / 2 * sum of g over the columns the position
              covers and B(ver) = dx * sum of f over the EVEN rows it covers — the values of g and f on the five samples at each end of the block set both profiles freely.
              Six constructed ties, one constructed draw per position and seeded draws give, per size and axis: every quotient -7 .. 7, +8 at and off the centre, -8 (at the centre only: the scan is
              strict, so a left / top neighbour as cheap as the winner would have won), a zero denominator, and each of the 25 positions winning
  phases      a textured and a two-level plane with all 256 (fx, fy) of either list, and the 16 pairs of code paths (copy, horizontal, vertical, both; per list)
  layout      row pitches 320 and 200 (different, neither a power of two), every pair of residues modulo 8 of the two block columns, blocks at the first and at the last
              sample the entry may read (kernel_footprint), and every sample inside the kernel's footprint but outside the reference's own an alternating -32768 / 32767
  tie_pairs   list 0 flat, list 1 raised everywhere but on the samples two positions cover: exactly these two tie at cost 0, and of each pair one comes first in the
              reference's raster order and the other in a column-major order
  lists       n in LIST_NS (partial last workgroups of four sub-blocks; grids below, at and beyond multiples of the eight-way remap), the same list shuffled, identical items
Bit depth 9, which the entry accepts, is part of every family but `threshold` (the CPU tier shows oracle == reference there, both rows).

SAD-X5: widths 8 / 16 x heights 4 .. 128 x sub_shift x calc_centre x n in X5_NS — 5 n teams of 2 .. 64 lanes against 256-lane workgroups — on two-level planes of 8, 10,
12 (0 .. 4095 and -2048 .. 2047) and 15 bits, with odd cur offsets, one item whose cur - 4 is the first sample of the plane and one whose org + 4 block ends at its last.  The oracle equals the
reference's scalar row on all of it.  The x86 row is DMVR's own routine and no general one (x5_rows_agree; the CPU tier finds these rules and leaves it out by them): it
sums a column pair's differences over the rows in a signed 16-bit lane, so the two rows agree while rows * (max - min) <= 32767 — at DMVR's heights (8 rows of 16) up to
12-bit operands, which is the widest range of the planes compared with both rows; and its 16-wide form takes every second row whatever sub_shift says and eight rows
per trip, so it has no sub_shift 0 and no height 4.

SAD surface: sizes x ranges x sub_shift on uniform 10-bit, two-level 8- and 10-bit and full-range planes (-32768 / 32767 checker against its complement: every
difference is 65535 and a 128x128 surface value 2^30 — the biased v_sad_u16 and the 32-bit accumulator), the four KDY instantiations (the host's formula, restated in
surface_launch for the guard only), n_blocks = 1 (the maximal gridDim.y split) against the same blocks in a list of 1025 (no split), a window between 64 KiB and
160 KiB of LDS and one beyond 160 KiB (refused).

The int64 model below restates the bilinear two-pass with the reference's shifts (InterpolationFilter.cpp:662-681), the mirrored every-second-row SAD, the quarter
reduction, the threshold, the raster scan and xSubPelErrorSrfc (InterPrediction.cpp:1131-1187, :1312-1384), xGetSAD8X5 / 16X5 (RdCost.cpp:1984-2034) and the SAD
surface.  It serves the guards and the mutations of the sensitivity test only: expected values of both tiers come from oracle.dmvr_refine, oracle.sad_x5 and
oracle.dist("SAD", ...), never from it.  Numpy only: no GPU, no oracle, no reference.
"""
from functools import lru_cache

import numpy as np

from interp_extremes import filler

SIZES = ((16, 16), (8, 8), (16, 8), (8, 16))
BITDEPTHS = (8, 9, 10)
SENTINELS = (-32768, 32767)

# the layouts of vvhip_dmvr_item / vvhip_dmvr_result (vvenc_amd.hotpath.DMVR_ITEM_DTYPE / DMVR_RESULT_DTYPE; restated so that the CPU tier imports nothing of the device package)
DMVR_ITEM = np.dtype([("ref0_off", "<i4"), ("ref1_off", "<i4"), ("frac0_x", "<i2"), ("frac0_y", "<i2"), ("frac1_x", "<i2"), ("frac1_y", "<i2")])
DMVR_RESULT = np.dtype([("mvd_x", "<i2"), ("mvd_y", "<i2"), ("pad", "<i4"), ("min_cost", "<u8")])


def _ro(v):
    return np.ascontiguousarray(v, np.int16)


# ---- read footprints (rows and columns relative to ref*_off, inclusive) ---------------------------------------------------------
def kernel_footprint(dx, dy):
    """what dmvrRefineKernel loads of either list whatever the fractions: rows 0 .. dy + 4 of the window at (-2, -2), and per row `segs` = (dx + 4 + 7) >> 3 lanes of ten
    samples (a 16-byte load and a dword) at a pitch of eight -> (row_lo, row_hi, col_lo, col_hi) = (-2, dy + 2, -2, 8 * segs - 1): 21 rows x 26 columns at 16x16"""
    segs = (dx + 4 + 7) >> 3
    return -2, dy + 2, -2, 8 * segs - 1


def reference_footprint(dx, dy, fx, fy):
    """what filterN2_2D reads for the (dx + 4) x (dy + 4) prediction: one more column with a horizontal fraction, one more row with a vertical one"""
    return -2, dy + 1 + (1 if fy else 0), -2, dx + 1 + (1 if fx else 0)


# ---- the int64 model ------------------------------------------------------------------------------------------------------------
MUTATIONS = ("scan_le", "no_quarter", "thr_gt", "cost_mod16", "no_round1_8", "shift2_from_1", "odd_rows", "no_mirror", "pm8_swapped", "surface_on_border", "col_major_ties",
             "x5_plus", "x5_no_shift")


def wrap16(v):
    return ((v + 32768) & 0xffff) - 32768


def bilinear(a, y, x, w, h, fx, fy, bd, mut=()):
    """filterN2_2D: the w x h bilinear prediction at (x, y) of the int64 array a, 10-bit internal precision, no clipping, Pel truncation after each pass"""
    sh1 = 4 - (10 - bd)
    of1 = 0 if ("no_round1_8" in mut and bd == 8) else 1 << (sh1 - 1)
    s = a[y:y + h + 1, x:x + w + 1]
    if not fx and not fy:
        return wrap16(s[:h, :w] << (10 - bd))
    if fx and fy:
        t = wrap16(((16 - fx) * s[:h + 1, :w] + fx * s[:h + 1, 1:w + 1] + of1) >> sh1)
        sh2, of2 = (sh1, 1 << (sh1 - 1)) if "shift2_from_1" in mut else (4, 8)
        return wrap16(((16 - fy) * t[:h] + fy * t[1:h + 1] + of2) >> sh2)
    if fx:
        return wrap16(((16 - fx) * s[:h, :w] + fx * s[:h, 1:w + 1] + of1) >> sh1)
    return wrap16(((16 - fy) * s[:h, :w] + fy * s[1:h + 1, :w] + of1) >> sh1)


def div_for_maxq7(n, d):
    sign, q = 0, 0
    if n < 0:
        sign, n = 1, -n
    d <<= 3
    if n >= d:
        n -= d; q += 1
    q <<= 1
    d >>= 1
    if n >= d:
        n -= d; q += 1
    q <<= 1
    if n >= (d >> 1):
        q += 1
    return -q if sign else q


def error_surface_axis(w, lo, hi, mut=()):
    """one axis of xSubPelErrorSrfc: winner's cost w, the neighbour before it (left / top) and after it -> (delta, branch)"""
    den = lo + hi - 2 * w
    if den == 0:
        return 0, ("den0",)
    if lo != w and hi != w:
        q = div_for_maxq7((lo - hi) << 4, den)
        return q, ("q", q)
    m8, p8 = (8, -8) if "pm8_swapped" in mut else (-8, 8)
    return (m8, ("m8",)) if lo == w else (p8, ("p8",))


def search(cost25, dx, dy, mut=(), tr=None):
    """the search of DMVR::xProcessDMVR on the 25 raw costs (raster order, the centre not yet reduced) -> (mvd_x, mvd_y, min_cost)"""
    sad = [int(c) for c in cost25]
    c = sad[12]
    red = c if "no_quarter" in mut else c - (c >> 2)
    if tr is not None:
        tr.update(costs=list(sad), centre=red, searched=False, winner=(0, 0), branches=None)
    if (red <= dx * dy) if "thr_gt" in mut else (red < dx * dy):
        return 0, 0, red
    sad[12] = red
    best, bh, bv = red, 0, 0
    order = [(h, v) for h in range(-2, 3) for v in range(-2, 3)] if "col_major_ties" in mut else [(h, v) for v in range(-2, 3) for h in range(-2, 3)]
    for h, v in order:
        k = sad[(v + 2) * 5 + h + 2]
        if (k <= best) if "scan_le" in mut else (k < best):
            best, bh, bv = k, h, v
    tx, ty = 16 * bh, 16 * bv
    br = None
    if "surface_on_border" in mut or (abs(bh) != 2 and abs(bv) != 2):
        p = 12 + bv * 5 + bh
        at = lambda i: sad[i % 25]
        ex, b0 = error_surface_axis(at(p), at(p - 1), at(p + 1), mut)
        ey, b1 = error_surface_axis(at(p), at(p - 5), at(p + 5), mut)
        tx, ty, br = tx + ex, ty + ey, (b0, b1)
    if tr is not None:
        tr.update(costs=list(sad), searched=True, winner=(bh, bv), branches=br)
    return tx, ty, best


def dmvr_model(a0, y0, x0, a1, y1, x1, f0, f1, dx, dy, bd, mut=(), tr=None):
    """one sub-block end to end on int64 planes: (x, y) = the integer position of the merge vector of either list"""
    p0 = bilinear(a0, y0 - 2, x0 - 2, dx + 4, dy + 4, f0[0], f0[1], bd, mut)
    p1 = bilinear(a1, y1 - 2, x1 - 2, dx + 4, dy + 4, f1[0], f1[1], bd, mut)
    rows = np.arange(1 if "odd_rows" in mut else 0, dy, 2)
    costs = []
    for v in range(-2, 3):
        for h in range(-2, 3):
            h1, v1 = (h, v) if "no_mirror" in mut else (-h, -v)
            s = int(np.abs(p0[2 + v + rows, 2 + h:2 + h + dx] - p1[2 + v1 + rows, 2 + h1:2 + h1 + dx]).sum())
            s = (s << 1) >> 1                                  # xGetSAD with subShift 1, then the callers' >> 1
            costs.append(s & 0xffff if "cost_mod16" in mut else s)
    return search(costs, dx, dy, mut, tr)


def x5_model(org, oy, ox, cur, cy, cx, w, h, ss, calc_centre, mut=()):
    """xGetSAD8X5 / 16X5: SAD(org + k, cur - k) >> 1 for k = 0 .. 4; entry 2 is None when calc_centre is 0"""
    out = []
    for k in range(5):
        if k == 2 and not calc_centre:
            out.append(None)
            continue
        kc = k if "x5_plus" in mut else -k
        s = int(np.abs(org[oy:oy + h:1 << ss, ox + k:ox + k + w].astype(np.int64) - cur[cy:cy + h:1 << ss, cx + kc:cx + kc + w]).sum()) << ss
        out.append(s if "x5_no_shift" in mut else s >> 1)
    return out


def surface_model(org, oy, ox, ref, ry0, rx0, w, h, ss, rx, ry):
    """(2 ry + 1, 2 rx + 1) int64: xGetSAD of the block against every displacement"""
    o = org[oy:oy + h:1 << ss, ox:ox + w].astype(np.int64)
    out = np.zeros((2 * ry + 1, 2 * rx + 1), np.int64)
    for dy in range(-ry, ry + 1):
        for dx in range(-rx, rx + 1):
            out[dy + ry, dx + rx] = int(np.abs(o - ref[ry0 + dy:ry0 + dy + h:1 << ss, rx0 + dx:rx0 + dx + w]).sum()) << ss
    return out


# ---- DMVR families ----------------------------------------------------------------------------------------------------------------
ITEM = np.dtype([("x0", "<i4"), ("y0", "<i4"), ("x1", "<i4"), ("y1", "<i4"), ("f0x", "<i2"), ("f0y", "<i2"), ("f1x", "<i2"), ("f1y", "<i2")])


class Family:
    """one list: the two planes (any sizes; their widths are multiples of 8, so a device plane keeps them as row pitches) and the items' positions and fractions"""

    def __init__(self, name, bd, dx, dy, ref0, ref1, items, tags=None):
        self.name, self.bd, self.dx, self.dy, self.ref0, self.ref1 = name, bd, dx, dy, _ro(ref0), _ro(ref1)
        self.items = np.array(items, ITEM)
        self.tags = tags
        assert self.ref0.shape[1] % 8 == 0 and self.ref1.shape[1] % 8 == 0
        r_lo, r_hi, c_lo, c_hi = kernel_footprint(dx, dy)
        for l, a in ((0, self.ref0), (1, self.ref1)):              # the kernel's loads stay inside the planes
            x, y = self.items["x%d" % l], self.items["y%d" % l]
            assert not self.items.size or (x.min() + c_lo >= 0 and y.min() + r_lo >= 0 and x.max() + c_hi < a.shape[1] and y.max() + r_hi < a.shape[0]), (name, bd, dx, dy, l)

    def __len__(self):
        return self.items.size

    def records(self, stride0, stride1, sel=None):
        it = self.items if sel is None else self.items[sel]
        r = np.zeros(it.size, DMVR_ITEM)
        r["ref0_off"], r["ref1_off"] = it["y0"] * stride0 + it["x0"], it["y1"] * stride1 + it["x1"]
        r["frac0_x"], r["frac0_y"], r["frac1_x"], r["frac1_y"] = it["f0x"], it["f0y"], it["f1x"], it["f1y"]
        return r

    def host(self, ref0=None, ref1=None):
        """the planes for a host call: two rows of slack below (a vector load of the x86 row may run past the last sample the filter uses)"""
        pad = lambda a: _ro(np.concatenate([a, np.zeros((2, a.shape[1]), np.int16)]))
        return pad(self.ref0 if ref0 is None else ref0), pad(self.ref1 if ref1 is None else ref1)

    def expected(self, lib, ref0=None, ref1=None):
        """[(mvd_x, mvd_y, min_cost)] from lib.dmvr_refine (the oracle or a reference row)"""
        h0, h1 = self.host(ref0, ref1)
        return [lib.dmvr_refine((h0, int(i["y0"]), int(i["x0"])), (h1, int(i["y1"]), int(i["x1"])), (int(i["f0x"]), int(i["f0y"])), (int(i["f1x"]), int(i["f1y"])), self.dx, self.dy, self.bd)
                for i in self.items]

    def model(self, mut=(), traces=None):
        a0, a1 = self.ref0.astype(np.int64), self.ref1.astype(np.int64)
        out = []
        for i in self.items:
            tr = {} if traces is not None else None
            out.append(dmvr_model(a0, int(i["y0"]), int(i["x0"]), a1, int(i["y1"]), int(i["x1"]), (int(i["f0x"]), int(i["f0y"])), (int(i["f1x"]), int(i["f1y"])), self.dx, self.dy, self.bd, mut, tr))
            if traces is not None:
                traces.append(tr)
        return out


PH, PW = 32, 48                               # a small plane: a 16x16 block at (8 .. 13, 6 .. 8) with the kernel's footprint inside
FRACS6 = ((0, 0), (8, 8), (15, 1), (1, 15), (0, 15), (15, 0))
KINDS0 = ("const_max", "checker", "col_stripe", "row_stripe", "blocks4", "random")


def _stack(planes):
    return _ro(np.concatenate(planes, axis=0))


@lru_cache(maxsize=None)
def saturated(bd, dx, dy):
    """list 0: the six two-level kinds; list 1: constant 0, constant max, the complement of list 0's plane, random of the extremes; the six fractions per list"""
    mx = (1 << bd) - 1
    p0 = [filler(k, mx, 0, PH, PW, 1) for k in KINDS0]
    p1 = [filler("const_0", mx, 0, PH, PW), filler("const_max", mx, 0, PH, PW), filler("random", mx, 0, PH, PW, 2)] + [mx - p for p in p0]
    items, tags, n = [], [], 0
    for i0, k0 in enumerate(KINDS0):
        for j1, k1 in ((0, "const_0"), (1, "const_max"), (3 + i0, "complement"), (2, "random")):
            for f0 in FRACS6:
                for f1 in FRACS6:
                    same = k1 == "complement" and n % 3 == 0          # a third of the complement items at list 0's position: every difference of the centre is the maximum
                    items.append((10 + n % 4, i0 * PH + 6 + n % 3, 10 + (n if same else n // 4) % 4, j1 * PH + 6 + (n if same else n // 16) % 3) + f0 + f1)
                    tags.append((k0, k1, f0, f1))
                    n += 1
    return Family("saturated", bd, dx, dy, _stack(p0), _stack(p1), items, tags)


def max_cost(dx, dy):
    """the largest SAD of a size on the 10-bit internal scale: every difference 1023 (255 << 2 = 1020 at 8 bits, 511 << 1 = 1022 at 9) on dy / 2 rows"""
    return (dx * dy // 2) * 1023


def raw_for_reduced(target):
    """the raw centre sums s with s - (s >> 2) == target"""
    return [s for s in range(target, 2 * target + 4) if s - (s >> 2) == target]


@lru_cache(maxsize=None)
def threshold(dx, dy):
    """10 bits, fractions 0, both planes flat at 100; list 1 raised on row 0 of the block (an even row; no displaced position with ver = -2 covers it, so position
    (-2, -2) costs 0) so that the reduced centre is dx * dy - 1, dx * dy, dx * dy + 1"""
    n = dx * dy
    p0, p1, items, tags = [], [], [], []
    for k, target in enumerate((n - 1, n, n + 1)):
        s = raw_for_reduced(target)[-1]
        a, b = np.full((PH, PW), 100, np.int64), np.full((PH, PW), 100, np.int64)
        b[8, 12:12 + dx] += s // dx
        b[8, 12:12 + s % dx] += 1
        assert int((b - a).sum()) == s
        p0.append(a); p1.append(b)
        items.append((12, k * PH + 8, 12, k * PH + 8, 0, 0, 0, 0))
        tags.append((target, s))
    return Family("threshold", 10, dx, dy, _stack(p0), _stack(p1), items, tags)


C0 = 100
SX, SY = 12, 8                                # the block of a surface case


def surface_profiles(dx, dy, gl, gr, fl, fr):
    """A[hor + 2], B[ver + 2] of the separable costs: gl / gr = g on the five columns SX - 2 .. SX + 2 / SX + dx - 3 .. SX + dx + 1 (0 between), fl / fr = f on the rows alike"""
    g, f = np.zeros(dx + 4, np.int64), np.zeros(dy + 4, np.int64)
    g[:5], g[dx - 1:], f[:5], f[dy - 1:] = gl, gr, fl, fr
    A = [int(g[2 - h:2 - h + dx].sum()) * (dy // 2) for h in range(-2, 3)]
    B = [int(f[2 - v:2 - v + dy:2].sum()) * dx for v in range(-2, 3)]
    return A, B


def surface_classes(A, B, dx, dy):
    """the classes a separable case falls in (None: the search does not start)"""
    tr = {}
    search([A[h] + B[v] for v in range(5) for h in range(5)], dx, dy, (), tr)
    return trace_classes(tr)


def trace_classes(tr):
    if not tr["searched"]:
        return None
    out = [("win",) + tr["winner"]]
    if tr["branches"] is not None:
        for axis, b in zip("xy", tr["branches"]):
            out.append((axis,) + b + ((("centre" if tr["winner"] == (0, 0) else "off"),) if b == ("p8",) else ()))
    return out


def surface_wanted():
    w = {("win", h, v) for h in range(-2, 3) for v in range(-2, 3)}
    for axis in "xy":
        w |= {(axis, "q", q) for q in range(-7, 8)} | {(axis, "p8", "centre"), (axis, "p8", "off"), (axis, "m8"), (axis, "den0")}
    return w


def _centre_ties(dx, dy):
    """six constructed draws: the centre wins with its left / right (top / bottom) neighbour, or both, exactly as cheap as the reduced centre.  With m = 12 and u = dy / 2:
    A(0) = 4 m u reduces to 3 m u; A(1) = 3 m u + u * e1 and A(-1) = 3 m u + u * e2 (e = 0: a tie, 5: none); the border positions cost more.  Vertically B(0) sums even
    rows and B(+-1) odd rows, so f(SY) = f(SY + dy) = 4 m, f(SY + 1) = 3 m and e on rows SY - 1 / SY + dy - 1 do the same"""
    m, z = 12, [0] * 5
    out = []
    for e1, e2 in ((0, 0), (5, 0), (0, 5)):                      # a zero denominator, -8 (the neighbour before ties), +8 (the neighbour after ties)
        out.append(([30, e1, m, m, 0], [0, m, m, e2, 30], z, z))
        out.append((z, z, [0, e1, 4 * m, 3 * m, 0], [0, 0, e2, 4 * m, 0]))
    return out


def _winners():
    """25 constructed draws, one per position: g and f are 0 on the apron samples the position covers and 50 on the others, so it alone costs nothing"""
    out = []
    for v in range(-2, 3):
        for h in range(-2, 3):
            gl, gr = [0 if j >= 2 - h else 50 for j in range(4)] + [0], [0] + [0 if j < 2 - h else 50 for j in range(4)]
            # rows SY - 2 .. SY + 2 and SY + dy - 3 .. SY + dy + 1 (dy is even): row SY + i is covered when i + v is even and 0 <= i + v <= dy - 2
            fl = [0 if (i + v) % 2 == 0 and i + v >= 0 else 50 for i in range(-2, 3)]
            fr = [0 if (i + v) % 2 == 0 and i + v <= -2 else 50 for i in range(-3, 2)]
            out.append((gl, gr, fl, fr))
    return out


@lru_cache(maxsize=None)
def surface_draws(dx, dy, n_draws=4000):
    """the selected (gl, gr, fl, fr): the constructed ties, then seeded draws (values 0 .. 59; every third draw on a coarse grid of 0, 16, 32, 48, where neighbours tie
    often), one per class not met before"""
    rng = np.random.default_rng(1200 + dx * 32 + dy)
    seen, picked = set(), []
    cands = _centre_ties(dx, dy) + _winners()
    for k in range(n_draws):
        if k % 3 == 2:
            cands.append(tuple((rng.integers(0, 4, 5) * 16).tolist() for _ in range(4)))
        else:
            cands.append(tuple(rng.integers(0, 60, 5).tolist() for _ in range(4)))
    for d in cands:
        cl = surface_classes(*surface_profiles(dx, dy, *d), dx, dy)
        if cl and not set(cl) <= seen:
            seen |= set(cl)
            picked.append(d)
    return picked, seen


@lru_cache(maxsize=None)
def surface(bd, dx, dy):
    """the selected draws as planes: list 0 flat at C0, list 1 = C0 + g + f around the block at (SX, SY); fractions 0"""
    draws, _ = surface_draws(dx, dy)
    p1, items = [], []
    for k, (gl, gr, fl, fr) in enumerate(draws):
        g, f = np.zeros(PW, np.int64), np.zeros(PH, np.int64)
        g[SX - 2:SX + 3], g[SX + dx - 3:SX + dx + 2], f[SY - 2:SY + 3], f[SY + dy - 3:SY + dy + 2] = gl, gr, fl, fr
        p1.append(C0 + g[None, :] + f[:, None])
        items.append((SX, SY, SX, k * PH + SY, 0, 0, 0, 0))
    return Family("surface", bd, dx, dy, np.full((PH, PW), C0), _stack(p1), items, draws)


def textured(bd, h, w, seed):
    yy, xx = np.mgrid[0:h, 0:w]
    rng = np.random.default_rng(seed)
    t = 512 + 300 * np.sin(xx / 3.7) * np.cos(yy / 2.9) + 90 * np.sin((xx - yy) / 2.3) + rng.normal(0, 30, (h, w))
    return _ro(np.clip(t * (1 << bd) / 1024.0, 0, (1 << bd) - 1))


PATHS4 = ((0, 0), (5, 0), (0, 11), (7, 9))    # copy, horizontal only, vertical only, both


def code_path(fx, fy):
    return (1 if fx else 0) + (2 if fy else 0)


@lru_cache(maxsize=None)
def phases(bd, dx, dy):
    """a textured pair and a two-level pair: item k has (fx, fy) = (k % 16, k // 16) in list 0 and the k-th of a permutation of the 256 in list 1; then the 16 pairs of
    code paths on either pair"""
    mx = (1 << bd) - 1
    H, W = 40, 64
    p0 = [textured(bd, H, W, 31), filler("blocks4", mx, 0, H, W)]
    p1 = [np.roll(textured(bd, H, W, 32), (1, -1), (0, 1)), filler("random", mx, 0, H, W, 3)]
    items = []
    for p in (0, 1):
        for k in range(256):
            j = (k * 77 + 5) % 256
            items.append((10 + k % 9, p * H + 6 + k % 7, 12 + k % 11, p * H + 8 + k % 5, k % 16, k // 16, j % 16, j // 16))
        for a in PATHS4:
            for b in PATHS4:
                items.append((13, p * H + 9, 11, p * H + 7) + a + b)
    return Family("phases", bd, dx, dy, _stack(p0), _stack(p1), items)


TIE_PAIRS = (((1, -1), (-1, 1)), ((2, -2), (-2, 2)), ((0, -1), (-1, 0)), ((1, 0), (0, 1)), ((2, -1), (-2, 1)))


@lru_cache(maxsize=None)
def tie_pairs(bd, dx, dy):
    """list 0 flat at C0; list 1 is C0 on the samples that the windows of two positions (hor, ver) cover — columns SX - hor .. SX - hor + dx - 1 of the rows
    SY - ver + 0, 2, .. — and C0 + 120 elsewhere (the centre misses at least four of them: it passes the threshold): exactly these two positions cost 0.  In each pair the first comes first in the raster order and the second first in a
    column-major order.  Fractions 0"""
    p1, items = [], []
    for k, pair in enumerate(TIE_PAIRS):
        a = np.full((PH, PW), C0 + 120, np.int64)
        for h, v in pair:
            a[SY - v:SY - v + dy:2, SX - h:SX - h + dx] = C0
        p1.append(a)
        items.append((SX, SY, SX, k * PH + SY, 0, 0, 0, 0))
    return Family("tie_pairs", bd, dx, dy, np.full((PH, PW), C0), _stack(p1), items, list(TIE_PAIRS))


CELL_W = 40
LAYOUT_COLS = (8, 5)                          # cells per row of the two planes: row pitches 320 and 200


@lru_cache(maxsize=None)
def layout(bd, dx, dy, sentinels=True):
    """64 items, one per pair of residues modulo 8 of the two block columns, each in a cell of its own of either plane: CELL_W columns by dy + 5 rows, the cell rows stacked
    without a gap (the first item's loads start at sample 0 of the plane); one more item whose loads end at the plane's last sample.  A cell holds texture inside the
    reference's footprint of its item and, with sentinels, -32768 / 32767 alternating everywhere else — the rest of the kernel's footprint included"""
    r_lo, r_hi, c_lo, c_hi = kernel_footprint(dx, dy)
    ch = r_hi - r_lo + 1
    mx = (1 << bd) - 1
    rng = np.random.default_rng(7700 + bd * 64 + dx * 2 + dy)
    pos = [[], []]
    fr = []
    for k in range(65):
        f = [(0, 0, 0, 0), (3, 0, 0, 14), (0, 9, 12, 0), (15, 15, 1, 1), (0, 0, 8, 8), (6, 13, 0, 0)][k % 6]
        fr.append(f)
        for l in (0, 1):
            ncol = LAYOUT_COLS[l]
            rows = (64 + ncol - 1) // ncol + 1
            if k < 64:
                want = (k + 2) % 8 if l == 0 else (k // 8 + 2) % 8          # item 0: column 2 of both planes
                cx, cy = k % ncol, k // ncol
                pos[l].append((cx * CELL_W + 2 + (want - 2) % 8, cy * ch + 2))
            else:
                pos[l].append((ncol * CELL_W - 1 - c_hi, rows * ch - 1 - r_hi))
    planes = []
    for l in (0, 1):
        ncol = LAYOUT_COLS[l]
        rows = (64 + ncol - 1) // ncol + 1
        H, W = rows * ch, ncol * CELL_W
        yy, xx = np.mgrid[0:H, 0:W]
        a = np.where((xx + yy) & 1, SENTINELS[1], SENTINELS[0]).astype(np.int64) if sentinels else np.zeros((H, W), np.int64)
        for k, (x, y) in enumerate(pos[l]):
            fx, fy = fr[k][2 * l:2 * l + 2]
            q_lo, q_hi, d_lo, d_hi = reference_footprint(dx, dy, fx, fy)
            a[y + q_lo:y + q_hi + 1, x + d_lo:x + d_hi + 1] = rng.integers(0, mx + 1, (q_hi - q_lo + 1, d_hi - d_lo + 1))
        planes.append(a)
    items = [pos[0][k] + pos[1][k] + fr[k] for k in range(65)]
    return Family("layout", bd, dx, dy, planes[0], planes[1], items)


LIST_NS = (0, 1, 2, 3, 4, 5, 31, 32, 33, 35, 67, 259)


@lru_cache(maxsize=None)
def lists(bd, dx, dy):
    """259 items on a textured pair (list 1 = list 0 moved by (1, -1) with other noise: the search moves); the lists of LIST_NS are its first n items"""
    H, W = 96, 160
    rng = np.random.default_rng(900 + bd * 64 + dx * 2 + dy)
    a = textured(bd, H, W, 41)
    b = np.clip(np.roll(a, (-1, 1), (0, 1)).astype(np.int64) + rng.integers(-6, 7, (H, W)) * (1 << bd) // 256, 0, (1 << bd) - 1)
    items = [(int(rng.integers(2, W - 24)), int(rng.integers(2, H - dy - 3)), int(rng.integers(2, W - 24)), int(rng.integers(2, H - dy - 3))) + tuple(int(v) for v in rng.integers(0, 16, 4)) for _ in range(259)]
    for k in range(0, 259, 3):                # a third of the items at one position in both planes: the winner is near the true displacement
        items[k] = items[k][:2] + items[k][:2] + items[k][4:]
    return Family("lists", bd, dx, dy, a, b, items)


def list_selections(n_all=259):
    """(name, indices into the 259 items): the first n, the whole list shuffled, 67 identical items"""
    out = [("first %d" % n, np.arange(n)) for n in LIST_NS]
    out.append(("shuffled", np.random.default_rng(5).permutation(n_all)))
    out.append(("identical", np.full(67, 3)))
    return out


def families(bd, dx, dy):
    out = [saturated(bd, dx, dy), surface(bd, dx, dy), phases(bd, dx, dy), layout(bd, dx, dy), lists(bd, dx, dy)]
    if bd == 10:
        out.insert(1, threshold(dx, dy))
    out.append(tie_pairs(bd, dx, dy))
    return out


# ---- SAD-X5 ------------------------------------------------------------------------------------------------------------------------
# (min, max, width in bits of max - min): 12 bits are the widest operands at which the reference's two rows agree at DMVR's heights — unsigned, and signed for the kernel's
# bias; 15 bits: the scalar row alone
X5_SETS = ((0, 255, 8), (0, 1023, 10), (0, 4095, 12), (-2048, 2047, 12), (0, 32767, 15))
X5_NS = (1, 3, 13, 51, 52, 205)
X5_H, X5_W = 136, 40                          # planes: a 16 x 128 block, k to 4, a few positions


@lru_cache(maxsize=None)
def x5_planes():
    """(org, cur): per operand width the six two-level kinds stacked; cur holds constants, a random plane and the complements"""
    org, cur = [], []
    for lo, mx, _ in X5_SETS:
        o = [filler(k, mx, lo, X5_H, X5_W, 11) for k in KINDS0]
        org += o
        cur += [filler("const_0", mx, lo, X5_H, X5_W), filler("const_max", mx, lo, X5_H, X5_W), filler("random", mx, lo, X5_H, X5_W, 12)] + [lo + mx - p for p in o[1:4]]
    return _stack(org), _stack(cur)


def x5_rows_agree(w, h, ss, bits):
    """whether the reference's x86 row computes what its scalar row does (module docstring)"""
    return (h >> ss) * ((1 << bits) - 1) <= 32767 and not (w == 16 and (ss == 0 or h < 8))


def x5_cases():
    """(w, h, sub_shift, calc_centre, n, items) with items = [(ox, oy, cx, cy, bits)] in the stacked planes: positions with odd and even cur columns in planes of one
    operand width (bits: the wider of the two); item 0 has cur - 4 at sample 0 of the plane, item 1 (n > 1) the last sample of its org + 4 block at the plane's last sample"""
    nk = len(KINDS0)
    total = len(X5_SETS) * nk * X5_H
    for w in (8, 16):
        for h in (4, 8, 16, 32, 128):
            for ss in (0, 1):
                for cc in (0, 1):
                    for n in X5_NS:
                        rng = np.random.default_rng(w * 1000 + h * 8 + ss * 4 + cc * 2 + n * 131)
                        items = []
                        for k in range(n):
                            b, ko, kc = int(rng.integers(0, len(X5_SETS))), int(rng.integers(0, nk)), int(rng.integers(0, nk))
                            items.append((int(rng.integers(0, X5_W - w - 4 + 1)), (b * nk + ko) * X5_H + int(rng.integers(0, X5_H - h + 1)),
                                          4 + int(rng.integers(0, X5_W - w - 4 + 1)), (b * nk + kc) * X5_H + int(rng.integers(0, X5_H - h + 1)), X5_SETS[b][2]))
                        items[0] = (items[0][0], items[0][1], 4, 0, items[0][4])
                        if n > 1:
                            cx = items[1][2] | 1
                            items[1] = (X5_W - w - 4, total - h, cx if cx + w <= X5_W else cx - 2, items[1][3], X5_SETS[-1][2])
                        yield w, h, ss, cc, n, items


def x5_team_lanes(w, h, ss):
    """lanes per team of launchSadSse (restated for the guard): the largest power of two <= (w / 8) * (h >> ss), at most 64"""
    c = (w // 8) * (h >> ss)
    p = 1
    while p * 2 <= c:
        p *= 2
    return min(p, 64)


# ---- SAD surface -------------------------------------------------------------------------------------------------------------------
def surface_launch(w, h, ss, rx, ry, n_blocks):
    """the host's choice in vvhip_sad_surface, restated for the guards: (kdy, splits, LDS bytes)"""
    nx, ny = 2 * rx + 1, 2 * ry + 1
    kdy, best = 1, 1 << 30
    for k in (1, 2, 4, 8):
        cost = ((nx * ((ny + k - 1) // k) + 63) // 64) * (k + 1)
        if cost < best:
            best, kdy = cost, k
    nyg = (ny + kdy - 1) // kdy
    splits = max(1, min(nyg, (1024 + n_blocks - 1) // n_blocks))
    gps = (nyg + splits - 1) // splits
    splits = (nyg + gps - 1) // gps
    win_w, win_rows = w + 2 * rx, h + gps * kdy
    pitch = ((win_w + 2) // 2) | 1
    copy_b = ((pitch * win_rows + 31) & ~31) + 16
    return kdy, splits, (2 * copy_b + ((h >> ss) * w) // 2 + 8) * 4


SURF_H, SURF_W = 200, 272                     # a 128x128 block with 16 columns / 32 rows of range on either side, three positions
SURF_PLANES = ("uniform10", "two_level8", "two_level10", "full_range")
SURF_RANGES = ((0, 0), (0, 5), (7, 0), (16, 3))
SURF_SIZES = ((2, 2), (4, 4), (8, 16), (64, 64), (128, 128))
SURF_KDY = ((8, 8, 8, 8), (8, 8, 10, 5), (8, 16, 3, 32))          # (w, h, rx, ry) whose launches take KDY 2, 4 and 8 (the ranges above all take 1)
SURF_TOO_BIG = (128, 128, 0, 64, 16)          # (w, h, ss, rx, ry): beyond 160 KiB of LDS with and without the split


@lru_cache(maxsize=None)
def surf_planes(kind):
    """(org, ref)"""
    if kind == "uniform10":
        rng = np.random.default_rng(102)
        return _ro(rng.integers(0, 1024, (SURF_H, SURF_W))), _ro(rng.integers(0, 1024, (SURF_H, SURF_W)))
    if kind == "full_range":
        c = filler("checker", 32767, -32768, SURF_H, SURF_W)
        return c, _ro(-1 - c.astype(np.int64))
    mx = 255 if kind == "two_level8" else 1023
    return filler("blocks4", mx, 0, SURF_H, SURF_W), filler("random", mx, 0, SURF_H, SURF_W, 21)


def surf_geometries():
    """(w, h, ss, rx, ry): every size x range x sub_shift, then the KDY geometries with sub_shift 0 and 1"""
    out = [(w, h, ss, rx, ry) for (w, h) in SURF_SIZES for (rx, ry) in SURF_RANGES for ss in (0, 1)]
    out += [(w, h, ss, rx, ry) for (w, h, rx, ry) in SURF_KDY for ss in (0, 1)]
    return out


def surf_blocks(w, h, rx, ry):
    """three block positions (x, y), the same in both planes: the window of the first starts at sample 0, that of the last ends at the plane's last sample, one is odd"""
    return [(rx, ry), (SURF_W - w - rx, SURF_H - h - ry), (rx + 1 + (SURF_W - w - 2 * rx - 1) // 3 | 1, ry + (SURF_H - h - 2 * ry) // 2)]


def surf_expected(lib, kind, w, h, ss, rx, ry):
    """(3, 2 ry + 1, 2 rx + 1) from lib.dist("SAD", ...)"""
    org, ref = surf_planes(kind)
    out = np.zeros((3, 2 * ry + 1, 2 * rx + 1), np.int64)
    for b, (x, y) in enumerate(surf_blocks(w, h, rx, ry)):
        for dy in range(-ry, ry + 1):
            for dx in range(-rx, rx + 1):
                out[b, dy + ry, dx + rx] = lib.dist("SAD", (org, y, x), (ref, y + dy, x + dx), w, h, 10, ss)
    return out
