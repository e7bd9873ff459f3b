"""Deterministic extreme inputs of the distortion list entries of vvenc_amd/csrc/dist.hip — vvhip_dist_batch, vvhip_dist_multi, vvhip_dist_multi_func, vvhip_dist_multi_func_tiled,
vvhip_plane_tile8, vvhip_plane_shift1, vvhip_planes_derive, vvhip_sad_mask_batch, vvhip_fix_weighted_sse_batch — shared by the CPU tier (tests/test_oracle_dist_extremes.py: oracle
against the compiled reference, the int64 models, the guards, the sensitivity test) and the GPU tier (tests/test_gpu_dist_extremes.py: every entry against the oracle, tolerance 0).

The parity suite runs these entries on uniform random 10-bit planes, whose sums never come near the ranges the packed arithmetic is sized for.  The families here:
  A  Hadamard operand range.  One sign picture (a_signs: 448 x 128, every sample +1 or -1) per domain, mapped to two sample levels so that every difference is +-D:
       M   256 8x8 tiles: the 64 two-dimensional Walsh functions with either sign (each drives ONE coefficient and the partial sums of every butterfly stage on the way to
           it to 64 D; neighbours W, -W form a 16x8 Walsh function), then 128 random pictures of the two levels
       R1  64 cells of 16x16: the Walsh functions on 2x2-replicated samples (the 16x16_fast tile averages them back exactly)
       R2  64 cells of 16x16 that differ inside a 2x2 cell: -DC, random two-level cells and Walsh functions with one sample of every 2x2 cell flipped (every remainder of
           the rounded average, negative sums in the signed domain)
       C   eight cells of 32x32: constant of either sign, checkerboard, columns, rows, 2x2, 4x4 and 8x8 blocks (Walsh functions of EVERY tile kind of the ladder)
     A plane holds the picture twice, at column 0 and at column 137: a candidate at an odd x meets the same patterns as one at an even x.  Domains: samples of 10 and 8 bits
     with VVHIP_DIST_FLAG_SAMPLES (org in {0, max}, cur the complement: D = max, the all-packed form sized by 32 * 1023 < 32768); the bi-prediction pattern without the flag
     (org in {2^(bd+1) - 2, -(2^bd - 1)}, cur in {0, max}: D = 2^(bd+1) - 2, the form with four packed stages sized by 16 * 2047 < 32768); 12-bit samples (the 32-bit merged
     kernel); full int16 (-32768 / 32767: D = 65535) through vvhip_dist_batch only
  B  SAD / SSE accumulators and row walks.  Constant largest differences of either sign, checkers, stripes and a region a few levels below the extreme (so that a wrong row
     or segment shows): |d| = 65535 for SAD up to 128x128, 46340 for SSE (below), 4095 and 1023 for the flagged SSE; widths 2, 4, 6, 12 (the narrow vector forms) and
     24, 40, 72, 96, 120 (lanes per row no power of two), as batches and as merged jobs; sub_shift 0 and 1, one evaluated row (h = 2 with sub_shift 1), h = 1
  C  list mechanics on a 10-bit texture: n = 1, 2, 3, 63, 64, 65, 127, 129, 257; neighbouring items that share org_off, that do not, and a mix; job tables of 9, 16 and 17
     mergeable jobs (a launch takes eight), an interleaved table with unmergeable and empty jobs, jobs of 8, 9, 15 and 17 workgroups (the XCD remap's remainder); every table
     forward, reversed and shuffled
  D  derived copies: planes of 63 and 64 rows with strides congruent to 0, 1, 4 and 7 mod 8 (two of them odd: the shifted copy is then ignored); 8x8 SAD, SSE and flagged SSE
     at every phase (x & 7, y & 7) of the candidate with every original phase of {0, 1, 7} x {0, 1, 7}, a wave of 64 tile-aligned candidates with and without one unaligned
     candidate, and the four corners of the padded plane (last tile column and row included)
  E  masked SAD with |d| = 65535 against masks 32767, -32768 and mixed signs, step_x 1, -1, 2, three mask_stride2, sub_shift 0 and 1, sizes 1x1, 3x5, 8x8, 128x16, 128x128;
     fixed-weight SSE with weights 0, 1, 2^16 - 1, 2^16, 2^20 and per difference level the largest weight whose term still fits `int`, widths 1, 2, 128

Inputs the reference does not define are kept out by construction; the models return the int64 value of each such intermediate so that the CPU tier can assert it in range:
  RdCost.cpp:668-675      xGetSSE (and its width twins to :1000) squares an Intermediate_Int: |d| <= 46340.  No SSE item is built on the 65535 planes
  RdCost.cpp:1948-1952    getWeightedMSE: iTemp * iTemp is an `int` (|d| <= 46340) and the weighted, shifted term is cast to Intermediate_Int: the weights of a level stop at
                          wsse_max_weight(d), the largest w with (w d^2 + 2^15) >> 16 <= 2^31 - 1
  RdCost.cpp:318-334      the scalar SAD functions accumulate in Distortion (64 bits); the x86 rows add 32-bit lanes.  The largest SAD here is 128 * 128 * 65535 = 1.07e9, inside `int`
  RdCost.cpp:2083         abs( org - cur ) * *mask is an `int` product: 65535 * 32767 and 65535 * -32768 are inside `int` by 33 000; the sum is a Distortion, where a negative
                          term wraps modulo 2^64 (defined: unsigned arithmetic), as it does in the oracle and on the device
  RdCost.cpp:1467, :1606, :1682, :1763   `int sad` and (int)( sad / sqrt( w h ) * 2 ) of the rectangular tiles: the largest tile sum here is 128 * 65535 * 8 < 2^31
  RdCost.cpp:1782-1789    (found while building this tier) xGetHAD2SADs takes its SAD over height >> 2 rows of 4 width samples in steps of 16: with a height below 4 the SAD
                          is 0 (and so is the minimum), with a width of 2 it reads beyond the block.  HAD_2SAD is built on the 13 shapes of A_SHAPES whose sides are
                          multiples of 4, not on 2x2, 2x8 and 8x2 (HAD and HAD_fast are)
  RdCost.cpp:177-181, :214               (found while building this tier) the table of width-specialised functions is indexed by Log2( width ): a width that is no power of two
                          lands on the function of the power of two below it, which reads that many columns only (xGetSAD4 .. xGetSAD64, xGetSSE4 .. xGetSSE64 are unrolled).
                          The encoder has no such blocks.  The CPU tier compares those widths with the general functions xGetSAD / xGetSSE (the table's first entry of each
                          block, width taken from the DistParam), which is what the oracle and the device compute
  x86/RdCostX86.h:655-659, :800-804      the x86 Hadamard rows refuse bit depths above 10; the x86 SAD / SSE rows subtract in 16 bits.  Both are classes the CPU tier leaves
                          the x86 row out for, by name and with a count

The int64 models below restate xGetSAD, xGetSSE, the tile ladder of xGetHADs (RdCost.cpp:1818-1938) with its tiles, xGetHAD2SADs, xGetSADwMask, fixWeightedSSE_Core, the packed
8x8 / 16x16_fast tile of dist.hip (to mutate the stage at which it stops wrapping), and the tiled and shifted plane copies.  They serve the guards and the mutations of the
sensitivity test only: expected values of both tiers come from the oracle, never from them.  Numpy only: no GPU, no oracle, no reference.
"""
import math
from functools import lru_cache

import numpy as np

INT_MAX = 2 ** 31 - 1
U64 = (1 << 64) - 1
FLAG_SAMPLES = 1                              # VVHIP_DIST_FLAG_SAMPLES
SENT16 = -21846                               # 0xAAAA

MUTATIONS = ("narrow_late", "narrow_early", "wide_late", "wide_early", "sse_acc32", "dc_not_quartered", "no_subshift", "had2sad_no_min", "rect_int_shift", "avg_unsigned",
             "funnel_off", "shift_at_k", "pair_reuse")


def _ro(v):
    return np.ascontiguousarray(v, np.int16)


def wrap16(v):
    return ((v + 32768) & 0xffff) - 32768


def wrap15(v):
    return ((v + 16384) & 0x7fff) - 16384


def is_pow2(v):
    return v & (v - 1) == 0


class Job:
    """one list: func, width, height, sub_shift and items [(ox, oy, cx, cy)] in the coordinates of a domain's numpy planes"""

    def __init__(self, func, w, h, ss, items, tag=""):
        self.func, self.w, self.h, self.ss, self.items, self.tag = func, w, h, ss, [tuple(int(v) for v in it) for it in items], tag

    @property
    def n(self):
        return len(self.items)

    def key(self, k):
        return (self.func, self.w, self.h, self.ss) + self.items[k]


class Domain:
    def __init__(self, name, bd, flags, org, cur, d_max, any_pitch=False):
        self.name, self.bd, self.flags, self.org, self.cur, self.d_max = name, bd, flags, _ro(org), _ro(cur), d_max
        assert any_pitch or (self.org.shape[1] % 8 == 0 and self.cur.shape[1] % 8 == 0)      # Plane.from_numpy keeps a pitch that is a multiple of 8

    def blocks(self, job, k):
        ox, oy, cx, cy = job.items[k]
        o, c = self.org[oy:oy + job.h, ox:ox + job.w], self.cur[cy:cy + job.h, cx:cx + job.w]
        assert o.shape == c.shape == (job.h, job.w), (self.name, job.func, job.w, job.h, job.items[k])
        return o.astype(np.int64), c.astype(np.int64)


def expected(lib, dom, job, k):
    """the value of item k from the oracle or from a row of the reference (HAD_2SAD: compact copies, RdCost.cpp:1778)"""
    ox, oy, cx, cy = job.items[k]
    if job.func == "HAD_2SAD":
        return lib.dist("HAD_2SAD", np.ascontiguousarray(dom.org[oy:oy + job.h, ox:ox + job.w]), np.ascontiguousarray(dom.cur[cy:cy + job.h, cx:cx + job.w]), job.w, job.h)
    return lib.dist(job.func, (dom.org, oy, ox), (dom.cur, cy, cx), job.w, job.h, dom.bd, job.ss)


# ---- the int64 models --------------------------------------------------------------------------------------------------------------------------------------------
def hadamard(n):
    h = np.ones((1, 1), np.int64)
    while h.shape[0] < n:
        h = np.block([[h, h], [h, -h]])
    return h


@lru_cache(maxsize=None)
def walsh8():
    H = hadamard(8)
    return [np.outer(H[u], H[v]) for u in range(8) for v in range(8)]


def sad_model(o, c, ss=0, mut=()):
    s = int(np.abs(o[::1 << ss] - c[::1 << ss]).sum())
    return s if "no_subshift" in mut else s << ss


def sse_model(o, c, mut=()):
    d = o - c
    s = int((d * d).sum())
    return s & 0xffffffff if "sse_acc32" in mut else s


def _tiles(d, tw, th):
    """(h, w) -> (tiles, th, tw)"""
    h, w = d.shape
    return d.reshape(h // th, th, w // tw, tw).transpose(0, 2, 1, 3).reshape(-1, th, tw)


def _tile_sums(t, mut=()):
    """sum of |H D H'| per tile with |DC| counted a quarter (the tail of every xCalcHADs*)"""
    th, tw = t.shape[1:]
    c = np.einsum("ij,tjk,lk->til", hadamard(th), t, hadamard(tw))
    s = np.abs(c).sum(axis=(1, 2))
    dc = np.abs(c[:, 0, 0])
    return s - dc + (dc if "dc_not_quartered" in mut else dc >> 2)


def pk_tile_sums(t, stages, early=False):
    """the 8x8 tile of hadTilePkBody: dword 4 r + q holds the differences (r, 2 q), (r, 2 q + 1); the packed subtraction and the first `stages` butterfly stages over the
    dword index wrap at 16 bits (5: the all-packed form; 4: the general form), the rest is exact; stage six pairs the two halves of a dword.  early: the last packed stage
    wraps at 15 bits, as if the wrap of the stage behind it came one stage sooner"""
    v = wrap16(t.reshape(-1, 32, 2))
    n, ln, st = v.shape[0], 1, 0
    while ln < 32:
        g = v.reshape(n, 32 // (2 * ln), 2, ln, 2)
        a, b = g[:, :, 0], g[:, :, 1]
        v = np.stack([a + b, a - b], 2).reshape(n, 32, 2)
        st += 1
        if st <= stages:
            v = wrap15(v) if (early and st == stages) else wrap16(v)
        ln *= 2
    lo, hi = v[:, :, 0], v[:, :, 1]
    six = np.concatenate([lo + hi, lo - hi], 1)
    if stages >= 6:
        six = wrap16(six)
    dc = np.abs(six[:, 0])
    return np.abs(six).sum(axis=1) - dc + (dc >> 2)


def avg2x2(a, mut=()):
    s = a[0::2, 0::2] + a[1::2, 0::2] + a[0::2, 1::2] + a[1::2, 1::2] + 2
    return ((s & 0xffff) >> 2) if "avg_unsigned" in mut else s >> 2


def ladder(w, h, fast):
    """(tile width, tile height, kind) of xGetHADs<fast>, RdCost.cpp:1836-1935; kind: rect, fast16, sq"""
    if w > h and h % 8 == 0 and w % 16 == 0:
        return 16, 8, "rect"
    if w < h and w % 8 == 0 and h % 16 == 0:
        return 8, 16, "rect"
    if w > h and h % 4 == 0 and w % 8 == 0:
        return 8, 4, "rect"
    if w < h and w % 4 == 0 and h % 8 == 0:
        return 4, 8, "rect"
    if fast and h % 32 == 0 and w % 32 == 0 and h == w:
        return 16, 16, "fast16"
    for t in (8, 4, 2):
        if h % t == 0 and w % t == 0:
            return t, t, "sq"
    raise ValueError((w, h))


PK_STAGES = {"narrow": 5, "wide": 4}


def had_model(o, c, fast=False, mut=(), form=None):
    """xGetHADs<fast>; form (narrow / wide): the 8x8 and 16x16_fast tiles through the packed model, with the mutations <form>_late (one more wrapping stage) and
    <form>_early"""
    h, w = o.shape
    tw, th, kind = ladder(w, h, fast)
    if kind == "fast16":
        t = _tiles(avg2x2(o, mut) - avg2x2(c, mut), 8, 8)
    else:
        t = _tiles(o - c, tw, th)
    if form and t.shape[1:] == (8, 8):
        s = pk_tile_sums(t, PK_STAGES[form] + (1 if form + "_late" in mut else 0), form + "_early" in mut)
    else:
        s = _tile_sums(t, mut)
    if kind == "fast16":
        return int((((s + 2) >> 2) << 2).sum())
    if kind == "rect":
        if "rect_int_shift" in mut:
            return int(((2 * s) >> ((tw * th).bit_length() // 2)).sum())
        return sum(int(float(int(v)) / math.sqrt(float(tw * th)) * 2) for v in s.tolist())
    return int((((s + 2) >> 2) if tw == 8 else ((s + 1) >> 1) if tw == 4 else s).sum())


def dist_model(func, o, c, ss=0, mut=(), form=None):
    if func == "SAD":
        return sad_model(o, c, ss, mut)
    if func == "SSE":
        return sse_model(o, c, mut)
    if func == "HAD_2SAD":
        hv = had_model(o, c, False, mut)
        return hv if "had2sad_no_min" in mut else min(hv, 2 * sad_model(o, c))
    return had_model(o, c, func == "HAD_fast", mut, form)


def tile_max(o, c, fast):
    """the largest tile sum of a Hadamard item before its normalisation (an `int` in the reference)"""
    tw, th, kind = ladder(o.shape[1], o.shape[0], fast)
    t = _tiles(avg2x2(o) - avg2x2(c), 8, 8) if kind == "fast16" else _tiles(o - c, tw, th)
    return int(_tile_sums(t).max())


def list_model(dom, job, mut=()):
    """the values of a list from the models.  Mutations of the list's addressing: funnel_off — an unaligned candidate is read one sample further; shift_at_k — a candidate
    at an odd x is read from the shifted copy at k instead of k - 1 (one sample further); pair_reuse — the second item of a pair takes the first's original block"""
    out = []
    for k in range(job.n):
        ox, oy, cx, cy = job.items[k]
        if "funnel_off" in mut and cx & 7:
            cx += 1
        if "shift_at_k" in mut and cx & 1:
            cx += 1
        if "pair_reuse" in mut and k & 1:
            ox, oy = job.items[k - 1][:2]
        o, c = dom.org[oy:oy + job.h, ox:ox + job.w].astype(np.int64), dom.cur[cy:cy + job.h, cx:cx + job.w].astype(np.int64)
        out.append(dist_model(job.func, o, c, job.ss, mut))
    return out


def mask_sad_model(o, c, mask, my, mx, step_x, ms2, ss):
    """xGetSADwMask on the int64 blocks o, c and the 2-D mask (row pitch = its width) -> (value modulo 2^64, the largest |product|, the smallest lane-free partial sum)"""
    h, w = o.shape
    flat, pitch, step = mask.reshape(-1).astype(np.int64), mask.shape[1], 1 << ss
    p, total, big, low = my * pitch + mx, 0, 0, 0
    for y in range(0, h, step):
        idx = p + step_x * np.arange(w)
        assert idx.min() >= 0 and idx.max() < flat.size
        prod = np.abs(o[y] - c[y]) * flat[idx]
        total += int(prod.sum())
        big, low = max(big, int(np.abs(prod).max())), min(low, total)
        p += w * step_x + pitch * step + ms2
    return (total << ss) & U64, big, low


def wsse_max_weight(d):
    """the largest uint32 weight whose term (w d^2 + 2^15) >> 16 fits `int`"""
    return (1 << 32) - 1 if d == 0 else min((1 << 32) - 1, ((1 << 47) - 32768 - 1) // (d * d))


def wsse_model(o, c, weight):
    """fixWeightedSSE_Core -> (value, the largest term, the largest squared difference)"""
    d = o - c
    t = (weight * d * d + 32768) >> 16
    return int(t.sum()), int(t.max()), int((d * d).max())


def tile8_model(storage):
    """vvhip_plane_tile8 of a (rows, stride) plane -> the tiled samples without the two tiles of slack: tile (ty, tx) holds rows 8 ty .. 8 ty + 7 of columns 8 tx .. 8 tx + 7,
    zero beyond the plane"""
    rows, stride = storage.shape
    R, T = (rows + 7) // 8, (stride + 7) // 8
    p = np.zeros((R * 8, T * 8), np.int16)
    p[:rows, :stride] = storage
    return p.reshape(R, 8, T, 8).transpose(0, 2, 1, 3).reshape(-1)


def tiled8_elems(stride, rows):
    return ((rows + 7) // 8) * ((stride + 7) // 8) * 64 + 128


def shift1_model(storage):
    f = storage.reshape(-1)
    return np.concatenate([f[1:], np.zeros(1, np.int16)])


def lanes_per_row(w):
    """(samples per lane, lanes per row) of launchSadSse"""
    ch = 8 if w % 8 == 0 else 4 if w % 4 == 0 else 2
    return ch, w // ch


def _pow2floor(v):
    p = 1
    while p * 2 <= v:
        p *= 2
    return p


def blocks_model(func, w, h, ss, n, tiled=False):
    """workgroups of a mergeable job in distMultiFunc (dist.hip): SAD / SSE two candidates per lane team and 256 lanes, Hadamard one tile per lane and 64 lanes"""
    if func in ("SAD", "SSE"):
        if tiled and w == 8 and h == 8 and (ss == 0 or func == "SSE"):
            return (n + 255) // 256
        rows = h if func == "SSE" else h >> ss
        lpc = min(64, _pow2floor(w // 8 * rows))
        return ((n + 1) // 2 * lpc + 255) // 256
    px = 16 if (func == "HAD_fast" and w % 32 == 0) else 8
    tiles = (w // px) * (h // px)
    lpc = min(64, _pow2floor(tiles))
    if tiles % lpc:
        lpc = 1
    return (n * lpc + 63) // 64


def mergeable(func, w, h, ss, n):
    if n <= 0 or w < 8:
        return False
    if func in ("SAD", "SSE"):
        return w % 8 == 0
    return func in ("HAD", "HAD_fast") and w == h and w % 8 == 0


def kernel_form(route, func, w, h, ss, bd, flags, tiled=False):
    """the kernel form an item is computed by, restated from the host code of dist.hip (the coverage assertion of the GPU tier counts items per form and shape)"""
    merged = route != "batch" and mergeable(func, w, h, ss, 1)
    if func in ("SAD", "SSE"):
        if merged:
            pk = func == "SSE" and (flags & FLAG_SAMPLES) and bd <= 12
            if tiled and bd <= 10 and w == 8 and h == 8 and (ss == 0 or func == "SSE"):
                return "tiled8-" + ("sse-pk" if pk else func.lower())
            return "merged-" + ("sse-pk" if pk else func.lower()) + ("" if is_pow2(w // 8) else "-div")
        ch, lpr = lanes_per_row(w)
        return "%s<%d>%s" % (func.lower(), ch, "" if is_pow2(lpr) else "-div")
    if func == "HAD_2SAD":
        return "had2sad"
    tw, th, kind = ladder(w, h, func == "HAD_fast")
    if merged:
        t = "fast16" if kind == "fast16" else "8x8"
        return "merged-%s-%s" % (t, "32bit" if bd > 10 else "narrow" if flags & FLAG_SAMPLES else "wide")
    return "had-%s" % ("fast16" if kind == "fast16" else "%dx%d" % (tw, th))


# ---- family A ----------------------------------------------------------------------------------------------------------------------------------------------------
BASE_W, BASE_H = 128, 448
M_Y, R1_Y, R2_Y, C_Y = 0, 128, 256, 384
SHIFT_X = 137                                 # the second copy of the picture: a candidate at SHIFT_X + x (x even) is at an odd sample address
A_W = 272


@lru_cache(maxsize=None)
def a_signs():
    rng = np.random.default_rng(4100)
    S = np.ones((BASE_H, BASE_W), np.int64)
    W = walsh8()
    for t in range(256):
        ty, tx = divmod(t, 16)
        S[ty * 8:ty * 8 + 8, tx * 8:tx * 8 + 8] = W[t // 2] * (1 - 2 * (t % 2)) if t < 128 else rng.choice([-1, 1], (8, 8))
    two = np.ones((2, 2), np.int64)
    for k in range(64):
        y, x = R1_Y + 16 * (k // 8), 16 * (k % 8)
        S[y:y + 16, x:x + 16] = np.kron(W[k] * (1 - 2 * (k % 2)), two)
        y += 128
        if k == 0:
            cell = -np.ones((16, 16), np.int64)
        elif k < 32:
            cell = rng.choice([-1, 1], (16, 16))
        else:
            cell = np.kron(W[(k * 5) % 64], two)
            cell[(k % 2)::2, ((k // 2) % 2)::2] *= -1
        S[y:y + 16, x:x + 16] = cell
    yy, xx = np.mgrid[0:32, 0:32]
    cells = (xx * 0, xx * 0 + 1, (xx + yy) & 1, xx & 1, yy & 1, ((xx >> 1) + (yy >> 1)) & 1, ((xx >> 2) + (yy >> 2)) & 1, ((xx >> 3) + (yy >> 3)) & 1)
    for k, cmap in enumerate(cells):
        y, x = C_Y + 32 * (k // 4), 32 * (k % 4)
        S[y:y + 32, x:x + 32] = 1 - 2 * cmap
    S.setflags(write=False)
    return S


def _a_layout(base):
    p = np.zeros((BASE_H, A_W), np.int64)
    p[:, :BASE_W] = base
    p[:, BASE_W:SHIFT_X] = base[:, :SHIFT_X - BASE_W]
    p[:, SHIFT_X:SHIFT_X + BASE_W] = base
    p[:, SHIFT_X + BASE_W:] = base[:, :A_W - SHIFT_X - BASE_W]
    return p


A_DOMAINS = ("s10", "s8", "b10", "b8", "s12", "i16")
A_MULTI_DOMAINS = A_DOMAINS[:5]


@lru_cache(maxsize=None)
def a_domain(name):
    S = a_signs() > 0
    if name[0] == "s":
        bd = int(name[1:])
        mx = (1 << bd) - 1
        org = np.where(S, mx, 0)
        return Domain(name, bd, FLAG_SAMPLES, _a_layout(org), _a_layout(mx - org), mx)
    if name[0] == "b":
        bd = int(name[1:])
        mx = (1 << bd) - 1
        return Domain(name, bd, 0, _a_layout(np.where(S, 2 * mx, -mx)), _a_layout(np.where(S, 0, mx)), 2 * mx)
    return Domain(name, 16, 0, _a_layout(np.where(S, 32767, -32768)), _a_layout(np.where(S, -32768, 32767)), 65535)


def _grid(w, h, y0, rows):
    return [(x, y) for y in range(y0, y0 + rows - h + 1, h) for x in range(0, BASE_W - w + 1, w)]


@lru_cache(maxsize=None)
def a_multi_jobs():
    """squares 8 .. 128 x HAD, HAD_fast: every tile of M (8), every cell of M and R1 (16), of all regions (32 .. 128), with the candidate at an even and at an odd x;
    for 8 and 16 also both blocks at an odd x"""
    jobs = []
    for func in ("HAD", "HAD_fast"):
        for S in (8, 16, 32, 64, 128):
            pos = _grid(S, S, M_Y, 128)
            if S >= 16:
                pos += _grid(S, S, R1_Y, 128)
            if S >= 32:
                pos += _grid(S, S, R2_Y, 128) + _grid(S, S, C_Y, 64)
            jobs.append(Job(func, S, S, 0, [(x, y, x, y) for x, y in pos], "even"))
            jobs.append(Job(func, S, S, 0, [(x, y, SHIFT_X + x, y) for x, y in pos], "odd"))
            if S <= 16:
                jobs.append(Job(func, S, S, 0, [(SHIFT_X + x, y, SHIFT_X + x, y) for x, y in pos[::4]], "odd-odd"))
    return jobs


A_SHAPES = ((16, 8), (128, 64), (8, 16), (64, 128), (8, 4), (16, 4), (4, 8), (4, 16), (32, 32), (128, 128), (8, 8), (16, 16), (4, 4), (2, 2), (2, 8), (8, 2))
A_FUNCS = ("HAD", "HAD_fast", "HAD_2SAD")


def had2sad_defined(w, h):
    """xGetHAD2SADs walks height >> 2 rows of 4 width samples in steps of 16 (RdCost.cpp:1782-1789)"""
    return w % 4 == 0 and h % 4 == 0


@lru_cache(maxsize=None)
def a_batch_jobs():
    """one shape per tile kind of the ladder and its largest multiple: up to 40 positions on the shape's own grid over the four regions, the cells of C, eight at an odd x"""
    jobs = []
    for (w, h) in A_SHAPES:
        pos = _grid(w, h, 0, BASE_H)
        pos = pos[::max(1, len(pos) // 40)][:40]
        if w <= 32 and h <= 32:
            pos += [(32 * (k % 4), C_Y + 32 * (k // 4)) for k in range(8)]
        items = [(x, y, x, y) for x, y in pos] + [(x, y, SHIFT_X + x, y) for x, y in pos[::max(1, len(pos) // 8)]]
        for func in A_FUNCS:
            if func != "HAD_2SAD" or had2sad_defined(w, h):
                jobs.append(Job(func, w, h, 0, items))
    return jobs


# ---- family B ----------------------------------------------------------------------------------------------------------------------------------------------------
B_W, B_RH = 136, 132
B_KINDS = ("hi_lo", "lo_hi", "checker", "vstripe", "hstripe", "near")
B_DOMAINS = ("d65535", "d46340", "p12", "p10")
B_LEVELS = {"d65535": (32767, -32768, 16, 0), "d46340": (23170, -23170, 16, 0), "p12": (4095, 0, 12, FLAG_SAMPLES), "p10": (1023, 0, 10, FLAG_SAMPLES)}


@lru_cache(maxsize=None)
def b_domain(name):
    hi, lo, bd, flags = B_LEVELS[name]
    rng = np.random.default_rng(4200 + bd)
    yy, xx = np.mgrid[0:B_RH, 0:B_W]
    orgs, curs = [], []
    for k in B_KINDS:
        if k == "hi_lo":
            o, c = xx * 0 + hi, xx * 0 + lo
        elif k == "lo_hi":
            o, c = xx * 0 + lo, xx * 0 + hi
        elif k == "near":
            o, c = hi - rng.integers(0, 4, xx.shape), lo + rng.integers(0, 4, xx.shape)
        else:
            m = {"checker": (xx + yy) & 1, "vstripe": xx & 1, "hstripe": yy & 1}[k] == 1
            o, c = np.where(m, hi, lo), np.where(m, lo, hi)
        orgs.append(o)
        curs.append(c)
    return Domain(name, bd, flags, np.concatenate(orgs), np.concatenate(curs), hi - lo)


B_SAD = ((128, 128, 0), (128, 128, 1), (64, 64, 0), (64, 64, 1), (16, 16, 1), (8, 8, 0), (128, 2, 1), (8, 2, 1), (2, 2, 1), (16, 1, 0), (128, 1, 0), (2, 1, 0),
         (2, 4, 0), (2, 8, 1), (4, 4, 0), (4, 8, 1), (6, 6, 0), (6, 4, 1), (12, 8, 0), (12, 16, 1),
         (24, 16, 0), (24, 16, 1), (40, 8, 0), (40, 8, 1), (72, 24, 0), (72, 24, 1), (96, 4, 0), (96, 4, 1), (120, 128, 0), (120, 128, 1))
B_SSE = tuple(sorted({(w, h, 0) for (w, h, _) in B_SAD}))
B_PLACES = ((0, 0, 0, 0), (2, 0, 3, 1), (1, 1, 4, 0), (0, 0, 1, 0))          # the last one turns the checkers and the column stripes into equal blocks


def _b_items(w, h):
    return [(ox, r * B_RH + oy, cx, r * B_RH + cy) for r in range(len(B_KINDS)) for (ox, oy, cx, cy) in B_PLACES if max(ox, cx) + w <= B_W and max(oy, cy) + h <= B_RH]


@lru_cache(maxsize=None)
def b_jobs(name):
    """SAD of every shape; SSE of every shape except on the 65535 planes, where the reference's `int` square is undefined"""
    jobs = [Job("SAD", w, h, ss, _b_items(w, h)) for (w, h, ss) in B_SAD]
    if name != "d65535":
        jobs += [Job("SSE", w, h, 0, _b_items(w, h)) for (w, h, _) in B_SSE]
    return jobs


# ---- family C ----------------------------------------------------------------------------------------------------------------------------------------------------
C_H, C_W = 160, 264
C_NS = (1, 2, 3, 63, 64, 65, 127, 129, 257)
C_KINDS = ("shared", "unshared", "mixed")
C_FUNCS = (("SAD", 8, 8, 0), ("SAD", 16, 16, 1), ("SSE", 16, 16, 0), ("SSE", 8, 8, 0), ("HAD", 8, 8, 0), ("HAD_fast", 32, 32, 0), ("HAD", 16, 16, 0), ("SAD", 24, 8, 0), ("SAD", 64, 64, 0))


@lru_cache(maxsize=None)
def c_domain(flags=0):
    rng = np.random.default_rng(4300)
    org, cur = rng.integers(0, 1024, (C_H, C_W)), rng.integers(0, 1024, (C_H, C_W))
    cur[40:120, 60:200] = np.clip(org[40:120, 60:200] + rng.integers(-4, 5, (80, 140)), 0, 1023)
    org[:40, :72] = np.where(rng.integers(0, 2, (40, 72)) == 1, 1023, 0)
    cur[:40, :72] = 1023 - org[:40, :72]
    org[120:, :64] = cur[120:, :64] = 512                      # equal blocks but for one sample in 64: the Hadamard cost is far above twice the SAD
    cur[124::8, 4:64:8] = 1023
    return Domain("tex%d" % flags, 10, flags, org, cur, 1023)


def c_items(n, kind, w, h, seed):
    """n items: `shared` — items 2 k and 2 k + 1 have one org_off (a lane team's two candidates); `unshared` — never; `mixed` — every second pair"""
    rng = np.random.default_rng(4400 + seed)
    out = []
    for i in range(n):
        share = kind == "shared" or (kind == "mixed" and (i // 2) % 2 == 0)
        if i % 2 and share:
            ox, oy = out[-1][:2]
        else:
            ox, oy = int(rng.integers(0, C_W - w + 1)), int(rng.integers(0, C_H - h + 1))
            if i % 2 and (ox, oy) == out[-1][:2]:
                ox = (ox + 1) % (C_W - w + 1)
        out.append((ox, oy, int(rng.integers(0, C_W - w + 1)), int(rng.integers(0, C_H - h + 1))))
    return out


@lru_cache(maxsize=None)
def c_list_jobs():
    jobs = []
    for i, n in enumerate(C_NS):
        for j, (func, w, h, ss) in enumerate(C_FUNCS):
            if w == 64 and n > 129:
                continue
            jobs.append(Job(func, w, h, ss, c_items(n, C_KINDS[(i + j) % 3], w, h, 16 * i + j), C_KINDS[(i + j) % 3]))
    # HAD_2SAD on both sides of its minimum: blocks a few levels apart (the cost near twice the SAD), single-sample differences (far above it), unrelated blocks (below it)
    for (w, h) in ((8, 8), (16, 16), (4, 4), (8, 4), (32, 32)):
        near = [(x, y, x, y) for y in range(40, 120 - h + 1, max(h, 16)) for x in range(60, 200 - w + 1, max(w, 24))]
        lone = [(x, y, x, y) for y in range(120, 160 - h + 1, max(h, 8)) for x in range(0, 64 - w + 1, max(w, 8))]
        jobs.append(Job("HAD_2SAD", w, h, 0, near + lone + c_items(9, "unshared", w, h, 2000 + w), "unshared"))
    return jobs


C_XCD = (("HAD", 64, 8), ("HAD", 64, 9), ("HAD", 64, 15), ("HAD", 64, 17), ("SAD", 64, 63), ("SAD", 64, 65), ("SAD", 64, 118), ("SAD", 64, 129))
_C_SIZES = ((8, 8), (16, 16), (32, 32), (64, 64), (16, 8), (32, 16), (24, 24), (8, 16))
_C_TN = (5, 64, 3, 65, 2, 33, 1, 17)


@lru_cache(maxsize=None)
def c_tables():
    """{name: [Job]}: 9, 16 and 17 mergeable SAD / SSE jobs, the same of Hadamard jobs, the workgroup counts of C_XCD, and an interleaved table (None: a job with n = 0)"""
    t = {}
    for k in (9, 16, 17):
        t["sadsse%d" % k] = [Job(("SAD", "SSE")[i % 2], *_C_SIZES[i % 8], (i // 2) % 2 if i % 2 == 0 and _C_SIZES[i % 8][1] >= 2 else 0,
                                 c_items(_C_TN[(i + k) % 8], C_KINDS[i % 3], *_C_SIZES[i % 8], 300 + 20 * k + i)) for i in range(k)]
        t["had%d" % k] = [Job(("HAD", "HAD_fast")[(i // 2) % 2], s, s, 0, c_items(_C_TN[(i + k) % 8] % 40 + 1, "unshared", s, s, 700 + 20 * k + i))
                          for i, s in ((i, (8, 16, 32, 64)[i % 4]) for i in range(k))]
    t["xcd"] = [Job(f, s, s, 0, c_items(n, "mixed", s, s, 900 + i)) for i, (f, s, n) in enumerate(C_XCD)]
    mk = lambda f, w, h, ss, n, s: Job(f, w, h, ss, c_items(n, "mixed", w, h, 1000 + s))
    t["mixed"] = [mk("SAD", 8, 8, 0, 65, 0), mk("HAD", 8, 8, 0, 9, 1), mk("SSE", 16, 16, 0, 3, 2), mk("HAD", 4, 4, 0, 7, 3), None, mk("HAD_fast", 32, 32, 0, 5, 4), mk("SAD", 64, 64, 0, 63, 5),
                  mk("SAD", 4, 4, 0, 6, 6), mk("HAD", 64, 64, 0, 9, 7), None, mk("SSE", 32, 32, 0, 2, 8), mk("HAD", 16, 16, 0, 17, 9), mk("SAD", 16, 16, 1, 64, 10), None,
                  mk("HAD_fast", 16, 16, 0, 4, 11), mk("SSE", 8, 8, 0, 129, 12), mk("HAD", 8, 4, 0, 5, 13), mk("SAD", 24, 8, 0, 33, 14)]
    return t


def table_orders(n):
    """forward, reversed, shuffled"""
    return list(range(n)), list(range(n))[::-1], [int(v) for v in np.random.default_rng(4500 + n).permutation(n)]


# ---- family D ----------------------------------------------------------------------------------------------------------------------------------------------------
D_PAD, D_W = 9, 70
D_PLANES = ((88, 45), (89, 45), (92, 45), (95, 45), (96, 46))      # (stride, height): 63 rows (64 the last); strides 0, 1, 4, 7, 0 mod 8; 89 and 95 are odd
D_ORG_PHASES = (0, 1, 7)


@lru_cache(maxsize=None)
def d_storage(stride, height):
    """(org, cur): the whole storage of a padded plane, margins and the columns beyond them included, as 10-bit samples with a patch of the two extremes"""
    rng = np.random.default_rng(4600 + stride)
    rows = height + 2 * D_PAD
    org, cur = rng.integers(0, 1024, (rows, stride)), rng.integers(0, 1024, (rows, stride))
    org[8:32, 16:56] = np.where(rng.integers(0, 2, (24, 40)) == 1, 1023, 0)
    cur[8:32, 16:56] = 1023 - org[8:32, 16:56]
    return _ro(org), _ro(cur)


@lru_cache(maxsize=None)
def d_items(stride, height):
    """{name: [(ox, oy, cx, cy)]} in STORAGE coordinates (sample (0, 0) of the plane is at (D_PAD, D_PAD)).  phases: every candidate phase with the nine original phases of
    D_ORG_PHASES squared, the tile indices walking over the plane; aligned: 64 items on the tile grid; one_off: the same with item 37's candidate three samples to the
    right; corners: the four corners of the storage, original x candidate"""
    rows = height + 2 * D_PAD
    tx, ty = (stride - 8) // 8, (rows - 8) // 8          # a block at tile (tx, ty) with phase 7 ends at 8 tx + 14 <= stride - 1 + 7: keep x + 8 <= stride
    ph, k = [], 0
    for py in D_ORG_PHASES:
        for px in D_ORG_PHASES:
            for q in range(64):
                qx, qy = q & 7, q >> 3
                a, b, c, d = (k * 3) % tx, (k * 5) % ty, (k * 7 + 1) % tx, (k + 2) % ty
                ph.append((8 * a + px, 8 * b + py, 8 * c + qx, 8 * d + qy))
                k += 1
    al = [(8 * ((i * 3) % (tx + 1)), 8 * ((i * 5) % (ty + 1)), 8 * ((i * 7 + 1) % (tx + 1)), 8 * ((i + 2) % (ty + 1))) for i in range(64)]
    one = list(al)
    one[37] = (al[37][0], al[37][1], 8 * 2 + 3, al[37][3])
    cs = ((0, 0), (stride - 8, 0), (0, rows - 8), (stride - 8, rows - 8))
    out = {"phases": ph, "aligned": al, "one_off": one, "corners": [o + c for o in cs for c in cs]}
    for v in out.values():
        assert all(0 <= x and x + 8 <= stride and 0 <= y and y + 8 <= rows for (ox, oy, cx, cy) in v for (x, y) in ((ox, oy), (cx, cy)))
    return out


@lru_cache(maxsize=None)
def d_domain(stride, height):
    org, cur = d_storage(stride, height)
    return Domain("d%d" % stride, 10, 0, org, cur, 1023, any_pitch=True)


@lru_cache(maxsize=None)
def d_jobs(stride, height):
    """8x8 SAD and SSE on every item list of d_items (the flagged SSE has the SSE's values), and 16x16 SAD with sub_shift 1 on the phase items that leave room for it (the
    row-major body with the shifted copy, which an odd stride must ignore)"""
    rows = height + 2 * D_PAD
    it = d_items(stride, height)
    jobs = [Job(f, 8, 8, 0, v, k) for k, v in it.items() for f in ("SAD", "SSE")]
    big = [i for i in it["phases"] if max(i[0], i[2]) + 16 <= stride and max(i[1], i[3]) + 16 <= rows]
    return jobs + [Job("SAD", 16, 16, 1, big[:150], "phases")]


def dist_work():
    """(family, Domain, Job) of everything the GPU tier asks the oracle about the five list functions (the masked SAD and the fixed-weight SSE have their own item lists)"""
    for name in A_DOMAINS:
        for job in a_batch_jobs():
            yield "A-batch", a_domain(name), job
    for name in A_MULTI_DOMAINS:
        for job in a_multi_jobs():
            yield "A-multi", a_domain(name), job
    for name in B_DOMAINS:
        for job in b_jobs(name):
            yield "B", b_domain(name), job
    for job in c_list_jobs():
        yield "C-lists", c_domain(), job
    for name, table in c_tables().items():
        for job in table:
            if job is not None:
                yield "C-" + name, c_domain(), job
    for (stride, height) in D_PLANES:
        for job in d_jobs(stride, height):
            yield "D", d_domain(stride, height), job


# ---- family E ----------------------------------------------------------------------------------------------------------------------------------------------------
E_SIZES = ((1, 1), (3, 5), (8, 8), (128, 16), (128, 128))
E_STEPS = (1, -1, 2)
E_MW, E_MRH, E_MX, E_MY = 704, 140, 288, 2
E_MASKS = ("max", "min", "mixed")
E_DOMAINS = ("d65535", "p10")


@lru_cache(maxsize=None)
def e_mask():
    rng = np.random.default_rng(4700)
    m = np.zeros((3 * E_MRH, E_MW), np.int64)
    m[:E_MRH], m[E_MRH:2 * E_MRH] = 32767, -32768
    m[2 * E_MRH:] = rng.choice([32767, -32768, -32768, -1, 1, 0, 8, -9], (E_MRH, E_MW))
    return _ro(m)


def e_ms2(w, step_x):
    """three mask_stride2: the mask window goes straight down, drifts one column to the right, one to the left per evaluated row"""
    return (-w * step_x, -w * step_x + 1, -w * step_x - 1)


@lru_cache(maxsize=None)
def e_mask_items(name):
    """[(w, h, ss, step_x, ms2, [(ox, oy, cx, cy, mx, my)])]: per size the regions of the B planes x the three masks"""
    out = []
    for (w, h) in E_SIZES:
        for ss in ((0, 1) if h % 2 == 0 else (0,)):
            for sx in E_STEPS:
                for ms2 in e_ms2(w, sx):
                    items = []
                    for r, (ox, oy, cx, cy) in enumerate(((0, 0, 0, 0), (2, B_RH, 3, B_RH + 1), (1, 2 * B_RH + 1, 4, 2 * B_RH), (0, 5 * B_RH, 1, 5 * B_RH))):
                        if max(ox, cx) + w > B_W:
                            ox = cx = 0
                        for mk in range(3):
                            items.append((ox, oy, cx, cy, E_MX + (w - 1 if sx < 0 else 0) + r, mk * E_MRH + E_MY + r))
                    out.append((w, h, ss, sx, ms2, items))
    return out


E_LEVELS = (0, 1, 255, 1023, 4095, 32767, 46340)
E_WEIGHTS = (0, 1, (1 << 16) - 1, 1 << 16, 1 << 20)
E_WSIZES = ((1, 1), (1, 128), (2, 2), (2, 128), (128, 1), (128, 128), (8, 8))
E_LW, E_LRH = 136, 130


@lru_cache(maxsize=None)
def e_levels_domain():
    """one region per difference level d: org = ceil(d / 2) minus 0 .. 1 on a checker of 3x3 blocks, cur = org - d at its even samples (so |d| <= the level everywhere and
    equal to it on most samples)"""
    yy, xx = np.mgrid[0:E_LRH, 0:E_LW]
    dip = (((xx // 3) + (yy // 3)) & 1) * ((xx + yy) & 1)
    orgs, curs = [], []
    for d in E_LEVELS:
        o = xx * 0 + (d + 1) // 2
        orgs.append(o)
        curs.append(o - d + (dip if d else 0))
    return Domain("levels", 16, 0, np.concatenate(orgs), np.concatenate(curs), E_LEVELS[-1])


@lru_cache(maxsize=None)
def e_wsse_items():
    """[(w, h, [(ox, oy, cx, cy, weight)])]: per level the fixed weights that keep the term inside `int`, and the largest weight that does"""
    out = []
    for (w, h) in E_WSIZES:
        items = []
        for r, d in enumerate(E_LEVELS):
            top = wsse_max_weight(d)
            for i, wt in enumerate(sorted({v for v in E_WEIGHTS if v <= top} | {top})):
                items.append((i % 3, r * E_LRH + (i % 2), (i + 1) % 4, r * E_LRH + ((i + 1) % 2), wt))
        out.append((w, h, items))
    return out
