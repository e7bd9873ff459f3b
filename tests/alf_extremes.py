"""Deterministic extreme inputs of the ALF stage (classification, covariance statistics, 7x7 / 5x5 filtering, CC-ALF statistics and filtering),
shared by the CPU tier (tests/test_oracle_alf_extremes.py: oracle against the compiled reference) and the GPU tier
(tests/test_gpu_alf_extremes.py: every kernel form against the oracle).

The pictures of the parity suites (sinusoids with noise, org - rec within +-12, coefficients within +-40) stay far from the limits of the
arithmetic.  These reach them: two-level planes of (0, 2^bd - 1) push every per-block int32 dot product of the statistics beyond 2^24, where
the int -> float conversion and every float addition of the ordered chains round; class maps supplied by the test hit every class, every
transpose index and the longest chain; low-amplitude planes put the classifier's comparisons on exact equality; full-range coefficients
drive the filters into both clips, also on the rows next to the virtual boundary.  The int64 models below compute the intermediates the
guards of the CPU tier check, so a test shows that a limit was reached and not only that two outputs matched.

Chroma planes are generated at the chroma size (half the luma shape) instead of decimating a luma pattern: a 2:1 decimation of a period-2
pattern is a constant.
"""
import numpy as np

# (H, W), CTU size, (vb_ctu_height, vb_pos) — luma
LUMA_32 = ((72, 104), 32, (32, 28))            # partial CTUs on both axes, a last block row of 2 (rows % 4 != 0 in the four-row ring of the ordered kernel)
LUMA_128 = ((132, 136), 128, (128, 124))       # one full 32x32-block CTU (all 32 lanes of a class row) plus slivers 8 wide and 4 high
LUMA_WIDE = ((36, 264), 32, (32, 28))          # crosses the filter's 256x16 LDS tile in x with an 8-sample remainder; the last tile row is partial
CCALF_LUMA = ((64, 96), 32, (32, 28))          # chroma 32x48 with chroma CTU 16: whole chroma CTUs, the boundary-free last CTU row
CLASSIFY_VB = ((32, 28), (128, 124), (8, 4))
# (statistics unit, CTU) pairs of the 72x104 plane; (128, 16) and (128, 8) need 256 / 512 steps of the unit walk
UNIT_PAIRS = ((64, 32), (128, 32), (128, 64), (128, 16), (64, 8), (128, 8))
CHROMA_UNIT_PAIRS = ((32, 16), (64, 16), (64, 8))

KINDS = ("const_max", "const_0", "checker", "cols", "rows", "blocks2", "blocks4", "diag0", "diag1", "random")
# (org, rec) of the statistics
STAT_PAIRS = (("checker", "const_max"), ("const_max", "checker"), ("random", "random"), ("cols", "rows"), ("blocks4", "blocks2"), ("const_max", "const_0"))
CCALF_LUMA_KINDS = ("checker", "cols", "rows", "blocks2", "diag0", "random")      # luma of the CC-ALF cases
CLASS_MAPS = ("derived", "every", "one", "every_unused")
# (amplitude, seed) of the low-amplitude planes.  Counted with tie_counts below at 10 bits / 72x104 / virtual boundary (32, 28), non-zero operands, blocks off the
# boundary rows: these four planes give V == H 47 times, D0 == D1 55, the cross product 8, hvd1 == 2 hvd0 once, 2 hvd1 == 9 hvd0 never
TIE_SEEDS = ((1, 5), (2, 5), (3, 5), (5, 5))
# (stripe amplitude, noise density, seed) of striped_low planes: noise alone never gave 2 hvd1 == 9 hvd0 with non-zero operands (4 amplitudes x 200 seeds searched), a
# strongly directional plane with sparse +-1 noise does: 6 and 3 such blocks; the second one also yields class 16 (activity 1, vertical, moderate), which no other
# 10-bit plane here does
STRIPE_SEEDS = ((1, 0.2, 17), (3, 0.5, 33))


def chroma_of(setting):
    (h, w), ctu, (vbh, vbp) = setting
    return (h // 2, w // 2), ctu // 2, (vbh // 2, vbp // 2)


def pattern(kind, bd, h, w, seed=0):
    """two-level planes of (0, 2^bd - 1)"""
    a, b = (1 << bd) - 1, 0
    yy, xx = np.mgrid[0:h, 0:w]
    if kind == "const_max":
        v = np.full((h, w), a)
    elif kind == "const_0":
        v = np.full((h, w), b)
    elif kind == "checker":
        v = np.where((xx + yy) & 1, a, b)
    elif kind == "cols":
        v = np.where(xx & 1, a, b)
    elif kind == "rows":
        v = np.where(yy & 1, a, b)
    elif kind == "blocks2":
        v = np.where(((xx >> 1) + (yy >> 1)) & 1, a, b)
    elif kind == "blocks4":
        v = np.where(((xx >> 2) + (yy >> 2)) & 1, a, b)
    elif kind == "diag0":
        v = np.where((xx + yy) % 3 == 0, a, b)
    elif kind == "diag1":
        v = np.where((xx - yy) % 3 == 0, a, b)
    elif kind == "random":
        v = np.where(np.random.default_rng(9000 + seed).integers(0, 2, (h, w)) == 1, a, b)
    else:
        raise ValueError(kind)
    return np.ascontiguousarray(v.astype(np.int16))


def stat_planes(bd, h, w):
    """the two-level planes of the statistics by kind, plus a second random one"""
    return {k: pattern(k, bd, h, w, seed) for seed, k in enumerate(KINDS)} | {"random2": pattern("random", bd, h, w, 77)}


def stat_pair(planes, o, r):
    """(org, rec) of a STAT_PAIRS entry: (random, random) takes two different random planes"""
    return planes[o], planes["random2" if (o, r) == ("random", "random") else r]


def low_amplitude(bd, h, w, a, seed):
    """mid + U{0..a}: Laplacian sums of a few units each, where the classifier's comparisons meet exact equality"""
    rng = np.random.default_rng(100 * a + seed)
    return ((1 << (bd - 1)) + rng.integers(0, a + 1, (h, w))).astype(np.int16)


def striped_low(bd, h, w, s, p, seed):
    """mid + s (x & 1) + sparse noise of -1 / 0 / +1 with density p: one dominant direction and a small second one, for the two strength thresholds"""
    rng = np.random.default_rng(seed)
    xx = np.mgrid[0:h, 0:w][1]
    n = np.where(rng.random((h, w)) < p, rng.integers(-1, 2, (h, w)), 0)
    return ((1 << (bd - 1)) + s * (xx & 1) + n).astype(np.int16)


def ramp(bd, h, w, kind, seed=0):
    """noise / stripes whose amplitude grows from 0 at the left edge to the full range at the right: sweeps the activity value through 0..15 and beyond its clip"""
    mid, top = 1 << (bd - 1), (1 << bd) - 1
    yy, xx = np.mgrid[0:h, 0:w]
    amp = (xx.astype(np.float64) / max(w - 1, 1)) ** 2 * mid
    if kind == "noise":
        s = np.random.default_rng(7000 + seed).uniform(-1, 1, (h, w))
    elif kind == "cols":
        s = np.where(xx & 1, 1.0, -1.0)
    elif kind == "rows":
        s = np.where(yy & 1, 1.0, -1.0)
    else:
        s = np.where((xx + yy) % 3 == 0, 1.0, -0.5)
    return np.clip(np.rint(mid + amp * s), 0, top).astype(np.int16)


def classify_planes(bd, h, w):
    """[(name, plane)]: every two-level pattern, the low-amplitude planes of TIE_SEEDS and STRIPE_SEEDS, the amplitude ramps"""
    out = [(k, pattern(k, bd, h, w)) for k in KINDS]
    out += [("low%d_s%d" % (a, s), low_amplitude(bd, h, w, a, s)) for a, s in TIE_SEEDS]
    out += [("stripes%d_s%d" % (a, s), striped_low(bd, h, w, a, p, s)) for a, p, s in STRIPE_SEEDS]
    out += [("ramp_" + k, ramp(bd, h, w, k)) for k in ("noise", "cols", "rows", "diag")]
    return out


def filter_planes(bd, h, w):
    """planes of the filter tests: two-level patterns (both clips), ramps and a low-amplitude plane (results inside the range)"""
    out = [(k, pattern(k, bd, h, w)) for k in ("checker", "cols", "rows", "blocks2", "diag0", "random")]
    out += [("ramp_" + k, ramp(bd, h, w, k)) for k in ("noise", "diag")]
    out.append(("low5", low_amplitude(bd, h, w, 5, 1)))
    return out


# ---- class maps --------------------------------------------------------------------------------------------------------------
def class_map(kind, h, w, derived=None):
    """(h/4, w/4, 2) uint8 {classIdx, transposeIdx}: `derived` (the caller's classification), `every` (block i: class i % 25, transpose (i // 25) % 4: all 100 pairs),
    `one` (all blocks {24, 3}: the longest chain), `every_unused` (`every` with a third of the blocks {255, 255})"""
    bh, bw = h // 4, w // 4
    if kind == "derived":
        assert derived is not None and derived.shape == (bh, bw, 2)
        return np.ascontiguousarray(derived, np.uint8)
    i = np.arange(bh * bw).reshape(bh, bw)
    if kind == "one":
        m = np.stack([np.full_like(i, 24), np.full_like(i, 3)], -1)
    else:
        m = np.stack([i % 25, (i // 25) % 4], -1)
        if kind == "every_unused":
            m[i % 3 == 1] = 255
        elif kind != "every":
            raise ValueError(kind)
    return np.ascontiguousarray(m.astype(np.uint8))


# ---- filter sets -------------------------------------------------------------------------------------------------------------
COEFF_KINDS = ("p127", "m128", "alt", "uniform")


def coeff_set(kind, num_classes, seed=0, limit=None):
    """(num_classes, 13) int16 coefficients of the syntax range -128..127 (slot 12 = 0); `limit`: sum of |c_k| over the 12 taps bounded by it (equal magnitudes)"""
    c = np.zeros((num_classes, 13), np.int64)
    k = np.arange(12)
    if kind == "p127":
        c[:, :12] = 127
    elif kind == "m128":
        c[:, :12] = -128
    elif kind == "alt":
        c[:, :12] = np.where((k[None, :] + np.arange(num_classes)[:, None]) & 1, -128, 127)
    elif kind == "uniform":
        c[:, :12] = np.random.default_rng(300 + seed).integers(-128, 128, (num_classes, 12))
    else:
        raise ValueError(kind)
    if limit is not None:
        m = limit // 12
        c[:, :12] = np.where(c[:, :12] < 0, -m, m) if kind != "uniform" else np.clip(c[:, :12], -m, m)
    return c.astype(np.int16)


def coeff_sets(num_classes, seed=0, limit=None):
    """(4, num_classes, 13): one set per COEFF_KINDS entry"""
    return np.ascontiguousarray(np.stack([coeff_set(k, num_classes, seed, limit) for k in COEFF_KINDS]))


def clip_values(bd):
    """the clipping values of AlfClipIdx 0..3 (index 0 = 1 << bd never bites)"""
    return np.array([1 << bd, 1 << (bd - 3), 1 << (bd - 5), 1 << max(1, bd - 7)], np.int16)


CLIP_KINDS = ("idx0", "idx1", "idx2", "idx3", "mixed")


def clip_sets(kind, bd, num_sets, num_classes, seed=0):
    v = clip_values(bd)
    if kind == "mixed":
        return np.ascontiguousarray(v[np.random.default_rng(500 + seed).integers(0, 4, (num_sets, num_classes, 13))])
    return np.full((num_sets, num_classes, 13), v[int(kind[3])], np.int16)


def ctu_sets(nctu, num_sets, seed=0):
    """filter set per CTU, disabled CTUs (-1) mixed in; every set and -1 occur when nctu allows"""
    s = (np.arange(nctu) + seed) % (num_sets + 1) - 1
    return s.astype(np.int16)


def ccalf_coeffs(seed=0):
    """(4, 8) int16 CC-ALF filters (7 slots used): all +64, all -64, alternating +-64, random signed powers of two"""
    c = np.zeros((4, 8), np.int64)
    c[0, :7], c[1, :7] = 64, -64
    c[2, :7] = np.where(np.arange(7) & 1, -64, 64)
    rng = np.random.default_rng(600 + seed)
    c[3, :7] = np.array([1, 2, 4, 8, 16, 32, 64])[rng.integers(0, 7, 7)] * rng.choice([-1, 1], 7)
    return c.astype(np.int16)


# ---- int64 models for the guards ---------------------------------------------------------------------------------------------
def laplacian_sums(plane):
    """(4, H/4, W/4) int64: sumV, sumH, sumD0, sumD1 of every 4x4 block with all four rows of 2:1-subsampled positions counted and no row folded:
    what the classifier sums for blocks that are not on a virtual-boundary row (see off_boundary)"""
    h, w = plane.shape
    P = np.pad(plane.astype(np.int64), 4, mode="edge")
    ny, nx = h // 2 + 2, w // 2 + 2                                  # positions y = -2, 0, .., h; x = -2, 0, .., w

    def S(dy, dx):
        return P[2 + dy:2 + dy + 2 * ny:2, 2 + dx:2 + dx + 2 * nx:2]
    y0, y1 = 2 * S(0, 0), 2 * S(1, 1)
    lap = (np.abs(y0 - S(-1, 0) - S(1, 0)) + np.abs(y1 - S(0, 1) - S(2, 1)),
           np.abs(y0 - S(0, 1) - S(0, -1)) + np.abs(y1 - S(1, 2) - S(1, 0)),
           np.abs(y0 - S(-1, -1) - S(1, 1)) + np.abs(y1 - S(0, 0) - S(2, 2)),
           np.abs(y0 - S(1, -1) - S(-1, 1)) + np.abs(y1 - S(2, 0) - S(0, 2)))
    bh, bw = h // 4, w // 4
    return np.stack([sum(L[i:i + 2 * bh:2, j:j + 2 * bw:2] for i in range(4) for j in range(4)) for L in lap])


def off_boundary(h, w, vbh, vbp):
    """(H/4, W/4) bool: blocks whose row is not one of the two block rows next to the virtual boundary"""
    ym = (np.arange(h // 4) * 4) % vbh
    return np.repeat(((ym != vbp) & (ym != vbp - 4))[:, None], w // 4, 1)


def classify_model(sums, bd):
    """the classifier's decisions from the four sums -> dict: cls (H/4, W/4, 2), act_raw (activity before its clip at 15), and the five comparisons'
    equalities with non-zero operands: vh (V == H), d (D0 == D1), cross (d1 hv0 == hv1 d0 in uint32), s1 (hvd1 == 2 hvd0), s2 (2 hvd1 == 9 hvd0)"""
    V, H, D0, D1 = sums
    act_raw = ((V + H) * 64) >> (bd + 4)
    th = np.array([0, 1, 2, 2, 2, 2, 2, 3, 3, 3, 3, 3, 3, 3, 3, 4])[np.clip(act_raw, 0, 15)]
    vgt, dgt = V > H, D0 > D1
    hv1, hv0, dir_hv = np.where(vgt, V, H), np.where(vgt, H, V), np.where(vgt, 1, 3)
    d1, d0, dir_d = np.where(dgt, D0, D1), np.where(dgt, D1, D0), np.where(dgt, 0, 2)
    lhs, rhs = (d1 * hv0) & 0xffffffff, (hv1 * d0) & 0xffffffff
    dm = lhs > rhs
    hvd1, hvd0 = np.where(dm, d1, hv1), np.where(dm, d0, hv0)
    main, sec = np.where(dm, dir_d, dir_hv), np.where(dm, dir_hv, dir_d)
    strength = np.where(2 * hvd1 > 9 * hvd0, 2, np.where(hvd1 > 2 * hvd0, 1, 0))
    cls = th + np.where(strength > 0, (((main & 1) << 1) + strength) * 5, 0)
    tr = np.array([0, 1, 0, 2, 2, 3, 1, 3])[main * 2 + (sec >> 1)]
    return {"cls": np.stack([cls, tr], -1).astype(np.uint8), "act_raw": act_raw,
            "vh": (V == H) & (V > 0), "d": (D0 == D1) & (D0 > 0), "cross": (lhs == rhs) & (lhs > 0), "s1": (hvd1 == 2 * hvd0) & (hvd0 > 0), "s2": (2 * hvd1 == 9 * hvd0) & (hvd0 > 0)}


TIES = ("vh", "d", "cross", "s1", "s2")


def tie_counts(plane, bd, vbh, vbp):
    m = classify_model(laplacian_sums(plane), bd)
    ok = off_boundary(plane.shape[0], plane.shape[1], vbh, vbp)
    return {k: int((m[k] & ok).sum()) for k in TIES}


def block_dots(org, rec, vbh, vbp):
    """(5, H/4, W/4) int64 per-block dot products of the 7x7 statistics that every transpose index has: pixAcc = sum (org - rec)^2, the centre term sum rec^2, and the
    diagonal entries of the taps (0, -1), (0, -2) and (-1, 0): sums of squared horizontal (distance 1 and 2) / vertical second differences (the vertical one 0 on the
    blocks next to the virtual boundary, where the tap folds)"""
    h, w = rec.shape
    d = org.astype(np.int64) - rec.astype(np.int64)
    P = np.pad(rec.astype(np.int64), 2, mode="edge")
    r = P[2:-2, 2:-2]
    dh = P[2:-2, 1:-3] + P[2:-2, 3:-1] - 2 * r
    dh2 = P[2:-2, :-4] + P[2:-2, 4:] - 2 * r
    dv = (P[1:-3, 2:-2] + P[3:-1, 2:-2] - 2 * r) * np.repeat(np.repeat(off_boundary(h, w, vbh, vbp), 4, 0), 4, 1)
    return np.stack([(a * a).reshape(h // 4, 4, w // 4, 4).sum(axis=(1, 3)) for a in (d, r, dh, dh2, dv)])


def ccalf_sums(luma, coeff, vbh, vbp):
    """CC-ALF (4:2:0): the rounded, unclamped correction (sum + 64) >> 7 of every chroma sample for one filter (7 coefficients) -> (int64 (H/2, W/2), valid): rows whose
    luma row is within two of the virtual boundary fold their taps and are left to the oracle (valid False)"""
    h, w = luma.shape
    P = np.pad(luma.astype(np.int64), 2, mode="edge")

    def S(dy, dx):
        return P[2 + dy:2 + dy + h:2, 2 + dx:2 + dx + w:2]
    c = S(0, 0)
    cf = [int(v) for v in coeff[:7]]
    s = cf[0] * (S(-1, 0) - c) + cf[1] * (S(0, -1) - c) + cf[2] * (S(0, 1) - c) + cf[3] * (S(1, -1) - c) + cf[4] * (S(1, 0) - c) + cf[5] * (S(1, 1) - c) + cf[6] * (S(2, 0) - c)
    pos = (np.arange(h // 2) * 2) & (vbh - 1)
    valid = ~np.isin(pos, (vbp - 2, vbp - 1, vbp, vbp + 1))
    return (s + 64) >> 7, np.repeat(valid[:, None], w // 2, 1)
