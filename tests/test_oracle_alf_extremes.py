"""Pins the oracle to the compiled reference (scalar row and x86 SIMD row, tolerance 0, floats as bit patterns) on the ALF stage's extreme inputs of
tests/alf_extremes.py: two-level planes at the bit-depth maximum, class maps that hit every class / transpose index / the longest chain, statistics units down to
CTUs of 8 inside units of 128, low-amplitude planes on the classifier's exact ties, full-range filter coefficients and clipping values, CC-ALF at both clamps.
The GPU tier (tests/test_gpu_alf_extremes.py) compares the kernels with the oracle on the same sets; this file is what makes the oracle trustworthy there.
The guards assert that the sets reach the limits they are built for; they are computed from the oracle's outputs and the int64 models of alf_extremes.

One place where the reference's two rows part: at 12 bits with large coefficients the x86 row of filterBlk leaves the scalar row (it packs sum >> 7 to 16 bits
with saturation; 2 * 4095 * sum |c_k| / 128 exceeds 32767 once sum |c_k| > 512).  Measured here with 12 equal-magnitude taps on the filter planes (72x104 and
36x264, three sign patterns, two clipping sets: 108 cases per magnitude): the rows agree in 108 of 108 cases for every sum |c_k| <= 504 and differ in 2 of 108
from 516 on.  The oracle and the kernels' int32 arithmetic follow the scalar row.  So the 12-bit cases with sum |c_k| <= 400 assert scalar == x86 == oracle
with no case left out, and the full-range 12-bit cases are compared with the scalar row only.
"""
import numpy as np
import pytest

import alf_extremes as X

pytestmark = pytest.mark.ref

F24 = float(1 << 24)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _ref_classify(reflib, p, bd, vbh, vbp):
    """the x86 row classifies areas whose height is a multiple of 8 only (it asserts so): a plane with 4 rows left over is handed over with its replicated border's
    first 4 rows as samples — the same values the classifier reads below the last row anyway — and the classes of the plane's own block rows are returned"""
    h = p.shape[0]
    if reflib.simd and h % 8:
        return reflib.alf_classify(np.pad(p, ((0, 8 - h % 8), (0, 0)), mode="edge"), bd, vbh, vbp)[:h // 4]
    return reflib.alf_classify(p, bd, vbh, vbp)


def test_classification_on_extreme_planes(oracle, reflib):
    """deriveClassificationBlk on every plane at 8 / 10 / 12 bits and three virtual-boundary settings.  Guards: the int64 model reproduces the oracle on every block
    off the boundary rows; all 25 classes and 4 transpose indices occur; every activity value 0..15 occurs and the clip at 15 bites; each of the five comparisons
    meets exact equality with non-zero operands"""
    classes, transposes, acts = set(), set(), set()
    over = 0
    ties = {k: 0 for k in X.TIES}
    for bd in (8, 10, 12):
        for (h, w), _, _ in (X.LUMA_32, X.LUMA_128):
            for name, p in X.classify_planes(bd, h, w):
                m = X.classify_model(X.laplacian_sums(p), bd)
                for vbh, vbp in X.CLASSIFY_VB:
                    a, b = oracle.alf_classify(p, bd, vbh, vbp), _ref_classify(reflib, p, bd, vbh, vbp)
                    assert np.array_equal(a, b), (bd, h, w, name, vbh, vbp)
                    ok = X.off_boundary(h, w, vbh, vbp)
                    assert np.array_equal(a[ok], m["cls"][ok]), ("model", bd, h, w, name, vbh, vbp)
                    classes |= set(a[..., 0].ravel().tolist())
                    transposes |= set(a[..., 1].ravel().tolist())
                    acts |= set(np.clip(m["act_raw"][ok], 0, 15).ravel().tolist())
                    over += int((m["act_raw"][ok] > 15).sum())
                    for k in X.TIES:
                        ties[k] += int((m[k] & ok).sum())
    print("classification guards: classes %d, transposes %d, activities %d, blocks over 15: %d, ties %s" % (len(classes), len(transposes), len(acts), over, ties))
    assert classes == set(range(25)) and transposes == set(range(4)), (sorted(classes), sorted(transposes))
    assert acts == set(range(16)) and over > 0, (sorted(acts), over)
    assert all(v > 0 for v in ties.values()), ties
    # the seeds written into alf_extremes: at 10 bits / 72x104 / boundary (32, 28) alone every tie occurs too
    (h, w), _, (vbh, vbp) = X.LUMA_32
    t10 = {k: sum(X.tie_counts(p, 10, vbh, vbp)[k] for _, p in X.classify_planes(10, h, w)) for k in X.TIES}
    assert all(v > 0 for v in t10.values()), t10


@pytest.mark.parametrize("bd", [8, 10])
def test_statistics_on_extreme_planes(oracle, reflib, bd):
    """getPreBlkStats + the accumulate entry on two-level (org, rec) pairs: luma 7x7 with the four class maps, a plain CTU and every unit / CTU pair (down to CTUs of 8
    in units of 128: 512 steps of the unit walk), the 132x136 plane at CTU 128 with one class (the longest chain) and every class; chroma 5x5 plain and with units.
    Guards: >= 100 record entries >= 2^24 for at least four pairs; with the `every` map all 25 classes have a non-zero pixAcc; at 10 bits per-block dot products >= 2^24"""
    (h, w), ctu, (vbh, vbp) = X.LUMA_32
    planes = X.stat_planes(bd, h, w)
    big = {}
    for o, r in X.STAT_PAIRS:
        org, rec = X.stat_pair(planes, o, r)
        derived = oracle.alf_classify(rec, bd, vbh, vbp)
        n_big = 0
        for kind in X.CLASS_MAPS:
            cm = X.class_map(kind, h, w, derived)
            a, b = oracle.alf_stats_plane(org, rec, ctu, 7, cm, vbh, vbp), reflib.alf_stats_plane(org, rec, ctu, 7, cm, vbh, vbp)
            assert np.array_equal(_bits(a), _bits(b)), (bd, o, r, kind)
            n_big += int((np.abs(a) >= F24).sum())
            if kind == "every":
                assert a.shape[1] == 25 and (a[:, :, 182].sum(axis=0) > 0).all(), (bd, o, r, "a class without samples")
            for unit, c in X.UNIT_PAIRS:
                d = oracle.alf_classify(rec, bd, c, c - 4) if kind == "derived" else None
                cmu = X.class_map(kind, h, w, d)
                a = oracle.alf_stats_plane(org, rec, unit, 7, cmu, c, c - 4, ctu_in_unit=c)
                b = reflib.alf_stats_plane(org, rec, unit, 7, cmu, c, c - 4, ctu_in_unit=c)
                assert np.array_equal(_bits(a), _bits(b)), (bd, o, r, kind, unit, c)
                n_big += int((np.abs(a) >= F24).sum())
        big[(o, r)] = n_big
        if bd == 10 and r not in ("const_max", "const_0"):          # a constant rec leaves 16 * 1023^2 = 2^24 - 32752 as the largest per-block term
            dots = X.block_dots(org, rec, vbh, vbp).max(axis=0)[X.off_boundary(h, w, vbh, vbp)]
            assert (dots >= 1 << 24).mean() >= 0.9, (o, r, "blocks with a dot product >= 2^24", (dots >= 1 << 24).mean())      # all blocks of the periodic patterns
    print("statistics guards, %d bits: record entries >= 2^24 per pair %s" % (bd, big))
    assert sum(v >= 100 for v in big.values()) >= 4, big
    # CTU 128: a full CTU of 32x32 blocks; units of 128 with CTUs of 16 / 8 walk 256 / 512 steps
    (h, w), ctu, (vbh, vbp) = X.LUMA_128
    planes = X.stat_planes(bd, h, w)
    for o, r in X.STAT_PAIRS:
        org, rec = X.stat_pair(planes, o, r)
        for kind in ("one", "every"):
            cm = X.class_map(kind, h, w)
            a, b = oracle.alf_stats_plane(org, rec, ctu, 7, cm, vbh, vbp), reflib.alf_stats_plane(org, rec, ctu, 7, cm, vbh, vbp)
            assert np.array_equal(_bits(a), _bits(b)), (bd, o, r, kind, "CTU 128")
            if kind == "one":
                assert (a[:, :24] == 0).all() and (a[:, 24, 182] > 0).all(), (bd, o, r, "one class")
            for c in (16, 8):
                a = oracle.alf_stats_plane(org, rec, 128, 7, cm, c, c - 4, ctu_in_unit=c)
                b = reflib.alf_stats_plane(org, rec, 128, 7, cm, c, c - 4, ctu_in_unit=c)
                assert np.array_equal(_bits(a), _bits(b)), (bd, o, r, kind, "unit 128", c)
    # chroma 5x5, one class
    (h, w), ctu, (vbh, vbp) = X.chroma_of(X.LUMA_32)
    planes = X.stat_planes(bd, h, w)
    for o, r in X.STAT_PAIRS:
        org, rec = X.stat_pair(planes, o, r)
        a, b = oracle.alf_stats_plane(org, rec, ctu, 5, None, vbh, vbp), reflib.alf_stats_plane(org, rec, ctu, 5, None, vbh, vbp)
        assert np.array_equal(_bits(a), _bits(b)), (bd, o, r, "chroma")
        for unit, c in X.CHROMA_UNIT_PAIRS:
            a = oracle.alf_stats_plane(org, rec, unit, 5, None, c, c - 2, ctu_in_unit=c)
            b = reflib.alf_stats_plane(org, rec, unit, 5, None, c, c - 2, ctu_in_unit=c)
            assert np.array_equal(_bits(a), _bits(b)), (bd, o, r, "chroma", unit, c)


@pytest.mark.parametrize("bd", [8, 10])
def test_ccalf_statistics_on_extreme_planes(oracle, reflib, bd):
    """getBlkStatsCcAlf with org, ALF-filtered chroma and luma from the two-level patterns; partial chroma CTUs (36x52) and whole ones (32x48), both with the
    boundary-free last CTU row.  Guard: at 10 bits record entries >= 2^24 occur for every luma pattern"""
    for setting in (X.LUMA_32, X.CCALF_LUMA):
        (h, w), ctu, (vbh, vbp) = setting
        cp = X.stat_planes(bd, h // 2, w // 2)
        for k, lk in enumerate(X.CCALF_LUMA_KINDS):
            luma = X.pattern(lk, bd, h, w, 3)
            n_big = 0
            for o, r in (X.STAT_PAIRS[k], X.STAT_PAIRS[(k + 3) % 6]):
                org, slf = X.stat_pair(cp, o, r)
                a, b = oracle.ccalf_stats_plane(org, slf, luma, ctu // 2, vbh, vbp), reflib.ccalf_stats_plane(org, slf, luma, ctu // 2, vbh, vbp)
                assert np.array_equal(_bits(a), _bits(b)), (bd, h, w, lk, o, r)
                n_big += int((np.abs(a) >= F24).sum())
            assert n_big > 0 or bd == 8, (bd, h, w, lk)          # 8 bits: a chroma CTU of 16 blocks stays below 16 * 16 * 255^2 < 2^24


def _filter_cases(bd):
    """(label, coefficient limit or None) of a bit depth: full range everywhere; at 12 bits also the sets with sum |c_k| <= 400"""
    return (("full", None), ("sum400", 400)) if bd == 12 else (("full", None),)


@pytest.mark.parametrize("bd", [8, 10, 12])
def test_filtering_on_extreme_planes(oracle, reflib, bd):
    """filterBlk 7x7 (the `every` class map: 25 classes x 4 transposes) and 5x5 with full-range coefficients, every clipping set and the linear table entry, disabled CTUs
    mixed in, on the three shapes.  Guards (10 bits, 36x264, uniform full-range coefficients, clipping values that never bite): outputs clipped to 0 and to the maximum
    each exceed 10 % of the samples, and samples strictly inside the range occur on rows with the 7-bit shift and on the two rows next to the virtual boundary"""
    mx = (1 << bd) - 1
    for label, limit in _filter_cases(bd):
        if bd == 12 and limit is None and reflib.simd:
            continue                                    # the x86 row saturates sum >> 7 at 16 bits (module docstring): full-range 12-bit cases follow the scalar row
        for setting in (X.LUMA_32, X.LUMA_128, X.LUMA_WIDE):
            (h, w), ctu, (vbh, vbp) = setting
            nctu = -(-h // ctu) * -(-w // ctu)
            cm = X.class_map("every", h, w)
            cf = X.coeff_sets(25, 0, limit)
            ctu_set = X.ctu_sets(nctu, 4, h)
            for name, p in X.filter_planes(bd, h, w):
                for ck in X.CLIP_KINDS:
                    cl = X.clip_sets(ck, bd, 4, 25)
                    a = oracle.alf_filter_plane(p, ctu, bd, 7, cf, cl, ctu_set, cm, None, vbh, vbp)
                    b = reflib.alf_filter_plane(p, ctu, bd, 7, cf, cl, ctu_set, cm, None, vbh, vbp)
                    assert np.array_equal(a, b), ("7x7", bd, label, h, w, name, ck)
            (hc, wc), ctu_c, (vbh_c, vbp_c) = X.chroma_of(setting)
            if hc % 4 or wc % 4:
                continue
            cf = X.coeff_sets(1, 1, limit)
            for name, p in X.filter_planes(bd, hc, wc):
                for ck in X.CLIP_KINDS:
                    cl = X.clip_sets(ck, bd, 4, 1)
                    a = oracle.alf_filter_plane(p, ctu_c, bd, 5, cf, cl, ctu_set, None, None, vbh_c, vbp_c)
                    b = reflib.alf_filter_plane(p, ctu_c, bd, 5, cf, cl, ctu_set, None, None, vbh_c, vbp_c)
                    assert np.array_equal(a, b), ("5x5", bd, label, hc, wc, name, ck)
    if bd == 10:
        (h, w), ctu, (vbh, vbp) = X.LUMA_WIDE
        nctu = -(-h // ctu) * -(-w // ctu)
        rows = np.arange(h) & (vbh - 1)
        near = (rows == vbp - 1) | (rows == vbp)
        cf, cl = X.coeff_sets(25), X.clip_sets("idx0", bd, 4, 25)
        for name in ("checker", "blocks2", "random"):
            p = dict(X.filter_planes(bd, h, w))[name]
            o = oracle.alf_filter_plane(p, ctu, bd, 7, cf, cl, np.full(nctu, X.COEFF_KINDS.index("uniform"), np.int16), X.class_map("every", h, w), None, vbh, vbp)
            inside = (o > 0) & (o < mx)
            print("filter guards, %s: %d at 0, %d at max, %d inside (%d on the rows next to the boundary) of %d" % (name, (o == 0).sum(), (o == mx).sum(), inside.sum(), inside[near].sum(), o.size))
            assert (o == 0).sum() > 0.1 * o.size and (o == mx).sum() > 0.1 * o.size, name
            assert inside[near].any() and inside[~near].any(), name


@pytest.mark.parametrize("bd", [8, 10])
def test_ccalf_filtering_on_extreme_planes(oracle, reflib, bd):
    """filterBlkCcAlf with +-64 in every slot and random signed powers of two on two-level luma, chroma at 0 / maximum / mid, every filter and `off`.  Guards (int64
    model of the unclamped correction, rows off the virtual boundary): both ends of the first clamp (sum + half) and of the second (+ dst) bite"""
    mx, half = (1 << bd) - 1, 1 << (bd - 1)
    coeff = X.ccalf_coeffs()
    first_lo = first_hi = second_lo = second_hi = 0
    for setting in (X.LUMA_32, X.CCALF_LUMA):
        (h, w), ctu, (vbh, vbp) = setting
        nctu = -(-(h // 2) // (ctu // 2)) * -(-(w // 2) // (ctu // 2))
        ctu_filter = (np.arange(nctu) % 5).astype(np.uint8)
        for lk in X.CCALF_LUMA_KINDS:
            luma = X.pattern(lk, bd, h, w, 3)
            for level in (0, mx, half):
                chroma = np.full((h // 2, w // 2), level, np.int16)
                for flt in (ctu_filter, np.full(nctu, 1, np.uint8), np.full(nctu, 4, np.uint8)):
                    a = oracle.ccalf_filter_plane(chroma, luma, ctu // 2, bd, coeff, flt, vbh, vbp)
                    b = reflib.ccalf_filter_plane(chroma, luma, ctu // 2, bd, coeff, flt, vbh, vbp)
                    assert np.array_equal(a, b), (bd, h, w, lk, level)
            for f in range(4):
                s, valid = X.ccalf_sums(luma, coeff[f], vbh, vbp)
                s = s[valid]
                c1 = np.clip(s + half, 0, mx) - half
                first_lo += int((s + half < 0).sum()); first_hi += int((s + half > mx).sum())
                second_lo += int((c1 + 0 < 0).sum()); second_hi += int((c1 + mx > mx).sum())
                got = oracle.ccalf_filter_plane(np.full((h // 2, w // 2), half, np.int16), luma, ctu // 2, bd, coeff, np.full(nctu, f + 1, np.uint8), vbh, vbp)
                assert np.array_equal(got[valid], np.clip(c1 + half, 0, mx)), ("model", bd, lk, f)
    print("CC-ALF guards, %d bits: first clamp below 0: %d, above max: %d; second clamp below 0: %d, above max: %d" % (bd, first_lo, first_hi, second_lo, second_hi))
    assert min(first_lo, first_hi, second_lo, second_hi) > 0
