"""-m gpu: every ALF kernel form against the oracle (tolerance 0, floats as bit patterns) on the extreme inputs of tests/alf_extremes.py.  The oracle itself is pinned to
the compiled reference on the same sets by tests/test_oracle_alf_extremes.py, which also holds the guards that show the sets reach the limits: per-block dot products
and record entries beyond 2^24 (where v_cvt_f32_i32 and every float addition of the ordered chains round), every class / transpose index / the longest chain, the
classifier's comparisons on exact equality, both clips of the filters on ordinary rows and on the rows next to the virtual boundary, both clamps of CC-ALF.

Measured on an MI355X: every case below takes 0.01 to 0.20 s (filter at 12 bits 0.20 s, filter at 8 / 10 bits 0.10 s, luma statistics 0.09 s, the rest less).

At 12 bits the kernels' int32 arithmetic follows the reference's scalar row at every coefficient magnitude (see the CPU tier's docstring for where its x86 row leaves it).
"""
import numpy as np
import pytest

import alf_extremes as X

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hip():
    from hip_backend import HipBackend
    return HipBackend()


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _same(got, exp, what):
    got = got.cpu().numpy() if hasattr(got, "cpu") else got
    assert np.array_equal(_bits(got), _bits(exp)), (what, "first differing entries", np.argwhere(_bits(got) != _bits(exp))[:4].tolist())


@pytest.mark.parametrize("bd", [8, 10, 12])
def test_classify_extreme_planes(hip, oracle, bd):
    """alfClassifyKernel on every plane (two-level patterns, low-amplitude planes on the exact ties, amplitude ramps through the activity clip), both shapes, the virtual
    boundary at (32, 28), (128, 124) and (8, 4) (every block row a boundary row: the 96 scale and the dropped row pair at the clip)"""
    hp = hip.hp
    for (h, w), _, _ in (X.LUMA_32, X.LUMA_128):
        for name, p in X.classify_planes(bd, h, w):
            d_p = hp.plane(p, 8)
            for vbh, vbp in X.CLASSIFY_VB:
                got = hp.alf_classify(d_p, bd, vbh, vbp).cpu().numpy()
                exp = oracle.alf_classify(p, bd, vbh, vbp)
                assert np.array_equal(got, exp), (bd, h, w, name, vbh, vbp, np.argwhere(got != exp)[:4].tolist())


@pytest.mark.parametrize("bd", [8, 10])
def test_stats_luma_extreme_planes(hip, oracle, bd):
    """alfBlockSumsKernel<0> + alfOrderedAddKernel<25, false / true>: the (org, rec) pattern pairs x the four class maps, a plain CTU and every unit / CTU pair on the
    72x104 plane (CTUs of 16 and 8 in units of 128: more steps than one CTU has block rows), continued chains started from records that are already >= 2^24"""
    hp = hip.hp
    (h, w), ctu, (vbh, vbp) = X.LUMA_32
    planes = X.stat_planes(bd, h, w)
    for o, r in X.STAT_PAIRS:
        org, rec = X.stat_pair(planes, o, r)
        d_org, d_rec = hp.plane(org, 0), hp.plane(rec, 8)
        derived = oracle.alf_classify(rec, bd, vbh, vbp)
        for kind in X.CLASS_MAPS:
            cm = X.class_map(kind, h, w, derived)
            d_cm = hp.to_device(cm)
            exp = oracle.alf_stats_plane(org, rec, ctu, 7, cm, vbh, vbp)
            first = hp.alf_stats_plane(d_org, d_rec, ctu, 7, d_cm, vbh, vbp)
            _same(first, exp, (bd, o, r, kind))
            # init = out = first: the chains go on from the records in place
            got = hp.alf_stats_plane(d_org, d_rec, ctu, 7, d_cm, vbh, vbp, init=first, out=first)
            _same(got, oracle.alf_stats_plane(org, rec, ctu, 7, cm, vbh, vbp, init=exp), (bd, o, r, kind, "continued"))
            for unit, c in X.UNIT_PAIRS:
                cmu = X.class_map(kind, h, w, oracle.alf_classify(rec, bd, c, c - 4) if kind == "derived" else None)
                got = hp.alf_stats_plane(d_org, d_rec, unit, 7, hp.to_device(cmu), c, c - 4, ctu_in_unit=c)
                _same(got, oracle.alf_stats_plane(org, rec, unit, 7, cmu, c, c - 4, ctu_in_unit=c), (bd, o, r, kind, unit, c))


@pytest.mark.parametrize("bd", [8, 10])
def test_stats_luma_full_ctu_128(hip, oracle, bd):
    """the 132x136 plane at CTU 128: all 32 lanes of a class row, slivers 8 wide and 4 high; one class for all 1024 blocks of the CTU (the longest chain, class 24 =
    the last accumulator) and every class; units of 128 with CTUs of 16 / 8: 256 / 512 steps, the longest unit walk the entry point admits"""
    hp = hip.hp
    (h, w), ctu, (vbh, vbp) = X.LUMA_128
    planes = X.stat_planes(bd, h, w)
    for o, r in X.STAT_PAIRS:
        org, rec = X.stat_pair(planes, o, r)
        d_org, d_rec = hp.plane(org, 0), hp.plane(rec, 8)
        for kind in ("one", "every"):
            cm = X.class_map(kind, h, w)
            d_cm = hp.to_device(cm)
            exp = oracle.alf_stats_plane(org, rec, ctu, 7, cm, vbh, vbp)
            first = hp.alf_stats_plane(d_org, d_rec, ctu, 7, d_cm, vbh, vbp)
            _same(first, exp, (bd, o, r, kind))
            got = hp.alf_stats_plane(d_org, d_rec, ctu, 7, d_cm, vbh, vbp, init=first, out=first)
            _same(got, oracle.alf_stats_plane(org, rec, ctu, 7, cm, vbh, vbp, init=exp), (bd, o, r, kind, "continued"))
            for c in (16, 8):
                got = hp.alf_stats_plane(d_org, d_rec, 128, 7, d_cm, c, c - 4, ctu_in_unit=c)
                _same(got, oracle.alf_stats_plane(org, rec, 128, 7, cm, c, c - 4, ctu_in_unit=c), (bd, o, r, kind, "unit 128", c))


@pytest.mark.parametrize("bd", [8, 10])
def test_stats_chroma_extreme_planes(hip, oracle, bd):
    """chroma 5x5, alfOrderedAddKernel<1, false / true>: the same pattern pairs at the chroma shape (36x52, chroma CTU 16), plain, with units, continued chains"""
    hp = hip.hp
    (h, w), ctu, (vbh, vbp) = X.chroma_of(X.LUMA_32)
    planes = X.stat_planes(bd, h, w)
    for o, r in X.STAT_PAIRS:
        org, rec = X.stat_pair(planes, o, r)
        d_org, d_rec = hp.plane(org, 0), hp.plane(rec, 8)
        exp = oracle.alf_stats_plane(org, rec, ctu, 5, None, vbh, vbp)
        first = hp.alf_stats_plane(d_org, d_rec, ctu, 5, None, vbh, vbp)
        _same(first, exp, (bd, o, r))
        got = hp.alf_stats_plane(d_org, d_rec, ctu, 5, None, vbh, vbp, init=first, out=first)
        _same(got, oracle.alf_stats_plane(org, rec, ctu, 5, None, vbh, vbp, init=exp), (bd, o, r, "continued"))
        for unit, c in X.CHROMA_UNIT_PAIRS:
            got = hp.alf_stats_plane(d_org, d_rec, unit, 5, None, c, c - 2, ctu_in_unit=c)
            _same(got, oracle.alf_stats_plane(org, rec, unit, 5, None, c, c - 2, ctu_in_unit=c), (bd, o, r, unit, c))


@pytest.mark.parametrize("bd", [8, 10])
def test_ccalf_stats_extreme_planes(hip, oracle, bd):
    """alfBlockSumsKernel<1> + alfOrderedAddKernel<1, false>: org, ALF-filtered chroma and luma from the two-level patterns, partial (36x52) and whole (32x48) chroma
    CTUs, the boundary-free last CTU row in both, continued chains"""
    hp = hip.hp
    for setting in (X.LUMA_32, X.CCALF_LUMA):
        (h, w), ctu, (vbh, vbp) = setting
        cp = X.stat_planes(bd, h // 2, w // 2)
        for k, lk in enumerate(X.CCALF_LUMA_KINDS):
            luma = X.pattern(lk, bd, h, w, 3)
            d_luma = hp.plane(luma, 8)
            for o, r in (X.STAT_PAIRS[k], X.STAT_PAIRS[(k + 3) % 6]):
                org, slf = X.stat_pair(cp, o, r)
                d_org, d_slf = hp.plane(org, 0), hp.plane(slf, 0)
                exp = oracle.ccalf_stats_plane(org, slf, luma, ctu // 2, vbh, vbp)
                first = hp.ccalf_stats_plane(d_org, d_slf, d_luma, ctu // 2, vbh, vbp)
                _same(first, exp, (bd, h, w, lk, o, r))
                got = hp.ccalf_stats_plane(d_org, d_slf, d_luma, ctu // 2, vbh, vbp, init=first, out=first)
                _same(got, oracle.ccalf_stats_plane(org, slf, luma, ctu // 2, vbh, vbp, init=exp), (bd, h, w, lk, o, r, "continued"))


def _filter_to_odd_stride(hp, p, ctu, bd, fl, cf, cl, ctu_set, cm, vbh, vbp):
    """destination with an odd stride and a 2-byte aligned origin: the 16-bit store path"""
    import torch
    from vvenc_amd.hotpath import Plane
    h, w = p.shape
    dst = Plane(hp.device, w, h, 1, stride=w + 3)
    dst.storage[1:1 + h, 1:1 + w] = torch.from_numpy(p).to(hp.device)
    hp.alf_filter_plane(hp.plane(p, 4), dst, ctu, bd, fl, hp.to_device(cf), hp.to_device(cl) if cl is not None else None, hp.to_device(ctu_set),
                        hp.to_device(cm) if cm is not None else None, vbh, vbp)
    return dst.visible().cpu().numpy()


@pytest.mark.parametrize("bd", [8, 10, 12])
def test_filter_extreme_planes(hip, oracle, bd):
    """alfFilterKernel<7 / 5, linear / non-linear>: full-range coefficients (+127, -128, alternating, uniform: one set each, chosen per CTU, disabled CTUs mixed in), every
    clipping set, the `every` class map (25 classes x 4 transposes), the three shapes (36x264 crosses the 256-wide LDS tile), both store paths; at 12 bits also the
    sets with sum |c_k| <= 400"""
    hp = hip.hp
    for limit in ((None, 400) if bd == 12 else (None,)):
        for setting in (X.LUMA_32, X.LUMA_128, X.LUMA_WIDE):
            (h, w), ctu, (vbh, vbp) = setting
            nctu = -(-h // ctu) * -(-w // ctu)
            cm = X.class_map("every", h, w)
            cf = X.coeff_sets(25, 0, limit)
            ctu_set = X.ctu_sets(nctu, 4, h)
            for name, p in X.filter_planes(bd, h, w):
                for ck in X.CLIP_KINDS:
                    cl = X.clip_sets(ck, bd, 4, 25)
                    exp = oracle.alf_filter_plane(p, ctu, bd, 7, cf, cl, ctu_set, cm, None, vbh, vbp)
                    got = hip.alf_filter_plane(p, ctu, bd, 7, cf, cl, ctu_set, cm, None, vbh, vbp)
                    assert np.array_equal(got, exp), ("7x7", bd, limit, h, w, name, ck, np.argwhere(got != exp)[:4].tolist())
                    if ck == "idx0":                    # clipping values that never bite = the linear table entry
                        got = hip.alf_filter_plane(p, ctu, bd, 7, cf, cl, ctu_set, cm, None, vbh, vbp, linear_entry=True)
                        assert np.array_equal(got, exp), ("7x7 linear", bd, limit, h, w, name, np.argwhere(got != exp)[:4].tolist())
                    if ck in ("idx0", "mixed"):
                        got = _filter_to_odd_stride(hp, p, ctu, bd, 7, cf, cl if ck == "mixed" else None, ctu_set, cm, vbh, vbp)
                        assert np.array_equal(got, exp), ("7x7 odd stride", bd, limit, h, w, name, ck)
            (hc, wc), ctu_c, (vbh_c, vbp_c) = X.chroma_of(setting)
            if hc % 4 or wc % 4:
                continue
            cf = X.coeff_sets(1, 1, limit)
            for name, p in X.filter_planes(bd, hc, wc):
                for ck in X.CLIP_KINDS:
                    cl = X.clip_sets(ck, bd, 4, 1)
                    exp = oracle.alf_filter_plane(p, ctu_c, bd, 5, cf, cl, ctu_set, None, None, vbh_c, vbp_c)
                    got = hip.alf_filter_plane(p, ctu_c, bd, 5, cf, cl, ctu_set, None, None, vbh_c, vbp_c)
                    assert np.array_equal(got, exp), ("5x5", bd, limit, hc, wc, name, ck, np.argwhere(got != exp)[:4].tolist())
                    if ck == "idx0":
                        got = hip.alf_filter_plane(p, ctu_c, bd, 5, cf, cl, ctu_set, None, None, vbh_c, vbp_c, linear_entry=True)
                        assert np.array_equal(got, exp), ("5x5 linear", bd, limit, hc, wc, name)
                    if ck in ("idx0", "mixed"):
                        got = _filter_to_odd_stride(hp, p, ctu_c, bd, 5, cf, cl if ck == "mixed" else None, ctu_set, None, vbh_c, vbp_c)
                        assert np.array_equal(got, exp), ("5x5 odd stride", bd, limit, hc, wc, name, ck)


@pytest.mark.parametrize("bd", [8, 10, 12])
def test_ccalf_filter_extreme_planes(hip, oracle, bd):
    """ccAlfFilterKernel: +-64 in every slot and random signed powers of two on two-level luma, chroma at 0 / maximum / mid (both ends of both clamps), a filter choice
    per CTU incl. off, and each of the strongest filters on every CTU"""
    mx, half = (1 << bd) - 1, 1 << (bd - 1)
    coeff = X.ccalf_coeffs()
    for setting in (X.LUMA_32, X.CCALF_LUMA):
        (h, w), ctu, (vbh, vbp) = setting
        nctu = -(-(h // 2) // (ctu // 2)) * -(-(w // 2) // (ctu // 2))
        ctu_filter = (np.arange(nctu) % 5).astype(np.uint8)
        for lk in X.CCALF_LUMA_KINDS:
            luma = X.pattern(lk, bd, h, w, 3)
            for level in (0, mx, half):
                chroma = np.full((h // 2, w // 2), level, np.int16)
                for flt in (ctu_filter, np.full(nctu, 1, np.uint8), np.full(nctu, 2, np.uint8), np.full(nctu, 4, np.uint8)):
                    exp = oracle.ccalf_filter_plane(chroma, luma, ctu // 2, bd, coeff, flt, vbh, vbp)
                    got = hip.ccalf_filter_plane(chroma, luma, ctu // 2, bd, coeff, flt, vbh, vbp)
                    assert np.array_equal(got, exp), (bd, h, w, lk, level, flt[:5].tolist(), np.argwhere(got != exp)[:4].tolist())
