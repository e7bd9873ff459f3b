"""Pins the oracle to the compiled reference (scalar row and x86 SIMD row, tolerance 0) on the extreme inputs of tests/interp_extremes.py, for everything the GPU tier
(tests/test_gpu_interp_extremes.py) asks the oracle: the one-pass table slots (8 / 6 / 4 / 2 taps, both directions, every first / last combination), the copy forms,
if_pred_luma (rnd 0 / 1, the alternative half-sample filter, the 4x4 rules), if_pred_luma_me (reduce_tap 0 / 1 / 2), the chroma composition of tests/pred_ref.py, the
prediction list's expected blocks and the distortion of the resulting blocks, at 8, 10 and 12 bits.

The scalar row is compared on every case.  The x86 row is compared on every case whose samples are in range and that it implements — interp_extremes.assert_no_wrap
derives that no pass leaves int16 there, so a saturating pack has nothing to change, and the rows agree wherever both exist, 12 bits included.  Six rules leave cases to
the scalar row alone; the last test of the file prints their counts (over the three bit depths):
  - one pass of width 5 (3576 slot cases): simdFilter (x86/InterpolationFilterX86.h:1583-1626) sends every odd width to its one-column routine, which writes column 0
    only; its 6-tap branch (:1561-1578) has no odd width but 1 at all, its 2-tap routine (:1435-1458) ends with four columns.  The encoder asks for width 1 and even widths.
    A width the x86 row does not have, not an arithmetic difference.
  - a 2-tap last pass (900 slot cases): simdInterpolateN2_10BIT_M4 refuses isLast (:1427); DMVR's bilinear passes are never last.
  - not-first inputs of 32767 / -32768, the set beyond the contract (1857 slot and copy cases): the scalar row's `Pel val` wraps where a saturating pack would not.
  - a plain copy (first == last) of 14-bit values (18 cases): fullPelCopy clips it to 0 .. max (:168-171, :229-232), the scalar row copies.  On samples the rows agree.
  - Hadamard at 12 bits (569 cases): xCalcHAD*_SSE refuses bit depths beyond 10 (x86/RdCostX86.h:659).
  - SSE at 12 bits of more than 2048 samples (40 cases, 64x64): xGetSSE_NxN_SIMD (:176-194) keeps eight 32-bit lanes over the whole block; a lane stays below 2^32 while
    w * h * 4095^2 / 8 does, that is up to 2048 samples.  On 64x64 of a plane against its complement it returns 26 826 246 208 for 35 416 180 800: 2^33 short.  The oracle and
    the kernels' 64-bit sums follow the scalar row.  At 10 bits 128x64 (8 573 165 568) the rows agree.

The guards are computed with the int64 model of interp_extremes, not read back from clipped outputs; the model itself is asserted equal to the oracle on every case it
is used on, so a mutation of the model that changes a compared sample (test_sensitivity) is an error a kernel would fail on.

Measured on a CPU host: 27 s for the file (both rows; the sensitivity test 3.4 s, every other case below 1.5 s).
"""
import numpy as np
import pytest

import interp_extremes as X
import pred_ref as PR

pytestmark = pytest.mark.ref

_x86_skipped = {}
BEYOND = "not-first input of 32767 / -32768"
ODD_WIDTH = "one pass of width 5"
BILINEAR_LAST = "2-tap last pass"
PLAIN_COPY = "plain copy of values outside 0 .. max"
HAD_12 = "Hadamard at 12 bits"
SSE_12 = "SSE at 12 bits of more than 2048 samples"


def _both(oracle, reflib, fn, what, x86=None):
    """fn(lib) from the oracle and from the reference row; x86 = the rule (a string) by which the x86 row is left out of this case, if any"""
    a = fn(oracle)
    if reflib.simd and x86:
        _x86_skipped[x86] = _x86_skipped.get(x86, 0) + 1
        return a
    b = fn(reflib)
    assert np.array_equal(a, b), (what, "simd" if reflib.simd else "scalar", np.argwhere(np.asarray(a) != np.asarray(b))[:4].tolist())
    return a


def test_tap_tables(oracle, reflib):
    """the tables restated in interp_extremes against the oracle's and the reference's own rows, every set and phase; and the derivation that no pass wraps int16"""
    for lib in (oracle, reflib):
        for set_ in (X.LUMA8, X.LUMA6, X.CHROMA4, X.ALT, X.BILINEAR):
            for p in [0] + list(X.phases(set_)):
                if set_ == X.ALT:
                    p = 8
                n, row = lib.if_coeff(set_, p)
                want = X.table_row(set_, p)
                assert n == X.ntaps(set_) and tuple(int(v) for v in row[:len(want)]) == tuple(want), (X.SET_NAMES[set_], p, row)
    f_hi, f_lo, s_hi, s_lo = X.assert_no_wrap()
    print("range guards: first pass %d .. %d, second pass (rnd 0) %d .. %d" % (f_lo, f_hi, s_lo, s_hi))


@pytest.mark.parametrize("bd", X.BITDEPTHS)
def test_slot_passes(oracle, reflib, bd):
    """if_filter on the slot cases.  Guards: a single last pass of every (set, phase, direction) with a negative tap has a compared sample whose unclipped value is
    above the maximum and one below 0; the first pass of every (set, phase, direction) reaches both analytic bounds exactly"""
    mx = (1 << bd) - 1
    over, under, top, bottom, n = {}, {}, {}, {}, 0
    for set_, p, vertical, first, last, name, pl, w, h, ok in X.slot_cases(bd):
        row, nt = X.table_row(set_, p), X.ntaps(set_)
        x, y = X.ORIGIN
        got = _both(oracle, reflib, lambda lib: lib.if_filter(nt, vertical, first, last, bd, (pl, y, x), w, h, row), ("slot", bd, X.SET_NAMES[set_], p, vertical, first, last, name, w, h),
                    BEYOND if not ok else ODD_WIDTH if w == 5 else BILINEAR_LAST if set_ == X.BILINEAR and last else None)
        c, lo = X.window(set_, p)
        tr = {}
        assert np.array_equal(got, X.one_pass(pl.astype(np.int64), y, x, w, h, c, lo, vertical, first, last, bd, tr=tr)), ("model", bd, set_, p, vertical, first, last, name)
        n += 1
        key = (set_, p, vertical)
        if first and last:
            over[key] = over.get(key, False) or bool((tr["raw"] > mx).any())
            under[key] = under.get(key, False) or bool((tr["raw"] < 0).any())
        if first and not last:
            top[key], bottom[key] = max(top.get(key, -1 << 40), int(tr["raw"].max())), min(bottom.get(key, 1 << 40), int(tr["raw"].min()))
    neg = [k for k in over if X.tap_sums(k[0], k[1])[1] < 0]
    print("slot guards, %d bits: %d cases; last pass above max and below 0 for %d of %d (set, phase, direction) with a negative tap; first pass at both bounds for %d"
          % (bd, n, sum(over[k] and under[k] for k in neg), len(neg), sum((top[k], bottom[k]) == X.first_pass_bounds(k[0], k[1], bd) for k in top)))
    assert neg and all(over[k] and under[k] for k in neg), [k for k in neg if not (over[k] and under[k])]
    assert top and all((top[k], bottom[k]) == X.first_pass_bounds(k[0], k[1], bd) for k in top), [k for k in top if (top[k], bottom[k]) != X.first_pass_bounds(k[0], k[1], bd)]
    assert len(top) == (2 * (15 + 15 + 31 + 1 + 15) if bd <= 10 else 2 * (15 + 15 + 31 + 1))


@pytest.mark.parametrize("bd", X.BITDEPTHS)
def test_copy_forms(oracle, reflib, bd):
    """if_copy in its four modes.  Guard: the last-not-first mode meets both clip ends on the reachable first-pass extremes"""
    mx = (1 << bd) - 1
    x, y = X.ORIGIN
    hi = lo = 0
    for first, last, bi, name, pl, w, h, ok in X.copy_cases(bd):
        got = _both(oracle, reflib, lambda lib: lib.if_copy(first, last, bd, (pl, y, x), w, h, bool(bi)), ("copy", bd, first, last, bi, name, w, h),
                    None if ok else PLAIN_COPY if first == last else BEYOND)
        tr = {}
        assert np.array_equal(got, X.copy_form(pl.astype(np.int64), y, x, w, h, first, last, bd, bool(bi), tr=tr)), ("model", bd, first, last, bi, name)
        if last and not first and ok:
            hi += int((tr["raw"] > mx).sum()); lo += int((tr["raw"] < 0).sum())
    print("copy guards, %d bits: last-not-first above max %d, below 0 %d" % (bd, hi, lo))
    assert hi > 0 and lo > 0


def _second_pass_guard(reached, fam, key, tr, rows, rnd, bd):
    """sample (0, 0) of a block at ORIGIN on a separable plane: the matched plane must give the analytic maximum of the second pass, the complement its minimum"""
    if key[0] != "sep" or "raw1" not in tr:
        return
    want = X.second_pass_bounds(rows[0], rows[1], rnd, bd)[1 if key[3] else 0]
    assert int(tr["raw2"][0, 0]) == want, (fam, key, rnd, bd, int(tr["raw2"][0, 0]), want)
    reached.add((fam, key[1], key[2], key[3]))


def _all_pairs(fam):
    """the pairs of signatures of two non-zero phases, matched and complement"""
    sigs = [s for s in X.family_sigs(fam) if s != X.SIG_ZERO]
    return {(fam, a, b, c) for a in sigs for b in sigs for c in (False, True)}


@pytest.mark.parametrize("bd", X.BITDEPTHS)
def test_luma_blocks(oracle, reflib, bd):
    """if_pred_luma (mode 0) and if_pred_luma_me (reduce_tap 1 / 2) on the batched luma blocks.  Guard: for every family (8-tap with the alternative row, 6-tap with
    the alternative row, 4-tap) and every pair of sign signatures the two-pass form reaches the separable plane's analytic second-pass maximum and minimum"""
    reached, n = set(), 0
    for w, h, mode, alt, rnd, fam, blocks in X.luma_groups(bd):
        at = X.atlas(bd, fam)
        a64 = at.arr.astype(np.int64)
        for key, x, y, xf, yf in blocks:
            yy = at.row(key) + y
            got = _both(oracle, reflib, lambda lib: X.luma_expected(lib, at.arr, yy, x, w, h, xf, yf, rnd, bd, alt, mode), ("luma", bd, w, h, mode, alt, rnd, key, x, y, xf, yf))
            tr = {}
            m = X.pred_luma(a64, yy, x, w, h, xf, yf, rnd, bd, alt, tr=tr) if mode == 0 else X.pred_luma_me(a64, yy, x, w, h, xf, yf, bd, alt, mode, tr=tr)
            assert np.array_equal(got, m), ("model", bd, w, h, mode, alt, rnd, key, xf, yf)
            n += 1
            if (x, y) == X.ORIGIN and xf and yf:
                if mode == 0:
                    rows = X.window(X.luma_set_pred(w, h, xf, True, alt), xf)[0], X.window(X.luma_set_pred(w, h, yf, True, alt), yf)[0]
                else:
                    rows = X.window(*X.luma_set_me(w, h + 7, xf, False, alt, mode))[0], X.window(*X.luma_set_me(w, h, yf, True, alt, mode))[0]
                _second_pass_guard(reached, fam, key, tr, rows, rnd, bd)
    want = _all_pairs("luma8") | _all_pairs("luma6") | _all_pairs("chroma4")
    print("luma guards, %d bits: %d blocks; second-pass maximum / minimum reached for %d of %d (family, signature pair, end)" % (bd, n, len(reached & want), len(want)))
    assert want <= reached, sorted(want - reached)[:4]


@pytest.mark.parametrize("bd", X.BITDEPTHS)
def test_chroma_blocks(oracle, reflib, bd):
    """the chroma composition of tests/pred_ref.py on the batched chroma blocks, all 32x32 phases at 8x8.  Guard: as for luma, every pair of chroma signatures"""
    reached, n = set(), 0
    at = X.atlas(bd, "chroma4")
    a64 = at.arr.astype(np.int64)
    for w, h, rnd, blocks in X.chroma_groups(bd):
        for key, x, y, xf, yf in blocks:
            yy = at.row(key) + y
            got = _both(oracle, reflib, lambda lib: PR.chroma_pred(lib, at.arr, yy, x, w, h, xf, yf, rnd, bd), ("chroma", bd, w, h, rnd, key, x, y, xf, yf))
            tr = {}
            assert np.array_equal(got, X.pred_chroma(a64, yy, x, w, h, xf, yf, rnd, bd, tr=tr)), ("model", bd, w, h, rnd, key, xf, yf)
            n += 1
            if (x, y) == X.ORIGIN and xf and yf:
                _second_pass_guard(reached, "chroma4", key, tr, (X.window(X.CHROMA4, xf)[0], X.window(X.CHROMA4, yf)[0]), rnd, bd)
    want = _all_pairs("chroma4")
    print("chroma guards, %d bits: %d blocks; second-pass maximum / minimum reached for %d of %d (signature pair, end)" % (bd, n, len(reached & want), len(want)))
    assert want <= reached, sorted(want - reached)[:4]


@pytest.mark.parametrize("bd", X.BITDEPTHS)
def test_distortion_of_clipped_predictions(oracle, reflib, bd):
    """SAD, SSE, HAD and HAD_fast of the clipped predictions against two-level originals.  Guard: expected SSEs beyond 2^32 at 12 bits 64x64 and at 10 bits 128x64"""
    org = X.org_atlas(bd)
    big = {}
    for w, h, mode, alt, items in X.dist_groups(bd):
        at = X.atlas(bd, X.LUMA_FAMILY[mode])
        for okey, rkey, xf, yf in items:
            x, y = X.ORIGIN
            pred = np.ascontiguousarray(_both(oracle, reflib, lambda lib: X.luma_expected(lib, at.arr, at.row(rkey) + y, x, w, h, xf, yf, 1, bd, alt, mode), ("dist pred", bd, w, h, mode, alt, rkey, xf, yf)))
            for func in X.DIST_FUNCS:
                d = _both(oracle, reflib, lambda lib: lib.dist(func, (org.arr, org.row(okey) + y, x), pred, w, h, bd, 0), ("dist", func, bd, w, h, mode, alt, okey, rkey, xf, yf),
                          HAD_12 if bd > 10 and func.startswith("HAD") else SSE_12 if bd > 10 and func == "SSE" and w * h > 2048 else None)
                if func == "SSE" and d > 1 << 32:
                    big[(w, h)] = big.get((w, h), 0) + 1
    print("distortion guards, %d bits: SSEs beyond 2^32 per size %s" % (bd, big))
    assert bd == 8 or big.get((64, 64) if bd == 12 else (128, 64), 0) > 0, big


@pytest.mark.parametrize("bd", X.BITDEPTHS)
def test_refinement_costs(oracle, reflib, bd):
    """what the GPU tier asks for the pattern refinement: if_pred_luma_me at the base vector plus each offset (base fractions 13 .. 15, offsets to +-16), then dist"""
    org = X.org_atlas(bd)
    x, y = X.ORIGIN
    for w, h, mode, alt, func, offs, bases in X.refine_groups(bd):
        at = X.atlas(bd, X.LUMA_FAMILY[mode])
        xy = [(x, org.row(ok) + y, x, at.row(rk) + y, fx, fy) for ok, rk, fx, fy in bases]
        preds = _both(oracle, reflib, lambda lib: X.refine_preds(lib, at.arr, w, h, mode, alt, offs, xy, bd), ("refine pred", bd, w, h, mode, alt, len(offs)))
        _both(oracle, reflib, lambda lib: X.refine_costs(lib, org.arr, preds, w, h, func, len(offs), xy, bd), ("refine cost", bd, w, h, mode, alt, func, len(offs)),
              HAD_12 if bd > 10 and func.startswith("HAD") else None)


@pytest.mark.parametrize("bd", X.BITDEPTHS)
def test_prediction_list_blocks(oracle, reflib, bd):
    """the expected blocks of the plain prediction list (tests/pred_ref.py: uni, bi with addAvg) from the oracle and from the reference.  Guard: addAvg meets both clip
    ends from two interpolated, non-constant 14-bit blocks"""
    mx = (1 << bd) - 1
    fams, ats = X.pred_planes(bd)
    planes = [a.arr for a in ats]
    a64 = [a.arr.astype(np.int64) for a in ats]
    it, pos, _ = X.pred_list_records(bd, [a.arr.shape[1] for a in ats])
    hi = lo = 0
    for k in range(it.size):
        got = _both(oracle, reflib, lambda lib: PR.expected_block(lib, planes, pos[k], it[k], bd), ("pred list", bd, k))
        w, h, chroma, alt = int(it[k]["width"]), int(it[k]["height"]), int(it[k]["chroma"]), int(it[k]["alt_hpel"])
        used = [l for l in (0, 1) if it[k]["ref_plane"][l] >= 0]
        blk = []
        for l in used:
            (x, y), (xf, yf), a = pos[k][l], (int(it[k]["frac"][l][0]), int(it[k]["frac"][l][1])), a64[int(it[k]["ref_plane"][l])]
            blk.append(X.pred_chroma(a, y, x, w, h, xf, yf, len(used) == 1, bd) if chroma else X.pred_luma(a, y, x, w, h, xf, yf, len(used) == 1, bd, alt))
        if len(used) == 2:
            tr = {}
            m = X.add_avg(blk[0], blk[1], bd, tr)
            if all(np.ptp(b) > 0 for b in blk) and (xf or yf):
                hi += int((tr["avg"] > mx).sum()); lo += int((tr["avg"] < 0).sum())
        else:
            m = blk[0]
        assert np.array_equal(got, m), ("model", bd, k)
    print("addAvg guards, %d bits: above max %d, below 0 %d (both inputs interpolated and non-constant)" % (bd, hi, lo))
    assert hi > 0 and lo > 0


MUTATION_CASES = {      # which luma groups (w, h, mode, alt, rnd) a mutation is looked for in
    "no_round": lambda w, h, mode, alt, rnd: (w, h, mode, alt, rnd) == (16, 16, 0, 0, 1),
    "no_upper_clip": lambda w, h, mode, alt, rnd: (w, h, mode, alt, rnd) == (16, 16, 0, 0, 1),
    "no_lower_clip": lambda w, h, mode, alt, rnd: (w, h, mode, alt, rnd) == (16, 16, 0, 0, 1),
    "no_mirror": lambda w, h, mode, alt, rnd: (w, h, mode, alt, rnd) == (16, 16, 0, 0, 1),
    "8tap_4x4": lambda w, h, mode, alt, rnd: (w, h, mode, alt) == (4, 4, 0, 0),
    "6tap_4x8": lambda w, h, mode, alt, rnd: (w, h, mode, alt) == (4, 8, 0, 0),
    "alt_both": lambda w, h, mode, alt, rnd: (w, h) != (4, 4) and mode == 0 and alt == 1,
    "no_alt_me": lambda w, h, mode, alt, rnd: mode > 0 and alt == 1,
    "chroma_not_doubled": lambda w, h, mode, alt, rnd: mode == 2 and alt == 0,
    "copy_no_bias": lambda w, h, mode, alt, rnd: (w, h, mode, alt) == (8, 8, 1, 0) or (w, h, mode, alt, rnd) == (8, 8, 0, 0, 0),
}


def test_sensitivity():
    """each mutation of the model — the rounding offset of the last pass dropped; the upper clip alone and the lower clip alone dropped; the tap row not mirrored above
    the half phase; the 8-tap set used for 4x4 and the 6-tap set for 4x8; the alternative row applied to both directions outside 4x4 and not applied at phase 8 inside
    the ME modes; the chroma phase not doubled in filter mode 2; the - 8192 bias dropped from a copy form — changes at least one compared sample of the luma blocks
    (which test_luma_blocks pins, sample by sample, to oracle, reference and the unmutated model): a kernel with that error fails the GPU tier"""
    assert set(MUTATION_CASES) == set(X.MUTATIONS)
    bd = 10
    changed = {}
    for mut, want in MUTATION_CASES.items():
        n = 0
        for w, h, mode, alt, rnd, fam, blocks in X.luma_groups(bd):
            if not want(w, h, mode, alt, rnd):
                continue
            at = X.atlas(bd, fam)
            a64 = at.arr.astype(np.int64)
            for key, x, y, xf, yf in blocks:
                yy = at.row(key) + y
                f = (lambda m: X.pred_luma(a64, yy, x, w, h, xf, yf, rnd, bd, alt, m)) if mode == 0 else (lambda m: X.pred_luma_me(a64, yy, x, w, h, xf, yf, bd, alt, mode, m))
                n += int((f((mut,)) != f(())).sum())
        changed[mut] = n
    print("sensitivity: compared samples changed per mutation %s" % changed)
    assert all(v > 0 for v in changed.values()), changed


def test_x86_row_skips_only_the_set_beyond_the_contract(reflib):
    """runs last in the file: the only cases the x86 row was not compared on are those of the rules of the module docstring"""
    print("cases compared with the scalar row only, by rule: %s" % _x86_skipped)
    most = {ODD_WIDTH: 3576, BEYOND: 1857, BILINEAR_LAST: 900, PLAIN_COPY: 18, HAD_12: 569, SSE_12: 40}          # the counts of a whole run of this file
    assert set(_x86_skipped) <= set(most) and all(n <= most[k] for k, n in _x86_skipped.items()), _x86_skipped
