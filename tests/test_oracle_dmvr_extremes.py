"""Pins the oracle to the compiled reference (scalar row and x86 row, tolerance 0) on the extreme inputs of tests/dmvr_extremes.py, for everything the GPU tier
(tests/test_gpu_dmvr_extremes.py) asks the oracle: dmvr_refine on every family at 8, 9 and 10 bits and all four sub-block sizes, sad_x5 on every X5 case, dist("SAD")
on every surface geometry.  The int64 model of dmvr_extremes is asserted equal to the oracle on every case; the guards are computed from it and the sensitivity test
mutates it.  Only the tests that call the compiled reference carry the `ref` mark.

Where the x86 row is left out (the last test prints the counts of a whole run):
  - sad_x5 with rows * (2^bits - 1) > 32767 (dmvr_extremes.x5_rows_agree): xGetSADX5_8xN_SIMD / 16xN (x86/RdCostX86.h) keep a column pair's sum over the rows in a signed
    16-bit lane.  test_x5_operand_range finds the bound: at DMVR's own heights (16 rows, every second one) both rows agree up to 12-bit operands and differ at 13.
  - sad_x5 at width 16 with sub_shift 0 or height 4: the 16-wide x86 routine takes every second row whatever sub_shift says (it returns the sub_shift-1 value) and eight
    rows per trip (height 4: all zero).  DMVR calls it with sub_shift 1 and heights 8 and 16 only.
  - the full-range surface planes (-32768 / 32767): the x86 SAD takes differences in 16-bit lanes, where 65535 wraps to 1; the oracle is pinned to the int64 model there (the scalar row is
    compared as everywhere).
Bit depth 9: oracle == both reference rows on every family, so the tiers keep it.

Measured on a CPU host: 17 s for the file with both reference rows (the sensitivity test 3 s, the model comparisons 2 s per bit depth, every other test below 2 s).
"""
import numpy as np
import pytest

import dmvr_extremes as D

_x86_skipped = {}
X5_LANES = "sad_x5: rows * operand range beyond a signed 16-bit lane"
X5_WIDE = "sad_x5 16 wide with sub_shift 0 or height 4"
FULL_RANGE = "surface on -32768 / 32767"

_cache = {}


def _expected(oracle, fam):
    key = (fam.name, fam.bd, fam.dx, fam.dy)
    if key not in _cache:
        _cache[key] = [tuple(e) for e in fam.expected(oracle)]
    return _cache[key]


def _all_families():
    for bd in D.BITDEPTHS:
        for dx, dy in D.SIZES:
            for fam in D.families(bd, dx, dy):
                yield fam


# ---- DMVR ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.ref
@pytest.mark.parametrize("bd", D.BITDEPTHS)
def test_dmvr_oracle_equals_reference(oracle, reflib, bd):
    """oracle.dmvr_refine == the reference's pieces (filterN2_2D, distFunc, dmvrSadX5, xSubPelErrorSrfc) on every family, size and bit depth — 9 included; the layout
    family also without its sentinels: neither depends on a sample outside the reference's own footprint"""
    n = 0
    for dx, dy in D.SIZES:
        for fam in D.families(bd, dx, dy):
            exp = _expected(oracle, fam)
            got = [tuple(e) for e in fam.expected(reflib)]
            assert got == exp, (fam.name, bd, dx, dy, [(k, got[k], exp[k]) for k in range(len(exp)) if got[k] != exp[k]][:4])
            n += len(exp)
        plain = D.layout(bd, dx, dy, False)
        assert [tuple(e) for e in plain.expected(reflib)] == _expected(oracle, D.layout(bd, dx, dy)), ("layout without sentinels", bd, dx, dy)
    print("DMVR, %d bits: %d sub-blocks compared with the %s row" % (bd, n, "x86" if reflib.simd else "scalar"))


@pytest.mark.parametrize("bd", D.BITDEPTHS)
def test_dmvr_model_equals_oracle(oracle, bd):
    for dx, dy in D.SIZES:
        for fam in D.families(bd, dx, dy):
            exp, got = _expected(oracle, fam), fam.model()
            assert got == exp, (fam.name, bd, dx, dy, [(k, got[k], exp[k]) for k in range(len(exp)) if got[k] != exp[k]][:4])


def test_saturated_guards(oracle):
    """per size: a case whose min_cost is the largest the size allows — (dx * dy / 2) * 1023 less the centre's quarter; at 16x16 a case whose 25 costs are all >= 2^16"""
    for dx, dy in D.SIZES:
        fam = D.saturated(10, dx, dy)
        exp = _expected(oracle, fam)
        c = D.max_cost(dx, dy)
        top = [k for k, e in enumerate(exp) if e[2] == c - (c >> 2)]
        assert top, (dx, dy)
        tr = []
        fam.model(traces=tr)
        big = [k for k, t in enumerate(tr) if t["searched"] and min(t["costs"]) >= 1 << 16]
        print("saturated %dx%d: %d cases at the largest min_cost %d, %d with all 25 costs >= 2^16, largest cost %d" % (dx, dy, len(top), c - (c >> 2), len(big), max(max(t["costs"]) for t in tr)))
        assert max(max(t["costs"]) for t in tr) == c
        assert (dx, dy) != (16, 16) or big
        for bd in (8, 9):                     # the same planes at 8 and 9 bits: 255 << 2 and 511 << 1
            c2 = (dx * dy // 2) * (((1 << bd) - 1) << (10 - bd))
            assert any(e[2] == c2 - (c2 >> 2) for e in _expected(oracle, D.saturated(bd, dx, dy))), (bd, dx, dy)


def test_threshold_guards(oracle):
    """below dx * dy the result is (0, 0, centre); at and above it the search moves — to (-32, -32) with cost 0, the first position that misses the raised row"""
    for dx, dy in D.SIZES:
        fam = D.threshold(dx, dy)
        n = dx * dy
        assert [t[0] for t in fam.tags] == [n - 1, n, n + 1]
        assert (dx, dy) != (16, 16) or [t[1] for t in fam.tags] == [340, 341, 342]
        exp = _expected(oracle, fam)
        print("threshold %dx%d: raw sums %s -> %s" % (dx, dy, [t[1] for t in fam.tags], exp))
        assert exp == [(0, 0, n - 1), (-32, -32, 0), (-32, -32, 0)], (dx, dy, exp)


def test_surface_guards(oracle):
    """per size at 10 bits, from the model's traces of the selected draws: per axis every quotient -7 .. 7, +8 at and off the centre, -8, a zero denominator; each of the
    25 positions wins, and the oracle's mvd of a border winner is 16 * position (no surface there)"""
    for dx, dy in D.SIZES:
        fam = D.surface(10, dx, dy)
        exp = _expected(oracle, fam)
        tr = []
        fam.model(traces=tr)
        seen, border = set(), set()
        for k, t in enumerate(tr):
            cl = D.trace_classes(t)
            assert cl is not None and set(cl) == set(D.surface_classes(*D.surface_profiles(dx, dy, *fam.tags[k]), dx, dy)), (dx, dy, k)
            seen |= set(cl)
            h, v = t["winner"]
            if abs(h) == 2 or abs(v) == 2:
                assert exp[k][:2] == (16 * h, 16 * v), (dx, dy, k, exp[k])
                border.add((h, v))
        print("surface %dx%d: %d draws, %d classes of %d, %d border winners" % (dx, dy, len(fam), len(seen & D.surface_wanted()), len(D.surface_wanted()), len(border)))
        assert D.surface_wanted() <= seen, sorted(D.surface_wanted() - seen)
        assert len(border) == 16


def test_tie_pair_guards(oracle):
    """exactly the two positions of a pair have the smallest cost, and the oracle takes the one that is first in the raster order"""
    for bd in D.BITDEPTHS:
        for dx, dy in D.SIZES:
            fam = D.tie_pairs(bd, dx, dy)
            tr = []
            fam.model(traces=tr)
            for k, (t, pair) in enumerate(zip(tr, fam.tags)):
                low = {(i % 5 - 2, i // 5 - 2) for i, c in enumerate(t["costs"]) if c == min(t["costs"])}
                assert t["searched"] and low == set(pair) and t["winner"] == pair[0], (bd, dx, dy, k, low, t["winner"])
                e = _expected(oracle, fam)[k]
                assert ((e[0] + 8) // 16, (e[1] + 8) // 16, e[2]) == pair[0] + (0,) or abs(pair[0][0]) == 2, (bd, dx, dy, k, e)


def test_phase_guards():
    """all 256 fractions of either list and all 16 pairs of code paths, at every size and bit depth"""
    for bd in D.BITDEPTHS:
        for dx, dy in D.SIZES:
            it = D.phases(bd, dx, dy).items
            assert len({(int(i["f0x"]), int(i["f0y"])) for i in it}) == 256 and len({(int(i["f1x"]), int(i["f1y"])) for i in it}) == 256
            assert len({(D.code_path(int(i["f0x"]), int(i["f0y"])), D.code_path(int(i["f1x"]), int(i["f1y"]))) for i in it}) == 16


def test_layout_guards(oracle):
    """the row pitches differ and neither is a power of two; every pair of column residues; the first item's loads start at sample 0 of both planes and the last item's
    end at their last sample; every sample of the kernel's footprint outside the reference's own is a sentinel; the oracle's result does not depend on the sentinels"""
    for bd in D.BITDEPTHS:
        for dx, dy in D.SIZES:
            fam, plain = D.layout(bd, dx, dy), D.layout(bd, dx, dy, False)
            w0, w1 = fam.ref0.shape[1], fam.ref1.shape[1]
            assert w0 != w1 and all(w & (w - 1) and w % 8 == 0 for w in (w0, w1))
            it = fam.items
            assert {(int(i["x0"]) % 8, int(i["x1"]) % 8) for i in it[:64]} == {(a, b) for a in range(8) for b in range(8)}
            r_lo, r_hi, c_lo, c_hi = D.kernel_footprint(dx, dy)
            n_sent = 0
            for l, a in ((0, fam.ref0), (1, fam.ref1)):
                x, y = it["x%d" % l], it["y%d" % l]
                assert (int(x[0]) + c_lo, int(y[0]) + r_lo) == (0, 0) and (int(x[64]) + c_hi, int(y[64]) + r_hi) == (a.shape[1] - 1, a.shape[0] - 1)
                for i in it:
                    fx, fy = (int(i["f0x"]), int(i["f0y"])) if l == 0 else (int(i["f1x"]), int(i["f1y"]))
                    q_lo, q_hi, d_lo, d_hi = D.reference_footprint(dx, dy, fx, fy)
                    xx, yy = int(i["x%d" % l]), int(i["y%d" % l])
                    k = a[yy + r_lo:yy + r_hi + 1, xx + c_lo:xx + c_hi + 1].astype(np.int64).copy()
                    assert k.shape == (r_hi - r_lo + 1, c_hi - c_lo + 1)
                    inner = k[q_lo - r_lo:q_hi - r_lo + 1, d_lo - c_lo:d_hi - c_lo + 1]
                    assert inner.min() >= 0 and inner.max() < 1 << bd
                    k[q_lo - r_lo:q_hi - r_lo + 1, d_lo - c_lo:d_hi - c_lo + 1] = D.SENTINELS[0]
                    assert np.isin(k, D.SENTINELS).all()
                    n_sent += k.size - inner.size
            assert _expected(oracle, fam) == [tuple(e) for e in plain.expected(oracle)], (bd, dx, dy)
    print("layout %dx%d: %d sentinel samples inside the kernel's footprint" % (dx, dy, n_sent))


def test_list_guards():
    """n = 0, one to five sub-blocks (a workgroup takes four), grids of 8 workgroups with a partial last one (31) and full (32), of 9 (one past the eight-way remap), of
    17 and of 65"""
    assert D.LIST_NS == (0, 1, 2, 3, 4, 5, 31, 32, 33, 35, 67, 259)
    grids = [(n + 3) // 4 for n in D.LIST_NS]
    assert any(n % 4 for n in D.LIST_NS) and any(g and g < 8 for g in grids) and any(g >= 8 and g % 8 == 0 for g in grids) and any(g > 8 and g % 8 for g in grids)
    sel = dict(D.list_selections())
    assert sorted(sel["shuffled"].tolist()) == list(range(259)) and len(set(sel["identical"].tolist())) == 1


def _mutated(fams, mut):
    """cases whose result the mutation changes"""
    n = 0
    for fam in fams:
        n += sum(a != b for a, b in zip(fam.model((mut,)), fam.model()))
    return n


def test_sensitivity():
    """each mutation of the model changes the result of at least one case (which test_dmvr_model_equals_oracle and the X5 test pin to the oracle): `<=` in the scan; no
    quarter reduction of the centre; `>` at the threshold; costs accumulated modulo 2^16; the first pass's rounding offset dropped at 8 bits; the second pass's shift
    taken from the first; odd rows instead of even ones; list 1 not mirrored; +-8 swapped; the surface applied on the border; column-major tie order; X5's cur - k
    turned into cur + k; X5's >> 1 dropped"""
    where = {
        "scan_le": [D.saturated(10, 16, 16)],
        "no_quarter": [D.threshold(8, 8), D.surface(10, 8, 16)],
        "thr_gt": [D.threshold(dx, dy) for dx, dy in D.SIZES],
        "cost_mod16": [D.saturated(10, 16, 16)],
        "no_round1_8": [D.phases(8, 16, 8)],
        "shift2_from_1": [D.phases(8, 8, 16), D.phases(9, 8, 8)],
        "odd_rows": [D.phases(10, 8, 8)],
        "no_mirror": [D.phases(10, 16, 16)],
        "pm8_swapped": [D.surface(10, 16, 16)],
        "surface_on_border": [D.surface(10, 16, 8)],
        "col_major_ties": [D.tie_pairs(10, 16, 16), D.tie_pairs(8, 8, 16)],
    }
    changed = {m: _mutated(f, m) for m, f in where.items()}
    thr = {(dx, dy): _mutated([D.threshold(dx, dy)], "thr_gt") for dx, dy in D.SIZES}
    assert all(v == 1 for v in thr.values()), thr          # exactly the case at equality, at every size
    org, cur = D.x5_planes()
    o64, c64 = org.astype(np.int64), cur.astype(np.int64)
    for m in ("x5_plus", "x5_no_shift"):
        n = 0
        for w, h, ss, cc, _, items in D.x5_cases():
            if h > 16:
                continue
            for (ox, oy, cx, cy, _) in items[:3]:
                if m == "x5_plus" and cx + 4 + w > D.X5_W:
                    continue
                n += D.x5_model(o64, oy, ox, c64, cy, cx, w, h, ss, cc, (m,)) != D.x5_model(o64, oy, ox, c64, cy, cx, w, h, ss, cc)
        changed[m] = n
    print("sensitivity: cases changed per mutation %s" % changed)
    assert set(changed) == set(D.MUTATIONS)
    assert all(v > 0 for v in changed.values()), changed


# ---- SAD-X5 -------------------------------------------------------------------------------------------------------------------------
_x5_cache = {}


def _x5_expected(oracle):
    if not _x5_cache:
        org, cur = D.x5_planes()
        for w, h, ss, cc, n, items in D.x5_cases():
            _x5_cache[(w, h, ss, cc, n)] = [oracle.sad_x5((org, oy, ox), (cur, cy, cx), w, h, ss, bool(cc)).tolist() for (ox, oy, cx, cy, _) in items]
    return _x5_cache


@pytest.mark.ref
def test_x5_oracle_equals_reference(oracle, reflib):
    """oracle.sad_x5 == xGetSAD8X5 / 16X5 on every case; the x86 row where dmvr_extremes.x5_rows_agree says it computes the same.  With calc_centre 0 both leave entry 2 as
    they found it (0 here)"""
    org, cur = D.x5_planes()
    exp = _x5_expected(oracle)
    n = 0
    for w, h, ss, cc, cnt, items in D.x5_cases():
        for k, (ox, oy, cx, cy, bits) in enumerate(items):
            if reflib.simd and not D.x5_rows_agree(w, h, ss, bits):
                rule = X5_WIDE if w == 16 and (ss == 0 or h < 8) else X5_LANES
                _x86_skipped[rule] = _x86_skipped.get(rule, 0) + 1
                continue
            got = reflib.sad_x5((org, oy, ox), (cur, cy, cx), w, h, ss, bool(cc)).tolist()
            assert got == exp[(w, h, ss, cc, cnt)][k], (w, h, ss, cc, cnt, k, bits, got, exp[(w, h, ss, cc, cnt)][k])
            assert cc or got[2] == 0
            n += 1
    print("SAD-X5: %d items compared with the %s row" % (n, "x86" if reflib.simd else "scalar"))
    assert n == 13000 if not reflib.simd else n > 3000


@pytest.mark.ref
def test_x5_operand_range(oracle, reflib):
    """finds the widest operands at which the two reference rows agree: a two-level checker of (0, 2^bits - 1) against its complement makes every difference the range.
    The scalar row equals the oracle at every width; the x86 row exactly where x5_rows_agree says — up to 12 bits at DMVR's heights"""
    widest = {}
    for bits in range(8, 16):
        mx = (1 << bits) - 1
        a = D.filler("checker", mx, 0, D.X5_H, D.X5_W)
        c = D._ro(mx - a.astype(np.int64))
        for w in (8, 16):
            for h in (4, 8, 16, 32, 128):
                for ss in (0, 1):
                    same = oracle.sad_x5((a, 2, 6), (c, 2, 6), w, h, ss, True).tolist() == reflib.sad_x5((a, 2, 6), (c, 2, 6), w, h, ss, True).tolist()
                    assert same == (not reflib.simd or D.x5_rows_agree(w, h, ss, bits)), (bits, w, h, ss, same)
                    if same and ss == 1 and h in (8, 16):
                        widest[(w, h)] = max(widest.get((w, h), 0), bits)
    print("SAD-X5 operand range, %s row: widest agreeing operand width per (w, h) at sub_shift 1: %s" % ("x86" if reflib.simd else "scalar", widest))
    assert min(widest.values()) == (12 if reflib.simd else 15)
    assert max(b for _, _, b in D.X5_SETS[:-1]) == 12 and D.X5_SETS[-1][2] == 15


def test_x5_model_and_guards(oracle):
    """the model equals the oracle on every case.  Guards: every team width 2 .. 64 occurs, each with a last workgroup that is partly empty and with 5 n teams that split
    an item over two workgroups; odd and even cur columns; cur - 4 at sample 0 and the org + 4 block's end at the last sample of the plane"""
    org, cur = D.x5_planes()
    o64, c64 = org.astype(np.int64), cur.astype(np.int64)
    exp = _x5_expected(oracle)
    lanes, partial, straddle, odd = set(), set(), set(), [0, 0]
    for w, h, ss, cc, n, items in D.x5_cases():
        for k, (ox, oy, cx, cy, _) in enumerate(items):
            m = D.x5_model(o64, oy, ox, c64, cy, cx, w, h, ss, cc)
            assert [0 if v is None else v for v in m] == exp[(w, h, ss, cc, n)][k], (w, h, ss, cc, n, k)
            odd[cx & 1] += 1
        assert items[0][2:4] == (4, 0) and (n == 1 or (items[1][0] + 4 + w, items[1][1] + h) == (org.shape[1], org.shape[0]))
        lp = D.x5_team_lanes(w, h, ss)
        lanes.add(lp)
        per_wg = 256 // lp
        if (5 * n) % per_wg:
            partial.add(lp)
        if per_wg % 5 and 5 * n > per_wg:
            straddle.add(lp)
    print("SAD-X5 guards: team widths %s, odd / even cur columns %s" % (sorted(lanes), odd))
    assert lanes == partial == straddle == {2, 4, 8, 16, 32, 64} and min(odd) > 1000


# ---- SAD surface --------------------------------------------------------------------------------------------------------------------
_surf_cache = {}


def _surf_expected(oracle, kind, g):
    if (kind, g) not in _surf_cache:
        _surf_cache[(kind, g)] = D.surf_expected(oracle, kind, *g)
    return _surf_cache[(kind, g)]


@pytest.mark.ref
def test_surface_oracle_equals_reference(oracle, reflib):
    """oracle.dist("SAD") == the reference's xGetSAD rows on every surface geometry and plane kind; on the full-range planes the scalar row only"""
    n = 0
    for kind in D.SURF_PLANES:
        for g in D.surf_geometries():
            if reflib.simd and kind == "full_range":
                _x86_skipped[FULL_RANGE] = _x86_skipped.get(FULL_RANGE, 0) + 1
                continue
            assert np.array_equal(D.surf_expected(reflib, kind, *g), _surf_expected(oracle, kind, g)), (kind, g)
            n += 1
    print("SAD surface: %d geometries compared with the %s row" % (n, "x86" if reflib.simd else "scalar"))


def test_surface_model_and_guards(oracle):
    """the model equals the oracle on every geometry — the full-range planes included, where it is what pins the oracle.  Guards: the four KDY instantiations; n_blocks = 1
    splits every geometry with more than one displacement-row group and 1025 blocks split none; a window between 64 KiB and 160 KiB of LDS for both; the refused
    geometry is beyond 160 KiB for both; a surface value >= 2^29; ranges 0 and rx != ry; windows that start at sample 0 and end at the last sample of the plane"""
    kdys, mid, top = set(), 0, 0
    for g in D.surf_geometries():
        w, h, ss, rx, ry = g
        kdy, splits1, lds1 = D.surface_launch(w, h, ss, rx, ry, 1)
        kdy2, splits2, lds2 = D.surface_launch(w, h, ss, rx, ry, 1025)
        assert kdy == kdy2 and splits2 == 1 and splits1 == (2 * ry + 1 + kdy - 1) // kdy and max(lds1, lds2) <= 160 * 1024
        kdys.add(kdy)
        mid += min(lds1, lds2) > 64 * 1024
        blocks = D.surf_blocks(w, h, rx, ry)
        assert blocks[0] == (rx, ry) and (blocks[1][0] + w + rx, blocks[1][1] + h + ry) == (D.SURF_W, D.SURF_H) and blocks[2][0] & 1
        for kind in D.SURF_PLANES:
            org, ref = D.surf_planes(kind)
            exp = _surf_expected(oracle, kind, g)
            o64, r64 = org.astype(np.int64), ref.astype(np.int64)
            for b, (x, y) in enumerate(blocks):
                assert np.array_equal(D.surface_model(o64, y, x, r64, y, x, w, h, ss, rx, ry), exp[b]), (kind, g, b)
            top = max(top, int(exp.max()))
    w, h, ss, rx, ry = D.SURF_TOO_BIG
    assert min(D.surface_launch(w, h, ss, rx, ry, n)[2] for n in (1, 3, 1025)) > 160 * 1024
    print("surface guards: KDY %s, %d geometries between 64 KiB and 160 KiB, largest value %d" % (sorted(kdys), mid, top))
    assert kdys == {1, 2, 4, 8} and mid > 0 and 1 << 29 <= top < 1 << 32
    assert {(0, 0), (0, 5), (7, 0), (16, 3)} <= {(g[3], g[4]) for g in D.surf_geometries()} and {(2, 2), (4, 4), (8, 16), (64, 64), (128, 128)} <= {g[:2] for g in D.surf_geometries()}


@pytest.mark.ref
def test_x86_row_skips_only_by_the_rules(reflib):
    """runs last in the file: the only cases the x86 row was not compared on are those of the rules of the module docstring"""
    print("cases compared with the scalar row only, by rule: %s" % _x86_skipped)
    assert set(_x86_skipped) <= {X5_LANES, X5_WIDE, FULL_RANGE}, _x86_skipped
