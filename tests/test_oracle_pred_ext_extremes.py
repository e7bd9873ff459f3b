"""CPU tier of the limits tests of the picture-level prediction entries (BDOF, DMVR's padded reference, BCW, GEO, CIIP, affine with PROF) at 8, 10 and 12 bits.
Inputs, lists and the int64 model: tests/pred_ext_extremes.py.  The GPU tier (tests/test_gpu_pred_ext_extremes.py) runs the same lists on the device.

1. The models equal the reference's own functions on the new fixtures tests/golden/{bdof,blend,ciip,affine}_limits.npz (made by tests/limits_golden_gen.py with the four
   generators): bdof_ref.bdof_from_frames and the int64 model against xApplyBDOF, blend_ref.blend and the GEO weights against addWeightedAvg / xWeightedGeoBlk, the ciip_ref
   steps against xPredIntraPlanar / IntraPredSampleFilter / weightCiip, affine_ref against xPredAffineBlk; scalar row and x86 row.
   Rule-based exclusions from the x86 comparison: none.  The generators assert that the two rows agree on every blend and CIIP case; for BDOF and affine the rows are
   compared here, on every case (153 BDOF cases, 48 affine cases).
2. Guards, computed with the int64 model over the lists the GPU tier runs.  Reached on those lists (8 / 10 / 12 bits):
     BDOF units     frames +24958 / +25055 / +25079 and -25022 / -25072 / -25085 in both lists (the ring's range ends at 8128 / 8176 / 8188 and -8192);
                    |gradient| 518 / 519 / 519 (in-range frames: at most 255); |dI| 3123 / 3132 / 3135 (in-range: at most 1023); |b| 16185 / 16410 / 16425;
                    the value in front of the cast and the clip -263 .. 519 / -1055 .. 2083 / -4223 .. 8318; both clip ends act inside one unit in 103 units
     low-noise      every value of tmpx and of tmpy from -15 to 15; units where truncating the halving of a negative odd sSign * tmpx changes tmpy: 6 / 2 / 2
     DMVR + BDOF    frames +-12 0xx, |dI| 1068 / 1071 / 1072, in front of the clip -39 .. 297 / -158 .. 1191 / -630 .. 4766; both clip ends in 36 units
   "In-range" bounds: a frame of samples s in [ 0, 2^bd ) holds ( s << hr ) - 8192 in [ -8192, 8191 ]; ( f >> 6 ) is then in [ -128, 127 ] and a gradient in [ -255, 255 ],
   ( f >> 4 ) in [ -512, 511 ] and dI in [ -1023, 1023 ].
   What the issue asks for and geometry rules out (asserted here as such, with the reason):
     * the ring's own clamp under DMVR never acts: the ring spans refined - 1 + ( frac >= 8 ) .. refined + size + ( frac >= 8 ), the window start - 3 .. start + size + 3, and
       |refined - start| <= 2, so every ring sample lies inside the window.  The `ring_unclamped` mutation therefore changes no case (asserted on all lists).
     * a full swing between the clamped and the unclamped EXPECTATION is out of reach without BDOF: past the window lie the two outermost taps, |4| + |-1| of 64.  The
       guard is asserted on what the taps FETCH (the clamped and the unclamped sample differ by the full swing 2^bd - 1 for every moved list of every item) and on the
       expectations differing at all (every item); the count of items whose expectations differ by more than half the range (BDOF amplifies the few percent) is printed.
     * `15 - bd` as `hr + 1` and PROF's limit as `1 << 13` are the same numbers at every bit depth the entries accept (8 .. 12: hr = 14 - bd, max( bd + 1, 13 ) = 13):
       no list can tell them apart, asserted as equalities.
     * the (int16_t) cast of the output in front of the clip cannot act on frames that come from planes: the value stays below 2^15 (bound asserted in
       test_the_output_cast_cannot_act_on_frames_from_planes).  Only the recorded int16-noise frames of bdof.npz / bdof_limits.npz exercise it, on the models.
3. Model mutations (items changed at 8 / 10 / 12 bits, of 230 BDOF items): truncation in the tmpx shift 85 / 93 / 103, in the tmpy shift 103 / 127 / 132, the halving of
   sSign * tmpx dropped 175 / 175 / 175, tdi / tgx / tgy wrapped to 12 bits 45 / 45 / 45, the ring always one sample up and left 215 / 215 / 215, the offset clip at 14
   189 / 198 / 204, at 16 165 / 194 / 197; BCW's shift as hr + 2 and CIIP's weight as num_intra: more than half of their lists.  The mutations of the four points
   above (the cast dropped or behind the clip, hr + 1, the unclamped ring) change none; PROF's 1 << 13 is the same number.
"""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import affine_ref as AR  # noqa: E402
import bdof_ref as BR  # noqa: E402
import blend_ref as BL  # noqa: E402
import ciip_ref as CR  # noqa: E402
import interp_extremes as X  # noqa: E402
import pred_ext_extremes as E  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
LARGEST_OLD = os.path.getsize(os.path.join(GOLDEN, "ciip.npz"))


def _cases(name, keys):
    z = np.load(os.path.join(GOLDEN, name))
    return z, [dict(hdr=[int(v) for v in z["c%03d_hdr" % i]], **{k: z["c%03d_%s" % (i, k)] for k in keys}) for i in range(int(z["n"]))]


def _ext_lists(bd):
    return (("bdof", E.bdof_list(bd)), ("ramp", E.ramp_list(bd)), ("dmvr", E.dmvr_list(bd)))


# ---- 1. the models against the reference's own functions ---------------------------------------------------------------------------
def test_fixture_sizes():
    for f in ("bdof_limits.npz", "blend_limits.npz", "ciip_limits.npz", "affine_limits.npz"):
        assert os.path.getsize(os.path.join(GOLDEN, f)) <= LARGEST_OLD, f


def test_bdof_models_equal_the_fixture_on_both_rows():
    """bdof_ref.bdof_from_frames (the expectation of the GPU tier) and the int64 model == xApplyBDOF, scalar row and x86 row, on every case; the fixture holds 12-bit
    cases of every family of bdof.npz and, at all three bit depths, frames of the two-level planes beyond the ring's range in both lists"""
    _, cases = _cases("bdof_limits.npz", ("f0", "f1", "scalar", "simd"))
    seen = {}
    for i, c in enumerate(cases):
        bd, w, h = c["hdr"]
        got = BR.bdof_from_frames(c["f0"], c["f1"], bd)
        assert got.dtype == np.int16 and np.array_equal(got, c["scalar"]), ("bdof_ref", i, bd, w, h)
        assert np.array_equal(E.bdof_model(c["f0"], c["f1"], bd)["out"], c["scalar"]), ("int64 model", i, bd, w, h)
        assert np.array_equal(c["simd"], c["scalar"]), ("the reference's x86 row leaves its scalar row", i, bd, w, h)
        s = seen.setdefault(bd, dict(n=0, hi=[-1 << 20] * 2, lo=[1 << 20] * 2, shapes=set()))
        s["n"] += 1
        s["shapes"].add((w, h))
        for l, f in enumerate((c["f0"], c["f1"])):
            s["hi"][l], s["lo"][l] = max(s["hi"][l], int(f.max())), min(s["lo"][l], int(f.min()))
    assert set(seen) == set(E.BITDEPTHS) and seen[12]["n"] >= 60
    for bd, s in seen.items():
        top = (((1 << bd) - 1) << X.headroom(bd)) - 8192
        assert s["shapes"] == set(E.UNIT_SHAPES) and min(s["hi"]) > 3 * top and max(s["lo"]) < -3 * 8192, (bd, s)


def test_blend_model_equals_the_fixture():
    z, cases = _cases("blend_limits.npz", ("s0", "s1", "scalar", "simd"))
    import limits_golden_gen as G
    at = 0
    for (sd, w, h, c) in G.weight_blocks():
        n = (w >> c) * (h >> c)
        for row in ("weights_scalar", "weights_simd"):
            assert np.array_equal(BL.geo_weights(sd, w, h, c).reshape(-1), z[row][at:at + n]), (row, sd, w, h, c)
        at += n
    assert at == z["weights_scalar"].size
    kinds = set()
    for i, c in enumerate(cases):
        kind, bd, w, h, chroma, param = c["hdr"]
        assert bd == 12
        got = BL.blend(c["s0"], c["s1"], kind, param, bd, chroma)
        assert np.array_equal(got, c["scalar"]) and np.array_equal(got, c["simd"]), (i, c["hdr"])
        kinds.add((kind, chroma, int(got.min()) == 0, int(got.max()) == 4095))
    assert {k[:2] for k in kinds} == {(1, 0), (1, 1), (2, 0), (2, 1)} and any(k[2] and k[3] for k in kinds)


def test_ciip_model_equals_the_fixture():
    """(the generator asserts that the reference's two rows agree on every case; the file keeps one)"""
    _, cases = _cases("ciip_limits.npz", ("line", "inter", "intra", "result"))
    seen = set()
    for i, c in enumerate(cases):
        bd, w, h, chroma, ni = c["hdr"]
        assert bd == 12
        intra = CR.planar_intra(c["line"], w, h, chroma)
        assert np.array_equal(intra, c["intra"]), ("planar", i, c["hdr"])
        assert np.array_equal(CR.weight(c["inter"], intra, ni), c["result"]), ("weight", i, c["hdr"])
        seen |= {(w, h, chroma), ("ni", ni)}
    assert all(s in seen for s in E.CIIP_SIZES) and all(("ni", k) in seen for k in range(3))
    # every item of the list the GPU tier runs at 12 bits is in the file (of the 64x64 and 32x32 items every second one)
    pl, items, ext, blend, ciip, lines, pos = E.ciip_list(12)
    have = {(c["hdr"][1], c["hdr"][2], c["hdr"][3], c["hdr"][4], c["line"].tobytes(), c["inter"].tobytes()) for c in cases}
    n = 0
    for k, it in enumerate(items):
        w, h, o = int(it["width"]), int(it["height"]), int(ciip[k]["ref_off"])
        n += (w, h, int(it["chroma"]), int(ciip[k]["num_intra"]), lines[o:o + CR.line_len(w, h)].tobytes(), E.ciip_inter(pl, pos[k], it, blend[k], 12).tobytes()) in have
    assert n >= len(items) - 16, (n, len(items))


def _affine_rows():
    from oracle.oracle import Oracle, RefLib
    return [("oracle", Oracle(), "scalar")] + ([("ref-scalar", RefLib(0), "scalar"), ("ref-simd", RefLib(1), "simd")] if RefLib.available() else [])


@pytest.mark.parametrize("row", ["oracle", "ref-scalar", "ref-simd"])
def test_affine_model_equals_the_fixture(row):
    """affine_ref around the interpolation of the C restatement / of the compiled reference's two rows == what xPredAffineBlk of that row recorded at 12 bits, per list,
    luma and Cb; the recorded rows agree on every case; the cases reach dMv = +-31 and dI at its clip"""
    rows = {r[0]: r for r in _affine_rows()}
    if row not in rows:
        pytest.skip("oracle/_ref/libvvenc_ref.so not built (needs the reference sources)")
    _, lib, rec_row = rows[row]
    (pic_w, pic_h, ctu, _), planes, cases = E.affine_limits_cases()
    assert list(planes) == [12] and len(cases) == 48 and max(int(p.max()) for p in planes[12]) == 4095
    n_dmv = 0
    for k, (bd, lu, ch, pos, rec) in enumerate(cases):
        assert bd == 12
        for key in rec["scalar"]:
            assert np.array_equal(rec["scalar"][key], rec["simd"][key]), ("the reference's x86 row leaves its scalar row", k, key)
        for it, cc in ((lu, 0), (ch, 1)):
            for l in (0, 1):
                if it["ref_plane"][l] < 0:
                    continue
                got = AR.list_block(lib, planes[bd], pos[cc], it, l, bd, pic_w, pic_h, ctu)
                assert np.array_equal(got, rec[rec_row][(l, cc)]), (k, cc, l, lu)
                m = AR.ListModel(lu, l)
                n_dmv += bool(cc == 0 and m.prof and max(np.abs(m.dmx).max(), np.abs(m.dmy).max()) == 31)
    assert n_dmv >= 8


@pytest.mark.ref
@pytest.mark.parametrize("bd", E.BITDEPTHS)
def test_rows_agree_on_the_extension_lists(oracle, bd):
    """the expected values of the three extension lists from the C restatement, the reference's scalar row and its x86 row"""
    from oracle.oracle import RefLib
    if not RefLib.available():
        pytest.skip("oracle/_ref/libvvenc_ref.so not built (needs the reference sources)")
    r0, r1 = RefLib(0), RefLib(1)
    pl = E.planes(bd)
    for name, (items, ext, pos) in _ext_lists(bd):
        for k, (it, e, p) in enumerate(zip(items, ext, pos)):
            a = BR.expected_block_ex(oracle, pl, p, it, e, bd)
            assert np.array_equal(a, BR.expected_block_ex(r0, pl, p, it, e, bd)) and np.array_equal(a, BR.expected_block_ex(r1, pl, p, it, e, bd)), (name, bd, k, it)


# ---- 2. guards -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bd", E.BITDEPTHS)
def test_int64_model_is_the_expectation_on_the_lists(oracle, bd):
    """what computes the guards == what the GPU tier expects (bdof_ref around the oracle's interpolation), on every item of the three lists; the lists keep the entry's
    margins"""
    pl = E.planes(bd)
    for name, (items, ext, pos) in _ext_lists(bd):
        E.check_margins(pl, items, ext, pos)
        for k, (it, e, p) in enumerate(zip(items, ext, pos)):
            assert np.array_equal(E.model_item(pl, p, it, e, bd), BR.expected_block_ex(oracle, pl, p, it, e, bd)), (name, bd, k, it, e)


def _stats(bd, name, lst):
    pl, top = E.planes(bd), (1 << bd) - 1
    items, ext, pos = lst
    s = dict(hi=[-1 << 20] * 2, lo=[1 << 20] * 2, g=0, di=0, b=0, raw=[1 << 20, -1 << 20], both=0, tx=set(), ty=set(), inexact=0, odd=0, tcx=0, tch=0, shapes=set(), units=0)
    for it, e, p in zip(items, ext, pos):
        if not int(e["flags"]) & BR.EXT_BDOF:
            continue
        det = []
        E.model_block(pl, p, it, e, bd, detail=det)
        for (u, m, f0, f1) in det:
            s["units"] += 1
            for l, f in enumerate((f0, f1)):
                s["hi"][l], s["lo"][l] = max(s["hi"][l], int(f.max())), min(s["lo"][l], int(f.min()))
            s["g"] = max(s["g"], int(np.abs(m["gx"]).max()), int(np.abs(m["gy"]).max()))
            s["di"], s["b"] = max(s["di"], int(np.abs(m["di"]).max())), max(s["b"], int(np.abs(m["b"]).max()))
            s["raw"] = [min(s["raw"][0], int(m["raw"].min())), max(s["raw"][1], int(m["raw"].max()))]
            s["both"] += bool(m["raw"].min() < 0 and m["raw"].max() > top)
            s["tx"] |= set(m["tmpx"].ravel().tolist())
            s["ty"] |= set(m["tmpy"].ravel().tolist())
            s["inexact"] += m["neg_inexact_x"]
            s["odd"] += m["neg_odd_cross"]
            s["tcx"] += m["trunc_changes_x"]
            s["tch"] += m["trunc_changes_half"]
            s["shapes"].add(u[2:])
    print("%d bit %-5s %3d units: frames max %s min %s |grad| %d |dI| %d |b| %d before the clip %s both clip ends in %d units; negative inexact 4 sDIX in %d, negative odd "
          "sSign tmpx in %d, truncation changes tmpx in %d, truncation of the halving changes tmpy in %d" % (bd, name, s["units"], s["hi"], s["lo"], s["g"], s["di"], s["b"], s["raw"], s["both"],
                                                                                                      s["inexact"], s["odd"], s["tcx"], s["tch"]))
    return s


@pytest.mark.parametrize("bd", E.BITDEPTHS)
def test_guards_bdof(bd):
    """each limit is reached, not approached: frames above ( max << hr ) - 8192 and below -8192 in list 0 and in list 1; |gradient| > 255 and |dI| > 1023 (what frames of
    in-range samples cannot exceed); both ends of the final clip inside one unit; tmpx and tmpy each at -15, -14, -1, 0, 1, 14, 15; a negative 4 sDIX the shift does not
    divide exactly and a negative odd sSign * tmpx; all three unit shapes and the cut of 32x16 and 64x64 into units"""
    top = (1 << bd) - 1
    ring_hi = (top << X.headroom(bd)) - 8192
    st = {name: _stats(bd, name, lst) for name, lst in _ext_lists(bd)}
    s = st["bdof"]
    for l in (0, 1):
        assert s["hi"][l] > ring_hi and s["lo"][l] < -8192, (bd, l, s["hi"], s["lo"])
        assert st["dmvr"]["hi"][l] > ring_hi and st["dmvr"]["lo"][l] < -8192
    assert s["g"] > 255 and s["di"] > 1023 and st["dmvr"]["di"] > 1023
    assert s["raw"][0] < 0 and s["raw"][1] > top and s["both"] > 0
    assert st["dmvr"]["raw"][0] < 0 and st["dmvr"]["raw"][1] > top and st["dmvr"]["both"] > 0
    assert s["shapes"] == set(E.UNIT_SHAPES) and st["dmvr"]["shapes"] == set(E.UNIT_SHAPES)
    items = E.bdof_list(bd)[0]
    assert {(32, 16), (64, 64)} <= {(int(i["width"]), int(i["height"])) for i in items} and s["units"] > len(items) + 30
    want = {-15, -14, -1, 0, 1, 14, 15}
    for name in ("bdof", "ramp"):
        assert want <= st[name]["tx"] and want <= st[name]["ty"], (bd, name)
        assert st[name]["inexact"] > 0 and st[name]["odd"] > 0 and st[name]["tcx"] > 0
    assert st["ramp"]["tch"] > 0          # a negative odd sSign * tmpx whose halving, truncated toward zero, gives another tmpy
    assert st["ramp"]["hi"][0] < ring_hi and st["ramp"]["lo"][0] > -8192          # the low-noise pictures stay in range: their job is the interior of the offsets
    assert {tuple(i["ref_plane"]) for i in items} >= {(E.SEP, E.SEP), (E.SEP, E.CMP), (E.CMP, E.SEP), (E.SEP, E.CHK), (E.CHK, E.SEP)}
    assert {(tuple(i["frac"][0]), tuple(i["frac"][1])) for i in items} == set(E.PHASES) and any(int(i["alt_hpel"]) for i in items)


@pytest.mark.parametrize("bd", E.BITDEPTHS)
def test_guards_padded_reference(bd):
    """every moved list of every item fetches, through the clamp, at least one sample that differs by the full swing from the sample the unclamped read would fetch
    (the clamped column / row carries the other level), and every item's clamped expectation differs from its unclamped one; luma deltas +-2 and +-1, chroma +-1, with
    and without BDOF; both ends of the final clip act in items without BDOF as well"""
    pl, top = E.planes(bd), (1 << bd) - 1
    items, ext, pos = E.dmvr_list(bd)
    big = lo = hi = 0
    deltas = set()
    for k, (it, e, p) in enumerate(zip(items, ext, pos)):
        assert E.clamp_swing(pl, p, it, e) == top, (bd, k)
        a, b = E.model_item(pl, p, it, e, bd), E.model_item(pl, p, it, e, bd, clamp=False)
        assert not np.array_equal(a, b), (bd, k, it, e)
        big += int(np.abs(a.astype(np.int64) - b).max()) > top // 2
        deltas.add((int(it["chroma"]), int(e["flags"]) & 1, int(e["pad_dx"][0]), int(e["pad_dy"][0])))
        if not int(e["flags"]) & BR.EXT_BDOF:
            tr = {}
            E.model_plain(pl, p, it, e, bd, tr=tr)
            lo, hi = lo + bool(tr["avg"].min() < 0), hi + bool(tr["avg"].max() > top)
    print("%d bit: %d padded-reference items, %d of them differ from the unclamped expectation by more than half the range; the default average clips below in %d, above in %d"
          % (bd, len(items), big, lo, hi))
    assert lo > 0 and hi > 0
    for d in ((2, 0), (-2, 0), (0, 2), (0, -2)):
        assert (0, 0) + d in deltas and (0, 1) + d in deltas
    for d in ((1, 0), (-1, 0), (0, 1), (0, -1)):
        assert (1, 0) + d in deltas


@pytest.mark.parametrize("bd", E.BITDEPTHS)
def test_guards_blend_and_ciip(bd):
    """BCW / GEO: both clip ends act and a weight of -2 / 10 meets them; CIIP: both ends of the clip of the inter part act (uni, bi and BCW), every line kind, every
    num_intra against every kind of inter part, and the weighting moves the result"""
    top = (1 << bd) - 1
    pl, items, ext, blend, pos = E.blend_list(bd)
    lo = hi = 0
    for it, bl, p in zip(items, blend, pos):
        s0, s1 = E.hypotheses14(pl, p, it, bd)
        raw, out = E.blend_mut(s0, s1, int(bl["mode"]), int(bl["param"]), bd, int(it["chroma"]))
        lo, hi = lo + bool(raw.min() < 0), hi + bool(raw.max() > top)
    assert lo > 20 and hi > 20, (lo, hi)
    pl, items, ext, blend, ciip, lines, pos = E.ciip_list(bd)
    ends, combos, moved = set(), set(), 0
    for k, it in enumerate(items):
        tr = {}
        inter = E.ciip_inter(pl, pos[k], it, blend[k], bd, tr)
        kind = (int(it["ref_plane"][0]) >= 0) + (int(it["ref_plane"][1]) >= 0) + int(blend[k]["mode"])
        if tr["raw"].min() < 0:
            ends.add((kind, "lo"))
        if tr["raw"].max() > top:
            ends.add((kind, "hi"))
        combos.add((kind, int(blend[k]["param"]), int(ciip[k]["num_intra"])))
        w, h, o = int(it["width"]), int(it["height"]), int(ciip[k]["ref_off"])
        moved += not np.array_equal(CR.ciip(inter, lines[o:o + CR.line_len(w, h)], int(it["chroma"]), int(ciip[k]["num_intra"])), inter)
    assert ends == {(k, e) for k in (1, 2, 3) for e in ("lo", "hi")}, ends
    assert len(combos) == 12 and moved > len(items) * 3 // 4, (sorted(combos), moved)
    assert {(int(i["width"]), int(i["height"]), int(i["chroma"])) for i in items} == set(E.CIIP_SIZES)


def _prof_hits(world, items, pos, bd, mutated=False):
    """(sub-lists with |dMv| = 31, lists whose dI meets its clip) over the luma items"""
    hr, lim = X.headroom(bd), E.prof_limit(bd, mutated)
    hit_dmv = hit_di = 0
    for k in range(len(items)):
        it = items[k]
        if int(it["chroma"]):
            continue
        for l in (0, 1):
            if it["ref_plane"][l] < 0:
                continue
            m = AR.ListModel(it, l)
            if not m.prof:
                continue
            hit_dmv += int(np.abs(m.dmx).max() == 31 or np.abs(m.dmy).max() == 31)
            vec = AR.sub_vectors(it, m, world.pic_w, world.pic_h, world.ctu)
            arr, (x0, y0) = world.np[int(it["ref_plane"][l])], pos[k][l]
            hit = False
            for sy in range(vec.shape[0]):
                for sx in range(vec.shape[1]):
                    xi, yi, xf, yf = (int(v) for v in vec[sy, sx])
                    x, y = x0 + 4 * sx + xi, y0 + 4 * sy + yi
                    fr = (arr[y + (yf >> 3) - 1:y + (yf >> 3) + 5, x + (xf >> 3) - 1:x + (xf >> 3) + 5].astype(np.int64) << hr) - 8192
                    fr[1:5, 1:5] = X.pred_luma(arr, y, x, 4, 4, xf, yf, False, bd)
                    raw = m.dmx * ((fr[1:5, 2:6] >> 6) - (fr[1:5, 0:4] >> 6)) + m.dmy * ((fr[2:6, 1:5] >> 6) - (fr[0:4, 1:5] >> 6))
                    hit = hit or raw.max() > lim - 1 or raw.min() < -lim
            hit_di += int(hit)
    return hit_dmv, hit_di


def test_guard_prof_at_12_bits():
    """what affine_cases.extreme_list promises at 8 and 10 bits holds at 12: dMv at +-31 and, on the checkerboard, dI in its clip.  The clip is 1 << max( bd + 1, 13 ):
    1 << 13 at every bit depth the entry accepts, so 12 bits cannot tell a kernel that hard-codes 13 (asserted as an equality of the two limits)"""
    for ctu in (32, 128):
        world, lists = E.affine_lists(12, ctu, "checker")
        name, items, pos = lists[0]
        hit_dmv, hit_di = _prof_hits(world, items, pos, 12)
        print("12 bit, CTU %d, checkerboard: %d lists with |dMv| = 31, %d with dI in its clip" % (ctu, hit_dmv, hit_di))
        assert hit_dmv >= 10 and hit_di >= 3, (ctu, hit_dmv, hit_di)
    assert all(E.prof_limit(bd) == E.prof_limit(bd, True) == 8192 for bd in range(8, 13)) and E.prof_limit(13) != E.prof_limit(13, True)


# ---- 3. mutations ----------------------------------------------------------------------------------------------------------------------
INVISIBLE = {"sn_hr1": "15 - bd == max( 2, 14 - bd ) + 1 for bd <= 12", "ring_unclamped": "every ring sample lies inside the clamp window (|delta| <= 2, window reach 3)",
             "no_cast": "the value in front of the cast stays inside int16 for every frame a plane can produce (test_the_output_cast_cannot_act_on_frames_from_planes)",
             "cast_after_clip": "as no_cast"}


def test_the_output_cast_cannot_act_on_frames_from_planes():
    """the (int16_t) in front of the final clip: with |s| <= 25 100 (interp_extremes.assert_no_wrap: the second pass with rnd 0), |gradient| <= ( 25100 + 25100 ) >> 6 + 1
    and |tmp| <= 15, ( s0 + s1 + b + offset ) >> ( 15 - bd ) stays below 2^15 at every bit depth of 8 .. 12 — only the recorded int16-noise frames of the fixtures reach
    the cast, and no plane produces them"""
    _, _, s_hi, s_lo = X.assert_no_wrap()
    s = max(s_hi, -s_lo)
    g = ((2 * s) >> 6) + 1
    for bd in range(8, 13):
        sn = 15 - bd
        assert (2 * s + 15 * 4 * g + (1 << (sn - 1)) + 2 * 8192) >> sn < 32768 and (-2 * s - 15 * 4 * g) >> sn >= -32768, bd


def test_model_mutations_change_the_lists():
    """every mutation of the BDOF model changes the expected output of at least one item of the lists the GPU tier runs, at every bit depth it can (the two offset shifts
    as truncations, the halving dropped, 12-bit tdi / tgx / tgy, the int16 cast dropped or behind the clip, the ring one sample off, the offset clip at 14 or 16) —
    except those that arithmetic or geometry makes invisible (INVISIBLE), which change none"""
    table = {}
    for bd in E.BITDEPTHS:
        pl = E.planes(bd)
        for name, (items, ext, pos) in _ext_lists(bd):
            for it, e, p in zip(items, ext, pos):
                if not int(e["flags"]) & BR.EXT_BDOF:
                    continue
                base = E.model_block(pl, p, it, e, bd)
                for mut in E.MUTATIONS:
                    table.setdefault((mut, bd), 0)
                    table[(mut, bd)] += not np.array_equal(E.model_block(pl, p, it, e, bd, (mut,)), base)
    for mut in E.MUTATIONS:
        print("%-16s changes %s items at 8 / 10 / 12 bits" % (mut, [table[(mut, bd)] for bd in E.BITDEPTHS]))
        for bd in E.BITDEPTHS:
            assert (table[(mut, bd)] == 0) == (mut in INVISIBLE), (mut, bd, table[(mut, bd)])


@pytest.mark.parametrize("bd", E.BITDEPTHS)
def test_blend_and_ciip_mutations_change_the_lists(bd):
    """BCW's / GEO's shift as hr + 2 and CIIP's weight as num_intra change items of the lists"""
    pl, items, ext, blend, pos = E.blend_list(bd)
    n = 0
    for it, bl, p in zip(items, blend, pos):
        s0, s1 = E.hypotheses14(pl, p, it, bd)
        good = E.blend_mut(s0, s1, int(bl["mode"]), int(bl["param"]), bd, int(it["chroma"]))[1]
        assert np.array_equal(good, BL.blend(s0.astype(np.int16), s1.astype(np.int16), int(bl["mode"]), int(bl["param"]), bd, int(it["chroma"])))
        n += not np.array_equal(good, E.blend_mut(s0, s1, int(bl["mode"]), int(bl["param"]), bd, int(it["chroma"]), shift_less=1)[1])
    assert n > len(items) // 2, n
    pl, items, ext, blend, ciip, lines, pos = E.ciip_list(bd)
    n = 0
    for k, it in enumerate(items):
        w, h, o = int(it["width"]), int(it["height"]), int(ciip[k]["ref_off"])
        inter = E.ciip_inter(pl, pos[k], it, blend[k], bd)
        intra = CR.planar_intra(lines[o:o + CR.line_len(w, h)], w, h, int(it["chroma"]))
        good = E.ciip_weight_mut(inter, intra, int(ciip[k]["num_intra"]))
        assert np.array_equal(good, CR.weight(inter, intra, int(ciip[k]["num_intra"])))
        n += not np.array_equal(good, E.ciip_weight_mut(inter, intra, int(ciip[k]["num_intra"]), plus_one=False))
    assert n > len(items) // 2, n
