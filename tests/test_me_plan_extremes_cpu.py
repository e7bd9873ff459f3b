"""CPU tier of the motion-search plan limits (tests/me_plan_extremes.py; the device tier is tests/test_gpu_me_plan_extremes.py).  No device.

  * every named edge of REQUIRED is reached by some plan — from schedule_model, the restatement of the host scheduler's counting rules, and for the few edges it cannot
    see (a pool as the originals' plane, a window at the first / last readable sample) from the builder;
  * the launch combinations of family C are the ones their names promise, and the windows next to the 6 KB / 24 KB caps lie on either side of them;
  * every evaluated stage position is within one sample of its block, every window row with the 18 bytes it is fetched beyond itself, every stage's neighbourhood and
    every item block lies inside its plane's storage;
  * sensitivity: window_model equals the oracle on every candidate of family A, and each of its four addressing mutations changes a cost of family A; the fifth
    mutation, the extent compared with < in the clustering, changes no cost by its nature but the number of windows of every plan of family A, which the device tier
    compares with vvhip_me_plan_info;
  * the environment knobs of family H each change the compact plan's schedule in the model (or, for the three that only reorder or regroup launches, are named as such);
  * the oracle equals the compiled reference (scalar row, x86 row) on family F's operand blocks and on family D's position sweep, where the reference is built.
"""
import numpy as np
import pytest

import me_plan_extremes as M


@pytest.fixture(scope="module")
def plans():
    return M.all_plans()


def test_every_required_edge_is_reached(plans):
    edges, by = set(), {}
    for p in plans + M.long_plans():
        e = p.model()["edges"] | p.edges
        assert e <= set(M.REQUIRED), (p.name, e - set(M.REQUIRED))
        for k in e:
            by.setdefault(k, p.name)
        edges |= e
    assert [k for k in M.REQUIRED if k not in edges] == []
    print("edges -> first plan that reaches it:", by)


def test_launch_combinations_are_what_their_names_say(plans):
    m = {p.name: p.model() for p in plans if p.name.startswith("C ")}
    for n in (1, 2, 3, 4, 5, 36, 37, 39):
        x = m["C %d small windows" % n]
        assert (x["n_small"], x["n_mid"], x["n_large"], x["int_launches"]) == (n, 0, 0, 1)
    cls = lambda x: (x["n_small"] > 0, x["n_mid"] > 0, x["n_large"] > 0)
    assert cls(m["C mid only"]) == (False, True, False) and cls(m["C large only"]) == (False, False, True) and m["C large only"]["lds_int"] > 64 * 1024
    assert cls(m["C small + mid"]) == (True, True, False) and m["C small + mid"]["int_launches"] == 1
    x = m["C small + large, split"]
    assert cls(x) == (True, False, True) and x["int_split"] and x["int_launches"] == 2
    x = m["C small + large, one launch"]
    assert cls(x) == (True, False, True) and not x["int_split"] and x["int_launches"] == 1
    x = m["C mid + large, split"]
    assert cls(x) == (False, True, True) and x["split_large"] and x["int_launches"] == 2
    x = m["C mid + large, one launch"]
    assert cls(x) == (False, True, True) and not x["split_large"] and x["int_launches"] == 1
    x = m["C three classes, both splits"]
    assert cls(x) == (True, True, True) and x["split_large"] and x["int_split"] and x["int_launches"] == 3
    x = m["C windows next to the 6 KB and 24 KB caps"]
    got = sorted(w["lds"] for row in x["windows"] for w in row)
    (lo6, _), (hi6, _) = M.closest_to_cap(6 * 1024)
    (lo24, _), (hi24, _) = M.closest_to_cap(24 * 1024)
    assert got == [lo6, hi6, lo24, hi24] and lo6 <= 6144 < hi6 and lo24 <= 24576 < hi24, got
    # as close as shapes and extents allow: the pitch moves in steps of 4 bytes per row, the rows in steps of the pitch
    assert 6144 - lo6 < 64 and hi6 - 6144 < 64 and 24576 - lo24 < 256 and hi24 - 24576 < 256, got
    x = m["C one workgroup of an 8x4 window next to 32x32 windows"]
    lds = sorted(w["lds"] for row in x["windows"] for w in row)
    assert x["n_small"] == 4 and lds[0] < 200 and lds[-1] > 4096, lds


def test_stage_schedule_is_what_the_cases_are_for(plans):
    m = {p.name: (p, p.model()) for p in plans}
    p, x = m["D tile kinds and deals, 10 bits"]
    deal = {}
    for s, st in zip(p.sj, x["stages"]):
        if int(s["mask"]) == 511:
            deal[(int(s["width"]), int(s["height"]))] = (st["units"], st["deal"], st["variants"])
    # (units, deal: 2 single / 0 shared by a workgroup's two waves / 1 atomic, horizontal variants as waves of their own)
    assert deal[(64, 32)] == (1, 2, 3) and deal[(64, 64)][:2] == (2, 0) and deal[(128, 32)][:2] == (2, 0)
    assert deal[(32, 128)][:2] == (4, 1) and deal[(128, 64)][:2] == (4, 1) and deal[(128, 128)] == (8, 1, 3)      # 24 waves add into one stage
    for (w, h) in ((8, 4), (4, 8), (4, 32), (16, 8), (8, 16), (16, 16), (32, 32)):
        assert deal[(w, h)][:2] == (1, 2)
    for bd in (10, 8):
        for n, waves in ((7, 1), (8, 1), (9, 2), (17, 3)):
            assert m["D %d equal 8x4 units, %d bits" % (n, bd)][1]["waves_stage"] == waves
        for work, waves in ((76, 1), (80, 1), (84, 2)):
            assert m["D bundle of %d row groups, %d bits" % (work, bd)][1]["waves_stage"] == waves
        assert m["D one bundle, three tap tables, %d bits" % bd][1]["waves_stage"] == 1
        long_p, small_p, n = M.family_d_unsplit(bd)
        xl, xs = long_p.model(), small_p.model()
        assert not xl["split_variants"] and xs["split_variants"] and sum(st["units"] for st in xl["stages"]) >= 8192
        assert [st["variants"] for st in xl["stages"][-n:]] == [1, 1, 1] and [st["variants"] for st in xs["stages"]] == [3, 3, 3]
        assert (long_p.sj[-n:] == small_p.sj).all()


def test_item_schedule_is_what_the_cases_are_for(plans):
    for p in M.family_e_long():
        x = p.model()
        assert sorted((x["waves_item_lean"], x["waves_item_generic"])) == [65536, 65537], p.name
    m = {p.name: p.model() for p in plans}
    assert m["E lean items only"]["waves_item_generic"] == 0 and m["E lean items only"]["waves_item_masked"] == 0
    assert m["E generic items only"]["waves_item_lean"] == 0 and m["E generic items only"]["waves_item_generic"] > 0
    x = m["E masked items only, behind zero plain items"]
    assert x["waves_item_lean"] == x["waves_item_generic"] == 0 and x["waves_item_masked"] > 0
    assert "item_band_order" in m["E a class of 37 waves (band order, a remainder)"]["edges"]
    per_wave = {(f, w, h): max(1, 64 // M.item_lanes(M.DF["SAD"] if f == "MASK" else M.DF[f], w, h, 0)) for f in M.E_FUNCS for (w, h) in M.E_SHAPES}
    assert per_wave[("SAD", 2, 2)] == 32 and per_wave[("HAD", 4, 4)] == 64 and per_wave[("SAD", 64, 8)] == 1 and per_wave[("HAD", 128, 128)] == 1 and per_wave[("HAD", 16, 8)] == 4


def test_positions_in_reach_and_reads_inside_the_planes(plans):
    n_rows = n_st = n_it = 0
    for p in plans + M.long_plans():
        x = p.model()
        for j, row in zip(p.ij, x["windows"]):
            arr, pad = p.planes[int(j["ref_plane"])]
            rs = arr.shape[1]
            for wn in row:
                first = int(j["ref_off"]) + pad * rs + pad + wn["minDy"] * rs + wn["minDx"]
                last_row = first + (wn["winH"] - 1) * rs
                fetched = ((wn["winW"] + 2 + 7) >> 3) * 8
                assert fetched - wn["winW"] <= M.ROW_SLACK                               # the documented margin: 18 bytes beyond a window row
                assert first >= 0 and last_row + wn["winW"] + M.ROW_SLACK <= arr.size, (p.name, wn["minDx"], wn["minDy"])
                n_rows += wn["winH"]
            oarr, opad = p.planes[int(j["org_plane"])]
            w, h = int(j["width"]), int(j["height"])
            o0 = int(j["org_off"]) + (0 if opad is None else opad * oarr.shape[1] + opad)
            assert o0 >= 0 and o0 + (h - 1) * (w if opad is None else oarr.shape[1]) + w <= oarr.size
        for s in p.sj:
            for k, tx, ty in M.stage_positions(s):
                assert -16 <= tx <= 16 and -16 <= ty <= 16, (p.name, k, tx, ty)
            arr, pad = p.planes[int(s["ref_plane"])]
            y, x0 = divmod(int(s["ref_off"]) + pad * arr.shape[1] + pad, arr.shape[1])
            bx0, by0, bx1, by1 = M.stage_read_box(s)
            assert x0 + bx0 >= 0 and y + by0 >= 0 and x0 + bx1 <= arr.shape[1] and y + by1 <= arr.shape[0], (p.name, x0, y)
            n_st += 1
        def inside(pl, off, w, rows, slack):
            arr, pad = p.planes[pl]
            if pad is None:                                                              # a pool: compact rows
                assert 0 <= off and off + w * rows + slack <= arr.size, (p.name, pl, off)
            else:
                y, x0 = divmod(off + pad * arr.shape[1] + pad, arr.shape[1])
                assert 0 <= y and y + rows < arr.shape[0] and x0 + w + slack <= arr.shape[1], (p.name, pl, x0, y)
        for it in np.unique(p.items):                                                    # (distinct records: the long plans repeat 64 block pairs)
            for pl, of in (("org_plane", "org_off"), ("cur_plane", "cur_off")):
                inside(int(it[pl]), int(it[of]), int(it["width"]), int(it["height"]), 8)
            n_it += 1
        for it in np.unique(p.mask_items):
            for pl, of in (("org_plane", "org_off"), ("cur_plane", "cur_off")):
                inside(int(it[pl]), int(it[of]), int(it["width"]), int(it["height"]), 8)
            assert p.planes[int(it["mask_plane"])][1] is None
            inside(int(it["mask_plane"]), int(it["mask_off"]), int(it["width"]), int(it["height"]) >> int(it["sub_shift"]), 8)
            marr = p.planes[int(it["mask_plane"])][0]
            assert marr.min() >= 0 and marr.max() <= 8                                   # GEO weights
            n_it += 1
    assert n_rows and n_st and n_it
    # the Hadamard family's operand contract (stages and HAD items): predictions are samples, originals samples or bi-prediction patterns; SAD, SSE and windows take any int16
    for p in plans:
        top = 1 << p.bd
        had = [(int(s["org_plane"]), int(s["ref_plane"])) for s in p.sj] + [(int(i["org_plane"]), int(i["cur_plane"])) for i in p.items if int(i["func"]) >= M.DF["HAD"]]
        for po, pc in set(had):
            assert p.planes[pc][0].min() >= 0 and p.planes[pc][0].max() < top and p.planes[po][0].min() > -top and p.planes[po][0].max() < 2 * top, (p.name, po, pc)
    a24 =[p for p in plans if p.name == "A max_window 24"][0]
    arr, pad = a24.planes[1]
    firsts, lasts = [], []
    for j, row in zip(a24.ij, a24.model()["windows"]):
        for wn in row:
            f = int(j["ref_off"]) + pad * arr.shape[1] + pad + wn["minDy"] * arr.shape[1] + wn["minDx"]
            firsts.append(f); lasts.append(f + (wn["winH"] - 1) * arr.shape[1] + wn["winW"])
    assert min(firsts) == 0 and max(lasts) == arr.size - arr.shape[1]                     # the first sample of the storage; the end of the last row but one


def test_window_model_equals_the_oracle_and_its_mutations_do_not(oracle):
    """the planes and candidate sets of family A would notice a window kernel with an even pitch, the wrong half split, no parity, an uncut last chunk or an extent
    compared with < : each mutation of the model changes at least one cost, and the unmutated model gives the oracle's cost for every candidate"""
    fam = M.family_a()
    hits = {mu: {} for mu in M.MUTATIONS}          # mutation -> block (w, h, ss) -> windows in which it changed a cost
    n = n_win = 0
    for p in fam:
        cc, _, _ = M.expected(p, oracle)
        x = p.model()
        for j, row in zip(p.ij, x["windows"]):
            blk = (int(j["width"]), int(j["height"]), int(j["sub_shift"]))
            for wn in row:
                got, _ = M.window_model(p, j, wn)
                assert len(got) == sum(len(q[2]) for q in wn["cands"])
                for e, v in got.items():
                    assert v == cc[e], (p.name, wn["minDx"], wn["minDy"], wn["winW"], wn["winH"], e, v, int(cc[e]))
                n += len(got)
                n_win += 1
                for mut in M.MUTATIONS:
                    bad, _ = M.window_model(p, j, wn, mut)
                    if any(bad[e] != cc[e] for e in bad):
                        hits[mut][blk] = hits[mut].get(blk, 0) + 1
    assert n == sum(p.cands.size for p in fam)
    caught = [mu for mu in M.MUTATIONS if hits[mu]]
    # how strong the cases are: windows that notice each mutation, per block.  Every block of the family notices every mutation — but the half split, which only
    # exists under sub_shift 1 — the 128-wide ones (largest pitch, two halves, originals beyond four chunks per lane) included
    blocks = sorted({(int(j["width"]), int(j["height"]), int(j["sub_shift"])) for p in fam for j in p.ij})
    for mu in M.MUTATIONS:
        print("%-18s windows that notice it, of %d: %d; per block %s" % (mu, n_win, sum(hits[mu].values()), {"%dx%d ss%d" % b: hits[mu].get(b, 0) for b in blocks}))
        for b in blocks:
            if mu != "half0_floor" or b[2]:
                assert hits[mu].get(b, 0) > 0, (mu, b)
    # the extent compared with < instead of <= : a slip of the host's clustering.  Costs cannot show it (every window it makes is a valid one); the window count does
    lt = [(p.name, p.model()["waves_int"], p.model(extent_lt=True)["waves_int"]) for p in fam]
    assert all(b > a for _, a, b in lt), lt
    caught.append("extent_lt")
    print("candidates of family A compared with the oracle: %d; mutations caught: %s; windows with <= and with <: %s" % (n, caught, lt))
    assert caught == list(M.MUTATIONS) + ["extent_lt"], sorted(todo)


def test_knobs_change_the_compact_plans_schedule():
    """family H: each knob that changes a count must do so on the compact plan (the device tier asserts these counts in the child processes)"""
    p = M.compact_plan()
    base = p.model()
    key = lambda x: (x["waves_int"], x["waves_stage"], x["waves_item"], x["lds_bytes"])
    for kn in (dict(dedupe=False), dict(cand_cap=64), dict(atomic_stages=False), dict(split_below=0), dict(bundle_work=320)):
        assert key(p.model(**kn)) != key(base), kn
    assert p.model(dedupe=False)["waves_int"] == base["waves_int"] + 1 and p.model(cand_cap=64)["waves_int"] == base["waves_int"] - 1
    assert p.model(bundle_work=320)["waves_stage"] == base["waves_stage"] - 2
    # VVHIP_ME_XCD_BAND, _ITEM_INTERLEAVE and _ITEM_SPANS reorder workgroups or regroup spans per wave: no count changes; their preconditions are met —
    assert base["waves_item_lean"] > 64                                                  # the interleave needs more than 64 lean waves
    assert all(x.model()["waves_item_lean"] > 65536 or x.model()["waves_item_generic"] > 65536 for x in M.family_e_long())      # the spans: launches beyond 65 536 waves


X86_DIFF16 = "x86 SAD rows subtract in 16 bits: |org - cur| > 32767 is not defined there"
_left_out = {}


@pytest.mark.ref
def test_oracle_equals_reference_on_operand_blocks(oracle, reflib):
    """family F: every candidate of every operand block and range; the x86 row left out for the full-int16 range only (by name, counted)"""
    n = 0
    for p in M.family_f():
        wide = "int16" in p.name
        for j in p.ij:
            w, h, ss = int(j["width"]), int(j["height"]), int(j["sub_shift"])
            ov = M._view(p, int(j["org_plane"]), int(j["org_off"]), w, h)
            ra, ry, rx = M._view(p, int(j["ref_plane"]), int(j["ref_off"]), w, h)
            for k in range(int(j["first_cand"]), int(j["first_cand"]) + int(j["n_cand"])):
                if reflib.simd and wide:
                    _left_out[X86_DIFF16] = _left_out.get(X86_DIFF16, 0) + 1
                    continue
                cur = (ra, ry + int(p.cands[k]["dy"]), rx + int(p.cands[k]["dx"]))
                assert oracle.dist("SAD", ov, cur, w, h, p.bd, ss) == reflib.dist("SAD", ov, cur, w, h, p.bd, ss), (p.name, w, h, k)
                n += 1
    print("family F: %d candidates compared with the %s row; left out: %s" % (n, "x86" if reflib.simd else "scalar", _left_out))
    assert n == (120 if reflib.simd else 180) and set(_left_out) <= {X86_DIFF16}


@pytest.mark.ref
@pytest.mark.parametrize("bd", [10, 8])
def test_oracle_equals_reference_on_the_position_sweep(oracle, reflib, bd):
    """family D's sweep: both passes of the interpolation and the stage's function at every evaluated position; nothing left out (8 and 10 bits, sample operands)"""
    p = M.family_d_sweep(bd)
    n = 0
    for s in p.sj:
        w, h, f = int(s["width"]), int(s["height"]), M.DF_NAME[int(s["func"])]
        ov = M._view(p, int(s["org_plane"]), int(s["org_off"]), w, h)
        ra, ry, rx = M._view(p, int(s["ref_plane"]), int(s["ref_off"]), w, h)
        for k, tx, ty in M.stage_positions(s):
            a = (ra, ry + (ty >> 4), rx + (tx >> 4)), w, h, tx & 15, ty & 15, bd, bool(s["alt_hpel"]), int(s["filter_mode"])
            po, pr = oracle.if_pred_luma_me(*a), reflib.if_pred_luma_me(*a)
            assert np.array_equal(po, pr), (k, tx, ty, int(s["filter_mode"]), int(s["alt_hpel"]))
            assert oracle.dist(f, ov, (po, 0, 0), w, h, bd, 0) == reflib.dist(f, ov, (pr, 0, 0), w, h, bd, 0), (k, tx, ty, f)
            n += 1
    assert n == sum(len(M.stage_positions(s)) for s in p.sj) and n > 3000
