"""Pins the oracle to the compiled reference (scalar row and x86 row, tolerance 0) on the extreme inputs of tests/dist_extremes.py, for everything the GPU tier
(tests/test_gpu_dist_extremes.py) asks the oracle: every item of the SAD / SSE / Hadamard lists of the families A to D, the masked SAD and the fixed-weight SSE of family E.
The int64 models of dist_extremes are asserted equal to the oracle on every item; the guards are computed from them, and the sensitivity test mutates them.  Only the tests
that call the compiled reference carry the `ref` mark.

Where the x86 row is left out (the last test prints the counts of a whole run); the scalar row is compared on every item, without exception:
  - Hadamard at a bit depth above 10 (the 12-bit and the full-int16 domain of family A): xCalcHAD8x8_SSE / xCalcHAD16x16_fast_SSE refuse it (x86/RdCostX86.h:655-659,
    :800-804) and the encoder routes those depths to the scalar row (RdCost.cpp:174)
  - an operand pair whose difference does not fit 16 bits (|d| = 65535 and 46340 of the families B and E, the full-int16 domain of A, the difference levels 32767 and
    46340 of the fixed-weight SSE): the x86 SAD / SSE / masked-SAD rows subtract in 16 bits
  - SAD / SSE on a width that is no multiple of 4 (2 and 6 of family B): xGetSAD_SIMD refuses it (x86/RdCostX86.h:291) and xGetSSE_SIMD takes four columns per step (:124)
  - an SSE whose sum exceeds 2^31 - 1 (the constant differences 1023 and 4095 of family B from 64x64 and 16x8 samples on): xGetSSE_SIMD and its width twins add in 32-bit
    lanes and return the low 32 bits of the sum (x86/RdCostX86.h:80-96)
  - a masked SAD of width 4 or more with step_x 2, with a mask_stride2 other than -step_x * width, with a width that is no multiple of 8, or with a sum beyond 32 bits:
    xGetSADwMask_SIMD reads the mask in whole vectors at steps of +-1, never adds maskStride2 and adds in 32-bit lanes (x86/RdCostX86.h:2652-2715)
  - a fixed-weight SSE with a weight of 2^31 or more (the largest weights of the difference levels 0, 1 and 255): fixWeightedSSE_SIMD multiplies the weight as a signed
    32-bit value (_mm_mul_epi32, x86/RdCostX86.h:2891-2911)
The families with flagged samples of 10 and 8 bits, the bi-prediction domains, the list mechanics and the derived copies are compared on both rows in full.
Widths that are no power of two are compared with the reference's general functions (dist_extremes: RdCost.cpp:177-181), on both rows.

Inputs the reference leaves undefined are listed in the docstring of dist_extremes; test_undefined_corners_stay_out asserts from the models that no item reaches them.

Measured on a CPU host: 13.4 s for the file with both reference rows (24 tests) and 11.8 s without the reference (10 tests, the 14 `ref` tests skipped): the guards of the
undefined corners 4.3 s, the models against the oracle 2.4 s and 2.3 s for the two parts of family A and below 0.5 s for the others, the sensitivity test 1.2 s, family E's models
0.9 s; the oracle against a reference row 0.5 s at most per family (12 510 items the largest).
"""
import numpy as np
import pytest

import dist_extremes as M

_x86_skipped = {}
HAD_DEPTH = "Hadamard at a bit depth above 10"
DIFF16 = "a difference that does not fit 16 bits"
WIDTH4 = "SAD / SSE on a width that is no multiple of 4"
SSE32 = "an SSE sum beyond 2^31 - 1"
WEIGHT31 = "a fixed weight of 2^31 or more"
MASK_WALK = "a masked SAD outside the x86 row's mask walk or 32-bit sum"

_exp = {}


def _expected(oracle, dom, job):
    out = []
    for k in range(job.n):
        key = (dom.name,) + job.key(k)
        if key not in _exp:
            _exp[key] = M.expected(oracle, dom, job, k)
        out.append(_exp[key])
    return out


def _ref_value(reflib, dom, job, k):
    if job.func in ("SAD", "SSE") and not M.is_pow2(job.w):
        # the general functions xGetSAD / xGetSSE are the first entry of their block of the table; the reference's wrapper adds Log2( width ) to the index it is given
        ox, oy, cx, cy = job.items[k]
        (po, so), (pc, sc) = reflib._ptr_stride((dom.org, oy, ox)), reflib._ptr_stride((dom.cur, cy, cx))
        return reflib.L.vvref_dist(reflib.simd, reflib._df[job.func] - (job.w.bit_length() - 1), po, so, pc, sc, job.w, job.h, dom.bd, job.ss)
    return M.expected(reflib, dom, job, k)


def _x86_rule(dom, job, value):
    if job.func.startswith("HAD") and dom.bd > 10:
        return HAD_DEPTH
    if dom.d_max > 32767:
        return DIFF16
    if job.func in ("SAD", "SSE") and job.w % 4:
        return WIDTH4
    if job.func == "SSE" and value > M.INT_MAX:
        return SSE32
    return None


def _skip(rule, n=1):
    _x86_skipped[rule] = _x86_skipped.get(rule, 0) + n


FAMILIES = ("A-batch", "A-multi", "B", "C", "D")


def _work(family):
    return [(f, d, j) for (f, d, j) in M.dist_work() if f.startswith(family)]


@pytest.mark.ref
@pytest.mark.parametrize("family", FAMILIES)
def test_lists_oracle_equals_reference(oracle, reflib, family):
    """every item of every list of the family; the x86 row left out by the rules of the module docstring only"""
    n = 0
    seen = set()
    for _, dom, job in _work(family):
        exp = _expected(oracle, dom, job)
        for k in range(job.n):
            key = (dom.name,) + job.key(k)
            if key in seen:
                continue
            seen.add(key)
            rule = _x86_rule(dom, job, exp[k]) if reflib.simd else None
            if rule:
                _skip(rule)
                continue
            got = _ref_value(reflib, dom, job, k)
            assert got == exp[k], (family, dom.name, job.func, job.w, job.h, job.ss, job.items[k], got, exp[k])
            n += 1
    print("%s: %d distinct items compared with the %s row" % (family, n, "x86" if reflib.simd else "scalar"))
    assert n > 0


@pytest.mark.parametrize("family", FAMILIES)
def test_lists_model_equals_oracle(oracle, family):
    """the int64 models equal the oracle on every item; on the merged Hadamard jobs of 10 and 8 bits the model of the packed tile (five wrapping stages with the flag,
    four without) does too"""
    seen = set()
    for _, dom, job in _work(family):
        exp = _expected(oracle, dom, job)
        form = None
        if family == "A-multi" and dom.bd <= 10:
            form = "narrow" if dom.flags else "wide"
        for k in range(job.n):
            key = (dom.name,) + job.key(k)
            if key in seen:
                continue
            seen.add(key)
            o, c = dom.blocks(job, k)
            assert M.dist_model(job.func, o, c, job.ss) == exp[k], (family, dom.name, job.func, job.w, job.h, job.items[k])
            if form:
                assert M.dist_model(job.func, o, c, job.ss, (), form) == exp[k], (family, dom.name, form, job.func, job.w, job.items[k])
                if dom.flags:       # samples are inside the general form's domain too (vvhip_dist_multi has no flag)
                    assert M.dist_model(job.func, o, c, job.ss, (), "wide") == exp[k]


# ---- family E ----------------------------------------------------------------------------------------------------------------------------------------------------
def _mask_expected(lib, name):
    dom, mask = M.b_domain(name), M.e_mask()
    return [[lib.sad_mask((dom.org, oy, ox), (dom.cur, cy, cx), (mask, my, mx), sx, ms2, w, h, ss) for (ox, oy, cx, cy, mx, my) in items]
            for (w, h, ss, sx, ms2, items) in M.e_mask_items(name)]


def _wsse_expected(lib):
    dom = M.e_levels_domain()
    return [[lib.fix_weighted_sse((dom.org, oy, ox), (dom.cur, cy, cx), w, h, wt) for (ox, oy, cx, cy, wt) in items] for (w, h, items) in M.e_wsse_items()]


@pytest.mark.ref
def test_masked_sad_and_weighted_sse_oracle_equals_reference(oracle, reflib):
    n = 0
    for name in M.E_DOMAINS:
        if reflib.simd and M.b_domain(name).d_max > 32767:
            _skip(DIFF16, sum(len(x[5]) for x in M.e_mask_items(name)))
            continue
        dom, mask = M.b_domain(name), M.e_mask()
        for (w, h, ss, sx, ms2, items), exp in zip(M.e_mask_items(name), _mask_expected(oracle, name)):
            for (ox, oy, cx, cy, mx, my), e in zip(items, exp):
                total = (e - (1 << 64) if e >> 63 else e) >> ss
                if reflib.simd and w >= 4 and (abs(sx) != 1 or ms2 != -w * sx or w % 8 or abs(total) > M.INT_MAX):
                    _skip(MASK_WALK)
                    continue
                assert reflib.sad_mask((dom.org, oy, ox), (dom.cur, cy, cx), (mask, my, mx), sx, ms2, w, h, ss) == e, (name, w, h, ss, sx, ms2)
                n += 1
    dom = M.e_levels_domain()
    exp = _wsse_expected(oracle)
    for (w, h, items), e in zip(M.e_wsse_items(), exp):
        for (ox, oy, cx, cy, wt), ev in zip(items, e):
            d = M.E_LEVELS[oy // M.E_LRH]
            if reflib.simd and (d > 32767 or wt >> 31):
                _skip(DIFF16 if d > 32767 else WEIGHT31)
                continue
            assert reflib.fix_weighted_sse((dom.org, oy, ox), (dom.cur, cy, cx), w, h, wt) == ev, (w, h, d, wt)
            n += 1
    print("masked SAD and fixed-weight SSE: %d items compared with the %s row" % (n, "x86" if reflib.simd else "scalar"))


def test_masked_sad_and_weighted_sse_model_and_guards(oracle):
    """the models equal the oracle.  Guards: the largest |product| of the masked SAD is 65535 * 32768 (inside `int`); running sums go negative (the Distortion wraps) with
    the mixed and the negative masks; every weight of a level keeps its term inside `int`, the largest one lands within one term of 2^31 - 1, and the weight above it would not"""
    mask = M.e_mask().astype(np.int64)
    for name in M.E_DOMAINS:
        dom = M.b_domain(name)
        big = low = 0
        for (w, h, ss, sx, ms2, items), exp in zip(M.e_mask_items(name), _mask_expected(oracle, name)):
            for (ox, oy, cx, cy, mx, my), e in zip(items, exp):
                o, c = dom.org[oy:oy + h, ox:ox + w].astype(np.int64), dom.cur[cy:cy + h, cx:cx + w].astype(np.int64)
                v, b, l = M.mask_sad_model(o, c, mask, my, mx, sx, ms2, ss)
                assert v == e, (name, w, h, ss, sx, ms2)
                big, low = max(big, b), min(low, l)
        assert big <= M.INT_MAX and low < 0
        if name == "d65535":
            assert big == 65535 * 32768
    dom = M.e_levels_domain()
    tops = {}
    for (w, h, items), exp in zip(M.e_wsse_items(), _wsse_expected(oracle)):
        for (ox, oy, cx, cy, wt), e in zip(items, exp):
            o, c = dom.org[oy:oy + h, ox:ox + w].astype(np.int64), dom.cur[cy:cy + h, cx:cx + w].astype(np.int64)
            v, t, d2 = M.wsse_model(o, c, wt)
            assert v == e and t <= M.INT_MAX and d2 <= 46340 * 46340, (w, h, wt, v, e, t)
            tops[oy // M.E_LRH] = max(tops.get(oy // M.E_LRH, 0), t)
    for r, d in enumerate(M.E_LEVELS):
        top = M.wsse_max_weight(d)
        if d and top < (1 << 32) - 1:
            assert ((top + 1) * d * d + 32768) >> 16 > M.INT_MAX and M.INT_MAX - tops[r] <= (d * d) >> 16, (d, top, tops[r])
    assert {w for w, _, _ in M.e_wsse_items()} >= {1, 2, 128} and set(M.E_WEIGHTS) == {0, 1, 65535, 65536, 1 << 20}


# ---- guards ------------------------------------------------------------------------------------------------------------------------------------------------------
def test_family_guards(oracle):
    """A: each of the 64 coefficients of an 8x8 tile reaches 64 D with either sign in every merged domain, and the fast tile's averages take every remainder; B: the
    accumulators reach 128 * 128 * 65535 (SAD) and pass 2^32 (SSE); C: the list lengths, the shared / unshared pairs, the tables of 9, 16, 17 jobs, the workgroup counts
    8, 9, 15, 17; D: all 64 candidate phases with the nine original phases, both odd strides, a row count that is no multiple of 8"""
    H8 = M.hadamard(8)
    for name in M.A_MULTI_DOMAINS:
        dom = M.a_domain(name)
        job = [j for j in M.a_multi_jobs() if j.w == 8 and j.tag == "even"][0]
        hit = set()
        for k in range(job.n):
            o, c = dom.blocks(job, k)
            co = H8 @ (o - c) @ H8.T
            if np.abs(co).max() == 64 * dom.d_max:
                u, v = np.unravel_index(np.abs(co).argmax(), co.shape)
                hit.add((int(u), int(v), int(np.sign(co[u, v]))))
        assert len(hit) == 128, (name, len(hit))
    for name in ("s10", "b10"):
        dom = M.a_domain(name)
        rem = set()
        for arr in (dom.org, dom.cur):
            a = arr[M.R2_Y:M.R2_Y + 128, :128].astype(np.int64)
            rem |= set(((a[0::2, 0::2] + a[1::2, 0::2] + a[0::2, 1::2] + a[1::2, 1::2]) & 3).ravel().tolist())
        assert rem == {0, 1, 2, 3}, (name, rem)
    assert (M.a_domain("b10").org.min(), M.a_domain("b10").org.max(), M.a_domain("b8").org.min(), M.a_domain("b8").org.max()) == (-1023, 2046, -255, 510)
    assert {(j.w, j.h) for j in M.a_batch_jobs()} == set(M.A_SHAPES) and {j.func for j in M.a_batch_jobs()} == set(M.A_FUNCS)
    top_sad = max(max(_expected(oracle, M.b_domain("d65535"), j)) for j in M.b_jobs("d65535"))
    top_sse = max(max(_expected(oracle, M.b_domain("d46340"), j)) for j in M.b_jobs("d46340") if j.func == "SSE")
    assert top_sad == 128 * 128 * 65535 and top_sse == 128 * 128 * 46340 * 46340 > 1 << 32
    assert max(max(_expected(oracle, M.b_domain("p12"), j)) for j in M.b_jobs("p12") if j.func == "SSE") == 128 * 128 * 4095 * 4095
    widths = {j.w for j in M.b_jobs("p10")}
    assert widths >= {2, 4, 6, 12, 24, 40, 72, 96, 120} and {M.lanes_per_row(w)[0] for w in widths} == {2, 4, 8}
    assert any(j.h == 2 and j.ss == 1 for j in M.b_jobs("p10")) and any(j.h == 1 for j in M.b_jobs("p10"))
    assert {j.n for j in M.c_list_jobs() if j.func != "HAD_2SAD"} == set(M.C_NS) and {j.tag for j in M.c_list_jobs()} == set(M.C_KINDS)
    for job in M.c_list_jobs():
        same = [job.items[i][:2] == job.items[i + 1][:2] for i in range(0, job.n - 1, 2)]
        if same:
            assert {"shared": all(same), "unshared": not any(same), "mixed": job.n < 4 or (any(same) and not all(same))}[job.tag], (job.tag, job.n)
    t = M.c_tables()
    for k in (9, 16, 17):
        assert len(t["sadsse%d" % k]) == len(t["had%d" % k]) == k and all(M.mergeable(j.func, j.w, j.h, j.ss, j.n) for j in t["sadsse%d" % k] + t["had%d" % k])
    assert [M.blocks_model(j.func, j.w, j.h, j.ss, j.n) for j in t["xcd"]] == [8, 9, 15, 17, 8, 9, 15, 17]
    assert sum(j is None for j in t["mixed"]) == 3 and sum(j is not None and not M.mergeable(j.func, j.w, j.h, j.ss, j.n) for j in t["mixed"]) == 3
    assert sorted(s % 8 for s, _ in M.D_PLANES) == [0, 0, 1, 4, 7] and {(h + 2 * M.D_PAD) % 8 for _, h in M.D_PLANES} == {7, 0}
    for (stride, height) in M.D_PLANES:
        it = M.d_items(stride, height)
        assert {(ox & 7, oy & 7, cx & 7, cy & 7) for (ox, oy, cx, cy) in it["phases"]} == {(a, b, c, d) for a in M.D_ORG_PHASES for b in M.D_ORG_PHASES for c in range(8) for d in range(8)}
        assert all((v & 7) == 0 for i in it["aligned"] for v in i) and sum(any(v & 7 for v in i) for i in it["one_off"]) == 1 and len(it["aligned"]) == 64
        rows = height + 2 * M.D_PAD
        assert {(i[2], i[3]) for i in it["corners"]} == {(0, 0), (stride - 8, 0), (0, rows - 8), (stride - 8, rows - 8)}


def test_undefined_corners_stay_out(oracle):
    """from the int64 models, over every item: no SSE difference beyond 46340 (the `int` square), no SAD sum and no Hadamard tile sum beyond `int`, bit depths of the
    flagged jobs at most 12 and their samples inside [0, 2^bd); the masked SAD's product and the fixed-weight SSE's term are asserted by the test of family E"""
    worst = dict(sse_d=0, sad=0, tile=0)
    seen = set()
    for fam, dom, job in M.dist_work():
        if dom.flags:
            assert dom.bd <= 12 and dom.org.min() >= 0 and dom.cur.min() >= 0 and max(dom.org.max(), dom.cur.max()) < 1 << dom.bd, dom.name
        for k in range(job.n):
            key = (dom.name,) + job.key(k)
            if key in seen:
                continue
            seen.add(key)
            o, c = dom.blocks(job, k)
            if job.func == "SSE":
                worst["sse_d"] = max(worst["sse_d"], int(np.abs(o - c).max()))
            elif job.func == "SAD":
                worst["sad"] = max(worst["sad"], M.sad_model(o, c, job.ss))
            else:
                worst["tile"] = max(worst["tile"], M.tile_max(o, c, job.func == "HAD_fast"))
                if job.func == "HAD_2SAD":
                    worst["sad"] = max(worst["sad"], 2 * M.sad_model(o, c))
    mask = M.e_mask().astype(np.int64)
    worst.update(prod=0, term=0, wsse_d=0)
    for name in M.E_DOMAINS:
        dom = M.b_domain(name)
        for (w, h, ss, sx, ms2, items) in M.e_mask_items(name):
            for (ox, oy, cx, cy, mx, my) in items[::3] + items[1::3][:1] + items[2::3][:1]:
                o, c = dom.org[oy:oy + h, ox:ox + w].astype(np.int64), dom.cur[cy:cy + h, cx:cx + w].astype(np.int64)
                assert o.shape == c.shape == (h, w)
                worst["prod"] = max(worst["prod"], M.mask_sad_model(o, c, mask, my, mx, sx, ms2, ss)[1])
    dom = M.e_levels_domain()
    for (w, h, items) in M.e_wsse_items():
        for (ox, oy, cx, cy, wt) in items:
            o, c = dom.org[oy:oy + h, ox:ox + w].astype(np.int64), dom.cur[cy:cy + h, cx:cx + w].astype(np.int64)
            assert o.shape == c.shape == (h, w)
            _, t, d2 = M.wsse_model(o, c, wt)
            worst["term"], worst["wsse_d"] = max(worst["term"], t), max(worst["wsse_d"], d2)
    print("undefined corners: largest SSE difference %d (limit 46340), largest SAD sum %d, largest Hadamard tile sum %d, largest masked product %d, largest weighted term %d "
          "(limit 2^31 - 1), largest squared difference of the fixed-weight SSE %d" % (worst["sse_d"], worst["sad"], worst["tile"], worst["prod"], worst["term"], worst["wsse_d"]))
    assert worst["sse_d"] == 46340 and worst["sad"] <= M.INT_MAX and worst["tile"] <= M.INT_MAX
    assert worst["prod"] == 65535 * 32768 <= M.INT_MAX and worst["term"] <= M.INT_MAX and worst["wsse_d"] == 46340 * 46340 <= M.INT_MAX
    assert all(j.func == "SAD" for j in M.b_jobs("d65535"))


# ---- sensitivity -------------------------------------------------------------------------------------------------------------------------------------------------
def test_sensitivity():
    """each mutation of a model changes the value of at least one item of the families: a packed stage that wraps one stage later (<form>_late) or as if one stage sooner
    (<form>_early) in either form; a 32-bit SSE accumulator; the DC not quartered; `<< sub_shift` dropped; HAD_2SAD without the min; an integer shift for the rectangular
    tiles' double rounding; an unsigned shift in the 2x2 average; a funnel shift off by one sample; the shifted copy read at k; the second item of a pair on the first's
    original rows"""
    changed = {}

    def count(mut, work, form=None, pick=lambda dom, job: True, lim=400):
        n = 0
        for dom, job in work:
            if not pick(dom, job):
                continue
            for k in range(0, min(job.n, lim)):
                o, c = dom.blocks(job, k)
                n += M.dist_model(job.func, o, c, job.ss, (mut,), form) != M.dist_model(job.func, o, c, job.ss, (), form)
        return n

    multi = lambda name: [(M.a_domain(name), j) for j in M.a_multi_jobs() if j.w <= 32 and j.tag == "even"]
    batch = lambda name: [(M.a_domain(name), j) for j in M.a_batch_jobs()]
    for form, name in (("narrow", "s10"), ("wide", "b10")):
        changed[form + "_late"] = count(form + "_late", multi(name), form)
        changed[form + "_early"] = count(form + "_early", multi(name), form)
    changed["sse_acc32"] = count("sse_acc32", [(M.b_domain("d46340"), j) for j in M.b_jobs("d46340")], pick=lambda d, j: j.func == "SSE")
    changed["dc_not_quartered"] = count("dc_not_quartered", batch("s10"), pick=lambda d, j: j.func == "HAD")
    changed["no_subshift"] = count("no_subshift", [(M.b_domain("p10"), j) for j in M.b_jobs("p10")], pick=lambda d, j: j.func == "SAD" and j.ss == 1)
    changed["had2sad_no_min"] = count("had2sad_no_min", [(M.c_domain(), j) for j in M.c_list_jobs()], pick=lambda d, j: j.func == "HAD_2SAD")
    changed["rect_int_shift"] = count("rect_int_shift", batch("s8"), pick=lambda d, j: j.func == "HAD" and j.w != j.h)
    changed["avg_unsigned"] = count("avg_unsigned", [(M.a_domain("b10"), j) for j in M.a_multi_jobs() if j.func == "HAD_fast" and j.w == 32 and j.tag == "even"])
    lists = {"funnel_off": [(M.d_domain(*p), j) for p in M.D_PLANES[:2] for j in M.d_jobs(*p) if j.tag == "phases"],
             "shift_at_k": [(M.a_domain("s10"), j) for j in M.a_multi_jobs() if j.tag == "odd" and j.w <= 16] + [(M.d_domain(*M.D_PLANES[0]), M.d_jobs(*M.D_PLANES[0])[-1])],
             "pair_reuse": [(M.c_domain(), j) for j in M.c_list_jobs() if j.tag in ("unshared", "mixed") and j.func in ("SAD", "SSE") and j.n <= 65]}
    for mut, work in lists.items():
        changed[mut] = sum(a != b for dom, job in work for a, b in zip(M.list_model(dom, job, (mut,)), M.list_model(dom, job)))
    shared = [(M.c_domain(), j) for j in M.c_list_jobs() if j.tag == "shared" and j.func == "SAD" and j.n <= 65]
    assert all(M.list_model(d, j, ("pair_reuse",)) == M.list_model(d, j) for d, j in shared)      # and where the pairs do share, reuse is right
    print("sensitivity: items changed per mutation %s" % changed)
    assert set(changed) == set(M.MUTATIONS)
    assert all(v > 0 for v in changed.values()), changed


def test_copies_model():
    """the restatements of the tiled and the shifted copy on a plane whose samples are their own addresses"""
    a = np.arange(11 * 19, dtype=np.int16).reshape(11, 19)
    t = M.tile8_model(a)
    assert t.size + 128 == M.tiled8_elems(19, 11) and t.size == 2 * 3 * 64
    for (y, x) in ((0, 0), (7, 7), (8, 0), (10, 18), (3, 16)):
        assert t[((y >> 3) * 3 + (x >> 3)) * 64 + (y & 7) * 8 + (x & 7)] == a[y, x]
    assert t[(1 * 3 + 2) * 64 + 2 * 8 + 3] == 0 and t[(1 * 3 + 0) * 64 + 3 * 8] == 0          # beyond the stride; beyond the rows
    s = M.shift1_model(a)
    assert np.array_equal(s[:-1], a.reshape(-1)[1:]) and s[-1] == 0


@pytest.mark.ref
def test_x86_row_skips_only_by_the_rules(reflib):
    """runs last in the file: the only items the x86 row was not compared on are those of the rules of the module docstring"""
    print("items compared with the scalar row only, by rule: %s" % _x86_skipped)
    assert set(_x86_skipped) <= {HAD_DEPTH, DIFF16, WIDTH4, SSE32, MASK_WALK, WEIGHT31}, _x86_skipped
