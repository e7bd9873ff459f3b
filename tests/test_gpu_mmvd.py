"""GPU tier of the MMVD merge-candidate entry: vvhip_merge_mmvd_costs_batch through HotPath.merge_mmvd_costs, tolerance 0.

Expected values: the model of tests/mmvd_ref.py — its vectors restated from the reference, its interpolation and Hadamard sums executed from the oracle library — on the fixed
case list and on a mixed list, and the library's own two-launch form ( vvhip_pred_inter_batch_blend, then the Hadamard list ) on items built with vvhip_mmvd_candidate.
Costs land in sentinel-filled tensors: a slot the mask does not name must come back untouched.  Every requested candidate is compared."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import mmvd_cases as MC  # noqa: E402
import mmvd_ref as MR  # noqa: E402

E_ARG = "vvenc_hip error -1"
ENTRY = "vvhip_merge_mmvd_costs_batch"
SENT32 = int(np.array(MC.SENTINEL, np.uint32).view(np.int32))


@pytest.fixture(scope="module")
def hp():
    from vvenc_amd.hotpath import HotPath
    return HotPath()


_dev = {}


def dev_planes(hp, geom, bd, kind="natural"):
    """the group's planes on the device, with eight spare samples round the arrays -> ( [ reference Planes ], original Plane )"""
    key = (geom, bd, kind)
    if key not in _dev:
        refs, org = MC.planes(geom, bd, kind)
        _dev[key] = ([hp.plane(np.array(p), 8, extend=False) for p in refs], hp.plane(np.array(org), 8, extend=False))
    return _dev[key]


def run(hp, group, items, kind="natural", cost=None):
    """the entry on a sentinel-filled tensor -> uint32 [ n, 64 ]"""
    import torch
    geom, bd, func, df = group
    pw, ph, ctu, _ = MC.GEOMS[geom]
    refs, org = dev_planes(hp, geom, bd, kind)
    if cost is None:
        cost = torch.full((max(1, len(items)), 64), SENT32, dtype=torch.int32, device=hp.device)
    hp.merge_mmvd_costs(refs, items, org, pw, ph, ctu, bd, func, df, cost=cost)
    torch.cuda.synchronize()
    return cost.cpu().numpy().view(np.uint32)


def records(hp, group, cl, kind="natural"):
    refs, org = dev_planes(hp, group[0], group[1], kind)
    return MC.as_list(cl, refs[0].stride, org.stride)


def mismatches(got, want):
    return np.argwhere(got != want).tolist()[:8]


_expected = {}


def expected(oracle, name, group, cl):
    if (name, group) not in _expected:
        _expected[(name, group)] = MC.expected_group(oracle, group, cl)
    return _expected[(name, group)]


def test_case_list(hp, oracle):
    for group, cl in MC.groups(MC.cases()).items():
        got = run(hp, group, records(hp, group, cl))
        want = expected(oracle, "cases", group, cl)
        assert np.array_equal(got, want), (group, [c["name"] for c in cl], mismatches(got, want))


def mixed():
    """a few hundred CUs of sides up to 32: every base shape ( random_cu ), both functions, the three bit depths, dis_frac on one group; some with the full mask"""
    rng = np.random.default_rng(2026)
    out = []
    for g, (bd, func, df) in enumerate(((8, "HAD", 0), (10, "HAD", 0), (12, "HAD", 0), (8, "HAD_fast", 0), (10, "HAD_fast", 1), (12, "HAD_fast", 0))):
        for k in range(50):
            out.append(MC.random_cu(rng, "mixed%d_%d" % (g, k), ("small", bd, func, df), 32, 64 if k % 10 == 0 else 12))
    return out


MIXED = mixed()


def test_mixed_list_equals_the_model(hp, oracle):
    n = 0
    for group, cl in MC.groups(MIXED).items():
        got = run(hp, group, records(hp, group, cl))
        want = expected(oracle, "mixed", group, cl)
        assert np.array_equal(got, want), (group, mismatches(got, want))
        n += int((want != MC.SENTINEL).sum())
    assert len(MIXED) == 300 and n > 4000


def test_mixed_list_equals_the_two_launch_form(hp):
    import torch
    from vvenc_amd.hotpath import Plane
    for group, cl in MC.groups(MIXED).items():
        geom, bd, func, df = group
        refs, org = dev_planes(hp, geom, bd)
        it = records(hp, group, cl)
        got = run(hp, group, it)
        pit, bl, rows, by_size = MC.two_launch_lists(hp, it, group, refs[0].stride)
        pp = Plane(hp.device, 1024, rows, 0)
        for k in range(pit.size):
            x, y = next((t[1], t[2]) for t in by_size[(int(pit[k]["width"]), int(pit[k]["height"]))] if t[5] == k)
            pit[k]["dst_off"] = y * pp.stride + x
        hp.pred_inter_batch(refs, pit, pp.storage.view(-1), pp.stride, bd, blend=bl)
        jobs, outs = [], []
        for (w, h), lst in by_size.items():
            pairs = torch.from_numpy(np.array([(o, y * pp.stride + x) for (o, x, y, _, _, _) in lst], np.int32)).to(hp.device)
            out = torch.zeros(len(lst), dtype=torch.int64, device=hp.device)
            jobs.append((w, h, 0, len(lst), pairs, out))
            outs.append((lst, out))
        hp.dist_multi(func, org, pp, jobs, bd)
        torch.cuda.synchronize()
        want = np.full_like(got, MC.SENTINEL)
        for lst, out in outs:
            o = out.cpu().numpy()
            for j, (_, _, _, i, v, _) in enumerate(lst):
                want[i, v] = o[j]
        assert np.array_equal(got, want), (group, mismatches(got, want))


def test_permuted_list_gives_the_same_items(hp):
    group, cl = next(iter(MC.groups(MIXED).items()))
    it = records(hp, group, cl)
    a = run(hp, group, it)
    perm = np.random.default_rng(5).permutation(it.size)
    pit = it[perm].copy()
    pit["cost_off"] = 64 * np.arange(it.size)
    b = run(hp, group, pit)
    assert np.array_equal(b, a[perm])


def test_two_runs_give_identical_bytes(hp):
    for group, cl in MC.groups([c for c in MC.cases() if c["group"][0] == "large"] + MIXED[:50]).items():
        it = records(hp, group, cl)
        assert run(hp, group, it).tobytes() == run(hp, group, it).tobytes()


def test_partial_masks_leave_the_other_slots(hp, oracle):
    group, cl = next(iter(MC.groups(MIXED).items()))
    rng = np.random.default_rng(9)
    cl = [dict(c, mask=tuple(int(m) & int(rng.integers(0, 1 << 32)) for m in c["mask"])) for c in cl[:20]]
    cl[3] = dict(cl[3], mask=(0, 0))
    got = run(hp, group, records(hp, group, cl))
    want = MC.expected_group(oracle, group, cl)
    assert np.array_equal(got, want) and (got[3] == MC.SENTINEL).all() and (want == MC.SENTINEL).sum() > 20 * 40


def test_empty_list(hp):
    group = ("small", 10, "HAD", 0)
    got = run(hp, group, np.zeros(0, MC.MMVD_ITEM_DTYPE))
    assert (got == MC.SENTINEL).all()


def bad_items():
    """( what, change applied to a good record ) — each must be refused"""
    def f(field, value, idx=None):
        def g(it):
            if idx is None:
                it[0][field] = value
            else:
                it[0][field][idx] = value
        return g
    return [("w not a power of two", f("w", 12)), ("h too small for w", f("h", 4)), ("w of 2", f("w", 2)), ("h of 0", f("h", 0)),
            ("plane outside the table", f("ref_plane", 3, (0, 0))), ("plane below -1", f("ref_plane", -2, (0, 1))), ("bcw_idx 5", f("bcw_idx", 5, 0)),
            ("cu outside the picture", f("cu_x", 96)), ("cu above the picture", f("cu_y", -4)), ("negative org_off", f("org_off", -1)), ("negative cost_off", f("cost_off", -64)),
            ("negative ref_off", f("ref_off", -1, (0, 0))), ("reserved byte", f("rsv", 1, 13)), ("reserved byte in front", f("rsv0", 1, 0)),
            ("a base vector beyond 18 bits", f("mv", 1 << 17, (0, 0, 1))),
            ("a base without lists and with candidates", lambda it: it[0]["ref_plane"].__setitem__((1, slice(None)), -1))]


def test_argument_errors_write_nothing(hp):
    import torch
    from vvenc_amd import VVHipError
    group = ("small", 10, "HAD", 0)
    pw, ph, ctu, _ = MC.GEOMS["small"]
    refs, org = dev_planes(hp, "small", 10)
    good = records(hp, group, [MC.cu("good", group, 4, 8, 16, 16, MC.base((5, 5), (-5, 9)), MC.base((1, 2), None))] * 2)
    cost = torch.full((2, 64), SENT32, dtype=torch.int32, device=hp.device)

    def refused(call, what):
        with pytest.raises(VVHipError) as e:
            call()
        assert E_ARG in str(e.value) and ENTRY in str(e.value), (what, str(e.value))
        torch.cuda.synchronize()
        assert (cost.cpu().numpy() == SENT32).all(), what
    for what, change in bad_items():
        it = good.copy()
        change(it[1:])
        refused(lambda: hp.merge_mmvd_costs(refs, it, org, pw, ph, ctu, 10, "HAD", 0, cost=cost), what)
    refused(lambda: hp.merge_mmvd_costs(refs, good, org, pw, ph, ctu, 7, "HAD", 0, cost=cost), "bit depth 7")
    refused(lambda: hp.merge_mmvd_costs(refs, good, org, pw, ph, ctu, 13, "HAD", 0, cost=cost), "bit depth 13")
    refused(lambda: hp.merge_mmvd_costs(refs, good, org, pw, ph, ctu, 10, "SAD", 0, cost=cost), "func SAD")
    refused(lambda: hp.merge_mmvd_costs(refs, good, org, pw, ph, ctu, 10, "HAD_2SAD", 0, cost=cost), "func HAD_2SAD")
    refused(lambda: hp.merge_mmvd_costs(refs, good, org, pw, ph, 48, 10, "HAD", 0, cost=cost), "ctu 48")
    refused(lambda: hp.merge_mmvd_costs(refs[:1], good, org, pw, ph, ctu, 10, "HAD", 0, cost=cost), "a table of one plane")
    refused(lambda: hp.merge_mmvd_costs(refs, good, None, pw, ph, ctu, 10, "HAD", 0, cost=cost), "d_org missing")
    refused(lambda: hp._ck(hp.L.vvhip_merge_mmvd_costs_batch(hp.ctx, None, 0, good.ctypes.data, 2, pw, ph, ctu, 10, 2, 0, org.buf_ptr, org.stride, cost.data_ptr())), "planes missing")
    refused(lambda: hp._ck(hp.L.vvhip_merge_mmvd_costs_batch(hp.ctx, None, 0, None, 2, pw, ph, ctu, 10, 2, 0, org.buf_ptr, org.stride, cost.data_ptr())), "items missing")
    refused(lambda: hp._ck(hp.L.vvhip_merge_mmvd_costs_batch(hp.ctx, None, 0, good.ctypes.data, 2, pw, ph, ctu, 10, 2, 0, org.buf_ptr, org.stride, None)), "d_cost missing")
    # and the good list runs
    hp.merge_mmvd_costs(refs, good, org, pw, ph, ctu, 10, "HAD", 0, cost=cost)
    torch.cuda.synchronize()
    assert (cost.cpu().numpy() != SENT32).all()
