"""GPU tier of the intra chroma mode pre-selection: vvhip_intra_chroma_modes_batch through HotPath.intra_chroma_modes, tolerance 0.

Expected values: the reference's own results recorded in tests/golden/intra_chroma.npz (replayed directly), and the numpy model of tests/intra_chroma_ref.py — which the CPU
tier holds equal to that fixture — on a mixed list.  Outputs land in sentinel-filled tensors: what the entry does not own must come back untouched."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import intra_chroma_cases as CC  # noqa: E402
import intra_chroma_ref as CR  # noqa: E402

COST_SENTINEL, PRED_SENTINEL = -0x12345678, -0x5A5B
E_ARG = "vvenc_hip error -1"
ENTRY = "vvhip_intra_chroma_modes_batch"


@pytest.fixture(scope="module")
def hp():
    from vvenc_amd.hotpath import HotPath
    return HotPath()


def dev(hp, arr):
    import torch
    return torch.from_numpy(np.ascontiguousarray(arr)).to(hp.device)


def run(hp, items, luma, ref, org, npred, guard=64):
    """the entry on sentinel-filled outputs -> ( costs int32 [n][8], pred int16 [npred + guard] ) as numpy"""
    import torch
    cost = torch.full((len(items), CR.NUM_SLOTS), COST_SENTINEL, dtype=torch.int32, device=hp.device)
    pred = torch.full((npred + guard,), PRED_SENTINEL, dtype=torch.int16, device=hp.device)
    hp.intra_chroma_modes(items, None if luma is None else dev(hp, luma), dev(hp, ref), dev(hp, org), cost=cost, pred=pred)
    torch.cuda.synchronize()
    return cost.cpu().numpy(), pred.cpu().numpy()


def item_preds(items, i, pred, shape):
    """the predictions of item i as [ slots of pred_mask ][2][h][w]"""
    n = shape[-1] * shape[-2]
    return np.stack([pred[int(items[i]["pred_off"][c]):int(items[i]["pred_off"][c]) + shape[0] * n].reshape(shape[0], shape[-2], shape[-1]) for c in (0, 1)], axis=1) if shape[0] else np.zeros(shape, np.int16)


def scored_of(mask):
    return np.array([(int(mask) >> s) & 1 for s in range(CR.NUM_SLOTS)], bool)


def test_golden_cases(hp):
    golden = CC.load_golden()
    cl = [g[0] for g in golden.values()]
    items, luma, ref, org, npred = CC.as_list(cl)
    cost, pred = run(hp, items, luma, ref, org, npred)
    assert (pred[npred:] == PRED_SENTINEL).all()
    for i, (name, (c, gcost, _, gpred)) in enumerate(golden.items()):
        scored = scored_of(c.mode_mask)
        assert np.array_equal(cost[i][scored].astype(np.uint32), gcost[scored]), (name, np.argwhere(cost[i].astype(np.uint32) != gcost).reshape(-1).tolist())
        assert (cost[i][~scored] == COST_SENTINEL).all(), name
        assert np.array_equal(item_preds(items, i, pred, gpred.shape), gpred), name


AVAIL = (0, CR.F_ABOVE, CR.F_LEFT, CR.F_ABOVE | CR.F_LEFT)
KINDS = ("smooth", "smooth", "full", "two_level", "overshoot", "steep_neg")


def mixed_cases():
    """a few hundred items: all 16 shapes x the four availability patterns x six seeds — random flags, template counts, candidate lists with random regular modes (two-tap
    modes at 12 bits among them), partial masks, bit depths and patterns mixed"""
    rng = np.random.default_rng(78)
    out = []
    for (w, h) in CC.SHAPES:
        for av in AVAIL:
            for k in range(6):
                bd = (10, 10, 8, 12, 10, 9)[k]
                flags = av | (CR.F_FIRST_ROW if rng.integers(0, 3) == 0 else 0) | (CR.F_VER_COLLOCATED if rng.integers(0, 2) else 0)
                n_ar = 2 * int(rng.integers(0, w // 2 + 1)) if av & CR.F_ABOVE else 0
                n_lb = 2 * int(rng.integers(0, h // 2 + 1)) if av & CR.F_LEFT else 0
                cand = list(CC.cand_list(int(rng.integers(0, 67))))
                if k % 2:
                    cand[:4] = rng.choice(np.arange(2, 67), 4, replace=False).tolist()
                mm = 0xff if k < 3 else int(rng.integers(1, 256))
                pm = mm & (int(rng.integers(0, 256)) if w * h <= 256 else 1 << int(rng.integers(0, 8)))
                out.append(CC.Case("x%d_%dx%d_%d" % (av, w, h, k), w, h, bd, flags, n_ar, n_lb, cand, *CC.fields(rng, w, h, bd, KINDS[k]), mode_mask=mm, pred_mask=pm))
    return out


@pytest.fixture(scope="module")
def mixed(hp):
    """the mixed list: its cases, the model's results (computed once) and the device's"""
    cl = mixed_cases()
    want = [CC.expected(c) for c in cl]
    L = CC.as_list(cl)
    cost, pred = run(hp, *L)
    return cl, want, L, cost, pred


def check(cl, want, items, cost, pred, order=None):
    for j, i in enumerate(order if order is not None else range(len(cl))):
        c, (wc, _, wp) = cl[i], want[i]
        scored = scored_of(c.mode_mask)
        assert np.array_equal(cost[j][scored].astype(np.uint32), wc[scored]) and (cost[j][~scored] == COST_SENTINEL).all(), (c.name, cost[j].tolist(), wc.tolist())
        assert np.array_equal(item_preds(items, j, pred, wp.shape), wp), c.name


def test_mixed_list_equals_the_model(mixed):
    cl, want, (items, luma, ref, org, npred), cost, pred = mixed
    assert len(cl) >= 300 and {(c.w, c.h, c.flags & 3) for c in cl} == {(w, h, a) for (w, h) in CC.SHAPES for a in AVAIL}
    assert any(c.bit_depth == 12 and any(2 < m < 66 and m not in (18, 34, 50) for m in c.cand) for c in cl)
    check(cl, want, items, cost, pred)
    assert (pred[npred:] == PRED_SENTINEL).all()


def test_permuted_list_gives_the_same_items(hp, mixed):
    cl, want, _, cost0, _ = mixed
    order = np.random.default_rng(5).permutation(len(cl))
    items, luma, ref, org, npred = CC.as_list([cl[i] for i in order])
    cost, pred = run(hp, items, luma, ref, org, npred)
    check(cl, want, items, cost, pred, order)
    assert np.array_equal(cost, cost0[order])


def test_two_runs_give_identical_bytes(hp, mixed):
    _, _, L, cost0, pred0 = mixed
    cost, pred = run(hp, *L)
    assert cost.tobytes() == cost0.tobytes() and pred.tobytes() == pred0.tobytes()


def test_partial_masks(hp):
    golden = CC.load_golden()
    names = ["s8x8", "s16x4", "s4x4", "s32x8", "vleft1_4x16", "s32x32", "r3_8x16"]
    full = [golden[n][0] for n in names]
    fitems, fluma, fref, forg, fnpred = CC.as_list(full, pred="all")
    fcost, fpred = run(hp, fitems, fluma, fref, forg, fnpred)
    rng = np.random.default_rng(3)
    part = []
    for c in full:
        mm = int(rng.integers(1, 255))
        part.append(CC.Case(c.name, c.w, c.h, c.bit_depth, c.flags, c.n_ar, c.n_lb, c.cand, c.luma, c.lines, c.org, mm, mm & int(rng.integers(0, 256))))
    items, luma, ref, org, npred = CC.as_list(part)
    cost, pred = run(hp, items, luma, ref, org, npred)
    assert (pred[npred:] == PRED_SENTINEL).all()
    for i, c in enumerate(part):
        for s in range(CR.NUM_SLOTS):
            assert cost[i][s] == (fcost[i][s] if (c.mode_mask >> s) & 1 else COST_SENTINEL), (c.name, s)
        n = c.w * c.h
        for comp in (0, 1):
            for k, s in enumerate(CR.mask_bits(c.pred_mask)):
                o, fo = int(items[i]["pred_off"][comp]) + k * n, int(fitems[i]["pred_off"][comp]) + s * n
                assert np.array_equal(pred[o:o + n], fpred[fo:fo + n]), (c.name, comp, s)
    # costs only: no prediction tensor at all
    import torch
    items, luma, ref, org, npred = CC.as_list(part, pred="none")
    conly = torch.full((len(items), CR.NUM_SLOTS), COST_SENTINEL, dtype=torch.int32, device=hp.device)
    hp.intra_chroma_modes(items, dev(hp, luma), dev(hp, ref), dev(hp, org), cost=conly, pred=None)
    assert npred == 0 and np.array_equal(conly.cpu().numpy(), cost)
    # regular modes only: no luma plane at all
    reg = [CC.Case(c.name, c.w, c.h, c.bit_depth, c.flags, c.n_ar, c.n_lb, c.cand, c.luma, c.lines, c.org, 0x8f, 0x81) for c in full]
    items, luma, ref, org, npred = CC.as_list(reg)
    rcost, rpred = run(hp, items, None, ref, org, npred)
    for i, c in enumerate(reg):
        for s in range(CR.NUM_SLOTS):
            assert rcost[i][s] == (fcost[i][s] if (0x8f >> s) & 1 else COST_SENTINEL), (c.name, s)
        n = c.w * c.h
        for comp in (0, 1):
            for k, s in enumerate((0, 7)):
                o, fo = int(items[i]["pred_off"][comp]) + k * n, int(fitems[i]["pred_off"][comp]) + s * n
                assert np.array_equal(rpred[o:o + n], fpred[fo:fo + n]), (c.name, comp, s)


def test_luma_outside_the_footprint_is_not_read(hp):
    """two clean runs whose luma planes differ in every sample OUTSIDE the documented footprint of each item (the model records every sample loadLMLumaRecPels' restatement
    reads; the header's table is checked against that record first) give the same results, and results that equal the model's"""
    golden = CC.load_golden()
    cl = [g[0] for g in golden.values()]
    items, luma, ref, org, npred = CC.as_list(cl, pred="all")
    keep = np.zeros(luma.size, bool)
    for i, c in enumerate(cl):
        touched = set()
        CC.expected(c, None, touched)
        off, st = int(items[i]["luma_off"]), int(items[i]["luma_stride"])
        t = np.array(sorted(touched), np.int64) + off - (CC.ORG * st + CC.ORG)          # (the model ran on the case's own window: its offsets -> offsets into the list's plane)
        if t.size == 0:
            continue
        y, x = np.floor_divide(t - off + 4 * st + 4, st) - 4, (t - off + 4 * st + 4) % st - 4          # ( x, y ) from the area's top-left sample; x in [ -4, pitch - 4 )
        above, left, first, vc = (bool(c.flags & f) for f in (CR.F_ABOVE, CR.F_LEFT, CR.F_FIRST_ROW, CR.F_VER_COLLOCATED))
        ar, lb = min(c.n_ar, c.h), min(c.n_lb, c.w)
        inner = (y >= (-1 if vc and above else 0)) & (y < 2 * c.h) & (x >= (-1 if left else 0)) & (x < 2 * c.w)
        top = above & (y < 0) & (y >= (-1 if first else (-3 if vc else -2))) & (x >= (-1 if left else 0)) & (x < 2 * (c.w + ar))
        lft = left & (x < 0) & (x >= -3) & (y >= (-1 if vc and above else 0)) & (y < 2 * (c.h + lb))
        assert (inner | top | lft).all(), (c.name, "the model read outside the footprint the header documents")
        keep[t] = True
    assert keep.any() and not keep.all()
    rng = np.random.default_rng(11)
    results = []
    for k in range(2):
        plane = np.where(keep, luma, rng.integers(0, 1 << 12, luma.size).astype(np.int16))
        results.append(run(hp, items, plane, ref, org, npred))
    assert results[0][0].tobytes() == results[1][0].tobytes() and results[0][1].tobytes() == results[1][1].tobytes()
    base = run(hp, items, luma, ref, org, npred)
    assert base[0].tobytes() == results[0][0].tobytes() and base[1].tobytes() == results[0][1].tobytes()


def test_empty_list(hp):
    import torch
    cost = torch.full((4, CR.NUM_SLOTS), COST_SENTINEL, dtype=torch.int32, device=hp.device)
    z = torch.zeros(16, dtype=torch.int16, device=hp.device)
    hp.intra_chroma_modes(np.zeros(0, CR.ITEM_DTYPE), z, z, z, cost=cost, pred=None)
    torch.cuda.synchronize()
    assert (cost.cpu().numpy() == COST_SENTINEL).all()


def _bad(field, value, index=None):
    def f(it):
        if index is None:
            it[1][field] = value
        else:
            it[1][field][index] = value
    return f


def _count_without_side(field, flag):
    def f(it):
        it[1]["flags"] &= ~np.uint8(flag)
        it[1][field] = 2
    return f


def _not_subset(it):
    it[1]["pred_mask"] |= np.uint8(4)
    it[1]["mode_mask"] &= ~np.uint8(4)


ERRORS = {
    "width": _bad("w", 12), "height_2": _bad("h", 2), "width_64": _bad("w", 64), "depth_low": _bad("bit_depth", 7), "depth_high": _bad("bit_depth", 13),
    "cand_70": _bad("cand", 70, 2), "flag_bits": _bad("flags", 0x13), "odd_above_right": _bad("n_above_right", 3), "odd_left_below": _bad("n_left_below", 1),
    "above_right_beyond_w": _bad("n_above_right", 10), "left_below_beyond_h": _bad("n_left_below", 10),          # item 1 is 8x8: w + 2, h + 2
    "above_right_without_above": _count_without_side("n_above_right", CR.F_ABOVE), "left_below_without_left": _count_without_side("n_left_below", CR.F_LEFT),
    "pred_not_subset": _not_subset, "luma_off": _bad("luma_off", -1), "luma_stride": _bad("luma_stride", -8), "ref_off": _bad("ref_off", -1, 1), "org_off": _bad("org_off", -2, 0),
    "pred_off": _bad("pred_off", -1, 1), "cost_off": _bad("cost_off", -8), "rsv": _bad("rsv", 1, 11),
}


MISSING = ("no_items", "no_ref", "no_org", "no_cost")


@pytest.mark.parametrize("what", sorted(ERRORS) + ["n_negative", "no_pred_tensor", "no_luma_plane"] + list(MISSING))
def test_argument_errors_write_nothing(hp, what):
    import ctypes as C
    import torch
    from vvenc_amd.lib import VVHipError
    golden = CC.load_golden()
    cl = [golden[n][0] for n in ("s4x4", "s8x8", "s16x4")]
    items, luma, ref, org, npred = CC.as_list(cl)
    cost = torch.full((len(items), CR.NUM_SLOTS), COST_SENTINEL, dtype=torch.int32, device=hp.device)
    pred = torch.full((npred,), PRED_SENTINEL, dtype=torch.int16, device=hp.device)
    dluma, dref, dorg = dev(hp, luma), dev(hp, ref), dev(hp, org)
    if what == "n_negative" or what in MISSING:
        args = {"no_items": items.ctypes.data_as(C.c_void_p), "no_ref": C.c_void_p(dref.data_ptr()), "no_org": C.c_void_p(dorg.data_ptr()), "no_cost": C.c_void_p(cost.data_ptr())}
        if what in MISSING:
            args[what] = None
        rc = hp.L.vvhip_intra_chroma_modes_batch(hp.ctx, args["no_items"], -1 if what == "n_negative" else len(items), C.c_void_p(dluma.data_ptr()), args["no_ref"], args["no_org"],
                                                 C.c_void_p(pred.data_ptr()), args["no_cost"])
        assert rc == -1 and ENTRY.encode() in hp.L.vvhip_last_error(hp.ctx)
    else:
        if what in ERRORS:
            ERRORS[what](items)
        with pytest.raises(VVHipError) as e:
            hp.intra_chroma_modes(items, None if what == "no_luma_plane" else dluma, dref, dorg, cost=cost, pred=None if what == "no_pred_tensor" else pred)
        assert E_ARG in str(e.value) and ENTRY in str(e.value)
    torch.cuda.synchronize()
    assert (cost.cpu().numpy() == COST_SENTINEL).all() and (pred.cpu().numpy() == PRED_SENTINEL).all()
