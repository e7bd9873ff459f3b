"""GPU tier of the intra luma mode pre-selection: vvhip_intra_luma_modes_batch through HotPath.intra_luma_modes, tolerance 0.

Expected values: the reference's own results recorded in tests/golden/intra.npz (replayed directly), and the numpy model of tests/intra_ref.py — which the CPU tier holds equal
to that fixture — on a mixed list.  Outputs land in sentinel-filled tensors: what the entry does not own must come back untouched."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import intra_cases as IC  # noqa: E402
import intra_ref as IR  # noqa: E402

COST_SENTINEL, PRED_SENTINEL = -0x12345678, -0x5A5B
E_ARG = "vvenc_hip error -1"


@pytest.fixture(scope="module")
def hp():
    from vvenc_amd.hotpath import HotPath
    return HotPath()


def dev(hp, arr):
    import torch
    return torch.from_numpy(np.ascontiguousarray(arr)).to(hp.device)


def run(hp, items, ref, org, npred, guard=64):
    """the entry on sentinel-filled outputs -> ( costs int32 [n][67], pred int16 [npred + guard] ) as numpy"""
    import torch
    cost = torch.full((len(items), IR.NUM_MODES), COST_SENTINEL, dtype=torch.int32, device=hp.device)
    pred = torch.full((npred + guard,), PRED_SENTINEL, dtype=torch.int16, device=hp.device)
    hp.intra_luma_modes(items, dev(hp, ref), dev(hp, org), cost=cost, pred=pred)
    torch.cuda.synchronize()
    return cost.cpu().numpy(), pred.cpu().numpy()


def test_golden_cases(hp):
    golden = IC.load_golden()
    cl = [g[0] for g in golden.values()]
    items, ref, org, npred = IC.as_list(cl)
    cost, pred = run(hp, items, ref, org, npred)
    assert (pred[npred:] == PRED_SENTINEL).all()
    for i, (name, (c, gcost, gpred)) in enumerate(golden.items()):
        scored = np.zeros(IR.NUM_MODES, bool)
        scored[list(c.modes)] = True
        assert np.array_equal(cost[i][scored].astype(np.uint32), gcost[scored]), (name, np.argwhere(cost[i].astype(np.uint32) != gcost).reshape(-1).tolist())
        assert (cost[i][~scored] == COST_SENTINEL).all(), name
        o = int(items[i]["pred_off"])
        assert np.array_equal(pred[o:o + gpred.size].reshape(gpred.shape), gpred), name


def mixed_cases():
    """a few hundred items: every shape x the three multi_ref_idx values x six seeds, about a dozen random modes each (planar only with reference line 0), bit depths mixed"""
    rng = np.random.default_rng(77)
    out = []
    for (w, h) in IC.SHAPES:
        for mri in (0, 1, 2):
            for k in range(6):
                bd = (10, 10, 8, 12, 10, 9)[k]
                lines, org = IC.seeded(rng, w, h, bd, mri)
                modes = sorted(set(rng.choice(np.arange(1 if mri else 0, IR.NUM_MODES), 12, replace=False).tolist()))
                pm = tuple(modes[::5]) if w * h <= 1024 else tuple(modes[:1])
                out.append(IC.Case("x%d_%dx%d_%d" % (mri, w, h, k), w, h, bd, mri, lines, org, modes, pm))
    return out


@pytest.fixture(scope="module")
def mixed(hp):
    """the mixed list: its cases, the model's results (computed once) and the device's"""
    cl = mixed_cases()
    want = [IC.expected(c) for c in cl]
    items, ref, org, npred = IC.as_list(cl)
    cost, pred = run(hp, items, ref, org, npred)
    return cl, want, (items, ref, org, npred), cost, pred


def check(cl, want, items, cost, pred, order=None):
    for j, i in enumerate(order if order is not None else range(len(cl))):
        c, (wc, wp) = cl[i], want[i]
        scored = np.zeros(IR.NUM_MODES, bool)
        scored[list(c.modes)] = True
        assert np.array_equal(cost[j][scored].astype(np.uint32), wc[scored]) and (cost[j][~scored] == COST_SENTINEL).all(), c.name
        o = int(items[j]["pred_off"])
        assert np.array_equal(pred[o:o + wp.size].reshape(wp.shape), wp), c.name


def test_mixed_list_equals_the_model(mixed):
    cl, want, (items, ref, org, npred), cost, pred = mixed
    assert len(cl) >= 250 and {(c.w, c.h, c.mri) for c in cl} == {(w, h, m) for (w, h) in IC.SHAPES for m in (0, 1, 2)}
    check(cl, want, items, cost, pred)
    assert (pred[npred:] == PRED_SENTINEL).all()


def test_permuted_list_gives_the_same_items(hp, mixed):
    cl, want, _, cost0, _ = mixed
    order = np.random.default_rng(5).permutation(len(cl))
    items, ref, org, npred = IC.as_list([cl[i] for i in order])
    cost, pred = run(hp, items, ref, org, npred)
    check(cl, want, items, cost, pred, order)
    assert np.array_equal(cost, cost0[order])


def test_two_runs_give_identical_bytes(hp, mixed):
    _, _, (items, ref, org, npred), cost0, pred0 = mixed
    cost, pred = run(hp, items, ref, org, npred)
    assert cost.tobytes() == cost0.tobytes() and pred.tobytes() == pred0.tobytes()


def test_partial_masks(hp):
    golden = IC.load_golden()
    names = ["s8x8", "s16x4", "s4x4", "s32x8", "m2_4x16", "s32x32"]
    full = [golden[n][0] for n in names]
    fitems, fref, forg, fnpred = IC.as_list(full, pred="all")
    fcost, fpred = run(hp, fitems, fref, forg, fnpred)
    rng = np.random.default_rng(3)
    part = []
    for c in full:
        modes = sorted(rng.choice(c.modes, 9, replace=False).tolist())
        part.append(IC.Case(c.name, c.w, c.h, c.bit_depth, c.mri, c.lines, c.org, modes, modes[1::3]))
    items, ref, org, npred = IC.as_list(part)
    cost, pred = run(hp, items, ref, org, npred)
    assert (pred[npred:] == PRED_SENTINEL).all()
    for i, (c, f) in enumerate(zip(part, full)):
        for m in range(IR.NUM_MODES):
            assert cost[i][m] == (fcost[i][m] if m in c.modes else COST_SENTINEL), (c.name, m)
        n = c.w * c.h
        for k, m in enumerate(c.pred_modes):
            o, fo = int(items[i]["pred_off"]) + k * n, int(fitems[i]["pred_off"]) + f.modes.index(m) * n
            assert np.array_equal(pred[o:o + n], fpred[fo:fo + n]), (c.name, m)
    # costs only: no prediction tensor at all
    items, ref, org, npred = IC.as_list(part, pred="none")
    import torch
    conly = torch.full((len(items), IR.NUM_MODES), COST_SENTINEL, dtype=torch.int32, device=hp.device)
    hp.intra_luma_modes(items, dev(hp, ref), dev(hp, org), cost=conly, pred=None)
    assert npred == 0 and np.array_equal(conly.cpu().numpy(), cost)


def test_empty_list(hp):
    import torch
    cost = torch.full((4, IR.NUM_MODES), COST_SENTINEL, dtype=torch.int32, device=hp.device)
    z = torch.zeros(16, dtype=torch.int16, device=hp.device)
    hp.intra_luma_modes(np.zeros(0, IR.ITEM_DTYPE), z, z, cost=cost, pred=None)
    torch.cuda.synchronize()
    assert (cost.cpu().numpy() == COST_SENTINEL).all()


def _bad(field, value):
    def f(it):
        it[1][field] = value
    return f


def _mask_bit(field, word, bit, extra=None):
    def f(it):
        it[1][field][word] |= np.uint32(1 << bit)
        if extra:
            it[1][extra][word] |= np.uint32(1 << bit)
    return f


def _planar_mrl(it):
    it[1]["multi_ref_idx"] = 1
    it[1]["mode_mask"][0] |= np.uint32(1)


def _not_subset(it):
    it[1]["pred_mask"][0] |= np.uint32(4)
    it[1]["mode_mask"][0] &= ~np.uint32(4)


ERRORS = {
    "width": _bad("w", 12), "height": _bad("h", 2), "height_128": _bad("h", 128), "depth_low": _bad("bit_depth", 7), "depth_high": _bad("bit_depth", 13),
    "multi_ref_idx": _bad("multi_ref_idx", 3), "planar_with_mrl": _planar_mrl, "mode_bit_67": _mask_bit("mode_mask", 2, 3), "pred_bit_67": _mask_bit("pred_mask", 2, 3, "mode_mask"),
    "pred_not_subset": _not_subset,
    "ref_off": _bad("ref_off", -1), "org_off": _bad("org_off", -2), "pred_off": _bad("pred_off", -1), "cost_off": _bad("cost_off", -67), "rsv": _bad("rsv", 1),
}


@pytest.mark.parametrize("what", sorted(ERRORS) + ["n_negative", "no_pred_tensor"])
def test_argument_errors_write_nothing(hp, what):
    import ctypes as C
    import torch
    from vvenc_amd.lib import VVHipError
    golden = IC.load_golden()
    cl = [golden[n][0] for n in ("s4x4", "s8x8", "s16x4")]
    items, ref, org, npred = IC.as_list(cl)
    cost = torch.full((len(items), IR.NUM_MODES), COST_SENTINEL, dtype=torch.int32, device=hp.device)
    pred = torch.full((npred,), PRED_SENTINEL, dtype=torch.int16, device=hp.device)
    dref, dorg = dev(hp, ref), dev(hp, org)
    if what == "n_negative":
        rc = hp.L.vvhip_intra_luma_modes_batch(hp.ctx, items.ctypes.data_as(C.c_void_p), -1, C.c_void_p(dref.data_ptr()), C.c_void_p(dorg.data_ptr()), C.c_void_p(pred.data_ptr()), C.c_void_p(cost.data_ptr()))
        assert rc == -1 and b"vvhip_intra_luma_modes_batch" in hp.L.vvhip_last_error(hp.ctx)
    else:
        if what != "no_pred_tensor":
            ERRORS[what](items)
        with pytest.raises(VVHipError) as e:
            hp.intra_luma_modes(items, dref, dorg, cost=cost, pred=None if what == "no_pred_tensor" else pred)
        assert E_ARG in str(e.value) and "vvhip_intra_luma_modes_batch" in str(e.value)
    torch.cuda.synchronize()
    assert (cost.cpu().numpy() == COST_SENTINEL).all() and (pred.cpu().numpy() == PRED_SENTINEL).all()
