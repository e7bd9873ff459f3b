"""GPU tier of the blend forms of the prediction list: vvhip_pred_inter_batch_blend (BCW weights, GEO partitions), tolerance 0.

Expected values: tests/blend_ref.py — the interpolation of each hypothesis executed from the C restatement of the reference (the `oracle` fixture), the blend restated
in numpy there and anchored to the reference's own xWeightedGeoBlk / addWeightedAvg by tests/golden/blend.npz (tests/test_blend_cpu.py), which this file also runs the
device against directly.  The lists come from tests/blend_cases.py; tests/test_blend_cpu.py asserts their margins, their disjoint outputs and that ignoring the blend
record gives other values on them."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import affine_cases as AC  # noqa: E402
import blend_cases as BLC  # noqa: E402
import blend_ref as BL  # noqa: E402
import pred_ref as PR  # noqa: E402

SENTINEL = -7


@pytest.fixture(scope="module")
def hp():
    from vvenc_amd.hotpath import HotPath
    return HotPath()


class World:
    def __init__(self, hp, bd, seed):
        self.bd = bd
        self.np, self.org_np = BLC.planes(bd, seed)
        self.dev = [hp.plane(a, 0) for a in self.np]
        for a, p in zip(self.np, self.dev):
            assert p.stride == a.shape[1]
        self.org = hp.plane(self.org_np, 0)


_worlds = {}


def world_of(hp, bd):
    if bd not in _worlds:
        _worlds[bd] = World(hp, bd, 100 + bd)
    return _worlds[bd]


def run_compact(hp, world, items, ext, blend, org=False):
    import torch
    items = items.copy()
    off, total = BLC.compact_offsets(items)
    items["dst_off"] = off
    pred = torch.full((total,), SENTINEL, dtype=torch.int16, device=hp.device)
    resi = torch.full((total,), SENTINEL, dtype=torch.int16, device=hp.device) if org else None
    hp.pred_inter_batch(world.dev, items, pred, 0, world.bd, world.org if org else None, resi, ext=ext, blend=blend)
    torch.cuda.synchronize()
    return items, pred.cpu().numpy(), (resi.cpu().numpy() if org else None)


def blocks_of(buf, items):
    return [buf[int(it["dst_off"]):int(it["dst_off"]) + int(it["width"]) * int(it["height"])].reshape(int(it["height"]), int(it["width"])) for it in items]


def check_blocks(got, items, ext, blend, pos, world, lib, what):
    for i, (g, it) in enumerate(zip(got, items)):
        e = BLC.expected(lib, world.np, pos[i], it, ext[i], blend[i], world.bd)
        assert np.array_equal(g, e), (what, i, it, ext[i], blend[i], pos[i], np.argwhere(g != e)[:3].tolist())


_geo_runs = {}


def geo_run(hp, bd):
    """the GEO list of one bit depth on the device, once for the tests that look at it"""
    if bd not in _geo_runs:
        world = world_of(hp, bd)
        items, ext, blend, pos = BLC.geo_list(world.np, 200 + bd, BL.GEO_SIZES if bd == 10 else BLC.GEO_8BIT)
        its, pred, _ = run_compact(hp, world, items, None, blend)
        _geo_runs[bd] = (world, its, ext, blend, pos, pred)
    return _geo_runs[bd]


# ---- 1 ----
@pytest.mark.parametrize("bd", [10, 8])
def test_geo_every_split_direction_and_size(hp, oracle, bd):
    """10 bit: 64 split directions x 16 CU sizes, each CU as its luma and its chroma block — 2048 items in one call; 8 bit: the 8x8, 8x32, 32x8 and 64x64 CUs.
    Seeded fractions, zero fractions on one or both axes, phase 8 with alt_hpel; hypotheses from two planes, swapped, and from one plane twice"""
    world, its, ext, blend, pos, pred = geo_run(hp, bd)
    assert len(its) == (2048 if bd == 10 else 512)
    check_blocks(blocks_of(pred, its), its, ext, blend, pos, world, oracle, "GEO %d bit" % bd)


# ---- 2 ----
@pytest.mark.parametrize("bd", [10, 8])
def test_bcw_every_index_and_kernel_form(hp, oracle, bd):
    """the five indices on luma 4x4, 4x64, 8x8, 16x16, 64x16, 128x128 and chroma 2x2, 2x8, 4x4, 8x4, 64x64; two planes and one plane twice"""
    world = world_of(hp, bd)
    items, ext, blend, pos = BLC.bcw_list(world.np, 300 + bd)
    its, pred, _ = run_compact(hp, world, items, None, blend)
    check_blocks(blocks_of(pred, its), its, ext, blend, pos, world, oracle, "BCW %d bit" % bd)


def test_golden_weight_blocks_on_the_device(hp):
    """the device against the recorded weight blocks directly: on a flat plane of 16 against a flat plane of 0 at fraction zero the 14-bit blocks are -7936 and -8192,
    and ( -7936 w0 - 8192 ( 8 - w0 ) + 64 + 65536 ) >> 7 = ( 256 w0 + 64 ) >> 7 = 2 w0 at 10 bit — for all 2048 blocks: output == 2 x what the reference function returned"""
    import torch
    z = np.load(os.path.join(ROOT, "tests", "golden", "blend.npz"))
    ref = z["weights_scalar"]
    W = 96
    p0, p1 = np.full((80, W), 16, np.int16), np.zeros((80, W), np.int16)
    dev = [hp.plane(p0, 0), hp.plane(p1, 0)]
    assert all(d.stride == W for d in dev)
    import blend_golden_gen as GEN
    wb = GEN.weight_blocks()
    items, blend = np.zeros(len(wb), BLC.PRED_ITEM_DTYPE), np.zeros(len(wb), BLC.PRED_BLEND_DTYPE)
    for k, (sd, w, h, c) in enumerate(wb):
        items[k]["width"], items[k]["height"], items[k]["chroma"], items[k]["ref_plane"], items[k]["ref_off"] = w >> c, h >> c, c, (0, 1), 8 * W + 8
        blend[k] = (BL.BLEND_GEO, sd, (0, 0))
    off, total = BLC.compact_offsets(items)
    items["dst_off"] = off
    assert total == ref.size
    pred = torch.full((total,), SENTINEL, dtype=torch.int16, device=hp.device)
    hp.pred_inter_batch(dev, items, pred, 0, 10, blend=blend)
    got = pred.cpu().numpy()
    assert np.array_equal(got, 2 * ref.astype(np.int16)), np.argwhere(got != 2 * ref)[:3].tolist()


# ---- 3 ----
def test_bcw_default_index_is_the_plain_entry(hp):
    """(a) bcw_idx = 2 on every item == the same list with blend = NULL, through the blend entry and through the plain one"""
    world = world_of(hp, 10)
    items, ext, blend, pos = BLC.bcw_list(world.np, 310)
    blend = blend.copy()
    blend["param"] = 2
    _, with_bcw, _ = run_compact(hp, world, items, None, blend)
    _, plain, _ = run_compact(hp, world, items, None, None)
    assert with_bcw.min() >= 0 and np.array_equal(with_bcw, plain)
    none = blend.copy()
    none["mode"], none["param"] = BL.BLEND_DEFAULT, 0
    _, default_mode, _ = run_compact(hp, world, items, None, none)
    assert np.array_equal(default_mode, plain)


def test_geo_full_weights_are_the_uni_prediction(hp):
    """(b) in the GEO list's output every sample whose weight is 8 (0) equals the uni-prediction of hypothesis 0 (1) from the plain entry: ( 8 s + offset ) >> shift is
    the rounding of rndRes = 1.  The compared share: 42.9 % of all samples have weight 8 and 46.8 % weight 0 over the 2048 blocks (tests/test_blend_cpu.py confirms it
    from the fixture) — 89.7 % together; at least 80 % is asserted"""
    world, its, ext, blend, pos, pred = geo_run(hp, 10)
    uni = []
    for l in (0, 1):
        one = its.copy()
        one["ref_plane"][:, 1 - l] = -1
        uni.append(run_compact(hp, world, one, None, None)[1])
    wts = np.concatenate([BL.geo_weights(int(b["param"]), int(i["width"]) << int(i["chroma"]), int(i["height"]) << int(i["chroma"]), int(i["chroma"])).reshape(-1)
                          for i, b in zip(its, blend)])
    assert wts.size == pred.size
    full0, full1 = wts == 8, wts == 0
    share = float(full0.mean() + full1.mean())
    print("samples with weight 8: %.4f, weight 0: %.4f, compared %.4f" % (full0.mean(), full1.mean(), share))
    assert share >= 0.80
    assert np.array_equal(pred[full0], uni[0][full0]) and np.array_equal(pred[full1], uni[1][full1])
    assert not np.array_equal(pred[~(full0 | full1)], uni[0][~(full0 | full1)])


# ---- 4 ----
@pytest.mark.parametrize("bd", [10, 8])
def test_extremes_reach_both_clip_ends(hp, oracle, bd):
    """the 0 / max checkerboards against each other, BCW 0 and 4 (weights 10 : -2 and -2 : 10) and GEO edges through the block: exact, and both clip ends are reached
    by both tools on both components"""
    world = world_of(hp, bd)
    top = (1 << bd) - 1
    items, ext, blend, pos = BLC.extremes_list(world.np, 400 + bd)
    its, pred, _ = run_compact(hp, world, items, None, blend)
    got = blocks_of(pred, its)
    check_blocks(got, its, ext, blend, pos, world, oracle, "extremes %d bit" % bd)
    assert pred.min() == 0 and pred.max() == top
    for mode in (BL.BLEND_BCW, BL.BLEND_GEO):
        for chroma in (0, 1):
            mine = [g for g, i, b in zip(got, its, blend) if int(b["mode"]) == mode and int(i["chroma"]) == chroma]
            assert any((g == 0).any() for g in mine) and any((g == top).any() for g in mine), (mode, chroma)


# ---- 5 ----
def test_mixed_list_orders_layouts_residual_and_caches(hp, oracle):
    """plain, BDOF, DMVR-pad, BCW and GEO items in one list: equal under two orders; compact and in a plane; resi == org - pred; the same list again reuses its
    schedule; alternating with the plain entry and with vvhip_pred_affine_batch evicts nothing"""
    import torch
    world = world_of(hp, 10)
    items, ext, blend, pos = BLC.mixed_list(world.np, 510)
    rng = np.random.default_rng(42)
    H, W = world.org_np.shape
    for i, it in enumerate(items):
        items["org_off"][i] = int(rng.integers(0, H - 1 - int(it["height"]) + 1)) * world.org.stride + int(rng.integers(0, W - int(it["width"]) + 1))
    its, pred, resi = run_compact(hp, world, items, ext, blend, org=True)
    exp = [BLC.expected(oracle, world.np, pos[i], it, ext[i], blend[i], 10) for i, it in enumerate(its)]
    for i, (p, r, it) in enumerate(zip(blocks_of(pred, its), blocks_of(resi, its), its)):
        assert np.array_equal(p, exp[i]), ("compact", i, it, ext[i], blend[i])
        oy, ox = divmod(int(it["org_off"]), world.org.stride)
        assert np.array_equal(r, PR.residual(world.org_np[oy:oy + int(it["height"]), ox:ox + int(it["width"])], exp[i])), ("residual", i)
    # two other orders of the same list
    for order in (rng.permutation(len(its)), np.arange(len(its))[::-1]):
        out = torch.full((pred.size,), SENTINEL, dtype=torch.int16, device=hp.device)
        hp.pred_inter_batch(world.dev, its[order], out, 0, 10, ext=ext[order], blend=blend[order])
        assert np.array_equal(out.cpu().numpy(), pred)
    # in a plane
    pw = 512
    where, rows = PR.shelf_pack([(int(i["width"]), int(i["height"])) for i in items], pw)
    itp = items.copy()
    itp["dst_off"] = [y * pw + x for (x, y) in where]
    plane, rplane = (torch.full((rows * pw,), SENTINEL, dtype=torch.int16, device=hp.device) for _ in range(2))
    hp.pred_inter_batch(world.dev, itp, plane, pw, 10, world.org, rplane, ext=ext, blend=blend)
    out, rout = plane.cpu().numpy().reshape(rows, pw), rplane.cpu().numpy().reshape(rows, pw)
    mask = np.zeros((rows, pw), bool)
    for i, (it, (x, y)) in enumerate(zip(itp, where)):
        w, h = int(it["width"]), int(it["height"])
        assert np.array_equal(out[y:y + h, x:x + w], exp[i]), ("plane output", i, it)
        oy, ox = divmod(int(it["org_off"]), world.org.stride)
        assert np.array_equal(rout[y:y + h, x:x + w], PR.residual(world.org_np[oy:oy + h, ox:ox + w], exp[i])), ("plane residual", i)
        mask[y:y + h, x:x + w] = True
    assert np.all(out[~mask] == SENTINEL) and np.all(rout[~mask] == SENTINEL)

    # the schedule cache: the same list again allocates nothing on the device and gives the same samples; the same items with other blend records are another list
    def again(bl):
        o = torch.full((pred.size,), SENTINEL, dtype=torch.int16, device=hp.device)
        hp.pred_inter_batch(world.dev, its, o, 0, 10, ext=ext, blend=bl)
        return o.cpu().numpy()
    assert np.array_equal(again(blend), pred)
    o = torch.full((pred.size,), SENTINEL, dtype=torch.int16, device=hp.device)
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info()[0]
    for _ in range(3):
        hp.pred_inter_batch(world.dev, its, o, 0, 10, ext=ext, blend=blend)
    torch.cuda.synchronize()
    assert torch.cuda.mem_get_info()[0] == free0 and np.array_equal(o.cpu().numpy(), pred)
    other = blend.copy()
    other["param"][other["mode"] == BL.BLEND_BCW] = 2
    assert not np.array_equal(again(other), pred)
    assert np.array_equal(again(blend), pred)
    # alternating with the plain entry (a smaller list: its schedule must not be read for the blend list, nor the other way round) and with the affine entry
    plain_items = its[blend["mode"] == BL.BLEND_DEFAULT][:7].copy()
    plain_ext = ext[blend["mode"] == BL.BLEND_DEFAULT][:7]
    plain_items["dst_off"] = BLC.compact_offsets(plain_items)[0]
    ntot = BLC.compact_offsets(plain_items)[1]
    aw = AC.World(10, 128, seed=7)
    aitems, _ = AC.size_list(aw, 16, 7)
    aitems = aitems[:12].copy()
    aoff, atot = AC.compact_offsets(aitems)
    aitems["dst_off"] = aoff
    adev = [hp.plane(a, 0) for a in aw.np]
    first = None
    for _ in range(2):
        o1 = torch.full((ntot,), SENTINEL, dtype=torch.int16, device=hp.device)
        hp.pred_inter_batch(world.dev, plain_items, o1, 0, 10, ext=plain_ext)
        o2 = torch.full((atot,), SENTINEL, dtype=torch.int16, device=hp.device)
        hp.pred_affine_batch(adev, aitems, o2, 0, 10, aw.pic_w, aw.pic_h, aw.ctu)
        assert np.array_equal(again(blend), pred)
        got = (o1.cpu().numpy(), o2.cpu().numpy())
        assert got[0].min() >= 0 and got[1].min() >= 0
        if first is None:
            first = got
        assert np.array_equal(got[0], first[0]) and np.array_equal(got[1], first[1])


# ---- 6 ----
def test_blend_argument_errors(hp):
    """every argument error of the blend record returns VVHIP_E_ARG with a message naming the entry, launches nothing and leaves the context usable"""
    import torch
    from vvenc_amd.lib import VVHipError
    world = world_of(hp, 10)
    good = np.zeros(3, BLC.PRED_ITEM_DTYPE)
    for k in range(3):
        good[k]["width"], good[k]["height"], good[k]["ref_plane"] = 16, 16, (0, 1)
        good[k]["ref_off"] = 20 * world.dev[0].stride + 20
        good[k]["dst_off"] = 256 * k
    gblend = np.zeros(3, BLC.PRED_BLEND_DTYPE)
    gblend["mode"], gblend["param"] = BL.BLEND_GEO, 5
    gext = np.zeros(3, BLC.PRED_EXT_DTYPE)

    def case(item_changes=(), blend_changes=(), ext_changes=()):
        it, bl, ex = good.copy(), gblend.copy(), gext.copy()
        for f, v in item_changes:
            it[f][2] = v
        for f, v in blend_changes:
            bl[f][2] = v
        for f, v in ext_changes:
            ex[f][2] = v
        return it, bl, ex
    cases = [case((), [("mode", 3)]),                                                          # unknown mode
             case((), [("mode", 255)]),
             case((), [("param", 64)]),                                                        # GEO split direction out of range
             case((), [("mode", BL.BLEND_BCW), ("param", 5)]),                                 # BCW index out of range
             case((), [("rsv", (1, 0))]),                                                      # non-zero reserved bytes
             case((), [("mode", BL.BLEND_DEFAULT), ("param", 0), ("rsv", (0, 7))]),
             case([("ref_plane", (0, -1))]),                                                   # GEO with one hypothesis
             case([("ref_plane", (-1, 1))], [("mode", BL.BLEND_BCW), ("param", 0)]),           # BCW with one hypothesis
             case([("width", 4), ("height", 8)]),                                              # GEO sizes outside the set
             case([("width", 128), ("height", 64)]),
             case([("width", 16), ("height", 4)]),
             case([("chroma", 1), ("ref_plane", (2, 3)), ("width", 2), ("height", 4)]),
             case([("chroma", 1), ("ref_plane", (2, 3)), ("width", 64), ("height", 32)]),
             case((), (), [("flags", 1)]),                                                     # GEO with BDOF, with DMVR's padded reference
             case((), (), [("flags", 2)]),
             case((), [("mode", BL.BLEND_BCW), ("param", 1)], [("flags", 1)]),                 # BCW likewise
             case((), [("mode", BL.BLEND_BCW), ("param", 1)], [("flags", 2), ("pad_dx", (1, 0))])]
    for k, (it, bl, ex) in enumerate(cases):
        pred = torch.full((768,), SENTINEL, dtype=torch.int16, device=hp.device)
        with pytest.raises(VVHipError) as e:
            hp.pred_inter_batch(world.dev, it, pred, 0, 10, ext=ex, blend=bl)
        assert "vvhip_pred_inter_batch_blend" in str(e.value) and "error -1" in str(e.value), (k, str(e.value))
        torch.cuda.synchronize()
        assert np.all(pred.cpu().numpy() == SENTINEL), k
    # the extension's own rules still hold through this entry: flag bit 4 and non-zero reserved bytes of vvhip_pred_ext
    for f, v in (("flags", 4), ("rsv", (0, 1, 0))):
        it, bl, ex = case((), [("mode", BL.BLEND_DEFAULT), ("param", 0)], [(f, v)])
        pred = torch.full((768,), SENTINEL, dtype=torch.int16, device=hp.device)
        with pytest.raises(VVHipError):
            hp.pred_inter_batch(world.dev, it, pred, 0, 10, ext=ex, blend=bl)
        assert np.all(pred.cpu().numpy() == SENTINEL)
    pred = torch.full((768,), SENTINEL, dtype=torch.int16, device=hp.device)          # the context is still usable
    hp.pred_inter_batch(world.dev, good, pred, 0, 10, ext=gext, blend=gblend)
    assert pred.cpu().numpy().min() >= 0
