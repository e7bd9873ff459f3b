"""GPU tier of the affine prediction entry: vvhip_pred_affine_batch against the model of tests/affine_ref.py (anchored on the reference's own xPredAffineBlk by
tests/golden/affine.npz, see tests/test_affine_cpu.py), tolerance 0.  Every interpolation pass of the expected values is executed from the compiled reference (the `reflib`
rows) or from its C restatement; the lists come from tests/affine_cases.py, where the CPU guards check what they exercise."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import affine_cases as AC  # noqa: E402
import affine_ref as AR  # noqa: E402
import pred_ref as PR  # noqa: E402

SENTINEL = -7


@pytest.fixture(scope="module")
def hp():
    from vvenc_amd.hotpath import HotPath
    return HotPath()


class Dev:
    """the planes of an affine_cases.World (or of the golden fixture) on the device"""

    def __init__(self, hp, planes, org=None):
        self.dev = [hp.plane(a, 0) for a in planes]
        for a, p in zip(planes, self.dev):
            assert p.stride == a.shape[1]
        self.org = [hp.plane(a, 0) for a in org] if org is not None else None


def run(hp, dev, items, bd, pic_w, pic_h, ctu, org=None, stride=0, total=None):
    """compact run (dst_off must be set) -> (pred, resi or None) as numpy"""
    import torch
    if total is None:
        total = AC.compact_offsets(items)[1]
    pred = torch.full((total,), SENTINEL, dtype=torch.int16, device=hp.device)
    resi = torch.full((total,), SENTINEL, dtype=torch.int16, device=hp.device) if org is not None else None
    hp.pred_affine_batch(dev.dev, items, pred, stride, bd, pic_w, pic_h, ctu, org, resi)
    torch.cuda.synchronize()
    return pred.cpu().numpy(), (resi.cpu().numpy() if resi is not None else None)


def with_offsets(items):
    items = items.copy()
    items["dst_off"] = AC.compact_offsets(items)[0]
    return items


def block_of(buf, it):
    c = int(it["chroma"])
    bw, bh = int(it["cu_w"]) >> c, int(it["cu_h"]) >> c
    return buf[int(it["dst_off"]):int(it["dst_off"]) + bw * bh].reshape(bh, bw)


def check(pred, items, pos, world, lib, what):
    for k in range(len(items)):
        e = AR.expected_block(lib, world.np, pos[k], items[k], world.bd, world.pic_w, world.pic_h, world.ctu)
        g = block_of(pred, items[k])
        assert np.array_equal(g, e), (what, getattr(lib, "name", "oracle"), k, items[k], np.argwhere(g != e)[:3].tolist())


_device_results = {}


def _tier(hp, key):
    """the device's output for one list of AC.TIER_LISTS, computed once and shared by the two reference rows"""
    if key not in _device_results:
        bd, D, seed = key
        world = AC.World(bd, 128, seed=seed)
        items, pos = AC.size_list(world, D, seed)
        items = with_offsets(items)
        pred, _ = run(hp, Dev(hp, world.np), items, bd, world.pic_w, world.pic_h, world.ctu)
        _device_results[key] = (world, items, pos, pred)
    return _device_results[key]


# ---- 1 ----
@pytest.mark.parametrize("key", AC.TIER_LISTS, ids=["%dbit-D%d" % (k[0], k[1]) for k in AC.TIER_LISTS])
def test_every_cu_size_against_the_model(hp, reflib, key):
    """every CU size 8..128 x 8..128, luma and chroma, both models, list 0 / list 1 / both, prof 0..3, at this bit depth and D: device == model on the reference row"""
    world, items, pos, pred = _tier(hp, key)
    assert {(int(i["cu_w"]), int(i["cu_h"]), int(i["chroma"])) for i in items} == {(w, h, c) for (w, h) in AR.SIZES for c in (0, 1)}
    combos = {(int(i["six_param"]), tuple(int(p) >= 0 for p in i["ref_plane"]), int(i["prof"])) for i in items}
    assert len(combos) == 24
    check(pred, items, pos, world, reflib, "sizes")
    assert pred.min() >= 0          # every sample of the compact buffer was written


# ---- 2 ----
def test_golden_cases_on_the_device(hp):
    """the cases the reference's own xPredAffineBlk recorded, run from the fixture's planes: device == recorded output (two lists: the default average of the two recorded blocks)"""
    (pic_w, pic_h, ctu, _), planes, cases = AC.golden_cases()
    for bd in (8, 10):
        sel = [c for c in cases if c[0] == bd]
        assert len(sel) >= 10
        items = with_offsets(np.concatenate([np.stack([lu, ch]) for (_, lu, ch, _, _) in sel]))
        pred, _ = run(hp, Dev(hp, planes[bd]), items, bd, pic_w, pic_h, ctu)
        for k, (_, lu, ch, pos, rec) in enumerate(sel):
            for cc in (0, 1):
                blocks = [rec["scalar"][(l, cc)] for l in (0, 1) if (l, cc) in rec["scalar"]]
                e = blocks[0] if len(blocks) == 1 else PR.bi_average(blocks[0], blocks[1], bd)
                g = block_of(pred, items[2 * k + cc])
                assert np.array_equal(g, e), (bd, k, cc, items[2 * k + cc], np.argwhere(g != e)[:3].tolist())


# ---- 3 ----
def test_prof_off_equals_the_expanded_list_on_the_device(hp):
    """prof = 0 items == vvhip_pred_inter_batch on the same CUs expanded by the host into 4x4 items: device against device"""
    import torch
    from vvenc_amd.hotpath import PRED_ITEM_DTYPE
    world = AC.World(10, 128, seed=41)
    items, _ = AC.size_list(world, 32, 41, reps=1)
    items["prof"] = 0
    items = with_offsets(items)
    dev = Dev(hp, world.np)
    pred, _ = run(hp, dev, items, 10, world.pic_w, world.pic_h, world.ctu)
    strides = [a.shape[1] for a in world.np]
    ex = []
    for k in range(len(items)):
        e, _, _ = AR.expand_items(items[k], strides, world.pic_w, world.pic_h, world.ctu, PRED_ITEM_DTYPE)
        e["dst_off"] += int(items[k]["dst_off"])
        ex.append(e)
    ex = np.concatenate(ex)
    out = torch.full((pred.size,), SENTINEL, dtype=torch.int16, device=hp.device)
    hp.pred_inter_batch(dev.dev, ex, out, 0, 10)
    out = out.cpu().numpy()
    for k in range(len(items)):
        c = int(items[k]["chroma"])
        bw, bh = int(items[k]["cu_w"]) >> c, int(items[k]["cu_h"]) >> c
        o = int(items[k]["dst_off"])
        assert np.array_equal(AR.blocks_to_block(out[o:o + bw * bh], bw, bh), block_of(pred, items[k])), (k, items[k])


# ---- 4 ----
@pytest.mark.parametrize("ctu", [32, 64, 128])
def test_picture_edges_and_corners(hp, oracle, ctu):
    """CUs at the four edges and corners with vectors more than ctu samples outward: the picture clip, reads inside the margin of ctu + 16"""
    world = AC.World(10, ctu, seed=ctu)
    items, pos = AC.edge_list(world, ctu)
    items = with_offsets(items)
    pred, _ = run(hp, Dev(hp, world.np), items, 10, world.pic_w, world.pic_h, ctu)
    check(pred, items, pos, world, oracle, "edges ctu %d" % ctu)


# ---- 5 ----
@pytest.mark.parametrize("bd", [8, 10])
@pytest.mark.parametrize("kind", ["zero", "max", "checker"])
def test_extremes(hp, oracle, kind, bd):
    """planes all 0, all max and checkerboards of 0 / max; model deltas that drive dMv to +-31 and, on the checkerboard, dI into its clip"""
    world = AC.World(bd, 128, kind, seed=9)
    items, pos = AC.extreme_list(world, 9)
    items = with_offsets(items)
    pred, _ = run(hp, Dev(hp, world.np), items, bd, world.pic_w, world.pic_h, world.ctu)
    check(pred, items, pos, world, oracle, "extremes %s %d bit" % (kind, bd))
    if kind != "checker":
        assert np.all(pred == (0 if kind == "zero" else (1 << bd) - 1))


# ---- 6 ----
def test_outputs_compact_strided_and_residual(hp, oracle):
    """compact blocks and blocks inside a plane hold the same samples; the residual is org - expected in both layouts; nothing is written outside the blocks"""
    import torch
    world = AC.World(10, 64, seed=77)
    items, pos = AC.size_list(world, 32, 77, reps=1)
    keep = [k for k in range(len(items)) if int(items[k]["cu_w"]) * int(items[k]["cu_h"]) <= 64 * 64]
    items, pos = with_offsets(items[keep]), [pos[k] for k in keep]
    dev = Dev(hp, world.np, world.org_np)
    lum, chr_ = np.flatnonzero(items["chroma"] == 0), np.flatnonzero(items["chroma"] == 1)
    for comp, idx in ((0, lum), (1, chr_)):          # one original pitch per call: one call per component
        it = with_offsets(items[idx])
        pred, resi = run(hp, dev, it, 10, world.pic_w, world.pic_h, world.ctu, org=dev.org[comp])
        ps = [pos[k] for k in idx]
        check(pred, it, ps, world, oracle, "compact")
        sizes = [(int(i["cu_w"]) >> comp, int(i["cu_h"]) >> comp) for i in it]
        for k in range(len(it)):
            bw, bh = sizes[k]
            x, y = world.block_pos(it[k])
            assert np.array_equal(block_of(resi, it[k]), PR.residual(world.org_np[comp][y:y + bh, x:x + bw], block_of(pred, it[k]))), ("residual", comp, k)
        # into a plane of pitch 520 at odd positions (unaligned rows), with its residual
        pw = 520
        where, rows = PR.shelf_pack([(w + 1, h + 1) for (w, h) in sizes], pw)
        itp = it.copy()
        itp["dst_off"] = [(y + 1) * pw + x + 1 for (x, y) in where]
        plane = torch.full(((rows + 2) * pw,), SENTINEL, dtype=torch.int16, device=hp.device)
        rplane = torch.full(((rows + 2) * pw,), SENTINEL, dtype=torch.int16, device=hp.device)
        hp.pred_affine_batch(dev.dev, itp, plane, pw, 10, world.pic_w, world.pic_h, world.ctu, dev.org[comp], rplane)
        out, rout = plane.cpu().numpy().reshape(rows + 2, pw), rplane.cpu().numpy().reshape(rows + 2, pw)
        mask = np.zeros((rows + 2, pw), bool)
        for k, (x, y) in enumerate(where):
            bw, bh = sizes[k]
            assert np.array_equal(out[y + 1:y + 1 + bh, x + 1:x + 1 + bw], block_of(pred, it[k])), ("plane output", comp, k)
            assert np.array_equal(rout[y + 1:y + 1 + bh, x + 1:x + 1 + bw], block_of(resi, it[k])), ("plane residual", comp, k)
            mask[y + 1:y + 1 + bh, x + 1:x + 1 + bw] = True
        assert np.all(out[~mask] == SENTINEL) and np.all(rout[~mask] == SENTINEL)


# ---- 7 ----
def test_schedule_and_cache(hp, oracle):
    """order independence; the same list twice; the same items with another prof give other values (the schedule is not reused); alternating with a plain
    vvhip_pred_inter_batch list on the same context keeps both right"""
    import torch
    from vvenc_amd.hotpath import PRED_ITEM_DTYPE
    world = AC.World(10, 64, seed=88)
    items, pos = AC.size_list(world, 32, 88, reps=1)
    keep = [k for k in range(len(items)) if int(items[k]["cu_w"]) * int(items[k]["cu_h"]) <= 64 * 32]
    items, pos = with_offsets(items[keep]), [pos[k] for k in keep]
    dev = Dev(hp, world.np)
    total = AC.compact_offsets(items)[1]
    first, _ = run(hp, dev, items, 10, world.pic_w, world.pic_h, world.ctu)
    check(first, items, pos, world, oracle, "cache: first run")
    rng = np.random.default_rng(5)
    for order in (rng.permutation(len(items)), np.arange(len(items))[::-1], np.arange(len(items)), np.arange(len(items))):          # (the last two: the same list twice)
        again, _ = run(hp, dev, items[order], 10, world.pic_w, world.pic_h, world.ctu, total=total)
        assert np.array_equal(again, first)
    # another prof: other values, and the right ones
    other = items.copy()
    other["prof"] = np.where(items["prof"] == 0, 1, 0)
    second, _ = run(hp, dev, other, 10, world.pic_w, world.pic_h, world.ctu)
    assert not np.array_equal(second, first)
    check(second, other, pos, world, oracle, "cache: other prof")
    # alternating with a plain list: neither schedule is evicted or mixed up
    plain = np.zeros(6, PRED_ITEM_DTYPE)
    ppos = []
    for k in range(6):
        plain[k]["width"], plain[k]["height"], plain[k]["ref_plane"], plain[k]["frac"][0], plain[k]["dst_off"] = 16, 8, (k & 1, -1), (3 + k, 2 * k), 128 * k
        x, y = world.m + 24 * k, world.m + 10 + 7 * k
        plain[k]["ref_off"][0] = y * world.np[0].shape[1] + x
        ppos.append([(x, y), None])
    for _ in range(3):
        a, _ = run(hp, dev, items, 10, world.pic_w, world.pic_h, world.ctu)
        out = torch.full((128 * 6,), SENTINEL, dtype=torch.int16, device=hp.device)
        hp.pred_inter_batch(dev.dev, plain, out, 0, 10)
        out = out.cpu().numpy()
        assert np.array_equal(a, first)
        for k in range(6):
            assert np.array_equal(out[128 * k:128 * k + 128].reshape(8, 16), PR.expected_block(oracle, world.np, ppos[k], plain[k], 10)), k


# ---- 8 ----
def test_affine_argument_errors(hp):
    """every invalid input fails with VVHIP_E_ARG and a message that names the entry; nothing is launched (the output keeps its fill); the context stays usable"""
    import torch
    from vvenc_amd.lib import VVHipError
    world = AC.World(10, 64, seed=99)
    dev = Dev(hp, world.np)
    rng = np.random.default_rng(1)
    good, _ = AC.finish(world, [AC._cu(rng, 16, 16, 32 * k, 16, 0, 0, 1, 32)[0] for k in range(3)])
    good = with_offsets(good)

    def broken(field, value):
        b = good.copy()
        b[field][2] = value
        return b
    cases = [(broken("cu_w", 4), 64), (broken("cu_h", 256), 64), (broken("cu_w", 24), 64),          # below 8, above 128, not a power of two
             (broken("ref_plane", (-1, -1)), 64),                                                    # neither list used
             (broken("ref_plane", (9, -1)), 64),                                                     # plane outside the table
             (broken("chroma", 2), 64), (broken("prof", 4), 64), (broken("rsv", (0, 1, 0)), 64),
             (good, 48), (good, 256),                                                                # CTU size not 32 / 64 / 128
             (broken("cu_x", world.pic_w - 8), 64), (broken("cu_y", -8), 64)]                        # CU outside the picture
    for k, (items, ctu) in enumerate(cases):
        pred = torch.full((3 * 256,), SENTINEL, dtype=torch.int16, device=hp.device)
        with pytest.raises(VVHipError) as e:
            hp.pred_affine_batch(dev.dev, items, pred, 0, 10, world.pic_w, world.pic_h, ctu)
        assert "vvhip_pred_affine_batch" in str(e.value) and "error -1" in str(e.value), (k, str(e.value))
        torch.cuda.synchronize()
        assert np.all(pred.cpu().numpy() == SENTINEL), k
    pred, _ = run(hp, dev, good, 10, world.pic_w, world.pic_h, 64)
    assert pred.min() >= 0
