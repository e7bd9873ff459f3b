"""GPU tier of the CIIP form of the prediction list: vvhip_pred_inter_batch_ciip (planar intra part and weighting), tolerance 0.

Expected values: the reference's own results recorded in tests/golden/ciip.npz (replayed directly), and tests/ciip_ref.py — the inter part executed from the C
restatement of the reference (the `oracle` fixture), the four CIIP steps restated in numpy there and pinned to the fixture by tests/test_ciip_cpu.py.  The lists come
from tests/ciip_cases.py; tests/test_ciip_cpu.py asserts what they cover."""
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
import ciip_cases as CC  # noqa: E402
import ciip_ref as CR  # noqa: E402
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


def dev_lines(hp, lines):
    import torch
    return torch.from_numpy(np.ascontiguousarray(lines, np.int16)).to(hp.device)


def run_compact(hp, world, items, ext, blend, ciip, lines, org=False):
    import torch
    items = items.copy()
    off, total = BLC.compact_offsets(items)
    items["dst_off"] = off
    pred = torch.full((total,), SENTINEL, dtype=torch.int16, device=hp.device)
    resi = torch.full((total,), SENTINEL, dtype=torch.int16, device=hp.device) if org else None
    hp.pred_inter_batch(world.dev, items, pred, 0, world.bd, world.org if org else None, resi, ext=ext, blend=blend, ciip=ciip, intra_ref=lines)
    torch.cuda.synchronize()
    return items, pred.cpu().numpy(), (resi.cpu().numpy() if org else None)


def blocks_of(buf, items):
    return [buf[int(it["dst_off"]):int(it["dst_off"]) + int(it["width"]) * int(it["height"])].reshape(int(it["height"]), int(it["width"])) for it in items]


# ---- 1 ----
def test_replay_of_the_reference_fixture(hp):
    """every fixture case as one uni-predicted item with a zero fraction on a plane that holds the case's inter block, all cases in one list: the output is the result
    the reference recorded, on every case.  (One call has one bit depth: the list runs at 10 bits, where the zero-fraction inter part of an 8-bit block is the block
    itself as well — ( 1024 s + 512 ) >> 10 = s, below the 10-bit clip — and nothing in the CIIP steps depends on the bit depth.)"""
    import torch
    cases = CR.golden_cases()
    plane, items, ciip, lines = CC.golden_replay_list(cases)
    dev = [hp.plane(plane, 0)]
    assert dev[0].stride == plane.shape[1]
    total = BLC.compact_offsets(items)[1]
    pred = torch.full((total,), SENTINEL, dtype=torch.int16, device=hp.device)
    hp.pred_inter_batch(dev, items, pred, 0, 10, ciip=ciip, intra_ref=dev_lines(hp, lines))
    got = blocks_of(pred.cpu().numpy(), items)
    assert len(got) == len(cases) >= 150
    for i, (g, c) in enumerate(zip(got, cases)):
        assert np.array_equal(g, c["result"]), (i, c["bd"], c["w"], c["h"], c["chroma"], c["num_intra"], np.argwhere(g != c["result"])[:3].tolist())
    # and without the records the same list is the inter blocks themselves
    plain = torch.full((total,), SENTINEL, dtype=torch.int16, device=hp.device)
    hp.pred_inter_batch(dev, items, plain, 0, 10)
    for g, c in zip(blocks_of(plain.cpu().numpy(), items), cases):
        assert np.array_equal(g, c["inter"])


# ---- 2 ----
@pytest.mark.parametrize("bd", [10, 8])
def test_every_size_against_the_model(hp, oracle, bd):
    """every luma and chroma size as uni, bi, BCW 0 and BCW 4 items at fractional phases (the 64x64, 64x32 and 32x64 luma items are cut into tiles): compact with the
    residual, in a plane, and in shuffled order"""
    import torch
    world = world_of(hp, bd)
    items, ext, blend, ciip, lines, pos = CC.model_list(world.np, 600 + bd)
    dl = dev_lines(hp, lines)
    rng = np.random.default_rng(43)
    H, W = world.org_np.shape
    for i, it in enumerate(items):
        items["org_off"][i] = int(rng.integers(0, H - 1 - int(it["height"]) + 1)) * world.org.stride + int(rng.integers(0, W - int(it["width"]) + 1))
    its, pred, resi = run_compact(hp, world, items, None, blend, ciip, dl, org=True)
    exp = [CC.expected(oracle, world.np, pos[i], it, ext[i], blend[i], ciip[i], lines, bd) for i, it in enumerate(its)]
    for i, (p, r, it) in enumerate(zip(blocks_of(pred, its), blocks_of(resi, its), its)):
        assert np.array_equal(p, exp[i]), ("compact", i, it, blend[i], ciip[i], np.argwhere(p != exp[i])[:3].tolist())
        oy, ox = divmod(int(it["org_off"]), world.org.stride)
        assert np.array_equal(r, PR.residual(world.org_np[oy:oy + int(it["height"]), ox:ox + int(it["width"])], exp[i])), ("residual", i)
    for order in (rng.permutation(len(its)), np.arange(len(its))[::-1]):
        out = torch.full((pred.size,), SENTINEL, dtype=torch.int16, device=hp.device)
        hp.pred_inter_batch(world.dev, its[order], out, 0, bd, blend=blend[order], ciip=ciip[order], intra_ref=dl)
        assert np.array_equal(out.cpu().numpy(), pred)
    pw = 512
    where, rows = PR.shelf_pack([(int(i["width"]), int(i["height"])) for i in items], pw)
    itp = items.copy()
    itp["dst_off"] = [y * pw + x for (x, y) in where]
    plane, rplane = (torch.full((rows * pw,), SENTINEL, dtype=torch.int16, device=hp.device) for _ in range(2))
    hp.pred_inter_batch(world.dev, itp, plane, pw, bd, world.org, rplane, blend=blend, ciip=ciip, intra_ref=dl)
    out, rout = plane.cpu().numpy().reshape(rows, pw), rplane.cpu().numpy().reshape(rows, pw)
    mask = np.zeros((rows, pw), bool)
    for i, (it, (x, y)) in enumerate(zip(itp, where)):
        w, h = int(it["width"]), int(it["height"])
        assert np.array_equal(out[y:y + h, x:x + w], exp[i]), ("plane output", i, it)
        oy, ox = divmod(int(it["org_off"]), world.org.stride)
        assert np.array_equal(rout[y:y + h, x:x + w], PR.residual(world.org_np[oy:oy + h, ox:ox + w], exp[i])), ("plane residual", i)
        mask[y:y + h, x:x + w] = True
    assert np.all(out[~mask] == SENTINEL) and np.all(rout[~mask] == SENTINEL)


# ---- 3 ----
def test_without_on_records_it_is_the_blend_entry(hp, oracle):
    """on a mixed list (plain, BDOF, DMVR, BCW, GEO): ciip = NULL and an array with every record OFF give bit for bit the blend entry's output; with OFF and ON records
    mixed the OFF items keep that output and the ON items are the model's"""
    world = world_of(hp, 10)
    items, ext, blend, ciip, lines, pos = CC.mixed_on_off(world.np, 510)
    its, base, _ = run_compact(hp, world, items, ext, blend, None, None)
    assert base.min() >= 0
    off = np.zeros(len(items), CC.PRED_CIIP_DTYPE)
    assert np.array_equal(run_compact(hp, world, items, ext, blend, off, None)[1], base)
    assert np.array_equal(run_compact(hp, world, items, ext, blend, off, dev_lines(hp, lines))[1], base)
    _, mixed, _ = run_compact(hp, world, items, ext, blend, ciip, dev_lines(hp, lines))
    n_on = 0
    for i, (g, b, it) in enumerate(zip(blocks_of(mixed, its), blocks_of(base, its), its)):
        if int(ciip[i]["mode"]) == CR.CIIP_OFF:
            assert np.array_equal(g, b), ("OFF item", i, it)
        else:
            e = CC.expected(oracle, world.np, pos[i], it, ext[i], blend[i], ciip[i], lines, 10)
            assert np.array_equal(g, e) and not np.array_equal(g, b), ("ON item", i, it, blend[i], ciip[i])
            n_on += 1
    assert n_on >= 8


# ---- 4 and 5 ----
def test_reference_samples_change_between_runs_and_nothing_is_evicted(hp, oracle):
    """the contents of intra_ref are data, not schedule: other samples at the same address change the output accordingly while repeated runs allocate nothing on the
    device; the same items with other CIIP records are another list; alternating with the plain, the blend and the affine entry on one context leaves every entry's
    output unchanged and allocates nothing (a list with a CIIP array has a schedule slot of its own)"""
    import torch
    world = world_of(hp, 10)
    items, ext, blend, ciip, lines, pos = CC.model_list(world.np, 610)
    keep = np.arange(0, len(items), 3)
    items, blend, ciip, pos, ext = items[keep].copy(), blend[keep], ciip[keep], [pos[i] for i in keep], ext[keep]
    dl = dev_lines(hp, lines)
    its, pred, _ = run_compact(hp, world, items, None, blend, ciip, dl)

    o = torch.full((pred.size,), SENTINEL, dtype=torch.int16, device=hp.device)          # (every device tensor of this test exists before free memory is first read)

    def again(ci=ciip, bl=blend):
        o.fill_(SENTINEL)
        hp.pred_inter_batch(world.dev, its, o, 0, 10, blend=bl, ciip=ci, intra_ref=dl)
        return o.cpu().numpy()
    exp = [CC.expected(oracle, world.np, pos[i], it, ext[i], blend[i], ciip[i], lines, 10) for i, it in enumerate(its)]
    assert all(np.array_equal(g, e) for g, e in zip(blocks_of(pred, its), exp))
    lines2 = np.where(lines >= 0, 1023 - lines, lines).astype(np.int16)
    dl1, dl2 = dev_lines(hp, lines), dev_lines(hp, lines2)
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info()[0]
    dl.copy_(dl2)          # other samples at the same address
    for _ in range(3):
        hp.pred_inter_batch(world.dev, its, o, 0, 10, blend=blend, ciip=ciip, intra_ref=dl)
    torch.cuda.synchronize()
    assert torch.cuda.mem_get_info()[0] == free0
    got2 = o.cpu().numpy()
    exp2 = [CC.expected(oracle, world.np, pos[i], it, ext[i], blend[i], ciip[i], lines2, 10) for i, it in enumerate(its)]
    assert all(np.array_equal(g, e) for g, e in zip(blocks_of(got2, its), exp2)) and not np.array_equal(got2, pred)
    dl.copy_(dl1)
    assert np.array_equal(again(), pred)
    other = ciip.copy()
    other["num_intra"] = (other["num_intra"] + 1) % 3
    assert not np.array_equal(again(other), pred)
    assert np.array_equal(again(), pred)
    # alternating with the other entries, each with a list of its own size
    plain_items = its[blend["mode"] == BL.BLEND_DEFAULT][:7].copy()
    plain_items["dst_off"], ntot = BLC.compact_offsets(plain_items)
    bitems, _, bblend, _ = BLC.bcw_list(world.np, 300)
    bitems = bitems[:11].copy()
    bitems["dst_off"], btot = BLC.compact_offsets(bitems)
    aw = AC.World(10, 128, seed=7)
    aitems, _ = AC.size_list(aw, 16, 7)
    aitems = aitems[:12].copy()
    aitems["dst_off"], atot = AC.compact_offsets(aitems)
    adev = [hp.plane(a, 0) for a in aw.np]
    first, free1 = None, None
    o1, o2, o3 = (torch.empty((t,), dtype=torch.int16, device=hp.device) for t in (ntot, btot, atot))
    for rnd in range(3):
        for t in (o1, o2, o3):
            t.fill_(SENTINEL)
        hp.pred_inter_batch(world.dev, plain_items, o1, 0, 10)
        hp.pred_inter_batch(world.dev, bitems, o2, 0, 10, blend=bblend[:11])
        hp.pred_affine_batch(adev, aitems, o3, 0, 10, aw.pic_w, aw.pic_h, aw.ctu)
        assert np.array_equal(again(), pred)
        got = (o1.cpu().numpy(), o2.cpu().numpy(), o3.cpu().numpy())
        assert all(g.min() >= 0 for g in got)
        if first is None:
            first = got
        assert all(np.array_equal(g, f) for g, f in zip(got, first))
        torch.cuda.synchronize()
        if rnd == 0:
            free1 = torch.cuda.mem_get_info()[0]          # every entry has built its schedule once
        assert torch.cuda.mem_get_info()[0] == free1
    # the plain entry's first output is what the list gives without its CIIP records
    for g, it, p in zip(blocks_of(first[0], plain_items), plain_items, [pos[i] for i in np.flatnonzero(blend["mode"] == BL.BLEND_DEFAULT)[:7]]):
        assert np.array_equal(g, PR.expected_block(oracle, world.np, p, it, 10))


# ---- 6 ----
def test_ciip_argument_errors(hp):
    """every argument error of the CIIP record returns VVHIP_E_ARG with a message naming the entry, launches nothing and leaves the context usable"""
    import torch
    from vvenc_amd.lib import VVHipError
    world = world_of(hp, 10)
    good = np.zeros(3, CC.PRED_ITEM_DTYPE)
    for k in range(3):
        good[k]["width"], good[k]["height"], good[k]["ref_plane"] = 16, 16, (0, 1)
        good[k]["ref_off"] = 20 * world.dev[0].stride + 20
        good[k]["dst_off"] = 256 * k
    gciip = np.zeros(3, CC.PRED_CIIP_DTYPE)
    gciip["mode"], gciip["num_intra"], gciip["ref_off"] = CR.CIIP_ON, 1, (0, 40, 80)
    gblend, gext = np.zeros(3, CC.PRED_BLEND_DTYPE), np.zeros(3, CC.PRED_EXT_DTYPE)
    lines = dev_lines(hp, np.full(128, 500, np.int16))

    def case(item_changes=(), ciip_changes=(), blend_changes=(), ext_changes=(), no_lines=False):
        it, ci, bl, ex = good.copy(), gciip.copy(), gblend.copy(), gext.copy()
        for arr, changes in ((it, item_changes), (ci, ciip_changes), (bl, blend_changes), (ex, ext_changes)):
            for f, v in changes:
                arr[f][2] = v
        return it, ci, bl, ex, no_lines
    chroma = [("chroma", 1), ("ref_plane", (2, 3))]
    cases = [case((), [("mode", 2)]),                                                          # unknown mode
             case((), [("mode", 255)]),
             case((), [("num_intra", 3)]),                                                     # num_intra out of range
             case((), [("rsv", (1, 0))]),                                                      # non-zero reserved bytes
             case((), [("mode", CR.CIIP_OFF), ("rsv", (0, 9))]),
             case((), [("ref_off", -1)]),                                                      # a negative offset
             case([("width", 4), ("height", 4)]),                                              # luma sizes outside the set
             case([("width", 4), ("height", 8)]),
             case([("width", 8), ("height", 4)]),
             case([("width", 128), ("height", 16)]),
             case([("width", 16), ("height", 128)]),
             case(chroma + [("width", 2), ("height", 8)]),                                     # chroma sizes outside the set
             case(chroma + [("width", 4), ("height", 2)]),
             case(chroma + [("width", 64), ("height", 16)]),
             case(chroma + [("width", 16), ("height", 64)]),
             case((), (), [("mode", BL.BLEND_GEO), ("param", 5)]),                             # CIIP on a GEO item
             case((), (), (), [("flags", 1)]),                                                 # CIIP with BDOF, with DMVR's padded reference
             case((), (), (), [("flags", 2), ("pad_dx", (1, 0))]),
             case(no_lines=True)]                                                              # no reference samples while a record is ON
    for k, (it, ci, bl, ex, no_lines) in enumerate(cases):
        pred = torch.full((768,), SENTINEL, dtype=torch.int16, device=hp.device)
        with pytest.raises(VVHipError) as e:
            hp.pred_inter_batch(world.dev, it, pred, 0, 10, ext=ex, blend=bl, ciip=ci, intra_ref=None if no_lines else lines)
        assert "vvhip_pred_inter_batch_ciip" in str(e.value) and "error -1" in str(e.value), (k, str(e.value))
        torch.cuda.synchronize()
        assert np.all(pred.cpu().numpy() == SENTINEL), k
    # the rules of the other records still hold through this entry
    for changes in (dict(blend_changes=[("mode", 3)]), dict(ext_changes=[("flags", 4)]), dict(item_changes=[("width", 24)])):
        it, ci, bl, ex, _ = case(**changes)
        pred = torch.full((768,), SENTINEL, dtype=torch.int16, device=hp.device)
        with pytest.raises(VVHipError):
            hp.pred_inter_batch(world.dev, it, pred, 0, 10, ext=ex, blend=bl, ciip=ci, intra_ref=lines)
        assert np.all(pred.cpu().numpy() == SENTINEL)
    # a cached list run again WITHOUT its reference samples is refused too, and then runs again with them: the context is still usable
    pred = torch.full((768,), SENTINEL, dtype=torch.int16, device=hp.device)
    hp.pred_inter_batch(world.dev, good, pred, 0, 10, ext=gext, blend=gblend, ciip=gciip, intra_ref=lines)
    first = pred.cpu().numpy()
    assert first.min() >= 0
    pred2 = torch.full((768,), SENTINEL, dtype=torch.int16, device=hp.device)
    with pytest.raises(VVHipError) as e:
        hp.pred_inter_batch(world.dev, good, pred2, 0, 10, ext=gext, blend=gblend, ciip=gciip, intra_ref=None)
    assert "vvhip_pred_inter_batch_ciip" in str(e.value)
    assert np.all(pred2.cpu().numpy() == SENTINEL)
    hp.pred_inter_batch(world.dev, good, pred2, 0, 10, ext=gext, blend=gblend, ciip=gciip, intra_ref=lines)
    assert np.array_equal(pred2.cpu().numpy(), first)
