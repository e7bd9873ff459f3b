"""GPU tier of the extension forms of the prediction list: vvhip_pred_inter_batch_ex (BDOF, DMVR's padded reference), tolerance 0.

Expected values: tests/bdof_ref.py — the interpolation of each list executed from the compiled reference (scalar row and x86 row, the `reflib` fixture), for DMVR
items on an edge-padded copy of the prefetched window; the BDOF steps restated in numpy there and anchored to the reference's own xApplyBDOF by tests/golden/bdof.npz
(tests/test_bdof_cpu.py), which this file also runs the device against directly.  The lists come from tests/bdof_cases.py; tests/test_bdof_cpu.py asserts on the model
alone that ignoring a flag gives other values on them."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import bdof_cases as BC  # noqa: E402
import bdof_ref as BR  # noqa: E402
import pred_ref as PR  # noqa: E402

SENTINEL = -7


@pytest.fixture(scope="module")
def hp():
    from vvenc_amd.hotpath import HotPath
    return HotPath()


class World:
    def __init__(self, hp, bd, seed):
        self.bd = bd
        self.np, self.org_np = BC.planes(bd, seed)
        self.dev = [hp.plane(a, 0) for a in self.np]
        for a, p in zip(self.np, self.dev):
            assert p.stride == a.shape[1]
        self.org = hp.plane(self.org_np, 0)


_worlds = {}


def world_of(hp, bd, seed):
    if (bd, seed) not in _worlds:
        _worlds[(bd, seed)] = World(hp, bd, seed)
    return _worlds[(bd, seed)]


def run_compact(hp, world, items, ext, org=False):
    import torch
    items = items.copy()
    off, total = BC.compact_offsets(items)
    items["dst_off"] = off
    pred = torch.full((total,), SENTINEL, dtype=torch.int16, device=hp.device)
    resi = torch.full((total,), SENTINEL, dtype=torch.int16, device=hp.device) if org else None
    hp.pred_inter_batch(world.dev, items, pred, 0, world.bd, world.org if org else None, resi, ext=ext)
    torch.cuda.synchronize()
    return items, pred.cpu().numpy(), resi


def blocks_of(buf, items):
    return [buf[int(it["dst_off"]):int(it["dst_off"]) + int(it["width"]) * int(it["height"])].reshape(int(it["height"]), int(it["width"])) for it in items]


def check_blocks(got, items, ext, pos, world, lib, what):
    for i, (g, it) in enumerate(zip(got, items)):
        e = BR.expected_block_ex(lib, world.np, pos[i], it, ext[i], world.bd)
        assert np.array_equal(g, e), (what, lib.name, i, it, ext[i], pos[i], np.argwhere(g != e)[:3].tolist())


def plane_from_frame(frame, bd):
    """a reference plane whose integer samples, read with fraction zero, give exactly this frame: v = ( f + 8192 ) >> headroom (only for frames made of such values)"""
    hr = max(2, 14 - bd)
    v = (frame.astype(np.int32) + 8192) >> hr
    assert np.array_equal(((v << hr) - 8192).astype(np.int16), frame) and v.min() >= 0 and v.max() < (1 << bd)
    return v.astype(np.int16)


# ---- 1 ----
@pytest.mark.parametrize("bd", [10, 8])
def test_bdof_every_size_and_phase(hp, reflib, bd):
    """every luma size 8..128 x 8..128 that passes the size rule, all 16 x 16 phases across the list, alt_hpel, blocks at the margin limits, the all-zero and all-max
    planes, identical references in both lists"""
    world = world_of(hp, bd, 100 + bd)
    items, ext, pos = BC.bdof_list(world.np, 200 + bd)
    assert {(int(i["width"]), int(i["height"])) for i in items} == set(BC.BDOF_SIZES) and len(BC.BDOF_SIZES) == 24
    assert len({tuple(i["frac"][0]) for i in items}) == 256
    its, pred, _ = run_compact(hp, world, items, ext)
    check_blocks(blocks_of(pred, its), its, ext, pos, world, reflib, "BDOF %d bit" % bd)


# ---- 2 ----
def test_bdof_golden_cases_on_the_device(hp):
    """the recorded cases of the reference's xApplyBDOF whose frames a reference plane can produce (fraction zero: the 14-bit block and the ring are both
    ( sample << headroom ) - 8192): flat blocks, the extreme values 0 and max, pictures — device output == the reference's recorded output"""
    import torch
    z = np.load(os.path.join(ROOT, "tests", "golden", "bdof.npz"))
    ran = {}
    for bd in (8, 10):
        planes, recs, want = [], [], []
        for i in range(int(z["n"])):
            hdr = z["c%03d_hdr" % i]
            if int(hdr[0]) != bd:
                continue
            f0, f1 = z["c%03d_f0" % i], z["c%03d_f1" % i]
            try:
                p0, p1 = plane_from_frame(f0, bd), plane_from_frame(f1, bd)
            except AssertionError:
                continue
            planes.append((p0, p1)); want.append(z["c%03d_scalar" % i]); recs.append((int(hdr[1]), int(hdr[2])))
        assert len(planes) >= 30
        # all frames of one list side by side in one plane, 8 samples of margin round each
        cell = 16 + 2 + 16
        W = (cell * len(planes) + 16 + 7) // 8 * 8          # (planes are allocated with a row pitch that is a multiple of 8)
        big = [np.zeros((cell + 1, W), np.int16) for _ in (0, 1)]
        items, ext = np.zeros(len(planes), BC.PRED_ITEM_DTYPE), np.zeros(len(planes), BC.PRED_EXT_DTYPE)
        for k, ((p0, p1), (w, h)) in enumerate(zip(planes, recs)):
            for l, p in enumerate((p0, p1)):
                big[l][8:8 + h + 2, 8 + k * cell:8 + k * cell + w + 2] = p
                items[k]["ref_off"][l] = 9 * W + 9 + k * cell          # fraction 0 < 8: the frame's origin is one sample up and left of the block
            items[k]["width"], items[k]["height"], items[k]["ref_plane"], ext[k]["flags"] = w, h, (0, 1), BR.EXT_BDOF
        off, total = BC.compact_offsets(items)
        items["dst_off"] = off
        dev = [hp.plane(b, 0) for b in big]
        assert all(d.stride == W for d in dev)
        pred = torch.full((total,), SENTINEL, dtype=torch.int16, device=hp.device)
        hp.pred_inter_batch(dev, items, pred, 0, bd, ext=ext)
        for k, (g, e) in enumerate(zip(blocks_of(pred.cpu().numpy(), items), want)):
            assert np.array_equal(g, e), (bd, k, recs[k])
        ran[bd] = len(planes)
    print("golden cases run on the device:", ran)


# ---- 3 ----
@pytest.mark.parametrize("bd", [10, 8])
def test_dmvr_every_delta_and_shape(hp, reflib, bd):
    """all 25 integer deltas x sub-block shapes 8x8 / 16x8 / 8x16 / 16x16, luma with and without BDOF, chroma (9 deltas); clamp windows touching the plane margin"""
    world = world_of(hp, bd, 100 + bd)
    items, ext, pos = BC.dmvr_list(world.np, 300 + bd)
    luma = [(int(i["width"]), int(i["height"]), int(e["pad_dx"][0]), int(e["pad_dy"][0]), int(e["flags"]) & 1) for i, e in zip(items, ext) if not int(i["chroma"]) and int(i["ref_plane"][1]) >= 0]
    for (w, h) in BC.DMVR_SHAPES:
        for dy in range(-2, 3):
            for dx in range(-2, 3):
                assert (w, h, dx, dy, 0) in luma and ((w, h, dx, dy, 1) in luma or (w, h) == (8, 8))
    x0, x1, y0, y1 = BC.limits(world.np[0], 16, 16, 0)
    starts = [(p[0][0] - int(e["pad_dx"][0]), p[0][1] - int(e["pad_dy"][0])) for i, e, p in zip(items, ext, pos) if (int(i["width"]), int(i["height"]), int(i["chroma"])) == (16, 16, 0)]
    assert any(s[0] == x0 for s in starts) and any(s[0] == x1 for s in starts) and any(s[1] == y0 for s in starts) and any(s[1] == y1 for s in starts)
    its, pred, _ = run_compact(hp, world, items, ext)
    check_blocks(blocks_of(pred, its), its, ext, pos, world, reflib, "DMVR %d bit" % bd)


# ---- 4 ----
def test_mixed_launch_compact_strided_residual(hp, reflib):
    """one launch mixing BDOF items, DMVR items, plain bi, uni and chroma items: compact and strided output, with the residual"""
    import torch
    world = world_of(hp, 10, 110)
    items, ext, pos = BC.mixed_list(world.np, 41)
    rng = np.random.default_rng(42)
    H, W = world.org_np.shape
    for i, it in enumerate(items):
        items["org_off"][i] = int(rng.integers(0, H - int(it["height"]) + 1)) * world.org.stride + int(rng.integers(0, W - int(it["width"]) + 1))
    its, pred, d_resi = run_compact(hp, world, items, ext, org=True)
    resi = d_resi.cpu().numpy()
    exp = [BR.expected_block_ex(reflib, world.np, pos[i], it, ext[i], 10) for i, it in enumerate(its)]
    for i, (p, r, it) in enumerate(zip(blocks_of(pred, its), blocks_of(resi, its), its)):
        assert np.array_equal(p, exp[i]), ("compact", reflib.name, i, it, ext[i])
        oy, ox = divmod(int(it["org_off"]), world.org.stride)
        assert np.array_equal(r, PR.residual(world.org_np[oy:oy + int(it["height"]), ox:ox + int(it["width"])], exp[i])), ("residual", i)
    pw = 512
    where, rows = PR.shelf_pack([(int(i["width"]), int(i["height"])) for i in items], pw)
    itp = items.copy()
    itp["dst_off"] = [y * pw + x for (x, y) in where]
    plane, rplane = (torch.full((rows * pw,), SENTINEL, dtype=torch.int16, device=hp.device) for _ in range(2))
    hp.pred_inter_batch(world.dev, itp, plane, pw, 10, world.org, rplane, ext=ext)
    out, rout = plane.cpu().numpy().reshape(rows, pw), rplane.cpu().numpy().reshape(rows, pw)
    mask = np.zeros((rows, pw), bool)
    for i, (it, (x, y)) in enumerate(zip(itp, where)):
        w, h = int(it["width"]), int(it["height"])
        assert np.array_equal(out[y:y + h, x:x + w], exp[i]), ("plane output", i, it)
        oy, ox = divmod(int(it["org_off"]), world.org.stride)
        assert np.array_equal(rout[y:y + h, x:x + w], PR.residual(world.org_np[oy:oy + h, ox:ox + w], exp[i])), ("plane residual", i)
        mask[y:y + h, x:x + w] = True
    assert np.all(out[~mask] == SENTINEL) and np.all(rout[~mask] == SENTINEL)


# ---- 5 ----
def test_bdof_residual_feeds_the_tu_pipeline(hp, oracle):
    """the residual of a BDOF list is a d_resi of vvhip_tu_rdo_multi_strided: levels, reconstruction and statistics equal the same call on the expected residual"""
    import torch
    from oracle.oracle import RefLib
    from vvenc_amd.hotpath import STATS_DTYPE, HotPath
    lib = RefLib(1) if RefLib.available() else oracle
    world = world_of(hp, 10, 110)
    b = BC.ListBuilder(world.np, 51)
    for S in (16, 32, 64):
        for k in range(6):
            b.add(S, S, 0, 0, ((int(b.rng.integers(0, 16)), int(b.rng.integers(0, 16))), (int(b.rng.integers(0, 16)), int(b.rng.integers(0, 16)))), (k & 1, 1 - (k & 1)), BR.EXT_BDOF)
    items, ext, pos = b.done()
    for i in range(len(items)):
        items["org_off"][i] = pos[i][0][1] * world.org.stride + pos[i][0][0]
    its, pred, d_resi = run_compact(hp, world, items, ext, org=True)
    exp_resi = np.full(pred.shape, SENTINEL, np.int16)
    for i, it in enumerate(its):
        w, h = int(it["width"]), int(it["height"])
        e = BR.expected_block_ex(lib, world.np, pos[i], it, ext[i], 10)
        oy, ox = divmod(int(it["org_off"]), world.org.stride)
        exp_resi[int(it["dst_off"]):int(it["dst_off"]) + w * h] = PR.residual(world.org_np[oy:oy + h, ox:ox + w], e).reshape(-1)
    assert np.array_equal(d_resi.cpu().numpy(), exp_resi)
    d_exp = hp.to_device(exp_resi)
    results = []
    for src in (d_resi, d_exp):
        jobs, strides = [], []
        r2 = np.random.default_rng(63)
        for (w, h) in ((16, 16), (32, 32), (64, 64)):
            idx = [i for i, it in enumerate(its) if (int(it["width"]), int(it["height"])) == (w, h)]
            n = len(idx)
            off = hp.to_device(its["dst_off"][idx].astype(np.int32))
            qp = hp.to_device(HotPath.tu_qp(r2.integers(22, 48, n), 1, 1))
            lev = torch.full((n * w * h,), 0x7777, dtype=torch.int16, device=hp.device)
            rec = torch.full((n * w * h,), 0x5555, dtype=torch.int16, device=hp.device)
            st = torch.full((n, STATS_DTYPE.itemsize), 0xEE, dtype=torch.uint8, device=hp.device)
            jobs.append((w, h, 0, 0, n, 8, off, qp, lev, rec, st))
            strides.append(w)
        hp.tu_rdo_multi_strided(src, strides, jobs, 10)
        torch.cuda.synchronize()
        results.append([(j[8].cpu().numpy(), j[9].cpu().numpy(), j[10].cpu().numpy()) for j in jobs])
    for a, bb in zip(*results):
        for x, y in zip(a, bb):
            assert np.array_equal(x, y)
    assert any(r[0].any() for r in results[0])


# ---- 6 ----
def test_order_cache_and_stale_schedules(hp):
    """order independence under a shuffle; the same list run twice (schedule cache); the same items with other extensions must not reuse a stale schedule;
    ext = None and all-zero extensions are bit-equal to vvhip_pred_inter_batch"""
    import torch
    world = world_of(hp, 10, 110)
    i1, e1, _ = BC.mixed_list(world.np, 71)
    i2, e2, _ = BC.bdof_list(world.np, 72)
    items, ext = np.concatenate([i1, i2[::5]]), np.concatenate([e1, e2[::5]])
    off, total = BC.compact_offsets(items)
    items["dst_off"] = off

    def run(it, ex):
        pred = torch.full((total,), SENTINEL, dtype=torch.int16, device=hp.device)
        hp.pred_inter_batch(world.dev, it, pred, 0, 10, ext=ex)
        return pred.cpu().numpy()
    base = run(items, ext)
    assert base.min() >= 0
    rng = np.random.default_rng(5)
    for order in (rng.permutation(len(items)), np.arange(len(items))[::-1]):
        assert np.array_equal(run(items[order], ext[order]), base)
    assert np.array_equal(run(items, ext), base) and np.array_equal(run(items, ext), base)          # the cached schedule, twice
    # the same items, other extensions: BDOF off where it was on
    off_ext = ext.copy()
    off_ext["flags"] &= ~np.uint8(BR.EXT_BDOF)
    plain = run(items, off_ext)
    assert not np.array_equal(plain, base)
    assert np.array_equal(run(items, ext), base)
    # no extension at all == the old entry, on items whose deltas are zero
    keep = (ext["pad_dx"] == 0).all(axis=1) & (ext["pad_dy"] == 0).all(axis=1)
    it0 = items[keep].copy()
    o0, total0 = BC.compact_offsets(it0)
    it0["dst_off"] = o0
    outs = []
    for ex in ("old", None, np.zeros(len(it0), BC.PRED_EXT_DTYPE)):
        pred = torch.full((total0,), SENTINEL, dtype=torch.int16, device=hp.device)
        if isinstance(ex, str):
            hp.pred_inter_batch(world.dev, it0, pred, 0, 10)
        else:
            hp.pred_inter_batch(world.dev, it0, pred, 0, 10, ext=ex)
        outs.append(pred.cpu().numpy())
    assert np.array_equal(outs[0], outs[1]) and np.array_equal(outs[0], outs[2]) and outs[0].min() >= 0


# ---- 7 ----
def test_ext_none_and_zero_equal_the_old_entry_on_the_existing_mixed_list(hp):
    """the mixed lists of tests/test_gpu_pred_inter.py (every luma and chroma size, uni and bi) through the new entry with ext = NULL and with all-zero extensions"""
    import torch
    import test_gpu_pred_inter as TI
    world = TI.World(hp, 10, 25)
    ua, _ = TI.build_list(world, False, 10)
    ba, _ = TI.build_list(world, True, 11)
    items = np.concatenate([ua, ba])
    off, total = BC.compact_offsets(items)
    items["dst_off"] = off
    outs = []
    for mode in range(3):
        pred = torch.full((total,), SENTINEL, dtype=torch.int16, device=hp.device)
        if mode == 0:
            hp.pred_inter_batch(world.dev, items, pred, 0, 10)
        elif mode == 1:
            import ctypes as C
            tab = (hp._MePlane * len(world.dev))(*[hp._MePlane(p.buf_ptr.value, p.stride, 0) for p in world.dev])
            assert hp.L.vvhip_pred_inter_batch_ex(hp.ctx, C.cast(tab, C.c_void_p), len(world.dev), items.ctypes.data_as(C.c_void_p), None, len(items), 10,
                                                  C.c_void_p(pred.data_ptr()), 0, None, 0, None) == 0
        else:
            hp.pred_inter_batch(world.dev, items, pred, 0, 10, ext=np.zeros(len(items), BC.PRED_EXT_DTYPE))
        outs.append(pred.cpu().numpy())
    assert np.array_equal(outs[0], outs[1]) and np.array_equal(outs[0], outs[2]) and outs[0].min() >= 0


# ---- 8 ----
def test_dmvr_search_results_chain_into_the_list(hp, reflib):
    """vvhip_dmvr_refine_batch -> dmvr_pred_items -> vvhip_pred_inter_batch_ex, against the model driven by the same results: refined sub-blocks through the padded
    reference, BDOF where min_cost allows it, luma and chroma"""
    from vvenc_amd.hotpath import DMVR_ITEM_DTYPE, DMVR_RESULT_DTYPE, dmvr_pred_items
    bd = 10
    rng = np.random.default_rng(81)
    yy, xx = np.mgrid[0:LHH, 0:LWW]
    tex = 512 + 220 * np.sin(xx / 6.0) * np.cos(yy / 5.0) + 80 * np.sin((xx - yy) / 3.0)
    r0 = np.clip(tex + rng.normal(0, 6, tex.shape), 0, 1023).astype(np.int16)
    r1 = np.clip(np.roll(tex, (2, -4), (0, 1)) + rng.normal(0, 6, tex.shape), 0, 1023).astype(np.int16)
    c0, c1 = np.ascontiguousarray(r0[::2, ::2]), np.ascontiguousarray(r1[::2, ::2])
    pl = [r0, r1, c0, c1]
    dev = [hp.plane(a, 0) for a in pl]
    moved = with_bdof = 0
    for (dx, dy) in ((16, 16), (16, 8), (8, 16)):
        n = 40
        pos = [(int(rng.integers(12, LWW - dx - 12)), int(rng.integers(12, LHH - 1 - dy - 12))) for _ in range(n)]
        start = [((int(rng.integers(-40, 41)), int(rng.integers(-40, 41))), (int(rng.integers(-40, 41)), int(rng.integers(-40, 41)))) for _ in range(n)]
        it = np.zeros(n, DMVR_ITEM_DTYPE)
        for k in range(n):
            (ax, ay), (bx, by) = start[k]
            it[k] = ((pos[k][1] + (ay >> 4)) * dev[0].stride + pos[k][0] + (ax >> 4), (pos[k][1] + (by >> 4)) * dev[1].stride + pos[k][0] + (bx >> 4), ax & 15, ay & 15, bx & 15, by & 15)
        res = hp.dmvr_refine_batch(dev[0], dev[1], hp.to_device(it), n, dx, dy, bd).cpu().numpy().reshape(-1).view(DMVR_RESULT_DTYPE)
        items, ext = dmvr_pred_items(res, start, pos, (0, 1), (dev[0].stride, dev[1].stride), dx, dy, bdof=True, chroma_planes=((2, 3),), chroma_strides=(dev[2].stride, dev[3].stride))
        world = type("W", (), dict(np=pl, dev=dev, bd=bd, org=None))
        its, pred, _ = run_compact(hp, world, items, ext)
        where = []
        for k in range(len(its)):
            stride = dev[int(its[k]["ref_plane"][0])].stride
            where.append([(int(its[k]["ref_off"][l]) % stride, int(its[k]["ref_off"][l]) // stride) for l in (0, 1)])
        check_blocks(blocks_of(pred, its), its, ext, where, world, reflib, "chain %dx%d" % (dx, dy))
        moved += int(np.count_nonzero(ext["flags"][:n] & BR.EXT_DMVR_PAD))
        with_bdof += int(np.count_nonzero(ext["flags"][:n] & BR.EXT_BDOF))
    assert moved >= 10 and with_bdof >= 10, (moved, with_bdof)


LWW, LHH = 192, 161


# ---- 9 ----
def test_ex_argument_errors(hp):
    """every argument error of the extension returns VVHIP_E_ARG with a message and leaves the output sentinel untouched"""
    import torch
    from vvenc_amd.lib import VVHipError
    world = world_of(hp, 10, 110)
    good = np.zeros(3, BC.PRED_ITEM_DTYPE)
    for k in range(3):
        good[k]["width"], good[k]["height"], good[k]["ref_plane"] = 16, 16, (0, 1)
        good[k]["ref_off"] = 20 * world.dev[0].stride + 20
        good[k]["dst_off"] = 256 * k
    gext = np.zeros(3, BC.PRED_EXT_DTYPE)
    gext["flags"] = BR.EXT_BDOF

    def case(item_changes=(), ext_changes=()):
        it, ex = good.copy(), gext.copy()
        for f, v in item_changes:
            it[f][2] = v
        for f, v in ext_changes:
            ex[f][2] = v
        return it, ex
    cases = [case([("chroma", 1), ("ref_plane", (2, 3))]),                                   # BDOF on chroma
             case([("ref_plane", (0, -1))]),                                                  # BDOF with one list
             case([("ref_plane", (-1, 1))]),
             case([("width", 8), ("height", 8)]),                                             # sizes that fail the rule
             case([("width", 4), ("height", 32)]),
             case([("width", 64), ("height", 4)]),
             case((), [("flags", BR.EXT_DMVR_PAD), ("pad_dx", (3, 0))]),                      # |pad| > 2 for luma
             case((), [("flags", BR.EXT_DMVR_PAD), ("pad_dy", (0, -3))]),
             case([("chroma", 1), ("ref_plane", (2, 3))], [("flags", BR.EXT_DMVR_PAD), ("pad_dx", (2, 0))]),          # > 1 for chroma
             case([("chroma", 1), ("ref_plane", (2, 3))], [("flags", BR.EXT_DMVR_PAD), ("pad_dy", (0, -2))]),
             case((), [("rsv", (0, 1, 0))]),                                                  # non-zero reserved bytes
             case((), [("flags", 4)])]                                                        # unknown flag bit
    for k, (it, ex) in enumerate(cases):
        pred = torch.full((768,), SENTINEL, dtype=torch.int16, device=hp.device)
        with pytest.raises(VVHipError) as e:
            hp.pred_inter_batch(world.dev, it, pred, 0, 10, ext=ex)
        assert "vvhip_pred_inter_batch_ex" in str(e.value) and "error -1" in str(e.value), (k, str(e.value))
        torch.cuda.synchronize()
        assert np.all(pred.cpu().numpy() == SENTINEL), k
    pred = torch.full((768,), SENTINEL, dtype=torch.int16, device=hp.device)          # the context is still usable
    hp.pred_inter_batch(world.dev, good, pred, 0, 10, ext=gext)
    assert pred.cpu().numpy().min() >= 0
