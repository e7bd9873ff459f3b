"""GPU tier of the inter-prediction list entry: vvhip_interp_chroma_batch and vvhip_pred_inter_batch against the compiled reference, tolerance 0.

Expected values: tests/pred_ref.py — every interpolation pass executed from the compiled reference (scalar row and x86 row, the `reflib` fixture), composed the way
InterPredInterpolation::xPredInterBlk composes them (CommonLib/InterPrediction.cpp:838-866).  The bi-prediction average (AreaBuf<Pel>::addAvg, CommonLib/Buffer.cpp:549-575,
core :129-141) and the residual subtraction are restated in numpy there (one line each): the only two steps not executed from the reference library."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import pred_ref as PR  # noqa: E402

LW, LH, LM = 160, 160, 4          # luma reference planes: visible size incl. margin LM on every side (+ one spare row: the 16-byte rule)
CW, CH, CM = 96, 96, 2            # chroma reference planes
SENTINEL = -7


@pytest.fixture(scope="module")
def hp():
    from vvenc_amd.hotpath import HotPath
    return HotPath()


def _picture(rng, h, w, bd, seed_shift=0):
    yy, xx = np.mgrid[0:h, 0:w]
    top = (1 << bd) - 1
    return np.clip(top / 2 + top / 4 * np.sin((xx + seed_shift) / 6.0) * np.cos((yy - seed_shift) / 5.0) + rng.normal(0, top / 25, (h, w)), 0, top).astype(np.int16)


class World:
    """reference planes (numpy + device) of one bit depth: 0, 1 luma; 2, 3 chroma; 4 all zero; 5 all max; plus an original plane"""

    def __init__(self, hp, bd, seed):
        rng = np.random.default_rng(seed)
        top = (1 << bd) - 1
        self.bd = bd
        self.np = [_picture(rng, LH + 1, LW, bd, 0), _picture(rng, LH + 1, LW, bd, 3), _picture(rng, CH + 1, CW, bd, 1), _picture(rng, CH + 1, CW, bd, 7),
                   np.zeros((LH + 1, LW), np.int16), np.full((LH + 1, LW), top, np.int16)]
        self.dev = [hp.plane(a, 0) for a in self.np]
        for a, p in zip(self.np, self.dev):
            assert p.stride == a.shape[1]
        self.org_np = np.clip(self.np[0].astype(np.int32) + rng.integers(-12, 13, self.np[0].shape), 0, top).astype(np.int16)
        self.org = hp.plane(self.org_np, 0)

    def limits(self, plane, w, h, chroma):
        """inclusive range of integer block positions that keep the taps inside the plane's margin"""
        H, W = self.np[plane].shape
        m = CM if chroma else LM
        return m, W - w - m, m, H - 1 - h - m


def _place(rng, world, plane, w, h, chroma, k):
    x0, x1, y0, y1 = world.limits(plane, w, h, chroma)
    if k % 4 == 0:          # every fourth block touches the margin: one of the four corners of the allowed range
        c = (k // 4) % 4
        return (x0 if c & 1 == 0 else x1), (y0 if c & 2 == 0 else y1)
    return int(rng.integers(x0, x1 + 1)), int(rng.integers(y0, y1 + 1))


def build_list(world, bi, seed):
    """one list mixing all luma sizes 4..128 x 4..128 and all chroma sizes 2..64 x 2..64: all 16 x 16 luma phases, the alternative half-sample filter, 4x4 luma;
    bi: the second list from another plane — or the same —, items with every fraction zero, and the all-zero / all-max planes.  -> (items, pos) with pos[i][l] = (x, y)"""
    from vvenc_amd.hotpath import PRED_ITEM_DTYPE
    rng = np.random.default_rng(seed)
    recs, pos = [], []
    phase = 0

    def add(w, h, chroma, alt, fr, planes):
        it = np.zeros((), PRED_ITEM_DTYPE)
        it["width"], it["height"], it["chroma"], it["alt_hpel"] = w, h, chroma, alt
        p = [None, None]
        for l in (0, 1):
            it["ref_plane"][l] = planes[l]
            if planes[l] < 0:
                continue
            x, y = _place(rng, world, planes[l], w, h, chroma, len(recs) + l)
            p[l] = (x, y)
            it["ref_off"][l] = y * world.dev[planes[l]].stride + x
            it["frac"][l] = fr[l]
        recs.append(it)
        pos.append(p)

    def lists(k, a, b):
        if bi:
            return (a, a) if k % 5 == 4 else (a, b)          # every fifth item: both lists point at the same plane
        return (a, -1) if k % 2 == 0 else (-1, a)

    for (w, h) in PR.LUMA_SIZES:
        for k in range(8):
            f0 = (phase % 16, phase // 16 % 16)
            phase += 1
            a = int(rng.integers(0, 2))
            add(w, h, 0, 0, (f0, (int(rng.integers(0, 16)), int(rng.integers(0, 16)))) if k % 2 == 0 or bi else ((0, 0), f0), lists(k, a, 1 - a))
        for k in range(4):          # IMV_HPEL: half-sample vectors through m_lumaAltHpelIFilter
            f0 = (8 * (k & 1), 8 * (k >> 1))
            add(w, h, 0, 1, (f0, (8 * ((k + 1) & 1), 8 * ((k + 2) >> 1 & 1))) if k % 2 == 0 or bi else ((0, 0), f0), lists(k, k & 1, 1 - (k & 1)))
    assert phase >= 256
    for (w, h) in PR.CHROMA_SIZES:
        for k in range(8):
            f0 = (int(rng.integers(0, 32)), int(rng.integers(0, 32)))
            a = 2 + int(rng.integers(0, 2))
            add(w, h, 1, 0, (f0, (int(rng.integers(0, 32)), int(rng.integers(0, 32)))) if k % 2 == 0 or bi else ((0, 0), f0), lists(k, a, 5 - a))
    if bi:
        for (w, h, chroma) in ((4, 4, 0), (16, 8, 0), (64, 64, 0), (128, 32, 0), (2, 2, 1), (4, 4, 1), (8, 32, 1), (64, 16, 1)):
            ra, rb = (2, 3) if chroma else (0, 1)
            add(w, h, chroma, 0, ((0, 0), (0, 0)), (ra, rb))              # copy path with the 14-bit shift on both lists
            add(w, h, chroma, 0, ((0, 0), (5, 0)), (ra, ra))
            for planes in ((4, 4), (5, 5), (4, 5), (5, ra)):               # saturated operands: the clip of the average
                add(w, h, chroma, 0, ((int(rng.integers(0, 16)), int(rng.integers(0, 16))), (int(rng.integers(0, 16)), int(rng.integers(0, 16)))), planes)
    else:
        for l, fr in enumerate((((3, 0), (0, 0)), ((0, 0), (0, 11)))):      # uni-prediction from the saturated planes
            add(32, 32, 0, 0, fr, (5, -1) if l == 0 else (-1, 5))
    items = np.concatenate([r.reshape(1) for r in recs])
    return items, pos


def compact_offsets(items):
    sizes = items["width"].astype(np.int64) * items["height"]
    off = np.concatenate([[0], np.cumsum(sizes)[:-1]])
    return off.astype(np.int32), int(sizes.sum())


def run_compact(hp, world, items, org=False):
    import torch
    items = items.copy()
    off, total = compact_offsets(items)
    items["dst_off"] = off
    pred = torch.full((total,), SENTINEL, dtype=torch.int16, device=hp.device)
    resi = torch.full((total,), SENTINEL, dtype=torch.int16, device=hp.device) if org else None
    hp.pred_inter_batch(world.dev, items, pred, 0, world.bd, world.org if org else None, resi)
    torch.cuda.synchronize()
    return (items, pred.cpu().numpy(), resi) if org else (items, pred.cpu().numpy(), None)


def blocks_of(buf, items):
    return [buf[int(it["dst_off"]):int(it["dst_off"]) + int(it["width"]) * int(it["height"])].reshape(int(it["height"]), int(it["width"])) for it in items]


def check_blocks(got, items, pos, world, lib, what):
    for i, (g, it) in enumerate(zip(got, items)):
        e = PR.expected_block(lib, world.np, pos[i], it, world.bd)
        assert np.array_equal(g, e), (what, lib.name, i, it, pos[i], np.argwhere(g != e)[:3].tolist())


# ---- 3 ----
def test_interp_chroma_batch_every_size_and_phase(hp, reflib):
    """vvhip_interp_chroma_batch: every chroma size 2..64 x 2..64, all 32 x 32 phases once per size — dealt over four launches per size: rnd_res 0 / 1 x 8 / 10 bits —,
    every fourth block touching the plane margin"""
    from vvenc_amd.hotpath import SUBPEL_DTYPE
    worlds = {8: World(hp, 8, 11), 10: World(hp, 10, 12)}
    rng = np.random.default_rng(31)
    for (w, h) in PR.CHROMA_SIZES:
        for combo in range(4):
            rnd, bd = combo & 1, (8, 10)[combo >> 1]
            world = worlds[bd]
            ph = [(xf, yf) for yf in range(32) for xf in range(32) if (xf + 2 * yf + (xf >> 2)) % 4 == combo]
            it = np.zeros(len(ph), SUBPEL_DTYPE)
            where = []
            for k, (xf, yf) in enumerate(ph):
                x, y = _place(rng, world, 2, w, h, True, k)
                where.append((x, y))
                it[k] = (0, y * world.dev[2].stride + x, xf, yf)
            got = hp.interp_chroma_batch(world.dev[2], hp.to_device(it), len(ph), w, h, bd, bool(rnd)).cpu().numpy().reshape(len(ph), h, w)
            for k, ((xf, yf), (x, y)) in enumerate(zip(ph, where)):
                e = PR.chroma_pred(reflib, world.np[2], y, x, w, h, xf, yf, rnd, bd)
                assert np.array_equal(got[k], e), (reflib.name, w, h, xf, yf, rnd, bd, x, y)
    assert sum(len([1 for yf in range(32) for xf in range(32) if (xf + 2 * yf + (xf >> 2)) % 4 == c]) for c in range(4)) == 1024


# ---- 4 ----
def test_pred_list_uni(hp, reflib):
    """one list, every luma and chroma size, one reference list per item; compact output and output into a plane (samples outside the blocks stay untouched)"""
    import torch
    world = World(hp, 10, 21)
    items, pos = build_list(world, False, 5)
    its, pred, _ = run_compact(hp, world, items)
    check_blocks(blocks_of(pred, its), its, pos, world, reflib, "uni compact")
    # into a plane
    pw = 1024
    where, rows = PR.shelf_pack([(int(i["width"]), int(i["height"])) for i in items], pw)
    itp = items.copy()
    itp["dst_off"] = [y * pw + x for (x, y) in where]
    plane = torch.full((rows * pw,), SENTINEL, dtype=torch.int16, device=hp.device)
    hp.pred_inter_batch(world.dev, itp, plane, pw, world.bd)
    out = plane.cpu().numpy().reshape(rows, pw)
    mask = np.zeros((rows, pw), bool)
    comp = blocks_of(pred, its)
    for i, (it, (x, y)) in enumerate(zip(itp, where)):
        w, h = int(it["width"]), int(it["height"])
        assert np.array_equal(out[y:y + h, x:x + w], comp[i]), ("plane output", i, it)
        mask[y:y + h, x:x + w] = True
    assert np.all(out[~mask] == SENTINEL)


# ---- 5 ----
def test_pred_list_bi(hp, reflib):
    """the same sizes bi-predicted from two planes: same-plane pairs, all-zero fractions, saturated references"""
    for bd, seed in ((10, 22), (8, 23)):
        world = World(hp, bd, seed)
        items, pos = build_list(world, True, 6 + bd)
        if bd == 8:
            items, pos = items[::3], pos[::3]
        its, pred, _ = run_compact(hp, world, items)
        check_blocks(blocks_of(pred, its), its, pos, world, reflib, "bi %d bit" % bd)


# ---- 6 ----
def test_residual_output_feeds_the_tu_pipeline(hp, oracle):
    """d_resi == org - pred per item (pred: the x86 row of the reference, or the C restatement where the compiled reference is absent), and the compact residual buffer IS a d_resi of
    vvhip_tu_rdo_multi_strided: statistics, levels and reconstruction equal the oracle's tu_rdo on the host-made residual"""
    import torch
    from oracle.oracle import RefLib
    from vvenc_amd.hotpath import STATS_DTYPE, HotPath
    lib = RefLib(1) if RefLib.available() else oracle
    world = World(hp, 10, 24)
    ua, up = build_list(world, False, 8)
    ba, bp = build_list(world, True, 9)
    items = np.concatenate([ua[::2], ba[1::2]])
    pos = up[::2] + bp[1::2]
    rng = np.random.default_rng(61)
    H, W = world.org_np.shape
    for i, it in enumerate(items):
        w, h = int(it["width"]), int(it["height"])
        l = 0 if int(it["ref_plane"][0]) >= 0 else 1
        x, y = pos[i][l] if not int(it["chroma"]) and int(it["ref_plane"][l]) < 2 else (int(rng.integers(0, W - w + 1)), int(rng.integers(0, H - h + 1)))
        items["org_off"][i] = y * world.org.stride + x
    its, pred, d_resi = run_compact(hp, world, items, org=True)
    resi = d_resi.cpu().numpy()
    host_resi = []
    for i, (p, r, it) in enumerate(zip(blocks_of(pred, its), blocks_of(resi, its), its)):
        w, h = int(it["width"]), int(it["height"])
        e = PR.expected_block(lib, world.np, pos[i], it, world.bd)
        assert np.array_equal(p, e), ("pred", i, it)
        oy, ox = divmod(int(it["org_off"]), world.org.stride)
        host_resi.append(PR.residual(world.org_np[oy:oy + h, ox:ox + w], e))
        assert np.array_equal(r, host_resi[-1]), ("resi", i, it)
    # leg B on the device-made residual
    jobs, strides, keep = [], [], []
    for S in (4, 8, 16, 32, 64):
        idx = [i for i, it in enumerate(its) if int(it["width"]) == S and int(it["height"]) == S and not int(it["chroma"])]
        n = len(idx)
        assert n >= 4
        qps = rng.integers(22, 48, n)
        off = hp.to_device(its["dst_off"][idx].astype(np.int32))
        qp = hp.to_device(HotPath.tu_qp(qps, 1, 1))
        lev = torch.full((n * S * S,), 0x7777, dtype=torch.int16, device=hp.device)
        rec = torch.full((n * S * S,), 0x5555, dtype=torch.int16, device=hp.device)
        st = torch.full((n, STATS_DTYPE.itemsize), 0xEE, dtype=torch.uint8, device=hp.device)
        jobs.append((S, S, 0, 0, n, 8, off, qp, lev, rec, st))
        strides.append(S)
        keep.append((S, idx, qps))
    hp.tu_rdo_multi_strided(d_resi, strides, jobs, 10)
    torch.cuda.synchronize()
    for (S, idx, qps), job in zip(keep, jobs):
        n = len(idx)
        lv, rc = job[8].cpu().numpy().reshape(n, S, S), job[9].cpu().numpy().reshape(n, S, S)
        sv = job[10].cpu().numpy().view(STATS_DTYPE).reshape(n)
        for k, i in enumerate(idx):
            el, er, es = oracle.tu_rdo(host_resi[i], int(qps[k]), 1, 0, 0, 10, 8, 1)
            assert np.array_equal(lv[k], el), ("lev", S, k)
            assert np.array_equal(rc[k], er), ("rec", S, k)
            got = (int(sv["abs_sum"][k]), int(sv["last_scan_pos"][k]), int(sv["need_rdoq"][k]), int(sv["sse"][k]))
            assert got == (es["abs_sum"], es["last_scan_pos"], es["need_rdoq"], es["sse"]), (S, k, got, es)


# ---- 7 ----
def test_list_order_does_not_leak_into_results(hp):
    """the host-side size-class sort and the XCD deal are invisible: the same items in three other orders write the same buffer"""
    import torch
    world = World(hp, 10, 25)
    ua, _ = build_list(world, False, 10)
    ba, _ = build_list(world, True, 11)
    items = np.concatenate([ua, ba])
    off, total = compact_offsets(items)
    items["dst_off"] = off
    outs = []
    rng = np.random.default_rng(3)
    for order in (np.arange(len(items)), rng.permutation(len(items)), np.arange(len(items))[::-1], rng.permutation(len(items))):
        pred = torch.full((total,), SENTINEL, dtype=torch.int16, device=hp.device)
        hp.pred_inter_batch(world.dev, items[order], pred, 0, world.bd)
        outs.append(pred.cpu().numpy())
    for o in outs[1:]:
        assert np.array_equal(o, outs[0])
    assert outs[0].min() >= 0


# ---- 8 ----
def test_luma_uni_items_equal_interp_luma_batch(hp):
    """old and new path agree: the luma uni-prediction items through vvhip_pred_inter_batch == vvhip_interp_luma_batch on the same items (filter_mode 0)"""
    from vvenc_amd.hotpath import SUBPEL_DTYPE
    world = World(hp, 10, 26)
    items, _ = build_list(world, False, 12)
    items = items[items["chroma"] == 0]
    its, pred, _ = run_compact(hp, world, items)
    new = blocks_of(pred, its)
    groups = {}
    for i, it in enumerate(its):
        l = 0 if int(it["ref_plane"][0]) >= 0 else 1
        groups.setdefault((int(it["width"]), int(it["height"]), int(it["ref_plane"][l]), int(it["alt_hpel"])), []).append((i, l))
    assert len(groups) >= 36
    for (w, h, plane, alt), members in groups.items():
        sp = np.zeros(len(members), SUBPEL_DTYPE)
        for k, (i, l) in enumerate(members):
            sp[k] = (0, int(its["ref_off"][i][l]), int(its["frac"][i][l][0]), int(its["frac"][i][l][1]))
        old = hp.interp_luma_batch(world.dev[plane], hp.to_device(sp), len(members), w, h, 10, True, 0, bool(alt)).cpu().numpy().reshape(len(members), h, w)
        for k, (i, _) in enumerate(members):
            assert np.array_equal(old[k], new[i]), (w, h, plane, alt, its[i])


# ---- 9 ----
def test_pred_argument_errors(hp):
    """unsupported input fails with VVHIP_E_ARG and a message; nothing is launched (the output keeps its fill)"""
    import torch
    from vvenc_amd.hotpath import PRED_ITEM_DTYPE, SUBPEL_DTYPE
    from vvenc_amd.lib import VVHipError
    world = World(hp, 10, 27)
    good = np.zeros(3, PRED_ITEM_DTYPE)
    for k in range(3):
        good[k]["width"], good[k]["height"] = 8, 8
        good[k]["ref_plane"] = (0, -1)
        good[k]["ref_off"][0] = 20 * world.dev[0].stride + 20
        good[k]["dst_off"] = 64 * k

    def broken(field, value):
        b = good.copy()
        b[field][2] = value
        return b
    cases = [broken("width", 12),                    # not a power of two
             broken("height", 256),                  # out of range
             broken("ref_plane", (9, -1)),           # plane index outside the table
             broken("ref_plane", (-1, -1)),          # both lists unused
             broken("frac", ((16, 0), (0, 0)))]      # luma fraction outside 1/16
    for k, items in enumerate(cases):
        pred = torch.full((192,), SENTINEL, dtype=torch.int16, device=hp.device)
        with pytest.raises(VVHipError) as e:
            hp.pred_inter_batch(world.dev, items, pred, 0, 10)
        assert "vvhip_pred_inter_batch" in str(e.value) and "error -1" in str(e.value), (k, str(e.value))
        torch.cuda.synchronize()
        assert np.all(pred.cpu().numpy() == SENTINEL), k
    with pytest.raises(VVHipError) as e:
        hp.interp_chroma_batch(world.dev[2], hp.to_device(np.zeros(1, SUBPEL_DTYPE)), 1, 6, 8)
    assert "vvhip_interp_chroma_batch" in str(e.value)
    # the context is still usable
    pred = torch.full((192,), SENTINEL, dtype=torch.int16, device=hp.device)
    hp.pred_inter_batch(world.dev, good, pred, 0, 10)
    assert pred.cpu().numpy().min() >= 0
