"""-m gpu: vvhip_dmvr_refine_batch, vvhip_sad_x5_batch and vvhip_sad_surface against the oracle (tolerance 0) on the extreme inputs of tests/dmvr_extremes.py.  The oracle
itself is pinned to the compiled reference on the same cases by tests/test_oracle_dmvr_extremes.py, which also holds the guards (the largest cost of a size and 25 costs
beyond 2^16, the early exit on both sides of equality, every quotient and both +-8 branches and the zero denominator of the error surface, each of the 25 positions
winning, all 256 fractions and 16 pairs of code paths, sentinels in the kernel's footprint, every team width of the X5 launch, the four KDY instantiations, both LDS
classes, a surface value of 2^30) and the sensitivity test.

What is compared:
  vvhip_dmvr_refine_batch   16x16, 8x8, 16x8, 8x16 x 8, 9 and 10 bits x the families saturated (864 sub-blocks), threshold (3, 10 bits), surface (52 to 55), phases (544),
                            layout (65: row pitches 320 and 200, sentinels around the reference's footprint), tie_pairs (5): one launch per family and size; the lists
                            of n = 0 .. 259, shuffled and identical items; the argument errors.  Every launch writes into a buffer pre-filled with a byte pattern that
                            carries eight guard records past n; the results' pad field is 0
  vvhip_sad_x5_batch        widths 8, 16 x heights 4 .. 128 x sub_shift 0, 1 x calc_centre 0, 1 x n = 1 .. 205 (240 launches, 13 000 items) on two-level planes of 8 to 15
                            bits; with calc_centre 0 entry 2 keeps the pattern; n = 0
  vvhip_sad_surface         2x2 .. 128x128 x ranges (0, 0), (0, 5), (7, 0), (16, 3) x sub_shift 0, 1 and the KDY 2 / 4 / 8 geometries on uniform, two-level and full-range
                            planes: each block alone (n_blocks = 1: gridDim.y = the displacement-row groups), the three together and in a list of 1025 (no split);
                            the window beyond 160 KiB of LDS is refused with the output untouched
Every expected value comes from the oracle.

Measured on an MI355X, per test: the DMVR families 0.07 to 0.08 s per bit depth (0.74 s for the first, which loads the kernels), the lists 0.01 to 0.02 s, the argument
errors 0.11 s, SAD-X5 0.17 s, the SAD surface 0.10 s per kind of planes, the refusal below 0.005 s; the file 4.1 s with 1.8 s of set-up (the device context).
"""
import ctypes as C

import numpy as np
import pytest

import dmvr_extremes as D

pytestmark = pytest.mark.gpu

FILL = 0xA5
GUARD = 8


@pytest.fixture(scope="module")
def hip():
    from hip_backend import HipBackend
    return HipBackend()


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _dmvr(hp, p0, p1, rec, dx, dy, bd):
    """one launch into a pre-filled buffer with GUARD records past n -> DMVR_RESULT records; asserts the guard records and the pad field"""
    import torch
    n = rec.size
    out = torch.full((n + GUARD, D.DMVR_RESULT.itemsize), FILL, dtype=torch.uint8, device=hp.device)
    d_items = hp.to_device(rec if n else np.zeros(1, D.DMVR_ITEM))
    rc = hp.L.vvhip_dmvr_refine_batch(hp.ctx, p0.buf_ptr, p0.stride, p1.buf_ptr, p1.stride, _ptr(d_items), n, dx, dy, bd, _ptr(out))
    assert rc == 0, (rc, hp.L.vvhip_last_error(hp.ctx))
    raw = out.cpu().numpy()
    assert (raw[n:] == FILL).all(), ("records past n were written", n, dx, dy, bd)
    res = raw[:n].reshape(-1).view(D.DMVR_RESULT)
    assert (res["pad"] == 0).all()
    return [(int(r["mvd_x"]), int(r["mvd_y"]), int(r["min_cost"])) for r in res]


def _planes(hp, fam):
    p0, p1 = hp.plane(fam.ref0, 0), hp.plane(fam.ref1, 0)
    assert (p0.stride, p1.stride) == (fam.ref0.shape[1], fam.ref1.shape[1])          # the kernel's footprint was checked against these shapes (Family.__init__)
    return p0, p1


@pytest.mark.parametrize("bd", D.BITDEPTHS)
def test_dmvr_families(hip, oracle, bd):
    """every family but the lists, one launch per family and size"""
    from vvenc_amd.hotpath import DMVR_ITEM_DTYPE, DMVR_RESULT_DTYPE
    assert D.DMVR_ITEM == DMVR_ITEM_DTYPE and D.DMVR_RESULT == DMVR_RESULT_DTYPE
    hp = hip.hp
    n = 0
    for dx, dy in D.SIZES:
        for fam in D.families(bd, dx, dy):
            if fam.name == "lists":
                continue
            p0, p1 = _planes(hp, fam)
            got = _dmvr(hp, p0, p1, fam.records(p0.stride, p1.stride), dx, dy, bd)
            exp = [tuple(e) for e in fam.expected(oracle)]
            bad = [(k, got[k], exp[k]) for k in range(len(exp)) if got[k] != exp[k]]
            assert not bad, (fam.name, bd, dx, dy, len(bad), bad[:4], None if fam.tags is None else fam.tags[bad[0][0]])
            n += len(exp)
    assert n > 5800


@pytest.mark.parametrize("bd", D.BITDEPTHS)
def test_dmvr_lists(hip, oracle, bd):
    """n = 0 .. 259: partial last workgroups, grids below, at and past a multiple of the eight-way remap; the whole list shuffled; 67 identical items.  n = 0 is no error
    and writes nothing"""
    hp = hip.hp
    for dx, dy in D.SIZES:
        fam = D.lists(bd, dx, dy)
        p0, p1 = _planes(hp, fam)
        exp = [tuple(e) for e in fam.expected(oracle)]
        assert sum(e[0] != 0 or e[1] != 0 for e in exp) > 60
        for name, sel in D.list_selections():
            got = _dmvr(hp, p0, p1, fam.records(p0.stride, p1.stride, sel), dx, dy, bd)
            assert got == [exp[k] for k in sel], (name, bd, dx, dy, [(i, got[i], exp[k]) for i, k in enumerate(sel) if got[i] != exp[k]][:4])


def test_dmvr_argument_errors(hip):
    """sub-blocks of 4 or 32 per side, bit depths 7 and 11, a negative n, null pointers with n > 0: VVHIP_E_ARG, nothing written, and the context stays usable"""
    import torch
    hp = hip.hp
    fam = D.threshold(8, 8)
    p0, p1 = _planes(hp, fam)
    rec = fam.records(p0.stride, p1.stride)
    d_items = hp.to_device(rec)
    out = torch.full((rec.size + GUARD, 16), FILL, dtype=torch.uint8, device=hp.device)
    a = dict(r0=p0.buf_ptr, s0=p0.stride, r1=p1.buf_ptr, s1=p1.stride, it=_ptr(d_items), n=rec.size, dx=8, dy=8, bd=10, out=_ptr(out))
    bad = [dict(dx=4), dict(dx=32), dict(dy=4), dict(dy=32), dict(dx=12), dict(bd=7), dict(bd=11), dict(n=-1), dict(r0=None), dict(r1=None), dict(it=None), dict(out=None)]
    for ch in bad:
        b = dict(a, **ch)
        rc = hp.L.vvhip_dmvr_refine_batch(hp.ctx, b["r0"], b["s0"], b["r1"], b["s1"], b["it"], b["n"], b["dx"], b["dy"], b["bd"], b["out"])
        assert rc == -1, (ch, rc)
        assert hp.L.vvhip_last_error(hp.ctx)
    assert hp.L.vvhip_dmvr_refine_batch(hp.ctx, None, 0, None, 0, None, 0, 8, 8, 10, None) == 0          # n = 0 needs no pointers
    torch.cuda.synchronize()
    assert bool((out == FILL).all())
    assert _dmvr(hp, p0, p1, rec, 8, 8, 10) == [(0, 0, 63), (-32, -32, 0), (-32, -32, 0)]


def test_sad_x5(hip, oracle):
    """every X5 case: 5 n teams of 2 .. 64 lanes, partial last workgroups, odd cur offsets, the first and the last sample of the planes; with calc_centre 0 entry 2 keeps
    what it held; five guard entries past 5 n; n = 0"""
    import torch
    hp = hip.hp
    org, cur = D.x5_planes()
    po, pc = hp.plane(org, 0), hp.plane(cur, 0)
    assert (po.stride, pc.stride) == (D.X5_W, D.X5_W)
    pat = int(np.array([FILL] * 8, np.uint8).view(np.int64)[0])
    total = 0
    for w, h, ss, cc, n, items in D.x5_cases():
        assert all(0 <= ox and ox + 4 + w <= D.X5_W and 0 <= cx - 4 and cx + w <= D.X5_W and 0 <= oy and oy + h <= org.shape[0] and 0 <= cy and cy + h <= cur.shape[0] for (ox, oy, cx, cy, _) in items)
        d_it = hp.to_device(np.array([(oy * po.stride + ox, cy * pc.stride + cx) for (ox, oy, cx, cy, _) in items], np.int32))
        out = torch.full((5 * n + 5,), pat, dtype=torch.int64, device=hp.device)
        rc = hp.L.vvhip_sad_x5_batch(hp.ctx, po.buf_ptr, po.stride, pc.buf_ptr, pc.stride, w, h, ss, cc, _ptr(d_it), n, _ptr(out))
        assert rc == 0, (rc, w, h, ss, cc, n)
        got = out.cpu().numpy()
        assert (got[5 * n:] == pat).all(), (w, h, ss, cc, n)
        exp = np.array([oracle.sad_x5((org, oy, ox), (cur, cy, cx), w, h, ss, True).tolist() for (ox, oy, cx, cy, _) in items], np.int64)
        if not cc:
            exp[:, 2] = pat
        assert np.array_equal(got[:5 * n].reshape(n, 5), exp), (w, h, ss, cc, n, np.argwhere(got[:5 * n].reshape(n, 5) != exp)[:4].tolist())
        total += n
    assert total == 13000
    out = torch.full((5,), pat, dtype=torch.int64, device=hp.device)
    assert hp.L.vvhip_sad_x5_batch(hp.ctx, po.buf_ptr, po.stride, pc.buf_ptr, pc.stride, 8, 8, 1, 1, None, 0, _ptr(out)) == 0
    assert bool((out == pat).all())


def _surface(hp, po, pr, blocks, w, h, ss, rx, ry):
    """one launch over `blocks` = [(x, y)] into a pre-filled buffer with a guard of eight displacement rows and 64 entries -> (n, 2 ry + 1, 2 rx + 1) int64"""
    import torch
    nx, ny, n = 2 * rx + 1, 2 * ry + 1, len(blocks)
    off = hp.to_device(np.array([y * po.stride + x for x, y in blocks], np.int32))
    guard = 8 * nx + 64
    out = torch.full((n * nx * ny + guard,), 0x7b7b7b7b, dtype=torch.int32, device=hp.device)
    rc = hp.L.vvhip_sad_surface(hp.ctx, po.buf_ptr, po.stride, pr.buf_ptr, pr.stride, w, h, ss, rx, ry, _ptr(off), _ptr(off), n, _ptr(out))
    assert rc == 0, (rc, hp.L.vvhip_last_error(hp.ctx), w, h, ss, rx, ry, n)
    got = out.cpu().numpy()
    assert (got[n * nx * ny:] == 0x7b7b7b7b).all(), ("entries past the last block were written", w, h, ss, rx, ry, n)
    return got[:n * nx * ny].view(np.uint32).astype(np.int64).reshape(n, ny, nx)


@pytest.mark.parametrize("kind", D.SURF_PLANES)
def test_sad_surface(hip, oracle, kind):
    """every geometry on one kind of planes: each block alone (the maximal split over gridDim.y), the three in one launch, and in a list of 1025 (one workgroup per block,
    no split) — all equal to the oracle, so equal to each other"""
    hp = hip.hp
    org, ref = D.surf_planes(kind)
    po, pr = hp.plane(org, 0), hp.plane(ref, 0)
    assert po.stride == pr.stride == D.SURF_W
    top = 0
    for (w, h, ss, rx, ry) in D.surf_geometries():
        blocks = D.surf_blocks(w, h, rx, ry)
        assert all(rx <= x <= D.SURF_W - w - rx and ry <= y <= D.SURF_H - h - ry for x, y in blocks)
        exp = D.surf_expected(oracle, kind, w, h, ss, rx, ry)
        top = max(top, int(exp.max()))
        for b in range(3):
            got = _surface(hp, po, pr, blocks[b:b + 1], w, h, ss, rx, ry)
            assert np.array_equal(got[0], exp[b]), (kind, w, h, ss, rx, ry, "alone", b, np.argwhere(got[0] != exp[b])[:4].tolist())
        got = _surface(hp, po, pr, blocks, w, h, ss, rx, ry)
        assert np.array_equal(got, exp), (kind, w, h, ss, rx, ry, "three blocks", np.argwhere(got != exp)[:4].tolist())
        got = _surface(hp, po, pr, [blocks[i % 3] for i in range(1025)], w, h, ss, rx, ry)
        assert np.array_equal(got, exp[np.arange(1025) % 3]), (kind, w, h, ss, rx, ry, "1025 blocks", np.argwhere(got != exp[np.arange(1025) % 3])[:4].tolist())
    assert kind != "full_range" or top >= 1 << 29


def test_sad_surface_refuses_a_window_beyond_160_kib(hip, oracle):
    """VVHIP_E_UNSUPPORTED with the output untouched, split or not; the context stays usable"""
    import torch
    hp = hip.hp
    org, ref = D.surf_planes("uniform10")
    po, pr = hp.plane(org, 0), hp.plane(ref, 0)
    w, h, ss, rx, ry = D.SURF_TOO_BIG
    blocks = D.surf_blocks(w, h, rx, ry)
    for n in (1, 3, 1025):
        off = hp.to_device(np.array([blocks[i % 3][1] * po.stride + blocks[i % 3][0] for i in range(n)], np.int32))
        out = torch.full((4096,), 0x7b7b7b7b, dtype=torch.int32, device=hp.device)
        rc = hp.L.vvhip_sad_surface(hp.ctx, po.buf_ptr, po.stride, pr.buf_ptr, pr.stride, w, h, ss, rx, ry, _ptr(off), _ptr(off), n, _ptr(out))
        assert rc == -4 and b"LDS" in hp.L.vvhip_last_error(hp.ctx), (n, rc)
        torch.cuda.synchronize()
        assert bool((out == 0x7b7b7b7b).all())
    got = _surface(hp, po, pr, D.surf_blocks(8, 16, 7, 0), 8, 16, 0, 7, 0)
    assert np.array_equal(got, D.surf_expected(oracle, "uniform10", 8, 16, 0, 7, 0))
