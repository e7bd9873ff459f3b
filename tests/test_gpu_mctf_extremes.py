"""-m gpu: the MCTF device code against the oracle (tolerance 0) on the extreme inputs of tests/mctf_extremes.py — vvhip_mctf_error_batch, vvhip_mctf_calc_var_batch,
vvhip_mctf_subsample, vvhip_extend_border, the search through both routes (vvhip_mctf_motion_estimation and level by level through vvhip_mctf_me_level) and
vvhip_mctf_apply_plane.  The oracle itself is pinned to the compiled reference on the same cases by tests/test_oracle_mctf_extremes.py, which also holds the guards (the
largest error sum of every size, 2^31 - 1 where a size allows more; ties at every level; the schedule's reach in four directions; all 256 phases; both sides of every
threshold; clipping at both ends; the reference's undefined corners kept out) and the sensitivity test.

What is compared:
  vvhip_mctf_error_batch     8 .. 64 x 8 .. 64 x both tap sets x 8 and 10 bits: every page pair at integer displacement and the 255 phases, one launch per size (279 items);
                             the saturated pair of every size; lists of n = 0, 1, 63, 64, 65, 300; the argument errors.  Every launch writes into a buffer pre-filled
                             with a pattern that carries eight guard entries past n
  vvhip_mctf_calc_var_batch  72 sizes from 1x1 to 128x128 x flat, half 0 / half max, checker, near-end and texture blocks
  vvhip_mctf_subsample / vvhip_extend_border
                             13 planes from 1x1 to 301x5 x pads 0, 1, 16, 128, the destination inside sentinel-filled storage at an odd pitch: the plane and its border
                             equal the oracle's, no sample outside them changes, the source stays as it was
  the search                 per configuration (unit x speed x add_level) 16 pictures of 64x64 .. 208x136: x, y, error at every level through the per-level route, the five
                             fields of the last level through both routes; four pictures of family c and two of family d through the row hand-off (a child process with
                             VVHIP_MCTF_DIAG=0)
  vvhip_mctf_apply_plane     26 pictures of 4:2:0 up to 96x64: every plane the entry accepts (the 32x32 luma blocks of unit 32 are refused: asserted), the output inside
                             sentinel-filled storage; 13 references are refused
Every expected value comes from the oracle.

Measured on an MI355X, per test: the error families 0.6 to 0.9 s per bit depth and tap set (64 launches of 279 items and their 17 800 oracle values), the saturated pairs
0.06 s, the lists and the argument errors 0.1 s, the variance and the planes 0.01 s, the search 0.05 to 0.3 s per configuration, the row hand-off 2.3 s (a child process
with its own device context), the apply side 0.01 to 0.05 s per quarter; the file 9.5 s with 2.1 s of set-up (the device context).
"""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import mctf_extremes as M

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FILL = 0x5A
GUARD = 8


@pytest.fixture(scope="module")
def hip():
    from hip_backend import HipBackend
    return HipBackend()


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _errors(hp, po, pb, rec, w, h, tap4, bd):
    """one launch into a pre-filled buffer with GUARD entries past n -> the n errors; asserts the guard entries"""
    import torch
    n = rec.size
    pat = int(np.array([FILL] * 4, np.uint8).view(np.int32)[0])
    out = torch.full((n + GUARD,), pat, dtype=torch.int32, device=hp.device)
    d_items = hp.to_device(rec if n else np.zeros(1, M.ERR_ITEM))
    rc = hp.L.vvhip_mctf_error_batch(hp.ctx, po.buf_ptr, po.stride, pb.buf_ptr, pb.stride, w, h, int(tap4), bd, _ptr(d_items), n, _ptr(out))
    assert rc == 0, (rc, hp.L.vvhip_last_error(hp.ctx))
    got = out.cpu().numpy()
    assert (got[n:] == pat).all(), ("entries past n were written", n, w, h)
    return got[:n].tolist()


def _oracle_errors(oracle, org, buf, items, w, h, tap4, bd):
    return [oracle.mctf_err_frac(tap4, (org, oy, ox), (buf, by, bx), w, h, fx, fy, bd) if (fx | fy) else oracle.mctf_err_int((org, oy, ox), (buf, by, bx), w, h)
            for (ox, oy, bx, by, fx, fy, _, _) in items]


@pytest.mark.parametrize("tap4", (False, True))
@pytest.mark.parametrize("bd", M.BITDEPTHS)
def test_error_families(hip, oracle, bd, tap4):
    """every size: all page pairs at integer displacement and the 255 phases of the tap set, one launch per size"""
    hp = hip.hp
    org, buf = M.err_planes(bd)
    po, pb = hp.plane(org, 0), hp.plane(buf, 0)
    assert (po.stride, pb.stride) == (M.ORG_W, M.BUF_W)              # the footprints were laid out against these pitches (mctf_extremes._place)
    total = 0
    for (w, h) in M.ERR_SIZES:
        items, _ = M.err_items(bd, w, h, tap4)
        r_lo, r_hi, c_lo, c_hi = M.err_footprint(w, h)
        assert all(bx + c_lo >= 0 and bx + c_hi < M.BUF_W and by + r_lo >= 0 and by + r_hi < buf.shape[0] and ox >= 0 and ox + w <= M.ORG_W and oy + h <= org.shape[0]
                   for (ox, oy, bx, by, _, _, _, _) in items)
        got = _errors(hp, po, pb, M.err_records(items), w, h, tap4, bd)
        exp = _oracle_errors(oracle, org, buf, items, w, h, tap4, bd)
        bad = [(k, items[k][4:7], got[k], exp[k]) for k in range(len(exp)) if got[k] != exp[k]]
        assert not bad, (bd, w, h, tap4, len(bad), bad[:4])
        total += len(exp)
    assert total >= 64 * 270


@pytest.mark.parametrize("bd", M.BITDEPTHS)
def test_error_saturated(hip, oracle, bd):
    """per size the pair whose sum is min(w h max^2, 2^31 - 1): the packed 16-bit subtraction and the dot-product accumulation at the top of `int`"""
    hp = hip.hp
    so, sb, items = M.saturated(bd)
    po, pb = hp.plane(so, 0), hp.plane(sb, 0)
    assert po.stride == pb.stride == M.BUF_W
    top = 0
    for (ox, oy, bx, by, w, h) in items:
        rec = np.zeros(1, M.ERR_ITEM)
        rec[0] = (oy * M.BUF_W + ox, by * M.BUF_W + bx, 0, 0)
        got = _errors(hp, po, pb, rec, w, h, True, bd)[0]
        assert got == oracle.mctf_err_int((so, oy, ox), (sb, by, bx), w, h) == M.sat_bound(bd, w, h), (bd, w, h, got)
        top = max(top, got)
    assert top == (M.INT_MAX if bd == 10 else 64 * 64 * 255 * 255)


def test_error_lists(hip, oracle):
    """n = 0, 1, 63, 64, 65, 300 of the 16x16 and 64x8 items of either tap set; n = 0 writes nothing and needs no pointers"""
    hp = hip.hp
    org, buf = M.err_planes(10)
    po, pb = hp.plane(org, 0), hp.plane(buf, 0)
    for (w, h, tap4) in ((16, 16, True), (64, 8, False)):
        items, _ = M.err_items(10, w, h, tap4)
        exp = _oracle_errors(oracle, org, buf, items, w, h, tap4, 10)
        for n in M.LIST_NS:
            sel = [(7 * i) % len(items) for i in range(n)]
            got = _errors(hp, po, pb, M.err_records([items[k] for k in sel]), w, h, tap4, 10)
            assert got == [exp[k] for k in sel], (w, h, tap4, n)
    assert hp.L.vvhip_mctf_error_batch(hp.ctx, None, 0, None, 0, 8, 8, 1, 10, None, 0, None) == 0


def test_error_argument_errors(hip, oracle):
    """sizes outside 8 .. 64 or no multiple of 8, bit depths 7 and 13, a negative n: VVHIP_E_ARG, nothing written, and the context stays usable"""
    import torch
    hp = hip.hp
    org, buf = M.err_planes(10)
    po, pb = hp.plane(org, 0), hp.plane(buf, 0)
    items, _ = M.err_items(10, 8, 8, True)
    d_items = hp.to_device(M.err_records(items[:4]))
    out = torch.full((4 + GUARD,), 0x5A5A5A5A, dtype=torch.int32, device=hp.device)
    for (w, h, bd, n) in ((0, 8, 10, 4), (8, 0, 10, 4), (4, 8, 10, 4), (12, 8, 10, 4), (8, 20, 10, 4), (72, 8, 10, 4), (8, 72, 10, 4), (8, 8, 7, 4), (8, 8, 13, 4), (8, 8, 10, -1)):
        rc = hp.L.vvhip_mctf_error_batch(hp.ctx, po.buf_ptr, po.stride, pb.buf_ptr, pb.stride, w, h, 1, bd, _ptr(d_items), n, _ptr(out))
        assert rc == -1 and hp.L.vvhip_last_error(hp.ctx), (w, h, bd, n, rc)
    torch.cuda.synchronize()
    assert bool((out == 0x5A5A5A5A).all())
    assert _errors(hp, po, pb, M.err_records(items[:4]), 8, 8, True, 10) == _oracle_errors(oracle, org, buf, items[:4], 8, 8, True, 10)


def test_calc_var(hip, oracle):
    """every size x kind in one launch per size; 16 guard entries past n"""
    import torch
    hp = hip.hp
    pat = int(np.array([FILL] * 8, np.uint8).view(np.int64)[0])
    for bd in M.BITDEPTHS:
        p = M.var_plane(bd)
        pp = hp.plane(p, 0)
        assert pp.stride == 136
        for (w, h) in M.VAR_SIZES:
            items = M.var_items(w, h)
            assert all(x + w <= 136 and y + h <= p.shape[0] for x, y, _ in items)
            n = len(items)
            out = torch.full((n + 16,), pat, dtype=torch.int64, device=hp.device)
            d_off = hp.to_device(np.array([y * pp.stride + x for x, y, _ in items], np.int32))
            assert hp.L.vvhip_mctf_calc_var_batch(hp.ctx, pp.buf_ptr, pp.stride, w, h, _ptr(d_off), n, _ptr(out)) == 0
            got = out.cpu().numpy()
            assert (got[n:] == pat).all()
            exp = [oracle.mctf_calc_var((p, y, x), w, h) for x, y, _ in items]
            assert [g / 256.0 for g in got[:n].tolist()] == exp, (bd, w, h, [k for _, _, k in items])


class Held:
    """a w x h plane with `pad` samples of border inside sentinel-filled storage: `base` samples in front, an odd pitch, four rows behind"""

    def __init__(self, hp, w, h, pad, arr=None):
        import torch
        self.w, self.h, self.pad = w, h, pad
        self.stride = w + 2 * pad + 3
        self.base = 37
        rows = h + 2 * pad + 4
        self.host = np.full(self.base + rows * self.stride, M.SENT16, np.int16)
        self.origin = self.base + pad * self.stride + pad
        if arr is not None:
            for y in range(h):
                self.host[self.origin + y * self.stride:self.origin + y * self.stride + w] = arr[y]
        self.dev = torch.from_numpy(self.host.copy()).to(hp.device)

    @property
    def buf_ptr(self):
        return C.c_void_p(self.dev.data_ptr() + 2 * self.origin)

    def read(self):
        """-> (the plane with its border, whether every sample outside it still holds the sentinel)"""
        now = self.dev.cpu().numpy()
        H, W = self.h + 2 * self.pad, self.w + 2 * self.pad
        inside = np.zeros(now.size, bool)
        first = self.origin - self.pad * self.stride - self.pad
        for y in range(H):
            inside[first + y * self.stride:first + y * self.stride + W] = True
        return now[inside].reshape(H, W), bool((now[~inside] == M.SENT16).all())


def _oracle_border(oracle, a, pad):
    h, w = a.shape
    buf = np.full((h + 2 * pad, w + 2 * pad), M.SENT16, np.int16)
    buf[pad:pad + h, pad:pad + w] = a
    if pad:
        oracle.L.orc_extend_border(C.c_void_p(buf.ctypes.data + 2 * (pad * (w + 2 * pad) + pad)), w + 2 * pad, w, h, pad)
    return buf


@pytest.mark.parametrize("bd", M.BITDEPTHS)
def test_subsample_and_border(hip, oracle, bd):
    """every plane x pad: extend_border in place, and subsample into a destination with that pad — plane and border equal the oracle's, nothing outside them is written,
    the source of the subsample stays as it was"""
    import torch
    hp = hip.hp
    for name, a in M.plane_cases(bd):
        h, w = a.shape
        for pad in M.PLANE_PADS:
            held = Held(hp, w, h, pad, a)
            assert hp.L.vvhip_extend_border(hp.ctx, held.buf_ptr, held.stride, w, h, pad) == 0
            got, clean = held.read()
            assert clean, (name, pad, "extend_border wrote outside the plane and its border")
            assert np.array_equal(got, _oracle_border(oracle, a, pad)), (name, pad)
            if h >= 2 and w >= 2:
                src = Held(hp, w, h, 0, a)
                dst = Held(hp, w // 2, h // 2, pad)
                assert hp.L.vvhip_mctf_subsample(hp.ctx, src.buf_ptr, src.stride, w, h, dst.buf_ptr, dst.stride, pad) == 0
                got, clean = dst.read()
                assert clean, (name, pad, "subsample wrote outside the plane and its border")
                assert np.array_equal(got, _oracle_border(oracle, oracle.mctf_subsample(np.ascontiguousarray(a)), pad)), (name, pad)
                assert np.array_equal(src.dev.cpu().numpy(), src.host), (name, pad, "the source was written")
    torch.cuda.synchronize()
    assert hp.L.vvhip_mctf_subsample(hp.ctx, None, 8, 1, 1, None, 8, 0) == -1 and hp.L.vvhip_extend_border(hp.ctx, None, 4, 4, 4, 1) == -1          # no room: refused before any launch


# ---- the search ------------------------------------------------------------------------------------------------------------------------------------------------
FIELDS3, FIELDS5 = ("x", "y", "error"), ("x", "y", "error", "rmsme", "overlap")


def _search_one(hip, oracle, case):
    import torch
    from vvenc_amd.hotpath import MV_DTYPE
    assert MV_DTYPE == M.MV_DTYPE
    hp = hip.hp
    exp = case.expected(oracle)
    lv = hip.mctf_me_levels(case.org, case.ref, case.bd, case.unit, case.speed, case.add_level)
    for k in range(5):
        assert (exp[k] is None) == (lv[k] is None), (case.name, k)
        if exp[k] is not None:
            for f in (FIELDS5 if k == 4 else FIELDS3):
                assert np.array_equal(lv[k][f], exp[k][f]), (case.name, "per-level route, level", k, f, np.argwhere(lv[k][f] != exp[k][f])[:4].tolist())
    cur, ref = hp.plane(case.org, M.PAD), hp.plane(case.ref, M.PAD)
    dh, dw = exp[4].shape
    out = torch.full((dw * dh + GUARD, M.MV_DTYPE.itemsize), FILL, dtype=torch.uint8, device=hp.device)
    hp.mctf_motion_estimation(cur, [ref], case.bd, case.unit, case.speed, case.add_level, out=[out])
    raw = out.cpu().numpy()
    assert (raw[dw * dh:] == FILL).all(), (case.name, "records past the field were written")
    full = raw[:dw * dh].reshape(-1).view(M.MV_DTYPE).reshape(dh, dw)
    for f in FIELDS5:
        assert np.array_equal(full[f], exp[4][f]), (case.name, "whole hierarchy", f, np.argwhere(full[f] != exp[4][f])[:4].tolist())


@pytest.mark.parametrize("cfg", range(len(M.CONFIGS)))
def test_search(hip, oracle, cfg):
    """the families a, b, c, f on the five geometries and d, e in the diagonal directions, for one unit, speed and add_level"""
    cases = M.search_cases(cfg)
    assert {c.family for c in cases} == set("abcdef") and len(cases) == 16
    for case in cases:
        _search_one(hip, oracle, case)


FALLBACK = r'''
import sys, json
sys.path.insert(0, %r); sys.path.insert(0, %r)
import numpy as np
import mctf_extremes as M
from hip_backend import HipBackend
from oracle.oracle import Oracle
hip, orc = HipBackend(), Oracle()
bad = []
for case in M.fallback_cases():
    exp = case.expected(orc)
    got = hip.mctf_me_levels(case.org, case.ref, case.bd, case.unit, case.speed, case.add_level)
    for k in range(5):
        if exp[k] is not None:
            for f in (("x", "y", "error", "rmsme", "overlap") if k == 4 else ("x", "y", "error")):
                if not np.array_equal(got[k][f], exp[k][f]):
                    bad.append((case.name, k, f))
    full = hip.mctf_me(case.org, case.ref, case.bd, case.unit, case.speed, case.add_level)[4]
    bad += [(case.name, "whole", f) for f in ("x", "y", "error", "rmsme", "overlap") if not np.array_equal(full[f], exp[4][f])]
print(json.dumps({"bad": bad, "cases": len(M.fallback_cases())}))
'''


def test_search_row_hand_off():
    """four pictures of family c and two of family d through meWavefrontKernel (VVHIP_MCTF_DIAG=0, read once per process: a fresh child)"""
    env = dict(os.environ, VVHIP_MCTF_DIAG="0")
    r = subprocess.run([sys.executable, "-c", FALLBACK % (ROOT, os.path.join(ROOT, "tests"))], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    res = json.loads(r.stdout.strip().splitlines()[-1])
    assert res["cases"] == 6 and res["bad"] == [], res


# ---- the apply side ----------------------------------------------------------------------------------------------------------------------------------------------
def _apply_planes(hp, case, c, out=None, refs=None):
    """vvhip_mctf_apply_plane on component c into sentinel-filled storage -> (return code, Held)"""
    cs = 1 if c else 0
    h, w = case.org[c].shape
    po = hp.plane(case.org[c], M.PAD >> cs)
    prs = [hp.plane(r[c], M.PAD >> cs) for r in (case.refs if refs is None else refs)]
    d_mvs = [hp.to_device(np.ascontiguousarray(m)) for m in case.mvs][:len(prs)]
    while len(d_mvs) < len(prs):
        d_mvs.append(d_mvs[0])
    n = len(prs)
    sigma, scaling = hp.mctf_filter_params(case.qp, case.bd, 0.95, c > 0)
    held = Held(hp, w, h, 0)
    rp = (C.c_void_p * n)(*[r.buf_ptr.value for r in prs])
    mp = (C.c_void_p * n)(*[m.data_ptr() for m in d_mvs])
    rs = (C.c_double * n)(*[M.REF_STRENGTHS[(case.ref_index[i % len(case.ref_index)])] for i in range(n)])
    rc = hp.L.vvhip_mctf_apply_plane(hp.ctx, po.buf_ptr, po.stride, w, h, cs, case.bd, case.unit, int(case.low_res), case.qp, n, rp, prs[0].stride, mp, case.wb, rs,
                                     C.c_double(scaling), C.c_double(sigma), held.buf_ptr, held.stride)
    return rc, held


@pytest.mark.parametrize("part", range(4))
def test_apply(hip, oracle, part):
    """every apply case, component by component; unit 32 has 32x32 luma blocks, which the entry refuses (its chroma planes, 16x16, run)"""
    hp = hip.hp
    cases = (M.apply_cases() + M.noise_cases())[part::4]
    ran = 0
    for case in cases:
        exp = case.expected(oracle)
        for c in range(3):
            rc, held = _apply_planes(hp, case, c)
            if case.unit == 32 and c == 0:
                assert rc == -1, (case.name, rc)
                got, clean = held.read()
                assert clean and (got == M.SENT16).all()
                continue
            assert rc == 0, (case.name, c, rc, hp.L.vvhip_last_error(hp.ctx))
            got, clean = held.read()
            assert clean, (case.name, c, "a sample outside the plane was written")
            assert np.array_equal(got, exp[c]), (case.name, c, int((got != exp[c]).sum()), np.argwhere(got != exp[c])[:4].tolist())
            ran += 1
    assert ran >= 3 * len(cases) - sum(c.unit == 32 for c in cases)


def test_apply_refuses_13_references(hip, oracle):
    """12 references run (the cases above), 13 are refused with the output untouched; the context stays usable"""
    hp = hip.hp
    case = [c for c in M.apply_cases() if len(c.refs) == 12 and c.unit == 16][0]
    rc, held = _apply_planes(hp, case, 0, refs=case.refs + case.refs[:1])
    assert rc == -1 and hp.L.vvhip_last_error(hp.ctx)
    got, clean = held.read()
    assert clean and (got == M.SENT16).all()
    rc, held = _apply_planes(hp, case, 0)
    assert rc == 0 and np.array_equal(held.read()[0], case.expected(oracle)[0])
