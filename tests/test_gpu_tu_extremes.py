"""-m gpu: every TU entry and every kernel form on the extreme inputs of tests/tu_extremes.py, against the oracle, tolerance 0.

  * vvhip_fwd_transform_batch / vvhip_inv_transform_batch: basis-aligned residuals at the bit-depth maximum, coefficient blocks that overflow
    the inverse first stage, the int8 byte-split edges; every shape 2..64, every legal type pair
  * vvhip_quant_batch / _dequant_batch / _need_rdoq_batch: the level edges (k = 1, 2, the clip at 32767), the need-RDOQ edge (luma and
    chroma), the coefficient-group edge, DeQuantCore's input clamp — every QP' of 8- and 10-bit video in one launch per shape
  * the raw table forms of the shim: vvhip_quant_core, _quant_core_lfnst, _dequant_core, _need_rdoq_core
  * vvhip_tu_rdo_batch in every form (matrix-core, row kernel, generic) and vvhip_tu_rdo_multi / _multi_strided (single launch and the
    per-kind split, sparse outputs off and on): residuals whose DC coefficient sits on a level / need-RDOQ edge, residuals whose
    coefficient-group decision hangs on `>` against `>=`, the forward-extreme set at every QP', luma and chroma, thr 8 and 4
  * residuals beyond the bit-depth contract (up to +-32767, both sides of the SSE fast path's -4096 / 4095 window): the forms agree
Output buffers are pre-filled with garbage: a form that skips a store fails.  Oracle results are pinned to the reference on the same
sets by tests/test_oracle_tu_extremes.py."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import tu_extremes as X  # noqa: E402

GARBAGE16, GARBAGE32 = 0x5A5A, 0x5A5A5A5A


@pytest.fixture(scope="module")
def env():
    from vvenc_amd.hotpath import HotPath
    from oracle.oracle import Oracle
    return HotPath(), Oracle()


def _p(t):
    import ctypes as C
    return C.c_void_p(t.data_ptr())


def _stats(sv, i):
    return (int(sv["abs_sum"][i]), int(sv["last_scan_pos"][i]), int(sv["need_rdoq"][i]), int(sv["sse"][i]))


# ---- transforms ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bd", [8, 10])
def test_transform_batches_on_extremes(env, bd):
    import torch
    from vvenc_amd.hotpath import Plane
    hp, orc = env
    for w in X.SIZES:
        for h in X.SIZES:
            for th, tv in X.tr_types(w, h):
                resi = X.fwd_residuals(orc.tr_matrix, w, h, th, tv, bd)
                n = len(resi)
                plane = Plane.from_numpy(hp.device, resi.reshape(n * h, w))
                d_off = hp.to_device(np.arange(n, dtype=np.int32) * (h * plane.stride))
                out = torch.full((n * w * h,), GARBAGE32, dtype=torch.int32, device=hp.device)
                got = hp.fwd_transform(plane, d_off, n, w, h, th, tv, bd, out=out).cpu().numpy().reshape(n, h, w)
                for i in range(n):
                    assert np.array_equal(got[i], orc.xT(resi[i], th, tv, bd)), ("xT", w, h, th, tv, bd, i)
                coef = X.inv_coefs(orc.tr_matrix, w, h, th, tv, seed=w * h)
                n = len(coef)
                plane = Plane(hp.device, w, n * h)
                plane.storage.fill_(GARBAGE16)
                d_off = hp.to_device(np.arange(n, dtype=np.int32) * (h * plane.stride))
                hp.inv_transform(hp.to_device(coef.ravel()), n, w, h, plane, d_off, th, tv, bd)
                got = plane.visible().cpu().numpy().reshape(n, h, w)
                for i in range(n):
                    assert np.array_equal(got[i], orc.xIT(coef[i], th, tv, bd)), ("xIT", w, h, th, tv, bd, i)


# ---- quantiser batches and raw forms --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bd", [8, 10])
def test_quant_batches_at_every_qp(env, bd):
    """one launch per (shape, thr) holds every QP' x irap; levels clip at 32767 somewhere, DeQuantCore's clamp bites somewhere"""
    import torch
    from vvenc_amd.hotpath import HotPath
    hp, orc = env
    clipped = clamp_bites = 0
    for w in X.SIZES:
        for h in X.SIZES:
            scan = orc.scan_order(X.log2(w), X.log2(h))
            for thr in (8, 4):
                blocks, qps, iraps = [], [], []
                for qp in range(X.qp_max(bd) + 1):
                    for irap in (0, 1):
                        b = X.quant_blocks(orc, w, h, bd, qp, irap, thr)
                        blocks.append(b); qps += [qp] * len(b); iraps += [irap] * len(b)
                coef = np.concatenate(blocks)
                n = len(coef)
                qps, iraps = np.array(qps), np.array(iraps)
                luma = np.arange(n) & 1
                d_coef = hp.to_device(coef.ravel())
                d_qp = hp.to_device(HotPath.tu_qp(qps, iraps, luma))
                lev = torch.full((n * w * h,), GARBAGE16, dtype=torch.int16, device=hp.device)
                du = torch.full((n * w * h,), GARBAGE32, dtype=torch.int32, device=hp.device)
                s = torch.full((n,), GARBAGE32, dtype=torch.int32, device=hp.device)
                last = torch.full((n,), GARBAGE32, dtype=torch.int32, device=hp.device)
                hp._ck(hp.L.vvhip_quant_batch(hp.ctx, _p(d_coef), n, w, h, bd, _p(d_qp), thr, _p(lev), _p(du), _p(s), _p(last)))
                lev, du = lev.cpu().numpy().reshape(n, h, w), du.cpu().numpy().reshape(n, h * w)
                s, last = s.cpu().numpy(), last.cpu().numpy()
                for i in range(n):
                    e = orc.quant_tu(coef[i], int(qps[i]), int(iraps[i]), thr, bd)
                    assert (int(s[i]), int(last[i])) == (e[2], e[3]), (w, h, bd, thr, int(qps[i]), i)
                    assert np.array_equal(lev[i], e[0]), ("levels", w, h, bd, thr, int(qps[i]), i)
                    keep = np.zeros(h * w, bool)
                    keep[scan[: e[3] + 1]] = True
                    assert np.array_equal(du[i][keep], e[1][keep]), ("deltaU", w, h, bd, thr, int(qps[i]), i)
                    clipped += int(np.abs(e[0].astype(np.int64)).max() == 32767)
                need = hp.need_rdoq(d_coef, n, w, h, d_qp, bd).cpu().numpy()
                for i in range(n):
                    assert int(need[i]) == orc.need_rdoq_tu(coef[i], int(qps[i]), int(luma[i]), bd), ("need", w, h, bd, int(qps[i]), i)
            # need-RDOQ edges (luma / chroma) and DeQuantCore's input clamp, every QP'
            nb, nq, nl, lv, lq = [], [], [], [], []
            for qp in range(X.qp_max(bd) + 1):
                for luma in (0, 1):
                    b = X.need_rdoq_blocks(orc, w, h, bd, qp, luma)
                    nb.append(b); nq += [qp] * len(b); nl += [luma] * len(b)
                d = X.dequant_levels(h, w, seed=qp)
                lv.append(d); lq += [qp] * len(d)
                clamp_bites += orc.dequant_params(w, h, bd, qp)[2] < 32767
            coef, lvl = np.concatenate(nb), np.concatenate(lv)
            d_qp = hp.to_device(HotPath.tu_qp(np.array(nq), 0, np.array(nl)))
            need = hp.need_rdoq(hp.to_device(coef.ravel()), len(coef), w, h, d_qp, bd).cpu().numpy()
            for i in range(len(coef)):
                assert int(need[i]) == orc.need_rdoq_tu(coef[i], nq[i], nl[i], bd), ("need edge", w, h, bd, nq[i], nl[i], i)
            d_qp = hp.to_device(HotPath.tu_qp(np.array(lq), 0, 1))
            out = torch.full((len(lvl) * w * h,), GARBAGE32, dtype=torch.int32, device=hp.device)
            hp._ck(hp.L.vvhip_dequant_batch(hp.ctx, _p(hp.to_device(lvl.ravel())), len(lvl), w, h, bd, _p(d_qp), _p(out)))
            deq = out.cpu().numpy().reshape(len(lvl), h, w)
            for i in range(len(lvl)):
                assert np.array_equal(deq[i], orc.dequant_tu(lvl[i], lq[i], bd)), ("dequant", w, h, bd, lq[i], i)
    assert clipped > 0 and clamp_bites > 0, (clipped, clamp_bites)


RAW_SHAPES = [(4, 4), (8, 8), (16, 16), (32, 32), (64, 64), (8, 4), (4, 16), (32, 8), (2, 8), (16, 64)]


@pytest.mark.parametrize("bd", [8, 10])
def test_raw_quant_forms_at_every_qp(env, bd):
    """the table-shaped forms (one block per call, QuantCore's own argument list): every QP' once per form and bit depth, the shapes in turn"""
    import ctypes as C
    import torch
    hp, orc = env
    dev = hp.device
    for qp in range(X.qp_max(bd) + 1):
        w, h = RAW_SHAPES[qp % len(RAW_SHAPES)]
        irap = qp & 1
        scale, q_bits, add = orc.quant_params(w, h, bd, qp, irap)
        for thr in (8, 4):
            for i, c in enumerate(X.quant_blocks(orc, w, h, bd, qp, irap, thr)):
                e = orc.quant_core(c, scale, q_bits, add, thr)
                d_c = hp.to_device(np.ascontiguousarray(c).ravel())
                d_l = torch.full((h * w,), GARBAGE16, dtype=torch.int16, device=dev)
                d_u = torch.full((h * w,), GARBAGE32, dtype=torch.int32, device=dev)
                d_s = torch.full((2,), GARBAGE32, dtype=torch.int32, device=dev)
                hp._ck(hp.L.vvhip_quant_core(hp.ctx, _p(d_c), w, h, scale, q_bits, add, thr, _p(d_l), _p(d_u), _p(d_s), C.c_void_p(d_s.data_ptr() + 4)))
                sv = d_s.cpu().numpy()
                assert (int(sv[0]), int(sv[1])) == (e[2], e[3]), ("quant_core", w, h, bd, qp, thr, i)
                assert np.array_equal(d_l.cpu().numpy().reshape(h, w), e[0]), ("quant_core levels", w, h, bd, qp, thr, i)
                for lf in (1, 2):
                    g = hp.quant_core(c, scale, q_bits, add, thr, lfnst_idx=lf)
                    e = orc.quant_core(c, scale, q_bits, add, thr, lfnst_idx=lf)
                    assert (g[2], g[3]) == (e[2], e[3]) and np.array_equal(g[0], e[0]), ("quant_core_lfnst", w, h, bd, qp, thr, lf, i)
        sc, rs, imax = orc.dequant_params(w, h, bd, qp)
        for i, lv in enumerate(X.dequant_levels(h, w, seed=qp)):
            stride = w + 3                                                  # strided levels, as the shim passes them
            pad = np.full((h, stride), 0x3333, np.int16)
            pad[:, :w] = lv
            d_c = torch.full((h * w,), GARBAGE32, dtype=torch.int32, device=dev)
            hp._ck(hp.L.vvhip_dequant_core(hp.ctx, w - 1, h - 1, sc, _p(hp.to_device(pad.ravel())), stride, _p(d_c), rs, imax, 32767))
            assert np.array_equal(d_c.cpu().numpy().reshape(h, w), orc.dequant_core(lv, sc, rs, imax)), ("dequant_core", w, h, bd, qp, i)
        for luma in (0, 1):
            qc, qb, off, num = orc.need_rdoq_params(w, h, bd, qp, luma)
            for i, c in enumerate(X.need_rdoq_blocks(orc, w, h, bd, qp, luma)):
                flat = np.ascontiguousarray(c.ravel()[:num])
                d_n = torch.full((1,), 0x5A, dtype=torch.uint8, device=dev)
                hp._ck(hp.L.vvhip_need_rdoq_core(hp.ctx, _p(hp.to_device(flat)), num, qc, off, qb, _p(d_n)))
                assert int(d_n.cpu().numpy()[0]) == orc.need_rdoq(flat, qc, off, qb), ("need_rdoq_core", w, h, bd, qp, luma, i)


# ---- the fused TU pipeline ------------------------------------------------------------------------------------------------------
def _cg_decisive(coef, scan, num, t):
    """True where QuantCore's coefficient-group decision (last scan position) differs between |c| > t and |c| >= t"""
    a = np.abs(coef.reshape(-1)[scan[:num]].astype(np.int64))
    nz = np.nonzero(a)[0]
    if nz.size == 0 or nz[-1] < 16:
        return False
    last = nz[-1]
    m = np.where(np.arange(num) <= last, a, 0).reshape(-1, 16).max(axis=1)[1:last // 16 + 1]
    g1 = np.nonzero(m > t)[0]
    g2 = np.nonzero(m >= t)[0]
    return (g1[-1] if g1.size else -1) != (g2[-1] if g2.size else -1)


def fused_lists(orc, w, h, th, tv, bd, thr, rng):
    """(residuals (n, h, w) int16, qps, irap, luma) of one fused list: the forward-extreme set at QPs that sweep the range, residuals on the
    level / need-RDOQ edges (DC coefficient), residuals whose coefficient-group decision is `>`-vs-`>=` sensitive (QP' = 4 mod 6)"""
    qmax = X.qp_max(bd)
    base = X.fwd_residuals(orc.tr_matrix, w, h, th, tv, bd)
    reps = 1 if w * h >= 1024 else (2 if w * h >= 256 else 4)
    resi = [np.tile(base, (reps, 1, 1))]
    qps = [rng.permutation(np.resize(np.arange(qmax + 1), len(resi[0])))]
    irap = [rng.integers(0, 2, len(resi[0]))]
    luma = [rng.integers(0, 2, len(resi[0]))]
    # DC on a level edge (k = 1, 2) / on the need-RDOQ edge, luma and chroma
    for qp in rng.choice(qmax + 1, size=4 if w * h >= 1024 else 8, replace=False):
        for flag in (0, 1):
            scale, qb, add = orc.quant_params(w, h, bd, int(qp), flag)
            nsc, nqb, noff, _ = orc.need_rdoq_params(w, h, bd, int(qp), flag)
            tg = []
            for k in (1, 2):
                e = X.level_edge(k, scale, qb, add)
                tg += [e, e - 1]
            e = X.level_edge(1, nsc, nqb, noff)
            tg += [e, e - 1]
            r = X.edge_residuals(orc, w, h, th, tv, bd, [t for t in tg if t < 32000], 8, seed=int(qp) * 2 + flag)
            resi.append(r); qps.append(np.full(len(r), qp)); irap.append(np.full(len(r), flag)); luma.append(np.full(len(r), flag))
    # coefficient-group edge: small residuals selected on the int64 model at QP' = 4 mod 6 (scale 16384: |c| * scale == thres >> 2 can hold)
    if w * h >= 64 and w >= 4 and h >= 4:
        Th, Tv = orc.tr_matrix(th, X.log2(w)).astype(np.int64), orc.tr_matrix(tv, X.log2(h)).astype(np.int64)
        num = min(w, 32) * min(h, 32)
        scan = orc.scan_order(X.log2(w), X.log2(h))
        sel, sq = [], []
        for qp in range(4, min(qmax, 40) + 1, 6):
            scale, qb, _ = orc.quant_params(w, h, bd, qp, 0)
            if scale != 16384:
                continue
            t = X.cg_thres(scale, qb, thr)
            amp = max(2, min((1 << bd) - 1, t // 3 + 2))
            cand = rng.integers(-amp, amp + 1, size=(64, h, w)) * (rng.random((64, h, w)) < 0.3)
            coef = X.zero_out(X.fwd_model(cand, Th, Tv, bd), th, tv)
            for i in range(len(cand)):
                if _cg_decisive(coef[i], scan, num, t):
                    sel.append(cand[i]); sq.append(qp)
                    if len(sel) % 3 == 0:
                        break
        if sel:
            resi.append(np.array(sel, np.int16)); qps.append(np.array(sq)); irap.append(rng.integers(0, 2, len(sel))); luma.append(np.ones(len(sel), int))
    n_cg = len(sel) if w * h >= 64 and w >= 4 and h >= 4 else 0
    return (np.concatenate(resi).astype(np.int16), np.concatenate(qps).astype(int), np.concatenate(irap).astype(int), np.concatenate(luma).astype(int), n_cg)


def _forms(w, h, th, tv):
    sq = w == h
    if sq and (w in (4, 8, 16, 32) or (w == 64 and (th, tv) == (0, 0))):
        yield "matrix-core"
    if sq and w in (8, 16, 32):
        yield "row"
    yield "generic"


def _set_form(monkeypatch, form):
    monkeypatch.delenv("VVHIP_TU_KERNEL", raising=False)
    monkeypatch.delenv("VVHIP_TU_GENERIC", raising=False)
    if form == "row":
        monkeypatch.setenv("VVHIP_TU_KERNEL", "row")
    elif form == "generic":
        monkeypatch.setenv("VVHIP_TU_GENERIC", "1")


def _run_batch(hp, resi, qps, irap, luma, w, h, th, tv, bd, thr):
    import torch
    from vvenc_amd.hotpath import STATS_DTYPE, HotPath, Plane
    n = len(resi)
    plane = Plane.from_numpy(hp.device, resi.reshape(n * h, w))
    d_off = hp.to_device(np.arange(n, dtype=np.int32) * (h * plane.stride))
    d_qp = hp.to_device(HotPath.tu_qp(qps, irap, luma))
    lev = torch.full((n * w * h,), GARBAGE16, dtype=torch.int16, device=hp.device)
    rec = torch.full((n * w * h,), GARBAGE16, dtype=torch.int16, device=hp.device)
    st = torch.full((n, STATS_DTYPE.itemsize), 0xA5, dtype=torch.uint8, device=hp.device)
    hp.tu_rdo(plane, d_off, n, w, h, d_qp, th, tv, bd, thr, level=lev, rec=rec, stats=st)
    return lev.cpu().numpy().reshape(n, h, w), rec.cpu().numpy().reshape(n, h, w), st.cpu().numpy().view(STATS_DTYPE).reshape(n)


FUSED_SHAPES = [(s, s) for s in (4, 8, 16, 32, 64)] + [(8, 4), (4, 8), (16, 4), (4, 16), (32, 8), (8, 32), (16, 32), (64, 32), (32, 64), (2, 8), (8, 2), (64, 16)]


@pytest.mark.parametrize("bd", [8, 10])
def test_fused_tu_forms_on_edges_vs_oracle(env, monkeypatch, bd):
    """vvhip_tu_rdo_batch, every form that takes the shape (matrix-core 4/8/16/32 all type pairs + 64 DCT-2, row 8/16/32, generic everything,
    non-square shapes), thr 8 and 4, luma and chroma, every QP' of the bit depth; guards: DC edges and coefficient-group-sensitive TUs were
    generated, the QP' range was covered per form, and at 10 bits one 64x64 TU has an SSE >= 2^31"""
    hp, orc = env
    rng = np.random.default_rng(9000 + bd)
    seen_qp = {}
    n_cg = n_edge = 0
    big_sse = 0
    for (w, h) in FUSED_SHAPES:
        for th, tv in X.tr_types(w, h):
            for thr in (8, 4):
                if thr == 4 and (th, tv) not in ((0, 0), (2, 2)):
                    continue
                resi, qps, irap, luma, k = fused_lists(orc, w, h, th, tv, bd, thr, rng)
                exp = [orc.tu_rdo(resi[i], int(qps[i]), int(irap[i]), th, tv, bd, thr, int(luma[i])) for i in range(len(resi))]
                n_edge += len(resi)
                n_cg += k
                for form in _forms(w, h, th, tv):
                    _set_form(monkeypatch, form)
                    lev, rec, sv = _run_batch(hp, resi, qps, irap, luma, w, h, th, tv, bd, thr)
                    seen_qp.setdefault(form, set()).update(int(q) for q in qps)
                    for i, (el, er, es) in enumerate(exp):
                        assert np.array_equal(lev[i], el), ("lev", form, w, h, th, tv, bd, thr, int(qps[i]), i)
                        assert np.array_equal(rec[i], er), ("rec", form, w, h, th, tv, bd, thr, int(qps[i]), i)
                        assert _stats(sv, i) == (es["abs_sum"], es["last_scan_pos"], es["need_rdoq"], es["sse"]), \
                            ("stats", form, w, h, th, tv, bd, thr, int(qps[i]), int(luma[i]), i, _stats(sv, i), es)
                        big_sse = max(big_sse, es["sse"])
    _set_form(monkeypatch, None)
    for form, qs in seen_qp.items():
        assert qs == set(range(X.qp_max(bd) + 1)), (form, sorted(set(range(X.qp_max(bd) + 1)) - qs))
    assert n_edge > 1000 and n_cg > 20, (n_edge, n_cg)
    assert big_sse >= (1 << 31 if bd == 10 else 4096 * 255 * 255 * 9 // 10), big_sse      # 64x64 checkerboard at +-(2^bd - 1): ~4096 (2^bd - 1)^2


@pytest.mark.parametrize("bd", [8, 10])
@pytest.mark.parametrize("sparse", [0, 1], ids=["dense", "sparse"])
def test_tu_rdo_multi_on_edges_vs_oracle(env, bd, sparse):
    """vvhip_tu_rdo_multi (one plane) and _multi_strided (compact blocks): a list set that fits one launch (<= 8 mergeable jobs) and one
    with 11 mergeable jobs (the per-kind split launches, 4x4 / 64x64 apart); sparse outputs: levels / reconstruction checked where abs_sum != 0"""
    import torch
    from vvenc_amd.hotpath import STATS_DTYPE, HotPath, Plane
    hp, orc = env
    rng = np.random.default_rng(300 + bd)
    small = [(8, 8, 0, 0, 8), (16, 16, 2, 2, 8), (32, 32, 0, 0, 4), (4, 4, 0, 0, 8), (64, 64, 0, 0, 8), (16, 8, 0, 0, 8)]
    large = small + [(8, 8, 1, 2, 4), (16, 16, 0, 0, 4), (32, 32, 2, 1, 8), (4, 4, 2, 2, 4), (8, 8, 0, 0, 4), (32, 32, 0, 0, 8), (8, 32, 0, 2, 8)]
    hp.tu_set_sparse_outputs(sparse)
    try:
        for spec in (small, large):
            lists = []
            for (w, h, th, tv, thr) in spec:
                resi, qps, irap, luma, _ = fused_lists(orc, w, h, th, tv, bd, thr, rng)
                keep = rng.permutation(len(resi))[:48]
                resi, qps, irap, luma = resi[keep], qps[keep], irap[keep], luma[keep]
                exp = [orc.tu_rdo(resi[i], int(qps[i]), int(irap[i]), th, tv, bd, thr, int(luma[i])) for i in range(len(resi))]
                lists.append((w, h, th, tv, thr, resi, qps, irap, luma, exp))
            for strided in (False, True):
                rows = sum(len(L[5]) * L[1] for L in lists)
                plane = Plane(hp.device, 64, rows)
                pool = np.concatenate([L[5].reshape(-1) for L in lists])
                d_pool = hp.to_device(pool)
                jobs, strides, at_row, at = [], [], 0, 0
                for (w, h, th, tv, thr, resi, qps, irap, luma, exp) in lists:
                    n = len(resi)
                    if strided:
                        off = at + np.arange(n, dtype=np.int32) * w * h
                    else:
                        plane.storage[at_row:at_row + n * h, :w] = torch.from_numpy(resi.reshape(n * h, w)).to(hp.device)
                        off = (at_row + np.arange(n, dtype=np.int32) * h) * plane.stride
                    lv = torch.full((n * w * h,), GARBAGE16, dtype=torch.int16, device=hp.device)
                    rc = torch.full((n * w * h,), GARBAGE16, dtype=torch.int16, device=hp.device)
                    st = torch.full((n, STATS_DTYPE.itemsize), 0xA5, dtype=torch.uint8, device=hp.device)
                    jobs.append((w, h, th, tv, n, thr, hp.to_device(off.astype(np.int32)), hp.to_device(HotPath.tu_qp(qps, irap, luma)), lv, rc, st))
                    strides.append(w)
                    at_row += n * h
                    at += n * w * h
                if strided:
                    hp.tu_rdo_multi_strided(d_pool, strides, jobs, bd)
                else:
                    hp.tu_rdo_multi(plane, jobs, bd)
                torch.cuda.synchronize()
                for L, J in zip(lists, jobs):
                    (w, h, th, tv, thr, resi, qps, irap, luma, exp) = L
                    lv, rc = J[8].cpu().numpy().reshape(-1, h, w), J[9].cpu().numpy().reshape(-1, h, w)
                    sv = J[10].cpu().numpy().view(STATS_DTYPE).reshape(-1)
                    for i, (el, er, es) in enumerate(exp):
                        what = (len(spec), strided, sparse, w, h, th, tv, bd, thr, int(qps[i]), i)
                        assert _stats(sv, i) == (es["abs_sum"], es["last_scan_pos"], es["need_rdoq"], es["sse"]), ("stats",) + what
                        if es["abs_sum"] or not sparse:
                            assert np.array_equal(lv[i], el), ("lev",) + what
                            assert np.array_equal(rc[i], er), ("rec",) + what
    finally:
        hp.tu_set_sparse_outputs(0)


def _beyond_contract(rng, S, n):
    """residuals outside the bit-depth contract: +-32767 sign patterns, uniform int16, and values on both sides of -4096 / 4095"""
    out = []
    yy, xx = np.mgrid[0:S, 0:S]
    for v in (32767, -32768, 4095, 4096, -4096, -4097):
        out.append(np.full((S, S), v))
        out.append(np.where((yy + xx) & 1, v, -v if v != -32768 else 32767))
    edges = np.array([4094, 4095, 4096, 4097, -4095, -4096, -4097, -4098, 12287, -12288, 0], np.int64)
    while len(out) < n:
        k = len(out) % 3
        if k == 0:
            out.append(rng.integers(-32768, 32768, (S, S)))
        elif k == 1:
            out.append(rng.choice(edges, (S, S)))
        else:
            out.append(rng.integers(-4200, 4200, (S, S)))
    return np.array(out, np.int16)


@pytest.mark.parametrize("bd", [8, 10])
def test_fused_forms_agree_beyond_the_contract(env, monkeypatch, bd):
    """residuals up to +-32767 and around the SSE fast path's window: matrix-core == row == generic, bit for bit (the oracle's scalar
    transform does not saturate like the kernels' x86-row passes, so the forms are held to each other)"""
    hp, _ = env
    rng = np.random.default_rng(77 + bd)
    for S in (4, 8, 16, 32, 64):
        for th, tv in ((0, 0), (2, 2), (1, 2)) if S <= 32 else ((0, 0),):
            resi = _beyond_contract(rng, S, 40 if S < 64 else 24)
            n = len(resi)
            qps = rng.integers(0, X.qp_max(bd) + 1, n)
            irap, luma = rng.integers(0, 2, n), rng.integers(0, 2, n)
            outs = {}
            for form in _forms(S, S, th, tv):
                _set_form(monkeypatch, form)
                outs[form] = _run_batch(hp, resi, qps, irap, luma, S, S, th, tv, bd, 8)
            _set_form(monkeypatch, None)
            ref = outs.pop("generic")
            for form, got in outs.items():
                for name, a, b in zip(("lev", "rec", "stats"), got, ref):
                    assert np.array_equal(a, b), (name, form, S, th, tv, bd)
