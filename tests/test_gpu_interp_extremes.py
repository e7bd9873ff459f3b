"""-m gpu: every sub-pel interpolation entry against the oracle (tolerance 0) on the extreme inputs of tests/interp_extremes.py, at 8, 10 and 12 bits.  The oracle itself is
pinned to the compiled reference on the same cases by tests/test_oracle_interp_extremes.py, which also holds the guards (both final clips, both first-pass bounds, the
largest and smallest second-pass sums, both ends of addAvg, SSEs beyond 2^32) and the sensitivity test that shows the cases catch a wrong rounding offset, a one-sided
clip, an unmirrored tap row, the 4x4 / 4x8 tap-set rules, the alternative half-sample rules, an undoubled chroma phase and a copy form without its bias.

What is compared (entries x forms x bit depths; per bit depth unless noted):
  vvhip_if_filter (ifSlotKernel)         8 / 6 (two sets) / 4 / 2 taps x every phase x horizontal / vertical x the four first / last combinations x (matched, complement and
                                         two fillers at 24x9; matched and complement at 1x9 and 5x9; not-first: also 32767 / -32768): 5544 cases at 8 and 10 bits, 5064 at
                                         12, where the 2-tap first pass is rejected (asserted, with the output buffer unchanged)
  vvhip_if_copy (ifCopyKernel)           copy, first-not-last, last-not-first, DMVR's first pass (to 10 bits: its shift is 10 - bitDepth) x 1x9, 5x9, 24x9: 51 / 51 / 42 cases
  vvhip_interp_luma_batch                narrow kernel 4x4 (all 256 phases), 4x8, 4x16; wide kernel 8x4, 8x8, 16x16 (all 256 phases), 64x64, 128x8; filter_mode 0 with rnd_res
                                         1 / 0, filter_mode 1 / 2 at 4x4, 8x8 (all 256 phases), 16x16; alt on / off; origins on and off the residue: 44 launches, 4732 blocks
  vvhip_interp_chroma_batch              2x2, 4x2, 2x8, 8x8 (all 32x32 phases), 64x4 x rnd_res 1 / 0: 10 launches, 5354 blocks
  vvhip_subpel_dist_batch                SAD, SSE, HAD, HAD_fast x 8x8, 16x16, 32x16 (+ 64x64 at 12 bits, 128x64 at 10 bits: SSEs beyond 2^32) x filter_mode 0 / 1 / 2, alt
  vvhip_subpel_refine_batch              against the oracle directly: 8x8, 16x8, 16x16 (wave barrier), 32x16, 32x32 (workgroup barrier), 64x32 (expand path) x seven
                                         (filter_mode, alt, offsets) forms — half- and quarter-sample neighbourhoods, 16 offsets with 16 distinct dx over -16 .. 16 — x 8 bases
                                         with fractions 0, 8, 13, 14, 15: 42 launches, 3936 candidates
  vvhip_pred_inter_batch                 luma 4x4, 8x8, 16x4, 32x32, 128x16 and chroma 2x2, 4x4, 8x2, 32x8, uni (either list) and bi (matched with itself, its complement,
                                         a constant): 279 items in one launch, compact output, and once into a plane with sentinels around the blocks
Every expected value comes from the oracle (tests/pred_ref.py for the chroma composition and addAvg).

Measured on an MI355X, per case (each test runs once per bit depth): slot passes 0.24 to 0.36 s, luma batch 0.14 s, chroma batch 0.10 s, refinement 0.08 s, candidate
distortion 0.01 to 0.02 s, prediction list 0.01 s, copy forms below 0.005 s; the file 4.3 s with 1.7 s of set-up (the device context).
"""
import numpy as np
import pytest

import interp_extremes as X
import pred_ref as PR

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hip():
    from hip_backend import HipBackend
    return HipBackend()


def _items(blocks, at, stride, org=None):
    """SUBPEL_DTYPE records of blocks (ref key, x, y, xf, yf[, org key]) in the atlas `at`"""
    from vvenc_amd.hotpath import SUBPEL_DTYPE
    it = np.zeros(len(blocks), SUBPEL_DTYPE)
    for k, b in enumerate(blocks):
        key, x, y, xf, yf = b[:5]
        it[k] = (0 if org is None else (org.row(b[5]) + y) * stride + x, (at.row(key) + y) * stride + x, xf, yf)
    return it


@pytest.mark.parametrize("bd", X.BITDEPTHS)
def test_slot_passes(hip, oracle, bd):
    """ifSlotKernel: every tap count, phase, direction and first / last combination on the matched planes, their complements and transposes, the reachable first-pass
    extremes and 32767 / -32768; widths 1, 5 and 24; the documented rejection of the 2-tap first pass beyond 10 bits"""
    x, y = X.ORIGIN
    n = 0
    for set_, p, vertical, first, last, name, pl, w, h, _ in X.slot_cases(bd):
        row, nt = X.table_row(set_, p), X.ntaps(set_)
        got = hip.if_filter(nt, vertical, first, last, bd, (pl, y, x), w, h, row)
        exp = oracle.if_filter(nt, vertical, first, last, bd, (pl, y, x), w, h, row)
        assert np.array_equal(got, exp), (bd, X.SET_NAMES[set_], p, vertical, first, last, name, w, h, np.argwhere(got != exp)[:4].tolist())
        n += 1
    assert n == (5544 if bd <= 10 else 5064)
    if bd > 10:
        import torch
        from vvenc_amd.lib import VVHipError
        hp = hip.hp
        src = hp.plane(X.filler("random", (1 << bd) - 1, 0, X.SLOT_H, X.SLOT_W), 0)
        dst = torch.full((9 * 24,), -99, dtype=torch.int16, device=hp.device)
        for vertical in (0, 1):
            for last in (0, 1):
                with pytest.raises(VVHipError):
                    hp.if_filter(2, vertical, 1, last, bd, src.storage, src.origin + y * src.stride + x, src.stride, dst, 0, 24, 24, 9, X.table_row(X.BILINEAR, 5))
        torch.cuda.synchronize()
        assert bool((dst == -99).all())
        hp.if_filter(2, 0, 0, 0, bd, src.storage, src.origin + y * src.stride + x, src.stride, dst, 0, 24, 24, 9, X.table_row(X.BILINEAR, 5))      # the context stays usable
        assert not bool((dst == -99).any())


@pytest.mark.parametrize("bd", X.BITDEPTHS)
def test_copy_forms(hip, oracle, bd):
    """ifCopyKernel in its four modes, samples and first-pass extremes, widths 1, 5 and 24"""
    x, y = X.ORIGIN
    for first, last, bi, name, pl, w, h, _ in X.copy_cases(bd):
        got = hip.if_copy(first, last, bd, (pl, y, x), w, h, bool(bi))
        exp = oracle.if_copy(first, last, bd, (pl, y, x), w, h, bool(bi))
        assert np.array_equal(got, exp), (bd, first, last, bi, name, w, h, np.argwhere(got != exp)[:4].tolist())


@pytest.mark.parametrize("bd", X.BITDEPTHS)
def test_luma_batch(hip, oracle, bd):
    """ifPredBatchKernel (width 4: eight blocks per workgroup) and ifPredBatchWideKernel (16 to 256 threads per block), every filter mode, alt, rnd_res, all 16x16
    phases on the separable planes, block counts that leave a workgroup partly empty"""
    hp = hip.hp
    dev, n = {}, 0
    for w, h, mode, alt, rnd, fam, blocks in X.luma_groups(bd):
        at = X.atlas(bd, fam)
        if fam not in dev:
            dev[fam] = hp.plane(at.arr, 0)
        pr = dev[fam]
        it = _items(blocks, at, pr.stride)
        got = hp.interp_luma_batch(pr, hp.to_device(it), len(blocks), w, h, bd, bool(rnd), mode, bool(alt)).cpu().numpy().reshape(len(blocks), h, w)
        for k, (key, x, y, xf, yf) in enumerate(blocks):
            exp = X.luma_expected(oracle, at.arr, at.row(key) + y, x, w, h, xf, yf, rnd, bd, alt, mode)
            assert np.array_equal(got[k], exp), (bd, w, h, mode, alt, rnd, key, x, y, xf, yf, np.argwhere(got[k] != exp)[:4].tolist())
        n += len(blocks)
    assert n == 4732


@pytest.mark.parametrize("bd", X.BITDEPTHS)
def test_chroma_batch(hip, oracle, bd):
    """vvhip_interp_chroma_batch: every size class of the 4-tap kernel forms, all 32x32 phases at 8x8, rnd_res 1 and 0"""
    hp = hip.hp
    at = X.atlas(bd, "chroma4")
    pr = hp.plane(at.arr, 0)
    n = 0
    for w, h, rnd, blocks in X.chroma_groups(bd):
        it = _items(blocks, at, pr.stride)
        got = hp.interp_chroma_batch(pr, hp.to_device(it), len(blocks), w, h, bd, bool(rnd)).cpu().numpy().reshape(len(blocks), h, w)
        for k, (key, x, y, xf, yf) in enumerate(blocks):
            exp = PR.chroma_pred(oracle, at.arr, at.row(key) + y, x, w, h, xf, yf, rnd, bd)
            assert np.array_equal(got[k], exp), (bd, w, h, rnd, key, x, y, xf, yf, np.argwhere(got[k] != exp)[:4].tolist())
        n += len(blocks)
    assert n == 5354


@pytest.mark.parametrize("bd", X.BITDEPTHS)
def test_subpel_dist(hip, oracle, bd):
    """vvhip_subpel_dist_batch: SAD, SSE, HAD and HAD_fast of the clipped predictions against two-level originals; 64x64 at 12 bits and 128x64 at 10 bits carry SSEs
    beyond 2^32"""
    hp = hip.hp
    org = X.org_atlas(bd)
    po = hp.plane(org.arr, 0)
    dev, big = {}, 0
    x, y = X.ORIGIN
    for w, h, mode, alt, items in X.dist_groups(bd):
        fam = X.LUMA_FAMILY[mode]
        at = X.atlas(bd, fam)
        if fam not in dev:
            dev[fam] = hp.plane(at.arr, 0)
        pr = dev[fam]
        assert po.stride == pr.stride
        d_it = hp.to_device(_items([(rk, x, y, xf, yf, ok) for ok, rk, xf, yf in items], at, pr.stride, org))
        preds = [np.ascontiguousarray(X.luma_expected(oracle, at.arr, at.row(rk) + y, x, w, h, xf, yf, 1, bd, alt, mode)) for _, rk, xf, yf in items]
        for func in X.DIST_FUNCS:
            got = hp.subpel_dist_batch(func, po, pr, d_it, len(items), w, h, bd, mode, bool(alt)).cpu().numpy().view(np.uint64)
            for k, (ok, rk, xf, yf) in enumerate(items):
                exp = oracle.dist(func, (org.arr, org.row(ok) + y, x), preds[k], w, h, bd, 0)
                assert int(got[k]) == exp, (bd, func, w, h, mode, alt, ok, rk, xf, yf, int(got[k]), exp)
                big += func == "SSE" and exp > 1 << 32
    assert bd == 8 or big > 0


@pytest.mark.parametrize("bd", X.BITDEPTHS)
def test_subpel_refine(hip, oracle, bd):
    """vvhip_subpel_refine_batch against the oracle directly (not against the candidate-list entry): the wave-barrier, workgroup-barrier and expand forms; half- and
    quarter-sample neighbourhoods and 16 offsets with 16 distinct horizontal ones over -16 .. 16; base fractions 0, 8, 13, 14, 15; zero phases in one direction, in
    both, and after the offset is added (the copy forms inside the two-pass identity); every filter mode and alt"""
    hp = hip.hp
    org = X.org_atlas(bd)
    po = hp.plane(org.arr, 0)
    dev, n = {}, 0
    x, y = X.ORIGIN
    for w, h, mode, alt, func, offs, bases in X.refine_groups(bd):
        fam = X.LUMA_FAMILY[mode]
        at = X.atlas(bd, fam)
        if fam not in dev:
            dev[fam] = hp.plane(at.arr, 0)
        pr = dev[fam]
        d_b = hp.to_device(_items([(rk, x, y, fx, fy, ok) for ok, rk, fx, fy in bases], at, pr.stride, org))
        got = hp.subpel_refine_batch(func, po, pr, d_b, len(bases), offs, w, h, bd, mode, bool(alt)).cpu().numpy().view(np.uint64)
        xy = [(x, org.row(ok) + y, x, at.row(rk) + y, fx, fy) for ok, rk, fx, fy in bases]
        exp = np.array(X.refine_expected(oracle, org.arr, at.arr, w, h, mode, alt, func, offs, xy, bd), np.uint64)
        assert np.array_equal(got, exp), (bd, w, h, mode, alt, func, len(offs), np.argwhere(got != exp)[:4].ravel().tolist(), got[:4], exp[:4])
        n += got.size
    assert n == 3936


@pytest.mark.parametrize("bd", X.BITDEPTHS)
def test_pred_list(hip, oracle, bd):
    """vvhip_pred_inter_batch, the plain list: every size class of pred.hip uni- and bi-predicted, luma and chroma, bi items of a matched plane with itself, its
    complement and a constant; compact output, then the same list into a plane with sentinels around the blocks"""
    import torch
    from vvenc_amd.hotpath import PRED_ITEM_DTYPE
    assert X.PRED_ITEM == PRED_ITEM_DTYPE
    hp = hip.hp
    fams, ats = X.pred_planes(bd)
    planes = [a.arr for a in ats]
    dev = [hp.plane(p, 0) for p in planes]
    it, pos, total = X.pred_list_records(bd, [d.stride for d in dev])
    exp = [PR.expected_block(oracle, planes, pos[k], it[k], bd) for k in range(it.size)]
    pred = torch.full((total,), -1, dtype=torch.int16, device=hp.device)
    hp.pred_inter_batch(dev, it, pred, 0, bd)
    got = pred.cpu().numpy()
    for k in range(it.size):
        w, h, o = int(it[k]["width"]), int(it[k]["height"]), int(it[k]["dst_off"])
        assert np.array_equal(got[o:o + w * h].reshape(h, w), exp[k]), (bd, "compact", k, w, h, int(it[k]["chroma"]), it[k]["frac"].tolist(), it[k]["ref_plane"].tolist())
    # into a plane: blocks two samples apart, everything between them keeps the sentinel
    pitch = 328
    where, rows = PR.shelf_pack([(int(r["width"]) + 2, int(r["height"]) + 2) for r in it], pitch)
    it2 = it.copy()
    for k, (px, py) in enumerate(where):
        it2[k]["dst_off"] = (py + 1) * pitch + px + 1
    plane = torch.full((rows * pitch,), -12345, dtype=torch.int16, device=hp.device)
    hp.pred_inter_batch(dev, it2, plane, pitch, bd)
    got = plane.cpu().numpy().reshape(rows, pitch).copy()
    for k, (px, py) in enumerate(where):
        w, h = int(it[k]["width"]), int(it[k]["height"])
        assert np.array_equal(got[py + 1:py + 1 + h, px + 1:px + 1 + w], exp[k]), (bd, "plane", k, w, h)
        got[py + 1:py + 1 + h, px + 1:px + 1 + w] = -12345
    assert (got == -12345).all(), (bd, "samples outside the blocks were written", np.argwhere(got != -12345)[:4].tolist())
