"""-m gpu: the picture-level prediction entries behind the interpolation — vvhip_pred_inter_batch_ex (BDOF, DMVR's padded reference), _blend (BCW, GEO), _ciip and
vvhip_pred_affine_batch (PROF) — on the extreme inputs of tests/pred_ext_extremes.py at 8, 10 and 12 bits, tolerance 0.

Expected values: tests/bdof_ref.py, blend_ref.py, ciip_ref.py and affine_ref.py.  The interpolation inside them is executed from the compiled reference (the `reflib` rows)
for the extension lists, as in tests/test_gpu_pred_bdof.py, and from the oracle for the blend, CIIP and affine lists, as in their own GPU tiers.  The models are pinned to
the reference's own functions at 12 bits — and, for BDOF, on the frames of these very lists at all three bit depths — by tests/test_oracle_pred_ext_extremes.py, which also
holds the guards (frames beyond the ring's range in both lists, |gradient| > 255, |dI| > 1023, both clip ends inside one unit, every tmpx / tmpy, negative sums the shifts
do not divide) and the model mutations.  Three files of those fixtures are replayed here directly: device == what the reference recorded.

What is compared (every test once per bit depth unless noted):
  BDOF units          153 units in 116 items: 16x16, 16x8, 8x16, 32x16, 64x64 on the separable two-level plane against itself, its complement and a checkerboard, both
                      plane orders, six phase pairs and alt_hpel, origins on and off the 3-mod-8 residue; compact, then into a plane with sentinels round the blocks
  low-noise pictures  60 units over a flow field (every value of tmpx and tmpy), compact with the residual
  padded reference    158 items on planes in column / row runs of two: luma deltas +-2 and +-1 with and without BDOF, chroma +-1; compact, then into a plane
  BCW / GEO           the 216 items of blend_cases.extremes_list at 12 bits (8 and 10: tests/test_gpu_pred_blend.py)
  CIIP                96 items: lines all 0, all max, alternating; inter part uni, bi, BCW 0 / 4 from the checkerboards at fractional phases; num_intra 0..2
  affine, PROF        affine_cases.extreme_list and edge_list at 12 bits on texture, checkerboard, all-zero and all-max planes, CTU 32 and 128
  fixture replay      bdof_limits.npz (the frames a plane produces at fraction zero), ciip_limits.npz, affine_limits.npz

Mutation evidence on the device (one arithmetic line of pred.hip / predaffine.hip broken at a time in a scratch copy, this file run once; every mutation was caught):
  tmpx shift as a division, tmpy shift as a division, the halving dropped, the offset clip at 14 (tmpx) or 16 (tmpy), tmpx unpacked without its sign, tmpy unpacked with
  a logical shift, the vertical gradient or dI by division instead of shift, the rounding offset dropped, the ring's store cut to 13 bits, sSign counting g where the
  vertical gradient is zero               -> BDOF units, low-noise pictures, padded reference, BDOF fixture replay (all bit depths)
  the halving as a division               -> low-noise pictures only (10 and 12 bits on the device; the CPU guard finds such units at 8 bits as well)
  tdi cut to 12 bits, the 14-bit frame store cut to 15 bits -> BDOF units only        tgx cut to 9 bits -> BDOF units, padded reference
  BCW / GEO shift as hr + 2               -> BCW / GEO
  CIIP weight as num_intra, rounding + 1  -> CIIP, CIIP fixture replay
  PROF limit 1 << 12, limit symmetric     -> affine (the second on the checkerboards only); dMv clip at 30 -> affine, affine fixture replay

Measured on an MI355X, per test (the extension tests run once per reference row): BDOF units 0.03 to 0.15 s, low-noise pictures 0.01 s, padded reference 0.02 to 0.03 s,
BCW / GEO 0.02 s, CIIP 0.01 s, affine 0.07 to 0.16 s at CTU 32 and 0.31 to 0.33 s at CTU 128 (the model's 4x4 sub-blocks on the host), the fixture replays 0.03 and 0.08 s;
the file 4.7 s with 1.8 s of set-up (the device context).
"""
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
import bdof_cases as BC  # noqa: E402
import bdof_ref as BR  # noqa: E402
import blend_cases as BLC  # noqa: E402
import ciip_cases as CC  # noqa: E402
import ciip_ref as CR  # noqa: E402
import pred_ext_extremes as E  # noqa: E402
import pred_ref as PR  # noqa: E402

SENTINEL = -12345
GOLDEN = os.path.join(ROOT, "tests", "golden")


@pytest.fixture(scope="module")
def hp():
    from vvenc_amd.hotpath import HotPath
    return HotPath()


_dev = {}


def dev_planes(hp, key, arrays):
    """device copies of a set of planes, uploaded once per module"""
    if key not in _dev:
        _dev[key] = [hp.plane(a, 0) for a in arrays]
        for a, p in zip(arrays, _dev[key]):
            assert p.stride == a.shape[1]
    return _dev[key]


def explain(g, e, it):
    """item, unit and first differing samples of a block that is not the expected one"""
    where = np.argwhere(g != e)
    y, x = (int(v) for v in where[0])
    return dict(item=it, unit=(x // 16, y // 16), differing=len(where), first=[(int(b), int(a), int(g[b, a]), int(e[b, a])) for b, a in where[:4]])


def run_both_layouts(hp, dev, items, bd, exp, what, org=None, org_np=None, **records):
    """the list compact (with the residual when `org` is given), then into a plane with one sample of sentinel round every block: both equal `exp`, nothing else is written"""
    import torch
    items = items.copy()
    off, total = BC.compact_offsets(items)
    items["dst_off"] = off
    BLC.check_no_overlap(items, total)
    pred = torch.full((total,), SENTINEL, dtype=torch.int16, device=hp.device)
    resi = torch.full((total,), SENTINEL, dtype=torch.int16, device=hp.device) if org is not None else None
    hp.pred_inter_batch(dev, items, pred, 0, bd, org, resi, **records)
    torch.cuda.synchronize()
    got, r_all = pred.cpu().numpy(), (resi.cpu().numpy() if org is not None else None)
    for k, it in enumerate(items):
        w, h, o = int(it["width"]), int(it["height"]), int(it["dst_off"])
        g = got[o:o + w * h].reshape(h, w)
        assert np.array_equal(g, exp[k]), (what, bd, "compact", k, explain(g, exp[k], it))
        if org is not None:
            oy, ox = divmod(int(it["org_off"]), org.stride)
            assert np.array_equal(r_all[o:o + w * h].reshape(h, w), PR.residual(org_np[oy:oy + h, ox:ox + w], exp[k])), (what, bd, "residual", k, it)
    pitch = 328
    where, rows = PR.shelf_pack([(int(r["width"]) + 2, int(r["height"]) + 2) for r in items], pitch)
    it2 = items.copy()
    for k, (px, py) in enumerate(where):
        it2[k]["dst_off"] = (py + 1) * pitch + px + 1
    BLC.check_no_overlap(it2, rows * pitch, pitch)
    plane = torch.full((rows * pitch,), SENTINEL, dtype=torch.int16, device=hp.device)
    hp.pred_inter_batch(dev, it2, plane, pitch, bd, **records)
    torch.cuda.synchronize()
    got = plane.cpu().numpy().reshape(rows, pitch).copy()
    for k, (px, py) in enumerate(where):
        w, h = int(items[k]["width"]), int(items[k]["height"])
        g = got[py + 1:py + 1 + h, px + 1:px + 1 + w]
        assert np.array_equal(g, exp[k]), (what, bd, "plane", k, explain(g, exp[k], items[k]))
        got[py + 1:py + 1 + h, px + 1:px + 1 + w] = SENTINEL
    assert (got == SENTINEL).all(), (what, bd, "samples outside the blocks were written", np.argwhere(got != SENTINEL)[:4].tolist())


def _extension(hp, reflib, bd, name, lst, residual=False):
    pl = E.planes(bd)
    items, ext, pos = lst
    E.check_margins(pl, items, ext, pos)
    dev = dev_planes(hp, ("ext", bd), pl)
    exp = [BR.expected_block_ex(reflib, pl, pos[k], items[k], ext[k], bd) for k in range(len(items))]
    org = org_np = None
    if residual:
        items = items.copy()
        org_np, org = pl[E.RAMP0], dev[E.RAMP0]
        for k in range(len(items)):
            items["org_off"][k] = pos[k][0][1] * org.stride + pos[k][0][0]
    run_both_layouts(hp, dev, items, bd, exp, "%s (%s)" % (name, reflib.name), org, org_np, ext=ext)


# ---- 1 ----
@pytest.mark.parametrize("bd", E.BITDEPTHS)
def test_bdof_units_on_two_level_planes(hp, reflib, bd):
    """frames far outside the ring's range in both lists, gradients and dI beyond what samples give, both clip ends inside one unit: every (int16_t) store, the packed
    tmpx | tmpy << 16 shuffle and the arithmetic shifts of negative sums of the BDOF body"""
    _extension(hp, reflib, bd, "BDOF units", E.bdof_list(bd))


# ---- 2 ----
@pytest.mark.parametrize("bd", E.BITDEPTHS)
def test_bdof_low_noise_pictures(hp, reflib, bd):
    """the interior of the tmpx / tmpy range: every value from -15 to 15; with the residual"""
    _extension(hp, reflib, bd, "low-noise pictures", E.ramp_list(bd), residual=True)


# ---- 3 ----
@pytest.mark.parametrize("bd", E.BITDEPTHS)
def test_padded_reference_on_two_level_planes(hp, reflib, bd):
    """the clamped column / row carries the other level than the unclamped read would fetch, in every moved list of every item; with and without BDOF, luma and chroma"""
    _extension(hp, reflib, bd, "padded reference", E.dmvr_list(bd))


# ---- 4 ----
def test_bcw_geo_at_12_bits(hp, oracle):
    """blend_cases.extremes_list at 12 bits: the 0 / max checkerboards at half-sample fractions under the weights -2 / 10 and GEO edges; both clip ends"""
    pl, items, ext, blend, pos = E.blend_list(12)
    BLC.check_margins(pl, items, ext, pos)
    exp = [BLC.expected(oracle, pl, pos[k], items[k], ext[k], blend[k], 12) for k in range(len(items))]
    assert any(e.min() == 0 and e.max() == 4095 for e in exp)
    run_both_layouts(hp, dev_planes(hp, ("blend", 12), pl), items, 12, exp, "BCW / GEO", blend=blend)


# ---- 5 ----
@pytest.mark.parametrize("bd", E.BITDEPTHS)
def test_ciip_extreme_lines_behind_a_real_interpolation(hp, oracle, bd):
    """reference lines all 0, all max and alternating on the smallest and largest luma and chroma sizes; the inter part uni, bi, BCW 0 and BCW 4 from the checkerboards
    at fractional phases (both ends of its clip act); num_intra 0..2"""
    import torch
    pl, items, ext, blend, ciip, lines, pos = E.ciip_list(bd)
    BLC.check_margins(pl, items, ext, pos)
    assert int(ciip["ref_off"].min()) >= 0 and all(int(c["ref_off"]) + CR.line_len(int(i["width"]), int(i["height"])) <= lines.size for c, i in zip(ciip, items))
    exp = [CC.expected(oracle, pl, pos[k], items[k], ext[k], blend[k], ciip[k], lines, bd) for k in range(len(items))]
    dl = torch.from_numpy(np.ascontiguousarray(lines, np.int16)).to(hp.device)
    run_both_layouts(hp, dev_planes(hp, ("blend", bd), pl), items, bd, exp, "CIIP", blend=blend, ciip=ciip, intra_ref=dl)


# ---- 6 ----
def _affine_run(hp, planes, items, bd, pic_w, pic_h, ctu):
    import torch
    total = AC.compact_offsets(items)[1]
    pred = torch.full((total,), SENTINEL, dtype=torch.int16, device=hp.device)
    hp.pred_affine_batch([hp.plane(a, 0) for a in planes], items, pred, 0, bd, pic_w, pic_h, ctu)
    torch.cuda.synchronize()
    return pred.cpu().numpy()


def _affine_block(buf, it):
    c = int(it["chroma"])
    bw, bh = int(it["cu_w"]) >> c, int(it["cu_h"]) >> c
    return buf[int(it["dst_off"]):int(it["dst_off"]) + bw * bh].reshape(bh, bw)


@pytest.mark.parametrize("ctu,kind", E.AFFINE_WORLDS, ids=["ctu%d-%s" % w for w in E.AFFINE_WORLDS])
def test_affine_prof_at_12_bits(hp, oracle, ctu, kind):
    """affine_cases.extreme_list (dMv at +-31; on the checkerboard dI in its clip) and edge_list (the picture clip) at 12 bits"""
    world, lists = E.affine_lists(12, ctu, kind)
    top = 4095
    for name, items, pos in lists:
        for it in items:
            assert max(AR.read_extent(it, world.pic_w, world.pic_h, ctu)) <= world.m >> int(it["chroma"]), (name, it)
        pred = _affine_run(hp, world.np, items, 12, world.pic_w, world.pic_h, ctu)
        for k in range(len(items)):
            e = AR.expected_block(oracle, world.np, pos[k], items[k], 12, world.pic_w, world.pic_h, ctu)
            g = _affine_block(pred, items[k])
            assert np.array_equal(g, e), (name, ctu, kind, k, explain(g, e, items[k]))
        if kind in ("zero", "max"):
            assert np.all(pred == (0 if kind == "zero" else top))
        assert pred.min() >= 0


# ---- 7 ----
def _plane_from_frame(frame, bd):
    """a plane whose samples, read with fraction zero, give exactly this frame — or None"""
    hr = max(2, 14 - bd)
    v = (frame.astype(np.int32) + 8192) >> hr
    ok = np.array_equal(((v << hr) - 8192).astype(np.int16), frame) and v.min() >= 0 and v.max() < (1 << bd)
    return v.astype(np.int16) if ok else None


def test_bdof_fixture_frames_on_the_device(hp):
    """the recorded cases of bdof_limits.npz whose frames a plane can produce at fraction zero (flat blocks, the extreme values 0 and max, pictures; 12 bits above all):
    device output == what the reference's xApplyBDOF recorded"""
    import torch
    z = np.load(os.path.join(GOLDEN, "bdof_limits.npz"))
    ran = {}
    for bd in E.BITDEPTHS:
        sel = []
        for i in range(int(z["n"])):
            hdr = z["c%03d_hdr" % i]
            if int(hdr[0]) != bd:
                continue
            p0, p1 = _plane_from_frame(z["c%03d_f0" % i], bd), _plane_from_frame(z["c%03d_f1" % i], bd)
            if p0 is not None and p1 is not None:
                sel.append((p0, p1, int(hdr[1]), int(hdr[2]), z["c%03d_scalar" % i]))
        ran[bd] = len(sel)
        if not sel:
            continue
        cell = 16 + 2 + 16
        W = (cell * len(sel) + 16 + 7) // 8 * 8
        big = [np.zeros((cell + 1, W), np.int16) for _ in (0, 1)]
        items, ext = np.zeros(len(sel), BC.PRED_ITEM_DTYPE), np.zeros(len(sel), BC.PRED_EXT_DTYPE)
        for k, (p0, p1, w, h, _) in enumerate(sel):
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
        got = pred.cpu().numpy()
        for k, (_, _, w, h, want) in enumerate(sel):
            g = got[int(off[k]):int(off[k]) + w * h].reshape(h, w)
            assert np.array_equal(g, want), (bd, k, explain(g, want, items[k]))
    print("fixture cases run on the device:", ran)
    assert ran[12] >= 25, ran


def test_ciip_and_affine_fixtures_on_the_device(hp):
    """ciip_limits.npz: every case as a uni-predicted item with a zero fraction on a plane that holds its inter block, at 12 bits: output == the result the reference
    recorded.  affine_limits.npz: the cases from the fixture's 12-bit planes: output == what xPredAffineBlk recorded (two lists: their default average)"""
    import torch
    z = np.load(os.path.join(GOLDEN, "ciip_limits.npz"))
    cases = [dict(zip(("bd", "w", "h", "chroma", "num_intra"), (int(v) for v in z["c%03d_hdr" % i])), line=z["c%03d_line" % i], inter=z["c%03d_inter" % i],
                  result=z["c%03d_result" % i]) for i in range(int(z["n"]))]
    plane, items, ciip, lines = CC.golden_replay_list(cases)
    dev = [hp.plane(plane, 0)]
    assert dev[0].stride == plane.shape[1]
    total = BC.compact_offsets(items)[1]
    pred = torch.full((total,), SENTINEL, dtype=torch.int16, device=hp.device)
    hp.pred_inter_batch(dev, items, pred, 0, 12, ciip=ciip, intra_ref=torch.from_numpy(np.ascontiguousarray(lines, np.int16)).to(hp.device))
    got = pred.cpu().numpy()
    for k, (it, c) in enumerate(zip(items, cases)):
        g = got[int(it["dst_off"]):int(it["dst_off"]) + c["w"] * c["h"]].reshape(c["h"], c["w"])
        assert np.array_equal(g, c["result"]), ("CIIP fixture", k, explain(g, c["result"], it))
    (pic_w, pic_h, ctu, _), planes, acases = E.affine_limits_cases()
    aitems = np.concatenate([np.stack([lu, ch]) for (_, lu, ch, _, _) in acases])
    aitems["dst_off"] = AC.compact_offsets(aitems)[0]
    pred = _affine_run(hp, planes[12], aitems, 12, pic_w, pic_h, ctu)
    for k, (_, lu, ch, pos, rec) in enumerate(acases):
        for cc in (0, 1):
            blocks = [rec["scalar"][(l, cc)] for l in (0, 1) if (l, cc) in rec["scalar"]]
            e = blocks[0] if len(blocks) == 1 else PR.bi_average(blocks[0], blocks[1], 12)
            g = _affine_block(pred, aitems[2 * k + cc])
            assert np.array_equal(g, e), ("affine fixture", k, cc, explain(g, e, aitems[2 * k + cc]))
