"""Expected values for the MMVD merge-candidate entry (vvhip_merge_mmvd_costs_batch, vvhip_mmvd_candidate): a model shared by the CPU and GPU tests.

Steps 1 to 3 — the candidate's vectors — are restated here in plain Python integers, line by line after the reference and independently of vvenc_amd/csrc/mmvd_cand.h:
  MergeCtx::getMmvdDeltaMv          CommonLib/ContextModelling.cpp:261-342
  MergeCtx::setMmvdMergeCandiInfo   :344-404   (Mv::clipToStorageBitDepth Mv.h:274-278, CU::restrictBiPredMergeCandsOne UnitTools.cpp:3085-3097)
  CU::getDistScaleFactor            CommonLib/UnitTools.cpp:1354-1371;  Mv::scaleMv  CommonLib/Mv.h:182-187
  xCheckIdenticalMotion             CommonLib/InterPrediction.cpp:292-324;  clipMv  CommonLib/Mv.cpp:68-80
Steps 4 and 5 stand on the existing models: every interpolation pass and the Hadamard sum are EXECUTED from the library handed in (`Oracle()`, the C restatement, or a
`RefLib` row of the compiled reference) as tests/pred_ref.py does, the averages are pred_ref.bi_average / blend_ref.blend.

A CU is a dict: w, h, cu_x, cu_y, mask ( two 32-bit words ), bases = two dicts with mv ( ( x, y ) per list ), ref ( plane index or -1 per list ), poc ( reference POC minus
current POC per list ), lt ( long-term per list ), bcw, alt.  `cnt` collects the branches a run went through (REQUIRED: what the case list has to reach)."""
import numpy as np

import blend_ref as BL
import pred_ref as PR

MV_MIN, MV_MAX = -(1 << 17), (1 << 17) - 1
COST_BOUND = 256 * (64 * 64 * 4095 // 4)      # a 128 x 128 CU at 12 bits: 256 tiles of 8 x 8, 64 coefficients of at most 64 * 4095 each, normalised by 4
assert COST_BOUND < 1 << 32

REQUIRED = ("equal_dist", "scale_onto_l0", "scale_onto_l1", "opposite_sides", "scale_at_clip", "lt_copy", "lt_mirror", "dis_frac", "storage_clip",
            "pic_clip_left", "pic_clip_right", "pic_clip_top", "pic_clip_bottom", "bi_to_uni_8x4", "bi_to_uni_4x8", "identical_motion", "uni_l0", "uni_l1",
            "bcw0", "bcw1", "bcw2", "bcw3", "bcw4", "alt_hpel_phase8", "frac_x0", "frac_y0", "frac_both0",
            "HAD_8x8", "HAD_16x8", "HAD_8x16", "HAD_8x4", "HAD_4x8", "HAD_fast_8x8", "HAD_fast_16x16", "HAD_fast_16x8", "HAD_fast_8x16", "HAD_fast_8x4", "HAD_fast_4x8")


def bump(cnt, key):
    if cnt is not None:
        cnt[key] = cnt.get(key, 0) + 1


def clip3(lo, hi, v):
    return lo if v < lo else hi if v > hi else v


def cdiv(a, b):
    """C's integer division: towards zero"""
    q = abs(a) // abs(b)
    return q if (a < 0) == (b < 0) else -q


def dist_scale_factor(cur_poc, cur_ref_poc, col_poc, col_ref_poc, cnt=None):
    d, b = col_poc - col_ref_poc, cur_poc - cur_ref_poc
    if d == b:
        return 4096
    tdb, tdd = clip3(-128, 127, b), clip3(-128, 127, d)
    x = cdiv(0x4000 + abs(cdiv(tdd, 2)), tdd)
    if tdb != b or tdd != d:          # |B| <= |D| at both call sites, so the +-4096 clip of the factor cannot act: the clip that does is the one on the POC distances
        bump(cnt, "scale_at_clip")
    return clip3(-4096, 4095, (tdb * x + 32) >> 6)


def scale_mv(mv, scale):
    out = []
    for v in mv:
        p = scale * v
        out.append(clip3(MV_MIN, MV_MAX, (p + 128 - (1 if p >= 0 else 0)) >> 8))
    return tuple(out)


def delta_mv(base, val, dis_frac, cnt=None):
    step, pos = (val >> 2) & 7, val & 3
    offset = 1 << (step + 2)
    if dis_frac:
        offset <<= 2
        bump(cnt, "dis_frac")
    table = ((offset, 0), (-offset, 0), (0, offset), (0, -offset))
    d = [(0, 0), (0, 0)]
    r0, r1 = base["ref"][0] >= 0, base["ref"][1] >= 0
    if r0 and r1:
        poc0, poc1, cur = base["poc"][0], base["poc"][1], 0
        lt = base["lt"][0] or base["lt"][1]
        d[0] = table[pos]
        if poc0 - cur == poc1 - cur:
            d[1] = d[0]
            bump(cnt, "equal_dist")
        elif abs(poc1 - cur) > abs(poc0 - cur):
            scale = dist_scale_factor(cur, poc0, cur, poc1, None if lt else cnt)
            d[1] = d[0]
            if lt:
                if (poc1 - cur) * (poc0 - cur) > 0:
                    d[0] = d[1]
                    bump(cnt, "lt_copy")
                else:
                    d[0] = (-d[1][0], -d[1][1])
                    bump(cnt, "lt_mirror")
            else:
                d[0] = scale_mv(d[1], scale)
                bump(cnt, "scale_onto_l0")
                if scale < 0:
                    bump(cnt, "opposite_sides")
        else:
            scale = dist_scale_factor(cur, poc1, cur, poc0, None if lt else cnt)
            if lt:
                if (poc1 - cur) * (poc0 - cur) > 0:
                    d[1] = d[0]
                    bump(cnt, "lt_copy")
                else:
                    d[1] = (-d[0][0], -d[0][1])
                    bump(cnt, "lt_mirror")
            else:
                d[1] = scale_mv(d[0], scale)
                bump(cnt, "scale_onto_l1")
                if scale < 0:
                    bump(cnt, "opposite_sides")
    elif r0:
        d[0] = table[pos]
    elif r1:
        d[1] = table[pos]
    return d


def candidate(cu, val, pic_w, pic_h, ctu, dis_frac, cnt=None):
    """-> dict: stored ( cu.mv per list ), mv ( after clipMv ), used ( the lists the prediction reads ), bcw, alt"""
    base = cu["bases"][val >> 5]
    d = delta_mv(base, val, dis_frac, cnt)
    ref = [base["ref"][0], base["ref"][1]]
    assert ref[0] >= 0 or ref[1] >= 0
    stored = [(0, 0), (0, 0)]
    for l in (0, 1):
        if ref[l] >= 0:
            raw = (base["mv"][l][0] + d[l][0], base["mv"][l][1] + d[l][1])
            stored[l] = (clip3(MV_MIN, MV_MAX, raw[0]), clip3(MV_MIN, MV_MAX, raw[1]))
            if stored[l] != raw:
                bump(cnt, "storage_clip")
    bcw = base["bcw"] if ref[0] >= 0 and ref[1] >= 0 else 2
    if ref[0] >= 0 and ref[1] >= 0 and cu["w"] + cu["h"] == 12:                        # restrictBiPredMergeCandsOne
        ref[1], stored[1], bcw = -1, (0, 0), 2
        bump(cnt, "bi_to_uni_%dx%d" % (cu["w"], cu["h"]))
    used = [ref[0] >= 0, ref[1] >= 0]
    if used[0] and used[1] and base["poc"][0] == base["poc"][1] and stored[0] == stored[1]:      # xCheckIdenticalMotion: xPredInterUni of list 0
        used[1], bcw = False, 2
        bump(cnt, "identical_motion")
    hor = ((-ctu - 8 - cu["cu_x"] + 1) * 16, (pic_w + 8 - cu["cu_x"] - 1) * 16)
    ver = ((-ctu - 8 - cu["cu_y"] + 1) * 16, (pic_h + 8 - cu["cu_y"] - 1) * 16)
    mv = []
    for l in (0, 1):
        x, y = min(hor[1], max(hor[0], stored[l][0])), min(ver[1], max(ver[0], stored[l][1]))
        if used[l]:
            for key, hit in (("pic_clip_left", x > stored[l][0]), ("pic_clip_right", x < stored[l][0]), ("pic_clip_top", y > stored[l][1]), ("pic_clip_bottom", y < stored[l][1])):
                if hit:
                    bump(cnt, key)
        mv.append((x, y))
    if used[0] and used[1]:
        bump(cnt, "bcw%d" % bcw)
    else:
        bump(cnt, "uni_l0" if used[0] else "uni_l1")
    return dict(stored=stored, mv=mv, used=used, ref=[base["ref"][l] if used[l] else -1 for l in (0, 1)], bcw=bcw, alt=int(base["alt"]))


def predict(lib, planes, cu, val, cand, bd, cnt=None):
    """the luma prediction of a candidate; cu["pos"][b][l] = ( x, y ) of the CU at vector zero in planes[ref]"""
    b, w, h = val >> 5, cu["w"], cu["h"]
    blocks = []
    for l in (0, 1):
        if not cand["used"][l]:
            continue
        x, y = cu["pos"][b][l]
        mx, my = cand["mv"][l]
        fx, fy = mx & 15, my & 15
        bump(cnt, "frac_both0" if fx == 0 and fy == 0 else "frac_x0" if fx == 0 else "frac_y0" if fy == 0 else "frac_xy")
        if cand["alt"] and (fx == 8 or fy == 8):
            bump(cnt, "alt_hpel_phase8")
        rnd = not (cand["used"][0] and cand["used"][1])
        blocks.append(PR.luma_pred(lib, planes[cand["ref"][l]], y + (my >> 4), x + (mx >> 4), w, h, fx, fy, rnd, bd, cand["alt"]))
    if len(blocks) == 1:
        return blocks[0]
    if cand["bcw"] == 2:
        return PR.bi_average(blocks[0], blocks[1], bd)
    return BL.blend(blocks[0], blocks[1], BL.BLEND_BCW, cand["bcw"], bd)


def tile_kind(w, h, fast):
    """the ladder of RdCost::xGetHADs (RdCost.cpp:1818-1938): first match wins"""
    if w > h and h % 8 == 0 and w % 16 == 0:
        return "16x8"
    if w < h and w % 8 == 0 and h % 16 == 0:
        return "8x16"
    if w > h and h % 4 == 0 and w % 8 == 0:
        return "8x4"
    if w < h and w % 4 == 0 and h % 8 == 0:
        return "4x8"
    if fast and w == h and w % 32 == 0:
        return "16x16"
    if w % 8 == 0 and h % 8 == 0:
        return "8x8"
    return "4x4"


def cost(lib, org, ox, oy, pred, bd, fast, cnt=None):
    h, w = pred.shape
    bump(cnt, ("HAD_fast_" if fast else "HAD_") + tile_kind(w, h, fast))
    c = int(lib.dist("HAD_fast" if fast else "HAD", (org, oy, ox), (np.ascontiguousarray(pred), 0, 0), w, h, bd, 0))
    assert 0 <= c <= COST_BOUND, "a cost beyond the bound that makes 32 bits enough"
    return c


def vals_of(mask):
    return [v for v in range(64) if (int(mask[v >> 5]) >> (v & 31)) & 1]


def expected(lib, planes, org, cu, pic_w, pic_h, ctu, bd, fast, dis_frac, cnt=None, keep=None):
    """-> { val: cost } of the CU's requested candidates; keep: a dict that receives { val: ( candidate, prediction ) }"""
    out = {}
    for val in vals_of(cu["mask"]):
        cand = candidate(cu, val, pic_w, pic_h, ctu, dis_frac, cnt)
        pred = predict(lib, planes, cu, val, cand, bd, cnt)
        out[val] = cost(lib, org, cu["org_pos"][0], cu["org_pos"][1], pred, bd, fast, cnt)
        if keep is not None:
            keep[val] = (cand, pred)
    return out
