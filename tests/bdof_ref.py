"""Expected values for the extension forms of the inter-prediction list entry (vvhip_pred_inter_batch_ex): BDOF and DMVR's padded reference.

Builds on tests/pred_ref.py.  The 14-bit interpolation of each list is still EXECUTED from the library handed in (`RefLib(0)` scalar row, `RefLib(1)` x86 row of the
compiled reference, or `Oracle()`).  For a DMVR item it is executed on an edge-padded copy of the prefetched window (`padded_window`: np.pad(..., mode="edge"), then
if_pred_luma / if_filter at the displaced position), i.e. the reference's own filters run on the layout DMVR::xCopyAndPad builds (CommonLib/InterPrediction.cpp:1088-1130)
and DMVR::xFinalPaddedMCForDMVR reads (:1189-1225).

The compiled reference exports no BDOF entry, so these steps are restated in numpy; tests/golden/bdof.npz anchors `bdof_from_frames` to what the reference's own
xApplyBDOF computes on recorded frames (generator: tests/bdof_golden_gen.cpp + tests/bdof_golden_gen.py).
  ring_frame        the one-sample ring of integer samples round the 14-bit block        InterPredInterpolation::xPredInterBlk :822-831, :868-901
  gradients         (s[x+1] >> 6) - (s[x-1] >> 6), same vertically                       gradFilterCore :114-131
  replicate         border replication of the gradients and of the 14-bit block          gradFilterCore :133-154, xApplyBDOF :932-950
  window_sums       the five sums over the 6x6 window of a 4x4 unit                      calcBDOFSumsCore :157-186
  offsets           tmpx, tmpy                                                            xFpBiDirOptFlowCore :642-647 (xRightShiftMSB :602-605)
  bdof_output       ClipPel((int16)((s0 + s1 + b + offset) >> shiftNum))                  addBDOFAvgCore :63-86, xApplyBDOF :952-957
  bdof_units        the cut into min(16, w) x min(16, h) regions                         InterPrediction::xSubPuBDOF :326-357
The ring is a numpy restatement: driving xPredInterBlk through srcPadBuf needs a CodingUnit with slice, picture and coding structure behind it, which is not practical
in a small generator; the interior of the frame is the interpolation the reference executes.
"""
import numpy as np

import pred_ref as PR

EXT_BDOF, EXT_DMVR_PAD = 1, 2
SLACK = 16          # the x86 rows of the reference read whole vectors: room round every array handed to them


def bdof_applies(w, h):
    """the size rule (InterPrediction.cpp:465-490)"""
    return min(w, h) >= 8 and w * h >= 128


def bdof_units(w, h):
    """xSubPuBDOF :326-357: (x0, y0, uw, uh) of the regions predicted on their own"""
    uw, uh = min(w, 16), min(h, 16)
    return [(x0, y0, uw, uh) for y0 in range(0, h, uh) for x0 in range(0, w, uw)]


def padded_window(arr, y, x, w, h, taps, pad):
    """xCopyAndPad :1088-1130: the (w + taps - 1) x (h + taps - 1) window from start - (taps / 2 - 1), replication-padded by `pad` samples, inside SLACK zeros.
    -> (array, row, column) of the START position in it"""
    r = taps // 2 - 1
    win = arr[y - r:y - r + h + taps - 1, x - r:x - r + w + taps - 1]
    assert win.shape == (h + taps - 1, w + taps - 1), "window outside the plane"
    out = np.pad(np.pad(win, pad, mode="edge"), SLACK, mode="constant")
    return np.ascontiguousarray(out), r + pad + SLACK, r + pad + SLACK


def clamped_plane(arr, y, x, w, h, taps):
    """the equivalent statement: the true plane with every coordinate clamped to the prefetched window (used only to show the guard conditions, never as expectation)"""
    r = taps // 2 - 1
    H, W = arr.shape
    yy = np.clip(np.arange(H), y - r, y - r + h + taps - 2)
    xx = np.clip(np.arange(W), x - r, x - r + w + taps - 2)
    return np.ascontiguousarray(arr[np.ix_(yy, xx)])


def source(arr, y, x, w, h, chroma, delta):
    """where list l of an item reads: (array, row, column) of the REFINED integer position (x, y); delta = refined_int - start_int or None"""
    if delta is None or (delta[0] == 0 and delta[1] == 0):
        return arr, y, x
    taps, pad = (4, 1) if chroma else (8, 2)
    assert abs(delta[0]) <= pad and abs(delta[1]) <= pad
    pw, py, px = padded_window(arr, y - delta[1], x - delta[0], w, h, taps, pad)
    return pw, py + delta[1], px + delta[0]


def ring_frame(src, y, x, w, h, xf, yf, bd, interior):
    """xPredInterBlk :868-901: the (h + 2) x (w + 2) frame — the 14-bit block inside a ring of integer samples at the nearest-integer position"""
    hr = max(2, 14 - bd)
    xo, yo = (1 if xf < 8 else 0), (1 if yf < 8 else 0)
    near = src[y - yo:y - yo + h + 2, x - xo:x - xo + w + 2].astype(np.int32)
    frame = ((near << hr) - 8192).astype(np.int16)
    frame[1:-1, 1:-1] = interior
    return frame


def gradients(frame):
    """gradFilterCore :114-131 on the interior, the ring as neighbours; arithmetic shifts on int16"""
    s = frame.astype(np.int32) >> 6
    gx = (s[1:-1, 2:] - s[1:-1, :-2]).astype(np.int16)
    gy = (s[2:, 1:-1] - s[:-2, 1:-1]).astype(np.int16)
    return gx, gy


def replicate(a):
    """columns first, then rows (gradFilterCore :133-154, xApplyBDOF :939-949): the same as edge padding"""
    return np.pad(a, 1, mode="edge")


def window_sums(gx0, gx1, gy0, gy1, s0, s1):
    """calcBDOFSumsCore :157-186 for every 4x4 unit; inputs are the replication-padded (h + 2) x (w + 2) arrays -> five (h / 4, w / 4) arrays"""
    g = (gx0.astype(np.int32) + gx1) >> 1
    v = (gy0.astype(np.int32) + gy1) >> 1
    d = (s1.astype(np.int32) >> 4) - (s0.astype(np.int32) >> 4)
    terms = (np.abs(g), np.abs(v), np.sign(g) * d, np.sign(v) * d, np.sign(v) * g)
    win = np.lib.stride_tricks.sliding_window_view
    return [win(t.astype(np.int64), (6, 6))[::4, ::4].sum(axis=(2, 3)) for t in terms]


def _floor_log2(a):
    return (np.frexp(np.maximum(a, 1).astype(np.float64))[1] - 1).astype(np.int64)          # exact for integers below 2^53


def offsets(sums):
    """xFpBiDirOptFlowCore :642-647"""
    s_agx, s_agy, s_dix, s_diy, s_sign = sums
    tmpx = np.where(s_agx == 0, 0, np.clip((4 * s_dix) >> _floor_log2(s_agx), -15, 15))
    tmpy = np.where(s_agy == 0, 0, np.clip((4 * s_diy - ((s_sign * tmpx) >> 1)) >> _floor_log2(s_agy), -15, 15))
    return tmpx, tmpy


def bdof_output(s0, s1, gx0, gx1, gy0, gy1, tmpx, tmpy, bd):
    """addBDOFAvgCore :63-86 with xApplyBDOF's shiftNum / offset (:952-953); interior arrays, tmpx / tmpy per 4x4 unit.  The int16 cast is kept."""
    sn = 15 - bd
    off = (1 << (sn - 1)) + 2 * 8192
    tx, ty = np.kron(tmpx, np.ones((4, 4), np.int64)), np.kron(tmpy, np.ones((4, 4), np.int64))
    b = tx * (gx0.astype(np.int64) - gx1) + ty * (gy0.astype(np.int64) - gy1)
    v = ((s0.astype(np.int64) + s1 + b + off) >> sn).astype(np.int16)
    return np.clip(v, 0, (1 << bd) - 1).astype(np.int16)


def bdof_from_frames(f0, f1, bd, detail=False):
    """xApplyBDOF :911-958 on the two (h + 2) x (w + 2) frames xPredInterBlk left in m_filteredBlockTmp[2] / [3]"""
    gx0, gy0 = gradients(f0)
    gx1, gy1 = gradients(f1)
    s0, s1 = f0[1:-1, 1:-1], f1[1:-1, 1:-1]
    sums = window_sums(replicate(gx0), replicate(gx1), replicate(gy0), replicate(gy1), replicate(s0), replicate(s1))
    tmpx, tmpy = offsets(sums)
    out = bdof_output(s0, s1, gx0, gx1, gy0, gy1, tmpx, tmpy, bd)
    return (out, tmpx, tmpy, sums) if detail else out


def _list_pred(lib, src, y, x, w, h, xf, yf, rnd, bd, chroma, alt):
    return PR.chroma_pred(lib, src, y, x, w, h, xf, yf, rnd, bd) if chroma else PR.luma_pred(lib, src, y, x, w, h, xf, yf, rnd, bd, alt)


def expected_block_ex(lib, planes, pos, it, ext, bd, clamp=True, bdof=True):
    """as pred_ref.expected_block, with the item's extension record (PRED_EXT_DTYPE or None).  pos[l] = (x, y) of the REFINED integer position.
    clamp=False / bdof=False switch one rule off: the guard conditions of the tests compare against them."""
    w, h, chroma, alt = int(it["width"]), int(it["height"]), int(it["chroma"]), int(it["alt_hpel"])
    flags = int(ext["flags"]) if ext is not None else 0
    used = [l for l in (0, 1) if int(it["ref_plane"][l]) >= 0]
    do_bdof = bool(flags & EXT_BDOF) and bdof
    if flags & EXT_BDOF:
        assert not chroma and len(used) == 2 and bdof_applies(w, h)
    srcs = []
    for l in used:
        delta = (int(ext["pad_dx"][l]), int(ext["pad_dy"][l])) if (flags & EXT_DMVR_PAD) and clamp else None
        srcs.append(source(planes[int(it["ref_plane"][l])], pos[l][1], pos[l][0], w, h, chroma, delta))
    fr = [(int(it["frac"][l][0]), int(it["frac"][l][1])) for l in used]
    if not do_bdof:
        out = [_list_pred(lib, s, y, x, w, h, f[0], f[1], len(used) == 1, bd, chroma, alt) for (s, y, x), f in zip(srcs, fr)]
        return out[0] if len(out) == 1 else PR.bi_average(out[0], out[1], bd)
    res = np.zeros((h, w), np.int16)
    for (x0, y0, uw, uh) in bdof_units(w, h):
        frames = []
        for (s, y, x), f in zip(srcs, fr):
            inner = PR.luma_pred(lib, s, y + y0, x + x0, uw, uh, f[0], f[1], False, bd, alt)
            frames.append(ring_frame(s, y + y0, x + x0, uw, uh, f[0], f[1], bd, inner))
        res[y0:y0 + uh, x0:x0 + uw] = bdof_from_frames(frames[0], frames[1], bd)
    return res
