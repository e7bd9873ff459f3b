"""Expected values for the CIIP form of the prediction list (vvhip_pred_inter_batch_ciip: planar intra part and weighting): a numpy model shared by the CPU and GPU tests.

The four steps of the reference on one component block, from its reference line `line` = top[0 .. w + 2] followed by left[0 .. h + 2] (unfiltered, top[0] == left[0]):
  smoothing   IntraPrediction::xFilterReferenceSamples (CommonLib/IntraPrediction.cpp:994-1030), luma only: f[i] = ( u[i-1] + 2 u[i] + u[i+1] + 2 ) >> 2 for i >= 1
  planar      xPredIntraPlanar_Core (:79-135)
  PDPC        IntraPredSampleFilter_Core (:137-157), where min( w, h ) >= 4
  weighting   weightCiipCore (CommonLib/Buffer.cpp:60-81): ( wI * intra + ( 4 - wI ) * inter + 2 ) >> 2, wI = num_intra + 1, not clipped
Planar is modelled the way the reference runs it — the two running sums horPred and topRow[x], accumulated along the row and down the column — and NOT as the closed
form the kernel evaluates per sample: the two meet in the tests, both pinned to what the reference's own functions returned (tests/golden/ciip.npz, made by
tests/ciip_golden_gen.cpp).  The inter part of an item is executed from the library handed in, as in tests/pred_ref.py and tests/blend_ref.py."""
import os

import numpy as np

import blend_ref as BL
import pred_ref as PR

CIIP_OFF, CIIP_ON = 0, 1
PRED_CIIP_DTYPE = np.dtype([("ref_off", "<i4"), ("mode", "u1"), ("num_intra", "u1"), ("rsv", "u1", (2,))])
LUMA_SIZES = [(w, h) for w in (4, 8, 16, 32, 64) for h in (4, 8, 16, 32, 64) if w * h >= 64]          # component blocks of a CIIP CU (EncCu.cpp:1926)
CHROMA_SIZES = [(w, h) for w in (4, 8, 16, 32) for h in (2, 4, 8, 16, 32) if w * h >= 16]            # 4:2:0, chromaSize().width > 2 (EncCu.cpp:2213-2219)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ciip.npz")


def line_len(w, h):
    return w + h + 6


def split_line(line, w, h):
    line = np.asarray(line, np.int32)
    assert line.size == line_len(w, h)
    return line[:w + 3], line[w + 3:]


def smooth(row):
    """samples 1 .. len - 2 of one row after the [1 2 1] filter; sample 0 and the last one are never read by planar or PDPC (kept as they are)"""
    out = row.copy()
    out[1:-1] = (row[:-2] + 2 * row[1:-1] + row[2:] + 2) >> 2
    return out


def planar_intra(line, w, h, chroma, smoothing=True, pdpc=True):
    """the intra part of a CIIP block: int16 [h, w].  smoothing / pdpc = False drop the step (the sensitivity tests)"""
    top, left = split_line(line, w, h)
    if not chroma and smoothing:
        top, left = smooth(top), smooth(left)
    l2w, l2h = w.bit_length() - 1, h.bit_length() - 1
    t, l = top[1:w + 2], left[1:h + 2]                     # topRow[0 .. w], leftColumn[0 .. h]
    bottom_row, right_col = l[h] - t[:w], t[w] - l[:h]
    hor = (l[:h, None] << l2w) + np.cumsum(np.broadcast_to(right_col[:, None], (h, w)), axis=1)      # horPred += rightColumn[y] along the row
    ver = (t[None, :w] << l2h) + np.cumsum(np.broadcast_to(bottom_row[None, :], (h, w)), axis=0)     # topRow[x] += bottomRow[x] down the column
    pred = ((hor << l2h) + (ver << l2w) + (1 << (l2w + l2h))) >> (1 + l2w + l2h)
    if pdpc and min(w, h) >= 4:
        scale = (l2w + l2h - 2) >> 2
        wt = 32 >> np.minimum(31, (2 * np.arange(h)) >> scale)
        wl = 32 >> np.minimum(31, (2 * np.arange(w)) >> scale)
        pred = pred + ((wl[None, :] * (l[:h, None] - pred) + wt[:, None] * (t[None, :w] - pred) + 32) >> 6)
    return pred.astype(np.int16)


def weight(inter, intra, num_intra):
    wi = int(num_intra) + 1
    return ((wi * intra.astype(np.int32) + (4 - wi) * inter.astype(np.int32) + 2) >> 2).astype(np.int16)


def ciip(inter, line, chroma, num_intra, smoothing=True, pdpc=True):
    h, w = inter.shape
    return weight(inter, planar_intra(line, w, h, chroma, smoothing, pdpc), num_intra)


def line_at(pic, x, y, w, h):
    """the reference line of the w x h block at ( x, y ) of a picture whose neighbours are all available: top = row y - 1 from x - 1, left = column x - 1 from y - 1"""
    return np.concatenate([pic[y - 1, x - 1:x + w + 2], pic[y - 1:y + h + 2, x - 1]]).astype(np.int16)


def expected_block_ciip(lib, planes, pos, it, bl, ci, lines, bd):
    """planes / pos / it / bl as blend_ref.expected_block_blend (bl may be None); ci: a PRED_CIIP_DTYPE record; lines: the int16 array ref_off points into"""
    inter = BL.expected_block_blend(lib, planes, pos, it, bl, bd) if bl is not None else PR.expected_block(lib, planes, pos, it, bd)
    if int(ci["mode"]) == CIIP_OFF:
        return inter
    w, h, o = int(it["width"]), int(it["height"]), int(ci["ref_off"])
    return ciip(inter, lines[o:o + line_len(w, h)], int(it["chroma"]), int(ci["num_intra"]))


def golden_cases():
    """the fixture as a list of dicts: bd, w, h, chroma, num_intra, line, inter, intra, result"""
    z = np.load(GOLDEN)
    out = []
    for i in range(int(z["n"])):
        bd, w, h, chroma, ni = (int(v) for v in z["c%03d_hdr" % i])
        out.append(dict(bd=bd, w=w, h=h, chroma=chroma, num_intra=ni, line=z["c%03d_line" % i], inter=z["c%03d_inter" % i], intra=z["c%03d_intra" % i],
                        result=z["c%03d_result" % i]))
    return out
