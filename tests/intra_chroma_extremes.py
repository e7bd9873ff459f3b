"""Items of the intra chroma mode pre-selection at operand limits (tests/test_gpu_intra_chroma_extremes.py), 12 bits throughout: the largest products, shifts and offsets the
CCLM arithmetic can meet.  Every item is checked against the model (tests/intra_chroma_ref.py); the model is anchored to the reference by the fixture's cases of the same kind
(pzero / pmax / ptwo_level / pfull / psteep_pos / psteep_neg / povershoot at 12 bits in tests/intra_chroma_cases.py).
  largest_diff    luma templates at 0 and 4095 on opposite sides ( diff = 4095: floorLog2 11, the longest normalisation ), chroma templates at the opposite extremes
                  ( diffC = +-4095 ), the block's luma full range
  steepest        luma templates that differ by one level at the top of the range ( 4094 / 4095 ), chroma templates 0 / 4095: iShift < 1, a = +-15 with minLuma = 4094 —
                  b = minC -+ ( 15 * 4094 >> 1 ) lies about 30000 outside the clip range on either side, a * luma reaches +-61425, and the block's luma ( 0, 4094, 4095 ) drives
                  the result to both clip bounds
  flat            every luma sample 4095 ( diff == 0 ) with chroma templates at 0 and at 4095: b at both clip bounds
  checker         luma alternating 0 / 4095 sample by sample: every down-sampling filter at its largest sums
Bounds that follow: | a * luma | <= 15 * 4095 and | b | <= 4095 + 15 * 4095 / 2 — far inside 32 bits; the device holds a, b and shift as int32."""
import numpy as np

import intra_chroma_cases as CC
import intra_chroma_ref as CR

BD, VMAX = 12, 4095
SHAPES = [(4, 4), (8, 8), (16, 4), (4, 16), (32, 8), (32, 32)]
KINDS = ("largest_diff", "largest_diff_neg", "steepest_pos", "steepest_neg", "flat_low", "flat_high", "checker")


def fields(kind, rng, w, h):
    wh, ww = CC.window_shape(w, h)
    yy, xx = np.mgrid[0:wh, 0:ww]
    above, left = yy < CC.ORG, xx < CC.ORG          # the rows above / the columns left of the collocated area (the corner counts as above)
    inner = rng.integers(0, 2, (wh, ww)) * VMAX if kind != "checker" else ((xx + yy) & 1) * VMAX
    n, nt = CR.line_len(w, h), 2 * w + 1
    is_top = np.arange(n) < nt
    if kind.startswith("largest_diff"):
        luma = np.where(above, VMAX, np.where(left, 0, inner))
        hi_top = kind == "largest_diff"
        lines = [np.where(is_top == (hi_top ^ bool(c)), VMAX, 0) for c in (0, 1)]
    elif kind.startswith("steepest"):
        luma = np.where(above, VMAX, np.where(left, VMAX - 1, rng.choice([0, VMAX - 1, VMAX], (wh, ww))))
        pos = kind == "steepest_pos"
        lines = [np.where(is_top == (pos ^ bool(c)), VMAX, 0) for c in (0, 1)]
    elif kind.startswith("flat"):
        luma = np.full((wh, ww), VMAX)
        lines = [np.full(n, 0 if (kind == "flat_low") ^ bool(c) else VMAX) for c in (0, 1)]
    else:
        luma = inner
        lines = [rng.integers(0, 2, n) * VMAX for _ in (0, 1)]
    for l in lines:
        l[nt] = l[0]
    org = [rng.integers(0, 2, (h, w)) * VMAX for _ in (0, 1)]
    return luma.astype(np.int16), np.stack(lines).astype(np.int16), np.stack(org).astype(np.int16)


def cases():
    """-> [ Case ]: every kind on every shape with both sides available (so that both templates enter the LM_CHROMA parameters), verCollocatedChroma alternating; MDLM with the
    longest templates; plus each kind on 8x8 with one side only"""
    rng = np.random.default_rng(4095)
    out = []
    both = CR.F_ABOVE | CR.F_LEFT
    for k, kind in enumerate(KINDS):
        for j, (w, h) in enumerate(SHAPES):
            fl = both | (CR.F_VER_COLLOCATED if (k + j) & 1 else 0) | (CR.F_FIRST_ROW if j == 2 else 0)
            pm = 0x70 if w * h <= 256 else 0x10
            out.append(CC.Case("%s_%dx%d" % (kind, w, h), w, h, BD, fl, w, h, CC.cand_list(34), *fields(kind, rng, w, h), mode_mask=0xff, pred_mask=pm))
        for fl in (CR.F_ABOVE, CR.F_LEFT | CR.F_VER_COLLOCATED):
            n_ar, n_lb = CC.full_counts(8, 8, fl)
            out.append(CC.Case("%s_8x8_f%d" % (kind, fl), 8, 8, BD, fl, n_ar, n_lb, CC.cand_list(50), *fields(kind, rng, 8, 8), mode_mask=0x70, pred_mask=0x70))
    return out
