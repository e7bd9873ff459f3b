"""Expected values for the inter-prediction list entry (vvhip_pred_inter_batch / vvhip_interp_chroma_batch): helpers shared by the CPU and GPU tests.

Every interpolation pass is EXECUTED from the library handed in (`RefLib(0)` scalar row, `RefLib(1)` x86 row of the compiled reference, or `Oracle()`,
the C restatement), called the way InterPredInterpolation::xPredInterBlk calls it (CommonLib/InterPrediction.cpp:838-866).  Two steps are restated here in
numpy because the compiled reference exports no entry for them — `bi_average` (AreaBuf<Pel>::addAvg, CommonLib/Buffer.cpp:549-575, core :129-141) and
`residual` (org - pred, the subtraction in front of InterSearch::xEstimateInterResidualQT) — one line each.

For chroma blocks 4x4 / 8xH / 16xH with two non-zero fractions xPredInterBlk takes the fused table entries m_filter4x4 / m_filter8xH / m_filter16xH [1]
(filterWxH_N4, InterpolationFilter.cpp:214-227); the compiled reference exports them for luma only (if_pred_luma), so chroma is composed from the two
table passes here for every width — the fused entries are the same two passes in one function.
"""
import numpy as np

LUMA_SIZES = [(w, h) for w in (4, 8, 16, 32, 64, 128) for h in (4, 8, 16, 32, 64, 128)]
CHROMA_SIZES = [(w, h) for w in (2, 4, 8, 16, 32, 64) for h in (2, 4, 8, 16, 32, 64)]


def chroma_pred(lib, arr, y, x, w, h, xf, yf, rnd, bd):
    """4:2:0 chroma block at integer position (x, y) of `arr`, fractions in 1/32 sample (xPredInterBlk :838-866 with vFilterSize = NTAPS_CHROMA)"""
    ch, cv = lib.if_coeff(2, xf)[1], lib.if_coeff(2, yf)[1]
    if xf and yf:
        tmp = lib.if_filter(4, 0, 1, 0, bd, (arr, y - 1, x), w, h + 3, ch)          # h + 3 rows starting one row above the block
        pad = np.zeros((h + 3 + 8, w + 32), np.int16)                                 # slack: the x86 rows read whole vectors
        pad[4:4 + h + 3, 8:8 + w] = tmp
        return lib.if_filter(4, 1, 0, int(rnd), bd, (pad, 4 + 1, 8), w, h, cv)      # from the second row of the intermediate
    if xf:
        return lib.if_filter(4, 0, 1, int(rnd), bd, (arr, y, x), w, h, ch)
    if yf:
        return lib.if_filter(4, 1, 1, int(rnd), bd, (arr, y, x), w, h, cv)
    return lib.if_copy(1, int(rnd), bd, (arr, y, x), w, h)


def luma_pred(lib, arr, y, x, w, h, xf, yf, rnd, bd, alt):
    return lib.if_pred_luma((arr, y, x), w, h, xf, yf, bool(rnd), bd, bool(alt))


def bi_average(a, b, bd):
    """AreaBuf<Pel>::addAvg (Buffer.cpp:549-575; core :129-141): ClipPel( ( a + b + offset ) >> shiftNum )"""
    shift = max(2, 14 - bd) + 1
    return np.clip((a.astype(np.int32) + b.astype(np.int32) + (1 << (shift - 1)) + 2 * 8192) >> shift, 0, (1 << bd) - 1).astype(np.int16)


def residual(org_block, pred_block):
    return (org_block.astype(np.int32) - pred_block.astype(np.int32)).astype(np.int16)


def expected_block(lib, planes, pos, it, bd):
    """planes[k]: 2-D int16 array (margins included); pos[l] = (x, y) of the item's integer position in planes[it.ref_plane[l]]; it: a PRED_ITEM_DTYPE record"""
    w, h, chroma, alt = int(it["width"]), int(it["height"]), int(it["chroma"]), int(it["alt_hpel"])
    used = [l for l in (0, 1) if int(it["ref_plane"][l]) >= 0]
    out = []
    for l in used:
        arr, (x, y) = planes[int(it["ref_plane"][l])], pos[l]
        xf, yf = int(it["frac"][l][0]), int(it["frac"][l][1])
        rnd = len(used) == 1
        out.append(chroma_pred(lib, arr, y, x, w, h, xf, yf, rnd, bd) if chroma else luma_pred(lib, arr, y, x, w, h, xf, yf, rnd, bd, alt))
    return out[0] if len(out) == 1 else bi_average(out[0], out[1], bd)


def kernel_form(taps_h, lo_h, taps_v, lo_v, arr, y, x, w, h, rnd, bd):
    """numpy model of the ARITHMETIC FORM the device kernel uses for every fraction pair: always horizontal (isFirst, !isLast) then vertical (!isFirst), a zero
    fraction being the one-tap set { 64 } — to be compared with the reference's single-pass and copy forms on the CPU"""
    hr = max(2, 14 - bd)
    s1 = 6 - hr
    a = arr.astype(np.int64)
    rows = h + len(taps_v) - 1
    tmp = np.zeros((rows, w), np.int64)
    for k, c in enumerate(taps_h):
        tmp += c * a[y - lo_v:y - lo_v + rows, x - lo_h + k:x - lo_h + k + w]
    tmp = ((tmp - (8192 << s1)) >> s1).astype(np.int16).astype(np.int64)
    acc = np.zeros((h, w), np.int64)
    for k, c in enumerate(taps_v):
        acc += c * tmp[k:k + h]
    if rnd:
        s2 = 6 + hr
        return np.clip(((acc + (1 << (s2 - 1)) + (8192 << 6)) >> s2).astype(np.int16), 0, (1 << bd) - 1).astype(np.int16)
    return (acc >> 6).astype(np.int16)


def shelf_pack(sizes, plane_w):
    """non-overlapping positions (x, y) for blocks of the given (w, h) in a plane plane_w wide; returns (positions, rows used)"""
    out, x, y, shelf = [], 0, 0, 0
    for (w, h) in sizes:
        if x + w > plane_w:
            x, y, shelf = 0, y + shelf, 0
        out.append((x, y))
        x += w
        shelf = max(shelf, h)
    return out, y + shelf
