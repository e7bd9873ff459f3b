"""Expected values for the blend forms of the prediction list (vvhip_pred_inter_batch_blend: BCW weights, GEO partitions): a numpy model shared by the CPU and GPU tests.

Both tools are  ClipPel( ( w0 * s0 + ( 8 - w0 ) * s1 + offset ) >> shift )  on the two 14-bit intermediates, shift = max( 2, 14 - bitDepth ) + 3,
offset = ( 1 << ( shift - 1 ) ) + ( 8192 << 3 ):
  BCW   AreaBuf<Pel>::addWeightedAvg (CommonLib/Buffer.cpp:509-546, core :143-156), getBcwWeight (Rom.cpp:1150-1163): w1 = BCW_W1[bcw_idx], w0 = 8 - w1
  GEO   InterpolationFilter::xWeightedGeoBlk (CommonLib/InterpolationFilter.cpp:1005-1064): w0 read from one of six 112 x 112 masks (Rom.cpp:1304-1382)
The GEO weights are modelled the way the reference keeps them — the six masks are built once, and a block is a strided, possibly mirrored, read out of its mask — and NOT
as the clamped line the library evaluates per sample: the two forms meet in tests/test_blend_cpu.py, both pinned to what the reference function itself returned
(tests/golden/blend.npz, made by tests/blend_golden_gen.cpp).  The interpolation of each hypothesis is executed from the library handed in, as in tests/pred_ref.py."""
import numpy as np

import pred_ref as PR

BLEND_DEFAULT, BLEND_BCW, BLEND_GEO = 0, 1, 2
PRED_BLEND_DTYPE = np.dtype([("mode", "u1"), ("param", "u1"), ("rsv", "u1", (2,))])
BCW_W1 = (-2, 3, 4, 5, 10)
GEO_SIZES = [(w, h) for w in (8, 16, 32, 64) for h in (8, 16, 32, 64)]          # CU luma sizes xWeightedGeoBlk is defined for
MASK = 112

ANGLE2MASK = (0, -1, 1, 2, 3, 4, -1, -1, 5, -1, -1, 4, 3, 2, 1, -1, 0, -1, 1, 2, 3, 4, -1, -1, 5, -1, -1, 4, 3, 2, 1, -1)
DIS = (8, 8, 8, 8, 4, 4, 2, 1, 0, -1, -2, -4, -4, -8, -8, -8, -8, -8, -8, -8, -4, -4, -2, -1, 0, 1, 2, 4, 4, 8, 8, 8)
ANGLE2MIRROR = (0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 2, 2, 2, 2)


def _geo_params():
    """g_GeoParams: ( angleIdx, distanceIdx ) of the 64 split directions"""
    out = []
    for a in range(32):
        for d in range(4):
            if (d == 0 and a >= 16) or (d in (0, 2) and ANGLE2MASK[a] in (0, 5)) or ANGLE2MASK[a] == -1:
                continue
            out.append((a, d))
    assert len(out) == 64
    return out


def _masks():
    """g_globalGeoWeights: six 112 x 112 masks, one per angle 0, 2, 3, 4, 5, 8"""
    m = np.zeros((6, MASK, MASK), np.int8)
    pos = 2 * (np.arange(MASK) + 8) + 1          # sample positions in half samples of the 128-wide frame the masks are cut from
    for a in range(9):
        if ANGLE2MASK[a] < 0:
            continue
        dx, dy = DIS[a], DIS[(a + 8) % 32]
        rho = (dx + dy) * 128
        idx = pos[None, :] * dx + pos[:, None] * dy - rho
        m[ANGLE2MASK[a]] = np.clip((32 + idx + 4) >> 3, 0, 8)
    return m


GEO_PARAMS = _geo_params()
GEO_MASKS = _masks()


def geo_offset(split_dir, w, h):
    """g_weightOffset of a w x h (luma) CU"""
    angle, dist = GEO_PARAMS[split_dir]
    ox, oy = (MASK - w) >> 1, (MASK - h) >> 1
    if dist > 0:
        if angle % 16 == 8 or (angle % 16 != 0 and h >= w):
            oy += (dist * h) >> 3 if angle < 16 else -((dist * h) >> 3)
        else:
            ox += (dist * w) >> 3 if angle < 16 else -((dist * w) >> 3)
    return ox, oy


def geo_weights(split_dir, w, h, chroma=0):
    """w0 of one component block of a w x h (luma) CU: int8 [h >> chroma, w >> chroma], values 0..8"""
    angle, _ = GEO_PARAMS[split_dir]
    ox, oy = geo_offset(split_dir, w, h)
    step = 1 << chroma
    xs, ys = ox + np.arange(0, w, step), oy + np.arange(0, h, step)
    if ANGLE2MIRROR[angle] == 1:
        xs = MASK - 1 - xs
    elif ANGLE2MIRROR[angle] == 2:
        ys = MASK - 1 - ys
    assert xs.min() >= 0 and xs.max() < MASK and ys.min() >= 0 and ys.max() < MASK
    return GEO_MASKS[ANGLE2MASK[angle]][np.ix_(ys, xs)].copy()


def weights_of(shape, mode, param, chroma=0):
    """w0 per sample of a component block of the given ( h, w )"""
    h, w = shape
    if mode == BLEND_BCW:
        return np.full((h, w), 8 - BCW_W1[param], np.int32)
    assert mode == BLEND_GEO
    return geo_weights(param, w << chroma, h << chroma, chroma).astype(np.int32)


def blend(s0, s1, mode, param, bit_depth, chroma=0):
    """the two 14-bit blocks -> final samples"""
    w0 = weights_of(s0.shape, mode, param, chroma)
    shift = max(2, 14 - bit_depth) + 3
    v = (w0 * s0.astype(np.int32) + (8 - w0) * s1.astype(np.int32) + (1 << (shift - 1)) + (8192 << 3)) >> shift
    return np.clip(v, 0, (1 << bit_depth) - 1).astype(np.int16)


def hypothesis(lib, planes, pos, it, l, bd, rnd):
    """list l of the item interpolated from the library: rnd False = the 14-bit block, True = final samples (the uni-prediction of that hypothesis)"""
    w, h = int(it["width"]), int(it["height"])
    arr, (x, y) = planes[int(it["ref_plane"][l])], pos[l]
    xf, yf = int(it["frac"][l][0]), int(it["frac"][l][1])
    if int(it["chroma"]):
        return PR.chroma_pred(lib, arr, y, x, w, h, xf, yf, rnd, bd)
    return PR.luma_pred(lib, arr, y, x, w, h, xf, yf, rnd, bd, int(it["alt_hpel"]))


def expected_block_blend(lib, planes, pos, it, bl, bd):
    """planes / pos / it as pred_ref.expected_block; bl: a PRED_BLEND_DTYPE record"""
    mode = int(bl["mode"])
    if mode == BLEND_DEFAULT:
        return PR.expected_block(lib, planes, pos, it, bd)
    s0, s1 = (hypothesis(lib, planes, pos, it, l, bd, False) for l in (0, 1))
    return blend(s0, s1, mode, int(bl["param"]), bd, int(it["chroma"]))
