"""numpy / Python-int model of the sub-block transform (SBT) pieces around the TU pipeline, restated from the reference line by line:
  part_sums, estimate, skip_all  InterSearch::xCalcMinDistSbt (EncoderLib/InterSearch.cpp:3272-3464)
  tiling, coded_tile, tr_types   CU::getSbtTuSplit (CommonLib/UnitTools.cpp:3388), PartitionerImpl::getSbtTuTiling (CommonLib/UnitPartitioner.cpp:995-1056), the SBT branch of
                                 TrQuant::xSetTrTypes (CommonLib/TrQuant.cpp:435-466)
  place, sse                     the coded tile's reconstruction inside the CU's block with the other tile zero (tu.noResidual, InterSearch.cpp:3562, :3758-3762)
Distortions are uint64 there: here Python ints reduced modulo 2^64 wherever the reference's arithmetic could wrap.  Pinned to the reference's own results in
tests/golden/sbt.npz by tests/test_sbt_cpu.py (the fixture is written by tests/sbt_golden_gen.py)."""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sbt.npz")
SBT_ITEM_DTYPE = np.dtype([("y_off", "<i4"), ("cb_off", "<i4"), ("cr_off", "<i4"), ("stride_y", "<i4"), ("stride_c", "<i4"), ("width", "<i2"), ("height", "<i2"),
                           ("sbt_allowed", "u1"), ("rsv", "u1", (3,))])      # vvhip_sbt_item (28 bytes)
SBT_PLACE_DTYPE = np.dtype([("y_off", "<i4"), ("cb_off", "<i4"), ("cr_off", "<i4"), ("stride_y", "<i4"), ("stride_c", "<i4"), ("tile_off", "<i4", (3,)), ("stats_idx", "<i4", (3,)),
                            ("width", "<i2"), ("height", "<i2"), ("sbt_allowed", "u1"), ("mode", "u1"), ("rsv", "u1", (2,))])      # vvhip_sbt_place_item (52 bytes)
SBT_VER_HALF, SBT_HOR_HALF, SBT_VER_QUAD, SBT_HOR_QUAD = 1, 2, 3, 4      # SbtIdx (TypeDef.h:266-270) = the bit of sbt_allowed
SBT_VER_H0, SBT_VER_H1, SBT_HOR_H0, SBT_HOR_H1, SBT_VER_Q0, SBT_VER_Q1, SBT_HOR_Q0, SBT_HOR_Q1 = range(8)      # SbtMode (TypeDef.h:284-291)
MAX_DISTORTION = (1 << 64) - 1      # CommonDef.h:202
SBT_NUM_RDO = 2                     # CommonDef.h:491
SCALE_BITS = 15
DCT2, DCT8, DST7 = 0, 1, 2          # TransType
MTS_INTER_MAX_CU_SIZE = 32
M64 = (1 << 64) - 1
SIZES = [(4, 8), (8, 4), (8, 8), (16, 8), (8, 16), (16, 16), (32, 32), (64, 4), (4, 64), (64, 64), (64, 16)]      # the sizes the issue names
ALL_SIZES = [(w, h) for w in (4, 8, 16, 32, 64) for h in (4, 8, 16, 32, 64) if (w, h) != (4, 4)]


def allowed_of(w, h):
    """CU::checkAllowedSbt's size rule (UnitTools.cpp:256-267; MIN_CU_LOG2 = 2: halves from a side of 8, quads from 16)"""
    return ((w >= 8) << SBT_VER_HALF) | ((h >= 8) << SBT_HOR_HALF) | ((w >= 16) << SBT_VER_QUAD) | ((h >= 16) << SBT_HOR_QUAD)


def modes_of(allowed):
    return [m for m in range(8) if (allowed >> (1 + (m >> 1))) & 1]


def subsets_of(allowed):
    """every non-empty subset of the bits of `allowed`"""
    bits = [b for b in range(1, 5) if (allowed >> b) & 1]
    return [sum(1 << b for k, b in enumerate(bits) if (s >> k) & 1) for s in range(1, 1 << len(bits))]


def num_parts(side):
    return 4 if side >= 16 else (1 if side == 4 else 2)      # InterSearch.cpp:3291-3292


def part_sums(y, cb, cr):
    """-> [3][16] Python ints: the unweighted sum of squares of every part per component, [j * 4 + i] in a 4 x 4 frame, zero outside the grid (:3296-3335 without the weight)"""
    h, w = y.shape
    npx, npy = num_parts(w), num_parts(h)
    out = [[0] * 16 for _ in range(3)]
    for c, blk in enumerate((y, cb, cr)):
        b = np.asarray(blk, np.int16).astype(np.int64)
        assert b.shape == ((h, w) if c == 0 else (h // 2, w // 2))
        lx, ly = b.shape[1] // npx, b.shape[0] // npy
        for j in range(npy):
            for i in range(npx):
                p = b[j * ly:(j + 1) * ly, i * lx:(i + 1) * lx]
                out[c][4 * j + i] = int((p * p).sum())
    return out


def weighted(parts, chroma_weight):
    """dist[j][i] of :3329-3333: luma as it is, chroma (Distortion)( uiSum * weight ) — ONE double multiplication, truncated — per component, then added"""
    cw = float(chroma_weight)
    return [(parts[0][k] + int(float(parts[1][k]) * cw) + int(float(parts[2][k]) * cw)) & M64 for k in range(16)]


def estimate(parts, w, h, allowed, chroma_weight):
    """-> (est[9], order[8]) as :3338-3463 leaves m_estMinDistSbt and m_sbtRdoOrder (without fast algorithm 1: see skip_all)"""
    npx, npy = num_parts(w), num_parts(h)
    d = weighted(parts, chroma_weight)
    dist = [[d[4 * j + i] for i in range(4)] for j in range(4)]
    est = [MAX_DISTORTION] * 9
    est[8] = 0
    for j in range(npy):
        for i in range(npx):
            est[8] = (est[8] + dist[j][i]) & M64
    shift = 5
    if (allowed >> SBT_VER_HALF) & 1:
        assert npx >= 2
        resi = no = 0
        for j in range(npy):
            for i in range(npx // 2):
                resi, no = (resi + dist[j][i]) & M64, (no + dist[j][i + npx // 2]) & M64
        est[SBT_VER_H0], est[SBT_VER_H1] = ((resi >> shift) + no) & M64, ((no >> shift) + resi) & M64
    if (allowed >> SBT_HOR_HALF) & 1:
        assert npy >= 2
        resi = no = 0
        for j in range(npy // 2):
            for i in range(npx):
                resi, no = (resi + dist[j][i]) & M64, (no + dist[j + npy // 2][i]) & M64
        est[SBT_HOR_H0], est[SBT_HOR_H1] = ((resi >> shift) + no) & M64, ((no >> shift) + resi) & M64
    if (allowed >> SBT_VER_QUAD) & 1:
        assert npx == 4
        q0 = q1 = 0
        for j in range(npy):
            q0 = (q0 + dist[j][0] + (((dist[j][1] + dist[j][2] + dist[j][3]) << shift) & M64)) & M64
            q1 = (q1 + dist[j][3] + (((dist[j][0] + dist[j][1] + dist[j][2]) << shift) & M64)) & M64
        est[SBT_VER_Q0], est[SBT_VER_Q1] = q0 >> shift, q1 >> shift
    if (allowed >> SBT_HOR_QUAD) & 1:
        assert npy == 4
        q0 = q1 = 0
        for i in range(npx):
            q0 = (q0 + dist[0][i] + (((dist[1][i] + dist[2][i] + dist[3][i]) << shift) & M64)) & M64
            q1 = (q1 + dist[3][i] + (((dist[0][i] + dist[1][i] + dist[2][i]) << shift) & M64)) & M64
        est[SBT_HOR_Q0], est[SBT_HOR_Q1] = q0 >> shift, q1 >> shift
    temp, order, start = est[:8], [255] * 8, 0
    for lo, bits in ((SBT_VER_H0, (SBT_VER_HALF, SBT_HOR_HALF)), (SBT_VER_Q0, (SBT_VER_QUAD, SBT_HOR_QUAD))):
        num = min(sum((allowed >> b) & 1 for b in bits) << 1, SBT_NUM_RDO)
        for i in range(start, start + num):
            best = MAX_DISTORTION
            for n in range(lo, lo + 4):
                if temp[n] < best:
                    best, order[i] = temp[n], n
            temp[order[i]] = MAX_DISTORTION
        start += num
    return est, order


def skip_all(total, dist_scale):
    """fast algorithm 1 (:3353-3359): calcRdCost( 0, total ) < calcRdCost( 12 << SCALE_BITS, 0 ) with RdCost::calcRdCost = distScale * double( dist ) + double( bits ) (RdCost.h:167-170).
    Needs lambda, so it stays with the caller of the device entry: one comparison on est[8]."""
    return float(dist_scale) * float(total) + 0.0 < float(dist_scale) * 0.0 + float(12 << SCALE_BITS)


def tiling(w, h, mode):
    """getSbtTuTiling on one component block: -> [tile 0, tile 1] as (x, y, width, height), with the factors ( dim * f ) >> 2"""
    idx, pos = 1 + (mode >> 1), mode & 1
    out = []
    for i in range(2):
        if idx >= SBT_VER_QUAD:
            own = (i == 0 and pos == 0) or (i == 1 and pos == 1)
            if idx == SBT_HOR_QUAD:
                wf, xf, hf, yf = 4, 0, (1 if own else 3), (0 if i == 0 else (1 if pos == 0 else 3))
            else:
                wf, xf, hf, yf = (1 if own else 3), (0 if i == 0 else (1 if pos == 0 else 3)), 4, 0
        elif idx == SBT_HOR_HALF:
            wf, xf, hf, yf = 4, 0, 2, (0 if i == 0 else 2)
        else:
            wf, xf, hf, yf = 2, (0 if i == 0 else 2), 4, 0
        out.append(((w * xf) >> 2, (h * yf) >> 2, (w * wf) >> 2, (h * hf) >> 2))
    return out


def coded_tile(w, h, mode):
    """tile 0 is coded for position 0 and tile 1 for position 1 (the other one has tu.noResidual)"""
    return tiling(w, h, mode)[mode & 1]


def tr_types(w, h, mode):
    """(trHor, trVer) of the coded LUMA tile of a w x h CU (TrQuant.cpp:435-466); chroma is DCT-2 both ways"""
    _, _, tw, th = coded_tile(w, h, mode)
    idx, pos = 1 + (mode >> 1), mode & 1
    if idx in (SBT_VER_HALF, SBT_VER_QUAD):
        assert tw <= MTS_INTER_MAX_CU_SIZE
        if th > MTS_INTER_MAX_CU_SIZE:
            return DCT2, DCT2
        return (DCT8, DST7) if pos == 0 else (DST7, DST7)
    assert th <= MTS_INTER_MAX_CU_SIZE
    if tw > MTS_INTER_MAX_CU_SIZE:
        return DCT2, DCT2
    return (DST7, DCT8) if pos == 0 else (DST7, DST7)


def place(tile_rec, w, h, mode):
    """the w x h component block of the CU's reconstructed residual: the coded tile's reconstruction (None: no levels / no coefficients) in place, zero elsewhere"""
    out = np.zeros((h, w), np.int16)
    if tile_rec is not None:
        x, y, tw, th = coded_tile(w, h, mode)
        out[y:y + th, x:x + tw] = np.asarray(tile_rec, np.int16).reshape(th, tw)
    return out


def sse(a, b):
    d = np.asarray(a, np.int64) - np.asarray(b, np.int64)
    return int((d * d).sum())


def golden():
    """-> dict: cus = list of dicts (w, h, allowed, cw, dist_scale, kind, y, cb, cr, est [9] ints, order [8] ints, skip, parts [3][16] ints), tilings = list of (w, h, mode,
    rects int32 [2][3][4], (trHor, trVer)), placed = list of dicts (w, h, mode, org, tile, sse)"""
    z = np.load(GOLDEN)
    cus = []
    for i in range(int(z["n_cus"])):
        k = "u%03d_" % i
        w, h, allowed, kind = (int(v) for v in z[k + "hdr"])
        cus.append(dict(w=w, h=h, allowed=allowed, kind=kind, cw=float(z[k + "wt"][0]), dist_scale=float(z[k + "wt"][1]), y=z[k + "y"], cb=z[k + "cb"], cr=z[k + "cr"],
                        est=[int(v) for v in z[k + "est"]], order=[int(v) for v in z[k + "order"]], skip=bool(z[k + "skip"]), parts=[[int(v) for v in row] for row in z[k + "parts"]]))
    til = [(int(r[0]), int(r[1]), int(r[2]), z["til_rects"][n], (int(z["til_types"][n][0]), int(z["til_types"][n][1]))) for n, r in enumerate(z["til_hdr"])]
    placed = []
    for i in range(int(z["n_placed"])):
        k = "p%03d_" % i
        w, h, mode = (int(v) for v in z[k + "hdr"])
        placed.append(dict(w=w, h=h, mode=mode, org=z[k + "org"], tile=z[k + "tile"], sse=int(z[k + "sse"])))
    return dict(cus=cus, tilings=til, placed=placed)
