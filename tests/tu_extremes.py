"""Deterministic extreme inputs of the TU pipeline (transforms, quantiser, fused TU RDO), shared by the CPU tier
(tests/test_oracle_tu_extremes.py: oracle against the compiled reference) and the GPU tier (tests/test_gpu_tu_extremes.py: every
kernel form against the oracle).

Random inputs reach about sqrt(N) of a sum's bound; these reach the bound itself: basis-aligned sign patterns at the bit-depth maximum
drive the forward first stage to within 0.4 % of 16 bits, sign-aligned coefficient blocks overflow the inverse first stage (its clip is
the result), and quantiser inputs sit exactly on the level, need-RDOQ and coefficient-group thresholds.  Basis rows are read from the
integer matrices (a ``tr_matrix(tr_type, log2n)`` callable: Oracle.tr_matrix), never restated.  The int64 models below compute the
intermediates the guards check, so a test shows that a limit was reached and not only that two outputs matched.
"""
import numpy as np

DCT2, DCT8, DST7 = 0, 1, 2
SIZES = (2, 4, 8, 16, 32, 64)
BYTE_EDGES = (127, -127, 128, -128, 255, -255, 256, -256, -32768, 32767)      # the int8 byte-split MFMA operands' edges


def log2(n):
    return int(n).bit_length() - 1


def qp_max(bd):
    """largest QP' (QpParam::Qp incl. qpBdOffset = 6 (bd - 8)) of a bd-bit encode"""
    return 63 + 6 * (bd - 8)


def tr_types(w, h):
    """the legal (tr_hor, tr_ver) pairs of a w x h TU: DCT-2 everywhere, DST-7 / DCT-8 on 4..32-point sides"""
    yield DCT2, DCT2
    if 4 <= w <= 32 and 4 <= h <= 32:
        for th in (DST7, DCT8):
            for tv in (DST7, DCT8):
                yield th, tv
    if 4 <= w <= 32:
        yield DST7, DCT2
    if 4 <= h <= 32:
        yield DCT2, DST7


def skips(w, h, th, tv):
    """zero-out: 64-point beyond 32, MTS 32-point beyond 16 (TrQuant.cpp:496-497)"""
    sw = 16 if (th != DCT2 and w == 32) else max(0, w - 32)
    sh = 16 if (tv != DCT2 and h == 32) else max(0, h - 32)
    return sw, sh


def zero_out(coef, th, tv):
    h, w = coef.shape[-2:]
    sw, sh = skips(w, h, th, tv)
    coef = coef.copy()
    if sw:
        coef[..., :, w - sw:] = 0
    if sh:
        coef[..., h - sh:, :] = 0
    return coef


def _sgn(v):
    return np.where(np.asarray(v) < 0, -1, 1).astype(np.int64)


# ---- forward ------------------------------------------------------------------------------------------------------------------
def fwd_residuals(tr_matrix, w, h, th, tv, bd):
    """(k, h, w) int16 residual blocks with |r| <= 2^bd - 1: +-A sign(b_v[k] x b_h[l]) for (k, l) = (0,0), (0,1), (1,0), last, middle;
    constants, checkerboard, row and column stripes at +-A; single +-A impulses in each corner"""
    A = (1 << bd) - 1
    Th, Tv = tr_matrix(th, log2(w)).astype(np.int64), tr_matrix(tv, log2(h)).astype(np.int64)
    out = []
    for kv, kh in {(0, 0), (0, min(1, w - 1)), (min(1, h - 1), 0), (h - 1, w - 1), (h // 2, w // 2)}:
        b = np.outer(_sgn(Tv[kv]), _sgn(Th[kh]))
        out += [A * b, -A * b]
    yy, xx = np.mgrid[0:h, 0:w]
    for pat in (np.ones((h, w), np.int64), np.where((yy + xx) & 1, -1, 1), np.where(yy & 1, -1, 1), np.where(xx & 1, -1, 1)):
        out += [A * pat, -A * pat]
    for y, x in ((0, 0), (0, w - 1), (h - 1, 0), (h - 1, w - 1)):
        for s in (A, -A):
            z = np.zeros((h, w), np.int64)
            z[y, x] = s
            out.append(z)
    return np.stack(out).astype(np.int16)


def _imatmul(a, b):
    """exact integer matrix product through float64 (BLAS): every sum here stays far below 2^53"""
    return np.rint(np.asarray(a, np.float64) @ np.asarray(b, np.float64)).astype(np.int64)


def fwd_stage1(resi, Th, shift1):
    """the forward first stage before any saturation, int64: tmp[.., y, k] = (sum_x r[y][x] Th[k][x] + rnd) >> shift1"""
    rnd = (1 << (shift1 - 1)) if shift1 > 0 else 0
    return (_imatmul(resi, np.asarray(Th).T) + rnd) >> shift1


def fwd_shift1(w, bd):
    return log2(w) + bd - 9


# ---- inverse ------------------------------------------------------------------------------------------------------------------
def inv_coefs(tr_matrix, w, h, th, tv, seed=0):
    """(k, h, w) int32 coefficient blocks inside the zero-out rules: all 32767 / all -32768; sign patterns that maximise one first-stage
    output (the sign of the basis column, for the first / middle / last sample, also joined with a row pattern); the byte-split edges"""
    Th, Tv = tr_matrix(th, log2(w)).astype(np.int64), tr_matrix(tv, log2(h)).astype(np.int64)
    rng = np.random.default_rng(seed)
    out = [np.full((h, w), 32767, np.int64), np.full((h, w), -32768, np.int64)]
    for j in sorted({0, h // 2, h - 1}):
        col = _sgn(Tv[:, j])                                       # sign of basis column j: every coefficient column adds up at output j
        out += [32767 * np.repeat(col[:, None], w, 1), -32767 * np.repeat(col[:, None], w, 1) - (col[:, None] > 0)]
        for i in sorted({0, w - 1}):
            out.append(np.where(np.outer(col, _sgn(Th[:, i])) > 0, 32767, -32768))
    for v in BYTE_EDGES:
        out.append(np.full((h, w), v, np.int64))
    for _ in range(2):
        out.append(rng.choice(np.array(BYTE_EDGES, np.int64), size=(h, w)))
    return zero_out(np.stack(out), th, tv).astype(np.int32)


def inv_stage1(coef, Tv):
    """the inverse first stage before its clip, int64: t1[.., j, i] = (sum_k coef[k][i] Tv[k][j] + 64) >> 7"""
    return (_imatmul(np.asarray(Tv).T, coef) + 64) >> 7


# ---- quantiser ----------------------------------------------------------------------------------------------------------------
def ceil_div(a, b):
    return -((-a) // b)


def level_edge(k, scale, q_bits, add):
    """smallest |c| whose level (|c| scale + add) >> qBits is k"""
    return ceil_div((k << q_bits) - add, scale)


def cg_thres(scale, q_bits, thr):
    """QuantCore's coefficient-group threshold useThres (Quant.cpp:173-180, int32 as the reference computes it)"""
    t = (thr << (q_bits - 1)) if q_bits else ((thr >> 1) << q_bits)
    t = ((t + (1 << 31)) % (1 << 32)) - (1 << 31)
    return int(np.trunc(t / (scale << 2)))


def quant_blocks(orc, w, h, bd, qp, irap, thr, seed=0):
    """(k, h, w) int32 coefficient blocks for one (size, QP', irap, thr): every coefficient on a level edge (k = 1, 2 and the k that clips
    at 32767, where |c| fits 31 bits) or one below it, both signs; a block on the coefficient-group threshold (one coefficient of an
    inner group at useThres / useThres + 1 behind a small top group)"""
    rng = np.random.default_rng(seed + 977 * qp + 131 * w + 17 * h + 5 * irap + thr)
    scale, q_bits, add = orc.quant_params(w, h, bd, qp, irap)
    vals = []
    for k in (1, 2, 32768):
        e = level_edge(k, scale, q_bits, add)
        if e < (1 << 30):
            vals += [e, e - 1, -e, -(e - 1)]
    vals = np.array(vals, np.int64)
    cw, ch = min(w, 32), min(h, 32)
    out = []
    for _ in range(2):
        b = np.zeros((h, w), np.int64)
        b[:ch, :cw] = rng.choice(vals, size=(ch, cw))
        out.append(b)
    out.append(cg_block(orc, w, h, scale, q_bits, thr, rng, 0))
    out.append(cg_block(orc, w, h, scale, q_bits, thr, rng, 1))
    return np.stack(out).astype(np.int32)


def cg_block(orc, w, h, scale, q_bits, thr, rng, above):
    """a coefficient of group g1 >= 1 at useThres + above, a small non-zero one in a later group g2, the DC non-zero"""
    b = np.zeros((h, w), np.int64)
    num = min(w, 32) * min(h, 32)
    scan = orc.scan_order(log2(w), log2(h))[:num]
    ut = max(cg_thres(scale, q_bits, thr), 0)
    b.flat[scan[0]] = ut + 7
    if num >= 48:
        g1 = int(rng.integers(1, num // 16 - 1))
        g2 = int(rng.integers(g1 + 1, num // 16))
        b.flat[scan[16 * g1 + int(rng.integers(0, 16))]] = (ut + above) * (1 if rng.integers(0, 2) else -1) or 1
        b.flat[scan[16 * g2 + int(rng.integers(0, 16))]] = max(1, min(ut, 3)) * (1 if rng.integers(0, 2) else -1)
    return b


def need_rdoq_blocks(orc, w, h, bd, qp, luma, seed=0):
    """(k, h, w) int32 blocks on the need-RDOQ edge (offset 171 luma / 256 chroma, Quant.cpp:874): all of the efficient area one below
    the edge (no RDOQ), the same with one coefficient on it, one lone coefficient on the edge / below it at a random position"""
    rng = np.random.default_rng(seed + 31 * qp + 7 * w + h + luma)
    scale, q_bits, off, num = orc.need_rdoq_params(w, h, bd, qp, luma)
    e = level_edge(1, scale, q_bits, off)
    out = []
    b = np.zeros((h, w), np.int64)
    b.flat[:num] = (e - 1) * np.where(rng.integers(0, 2, num) == 1, 1, -1)
    out.append(b.copy())
    b.flat[int(rng.integers(0, num))] = -e
    out.append(b)
    for v in (e, e - 1):
        b = np.zeros((h, w), np.int64)
        b.flat[int(rng.integers(0, num))] = v
        out.append(b)
    return np.stack(out).astype(np.int32)


def dequant_levels(h, w, seed=0):
    """(k, h, w) int16 levels around DeQuantCore's input clamp (inputMaximum 2^14 - 1 or 2^15 - 1, Quant.cpp:606) and the 16-bit edges"""
    rng = np.random.default_rng(seed + 7 * w + h)
    edges = np.array([16383, 16384, -16384, -16385, 32767, -32768, 8191, -8192, 1, -1, 0], np.int64)
    return np.stack([np.full((h, w), 32767), np.full((h, w), -32768), rng.choice(edges, size=(h, w)), rng.choice(edges, size=(h, w))]).astype(np.int16)


def fwd_model(resi, Th, Tv, bd):
    """xT in int64 (conforming residuals: the first stage never saturates), zero-out not applied: (.., h, w) coefficients"""
    h, w = np.asarray(resi).shape[-2:]
    t = fwd_stage1(resi, Th, fwd_shift1(w, bd))                       # [.., y, k]
    s2 = log2(h) + 6
    return (_imatmul(Tv, t) + (1 << (s2 - 1))) >> s2


def edge_residuals(orc, w, h, th, tv, bd, targets, n, seed=0):
    """up to n residual blocks (|r| <= 2^bd - 1) whose DC coefficient is exactly one of `targets` (level / need-RDOQ edges of the fused
    kernel): a constant plus a few +-1 / +-7 tweaks, found by search on the int64 forward model"""
    rng = np.random.default_rng(seed + 101 * w + 11 * h + 3 * th + tv + bd)
    A = (1 << bd) - 1
    Th, Tv = orc.tr_matrix(th, log2(w)).astype(np.int64), orc.tr_matrix(tv, log2(h)).astype(np.int64)
    dc_gain = int(fwd_model(np.ones((h, w), np.int64), Th, Tv, bd)[0, 0])
    out = []
    for t in targets:
        base = int(np.clip(round(t / max(dc_gain, 1)), -A + 8, A - 8))
        cand = np.full((96, h, w), base, np.int64)
        for c in range(1, 96):
            k = int(rng.integers(1, 5))
            idx = rng.integers(0, h * w, size=k)
            cand[c].flat[idx] += rng.choice([-7, -1, 1, 7], size=k)
        dc = fwd_model(cand, Th, Tv, bd)[:, 0, 0]
        hit = np.nonzero(dc == t)[0]
        if hit.size:
            out.append(cand[hit[0]])
        if len(out) >= n:
            break
    return np.array(out, np.int16).reshape(-1, h, w)
