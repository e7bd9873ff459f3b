"""Deterministic TU lists for the all-zero path of the fused matrix-core TU kernel (tuMxBody / tuMx64Body in vvenc_amd/csrc/trquant.hip),
shared by the CPU tier (tests/test_tu_zero_path_inputs.py: the lists have the properties claimed here, by the oracle and — where it is
built — by the compiled reference) and the GPU tier (tests/test_gpu_tu_zero_path.py: the kernel against the oracle on the same lists).

A tile whose TUs all quantise to nothing takes a shortcut: no quantiser loop, no inverse passes, SSE = the residual's energy.  When every
sample of the wave is inside -4096 .. 4095 that energy comes from the registers of the first read (32-bit sums); otherwise the kernel reads
the residual a second time and sums 64-bit squares.  The lists below steer a wave onto each of these routes:

  small_zero  one full 32x32 tile + one partial tile (n = TPT + 1 TUs; 64x64: 3 TUs), top QP', samples within +-4095  -> the shortcut
              (every TU's LARGEST coefficient quantises to 0, see plain_zero: the tile cannot need the quantiser)
  large_zero  the same shape, zeros / tiny noise with one impulse beyond +-4095 in every second TU, top QP'            -> the 64-bit route
  mixed       one full tile of 8x8 / 16x16 TUs in which exactly one TU has a level                                     -> the long way
  multi       64, 32, 16, 8 and 4-point lists for ONE launch, zero and non-zero TUs side by side

Every list is (N, bd, th, tv, thr, resi (n, N, N) int16, qps, irap, luma); `expected` runs it through Oracle.tu_rdo.
"""
import functools

import numpy as np

import tu_extremes as X

THR = 8


def tpt(n):
    """TUs per 32x32 tile of the kernel (a 64x64 TU is a wave of its own)"""
    return 1 if n == 64 else (32 // n) ** 2


def n_partial(n):
    """one full tile and one partial tile: the second tile's unused lanes must contribute nothing"""
    return 3 if n == 64 else tpt(n) + 1


def plain_zero(orc, r, qp, bd, th, tv, irap):
    """the TU's largest coefficient quantises to level 0 — every level is 0 before the coefficient-group threshold has removed any (the quantiser is
    monotonic in |c|): the condition under which a kernel may skip the quantiser.  (abs_sum == 0 alone can be the threshold's doing.)"""
    n = r.shape[-1]
    scale, q_bits, add = orc.quant_params(n, n, bd, qp, irap)
    mx = int(np.abs(orc.xT(r, th, tv, bd).astype(np.int64)).max())
    return ((mx * scale + add) >> q_bits) == 0


def _all_zero(orc, resi, qp, bd, th, tv, irap, luma):
    return all(plain_zero(orc, r, qp, bd, th, tv, irap) and orc.tu_rdo(r, qp, irap, th, tv, bd, THR, luma)[2]["abs_sum"] == 0 for r in resi)


def stage1_fits(orc, resi, th, bd):
    """the forward first stage stays inside 16 bits: the oracle's scalar passes and the saturating rows (x86, the kernels) then agree"""
    n = resi.shape[-1]
    t1 = X.fwd_stage1(resi.astype(np.int64), orc.tr_matrix(th, X.log2(n)).astype(np.int64), X.fwd_shift1(n, bd))
    return bool(t1.max() <= 32767 and t1.min() >= -32768)


def small_zero(orc, n, bd, th=X.DCT2, tv=X.DCT2):
    """noise of the largest amplitude 4095 >> k at which every TU still quantises to nothing at the top QP', then +4095 / -4095 planted in
    every TU that stays all-zero with them (the edge of the 32-bit window)"""
    rng = np.random.default_rng(1000 + 10 * n + bd + 3 * th)
    cnt, qp = n_partial(n), X.qp_max(bd)
    irap, luma = 0, 1
    amp = 4095
    while True:
        resi = rng.integers(-amp, amp + 1, size=(cnt, n, n)).astype(np.int16)
        if amp == 0 or (stage1_fits(orc, resi, th, bd) and _all_zero(orc, resi, qp, bd, th, tv, irap, luma)):
            break
        amp >>= 1
    for i in range(cnt):
        t = resi[i].copy()
        y, x = rng.integers(0, n, 2)
        t[y, x] = 4095
        t[(y + n // 2) % n, (x + 1) % n] = -4095
        if _all_zero(orc, t[None], qp, bd, th, tv, irap, luma) and stage1_fits(orc, t[None], th, bd):
            resi[i] = t
    return (n, bd, th, tv, THR, resi, np.full(cnt, qp), np.full(cnt, irap), np.full(cnt, luma))


# the (size, bit depth) pairs at which a sample beyond +-4095 can pass the forward first stage without saturating it: its DC row alone gives
# 64 |x| >> (log2 N + bd - 9) <= 32767, that is |x| <= 2047 (N = 8) / 4095 (N = 16) at 8 bits.  Beyond that the oracle's scalar transform and the
# saturating rows differ (see tests/test_gpu_tu_extremes.py::test_fused_forms_agree_beyond_the_contract), so those two pairs have no oracle case.
LARGE_CASES = [(8, 10), (16, 10), (32, 10), (64, 10), (32, 8), (64, 8)]


def large_zero(orc, n, bd):
    """every second TU: zeros with one impulse, searched downwards from 32767 for the largest value the oracle still quantises to nothing at the
    top QP' (and that does not saturate the first stage); the other TUs: noise of +-2.  -> (list, impulse)"""
    rng = np.random.default_rng(2000 + 10 * n + bd)
    cnt, qp = n_partial(n), X.qp_max(bd)
    where = rng.integers(0, n, size=(cnt, 2))
    noise = rng.integers(-2, 3, size=(cnt, n, n)).astype(np.int16)

    def build(v):
        resi = noise.copy()
        for i in range(0, cnt, 2):
            resi[i] = 0
            resi[i, where[i, 0], where[i, 1]] = v if (i & 2) == 0 else -v
        return resi

    for v in range(32767, 4095, -97):
        resi = build(v)
        if stage1_fits(orc, resi, X.DCT2, bd) and _all_zero(orc, resi, qp, bd, X.DCT2, X.DCT2, 0, 1):
            return (n, bd, X.DCT2, X.DCT2, THR, resi, np.full(cnt, qp), np.zeros(cnt, int), np.ones(cnt, int)), v
    return None, 0


def mixed(orc, n, bd):
    """one full tile: TU `hot` carries a residual that quantises to levels, the others +-1 noise that does not -> (list, hot)"""
    rng = np.random.default_rng(3000 + 10 * n + bd)
    cnt, qp = tpt(n), 30 + 6 * (bd - 8)
    resi = rng.integers(-1, 2, size=(cnt, n, n)).astype(np.int16)
    hot = int(rng.integers(0, cnt))
    resi[hot] = rng.integers(-(40 << (bd - 8)), (40 << (bd - 8)) + 1, size=(n, n))
    return (n, bd, X.DCT2, X.DCT2, THR, resi, np.full(cnt, qp), rng.integers(0, 2, cnt), rng.integers(0, 2, cnt)), hot


def multi(orc, bd):
    """lists of 64, 32, 16, 8 and 4-point TUs for one launch (the instance with every body): a few tiles each, the last one partial; two TUs in
    three carry +-1 noise (all-zero at this QP'), the others a residual with levels"""
    rng = np.random.default_rng(4000 + bd)
    qp = 30 + 6 * (bd - 8)
    out = []
    for n, cnt in ((64, 3), (32, 3), (16, 9), (8, 37), (4, 133)):
        resi = rng.integers(-1, 2, size=(cnt, n, n)).astype(np.int16)
        for i in range(1, cnt, 3):
            resi[i] = rng.integers(-(60 << (bd - 8)), (60 << (bd - 8)) + 1, size=(n, n))
        out.append((n, bd, X.DCT2, X.DCT2, THR, resi, np.full(cnt, qp), rng.integers(0, 2, cnt), rng.integers(0, 2, cnt)))
    return out


def expected(orc, lst):
    n, bd, th, tv, thr, resi, qps, irap, luma = lst
    return [orc.tu_rdo(resi[i], int(qps[i]), int(irap[i]), th, tv, bd, thr, int(luma[i])) for i in range(len(resi))]


@functools.lru_cache(maxsize=None)
def cached(kind, *key):
    """(list or lists, expected, extra) computed once per process and shared by the tests that need it (treat as read-only)"""
    from oracle.oracle import Oracle
    orc = Oracle()
    if kind == "small":
        lst, extra = small_zero(orc, *key), None
    elif kind == "large":
        lst, extra = large_zero(orc, *key)
    elif kind == "mixed":
        lst, extra = mixed(orc, *key)
    else:
        lst, extra = multi(orc, *key), None
    if lst is None:
        return None, None, extra
    return lst, ([expected(orc, x) for x in lst] if kind == "multi" else expected(orc, lst)), extra
