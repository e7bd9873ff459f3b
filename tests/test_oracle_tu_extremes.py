"""Pins the oracle to the compiled reference (scalar row and x86 SIMD row, tolerance 0) on the TU pipeline's extreme inputs of
tests/tu_extremes.py: basis-aligned residuals at the bit-depth maximum, coefficient blocks that overflow the inverse first stage, the
int8 byte-split edges, and quantiser inputs on the level / need-RDOQ / coefficient-group edges at EVERY QP' of 8- and 10-bit video.
The GPU tier (tests/test_gpu_tu_extremes.py) compares the kernels with the oracle on the same sets; this file is what makes the oracle
trustworthy there.  The guards assert that the sets reach the limits they are built for.

The two reference rows agree on every in-contract input here, so no case needs the x86-row rule of
tests/test_e2e_bitstream.py::test_production_mask_equals_the_x86_row_where_the_references_rows_differ.
"""
import numpy as np
import pytest

import tu_extremes as X

pytestmark = pytest.mark.ref


@pytest.mark.parametrize("bd", [8, 10])
def test_transforms_on_extreme_inputs(oracle, reflib, bd):
    """xT on the forward-extreme residuals, xIT on the inverse-extreme blocks, every shape 2..64 and legal type pair; the guards: the
    forward first stage comes within 1 % of 32767 on the DCT-2 set of every shape, the inverse first stage leaves [-32768, 32767]"""
    inv_clipped = 0
    for w in X.SIZES:
        for h in X.SIZES:
            for th, tv in X.tr_types(w, h):
                resi = X.fwd_residuals(oracle.tr_matrix, w, h, th, tv, bd)
                if (th, tv) == (X.DCT2, X.DCT2):
                    t1 = X.fwd_stage1(resi, oracle.tr_matrix(th, X.log2(w)), X.fwd_shift1(w, bd))
                    assert np.abs(t1).max() >= 0.99 * 32767, ("forward stage 1 below its bound", w, h, bd, int(np.abs(t1).max()))
                    assert np.abs(t1).max() <= 32768
                for i in range(len(resi)):
                    a, b = oracle.xT(resi[i], th, tv, bd), reflib.xT(resi[i], th, tv, bd)
                    assert np.array_equal(a, b), ("xT", w, h, th, tv, bd, i)
                coef = X.inv_coefs(oracle.tr_matrix, w, h, th, tv, seed=w * h)
                t1 = X.inv_stage1(coef, oracle.tr_matrix(tv, X.log2(h)))
                inv_clipped += int(((t1 < -32768) | (t1 > 32767)).any(axis=(1, 2)).sum())
                for i in range(len(coef)):
                    a, b = oracle.xIT(coef[i], th, tv, bd), reflib.xIT(coef[i], th, tv, bd)
                    assert np.array_equal(a, b), ("xIT", w, h, th, tv, bd, i)
    assert inv_clipped > 100, inv_clipped


def test_1d_passes_on_extreme_rows(oracle, reflib):
    """fwd_1d / inv_1d (every g_tCoeffOps size and type) on rows that saturate them: the sign of a basis row / column at the 16-bit
    edges, the byte-split edges, with and without the zero-out skips"""
    for t, logs in ((X.DCT2, range(1, 7)), (X.DCT8, range(2, 6)), (X.DST7, range(2, 6))):
        for l in logs:
            n = 1 << l
            T = oracle.tr_matrix(t, l).astype(np.int64)
            for line in (4, 16, 64):
                for skip, skip2 in ((0, 0), (line // 2, n // 2 if n >= 8 else 0)):
                    for k in sorted({0, 1 % n, n // 2, n - 1}):
                        # forward: lines of sign(b_k) at the 16-bit edges, shifts that keep / overflow 16 bits
                        src = np.tile(np.where(T[k] < 0, -32768, 32767), line).astype(np.int32)
                        for sh in (6, 9, 12):
                            a, b = oracle.fwd_1d(t, l, src, sh, line, skip, skip2), reflib.fwd_1d(t, l, src, sh, line, skip, skip2)
                            assert np.array_equal(a, b), ("fwd", t, n, line, skip, skip2, k, sh)
                        # inverse: column k's signs in every line (row-major [k][line])
                        srci = np.repeat(np.where(T[:, k] < 0, -32768, 32767)[:, None], line, 1).astype(np.int32)
                        if skip2:
                            srci[n - skip2:, :] = 0
                        for sh in (7, 12):
                            a, b = oracle.inv_1d(t, l, srci.ravel(), sh, line, skip, skip2), reflib.inv_1d(t, l, srci.ravel(), sh, line, skip, skip2)
                            assert np.array_equal(a, b), ("inv", t, n, line, skip, skip2, k, sh)
                            assert a.max() == 32767 or a.min() == -32768 or sh == 12
                    edges = np.resize(np.array(X.BYTE_EDGES, np.int32), n * line)
                    a, b = oracle.fwd_1d(t, l, edges, 8, line, skip, skip2), reflib.fwd_1d(t, l, edges, 8, line, skip, skip2)
                    assert np.array_equal(a, b), ("fwd edges", t, n, line)
                    if skip2:
                        edges.reshape(n, line)[n - skip2:, :] = 0
                    a, b = oracle.inv_1d(t, l, edges, 7, line, skip, skip2), reflib.inv_1d(t, l, edges, 7, line, skip, skip2)
                    assert np.array_equal(a, b), ("inv edges", t, n, line)


@pytest.mark.parametrize("bd", [8, 10])
def test_quantiser_at_every_qp(oracle, reflib, bd):
    """QuantCore (thr 8 and 4, sign hiding on), DeQuantCore and needRdoqCore at every QP' 0..63 + 6 (bd - 8), irap 0 / 1, luma / chroma,
    every shape, on the level edges (k = 1, 2 and the clip at 32767), the need-RDOQ edge and the coefficient-group edge; the guards: levels
    clip at 32767, the clamp of DeQuantCore's input bites, both need-RDOQ outcomes and both coefficient-group outcomes occur"""
    clipped = clamp_bites = 0
    need_seen, cg_seen = set(), set()
    for w in X.SIZES:
        for h in X.SIZES:
            scan = oracle.scan_order(X.log2(w), X.log2(h))
            for qp in range(X.qp_max(bd) + 1):
                for irap in (0, 1):
                    scale, q_bits, add = oracle.quant_params(w, h, bd, qp, irap)
                    for thr in (8, 4):
                        blocks = X.quant_blocks(oracle, w, h, bd, qp, irap, thr)
                        for i, c in enumerate(blocks):
                            a = oracle.quant_core(c, scale, q_bits, add, thr)
                            b = reflib.quant_core(c, scale, q_bits, add, thr, sign_hiding=True)
                            assert (a[2], a[3]) == (b[2], b[3]), ("sum/last", w, h, bd, qp, irap, thr, i, a[2:], b[2:])
                            assert np.array_equal(a[0], b[0]), ("levels", w, h, bd, qp, irap, thr, i)
                            keep = np.zeros(h * w, bool)
                            keep[scan[: a[3] + 1]] = True
                            assert np.array_equal(a[1][keep], b[1][keep]), ("deltaU", w, h, bd, qp, irap, thr, i)
                            clipped += int((np.abs(a[0].astype(np.int64)) == 32767).any() and np.abs(c).max() >= X.level_edge(32768, scale, q_bits, add))
                            if i >= 2 and w * h >= 64:
                                cg_seen.add((i, a[3] > 15))
                sc, rs, imax = oracle.dequant_params(w, h, bd, qp)
                for i, lv in enumerate(X.dequant_levels(h, w, seed=qp)):
                    a, b = oracle.dequant_core(lv, sc, rs, imax), reflib.dequant_core(lv, sc, rs, imax)
                    assert np.array_equal(a, b), ("dequant", w, h, bd, qp, i)
                clamp_bites += imax < 32767
                for luma in (0, 1):
                    qc, qb, off, num = oracle.need_rdoq_params(w, h, bd, qp, luma)
                    for i, c in enumerate(X.need_rdoq_blocks(oracle, w, h, bd, qp, luma)):
                        a, b = oracle.need_rdoq(c.ravel()[:num], qc, off, qb), reflib.need_rdoq(c.ravel()[:num], qc, off, qb)
                        assert a == b, ("need", w, h, bd, qp, luma, i)
                        need_seen.add((i, a))
    assert clipped > 0 and clamp_bites > 0, (clipped, clamp_bites)
    assert need_seen == {(0, 0), (1, 1), (2, 1), (3, 0)}, need_seen
    assert {(2, False), (3, True)} <= cg_seen, cg_seen
