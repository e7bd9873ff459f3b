"""CPU tier: the lists of tests/tu_zero_inputs.py have the properties the GPU tier (tests/test_gpu_tu_zero_path.py) relies on — shown by the
oracle alone, and by the compiled reference's two rows where oracle/_ref is built — so the inputs are valid without the code under test:

  * small_zero: every TU's abs_sum is 0 at the top QP', every sample is within +-4095, the first forward stage does not saturate
  * large_zero: at least one sample beyond +-4095 per list, abs_sum 0 everywhere, an SSE that is that residual's energy
  * mixed: exactly one TU of the tile has levels
  * multi: every size of the launch holds all-zero and non-zero TUs
"""
import numpy as np
import pytest

import tu_extremes as X
import tu_zero_inputs as Z

SMALL = [(8, X.DCT2), (16, X.DCT2), (32, X.DCT2), (32, X.DST7), (64, X.DCT2)]


def _energy(r):
    return int((r.astype(np.int64) ** 2).sum())


@pytest.mark.parametrize("bd", [8, 10])
@pytest.mark.parametrize("n,tr", SMALL)
def test_small_zero_lists_are_all_zero_and_small(oracle, n, tr, bd):
    lst, exp, _ = Z.cached("small", n, bd, tr, tr)
    resi = lst[5]
    assert len(resi) == Z.n_partial(n)
    assert np.abs(resi.astype(np.int32)).max() <= 4095
    assert np.abs(resi.astype(np.int32)).max() > 0
    assert Z.stage1_fits(oracle, resi, tr, bd)
    for i, (lev, rec, st) in enumerate(exp):
        assert st["abs_sum"] == 0 and not lev.any() and not rec.any(), (n, bd, i)
        assert st["sse"] == _energy(resi[i]), (n, bd, i)
        assert Z.plain_zero(oracle, resi[i], int(lst[6][i]), bd, tr, tr, int(lst[7][i])), (n, bd, i)


@pytest.mark.parametrize("n,bd", Z.LARGE_CASES)
def test_large_zero_lists_hold_an_impulse_beyond_the_window(oracle, n, bd):
    lst, exp, v = Z.cached("large", n, bd)
    assert lst is not None and v > 4095, (n, bd, v)
    resi = lst[5]
    big = np.abs(resi.astype(np.int32)).reshape(len(resi), -1).max(axis=1)
    assert (big > 4095).sum() == (len(resi) + 1) // 2 and big.max() == v
    assert (big[1::2] <= 2).all()                                   # the TUs in between are small: the wave decides, not the TU
    assert Z.stage1_fits(oracle, resi, X.DCT2, bd)
    for i, (lev, rec, st) in enumerate(exp):
        assert st["abs_sum"] == 0 and not lev.any() and not rec.any(), (n, bd, i)
        assert st["sse"] == _energy(resi[i]), (n, bd, i)
        assert Z.plain_zero(oracle, resi[i], int(lst[6][i]), bd, X.DCT2, X.DCT2, int(lst[7][i])), (n, bd, i)


@pytest.mark.parametrize("n,bd", sorted({(8, 8), (16, 8)} - set(Z.LARGE_CASES)))
def test_no_large_impulse_exists_where_the_first_stage_saturates(oracle, n, bd):
    """the two (size, bit depth) pairs left out of LARGE_CASES: any sample beyond +-4095 saturates the forward first stage"""
    for v in (4096, -4097, 32767):
        r = np.zeros((1, n, n), np.int16)
        r[0, n // 2, n // 3] = v
        assert not Z.stage1_fits(oracle, r, X.DCT2, bd), (n, bd, v)


@pytest.mark.parametrize("bd", [8, 10])
@pytest.mark.parametrize("n", [8, 16])
def test_mixed_tile_has_exactly_one_tu_with_levels(oracle, n, bd):
    lst, exp, hot = Z.cached("mixed", n, bd)
    assert len(lst[5]) == Z.tpt(n)
    nz = [i for i, e in enumerate(exp) if e[2]["abs_sum"] != 0]
    assert nz == [hot], (n, bd, nz, hot)
    assert exp[hot][0].any()


@pytest.mark.parametrize("bd", [8, 10])
def test_multi_lists_mix_zero_and_nonzero_tus_in_every_size(oracle, bd):
    lists, exps, _ = Z.cached("multi", bd)
    assert [x[0] for x in lists] == [64, 32, 16, 8, 4]
    for lst, exp in zip(lists, exps):
        s = np.array([e[2]["abs_sum"] for e in exp])
        assert (s == 0).any() and (s != 0).any(), (lst[0], bd)
        assert lst[0] >= 32 or len(exp) % Z.tpt(lst[0]) != 0          # the last tile of the small sizes is partial


def _ref_stats(oracle, ref, lst, i):
    """abs_sum / last / need-RDOQ of TU i from the reference's own kernels (xT -> QuantCore, needRdoq), with the oracle's parameter derivation"""
    n, bd, th, tv, thr, resi, qps, irap, luma = lst
    coef = ref.xT(resi[i], th, tv, bd)
    scale, qb, add = oracle.quant_params(n, n, bd, int(qps[i]), int(irap[i]))
    lev, _, s, last = ref.quant_core(coef, scale, qb, add, thr)
    nsc, nqb, noff, num = oracle.need_rdoq_params(n, n, bd, int(qps[i]), int(luma[i]))
    return lev, s, last, ref.need_rdoq(coef.ravel()[:num], nsc, noff, nqb)


@pytest.mark.ref
@pytest.mark.parametrize("bd", [8, 10])
def test_reference_rows_agree_on_the_lists(oracle, reflib, bd):
    """both rows of the compiled reference give the oracle's levels and statistics on every list"""
    todo = [Z.cached("small", n, bd, tr, tr)[:2] for n, tr in SMALL]
    todo += [Z.cached("large", n, b)[:2] for n, b in Z.LARGE_CASES if b == bd]
    todo += [Z.cached("mixed", n, bd)[:2] for n in (8, 16)]
    lists, exps, _ = Z.cached("multi", bd)
    todo += list(zip(lists, exps))
    for lst, exp in todo:
        for i, (lev, _, st) in enumerate(exp):
            rl, s, last, need = _ref_stats(oracle, reflib, lst, i)
            assert np.array_equal(rl, lev), (lst[0], bd, i)
            assert (s, last, need) == (st["abs_sum"], st["last_scan_pos"], st["need_rdoq"]), (lst[0], bd, i)
