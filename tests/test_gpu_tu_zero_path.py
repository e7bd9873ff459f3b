"""-m gpu: the all-zero path of the fused matrix-core TU kernel against the oracle, tolerance 0, on the lists of tests/tu_zero_inputs.py
(tests/test_tu_zero_path_inputs.py shows on the CPU that the lists are what they claim to be).

A tile whose TUs all quantise to nothing gets its SSE from the energy taken at the FIRST read of the residual when every sample of the wave
is within -4096 .. 4095, and from a second read with 64-bit squares otherwise.  Every list goes through vvhip_tu_rdo_multi_strided (compact
blocks, pitch = width) and vvhip_tu_rdo_multi (one plane, pitch > width), dense and sparse outputs, four waves and one wave per workgroup
($VVHIP_TU_WG1); level, reconstruction and all five statistics fields are compared.  Output buffers are pre-filled with garbage: a store
that is skipped fails, and with sparse outputs an all-zero TU must leave levels and reconstruction untouched.
"""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import tu_extremes as X  # noqa: E402
import tu_zero_inputs as Z  # noqa: E402

GARBAGE16 = 0x5A5A
SMALL = [(8, X.DCT2), (16, X.DCT2), (32, X.DCT2), (32, X.DST7), (64, X.DCT2)]


@pytest.fixture(scope="module")
def hp():
    from vvenc_amd.hotpath import HotPath
    return HotPath()


def _launch(hp, lists, bd, strided):
    """one launch of all `lists`; -> per list (levels, reconstruction, stats records)"""
    import torch
    from vvenc_amd.hotpath import STATS_DTYPE, HotPath, Plane
    jobs, strides, at_row, at = [], [], 0, 0
    plane = None if strided else Plane(hp.device, 64 + 8, sum(len(L[5]) * L[0] for L in lists))
    pool = hp.to_device(np.concatenate([L[5].reshape(-1) for L in lists])) if strided else None
    for (n, _, th, tv, thr, resi, qps, irap, luma) in lists:
        k = len(resi)
        if strided:
            off = at + np.arange(k, dtype=np.int32) * n * n
        else:
            plane.storage[at_row:at_row + k * n, :n] = torch.from_numpy(resi.reshape(k * n, n)).to(hp.device)
            off = (at_row + np.arange(k, dtype=np.int32) * n) * plane.stride
        lv = torch.full((k * n * n,), GARBAGE16, dtype=torch.int16, device=hp.device)
        rc = torch.full((k * n * n,), GARBAGE16, dtype=torch.int16, device=hp.device)
        st = torch.full((k, STATS_DTYPE.itemsize), 0xA5, dtype=torch.uint8, device=hp.device)
        jobs.append((n, n, th, tv, k, thr, hp.to_device(off.astype(np.int32)), hp.to_device(HotPath.tu_qp(qps, irap, luma)), lv, rc, st))
        strides.append(n)
        at_row += k * n
        at += k * n * n
    if strided:
        hp.tu_rdo_multi_strided(pool, strides, jobs, bd)
    else:
        assert plane.stride > 64
        hp.tu_rdo_multi(plane, jobs, bd)
    torch.cuda.synchronize()
    return [(J[8].cpu().numpy().reshape(-1, L[0], L[0]), J[9].cpu().numpy().reshape(-1, L[0], L[0]), J[10].cpu().numpy().view(STATS_DTYPE).reshape(-1))
            for L, J in zip(lists, jobs)]


def _check(hp, monkeypatch, lists, exps, bd, tag, whole_tiles_zero=False):
    """every form of the launch: compact / strided residuals x dense / sparse outputs x four waves / one wave per workgroup.  Sparse outputs: a TU
    without levels is untouched (its tile took the shortcut: required when every TU of the lists is all-zero) or zero (it shared a tile with levels)"""
    garbage = np.int16(GARBAGE16)
    try:
        for wg1 in ("0", "1"):
            monkeypatch.setenv("VVHIP_TU_WG1", wg1)
            for sparse in (0, 1):
                hp.tu_set_sparse_outputs(sparse)
                for strided in (True, False):
                    for L, exp, (lv, rc, sv) in zip(lists, exps, _launch(hp, lists, bd, strided)):
                        for i, (el, er, es) in enumerate(exp):
                            what = (tag, L[0], bd, "wg1=" + wg1, "sparse" if sparse else "dense", "compact" if strided else "plane", i)
                            got = (int(sv["abs_sum"][i]), int(sv["last_scan_pos"][i]), int(sv["need_rdoq"][i]), int(sv["pad"][i]), int(sv["sse"][i]))
                            assert got == (es["abs_sum"], es["last_scan_pos"], es["need_rdoq"], 0, es["sse"]), ("stats",) + what + (got, es)
                            if es["abs_sum"] or not sparse:
                                assert np.array_equal(lv[i], el), ("lev",) + what
                                assert np.array_equal(rc[i], er), ("rec",) + what
                            else:
                                untouched = bool((lv[i] == garbage).all() and (rc[i] == garbage).all())
                                assert untouched or (not whole_tiles_zero and not lv[i].any() and not rc[i].any()), ("sparse outputs",) + what
    finally:
        hp.tu_set_sparse_outputs(0)


@pytest.mark.parametrize("bd", [8, 10])
@pytest.mark.parametrize("n,tr", SMALL)
def test_all_zero_tiles_small_samples(hp, monkeypatch, n, tr, bd):
    """one full and one partial tile, top QP', samples within +-4095: the shortcut without a second read (asserted: every abs_sum is 0)"""
    lst, exp, _ = Z.cached("small", n, bd, tr, tr)
    assert all(e[2]["abs_sum"] == 0 for e in exp)
    assert np.abs(lst[5].astype(np.int32)).max() <= 4095
    _check(hp, monkeypatch, [lst], [exp], bd, "small", whole_tiles_zero=True)


@pytest.mark.parametrize("n,bd", Z.LARGE_CASES)
def test_all_zero_tiles_large_samples(hp, monkeypatch, n, bd):
    """an impulse beyond +-4095 in every second TU (the largest the oracle still quantises to nothing), top QP': the 64-bit route"""
    lst, exp, v = Z.cached("large", n, bd)
    assert v > 4095 and np.abs(lst[5].astype(np.int32)).max() == v
    assert all(e[2]["abs_sum"] == 0 for e in exp)
    _check(hp, monkeypatch, [lst], [exp], bd, "large", whole_tiles_zero=True)


@pytest.mark.parametrize("bd", [8, 10])
@pytest.mark.parametrize("n", [8, 16])
def test_mixed_tile_takes_the_long_way(hp, monkeypatch, n, bd):
    """one tile, exactly one TU with a level: the wave runs the quantiser and the inverse passes for all of them"""
    lst, exp, hot = Z.cached("mixed", n, bd)
    s = [e[2]["abs_sum"] for e in exp]
    assert s[hot] != 0 and sum(1 for x in s if x == 0) == len(s) - 1 and len(s) > 1
    _check(hp, monkeypatch, [lst], [exp], bd, "mixed")


@pytest.mark.parametrize("bd", [8, 10])
def test_one_launch_with_every_size(hp, monkeypatch, bd):
    """64, 32, 16, 8 and 4-point lists in one launch (the instance that holds every body): the 4-point list next to the changed bodies"""
    lists, exps, _ = Z.cached("multi", bd)
    assert [L[0] for L in lists] == [64, 32, 16, 8, 4]
    _check(hp, monkeypatch, lists, exps, bd, "multi")


def test_small_and_large_lists_in_one_launch(hp, monkeypatch):
    """both routes of the all-zero path side by side, every size, one launch (10-bit: every size has a large case)"""
    lists, exps = [], []
    for n in (64, 32, 16, 8):
        for kind, key in (("small", (n, 10, X.DCT2, X.DCT2)), ("large", (n, 10))):
            lst, exp, _ = Z.cached(kind, *key)
            lists.append(lst)
            exps.append(exp)
    _check(hp, monkeypatch, lists, exps, 10, "small+large", whole_tiles_zero=True)
