"""GPU tier: vvhip_intra_chroma_modes_batch at operand limits (tests/intra_chroma_extremes.py) — 12-bit planes at 0 / 4095 with the largest diff, a = +-15 with the largest
luma, b beyond the clip range — every item against the model, tolerance 0.  That the list reaches the limits it is named after is checked in the CPU tier
(tests/test_intra_chroma_cpu.py::test_extremes_list_reaches_the_limits)."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import intra_chroma_cases as CC  # noqa: E402
import intra_chroma_extremes as CX  # noqa: E402
import intra_chroma_ref as CR  # noqa: E402

COST_SENTINEL, PRED_SENTINEL = -0x12345678, -0x5A5B


@pytest.fixture(scope="module")
def hp():
    from vvenc_amd.hotpath import HotPath
    return HotPath()


@pytest.fixture(scope="module")
def extremes():
    cl = CX.cases()
    cnt = {}
    return cl, [CC.expected(c, cnt) for c in cl], cnt


def test_extreme_items_equal_the_model(hp, extremes):
    import torch
    cl, want, _ = extremes
    items, luma, ref, org, npred = CC.as_list(cl)
    cost = torch.full((len(items), CR.NUM_SLOTS), COST_SENTINEL, dtype=torch.int32, device=hp.device)
    pred = torch.full((npred + 64,), PRED_SENTINEL, dtype=torch.int16, device=hp.device)
    t = [torch.from_numpy(np.ascontiguousarray(v)).to(hp.device) for v in (luma, ref, org)]
    hp.intra_chroma_modes(items, *t, cost=cost, pred=pred)
    torch.cuda.synchronize()
    cost, pred = cost.cpu().numpy(), pred.cpu().numpy()
    assert (pred[npred:] == PRED_SENTINEL).all()
    for i, (c, (wc, _, wp)) in enumerate(zip(cl, want)):
        for s in range(CR.NUM_SLOTS):
            assert cost[i][s] == (np.int64(wc[s]) if (c.mode_mask >> s) & 1 else COST_SENTINEL), (c.name, s, int(cost[i][s]), int(wc[s]))
        n = c.w * c.h
        for comp in (0, 1):
            o = int(items[i]["pred_off"][comp])
            assert np.array_equal(pred[o:o + wp.shape[0] * n].reshape(wp.shape[0], c.h, c.w), wp[:, comp]), (c.name, comp)
