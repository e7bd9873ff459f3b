"""GPU tier: vvhip::InterPredOps::predictList (the table-shaped shim's entry to vvhip_pred_inter_batch) on registered pictures — mirror lookup, offsets at the pictures' own line
pitch, blocks reaching into the margins, residual — against the reference (tests/pred_ref.py).  tests/cpp/pred_shim_driver.cpp is compiled here against the built shim."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import pred_ref as PR  # noqa: E402


def test_shim_predict_list(tmp_path, oracle):
    from oracle.oracle import RefLib
    from vvenc_amd.hotpath import PRED_ITEM_DTYPE
    lib = RefLib(1) if RefLib.available() else oracle
    exe = str(tmp_path / "pred_shim_driver")
    subprocess.check_call(["g++", "-std=c++14", "-O1", "-Wall", "-o", exe, os.path.join(ROOT, "tests", "cpp", "pred_shim_driver.cpp"), "-L" + os.path.join(ROOT, "vvenc_amd"),
                           "-lvvenc_hip_shim", "-lvvenc_hip", "-Wl,-rpath," + os.path.join(ROOT, "vvenc_amd"), "-Wl,-rpath,/opt/rocm/lib"])
    rng = np.random.default_rng(404)
    bd, M = 10, 8
    dims = [(128, 96), (128, 96), (64, 48), (64, 48), (128, 96)]          # luma list 0 / 1, chroma list 0 / 1, original; visible size, margin M around each
    planes = [rng.integers(0, 1 << bd, (h + 2 * M, w + 2 * M)).astype(np.int16) for (w, h) in dims]
    with open(tmp_path / "planes.bin", "wb") as f:
        f.write(np.int32(len(planes)).tobytes())
        for (w, h), a in zip(dims, planes):
            f.write(np.array([w, h, M, a.shape[1]], np.int32).tobytes())
            f.write(a.tobytes())
    spec = []          # (w, h, chroma, planes per list); positions relative to sample (0,0), some inside the margin
    for (w, h) in ((4, 4), (8, 8), (16, 8), (32, 32), (64, 16), (128, 64), (8, 64)):
        spec += [(w, h, 0, (0, -1)), (w, h, 0, (0, 1)), (w, h, 0, (-1, 1))]
    for (w, h) in ((2, 2), (4, 2), (4, 8), (16, 16), (32, 8), (64, 32)):
        spec += [(w, h, 1, (2, -1)), (w, h, 1, (2, 3)), (w, h, 1, (3, 3))]
    items, pos, at = np.zeros(len(spec), PRED_ITEM_DTYPE), [], 0
    for k, (w, h, chroma, rp) in enumerate(spec):
        pw, ph = dims[2 if chroma else 0]
        m = 2 if chroma else 4
        it = items[k]
        it["width"], it["height"], it["chroma"], it["ref_plane"], it["dst_off"] = w, h, chroma, rp, at
        ox, oy = int(rng.integers(0, 128 - w + 1)), int(rng.integers(0, 96 - h + 1))
        it["org_off"] = oy * planes[4].shape[1] + ox
        p = [None, None]
        for l in (0, 1):
            if rp[l] < 0:
                continue
            x, y = (int(rng.integers(m - M, pw + M - m - w + 1)), int(rng.integers(m - M, ph + M - m - h))) if k % 3 else (m - M, m - M)
            it["ref_off"][l] = y * planes[rp[l]].shape[1] + x
            it["frac"][l] = (int(rng.integers(0, 32 if chroma else 16)), int(rng.integers(0, 32 if chroma else 16)))
            p[l] = (x + M, y + M)
        pos.append((p, (ox + M, oy + M)))
        at += w * h
    with open(tmp_path / "items.bin", "wb") as f:
        f.write(np.array([len(items), at, 4, 4], np.int32).tobytes())
        f.write(items.tobytes())
    r = subprocess.run([exe, str(tmp_path), str(bd)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    pred, resi = np.fromfile(tmp_path / "pred.bin", np.int16), np.fromfile(tmp_path / "resi.bin", np.int16)
    assert pred.size == at and resi.size == at
    for k, it in enumerate(items):
        w, h, o = int(it["width"]), int(it["height"]), int(it["dst_off"])
        e = PR.expected_block(lib, planes, pos[k][0], it, bd)
        assert np.array_equal(pred[o:o + w * h].reshape(h, w), e), ("pred", k, it)
        ox, oy = pos[k][1]
        assert np.array_equal(resi[o:o + w * h].reshape(h, w), PR.residual(planes[4][oy:oy + h, ox:ox + w], e)), ("resi", k, it)
