"""GPU tier: vvhip::InterPredOps::predictList with extension records (the shim's entry to vvhip_pred_inter_batch_ex) on registered pictures — BDOF items of several sizes,
refined DMVR sub-blocks (luma with and without BDOF, chroma), plain items in the same list, residual — against tests/bdof_ref.py; and the same list without the
extension array, which must give the plain values.  tests/cpp/pred_shim_ext_driver.cpp is compiled here against the built shim."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import bdof_cases as BC  # noqa: E402
import bdof_ref as BR  # noqa: E402
import pred_ref as PR  # noqa: E402


def test_shim_predict_list_with_extensions(tmp_path, oracle):
    from oracle.oracle import RefLib
    lib = RefLib(1) if RefLib.available() else oracle
    exe = str(tmp_path / "pred_shim_ext_driver")
    subprocess.check_call(["g++", "-std=c++14", "-O1", "-Wall", "-o", exe, os.path.join(ROOT, "tests", "cpp", "pred_shim_ext_driver.cpp"), "-L" + os.path.join(ROOT, "vvenc_amd"),
                           "-lvvenc_hip_shim", "-lvvenc_hip", "-Wl,-rpath," + os.path.join(ROOT, "vvenc_amd"), "-Wl,-rpath,/opt/rocm/lib"])
    rng = np.random.default_rng(505)
    bd, M = 10, 8
    dims = [(128, 96), (128, 96), (64, 48), (64, 48), (128, 96)]          # luma list 0 / 1, chroma list 0 / 1, original; visible size, margin M around each
    yy, xx = np.mgrid[0:96 + 2 * M, 0:128 + 2 * M]
    tex = 512 + 200 * np.sin(xx / 6.0) * np.cos(yy / 5.0)
    planes = [np.clip(tex[:h + 2 * M, :w + 2 * M] + rng.normal(0, 30, (h + 2 * M, w + 2 * M)), 0, 1023).astype(np.int16) for (w, h) in dims]
    with open(tmp_path / "planes.bin", "wb") as f:
        f.write(np.int32(len(planes)).tobytes())
        for (w, h), a in zip(dims, planes):
            f.write(np.array([w, h, M, a.shape[1]], np.int32).tobytes())
            f.write(a.tobytes())
    spec = []          # (w, h, chroma, planes per list, flags, deltas)
    for (w, h) in ((8, 16), (16, 8), (16, 16), (32, 16), (64, 64), (128, 32)):
        spec += [(w, h, 0, (0, 1), BR.EXT_BDOF, None), (w, h, 0, (0, 1), 0, None), (w, h, 0, (0, -1), 0, None)]
    for (w, h) in ((16, 16), (8, 16), (16, 8)):
        spec += [(w, h, 0, (0, 1), BR.EXT_BDOF | BR.EXT_DMVR_PAD, ((2, -1), (-2, 1))), (w, h, 0, (0, 1), BR.EXT_DMVR_PAD, ((-1, 2), (1, -2))),
                 (w // 2, h // 2, 1, (2, 3), BR.EXT_DMVR_PAD, ((1, -1), (-1, 1))), (w // 2, h // 2, 1, (2, 3), 0, None)]
    items, ext, pos, at = np.zeros(len(spec), BC.PRED_ITEM_DTYPE), np.zeros(len(spec), BC.PRED_EXT_DTYPE), [], 0
    for k, (w, h, chroma, rp, flags, delta) in enumerate(spec):
        pw, ph = dims[2 if chroma else 0]
        m = 2 if chroma else 4
        it = items[k]
        it["width"], it["height"], it["chroma"], it["ref_plane"], it["dst_off"], ext[k]["flags"] = w, h, chroma, rp, at, flags
        ox, oy = int(rng.integers(0, 128 - w + 1)), int(rng.integers(0, 96 - h + 1))
        it["org_off"] = oy * planes[4].shape[1] + ox
        p = [None, None]
        for l in (0, 1):
            if rp[l] < 0:
                continue
            x, y = (int(rng.integers(m - M, pw + M - m - w + 1)), int(rng.integers(m - M, ph + M - m - h))) if k % 3 else (m - M, m - M)          # the START position
            if delta is not None:
                ext[k]["pad_dx"][l], ext[k]["pad_dy"][l] = delta[l]
                x, y = x + delta[l][0], y + delta[l][1]
            it["ref_off"][l] = y * planes[rp[l]].shape[1] + x
            it["frac"][l] = (int(rng.integers(0, 32 if chroma else 16)), int(rng.integers(0, 32 if chroma else 16)))
            p[l] = (x + M, y + M)
        pos.append((p, (ox + M, oy + M)))
        at += w * h
    with open(tmp_path / "items.bin", "wb") as f:
        f.write(np.array([len(items), at, 4, 4], np.int32).tobytes())
        f.write(items.tobytes())
        f.write(ext.tobytes())
    r = subprocess.run([exe, str(tmp_path), str(bd)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    pred, resi, plain = (np.fromfile(tmp_path / n, np.int16) for n in ("pred.bin", "resi.bin", "plain.bin"))
    assert pred.size == at and resi.size == at and plain.size == at
    changed = 0
    for k, it in enumerate(items):
        w, h, o = int(it["width"]), int(it["height"]), int(it["dst_off"])
        e = BR.expected_block_ex(lib, planes, pos[k][0], it, ext[k], bd)
        assert np.array_equal(pred[o:o + w * h].reshape(h, w), e), ("pred", k, it, ext[k])
        ox, oy = pos[k][1]
        assert np.array_equal(resi[o:o + w * h].reshape(h, w), PR.residual(planes[4][oy:oy + h, ox:ox + w], e)), ("resi", k, it)
        e0 = PR.expected_block(lib, planes, pos[k][0], it, bd)
        assert np.array_equal(plain[o:o + w * h].reshape(h, w), e0), ("without extensions", k, it)
        changed += int(ext[k]["flags"]) != 0 and not np.array_equal(e, e0)
    assert changed * 2 > int(np.count_nonzero(ext["flags"]))          # the extensions matter on this list
