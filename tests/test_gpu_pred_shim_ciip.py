"""GPU tier: vvhip::InterPredOps::predictList with CIIP records (the shim's entry to vvhip_pred_inter_batch_ciip) on registered pictures — one CIIP CU as its luma block
and its chroma block, a BCW CIIP block and a uni-predicted one, beside a plain, a GEO and a BDOF item with their records OFF in the same list, with the residual —
against tests/ciip_ref.py; the same list without the CIIP array, which must give the blend entry's output; and the list with its records once more (the schedule slots
of the two entries side by side).  tests/cpp/pred_shim_ciip_driver.cpp is compiled here against the built shim."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import bdof_ref as BR  # noqa: E402
import blend_cases as BLC  # noqa: E402
import blend_ref as BL  # noqa: E402
import ciip_cases as CC  # noqa: E402
import ciip_ref as CR  # noqa: E402
import pred_ref as PR  # noqa: E402


def test_shim_predict_list_with_ciip_records(tmp_path, oracle):
    exe = str(tmp_path / "pred_shim_ciip_driver")
    subprocess.check_call(["g++", "-std=c++14", "-O1", "-Wall", "-o", exe, os.path.join(ROOT, "tests", "cpp", "pred_shim_ciip_driver.cpp"), "-L" + os.path.join(ROOT, "vvenc_amd"),
                           "-lvvenc_hip_shim", "-lvvenc_hip", "-Wl,-rpath," + os.path.join(ROOT, "vvenc_amd"), "-Wl,-rpath,/opt/rocm/lib"])
    rng = np.random.default_rng(707)
    bd, M = 10, 8
    dims = [(128, 96), (128, 96), (64, 48), (64, 48), (128, 96)]          # luma list 0 / 1, chroma list 0 / 1, original; visible size, margin M around each
    yy, xx = np.mgrid[0:96 + 2 * M, 0:128 + 2 * M]
    tex = 512 + 200 * np.sin(xx / 6.0) * np.cos(yy / 5.0)
    planes = [np.clip(tex[:h + 2 * M, :w + 2 * M] + rng.normal(0, 30, (h + 2 * M, w + 2 * M)) + 60 * k, 0, 1023).astype(np.int16) for k, (w, h) in enumerate(dims)]
    with open(tmp_path / "planes.bin", "wb") as f:
        f.write(np.int32(len(planes)).tobytes())
        for (w, h), a in zip(dims, planes):
            f.write(np.array([w, h, M, a.shape[1]], np.int32).tobytes())
            f.write(a.tobytes())
    spec = [(64, 32, 0, (0, 1), 0, BL.BLEND_DEFAULT, 0, 2), (32, 16, 1, (2, 3), 0, BL.BLEND_DEFAULT, 0, 2),          # (w, h, chroma, planes per list, flags, mode, param, num_intra / None)
            (16, 16, 0, (1, 0), 0, BL.BLEND_BCW, 4, 0), (16, 4, 0, (0, -1), 0, BL.BLEND_DEFAULT, 0, 1), (8, 2, 1, (-1, 3), 0, BL.BLEND_DEFAULT, 0, 1),
            (16, 16, 0, (0, 1), 0, BL.BLEND_DEFAULT, 0, None), (32, 32, 0, (1, 0), 0, BL.BLEND_GEO, 21, None), (32, 16, 0, (0, 1), BR.EXT_BDOF, BL.BLEND_DEFAULT, 0, None)]
    n = len(spec)
    items, ext, blend, ciip = np.zeros(n, CC.PRED_ITEM_DTYPE), np.zeros(n, CC.PRED_EXT_DTYPE), np.zeros(n, CC.PRED_BLEND_DTYPE), np.zeros(n, CC.PRED_CIIP_DTYPE)
    pos, at, lines = [], 0, [np.full(3, -1, np.int16)]
    for k, (w, h, chroma, rp, flags, mode, param, ni) in enumerate(spec):
        pw, ph = dims[2 if chroma else 0]
        m = 2 if chroma else 4
        it = items[k]
        it["width"], it["height"], it["chroma"], it["ref_plane"], it["dst_off"], ext[k]["flags"], blend[k]["mode"], blend[k]["param"] = w, h, chroma, rp, at, flags, mode, param
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
        if ni is not None:
            pic = planes[3 if chroma else 1]
            ciip[k] = (sum(a.size for a in lines), CR.CIIP_ON, ni, (0, 0))
            lines.append(CR.line_at(pic, int(rng.integers(1, 20)), int(rng.integers(1, 20)), w, h))
        at += w * h
    lines = np.concatenate(lines)
    with open(tmp_path / "items.bin", "wb") as f:
        f.write(np.array([n, at, 4, 4, lines.size, 0], np.int32).tobytes())
        f.write(items.tobytes())
        f.write(ext.tobytes())
        f.write(blend.tobytes() + (b"\0\0\0\0" if n & 1 else b""))
        f.write(ciip.tobytes())
        f.write(lines.tobytes())
    r = subprocess.run([exe, str(tmp_path), str(bd)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    pred, resi, plain, again = (np.fromfile(tmp_path / name, np.int16) for name in ("pred.bin", "resi.bin", "plain.bin", "again.bin"))
    assert pred.size == at and resi.size == at and plain.size == at and np.array_equal(again, pred)
    for k, it in enumerate(items):
        w, h, o = int(it["width"]), int(it["height"]), int(it["dst_off"])
        e = CC.expected(oracle, planes, pos[k][0], it, ext[k], blend[k], ciip[k], lines, bd)
        assert np.array_equal(pred[o:o + w * h].reshape(h, w), e), ("pred", k, it, ciip[k])
        ox, oy = pos[k][1]
        assert np.array_equal(resi[o:o + w * h].reshape(h, w), PR.residual(planes[4][oy:oy + h, ox:ox + w], e)), ("resi", k, it)
        e0 = BLC.expected(oracle, planes, pos[k][0], it, ext[k], blend[k], bd)
        assert np.array_equal(plain[o:o + w * h].reshape(h, w), e0), ("without CIIP records", k, it)
        assert np.array_equal(e, e0) == (int(ciip[k]["mode"]) == CR.CIIP_OFF), ("the CIIP record changes nothing on item", k)
