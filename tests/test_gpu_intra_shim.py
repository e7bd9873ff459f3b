"""GPU tier: vvhip::IntraOps (the shim's entry to vvhip_intra_luma_modes_batch) on host buffers shaped like the reference's — the unfiltered reference buffer at its own pitch,
the original at a picture pitch — against the reference's own results recorded in tests/golden/intra.npz.  tests/cpp/intra_shim_driver.cpp is compiled here against the built shim, once."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import intra_cases as IC  # noqa: E402
import intra_ref as IR  # noqa: E402

NAMES = ("s4x4", "s8x4", "s8x8", "s16x4", "s4x32", "s32x8", "s8x32", "s16x16", "m1_4x16", "m2_16x16", "b8_8x8", "b12_16x4", "lalt_8x8", "lstep_16x4", "s32x32")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("intra_shim") / "intra_shim_driver")
    subprocess.check_call(["g++", "-std=c++14", "-O1", "-Wall", "-o", path, os.path.join(ROOT, "tests", "cpp", "intra_shim_driver.cpp"), "-L" + os.path.join(ROOT, "vvenc_amd"),
                           "-lvvenc_hip_shim", "-lvvenc_hip", "-Wl,-rpath," + os.path.join(ROOT, "vvenc_amd"), "-Wl,-rpath,/opt/rocm/lib"])
    return path


def test_shim_intra_equals_the_fixture(exe, tmp_path):
    golden = IC.load_golden()
    rng = np.random.default_rng(41)
    blob, want_cost, want_pred = [np.array([len(NAMES)], np.int32).tobytes()], [], []
    for k, name in enumerate(NAMES):
        c, gcost, gpred = golden[name]
        modes = list(c.modes) if k % 2 == 0 else sorted(rng.choice(c.modes, 11, replace=False).tolist())
        pmodes = [m for m in modes if m in c.pred_modes][::3]
        nt, nl = 2 * c.w + 1 + c.mri, 2 * c.h + 1 + c.mri
        ref_stride, org_stride = nt + 3 * (k % 3), c.w + 8 * (k % 2)
        ref = rng.integers(0, 1 << c.bit_depth, ref_stride + nl).astype(np.int16)          # what lies between the rows must not matter
        ref[:nt], ref[ref_stride:] = c.lines[:nt], c.lines[nt:]
        org = rng.integers(0, 1 << c.bit_depth, (c.h, org_stride)).astype(np.int16)
        org[:, :c.w] = c.org
        blob += [np.array([c.w, c.h, c.bit_depth, c.mri, ref_stride, org_stride, len(modes), len(pmodes)] + modes + pmodes, np.int32).tobytes(), ref.tobytes(), org.tobytes()]
        wc = np.zeros(IR.NUM_MODES, np.uint32)
        wc[modes] = gcost[modes]
        want_cost.append(wc)
        want_pred += [gpred[c.pred_modes.index(m)].reshape(-1) for m in pmodes]
    with open(tmp_path / "list.bin", "wb") as f:
        f.write(b"".join(blob))
    r = subprocess.run([exe, str(tmp_path)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stderr)
    assert open(tmp_path / "flow.txt").read().count("\n") == 4
    cost = np.fromfile(tmp_path / "cost.bin", np.uint32).reshape(len(NAMES), IR.NUM_MODES)
    assert np.array_equal(cost, np.stack(want_cost)), np.argwhere(cost != np.stack(want_cost))[:6].tolist()
    assert np.array_equal(np.fromfile(tmp_path / "pred.bin", np.int16), np.concatenate(want_pred))
