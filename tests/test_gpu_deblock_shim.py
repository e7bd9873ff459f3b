"""GPU tier: vvhip::DeblockOps (the shim's entry to vvhip_deblock) on host planes — a 3 x 2-CTU 4:2:0 picture uploaded unfiltered and filtered band by band, top to
bottom, then downloaded — against the reference's own results in tests/golden/deblock.npz.  end before every band was issued returns false; bands come in order, each
once.  tests/cpp/deblock_shim_driver.cpp is compiled here against the built shim."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import deblock_cases as DC  # noqa: E402
import deblock_ref as DR  # noqa: E402


def test_shim_deblock_band_by_band_equals_the_fixture(tmp_path):
    exe = str(tmp_path / "deblock_shim_driver")
    subprocess.check_call(["g++", "-std=c++14", "-O1", "-Wall", "-o", exe, os.path.join(ROOT, "tests", "cpp", "deblock_shim_driver.cpp"), "-L" + os.path.join(ROOT, "vvenc_amd"),
                           "-lvvenc_hip_shim", "-lvvenc_hip", "-Wl,-rpath," + os.path.join(ROOT, "vvenc_amd"), "-Wl,-rpath,/opt/rocm/lib"])
    golden = np.load(DR.GOLDEN)
    c = DC.cases()["g136"]
    assert (-(-c.width // c.ctu), c.ctu_rows) == (3, 2) and all(cl == (0, (1 << c.bit_depth) - 1) for cl in c.clip) and any(c.beta_offsets) and any(c.tc_offsets)
    rng = np.random.default_rng(241)
    strides, dst_strides, lfp_stride = (141, 75, 68), (136, 71, 80), c.width // 4 + 3      # odd pitches among them; a map pitch larger than the picture's
    with open(tmp_path / "pic.bin", "wb") as f:
        f.write(np.array([c.width, c.height, c.bit_depth, c.ctu, *strides, *dst_strides, lfp_stride, *c.beta_offsets, *c.tc_offsets], np.int32).tobytes())
        for k, p in enumerate(c.planes):
            h, w = p.shape
            wide = rng.integers(0, 1 << c.bit_depth, (h, strides[k])).astype(np.int16)      # what lies between the rows must not matter
            wide[:, :w] = p
            f.write(wide.tobytes())
        for m in (c.lfp_ver, c.lfp_hor):
            wide = np.frombuffer(rng.integers(0, 256, m.shape[0] * lfp_stride * 6, dtype=np.uint8).tobytes(), DR.LF_PARAM_DTYPE).reshape(m.shape[0], lfp_stride).copy()
            wide[:, :m.shape[1]] = m      # records beyond width / 4 are never read, whatever they hold
            f.write(wide.tobytes())
    r = subprocess.run([exe, str(tmp_path)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stderr)
    assert open(tmp_path / "flow.txt").read().count("\n") == 4
    for k, p in enumerate(c.planes):
        h, w = p.shape
        got = np.fromfile(tmp_path / ("dst%d.bin" % k), np.int16).reshape(h, dst_strides[k])
        assert np.array_equal(got[:, :w], p + golden["g136_d%d" % k]), k
        assert (got[:, w:] == -7).all(), (k, "the pitch padding of the destination was written")
