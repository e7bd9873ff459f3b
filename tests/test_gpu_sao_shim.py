"""GPU tier: vvhip::SaoOps (the shim's entry to vvhip_sao_stats / vvhip_sao_offset) on host planes — the statistics of a 3 x 2-CTU 4:2:0 picture band by band, last
band first, then the offset filter of the picture from the planes the bands left in HBM — against the reference's own results in tests/golden/sao.npz.
statisticsEnd before every band was issued returns false; a band is taken once.  tests/cpp/sao_shim_driver.cpp is compiled here against the built shim."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import sao_cases as SC  # noqa: E402
import sao_ref as SR  # noqa: E402


def test_shim_sao_band_by_band_equals_the_fixture(tmp_path):
    exe = str(tmp_path / "sao_shim_driver")
    subprocess.check_call(["g++", "-std=c++14", "-O1", "-Wall", "-o", exe, os.path.join(ROOT, "tests", "cpp", "sao_shim_driver.cpp"), "-L" + os.path.join(ROOT, "vvenc_amd"),
                           "-lvvenc_hip_shim", "-lvvenc_hip", "-Wl,-rpath," + os.path.join(ROOT, "vvenc_amd"), "-Wl,-rpath,/opt/rocm/lib"])
    golden = np.load(SR.GOLDEN)
    ks = [n for n, _, _ in SC.stats_cases()].index("geo72/borders")
    ko = [n for n, _, _, _ in SC.offset_cases()].index("geo72/mixed")
    _, pic, prm, clip = SC.offset_cases()[ko]
    assert pic.grid == (3, 2) and all(c == (0, (1 << pic.bit_depth) - 1) for c in clip)
    rng = np.random.default_rng(239)
    strides = {"rec": (80, 43, 40), "org": (72, 36, 51), "dst": (77, 36, 48)}      # three pitches per plane kind, odd ones among them
    with open(tmp_path / "pic.bin", "wb") as f:
        f.write(np.array([pic.width, pic.height, pic.bit_depth, pic.ctu, *strides["rec"], *strides["org"], *strides["dst"]], np.int32).tobytes())
        for kind, planes in (("rec", pic.src), ("org", pic.org)):
            for c in range(3):
                h, w = planes[c].shape
                wide = rng.integers(0, 1 << pic.bit_depth, (h, strides[kind][c])).astype(np.int16)      # what lies between the rows must not matter
                wide[:, :w] = planes[c]
                f.write(wide.tobytes())
        f.write(np.ascontiguousarray(prm).tobytes())
    r = subprocess.run([exe, str(tmp_path)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stderr)
    assert open(tmp_path / "flow.txt").read().count("\n") == 4
    stats = np.fromfile(tmp_path / "stats.bin", np.int64).reshape(pic.n_ctus, 3, 5, 2, 32)
    assert np.array_equal(stats, golden["s%03d_rec" % ks])
    for c in range(3):
        h, w = pic.src[c].shape
        got = np.fromfile(tmp_path / ("dst%d.bin" % c), np.int16).reshape(h, strides["dst"][c])
        assert np.array_equal(got[:, :w], pic.src[c] + golden["o%03d_delta%d" % (ko, c)]), c
        assert (got[:, w:] == -7).all(), (c, "the pitch padding of the destination was written")
