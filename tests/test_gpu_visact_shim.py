"""GPU tier: vvhip::VisActOps (the shim's entry to vvhip_visact) on host planes with a line pitch of its own per pointer — the planes uploaded once, the list summed on them,
the records downloaded — against the reference's own results in tests/golden/visact.npz: the records, the VisAct fields (the doubles bit for bit) and getAvg of every area.
tests/cpp/visact_shim_driver.cpp is compiled here against the built shim, once."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import visact_cases as VC  # noqa: E402
import visact_ref as VR  # noqa: E402

RESULT = np.dtype([("rec", "<u8", 4), ("hp", "<u8", 3), ("int", "<u4", 4), ("avg", "<i8")])


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("visact_shim") / "visact_shim_driver")
    subprocess.check_call(["g++", "-std=c++14", "-O1", "-Wall", "-o", path, os.path.join(ROOT, "tests", "cpp", "visact_shim_driver.cpp"), "-L" + os.path.join(ROOT, "vvenc_amd"),
                           "-lvvenc_hip_shim", "-lvvenc_hip", "-Wl,-rpath," + os.path.join(ROOT, "vvenc_amd"), "-Wl,-rpath,/opt/rocm/lib"])
    return path


@pytest.mark.parametrize("name", list(VC.cases()))
def test_shim_visact_equals_the_fixture(exe, tmp_path, name):
    golden = np.load(VR.GOLDEN)
    c = VC.cases()[name]
    pic, rng = c.picture, np.random.default_rng(97)
    hdr, body = [len(pic.rows), pic.bit_depth, len(c.areas)], []
    for r, (cur, p1, p2) in enumerate(pic.rows):
        h, w = cur.shape
        strides = (w + 5, w + 11, w)
        hdr += [w, h, *strides, 1 | 2 | (4 if pic.same(r) else 0)]
        for p, s in zip((cur, None if pic.same(r) else p1, p2), strides):
            if p is not None:
                wide = rng.integers(0, 1 << pic.bit_depth, (h, s)).astype(np.int16)      # what lies between the rows must not matter
                wide[:, :w] = p
                body.append(wide.tobytes())
    with open(tmp_path / "pic.bin", "wb") as f:
        f.write(np.array(hdr, np.int32).tobytes() + b"".join(body) + np.ascontiguousarray(c.areas).tobytes())
    r = subprocess.run([exe, str(tmp_path)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stderr)
    assert open(tmp_path / "flow.txt").read().count("\n") == 4
    got = np.fromfile(tmp_path / "out.bin", RESULT)
    assert len(got) == len(c.areas)
    assert np.array_equal(got["rec"], golden[name + "_rec"]), (name, "records")
    assert np.array_equal(got["hp"], golden[name + "_hp"]), (name, "hpSpatAct, hpTempAct, hpVisAct bit patterns", np.argwhere(got["hp"] != golden[name + "_hp"])[:4].tolist())
    assert np.array_equal(got["int"], golden[name + "_int"]), (name, "spatAct, tempAct, minAct, visAct")
    assert np.array_equal(got["avg"], golden[name + "_avg"]), (name, "getAvg")
    if name == "mix10":      # the bypass is among them: a first-order area on the row whose prev1 is cur
        assert any(pic.same(int(a["plane"])) and a["order"] == 1 for a in c.areas)
