"""GPU tier: vvhip::MergeMmvdOps (the shim's entry to vvhip_merge_mmvd_costs_batch) on host pictures shaped like the reference's — reference planes and the original inside
registered pictures with a margin and their own line pitch, base vectors given as MergeCtx holds them ( vectors, the reference picture's plane, POC and long-term flag ) —
against the model, tolerance 0.  tests/cpp/mmvd_shim_driver.cpp is compiled here against the built shim, once."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import mmvd_cases as MC  # noqa: E402

CUR_POC = 16


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("mmvd_shim") / "mmvd_shim_driver")
    subprocess.check_call(["g++", "-std=c++14", "-O1", "-Wall", "-o", path, os.path.join(ROOT, "tests", "cpp", "mmvd_shim_driver.cpp"), "-L" + os.path.join(ROOT, "vvenc_amd"),
                           "-lvvenc_hip_shim", "-lvvenc_hip", "-Wl,-rpath," + os.path.join(ROOT, "vvenc_amd"), "-Wl,-rpath,/opt/rocm/lib"])
    return path


@pytest.mark.parametrize("group", [("small", 10, "HAD", 0), ("small", 12, "HAD_fast", 0), ("small", 8, "HAD_fast", 1)], ids=lambda g: "%s_%d_%s_%d" % g)
def test_shim_mmvd_equals_the_model(exe, tmp_path, oracle, group):
    rng = np.random.default_rng(61)
    cl = [c for c in MC.cases() if c["group"] == group] + [MC.random_cu(rng, "r%d" % k, group, 32, 12) for k in range(6)]
    pw, ph, ctu, m = MC.GEOMS[group[0]]
    refs, org = MC.planes(group[0], group[1])
    stride = pw + 2 * m + 8
    hdr = np.array([len(cl), pw, ph, ctu, m, stride, group[1], CUR_POC, group[3], int(group[2] == "HAD_fast"), MC.N_REF], np.int32)
    parts = [hdr.tobytes()]
    for p in list(refs) + [org]:
        a = rng.integers(0, 1 << group[1], (ph + 2 * m, stride)).astype(np.int16)          # what lies beyond the plane's width must not matter
        a[:, :pw + 2 * m] = p
        parts.append(a.tobytes())
    for c in cl:
        rec = [c["cu_x"], c["cu_y"], c["w"], c["h"]] + [int(v) - (1 << 32) if int(v) >= 1 << 31 else int(v) for v in c["mask"]]
        for bs in c["bases"]:
            rec += [bs["mv"][0][0], bs["mv"][1][0], bs["mv"][0][1], bs["mv"][1][1], bs["ref"][0], bs["ref"][1], CUR_POC + bs["poc"][0], CUR_POC + bs["poc"][1], bs["lt"][0], bs["lt"][1],
                    bs["bcw"], bs["alt"]]
        parts.append(np.array(rec, np.int32).tobytes())
    with open(tmp_path / "list.bin", "wb") as f:
        f.write(b"".join(parts))
    r = subprocess.run([exe, str(tmp_path)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stderr)
    assert open(tmp_path / "flow.txt").read().count("\n") == 5
    want = MC.expected_group(oracle, group, cl)
    req = want != MC.SENTINEL
    want[~req] = 0
    cost = np.fromfile(tmp_path / "cost.bin", np.uint32).reshape(len(cl), 64)
    assert req.sum() > 100 and np.array_equal(cost, want), np.argwhere(cost != want)[:6].tolist()
