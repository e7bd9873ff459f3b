"""GPU tier: vvhip::IntraChromaOps (the shim's entry to vvhip_intra_chroma_modes_batch) on host buffers shaped like the reference's — the two unfiltered reference buffers at
their own pitch, the originals at a picture pitch, the blocks' luma windows inside one pitched luma plane — against the reference's own results recorded in
tests/golden/intra_chroma.npz, and its selection helper's sorted list and disabled set for both values of m_reduceIntraChromaModesFullRD.
tests/cpp/intra_chroma_shim_driver.cpp is compiled here against the built shim, once."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import intra_chroma_cases as CC  # noqa: E402
import intra_chroma_ref as CR  # noqa: E402

NAMES = ("s8x8", "s4x4", "s8x4", "s16x4", "s4x32", "s32x4", "s32x8", "s16x16", "a0_4x16", "a1_32x4", "vabove0_8x8", "vleft1_16x4", "vnone1_4x4", "r1_16x4", "r3_8x16", "b8_8x8", "b12_8x16",
         "ptwo_level_16x16", "psteep_neg_8x4", "povershoot_4x4", "s32x32")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("intra_chroma_shim") / "intra_chroma_shim_driver")
    subprocess.check_call(["g++", "-std=c++14", "-O1", "-Wall", "-o", path, os.path.join(ROOT, "tests", "cpp", "intra_chroma_shim_driver.cpp"), "-L" + os.path.join(ROOT, "vvenc_amd"),
                           "-lvvenc_hip_shim", "-lvvenc_hip", "-Wl,-rpath," + os.path.join(ROOT, "vvenc_amd"), "-Wl,-rpath,/opt/rocm/lib"])
    return path


def test_shim_intra_chroma_equals_the_fixture(exe, tmp_path):
    golden = CC.load_golden()
    rng = np.random.default_rng(43)
    cases = [golden[n] for n in NAMES]
    # one luma plane: the windows below one another at varying horizontal positions, noise between them
    pw = max(c.luma.shape[1] for c, _, _, _ in cases) + 24
    stride, ph = pw + 8, sum(c.luma.shape[0] for c, _, _, _ in cases)
    plane = rng.integers(0, 1 << 12, (ph, stride)).astype(np.int16)
    blocks, want_cost, want_pred, masks, y0 = [], [], [], [], 0
    for k, (c, gcost, _, gpred) in enumerate(cases):
        x0 = 4 * (k % 5)
        plane[y0:y0 + c.luma.shape[0], x0:x0 + c.luma.shape[1]] = c.luma
        mm = c.mode_mask if k % 2 == 0 else int(rng.integers(1, 256)) | (0x10 if k == 0 else 0)
        stored = CR.mask_bits(c.pred_mask)
        pm = mm & c.pred_mask & (0xff if k % 3 else 0xa5)
        ref_stride, org_stride = (2 * c.w + 1 + 3 * (k % 3), 2 * c.w + 1 + 2 * (k % 2)), c.w + 8 * (k % 2)
        hdr = [c.w, c.h, c.bit_depth, int(bool(c.flags & CR.F_ABOVE)), int(bool(c.flags & CR.F_LEFT)), c.n_ar // 2, c.n_lb // 2, int(bool(c.flags & CR.F_FIRST_ROW)),
               int(bool(c.flags & CR.F_VER_COLLOCATED)), x0 + CC.ORG, y0 + CC.ORG, ref_stride[0], ref_stride[1], org_stride, mm, pm] + list(c.cand)
        parts = [np.array(hdr, np.int32).tobytes()]
        nt = 2 * c.w + 1
        for comp in (0, 1):
            ref = rng.integers(0, 1 << c.bit_depth, ref_stride[comp] + 2 * c.h + 1).astype(np.int16)          # what lies between the rows must not matter
            ref[:nt], ref[ref_stride[comp]:] = c.lines[comp][:nt], c.lines[comp][nt:]
            parts.append(ref.tobytes())
        for comp in (0, 1):
            org = rng.integers(0, 1 << c.bit_depth, (c.h, org_stride)).astype(np.int16)
            org[:, :c.w] = c.org[comp]
            parts.append(org.tobytes())
        blocks.append(b"".join(parts))
        wc = np.zeros(CR.NUM_SLOTS, np.uint32)
        for s in CR.mask_bits(mm):
            wc[s] = gcost[s]
        want_cost.append(wc)
        want_pred += [gpred[stored.index(s)][comp].reshape(-1) for comp in (0, 1) for s in CR.mask_bits(pm)]
        masks.append(mm)
        y0 += c.luma.shape[0]
    with open(tmp_path / "list.bin", "wb") as f:
        f.write(np.array([len(NAMES), pw, ph, stride], np.int32).tobytes() + plane.tobytes() + b"".join(blocks))
    r = subprocess.run([exe, str(tmp_path)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stderr)
    assert open(tmp_path / "flow.txt").read().count("\n") == 4
    cost = np.fromfile(tmp_path / "cost.bin", np.uint32).reshape(len(NAMES), CR.NUM_SLOTS)
    assert np.array_equal(cost, np.stack(want_cost)), np.argwhere(cost != np.stack(want_cost))[:6].tolist()
    assert np.array_equal(np.fromfile(tmp_path / "pred.bin", np.int16), np.concatenate(want_pred))
    sel = np.fromfile(tmp_path / "sel.bin", np.uint8).reshape(len(NAMES), 2, 78)
    for k, (c, _, _, _) in enumerate(cases):
        for red in (0, 1):
            modes, disabled = CR.select(want_cost[k], c.cand, masks[k], red)
            assert sel[k, red, :8].tolist() == modes and set(np.flatnonzero(sel[k, red, 8:]).tolist()) == disabled and len(disabled) <= (4 if red else 2), (NAMES[k], red)
