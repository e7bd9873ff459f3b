"""GPU tier: vvhip::InterPredOps::predictAffineList (the table-shaped shim's entry to vvhip_pred_affine_batch) on registered pictures — mirror lookup, offsets at the pictures'
own line pitch, luma with PROF and chroma, uni- and bi-predicted, CUs at the picture's edges, the residual — against tests/affine_ref.py; an unregistered plane is refused.
tests/cpp/pred_shim_affine_driver.cpp is compiled here against the built shim."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import affine_cases as AC  # noqa: E402
import affine_ref as AR  # noqa: E402
import pred_ref as PR  # noqa: E402


def test_shim_predict_affine_list(tmp_path, oracle):
    from oracle.oracle import RefLib
    lib = RefLib(1) if RefLib.available() else oracle
    exe = str(tmp_path / "pred_shim_affine_driver")
    subprocess.check_call(["g++", "-std=c++14", "-O1", "-Wall", "-o", exe, os.path.join(ROOT, "tests", "cpp", "pred_shim_affine_driver.cpp"), "-L" + os.path.join(ROOT, "vvenc_amd"),
                           "-lvvenc_hip_shim", "-lvvenc_hip", "-Wl,-rpath," + os.path.join(ROOT, "vvenc_amd"), "-Wl,-rpath,/opt/rocm/lib"])
    bd, ctu = 10, 32
    world = AC.World(bd, ctu, seed=606, pic_w=128, pic_h=96)
    rng = np.random.default_rng(606)
    recs, k = [], 0
    for (w, h) in ((8, 8), (16, 16), (32, 32), (16, 8), (8, 32), (32, 16)):
        for rep in range(2):
            x, y = 8 * int(rng.integers(0, (world.pic_w - w) // 8 + 1)), 8 * int(rng.integers(0, (world.pic_h - h) // 8 + 1))
            recs += AC._cu(rng, w, h, x, y, k & 1, (k >> 1) % 3, 1 + k % 3, 32)
            k += 1
    items, pos = AC.finish(world, recs)
    edge, epos = AC.edge_list(world, 7)
    items, pos = np.concatenate([items, edge[::3]]), pos + epos[::3]
    # the shim's offsets are relative to the picture's first sample, at the picture's line pitch; luma and chroma originals have different pitches: the luma blocks carry the residual
    lum = items["chroma"] == 0
    items, pos = np.concatenate([items[lum], items[~lum]]), [p for p, f in zip(pos, lum) if f] + [p for p, f in zip(pos, lum) if not f]
    off, total = AC.compact_offsets(items)
    items["dst_off"] = off
    m = world.m
    planes = [world.np[0][:-1], world.np[1][:-1], world.np[2][:-1], world.np[3][:-1], world.org_np[0][:-1]]          # (the registered pictures have no spare row)
    dims = [(128, 96, m), (128, 96, m), (64, 48, m // 2), (64, 48, m // 2), (128, 96, m)]
    for k in range(len(items)):
        c = int(items[k]["chroma"])
        st = planes[2 if c else 0].shape[1]
        o = (int(items[k]["cu_y"]) >> c) * st + (int(items[k]["cu_x"]) >> c)
        items[k]["ref_off"] = [o if p >= 0 else 0 for p in items[k]["ref_plane"]]
        items[k]["org_off"] = int(items[k]["cu_y"]) * planes[4].shape[1] + int(items[k]["cu_x"])
    with open(tmp_path / "planes.bin", "wb") as f:
        f.write(np.int32(len(planes)).tobytes())
        for (w, h, mm), a in zip(dims, planes):
            f.write(np.array([w, h, mm, a.shape[1]], np.int32).tobytes())
            f.write(np.ascontiguousarray(a).tobytes())
    n_lum = int(lum.sum())
    for part, sel in (("luma", slice(0, n_lum)), ("chroma", slice(n_lum, len(items)))):
        sub = items[sel].copy()
        base = int(sub["dst_off"][0])
        sub["dst_off"] -= base
        elems = AC.compact_offsets(sub)[1]
        with open(tmp_path / "items.bin", "wb") as f:
            f.write(np.array([len(sub), elems, 4 if part == "luma" else -1, 4, world.pic_w, world.pic_h, ctu, 0], np.int32).tobytes())
            f.write(sub.tobytes())
        r = subprocess.run([exe, str(tmp_path), str(bd)], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr
        pred, resi = (np.fromfile(tmp_path / n, np.int16) for n in ("pred.bin", "resi.bin"))
        assert pred.size == elems and resi.size == elems
        for j in range(len(sub)):
            k = sel.start + j
            it = sub[j]
            c = int(it["chroma"])
            bw, bh, o = int(it["cu_w"]) >> c, int(it["cu_h"]) >> c, int(it["dst_off"])
            e = AR.expected_block(lib, world.np, pos[k], items[k], bd, world.pic_w, world.pic_h, ctu)
            assert np.array_equal(pred[o:o + bw * bh].reshape(bh, bw), e), ("pred", part, j, it)
            if part == "luma":
                x, y = world.block_pos(it)
                assert np.array_equal(resi[o:o + bw * bh].reshape(bh, bw), PR.residual(world.org_np[0][y:y + bh, x:x + bw], e)), ("resi", j, it)
