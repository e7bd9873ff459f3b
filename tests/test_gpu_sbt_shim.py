"""GPU tier: vvhip::SbtOps::codeList (the shim's entry to vvhip_sbt_parts_batch -> vvhip_tu_rdo_multi_strided -> vvhip_sbt_place_batch) on host blocks — the chain's CUs
with strided host blocks and two candidates each, at QPs where some tiles quantise to zero — against the Python chain HotPath.tu_rdo_sbt on the same CUs and against
tests/sbt_ref.py around the oracle's TU pipeline.  tests/cpp/sbt_shim_driver.cpp is compiled here against the built shim."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import sbt_cases as SC  # noqa: E402
import sbt_ref as SR  # noqa: E402


def test_shim_sbt_chain_equals_the_python_chain_and_the_model(tmp_path, oracle):
    import torch
    from vvenc_amd.hotpath import HotPath, STATS_DTYPE
    exe = str(tmp_path / "sbt_shim_driver")
    subprocess.check_call(["g++", "-std=c++14", "-O1", "-Wall", "-o", exe, os.path.join(ROOT, "tests", "cpp", "sbt_shim_driver.cpp"), "-L" + os.path.join(ROOT, "vvenc_amd"),
                           "-lvvenc_hip_shim", "-lvvenc_hip", "-Wl,-rpath," + os.path.join(ROOT, "vvenc_amd"), "-Wl,-rpath,/opt/rocm/lib"])
    world = SC.chain_world()
    L, cand, bd, irap, thr, cw = world["listed"], world["candidates"], world["bd"], 0, 8, SC.WEIGHTS[3]
    qps = SC.CHAIN_QPS[1]
    rng = np.random.default_rng(606)
    with open(tmp_path / "cus.bin", "wb") as f:
        f.write(np.array([len(L.items), len(cand), bd, irap, thr], np.int32).tobytes() + np.float64(cw).tobytes())
        pads = [(0, 3, 8)[k % 3] for k in range(len(L.items))]
        for k, it in enumerate(L.items):
            w, h = int(it["width"]), int(it["height"])
            f.write(np.array([w, h, w + pads[k], w // 2 + pads[k], int(it["sbt_allowed"])], np.int32).tobytes())
        for (cu, mode) in cand:
            f.write(np.array([cu, mode, qps[0], qps[1], qps[2]], np.int32).tobytes())
        for k, blocks in enumerate(L.blocks):
            for b in blocks:
                wide = rng.integers(-999, 1000, (b.shape[0], b.shape[1] + pads[k])).astype(np.int16)      # what lies between the rows must not matter
                wide[:, :b.shape[1]] = b
                f.write(wide.tobytes())
    r = subprocess.run([exe, str(tmp_path)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    parts, est = np.fromfile(tmp_path / "parts.bin", np.uint64).reshape(-1, 3, 16), np.fromfile(tmp_path / "est.bin", np.uint64).reshape(-1, 9)
    order = np.fromfile(tmp_path / "order.bin", np.uint8).reshape(-1, 8)
    sse, again = (np.fromfile(tmp_path / name, np.uint64).reshape(-1, 3) for name in ("sse.bin", "again.bin"))
    levels, rec = (np.fromfile(tmp_path / name, np.int16) for name in ("levels.bin", "rec.bin"))
    stats = np.fromfile(tmp_path / "stats.bin", STATS_DTYPE).reshape(-1, 3)
    # ---- the Python chain on the same CUs
    hp = HotPath()
    d_resi = torch.from_numpy(L.resi).to(hp.device)
    p_parts, p_est, p_order, p_rec, p_sse, p_level, p_stats = hp.tu_rdo_sbt(d_resi, L.items, cand, qps, cw, bd, irap, thr)
    torch.cuda.synchronize()
    place = hp.last_sbt_place
    p_rec, p_level, p_st = p_rec.cpu().numpy(), p_level.cpu().numpy(), p_stats.cpu().numpy().view(STATS_DTYPE).reshape(-1)
    assert np.array_equal(parts, p_parts.cpu().numpy().view(np.uint64)) and np.array_equal(est, p_est.cpu().numpy().view(np.uint64)) and np.array_equal(order, p_order.cpu().numpy())
    assert np.array_equal(sse, p_sse.cpu().numpy().view(np.uint64)) and np.array_equal(again, sse)
    ep, ee, eo = SC.expected_parts(L, cw)
    assert np.array_equal(parts, ep) and np.array_equal(est, ee) and np.array_equal(order, eo)
    exp = SC.chain_expected(oracle, world, qps, irap)
    at_rec = at_lev = n_zero = 0
    seen = {}
    for k, ((cu, mode), comps) in enumerate(zip(cand, exp)):
        plane = seen.get(cu, 0)
        seen[cu] = plane + 1
        for c, e in enumerate(comps):
            what = (k, cu, mode, c)
            h, w = L.blocks[cu][c].shape
            x, y, tw, th = e["tile"]
            got = stats[k][c]
            assert got.tobytes() == p_st[int(place[k]["stats_idx"][c])].tobytes(), ("stats against the Python chain",) + what
            assert (int(got["abs_sum"]), int(got["last_scan_pos"]), int(got["need_rdoq"]), int(got["sse"])) == tuple(e["stats"][f] for f in ("abs_sum", "last_scan_pos", "need_rdoq", "sse")), ("stats",) + what
            lev = levels[at_lev:at_lev + tw * th].reshape(th, tw)
            assert np.array_equal(lev, e["level"]), ("levels",) + what
            if e["stats"]["abs_sum"]:
                o = int(place[k]["tile_off"][c])
                assert np.array_equal(p_level[o:o + tw * th].reshape(th, tw), lev), ("levels against the Python chain",) + what
            blk = rec[at_rec:at_rec + w * h].reshape(h, w)
            assert np.array_equal(blk, e["placed"]) and np.array_equal(blk, L.view(p_rec[plane], cu, c)), ("reconstruction",) + what
            assert int(sse[k][c]) == e["sse"], ("sse",) + what
            n_zero += e["stats"]["abs_sum"] == 0
            at_rec += w * h
            at_lev += tw * th
    assert at_rec == rec.size and at_lev == levels.size and 0 < n_zero < 3 * len(cand)
