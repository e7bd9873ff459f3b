"""CPU tier: bench.py --dump-outputs (tools/bench_outputs.py).  Two recordings of the same encode hold the same calls in different orders (the recorder merges its worker
threads' logs as they come): list positions, pool offsets and the order of the reference planes differ.  The dump must not: the same work with the same results writes the
same arrays, whatever the order; a different result shows."""
import os
import subprocess
import sys
from types import SimpleNamespace

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

PLANES = [(0, 8, 0), (0, 8, 1), (0, 8, 2), (1, 0, 0), (1, 16, 0)]          # (kind, poc, comp): originals Y / Cb / Cr, two reference pictures


def _work(seed=3):
    """one picture's work in logical form: every entry carries its inputs (pool blocks as sample arrays) and its result"""
    rng = np.random.default_rng(seed)
    blk = lambda n: rng.integers(-512, 512, n).astype(np.int16)
    w = {"int": [], "stage": [], "item": [], "mask": [], "tu": [], "dmvr": []}
    for k in range(6):
        pattern = blk(16 * 8) if k % 3 == 0 else None
        w["int"].append(dict(org=pattern, org_off=40 * k, ref=3 + k % 2, ref_off=100 + 7 * k, w=16, h=8, ss=k % 2,
                             cands=[(int(rng.integers(-8, 8)), int(rng.integers(-8, 8)), int(rng.integers(1, 1 << 40))) for _ in range(1 + k % 4)]))
        w["stage"].append(dict(org=pattern, org_off=40 * k, ref=3 + k % 2, ref_off=90 + 5 * k, w=16, h=8, mask=0b101010101 | k,
                               cost=rng.integers(1, 1 << 30, 9)))
    for k in range(7):
        w["item"].append(dict(org=blk(8 * 4) if k % 2 else None, org_off=12 * k, cur=3 + k % 2, cur_off=300 + k, w=8, h=4, func=k % 3, cost=int(rng.integers(1, 1 << 30))))
    for k in range(3):
        w["mask"].append(dict(org_off=8 * k, cur=3, cur_off=50 + k, mask=blk(8 * 8), w=8, h=8, cost=int(rng.integers(1, 1 << 30))))
    for (tw, th) in ((4, 4), (8, 4)):
        for k in range(5):
            lv = rng.integers(-9, 9, tw * th).astype(np.int16) * (k % 2)
            w["tu"].append(dict(w=tw, h=th, res=blk(tw * th), qp=30 + k, flag=k % 2, level=lv, rec=rng.integers(-99, 99, tw * th).astype(np.int16),
                                stats=(int(np.abs(lv).sum()), int(rng.integers(0, 15)), k % 2, int(rng.integers(0, 1 << 40)))))
    for k in range(4):
        w["dmvr"].append(dict(r0=3, r1=4, off0=10 * k, off1=11 * k, frac=(k, 0, 0, k), res=(k - 2, 1, int(rng.integers(0, 1 << 20)))))
    return w


def _lists(work, order_seed):
    """the work as RecordedLists-shaped host lists + the raw outputs in list order, laid out in an order set by order_seed"""
    from vvenc_amd.replay import ME_CAND, ME_INT_JOB, ME_ITEM, ME_MASK_ITEM, ME_STAGE_JOB
    from vvenc_amd.hotpath import DMVR_ITEM_DTYPE, DMVR_RESULT_DTYPE, STATS_DTYPE
    rng = np.random.default_rng(order_seed)
    refs = [3, 4] if order_seed % 2 else [4, 3]                              # reference plane index of logical plane 3 / 4
    pidx = lambda p: p if p < 3 else refs[p - 3]
    planes = np.zeros(len(PLANES), [("kind", "<i4"), ("poc", "<i4"), ("comp", "<i4")])
    for i, p in enumerate(PLANES):
        planes[pidx(i)] = p
    pool, pool_index = [np.zeros(int(rng.integers(0, 16)), np.int16)], len(PLANES)

    def put(b):
        off = sum(x.size for x in pool)
        pool.extend([b, np.zeros(int(rng.integers(0, 8)), np.int16)])
        return off

    perm = lambda n: rng.permutation(n)
    L = SimpleNamespace(pic=SimpleNamespace(planes=planes), n_pic_planes=len(PLANES), pool_index=pool_index)
    ints = [work["int"][i] for i in perm(len(work["int"]))]
    jobs, pc, cand_out = np.zeros(len(ints), ME_INT_JOB), [], []
    for i, j in enumerate(ints):
        cands = [j["cands"][c] for c in perm(len(j["cands"]))]
        jobs[i] = (put(j["org"]) if j["org"] is not None else j["org_off"], j["ref_off"], j["w"], j["h"], pool_index if j["org"] is not None else 0, pidx(j["ref"]), j["ss"], 0,
                   0, 0, 0, 0, len(pc), len(cands))
        pc += [(dx, dy) for dx, dy, _ in cands]
        cand_out += [c for _, _, c in cands]
    L.int_jobs, L.plan_cands = jobs, np.array(pc, ME_CAND)
    sts = [work["stage"][i] for i in perm(len(work["stage"]))]
    L.stage_jobs = np.zeros(len(sts), ME_STAGE_JOB)
    for i, s in enumerate(sts):
        L.stage_jobs[i] = (put(s["org"]) if s["org"] is not None else s["org_off"], s["ref_off"], s["w"], s["h"], pool_index if s["org"] is not None else 0, pidx(s["ref"]),
                           2, 2, 0, 3, 0, 0, s["mask"], 0)
    L.stage_evaluated = np.array([[(s["mask"] >> b) & 1 == 1 for b in range(9)] for s in sts]).reshape(-1, 9)
    stage_out = np.array([s["cost"] for s in sts], np.uint64).reshape(-1)
    its = [work["item"][i] for i in perm(len(work["item"]))]
    L.items = np.zeros(len(its), ME_ITEM)
    for i, t in enumerate(its):
        L.items[i] = (put(t["org"]) if t["org"] is not None else t["org_off"], t["cur_off"], pool_index if t["org"] is not None else 0, pidx(t["cur"]), t["func"], 0, t["w"], t["h"])
    mks = [work["mask"][i] for i in perm(len(work["mask"]))]
    L.mask_items = np.zeros(len(mks), ME_MASK_ITEM)
    for i, m in enumerate(mks):
        L.mask_items[i] = (m["org_off"], m["cur_off"], put(m["mask"]), 0, pidx(m["cur"]), pool_index, 0, m["w"], m["h"], 0)
    item_out = np.array([t["cost"] for t in its] + [m["cost"] for m in mks], np.uint64)
    L.tu_groups, tu_out = [], []
    for (tw, th) in ((8, 4), (4, 4)) if order_seed % 2 else ((4, 4), (8, 4)):
        g = [t for t in work["tu"] if (t["w"], t["h"]) == (tw, th)]
        g = [g[i] for i in perm(len(g))]
        qf = np.array([(t["qp"], t["flag"]) for t in g], np.int16)
        L.tu_groups.append(dict(w=tw, h=th, tr_hor=0, tr_ver=0, n=len(g), qf=qf, off=np.array([put(t["res"]) for t in g], np.int32)))
        st = np.zeros(len(g), STATS_DTYPE)
        for i, t in enumerate(g):
            st[i]["abs_sum"], st[i]["last_scan_pos"], st[i]["need_rdoq"], st[i]["sse"] = t["stats"]
        junk = rng.integers(-999, 999, (len(g), tw * th)).astype(np.int16)            # sparse outputs: an all-zero TU's buffers are not written
        nz = st["abs_sum"] != 0
        tu_out.append({"stats": st, "level": np.where(nz[:, None], np.array([t["level"] for t in g]), junk).reshape(-1),
                       "rec": np.where(nz[:, None], np.array([t["rec"] for t in g]), junk).reshape(-1)})
    dms = [work["dmvr"][i] for i in perm(len(work["dmvr"]))]
    items = np.zeros(len(dms), DMVR_ITEM_DTYPE)
    res = np.zeros(len(dms), DMVR_RESULT_DTYPE)
    for i, d in enumerate(dms):
        items[i] = (d["off0"], d["off1"]) + d["frac"]
        res[i]["mvd_x"], res[i]["mvd_y"], res[i]["min_cost"] = d["res"]
    L.dmvr_groups = [dict(r0=pidx(3), r1=pidx(4), dx=8, dy=8, n=len(dms), items=items)]
    L.pool = np.concatenate(pool + [np.zeros(256, np.int16)])
    return L, {"cand": np.array(cand_out, np.uint64), "stage": stage_out, "item": item_out, "tu": tu_out, "dmvr": [res]}


def test_dump_does_not_depend_on_list_order(tmp_path):
    import bench_outputs as BO
    work = _work()
    a = BO.canonical(*_lists(work, 1))
    b = BO.canonical(*_lists(work, 2))
    assert set(a) == set(b) and a["me_integer_costs"].size == sum(len(j["cands"]) for j in work["int"]) and a["tu_levels"].size == 5 * 16 + 5 * 32
    for k in a:
        assert a[k].dtype in (np.float32, np.float64) and np.array_equal(a[k], b[k]), k
    # what the timed path returns, not what an all-zero TU's unwritten buffers hold
    assert sorted(a["tu_levels"].tolist()) == sorted(np.concatenate([t["level"] for t in work["tu"]]).astype(np.float32).tolist())
    shapes = BO.write(str(tmp_path / "d"), a)
    assert shapes["me_subpel_costs"] == [6, 9] and np.array_equal(np.load(str(tmp_path / "d" / "dmvr.npy")), a["dmvr"])
    assert sorted(os.listdir(str(tmp_path / "d"))) == sorted(k + ".npy" for k in a)
    # a class without work (no masked SADs, no DMVR) writes no file rather than an empty one
    del work["mask"][:], work["dmvr"][:]
    e = BO.canonical(*_lists(work, 1))
    assert e["masked_sad_costs"].size == 0 and e["dmvr"].size == 0
    shapes = BO.write(str(tmp_path / "e"), e)
    assert "masked_sad_costs" not in shapes and "dmvr" not in shapes and all(np.prod(v) > 0 for v in shapes.values())
    assert sorted(os.listdir(str(tmp_path / "e"))) == sorted(k + ".npy" for k in shapes)
    # one result changes -> the dump changes
    work["tu"][3]["rec"][0] += 1
    c = BO.canonical(*_lists(work, 2))
    assert not np.array_equal(a["tu_reconstruction"], c["tu_reconstruction"])


def test_dump_stays_within_its_budget(monkeypatch):
    import bench_outputs as BO
    work = _work()
    full = BO.canonical(*_lists(work, 1))
    monkeypatch.setattr(BO, "BUDGET_BYTES", sum(v.nbytes for v in full.values()) - 200)
    a, b = BO.canonical(*_lists(work, 1)), BO.canonical(*_lists(work, 2))
    assert "tu_sample" in a and 0 < a["tu_levels"].size < full["tu_levels"].size
    assert sum(v.nbytes for v in a.values()) <= BO.BUDGET_BYTES
    for k in a:
        assert np.array_equal(a[k], b[k]), k                 # (a fixed sample: the same rows every time)


def test_bench_options():
    """--steps, --warmup, --dump-outputs and --full are bench.py options (the plain run is the headline alone)"""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--help"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    for opt in ("--gpus", "--steps", "--warmup", "--dump-outputs", "--full"):
        assert opt in r.stdout, opt
