#!/usr/bin/env python3
"""Times the intra luma mode pre-selection entry (vvenc_amd/csrc/intra.hip) on a synthetic list shaped like an intra picture of 1920x1080, 10 bit, reference line 0, all 67
modes per block:

  (a) costs     the entry with full masks, costs only
  (b) best3     the entry with full masks and the predictions of each block's three cheapest modes written
  (c) unfused   the entry writing ALL predictions, then the existing vvhip_dist_batch with HAD_2SAD on ( original, prediction ) pairs, one call per block shape — what the
                pair of existing-style entries (a predictor that writes, a distortion list that reads) would cost; its costs must equal (a)'s

list   : no recorded intra picture's block list is at hand (vvenc_amd/recorded.py holds inter pictures' table calls, not intra TU lists), so the mix is STATED, by share of the
         picture's area: 64x64 10 %, 32x32 25 %, 16x16 28 %, 8x8 14 %, 4x4 3 %, 32x8 and 8x32 4 % each, 16x4, 4x16, 8x4, 4x8 2 % each, 32x4, 4x32, 64x4, 4x64 1 % each —
         about 15 500 blocks, 1.04 million ( block, mode ) pairs.  Lines and originals: tests/intra_cases.seeded (smooth plus noise).
check  : before anything is timed, 45 blocks of the list (three per shape) are compared with tests/intra_ref.py, and (c)'s costs with (a)'s on the whole list.
time   : device = events around one workload issued behind ~2 ms of other work on the stream (the upload of the item list included, the host not);
         call   = `reps` back-to-back runs between two host clock readings that end in a device synchronise.  `rounds` times each, the workloads alternating inside a round;
         medians, minima, spread ( max - min ) / median.
usage: tools/intra_time.py [--rounds 9] [--reps 5] [--json out.json] [--quick]"""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402

BD, WIDTH, HEIGHT = 10, 1920, 1080
MIX = (((64, 64), .10), ((32, 32), .25), ((16, 16), .28), ((8, 8), .14), ((4, 4), .03), ((32, 8), .04), ((8, 32), .04), ((16, 4), .02), ((4, 16), .02), ((8, 4), .02), ((4, 8), .02),
       ((32, 4), .01), ((4, 32), .01), ((64, 4), .01), ((4, 64), .01))


def picture_cases(variants=24):
    """the list as tests/intra_cases.Case objects: per shape `variants` distinct seeded blocks, repeated to the shape's count (the kernel does not know)"""
    import intra_cases as IC
    out = []
    for k, ((w, h), share) in enumerate(MIX):
        n = int(round(share * WIDTH * HEIGHT / (w * h)))
        pool = [IC.Case("t%dx%d_%d" % (w, h, v), w, h, BD, 0, *IC.seeded(np.random.default_rng(9000 + 100 * k + v), w, h, BD, 0), IC.ALL_MODES, ()) for v in range(min(variants, n))]
        out += [pool[i % len(pool)] for i in range(n)]
    return out


def picture_blocks():
    """the list in the form tests/intra_golden_gen.py hands to the reference's generator: ( w, h, bit_depth, mri, modes, lines, org )"""
    return [(c.w, c.h, c.bit_depth, c.mri, c.modes, c.lines, c.org) for c in picture_cases()]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--json")
    ap.add_argument("--quick", action="store_true")
    args = ap.parse_args()
    import torch
    import intra_cases as IC
    import intra_ref as IR
    from vvenc_amd.hotpath import DF, HotPath
    hp = HotPath()
    rounds, reps = (1, 2) if args.quick else (args.rounds, args.reps)
    cl = picture_cases()
    items, ref, org, _ = IC.as_list(cl, pred="none")
    dref, dorg = torch.from_numpy(ref).to(hp.device), torch.from_numpy(org).to(hp.device)
    n, pairs = len(cl), len(cl) * IR.NUM_MODES
    cost_a = torch.zeros((n, IR.NUM_MODES), dtype=torch.int32, device=hp.device)
    hp.intra_luma_modes(items, dref, dorg, cost=cost_a, pred=None)
    hp.sync()
    ca = cost_a.cpu().numpy().astype(np.uint32)
    first = {}
    for i, c in enumerate(cl):
        first.setdefault((c.w, c.h), []).append(i)
    for idx in first.values():
        for i in idx[:3]:
            assert np.array_equal(ca[i], IC.expected(cl[i])[0]), cl[i].name
    print("check: %d blocks of the list equal the model" % (3 * len(first)))
    # (b) the three cheapest modes of every block
    items_b = items.copy()
    best = np.argsort(ca, axis=1, kind="stable")[:, :3]
    at = 0
    for i in range(n):
        items_b[i]["pred_mask"] = IR.make_mask(best[i].tolist())
        items_b[i]["pred_off"] = at
        at += 3 * int(items[i]["w"]) * int(items[i]["h"])
    pred_b = torch.zeros(at, dtype=torch.int16, device=hp.device)
    cost_b = torch.zeros_like(cost_a)
    # (c) every prediction written, then the distortion list per shape
    items_c = items.copy()
    at = 0
    for i in range(n):
        items_c[i]["pred_mask"] = items[i]["mode_mask"]
        items_c[i]["pred_off"] = at
        at += IR.NUM_MODES * int(items[i]["w"]) * int(items[i]["h"])
    pred_c = torch.zeros(at, dtype=torch.int16, device=hp.device)
    cost_c = torch.zeros_like(cost_a)
    dist_calls = []
    for (w, h), idx in first.items():
        di = np.zeros((len(idx) * IR.NUM_MODES, 2), np.int32)
        for j, i in enumerate(idx):
            di[j * IR.NUM_MODES:(j + 1) * IR.NUM_MODES, 0] = int(items_c[i]["org_off"])
            di[j * IR.NUM_MODES:(j + 1) * IR.NUM_MODES, 1] = int(items_c[i]["pred_off"]) + np.arange(IR.NUM_MODES) * w * h
        dist_calls.append((w, h, idx, torch.from_numpy(di).to(hp.device), torch.zeros(len(di), dtype=torch.int64, device=hp.device)))

    def run_a():
        hp.intra_luma_modes(items, dref, dorg, cost=cost_a, pred=None)

    def run_b():
        hp.intra_luma_modes(items_b, dref, dorg, cost=cost_b, pred=pred_b)

    def run_c():
        hp.intra_luma_modes(items_c, dref, dorg, cost=cost_c, pred=pred_c)
        for (w, h, idx, di, do) in dist_calls:
            hp._ck(hp.L.vvhip_dist_batch(hp.ctx, DF["HAD_2SAD"], C.c_void_p(dorg.data_ptr()), w, C.c_void_p(pred_c.data_ptr()), w, w, h, 0, BD, C.c_void_p(di.data_ptr()), di.shape[0],
                                         C.c_void_p(do.data_ptr())))

    fns = {"costs": run_a, "best3": run_b, "unfused": run_c}
    for fn in fns.values():
        fn()
    hp.sync()
    assert np.array_equal(cost_b.cpu().numpy(), cost_a.cpu().numpy()) and np.array_equal(cost_c.cpu().numpy(), cost_a.cpu().numpy())
    for (w, h, idx, di, do) in dist_calls:
        assert np.array_equal(do.cpu().numpy().reshape(len(idx), IR.NUM_MODES), ca[idx].astype(np.int64)), (w, h)
    print("check: the unfused chain's %d costs equal the entry's" % pairs)
    busy = torch.zeros(64 << 20, dtype=torch.int16, device=hp.device)
    t_call, t_dev = ({k: [] for k in fns} for _ in range(2))
    for _ in range(rounds):
        for k, fn in fns.items():
            t0 = time.perf_counter()
            for _ in range(reps):
                fn()
            hp.sync()
            t_call[k].append((time.perf_counter() - t0) / reps * 1e6)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            for _ in range(32):
                busy.add_(1)
            e0.record()
            fn()
            e1.record()
            hp.sync()
            t_dev[k].append(e0.elapsed_time(e1) * 1e3)
    out = {"bit_depth": BD, "width": WIDTH, "height": HEIGHT, "blocks": n, "pairs": pairs, "rounds": rounds, "reps": reps,
           "written_MB": {"costs": 0.0, "best3": pred_b.numel() * 2 / 1e6, "unfused": pred_c.numel() * 2 / 1e6}}
    for k in fns:
        v, dv = np.array(t_call[k]), np.array(t_dev[k])
        out[k] = {"call_median_us": float(np.median(v)), "call_min_us": float(v.min()), "call_spread": float((v.max() - v.min()) / np.median(v)),
                  "device_median_us": float(np.median(dv)), "device_min_us": float(dv.min()), "device_spread": float((dv.max() - dv.min()) / np.median(dv))}
        print("%-8s blocks %5d pairs %7d  call median %9.1f us (min %9.1f, spread %5.1f %%)  device %9.1f us (min %9.1f, spread %5.1f %%)  predictions written %7.2f MB"
              % (k, n, pairs, out[k]["call_median_us"], v.min(), 100 * out[k]["call_spread"], out[k]["device_median_us"], dv.min(), 100 * out[k]["device_spread"], out["written_MB"][k]))
    if args.json:
        with open(args.json, "w") as f:
            json.dump(out, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
