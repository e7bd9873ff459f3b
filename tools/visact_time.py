#!/usr/bin/env python3
"""Times the visual-activity entry (vvenc_amd/csrc/visact.hip) on the area lists of two pictures, 4:2:0, 10 bit, CTU 128, first and second order:

  hd     1920x1080: the HD form — 135 CTU areas with a guard frame of 1 sample and their mean rectangles, then the three whole planes
  uhd    3840x2160: the down-sampling form on luma (guard frame 2), the HD form on the two 4:2:0 chroma planes — 510 CTU areas, then the three whole planes
  read   a plain device read of the same planes (torch: the sum of every plane the list reads), the yardstick the entry's device time is given as a multiple of

lists  : HotPath.visact_picture_areas — the reference's own list (BitAllocation.cpp:553-573, :610-616).  Every luma sample is read by its CTU's area, by the whole-plane
         area and (a guard frame's worth) by the neighbours: the entry reads the picture about twice.
check  : before anything is timed the entry is compared with tests/visact_ref.py on the 1920x1080 list (numpy, a few seconds).
time   : call   = `reps` back-to-back calls between two host clock readings that end in a device synchronise; the entry waits for the launch that still reads its tile list
                  before it refills it, so back-to-back calls do not overlap
         host   = one call on an idle device, the host clock around the call alone: validation, the cut into tiles, the enqueue of the upload and of the two launches
         device = events around one call issued behind ~2 ms of other work on the stream: the upload of the tile list plus the two launches, without the host
         `rounds` times each, the variants alternating inside a round; medians, minima, spread ( max - min ) / median.
usage: tools/visact_time.py [--rounds 9] [--reps 20] [--json out.json] [--quick]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402

BD, CTU = 10, 128
SIZES = {"hd": (1920, 1080, False), "uhd": (3840, 2160, True)}


def pictures():
    """label -> ( tests/visact_cases.Picture, { order: area list } )"""
    import visact_cases as VC
    import visact_ref as VR
    out = {}
    for label, (w, h, high_res) in SIZES.items():
        rng = np.random.default_rng(6100 + w)
        pic = VC.Picture(label, BD, [VC.natural(rng, w >> s, h >> s, BD) for s in (0, 1, 1)])
        out[label] = (pic, {o: VR.picture_areas(VC.sizes(pic), CTU, high_res, o, "420") for o in (1, 2)})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--json")
    ap.add_argument("--quick", action="store_true")
    args = ap.parse_args()
    import torch
    import visact_ref as VR
    from vvenc_amd.hotpath import HotPath
    hp = HotPath()
    rounds, reps = (1, 3) if args.quick else (args.rounds, args.reps)
    out = {"bit_depth": BD, "ctu": CTU, "rounds": rounds, "reps": reps}
    busy = torch.zeros(64 << 20, dtype=torch.int16, device=hp.device)
    for label, (pic, lists) in pictures().items():
        dev = [[hp.plane(p) for p in row] for row in pic.rows]
        table = [(r[0], r[1], r[2], BD) for r in dev]
        assert all(np.array_equal(hp.visact_picture_areas([(r[0].width, r[0].height) for r in dev], CTU, SIZES[label][2], o, "420"), a) for o, a in lists.items())
        if label == "hd":
            got = hp.visact(table, lists[2]).cpu().numpy().view(np.uint64)
            assert np.array_equal(got, VR.records(pic.rows, lists[2]))
            print("check: the 1920x1080 list, second order, is the model's (%d areas)" % len(lists[2]))
        fns, read_bytes = {}, {}
        for o, areas in lists.items():
            fns["order%d" % o] = (lambda a=areas: hp.visact(table, a))
            fns["read%d" % o] = (lambda n=o: [p.storage.sum() for r in dev for p in r[:n + 1]])
            read_bytes[o] = sum(p.width * p.height * 2 for r in dev for p in r[:o + 1])
        for fn in fns.values():
            for _ in range(3):
                fn()
        hp.sync()
        t_call, t_host, t_dev = ({k: [] for k in fns} for _ in range(3))
        for _ in range(rounds):
            for k, fn in fns.items():
                t0 = time.perf_counter()
                for _ in range(reps):
                    fn()
                hp.sync()
                t_call[k].append((time.perf_counter() - t0) / reps * 1e6)
                t0 = time.perf_counter()
                fn()
                t_host[k].append((time.perf_counter() - t0) * 1e6)
                hp.sync()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                for _ in range(32):
                    busy.add_(1)
                e0.record()
                fn()
                e1.record()
                hp.sync()
                t_dev[k].append(e0.elapsed_time(e1) * 1e3)
        res = {"width": SIZES[label][0], "height": SIZES[label][1], "areas": len(lists[1])}
        for k in fns:
            o = int(k[-1])
            v, hst, dv = np.array(t_call[k]), np.array(t_host[k]), np.array(t_dev[k])
            med, yard = float(np.median(v)), float(np.median(t_dev["read%d" % o]))
            res[k] = {"call_median_us": med, "call_min_us": float(v.min()), "call_spread": float((v.max() - v.min()) / med), "host_median_us": float(np.median(hst)),
                      "device_median_us": float(np.median(dv)), "device_min_us": float(dv.min()), "plane_bytes": read_bytes[o], "device_over_read": float(np.median(dv)) / yard}
            print("%-3s %-6s areas %3d  call median %8.1f us (min %8.1f, spread %5.1f %%)  host %7.1f us  device %8.1f us (min %8.1f) = %5.2f x the plain read of %6.2f MB"
                  % (label, k, len(lists[o]), med, v.min(), 100 * res[k]["call_spread"], res[k]["host_median_us"], res[k]["device_median_us"], dv.min(), res[k]["device_over_read"], read_bytes[o] / 1e6))
        out[label] = res
    if args.json:
        with open(args.json, "w") as f:
            json.dump(out, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
