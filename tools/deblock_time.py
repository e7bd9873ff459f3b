#!/usr/bin/env python3
"""Times the deblocking entry (vvenc_amd/csrc/deblock.hip) on one 1920x1080 4:2:0 10-bit picture at CTU 128 and CTU 64:

  whole        vvhip_deblock, the whole picture (three planes), both directions: one call, two launches
  bands        the same picture as one call per CTU row with both directions (what DeblockOps::band issues), top to bottom: 2 launches per row
  ver / hor    one direction alone, the whole picture: one launch each
  copy         a plain device copy of the three planes (torch), the yardstick the filter's time is given as a fraction of

picture: samples and legal maps from the case builder of the tests (tests/deblock_cases.make_case) at 1920x1080 — blocks of 4..CTU samples, bS / QP / lengths as there.
         The filter works in place, so call after call filters what the call before left: the decisions drift towards "nothing to do" (d >= beta is rarer, steps get
         smaller), the memory traffic and the number of segments looked at do not change.  The planes are restored before the device-time measurement.
check  : before anything is timed the entry is compared with tests/deblock_ref.py on the 264x136 case of the fixture (CTU 128, 12 bit) — the model in Python takes too long
         for the 1920x1080 picture — and on the 1920x1080 picture the band-by-band result is compared with the one-call result.
time   : call   = `reps` back-to-back calls between two host clock readings that end in a device synchronise: the larger of what the host needs to issue a call and what
                  the device needs to run it; the entry waits for the launch that still reads its record slot before it refills it, so back-to-back calls do not overlap
         host   = one call on an idle device, the host clock around the call alone: validation of the band's records, their conversion, the enqueue of the upload and
                  of the launches
         device = events around one call issued behind ~2 ms of other work on the stream, so that everything the call enqueues is waiting when the device gets to it:
                  the upload of the records plus the launches, without the host
         `rounds` times each, the variants alternating inside a round; medians, minima, spread ( max - min ) / median.
bytes  : what must move — the planes read and written once (2 x 6.22 MB) and the records uploaded (8 bytes per 4 x 4 luma unit and direction).  The picture fits the 256 MB
         last-level cache: the rates are rates out of that cache.
usage: tools/deblock_time.py [--rounds 9] [--reps 20] [--json out.json] [--quick]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402

W, H, BD = 1920, 1080, 10
HBM_PEAK = 8.0e12


def picture(ctu):
    """-> the 1920x1080 case at CTU size `ctu` (tests/deblock_cases.Case)"""
    import deblock_cases as DC
    return DC.make_case("hd%d" % ctu, 5000 + ctu, W, H, ctu, BD)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--json")
    ap.add_argument("--quick", action="store_true")
    args = ap.parse_args()
    import torch
    import deblock_cases as DC
    import deblock_ref as DR
    from vvenc_amd.hotpath import HotPath
    hp = HotPath()
    c = DC.cases()["g264"]
    dev = [hp.plane(p) for p in c.planes]
    hp.deblock(dev, c.lfp_ver, c.lfp_hor, c.ctu, c.bit_depth, clip=c.clip, beta_offsets=c.beta_offsets, tc_offsets=c.tc_offsets)
    want = DR.deblock(c.planes, c.lfp_ver, c.lfp_hor, c.ctu, c.bit_depth, c.clip, c.beta_offsets, c.tc_offsets)
    assert all(np.array_equal(d.visible().cpu().numpy(), w) for d, w in zip(dev, want))
    print("check: the 264x136 case at CTU 128 is the model's")
    rounds, reps = (1, 3) if args.quick else (args.rounds, args.reps)
    out = {"width": W, "height": H, "bit_depth": BD}
    busy = torch.zeros(64 << 20, dtype=torch.int16, device=hp.device)
    for ctu in (128, 64):
        pic = picture(ctu)
        gy = pic.ctu_rows
        plane_bytes = sum(p.size * 2 for p in pic.planes)
        rec_bytes = 2 * pic.lfp_ver.size * 8
        dev = [hp.plane(p) for p in pic.planes]
        keep = [d.storage.clone() for d in dev]
        other = [torch.empty_like(k) for k in keep]

        def restore():
            for d, k in zip(dev, keep):
                d.storage.copy_(k)

        def call(**kw):
            hp.deblock(dev, pic.lfp_ver, pic.lfp_hor, ctu, BD, **kw)

        call()
        whole = [d.visible().cpu().numpy() for d in dev]
        restore()
        for r in range(gy):
            call(rows=(r, 1))
        assert all(np.array_equal(d.visible().cpu().numpy(), w) for d, w in zip(dev, whole)) and any((w != p).any() for w, p in zip(whole, pic.planes))
        print("check: CTU %d: one-row bands top to bottom give the one-call result (%d luma samples changed)" % (ctu, int((whole[0] != pic.planes[0]).sum())))
        fns = {"whole": lambda: call(), "bands": lambda: [call(rows=(r, 1)) for r in range(gy)], "ver": lambda: call(dirs=1), "hor": lambda: call(dirs=2),
               "copy": lambda: [o.copy_(k) for o, k in zip(other, keep)]}
        launches = {"whole": 2, "bands": 2 * gy, "ver": 1, "hor": 1, "copy": 3}
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
                restore()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                for _ in range(32):
                    busy.add_(1)
                e0.record()
                fn()
                e1.record()
                hp.sync()
                t_dev[k].append(e0.elapsed_time(e1) * 1e3)
        res = {"ctu_rows": gy, "plane_bytes": plane_bytes, "record_bytes": rec_bytes, "launches": launches}
        copy_dev = float(np.median(t_dev["copy"]))
        for k in fns:
            moved = 2 * plane_bytes + (0 if k == "copy" else rec_bytes if k in ("whole", "bands") else rec_bytes // 2)
            v, hst, dv = np.array(t_call[k]), np.array(t_host[k]), np.array(t_dev[k])
            med = float(np.median(v))
            res[k] = {"call_median_us": med, "call_min_us": float(v.min()), "call_spread": float((v.max() - v.min()) / med), "host_median_us": float(np.median(hst)),
                      "device_median_us": float(np.median(dv)), "device_min_us": float(dv.min()), "bytes": moved, "device_bytes_per_s": moved / (float(np.median(dv)) * 1e-6),
                      "device_over_copy": float(np.median(dv)) / copy_dev}
            print("CTU %3d  %-6s launches %3d  call median %8.1f us (min %8.1f, spread %5.1f %%)  host %7.1f us  device %8.1f us (min %8.1f) = %5.2f x the copy; %6.2f MB -> %5.2f TB/s = %4.1f %% of the HBM peak"
                  % (ctu, k, launches[k], med, v.min(), 100 * res[k]["call_spread"], res[k]["host_median_us"], res[k]["device_median_us"], dv.min(), res[k]["device_over_copy"], moved / 1e6,
                     res[k]["device_bytes_per_s"] / 1e12, 100 * res[k]["device_bytes_per_s"] / HBM_PEAK))
        out["ctu%d" % ctu] = res
    out["rounds"], out["reps"] = rounds, reps
    if args.json:
        with open(args.json, "w") as f:
            json.dump(out, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
