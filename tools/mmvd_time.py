#!/usr/bin/env python3
"""Times the MMVD merge-candidate entry (vvenc_amd/csrc/mmvd.hip) on a synthetic list shaped like the inter CUs of a 1920x1080 picture, 10 bit, CTU 128:

  (a) walk      the candidates a `fast`-preset walk can visit at most ( m_MMVD 3, MmvdDisNum 6: per base the four directions of step 0, then ONE direction of steps 1..5 —
                nine per base, the kept direction drawn per CU ), costs only
  (b) full      all 64 candidates of every CU, costs only
  (c) two       the same 64 candidates the long way: vvhip_pred_inter_batch_blend on items built with vvhip_mmvd_candidate — every prediction written to HBM — followed by
                vvhip_dist_multi with HAD_fast on ( original, prediction ) pairs; its costs must equal (b)'s

list   : CU sizes by share of the picture's area ( MIX below: a stated mix, no recorded picture's PU list is at hand without an encode ), positions on the CU grid, per CU two
         base vectors — uni-predicted from either list, bi-predicted with equal, scaled and mirrored POC distances, BCW on a quarter of the bi-predicted ones — with vectors of
         a few samples.  Planes: tests/mmvd_cases-style smooth fields plus noise, three references and the original.
check  : before anything is timed, (c)'s costs are compared with (b)'s on the whole list and (a)'s slots with (b)'s.
time   : device = events around one workload issued behind ~2 ms of other work on the stream (the upload of the list included, the host not);
         call   = `reps` back-to-back runs between two host clock readings that end in a device synchronise.  `rounds` times each, the workloads alternating inside a round;
         medians, minima, spread ( max - min ) / median.
usage: tools/mmvd_time.py [--rounds 9] [--reps 3] [--json out.json] [--quick]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402

WIDTH, HEIGHT, CTU, MARGIN, BD = 1920, 1080, 128, 144, 10
MIX = (((64, 64), .10), ((32, 32), .22), ((32, 16), .08), ((16, 32), .08), ((16, 16), .20), ((16, 8), .07), ((8, 16), .07), ((8, 8), .10), ((8, 4), .03), ((4, 8), .03), ((64, 32), .02))


def picture_list(rng):
    import mmvd_cases as MC
    MC.GEOMS["hd"] = (WIDTH, HEIGHT, CTU, MARGIN)
    group, out = ("hd", BD, "HAD_fast", 0), []
    for (w, h), share in MIX:
        for k in range(int(round(share * WIDTH * HEIGHT / (w * h)))):
            x, y = int(rng.integers(0, (WIDTH - w) // w + 1)) * w, int(rng.integers(0, (HEIGHT - h) // h + 1)) * h
            mv = lambda: (int(rng.integers(-80, 81)), int(rng.integers(-80, 81)))

            def rb():
                s = int(rng.integers(0, 5))
                ref = (int(rng.integers(0, MC.N_REF)), int(rng.integers(0, MC.N_REF)))
                if s == 0:
                    return MC.base(mv(), None, ref=ref)
                if s == 1:
                    return MC.base(None, mv(), ref=ref)
                return MC.base(mv(), mv(), ref=ref, poc=((-1, 1), (-2, -4), (4, -1))[s - 2], bcw=int(rng.choice((0, 1, 3, 4))) if rng.integers(0, 4) == 0 else 2)
            out.append(MC.cu("t%d" % len(out), group, w, h, x, y, rb(), rb()))
    return group, out


def walk_mask(rng):
    """per base: step 0 in all four directions, steps 1..5 in one"""
    d = int(rng.integers(0, 4))
    return 0xF | sum(1 << (4 * s + d) for s in range(1, 6))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--json")
    ap.add_argument("--quick", action="store_true")
    args = ap.parse_args()
    import torch
    import mmvd_cases as MC
    from vvenc_amd.hotpath import HotPath, Plane
    hp = HotPath()
    rounds, reps = (1, 1) if args.quick else (args.rounds, args.reps)
    rng = np.random.default_rng(404)
    group, cl = picture_list(rng)
    n = len(cl)
    refs, org = MC.planes("hd", BD)
    drefs, dorg = [hp.plane(np.array(p), 8, extend=False) for p in refs], hp.plane(np.array(org), 8, extend=False)
    items_b = MC.as_list(cl, drefs[0].stride, dorg.stride)
    items_a = items_b.copy()
    for i in range(n):
        items_a[i]["cand_mask"] = [walk_mask(rng) if m else 0 for m in items_b[i]["cand_mask"]]
    cost_a, cost_b = (torch.zeros((n, 64), dtype=torch.int32, device=hp.device) for _ in range(2))
    pit, bl, rows, by_size = MC.two_launch_lists(hp, items_b, group, drefs[0].stride, 4096)
    pp = Plane(hp.device, 4096, rows, 0)
    jobs, outs = [], []
    for (w, h), lst in by_size.items():
        for (o, x, y, i, v, k) in lst:
            pit[k]["dst_off"] = y * pp.stride + x
        pairs = torch.from_numpy(np.array([(o, y * pp.stride + x) for (o, x, y, _, _, _) in lst], np.int32)).to(hp.device)
        out = torch.zeros(len(lst), dtype=torch.int64, device=hp.device)
        jobs.append((w, h, 0, len(lst), pairs, out))
        outs.append((lst, out))
    table = hp.make_dist_jobs(jobs)
    flat = pp.storage.view(-1)

    def run_a():
        hp.merge_mmvd_costs(drefs, items_a, dorg, WIDTH, HEIGHT, CTU, BD, "HAD_fast", 0, cost=cost_a)

    def run_b():
        hp.merge_mmvd_costs(drefs, items_b, dorg, WIDTH, HEIGHT, CTU, BD, "HAD_fast", 0, cost=cost_b)

    def run_c():
        hp.pred_inter_batch(drefs, pit, flat, pp.stride, BD, blend=bl)
        hp.dist_multi("HAD_fast", dorg, pp, table, BD)

    fns = {"walk": run_a, "full": run_b, "two": run_c}
    for fn in fns.values():
        fn()
    hp.sync()
    ca, cb = cost_a.cpu().numpy().view(np.uint32), cost_b.cpu().numpy().view(np.uint32)
    want = np.zeros_like(cb)
    for lst, out in outs:
        o = out.cpu().numpy()
        for j, (_, _, _, i, v, _) in enumerate(lst):
            want[i, v] = o[j]
    assert np.array_equal(cb, want), "the two-launch form's costs differ from the entry's"
    req = np.array([[(int(items_a[i]["cand_mask"][v >> 5]) >> (v & 31)) & 1 for v in range(64)] for i in range(n)], bool)
    assert np.array_equal(ca[req], cb[req]) and not ca[~req].any()
    print("check: %d CUs, %d candidates: the two-launch form's costs equal the entry's; the walk's %d slots equal the full run's" % (n, pit.size, int(req.sum())))
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
    cands = {"walk": int(req.sum()), "full": int(pit.size), "two": int(pit.size)}
    written = {"walk": 4 * cands["walk"] / 1e6, "full": 4 * cands["full"] / 1e6, "two": (2 * sum(int(p["width"]) * int(p["height"]) for p in pit) + 8 * pit.size) / 1e6}
    out = {"bit_depth": BD, "width": WIDTH, "height": HEIGHT, "cus": n, "shapes": {"%dx%d" % k: len(v) // 64 for k, v in by_size.items()}, "rounds": rounds, "reps": reps, "written_MB": written}
    for k in fns:
        v, dv = np.array(t_call[k]), np.array(t_dev[k])
        out[k] = {"candidates": cands[k], "call_median_us": float(np.median(v)), "call_min_us": float(v.min()), "call_spread": float((v.max() - v.min()) / np.median(v)),
                  "device_median_us": float(np.median(dv)), "device_min_us": float(dv.min()), "device_spread": float((dv.max() - dv.min()) / np.median(dv))}
        print("%-5s CUs %5d candidates %7d  call median %9.1f us (min %9.1f, spread %5.1f %%)  device %9.1f us (min %9.1f, spread %5.1f %%)  written %7.2f MB"
              % (k, n, cands[k], out[k]["call_median_us"], v.min(), 100 * out[k]["call_spread"], out[k]["device_median_us"], dv.min(), 100 * out[k]["device_spread"], written[k]))
    if args.json:
        with open(args.json, "w") as f:
            json.dump(out, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
