#!/usr/bin/env python3
"""Times the SAO entries (vvenc_amd/csrc/sao.hip) on one 1920x1080 4:2:0 10-bit picture at CTU 128 and CTU 64:

  stats        vvhip_sao_stats, the whole picture (three planes) in one launch
  stats_bands  the same picture as one launch per CTU row (what the encoder's row tasks issue through SaoOps::statisticsBand), all rows, one after the other
  offset       vvhip_sao_offset, the whole picture, every CTU on (the edge types and the band type cycling over CTUs and planes)

picture: frame 0 of the synthetic clip the end-to-end tools encode (tests/e2e_fps.synth_clip_chunk) as the original; the "deblocked" planes are the original plus seeded
         noise of +-4 — there is no recorded deblocked picture; the kernels' work does not depend on the values (the band histogram's LDS adds do a little: noise is its
         worst case, runs of equal bands its best).
check  : before anything is timed both entries are compared with tests/sao_ref.py on this picture (CTU 128).
time   : every variant is warmed and timed as `reps` back-to-back calls of the entry between two host clock readings that end in a device synchronise, `rounds` times, the
         variants alternating inside a round; medians, minima and the spread ( max - min ) / median.  A call is the host's argument check (and, for the filter, the
         conversion and upload of the parameter records) plus the launch: the figure is the larger of what the host needs to issue a call and what the device needs to run
         it — what a caller that issues picture after picture sees.
bytes  : what must move — stats: original + deblocked planes read once, the records written; offset: deblocked planes read, SAO'd planes written — over the median time,
         as a fraction of the 8.0 TB/s HBM3E peak of the MI355X (and of the 6.29 TB/s a plain copy reaches).  The picture (12.4 MB) fits the 256 MB last-level cache: with
         the same planes read launch after launch these are rates out of that cache, not out of HBM — an upper bound of what a pipeline's first touch would see.
usage: tools/sao_time.py [--rounds 9] [--reps 40] [--json out.json] [--quick]"""
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
HBM_PEAK, HBM_COPY = 8.0e12, 6.29e12


def picture():
    """-> ( org [3], src [3] ) int16 planes"""
    from e2e_fps import synth_clip_chunk
    y, u, v = synth_clip_chunk(W, H, 0, 1)
    org = [np.ascontiguousarray(p[0]) for p in (y, u, v)]
    rng = np.random.default_rng(294)
    src = [np.clip(p.astype(np.int32) + rng.integers(-4, 5, p.shape), 0, (1 << BD) - 1).astype(np.int16) for p in org]
    return org, src


def params(n_ctus):
    import sao_ref as SR
    prm = np.zeros((n_ctus, 3), SR.PARAM_DTYPE)
    for i in range(n_ctus):
        for c in range(3):
            prm[i, c]["type"], prm[i, c]["band"], prm[i, c]["offs"] = (i + c) % 5, (7 * i) % 32, (3, 1, 0, -1, -3)
    return prm


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--json")
    ap.add_argument("--quick", action="store_true")
    args = ap.parse_args()
    import torch
    import sao_ref as SR
    from vvenc_amd.hotpath import HotPath
    org, src = picture()
    hp = HotPath()
    d_org, d_src, d_dst = [hp.plane(p) for p in org], [hp.plane(p) for p in src], [hp.plane(np.zeros_like(p)) for p in src]
    sp, op = list(zip(d_org, d_src)), list(zip(d_src, d_dst))
    plane_bytes = sum(p.size * 2 for p in org)
    out = {"width": W, "height": H, "bit_depth": BD, "plane_bytes": plane_bytes}
    # ---- check (CTU 128)
    gx, gy = SR.grid(W, H, 128, 128)
    prm = params(gx * gy)
    prm["avail"] = SR.border_avail(gx, gy)[:, None]
    rec = hp.sao_stats(sp, 128, BD).cpu().numpy()
    hp.sao_offset(op, prm, 128, BD)
    for c in range(3):
        cs = 128 >> (c > 0)
        assert np.array_equal(rec[:, c], SR.stats_picture(org[c], src[c], cs, cs, BD, c == 0)), ("statistics", c)
        assert np.array_equal(d_dst[c].visible().cpu().numpy(), SR.offset_picture(src[c], prm[:, c], cs, cs, BD)), ("offset", c)
    print("check: statistics and offset filter of the %dx%d picture at CTU 128 are the model's" % (W, H))
    rounds, reps = (1, 5) if args.quick else (args.rounds, args.reps)
    for ctu in (128, 64):
        gx, gy = SR.grid(W, H, ctu, ctu)
        prm = params(gx * gy)
        prm["avail"] = SR.border_avail(gx, gy)[:, None]
        st = torch.zeros((gx * gy, 3, 5, 2, 32), dtype=torch.int64, device=hp.device)
        fns = {"stats": lambda: hp.sao_stats(sp, ctu, BD, out=st),
               "stats_bands": lambda: [hp.sao_stats(sp, ctu, BD, rows=(r, 1), out=st) for r in range(gy)],
               "offset": lambda: hp.sao_offset(op, prm, ctu, BD)}
        for fn in fns.values():      # warm-up: code objects, the parameter slot
            for _ in range(3):
                fn()
        hp.sync()
        times = {k: [] for k in fns}
        for _ in range(rounds):
            for k, fn in fns.items():
                t0 = time.perf_counter()
                for _ in range(reps):
                    fn()
                hp.sync()
                times[k].append((time.perf_counter() - t0) / reps * 1e6)
        moved = {"stats": 2 * plane_bytes + st.numel() * 8, "stats_bands": 2 * plane_bytes + st.numel() * 8, "offset": 2 * plane_bytes}
        res = {"ctus": gx * gy, "launches": {"stats": 1, "stats_bands": gy, "offset": 1}}
        for k, v in times.items():
            v = np.array(v)
            med = float(np.median(v))
            res[k] = {"median_us": med, "min_us": float(v.min()), "spread": float((v.max() - v.min()) / med), "bytes": moved[k], "bytes_per_s": moved[k] / (med * 1e-6),
                      "of_hbm_peak": moved[k] / (med * 1e-6) / HBM_PEAK, "of_hbm_copy": moved[k] / (med * 1e-6) / HBM_COPY}
            print("CTU %3d  %-11s median %8.1f us  min %8.1f us  spread %5.1f %%  %6.2f MB -> %5.2f TB/s = %4.1f %% of the HBM peak (%4.1f %% of a plain copy's rate)"
                  % (ctu, k, med, v.min(), 100 * res[k]["spread"], moved[k] / 1e6, res[k]["bytes_per_s"] / 1e12, 100 * res[k]["of_hbm_peak"], 100 * res[k]["of_hbm_copy"]))
        out["ctu%d" % ctu] = res
    out["rounds"], out["reps"] = rounds, reps
    if args.json:
        with open(args.json, "w") as f:
            json.dump(out, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
