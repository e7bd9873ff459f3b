#!/usr/bin/env python3
"""Times the intra chroma mode pre-selection entry (vvenc_amd/csrc/intrachroma.hip) on a synthetic list shaped like the chroma of an intra picture of 1920x1080 4:2:0, 10 bit:

  (a) precheck  the five slots IntraSearch::estIntraPredChromaQT pre-checks (the three regular defaults, MDLM_L, MDLM_T: IntraSearch.cpp:806-813), costs only
  (b) all8      all eight slots, costs only
  (c) unfused   the entry writing ALL predictions of all eight slots, then the existing vvhip_dist_batch with HAD and with SAD on ( original, prediction ) pairs, one pair of
                calls per block shape — the long way; min( 2 SAD, HAD ) of Cb plus Cr formed from its outputs must equal (b)'s costs

list   : the block list tools/intra_time.py builds (its stated mix by share of the picture's area), halved: a luma block w x h gives the chroma block w/2 x h/2; luma blocks with
         a side of 4 (chroma side 2) are outside the entry's scope and stay with the caller — 32x32 10 %, 16x16 25 %, 8x8 28 %, 4x4 14 %, 16x4 and 4x16 4 % each of the
         picture's area.  Every block: both sides available with the longest templates, the candidate list of CU::getIntraChromaCandModes with DM cycling through 16 modes,
         its own window of reconstructed luma in one luma array.  Luma, lines and originals: tests/intra_chroma_cases.fields (smooth plus noise, chroma correlated with luma).
check  : before anything is timed, three blocks of every shape are compared with tests/intra_chroma_ref.py, and (c)'s costs with (b)'s on the whole list.
time   : device = events around one workload issued behind ~2 ms of other work on the stream (the upload of the item list included, the host not);
         call   = `reps` back-to-back runs between two host clock readings that end in a device synchronise.  `rounds` times each, the workloads alternating inside a round;
         medians, minima, spread ( max - min ) / median.
usage: tools/intra_chroma_time.py [--rounds 9] [--reps 5] [--json out.json] [--quick]"""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np  # noqa: E402

import intra_time as IT  # noqa: E402

BD = IT.BD
PRECHECK_MASK = 0x6e          # slots 1, 2, 3 (the regular defaults besides planar), 5 (MDLM_L), 6 (MDLM_T)


def chroma_mix():
    """tools/intra_time.py's mix halved -> [ ( ( w, h ), count ) ] of the chroma shapes inside the entry's scope"""
    out = []
    for (w, h), share in IT.MIX:
        if min(w, h) >= 8:
            out.append(((w // 2, h // 2), int(round(share * IT.WIDTH * IT.HEIGHT / (w * h)))))
    return out


def picture_cases(variants=24):
    """the list as tests/intra_chroma_cases.Case objects: per shape `variants` distinct blocks, repeated to the shape's count (the kernel does not know)"""
    import intra_chroma_cases as CC
    import intra_chroma_ref as CR
    out = []
    for k, ((w, h), n) in enumerate(chroma_mix()):
        pool = [CC.Case("t%dx%d_%d" % (w, h, v), w, h, BD, CR.F_ABOVE | CR.F_LEFT, w, h, CC.cand_list(CC.DM_CYCLE[v % 16]),
                        *CC.fields(np.random.default_rng(9500 + 100 * k + v), w, h, BD, "smooth"), pred_mask=0) for v in range(min(variants, n))]
        out += [pool[i % len(pool)] for i in range(n)]
    return out


def build_list(cl, mode_mask, pred):
    """the list with every DISTINCT case's luma window, lines and originals stored once -> ( items, luma, ref, org, prediction samples )"""
    import intra_chroma_cases as CC
    distinct, index = [], {}
    for c in cl:
        if id(c) not in index:
            index[id(c)] = len(distinct)
            distinct.append(c)
    base, luma, ref, org, _ = CC.as_list(distinct, pred="none", mode_mask=mode_mask)
    items = base[[index[id(c)] for c in cl]].copy()
    at = 0
    for i in range(items.size):
        n = int(items[i]["w"]) * int(items[i]["h"])
        npred = bin(mode_mask).count("1") if pred else 0
        items[i]["pred_mask"] = mode_mask if pred else 0
        items[i]["pred_off"], items[i]["cost_off"] = (at, at + npred * n), 8 * i
        at += 2 * npred * n
    return items, luma, ref, org, at


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--json")
    ap.add_argument("--quick", action="store_true")
    args = ap.parse_args()
    import torch
    import intra_chroma_cases as CC
    from vvenc_amd.hotpath import DF, HotPath
    hp = HotPath()
    rounds, reps = (1, 2) if args.quick else (args.rounds, args.reps)
    cl = picture_cases()
    n = len(cl)
    items_a, luma, ref, org, _ = build_list(cl, PRECHECK_MASK, False)
    items_b = build_list(cl, 0xff, False)[0]
    items_c, _, _, _, npred = build_list(cl, 0xff, True)
    dluma, dref, dorg = (torch.from_numpy(v).to(hp.device) for v in (luma, ref, org))
    cost_a, cost_b, cost_c = (torch.zeros((n, 8), dtype=torch.int32, device=hp.device) for _ in range(3))
    pred_c = torch.zeros(npred, dtype=torch.int16, device=hp.device)
    hp.intra_chroma_modes(items_b, dluma, dref, dorg, cost=cost_b, pred=None)
    hp.sync()
    cb = cost_b.cpu().numpy().astype(np.uint32)
    first = {}
    for i, c in enumerate(cl):
        first.setdefault((c.w, c.h), []).append(i)
    for idx in first.values():
        for i in idx[:3]:
            assert np.array_equal(cb[i], CC.expected(cl[i])[0]), cl[i].name
    print("check: %d blocks of the list equal the model" % (3 * len(first)))
    # (c): per shape one list of ( original, prediction ) pairs over both components and all eight slots
    dist_calls = []
    for (w, h), idx in first.items():
        di = np.zeros((len(idx) * 16, 2), np.int32)
        for j, i in enumerate(idx):
            for comp in (0, 1):
                rows = slice(j * 16 + comp * 8, j * 16 + comp * 8 + 8)
                di[rows, 0] = int(items_c[i]["org_off"][comp])
                di[rows, 1] = int(items_c[i]["pred_off"][comp]) + np.arange(8) * w * h
        dist_calls.append((w, h, idx, torch.from_numpy(di).to(hp.device), torch.zeros(len(di), dtype=torch.int64, device=hp.device), torch.zeros(len(di), dtype=torch.int64, device=hp.device)))

    def run_a():
        hp.intra_chroma_modes(items_a, dluma, dref, dorg, cost=cost_a, pred=None)

    def run_b():
        hp.intra_chroma_modes(items_b, dluma, dref, dorg, cost=cost_b, pred=None)

    def run_c():
        hp.intra_chroma_modes(items_c, dluma, dref, dorg, cost=cost_c, pred=pred_c)
        for (w, h, idx, di, dhad, dsad) in dist_calls:
            for f, do in (("HAD", dhad), ("SAD", dsad)):
                hp._ck(hp.L.vvhip_dist_batch(hp.ctx, DF[f], C.c_void_p(dorg.data_ptr()), w, C.c_void_p(pred_c.data_ptr()), w, w, h, 0, BD, C.c_void_p(di.data_ptr()), di.shape[0],
                                             C.c_void_p(do.data_ptr())))

    fns = {"precheck": run_a, "all8": run_b, "unfused": run_c}
    for fn in fns.values():
        fn()
    hp.sync()
    ca = cost_a.cpu().numpy()
    assert np.array_equal(cost_c.cpu().numpy(), cost_b.cpu().numpy()) and all(np.array_equal(ca[:, s], cb[:, s].astype(np.int32)) for s in range(8) if (PRECHECK_MASK >> s) & 1)
    for (w, h, idx, di, dhad, dsad) in dist_calls:
        per = np.minimum(dhad.cpu().numpy(), 2 * dsad.cpu().numpy()).reshape(len(idx), 2, 8).sum(axis=1)
        assert np.array_equal(per, cb[idx].astype(np.int64)), (w, h)
    print("check: the unfused chain's %d costs equal the entry's" % (8 * n))
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
    slots = {"precheck": bin(PRECHECK_MASK).count("1"), "all8": 8, "unfused": 8}
    out = {"bit_depth": BD, "width": IT.WIDTH, "height": IT.HEIGHT, "blocks": n, "shapes": {"%dx%d" % k: len(v) for k, v in first.items()}, "rounds": rounds, "reps": reps,
           "luma_MB": luma.nbytes / 1e6, "written_MB": {"precheck": 0.0, "all8": 0.0, "unfused": pred_c.numel() * 2 / 1e6}}
    for k in fns:
        v, dv = np.array(t_call[k]), np.array(t_dev[k])
        out[k] = {"slots": slots[k], "pairs": slots[k] * n, "call_median_us": float(np.median(v)), "call_min_us": float(v.min()), "call_spread": float((v.max() - v.min()) / np.median(v)),
                  "device_median_us": float(np.median(dv)), "device_min_us": float(dv.min()), "device_spread": float((dv.max() - dv.min()) / np.median(dv))}
        print("%-8s blocks %5d (block, slot) pairs %7d  call median %9.1f us (min %9.1f, spread %5.1f %%)  device %9.1f us (min %9.1f, spread %5.1f %%)  predictions written %7.2f MB"
              % (k, n, slots[k] * n, out[k]["call_median_us"], v.min(), 100 * out[k]["call_spread"], out[k]["device_median_us"], dv.min(), 100 * out[k]["device_spread"], out["written_MB"][k]))
    if args.json:
        with open(args.json, "w") as f:
            json.dump(out, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
