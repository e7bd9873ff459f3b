#!/usr/bin/env python3
"""tools/sbt_time.py — what testing two SBT candidates per inter CU costs on the device, against the same CUs coded unsplit, and what the part energies cost against the only
way to get them without the new entry.

  python tools/sbt_time.py [--rounds 9] [--reps 40] [--poc 23] [--json PATH] [--quick]

The list is SYNTHETIC: no SBT work list was ever recorded (the recordings are of preset faster, where SBT is off).  It is built from the recorded 1920x1080 picture --poc:
every luma TU of that picture with both sides >= 8 is taken as an inter CU (its recorded residual block and QP), its Cb and Cr residuals are the two 2:1 decimations of that
block at half amplitude (one negated), sbt_allowed is the size rule of CU::checkAllowedSbt, the chroma weight 2^(1/3), and the candidates are the two best half modes of
every CU from the device's own `order`.  The CUs lie shelf-packed in one buffer of ONE row pitch (luma rows, then the Cb and the Cr rows), so that the distortion lists, which
take one pitch per call, can read the same buffer.
  (a) parts   : vvhip_sbt_parts_batch (part sums, estimates, order)  against  dist : the same sums with today's entries — one SSE item per part and component against a zero
                plane through vvhip_dist_multi_func, one job per part size (the estimates and the order would still be host work on 48 downloaded sums per CU)
  (b) chain   : parts -> vvhip_tu_rdo_multi_strided on the coded tiles of both candidates, read in place -> vvhip_sbt_place_batch over all candidates for the SSEs (the
                candidates of a CU share its block of the reconstruction, so the reconstruction is placed for the winners alone: variant `winners`, one candidate per CU with
                d_rec)  against  unsplit : the same CUs' three blocks as whole DCT-2 TUs through vvhip_tu_rdo_multi_strided
  (c) bytes   : what the two new kernels move (residual in, sums out; tiles and original residual in, blocks and sums out), printed with the times
Steps, each a child process with a time limit of its own, the next one only after the previous one ended well:
  check : part sums, estimates and order against the model (tests/sbt_ref.py) on every CU; every candidate's placed blocks and SSEs against the model applied to the chain's
          own tile reconstructions and statistics, dense and sparse outputs; the distortion lists' sums against the parts entry's
  time  : every variant is warmed, recorded into a launch graph and timed as `reps` graph launches between two host clock readings that end in a device synchronise, `rounds`
          times, the variants alternating inside a round; medians, minima and the spread ( max - min ) / median.
--quick: one round of few launches (for a profiler run)."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np  # noqa: E402

PITCH, BD, CW = 2048, 10, 2.0 ** (1.0 / 3.0)
STEP_LIMIT = {"check": 300, "time": 420}          # seconds


def picture(poc):
    """-> ( SBT items, residual buffer [rows, PITCH] int16, luma QPs ) from the recorded picture's luma TUs of side >= 8"""
    from bench_common import prepare_recordings
    from vvenc_amd.hotpath import make_sbt_items, sbt_allowed_of
    import sbt_cases as SC
    pic = prepare_recordings(1920, 1080, 65, [poc])[0][poc]
    tu = pic.tu
    sel = [t for t in tu if int(t["comp"]) == 0 and int(t["w"]) >= 8 and int(t["h"]) >= 8 and int(t["w"]) <= 64 and int(t["h"]) <= 64]
    sel.sort(key=lambda t: (-int(t["w"]) * int(t["h"]), -int(t["w"])))
    where, rows = SC.shelf_pack([(int(t["w"]), int(t["h"])) for t in sel], PITCH)
    rows += rows & 1
    buf = np.zeros((2 * rows, PITCH), np.int16)          # luma rows, then rows / 2 of Cb and rows / 2 of Cr
    cus, qps = [], []
    for t, (x, y) in zip(sel, where):
        w, h = int(t["w"]), int(t["h"])
        blk = np.asarray(pic.pool[int(t["pool"]):int(t["pool"]) + w * h]).reshape(h, w)
        buf[y:y + h, x:x + w] = blk
        cy = (rows + y // 2, rows + rows // 2 + y // 2)
        buf[cy[0]:cy[0] + h // 2, x // 2:x // 2 + w // 2] = blk[::2, ::2] // 2
        buf[cy[1]:cy[1] + h // 2, x // 2:x // 2 + w // 2] = -(blk[1::2, 1::2] // 2)
        cus.append((y * PITCH + x, cy[0] * PITCH + x // 2, cy[1] * PITCH + x // 2, PITCH, PITCH, w, h, sbt_allowed_of(w, h)))
        qps.append(int(t["qp"]))
    return make_sbt_items(cus), buf, np.array(qps, np.int32)


class World:
    def __init__(self, poc):
        import torch
        from vvenc_amd.hotpath import HotPath, STATS_DTYPE
        self.items, self.buf, self.qps = picture(poc)
        n = len(self.items)
        self.hp, self.hp_w, self.hp_u, self.hp_d = (HotPath() for _ in range(4))          # a context per variant: each caches the schedules / job table of ONE list
        hp = self.hp
        self.resi = torch.from_numpy(self.buf.reshape(-1)).to(hp.device)
        self.parts = torch.zeros((n, 3, 16), dtype=torch.int64, device=hp.device)
        self.est = torch.zeros((n, 9), dtype=torch.int64, device=hp.device)
        self.order = torch.zeros((n, 8), dtype=torch.uint8, device=hp.device)
        hp.sbt_parts_batch(self.resi, self.items, CW, self.parts, self.est, self.order)
        torch.cuda.synchronize()
        order = self.order.cpu().numpy()
        self.cand = [(i, int(m)) for i in range(n) for m in order[i][:2]]          # the two best half modes of every CU, from the device's own order
        assert all(0 <= m <= 3 for (_, m) in self.cand)
        cq = np.array([[self.qps[i], self.qps[i] + 1, self.qps[i] + 1] for (i, _) in self.cand], np.int32)
        self.place, jobs, self.strides, self.level, self.tile_rec, self.stats = hp.make_sbt_tu_jobs(self.items, self.cand, cq)
        self.jobs = hp.make_tu_jobs(jobs)
        self.sse = torch.zeros((len(self.cand), 3), dtype=torch.int64, device=hp.device)
        # the winners: the first candidate of every CU, placed with the reconstruction
        self.win = self.place[0::2].copy()
        self.rec = torch.zeros_like(self.resi)
        self.win_sse = torch.zeros((n, 3), dtype=torch.int64, device=hp.device)
        # unsplit: every component block of every CU as one DCT-2 TU, one job per ( width, height )
        groups = {}
        for i, it in enumerate(self.items):
            for c, off in enumerate((it["y_off"], it["cb_off"], it["cr_off"])):
                groups.setdefault((int(it["width"]) >> (c > 0), int(it["height"]) >> (c > 0)), []).append((int(off), self.qps[i] + (c > 0), c == 0))
        total, ntu = sum(w * h * len(v) for (w, h), v in groups.items()), sum(len(v) for v in groups.values())
        self.u_level, self.u_rec = (torch.zeros(total, dtype=torch.int16, device=hp.device) for _ in range(2))
        self.u_stats = torch.zeros((ntu, STATS_DTYPE.itemsize), dtype=torch.uint8, device=hp.device)
        ujobs, first, base = [], 0, 0
        for (w, h) in sorted(groups, reverse=True):
            v = groups[(w, h)]
            k = len(v)
            ujobs.append((w, h, 0, 0, k, 8, hp.to_device(np.array([o for (o, _, _) in v], np.int32)), hp.to_device(HotPath.tu_qp([q for (_, q, _) in v], 0, np.array([l for (_, _, l) in v], np.int16))),
                          self.u_level[base:base + k * w * h], self.u_rec[base:base + k * w * h], self.u_stats[first:first + k]))
            first, base = first + k, base + k * w * h
        self.u_jobs, self.u_strides, self.n_unsplit = hp.make_tu_jobs(ujobs), [PITCH] * len(ujobs), ntu
        # dist: one SSE item per part and component against a zero plane, one job per part size
        self.org = self.hp_d.plane(self.buf, 0)
        self.zero = self.hp_d.plane(np.zeros_like(self.buf), 0)
        assert self.org.stride == PITCH
        dg = {}
        for i, it in enumerate(self.items):
            w, h = int(it["width"]), int(it["height"])
            npx, npy = (4 if w >= 16 else 2), (4 if h >= 16 else 2)
            for c, off in enumerate((it["y_off"], it["cb_off"], it["cr_off"])):
                pw, ph = (w >> (c > 0)) // npx, (h >> (c > 0)) // npy
                for j in range(npy):
                    for ii in range(npx):
                        o = int(off) + j * ph * PITCH + ii * pw
                        dg.setdefault((pw, ph), []).append((o, (i * 3 + c) * 16 + 4 * j + ii))
        self.d_where = {k: np.array([p for (_, p) in v]) for k, v in dg.items()}
        self.d_out = {k: torch.zeros(len(v), dtype=torch.int64, device=hp.device) for k, v in dg.items()}
        self.d_jobs = self.hp_d.make_dist_fjobs([("SSE", pw, ph, 0, len(v), hp.to_device(np.array([(o, o) for (o, _) in v], np.int32)), self.d_out[(pw, ph)]) for (pw, ph), v in dg.items()])
        self.n_dist = sum(len(v) for v in dg.values())

    def run_parts(self):
        self.hp.sbt_parts_batch(self.resi, self.items, CW, self.parts, self.est, self.order)

    def run_chain(self):
        self.run_parts()
        self.hp.tu_rdo_multi_strided(self.resi, self.strides, self.jobs, BD)
        self.hp.sbt_place_batch(self.tile_rec, self.place, self.stats, None, self.resi, self.sse)

    def run_winners(self):
        self.hp_w.sbt_place_batch(self.tile_rec, self.win, self.stats, self.rec, self.resi, self.win_sse)

    def run_unsplit(self):
        self.hp_u.tu_rdo_multi_strided(self.resi, self.u_strides, self.u_jobs, BD)

    def run_dist(self):
        self.hp_d.dist_multi_func(self.org, self.zero, self.d_jobs, BD)

    def bytes_moved(self):
        """-> ( parts kernel, placement kernel over all candidates, placement of the winners ) in bytes: samples in and out, sums and records"""
        from vvenc_amd.hotpath import STATS_DTYPE
        st = self.stats.cpu().numpy().view(STATS_DTYPE).reshape(-1)
        area = lambda it: int(it["width"]) * int(it["height"]) * 3 // 2
        parts = sum(2 * area(it) + 28 + (48 + 9 + 1) * 8 for it in self.items)
        def place(items, with_rec):
            b = 0
            for p in items:
                a = area(p)
                tile = sum((a * 2 // 3 if c == 0 else a // 6) for c in range(3) if st[int(p["stats_idx"][c])]["abs_sum"])          # half of the component block, 2 bytes a sample
                b += 2 * a + tile + (2 * a if with_rec else 0) + 56 + 24 + 3 * 24
            return b
        return parts, place(self.place, False), place(self.win, True)


def step_check(args):
    import torch
    from vvenc_amd.hotpath import STATS_DTYPE
    import sbt_ref as SR
    W = World(args.poc)
    n = len(W.items)
    parts, est, order = W.parts.cpu().numpy().view(np.uint64), W.est.cpu().numpy().view(np.uint64), W.order.cpu().numpy()
    view = lambda buf, off, w, h: buf.reshape(-1)[off + PITCH * np.arange(h)[:, None] + np.arange(w)[None, :]]
    blocks = []
    for i, it in enumerate(W.items):
        w, h = int(it["width"]), int(it["height"])
        b = (view(W.buf, int(it["y_off"]), w, h), view(W.buf, int(it["cb_off"]), w // 2, h // 2), view(W.buf, int(it["cr_off"]), w // 2, h // 2))
        blocks.append(b)
        p = SR.part_sums(*b)
        e, o = SR.estimate(p, w, h, int(it["sbt_allowed"]), CW)
        assert [[int(v) for v in r] for r in parts[i]] == p and [int(v) for v in est[i]] == e and [int(v) for v in order[i]] == o, ("parts", i, w, h)
    W.run_dist()
    torch.cuda.synchronize()
    flat = parts.reshape(-1)
    for k, out in W.d_out.items():
        assert np.array_equal(out.cpu().numpy().view(np.uint64), flat[W.d_where[k]]), ("distortion lists", k)
    n_zero = 0
    for sparse in (0, 1):
        W.hp.tu_set_sparse_outputs(sparse)
        W.hp_w.tu_set_sparse_outputs(sparse)
        W.tile_rec.fill_(-7)
        W.run_chain(); W.run_winners()
        torch.cuda.synchronize()
        st = W.stats.cpu().numpy().view(STATS_DTYPE).reshape(-1)
        tile_rec, sse, rec, wsse = W.tile_rec.cpu().numpy(), W.sse.cpu().numpy().view(np.uint64), W.rec.cpu().numpy(), W.win_sse.cpu().numpy().view(np.uint64)
        for k, (cu, mode) in enumerate(W.cand):
            for c, blk in enumerate(blocks[cu]):
                h, w = blk.shape
                x, y, tw, th = SR.coded_tile(w, h, mode)
                zero = int(st[int(W.place[k]["stats_idx"][c])]["abs_sum"]) == 0
                n_zero += zero
                o = int(W.place[k]["tile_off"][c])
                e = SR.place(None if zero else tile_rec[o:o + tw * th], w, h, mode)
                assert int(sse[k][c]) == SR.sse(e, blk), ("sse", sparse, k, c)
                if k % 2 == 0:
                    off = int(W.items[cu][("y_off", "cb_off", "cr_off")[c]])
                    assert np.array_equal(view(rec, off, w, h), e) and int(wsse[k // 2][c]) == int(sse[k][c]), ("winner", sparse, k, c)
    W.hp.tu_set_sparse_outputs(0)
    print("check: %d CUs, %d candidates, %d of %d tiles without levels: parts, estimates, order, placement and SSEs are the model's; %d distortion items give the same part sums"
          % (n, len(W.cand), n_zero // 2, 3 * len(W.cand), W.n_dist))
    assert 0 < n_zero // 2 < 3 * len(W.cand)


def step_time(args):
    import torch
    W = World(args.poc)
    W.run_chain(); W.run_winners()
    torch.cuda.synchronize()
    hp_p = type(W.hp)()          # the parts entry alone, on a context of its own
    fns = {"parts": (hp_p, lambda: hp_p.sbt_parts_batch(W.resi, W.items, CW, W.parts, W.est, W.order)), "dist": (W.hp_d, W.run_dist), "chain": (W.hp, W.run_chain),
           "winners": (W.hp_w, W.run_winners), "unsplit": (W.hp_u, W.run_unsplit)}
    graphs, first_call, variants = {}, {}, {}
    for name, (h, fn) in fns.items():
        h.use_own_stream()          # warm-up (schedules, job tables) on the stream the graph is recorded on
        t0 = time.perf_counter(); fn(); first_call[name] = time.perf_counter() - t0
        h.sync()
        graphs[name] = h.graph_capture(fn)
        variants[name] = (lambda h, g: (lambda reps: ([h.graph_launch(g) for _ in range(reps)], h.sync())))(h, graphs[name])
    rounds, reps = (1, 5) if args.quick else (args.rounds, args.reps)
    for fn in variants.values():
        fn(3)
    times = {k: [] for k in variants}
    for _ in range(rounds):
        for k, fn in variants.items():
            t0 = time.perf_counter()
            fn(reps)
            times[k].append((time.perf_counter() - t0) / reps * 1e6)
    hist = {}
    for it in W.items:
        hist[(int(it["width"]), int(it["height"]))] = hist.get((int(it["width"]), int(it["height"])), 0) + 1
    out = {"poc": args.poc, "cus": len(W.items), "candidates": len(W.cand), "sizes": {"%dx%d" % k: v for k, v in sorted(hist.items(), reverse=True)}, "tu_jobs_chain": W.jobs[1],
           "tus_unsplit": W.n_unsplit, "dist_items": W.n_dist, "dist_jobs": W.d_jobs[1], "samples": int(sum(int(i["width"]) * int(i["height"]) * 3 // 2 for i in W.items)),
           "rounds": rounds, "reps": reps, "first_call_ms": {k: 1e3 * v for k, v in first_call.items()}}
    print("%d CUs %s, %d candidates in %d TU jobs; unsplit %d TUs; %d distortion items in %d jobs" % (out["cus"], out["sizes"], out["candidates"], out["tu_jobs_chain"], out["tus_unsplit"], out["dist_items"], out["dist_jobs"]))
    print("first call (host: sort, schedule, upload): " + ", ".join("%s %.2f ms" % (k, 1e3 * v) for k, v in first_call.items()))
    for k, v in times.items():
        v = np.array(v)
        out[k] = {"median_us": float(np.median(v)), "min_us": float(v.min()), "spread": float((v.max() - v.min()) / np.median(v))}
        print("%-9s median %9.1f us  min %9.1f us  spread %5.1f %%" % (k, out[k]["median_us"], out[k]["min_us"], 100 * out[k]["spread"]))
    out["parts_over_dist"] = out["parts"]["median_us"] / out["dist"]["median_us"]
    out["chain_over_unsplit"] = out["chain"]["median_us"] / out["unsplit"]["median_us"]
    b = W.bytes_moved()
    out["bytes"] = {"parts": b[0], "place_all": b[1], "place_winners": b[2]}
    print("parts / dist = %.3f   chain / unsplit = %.3f   ( chain + winners ) / unsplit = %.3f" % (out["parts_over_dist"], out["chain_over_unsplit"], (out["chain"]["median_us"] + out["winners"]["median_us"]) / out["unsplit"]["median_us"]))
    print("bytes moved: parts kernel %.2f MB, placement of all candidates (SSEs only) %.2f MB, placement of the winners (with the reconstruction) %.2f MB" % tuple(v / 1e6 for v in b))
    if args.json:
        with open(args.json, "w") as f:
            json.dump(out, f, indent=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--poc", type=int, default=23)
    ap.add_argument("--json")
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--step", choices=sorted(STEP_LIMIT))
    args = ap.parse_args()
    if args.step:
        {"check": step_check, "time": step_time}[args.step](args)
        return 0
    for step in ("check", "time"):
        cmd = [sys.executable, os.path.abspath(__file__), "--step", step] + [a for a in sys.argv[1:]]
        try:
            rc = subprocess.run(cmd, timeout=STEP_LIMIT[step]).returncode
        except subprocess.TimeoutExpired:
            print("step %s ran into its limit of %d s: stopping" % (step, STEP_LIMIT[step]), file=sys.stderr)
            return 124
        if rc != 0:
            print("step %s ended with %d: stopping" % (step, rc), file=sys.stderr)
            return rc
    return 0


if __name__ == "__main__":
    sys.exit(main())
