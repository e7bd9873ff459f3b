#!/usr/bin/env python3
"""tools/ict_time.py — what joint Cb-Cr coding of a picture's chroma TUs costs on the device, against the same TUs coded as separate Cb and Cr jobs.

  python tools/ict_time.py [--rounds 9] [--reps 40] [--scale 1] [--other-lib PATH] [--json PATH] [--quick]

The list: the chroma TUs of one 1920x1080 B picture — the fixed histogram TU_HIST below (synthetic: the 4:2:0 chroma blocks of tools/pred_time.py's prediction units, shaped
like the recorded 1080p lists: most samples in 32x32 and 16x16 blocks, most blocks 8x8 and smaller), seeded residuals (a shared smooth part, a part of each component's own,
noise; a third of the TUs nearly flat so that they quantise to nothing), ICT modes cycling over the six, one joint QP.  Cb and Cr blocks lie compactly one after the other.
--scale N multiplies every count of the histogram (4: the chroma TUs of a 3840x2160 picture).
  joint    : vvhip_ict_fwd_batch -> vvhip_tu_rdo_multi_strided on the joint buffer (one job per size) -> vvhip_ict_inv_batch with the jobs' statistics (HotPath.tu_rdo_joint):
             ONE pass through transform / quantisation / dequantisation / inverse transform per TU plus two elementwise passes
  separate : the same TUs as Cb jobs and Cr jobs through vvhip_tu_rdo_multi_strided of the same build: TWO passes per TU
  parent   : with --other-lib, the separate jobs through vvhip_tu_rdo_multi_strided of ANOTHER build of the library (the parent commit's), in the same rounds
Steps, each a child process with a time limit of its own, the next one only after the previous one ended well:
  check : the chain's forward and inverse outputs against the numpy model (tests/ict_ref.py) applied to the residuals and to the chain's own joint reconstruction and
          statistics, dense and sparse outputs — the chain is composed right before anything is timed
  time  : every variant is warmed, recorded into a launch graph and timed as `reps` graph launches between two host clock readings that end in a device synchronise, `rounds`
          times, the variants alternating inside a round; medians, minima and the spread ( max - min ) / median are printed, and joint / separate (and separate / parent).
--quick: one round of few launches (for a profiler run)."""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402

# chroma TUs of one picture: (width, height) -> count
TU_HIST = {(32, 32): 150, (16, 16): 420, (32, 16): 60, (16, 32): 60, (16, 8): 160, (8, 16): 160, (8, 8): 900, (8, 4): 260, (4, 8): 260, (4, 4): 700}
SEED, QP, BD = 20250, 34, 10
MODES = (1, -1, 2, -2, 3, -3)
STEP_LIMIT = {"check": 240, "time": 420}          # seconds


def picture(rng, scale=1):
    """-> ( blocks for make_ict_items, the residual buffer ): Cb block then Cr block per TU, compact"""
    blocks, parts, at, k = [], [], 0, 0
    for (w, h), count in TU_HIST.items():
        yy, xx = np.mgrid[0:h, 0:w]
        for _ in range(count * scale):
            flat = k % 3 == 0
            amp = 3.0 if flat else 90.0
            base = rng.normal(0, amp) * np.cos((xx + 0.5) * np.pi / w) + rng.normal(0, amp) * np.cos((yy + 0.5) * np.pi / h) + rng.normal(0, amp / 3, (h, w))
            cb = np.clip(np.rint(base), -1023, 1023).astype(np.int16)
            cr = np.clip(np.rint(rng.choice([-1.0, -0.5, 0.5, 1.0]) * base + rng.normal(0, amp / 4, (h, w))), -1023, 1023).astype(np.int16)
            blocks.append((at, at + w * h, w, w, h, MODES[k % 6]))
            parts += [cb.reshape(-1), cr.reshape(-1)]
            at += 2 * w * h
            k += 1
    return blocks, np.concatenate(parts)


def separate_jobs(hp, blocks, qp):
    """the Cb and Cr blocks as plain TU jobs on the residual buffer: one job per size, 2 x count TUs -> ( jobs, strides, level, rec, stats )"""
    import torch
    from vvenc_amd.hotpath import STATS_DTYPE, HotPath
    n2 = 2 * len(blocks)
    total = sum(2 * w * h for (_, _, _, w, h, _) in blocks)
    level, rec = (torch.zeros(total, dtype=torch.int16, device=hp.device) for _ in range(2))
    stats = torch.zeros((n2, STATS_DTYPE.itemsize), dtype=torch.uint8, device=hp.device)
    jobs, strides, first, base = [], [], 0, 0
    for (w, h) in TU_HIST:
        offs = np.array([o for (cb, cr, _, bw, bh, _) in blocks if (bw, bh) == (w, h) for o in (cb, cr)], np.int32)
        k = offs.size
        jobs.append((w, h, 0, 0, k, 8, hp.to_device(offs), hp.to_device(HotPath.tu_qp([qp] * k, 0, 0)), level[base:base + k * w * h], rec[base:base + k * w * h], stats[first:first + k]))
        strides.append(w)
        first += k
        base += k * w * h
    return jobs, strides, level, rec, stats


class OtherBuild:
    """vvhip_tu_rdo_multi_strided of another build of the library, through its own context (its own stream)"""

    def __init__(self, path, device):
        vp, i32 = C.c_void_p, C.c_int
        self.L = L = C.CDLL(path)
        L.vvhip_create.argtypes = [C.POINTER(vp), i32]
        L.vvhip_destroy.argtypes = [vp]
        L.vvhip_destroy.restype = None
        L.vvhip_last_error.restype = C.c_char_p
        L.vvhip_last_error.argtypes = [vp]
        for n in ("vvhip_use_own_stream", "vvhip_sync", "vvhip_graph_begin"):
            getattr(L, n).argtypes = [vp]
        L.vvhip_graph_end.argtypes = [vp, vp]
        L.vvhip_graph_launch.argtypes = [vp, vp]
        L.vvhip_tu_rdo_multi_strided.argtypes = [vp, vp, vp, i32, vp, i32]
        self.ctx = vp()
        self.ck(L.vvhip_create(C.byref(self.ctx), device))
        self.ck(L.vvhip_use_own_stream(self.ctx))

    def ck(self, rc):
        if rc:
            raise RuntimeError("other build: error %d: %s" % (rc, self.L.vvhip_last_error(self.ctx).decode()))

    def capture(self, fn):
        fn()
        self.ck(self.L.vvhip_sync(self.ctx))
        self.ck(self.L.vvhip_graph_begin(self.ctx))
        fn()
        g = C.c_void_p()
        self.ck(self.L.vvhip_graph_end(self.ctx, C.byref(g)))
        return g

    def run(self, g, reps):
        for _ in range(reps):
            self.ck(self.L.vvhip_graph_launch(self.ctx, g))
        self.ck(self.L.vvhip_sync(self.ctx))


def world(hp, scale=1):
    from vvenc_amd.hotpath import make_ict_items
    import torch
    rng = np.random.default_rng(SEED)
    blocks, resi_np = picture(rng, scale)
    resi = torch.from_numpy(resi_np).to(hp.device)
    items, _ = make_ict_items(blocks)
    items, jobs, strides, level, joint_rec, stats = hp.make_joint_tu_jobs(items, QP)
    joint = torch.zeros_like(joint_rec)
    dist, sse = (torch.zeros((len(items), 2), dtype=torch.int64, device=hp.device) for _ in range(2))
    rec = torch.zeros_like(resi)
    J = dict(items=items, jobs=hp.make_tu_jobs(jobs), strides=strides, level=level, joint_rec=joint_rec, stats=stats, joint=joint, dist=dist, sse=sse, rec=rec)
    sj, sstrides, slevel, srec, sstats = separate_jobs(hp, blocks, QP)
    S = dict(jobs=hp.make_tu_jobs(sj), strides=sstrides, level=slevel, rec=srec, stats=sstats)
    return blocks, resi_np, resi, J, S


def run_joint(hp, resi, J):
    hp.tu_rdo_joint(resi, J["items"], J["jobs"], J["strides"], J["joint_rec"], J["stats"], BD, joint=J["joint"], dist=J["dist"], rec=J["rec"], sse=J["sse"])


def step_check(args):
    import torch
    from vvenc_amd.hotpath import STATS_DTYPE, HotPath
    import ict_ref as IR
    hp = HotPath()
    blocks, resi_np, resi, J, S = world(hp, args.scale)
    for sparse in (0, 1):
        hp.tu_set_sparse_outputs(sparse)
        run_joint(hp, resi, J)
        torch.cuda.synchronize()
    hp.tu_set_sparse_outputs(0)
    items = J["items"]
    joint, dist, rec, sse = (J[k].cpu().numpy() for k in ("joint", "dist", "rec", "sse"))
    jrec, st = J["joint_rec"].cpu().numpy(), J["stats"].cpu().numpy().view(STATS_DTYPE).reshape(-1)
    n_zero = 0
    for k, (cbo, cro, _, w, h, m) in enumerate(blocks):
        cb, cr = resi_np[cbo:cbo + w * h].reshape(h, w), resi_np[cro:cro + w * h].reshape(h, w)
        ej, d1, d2 = IR.fwd(cb, cr, m)
        o = int(items[k]["joint_off"])
        assert np.array_equal(joint[o:o + w * h].reshape(h, w), ej) and (int(dist[k][0]), int(dist[k][1])) == (d1, d2), ("forward", k)
        zero = int(st[int(items[k]["stats_idx"])]["abs_sum"]) == 0
        n_zero += zero
        seen = np.zeros((h, w), np.int16) if zero else jrec[o:o + w * h].reshape(h, w)
        a, b = IR.inv(seen, m)
        assert np.array_equal(rec[cbo:cbo + w * h].reshape(h, w), a) and np.array_equal(rec[cro:cro + w * h].reshape(h, w), b), ("inverse", k)
        assert (int(sse[k][0]), int(sse[k][1])) == (IR.sse(a, cb), IR.sse(b, cr)), ("sse", k)
    print("check: %d chroma TUs, %d of them without levels at QP %d: the chain's outputs are the model's" % (len(blocks), n_zero, QP))
    assert 0 < n_zero < len(blocks)


def step_time(args):
    import torch
    from vvenc_amd.hotpath import HotPath
    hp = HotPath()
    blocks, resi_np, resi, J, S = world(hp, args.scale)
    hps = HotPath()          # a context per variant: each caches the job table of ONE TU list
    torch.cuda.synchronize()
    variants, first_call = {}, {}
    fns = {"joint": (hp, lambda: run_joint(hp, resi, J)), "separate": (hps, lambda: hps.tu_rdo_multi_strided(resi, S["strides"], S["jobs"], BD))}
    graphs = {}
    for name, (h, fn) in fns.items():
        h.use_own_stream()          # warm-up (schedules, job tables) on the stream the graph is recorded on
        t0 = time.perf_counter(); fn(); first_call[name] = time.perf_counter() - t0
        h.sync()
        graphs[name] = h.graph_capture(fn)
    variants["joint"] = lambda reps: ([hp.graph_launch(graphs["joint"]) for _ in range(reps)], hp.sync())
    variants["separate"] = lambda reps: ([hps.graph_launch(graphs["separate"]) for _ in range(reps)], hps.sync())
    if args.other_lib:
        ob = OtherBuild(args.other_lib, hp.device.index or 0)
        arr = (C.c_int32 * len(S["strides"]))(*S["strides"])
        gp = ob.capture(lambda: ob.ck(ob.L.vvhip_tu_rdo_multi_strided(ob.ctx, C.c_void_p(resi.data_ptr()), C.cast(arr, C.c_void_p), BD, S["jobs"][0], S["jobs"][1])))
        variants["parent"] = lambda reps: ob.run(gp, reps)
    rounds, reps = (1, 5) if args.quick else (args.rounds, args.reps)
    for fn in variants.values():          # warm-up
        fn(3)
    times = {k: [] for k in variants}
    for _ in range(rounds):
        for k, fn in variants.items():
            t0 = time.perf_counter()
            fn(reps)
            times[k].append((time.perf_counter() - t0) / reps * 1e6)
    out = {"scale": args.scale, "tus": len(blocks), "chroma_samples": int(resi_np.size), "qp": QP, "rounds": rounds, "reps": reps, "first_call_ms": {k: 1e3 * v for k, v in first_call.items()}}
    print("first call (host: sort, schedule, upload): " + ", ".join("%s %.2f ms" % (k, 1e3 * v) for k, v in first_call.items()))
    for k, v in times.items():
        v = np.array(v)
        out[k] = {"median_us": float(np.median(v)), "min_us": float(v.min()), "spread": float((v.max() - v.min()) / np.median(v))}
        print("%-9s median %9.1f us  min %9.1f us  spread %5.1f %%" % (k, out[k]["median_us"], out[k]["min_us"], 100 * out[k]["spread"]))
    out["joint_over_separate"] = out["joint"]["median_us"] / out["separate"]["median_us"]
    print("joint / separate = %.3f" % out["joint_over_separate"])
    if "parent" in out:
        out["separate_over_parent"] = out["separate"]["median_us"] / out["parent"]["median_us"]
        out["joint_over_parent"] = out["joint"]["median_us"] / out["parent"]["median_us"]
        print("separate / parent = %.3f   joint / parent = %.3f" % (out["separate_over_parent"], out["joint_over_parent"]))
    if args.json:
        with open(args.json, "w") as f:
            json.dump(out, f, indent=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--scale", type=int, default=1)
    ap.add_argument("--other-lib")
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
