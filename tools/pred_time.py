#!/usr/bin/env python3
"""tools/pred_time.py — what the prediction-list entry (vvhip_pred_inter_batch, vvenc_amd/csrc/pred.hip) costs on a 1920x1080 picture.

  python tools/pred_time.py [--rounds 9] [--reps 40] [--other-lib PATH] [--json PATH] [--quick] [--ciip-only]

A. the path it generalises: a picture's worth of luma 16x16 uni-prediction blocks (120 x 67 = 8040, seeded vectors within +-8 samples, all 256 phases) through
   vvhip_interp_luma_batch and through vvhip_pred_inter_batch — and, with --other-lib, through vvhip_interp_luma_batch of ANOTHER build of the library (the parent commit's)
   in the same rounds.  The two outputs of this build are compared sample for sample first.
B. the realistic list: a B picture's mix of prediction units — the fixed histogram PU_HIST below (synthetic: shaped like the motion-estimation records of the recorded 1080p
   lists, most samples in 64x64 and 32x32 units, most units 16x16 and smaller), half of the units bi-predicted (seeded), luma + both 4:2:0 chroma blocks per unit, residual
   output on.  Reported: time per picture, the bytes the algorithm reads and writes (per list the window (w + taps - 1) x (h + taps - 1), the original block, prediction and
   residual blocks; 2 bytes per sample) and their fraction of the HBM peak, the host time of a first call (sort + schedule + upload) and of a repeated call (the list is
   recognised).  The same list again with BDOF set on its true bi-predicted luma items that pass BDOF's size rule (vvhip_pred_inter_batch_ex), in the same rounds.
C. the affine mix: seeded affine CUs AFFINE_HIST (sizes 16..64, half bi-predicted, both models, control-point spread D = 32, luma + Cb + Cr, prof = 0) through
   vvhip_pred_affine_batch, and the same CUs expanded by the host into 4x4 items (tests/affine_ref.expand_items: what a caller had to do before) through
   vvhip_pred_inter_batch of the same build, in the same rounds; the outputs are compared first.  Then the same mix with prof = 1.  Reported besides the times: the host
   time of each first call and the bytes of list records and of device schedule each path uploads (from the record sizes of pred.hip / predaffine.hip).
D. the blend mix: seeded two-hypothesis CUs BLEND_HIST (the GEO size range 8..64, 1080p positions, luma + Cb + Cr), half of them BCW (index 0, 1, 3 or 4) and half GEO
   (any split direction), through vvhip_pred_inter_batch_blend — and the same items as plain bi-predicted items (blend = NULL: the cost floor of these blocks) through
   a second context, in the same rounds.  Reported: both times, their ratio, and how many samples the blend records change.
E. the CIIP mix: seeded CIIP CUs CIIP_HIST (the CIIP size range, 1080p positions, luma + Cb + Cr — the 2-wide chroma blocks of 4-wide CUs carry no CIIP, as in the
   reference), half of them bi-predicted, a third per num_intra value, each block's reference line taken from the row above and the column left of it in the list-0
   pictures, through vvhip_pred_inter_batch_ciip — and the same items with ciip = NULL (what these blocks cost without the intra part and the weighting: the cost
   floor) through a second context, in the same rounds.  Reported: both times, their ratio, and the share of samples the CIIP records change.  --ciip-only: this
   section alone.
Every variant is recorded into a launch graph once and timed as `reps` graph launches between two host clock readings that end in a device synchronise, `rounds` times, the
variants alternating inside a round; medians, minima and the spread ( max - min ) / median are printed.  --quick: one round of few launches (for a profiler run)."""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

W, H = 1920, 1080
HBM_PEAK = 8.0e12          # bytes / s (the figure bench.py's roofline uses)
# luma prediction units of one B picture: (width, height) -> count.  1.80 of the picture's 2.07 M luma samples are inter-predicted.
PU_HIST = {(64, 64): 150, (32, 32): 420, (64, 32): 60, (32, 64): 60, (32, 16): 160, (16, 32): 160, (16, 16): 900, (16, 8): 260, (8, 16): 260, (8, 8): 700, (8, 4): 120, (4, 8): 120}
SEED = 20240
# affine CUs of one picture: (width, height) -> count
AFFINE_HIST = {(64, 64): 60, (32, 32): 200, (64, 32): 40, (32, 64): 40, (32, 16): 100, (16, 32): 100, (16, 16): 500}
AFFINE_CTU, AFFINE_D = 128, 32
# two-hypothesis CUs with a blend record of one picture: (width, height) -> count
BLEND_HIST = {(64, 64): 30, (32, 32): 90, (64, 32): 20, (32, 64): 20, (32, 16): 50, (16, 32): 50, (16, 16): 160, (16, 8): 40, (8, 16): 40, (8, 8): 100}
# CIIP CUs of one picture: (width, height) -> count
CIIP_HIST = {(64, 64): 30, (32, 32): 90, (64, 32): 20, (32, 64): 20, (32, 16): 50, (16, 32): 50, (16, 16): 160, (16, 8): 40, (8, 16): 40, (8, 8): 100, (16, 4): 20, (4, 16): 20}


class OtherBuild:
    """vvhip_interp_luma_batch of another build of the library, through its own context (its own stream)"""

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
        L.vvhip_interp_luma_batch.argtypes = [vp, vp, i32, vp, i32, i32, i32, i32, i32, i32, i32, vp]
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


def chroma_of(y, k):
    return np.clip((y[::2, ::2].astype(np.int32) * (3 + k)) // 4 + 60 * k, 0, 1023).astype(np.int16)


def luma16_items(rng, stride):
    from vvenc_amd.hotpath import PRED_ITEM_DTYPE, SUBPEL_DTYPE
    bx, by = np.meshgrid(np.arange(W // 16), np.arange(H // 16))
    n = bx.size
    mvx, mvy = rng.integers(-8 * 16, 8 * 16 + 1, n), rng.integers(-8 * 16, 8 * 16 + 1, n)
    x, y = bx.ravel() * 16 + (mvx >> 4), by.ravel() * 16 + (mvy >> 4)
    sp = np.zeros(n, SUBPEL_DTYPE)
    sp["ref_off"], sp["frac_x"], sp["frac_y"] = y * stride + x, mvx & 15, mvy & 15
    it = np.zeros(n, PRED_ITEM_DTYPE)
    it["dst_off"], it["width"], it["height"] = np.arange(n) * 256, 16, 16
    it["ref_off"][:, 0], it["frac"][:, 0, 0], it["frac"][:, 0, 1] = sp["ref_off"], sp["frac_x"], sp["frac_y"]
    it["ref_plane"][:, 0], it["ref_plane"][:, 1] = 0, -1
    return sp, it


def b_picture_items(rng, luma_stride, chroma_stride, org_stride):
    """luma + Cb + Cr items of every unit of PU_HIST; planes 0 / 1: luma of list 0 / 1, 2 / 3: Cb, 4 / 5: Cr; the original picture is ONE buffer of row pitch org_stride
    (Y on top, Cb and Cr side by side below it).  -> (items, algorithmic bytes read, written)"""
    from vvenc_amd.hotpath import PRED_ITEM_DTYPE
    recs, at, rd, wr = [], 0, 0, 0
    for (w, h), count in PU_HIST.items():
        for _ in range(count):
            px, py = int(rng.integers(0, (W - w) // w + 1)) * w, int(rng.integers(0, (H - h) // h + 1)) * h
            bi = bool(rng.integers(0, 2))
            first = int(rng.integers(0, 2))
            mv = [(int(rng.integers(-128, 129)), int(rng.integers(-128, 129))) for _ in range(2)]
            for comp in range(3):
                cs = 1 if comp else 0
                it = np.zeros(1, PRED_ITEM_DTYPE)
                cw, chh, cx, cy = w >> cs, h >> cs, px >> cs, py >> cs
                it["width"], it["height"], it["chroma"], it["dst_off"] = cw, chh, cs, at
                it["org_off"] = cy * org_stride + cx if comp == 0 else (H + cy) * org_stride + (comp - 1) * (W // 2) + cx
                taps = 4 if cs else 8
                for l in (0, 1):
                    if not bi and l != first:
                        it["ref_plane"][0, l] = -1
                        continue
                    sh, stride = 4 + cs, chroma_stride if cs else luma_stride
                    it["ref_plane"][0, l] = 2 * comp + l
                    it["ref_off"][0, l] = (cy + (mv[l][1] >> sh)) * stride + cx + (mv[l][0] >> sh)
                    it["frac"][0, l] = (mv[l][0] & ((1 << sh) - 1), mv[l][1] & ((1 << sh) - 1))
                    rd += 2 * (cw + taps - 1) * (chh + taps - 1)
                rd += 2 * cw * chh
                wr += 4 * cw * chh
                at += cw * chh
                recs.append(it)
    items = np.concatenate(recs)
    return items[rng.permutation(len(items))], at, rd, wr


def affine_items(rng, prof):
    """luma + Cb + Cr items of every CU of AFFINE_HIST; planes 0 / 1: luma of list 0 / 1, 2 / 3: Cb, 4 / 5: Cr (offsets filled by the caller: they depend on the planes)"""
    from vvenc_amd.hotpath import PRED_AFFINE_ITEM_DTYPE
    recs = []
    for (w, h), count in AFFINE_HIST.items():
        for _ in range(count):
            it = np.zeros(1, PRED_AFFINE_ITEM_DTYPE)
            it["cu_w"], it["cu_h"], it["cu_x"], it["cu_y"] = w, h, int(rng.integers(0, (W - w) // w + 1)) * w, int(rng.integers(0, (H - h) // h + 1)) * h
            it["six_param"], it["prof"] = int(rng.integers(0, 2)), prof
            bi, first = bool(rng.integers(0, 2)), int(rng.integers(0, 2))
            for l in (0, 1):
                lt = rng.integers(-128, 129, 2)
                it["cpmv"][0, l, 0] = lt
                it["cpmv"][0, l, 1] = lt + rng.integers(-AFFINE_D * w // 16, AFFINE_D * w // 16 + 1, 2)
                it["cpmv"][0, l, 2] = lt + rng.integers(-AFFINE_D * h // 16, AFFINE_D * h // 16 + 1, 2)
                it["ref_plane"][0, l] = l if bi or l == first else -1
            for comp in range(3):
                c = it.copy()
                c["chroma"] = 1 if comp else 0
                c["ref_plane"] = np.where(it["ref_plane"] >= 0, it["ref_plane"] + 2 * comp, -1)
                recs.append(c)
    return np.concatenate(recs)


def blend_items(rng, luma_stride, chroma_stride):
    """luma + Cb + Cr items of every CU of BLEND_HIST, all with two hypotheses; planes as b_picture_items.  -> (items, blend records, samples)"""
    from vvenc_amd.hotpath import PRED_BLEND_BCW, PRED_BLEND_DTYPE, PRED_BLEND_GEO, PRED_ITEM_DTYPE
    recs, bl, at = [], [], 0
    for (w, h), count in BLEND_HIST.items():
        for k in range(count):
            px, py = int(rng.integers(0, (W - w) // w + 1)) * w, int(rng.integers(0, (H - h) // h + 1)) * h
            mv = [(int(rng.integers(-128, 129)), int(rng.integers(-128, 129))) for _ in range(2)]
            mode, param = (PRED_BLEND_BCW, int(rng.choice([0, 1, 3, 4]))) if k % 2 == 0 else (PRED_BLEND_GEO, int(rng.integers(0, 64)))
            for comp in range(3):
                cs = 1 if comp else 0
                it, b = np.zeros(1, PRED_ITEM_DTYPE), np.zeros(1, PRED_BLEND_DTYPE)
                cw, chh, cx, cy = w >> cs, h >> cs, px >> cs, py >> cs
                it["width"], it["height"], it["chroma"], it["dst_off"] = cw, chh, cs, at
                b["mode"], b["param"] = mode, param
                sh, stride = 4 + cs, chroma_stride if cs else luma_stride
                for l in (0, 1):
                    it["ref_plane"][0, l] = 2 * comp + l
                    it["ref_off"][0, l] = (cy + (mv[l][1] >> sh)) * stride + cx + (mv[l][0] >> sh)
                    it["frac"][0, l] = (mv[l][0] & ((1 << sh) - 1), mv[l][1] & ((1 << sh) - 1))
                at += cw * chh
                recs.append(it); bl.append(b)
    order = rng.permutation(len(recs))
    return np.concatenate(recs)[order], np.concatenate(bl)[order], at


def ciip_items(rng, luma_stride, chroma_stride, pics):
    """luma + Cb + Cr items of every CU of CIIP_HIST; planes as b_picture_items; pics: the host pictures (Y, Cb, Cr) the reference lines are cut from.
    -> (items, CIIP records, reference lines, samples)"""
    from vvenc_amd.hotpath import PRED_CIIP_DTYPE, PRED_CIIP_ON, PRED_ITEM_DTYPE
    padded = [np.pad(p, ((1, 2), (1, 2)), mode="edge") for p in pics]          # a block at the picture's edge takes the replicated neighbour
    recs, ci, lines, at, lat, k = [], [], [], 0, 0, 0
    for (w, h), count in CIIP_HIST.items():
        for _ in range(count):
            px, py = int(rng.integers(0, (W - w) // w + 1)) * w, int(rng.integers(0, (H - h) // h + 1)) * h
            bi, first = bool(rng.integers(0, 2)), int(rng.integers(0, 2))
            mv = [(int(rng.integers(-128, 129)), int(rng.integers(-128, 129))) for _ in range(2)]
            for comp in range(3):
                cs = 1 if comp else 0
                it, c = np.zeros(1, PRED_ITEM_DTYPE), np.zeros(1, PRED_CIIP_DTYPE)
                cw, chh, cx, cy = w >> cs, h >> cs, px >> cs, py >> cs
                it["width"], it["height"], it["chroma"], it["dst_off"] = cw, chh, cs, at
                sh, stride = 4 + cs, chroma_stride if cs else luma_stride
                for l in (0, 1):
                    if not bi and l != first:
                        it["ref_plane"][0, l] = -1
                        continue
                    it["ref_plane"][0, l] = 2 * comp + l
                    it["ref_off"][0, l] = (cy + (mv[l][1] >> sh)) * stride + cx + (mv[l][0] >> sh)
                    it["frac"][0, l] = (mv[l][0] & ((1 << sh) - 1), mv[l][1] & ((1 << sh) - 1))
                if cw >= 4:
                    P = padded[comp]
                    line = np.concatenate([P[cy, cx:cx + cw + 3], P[cy:cy + chh + 3, cx]])
                    c["mode"], c["num_intra"], c["ref_off"] = PRED_CIIP_ON, k % 3, lat
                    lines.append(line); lat += line.size
                at += cw * chh
                recs.append(it); ci.append(c)
            k += 1
    order = rng.permutation(len(recs))
    return np.concatenate(recs)[order], np.concatenate(ci)[order], np.concatenate(lines).astype(np.int16), at


def ciip_section(table, pics, a):
    """section E -> its result record"""
    import torch
    from vvenc_amd.hotpath import HotPath
    crng = np.random.default_rng(SEED + 3)
    citems, cciip, clines, ctotal = ciip_items(crng, table[0].stride, table[2].stride, pics)
    hpc, hpn = HotPath(), HotPath()
    d_lines = torch.from_numpy(clines).to(hpc.device)
    couts = [torch.zeros(ctotal, dtype=torch.int16, device=hpc.device) for _ in range(2)]
    cfns = {"ciip_batch": (hpc, lambda: hpc.pred_inter_batch(table, citems, couts[0], 0, 10, ciip=cciip, intra_ref=d_lines)),
            "same_items_no_ciip": (hpn, lambda: hpn.pred_inter_batch(table, citems, couts[1], 0, 10))}
    cgraphs, cfirst = {}, {}
    for name, (h, fn) in cfns.items():
        h.use_own_stream()
        t0 = time.perf_counter(); fn(); cfirst[name] = time.perf_counter() - t0
        h.sync()
        cgraphs[name] = h.graph_capture(fn)

    def run_ciip(name, reps):
        h = cfns[name][0]
        t0 = time.perf_counter()
        for _ in range(reps):
            h.graph_launch(cgraphs[name])
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / reps
    cnames = list(cfns)
    ctimes = {k: [] for k in cnames}
    for k in cnames:
        run_ciip(k, 5)
    for r in range(a.rounds):
        for k in (cnames if r % 2 == 0 else cnames[::-1]):
            ctimes[k].append(run_ciip(k, a.reps))
    cst = {k: stats(v) for k, v in ctimes.items()}
    on = cciip["mode"] == 1
    changed = int((couts[0] != couts[1]).sum().item())
    return {"cus": int(sum(CIIP_HIST.values())), "items": int(len(citems)), "ciip_items": int(on.sum()), "bi_items": int(((citems["ref_plane"][:, 0] >= 0) & (citems["ref_plane"][:, 1] >= 0)).sum()),
            "samples": int(ctotal), "line_samples": int(clines.size), **cst, "ratio_to_no_ciip": round(cst["ciip_batch"]["median_us"] / cst["same_items_no_ciip"]["median_us"], 3),
            "changed_samples": changed, "changed_share": round(changed / ctotal, 4), "host_first_call_us": {k: round(v * 1e6, 1) for k, v in cfirst.items()}}


def finish(res, a):
    for k, v in res.items():
        print(k, json.dumps(v) if isinstance(v, dict) else v)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)
    print(json.dumps(res))


def stats(ts):
    ts = sorted(ts)
    med = ts[len(ts) // 2]
    return {"median_us": round(med * 1e6, 2), "min_us": round(ts[0] * 1e6, 2), "spread": round((ts[-1] - ts[0]) / med, 4), "rounds": len(ts)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--other-lib", default=None, help="another build of libvvenc_hip.so: its vvhip_interp_luma_batch is timed in the same rounds")
    ap.add_argument("--json", default=None)
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--ciip-only", action="store_true", help="section E alone")
    a = ap.parse_args()
    if a.quick:
        a.rounds, a.reps = 1, 5
    import torch
    from vvenc_amd.hotpath import HotPath
    from vvenc_amd.workload import synth_frame_pair
    hp = HotPath()
    rng = np.random.default_rng(SEED)
    y0, y1 = synth_frame_pair(W, H, SEED)
    PAD = 32
    luma = [hp.plane(y0, PAD), hp.plane(y1, PAD)]
    chroma = [hp.plane(chroma_of(y, k), PAD) for k in (0, 1) for y in (y0, y1)]          # Cb list 0, Cb list 1, Cr list 0, Cr list 1
    planes = luma + chroma
    org_np = np.zeros((H + H // 2, W), np.int16)
    org_np[:H] = np.clip(y0.astype(np.int32) + rng.integers(-9, 10, y0.shape), 0, 1023)
    org_np[H:, :W // 2], org_np[H:, W // 2:] = chroma_of(y1, 0), chroma_of(y1, 1)
    org = hp.plane(org_np, 0)
    res = {"picture": [W, H], "rounds": a.rounds, "reps": a.reps}
    pics = [y0, chroma_of(y0, 0), chroma_of(y0, 1)]
    if a.ciip_only:
        res["ciip_mix"] = ciip_section([luma[0], luma[1], chroma[0], chroma[1], chroma[2], chroma[3]], pics, a)
        return finish(res, a)

    # ---- A: luma 16x16 uni-prediction, old entry / new entry / the other build's old entry
    sp, it = luma16_items(rng, luma[0].stride)
    n = len(sp)
    d_sp = hp.to_device(sp)
    out_old = torch.zeros(n * 256, dtype=torch.int16, device=hp.device)
    out_new = torch.zeros(n * 256, dtype=torch.int16, device=hp.device)
    out_oth = torch.zeros(n * 256, dtype=torch.int16, device=hp.device)
    hp.use_own_stream()          # warm-up (scratch, schedule upload) on the stream the graphs are recorded on
    old_fn = lambda: hp.interp_luma_batch(luma[0], d_sp, n, 16, 16, 10, True, 0, False, out=out_old)
    new_fn = lambda: hp.pred_inter_batch(planes[:1], it, out_new, 0, 10)
    old_fn(); new_fn(); hp.sync()
    assert torch.equal(out_old, out_new), "old and new entry disagree"
    variants = {"interp_luma_batch": hp.graph_capture(old_fn), "pred_inter_batch": hp.graph_capture(new_fn)}
    other = None
    if a.other_lib:
        other = OtherBuild(a.other_lib, hp.device.index or 0)
        vp = C.c_void_p
        g_oth = other.capture(lambda: other.ck(other.L.vvhip_interp_luma_batch(other.ctx, luma[0].buf_ptr, luma[0].stride, vp(d_sp.data_ptr()), n, 16, 16, 10, 1, 0, 0, vp(out_oth.data_ptr()))))
        assert torch.equal(out_old, out_oth), "the other build's vvhip_interp_luma_batch disagrees"

    def run(name, reps):
        t0 = time.perf_counter()
        if name == "other_build.interp_luma_batch":
            other.run(g_oth, reps)
        else:
            for _ in range(reps):
                hp.graph_launch(variants[name])
            torch.cuda.synchronize()
        return (time.perf_counter() - t0) / reps

    names = list(variants) + (["other_build.interp_luma_batch"] if other else [])
    times = {k: [] for k in names}
    for k in names:
        run(k, 5)
    for r in range(a.rounds):
        for k in (names if r % 2 == 0 else names[::-1]):
            times[k].append(run(k, a.reps))
    res["luma16x16_uni"] = {"items": n, **{k: stats(v) for k, v in times.items()}}

    # ---- B: the B picture's mix, residual on
    items, total, rd, wr = b_picture_items(rng, luma[0].stride, chroma[0].stride, org.stride)
    table = [luma[0], luma[1], chroma[0], chroma[1], chroma[2], chroma[3]]
    pred = torch.zeros(total, dtype=torch.int16, device=hp.device)
    resi = torch.zeros(total, dtype=torch.int16, device=hp.device)
    mix_fn = lambda: hp.pred_inter_batch(table, items, pred, 0, 10, org, resi)
    hp.use_own_stream()
    t0 = time.perf_counter(); mix_fn(); host_first = time.perf_counter() - t0
    hp.sync()
    t0 = time.perf_counter(); mix_fn(); host_again = time.perf_counter() - t0
    hp.sync()
    g_mix = hp.graph_capture(mix_fn)
    variants["b_picture"] = g_mix
    # the same list with BDOF on every true bi-predicted luma item the size rule admits (a second context: each context caches the schedule of ONE list)
    from vvenc_amd.hotpath import PRED_EXT_BDOF, PRED_EXT_DTYPE
    ext = np.zeros(len(items), PRED_EXT_DTYPE)
    on = (items["chroma"] == 0) & (items["ref_plane"][:, 0] >= 0) & (items["ref_plane"][:, 1] >= 0) & (np.minimum(items["width"], items["height"]) >= 8) & \
         (items["width"].astype(np.int32) * items["height"] >= 128)
    ext["flags"][on] = PRED_EXT_BDOF
    hp2 = HotPath()
    hp2.use_own_stream()
    pred2 = torch.zeros(total, dtype=torch.int16, device=hp.device)
    resi2 = torch.zeros(total, dtype=torch.int16, device=hp.device)
    bdof_fn = lambda: hp2.pred_inter_batch(table, items, pred2, 0, 10, org, resi2, ext=ext)
    bdof_fn(); hp2.sync()
    g_bdof = hp2.graph_capture(bdof_fn)

    def run_bdof(reps):
        t0 = time.perf_counter()
        for _ in range(reps):
            hp2.graph_launch(g_bdof)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / reps
    run("b_picture", 5); run_bdof(5)
    tm, tb = [], []
    for r in range(a.rounds):
        if r % 2 == 0:
            tm.append(run("b_picture", a.reps)); tb.append(run_bdof(a.reps))
        else:
            tb.append(run_bdof(a.reps)); tm.append(run("b_picture", a.reps))
    st, sb = stats(tm), stats(tb)
    sec = st["median_us"] * 1e-6
    res["b_picture_mix"] = {"units": int(sum(PU_HIST.values())), "items": int(len(items)), "bi_items": int(((items["ref_plane"][:, 0] >= 0) & (items["ref_plane"][:, 1] >= 0)).sum()),
                            "samples": int(total), **st, "bytes_read": int(rd), "bytes_written": int(wr), "achieved_GBps": round((rd + wr) / sec / 1e9, 1),
                            "hbm_peak_fraction": round((rd + wr) / sec / HBM_PEAK, 4), "host_first_call_us": round(host_first * 1e6, 1), "host_repeated_call_us": round(host_again * 1e6, 1)}
    res["b_picture_mix_bdof"] = {"items": int(len(items)), "bdof_items": int(on.sum()), "bdof_samples": int((items["width"].astype(np.int64) * items["height"])[on].sum()), **sb,
                                 "ratio_to_plain": round(sb["median_us"] / st["median_us"], 3), "changed_samples": int((pred2 != pred).sum().item())}
    # ---- C: the affine mix through vvhip_pred_affine_batch and, expanded into 4x4 items, through vvhip_pred_inter_batch; then with PROF
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import affine_ref as AR
    from vvenc_amd.hotpath import PRED_ITEM_DTYPE
    APAD = AFFINE_CTU + 16
    aplanes = [hp.plane(y0, APAD), hp.plane(y1, APAD)] + [hp.plane(chroma_of(y, k), APAD // 2) for k in (0, 1) for y in (y0, y1)]
    arng = np.random.default_rng(SEED + 1)
    aff = affine_items(arng, 0)
    sizes = (aff["cu_w"].astype(np.int64) >> aff["chroma"]) * (aff["cu_h"].astype(np.int64) >> aff["chroma"])
    aff["dst_off"] = np.concatenate([[0], np.cumsum(sizes)[:-1]])
    atotal = int(sizes.sum())
    strides = [p.stride for p in aplanes]
    for k in range(len(aff)):
        c = int(aff[k]["chroma"])
        for l in (0, 1):
            if aff[k]["ref_plane"][l] >= 0:
                aff[k]["ref_off"][l] = (int(aff[k]["cu_y"]) >> c) * strides[int(aff[k]["ref_plane"][l])] + (int(aff[k]["cu_x"]) >> c)          # (Plane.buf_ptr addresses sample (0, 0))
    t0 = time.perf_counter()
    ex = []
    for k in range(len(aff)):
        e, _, _ = AR.expand_items(aff[k], strides, W, H, AFFINE_CTU, PRED_ITEM_DTYPE)
        e["dst_off"] += int(aff[k]["dst_off"])
        ex.append(e)
    ex = np.concatenate(ex)
    expand_s = time.perf_counter() - t0
    hpa, hpe, hpp = HotPath(), HotPath(), HotPath()
    outs = [torch.zeros(atotal, dtype=torch.int16, device=hp.device) for _ in range(3)]
    affp = aff.copy()
    affp["prof"] = 1
    fns = {"affine_batch": (hpa, lambda: hpa.pred_affine_batch(aplanes, aff, outs[0], 0, 10, W, H, AFFINE_CTU)),
           "expanded_4x4_inter_batch": (hpe, lambda: hpe.pred_inter_batch(aplanes, ex, outs[1], 0, 10)),
           "affine_batch_prof": (hpp, lambda: hpp.pred_affine_batch(aplanes, affp, outs[2], 0, 10, W, H, AFFINE_CTU))}
    first_call, graphs = {}, {}
    for name, (h, fn) in fns.items():
        h.use_own_stream()
        t0 = time.perf_counter(); fn(); first_call[name] = time.perf_counter() - t0
        h.sync()
        graphs[name] = h.graph_capture(fn)
    a_np, e_np = outs[0].cpu().numpy(), outs[1].cpu().numpy()
    for k in range(len(aff)):
        c, o = int(aff[k]["chroma"]), int(aff[k]["dst_off"])
        bw, bh = int(aff[k]["cu_w"]) >> c, int(aff[k]["cu_h"]) >> c
        assert np.array_equal(AR.blocks_to_block(e_np[o:o + bw * bh], bw, bh), a_np[o:o + bw * bh].reshape(bh, bw)), ("the affine entry and the expanded list disagree on item", k)

    def run_aff(name, reps):
        h = fns[name][0]
        t0 = time.perf_counter()
        for _ in range(reps):
            h.graph_launch(graphs[name])
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / reps
    anames = list(fns)
    atimes = {k: [] for k in anames}
    for k in anames:
        run_aff(k, 5)
    for r in range(a.rounds):
        for k in (anames if r % 2 == 0 else anames[::-1]):
            atimes[k].append(run_aff(k, a.reps))
    ast = {k: stats(v) for k, v in atimes.items()}
    tiles = int(sum(max(1, (int(i["cu_w"]) >> int(i["chroma"])) * (int(i["cu_h"]) >> int(i["chroma"])) // 256) for i in aff))
    allow = max(ast["affine_batch"]["spread"], ast["expanded_4x4_inter_batch"]["spread"]) * ast["expanded_4x4_inter_batch"]["median_us"]
    res["affine_mix"] = {"cus": int(sum(AFFINE_HIST.values())), "items": int(len(aff)), "expanded_items": int(len(ex)), "samples": atotal, "outputs_equal": True,
                         **{k: v for k, v in ast.items()},
                         "condition_affine_not_slower_than_expanded_plus_spread": bool(ast["affine_batch"]["median_us"] <= ast["expanded_4x4_inter_batch"]["median_us"] + allow),
                         "host_first_call_us": {k: round(v * 1e6, 1) for k, v in first_call.items()}, "host_expansion_ms": round(expand_s * 1e3, 1),
                         "record_bytes": {"affine_batch": int(len(aff)) * 80, "expanded_4x4_inter_batch": int(len(ex)) * 32},
                         "schedule_bytes": {"affine_batch": int(len(aff)) * 96 + tiles * 8 + ((tiles + 3) // 4) * 4 * 16, "expanded_4x4_inter_batch": int(len(ex)) * (48 + 8) + ((len(ex) + 63) // 64) * 4 * 16},
                         "prof_changed_samples": int((outs[2] != outs[0]).sum().item()), "prof_ratio_to_plain": round(ast["affine_batch_prof"]["median_us"] / ast["affine_batch"]["median_us"], 3)}
    # ---- D: the blend mix through vvhip_pred_inter_batch_blend, and the same items as plain bi-predicted items
    brng = np.random.default_rng(SEED + 2)
    bitems, bblend, btotal = blend_items(brng, luma[0].stride, chroma[0].stride)
    hpb, hpn = HotPath(), HotPath()
    bouts = [torch.zeros(btotal, dtype=torch.int16, device=hp.device) for _ in range(2)]
    bfns = {"blend_batch": (hpb, lambda: hpb.pred_inter_batch(table, bitems, bouts[0], 0, 10, blend=bblend)),
            "same_items_plain_bi": (hpn, lambda: hpn.pred_inter_batch(table, bitems, bouts[1], 0, 10))}
    bgraphs, bfirst = {}, {}
    for name, (h, fn) in bfns.items():
        h.use_own_stream()
        t0 = time.perf_counter(); fn(); bfirst[name] = time.perf_counter() - t0
        h.sync()
        bgraphs[name] = h.graph_capture(fn)

    def run_blend(name, reps):
        h = bfns[name][0]
        t0 = time.perf_counter()
        for _ in range(reps):
            h.graph_launch(bgraphs[name])
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / reps
    bnames = list(bfns)
    btimes = {k: [] for k in bnames}
    for k in bnames:
        run_blend(k, 5)
    for r in range(a.rounds):
        for k in (bnames if r % 2 == 0 else bnames[::-1]):
            btimes[k].append(run_blend(k, a.reps))
    bst = {k: stats(v) for k, v in btimes.items()}
    res["blend_mix"] = {"cus": int(sum(BLEND_HIST.values())), "items": int(len(bitems)), "bcw_items": int((bblend["mode"] == 1).sum()), "geo_items": int((bblend["mode"] == 2).sum()),
                        "samples": int(btotal), **bst, "ratio_to_plain": round(bst["blend_batch"]["median_us"] / bst["same_items_plain_bi"]["median_us"], 3),
                        "changed_samples": int((bouts[0] != bouts[1]).sum().item()), "host_first_call_us": {k: round(v * 1e6, 1) for k, v in bfirst.items()}}
    # ---- E: the CIIP mix through vvhip_pred_inter_batch_ciip, and the same items without their CIIP records
    res["ciip_mix"] = ciip_section(table, pics, a)
    finish(res, a)


if __name__ == "__main__":
    main()
