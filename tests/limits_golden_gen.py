"""Second, seeded case lists of the four fixture generators tests/{bdof,blend,ciip,affine}_golden_gen.cpp: the 12-bit anchors of tests/test_oracle_pred_ext_extremes.py.
The generators are the ones of the first lists (compile commands in their header comments; nothing of them changes: none refuses 12 bits), the record formats are those
of tests/{bdof,blend,ciip,affine}_golden_gen.py, whose case families are restated here with the bit depth, the seed and the counts as arguments; the existing fixtures
are not touched.  Writes, arrays only:
  bdof    tests/golden/bdof_limits.npz    the four families of bdof.npz at 12 bits, and, at 8, 10 and 12 bits, the frames the int64 model of tests/pred_ext_extremes.py
                                          derives from its two-level planes for a part of the lists the GPU tier runs (BDOF units, the low-noise pictures, DMVR sub-blocks
                                          with BDOF; of a 64x64 item its first two units), so that the reference's own xApplyBDOF has seen exactly those frames
  blend   tests/golden/blend_limits.npz   the weight blocks of four CU sizes through the reference function at 12 bits ( s0 = -8160, s1 = -8192: ( 32 w + 16 ) >> 5 = w ) and
                                          seeded BCW, GEO and checkerboard cases at 12 bits, the checkerboard ones drawn from tests/pred_ext_extremes.blend_list
  ciip    tests/golden/ciip_limits.npz    the sweep (sizes up to 1024 samples) and the extremes of ciip.npz at 12 bits, and the items of tests/pred_ext_extremes.ciip_list( 12 )
                                          (of the 64x64 and 32x32 items every second one), the inter block being the clipped inter part of the int64 interpolation model
  affine  tests/golden/affine_limits.npz  40 seeded cases of the families of affine.npz at 12 bits on 12-bit planes (the generator takes the planes as they are for every bit
                                          depth but 8; `plane_bd` in the file says what they hold) with 0 / 4095 checkerboard patches, and eight zooms and shears of 11 / 16 on
                                          the patches that drive the dMv table to +-31 and dI into its clip
usage: python tests/limits_golden_gen.py bdof|blend|ciip|affine /path/to/<that generator>"""
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import affine_cases as AC  # noqa: E402
import affine_ref as AR  # noqa: E402
import bdof_cases as BC  # noqa: E402
import blend_cases as BLC  # noqa: E402
import blend_ref as BL  # noqa: E402
import ciip_ref as CR  # noqa: E402
import pred_ext_extremes as E  # noqa: E402
import pred_ref as PR  # noqa: E402

GOLDEN = os.path.join(HERE, "golden")


# ---- BDOF ( format and families: tests/bdof_golden_gen.py ) -------------------------------------------------------------------------
SHAPES = [(16, 16), (16, 8), (8, 16)]


def bdof_families(bds, seed, pictures, noise):
    rng = np.random.default_rng(seed)
    out = []
    for bd in bds:
        hr, top = max(2, 14 - bd), (1 << bd) - 1
        lo, hi = -8192, (top << hr) - 8192

        def conv(a):
            return ((np.asarray(a).astype(np.int32) << hr) - 8192).astype(np.int16)

        for (w, h) in SHAPES:
            yy, xx = np.mgrid[0:h + 2, 0:w + 2].astype(np.float64)
            for k in range(pictures):          # pictures
                def pic(dx, dy):
                    return np.clip(top / 2 + top / 3 * np.sin((xx + dx) / (2.0 + k)) * np.cos((yy + dy) / (3.0 + k)) + rng.normal(0, top / (8 + 10 * k), xx.shape), 0, top)
                d = rng.uniform(-1.5, 1.5, 2)
                out.append((bd, w, h, conv(np.round(pic(0, 0))), conv(np.round(pic(d[0], d[1])))))
            for (a, b) in ((lo, lo), (hi, hi), (lo, hi), (0, 0), (100, -300), (hi, lo)):          # flat
                out.append((bd, w, h, np.full((h + 2, w + 2), a, np.int16), np.full((h + 2, w + 2), b, np.int16)))
            for sx, sy, sd in ((1, 1, 1), (1, 1, -1), (-1, 1, 1), (1, -1, -1), (1, 0, 1), (0, 1, -1)):          # ramps: gradient of the same sign in both lists, a large difference
                g = 96
                base = np.clip(sx * g * (xx - w / 2) + sy * g * (yy - h / 2), lo // 2, hi // 2)
                f0 = np.clip(base - sd * 1500, lo, hi).astype(np.int16)
                f1 = np.clip(base + sd * 1500, lo, hi).astype(np.int16)
                out.append((bd, w, h, f0, f1))
            for k in range(4):          # extremes: 0 and max
                m = rng.integers(0, 2, (h + 2, w + 2)) if k < 2 else ((xx.astype(int) // (k + 1) + yy.astype(int) // (k + 1)) & 1)
                m2 = rng.integers(0, 2, (h + 2, w + 2)) if k % 2 == 0 else 1 - m
                out.append((bd, w, h, conv(m * top), conv(m2 * top)))
            for k in noise:          # everything the 14-bit intermediate can hold, and beyond it: the int16 cast of the output
                span = (lo, hi + 1) if k < 2 else (-32768, 32768)
                out.append((bd, w, h, rng.integers(span[0], span[1], (h + 2, w + 2)).astype(np.int16), rng.integers(span[0], span[1], (h + 2, w + 2)).astype(np.int16)))
    return out


def bdof_cases():
    """12-bit cases of every family of bdof.npz, then the frames of the two-level planes at all three bit depths (a part of every list of the GPU tier; of a 64x64 item its
    first two units)"""
    out = bdof_families((12,), 20251, 2, (1, 2))
    for bd in E.BITDEPTHS:
        pl = E.planes(bd)
        for (items, ext, pos), step in ((E.bdof_list(bd), 6), (E.ramp_list(bd), 18), (E.dmvr_list(bd), 12)):
            keep = [k for k in range(len(items)) if int(ext[k]["flags"]) & 1][::step]
            for k in keep:
                for (x0, y0, uw, uh, f0, f1) in E.unit_frames(pl, pos[k], items[k], ext[k], bd)[:2]:
                    out.append((bd, uw, uh, f0.astype(np.int16), f1.astype(np.int16)))
    return out


def bdof_main(exe):
    cs = bdof_cases()
    with tempfile.TemporaryDirectory() as td:
        fi, fo = os.path.join(td, "in.bin"), os.path.join(td, "out.bin")
        with open(fi, "wb") as f:
            f.write(np.int32(len(cs)).tobytes())
            for (bd, w, h, f0, f1) in cs:
                f.write(np.array([bd, w, h], np.int32).tobytes() + np.ascontiguousarray(f0).tobytes() + np.ascontiguousarray(f1).tobytes())
        subprocess.check_call([exe, fi, fo])
        raw = np.fromfile(fo, np.int16)
    arrays, at = {"n": np.int32(len(cs))}, 0
    for i, (bd, w, h, f0, f1) in enumerate(cs):
        arrays["c%03d_hdr" % i] = np.array([bd, w, h], np.int32)
        arrays["c%03d_f0" % i], arrays["c%03d_f1" % i] = f0, f1
        arrays["c%03d_scalar" % i] = raw[at:at + w * h].reshape(h, w); at += w * h
        arrays["c%03d_simd" % i] = raw[at:at + w * h].reshape(h, w); at += w * h
    assert at == raw.size
    dst = os.path.join(GOLDEN, "bdof_limits.npz")
    np.savez_compressed(dst, **arrays)
    print("%d cases -> %s (%d bytes)" % (len(cs), dst, os.path.getsize(dst)))


# ---- BCW, GEO ( format and families: tests/blend_golden_gen.py ) ---------------------------------------------------------------------
LIMITS_WEIGHT_SIZES = [(8, 8), (16, 32), (32, 8), (64, 64)]


def weight_blocks(sizes=LIMITS_WEIGHT_SIZES):
    return [(sd, w, h, c) for sd in range(64) for (w, h) in sizes for c in (0, 1)]


def intermediate(orc, pl, pos, it, l, bd):
    """the 14-bit block of one hypothesis from the numpy model of the two passes"""
    w, h, chroma = int(it["width"]), int(it["height"]), int(it["chroma"])
    arr, (x, y) = pl[int(it["ref_plane"][l])], pos[l]
    xf, yf = int(it["frac"][l][0]), int(it["frac"][l][1])
    s, lo, nt = (2, 1, 4) if chroma else (1 if (w, h) == (4, 4) else 0, 3, 8)
    th = ([int(c) for c in orc.if_coeff(s, xf)[1][:nt]], lo) if xf else ([64], 0)
    tv = ([int(c) for c in orc.if_coeff(s, yf)[1][:nt]], lo) if yf else ([64], 0)
    return PR.kernel_form(th[0], th[1], tv[0], tv[1], arr, y, x, w, h, False, bd)


def blend_cases(orc, bds=(12,), n_extremes=30, plane_seed=100, extremes_seed=500):
    out = []
    for bd in bds:
        pl, _ = BLC.planes(bd, plane_seed + bd)
        rng = np.random.default_rng(50 + bd)
        picked = []
        items, _, blend, pos = BLC.bcw_list(pl, 60 + bd)
        keep = [k for k in range(len(items)) if int(items[k]["width"]) * int(items[k]["height"]) <= 1024 and not int(items[k]["alt_hpel"])]
        picked += [(items[k], blend[k], pos[k]) for k in rng.choice(keep, 9, replace=False)]
        items, _, blend, pos = BLC.geo_list(pl, 70 + bd)
        keep = [k for k in range(len(items)) if int(items[k]["width"]) * int(items[k]["height"]) <= 1024 and not int(items[k]["alt_hpel"])]
        picked += [(items[k], blend[k], pos[k]) for k in rng.choice(keep, 9, replace=False)]
        items, _, blend, pos = BLC.extremes_list(pl, extremes_seed + bd)
        keep = [k for k in range(len(items)) if int(items[k]["width"]) <= 32]
        picked += [(items[k], blend[k], pos[k]) for k in rng.choice(keep, n_extremes, replace=False)]
        for it, bl, p in picked:
            s0, s1 = (intermediate(orc, pl, p, it, l, bd) for l in (0, 1))
            out.append((int(bl["mode"]), bd, int(it["width"]), int(it["height"]), int(it["chroma"]), int(bl["param"]), s0, s1))
    return out


def blend_main(exe):
    from oracle.oracle import Oracle
    cs = blend_cases(Oracle())
    wb = weight_blocks()
    wbd, ws0 = 12, -8160
    with tempfile.TemporaryDirectory() as td:
        fi, fo = os.path.join(td, "in.bin"), os.path.join(td, "out.bin")
        with open(fi, "wb") as f:
            f.write(np.int32(len(wb) + len(cs)).tobytes())
            for (sd, w, h, c) in wb:
                bw, bh = w >> c, h >> c
                f.write(np.array([2, wbd, bw, bh, c, sd], np.int32).tobytes() + np.full(bw * bh, ws0, np.int16).tobytes() + np.full(bw * bh, -8192, np.int16).tobytes())
            for (kind, bd, w, h, c, param, s0, s1) in cs:
                f.write(np.array([kind, bd, w, h, c, param], np.int32).tobytes() + np.ascontiguousarray(s0, np.int16).tobytes() + np.ascontiguousarray(s1, np.int16).tobytes())
        subprocess.check_call([exe, fi, fo])
        raw = np.fromfile(fo, np.int16)
    at, ws, wx = 0, [], []
    for (sd, w, h, c) in wb:
        n = (w >> c) * (h >> c)
        ws.append(raw[at:at + n]); wx.append(raw[at + n:at + 2 * n]); at += 2 * n
    ws, wx = np.concatenate(ws), np.concatenate(wx)
    assert ws.min() == 0 and ws.max() == 8 and np.array_equal(ws, wx), "weight blocks: rows differ or out of range"
    arrays = {"n": np.int32(len(cs)), "weights_scalar": ws.astype(np.int8), "weights_simd": wx.astype(np.int8)}
    for i, (kind, bd, w, h, c, param, s0, s1) in enumerate(cs):
        arrays["c%03d_hdr" % i] = np.array([kind, bd, w, h, c, param], np.int32)
        arrays["c%03d_s0" % i], arrays["c%03d_s1" % i] = s0, s1
        arrays["c%03d_scalar" % i] = raw[at:at + w * h].reshape(h, w); at += w * h
        arrays["c%03d_simd" % i] = raw[at:at + w * h].reshape(h, w); at += w * h
        assert np.array_equal(arrays["c%03d_scalar" % i], arrays["c%03d_simd" % i]), "case %d: the reference's scalar row and x86 row differ" % i
    assert at == raw.size
    dst = os.path.join(GOLDEN, "blend_limits.npz")
    np.savez_compressed(dst, **arrays)
    print("%d weight samples, %d cases -> %s (%d bytes)" % (ws.size, len(cs), dst, os.path.getsize(dst)))


# ---- CIIP ( format and families: tests/ciip_golden_gen.py ) -------------------------------------------------------------------------
EXTREME_SIZES = [(8, 8, 0), (4, 16, 0), (16, 4, 0), (16, 16, 0), (4, 4, 1), (8, 2, 1), (8, 8, 1)]


def ciip_families(bds, seed, max_samples):
    """-> list of ( bd, w, h, chroma, num_intra, line, inter )"""
    out = []
    pics = {}
    for bd in bds:
        rng = np.random.default_rng(seed + bd)
        pics[bd] = (BC._picture(rng, 140, 160, bd, 0.0), BC._picture(rng, 140, 160, bd, 2.9), rng)

    def seeded(bd, w, h, chroma, ni):
        a, b, rng = pics[bd]
        x, y = int(rng.integers(1, 160 - w - 2)), int(rng.integers(1, 140 - h - 2))
        bx, by = int(rng.integers(0, 160 - w)), int(rng.integers(0, 140 - h))
        out.append((bd, w, h, chroma, ni, CR.line_at(a, x, y, w, h), b[by:by + h, bx:bx + w].copy()))
    sizes = [(w, h, 0) for (w, h) in CR.LUMA_SIZES] + [(w, h, 1) for (w, h) in CR.CHROMA_SIZES]
    for k, (w, h, c) in enumerate(sizes):
        if w * h > max_samples:
            continue
        seeded(bds[0] if k % 2 else bds[-1], w, h, c, k % 3)
    for k, (w, h, c) in enumerate(sizes):
        if w * h <= 256 and len(bds) > 1:
            seeded(bds[-1] if k % 2 else bds[0], w, h, c, (k + 1) % 3)
    k = 0
    for bd in bds:
        top = (1 << bd) - 1
        for (w, h, c) in EXTREME_SIZES:
            n = CR.line_len(w, h)
            alt = np.concatenate([(np.arange(w + 3) & 1) * top, (np.arange(h + 3) & 1) * top]).astype(np.int16)      # top[0] == left[0] == 0
            for line, blk in ((np.zeros(n, np.int16), 0), (np.full(n, top, np.int16), top), (alt, top), ((top - alt).astype(np.int16), 0),
                              (np.zeros(n, np.int16), top), (np.full(n, top, np.int16), 0)):
                out.append((bd, w, h, c, k % 3, line, np.full((h, w), blk, np.int16)))
                k += 1
    return out


def ciip_cases():
    out = ciip_families((12,), 930, 1024)          # (the sweep up to 1024 samples: the file's size; the 64x64 luma block is among the items of the GPU list)
    pl, items, ext, blend, ciip, lines, pos = E.ciip_list(12)
    for k, it in enumerate(items):
        w, h, o = int(it["width"]), int(it["height"]), int(ciip[k]["ref_off"])
        if w * h >= 1024 and (k // 4 + k % 4) % 2:          # of the 64x64 and 32x32 items every second one: each line and each kind still twice
            continue
        out.append((12, w, h, int(it["chroma"]), int(ciip[k]["num_intra"]), lines[o:o + CR.line_len(w, h)].copy(), E.ciip_inter(pl, pos[k], it, blend[k], 12)))
    return out


def ciip_main(exe):
    cs = ciip_cases()
    dst = os.path.join(GOLDEN, "ciip_limits.npz")
    with tempfile.TemporaryDirectory() as td:
        fi, fo = os.path.join(td, "in.bin"), os.path.join(td, "out.bin")
        with open(fi, "wb") as f:
            f.write(np.int32(len(cs)).tobytes())
            for (bd, w, h, c, ni, line, inter) in cs:
                assert line.size == CR.line_len(w, h) and inter.shape == (h, w) and line[0] == line[w + 3]
                f.write(np.array([bd, w, h, c, ni], np.int32).tobytes() + np.ascontiguousarray(line, np.int16).tobytes() + np.ascontiguousarray(inter, np.int16).tobytes())
        subprocess.check_call([exe, fi, fo])
        raw = np.fromfile(fo, np.int16)
    at, arrays = 0, {"n": np.int32(len(cs))}
    seen = set()
    for i, (bd, w, h, c, ni, line, inter) in enumerate(cs):
        rows = []
        for _ in range(2):
            rows.append((raw[at:at + w * h].reshape(h, w), raw[at + w * h:at + 2 * w * h].reshape(h, w)))
            at += 2 * w * h
        assert np.array_equal(rows[0][0], rows[1][0]) and np.array_equal(rows[0][1], rows[1][1]), "case %d: the reference's scalar row and x86 row differ" % i
        flat = line.min() == line.max() == inter.min() == inter.max()
        assert np.array_equal(rows[0][1], inter) == bool(flat), "case %d: the result %s the inter block" % (i, "differs from" if flat else "equals")
        arrays["c%03d_hdr" % i] = np.array([bd, w, h, c, ni], np.int32)
        arrays["c%03d_line" % i], arrays["c%03d_inter" % i] = line, inter
        arrays["c%03d_intra" % i], arrays["c%03d_result" % i] = rows[0]
        seen.add((w, h, c)); seen.add(("ni", ni)); seen.add(("bd", bd))
    assert at == raw.size
    assert all(("ni", k) in seen for k in range(3))
    np.savez_compressed(dst, **arrays)
    print("%d cases -> %s (%d bytes)" % (len(cs), dst, os.path.getsize(dst)))


# ---- affine ( format and families: tests/affine_golden_gen.py ) ---------------------------------------------------------------------
PIC_W, PIC_H, CTU, MARGIN = 128, 96, 32, 48


def affine_planes(bd=12):
    """-> [y0, c0, y1, c1]: smooth texture + a little noise (it compresses), with a 0 / max checkerboard patch in each luma plane"""
    w = AC.World(bd, CTU, "texture", seed=4242, pic_w=PIC_W, pic_h=PIC_H, margin=MARGIN)
    out = []
    for p in (0, 1):
        y = (w.np[p][:PIC_H + 2 * MARGIN] & ~3).astype(np.int16)
        yy, xx = np.mgrid[0:24, 0:32]
        y[MARGIN + 40:MARGIN + 64, MARGIN + 20 + 50 * p:MARGIN + 52 + 50 * p] = ((xx + yy) & 1) * ((1 << bd) - 1)
        out += [y, (w.np[2 + p][:PIC_H // 2 + MARGIN] & ~3).astype(np.int16)]
    return out


def affine_families(seed, n_cases, bd_of):
    rng = np.random.default_rng(seed)
    rows, k = [], 0
    while len(rows) < n_cases:
        w, h = (int(rng.choice([8, 16, 32, 64], p=[0.3, 0.35, 0.25, 0.1])) for _ in (0, 1))
        x, y = 8 * int(rng.integers(0, (PIC_W - w) // 8 + 1)), 8 * int(rng.integers(0, (PIC_H - h) // 8 + 1))
        D = (4, 32, 256)[k % 3]
        far = k % 7 == 6 and max(w, h) <= 32
        lt = None
        if far:
            ex, ey = int(rng.integers(-1, 2)), int(rng.choice([-1, 1]))
            lt = [(ex * 70 * 16 + int(rng.integers(-40, 41)), ey * 70 * 16 + int(rng.integers(-40, 41))) for _ in (0, 1)]
        lu, _ = AC._cu(rng, w, h, x, y, k & 1, (k >> 1) % 3, (k // 6) % 4, D, lt_range=384, lt=lt)
        ch = lu.copy()
        ch["chroma"] = 1
        if any(e > m for it, m in ((lu, MARGIN), (ch, MARGIN // 2)) for e in AR.read_extent(it, PIC_W, PIC_H, CTU)):
            continue
        inter_dir = (1 if lu["ref_plane"][0] >= 0 else 0) | (2 if lu["ref_plane"][1] >= 0 else 0)
        rows.append([bd_of(k), x, y, w, h, k & 1, inter_dir, int(lu["prof"]), max(int(lu["ref_plane"][0]), 0), max(int(lu["ref_plane"][1]), 0)] +
                    [int(v) for v in lu["cpmv"].reshape(-1)])
        k += 1
    return np.array(rows, np.int32)


def affine_cases():
    """40 seeded cases at 12 bits, then zooms and shears of 11 / 16 (|dMv| reaches 31) on the checkerboard patch of each picture, uni- and bi-predicted, both models"""
    cs = affine_families(31338, 40, lambda k: 12)
    rng = np.random.default_rng(31339)
    rows = []
    for k, (zx, zy) in enumerate(((11, 0), (-11, 0), (0, 11), (0, -11), (11, 11), (-11, 11), (11, -11), (-11, -11))):
        p = k & 1
        w, h = ((16, 16), (16, 8), (8, 16), (16, 16))[k % 4]
        x, y = 24 + 48 * p, 40          # inside the patch of picture p: x 20 + 50 p .. 52 + 50 p, y 40 .. 64
        lu, _ = AC._cu(rng, w, h, x, y, (k >> 1) & 1, 2 if k >= 4 else p, 1, 0, lt_range=16)
        for l in (0, 1):
            if lu["ref_plane"][l] >= 0:
                lu["ref_plane"][l] = p
            a = lu["cpmv"][l][0].copy()
            lu["cpmv"][l][1] = a + np.array([zx * w, zy * w])
            lu["cpmv"][l][2] = a + np.array([-zy * h, zx * h])
        ch = lu.copy()
        ch["chroma"] = 1
        assert all(e <= m for it, m in ((lu, MARGIN), (ch, MARGIN // 2)) for e in AR.read_extent(it, PIC_W, PIC_H, CTU))
        inter_dir = (1 if lu["ref_plane"][0] >= 0 else 0) | (2 if lu["ref_plane"][1] >= 0 else 0)
        rows.append([12, x, y, w, h, (k >> 1) & 1, inter_dir, 1, max(int(lu["ref_plane"][0]), 0), max(int(lu["ref_plane"][1]), 0)] + [int(v) for v in lu["cpmv"].reshape(-1)])
    return np.concatenate([cs, np.array(rows, np.int32)])


def affine_main(exe):
    pl, cs = affine_planes(12), affine_cases()
    with tempfile.TemporaryDirectory() as td:
        fi, fo = os.path.join(td, "in.bin"), os.path.join(td, "out.bin")
        with open(fi, "wb") as f:
            f.write(np.array([PIC_W, PIC_H, CTU, MARGIN, len(cs)], np.int32).tobytes())
            for p in pl:
                f.write(np.ascontiguousarray(p).tobytes())
            f.write(cs.tobytes())
        subprocess.check_call([exe, fi, fo])
        raw = np.fromfile(fo, np.int16)
    # the generator writes, per case: scalar row ( per list: luma, Cb ), then the x86 row
    scalar, simd, at = [], [], 0
    for c in cs:
        n = (c[3] * c[4] + c[3] * c[4] // 4) * (2 if c[6] == 3 else 1)
        scalar.append(raw[at:at + n]); at += n
        simd.append(raw[at:at + n]); at += n
    assert at == raw.size
    dst = os.path.join(GOLDEN, "affine_limits.npz")
    np.savez_compressed(dst, plane_bd=np.int32(12), hdr=np.array([PIC_W, PIC_H, CTU, MARGIN], np.int32), y0=pl[0], c0=pl[1], y1=pl[2], c1=pl[3], cases=cs,
                        scalar=np.concatenate(scalar), simd=np.concatenate(simd))
    print("%d cases -> %s (%d bytes)" % (len(cs), dst, os.path.getsize(dst)))


if __name__ == "__main__":
    {"bdof": bdof_main, "blend": blend_main, "ciip": ciip_main, "affine": affine_main}[sys.argv[1]](sys.argv[2])
