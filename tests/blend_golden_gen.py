"""Driver of tests/blend_golden_gen.cpp: builds the recorded inputs, runs the generator (its path is argv[1]; compile command in its header comment) and writes
tests/golden/blend.npz — arrays only.

(a) weights   every GEO weight block, taken through the reference function itself: 64 split directions x 16 CU sizes x { luma, chroma } at 10 bit with s0 = -8064 and
              s1 = -8192 everywhere, where ( w * s0 + ( 8 - w ) * s1 + 64 + 65536 ) >> 7 = ( 128 w + 64 ) >> 7 = w.  Stored as one int8 vector per row of the reference
              (scalar, x86), the blocks one after the other in the order of weight_blocks().
(b) cases     seeded BCW and GEO cases at bit depths 8 and 10, luma and chroma.  The two input blocks are real 14-bit intermediates: the rnd_res = 0 output of
              pred_ref.kernel_form on the planes of tests/blend_cases.py — pictures, and the 0 / max checkerboards at half-sample fractions, where the taps overshoot and
              meet the weights -2 / 10 and both clip ends.  (No arbitrary int16 inputs: the x86 rows are only specified on the range the interpolation produces.)
              Per case: hdr = [ kind 1 BCW / 2 GEO, bitDepth, w, h, chroma, param ], s0, s1, and the output of the scalar row and of the x86 row.
The generator's two rows must agree on everything; this driver asserts it.
usage: python tests/blend_golden_gen.py /path/to/blend_golden_gen"""
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import blend_cases as BLC  # noqa: E402
import blend_ref as BL  # noqa: E402
import pred_ref as PR  # noqa: E402


def weight_blocks():
    return [(sd, w, h, c) for sd in range(64) for (w, h) in BL.GEO_SIZES for c in (0, 1)]


def intermediate(orc, pl, pos, it, l, bd):
    """the 14-bit block of one hypothesis from the numpy model of the two passes"""
    w, h, chroma = int(it["width"]), int(it["height"]), int(it["chroma"])
    arr, (x, y) = pl[int(it["ref_plane"][l])], pos[l]
    xf, yf = int(it["frac"][l][0]), int(it["frac"][l][1])
    s, lo, nt = (2, 1, 4) if chroma else (1 if (w, h) == (4, 4) else 0, 3, 8)
    th = ([int(c) for c in orc.if_coeff(s, xf)[1][:nt]], lo) if xf else ([64], 0)
    tv = ([int(c) for c in orc.if_coeff(s, yf)[1][:nt]], lo) if yf else ([64], 0)
    return PR.kernel_form(th[0], th[1], tv[0], tv[1], arr, y, x, w, h, False, bd)


def blend_cases(orc):
    out = []
    for bd in (8, 10):
        pl, _ = BLC.planes(bd, 40 + bd)
        rng = np.random.default_rng(50 + bd)
        picked = []
        items, _, blend, pos = BLC.bcw_list(pl, 60 + bd)
        keep = [k for k in range(len(items)) if int(items[k]["width"]) * int(items[k]["height"]) <= 1024 and not int(items[k]["alt_hpel"])]
        picked += [(items[k], blend[k], pos[k]) for k in rng.choice(keep, 9, replace=False)]
        items, _, blend, pos = BLC.geo_list(pl, 70 + bd)
        keep = [k for k in range(len(items)) if int(items[k]["width"]) * int(items[k]["height"]) <= 1024 and not int(items[k]["alt_hpel"])]
        picked += [(items[k], blend[k], pos[k]) for k in rng.choice(keep, 9, replace=False)]
        items, _, blend, pos = BLC.extremes_list(pl, 80 + bd)
        keep = [k for k in range(len(items)) if int(items[k]["width"]) <= 32]
        picked += [(items[k], blend[k], pos[k]) for k in rng.choice(keep, 12, replace=False)]
        for it, bl, p in picked:
            s0, s1 = (intermediate(orc, pl, p, it, l, bd) for l in (0, 1))
            out.append((int(bl["mode"]), bd, int(it["width"]), int(it["height"]), int(it["chroma"]), int(bl["param"]), s0, s1))
    return out


def main(exe):
    from oracle.oracle import Oracle
    cs = blend_cases(Oracle())
    wb = weight_blocks()
    with tempfile.TemporaryDirectory() as td:
        fi, fo = os.path.join(td, "in.bin"), os.path.join(td, "out.bin")
        with open(fi, "wb") as f:
            f.write(np.int32(len(wb) + len(cs)).tobytes())
            for (sd, w, h, c) in wb:
                bw, bh = w >> c, h >> c
                f.write(np.array([2, 10, bw, bh, c, sd], np.int32).tobytes() + np.full(bw * bh, -8064, np.int16).tobytes() + np.full(bw * bh, -8192, np.int16).tobytes())
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
    dst = os.path.join(HERE, "golden", "blend.npz")
    np.savez_compressed(dst, **arrays)
    print("%d weight samples, %d cases -> %s (%d bytes)" % (ws.size, len(cs), dst, os.path.getsize(dst)))


if __name__ == "__main__":
    main(sys.argv[1])
