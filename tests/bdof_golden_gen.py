"""Driver of tests/bdof_golden_gen.cpp: builds the recorded inputs, runs the generator (its path is argv[1]; compile command in its header comment) and writes
tests/golden/bdof.npz — arrays only: per case the bit depth, the unit shape, the two frames (the 14-bit block of each list inside its one-sample ring) and what the
reference's xApplyBDOF returned on its scalar row and on its x86 row.

Cases, for each unit shape 16x16 / 16x8 / 8x16 at bit depths 8 and 10:
  pictures   a 14-bit block interpolated-looking from a smooth picture with noise, the second list displaced by a fraction of a sample; ring = integer-looking samples
  flat       both frames constant (all sums zero: tmpx = tmpy = 0), equal and unequal constants, 14-bit extremes included
  ramps      steep opposite ramps that drive tmpx / tmpy to +15 and to -15
  extremes   frames made of the extreme sample values 0 and max ( ( v << headroom ) - 8192 ) in blocks and checkerboards, and full-range int16 noise
usage: python tests/bdof_golden_gen.py /path/to/bdof_golden_gen"""
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SHAPES = [(16, 16), (16, 8), (8, 16)]


def cases():
    rng = np.random.default_rng(20250)
    out = []
    for bd in (8, 10):
        hr, top = max(2, 14 - bd), (1 << bd) - 1
        lo, hi = -8192, (top << hr) - 8192

        def conv(a):
            return ((np.asarray(a).astype(np.int32) << hr) - 8192).astype(np.int16)

        for (w, h) in SHAPES:
            yy, xx = np.mgrid[0:h + 2, 0:w + 2].astype(np.float64)
            for k in range(6):          # pictures
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
            for k in range(3):          # everything the 14-bit intermediate can hold, and beyond it: the int16 cast of the output
                span = (lo, hi + 1) if k < 2 else (-32768, 32768)
                out.append((bd, w, h, rng.integers(span[0], span[1], (h + 2, w + 2)).astype(np.int16), rng.integers(span[0], span[1], (h + 2, w + 2)).astype(np.int16)))
    return out


def main(exe):
    cs = cases()
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
    dst = os.path.join(HERE, "golden", "bdof.npz")
    np.savez_compressed(dst, **arrays)
    print("%d cases -> %s (%d bytes)" % (len(cs), dst, os.path.getsize(dst)))


if __name__ == "__main__":
    main(sys.argv[1])
