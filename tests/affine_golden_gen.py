"""Driver of tests/affine_golden_gen.cpp: builds the recorded inputs, runs the generator (its path is argv[1]; compile command in its header comment) and writes
tests/golden/affine.npz — arrays only: the picture geometry, the two reference pictures (luma + Cb, 10 bit, margins included; the 8-bit cases use the same planes >> 2),
the case table and what the reference's own xPredAffineBlk returned per case, per list used, for the luma and the Cb block, on its scalar row and on its x86 row.

Picture 128x96, CTU 32, margin 48.  Cases: seeded CUs 8..64 x 8..64 anywhere in the picture, both models, list 0 / list 1 / both, the four PROF settings, bit depths 8 and 10,
control-point spreads D = 4, 32, 256 (RT - LT uniform in +-D * w / 16, LB - LT in +-D * h / 16, 1/16 sample); LT up to 24 samples, and for some cases far outside the picture
so that the picture clip acts.  A drawn CU whose sub-blocks would read outside the margin (possible only because CUs larger than the CTU are recorded) is drawn again.
usage: python tests/affine_golden_gen.py /path/to/affine_golden_gen"""
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import affine_cases as AC  # noqa: E402
import affine_ref as AR  # noqa: E402

PIC_W, PIC_H, CTU, MARGIN, N_CASES = 128, 96, 32, 48, 56


def planes():
    """-> [y0, c0, y1, c1]: smooth texture + a little noise (it compresses), with a 0 / 1023 checkerboard patch in each luma plane"""
    w = AC.World(10, CTU, "texture", seed=4242, pic_w=PIC_W, pic_h=PIC_H, margin=MARGIN)
    out = []
    for p in (0, 1):
        y = (w.np[p][:PIC_H + 2 * MARGIN] & ~3).astype(np.int16)
        yy, xx = np.mgrid[0:24, 0:32]
        y[MARGIN + 40:MARGIN + 64, MARGIN + 20 + 50 * p:MARGIN + 52 + 50 * p] = ((xx + yy) & 1) * 1023
        out += [y, (w.np[2 + p][:PIC_H // 2 + MARGIN] & ~3).astype(np.int16)]
    return out


def cases():
    rng = np.random.default_rng(31337)
    rows, k = [], 0
    while len(rows) < N_CASES:
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
        rows.append([8 if k % 4 == 3 else 10, x, y, w, h, k & 1, inter_dir, int(lu["prof"]), max(int(lu["ref_plane"][0]), 0), max(int(lu["ref_plane"][1]), 0)] +
                    [int(v) for v in lu["cpmv"].reshape(-1)])
        k += 1
    return np.array(rows, np.int32)


def main(exe):
    pl, cs = planes(), cases()
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
    dst = os.path.join(HERE, "golden", "affine.npz")
    np.savez_compressed(dst, hdr=np.array([PIC_W, PIC_H, CTU, MARGIN], np.int32), y0=pl[0], c0=pl[1], y1=pl[2], c1=pl[3], cases=cs,
                        scalar=np.concatenate(scalar), simd=np.concatenate(simd))
    print("%d cases -> %s (%d bytes)" % (len(cs), dst, os.path.getsize(dst)))


if __name__ == "__main__":
    main(sys.argv[1])
