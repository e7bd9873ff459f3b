"""Driver of tests/ciip_golden_gen.cpp: builds the recorded inputs, runs the generator (its path is argv[1]; compile command in its header comment) and writes
tests/golden/ciip.npz — arrays only.

Per case: hdr = [ bitDepth, w, h, chroma, num_intra ], line (top[0 .. w + 2] then left[0 .. h + 2], unfiltered), inter (the clipped inter block), and what the
reference's own functions made of them: intra (smoothing on luma, planar, PDPC) and result (weightCiip).  The cases:
(a) sweep     every luma size and every 4:2:0 chroma size of a CIIP CU once, the bit depth alternating 10 / 8 and num_intra cycling 0, 1, 2 along the sweep; line and inter
              block from seeded pictures — the line is the row above and the column left of a block position in one picture, the inter block a block of another picture.
(b) again     the sizes of at most 256 samples at the other bit depth and the next num_intra.
(c) extremes  on four luma and three chroma sizes, at both bit depths: line and block all 0; all max; the line 0 / max alternating (starting with either) against a block
              at all max / all 0; the line all 0 against a block all max and the other way round.
The generator's two rows (scalar, x86) must agree on everything, and the result must differ from the inter block except where line and block are one flat value; this
driver asserts both.
usage: python tests/ciip_golden_gen.py /path/to/ciip_golden_gen"""
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import bdof_cases as BC  # noqa: E402
import ciip_ref as CR  # noqa: E402

EXTREME_SIZES = [(8, 8, 0), (4, 16, 0), (16, 4, 0), (16, 16, 0), (4, 4, 1), (8, 2, 1), (8, 8, 1)]


def cases():
    """-> list of ( bd, w, h, chroma, num_intra, line, inter )"""
    out = []
    pics = {}
    for bd in (8, 10):
        rng = np.random.default_rng(900 + bd)
        pics[bd] = (BC._picture(rng, 140, 160, bd, 0.0), BC._picture(rng, 140, 160, bd, 2.9), rng)

    def seeded(bd, w, h, chroma, ni):
        a, b, rng = pics[bd]
        x, y = int(rng.integers(1, 160 - w - 2)), int(rng.integers(1, 140 - h - 2))
        bx, by = int(rng.integers(0, 160 - w)), int(rng.integers(0, 140 - h))
        out.append((bd, w, h, chroma, ni, CR.line_at(a, x, y, w, h), b[by:by + h, bx:bx + w].copy()))
    sizes = [(w, h, 0) for (w, h) in CR.LUMA_SIZES] + [(w, h, 1) for (w, h) in CR.CHROMA_SIZES]
    for k, (w, h, c) in enumerate(sizes):
        seeded(10 if k % 2 == 0 else 8, w, h, c, k % 3)
    for k, (w, h, c) in enumerate(sizes):
        if w * h <= 256:
            seeded(8 if k % 2 == 0 else 10, w, h, c, (k + 1) % 3)
    k = 0
    for bd in (8, 10):
        top = (1 << bd) - 1
        for (w, h, c) in EXTREME_SIZES:
            n = CR.line_len(w, h)
            alt = np.concatenate([(np.arange(w + 3) & 1) * top, (np.arange(h + 3) & 1) * top]).astype(np.int16)      # top[0] == left[0] == 0
            for line, blk in ((np.zeros(n, np.int16), 0), (np.full(n, top, np.int16), top), (alt, top), ((top - alt).astype(np.int16), 0),
                              (np.zeros(n, np.int16), top), (np.full(n, top, np.int16), 0)):
                out.append((bd, w, h, c, k % 3, line, np.full((h, w), blk, np.int16)))
                k += 1
    return out


def main(exe):
    cs = cases()
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
    assert all((w, h, 0) in seen for (w, h) in CR.LUMA_SIZES) and all((w, h, 1) in seen for (w, h) in CR.CHROMA_SIZES) and all(("ni", k) in seen for k in range(3))
    np.savez_compressed(CR.GOLDEN, **arrays)
    print("%d cases -> %s (%d bytes)" % (len(cs), CR.GOLDEN, os.path.getsize(CR.GOLDEN)))


if __name__ == "__main__":
    main(sys.argv[1])
