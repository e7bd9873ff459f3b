"""Driver of tests/ict_golden_gen.cpp: builds the recorded inputs, runs the generator (its path is argv[1]; compile command in its header comment) and writes
tests/golden/ict.npz — arrays only.

Per case: hdr = [ mode, w, h, kind ], cb, cr (the two residual blocks) and what the reference's own TrQuant::fwdTransformICT / invTransformICT made of them: dist = ( d1, d2 )
and, for mode != 0, joint, ( rec_cb, rec_cr ) = the inverse of the joint block, ( in_cb, in_cr ) = the inverse with the case's own input block as the coded component.
The reference has ONE row of these functions (no x86 variant: TrQuant.cpp:230-247), so there is nothing to compare a second row against.  The cases:
(0) sweep     every size pair { 2, 4, 8, 16, 32 } x { 2, 4, 8, 16, 32 } once and 64x64 once, the mode cycling over the six non-zero modes and 0 along the sweep and the
              bit depth alternating 10 / 8; seeded residuals of a smooth part plus noise, |r| <= 2^bd - 1.
(1) modes     every mode on 4x4, 8x4 and 16x8 at both bit depths, seeded likewise.
(2) extremes  on 4x4, 8x2 and 16x16, every mode: both components at +max, both at -max, opposite signs, 0 / +-max alternating — each once at residual range
              ( +-1023 ) and once at int16 range ( 32767 / -32768 ), which pins the narrowing wrap.
This driver asserts that on the seeded cases every non-zero mode's joint block differs from both inputs.
usage: python tests/ict_golden_gen.py /path/to/ict_golden_gen"""
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import ict_ref as IR  # noqa: E402

ALL_MODES = IR.MODES + (0,)
EXTREME_SIZES = [(4, 4), (8, 2), (16, 16)]


def seeded(rng, w, h, bd):
    """two correlated residual blocks: a shared smooth part, a part of each one's own and noise, clipped to |r| <= 2^bd - 1"""
    top = (1 << bd) - 1
    yy, xx = np.mgrid[0:h, 0:w]
    base = rng.normal(0, top / 6.0) + rng.normal(0, top / 8.0) * np.cos((xx + 0.5) * np.pi / (2 * w)) + rng.normal(0, top / 8.0) * np.cos((yy + 0.5) * np.pi / (2 * h))
    out = []
    for g in (1.0, rng.choice([-1.0, -0.5, 0.5, 1.0])):
        out.append(np.clip(np.rint(g * base + rng.normal(0, top / 16.0, (h, w))), -top, top).astype(np.int16))
    return out


def cases():
    """-> list of ( mode, w, h, kind, cb, cr )"""
    out = []
    rng = np.random.default_rng(1453)
    sweep = [(w, h) for w in (2, 4, 8, 16, 32) for h in (2, 4, 8, 16, 32)] + [(64, 64)]
    for k, (w, h) in enumerate(sweep):
        out.append((ALL_MODES[k % 7], w, h, 0) + tuple(seeded(rng, w, h, 10 if k % 2 == 0 else 8)))
    for bd in (8, 10):
        for (w, h) in ((4, 4), (8, 4), (16, 8)):
            for m in ALL_MODES:
                out.append((m, w, h, 1) + tuple(seeded(rng, w, h, bd)))
    for (hi, lo) in ((1023, -1023), (32767, -32768)):
        for (w, h) in EXTREME_SIZES:
            k = np.arange(w * h).reshape(h, w)
            alt_cb = np.choose(k % 4, [0, hi, 0, lo]).astype(np.int16)
            alt_cr = np.choose(k % 4, [hi, 0, lo, 0]).astype(np.int16)
            full = lambda v: np.full((h, w), v, np.int16)
            for m in ALL_MODES:
                for cb, cr in ((full(hi), full(hi)), (full(lo), full(lo)), (full(hi), full(lo)), (alt_cb, alt_cr)):
                    out.append((m, w, h, 2, cb, cr))
    return out


def main(exe):
    cs = cases()
    with tempfile.TemporaryDirectory() as td:
        fi, fo = os.path.join(td, "in.bin"), os.path.join(td, "out.bin")
        with open(fi, "wb") as f:
            f.write(np.int32(len(cs)).tobytes())
            for (m, w, h, kind, cb, cr) in cs:
                assert cb.shape == cr.shape == (h, w) and cb.dtype == cr.dtype == np.int16
                f.write(np.array([m, w, h], np.int32).tobytes() + np.ascontiguousarray(cb).tobytes() + np.ascontiguousarray(cr).tobytes())
        subprocess.check_call([exe, fi, fo])
        raw = open(fo, "rb").read()
    at, arrays = 0, {"n": np.int32(len(cs))}
    seen = set()
    for i, (m, w, h, kind, cb, cr) in enumerate(cs):
        k = "c%03d_" % i
        arrays[k + "hdr"] = np.array([m, w, h, kind], np.int32)
        arrays[k + "cb"], arrays[k + "cr"] = cb, cr
        arrays[k + "dist"] = np.frombuffer(raw, np.int64, 2, at).copy()
        at += 16
        if m != 0:
            for name in ("joint", "rec_cb", "rec_cr", "in_cb", "in_cr"):
                arrays[k + name] = np.frombuffer(raw, np.int16, w * h, at).reshape(h, w).copy()
                at += 2 * w * h
            if kind != 2:
                assert not np.array_equal(arrays[k + "joint"], cb) and not np.array_equal(arrays[k + "joint"], cr), "case %d: the joint block of mode %d equals an input" % (i, m)
        seen.add((w, h)); seen.add(("mode", m))
    assert at == len(raw)
    assert all(("mode", m) in seen for m in ALL_MODES) and all((w, h) in seen for w in (2, 4, 8, 16, 32) for h in (2, 4, 8, 16, 32)) and (64, 64) in seen
    np.savez_compressed(IR.GOLDEN, **arrays)
    print("%d cases -> %s (%d bytes)" % (len(cs), IR.GOLDEN, os.path.getsize(IR.GOLDEN)))


if __name__ == "__main__":
    main(sys.argv[1])
