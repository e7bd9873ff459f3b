"""Driver of tests/sbt_golden_gen.cpp: builds the recorded inputs, runs the generator (its path is argv[1]; compile command in its header comment) and writes
tests/golden/sbt.npz — arrays only.

cus      per CU: hdr = [ w, h, sbt_allowed, kind ], wt = [ chroma weight, distortion scale ], the residual blocks y, cb, cr and what the reference's own
         InterSearch::xCalcMinDistSbt made of them — est [9], order [8] (recorded with an infinite distortion scale, so that "fast algorithm 1" never returns early: see
         the generator's header), skip = m_skipSbtAll at the CU's distortion scale — and parts [3][16], the unweighted part sums from the reference's SSE table entry; the
         driver fails unless the entry's scalar row and its x86 row agree on every part of every CU inside the 10-bit residual range (beyond it the x86 row's 32-bit lanes
         wrap; the scalar row is recorded).
         kind 0  sweep      every size of sbt_ref.SIZES at 8 and 10 bits, seeded smooth-plus-noise residuals, the size's full sbt_allowed, the weights cycling
         kind 1  subsets    every non-empty subset of the size's sbt_allowed on 8x4, 4x8, 8x8, 16x8, 8x16 and 16x16, and some on 32x32
         kind 2  content    all zero; left/right and top/bottom mirrored; energy confined to each quarter; +-( 2^bd - 1 ) everywhere; the int16 extremes -32768 / 32767
         kind 3  weights    chroma-heavy CUs at every weight of sbt_cases.WEIGHTS, among them parts whose weighted product has a fraction above one half (truncation, not
                            rounding) and CUs whose weighted total differs from the unweighted one
tilings  every size of sbt_ref.ALL_SIZES x every mode its sides allow: both tiles of every component from PartitionerImpl::getSbtTuTiling, the luma types from xSetTrTypes
placed   a placed reconstruction (sbt_ref.place of a seeded tile reconstruction) against a seeded original block: the whole block's SSE from the same SSE entry (both rows)
The driver asserts that the fixture is not vacuous: every mode is first of its kind in `order` somewhere, there are ties, a quad mode's estimate lies below both half modes
of the other direction somewhere, and weighted and unweighted totals differ where the weight is not 1.
usage: python tests/sbt_golden_gen.py /path/to/sbt_golden_gen"""
import os
import struct
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import sbt_cases as SC  # noqa: E402
import sbt_ref as SR  # noqa: E402

DIST_SCALES = (1.0, 37.5, 800.0, 32768.0 / 57.9)      # 2^SCALE_BITS / lambda for a few lambdas: fast algorithm 1 fires on some CUs and not on others


def cu_cases():
    """-> list of ( w, h, allowed, kind, cw, blocks )"""
    rng = np.random.default_rng(3272)
    out = []
    W = SC.WEIGHTS
    for k, (w, h) in enumerate(SR.SIZES):
        for bd in (8, 10):
            out.append((w, h, SR.allowed_of(w, h), 0, W[(k + bd) % len(W)], SC.seeded(rng, w, h, bd)))
    for (w, h) in ((8, 4), (4, 8), (8, 8), (16, 8), (8, 16), (16, 16)):
        for j, a in enumerate(SR.subsets_of(SR.allowed_of(w, h))):
            out.append((w, h, a, 1, W[j % len(W)], SC.seeded(rng, w, h, 10 if j % 2 else 8)))
    for j, a in enumerate((2, 4, 8, 16, 24, 6, 18)):
        out.append((32, 32, a, 1, W[j % len(W)], SC.seeded(rng, 32, 32, 10)))
    for (w, h) in ((8, 8), (16, 16), (64, 64), (64, 4), (4, 64)):
        out.append((w, h, SR.allowed_of(w, h), 2, 1.0 if w == 8 else W[2], SC.constant(w, h, 0)))
    for (w, h) in ((8, 8), (16, 16), (32, 32), (64, 16)):
        for axis in (0, 1):
            out.append((w, h, SR.allowed_of(w, h), 2, 1.0, SC.mirrored(rng, w, h, 10, axis)))
    for (w, h) in ((16, 16), (32, 32)):
        for mode in (4, 5, 6, 7):
            out.append((w, h, SR.allowed_of(w, h), 2, W[mode % len(W)], SC.quarter(rng, w, h, 10, mode)))
    for v in (255, -255, 1023, -1023, 32767, -32768):
        for (w, h) in ((16, 16), (64, 64)) if abs(v) != 255 else ((16, 16),):
            out.append((w, h, SR.allowed_of(w, h), 2, W[3] if v > 0 else 1.0, SC.constant(w, h, v)))
    k = np.arange(64).reshape(8, 8)
    alt = np.choose(k % 4, [0, 32767, 0, -32768]).astype(np.int16)
    out.append((8, 8, SR.allowed_of(8, 8), 2, W[1], (alt, alt[:4, :4].copy(), alt[4:, 4:].copy())))
    for j, cw in enumerate(W):
        for (w, h) in ((8, 8), (16, 16)):
            y, cb, cr = SC.seeded(rng, w, h, 10)
            out.append((w, h, SR.allowed_of(w, h), 3, cw, ((y // 8).astype(np.int16), cb, cr)))
    return out


def main(exe):
    cus = cu_cases()
    rng = np.random.default_rng(995)
    tilings = [(w, h, m) for (w, h) in SR.ALL_SIZES for m in SR.modes_of(SR.allowed_of(w, h))]
    placed = []
    for (w, h, modes) in ((8, 8, (0, 3)), (4, 4, (1, 2)), (16, 16, (4, 5, 6, 7)), (32, 8, (0, 5)), (8, 32, (2, 7)), (2, 8, (3,)), (64, 64, (1, 6))):
        for m in modes:
            x, y, tw, th = SR.coded_tile(w, h, m)
            org = rng.integers(-1023, 1024, (h, w)).astype(np.int16)
            tile = np.clip(org[y:y + th, x:x + tw] + rng.integers(-40, 41, (th, tw)), -32768, 32767).astype(np.int16) if m != 7 else rng.integers(-32768, 32768, (th, tw)).astype(np.int16)
            placed.append((w, h, m, org, tile))
    with tempfile.TemporaryDirectory() as td:
        fi, fo = os.path.join(td, "in.bin"), os.path.join(td, "out.bin")
        with open(fi, "wb") as f:
            for i, (w, h, allowed, kind, cw, blocks) in enumerate(cus):
                assert blocks[0].shape == (h, w) and blocks[1].shape == blocks[2].shape == (h // 2, w // 2) and all(b.dtype == np.int16 for b in blocks)
                f.write(struct.pack("<iiii", 1, w, h, allowed) + struct.pack("<dd", cw, DIST_SCALES[i % len(DIST_SCALES)]) + b"".join(np.ascontiguousarray(b).tobytes() for b in blocks))
            for (w, h, m) in tilings:
                f.write(struct.pack("<iiii", 2, w, h, m))
            for (w, h, m, org, tile) in placed:
                f.write(struct.pack("<iii", 3, w, h) + org.tobytes() + SR.place(tile, w, h, m).tobytes())
        subprocess.check_call([exe, fi, fo])
        raw = open(fo, "rb").read()
    at, arrays = 0, {"n_cus": np.int32(len(cus)), "n_placed": np.int32(len(placed))}
    first, ties, quad_low, weight_matters, trunc, wrapped = set(), 0, 0, 0, 0, 0
    for i, (w, h, allowed, kind, cw, blocks) in enumerate(cus):
        k = "u%03d_" % i
        est = np.frombuffer(raw, np.uint64, 9, at).copy(); at += 72
        order = np.frombuffer(raw, np.uint8, 8, at).copy(); at += 8
        skip = raw[at]; at += 1
        rows = np.frombuffer(raw, np.uint64, 96, at).reshape(2, 3, 16).copy(); at += 768
        # the x86 row multiply-adds pairs of 16-bit differences and sums them in 32-bit lanes: exact inside the residual range of 10 bits, which is all the encoder hands it;
        # on the int16 extremes it wraps (xCalcMinDistSbt's own loop does not: it is scalar 64-bit code), and the scalar row is what is recorded
        if max(int(np.abs(b.astype(np.int32)).max()) for b in blocks) <= 1023:
            assert np.array_equal(rows[0], rows[1]), "CU %d (%dx%d): the scalar and the x86 row of the SSE entry differ on a part" % (i, w, h)
        else:
            wrapped += not np.array_equal(rows[0], rows[1])
        arrays[k + "hdr"] = np.array([w, h, allowed, kind], np.int32)
        arrays[k + "wt"] = np.array([cw, DIST_SCALES[i % len(DIST_SCALES)]], np.float64)
        arrays[k + "y"], arrays[k + "cb"], arrays[k + "cr"] = blocks
        arrays[k + "est"], arrays[k + "order"], arrays[k + "skip"], arrays[k + "parts"] = est, order, np.uint8(skip), rows[0]
        # ---- what the fixture must show
        n_half = min(2 * (((allowed >> 1) & 1) + ((allowed >> 2) & 1)), 2)
        first.add(int(order[0])); first.add(int(order[n_half]) if n_half < 8 else 255)
        e = [int(v) for v in est]
        live = [v for v in e[:8] if v != SR.MAX_DISTORTION]
        ties += len(set(live)) < len(live)
        quad_low += any(e[q] < min(e[a], e[b]) for q, a, b in ((4, 2, 3), (5, 2, 3), (6, 0, 1), (7, 0, 1)) if e[q] != SR.MAX_DISTORTION and e[a] != SR.MAX_DISTORTION and e[b] != SR.MAX_DISTORTION)
        total_plain = int(sum(int(v) for v in rows[0].reshape(-1)))
        if cw != 1.0 and total_plain:
            assert e[8] != total_plain, "CU %d: the weight %.6f changes nothing" % (i, cw)
            weight_matters += 1
            trunc += any((float(int(v)) * cw) % 1.0 > 0.5 for v in rows[0][1:].reshape(-1))
    til_rects, til_types = np.zeros((len(tilings), 2, 3, 4), np.int32), np.zeros((len(tilings), 2), np.int32)
    for n in range(len(tilings)):
        til_rects[n] = np.frombuffer(raw, np.int32, 24, at).reshape(2, 3, 4); at += 96
        til_types[n] = np.frombuffer(raw, np.int32, 2, at); at += 8
    arrays["til_hdr"], arrays["til_rects"], arrays["til_types"] = np.array(tilings, np.int32), til_rects, til_types
    for i, (w, h, m, org, tile) in enumerate(placed):
        k = "p%03d_" % i
        s = np.frombuffer(raw, np.uint64, 2, at); at += 16
        assert s[0] == s[1] or m == 7, "placed block %d: the scalar and the x86 row of the SSE entry differ" % i      # (mode 7's tiles span the int16 range: see above)
        arrays[k + "hdr"], arrays[k + "org"], arrays[k + "tile"], arrays[k + "sse"] = np.array([w, h, m], np.int32), org, tile, np.uint64(s[0])
    assert at == len(raw)
    assert all(m in first for m in range(8)), "modes never first of their kind: %s" % sorted(set(range(8)) - first)
    assert ties > 0 and quad_low > 0 and weight_matters > 0 and trunc > 0, (ties, quad_low, weight_matters, trunc)
    assert len({tuple(t) for t in til_types.tolist()}) == 4
    np.savez_compressed(SR.GOLDEN, **arrays)
    print("%d CUs (%d with a tie, %d with a quad below the other halves, %d truncating, %d beyond the x86 row's range), %d tilings, %d placed blocks -> %s (%d bytes)"
          % (len(cus), ties, quad_low, trunc, wrapped, len(tilings), len(placed), SR.GOLDEN, os.path.getsize(SR.GOLDEN)))


if __name__ == "__main__":
    main(sys.argv[1])
