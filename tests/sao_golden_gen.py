"""Driver of tests/sao_golden_gen.cpp: builds the recorded inputs from tests/sao_cases.py, runs the generator (its path is argv[1]; compile command in its header comment)
and writes tests/golden/sao.npz — arrays only.

pictures   per picture of sao_cases.PICTURES: pic_<name>_hdr = [ width, height, ctu, bit depth ], pic_<name>_org<c> / _src<c> for the three planes (4:2:0)
stats      stats_names, and per case s<k>_flags (uint8 per CTU; what the picture's borders give where the case has none), s<k>_borders (1: the case hands no flags over)
           and s<k>_rec = int64 [ctus][3][5][2][32]: SAOStatData[5] of every CTU and plane from EncSampleAdaptiveOffset::getBlkStats itself, called per CTU the way
           getStatistics walks a picture
offsets    offset_names, and per case o<k>_prm ( [ctus][3] parameter records ), o<k>_clip ( [3][2] ) and o<k>_delta<c> = res - src per plane, int16, from the offsetBlock
           table entry itself called per CTU that is on, the way offsetCTU does (res starts as a copy of src)
Both rows of the reference are called on every record — the table of SampleAdaptiveOffset( false ) and the x86 row; the driver fails unless they agree on every
record whose clip range is the bit depth's (the x86 row's vector paths ignore a narrower ClpRng) and whose availability mask lies in in_x86_subset(), and records the scalar row.  It then asserts, from the reference's results alone, that the fixture is not vacuous (coverage(); tests/test_sao_cpu.py repeats it).
usage: python tests/sao_golden_gen.py /path/to/sao_golden_gen
       python tests/sao_golden_gen.py /path/to/sao_golden_gen --time      (a context figure for profiles/sao.md: the reference's own loops on the 1920x1080 picture of
                                                                           tools/sao_time.py, one core; writes nothing)"""
import os
import struct
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import sao_cases as SC  # noqa: E402
import sao_ref as SR  # noqa: E402


def _ctus(pic, c):
    """-> ( index, x, y, w, h ) of every CTU of plane c"""
    cw, ch = pic.ctus[c]
    H, W = pic.src[c].shape
    gx, gy = pic.grid
    return [(cy * gx + cx, cx * cw, cy * ch, min(cw, W - cx * cw), min(ch, H - cy * ch)) for cy in range(gy) for cx in range(gx)]


def coverage(stats, offsets):
    """what the fixture must show, from recorded results alone.  stats: list of ( name, flags [ctus], rec [ctus][3][5][2][32] ); offsets: list of ( name, Pic, prm, clip,
    [ delta per plane ] )"""
    for label, sel in (("luma", slice(0, 1)), ("chroma", slice(1, 3))):
        hit = np.zeros((5, 32), bool)
        for _, _, rec in stats:
            hit |= (rec[:, sel, :, 1, :] > 0).any(axis=(0, 1))
        assert hit[:4, :5].all() and hit[4].all(), "%s: bins never counted: %s" % (label, np.argwhere(~hit[:, :5] if not hit[:4, :5].all() else ~hit).tolist())
    by = {n: (f, r) for n, f, r in stats}
    full, none = by["grid3/borders"][1][4], by["grid3/none"][1][4]
    for f in SR.STAT_FLAGS:
        if f == SR.ABOVE_RIGHT:      # looked at only where right is missing
            assert not np.array_equal(by["grid3/clear40"][1][4], by["grid3/clear8"][1][4]), "clearing flag %d changes nothing" % f
        else:
            assert not np.array_equal(by["grid3/clear%d" % f][1][4], full), "clearing flag %d changes nothing" % f
        assert not np.array_equal(by["grid3/only%d" % f][1][4], none), "setting flag %d changes nothing" % f
        assert by["grid3/clear%d" % f][0][4] & f == 0 and by["grid3/only%d" % f][0][4] & f
    types, low, high, untouched = set(), 0, 0, 0
    for name, pic, prm, clip, delta in offsets:
        q = SR.max_offset_qval(pic.bit_depth)
        for c in range(3):
            d, src = delta[c].astype(np.int64), pic.src[c].astype(np.int64)
            res = src + d
            for (i, x, y, w, h) in _ctus(pic, c):
                blk = d[y:y + h, x:x + w]
                if prm[i, c]["type"] >= 0 and blk.any():
                    types.add(int(prm[i, c]["type"]))
                if prm[i, c]["type"] >= 0 and np.abs(prm[i, c]["offs"]).min() > 0 and ((blk == 0) & (res[y:y + h, x:x + w] > clip[c][0]) & (res[y:y + h, x:x + w] < clip[c][1])).any():
                    untouched += 1      # every class has an offset and the sample sits inside the clip range, yet it kept its value: it was outside the processed ranges
            if name.startswith("ends/"):      # every offset of these cases is +- q or 0: a smaller change is a clipped one
                high += int(((res == clip[c][1]) & (d > 0) & (d < q)).sum())
                low += int(((res == clip[c][0]) & (d < 0) & (d > -q)).sum())
    assert types == {0, 1, 2, 3, 4}, "filter types that change no sample: %s" % sorted({0, 1, 2, 3, 4} - types)
    assert low > 0 and high > 0, "a clip end never fires (low %d, high %d)" % (low, high)
    assert untouched > 0, "no sample stays unfiltered in a filtered CTU"
    return {"clipped_low": low, "clipped_high": high, "ctus_with_unfiltered_samples": untouched}


def in_x86_subset(typ, m):
    """the masks on which the x86 row is offsetBlock_core.  Its vector paths of BOTH diagonal types are entered when left, right, above-left and below-right are all there
    (SampleAdaptiveOffsetX86.h:306, :481) and then filter whole rows, looking at above / below only: that is the scalar row's result where above and below are there too
    and, for EO_45, above-right and below-left as well"""
    fast = SR.A_LEFT | SR.A_RIGHT | SR.A_ABOVE_LEFT | SR.A_BELOW_RIGHT
    if typ not in (2, 3) or (m & fast) != fast:
        return True
    need = SR.A_ABOVE | SR.A_BELOW | ((SR.A_ABOVE_RIGHT | SR.A_BELOW_LEFT) if typ == 3 else 0)
    return (m & need) == need


def run(exe, blob):
    with tempfile.TemporaryDirectory() as td:
        fi, fo = os.path.join(td, "in.bin"), os.path.join(td, "out.bin")
        with open(fi, "wb") as f:
            f.write(blob)
        subprocess.check_call([exe, fi, fo])
        return open(fo, "rb").read()


def set_planes(pic_org, pic_src, chroma, bd):
    h, w = pic_src.shape
    return struct.pack("<iiiii", 0, int(chroma), bd, w, h) + np.ascontiguousarray(pic_org, np.int16).tobytes() + np.ascontiguousarray(pic_src, np.int16).tobytes()


def main(exe):
    P = SC.pictures()
    scases, ocases = SC.stats_cases(), SC.offset_cases()
    blob, pending = [], []      # pending: ( kind, case index, plane, ctu, w, h )
    for name, pic in P.items():
        for c in range(3):
            blob.append(set_planes(pic.org[c], pic.src[c], c > 0, pic.bit_depth))
            for k, (_, p, flags) in enumerate(scases):
                if p is pic:
                    fl = SR.border_flags(*pic.grid) if flags is None else flags
                    for (i, x, y, w, h) in _ctus(pic, c):
                        blob.append(struct.pack("<iiiiii", 1, x, y, w, h, int(fl[i])))
                        pending.append((1, k, c, i, w, h))
            for k, (_, p, prm, clip) in enumerate(ocases):
                if p is pic:
                    for (i, x, y, w, h) in _ctus(pic, c):
                        r = prm[i, c]
                        if r["type"] >= 0:
                            blob.append(struct.pack("<iiiiiiiii5i", 2, x, y, w, h, int(r["type"]), int(r["band"]), int(r["avail"]), int(clip[c][1] + 1).bit_length() - 1, *[int(v) for v in r["offs"]]))
                            pending.append((2, k, c, i, w, h))
    raw = run(exe, b"".join(blob))
    recs = [np.zeros((p.n_ctus, 3, 5, 2, 32), np.int64) for (_, p, _) in scases]
    deltas = [[np.zeros(p.src[c].shape, np.int16) for c in range(3)] for (_, p, _, _) in ocases]
    at, narrowed_differs = 0, 0
    for (kind, k, c, i, w, h) in pending:
        if kind == 1:
            rows = np.frombuffer(raw, np.int64, 640, at).reshape(2, 5, 2, 32); at += 5120
            assert np.array_equal(rows[0], rows[1]), "statistics case %s plane %d CTU %d: the scalar and the x86 row differ" % (scases[k][0], c, i)
            recs[k][i, c] = rows[0]
        else:
            rows = np.frombuffer(raw, np.int16, 2 * w * h, at).reshape(2, h, w); at += 4 * w * h
            pic = ocases[k][1]
            # the x86 row clips its vector paths to [0, 2^channelBitDepth - 1] whatever the ClpRng says: with a narrowed clip range it is the scalar row alone that
            # honours the argument, and the scalar row is what is recorded
            # likewise outside in_x86_subset(): there the scalar row, offsetBlock_core, is the definition
            if ocases[k][3][c][1] == (1 << pic.bit_depth) - 1 and in_x86_subset(int(ocases[k][2][i, c]["type"]), int(ocases[k][2][i, c]["avail"])):
                assert np.array_equal(rows[0], rows[1]), "offset case %s plane %d CTU %d: the scalar and the x86 row differ" % (ocases[k][0], c, i)
            else:
                narrowed_differs += not np.array_equal(rows[0], rows[1])
            cw, ch = pic.ctus[c]
            x, y = (i % pic.grid[0]) * cw, (i // pic.grid[0]) * ch
            deltas[k][c][y:y + h, x:x + w] = rows[0] - pic.src[c][y:y + h, x:x + w]
    assert at == len(raw)
    arrays = {"pic_names": np.array(list(P)), "stats_names": np.array([n for n, _, _ in scases]), "offset_names": np.array([n for n, _, _, _ in ocases])}
    for name, pic in P.items():
        arrays["pic_%s_hdr" % name] = np.array([pic.width, pic.height, pic.ctu, pic.bit_depth], np.int32)
        for c in range(3):
            arrays["pic_%s_org%d" % (name, c)], arrays["pic_%s_src%d" % (name, c)] = pic.org[c], pic.src[c]
    st = []
    for k, (name, pic, flags) in enumerate(scases):
        fl = SR.border_flags(*pic.grid) if flags is None else np.asarray(flags, np.uint8)
        arrays["s%03d_flags" % k], arrays["s%03d_borders" % k], arrays["s%03d_rec" % k] = fl, np.uint8(flags is None), recs[k]
        st.append((name, fl, recs[k]))
    of = []
    for k, (name, pic, prm, clip) in enumerate(ocases):
        arrays["o%03d_prm" % k], arrays["o%03d_clip" % k] = prm, np.array(clip, np.int32)
        for c in range(3):
            arrays["o%03d_delta%d" % (k, c)] = deltas[k][c]
        of.append((name, pic, prm, clip, deltas[k]))
    seen = coverage(st, of)
    np.savez_compressed(SR.GOLDEN, **arrays)
    print("%d pictures, %d statistics cases, %d offset cases (%d CTUs outside the x86 row's subset on which it differs), %s -> %s (%d bytes)"
          % (len(P), len(scases), len(ocases), narrowed_differs, seen, SR.GOLDEN, os.path.getsize(SR.GOLDEN)))


def time_reference(exe, reps=7):
    sys.path.insert(0, os.path.join(os.path.dirname(HERE), "tools"))
    import sao_time as ST
    org, src = ST.picture()
    for ctu in (128, 64):
        tot = [0.0, 0.0]
        for c in range(3):
            cs = ctu >> (c > 0)
            raw = run(exe, set_planes(org[c], src[c], c > 0, 10) + struct.pack("<iiii", 3, cs, cs, reps))
            s = np.frombuffer(raw, np.float64, 2)
            tot[0] += s[0]; tot[1] += s[1]
        print("CPU, one core, the reference's x86 row, CTU %3d: getBlkStats over the picture %.2f ms, offsetBlock (EO_135, every CTU on) %.2f ms" % (ctu, 1e3 * tot[0], 1e3 * tot[1]))


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[2] == "--time":
        time_reference(sys.argv[1])
    else:
        main(sys.argv[1])
