"""Driver of tests/visact_golden_gen.cpp: hands every case of tests/visact_cases.py to the generator (its path is argv[1]; compile command in its header comment) and
writes tests/golden/visact.npz — arrays only.

pictures, cases        the names
<pic>_hdr              int32 [ bit depth, table rows, then per row: 1 prev1 present | 2 prev2 present | 4 prev1 IS cur ]
<pic>_c<r>             cur of table row r, int16; <pic>_d1<r> = prev1 - cur, <pic>_d2<r> = prev2 - prev1 (int16; small numbers pack well) where present and not cur itself
<case>_pic             index into pictures
<case>_areas           the area list as bytes, uint8 [n][40] (vvhip_visact_area)
<case>_rec             uint64 [n][4]: saAct, taAct, the accumulator of getAvg over the mean rectangle, positions
<case>_hp              uint64 [n][3]: the bit patterns of the doubles hpSpatAct, hpTempAct, hpVisAct
<case>_int             uint32 [n][4]: spatAct, tempAct, minAct, visAct
<case>_avg             int64 [n]: getAvg of the mean rectangle, -1 where there is none
Both rows of the reference run every case — g_pelBufOP as constructed, the scalar row, and after initPelBufOps( true ), the x86 row — on copies of the planes in different
surroundings and at different strides per pointer.  The SCALAR row is recorded.  The x86 row of this reference is another function in a few places (x86_may_differ lists them
with their lines: a width <= 6 in the down-sampling form, and 16-bit lane arithmetic in the temporal entries); the driver fails unless the rows agree in every byte
everywhere else — getAvg, the positions, and the spatial part outside the one named place always.  It then fails unless the model (tests/visact_ref.py) equals the
recorded results, and unless every form x order occurs with a non-zero spatial and (order > 0) temporal sum.
usage: python tests/visact_golden_gen.py /path/to/visact_golden_gen
       python tests/visact_golden_gen.py /path/to/visact_golden_gen --time      (CPU context figures for profiles/visact.md: the reference's own
                                                                                 filterAndCalculateAverageActivity + getAvg over the two lists of tools/visact_time.py, one core; writes nothing)"""
import os
import struct
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import visact_cases as VC  # noqa: E402
import visact_ref as VR  # noqa: E402

RESULT = np.dtype([("rec", "<u8", 4), ("hp", "<u8", 3), ("int", "<u4", 4), ("avg", "<i8")])
assert RESULT.itemsize == 80


def run(exe, blob):
    with tempfile.TemporaryDirectory() as td:
        fi, fo = os.path.join(td, "in.bin"), os.path.join(td, "out.bin")
        with open(fi, "wb") as f:
            f.write(blob)
        subprocess.check_call([exe, fi, fo])
        return open(fo, "rb").read()


def row_flags(pic, r):
    cur, p1, p2 = pic.rows[r]
    return (1 if p1 is not None else 0) | (2 if p2 is not None else 0) | (4 if pic.same(r) else 0)


def request(pic, areas, reps=0):
    blob = struct.pack("<4i", pic.bit_depth, len(pic.rows), len(areas), reps)
    for r, (cur, p1, p2) in enumerate(pic.rows):
        blob += struct.pack("<3i", cur.shape[1], cur.shape[0], row_flags(pic, r))
    for r, (cur, p1, p2) in enumerate(pic.rows):
        for p in (cur, None if pic.same(r) else p1, p2):
            if p is not None:
                blob += np.ascontiguousarray(p, np.int16).tobytes()
    return blob + np.ascontiguousarray(areas, VR.AREA_DTYPE).tobytes()


def x86_may_differ(case, a):
    """-> ( spatial, temporal ): where the x86 row of this reference build is ANOTHER function than the scalar row (CommonLib/x86/BufferX86.h:1715-2488)
    spatial   AvgHighPassWithDownsampling_SIMD returns 0 for a width <= 6 (:2228)
    temporal  all four entries sum in 16-bit lanes with saturating horizontal adds (:1927, :2041, :2339, :2427): two-level planes at the ends of the sample range saturate them;
              HDHighPass_SIMD adds the | t | of two neighbours BEFORE ( 1 + 3 .. ) >> 1 (:1919-1925) for a width > 8; HDHighPass_SIMD / HDHighPass2_SIMD read one row too high for
              a width <= 8 (:1906, :2003-2011); the two down-sampling entries drop the row's last cell where ( width - 4 ) % 8 == 2 (:2320, :2354)"""
    ds, order, w = int(a["ds"]), int(a["order"]), int(a["w"])
    two_level = case.picture.name.startswith("ext")
    temporal = order > 0 and (two_level or (ds == 0 and (order == 1 or w <= 8)) or (ds == 1 and (w - 4) % 8 == 2))
    return ds == 1 and w <= 6, temporal


def reference(exe, case):
    """-> the scalar row's results (RESULT [n]), the number of areas on which the x86 row differs; fails unless the x86 row agrees wherever x86_may_differ does not name a reason"""
    raw = np.frombuffer(run(exe, request(case.picture, case.areas)), RESULT).reshape(2, len(case.areas))
    differ = 0
    for i, a in enumerate(case.areas):
        s, x = raw[0][i], raw[1][i]
        spat, temp = x86_may_differ(case, a)
        assert s["rec"][2] == x["rec"][2] and s["rec"][3] == x["rec"][3] and s["avg"] == x["avg"], "case %s area %d: the rows differ in getAvg" % (case.name, i)
        assert spat or (s["rec"][0] == x["rec"][0] and s["hp"][0] == x["hp"][0] and s["int"][0] == x["int"][0]), "case %s area %d: the rows differ in the spatial part" % (case.name, i)
        assert temp or (s["rec"][1] == x["rec"][1] and s["hp"][1] == x["hp"][1] and s["int"][1] == x["int"][1]), "case %s area %d: the rows differ in the temporal part" % (case.name, i)
        assert spat or temp or s.tobytes() == x.tobytes(), "case %s area %d: the rows differ" % (case.name, i)
        differ += s.tobytes() != x.tobytes()
    return raw[0], differ


def main(exe):
    pics, cases = VC.pictures(), VC.cases()
    arrays = {"pictures": np.array(list(pics)), "cases": np.array(list(cases))}
    for name, p in pics.items():
        arrays[name + "_hdr"] = np.array([p.bit_depth, len(p.rows)] + [row_flags(p, r) for r in range(len(p.rows))], np.int32)
        for r, (cur, p1, p2) in enumerate(p.rows):
            arrays["%s_c%d" % (name, r)] = cur
            if p1 is not None and not p.same(r):
                arrays["%s_d1%d" % (name, r)] = (p1.astype(np.int32) - cur).astype(np.int16)
            if p2 is not None:
                arrays["%s_d2%d" % (name, r)] = (p2.astype(np.int32) - p1).astype(np.int16)
    seen, differ = {}, 0
    for name, c in cases.items():
        ref, d = reference(exe, c)
        differ += d
        rec, hp, ints, avg = VC.expected(c)
        for k, (got, want) in enumerate(((ref["rec"], rec), (ref["hp"], hp), (ref["int"], ints), (ref["avg"], avg))):
            assert np.array_equal(got, want), "case %s: the model differs from the reference in %s at areas %s" % (name, ("the sums", "the doubles", "the integers", "getAvg")[k],
                                                                                                              np.argwhere(got != want)[:4].tolist())
        arrays[name + "_pic"] = np.array(list(pics).index(c.picture.name), np.int32)
        arrays[name + "_areas"] = np.ascontiguousarray(c.areas).view(np.uint8).reshape(len(c.areas), 40)
        arrays[name + "_rec"], arrays[name + "_hp"], arrays[name + "_int"], arrays[name + "_avg"] = ref["rec"].copy(), ref["hp"].copy(), ref["int"].copy(), ref["avg"].copy()
        for a, r in zip(c.areas, ref["rec"]):
            key = (int(a["ds"]), int(a["order"]))
            seen[key] = seen.get(key, False) or (int(r[0]) > 0 and (a["order"] == 0 or int(r[1]) > 0))
    missing = [k for k in ((f, o) for f in (0, 1) for o in (0, 1, 2)) if not seen.get(k)]
    assert not missing, "( form, order ) without a non-zero sum: %s" % missing
    np.savez_compressed(VR.GOLDEN, **arrays)
    print("%d pictures, %d cases, %d areas (the x86 row differs on %d, each for a reason x86_may_differ names; the scalar row is recorded), every form x order with non-zero sums -> %s (%d bytes)"
          % (len(pics), len(cases), sum(len(c.areas) for c in cases.values()), differ, VR.GOLDEN, os.path.getsize(VR.GOLDEN)))


def time_reference(exe, reps=7):
    sys.path.insert(0, os.path.join(os.path.dirname(HERE), "tools"))
    import visact_time as VT
    for label, (pic, lists) in VT.pictures().items():
        for order, areas in lists.items():
            s = np.frombuffer(run(exe, request(pic, areas, reps)), np.float64, 1)[0]
            print("CPU, one core, the reference's x86 row, %s, order %d: filterAndCalculateAverageActivity + getAvg over the %d areas %.2f ms" % (label, order, len(areas), 1e3 * s))


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[2] == "--time":
        time_reference(sys.argv[1])
    else:
        main(sys.argv[1])
