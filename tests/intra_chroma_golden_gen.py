"""Driver of tests/intra_chroma_golden_gen.cpp: hands every case of tests/intra_chroma_cases.py to the generator (its path is argv[1]; compile command in its header
comment) and writes tests/golden/intra_chroma.npz — arrays only.

cases                  the names
<case>_hdr             int32 [ w, h, bit depth, flags, n_above_right, n_left_below, mode_mask, pred_mask ]
<case>_cand            uint8 [8]: the candidate modes by slot
<case>_luma            int16 [ 4h + 6 ][ 4w + 6 ]: the window of reconstructed luma, the collocated area's top-left sample at ( 4, 4 )
<case>_lines           int16 [2][ 2w + 1 + 2h + 1 ]: the unfiltered Cb and Cr reference lines (top row from the corner, then the left row from the corner)
<case>_org             int16 [2][h][w]
<case>_cost            uint32 [8]: min( 2 SAD, HAD ) of Cb plus the same of Cr per scored slot, 0 elsewhere
<case>_prm             int32 [8][2][3]: ( a, b, shift ) of xGetLMParameters per slot and component, 0 for regular modes
<case>_pred            int16 [ slots of pred_mask, ascending ][2][h][w]
Both rows of the reference run every case and every slot (the generator itself fails unless the x86 row's function pointers differ from the scalar ones), each with a
different fill around the luma window.  The driver fails unless the rows agree in every sample, cost and parameter, unless the availability the reference derived from the
CodingStructure equals the case's flags and counts, unless the model (tests/intra_chroma_ref.py) equals the reference, and unless the model's branch counters show every
branch of intra_chroma_cases.REQUIRED.
usage: python tests/intra_chroma_golden_gen.py /path/to/intra_chroma_golden_gen
       python tests/intra_chroma_golden_gen.py /path/to/intra_chroma_golden_gen --time      (a CPU context figure for profiles/intra_chroma.md: the reference's own loop over
                                                                                             the list of tools/intra_chroma_time.py, one core; writes nothing)"""
import os
import struct
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import intra_chroma_cases as CC  # noqa: E402
import intra_chroma_ref as CR  # noqa: E402


def run(exe, blob):
    with tempfile.TemporaryDirectory() as td:
        fi, fo = os.path.join(td, "in.bin"), os.path.join(td, "out.bin")
        with open(fi, "wb") as f:
            f.write(blob)
        subprocess.check_call([exe, fi, fo])
        return open(fo, "rb").read()


def request(case_list, reps=0, mode_mask=None):
    blob = [struct.pack("<2i", len(case_list), reps)]
    for c in case_list:
        mm = c.mode_mask if mode_mask is None else mode_mask
        blob.append(struct.pack("<17i", c.w, c.h, c.bit_depth, c.flags, c.n_ar, c.n_lb, mm, *c.cand, c.luma.shape[1], c.luma.shape[0]))
        blob += [c.luma.tobytes(), c.lines.tobytes(), c.org.tobytes()]
    return b"".join(blob)


def reference(exe, case_list):
    """-> per case ( costs [8], params [8][2][3], predictions [ every scored slot ][2][h][w] ) of the scalar row; fails unless the x86 row agrees and the availability holds"""
    raw = run(exe, request(case_list))
    per_row = sum(16 + len(CR.mask_bits(c.mode_mask)) * (4 + 24 + 4 * c.w * c.h) for c in case_list)
    assert len(raw) == 2 * per_row, "the generator's answer has %d bytes, expected %d" % (len(raw), 2 * per_row)
    rows = []
    for r in range(2):
        at, out = r * per_row, []
        for c in case_list:
            av = struct.unpack_from("<4i", raw, at)
            want = (int(bool(c.flags & CR.F_ABOVE)), int(bool(c.flags & CR.F_LEFT)), c.n_ar, c.n_lb)
            assert av == want, "case %s: the reference derived the availability %s from its CodingStructure, the case says %s" % (c.name, av, want)
            at += 16
            costs, prm, preds = np.zeros(CR.NUM_SLOTS, np.uint32), np.zeros((CR.NUM_SLOTS, 2, 3), np.int32), []
            for s in CR.mask_bits(c.mode_mask):
                costs[s] = struct.unpack_from("<I", raw, at)[0]
                prm[s] = np.frombuffer(raw, np.int32, 6, at + 4).reshape(2, 3)
                preds.append(np.frombuffer(raw, np.int16, 2 * c.w * c.h, at + 28).reshape(2, c.h, c.w))
                at += 28 + 4 * c.w * c.h
            out.append((costs, prm, np.stack(preds)))
        rows.append(out)
    for c, (sc, sp, spr), (xc, xp, xpr) in zip(case_list, rows[0], rows[1]):
        assert np.array_equal(sc, xc), "case %s: the rows differ in the cost of slots %s" % (c.name, np.argwhere(sc != xc).reshape(-1).tolist())
        assert np.array_equal(sp, xp), "case %s: the rows differ in the parameters" % c.name
        assert np.array_equal(spr, xpr), "case %s: the rows differ in a prediction" % c.name
    return rows[0]


def main(exe):
    cases = CC.cases()
    ref = reference(exe, list(cases.values()))
    arrays, cnt = {"cases": np.array(list(cases))}, {}
    for (name, c), (rc, rp, rpred) in zip(cases.items(), ref):
        full = CC.Case(name, c.w, c.h, c.bit_depth, c.flags, c.n_ar, c.n_lb, c.cand, c.luma, c.lines, c.org, c.mode_mask, c.mode_mask)
        _, _, mfull = CC.expected(full)
        mc, mp, mpred = CC.expected(c, cnt)
        slots = CR.mask_bits(c.mode_mask)
        for k, s in enumerate(slots):
            assert np.array_equal(mp[s], rp[s]), "case %s slot %d (mode %d): the model's ( a, b, shift ) %s differ from the reference's %s" % (name, s, c.cand[s], mp[s].tolist(), rp[s].tolist())
            assert np.array_equal(mfull[k], rpred[k]), "case %s slot %d (mode %d): the model's prediction differs from the reference at %s" % (name, s, c.cand[s], np.argwhere(mfull[k] != rpred[k])[:4].tolist())
        assert np.array_equal(mc, rc), "case %s: the model's cost differs from the reference in slots %s" % (name, np.argwhere(mc != rc).reshape(-1).tolist())
        keep = [k for k, s in enumerate(slots) if (c.pred_mask >> s) & 1]
        assert np.array_equal(mpred, rpred[keep])
        arrays[name + "_hdr"] = np.array([c.w, c.h, c.bit_depth, c.flags, c.n_ar, c.n_lb, c.mode_mask, c.pred_mask], np.int32)
        arrays[name + "_cand"] = np.array(c.cand, np.uint8)
        arrays[name + "_luma"], arrays[name + "_lines"], arrays[name + "_org"] = c.luma, c.lines, c.org
        arrays[name + "_cost"], arrays[name + "_prm"], arrays[name + "_pred"] = rc.copy(), rp.copy(), rpred[keep].copy()
    missing = [k for k in CC.REQUIRED if not cnt.get(k)]
    assert not missing, "branches the fixture does not exercise: %s" % missing
    np.savez_compressed(CR.GOLDEN, **arrays)
    print("%d cases, %d (block, slot) pairs, both rows agree, the availability agrees, the model agrees, branches %s -> %s (%d bytes)"
          % (len(cases), sum(len(CR.mask_bits(c.mode_mask)) for c in cases.values()), {k: cnt[k] for k in CC.REQUIRED}, CR.GOLDEN, os.path.getsize(CR.GOLDEN)))


def time_reference(exe, reps=5):
    sys.path.insert(0, os.path.join(os.path.dirname(HERE), "tools"))
    import intra_chroma_time as CT
    blocks = CT.picture_cases()
    for label, mm in (("the five slots the reference pre-checks", CT.PRECHECK_MASK), ("all eight slots", 0xff)):
        s = np.frombuffer(run(exe, request(blocks, reps, mm)), np.float64, 1)[0]
        print("CPU, one core, the reference's x86 row: loadLMLumaRecPels + predict + 2 x ( SAD, HAD ) per slot of the %d blocks of the list, %s (%d pairs) %.2f ms"
              % (len(blocks), label, len(blocks) * bin(mm).count("1"), 1e3 * s))


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[2] == "--time":
        time_reference(sys.argv[1])
    else:
        main(sys.argv[1])
