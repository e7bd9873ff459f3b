"""Driver of tests/intra_golden_gen.cpp: hands every case of tests/intra_cases.py to the generator (its path is argv[1]; compile command in its header comment) and writes
tests/golden/intra.npz — arrays only.

cases                  the names
<case>_hdr             int32 [ w, h, bit depth, multi_ref_idx ]
<case>_lines           int16: the unfiltered reference lines (top row from the corner, then the left row from the corner)
<case>_org             int16 [h][w]
<case>_modes           uint32 [3]: the mask of scored modes; <case>_pmodes: the mask of modes whose prediction is stored (all of them for blocks of up to 256 samples)
<case>_cost            uint32 [67]: min( HAD, 2 SAD ) per scored mode, 0 elsewhere
<case>_pred            int16 [ stored modes, ascending ][h][w]
Both rows of the reference run every case and every mode — IntraPrediction( false ) + RdCost::create( false ), the scalar row, and IntraPrediction( true ) +
RdCost::create( true ), the x86 row (the generator itself fails unless the x86 row's function pointers differ from the scalar ones).  The driver fails unless the rows agree in
every sample and every cost, unless the model (tests/intra_ref.py) equals them, and unless the model's branch counters show every branch of intra_cases.REQUIRED.
usage: python tests/intra_golden_gen.py /path/to/intra_golden_gen
       python tests/intra_golden_gen.py /path/to/intra_golden_gen --time      (a CPU context figure for profiles/intra.md: the reference's own predict + score loop over the
                                                                               list of tools/intra_time.py, one core; writes nothing)"""
import os
import struct
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import intra_cases as IC  # noqa: E402
import intra_ref as IR  # noqa: E402


def run(exe, blob):
    with tempfile.TemporaryDirectory() as td:
        fi, fo = os.path.join(td, "in.bin"), os.path.join(td, "out.bin")
        with open(fi, "wb") as f:
            f.write(blob)
        subprocess.check_call([exe, fi, fo])
        return open(fo, "rb").read()


def request(blocks, reps=0):
    """blocks: ( w, h, bit_depth, mri, modes, lines, org )"""
    blob = [struct.pack("<2i", len(blocks), reps)]
    for (w, h, bd, mri, modes, lines, org) in blocks:
        blob.append(struct.pack("<5i", w, h, bd, mri, len(modes)))
        blob.append(np.asarray(modes, np.int32).tobytes())
        blob.append(np.ascontiguousarray(lines, np.int16).tobytes())
        blob.append(np.ascontiguousarray(org, np.int16).tobytes())
    return b"".join(blob)


def reference(exe, case_list):
    """-> per case ( costs [67], predictions [ every scored mode ][h][w] ) of the scalar row; fails unless the x86 row agrees"""
    raw = run(exe, request([(c.w, c.h, c.bit_depth, c.mri, c.modes, c.lines, c.org) for c in case_list]))
    per_row = sum(len(c.modes) * (4 + 2 * c.w * c.h) for c in case_list)
    assert len(raw) == 2 * per_row, "the generator's answer has %d bytes, expected %d" % (len(raw), 2 * per_row)
    rows = []
    for r in range(2):
        at, out = r * per_row, []
        for c in case_list:
            costs, preds = np.zeros(IR.NUM_MODES, np.uint32), []
            for m in c.modes:
                costs[m] = struct.unpack_from("<I", raw, at)[0]
                preds.append(np.frombuffer(raw, np.int16, c.w * c.h, at + 4).reshape(c.h, c.w))
                at += 4 + 2 * c.w * c.h
            out.append((costs, np.stack(preds)))
        rows.append(out)
    for c, (sc, sp), (xc, xp) in zip(case_list, rows[0], rows[1]):
        assert np.array_equal(sc, xc), "case %s: the rows differ in the cost of modes %s" % (c.name, np.argwhere(sc != xc).reshape(-1).tolist())
        assert np.array_equal(sp, xp), "case %s: the rows differ in the prediction of modes %s" % (c.name, sorted({c.modes[k] for k in np.argwhere(sp != xp)[:, 0]}))
    return rows[0]


def main(exe):
    cases = IC.cases()
    ref = reference(exe, list(cases.values()))
    arrays, cnt = {"cases": np.array(list(cases))}, {}
    for (name, c), (rc, rp) in zip(cases.items(), ref):
        mc, mp = IC.expected(c, cnt)
        keep = [k for k, m in enumerate(c.modes) if m in c.pred_modes]
        for k, m in enumerate(c.modes):
            full = IR.predict(c.lines, c.w, c.h, m, c.mri, c.bit_depth)
            assert np.array_equal(full, rp[k]), "case %s mode %d: the model's prediction differs from the reference at %s" % (name, m, np.argwhere(full != rp[k])[:4].tolist())
        assert np.array_equal(mc, rc), "case %s: the model's cost differs from the reference in modes %s" % (name, np.argwhere(mc != rc).reshape(-1).tolist())
        assert np.array_equal(mp, rp[keep])
        arrays[name + "_hdr"] = np.array([c.w, c.h, c.bit_depth, c.mri], np.int32)
        arrays[name + "_lines"], arrays[name + "_org"] = c.lines, c.org
        arrays[name + "_modes"], arrays[name + "_pmodes"] = IR.make_mask(c.modes), IR.make_mask(c.pred_modes)
        arrays[name + "_cost"], arrays[name + "_pred"] = rc.copy(), rp[keep].copy()
    missing = [k for k in IC.REQUIRED if not cnt.get(k)]
    assert not missing, "branches the fixture does not exercise: %s" % missing
    np.savez_compressed(IR.GOLDEN, **arrays)
    print("%d cases, %d (block, mode) pairs, both rows agree, the model agrees, branches %s -> %s (%d bytes)"
          % (len(cases), sum(len(c.modes) for c in cases.values()), {k: cnt[k] for k in IC.REQUIRED}, IR.GOLDEN, os.path.getsize(IR.GOLDEN)))


def time_reference(exe, reps=5):
    sys.path.insert(0, os.path.join(os.path.dirname(HERE), "tools"))
    import intra_time as IT
    blocks = IT.picture_blocks()
    s = np.frombuffer(run(exe, request(blocks, reps)), np.float64, 1)[0]
    print("CPU, one core, the reference's x86 row: predict + HAD_2SAD of every mode of the %d blocks of the list (%d pairs) %.2f ms" % (len(blocks), sum(len(b[4]) for b in blocks), 1e3 * s))


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[2] == "--time":
        time_reference(sys.argv[1])
    else:
        main(sys.argv[1])
