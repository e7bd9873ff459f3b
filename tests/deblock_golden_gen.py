"""Driver of tests/deblock_golden_gen.cpp: hands every case of tests/deblock_cases.py to the generator (its path is argv[1]; compile command in its header comment) and
writes tests/golden/deblock.npz — arrays only.

names                  the case names
<name>_hdr             int32 [ width, height, ctu, bit depth, planes, clip max, beta offsets / 2 [3], tc offsets / 2 [3] ]
<name>_p<c>            the unfiltered planes, int16
<name>_ver, <name>_hor the maps as bytes, uint8 [ height / 4 ][ width / 4 ][ 6 ]
<name>_v<c>            plane after xDeblockArea<EDGE_VER> over every CTU, minus the unfiltered plane, int16
<name>_d<c>            plane after xDeblockArea<EDGE_VER> and then <EDGE_HOR> over every CTU, minus the unfiltered plane, int16
Both rows of the reference run every case — LoopFilter( false ), the scalar row, and the x86 row — on copies of the planes in different surroundings; the driver fails
unless they agree.  It then runs the model (tests/deblock_ref.py) and, once the model equals the recorded planes on every case, asserts from the model's branch counters
that the fixture is not vacuous (deblock_ref.coverage; tests/test_deblock_cpu.py repeats it).
usage: python tests/deblock_golden_gen.py /path/to/deblock_golden_gen
       python tests/deblock_golden_gen.py /path/to/deblock_golden_gen --time      (a context figure for profiles/deblock.md: the reference's own xDeblockArea over the
                                                                                   1920x1080 picture of tools/deblock_time.py, one core; writes nothing)"""
import os
import struct
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import deblock_cases as DC  # noqa: E402
import deblock_ref as DR  # noqa: E402


def run(exe, blob):
    with tempfile.TemporaryDirectory() as td:
        fi, fo = os.path.join(td, "in.bin"), os.path.join(td, "out.bin")
        with open(fi, "wb") as f:
            f.write(blob)
        subprocess.check_call([exe, fi, fo])
        return open(fo, "rb").read()


def request(c, reps=0):
    clip_bd = int(c.clip[0][1] + 1).bit_length() - 1
    assert all(cl == (0, (1 << clip_bd) - 1) for cl in c.clip), "a ClpRng of the reference is [0, 2^bd - 1]"
    blob = struct.pack("<13i", c.width, c.height, c.ctu, c.bit_depth, int(len(c.planes) == 3), clip_bd, *c.beta_offsets, *c.tc_offsets, reps)
    return blob + b"".join(np.ascontiguousarray(p, np.int16).tobytes() for p in c.planes) + np.ascontiguousarray(c.lfp_ver).tobytes() + np.ascontiguousarray(c.lfp_hor).tobytes()


def reference(exe, c):
    """-> ( planes after VER, planes after VER + HOR ) of the scalar row; fails unless the x86 row agrees"""
    raw, at, rows = run(exe, request(c)), 0, []
    for r in range(2):
        stages = []
        for _ in range(2):
            planes = []
            for p in c.planes:
                planes.append(np.frombuffer(raw, np.int16, p.size, at).reshape(p.shape))
                at += 2 * p.size
            stages.append(planes)
        rows.append(stages)
    assert at == len(raw)
    for s in range(2):
        for k in range(len(c.planes)):
            assert np.array_equal(rows[0][s][k], rows[1][s][k]), "case %s plane %d after %s: the scalar and the x86 row differ" % (c.name, k, ("VER", "VER + HOR")[s])
    return rows[0]


def main(exe):
    cases = DC.cases()
    arrays, cnt = {"names": np.array(list(cases))}, DR.Counter()
    for name, c in cases.items():
        ver, both = reference(exe, c)
        arrays[name + "_hdr"] = np.array([c.width, c.height, c.ctu, c.bit_depth, len(c.planes), c.clip[0][1], *c.beta_offsets, *c.tc_offsets], np.int32)
        arrays[name + "_ver"] = np.ascontiguousarray(c.lfp_ver).view(np.uint8).reshape(c.height // 4, c.width // 4, 6)
        arrays[name + "_hor"] = np.ascontiguousarray(c.lfp_hor).view(np.uint8).reshape(c.height // 4, c.width // 4, 6)
        m_ver = DR.deblock(c.planes, c.lfp_ver, c.lfp_hor, c.ctu, c.bit_depth, c.clip, c.beta_offsets, c.tc_offsets, dirs=DR.VER)
        m_both = DR.deblock(c.planes, c.lfp_ver, c.lfp_hor, c.ctu, c.bit_depth, c.clip, c.beta_offsets, c.tc_offsets, counters=cnt)
        for k, p in enumerate(c.planes):
            arrays["%s_p%d" % (name, k)] = p
            arrays["%s_v%d" % (name, k)] = (ver[k].astype(np.int32) - p).astype(np.int16)
            arrays["%s_d%d" % (name, k)] = (both[k].astype(np.int32) - p).astype(np.int16)
            assert np.array_equal(m_ver[k], ver[k]), "case %s plane %d: the model differs from the reference after VER at %s" % (name, k, np.argwhere(m_ver[k] != ver[k])[:4].tolist())
            assert np.array_equal(m_both[k], both[k]), "case %s plane %d: the model differs from the reference after VER + HOR at %s" % (name, k, np.argwhere(m_both[k] != both[k])[:4].tolist())
            assert np.any(both[k] != ver[k]) and np.any(ver[k] != p), "case %s plane %d: a pass changes nothing" % (name, k)
    missing = DR.coverage(cnt)
    assert not missing, "branches the cases never take: %s" % missing
    np.savez_compressed(DR.GOLDEN, **arrays)
    print("%d cases, every branch taken (%s) -> %s (%d bytes)" % (len(cases), ", ".join("%s %d" % kv for kv in sorted(cnt.items())), DR.GOLDEN, os.path.getsize(DR.GOLDEN)))


def time_reference(exe, reps=7):
    sys.path.insert(0, os.path.join(os.path.dirname(HERE), "tools"))
    import deblock_time as DT
    for ctu in (128, 64):
        s = np.frombuffer(run(exe, request(DT.picture(ctu), reps)), np.float64, 1)[0]
        print("CPU, one core, the reference's x86 row, CTU %3d: xDeblockArea<EDGE_VER> + <EDGE_HOR> over the picture %.2f ms" % (ctu, 1e3 * s))


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[2] == "--time":
        time_reference(sys.argv[1])
    else:
        main(sys.argv[1])
