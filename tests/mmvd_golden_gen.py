#!/usr/bin/env python3
"""Driver of tests/mmvd_golden_gen.cpp: writes the plane sets and the case table, runs the generator — which runs the reference's own setMmvdMergeCandiInfo, clipMv,
InterPrediction::motionCompensation ( mcControl = 2 | 1 ) and the DistParam functions of DF_HAD and DF_HAD_fast on its scalar and on its x86 row and fails when the rows are
the same functions or disagree —, compares everything it returned with the model of tests/mmvd_ref.py — a difference in a vector, a prediction sample or a cost fails —,
checks that the recorded cases reach every branch of mmvd_ref.REQUIRED, records the walk traces ( EncCu::xCheckMMVDCand itself, m_MMVD 1 .. 4, cost arrays with ties ) and
compares them with the plain restatement of tests/mmvd_walk_ref.py, and writes tests/golden/mmvd.npz ( arrays only ):

  sets      int32 [ nSets, 3 ]        geometry ( index into GEOM_NAMES ), bit depth, kind ( index into KINDS ) of the planes a case reads — the planes themselves are
  set_crc   uint32 [ nSets ]          tests/mmvd_cases.planes(): made from a seed, and held here by the CRC-32 of their bytes ( references, then the original )
  cases     int32 [ n, 34 ]           as the generator reads them
  cands     int32 [ n, 2, 32, 13 ]    as it wrote them, -1 rows for a base without lists
  cost      uint32 [ n, 64, 2 ]       DF_HAD and DF_HAD_fast of every requested candidate ( 0 elsewhere )
  pred_crc  uint32 [ n, 64 ]          CRC-32 of the int16 prediction block of every requested candidate ( 0 elsewhere )
  pred_at   int32 [ m, 2 ]            ( case, val ) of the candidates whose prediction is stored whole: the first two requested ones of every case with at most 1024 samples
  pred_off  int64 [ m + 1 ], pred int16   their samples, row by row
  walk_in / walk_out                  the records of tests/mmvd_walk_ref.py

usage: tests/mmvd_golden_gen.py <path of the compiled generator>
       tests/mmvd_golden_gen.py --time <path of the compiled generator> [reps]   the reference's own loop over the list of tools/mmvd_time.py on one core (a context figure)"""
import os
import subprocess
import sys
import tempfile
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import mmvd_cases as MC  # noqa: E402
import mmvd_extremes as MX  # noqa: E402
import mmvd_ref as MR  # noqa: E402
import mmvd_walk_ref as WR  # noqa: E402

GEOM_NAMES = ("small", "large", "hd")
KINDS = ("natural", "two_level")
STORE_MAX, STORE_PER_CASE = 1024, 2


def case_list():
    rng = np.random.default_rng(77)
    out = MC.cases() + MX.cases()
    for k in range(120):
        out.append(MC.random_cu(rng, "rand%d" % k, ("small", 10, "HAD", k & 1), 32, 64))
    return out


def set_key(c):
    return (c["group"][0], c["group"][1], c.get("planes", "natural"))


def table(cl):
    """-> ( the set keys in first-seen order, int32 [ n, 34 ] )"""
    keys, t = [], np.zeros((len(cl), 34), np.int32)
    for i, c in enumerate(cl):
        k = set_key(c)
        if k not in keys:
            keys.append(k)
        ctu = MC.GEOMS[c["group"][0]][2]
        m = [int(v) - (1 << 32) if int(v) >= 1 << 31 else int(v) for v in c["mask"]]
        t[i, :10] = (keys.index(k), c["group"][1], ctu, c["group"][3], c["cu_x"], c["cu_y"], c["w"], c["h"], m[0], m[1])
        for b, bs in enumerate(c["bases"]):
            t[i, 10 + 12 * b:22 + 12 * b] = (*bs["mv"][0], *bs["mv"][1], bs["ref"][0], bs["ref"][1], *bs["poc"], *bs["lt"], bs["bcw"], bs["alt"])
    return keys, t


def set_bytes(key):
    refs, org = MC.planes(*key)
    return b"".join(np.ascontiguousarray(p, np.int16).tobytes() for p in list(refs) + [org])


def write_input(path, keys, t):
    with open(path, "wb") as f:
        f.write(np.array([len(keys), len(t)], np.int32).tobytes())
        for k in keys:
            pw, ph, _, m = MC.GEOMS[k[0]]
            f.write(np.array([pw, ph, m, MC.N_REF], np.int32).tobytes() + set_bytes(k))
        f.write(t.tobytes())


def case_of(row, keys):
    """a table row back as the model's CU dict (what the CPU tier replays) -> ( cu, ( pic_w, pic_h, ctu, dis_frac ), set key )"""
    key = tuple(keys[int(row[0])])
    pw, ph, ctu, m = MC.GEOMS[key[0]]
    bases = []
    for b in (0, 1):
        q = [int(v) for v in row[10 + 12 * b:22 + 12 * b]]
        bases.append(dict(mv=((q[0], q[1]), (q[2], q[3])), ref=(q[4], q[5]), poc=(q[6], q[7]), lt=(q[8], q[9]), bcw=q[10], alt=q[11]))
    x, y = int(row[4]), int(row[5])
    cu = dict(w=int(row[6]), h=int(row[7]), cu_x=x, cu_y=y, bases=tuple(bases), mask=(int(row[8]) & 0xFFFFFFFF, int(row[9]) & 0xFFFFFFFF), pos=[[(m + x, m + y)] * 2] * 2, org_pos=(m + x, m + y))
    return cu, (pw, ph, int(row[2]), int(row[3])), key


def compare_vectors(c, geo, rec, cnt=None):
    """the generator's 13 numbers of every candidate of a case against the model -> number compared"""
    pw, ph, ctu, df = geo
    n = 0
    for b in (0, 1):
        bs = c["bases"][b]
        if bs["ref"][0] < 0 and bs["ref"][1] < 0:
            assert (rec[b] == -1).all()
            continue
        for k in range(32):
            m, g = MR.candidate(c, 32 * b + k, pw, ph, ctu, df, cnt), [int(v) for v in rec[b, k]]
            bi_cut = bs["ref"][0] >= 0 and bs["ref"][1] >= 0 and c["w"] + c["h"] == 12
            ref = [bs["ref"][0] >= 0, bs["ref"][1] >= 0 and not bi_cut]          # the lists cu.refIdx names: before identical motion, which motionCompensation decides
            assert (g[0], g[1]) == m["stored"][0] and (g[2], g[3]) == m["stored"][1], ("stored vectors", b, k, g, m)
            assert [g[4] >= 0, g[5] >= 0] == ref and g[6] == ref[0] + 2 * ref[1], ("lists", b, k, g, m)
            assert g[7] == (bs["bcw"] if ref[0] and ref[1] else 2) and g[8] == (3 if bs["alt"] else 0), ("BcwIdx / imv", b, k, g, m)
            assert all((g[9 + 2 * l], g[10 + 2 * l]) == m["mv"][l] for l in (0, 1) if ref[l]), ("clipped vectors", b, k, g, m)
            n += 1
    return n


def crc(a):
    return zlib.crc32(np.ascontiguousarray(a, np.int16).tobytes()) & 0xFFFFFFFF


def model_case(lib, c, geo, key, cnt=None):
    """the model's prediction and both costs of every requested candidate -> { val: ( prediction, HAD, HAD_fast ) }"""
    pw, ph, ctu, df = geo
    refs, org = MC.planes(*key)
    out = {}
    for val in MR.vals_of(c["mask"]):
        cand = MR.candidate(c, val, pw, ph, ctu, df)
        pred = MR.predict(lib, refs, c, val, cand, key[1], cnt)
        out[val] = (pred, MR.cost(lib, org, c["org_pos"][0], c["org_pos"][1], pred, key[1], False, cnt), MR.cost(lib, org, c["org_pos"][0], c["org_pos"][1], pred, key[1], True, cnt))
    return out


def time_mode(gen, reps):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import mmvd_time as MT
    group, cl = MT.picture_list(np.random.default_rng(404))
    keys, t = table(cl)
    with tempfile.TemporaryDirectory() as d:
        fin = os.path.join(d, "in.bin")
        write_input(fin, keys, t)
        n, sec = subprocess.check_output([gen, "--time", fin, str(reps)], text=True).split()
    print("%d CUs, %s candidates: the reference's own loop ( x86 row, one core ), best of %d: %.1f ms" % (len(cl), n, reps, 1e3 * float(sec)))


def main():
    if sys.argv[1] == "--time":
        return time_mode(sys.argv[2], int(sys.argv[3]) if len(sys.argv) > 3 else 3)
    from oracle.oracle import Oracle
    lib = Oracle()
    gen = sys.argv[1]
    cl = case_list()
    keys, t = table(cl)
    walk_in = WR.walk_cases()
    with tempfile.TemporaryDirectory() as d:
        fin, fout, win, wout = (os.path.join(d, n) for n in ("in.bin", "out.bin", "walk_in.bin", "walk_out.bin"))
        write_input(fin, keys, t)
        subprocess.check_call([gen, fin, fout])
        raw = np.fromfile(fout, np.uint8)
        with open(win, "wb") as f:
            f.write(np.int32(len(walk_in)).tobytes() + walk_in.tobytes())
        subprocess.check_call([gen, "--walk", win, wout])
        walk_out = np.fromfile(wout, WR.WALK_OUT)
    n = len(cl)
    cands, cost, pred_crc = np.full((n, 2, 32, 13), -1, np.int32), np.zeros((n, 64, 2), np.uint32), np.zeros((n, 64), np.uint32)
    pred_at, pred_off, preds, at = [], [0], [], 0
    cnt, n_vec, n_pred = {}, 0, 0
    for i, c0 in enumerate(cl):
        c, geo, key = case_of(t[i], keys)
        want = model_case(lib, c, geo, key, cnt)
        stored = 0
        for b in (0, 1):
            if c["bases"][b]["ref"][0] < 0 and c["bases"][b]["ref"][1] < 0:
                continue
            for k in range(32):
                val = 32 * b + k
                cands[i, b, k] = raw[at:at + 52].view(np.int32)
                at += 52
                if not (c["mask"][b] >> k) & 1:
                    continue
                refined, had, fast = (int(v) for v in raw[at:at + 12].view(np.uint32))
                at += 12
                p = raw[at:at + 2 * c["w"] * c["h"]].view(np.int16).reshape(c["h"], c["w"])
                at += 2 * c["w"] * c["h"]
                assert refined == 0, ("motionCompensation applied BDOF or DMVR", c0["name"], val)
                assert np.array_equal(p, want[val][0]), ("prediction", c0["name"], val, np.argwhere(p != want[val][0])[:4].tolist())
                assert (had, fast) == want[val][1:], ("cost", c0["name"], val, had, fast, want[val][1:])
                cost[i, val], pred_crc[i, val] = (had, fast), crc(p)
                n_pred += 1
                if c["w"] * c["h"] <= STORE_MAX and stored < STORE_PER_CASE:
                    pred_at.append((i, val))
                    preds.append(p.reshape(-1).copy())
                    pred_off.append(pred_off[-1] + p.size)
                    stored += 1
        n_vec += compare_vectors(c, geo, cands[i], cnt)
    assert at == raw.size
    missing = [k for k in MR.REQUIRED if not cnt.get(k)]
    assert not missing, missing
    for r, o in zip(walk_in, walk_out):
        tested, bco, bcm, bd = WR.walk(r["dist"], r["bits_cost"], r["list_cost"][:r["n_list"]], int(r["mmvd"]), int(r["dis_num"]), int(r["num_valid"]), int(r["mrg_cnd0"]), int(r["mrg_cnd1"]),
                                       int(r["max_tracking"]), int(r["skip"]))
        assert tested == o["tested"][:o["count"]].tolist() and (bco, bcm, bd) == (o["best_cost_offset"], o["best_cost_merge"], o["best_dir"]), ("walk", r, o, tested)
    sets = np.array([(GEOM_NAMES.index(k[0]), k[1], KINDS.index(k[2])) for k in keys], np.int32)
    set_crc = np.array([zlib.crc32(set_bytes(k)) & 0xFFFFFFFF for k in keys], np.uint32)
    out = os.path.join(ROOT, "tests", "golden", "mmvd.npz")
    np.savez_compressed(out, sets=sets, set_crc=set_crc, cases=t, cands=cands, cost=cost, pred_crc=pred_crc, pred_at=np.array(pred_at, np.int32), pred_off=np.array(pred_off, np.int64),
                        pred=np.concatenate(preds), walk_in=walk_in, walk_out=walk_out)
    print("%d cases: %d candidates' vectors, %d predictions and costs equal the model on both rows; %d walk traces; %s: %d bytes"
          % (n, n_vec, n_pred, len(walk_in), out, os.path.getsize(out)))


if __name__ == "__main__":
    main()
