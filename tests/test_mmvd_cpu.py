"""CPU tier of the MMVD merge-candidate entry (no device): the model of tests/mmvd_ref.py reaches every branch of REQUIRED on the case list and on the limits list, the record
layouts equal the header, vvhip_mmvd_candidate — the code the kernel derives its vectors with — equals the model's vectors on every candidate of both lists, called
through ctypes on the host library, the model equals what the reference's own functions returned (tests/golden/mmvd.npz: vectors, predictions, costs), and the shim's walk and
BDOF helpers (tests/cpp/mmvd_shim_driver.cpp, compiled here) equal a plain Python restatement and the traces recorded from EncCu::xCheckMMVDCand."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import mmvd_cases as MC  # noqa: E402
import mmvd_extremes as MX  # noqa: E402
import mmvd_ref as MR  # noqa: E402


@pytest.fixture(scope="module")
def modelled(oracle):
    """the model on the case list, once: ( counters, { case name: { val: ( candidate, prediction ) } }, { group: costs } )"""
    cnt, keep, cost = {}, {}, {}
    for group, cl in MC.groups(MC.cases()).items():
        cost[group] = MC.expected_group(oracle, group, cl, cnt, keep)
    return cnt, keep, cost


def test_case_list_covers_required(modelled):
    cnt = modelled[0]
    assert [k for k in MR.REQUIRED if not cnt.get(k)] == []


def test_case_list_has_the_sizes_and_depths():
    L = MC.cases()
    sizes = {(c["w"], c["h"]) for c in L}
    assert {(8, 4), (4, 8), (8, 8), (16, 8), (8, 16), (16, 16), (32, 8), (32, 32), (64, 64), (128, 128)} <= sizes
    assert {c["group"][1] for c in L} == {8, 10, 12} and {c["group"][2] for c in L} == {"HAD", "HAD_fast"} and {c["group"][3] for c in L} == {0, 1}


def test_costs_fit_32_bits(modelled):
    """the bound the header states, and every modelled cost below it (mmvd_ref.cost asserts it per candidate; the limits list drives the extreme)"""
    assert MR.COST_BOUND == 256 * 4193280 == 1073479680 < 1 << 32
    for cost in modelled[2].values():
        req = cost != MC.SENTINEL
        assert req.any() and int(cost[req].max()) <= MR.COST_BOUND


def parse_struct(txt, name):
    body = re.search(r"typedef struct\s*\{([^}]*)\}\s*%s;" % name, txt).group(1)
    sizes, at, fields = {"uint8_t": 1, "int8_t": 1, "int16_t": 2, "int32_t": 4, "uint32_t": 4}, 0, []
    for line in body.splitlines():
        m = re.match(r"\s*(uint8_t|int8_t|int16_t|int32_t|uint32_t)\s+([^;]+);", line)
        if not m:
            continue
        sz = sizes[m.group(1)]
        for decl in m.group(2).split(","):
            d = re.match(r"\s*(\w+)((?:\[\d+\])*)\s*$", decl)
            n = int(np.prod([int(v) for v in re.findall(r"\[(\d+)\]", d.group(2))], dtype=int))
            at = (at + sz - 1) // sz * sz
            fields.append((d.group(1), at, sz, n))
            at += sz * n
    return fields, at


def test_record_layout_equals_the_header():
    """vvhip_mmvd_item and vvhip_mmvd_cand as include/vvenc_hip.h declares them: the same fields at the same offsets in the case list's and in HotPath's dtypes"""
    from vvenc_amd.hotpath import MMVD_CAND_DTYPE, MMVD_ITEM_DTYPE
    txt = open(os.path.join(ROOT, "include", "vvenc_hip.h")).read()
    for name, size, dts in (("vvhip_mmvd_item", 112, (MC.MMVD_ITEM_DTYPE, MMVD_ITEM_DTYPE)), ("vvhip_mmvd_cand", 36, (MMVD_CAND_DTYPE,))):
        fields, at = parse_struct(txt, name)
        assert at == size and (name != "vvhip_mmvd_item" or "sizeof( vvhip_mmvd_item ) == 112" in txt)
        for dt in dts:
            assert dt.itemsize == size and list(dt.names) == [f[0] for f in fields]
            for fname, off, sz, n in fields:
                sub, o = dt.fields[fname][0], dt.fields[fname][1]
                assert o == off and sub.base.itemsize == sz and int(np.prod(sub.shape, dtype=int)) == n, (name, fname)


def host_candidate(lib, rec, val, pw, ph, ctu, df):
    from vvenc_amd.hotpath import MMVD_CAND_DTYPE
    out = np.zeros(1, MMVD_CAND_DTYPE)
    rc = lib.vvhip_mmvd_candidate(rec.ctypes.data_as(C.c_void_p), val, pw, ph, ctu, df, out.ctypes.data_as(C.c_void_p))
    return rc, out[0]


def same(o, cand):
    return [tuple(int(v) for v in o["mv"][l]) for l in (0, 1)] == [tuple(m) for m in cand["mv"]] and [tuple(int(v) for v in o["stored_mv"][l]) for l in (0, 1)] == [tuple(m) for m in cand["stored"]] \
        and [int(v) for v in o["ref_plane"]] == cand["ref"] and int(o["bcw_idx"]) == cand["bcw"] and int(o["alt_hpel"]) == cand["alt"]


def test_host_candidate_equals_the_model(modelled):
    from vvenc_amd.lib import load_library
    lib = load_library()
    n = 0
    for group, cl in MC.groups(MC.cases() + MX.cases()).items():
        pw, ph, ctu, _ = MC.GEOMS[group[0]]
        it = MC.as_list(cl, 208, 208)
        for i, c in enumerate(cl):
            for val in MR.vals_of(c["mask"]):
                rc, o = host_candidate(lib, it[i:i + 1], val, pw, ph, ctu, group[3])
                assert rc == 0 and same(o, MR.candidate(c, val, pw, ph, ctu, group[3])), (c["name"], val)
                n += 1
    assert n > 1600


def test_host_candidate_refuses():
    from vvenc_amd.lib import load_library
    lib = load_library()
    g = ("small", 10, "HAD", 0)
    it = MC.as_list([MC.cu("c", g, 8, 8, 0, 0, MC.base((1, 1), None), None)], 208, 208)
    assert host_candidate(lib, it, 3, 96, 80, 32, 0)[0] == 0
    assert host_candidate(lib, it, 64, 96, 80, 32, 0)[0] != 0 and host_candidate(lib, it, -1, 96, 80, 32, 0)[0] != 0
    assert host_candidate(lib, it, 35, 96, 80, 32, 0)[0] != 0            # base 1 uses neither list
    assert host_candidate(lib, it, 3, 96, 80, 48, 0)[0] != 0
    it[0]["h"] = 2
    assert host_candidate(lib, it, 3, 96, 80, 32, 0)[0] != 0


def test_limits_list_reaches_the_limits(oracle):
    """tests/mmvd_extremes.py: two-level planes at 12 bits with half-sample fractions and bcw_idx 0 / 4 so that both clip ends act, a 128 x 128 CU whose cost comes closest to the
    32-bit bound, base vectors at +-( 2^17 - 1 )"""
    cnt, keep, top = {}, {}, 0
    for group, cl in MC.groups(MX.cases()).items():
        cost = MC.expected_group(oracle, group, cl, cnt, keep)
        top = max(top, int(cost[cost != MC.SENTINEL].max()))
    vmax = (1 << 12) - 1
    for name in ("clip_bcw0", "clip_bcw4"):
        preds = [p for (c, p) in keep[name].values() if c["used"][0] and c["used"][1] and (c["mv"][0][0] & 15) == 8]
        assert preds and any((p == 0).any() for p in preds) and any((p == vmax).any() for p in preds), name
    assert cnt.get("storage_clip") and cnt.get("bcw0") and cnt.get("bcw4")
    assert any(abs(v) == MR.MV_MAX for c in MX.cases() for b in c["bases"] for m in b["mv"] for v in m)
    # the 128 x 128 CU: 256 tiles whose 64 coefficients all have the magnitude 8 * 4095, the DC a quarter: ( 63 * 32760 + 8190 + 2 ) >> 2 each.  No block scores more — the
    # sum of magnitudes is at most 64 * sqrt( 64 * 4095^2 ) —, so the stated bound ( every coefficient at 64 * 4095 ) has a factor of eight in hand
    assert keep["bound_128x128"][0][0]["mv"][0] == (0, 0) and top == 256 * ((63 * 8 * 4095 + (8 * 4095 >> 2) + 2) >> 2) == 132612608 <= MR.COST_BOUND // 8


@pytest.fixture(scope="module")
def golden():
    z = np.load(os.path.join(ROOT, "tests", "golden", "mmvd.npz"))
    import mmvd_golden_gen as GG
    keys = [(GG.GEOM_NAMES[g], int(bd), GG.KINDS[k]) for g, bd, k in z["sets"]]
    return z, keys


def test_fixture_planes_are_the_case_lists_planes(golden):
    """the fixture holds the planes by their CRC-32: the seeded planes of tests/mmvd_cases.py are the ones the reference predicted from"""
    import zlib
    import mmvd_golden_gen as GG
    z, keys = golden
    assert [zlib.crc32(GG.set_bytes(k)) & 0xFFFFFFFF for k in keys] == z["set_crc"].tolist()


def test_model_equals_the_fixture(golden, oracle):
    """tests/golden/mmvd.npz: what the reference's own setMmvdMergeCandiInfo, clipMv, motionCompensation ( mcControl = 2 | 1 ) and the DistParam functions of DF_HAD and
    DF_HAD_fast returned on both rows (tests/mmvd_golden_gen.cpp) — the model's vectors on every candidate, its prediction ( by CRC-32 on every requested candidate, sample by
    sample on the stored ones ) and both costs; and the fixture reaches every branch of REQUIRED"""
    import mmvd_golden_gen as GG
    z, keys = golden
    cases, cands, cost, pred_crc = z["cases"], z["cands"], z["cost"], z["pred_crc"]
    stored = {(int(i), int(v)): z["pred"][int(a):int(b)] for (i, v), a, b in zip(z["pred_at"], z["pred_off"][:-1], z["pred_off"][1:])}
    cnt, n_vec, n_pred, sizes = {}, 0, 0, set()
    for i in range(len(cases)):
        c, geo, key = GG.case_of(cases[i], keys)
        n_vec += GG.compare_vectors(c, geo, cands[i], cnt)
        sizes.add((c["w"], c["h"]))
        for val, (pred, had, fast) in GG.model_case(oracle, c, geo, key, cnt).items():
            assert (had, fast) == tuple(int(v) for v in cost[i, val]) and GG.crc(pred) == int(pred_crc[i, val]), (i, val)
            if (i, val) in stored:
                assert np.array_equal(pred.reshape(-1), stored[(i, val)]), (i, val)
            n_pred += 1
    assert n_vec == 10272 and n_pred == 9644 and len(stored) > 250 and [k for k in MR.REQUIRED if not cnt.get(k)] == []
    assert {(8, 4), (4, 8), (8, 8), (16, 8), (8, 16), (16, 16), (32, 8), (32, 32), (64, 64), (128, 128), (128, 4), (4, 128), (8, 128), (128, 8), (128, 64)} <= sizes
    assert {k[1] for k in keys} == {8, 10, 12}
    assert int((cost != 0).any(axis=2).sum()) == n_pred


def test_host_candidate_equals_the_fixture(golden):
    """vvhip_mmvd_candidate on every recorded candidate: the reference's stored and clipped vectors and the lists it names"""
    import mmvd_golden_gen as GG
    from vvenc_amd.lib import load_library
    lib = load_library()
    z, keys = golden
    cases, cands = z["cases"], z["cands"]
    n = 0
    for i in range(len(cases)):
        c, (pw, ph, ctu, df), _ = GG.case_of(cases[i], keys)
        c = dict(c, mask=tuple(0xFFFFFFFF if c["bases"][b]["ref"] != (-1, -1) else 0 for b in (0, 1)))
        rec = MC.as_list([c], 0, 0)
        for val in MR.vals_of(c["mask"]):
            rc, o = host_candidate(lib, rec, val, pw, ph, ctu, df)
            g = [int(v) for v in cands[i, val >> 5, val & 31]]
            assert rc == 0 and [tuple(int(v) for v in o["stored_mv"][l]) for l in (0, 1)] == [(g[0], g[1]), (g[2], g[3])], (i, val)
            assert all(tuple(int(v) for v in o["mv"][l]) == (g[9 + 2 * l], g[10 + 2 * l]) for l in (0, 1) if g[4 + l] >= 0), (i, val)
            assert all(o["ref_plane"][l] < 0 for l in (0, 1) if g[4 + l] < 0), (i, val)
            n += 1
    assert n == 10272


@pytest.fixture(scope="module")
def shim_driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("mmvd_shim") / "mmvd_shim_driver")
    subprocess.check_call(["g++", "-std=c++14", "-O1", "-Wall", "-o", exe, os.path.join(ROOT, "tests", "cpp", "mmvd_shim_driver.cpp"), "-L" + os.path.join(ROOT, "vvenc_amd"),
                           "-lvvenc_hip_shim", "-lvvenc_hip", "-Wl,-rpath," + os.path.join(ROOT, "vvenc_amd"), "-Wl,-rpath,/opt/rocm/lib"])
    return exe


def run_walk(exe, tmp_path, recs):
    import mmvd_walk_ref as WR
    with open(tmp_path / "in.bin", "wb") as f:
        f.write(np.int32(len(recs)).tobytes() + np.ascontiguousarray(recs, WR.WALK_IN).tobytes())
    subprocess.check_call([exe, "--walk", str(tmp_path / "in.bin"), str(tmp_path / "out.bin")])
    return np.fromfile(tmp_path / "out.bin", WR.WALK_OUT)


def test_walk_equals_the_restatement_and_the_traces(shim_driver, tmp_path, golden):
    """vvhip::MergeMmvdOps::walk (host arithmetic, no device) on cost arrays with ties, for m_MMVD 1 .. 4: the candidates it visits, in order, and the three running values
    equal the plain Python restatement of addMmvdCandsToPruningList / xCheckMMVDCand and the traces recorded from EncCu::xCheckMMVDCand itself"""
    import mmvd_walk_ref as WR
    z = golden[0]
    recs = WR.walk_cases()
    assert recs.tobytes() == z["walk_in"].tobytes()
    got = run_walk(shim_driver, tmp_path, recs)
    assert got.tobytes() == z["walk_out"].tobytes()
    seen, lengths = set(), set()
    for r, o in zip(recs, got):
        tested, bco, bcm, bd = WR.walk(r["dist"], r["bits_cost"], r["list_cost"][:r["n_list"]], int(r["mmvd"]), int(r["dis_num"]), int(r["num_valid"]), int(r["mrg_cnd0"]),
                                       int(r["mrg_cnd1"]), int(r["max_tracking"]), int(r["skip"]))
        assert tested == o["tested"][:o["count"]].tolist() and (bco, bcm, bd) == (float(o["best_cost_offset"]), float(o["best_cost_merge"]), int(o["best_dir"]))
        assert (o["tested"][o["count"]:] == 255).all()
        seen.add(int(r["mmvd"]))
        lengths.add((int(r["mmvd"]), len(tested)))
    # every m_MMVD; walks that test nothing ( m_MMVD 4, both best candidates beyond 1 ), that stop early, that keep one direction, and the full 64 of m_MMVD 1
    assert seen == {1, 2, 3, 4} and (4, 0) in lengths and (1, 64) in lengths and any(m == 2 and n == 2 * (4 + 7) for m, n in lengths) and any(m == 3 and 0 < n < 9 for m, n in lengths)


def test_bdof_candidates_equal_the_restatement(shim_driver, tmp_path):
    """vvhip::MergeMmvdOps::bdofCands: the candidates the reference's SATD stage predicts with BDOF ( EncCu.cpp:2225, InterPrediction.cpp:474-479 )"""
    import mmvd_walk_ref as WR
    rng = np.random.default_rng(9)
    rows = []
    for k in range(400):
        w, h = int(rng.choice((4, 8, 16, 32, 64))), int(rng.choice((4, 8, 16, 32)))
        if w + h < 12:
            continue
        row = [w, h, 8, 1 + (k % 7 == 0) * int(rng.integers(1, 4)), int(k % 11 != 0), int(k % 3 != 0)]
        for b in (0, 1):
            d = int(rng.integers(1, 4))
            poc = (8 - d, 8 + d) if rng.integers(0, 3) else (8 - d, 8 + int(rng.integers(-3, 4)))
            row += [int(rng.integers(0, 4) != 0), int(rng.integers(0, 4) != 0), poc[0], poc[1], int(rng.integers(0, 6) == 0), int(rng.integers(0, 6) == 0), int(rng.choice((2, 2, 2, 0, 4)))]
        rows.append(row)
    t = np.array(rows, np.int32)
    with open(tmp_path / "in.bin", "wb") as f:
        f.write(np.int32(len(t)).tobytes() + t.tobytes())
    subprocess.check_call([shim_driver, "--bdof", str(tmp_path / "in.bin"), str(tmp_path / "out.bin")])
    got = np.fromfile(tmp_path / "out.bin", np.uint64)
    want = [WR.bdof_cands(r[0], r[1], [dict(used=(r[6 + 7 * b], r[7 + 7 * b]), poc=(r[8 + 7 * b], r[9 + 7 * b]), lt=(r[10 + 7 * b], r[11 + 7 * b]), bcw=r[12 + 7 * b]) for b in (0, 1)],
                          r[2], r[3], bool(r[4]), bool(r[5])) for r in rows]
    assert [int(v) for v in got] == want
    assert {0, 0xFFF, 0xFFF << 32, 0xFFF | 0xFFF << 32} <= set(want)
