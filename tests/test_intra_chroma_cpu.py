"""CPU tier of the intra chroma mode pre-selection: the numpy model (tests/intra_chroma_ref.py) against the reference's own results recorded in
tests/golden/intra_chroma.npz (tolerance 0), the coverage the fixture must have, the item record against the header, and the shim's selection helper against a plain Python
restatement of the reference's sort."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import intra_chroma_cases as CC  # noqa: E402
import intra_chroma_extremes as CX  # noqa: E402
import intra_chroma_ref as CR  # noqa: E402


@pytest.fixture(scope="module")
def golden():
    return CC.load_golden()


@pytest.fixture(scope="module")
def model(golden):
    """the model on every golden case, once: { name: ( costs, params, predictions ) } and the branch counters"""
    cnt, out = {}, {}
    for name, (c, _, _, _) in golden.items():
        out[name] = CC.expected(c, cnt)
    return out, cnt


def test_fixture_is_the_case_list(golden):
    cases = CC.cases()
    assert list(golden) == list(cases)
    for name, c in cases.items():
        g = golden[name][0]
        assert (g.w, g.h, g.bit_depth, g.flags, g.n_ar, g.n_lb, g.cand, g.mode_mask, g.pred_mask) == (c.w, c.h, c.bit_depth, c.flags, c.n_ar, c.n_lb, c.cand, c.mode_mask, c.pred_mask), name
        assert np.array_equal(g.luma, c.luma) and np.array_equal(g.lines, c.lines) and np.array_equal(g.org, c.org), name


def test_model_equals_golden(golden, model):
    for name, (c, cost, prm, pred) in golden.items():
        mc, mp, mpred = model[0][name]
        assert np.array_equal(mc, cost), (name, np.argwhere(mc != cost).reshape(-1).tolist())
        assert np.array_equal(mp, prm), (name, mp.tolist(), prm.tolist())
        assert np.array_equal(mpred, pred), name


def test_fixture_covers_every_branch(golden, model):
    cnt = model[1]
    missing = [k for k in CC.REQUIRED if not cnt.get(k)]
    assert not missing, missing
    cases = [g[0] for g in golden.values()]
    assert {(c.w, c.h) for c in cases} == set(CC.SHAPES) and {(4, 4), (4, 32), (32, 4)} <= {(c.w, c.h) for c in cases}
    assert {c.bit_depth for c in cases} == {8, 10, 12}
    assert {c.flags & 3 for c in cases} == {0, 1, 2, 3}
    # the parameters of the fixture reach both +-15 (the iShift < 1 clamp), a == 0 and the default b
    a = np.concatenate([g[2][:, :, 0].reshape(-1) for g in golden.values()])
    assert a.min() == -15 and a.max() == 15
    assert any((g[2][4:7, :, 1] == 1 << (g[0].bit_depth - 1)).any() and not g[0].flags & 3 for g in golden.values())
    assert os.path.getsize(CR.GOLDEN) < 1024 * 1024


def test_record_layout_equals_the_header():
    """vvhip_intra_chroma_item as include/vvenc_hip.h declares it: the same fields at the same offsets in the model's and in HotPath's dtype"""
    from vvenc_amd.hotpath import INTRA_CHROMA_ITEM_DTYPE
    txt = open(os.path.join(ROOT, "include", "vvenc_hip.h")).read()
    body = re.search(r"typedef struct\s*\{([^}]*)\}\s*vvhip_intra_chroma_item;", txt).group(1)
    sizes, at, fields = {"uint8_t": 1, "int32_t": 4, "uint32_t": 4}, 0, []
    for line in body.splitlines():
        m = re.match(r"\s*(uint8_t|int32_t|uint32_t)\s+([^;]+);", line)
        if not m:
            continue
        sz = sizes[m.group(1)]
        for decl in m.group(2).split(","):
            d = re.match(r"\s*(\w+)(?:\[(\d+)\])?\s*$", decl)
            n = int(d.group(2) or 1)
            at = (at + sz - 1) // sz * sz
            fields.append((d.group(1), at, sz, n))
            at += sz * n
    assert at == 64 and "sizeof( vvhip_intra_chroma_item ) == 64" in txt
    for dt in (CR.ITEM_DTYPE, INTRA_CHROMA_ITEM_DTYPE):
        assert dt.itemsize == 64 and list(dt.names) == [f[0] for f in fields]
        for name, off, sz, n in fields:
            sub, o = dt.fields[name][0], dt.fields[name][1]
            assert o == off and sub.base.itemsize == sz and int(np.prod(sub.shape, dtype=int)) == n, name
    assert (CR.F_ABOVE, CR.F_LEFT, CR.F_FIRST_ROW, CR.F_VER_COLLOCATED) == tuple(int(re.search(r"#define %s\s+(\d+)" % k, txt).group(1)) for k in
                                                                                ("VVHIP_ICH_ABOVE", "VVHIP_ICH_LEFT", "VVHIP_ICH_FIRST_ROW", "VVHIP_ICH_VER_COLLOCATED"))


def test_extremes_list_reaches_the_limits():
    """the list of tests/intra_chroma_extremes.py (run on the device by tests/test_gpu_intra_chroma_extremes.py) holds the operand limits it is named after"""
    cl, cnt = CX.cases(), {}
    want = [CC.expected(c, cnt) for c in cl]
    prm = np.concatenate([w[1][4:7].reshape(-1, 3) for w in want])
    a, b, sh = prm[:, 0], prm[:, 1], prm[:, 2]
    assert a.min() == -15 and a.max() == 15 and sh[np.abs(a) == 15].min() == 1
    assert b.min() < -30000 and b.max() > 30000 + CX.VMAX          # b far beyond the clip range on both sides
    assert cnt.get("diff_zero") and cnt.get("lm_clip_low") and cnt.get("lm_clip_high") and cnt.get("shift_clamp_positive") and cnt.get("shift_clamp_negative")
    # the largest diff: a template pair ( 0, 4095 ) — its parameters are those of diff = 4095, diffC = +-4095: a = +-8 at shift 3
    assert any((w[1][4] == (8, 0, 3)).all(axis=-1).any() for w in want) and any((w[1][4] == (-8, CX.VMAX, 3)).all(axis=-1).any() for w in want)
    assert {(c.w, c.h) for c in cl} == set(CX.SHAPES) and all(c.bit_depth == 12 for c in cl)


def reference_sort(costs, cand, reduce_full_rd):
    """IntraSearch.cpp:847-862, restated plainly"""
    modes, c = list(cand), list(costs)
    for i in range(8):
        for j in range(i + 1, 8):
            if c[j] < c[i]:
                modes[i], modes[j] = modes[j], modes[i]
                c[i], c[j] = c[j], c[i]
    disabled = np.zeros(70, bool)
    for i in range(8 >> (1 if reduce_full_rd else 2)):
        disabled[modes[7 - i]] = True
    return modes, disabled


def test_selection_helper_order(tmp_path):
    """vvhip::IntraChromaOps::select (host arithmetic, no device) on tied costs, zero costs of skipped slots and plain random costs"""
    exe = str(tmp_path / "intra_chroma_shim_driver")
    subprocess.check_call(["g++", "-std=c++14", "-O1", "-Wall", "-o", exe, os.path.join(ROOT, "tests", "cpp", "intra_chroma_shim_driver.cpp"), "-L" + os.path.join(ROOT, "vvenc_amd"),
                           "-lvvenc_hip_shim", "-lvvenc_hip", "-Wl,-rpath," + os.path.join(ROOT, "vvenc_amd"), "-Wl,-rpath,/opt/rocm/lib"])
    rng = np.random.default_rng(9)
    entries = []
    for k in range(60):
        cand = CC.cand_list(int(rng.integers(0, 67)))
        if k % 3 == 0:
            costs = rng.integers(0, 4, 8) * 100          # many ties
        elif k % 3 == 1:
            costs = rng.integers(1, 1 << 20, 8)
            costs[[0, 4, 7]] = 0                          # the slots IntraSearch.cpp:810 skips keep cost 0
        else:
            costs = rng.integers(0, 1 << 31, 8)
        entries.append((costs.astype(np.uint32), np.array(cand, np.uint8), k % 2))
    entries.append((np.zeros(8, np.uint32), np.array(CC.cand_list(50), np.uint8), 0))
    entries.append((np.full(8, 0xffffffff, np.uint32), np.array(CC.cand_list(1), np.uint8), 1))
    with open(tmp_path / "in.bin", "wb") as f:
        f.write(np.array([len(entries)], np.int32).tobytes() + b"".join(c.tobytes() + m.tobytes() + bytes([r]) for c, m, r in entries))
    subprocess.check_call([exe, "--select", str(tmp_path / "in.bin"), str(tmp_path / "out.bin")])
    got = np.fromfile(tmp_path / "out.bin", np.uint8).reshape(len(entries), 78)
    for (costs, cand, red), g in zip(entries, got):
        modes, disabled = reference_sort([int(v) for v in costs], [int(m) for m in cand], red)
        assert g[:8].tolist() == modes and np.array_equal(g[8:].astype(bool), disabled), (costs.tolist(), cand.tolist(), red)
        assert (modes, set(np.flatnonzero(disabled).tolist())) == CR.select(costs, cand, 0xff, red)
