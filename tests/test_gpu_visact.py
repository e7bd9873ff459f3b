"""GPU tier of the visual-activity entry: vvhip_visact through HotPath.visact / HotPath.visact_picture, tolerance 0.

Expected values: the reference's own results recorded in tests/golden/visact.npz (replayed directly) on the pictures and area lists of tests/visact_cases.py.  The planes
sit in storage with a leading offset and a pitch of its own per pointer; the records land in the middle of a canary-filled tensor that must come back untouched around them."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import visact_cases as VC  # noqa: E402
import visact_ref as VR  # noqa: E402

CANARY = -0x0123456789ABCDEF
GUARD = 16      # canary rows of four in front of and behind the records
E_ARG = "vvenc_hip error -1"


@pytest.fixture(scope="module")
def hp():
    from vvenc_amd.hotpath import HotPath
    return HotPath()


@pytest.fixture(scope="module")
def golden():
    return np.load(VR.GOLDEN)


def held(hp, arr, layout):
    import torch
    from vvenc_amd.hotpath import PlaneView
    base, extra = layout
    h, w = arr.shape
    stride = w + extra
    host = np.full(base + h * stride, -77, np.int16)
    for y in range(h):
        host[base + y * stride:base + y * stride + w] = arr[y]
    return PlaneView(torch.from_numpy(host).to(hp.device), base, stride, w, h)


_tables = {}


def table(hp, pic, layout=VC.LAYOUTS[0]):
    """the device plane table of a picture in a layout, uploaded once and shared (the entry never writes a plane)"""
    key = (pic.name, layout)
    if key not in _tables:
        rows = []
        for r, (cur, p1, p2) in enumerate(pic.rows):
            c = held(hp, cur, layout[0])
            rows.append((c, c if pic.same(r) else held(hp, p1, layout[1]), held(hp, p2, layout[2]), pic.bit_depth))
        _tables[key] = rows
    return _tables[key]


def run(hp, planes, areas, raw=False):
    """-> the records as uint64 [n][4]; the canary around them must be intact"""
    import torch
    n = len(areas)
    buf = torch.full((n + 2 * GUARD, 4), CANARY, dtype=torch.int64, device=hp.device)
    hp.visact(planes, areas, out=buf[GUARD:GUARD + n])
    torch.cuda.synchronize()
    got = buf.cpu().numpy()
    assert (got[:GUARD] == CANARY).all() and (got[GUARD + n:] == CANARY).all(), "something outside [n][4] was written"
    rec = got[GUARD:GUARD + n]
    assert n == 0 or not (rec == CANARY).any(), "a field of a record was not written"
    return rec.tobytes() if raw else rec.view(np.uint64)


@pytest.mark.parametrize("layout", VC.LAYOUTS)
def test_every_case_equals_the_fixture(hp, golden, layout):
    names = list(VC.cases())
    assert names == list(golden["cases"])
    for name in names:
        c = VC.cases()[name]
        got = run(hp, table(hp, c.picture, layout), c.areas)
        want = golden[name + "_rec"]
        assert np.array_equal(got, want), (name, layout, np.argwhere(got != want)[:6].tolist(), got[got != want][:6], want[got != want][:6])


def test_visact_picture_builds_the_reference_list(hp, golden):
    for name, ctu, high_res, order, chroma in (("p72_10_hd1", 32, False, 1, "420"), ("p72_8_ds2", 32, True, 2, "420"), ("p72x_10_ds1", 32, True, 1, "444"), ("p264_10_ds2", 128, True, 2, "420"),
                                               ("p264_10_hd0", 128, False, 0, "420")):
        c = VC.cases()[name]
        t = table(hp, c.picture)
        rec, areas = hp.visact_picture([r[0] for r in t], [r[1] for r in t] if order else None, [r[2] for r in t] if order == 2 else None, ctu, c.picture.bit_depth, high_res, order, chroma)
        assert areas.tobytes() == np.ascontiguousarray(c.areas).tobytes(), name
        assert np.array_equal(rec.cpu().numpy().view(np.uint64), golden[name + "_rec"]), name


def test_records_do_not_depend_on_the_order_or_the_rest_of_the_list(hp, golden):
    for name in ("mix10", "p264_10_ds1", "ext10"):
        c = VC.cases()[name]
        t, want = table(hp, c.picture, VC.LAYOUTS[1]), golden[name + "_rec"]
        perm = np.random.default_rng(5).permutation(len(c.areas))
        assert np.array_equal(run(hp, t, c.areas[perm]), want[perm]), (name, "shuffled")
        assert np.array_equal(run(hp, t, c.areas[::-1]), want[::-1]), (name, "reversed")
        for i in (0, len(c.areas) // 2, len(c.areas) - 1):
            assert np.array_equal(run(hp, t, c.areas[i:i + 1]), want[i:i + 1]), (name, "alone", i)
        twice = np.concatenate([c.areas, c.areas[:3]])
        assert np.array_equal(run(hp, t, twice), np.concatenate([want, want[:3]])), (name, "with duplicates")


def test_two_runs_give_identical_bytes(hp):
    for name in ("mix10", "ext12", "p264_10_hd2"):
        c = VC.cases()[name]
        t = table(hp, c.picture, VC.LAYOUTS[2])
        assert run(hp, t, c.areas, raw=True) == run(hp, t, c.areas, raw=True), name


def test_an_empty_list_succeeds_and_writes_nothing(hp):
    c = VC.cases()["one10"]
    assert len(run(hp, table(hp, c.picture), c.areas[:0])) == 0


def test_argument_errors_launch_nothing(hp):
    import ctypes as C
    import torch
    from vvenc_amd.hotpath import HotPath, VVHipError
    c = VC.cases()["one10"]
    (cur, p1, p2, bd), = table(hp, c.picture)      # a 12 x 11 plane
    buf = torch.full((8, 4), CANARY, dtype=torch.int64, device=hp.device)

    def refused(planes, areas, what):
        with pytest.raises(VVHipError) as e:
            hp.visact(planes, areas, out=buf)
        assert E_ARG in str(e.value) and "vvhip_visact" in str(e.value), (what, str(e.value))

    full, ok = [(cur, p1, p2, bd)], VR.area(0, 0, 2, 1, 1, 8, 8, (2, 2, 4, 4))
    good = run(hp, full, np.array([ok], VR.AREA_DTYPE))

    def bad(**kw):
        a = np.array([ok, ok], VR.AREA_DTYPE)      # the good area first: an error further down the list must keep it from being launched as well
        for k, v in kw.items():
            a[1][k] = v
        return a

    for what, a in (("plane index outside the table", bad(plane=1)), ("area right of the plane", bad(x=5)), ("area below the plane", bad(y=4)), ("negative x", bad(x=-1)),
                    ("negative y", bad(y=-1)), ("mean rectangle outside", bad(mx=9)), ("mean rectangle below", bad(my=8)), ("negative mean origin", bad(mx=-1)),
                    ("mean width without height", bad(mh=0)), ("HD narrower than 3", bad(w=2)), ("HD lower than 3", bad(h=2)), ("ds narrower than 6", bad(ds=1, w=4, h=8)),
                    ("ds lower than 6", bad(ds=1, w=8, h=4)), ("ds odd width", bad(ds=1, w=7, h=8)), ("ds odd height", bad(ds=1, w=8, h=7)), ("order 3", bad(order=3)),
                    ("ds 2", bad(ds=2)), ("reserved byte", bad(rsv0=1)), ("reserved word", bad(rsv1=1))):
        refused(full, a, what)
    refused([(cur, None, p2, bd)], bad(order=1), "order 1 without prev1")
    refused([(cur, None, None, bd)], bad(order=2), "order 2 without prev1")
    refused([(cur, p1, None, bd)], bad(), "order 2 without prev2")
    torch.cuda.synchronize()
    assert (buf.cpu().numpy() == CANARY).all(), "an argument error wrote records"
    # n < 0, through the C entry itself
    desc = (HotPath._VisActPlane * 1)(HotPath._VisActPlane(cur.buf_ptr, p1.buf_ptr, p2.buf_ptr, cur.stride, p1.stride, p2.stride, cur.width, cur.height, bd))
    one = np.array([ok], VR.AREA_DTYPE)
    assert hp.L.vvhip_visact(hp.ctx, desc, 1, one.ctypes.data_as(C.c_void_p), -1, C.c_void_p(buf.data_ptr())) == -1
    assert b"vvhip_visact" in hp.L.vvhip_last_error(hp.ctx)
    torch.cuda.synchronize()
    assert (buf.cpu().numpy() == CANARY).all()
    # orders the table can serve still pass with the previous originals absent, and the entry works after the refusals
    assert np.array_equal(run(hp, [(cur, p1, None, bd)], np.array([VR.area(0, 0, 1, 1, 1, 8, 8, (2, 2, 4, 4))], VR.AREA_DTYPE))[:, [0, 2, 3]], good[:, [0, 2, 3]])
    assert np.array_equal(run(hp, full, np.array([ok], VR.AREA_DTYPE)), good)
