"""GPU tier of the deblocking entry: vvhip_deblock through HotPath.deblock, tolerance 0.

Expected values: the reference's own results recorded in tests/golden/deblock.npz (replayed directly) and tests/deblock_ref.py, the model pinned to that fixture by
tests/test_deblock_cpu.py, on the pictures and maps of tests/deblock_cases.py.  The planes sit in storage whose pitch padding, leading samples and trailing rows are a
sentinel that must come back untouched."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import deblock_cases as DC  # noqa: E402
import deblock_ref as DR  # noqa: E402

SENT16 = -12345
GUARD_ROWS = 2


@pytest.fixture(scope="module")
def hp():
    from vvenc_amd.hotpath import HotPath
    return HotPath()


@pytest.fixture(scope="module")
def golden():
    return np.load(DR.GOLDEN)


@pytest.fixture(scope="module")
def model():
    """name -> the model's planes after both passes, computed once and shared"""
    return {n: DR.deblock(c.planes, c.lfp_ver, c.lfp_hor, c.ctu, c.bit_depth, c.clip, c.beta_offsets, c.tc_offsets) for n, c in DC.cases().items()}


class Held:
    """a plane inside sentinel-filled storage: `base` samples in front, pitch = width rounded up to 8 + `extra`, GUARD_ROWS rows behind"""

    def __init__(self, hp, arr, layout):
        import torch
        from vvenc_amd.hotpath import PlaneView
        base, extra = layout
        h, w = arr.shape
        self.stride, self.h, self.w = ((w + 7) // 8) * 8 + extra, h, w
        self.host = np.full(base + (h + GUARD_ROWS) * self.stride, SENT16, np.int16)
        self.inside = np.zeros(self.host.size, bool)
        for y in range(h):
            self.inside[base + y * self.stride:base + y * self.stride + w] = True
        self.host[self.inside] = arr.reshape(-1)
        self.dev = torch.from_numpy(self.host).to(hp.device)
        self.view = PlaneView(self.dev, base, self.stride, w, h)

    def read(self):
        """-> the plane as the device holds it now; everything else must still be the sentinel"""
        now = self.dev.cpu().numpy()
        assert (now[~self.inside] == SENT16).all(), "a sample outside the plane was written"
        return now[self.inside].reshape(self.h, self.w)

    def unchanged(self):
        return np.array_equal(self.dev.cpu().numpy(), self.host)


def hold(hp, c, layout=(0, 0), planes=None):
    return [Held(hp, p, layout) for p in (c.planes if planes is None else planes)]


def run(hp, c, held, **kw):
    import torch
    hp.deblock([h.view for h in held], c.lfp_ver, c.lfp_hor, c.ctu, c.bit_depth, clip=c.clip[:len(held)], beta_offsets=c.beta_offsets, tc_offsets=c.tc_offsets, **kw)
    torch.cuda.synchronize()
    return [h.read() for h in held]


@pytest.mark.parametrize("layout", DC.LAYOUTS)
def test_every_case_equals_the_fixture_and_the_model(hp, golden, model, layout):
    for name, c in DC.cases().items():
        got = run(hp, c, hold(hp, c, layout))
        for k, p in enumerate(c.planes):
            assert np.array_equal(got[k], p + golden["%s_d%d" % (name, k)]), (name, k, "fixture", np.argwhere(got[k] != p + golden["%s_d%d" % (name, k)])[:6].tolist())
            assert np.array_equal(got[k], model[name][k]), (name, k, "model")


def test_the_vertical_pass_alone_equals_the_recorded_intermediate(hp, golden):
    for name, c in DC.cases().items():
        got = run(hp, c, hold(hp, c, DC.LAYOUTS[1]), dirs=DR.VER)
        assert all(np.array_equal(got[k], p + golden["%s_v%d" % (name, k)]) for k, p in enumerate(c.planes)), name
        # and the horizontal pass on top of it gives the whole
        held = hold(hp, c, DC.LAYOUTS[2], planes=got)
        both = run(hp, c, held, dirs=DR.HOR)
        assert all(np.array_equal(both[k], p + golden["%s_d%d" % (name, k)]) for k, p in enumerate(c.planes)), name


def test_every_partition_into_bands_gives_the_whole(hp, golden, model):
    for name in ("g136", "g64", "g72", "mono"):
        c = DC.cases()[name]
        assert c.ctu_rows >= 2
        held = hold(hp, c, DC.LAYOUTS[1])
        for r in range(c.ctu_rows):      # one-row bands top to bottom, both directions each
            got = run(hp, c, held, rows=(r, 1))
        assert all(np.array_equal(g, w) for g, w in zip(got, model[name])), (name, "top to bottom")
        held = hold(hp, c, DC.LAYOUTS[2])
        for r in reversed(range(c.ctu_rows)):      # every vertical band, last first, then every horizontal band, last first
            run(hp, c, held, rows=(r, 1), dirs=DR.VER)
        for r in reversed(range(c.ctu_rows)):
            got = run(hp, c, held, rows=(r, 1), dirs=DR.HOR)
        assert all(np.array_equal(g, w) for g, w in zip(got, model[name])), (name, "all VER, then all HOR, in reverse")
        assert all(np.array_equal(g, p + golden["%s_d%d" % (name, k)]) for k, (g, p) in enumerate(zip(got, c.planes))), name


def test_a_band_writes_its_rows_and_three_luma_one_chroma_row_above(hp):
    for name in ("g136", "g64"):
        c = DC.cases()[name]
        r = c.ctu_rows - 1
        got = run(hp, c, hold(hp, c), rows=(r, 1))
        want = DR.deblock(c.planes, c.lfp_ver, c.lfp_hor, c.ctu, c.bit_depth, c.clip, c.beta_offsets, c.tc_offsets, rows=(r, 1))
        above = 0
        for k, p in enumerate(c.planes):
            y0 = (r * c.ctu) >> (k > 0)
            reach = 1 if k else 3
            assert np.array_equal(got[k], want[k]), (name, k)
            assert np.array_equal(got[k][:y0 - reach], p[:y0 - reach]), (name, k, "rows further above the band were written")
            above += int((got[k][y0 - reach:y0] != p[y0 - reach:y0]).sum())
            assert (got[k][y0:] != p[y0:]).any(), (name, k)
        assert above > 0, (name, "the band's top CTU boundary was not filtered")
        # the vertical pass of a band stays inside the band's rows
        got = run(hp, c, hold(hp, c), rows=(r, 1), dirs=DR.VER)
        want = DR.deblock(c.planes, c.lfp_ver, c.lfp_hor, c.ctu, c.bit_depth, c.clip, c.beta_offsets, c.tc_offsets, rows=(r, 1), dirs=DR.VER)
        for k, p in enumerate(c.planes):
            y0 = (r * c.ctu) >> (k > 0)
            assert np.array_equal(got[k], want[k]) and np.array_equal(got[k][:y0], p[:y0]), (name, k)
        assert (got[0] != c.planes[0]).any(), name


def test_results_are_identical_from_run_to_run(hp):
    c = DC.cases()["g264"]
    first = run(hp, c, hold(hp, c))
    for _ in range(3):
        again = run(hp, c, hold(hp, c))
        assert all(np.array_equal(a, b) for a, b in zip(again, first))


def test_luma_only(hp, golden):
    for name in ("g72", "narrow"):
        c = DC.cases()[name]
        held = hold(hp, c, DC.LAYOUTS[1])
        got = run(hp, c, held[:1])
        assert np.array_equal(got[0], c.planes[0] + golden[name + "_d0"]) and held[1].unchanged() and held[2].unchanged(), name


def test_argument_rules(hp):
    import torch
    from vvenc_amd.hotpath import PlaneView
    from vvenc_amd.lib import VVHipError
    c = DC.cases()["g72"]
    held = hold(hp, c)
    views = [h.view for h in held]
    ver, hor = c.lfp_ver, c.lfp_hor

    def refused(planes=views, v=ver, h=hor, ctu=32, bd=10, **kw):
        with pytest.raises(VVHipError):
            hp.deblock(planes, v, h, ctu, bd, **kw)

    refused(planes=views[:2])                                               # 2 planes
    refused(planes=[views[0], views[1], PlaneView(held[2].dev, 0, held[2].stride, 36, 16)])      # a chroma plane that is not half the luma plane
    refused(planes=[views[0], PlaneView(held[1].dev, 0, held[1].stride, 32, 20), views[2]])
    refused(planes=[PlaneView(held[0].dev, 0, held[0].stride, 68, 40)], v=ver[:, :17], h=hor[:, :17])      # luma width / height no multiple of 8
    refused(planes=[PlaneView(held[0].dev, 0, held[0].stride, 72, 36)], v=ver[:9], h=hor[:9])
    for bd in (7, 13):
        refused(bd=bd)
    for ctu in (8, 48, 256):
        refused(ctu=ctu)
    for rows in ((2, 1), (1, 2), (-1, 1), (0, 0)):
        refused(rows=rows)
    for dirs in (0, 4):
        refused(dirs=dirs)
    refused(v=ver[:, :-1], h=hor[:, :-1])                                   # fewer records per map row than width / 4
    refused(clip=[(0, 1023), (5, 4), (0, 1023)])

    def with_record(which, y, x, **fields):
        m = (ver if which == "v" else hor).copy()
        for f, val in fields.items():
            m[y, x][f] = val
        return {which: m}

    for bs in (3, 3 << 2, 3 << 4):                                          # a bs field of 3
        refused(**with_record("v", 2, 3, bs=bs))
        refused(**with_record("h", 2, 3, bs=bs))
    for ln in (0x43, 0x36, 0x64, 0x14):                                     # a P or Q length of 4 or 6 where the luma bs is non-zero
        refused(**with_record("v", 1, 2, bs=1, side_max_filt_length=ln))
    for fl in (4, 8, 16, 64, 128):                                          # flag bits other than 0, 1, 5
        refused(**with_record("h", 3, 1, flags=fl))
    for bs in (1, 2 << 2, 1 << 4):                                          # an edge that would read outside the picture
        refused(**with_record("v", 4, 0, bs=bs, side_max_filt_length=0x11))
        refused(**with_record("h", 0, 5, bs=bs, side_max_filt_length=0x11))
    torch.cuda.synchronize()
    assert all(h.unchanged() for h in held), "a refused call wrote samples"
    # what is not refused: a length of 4 where the luma bs is 0; bs in row 0 of the VERTICAL map and column 0 of the HORIZONTAL one; bits 6-7 of bs; a bad record outside the band
    ok_v = with_record("v", 1, 2, bs=2 << 2, side_max_filt_length=0x44)["v"]
    ok_v[0, 3]["bs"], ok_v[0, 3]["side_max_filt_length"] = 1 | 0xc0, 0x11
    ok_h = with_record("h", 3, 0, bs=1, side_max_filt_length=0x11)["h"]
    scratch = hold(hp, c)
    hp.deblock([h.view for h in scratch], ok_v, ok_h, 32, 10)
    bad_top = with_record("v", 0, 3, bs=3)["v"]
    hp.deblock([h.view for h in scratch], bad_top, hor, 32, 10, rows=(1, 1))
    torch.cuda.synchronize()


def test_deblock_then_sao_on_resident_planes(hp):
    """the chain a caller runs: the unfiltered reconstruction is uploaded once; deblock filters it in place, sao_stats reads it where it lies, parameters are made from
    the records by a fixed rule (per CTU and plane the edge type with the largest sum of | diff |, offsets = clamped diff / count; a CTU without any diff is off), sao_offset
    filters it — compared to the models end to end"""
    import torch
    import sao_ref as SR
    from vvenc_amd.hotpath import SAO_PARAM_DTYPE
    c = DC.cases()["g136"]
    rng = np.random.default_rng(77)
    mx = (1 << c.bit_depth) - 1
    orgs = [np.clip(p.astype(np.int32) + rng.integers(-4, 5, p.shape), 0, mx).astype(np.int16) for p in c.planes]
    rec = hold(hp, c, DC.LAYOUTS[2])
    org = hold(hp, c, DC.LAYOUTS[1], planes=orgs)
    dst = hold(hp, c, DC.LAYOUTS[0], planes=[np.full_like(p, SENT16) for p in c.planes])
    hp.deblock([h.view for h in rec], c.lfp_ver, c.lfp_hor, c.ctu, c.bit_depth, clip=c.clip, beta_offsets=c.beta_offsets, tc_offsets=c.tc_offsets)
    stats = hp.sao_stats([(o.view, s.view) for o, s in zip(org, rec)], c.ctu, c.bit_depth).cpu().numpy()
    dbk = DR.deblock(c.planes, c.lfp_ver, c.lfp_hor, c.ctu, c.bit_depth, c.clip, c.beta_offsets, c.tc_offsets)
    ctus = [(c.ctu, c.ctu), (c.ctu // 2, c.ctu // 2), (c.ctu // 2, c.ctu // 2)]
    assert np.array_equal(stats, np.stack([SR.stats_picture(orgs[k], dbk[k], ctus[k][0], ctus[k][1], c.bit_depth, k == 0) for k in range(3)], axis=1))
    gx, gy = SR.grid(c.width, c.height, c.ctu, c.ctu)
    q = SR.max_offset_qval(c.bit_depth)
    prm = np.zeros((gx * gy, 3), SAO_PARAM_DTYPE)
    prm["avail"] = SR.border_avail(gx, gy)[:, None]
    for i in range(gx * gy):
        for k in range(3):
            weight = np.abs(stats[i, k, :4, 0, :5]).sum(axis=1)
            t = int(np.argmax(weight))
            prm[i, k]["type"] = t if weight[t] else -1
            prm[i, k]["offs"] = np.clip(stats[i, k, t, 0, :5] // np.maximum(stats[i, k, t, 1, :5], 1), -q, q)
    assert (prm["type"] >= 0).any() and (prm["offs"] != 0).any()
    hp.sao_offset([(s.view, d.view) for s, d in zip(rec, dst)], prm, c.ctu, c.bit_depth)
    torch.cuda.synchronize()
    changed = 0
    for k in range(3):
        want = SR.offset_picture(dbk[k], prm[:, k], ctus[k][0], ctus[k][1], c.bit_depth)
        assert np.array_equal(dst[k].read(), want) and np.array_equal(rec[k].read(), dbk[k]) and org[k].unchanged(), k
        changed += int((want != dbk[k]).sum())
    assert changed > 0
