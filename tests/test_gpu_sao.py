"""GPU tier of the SAO entries: vvhip_sao_stats / vvhip_sao_offset through HotPath.sao_stats / HotPath.sao_offset, tolerance 0.

Expected values: the reference's own results recorded in tests/golden/sao.npz (replayed directly) and tests/sao_ref.py, the model pinned to that fixture by
tests/test_sao_cpu.py, on the lists of tests/sao_cases.py.  Every output is pre-filled with a sentinel: the statistics tensor has guard records behind the picture's,
the planes sit in storage whose pitch padding, leading samples and trailing rows must come back untouched, and every input is compared with what was uploaded."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import sao_cases as SC  # noqa: E402
import sao_ref as SR  # noqa: E402

SENT64 = -0x0123456789ABCDEF
SENT16 = -12345
GUARD = 2          # records behind the picture's
GUARD_ROWS = 2     # storage rows behind a plane's last


@pytest.fixture(scope="module")
def hp():
    from vvenc_amd.hotpath import HotPath
    return HotPath()


@pytest.fixture(scope="module")
def golden():
    return np.load(SR.GOLDEN)


@pytest.fixture(scope="module")
def model():
    """the model's records / planes per case, computed once and shared"""
    cache = {}

    def stats(k):
        if ("s", k) not in cache:
            _, pic, flags = SC.stats_cases()[k]
            cache[("s", k)] = np.stack([SR.stats_picture(pic.org[c], pic.src[c], pic.ctus[c][0], pic.ctus[c][1], pic.bit_depth, c == 0, flags) for c in range(3)], axis=1)
        return cache[("s", k)]

    def planes(k):
        if ("o", k) not in cache:
            _, pic, prm, clip = SC.offset_cases()[k]
            cache[("o", k)] = [SR.offset_picture(pic.src[c], prm[:, c], pic.ctus[c][0], pic.ctus[c][1], pic.bit_depth, clip[c]) for c in range(3)]
        return cache[("o", k)]
    return stats, planes


class Held:
    """a plane inside sentinel-filled storage: `base` samples in front, pitch = width rounded up to 8 + `extra`, GUARD_ROWS rows behind"""

    def __init__(self, hp, arr, layout, fill=None):
        import torch
        from vvenc_amd.hotpath import PlaneView
        base, extra = layout
        h, w = arr.shape
        self.stride, self.base, self.h, self.w = ((w + 7) // 8) * 8 + extra, base, h, w
        self.host = np.full(base + (h + GUARD_ROWS) * self.stride, SENT16, np.int16)
        self.inside = np.zeros(self.host.size, bool)
        for y in range(h):
            self.inside[base + y * self.stride:base + y * self.stride + w] = True
        if fill is None:
            self.host[self.inside] = arr.reshape(-1)
        self.dev = torch.from_numpy(self.host).to(hp.device)
        self.view = PlaneView(self.dev, base, self.stride, w, h)

    def read(self):
        """-> ( the plane, everything else ) as the device holds them now"""
        now = self.dev.cpu().numpy()
        return now[self.inside].reshape(self.h, self.w), now[~self.inside]

    def unchanged(self):
        return np.array_equal(self.dev.cpu().numpy(), self.host)


def run_stats(hp, pic, flags, layout=(0, 0), rows=None, out=None):
    import torch
    held = [(Held(hp, pic.org[c], layout), Held(hp, pic.src[c], layout)) for c in range(3)]
    if out is None:
        out = torch.full((pic.n_ctus + GUARD, 3, 5, 2, 32), SENT64, dtype=torch.int64, device=hp.device)
    hp.sao_stats([(o.view, s.view) for o, s in held], pic.ctu, pic.bit_depth, rows=rows, flags=flags, out=out)
    torch.cuda.synchronize()
    assert all(o.unchanged() and s.unchanged() for o, s in held), "an input plane was written"
    return out


@pytest.mark.parametrize("layout", SC.LAYOUTS)
def test_stats_equal_the_fixture_and_the_model(hp, golden, model, layout):
    for k, (name, pic, flags) in enumerate(SC.stats_cases()):
        got = run_stats(hp, pic, flags, layout).cpu().numpy()
        assert (got[pic.n_ctus:] == SENT64).all(), (name, "a record behind the picture was written")
        assert np.array_equal(got[:pic.n_ctus], golden["s%03d_rec" % k]), (name, "fixture")
        assert np.array_equal(got[:pic.n_ctus], model[0](k)), (name, "model")
        if flags is None:      # the picture's borders handed over explicitly are the same thing
            again = run_stats(hp, pic, SR.border_flags(*pic.grid), layout).cpu().numpy()
            assert np.array_equal(again, got), name


def test_stats_in_bands_equal_the_whole(hp, golden):
    import torch
    names = [n for n, _, _ in SC.stats_cases()]
    for name in ("geo72/borders", "geo264/borders", "geo8/borders", "grid3/only4"):
        k = names.index(name)
        _, pic, flags = SC.stats_cases()[k]
        gx, gy = pic.grid
        out = torch.full((pic.n_ctus + GUARD, 3, 5, 2, 32), SENT64, dtype=torch.int64, device=hp.device)
        for r in reversed(range(gy)):      # one-row bands, last first: each writes its own records only
            before = out.cpu().numpy().copy()
            run_stats(hp, pic, flags, SC.LAYOUTS[1], rows=(r, 1), out=out)
            now = out.cpu().numpy()
            mine = np.zeros(pic.n_ctus + GUARD, bool)
            mine[r * gx:(r + 1) * gx] = True
            assert np.array_equal(now[~mine], before[~mine]), (name, r, "a band wrote records of another")
        assert np.array_equal(out.cpu().numpy()[:pic.n_ctus], golden["s%03d_rec" % k]), name
        if gy >= 2:
            two = run_stats(hp, pic, flags, rows=(0, 2)).cpu().numpy()
            assert np.array_equal(two[:2 * gx], golden["s%03d_rec" % k][:2 * gx]) and (two[2 * gx:] == SENT64).all(), name


def test_stats_are_identical_from_run_to_run(hp):
    _, pic, flags = SC.stats_cases()[2]
    first = run_stats(hp, pic, flags).cpu().numpy()
    for _ in range(3):
        assert np.array_equal(run_stats(hp, pic, flags).cpu().numpy(), first)


def run_offset(hp, pic, prm, clip, layout=(0, 0), rows=None, n_planes=3):
    import torch
    src = [Held(hp, pic.src[c], layout) for c in range(n_planes)]
    dst = [Held(hp, pic.src[c], (layout[0] ^ 2, layout[1] + 8), fill=SENT16) for c in range(n_planes)]      # a layout of its own: source and destination pitches differ
    hp.sao_offset([(s.view, d.view) for s, d in zip(src, dst)], prm[:, :n_planes], pic.ctu, pic.bit_depth, rows=rows, clip=clip[:n_planes])
    torch.cuda.synchronize()
    assert all(s.unchanged() for s in src), "a source plane was written"
    got = []
    for d in dst:
        plane, rest = d.read()
        assert (rest == SENT16).all(), "a sample outside the destination plane was written"
        got.append(plane)
    return got


@pytest.mark.parametrize("layout", SC.LAYOUTS)
def test_offset_equals_the_fixture_and_the_model(hp, golden, model, layout):
    for k, (name, pic, prm, clip) in enumerate(SC.offset_cases()):
        if layout != SC.LAYOUTS[0] and name.startswith("grid3/") and k % 3:      # the single-bit sweep of the masks runs in full at the aligned layout, every third case elsewhere
            continue
        got = run_offset(hp, pic, prm, clip, layout)
        for c in range(3):
            assert np.array_equal(got[c], pic.src[c] + golden["o%03d_delta%d" % (k, c)]), (name, c, "fixture")
            assert np.array_equal(got[c], model[1](k)[c]), (name, c, "model")


def test_offset_in_bands_and_with_a_lower_clip_bound(hp):
    names = [n for n, _, _, _ in SC.offset_cases()]
    for name in ("geo72/mixed", "geo264/mixed", "geo8/mixed"):
        _, pic, prm, clip = SC.offset_cases()[names.index(name)]
        clip = [(70, 900)] * 3 if pic.bit_depth == 10 else clip      # a lower bound above 0: only the model can say (a ClpRng of the reference starts at 0)
        whole = [SR.offset_picture(pic.src[c], prm[:, c], pic.ctus[c][0], pic.ctus[c][1], pic.bit_depth, clip[c]) for c in range(3)]
        assert any((w == clip[c][0]).any() and (pic.src[c] < clip[c][0]).any() for c, w in enumerate(whole)) or pic.bit_depth != 10
        got = run_offset(hp, pic, prm, clip, SC.LAYOUTS[2])
        assert all(np.array_equal(got[c], whole[c]) for c in range(3)), name
        for r in range(pic.grid[1]):      # a band fills its own rows of the destination and leaves the others alone
            got = run_offset(hp, pic, prm, clip, SC.LAYOUTS[1], rows=(r, 1))
            for c in range(3):
                ch = pic.ctus[c][1]
                y0, y1 = r * ch, min((r + 1) * ch, pic.src[c].shape[0])
                assert np.array_equal(got[c][y0:y1], whole[c][y0:y1]), (name, r, c)
                assert (got[c][:y0] == SENT16).all() and (got[c][y1:] == SENT16).all(), (name, r, c, "rows of another band were written")
    # fewer planes than three
    _, pic, prm, clip = SC.offset_cases()[names.index("geo72/eo2")]
    got = run_offset(hp, pic, prm, clip, n_planes=1)
    assert np.array_equal(got[0], SR.offset_picture(pic.src[0], prm[:, 0], 32, 32, 10))


def test_stats_then_a_parameter_rule_then_offset_on_resident_planes(hp):
    """the second entry reads what a real caller hands it: device planes that stay where they are, parameters made from the first entry's records by a fixed rule
    (per CTU and plane the edge type with the largest sum of | diff |, offsets = clamped diff / count; a CTU without any diff is off)"""
    import torch
    from vvenc_amd.hotpath import SAO_PARAM_DTYPE
    pic = SC.pictures()["geo136"]
    org = [Held(hp, pic.org[c], SC.LAYOUTS[1]) for c in range(3)]
    src = [Held(hp, pic.src[c], SC.LAYOUTS[2]) for c in range(3)]
    dst = [Held(hp, pic.src[c], SC.LAYOUTS[0], fill=SENT16) for c in range(3)]
    rec = hp.sao_stats([(o.view, s.view) for o, s in zip(org, src)], pic.ctu, pic.bit_depth).cpu().numpy()
    assert np.array_equal(rec, np.stack([SR.stats_picture(pic.org[c], pic.src[c], pic.ctus[c][0], pic.ctus[c][1], pic.bit_depth, c == 0) for c in range(3)], axis=1))
    q = SR.max_offset_qval(pic.bit_depth)
    prm = np.zeros((pic.n_ctus, 3), SAO_PARAM_DTYPE)
    prm["avail"] = SR.border_avail(*pic.grid)[:, None]
    for i in range(pic.n_ctus):
        for c in range(3):
            weight = np.abs(rec[i, c, :4, 0, :5]).sum(axis=1)
            t = int(np.argmax(weight))
            prm[i, c]["type"] = t if weight[t] else -1
            prm[i, c]["offs"] = np.clip(rec[i, c, t, 0, :5] // np.maximum(rec[i, c, t, 1, :5], 1), -q, q)
    assert (prm["type"] >= 0).any() and (prm["offs"] != 0).any()
    hp.sao_offset([(s.view, d.view) for s, d in zip(src, dst)], prm, pic.ctu, pic.bit_depth)
    torch.cuda.synchronize()
    changed = 0
    for c in range(3):
        plane, rest = dst[c].read()
        want = SR.offset_picture(pic.src[c], prm[:, c], pic.ctus[c][0], pic.ctus[c][1], pic.bit_depth)
        assert np.array_equal(plane, want) and (rest == SENT16).all() and src[c].unchanged() and org[c].unchanged(), c
        changed += int((want != pic.src[c]).sum())
    assert changed > 0


def test_argument_rules(hp):
    import torch
    from vvenc_amd.hotpath import PlaneView, SAO_PARAM_DTYPE
    from vvenc_amd.lib import VVHipError
    pic = SC.pictures()["geo72"]
    org = [Held(hp, pic.org[c], (0, 0)) for c in range(3)]
    src = [Held(hp, pic.src[c], (0, 0)) for c in range(3)]
    dst = [Held(hp, pic.src[c], (0, 0), fill=SENT16) for c in range(3)]
    sp = [(o.view, s.view) for o, s in zip(org, src)]
    op = [(s.view, d.view) for s, d in zip(src, dst)]
    out = torch.full((pic.n_ctus, 3, 5, 2, 32), SENT64, dtype=torch.int64, device=hp.device)
    prm = np.zeros((pic.n_ctus, 3), SAO_PARAM_DTYPE)
    prm["avail"] = SR.border_avail(*pic.grid)[:, None]

    def refused(fn, *a, **kw):
        with pytest.raises(VVHipError):
            fn(*a, **kw)

    # planes whose CTU grids differ; CTU sizes outside 8..128; a band outside the picture
    refused(hp.sao_stats, sp, [(32, 32), (16, 16), (32, 16)], 10, out=out)
    refused(hp.sao_offset, op, prm, [(32, 32), (16, 16), (32, 16)], 10)
    refused(hp.sao_stats, sp[:1], [(4, 32)], 10, out=out)
    refused(hp.sao_stats, sp[:1], [(32, 256)], 10, out=out)
    refused(hp.sao_stats, sp, 32, 10, rows=(1, 2), out=out)
    refused(hp.sao_stats, sp, 32, 10, rows=(0, 0), out=out)
    refused(hp.sao_offset, op, prm, 32, 10, rows=(2, 1))
    refused(hp.sao_stats, sp, 32, 7, out=out)
    # a flag / an availability bit for a neighbour outside the picture: every CTU of the grid's rim, every bit its position rules out
    gx, gy = pic.grid
    base, avail = SR.border_flags(gx, gy), SR.border_avail(gx, gy)
    for i in range(pic.n_ctus):
        for f in SR.STAT_FLAGS:
            if not base[i] & f:
                bad = base.copy()
                bad[i] |= f
                refused(hp.sao_stats, sp, 32, 10, flags=bad, out=out)
        for f in SR.AVAIL_BITS:
            if not avail[i] & f:
                bad = prm.copy()
                bad[i, 1]["avail"] |= f
                bad[i, 1]["type"] = 2
                refused(hp.sao_offset, op, bad, 32, 10)
    # ... but an off CTU's mask is not looked at, and a band is judged by its own CTUs alone
    ok = prm.copy()
    ok["type"] = -1
    ok[0, 0]["avail"] = 255
    hp.sao_offset(op, ok, 32, 10)
    bad = base.copy()
    bad[0] = 63
    hp.sao_stats(sp, 32, 10, rows=(1, 1), flags=bad, out=out)
    # parameter records: type, band, rsv
    for field, v in (("type", 5), ("type", -2), ("band", 32), ("rsv", 1)):
        bad = prm.copy()
        bad[3, 2][field] = v
        refused(hp.sao_offset, op, bad, 32, 10)
    refused(hp.sao_offset, op, prm, 32, 10, clip=[(5, 4)] * 3)
    # a source that overlaps a destination: the same plane, a plane shifted by a row, another plane's destination
    refused(hp.sao_offset, [(src[0].view, src[0].view)], prm[:, :1], 32, 10)
    big = torch.zeros(80 * 50, dtype=torch.int16, device=hp.device)
    refused(hp.sao_offset, [(PlaneView(big, 0, 80, 72, 40), PlaneView(big, 80, 80, 72, 40))], prm[:, :1], 32, 10)
    refused(hp.sao_offset, [(src[0].view, dst[0].view), (src[1].view, dst[1].view), (dst[0].view, dst[2].view)], prm, [(32, 32), (16, 16), (32, 32)], 10)
    # a last CTU column of one sample
    refused(hp.sao_stats, [(PlaneView(big, 0, 80, 33, 40), PlaneView(big, 0, 80, 33, 40))], 32, 10, out=out)
    torch.cuda.synchronize()
    assert (out.cpu().numpy()[:gx] == SENT64).all(), "a refused call wrote records"
    assert all(s.unchanged() and o.unchanged() for s, o in zip(src, org))
    # interleaved rows of one allocation do not overlap as sets of samples, but their spans do: refused, the spans are what is compared
    refused(hp.sao_offset, [(PlaneView(big, 0, 160, 72, 20), PlaneView(big, 80, 160, 72, 20))], np.zeros((3, 1), SAO_PARAM_DTYPE), [(32, 32)], 10)
