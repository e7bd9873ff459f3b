"""GPU tier of the context's host-list slots (common.h: HostList): the paths of the cached schedules and of the per-call arrays that the entries' own tests do not reach —
a cached list run again on another stream, a per-call array uploaded again while the launch that reads it may still run, a cached list inside a launch graph.  Tolerance 0.

The lists come from the families' own case builders (tests/blend_cases.py, affine_cases.py, ict_cases.py, sbt_cases.py, intra_cases.py, visact_cases.py) and are checked against
the models the families' own tests use; they are the smallest that still give more than one size class and more than one wave unit, so the sorted schedule differs from list order."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import affine_cases as AC  # noqa: E402
import affine_ref as AR  # noqa: E402
import blend_cases as BLC  # noqa: E402
import ict_cases as IC  # noqa: E402
import intra_cases as INC  # noqa: E402
import sbt_cases as SBC  # noqa: E402
import visact_cases as VC  # noqa: E402
import visact_ref as VR  # noqa: E402

SENTINEL = -7
SENT64 = -0x0123456789ABCDEF
SENT8 = 0x5A


@pytest.fixture(scope="module")
def hp():
    from vvenc_amd.hotpath import HotPath
    return HotPath()


def dev16(hp, a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, np.int16)).to(hp.device)


# ---- one entry per cached family: two lists A and B, the entry call into given outputs, the family's model ----
class PredFamily:
    """vvhip_pred_inter_batch: uni- and bi-predicted luma blocks and bi-predicted chroma blocks of four sizes"""

    def __init__(self, hp, oracle):
        self.hp, self.oracle = hp, oracle
        self.pl, _ = BLC.planes(10, 110)
        self.dev = [hp.plane(a, 0) for a in self.pl]
        self.A = self.make(501, ((8, 8), (16, 8), (32, 16), (16, 16)))
        self.B = self.make(502, ((16, 16), (8, 16), (64, 16), (8, 8)))

    def make(self, seed, sizes):
        b = BLC.Builder(self.pl, seed)
        f = lambda n: (int(b.rng.integers(0, n)), int(b.rng.integers(0, n)))
        for (w, h) in sizes:
            b.add(w, h, 0, 0, (f(16), f(16)), (0, 1))
            b.add(w, h, 0, 0, (f(16), f(16)), (1, -1))
            b.add(w // 2, h // 2, 1, 0, (f(32), f(32)), (2, 3))
        items, ext, blend, pos = b.done()
        items["dst_off"], total = BLC.compact_offsets(items)
        return items, ext, blend, pos, total

    def outputs(self, L):
        return [(L[4], "int16", SENTINEL)]

    def call(self, L, outs):
        self.hp.pred_inter_batch(self.dev, L[0], outs[0], 0, 10)

    def check(self, L, got, what):
        items, ext, blend, pos, _ = L
        for i, it in enumerate(items):
            w, h, o = int(it["width"]), int(it["height"]), int(it["dst_off"])
            e = BLC.expected(self.oracle, self.pl, pos[i], it, ext[i], blend[i], 10)
            assert np.array_equal(got[0][o:o + w * h].reshape(h, w), e), (what, i, it)


class AffineFamily:
    """vvhip_pred_affine_batch: the luma and the chroma block of CUs of four sizes in a 64 x 48 picture, CTU 32"""

    def __init__(self, hp, oracle):
        self.hp, self.oracle = hp, oracle
        self.world = AC.World(10, 32, seed=503, pic_w=64, pic_h=48)
        self.dev = [hp.plane(a, 0) for a in self.world.np]
        self.A = self.make(504, ((8, 8), (16, 16), (32, 16), (16, 8), (8, 32), (16, 16)))
        self.B = self.make(505, ((16, 8), (8, 8), (32, 32), (8, 16), (16, 16), (64, 16)))

    def make(self, seed, sizes):
        rng = np.random.default_rng(seed)
        recs = []
        for k, (w, h) in enumerate(sizes):
            x, y = 8 * int(rng.integers(0, (64 - w) // 8 + 1)), 8 * int(rng.integers(0, (48 - h) // 8 + 1))
            recs += AC._cu(rng, w, h, x, y, k & 1, (k >> 1) % 3, k % 4, 32)
        items, pos = AC.finish(self.world, recs)
        items["dst_off"], total = AC.compact_offsets(items)
        return items, pos, total

    def outputs(self, L):
        return [(L[2], "int16", SENTINEL)]

    def call(self, L, outs):
        self.hp.pred_affine_batch(self.dev, L[0], outs[0], 0, 10, 64, 48, 32)

    def check(self, L, got, what):
        items, pos, _ = L
        for k, it in enumerate(items):
            c = int(it["chroma"])
            bw, bh, o = int(it["cu_w"]) >> c, int(it["cu_h"]) >> c, int(it["dst_off"])
            e = AR.expected_block(self.oracle, self.world.np, pos[k], it, 10, 64, 48, 32)
            assert np.array_equal(got[0][o:o + bw * bh].reshape(bh, bw), e), (what, k, it)


class IctFamily:
    """vvhip_ict_fwd_batch: Cb / Cr block pairs of eight sizes, then six small ones of which a wave holds several"""

    def __init__(self, hp, oracle):
        self.hp = hp
        specs = IC.mixed_specs(506, False)
        self.A, self.B = IC.compact(specs[0::3][:8] + specs[40:46]), IC.compact(specs[1::3][:8] + specs[46:52])
        self.resi = {id(L): dev16(hp, L.resi) for L in (self.A, self.B)}

    def outputs(self, L):
        return [(L.joint_total, "int16", SENTINEL), ((len(L.items), 2), "int64", SENT64)]

    def call(self, L, outs):
        self.hp.ict_fwd_batch(self.resi[id(L)], L.items, outs[0], outs[1])

    def check(self, L, got, what):
        ej, ed = IC.expected_fwd(L)
        for i, e in enumerate(ej):
            if e is not None:
                assert np.array_equal(L.joint(got[0], i), e), (what, "joint", i, L.items[i])
        assert np.array_equal(got[1], ed), (what, "dist")
        assert (got[0][~L.joint_mask()] == SENTINEL).all(), (what, "a sample outside the joint blocks was written")


class SbtFamily:
    """vvhip_sbt_parts_batch: a dozen CUs over several sizes and sets of allowed modes"""
    CW = SBC.WEIGHTS[2]

    def __init__(self, hp, oracle):
        self.hp = hp
        specs = SBC.mixed_specs(507)
        self.A, self.B = SBC.compact(specs[0:12]), SBC.compact(specs[12:24])
        self.resi = {id(L): dev16(hp, L.resi) for L in (self.A, self.B)}

    def outputs(self, L):
        n = len(L.items)
        return [((n, 3, 16), "int64", SENT64), ((n, 9), "int64", SENT64), ((n, 8), "uint8", SENT8)]

    def call(self, L, outs):
        self.hp.sbt_parts_batch(self.resi[id(L)], L.items, self.CW, outs[0], outs[1], outs[2])

    def check(self, L, got, what):
        ep, ee, eo = SBC.expected_parts(L, self.CW)
        assert np.array_equal(got[0].view(np.uint64), ep), (what, "part sums")
        assert np.array_equal(got[1].view(np.uint64), ee), (what, "estimates")
        assert np.array_equal(got[2], eo), (what, "order")


FAMILIES = {"pred_inter_batch": PredFamily, "pred_affine_batch": AffineFamily, "ict_fwd_batch": IctFamily, "sbt_parts_batch": SbtFamily}


def make_outputs(hp, spec):
    import torch
    return [torch.empty(shape, dtype=getattr(torch, dt), device=hp.device) for (shape, dt, _) in spec]


def run(hp, fam, L, outs=None):
    """the entry on the context's current stream into sentinel-filled outputs -> ( results as numpy, the output tensors ).  The fills run on torch's stream and the context may
    be on its own, so everything torch queued is waited for in front of the call, and the context's stream behind it"""
    import torch
    spec = fam.outputs(L)
    outs = make_outputs(hp, spec) if outs is None else outs
    for t, (_, _, fill) in zip(outs, spec):
        t.fill_(fill)
    torch.cuda.synchronize()
    fam.call(L, outs)
    hp.sync()
    return [t.cpu().numpy().copy() for t in outs], outs


def same(a, b):
    return len(a) == len(b) and all(np.array_equal(x, y) for x, y in zip(a, b))


# ---- 1 ----
@pytest.mark.parametrize("entry", list(FAMILIES))
def test_same_list_on_another_stream(hp, oracle, entry):
    """a cached list run again after the context changed streams: the key matches and the stream differs, so the new stream is ordered behind the slot's event and nothing is
    uploaded; then another list on that stream (a rebuild behind an event recorded on the same stream), then the first list back on torch's stream (a rebuild behind an event
    recorded on the other stream); a further run of it allocates nothing on the device"""
    import torch
    fam = FAMILIES[entry](hp, oracle)
    A, B = fam.A, fam.B
    try:
        ra, outs_a = run(hp, fam, A)
        fam.check(A, ra, "A on torch's stream")
        hp.use_own_stream()
        again, _ = run(hp, fam, A, outs_a)
        assert same(again, ra), "the cached list on the context's own stream"
        rb, _ = run(hp, fam, B)
        fam.check(B, rb, "B on the context's own stream")
        hp.use_torch_stream()
        back, _ = run(hp, fam, A, outs_a)
        assert same(back, ra), "A rebuilt on torch's stream"
        free0 = torch.cuda.mem_get_info()[0]
        once_more, _ = run(hp, fam, A, outs_a)
        assert same(once_more, ra)
        assert torch.cuda.mem_get_info()[0] == free0
    finally:
        hp.use_torch_stream()


# ---- 2 ----
def test_per_call_arrays_back_to_back(hp):
    """vvhip_intra_luma_modes_batch and vvhip_visact keep their per-call host array in a slot: list A then list B with no synchronisation between, into separate outputs, give
    what A and B give alone — the second upload has to wait for the first launch's event before the slot's host copy and device copy are rewritten.  This checks the ordering
    as far as results can show it; it cannot prove the absence of a race (a launch that has already read its items is not disturbed by a rewrite that comes too early)"""
    import torch
    rng = np.random.default_rng(508)

    def intra_list(spec, tag):
        cl = [INC.Case("%s%d" % (tag, k), w, h, bd, mri, *INC.seeded(rng, w, h, bd, mri), modes, pm) for k, (w, h, bd, mri, modes, pm) in enumerate(spec)]
        items, ref, org, npred = INC.as_list(cl)
        return cl, items, dev16(hp, ref), dev16(hp, org), npred
    every = tuple(range(67))
    IA = intra_list([(16, 16, 10, 0, every, (0, 1, 34)), (8, 8, 10, 0, every, (18, 50)), (16, 4, 10, 0, (1, 2, 7, 50, 66), (2,)), (4, 8, 10, 2, (1, 2, 30, 54, 66), (54,)), (32, 32, 10, 0, every, (0, 66))], "a")
    IB = intra_list([(8, 8, 12, 0, every, (0, 51)), (4, 4, 10, 0, every, (1, 2, 66)), (32, 8, 10, 1, every[1:], (10,)), (8, 16, 8, 0, every, (26, 42)), (16, 16, 10, 0, every, (3, 49)), (64, 16, 10, 0, every, (50,))], "b")

    def intra_out(L):
        return (torch.full((len(L[1]) * 67,), SENTINEL, dtype=torch.int32, device=hp.device), torch.full((L[4],), SENTINEL, dtype=torch.int16, device=hp.device))

    def intra_call(L, out):
        hp.intra_luma_modes(L[1], L[2], L[3], cost=out[0], pred=out[1])
    alone = []
    for L in (IA, IB):
        out = intra_out(L)
        torch.cuda.synchronize()
        intra_call(L, out)
        torch.cuda.synchronize()
        alone.append([t.cpu().numpy() for t in out])
        cost = alone[-1][0].view(np.uint32).reshape(-1, 67)
        for k, c in enumerate(L[0]):
            wc, wp = INC.expected(c)
            o = int(L[1][k]["pred_off"])
            assert np.array_equal(cost[k][list(c.modes)], wc[list(c.modes)]) and int(wc.sum()) > 0, ("intra costs alone", c.name)
            assert np.array_equal(alone[-1][1][o:o + wp.size].reshape(wp.shape), wp), ("intra predictions alone", c.name)
    oa, ob = intra_out(IA), intra_out(IB)
    torch.cuda.synchronize()
    intra_call(IA, oa)
    intra_call(IB, ob)
    torch.cuda.synchronize()
    assert all(np.array_equal(t.cpu().numpy(), e) for t, e in zip(oa, alone[0])), "intra list A with list B issued right behind it"
    assert all(np.array_equal(t.cpu().numpy(), e) for t, e in zip(ob, alone[1])), "intra list B issued right behind list A"

    # the visual activity: the 72 x 40 picture's own area lists, HD first order and down-sampling second order — other tiles, other spans, another count of partial records
    from vvenc_amd.hotpath import PlaneView
    cases = VC.cases()
    VA, VB = cases["p72_10_hd1"], cases["p72_10_ds2"]
    assert VA.picture is VB.picture and len(VA.areas) > 1 and not np.array_equal(VA.areas, VB.areas)
    rows = []
    for (cur, p1, p2) in VA.picture.rows:
        rows.append(tuple(PlaneView(dev16(hp, a.reshape(-1)), 0, a.shape[1], a.shape[1], a.shape[0]) for a in (cur, p1, p2)) + (VA.picture.bit_depth,))

    def visact_out(c):
        return torch.full((len(c.areas), 4), SENT64, dtype=torch.int64, device=hp.device)
    valone = []
    for c in (VA, VB):
        out = visact_out(c)
        torch.cuda.synchronize()
        hp.visact(rows, c.areas, out=out)
        torch.cuda.synchronize()
        valone.append(out.cpu().numpy())
        assert np.array_equal(valone[-1].view(np.uint64), VR.records(c.picture.rows, c.areas)), ("visual activity alone", c.name)
    va, vb = visact_out(VA), visact_out(VB)
    torch.cuda.synchronize()
    hp.visact(rows, VA.areas, out=va)
    hp.visact(rows, VB.areas, out=vb)
    torch.cuda.synchronize()
    assert np.array_equal(va.cpu().numpy(), valone[0]), "visual-activity list A with list B issued right behind it"
    assert np.array_equal(vb.cpu().numpy(), valone[1]), "visual-activity list B issued right behind list A"


# ---- 3 ----
def test_cached_list_in_a_launch_graph(hp, oracle):
    """a vvhip_pred_inter_batch list that the slot already holds, recorded into a launch graph (one linear capture on one stream): the recorded call is launches only, and the
    replay gives what the direct call gave; a changed list called directly afterwards rebuilds the schedule behind an event that predates the capture, and is right"""
    import torch
    fam = PredFamily(hp, oracle)
    A, B = fam.A, fam.B
    try:
        direct, outs = run(hp, fam, A)
        fam.check(A, direct, "direct")
        g = hp.graph_capture(lambda: fam.call(A, outs))
        try:
            outs[0].fill_(SENTINEL)
            torch.cuda.synchronize()
            hp.graph_launch(g)
            hp.sync()
            assert np.array_equal(outs[0].cpu().numpy(), direct[0]), "the replayed list"
            rb, _ = run(hp, fam, B)
            fam.check(B, rb, "another list after the capture")
        finally:
            hp.graph_destroy(g)
    finally:
        hp.use_torch_stream()
