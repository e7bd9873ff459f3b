"""-m gpu: the distortion list entries of dist.hip against the oracle (tolerance 0) on the extreme inputs of tests/dist_extremes.py — vvhip_dist_batch, vvhip_dist_multi,
vvhip_dist_multi_func, vvhip_dist_multi_func_tiled, vvhip_plane_tile8, vvhip_plane_shift1, vvhip_planes_derive, vvhip_sad_mask_batch and vvhip_fix_weighted_sse_batch, all
through HotPath.  The oracle itself is pinned to the compiled reference on the same items by tests/test_oracle_dist_extremes.py, which also holds the guards (every Hadamard
coefficient at 64 D with either sign, accumulators at 128 * 128 * 65535 and beyond 2^32, the list lengths, table sizes and workgroup counts, all phases of the tiled copies,
the reference's undefined corners kept out) and the sensitivity test.

What is compared (every expected value comes from the oracle; every output list sits between eight canary entries on either side, which must come back intact):
  A  vvhip_dist_batch: the 16 shapes of the tile ladder x HAD, HAD_fast, HAD_2SAD x six domains (samples of 10, 8, 12 bits, the bi-prediction pattern of 10 and 8 bits,
     full int16).  Merged: squares 8 .. 128 x HAD, HAD_fast x five domains through vvhip_dist_multi (the general packed form, or the 32-bit kernel at 12 bits),
     vvhip_dist_multi_func (with the domain's flag: the all-packed form for the sample domains) and vvhip_dist_multi_func_tiled with the shifted copy; candidates at even
     and odd x
  B  SAD and SSE of 30 shapes x four domains through vvhip_dist_batch; the shapes whose width is a multiple of 8 also through vvhip_dist_multi and vvhip_dist_multi_func
     with and without the flag (the v_dot2 SSE at 12 and 10 bits)
  C  lists of 1 .. 257 items through vvhip_dist_batch, vvhip_dist_multi_func and vvhip_dist_multi_func_tiled (tiled copies and shifted copy), flagged and not; the job
     tables of 9, 16, 17 jobs, of 8 / 9 / 15 / 17 workgroups and the interleaved one, forward, reversed and shuffled, through both merged entries
  D  the three copy entries against their numpy restatement on planes built through Plane(..., stride=...), canaries behind vvhip_tiled8_elems and behind the shifted
     copy, the shifted copy into an unaligned destination too; 8x8 SAD, SSE, flagged SSE and 16x16 SAD lists on the copies, each item against the oracle
  E  the masked SAD (72 configurations x 12 items x two domains) and the fixed-weight SSE (seven sizes x 40 level / weight pairs)
The last test asserts that every (entry, kernel form, shape) cell that the families define was compared, and that the cells cover every kernel form of the host code.

Measured on an MI355X: the file 2.8 s, of which 1.6 s are set-up (the device context); per test 0.12 s the first batch test of family A, 0.07 s the lists of family C,
0.05 s the job tables, 0.02 s and less every other one (195 436 items compared with the oracle, 45 000 oracle calls, cached over the entries).  In the same visit the whole
GPU suite of the parent commit (`-m gpu`, everything but this file: 474 passed, 2 skipped) took 400.7 s.
"""
import numpy as np
import pytest

import dist_extremes as M

pytestmark = pytest.mark.gpu

GUARD = 8
PAT = 0x5A5A5A5A5A5A5A5A
COVER = {}                                    # (entry, kernel form, (w, h)) -> items compared with the oracle

FORMS = {"sad<2>", "sad<4>", "sad<8>", "sad<2>-div", "sad<4>-div", "sad<8>-div", "sse<2>", "sse<4>", "sse<8>", "sse<2>-div", "sse<4>-div", "sse<8>-div", "had2sad",
         "had-16x8", "had-8x16", "had-8x4", "had-4x8", "had-fast16", "had-8x8", "had-4x4", "had-2x2",
         "merged-sad", "merged-sad-div", "merged-sse", "merged-sse-div", "merged-sse-pk", "merged-sse-pk-div", "tiled8-sad", "tiled8-sse", "tiled8-sse-pk",
         "merged-8x8-narrow", "merged-8x8-wide", "merged-8x8-32bit", "merged-fast16-narrow", "merged-fast16-wide", "merged-fast16-32bit", "mask", "wsse"}


@pytest.fixture(scope="module")
def hip():
    from hip_backend import HipBackend
    return HipBackend()


_exp = {}


def _expected(oracle, dom, job):
    out = []
    for k in range(job.n):
        key = (dom.name[:3] if dom.name.startswith("tex") else dom.name,) + job.key(k)
        if key not in _exp:
            _exp[key] = M.expected(oracle, dom, job, k)
        out.append(_exp[key])
    return out


def _cover(entry, form, w, h, n):
    COVER[(entry, form, (w, h))] = COVER.get((entry, form, (w, h)), 0) + n


class Dev:
    """a domain's two planes on the device; origin: where sample (0, 0) of the numpy planes lies relative to the device planes' sample (0, 0)"""

    def __init__(self, hp, dom, planes=None, origin=(0, 0)):
        self.dom = dom
        self.po, self.pc = planes if planes else (hp.plane(dom.org, 0), hp.plane(dom.cur, 0))
        self.origin = origin
        self._items = {}

    def items(self, hp, job):
        if id(job) not in self._items:
            dx, dy = self.origin
            it = np.array([((oy + dy) * self.po.stride + ox + dx, (cy + dy) * self.pc.stride + cx + dx) for (ox, oy, cx, cy) in job.items] or [(0, 0)], np.int32)
            self._items[id(job)] = hp.to_device(it)
        return self._items[id(job)]


def _held(hp, n):
    import torch
    return torch.full((n + 2 * GUARD,), PAT, dtype=torch.int64, device=hp.device)


def _read(held, n, what):
    a = held.cpu().numpy()
    assert (a[:GUARD] == PAT).all() and (a[GUARD + n:] == PAT).all(), ("an entry outside [0, n) was written", what)
    return a[GUARD:GUARD + n].view(np.uint64).tolist()


def _compare(got, exp, what):
    bad = [(k, got[k], exp[k]) for k in range(len(exp)) if got[k] != exp[k]]
    assert not bad, (what, len(bad), bad[:4])


def run_batch(hp, dv, job, oracle):
    held = _held(hp, job.n)
    hp.dist_batch(job.func, dv.po, dv.pc, dv.items(hp, job), job.n, job.w, job.h, job.ss, dv.dom.bd, out=held[GUARD:GUARD + job.n])
    what = ("vvhip_dist_batch", dv.dom.name, job.func, job.w, job.h, job.ss, job.tag)
    _compare(_read(held, job.n, what), _expected(oracle, dv.dom, job), what)
    _cover("batch", M.kernel_form("batch", job.func, job.w, job.h, job.ss, dv.dom.bd, 0), job.w, job.h, job.n)


def run_table(hp, dv, jobs, oracle, entry, flags=0, tiled=None, shift=None, order=None):
    """one call of a merged entry on a job table (None: a job with n = 0) -> every job's values against the oracle.  entry: multi (one function, no flags), multi_func,
    multi_func_tiled (tiled: the two tiled copies or None; shift: the shifted copy or None)"""
    order = list(range(len(jobs))) if order is None else order
    table, helds = [], []
    for i in order:
        job = jobs[i]
        if job is None:
            table.append(("SAD", 8, 8, 0, 0, hp.to_device(np.zeros((1, 2), np.int32)), _held(hp, 0)))
            helds.append(table[-1][6])
            continue
        held = _held(hp, job.n)
        helds.append(held)
        table.append((job.func, job.w, job.h, job.ss, job.n, dv.items(hp, job), held[GUARD:GUARD + job.n]))
    bd = dv.dom.bd
    if entry == "multi":
        assert len({t[0] for t in table}) == 1 and not flags
        hp.dist_multi(table[0][0], dv.po, dv.pc, [t[1:] for t in table], bd)
    elif entry == "multi_func":
        hp.dist_multi_func(dv.po, dv.pc, hp.make_dist_fjobs(table, flags=flags), bd)
    else:
        hp.dist_multi_func_tiled(dv.po, dv.pc, tiled[0] if tiled else None, tiled[1] if tiled else None, hp.make_dist_fjobs(table, flags=flags), bd, cur_shift=shift)
    for i, held in zip(order, helds):
        job = jobs[i]
        what = ("vvhip_dist_" + entry, dv.dom.name, flags, tiled is not None, shift is not None, i, job and (job.func, job.w, job.h, job.ss, job.n, job.tag))
        if job is None:
            _read(held, 0, what)
            continue
        _compare(_read(held, job.n, what), _expected(oracle, dv.dom, job), what)
        _cover(entry + ("+tiled" if tiled else "") + ("+shift" if shift is not None else ""),
               M.kernel_form(entry, job.func, job.w, job.h, job.ss, bd, flags, tiled is not None), job.w, job.h, job.n)


# ---- family A ----------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", M.A_DOMAINS)
def test_hadamard_operand_range_batches(hip, oracle, name):
    dv = Dev(hip.hp, M.a_domain(name))
    for job in M.a_batch_jobs():
        run_batch(hip.hp, dv, job, oracle)


@pytest.mark.parametrize("name", M.A_MULTI_DOMAINS)
def test_hadamard_operand_range_merged(hip, oracle, name):
    """the squares through vvhip_dist_multi (no flag: the general packed form on every domain of 10 and 8 bits), vvhip_dist_multi_func with the domain's flag, and
    vvhip_dist_multi_func_tiled with the shifted copy present"""
    hp = hip.hp
    dom = M.a_domain(name)
    dv = Dev(hp, dom)
    jobs = M.a_multi_jobs()
    for func in ("HAD", "HAD_fast"):
        run_table(hp, dv, [j for j in jobs if j.func == func], oracle, "multi")
    run_table(hp, dv, jobs, oracle, "multi_func", dom.flags)
    sh = hp.shift_plane(dv.pc)
    run_table(hp, dv, jobs, oracle, "multi_func_tiled", dom.flags, None, sh)
    if dom.flags:
        run_table(hp, dv, jobs, oracle, "multi_func_tiled", 0, None, sh)


# ---- family B ----------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", M.B_DOMAINS)
def test_sad_sse_accumulators_and_row_walks(hip, oracle, name):
    hp = hip.hp
    dom = M.b_domain(name)
    dv = Dev(hp, dom)
    jobs = M.b_jobs(name)
    for job in jobs:
        run_batch(hp, dv, job, oracle)
    merged = [j for j in jobs if j.w % 8 == 0]
    assert {j.w for j in merged} >= {24, 40, 72, 96, 120, 128}
    for func in ("SAD", "SSE"):
        if [j for j in merged if j.func == func]:
            run_table(hp, dv, [j for j in merged if j.func == func], oracle, "multi")
    for flags in {0, dom.flags}:
        run_table(hp, dv, merged, oracle, "multi_func", flags)
    run_table(hp, dv, merged, oracle, "multi_func_tiled", dom.flags, None, hp.shift_plane(dv.pc))


# ---- family C ----------------------------------------------------------------------------------------------------------------------------------------------------
def _derived(hp, dv):
    return (hp.tile_plane(dv.po), hp.tile_plane(dv.pc)), hp.shift_plane(dv.pc)


@pytest.mark.parametrize("flags", (0, M.FLAG_SAMPLES))
def test_list_lengths_and_shared_originals(hip, oracle, flags):
    hp = hip.hp
    dv = Dev(hp, M.c_domain(flags))
    jobs = M.c_list_jobs()
    if not flags:
        for job in jobs:
            run_batch(hp, dv, job, oracle)
    merged = [j for j in jobs if j.func != "HAD_2SAD"]
    tiled, sh = _derived(hp, dv)
    run_table(hp, dv, merged, oracle, "multi_func", flags)
    run_table(hp, dv, merged, oracle, "multi_func_tiled", flags, tiled, sh)
    run_table(hp, dv, merged, oracle, "multi_func_tiled", flags, tiled, None)


@pytest.mark.parametrize("flags", (0, M.FLAG_SAMPLES))
def test_job_tables_in_any_order(hip, oracle, flags):
    """every table forward, reversed and shuffled: the values depend on no job's place in its launch"""
    hp = hip.hp
    dv = Dev(hp, M.c_domain(flags))
    tiled, sh = _derived(hp, dv)
    for name, table in M.c_tables().items():
        for order in M.table_orders(len(table)):
            run_table(hp, dv, table, oracle, "multi_func", flags, order=order)
            run_table(hp, dv, table, oracle, "multi_func_tiled", flags, tiled, sh, order=order)


# ---- family D ----------------------------------------------------------------------------------------------------------------------------------------------------
def _d_planes(hp, stride, height):
    import torch
    from vvenc_amd.hotpath import Plane
    out = []
    for a in M.d_storage(stride, height):
        p = Plane(hp.device, M.D_W, height, M.D_PAD, stride=stride)
        assert tuple(p.storage.shape) == a.shape and p.stride == stride
        p.storage.copy_(torch.from_numpy(a).to(hp.device))
        out.append(p)
    return out


def _sent(hp, n):
    import torch
    return torch.full((n,), M.SENT16, dtype=torch.int16, device=hp.device)


@pytest.mark.parametrize("stride,height", M.D_PLANES)
def test_derived_copies(hip, stride, height):
    """vvhip_plane_tile8, vvhip_plane_shift1 and vvhip_planes_derive against their restatements; nothing behind vvhip_tiled8_elems or behind the shifted copy is written;
    the shifted copy also into a destination that is 2-byte aligned only (the scalar path of the kernel)"""
    hp = hip.hp
    po, pc = _d_planes(hp, stride, height)
    so, sc = M.d_storage(stride, height)
    rows = height + 2 * M.D_PAD
    n = int(hp.L.vvhip_tiled8_elems(stride, rows))
    assert n == M.tiled8_elems(stride, rows)
    for plane, a in ((po, so), (pc, sc)):
        t = hp.tile_plane(plane, out=_sent(hp, n + 64)).cpu().numpy()
        assert np.array_equal(t[:n - 128], M.tile8_model(a)), (stride, "tiled copy")
        assert (t[n:] == M.SENT16).all(), (stride, "samples behind vvhip_tiled8_elems were written")
    for lead in (0, 8, 3):
        buf = _sent(hp, lead + sc.size + 64)
        hp.shift_plane(pc, out=buf[lead:])
        s = buf.cpu().numpy()
        assert np.array_equal(s[lead:lead + sc.size], M.shift1_model(sc)), (stride, lead, "shifted copy")
        assert (s[:lead] == M.SENT16).all() and (s[lead + sc.size:] == M.SENT16).all(), (stride, lead, "samples around the shifted copy were written")
    to, tc, sh = _sent(hp, n + 64), _sent(hp, n + 64), _sent(hp, sc.size + 64)
    hp.planes_derive(po, pc, to, tc, sh)
    to, tc, sh = to.cpu().numpy(), tc.cpu().numpy(), sh.cpu().numpy()
    assert np.array_equal(to[:n - 128], M.tile8_model(so)) and np.array_equal(tc[:n - 128], M.tile8_model(sc)) and np.array_equal(sh[:sc.size], M.shift1_model(sc)), stride
    assert (to[n:] == M.SENT16).all() and (tc[n:] == M.SENT16).all() and (sh[sc.size:] == M.SENT16).all(), stride
    only = _sent(hp, sc.size + 64)
    hp.planes_derive(po, pc, None, None, only)
    assert np.array_equal(only.cpu().numpy()[:sc.size], M.shift1_model(sc))
    assert np.array_equal(po.storage.cpu().numpy(), so) and np.array_equal(pc.storage.cpu().numpy(), sc)
    _cover("copies", "tile8+shift1+derive", stride, rows, 1)


@pytest.mark.parametrize("stride,height", M.D_PLANES)
def test_lists_on_the_derived_copies(hip, oracle, stride, height):
    """every phase of the funnel shift, the wave-aligned shortcut with and without one unaligned candidate, the corners of the padded plane: each item against the oracle,
    with the flag (the packed SSE) and without (the 64-bit SSE); an odd stride ignores the shifted copy"""
    hp = hip.hp
    dom = M.d_domain(stride, height)
    po, pc = _d_planes(hp, stride, height)
    dv = Dev(hp, dom, (po, pc), (-M.D_PAD, -M.D_PAD))
    tiled, sh = _derived(hp, dv)
    jobs = M.d_jobs(stride, height)
    for flags in (0, M.FLAG_SAMPLES):
        run_table(hp, dv, jobs, oracle, "multi_func_tiled", flags, tiled, sh)
        run_table(hp, dv, jobs, oracle, "multi_func_tiled", flags, tiled, None)
        run_table(hp, dv, jobs, oracle, "multi_func_tiled", flags, None, sh)
    run_table(hp, dv, jobs, oracle, "multi_func", 0)


# ---- family E ----------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", M.E_DOMAINS)
def test_masked_sad(hip, oracle, name):
    hp = hip.hp
    dom, mask = M.b_domain(name), M.e_mask()
    dv = Dev(hp, dom)
    pm = hp.plane(mask, 0)
    assert pm.stride == mask.shape[1]
    for (w, h, ss, sx, ms2, items) in M.e_mask_items(name):
        n = len(items)
        d_it = hp.to_device(np.array([(oy * dv.po.stride + ox, cy * dv.pc.stride + cx) for (ox, oy, cx, cy, _, _) in items], np.int32))
        d_mo = hp.to_device(np.array([my * pm.stride + mx for (_, _, _, _, mx, my) in items], np.int32))
        held = _held(hp, n)
        hp.sad_mask_batch(dv.po, dv.pc, pm, sx, ms2, d_it, d_mo, n, w, h, ss, dom.bd, out=held[GUARD:GUARD + n])
        what = ("vvhip_sad_mask_batch", name, w, h, ss, sx, ms2)
        exp = [oracle.sad_mask((dom.org, oy, ox), (dom.cur, cy, cx), (mask, my, mx), sx, ms2, w, h, ss) for (ox, oy, cx, cy, mx, my) in items]
        _compare(_read(held, n, what), exp, what)
        _cover("sad_mask", "mask", w, h, n)


def test_fixed_weight_sse(hip, oracle):
    hp = hip.hp
    dom = M.e_levels_domain()
    dv = Dev(hp, dom)
    for (w, h, items) in M.e_wsse_items():
        n = len(items)
        d_it = hp.to_device(np.array([(oy * dv.po.stride + ox, cy * dv.pc.stride + cx) for (ox, oy, cx, cy, _) in items], np.int32))
        d_w = hp.to_device(np.array([wt for (_, _, _, _, wt) in items], np.uint32).view(np.int32))
        held = _held(hp, n)
        hp.fix_weighted_sse_batch(dv.po, dv.pc, d_it, d_w, n, w, h, dom.bd, out=held[GUARD:GUARD + n])
        what = ("vvhip_fix_weighted_sse_batch", w, h)
        exp = [oracle.fix_weighted_sse((dom.org, oy, ox), (dom.cur, cy, cx), w, h, wt) for (ox, oy, cx, cy, wt) in items]
        _compare(_read(held, n, what), exp, what)
        _cover("fix_weighted_sse", "wsse", w, h, n)


# ---- coverage ----------------------------------------------------------------------------------------------------------------------------------------------------
def _cells():
    """every (entry, kernel form, shape) the tests above are meant to compare, from the family builders and the restated host dispatch"""
    cells = set()

    def add(entry, route, job, bd, flags, tiled=False):
        cells.add((entry, M.kernel_form(route, job.func, job.w, job.h, job.ss, bd, flags, tiled), (job.w, job.h)))

    for name in M.A_DOMAINS:
        for job in M.a_batch_jobs():
            add("batch", "batch", job, M.a_domain(name).bd, 0)
    for name in M.A_MULTI_DOMAINS:
        dom = M.a_domain(name)
        for job in M.a_multi_jobs():
            add("multi", "multi", job, dom.bd, 0)
            add("multi_func", "multi_func", job, dom.bd, dom.flags)
            add("multi_func_tiled+shift", "multi_func_tiled", job, dom.bd, dom.flags)
            add("multi_func_tiled+shift", "multi_func_tiled", job, dom.bd, 0)
    for name in M.B_DOMAINS:
        dom = M.b_domain(name)
        for job in M.b_jobs(name):
            add("batch", "batch", job, dom.bd, 0)
            if job.w % 8 == 0:
                add("multi", "multi", job, dom.bd, 0)
                add("multi_func", "multi_func", job, dom.bd, 0)
                add("multi_func", "multi_func", job, dom.bd, dom.flags)
                add("multi_func_tiled+shift", "multi_func_tiled", job, dom.bd, dom.flags)
    for job in M.c_list_jobs():
        add("batch", "batch", job, 10, 0)
    for job in [j for j in M.c_list_jobs() if j.func != "HAD_2SAD"] + [j for t in M.c_tables().values() for j in t if j is not None]:
        for flags in (0, M.FLAG_SAMPLES):
            add("multi_func", "multi_func", job, 10, flags)
            add("multi_func_tiled+tiled+shift", "multi_func_tiled", job, 10, flags, True)
    for (stride, height) in M.D_PLANES:
        cells.add(("copies", "tile8+shift1+derive", (stride, height + 2 * M.D_PAD)))
        for job in M.d_jobs(stride, height):
            for flags in (0, M.FLAG_SAMPLES):
                add("multi_func_tiled+tiled+shift", "multi_func_tiled", job, 10, flags, True)
                add("multi_func_tiled+tiled", "multi_func_tiled", job, 10, flags, True)
                add("multi_func_tiled+shift", "multi_func_tiled", job, 10, flags)
            add("multi_func", "multi_func", job, 10, 0)
    for name in M.E_DOMAINS:
        cells |= {("sad_mask", "mask", (w, h)) for (w, h, _, _, _, _) in M.e_mask_items(name)}
    cells |= {("fix_weighted_sse", "wsse", (w, h)) for (w, h, _) in M.e_wsse_items()}
    return cells


def test_every_cell_was_compared():
    """runs last in the file: no (entry, kernel form, shape) cell of the families is empty, and the cells name every kernel form and every entry — the tier cannot pass by
    skipping"""
    cells = _cells()
    empty = sorted(c for c in cells if COVER.get(c, 0) == 0)
    assert not empty, (len(empty), empty[:8])
    assert {f for (_, f, _) in cells if f != "tile8+shift1+derive"} == FORMS, ({f for (_, f, _) in cells} ^ FORMS)
    assert {e.split("+")[0] for (e, _, _) in cells} == {"batch", "multi", "multi_func", "multi_func_tiled", "copies", "sad_mask", "fix_weighted_sse"}
    print("cells compared: %d, items compared with the oracle: %d" % (len(cells), sum(COVER.values())))
