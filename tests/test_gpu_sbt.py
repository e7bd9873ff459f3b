"""GPU tier of the SBT entries: vvhip_sbt_parts_batch / vvhip_sbt_place_batch and the chain HotPath.tu_rdo_sbt, tolerance 0.

Expected values: the reference's own results recorded in tests/golden/sbt.npz (replayed directly) and tests/sbt_ref.py, the model pinned to that fixture by
tests/test_sbt_cpu.py; around the chain the `oracle` fixture's TU pipeline.  The lists come from tests/sbt_cases.py; tests/test_sbt_cpu.py asserts what they cover."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import ict_cases as IC  # noqa: E402
import sbt_cases as SC  # noqa: E402
import sbt_ref as SR  # noqa: E402

SENTINEL = SC.SENTINEL
SENT64 = -0x0123456789ABCDEF
GUARD = 3      # rows of the dense outputs behind the list's own, which must stay untouched


@pytest.fixture(scope="module")
def hp():
    from vvenc_amd.hotpath import HotPath
    return HotPath()


def dev16(hp, a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, np.int16)).to(hp.device)


def run_parts(hp, L, cw, resi=None, want=(True, True, True)):
    """-> ( parts [n, 3, 16], est [n, 9] as uint64, order [n, 8] ) as numpy (None where not asked for); the outputs are pre-filled with sentinels and have guard rows"""
    import torch
    n = len(L.items)
    parts = torch.full((n + GUARD, 3, 16), SENT64, dtype=torch.int64, device=hp.device) if want[0] else None
    est = torch.full((n + GUARD, 9), SENT64, dtype=torch.int64, device=hp.device) if want[1] else None
    order = torch.full((n + GUARD, 8), 0x5A, dtype=torch.uint8, device=hp.device) if want[2] else None
    d_resi = dev16(hp, L.resi) if resi is None else resi
    hp.sbt_parts_batch(d_resi, L.items, cw, parts, est, order)
    torch.cuda.synchronize()
    out = []
    for t, fill in ((parts, SENT64), (est, SENT64), (order, 0x5A)):
        if t is None:
            out.append(None)
            continue
        a = t.cpu().numpy()
        assert (a[n:] == fill).all(), "a row behind the list was written"
        out.append(a[:n].view(np.uint64) if a.dtype == np.int64 else a[:n])
    if resi is None:
        assert np.array_equal(d_resi.cpu().numpy(), L.resi), "the residual was written"
    return tuple(out)


def run_place(hp, L, P, want_rec=True, want_sse=True, items=None):
    """-> ( reconstruction laid out like the residual, sse [n, 3] as uint64 ) as numpy; pre-filled with sentinels"""
    import torch
    items = P["items"] if items is None else items
    n = len(items)
    rec = torch.full((L.resi.size,), SENTINEL, dtype=torch.int16, device=hp.device) if want_rec else None
    sse = torch.full((n + GUARD, 3), SENT64, dtype=torch.int64, device=hp.device) if want_sse else None
    hp.sbt_place_batch(dev16(hp, P["tile_rec"]), items, hp.to_device(P["stats"]), rec, dev16(hp, L.resi) if want_sse else None, sse)
    torch.cuda.synchronize()
    if want_sse:
        s = sse.cpu().numpy()
        assert (s[n:] == SENT64).all(), "a row behind the list was written"
    return (rec.cpu().numpy() if want_rec else None), (s[:n].view(np.uint64) if want_sse else None)


def check_place(L, P, cand, rec, sse, tag):
    for k, (cu, _) in enumerate(cand):
        for c in range(3):
            assert np.array_equal(L.view(rec, cu, c), P["blocks"][k][c]), (tag, "rec", k, c, P["items"][k])
    assert np.array_equal(sse, P["sse"]), (tag, "sse", np.argwhere(sse != P["sse"])[:3].tolist())
    assert (rec[~L.block_mask([cu for (cu, _) in cand])] == SENTINEL).all(), (tag, "a sample outside the blocks was written")


# ---- 1 ----
def test_replay_of_the_reference_fixture(hp):
    """every fixture CU through the parts entry, one list per chroma weight: part sums, estimates and order are what the reference's xCalcMinDistSbt and SSE entry recorded;
    every placed block of the fixture through the placement entry: the block and its SSE"""
    gold = SR.golden()
    assert len(gold["cus"]) >= 100
    for cw in sorted({c["cw"] for c in gold["cus"]}):
        cs = [c for c in gold["cus"] if c["cw"] == cw]
        L = SC.compact([(c["allowed"], (c["y"], c["cb"], c["cr"])) for c in cs])
        parts, est, order = run_parts(hp, L, cw)
        for i, c in enumerate(cs):
            what = (cw, i, c["w"], c["h"], c["allowed"])
            assert [[int(v) for v in row] for row in parts[i]] == c["parts"], ("parts",) + what
            assert [int(v) for v in est[i]] == c["est"], ("est",) + what
            assert [int(v) for v in order[i]] == c["order"], ("order",) + what
    # a placed block is the Cb block of a CU of twice its size (64 x 64: the luma block); the other components have no coefficients
    specs, cand, tiles, stats, at = [], [], [], [], 0
    for p in gold["placed"]:
        luma = p["w"] == 64
        W, H = (p["w"], p["h"]) if luma else (2 * p["w"], 2 * p["h"])
        z = SC.constant(W, H, 0)
        specs.append((SR.allowed_of(W, H), (p["org"], z[1], z[2]) if luma else (z[0], p["org"], z[2])))
    L = SC.compact(specs)
    items = np.zeros(len(specs), SR.SBT_PLACE_DTYPE)
    for k, p in enumerate(gold["placed"]):
        for name in ("y_off", "cb_off", "cr_off", "stride_y", "stride_c", "width", "height", "sbt_allowed"):
            items[k][name] = L.items[k][name]
        c = 0 if p["w"] == 64 else 1
        items[k]["mode"], items[k]["stats_idx"] = p["mode"], -1
        items[k]["stats_idx"][c], items[k]["tile_off"][c] = k, at
        tiles.append(p["tile"].reshape(-1)); at += p["tile"].size
        cand.append((k, p["mode"]))
    st = np.zeros(len(specs), SC.STATS_DTYPE)
    st["abs_sum"] = 5
    P = dict(items=items, tile_rec=np.concatenate(tiles), stats=st)
    rec, sse = run_place(hp, L, P)
    for k, p in enumerate(gold["placed"]):
        c = 0 if p["w"] == 64 else 1
        assert np.array_equal(L.view(rec, k, c), SR.place(p["tile"], p["w"], p["h"], p["mode"])) and int(sse[k][c]) == p["sse"], (k, p["w"], p["h"], p["mode"])
        assert all(not L.view(rec, k, o).any() and int(sse[k][o]) == 0 for o in range(3) if o != c)


# ---- 2 ----
@pytest.mark.parametrize("layout", ["compact", "compact-odd", "planes", "planes-odd"])
def test_parts_on_a_mixed_list_in_every_layout_and_shuffled(hp, layout):
    """72 CUs over every size in shuffled order (16-byte, 4-byte and 2-byte accesses by layout): against the model at a non-dyadic weight; the same list shuffled gives the
    same results per CU; run again it allocates nothing; each output may be absent; an empty list is no error"""
    import torch
    specs = SC.mixed_specs(41)
    L = {"compact": lambda: SC.compact(specs), "compact-odd": lambda: SC.compact(specs, odd_gaps=True), "planes": lambda: SC.planes(specs), "planes-odd": lambda: SC.planes(specs, odd=True)}[layout]()
    cw = SC.WEIGHTS[2]
    ep, ee, eo = SC.expected_parts(L, cw)
    parts, est, order = run_parts(hp, L, cw)
    assert np.array_equal(parts, ep), ("parts", np.argwhere(parts != ep)[:3].tolist())
    assert np.array_equal(est, ee), ("est", np.argwhere(est != ee)[:3].tolist())
    assert np.array_equal(order, eo), ("order", np.argwhere(order != eo)[:3].tolist())
    rng = np.random.default_rng(6)
    for perm in (rng.permutation(len(L.items)), np.arange(len(L.items))[::-1]):
        p2, e2, o2 = run_parts(hp, L.reordered(perm), cw)
        assert np.array_equal(p2, ep[perm]) and np.array_equal(e2, ee[perm]) and np.array_equal(o2, eo[perm])
    d_resi = dev16(hp, L.resi)
    run_parts(hp, L, cw, resi=d_resi)
    free0 = torch.cuda.mem_get_info()[0]
    for _ in range(3):
        again = run_parts(hp, L, cw, resi=d_resi)
    assert torch.cuda.mem_get_info()[0] == free0 and all(np.array_equal(a, b) for a, b in zip(again, (ep, ee, eo)))
    for want in ((True, False, False), (False, True, False), (False, False, True)):
        got = run_parts(hp, L, 1.0, resi=d_resi, want=want)
        e1 = SC.expected_parts(L, 1.0)
        assert all(g is None or np.array_equal(g, e) for g, e in zip(got, e1)), want
    hp.sbt_parts_batch(d_resi, L.items[:0], cw, None, None, None)
    hp.sbt_parts_batch(None, L.items[:0], cw, None, None, None)


# ---- 3 ----
@pytest.mark.parametrize("layout", ["compact", "compact-odd", "planes", "planes-odd"])
def test_placement_on_a_mixed_list_in_every_layout_and_shuffled(hp, layout):
    """one candidate per CU of the mixed list, coded / without levels / dropped per component, some tiles over the int16 range: every CU block of the reconstruction is
    written whole and nothing else, tiles without levels are never read (their memory holds other values), the SSEs against the model; shuffled; outputs may be absent"""
    specs = SC.mixed_specs(42)
    odd = layout.endswith("odd")
    L = SC.compact(specs, odd_gaps=odd) if layout.startswith("compact") else SC.planes(specs, odd=odd)
    cand = SC.all_candidates(L)
    P = SC.place_world(L, cand, 17, tile_gaps=odd, wide=True)
    assert {int(s) for s in P["items"]["stats_idx"].reshape(-1)} >= {-1, 0} and (P["stats"]["abs_sum"] == 0).any() and {m for (_, m) in cand} == set(range(8))
    rec, sse = run_place(hp, L, P)
    check_place(L, P, cand, rec, sse, layout)
    perm = np.random.default_rng(8).permutation(len(cand))
    Q = dict(P, items=P["items"][perm], blocks=[P["blocks"][i] for i in perm], sse=P["sse"][perm])
    rec2, sse2 = run_place(hp, L, Q)
    assert np.array_equal(rec2, rec) and np.array_equal(sse2, P["sse"][perm])
    rec3, _ = run_place(hp, L, P, want_sse=False)
    _, sse3 = run_place(hp, L, P, want_rec=False)
    assert np.array_equal(rec3, rec) and np.array_equal(sse3, sse)
    hp.sbt_place_batch(None, P["items"][:0], None, None, None, None)


# ---- 4 ----
def test_chain_sparse_outputs_off_and_on(hp, oracle):
    """HotPath.tu_rdo_sbt on the chain's 34 CUs with two candidates each, at QPs where tiles keep levels and at QPs where the flat CUs' tiles quantise to nothing: parts,
    estimates, order, levels, statistics, the placed reconstruction of both planes and the SSEs equal the model around the oracle's TU pipeline; with sparse outputs on the
    results are identical, rec included where tiles are all zero; a dropped component is zero"""
    import torch
    from vvenc_amd.hotpath import STATS_DTYPE
    world = SC.chain_world()
    L, cand = world["listed"], world["candidates"]
    d_resi = dev16(hp, L.resi)
    ep, ee, eo = SC.expected_parts(L, SC.WEIGHTS[1])
    for qps in SC.CHAIN_QPS:
        drop = ((3, 1), (8, 0)) if qps == SC.CHAIN_QPS[0] else ()
        exp = SC.chain_expected(oracle, world, qps, drop=drop)
        runs = []
        for sparse in (0, 1):
            hp.tu_set_sparse_outputs(sparse)
            try:
                parts, est, order, rec, sse, level, stats = hp.tu_rdo_sbt(d_resi, L.items, cand, qps, SC.WEIGHTS[1], world["bd"], drop=drop)
                torch.cuda.synchronize()
            finally:
                hp.tu_set_sparse_outputs(0)
            place = hp.last_sbt_place
            parts, est, order = parts.cpu().numpy().view(np.uint64), est.cpu().numpy().view(np.uint64), order.cpu().numpy()
            rec, sse, level = rec.cpu().numpy(), sse.cpu().numpy().view(np.uint64), level.cpu().numpy()
            st = stats.cpu().numpy().view(STATS_DTYPE).reshape(-1)
            assert np.array_equal(parts, ep) and np.array_equal(est, ee) and np.array_equal(order, eo)
            assert rec.shape == (2, L.resi.size)
            seen, n_zero = {}, 0
            for k, ((cu, mode), comps) in enumerate(zip(cand, exp)):
                plane = seen.get(cu, 0)
                seen[cu] = plane + 1
                for c, e in enumerate(comps):
                    what = (qps, sparse, k, cu, mode, c)
                    si = int(place[k]["stats_idx"][c])
                    if e["stats"] is None:
                        assert si == -1, what
                    else:
                        g = st[si]
                        assert (int(g["abs_sum"]), int(g["last_scan_pos"]), int(g["need_rdoq"]), int(g["sse"])) == tuple(e["stats"][f] for f in ("abs_sum", "last_scan_pos", "need_rdoq", "sse")), what
                        n_zero += e["stats"]["abs_sum"] == 0
                        if e["stats"]["abs_sum"]:      # (sparse outputs leave the levels of a TU without any unspecified)
                            o, cnt = int(place[k]["tile_off"][c]), e["level"].size
                            assert np.array_equal(level[o:o + cnt].reshape(e["level"].shape), e["level"]), what
                    assert np.array_equal(L.view(rec[plane], cu, c), e["placed"]), what
                    assert int(sse[k][c]) == e["sse"], what
            assert (rec[:, ~L.block_mask()] == 0).all()
            assert n_zero > 0 and n_zero < 3 * len(cand)
            runs.append((rec, sse))
        assert np.array_equal(runs[0][0], runs[1][0]) and np.array_equal(runs[0][1], runs[1][1])


# ---- 5 ----
def test_argument_errors(hp):
    """every argument error returns VVHIP_E_ARG with the entry's name in the message, launches nothing and leaves the outputs untouched and the context usable"""
    import torch
    from vvenc_amd.lib import VVHipError
    rng = np.random.default_rng(3)
    specs = [(SR.allowed_of(w, h), SC.seeded(rng, w, h, 10)) for (w, h) in ((16, 16), (8, 16), (16, 8))]
    L = SC.compact(specs)
    cand = [(0, 4), (1, 2), (2, 5)]
    P = SC.place_world(L, cand, 5)
    d_resi, d_tiles, d_stats = dev16(hp, L.resi), dev16(hp, P["tile_rec"]), hp.to_device(P["stats"])

    def broken(items, k=1, **changes):
        it = items.copy()
        for f, v in changes.items():
            it[k][f] = v
        return it
    geometry = [dict(width=12), dict(height=128), dict(width=2), dict(stride_y=4), dict(stride_c=3), dict(y_off=-2), dict(cb_off=-1), dict(cr_off=-8), dict(sbt_allowed=0),
                dict(sbt_allowed=1), dict(sbt_allowed=32 | 4), dict(sbt_allowed=2 | 8), dict(sbt_allowed=4 | 8), dict(rsv=1)]      # item 1 is 8 x 16: no vertical quad
    for entry in ("parts", "place"):
        name = "vvhip_sbt_%s_batch" % entry
        base = L.items if entry == "parts" else P["items"]
        cases = [(broken(base, **g), {}) for g in geometry]
        if entry == "parts":
            cases += [(base, dict(no_resi=True)), (base, dict(cw=-1.0)), (base, dict(cw=float("nan")))]
        else:
            cases += [(broken(base, mode=8), {}), (broken(base, mode=255), {}), (broken(base, mode=4), {}), (broken(base, k=2, mode=6), {}), (broken(base, k=0, sbt_allowed=6), {}),
                      (broken(base, stats_idx=(-2, 0, 0)), {}), (broken(base, k=0, tile_off=(-4, 0, 0)), {}), (base, dict(no_stats=True)), (base, dict(no_tiles=True)), (base, dict(no_org=True))]
        for k, (it, opt) in enumerate(cases):
            rec = torch.full((L.resi.size,), SENTINEL, dtype=torch.int16, device=hp.device)
            sums = torch.full((3, 48), SENT64, dtype=torch.int64, device=hp.device)
            order = torch.full((3, 8), 0x5A, dtype=torch.uint8, device=hp.device)
            with pytest.raises(VVHipError) as e:
                if entry == "parts":
                    hp.sbt_parts_batch(None if opt.get("no_resi") else d_resi, it, opt.get("cw", 1.0), sums, sums, order)
                else:
                    hp.sbt_place_batch(None if opt.get("no_tiles") else d_tiles, it, None if opt.get("no_stats") else d_stats, rec, None if opt.get("no_org") else d_resi, sums)
            assert name in str(e.value) and "error -1" in str(e.value), (entry, k, str(e.value))
            torch.cuda.synchronize()
            assert (rec.cpu().numpy() == SENTINEL).all() and (sums.cpu().numpy() == SENT64).all() and (order.cpu().numpy() == 0x5A).all(), (entry, k)
        rc = getattr(hp.L, name)(hp.ctx, None, None, -1, *([1.0, None, None, None] if entry == "parts" else [None] * 4))
        assert rc == -1 and name in hp.L.vvhip_last_error(hp.ctx).decode()
    # a list without statistics entries needs neither statistics nor tiles, and the context still works
    dropped = P["items"].copy()
    dropped["stats_idx"] = -1
    rec = torch.full((L.resi.size,), SENTINEL, dtype=torch.int16, device=hp.device)
    sse = torch.empty((3, 3), dtype=torch.int64, device=hp.device)
    hp.sbt_place_batch(None, dropped, None, rec, d_resi, sse)
    torch.cuda.synchronize()
    assert [[int(v) for v in r] for r in sse.cpu().numpy()] == [[SR.sse(b, 0) for b in L.blocks[cu]] for (cu, _) in cand]
    assert (rec.cpu().numpy()[L.block_mask()] == 0).all()
    rec, sse = run_place(hp, L, P)
    check_place(L, P, cand, rec, sse, "after the errors")


# ---- 6 ----
def test_alternating_with_the_joint_and_prediction_entries_keeps_every_schedule(hp):
    """the SBT entries, the joint Cb-Cr entries and vvhip_pred_inter_batch alternating on one context: every output stays what it was and nothing is allocated on the device"""
    import torch
    import blend_cases as BLC
    pl, _ = BLC.planes(10, 110)
    dev = [hp.plane(a, 0) for a in pl]
    pitems = BLC.bcw_list(pl, 300)[0][:9].copy()
    pitems["dst_off"], ptot = BLC.compact_offsets(pitems)
    F = IC.compact(IC.mixed_specs(34, False, n=40))
    L = SC.planes(SC.mixed_specs(43, n=40))
    cand = SC.all_candidates(L)
    P = SC.place_world(L, cand, 19)
    ep, ee, eo = SC.expected_parts(L, SC.WEIGHTS[4])
    d_f, d_resi, d_tiles, d_stats = dev16(hp, F.resi), dev16(hp, L.resi), dev16(hp, P["tile_rec"]), hp.to_device(P["stats"])
    o_pred = torch.empty((ptot,), dtype=torch.int16, device=hp.device)
    o_joint = torch.empty((F.joint_total,), dtype=torch.int16, device=hp.device)
    o_dist = torch.empty((len(F.items), 2), dtype=torch.int64, device=hp.device)
    o_parts = torch.empty((len(L.items), 3, 16), dtype=torch.int64, device=hp.device)
    o_est = torch.empty((len(L.items), 9), dtype=torch.int64, device=hp.device)
    o_order = torch.empty((len(L.items), 8), dtype=torch.uint8, device=hp.device)
    o_rec = torch.empty((L.resi.size,), dtype=torch.int16, device=hp.device)
    o_sse = torch.empty((len(cand), 3), dtype=torch.int64, device=hp.device)
    first, free1 = None, None
    for rnd in range(3):
        for t in (o_pred, o_joint, o_rec):
            t.fill_(SENTINEL)
        hp.sbt_parts_batch(d_resi, L.items, SC.WEIGHTS[4], o_parts, o_est, o_order)
        hp.pred_inter_batch(dev, pitems, o_pred, 0, 10)
        hp.ict_fwd_batch(d_f, F.items, o_joint, o_dist)
        hp.sbt_place_batch(d_tiles, P["items"], d_stats, o_rec, d_resi, o_sse)
        torch.cuda.synchronize()
        got = [t.cpu().numpy().copy() for t in (o_pred, o_joint, o_dist, o_parts, o_est, o_order, o_rec, o_sse)]
        if rnd == 0:
            first, free1 = got, torch.cuda.mem_get_info()[0]
            assert np.array_equal(got[3].view(np.uint64), ep) and np.array_equal(got[4].view(np.uint64), ee) and np.array_equal(got[5], eo)
            check_place(L, P, cand, got[6], got[7].view(np.uint64), "alternating")
            assert got[0].min() >= 0
        else:
            assert all(np.array_equal(a, b) for a, b in zip(got, first)), rnd
            assert torch.cuda.mem_get_info()[0] == free1, rnd
