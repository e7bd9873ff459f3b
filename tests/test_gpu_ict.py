"""GPU tier of the joint Cb-Cr entries: vvhip_ict_fwd_batch / vvhip_ict_inv_batch and the chain HotPath.tu_rdo_joint, tolerance 0.

Expected values: the reference's own results recorded in tests/golden/ict.npz (replayed directly) and tests/ict_ref.py, the numpy model pinned to that fixture by
tests/test_ict_cpu.py; around the chain the `oracle` fixture's TU pipeline.  The lists come from tests/ict_cases.py; tests/test_ict_cpu.py asserts what they cover."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import blend_cases as BLC  # noqa: E402
import ict_cases as IC  # noqa: E402
import ict_ref as IR  # noqa: E402

SENTINEL = IC.SENTINEL
SENT64 = -0x0123456789ABCDEF


@pytest.fixture(scope="module")
def hp():
    from vvenc_amd.hotpath import HotPath
    return HotPath()


def dev16(hp, a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, np.int16)).to(hp.device)


def run_fwd(hp, L, resi=None, want_dist=True):
    """-> ( joint buffer, dist [n, 2] ) as numpy; the outputs are pre-filled with sentinels"""
    import torch
    joint = torch.full((max(L.joint_total, 1),), SENTINEL, dtype=torch.int16, device=hp.device)
    dist = torch.full((len(L.items), 2), SENT64, dtype=torch.int64, device=hp.device) if want_dist else None
    hp.ict_fwd_batch(dev16(hp, L.resi) if resi is None else resi, L.items, joint, dist)
    torch.cuda.synchronize()
    return joint.cpu().numpy(), (dist.cpu().numpy() if want_dist else None)


def run_inv(hp, L, joint_rec, stats=None, want_rec=True, want_sse=True):
    """-> ( reconstruction laid out like the residual, sse [n, 2] as uint64 ) as numpy; pre-filled with sentinels"""
    import torch
    rec = torch.full((L.resi.size,), SENTINEL, dtype=torch.int16, device=hp.device) if want_rec else None
    sse = torch.full((len(L.items), 2), SENT64, dtype=torch.int64, device=hp.device) if want_sse else None
    hp.ict_inv_batch(dev16(hp, joint_rec), L.items, stats, rec, dev16(hp, L.resi) if want_sse else None, sse)
    torch.cuda.synchronize()
    return (rec.cpu().numpy() if want_rec else None), (sse.cpu().numpy().view(np.uint64) if want_sse else None)


def joint_buffer(L, blocks, fill=SENTINEL):
    buf = np.full(max(L.joint_total, 1), fill, np.int16)
    for i, b in enumerate(blocks):
        if b is not None:
            L.joint(buf, i)[:] = b
    return buf


def check_fwd(L, joint, dist, tag):
    ej, ed = IC.expected_fwd(L)
    for i, e in enumerate(ej):
        if e is not None:
            assert np.array_equal(L.joint(joint, i), e), (tag, "joint", i, L.items[i])
    assert np.array_equal(dist, ed), (tag, "dist", np.argwhere(dist != ed)[:3].tolist())
    assert (joint[~L.joint_mask()] == SENTINEL).all(), (tag, "a sample outside the joint blocks was written")


def check_inv(L, jblocks, rec, sse, tag):
    er, es = IC.expected_inv(L, jblocks)
    for i, (a, b) in enumerate(er):
        assert np.array_equal(L.cb(rec, i), a) and np.array_equal(L.cr(rec, i), b), (tag, "rec", i, L.items[i])
    assert np.array_equal(sse, es), (tag, "sse", np.argwhere(sse != es)[:3].tolist())
    assert (rec[~L.block_mask()] == SENTINEL).all(), (tag, "a sample outside the blocks was written")


# ---- 1 ----
def test_replay_of_the_reference_fixture(hp):
    """every fixture case through both entries, all cases in one list: joint blocks, d1 / d2, both reconstructions (from the joint block and from the input block as the coded
    component) and both SSEs are what the reference recorded"""
    cases = IR.golden_cases()
    L = IC.compact(IC.golden_specs(cases))
    joint, dist = run_fwd(hp, L)
    assert len(cases) >= 200
    for i, c in enumerate(cases):
        assert (int(dist[i][0]), int(dist[i][1])) == (c["d1"], c["d2"]), (i, c["mode"], c["w"], c["h"])
        if c["mode"]:
            assert np.array_equal(L.joint(joint, i), c["joint"]), (i, c["mode"], c["w"], c["h"])
    assert (joint[~L.joint_mask()] == SENTINEL).all()
    nz = [c for c in cases if c["mode"]]
    N = IC.compact(IC.golden_specs(nz))
    for src, out in (("joint", ("rec_cb", "rec_cr")), (None, ("in_cb", "in_cr"))):
        blocks = [c["joint"] if src else (c["cr"] if abs(c["mode"]) == 3 else c["cb"]) for c in nz]
        rec, sse = run_inv(hp, N, joint_buffer(N, blocks))
        for i, c in enumerate(nz):
            assert np.array_equal(N.cb(rec, i), c[out[0]]) and np.array_equal(N.cr(rec, i), c[out[1]]), (src, i, c["mode"], c["w"], c["h"])
            assert (int(sse[i][0]), int(sse[i][1])) == (IR.sse(c[out[0]], c["cb"]), IR.sse(c[out[1]], c["cr"])), (src, i)


# ---- 2 and 3 ----
@pytest.mark.parametrize("layout", ["compact", "planes"])
def test_mixed_list_in_both_layouts_and_shuffled(hp, layout):
    """about 200 items over all sizes and modes (compact: some blocks at odd offsets, so every vector width runs): both entries against the model, nothing outside the
    blocks changes; the same list shuffled gives the same results per item; a list that is run again allocates nothing on the device; optional outputs may be absent"""
    import torch
    make = (lambda s: IC.compact(s, odd_gaps=True)) if layout == "compact" else IC.planes
    F, V = make(IC.mixed_specs(31, True)), make(IC.mixed_specs(32, False))
    joint, dist = run_fwd(hp, F)
    check_fwd(F, joint, dist, layout)
    rng = np.random.default_rng(5)
    jblocks = [rng.integers(-32768, 32768, (int(it["height"]), int(it["width"]))).astype(np.int16) if k % 3 else rng.integers(-600, 601, (int(it["height"]), int(it["width"]))).astype(np.int16)
               for k, it in enumerate(V.items)]
    jrec = joint_buffer(V, jblocks)
    rec, sse = run_inv(hp, V, jrec)
    check_inv(V, jblocks, rec, sse, layout)
    # shuffled: the same results per item (the outputs are addressed by the items, the sums by the list position)
    for order in (rng.permutation(len(F.items)), np.arange(len(F.items))[::-1]):
        j2, d2 = run_fwd(hp, F.reordered(order))
        assert np.array_equal(j2, joint) and np.array_equal(d2, dist[order])
    order = rng.permutation(len(V.items))
    r2, s2 = run_inv(hp, V.reordered(order), jrec)
    assert np.array_equal(r2, rec) and np.array_equal(s2, sse[order])
    # without the optional outputs
    j3, _ = run_fwd(hp, F, want_dist=False)
    assert np.array_equal(j3, joint)
    r3, _ = run_inv(hp, V, jrec, want_sse=False)
    assert np.array_equal(r3, rec)
    _, s3 = run_inv(hp, V, jrec, want_rec=False)
    assert np.array_equal(s3, sse)
    # the schedule cache: the same lists again upload and allocate nothing
    d_resi, d_vresi, d_jrec = dev16(hp, F.resi), dev16(hp, V.resi), dev16(hp, jrec)
    o_joint = torch.full((F.joint_total,), SENTINEL, dtype=torch.int16, device=hp.device)
    o_dist = torch.zeros((len(F.items), 2), dtype=torch.int64, device=hp.device)
    o_rec = torch.full((V.resi.size,), SENTINEL, dtype=torch.int16, device=hp.device)
    o_sse = torch.zeros((len(V.items), 2), dtype=torch.int64, device=hp.device)
    hp.ict_fwd_batch(d_resi, F.items, o_joint, o_dist)
    hp.ict_inv_batch(d_jrec, V.items, None, o_rec, d_vresi, o_sse)
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info()[0]
    for _ in range(3):
        hp.ict_fwd_batch(d_resi, F.items, o_joint, o_dist)
        hp.ict_inv_batch(d_jrec, V.items, None, o_rec, d_vresi, o_sse)
    torch.cuda.synchronize()
    assert torch.cuda.mem_get_info()[0] == free0
    assert np.array_equal(o_joint.cpu().numpy(), joint) and np.array_equal(o_dist.cpu().numpy(), dist)
    assert np.array_equal(o_rec.cpu().numpy(), rec) and np.array_equal(o_sse.cpu().numpy().view(np.uint64), sse)


# ---- 4 ----
def test_zero_shortcut(hp):
    """items whose statistics entry has abs_sum == 0 reconstruct to zero and score the energy of the original residual although their joint reconstruction holds a
    sentinel; items with abs_sum != 0 or without an entry in the same list read their block (one of them a block of sentinels: it IS read)"""
    from vvenc_amd.hotpath import STATS_DTYPE
    L = IC.compact(IC.mixed_specs(33, False, n=90))
    n = len(L.items)
    rng = np.random.default_rng(9)
    perm = rng.permutation(n)
    stats = np.zeros(n + 3, STATS_DTYPE)
    stats["abs_sum"] = 1 << 20          # (entries no item names)
    jblocks, zero = [], []
    for i in range(n):
        kind = i % 3          # 0: abs_sum == 0, 1: abs_sum != 0, 2: no entry
        L.items[i]["stats_idx"] = -1 if kind == 2 else int(perm[i])
        if kind != 2:
            stats[perm[i]]["abs_sum"] = 0 if kind == 0 else 1 + i
        zero.append(kind == 0)
        h, w = int(L.items[i]["height"]), int(L.items[i]["width"])
        jblocks.append(np.full((h, w), SENTINEL, np.int16) if kind == 0 or i == 1 else rng.integers(-2000, 2001, (h, w)).astype(np.int16))
    rec, sse = run_inv(hp, L, joint_buffer(L, jblocks), hp.to_device(stats))
    seen = [np.zeros_like(b) if z else b for b, z in zip(jblocks, zero)]
    check_inv(L, seen, rec, sse, "zero shortcut")
    for i in range(n):
        if zero[i]:
            assert not L.cb(rec, i).any() and not L.cr(rec, i).any() and (int(sse[i][0]), int(sse[i][1])) == (IR.sse(L.blocks[i][0], 0), IR.sse(L.blocks[i][1], 0))
    assert L.cb(rec, 1).any() and sum(zero) >= 25


# ---- 5 ----
@pytest.mark.parametrize("sparse", [0, 1])
@pytest.mark.parametrize("qp", IC.CHAIN_QPS)
def test_chain_from_the_prediction_list(hp, oracle, qp, sparse):
    """pred_inter_batch with the residual on the Cb and Cr blocks of 4x4, 8x8 and 16x8 chroma TUs -> tu_rdo_joint (forward, the fused TU pipeline on the joint buffer,
    inverse) against the model around the oracle's TU pipeline, sparse outputs off and on.  At QP 45 some joint TUs quantise to zero and some do not (asserted)."""
    import torch
    from vvenc_amd.hotpath import STATS_DTYPE
    w = IC.chain_world()
    exp = IC.chain_expected(oracle, w, qp)
    dev = [hp.plane(a, 0) for a in w["planes"]]
    org = hp.plane(w["org"], 0)
    assert all(p.stride == a.shape[1] for p, a in zip(dev + [org], w["planes"] + [w["org"]]))
    pred, resi = (torch.full((w["resi_total"],), SENTINEL, dtype=torch.int16, device=hp.device) for _ in range(2))
    hp.pred_inter_batch(dev, w["pred_items"], pred, 0, w["bd"], org, resi)
    from vvenc_amd.hotpath import make_ict_items
    items, total = make_ict_items([(int(i["cb_off"]), int(i["cr_off"]), int(i["stride"]), int(i["width"]), int(i["height"]), int(i["mode"])) for i in w["ict_items"]])
    items, jobs, strides, level, joint_rec, stats = hp.make_joint_tu_jobs(items, qp)
    level.fill_(SENTINEL); joint_rec.fill_(SENTINEL)
    rec = torch.full_like(resi, SENTINEL)
    try:
        hp.tu_set_sparse_outputs(sparse)
        joint, dist, rec, sse = hp.tu_rdo_joint(resi, items, jobs, strides, joint_rec, stats, w["bd"], rec=rec)
        torch.cuda.synchronize()
    finally:
        hp.tu_set_sparse_outputs(0)
    resi_np, joint, dist, rec, sse = resi.cpu().numpy(), joint.cpu().numpy(), dist.cpu().numpy(), rec.cpu().numpy(), sse.cpu().numpy().view(np.uint64)
    level, joint_rec, st = level.cpu().numpy(), joint_rec.cpu().numpy(), stats.cpu().numpy().view(STATS_DTYPE).reshape(-1)
    L = IC.Listed(items, resi_np, [(e["cb"], e["cr"]) for e in exp], total)
    n_zero = 0
    for i, e in enumerate(exp):
        what = (qp, sparse, i, items[i])
        assert np.array_equal(L.cb(resi_np, i), e["cb"]) and np.array_equal(L.cr(resi_np, i), e["cr"]), ("residual",) + what
        assert np.array_equal(L.joint(joint, i), e["joint"]) and (int(dist[i][0]), int(dist[i][1])) == e["dist"], ("forward",) + what
        s = st[int(items[i]["stats_idx"])]
        assert (int(s["abs_sum"]), int(s["last_scan_pos"]), int(s["need_rdoq"]), int(s["sse"])) == tuple(e["stats"][k] for k in ("abs_sum", "last_scan_pos", "need_rdoq", "sse")), ("stats",) + what
        if e["stats"]["abs_sum"] or not sparse:
            assert np.array_equal(L.joint(level, i), e["level"]) and np.array_equal(L.joint(joint_rec, i), e["joint_rec"]), ("levels / joint reconstruction",) + what
        n_zero += e["stats"]["abs_sum"] == 0
        assert np.array_equal(L.cb(rec, i), e["rec_cb"]) and np.array_equal(L.cr(rec, i), e["rec_cr"]), ("reconstruction",) + what
        assert (int(sse[i][0]), int(sse[i][1])) == e["sse"], ("sse",) + what
    assert (rec[~L.block_mask()] == SENTINEL).all()
    if qp == 45:
        assert 0 < n_zero < len(exp)


# ---- 6 ----
def test_argument_errors(hp):
    """every argument error returns VVHIP_E_ARG with the entry's name in the message, launches nothing and leaves the outputs untouched and the context usable"""
    import torch
    from vvenc_amd.hotpath import STATS_DTYPE
    from vvenc_amd.lib import VVHipError
    rng = np.random.default_rng(3)
    specs = [(m, rng.integers(-500, 501, (4, 8)).astype(np.int16), rng.integers(-500, 501, (4, 8)).astype(np.int16)) for m in (1, -2, 3)]
    L = IC.compact(specs)
    d_resi, d_jrec = dev16(hp, L.resi), dev16(hp, rng.integers(-500, 501, L.joint_total))
    d_stats = hp.to_device(np.zeros(4, STATS_DTYPE))

    def broken(**changes):
        it = L.items.copy()
        for f, v in changes.items():
            it[1][f] = v
        return it
    bad = [broken(width=6), broken(height=128), broken(width=1), broken(stride=4), broken(cb_off=-2), broken(cr_off=-1), broken(joint_off=-8), broken(mode=4), broken(mode=-4),
           broken(rsv=(0, 1, 0))]
    for entry in ("fwd", "inv"):
        name = "vvhip_ict_%s_batch" % entry
        cases = [(it, {}) for it in bad]
        if entry == "fwd":
            cases += [(L.items, dict(no_resi=True)), (L.items, dict(no_joint=True))]
        else:
            cases += [(broken(mode=0), {}), (L.items, dict(no_jrec=True)), (L.items, dict(no_org=True)), (broken(stats_idx=2), dict(no_stats=True))]
        for k, (it, opt) in enumerate(cases):
            joint = torch.full((L.joint_total,), SENTINEL, dtype=torch.int16, device=hp.device)
            rec = torch.full((L.resi.size,), SENTINEL, dtype=torch.int16, device=hp.device)
            sums = torch.full((3, 2), SENT64, dtype=torch.int64, device=hp.device)
            with pytest.raises(VVHipError) as e:
                if entry == "fwd":
                    hp.ict_fwd_batch(None if opt.get("no_resi") else d_resi, it, None if opt.get("no_joint") else joint, sums)
                else:
                    hp.ict_inv_batch(None if opt.get("no_jrec") else d_jrec, it, None if opt.get("no_stats") else d_stats, rec, None if opt.get("no_org") else d_resi, sums)
            assert name in str(e.value) and "error -1" in str(e.value), (entry, k, str(e.value))
            torch.cuda.synchronize()
            assert (joint.cpu().numpy() == SENTINEL).all() and (rec.cpu().numpy() == SENTINEL).all() and (sums.cpu().numpy() == SENT64).all(), (entry, k)
        # n < 0
        rc = getattr(hp.L, name)(hp.ctx, *([None] * 2), -1, *([None] * (2 if entry == "fwd" else 4)))
        assert rc == -1 and name in hp.L.vvhip_last_error(hp.ctx).decode()
    # an empty list is no error, a forward list of mode 0 needs no joint buffer, and the context still works
    hp.ict_fwd_batch(d_resi, L.items[:0], None, None)
    zero = L.items.copy()
    zero["mode"] = 0
    _, d0 = run_fwd(hp, IC.Listed(zero, L.resi, L.blocks, 0))
    assert [tuple(int(v) for v in r) for r in d0] == [(IR.sse(cb, 0), IR.sse(cr, 0)) for (cb, cr) in L.blocks]
    joint, dist = run_fwd(hp, L)
    check_fwd(L, joint, dist, "after the errors")


# ---- 7 ----
def test_alternating_with_the_prediction_list_keeps_both_schedules(hp):
    """the joint entries and vvhip_pred_inter_batch alternating on one context: every output stays what it was and nothing is allocated on the device"""
    import torch
    pl, org_np = BLC.planes(10, 110)
    dev = [hp.plane(a, 0) for a in pl]
    pitems = BLC.bcw_list(pl, 300)[0][:9].copy()
    pitems["dst_off"], ptot = BLC.compact_offsets(pitems)
    F = IC.compact(IC.mixed_specs(34, False, n=60))
    rng = np.random.default_rng(11)
    jrec = joint_buffer(F, [rng.integers(-900, 901, (int(it["height"]), int(it["width"]))).astype(np.int16) for it in F.items])
    d_resi, d_jrec = dev16(hp, F.resi), dev16(hp, jrec)
    o_pred = torch.empty((ptot,), dtype=torch.int16, device=hp.device)
    o_joint = torch.empty((F.joint_total,), dtype=torch.int16, device=hp.device)
    o_rec = torch.empty((F.resi.size,), dtype=torch.int16, device=hp.device)
    o_dist, o_sse = (torch.empty((len(F.items), 2), dtype=torch.int64, device=hp.device) for _ in range(2))
    first, free1 = None, None
    for rnd in range(3):
        for t in (o_pred, o_joint, o_rec):
            t.fill_(SENTINEL)
        hp.pred_inter_batch(dev, pitems, o_pred, 0, 10)
        hp.ict_fwd_batch(d_resi, F.items, o_joint, o_dist)
        hp.ict_inv_batch(d_jrec, F.items, None, o_rec, d_resi, o_sse)
        torch.cuda.synchronize()
        got = [t.cpu().numpy().copy() for t in (o_pred, o_joint, o_dist, o_rec, o_sse)]
        if rnd == 0:
            first, free1 = got, torch.cuda.mem_get_info()[0]
            check_fwd(F, got[1], got[2], "alternating")
            assert got[0].min() >= 0
        else:
            assert all(np.array_equal(a, b) for a, b in zip(got, first)), rnd
            assert torch.cuda.mem_get_info()[0] == free1, rnd
