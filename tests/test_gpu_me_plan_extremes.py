"""-m gpu: the motion-search plans of vvenc_amd/csrc/me.hip (vvhip_me_plan_create / _create_lists / _run / _run_parts / _info) on the deterministic limit cases of
tests/me_plan_extremes.py — window geometry (A), candidate lists (B), window launches (C), stage positions and schedule (D), items (E), operands of integer windows (F),
plan lifecycle (G) and the environment knobs said to leave results identical (H).

Every expected cost is one call of the oracle (dist, if_pred_luma_me, sad_mask), never a model and never another HIP kernel; tolerance 0.  For every plan:
  * vvhip_me_plan_info's waves_int, waves_stage, waves_item and LDS bytes equal schedule_model's prediction — a case that no longer reaches the edge it is named for
    fails here (tests/test_me_plan_extremes_cpu.py asserts, from the same model, that every named edge is reached);
  * the three cost arrays are pre-filled with a sentinel and sit between guard entries, which must come back intact; every cost of the case is compared and their number
    equals the number the builder produced;
  * every input plane is read back and compared with what was uploaded.

Measured on an MI355X, on the tests as they stand: the file 8.6 s (30 tests), of which 4.6 s are the two child processes of the knob test and 1.6 s the device context;
the two plans of 131 073 items 0.36 s each, the plans of 8 195 stages 0.25 s each, every other test 0.28 s and less (66 plans, 446 864 costs).  docs/ROUND_NOTES.md,
"Motion-search plan limits", lists every test function.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import me_plan_extremes as M

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

GUARD = 8
SENT = 0x5A5A5A5A5A5A5A5A


@pytest.fixture(scope="module")
def env():
    from vvenc_amd.hotpath import HotPath
    from oracle.oracle import Oracle
    return HotPath(), Oracle(), {}


class Dev:
    """a plan case on the device: its planes uploaded as they are (margins included), the plane table of a run"""

    def __init__(self, hp, plan):
        import torch
        from vvenc_amd import replay as RP
        self.plan, self.hp = plan, hp
        self.t, up = [], {}
        for arr, pad in plan.planes:
            if id(arr) not in up:
                up[id(arr)] = torch.from_numpy(arr).to(hp.device)
            self.t.append(up[id(arr)])
        self.tab = (RP.MePlane * 16)()
        for k, ((arr, pad), t) in enumerate(zip(plan.planes, self.t)):
            if pad is None:
                self.tab[k] = RP.MePlane(t.data_ptr(), 0, 0)
            else:
                self.tab[k] = RP.MePlane(t.data_ptr() + 2 * (pad * arr.shape[1] + pad), arr.shape[1], 0)
        self.n_planes = len(plan.planes)

    def held(self):
        import torch
        return [torch.full((n + 2 * GUARD,), SENT, dtype=torch.int64, device=self.hp.device) for n in self.plan.counts()]

    def create(self):
        p = self.plan
        return self.hp.me_plan_create(p.ij, p.cands, p.sj, p.items, p.bd, p.max_window, mask_items=p.mask_items)

    def run(self, handle, held, parts=7):
        args = [h[GUARD:h.numel() - GUARD] for h in held]
        if parts == 7:
            self.hp.me_plan_run(handle, self.tab, self.n_planes, *args)
        else:
            self.hp.me_plan_run_parts(handle, self.tab, self.n_planes, *args, parts)

    def read(self, held):
        import torch
        torch.cuda.synchronize()
        out = []
        for h, what in zip(held, ("candidate", "stage", "item")):
            a = h.cpu().numpy()
            assert (a[:GUARD] == SENT).all() and (a[a.size - GUARD:] == SENT).all(), (self.plan.name, "an entry outside the %s costs was written" % what)
            out.append(a[GUARD:a.size - GUARD])
        return out

    def planes_unchanged(self):
        for (arr, pad), t in zip(self.plan.planes, self.t):
            assert np.array_equal(t.cpu().numpy(), arr), (self.plan.name, "an input plane was written")


def check_info(hp, handle, plan):
    info, x = hp.me_plan_info(handle), plan.model()
    assert (info["waves_int"], info["waves_stage"], info["waves_item"], info["lds_bytes"]) == (x["waves_int"], x["waves_stage"], x["waves_item"], x["lds_bytes"]), (plan.name, info)
    return x


def compare(plan, got, exp):
    n = 0
    for g, e, what in zip(got, (exp[0], exp[1].reshape(-1), exp[2]), ("candidate", "stage", "item")):
        assert g.size == e.size
        bad = np.nonzero(g != e)[0]
        assert bad.size == 0, (plan.name, what, int(bad.size), [(int(k), int(g[k]), int(e[k])) for k in bad[:6]])
        n += g.size
    assert n == sum(plan.counts())
    return n


def run_case(env, plan):
    hp, orc, memo = env
    dv = Dev(hp, plan)
    handle = dv.create()
    try:
        check_info(hp, handle, plan)
        held = dv.held()
        dv.run(handle, held)
        got = dv.read(held)
    finally:
        hp.me_plan_destroy(handle)
    n = compare(plan, got, M.expected(plan, orc, memo))
    dv.planes_unchanged()
    return n


# ---- A, B, C, F: integer windows -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", range(6), ids=["mw0", "mw1", "mw8", "mw16", "mw24", "mw40"])
def test_window_geometry(env, k):
    plan = M.family_a()[k]
    assert run_case(env, plan) == plan.cands.size > 0


def test_candidate_lists(env):
    for plan in M.family_b():
        assert run_case(env, plan) == plan.cands.size > 1500


def test_window_launches(env):
    plans = M.family_c()
    assert len(plans) == 18
    for plan in plans:
        run_case(env, plan)


@pytest.mark.parametrize("k", range(3), ids=["samples", "biprediction", "int16"])
def test_integer_window_operands(env, k):
    plan = M.family_f()[k]
    assert run_case(env, plan) == 60


# ---- D: stages -------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bd", [10, 8])
def test_stage_position_sweep(env, bd):
    plan = M.family_d_sweep(bd)
    assert run_case(env, plan) == 9 * 6 * 2 * 49


@pytest.mark.parametrize("bd", [10, 8])
def test_stage_tile_kinds_and_deals(env, bd):
    plan = M.family_d_shapes(bd)
    assert run_case(env, plan) == 9 * (11 * len(M.D_SHAPES) + 3) + 12


@pytest.mark.parametrize("bd", [10, 8])
def test_stage_bundles(env, bd):
    plans = M.family_d_bundles(bd)
    assert len(plans) == 9
    for plan in plans:
        run_case(env, plan)


@pytest.mark.parametrize("bd", [10, 8])
def test_stage_unsplit_path(env, bd):
    """at least 8 192 units: a wide unit's horizontal variants stay in one wave — the wide stages' costs equal the oracle's and those of the same records in a small plan"""
    hp, orc, memo = env
    long_p, small_p, n = M.family_d_unsplit(bd)
    got = {}
    for plan in (long_p, small_p):
        dv = Dev(hp, plan)
        handle = dv.create()
        try:
            check_info(hp, handle, plan)
            held = dv.held()
            dv.run(handle, held)
            got[plan.name] = dv.read(held)
        finally:
            hp.me_plan_destroy(handle)
        compare(plan, got[plan.name], M.expected(plan, orc, memo))
        dv.planes_unchanged()
    assert np.array_equal(got[long_p.name][1][-9 * n:], got[small_p.name][1]) and (got[small_p.name][1] > 0).all()


# ---- E: items --------------------------------------------------------------------------------------------------------------------------------------------
def test_item_runs_at_the_wave_size(env):
    plans = M.family_e_runs()
    assert len(plans) == 4
    for plan in plans:
        run_case(env, plan)


def test_item_classes(env):
    plans = M.family_e_classes()
    assert len(plans) == 5
    for plan in plans:
        run_case(env, plan)


@pytest.mark.parametrize("k", range(2), ids=["lean65536-generic65537", "lean65537-generic65536"])
def test_item_launches_beyond_65536_waves(env, k):
    plan = M.family_e_long()[k]
    assert run_case(env, plan) == 2 * 65536 + 1


# ---- G: lifecycle ----------------------------------------------------------------------------------------------------------------------------------------
def test_empty_plan_creates_runs_and_destroys(env):
    hp = env[0]
    plan = M.Plan("G empty", 10, 0)
    plan.plane(M.a_planes()[0], M.A_PAD)
    dv = Dev(hp, plan)
    handle = dv.create()
    info = hp.me_plan_info(handle)
    assert (info["waves_int"], info["waves_stage"], info["waves_item"]) == (0, 0, 0)
    held = dv.held()
    dv.run(handle, held)
    for parts in (1, 2, 4):
        dv.run(handle, held, parts)
    assert all(g.size == 0 for g in dv.read(held))
    hp.me_plan_destroy(handle)


def test_three_runs_into_the_same_buffers(env):
    """the atomic stages add into the cost array: every run clears it first"""
    hp, orc, memo = env
    plan = M.compact_plan()
    assert "atomic_clear" in plan.model()["edges"]
    exp = M.expected(plan, orc, memo)
    dv = Dev(hp, plan)
    handle = dv.create()
    check_info(hp, handle, plan)
    held = dv.held()
    for _ in range(3):
        dv.run(handle, held)
        compare(plan, dv.read(held), exp)
    hp.me_plan_destroy(handle)
    dv.planes_unchanged()


def test_run_parts(env):
    """each part alone writes its own cost array and leaves the other two at the sentinel; the three parts in any order equal one full run"""
    import itertools
    hp, orc, memo = env
    plan = M.compact_plan()
    exp = M.expected(plan, orc, memo)
    dv = Dev(hp, plan)
    handle = dv.create()
    check_info(hp, handle, plan)
    for parts, mine in ((1, 1), (2, 0), (4, 2)):               # bit 0: stages, bit 1: integer windows, bit 2: table calls
        held = dv.held()
        dv.run(handle, held, parts)
        got = dv.read(held)
        for k in range(3):
            if k == mine:
                assert np.array_equal(got[k], (exp[0], exp[1].reshape(-1), exp[2])[k]), (parts, k)
            else:
                assert got[k].size and (got[k] == SENT).all(), (parts, k)
    for order in itertools.permutations((1, 2, 4)):
        held = dv.held()
        for parts in order:
            dv.run(handle, held, parts)
        compare(plan, dv.read(held), exp)
    for pair in ((3, 4), (5, 2), (6, 1)):
        held = dv.held()
        for parts in pair:
            dv.run(handle, held, parts)
        compare(plan, dv.read(held), exp)
    hp.me_plan_destroy(handle)
    dv.planes_unchanged()


def test_two_plans_alive_at_once(env):
    hp, orc, memo = env
    pa, pb = M.compact_plan(), M.family_d_shapes(10)
    ea, eb = M.expected(pa, orc, memo), M.expected(pb, orc, memo)
    da, db = Dev(hp, pa), Dev(hp, pb)
    ha, hb = da.create(), db.create()
    check_info(hp, ha, pa)
    check_info(hp, hb, pb)
    held_a, held_b = da.held(), db.held()
    for _ in range(2):
        da.run(ha, held_a)
        db.run(hb, held_b)
    compare(pa, da.read(held_a), ea)
    compare(pb, db.read(held_b), eb)
    hp.me_plan_destroy(ha)
    db.run(hb, held_b)                                         # the other plan outlives it
    compare(pb, db.read(held_b), eb)
    hp.me_plan_destroy(hb)


def test_rejections_leave_the_context_usable(env):
    from vvenc_amd.lib import VVHipError
    hp, orc, memo = env
    plan = M.compact_plan()
    for bd in (11, 12):
        with pytest.raises(VVHipError) as e:
            hp.me_plan_create(plan.ij, plan.cands, plan.sj, plan.items, bd, 0, mask_items=plan.mask_items)
        assert "bit depth" in str(e.value)
    # a max_window whose window exceeds 160 KB: a 64x64 block with candidates 250 samples apart both ways (314 rows of 318 samples + the block: 203 KB)
    big = M.Plan("G window beyond 160 KB", 10, 250)
    org, ref, _ = M.a_planes()
    big.plane(org, M.A_PAD); big.plane(ref, M.A_PAD)
    big.int_job(0, big.off(0, 8, 8), 1, 8, 8, 64, 64, 0, [(0, 0), (250, 250)])
    assert big.model()["lds_int"] > 160 * 1024
    with pytest.raises(VVHipError) as e:
        hp.me_plan_create(big.ij, big.cands, big.sj, big.items, 10, 250)
    assert "LDS" in str(e.value)
    assert run_case(env, plan) == sum(plan.counts())           # the same context still creates and runs a valid plan


# ---- H: knobs --------------------------------------------------------------------------------------------------------------------------------------------
CHILD = """
import json, sys
sys.path.insert(0, %r); sys.path.insert(0, %r)
import numpy as np, torch
import me_plan_extremes as M
import test_gpu_me_plan_extremes as T
from vvenc_amd.hotpath import HotPath
hp = HotPath()
exp = np.load(%r)
model_knobs, with_long = json.loads(%r), %r
bad = n = 0
info_ok = True
for tag, plan in [("", M.compact_plan())] + ([("long_", M.family_e_long()[0])] if with_long else []):
    dv = T.Dev(hp, plan)
    handle = dv.create()
    info, x = hp.me_plan_info(handle), plan.model(**model_knobs)
    info_ok = info_ok and (info["waves_int"], info["waves_stage"], info["waves_item"], info["lds_bytes"]) == (x["waves_int"], x["waves_stage"], x["waves_item"], x["lds_bytes"])
    held = dv.held()
    dv.run(handle, held)
    got = dv.read(held)
    hp.me_plan_destroy(handle)
    dv.planes_unchanged()
    bad += sum(int((g != exp[tag + k]).sum()) for g, k in zip(got, ("c", "s", "i")))
    n += sum(g.size for g in got)
    assert sum(g.size for g in got) == sum(plan.counts())
print(json.dumps({"bad": bad, "n": n, "info_ok": bool(info_ok)}))
sys.exit(0 if bad == 0 and info_ok else 1)
"""

# (environment of the child, the same knobs as schedule_model's arguments, whether the child also runs a plan of more than 65 536 waves per launch)
# VVHIP_ME_XCD_BAND, _ITEM_INTERLEAVE and _ITEM_SPANS reorder workgroups or regroup spans per wave: they change no count of vvhip_me_plan_info — their check is the
# costs alone; _ITEM_SPANS is read only by launches of more than 65 536 waves, which is why the second child runs the long plan as well
KNOBS = [(dict(VVHIP_ME_XCD_BAND="0", VVHIP_ME_ATOMIC_STAGES="0", VVHIP_ME_DEDUPE="0", VVHIP_ME_SPLIT_VARIANTS="0"), dict(band=False, atomic_stages=False, dedupe=False, split_below=0), False),
         (dict(VVHIP_ME_ITEM_INTERLEAVE="4", VVHIP_ME_CAND_CAP="64", VVHIP_ME_BUNDLE_WORK="320", VVHIP_ME_ITEM_SPANS="3"), dict(cand_cap=64, bundle_work=320), True)]


def test_knobs_leave_results_identical(env, tmp_path):
    """two fresh processes, one after the other, each with four of the VVHIP_ME_* knobs: the compact plan's costs (in the second child also those of a plan with 65 536 lean
    and 65 537 generic waves) equal the values this process took from the oracle, and vvhip_me_plan_info equals the model WITH the knobs — which differs from the model
    without them, so every knob that changes a count is shown to have been honoured"""
    hp, orc, memo = env
    plan, long_plan = M.compact_plan(), M.family_e_long()[0]
    x = plan.model()
    assert x["waves_item_lean"] > 64 and {"dedupe_fold", "split_by_cap", "deal_atomic", "deal_shared", "deal_single", "variants_split"} <= x["edges"]
    key = lambda m: (m["waves_int"], m["waves_stage"], m["waves_item"], m["lds_bytes"])
    for kn in (dict(atomic_stages=False), dict(dedupe=False), dict(split_below=0), dict(cand_cap=64), dict(bundle_work=320)):
        assert key(plan.model(**kn)) != key(x), kn
    cc, sc, ic = M.expected(plan, orc, memo)
    lc, ls, li = M.expected(long_plan, orc, memo)
    path = str(tmp_path / "expected.npz")
    np.savez(path, c=cc, s=sc.reshape(-1), i=ic, long_c=lc, long_s=ls.reshape(-1), long_i=li)
    for env_knobs, model_knobs, with_long in KNOBS:
        code = CHILD % (ROOT, os.path.join(ROOT, "tests"), path, json.dumps(model_knobs), with_long)
        r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300, env=dict(os.environ, **env_knobs))
        assert r.returncode == 0, (env_knobs, r.stdout[-500:], r.stderr[-2000:])
        out = json.loads(r.stdout.strip().splitlines()[-1])
        assert out == {"bad": 0, "n": sum(plan.counts()) + (sum(long_plan.counts()) if with_long else 0), "info_ok": True}, (env_knobs, out)


def test_every_plan_of_the_families_has_its_test():
    """no case is skipped: every test above walks the whole list its builder returns and asserts the number of costs it compared; this one asserts that the builders the
    tests use are all there are (no state shared with the other tests: it holds for any selection or order)"""
    used = (M.family_a() + M.family_b() + M.family_c() + M.family_f() + [M.family_d_sweep(10), M.family_d_sweep(8), M.family_d_shapes(10), M.family_d_shapes(8)] + M.family_d_bundles(10) + M.family_d_bundles(8) +
            list(M.family_d_unsplit(10)[:2]) + list(M.family_d_unsplit(8)[:2]) + M.family_e_runs() + M.family_e_classes() + M.family_e_long() + [M.compact_plan()])
    every = M.all_plans() + M.long_plans()
    assert sorted(p.name for p in used) == sorted(p.name for p in every) and len({p.name for p in every}) == len(every) == 66
    print("plans: %d, costs compared with the oracle: %d" % (len(every), sum(sum(p.counts()) for p in every)))
