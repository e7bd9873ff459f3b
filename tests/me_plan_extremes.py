"""Deterministic limit cases for the motion-search plans of vvenc_amd/csrc/me.hip (vvhip_me_plan_create / _run / _run_parts), and two models of what the plans do with them.
numpy only: no device, no oracle import (the tests hand an oracle to `expected`).

A *plan case* (class Plan) is everything one vvhip_me_plan_create call takes: the plane table (every plane as the FULL numpy array with its margin, sample (0, 0) at
[pad, pad]; a pool of compact blocks is a 1-D array with stride 0), the five job arrays in the dtypes of vvenc_amd/replay.py, bit_depth and max_window, a name that says
which edge the case is for.  `expected(plan, oracle)` gives every cost of the case from the oracle's dist / if_pred_luma_me / sad_mask and nothing else.

`schedule_model` restates the COUNTING rules of the host scheduler (mePlanCreate and the launch choices of mePlanRun) in one place: windows per integer job with their
(minDx, minDy, winW, winH, nCand), LDS bytes and class per window, the window launches, units / deal / variant count per stage and the stage waves, the item waves lean /
generic / masked — and the set of named edges (REQUIRED) the lists reached.  A change of the scheduler changes this one function.  The GPU tier compares it with
vvhip_me_plan_info on every plan, so a case that no longer reaches its edge fails instead of passing for nothing.

`window_model` restates intBody's ADDRESSING in int64 (the sums need no bias there): the LDS row pitch (an odd number of dwords), 16-byte chunks per row with the last one
cut at the pitch, the even / odd halves of a window under sub_shift 1, odd displacements as the even dword below plus a funnel shift.  It is used by the sensitivity test
of the CPU tier only — never as an expected value.  Its four mutations break the STAGING side the way a one-line slip in
the kernel would.  The fifth mutation of the sensitivity test, the extent compared with < instead of <=, is a slip of the host's clustering: it changes no cost (a correct
kernel scores whatever windows it is given), it changes the NUMBER of windows — schedule_model(extent_lt=True), which is what the device tier's comparison with
vvhip_me_plan_info notices.

Families (the issue's letters): A window geometry, B candidate lists, C window launches, D stage positions and schedule, E items, F operands of integer windows,
G lifecycle and H knobs (the compact plan).  Facts the cases rest on:
  * a window row is fetched as ( winW + 2 + 7 ) >> 3 chunks of 16 bytes from its first sample: up to 9 samples (18 bytes) beyond the row's winW samples
    (winW = 7 mod 8) — the margin include/vvenc_hip.h states;
  * unit work ( positions x max( 1, unit width / 8 ) x unit height ) is a multiple of 4 for every legal shape, so the sums next to the bundle budget of 80 row groups
    are 76, 80 and 84 — 79 and 81 do not exist;
  * integer windows are exact for ANY int16 operands: both are XORed with 0x8000 per sample ( = + 32768 as uint16 ), v_sad_u16 adds |a - b| of the unsigned halves into
    32 bits, and 128 * 128 * 65535 < 2^32.
"""
import numpy as np


class _Dtypes:
    """the record dtypes of vvenc_amd/replay.py, imported when the first array is built (that module brings torch along)"""

    def __getattr__(self, name):
        from vvenc_amd import replay
        return getattr(replay, name)


RP = _Dtypes()

DF = {"SSE": 0, "SAD": 1, "HAD": 2, "HAD_fast": 3, "HAD_2SAD": 4}
DF_NAME = {v: k for k, v in DF.items()}
REFINE_X = (0, 0, 0, -1, 1, -1, 1, -1, 1)
REFINE_YH = (0, -1, 1, 0, 0, -1, -1, 1, 1)
REFINE_YQ = (0, -1, 1, -1, -1, 0, 0, 1, 1)
ROW_SLACK = 9                                  # samples a window row is read beyond its winW samples, at most

REQUIRED = (
    # A / B: clustering
    "reach_default_24", "reach_forced_16", "extent_eq_reach_x", "extent_eq_reach_y", "split_by_reach", "split_by_cap", "cand_cap_full", "dedupe_fold", "dedupe_team_full",
    "job_without_candidates", "max_window_1", "max_window_40",
    # A: LDS layout
    "minDx_even", "minDx_odd", "x_even_extreme", "x_odd_extreme", "winH_even_ss1", "winH_odd_ss1", "dy_even_extreme_ss1", "dy_odd_extreme_ss1", "last_chunk_cut", "org_beyond_4_chunks",
    "negative_displacement", "read_at_plane_start", "read_at_plane_end",
    # C: launches
    "lds_small", "lds_mid", "lds_large", "lds_over_64k", "launch_single", "launch_split_large", "launch_split_small", "launch_three", "small_group_short", "small_groups_banded",
    # D: stages
    "deal_single", "deal_shared", "deal_atomic", "variants_split", "variants_unsplit", "bundle_cap_8", "bundle_work_at_80", "bundle_work_over_80", "tap_reload", "atomic_clear",
    "odd_class_then_shared", "stage_org_pool", "int_org_pool", "stage_disp_pm16", "stage_mask_empty",
    # E: items
    "item_lean", "item_generic", "item_masked", "item_wave_full", "item_wave_partial", "item_band_order", "item_long_lean", "item_long_generic", "item_sorted", "plane_15",
)


# ---------------------------------------------------------------------------------------------------------------------------------------------------------
# plan cases
# ---------------------------------------------------------------------------------------------------------------------------------------------------------
class Plan:
    def __init__(self, name, bd=10, max_window=0):
        self.name, self.bd, self.max_window = name, bd, max_window
        self.planes = []                        # (full array, pad); pad None: a pool (1-D, stride 0)
        self._ij, self._c, self._sj, self._it, self._mk = [], [], [], [], []
        self.edges = set()                      # edges the builder vouches for itself (the model adds what it can see)
        self._cache = {}

    def plane(self, arr, pad):
        assert arr.dtype == np.int16 and arr.ndim == 2 and arr.flags["C_CONTIGUOUS"]
        self.planes.append((arr, pad))
        return len(self.planes) - 1

    def pool(self, arr):
        assert arr.dtype == np.int16 and arr.ndim == 1
        self.planes.append((arr, None))
        return len(self.planes) - 1

    def stride(self, p):
        arr, pad = self.planes[p]
        return 0 if pad is None else arr.shape[1]

    def off(self, p, x, y):
        return y * self.stride(p) + x

    def int_job(self, op, oo, rp, rx, ry, w, h, ss, cand_list, first=None):
        """oo: the original block's offset (a sample offset in a plane, an element offset in a pool); first: reuse candidates that are already in the list"""
        if first is None:
            first = len(self._c)
            self._c.extend((int(a), int(b)) for a, b in cand_list)
        self._ij.append((oo, self.off(rp, rx, ry), w, h, op, rp, ss, 0, 0, 0, 0, 0, first, len(cand_list)))

    def stage(self, op, oo, rp, rx, ry, w, h, i_frac, mode, alt, func, bq, mask):
        self._sj.append((oo, self.off(rp, rx, ry), w, h, op, rp, i_frac, mode, alt, DF[func], bq[0], bq[1], mask, 0))

    def item(self, op, oo, cp, co, func, ss, w, h):
        self._it.append((oo, co, op, cp, DF[func], ss, w, h))

    def mask_item(self, op, oo, cp, co, mp, mo, ss, w, h):
        self._mk.append((oo, co, mo, op, cp, mp, ss, w, h, 0))

    def _arr(self, lst, dt):
        # (the arrays are built once per list length: the long plans hold 131 073 items)
        if self._cache.get(id(lst), (None, None))[0] != len(lst):
            self._cache[id(lst)] = (len(lst), np.array(lst, dt) if lst else np.zeros(0, dt))
        return self._cache[id(lst)][1]

    @property
    def ij(self): return self._arr(self._ij, RP.ME_INT_JOB)
    @property
    def cands(self): return self._arr(self._c, RP.ME_CAND)
    @property
    def sj(self): return self._arr(self._sj, RP.ME_STAGE_JOB)
    @property
    def items(self): return self._arr(self._it, RP.ME_ITEM)
    @property
    def mask_items(self): return self._arr(self._mk, RP.ME_MASK_ITEM)

    def model(self, **knobs):
        return schedule_model(self.ij, self.cands, self.sj, self.items, self.mask_items, self.max_window, **knobs)

    def counts(self):
        return len(self._c), 9 * len(self._sj), len(self._it) + len(self._mk)


def texture(seed, h, w, lo, hi):
    return np.random.default_rng(seed).integers(lo, hi + 1, size=(h, w)).astype(np.int16)


def ramp(h, w):
    """every sample differs from every other one closer than 2^15 in raster order (a 2^15 ramp over the raster index): a wrong column moves every difference by 1, a wrong
    row by the pitch"""
    return (np.arange(h * w, dtype=np.int64) & 0x7fff).astype(np.int16).reshape(h, w)


# ---------------------------------------------------------------------------------------------------------------------------------------------------------
# expected values: the oracle only
# ---------------------------------------------------------------------------------------------------------------------------------------------------------
def _view(plan, p, off, w, h):
    """the oracle's (array, y, x) view of a block at offset `off` of plane p; a pool block is its own compact array"""
    arr, pad = plan.planes[p]
    if pad is None:
        return (np.ascontiguousarray(arr[off:off + w * h].reshape(h, w)), 0, 0)
    y, x = divmod(off + pad * arr.shape[1] + pad, arr.shape[1])
    return (arr, y, x)


def stage_positions(s):
    """[(k, tx, ty)] of the stage's evaluated positions, displacements in 1/16 sample"""
    f = int(s["i_frac"])
    ry = REFINE_YH if f == 2 else REFINE_YQ
    return [(k, (REFINE_X[k] + int(s["base_qx"])) * f * 4, (ry[k] + int(s["base_qy"])) * f * 4) for k in range(9) if (int(s["mask"]) >> k) & 1]


def expected(plan, orc, memo=None):
    """(candidate costs, stage costs [n, 9], item costs incl. the masked ones) of a plan, every value one oracle call (cached per distinct block pair in `memo`)"""
    memo = {} if memo is None else memo
    bd = plan.bd
    ij, cands, sj, items, mk = plan.ij, plan.cands, plan.sj, plan.items, plan.mask_items
    cc = np.full(cands.size, -1, np.int64)
    for j in ij:
        w, h, ss = int(j["width"]), int(j["height"]), int(j["sub_shift"])
        ov = _view(plan, int(j["org_plane"]), int(j["org_off"]), w, h)
        ra, ry, rx = _view(plan, int(j["ref_plane"]), int(j["ref_off"]), w, h)
        for k in range(int(j["first_cand"]), int(j["first_cand"]) + int(j["n_cand"])):
            dx, dy = int(cands[k]["dx"]), int(cands[k]["dy"])
            key = ("i", plan.name, int(j["org_plane"]), int(j["org_off"]), int(j["ref_plane"]), int(j["ref_off"]), w, h, ss, dx, dy)
            if key not in memo:
                memo[key] = orc.dist("SAD", ov, (ra, ry + dy, rx + dx), w, h, bd, ss)
            assert cc[k] in (-1, memo[key]), "two jobs that share a candidate entry must give it the same cost"
            cc[k] = memo[key]
    sc = np.zeros((sj.size, 9), np.int64)
    for n, s in enumerate(sj):
        w, h = int(s["width"]), int(s["height"])
        key = ("s", plan.name) + tuple(int(s[f]) for f in ("org_plane", "org_off", "ref_plane", "ref_off", "width", "height", "i_frac", "filter_mode", "alt_hpel", "func", "base_qx", "base_qy", "mask"))
        if key not in memo:
            ov = _view(plan, int(s["org_plane"]), int(s["org_off"]), w, h)
            ra, ry, rx = _view(plan, int(s["ref_plane"]), int(s["ref_off"]), w, h)
            row = np.zeros(9, np.int64)
            for k, tx, ty in stage_positions(s):
                pred = orc.if_pred_luma_me((ra, ry + (ty >> 4), rx + (tx >> 4)), w, h, tx & 15, ty & 15, bd, bool(s["alt_hpel"]), int(s["filter_mode"]))
                row[k] = orc.dist(DF_NAME[int(s["func"])], ov, (pred, 0, 0), w, h, bd, 0)
            memo[key] = row
        sc[n] = memo[key]
    ic = np.zeros(items.size + mk.size, np.int64)
    for n, it in enumerate(items):
        w, h, ss, f = int(it["width"]), int(it["height"]), int(it["sub_shift"]), DF_NAME[int(it["func"])]
        key = ("t", plan.name, int(it["org_plane"]), int(it["org_off"]), int(it["cur_plane"]), int(it["cur_off"]), w, h, ss, f)
        if key not in memo:
            ov, cv = _view(plan, int(it["org_plane"]), int(it["org_off"]), w, h), _view(plan, int(it["cur_plane"]), int(it["cur_off"]), w, h)
            if f == "HAD_2SAD":                 # (the entry takes compact operands, RdCost.cpp:1778)
                ov, cv = [(np.ascontiguousarray(a[y:y + h, x:x + w]), 0, 0) for a, y, x in (ov, cv)]
            memo[key] = orc.dist(f, ov, cv, w, h, bd, ss)
        ic[n] = memo[key]
    for n, it in enumerate(mk):
        w, h, ss = int(it["width"]), int(it["height"]), int(it["sub_shift"])
        key = ("m", plan.name) + tuple(int(it[f]) for f in ("org_plane", "org_off", "cur_plane", "cur_off", "mask_plane", "mask_off", "width", "height", "sub_shift"))
        if key not in memo:
            ov, cv = _view(plan, int(it["org_plane"]), int(it["org_off"]), w, h), _view(plan, int(it["cur_plane"]), int(it["cur_off"]), w, h)
            marr, mpad = plan.planes[int(it["mask_plane"])]
            assert mpad is None
            mo = int(it["mask_off"])
            mblk = np.ascontiguousarray(marr[mo:mo + w * (h >> ss)].reshape(h >> ss, w))      # compact: one row of w per evaluated row
            memo[key] = orc.sad_mask(ov, cv, (mblk, 0, 0), 1, -(w << ss), w, h, ss)
        ic[items.size + n] = memo[key]
    return cc, sc, ic


# ---------------------------------------------------------------------------------------------------------------------------------------------------------
# the scheduler's counting rules
# ---------------------------------------------------------------------------------------------------------------------------------------------------------
def win_pitch(win_w):
    return 2 * (((win_w + 3) >> 1) | 1)


def win_samples(win_w, win_h):
    return (win_h * win_pitch(win_w) + 7) & ~7


def window_lds(w, h, ss, win_w, win_h, n_cand):
    return (win_samples(win_w, win_h) + (h >> ss) * w) * 2 + n_cand * 8


def lds_class(lds):
    return 0 if lds > 24 * 1024 else (1 if lds > 6 * 1024 else 2)


TK_8x8, TK_16F, TK_16x8, TK_8x16, TK_8x4, TK_4x8, TK_4x4, TK_2x2 = range(8)


def tile_kind(w, h, fast):
    if w > h and not h & 7 and not w & 15: return TK_16x8
    if w < h and not w & 7 and not h & 15: return TK_8x16
    if w > h and not h & 3 and not w & 7: return TK_8x4
    if w < h and not w & 3 and not h & 7: return TK_4x8
    if fast and w == h and not w & 31: return TK_16F
    if not w & 7 and not h & 7: return TK_8x8
    if not w & 3 and not h & 3: return TK_4x4
    return TK_2x2


TILE_W = {TK_16F: 16, TK_16x8: 16, TK_4x8: 4, TK_4x4: 4, TK_2x2: 2}
TILE_H = {TK_16F: 16, TK_8x16: 16, TK_8x4: 4, TK_4x4: 4, TK_2x2: 2}
TILE_LANES = {TK_16x8: 16, TK_8x16: 16, TK_8x4: 4, TK_4x8: 4, TK_4x4: 2, TK_2x2: 1}


def team_lanes(w, h, ss):
    return min(64, (h >> ss) * (w >> 3))


def item_lanes(func, w, h, ss):
    if func in (DF["SAD"], DF["SSE"]):
        cw = 8 if w >= 8 else (4 if w >= 4 else 2)
        n = (h >> (ss if func == DF["SAD"] else 0)) * (w // cw)
    else:
        kind = tile_kind(w, h, func == DF["HAD_fast"])
        n = 1 if kind == TK_4x4 else (w // TILE_W.get(kind, 8)) * (h // TILE_H.get(kind, 8)) * TILE_LANES.get(kind, 8)
    return min(64, n)


def item_generic(func, w, h):
    if func in (DF["SAD"], DF["SSE"]):
        return w < 4
    kind = tile_kind(w, h, func == DF["HAD_fast"])
    return not (kind in (TK_8x8, TK_16F) or (kind == TK_4x4 and w == 4 and h == 4))


def cluster(job, cands, max_window, cand_cap=16, dedupe=True, extent_lt=False, edges=None):
    """the windows of one integer job, greedy in list order: [dict(x0, y0, x1, y1, c=[[dx, dy, [entries]]])]"""
    edges = set() if edges is None else edges
    w, h, ss = int(job["width"]), int(job["height"]), int(job["sub_shift"])
    mw = max_window if max_window > 0 else 24
    forced = w * h >= 128 * 64
    reach = min(mw, 16) if forced else mw
    if forced and mw > 16: edges.add("reach_forced_16")
    if max_window <= 0: edges.add("reach_default_24")
    tl = team_lanes(w, h, ss)
    wins = []
    f0, n = int(job["first_cand"]), int(job["n_cand"])
    if n == 0: edges.add("job_without_candidates")
    for k in range(f0, f0 + n):
        dx, dy = int(cands[k]["dx"]), int(cands[k]["dy"])
        placed = False
        if dedupe:
            for wn in wins:
                for q in wn["c"]:
                    if q[0] == dx and q[1] == dy:
                        if len(q[2]) < tl:
                            q[2].append(k); placed = True; edges.add("dedupe_fold")
                            break
                        edges.add("dedupe_team_full")
                if placed: break
        if placed: continue
        for wn in wins:
            if len(wn["c"]) >= cand_cap:
                edges.add("split_by_cap")
                continue
            x0, y0, x1, y1 = min(wn["x0"], dx), min(wn["y0"], dy), max(wn["x1"], dx), max(wn["y1"], dy)
            ok = (x1 - x0 < reach and y1 - y0 < reach) if extent_lt else (x1 - x0 <= reach and y1 - y0 <= reach)
            if ok:
                wn.update(x0=x0, y0=y0, x1=x1, y1=y1); wn["c"].append([dx, dy, [k]]); placed = True
                break
            edges.add("split_by_reach")
        if not placed:
            wins.append(dict(x0=dx, y0=dy, x1=dx, y1=dy, c=[[dx, dy, [k]]]))
    for wn in wins:
        ex, ey = wn["x1"] - wn["x0"], wn["y1"] - wn["y0"]
        if len(wn["c"]) == cand_cap: edges.add("cand_cap_full")
        if ex == reach and reach > 1: edges.add("extent_eq_reach_x")
        if ey == reach and reach > 1: edges.add("extent_eq_reach_y")
        edges.add("minDx_odd" if wn["x0"] & 1 else "minDx_even")
        if wn["x0"] < 0 or wn["y0"] < 0: edges.add("negative_displacement")
        for q in wn["c"]:
            if q[0] == wn["x1"] and ex: edges.add("x_odd_extreme" if ex & 1 else "x_even_extreme")
            if ss and q[1] == wn["y1"] and ey: edges.add("dy_odd_extreme_ss1" if ey & 1 else "dy_even_extreme_ss1")
        if ss: edges.add("winH_odd_ss1" if (ey + h) & 1 else "winH_even_ss1")
        win_w = ex + w
        if (win_pitch(win_w) >> 1) - (((win_w + 9) >> 3) - 1) * 4 < 4: edges.add("last_chunk_cut")
    return wins


def schedule_model(ij, cands, sj, items, mask_items, max_window, cand_cap=16, dedupe=True, atomic_stages=True, split_below=8192, bundle_work=80, band=True, extent_lt=False):
    """the counting rules of mePlanCreate / mePlanRun (see the module docstring) -> dict.  The keyword arguments are the scheduler's environment knobs
    (VVHIP_ME_CAND_CAP, _DEDUPE, _ATOMIC_STAGES, _SPLIT_VARIANTS, _BUNDLE_WORK, _XCD_BAND: without the band order a sub-class is sorted heaviest first, which changes
    the bundles); extent_lt is the sensitivity test's slip in the clustering ( < instead of <= the reach ).
    What vvhip_me_plan_info confirms on the device: the number of windows, of stage waves and of item waves, and the largest LDS need — so every edge that changes one
    of them (caps, reach, dedupe, deals, variants, bundle limits, items per wave) is checked against the library.  Taken on trust from this restatement, because the
    info has no field for them: the launch split (launch_*), the order edges (item_band_order, small_groups_banded, item_sorted, odd_class_then_shared) and tap_reload;
    they were compared with mePlanCreate / mePlanRun by reading, and the costs of those plans are compared with the oracle like all others."""
    edges = set()
    if max_window == 1: edges.add("max_window_1")
    if max_window == 40: edges.add("max_window_40")
    # ---- integer windows
    windows, flat = [], []
    for j in ij:
        w, h, ss = int(j["width"]), int(j["height"]), int(j["sub_shift"])
        row = []
        for wn in cluster(j, cands, max_window, cand_cap, dedupe, extent_lt, edges=edges):
            win_w, win_h, nc = wn["x1"] - wn["x0"] + w, wn["y1"] - wn["y0"] + h, len(wn["c"])
            lds = window_lds(w, h, ss, win_w, win_h, nc)
            rec = dict(minDx=wn["x0"], minDy=wn["y0"], winW=win_w, winH=win_h, nCand=nc, lds=lds, cls=lds_class(lds), cands=wn["c"])
            row.append(rec); flat.append(rec)
            edges.add(("lds_large", "lds_mid", "lds_small")[rec["cls"]])
            if (h >> ss) * (w >> 3) > 4 * (64 if rec["cls"] == 2 else 256): edges.add("org_beyond_4_chunks")
        windows.append(row)
    al = lambda v: (v + 15) & ~15
    n_large, n_mid, n_small = (sum(1 for r in flat if r["cls"] == c) for c in (0, 1, 2))
    lds_int = al(max([r["lds"] for r in flat] or [0]))
    lds_mid, lds_small = (al(max([r["lds"] for r in flat if r["cls"] == c] or [0])) for c in (1, 2))
    int_big = n_large + n_mid
    int_split = int_big > 0 and n_small > 0 and lds_int > 8 * lds_small and lds_int > 32 * 1024
    split_large = n_large > 0 and n_mid > 0 and lds_int > lds_mid + lds_mid // 2
    launches = 0
    if flat:
        launches = 1 if not (split_large or int_split) else (2 if split_large else 1) + (1 if int_split and n_small else 0)
        edges.add({1: "launch_single", 2: "launch_split_large" if split_large else "launch_split_small", 3: "launch_three"}[launches])
        if lds_int > 64 * 1024: edges.add("lds_over_64k")
        if n_small % 4: edges.add("small_group_short")
        if (n_small + 3) // 4 > 8: edges.add("small_groups_banded")
    # ---- stages
    tap_set = lambda s: 0 if (s["filter_mode"] == 2 and not s["alt_hpel"]) else (2 if s["filter_mode"] == 0 else 1)
    set_of = lambda s: 2 * tap_set(s) + (0 if (s["width"] == s["height"] and 8 <= s["width"] <= 64) else 1)
    unit_w = lambda s: min(int(s["width"]), 64)
    unit_h = lambda s: min(int(s["height"]), 32)
    units_of = lambda s: (int(s["width"]) // unit_w(s)) * (int(s["height"]) // unit_h(s))
    deal_of = lambda s: 2 if units_of(s) == 1 else (1 if units_of(s) > 2 and atomic_stages else 0)
    unit_work = lambda s: bin(int(s["mask"])).count("1") * max(1, unit_w(s) // 8) * unit_h(s)
    units_unsplit = sum(units_of(s) for s in sj)
    split_variants = units_unsplit < split_below
    st_order, stages = [], []
    for i, s in enumerate(sj):
        n = units_of(s)
        n_var = 1
        if split_variants and unit_w(s) >= 32 and (n <= 2 or atomic_stages):
            n_var = max(1, len({tx for _, tx, _ in stage_positions(s)}))
        if unit_w(s) >= 32 and len({tx for _, tx, _ in stage_positions(s)}) > 1:
            edges.add("variants_split" if n_var > 1 else "variants_unsplit")
        stages.append(dict(units=n, deal=deal_of(s), variants=n_var))
        edges.add(("deal_shared", "deal_atomic", "deal_single")[deal_of(s)])
        if deal_of(s) == 1: edges.add("atomic_clear")
        if not int(s["mask"]): edges.add("stage_mask_empty")
        if any(abs(tx) == 16 or abs(ty) == 16 for _, tx, ty in stage_positions(s)): edges.add("stage_disp_pm16")
        for vr in range(n_var):
            st_order.extend((i, vr, u) for u in range(n))
    st_order.sort(key=lambda e: (set_of(sj[e[0]]), deal_of(sj[e[0]]), -unit_w(sj[e[0]]), int(sj[e[0]]["ref_off"]) if band else -unit_work(sj[e[0]])))      # (stable, like the host's)
    set_waves, lds_stage, waves_stage, i = [0] * 6, 0, 0, 0
    first_deal = {}
    while i < len(st_order):
        s0 = sj[st_order[i][0]]
        work, count = 0, 0
        if deal_of(s0) == 0: count = units_of(s0) // 2
        elif deal_of(s0) == 1: count = 1
        else:
            while i + count < len(st_order) and count < 8:
                s = sj[st_order[i + count][0]]
                if unit_w(s) != unit_w(s0) or set_of(s) != set_of(s0) or deal_of(s) != 2: break
                if count and work + unit_work(s) > bundle_work:
                    edges.add("bundle_work_over_80")
                    break
                work += unit_work(s); count += 1
            if count == 8 and i + count < len(st_order) and set_of(sj[st_order[i + 8][0]]) == set_of(s0) and unit_w(sj[st_order[i + 8][0]]) == unit_w(s0): edges.add("bundle_cap_8")
            if work == bundle_work and count > 1: edges.add("bundle_work_at_80")
            tabs = [int(sj[st_order[i + u][0]]["filter_mode"]) * 2 + (1 if sj[st_order[i + u][0]]["alt_hpel"] else 0) for u in range(count)]
            if any(a != b for a, b in zip(tabs, tabs[1:])): edges.add("tap_reload")
        first_deal.setdefault(set_of(s0), deal_of(s0))
        set_waves[set_of(s0)] += 1
        waves_stage += 1
        bh = max(unit_h(sj[st_order[i + u][0]]) for u in range(count))
        nt = (4, 6, 8)[tap_set(s0)]
        lds_stage = max(lds_stage, (2 * (128 + 64 + 16 + 16) + (3 if unit_w(s0) <= 16 else 1) * (bh + nt) * (max(8, unit_w(s0)) + 8)) * 2)
        i += count
    used = [k for k in range(6) if set_waves[k]]
    if any(set_waves[a] & 1 and first_deal[b] == 0 for a, b in zip(used, used[1:])): edges.add("odd_class_then_shared")
    # ---- items
    waves_lean = waves_gen = 0
    lean_classes = []                           # waves per lean class, in schedule order
    if len(items):
        f_, w_, h_, s_ = (items[n].astype(np.int64) for n in ("func", "width", "height", "sub_shift"))
        base = w_ << 32 | h_ << 16 | f_ << 8 | s_
        ub, inv = np.unique(base, return_inverse=True)
        lean_u = np.array([0 if item_generic(int(k >> 8) & 0xff, int(k >> 32), int(k >> 16) & 0xffff) else 1 for k in ub], np.int64)
        keys = base | lean_u[inv] << 48
        order = np.argsort(-keys, kind="stable")
        if (np.diff(order) < 0).any(): edges.add("item_sorted")
        ks = keys[order]
        starts = np.concatenate([[0], np.nonzero(np.diff(ks))[0] + 1, [ks.size]])
        for a, b in zip(starts[:-1], starts[1:]):
            k = int(ks[a])
            per = max(1, 64 // item_lanes((k >> 8) & 0xff, (k >> 32) & 0xffff, (k >> 16) & 0xffff, k & 0xff))
            run = int(b - a)
            if per > 1 and run >= per: edges.add("item_wave_full")
            if per > 1 and run % per: edges.add("item_wave_partial")
            waves = (run + per - 1) // per
            if k >> 48: waves_lean += waves; lean_classes.append(waves)
            else: waves_gen += waves
    if waves_lean: edges.add("item_lean")
    if waves_gen: edges.add("item_generic")
    if waves_lean > 65536: edges.add("item_long_lean")
    if waves_gen > 65536: edges.add("item_long_generic")
    if waves_lean <= 65536:                     # band order: classes of more than 8 whole workgroups
        w0 = 0
        for waves in lean_classes:
            if (w0 + waves - ((w0 + 3) & ~3)) // 4 > 8: edges.add("item_band_order")
            w0 += waves
    mkey = lambda it: int(it["width"]) << 32 | int(it["height"]) << 16 | int(it["sub_shift"])
    mkeys = sorted((mkey(it) for it in mask_items), reverse=True)
    waves_mask, i = 0, 0
    while i < len(mkeys):
        k = mkeys[i]
        w, h, ss = k >> 32, (k >> 16) & 0xffff, k & 0xffff
        per = max(1, 64 // min(64, (h >> ss) * (w // (8 if w >= 8 else (4 if w >= 4 else 2)))))
        count = 0
        while i + count < len(mkeys) and count < per and mkeys[i + count] == k: count += 1
        waves_mask += 1
        i += count
    if waves_mask: edges.add("item_masked")
    for arr, fields in ((ij, ("org_plane", "ref_plane")), (sj, ("org_plane", "ref_plane")), (items, ("org_plane", "cur_plane")), (mask_items, ("org_plane", "cur_plane", "mask_plane"))):
        if any((arr[f] == 15).any() for f in fields): edges.add("plane_15")
    return dict(windows=windows, waves_int=len(flat), lds_int=lds_int, lds_mid=lds_mid, lds_small=lds_small, n_large=n_large, n_mid=n_mid, n_small=n_small,
                split_large=split_large, int_split=int_split, int_launches=launches, stages=stages, waves_stage=waves_stage, set_waves=set_waves, lds_stage=al(lds_stage),
                split_variants=split_variants, waves_item_lean=waves_lean, waves_item_generic=waves_gen, waves_item_masked=waves_mask,
                waves_item=waves_lean + waves_gen + waves_mask, lds_bytes=max(lds_int, al(lds_stage)), edges=edges)


# ---------------------------------------------------------------------------------------------------------------------------------------------------------
# intBody's addressing in int64 (sensitivity test only)
# ---------------------------------------------------------------------------------------------------------------------------------------------------------
MUTATIONS = ("even_pitch", "half0_floor", "parity_dropped", "last_chunk_uncut")      # of window_model; the fifth, extent_lt, is a slip of the clustering: schedule_model
GARBAGE = -12345                                # what LDS holds where nothing was staged


def window_model(plan, job, win, mutation=None):
    """{candidate entry: cost} of one window (a record of schedule_model) of integer job `job`.  Staging: rows of ( winW + 9 ) >> 3 chunks of 8 samples from the plane
    into rows of `pitch` samples, a chunk's dwords beyond the pitch dropped, under sub_shift 1 the even rows first and the odd rows from row half0 on; scoring: every
    second row under sub_shift 1, columns from the even sample below x plus one sample when x is odd.  `reads`: the flat (first, last) element range fetched from the
    reference plane is returned as the second value."""
    w, h, ss = int(job["width"]), int(job["height"]), int(job["sub_shift"])
    rows_eff = h >> ss
    win_w, win_h = win["winW"], win["winH"]
    pitch, half0 = win_pitch(win_w), (win_h + 1) >> 1
    pitch_s = 2 * ((win_w + 3) >> 1) if mutation == "even_pitch" else pitch              # the staging side's values
    half0_s = win_h >> 1 if mutation == "half0_floor" else half0
    oa, oy, ox = _view(plan, int(job["org_plane"]), int(job["org_off"]), w, h)
    org = oa[oy:oy + h:1 << ss, ox:ox + w].astype(np.int64)
    ra, rpad = plan.planes[int(job["ref_plane"])]
    rs = ra.shape[1]
    flat = ra.reshape(-1)
    base = int(job["ref_off"]) + rpad * rs + rpad + win["minDy"] * rs + win["minDx"]
    cpr = (win_w + 2 + 7) >> 3
    lds = np.full(win_samples(win_w, win_h) + 4 * pitch + 64, GARBAGE, np.int64)
    r = np.arange(win_h)
    dr = np.where(r & 1, half0_s, 0) + (r >> 1) if ss else r
    # every (chunk c, dword d, row r, sample k) of the window at once, in the order chunk, dword, row: where stores overlap (they do under a mutation only) the later
    # chunk wins, and the dwords that a cut drops land last — as a slower lane's stores would
    c = np.arange(cpr)[:, None, None, None]
    d = np.arange(4)[None, :, None, None]
    k = np.arange(2)[None, None, None, :]
    src = base + r[None, None, :, None] * rs + c * 8 + 2 * d + k
    dst = dr[None, None, :, None] * pitch_s + c * 8 + 2 * d + k
    keep = np.broadcast_to((d == 0) | ((pitch_s >> 1) - c * 4 > d), dst.shape)            # dwords of the chunk inside the row
    lds[dst[keep]] = flat[src[keep]]
    if mutation == "last_chunk_uncut":
        lds[dst[~keep]] = flat[src[~keep]]
    reads = (base, base + (win_h - 1) * rs + cpr * 8 - 1)
    out = {}
    ex, ey = win_w - w, win_h - h
    for dx, dy, entries in win["cands"]:
        x, y = dx - win["minDx"], dy - win["minDy"]
        assert 0 <= x <= ex and 0 <= y <= ey
        row_base = (half0 if y & 1 else 0) + (y >> 1) if ss else y
        par = 0 if mutation == "parity_dropped" else (x & 1)
        idx = (row_base + np.arange(rows_eff))[:, None] * pitch + (x & ~1) + par + np.arange(w)[None, :]
        cost = int(np.abs(lds[idx] - org).sum()) << ss
        for e in entries:
            out[e] = cost
    return out, reads


# ---------------------------------------------------------------------------------------------------------------------------------------------------------
# families
# ---------------------------------------------------------------------------------------------------------------------------------------------------------
A_PAD, A_VIS = 48, 192
A_BLOCKS = [(8, 4, 0), (8, 8, 0), (16, 16, 0), (16, 16, 1), (32, 8, 0), (64, 64, 1), (128, 64, 1), (128, 128, 0), (128, 128, 1)]
_planes_cache = {}


def a_planes():
    if "a" not in _planes_cache:
        full = A_VIS + 2 * A_PAD
        _planes_cache["a"] = (texture(101, full, full, 0, 1023), texture(102, full, full, 0, 1023), ramp(full, full))
    return _planes_cache["a"]


def _a_new(name, mw):
    p = Plan(name, 10, mw)
    org, ref, rmp = a_planes()
    p.plane(org, A_PAD); p.plane(ref, A_PAD); p.plane(rmp, A_PAD)
    return p


def _extent_sets(ex, ey):
    """candidates whose bounding box is exactly ex x ey: the corners, and a point one short of the far corner (the other parity of x and y)"""
    pts = [(0, 0), (ex, ey), (ex, 0), (0, ey), (max(ex - 1, 0), max(ey - 1, 0))]
    return list(dict.fromkeys(pts))


def family_a():
    """window geometry: one plan per max_window; in every plan each block with extents {0, 1, reach - 1, reach}^2 at both parities of (minDx, minDy), on the texture and on
    the ramp; the same sets with an extent of reach + 1, which split; windows at the first and the last readable sample of the plane"""
    plans = []
    for mw in (0, 1, 8, 16, 24, 40):
        p = _a_new("A max_window %d" % mw, mw)
        blocks = [(32, 32, 0)] if mw == 40 else A_BLOCKS + ([(64, 128, 1), (128, 64, 0)] if mw == 24 else [])
        for (w, h, ss) in blocks:
            mwe = mw if mw > 0 else 24
            reach = min(mwe, 16) if w * h >= 8192 else mwe
            exts = sorted({0, 1, max(reach - 1, 0), reach})
            bx = by = 24
            for ex in exts + [reach + 1]:
                for ey in exts + [reach + 1]:
                    if ex > reach and ey > reach:
                        continue                                                         # (one more than the reach in one direction at a time: two windows)
                    for v in (0, 1):                                                     # parity of (minDx, minDy)
                        cl = [(a - 6 - v, b - 3 + v) for a, b in _extent_sets(ex, ey)]
                        for rp in (1, 2):                                                # the texture and the ramp
                            p.int_job(0, p.off(0, bx, by), rp, bx, by, w, h, ss, cl)
        if mw == 24:
            # the first sample of the plane's storage, and the last row but one up to the plane's right edge (the row behind it holds the 18 bytes a row is read beyond itself)
            for (w, h, ss) in ((8, 4, 0), (16, 16, 1), (64, 64, 1)):
                p.int_job(0, p.off(0, 0, 0), 1, 0, 0, w, h, ss, [(-A_PAD, -A_PAD), (-A_PAD + 7, -A_PAD + 3)])
                p.int_job(0, p.off(0, 0, 0), 1, A_VIS - w, A_VIS - h, w, h, ss, [(A_PAD, A_PAD - 1), (A_PAD - 7, A_PAD - 4)])
            p.edges |= {"read_at_plane_start", "read_at_plane_end"}
        plans.append(p)
    return plans


def family_b():
    """candidate lists: distinct positions at the cap of 16 and its multiples, a raster of 300, repeats at the team size, empty jobs, shared and last candidate ranges"""
    p = _a_new("B candidate lists", 0)
    grid = [(a - 3, b - 3) for b in range(7) for a in range(7)]
    for n in (1, 15, 16, 17, 32, 33, 49):
        p.int_job(0, p.off(0, 30, 30), 1, 30, 30, 16, 16, 0, grid[:n])
        p.int_job(0, p.off(0, 30, 30), 1, 30, 30, 8, 8, 0, [])                          # n_cand 0 between the others
    p.int_job(0, p.off(0, 40, 40), 2, 40, 40, 32, 8, 0, [(a - 10, b - 7) for b in range(15) for a in range(20)])      # 300 in raster order
    for (w, h, ss) in ((8, 4, 0), (8, 8, 0), (64, 64, 1)):
        tl = team_lanes(w, h, ss)
        for rep in (tl - 1, tl, tl + 1, 2 * tl + 1):
            s, o = (1, -2), (2, -2)
            p.int_job(0, p.off(0, 20, 28), 1, 20, 28, w, h, ss, [s] * rep + [o])                             # adjacent, at the front
            p.int_job(0, p.off(0, 20, 28), 2, 20, 28, w, h, ss, [o] + [s] * rep)                             # at the end
            half = rep // 2
            p.int_job(0, p.off(0, 20, 28), 1, 20, 28, w, h, ss, [s] * half + [o, (0, 3)] + [s] * (rep - half))      # at both ends
        # a position whose first window is full: 17 distinct, then the first one again, more often than a team has lanes
        p.int_job(0, p.off(0, 20, 28), 1, 20, 28, w, h, ss, grid[:17] + [grid[0]] * (tl + 2))
    # two jobs of one block that share a part of their candidate range
    first = len(p._c)
    p._c.extend(grid[:15])
    p.int_job(0, p.off(0, 50, 50), 1, 50, 50, 16, 16, 1, grid[:10], first=first)
    p.int_job(0, p.off(0, 50, 50), 1, 50, 50, 16, 16, 1, grid[5:15], first=first + 5)
    p.int_job(0, p.off(0, 8, 8), 2, 8, 8, 8, 4, 0, [(0, 0), (-5, 7), (0, 0)])             # the last n_cand entries of the list
    assert int(p.ij[-1]["first_cand"]) + int(p.ij[-1]["n_cand"]) == p.cands.size
    return [p]


SMALL_WIN, MID_WIN, LARGE_WIN, LARGE_LOW, HUGE_WIN = (8, 4, 0, 0), (64, 64, 0, 0), (128, 64, 0, 0), (128, 64, 1, 0), (128, 128, 0, 16)


def closest_to_cap(cap):
    """(below, above): the (w, h, ss, ex, ey) whose window needs the most LDS <= cap / the least > cap, candidates at the two corners of the extent"""
    best_lo, best_hi = None, None
    for (w, h, ss) in A_BLOCKS + [(32, 32, 0), (64, 32, 0), (32, 16, 0), (128, 32, 0)]:
        reach = 16 if w * h >= 8192 else 24
        for ex in range(reach + 1):
            for ey in range(reach + 1):
                lds = window_lds(w, h, ss, w + ex, h + ey, 2 if ex or ey else 1)
                if lds <= cap and (best_lo is None or lds > best_lo[0]): best_lo = (lds, (w, h, ss, ex, ey))
                if lds > cap and (best_hi is None or lds < best_hi[0]): best_hi = (lds, (w, h, ss, ex, ey))
    return best_lo, best_hi


def family_c():
    """window launches: every combination of the three LDS classes and the two split decisions, workgroups of small windows at 1 .. 39 windows, windows next to the caps"""
    plans = []

    def add(p, spec, k, rp=1):
        w, h, ss, ext = spec
        x, y = 8 + 5 * (k % 9), 8 + 3 * (k % 11)
        p.int_job(0, p.off(0, x, y), rp, x, y, w, h, ss, [(-1, 0), (-1 + ext, ext)] if ext else [(k % 3 - 1, -(k % 2))])
    for n in (1, 2, 3, 4, 5, 36, 37, 39):
        p = _a_new("C %d small windows" % n, 0)
        for k in range(n): add(p, SMALL_WIN, k, 1 + k % 2)
        plans.append(p)
    combos = {"mid only": [MID_WIN] * 3, "large only": [LARGE_WIN] * 2 + [HUGE_WIN], "small + mid": [SMALL_WIN] * 5 + [MID_WIN] * 2,
              "small + large, split": [SMALL_WIN] * 6 + [LARGE_WIN], "small + large, one launch": [(32, 32, 0, 0)] * 3 + [LARGE_LOW],
              "mid + large, split": [MID_WIN] * 2 + [LARGE_WIN] * 2, "mid + large, one launch": [(64, 64, 0, 16)] * 2 + [LARGE_LOW],
              "three classes, both splits": [SMALL_WIN] * 7 + [MID_WIN] * 2 + [LARGE_WIN, HUGE_WIN]}
    for name, specs in combos.items():
        p = _a_new("C " + name, 0)
        for k, sp in enumerate(specs): add(p, sp, k)
        plans.append(p)
    p = _a_new("C windows next to the 6 KB and 24 KB caps", 0)
    for cap in (6 * 1024, 24 * 1024):
        for (lds, (w, h, ss, ex, ey)) in closest_to_cap(cap):
            p.int_job(0, p.off(0, 16, 16), 1, 16, 16, w, h, ss, [(-3, -2), (-3 + ex, -2 + ey)] if ex or ey else [(-3, -2)])
    plans.append(p)
    p = _a_new("C one workgroup of an 8x4 window next to 32x32 windows", 0)
    add(p, SMALL_WIN, 0); add(p, (32, 32, 0, 3), 1); add(p, SMALL_WIN, 2); add(p, (32, 32, 0, 0), 3)
    plans.append(p)
    return plans


D_PAD, D_VIS = 16, 176


def d_planes(bd):
    if ("d", bd) not in _planes_cache:
        full = D_VIS + 2 * D_PAD
        top = (1 << bd) - 1
        _planes_cache[("d", bd)] = (texture(200 + bd, full, full, 0, top), texture(300 + bd, full, full, 0, top),
                                    texture(400 + bd, 1, 1 << 16, -top, 2 * top).reshape(-1))      # the pool: bi-prediction patterns 2 org - pred
    return _planes_cache[("d", bd)]


def _d_new(name, bd):
    p = Plan(name, bd, 0)
    org, ref, pool = d_planes(bd)
    p.plane(org, D_PAD); p.plane(ref, D_PAD); p.pool(pool)
    return p


TAP_FORMS = ((2, 0, "HAD"), (1, 0, "SAD"), (1, 1, "SAD"), (2, 1, "SAD"), (0, 0, "HAD_fast"), (0, 1, "HAD_fast"))      # (filter_mode, alt_hpel, function of the tap support)


def _reach_mask(i_frac, bq):
    ry = REFINE_YH if i_frac == 2 else REFINE_YQ
    return sum(1 << k for k in range(9) if abs((REFINE_X[k] + bq[0]) * i_frac * 4) <= 16 and abs((ry[k] + bq[1]) * i_frac * 4) <= 16)


def family_d_sweep(bd):
    """every valid (i_frac, base, k) of an 8x8 block under the six (tap table, alternative half-sample filter) forms"""
    p = _d_new("D position sweep, %d bits" % bd, bd)
    n = 0
    for (mode, alt, func) in TAP_FORMS:
        for i_frac in (1, 2):
            for bqy in range(-3, 4):
                for bqx in range(-3, 4):
                    mask = _reach_mask(i_frac, (bqx, bqy))
                    assert i_frac == 2 or mask == 511
                    x, y = 8 + 8 * (n % 17), 8 + 8 * (n % 13)
                    p.stage(0, p.off(0, x, y), 1, x + 1, y - 1, 8, 8, i_frac, mode, alt, func, (bqx, bqy), mask)
                    n += 1
    return p


D_SHAPES = [(8, 4, "HAD"), (4, 8, "HAD"), (4, 32, "HAD"), (16, 8, "HAD"), (8, 16, "HAD"), (16, 16, "HAD_fast"), (32, 32, "HAD_fast"), (64, 32, "HAD"), (64, 64, "HAD_fast"),
            (128, 32, "SAD"), (32, 128, "HAD"), (128, 64, "HAD"), (128, 128, "HAD_fast")]


def wide_stages(p):
    """the three wide stages the unsplit plan shares with the small one (same records: their costs must not depend on how the variants are dealt)"""
    p.stage(0, p.off(0, 8, 8), 1, 9, 7, 64, 32, 1, 2, 0, "HAD", (1, -1), 511)
    p.stage(0, p.off(0, 40, 16), 1, 41, 17, 64, 64, 2, 1, 1, "HAD_fast", (0, 0), 511)
    p.stage(0, p.off(0, 16, 24), 1, 15, 24, 128, 128, 1, 0, 0, "HAD", (-2, 2), 511)
    return 3


def family_d_shapes(bd):
    """one shape per tile kind and deal, each with the full mask, every single bit and the empty mask; originals from the pool on every second shape"""
    p = _d_new("D tile kinds and deals, %d bits" % bd, bd)
    for n, (w, h, func) in enumerate(D_SHAPES):
        mode, alt = ((2, 0), (1, 0), (0, 0), (1, 1))[n % 4]
        for m, mask in enumerate([511] + [1 << k for k in range(9)] + [0]):
            x, y = 16 + (n % 5), 16 + (m % 7)
            i_frac = 1 + (m + n) % 2
            if n % 2:
                p.stage(2, 64 * (n + 3 * m), 1, x, y, w, h, i_frac, mode, alt, func, (0, 0), mask)
                p.edges.add("stage_org_pool")
            else:
                p.stage(0, p.off(0, x + 3, y + 1), 1, x, y, w, h, i_frac, mode, alt, func, (0, 0), mask)
    wide_stages(p)
    # integer jobs whose original block comes from the pool
    for (w, h, ss) in ((8, 4, 0), (64, 64, 1), (128, 128, 0)):
        p.int_job(2, 128 + 2 * w, 1, 20, 20, w, h, ss, [(0, 0), (-3, 2), (5, 5), (0, 0)])
    p.edges.add("int_org_pool")
    return p


def family_d_bundles(bd=10):
    plans = []
    for n in (7, 8, 9, 17):
        p = _d_new("D %d equal 8x4 units, %d bits" % (n, bd), bd)
        for k in range(n):
            p.stage(0, p.off(0, 8 * k, 8), 1, 8 * k + 1, 8, 8, 4, 2, 2, 0, "HAD", (0, 0), 1 << (k % 9))
        plans.append(p)
    # 64 + 12 / 64 + 16 / 64 + 20 row groups: one bundle, one bundle at the budget, two bundles  (an 8x32 unit with two positions, an 8x4 unit with 3 / 4 / 5)
    for extra in (3, 4, 5):
        p = _d_new("D bundle of %d row groups, %d bits" % (64 + 4 * extra, bd), bd)
        p.stage(0, p.off(0, 8, 8), 1, 8, 8, 8, 32, 2, 2, 0, "HAD", (0, 0), 0b11)
        p.stage(0, p.off(0, 24, 8), 1, 24, 9, 8, 4, 2, 2, 0, "HAD", (0, 0), (1 << extra) - 1)
        plans.append(p)
    p = _d_new("D one bundle, three tap tables, %d bits" % bd, bd)
    for k in range(6):
        mode, alt = ((1, 0), (1, 1), (2, 1))[k % 3]
        p.stage(0, p.off(0, 8 * k, 16), 1, 8 * k, 17, 8, 4, 2, mode, alt, "HAD", (0, 0), 0b101)      # (the half-sample positions: where the alternative filter differs)
    plans.append(p)
    p = _d_new("D classes that end on an odd wave in front of shared stages, %d bits" % bd, bd)
    for k in range(3):
        p.stage(0, p.off(0, 8 * k, 8), 1, 8 * k, 8, 8, 8, 2, 2, 0, "HAD", (0, 0), 0b1001)              # 4-tap, square: one wave
    p.stage(0, p.off(0, 8, 24), 1, 9, 24, 128, 32, 2, 2, 0, "HAD", (0, 0), 511)                        # 4-tap, any shape: shared (halves)
    p.stage(0, p.off(0, 8, 40), 1, 8, 41, 16, 8, 1, 2, 0, "HAD", (1, 1), 511)                           # ... and one single-unit wave behind it: three waves
    p.stage(0, p.off(0, 30, 30), 1, 30, 31, 64, 64, 2, 1, 0, "HAD_fast", (0, 0), 511)                   # 6-tap, square: shared
    plans.append(p)
    return plans


def family_d_unsplit(bd=10):
    """at least 8 192 units: the horizontal variants of a wide unit stay in one wave"""
    p = _d_new("D 8192 narrow stages + the wide ones, %d bits" % bd, bd)
    for k in range(8192):
        q = k % 64
        p.stage(0, p.off(0, 8 * (q % 8), 8 * (q // 8)), 1, 8 * (q % 8) + 1, 8 * (q // 8) + 2, 32, 8, 1 + q % 2, 2, 0, "HAD", (0, 0), 1 << (q % 9))
    n = wide_stages(p)
    small = _d_new("D the wide stages of the long plan alone, %d bits" % bd, bd)
    wide_stages(small)
    return p, small, n


E_SHAPES = [(2, 2), (4, 4), (8, 8), (16, 8), (64, 8), (128, 128)]
E_FUNCS = ("SAD", "SSE", "HAD", "HAD_fast", "HAD_2SAD", "MASK")


def _e_new(name):
    p = _a_new(name, 0)
    w = np.random.default_rng(77).integers(0, 9, 1 << 15).astype(np.int16)             # GEO weights 0 .. 8
    p.pool(w)                                                                           # plane 3
    return p


def _e_item(p, f, w, h, k, ss=0):
    x, y = 3 * (k % 8), 5 * (k % 8)                                                     # eight distinct block pairs per key
    if f == "MASK":
        p.mask_item(0, p.off(0, x, y), 1, p.off(1, x - 7, y + 9), 3, 64 * (k % 8), ss, w, h)
    else:
        # (the ramp holds values up to 2^15: inside the contract of SAD and SSE items, outside the Hadamard family's operand range)
        p.item(0, p.off(0, x, y), 1 + k % 2 if f in ("SAD", "SSE") else 1, p.off(1, x - 7, y + 9), f, ss, w, h)


def family_e_runs():
    """per function and shape runs of perWave - 1, perWave, perWave + 1 and 4 perWave + 1 items of one key, the keys interleaved in the caller's list"""
    plans = []
    for tag, run_of in (("perWave - 1", lambda per: per - 1), ("perWave", lambda per: per), ("perWave + 1", lambda per: per + 1), ("4 perWave + 1", lambda per: 4 * per + 1)):
        p = _e_new("E runs of %s items" % tag)
        todo = []
        for f in E_FUNCS:
            for (w, h) in E_SHAPES:
                lanes = item_lanes(DF["SAD"] if f == "MASK" else DF[f], w, h, 0)
                todo.append([f, w, h, run_of(max(1, 64 // lanes))])
        k = 0
        while any(t[3] for t in todo):                                                  # round robin over the keys: the sort must bring each run together again
            for t in todo:
                if t[3]:
                    _e_item(p, t[0], t[1], t[2], k); t[3] -= 1; k += 1
        plans.append(p)
    return plans


def family_e_classes():
    plans = []
    p = _e_new("E a class of 37 waves (band order, a remainder)")
    for k in range(37): _e_item(p, "SAD", 64, 8, k)
    for k in range(5): _e_item(p, "SAD", 16, 16, k, 1)
    plans.append(p)
    p = _e_new("E lean items only")
    for k in range(9): _e_item(p, ("SAD", "SSE", "HAD")[k % 3], 8, 8, k)
    plans.append(p)
    p = _e_new("E generic items only")
    for k in range(9): _e_item(p, ("HAD", "HAD_fast", "HAD_2SAD")[k % 3], (16, 8, 2)[k % 3], (8, 16, 2)[k % 3], k)
    plans.append(p)
    p = _e_new("E masked items only, behind zero plain items")
    for k in range(9): _e_item(p, "MASK", (8, 16, 4)[k % 3], (8, 16, 8)[k % 3], k, k % 2)
    plans.append(p)
    p = _e_new("E plane 15 of a 16-entry table")
    org, ref, rmp = a_planes()
    while len(p.planes) < 15: p.plane(ref, A_PAD)
    p.plane(texture(103, *ref.shape, 0, 1023), A_PAD)                                    # plane 15: a texture of its own (any other entry of the table gives another cost)
    p.item(0, p.off(0, 8, 8), 15, p.off(15, 11, 12), "SAD", 0, 16, 16)
    p.item(0, p.off(0, 8, 8), 15, p.off(15, -3, 40), "HAD", 0, 8, 8)
    plans.append(p)
    return plans


def family_e_long():
    """65 536 and 65 537 waves per launch: at most 65 536 go as four-wave workgroups, more as one wave per workgroup; 64 distinct block pairs"""
    plans = []
    for n_lean, n_gen in ((65536, 65537), (65537, 65536)):
        p = _e_new("E %d lean + %d generic waves" % (n_lean, n_gen))
        for k in range(n_lean):
            q = k % 64
            p.item(0, p.off(0, q, 2 * q), 1, p.off(1, 2 * q - 5, q + 3), "SAD", 0, 64, 8)
        for k in range(n_gen):
            q = (k * 7) % 64
            p.item(0, p.off(0, q, q), 1, p.off(1, q + 2, 2 * q - 9), "HAD", 0, 64, 32)
        plans.append(p)
    return plans


F_RANGES = {"samples": (0, 1023), "bi-prediction": (-1023, 2047), "int16": (-32768, 32767)}


def f_blocks(lo, hi, n=144):
    """(org, ref) pairs of n x n samples: the largest difference of either sign, checkers, a region a few levels below the extreme"""
    rng = np.random.default_rng(hi - lo)
    yy, xx = np.mgrid[0:n, 0:n]
    chk = ((yy + xx) & 1).astype(bool)
    c = lambda v: np.full((n, n), v, np.int16)
    return {"org high": (c(hi), c(lo)), "org low": (c(lo), c(hi)),
            "checkers": (np.where(chk, hi, lo).astype(np.int16), np.where(chk, lo, hi).astype(np.int16)),
            "near the extreme": ((hi - rng.integers(0, 4, (n, n))).astype(np.int16), (lo + rng.integers(0, 4, (n, n))).astype(np.int16))}


def family_f():
    plans = []
    for name, (lo, hi) in F_RANGES.items():
        p = Plan("F operands: " + name, 10, 0)
        for tag, (org, ref) in f_blocks(lo, hi).items():
            po, pr = p.plane(org, 8), p.plane(ref, 8)
            for (w, h, ss) in ((8, 4, 0), (64, 64, 0), (128, 128, 0)):
                p.int_job(po, p.off(po, 0, 0), pr, 0, 0, w, h, ss, [(0, 0), (1, 0), (0, 1), (-1, -1), (0, 0)])
        plans.append(p)
    return plans


def compact_plan():
    """families G and H: windows with repeats and more than 16 positions, a 128x128 stage, wide and narrow stages, more than 64 lean item waves, generic and masked items"""
    p = _d_new("compact plan", 10)
    grid = [(a - 3, b - 2) for b in range(5) for a in range(5)]
    p.int_job(0, p.off(0, 16, 16), 1, 16, 16, 16, 16, 1, grid + [grid[0]] * 8 + [(9, -9)])      # 26 positions in 34 entries: two windows, three without the dedupe, one at a cap of 64
    p.int_job(0, p.off(0, 8, 24), 1, 9, 23, 64, 64, 1, [(0, 0), (1, 0), (0, 0), (-2, 3), (0, 0)])
    p.int_job(0, p.off(0, 4, 4), 1, 4, 4, 8, 4, 0, [(0, 0)] * 6 + [(1, 1)])
    p.int_job(0, p.off(0, 16, 16), 1, 16, 16, 128, 128, 0, [(0, 0), (3, -3)])
    wide_stages(p)
    p.stage(0, p.off(0, 8, 8), 1, 8, 9, 8, 8, 2, 2, 0, "HAD", (0, 0), 511)
    p.stage(0, p.off(0, 24, 8), 1, 24, 9, 16, 16, 1, 1, 1, "HAD", (2, 0), 511)
    p.stage(2, 4096, 1, 40, 40, 4, 8, 2, 0, 0, "SAD", (0, 0), 0b10101)
    p.stage(0, p.off(0, 8, 40), 1, 8, 41, 32, 128, 2, 2, 0, "HAD", (0, 0), 0b111)
    for k in range(6):                                                                  # six equal narrow units of 32 row groups: three bundles at the budget of 80, one at 320
        p.stage(0, p.off(0, 8 * k, 64), 1, 8 * k + 1, 63, 8, 16, 2, 2, 0, "HAD", (0, 0), 0b11)
    for k in range(70):
        p.item(0, p.off(0, k % 8, k % 5), 1, p.off(1, k % 7 - 3, k % 3), "SAD", 0, 64, 8)
    for k in range(6):
        p.item(0, p.off(0, 8, 8), 1, p.off(1, 9 + k, 7), ("HAD", "SSE", "HAD_2SAD")[k % 3], 0, (16, 8, 8)[k % 3], (8, 8, 8)[k % 3])
    w = (np.arange(1 << 12) % 9).astype(np.int16)
    mp = p.pool(w)
    for k in range(3):
        p.mask_item(0, p.off(0, 8, 8), 1, p.off(1, 5 + k, 11), mp, 32 * k, k % 2, 16, 8)
    return p


def long_plans():
    """the plans the tiers take on their own: 131 073 items, 8 195 stages"""
    return family_e_long() + [q for bd in (10, 8) for q in family_d_unsplit(bd)[:2]]


def all_plans():
    """every plan of families A .. F (not the long ones of D and E, which the tiers take on their own)"""
    out = family_a() + family_b() + family_c()
    for bd in (10, 8):
        out += [family_d_sweep(bd), family_d_shapes(bd)] + family_d_bundles(bd)
    out += family_e_runs() + family_e_classes() + family_f() + [compact_plan()]
    return out


def stage_read_box(s):
    """(x0, y0, x1, y1) relative to the block at ref_off: a bound on what stageBody fetches — one sample of displacement, the taps 3 to the left / above and 4 to the right /
    below, and the 16-byte chunks a row is fetched in (8 samples left of the unit, 16 beyond it)"""
    return -1 - 3 - 8, -1 - 4, int(s["width"]) + 1 + 4 + 16, int(s["height"]) + 1 + 4
