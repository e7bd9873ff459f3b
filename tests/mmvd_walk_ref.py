"""Plain Python restatement of the visiting order of EncCu::addMmvdCandsToPruningList with EncCu::xCheckMMVDCand (EncoderLib/EncCu.cpp:2361-2447, :4116-4158) over costs that
are already there, of MergeItemList::insertMergeItemToList on the costs alone (:4444-4471) and of the conditions under which the reference's SATD stage predicts an MMVD
candidate with BDOF (EncCu.cpp:2225, CommonLib/InterPrediction.cpp:474-479) — what vvhip::MergeMmvdOps::walk and ::bdofCands are held against, and the packing of the
driver's records (tests/cpp/mmvd_shim_driver.cpp)."""
import numpy as np

MAX_DOUBLE = 1.7e+308
ADD_NUM = 64
MMVD_MAX_REFINE_NUM = 32

WALK_IN = np.dtype([("dist", "<u4", 64), ("bits_cost", "<f8", 64), ("list_cost", "<f8", 8), ("skip", "<u8"), ("n_list", "<i4"), ("mmvd", "<i4"), ("dis_num", "<i4"),
                    ("num_valid", "<i4"), ("mrg_cnd0", "<i4"), ("mrg_cnd1", "<i4"), ("max_tracking", "<i4"), ("pad", "<i4")])
WALK_OUT = np.dtype([("best_cost_offset", "<f8"), ("best_cost_merge", "<f8"), ("best_dir", "<i4"), ("count", "<i4"), ("tested", "u1", 64)])


class MergeItemList:
    """the costs of m_list"""

    def __init__(self, costs, max_tracking):
        self.m_list, self.max_tracking = [float(c) for c in costs], max_tracking

    def insert(self, cost):
        full = self.max_tracking > 0 and len(self.m_list) == self.max_tracking
        if not self.m_list:
            self.m_list.append(cost)
        elif full and cost >= self.m_list[-1]:
            return False
        else:
            if full:
                self.m_list.pop()
            at = next((k for k, c in enumerate(self.m_list) if cost < c), len(self.m_list))
            self.m_list.insert(at, cost)
        return True


def x_check_mmvd_cand(st, mmvd, temp_num, best_cost_list):
    """st: dict( val, best_dir, best_cost_offset, best_cost_merge ), changed in place as the reference changes its reference arguments -> 0, 1 or 2"""
    base_idx = st["val"] // MMVD_MAX_REFINE_NUM
    cand_cur = st["val"] - MMVD_MAX_REFINE_NUM * base_idx
    if mmvd > 2:
        if cand_cur % 4 == 0:
            if st["best_cost_offset"] >= st["best_cost_merge"] and cand_cur >= 4:
                if st["val"] > MMVD_MAX_REFINE_NUM:
                    return 2
                st["val"] = MMVD_MAX_REFINE_NUM
                if temp_num == st["val"]:
                    return 2
            st["best_cost_offset"] = MAX_DOUBLE
            st["best_cost_merge"] = best_cost_list
    if st["val"] == MMVD_MAX_REFINE_NUM:
        st["best_dir"] = 0
    if cand_cur >= 4:
        if cand_cur % 4 != st["best_dir"]:
            return 1
    return 0


def walk(dist, bits_cost, list_cost, mmvd, dis_num, num_valid, mrg_cnd0=0, mrg_cnd1=1, max_tracking=0, skip=0):
    """-> ( [ MmvdIdx::val tested, in order ], bestCostOffset, bestCostMerge, bestDir )"""
    items = MergeItemList(list_cost, max_tracking)
    mmvd_test_num = ADD_NUM if num_valid > 1 else ADD_NUM >> 1
    cur_list_size = len(items.m_list)
    st = dict(val=0, best_dir=0, best_cost_offset=MAX_DOUBLE, best_cost_merge=items.m_list[cur_list_size - 1])
    shift_cand_start = 0
    if mmvd == 4:
        if mrg_cnd0 > 1 and mrg_cnd1 > 1:
            mmvd_test_num = 0
        elif mrg_cnd0 > 1 or mrg_cnd1 > 1:
            shift_cand = mrg_cnd0 if mrg_cnd0 < 2 else mrg_cnd1
            if shift_cand:
                shift_cand_start = MMVD_MAX_REFINE_NUM
            else:
                mmvd_test_num = MMVD_MAX_REFINE_NUM
    tested = []
    cand = shift_cand_start
    while cand < mmvd_test_num:
        st["val"] = cand
        step = (cand >> 2) & 7
        if step >= dis_num:
            cand += 1
            continue
        if mmvd > 1:
            check = x_check_mmvd_cand(st, mmvd, mmvd_test_num, items.m_list[cur_list_size - 1])
            cand = st["val"]
            if check:
                if check == 2:
                    break
                cand += 1
                continue
        if (skip >> st["val"]) & 1:
            cand += 1
            continue
        cost = float(int(dist[st["val"]])) + float(bits_cost[st["val"]])
        tested.append(st["val"])
        items.insert(cost)
        if mmvd > 1 and cost < st["best_cost_offset"]:
            st["best_cost_offset"] = cost
            cand_cur = st["val"] - MMVD_MAX_REFINE_NUM * (st["val"] >> 5)
            if cand_cur < 4:
                st["best_dir"] = cand_cur
        cand += 1
    return tested, st["best_cost_offset"], st["best_cost_merge"], st["best_dir"]


def bdof_cands(w, h, bases, cur_poc, mmvd, bdof_enabled, bcw_enabled):
    """bases: per base dict( used=( l0, l1 ), poc=( p0, p1 ), lt=( t0, t1 ), bcw ) -> the 64-bit mask of candidates predicted with BDOF"""
    out = 0
    for val in range(ADD_NUM):
        b, step = val >> 5, (val >> 2) & 7
        s = bases[b]
        mcc_no_bdof = step > 2 or mmvd > 1                                                            # EncCu.cpp:2225
        inter_dir_3 = s["used"][0] and s["used"][1] and w + h != 12                                   # restrictBiPredMergeCandsOne
        eq_dist = inter_dir_3 and not s["lt"][0] and not s["lt"][1] and cur_poc - s["poc"][0] == s["poc"][1] - cur_poc
        if bdof_enabled and eq_dist and min(w, h) >= 8 and w * h >= 128 and not (bcw_enabled and s["bcw"] != 2) and not mcc_no_bdof:
            out |= 1 << val
    return out


def walk_cases():
    """cost arrays with ties, for m_MMVD 1 .. 4: WALK_IN records"""
    rng = np.random.default_rng(2026)
    out = []
    for k in range(240):
        r = np.zeros((), WALK_IN)
        kind = k % 6
        if kind == 0:
            r["dist"] = rng.integers(100, 108, 64)                      # many ties
        elif kind == 1:
            r["dist"] = 1000
        elif kind == 2:
            r["dist"] = rng.integers(0, 1 << 20, 64)
        elif kind == 3:
            r["dist"] = np.sort(rng.integers(0, 4000, 64))
        elif kind == 4:
            r["dist"] = np.sort(rng.integers(0, 4000, 64))[::-1]
        else:
            r["dist"] = rng.integers(0, 4000, 64) // 500 * 500
        r["bits_cost"] = rng.integers(0, 6, 64) * (0.5 if k % 4 else 0.0) * (37.25 if k % 3 else 1.0)
        n = int(rng.integers(1, 7))
        lo = int(r["dist"].min()) if k % 5 else int(np.median(r["dist"]))
        r["list_cost"][:n] = np.sort(rng.integers(lo, lo + (8 if kind < 2 else 3000), n)).astype(np.float64)
        if kind == 1 and k % 2:
            r["list_cost"][:n] = 1000.0                                  # the list ties with every candidate
        r["n_list"], r["mmvd"], r["dis_num"], r["num_valid"] = n, 1 + k % 4, (8, 6, 4, 3, 1)[k % 5], 1 + (k % 7 != 0)
        r["mrg_cnd0"], r["mrg_cnd1"] = ((0, 1), (1, 0), (0, 2), (2, 0), (1, 3), (3, 1), (2, 3), (0, 0))[(k // 4) % 8]
        if n == 1:
            r["mrg_cnd1"] = r["mrg_cnd0"]                                # a list of one item: the reference reads entry 0 twice
        r["max_tracking"] = (0, n, n + 2)[k % 3]
        r["skip"] = 0 if k % 8 else int(rng.integers(0, 1 << 63)) & int(rng.integers(0, 1 << 63))
        out.append(r)
    return np.array(out, WALK_IN)
