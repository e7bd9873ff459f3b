"""bench.py --dump-outputs DIR: what the timed path computed in its last step — the results a caller of the replayed picture's launches receives — as DIR/<name>.npy.

The recorded lists hold the same calls from one recording to the next (the encoder is deterministic), but the recorder merges its worker threads' logs in the order the threads
met the picture, so list positions and pool offsets differ between recordings.  Every output array is therefore written in an order keyed by the inputs of its rows: plane
identities (kind, POC, component) instead of plane indices, a fixed linear hash of the samples instead of a pool offset, then the job's own fields; rows with equal inputs are
ordered by their outputs.  Two builds that compute the same values on the same clip write the same files.

  me_integer_costs     (n,)    integer-candidate costs of the motion-search windows
  me_subpel_costs      (n, 9)  refinement-stage costs (positions the encoder did not evaluate: 0)
  table_call_costs     (n,)    plain distortion table calls;  masked_sad_costs (n,): the masked SADs
  tu_stats             (n, 4)  per TU: abs_sum, last_scan_pos (0 when abs_sum is 0), need_rdoq, sse
  tu_levels, tu_reconstruction  the coefficients of the TUs in tu_stats' order, concatenated (0 where abs_sum is 0: the caller reads neither)
  dmvr                 (n, 3)  per sub-block: mvd_x, mvd_y, min_cost
A class the picture has no work of (masked SADs outside GEO, DMVR and motion search in the intra picture) writes no file: an empty array is no output.
Costs as float64 (exact below 2^53), samples as float32.  Over BUDGET_BYTES in all, the TU coefficients are a fixed seeded sample of whole TUs (tu_sample: their rows in tu_stats).
Host logic apart from device_outputs(): tests/test_bench_outputs.py runs it on permuted lists without a device."""
import os

import numpy as np

BUDGET_BYTES = 60 * 1000 * 1000          # (64 MB read either way, .npy headers included)
_W = np.random.default_rng(0x5EED).integers(-(1 << 62), 1 << 62, size=128 * 128, dtype=np.int64)
_CHUNK = 1 << 14


def block_hash(pool, off, length):
    """one int64 per compact pool block (off, length samples): a fixed random linear form of its samples, mod 2^64"""
    off = np.asarray(off, np.int64).reshape(-1)
    length = np.broadcast_to(np.asarray(length, np.int64), off.shape)
    out = np.zeros(off.size, np.int64)
    pool = np.asarray(pool)
    for L in np.unique(length):
        sel = np.nonzero(length == L)[0]
        for a in range(0, sel.size, _CHUNK):
            s = sel[a:a + _CHUNK]
            blk = pool[off[s, None] + np.arange(int(L))].astype(np.int64)
            with np.errstate(over="ignore"):
                out[s] = blk @ _W[:int(L)]
    return out


def _plane_cols(lists, plane):
    """(kind, poc, comp) of plane indices; the pool entry: (-1, -1, -1)"""
    plane = np.asarray(plane, np.int64)
    pp = lists.pic.planes
    idx = np.clip(plane, 0, len(pp) - 1)
    pool = plane >= lists.n_pic_planes
    return [np.where(pool, -1, pp[f][idx].astype(np.int64)) for f in ("kind", "poc", "comp")]


def _operand_cols(lists, plane, off, length):
    """an operand as columns that do not depend on list order: the plane's identity and the offset in it, or a pool block's hash"""
    plane, off = np.asarray(plane, np.int64), np.asarray(off, np.int64)
    pool = plane == lists.pool_index
    h = block_hash(lists.pool, np.where(pool, off, 0), length) if pool.any() else np.zeros(off.size, np.int64)
    return _plane_cols(lists, plane) + [np.where(pool, h, off)]


def _order(keys, outs=()):
    """rows sorted by the key columns, then by the outputs (ties of equal inputs)"""
    cols = [np.asarray(k).reshape(-1) for k in keys]
    for o in outs:
        o = np.asarray(o)
        cols += [o] if o.ndim == 1 else [o[:, j] for j in range(o.shape[1])]
    if not cols or cols[0].size == 0:
        return np.zeros(0, np.int64)
    return np.lexsort(cols[::-1])


def canonical(lists, raw):
    """lists: a RecordedLists (vvenc_amd/replay.py); raw: the outputs in list order (device_outputs) -> {name: array} in the input-keyed order"""
    out = {}
    # ---- integer candidates of the window jobs
    jobs, pc = lists.int_jobs, lists.plan_cands
    cost = np.asarray(raw["cand"], np.uint64)[:pc.size]
    j = np.repeat(np.arange(jobs.size), jobs["n_cand"].astype(np.int64)) if jobs.size else np.zeros(0, np.int64)
    w, h = jobs["width"].astype(np.int64)[j], jobs["height"].astype(np.int64)[j]
    keys = _operand_cols(lists, jobs["org_plane"][j], jobs["org_off"][j], w * h) + _plane_cols(lists, jobs["ref_plane"][j]) + \
        [jobs["ref_off"][j], w, h, jobs["sub_shift"][j], pc["dx"], pc["dy"]]
    out["me_integer_costs"] = cost[_order(keys, [cost])].astype(np.float64)
    # ---- refinement stages
    sj = lists.stage_jobs
    sc = np.asarray(raw["stage"], np.uint64)[:9 * sj.size].reshape(-1, 9)
    sc = np.where(lists.stage_evaluated, sc, 0).astype(np.uint64)
    w, h = sj["width"].astype(np.int64), sj["height"].astype(np.int64)
    keys = _operand_cols(lists, sj["org_plane"], sj["org_off"], w * h) + _plane_cols(lists, sj["ref_plane"]) + \
        [sj[f] for f in ("ref_off", "width", "height", "i_frac", "filter_mode", "alt_hpel", "func", "base_qx", "base_qy", "mask")]
    out["me_subpel_costs"] = sc[_order(keys, [sc])].astype(np.float64).reshape(-1, 9)
    # ---- table calls (plain, masked)
    it, mi = lists.items, lists.mask_items
    ic = np.asarray(raw["item"], np.uint64)[:it.size + mi.size]
    w, h = it["width"].astype(np.int64), it["height"].astype(np.int64)
    keys = _operand_cols(lists, it["org_plane"], it["org_off"], w * h) + _operand_cols(lists, it["cur_plane"], it["cur_off"], w * h) + \
        [it["func"], it["sub_shift"], w, h]
    c = ic[:it.size]
    out["table_call_costs"] = c[_order(keys, [c])].astype(np.float64)
    w, h = mi["width"].astype(np.int64), mi["height"].astype(np.int64)
    keys = _operand_cols(lists, mi["org_plane"], mi["org_off"], w * h) + _operand_cols(lists, mi["cur_plane"], mi["cur_off"], w * h) + \
        [block_hash(lists.pool, mi["mask_off"], w * (h >> mi["sub_shift"].astype(np.int64))), mi["sub_shift"], w, h]
    c = ic[it.size:]
    out["masked_sad_costs"] = c[_order(keys, [c])].astype(np.float64)
    # ---- DMVR sub-blocks
    d_rows, k_rows = [], []
    for g, res in zip(lists.dmvr_groups, raw["dmvr"]):
        itm = g["items"]
        d_rows.append(np.stack([res["mvd_x"], res["mvd_y"], res["min_cost"].astype(np.int64)], 1).astype(np.int64))
        k_rows.append(np.stack(_plane_cols(lists, np.full(g["n"], g["r0"])) + _plane_cols(lists, np.full(g["n"], g["r1"])) +
                               [itm[f] for f in ("ref0_off", "ref1_off", "frac0_x", "frac0_y", "frac1_x", "frac1_y")] + [np.full(g["n"], g["dx"]), np.full(g["n"], g["dy"])], 1).astype(np.int64))
    dres = np.concatenate(d_rows) if d_rows else np.zeros((0, 3), np.int64)
    keys = np.concatenate(k_rows) if k_rows else np.zeros((0, 14), np.int64)
    out["dmvr"] = dres[_order([keys[:, k] for k in range(keys.shape[1])], [dres])].astype(np.float64)
    # ---- TU lists: one row per TU over all groups
    st_rows, lv_rows, rc_rows, key_rows = [], [], [], []
    for g, r in zip(lists.tu_groups, raw["tu"]):
        n, wh = g["n"], g["w"] * g["h"]
        st = r["stats"]
        nz = st["abs_sum"] != 0
        st_rows.append(np.stack([st["abs_sum"], np.where(nz, st["last_scan_pos"], 0), st["need_rdoq"], st["sse"].astype(np.int64)], 1).astype(np.int64))
        lv_rows.append(np.where(nz[:, None], np.asarray(r["level"]).reshape(n, wh), 0))
        rc_rows.append(np.where(nz[:, None], np.asarray(r["rec"]).reshape(n, wh), 0))
        key_rows.append(np.stack([np.full(n, g["w"]), np.full(n, g["h"]), np.full(n, g["tr_hor"]), np.full(n, g["tr_ver"]), g["qf"][:, 0], g["qf"][:, 1],
                                  block_hash(lists.pool, g["off"], wh)], 1).astype(np.int64))
    stats = np.concatenate(st_rows) if st_rows else np.zeros((0, 4), np.int64)
    keys = np.concatenate(key_rows) if key_rows else np.zeros((0, 7), np.int64)
    order = _order([keys[:, k] for k in range(keys.shape[1])], [stats])
    out["tu_stats"] = stats[order].astype(np.float64)
    sizes = np.concatenate([np.full(g["n"], g["w"] * g["h"], np.int64) for g in lists.tu_groups]) if lists.tu_groups else np.zeros(0, np.int64)
    first = np.concatenate([[0], np.cumsum(sizes)[:-1]]) if sizes.size else sizes
    lv = np.concatenate([x.reshape(-1) for x in lv_rows]) if lv_rows else np.zeros(0, np.int16)
    rc = np.concatenate([x.reshape(-1) for x in rc_rows]) if rc_rows else np.zeros(0, np.int16)
    rows = order
    room = BUDGET_BYTES - sum(a.nbytes for a in out.values())          # (the rest is in `out` by now; levels + reconstruction as float32: 8 bytes a coefficient)
    if 8 * int(sizes.sum()) > room:
        take = np.random.default_rng(7).permutation(order.size)
        keep = np.cumsum(8 * sizes[order[take]]) <= room - 8 * order.size          # (room for tu_sample itself)
        rows_at = np.sort(take[keep])
        out["tu_sample"] = rows_at.astype(np.float64)
        rows = order[rows_at]
    sel = np.concatenate([first[k] + np.arange(sizes[k]) for k in rows]) if rows.size else np.zeros(0, np.int64)
    out["tu_levels"] = lv[sel].astype(np.float32)
    out["tu_reconstruction"] = rc[sel].astype(np.float32)
    return out


def device_outputs(wl):
    """the result buffers of a RecordedWorkload (vvenc_amd/replay.py) on the host, in list order"""
    import torch
    from vvenc_amd.hotpath import DMVR_RESULT_DTYPE, STATS_DTYPE
    torch.cuda.synchronize()
    return {"cand": wl.cand_cost.cpu().numpy().view(np.uint64), "stage": wl.stage_cost.cpu().numpy().view(np.uint64), "item": wl.item_cost.cpu().numpy().view(np.uint64),
            "tu": [{"stats": g["stats"].cpu().numpy().view(STATS_DTYPE).reshape(-1), "level": g["level"].cpu().numpy(), "rec": g["rec"].cpu().numpy()} for g in wl.tu_groups],
            "dmvr": [g["out"].cpu().numpy().view(DMVR_RESULT_DTYPE).reshape(-1) for g in wl.dmvr_groups]}


def write(directory, arrays):
    """DIR/<name>.npy for every array with at least one value (an empty one is no output) -> {name: shape}"""
    arrays = {k: a for k, a in arrays.items() if a.size}
    assert arrays and sum(a.nbytes for a in arrays.values()) <= BUDGET_BYTES, {k: a.nbytes for k, a in arrays.items()}
    os.makedirs(directory, exist_ok=True)
    for name, a in arrays.items():
        assert a.dtype in (np.float32, np.float64), (name, a.dtype)
        np.save(os.path.join(directory, name + ".npy"), a)
    return {k: list(a.shape) for k, a in arrays.items()}


def dump(wl, directory):
    """bench.py's --dump-outputs: the last step's outputs of the replayed picture `wl`"""
    return write(directory, canonical(wl.lists, device_outputs(wl)))
