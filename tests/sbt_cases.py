"""Inputs shared by the fixture driver and the CPU and GPU tiers of the SBT entries (vvhip_sbt_parts_batch / vvhip_sbt_tiles / vvhip_sbt_place_batch): residual content,
lists of CUs with the buffer they point into, candidates and the expected chain.  Everything here is numpy; the GPU tier uploads the buffers.  Expected values:
tests/sbt_ref.py; tests/test_sbt_cpu.py asserts what the lists cover."""
import numpy as np

import sbt_ref as SR

SENTINEL = -7
WEIGHTS = [1.0] + [2.0 ** (k / 3.0) for k in (-2, 1, 2, 4, -4)]      # RdCost::setDistortionWeight's 2^( dQP / 3 ): 1 and non-dyadic values


# ---- residual content: -> ( y, cb, cr ) int16 ----
def seeded(rng, w, h, bd):
    """a smooth part plus noise, |r| <= 2^bd - 1, chroma correlated with nothing"""
    top = (1 << bd) - 1
    out = []
    for c in range(3):
        ww, hh = (w, h) if c == 0 else (w // 2, h // 2)
        yy, xx = np.mgrid[0:hh, 0:ww]
        base = rng.normal(0, top / 8.0) + rng.normal(0, top / 6.0) * np.cos((xx + 0.5) * np.pi / ww) + rng.normal(0, top / 6.0) * np.cos((yy + 0.5) * np.pi / hh)
        out.append(np.clip(np.rint(base + rng.normal(0, top / 12.0, (hh, ww))), -top, top).astype(np.int16))
    return tuple(out)


def constant(w, h, v):
    return tuple(np.full(((h, w) if c == 0 else (h // 2, w // 2)), v, np.int16) for c in range(3))


def mirrored(rng, w, h, bd, axis):
    """left/right (axis 1) or top/bottom (axis 0) mirrored content: the two half modes across that axis tie exactly"""
    out = []
    for b in seeded(rng, w, h, bd):
        half = b[:, :b.shape[1] // 2] if axis == 1 else b[:b.shape[0] // 2, :]
        out.append(np.concatenate([half, np.flip(half, axis)], axis))
    return tuple(out)


def quarter(rng, w, h, bd, mode):
    """energy confined to the quarter that quad mode `mode` (4..7) codes"""
    out = []
    for c, b in enumerate(seeded(rng, w, h, bd)):
        x, y, tw, th = SR.coded_tile(b.shape[1], b.shape[0], mode)
        m = np.zeros_like(b)
        m[y:y + th, x:x + tw] = b[y:y + th, x:x + tw] | 1
        out.append(m)
    return tuple(out)


# ---- lists ----
class Listed:
    """items (SBT_ITEM_DTYPE) + the residual buffer they read + blocks[i] = ( y, cb, cr )"""

    def __init__(self, items, resi, blocks):
        self.items, self.resi, self.blocks = items, resi, blocks

    def view(self, buf, i, c):
        it = self.items[i]
        w, h = int(it["width"]) >> (c > 0), int(it["height"]) >> (c > 0)
        off, s = int(it[("y_off", "cb_off", "cr_off")[c]]), int(it["stride_c" if c else "stride_y"])
        return buf[off + s * np.arange(h)[:, None] + np.arange(w)[None, :]]

    def block_mask(self, only=None):
        m = np.zeros(self.resi.size, bool)
        for i in (range(len(self.items)) if only is None else only):
            it = self.items[i]
            for c in range(3):
                w, h = int(it["width"]) >> (c > 0), int(it["height"]) >> (c > 0)
                off, s = int(it[("y_off", "cb_off", "cr_off")[c]]), int(it["stride_c" if c else "stride_y"])
                m[off + s * np.arange(h)[:, None] + np.arange(w)[None, :]] = True
        return m

    def reordered(self, order):
        return Listed(self.items[order].copy(), self.resi, [self.blocks[i] for i in order])


def compact(specs, odd_gaps=False):
    """specs = ( allowed, ( y, cb, cr ) ) each -> Listed: every CU's Y, Cb and Cr block one after the other, row pitch = width; odd_gaps: a sentinel sample in front of some
    blocks, so that offsets are odd (2-byte accesses) or 4-byte aligned only"""
    items = np.zeros(len(specs), SR.SBT_ITEM_DTYPE)
    parts, at = [], 0
    for k, (allowed, blocks) in enumerate(specs):
        h, w = blocks[0].shape
        offs = []
        for c, b in enumerate(blocks):
            gap = (1 if (k + c) % 3 == 0 else 2 if (k + c) % 3 == 1 else 0) if odd_gaps else 0
            parts.append(np.full(gap, SENTINEL, np.int16)); at += gap
            offs.append(at)
            parts.append(np.ascontiguousarray(b, np.int16).reshape(-1)); at += b.size
        it = items[k]
        it["y_off"], it["cb_off"], it["cr_off"], it["stride_y"], it["stride_c"], it["width"], it["height"], it["sbt_allowed"] = offs[0], offs[1], offs[2], w, w // 2, w, h, allowed
    parts.append(np.full(8, SENTINEL, np.int16))
    return Listed(items, np.concatenate(parts), [b for (_, b) in specs])


def shelf_pack(sizes, pitch):
    where, x, y, shelf = [], 0, 0, 0
    for (w, h) in sizes:
        if x + w > pitch:
            x, y, shelf = 0, y + shelf, 0
        where.append((x, y))
        x += w
        shelf = max(shelf, h)
    return where, y + shelf


def planes(specs, pitch_y=264, pitch_c=135, odd=False):
    """specs as compact's -> Listed in a picture layout: a luma plane (pitch 264: a multiple of 8 that is no power of two), then a Cb and a Cr plane of an ODD pitch (135: the
    2-byte path) — sentinel between the blocks; odd: the luma blocks start one sample to the right"""
    where, rows = shelf_pack([(b[0].shape[1] + (2 if odd else 0), b[0].shape[0]) for (_, b) in specs], pitch_y)
    rows += rows & 1
    lum = np.full((rows, pitch_y), SENTINEL, np.int16)
    chr_ = np.full((2, rows // 2, pitch_c), SENTINEL, np.int16)
    items = np.zeros(len(specs), SR.SBT_ITEM_DTYPE)
    for k, ((allowed, (y, cb, cr)), (x0, y0)) in enumerate(zip(specs, where)):
        h, w = y.shape
        x0 += 1 if odd else 0
        y0 += y0 & 1
        lum[y0:y0 + h, x0:x0 + w] = y
        cx, cy = x0 // 2, y0 // 2
        chr_[0, cy:cy + h // 2, cx:cx + w // 2] = cb
        chr_[1, cy:cy + h // 2, cx:cx + w // 2] = cr
        it = items[k]
        base = lum.size
        it["y_off"], it["cb_off"], it["cr_off"] = y0 * pitch_y + x0, base + cy * pitch_c + cx, base + chr_[0].size + cy * pitch_c + cx
        it["stride_y"], it["stride_c"], it["width"], it["height"], it["sbt_allowed"] = pitch_y, pitch_c, w, h, allowed
    return Listed(items, np.concatenate([lum.reshape(-1), chr_.reshape(-1)]), [b for (_, b) in specs])


def mixed_specs(seed, n=72):
    """every size of SR.ALL_SIZES once with its full sbt_allowed, then small sizes (at most 16 x 16, where a wave holds several CUs) with seeded subsets; every seventh CU
    spans the whole int16 range, every eleventh is all zero; shuffled"""
    rng = np.random.default_rng(seed)
    specs = []
    small = [s for s in SR.ALL_SIZES if s[0] <= 16 and s[1] <= 16 and SR.allowed_of(*s)]
    sizes = [s for s in SR.ALL_SIZES if SR.allowed_of(*s)]
    while len(specs) < n:
        k = len(specs)
        w, h = sizes[k] if k < len(sizes) else small[int(rng.integers(len(small)))]
        full = SR.allowed_of(w, h)
        allowed = full if k < len(sizes) else int(rng.choice(SR.subsets_of(full)))
        if k % 7 == 3:
            blocks = tuple(rng.integers(-32768, 32768, b.shape).astype(np.int16) for b in constant(w, h, 0))
        elif k % 11 == 5:
            blocks = constant(w, h, 0)
        else:
            blocks = seeded(rng, w, h, 10 if k % 2 else 8)
        specs.append((allowed, blocks))
    return [specs[i] for i in rng.permutation(len(specs))]


def expected_parts(listed, chroma_weight):
    """-> ( uint64 [n, 3, 16], uint64 [n, 9], uint8 [n, 8] ) from the model"""
    n = len(listed.items)
    parts, est, order = np.zeros((n, 3, 16), np.uint64), np.zeros((n, 9), np.uint64), np.zeros((n, 8), np.uint8)
    for i, (y, cb, cr) in enumerate(listed.blocks):
        p = SR.part_sums(y, cb, cr)
        e, o = SR.estimate(p, y.shape[1], y.shape[0], int(listed.items[i]["sbt_allowed"]), chroma_weight)
        parts[i], est[i], order[i] = np.array(p, np.uint64), np.array(e, np.uint64), o
    return parts, est, order


def best_candidates(listed, order, per_cu=2):
    """the first per_cu modes of every CU's order -> [( cu, mode )]"""
    return [(i, int(m)) for i in range(len(listed.items)) for m in order[i][:per_cu] if int(m) != 255]


# ---- the chain ----
CHAIN_SIZES = [(8, 8)] * 6 + [(16, 16)] * 6 + [(16, 8)] * 4 + [(8, 16)] * 4 + [(32, 32)] * 3 + [(64, 16), (4, 64), (64, 4), (64, 64), (32, 8)]
CHAIN_QPS = ((30, 31, 32), (49, 50, 50))      # ( Y, Cb, Cr ) per run; at the second the flat CUs' tiles quantise to zero and the textured ones' do not (asserted by both tiers)


def chain_world(seed=99, bd=10):
    """the CUs of CHAIN_SIZES in the picture layout with seeded residuals — even CUs FLAT (noise of -2..2), odd ones textured — and two candidates per CU: all modes of the
    size cycled through.  -> dict: listed, candidates [( cu, mode )], bd"""
    rng = np.random.default_rng(seed)
    specs = []
    for k, (w, h) in enumerate(CHAIN_SIZES):
        blocks = tuple(rng.integers(-2, 3, b.shape).astype(np.int16) for b in constant(w, h, 0)) if k % 2 == 0 else seeded(rng, w, h, bd)
        specs.append((SR.allowed_of(w, h), blocks))
    L = planes(specs)
    cand, turn = [], 0
    for i, (allowed, _) in enumerate(specs):
        ms = SR.modes_of(allowed)
        for r in range(2):
            cand.append((i, ms[(turn + r * (len(ms) // 2)) % len(ms)]))
        turn += 1
    return dict(listed=L, candidates=cand, bd=bd)


_chain_cache = {}


def chain_expected(oracle, world, qps, irap=0, drop=()):
    """per candidate of chain_world and component: the coded tile's residual through the oracle's TU pipeline with the tile's transform types (levels, reconstruction,
    statistics), the placed block and its SSE against the CU's residual; computed once per QP triple.  drop = ( candidate, component ) pairs without coefficients."""
    key = (id(world), tuple(qps), irap, tuple(drop))
    if key in _chain_cache:
        return _chain_cache[key]
    out = []
    L = world["listed"]
    for k, (cu, mode) in enumerate(world["candidates"]):
        comps = []
        for c, blk in enumerate(L.blocks[cu]):
            h, w = blk.shape
            x, y, tw, th = SR.coded_tile(w, h, mode)
            th_, tv_ = SR.tr_types(L.blocks[cu][0].shape[1], L.blocks[cu][0].shape[0], mode) if c == 0 else (SR.DCT2, SR.DCT2)
            if (k, c) in drop:
                lev, rec, st = None, None, None
            else:
                lev, rec, st = oracle.tu_rdo(blk[y:y + th, x:x + tw], qps[c], irap, tr_hor=th_, tr_ver=tv_, bit_depth=world["bd"], is_luma=int(c == 0))
            placed = SR.place(rec if st is not None and st["abs_sum"] else None, w, h, mode)
            comps.append(dict(level=lev, tile_rec=rec, stats=st, placed=placed, sse=SR.sse(placed, blk), tile=(x, y, tw, th), types=(th_, tv_)))
        out.append(comps)
    _chain_cache[key] = out
    return out


# ---- placement lists ----
STATS_DTYPE = np.dtype([("abs_sum", "<i4"), ("last_scan_pos", "<i4"), ("need_rdoq", "<i4"), ("pad", "<i4"), ("sse", "<u8")])      # vvhip_tu_stats


def all_candidates(listed):
    """one candidate per CU, the modes its sbt_allowed holds cycling along the list -> [( cu, mode )]"""
    out = []
    for i, it in enumerate(listed.items):
        ms = SR.modes_of(int(it["sbt_allowed"]))
        out.append((i, ms[i % len(ms)]))
    return out


def place_world(listed, candidates, seed, tile_gaps=False, wide=False):
    """a placement list on `listed` (at most one candidate per CU: candidates of one CU share its block of the reconstruction).  Per candidate and component one of three
    states, cycling: coded (a seeded tile reconstruction, statistics with levels), no levels (abs_sum == 0: the tile's place in the buffer holds garbage that must not be
    read), dropped (stats_idx -1).  tile_gaps: some tiles start at odd samples.
    -> dict: items (SBT_PLACE_DTYPE), tile_rec, stats (STATS_DTYPE), blocks[k][c] = the expected component block, sse uint64 [n, 3]"""
    rng = np.random.default_rng(seed)
    items = np.zeros(len(candidates), SR.SBT_PLACE_DTYPE)
    tiles, stats, blocks, at = [], [], [], 0
    sse = np.zeros((len(candidates), 3), np.uint64)
    for k, (cu, mode) in enumerate(candidates):
        src = listed.items[cu]
        for name in ("y_off", "cb_off", "cr_off", "stride_y", "stride_c", "width", "height", "sbt_allowed"):
            items[k][name] = src[name]
        items[k]["mode"] = mode
        row = []
        for c in range(3):
            w, h = int(src["width"]) >> (c > 0), int(src["height"]) >> (c > 0)
            x, y, tw, th = SR.coded_tile(w, h, mode)
            state = (k + c) % 3 if k % 4 else 0
            t = (rng.integers(-32768, 32768, (th, tw)) if wide and k % 2 else rng.integers(-700, 701, (th, tw))).astype(np.int16)
            if state == 2:
                items[k]["stats_idx"][c], items[k]["tile_off"][c] = -1, (7 if k % 2 else 0)
            else:
                if tile_gaps and (k + c) % 3 != 1:
                    gap = 1 + (k + c) % 2 * 3
                    tiles.append(np.full(gap, SENTINEL, np.int16)); at += gap
                items[k]["stats_idx"][c], items[k]["tile_off"][c] = len(stats), at
                st = np.zeros((), STATS_DTYPE)
                st["abs_sum"], st["last_scan_pos"] = (0, -1) if state == 1 else (int(rng.integers(1, 900)), 3)
                stats.append(st)
                tiles.append(t.reshape(-1)); at += t.size
            blk = SR.place(t if state == 0 else None, w, h, mode)
            row.append(blk)
            sse[k][c] = SR.sse(blk, listed.blocks[cu][c])
        blocks.append(row)
    tiles.append(np.full(8, SENTINEL, np.int16))
    return dict(items=items, tile_rec=np.concatenate(tiles), stats=np.array(stats, STATS_DTYPE) if stats else np.zeros(1, STATS_DTYPE), blocks=blocks, sse=sse)
