"""Inputs shared by the CPU and GPU tiers of the joint Cb-Cr entries (vvhip_ict_fwd_batch / vvhip_ict_inv_batch): lists of items with the buffers they point into, in
both layouts.  Everything here is numpy; the GPU tier uploads the buffers.  Expected values: tests/ict_ref.py; tests/test_ict_cpu.py asserts what the lists cover.
  compact : every Cb block and every Cr block one after the other in one buffer, row pitch = width
  planes  : one buffer of two planes of a shared row pitch, the Cb blocks shelf-packed in the first and each Cr block at the same position of the second
The joint blocks are always compact, in list order (an item of mode 0 has none and takes no room)."""
import numpy as np

import ict_ref as IR

ICT_ITEM_DTYPE = IR.ICT_ITEM_DTYPE
SENTINEL = -7
PLANE_PITCH = 264          # a multiple of 8 that is no power of two


class Listed:
    """items + the residual buffer they read + where each block is: blocks[i] = ( cb, cr ) the h x w inputs"""

    def __init__(self, items, resi, blocks, joint_total):
        self.items, self.resi, self.blocks, self.joint_total = items, resi, blocks, joint_total

    def view(self, buf, off, i):
        """the h x w block of item i at sample offset `off` of a buffer laid out like the residual"""
        it = self.items[i]
        w, h, s = int(it["width"]), int(it["height"]), int(it["stride"])
        idx = off + s * np.arange(h)[:, None] + np.arange(w)[None, :]
        return buf[idx]

    def cb(self, buf, i):
        return self.view(buf, int(self.items[i]["cb_off"]), i)

    def cr(self, buf, i):
        return self.view(buf, int(self.items[i]["cr_off"]), i)

    def joint(self, buf, i):
        it = self.items[i]
        w, h, o = int(it["width"]), int(it["height"]), int(it["joint_off"])
        return buf[o:o + w * h].reshape(h, w)

    def block_mask(self):
        """True on every sample of the residual layout that belongs to a block"""
        m = np.zeros(self.resi.size, bool)
        for i, it in enumerate(self.items):
            w, h, s = int(it["width"]), int(it["height"]), int(it["stride"])
            idx = s * np.arange(h)[:, None] + np.arange(w)[None, :]
            m[int(it["cb_off"]) + idx] = True
            m[int(it["cr_off"]) + idx] = True
        return m

    def joint_mask(self):
        m = np.zeros(max(self.joint_total, 1), bool)
        for it in self.items:
            if int(it["mode"]) != 0:
                m[int(it["joint_off"]):int(it["joint_off"]) + int(it["width"]) * int(it["height"])] = True
        return m

    def reordered(self, order):
        return Listed(self.items[order].copy(), self.resi, [self.blocks[i] for i in order], self.joint_total)


def _joint_offsets(items, odd_gaps=False):
    at = 0
    for k in range(len(items)):
        items[k]["joint_off"] = at
        if int(items[k]["mode"]) != 0:
            at += int(items[k]["width"]) * int(items[k]["height"])
            if odd_gaps and k % 5 == 2:
                at += 1          # every fifth joint block starts at an odd sample: narrower vectors
    return at


def compact(specs, odd_gaps=False):
    """specs = ( mode, cb, cr ) each -> Listed in the compact layout"""
    items = np.zeros(len(specs), ICT_ITEM_DTYPE)
    parts, at = [], 0
    for k, (mode, cb, cr) in enumerate(specs):
        h, w = cb.shape
        if odd_gaps and k % 7 == 3:
            parts.append(np.full(1, SENTINEL, np.int16)); at += 1
        items[k]["cb_off"], items[k]["cr_off"], items[k]["stride"], items[k]["width"], items[k]["height"], items[k]["mode"], items[k]["stats_idx"] = at, at + w * h, w, w, h, mode, -1
        parts += [np.ascontiguousarray(cb, np.int16).reshape(-1), np.ascontiguousarray(cr, np.int16).reshape(-1)]
        at += 2 * w * h
    total = _joint_offsets(items, odd_gaps)
    return Listed(items, np.concatenate(parts), [(cb, cr) for (_, cb, cr) in specs], total)


def shelf_pack(sizes, pitch):
    """first-fit shelves in list order -> ( [( x, y )], rows )"""
    where, x, y, shelf = [], 0, 0, 0
    for (w, h) in sizes:
        if x + w > pitch:
            x, y, shelf = 0, y + shelf, 0
        where.append((x, y))
        x += w
        shelf = max(shelf, h)
    return where, y + shelf


def planes(specs, pitch=PLANE_PITCH):
    """specs = ( mode, cb, cr ) each -> Listed in the plane layout: Cb plane, then Cr plane, SENTINEL between the blocks"""
    where, rows = shelf_pack([(cb.shape[1], cb.shape[0]) for (_, cb, _) in specs], pitch)
    buf = np.full((2 * rows, pitch), SENTINEL, np.int16)
    items = np.zeros(len(specs), ICT_ITEM_DTYPE)
    for k, ((mode, cb, cr), (x, y)) in enumerate(zip(specs, where)):
        h, w = cb.shape
        buf[y:y + h, x:x + w] = cb
        buf[rows + y:rows + y + h, x:x + w] = cr
        items[k]["cb_off"], items[k]["cr_off"], items[k]["stride"], items[k]["width"], items[k]["height"], items[k]["mode"], items[k]["stats_idx"] = y * pitch + x, (rows + y) * pitch + x, pitch, w, h, mode, -1
    total = _joint_offsets(items)
    return Listed(items, buf.reshape(-1), [(cb, cr) for (_, cb, cr) in specs], total)


def _blocks(rng, w, h, wide):
    """two residual blocks: 10-bit residual range, or (wide) the whole int16 range"""
    if wide:
        return tuple(rng.integers(-32768, 32768, (h, w)).astype(np.int16) for _ in range(2))
    a = rng.integers(-1023, 1024, (h, w))
    b = np.clip(rng.choice([-1, 1]) * a // rng.choice([1, 2]) + rng.integers(-90, 91, (h, w)), -1023, 1023)
    return a.astype(np.int16), b.astype(np.int16)


def mixed_specs(seed, with_zero=True, n=200):
    """about 200 items over all 36 sizes and all modes: every size once with the mode cycling, then small sizes (at most 16x16) with seeded modes; every ninth item spans the
    int16 range; with_zero: some items of mode 0 (forward only)"""
    rng = np.random.default_rng(seed)
    modes = IR.MODES + ((0,) if with_zero else ())
    specs = []
    for k, (w, h) in enumerate(IR.SIZES):
        specs.append((modes[k % len(modes)],) + _blocks(rng, w, h, k % 9 == 4))
    small = [s for s in IR.SIZES if s[0] <= 16 and s[1] <= 16]
    while len(specs) < n:
        w, h = small[int(rng.integers(len(small)))]
        specs.append((modes[int(rng.integers(len(modes)))],) + _blocks(rng, w, h, len(specs) % 9 == 4))
    return specs


def golden_specs(cases):
    return [(c["mode"], c["cb"], c["cr"]) for c in cases]


def expected_fwd(listed):
    """-> ( [joint block or None], int64 [n, 2] ) from the model"""
    joints, dist = [], np.zeros((len(listed.items), 2), np.int64)
    for i, (cb, cr) in enumerate(listed.blocks):
        j, d1, d2 = IR.fwd(cb, cr, int(listed.items[i]["mode"]))
        joints.append(j)
        dist[i] = (d1, d2)
    return joints, dist


def expected_inv(listed, joint_blocks):
    """-> ( [( rec_cb, rec_cr )], uint64 [n, 2] ) from the model: the SSEs are against the list's own blocks"""
    recs, sse = [], np.zeros((len(listed.items), 2), np.uint64)
    for i, (cb, cr) in enumerate(listed.blocks):
        a, b = IR.inv(joint_blocks[i], int(listed.items[i]["mode"]))
        recs.append((a, b))
        sse[i] = (IR.sse(a, cb), IR.sse(b, cr))
    return recs, sse


# ---- the chain: chroma TUs whose residual comes from the prediction list ----
CHAIN_SIZES = [(4, 4)] * 6 + [(8, 8)] * 5 + [(16, 8)] * 5
CHAIN_QPS = (27, 45)          # the joint QP per run; at 45 the flat TUs quantise to zero and the textured ones do not (asserted by both tiers)


def chain_world(seed=77, bd=10):
    """the chroma TUs of CHAIN_SIZES as a prediction list with the residual: two items per TU (Cb from reference plane 0, Cr from plane 1, uni-predicted, chroma taps),
    the residual compact — Cb block, then Cr block — so that a TU's ICT item names the two dst_off with pitch = width.  Even TUs are FLAT: a zero fraction and an original
    that is the reference block plus noise of -1..1 (the joint residual quantises to nothing at any QP used); odd TUs are TEXTURED: a fractional vector and an original with
    a strong pattern of its own.  The original plane holds the Cb picture in its left half and the Cr picture in its right half (one pitch per call).
    -> dict: planes (2 numpy planes), org (numpy plane), pred_items, pos, ict_items (modes cycling over the six), joint_total"""
    from blend_cases import PRED_ITEM_DTYPE
    rng = np.random.default_rng(seed)
    H, W, top = 64, 96, (1 << bd) - 1
    yy, xx = np.mgrid[0:H, 0:W]
    ref = [np.clip(512 + 260 * np.sin(xx / (7.0 + 3 * c)) * np.cos(yy / (5.0 + 2 * c)) + rng.normal(0, 12, (H, W)), 0, top).astype(np.int16) for c in (0, 1)]
    org = np.zeros((H, 2 * W), np.int16)
    where, _ = shelf_pack([(w + 8, h + 8) for (w, h) in CHAIN_SIZES], W - 8)
    pit = np.zeros(2 * len(CHAIN_SIZES), PRED_ITEM_DTYPE)
    ict = np.zeros(len(CHAIN_SIZES), ICT_ITEM_DTYPE)
    pos, at = [], 0
    for k, ((w, h), (x0, y0)) in enumerate(zip(CHAIN_SIZES, where)):
        x, y = x0 + 6, y0 + 4
        assert y + h + 4 <= H and x + w + 4 <= W
        textured = k % 2 == 1
        delta = rng.integers(-160, 161, (h, w)) if textured else rng.integers(-1, 2, (h, w))
        for c in (0, 1):
            it = pit[2 * k + c]
            it["width"], it["height"], it["chroma"], it["ref_plane"], it["ref_off"][0], it["dst_off"], it["org_off"] = w, h, 1, (c, -1), y * W + x, at, y * 2 * W + c * W + x
            it["frac"][0] = (int(rng.integers(1, 32)), int(rng.integers(0, 32))) if textured else (0, 0)
            org[y:y + h, c * W + x:c * W + x + w] = np.clip(ref[c][y:y + h, x:x + w].astype(np.int32) + (delta if c == 0 else -delta // 2 + rng.integers(-1, 2, (h, w))), 0, top)
            pos.append(((x, y), None))
            at += w * h
        ict[k]["cb_off"], ict[k]["cr_off"], ict[k]["stride"], ict[k]["width"], ict[k]["height"], ict[k]["mode"], ict[k]["stats_idx"] = at - 2 * w * h, at - w * h, w, w, h, IR.MODES[k % 6], -1
    return dict(planes=ref, org=org, pred_items=pit, pos=pos, ict_items=ict, resi_total=at, bd=bd)


_chain_cache = {}


def chain_expected(oracle, world, qp, irap=0):
    """per TU of chain_world: the residuals (the original minus the oracle's prediction), the model's joint block and pair distortion, the oracle's TU pipeline on the joint
    block at the chroma scale (levels, joint reconstruction, statistics), the model's two reconstructions and their SSEs; computed once per QP"""
    import pred_ref as PR
    key = (id(world), qp, irap)
    if key in _chain_cache:
        return _chain_cache[key]
    out, ow = [], world["org"].shape[1]
    for k, ict in enumerate(world["ict_items"]):
        resi = []
        for c in (0, 1):
            it = world["pred_items"][2 * k + c]
            oy, ox = divmod(int(it["org_off"]), ow)
            pred = PR.expected_block(oracle, world["planes"], world["pos"][2 * k + c], it, world["bd"])
            resi.append(PR.residual(world["org"][oy:oy + int(it["height"]), ox:ox + int(it["width"])], pred))
        mode = int(ict["mode"])
        joint, d1, d2 = IR.fwd(resi[0], resi[1], mode)
        lev, jrec, st = oracle.tu_rdo(joint, qp, irap, bit_depth=world["bd"], is_luma=0)
        a, b = IR.inv(jrec, mode)
        out.append(dict(cb=resi[0], cr=resi[1], joint=joint, dist=(d1, d2), level=lev, joint_rec=jrec, stats=st, rec_cb=a, rec_cr=b, sse=(IR.sse(a, resi[0]), IR.sse(b, resi[1]))))
    _chain_cache[key] = out
    return out
