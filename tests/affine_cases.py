"""Inputs of the affine prediction tests (vvhip_pred_affine_batch), shared by the CPU guards (tests/test_affine_cpu.py) and the GPU tier (tests/test_gpu_pred_affine.py):
worlds of reference planes (numpy only here) and seeded lists of CU records.

Input family (measured on the reference alone before the kernel existed): RT - LT components uniform in +-D * w / 16, LB - LT components uniform in +-D * h / 16, in 1/16 sample.
D = 32: PROF changes > 99 % of the CUs, none over the spread limit, 56-60 % under the search threshold.  D = 256: about a quarter of the CUs over the spread limit."""
import os

import numpy as np

import affine_ref as AR

PIC_W, PIC_H = 256, 192
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "affine.npz")
ITEM_DTYPE = np.dtype([("dst_off", "<i4"), ("org_off", "<i4"), ("ref_off", "<i4", (2,)), ("cpmv", "<i4", (2, 3, 2)), ("cu_x", "<i2"), ("cu_y", "<i2"), ("cu_w", "<i2"),
                       ("cu_h", "<i2"), ("ref_plane", "i1", (2,)), ("chroma", "u1"), ("six_param", "u1"), ("prof", "u1"), ("rsv", "u1", (3,))])      # vvhip_pred_affine_item


def _texture(rng, h, w, bd, shift):
    yy, xx = np.mgrid[0:h, 0:w]
    top = (1 << bd) - 1
    return np.clip(top / 2 + top / 4 * np.sin((xx + shift) / 6.0) * np.cos((yy - shift) / 5.0) + rng.normal(0, top / 25, (h, w)), 0, top).astype(np.int16)


class World:
    """reference planes of one bit depth for a PIC_W x PIC_H picture with the reference encoder's own margin of ctu + 16 luma samples on every side (+ one spare row: the
    aligned-dword rule): planes 0, 1 luma, 2, 3 chroma (4:2:0), and an original plane per component.
    kind: "texture" (smooth + noise), "zero", "max", "checker" (0 / max: the first plane of a component sample by sample, the second in cells of 2 x 2)"""

    def __init__(self, bd, ctu, kind="texture", seed=1, pic_w=PIC_W, pic_h=PIC_H, margin=None):
        rng = np.random.default_rng(seed)
        self.bd, self.ctu, self.pic_w, self.pic_h = bd, ctu, pic_w, pic_h
        self.m = ctu + 16 if margin is None else margin
        top = (1 << bd) - 1
        lh, lw, ch, cw = pic_h + 2 * self.m + 1, pic_w + 2 * self.m, pic_h // 2 + self.m + 1, pic_w // 2 + self.m

        def make(h, w, shift):
            if kind == "texture":
                return _texture(rng, h, w, bd, shift)
            if kind == "checker":
                yy, xx = np.mgrid[0:h, 0:w]
                cell = 0 if shift < 2 else 1          # the second plane of a component: cells of 2 x 2 (there sample x - 1 and sample x + 1 always differ: full gradients)
                return ((((xx >> cell) + (yy >> cell)) & 1) * top).astype(np.int16)
            return np.full((h, w), top if kind == "max" else 0, np.int16)
        self.np = [make(lh, lw, 0), make(lh, lw, 3), make(ch, cw, 1), make(ch, cw, 6)]
        self.org_np = [np.clip(self.np[0].astype(np.int32) + rng.integers(-12, 13, self.np[0].shape), 0, top).astype(np.int16),
                       np.clip(self.np[2].astype(np.int32) + rng.integers(-12, 13, self.np[2].shape), 0, top).astype(np.int16)]

    def origin(self, chroma):
        """(x, y) of the picture's first sample inside a plane of the component"""
        return (self.m // 2, self.m // 2) if chroma else (self.m, self.m)

    def block_pos(self, it):
        c = int(it["chroma"])
        ox, oy = self.origin(c)
        return ox + (int(it["cu_x"]) >> c), oy + (int(it["cu_y"]) >> c)

    def place(self, it):
        """fills ref_off / org_off of an item from its CU position (plane indices must be set); -> pos per list for affine_ref.expected_block"""
        x, y = self.block_pos(it)
        pos = [None, None]
        for l in (0, 1):
            p = int(it["ref_plane"][l])
            if p >= 0:
                it["ref_off"][l] = y * self.np[p].shape[1] + x
                pos[l] = (x, y)
        it["org_off"] = y * self.org_np[int(it["chroma"])].shape[1] + x
        return pos


def _cu(rng, w, h, x, y, six, lists, prof, D, lt_range=320, lt=None):
    """-> (luma item, chroma item) of one CU; lists: 0 = list 0 only, 1 = list 1 only, 2 = both"""
    it = np.zeros((), ITEM_DTYPE)
    it["cu_x"], it["cu_y"], it["cu_w"], it["cu_h"], it["six_param"], it["prof"] = x, y, w, h, six, prof
    for l in (0, 1):
        if lists != 2 and lists != l:
            it["ref_plane"][l] = -1
            continue
        it["ref_plane"][l] = int(rng.integers(0, 2))
        a = np.array(lt[l] if lt is not None else rng.integers(-lt_range, lt_range + 1, 2))
        dw, dh = D * w // 16, D * h // 16
        it["cpmv"][l][0] = a
        it["cpmv"][l][1] = a + rng.integers(-dw, dw + 1, 2)
        it["cpmv"][l][2] = a + rng.integers(-dh, dh + 1, 2)
    ch = it.copy()
    ch["chroma"] = 1
    ch["ref_plane"] = [p + 2 if p >= 0 else -1 for p in it["ref_plane"]]
    return it, ch


def finish(world, recs):
    """-> (items, pos) with ref_off / org_off filled"""
    items = np.concatenate([r.reshape(1) for r in recs])
    pos = [world.place(items[k]) for k in range(len(items))]
    return items, pos


def size_list(world, D, seed, reps=2):
    """every CU size 8..128 x 8..128, luma and chroma; the model, the lists used and prof cycle through all 24 combinations, shifted per list so that the four lists of the
    GPU tier (two bit depths x two D) show each size other combinations"""
    rng = np.random.default_rng(seed)
    recs, k = [], seed
    for (w, h) in AR.SIZES:
        for _ in range(reps):
            x, y = 8 * int(rng.integers(0, (world.pic_w - w) // 8 + 1)), 8 * int(rng.integers(0, (world.pic_h - h) // 8 + 1))
            recs += _cu(rng, w, h, x, y, k & 1, (k >> 1) % 3, (k // 6) % 4, D)
            k += 1
    return finish(world, recs)


def edge_list(world, seed):
    """CUs at the four edges and the four corners of the picture whose vectors point more than ctu samples outward: the picture clip moves every one of them"""
    rng = np.random.default_rng(seed)
    ctu, recs, k = world.ctu, [], 0
    out = (ctu + 40) * 16
    for (w, h) in ((8, 8), (ctu, ctu), (16, 8), (8, 32)):
        for ex in (-1, 0, 1):
            for ey in (-1, 0, 1):
                if ex == 0 and ey == 0:
                    continue
                x = 0 if ex < 0 else world.pic_w - w if ex > 0 else 8 * int(rng.integers(1, (world.pic_w - w) // 8))
                y = 0 if ey < 0 else world.pic_h - h if ey > 0 else 8 * int(rng.integers(1, (world.pic_h - h) // 8))
                lt = [(ex * out + int(rng.integers(-64, 65)), ey * out + int(rng.integers(-64, 65))) for _ in (0, 1)]
                recs += _cu(rng, w, h, x, y, k & 1, (k >> 1) % 3, 1 if k % 4 else 0, 32, lt=lt)
                k += 1
    return finish(world, recs)


def extreme_list(world, seed):
    """zooms and shears strong enough to drive the dMv table to +-31 without passing the spread limit (on the checkerboard the gradients then drive dI into its clip),
    besides ordinary D = 32 CUs; uni and bi, both models, prof 1"""
    rng = np.random.default_rng(seed)
    recs, k = [], 0
    for (w, h) in ((16, 16), (8, 32), (32, 8), (64, 16)):
        for (zx, zy) in ((11, 0), (-11, 0), (0, 11), (0, -11), (11, 11), (-11, 11)):
            x, y = 8 * int(rng.integers(2, (world.pic_w - w) // 8 - 1)), 8 * int(rng.integers(2, (world.pic_h - h) // 8 - 1))
            lu, ch = _cu(rng, w, h, x, y, k & 1, (k >> 1) % 3, 1, 0, lt_range=160)
            for it in (lu, ch):
                for l in (0, 1):
                    a = it["cpmv"][l][0].copy()
                    it["cpmv"][l][1] = a + np.array([zx * w, zy * w])          # ( RT - LT ) << ( 7 - log2 w ) = 128 * z: |dMv| reaches 6 * 128 * 11 >> 8 = 33 > 31, and a bi-predicted pure zoom of 11 / 16 stays under the spread limit
                    it["cpmv"][l][2] = a + np.array([-zy * h, zx * h])
            recs += [lu, ch]
            k += 1
        x, y = 8 * int(rng.integers(0, (world.pic_w - w) // 8 + 1)), 8 * int(rng.integers(0, (world.pic_h - h) // 8 + 1))
        recs += _cu(rng, w, h, x, y, k & 1, 2, 1, 32)
    return finish(world, recs)


def compact_offsets(items):
    sizes = (items["cu_w"].astype(np.int64) >> items["chroma"]) * (items["cu_h"].astype(np.int64) >> items["chroma"])
    off = np.concatenate([[0], np.cumsum(sizes)[:-1]])
    return off.astype(np.int32), int(sizes.sum())


# the four lists of the GPU tier's size test: (bit depth, D, seed); the CPU guards check what they exercise
TIER_LISTS = [(8, 32, 11), (8, 256, 12), (10, 32, 13), (10, 256, 14)]


def golden_cases():
    """-> (hdr, planes per bit depth {bd: [y0, y1, c0, c1]}, list of (bd, luma item, chroma item, pos per component, {row: {(l, chroma): block}}))"""
    g = np.load(GOLDEN)
    pic_w, pic_h, ctu, margin = (int(v) for v in g["hdr"])

    def spare(a):          # one spare row: the aligned-dword rule of the device planes
        return np.concatenate([a, a[-1:]]).astype(np.int16)
    p10 = [spare(g["y0"]), spare(g["y1"]), spare(g["c0"]), spare(g["c1"])]
    planes = {10: p10, 8: [(a >> 2).astype(np.int16) for a in p10]}
    out, at = [], 0
    for c in g["cases"]:
        bd, x, y, w, h, six, inter_dir, prof = (int(v) for v in c[:8])
        lu = np.zeros((), ITEM_DTYPE)
        lu["cu_x"], lu["cu_y"], lu["cu_w"], lu["cu_h"], lu["six_param"], lu["prof"] = x, y, w, h, six, prof
        lu["cpmv"] = c[10:22].reshape(2, 3, 2)
        lu["ref_plane"] = [int(c[8 + l]) if inter_dir & (1 << l) else -1 for l in (0, 1)]
        ch = lu.copy()
        ch["chroma"] = 1
        ch["ref_plane"] = [p + 2 if p >= 0 else -1 for p in lu["ref_plane"]]
        pos = {0: [(margin + x, margin + y)] * 2, 1: [(margin // 2 + x // 2, margin // 2 + y // 2)] * 2}
        for it, cc in ((lu, 0), (ch, 1)):
            for l in (0, 1):
                if it["ref_plane"][l] >= 0:
                    it["ref_off"][l] = pos[cc][l][1] * planes[10][int(it["ref_plane"][l])].shape[1] + pos[cc][l][0]
        rec = {"scalar": {}, "simd": {}}
        n = (w * h + w * h // 4) * (2 if inter_dir == 3 else 1)
        for row in ("scalar", "simd"):
            a = at
            for l in (0, 1):
                if inter_dir & (1 << l):
                    rec[row][(l, 0)] = g[row][a:a + w * h].reshape(h, w); a += w * h
                    rec[row][(l, 1)] = g[row][a:a + w * h // 4].reshape(h // 2, w // 2); a += w * h // 4
        at += n
        out.append((bd, lu, ch, pos, rec))
    assert at == g["scalar"].size == g["simd"].size
    return (pic_w, pic_h, ctu, margin), planes, out
