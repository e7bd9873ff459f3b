"""Seeded pictures with legal loop-filter maps, shared by the fixture generator (tests/deblock_golden_gen.py), the CPU tier (tests/test_deblock_cpu.py), the GPU tier
(tests/test_gpu_deblock.py, tests/test_gpu_deblock_shim.py), smoke() and tools/deblock_time.py.

A picture is split CTU by CTU into blocks of 4 .. CTU samples per side (a random quad / binary split; blocks that would cross the picture's border are split further).
The maps are what calcFilterStrengths would leave for such a partitioning (CommonLib/LoopFilter.cpp):
  - the left / top border of every block is a transform edge with the lengths of xSetMaxFilterLengthPQFromTransformSizes (:895-913): 1 / 1 where a side is 4 samples, else
    7 on a side of >= 32 samples (5 on the P side where that block is an affine one) and 3 otherwise; the chroma flag filterCMFL where both sides have >= 8 chroma samples (:916)
  - some blocks are "affine": they carry sub-block edges on the 8-sample grid with the lengths of xSetMaxFilterLengthPQForCodingSubBlocks (:932-995): the Q side of their
    own border drops to 5, the inner edges get 2 next to the borders (and at 8) and 3 elsewhere
  - bS 0..2 per component and record, the QP of an edge the rounded mean of its two blocks' QPs, which are drawn from a list with -12, 0, 17 and 63 in it
Such maps are legal: no edge of a direction writes a sample another edge of that direction reads or writes (tests/test_deblock_cpu.py shows it by shuffling).
Sample content is per block, on top of a level that changes slowly over the picture and sits at 0 or 2^bd - 1 in some regions: flat blocks a small step apart (strong and
long filters), steps around tc and 10 tc, ramps, light noise (second samples on one side only), heavy noise (d >= beta), the two ends of the sample range.

LAYOUTS    ( base offset in samples, extra pitch ) the GPU tier hands the planes over with, as tests/sao_cases.py has them."""
import numpy as np

import deblock_ref as DR

LAYOUTS = ((0, 0), (1, 3), (3, 5))

QPS = (-12, 0, 17, 63, 22, 27, 30, 32, 34, 37, 40, 42, 45, 47, 51, 56)
STEPS = (0, 0, 1, 1, 2, 3, 4, 6, 9, 14, 22, 40, 90)


class Block:
    __slots__ = ("x", "y", "w", "h", "affine", "qp", "kind", "seed")


class Case:
    def __init__(self, name, width, height, ctu, bit_depth, planes, lfp_ver, lfp_hor, clip, beta_offsets, tc_offsets, blocks):
        self.name, self.width, self.height, self.ctu, self.bit_depth, self.planes = name, width, height, ctu, bit_depth, planes
        self.lfp_ver, self.lfp_hor, self.clip, self.beta_offsets, self.tc_offsets, self.blocks = lfp_ver, lfp_hor, clip, beta_offsets, tc_offsets, blocks
        self.ctu_rows = -(-height // ctu)


def _split(rng, x, y, w, h, W, H, out):
    if x >= W or y >= H:
        return
    cross_x, cross_y = x + w > W, y + h > H
    if cross_x or cross_y:
        how = "quad" if cross_x and cross_y else "ver" if cross_x else "hor"
    else:
        big = max(w, h)
        stop = 0.05 if big >= 128 else 0.30 if big >= 64 else 0.55 if big >= 32 else 0.40 if big >= 16 else 0.55
        r = rng.random()
        how = "stop" if r < stop or (w == 4 and h == 4) else ("quad", "ver", "hor")[int(rng.integers(0, 3))]
        if (how in ("quad", "ver") and w == 4) or (how in ("quad", "hor") and h == 4):
            how = "stop"
    if how == "stop":
        b = Block()
        b.x, b.y, b.w, b.h = x, y, w, h
        large = max(w, h) >= 32
        b.affine = bool(min(w, h) >= 8 and max(w, h) >= 16 and rng.random() < (0.45 if large else 0.3))
        b.qp = [int(QPS[int(rng.integers(0, len(QPS)))]) if rng.random() < (0.2 if large else 0.5) else int(rng.integers(30, 48)) for _ in range(3)]
        kinds = ("flat", "flat", "flat", "flat", "flat", "flat", "tiny", "tiny", "ramp", "lnoise") if large else ("flat", "flat", "flat", "flat", "ramp", "ramp", "lnoise", "lnoise", "noise", "tiny")
        b.kind = kinds[int(rng.integers(0, 10))]
        b.seed = int(rng.integers(0, 1 << 30))
        out.append(b)
    elif how == "quad":
        for (dx, dy) in ((0, 0), (w // 2, 0), (0, h // 2), (w // 2, h // 2)):
            _split(rng, x + dx, y + dy, w // 2, h // 2, W, H, out)
    elif how == "ver":
        _split(rng, x, y, w // 2, h, W, H, out)
        _split(rng, x + w // 2, y, w // 2, h, W, H, out)
    else:
        _split(rng, x, y, w, h // 2, W, H, out)
        _split(rng, x, y + h // 2, w, h // 2, W, H, out)


def partition(rng, width, height, ctu):
    blocks = []
    for y in range(0, height, ctu):
        for x in range(0, width, ctu):
            _split(rng, x, y, ctu, ctu, width, height, blocks)
    return blocks


def _pq_len(size_p, size_q, p_affine):
    if size_p <= 4 or size_q <= 4:
        return 0x11 | 128
    return ((((5 if p_affine else 7) if size_p >= 32 else 3) << 4) | (7 if size_q >= 32 else 3)) | 128


def _draw_bs(rng):
    v = 0
    for c in range(3):
        v |= int(rng.choice((0, 1, 1, 2, 2, 2) if c == 0 else (0, 1, 1, 2, 2))) << (2 * c)
    return v


def build_maps(rng, width, height, blocks):
    """-> ( lfp_ver, lfp_hor ): LF_PARAM_DTYPE [ height / 4 ][ width / 4 ]"""
    uw, uh = width // 4, height // 4
    owner = np.zeros((uh, uw), np.int32)
    for i, b in enumerate(blocks):
        owner[b.y // 4:(b.y + b.h) // 4, b.x // 4:(b.x + b.w) // 4] = i
    maps = []
    for ver in (True, False):
        m = np.zeros((uh, uw), DR.LF_PARAM_DTYPE)
        for b in blocks:
            perp_pos, perp_size, parl_size = (b.x, b.w, b.h) if ver else (b.y, b.h, b.w)
            for j in range(parl_size // 4):
                ux, uy = (b.x // 4, b.y // 4 + j) if ver else (b.x // 4 + j, b.y // 4)
                if perp_pos > 0:      # the block's own border: a transform edge
                    p = blocks[owner[uy, ux - 1] if ver else owner[uy - 1, ux]]
                    size_p = p.w if ver else p.h
                    ln = _pq_len(size_p, perp_size, p.affine)
                    if b.affine:
                        ln = (ln & 0xf0) | min(ln & 7, 5)
                    r = m[uy, ux]
                    r["side_max_filt_length"], r["bs"] = ln, _draw_bs(rng)
                    r["qp"] = [(p.qp[c] + b.qp[c] + 1) >> 1 for c in range(3)]
                    r["flags"] = 3 | (DR.FLAG_CMFL if size_p >= 16 and perp_size >= 16 else 0)
                if b.affine:      # sub-block edges inside the block
                    for d in range(8, perp_size, 8):
                        ln = 2 if d == 8 or d + 8 >= perp_size else 3
                        r = m[uy, ux + d // 4] if ver else m[uy + d // 4, ux]
                        r["side_max_filt_length"], r["bs"], r["qp"], r["flags"] = (ln << 4) | ln, _draw_bs(rng) & 0x3d, b.qp, 3
        maps.append(m)
    return maps


def _fill(rng, blocks, width, height, bd, shift, plane_idx):
    """the samples of one plane (shift 1: a 4:2:0 chroma plane)"""
    mx = (1 << bd) - 1
    W, H = width >> shift, height >> shift
    out = np.zeros((H, W), np.int64)
    region = {}
    scale = 1 << (bd - 8)
    for b in blocks:
        key = b.x * 3 // width      # three bands side by side: one at 0, one at the maximum, one in the middle of the range
        if key not in region:
            if not region:
                order = rng.permutation(3)
            region[key] = (0, mx, int(rng.integers(mx // 4, 3 * mx // 4)))[int(order[key])]
        g = np.random.default_rng(b.seed + 977 * plane_idx)
        x, y, w, h = b.x >> shift, b.y >> shift, b.w >> shift, b.h >> shift
        if w == 0 or h == 0:
            continue
        level = region[key] + int(g.choice((-1, 1))) * int(g.choice(STEPS)) * int(g.choice((1, scale)))
        yy, xx = np.mgrid[0:h, 0:w]
        if b.kind == "flat":
            v = np.full((h, w), level)
        elif b.kind == "tiny":
            v = level + g.integers(0, 2, (h, w))
        elif b.kind == "ramp":
            v = level + (xx if g.random() < 0.5 else yy) * int(g.integers(1, 4)) * int(g.choice((-1, 1)))
        elif b.kind == "lnoise":
            a = int(g.integers(1, 4)) * int(g.choice((1, scale)))
            v = level + g.integers(-a, a + 1, (h, w))
        else:
            v = g.integers(0, mx + 1, (h, w))
        out[y:y + h, x:x + w] = v
    return np.clip(out, 0, mx).astype(np.int16)


def make_case(name, seed, width, height, ctu, bit_depth, chroma=True, narrow=False, beta_offsets=(0, 0, 0), tc_offsets=(0, 0, 0)):
    rng = np.random.default_rng(seed)
    blocks = partition(rng, width, height, ctu)
    lfp_ver, lfp_hor = build_maps(rng, width, height, blocks)
    planes = [_fill(rng, blocks, width, height, bit_depth, int(c > 0), c) for c in range(3 if chroma else 1)]
    lo, hi = 0, (1 << (bit_depth - 1 if narrow else bit_depth)) - 1      # narrowed: the range of one bit less — all a ClpRng of the reference can express
    return Case(name, width, height, ctu, bit_depth, planes, lfp_ver, lfp_hor, [(lo, hi)] * len(planes), beta_offsets, tc_offsets, blocks)


SPECS = (      # name, seed, luma width, height, CTU, bit depth, 4:2:0, narrowed clip range, beta offsets / 2, tc offsets / 2
    ("g72", 4116, 72, 40, 32, 10, True, False, (0, 0, 0), (0, 0, 0)),
    ("g136", 4102, 136, 72, 64, 8, True, False, (2, -1, 1), (1, 0, -2)),
    ("g264", 4103, 264, 136, 128, 12, True, False, (0, 0, 0), (0, 0, 0)),
    ("mono", 4104, 72, 40, 32, 8, False, False, (1, 0, 0), (-1, 0, 0)),
    ("narrow", 4105, 136, 72, 64, 10, True, True, (0, 0, 0), (0, 0, 0)),
    ("g64", 4115, 64, 64, 32, 10, True, False, (0, 0, 0), (0, 0, 0)),      # 2 x 2 whole CTUs: blocks of >= 16 samples on both sides of a horizontal CTU boundary (chroma)
)

_cases = None


def cases():
    """name -> Case"""
    global _cases
    if _cases is None:
        _cases = {s[0]: make_case(*s) for s in SPECS}
    return _cases
