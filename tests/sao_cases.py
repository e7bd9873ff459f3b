"""Seeded case lists of the SAO entries, shared by the fixture generator (tests/sao_golden_gen.py), the CPU tier (tests/test_sao_cpu.py) and the GPU tier
(tests/test_gpu_sao.py, tests/test_gpu_sao_shim.py).  Everything is 4:2:0: plane 0 is luma with CTU size `ctu`, planes 1 and 2 have half the size and half the CTU size.

pictures()       name -> Pic: the original and the deblocked ("src") planes.  The smallest geometries at which the kernels can still go wrong: a last CTU column / row
                 narrower than the vector width, one CTU larger than the picture, an 8-wide picture, CTU 128 for the many-rows-per-lane walk, a 3 x 3 grid whose centre CTU
                 has every neighbour; and contents that drive single classes: flat, ramps, checkerboard, rows of ties, the two sample extremes over a whole 128 x 128 CTU.
stats_cases()    ( name, picture, flags ): borders alone on every picture; on the 3 x 3 grid the centre CTU without any flag, and every single flag of it cleared from the full set and set alone
                 — among them the two combinations borders cannot produce, above-left without above and above-right without right.
offset_cases()   ( name, picture, params [ctus][3], clip [3] ): every type, offsets at +- getMaxOffsetQVal, bands 0 / 28 / 29 / 31 (wrapping), an off CTU between filtered
                 ones, a plane off with the others on, sources at both ends of the sample range so that both clip ends act, a narrowed clip range, and on the 3 x 3 grid
                 every single availability bit of the centre CTU cleared from the full mask and set alone, for the four edge types.
LAYOUTS          ( base offset in samples, extra pitch ) the GPU tier hands the planes over with."""
import numpy as np

import sao_ref as SR

LAYOUTS = ((0, 0), (1, 3), (3, 5))      # pitch = width rounded up to 8, + extra: the last two are no multiple of 8 and start at an odd sample


class Pic:
    def __init__(self, name, width, height, ctu, bit_depth, org, src):
        self.name, self.width, self.height, self.ctu, self.bit_depth, self.org, self.src = name, width, height, ctu, bit_depth, org, src
        self.ctus = [(ctu, ctu), (ctu // 2, ctu // 2), (ctu // 2, ctu // 2)]
        self.grid = SR.grid(width, height, ctu, ctu)
        self.n_ctus = self.grid[0] * self.grid[1]


def _content(kind, rng, w, h, bd):
    """-> ( org, src ) int16 h x w"""
    mx = (1 << bd) - 1
    yy, xx = np.mgrid[0:h, 0:w]
    amp = max(2, mx >> 6)
    if kind == "seeded":      # a gradient over the whole sample range (every band), waves and noise (every edge class)
        base = mx * (0.55 * xx / max(w - 1, 1) + 0.45 * yy / max(h - 1, 1)) + 0.08 * mx * np.sin(xx / 3.1) * np.cos(yy / 2.3)
        src = base + rng.integers(-amp, amp + 1, (h, w))
        org = src + rng.integers(-amp, amp + 1, (h, w))
    elif kind == "flat":
        src = np.full((h, w), mx // 2)
        org = src + rng.integers(-amp, amp + 1, (h, w))
    elif kind in ("hramp", "vramp", "dramp"):
        t = {"hramp": xx, "vramp": yy, "dramp": xx + yy}[kind]
        src = (t * 3) % (mx + 1)
        org = src + rng.integers(-amp, amp + 1, (h, w))
    elif kind == "checker":
        src = np.where((xx + yy) & 1, mx - 5, 7)
        org = src + np.where((xx + yy) & 1, -3, 2)
    elif kind == "ties":      # every row one value: the horizontal type sees ties only
        src = np.repeat(rng.integers(0, mx + 1, (h, 1)), w, axis=1)
        org = src + rng.integers(-amp, amp + 1, (h, w))
    elif kind == "src0":
        src, org = np.zeros((h, w)), np.full((h, w), mx)
    elif kind == "srcmax":
        src, org = np.full((h, w), mx), np.zeros((h, w))
    elif kind == "ends":      # samples within 3 of either end of the range
        src = np.where(rng.integers(0, 2, (h, w)), mx - rng.integers(0, 4, (h, w)), rng.integers(0, 4, (h, w)))
        org = src + rng.integers(-3, 4, (h, w))
    else:
        raise ValueError(kind)
    return np.clip(org, 0, mx).astype(np.int16), np.clip(src, 0, mx).astype(np.int16)


PICTURES = (      # name, content, luma width, height, CTU, bit depth
    ("geo72", "seeded", 72, 40, 32, 10), ("geo136", "seeded", 136, 72, 64, 8), ("geo264", "seeded", 264, 136, 128, 10), ("geo16", "seeded", 16, 8, 32, 8),
    ("geo8", "seeded", 8, 24, 16, 10), ("grid3", "seeded", 48, 48, 16, 10),
    ("flat", "flat", 72, 40, 32, 10), ("hramp", "hramp", 72, 40, 32, 10), ("vramp", "vramp", 72, 40, 32, 8), ("dramp", "dramp", 72, 40, 32, 10),
    ("checker", "checker", 72, 40, 32, 8), ("ties", "ties", 72, 40, 32, 10), ("src0", "src0", 128, 128, 128, 10), ("srcmax", "srcmax", 128, 128, 128, 8),
    ("ends", "ends", 72, 40, 32, 10),
)

_pics = None


def pictures():
    global _pics
    if _pics is None:
        _pics = {}
        for k, (name, kind, w, h, ctu, bd) in enumerate(PICTURES):
            rng = np.random.default_rng(810 + k)
            planes = [_content(kind, rng, w >> (c > 0), h >> (c > 0), bd) for c in range(3)]
            _pics[name] = Pic(name, w, h, ctu, bd, [p[0] for p in planes], [p[1] for p in planes])
    return _pics


def stats_cases():
    """-> list of ( name, Pic, flags or None )"""
    P = pictures()
    out = [(name + "/borders", P[name], None) for name in P]
    g = P["grid3"]
    base = SR.border_flags(*g.grid)
    assert base[4] == 63
    none = base.copy()
    none[4] = 0
    out.append(("grid3/none", g, none))
    for f in SR.STAT_FLAGS:
        a, b = base.copy(), base.copy()
        a[4], b[4] = 63 & ~f, f
        out += [("grid3/clear%d" % f, g, a), ("grid3/only%d" % f, g, b)]
    both = base.copy()
    both[4] = 63 & ~(SR.RIGHT | SR.ABOVE_RIGHT)      # above-right is looked at only where right is missing: its clearing shows against "clear8"
    out.append(("grid3/clear40", g, both))
    return out


def _uniform(pic, typ, offs, band=0, avail=None):
    prm = np.zeros((pic.n_ctus, 3), SR.PARAM_DTYPE)
    prm["type"], prm["band"], prm["offs"] = typ, band, offs
    prm["avail"] = (SR.border_avail(*pic.grid) if avail is None else avail)[:, None]
    return prm


def _mixed(pic, rng, plane_off=None):
    """types cycle over CTUs and planes, off CTUs between filtered ones; random offsets up to +- getMaxOffsetQVal"""
    q = SR.max_offset_qval(pic.bit_depth)
    prm = np.zeros((pic.n_ctus, 3), SR.PARAM_DTYPE)
    prm["avail"] = SR.border_avail(*pic.grid)[:, None]
    for i in range(pic.n_ctus):
        for c in range(3):
            prm[i, c]["type"] = -1 if c == plane_off else (i + 2 * c + 1) % 6 - 1
            prm[i, c]["band"] = rng.integers(0, 32)
            prm[i, c]["offs"] = rng.integers(-q, q + 1, 5)
    return prm


def offset_cases():
    """-> list of ( name, Pic, params [ctus][3], clip [3] )"""
    P = pictures()
    rng = np.random.default_rng(605)
    out = []

    def add(name, pic, prm, clip_bd=None):
        hi = (1 << (pic.bit_depth if clip_bd is None else clip_bd)) - 1
        out.append((name, pic, prm, [(0, hi)] * 3))

    g72, q10 = P["geo72"], SR.max_offset_qval(10)
    for t in range(4):
        add("geo72/eo%d" % t, g72, _uniform(g72, t, (q10, q10 // 2 + 1, -1, -(q10 // 2 + 1), -q10)))
    add("geo72/eo0neg", g72, _uniform(g72, 0, (-q10, -3, 2, 3, q10)))
    for band in (0, 12, 28, 29, 31):
        add("geo72/bo%d" % band, g72, _uniform(g72, 4, (q10, -q10, q10 // 2, -1, 0), band))
    add("geo72/mixed", g72, _mixed(g72, rng))
    add("geo136/mixed", P["geo136"], _mixed(P["geo136"], rng, plane_off=1))
    add("geo264/mixed", P["geo264"], _mixed(P["geo264"], rng))
    add("geo16/mixed", P["geo16"], _mixed(P["geo16"], rng))
    add("geo16/eo135", P["geo16"], _uniform(P["geo16"], 2, (7, 3, 1, -3, -7)))
    add("geo8/mixed", P["geo8"], _mixed(P["geo8"], rng))
    add("checker/eo45", P["checker"], _uniform(P["checker"], 3, (7, 7, 0, -7, -7)))
    ends = P["ends"]
    add("ends/eo90", ends, _uniform(ends, 1, (-q10, -q10, q10, q10, q10)))
    add("ends/eo0", ends, _uniform(ends, 0, (q10, q10, -q10, -q10, -q10)))
    add("ends/bo31", ends, _uniform(ends, 4, (q10, -q10, 0, 0, 0), 31))
    add("geo72/narrow-eo45", g72, _uniform(g72, 3, (q10, 2, 0, -2, -q10)), clip_bd=9)
    add("geo72/narrow-mixed", g72, _mixed(g72, rng), clip_bd=9)
    g = P["grid3"]
    for t in range(4):
        for bit in SR.AVAIL_BITS:
            for name, m in (("clear", 255 & ~bit), ("only", bit)):
                prm = _uniform(g, -1, (0, 0, 0, 0, 0))
                prm[4]["type"], prm[4]["avail"], prm[4]["offs"] = t, m, (q10, 9, -4, -9, -q10)
                add("grid3/eo%d-%s%d" % (t, name, bit), g, prm)
    return out
