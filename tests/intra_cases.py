"""The case list of the intra luma mode pre-selection fixture (tests/golden/intra.npz) and helpers shared by its driver and tests.

A case is one block: its shape, bit depth, multi_ref_idx, the unfiltered reference lines (tests/intra_ref.py: `lines`), the compact original, the modes that are scored and the
modes whose predictions the fixture stores.  The shapes are the smallest at which each branch exists:
  4x4, 8x4, 4x8                      at most 32 samples: no reference filter, always the cubic filter
  8x8, 16x16, 32x32                  one per row of m_aucIntraFilter that differs
  16x4, 4x16, 32x4, 4x32, 64x4, 4x64 wide angles in both directions with deltaSize 2, 3, 4
  32x8, 8x32                         rectangular Hadamard tiles (16x8, 8x16)
  64x64                              once
Every mode 0..66 at multi_ref_idx 0; modes 1..66 at multi_ref_idx 1 and 2 on MRL_SHAPES (a wide-angle one among them); 8 and 12 bits on 4x4, 8x8, 16x4; the limit patterns
(all 0, all max, alternating 0 / max — the cubic filter overshoots both clip bounds —, a step at the corner) on small shapes."""
import numpy as np

import intra_ref as IR

SHAPES = [(4, 4), (8, 4), (4, 8), (8, 8), (16, 16), (32, 32), (16, 4), (4, 16), (32, 4), (4, 32), (64, 4), (4, 64), (32, 8), (8, 32), (64, 64)]
MRL_SHAPES = [(4, 4), (8, 8), (16, 4), (4, 16), (16, 16)]
DEPTH_SHAPES = [(4, 4), (8, 8), (16, 4)]
LIMIT_SHAPES = [(4, 4, 8), (8, 8, 10), (16, 4, 12), (4, 16, 10), (16, 16, 10)]
PATTERNS = ("zero", "max", "alt", "step")
FULL_PRED_SAMPLES = 256
# the modes whose predictions are stored for larger blocks: planar, DC, pure H / V, the diagonals (integer slope), both negative orientations, fractional slopes on either side
# of the filter thresholds, the ends of the range
BIG_PRED_MODES = (0, 1, 2, 3, 10, 18, 19, 26, 34, 42, 49, 50, 51, 58, 65, 66)
ALL_MODES = tuple(range(IR.NUM_MODES))


class Case(object):
    def __init__(self, name, w, h, bit_depth, mri, lines, org, modes, pred_modes):
        self.name, self.w, self.h, self.bit_depth, self.mri = name, w, h, bit_depth, mri
        self.lines, self.org = np.ascontiguousarray(lines, np.int16), np.ascontiguousarray(org, np.int16)
        self.modes, self.pred_modes = tuple(modes), tuple(pred_modes)
        assert self.lines.size == IR.line_len(w, h, mri) and self.org.shape == (h, w) and set(self.pred_modes) <= set(self.modes)


def seeded(rng, w, h, bit_depth, mri):
    """smooth plus noise: a tilted plane with a ripple under the block and its lines, the same field sampled along the top row and the left column"""
    vmax = (1 << bit_depth) - 1
    gx, gy = rng.uniform(-0.02, 0.02, 2) * vmax
    amp, ph, fr = rng.uniform(0.03, 0.12) * vmax, rng.uniform(0, 6.28), rng.uniform(0.15, 0.6)
    noise = rng.uniform(0.004, 0.03) * vmax

    def field(x, y):
        return 0.5 * vmax + gx * x + gy * y + amp * np.sin(fr * (x + 0.6 * y) + ph)

    nt, nl = 2 * w + 1 + mri, 2 * h + 1 + mri
    top = field(np.arange(nt) - 1.0 - mri, -1.0 - mri)
    left = field(-1.0 - mri, np.arange(nl) - 1.0 - mri)
    lines = np.concatenate([top, left])
    lines = np.clip(np.rint(lines + rng.normal(0, noise, lines.size)), 0, vmax)
    y, x = np.mgrid[0:h, 0:w]
    org = np.clip(np.rint(field(x, y) + rng.normal(0, noise, (h, w))), 0, vmax)
    return lines.astype(np.int16), org.astype(np.int16)


def limit(pattern, rng, w, h, bit_depth, mri):
    vmax = (1 << bit_depth) - 1
    nt, nl = 2 * w + 1 + mri, 2 * h + 1 + mri
    org = rng.integers(0, vmax + 1, (h, w))
    if pattern == "zero":
        lines = np.zeros(nt + nl, np.int64)
    elif pattern == "max":
        lines = np.full(nt + nl, vmax, np.int64)
    elif pattern == "alt":
        lines = np.concatenate([(np.arange(nt) & 1) * vmax, (np.arange(nl) & 1) * vmax])
        org = ((np.add.outer(np.arange(h), np.arange(w)) & 1) ^ 1) * vmax
    else:          # a step at the corner: the top row at the maximum, the left column at zero
        lines = np.concatenate([np.full(nt, vmax), np.zeros(nl, np.int64)])
        lines[nt] = vmax          # the corner is one sample, seen from both rows
    return lines.astype(np.int16), org.astype(np.int16)


def pred_modes_of(w, h, modes):
    return tuple(modes) if w * h <= FULL_PRED_SAMPLES else tuple(m for m in BIG_PRED_MODES if m in modes)


def cases():
    """-> { name: Case } in a fixed order"""
    out = {}

    def add(name, w, h, bd, mri, lines, org):
        modes = ALL_MODES if mri == 0 else ALL_MODES[1:]
        out[name] = Case(name, w, h, bd, mri, lines, org, modes, pred_modes_of(w, h, modes))

    for k, (w, h) in enumerate(SHAPES):
        add("s%dx%d" % (w, h), w, h, 10, 0, *seeded(np.random.default_rng(1000 + k), w, h, 10, 0))
    for k, (w, h) in enumerate(MRL_SHAPES):
        for mri in (1, 2):
            add("m%d_%dx%d" % (mri, w, h), w, h, 10, mri, *seeded(np.random.default_rng(2000 + 10 * k + mri), w, h, 10, mri))
    for k, (w, h) in enumerate(DEPTH_SHAPES):
        for bd in (8, 12):
            add("b%d_%dx%d" % (bd, w, h), w, h, bd, 0, *seeded(np.random.default_rng(3000 + 10 * k + bd), w, h, bd, 0))
    for k, (w, h, bd) in enumerate(LIMIT_SHAPES):
        for j, pat in enumerate(PATTERNS):
            mri = 1 if (pat == "alt" and (w, h) == (16, 16)) else 0
            add("l%s_%dx%d" % (pat, w, h), w, h, bd, mri, *limit(pat, np.random.default_rng(4000 + 10 * k + j), w, h, bd, mri))
    return out


def expected(case, cnt=None):
    """the model on a case -> ( costs uint32 [67], 0 where not scored; predictions int16 [ len( pred_modes ) ][ h ][ w ] )"""
    costs, preds = np.zeros(IR.NUM_MODES, np.uint32), []
    for m in case.modes:
        p = IR.predict(case.lines, case.w, case.h, m, case.mri, case.bit_depth, cnt)
        costs[m] = IR.cost(case.org, p, cnt)
        if m in case.pred_modes:
            preds.append(p)
    return costs, np.stack(preds) if preds else np.zeros((0, case.h, case.w), np.int16)


# what the fixture must exercise (counter names of tests/intra_ref.py)
REQUIRED = ("ref_filter", "smoothing", "cubic", "integer_slope", "hv_pdpc", "hv_copy", "ang_pdpc_scale0", "ang_pdpc_scale1", "ang_pdpc_scale2", "ang_pdpc_off_negative_scale",
            "neg_ver", "neg_hor", "wide_below", "wide_above", "clip_low", "clip_high", "cost_had", "cost_2sad", "planar", "dc", "dc_pdpc", "transposed")


def load_golden():
    """-> { name: ( Case, costs, predictions ) } from tests/golden/intra.npz"""
    z = np.load(IR.GOLDEN)
    out = {}
    for name in z["cases"]:
        name = str(name)
        w, h, bd, mri = (int(v) for v in z[name + "_hdr"])
        c = Case(name, w, h, bd, mri, z[name + "_lines"], z[name + "_org"], IR.mask_bits(z[name + "_modes"]), IR.mask_bits(z[name + "_pmodes"]))
        out[name] = (c, z[name + "_cost"], z[name + "_pred"])
    return out


def as_list(case_list, pred="stored"):
    """a list of cases as ONE entry call -> ( items ITEM_DTYPE, ref int16, org int16, pred samples ).  pred: "stored" (the case's pred_modes), "all" or "none" """
    items = np.zeros(len(case_list), IR.ITEM_DTYPE)
    refs, orgs, ro, oo, po = [], [], 0, 0, 0
    for i, c in enumerate(case_list):
        pm = {"stored": c.pred_modes, "all": c.modes, "none": ()}[pred]
        items[i] = (c.w, c.h, c.bit_depth, c.mri, ro, oo, po, i * IR.NUM_MODES, IR.make_mask(c.modes), IR.make_mask(pm), 0)
        refs.append(c.lines)
        orgs.append(c.org.reshape(-1))
        ro, oo, po = ro + c.lines.size, oo + c.w * c.h, po + len(pm) * c.w * c.h
    return items, np.concatenate(refs), np.concatenate(orgs), po
