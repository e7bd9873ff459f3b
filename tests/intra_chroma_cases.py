"""The case list of the intra chroma mode pre-selection fixture (tests/golden/intra_chroma.npz) and helpers shared by its driver and tests.

A case is one 4:2:0 chroma block: its shape, bit depth, flags and template counts, the eight candidate modes, a WINDOW of reconstructed luma around its collocated area (the
area's top-left sample sits at ( ORG, ORG ) of the window; the window reaches four samples above and to the left and over twice the area's width and height, so every sample
loadLMLumaRecPels can read for any flag combination lies inside), the unfiltered Cb and Cr reference lines and the two compact originals.
  sweep     every ( w, h ) of { 4, 8, 16, 32 }^2, both sides available with the longest templates (the :1487 clamp bites where w > h, the :1493 clamp where h > w), the candidate
            list of CU::getIntraChromaCandModes with DM cycling through 66, 2, 34, odd modes and the four defaults (whose slot then carries 66)
  angles    eight regular modes per case on the shapes where each angular branch exists (any slot may carry any mode 0..66)
  avail     above only, left only and nothing available, with verCollocatedChroma on and off and on the first row of a CTU (left and above padding, the MDLM defaults)
  depth     8 and 12 bits
  patterns  two-level and full-range planes, flat planes ( diff == 0 ), a flat chroma template ( diffC == 0 ), a steep model ( iShift < 1, both signs ), a model whose output
            leaves the clip range at both ends
The fixture records only what both rows of the reference agree on.  They do not agree on the two-tap interpolation of IntraPredAngleChroma at 12 bits: the x86 row forms
( 32 - f ) * p0 + f * p1 + 16 in 16-bit lanes, which wraps for samples of 2048 and more, while the scalar row (and the standard, and the device) use 32 bits.  So the 12-bit
cases carry no fractional-slope candidate ( dm_of ); at 12 bits that path is checked against the model alone (tests/test_gpu_intra_chroma.py's random list), and the model's
two-tap path is anchored by every 8- and 10-bit case here."""
import numpy as np

import intra_chroma_ref as CR

ORG = 4          # the window's origin: the area's top-left sample
SHAPES = [(w, h) for w in CR.SIZES for h in CR.SIZES]
DEFAULT_CAND = (0, 50, 18, 1, CR.LM, CR.MDLM_L, CR.MDLM_T)
DM_CYCLE = (66, 2, 34, 3, 0, 50, 61, 18, 1, 35, 45, 7, 23, 55, 29, 41)
ANGLE_SETS = {(4, 4): ((2, 10, 18, 26, 34, 42, 58, 66), (3, 19, 33, 49, 50, 51, 60, 65)), (8, 8): ((2, 5, 17, 27, 34, 43, 59, 66), (4, 20, 32, 48, 52, 56, 62, 64)),
              (16, 4): ((2, 4, 7, 9, 11, 30, 58, 66), (3, 8, 18, 36, 50, 54, 63, 65)), (4, 16): ((2, 8, 14, 38, 57, 59, 62, 66), (3, 5, 18, 22, 50, 58, 61, 65)),
              (32, 4): ((2, 6, 10, 13, 15, 16, 50, 66), (5, 12, 14, 18, 44, 60, 64, 65)), (4, 32): ((2, 18, 34, 52, 53, 56, 62, 66), (3, 6, 50, 54, 55, 60, 63, 65)),
              (16, 16): ((2, 3, 18, 31, 35, 50, 55, 66),), (32, 32): ((2, 18, 34, 47, 50, 53, 57, 66),), (32, 8): ((2, 9, 12, 40, 58, 66, 0, 1),), (8, 32): ((2, 10, 56, 59, 66, 34, 0, 1),)}
AVAIL_SHAPES = [(4, 4), (8, 8), (16, 4), (4, 16)]
BIG_PRED_SLOTS = (0, 4, 5, 6, 7)          # the slots whose predictions the fixture stores for blocks above 256 samples


def window_shape(w, h):
    return (4 * h + ORG + 2, 4 * w + ORG + 2)


class Case(object):
    def __init__(self, name, w, h, bit_depth, flags, n_ar, n_lb, cand, luma, lines, org, mode_mask=0xff, pred_mask=None):
        self.name, self.w, self.h, self.bit_depth, self.flags, self.n_ar, self.n_lb = name, w, h, bit_depth, flags, n_ar, n_lb
        self.cand, self.mode_mask = tuple(int(m) for m in cand), mode_mask
        self.pred_mask = mode_mask if pred_mask is None else pred_mask
        self.luma, self.lines, self.org = np.ascontiguousarray(luma, np.int16), np.ascontiguousarray(lines, np.int16), np.ascontiguousarray(org, np.int16)
        assert len(self.cand) == 8 and self.luma.shape == window_shape(w, h) and self.lines.shape == (2, CR.line_len(w, h)) and self.org.shape == (2, h, w)
        assert not self.pred_mask & ~self.mode_mask and n_ar % 2 == 0 and n_lb % 2 == 0 and (flags & CR.F_ABOVE or not n_ar) and (flags & CR.F_LEFT or not n_lb)


def cand_list(dm):
    """CU::getIntraChromaCandModes for a luma mode that DM resolves to `dm`"""
    c = list(DEFAULT_CAND) + [dm]
    for i in range(4):
        if c[i] == dm:
            c[i] = 66
            break
    return tuple(c)


def fields(rng, w, h, bit_depth, kind):
    """-> ( luma window, lines [2], originals [2] ) of one pattern"""
    vmax = (1 << bit_depth) - 1
    wh, ww = window_shape(w, h)
    yy, xx = np.mgrid[0:wh, 0:ww]
    lx, ly = (xx - ORG) / 2.0, (yy - ORG) / 2.0          # chroma coordinates of a luma sample
    n = CR.line_len(w, h)
    cx = np.concatenate([np.arange(2 * w + 1) - 1.0, np.full(2 * h + 1, -1.0)])          # chroma coordinates along the lines
    cy = np.concatenate([np.full(2 * w + 1, -1.0), np.arange(2 * h + 1) - 1.0])
    by, bx = np.mgrid[0:h, 0:w]

    def rnd(a):
        return np.clip(np.rint(a), 0, vmax).astype(np.int16)

    if kind in ("smooth", "steep_pos", "steep_neg", "overshoot"):
        gx, gy = rng.uniform(-0.03, 0.03, 2) * vmax
        amp, ph, fr = rng.uniform(0.05, 0.15) * vmax, rng.uniform(0, 6.28), rng.uniform(0.15, 0.5)
        if kind in ("steep_pos", "steep_neg"):
            gx, gy, amp = 0.0, 0.0, 1.2          # a luma template that differs by about one level, a chroma template that differs by hundreds
        noise = rng.uniform(0.004, 0.02) * vmax if kind == "smooth" else 0.3

        def f(x, y):
            return 0.5 * vmax + gx * x + gy * y + amp * np.sin(fr * (x + 0.6 * y) + ph)

        slope = {"smooth": (rng.uniform(0.3, 1.2), -rng.uniform(0.2, 0.9)), "steep_pos": (0.2 * vmax, 0.15 * vmax), "steep_neg": (-0.2 * vmax, -0.15 * vmax), "overshoot": (3.5, -3.5)}[kind]
        luma = rnd(f(lx, ly) + rng.normal(0, noise, lx.shape))
        lines = [rnd(0.5 * vmax + s * (f(cx, cy) - 0.5 * vmax) + rng.normal(0, noise, n)) for s in slope]
        org = [rnd(0.5 * vmax + s * (f(bx, by) - 0.5 * vmax) + rng.normal(0, max(noise, 2.0), (h, w))) for s in slope]
        if kind == "overshoot":          # the block's luma runs far beyond the template's range: a * luma + b leaves [0, vmax] at both ends
            luma = luma.astype(np.int64)
            luma[ORG:, ORG:] = rnd(0.5 * vmax + 0.45 * vmax * np.sin(0.9 * lx[ORG:, ORG:] + 0.7 * ly[ORG:, ORG:]))
            luma = luma.astype(np.int16)
    elif kind == "two_level":
        lo, hi = sorted(int(v) for v in rng.integers(0, vmax + 1, 2))
        luma = np.where(rng.integers(0, 2, lx.shape) > 0, hi, lo).astype(np.int16)
        lines = [np.where(rng.integers(0, 2, n) > 0, vmax - lo, hi // 2).astype(np.int16) for _ in (0, 1)]
        org = [np.where(rng.integers(0, 2, (h, w)) > 0, hi, lo).astype(np.int16) for _ in (0, 1)]
    elif kind == "full":
        luma = rng.integers(0, vmax + 1, lx.shape).astype(np.int16)
        lines = [rng.integers(0, vmax + 1, n).astype(np.int16) for _ in (0, 1)]
        org = [rng.integers(0, vmax + 1, (h, w)).astype(np.int16) for _ in (0, 1)]
    elif kind in ("zero", "max"):
        v = 0 if kind == "zero" else vmax
        luma = np.full(lx.shape, v, np.int16)
        lines = [rng.integers(0, vmax + 1, n).astype(np.int16) for _ in (0, 1)]
        org = [rng.integers(0, vmax + 1, (h, w)).astype(np.int16) for _ in (0, 1)]
    elif kind == "flat_chroma":
        luma = rng.integers(0, vmax + 1, lx.shape).astype(np.int16)
        lines = [np.full(n, v, np.int16) for v in (vmax // 3, vmax)]
        org = [rng.integers(0, vmax + 1, (h, w)).astype(np.int16) for _ in (0, 1)]
    else:
        raise ValueError(kind)
    for l in lines:
        l[2 * w + 1] = l[0]          # the corner is one sample, seen from both rows
    return luma, np.stack(lines), np.stack(org)


def full_counts(w, h, flags):
    """the longest templates a block can have: every above-right / left-below unit available"""
    return (w if flags & CR.F_ABOVE else 0), (h if flags & CR.F_LEFT else 0)


def dm_of(bit_depth, w, h, k):
    """the mode DM resolves to in a case: DM_CYCLE, except at 12 bits, where only modes without the two-tap interpolation are used (see the module's last paragraph)"""
    if bit_depth <= 10:
        return DM_CYCLE[k % 16]
    return (66, 2, 34)[k % 3] if w == h else 34


def pred_mask_of(w, h, mode_mask):
    return mode_mask if w * h <= 256 else mode_mask & sum(1 << s for s in BIG_PRED_SLOTS)


def cases():
    """-> { name: Case } in a fixed order"""
    out = {}
    both = CR.F_ABOVE | CR.F_LEFT

    def add(name, w, h, bd, flags, counts, cand, kind, seed):
        n_ar, n_lb = full_counts(w, h, flags) if counts is None else counts
        out[name] = Case(name, w, h, bd, flags, n_ar, n_lb, cand, *fields(np.random.default_rng(seed), w, h, bd, kind), pred_mask=pred_mask_of(w, h, 0xff))

    for k, (w, h) in enumerate(SHAPES):
        add("s%dx%d" % (w, h), w, h, 10, both | (CR.F_VER_COLLOCATED if k % 3 == 1 else 0), None, cand_list(DM_CYCLE[k]), "smooth", 1000 + k)
    for (w, h), sets in ANGLE_SETS.items():
        for j, cand in enumerate(sets):
            add("a%d_%dx%d" % (j, w, h), w, h, 10, both, (0, 0), cand, "smooth", 2000 + 100 * j + 4 * w + h)
    k = 0
    for (w, h) in AVAIL_SHAPES:
        for av, fl in (("above", CR.F_ABOVE), ("left", CR.F_LEFT), ("none", 0)):
            for vc in (0, CR.F_VER_COLLOCATED):
                add("v%s%d_%dx%d" % (av, int(vc > 0), w, h), w, h, 10, fl | vc, None, cand_list(DM_CYCLE[k % 16]), "smooth", 3000 + k)
                k += 1
    for k, (w, h, fl, counts) in enumerate([(8, 8, both, None), (16, 4, CR.F_ABOVE, None), (4, 4, both, (2, 2)), (8, 16, both | CR.F_VER_COLLOCATED, (4, 6)), (16, 8, both, (8, 0)), (32, 4, both, (2, 4))]):
        add("r%d_%dx%d" % (k, w, h), w, h, 10, fl | CR.F_FIRST_ROW, counts, cand_list(DM_CYCLE[(k + 5) % 16]), "smooth", 4000 + k)
    for k, (w, h) in enumerate([(4, 4), (8, 8), (8, 16)]):
        for bd in (8, 12):
            add("b%d_%dx%d" % (bd, w, h), w, h, bd, both | (CR.F_VER_COLLOCATED if bd == 12 else 0), None, cand_list(dm_of(bd, w, h, k + 9)), "smooth", 5000 + 10 * k + bd)
    k = 0
    for kind in ("two_level", "full", "zero", "max", "flat_chroma", "steep_pos", "steep_neg", "overshoot"):
        for (w, h, bd, fl) in [(4, 4, 8, both), (8, 4, 10, both | CR.F_VER_COLLOCATED), (16, 16, 12, both), (4, 8, 12, CR.F_LEFT | CR.F_VER_COLLOCATED)]:
            add("p%s_%dx%d" % (kind, w, h), w, h, bd, fl, None, cand_list(dm_of(bd, w, h, k)), kind, 6000 + k)
            k += 1
    return out


def as_list(case_list, pred="stored", mode_mask=None):
    """a list of cases as ONE entry call -> ( items ITEM_DTYPE, luma int16, ref int16, org int16, pred samples ).  pred: "stored" (the case's pred_mask), "all" or "none";
    every case's luma window becomes a stretch of the one luma array, its own width the pitch"""
    items = np.zeros(len(case_list), CR.ITEM_DTYPE)
    lumas, refs, orgs, lo, ro, oo, po = [], [], [], 0, 0, 0, 0
    for i, c in enumerate(case_list):
        mm = c.mode_mask if mode_mask is None else mode_mask
        pm = {"stored": c.pred_mask & mm, "all": mm, "none": 0}[pred]
        n, npred = c.w * c.h, bin(pm).count("1")
        it = items[i]
        it["w"], it["h"], it["bit_depth"], it["flags"], it["n_above_right"], it["n_left_below"], it["mode_mask"], it["pred_mask"] = c.w, c.h, c.bit_depth, c.flags, c.n_ar, c.n_lb, mm, pm
        it["cand"] = c.cand
        it["luma_stride"], it["luma_off"] = c.luma.shape[1], lo + ORG * c.luma.shape[1] + ORG
        it["ref_off"], it["org_off"], it["pred_off"], it["cost_off"] = (ro, ro + c.lines.shape[1]), (oo, oo + n), (po, po + npred * n), i * CR.NUM_SLOTS
        lumas.append(c.luma.reshape(-1))
        refs.append(c.lines.reshape(-1))
        orgs.append(c.org.reshape(-1))
        lo, ro, oo, po = lo + c.luma.size, ro + c.lines.size, oo + 2 * n, po + 2 * npred * n
    return items, np.concatenate(lumas), np.concatenate(refs), np.concatenate(orgs), po


def expected(case, cnt=None, touched=None):
    """the model on a case -> ( costs uint32 [8]; ( a, b, shift ) int32 [8][2][3], 0 for regular slots; predictions int16 [ stored slots ][2][h][w] )"""
    items, luma, ref, org, _ = as_list([case])
    costs, prm, preds = CR.run_item(items[0], luma, ref, org, cnt, touched)
    if cnt is not None and case.mode_mask & 0x80:
        dm = case.cand[7]
        CR.bump(cnt, {66: "dm_66", 2: "dm_2", 34: "dm_34"}.get(dm, "dm_odd" if dm & 1 else "dm_other"))
    p = np.zeros((CR.NUM_SLOTS, 2, 3), np.int32)
    for s, v in prm.items():
        p[s] = v
    want = CR.mask_bits(case.pred_mask)
    return costs, p, (np.stack([preds[s] for s in want]) if want else np.zeros((0, 2, case.h, case.w), np.int16))


# what the fixture must exercise (counter names of tests/intra_chroma_ref.py and of expected above)
REQUIRED = ("avail_both", "avail_above", "avail_left", "avail_none", "first_row", "ver_collocated_on", "ver_collocated_off", "left_padding", "above_padding",
            "clamp_above_right_bites", "clamp_above_right_free", "clamp_left_below_bites", "clamp_left_below_free", "diff_zero", "diffc_zero", "a_negative",
            "shift_clamp_positive", "shift_clamp_negative", "lm_clip_low", "lm_clip_high", "mdlm_t_default", "mdlm_l_default", "lm_nothing_available",
            "wide_below", "wide_above", "neg_ver", "neg_hor", "integer_slope", "two_tap", "hv_pdpc", "ang_pdpc_scale0", "ang_pdpc_scale1", "ang_pdpc_scale2",
            "ang_pdpc_off_negative_scale", "dc", "dc_nonsquare", "planar", "dm_66", "dm_2", "dm_34", "dm_odd")


def load_golden():
    """-> { name: ( Case, costs, params, predictions ) } from tests/golden/intra_chroma.npz"""
    z = np.load(CR.GOLDEN)
    out = {}
    for name in z["cases"]:
        name = str(name)
        w, h, bd, flags, n_ar, n_lb, mm, pm = (int(v) for v in z[name + "_hdr"])
        c = Case(name, w, h, bd, flags, n_ar, n_lb, z[name + "_cand"], z[name + "_luma"], z[name + "_lines"], z[name + "_org"], mm, pm)
        out[name] = (c, z[name + "_cost"], z[name + "_prm"], z[name + "_pred"])
    return out
