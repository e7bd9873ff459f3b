"""Inputs shared by the CPU and GPU tiers of the CIIP form of the prediction list: the lists of items with their CIIP records and reference lines.
Everything here is numpy; the GPU tier uploads the planes and the lines.  Planes: tests/blend_cases.py.  Expected values: tests/ciip_ref.py."""
import numpy as np

import blend_cases as BLC
import blend_ref as BL
import ciip_ref as CR
import pred_ref as PR

PRED_ITEM_DTYPE, PRED_EXT_DTYPE, PRED_BLEND_DTYPE, PRED_CIIP_DTYPE = BLC.PRED_ITEM_DTYPE, BLC.PRED_EXT_DTYPE, BLC.PRED_BLEND_DTYPE, CR.PRED_CIIP_DTYPE
TILED = [(64, 64), (64, 32), (32, 64)]          # luma items of more than one tile (tiles of 32 x 16 samples)
ALL_SIZES = [(w, h, 0) for (w, h) in CR.LUMA_SIZES] + [(w, h, 1) for (w, h) in CR.CHROMA_SIZES]


class Builder(BLC.Builder):
    """blend_cases.Builder with a CIIP record per item and the array of reference lines the records point into"""

    def __init__(self, pl, seed):
        super().__init__(pl, seed)
        self.ciip, self.lines, self.at = [], [], 0

    def add(self, w, h, chroma, alt, fr, rp, mode=0, param=0, flags=0, delta=None, xy=None, num_intra=None, line=None):
        """num_intra None: a record that is OFF; line None: the row above and the column left of a seeded position in picture 1 (luma) / 3 (chroma)"""
        super().add(w, h, chroma, alt, fr, rp, mode, param, flags, delta, xy)
        c = np.zeros((), PRED_CIIP_DTYPE)
        if num_intra is not None:
            if line is None:
                pic = self.pl[3 if chroma else 1]
                x, y = int(self.rng.integers(1, pic.shape[1] - w - 2)), int(self.rng.integers(1, pic.shape[0] - h - 3))
                line = CR.line_at(pic, x, y, w, h)
            assert line.size == CR.line_len(w, h)
            if len(self.ciip) % 3 == 1:          # every third line starts at an odd sample
                self.lines.append(np.full(1, -1, np.int16)); self.at += 1
            c["mode"], c["num_intra"], c["ref_off"] = CR.CIIP_ON, num_intra, self.at
            self.lines.append(np.asarray(line, np.int16)); self.at += line.size
        self.ciip.append(c)

    def done(self):
        items, ext, blend, pos = super().done()
        lines = np.concatenate(self.lines) if self.lines else np.zeros(1, np.int16)
        return items, ext, blend, np.array(self.ciip, PRED_CIIP_DTYPE), lines, pos


def model_list(pl, seed):
    """every luma and chroma size of a CIIP CU as a uni-predicted item (list 0 or list 1), a bi-predicted one and BCW 0 and 4; every vector at a fractional phase in
    both directions; num_intra cycling"""
    b = Builder(pl, seed)
    rng, k = b.rng, 0
    for (w, h, c) in ALL_SIZES:
        n = 32 if c else 16
        f = lambda: (int(rng.integers(1, n)), int(rng.integers(1, n)))
        for kind in range(4):
            rp = ((0, -1) if k % 2 == 0 else (-1, 1)) if kind == 0 else ((0, 1), (1, 0), (0, 1))[kind - 1]
            rp = tuple(2 * c + r if r >= 0 else -1 for r in rp)
            mode, param = ((BL.BLEND_DEFAULT, 0), (BL.BLEND_DEFAULT, 0), (BL.BLEND_BCW, 0), (BL.BLEND_BCW, 4))[kind]
            b.add(w, h, c, 0, (f(), f()), rp, mode, param, num_intra=k % 3)
            k += 1
    return b.done()


def eligible(it, e, bl):
    """can this item of a mixed list carry a CIIP record that is ON?"""
    w, h, c = int(it["width"]), int(it["height"]), int(it["chroma"])
    return int(e["flags"]) == 0 and int(bl["mode"]) != BL.BLEND_GEO and ((w, h) in (CR.CHROMA_SIZES if c else CR.LUMA_SIZES))


def mixed_on_off(pl, seed):
    """blend_cases.mixed_list (plain, BDOF, DMVR, BCW, GEO) with a CIIP array: every second eligible item ON, all others OFF"""
    items, ext, blend, pos = BLC.mixed_list(pl, seed)
    rng = np.random.default_rng(seed + 1)
    ciip, lines, at, k = np.zeros(len(items), PRED_CIIP_DTYPE), [], 0, 0
    for i, it in enumerate(items):
        if not eligible(it, ext[i], blend[i]):
            continue
        k += 1
        if k % 2:
            continue
        w, h, c = int(it["width"]), int(it["height"]), int(it["chroma"])
        pic = pl[3 if c else 1]
        x, y = int(rng.integers(1, pic.shape[1] - w - 2)), int(rng.integers(1, pic.shape[0] - h - 3))
        ciip[i] = (at, CR.CIIP_ON, k % 3, (0, 0))
        lines.append(CR.line_at(pic, x, y, w, h)); at += lines[-1].size
    return items, ext, blend, ciip, np.concatenate(lines), pos


def expected(lib, pl, pos, it, e, bl, ci, lines, bd):
    """one item of a list with extension, blend and CIIP records"""
    inter = BLC.expected(lib, pl, pos, it, e, bl, bd)
    if int(ci["mode"]) == CR.CIIP_OFF:
        return inter
    return CR.ciip(inter, lines[int(ci["ref_off"]):int(ci["ref_off"]) + CR.line_len(int(it["width"]), int(it["height"]))], int(it["chroma"]), int(ci["num_intra"]))


def golden_replay_list(cases, pitch=512, margin=4):
    """every fixture case as one uni-predicted item with a zero fraction on ONE plane that holds the cases' inter blocks (each with `margin` samples around it):
    -> plane [rows + 1, pitch], items, ciip, lines"""
    where, rows = PR.shelf_pack([(c["w"] + 2 * margin, c["h"] + 2 * margin) for c in cases], pitch)
    plane = np.zeros((rows + 1, pitch), np.int16)
    items, ciip, lines, at = np.zeros(len(cases), PRED_ITEM_DTYPE), np.zeros(len(cases), PRED_CIIP_DTYPE), [], 0
    for k, (c, (x, y)) in enumerate(zip(cases, where)):
        x, y = x + margin, y + margin
        plane[y:y + c["h"], x:x + c["w"]] = c["inter"]
        items[k]["width"], items[k]["height"], items[k]["chroma"], items[k]["ref_plane"], items[k]["ref_off"] = c["w"], c["h"], c["chroma"], (0, -1), (y * pitch + x, 0)
        ciip[k] = (at, CR.CIIP_ON, c["num_intra"], (0, 0))
        lines.append(c["line"]); at += c["line"].size
    items["dst_off"] = BLC.compact_offsets(items)[0]
    return plane, items, ciip, np.concatenate(lines)
