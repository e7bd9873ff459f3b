"""numpy model of joint Cb-Cr residual coding (ICT): fwdTransformCbCr / invTransformCbCr of the reference (CommonLib/TrQuant.cpp:95-164), bit-exact for any int16 input —
truncating division, the int16 narrowing of Pel( ... ) and of the Pel stores, arithmetic shifts of the negated int.  Pinned to the reference's own results in
tests/golden/ict.npz by tests/test_ict_cpu.py (the fixture is written by tests/ict_golden_gen.py)."""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ict.npz")
ICT_MODES = ((0, 3, 1, 2), (0, -3, -1, -2))      # g_ictModes[jointCbCrSign][cbfMask] (Rom.cpp:1453)
MODES = (1, -1, 2, -2, 3, -3)
ICT_ITEM_DTYPE = np.dtype([("cb_off", "<i4"), ("cr_off", "<i4"), ("stride", "<i4"), ("joint_off", "<i4"), ("stats_idx", "<i4"), ("width", "<i2"), ("height", "<i2"),
                           ("mode", "i1"), ("rsv", "u1", (3,))])      # vvhip_ict_item (28 bytes)
SIZES = [(w, h) for w in (2, 4, 8, 16, 32, 64) for h in (2, 4, 8, 16, 32, 64)]


def _narrow(v):
    """int -> int16 the way a C conversion to Pel does: modulo 2^16"""
    return np.asarray(v, np.int64).astype(np.int16)


def _tdiv(t, d):
    """C's t / d on ints: truncation toward zero"""
    t = np.asarray(t, np.int64)
    return np.sign(t) * (np.abs(t) // d)


def fwd(cb, cr, mode):
    """-> (joint block int16 or None for mode 0, d1, d2) — python ints"""
    cb, cr = np.asarray(cb, np.int16).astype(np.int64), np.asarray(cr, np.int16).astype(np.int64)
    if mode == 0:
        return None, int((cb * cb).sum()), int((cr * cr).sum())
    s = 1 if mode > 0 else -1
    if abs(mode) == 1:
        c = _narrow(_tdiv(4 * cb + s * 2 * cr, 5)).astype(np.int64)
        d = (cb - c) ** 2 + (cr - ((s * c) >> 1)) ** 2
    elif abs(mode) == 2:
        c = _narrow(_tdiv(cb + s * cr, 2)).astype(np.int64)
        d = (cb - c) ** 2 + (cr - s * c) ** 2
    elif abs(mode) == 3:
        c = _narrow(_tdiv(4 * cr + s * 2 * cb, 5)).astype(np.int64)
        d = (cb - ((s * c) >> 1)) ** 2 + (cr - c) ** 2
    else:
        raise ValueError("ICT mode %d" % mode)
    return c.astype(np.int16), int(d.sum()), 0


def inv(joint, mode):
    """the joint reconstruction is the coded component (Cb for |mode| = 1, 2; Cr for |mode| = 3) -> (cb, cr) int16"""
    c = np.asarray(joint, np.int16).astype(np.int64)
    s = 1 if mode > 0 else -1
    if abs(mode) == 1:
        return c.astype(np.int16), _narrow((s * c) >> 1)
    if abs(mode) == 2:
        return c.astype(np.int16), _narrow(s * c)
    if abs(mode) == 3:
        return _narrow((s * c) >> 1), c.astype(np.int16)
    raise ValueError("ICT mode %d has no inverse" % mode)


def sse(a, b):
    d = np.asarray(a, np.int64) - np.asarray(b, np.int64)
    return int((d * d).sum())


def golden_cases():
    """-> list of dicts: mode, w, h, kind (0 sweep, 1 every mode, 2 extremes), cb, cr and the reference's d1, d2 and, for mode != 0, joint, ( rec_cb, rec_cr ) = invTransformICT
    run on the joint block and ( in_cb, in_cr ) = invTransformICT run with the case's own input block as the coded component"""
    z = np.load(GOLDEN)
    out = []
    for i in range(int(z["n"])):
        k = "c%03d_" % i
        mode, w, h, kind = (int(v) for v in z[k + "hdr"])
        c = dict(mode=mode, w=w, h=h, kind=kind, cb=z[k + "cb"], cr=z[k + "cr"], d1=int(z[k + "dist"][0]), d2=int(z[k + "dist"][1]), joint=None, rec_cb=None, rec_cr=None,
                 in_cb=None, in_cr=None)
        if mode != 0:
            c["joint"], c["rec_cb"], c["rec_cr"], c["in_cb"], c["in_cr"] = z[k + "joint"], z[k + "rec_cb"], z[k + "rec_cr"], z[k + "in_cb"], z[k + "in_cr"]
        out.append(c)
    return out
