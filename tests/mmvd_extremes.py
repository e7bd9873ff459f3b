"""The limits list of the MMVD merge-candidate entry: CUs on two-level planes ( 0 and the maximum ) at 12 bits — half-sample fractions overshoot, bcw_idx 0 and 4 ( weights
-2 : 10 and 10 : -2 ) drive both ends of the final clip —, a 128 x 128 CU whose Hadamard cost comes closest to the bound that makes 32 bits enough, and base vectors at
+-( 2^17 - 1 ), where the storage clip and then the picture clip act.  The CPU tier asserts that the list reaches these; the GPU tier replays it."""
import mmvd_cases as MC
import mmvd_ref as MR


def cases():
    S, G = ("small", 12, "HAD", 0), ("large", 12, "HAD", 0)
    Sf = ("small", 12, "HAD_fast", 0)
    L = []
    for name, bcw in (("clip_bcw0", 0), ("clip_bcw4", 4)):
        L.append(dict(MC.cu(name, S, 16, 16, 32, 32, MC.base((8, 8), (-24, 40), ref=(0, 2), bcw=bcw, poc=(-1, 2)), MC.base((24, -8), (8, 8), ref=(2, 0), bcw=bcw, poc=(-2, -2), alt=1)), planes="two_level"))
    L.append(dict(MC.cu("two_level_8x4", Sf, 8, 4, 48, 16, MC.base((8, 24), None), MC.base(None, (-8, 8), alt=1)), planes="two_level"))
    L.append(dict(MC.cu("two_level_32x32", Sf, 32, 32, 64, 48, MC.base((8, 8), (8, -8), bcw=4, poc=(1, -1)), None, mask=(0x00FF00FF, 0)), planes="two_level"))
    v = MR.MV_MAX
    L.append(dict(MC.cu("far_vectors", S, 8, 16, 40, 24, MC.base((v, -v), (-v, v), poc=(-1, 3), bcw=1), MC.base((-v, -v), None)), planes="two_level"))
    L.append(dict(MC.cu("far_vectors_b", Sf, 16, 8, 16, 56, MC.base(None, (v, v)), MC.base((-v - 1, v), (v, -v - 1), poc=(4, -4))), planes="two_level"))
    # the cost bound: candidate 0 of base 0 is the whole vector ( 0, 0 ) into plane 1, whose 8 x 8 pattern the original inverts — every difference is +-4095 and every
    # Hadamard coefficient of every tile has the magnitude 8 * 4095, the most the sum of magnitudes can be ( 64 * sqrt( 64 * 4095^2 ) by Cauchy-Schwarz )
    L.append(dict(MC.cu("bound_128x128", G, 128, 128, 64, 64, MC.base((-4, 0), None, ref=(1, 0)), MC.base(None, (16, 32), ref=(0, 2)), mask=(0x00000101, 0x00010001)), planes="two_level"))
    return L
