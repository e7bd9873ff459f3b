"""HotPath — Python host layer over the C ABI (include/vvenc_hip.h).

Mirrors the reference's kernel-object interface for this path in batched form:
  RdCost      -> dist_batch / sad_x5_batch / sad_surface     (CommonLib/RdCost.h:117-121)
  TCoeffOps   -> fwd_transform / inv_transform               (CommonLib/TrQuant_EMT.h:63-91 via TrQuant::xT/xIT)
  Quant       -> quant / dequant / need_rdoq / tu_rdo        (CommonLib/Quant.h:143-151)
  MCTF        -> mctf_error_batch / mctf_me_level / mctf_motion_estimation (CommonLib/MCTF.h:160-170)

All tensors are torch CUDA tensors (HBM resident); only raw pointers cross the ABI.  torch is
plumbing here (device memory + streams), nothing is computed with torch ops.
"""
import ctypes as C

import numpy as np
import torch

from .lib import VVHipError, load_library

DF = {"SSE": 0, "SAD": 1, "HAD": 2, "HAD_fast": 3, "HAD_2SAD": 4}
DCT2, DCT8, DST7 = 0, 1, 2

MV_DTYPE = np.dtype([("x", "<i4"), ("y", "<i4"), ("error", "<i4"), ("rmsme", "<i4"), ("overlap", "<f8")])
DMVR_ITEM_DTYPE = np.dtype([("ref0_off", "<i4"), ("ref1_off", "<i4"), ("frac0_x", "<i2"), ("frac0_y", "<i2"), ("frac1_x", "<i2"), ("frac1_y", "<i2")])
DMVR_RESULT_DTYPE = np.dtype([("mvd_x", "<i2"), ("mvd_y", "<i2"), ("pad", "<i4"), ("min_cost", "<u8")])
SUBPEL_DTYPE = np.dtype([("org_off", "<i4"), ("ref_off", "<i4"), ("frac_x", "<i2"), ("frac_y", "<i2")])
PRED_ITEM_DTYPE = np.dtype([("dst_off", "<i4"), ("org_off", "<i4"), ("ref_off", "<i4", (2,)), ("frac", "<i2", (2, 2)), ("width", "<i2"), ("height", "<i2"),
                            ("ref_plane", "i1", (2,)), ("chroma", "u1"), ("alt_hpel", "u1")])      # vvhip_pred_item (32 bytes)
PRED_EXT_DTYPE = np.dtype([("flags", "u1"), ("pad_dx", "i1", (2,)), ("pad_dy", "i1", (2,)), ("rsv", "u1", (3,))])      # vvhip_pred_ext (8 bytes)
PRED_EXT_BDOF, PRED_EXT_DMVR_PAD = 1, 2
PRED_BLEND_DTYPE = np.dtype([("mode", "u1"), ("param", "u1"), ("rsv", "u1", (2,))])      # vvhip_pred_blend (4 bytes)
PRED_BLEND_DEFAULT, PRED_BLEND_BCW, PRED_BLEND_GEO = 0, 1, 2      # param: - / bcw_idx 0..4 / geoSplitDir 0..63
PRED_CIIP_DTYPE = np.dtype([("ref_off", "<i4"), ("mode", "u1"), ("num_intra", "u1"), ("rsv", "u1", (2,))])      # vvhip_pred_ciip (8 bytes)
PRED_CIIP_OFF, PRED_CIIP_ON = 0, 1      # ON: ref_off = the block's line top[0 .. w + 2], left[0 .. h + 2] in intra_ref; num_intra 0..2
PRED_AFFINE_ITEM_DTYPE = np.dtype([("dst_off", "<i4"), ("org_off", "<i4"), ("ref_off", "<i4", (2,)), ("cpmv", "<i4", (2, 3, 2)), ("cu_x", "<i2"), ("cu_y", "<i2"), ("cu_w", "<i2"),
                                   ("cu_h", "<i2"), ("ref_plane", "i1", (2,)), ("chroma", "u1"), ("six_param", "u1"), ("prof", "u1"), ("rsv", "u1", (3,))])      # vvhip_pred_affine_item (80 bytes)


def dmvr_pred_items(results, start_mv, pos, ref_planes, strides, dx, dy, bdof=True, chroma_planes=None, chroma_strides=None):
    """the final motion compensation of DMVR sub-blocks as a prediction list (DMVR::xFinalPaddedMCForDMVR, CommonLib/InterPrediction.cpp:1189-1225).
    results = DMVR_RESULT_DTYPE records of vvhip_dmvr_refine_batch; start_mv[i][l] = the (clipped) merge vector (x, y) of list l in 1/16 sample; pos[i] = the sub-block's
    luma position (x, y) in the picture (plane coordinates, margins included); ref_planes = (plane index of list 0, of list 1), strides their row pitches; dx, dy the
    sub-block size.  List 0 moves by +mvd, list 1 by -mvd; the integer deltas are ( refined >> shift ) - ( start >> shift ) per component scale; BDOF is the caller's flag
    AND min_cost >= 2 * dx * dy (:1307, :1384).  With chroma_planes = ((cb0, cb1), (cr0, cr1)) two 4:2:0 chroma items per sub-block follow the luma items.
    -> (items, ext): PRED_ITEM_DTYPE / PRED_EXT_DTYPE records, dst_off / org_off zero (the caller lays the output out)."""
    res = np.ascontiguousarray(results).view(DMVR_RESULT_DTYPE).reshape(-1)
    n = res.size
    comps = [(0, ref_planes, strides, dx, dy)]
    for pl in (chroma_planes or ()):
        comps.append((1, pl, chroma_strides, dx // 2, dy // 2))
    items, ext = np.zeros(n * len(comps), PRED_ITEM_DTYPE), np.zeros(n * len(comps), PRED_EXT_DTYPE)
    for c, (chroma, planes, strd, w, h) in enumerate(comps):
        shift = 4 + chroma
        for i in range(n):
            k = c * n + i
            it, e = items[k], ext[k]
            it["width"], it["height"], it["chroma"], it["ref_plane"] = w, h, chroma, planes
            mvd = (int(res[i]["mvd_x"]), int(res[i]["mvd_y"]))
            moved = False
            for l in (0, 1):
                sx, sy = int(start_mv[i][l][0]), int(start_mv[i][l][1])
                rx, ry = (sx + mvd[0], sy + mvd[1]) if l == 0 else (sx - mvd[0], sy - mvd[1])
                px, py = int(pos[i][0]) >> chroma, int(pos[i][1]) >> chroma
                it["ref_off"][l] = (py + (ry >> shift)) * strd[l] + px + (rx >> shift)
                it["frac"][l] = (rx & ((1 << shift) - 1), ry & ((1 << shift) - 1))
                e["pad_dx"][l], e["pad_dy"][l] = (rx >> shift) - (sx >> shift), (ry >> shift) - (sy >> shift)
                moved = moved or e["pad_dx"][l] != 0 or e["pad_dy"][l] != 0
            fl = PRED_EXT_DMVR_PAD if moved else 0
            if not moved:
                e["pad_dx"], e["pad_dy"] = 0, 0
            if not chroma and bdof and int(res[i]["min_cost"]) >= 2 * dx * dy:
                fl |= PRED_EXT_BDOF
            e["flags"] = fl
    return items, ext
STATS_DTYPE = np.dtype([("abs_sum", "<i4"), ("last_scan_pos", "<i4"), ("need_rdoq", "<i4"), ("pad", "<i4"), ("sse", "<u8")])
ICT_ITEM_DTYPE = np.dtype([("cb_off", "<i4"), ("cr_off", "<i4"), ("stride", "<i4"), ("joint_off", "<i4"), ("stats_idx", "<i4"), ("width", "<i2"), ("height", "<i2"),
                           ("mode", "i1"), ("rsv", "u1", (3,))])      # vvhip_ict_item (28 bytes)
ICT_MODES = ((0, 3, 1, 2), (0, -3, -1, -2))      # g_ictModes[jointCbCrSign][cbfMask] (Rom.cpp:1453)


def make_ict_items(blocks):
    """the joint Cb-Cr items of a list of chroma TUs: blocks = (cb_off, cr_off, stride, width, height, mode) each -> (items, samples of the joint buffer): ICT_ITEM_DTYPE
    records with stats_idx = -1 and the joint blocks laid out compactly, grouped by size in list order inside a size — the blocks of one size are then one compact TU job
    (d_resi_off = their joint_off, pitch = width) whose compact reconstruction of n * w * h samples lands at the same offsets.  Items of mode 0 code no joint block."""
    it = np.zeros(len(blocks), ICT_ITEM_DTYPE)
    for k, (cb, cr, stride, w, h, mode) in enumerate(blocks):
        it[k]["cb_off"], it[k]["cr_off"], it[k]["stride"], it[k]["width"], it[k]["height"], it[k]["mode"], it[k]["stats_idx"] = cb, cr, stride, w, h, mode, -1
    at = 0
    for w, h in sorted({(int(i["width"]), int(i["height"])) for i in it}, reverse=True):
        for k in range(len(it)):
            if (int(it[k]["width"]), int(it[k]["height"])) == (w, h) and int(it[k]["mode"]) != 0:
                it[k]["joint_off"] = at
                at += w * h
    return it, at


SBT_ITEM_DTYPE = np.dtype([("y_off", "<i4"), ("cb_off", "<i4"), ("cr_off", "<i4"), ("stride_y", "<i4"), ("stride_c", "<i4"), ("width", "<i2"), ("height", "<i2"),
                           ("sbt_allowed", "u1"), ("rsv", "u1", (3,))])      # vvhip_sbt_item (28 bytes)
SBT_TILE_DTYPE = np.dtype([("resi_off", "<i4"), ("stride", "<i4"), ("x", "<i2"), ("y", "<i2"), ("width", "<i2"), ("height", "<i2"), ("tr_hor", "i1"), ("tr_ver", "i1"),
                           ("rsv", "u1", (2,))])      # vvhip_sbt_tile (20 bytes)
SBT_PLACE_DTYPE = np.dtype([("y_off", "<i4"), ("cb_off", "<i4"), ("cr_off", "<i4"), ("stride_y", "<i4"), ("stride_c", "<i4"), ("tile_off", "<i4", (3,)), ("stats_idx", "<i4", (3,)),
                            ("width", "<i2"), ("height", "<i2"), ("sbt_allowed", "u1"), ("mode", "u1"), ("rsv", "u1", (2,))])      # vvhip_sbt_place_item (52 bytes)
SBT_VER_HALF, SBT_HOR_HALF, SBT_VER_QUAD, SBT_HOR_QUAD = 1, 2, 3, 4      # SbtIdx (TypeDef.h:266-270): the bits of sbt_allowed; SBT mode = 2 * ( idx - 1 ) + pos
SAO_PARAM_DTYPE = np.dtype([("type", "i1"), ("avail", "u1"), ("band", "u1"), ("rsv", "u1"), ("offs", "<i2", (5,))])      # vvhip_sao_param (14 bytes)
SAO_OFF, SAO_EO_0, SAO_EO_90, SAO_EO_135, SAO_EO_45, SAO_BO = -1, 0, 1, 2, 3, 4
SAO_LEFT, SAO_ABOVE, SAO_ABOVE_LEFT, SAO_RIGHT, SAO_BELOW, SAO_ABOVE_RIGHT = 1, 2, 4, 8, 16, 32      # VVHIP_SAO_*: the statistics flags of a CTU
# the reference's availability mask of the filter (SampleAdaptiveOffset.h:75-85)
SAO_AVAIL_LEFT, SAO_AVAIL_RIGHT, SAO_AVAIL_ABOVE, SAO_AVAIL_BELOW, SAO_AVAIL_ABOVE_LEFT, SAO_AVAIL_ABOVE_RIGHT, SAO_AVAIL_BELOW_LEFT, SAO_AVAIL_BELOW_RIGHT = 1, 2, 4, 8, 16, 32, 64, 128
SAO_REC = 320      # VVHIP_SAO_REC: int64 per CTU and plane, [5][2][32] = SAOStatData[5]
LF_PARAM_DTYPE = np.dtype([("qp", "i1", (3,)), ("bs", "u1"), ("side_max_filt_length", "u1"), ("flags", "u1")])      # vvhip_lf_param (6 bytes) = LoopFilterParam
DBK_VER, DBK_HOR = 1, 2      # VVHIP_DBK_*
VISACT_AREA_DTYPE = np.dtype([("plane", "u1"), ("ds", "u1"), ("order", "u1"), ("rsv0", "u1"), ("x", "<i4"), ("y", "<i4"), ("w", "<i4"), ("h", "<i4"),
                              ("mx", "<i4"), ("my", "<i4"), ("mw", "<i4"), ("mh", "<i4"), ("rsv1", "<i4")])      # vvhip_visact_area (40 bytes)
INTRA_ITEM_DTYPE = np.dtype([("w", "u1"), ("h", "u1"), ("bit_depth", "u1"), ("multi_ref_idx", "u1"), ("ref_off", "<i4"), ("org_off", "<i4"), ("pred_off", "<i4"),
                             ("cost_off", "<i4"), ("mode_mask", "<u4", (3,)), ("pred_mask", "<u4", (3,)), ("rsv", "<u4")])      # vvhip_intra_item (48 bytes)
INTRA_MODES = 67      # NUM_LUMA_MODE: the cost slots of an item
INTRA_CHROMA_ITEM_DTYPE = np.dtype([("w", "u1"), ("h", "u1"), ("bit_depth", "u1"), ("flags", "u1"), ("n_above_right", "u1"), ("n_left_below", "u1"), ("mode_mask", "u1"),
                                    ("pred_mask", "u1"), ("cand", "u1", 8), ("luma_off", "<i4"), ("luma_stride", "<i4"), ("ref_off", "<i4", 2), ("org_off", "<i4", 2),
                                    ("pred_off", "<i4", 2), ("cost_off", "<i4"), ("rsv", "u1", 12)])      # vvhip_intra_chroma_item (64 bytes)
INTRA_CHROMA_SLOTS = 8      # NUM_CHROMA_MODE: the candidate and cost slots of an item
ICH_ABOVE, ICH_LEFT, ICH_FIRST_ROW, ICH_VER_COLLOCATED = 1, 2, 4, 8
MMVD_ITEM_DTYPE = np.dtype([("cu_x", "<i2"), ("cu_y", "<i2"), ("w", "u1"), ("h", "u1"), ("rsv0", "u1", 2), ("org_off", "<i4"), ("cost_off", "<i4"), ("cand_mask", "<u4", 2),
                            ("mv", "<i4", (2, 2, 2)), ("ref_off", "<i4", (2, 2)), ("poc_delta", "<i4", (2, 2)), ("ref_plane", "i1", (2, 2)), ("long_term", "u1", 2),
                            ("bcw_idx", "u1", 2), ("alt_hpel", "u1", 2), ("rsv", "u1", 14)])      # vvhip_mmvd_item (112 bytes)
MMVD_CAND_DTYPE = np.dtype([("mv", "<i4", (2, 2)), ("stored_mv", "<i4", (2, 2)), ("ref_plane", "i1", 2), ("bcw_idx", "u1"), ("alt_hpel", "u1")])      # vvhip_mmvd_cand (36 bytes)
MMVD_SLOTS = 64      # MmvdIdx::ADD_NUM: the cost slots of an item, indexed by position | step << 2 | baseIdx << 5
SBT_MAX_DIST = (1 << 64) - 1      # MAX_DISTORTION: the estimate of a mode whose type is not allowed


def sbt_allowed_of(w, h):
    """CU::checkAllowedSbt's size rule (UnitTools.cpp:256-267): halves from a side of 8, quads from a side of 16"""
    return ((w >= 8) << SBT_VER_HALF) | ((h >= 8) << SBT_HOR_HALF) | ((w >= 16) << SBT_VER_QUAD) | ((h >= 16) << SBT_HOR_QUAD)


def make_sbt_items(cus):
    """the SBT items of a list of CUs: cus = (y_off, cb_off, cr_off, stride_y, stride_c, width, height, sbt_allowed) each -> SBT_ITEM_DTYPE records"""
    it = np.zeros(len(cus), SBT_ITEM_DTYPE)
    for k, cu in enumerate(cus):
        for name, v in zip(("y_off", "cb_off", "cr_off", "stride_y", "stride_c", "width", "height", "sbt_allowed"), cu):
            it[k][name] = v
    return it


def sbt_coded_tile(w, h, mode):
    """the coded tile (x, y, width, height) of a w x h component block: getSbtTuTiling's factors ( dim * f ) >> 2 (UnitPartitioner.cpp:995-1056); tile 0 for position 0,
    tile 1 for position 1"""
    ver, quad, pos1 = ((mode >> 1) & 1) == 0, mode >= 4, mode & 1
    side = w if ver else h
    length, at = (side * (1 if quad else 2)) >> 2, ((side * (3 if quad else 2)) >> 2) if pos1 else 0
    return (at, 0, length, h) if ver else (0, at, w, length)


def sbt_tiles(item, mode):
    """the Python mirror of vvhip_sbt_tiles: the coded tile of each component (Y, Cb, Cr) of one SBT_ITEM_DTYPE record as SBT_TILE_DTYPE records — where it lies, the offset of
    its corner, the CU's pitch and the luma transform types of TrQuant::xSetTrTypes' SBT branch (TrQuant.cpp:435-466); chroma is DCT-2"""
    W, H = int(item["width"]), int(item["height"])
    ver, quad, pos1 = ((mode >> 1) & 1) == 0, mode >= 4, mode & 1
    if not 0 <= mode <= 7 or (W if ver else H) < (16 if quad else 8):
        raise ValueError("sbt_tiles: SBT mode %d on a %dx%d CU" % (mode, W, H))
    out = np.zeros(3, SBT_TILE_DTYPE)
    for c, (off, stride) in enumerate(((item["y_off"], item["stride_y"]), (item["cb_off"], item["stride_c"]), (item["cr_off"], item["stride_c"]))):
        x, y, w, h = sbt_coded_tile(W >> (c > 0), H >> (c > 0), mode)
        o = out[c]
        o["resi_off"], o["stride"], o["x"], o["y"], o["width"], o["height"] = int(off) + y * int(stride) + x, stride, x, y, w, h
        if c == 0 and (h if ver else w) <= 32:
            o["tr_hor"], o["tr_ver"] = (DCT8 if ver and not pos1 else DST7), (DCT8 if not ver and not pos1 else DST7)
    return out


def _ptr(t):
    if t is None:
        return None
    assert t.is_cuda and t.is_contiguous(), "device-resident contiguous tensors only"
    return C.c_void_p(t.data_ptr())


class Plane:
    """A picture plane in HBM with `pad` samples of margin on every side (int16 samples).

    `buf_ptr` addresses sample (0,0); stride is in samples, like the reference's CPelBuf
    (CommonLib/Buffer.h:149-159).
    """

    def __init__(self, device, width, height, pad=0, stride=None):
        self.width, self.height, self.pad = int(width), int(height), int(pad)
        self.stride = int(stride) if stride else ((self.width + 2 * self.pad + 7) // 8) * 8
        self.storage = torch.zeros((self.height + 2 * self.pad, self.stride), dtype=torch.int16, device=device)

    @classmethod
    def from_numpy(cls, device, arr, pad=0):
        arr = np.ascontiguousarray(arr, np.int16)
        p = cls(device, arr.shape[1], arr.shape[0], pad)
        p.storage[p.pad:p.pad + p.height, p.pad:p.pad + p.width] = torch.from_numpy(arr).to(device)
        return p

    @property
    def origin(self):
        return self.pad * self.stride + self.pad      # element offset of sample (0,0) inside storage

    @property
    def buf_ptr(self):
        return C.c_void_p(self.storage.data_ptr() + 2 * self.origin)

    def offset(self, x, y):
        return y * self.stride + x

    def visible(self):
        return self.storage[self.pad:self.pad + self.height, self.pad:self.pad + self.width]


class PlaneView:
    """width x height samples at element `offset` of a device int16 tensor, line pitch `stride`: a plane at any base alignment and pitch (what the SAO entries accept)"""

    def __init__(self, storage, offset, stride, width, height):
        assert storage.is_cuda and storage.dtype == torch.int16 and storage.is_contiguous()
        assert offset >= 0 and offset + (height - 1) * stride + width <= storage.numel()
        self.storage, self.off, self.stride, self.width, self.height = storage, int(offset), int(stride), int(width), int(height)

    @property
    def buf_ptr(self):
        return C.c_void_p(self.storage.data_ptr() + 2 * self.off)

    def visible(self):
        return torch.as_strided(self.storage.view(-1), (self.height, self.width), (self.stride, 1), self.off)


class HotPath:
    def __init__(self, device=None):
        self.L = load_library()
        if not torch.cuda.is_available():
            raise VVHipError("no GPU visible: vvenc_amd has no CPU fallback (HIP path only)")
        self.device = torch.device(device if device is not None else "cuda:%d" % torch.cuda.current_device())
        idx = self.device.index if self.device.index is not None else torch.cuda.current_device()
        ctx = C.c_void_p()
        rc = self.L.vvhip_create(C.byref(ctx), idx)
        if rc != 0:
            raise VVHipError("vvhip_create failed (%d): %s" % (rc, self.L.vvhip_last_error(None).decode()))
        self.ctx = ctx
        self.use_torch_stream()

    def fork(self, stream=None):
        """a second context on the same device, bound for good to `stream` (a torch.cuda.Stream): launches of independent work lists go to their own streams without any
        per-call stream switching on the host (what the binding's worker threads do with their per-thread contexts).
        stream=None: the lane IS the new context's own stream (wrapped as a torch ExternalStream for events and waits) — no second stream per lane: the runtime deals HIP
        streams onto $GPU_MAX_HW_QUEUES hardware queues in creation order, and a lane that shares its queue with another busy lane is serialized behind it
        (profiles/r06_hw_queues.log)"""
        o = object.__new__(HotPath)
        o.L, o.device = self.L, self.device
        idx = self.device.index if self.device.index is not None else torch.cuda.current_device()
        ctx = C.c_void_p()
        rc = self.L.vvhip_create(C.byref(ctx), idx)
        if rc != 0:
            raise VVHipError("vvhip_create failed (%d): %s" % (rc, self.L.vvhip_last_error(None).decode()))
        o.ctx = ctx
        if stream is None:
            with torch.cuda.device(self.device):
                o.stream = torch.cuda.ExternalStream(int(self.L.vvhip_get_stream(ctx)))
            return o
        o.stream = stream
        o._ck(self.L.vvhip_set_stream(ctx, C.c_void_p(stream.cuda_stream)))
        return o

    def bound(self, fn_name, *args):
        """a zero-argument callable issuing L.<fn_name>(ctx, *args) with the ctypes arguments converted once (per-step launches of fixed work lists)"""
        fn, ctx, a, ck = getattr(self.L, fn_name), self.ctx, args, self._ck

        def call():
            rc = fn(ctx, *a)
            if rc:
                ck(rc)
        return call

    def close(self):
        if getattr(self, "ctx", None):
            self.L.vvhip_destroy(self.ctx)
            self.ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- plumbing ----
    def _ck(self, rc):
        if rc != 0:
            raise VVHipError("vvenc_hip error %d: %s" % (rc, self.L.vvhip_last_error(self.ctx).decode()))

    def use_torch_stream(self):
        """run on torch's current stream so tensor ops and kernels are ordered"""
        with torch.cuda.device(self.device):
            self._ck(self.L.vvhip_set_stream(self.ctx, C.c_void_p(torch.cuda.current_stream().cuda_stream)))

    # ---- launch graphs: record a fixed sequence of batch calls once, replay it with one hipGraphLaunch ----
    def graph_capture(self, fn):
        """runs fn() under stream capture (fn may only issue batch calls whose scratch already exists) -> graph handle for graph_launch"""
        self.use_own_stream()                        # torch's current stream may be the legacy default stream, which cannot be captured
        try:
            self._ck(self.L.vvhip_graph_begin(self.ctx))
            try:
                fn()
            finally:
                g = C.c_void_p()
                rc = self.L.vvhip_graph_end(self.ctx, C.byref(g))
            self._ck(rc)
        finally:
            self.use_torch_stream()
        return g

    def graph_launch(self, g):
        self._ck(self.L.vvhip_graph_launch(self.ctx, g))

    def graph_destroy(self, g):
        self.L.vvhip_graph_destroy(g)

    def use_own_stream(self):
        self._ck(self.L.vvhip_use_own_stream(self.ctx))

    def stream_handle(self):
        return self.L.vvhip_get_stream(self.ctx)

    def sync(self):
        self._ck(self.L.vvhip_sync(self.ctx))

    def to_device(self, arr, dtype=None):
        a = np.ascontiguousarray(arr, dtype) if dtype is not None else np.ascontiguousarray(arr)
        if a.dtype.fields is not None:
            return torch.from_numpy(a.view(np.uint8).reshape(a.shape + (a.dtype.itemsize,))).to(self.device)
        if a.dtype == np.uint64:
            a = a.view(np.int64)
        if a.dtype == np.uint32:
            a = a.view(np.int32)
        if a.dtype == np.uint16:
            a = a.view(np.int16)
        return torch.from_numpy(a).to(self.device)

    def plane(self, arr, pad=0, extend=True):
        p = Plane.from_numpy(self.device, arr, pad)
        if pad and extend:
            self.extend_border(p)
        return p

    @staticmethod
    def items(pairs):
        """numpy (n,2) int32 array of (org_off, cur_off)"""
        return np.ascontiguousarray(pairs, np.int32).reshape(-1, 2)

    # ---- (A) distortion ----
    def dist_batch(self, func, org, cur, d_items, n, w, h, sub_shift=0, bit_depth=10, out=None):
        if out is None:
            out = torch.empty(n, dtype=torch.int64, device=self.device)
        self._ck(self.L.vvhip_dist_batch(self.ctx, DF[func] if isinstance(func, str) else func, org.buf_ptr, org.stride,
                                         cur.buf_ptr, cur.stride, w, h, sub_shift, bit_depth, _ptr(d_items), n, _ptr(out)))
        return out

    class _DistJob(C.Structure):
        _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("sub_shift", C.c_int32), ("n", C.c_int32), ("d_items", C.c_void_p), ("d_out", C.c_void_p)]

    def make_dist_jobs(self, jobs):
        """jobs: list of (w, h, sub_shift, n, d_items, d_out) -> prepared host job table (keep the tensors alive while it is in use)"""
        arr = (self._DistJob * len(jobs))(*[self._DistJob(w, h, ss, n, it.data_ptr(), out.data_ptr()) for (w, h, ss, n, it, out) in jobs])
        return arr, len(jobs), jobs

    def dist_multi(self, func, org, cur, jobs, bit_depth=10):
        """one merged launch per function where the kernels allow it; `jobs` = list of tuples or a table from make_dist_jobs"""
        if isinstance(jobs, list):
            jobs = self.make_dist_jobs(jobs)
        self._ck(self.L.vvhip_dist_multi(self.ctx, DF[func] if isinstance(func, str) else func, org.buf_ptr, org.stride, cur.buf_ptr, cur.stride,
                                         bit_depth, jobs[0], jobs[1]))

    class _DistFJob(C.Structure):
        _fields_ = [("func", C.c_int32), ("width", C.c_int32), ("height", C.c_int32), ("sub_shift", C.c_int32), ("n", C.c_int32), ("flags", C.c_int32),
                    ("d_items", C.c_void_p), ("d_out", C.c_void_p)]

    DIST_FLAG_SAMPLES = 1      # VVHIP_DIST_FLAG_SAMPLES: both operands are samples in [0, 2^bit_depth)

    def make_dist_fjobs(self, jobs, flags=0):
        """jobs: list of (func, w, h, sub_shift, n, d_items, d_out) -> prepared host job table for dist_multi_func"""
        arr = (self._DistFJob * len(jobs))(*[self._DistFJob(DF[f] if isinstance(f, str) else f, w, h, ss, n, flags, it.data_ptr(), out.data_ptr()) for (f, w, h, ss, n, it, out) in jobs])
        return arr, len(jobs), jobs

    def dist_multi_func(self, org, cur, jobs, bit_depth=10):
        """a frame's distortion lists with a function per job; SAD+SSE and HAD+HAD_fast jobs share launches"""
        if isinstance(jobs, list):
            jobs = self.make_dist_fjobs(jobs)
        self._ck(self.L.vvhip_dist_multi_func(self.ctx, org.buf_ptr, org.stride, cur.buf_ptr, cur.stride, bit_depth, jobs[0], jobs[1]))

    # ---- 8x8-tiled copies of planes (one 128-byte cache line = one 8x8 tile): what the 8x8 SAD / SSE lists and every Hadamard list read on the MI355X
    class _TiledPlanes(C.Structure):
        _fields_ = [("d_org_tiled", C.c_void_p), ("d_cur_tiled", C.c_void_p), ("org_margin", C.c_int32), ("cur_margin", C.c_int32), ("d_cur_shift1", C.c_void_p)]

    def tile_plane(self, plane, out=None):
        """tiled copy of a whole padded Plane (re-tile after the plane changes); returns the int16 tensor holding it"""
        rows = plane.storage.shape[0]
        n = int(self.L.vvhip_tiled8_elems(plane.stride, rows))
        if out is None:
            out = torch.empty(n, dtype=torch.int16, device=self.device)
        self._ck(self.L.vvhip_plane_tile8(self.ctx, plane.storage.data_ptr(), plane.stride, rows, out.data_ptr()))
        return out

    def shift_plane(self, plane, out=None):
        """copy of a whole padded Plane shifted by one sample (out[k] == storage[k + 1]): odd sample addresses become dword-aligned loads; re-make after the plane changes"""
        if out is None:
            out = torch.empty_like(plane.storage)
        self._ck(self.L.vvhip_plane_shift1(self.ctx, plane.storage.data_ptr(), plane.storage.numel(), out.data_ptr()))
        return out

    def planes_derive(self, org, cur, org_tiled=None, cur_tiled=None, cur_shift=None):
        """the derived copies of a picture's two planes in one launch (outputs that are None are skipped)"""
        self._ck(self.L.vvhip_planes_derive(self.ctx, org.storage.data_ptr(), org.stride, org.storage.shape[0], org_tiled.data_ptr() if org_tiled is not None else None,
                                            cur.storage.data_ptr(), cur.stride, cur.storage.shape[0], cur_tiled.data_ptr() if cur_tiled is not None else None,
                                            cur_shift.data_ptr() if cur_shift is not None else None))

    def dist_multi_func_tiled(self, org, cur, org_tiled, cur_tiled, jobs, bit_depth=10, cur_shift=None):
        """dist_multi_func with the tiled copies of both planes (either may be None) and the one-sample-shifted copy of the reference plane at hand (identical results)"""
        if isinstance(jobs, list):
            jobs = self.make_dist_fjobs(jobs)
        t = self._TiledPlanes(org_tiled.data_ptr() if org_tiled is not None else None, cur_tiled.data_ptr() if cur_tiled is not None else None, org.pad, cur.pad,
                              cur_shift.data_ptr() + 2 * cur.origin if cur_shift is not None else None)
        self._ck(self.L.vvhip_dist_multi_func_tiled(self.ctx, org.buf_ptr, org.stride, cur.buf_ptr, cur.stride, C.byref(t), bit_depth, jobs[0], jobs[1]))

    def sad_x5_batch(self, org, cur, d_items, n, w, h, sub_shift=1, calc_centre=True, out=None):
        if out is None:
            out = torch.zeros(n * 5, dtype=torch.int64, device=self.device)
        self._ck(self.L.vvhip_sad_x5_batch(self.ctx, org.buf_ptr, org.stride, cur.buf_ptr, cur.stride, w, h, sub_shift,
                                           int(calc_centre), _ptr(d_items), n, _ptr(out)))
        return out

    def sad_mask_batch(self, org, cur, mask, step_x, mask_stride2, d_items, d_mask_off, n, w, h, sub_shift=0, bit_depth=10, out=None):
        """GEO masked SAD (DF_SAD_WITH_MASK); `mask` is a Plane, d_mask_off per-candidate first-sample offsets (or None)"""
        if out is None:
            out = torch.zeros(n, dtype=torch.int64, device=self.device)
        self._ck(self.L.vvhip_sad_mask_batch(self.ctx, org.buf_ptr, org.stride, cur.buf_ptr, cur.stride, mask.buf_ptr, mask.stride, step_x, mask_stride2,
                                             w, h, sub_shift, bit_depth, _ptr(d_items), _ptr(d_mask_off) if d_mask_off is not None else None, n, _ptr(out)))
        return out

    def fix_weighted_sse_batch(self, org, cur, d_items, d_weights, n, w, h, bit_depth=10, out=None):
        """fixed-weight SSE (RdCost::m_fxdWtdPredPtr); d_weights: uint32 per candidate (stored in an int32 tensor)"""
        if out is None:
            out = torch.zeros(n, dtype=torch.int64, device=self.device)
        self._ck(self.L.vvhip_fix_weighted_sse_batch(self.ctx, org.buf_ptr, org.stride, cur.buf_ptr, cur.stride, w, h, bit_depth,
                                                     _ptr(d_items), _ptr(d_weights), n, _ptr(out)))
        return out

    def sad_surface(self, org, ref, d_org_off, d_ref_off, n_blocks, w, h, sub_shift, range_x, range_y, out=None):
        if out is None:
            out = torch.empty(n_blocks * (2 * range_x + 1) * (2 * range_y + 1), dtype=torch.int32, device=self.device)
        self._ck(self.L.vvhip_sad_surface(self.ctx, org.buf_ptr, org.stride, ref.buf_ptr, ref.stride, w, h, sub_shift,
                                          range_x, range_y, _ptr(d_org_off), _ptr(d_ref_off), n_blocks, _ptr(out)))
        return out

    # ---- (B) transform / quant ----
    def fwd_transform(self, resi, d_off, n, w, h, tr_hor=DCT2, tr_ver=DCT2, bit_depth=10, out=None):
        if out is None:
            out = torch.empty(n * w * h, dtype=torch.int32, device=self.device)
        self._ck(self.L.vvhip_fwd_transform_batch(self.ctx, resi.buf_ptr, resi.stride, _ptr(d_off), n, w, h, tr_hor, tr_ver, bit_depth, _ptr(out)))
        return out

    def inv_transform(self, d_coef, n, w, h, resi_out, d_off, tr_hor=DCT2, tr_ver=DCT2, bit_depth=10):
        self._ck(self.L.vvhip_inv_transform_batch(self.ctx, _ptr(d_coef), n, w, h, tr_hor, tr_ver, bit_depth,
                                                  resi_out.buf_ptr, resi_out.stride, _ptr(d_off)))
        return resi_out

    @staticmethod
    def tu_qp(qps, irap=0, luma=1):
        a = np.zeros((len(qps), 2), np.int16)
        a[:, 0] = qps
        a[:, 1] = (np.asarray(irap, np.int16) & 1) | ((np.asarray(luma, np.int16) & 1) << 1)
        return a

    def quant(self, d_coef, n, w, h, d_qp, bit_depth=10, thr_val=8, want_delta_u=True):
        level = torch.empty(n * w * h, dtype=torch.int16, device=self.device)
        du = torch.zeros(n * w * h, dtype=torch.int32, device=self.device) if want_delta_u else None
        s = torch.empty(n, dtype=torch.int32, device=self.device)
        last = torch.empty(n, dtype=torch.int32, device=self.device)
        self._ck(self.L.vvhip_quant_batch(self.ctx, _ptr(d_coef), n, w, h, bit_depth, _ptr(d_qp), thr_val, _ptr(level), _ptr(du), _ptr(s), _ptr(last)))
        return level, du, s, last

    def dequant(self, d_level, n, w, h, d_qp, bit_depth=10):
        out = torch.empty(n * w * h, dtype=torch.int32, device=self.device)
        self._ck(self.L.vvhip_dequant_batch(self.ctx, _ptr(d_level), n, w, h, bit_depth, _ptr(d_qp), _ptr(out)))
        return out

    def need_rdoq(self, d_coef, n, w, h, d_qp, bit_depth=10):
        out = torch.empty(n, dtype=torch.uint8, device=self.device)
        self._ck(self.L.vvhip_need_rdoq_batch(self.ctx, _ptr(d_coef), n, w, h, bit_depth, _ptr(d_qp), _ptr(out)))
        return out

    def tu_rdo(self, resi, d_off, n, w, h, d_qp, tr_hor=DCT2, tr_ver=DCT2, bit_depth=10, thr_val=8, level=None, rec=None, stats=None):
        if level is None:
            level = torch.empty(n * w * h, dtype=torch.int16, device=self.device)
        if rec is None:
            rec = torch.empty(n * w * h, dtype=torch.int16, device=self.device)
        if stats is None:
            stats = torch.empty((n, STATS_DTYPE.itemsize), dtype=torch.uint8, device=self.device)
        self._ck(self.L.vvhip_tu_rdo_batch(self.ctx, resi.buf_ptr, resi.stride, _ptr(d_off), n, w, h, tr_hor, tr_ver, bit_depth,
                                           _ptr(d_qp), thr_val, _ptr(level), _ptr(rec), _ptr(stats)))
        return level, rec, stats

    class _TuJob(C.Structure):
        _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("tr_hor", C.c_int32), ("tr_ver", C.c_int32), ("n", C.c_int32), ("thr_val", C.c_int32),
                    ("d_resi_off", C.c_void_p), ("d_qp", C.c_void_p), ("d_level", C.c_void_p), ("d_rec_resi", C.c_void_p), ("d_stats", C.c_void_p)]

    def make_tu_jobs(self, jobs):
        """jobs: list of (w, h, tr_hor, tr_ver, n, thr_val, d_off, d_qp, level, rec, stats) -> prepared host job table (tensors must stay alive)"""
        arr = (self._TuJob * len(jobs))(*[self._TuJob(w, h, th, tv, n, thr, off.data_ptr(), qp.data_ptr(),
                                                      lv.data_ptr() if lv is not None else None, rc.data_ptr() if rc is not None else None,
                                                      st.data_ptr() if st is not None else None)
                                          for (w, h, th, tv, n, thr, off, qp, lv, rc, st) in jobs])
        return arr, len(jobs), jobs

    def tu_rdo_multi(self, resi, jobs, bit_depth=10):
        """all TU lists of a residual plane in one call (square 8/16/32 sizes share one launch)"""
        if isinstance(jobs, list):
            jobs = self.make_tu_jobs(jobs)
        self._ck(self.L.vvhip_tu_rdo_multi(self.ctx, resi.buf_ptr, resi.stride, bit_depth, jobs[0], jobs[1]))

    def tu_rdo_multi_strided(self, d_resi, strides, jobs, bit_depth=10):
        """the same with a residual row pitch per job (compact per-TU blocks in one buffer: pitch = width)"""
        if isinstance(jobs, list):
            jobs = self.make_tu_jobs(jobs)
        arr = (C.c_int32 * len(strides))(*strides)
        self._ck(self.L.vvhip_tu_rdo_multi_strided(self.ctx, _ptr(d_resi), C.cast(arr, C.c_void_p), bit_depth, jobs[0], jobs[1]))

    # ---- joint Cb-Cr residual coding (ICT) around the TU lists ----
    def ict_fwd_batch(self, resi, items, joint=None, dist=None):
        """vvhip_ict_fwd_batch: resi = int16 DEVICE tensor holding the Cb / Cr residual blocks, items = ICT_ITEM_DTYPE records (HOST array), joint = int16 tensor for the compact
        joint blocks (None only if every mode is 0), dist = int64 tensor [n, 2] for the pair distortions ( d1, d2 ) or None."""
        it = np.ascontiguousarray(items, ICT_ITEM_DTYPE)
        self._ck(self.L.vvhip_ict_fwd_batch(self.ctx, _ptr(resi), it.ctypes.data_as(C.c_void_p) if it.size else None, int(it.size), _ptr(joint), _ptr(dist)))
        return joint, dist

    def ict_inv_batch(self, joint_rec, items, stats=None, rec=None, org_resi=None, sse=None):
        """vvhip_ict_inv_batch: joint_rec = int16 DEVICE tensor of the compact joint reconstructions, stats = the TU job's statistics the items' stats_idx index (or None),
        rec = int16 tensor laid out like the residual (both components are written) or None, org_resi + sse = the original residuals and a uint64-sized tensor [n, 2]
        (torch.int64 storage) for the Cb / Cr SSEs, or None."""
        it = np.ascontiguousarray(items, ICT_ITEM_DTYPE)
        self._ck(self.L.vvhip_ict_inv_batch(self.ctx, _ptr(joint_rec), it.ctypes.data_as(C.c_void_p) if it.size else None, int(it.size), _ptr(stats), _ptr(rec), _ptr(org_resi),
                                            _ptr(sse)))
        return rec, sse

    def make_joint_tu_jobs(self, items, qps, irap=0, tr_hor=DCT2, tr_ver=DCT2, thr_val=8):
        """the TU jobs of the joint blocks of make_ict_items' items (all modes non-zero): one job per size, its TUs in list order, reading the joint buffer at the items'
        joint_off (pitch = width) and reconstructing to the same offsets of a second buffer; qps = the joint QP per item (chroma scale).  Sets the items' stats_idx.
        -> (items, jobs, strides, level, joint_rec, stats): a make_tu_jobs list with the per-job pitches, and the three output buffers the jobs' tensors are views of."""
        it = np.ascontiguousarray(items, ICT_ITEM_DTYPE).copy()
        total = int(max((int(i["joint_off"]) + int(i["width"]) * int(i["height"]) for i in it), default=0))
        level, joint_rec = (torch.zeros(max(total, 1), dtype=torch.int16, device=self.device) for _ in range(2))
        stats = torch.zeros((max(len(it), 1), STATS_DTYPE.itemsize), dtype=torch.uint8, device=self.device)
        qps = np.broadcast_to(np.asarray(qps), (len(it),))
        jobs, strides, first = [], [], 0
        for w, h in sorted({(int(i["width"]), int(i["height"])) for i in it}, reverse=True):
            ks = [k for k in range(len(it)) if (int(it[k]["width"]), int(it[k]["height"])) == (w, h)]
            offs = it["joint_off"][ks].astype(np.int32)
            base = int(offs[0])
            if not np.array_equal(offs, base + w * h * np.arange(len(ks), dtype=np.int32)):
                raise ValueError("make_joint_tu_jobs: the %dx%d joint blocks are not one compact run in list order (make_ict_items lays them out so)" % (w, h))
            it["stats_idx"][ks] = first + np.arange(len(ks))
            jobs.append((w, h, tr_hor, tr_ver, len(ks), thr_val, self.to_device(offs), self.to_device(self.tu_qp(qps[ks], irap, 0)),
                         level[base:base + len(ks) * w * h], joint_rec[base:base + len(ks) * w * h], stats[first:first + len(ks)]))
            strides.append(w)
            first += len(ks)
        return it, jobs, strides, level, joint_rec, stats

    def tu_rdo_joint(self, resi, items, jobs, strides, joint_rec, stats, bit_depth=10, joint=None, dist=None, rec=None, sse=None):
        """the joint chroma chain of a picture's TUs on the device: ict_fwd_batch -> tu_rdo_multi_strided on the joint buffer -> ict_inv_batch (with the jobs' statistics,
        so it holds with sparse outputs on).  resi = int16 DEVICE tensor with the Cb / Cr residuals; items, jobs, strides, joint_rec, stats as make_joint_tu_jobs returns them
        (jobs a list or a prepared make_tu_jobs table).  -> (joint, dist, rec, sse): the joint residuals, the pair distortions [n, 2], the two reconstructed components in the
        layout of resi (elsewhere zero when allocated here), the SSEs [n, 2] (Cb, Cr) against resi."""
        it = np.ascontiguousarray(items, ICT_ITEM_DTYPE)
        n = int(it.size)
        if joint is None:
            joint = torch.empty_like(joint_rec)
        if dist is None:
            dist = torch.empty((n, 2), dtype=torch.int64, device=self.device)
        if rec is None:
            rec = torch.zeros_like(resi)
        if sse is None:
            sse = torch.empty((n, 2), dtype=torch.int64, device=self.device)
        self.ict_fwd_batch(resi, it, joint, dist)
        self.tu_rdo_multi_strided(joint, strides, jobs, bit_depth)
        self.ict_inv_batch(joint_rec, it, stats, rec, resi, sse)
        return joint, dist, rec, sse

    # ---- sub-block transform (SBT) around the TU lists ----
    def sbt_parts_batch(self, resi, items, chroma_weight=1.0, parts=None, est=None, order=None):
        """vvhip_sbt_parts_batch: resi = int16 DEVICE tensor holding the CUs' Y / Cb / Cr residual blocks, items = SBT_ITEM_DTYPE records (HOST array); parts [n, 3, 16] and
        est [n, 9] uint64-sized tensors (torch.int64 storage), order [n, 8] uint8 — each may be None."""
        it = np.ascontiguousarray(items, SBT_ITEM_DTYPE)
        self._ck(self.L.vvhip_sbt_parts_batch(self.ctx, _ptr(resi), it.ctypes.data_as(C.c_void_p) if it.size else None, int(it.size), float(chroma_weight), _ptr(parts), _ptr(est),
                                              _ptr(order)))
        return parts, est, order

    def sbt_tiles(self, item, mode):
        """vvhip_sbt_tiles (the library's own host arithmetic; the module function sbt_tiles mirrors it) -> SBT_TILE_DTYPE [3]"""
        it = np.ascontiguousarray(item, SBT_ITEM_DTYPE).reshape(1)
        out = np.zeros(3, SBT_TILE_DTYPE)
        self._ck(self.L.vvhip_sbt_tiles(it.ctypes.data_as(C.c_void_p), int(mode), out.ctypes.data_as(C.c_void_p)))
        return out

    def sbt_place_batch(self, tile_rec, items, stats=None, rec=None, org_resi=None, sse=None):
        """vvhip_sbt_place_batch: tile_rec = int16 DEVICE tensor of the compact tile reconstructions, items = SBT_PLACE_DTYPE records (HOST array), stats = the TU jobs'
        statistics the items' stats_idx index, rec = int16 tensor laid out like the residual (every CU block is written whole) or None, org_resi + sse = the original
        residuals and a uint64-sized tensor [n, 3] (torch.int64 storage) for the Y / Cb / Cr SSEs, or None."""
        it = np.ascontiguousarray(items, SBT_PLACE_DTYPE)
        self._ck(self.L.vvhip_sbt_place_batch(self.ctx, _ptr(tile_rec), it.ctypes.data_as(C.c_void_p) if it.size else None, int(it.size), _ptr(stats), _ptr(rec), _ptr(org_resi),
                                              _ptr(sse)))
        return rec, sse

    def make_sbt_tu_jobs(self, items, candidates, qps, irap=0, thr_val=8, drop=()):
        """the TU jobs of a list of SBT candidates: items = SBT_ITEM_DTYPE records, candidates = (CU index, SBT mode 0..7) each, qps = per candidate the QPs of (Y, Cb, Cr)
        (or one triple for all).  One TU per component and candidate — the coded tile, read in place in the CUs' residual buffer — grouped into jobs by (width, height,
        types, pitch) with the TUs of a job in list order; levels and reconstruction of a job are compact.  drop = (candidate, component) pairs whose coefficients the caller
        drops (cbf 0): no TU, stats_idx -1.
        -> (place_items, jobs, strides, level, tile_rec, stats): SBT_PLACE_DTYPE records whose tile_off / stats_idx name the TUs' outputs, a make_tu_jobs list with the
        per-job pitches, and the three output buffers the jobs' tensors are views of."""
        it = np.ascontiguousarray(items, SBT_ITEM_DTYPE)
        qps = np.broadcast_to(np.asarray(qps, np.int32), (len(candidates), 3))
        place = np.zeros(len(candidates), SBT_PLACE_DTYPE)
        groups = {}
        for k, (cu, mode) in enumerate(candidates):
            for name in ("y_off", "cb_off", "cr_off", "stride_y", "stride_c", "width", "height", "sbt_allowed"):
                place[k][name] = it[cu][name]
            place[k]["mode"] = mode
            place[k]["stats_idx"] = -1
            for c, t in enumerate(sbt_tiles(it[cu], mode)):
                if (k, c) not in drop:
                    groups.setdefault((int(t["width"]), int(t["height"]), int(t["tr_hor"]), int(t["tr_ver"]), int(t["stride"])), []).append((k, c, int(t["resi_off"])))
        total = sum(((w * h * len(v) + 7) & ~7) for (w, h, _, _, _), v in groups.items())      # (every job's compact outputs start 16-byte aligned)
        n_tus = sum(len(v) for v in groups.values())
        level, tile_rec = (torch.zeros(max(total, 1), dtype=torch.int16, device=self.device) for _ in range(2))
        stats = torch.zeros((max(n_tus, 1), STATS_DTYPE.itemsize), dtype=torch.uint8, device=self.device)
        jobs, strides, first, base = [], [], 0, 0
        for key in sorted(groups, reverse=True):
            w, h, th, tv, stride = key
            tus = groups[key]
            for j, (k, c, _) in enumerate(tus):
                place[k]["tile_off"][c], place[k]["stats_idx"][c] = base + j * w * h, first + j
            qp = np.array([qps[k][c] for (k, c, _) in tus], np.int32)
            luma = np.array([c == 0 for (_, c, _) in tus], np.int16)
            jobs.append((w, h, th, tv, len(tus), thr_val, self.to_device(np.array([o for (_, _, o) in tus], np.int32)), self.to_device(self.tu_qp(qp, irap, luma)),
                         level[base:base + len(tus) * w * h], tile_rec[base:base + len(tus) * w * h], stats[first:first + len(tus)]))
            strides.append(stride)
            first += len(tus)
            base += (len(tus) * w * h + 7) & ~7
        return place, jobs, strides, level, tile_rec, stats

    def tu_rdo_sbt(self, resi, cus, candidates, qps, chroma_weight=1.0, bit_depth=10, irap=0, thr_val=8, drop=()):
        """the SBT chain of a picture's inter CUs on the device: sbt_parts_batch -> tu_rdo_multi_strided on the coded tiles, read in place -> sbt_place_batch (with the jobs'
        statistics, so it holds with sparse outputs on).  resi = int16 DEVICE tensor with the CUs' residual blocks, cus = SBT_ITEM_DTYPE records, candidates = (CU index,
        mode) each, qps as make_sbt_tu_jobs takes them.  Candidates of one CU share its block of the reconstruction, so the r-th candidate of every CU is placed into plane r
        of rec, one placement call per plane.
        -> (parts [n, 3, 16], est [n, 9], order [n, 8], rec [planes, resi.numel()], sse [candidates, 3], levels, stats): levels / stats as make_sbt_tu_jobs lays them out
        (the returned place items of hp.last_sbt_place name them)."""
        it = np.ascontiguousarray(cus, SBT_ITEM_DTYPE)
        n = int(it.size)
        parts = torch.empty((n, 3, 16), dtype=torch.int64, device=self.device)
        est = torch.empty((n, 9), dtype=torch.int64, device=self.device)
        order = torch.empty((n, 8), dtype=torch.uint8, device=self.device)
        self.sbt_parts_batch(resi, it, chroma_weight, parts, est, order)
        place, jobs, strides, level, tile_rec, stats = self.make_sbt_tu_jobs(it, candidates, qps, irap, thr_val, drop)
        self.last_sbt_place = place
        if jobs:
            self.tu_rdo_multi_strided(resi, strides, jobs, bit_depth)
        seen, plane_of = {}, []
        for (cu, _) in candidates:
            plane_of.append(seen.get(cu, 0))
            seen[cu] = plane_of[-1] + 1
        planes = max(plane_of, default=-1) + 1
        rec = torch.zeros((max(planes, 1), resi.numel()), dtype=torch.int16, device=self.device)
        sse = torch.zeros((len(candidates), 3), dtype=torch.int64, device=self.device)
        for r in range(planes):
            ks = [k for k in range(len(candidates)) if plane_of[k] == r]
            part = torch.empty((len(ks), 3), dtype=torch.int64, device=self.device)
            self.sbt_place_batch(tile_rec, place[ks], stats, rec[r], resi, part)
            sse[torch.as_tensor(ks, device=self.device)] = part
        return parts, est, order, rec, sse, level, stats

    # ---- motion-search plans: integer candidates + sub-pel stages + plain table calls of a picture in one launch ----
    def me_plan_create(self, int_jobs, cands, stage_jobs, items, bit_depth=10, max_window=0, mask_items=None):
        """numpy record arrays (vvenc_amd/replay.py dtypes mirror vvhip_me_int_job / _cand / _stage_job / _item / _mask_item) -> plan handle"""
        keep = [np.ascontiguousarray(a) for a in (int_jobs, cands, stage_jobs, items)]
        plan = C.c_void_p()
        if mask_items is None or not mask_items.size:
            self._ck(self.L.vvhip_me_plan_create(self.ctx, keep[0].ctypes.data if keep[0].size else None, int(keep[0].size), keep[1].ctypes.data if keep[1].size else None, int(keep[1].size),
                                                 keep[2].ctypes.data if keep[2].size else None, int(keep[2].size), keep[3].ctypes.data if keep[3].size else None, int(keep[3].size),
                                                 bit_depth, max_window, C.byref(plan)))
            return plan
        keep.append(np.ascontiguousarray(mask_items))

        class Lists(C.Structure):          # vvhip_me_lists
            _fields_ = [(n, t) for k in range(5) for n, t in (("p%d" % k, C.c_void_p), ("n%d" % k, C.c_int32))]
        L = Lists()
        for k, a in enumerate(keep):
            setattr(L, "p%d" % k, a.ctypes.data if a.size else None)
            setattr(L, "n%d" % k, int(a.size))
        self._ck(self.L.vvhip_me_plan_create_lists(self.ctx, C.cast(C.pointer(L), C.c_void_p), bit_depth, max_window, C.byref(plan)))
        return plan

    def me_plan_destroy(self, plan):
        self.L.vvhip_me_plan_destroy(self.ctx, plan)

    def me_plan_info(self, plan):
        v = [C.c_int() for _ in range(4)]
        self._ck(self.L.vvhip_me_plan_info(plan, *[C.cast(C.pointer(x), C.c_void_p) for x in v]))
        return {"waves_int": v[0].value, "waves_stage": v[1].value, "waves_item": v[2].value, "lds_bytes": v[3].value}

    def me_plan_set_timing(self, plan, on=True):
        self._ck(self.L.vvhip_me_plan_set_timing(self.ctx, plan, 1 if on else 0))

    def me_plan_last_times(self, plan):
        """ms of the last run's parts: refinement stages, integer windows (one launch for both LDS classes), 0, table calls"""
        ms = (C.c_float * 4)()
        self._ck(self.L.vvhip_me_plan_last_times(self.ctx, plan, C.cast(ms, C.c_void_p)))
        return [float(x) for x in ms]

    def me_plan_run(self, plan, plane_table, n_planes, cand_cost, stage_cost, item_cost):
        self._ck(self.L.vvhip_me_plan_run(self.ctx, plan, C.cast(plane_table, C.c_void_p), n_planes, _ptr(cand_cost), _ptr(stage_cost), _ptr(item_cost)))

    def me_plan_run_parts(self, plan, plane_table, n_planes, cand_cost, stage_cost, item_cost, parts):
        """parts: bit 0 refinement stages, bit 1 integer windows, bit 2 table calls — only the cost arrays of the parts that run are written"""
        self._ck(self.L.vvhip_me_plan_run_parts(self.ctx, plan, C.cast(plane_table, C.c_void_p), n_planes, _ptr(cand_cost), _ptr(stage_cost), _ptr(item_cost), int(parts)))

    # ---- DMVR refinement search ----
    def dmvr_refine_batch(self, ref0, ref1, d_items, n, dx, dy, bit_depth=10, out=None):
        """d_items: DMVR_ITEM_DTYPE records -> tensor of DMVR_RESULT_DTYPE records (as uint8 rows)"""
        if out is None:
            out = torch.empty((n, DMVR_RESULT_DTYPE.itemsize), dtype=torch.uint8, device=self.device)
        self._ck(self.L.vvhip_dmvr_refine_batch(self.ctx, ref0.buf_ptr, ref0.stride, ref1.buf_ptr, ref1.stride, _ptr(d_items), n, dx, dy, bit_depth, _ptr(out)))
        return out

    # ---- ALF encoder statistics ----
    ALF_REC = 183

    def alf_classify(self, rec, bit_depth=10, vb_ctu_height=128, vb_pos=124, out=None):
        """rec: luma Plane with a replicated margin >= 4 -> uint8 tensor (H/4, W/4, 2) {classIdx, transposeIdx}"""
        if out is None:
            out = torch.empty((rec.height // 4, rec.width // 4, 2), dtype=torch.uint8, device=self.device)
        self._ck(self.L.vvhip_alf_classify(self.ctx, rec.buf_ptr, rec.stride, rec.width, rec.height, bit_depth, vb_ctu_height, vb_pos, _ptr(out)))
        return out

    def alf_stats_plane(self, org, rec, ctu_size, filter_length, d_cls=None, vb_ctu_height=128, vb_pos=124, out=None, init=None, ctu_in_unit=None):
        """covariance records of every CTU of a plane -> float32 tensor (numCtus, 25 or 1, ALF_REC): E[13][13], y[13], pixAcc"""
        nctu = ((rec.width + ctu_size - 1) // ctu_size) * ((rec.height + ctu_size - 1) // ctu_size)
        ncls = 25 if d_cls is not None else 1
        if out is None:
            out = torch.empty((nctu, ncls, self.ALF_REC), dtype=torch.float32, device=self.device)
        self._ck(self.L.vvhip_alf_stats_plane_units(self.ctx, org.buf_ptr, org.stride, rec.buf_ptr, rec.stride, rec.width, rec.height, ctu_size, ctu_in_unit or ctu_size, filter_length,
                                              _ptr(d_cls) if d_cls is not None else None, vb_ctu_height, vb_pos, _ptr(init) if init is not None else None, _ptr(out)))
        return out

    def ccalf_stats_plane(self, org_c, slf_c, rec_luma, ctu_size_c, vb_ctu_height=128, vb_pos=124, shift=(1, 1), out=None, init=None):
        """CC-ALF covariance records of every chroma CTU -> float32 tensor (numCtus, ALF_REC); org_c / slf_c chroma Planes, rec_luma with margin >= 2"""
        nctu = ((slf_c.width + ctu_size_c - 1) // ctu_size_c) * ((slf_c.height + ctu_size_c - 1) // ctu_size_c)
        if out is None:
            out = torch.empty((nctu, self.ALF_REC), dtype=torch.float32, device=self.device)
        self._ck(self.L.vvhip_ccalf_stats_plane(self.ctx, org_c.buf_ptr, org_c.stride, slf_c.buf_ptr, slf_c.stride, rec_luma.buf_ptr, rec_luma.stride, slf_c.width, slf_c.height,
                                                ctu_size_c, shift[0], shift[1], vb_ctu_height, vb_pos, rec_luma.height, _ptr(init) if init is not None else None, _ptr(out)))
        return out

    def alf_filter_plane(self, src, dst, ctu_size, bit_depth, filter_length, d_coeff, d_clip, d_ctu_set, d_cls=None, vb_ctu_height=128, vb_pos=124):
        """filterBlk over the enabled CTUs: src Plane (replicated margin >= 4) -> dst Plane (CTUs with d_ctu_set < 0 keep their samples).
        d_coeff / d_clip: int16 (numSets, 25 or 1, 13); d_clip None = linear filters; d_ctu_set: int16 per CTU"""
        self._ck(self.L.vvhip_alf_filter_plane(self.ctx, src.buf_ptr, src.stride, dst.buf_ptr, dst.stride, src.width, src.height, ctu_size, bit_depth, filter_length,
                                               _ptr(d_cls) if d_cls is not None else None, _ptr(d_coeff), _ptr(d_clip) if d_clip is not None else None, _ptr(d_ctu_set), vb_ctu_height, vb_pos))
        return dst

    def ccalf_filter_plane(self, dst_c, rec_luma, ctu_size_c, bit_depth, d_coeff, d_ctu_filter, vb_ctu_height=128, vb_pos=124, shift=(1, 1)):
        """filterBlkCcAlf: corrects the chroma Plane dst_c in place from rec_luma (margin >= 2).  d_coeff: int16 (numFilters, 8); d_ctu_filter: uint8 per CTU (0 = off)"""
        self._ck(self.L.vvhip_ccalf_filter_plane(self.ctx, dst_c.buf_ptr, dst_c.stride, rec_luma.buf_ptr, rec_luma.stride, dst_c.width, dst_c.height, ctu_size_c, shift[0], shift[1], bit_depth,
                                                 _ptr(d_coeff), _ptr(d_ctu_filter), vb_ctu_height, vb_pos))
        return dst_c

    # ---- SAO: statistics and offset filtering of a picture (sao.hip) ----
    class _SaoStatsPlane(C.Structure):
        _fields_ = [("d_org", C.c_void_p), ("d_src", C.c_void_p), ("org_stride", C.c_int32), ("src_stride", C.c_int32), ("width", C.c_int32), ("height", C.c_int32),
                    ("ctu_w", C.c_int32), ("ctu_h", C.c_int32), ("bit_depth", C.c_int32), ("is_luma", C.c_int32)]

    class _SaoOffsetPlane(C.Structure):
        _fields_ = [("d_src", C.c_void_p), ("d_dst", C.c_void_p), ("src_stride", C.c_int32), ("dst_stride", C.c_int32), ("width", C.c_int32), ("height", C.c_int32),
                    ("ctu_w", C.c_int32), ("ctu_h", C.c_int32), ("bit_depth", C.c_int32), ("clip_min", C.c_int32), ("clip_max", C.c_int32), ("rsv", C.c_int32)]

    @staticmethod
    def sao_geometry(planes, ctu):
        """planes: per plane a pair of Plane / PlaneView, plane 0 first; ctu: the CTU size of plane 0, or per plane ( ctu_w, ctu_h ) -> per plane ( ctu_w, ctu_h ) and the
        CTU grid of plane 0 ( a subsampled plane — smaller than plane 0 in a direction — has half the CTU size there: 4:2:0 / 4:2:2 )"""
        p0 = planes[0][0]
        if isinstance(ctu, int):
            ctu = [(ctu if p[0].width == p0.width else ctu // 2, ctu if p[0].height == p0.height else ctu // 2) for p in planes]
        return ctu, (-(-p0.width // ctu[0][0]), -(-p0.height // ctu[0][1]))

    def sao_stats(self, planes, ctu, bit_depth, rows=None, flags=None, out=None):
        """getBlkStats of every CTU of CTU rows `rows` = ( first, count ) (None: the picture) in one launch.  planes: per plane ( org, src ), Plane or PlaneView, plane 0 = luma.
        flags: uint8 per CTU of the picture (SAO_* bits) or None = picture borders alone.  -> int64 tensor ( ctus of the picture, planes, 5, 2, 32 ); only the band is written"""
        ctu, (gx, gy) = self.sao_geometry(planes, ctu)
        rows = (0, gy) if rows is None else rows
        if out is None:
            out = torch.zeros((gx * gy, len(planes), 5, 2, 32), dtype=torch.int64, device=self.device)
        desc = (self._SaoStatsPlane * len(planes))(*[self._SaoStatsPlane(o.buf_ptr, s.buf_ptr, o.stride, s.stride, s.width, s.height, cw, ch, bit_depth, int(k == 0))
                                                     for k, ((o, s), (cw, ch)) in enumerate(zip(planes, ctu))])
        fl = None
        if flags is not None:
            fl = np.ascontiguousarray(flags, np.uint8).reshape(-1)
            assert fl.size == gx * gy, "one flag byte per CTU of the picture"
        self._ck(self.L.vvhip_sao_stats(self.ctx, desc, len(planes), rows[0], rows[1], fl.ctypes.data_as(C.c_void_p) if fl is not None else None, _ptr(out)))
        return out

    def sao_offset(self, planes, params, ctu, bit_depth, rows=None, clip=None):
        """offsetBlock of every CTU of CTU rows `rows` in one launch.  planes: per plane ( src, dst ); params: SAO_PARAM_DTYPE ( ctus of the picture, planes ); clip: per plane
        ( min, max ), None = ( 0, 2^bit_depth - 1 ).  dst receives the band's complete rows (filtered samples, the source value everywhere else)"""
        ctu, (gx, gy) = self.sao_geometry(planes, ctu)
        rows = (0, gy) if rows is None else rows
        clip = [(0, (1 << bit_depth) - 1)] * len(planes) if clip is None else clip
        prm = np.ascontiguousarray(params, SAO_PARAM_DTYPE).reshape(-1)
        assert prm.size == gx * gy * len(planes), "one parameter record per CTU of the picture and plane"
        desc = (self._SaoOffsetPlane * len(planes))(*[self._SaoOffsetPlane(s.buf_ptr, d.buf_ptr, s.stride, d.stride, s.width, s.height, cw, ch, bit_depth, lo, hi, 0)
                                                      for (s, d), (cw, ch), (lo, hi) in zip(planes, ctu, clip)])
        self._ck(self.L.vvhip_sao_offset(self.ctx, desc, len(planes), prm.ctypes.data_as(C.c_void_p), rows[0], rows[1]))
        return [d for (_, d) in planes]

    # ---- LF: the deblocking filter of a picture (deblock.hip) ----
    class _DeblockPlane(C.Structure):
        _fields_ = [("d_plane", C.c_void_p), ("stride", C.c_int32), ("width", C.c_int32), ("height", C.c_int32), ("clip_min", C.c_int32), ("clip_max", C.c_int32),
                    ("beta_offset_div2", C.c_int32), ("tc_offset_div2", C.c_int32)]

    def deblock(self, planes, lfp_ver, lfp_hor, ctu_size, bit_depth, rows=None, dirs=3, clip=None, beta_offsets=(0, 0, 0), tc_offsets=(0, 0, 0)):
        """xDeblockArea<EDGE_VER> then <EDGE_HOR> over the CTUs of CTU rows `rows` = ( first, count ) (None: the picture), in place.  planes: [ luma ] or [ luma, cb, cr ]
        (4:2:0), Plane or PlaneView; lfp_ver / lfp_hor: LF_PARAM_DTYPE [ units down ][ units across ], one record per 4 x 4 luma unit (a map of a direction not in `dirs`
        may be None); clip: per plane ( min, max ), None = ( 0, 2^bit_depth - 1 ); the offsets are the slice's per component.  The band contract: vvenc_hip.h"""
        gy = -(-planes[0].height // ctu_size)
        rows = (0, gy) if rows is None else rows
        clip = [(0, (1 << bit_depth) - 1)] * len(planes) if clip is None else clip
        maps, stride = [], 0
        for m in (lfp_ver, lfp_hor):
            if m is not None:
                m = np.ascontiguousarray(m, LF_PARAM_DTYPE)
                assert m.ndim == 2 and (stride in (0, m.shape[1])), "the maps are 2-D and have one line pitch"
                stride = m.shape[1]
            maps.append(m)
        desc = (self._DeblockPlane * len(planes))(*[self._DeblockPlane(p.buf_ptr, p.stride, p.width, p.height, lo, hi, bo, to)
                                                    for p, (lo, hi), bo, to in zip(planes, clip, beta_offsets, tc_offsets)])
        self._ck(self.L.vvhip_deblock(self.ctx, desc, len(planes), bit_depth, ctu_size, *[m.ctypes.data_as(C.c_void_p) if m is not None else None for m in maps], stride,
                                      rows[0], rows[1], dirs))
        return planes

    # ---- QPA: the visual activity of the original picture (visact.hip) ----
    class _VisActPlane(C.Structure):
        _fields_ = [("d_cur", C.c_void_p), ("d_prev1", C.c_void_p), ("d_prev2", C.c_void_p), ("cur_stride", C.c_int32), ("prev1_stride", C.c_int32), ("prev2_stride", C.c_int32),
                    ("width", C.c_int32), ("height", C.c_int32), ("bit_depth", C.c_int32)]

    def visact(self, planes, areas, out=None):
        """the high-pass sums of calcSpatialVisAct / calcTemporalVisAct and getAvg's sample sum for a list of areas in one call.  planes: up to three table rows
        ( cur, prev1, prev2, bit_depth ), Plane or PlaneView, prev1 / prev2 may be None; areas: VISACT_AREA_DTYPE [ n ].  -> int64 tensor ( n, 4 ) holding the uint64 records
        [ spatial sum, temporal sum, sample sum of the mean rectangle, positions ] (vvenc_hip.h); with out given, only its first n rows are written"""
        ar = np.ascontiguousarray(areas, VISACT_AREA_DTYPE).reshape(-1)
        if out is None:
            out = torch.zeros((ar.size, 4), dtype=torch.int64, device=self.device)
        assert out.dtype == torch.int64 and out.numel() >= 4 * ar.size
        desc = (self._VisActPlane * len(planes))(*[self._VisActPlane(c.buf_ptr, p1.buf_ptr if p1 is not None else None, p2.buf_ptr if p2 is not None else None, c.stride,
                                                                     p1.stride if p1 is not None else 0, p2.stride if p2 is not None else 0, c.width, c.height, bd)
                                                   for (c, p1, p2, bd) in planes])
        self._ck(self.L.vvhip_visact(self.ctx, desc, len(planes), ar.ctypes.data_as(C.c_void_p), ar.size, _ptr(out)))
        return out

    @staticmethod
    def visact_picture_areas(sizes, ctu, high_res, order, chroma="420"):
        """the reference's own area list of a picture (BitAllocation.cpp:553-573, :610-616).  sizes: ( width, height ) per component -> VISACT_AREA_DTYPE: per CTU of plane 0,
        in raster order, the CTU with its guard frame of 1 (2 with high_res) samples, clipped to the picture, with the clipped CTU as the mean rectangle; then one whole-plane
        area per component (the plane is its own mean rectangle).  high_res selects the down-sampling form — for the chroma planes only with chroma == "444" """
        W, H = sizes[0]
        guard, out = (2 if high_res else 1), []
        for y in range(0, H, ctu):
            for x in range(0, W, ctu):
                fx, fy = (x - guard if x > 0 else 0), (y - guard if y > 0 else 0)
                fw, fh = ctu + guard * (2 if x > 0 else 1), ctu + guard * (2 if y > 0 else 1)
                out.append((0, int(high_res), order, 0, fx, fy, min(fw, W - fx), min(fh, H - fy), x, y, min(ctu, W - x), min(ctu, H - y), 0))
        for c, (w, h) in enumerate(sizes):
            out.append((c, int(bool(high_res) and (c == 0 or chroma == "444")), order, 0, 0, 0, w, h, 0, 0, w, h, 0))
        return np.array(out, VISACT_AREA_DTYPE)

    def visact_picture(self, cur, prev1, prev2, ctu, bit_depth, high_res, order, chroma="420", out=None):
        """vvhip_visact over the area list of visact_picture_areas.  cur / prev1 / prev2: per component a Plane or PlaneView ([ luma ] or [ luma, cb, cr ]); prev1 / prev2 may be
        None (order 0 / 1).  -> ( records ( n, 4 ), areas ): the CTUs' records first, then one per component"""
        n = len(cur)
        prev1, prev2 = prev1 if prev1 is not None else [None] * n, prev2 if prev2 is not None else [None] * n
        areas = self.visact_picture_areas([(p.width, p.height) for p in cur], ctu, high_res, order, chroma)
        return self.visact([(cur[c], prev1[c], prev2[c], bit_depth) for c in range(n)], areas, out), areas

    # ---- intra luma mode pre-selection (intra.hip) ----
    @staticmethod
    def intra_layout(items):
        """a copy of the items with cost_off = 67 * i and the predictions packed in list order -> ( items, prediction samples in all )"""
        it = np.ascontiguousarray(items, INTRA_ITEM_DTYPE).reshape(-1).copy()
        at = 0
        for i in range(it.size):
            it[i]["cost_off"], it[i]["pred_off"] = INTRA_MODES * i, at
            at += sum(bin(int(m)).count("1") for m in it[i]["pred_mask"]) * int(it[i]["w"]) * int(it[i]["h"])
        return it, at

    def intra_luma_modes(self, items, ref, org, cost=None, pred=None):
        """vvhip_intra_luma_modes_batch: every mode of mode_mask of every item predicted from the item's reference lines and scored with HAD_2SAD against its original; the
        predictions of pred_mask written.  items: INTRA_ITEM_DTYPE [ n ]; ref / org: int16 device tensors (the lines, the compact originals).
        Without cost / pred the items are laid out by intra_layout and fresh zeroed tensors are returned; with cost ( int32, the uint32 costs ) and pred ( int16, or None where no
        item asks for predictions ) given, the items' own cost_off / pred_off are used and nothing but the requested slots and blocks is written.
        -> ( cost viewed as ( -1, 67 ) where it was made here, pred, the items as run )"""
        it = np.ascontiguousarray(items, INTRA_ITEM_DTYPE).reshape(-1)
        if cost is None:
            it, npred = self.intra_layout(it)
            cost = torch.zeros((it.size, INTRA_MODES), dtype=torch.int32, device=self.device)
            pred = torch.zeros(npred, dtype=torch.int16, device=self.device) if npred else None
        assert cost.dtype == torch.int32 and ref.dtype == torch.int16 and org.dtype == torch.int16 and (pred is None or pred.dtype == torch.int16)
        self._ck(self.L.vvhip_intra_luma_modes_batch(self.ctx, it.ctypes.data_as(C.c_void_p), it.size, _ptr(ref), _ptr(org), _ptr(pred), _ptr(cost)))
        return cost, pred, it

    # ---- intra chroma mode pre-selection (intrachroma.hip) ----
    @staticmethod
    def intra_chroma_layout(items):
        """a copy of the items with cost_off = 8 * i and the predictions packed in list order, Cb before Cr per item -> ( items, prediction samples in all )"""
        it = np.ascontiguousarray(items, INTRA_CHROMA_ITEM_DTYPE).reshape(-1).copy()
        at = 0
        for i in range(it.size):
            n = bin(int(it[i]["pred_mask"])).count("1") * int(it[i]["w"]) * int(it[i]["h"])
            it[i]["cost_off"], it[i]["pred_off"] = INTRA_CHROMA_SLOTS * i, (at, at + n)
            at += 2 * n
        return it, at

    def intra_chroma_modes(self, items, luma, ref, org, cost=None, pred=None):
        """vvhip_intra_chroma_modes_batch: the Cb and the Cr prediction of every slot of mode_mask of every item — regular modes from the components' reference lines, modes
        67..69 from the reconstructed luma plane — scored with min( 2 SAD, HAD ) per component and added; the predictions of pred_mask written.  items:
        INTRA_CHROMA_ITEM_DTYPE [ n ]; luma / ref / org: int16 device tensors (luma may be None when no item asks for a mode >= 67).
        Without cost / pred the items are laid out by intra_chroma_layout and fresh zeroed tensors are returned; with cost ( int32, the uint32 costs ) and pred ( int16, or None
        where no item asks for predictions ) given, the items' own cost_off / pred_off are used and nothing but the requested slots and blocks is written.
        -> ( cost viewed as ( -1, 8 ) where it was made here, pred, the items as run )"""
        it = np.ascontiguousarray(items, INTRA_CHROMA_ITEM_DTYPE).reshape(-1)
        if cost is None:
            it, npred = self.intra_chroma_layout(it)
            cost = torch.zeros((it.size, INTRA_CHROMA_SLOTS), dtype=torch.int32, device=self.device)
            pred = torch.zeros(npred, dtype=torch.int16, device=self.device) if npred else None
        assert cost.dtype == torch.int32 and ref.dtype == torch.int16 and org.dtype == torch.int16 and (pred is None or pred.dtype == torch.int16) and (luma is None or luma.dtype == torch.int16)
        self._ck(self.L.vvhip_intra_chroma_modes_batch(self.ctx, it.ctypes.data_as(C.c_void_p), it.size, _ptr(luma), _ptr(ref), _ptr(org), _ptr(pred), _ptr(cost)))
        return cost, pred, it

    # ---- MMVD merge candidates (mmvd.hip) ----
    def merge_mmvd_costs(self, planes, items, org, pic_w, pic_h, ctu, bit_depth=10, func="HAD", dis_frac=False, cost=None):
        """vvhip_merge_mmvd_costs_batch: the Hadamard cost of every candidate of cand_mask of every CU of the list — base vector plus MMVD delta, the clips, the luma
        prediction (one list, the default average or BCW) and HAD / HAD_fast against the original, in one launch.  planes: the reference Planes the items' ref_plane
        indexes; items: MMVD_ITEM_DTYPE [ n ] (HOST array); org: the Plane of the original.  Without cost the items get cost_off = 64 * i and a fresh zeroed tensor is
        returned; with cost ( int32, the uint32 costs ) the items' own cost_off is used and nothing but the requested slots is written.
        -> ( cost viewed as ( -1, 64 ) where it was made here, the items as run )"""
        it = np.ascontiguousarray(items, MMVD_ITEM_DTYPE).reshape(-1)
        if cost is None:
            it = it.copy()
            it["cost_off"] = MMVD_SLOTS * np.arange(it.size)
            cost = torch.zeros((it.size, MMVD_SLOTS), dtype=torch.int32, device=self.device)
        assert cost.dtype == torch.int32
        tab = (self._MePlane * max(1, len(planes)))(*[self._MePlane(p.buf_ptr.value, p.stride, 0) for p in planes])
        self._ck(self.L.vvhip_merge_mmvd_costs_batch(self.ctx, C.cast(tab, C.c_void_p), len(planes), it.ctypes.data_as(C.c_void_p) if it.size else None, int(it.size),
                                                     int(pic_w), int(pic_h), int(ctu), bit_depth, DF[func] if isinstance(func, str) else func, int(dis_frac),
                                                     org.buf_ptr if org is not None else None, org.stride if org is not None else 0, _ptr(cost)))
        return cost, it

    def mmvd_candidate(self, item, val, pic_w, pic_h, ctu, dis_frac=False):
        """vvhip_mmvd_candidate (host only): candidate val of one MMVD_ITEM_DTYPE record -> a MMVD_CAND_DTYPE record"""
        it = np.ascontiguousarray(item, MMVD_ITEM_DTYPE).reshape(-1)[:1].copy()
        out = np.zeros(1, MMVD_CAND_DTYPE)
        if self.L.vvhip_mmvd_candidate(it.ctypes.data_as(C.c_void_p), int(val), int(pic_w), int(pic_h), int(ctu), int(dis_frac), out.ctypes.data_as(C.c_void_p)) != 0:
            raise ValueError("mmvd_candidate: candidate %d of a %dx%d item" % (val, int(it[0]["w"]), int(it[0]["h"])))
        return out[0]

    # ---- MCTF apply side ----
    REF_STRENGTHS = ((0.84375, 0.6, 0.4286, 0.3333, 0.2727, 0.2308), (1.12500, 1.0, 0.7143, 0.5556, 0.4545, 0.3846))      # MCTF.cpp:112-117

    def mctf_filter_params(self, qp, bit_depth, overall_strength, chroma):
        s, w = C.c_double(), C.c_double()
        self._ck(self.L.vvhip_mctf_filter_params(qp, bit_depth, overall_strength, int(chroma), C.byref(s), C.byref(w)))
        return s.value, w.value

    def mctf_apply_plane(self, org, refs, d_mvs, mv_w, chroma_shift, ref_strengths, weight_scaling, sigma_sq, bit_depth=10, unit=16, low_res=True, qp=32, out=None):
        """bilateral temporal filter of one plane: org / refs are Planes (same stride), d_mvs a list of device motion fields (MV_DTYPE records)"""
        if out is None:
            out = Plane(self.device, org.width, org.height, 0)
        assert all(r.stride == refs[0].stride for r in refs)
        rp = (C.c_void_p * len(refs))(*[r.buf_ptr.value for r in refs])
        mp = (C.c_void_p * len(refs))(*[m.data_ptr() for m in d_mvs])
        rs = (C.c_double * len(refs))(*[float(x) for x in ref_strengths])
        self._ck(self.L.vvhip_mctf_apply_plane(self.ctx, org.buf_ptr, org.stride, org.width, org.height, chroma_shift, bit_depth, unit, int(low_res), qp, len(refs),
                                               rp, refs[0].stride, mp, mv_w, rs, weight_scaling, sigma_sq, out.buf_ptr, out.stride))
        return out

    def mctf_bilateral(self, org_yuv, refs_yuv, mvs_np, ref_index, bit_depth=10, qp=32, unit=16, low_res=True, pic_reordering=True, overall_strength=0.95):
        """MCTF::bilateralFilter on 4:2:0 numpy planes (uploads with the reference's margins); returns numpy (Y, U, V)"""
        h, w = org_yuv[0].shape
        mv_w = (w + unit - 1) // unit
        d_mvs = [self.to_device(np.ascontiguousarray(m)) for m in mvs_np]
        strengths = [self.REF_STRENGTHS[0 if pic_reordering else 1][k] for k in ref_index]
        outs = []
        for c in range(3):
            cs = 1 if c else 0
            po = self.plane(org_yuv[c], 128 >> cs)
            prs = [self.plane(r[c], 128 >> cs) for r in refs_yuv]
            sigma, scaling = self.mctf_filter_params(qp, bit_depth, overall_strength, c > 0)
            o = self.mctf_apply_plane(po, prs, d_mvs, mv_w, cs, strengths, scaling, sigma, bit_depth, unit, low_res, qp)
            outs.append(o.visible().cpu().numpy())
        return tuple(outs)

    # ---- sub-pel interpolation ----
    def if_filter(self, taps, vertical, first, last, bit_depth, d_src, src_off, src_stride, d_dst, dst_off, dst_stride, w, h, coeff):
        """one pass on one block with the caller's taps (InterpolationFilter::m_filterHor / m_filterVer slot)"""
        c = np.ascontiguousarray(coeff, np.int16)
        self._ck(self.L.vvhip_if_filter(self.ctx, taps, int(vertical), int(first), int(last), bit_depth, C.c_void_p(d_src.data_ptr() + 2 * src_off), src_stride,
                                        C.c_void_p(d_dst.data_ptr() + 2 * dst_off), dst_stride, w, h, c.ctypes.data_as(C.c_void_p)))

    def if_copy(self, first, last, bit_depth, d_src, src_off, src_stride, d_dst, dst_off, dst_stride, w, h, bi_mc=False):
        self._ck(self.L.vvhip_if_copy(self.ctx, int(first), int(last), bit_depth, C.c_void_p(d_src.data_ptr() + 2 * src_off), src_stride,
                                      C.c_void_p(d_dst.data_ptr() + 2 * dst_off), dst_stride, w, h, int(bi_mc)))

    def interp_luma_batch(self, ref, d_items, n, w, h, bit_depth=10, rnd_res=True, filter_mode=0, use_alt_hpel=False, out=None):
        """motion-compensated luma prediction blocks at 1/16-sample vectors (d_items: SUBPEL_DTYPE records) -> (n, h, w) int16"""
        if out is None:
            out = torch.empty(n * w * h, dtype=torch.int16, device=self.device)
        self._ck(self.L.vvhip_interp_luma_batch(self.ctx, ref.buf_ptr, ref.stride, _ptr(d_items), n, w, h, bit_depth, int(rnd_res), filter_mode,
                                                int(use_alt_hpel), _ptr(out)))
        return out

    def interp_chroma_batch(self, ref, d_items, n, w, h, bit_depth=10, rnd_res=True, out=None):
        """4:2:0 chroma prediction blocks of one size at 1/32-sample vectors (d_items: SUBPEL_DTYPE records) -> (n, h, w) int16; rnd_res False: the 14-bit intermediate"""
        if out is None:
            out = torch.empty(n * w * h, dtype=torch.int16, device=self.device)
        self._ck(self.L.vvhip_interp_chroma_batch(self.ctx, ref.buf_ptr, ref.stride, _ptr(d_items), n, w, h, bit_depth, int(rnd_res), _ptr(out)))
        return out

    class _MePlane(C.Structure):          # vvhip_me_plane
        _fields_ = [("d_base", C.c_void_p), ("stride", C.c_int32), ("reserved", C.c_int32)]

    def pred_inter_batch(self, planes, items, pred, pred_stride=0, bit_depth=10, org=None, resi=None, ext=None, blend=None, ciip=None, intra_ref=None):
        """inter prediction of a list of prediction units in one launch: planes = the reference Planes the items' ref_plane indexes, items = PRED_ITEM_DTYPE records
        (HOST array: the library sorts it into size classes), pred = int16 tensor (compact blocks at dst_off, or a plane of row pitch pred_stride).
        org (a Plane) + resi (int16 tensor laid out like pred): also writes org - pred.
        ext = PRED_EXT_DTYPE records parallel to items (BDOF, DMVR's padded reference): vvhip_pred_inter_batch_ex.
        blend = PRED_BLEND_DTYPE records parallel to items (BCW weights, GEO partitions): vvhip_pred_inter_batch_blend, with ext or without.
        ciip = PRED_CIIP_DTYPE records parallel to items (planar intra part and weighting of CIIP CUs) + intra_ref = int16 DEVICE tensor of the reference-sample lines
        they point into: vvhip_pred_inter_batch_ciip, with ext / blend or without."""
        it = np.ascontiguousarray(items, PRED_ITEM_DTYPE)
        tab = (self._MePlane * max(1, len(planes)))(*[self._MePlane(p.buf_ptr.value, p.stride, 0) for p in planes])
        if ciip is not None:
            ci = np.ascontiguousarray(ciip, PRED_CIIP_DTYPE)
            ex = np.ascontiguousarray(ext, PRED_EXT_DTYPE) if ext is not None else None
            bl = np.ascontiguousarray(blend, PRED_BLEND_DTYPE) if blend is not None else None
            if ci.size != it.size or (ex is not None and ex.size != it.size) or (bl is not None and bl.size != it.size):
                raise ValueError("pred_inter_batch: %d CIIP records, %s extensions, %s blend records for %d items"
                                 % (ci.size, "no" if ex is None else ex.size, "no" if bl is None else bl.size, it.size))
            self._ck(self.L.vvhip_pred_inter_batch_ciip(self.ctx, C.cast(tab, C.c_void_p), len(planes), it.ctypes.data_as(C.c_void_p) if it.size else None,
                                                        ex.ctypes.data_as(C.c_void_p) if ex is not None and ex.size else None,
                                                        bl.ctypes.data_as(C.c_void_p) if bl is not None and bl.size else None,
                                                        ci.ctypes.data_as(C.c_void_p) if ci.size else None, _ptr(intra_ref), int(it.size), bit_depth, _ptr(pred), pred_stride,
                                                        org.buf_ptr if org is not None else None, org.stride if org is not None else 0, _ptr(resi)))
            return pred
        if blend is not None:
            bl = np.ascontiguousarray(blend, PRED_BLEND_DTYPE)
            ex = np.ascontiguousarray(ext, PRED_EXT_DTYPE) if ext is not None else None
            if bl.size != it.size or (ex is not None and ex.size != it.size):
                raise ValueError("pred_inter_batch: %d blend records, %s extensions for %d items" % (bl.size, "no" if ex is None else ex.size, it.size))
            self._ck(self.L.vvhip_pred_inter_batch_blend(self.ctx, C.cast(tab, C.c_void_p), len(planes), it.ctypes.data_as(C.c_void_p) if it.size else None,
                                                         ex.ctypes.data_as(C.c_void_p) if ex is not None and ex.size else None,
                                                         bl.ctypes.data_as(C.c_void_p) if bl.size else None, int(it.size), bit_depth, _ptr(pred), pred_stride,
                                                         org.buf_ptr if org is not None else None, org.stride if org is not None else 0, _ptr(resi)))
            return pred
        if ext is not None:
            ex = np.ascontiguousarray(ext, PRED_EXT_DTYPE)
            if ex.size != it.size:
                raise ValueError("pred_inter_batch: %d extensions for %d items" % (ex.size, it.size))
            self._ck(self.L.vvhip_pred_inter_batch_ex(self.ctx, C.cast(tab, C.c_void_p), len(planes), it.ctypes.data_as(C.c_void_p) if it.size else None,
                                                      ex.ctypes.data_as(C.c_void_p) if ex.size else None, int(it.size), bit_depth, _ptr(pred), pred_stride,
                                                      org.buf_ptr if org is not None else None, org.stride if org is not None else 0, _ptr(resi)))
            return pred
        self._ck(self.L.vvhip_pred_inter_batch(self.ctx, C.cast(tab, C.c_void_p), len(planes), it.ctypes.data_as(C.c_void_p) if it.size else None, int(it.size), bit_depth,
                                               _ptr(pred), pred_stride, org.buf_ptr if org is not None else None, org.stride if org is not None else 0, _ptr(resi)))
        return pred

    def geo_weights(self, split_dir, cu_w, cu_h, chroma=0):
        """the GEO weights w0 (0..8) of one component block of a cu_w x cu_h CU as the blend entry applies them (vvhip_get_geo_weights_host; host only) -> int8 [h, w]"""
        w, h = cu_w >> chroma, cu_h >> chroma
        out = np.zeros((h, w), np.int8)
        if self.L.vvhip_get_geo_weights_host(int(split_dir), int(cu_w).bit_length() - 1, int(cu_h).bit_length() - 1, int(chroma), out.ctypes.data_as(C.c_void_p)) != 0:
            raise ValueError("geo_weights: split_dir %d (0..63), CU %dx%d (8..64), chroma %d" % (split_dir, cu_w, cu_h, chroma))
        return out

    def pred_affine_batch(self, planes, items, pred, pred_stride, bit_depth, pic_w, pic_h, ctu, org=None, resi=None):
        """inter prediction of a list of affine CUs from their control-point vectors in one launch (vvhip_pred_affine_batch): items = PRED_AFFINE_ITEM_DTYPE records, one
        per component block (HOST array); planes, pred, pred_stride, org, resi as pred_inter_batch; pic_w / pic_h / ctu = the luma picture and CTU size of the picture clip."""
        it = np.ascontiguousarray(items, PRED_AFFINE_ITEM_DTYPE)
        tab = (self._MePlane * max(1, len(planes)))(*[self._MePlane(p.buf_ptr.value, p.stride, 0) for p in planes])
        self._ck(self.L.vvhip_pred_affine_batch(self.ctx, C.cast(tab, C.c_void_p), len(planes), it.ctypes.data_as(C.c_void_p) if it.size else None, int(it.size),
                                                int(pic_w), int(pic_h), int(ctu), bit_depth, _ptr(pred), pred_stride,
                                                org.buf_ptr if org is not None else None, org.stride if org is not None else 0, _ptr(resi)))
        return pred

    def subpel_dist_batch(self, func, org, ref, d_items, n, w, h, bit_depth=10, filter_mode=0, use_alt_hpel=False, out=None):
        """distortion of sub-pel candidates: interpolate at the fractional vector, score against the original block"""
        if out is None:
            out = torch.empty(n, dtype=torch.int64, device=self.device)
        self._ck(self.L.vvhip_subpel_dist_batch(self.ctx, DF[func] if isinstance(func, str) else func, org.buf_ptr, org.stride, ref.buf_ptr, ref.stride,
                                                w, h, bit_depth, filter_mode, int(use_alt_hpel), _ptr(d_items), n, _ptr(out)))
        return out

    def subpel_refine_batch(self, func, org, ref, d_bases, n_blocks, offsets, w, h, bit_depth=10, filter_mode=0, use_alt_hpel=False, out=None):
        """one xPatternRefinement stage for many blocks: offsets = [(dx, dy), ...] in 1/16 sample around each block's base vector -> (n_blocks, len(offsets)) costs"""
        offs = np.ascontiguousarray(offsets, np.int16).reshape(-1, 2)
        if out is None:
            out = torch.empty(n_blocks * offs.shape[0], dtype=torch.int64, device=self.device)
        self._ck(self.L.vvhip_subpel_refine_batch(self.ctx, DF[func] if isinstance(func, str) else func, org.buf_ptr, org.stride, ref.buf_ptr, ref.stride, w, h, bit_depth,
                                                  filter_mode, int(use_alt_hpel), _ptr(d_bases), n_blocks, offs.ctypes.data_as(C.c_void_p), offs.shape[0], _ptr(out)))
        return out

    # ---- (C) MCTF ----
    def extend_border(self, plane):
        self._ck(self.L.vvhip_extend_border(self.ctx, plane.buf_ptr, plane.stride, plane.width, plane.height, plane.pad))

    def mctf_subsample(self, src, pad=128):
        dst = Plane(self.device, src.width // 2, src.height // 2, pad)
        self._ck(self.L.vvhip_mctf_subsample(self.ctx, src.buf_ptr, src.stride, src.width, src.height, dst.buf_ptr, dst.stride, pad))
        return dst

    def mctf_error_batch(self, org, buf, d_items, n, w, h, tap4, bit_depth=10):
        out = torch.empty(n, dtype=torch.int32, device=self.device)
        self._ck(self.L.vvhip_mctf_error_batch(self.ctx, org.buf_ptr, org.stride, buf.buf_ptr, buf.stride, w, h, int(tap4), bit_depth, _ptr(d_items), n, _ptr(out)))
        return out

    def mctf_calc_var_batch(self, org, d_off, n, w, h):
        out = torch.empty(n, dtype=torch.int64, device=self.device)
        self._ck(self.L.vvhip_mctf_calc_var_batch(self.ctx, org.buf_ptr, org.stride, w, h, _ptr(d_off), n, _ptr(out)))
        return out

    def new_mv_field(self, w, h):
        t = torch.empty((h * w, MV_DTYPE.itemsize), dtype=torch.uint8, device=self.device)
        self._ck(self.L.vvhip_mctf_init_mvs(self.ctx, _ptr(t), w * h))
        return t

    def mctf_me_level(self, org, buf, block_size, prev, prev_dims, factor, double_res, mvs, mvs_dims, search_pattern=2, low_res=1, bit_depth=10, unit=16):
        pw, ph = prev_dims if prev is not None else (0, 0)
        self._ck(self.L.vvhip_mctf_me_level(self.ctx, org.buf_ptr, org.stride, buf.buf_ptr, buf.stride, org.width, org.height, block_size,
                                            _ptr(prev), pw, ph, factor, int(double_res), search_pattern, int(low_res), bit_depth, unit,
                                            _ptr(mvs), mvs_dims[0], mvs_dims[1]))
        return mvs

    def mctf_motion_estimation(self, cur, refs, bit_depth=10, unit=16, speed=4, add_level=None, out=None, wait=True):
        """cur / refs: Plane objects with identical geometry and pad >= 128 (borders extended).  wait=False: queued on the context's stream, no host wait
        (vvhip_mctf_motion_estimation_async)."""
        if add_level is None:
            add_level = cur.width >= 1920            # MCTF.cpp:768
        ow, oh = (cur.width + unit - 1) // unit, (cur.height + unit - 1) // unit
        if out is None:
            out = [torch.empty((ow * oh, MV_DTYPE.itemsize), dtype=torch.uint8, device=self.device) for _ in refs]
        ref_ptrs = (C.c_void_p * len(refs))(*[r.buf_ptr.value for r in refs])
        out_ptrs = (C.c_void_p * len(refs))(*[o.data_ptr() for o in out])
        for r in refs:
            assert (r.width, r.height, r.stride, r.pad) == (cur.width, cur.height, cur.stride, cur.pad)
        fn = self.L.vvhip_mctf_motion_estimation if wait else self.L.vvhip_mctf_motion_estimation_async
        self._ck(fn(self.ctx, cur.buf_ptr, ref_ptrs, len(refs), cur.stride, cur.width, cur.height, cur.pad, bit_depth, unit, speed, int(bool(add_level)), out_ptrs))
        return out, (ow, oh)

    def mctf_set_stats(self, on):
        self._ck(self.L.vvhip_mctf_set_stats(self.ctx, int(bool(on))))

    def quant_core(self, coef, quant_coeff, q_bits, add, thr_val=8, lfnst_idx=0):
        """QuantCore's own argument list on ONE block (numpy int32 h x w) -> (levels h x w int16, deltaU w*h int32, abs sum, last scan position); lfnst_idx > 0: the
        first-coefficient-group rule of LFNST TUs (vvhip_quant_core_lfnst)"""
        coef = np.ascontiguousarray(coef, np.int32)
        h, w = coef.shape
        d_c = self.to_device(coef.reshape(-1))
        d_l = torch.full((h * w,), 0x7777, dtype=torch.int16, device=self.device)
        d_u = torch.zeros(h * w, dtype=torch.int32, device=self.device)
        d_s = torch.zeros(2, dtype=torch.int32, device=self.device)
        self._ck(self.L.vvhip_quant_core_lfnst(self.ctx, _ptr(d_c), w, h, quant_coeff, q_bits, add, thr_val, int(lfnst_idx), _ptr(d_l), _ptr(d_u), C.c_void_p(d_s.data_ptr()),
                                               C.c_void_p(d_s.data_ptr() + 4)))
        torch.cuda.synchronize()
        sv = d_s.cpu().numpy()
        return d_l.cpu().numpy().reshape(h, w), d_u.cpu().numpy(), int(sv[0]), int(sv[1])

    def tu_set_sparse_outputs(self, on):
        """vvhip_tu_set_sparse_outputs: the fused TU launches write no levels / reconstruction for TUs whose levels are all zero (the caller treats them as zero)"""
        self._ck(self.L.vvhip_tu_set_sparse_outputs(self.ctx, int(bool(on))))

    def mctf_set_timing(self, on):
        self._ck(self.L.vvhip_mctf_set_timing(self.ctx, int(bool(on))))

    def mctf_last_times(self):
        """ms of the last motion-estimation call per class: (candidate scoring, neighbour scoring, sweep, final normalisation, rest)"""
        a = (C.c_float * 5)()
        self._ck(self.L.vvhip_mctf_last_times(self.ctx, a))
        return tuple(float(x) for x in a)

    def mctf_get_stats(self):
        """scored candidates of the MCTF search since mctf_set_stats(True): {phase: {int, int_bytes, frac, frac_bytes, grid, grid_window_bytes, ring, ring_window_bytes}}
        (include/vvenc_hip.h)"""
        a = np.zeros(24, np.uint64)
        self._ck(self.L.vvhip_mctf_get_stats(self.ctx, a.ctypes.data_as(C.c_void_p)))
        keys = ("int", "int_bytes", "frac", "frac_bytes", "grid", "grid_window_bytes", "ring", "ring_window_bytes")
        return {ph: {k: int(a[8 * i + j]) for j, k in enumerate(keys)} for i, ph in enumerate(("search", "neighbour", "sweep"))}

    @staticmethod
    def mv_to_numpy(t, dims):
        return t.cpu().numpy().view(MV_DTYPE).reshape(dims[1], dims[0])
