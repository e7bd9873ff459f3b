/*
 * vvenc_hip.h — C ABI of libvvenc_hip.so: the MI355X (gfx950) back-end for VVenC's block-level
 * RDO hot path (distortion kernels, transform + scalar quantisation, MCTF block matching).
 *
 * This is the drop-in boundary one level below the reference's C++ function-pointer tables:
 * the table-shaped shim (vvenc_amd/csrc/host/) forwards batches of CU/PU/TU
 * candidates to these entry points.  All bulk pointers are DEVICE pointers (prefix d_) into HBM
 * unless the name says `_host`; every call is asynchronous on the context's HIP stream and ordered
 * with respect to the other calls on the same context.  Results are bit-exact with the
 * reference's scalar and x86-SIMD kernels (citations: paths below /root/reference/source/Lib/).
 *
 * Error convention: every function returns VVHIP_OK (0) or a negative VVHIP_E_* code and records
 * a message retrievable with vvhip_last_error().  The reference has no error codes at this level
 * (programming errors THROW, CommonLib/TypeDef.h:635-636); the shim turns a non-zero return into
 * the same exception.  There is NO CPU fallback anywhere behind this ABI.
 *
 * Types: Pel = int16_t, TCoeff = int32_t, TCoeffSig = int16_t, TMatrixCoeff = int16_t,
 * Distortion = uint64_t (CommonLib/TypeDef.h:181-192).
 */
#ifndef VVENC_HIP_H
#define VVENC_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VVHIP_API __attribute__((visibility("default")))

enum {
  VVHIP_OK           = 0,
  VVHIP_E_ARG        = -1,  /* invalid argument (size/type combination the reference THROWs on)  */
  VVHIP_E_HIP        = -2,  /* a HIP runtime call failed; message holds hipGetErrorString          */
  VVHIP_E_NOMEM      = -3,
  VVHIP_E_UNSUPPORTED= -4
};

typedef struct vvhip_ctx vvhip_ctx;

/* ---------------------------------------------------------------------------------------------
 * Context, stream and raw device-memory helpers (so that a C/C++ host needs nothing but this ABI)
 * ------------------------------------------------------------------------------------------- */
VVHIP_API int         vvhip_create( vvhip_ctx** out, int device );     /* own non-blocking stream + ROM tables in HBM */
VVHIP_API void        vvhip_destroy( vvhip_ctx* ctx );
VVHIP_API const char* vvhip_last_error( const vvhip_ctx* ctx );        /* ctx may be NULL: error of vvhip_create       */
VVHIP_API int         vvhip_set_stream( vvhip_ctx* ctx, void* hip_stream ); /* borrow a caller's hipStream_t (NULL = the default stream) */
VVHIP_API int         vvhip_use_own_stream( vvhip_ctx* ctx );          /* back to the context's private stream          */
VVHIP_API void*       vvhip_get_stream( vvhip_ctx* ctx );
VVHIP_API int         vvhip_sync( vvhip_ctx* ctx );                    /* hipStreamSynchronize                          */
VVHIP_API int         vvhip_set_blocking_sync( vvhip_ctx* ctx, int on ); /* on: vvhip_sync and the downloads wait on a blocking event (the thread sleeps) instead of hipStreamSynchronize —
                                                                        * for hosts whose cores are all busy (an encoder's worker threads); default off (lowest latency) */
VVHIP_API int         vvhip_sync_all_devices( vvhip_ctx* ctx );        /* hipDeviceSynchronize on every device, the calling thread's current device restored: before host memory other
                                                                        * contexts may still be copying from is unpinned or released */
/* Launch graphs: the batch entry points only enqueue kernels on the context's stream, so a frame's fixed sequence of calls (the lists of one picture: same tables,
 * same buffers) can be recorded once and replayed with one hipGraphLaunch instead of one dispatch per call.  Between begin and end no call may synchronise, allocate
 * (call every entry point once beforehand so scratch buffers exist) or touch another stream; the stream must not be the legacy default stream (vvhip_use_own_stream).  No counterpart in the reference: its table entries are synchronous calls. */
typedef struct vvhip_graph vvhip_graph;
VVHIP_API int         vvhip_graph_begin( vvhip_ctx* ctx );                         /* hipStreamBeginCapture on the context's stream */
VVHIP_API int         vvhip_graph_end( vvhip_ctx* ctx, vvhip_graph** out );        /* end capture + instantiate                     */
VVHIP_API int         vvhip_graph_launch( vvhip_ctx* ctx, vvhip_graph* graph );    /* replay on the context's stream                */
VVHIP_API void        vvhip_graph_destroy( vvhip_graph* graph );
VVHIP_API int         vvhip_malloc( vvhip_ctx* ctx, void** d_ptr, size_t bytes );
VVHIP_API int         vvhip_free( vvhip_ctx* ctx, void* d_ptr );
VVHIP_API int         vvhip_upload( vvhip_ctx* ctx, void* d_dst, const void* host_src, size_t bytes );   /* async on stream */
VVHIP_API int         vvhip_download( vvhip_ctx* ctx, void* host_dst, const void* d_src, size_t bytes ); /* async + sync    */
VVHIP_API int         vvhip_download_async( vvhip_ctx* ctx, void* host_dst, const void* d_src, size_t bytes ); /* no sync: pair with vvhip_sync; host_dst should be pinned */
/* strided forms (pitches and width in BYTES): a picture window moves without a packing pass on the host (hipMemcpy2DAsync)               */
VVHIP_API int         vvhip_upload_2d( vvhip_ctx* ctx, void* d_dst, size_t dst_pitch, const void* host_src, size_t src_pitch, size_t width_bytes, size_t rows );
VVHIP_API int         vvhip_download_2d( vvhip_ctx* ctx, void* host_dst, size_t dst_pitch, const void* d_src, size_t src_pitch, size_t width_bytes, size_t rows ); /* async + sync */
/* Pin a caller-owned host range in place (hipHostRegister) so that uploads / downloads touching it are true asynchronous DMA at full PCIe rate instead of
 * being staged through the runtime's bounce buffers.  The encoder's picture buffers are recycled for the whole run: register once, unregister before free.   */
VVHIP_API int         vvhip_host_register( vvhip_ctx* ctx, const void* host_ptr, size_t bytes );
VVHIP_API int         vvhip_host_unregister( vvhip_ctx* ctx, const void* host_ptr );
/* pinned host memory owned by the library's caller (hipHostMalloc): download / upload areas that are not the encoder's own buffers                                  */
VVHIP_API int         vvhip_host_alloc( vvhip_ctx* ctx, void** host_ptr, size_t bytes );
VVHIP_API int         vvhip_host_free( vvhip_ctx* ctx, void* host_ptr );
/* Completion marks for work a worker thread leaves behind (hipEvent_t without timing): recorded on the recording context's stream, awaited by ANY thread — a picture stage
 * issued piecewise by several workers (the ALF statistics of a picture, one band per row task: EncoderLib/EncSlice.cpp:1135-1167) is collected by the thread that needs the
 * whole (EncAdaptiveLoopFilter::deriveFilter, EncoderLib/EncAdaptiveLoopFilter.cpp:1757) without a stream synchronisation per piece.                                          */
VVHIP_API int         vvhip_event_create( vvhip_ctx* ctx, void** event );
VVHIP_API int         vvhip_event_record( vvhip_ctx* ctx, void* event );          /* on the context's stream */
VVHIP_API int         vvhip_event_wait( vvhip_ctx* ctx, void* event );            /* host wait (ctx: error reporting only; an event never recorded is complete) */
VVHIP_API int         vvhip_event_destroy( vvhip_ctx* ctx, void* event );
/* Several GPUs in one process (one context per device and worker thread): number of devices, the device of a context, and a device-to-device copy of a
 * picture over xGMI (hipMemcpyPeerAsync on dst's stream, ordered after the work already queued on src's stream) — how an original or reconstructed
 * picture reaches the GPU that serves the pictures depending on it without a round trip through the host.                                        */
VVHIP_API int         vvhip_device_count( void );
VVHIP_API int         vvhip_get_device( const vvhip_ctx* ctx );
VVHIP_API int         vvhip_make_current( vvhip_ctx* ctx );              /* hipSetDevice( the context's device ) for the calling thread: call when a thread switches GPUs */
VVHIP_API int         vvhip_copy_peer( vvhip_ctx* dst_ctx, void* d_dst, vvhip_ctx* src_ctx, const void* d_src, size_t bytes );
VVHIP_API const char* vvhip_version( void );

/* ---------------------------------------------------------------------------------------------
 * (A) Distortion kernels — replaces RdCost::m_afpDistortFunc[0][DF_*] / m_afpDistortFuncX5
 *     (CommonLib/RdCost.h:117-121; scalar CommonLib/RdCost.cpp:301-2093; SIMD CommonLib/x86/RdCostX86.h)
 *
 * One call evaluates n candidates of ONE block size with ONE function.  A candidate is a pair of
 * sample offsets relative to d_org / d_cur (the DistParam's org.buf / cur.buf; offsets may be
 * negative = inside the picture margin).  out[i] is what distFunc(DistParam) returns.
 * ------------------------------------------------------------------------------------------- */
enum {                    /* reference table rows (CommonLib/TypeDef.h:339-382)                         */
  VVHIP_DF_SSE      = 0,  /* DF_SSE + log2(w)        xGetSSE*        RdCost.cpp:651-1000               */
  VVHIP_DF_SAD      = 1,  /* DF_SAD + log2(w)        xGetSAD*        RdCost.cpp:301-644  (subShift)    */
  VVHIP_DF_HAD      = 2,  /* DF_HAD + log2(w)        xGetHADs<false> RdCost.cpp:1818-1938              */
  VVHIP_DF_HAD_FAST = 3,  /* DF_HAD_fast + log2(w)   xGetHADs<true>                                    */
  VVHIP_DF_HAD_2SAD = 4   /* DF_HAD_2SAD             xGetHAD2SADs    RdCost.cpp:1768-1816              */
};

typedef struct { int32_t org_off; int32_t cur_off; } vvhip_dist_item;

VVHIP_API int vvhip_dist_batch( vvhip_ctx* ctx, int func,
                                const int16_t* d_org, int org_stride,
                                const int16_t* d_cur, int cur_stride,
                                int width, int height, int sub_shift, int bit_depth,
                                const vvhip_dist_item* d_items, int n, uint64_t* d_out );

/* Several batches of ONE function over the same plane pair (e.g. all block sizes of a frame's SAD work list) in as few launches as
 * possible: semantically n_jobs x vvhip_dist_batch; jobs the merged kernels cannot take run as separate launches.  `jobs` is a HOST array. */
typedef struct { int32_t width, height, sub_shift, n; const vvhip_dist_item* d_items; uint64_t* d_out; } vvhip_dist_job;
VVHIP_API int vvhip_dist_multi( vvhip_ctx* ctx, int func, const int16_t* d_org, int org_stride, const int16_t* d_cur, int cur_stride, int bit_depth,
                                const vvhip_dist_job* jobs_host, int n_jobs );

/* The same with a function per job: consecutive jobs of one kernel family — SAD and SSE, or HAD and HAD_fast — share a launch (a frame's
 * SAD and SSE lists are both short, memory-side work; together they fill the device better).
 * flags: VVHIP_DIST_FLAG_SAMPLES = the caller asserts that BOTH operands of the job hold samples in [0, 2^bit_depth) (original vs reconstructed /
 * predicted picture samples).  Without it the Hadamard jobs accept everything the encoder hands to a HAD table entry at that bit depth, including
 * the bi-prediction pattern 2*org - pred (values -(2^bd - 1) .. 2*(2^bd - 1), EncoderLib/InterSearch.cpp:1996-2003), through a slightly wider tile;
 * results are identical wherever both forms are defined.  An SSE job with the flag (bit depth <= 12; here the flag may also stand for residuals, |operand| < 2^bit_depth)
 * squares packed 16-bit differences (v_dot2_i32_i16).  vvhip_dist_multi (no flags field) always uses the general form.                 */
#define VVHIP_DIST_FLAG_SAMPLES 1
typedef struct { int32_t func, width, height, sub_shift, n, flags; const vvhip_dist_item* d_items; uint64_t* d_out; } vvhip_dist_fjob;
VVHIP_API int vvhip_dist_multi_func( vvhip_ctx* ctx, const int16_t* d_org, int org_stride, const int16_t* d_cur, int cur_stride, int bit_depth,
                                     const vvhip_dist_fjob* jobs_host, int n_jobs );

/* The same lists on 8x8-TILED copies of the planes (no counterpart in the reference: a memory-layout decision for the MI355X).  A 128-byte cache line holds one 8x8 tile of
 * int16 samples; in a row-major plane an 8x8 block is eight 16-byte pieces in eight lines, each its own L1 access (29 accesses per 8x8 SAD candidate, 10.5 on the tiled
 * copy: the lists run at the L1's access rate).  vvhip_plane_tile8 makes the tiled copy of a padded plane (d_base = first sample of the padded plane, `rows` lines of `stride` samples; d_tiled holds
 * vvhip_tiled8_elems( stride, rows ) samples; re-tile when the plane changes).  vvhip_dist_multi_func_tiled = vvhip_dist_multi_func, identical results, with the 8x8 SAD / SSE jobs
 * of bit depths <= 10 reading the tiled copies (the Hadamard jobs were measured slower there and stay on the row-major planes) (tiled may be NULL: no difference to vvhip_dist_multi_func; either tiled pointer may be NULL: those jobs stay on the row-major planes).  *_margin = samples of margin around
 * sample (0,0) of the plane the tiled copy was made from (d_org / d_cur still address sample (0,0) of the row-major planes, used by the other jobs).                          */
typedef struct { const int16_t* d_org_tiled; const int16_t* d_cur_tiled; int32_t org_margin, cur_margin;
                 const int16_t* d_cur_shift1;   /* optional (NULL: none): the sample of a ONE-SAMPLE-SHIFTED copy of the reference plane buffer that corresponds to d_cur, i.e.
                                                   d_cur_shift1[k] == d_cur[k + 1] for every sample of the padded plane (vvhip_plane_shift1 over the whole buffer).  Candidates at odd
                                                   sample addresses (half of all motion vectors) are then read from the copy with dword-aligned loads — an only 2-byte-aligned
                                                   16-byte lane load is split by the memory pipeline and costs 1.8x; every job on the row-major planes uses it */
               } vvhip_tiled_planes;
/* d_dst[i] = d_src[i + 1] for i < elems - 1, d_dst[elems - 1] = 0; both buffers with the same alignment modulo 4 bytes */
VVHIP_API int vvhip_plane_shift1( vvhip_ctx* ctx, const int16_t* d_src, size_t elems, int16_t* d_dst );
/* all three derived copies of a picture's planes in one launch (what a caller does once per picture): the 8x8-tiled copy of the original plane, the 8x8-tiled and the one-sample-shifted
 * copy of the reference plane.  *_base = first sample of the padded plane buffer, `rows` lines of `stride` samples; any output may be NULL (skipped).
 * d_cur_shift1 covers the whole buffer (stride * rows samples) like vvhip_plane_shift1. */
VVHIP_API int vvhip_planes_derive( vvhip_ctx* ctx, const int16_t* d_org_base, int org_stride, int org_rows, int16_t* d_org_tiled,
                                   const int16_t* d_cur_base, int cur_stride, int cur_rows, int16_t* d_cur_tiled, int16_t* d_cur_shift1 );
VVHIP_API size_t vvhip_tiled8_elems( int stride, int rows );
VVHIP_API int vvhip_plane_tile8( vvhip_ctx* ctx, const int16_t* d_base, int stride, int rows, int16_t* d_tiled );
VVHIP_API int vvhip_dist_multi_func_tiled( vvhip_ctx* ctx, const int16_t* d_org, int org_stride, const int16_t* d_cur, int cur_stride, const vvhip_tiled_planes* tiled_host, int bit_depth,
                                           const vvhip_dist_fjob* jobs_host, int n_jobs );

/* DMVR 5-position SAD: RdCost::xGetSAD8X5 / xGetSAD16X5 (RdCost.cpp:1984-2034). width 8 or 16.
 * d_out5[5*i+k] = SAD(org+k, cur-k) >> 1; entry 2 is left untouched when calc_centre == 0.       */
VVHIP_API int vvhip_sad_x5_batch( vvhip_ctx* ctx,
                                  const int16_t* d_org, int org_stride,
                                  const int16_t* d_cur, int cur_stride,
                                  int width, int height, int sub_shift, int calc_centre,
                                  const vvhip_dist_item* d_items, int n, uint64_t* d_out5 );

/* GEO masked SAD: RdCost::xGetSADwMask (RdCost.cpp:2062-2093), table slot DF_SAD_WITH_MASK (TypeDef.h:339-382).
 *   d_out[i] = ( sum over processed rows r, columns x of |org - cur| * mask[...] ) << sub_shift
 * with the mask walked exactly as the reference does: +step_x per sample, + mask_stride*(1<<sub_shift) + mask_stride2 per
 * processed row, starting at d_mask + d_mask_off[i] (d_mask_off may be NULL: every candidate starts at d_mask).               */
VVHIP_API int vvhip_sad_mask_batch( vvhip_ctx* ctx,
                                    const int16_t* d_org, int org_stride,
                                    const int16_t* d_cur, int cur_stride,
                                    const int16_t* d_mask, int mask_stride, int step_x, int mask_stride2,
                                    int width, int height, int sub_shift, int bit_depth,
                                    const vvhip_dist_item* d_items, const int32_t* d_mask_off, int n, uint64_t* d_out );

/* Fixed-weight SSE: RdCost::m_fxdWtdPredPtr = fixWeightedSSE_Core (RdCost.cpp:1948-1982, RdCost.h:117).
 *   d_out[i] = sum ( int )( ( weight_i * d*d + 2^15 ) >> 16 ),  width even or 1.                                               */
VVHIP_API int vvhip_fix_weighted_sse_batch( vvhip_ctx* ctx,
                                            const int16_t* d_org, int org_stride,
                                            const int16_t* d_cur, int cur_stride,
                                            int width, int height, int bit_depth,
                                            const vvhip_dist_item* d_items, const uint32_t* d_weights, int n, uint64_t* d_out );

/* Full-window SAD cost surface for one block size: for block b (top-left org sample offset
 * d_block_org_off[b], co-located reference offset d_block_ref_off[b]) and every integer displacement
 * (dx,dy), |dx| <= range_x, |dy| <= range_y:
 *   d_out[(b*(2*range_y+1) + dy+range_y)*(2*range_x+1) + dx+range_x] = xGetSAD(org, ref + dy*stride + dx)
 * (same subShift rule).  Exact integers, so any subset a host search asks for is bit-exact
 * (SURVEY §7 "cost-surface precompute").  The reference window is staged once in LDS.            */
VVHIP_API int vvhip_sad_surface( vvhip_ctx* ctx,
                                 const int16_t* d_org, int org_stride,
                                 const int16_t* d_ref, int ref_stride,
                                 int width, int height, int sub_shift,
                                 int range_x, int range_y,
                                 const int32_t* d_block_org_off, const int32_t* d_block_ref_off, int n_blocks,
                                 uint32_t* d_out );

/* ---------------------------------------------------------------------------------------------
 * (B) Transforms + scalar quantisation — replaces g_tCoeffOps.* as driven by TrQuant::xT / xIT
 *     (CommonLib/TrQuant.cpp:481-655, TrQuant_EMT.cpp:152-420,1917-2000) and Quant::xQuant /
 *     xDeQuant / xNeedRdoq (CommonLib/Quant.cpp:132-278 with the parameter derivation of
 *     Quant::quant :735-833, Quant::dequant :520-610, Quant::xNeedRDOQ :835-891).
 *
 * A batch holds n TUs of ONE size and ONE transform-type pair.  TU i reads/writes its residual
 * at d_resi + d_resi_off[i] (stride resi_stride); coefficient / level arrays are compact,
 * n * width * height, TU-major, raster inside the TU (what TrQuant::m_plTempCoeff holds).
 * ------------------------------------------------------------------------------------------- */
enum { VVHIP_DCT2 = 0, VVHIP_DCT8 = 1, VVHIP_DST7 = 2 };   /* TransType, CommonLib/TypeDef.h */

VVHIP_API int vvhip_fwd_transform_batch( vvhip_ctx* ctx, const int16_t* d_resi, int resi_stride, const int32_t* d_resi_off,
                                         int n, int width, int height, int tr_hor, int tr_ver, int bit_depth,
                                         int32_t* d_coef );
VVHIP_API int vvhip_inv_transform_batch( vvhip_ctx* ctx, const int32_t* d_coef,
                                         int n, int width, int height, int tr_hor, int tr_ver, int bit_depth,
                                         int16_t* d_resi, int resi_stride, const int32_t* d_resi_off );

/* per-TU quantiser control: qp = QpParam::Qp (base QP incl. qpBdOffset); flags bit0 = slice isIRAP
 * (iAdd 171 instead of 85, Quant.cpp:775), bit1 = luma (need-RDOQ offset 171 instead of 256, :874)   */
typedef struct { int16_t qp; int16_t flags; } vvhip_tu_qp;

VVHIP_API int vvhip_quant_batch( vvhip_ctx* ctx, const int32_t* d_coef, int n, int width, int height, int bit_depth,
                                 const vvhip_tu_qp* d_qp, int thr_val,
                                 int16_t* d_level, int32_t* d_delta_u /* may be NULL */,
                                 int32_t* d_abs_sum, int32_t* d_last_scan_pos );
VVHIP_API int vvhip_dequant_batch( vvhip_ctx* ctx, const int16_t* d_level, int n, int width, int height, int bit_depth,
                                   const vvhip_tu_qp* d_qp, int32_t* d_coef );
VVHIP_API int vvhip_need_rdoq_batch( vvhip_ctx* ctx, const int32_t* d_coef, int n, int width, int height, int bit_depth,
                                     const vvhip_tu_qp* d_qp, uint8_t* d_need );

/* Raw-parameter forms with exactly the argument lists of the reference's table entries Quant::xDeQuant / Quant::xNeedRdoq
 * (CommonLib/Quant.h:143-151; QuantCore / DeQuantCore / needRdoqCore, Quant.cpp:132-278;
 * vvhip_quant_core takes QuantCore's defaultQuantisationCoefficient, iQBits, iAdd, m_thrVal; lfnstIdx == 0 — vvhip_quant_core_lfnst any), for the table-shaped shim: ONE block per call.
 * d_level is strided (level_stride), d_coef compact (max_x+1) x (max_y+1); *d_need receives 0/1.                            */
VVHIP_API int vvhip_dequant_core( vvhip_ctx* ctx, int max_x, int max_y, int scale, const int16_t* d_level, size_t level_stride, int32_t* d_coef,
                                  int right_shift, int input_maximum, int32_t transform_maximum );
VVHIP_API int vvhip_quant_core( vvhip_ctx* ctx, const int32_t* d_coef, int width, int height, int quant_coeff, int q_bits, int64_t add, int thr_val,
                                int16_t* d_level /* w*h compact */, int32_t* d_delta_u /* may be NULL */, int32_t* d_abs_sum, int32_t* d_last_scan_pos );
/* QuantCore for a TU of a coding unit with lfnst_idx > 0 (CodingUnit::lfnstIdx, presets fast / medium): only the first coefficient group is quantised, its first 8 scan
 * positions for 4x4 and 8x8 TUs (Quant.cpp:149-159); lfnst_idx == 0 is vvhip_quant_core.  Replaces the same table entry (Quant::xQuant, Quant.h:143-146).            */
VVHIP_API int vvhip_quant_core_lfnst( vvhip_ctx* ctx, const int32_t* d_coef, int width, int height, int quant_coeff, int q_bits, int64_t add, int thr_val, int lfnst_idx,
                                      int16_t* d_level /* w*h compact */, int32_t* d_delta_u /* may be NULL */, int32_t* d_abs_sum, int32_t* d_last_scan_pos );
VVHIP_API int vvhip_need_rdoq_core( vvhip_ctx* ctx, const int32_t* d_coef, size_t num_coeff, int quant_coeff, int64_t offset, int shift, uint8_t* d_need );

/* Fused TU pipeline of the residual RDO loop (InterSearch::xEstimateInterResidualQT,
 * EncoderLib/InterSearch.cpp:3663-3714): xT -> xNeedRDOQ + QuantCore -> DeQuantCore -> xIT -> SSE(resi, rec).
 * Reads 2*w*h bytes, writes 2*w*h (levels) + 2*w*h (reconstructed residual) + 24 bytes of statistics per TU;
 * intermediate coefficients never leave the CU (LDS).  Any output pointer may be NULL.          */
typedef struct { int32_t abs_sum; int32_t last_scan_pos; int32_t need_rdoq; int32_t pad; uint64_t sse; } vvhip_tu_stats;

VVHIP_API int vvhip_tu_rdo_batch( vvhip_ctx* ctx, const int16_t* d_resi, int resi_stride, const int32_t* d_resi_off,
                                  int n, int width, int height, int tr_hor, int tr_ver, int bit_depth,
                                  const vvhip_tu_qp* d_qp, int thr_val,
                                  int16_t* d_level, int16_t* d_rec_resi /* compact n*w*h */, vvhip_tu_stats* d_stats );

/* A frame's TU work lists in one call: every job is one vvhip_tu_rdo_batch argument set on the same residual plane.  Square 8/16/32
 * TUs (any transform types) are merged into ONE launch, largest size first — the per-size launches are each too small to fill
 * the device; other shapes run as individual launches.  Results are identical to per-job vvhip_tu_rdo_batch calls.               */
typedef struct
{
  int32_t width, height, tr_hor, tr_ver, n, thr_val;
  const int32_t*     d_resi_off;
  const vvhip_tu_qp* d_qp;
  int16_t*           d_level;
  int16_t*           d_rec_resi;
  vvhip_tu_stats*    d_stats;
} vvhip_tu_job;
VVHIP_API int vvhip_tu_rdo_multi( vvhip_ctx* ctx, const int16_t* d_resi, int resi_stride, int bit_depth, const vvhip_tu_job* jobs_host, int n_jobs );
/* The same with a residual row pitch PER JOB (resi_strides_host[i] for jobs_host[i]): lists whose residual blocks are stored compactly, one after the other (pitch = width), as a
 * caller that gathers the TUs of many CUs into one buffer has them — e.g. every TU InterSearch::xEstimateInterResidualQT tests for a picture (EncoderLib/InterSearch.cpp:3663-3714). */
VVHIP_API int vvhip_tu_rdo_multi_strided( vvhip_ctx* ctx, const int16_t* d_resi, const int32_t* resi_strides_host, int bit_depth, const vvhip_tu_job* jobs_host, int n_jobs );

/* Sparse outputs of vvhip_tu_rdo_multi / _multi_strided (default off = every output of every TU is written).  On: for a TU whose levels are ALL ZERO (stats.abs_sum == 0)
 * d_level and d_rec_resi are UNSPECIFIED — left untouched wherever the matrix-core launch takes a whole 32x32 tile (or a 64x64 TU) through its all-zero shortcut, zeros
 * otherwise — and the caller treats them as zero.  That is what the reference's caller does: xEstimateInterResidualQT reads neither the levels nor the reconstruction of a TU
 * whose uiAbsSum is 0 (EncoderLib/InterSearch.cpp:3696-3714: invTransformNxN only runs for a non-zero abs sum).  Statistics (abs_sum, last_scan_pos, need_rdoq, sse) are always
 * written.  An all-zero tile then moves 2 w h bytes in and 24 bytes per TU out instead of 6 w h + 24.                                                                          */
VVHIP_API int vvhip_tu_set_sparse_outputs( vvhip_ctx* ctx, int on );

/* Joint Cb-Cr residual coding (ICT) around the fused TU pipeline: the detour every chroma TU with a coded block flag takes in InterSearch::xEstimateInterResidualQT
 * (EncoderLib/InterSearch.cpp:3770-3960) — TrQuant::selectICTCandidates -> fwdTransformICT (CommonLib/TrQuant.cpp:350-410), ONE pass of the joint residual through
 * transform / quantisation / dequantisation / inverse transform, invTransformICT (:358-362), two SSEs — as two list entries, so that a picture's chroma residuals stay on the
 * device: forward, then vvhip_tu_rdo_multi_strided on the joint buffer, then inverse.  The arithmetic is fwdTransformCbCr / invTransformCbCr (TrQuant.cpp:95-164), bit-exact
 * for ANY int16 input.  mode = the signed ICT mode g_ictModes[jointCbCrSign][cbfMask] (Rom.cpp:1453: { 0, 3, 1, 2 } / { 0, -3, -1, -2 }; TU::getICTMode), computed by the caller.
 *   forward, per sample with cb, cr widened to int ( / truncates toward zero; the quotient is narrowed to int16 as Pel( ... ) does, wrapping at the extremes; the distortion
 *   uses the narrowed value; ( -c ) >> 1 is an arithmetic shift of the negated int; sums are int64 ):
 *     mode +-1 : c = ( 4 cb +- 2 cr ) / 5,  d1 += ( cb - c )^2 + ( cr - ( ( +-c ) >> 1 ) )^2
 *     mode +-2 : c = ( cb +- cr ) / 2,      d1 += ( cb - c )^2 + ( cr -+ c )^2
 *     mode +-3 : c = ( 4 cr +- 2 cb ) / 5,  d1 += ( cb - ( ( +-c ) >> 1 ) )^2 + ( cr - c )^2
 *     mode 0   : no joint block,            d1 = sum cb^2, d2 = sum cr^2            ( d2 = 0 for the other modes )
 *   inverse: the joint reconstruction IS the coded component — Cb for |mode| = 1, 2, Cr for |mode| = 3 — and the other one is derived, narrowed to int16:
 *     mode +-1 : cr = ( +-cb ) >> 1        mode +-2 : cr = +-cb        mode +-3 : cb = ( +-cr ) >> 1
 *   item      : one chroma TU.  Its Cb and Cr blocks sit at cb_off / cr_off (sample offsets) with row pitch stride — in d_resi for the forward entry, in d_rec and
 *               d_org_resi for the inverse entry: the reconstruction mirrors the residual layout, as d_resi mirrors d_pred in the prediction lists (compact blocks, or two
 *               planes of one buffer).  The joint block is COMPACT (row pitch = width) at joint_off: d_joint is directly a d_resi of vvhip_tu_rdo_multi_strided with
 *               resi_strides_host[i] = width, and that job's d_rec_resi a d_joint_rec.  width / height independent powers of two, 2..64.
 *   forward   : writes the joint block (mode != 0) and d_dist[2i], d_dist[2i + 1] = ( d1, d2 ).  Several items may name the same Cb / Cr pair with different modes — the four
 *               masks selectICTCandidates tests for an intra CU — and the host selection (TrQuant.cpp:377-407) is fed from d_dist.
 *   inverse   : writes both components to d_rec and d_sse[2i], d_sse[2i + 1] = the plain sums of squared differences of the Cb / Cr reconstruction against d_org_resi —
 *               unweighted and without precision shift, like vvhip_tu_stats.sse (the chroma distortion weight of RdCost::getDistPart stays with the caller).
 *               With stats_idx >= 0 and d_stats[stats_idx].abs_sum == 0 the joint reconstruction is taken as ALL ZERO and d_joint_rec is not read for that item: the reference
 *               fills the block with zero there (InterSearch.cpp:3896-3899), and the sparse outputs of vvhip_tu_set_sparse_outputs leave that memory unspecified — with the
 *               TU job's statistics named here the chain runs with sparse outputs on.
 * items_host is a HOST array, like the prediction lists': the library sorts it into size classes (a wave never mixes shapes; small blocks share a wave — sixteen 4x4 or
 * thirty-two 2x2 blocks), and keeps the device copy of that schedule in the context, per entry and apart from the prediction entries' — the same list again uploads and
 * allocates nothing, and alternating with the prediction entries evicts none of their schedules.  Results do not depend on the order of the list; nothing outside the named
 * blocks is written; every access is a vector access as wide as the block's offsets, pitch and width and the buffers' addresses allow (16 bytes at best); every sum is
 * reduced inside one wave and stored once — no atomics, so the results are deterministic.  Output blocks of different items must not overlap.
 * Argument errors (VVHIP_E_ARG with a message naming the entry, nothing launched): n < 0; a size that is not a power of two in 2..64; stride < width; a negative offset;
 * mode outside -3..3; mode 0 in the inverse entry; non-zero rsv; a needed pointer that is NULL (d_resi; d_joint with any mode != 0; d_joint_rec; d_org_resi with d_sse);
 * stats_idx >= 0 with d_stats == NULL.
 * NOT done here (the caller's job): CABAC bit estimation and the lambda scaling of the joint mode (InterSearch.cpp:3846-3853), chroma transform skip candidates, the chroma
 * distortion weight.                                                                                                                                                       */
typedef struct
{
  int32_t cb_off, cr_off;   /* the TU's Cb / Cr block: sample offsets, row pitch `stride`                       */
  int32_t stride;
  int32_t joint_off;        /* the joint block, COMPACT (row pitch = width)                                      */
  int32_t stats_idx;        /* inverse only: index into d_stats, -1 = none                                       */
  int16_t width, height;    /* independent powers of two, 2..64                                                  */
  int8_t  mode;             /* signed ICT mode, -3..3                                                            */
  uint8_t rsv[3];           /* zero                                                                              */
} vvhip_ict_item;           /* 28 bytes */
VVHIP_API int vvhip_ict_fwd_batch( vvhip_ctx* ctx, const int16_t* d_resi, const vvhip_ict_item* items_host, int n,
                                   int16_t* d_joint /* may be NULL if every mode is 0 */, int64_t* d_dist /* 2 per item, may be NULL */ );
VVHIP_API int vvhip_ict_inv_batch( vvhip_ctx* ctx, const int16_t* d_joint_rec, const vvhip_ict_item* items_host, int n,
                                   const vvhip_tu_stats* d_stats /* may be NULL */, int16_t* d_rec /* may be NULL */,
                                   const int16_t* d_org_resi /* may be NULL */, uint64_t* d_sse /* 2 per item: Cb, Cr; may be NULL */ );

/* Sub-block transform (SBT) around the fused TU pipeline: the one residual tool of inter CUs that codes only ONE HALF or ONE QUARTER of the CU's residual, with
 * position-dependent DST-7 / DCT-8, and takes the rest as zero (InterSearch::xEstimateInterResidualQT with cu.sbtInfo; on in the reference's slow, slower and medium-low
 * presets).  A coded tile is an ordinary TU job on a sub-rectangle of the CU's residual — vvhip_tu_rdo_multi_strided reads it in place — so there are three pieces, all
 * data-parallel over a picture's CU list: parts, tiles, placement.  4:2:0 only: the chroma blocks are half size.
 * SBT mode 0..7 = SBT_VER_H0, SBT_VER_H1, SBT_HOR_H0, SBT_HOR_H1, SBT_VER_Q0, SBT_VER_Q1, SBT_HOR_Q0, SBT_HOR_Q1 (CommonLib/TypeDef.h:284-291) = 2 ( sbtIdx - 1 ) + sbtPos.
 * sbt_allowed = what CU::checkAllowedSbt returns (CommonLib/UnitTools.cpp:249-268): bit 1 SBT_VER_HALF (width >= 8), bit 2 SBT_HOR_HALF (height >= 8), bit 3 SBT_VER_QUAD
 * (width >= 16), bit 4 SBT_HOR_QUAD (height >= 16) — carried by the item and not derived, because the encoder also clears bits by picture width and size (EncCu.cpp:3797).
 *
 * vvhip_sbt_parts_batch = InterSearch::xCalcMinDistSbt (EncoderLib/InterSearch.cpp:3272-3464) for a list of CUs, bit for bit.  The CU's Y, Cb and Cr residual blocks sit at
 * y_off / cb_off / cr_off (sample offsets into d_resi) with row pitches stride_y / stride_c; org - pred of the reference IS that residual, and with
 * DISTORTION_PRECISION_ADJUSTMENT 0 (TypeDef.h:171) no bit depth is needed.  width / height (luma) independent powers of two, 4..64.  Every output pointer may be NULL:
 *   d_parts[n][3][16] : the UNWEIGHTED sum of squares of every part per component (Y, Cb, Cr), row-major [j][i] in a 4 x 4 frame; the grid has numPartX = width >= 16 ? 4 :
 *                       width == 4 ? 1 : 2 columns, rows likewise (:3291-3292); a chroma part is ( width / 2 ) / numPartX x ( height / 2 ) / numPartY, down to 2 x 2.
 *                       Cells outside the grid are zero.
 *   d_est[n][9]       : m_estMinDistSbt[0..8] as :3338-3425 leaves it — [8] the CU's total, a mode whose type is not allowed MAX_DISTORTION (all ones), the halves
 *                       ( resi >> 5 ) + noResi, the quads sum( own + ( others << 5 ) ) >> 5.  Every component's part sum is weighted on its own before the components are
 *                       added: luma as it is, chroma (uint64)( double( sum ) * chroma_weight ) — one IEEE multiplication, truncated toward zero (:3329-3333);
 *                       chroma_weight = RdCost::getChromaWeight() (RdCost.h:166).
 *   d_order[n][8]     : m_sbtRdoOrder as :3427-3463 leaves it — the min( 2 x allowed half types, SBT_NUM_RDO = 2 ) best half modes, then likewise the quad modes; strict <,
 *                       so a tie goes to the lower mode; unused entries 255.
 * NOT done here (the caller's job): items with sbt_allowed == 0 are an argument error — their plain SSE is a distortion list's; "fast algorithm 1" (:3353-3359,
 * m_skipSbtAll) needs lambda and is one comparison on d_est[i][8]; skipSbtByRDCost, the history-based initSbtRdoOrder and every CABAC bit.
 *
 * vvhip_sbt_tiles (host arithmetic, no context, nothing launched) = CU::getSbtTuSplit (UnitTools.cpp:3388), PartitionerImpl::getSbtTuTiling (CommonLib/UnitPartitioner.cpp:
 * 995-1056) and the SBT branch of TrQuant::xSetTrTypes (CommonLib/TrQuant.cpp:435-466): out[c], c = Y, Cb, Cr, is the CODED tile of the component block — tile 0 for
 * position 0, tile 1 for position 1 — with the factors ( dim * f ) >> 2 per component: where it lies inside the block ( x, y, width, height ), resi_off = the sample offset of
 * its corner and stride = the CU's pitch: one TU of a vvhip_tu_rdo_multi_strided job reads it in place.  The uncoded quad tile is three quarters of the CU, not a power of two,
 * and never transformed.  Luma types: vertical split DCT-8 / DST-7 (hor / ver) at position 0 and DST-7 / DST-7 at position 1, horizontal split DST-7 / DCT-8 at position 0
 * and DST-7 / DST-7 at position 1; DCT-2 / DCT-2 when the tile's side ALONG the split line — the height of a vertical split's tile, the width of a horizontal split's —
 * exceeds MTS_INTER_MAX_CU_SIZE (32); chroma always DCT-2.  Returns VVHIP_E_ARG for a mode outside 0..7, a size that is not a power of two in 4..64, a half mode on a side
 * below 8 or a quad mode on a side below 16.
 *
 * vvhip_sbt_place_batch: one item per CANDIDATE.  The CU's three blocks sit at y_off / cb_off / cr_off in d_rec and d_org_resi (the layout of the residual); per component
 * the compact reconstruction of the coded tile (row pitch = the tile's width: a TU job's d_rec_resi) sits at tile_off[c] in d_tile_rec, and stats_idx[c] names the TU's
 * statistics in d_stats.  Per component the entry writes the WHOLE block of d_rec — the coded tile from d_tile_rec, the other tile zero (tu.noResidual, InterSearch.cpp:3562,
 * :3758-3762) — and d_sse[3i + c] = the plain sum of squared differences of that block against d_org_resi, unweighted and unshifted like vvhip_tu_stats.sse: the tile's SSE
 * plus the energy of the zeroed part.  stats_idx[c] >= 0 with d_stats[stats_idx[c]].abs_sum == 0: the tile is ALL ZERO and d_tile_rec is not read, so the chain holds with
 * vvhip_tu_set_sparse_outputs on; stats_idx[c] == -1: the caller dropped that component's coefficients (cbf 0) — zero as well, tile_off[c] is ignored.
 *
 * Both list entries follow the joint Cb-Cr entries: items_host is a HOST array, sorted by the library into size classes (a wave never mixes classes, small CUs share a wave);
 * the device copy of that schedule stays in the context in slots of its own — the same list again uploads and allocates nothing, and alternating with the joint Cb-Cr and
 * prediction entries evicts none of theirs.  Accesses are vectors as wide as offsets, pitches, part / tile widths and base addresses allow (2..16 bytes); every sum is 64-bit,
 * reduced inside one wave and stored once — no atomics: results do not depend on the order of the list.  Nothing outside the named blocks is written.  Output blocks of
 * different items must not overlap.
 * Argument errors (VVHIP_E_ARG with a message naming the entry, nothing launched): n < 0; a size that is not a power of two in 4..64; a pitch below the width; a negative
 * offset; sbt_allowed == 0, or with a bit the size cannot have (bits outside 1..4, half types on a side below 8, quad types on a side below 16); non-zero rsv; a needed
 * pointer that is NULL (d_resi; d_org_resi with d_sse; d_stats or d_tile_rec with any stats_idx >= 0); a misaligned array; placement: mode outside 0..7, a mode whose type
 * bit is not in sbt_allowed, stats_idx below -1, a negative tile offset.
 * NOT done here (the caller's job): m_skipSbtAll, skipSbtByRDCost, the history order, bits and lambda, the chroma distortion weight of getDistPart, SBT combined with the MTS
 * candidates of the unsplit TU, 4:2:2 and 4:4:4.                                                                                                                            */
typedef struct
{
  int32_t y_off, cb_off, cr_off;   /* the CU's Y / Cb / Cr block: sample offsets                                  */
  int32_t stride_y, stride_c;      /* row pitches of the luma block and of both chroma blocks                     */
  int16_t width, height;           /* luma; independent powers of two, 4..64                                      */
  uint8_t sbt_allowed;             /* CU::checkAllowedSbt's bits, non-zero                                        */
  uint8_t rsv[3];                  /* zero                                                                        */
} vvhip_sbt_item;                  /* 28 bytes */
typedef struct
{
  int32_t resi_off, stride;        /* the coded tile's corner in the buffer of the CU's blocks, the CU's pitch    */
  int16_t x, y, width, height;     /* the coded tile inside the component block                                   */
  int8_t  tr_hor, tr_ver;          /* VVHIP_DCT2 / VVHIP_DCT8 / VVHIP_DST7                                        */
  uint8_t rsv[2];
} vvhip_sbt_tile;                  /* 20 bytes */
typedef struct
{
  int32_t y_off, cb_off, cr_off;   /* the CU's blocks in d_rec and d_org_resi                                     */
  int32_t stride_y, stride_c;
  int32_t tile_off[3];             /* per component: the coded tile's COMPACT reconstruction in d_tile_rec        */
  int32_t stats_idx[3];            /* per component: index into d_stats, -1 = no coefficients (all zero)          */
  int16_t width, height;
  uint8_t sbt_allowed;
  uint8_t mode;                    /* SBT mode 0..7                                                               */
  uint8_t rsv[2];                  /* zero                                                                        */
} vvhip_sbt_place_item;            /* 52 bytes */
VVHIP_API int vvhip_sbt_parts_batch( vvhip_ctx* ctx, const int16_t* d_resi, const vvhip_sbt_item* items_host, int n, double chroma_weight,
                                     uint64_t* d_parts /* n x 3 x 16, may be NULL */, uint64_t* d_est /* n x 9, may be NULL */, uint8_t* d_order /* n x 8, may be NULL */ );
VVHIP_API int vvhip_sbt_tiles( const vvhip_sbt_item* cu, int mode, vvhip_sbt_tile* out /* 3: Y, Cb, Cr */ );
VVHIP_API int vvhip_sbt_place_batch( vvhip_ctx* ctx, const int16_t* d_tile_rec /* may be NULL if no stats_idx >= 0 */, const vvhip_sbt_place_item* items_host, int n,
                                     const vvhip_tu_stats* d_stats /* may be NULL */, int16_t* d_rec /* may be NULL */,
                                     const int16_t* d_org_resi /* may be NULL */, uint64_t* d_sse /* 3 per item: Y, Cb, Cr; may be NULL */ );

/* ---- the g_tCoeffOps table slots one-to-one (CommonLib/TrQuant_EMT.h:63-91), device pointers, caller's matrix ------------------
 * vvhip_fast_fwd_core  <- fastFwdCore_2D/_1D[log2(tr_size)-2]  (TrQuant_EMT.cpp:1973-2000):
 *     dst[j*line + i] = ( sum_k src[i*tr_size + k] * tc[j*tr_size + k] + 2^(shift-1) ) >> shift,  i < reduced_line, j < cutoff
 * vvhip_fast_inv_core  <- fastInvCore[log2(tr_size)-2]         (:1953-1970): dst[i*tr_size + j] += sum_{k<rows} src[k*lines + i] * it[k*tr_size + j]
 *     (ACCUMULATES: the reference's caller zeroes dst first, :159)
 * vvhip_round_clip     <- roundClip4/8 (clipCore :1941-1950), vvhip_cpy_resi <- cpyResi4/8 (:1929-1938), vvhip_cpy_coeff <- cpyCoeff4/8 (:1917-1926).
 * The batched path uses the fused 2-D entries above; these give every slot of the table a device provider.                     */
VVHIP_API int vvhip_fast_fwd_core( vvhip_ctx* ctx, int tr_size, const int16_t* d_tc, const int32_t* d_src, int32_t* d_dst,
                                   unsigned line, unsigned reduced_line, unsigned cutoff, int shift );
VVHIP_API int vvhip_fast_inv_core( vvhip_ctx* ctx, int tr_size, const int16_t* d_it, const int32_t* d_src, int32_t* d_dst,
                                   unsigned lines, unsigned reduced_lines, unsigned rows );
VVHIP_API int vvhip_round_clip( vvhip_ctx* ctx, int32_t* d_dst, unsigned width, unsigned height, unsigned stride,
                                int32_t out_min, int32_t out_max, int32_t round, int32_t shift );
VVHIP_API int vvhip_cpy_resi( vvhip_ctx* ctx, const int32_t* d_src, int16_t* d_dst, ptrdiff_t stride, unsigned width, unsigned height );
VVHIP_API int vvhip_cpy_coeff( vvhip_ctx* ctx, const int16_t* d_src, ptrdiff_t stride, int32_t* d_dst, unsigned width, unsigned height );

/* ======================================================================================================================
 * SURVEY 8f rank 1 — sub-pel interpolation for fractional motion estimation / motion compensation
 * ====================================================================================================================== */
/* One pass of the separable interpolation on one block with the caller's taps: the table slots
 * InterpolationFilter::m_filterHor / m_filterVer [tap index][isFirst][isLast] (CommonLib/InterpolationFilter.h:113-114),
 * scalar core filter<N,isVertical,isFirst,isLast> (InterpolationFilter.cpp:356-441).  taps = 8, 6, 4 or 2 (bilinear); coeff_host is the
 * table ROW as the reference passes it (8 entries for 8 and 6 taps — the 6-tap core skips the first entry —, 4 for 4 taps).  */
VVHIP_API int vvhip_if_filter( vvhip_ctx* ctx, int taps, int is_vertical, int is_first, int is_last, int bit_depth,
                               const int16_t* d_src, int src_stride, int16_t* d_dst, int dst_stride, int width, int height,
                               const int16_t* coeff_host );
/* m_filterCopy[isFirst][isLast] (InterpolationFilter.h:115, filterCopy :255-333). */
VVHIP_API int vvhip_if_copy( vvhip_ctx* ctx, int is_first, int is_last, int bit_depth,
                             const int16_t* d_src, int src_stride, int16_t* d_dst, int dst_stride, int width, int height, int bi_mc_for_dmvr );

/* A sub-pel candidate: original block at org_off, reference block whose integer position is ref_off, vector fraction in 1/16 sample. */
typedef struct { int32_t org_off, ref_off; int16_t frac_x, frac_y; } vvhip_subpel_item;

/* Motion-compensated luma prediction blocks (compact, d_out[i*w*h + y*w + x]): the passes InterPredInterpolation::xPredInterBlk runs
 * (CommonLib/InterPrediction.cpp:832-865; no BDOF/DMVR) — frac_y == 0: horizontal only, frac_x == 0: vertical only, else horizontal
 * (14-bit intermediate) then vertical.  rnd_res = !bi (InterPrediction.cpp:775): 1 = final samples clipped to the bit depth, 0 = the
 * 14-bit intermediate a bi-prediction average consumes.
 * filter_mode 0: the motion-compensation taps (8-tap m_lumaFilter; 6-tap m_lumaFilter4x4 for 4x4 blocks);
 *             1 / 2: the reduced sets of the fast sub-pel search (m_meReduceTap 1 / 2: m_lumaFilter4x4 / m_chromaFilter[frac << 1],
 *             InterpolationFilter.cpp:586-593).  use_alt_hpel: m_lumaAltHpelIFilter at phase 8 (IMV_HPEL).                       */
VVHIP_API int vvhip_interp_luma_batch( vvhip_ctx* ctx, const int16_t* d_ref, int ref_stride, const vvhip_subpel_item* d_items, int n,
                                       int width, int height, int bit_depth, int rnd_res, int filter_mode, int use_alt_hpel,
                                       int16_t* d_out );

/* What InterSearch::xPatternRefinement computes per tested position (EncoderLib/InterSearch.cpp:850-873, minus the MV-bit cost the
 * host adds): distortion (func = VVHIP_DF_SAD / _HAD / _HAD_FAST / _SSE, subShift 0) between the original block and the block
 * interpolated at the candidate's fractional vector.  One call = all sub-pel candidates of a stage for many blocks.               */
VVHIP_API int vvhip_subpel_dist_batch( vvhip_ctx* ctx, int func, const int16_t* d_org, int org_stride, const int16_t* d_ref, int ref_stride,
                                       int width, int height, int bit_depth, int filter_mode, int use_alt_hpel,
                                       const vvhip_subpel_item* d_items, int n, uint64_t* d_out );

/* Pattern refinement in one call: for every block, n_offsets sub-pel positions around ITS base vector (d_bases[b]: original block, integer
 * position and fraction of the base vector) — candidate k is base + offsets_host[k] (dx, dy in 1/16 sample, |.| <= 16) —
 *   d_out[b * n_offsets + k] = distortion( original block, block interpolated at candidate k )       (func as vvhip_subpel_dist_batch)
 * i.e. one stage of InterSearch::xPatternRefinement (EncoderLib/InterSearch.cpp:760-880: the 8 half-sample neighbours, then the 8
 * quarter-sample neighbours) for many blocks.  Same values as vvhip_subpel_dist_batch on the expanded candidate list; the reference
 * window is staged in LDS once per block and the horizontal pass is shared between positions with the same
 * horizontal offset; the distortion kernels then score the prediction blocks.  width a multiple of 8, blocks up to 64x64; the
 * reference plane needs 5 samples of margin beyond every block.                                                                                                       */
VVHIP_API int vvhip_subpel_refine_batch( vvhip_ctx* ctx, int func, const int16_t* d_org, int org_stride, const int16_t* d_ref, int ref_stride,
                                         int width, int height, int bit_depth, int filter_mode, int use_alt_hpel,
                                         const vvhip_subpel_item* d_bases, int n_blocks, const int16_t* offsets_host, int n_offsets, uint64_t* d_out );

/* ======================================================================================================================
 * Motion-search plans (round 3): what ONE picture's inter search pushes through the distortion tables, in ONE launch.
 * Built for work lists with the shape the encoder really produces (recorded from it, vvenc_amd/recorded.py): per InterSearch::xMotionEstimation call
 * (EncoderLib/InterSearch.cpp:1976-2130) ~20 integer candidates inside a few samples of each other (start points, 4-point diamond + square at distance 1,
 * :2385-2410) followed by one or two xPatternRefinement stages (:760-880) of <= 9 sub-pel positions around the winner; blocks 4..64 square at the fast presets (most sample pairs in
 * 64x64 blocks), rectangular 4..128 at preset medium; plus merge / AMVP / intra / residual distortions on compact prediction blocks.
 *   integer job  : the block's candidate positions as displacements from ref_off; the kernel stages the candidates' bounding window of the reference plane in
 *                  LDS once (samples biased for v_sad_u16; odd displacements are taken from the even dword below with v_alignbit) and scores all candidates from it.
 *                  cost[first_cand + i] = xGetSAD*( org block, ref block at (dx_i, dy_i) ) incl. the subShift rule (RdCost.cpp:301-644).
 *   stage job    : position k (k = 0..8, evaluated when bit k of mask is set) lies ( refine[k] + (base_qx, base_qy) ) * i_frac quarter samples from the block at
 *                  ref_off, refine = s_acMvRefineH (i_frac 2) / s_acMvRefineQ (i_frac 1) (InterSearch.cpp:67-91).  The kernel interpolates like
 *                  xPatternRefinement's planes (filter_mode / alt_hpel as vvhip_interp_luma_batch; horizontal pass shared between positions) and scores each
 *                  prediction against the original block directly from LDS — the predictions never exist in HBM.  cost[9 * stage + k] as the table entry
 *                  `func` (VVHIP_DF_SAD / _HAD / _HAD_FAST) returns it; positions outside the mask read 0 (every stage's nine costs are written by every run).
 *                  Every evaluated position must lie within one sample of the block at ref_off vertically and horizontally ((refine + base) * i_frac in -4..4
 *                  quarter samples): the kernel stages exactly that neighbourhood; plan creation rejects anything else.
 *   item         : one plain table call: func on (org block, cur block) of any two planes / pools of the plan's plane table.
 *   masked item  : DF_SAD_WITH_MASK (xGetSADwMask, RdCost.cpp:2062-2093: GEO partitions of preset medium and slower): sum |org - cur| * mask over the rows the
 *                  subShift rule keeps, << subShift.  The mask block is COMPACT (row pitch = width, one row per evaluated row: the caller has applied the
 *                  reference's stepX / maskStride / maskStride2 walk).  Its costs follow the plain items': d_item_cost[n_items + i].
 * Offsets are in samples from sample (0,0) of the job's plane (negative = margin); planes must be readable 16 bytes beyond every block row they hold, and 18 bytes beyond
 * every row of an integer job's window (the candidates' bounding box + the block: a row of winW samples is fetched as ( winW + 2 + 7 ) / 8 chunks of 16 bytes from its
 * first sample, i.e. up to 9 samples further when winW = 7 mod 8).
 * A plane table entry with stride 0 is a pool of COMPACT blocks: the row pitch of a block read from it is the block's own width.
 * Shapes (round 4: everything preset medium's CTU 128 + multi-type tree produces): width and height independent powers of two — integer jobs 8..128 x 4..128,
 * stage jobs 4..128 x 4..128 (not 4x4), items 2..128 x 2..128; the Hadamard family follows the reference's tile ladder (16x8, 8x16, 8x4, 4x8 with the
 * double-precision normalisation, 16x16_fast, 8x8, 4x4, 2x2: RdCost.cpp:1818-1938); bit depths <= 10 (the packed Hadamard tile, like the reference's x86 rows).
 * Operand ranges of the Hadamard family (stage jobs and items): what the encoder hands to these table entries at the plan's bit depth — samples in [0, 2^bit_depth) or
 * bi-prediction patterns 2 org - pred in (-2^bit_depth, 2^(bit_depth+1)) against prediction samples, i.e. |org - cur| < 2^(bit_depth+1): the first two butterfly stages run on
 * packed 16-bit pairs.  SAD / SSE / masked-SAD items take any int16 operands (masked SADs: weights >= 0; sums in 64 bits outside the GEO range of samples and weights).
 * Operand range of integer jobs: ANY int16 values in both planes, -32768 .. 32767 (samples, bi-prediction patterns and beyond).  The window kernel flips the sign bit of
 * both operands ( x ^ 0x8000 = x + 32768 as uint16: order and differences are kept ), v_sad_u16 adds |a - b| of the unsigned halves into a 32-bit sum per lane, the team's
 * sums are added in 32 bits and shifted by sub_shift in 64: exact up to 128 * 128 * 65535 < 2^32 (tests/test_gpu_me_plan_extremes.py, family F, at both ends of the range).
 * Limits: fewer than 2^24 candidates and 2^22 stage jobs per plan.
 * Integer jobs: positions a job lists more than once (the search re-scores its start point) are scored once; every listed candidate still gets its cost.
 * A plan owns device copies of the job tables and the schedule derived from them (which wave takes which jobs, heaviest first); running it is one launch per kind.
 * ====================================================================================================================== */
typedef struct { const int16_t* d_base; int32_t stride; int32_t reserved; } vvhip_me_plane;
typedef struct { int32_t org_off, ref_off; int16_t width, height; uint8_t org_plane, ref_plane, sub_shift, reserved; int16_t min_dx, min_dy, win_w, win_h; int32_t first_cand, n_cand; } vvhip_me_int_job;
typedef struct { int16_t dx, dy; } vvhip_me_cand;
typedef struct { int32_t org_off, ref_off; int16_t width, height; uint8_t org_plane, ref_plane, i_frac, filter_mode, alt_hpel, func; int8_t base_qx, base_qy; uint16_t mask; uint16_t reserved; } vvhip_me_stage_job;
typedef struct { int32_t org_off, cur_off; uint8_t org_plane, cur_plane, func, sub_shift; int16_t width, height; } vvhip_me_item;
typedef struct { int32_t org_off, cur_off, mask_off; uint8_t org_plane, cur_plane, mask_plane, sub_shift; int16_t width, height; int32_t reserved; } vvhip_me_mask_item;
typedef struct
{
  const vvhip_me_int_job* int_jobs; int32_t n_int_jobs; const vvhip_me_cand* cands; int32_t n_cands;
  const vvhip_me_stage_job* stage_jobs; int32_t n_stage_jobs; const vvhip_me_item* items; int32_t n_items;
  const vvhip_me_mask_item* mask_items; int32_t n_mask_items;
} vvhip_me_lists;
typedef struct vvhip_me_plan vvhip_me_plan;
/* all job arrays are HOST arrays (copied); any of the three lists may be empty.  win_* / min_* of an integer job may be left 0: the library derives the window from the candidates
 * and splits jobs whose candidates spread further than max_window samples (0: default 24) into several windows. */
VVHIP_API int  vvhip_me_plan_create( vvhip_ctx* ctx, const vvhip_me_int_job* int_jobs, int n_int_jobs, const vvhip_me_cand* cands, int n_cands,
                                     const vvhip_me_stage_job* stage_jobs, int n_stage_jobs, const vvhip_me_item* items, int n_items,
                                     int bit_depth, int max_window, vvhip_me_plan** out );
/* the same with every list in one record (adds the masked items) */
VVHIP_API int  vvhip_me_plan_create_lists( vvhip_ctx* ctx, const vvhip_me_lists* lists, int bit_depth, int max_window, vvhip_me_plan** out );
VVHIP_API void vvhip_me_plan_destroy( vvhip_ctx* ctx, vvhip_me_plan* plan );
/* planes_host: the plan's plane table for THIS run (<= 16 entries; device pointers to sample (0,0)).  d_cand_cost: n_cands, d_stage_cost: 9 * n_stage_jobs,
 * d_item_cost: n_items + n_mask_items Distortion values; pointers of empty lists may be NULL.                                                               */
VVHIP_API int  vvhip_me_plan_run( vvhip_ctx* ctx, const vvhip_me_plan* plan, const vvhip_me_plane* planes_host, int n_planes,
                                  uint64_t* d_cand_cost, uint64_t* d_stage_cost, uint64_t* d_item_cost );
/* the same, restricted to some of the plan's three independent parts (bit 0: refinement stages, bit 1: integer windows, bit 2: table calls): a caller with several
 * contexts / streams issues the parts on different streams so that they share the device (bench.py) */
VVHIP_API int  vvhip_me_plan_run_parts( vvhip_ctx* ctx, const vvhip_me_plan* plan, const vvhip_me_plane* planes_host, int n_planes,
                                        uint64_t* d_cand_cost, uint64_t* d_stage_cost, uint64_t* d_item_cost, int parts );
/* per-kernel HIP events inside vvhip_me_plan_run (measurements: bench.py's roofline): with timing on, vvhip_me_plan_last_times waits for the last run and returns the
 * milliseconds of its parts — [0] refinement-stage kernel(s), [1] integer windows (both LDS classes: one launch), [2] 0 (was: the small
 * windows' own launch), [3] table calls. */
VVHIP_API int  vvhip_me_plan_set_timing( vvhip_ctx* ctx, vvhip_me_plan* plan, int on );
VVHIP_API int  vvhip_me_plan_last_times( vvhip_ctx* ctx, const vvhip_me_plan* plan, float* ms4_host );
/* what the schedule looks like (for measurements): waves per list and LDS bytes per wave */
VVHIP_API int  vvhip_me_plan_info( const vvhip_me_plan* plan, int* waves_int, int* waves_stage, int* waves_item, int* lds_bytes );

/* ======================================================================================================================
 * Inter prediction of a LIST of prediction units: what InterPredInterpolation::xPredInterBlk + xWeightedAverage produce for one component block of one PU
 * (CommonLib/InterPrediction.cpp:768-867, :960-1010), for a picture's worth of blocks of MIXED sizes in ONE launch — luma and 4:2:0 chroma, uni- and bi-predicted —
 * and, on request, the residual against the original.  A picture-level entry like the plans: the caller has the vectors (DMVR results, merge candidates, the winners of a
 * motion-search plan) and hands over the list; no per-PU call site of the encoder is involved.
 *   item      : one component block.  width / height independent powers of two, luma 4..128, chroma 2..64.  Per reference list l (ref_plane[l] = index into the plane
 *               table, -1 = list not used): ref_off[l] = the block's integer position ( mv >> shift ) in that plane, frac[l] = ( x, y ) fraction — 1/16 sample for luma,
 *               1/32 for 4:2:0 chroma (shiftHor = MV_FRACTIONAL_BITS_INTERNAL + 1, :777-785).
 *   luma      : the passes of vvhip_interp_luma_batch with filter_mode 0 — 8-tap m_lumaFilter, m_lumaFilter4x4 for 4x4 blocks, m_lumaAltHpelIFilter at phase 8 with
 *               alt_hpel (IMV_HPEL); horizontal only / vertical only / both with the 14-bit intermediate.
 *   chroma    : 4-tap m_chromaFilter, vFilterSize = NTAPS_CHROMA (:860-865): horizontal pass over height + 3 rows starting one row above the block, then vertical.
 *   one list  : rndRes = 1 — final samples clipped to the bit depth.
 *   two lists : both interpolated to the 14-bit intermediate (rndRes = 0), then the default weighted average AreaBuf<Pel>::addAvg (CommonLib/Buffer.cpp:549-575, core
 *               :129-141): ClipPel( ( a + b + offset ) >> shiftNum ), shiftNum = max( 2, IF_INTERNAL_PREC - bitDepth ) + 1, offset = ( 1 << ( shiftNum - 1 ) ) + 2 * IF_INTERNAL_OFFS.
 *               The two intermediates never leave the compute unit.
 *   output    : pred_stride == 0: compact blocks (row pitch = width) at d_pred + dst_off; pred_stride > 0: the block's position dst_off in a plane of that row pitch.
 *   residual  : with d_org and d_resi given, org - pred (int16) is written to d_resi in the layout of the prediction (same dst_off, same pitch): compact blocks one
 *               after the other are directly a d_resi of vvhip_tu_rdo_multi_strided with resi_strides_host[i] = width; with pred_stride > 0 a residual plane for
 *               vvhip_tu_rdo_multi.  The original block sits at d_org + org_off, row pitch org_stride (one pitch per call: the components of a picture buffer
 *               allocated with one pitch, or one call per component).
 * items_host is a HOST array: the library sorts it into size classes (a wave never mixes shapes; small blocks share a wave — sixteen 4x4 luma blocks, thirty-two 2x2
 * chroma blocks), cuts large blocks into tiles, deals the workgroups to the XCDs in horizontal picture bands and keeps the device copy of that schedule in the context — running the
 * same list again (same items, same plane table) uploads nothing and allocates nothing.  Results do not depend on the order of the list.  Items must not overlap in the output.
 * Margins: every reference plane must be readable 4 (luma) / 2 (chroma) samples beyond the block on all sides plus 16 bytes behind the last row touched (the window is
 * fetched as aligned dwords), and needs an even row pitch; a zero fraction reads no rows above / below the block.
 * Unsupported input (a size that is not a power of two or out of range, a plane index outside the table, both lists unused, a fraction out of range) returns VVHIP_E_ARG with a
 * message before anything is launched.
 * BDOF and the padded-reference rule of DMVR (DMVR::xFinalPaddedMCForDMVR, CommonLib/InterPrediction.cpp:1189-1225: a refined sub-block's final prediction reads a padded
 * copy of its PREFETCHED window, not the true plane) are per-item extensions: vvhip_pred_inter_batch_ex below.  Without them this entry is exact for DMVR sub-blocks whose
 * refinement is zero and for every PU BDOF does not apply to.
 * Affine CUs with PROF have an entry of their own that takes the control-point vectors: vvhip_pred_affine_batch below.
 * BCW's block weights and GEO's per-sample blending of two hypotheses are per-item blend records: vvhip_pred_inter_batch_blend below.
 * CIIP's planar intra part and its weighting are per-item CIIP records: vvhip_pred_inter_batch_ciip below.
 * NOT done here (the caller's job, as before): explicit weighted prediction (slice-level weight tables); IBC; CIIP in a picture with LMCS active (the forward luma mapping
 * before the weighting); reference picture resampling; the chroma phases of 4:2:2 and 4:4:4.
 * ====================================================================================================================== */
typedef struct
{
  int32_t dst_off;            /* sample offset of the block in d_pred (and in d_resi)                                  */
  int32_t org_off;            /* the block in the original plane (residual only)                                       */
  int32_t ref_off[2];         /* integer position ( mv >> shift ) in the reference plane, per list                     */
  int16_t frac[2][2];         /* ( x, y ) fraction per list: 1/16 sample luma, 1/32 chroma                             */
  int16_t width, height;
  int8_t  ref_plane[2];       /* index into the plane table, -1 = list not used                                        */
  uint8_t chroma;             /* 0: luma taps, 1: chroma taps                                                          */
  uint8_t alt_hpel;           /* luma: m_lumaAltHpelIFilter at phase 8                                                 */
} vvhip_pred_item;            /* 32 bytes */
VVHIP_API int vvhip_pred_inter_batch( vvhip_ctx* ctx, const vvhip_me_plane* planes_host, int n_planes /* <= 16, as vvhip_me_plan_run takes it (stride > 0) */,
                                      const vvhip_pred_item* items_host, int n, int bit_depth,
                                      int16_t* d_pred, int pred_stride,
                                      const int16_t* d_org /* may be NULL */, int org_stride, int16_t* d_resi /* may be NULL */ );
/* The same entry with a per-item extension (ext_host: a HOST array parallel to items_host; NULL = exactly vvhip_pred_inter_batch):
 *   VVHIP_PRED_EXT_BDOF     : bi-directional optical flow on a true bi-predicted luma block (InterPrediction.cpp:465-490, xSubPuBDOF :326-357, xPredInterBlk :822-831 +
 *               :868-901, xApplyBDOF :911-958, gradFilterCore :114-155, calcBDOFSumsCore :157-186, xFpBiDirOptFlowCore :607-661, addBDOFAvgCore :63-86).  Any luma size
 *               8..128 with min( w, h ) >= 8 and w * h >= 128; the library cuts the block into the 16x16 / 16x8 / 8x16 units the reference predicts on their own (each
 *               with its own one-sample ring of integer samples and its own replication padding).  The conditions on POC distances and CU flags (SMVD, BCW, CIIP, affine)
 *               are the caller's; the chroma blocks of such a PU are plain bi-predicted items.
 *   VVHIP_PRED_EXT_DMVR_PAD : the padded-reference rule of DMVR's final motion compensation (xCopyAndPad :1088-1130, xFinalPaddedMCForDMVR :1189-1225) for one refined
 *               sub-block (<= 16x16 luma, its chroma blocks likewise).  ref_off[l] / frac[l] describe the REFINED vector; pad_dx / pad_dy[l] = refined_int - start_int
 *               per list (|.| <= 2 luma, <= 1 chroma), so ref_off[l] - ( pad_dy[l] * stride + pad_dx[l] ) is the start position.  Every sample the block reads (the BDOF
 *               ring included) has its coordinates clamped to the window prefetched around the start vector: ( w + T - 1 ) x ( h + T - 1 ) samples from
 *               start - ( T / 2 - 1 ), T = 8 luma / 4 chroma — what reading the replication-padded copy gives.  A zero delta reads the true plane.
 *               With both flags the item is one BDOF unit (<= 16x16); the caller sets the BDOF flag per sub-block as its own flag AND min_cost >= 2 * dx * dy (:1307, :1384).
 * Argument errors (VVHIP_E_ARG with a message, nothing launched): BDOF on chroma, with one list or on a size that fails the rule; a delta out of range; unknown flag bits or
 * non-zero reserved bytes.  Everything vvhip_pred_inter_batch promises holds: order independence, the schedule cache (the extension array is part of the list's key),
 * the residual, both output layouts.  Margins: the BDOF ring lies one sample beyond the block, inside the 4-sample luma margin; a DMVR item reads inside the margin
 * of its START position.
 * Bit depths 8..12.  Compared with the reference at 8, 10 and 12 bits (the reference's own xApplyBDOF on recorded frames, scalar and x86 row; the interpolation from the
 * compiled reference).  Operand ranges established on planes of samples in [0, 2^bit_depth) (tests/test_oracle_pred_ext_extremes.py): the 14-bit block of a list within
 * +-25 100 while its ring stays in [-8192, 8191]; |gradient| up to 519 (255 if the block were in the ring's range), |dI| up to 3135 (1023), |b| up to 16 425; tmpx and tmpy
 * take every value of -15..15; the value in front of the (int16_t) cast and the final clip stays inside int16, so the cast never acts on frames made from planes; under
 * VVHIP_PRED_EXT_DMVR_PAD every ring sample already lies inside the clamp window (|delta| <= 2 against a reach of 3).                                                     */
#define VVHIP_PRED_EXT_BDOF     1
#define VVHIP_PRED_EXT_DMVR_PAD 2
typedef struct
{
  uint8_t flags;              /* VVHIP_PRED_EXT_*                                                                      */
  int8_t  pad_dx[2];          /* per list: refined_int - start_int, x (DMVR_PAD only)                                  */
  int8_t  pad_dy[2];          /* per list: refined_int - start_int, y                                                  */
  uint8_t rsv[3];             /* zero                                                                                  */
} vvhip_pred_ext;             /* 8 bytes */
VVHIP_API int vvhip_pred_inter_batch_ex( vvhip_ctx* ctx, const vvhip_me_plane* planes_host, int n_planes, const vvhip_pred_item* items_host,
                                         const vvhip_pred_ext* ext_host /* may be NULL */, int n, int bit_depth,
                                         int16_t* d_pred, int pred_stride,
                                         const int16_t* d_org /* may be NULL */, int org_stride, int16_t* d_resi /* may be NULL */ );
/* The same entry with a per-item blend record (blend_host: a HOST array parallel to items_host; NULL = exactly vvhip_pred_inter_batch_ex).  BCW and GEO are one arithmetic
 * on the two 14-bit intermediates:  ClipPel( ( w0 * s0 + ( 8 - w0 ) * s1 + offset ) >> shift ), shift = max( 2, IF_INTERNAL_PREC - bitDepth ) + 3,
 * offset = ( 1 << ( shift - 1 ) ) + ( IF_INTERNAL_OFFS << 3 ).
 *   VVHIP_PRED_BLEND_DEFAULT : the item is what it is without a blend record (its extension record, if any, applies).
 *   VVHIP_PRED_BLEND_BCW     : AreaBuf<Pel>::addWeightedAvg (CommonLib/Buffer.cpp:509-546, core :143-156), getBcwWeight (Rom.cpp:1150-1163): param = bcw_idx 0..4,
 *               w1 = { -2, 3, 4, 5, 10 }[bcw_idx], w0 = 8 - w1 for the whole block.  Every size the entry takes, luma and chroma; bcw_idx 2 is exactly the default average.
 *   VVHIP_PRED_BLEND_GEO     : InterpolationFilter::xWeightedGeoBlk (CommonLib/InterpolationFilter.cpp:1005-1064, tables Rom.cpp:1304-1382): param = geoSplitDir 0..63.
 *               The item is a WHOLE component block of the CU: luma w, h in { 8, 16, 32, 64 } (all 16 combinations), a 4:2:0 chroma item 4..32 per side with the CU's luma
 *               size taken as twice the item's.  ref_plane[k] / ref_off[k] / frac[k] describe partition k's hypothesis (which reference list it comes from does not matter);
 *               both are interpolated as uni-directional hypotheses to the 14-bit intermediate (InterPrediction.cpp:441, :1001-1004) and w0 = the weight mask at the sample.
 *               The host reduces split direction + CU size to three integers per item and the kernel derives each weight from them (no weight table or block on the device);
 *               vvhip_get_geo_weights_host returns the same weights.
 * A BCW or GEO item uses BOTH hypotheses.  The CU-level conditions are the caller's, as with BDOF: BCW's size rule, maxDim < 8 * minDim for GEO (EncCu.cpp:1946).
 * Argument errors (VVHIP_E_ARG with a message naming this entry, nothing launched): unknown mode; param out of range; non-zero rsv; a BCW or GEO item with one hypothesis;
 * a GEO size outside the set above; BCW or GEO on an item whose extension record carries VVHIP_PRED_EXT_BDOF or VVHIP_PRED_EXT_DMVR_PAD (the reference excludes both:
 * InterPrediction.cpp:478, :975).  Everything vvhip_pred_inter_batch promises holds: order independence, both output layouts, the residual, the schedule cache — the blend
 * array is part of the list's key, and a list with a blend array keeps a schedule of its own: alternating with vvhip_pred_inter_batch[_ex] and vvhip_pred_affine_batch on one
 * context evicts none of the three.
 * CIIP has a record of its own: vvhip_pred_inter_batch_ciip below.  Still the caller's: explicit weighted prediction, IBC.
 * Bit depths 8..12; compared with the reference's addWeightedAvg / xWeightedGeoBlk (scalar and x86 row) at 8, 10 and 12 bits, on 0 / max checkerboards at half-sample
 * fractions where the weights -2 / 10 drive both clip ends.                                                                                                              */
#define VVHIP_PRED_BLEND_DEFAULT 0   /* exactly what the item does without a blend record     */
#define VVHIP_PRED_BLEND_BCW     1   /* param = bcw_idx 0..4                                  */
#define VVHIP_PRED_BLEND_GEO     2   /* param = geoSplitDir 0..63                             */
typedef struct { uint8_t mode, param, rsv[2]; } vvhip_pred_blend;   /* 4 bytes, rsv zero */
VVHIP_API int vvhip_pred_inter_batch_blend( vvhip_ctx* ctx, const vvhip_me_plane* planes_host, int n_planes, const vvhip_pred_item* items_host,
                                            const vvhip_pred_ext* ext_host /* may be NULL */, const vvhip_pred_blend* blend_host /* may be NULL */, int n, int bit_depth,
                                            int16_t* d_pred, int pred_stride,
                                            const int16_t* d_org /* may be NULL */, int org_stride, int16_t* d_resi /* may be NULL */ );
/* The same entry with a per-item CIIP record (ciip_host: a HOST array parallel to items_host; NULL = exactly vvhip_pred_inter_batch_blend) and the intra reference samples
 * of the CIIP items (d_intra_ref: a DEVICE array, like the planes — its contents may change between runs of one list; neither they nor its address belong to the list's key).
 *   VVHIP_PRED_CIIP_OFF : the item is what it is without a CIIP record.
 *   VVHIP_PRED_CIIP_ON  : the item is a WHOLE component block of a CIIP CU (EncCu.cpp:1926, :2213-2219): luma w, h in 4..64 with w * h >= 64; a 4:2:0 chroma block 4..32
 *               wide and 2..32 high with w * h >= 16.  Its inter part is the item's FINAL clipped sample — one list, the default average, or BCW through its blend record
 *               (InterPrediction.cpp:973) — and the result is weightCiipCore (CommonLib/Buffer.cpp:60-81): ( wI * intra + ( 4 - wI ) * inter + 2 ) >> 2, wI = num_intra + 1,
 *               not clipped.  num_intra 0..2 is getNumIntraCiip (IntraPrediction.h:176-188), computed by the caller.
 *   intra     : IntraPrediction::predIntraAng with PLANAR_IDX (CommonLib/IntraPrediction.cpp:353-383).  d_intra_ref + ref_off holds top[0 .. w + 2] followed by
 *               left[0 .. h + 2] — w + h + 6 samples in [0, 2^bit_depth), top[0] == left[0] the corner: the UNFILTERED samples of the two rows xFillReferenceSamples (:755)
 *               leaves, neighbour availability and substitution done by the caller.  Nothing outside them is read.  Luma lines are smoothed with
 *               ( u[i-1] + 2 u[i] + u[i+1] + 2 ) >> 2 (xFilterReferenceSamples :994-1030; refFilterFlag :473-476 holds for every CIIP luma block), chroma lines are not
 *               (:461-468); then xPredIntraPlanar_Core (:79-135) and, where min( w, h ) >= 4 (:426), the PDPC of IntraPredSampleFilter_Core (:137-157) on the same line.
 *               Blocks larger than a tile are cut as always; planar and PDPC are evaluated in block coordinates.
 * Argument errors (VVHIP_E_ARG with a message naming this entry, nothing launched): unknown mode; num_intra > 2; non-zero rsv; a negative ref_off; a size outside the sets
 * above; CIIP on a GEO item; CIIP on an item whose extension record carries VVHIP_PRED_EXT_BDOF or VVHIP_PRED_EXT_DMVR_PAD (InterPrediction.cpp:468, UnitTools.cpp:1309);
 * d_intra_ref == NULL while any record is ON.  Everything vvhip_pred_inter_batch promises holds: order independence, both output layouts, the residual (taken from the CIIP
 * result), the schedule cache — the CIIP array is part of the list's key, and a list with a CIIP array keeps a schedule of its own: alternating with
 * vvhip_pred_inter_batch[_ex], vvhip_pred_inter_batch_blend and vvhip_pred_affine_batch on one context evicts none of them.
 * Still the caller's: explicit weighted prediction, IBC, and CIIP in a picture with LMCS active (the forward luma mapping of the inter part before the weighting); of CIIP
 * itself the CU-level conditions, the reference line and num_intra.
 * Bit depths 8..12; compared with the reference's planar prediction, PDPC and weightCiip (scalar and x86 row) at 8, 10 and 12 bits, with lines all 0, all 2^bit_depth - 1
 * and alternating, and with an inter part whose clip acts at both ends.                                                                                                   */
#define VVHIP_PRED_CIIP_OFF 0   /* exactly what the item does without a CIIP record      */
#define VVHIP_PRED_CIIP_ON  1   /* ref_off, num_intra as above                           */
typedef struct { int32_t ref_off; uint8_t mode, num_intra, rsv[2]; } vvhip_pred_ciip;   /* 8 bytes, rsv zero */
VVHIP_API int vvhip_pred_inter_batch_ciip( vvhip_ctx* ctx, const vvhip_me_plane* planes_host, int n_planes, const vvhip_pred_item* items_host,
                                           const vvhip_pred_ext* ext_host /* may be NULL */, const vvhip_pred_blend* blend_host /* may be NULL */,
                                           const vvhip_pred_ciip* ciip_host /* may be NULL */, const int16_t* d_intra_ref /* may be NULL without an ON record */,
                                           int n, int bit_depth, int16_t* d_pred, int pred_stride,
                                           const int16_t* d_org /* may be NULL */, int org_stride, int16_t* d_resi /* may be NULL */ );
/* Inter prediction of a LIST of AFFINE CUs from their control-point vectors: what InterPredInterpolation::xPredAffineBlk (CommonLib/InterPrediction.cpp:1497-1839) + the
 * default weighted average produce for one component block of one affine CU, PROF included, bit-exact.  One item is one component block; the CU record is all that
 * crosses to the device — the sub-block vectors, fractions and PROF's dMv table are derived in the kernel.
 *   model     : iDMvHor = ( RT - LT ) << ( 7 - log2 cu_w ); iDMvVer from LB (six_param) or ( -iDMvHorY, iDMvHorX ); base LT << 7 (:1528-1542).  Chroma uses the luma quantities.
 *   luma 4x4  : the value at the sub-block's centre ( 2 + w, 2 + h ), or at the CU's centre for every sub-block when isSubblockVectorSpreadOverLimit (:1457-1495) holds —
 *               its predType is 3 when both lists are used, else the one list's interDir; the rule branches on 3 only —, roundAffineMv( ., 7 ) (Mv.cpp:61-66), the 18-bit
 *               storage clip: the stored vector.  Then the picture clip [ ( -ctu_size - 8 - cu_x + 1 ) << 4, ( pic_width + 8 - cu_x - 1 ) << 4 ], likewise vertically
 *               (:1545-1550, :1725-1726); position >> 4, fraction & 15.
 *   chroma 4x4: the stored vectors of its top-left and bottom-right luma sub-blocks summed, roundAffineMv( ., 1 ), the same clip in luma units, >> 5 / & 31 (:1729-1765).
 *   taps      : as a 4x4 luma / 4x4 chroma item of vvhip_pred_inter_batch (m_lumaFilter4x4, m_chromaFilter): filter4x4 / filterHor / filterVer; isLast = !bi && !PROF.
 *   prof      : luma only, decided per list.  0: off.  1: on unless the list's control points are all equal (:1557) or the spread is over the limit (:1558) — the conditions
 *               the library evaluates itself.  2 / 3: additionally the search-time rule of :1559-1560 (m_encOnly && !checkLDC) with threshold 1 << 7 / 1 << 8: on only when a
 *               model delta exceeds it.  The other conditions (SPS / picture-header flags, m_skipPROF, equal picture sizes) are the caller's.  When on, per sub-block: the dMv
 *               table (:1583-1630: roundAffineMv( ., 8 ), clip to +-31), the 14-bit block inside a one-sample ring ( ref << shift ) - 8192 at the position rounded by
 *               frac >> 3 (:1797-1820), gradFilterCore<false> (:113-131), applyPROFCore (:88-111: dI clipped to 1 << max( bit_depth + 1, 13 ), stored as a sample before the
 *               rounding, no rounding when bi).
 *   two lists : each to the 14-bit block (with its own PROF decision), then the default average of vvhip_pred_inter_batch.  BDOF never applies to affine CUs; BCW is the caller's.
 *   output, residual, plane table: as vvhip_pred_inter_batch; a compact block's row pitch is the component block's width ( cu_w >> chroma ).
 * items_host is a HOST array.  The library keeps a device schedule of its own for this entry (CU records + one 8-byte record per tile of sixteen sub-blocks; own key, buffer and
 * event): the same list again uploads nothing, and alternating with vvhip_pred_inter_batch on one context evicts neither schedule.  Results do not depend on the list's order.
 * Read bound: after the picture clip a sub-block reads at most ctu_size + 8 + 3 samples left of / above the picture and at most 8 + cu_w + 3 + 1 ( 8 + cu_h + 3 + 1 ) samples
 * right of / below it (the + 1: PROF's ring) — with CUs no larger than the CTU inside the reference encoder's own picture margin of ctu_size + 16 —, plus the 16 bytes of the
 * aligned-dword rule; planes need an even row pitch.
 * Argument errors (VVHIP_E_ARG with a message naming the entry, nothing launched): a CU size that is not a power of two in 8..128; neither list used; a plane index outside the
 * table; chroma > 1; six_param > 1; prof > 3; non-zero reserved bytes; a control point outside the 18-bit vector range; ctu_size not 32 / 64 / 128; a CU outside the picture.
 * Bit depths 8..12; compared with the reference's xPredAffineBlk (scalar and x86 row) at 8, 10 and 12 bits, with dMv at +-31 and dI in its clip.  That clip is 1 << 13 at
 * every accepted bit depth ( max( bit_depth + 1, 13 ) = 13 up to 12 bits ).                                                                                                */
typedef struct
{
  int32_t dst_off;            /* sample offset of the block in d_pred (and in d_resi)                                  */
  int32_t org_off;            /* the block in the original plane (residual only)                                       */
  int32_t ref_off[2];         /* per list: the block's own (collocated, zero-vector) position in plane ref_plane[l]    */
  int32_t cpmv[2][3][2];      /* per list LT, RT, LB as ( hor, ver ) in 1/16 luma sample; LB ignored unless six_param  */
  int16_t cu_x, cu_y;         /* the CU in luma samples                                                                */
  int16_t cu_w, cu_h;         /* independent powers of two, 8..128                                                     */
  int8_t  ref_plane[2];       /* index into the plane table, -1 = list not used                                        */
  uint8_t chroma;             /* 0: the cu_w x cu_h luma block, 1: a 4:2:0 chroma block cu_w / 2 x cu_h / 2            */
  uint8_t six_param;          /* 1: the 6-parameter model                                                              */
  uint8_t prof;               /* 0..3, see above (luma only)                                                           */
  uint8_t rsv[3];             /* zero                                                                                  */
} vvhip_pred_affine_item;     /* 80 bytes */
VVHIP_API int vvhip_pred_affine_batch( vvhip_ctx* ctx, const vvhip_me_plane* planes_host, int n_planes, const vvhip_pred_affine_item* items_host, int n,
                                       int pic_width, int pic_height, int ctu_size /* luma: 32, 64, 128 */, int bit_depth,
                                       int16_t* d_pred, int pred_stride,
                                       const int16_t* d_org /* may be NULL */, int org_stride, int16_t* d_resi /* may be NULL */ );
/* The chroma twin of vvhip_interp_luma_batch: n blocks of ONE size (powers of two, 2..64) from one plane, items on the device (frac_x / frac_y in 1/32 sample, org_off unused),
 * compact output d_out[i*w*h + y*w + x]; rnd_res 1 = final samples, 0 = the 14-bit intermediate a bi-prediction average consumes.  Margins as above.                            */
VVHIP_API int vvhip_interp_chroma_batch( vvhip_ctx* ctx, const int16_t* d_ref, int ref_stride, const vvhip_subpel_item* d_items, int n,
                                         int width, int height, int bit_depth, int rnd_res, int16_t* d_out );

/* ROM accessors (host memory out): the tables the kernels use, for parity checks against
 * g_trCore* (CommonLib/RomTr.cpp:364-449) and getScanOrder (CommonLib/Rom.h:104).               */
VVHIP_API int vvhip_get_tr_matrix_host( int tr_type, int log2_size, int16_t* host_out );
VVHIP_API int vvhip_get_scan_order_host( int log2_w, int log2_h, uint32_t* host_out );
/* the GEO weights w0 (0..8) of one component block as vvhip_pred_inter_batch_blend applies them: split_dir 0..63, the CU's luma size as log2 3..6 per side, chroma 0 = the
 * luma block, 1 = a 4:2:0 chroma block ( cu_w / 2 ) x ( cu_h / 2 ); host_out takes width * height entries, row by row.  For parity checks against xWeightedGeoBlk
 * (g_globalGeoWeights / g_weightOffset / g_angle2mirror / g_GeoParams, CommonLib/Rom.cpp:1304-1382).  Needs no device.                                              */
VVHIP_API int vvhip_get_geo_weights_host( int split_dir, int log2_cu_w, int log2_cu_h, int chroma, int8_t* host_out );
/* the six tap tables of a motion-search plan's refinement-stage kernels at this bit depth (8..10), 6 x 192 dwords, table = filter_mode * 2 + alt_hpel:
 * [0..127] 16 phases x 8 window taps (tap k multiplies the sample at offset k - 3) of the SECOND pass, scaled by 2^(16 - shift2), shift2 = 6 + headRoom, headRoom = 14 - bit_depth
 * (InterpolationFilter.cpp:394-400: the filtered sample is the upper half of the 32-bit sum); [128..191] 16 phases x 4 packed int16 pairs (taps K0 + 2i, K0 + 2i + 1 of the table's
 * tap support: 4-tap search set 2..5, 6 taps / alternative half-sample filter 1..6, 8 taps 0..7) of the FIRST pass, scaled by 2^(8 - shift1), shift1 = 6 - headRoom (:401-408).     */
VVHIP_API int vvhip_get_me_tap_tables_host( int bit_depth, int32_t* host_out );

/* ---------------------------------------------------------------------------------------------
 * (C) MCTF block matching — replaces MCTF::m_motionErrorLumaInt8 / m_motionErrorLumaFrac8[2] /
 *     m_calcVar and the search schedule around them (CommonLib/MCTF.h:160-170,
 *     CommonLib/MCTF.cpp:122-257, 520-546, 1072-1397).
 * ------------------------------------------------------------------------------------------- */
typedef struct { int32_t org_off; int32_t buf_off; int16_t fx; int16_t fy; } vvhip_mctf_item;

/* out[i] = motionErrorLumaInt (fx==fy==0) or motionErrorLumaFrac{6,4} with the reference's
 * 1/16-pel filter rows fx, fy (tap4 != 0: m_interpolationFilter4, else m_interpolationFilter8).
 * The full error is returned (the reference's `> besterror` early exit is semantically inert,
 * MCTF.cpp:138-141 and callers :1201,:1223).                                                     */
VVHIP_API int vvhip_mctf_error_batch( vvhip_ctx* ctx, const int16_t* d_org, int org_stride,
                                      const int16_t* d_buf, int buf_stride, int width, int height,
                                      int tap4, int bit_depth, const vvhip_mctf_item* d_items, int n, int32_t* d_out );

/* calcVarCore (MCTF.cpp:520-546) for n blocks of one size: out[i] = variance * 256 as int64
 * (the double the reference returns is exactly out[i] / 256.0).                                   */
VVHIP_API int vvhip_mctf_calc_var_batch( vvhip_ctx* ctx, const int16_t* d_org, int org_stride, int width, int height,
                                         const int32_t* d_off, int n, int64_t* d_out_x256 );

/* MCTF::subsampleLuma (MCTF.cpp:1072-1097) incl. the border extension by `pad` samples.
 * d_dst points at sample (0,0) of a plane with >= pad samples of margin on every side.           */
VVHIP_API int vvhip_mctf_subsample( vvhip_ctx* ctx, const int16_t* d_src, int src_stride, int src_width, int src_height,
                                    int16_t* d_dst, int dst_stride, int pad );
VVHIP_API int vvhip_extend_border( vvhip_ctx* ctx, int16_t* d_plane, int stride, int width, int height, int pad );

/* layout of MotionVector (CommonLib/MCTF.h:72-82); x,y in 1/16 pel */
typedef struct { int32_t x, y, error, rmsme; double overlap; } vvhip_mv;

/* One level of MCTF::motionEstimationLuma (MCTF.cpp:1329-1397) = estimateLumaLn (:1166-1327) for every
 * block of the level, including the above/left wavefront dependency, in one call.
 * d_prev (may be NULL) is the coarser level's field, prev_w x prev_h, `factor` as in the reference.
 * d_mvs is mvs_w x mvs_h and must have been initialised with vvhip_mctf_init_mvs (default MotionVector).
 * search_pattern / low_res_filter: MCTF::m_searchPttrn / m_lowResFltSearch (MCTF.cpp:598-599).    */
VVHIP_API int vvhip_mctf_init_mvs( vvhip_ctx* ctx, vvhip_mv* d_mvs, int count );
VVHIP_API int vvhip_mctf_me_level( vvhip_ctx* ctx,
                                   const int16_t* d_org, int org_stride, const int16_t* d_buf, int buf_stride,
                                   int width, int height, int block_size,
                                   const vvhip_mv* d_prev, int prev_w, int prev_h, int factor, int double_res,
                                   int search_pattern, int low_res_filter, int bit_depth, int unit_size,
                                   vvhip_mv* d_mvs, int mvs_w, int mvs_h );

/* MCTF::motionEstimationMCTF (MCTF.cpp:666-707) for one current picture against n_refs reference
 * pictures: builds the 2x/4x(/8x) pyramids, runs every level for all references concurrently.
 * Planes are luma, `pad` (>= 128 = MCTF_PADDING) samples of replicated margin, pointers at sample (0,0).
 * d_mvs_out[r] receives ceil(w/unit) x ceil(h/unit) motion vectors of reference r.                 */
VVHIP_API int vvhip_mctf_motion_estimation( vvhip_ctx* ctx, const int16_t* d_cur, const int16_t* const* d_refs_host_array,
                                            int n_refs, int stride, int width, int height, int pad, int bit_depth,
                                            int unit_size, int mctf_speed, int add_level,
                                            vvhip_mv* const* d_mvs_out_host_array );

/* The same call WITHOUT the host wait at its end: every launch is queued on the context's stream and the call returns (like every other entry point); results are valid
 * once the stream has passed them.  What bench.py's sixth stream issues at the GOP's cadence while the other five run a picture's lists.  (A field whose anti-diagonals
 * exceed a workgroup — more than 320 blocks on the shorter side: beyond 8K — takes the row hand-off with its abort flag; the call then waits like the synchronous one.)
 * Replaces the same reference loop as above, MCTF.cpp:666-724 called per reference from MCTF::filter :779-800.                                              */
VVHIP_API int vvhip_mctf_motion_estimation_async( vvhip_ctx* ctx, const int16_t* d_cur, const int16_t* const* d_refs_host_array,
                                                  int n_refs, int stride, int width, int height, int pad, int bit_depth,
                                                  int unit_size, int mctf_speed, int add_level,
                                                  vvhip_mv* const* d_mvs_out_host_array );

/* Scored-candidate counters of the MCTF search (measurement: the algorithmic bytes of SURVEY 8d are priced per SCORED candidate, and which candidates estimateLumaLn
 * scores depends on the data — MCTF.cpp:1189-1306).  set_stats( 1 ) allocates and zeroes 24 counters and switches the counting kernel instances on, set_stats( 0 )
 * switches them off.  get_stats copies them to the host (waits for the stream).  Three phases x 8 counters:
 *   out[0..7]   phase A (estimateLumaLn up to the above/left tests): [0] integer candidates scored one by one, [1] their bytes (4 w h each), [2] fractional candidates scored
 *               one by one, [3] their bytes ((w + taps - 1)(h + taps - 1) 2 + 2 w h each; taps = 4 with the low-resolution search filter, 6 otherwise), [4] positions of the
 *               dense integer grids (MCTF.cpp:1216-1228) scored out of one staged window, [5] those windows' bytes in SURVEY 8d's window form ((w + 2R)^2 2 + 2 w h per block
 *               + 8 per position); the per-candidate figure of the grid positions is [4] x 4 w h with w = h = 32 (only full blocks take that path), [6] positions of the
 *               refinement rings (:1229-1288) whose horizontal passes are shared, [7] those rings' bytes in window form (( w + 4 )( h + 4 ) 2 + 2 w h + 8 per position: the
 *               positions of a ring lie within half a sample of its centre); per-candidate figure [6] x ((w + 3)(h + 3) 2 + 2 w h)
 *   out[8..15]  the above/left candidates scored in parallel at the neighbours' phase-A vectors, out[16..23] those scored while the recurrence is resolved.             */
VVHIP_API int vvhip_mctf_set_stats( vvhip_ctx* ctx, int on );
/* Per-class device time of the LAST motion-estimation call of the context (measurement; HIP events on the context's stream around every launch while on):
 * ms5 = { candidate scoring (meSearchKernel, all levels), neighbour scoring, sweep, final normalisation, everything else (pyramids, field initialisation) }.   */
VVHIP_API int vvhip_mctf_set_timing( vvhip_ctx* ctx, int on );
VVHIP_API int vvhip_mctf_last_times( vvhip_ctx* ctx, float* ms5 );
VVHIP_API int vvhip_mctf_get_stats( vvhip_ctx* ctx, uint64_t* out24 );

/* ======================================================================================================================
 * SURVEY 8f rank 2 — MCTF apply side: motion-compensated bilateral temporal filter of one component plane
 * (MCTF::bilateralFilter / xFinalizeBlkLine, CommonLib/MCTF.cpp:1399-1552, with applyFrac8Core_6Tap/_4Tap :259-358,
 * applyPlanarCorrectionCore :372-421 and applyBlockCore :423-518 fused per block).  Equals the reference's scalar row AND its x86 row
 * (CommonLib/x86/MCTFX86.h:861-1440): the two agree sample for sample (tests/test_oracle_vs_reference.py holds both to tolerance 0).
 *   d_org / d_refs[i] : sample (0,0) of planes whose margins cover the motion vectors (MCTF_PADDING 128 luma, 64 chroma)
 *   d_mvs[i]          : final-level motion field of reference i (what vvhip_mctf_motion_estimation returns), mv_w blocks per row
 *   chroma_shift      : 0 luma, 1 the chroma planes of 4:2:0 (vectors and block size are halved)
 *   ref_strengths     : host array, m_refStrengths[row][|POC offset| - 1] per reference (MCTF.cpp:112-117)
 *   weight_scaling / sigma_sq : per channel, see vvhip_mctf_filter_params
 * d_refs / d_mvs are HOST arrays of device pointers.                                                                              */
VVHIP_API int vvhip_mctf_apply_plane( vvhip_ctx* ctx, const int16_t* d_org, int org_stride, int width, int height, int chroma_shift,
                                      int bit_depth, int unit_size, int low_res_flt_apply, int qp, int num_refs,
                                      const int16_t* const* d_refs, int ref_stride, const vvhip_mv* const* d_mvs, int mv_w,
                                      const double* ref_strengths, double weight_scaling, double sigma_sq,
                                      int16_t* d_out, int out_stride );
/* sigmaSq and weightScaling exactly as MCTF::bilateralFilter (:1491-1501) and xFinalizeBlkLine (:1417) derive them (host only). */
VVHIP_API int vvhip_mctf_filter_params( int qp, int bit_depth, double overall_strength, int is_chroma, double* sigma_sq, double* weight_scaling );

/* ======================================================================================================================
 * SURVEY 8f rank 3 — DMVR refinement search (decoder-normative, integer): DMVR::xProcessDMVR, CommonLib/InterPrediction.cpp:1262-1392.
 * Per sub-block (dx, dy in {8, 16}; DMVR_SUBCU_SIZE 16): bilinear prediction of both lists around the (already clipped) merge vectors
 * (InterpolationFilter::filterN2_2D), centre cost with early exit, 25-point mirrored SAD search (dmvrSadX5 semantics, strict < in the
 * reference's scan order), parametric sub-pel error surface.
 *   ref0_off / ref1_off : the sub-block's integer position for the merge vector of list 0 / 1 (mv >> 4), frac* = mv & 15
 *   result              : mvd = cu.mvdL0SubPu[num] in 1/16 sample (list 1 moves by -mvd), min_cost = the value the BDOF switch compares
 *                         with 2*dx*dy (:1386).  The final motion compensation: sub-blocks whose refinement is zero go into a prediction list
 *                         (vvhip_pred_inter_batch: luma + chroma, both lists, the average); a refined sub-block reads through DMVR's padded-reference
 *                         rule (xFinalPaddedMCForDMVR, :1189-1225), with BDOF where min_cost allows it: vvhip_pred_inter_batch_ex.
 *   read footprint      : of either list, relative to the sample at ref*_off and whatever the fractions are: rows -2 .. dy + 2 and columns -2 .. 8 * segs - 1 with
 *                         segs = (dx + 4 + 7) >> 3 — 13 (dy 8) or 21 (dy 16) rows of 18 (dx 8) or 26 (dx 16) samples.  The reference reads rows -2 .. dy + 1 and columns
 *                         -2 .. dx + 1, and one more row / column where the vertical / horizontal fraction is not 0; the kernel loads whole lanes of ten samples at a pitch
 *                         of eight and always the extra row, so up to six more columns to the right and one more row below.  These samples must lie inside the
 *                         allocation (they may belong to the next row of the plane); their values never reach a result.                                  */
typedef struct { int32_t ref0_off, ref1_off; int16_t frac0_x, frac0_y, frac1_x, frac1_y; } vvhip_dmvr_item;
typedef struct { int16_t mvd_x, mvd_y; int32_t pad; uint64_t min_cost; } vvhip_dmvr_result;
VVHIP_API int vvhip_dmvr_refine_batch( vvhip_ctx* ctx, const int16_t* d_ref0, int stride0, const int16_t* d_ref1, int stride1,
                                       const vvhip_dmvr_item* d_items, int n, int dx, int dy, int bit_depth, vvhip_dmvr_result* d_out );

/* ======================================================================================================================
 * SURVEY 8f rank 4 — ALF encoder statistics (P_ALF, 19.5 % of single-thread time at preset faster).
 *   vvhip_alf_classify    <- AdaptiveLoopFilter::m_deriveClassificationBlk (deriveClassificationBlk, CommonLib/AdaptiveLoopFilter.cpp:524-728):
 *       class index / transpose index of every 4x4 luma block of a picture; d_cls holds 2 bytes per block {classIdx, transposeIdx},
 *       width/4 blocks per row.  vb_ctu_height / vb_pos = m_alfVBLumaCTUHeight / m_alfVBLumaPos (:411-415: CTU height, CTU height - 4).
 *   vvhip_alf_stats_plane <- EncAdaptiveLoopFilter::getPreBlkStats + m_getPreBlkStatsAccum for every CTU of a plane
 *       (EncoderLib/EncAdaptiveLoopFilter.cpp:3376-3541, :3266-3319), linear filters (numBins 1): filter_length 7 with d_cls (luma, 25
 *       classes) or 5 with d_cls == NULL (chroma, one class; ctu_size / vb_* in chroma samples).  d_out: [numCtus][numClasses][183] floats per
 *       record = E[13][13] (row-major, symmetric), y[13], pixAcc.  The float additions happen in the reference's order (4x4 blocks of a
 *       CTU in raster order, per class): results are bit-identical.  Blocks classified {255, 255} are skipped (m_ALF_UNUSED_CLASSIDX).
 *       d_init (optional, same layout as d_out; may alias it): the records the additions start from — a statistics unit that spans several CTUs
 *       (alfUnitSize > CTU size: getStatisticsASU, :1568-1590) continues its float chains from CTU to CTU.
 * d_rec carries a replicated border of >= 4 samples (the reference reads its extended m_tempBuf); width / height multiples of 4.      */
#define VVHIP_ALF_REC 183
VVHIP_API int vvhip_alf_classify( vvhip_ctx* ctx, const int16_t* d_rec, int stride, int width, int height, int bit_depth, int vb_ctu_height, int vb_pos, uint8_t* d_cls );
VVHIP_API int vvhip_alf_stats_plane( vvhip_ctx* ctx, const int16_t* d_org, int org_stride, const int16_t* d_rec, int rec_stride, int width, int height, int ctu_size,
                                     int filter_length, const uint8_t* d_cls /* NULL: chroma */, int vb_ctu_height, int vb_pos, const float* d_init /* may be NULL */, float* d_out );

/* The same with statistics units larger than a CTU (alfUnitSize > CTU size, EncAdaptiveLoopFilter::getStatisticsASU :1568-1590): one record set per unit of
 * unit_size x unit_size samples (<= 128), the float chains run through the unit's CTUs (ctu_size >= 8 dividing unit_size, raster order) and the blocks inside
 * each CTU.                                                                                                                                                */
VVHIP_API int vvhip_alf_stats_plane_units( vvhip_ctx* ctx, const int16_t* d_org, int org_stride, const int16_t* d_rec, int rec_stride, int width, int height, int unit_size,
                                           int ctu_size, int filter_length, const uint8_t* d_cls, int vb_ctu_height, int vb_pos, const float* d_init, float* d_out );

/* CC-ALF statistics <- EncAdaptiveLoopFilter::getBlkStatsCcAlf per chroma CTU (EncoderLib/EncAdaptiveLoopFilter.cpp:6061-6357; local terms
 * calcCovariance4CcAlf :6359-6422): 7 luma differences around the co-located luma sample against org - ALF-filtered chroma (d_slf_c).  One record of
 * VVHIP_ALF_REC floats per chroma CTU: E[0..6][0..6] (row pitch 13), y[0..6], pixAcc; float additions in the reference's order (bit-identical).
 * d_rec_luma carries a replicated border of >= 2 samples; shift_x / shift_y = chroma subsampling (4:2:0: 1, 1); vb_* and pic_height in luma samples
 * (the last CTU row has no virtual boundary, :6079-6082); d_init as in vvhip_alf_stats_plane.                                                  */
VVHIP_API int vvhip_ccalf_stats_plane( vvhip_ctx* ctx, const int16_t* d_org_c, int org_stride, const int16_t* d_slf_c, int slf_stride, const int16_t* d_rec_luma, int rec_stride,
                                       int width_c, int height_c, int ctu_size_c, int shift_x, int shift_y, int vb_ctu_height, int vb_pos, int pic_height,
                                       const float* d_init /* may be NULL */, float* d_out );

/* ALF filtering of a plane <- AdaptiveLoopFilter::m_filter7x7Blk / m_filter5x5Blk (filterBlk<ALF_FILTER_7 / ALF_FILTER_5>, CommonLib/AdaptiveLoopFilter.cpp:730-967) applied to
 * every enabled CTU the way EncAdaptiveLoopFilter::reconstructCTU does when no slice / tile / virtual picture boundary crosses the CTU (EncoderLib/EncAdaptiveLoopFilter.cpp:2035-2066).
 * filter_length 7 with d_cls (luma: class / transpose index per 4x4 block as written by vvhip_alf_classify, 25 classes) or 5 with d_cls == NULL (chroma, one class).
 * d_coeff / d_clip: [num_sets][numClasses][13] int16 — the reference's m_coeffApsLuma / m_fixedFilterSetCoeffDec / m_chromaCoeffFinal rows and the matching clipping values;
 * d_clip == NULL selects the linear table entries (m_filter*Blk[0]: the x86 row ignores the clipping values there).  d_ctu_set[ctu]: filter set (luma: alfCtuFilterIndex;
 * chroma: m_ctuAlternative) of the CTU, < 0 = m_ctuEnableFlag off (the CTU's samples in d_dst stay untouched).  d_src carries a replicated border of >= 4 samples and must not
 * overlap d_dst; any strides (in samples) and alignment.  vb_ctu_height / vb_pos as in vvhip_alf_classify (chroma: m_alfVBChmaCTUHeight / m_alfVBChmaPos).
 * The sums are int32 like the reference's scalar row at every bit depth; its x86 row saturates sum >> 7 at 16 bits, which 12-bit samples reach once sum |c_k| exceeds 512.       */
VVHIP_API int vvhip_alf_filter_plane( vvhip_ctx* ctx, const int16_t* d_src, ptrdiff_t src_stride, int16_t* d_dst, ptrdiff_t dst_stride, int width, int height, int ctu_size, int bit_depth,
                                      int filter_length, const uint8_t* d_cls, const int16_t* d_coeff, const int16_t* d_clip /* NULL: linear */, const int16_t* d_ctu_set,
                                      int vb_ctu_height, int vb_pos );

/* CC-ALF filtering of a chroma plane <- AdaptiveLoopFilter::m_filterCcAlf (filterBlkCcAlf, CommonLib/AdaptiveLoopFilter.cpp:969-1058) as EncAdaptiveLoopFilter::applyCcAlfFilterCTU
 * drives it (EncoderLib/EncAdaptiveLoopFilter.cpp:6606-6699): d_dst_c (the ALF-filtered chroma plane) is corrected in place from the unfiltered luma d_rec_luma (replicated border
 * >= 2).  d_coeff: [num_filters][8] int16 (ccAlfCoeff, 7 used); d_ctu_filter[ctu]: 0 = off, k = filter k-1 (m_ccAlfFilterControl).  vb_* in luma samples.                        */
VVHIP_API int vvhip_ccalf_filter_plane( vvhip_ctx* ctx, int16_t* d_dst_c, ptrdiff_t dst_stride, const int16_t* d_rec_luma, ptrdiff_t rec_stride, int width_c, int height_c, int ctu_size_c,
                                        int shift_x, int shift_y, int bit_depth, const int16_t* d_coeff, const uint8_t* d_ctu_filter, int vb_ctu_height, int vb_pos );

/* ======================================================================================================================
 * SAO (sample adaptive offset), the stage in front of ALF in the per-CTU pipeline CTU_ENCODE -> LF -> SAO -> ALF (EncoderLib/EncSlice.cpp:1058-1141): the statistics of a
 * picture and the offset filtering of a picture, each ONE launch for up to 3 planes and a band of CTU rows.  With both, a deblocked picture stays in
 * HBM through to the ALF entries above.
 *   vvhip_sao_stats  <- EncSampleAdaptiveOffset::getBlkStats (EncoderLib/EncSampleAdaptiveOffset.cpp:810-929) + the five calcSaoStatistics*_Core routines
 *       (CommonLib/SampleAdaptiveOffset.cpp:281-399) for every CTU, as getStatistics (:294-344) and getCtuStatistics (:239-292) drive them.
 *       d_out: int64 [ctu][plane][5][2][32] at the CTU's PICTURE-WIDE raster index — byte-compatible with SAOStatData[5] per CTU and plane ({ int64 diff[32]; int64 count[32]; },
 *       order EO_0, EO_90, EO_135, EO_45, BO; edge classes at 0..4 = edgeType + 2, bands at src >> ( bit_depth - 5 )).  Every record of the band is written completely
 *       (zeros and the unused indices 5..31 of the edge types included: no pre-zeroing), nothing else is written.  Integer sums: bit-identical in any order and from run to run.
 *       flags_host (may be NULL): one byte per CTU of the PICTURE (raster; only the band's entries are read), VVHIP_SAO_* bits = isLeftAvail, isAboveAvail, isAboveLeftAvail
 *       (slice / tile structure: the caller's deriveLoopFilterBoundaryAvailibility) and isRightAvail, isBelowAvail, isAboveRightAvail.  NULL: the picture's borders alone
 *       decide, as in getStatistics.  Where the right / below CTU is available the right 5 columns / bottom 4 rows of a luma CTU (3 / 2 of a chroma CTU: is_luma) are left
 *       out — they are not deblocked yet when the CTU's statistics are taken in the pipeline.
 *   vvhip_sao_offset <- offsetBlock_core (CommonLib/SampleAdaptiveOffset.cpp:64-280) as offsetCTU drives it (:605-652) from the DECIDED parameters of every CTU and plane:
 *       params_host [ctu][plane] at the picture-wide raster index (only the band's are read).  type -1 = SAO_MODE_OFF, 0..3 = EO_0, EO_90, EO_135, EO_45 with offs[edgeType + 2]
 *       (all five as given), 4 = BO with offs[i] on band ( band + i ) & 31, i < 4 — everything reconstructBlkSAOParam can produce, and the subset on which the reference's
 *       scalar and x86 rows agree.  avail = the reference's 8-bit mask (SampleAdaptiveOffset.h:75-85: 1 left, 2 right, 4 above, 8 below, 16 above-left, 32 above-right,
 *       64 below-left, 128 below-right).  d_dst receives the complete plane rows of the band: the filtered samples (clipped to [clip_min, clip_max], also where the offset is 0),
 *       and the source value everywhere else — outside the processed ranges and in CTUs that are off.  d_src is never written and must not overlap any d_dst.
 * Planes: any strides (in samples, >= width) and any base alignment; samples are read only inside width x height, no border is needed.  ctu_w / ctu_h are in the plane's
 * own samples (8..128); all planes of a call must have the same CTU grid.  Band = CTU rows [ctu_row0, ctu_row0 + n_rows), n_rows >= 1.
 * Operand contract: 0 <= src < 2^bit_depth (the band index is src >> ( bit_depth - 5 ); a violation lands in band ( index & 31 )), bit_depth 8..12, | org - src | < 2^15.
 * VVHIP_E_ARG: no planes / more than 3; a CTU size outside 8..128; planes with different CTU grids; a last CTU column or row of ONE sample (the reference's diagonal types read
 * past their block there); a band outside the picture; a flag / availability bit set for a neighbour outside the picture; a type outside -1..4, band > 31, rsv != 0;
 * clip_min > clip_max; a source plane that overlaps a destination plane (compared as spans, first to last sample: rows of two planes interleaved in one buffer overlap).
 * The filter follows offsetBlock_core for EVERY mask.  The reference's x86 row equals it on the masks a picture's borders give, and in general unless left, right, above-left
 * and below-right are all set while above or below is not (EO_135, EO_45) or above-right or below-left is not (EO_45); it also clips to the bit depth whatever the ClpRng.
 * Still the caller's: decideCtuParams / deriveOffsets / the rate estimation (serial over CTUs: CABAC contexts and the left / above merge candidates; they read only the
 * 2560-byte records), the merge list, decidePicParams, and the per-CTU pipeline timing of storeCtuReco.                                                                        */
#define VVHIP_SAO_LEFT        1
#define VVHIP_SAO_ABOVE       2
#define VVHIP_SAO_ABOVE_LEFT  4
#define VVHIP_SAO_RIGHT       8
#define VVHIP_SAO_BELOW       16
#define VVHIP_SAO_ABOVE_RIGHT 32
#define VVHIP_SAO_REC         320   /* int64 per CTU and plane: [5][2][32] */
typedef struct
{
  const int16_t* d_org;            /* the original plane                                                          */
  const int16_t* d_src;            /* the deblocked plane                                                         */
  int32_t org_stride, src_stride;  /* in samples                                                                  */
  int32_t width, height;           /* of the plane                                                                */
  int32_t ctu_w, ctu_h;            /* CTU size in the plane's own samples, 8..128                                 */
  int32_t bit_depth;               /* 8..12                                                                       */
  int32_t is_luma;                 /* skipped columns / rows: 5 / 4 (luma) or 3 / 2 (chroma)                      */
} vvhip_sao_stats_plane;           /* 48 bytes */
typedef struct
{
  const int16_t* d_src;            /* the deblocked plane, never written                                          */
  int16_t* d_dst;                  /* the SAO'd plane                                                             */
  int32_t src_stride, dst_stride;
  int32_t width, height;
  int32_t ctu_w, ctu_h;
  int32_t bit_depth;
  int32_t clip_min, clip_max;      /* ClpRng of the component                                                     */
  int32_t rsv;
} vvhip_sao_offset_plane;          /* 56 bytes */
typedef struct
{
  int8_t  type;                    /* -1 off, 0..3 EO_0 / EO_90 / EO_135 / EO_45, 4 BO                            */
  uint8_t avail;                   /* the reference's availability mask of the CTU                                */
  uint8_t band;                    /* BO: first band (typeAuxInfo), 0..31                                         */
  uint8_t rsv;                     /* 0                                                                           */
  int16_t offs[5];                 /* EO: offs[edgeType + 2]; BO: offs[0..3]                                      */
} vvhip_sao_param;                 /* 14 bytes */
VVHIP_API int vvhip_sao_stats( vvhip_ctx* ctx, const vvhip_sao_stats_plane* planes, int n_planes, int ctu_row0, int n_rows, const uint8_t* flags_host /* may be NULL */,
                               int64_t* d_out );
VVHIP_API int vvhip_sao_offset( vvhip_ctx* ctx, const vvhip_sao_offset_plane* planes, int n_planes, const vvhip_sao_param* params_host, int ctu_row0, int n_rows );

/* ======================================================================================================================
 * LF (the deblocking filter), the stage in front of SAO in the per-CTU pipeline CTU_ENCODE -> LF -> SAO -> ALF: with it the UNFILTERED reconstruction is uploaded once and
 * everything up to ALF's output happens in HBM.
 *   vvhip_deblock <- LoopFilter::xDeblockArea<EDGE_VER> over every CTU of the picture, then xDeblockArea<EDGE_HOR> over every CTU (CommonLib/LoopFilter.cpp:405-462, as
 *       EncoderLib/EncSlice.cpp:1020 / :1052 run them), in place on d_plane, bit-exact:
 *       luma   xEdgeFilterLuma (:1372-1520) per 4-sample edge segment of the 4 x 4 grid: bS = bs bits 0-1, qp[0], P / Q lengths = side_max_filt_length bits 4-6 / 0-2 (bit 7,
 *              the transform-edge mark, is ignored); at a horizontal CTU boundary the P side is never long (:1437); tc / beta from sm_tcTable / sm_betaTable (:79-87) with
 *              the bit-depth scaling of :1445-1446; the long-filter decision (xUseStrongFiltering, :1318-1370) and xFilteringPandQCore (:123-201) for the P / Q length
 *              pairs 7/7, 7/5, 5/7, 7/3, 3/7, 5/5, 5/3, 3/5; otherwise d < beta, the side thresholds only where both lengths > 1, the strong filter only where both > 2, and
 *              xPelFilterLumaCorePel (:217-264): strong, or weak with | delta | < 10 tc, the second samples, ClipPel to [clip_min, clip_max].
 *       chroma xEdgeFilterChroma (:1522-1635), 4:2:0, only where the chroma position inside the CTU is a multiple of 8 across the edge (:449-452), two samples per record:
 *              per component bS = bs bits 2-3 / 4-5, qp[1] / qp[2], the plane's own offsets; filtered where bS == 2, or bS == 1 with filterCMFL (flags bit 5); the
 *              large-boundary decision with dp3 / dq3 one line on; at a horizontal CTB boundary the shortened P side (xCalcDP's p1 - 2 p1 + p0, :1305, and the four-sample
 *              strong form of :301-304); xPelFilterChroma (:284-342) weak / strong.
 *       The reference's bPartPNoFilter / bPartQNoFilter are constant false; there is no lossless bypass.
 * Maps: lfp_ver_host / lfp_hor_host are HOST arrays of LoopFilterParam records (CommonLib/TypeDef.h:546-559; vvhip_lf_param is byte-compatible), one per 4 x 4 luma unit,
 * lfp_stride records per map row (>= width / 4).  Only the band's records are read.  They are validated, copied and uploaded by the call; the copy a previous launch may
 * still be reading is waited for first, so the caller's arrays are free when the call returns.  A map of a direction not in `dirs` may be NULL.
 * The maps must be LEGAL, as calcFilterStrengths (:552-1271) leaves them: no edge of a direction writes a sample another edge of that direction reads or writes.  The entry
 * cannot check that geometry; on other maps the result is undefined (but no sample outside width x height is read or written).
 * Bands: CTU rows [ctu_row0, ctu_row0 + n_rows), dirs = any non-empty subset of VVHIP_DBK_VER | VVHIP_DBK_HOR.  VER filters every vertical edge whose samples lie in the
 * band's rows.  HOR filters every horizontal edge with y in the band — the band's top CTU boundary included, so it may write up to 3 luma rows and 1 chroma row above the
 * band, and nothing else outside it.  With both bits VER of the band completes before its HOR starts (two launches in stream order).
 * CALLER'S CONTRACT: VER of CTU row r - 1 must have been issued (same stream, or ordered by events) before HOR of row r.  Under it every partition of a picture into bands
 * gives the one-call result: bands top to bottom with both bits, or all VER bands in any order followed by all HOR bands in any order.
 * Planes: n_planes 1 (4:0:0, or luma only) or 3 (4:2:0: planes 1, 2 exactly half of plane 0); any strides (in samples, >= width) and any base alignment; samples are read
 * and written only inside width x height.  Results are identical from run to run.
 * VVHIP_E_ARG, before any launch and with nothing written: n_planes not 1 or 3; chroma planes not exactly half the luma size; luma width or height no multiple of 8;
 * bit_depth outside 8..12; ctu_size no power of two in 16..128; a band outside the picture or n_rows < 1; dirs outside 1..3; lfp_stride < width / 4; clip_min > clip_max;
 * and in the band's records: a bs field of 3; a P or Q length outside { 0, 1, 2, 3, 5, 7 } where the luma bs is non-zero; flag bits other than 0, 1, 5; a non-zero bs in
 * column 0 of the vertical map or row 0 of the horizontal map (the reference would read outside the picture).
 * Still the caller's: calcFilterStrengths (serial, syntax-bound: CUs, TUs, motion) and the band ordering contract above.                                                     */
typedef struct
{
  int8_t  qp[3];                   /* the edge's QP per component                                                 */
  uint8_t bs;                      /* bS: bits 0-1 luma, 2-3 Cb, 4-5 Cr, each 0..2                                */
  uint8_t side_max_filt_length;    /* luma: P length in bits 4-6, Q length in bits 0-2                            */
  uint8_t flags;                   /* bits 0, 1: filterEdge per channel type (not read); bit 5: filterCMFL        */
} vvhip_lf_param;                  /* 6 bytes, byte-compatible with LoopFilterParam */
typedef struct
{
  int16_t* d_plane;                /* filtered in place                                                           */
  int32_t stride, width, height;   /* stride in samples                                                           */
  int32_t clip_min, clip_max;      /* ClpRng of the component (the weak filters' ClipPel)                         */
  int32_t beta_offset_div2, tc_offset_div2;   /* the slice's deblockingFilterBetaOffsetDiv2 / TcOffsetDiv2 of the component */
} vvhip_deblock_plane;             /* 40 bytes */
#define VVHIP_DBK_VER 1
#define VVHIP_DBK_HOR 2
VVHIP_API int vvhip_deblock( vvhip_ctx* ctx, const vvhip_deblock_plane* planes, int n_planes /* 1 = 4:0:0 or luma only, 3 = 4:2:0 */, int bit_depth, int ctu_size /* luma, 16..128 */,
                             const vvhip_lf_param* lfp_ver_host, const vvhip_lf_param* lfp_hor_host, int lfp_stride /* records per map row, >= width / 4 */,
                             int ctu_row0, int n_rows, int dirs );

/* ======================================================================================================================
 * QPA (perceptual QP adaptation): the visual activity of the ORIGINAL picture — the one picture-level, decision-free stage in front of the CTU tasks.  Its inputs are fixed
 * before any decision (the original plane and the two previous originals, the planes the MCTF entries already keep in HBM); its results are integer sums.
 *   vvhip_visact <- the six high-pass entries of g_pelBufOP (CommonLib/Buffer.cpp:323-435, Buffer.h:123-128) as calcSpatialVisAct (EncoderLib/BitAllocation.cpp:84-117) and
 *       calcTemporalVisAct (:119-195) call them, and the accumulator of AreaBuf::getAvg (CommonLib/Buffer.h:303-315), for a LIST of areas in one call:
 *       the CTU areas of BitAllocation::applyQPAdaptationSlice (:553-573: the CTU plus a guard frame of 1 or 2 samples, and the clipped CTU for the mean), the whole chroma
 *       planes (:610-616), the whole planes of PreProcess::xGetVisualActivity (EncoderLib/PreProcess.cpp:312-427), the sub-CTU areas of applyQPAdaptationSubCtu.
 * Per area, d_out[4 * i + ..] (uint64):
 *   [0] the spatial sum saAct.  ds == 0: AvgHighPass (Buffer.cpp:323-337) — | 12 c - 2 ( l + r + u + d ) - ( ul + ur + dl + dr ) | over 1 <= x <= w - 2, 1 <= y <= h - 2 of
 *       the area (calcSpatialVisAct's skipped first row is the y = 0 the loop starts behind).  ds == 1: AvgHighPassWithDownsampling (:371-392) — the 6 x 6 kernel on the 2 x 2
 *       cells at even x, y in 2 <= x < w - 2, 2 <= y < h - 2 RELATIVE TO THE AREA'S ORIGIN (what the reference uses where min( width, height ) of the source > 1280).
 *   [1] the temporal sum taAct over the same positions (ds: the same cells, on the 2 x 2 cell sums): order 1 — HDHighPass / AvgHighPassWithDownsamplingDiff1st:
 *       ( 1 + 3 | cur - prev1 | ) >> 1; order 2 — HDHighPass2 / AvgHighPassWithDownsamplingDiff2nd: | cur - 2 prev1 + prev2 |; order 0: 0.
 *   [2] the plain sample sum of the mean rectangle ( mx, my, mw, mh ) of the plane's cur (two's complement; 0 where mw == 0): getAvg's acc.
 *   [3] the number of positions summed into [0]: ( w - 2 ) ( h - 2 ), or ( w - 4 ) / 2 * ( h - 4 ) / 2.
 * Every record is written completely, nothing else is.  Areas may overlap, be a whole plane, come in any order; an area's record depends on nothing but the area.  All sums are
 * integers: results are identical from run to run (no atomics).  Samples are int16; the sums are exact for ANY int16 samples, bit_depth only documents the plane.
 * areas_host is a HOST array, validated, cut into tiles and uploaded by the call (the copy a previous launch may still read is waited for first); planes is read by the call.
 * VVHIP_E_ARG, before any launch and with nothing written: n < 0; n_planes outside 1..3; a plane without d_cur, with a stride < width, width or height < 1 or bit_depth outside
 * 8..16; a plane index outside the table; an area or a mean rectangle not inside its plane (mw > 0 needs mh > 0 and the reverse); ds == 0 with w < 3 or h < 3; ds == 1 with
 * w < 6 or h < 6 or an odd w or h (the reference's loop would read a row / column beyond the area); ds > 1; order > 2; order >= 1 with d_prev1 == NULL, order == 2 with
 * d_prev2 == NULL (or a stride < width of a plane an area uses); non-zero reserved bytes.  n == 0 succeeds and launches nothing.
 * Still the caller's (out of scope here): hooking the entry into the running encoder; the doubles made of the sums — hpSpatAct, hpTempAct, the 1.15625 factor, the
 * pS0 == pSM1 bypass, updateVisAct (the shim's VisActOps restates them) — and everything in applyQPAdaptationSlice behind the sums (apprI3Log2, the glaring-colour offset,
 * noise levels, peak smoothing, rate control); getCtuPumpingReducingQP; the film-grain analyser.                                                                            */
typedef struct
{
  const int16_t* d_cur;            /* the original plane                                                          */
  const int16_t* d_prev1;          /* the previous original (PREV_FRAME_1), may be NULL                           */
  const int16_t* d_prev2;          /* the one before (PREV_FRAME_2), may be NULL                                  */
  int32_t cur_stride, prev1_stride, prev2_stride;      /* in samples                                              */
  int32_t width, height, bit_depth;
} vvhip_visact_plane;              /* 48 bytes */
typedef struct
{
  uint8_t plane;                   /* row of the plane table                                                      */
  uint8_t ds;                      /* 0: the HD form, 1: the down-sampling form                                   */
  uint8_t order;                   /* 0: no temporal part, 1: first order, 2: second order                        */
  uint8_t rsv0;                    /* 0                                                                           */
  int32_t x, y, w, h;              /* the filter area, in samples of the plane                                    */
  int32_t mx, my, mw, mh;          /* the mean rectangle, in samples of the plane; mw == 0: none                  */
  int32_t rsv1;                    /* 0                                                                           */
} vvhip_visact_area;               /* 40 bytes */
VVHIP_API int vvhip_visact( vvhip_ctx* ctx, const vvhip_visact_plane* planes, int n_planes, const vvhip_visact_area* areas_host, int n, uint64_t* d_out /* [n][4] */ );

/* ======================================================================================================================
 * Intra luma mode pre-selection: the decision-free loop of IntraSearch::xEstimateLumaRdModeList (EncoderLib/IntraSearch.cpp:171-335) for a LIST of blocks in one call — per
 * block one set of reference lines, per requested mode the prediction and its DF_HAD_2SAD cost against the original.  Only the costs leave the device, plus the predictions
 * the caller asks for.
 *   vvhip_intra_luma_modes_batch <- per requested mode m of an item, bit for bit:
 *     IntraPrediction::initPredIntraParams (CommonLib/IntraPrediction.cpp:409-496) for a non-ISP, non-MIP, non-BDPCM luma block: getWideAngle (:335-351), the two angle tables,
 *       applyPDPC and angularScale, refFilterFlag / interpolationFlag from m_aucIntraFilter (:66-76) and isIntegerSlope, planar's w * h > 32 rule, and everything that
 *       multi_ref_idx != 0 switches off (PDPC, both filters' selection);
 *     the [1 2 1] reference filter of xFilterReferenceSamples (:994-1030), once per item;
 *     predIntraAng's dispatch (:353-383): planar (xPredIntraPlanar_Core :79-135), DC (xGetPredValDc :302-333 with its multiRefIndex + 1 offset), IntraPredSampleFilter
 *       (:137-157) for planar and DC under applyPDPC, and all of xPredIntraAng (:518-681): the negative-angle side projection with absInvAngle, the replication of the main
 *       reference's end ( maxIndex = ( multiRefIdx << s ) + 2 ), the pure horizontal / vertical copy with and without IntraHorVerPDPC (:159-175), the integer-slope copy, the
 *       4-tap path (IntraPredAngleLuma :191-223) with the cubic table (InterpolationFilter::getChromaFilterTable; clipped) or the smoothing filter built from deltaFract (not
 *       clipped), IntraAnglePDPC (:176-189), and the transposition of horizontal modes;
 *     the cost min( xGetHADs<false>, 2 * SAD >> DISTORTION_PRECISION_ADJUSTMENT ) of RdCost::xGetHAD2SADs (CommonLib/RdCost.cpp:1768-1816) — VVHIP_DF_HAD_2SAD on compact blocks.
 * The clip range is [0, 2^bit_depth - 1] (the reference's ClpRng).
 * Reference lines (d_ref + ref_off, int16): the UNFILTERED lines of the block exactly as xFillReferenceSamples (:755-990) leaves m_refBuffer[COMP_Y][PRED_BUF_UNFILTERED] for
 * the item's multi_ref_idx r, with predStride = 2w + 1 + r:
 *     [0]                          the corner sample, at ( -1 - r, -1 - r ) of the block
 *     [1 + k], k < 2w + r          the row above: sample ( -r + k, -1 - r )                         — 2w + 1 + r samples from the corner
 *     [predStride]                 the corner sample again
 *     [predStride + 1 + k], k < 2h + r   the column to the left: sample ( -1 - r, -r + k )          — 2h + 1 + r samples from the corner
 *   ( 2w + 1 + r ) + ( 2h + 1 + r ) samples in all.  Availability and substitution are the caller's: the entry reads every one of them.
 * Original (d_org + org_off, int16): the block, compact (stride = w), as xGetHAD2SADs assumes.
 * Costs (d_cost + cost_off, uint32): 67 slots per item, indexed by mode; slot m receives the cost of every mode m of mode_mask, the other slots are not written.
 * Predictions (d_pred + pred_off, int16): the blocks of the modes of pred_mask, compact, in ascending mode order — popcount( pred_mask ) * w * h samples; nothing beyond them
 * is written.  d_pred may be NULL when no item has a pred_mask bit.
 * A mask is 67 bits: mode m is bit ( m & 31 ) of word m >> 5.
 * An item's results depend on nothing but the item: they are independent of the list's order and identical from run to run (integer arithmetic; the per-mode tile sums are
 * integer additions, which commute).  Items whose output regions overlap are the caller's error.
 * items_host is a HOST array, validated and uploaded by the call (the copy a previous launch may still read is waited for first).
 * VVHIP_E_ARG, before any launch and with nothing written: n < 0; w or h outside { 4, 8, 16, 32, 64 }; bit_depth outside 8..12; multi_ref_idx > 2; PLANAR (mode 0) requested with
 * multi_ref_idx != 0 (the reference never forms it, IntraSearch.cpp:308); mask bits >= 67; pred_mask not a subset of mode_mask; a negative offset; a non-zero rsv;
 * d_pred == NULL with a non-empty pred_mask; a missing array with n > 0.  n == 0 succeeds and launches nothing.
 * Still the caller's (out of scope here): xFillReferenceSamples itself (availability and substitution are syntax-bound); the MPM list, xFracModeBitsIntraLuma, lambda and
 * updateCandList; the decimated rounds of IntraSearch.cpp:229-292 (a mode's cost does not depend on the round: one call with the full mask serves every round — INTEGRATION.md);
 * MIP, ISP, BDPCM; chroma (vvhip_intra_chroma_modes_batch below); LMCS; hooking the entry into the running encoder.                                                           */
typedef struct
{
  uint8_t  w, h;                   /* 4, 8, 16, 32, 64                                                            */
  uint8_t  bit_depth;              /* 8..12                                                                       */
  uint8_t  multi_ref_idx;          /* 0, 1, 2: the reference line                                                 */
  int32_t  ref_off;                /* into d_ref: the unfiltered lines (layout above)                             */
  int32_t  org_off;                /* into d_org: the original block, compact                                     */
  int32_t  pred_off;               /* into d_pred: the predictions of pred_mask, ascending modes                  */
  int32_t  cost_off;               /* into d_cost: 67 slots, indexed by mode                                      */
  uint32_t mode_mask[3];           /* the modes to score                                                          */
  uint32_t pred_mask[3];           /* the modes whose prediction is written: a subset of mode_mask                */
  uint32_t rsv;                    /* 0                                                                           */
} vvhip_intra_item;                /* 48 bytes */
VVHIP_API int vvhip_intra_luma_modes_batch( vvhip_ctx* ctx, const vvhip_intra_item* items_host, int n, const int16_t* d_ref, const int16_t* d_org, int16_t* d_pred /* may be NULL */,
                                            uint32_t* d_cost );

/* ======================================================================================================================
 * Intra chroma mode pre-selection: the decision-free loop of IntraSearch::estIntraPredChromaQT (EncoderLib/IntraSearch.cpp:778-862) for a LIST of 4:2:0 chroma blocks in one
 * call — per block the Cb and the Cr prediction of up to eight candidate modes, each scored with min( 2 * SAD, HAD ), the two added (:827-843).  Only one cost per candidate
 * leaves the device, plus the predictions the caller asks for (the survivors are predicted again with the same two functions, :1975-1990).
 *   vvhip_intra_chroma_modes_batch <- per requested slot s of an item with mode m = cand[s], bit for bit, for Cb and for Cr:
 *     m in 0..66: IntraPrediction::initPredIntraParams for a chroma block (CommonLib/IntraPrediction.cpp:409-496: getWideAngle, the two angle tables, applyPDPC, angularScale;
 *       no reference filter and no interpolation flag, :461-468), predIntraAng's planar / DC / IntraPredSampleFilter (:353-383), xPredIntraAng (:518-681) with
 *       IntraPredAngleChroma_Core (:225-245: ( ( 32 - f ) * p0 + f * p1 + 16 ) >> 5 in 32-bit arithmetic, not clipped), the integer-slope copy, IntraHorVerPDPC (clipped)
 *       and IntraAnglePDPC;
 *     m in 67..69 (LM_CHROMA, MDLM_L, MDLM_T): the 4:2:0 branches of loadLMLumaRecPels (:1165-1406: the [1 2 1] row of isFirstRowOfCtu, the five-tap cross of
 *       sps->verCollocatedChroma, the default six-tap, leftPadding, abovePadding), xGetLMParameters (:1408-1605: the template lengths per mode with the clamps of :1487 and
 *       :1493 applied HERE to n_above_right / n_left_below, startPos / pickStep, the four picked pairs, the four-comparison sort, the rounded means, floorLog2, DivSigTable,
 *       add, the iShift < 1 clamp to +-15, diff == 0, and the default b = 1 << ( bit_depth - 1 ) when the mode has no template) and linearTransform( a, iShift, b, clip )
 *       (Buffer.cpp:253) with the clip range [0, 2^bit_depth - 1].  With sides >= 4 every available template yields four pairs: the cnt == 2 branch (:1544) cannot be
 *       reached.  The parameters read at most four template positions per mode, so only the inner w x h block and the picked positions are down-sampled.
 *     the cost: min( 2 * SAD, xGetHADs<false> ) of Cb plus the same of Cr (DF_SAD, DF_HAD on compact blocks).
 * Scope: 4:2:0, chroma sides of 4, 8, 16, 32, bit depths 8..12.
 * Reference lines (d_ref + ref_off[c], int16; c = 0 Cb, 1 Cr): the UNFILTERED lines of the component in vvhip_intra_luma_modes_batch's layout with multi_ref_idx 0 — corner,
 *   2w samples above, corner again, 2h samples to the left: ( 2w + 1 ) + ( 2h + 1 ) samples.  They are also the chroma neighbours xGetLMParameters picks (:1523, :1535).
 * Originals (d_org + org_off[c], int16): compact (stride = w).
 * Luma (d_luma + luma_off, int16, pitch luma_stride): the top-left sample of the collocated 2w x 2h area in a plane of RECONSTRUCTED luma.  With ( x, y ) counted from that
 *   sample, AR = min( n_above_right, h ) and LB = min( n_left_below, w ), the entry reads nothing outside
 *     the area                 columns 0 .. 2w - 1 of rows 0 .. 2h - 1                                      (any mode >= 67 requested)
 *       left available           plus column -1 of those rows; without it column 0 stands in (leftPadding)
 *       verCollocatedChroma      plus row -1 over columns 0 .. 2w - 1 when above is available; without it row 0 stands in (abovePadding)
 *     above available          columns -1 .. 2w - 1 (LM_CHROMA requested) or -1 .. 2( w + AR ) - 1 (MDLM_T requested) of
 *       first row of the CTU     row -1
 *       verCollocatedChroma      rows -3 .. -1   (columns 2i +- 1 only in row -2)
 *       otherwise                rows -2, -1
 *                              column -1 only when left is available (leftPadding otherwise: column 0)
 *     left available           columns -3 .. -1 of rows 0 .. 2h - 1 (LM_CHROMA requested) or 0 .. 2( h + LB ) - 1 (MDLM_L requested);
 *       verCollocatedChroma      plus row -1 of column -2 when above is available (abovePadding otherwise); the row below a position ( 2j + 1 ) is always read
 *   and inside these regions only the 2 x 3 or cross neighbourhoods of the positions xGetLMParameters picks.  A list without a mode >= 67 reads no luma: d_luma may be NULL.
 * Costs (d_cost + cost_off, uint32): 8 slots per item, indexed by candidate slot; slot s receives the cost of every slot of mode_mask, the others are not written.
 * Predictions (d_pred + pred_off[c], int16): the blocks of the slots of pred_mask, compact, in ascending slot order — popcount( pred_mask ) * w * h samples per component;
 *   nothing beyond them is written.  d_pred may be NULL when no item has a pred_mask bit.
 * An item's results depend on nothing but the item: independent of the list's order and identical from run to run (integer arithmetic; tile sums are integer additions).
 * Items whose output regions overlap are the caller's error.  items_host is a HOST array, validated and uploaded by the call.
 * VVHIP_E_ARG, before any launch and with nothing written: n < 0; w or h outside { 4, 8, 16, 32 }; bit_depth outside 8..12; a cand value above 69 in any slot, requested or
 * not; unknown flag bits; an odd n_above_right / n_left_below, one that takes its template beyond 2w / 2h samples ( n_above_right > w, n_left_below > h: the reference's
 * availability walk cannot produce it, and the component's line ends there ), a non-zero one without its side's flag; pred_mask not a subset of mode_mask; a negative
 * offset or luma_stride; a non-zero rsv byte; d_luma == NULL with a requested mode >= 67; d_pred == NULL with a pred_mask bit; items / d_ref / d_org / d_cost missing with
 * n > 0.  n == 0 succeeds and launches nothing.
 * Still the caller's: initIntraPatternChType / xFillReferenceSamples and the availability walk; the isLMCModeEnabled / lmChromaCheckDisable masks and the list of :810 (they
 * become mode_mask); the sort, the disable list and the RD loop behind them (vvhip::IntraChromaOps offers the sort); BDPCM; chroma sides of 2 and 64; 4:2:2 and 4:4:4;
 * LMCS chroma scaling; DM from a MIP luma block (the caller puts PLANAR into the slot).                                                                                        */
#define VVHIP_ICH_ABOVE           1   /* the row above the block is available (aboveIsAvailable, :1226)                     */
#define VVHIP_ICH_LEFT            2   /* the column to the left is available (leftIsAvailable, :1222)                       */
#define VVHIP_ICH_FIRST_ROW       4   /* the collocated luma row is the first row of its CTU (isFirstRowOfCtu, :1241)      */
#define VVHIP_ICH_VER_COLLOCATED  8   /* sps->verCollocatedChroma                                                           */
typedef struct
{
  uint8_t  w, h;                   /* the chroma size: 4, 8, 16, 32                                               */
  uint8_t  bit_depth;              /* 8..12                                                                       */
  uint8_t  flags;                  /* VVHIP_ICH_*                                                                 */
  uint8_t  n_above_right;          /* avaiAboveRightUnits * 2: chroma samples, even, <= w, 0 without ABOVE        */
  uint8_t  n_left_below;           /* avaiLeftBelowUnits * 2: chroma samples, even, <= h, 0 without LEFT          */
  uint8_t  mode_mask;              /* the slots of cand to score                                                  */
  uint8_t  pred_mask;              /* the slots whose predictions are written: a subset of mode_mask              */
  uint8_t  cand[8];                /* CU::getIntraChromaCandModes: 0..66 regular (the DM slot carries the mode DM */
                                   /* resolves to), 67 LM_CHROMA, 68 MDLM_L, 69 MDLM_T                            */
  int32_t  luma_off;               /* into d_luma: the top-left sample of the collocated 2w x 2h area             */
  int32_t  luma_stride;            /* the luma plane's pitch in samples                                           */
  int32_t  ref_off[2];             /* into d_ref: the unfiltered lines of Cb, Cr                                  */
  int32_t  org_off[2];             /* into d_org: the originals of Cb, Cr, compact                                */
  int32_t  pred_off[2];            /* into d_pred: the predictions of pred_mask of Cb, Cr, ascending slots        */
  int32_t  cost_off;               /* into d_cost: 8 slots, indexed by candidate slot                             */
  uint8_t  rsv[12];                /* 0                                                                           */
} vvhip_intra_chroma_item;         /* 64 bytes */
#ifdef __cplusplus
static_assert( sizeof( vvhip_intra_chroma_item ) == 64, "vvhip_intra_chroma_item is 64 bytes" );
#else
_Static_assert( sizeof( vvhip_intra_chroma_item ) == 64, "vvhip_intra_chroma_item is 64 bytes" );
#endif
VVHIP_API int vvhip_intra_chroma_modes_batch( vvhip_ctx* ctx, const vvhip_intra_chroma_item* items_host, int n, const int16_t* d_luma /* may be NULL */, const int16_t* d_ref,
                                              const int16_t* d_org, int16_t* d_pred /* may be NULL */, uint32_t* d_cost );

/* ======================================================================================================================
 * MMVD merge candidates of a LIST of CUs: the decision-free part of EncCu::addMmvdCandsToPruningList (EncoderLib/EncCu.cpp:2353-2453) — per CU up to 64 candidates
 * ( MmvdIdx::ADD_NUM: two base vectors, eight steps, four directions ), each predicted (luma only) and scored with DF_HAD or DF_HAD_fast against the original, in ONE launch.
 * Only the 64 costs of a CU leave the device: no prediction is written, and a base vector's reference window is fetched once for the candidates it can serve.
 *   vvhip_merge_mmvd_costs_batch <- per requested candidate val = position | step << 2 | baseIdx << 5 (CommonLib/CommonDef.h:390-409), bit for bit:
 *     1. MergeCtx::getMmvdDeltaMv (CommonLib/ContextModelling.cpp:261-342): offset = 1 << ( step + 2 ), << 2 under dis_frac (picHeader->disFracMMVD); the four directions
 *        ( +x, -x, +y, -y ); a bi-predicted base: the copy at equal POC distances, else CU::getDistScaleFactor (CommonLib/UnitTools.cpp:1354-1371) with Mv::scaleMv
 *        (CommonLib/Mv.h:182-187) onto the list whose reference is nearer, or the copy / mirror when either reference is long-term.
 *     2. MergeCtx::setMmvdMergeCandiInfo (:344-404): base + delta, Mv::clipToStorageBitDepth per used list, BcwIdx only for a bi-predicted base, and
 *        CU::restrictBiPredMergeCandsOne (UnitTools.cpp:3085-3097): a bi-predicted base on a CU with w + h == 12 is predicted from list 0 alone with the default weight.
 *     3. InterPrediction::motionCompensation (CommonLib/InterPrediction.cpp:454-527) with mcControl = 2 | 1 (no chroma; no BDOF on an MMVD CU, :479; no DMVR: mvRefine is off):
 *        xCheckIdenticalMotion (:292-324) — both references the same picture ( poc_delta equal ) and both stored vectors equal: list 0 alone —, then per used list clipMv
 *        (CommonLib/Mv.cpp:68-80, applied at :382) with pic_width, pic_height, ctu_size, position = mv >> 4, fraction = mv & 15.
 *     4. the luma prediction exactly as vvhip_pred_inter_batch_blend documents it: the 8-tap passes (m_lumaAltHpelIFilter at phase 8 under alt_hpel), one list: the clipped
 *        sample; two lists: addAvg, or addWeightedAvg for bcw_idx != 2.
 *     5. RdCost::xGetHADs<false> ( VVHIP_DF_HAD ) or xGetHADs<true> ( VVHIP_DF_HAD_FAST ) of original against prediction, the tile ladder of RdCost.cpp:1818-1938, as uint32.
 *   cost width: a cost is at most that of a 128 x 128 CU at 12 bits — 256 tiles of 8 x 8, each at most 64 * 64 * 4095 / 4 (64 coefficients of at most 64 * 4095, normalised
 *        by 4) — 256 * 4 193 280 = 1 073 479 680 < 2^32; the rectangular tiles and the 16 x 16 fast tile ( an 8 x 8 transform of averages, times 4 ) stay below the same figure.
 * Planes: the table of vvhip_pred_inter_batch (<= 16 planes, stride > 0 and even).  ref_off[b][l] is the CU's own position (vector zero) in plane ref_plane[b][l].
 * Original: d_org + org_off, row pitch org_stride.  Costs: d_cost + cost_off addresses 64 uint32 slots indexed by val; the slots of cand_mask ( bit val & 31 of word val >> 5 )
 * are written, the others are not touched.
 * An item's results depend on nothing but the item: independent of the list's order and identical from run to run (integer arithmetic; a CU larger than a tile of 512 samples
 * is cut into tiles whose partial sums are added as integers).  items_host is a HOST array, validated and uploaded by the call.  n == 0 succeeds and launches nothing.
 * Read bound: after the picture clip a block reads at most ctu_size + 8 + 3 samples left of / above the picture and at most 8 + w + 4 ( 8 + h + 4 ) samples right of / below
 * it — with CUs no larger than the CTU inside the reference encoder's own picture margin of ctu_size + 16 —, plus the 16 bytes of the aligned-dword rule.  The window the kernel stages around
 * a base vector's own (clipped) position is moved back into the same region, so it adds nothing to the bound.  Every plane of the table must be readable that far.
 * VVHIP_E_ARG with a message naming the entry, before any launch and with nothing written: n < 0; w or h not a power of two in 4..128, or w + h < 12; bit_depth outside 8..12;
 * func other than VVHIP_DF_HAD / VVHIP_DF_HAD_FAST; a base with both lists unused while one of its candidates is requested; a plane index outside the table; bcw_idx > 4;
 * ctu_size other than 32, 64, 128; a CU outside the picture; a negative org_off, cost_off or ref_off of a used list; a base vector outside the 18-bit storage range;
 * non-zero reserved bytes; planes / items / d_org / d_cost missing with n > 0.
 * Still the caller's: the merge list itself (getInterMergeCandidates, getInterMMVDMergeCandidates), xCalcPuMeBits and lambda; insertMergeItemToList and shrinkList, and the
 * visiting order of addMmvdCandsToPruningList / xCheckMMVDCand (EncCu.cpp:2361-2447, :4116-4158), which runs unchanged over ready costs ( vvhip::MergeMmvdOps::walk of the shim restates it for a caller that wants the order without the loop ); the isMvInRangeFPP skip under m_ifpLines; the candidates the
 * reference's SATD stage predicts WITH BDOF ( m_MMVD == 1 and step <= 2 under the conditions of InterPrediction.cpp:474-479: leave them out of the mask and take them through
 * vvhip_pred_inter_batch_ex ); regular, CIIP, affine and GPM candidates; chroma; explicit weighted prediction and reference picture resampling; the survivors' predictions
 * (vvhip_mmvd_candidate gives what vvhip_pred_inter_batch_blend needs); hooking the entry into the running encoder.
 * Bit depths 8..12.  Differences are scored at 32 bits.                                                                                                                         */
typedef struct
{
  int16_t  cu_x, cu_y;             /* the CU's luma position in the picture                                        */
  uint8_t  w, h;                   /* powers of two 4..128, w + h >= 12                                            */
  uint8_t  rsv0[2];                /* 0                                                                            */
  int32_t  org_off;                /* into d_org                                                                   */
  int32_t  cost_off;               /* into d_cost: 64 slots indexed by MmvdIdx::val                                */
  uint32_t cand_mask[2];           /* word b: the candidates of base vector b, bit position | step << 2            */
  int32_t  mv[2][2][2];            /* [base][list]( hor, ver ) in 1/16 sample: mmvdBaseMv[b][l].mv                 */
  int32_t  ref_off[2][2];          /* [base][list] the CU at vector zero in plane ref_plane[b][l]                  */
  int32_t  poc_delta[2][2];        /* [base][list] POC of the reference picture minus the current POC              */
  int8_t   ref_plane[2][2];        /* [base][list] index into the plane table, -1 = list not used                  */
  uint8_t  long_term[2];           /* per base: bit l = list l's reference is a long-term picture                  */
  uint8_t  bcw_idx[2];             /* per base: BcwIdx[b], 0..4 (applies when both lists are used)                 */
  uint8_t  alt_hpel[2];            /* per base: mmvdUseAltHpelIf[b]                                                */
  uint8_t  rsv[14];                /* 0                                                                            */
} vvhip_mmvd_item;                 /* 112 bytes */
#ifdef __cplusplus
static_assert( sizeof( vvhip_mmvd_item ) == 112, "vvhip_mmvd_item is 112 bytes" );
#else
_Static_assert( sizeof( vvhip_mmvd_item ) == 112, "vvhip_mmvd_item is 112 bytes" );
#endif
VVHIP_API int vvhip_merge_mmvd_costs_batch( vvhip_ctx* ctx, const vvhip_me_plane* planes_host, int n_planes, const vvhip_mmvd_item* items_host, int n,
                                            int pic_width, int pic_height, int ctu_size /* luma: 32, 64, 128 */, int bit_depth, int func, int dis_frac,
                                            const int16_t* d_org, int org_stride, uint32_t* d_cost );
/* One candidate of an item as the entry above predicts it, on the host (no device, no context): steps 1 to 3.  stored_mv is cu.mv after setMmvdMergeCandiInfo (the storage
 * clip, ( 0, 0 ) for an unused list); mv the vector after the picture clip, from which a vvhip_pred_item takes ref_off[b][l] + ( mv >> 4 ) and frac = mv & 15; ref_plane -1
 * for a list the prediction does not use (the base's own, bi-to-uni at w + h == 12, identical motion); bcw_idx 2 unless two lists are predicted; alt_hpel the base's.
 * Returns VVHIP_E_ARG for val outside 0..63, a base with both lists unused, a size outside the rule or a ctu_size outside the set.                                            */
typedef struct
{
  int32_t  mv[2][2];               /* per list ( hor, ver ) after clipMv                                           */
  int32_t  stored_mv[2][2];        /* per list ( hor, ver ) as cu.mv holds it                                      */
  int8_t   ref_plane[2];           /* -1: the list is not predicted                                                */
  uint8_t  bcw_idx;                /* 0..4                                                                         */
  uint8_t  alt_hpel;
} vvhip_mmvd_cand;                 /* 36 bytes */
VVHIP_API int vvhip_mmvd_candidate( const vvhip_mmvd_item* item, int val, int pic_width, int pic_height, int ctu_size, int dis_frac, vvhip_mmvd_cand* out );

#ifdef __cplusplus
}
#endif
#endif /* VVENC_HIP_H */
