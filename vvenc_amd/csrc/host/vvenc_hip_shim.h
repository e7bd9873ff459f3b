// vvenc_hip_shim.h — C++ host side ABOVE the C ABI (include/vvenc_hip.h): the table-shaped mirror of the reference's
// kernel objects for this path.  Same names, argument meaning and calling convention as the reference so that the
// encoder's control logic (EncCu / InterSearch / TrQuant / MCTF) can call through it unmodified:
//
//   vvhip::RdCost::m_afpDistortFunc[2][DF_TOTAL_FUNCTIONS], m_afpDistortFuncX5[2]   <- CommonLib/RdCost.h:117-121
//   vvhip::DistParam / CPelBuf / FpDistFunc / FpDistFuncX5                          <- CommonLib/RdCost.h:74-111, Buffer.h:149-159
//   vvhip::TCoeffOps (cpyResi/cpyCoeff/fastInvCore/fastFwdCore_2D/roundClip)        <- CommonLib/TrQuant_EMT.h:63-91
//   vvhip::QuantOps (xQuant/xDeQuant/xNeedRdoq core signatures)                     <- CommonLib/Quant.h:143-151
//   vvhip::MCTFOps  (m_motionErrorLumaInt8, m_motionErrorLumaFrac8[2], m_calcVar)   <- CommonLib/MCTF.h:160-170
//
// Two ways to call:
//   (1) table entry, one candidate per call — the reference's synchronous signature.  Pointers are HOST pointers; if they
//       fall inside a picture registered with registerPicture() the call only ships two offsets, otherwise the two blocks
//       are staged.  Correct everywhere and re-entrant (per-thread contexts), but one launch + one round trip per call: plumbing, not speed.
//   (2) batching: enqueue( DistParam ) -> ticket, flush(), result( ticket ) — what the thin shim in INTEGRATION.md uses
//       inside xTZSearch / xPatternRefinement (all positions of a ring / raster / refinement are known before the first
//       cost is needed) and for whole MCTF levels.
// Errors: like the reference there are no return codes; any failure throws vvhip::Exception (THROW, TypeDef.h:635-636).
// There is no CPU fallback: without a GPU create() throws.
#pragma once
#include <cstddef>
#include <cstdint>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../../include/vvenc_hip.h"

namespace vvhip {

using Pel        = int16_t;
using TCoeff     = int32_t;
using TCoeffSig  = int16_t;
using TMatrixCoeff = int16_t;
using Distortion = uint64_t;

struct Exception : std::runtime_error { using std::runtime_error::runtime_error; };

// DFunc, CommonLib/TypeDef.h:339-382 (same order: index = base + log2(width))
enum DFunc
{
  DF_SSE = 0, DF_SSE2, DF_SSE4, DF_SSE8, DF_SSE16, DF_SSE32, DF_SSE64, DF_SSE128,
  DF_SAD = 8, DF_SAD2, DF_SAD4, DF_SAD8, DF_SAD16, DF_SAD32, DF_SAD64, DF_SAD128,
  DF_HAD = 16, DF_HAD2, DF_HAD4, DF_HAD8, DF_HAD16, DF_HAD32, DF_HAD64, DF_HAD128,
  DF_HAD_2SAD = 24, DF_SAD_WITH_MASK = 25,
  DF_HAD_fast = 26, DF_HAD2_fast, DF_HAD4_fast, DF_HAD8_fast, DF_HAD16_fast, DF_HAD32_fast, DF_HAD64_fast, DF_HAD128_fast,
  DF_TOTAL_FUNCTIONS = 34
};

struct CPelBuf { const Pel* buf = nullptr; int stride = 0; unsigned width = 0, height = 0; };

class DistParam;
typedef Distortion ( *FpDistFunc )( const DistParam& );
typedef void ( *FpDistFuncX5 )( const DistParam&, Distortion*, bool );

class DistParam
{
public:
  CPelBuf      org, cur;
  FpDistFunc   distFunc  = nullptr;
  FpDistFuncX5 dmvrSadX5 = nullptr;
  int          bitDepth  = 0;
  int          subShift  = 0;
  int          compID    = 0;
  bool         applyWeight = false;
  Distortion   maximumDistortionForEarlyExit = ~0ull;   // honoured as in the SIMD rows: ignored (full sums are returned)
  const void*    wpCur   = nullptr;                     // weighted prediction is refused like the reference does (RdCost.cpp:303-306)
  const CPelBuf* orgLuma = nullptr;
  // GEO masked SAD (DF_SAD_WITH_MASK, RdCost.h:100-103): mask walks +stepX per sample, +maskStride*(1<<subShift)+maskStride2 per row
  const Pel*   mask        = nullptr;
  int          maskStride  = 0;
  int          stepX       = 0;
  int          maskStride2 = 0;
};
typedef Distortion ( *FpFxdWtdDistFunc )( const DistParam&, uint32_t fixedWeight );      // RdCost.h:117

// Worker contexts and the registry of host pictures mirrored in HBM.
//   * Every encoder worker thread gets its OWN context (HIP stream, staging areas) on the GPU it currently serves, created on first use and recycled when the
//     thread ends: table entries called concurrently by the reference's workers (one RdCost / TrQuant / Quant per worker, shared g_tCoeffOps / MCTF; SURVEY 8b
//     "Threading") never wait on each other on the host.
//   * Several GPUs in one process: selectGpu() binds the calling thread to a device (pictures are mapped to devices by the binding: one picture <-> one device,
//     SURVEY 8e); mirrors live in a per-GPU registry shared by that GPU's contexts; copyMirror() moves a picture between GPUs over xGMI.
//   * Host buffers the encoder recycles (picture planes) can be pinned in place once (pinHost) so that their transfers are asynchronous DMA at PCIe rate.
class Device
{
public:
  static Device& get();                      // the calling thread's context on its selected GPU (creates it on first use; throws without a GPU)
  static void    selectGpu( int gpu );       // bind the calling thread to a device (< 0: the default, $VVHIP_DEVICE or 0)
  static int     selectedGpu();              // the calling thread's binding as selectGpu set it (< 0: default) — scopes save and restore it
  static int     gpuCount();                 // devices visible to the process
  static int     defaultGpu();
  int        gpu() const { return m_gpu; }
  vvhip_ctx* ctx() const { return m_ctx; }
  // Mirror a host plane (sample (0,0) at `origin`, `margin` samples around a w x h picture, line pitch `stride`) in this GPU's HBM.
  // Re-register (or call updatePicture) after the host changed it (e.g. a reference picture was reconstructed).
  // findable = false: the mirror is used through its id only and never substituted for host pointers by the per-call table entries
  // (for pictures whose host buffer may be rewritten while the mirror is kept)
  int  registerPicture( const Pel* origin, int stride, int width, int height, int margin, bool findable = true, bool upload = true );
  void updatePicture( int id );
  // rows [y0, y0 + rows) of the picture (y relative to sample row 0; the margins are rows < 0 and >= height), whole padded lines: a reconstructed picture is
  // mirrored CTU row by CTU row as the encoder finishes (and border-extends) it.  Synchronous: other threads' contexts may read the rows when this returns.
  void updatePictureRows( int id, int y0, int rows );
  void unregisterPicture( int id );
  // the same picture on another GPU: allocates a mirror there and fills it device-to-device (hipMemcpyPeerAsync over xGMI); returns the id in `dst`'s registry
  int  copyMirrorTo( int id, Device& dst );
  struct Mirror { const Pel* hostBase; const Pel* hostEnd; const Pel* origin; int stride, width, height, margin; int16_t* dBase; int16_t* dOrigin; bool live; bool findable; bool reference; };
  // (find / findReference / mirror hand out COPIES taken under the registry's lock: another thread may register into a freed slot at any time; the device memory of a picture
  //  is released by unregisterPicture only — the caller that owns the picture's life cycle — and hipFree itself waits for the device's work in flight)
  struct Found { bool ok = false; Mirror m; explicit operator bool() const { return ok; } const Mirror* operator->() const { return &m; } const Mirror& operator*() const { return m; } };
  Found find( const Pel* p ) const;  // which registered picture of this GPU contains host pointer p (nullptr: none)
  // reference pictures (reconstructions mirrored row by row, setReference): looked up by the motion-search entry points only — never by the generic table entries,
  // which may be handed the same host buffer while it is being rewritten as the current picture's reconstruction
  void setReference( int id );
  Found findReference( const Pel* p ) const;
  Mirror mirror( int id ) const;
  void check( int rc, const char* what ) const;
  int16_t* staging( size_t bytes );          // grow-only device scratch of THIS context for unregistered (compact temp) buffers
  void*    stagingAux( size_t bytes );
  // pin a recycled host buffer in place (hipHostRegister, once per range; false: left pageable).  $VVHIP_PIN=0 switches pinning off.
  static bool pinHost( const void* p, size_t bytes );
  static void unpinAll();                    // before the owner frees the buffers (encoder close)
  // traffic over PCIe / calls since the process started (all contexts): what a binding prints per picture
  struct Stats { uint64_t uploadBytes, downloadBytes, uploads, downloads, contexts, residentReferenceCalls; };
  static Stats stats();
private:
  explicit Device( int gpu );
  ~Device();
  friend struct DevicePool;
  int        m_gpu = 0;
  vvhip_ctx* m_ctx = nullptr;
  int16_t* m_stage = nullptr; size_t m_stageBytes = 0;
  void* m_aux = nullptr; size_t m_auxBytes = 0;
};

// grow-only pinned host area owned by the shim (hipHostMalloc through the C ABI): where picture-sized results land before they are scattered into the encoder's buffers
class PinnedBuffer
{
public:
  Pel* get( size_t elems );                  // at least `elems` samples (contents are not preserved when it grows)
  ~PinnedBuffer() {}                         // (released with the process: HIP teardown order at exit is not ours to rely on)
private:
  Pel* m_p = nullptr; size_t m_elems = 0;
};

class RdCost
{
public:
  FpDistFunc   m_afpDistortFunc[2][DF_TOTAL_FUNCTIONS];
  FpDistFuncX5 m_afpDistortFuncX5[2];
  FpFxdWtdDistFunc m_fxdWtdPredPtr;            // fixWeightedSSE_Core, RdCost.cpp:1948-1982
  void create( bool enableOpt = true );      // both rows point at the HIP entries (bit-exact for every bit depth)

  // RdCost::setDistParam, CommonLib/RdCost.cpp:158-206 (subShiftMode / useHadamard semantics identical)
  void setDistParam( DistParam& dp, const CPelBuf& org, const Pel* refY, int refStride, int bitDepth, int compID, int subShiftMode = 0, int useHadamard = 0 );
  // RdCost::setDistParamGeo, CommonLib/RdCost.cpp:2036-2060
  void setDistParamGeo( DistParam& dp, const CPelBuf& org, const Pel* refY, int refStride, const Pel* mask, int maskStride, int stepX, int maskStride2, int bitDepth, int compID );
  // RdCost::getDistPart, CommonLib/RdCost.cpp:267-291 (luma; chroma weighting stays with the caller)
  Distortion getDistPart( const CPelBuf& org, const CPelBuf& cur, int bitDepth, DFunc eDFunc );

  // One stage of InterSearch::xPatternRefinement (EncoderLib/InterSearch.cpp:760-880) in ONE device call: the distortion of the original block
  // against the reference block interpolated at each of n (<= 9) displacements qpel[i] = (hor, ver) in quarter samples around refBlk
  // (= pattern->buf, the block at the best integer vector; the reference picture's margin must be readable, 6 samples are touched).
  // hadMode 0 SAD, 1 HAD, 2 HAD_fast (m_bUseHADME / m_fastHad); reduceTap = m_meReduceTap; returns false for shapes the device entry
  // does not take (the caller keeps its CPU path).  The MV-bit cost and the strict-< update stay with the caller's loop.
  bool patternRefineCosts( const CPelBuf& org, const Pel* refBlk, int refStride, const int ( *qpel )[2], int n, int bitDepth, int hadMode, int reduceTap, bool useAltHpelIf,
                           Distortion* out );

  // The candidate positions of one integer-search stage (a TZ diamond round, a raster row, a refinement star; InterSearch::xTZSearchHelp,
  // EncoderLib/InterSearch.cpp:410-438) in ONE device call: out[i] = func( org, refBase + xy[i][1]*refStride + xy[i][0] ) with the given
  // subShift.  Host buffers: the original block and the bounding window of the positions are staged per call.
  void distAtPositions( int func, const CPelBuf& org, const Pel* refBase, int refStride, int subShift, int bitDepth, const int ( *xy )[2], int n, Distortion* out );

  // ---- batching (2) ----
  int        enqueue( const DistParam& dp );         // dp.distFunc must be one of this object's table entries
  void       flush();                                // one launch per (function, block size, subShift, plane pair) group
  Distortion result( int ticket ) const { return m_results[ticket]; }
  void       clear() { m_pending.clear(); m_results.clear(); }
private:
  struct Pending { int func, w, h, subShift; Device::Mirror mo, mc; int32_t orgOff, curOff; };
  std::vector<Pending>    m_pending;
  std::vector<Distortion> m_results;
};

// TCoeffOps, CommonLib/TrQuant_EMT.h:63-91 — same member names and signatures, host pointers, one call = one (synchronous) launch.
struct TCoeffOps
{
  TCoeffOps();
  // the table's own ten slots, reference signatures (host pointers; dst of fastInvCore is accumulated into, as in the reference)
  void ( *cpyResi8 )( const TCoeff* src, Pel* dst, ptrdiff_t stride, unsigned width, unsigned height );
  void ( *cpyResi4 )( const TCoeff* src, Pel* dst, ptrdiff_t stride, unsigned width, unsigned height );
  void ( *cpyCoeff8 )( const Pel* src, ptrdiff_t stride, TCoeff* dst, unsigned width, unsigned height );
  void ( *cpyCoeff4 )( const Pel* src, ptrdiff_t stride, TCoeff* dst, unsigned width, unsigned height );
  void ( *fastInvCore[5] )( const TMatrixCoeff* it, const TCoeff* src, TCoeff* dst, unsigned lines, unsigned reducedLines, unsigned rows );
  void ( *fastFwdCore_2D[5] )( const TMatrixCoeff* it, const TCoeff* src, TCoeff* dst, unsigned lines, unsigned reducedLines, unsigned cutoff, int shift );
  void ( *fastFwdCore_1D[5] )( const TMatrixCoeff* it, const TCoeff* src, TCoeff* dst, unsigned lines, unsigned reducedLines, unsigned cutoff, int shift );
  void ( *roundClip4 )( TCoeff* dst, unsigned width, unsigned height, unsigned stride, const TCoeff outputMin, const TCoeff outputMax, const TCoeff round, const TCoeff shift );
  void ( *roundClip8 )( TCoeff* dst, unsigned width, unsigned height, unsigned stride, const TCoeff outputMin, const TCoeff outputMax, const TCoeff round, const TCoeff shift );
  // 2-D drivers with the signature of TrQuant::xT / xIT's inner work (TrQuant.cpp:481-655): what a batching integration calls instead
  // of two 1-D passes + copies, because both passes (and the Pel <-> TCoeff conversion) are fused on the device.
  void ( *fwdTransform2D )( const Pel* resi, ptrdiff_t stride, TCoeff* coef, unsigned width, unsigned height, int trTypeHor, int trTypeVer, int bitDepth );
  void ( *invTransform2D )( const TCoeff* coef, Pel* resi, ptrdiff_t stride, unsigned width, unsigned height, int trTypeHor, int trTypeVer, int bitDepth );
};
extern TCoeffOps g_tCoeffOps;

// Quant::xQuant/xDeQuant/xNeedRdoq (CommonLib/Quant.h:143-151) with the TransformUnit reduced to what QuantCore reads (width, height).
struct QuantOps
{
  QuantOps();
  void ( *xDeQuant )( const int maxX, const int maxY, const int scale, const TCoeffSig* const piQCoef, const size_t piQCfStride, TCoeff* const piCoef,
                      const int rightShift, const int inputMaximum, const TCoeff transformMaximum );
  bool ( *xNeedRdoq )( const TCoeff* pCoeff, size_t numCoeff, int quantCoeff, int64_t offset, int shift );
  void ( *xQuant )( unsigned width, unsigned height, const TCoeff* piCoef, TCoeffSig* piQCoef, TCoeff& uiAbsSum, int& lastScanPos, TCoeff* deltaU,
                    const int qp, const bool isIRAP, const int bitDepth, const TCoeff thrVal );
  // QuantCore's own argument list (Quant.cpp:132): what a trampoline for Quant::xQuant forwards (piQCoef compact, stride = width)
  void ( *xQuantCore )( unsigned width, unsigned height, const TCoeff* piCoef, TCoeffSig* piQCoef, TCoeff& uiAbsSum, int& lastScanPos, TCoeff* deltaU,
                        const int defaultQuantisationCoefficient, const int iQBits, const int64_t iAdd, const TCoeff thrVal );
  // the same for a TU whose coding unit has lfnstIdx > 0: QuantCore's first-coefficient-group rule (Quant.cpp:149-159)
  void ( *xQuantCoreLfnst )( unsigned width, unsigned height, const TCoeff* piCoef, TCoeffSig* piQCoef, TCoeff& uiAbsSum, int& lastScanPos, TCoeff* deltaU,
                             const int defaultQuantisationCoefficient, const int iQBits, const int64_t iAdd, const TCoeff thrVal, const int lfnstIdx );
};

// Joint Cb-Cr residual coding of a LIST of chroma TUs in one device chain (vvhip_ict_fwd_batch -> vvhip_tu_rdo_multi_strided -> vvhip_ict_inv_batch): what
// InterSearch::xEstimateInterResidualQT does per chroma TU around TrQuant::fwdTransformICT / transformNxN / invTransformNxN / invTransformICT
// (EncoderLib/InterSearch.cpp:3770-3960, CommonLib/TrQuant.cpp:95-164, :350-410).  Host blocks in, host results out; nothing but the list crosses twice.
struct JointCbCrOps
{
  struct Tu
  {
    const Pel* cb; const Pel* cr;      // the TU's two residual blocks, row pitch `stride`
    int stride, width, height;         // width / height independent powers of two, 2..64
    int mode;                          // signed ICT mode g_ictModes[jointCbCrSign][cbfMask] (Rom.cpp:1453), -3..3
    int qp;                            // the joint block's QpParam::Qp (chroma scale)
  };
  // dist (2 per TU): the pair distortion ( d1, d2 ) of fwdTransformICT, for every mode including 0 — a candidate list (the four masks selectICTCandidates tests on one
  // Cb / Cr pair are four Tus) is this call with every other output nullptr: only the forward entry runs.
  // With any other output the whole chain runs and every mode must be non-zero.  Outputs are compact, TU after TU in list order (row pitch = width): levels = the joint
  // block's quantised levels, recCb / recCr = both reconstructed residuals, stats = the joint TU's vvhip_tu_stats (abs_sum == 0: levels and reconstructions are zero),
  // sse (2 per TU) = the plain SSEs of recCb / recCr against cb / cr.  Any of them may be nullptr.  Transform DCT-2 both ways, as the chroma TU of an inter CU has it.
  // false: an argument this method itself rejects (n < 0, no TUs array); throws like every table entry when the device rejects the list.
  bool codeList( const Tu* tus, int n, int bitDepth, bool isIRAP, TCoeff thrVal, int64_t* dist, TCoeffSig* levels = nullptr, Pel* recCb = nullptr, Pel* recCr = nullptr,
                 vvhip_tu_stats* stats = nullptr, uint64_t* sse = nullptr );
};

// Sub-block transform (SBT) of a LIST of inter CUs in one device chain (vvhip_sbt_parts_batch -> vvhip_tu_rdo_multi_strided on the coded tiles -> vvhip_sbt_place_batch): what
// InterSearch::xCalcMinDistSbt computes per CU before any candidate is coded (EncoderLib/InterSearch.cpp:3272-3464) and what xEstimateInterResidualQT does per SBT
// candidate around transformNxN / invTransformNxN — the tiling of PartitionerImpl::getSbtTuTiling, the types of TrQuant::xSetTrTypes, the uncoded tile zero.
// Host blocks in, host results out.
struct SbtOps
{
  struct Cu
  {
    const Pel* y; const Pel* cb; const Pel* cr;      // the CU's three residual blocks (4:2:0), row pitches strideY / strideC
    int strideY, strideC, width, height;             // luma width / height: independent powers of two, 4..64
    int sbtAllowed;                                  // CU::checkAllowedSbt's bits (after the encoder's own clearing), non-zero
  };
  struct Cand
  {
    int cu;                                          // index into the CU list
    int mode;                                        // SBT mode 0..7 = 2 ( sbtIdx - 1 ) + sbtPos (TypeDef.h:284-291)
    int qp[3];                                       // QpParam::Qp of Y, Cb, Cr
  };
  // Per CU: parts (3 x 16: the unweighted part sums), est (9: m_estMinDistSbt), order (8: m_sbtRdoOrder) — a call with nCands == 0 runs the parts entry alone.
  // Per candidate, in list order: levels = the coded tile's quantised levels of Y, Cb, Cr one after the other (compact, row pitch = the tile's width), rec = the CU's
  // three reconstructed residual blocks one after the other (compact, row pitch = the block's width; the uncoded tile zero), stats (3) = the tiles' vvhip_tu_stats
  // (abs_sum == 0: levels and reconstruction are zero), sse (3) = the plain SSEs of the three blocks against the CU's residual.  Any output may be nullptr.
  // false: an argument this method itself rejects (negative counts, no arrays); throws like every table entry when the device rejects a list.
  bool codeList( const Cu* cus, int nCus, const Cand* cands, int nCands, double chromaWeight, int bitDepth, bool isIRAP, TCoeff thrVal, uint64_t* parts, uint64_t* est,
                 uint8_t* order, TCoeffSig* levels = nullptr, Pel* rec = nullptr, vvhip_tu_stats* stats = nullptr, uint64_t* sse = nullptr );
};

// DMVR refinement search of one CU in one device call (DMVR::xProcessDMVR, CommonLib/InterPrediction.cpp:1262-1392).
// What to do with the result: sub-blocks whose refinement is zero (and every PU that is not refined at all) can go straight into a prediction list
// (InterPredOps::predictList: luma and chroma, both lists, the average); a sub-block with a non-zero refinement goes into the same list with an extension record
// (vvhip_pred_ext): DMVR's padded-reference rule for its final prediction (DMVR::xFinalPaddedMCForDMVR, :1189-1225), and BDOF where the cost switch leaves it on.
struct DMVROps
{
  // ref0 / ref1: the reference samples at the CU's position displaced by the integer part of the (clipped) merge vectors MINUS 2 samples in
  // both directions (= what the reference hands to its bilinear xPredInterBlk, :1285-1302); frac* = the vectors' 1/16 fractions.
  // Sub-blocks dx x dy (<= 16) in raster order: mvd[2*num], mvd[2*num+1] = cu.mvdL0SubPu[num]; minCost[num] = the value compared with 2*dx*dy (:1386).
  bool refineCu( const Pel* ref0, int stride0, int fx0, int fy0, const Pel* ref1, int stride1, int fx1, int fy1, int cuWidth, int cuHeight, int dx, int dy, int bitDepth,
                 int16_t* mvd, uint64_t* minCost );
};

// Inter prediction of a list of prediction units in one device call (vvhip_pred_inter_batch): InterPredInterpolation::xPredInterBlk + xWeightedAverage
// (CommonLib/InterPrediction.cpp:768-867, :960-1010) for every component block of the list — luma and 4:2:0 chroma, one or two reference lists, any mix of sizes.
struct InterPredOps
{
  // refPlanes[k]: host pointer to sample (0,0) of a plane that lies inside a picture registered with Device::registerPicture (reference pictures: setReference) — its mirror is
  // read, nothing is uploaded but the list.  items: vvhip_pred_item records whose ref_plane indexes refPlanes, ref_off in samples at the picture's own line pitch, dst_off the
  // block's place in the compact outputs (row pitch = width).  pred: predElems samples.  org (may be nullptr; a registered picture like the references) + resi: also
  // org - pred, laid out like pred; org_off at the picture's line pitch.  false: a plane is not registered on this GPU (nothing was run).  Throws like every table entry when
  // the device rejects the list (vvhip::Exception with the entry's message).
  // ext (may be nullptr): vvhip_pred_ext records parallel to items — BDOF on true bi-predicted luma blocks, DMVR's padded reference for refined sub-blocks
  // (vvhip_pred_inter_batch_ex).
  // blend (may be nullptr): vvhip_pred_blend records parallel to items — BCW's block weights and GEO's per-sample blending of two hypotheses; a GEO item is a whole
  // component block of its CU (vvhip_pred_inter_batch_blend).
  // ciip (may be nullptr): vvhip_pred_ciip records parallel to items — the planar intra part and the weighting of CIIP CUs; an ON item is a whole component block of its
  // CU and its ref_off points into intraRef, a HOST array of intraRefElems samples (per item top[0 .. w + 2], left[0 .. h + 2], unfiltered) that is uploaded with the list
  // (vvhip_pred_inter_batch_ciip).  Explicit weighted prediction, IBC and CIIP in a picture with LMCS active stay with the caller.
  bool predictList( const Pel* const* refPlanes, int numPlanes, const vvhip_pred_item* items, int n, int bitDepth, Pel* pred, size_t predElems, const Pel* org = nullptr, Pel* resi = nullptr,
                    const vvhip_pred_ext* ext = nullptr, const vvhip_pred_blend* blend = nullptr, const vvhip_pred_ciip* ciip = nullptr, const Pel* intraRef = nullptr,
                    size_t intraRefElems = 0 );
  // The same for a list of affine CUs given by their control-point vectors (vvhip_pred_affine_batch: InterPredInterpolation::xPredAffineBlk, :1497-1839, PROF included):
  // items: vvhip_pred_affine_item records, one per component block, ref_off / org_off = the block's own position at the picture's line pitch; picWidth / picHeight / ctuSize
  // (luma) feed the picture clip.  Planes, outputs, residual and the return value as predictList.
  bool predictAffineList( const Pel* const* refPlanes, int numPlanes, const vvhip_pred_affine_item* items, int n, int picWidth, int picHeight, int ctuSize, int bitDepth,
                          Pel* pred, size_t predElems, const Pel* org = nullptr, Pel* resi = nullptr );
};

// ALF encoder statistics: whole-plane forms of AdaptiveLoopFilter::m_deriveClassificationBlk (CommonLib/AdaptiveLoopFilter.h,
// table entry set at AdaptiveLoopFilter.cpp:73) and EncAdaptiveLoopFilter::getPreBlkStats + m_getPreBlkStatsAccum (EncAdaptiveLoopFilter.h:438).
// rec points at sample (0,0) of a plane that carries a replicated border of >= 4 samples (the reference's extended m_tempBuf).
struct ALFOps
{
  // cls: 2 bytes per 4x4 block {classIdx, transposeIdx} = AlfClassifier, width/4 per row.  vbCTUHeight / vbPos = m_alfVBLumaCTUHeight / m_alfVBLumaPos.
  bool deriveClassification( const Pel* rec, int recStride, int width, int height, int bitDepth, int vbCTUHeight, int vbPos, uint8_t* cls );
  // per CTU and class one record of 183 floats: E[13][13], y[13], pixAcc (AlfCovariance with numBins 1); cls == nullptr: chroma (filterLength 5, one class);
  // init (optional, same layout): the values the float chains start from (statistics units that span several CTUs)
  bool getStatistics( const Pel* org, int orgStride, const Pel* rec, int recStride, int width, int height, int ctuSize, int filterLength,
                      const uint8_t* cls, int vbCTUHeight, int vbPos, float* out, const float* init = nullptr );
  // whole-picture form (4:2:0): every plane is uploaded once; classes of the luma blocks (picture raster) and the records of every statistics unit
  // (unitSize x unitSize luma samples, made of CTUs of ctuSize: EncAdaptiveLoopFilter::getStatisticsASU) for the enabled components.
  // stats[c]: [numUnits][c == 0 ? 25 : 1][183]
  bool pictureStatistics( const Pel* const rec[3], const int recStride[3], const Pel* const org[3], const int orgStride[3], int width, int height, int bitDepth,
                          int ctuSize, int unitSize, int vbLumaH, int vbLumaPos, int vbChromaH, int vbChromaPos, const bool enabled[3], uint8_t* cls, float* const stats[3] );
  // The same picture call IN BANDS, issued by the encoder's row tasks while the picture's SAO is still running elsewhere (EncoderLib/EncSlice.cpp:1135-1167: the statistics task
  // of a CTU row starts when the row below it has left SAO, i.e. when every sample the row's statistics read is final): statisticsBegin sets the picture up (any thread),
  // statisticsBand( u ) uploads the rows of statistics-unit row u (+ 4 border rows on either side) from the encoder's planes, runs classification + statistics of those units and
  // requests their download into pinned host memory — all asynchronous on the CALLING thread's stream, completion marked by an event; statisticsEnd (the thread that runs
  // EncAdaptiveLoopFilter::deriveFilter, EncoderLib/EncAdaptiveLoopFilter.cpp:1757) waits for the marks and hands out the host copies.  Same kernels on the same samples as
  // pictureStatistics (a band starts on a CTU boundary: every position relative to the virtual boundaries is the one it has in the picture): bit-identical records.
  // The caller serialises the three calls per object (the binding's per-ALF-object lock); bands may come in any order, each exactly once.
  bool statisticsBegin( const int recStride[3], const int orgStride[3], int width, int height, int bitDepth, int ctuSize, int unitSize, int vbLumaH, int vbLumaPos,
                        int vbChromaH, int vbChromaPos, const bool enabled[3] );
  int  statisticsBands() const { return m_band.rows; }                                           // unit rows of the picture begun last
  bool statisticsBand( int unitRow, const Pel* const rec[3], const Pel* const org[3] );
  bool statisticsEnd( const Pel* const rec[3], const uint8_t** cls, const float* stats[3] );      // false: not every band was issued (the caller falls back to pictureStatistics)
  // EncAdaptiveLoopFilter::getBlkStatsCcAlf per chroma CTU (4:2:0): org / slf = chroma planes (slf = ALF-filtered), recLuma with a replicated border >= 2;
  // one record per chroma CTU (E[0..6][0..6], y[0..6], pixAcc), vb* / picHeight in luma samples
  bool getStatisticsCcAlf( const Pel* orgC, int orgStride, const Pel* slfC, int slfStride, const Pel* recLuma, int recStride, int widthC, int heightC, int ctuSizeC,
                           int vbCTUHeight, int vbPos, int picHeight, float* out, const float* init = nullptr );
  // AdaptiveLoopFilter::m_filter7x7Blk / m_filter5x5Blk (CommonLib/AdaptiveLoopFilter.h:129-136) over the enabled CTUs of a plane, the way EncAdaptiveLoopFilter::reconstructCTU
  // drives them: src with a replicated border >= 4; dst receives the filtered samples of the CTUs with ctuSet[ctu] >= 0 (filter set of the CTU), the others keep theirs.
  // coeffSets / clipSets: [numSets][cls ? 25 : 1][13]; clipSets == nullptr selects the linear entries ([0]).  cls as written by deriveClassification (luma), nullptr for chroma.
  bool filterPlane( const Pel* src, int srcStride, Pel* dst, int dstStride, int width, int height, int ctuSize, int bitDepth, int filterLength, const uint8_t* cls,
                    const short* coeffSets, const short* clipSets, int numSets, const short* ctuSet, int vbCTUHeight, int vbPos );
  // whole-picture form (4:2:0) of the ALF reconstruction: luma with numLumaSets filter sets (lumaCtuSet == nullptr: luma off), both chroma planes with the numChromaSets
  // alternatives (chromaCtuSet[c] == nullptr: plane off); src[c] = the unfiltered planes with their replicated border, dst[c] = the reconstruction picture
  bool filterPicture( const Pel* const src[3], const int srcStride[3], Pel* const dst[3], const int dstStride[3], int width, int height, int bitDepth, int ctuSize,
                      const uint8_t* cls, const short* lumaCoeff, const short* lumaClip, int numLumaSets, const short* lumaCtuSet,
                      const short* chromaCoeff, const short* chromaClip, int numChromaSets, const short* const chromaCtuSet[2],
                      int vbLumaH, int vbLumaPos, int vbChromaH, int vbChromaPos );
  // AdaptiveLoopFilter::m_filterCcAlf (:124) over a chroma plane (4:2:0) as applyCcAlfFilterCTU drives it: dstC corrected in place; coeff [numFilters][8]; ctuFilter[ctu] 0 = off
  bool filterCcAlf( Pel* dstC, int dstStride, const Pel* recLuma, int recStride, int widthC, int heightC, int ctuSizeC, int bitDepth, const int16_t* coeff, int numFilters,
                    const uint8_t* ctuFilter, int vbCTUHeight, int vbPos );
  // One ALFOps object per EncAdaptiveLoopFilter: pictureStatistics leaves the unfiltered planes (with their border) and the block classes of ITS picture in HBM;
  // filterPicture, handed the same host planes afterwards (statistics -> derivation on the host -> filtering, EncAdaptiveLoopFilter.cpp:1440-1520, :1902), skips
  // their upload.  dropResident() when the host planes change without a statistics call.
  void dropResident() { m_res.valid = false; }
  ~ALFOps();
private:
  struct Resident { bool valid = false; int gpu = -1, width = 0, height = 0; const Pel* rec[3] = { nullptr, nullptr, nullptr }; int stride[3] = { 0, 0, 0 };
                    int16_t* d = nullptr; size_t elems = 0, off[3] = { 0, 0, 0 }; uint8_t* dCls = nullptr; size_t clsBytes = 0; };
  Resident m_res;
  struct Banded { bool open = false; int gpu = -1, rows = 0, issued = 0, width = 0, height = 0, bitDepth = 0, ctuSize = 0, unitSize = 0, vbLumaH = 0, vbLumaPos = 0, vbChromaH = 0, vbChromaPos = 0;
                  bool enabled[3] = { false, false, false }; int rp[3] = { 0, 0, 0 }, op[3] = { 0, 0, 0 }; size_t rOff[3] = { 0, 0, 0 }, oOff[3] = { 0, 0, 0 }, stOff[3] = { 0, 0, 0 };
                  int16_t* dOrg = nullptr; size_t orgElems = 0; char* dSt = nullptr; size_t stBytes = 0; char* host = nullptr; size_t hostBytes = 0, nCls = 0;
                  std::vector<void*> events; std::vector<char> done; };
  Banded m_band;
  PinnedBuffer m_down;          // download area of filterPlane
  bool filterPlaneImpl( const Pel* src, int srcStride, const int16_t* dSrcResident, const uint8_t* dClsResident, Pel* dst, int dstStride, int width, int height, int ctuSize, int bitDepth,
                        int filterLength, const uint8_t* cls, const short* coeffSets, const short* clipSets, int numSets, const short* ctuSet, int vbCTUHeight, int vbPos );
};

// SAO of a picture (vvhip_sao_stats / vvhip_sao_offset), 4:2:0: the statistics of EncSampleAdaptiveOffset::getCtuStatistics / getBlkStats
// (EncoderLib/EncSampleAdaptiveOffset.cpp:239-292, :810-929) for whole CTU rows, and SampleAdaptiveOffset::offsetCTU (CommonLib/SampleAdaptiveOffset.cpp:605-652) for the
// whole picture.  Availability: the picture's borders (filtering across slices and tiles on, one slice: what getStatistics assumes).  decideCtuParams — serial over CTUs,
// CABAC contexts and merge candidates — stays with the encoder: it reads the records statisticsEnd hands out and produces the parameters offsetPicture takes.
struct SaoOps
{
  // statisticsBegin sets the picture up (any thread): line pitches of the deblocked ("rec") and the original planes, luma size, bit depth, luma CTU size (8..128).
  // statisticsBand( r ) uploads CTU row r of the three planes plus one row above and below it from the encoder's planes, runs the statistics of that row's CTUs and requests
  // their download into pinned host memory — all asynchronous on the CALLING thread's stream, completion marked by an event.  In the encoder's pipeline a row's task may run
  // once the row below it is deblocked (the rows it reads are final then; the columns and rows a CTU leaves out are those that are not).  statisticsEnd waits for the marks:
  // out = int64 [ctus][3][5][2][32], byte-compatible with SAOStatData[5] per CTU and component; false: not every band was issued.
  // The caller serialises the calls per object; bands may come in any order, each exactly once.
  bool statisticsBegin( const int recStride[3], const int orgStride[3], int width, int height, int bitDepth, int ctuSize );
  int  statisticsBands() const { return m_rows; }
  bool statisticsBand( int ctuRow, const Pel* const rec[3], const Pel* const org[3] );
  bool statisticsEnd( const int64_t** out );
  // offsetCTU over the picture begun last: params [ctus][3] (vvhip_sao_param: type -1 = off), clip range [0, 2^bitDepth - 1].  src handed over with the planes the bands
  // uploaded (same pointers, every band issued) is not uploaded again.  dst[c] (line pitch dstStride[c]) receives the whole SAO'd plane; the copy stays in HBM
  // (residentPlane) for the ALF entries.  false: no picture begun, or one on another GPU.
  bool offsetPicture( const Pel* const src[3], const vvhip_sao_param* params, Pel* const dst[3], const int dstStride[3] );
  const int16_t* residentPlane( int c ) const { return m_dDst ? m_dDst + m_off[c] : nullptr; }      // device pointer, line pitch = recStride[c]
  ~SaoOps();
private:
  bool m_open = false, m_planesResident = false;
  int m_gpu = -1, m_rows = 0, m_issued = 0, m_width = 0, m_height = 0, m_bitDepth = 0, m_ctuSize = 0, m_ctusX = 0;
  int m_rp[3] = { 0, 0, 0 }, m_op[3] = { 0, 0, 0 };
  size_t m_off[3] = { 0, 0, 0 }, m_oOff[3] = { 0, 0, 0 }, m_recElems = 0, m_orgElems = 0, m_stBytes = 0, m_hostBytes = 0, m_dstElems = 0;
  const Pel* m_rec[3] = { nullptr, nullptr, nullptr };
  int16_t* m_dRec = nullptr; int16_t* m_dOrg = nullptr; int16_t* m_dDst = nullptr; char* m_dSt = nullptr; char* m_host = nullptr;
  std::vector<void*> m_events; std::vector<char> m_done;
};

// The deblocking filter of a picture (vvhip_deblock), 4:2:0: LoopFilter::xDeblockArea<EDGE_VER> / <EDGE_HOR> (CommonLib/LoopFilter.cpp:405-462) for whole CTU rows, on planes
// that are uploaded UNFILTERED and stay in HBM.  calcFilterStrengths — serial, syntax-bound — stays with the encoder: it fills the two LoopFilterParam maps a band takes.
struct DeblockOps
{
  // begin sets the picture up (any thread): line pitches of the reconstruction planes, luma size (multiples of 8), bit depth, luma CTU size (16..128, a power of two), the
  // slice's deblockingFilterBetaOffsetDiv2 / TcOffsetDiv2 per component.  The clip range is [0, 2^bitDepth - 1].
  // band( r ) uploads CTU row r of the three unfiltered planes from the encoder's planes and the row's records of both maps (lfpStride records per map row; the maps'
  // first record is that of the picture's first unit) and filters the row — its vertical edges, then its horizontal edges, the row's top CTU boundary included — all
  // asynchronous on the CALLING thread's stream, completion marked by an event.  Bands come top to bottom, each exactly once (the horizontal edges of a row read the
  // row above after ITS vertical edges: vvenc_hip.h, the caller's contract of vvhip_deblock); a band issued by another thread than the one before waits for that band's mark.
  // end waits for the marks and downloads the filtered planes: dst[c] (line pitch dstStride[c]; may be NULL: nothing is downloaded); false: not every band was issued.
  // The filtered planes stay in HBM (residentPlane) for the SAO entries.
  bool begin( const int stride[3], int width, int height, int bitDepth, int ctuSize, const int betaOffsetDiv2[3], const int tcOffsetDiv2[3] );
  int  bands() const { return m_rows; }
  bool band( int ctuRow, const Pel* const rec[3], const vvhip_lf_param* lfpVer, const vvhip_lf_param* lfpHor, int lfpStride );
  bool end( Pel* const dst[3], const int dstStride[3] );
  const int16_t* residentPlane( int c ) const { return m_dRec ? m_dRec + m_off[c] : nullptr; }      // device pointer, line pitch = stride[c]
  ~DeblockOps();
private:
  bool m_open = false;
  int m_gpu = -1, m_rows = 0, m_issued = 0, m_width = 0, m_height = 0, m_bitDepth = 0, m_ctuSize = 0;
  int m_rp[3] = { 0, 0, 0 }, m_beta[3] = { 0, 0, 0 }, m_tc[3] = { 0, 0, 0 };
  size_t m_off[3] = { 0, 0, 0 }, m_recElems = 0;
  int16_t* m_dRec = nullptr;
  const void* m_lastCtx = nullptr;
  std::vector<void*> m_events;
};

// The visual activity of the original picture for perceptual QP adaptation (vvhip_visact): the sums of the six high-pass entries of g_pelBufOP (CommonLib/Buffer.h:123-128)
// and of AreaBuf::getAvg for a list of areas, and what calcSpatialVisAct / calcTemporalVisAct / updateVisAct (EncoderLib/BitAllocation.cpp:84-204) make of them.  Everything
// in applyQPAdaptationSlice behind the sums — apprI3Log2, the glaring-colour offset, noise levels, peak smoothing, rate control — stays with the encoder.
struct VisAct      // EncoderLib/BitAllocation.h:57-77
{
  double   hpSpatAct = 0.0, hpTempAct = 0.0, hpVisAct = 0.0;
  unsigned spatAct = 0, tempAct = 0, visAct = 0, minAct = 0;
};
struct VisActOps
{
  // picture uploads the original planes of up to three components and their two previous originals (any thread; host line pitches per pointer; prev1[c] / prev2[c] may be
  // NULL; prev1[c] == cur[c] — the first picture — is not uploaded twice and takes the reference's pS0 == pSM1 bypass).  The planes stay in HBM (residentPlane) until the
  // next picture: any number of lists may be summed on them — the CTU list of slice initialisation, the whole planes of pre-processing, sub-CTU areas.
  // sums runs vvhip_visact on a list and downloads the records; false: no picture, one on another GPU, or n < 1.  An illegal list throws like every failed entry.
  bool picture( int nPlanes, const Pel* const cur[], const Pel* const prev1[], const Pel* const prev2[], const int curStride[], const int prev1Stride[], const int prev2Stride[],
                const int width[], const int height[], int bitDepth );
  bool sums( const vvhip_visact_area* areas, int n );
  int  count() const { return ( int ) m_areas.size(); }
  const uint64_t* record( int i ) const { return m_rec.data() + 4 * ( size_t ) i; }      // saAct, taAct, getAvg's accumulator, positions
  // the VisAct of area i as filterAndCalculateAverageActivity leaves it: order 1 is a frame rate <= 31 (the 1.15625 factor), order 2 one above it, order 0 leaves the
  // temporal fields 0; bit for bit the reference's doubles
  VisAct visAct( int i ) const;
  int    avg( int i ) const;      // AreaBuf<Pel>::getAvg of the mean rectangle; -1 where the area has none
  static VisAct fromRecord( const uint64_t rec[4], int width, int height, uint32_t bitDepth, bool isUHD, int order, bool prev1IsCur );
  const int16_t* residentPlane( int c, int which ) const { return m_d ? m_pl[c][which] : nullptr; }      // device pointer (which: 0 cur, 1 prev1, 2 prev2), line pitch = width[c]
  ~VisActOps();
private:
  bool m_open = false;
  int m_gpu = -1, m_n = 0, m_bitDepth = 0;
  int m_w[3] = { 0, 0, 0 }, m_h[3] = { 0, 0, 0 };
  bool m_same[3] = { false, false, false };
  size_t m_elems = 0, m_outRecs = 0;
  int16_t* m_d = nullptr; const int16_t* m_pl[3][3] = { { nullptr, nullptr, nullptr }, { nullptr, nullptr, nullptr }, { nullptr, nullptr, nullptr } };
  uint64_t* m_dOut = nullptr;
  std::vector<vvhip_visact_area> m_areas;
  std::vector<uint64_t> m_rec;
};

// Intra luma mode pre-selection (vvhip_intra_luma_modes_batch): the predict-and-score loop of IntraSearch::xEstimateLumaRdModeList (EncoderLib/IntraSearch.cpp:171-335) for a
// list of blocks — per block the reference lines xFillReferenceSamples left, per mode initPredIntraParams, predIntraAng and DF_HAD_2SAD against the original.  The MPM list,
// the mode bits, lambda and updateCandList stay with the encoder: it reads the costs (and the predictions it asked for) and decides.
struct IntraOps
{
  // begin empties the list.  add appends one luma block (any thread that later calls run): refBuf is the UNFILTERED reference buffer as
  // m_refBuffer[COMP_Y][PRED_BUF_UNFILTERED] holds it for multiRefIdx — the top row at refBuf, the left row at refBuf + refStride, refStride >= 2 width + 1 + multiRefIdx
  // (m_refBufferStride) — piOrg / orgStride the original block (copied compact); intraDir[ numModes ] the modes to score, predDir[ numPred ] those of them whose prediction is
  // wanted (may be NULL / 0).  -> the block's index, -1 for an argument the entry would refuse on sight (size, bit depth, multiRefIdx, a mode beyond 66, PLANAR with
  // multiRefIdx != 0, a predDir that is not scored).
  // run uploads lines and originals, runs the entry on the calling thread's stream and downloads costs and predictions; false: an empty list.
  void begin();
  int  add( const Pel* refBuf, int refStride, const Pel* piOrg, int orgStride, int width, int height, int bitDepth, int multiRefIdx, const uint8_t* intraDir, int numModes,
            const uint8_t* predDir = nullptr, int numPred = 0 );
  bool run();
  int  count() const { return ( int ) m_items.size(); }
  bool scored( int i, int intraDir ) const { const vvhip_intra_item& q = m_items.at( i ); return intraDir >= 0 && intraDir < 67 && ( ( q.mode_mask[intraDir >> 5] >> ( intraDir & 31 ) ) & 1 ); }
  uint32_t cost( int i, int intraDir ) const { return m_cost.at( ( size_t ) 67 * i + intraDir ); }      // min( HAD, 2 SAD ) of a scored mode (Distortion)
  const Pel* pred( int i, int intraDir ) const;      // the prediction block, compact (stride = width); NULL where it was not asked for
  ~IntraOps();
private:
  bool m_ran = false;
  int m_gpu = -1;
  size_t m_devBytes = 0;
  char* m_d = nullptr;
  std::vector<vvhip_intra_item> m_items;
  std::vector<Pel> m_ref, m_org, m_pred;
  std::vector<uint32_t> m_cost;
};

// Intra chroma mode pre-selection (vvhip_intra_chroma_modes_batch): the predict-and-score loop of IntraSearch::estIntraPredChromaQT (EncoderLib/IntraSearch.cpp:778-862) for a
// list of 4:2:0 chroma blocks — per block the Cb and the Cr prediction of the candidate modes (regular modes from the components' reference lines, CCLM / MDLM from the
// reconstructed luma) and satdSortedCost.  Availability, the candidate list, the LM masks and everything behind the sort stay with the encoder; select() restates the sort and
// the disable list for it.
struct IntraChromaOps
{
  // begin empties the list and forgets the luma plane.  The luma plane of the list is EITHER a host plane (setLuma: recoLuma points at sample ( 0, 0 ) of a width x height
  // picture of reconstructed luma with line pitch stride; uploaded by run) OR a plane that is resident on the device (setResidentLuma: a device pointer at sample ( 0, 0 ),
  // e.g. the reconstruction DeblockOps / SaoOps / ALFOps keep resident; nothing is uploaded).  A list without a mode >= 67 needs neither.
  // add appends one chroma block (any thread that later calls run): refCb / refCr are the UNFILTERED reference buffers of the two components as
  // m_refBuffer[compID][PRED_BUF_UNFILTERED] holds them — the top row at ref, the left row at ref + refStride, refStride >= 2 width + 1 (m_refBufferStride[compID]) —
  // orgCb / orgCr the original blocks at the picture pitch orgStride (copied compact), ( lumaX, lumaY ) the luma position of the block (chromaArea.lumaPos()), width x height
  // the chroma size.  aboveAvail / leftAvail / avaiAboveRightUnits / avaiLeftBelowUnits are loadLMLumaRecPels' four availability numbers (units of two chroma samples, NOT yet
  // clamped: the device applies xGetLMParameters' clamps), firstRowOfCtu and verCollocatedChroma its two other inputs.  cand[8] is CU::getIntraChromaCandModes with the DM slot
  // resolved (getFinalIntraMode; PLANAR for a MIP luma block); modeMask the slots to score (bit s = slot s: what :806-813 does not skip), predMask those whose predictions
  // are wanted.  -> the block's index, -1 for an argument the entry would refuse on sight or a block whose luma footprint leaves the plane.
  // run uploads what the list needs, runs the entry on the calling thread's stream and downloads costs and predictions; false: an empty list.
  void begin();
  void setLuma( const Pel* recoLuma, int stride, int width, int height );
  void setResidentLuma( const int16_t* dLuma, int stride, int width, int height );
  int  add( const Pel* refCb, int refStrideCb, const Pel* refCr, int refStrideCr, const Pel* orgCb, const Pel* orgCr, int orgStride, int lumaX, int lumaY, int width, int height,
            int bitDepth, bool aboveAvail, bool leftAvail, int avaiAboveRightUnits, int avaiLeftBelowUnits, bool firstRowOfCtu, bool verCollocatedChroma, const uint8_t cand[8],
            unsigned modeMask, unsigned predMask = 0 );
  bool run();
  int  count() const { return ( int ) m_items.size(); }
  bool scored( int i, int slot ) const { return slot >= 0 && slot < 8 && ( ( m_items.at( i ).mode_mask >> slot ) & 1 ); }
  uint32_t cost( int i, int slot ) const { return m_cost.at( ( size_t ) 8 * i + slot ); }      // satdSortedCost of a scored slot; 0 for a slot that was skipped, as in the reference
  const Pel* pred( int i, int comp, int slot ) const;      // comp 0 Cb, 1 Cr: the prediction block, compact (stride = width); NULL where it was not asked for
  // the reference's selection from eight costs: the stable exchange sort of IntraSearch.cpp:847-857 over all eight slots (skipped slots carry cost 0) and the disable list of
  // :859-862 — the last NUM_CHROMA_MODE >> ( reduceIntraChromaModesFullRD ? 1 : 2 ) modes of the sorted list.  sortedModes[8] receives satdModeList after the sort,
  // disabled[70] is indexed by mode ( modeDisable ).  Host arithmetic only: needs no device.
  static void select( const uint32_t cost[8], const uint8_t cand[8], bool reduceIntraChromaModesFullRD, uint8_t sortedModes[8], bool disabled[70] );
  void select( int i, bool reduceIntraChromaModesFullRD, uint8_t sortedModes[8], bool disabled[70] ) const { select( &m_cost.at( ( size_t ) 8 * i ), m_items.at( i ).cand, reduceIntraChromaModesFullRD, sortedModes, disabled ); }
  ~IntraChromaOps();
private:
  bool m_ran = false;
  int m_gpu = -1;
  size_t m_devBytes = 0;
  char* m_d = nullptr;
  const Pel* m_hostLuma = nullptr; const int16_t* m_devLuma = nullptr;
  int m_lumaStride = 0, m_lumaW = 0, m_lumaH = 0;
  std::vector<vvhip_intra_chroma_item> m_items;
  std::vector<Pel> m_ref, m_org, m_pred;
  std::vector<uint32_t> m_cost;
};

// MMVD merge candidates (vvhip_merge_mmvd_costs_batch): the predict-and-score part of EncCu::addMmvdCandsToPruningList (EncoderLib/EncCu.cpp:2353-2453) for a list of CUs —
// per CU and requested candidate MergeCtx::setMmvdMergeCandiInfo, the luma prediction of motionCompensation with mcControl = 2 | 1 and DF_HAD / DF_HAD_fast against the
// original.  The merge list, xCalcPuMeBits, lambda, insertMergeItemToList / shrinkList, the isMvInRangeFPP skip and the candidates predicted WITH BDOF stay with the encoder;
// walk() restates the visiting order for it over ready costs and bdofCands() names the candidates to leave out of the mask.
struct MergeMmvdOps
{
  // one base vector as MergeCtx holds it (CommonLib/ContextModelling.h:521-533): mmvdBaseMv[b][l].mv, the reference picture behind mmvdBaseMv[b][l].refIdx — refPlane[l] is the
  // host pointer to luma sample ( 0, 0 ) of a picture registered with Device::registerPicture (nullptr: list l unused), refPoc[l] its POC, longTerm[l] its isLongTerm —,
  // BcwIdx[b] and mmvdUseAltHpelIf[b]
  struct Base { int mvHor[2] = { 0, 0 }, mvVer[2] = { 0, 0 }; const Pel* refPlane[2] = { nullptr, nullptr }; int refPoc[2] = { 0, 0 }; bool longTerm[2] = { false, false }; int bcwIdx = 2; bool altHpel = false; };
  // begin empties the list and fixes what one call fixes: the picture's luma size and CTU size (the picture clip), the bit depth, the current POC, picHeader->disFracMMVD,
  // hadFast ( true: DF_HAD_fast, false: DF_HAD — the two values EncCu.cpp:1961 chooses from ) and orgPlane, the host pointer to luma sample ( 0, 0 ) of the original picture
  // (registered like the references).
  // add appends one CU at luma position ( cuX, cuY ) with its two base vectors and the candidates to score (bit MmvdIdx::val of mask).  -> the CU's index, -1 for what the entry
  // would refuse on sight (size, position, bcwIdx, a requested candidate of a base without lists, a vector outside the storage range) or a 17th distinct reference plane.
  // run resolves the planes' mirrors, runs the entry on the calling thread's stream and downloads the costs; false: an empty list, or a plane that is not registered on this
  // GPU (nothing was run).
  void begin( int picWidth, int picHeight, int ctuSize, int bitDepth, int curPoc, bool disFracMMVD, bool hadFast, const Pel* orgPlane );
  int  add( int cuX, int cuY, int width, int height, const Base base[2], uint64_t mask );
  bool run();
  int  count() const { return ( int ) m_items.size(); }
  bool scored( int i, int val ) const { return val >= 0 && val < 64 && ( ( m_items.at( i ).cand_mask[val >> 5] >> ( val & 31 ) ) & 1 ); }
  uint32_t dist( int i, int val ) const { return m_cost.at( ( size_t ) 64 * i + val ); }      // the Hadamard sum of a scored candidate (Distortion); 0 where it was not scored
  const uint32_t* dists( int i ) const { return &m_cost.at( ( size_t ) 64 * i ); }            // the CU's 64 slots, indexed by MmvdIdx::val

  // The candidates of a CU that the reference's SATD stage predicts WITH BDOF — to be left out of the mask and taken through vvhip_pred_inter_batch_ex: none unless
  // sps->BDOF && !picHeader->disBdofFlag ( bdofEnabled ) and m_MMVD == 1; then, per base, the steps 0 .. 2 ( mccNoBdof is off for them, EncCu.cpp:2225 ) where
  // InterPrediction.cpp:474-479 holds: both lists used and not cut to one ( width + height != 12 ), neither reference long-term, curPoc - refPoc[0] == refPoc[1] - curPoc,
  // min( width, height ) >= 8, width * height >= 128 and ( !sps->BCW ( bcwEnabled ) || bcwIdx == 2 ).  Host arithmetic only.
  static uint64_t bdofCands( int width, int height, const Base base[2], int curPoc, int mmvd, bool bdofEnabled, bool bcwEnabled );

  // The visiting order of addMmvdCandsToPruningList with xCheckMMVDCand (EncCu.cpp:2361-2447, :4116-4158) over costs that are already there.  Host arithmetic only.
  struct WalkCfg
  {
    int mmvd = 3;                       // m_MMVD, 1 .. 4
    int mmvdDisNum = 6;                 // m_MmvdDisNum
    int numValidMergeCand = 2;          // mergeCtx.numValidMergeCand: one base vector only when it is 1
    int mrgCnd0 = 0, mrgCnd1 = 1;       // m_MMVD == 4: mergeIdx of the incoming list's entry 0 and of its entry 1 ( of entry 0 again when the list holds one item )
    int maxTrackingNum = 0;             // the list's m_maxTrackingNum (EncCu.cpp:4444-4471); <= 0: the list may grow without bound
    uint64_t skip = 0;                  // candidates the caller's isMvInRangeFPP test drops (m_ifpLines): visited by xCheckMMVDCand, neither tested nor counted
  };
  // dist[64]: the candidates' distortions; bitsCost[64]: the caller's fracBits * lambda per candidate, so that a candidate's cost is ( double ) dist + bitsCost as
  // calcLumaCost4MergePrediction forms it; listCost[ nList ], nList >= 1: the costs of the incoming m_mergeItemList in its own (ascending) order — the reference re-reads entry
  // nList - 1 of the list after every insertion, so the walk inserts each tested candidate's cost as insertMergeItemToList does.  tested[64] receives the MmvdIdx::val of
  // the candidates the reference would have predicted and scored, in order -> their number.  bestCostOffset / bestCostMerge / bestDir (may be NULL) receive the three
  // running values as the loop leaves them.
  static int walk( const uint32_t dist[64], const double bitsCost[64], const double* listCost, int nList, const WalkCfg& cfg, uint8_t tested[64],
                   double* bestCostOffset = nullptr, double* bestCostMerge = nullptr, int* bestDir = nullptr );
  ~MergeMmvdOps();
private:
  bool m_ran = false;
  int m_gpu = -1, m_picW = 0, m_picH = 0, m_ctu = 0, m_bitDepth = 0, m_curPoc = 0, m_func = 0;
  bool m_disFrac = false;
  const Pel* m_org = nullptr;
  size_t m_devBytes = 0;
  char* m_d = nullptr;
  std::vector<const Pel*> m_planes;
  std::vector<vvhip_mmvd_item> m_items;
  std::vector<uint32_t> m_cost;
};

// MCTF table, CommonLib/MCTF.h:160-170
struct MCTFOps
{
  MCTFOps();
  int ( *m_motionErrorLumaInt8 )( const Pel* org, const ptrdiff_t origStride, const Pel* buf, const ptrdiff_t buffStride, const int w, const int h, const int besterror );
  int ( *m_motionErrorLumaFrac8[2] )( const Pel* org, const ptrdiff_t origStride, const Pel* buf, const ptrdiff_t buffStride, const int w, const int h,
                                      const int16_t* xFilter, const int16_t* yFilter, const int bitDepth, const int besterror );
  double ( *m_calcVar )( const Pel* org, const ptrdiff_t origStride, const int w, const int h );
  // whole-picture replacement of MCTF::motionEstimationMCTF (MCTF.cpp:666-707) for pictures registered with Device:
  // out[r] receives ceil(w/unit) x ceil(h/unit) vvhip_mv (== MotionVector, MCTF.h:72-82) for reference r
  void motionEstimation( int curPicId, const int* refPicIds, int nRefs, int bitDepth, int unitSize, int mctfSpeed, bool addLevel, vvhip_mv** out );
  // whole-picture replacement of MCTF::bilateralFilter (MCTF.cpp:1489-1552) for planes registered with Device, one id per
  // component plane (numComp 1 or 3, 4:2:0): orgIds[c], refIds[3*r + c]; mvs[r] = final-level motion field of reference r (host, as
  // motionEstimation returned it); refStrengths[r] = m_refStrengths[row][index] (MCTF.cpp:112-117,1480); out[c] receives the filtered plane.
  // Equals the reference's scalar row (its x86 row is within +-1 by the reference's own unit test).
  void bilateralFilter( const int* orgIds, const int* refIds, int nRefs, const vvhip_mv* const* mvs, const double* refStrengths, int qp, int bitDepth, int unitSize,
                        bool lowResFltApply, double overallStrength, int numComp, Pel* const* out, const int* outStride );
};

// InterpolationFilter, CommonLib/InterpolationFilter.h:70-155: the function-pointer tables of the separable
// sub-pel filter with the reference's signatures (host pointers, one synchronous launch per call) and the two public dispatchers.
struct ClpRng { int bd; static constexpr int min() { return 0; } int max() const { return ( 1 << bd ) - 1; } };      // CommonDef.h:542-548
typedef int16_t TFilterCoeff;
class InterpolationFilter
{
public:
  InterpolationFilter();
  void initInterpolationFilter( bool /*enable*/ ) {}
  // [tap index: 0 = 8, 1 = 4, 2 = 2 (bilinear), 3 = 6 taps][isFirst][isLast]
  void ( *m_filterHor[4][2][2] )( const ClpRng& clpRng, Pel const* src, int srcStride, Pel* dst, int dstStride, int width, int height, TFilterCoeff const* coeff );
  void ( *m_filterVer[4][2][2] )( const ClpRng& clpRng, Pel const* src, int srcStride, Pel* dst, int dstStride, int width, int height, TFilterCoeff const* coeff );
  void ( *m_filterCopy[2][2] )( const ClpRng& clpRng, Pel const* src, int srcStride, Pel* dst, int dstStride, int width, int height, bool biMCForDMVR );
  // fused two-pass entries [0 = 8 taps, 1 = 4 taps (, 2 = 2 taps)][isLast]: horizontal pass (14-bit) then vertical pass
  void ( *m_filter4x4[2][2] )( const ClpRng& clpRng, Pel const* src, int srcStride, Pel* dst, int dstStride, int width, int height, TFilterCoeff const* coeffH, TFilterCoeff const* coeffV );
  void ( *m_filter8xH[3][2] )( const ClpRng& clpRng, Pel const* src, int srcStride, Pel* dst, int dstStride, int width, int height, TFilterCoeff const* coeffH, TFilterCoeff const* coeffV );
  void ( *m_filter16xH[3][2] )( const ClpRng& clpRng, Pel const* src, int srcStride, Pel* dst, int dstStride, int width, int height, TFilterCoeff const* coeffH, TFilterCoeff const* coeffV );
  // luma dispatch of InterpolationFilter::filterHor / filterVer (InterpolationFilter.cpp:557-661; nFilterIdx 0)
  void filterHor( Pel const* src, int srcStride, Pel* dst, int dstStride, int width, int height, int frac, bool isLast, const ClpRng& clpRng, bool useAltHpelIf = false, int reduceTap = 0 );
  void filterVer( Pel const* src, int srcStride, Pel* dst, int dstStride, int width, int height, int frac, bool isFirst, bool isLast, const ClpRng& clpRng, bool useAltHpelIf = false, int reduceTap = 0 );
  // tap rows as the reference's static tables hold them (8 entries for the luma sets, 4 for chroma)
  static const TFilterCoeff* lumaFilter( int frac );          // m_lumaFilter[frac]
  static const TFilterCoeff* lumaFilter4x4( int frac );       // m_lumaFilter4x4[frac]
  static const TFilterCoeff* lumaAltHpelIFilter();            // m_lumaAltHpelIFilter
  static const TFilterCoeff* chromaFilter( int frac32 );      // m_chromaFilter[frac32]
};

} // namespace vvhip
