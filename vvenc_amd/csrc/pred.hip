// pred.hip — inter prediction of a LIST of prediction units: luma and 4:2:0 chroma, uni- and bi-predicted, every block size in one launch,
// optionally with the residual against the original.
//
// Reference behaviour (all integer, bit-exact):
//   InterPredInterpolation::xPredInterBlk (fractions, which passes run)   CommonLib/InterPrediction.cpp:768-867
//   InterPredInterpolation::xWeightedAverage -> AreaBuf<Pel>::addAvg        :960-1010, CommonLib/Buffer.cpp:549-575 (core :129-141)
//   InterpolationFilter::filter<N,isVertical,isFirst,isLast> / filterCopy   CommonLib/InterpolationFilter.cpp:356-441, :255-333
//
// One wave takes one unit of the schedule the host derives from the list: a tile of a large block, or several whole small blocks of ONE size class
// (a 4x4 luma block occupies 4 lanes, a 2x2 chroma block 2: sixteen / thirty-two blocks per wave).  Per reference list a lane group
//   1. stages the tile's reference window in LDS (aligned dwords from HBM; only the rows / columns the two fractions reach),
//   2. runs the horizontal pass over the window rows into a 14-bit intermediate in LDS (isFirst, !isLast),
//   3. runs the vertical pass from it into registers (!isFirst; isLast for a uni-predicted block).
// A zero fraction takes the same two passes with the one-tap set { 64 }: the copy forms of the reference give the same values, and so does its single-pass dispatch for a
// vector with one zero fraction (floor( ( floor( a / 4 ) + b ) / c ) = floor( ( a + 4 b ) / ( 4 c ) ) for integers — the rule interp.hip's refinement kernel already relies on).
// A bi-predicted block keeps list 0's 14-bit block in registers while list 1 goes through the same LDS, then averages: the two intermediates never leave the wave.
// Waves synchronise with themselves only (no workgroup barrier); a workgroup is four independent waves.
//
// Items with an extension record (vvhip_pred_inter_batch_ex) run in predListExKernel, the same body with two additions:
//   DMVR's padded reference   DMVR::xCopyAndPad :1088-1130, xFinalPaddedMCForDMVR :1189-1225: step 1 clamps every sample's coordinates to the window prefetched round the START vector.
//   BDOF                      xSubPuBDOF :326-357, xPredInterBlk :822-831 + :868-901, xApplyBDOF :911-958, gradFilterCore :114-155, calcBDOFSumsCore :157-186,
//                             xFpBiDirOptFlowCore :607-661, addBDOFAvgCore :63-86: a lane group per 16x16 / 16x8 / 8x16 unit; each list's 14-bit block goes to LDS inside its ring
//                             of integer samples, the lanes take the gradients of their own samples, a lane pair per 4x4 unit sums the 6x6 window, the offsets come back by lane read.
// Items with a blend record (vvhip_pred_inter_batch_blend) run in predListBlendKernel, the same body with another combine step: both hypotheses go to the 14-bit block and
//   ClipPel( ( w0 * s0 + ( 8 - w0 ) * s1 + offset ) >> shift ), shift = headroom + 3, offset = ( 1 << ( shift - 1 ) ) + ( IF_INTERNAL_OFFS << 3 )
//   BCW   AreaBuf<Pel>::addWeightedAvg CommonLib/Buffer.cpp:509-546 (core :143-156), getBcwWeight Rom.cpp:1150-1163: w0 = 8 - { -2, 3, 4, 5, 10 }[bcw_idx] for the whole block
//   GEO   InterpolationFilter::xWeightedGeoBlk CommonLib/InterpolationFilter.cpp:1005-1064, tables Rom.cpp:1304-1382: w0 per sample, a clamped line in ( x, y ) whose three
//         integers the host derives from the split direction and the CU size (geoLine below; vvhipBlendW0 in common.h) — no weight table and no weight block on the device.
// Items with a CIIP record (vvhip_pred_inter_batch_ciip) run in predListCiipKernel, the same body with a step behind the combine: the final clipped inter sample (one list,
//   the default average or BCW) is weighted with the PLANAR intra prediction of the block, ( wI * intra + ( 4 - wI ) * inter + 2 ) >> 2, wI = num_intra + 1, no clip
//   CIIP  weightCiipCore CommonLib/Buffer.cpp:60-81; IntraPrediction::predIntraAng with PLANAR_IDX CommonLib/IntraPrediction.cpp:353-383: xFilterReferenceSamples :994-1030
//         (luma only), xPredIntraPlanar_Core :79-135, IntraPredSampleFilter_Core :137-157 (PDPC, min( w, h ) >= 4).  The planar running sums are linear in x + 1 and
//         y + 1, so a lane evaluates its own samples from the block's reference line in block coordinates; the line is read straight from the caller's device array
//         (a lane needs its row's left sample, the two far corners and its own columns of the top row: a few cached loads, no LDS and no further wave barrier).
// Still the caller's: the BDOF conditions on POC distances and CU flags, the CU-level conditions of BCW, GEO and CIIP (with the neighbour availability and substitution of
// the intra reference line and getNumIntraCiip), explicit weighted prediction (slice-level weight tables), IBC, CIIP in a picture with LMCS active (the forward luma mapping
// before the weighting).  Affine CUs with PROF have an entry of their own that takes the
// control-point vectors (vvhip_pred_affine_batch, predaffine.hip: its own kernel and its own schedule cache; the 4x4 forms here are what it is checked against).
#include <algorithm>
#include <string.h>
#include "common.h"

namespace {

// VVC tap sets, phases 0..P/2; row P-p is row p reversed (InterpolationFilter.cpp:64-142)
__constant__ int8_t cPLuma8[9][8] = {
  { 0, 0, 0, 64, 0, 0, 0, 0 }, { 0, 1, -3, 63, 4, -2, 1, 0 }, { -1, 2, -5, 62, 8, -3, 1, 0 }, { -1, 3, -8, 60, 13, -4, 1, 0 }, { -1, 4, -10, 58, 17, -5, 1, 0 },
  { -1, 4, -11, 52, 26, -8, 3, -1 }, { -1, 3, -9, 47, 31, -10, 4, -1 }, { -1, 4, -11, 45, 34, -10, 4, -1 }, { -1, 4, -11, 40, 40, -11, 4, -1 } };
__constant__ int8_t cPLuma6[9][8] = {
  { 0, 0, 0, 64, 0, 0, 0, 0 }, { 0, 1, -3, 63, 4, -2, 1, 0 }, { 0, 1, -5, 62, 8, -3, 1, 0 }, { 0, 2, -8, 60, 13, -4, 1, 0 }, { 0, 3, -10, 58, 17, -5, 1, 0 },
  { 0, 3, -11, 52, 26, -8, 2, 0 }, { 0, 2, -9, 47, 31, -10, 3, 0 }, { 0, 3, -11, 45, 34, -10, 3, 0 }, { 0, 3, -11, 40, 40, -11, 3, 0 } };
__constant__ int8_t cPAltHpel[8] = { 0, 3, 9, 20, 20, 9, 3, 0 };
__constant__ int8_t cPChroma4[17][4] = {
  { 0, 64, 0, 0 }, { -1, 63, 2, 0 }, { -2, 62, 4, 0 }, { -2, 60, 7, -1 }, { -2, 58, 10, -2 }, { -3, 57, 12, -2 }, { -4, 56, 14, -2 }, { -4, 55, 15, -2 }, { -4, 54, 16, -2 },
  { -5, 53, 18, -2 }, { -6, 52, 20, -2 }, { -6, 49, 24, -3 }, { -6, 46, 28, -4 }, { -5, 44, 29, -4 }, { -4, 42, 30, -4 }, { -4, 39, 33, -4 }, { -4, 36, 36, -4 } };

// ---- the schedule the host uploads ----
struct __attribute__( ( aligned( 16 ) ) ) PredDev      // one prediction item with the plane table resolved
{
  const int16_t* ref[2];         // reference block at its integer position; null = list not used
  int32_t stride[2];
  int32_t dstOff, orgOff;
  int16_t frac[2][2];
  int16_t w, h;
  uint8_t alt, pad[3];           // extension forms: pad[0] = flags, pad[1 + l] = ( pad_dx[l] + 2 ) | ( pad_dy[l] + 2 ) << 4
};
struct PredSub  { int32_t item; int16_t x0, y0; };      // one tile of an item
struct PredBlendDev { int32_t a, b, c; int16_t lo, hi; };      // w0( x, y ) of a BCW / GEO item (vvhipBlendW0); parallel to the items, read by predListBlendKernel only
struct PredCiipDev { int32_t refOff; int8_t w0; uint8_t wI, filt, pdpc; };      // a CIIP item: its line in the intra reference array, hypothesis 0's weight of the inter part (4: default average), num_intra + 1, luma smoothing, PDPC; read by predListCiipKernel only
struct PredUnit { int32_t firstSub; int16_t nSub, tw, th; uint8_t kind, log2Lanes, log2SegsRow, pad[3]; };      // what one wave does (pad[0]: the extension flags of its class)
static_assert( sizeof( PredDev ) == 48 && sizeof( PredSub ) == 8 && sizeof( PredUnit ) == 16 && sizeof( PredBlendDev ) == 16 && sizeof( PredCiipDev ) == 8, "schedule records" );

// kernel forms: samples per lane (a "segment": SEG horizontally adjacent samples) x taps per pass
enum { KIND_L8 = 0, KIND_L4 = 1, KIND_C8 = 2, KIND_C4 = 3, KIND_C2 = 4 };
enum { MODE_UNI = 0, MODE_BI = 1, MODE_RAW = 2 };      // final samples of one list / average of two / the 14-bit block of one list (rnd_res = 0)

struct TileShape { int tw, th, log2SegsRow, log2Lanes, kind; };
inline int segOfKind( int kind ) { return kind == KIND_L8 || kind == KIND_C8 ? 8 : kind == KIND_C2 ? 2 : 4; }
inline int tapsOfKind( int kind ) { return kind <= KIND_L4 ? 8 : 4; }

// a block is cut into tiles of at most 64 segments: 32 x 16, 16 x 32, 8 x 64, 4 x 64, 2 x 64 — or the whole block when it is smaller
TileShape tileShape( int w, int h, bool chroma )
{
  TileShape s;
  const int seg = w >= 8 ? 8 : w;
  s.kind = chroma ? ( seg == 8 ? KIND_C8 : seg == 4 ? KIND_C4 : KIND_C2 ) : ( seg == 8 ? KIND_L8 : KIND_L4 );
  s.tw = std::min( w, 32 );
  s.log2SegsRow = ilog2i( s.tw / seg );
  s.th = std::min( h, 64 >> s.log2SegsRow );
  s.log2Lanes = s.log2SegsRow + ilog2i( s.th );
  return s;
}
// LDS samples of one tile: the window (row pitch tw + taps + 2) and the first-pass block, th + taps - 1 rows each, both 16-byte aligned
__host__ __device__ inline int winElems( int tw, int th, int nt ) { return ( ( th + nt - 1 ) * ( tw + nt + 2 ) + 7 ) & ~7; }
__host__ __device__ inline int subElems( int tw, int th, int nt ) { return winElems( tw, th, nt ) + ( ( ( th + nt - 1 ) * tw + 7 ) & ~7 ); }

// what one lane needs to know about the tile its group works on
struct Lane
{
  bool on;
  const int16_t* ref[2];
  int stride[2], fx[2], fy[2];
  int w, h, alt;                 // the whole block (4x4 luma has its own tap set); alternative half-sample filter
  int x0, y0;                    // tile origin inside the block
  int lis;                       // lane inside the group
  int mode;
  int16_t* win; int16_t* tmp;
  int16_t* dst; int dstPitch;    // block origin in the prediction buffer
  const int16_t* org; int orgPitch;
  int16_t* res; int resPitch;    // null: no residual
  // extension forms only (predBody<.., true>): BDOF unit, DMVR clamp window per list in block coordinates (inclusive), BDOF arrays
  bool bdof, clamp;
  int cx0[2], cx1[2], cy0[2], cy1[2];
  int16_t* ext;
  // blend form only (predBody<.., FORM_BLEND>): the weight line of the item
  int ba, bb, bc, blo, bhi;
  // CIIP form only (predBody<.., FORM_CIIP>): top[0 .. w + 2] then left[0 .. h + 2] of the block, hypothesis 0's weight, the intra weight, smoothing and PDPC on / off
  const int16_t* line;
  int cw0, cwI, cfilt, cpdpc;
};

#define PRED_WAVE_SYNC() { __builtin_amdgcn_fence( __ATOMIC_ACQ_REL, "wavefront" ); __builtin_amdgcn_wave_barrier(); }

// taps of one direction as c[k] * sample[pos - lo + k]; a zero fraction is the one-tap set { 64 } at lo = 0
template<int NT>
__device__ __forceinline__ void loadTaps( int ( &c )[NT], int& lo, int frac, bool is4x4, bool both, int alt )
{
#pragma unroll
  for( int k = 0; k < NT; k++ ) c[k] = 0;
  lo = 0;
  if( frac == 0 ) { c[0] = 64; return; }
  lo = NT / 2 - 1;
  if( NT == 8 )
  {
    // 4x4 blocks: filter4x4 swaps in the alternative row for BOTH directions whatever the phase (InterpolationFilter.cpp:692-693); the 1-D dispatch only at phase 8 (:570-580)
    const bool useAlt = is4x4 ? ( alt && ( both || frac == 8 ) ) : ( alt && frac == 8 );
    const int p = frac <= 8 ? frac : 16 - frac;
#pragma unroll
    for( int k = 0; k < NT; k++ )
    {
      const int kk = frac <= 8 ? k : 7 - k;
      c[k] = useAlt ? cPAltHpel[k & 7] : is4x4 ? cPLuma6[p][kk & 7] : cPLuma8[p][kk & 7];
    }
  }
  else
  {
#pragma unroll
    for( int k = 0; k < NT; k++ ) c[k] = frac <= 16 ? cPChroma4[frac][k & 3] : cPChroma4[32 - frac][3 - ( k & 3 )];
  }
}

template<int SEG> struct __attribute__( ( aligned( SEG * 2 ) ) ) SegRow { int16_t v[SEG]; };

// LDS samples a BDOF unit keeps beside its window: list 0's 14-bit block with its one-sample ring, then ( gx0 + gx1 ) >> 1, ( gy0 + gy1 ) >> 1, ( s1 >> 4 ) - ( s0 >> 4 )
__host__ __device__ inline int bdofRingElems( int tw, int th ) { return ( ( tw + 2 ) * ( th + 2 ) + 7 ) & ~7; }
__host__ __device__ inline int bdofElems( int tw, int th ) { return bdofRingElems( tw, th ) + 3 * tw * th; }

__device__ __forceinline__ int clampi( int v, int lo, int hi ) { return v < lo ? lo : ( v > hi ? hi : v ); }

// FORM_PLAIN: the forms of vvhip_pred_inter_batch.  FORM_EX adds, per unit of the schedule, the DMVR clamp in the window staging and the BDOF form of the average.
// FORM_BLEND replaces the average by the weighted one of BCW / GEO (both hypotheses present: the host checks it).
// FORM_CIIP takes uni- and bi-predicted items (the average with hypothesis 0's weight cw0: 4 is the default average) and weights the final sample with planar intra prediction.
enum { FORM_PLAIN = 0, FORM_EX = 1, FORM_BLEND = 2, FORM_CIIP = 3 };

// sample i ( >= 1 ) of one row of the intra reference line as planar and PDPC read it: smoothed for luma (xFilterReferenceSamples), as it is for chroma
__device__ __forceinline__ int ciipRef( const int16_t* r, int i, int filt ) { const int c = r[i]; return filt ? ( ( int ) r[i - 1] + 2 * c + ( int ) r[i + 1] + 2 ) >> 2 : c; }
template<int SEG, int NT, int FORM = FORM_PLAIN>
__device__ __forceinline__ void predBody( const Lane& L, int tw, int th, int log2SegsRow, int lanes, int bitDepth )
{
  constexpr bool EX = FORM == FORM_EX;
  constexpr int ND = ( SEG + NT ) / 2 + 1;              // dwords that hold a segment's SEG + NT - 1 window samples at either alignment
  const int hr = 14 - bitDepth > 2 ? 14 - bitDepth : 2, maxv = ( 1 << bitDepth ) - 1;
  const int pitch = tw + NT + 2, segsRow = 1 << log2SegsRow;
  const int y = L.lis >> log2SegsRow, xs = ( L.lis & ( segsRow - 1 ) ) * SEG;      // this lane's output row and first column inside the tile
  const bool is4x4 = NT == 8 && L.w == 4 && L.h == 4;
  int first[SEG], acc[SEG];
#pragma unroll
  for( int j = 0; j < SEG; j++ ) first[j] = acc[j] = 0;

#pragma unroll
  for( int l = 0; l < 2; l++ )
  {
    const bool use = L.on && L.ref[l] != nullptr;
    const bool both = L.fx[l] != 0 && L.fy[l] != 0;
    int ch[NT], cv[NT], loX = 0, loY = 0;
    loadTaps<NT>( ch, loX, L.fx[l], is4x4, both, L.alt );
    loadTaps<NT>( cv, loY, L.fy[l], is4x4, both, L.alt );
    const int rows = th + ( L.fy[l] ? NT - 1 : 0 ), cols = tw + ( L.fx[l] ? NT - 1 : 0 );
    int sh = 0;
    // ---- 1. the window: rows y0 - loY .. , columns x0 - loX - sh .. as aligned dwords (sh = 1 when the first column sits in the upper half of its dword)
    if( use )
    {
      const int16_t* g = L.ref[l] + ( ptrdiff_t ) ( L.y0 - loY ) * L.stride[l] + ( L.x0 - loX );
      const uintptr_t a = reinterpret_cast<uintptr_t>( g );
      sh = ( int ) ( ( a >> 1 ) & 1 );
      const uint32_t* g32 = reinterpret_cast<const uint32_t*>( a & ~( uintptr_t ) 3 );
      const int dwRow = ( cols + sh + 1 ) >> 1, strideDw = L.stride[l] >> 1;        // (the stride is even: every row has the same alignment)
      uint32_t* w32 = reinterpret_cast<uint32_t*>( L.win );
      const int l2 = 32 - __builtin_clz( ( unsigned ) ( dwRow - 1 ) | 1u );      // rows are dealt in strides of the next power of two: no division (a quarter of the slots idle at worst)
      if( EX && L.clamp )
      {
        // DMVR's final motion compensation reads a replication-padded copy of the window prefetched around the START vector (xCopyAndPad, xFinalPaddedMCForDMVR):
        // the same dword slots, every sample's coordinates clamped to that window
        for( int i = L.lis; i < ( rows << l2 ); i += lanes )
        {
          const int r = i >> l2, d = i & ( ( 1 << l2 ) - 1 );
          if( d < dwRow )
          {
            const int yy = clampi( L.y0 - loY + r, L.cy0[l], L.cy1[l] ), xx = L.x0 - loX - sh + 2 * d;
            const int16_t* row = L.ref[l] + ( ptrdiff_t ) yy * L.stride[l];
            const uint32_t lo16 = ( uint16_t ) row[clampi( xx, L.cx0[l], L.cx1[l] )], hi16 = ( uint16_t ) row[clampi( xx + 1, L.cx0[l], L.cx1[l] )];
            w32[r * ( pitch >> 1 ) + d] = lo16 | ( hi16 << 16 );
          }
        }
      }
      else
      for( int i = L.lis; i < ( rows << l2 ); i += lanes )
      {
        const int r = i >> l2, d = i & ( ( 1 << l2 ) - 1 );
        if( d < dwRow ) w32[r * ( pitch >> 1 ) + d] = g32[( ptrdiff_t ) r * strideDw + d];
      }
    }
    PRED_WAVE_SYNC();
    // ---- 2. horizontal pass, isFirst && !isLast: ( sum - ( 8192 << s1 ) ) >> s1 with s1 = 6 - headroom
    if( use )
    {
      const int s1 = 6 - hr, off1 = -( 8192 << s1 );
      for( int i = L.lis; i < ( rows << log2SegsRow ); i += lanes )
      {
        const int r = i >> log2SegsRow, x = ( i & ( segsRow - 1 ) ) * SEG;
        const uint32_t* p = reinterpret_cast<const uint32_t*>( L.win + r * pitch + x );
        uint32_t d[ND];
#pragma unroll
        for( int k = 0; k < ND; k++ ) d[k] = p[k];
        int win[SEG + NT];
#pragma unroll
        for( int k = 0; k < ND - 1; k++ )
        {
          const uint32_t s = __builtin_amdgcn_alignbit( d[k + 1], d[k], ( uint32_t ) ( sh << 4 ) );
          win[2 * k] = ( int ) ( int16_t ) ( s & 0xffff ); win[2 * k + 1] = ( int ) ( int16_t ) ( s >> 16 );
        }
        SegRow<SEG> o;
#pragma unroll
        for( int j = 0; j < SEG; j++ )
        {
          int s = 0;
#pragma unroll
          for( int k = 0; k < NT; k++ ) s = __mul24( win[j + k], ch[k] ) + s;       // |sample| < 2^15, |tap| < 2^7: the 24-bit multiply is exact
          o.v[j] = ( int16_t ) ( ( s + off1 ) >> s1 );
        }
        *reinterpret_cast<SegRow<SEG>*>( L.tmp + r * tw + x ) = o;
      }
    }
    PRED_WAVE_SYNC();
    // ---- 3. vertical pass, !isFirst: isLast ( + clip ) for a uni-predicted block, the 14-bit block otherwise
    if( use )
    {
#pragma unroll
      for( int j = 0; j < SEG; j++ ) acc[j] = 0;
#pragma unroll
      for( int k = 0; k < NT; k++ )
      {
        const SegRow<SEG> row = *reinterpret_cast<const SegRow<SEG>*>( L.tmp + ( y + k ) * tw + xs );
#pragma unroll
        for( int j = 0; j < SEG; j++ ) acc[j] = __mul24( ( int ) row.v[j], cv[k] ) + acc[j];
      }
      if( L.mode == MODE_UNI )
      {
        const int s2 = 6 + hr, off2 = ( 1 << ( s2 - 1 ) ) + ( 8192 << 6 );
#pragma unroll
        for( int j = 0; j < SEG; j++ ) { const int v = ( int16_t ) ( ( acc[j] + off2 ) >> s2 ); acc[j] = v < 0 ? 0 : ( v > maxv ? maxv : v ); }
      }
      else
      {
#pragma unroll
        for( int j = 0; j < SEG; j++ ) acc[j] = ( int16_t ) ( acc[j] >> 6 );
      }
    }
    PRED_WAVE_SYNC();
    if( l == 0 )
    {
#pragma unroll
      for( int j = 0; j < SEG; j++ ) first[j] = acc[j];
    }
    if( EX && SEG == 8 && NT == 8 )
    {
      // ---- BDOF: the list's 14-bit block inside a one-sample ring of integer samples at the nearest-integer position, ( ref << headroom ) - IF_INTERNAL_OFFS
      //      (xPredInterBlk :868-901).  List 0 keeps its frame beside the window; list 1's frame reuses the window, which nobody reads any more.
      if( L.bdof && use )
      {
        const int pp = tw + 2;
        int16_t* P = l == 0 ? L.ext : L.win;
#pragma unroll
        for( int j = 0; j < SEG; j++ ) P[( y + 1 ) * pp + xs + 1 + j] = ( int16_t ) acc[j];
        const int xo = L.fx[l] < 8 ? 1 : 0, yo = L.fy[l] < 8 ? 1 : 0, nRing = 2 * pp + 2 * th;
        for( int i = L.lis; i < nRing; i += lanes )
        {
          int fx, fy;
          if( i < 2 * pp ) { fy = i < pp ? 0 : th + 1; fx = i < pp ? i : i - pp; }
          else { const int k = i - 2 * pp; fy = 1 + ( k >> 1 ); fx = ( k & 1 ) ? tw + 1 : 0; }
          int cx = L.x0 + fx - xo, cy = L.y0 + fy - yo;
          if( L.clamp ) { cx = clampi( cx, L.cx0[l], L.cx1[l] ); cy = clampi( cy, L.cy0[l], L.cy1[l] ); }
          P[fy * pp + fx] = ( int16_t ) ( ( ( int ) L.ref[l][( ptrdiff_t ) cy * L.stride[l] + cx] << hr ) - 8192 );
        }
      }
      if( L.bdof ) PRED_WAVE_SYNC();
    }
  }
  if( EX && SEG == 8 && NT == 8 )
  {
    if( L.bdof )      // (uniform over the wave: a unit of the schedule holds one form)
    {
      // ---- gradients of both lists on the lane's own samples, the ring as neighbours (gradFilterCore :114-131)
      const int pp = tw + 2;
      int dgx[SEG], dgy[SEG];
      SegRow<SEG> tgx, tgy, tdi;
      {
        int gx[2][SEG], gy[2][SEG];
#pragma unroll
        for( int l = 0; l < 2; l++ )
        {
          const int16_t* P = ( l == 0 ? L.ext : L.win ) + ( y + 1 ) * pp + xs + 1;
          int c[SEG + 2];
#pragma unroll
          for( int j = 0; j < SEG + 2; j++ ) c[j] = ( int ) P[j - 1] >> 6;
#pragma unroll
          for( int j = 0; j < SEG; j++ ) { gx[l][j] = c[j + 2] - c[j]; gy[l][j] = ( ( int ) P[j + pp] >> 6 ) - ( ( int ) P[j - pp] >> 6 ); }
        }
#pragma unroll
        for( int j = 0; j < SEG; j++ )
        {
          dgx[j] = gx[0][j] - gx[1][j]; dgy[j] = gy[0][j] - gy[1][j];
          tgx.v[j] = ( int16_t ) ( ( gx[0][j] + gx[1][j] ) >> 1 ); tgy.v[j] = ( int16_t ) ( ( gy[0][j] + gy[1][j] ) >> 1 );
          tdi.v[j] = ( int16_t ) ( ( acc[j] >> 4 ) - ( first[j] >> 4 ) );
        }
      }
      // the window sums read the replication-padded arrays (gradFilterCore :133-154, xApplyBDOF :939-949): the interior at clamped coordinates
      int16_t* tGX = L.ext + bdofRingElems( tw, th );
      int16_t* tGY = tGX + tw * th;
      int16_t* tDI = tGY + tw * th;
      *reinterpret_cast<SegRow<SEG>*>( tGX + y * tw + xs ) = tgx;
      *reinterpret_cast<SegRow<SEG>*>( tGY + y * tw + xs ) = tgy;
      *reinterpret_cast<SegRow<SEG>*>( tDI + y * tw + xs ) = tdi;
      PRED_WAVE_SYNC();
      // ---- a lane pair per 4x4 unit, three rows of its 6x6 window each (calcBDOFSumsCore :157-186); the group has exactly two lanes per unit
      const int u = L.lis >> 1, half = L.lis & 1, l2u = log2SegsRow + 1;
      const int uy = u >> l2u, ux = u & ( ( 1 << l2u ) - 1 );
      int sAbsGX = 0, sAbsGY = 0, sDIX = 0, sDIY = 0, sSign = 0;
#pragma unroll
      for( int r = 0; r < 3; r++ )
      {
        const int yy = clampi( 4 * uy - 1 + 3 * half + r, 0, th - 1 ) * tw;
#pragma unroll
        for( int cidx = 0; cidx < 6; cidx++ )
        {
          const int o = yy + clampi( 4 * ux - 1 + cidx, 0, tw - 1 );
          const int g = tGX[o], v = tGY[o], d = tDI[o];
          sAbsGX += g < 0 ? -g : g; sAbsGY += v < 0 ? -v : v;
          sDIX += g < 0 ? -d : ( g == 0 ? 0 : d );
          sDIY += v < 0 ? -d : ( v == 0 ? 0 : d );
          sSign += v < 0 ? -g : ( v == 0 ? 0 : g );
        }
      }
      sAbsGX += __shfl_xor( sAbsGX, 1 ); sAbsGY += __shfl_xor( sAbsGY, 1 ); sDIX += __shfl_xor( sDIX, 1 ); sDIY += __shfl_xor( sDIY, 1 ); sSign += __shfl_xor( sSign, 1 );
      // the two offsets (xFpBiDirOptFlowCore :642-647): floorLog2 = 31 - clz
      int tmpx = sAbsGX ? clampi( ( 4 * sDIX ) >> ( 31 - __builtin_clz( ( unsigned ) sAbsGX ) ), -15, 15 ) : 0;
      int tmpy = sAbsGY ? clampi( ( 4 * sDIY - ( ( sSign * tmpx ) >> 1 ) ) >> ( 31 - __builtin_clz( ( unsigned ) sAbsGY ) ), -15, 15 ) : 0;
      const int packed = ( tmpx & 0xffff ) | ( tmpy << 16 );
      const int base = ( int ) ( threadIdx.x & 63 ) - L.lis, ua = ( ( y >> 2 ) << l2u ) + ( xs >> 2 );
      const int pa = __shfl( packed, base + 2 * ua ), pb = __shfl( packed, base + 2 * ua + 2 );
      // ---- addBDOFAvgCore :63-86: ClipPel( (int16_t) ( ( s0 + s1 + b + offset ) >> shiftNum ) ), shiftNum = 15 - bitDepth
      const int sn = 15 - bitDepth, off = ( 1 << ( sn - 1 ) ) + 2 * 8192;
#pragma unroll
      for( int j = 0; j < SEG; j++ )
      {
        const int pk = j < 4 ? pa : pb, tx = ( int ) ( int16_t ) ( pk & 0xffff ), ty = pk >> 16;
        const int b = tx * dgx[j] + ty * dgy[j];
        const int v = ( int16_t ) ( ( first[j] + acc[j] + b + off ) >> sn );
        acc[j] = v < 0 ? 0 : ( v > maxv ? maxv : v );
      }
    }
  }
  if( !L.on ) return;
  if( EX && SEG == 8 && NT == 8 && L.bdof ) {}
  else if( FORM == FORM_BLEND )      // each lane's SEG adjacent samples: w0 constant (BCW) or stepping along the row (GEO), 32-bit (|10 * s| < 2^19)
  {
    const int sn = hr + 3, off = ( 1 << ( sn - 1 ) ) + ( 8192 << 3 );
#pragma unroll
    for( int j = 0; j < SEG; j++ )
    {
      const int w0 = vvhipBlendW0( L.ba, L.bb, L.bc, L.blo, L.bhi, L.x0 + xs + j, L.y0 + y );
      const int v = ( w0 * first[j] + ( 8 - w0 ) * acc[j] + off ) >> sn;
      acc[j] = v < 0 ? 0 : ( v > maxv ? maxv : v );
    }
  }
  else if( FORM == FORM_CIIP && L.mode == MODE_BI )      // the default average as w0 = 4 ( 4 ( a + b + offset ) >> ( shiftNum + 2 ) is the same number ), or BCW's
  {
    const int sn = hr + 3, off = ( 1 << ( sn - 1 ) ) + ( 8192 << 3 );
#pragma unroll
    for( int j = 0; j < SEG; j++ ) { const int v = ( L.cw0 * first[j] + ( 8 - L.cw0 ) * acc[j] + off ) >> sn; acc[j] = v < 0 ? 0 : ( v > maxv ? maxv : v ); }
  }
  else if( L.mode == MODE_BI )      // addAvg: ClipPel( ( a + b + offset ) >> shiftNum ), shiftNum = headroom + 1, offset = ( 1 << headroom ) + 2 * IF_INTERNAL_OFFS (Buffer.cpp:129-141, :549-575)
  {
    const int sn = hr + 1, off = ( 1 << hr ) + 2 * 8192;
#pragma unroll
    for( int j = 0; j < SEG; j++ ) { const int v = ( first[j] + acc[j] + off ) >> sn; acc[j] = v < 0 ? 0 : ( v > maxv ? maxv : v ); }
  }
  else if( L.ref[1] == nullptr )
  {
#pragma unroll
    for( int j = 0; j < SEG; j++ ) acc[j] = first[j];
  }
  const int row = L.y0 + y, col = L.x0 + xs;
  if( FORM == FORM_CIIP )
  {
    // planar at block coordinates ( col + j, row ): horPred = ( left << log2W ) + ( x + 1 ) * ( topRight - left ), vertPred = ( top << log2H ) + ( y + 1 ) * ( bottomLeft - top )
    // (xPredIntraPlanar_Core's running sums, closed), then PDPC on the same line, then the weighting with the clipped inter sample.  12-bit samples: every term < 2^25.
    const int16_t* top = L.line; const int16_t* left = L.line + L.w + 3;
    const int l2w = 31 - __builtin_clz( ( unsigned ) L.w ), l2h = 31 - __builtin_clz( ( unsigned ) L.h ), scale = ( l2w + l2h - 2 ) >> 2;
    const int lf = ciipRef( left, row + 1, L.cfilt ), tr = ciipRef( top, L.w + 1, L.cfilt ), bl = ciipRef( left, L.h + 1, L.cfilt );
    const int wT = L.cpdpc ? 32 >> min( 31, ( 2 * row ) >> scale ) : 0;
    int u[SEG + 2];
#pragma unroll
    for( int j = 0; j < SEG + 2; j++ ) u[j] = top[col + j];      // top[col .. col + SEG + 1], col + SEG <= w: inside top[0 .. w + 2]
#pragma unroll
    for( int j = 0; j < SEG; j++ )
    {
      const int t = L.cfilt ? ( u[j] + 2 * u[j + 1] + u[j + 2] + 2 ) >> 2 : u[j + 1];
      const int hor = ( lf << l2w ) + ( col + j + 1 ) * ( tr - lf ), ver = ( t << l2h ) + ( row + 1 ) * ( bl - t );
      int p = ( ( hor << l2h ) + ( ver << l2w ) + ( 1 << ( l2w + l2h ) ) ) >> ( 1 + l2w + l2h );
      const int wL = L.cpdpc ? 32 >> min( 31, ( 2 * ( col + j ) ) >> scale ) : 0;
      p += ( wL * ( lf - p ) + wT * ( t - p ) + 32 ) >> 6;
      acc[j] = ( L.cwI * p + ( 4 - L.cwI ) * acc[j] + 2 ) >> 2;
    }
  }
  SegRow<SEG> o;
#pragma unroll
  for( int j = 0; j < SEG; j++ ) o.v[j] = ( int16_t ) acc[j];
  int16_t* dp = L.dst + ( ptrdiff_t ) row * L.dstPitch + col;
  if( ( reinterpret_cast<uintptr_t>( dp ) & ( SEG * 2 - 1 ) ) == 0 ) *reinterpret_cast<SegRow<SEG>*>( dp ) = o;
  else
  {
#pragma unroll
    for( int j = 0; j < SEG; j++ ) dp[j] = o.v[j];
  }
  if( L.res )
  {
    const int16_t* op = L.org + ( ptrdiff_t ) row * L.orgPitch + col;
    SegRow<SEG> g;
    if( ( reinterpret_cast<uintptr_t>( op ) & ( SEG * 2 - 1 ) ) == 0 ) g = *reinterpret_cast<const SegRow<SEG>*>( op );
    else
    {
#pragma unroll
      for( int j = 0; j < SEG; j++ ) g.v[j] = op[j];
    }
#pragma unroll
    for( int j = 0; j < SEG; j++ ) g.v[j] = ( int16_t ) ( g.v[j] - o.v[j] );
    int16_t* rp = L.res + ( ptrdiff_t ) row * L.resPitch + col;
    if( ( reinterpret_cast<uintptr_t>( rp ) & ( SEG * 2 - 1 ) ) == 0 ) *reinterpret_cast<SegRow<SEG>*>( rp ) = g;
    else
    {
#pragma unroll
      for( int j = 0; j < SEG; j++ ) rp[j] = g.v[j];
    }
  }
}

__device__ __forceinline__ void predDispatch( int kind, const Lane& L, int tw, int th, int log2SegsRow, int lanes, int bitDepth )
{
  switch( kind )      // wave-uniform
  {
  case KIND_L8: predBody<8, 8>( L, tw, th, log2SegsRow, lanes, bitDepth ); break;
  case KIND_L4: predBody<4, 8>( L, tw, th, log2SegsRow, lanes, bitDepth ); break;
  case KIND_C8: predBody<8, 4>( L, tw, th, log2SegsRow, lanes, bitDepth ); break;
  case KIND_C4: predBody<4, 4>( L, tw, th, log2SegsRow, lanes, bitDepth ); break;
  default:      predBody<2, 4>( L, tw, th, log2SegsRow, lanes, bitDepth ); break;
  }
}

__device__ __forceinline__ void predDispatchEx( int kind, const Lane& L, int tw, int th, int log2SegsRow, int lanes, int bitDepth )
{
  switch( kind )      // wave-uniform
  {
  case KIND_L8: predBody<8, 8, FORM_EX>( L, tw, th, log2SegsRow, lanes, bitDepth ); break;
  case KIND_L4: predBody<4, 8, FORM_EX>( L, tw, th, log2SegsRow, lanes, bitDepth ); break;
  case KIND_C8: predBody<8, 4, FORM_EX>( L, tw, th, log2SegsRow, lanes, bitDepth ); break;
  case KIND_C4: predBody<4, 4, FORM_EX>( L, tw, th, log2SegsRow, lanes, bitDepth ); break;
  default:      predBody<2, 4, FORM_EX>( L, tw, th, log2SegsRow, lanes, bitDepth ); break;
  }
}

__device__ __forceinline__ void predDispatchBlend( int kind, const Lane& L, int tw, int th, int log2SegsRow, int lanes, int bitDepth )
{
  switch( kind )      // wave-uniform
  {
  case KIND_L8: predBody<8, 8, FORM_BLEND>( L, tw, th, log2SegsRow, lanes, bitDepth ); break;
  case KIND_L4: predBody<4, 8, FORM_BLEND>( L, tw, th, log2SegsRow, lanes, bitDepth ); break;
  case KIND_C8: predBody<8, 4, FORM_BLEND>( L, tw, th, log2SegsRow, lanes, bitDepth ); break;
  case KIND_C4: predBody<4, 4, FORM_BLEND>( L, tw, th, log2SegsRow, lanes, bitDepth ); break;
  default:      predBody<2, 4, FORM_BLEND>( L, tw, th, log2SegsRow, lanes, bitDepth ); break;
  }
}

__device__ __forceinline__ void predDispatchCiip( int kind, const Lane& L, int tw, int th, int log2SegsRow, int lanes, int bitDepth )
{
  switch( kind )      // wave-uniform (a CIIP block is at least 4 wide: no 2-sample form)
  {
  case KIND_L8: predBody<8, 8, FORM_CIIP>( L, tw, th, log2SegsRow, lanes, bitDepth ); break;
  case KIND_L4: predBody<4, 8, FORM_CIIP>( L, tw, th, log2SegsRow, lanes, bitDepth ); break;
  case KIND_C8: predBody<8, 4, FORM_CIIP>( L, tw, th, log2SegsRow, lanes, bitDepth ); break;
  default:      predBody<4, 4, FORM_CIIP>( L, tw, th, log2SegsRow, lanes, bitDepth ); break;
  }
}

struct PredArgs
{
  const PredDev* items; const PredSub* subs; const PredUnit* units;
  int nUnits, bitDepth, ldsPerWave;
  int16_t* pred; int predStride;
  const int16_t* org; int orgStride;
  int16_t* resi;
};

// a list of mixed sizes: wave -> unit of the host's schedule (size classes, picture bands per XCD)
__global__ void __launch_bounds__( 256 )
predListKernel( PredArgs a )
{
  extern __shared__ __attribute__( ( aligned( 16 ) ) ) int16_t sPred[];
  const int wave = __builtin_amdgcn_readfirstlane( ( int ) ( threadIdx.x >> 6 ) ), lane = threadIdx.x & 63;
  const int ui = ( int ) blockIdx.x * 4 + wave;
  if( ui >= a.nUnits ) return;
  const PredUnit u = a.units[ui];
  if( u.nSub == 0 ) return;
  const int nt = u.kind <= KIND_L4 ? 8 : 4, lanes = 1 << u.log2Lanes, si = lane >> u.log2Lanes;
  Lane L;
  L.on = si < u.nSub;
  L.lis = lane & ( lanes - 1 );
  L.win = sPred + ( size_t ) wave * a.ldsPerWave + ( size_t ) si * subElems( u.tw, u.th, nt );
  L.tmp = L.win + winElems( u.tw, u.th, nt );
  const PredSub s = a.subs[u.firstSub + ( L.on ? si : 0 )];
  const PredDev it = a.items[s.item];
  L.ref[0] = it.ref[0]; L.ref[1] = it.ref[1]; L.stride[0] = it.stride[0]; L.stride[1] = it.stride[1];
  L.fx[0] = it.frac[0][0]; L.fy[0] = it.frac[0][1]; L.fx[1] = it.frac[1][0]; L.fy[1] = it.frac[1][1];
  L.w = it.w; L.h = it.h; L.alt = it.alt; L.x0 = s.x0; L.y0 = s.y0;
  L.mode = it.ref[0] && it.ref[1] ? MODE_BI : MODE_UNI;
  if( !it.ref[0] ) { L.ref[0] = it.ref[1]; L.stride[0] = it.stride[1]; L.fx[0] = L.fx[1]; L.fy[0] = L.fy[1]; L.ref[1] = nullptr; }      // a list-1-only block runs as the first pass
  L.dstPitch = a.predStride ? a.predStride : it.w;
  L.dst = a.pred + it.dstOff;
  L.org = a.org ? a.org + it.orgOff : nullptr; L.orgPitch = a.orgStride;
  L.res = a.resi ? a.resi + it.dstOff : nullptr; L.resPitch = L.dstPitch;
  predDispatch( u.kind, L, u.tw, u.th, u.log2SegsRow, lanes, a.bitDepth );
}

// the units of items with an extension (vvhip_pred_inter_batch_ex): BDOF units (16x16 / 16x8 / 8x16, two or four per wave) and blocks read through DMVR's clamp window.
// A kernel of its own: the forms of predListKernel keep their registers.
__global__ void __launch_bounds__( 256 )
predListExKernel( PredArgs a )
{
  extern __shared__ __attribute__( ( aligned( 16 ) ) ) int16_t sPred[];
  const int wave = __builtin_amdgcn_readfirstlane( ( int ) ( threadIdx.x >> 6 ) ), lane = threadIdx.x & 63;
  const int ui = ( int ) blockIdx.x * 4 + wave;
  if( ui >= a.nUnits ) return;
  const PredUnit u = a.units[ui];
  if( u.nSub == 0 ) return;
  const int nt = u.kind <= KIND_L4 ? 8 : 4, lanes = 1 << u.log2Lanes, si = lane >> u.log2Lanes;
  Lane L;
  L.bdof = ( u.pad[0] & VVHIP_PRED_EXT_BDOF ) != 0; L.clamp = ( u.pad[0] & VVHIP_PRED_EXT_DMVR_PAD ) != 0;
  L.on = si < u.nSub;
  L.lis = lane & ( lanes - 1 );
  L.win = sPred + ( size_t ) wave * a.ldsPerWave + ( size_t ) si * ( subElems( u.tw, u.th, nt ) + ( L.bdof ? bdofElems( u.tw, u.th ) : 0 ) );
  L.tmp = L.win + winElems( u.tw, u.th, nt );
  L.ext = L.win + subElems( u.tw, u.th, nt );
  const PredSub s = a.subs[u.firstSub + ( L.on ? si : 0 )];
  const PredDev it = a.items[s.item];
  L.ref[0] = it.ref[0]; L.ref[1] = it.ref[1]; L.stride[0] = it.stride[0]; L.stride[1] = it.stride[1];
  L.fx[0] = it.frac[0][0]; L.fy[0] = it.frac[0][1]; L.fx[1] = it.frac[1][0]; L.fy[1] = it.frac[1][1];
  L.w = it.w; L.h = it.h; L.alt = it.alt; L.x0 = s.x0; L.y0 = s.y0;
  L.mode = it.ref[0] && it.ref[1] ? MODE_BI : MODE_UNI;
  const int reach = nt / 2 - 1;      // the prefetched window: ( w + taps - 1 ) x ( h + taps - 1 ) samples from start - ( taps / 2 - 1 )
#pragma unroll
  for( int l = 0; l < 2; l++ )
  {
    const int pdx = ( it.pad[1 + l] & 15 ) - 2, pdy = ( it.pad[1 + l] >> 4 ) - 2;
    L.cx0[l] = -reach - pdx; L.cx1[l] = it.w + reach - pdx; L.cy0[l] = -reach - pdy; L.cy1[l] = it.h + reach - pdy;
  }
  if( !it.ref[0] )      // a list-1-only block runs as the first pass
  {
    L.ref[0] = it.ref[1]; L.stride[0] = it.stride[1]; L.fx[0] = L.fx[1]; L.fy[0] = L.fy[1]; L.ref[1] = nullptr;
    L.cx0[0] = L.cx0[1]; L.cx1[0] = L.cx1[1]; L.cy0[0] = L.cy0[1]; L.cy1[0] = L.cy1[1];
  }
  L.dstPitch = a.predStride ? a.predStride : it.w;
  L.dst = a.pred + it.dstOff;
  L.org = a.org ? a.org + it.orgOff : nullptr; L.orgPitch = a.orgStride;
  L.res = a.resi ? a.resi + it.dstOff : nullptr; L.resPitch = L.dstPitch;
  predDispatchEx( u.kind, L, u.tw, u.th, u.log2SegsRow, lanes, a.bitDepth );
}

// the units of BCW / GEO items (vvhip_pred_inter_batch_blend): both hypotheses to the 14-bit block, then the weighted average with the item's weight line.
// A kernel of its own, as the extension forms: the other forms keep their registers.
__global__ void __launch_bounds__( 256 )
predListBlendKernel( PredArgs a, const PredBlendDev* __restrict__ blend )
{
  extern __shared__ __attribute__( ( aligned( 16 ) ) ) int16_t sPred[];
  const int wave = __builtin_amdgcn_readfirstlane( ( int ) ( threadIdx.x >> 6 ) ), lane = threadIdx.x & 63;
  const int ui = ( int ) blockIdx.x * 4 + wave;
  if( ui >= a.nUnits ) return;
  const PredUnit u = a.units[ui];
  if( u.nSub == 0 ) return;
  const int nt = u.kind <= KIND_L4 ? 8 : 4, lanes = 1 << u.log2Lanes, si = lane >> u.log2Lanes;
  Lane L;
  L.on = si < u.nSub;
  L.lis = lane & ( lanes - 1 );
  L.win = sPred + ( size_t ) wave * a.ldsPerWave + ( size_t ) si * subElems( u.tw, u.th, nt );
  L.tmp = L.win + winElems( u.tw, u.th, nt );
  const PredSub s = a.subs[u.firstSub + ( L.on ? si : 0 )];
  const PredDev it = a.items[s.item];
  const PredBlendDev bl = blend[s.item];
  L.ref[0] = it.ref[0]; L.ref[1] = it.ref[1]; L.stride[0] = it.stride[0]; L.stride[1] = it.stride[1];
  L.fx[0] = it.frac[0][0]; L.fy[0] = it.frac[0][1]; L.fx[1] = it.frac[1][0]; L.fy[1] = it.frac[1][1];
  L.w = it.w; L.h = it.h; L.alt = it.alt; L.x0 = s.x0; L.y0 = s.y0;
  L.mode = MODE_BI;
  L.ba = bl.a; L.bb = bl.b; L.bc = bl.c; L.blo = bl.lo; L.bhi = bl.hi;
  L.dstPitch = a.predStride ? a.predStride : it.w;
  L.dst = a.pred + it.dstOff;
  L.org = a.org ? a.org + it.orgOff : nullptr; L.orgPitch = a.orgStride;
  L.res = a.resi ? a.resi + it.dstOff : nullptr; L.resPitch = L.dstPitch;
  predDispatchBlend( u.kind, L, u.tw, u.th, u.log2SegsRow, lanes, a.bitDepth );
}

// the units of CIIP items (vvhip_pred_inter_batch_ciip): the item as it is otherwise — one list, the default average or BCW — then the weighting with planar intra prediction
// from the item's line of the caller's reference-sample array.  A kernel of its own, as the other forms: they keep their registers.
__global__ void __launch_bounds__( 256 )
predListCiipKernel( PredArgs a, const PredCiipDev* __restrict__ ciip, const int16_t* __restrict__ intraRef )
{
  extern __shared__ __attribute__( ( aligned( 16 ) ) ) int16_t sPred[];
  const int wave = __builtin_amdgcn_readfirstlane( ( int ) ( threadIdx.x >> 6 ) ), lane = threadIdx.x & 63;
  const int ui = ( int ) blockIdx.x * 4 + wave;
  if( ui >= a.nUnits ) return;
  const PredUnit u = a.units[ui];
  if( u.nSub == 0 ) return;
  const int nt = u.kind <= KIND_L4 ? 8 : 4, lanes = 1 << u.log2Lanes, si = lane >> u.log2Lanes;
  Lane L;
  L.on = si < u.nSub;
  L.lis = lane & ( lanes - 1 );
  L.win = sPred + ( size_t ) wave * a.ldsPerWave + ( size_t ) si * subElems( u.tw, u.th, nt );
  L.tmp = L.win + winElems( u.tw, u.th, nt );
  const PredSub s = a.subs[u.firstSub + ( L.on ? si : 0 )];
  const PredDev it = a.items[s.item];
  const PredCiipDev ci = ciip[s.item];
  L.ref[0] = it.ref[0]; L.ref[1] = it.ref[1]; L.stride[0] = it.stride[0]; L.stride[1] = it.stride[1];
  L.fx[0] = it.frac[0][0]; L.fy[0] = it.frac[0][1]; L.fx[1] = it.frac[1][0]; L.fy[1] = it.frac[1][1];
  L.w = it.w; L.h = it.h; L.alt = it.alt; L.x0 = s.x0; L.y0 = s.y0;
  L.mode = it.ref[0] && it.ref[1] ? MODE_BI : MODE_UNI;
  if( !it.ref[0] ) { L.ref[0] = it.ref[1]; L.stride[0] = it.stride[1]; L.fx[0] = L.fx[1]; L.fy[0] = L.fy[1]; L.ref[1] = nullptr; }      // a list-1-only block runs as the first pass
  L.line = intraRef + ci.refOff; L.cw0 = ci.w0; L.cwI = ci.wI; L.cfilt = ci.filt; L.cpdpc = ci.pdpc;
  L.dstPitch = a.predStride ? a.predStride : it.w;
  L.dst = a.pred + it.dstOff;
  L.org = a.org ? a.org + it.orgOff : nullptr; L.orgPitch = a.orgStride;
  L.res = a.resi ? a.resi + it.dstOff : nullptr; L.resPitch = L.dstPitch;
  predDispatchCiip( u.kind, L, u.tw, u.th, u.log2SegsRow, lanes, a.bitDepth );
}

// one block size per call, items on the device (the chroma twin of vvhip_interp_luma_batch): tile g of the launch is tile g % tilesPerItem of item g / tilesPerItem
__global__ void __launch_bounds__( 256 )
predOneSizeKernel( const int16_t* __restrict__ ref, int refStride, const vvhip_subpel_item* __restrict__ items, int n, int w, int h, int bitDepth, int rndRes,
                   int kind, int tw, int th, int log2SegsRow, int log2Lanes, int ldsPerWave, int16_t* __restrict__ out )
{
  extern __shared__ __attribute__( ( aligned( 16 ) ) ) int16_t sPred[];
  const int wave = __builtin_amdgcn_readfirstlane( ( int ) ( threadIdx.x >> 6 ) ), lane = threadIdx.x & 63;
  const int lanes = 1 << log2Lanes, si = lane >> log2Lanes, tilesX = w / tw, tilesPerItem = tilesX * ( h / th );
  const long long g = ( ( long long ) blockIdx.x * 4 + wave ) * ( 64 >> log2Lanes ) + si;
  if( ( ( long long ) blockIdx.x * 4 + wave ) * ( 64 >> log2Lanes ) >= ( long long ) n * tilesPerItem ) return;
  Lane L;
  L.on = g < ( long long ) n * tilesPerItem;
  const int item = L.on ? ( int ) ( g / tilesPerItem ) : 0, t = L.on ? ( int ) ( g - ( long long ) item * tilesPerItem ) : 0;
  const vvhip_subpel_item it = items[item];
  L.lis = lane & ( lanes - 1 );
  L.win = sPred + ( size_t ) wave * ldsPerWave + ( size_t ) si * subElems( tw, th, 4 );
  L.tmp = L.win + winElems( tw, th, 4 );
  L.ref[0] = ref + it.ref_off; L.ref[1] = nullptr; L.stride[0] = L.stride[1] = refStride;
  L.fx[0] = it.frac_x & 31; L.fy[0] = it.frac_y & 31; L.fx[1] = L.fy[1] = 0;
  L.w = w; L.h = h; L.alt = 0; L.x0 = ( t % tilesX ) * tw; L.y0 = ( t / tilesX ) * th;
  L.mode = rndRes ? MODE_UNI : MODE_RAW;
  L.dst = out + ( size_t ) item * w * h; L.dstPitch = w;
  L.org = nullptr; L.orgPitch = 0; L.res = nullptr; L.resPitch = 0;
  predDispatch( kind, L, tw, th, log2SegsRow, lanes, bitDepth );
}

// XCD-aware order of a class's workgroups (as me.hip's xcdBandOrder): workgroups are dealt round-robin to the 8 XCDs, each with a private L2; workgroup base + l of the launch
// is handed the next entry of the ( ( base + l ) % 8 )-th contiguous eighth of the class, whose entries are sorted by picture position: every L2 streams one horizontal band.
} // namespace
std::vector<int> predBandOrder( int nGroups, int base )      // (shared with predaffine.hip: declared in common.h)
{
  std::vector<int> perm( nGroups );
  const int q = ( nGroups + 7 ) / 8;
  int cursor[8], endOf[8];
  for( int x = 0; x < 8; x++ ) { cursor[x] = std::min( nGroups, x * q ); endOf[x] = std::min( nGroups, ( x + 1 ) * q ); }
  for( int l = 0; l < nGroups; l++ )
  {
    int x = ( base + l ) & 7;
    for( int t = 0; t < 8 && cursor[x] >= endOf[x]; t++ ) x = ( x + 1 ) & 7;
    perm[l] = cursor[x]++;
  }
  return perm;
}
namespace {

// the head of the schedule's blob: where its sections lie and what the launches need to know of them.  One unit table: the plain units, then the units of items with an
// extension (BDOF, DMVR's padded reference), of BCW / GEO items, of CIIP items — a kernel of its own each, with its own LDS per wave
struct PredHead
{
  size_t offItems, offSubs, offUnits, offBlend, offCiip;
  int    units, ldsPerWave, unitsEx, ldsPerWaveEx, unitsBlend, ldsPerWaveBlend, unitsCiip, ldsPerWaveCiip;
};

// ---- GEO: split direction + CU size -> the weight line of one component block (host) ----
// The reference reads g_globalGeoWeights[mask][my * 112 + mx] with mx = offX + X ( 111 - offX - X under mirror 1 ), my = offY + Y ( 111 - offY - Y under mirror 2 ),
// ( X, Y ) = ( x, y ) << scale (InterpolationFilter.cpp:1024-1062); the mask entry is Clip3( 0, 8, ( 2 Dx mx + 2 Dy my + 36 - 111 ( Dx + Dy ) ) >> 3 ) with
// Dx = g_Dis[angle], Dy = g_Dis[angle + 8] of the mask's own angle (Rom.cpp:1320-1342: sample positions 2 ( m + 8 ) + 1, rho = 128 ( Dx + Dy ), + 32 + 4).
const int8_t kGeoAngle2Mask[32]   = { 0, -1, 1, 2, 3, 4, -1, -1, 5, -1, -1, 4, 3, 2, 1, -1, 0, -1, 1, 2, 3, 4, -1, -1, 5, -1, -1, 4, 3, 2, 1, -1 };
const int8_t kGeoDis[32]          = { 8, 8, 8, 8, 4, 4, 2, 1, 0, -1, -2, -4, -4, -8, -8, -8, -8, -8, -8, -8, -4, -4, -2, -1, 0, 1, 2, 4, 4, 8, 8, 8 };
const int8_t kGeoAngle2Mirror[32] = { 0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 2, 2, 2, 2 };
const int8_t kGeoMaskAngle[6]     = { 0, 2, 3, 4, 5, 8 };      // the angle whose line a prestored mask holds
void geoLine( int splitDir, int log2CuW, int log2CuH, int chroma, PredBlendDev& o )
{
  int angle = 0, distance = 0, mode = 0;      // g_GeoParams (Rom.cpp:1306-1319)
  for( int ai = 0; ai < 32; ai++ ) for( int di = 0; di < 4; di++ )
  {
    if( ( di == 0 && ai >= 16 ) || ( ( di == 2 || di == 0 ) && ( kGeoAngle2Mask[ai] == 0 || kGeoAngle2Mask[ai] == 5 ) ) || kGeoAngle2Mask[ai] == -1 ) continue;
    if( mode++ == splitDir ) { angle = ai; distance = di; }
  }
  const int W = 1 << log2CuW, H = 1 << log2CuH;      // g_weightOffset (:1344-1370)
  int offX = ( 112 - W ) >> 1, offY = ( 112 - H ) >> 1;
  if( distance > 0 )
  {
    if( angle % 16 == 8 || ( angle % 16 != 0 && H >= W ) ) offY += angle < 16 ? ( distance * H ) >> 3 : -( ( distance * H ) >> 3 );
    else offX += angle < 16 ? ( distance * W ) >> 3 : -( ( distance * W ) >> 3 );
  }
  const int base = kGeoMaskAngle[kGeoAngle2Mask[angle]], Dx = kGeoDis[base], Dy = kGeoDis[base + 8];
  const int A = 2 * Dx, B = 2 * Dy, C = 36 - 111 * ( Dx + Dy ), mirror = kGeoAngle2Mirror[angle];
  const int sx = mirror == 1 ? -1 : 1, sy = mirror == 2 ? -1 : 1;
  o.a = sx * A * ( 1 << chroma ); o.b = sy * B * ( 1 << chroma );
  o.c = C + A * ( mirror == 1 ? 111 - offX : offX ) + B * ( mirror == 2 ? 111 - offY : offY );
  o.lo = 0; o.hi = 8;
}
const int8_t kBcwW1[5] = { -2, 3, 4, 5, 10 };      // g_BcwWeights (Rom.cpp:1152)

// validates the list, derives the schedule and uploads it; on success the context's key names the list (items + plane table) the device copy belongs to
int predBuildSchedule( vvhip_ctx* ctx, HostList& S, const vvhip_me_plane* planes_host, int n_planes, const vvhip_pred_item* items_host, const vvhip_pred_ext* ext_host,
                       const vvhip_pred_blend* blend_host, const vvhip_pred_ciip* ciip_host, const int16_t* d_intra_ref, int n, std::vector<unsigned char>& key )
{
  // ---- validation + plane table resolved; nothing is launched when any item is unsupported
  std::vector<PredDev> dev( n );
  std::vector<ListKeyed> order( n );
  std::vector<PredBlendDev> blendDev( blend_host ? n : 0 );
  std::vector<PredCiipDev> ciipDev( ciip_host ? n : 0 );
  for( int i = 0; i < n; i++ )
  {
    const vvhip_pred_item& it = items_host[i];
    const int lo = it.chroma ? 2 : 4, hi = it.chroma ? 64 : 128, fmax = it.chroma ? 32 : 16;
    if( it.chroma > 1 || !isPow2( it.width ) || !isPow2( it.height ) || it.width < lo || it.height < lo || it.width > hi || it.height > hi )
      return vvhip_fail( ctx, VVHIP_E_ARG, "vvhip_pred_inter_batch: item %d: %s block %dx%d (width and height powers of two, luma 4..128, chroma 2..64)", i, it.chroma ? "chroma" : "luma", it.width, it.height );
    if( it.ref_plane[0] < 0 && it.ref_plane[1] < 0 ) return vvhip_fail( ctx, VVHIP_E_ARG, "vvhip_pred_inter_batch: item %d uses neither reference list", i );
    if( it.alt_hpel && it.chroma ) return vvhip_fail( ctx, VVHIP_E_ARG, "vvhip_pred_inter_batch: item %d: the alternative half-sample filter is a luma filter", i );
    PredDev& d = dev[i];
    memset( &d, 0, sizeof( d ) );
    for( int l = 0; l < 2; l++ )
    {
      if( it.ref_plane[l] < 0 ) continue;
      if( it.ref_plane[l] >= n_planes || !planes_host[it.ref_plane[l]].d_base )
        return vvhip_fail( ctx, VVHIP_E_ARG, "vvhip_pred_inter_batch: item %d: list %d names plane %d of a table of %d", i, l, it.ref_plane[l], n_planes );
      if( it.frac[l][0] < 0 || it.frac[l][0] >= fmax || it.frac[l][1] < 0 || it.frac[l][1] >= fmax )
        return vvhip_fail( ctx, VVHIP_E_ARG, "vvhip_pred_inter_batch: item %d: list %d fraction (%d, %d) outside 0..%d", i, l, it.frac[l][0], it.frac[l][1], fmax - 1 );
      d.ref[l] = planes_host[it.ref_plane[l]].d_base + it.ref_off[l];
      d.stride[l] = planes_host[it.ref_plane[l]].stride;
      d.frac[l][0] = it.frac[l][0]; d.frac[l][1] = it.frac[l][1];
    }
    d.dstOff = it.dst_off; d.orgOff = it.org_off; d.w = it.width; d.h = it.height; d.alt = it.alt_hpel ? 1 : 0;
    // ---- the extension: BDOF (luma, both lists, min( w, h ) >= 8 and w * h >= 128: InterPrediction.cpp:465-490) and DMVR's padded reference (|delta| <= DMVR_NUM_ITERATION >> scale)
    uint32_t flags = 0;
    if( ext_host )
    {
      const vvhip_pred_ext& e = ext_host[i];
      if( ( e.flags & ~( VVHIP_PRED_EXT_BDOF | VVHIP_PRED_EXT_DMVR_PAD ) ) || e.rsv[0] || e.rsv[1] || e.rsv[2] )
        return vvhip_fail( ctx, VVHIP_E_ARG, "vvhip_pred_inter_batch_ex: item %d: unknown flag bits or non-zero reserved bytes in the extension", i );
      flags = e.flags;
      if( flags & VVHIP_PRED_EXT_BDOF )
      {
        if( it.chroma ) return vvhip_fail( ctx, VVHIP_E_ARG, "vvhip_pred_inter_batch_ex: item %d: BDOF is a luma tool", i );
        if( it.ref_plane[0] < 0 || it.ref_plane[1] < 0 ) return vvhip_fail( ctx, VVHIP_E_ARG, "vvhip_pred_inter_batch_ex: item %d: BDOF needs both reference lists", i );
        if( std::min( it.width, it.height ) < 8 || it.width * it.height < 128 )
          return vvhip_fail( ctx, VVHIP_E_ARG, "vvhip_pred_inter_batch_ex: item %d: BDOF on a %dx%d block (min( w, h ) >= 8 and w * h >= 128)", i, it.width, it.height );
      }
      if( flags & VVHIP_PRED_EXT_DMVR_PAD )
      {
        const int lim = it.chroma ? 1 : 2;
        for( int l = 0; l < 2; l++ )
          if( e.pad_dx[l] < -lim || e.pad_dx[l] > lim || e.pad_dy[l] < -lim || e.pad_dy[l] > lim )
            return vvhip_fail( ctx, VVHIP_E_ARG, "vvhip_pred_inter_batch_ex: item %d: list %d integer delta (%d, %d) outside -%d..%d", i, l, e.pad_dx[l], e.pad_dy[l], lim, lim );
        if( ( flags & VVHIP_PRED_EXT_BDOF ) && ( it.width > 16 || it.height > 16 ) )
          return vvhip_fail( ctx, VVHIP_E_ARG, "vvhip_pred_inter_batch_ex: item %d: a DMVR sub-block with BDOF is at most 16x16, not %dx%d", i, it.width, it.height );
        d.pad[1] = ( uint8_t ) ( ( e.pad_dx[0] + 2 ) | ( ( e.pad_dy[0] + 2 ) << 4 ) ); d.pad[2] = ( uint8_t ) ( ( e.pad_dx[1] + 2 ) | ( ( e.pad_dy[1] + 2 ) << 4 ) );
      }
      d.pad[0] = ( uint8_t ) flags;
    }
    // ---- the blend record: BCW (any size) or GEO (a whole component block of a CU 8..64 x 8..64); both hypotheses, no BDOF / DMVR (InterPrediction.cpp:478, :975)
    const bool bi = it.ref_plane[0] >= 0 && it.ref_plane[1] >= 0;
    uint32_t blended = 0;
    if( blend_host )
    {
      const vvhip_pred_blend& b = blend_host[i];
      memset( &blendDev[i], 0, sizeof( PredBlendDev ) );
      if( b.mode > VVHIP_PRED_BLEND_GEO || b.rsv[0] || b.rsv[1] )
        return vvhip_fail( ctx, VVHIP_E_ARG, "vvhip_pred_inter_batch_blend: item %d: unknown blend mode %d or non-zero reserved bytes", i, b.mode );
      if( b.mode != VVHIP_PRED_BLEND_DEFAULT )
      {
        const char* tool = b.mode == VVHIP_PRED_BLEND_BCW ? "BCW" : "GEO";
        if( b.param > ( b.mode == VVHIP_PRED_BLEND_BCW ? 4 : 63 ) ) return vvhip_fail( ctx, VVHIP_E_ARG, "vvhip_pred_inter_batch_blend: item %d: %s parameter %d out of range", i, tool, b.param );
        if( !bi ) return vvhip_fail( ctx, VVHIP_E_ARG, "vvhip_pred_inter_batch_blend: item %d: %s needs both hypotheses", i, tool );
        if( flags ) return vvhip_fail( ctx, VVHIP_E_ARG, "vvhip_pred_inter_batch_blend: item %d: %s excludes BDOF and DMVR's padded reference", i, tool );
        if( b.mode == VVHIP_PRED_BLEND_BCW )
        {
          const int w0 = 8 - kBcwW1[b.param];
          blendDev[i].c = 8 * w0; blendDev[i].lo = blendDev[i].hi = ( int16_t ) w0;
        }
        else
        {
          const int lo = it.chroma ? 4 : 8, hi = it.chroma ? 32 : 64;
          if( it.width < lo || it.height < lo || it.width > hi || it.height > hi )
            return vvhip_fail( ctx, VVHIP_E_ARG, "vvhip_pred_inter_batch_blend: item %d: GEO on a %s block %dx%d (the component block of a CU 8..64 x 8..64)", i, it.chroma ? "chroma" : "luma", it.width, it.height );
          geoLine( b.param, ilog2i( it.width ) + it.chroma, ilog2i( it.height ) + it.chroma, it.chroma, blendDev[i] );
        }
        blended = 1;
      }
    }
    // ---- the CIIP record: a whole component block of a CIIP CU (luma 4..64 with w * h >= 64; 4:2:0 chroma 4..32 wide, 2..32 high, w * h >= 16: EncCu.cpp:1926, :2213-2219),
    //      one list, the default average or BCW; no GEO, no BDOF / DMVR (InterPrediction.cpp:468, UnitTools.cpp:1309).  Such an item runs in the CIIP kernel whatever its blend record.
    uint32_t ciipOn = 0;
    if( ciip_host )
    {
      const vvhip_pred_ciip& c = ciip_host[i];
      memset( &ciipDev[i], 0, sizeof( PredCiipDev ) );
      if( c.mode > VVHIP_PRED_CIIP_ON || c.rsv[0] || c.rsv[1] )
        return vvhip_fail( ctx, VVHIP_E_ARG, "vvhip_pred_inter_batch_ciip: item %d: unknown CIIP mode %d or non-zero reserved bytes", i, c.mode );
      if( c.mode == VVHIP_PRED_CIIP_ON )
      {
        if( c.num_intra > 2 ) return vvhip_fail( ctx, VVHIP_E_ARG, "vvhip_pred_inter_batch_ciip: item %d: num_intra %d (0..2)", i, c.num_intra );
        if( c.ref_off < 0 ) return vvhip_fail( ctx, VVHIP_E_ARG, "vvhip_pred_inter_batch_ciip: item %d: negative offset %d into the intra reference samples", i, c.ref_off );
        if( !d_intra_ref ) return vvhip_fail( ctx, VVHIP_E_ARG, "vvhip_pred_inter_batch_ciip: item %d is a CIIP item and there are no intra reference samples", i );
        const bool sizeOk = it.chroma ? ( it.width >= 4 && it.width <= 32 && it.height >= 2 && it.height <= 32 && it.width * it.height >= 16 )
                                      : ( it.width >= 4 && it.width <= 64 && it.height >= 4 && it.height <= 64 && it.width * it.height >= 64 );
        if( !sizeOk )
          return vvhip_fail( ctx, VVHIP_E_ARG, "vvhip_pred_inter_batch_ciip: item %d: CIIP on a %s block %dx%d (luma 4..64 with w * h >= 64; chroma 4..32 wide, 2..32 high, w * h >= 16)", i, it.chroma ? "chroma" : "luma", it.width, it.height );
        if( blend_host && blend_host[i].mode == VVHIP_PRED_BLEND_GEO ) return vvhip_fail( ctx, VVHIP_E_ARG, "vvhip_pred_inter_batch_ciip: item %d: CIIP excludes GEO", i );
        if( flags ) return vvhip_fail( ctx, VVHIP_E_ARG, "vvhip_pred_inter_batch_ciip: item %d: CIIP excludes BDOF and DMVR's padded reference", i );
        ciipDev[i].refOff = c.ref_off; ciipDev[i].w0 = ( int8_t ) ( blended ? blendDev[i].lo : 4 ); ciipDev[i].wI = ( uint8_t ) ( c.num_intra + 1 );
        ciipDev[i].filt = it.chroma ? 0 : 1; ciipDev[i].pdpc = std::min( it.width, it.height ) >= 4 ? 1 : 0;
        ciipOn = 1; blended = 0;
      }
    }
    // size class: the most samples first (their waves run longest), then shape, form, component and uni / bi — a wave never mixes classes; inside a class picture order
    order[i].cls = ( ( uint32_t ) ( 14 - ilog2i( it.width ) - ilog2i( it.height ) ) << 10 ) | ( ( uint32_t ) ilog2i( it.width ) << 6 ) | ( ciipOn << 5 ) | ( blended << 4 ) | ( flags << 2 ) | ( it.chroma ? 2u : 0u ) | ( bi ? 1u : 0u );
    const int l0 = it.ref_plane[0] >= 0 ? 0 : 1;
    order[i].pos = ( ( int64_t ) it.ref_off[l0] << 5 ) | ( uint32_t ) ( it.ref_plane[l0] & 31 );
    order[i].idx = i;
  }
  std::sort( order.begin(), order.end() );

  // ---- schedule: per class the tiles in picture order, 64 lanes' worth per wave, four waves per workgroup, workgroups dealt to the XCDs in bands
  //      classes with an extension flag go to a list of their own, which predListExKernel runs; a BDOF block is cut into its 16x16 / 16x8 / 8x16 units (xSubPuBDOF :326-357)
  std::vector<PredSub> subs;
  std::vector<PredUnit> unitsPlain, unitsEx, unitsBlend, unitsCiip;
  int ldsPerWave = 0, ldsPerWaveEx = 0, ldsPerWaveBlend = 0, ldsPerWaveCiip = 0;
  for( int c0 = 0; c0 < n; )
  {
    int c1 = c0; while( c1 < n && order[c1].cls == order[c0].cls ) c1++;
    const vvhip_pred_item& f = items_host[order[c0].idx];
    const uint32_t flags = ( order[c0].cls >> 2 ) & 3u;
    const bool blended = ( order[c0].cls >> 4 ) & 1u, ciipOn = ( order[c0].cls >> 5 ) & 1u;
    std::vector<PredUnit>& units = ciipOn ? unitsCiip : blended ? unitsBlend : flags ? unitsEx : unitsPlain;
    TileShape ts = tileShape( f.width, f.height, f.chroma != 0 );
    if( flags & VVHIP_PRED_EXT_BDOF )
    {
      ts.tw = std::min<int>( f.width, 16 ); ts.th = std::min<int>( f.height, 16 );
      ts.log2SegsRow = ilog2i( ts.tw / 8 ); ts.log2Lanes = ts.log2SegsRow + ilog2i( ts.th );
    }
    const int subsPerWave = 64 >> ts.log2Lanes, nt = tapsOfKind( ts.kind );
    if( ciipOn ) ldsPerWaveCiip = std::max( ldsPerWaveCiip, subsPerWave * subElems( ts.tw, ts.th, nt ) );
    else if( blended ) ldsPerWaveBlend = std::max( ldsPerWaveBlend, subsPerWave * subElems( ts.tw, ts.th, nt ) );
    else if( flags ) ldsPerWaveEx = std::max( ldsPerWaveEx, subsPerWave * ( subElems( ts.tw, ts.th, nt ) + ( ( flags & VVHIP_PRED_EXT_BDOF ) ? bdofElems( ts.tw, ts.th ) : 0 ) ) );
    else ldsPerWave = std::max( ldsPerWave, subsPerWave * subElems( ts.tw, ts.th, nt ) );
    const size_t firstSub = subs.size();
    for( int k = c0; k < c1; k++ )
      for( int y0 = 0; y0 < f.height; y0 += ts.th ) for( int x0 = 0; x0 < f.width; x0 += ts.tw ) subs.push_back( PredSub{ order[k].idx, ( int16_t ) x0, ( int16_t ) y0 } );
    const int nSubs = ( int ) ( subs.size() - firstSub ), nWaves = ( nSubs + subsPerWave - 1 ) / subsPerWave, nWg = ( nWaves + 3 ) / 4;
    const std::vector<int> perm = predBandOrder( nWg, ( int ) ( units.size() / 4 ) );
    for( int l = 0; l < nWg; l++ ) for( int wv = 0; wv < 4; wv++ )
    {
      const int q = perm[l] * 4 + wv;
      PredUnit u; memset( &u, 0, sizeof( u ) );
      u.tw = ( int16_t ) ts.tw; u.th = ( int16_t ) ts.th; u.kind = ( uint8_t ) ts.kind; u.log2Lanes = ( uint8_t ) ts.log2Lanes; u.log2SegsRow = ( uint8_t ) ts.log2SegsRow; u.pad[0] = ( uint8_t ) flags;
      if( q < nWaves ) { u.firstSub = ( int32_t ) ( firstSub + ( size_t ) q * subsPerWave ); u.nSub = ( int16_t ) std::min( subsPerWave, nSubs - q * subsPerWave ); }
      units.push_back( u );
    }
    c0 = c1;
  }

  // ---- the blob: head, items, tiles, units, blend records, CIIP records right behind those
  std::vector<PredUnit> units( unitsPlain );
  units.insert( units.end(), unitsEx.begin(), unitsEx.end() );
  units.insert( units.end(), unitsBlend.begin(), unitsBlend.end() );
  units.insert( units.end(), unitsCiip.begin(), unitsCiip.end() );
  PredHead H;
  ListBlob blob( &H, sizeof( H ) );
  H.offItems = blob.add( dev.data(), dev.size() * sizeof( PredDev ) );
  H.offSubs = blob.add( subs.data(), subs.size() * sizeof( PredSub ) );
  H.offUnits = blob.add( units.data(), units.size() * sizeof( PredUnit ) );
  H.offBlend = blob.add( blendDev.data(), blendDev.size() * sizeof( PredBlendDev ) );
  H.offCiip = blob.add( ciipDev.data(), ciipDev.size() * sizeof( PredCiipDev ), sizeof( PredBlendDev ) );
  H.units = ( int ) unitsPlain.size(); H.ldsPerWave = ldsPerWave; H.unitsEx = ( int ) unitsEx.size(); H.ldsPerWaveEx = ldsPerWaveEx;
  H.unitsBlend = ( int ) unitsBlend.size(); H.ldsPerWaveBlend = ldsPerWaveBlend; H.unitsCiip = ( int ) unitsCiip.size(); H.ldsPerWaveCiip = ldsPerWaveCiip;
  return listUpload( ctx, S, blob, &key );
}

int predInterBatch( vvhip_ctx* ctx, const vvhip_me_plane* planes_host, int n_planes, const vvhip_pred_item* items_host, const vvhip_pred_ext* ext_host,
                    const vvhip_pred_blend* blend_host, const vvhip_pred_ciip* ciip_host, const int16_t* d_intra_ref, int n, int bit_depth, int16_t* d_pred, int pred_stride,
                    const int16_t* d_org, int org_stride, int16_t* d_resi )
{
  if( !ctx ) return VVHIP_E_ARG;
  if( !planes_host || n_planes < 1 || n_planes > 16 || n < 0 || n > ( 1 << 24 ) || bit_depth < 8 || bit_depth > 12 || pred_stride < 0 || ( n && ( !items_host || !d_pred ) ) || ( d_resi && !d_org ) )
    return vvhip_fail( ctx, VVHIP_E_ARG, "vvhip_pred_inter_batch: %d planes (1..16), %d items, bitDepth %d, prediction %p pitch %d, original %p, residual %p", n_planes, n, bit_depth,
                       ( void* ) d_pred, pred_stride, ( const void* ) d_org, ( void* ) d_resi );
  for( int p = 0; p < n_planes; p++ )
    if( planes_host[p].d_base && ( planes_host[p].stride < 2 || ( planes_host[p].stride & 1 ) ) )
      return vvhip_fail( ctx, VVHIP_E_ARG, "vvhip_pred_inter_batch: plane %d has stride %d (reference planes need an even row pitch in samples)", p, planes_host[p].stride );
  if( n == 0 ) return VVHIP_OK;

  // ---- a list that is run again (same items, same plane table) is launched at once: no sort, no upload, no allocation, no wait — such a call can be recorded in a launch graph
  //      (the extensions are part of the list: the same items with other extensions are another schedule)
  //      A list with a blend array keeps a schedule of its own (and its array is part of its key), and so does a list with a CIIP array.  The intra reference samples are
  //      device data like the planes: their address and contents are not part of the key (the address is a kernel argument of every launch).
  HostList& S = ctx->list[ciip_host ? LIST_PRED_CIIP : blend_host ? LIST_PRED_BLEND : LIST_PRED];
  const size_t bKeyItems = sizeof( int ) + ( size_t ) n_planes * sizeof( vvhip_me_plane ) + ( size_t ) n * sizeof( vvhip_pred_item ), bKeyExt = ext_host ? ( size_t ) n * sizeof( vvhip_pred_ext ) : 0;
  const size_t bKeyBlend = blend_host ? 1 + ( size_t ) n * sizeof( vvhip_pred_blend ) : 0;
  std::vector<unsigned char> key( bKeyItems + bKeyExt + bKeyBlend + ( ciip_host ? 2 + ( size_t ) n * sizeof( vvhip_pred_ciip ) : 0 ) );
  if( ext_host ) memcpy( key.data() + bKeyItems, ext_host, bKeyExt );
  if( blend_host ) { key[bKeyItems + bKeyExt] = ext_host ? 1 : 0; memcpy( key.data() + bKeyItems + bKeyExt + 1, blend_host, ( size_t ) n * sizeof( vvhip_pred_blend ) ); }
  if( ciip_host )
  {
    unsigned char* k = key.data() + bKeyItems + bKeyExt + bKeyBlend;
    k[0] = ext_host ? 1 : 0; k[1] = blend_host ? 1 : 0;
    memcpy( k + 2, ciip_host, ( size_t ) n * sizeof( vvhip_pred_ciip ) );
  }
  memcpy( key.data(), &n_planes, sizeof( int ) );
  memcpy( key.data() + sizeof( int ), planes_host, ( size_t ) n_planes * sizeof( vvhip_me_plane ) );
  memcpy( key.data() + sizeof( int ) + ( size_t ) n_planes * sizeof( vvhip_me_plane ), items_host, ( size_t ) n * sizeof( vvhip_pred_item ) );
  bool current = false;
  int rc = listCurrent( ctx, S, key, &current );
  if( rc == VVHIP_OK && !current ) rc = predBuildSchedule( ctx, S, planes_host, n_planes, items_host, ext_host, blend_host, ciip_host, d_intra_ref, n, key );
  if( rc ) return rc;
  const PredHead& H = listHead<PredHead>( S );
  if( H.unitsCiip && !d_intra_ref ) return vvhip_fail( ctx, VVHIP_E_ARG, "vvhip_pred_inter_batch_ciip: the list has CIIP items and there are no intra reference samples" );
  const char* base = static_cast<const char*>( S.d );
  const PredUnit* units = reinterpret_cast<const PredUnit*>( base + H.offUnits );
  PredArgs a;
  a.items = reinterpret_cast<const PredDev*>( base + H.offItems ); a.subs = reinterpret_cast<const PredSub*>( base + H.offSubs ); a.bitDepth = bit_depth;
  a.pred = d_pred; a.predStride = pred_stride; a.org = d_resi ? d_org : nullptr; a.orgStride = org_stride; a.resi = d_resi;
  if( H.units )
  {
    a.units = units; a.nUnits = H.units; a.ldsPerWave = H.ldsPerWave;
    hipLaunchKernelGGL( predListKernel, dim3( ( unsigned ) ( a.nUnits / 4 ) ), dim3( 256 ), ( size_t ) a.ldsPerWave * 4 * sizeof( int16_t ), ctx->stream, a );
    VVHIP_LAUNCH_CHECK( ctx );
  }
  if( H.unitsEx )
  {
    a.units = units + H.units; a.nUnits = H.unitsEx; a.ldsPerWave = H.ldsPerWaveEx;
    hipLaunchKernelGGL( predListExKernel, dim3( ( unsigned ) ( a.nUnits / 4 ) ), dim3( 256 ), ( size_t ) a.ldsPerWave * 4 * sizeof( int16_t ), ctx->stream, a );
    VVHIP_LAUNCH_CHECK( ctx );
  }
  if( H.unitsBlend )
  {
    a.units = units + H.units + H.unitsEx; a.nUnits = H.unitsBlend; a.ldsPerWave = H.ldsPerWaveBlend;
    hipLaunchKernelGGL( predListBlendKernel, dim3( ( unsigned ) ( a.nUnits / 4 ) ), dim3( 256 ), ( size_t ) a.ldsPerWave * 4 * sizeof( int16_t ), ctx->stream, a,
                        reinterpret_cast<const PredBlendDev*>( base + H.offBlend ) );
    VVHIP_LAUNCH_CHECK( ctx );
  }
  if( H.unitsCiip )
  {
    a.units = units + H.units + H.unitsEx + H.unitsBlend; a.nUnits = H.unitsCiip; a.ldsPerWave = H.ldsPerWaveCiip;
    hipLaunchKernelGGL( predListCiipKernel, dim3( ( unsigned ) ( a.nUnits / 4 ) ), dim3( 256 ), ( size_t ) a.ldsPerWave * 4 * sizeof( int16_t ), ctx->stream, a,
                        reinterpret_cast<const PredCiipDev*>( base + H.offCiip ), d_intra_ref );
    VVHIP_LAUNCH_CHECK( ctx );
  }
  return listLaunched( ctx, S );
}

} // namespace

extern "C" {

int vvhip_pred_inter_batch( vvhip_ctx* ctx, const vvhip_me_plane* planes_host, int n_planes, const vvhip_pred_item* items_host, int n, int bit_depth,
                            int16_t* d_pred, int pred_stride, const int16_t* d_org, int org_stride, int16_t* d_resi )
{
  return predInterBatch( ctx, planes_host, n_planes, items_host, nullptr, nullptr, nullptr, nullptr, n, bit_depth, d_pred, pred_stride, d_org, org_stride, d_resi );
}

int vvhip_pred_inter_batch_ex( vvhip_ctx* ctx, const vvhip_me_plane* planes_host, int n_planes, const vvhip_pred_item* items_host, const vvhip_pred_ext* ext_host, int n, int bit_depth,
                               int16_t* d_pred, int pred_stride, const int16_t* d_org, int org_stride, int16_t* d_resi )
{
  return predInterBatch( ctx, planes_host, n_planes, items_host, ext_host, nullptr, nullptr, nullptr, n, bit_depth, d_pred, pred_stride, d_org, org_stride, d_resi );
}

int vvhip_pred_inter_batch_blend( vvhip_ctx* ctx, const vvhip_me_plane* planes_host, int n_planes, const vvhip_pred_item* items_host, const vvhip_pred_ext* ext_host,
                                  const vvhip_pred_blend* blend_host, int n, int bit_depth, int16_t* d_pred, int pred_stride, const int16_t* d_org, int org_stride, int16_t* d_resi )
{
  return predInterBatch( ctx, planes_host, n_planes, items_host, ext_host, blend_host, nullptr, nullptr, n, bit_depth, d_pred, pred_stride, d_org, org_stride, d_resi );
}

int vvhip_pred_inter_batch_ciip( vvhip_ctx* ctx, const vvhip_me_plane* planes_host, int n_planes, const vvhip_pred_item* items_host, const vvhip_pred_ext* ext_host,
                                 const vvhip_pred_blend* blend_host, const vvhip_pred_ciip* ciip_host, const int16_t* d_intra_ref, int n, int bit_depth,
                                 int16_t* d_pred, int pred_stride, const int16_t* d_org, int org_stride, int16_t* d_resi )
{
  return predInterBatch( ctx, planes_host, n_planes, items_host, ext_host, blend_host, ciip_host, d_intra_ref, n, bit_depth, d_pred, pred_stride, d_org, org_stride, d_resi );
}

int vvhip_get_geo_weights_host( int split_dir, int log2_cu_w, int log2_cu_h, int chroma, int8_t* host_out )
{
  if( split_dir < 0 || split_dir > 63 || log2_cu_w < 3 || log2_cu_w > 6 || log2_cu_h < 3 || log2_cu_h > 6 || chroma < 0 || chroma > 1 || !host_out ) return VVHIP_E_ARG;
  PredBlendDev g;
  geoLine( split_dir, log2_cu_w, log2_cu_h, chroma, g );
  const int w = ( 1 << log2_cu_w ) >> chroma, h = ( 1 << log2_cu_h ) >> chroma;
  for( int y = 0; y < h; y++ ) for( int x = 0; x < w; x++ ) host_out[y * w + x] = ( int8_t ) vvhipBlendW0( g.a, g.b, g.c, g.lo, g.hi, x, y );
  return VVHIP_OK;
}

int vvhip_interp_chroma_batch( vvhip_ctx* ctx, const int16_t* d_ref, int ref_stride, const vvhip_subpel_item* d_items, int n,
                               int width, int height, int bit_depth, int rnd_res, int16_t* d_out )
{
  if( !ctx ) return VVHIP_E_ARG;
  if( !isPow2( width ) || !isPow2( height ) || width < 2 || height < 2 || width > 64 || height > 64 || bit_depth < 8 || bit_depth > 12 || n < 0 || ref_stride < 2 || ( ref_stride & 1 ) ||
      ( n && ( !d_ref || !d_items || !d_out ) ) )
    return vvhip_fail( ctx, VVHIP_E_ARG, "vvhip_interp_chroma_batch: block %dx%d (powers of two, 2..64) bitDepth %d stride %d (even)", width, height, bit_depth, ref_stride );
  if( n == 0 ) return VVHIP_OK;
  const TileShape ts = tileShape( width, height, true );
  const int subsPerWave = 64 >> ts.log2Lanes, ldsPerWave = subsPerWave * subElems( ts.tw, ts.th, 4 );
  const long long tiles = ( long long ) n * ( width / ts.tw ) * ( height / ts.th ), waves = ( tiles + subsPerWave - 1 ) / subsPerWave;
  hipLaunchKernelGGL( predOneSizeKernel, dim3( ( unsigned ) ( ( waves + 3 ) / 4 ) ), dim3( 256 ), ( size_t ) ldsPerWave * 4 * sizeof( int16_t ), ctx->stream, d_ref, ref_stride, d_items, n,
                      width, height, bit_depth, rnd_res ? 1 : 0, ts.kind, ts.tw, ts.th, ts.log2SegsRow, ts.log2Lanes, ldsPerWave, d_out );
  VVHIP_LAUNCH_CHECK( ctx );
  return VVHIP_OK;
}

} // extern "C"
