// intrachroma.hip — intra chroma mode pre-selection of a list of 4:2:0 blocks (gfx950): predict Cb and Cr of up to eight candidate modes of a block — regular modes from the
// components' reference lines, CCLM / MDLM from the reconstructed luma — and score each against its original with min( 2 * SAD, HAD ), in the kernel that makes the prediction.
//
// Restates, per requested slot, the arithmetic of IntraSearch::estIntraPredChromaQT's decision-free loop (EncoderLib/IntraSearch.cpp:778-862):
//   IntraPrediction::initPredIntraParams   CommonLib/IntraPrediction.cpp:409-496   (a chroma block: no reference filter, no interpolation flag; getWideAngle :335-351)
//   predIntraAng                           :353-383                                 (xPredIntraPlanar_Core :79-135, xGetPredValDc :302-333, IntraPredSampleFilter_Core :137-157)
//   xPredIntraAng                          :518-681                                 (IntraHorVerPDPC_Core :159-175, IntraAnglePDPC_Core :176-189, IntraPredAngleChroma_Core :225-245)
//   loadLMLumaRecPels                      :1165-1406                               (4:2:0: isFirstRowOfCtu, verCollocatedChroma, the six-tap, leftPadding, abovePadding)
//   xGetLMParameters                       :1408-1605
//   predIntraChromaLM, linearTransform     :385-397, Buffer.cpp:253
//   RdCost::xGetSAD, xGetHADs<false>       (tiles and normalisations: hadtile.h)
//
// One workgroup of ONE wave per item: a chroma item is at most 16 predictions of at most 1024 samples and most are 4x4 .. 8x8 — 16 lanes' to two waves' worth of slots — so a
// larger group would idle, and with one wave the group's barriers cost nothing.  Both components' lines and originals, the down-sampled luma block (only when a mode >= 67 is
// requested), one record per requested slot and ( a, b, shift ) per LM slot and component live in LDS (7 144 bytes, 7.1 KB: 22 groups per CU).  As in intra.hip a sample is a function of
// ( mode, x, y ), so the lanes are laid out for the Hadamard teams: a slot is ( candidate, component, tile, team lane ), a lane forms the 8 samples its team position
// transforms (16 for the 4x4 block), subtracts them from the original in LDS and the team scores the tile.  The LM parameters read four template positions per mode and
// component: one lane per ( slot, component ) down-samples those four positions straight from HBM, so the template is never formed.  Tile sums and SADs are added per
// ( slot, component ) with integer LDS atomics (they commute); a prediction reaches HBM only for pred_mask bits.
#include <string.h>
#include "common.h"
#include "hadtile.h"

namespace {

constexpr int IC_THREADS = 64, IC_SLOTS = 8, IC_LINE = 72;          // a line: 2 * 32 + 1 samples, rounded up
constexpr int C_VER = 1, C_PDPC = 2, C_PRED = 4, C_LM = 8;

struct IchMode { int16_t angle, inv; uint8_t mode, flags; int8_t scale; uint8_t predRank, slot, rsv[3]; };
static_assert( sizeof( IchMode ) == 12, "IchMode layout" );

struct IchLds
{
  int16_t  line[2][2][IC_LINE];          // [component][0 top row, 1 left row], each from the corner
  int16_t  org[2][32 * 32];
  int16_t  ds[32 * 32];                  // the down-sampled luma block
  IchMode  mp[IC_SLOTS];                 // by rank among the requested slots
  int32_t  lm[IC_SLOTS][2][3];           // ( a, b, shift ) by rank and component
  uint32_t acc[IC_SLOTS][2][2];          // by rank and component: Hadamard sum, SAD
  int      dc[2];
};

__device__ const int16_t kIchAng[32]    = { 0, 1, 2, 3, 4, 6, 8, 10, 12, 14, 16, 18, 20, 23, 26, 29, 32, 35, 39, 45, 51, 57, 64, 73, 86, 102, 128, 171, 256, 341, 512, 1024 };
__device__ const int16_t kIchInvAng[32] = { 0, 16384, 8192, 5461, 4096, 2731, 2048, 1638, 1365, 1170, 1024, 910, 819, 712, 630, 565, 512, 468, 420, 364, 321, 287, 256, 224, 191, 161, 128, 96, 64, 48, 32, 16 };
__device__ const uint8_t kIchModeShift[6] = { 0, 6, 10, 12, 14, 15 };
__device__ const uint8_t kDivSig[16]      = { 0, 7, 6, 5, 5, 4, 4, 3, 3, 2, 2, 1, 1, 1, 1, 0 };      // DivSigTable: 4-bit significands - 8

__device__ __forceinline__ int flog2( int v ) { return 31 - __builtin_clz( v ); }
__device__ __forceinline__ int clipS( int v, int vmax ) { return min( max( v, 0 ), vmax ); }

// initPredIntraParams for regular mode `mode` of a w x h chroma block (sides >= 4: applyPDPC starts out true)
__device__ __forceinline__ IchMode ichParams( int w, int h, int mode )
{
  IchMode p; p.angle = 0; p.inv = 0; p.mode = ( uint8_t ) mode; p.flags = 0; p.scale = -1; p.predRank = 0; p.slot = 0; p.rsv[0] = p.rsv[1] = p.rsv[2] = 0;
  int predMode = mode;
  if( mode > 1 )                                                                         // getWideAngle
  {
    const int ds = kIchModeShift[abs( flog2( w ) - flog2( h ) )];
    if( w > h && mode < 2 + ds )       predMode += 65;
    else if( h > w && mode > 66 - ds ) predMode -= 65;
  }
  const bool ver = predMode >= 34;
  bool pdpc = true;
  if( mode > 1 )
  {
    const int am = ver ? predMode - 50 : -( predMode - 18 ), aam = abs( am ), absAng = kIchAng[aam];
    p.inv = kIchInvAng[aam];
    p.angle = ( int16_t ) ( am < 0 ? -absAng : absAng );
    if( am < 0 ) pdpc = false;
    else if( am > 0 )
    {
      const int sc = min( 2, flog2( ver ? h : w ) - ( flog2( 3 * p.inv - 2 ) - 8 ) );
      p.scale = ( int8_t ) sc;
      pdpc = sc >= 0;
    }
    else p.scale = ( int8_t ) ( ( flog2( w ) + flog2( h ) - 2 ) >> 2 );                  // pure horizontal / vertical: the scale IntraHorVerPDPC is called with
  }
  p.flags = ( uint8_t ) ( ( ver ? C_VER : 0 ) | ( pdpc ? C_PDPC : 0 ) );
  return p;
}

struct IchGeo { int w, h, lw, lh, vmax; };

// IntraPredSampleFilter_Core on one sample
__device__ __forceinline__ int sampleFilter( int v, int top, int left, int x, int y, int scale )
{
  const int wT = 32 >> min( 31, ( y << 1 ) >> scale ), wL = 32 >> min( 31, ( x << 1 ) >> scale );
  return v + ( ( wL * ( left - v ) + wT * ( top - v ) + 32 ) >> 6 );
}

// sample ( x, y ) of the prediction of record p (rank r) for component c
__device__ __forceinline__ int ichSample( const IchLds& L, const IchGeo& g, const IchMode p, int r, int c, int x, int y )
{
  if( p.flags & C_LM )
    return clipS( ( ( L.lm[r][c][0] * ( int ) L.ds[y * g.w + x] ) >> L.lm[r][c][2] ) + L.lm[r][c][1], g.vmax );
  const int16_t* top  = L.line[c][0];
  const int16_t* left = L.line[c][1];
  if( p.mode == 0 )
  {
    const int t = top[1 + x], l = left[1 + y], tr = top[g.w + 1], bl = left[g.h + 1];
    const int hor = ( l << g.lw ) + ( x + 1 ) * ( tr - l ), ver = ( t << g.lh ) + ( y + 1 ) * ( bl - t );
    const int v = ( ( hor << g.lh ) + ( ver << g.lw ) + ( 1 << ( g.lw + g.lh ) ) ) >> ( 1 + g.lw + g.lh );
    return sampleFilter( v, t, l, x, y, ( g.lw + g.lh - 2 ) >> 2 );
  }
  if( p.mode == 1 ) return sampleFilter( L.dc[c], top[1 + x], left[1 + y], x, y, ( g.lw + g.lh - 2 ) >> 2 );
  const bool ver = p.flags & C_VER;
  const int xx = ver ? x : y, yy = ver ? y : x, W = ver ? g.w : g.h, H = ver ? g.h : g.w;      // the block as the main direction sees it
  const int16_t* mainL = ver ? top : left;
  const int16_t* sideL = ver ? left : top;
  const int angle = p.angle, inv = p.inv;
  // refMain[i]: below 0 the projected side samples (:545-550), beyond 2W the last sample (:563-572)
  auto M = [&]( int i ) -> int { return i < 0 ? ( int ) sideL[min( ( -i * inv + 256 ) >> 9, H )] : ( int ) mainL[min( i, 2 * W )]; };
  auto S = [&]( int j ) -> int { return sideL[min( j, 2 * H )]; };
  int v;
  if( angle == 0 )
  {
    v = M( 1 + xx );
    if( xx < min( 3 << p.scale, W ) ) v = clipS( v + ( ( ( 32 >> ( ( 2 * xx ) >> p.scale ) ) * ( S( 1 + yy ) - M( 0 ) ) + 32 ) >> 6 ), g.vmax );
    return v;
  }
  const int dpos = angle * ( 1 + yy ), dint = dpos >> 5, fr = dpos & 31;
  if( ( abs( angle ) & 31 ) == 0 ) v = M( dint + 1 + xx );
  else v = ( ( 32 - fr ) * M( dint + 1 + xx ) + fr * M( dint + 2 + xx ) + 16 ) >> 5;      // IntraPredAngleChroma_Core
  if( ( p.flags & C_PDPC ) && xx < min( 3 << p.scale, W ) )
  {
    const int lft = S( yy + ( ( 256 + inv * ( xx + 1 ) ) >> 9 ) + 1 );
    v += ( ( 32 >> ( ( 2 * xx ) >> p.scale ) ) * ( lft - v ) + 32 ) >> 6;
  }
  return v;
}

// ---- loadLMLumaRecPels, one position at a time.  P: the luma plane at the area's top-left sample, s its pitch -------------------------------------------
__device__ __forceinline__ int dsInner( const int16_t* P, ptrdiff_t s, int flags, int i, int j )
{
  const int lp = ( i == 0 && !( flags & VVHIP_ICH_LEFT ) ) ? 0 : 1;
  const int16_t* q = P + ( ptrdiff_t ) ( 2 * j ) * s + 2 * i;
  if( flags & VVHIP_ICH_VER_COLLOCATED )
  {
    const int ap = ( j == 0 && !( flags & VVHIP_ICH_ABOVE ) ) ? 0 : 1;
    return ( q[-ap * s] + 4 * q[0] + q[-lp] + q[1] + q[s] + 4 ) >> 3;
  }
  return ( 2 * q[0] + q[1] + q[-lp] + 2 * q[s] + q[s + 1] + q[s - lp] + 4 ) >> 3;
}
__device__ __forceinline__ int dsAbove( const int16_t* P, ptrdiff_t s, int flags, int i )
{
  const int lp = ( i == 0 && !( flags & VVHIP_ICH_LEFT ) ) ? 0 : 1;
  if( flags & VVHIP_ICH_FIRST_ROW ) { const int16_t* q = P - s + 2 * i; return ( 2 * q[0] + q[-lp] + q[1] + 2 ) >> 2; }
  const int16_t* q = P - 2 * s + 2 * i;
  if( flags & VVHIP_ICH_VER_COLLOCATED ) return ( q[-s] + 4 * q[0] + q[-lp] + q[1] + q[s] + 4 ) >> 3;
  return ( 2 * q[0] + q[1] + q[-lp] + 2 * q[s] + q[s + 1] + q[s - lp] + 4 ) >> 3;
}
__device__ __forceinline__ int dsLeft( const int16_t* P, ptrdiff_t s, int flags, int j )
{
  const int16_t* q = P + ( ptrdiff_t ) ( 2 * j ) * s - 2;
  if( flags & VVHIP_ICH_VER_COLLOCATED )
  {
    const int ap = ( j == 0 && !( flags & VVHIP_ICH_ABOVE ) ) ? 0 : 1;
    return ( q[-ap * s] + 4 * q[0] + q[-1] + q[1] + q[s] + 4 ) >> 3;
  }
  return ( 2 * q[0] + q[1] + q[-1] + 2 * q[s] + q[s + 1] + q[s - 1] + 4 ) >> 3;
}

// xGetLMParameters for mode 67..69 and one component (top / left: its lines in LDS) -> out = ( a, b, shift )
__device__ __forceinline__ void lmParams( const int16_t* P, ptrdiff_t s, const int16_t* top, const int16_t* left, int w, int h, int bitDepth, int flags, int nAR, int nLB, int mode, int32_t* out )
{
  bool above = flags & VVHIP_ICH_ABOVE, lft = flags & VVHIP_ICH_LEFT;
  int topN = 0, leftN = 0;
  if( mode == 69 )      { lft = false;   topN  = above ? w + min( nAR, h ) : 0; }        // MDLM_T (:1484-1489)
  else if( mode == 68 ) { above = false; leftN = lft ? h + min( nLB, w ) : 0; }           // MDLM_L (:1490-1495)
  else                  { topN = w; leftN = h; }
  if( !above && !lft ) { out[0] = 0; out[1] = 1 << ( bitDepth - 1 ); out[2] = 0; return; }
  const int aboveIs4 = lft ? 0 : 1, leftIs4 = above ? 0 : 1;
  const int start0 = topN >> ( 2 + aboveIs4 ), step0 = max( 1, topN >> ( 1 + aboveIs4 ) ), start1 = leftN >> ( 2 + leftIs4 ), step1 = max( 1, leftN >> ( 1 + leftIs4 ) );
  const int cntT = above ? ( ( 1 + aboveIs4 ) << 1 ) : 0;                                  // (sides >= 4: the templates hold at least 4 samples, cntT + cntL == 4)
  int l0, l1, l2, l3, c0, c1, c2, c3;
  auto pick = [&]( int k, int& l, int& c )
  {
    if( k < cntT ) { const int pos = start0 + k * step0;            l = dsAbove( P, s, flags, pos ); c = top[1 + pos]; }
    else           { const int pos = start1 + ( k - cntT ) * step1; l = dsLeft( P, s, flags, pos );  c = left[1 + pos]; }
  };
  pick( 0, l0, c0 ); pick( 1, l1, c1 ); pick( 2, l2, c2 ); pick( 3, l3, c3 );
  auto SL = [&]( int i ) { return i == 0 ? l0 : ( i == 1 ? l1 : ( i == 2 ? l2 : l3 ) ); };
  auto SC = [&]( int i ) { return i == 0 ? c0 : ( i == 1 ? c1 : ( i == 2 ? c2 : c3 ) ); };
  int mn0 = 0, mn1 = 2, mx0 = 1, mx1 = 3, t;
  if( SL( mn0 ) > SL( mn1 ) ) { t = mn0; mn0 = mn1; mn1 = t; }
  if( SL( mx0 ) > SL( mx1 ) ) { t = mx0; mx0 = mx1; mx1 = t; }
  if( SL( mn0 ) > SL( mx1 ) ) { t = mn0; mn0 = mx0; mx0 = t; t = mn1; mn1 = mx1; mx1 = t; }      // the two groups change places
  if( SL( mn1 ) > SL( mx0 ) ) { t = mn1; mn1 = mx0; mx0 = t; }
  const int minL = ( SL( mn0 ) + SL( mn1 ) + 1 ) >> 1, minC = ( SC( mn0 ) + SC( mn1 ) + 1 ) >> 1;
  const int maxL = ( SL( mx0 ) + SL( mx1 ) + 1 ) >> 1, maxC = ( SC( mx0 ) + SC( mx1 ) + 1 ) >> 1;
  const int diff = maxL - minL;
  if( diff <= 0 ) { out[0] = 0; out[1] = minC; out[2] = 0; return; }
  const int diffC = maxC - minC;
  int x = flog2( diff );
  const int normDiff = ( ( diff << 4 ) >> x ) & 15, v = kDivSig[normDiff] | 8;
  x += normDiff != 0;
  const int y = diffC == 0 ? 0 : flog2( abs( diffC ) ) + 1, add = ( 1 << y ) >> 1;
  int a = ( diffC * v + add ) >> y, sh = 3 + x - y;
  if( sh < 1 ) { sh = 1; a = a == 0 ? 0 : ( a < 0 ? -15 : 15 ); }
  out[0] = a; out[1] = minC - ( ( a * minL ) >> sh ); out[2] = sh;
}

__global__ void __launch_bounds__( IC_THREADS )
intraChromaModesKernel( const vvhip_intra_chroma_item* __restrict__ items, const int16_t* __restrict__ luma, const int16_t* __restrict__ ref, const int16_t* __restrict__ org,
                        int16_t* __restrict__ pred, uint32_t* __restrict__ cost )
{
  __shared__ IchLds L;
  const int tid = threadIdx.x, lane = tid & 63;
  const vvhip_intra_chroma_item* itp = items + blockIdx.x;
  const int w = itp->w, h = itp->h, flags = itp->flags, modeMask = itp->mode_mask, predMask = itp->pred_mask;
  IchGeo g; g.w = w; g.h = h; g.lw = flog2( w ); g.lh = flog2( h ); g.vmax = ( 1 << itp->bit_depth ) - 1;
  const int nt = 2 * w + 1, nl = 2 * h + 1, nSamples = w * h;
  const int nModes = __builtin_popcount( modeMask );
  if( nModes == 0 ) return;
  bool anyLm = false;
#pragma unroll
  for( int s = 0; s < IC_SLOTS; s++ ) anyLm = anyLm || ( ( ( modeMask >> s ) & 1 ) && itp->cand[s] >= 67 );
  const int16_t* P = anyLm ? luma + ( ptrdiff_t ) itp->luma_off : nullptr;                // (d_luma may be NULL without a requested mode >= 67)
  const ptrdiff_t ls = itp->luma_stride;
  const int refOff[2] = { itp->ref_off[0], itp->ref_off[1] }, orgOff[2] = { itp->org_off[0], itp->org_off[1] };      // (the record's fields are read once, not per trip)

  // ---- the lines, the originals, the down-sampled block ----
  for( int i = tid; i < 2 * ( nt + nl ); i += IC_THREADS )
  {
    const int c = i >= nt + nl, k = c ? i - ( nt + nl ) : i;
    const int16_t v = ref[( size_t ) ( c ? refOff[1] : refOff[0] ) + k];
    if( k < nt ) L.line[c][0][k] = v; else L.line[c][1][k - nt] = v;
  }
  for( int i = tid; i < 2 * nSamples; i += IC_THREADS )
  {
    const int c = i >= nSamples, k = c ? i - nSamples : i;
    L.org[c][k] = org[( size_t ) ( c ? orgOff[1] : orgOff[0] ) + k];
  }
  if( anyLm )
    for( int i = tid; i < nSamples; i += IC_THREADS ) L.ds[i] = ( int16_t ) dsInner( P, ls, flags, i & ( w - 1 ), i >> g.lw );
  if( tid < IC_SLOTS * 4 ) ( &L.acc[0][0][0] )[tid] = 0;
  __syncthreads();

  // ---- once per item: the DC values, the slot records, the LM parameters ----
#pragma unroll
  for( int c = 0; c < 2; c++ )                                                            // xGetPredValDc
  {
    uint32_t s = 0;
    for( int i = lane; i < w + h; i += 64 )
    {
      const bool inTop = i < w;
      if( inTop ? w >= h : w <= h ) s += ( uint32_t ) L.line[c][inTop ? 0 : 1][1 + ( inTop ? i : i - w )];
    }
    s = vvhipGroupSum32( s, 64, lane );
    const int den = w == h ? 2 * w : max( w, h );
    if( lane == 0 ) L.dc[c] = ( int ) ( ( s + ( den >> 1 ) ) >> flog2( den ) );
  }
  if( tid < IC_SLOTS && ( ( modeMask >> tid ) & 1 ) )
  {
    const int below = ( 1 << tid ) - 1, mode = itp->cand[tid];
    IchMode p = ichParams( w, h, mode < 67 ? mode : 0 );
    p.mode = ( uint8_t ) mode;
    if( mode >= 67 ) p.flags = C_LM;
    if( ( predMask >> tid ) & 1 ) p.flags |= C_PRED;
    p.predRank = ( uint8_t ) __builtin_popcount( predMask & below );
    p.slot = ( uint8_t ) tid;
    L.mp[__builtin_popcount( modeMask & below )] = p;
  }
  else if( tid >= 32 && tid < 32 + 2 * IC_SLOTS )                                         // one lane per ( slot, component ) of the LM slots
  {
    const int s = ( tid - 32 ) >> 1, c = tid & 1, mode = itp->cand[s];
    if( ( ( modeMask >> s ) & 1 ) && mode >= 67 )
      lmParams( P, ls, L.line[c][0], L.line[c][1], w, h, itp->bit_depth, flags, itp->n_above_right, itp->n_left_below, mode, L.lm[__builtin_popcount( modeMask & ( ( 1 << s ) - 1 ) )][c] );
  }
  __syncthreads();

  // ---- the slots: ( rank, component ) pairs, rank-major ----
  const int kind = hadTileKind( w, h, false ), nPreds = 2 * nModes;
  const int predOff[2] = { itp->pred_off[0], itp->pred_off[1] };
  if( kind == TK_4x4 )                                                                   // (only the 4x4 block) one lane per prediction
  {
    if( tid < nPreds )
    {
      const int r = tid >> 1, c = tid & 1;
      const IchMode p = L.mp[r];
      int16_t* out = ( p.flags & C_PRED ) ? pred + ( size_t ) ( c ? predOff[1] : predOff[0] ) + p.predRank * 16 : nullptr;      // (d_pred may be NULL without a pred_mask bit)
      int d[16]; uint32_t sad = 0;
#pragma unroll
      for( int i = 0; i < 16; i++ )
      {
        const int v = ichSample( L, g, p, r, c, i & 3, i >> 2 );
        if( p.flags & C_PRED ) out[i] = ( int16_t ) v;
        d[i] = L.org[c][i] - v;
        sad += ( uint32_t ) abs( d[i] );
      }
      L.acc[r][c][0] = hadamard4x4( d ); L.acc[r][c][1] = sad;
    }
  }
  else
  {
    const int PW = tileW( kind ), PH = tileH( kind ), LT = tileLanes( kind ), log2LT = flog2( LT );
    const int log2TX = g.lw - flog2( PW ), log2Slots = g.lw + g.lh - 3, slots = 1 << log2Slots, total = nPreds << log2Slots;
    for( int s0 = 0; s0 < total; s0 += IC_THREADS )
    {
      const int sl = s0 + tid;
      const bool valid = sl < total;                                                     // (teams are whole: total is a multiple of the team size)
      const int sv = valid ? sl : 0, pi = sv >> log2Slots, r = pi >> 1, c = pi & 1, rem = sv & ( slots - 1 ), t = rem >> log2LT, q = rem & ( LT - 1 );
      const IchMode p = L.mp[r];
      const int tx = ( t & ( ( 1 << log2TX ) - 1 ) ) * PW, ty = ( t >> log2TX ) * PH;
      // the lane's 8 samples (table in front of hadTeam, hadtile.h): a row of 8, or rows 2q and 2q + 1 of a 4x8 tile
      const int x0 = tx + ( kind == TK_16x8 ? 8 * ( q >> 3 ) : 0 ), y0 = ty + ( kind == TK_16x8 ? ( q & 7 ) : ( kind == TK_4x8 ? 2 * q : q ) );
      int16_t* out = ( p.flags & C_PRED ) ? pred + ( size_t ) ( c ? predOff[1] : predOff[0] ) + ( size_t ) p.predRank * nSamples : nullptr;
      int d[8]; uint32_t sad = 0;
#pragma unroll
      for( int i = 0; i < 8; i++ )
      {
        const int x = x0 + ( kind == TK_4x8 ? ( i & 3 ) : i ), y = y0 + ( kind == TK_4x8 ? ( i >> 2 ) : 0 );
        const int v = ichSample( L, g, p, r, c, x, y );
        if( valid && ( p.flags & C_PRED ) ) out[y * w + x] = ( int16_t ) v;
        d[i] = L.org[c][y * w + x] - v;
        sad += ( uint32_t ) abs( d[i] );
      }
      const uint32_t sres = hadTeam( d, q, LT, kind, lane );
      sad = vvhipGroupSum32( sad, LT, lane );
      if( valid && q == 0 ) { atomicAdd( &L.acc[r][c][0], sres ); atomicAdd( &L.acc[r][c][1], sad ); }
    }
  }
  __syncthreads();
  if( tid < nModes )
    cost[( size_t ) itp->cost_off + L.mp[tid].slot] = min( L.acc[tid][0][0], 2 * L.acc[tid][0][1] ) + min( L.acc[tid][1][0], 2 * L.acc[tid][1][1] );
}

} // namespace

extern "C" {

int vvhip_intra_chroma_modes_batch( vvhip_ctx* ctx, const vvhip_intra_chroma_item* items_host, int n, const int16_t* d_luma, const int16_t* d_ref, const int16_t* d_org,
                                    int16_t* d_pred, uint32_t* d_cost )
{
  if( !ctx ) return VVHIP_E_ARG;
  if( n < 0 || ( n > 0 && ( !items_host || !d_ref || !d_org || !d_cost ) ) )
    return vvhip_fail( ctx, VVHIP_E_ARG, "vvhip_intra_chroma_modes_batch: %d items (>= 0), items / d_ref / d_org / d_cost missing", n );
  for( int i = 0; i < n; i++ )
  {
    const vvhip_intra_chroma_item& q = items_host[i];
    auto sizeOk = []( int v ) { return v == 4 || v == 8 || v == 16 || v == 32; };
    if( !sizeOk( q.w ) || !sizeOk( q.h ) ) return vvhip_fail( ctx, VVHIP_E_ARG, "vvhip_intra_chroma_modes_batch: item %d: %dx%d (chroma sides of 4, 8, 16, 32)", i, q.w, q.h );
    if( q.bit_depth < 8 || q.bit_depth > 12 ) return vvhip_fail( ctx, VVHIP_E_ARG, "vvhip_intra_chroma_modes_batch: item %d: bit depth %d (8..12)", i, q.bit_depth );
    if( q.flags & ~( VVHIP_ICH_ABOVE | VVHIP_ICH_LEFT | VVHIP_ICH_FIRST_ROW | VVHIP_ICH_VER_COLLOCATED ) )
      return vvhip_fail( ctx, VVHIP_E_ARG, "vvhip_intra_chroma_modes_batch: item %d: unknown flag bits 0x%x", i, q.flags );
    bool lm = false;
    for( int s = 0; s < 8; s++ )
    {
      if( q.cand[s] > 69 ) return vvhip_fail( ctx, VVHIP_E_ARG, "vvhip_intra_chroma_modes_batch: item %d: candidate %d is mode %d (0..69)", i, s, q.cand[s] );
      lm = lm || ( ( ( q.mode_mask >> s ) & 1 ) && q.cand[s] >= 67 );
    }
    if( ( q.n_above_right & 1 ) || ( q.n_left_below & 1 ) ) return vvhip_fail( ctx, VVHIP_E_ARG, "vvhip_intra_chroma_modes_batch: item %d: odd template counts (%d above right, %d left below)", i, q.n_above_right, q.n_left_below );
    if( q.w + q.n_above_right > 2 * q.w || q.h + q.n_left_below > 2 * q.h )
      return vvhip_fail( ctx, VVHIP_E_ARG, "vvhip_intra_chroma_modes_batch: item %d: a template beyond 2w / 2h (%d above right of %d, %d left below of %d)", i, q.n_above_right, q.w, q.n_left_below, q.h );
    if( ( q.n_above_right && !( q.flags & VVHIP_ICH_ABOVE ) ) || ( q.n_left_below && !( q.flags & VVHIP_ICH_LEFT ) ) )
      return vvhip_fail( ctx, VVHIP_E_ARG, "vvhip_intra_chroma_modes_batch: item %d: an above-right / left-below count without its side (flags 0x%x)", i, q.flags );
    if( q.pred_mask & ~q.mode_mask ) return vvhip_fail( ctx, VVHIP_E_ARG, "vvhip_intra_chroma_modes_batch: item %d: pred_mask is not a subset of mode_mask", i );
    if( q.luma_off < 0 || q.luma_stride < 0 || q.ref_off[0] < 0 || q.ref_off[1] < 0 || q.org_off[0] < 0 || q.org_off[1] < 0 || q.pred_off[0] < 0 || q.pred_off[1] < 0 || q.cost_off < 0 )
      return vvhip_fail( ctx, VVHIP_E_ARG, "vvhip_intra_chroma_modes_batch: item %d: a negative offset or luma_stride", i );
    for( int k = 0; k < 12; k++ ) if( q.rsv[k] ) return vvhip_fail( ctx, VVHIP_E_ARG, "vvhip_intra_chroma_modes_batch: item %d: reserved bytes are not zero", i );
    if( lm && !d_luma ) return vvhip_fail( ctx, VVHIP_E_ARG, "vvhip_intra_chroma_modes_batch: item %d asks for a mode >= 67, d_luma is missing", i );
    if( q.pred_mask && !d_pred ) return vvhip_fail( ctx, VVHIP_E_ARG, "vvhip_intra_chroma_modes_batch: item %d asks for predictions, d_pred is missing", i );
  }
  if( n == 0 ) return VVHIP_OK;
  HostList& S = ctx->list[LIST_INTRA_CHROMA];
  const int rc = listUpload( ctx, S, ListBlob( items_host, ( size_t ) n * sizeof( vvhip_intra_chroma_item ) ) );
  if( rc != VVHIP_OK ) return rc;
  hipLaunchKernelGGL( intraChromaModesKernel, dim3( ( unsigned ) n ), dim3( IC_THREADS ), 0, ctx->stream, ( const vvhip_intra_chroma_item* ) S.d, d_luma, d_ref, d_org, d_pred, d_cost );
  VVHIP_LAUNCH_CHECK( ctx );
  return listLaunched( ctx, S );
}

} // extern "C"
