// deblock.hip — the deblocking filter of a picture: vvhip_deblock (gfx950 only).
//
// The loop filter (LF) is the first stage of the in-loop chain CTU_ENCODE -> LF -> SAO -> ALF.  Once calcFilterStrengths (CommonLib/LoopFilter.cpp:552-1271) has folded
// CUs, TUs and motion into the two maps of LoopFilterParam records, LoopFilter::xDeblockArea<dir> (:405-462) is pure sample arithmetic:
//   luma   : xEdgeFilterLuma (:1372-1520) — the long filters of xFilteringPandQCore (:123-201), else xPelFilterLumaCorePel (:217-264), decided per 4-sample edge segment
//   chroma : xEdgeFilterChroma (:1522-1635), 4:2:0 — xPelFilterChroma (:284-342), decided per 2-sample segment on the 8-sample chroma grid of a CTU
// and the standard guarantees that, on maps calcFilterStrengths leaves, no edge of a direction writes a sample another edge of that direction reads or writes: all edge
// segments of a direction are independent, and only the order "all vertical edges, then all horizontal edges" matters.  That order is TWO launches on one stream, not
// one fused kernel: a horizontal edge at the top of a CTU reads four rows of the CTU above after ITS vertical edges, so a fused kernel would have to filter the vertical
// edges of those halo rows a second time in every workgroup (and of the halo's own 8-column margin), while a second launch costs a few microseconds once per band.
//
// One workgroup of four waves per ( CTU, plane ) and direction.  The CTU and the 8 samples an edge can reach beyond it across the direction (left / right for vertical
// edges, above / below for horizontal ones) go to LDS once, with 8-byte loads where base and pitch allow: vertical edges walk ACROSS rows, which from global memory
// would be strided 2-byte accesses.  A lane takes one edge segment: it reads its lines from the tile, decides, filters in place in the tile and marks every sample it
// writes in a byte mask beside the tile.  The tile is then written back row by row — only marked samples, and only inside the picture: samples in the margins belong to
// the neighbouring workgroups' edges and must not be overwritten with stale values.  Which lane of which workgroup runs first is free (legal maps), so every run gives
// the same bits.  Reads of samples a decision does not use (the reference loads whole 8-sample lines too) may race with another segment's store; they feed nothing.
// Integer arithmetic only, no atomics, no scratch.
#include "common.h"
#include <algorithm>
#include <string.h>
#include <vector>

namespace {

constexpr int DBK_THREADS = 256;
constexpr int DBK_MARGIN = 8;      // samples an edge reaches across its direction: 8 on the P side (p7 of a long filter), 8 on the Q side

struct DbkPlaneDev { int16_t* p; int stride, width, height, clipMin, clipMax, betaOff, tcOff; };
struct DbkRec      { int8_t qp[3]; uint8_t bs, len, flags, pad[2]; };      // vvhip_lf_param widened to one 8-byte load
struct DbkArgs     { DbkPlaneDev pl[3]; const uint2* recs;      // a DbkRec as two dwords: x = qp[0] | qp[1] << 8 | qp[2] << 16 | bs << 24, y = len | flags << 8
                     int mapW, unitRow0, ctusX, ctuRow0, ctu, bitDepth, nPlanes; };

struct __attribute__( ( aligned( 8 ) ) ) DbkSeg4 { int16_t v[4]; };

// LoopFilter::sm_tcTable / sm_betaTable (CommonLib/LoopFilter.cpp:79-87)
__device__ const uint16_t dbkTcTable[66] = { 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 3, 4, 4, 4, 4, 5, 5, 5, 5, 7, 7, 8, 9, 10, 10, 11, 13, 14, 15, 17, 19, 21, 24, 25, 29, 33, 36, 41, 45, 51, 57,
                                             64, 71, 80, 89, 100, 112, 125, 141, 157, 177, 198, 222, 250, 280, 314, 352, 395 };
__device__ const uint8_t dbkBetaTable[64] = { 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 17, 18, 20, 22, 24, 26, 28, 30, 32, 34, 36, 38, 40, 42, 44, 46, 48, 50,
                                              52, 54, 56, 58, 60, 62, 64, 66, 68, 70, 72, 74, 76, 78, 80, 82, 84, 86, 88 };

__device__ __forceinline__ int dbkClip3( int lo, int hi, int v ) { return min( max( v, lo ), hi ); }
__device__ __forceinline__ int dbkTc( int qp, int bs, int tcOff, int bd )
{
  const int t = dbkTcTable[dbkClip3( 0, 65, qp + 2 * ( bs - 1 ) + 2 * tcOff )];
  return bd < 10 ? ( t + ( 1 << ( 9 - bd ) ) ) >> ( 10 - bd ) : t << ( bd - 10 );
}
__device__ __forceinline__ int dbkBeta( int qp, int betaOff, int bd ) { return ( int ) dbkBetaTable[dbkClip3( 0, 63, qp + 2 * betaOff )] << ( bd - 8 ); }

// a line of samples across an edge: v[8 + k] is the sample at offset k from the edge (k < 0: the P side).  Indexed with constants only: it lives in registers
struct DbkLine { int v[16]; };

template<int FIRST, int LAST>
__device__ __forceinline__ void dbkLoadLine( DbkLine& s, const int16_t* __restrict__ t, int off )
{
#pragma unroll
  for( int k = FIRST; k <= LAST; k++ ) s.v[8 + k] = t[k * off];
}

// xUseStrongFiltering (:1318-1370)
__device__ __forceinline__ bool dbkUseStrong( const DbkLine& s, int d, int beta, int tc, bool pL, bool qL, int lp, int lq, bool ctb )
{
  const int m3 = s.v[7], m4 = s.v[8];
  const bool large = pL || qL;
  if( !( d < ( beta >> ( large ? 4 : 2 ) ) && abs( m3 - m4 ) < ( ( tc * 5 + 1 ) >> 1 ) ) ) return false;
  const int m0 = s.v[4], m7 = s.v[11];
  int sp3 = ctb ? abs( s.v[6] - m3 ) : abs( m0 - m3 ), sq3 = abs( m7 - m4 );
  if( large )
  {
    if( pL )
    {
      const int mP4 = lp == 7 ? s.v[0] : s.v[2];
      if( lp == 7 ) sp3 += abs( s.v[3] - s.v[2] - s.v[1] + mP4 );
      sp3 = ( sp3 + abs( m0 - mP4 ) + 1 ) >> 1;
    }
    if( qL )
    {
      const int m11 = lq == 7 ? s.v[15] : s.v[13];
      if( lq == 7 ) sq3 += abs( s.v[12] - s.v[13] - s.v[14] + m11 );
      sq3 = ( sq3 + abs( m11 - m7 ) + 1 ) >> 1;
    }
    return sp3 + sq3 < ( beta * 3 >> 5 );
  }
  return sp3 + sq3 < ( beta >> 3 );
}

// a store into the tile, marked for the write-back
#define DBK_PUT( k, val ) do { t[( k ) * off] = ( int16_t ) ( val ); mk[( k ) * off] = 1; } while( 0 )

// xFilteringPandQCore + xBilinearFilter (:100-201) for one line; nP, nQ in { 3, 5, 7 }, not both 3
__device__ __forceinline__ void dbkLongLine( int16_t* __restrict__ t, uint8_t* __restrict__ mk, int off, int nP, int nQ, int tc )
{
  DbkLine s;
  dbkLoadLine<-8, 7>( s, t, off );
  int P[8], Q[8];
#pragma unroll
  for( int j = 0; j < 8; j++ ) { P[j] = s.v[7 - j]; Q[j] = s.v[8 + j]; }
  const int refP = ( ( nP == 7 ? P[6] + P[7] : nP == 5 ? P[4] + P[5] : P[2] + P[3] ) + 1 ) >> 1;
  const int refQ = ( ( nQ == 7 ? Q[6] + Q[7] : nQ == 5 ? Q[4] + Q[5] : Q[2] + Q[3] ) + 1 ) >> 1;
  int mid;
  if( nP == nQ )
  {
    if( nP == 5 ) mid = ( 2 * ( P[0] + Q[0] + P[1] + Q[1] + P[2] + Q[2] ) + P[3] + Q[3] + P[4] + Q[4] + 8 ) >> 4;
    else          mid = ( 2 * ( P[0] + Q[0] ) + P[1] + Q[1] + P[2] + Q[2] + P[3] + Q[3] + P[4] + Q[4] + P[5] + Q[5] + P[6] + Q[6] + 8 ) >> 4;
  }
  else
  {
    const int nb = max( nP, nQ ), ns = min( nP, nQ );
    if( nb == 7 && ns == 5 ) mid = ( 2 * ( P[0] + Q[0] + P[1] + Q[1] ) + P[2] + Q[2] + P[3] + Q[3] + P[4] + Q[4] + P[5] + Q[5] + 8 ) >> 4;
    else if( nb == 7 )
    {
      // the asymmetric 7 / 3 form: B = the long side, S = the short side
      const bool pBig = nP > nQ;
      int B[7], S[3];
#pragma unroll
      for( int j = 0; j < 7; j++ ) B[j] = pBig ? P[j] : Q[j];
#pragma unroll
      for( int j = 0; j < 3; j++ ) S[j] = pBig ? Q[j] : P[j];
      mid = ( 2 * ( B[0] + S[0] ) + S[0] + 2 * ( S[1] + S[2] ) + B[1] + S[1] + B[2] + B[3] + B[4] + B[5] + B[6] + 8 ) >> 4;
    }
    else mid = ( P[0] + Q[0] + P[1] + Q[1] + P[2] + Q[2] + P[3] + Q[3] + 4 ) >> 3;
  }
  // dbCoeffs7 = 59 - 9 j, dbCoeffs5 = 58 - 13 j, dbCoeffs3 = 53 - 21 j; tc7 = { 6, 5, 4, 3, 2, 1, 1 }, tc3 = { 6, 4, 2 }
#pragma unroll
  for( int j = 0; j < 7; j++ )
  {
    if( j < nP )
    {
      const int c = nP == 7 ? 59 - 9 * j : nP == 5 ? 58 - 13 * j : 53 - 21 * j, cv = ( tc * ( nP == 3 ? 6 - 2 * j : j < 6 ? 6 - j : 1 ) ) >> 1;
      DBK_PUT( -1 - j, dbkClip3( P[j] - cv, P[j] + cv, ( mid * c + refP * ( 64 - c ) + 32 ) >> 6 ) );
    }
    if( j < nQ )
    {
      const int c = nQ == 7 ? 59 - 9 * j : nQ == 5 ? 58 - 13 * j : 53 - 21 * j, cv = ( tc * ( nQ == 3 ? 6 - 2 * j : j < 6 ? 6 - j : 1 ) ) >> 1;
      DBK_PUT( j, dbkClip3( Q[j] - cv, Q[j] + cv, ( mid * c + refQ * ( 64 - c ) + 32 ) >> 6 ) );
    }
  }
}

// xEdgeFilterLuma (:1372-1520) for the edge segment whose q0 of line 0 is t[0]; off = the step across the edge, step = the step along it
__device__ __forceinline__ void dbkLuma( int16_t* __restrict__ t, uint8_t* __restrict__ mk, int off, int step, int bs, int qp, int len, bool ctuTop, int bd, const DbkPlaneDev& p )
{
  const int lp = ( len >> 4 ) & 7, lq = len & 7;
  const bool pL = lp > 3 && !ctuTop, qL = lq > 3;      // at a horizontal CTU boundary the P side is never long (:1437)
  const int tc = dbkTc( qp, bs, p.tcOff, bd ), beta = dbkBeta( qp, p.betaOff, bd );
  DbkLine s0, s3;
  dbkLoadLine<-8, 7>( s0, t, off );
  dbkLoadLine<-8, 7>( s3, t + 3 * step, off );
  const int dp0 = abs( s0.v[5] - 2 * s0.v[6] + s0.v[7] ), dq0 = abs( s0.v[8] - 2 * s0.v[9] + s0.v[10] );
  const int dp3 = abs( s3.v[5] - 2 * s3.v[6] + s3.v[7] ), dq3 = abs( s3.v[8] - 2 * s3.v[9] + s3.v[10] );
  const int d0 = dp0 + dq0, d3 = dp3 + dq3;
  if( pL || qL )
  {
    const int dp0L = pL ? ( dp0 + abs( s0.v[2] - 2 * s0.v[3] + s0.v[4] ) + 1 ) >> 1 : dp0, dq0L = qL ? ( dq0 + abs( s0.v[11] - 2 * s0.v[12] + s0.v[13] ) + 1 ) >> 1 : dq0;
    const int dp3L = pL ? ( dp3 + abs( s3.v[2] - 2 * s3.v[3] + s3.v[4] ) + 1 ) >> 1 : dp3, dq3L = qL ? ( dq3 + abs( s3.v[11] - 2 * s3.v[12] + s3.v[13] ) + 1 ) >> 1 : dq3;
    const int d0L = dp0L + dq0L, d3L = dp3L + dq3L;
    if( d0L + d3L < beta && dbkUseStrong( s0, 2 * d0L, beta, tc, pL, qL, lp, lq, false ) && dbkUseStrong( s3, 2 * d3L, beta, tc, pL, qL, lp, lq, false ) )
    {
      const int nP = pL ? lp : 3, nQ = qL ? lq : 3;
      for( int i = 0; i < 4; i++ ) dbkLongLine( t + i * step, mk + i * step, off, nP, nQ, tc );
      return;
    }
  }
  if( d0 + d3 >= beta ) return;
  bool secondP = false, secondQ = false;
  if( lp > 1 && lq > 1 )
  {
    const int side = ( beta + ( beta >> 1 ) ) >> 3;
    secondP = dp0 + dp3 < side; secondQ = dq0 + dq3 < side;
  }
  const bool sw = lp > 2 && lq > 2 && dbkUseStrong( s0, 2 * d0, beta, tc, false, false, 7, 7, false ) && dbkUseStrong( s3, 2 * d3, beta, tc, false, false, 7, 7, false );
  const int thr = tc * 10, lo = p.clipMin, hi = p.clipMax;
  // xPelFilterLumaCorePel (:217-264)
  for( int i = 0; i < 4; i++, t += step, mk += step )
  {
    DbkLine s;
    dbkLoadLine<-4, 3>( s, t, off );
    const int m0 = s.v[4], m1 = s.v[5], m2 = s.v[6], m3 = s.v[7], m4 = s.v[8], m5 = s.v[9], m6 = s.v[10], m7 = s.v[11];
    if( sw )
    {
      DBK_PUT( -3, dbkClip3( m1 - tc, m1 + tc, ( 2 * m0 + 3 * m1 + m2 + m3 + m4 + 4 ) >> 3 ) );
      DBK_PUT( -2, dbkClip3( m2 - 2 * tc, m2 + 2 * tc, ( m1 + m2 + m3 + m4 + 2 ) >> 2 ) );
      DBK_PUT( -1, dbkClip3( m3 - 3 * tc, m3 + 3 * tc, ( m1 + 2 * m2 + 2 * m3 + 2 * m4 + m5 + 4 ) >> 3 ) );
      DBK_PUT( 0, dbkClip3( m4 - 3 * tc, m4 + 3 * tc, ( m2 + 2 * m3 + 2 * m4 + 2 * m5 + m6 + 4 ) >> 3 ) );
      DBK_PUT( 1, dbkClip3( m5 - 2 * tc, m5 + 2 * tc, ( m3 + m4 + m5 + m6 + 2 ) >> 2 ) );
      DBK_PUT( 2, dbkClip3( m6 - tc, m6 + tc, ( m3 + m4 + m5 + 3 * m6 + 2 * m7 + 4 ) >> 3 ) );
    }
    else
    {
      int delta = ( 9 * ( m4 - m3 ) - 3 * ( m5 - m2 ) + 8 ) >> 4;
      if( abs( delta ) < thr )
      {
        delta = dbkClip3( -tc, tc, delta );
        const int tc2 = tc >> 1;
        DBK_PUT( -1, dbkClip3( lo, hi, m3 + delta ) );
        if( secondP ) DBK_PUT( -2, dbkClip3( lo, hi, m2 + dbkClip3( -tc2, tc2, ( ( ( m1 + m3 + 1 ) >> 1 ) - m2 + delta ) >> 1 ) ) );
        DBK_PUT( 0, dbkClip3( lo, hi, m4 - delta ) );
        if( secondQ ) DBK_PUT( 1, dbkClip3( lo, hi, m5 + dbkClip3( -tc2, tc2, ( ( ( m6 + m4 + 1 ) >> 1 ) - m5 - delta ) >> 1 ) ) );
      }
    }
  }
}

// xEdgeFilterChroma (:1522-1635) for one component and the 2-sample segment whose q0 of line 0 is t[0]; bs = the component's field
__device__ __forceinline__ void dbkChroma( int16_t* __restrict__ t, uint8_t* __restrict__ mk, int off, int step, int bs, int qp, bool large, bool ctb, int bd, const DbkPlaneDev& p )
{
  if( !( bs == 2 || ( large && bs == 1 ) ) ) return;
  const int tc = dbkTc( qp, bs, p.tcOff, bd ), lo = p.clipMin, hi = p.clipMax;
  DbkLine s0, s1;
  dbkLoadLine<-4, 3>( s0, t, off );
  dbkLoadLine<-4, 3>( s1, t + step, off );
  bool sw = false;
  if( large )
  {
    const int beta = dbkBeta( qp, p.betaOff, bd );
    // xCalcDP at a horizontal CTB boundary is | p1 - 2 p1 + p0 | (:1305)
    const int dp0 = ctb ? abs( s0.v[7] - s0.v[6] ) : abs( s0.v[5] - 2 * s0.v[6] + s0.v[7] ), dq0 = abs( s0.v[8] - 2 * s0.v[9] + s0.v[10] );
    const int dp3 = ctb ? abs( s1.v[7] - s1.v[6] ) : abs( s1.v[5] - 2 * s1.v[6] + s1.v[7] ), dq3 = abs( s1.v[8] - 2 * s1.v[9] + s1.v[10] );
    const int d0 = dp0 + dq0, d3 = dp3 + dq3;
    if( d0 + d3 < beta ) sw = dbkUseStrong( s0, 2 * d0, beta, tc, false, false, 7, 7, ctb ) && dbkUseStrong( s1, 2 * d3, beta, tc, false, false, 7, 7, ctb );
  }
  // xPelFilterChroma (:284-342)
#pragma unroll
  for( int i = 0; i < 2; i++, t += step, mk += step )
  {
    const DbkLine& s = i ? s1 : s0;
    const int m0 = s.v[4], m1 = s.v[5], m2 = s.v[6], m3 = s.v[7], m4 = s.v[8], m5 = s.v[9], m6 = s.v[10], m7 = s.v[11];
    if( sw )
    {
      if( ctb )
      {
        DBK_PUT( -1, dbkClip3( m3 - tc, m3 + tc, ( 3 * m2 + 2 * m3 + m4 + m5 + m6 + 4 ) >> 3 ) );
        DBK_PUT( 0, dbkClip3( m4 - tc, m4 + tc, ( 2 * m2 + m3 + 2 * m4 + m5 + m6 + m7 + 4 ) >> 3 ) );
      }
      else
      {
        DBK_PUT( -3, dbkClip3( m1 - tc, m1 + tc, ( 3 * m0 + 2 * m1 + m2 + m3 + m4 + 4 ) >> 3 ) );
        DBK_PUT( -2, dbkClip3( m2 - tc, m2 + tc, ( 2 * m0 + m1 + 2 * m2 + m3 + m4 + m5 + 4 ) >> 3 ) );
        DBK_PUT( -1, dbkClip3( m3 - tc, m3 + tc, ( m0 + m1 + m2 + 2 * m3 + m4 + m5 + m6 + 4 ) >> 3 ) );
        DBK_PUT( 0, dbkClip3( m4 - tc, m4 + tc, ( m1 + m2 + m3 + 2 * m4 + m5 + m6 + m7 + 4 ) >> 3 ) );
      }
      DBK_PUT( 1, dbkClip3( m5 - tc, m5 + tc, ( m2 + m3 + m4 + 2 * m5 + m6 + 2 * m7 + 4 ) >> 3 ) );
      DBK_PUT( 2, dbkClip3( m6 - tc, m6 + tc, ( m3 + m4 + m5 + 2 * m6 + 3 * m7 + 4 ) >> 3 ) );
    }
    else
    {
      const int delta = dbkClip3( -tc, tc, ( 4 * ( m4 - m3 ) + m2 - m5 + 4 ) >> 3 );
      DBK_PUT( -1, dbkClip3( lo, hi, m3 + delta ) );
      DBK_PUT( 0, dbkClip3( lo, hi, m4 - delta ) );
    }
  }
}
#undef DBK_PUT

// One direction of one ( CTU, plane ).  Tile: the CTU's w x h samples and DBK_MARGIN samples before and behind them ACROSS the direction; tile column of plane column x is
// x - tx0, tile row of plane row y is y - ty0; positions outside the picture hold 0 and are never written back.
template<bool VER>
__global__ void __launch_bounds__( DBK_THREADS )
dbkKernel( const DbkArgs a )
{
  extern __shared__ __attribute__( ( aligned( 16 ) ) ) unsigned char dbkLds[];
  const int tid = threadIdx.x, plane = blockIdx.y, chroma = plane > 0;
  const DbkPlaneDev& p = a.pl[plane];
  const int cx = ( int ) blockIdx.x % a.ctusX, cy = a.ctuRow0 + ( int ) blockIdx.x / a.ctusX, cs = a.ctu >> chroma;
  const int x0 = cx * cs, y0 = cy * cs, w = min( cs, p.width - x0 ), h = min( cs, p.height - y0 );
  const int tx0 = VER ? x0 - DBK_MARGIN : x0, ty0 = VER ? y0 : y0 - DBK_MARGIN;
  const int tw = VER ? w + 2 * DBK_MARGIN : w, th = VER ? h : h + 2 * DBK_MARGIN;
  const int pitch = ( VER ? cs + 2 * DBK_MARGIN : cs ) + 4, rowsMax = VER ? cs : cs + 2 * DBK_MARGIN;      // pitch: a multiple of 4 samples, rows of 4 stay 8-byte aligned
  int16_t* tile = reinterpret_cast<int16_t*>( dbkLds );
  uint8_t* mask = dbkLds + ( size_t ) pitch * rowsMax * sizeof( int16_t );
  // 8-byte groups of 4 samples: tx0, tw and the picture's width are multiples of 4, so a group lies inside the picture or outside it as a whole
  const bool vec = ( ( ( uintptr_t ) p.p | ( ( uintptr_t ) ( unsigned ) p.stride * 2u ) ) & 7u ) == 0;
  const int groups = tw >> 2;
  for( int i = tid; i < groups * th; i += DBK_THREADS )
  {
    const int r = i / groups, g = i - r * groups, x = tx0 + 4 * g, y = ty0 + r;
    DbkSeg4 s = { { 0, 0, 0, 0 } };
    if( x >= 0 && x < p.width && y >= 0 && y < p.height )
    {
      const int16_t* src = p.p + ( ptrdiff_t ) y * p.stride + x;
      if( vec ) s = *reinterpret_cast<const DbkSeg4*>( src );
      else { s.v[0] = src[0]; s.v[1] = src[1]; s.v[2] = src[2]; s.v[3] = src[3]; }
    }
    *reinterpret_cast<DbkSeg4*>( tile + r * pitch + 4 * g ) = s;
    *reinterpret_cast<uint32_t*>( mask + r * pitch + 4 * g ) = 0u;
  }
  __syncthreads();

  const int off = VER ? 1 : pitch, step = VER ? pitch : 1;
  if( !chroma )
  {
    // one segment per 4 x 4 unit of the CTU (xDeblockArea's dx / dy loops): the vertical edge at the unit's left, the horizontal edge at its top
    const int nux = w >> 2, nu = nux * ( h >> 2 );
    for( int u = tid; u < nu; u += DBK_THREADS )
    {
      const int uy = u / nux, ux = u - uy * nux, x = x0 + 4 * ux, y = y0 + 4 * uy;
      const uint2 rec = a.recs[( size_t ) ( ( y >> 2 ) - a.unitRow0 ) * a.mapW + ( x >> 2 )];
      const int bs = ( rec.x >> 24 ) & 3;
      if( !bs ) continue;
      const int at = ( y - ty0 ) * pitch + ( x - tx0 );
      dbkLuma( tile + at, mask + at, off, step, bs, ( int ) ( int8_t ) ( rec.x & 255u ), ( int ) ( rec.y & 255u ), !VER && ( y & ( a.ctu - 1 ) ) == 0, a.bitDepth, p );
    }
  }
  else
  {
    // 4:2:0: edges on the 8-sample grid of the chroma CTU (:449-452), one record — a 4 x 4 luma unit, 2 chroma samples along the edge — per segment
    const int across = ( ( VER ? w : h ) + 7 ) >> 3, along = ( VER ? h : w ) >> 1, ns = across * along;
    const int shift = 2 * plane;
    for( int u = tid; u < ns; u += DBK_THREADS )
    {
      const int e = u / along, j = u - e * along;
      const int x = x0 + ( VER ? 8 * e : 2 * j ), y = y0 + ( VER ? 2 * j : 8 * e );
      const uint2 rec = a.recs[( size_t ) ( ( y >> 1 ) - a.unitRow0 ) * a.mapW + ( x >> 1 )];
      const int bs = ( rec.x >> ( 24 + shift ) ) & 3;
      if( !bs ) continue;
      const int at = ( y - ty0 ) * pitch + ( x - tx0 );
      dbkChroma( tile + at, mask + at, off, step, bs, ( int ) ( int8_t ) ( ( rec.x >> ( 8 * plane ) ) & 255u ), ( rec.y & 0x2000u ) != 0, !VER && ( y & ( cs - 1 ) ) == 0, a.bitDepth, p );
    }
  }
  __syncthreads();

  // write-back: marked samples inside the picture only
  for( int i = tid; i < groups * th; i += DBK_THREADS )
  {
    const int r = i / groups, g = i - r * groups, x = tx0 + 4 * g, y = ty0 + r;
    const uint32_t m = *reinterpret_cast<const uint32_t*>( mask + r * pitch + 4 * g );
    if( !m || x < 0 || x >= p.width || y < 0 || y >= p.height ) continue;
    const DbkSeg4 s = *reinterpret_cast<const DbkSeg4*>( tile + r * pitch + 4 * g );
    int16_t* dst = p.p + ( ptrdiff_t ) y * p.stride + x;
    if( vec && m == 0x01010101u ) *reinterpret_cast<DbkSeg4*>( dst ) = s;
    else
    {
#pragma unroll
      for( int k = 0; k < 4; k++ )
        if( ( m >> ( 8 * k ) ) & 1u ) dst[k] = s.v[k];
    }
  }
}

inline bool dbkLenOk( int l ) { return l != 4 && l != 6; }

} // namespace

extern "C" {

int vvhip_deblock( vvhip_ctx* ctx, const vvhip_deblock_plane* planes, int n_planes, int bit_depth, int ctu_size, const vvhip_lf_param* lfp_ver_host, const vvhip_lf_param* lfp_hor_host,
                   int lfp_stride, int ctu_row0, int n_rows, int dirs )
{
  if( !ctx ) return VVHIP_E_ARG;
  if( !planes || ( n_planes != 1 && n_planes != 3 ) ) return vvhip_fail( ctx, VVHIP_E_ARG, "vvhip_deblock: %d planes (1 = luma only / 4:0:0, 3 = 4:2:0), planes missing", n_planes );
  if( bit_depth < 8 || bit_depth > 12 || ctu_size < 16 || ctu_size > 128 || ( ctu_size & ( ctu_size - 1 ) ) || dirs < 1 || dirs > 3 )
    return vvhip_fail( ctx, VVHIP_E_ARG, "vvhip_deblock: bitDepth %d (8..12), CTU size %d (16, 32, 64, 128), dirs %d (1..3)", bit_depth, ctu_size, dirs );
  const int W = planes[0].width, H = planes[0].height;
  if( W < 8 || H < 8 || ( W & 7 ) || ( H & 7 ) ) return vvhip_fail( ctx, VVHIP_E_ARG, "vvhip_deblock: luma %dx%d: both must be multiples of 8", W, H );
  DbkArgs A;
  memset( &A, 0, sizeof( A ) );
  for( int c = 0; c < n_planes; c++ )
  {
    const vvhip_deblock_plane& q = planes[c];
    if( !q.d_plane || q.stride < q.width || q.clip_min > q.clip_max || q.clip_min < -32768 || q.clip_max > 32767 || ( c && ( q.width * 2 != W || q.height * 2 != H ) ) )
      return vvhip_fail( ctx, VVHIP_E_ARG, "vvhip_deblock: plane %d: %dx%d (chroma: exactly half of luma %dx%d), stride %d, clip [%d, %d]", c, q.width, q.height, W, H, q.stride, q.clip_min, q.clip_max );
    DbkPlaneDev& p = A.pl[c];
    p.p = q.d_plane; p.stride = q.stride; p.width = q.width; p.height = q.height; p.clipMin = q.clip_min; p.clipMax = q.clip_max; p.betaOff = q.beta_offset_div2; p.tcOff = q.tc_offset_div2;
  }
  const int ctusX = ( W + ctu_size - 1 ) / ctu_size, ctusY = ( H + ctu_size - 1 ) / ctu_size, mapW = W >> 2;
  if( ctu_row0 < 0 || n_rows < 1 || ctu_row0 > ctusY - n_rows ) return vvhip_fail( ctx, VVHIP_E_ARG, "vvhip_deblock: CTU rows [%d, %d + %d) of %d", ctu_row0, ctu_row0, n_rows, ctusY );
  if( lfp_stride < mapW || ( ( dirs & VVHIP_DBK_VER ) && !lfp_ver_host ) || ( ( dirs & VVHIP_DBK_HOR ) && !lfp_hor_host ) )
    return vvhip_fail( ctx, VVHIP_E_ARG, "vvhip_deblock: map stride %d (>= %d), a map of dirs %d missing", lfp_stride, mapW, dirs );
  // the band's records of the wanted directions -> one blob of 8-byte records: [ VER ][ HOR ]
  const int unitRow0 = ctu_row0 * ( ctu_size >> 2 ), unitRows = std::min( H >> 2, ( ctu_row0 + n_rows ) * ( ctu_size >> 2 ) ) - unitRow0;
  const size_t perDir = ( size_t ) unitRows * mapW;
  std::vector<DbkRec> dev( perDir * ( dirs == 3 ? 2 : 1 ) );
  size_t at = 0;
  for( int bit = VVHIP_DBK_VER; bit <= VVHIP_DBK_HOR; bit <<= 1 )
  {
    if( !( dirs & bit ) ) continue;
    const vvhip_lf_param* map = bit == VVHIP_DBK_VER ? lfp_ver_host : lfp_hor_host;
    for( int r = 0; r < unitRows; r++ )
      for( int x = 0; x < mapW; x++, at++ )
      {
        const vvhip_lf_param& q = map[( size_t ) ( unitRow0 + r ) * lfp_stride + x];
        const int b0 = q.bs & 3, b1 = ( q.bs >> 2 ) & 3, b2 = ( q.bs >> 4 ) & 3;
        const bool first = bit == VVHIP_DBK_VER ? x == 0 : unitRow0 + r == 0;
        if( b0 == 3 || b1 == 3 || b2 == 3 || ( q.flags & ~0x23 ) || ( b0 && !( dbkLenOk( ( q.side_max_filt_length >> 4 ) & 7 ) && dbkLenOk( q.side_max_filt_length & 7 ) ) ) || ( first && ( q.bs & 0x3f ) ) )
          return vvhip_fail( ctx, VVHIP_E_ARG, "vvhip_deblock: %s map, unit (%d, %d): bs 0x%02x (fields 0..2; 0 in the first column / row: the edge would read outside the picture), lengths 0x%02x "
                             "(P, Q in 0, 1, 2, 3, 5, 7), flags 0x%02x (bits 0, 1, 5)", bit == VVHIP_DBK_VER ? "vertical" : "horizontal", x, unitRow0 + r, q.bs, q.side_max_filt_length, q.flags );
        DbkRec& o = dev[at];
        o.qp[0] = q.qp[0]; o.qp[1] = q.qp[1]; o.qp[2] = q.qp[2]; o.bs = q.bs & 0x3f; o.len = q.side_max_filt_length; o.flags = q.flags; o.pad[0] = o.pad[1] = 0;
      }
  }
  HostList& S = ctx->list[LIST_DEBLOCK];
  const int rc = listUpload( ctx, S, ListBlob( dev.data(), dev.size() * sizeof( DbkRec ) ) );
  if( rc != VVHIP_OK ) return rc;
  A.mapW = mapW; A.unitRow0 = unitRow0; A.ctusX = ctusX; A.ctuRow0 = ctu_row0; A.ctu = ctu_size; A.bitDepth = bit_depth; A.nPlanes = n_planes;
  const dim3 grid( ctusX * n_rows, n_planes );
  const size_t lds = ( size_t ) ( ctu_size + 4 ) * ( ctu_size + 2 * DBK_MARGIN ) * 3;      // the larger of the two tile shapes (the horizontal one), samples + mask: 57,024 bytes at CTU 128
  const uint2* d = ( const uint2* ) S.d;
  if( dirs & VVHIP_DBK_VER )
  {
    A.recs = d;
    hipLaunchKernelGGL( dbkKernel<true>, grid, dim3( DBK_THREADS ), lds, ctx->stream, A );
    VVHIP_LAUNCH_CHECK( ctx );
    d += perDir;
  }
  if( dirs & VVHIP_DBK_HOR )
  {
    A.recs = d;
    hipLaunchKernelGGL( dbkKernel<false>, grid, dim3( DBK_THREADS ), lds, ctx->stream, A );
    VVHIP_LAUNCH_CHECK( ctx );
  }
  return listLaunched( ctx, S );
}

} // extern "C"
