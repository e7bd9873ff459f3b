// predaffine.hip — inter prediction of a LIST of affine CUs from their control-point vectors: luma with PROF and 4:2:0 chroma, uni- and bi-predicted, every CU size in
// one launch, optionally with the residual against the original.
//
// Reference behaviour (all integer, bit-exact):
//   InterPredInterpolation::xPredAffineBlk                 CommonLib/InterPrediction.cpp:1497-1839 (model deltas :1528-1542, picture clip :1545-1550, PROF conditions :1555-1561,
//                                                          dMv table :1583-1630, sub-block vectors :1697-1765, interpolation :1784-1795, PROF ring :1797-1820)
//   InterPredInterpolation::isSubblockVectorSpreadOverLimit :1457-1495
//   roundAffineMv                                           CommonLib/Mv.cpp:61-66
//   gradFilterCore<false> / applyPROFCore                   CommonLib/InterPrediction.cpp:113-131 / :88-111
//   xWeightedAverage -> AreaBuf<Pel>::addAvg                :960-1010, CommonLib/Buffer.cpp:549-575 (core :129-141)
//
// The record that crosses PCIe and HBM is the CU (vvhip_pred_affine_item resolved against the plane table: AffDev); the schedule adds one 8-byte record per TILE of at most
// sixteen 4x4 sub-blocks (16x16, 8x32 or the whole block when it is smaller).  One wave takes sixteen sub-blocks of one class — one tile, or several whole small blocks —, four
// lanes per sub-block (one DPP quad), each lane one 4-sample row.  Every lane derives its sub-block's vector from the control points in registers: the model deltas, the value at
// the sub-block's centre (or at the CU's when the spread is over the limit), roundAffineMv, the 18-bit clip, for chroma the average of the two diagonal luma vectors, the picture
// clip, position and fraction, and for PROF its row of the dMv table.  Per reference list a quad
//   1. reads the rows of its sub-block's own window from HBM as aligned dwords (only the rows / columns the two fractions reach; neighbouring sub-blocks overlap in the cache),
//      runs the horizontal pass on them into the 14-bit intermediate in LDS (isFirst, !isLast) — lane r takes rows r, r + 4, r + 8,
//   2. runs the vertical pass from it into registers (!isFirst; isLast when the list is alone and PROF is off),
//   3. with PROF: takes the horizontal gradient from its own row and the two ring samples beside it, the vertical gradient from its quad neighbours by quad permute (the top
//      and the bottom lane read their ring row), and adds the clipped dMv * gradient term.
// The tap sets are those of today's 4x4 items (pred.hip: m_lumaFilter4x4, whose outer taps are zero — six taps here — and m_chromaFilter), a zero fraction the one-tap set { 64 }:
// see pred.hip for why the two-pass form gives the values of the reference's single-pass and copy forms.  A bi-predicted CU keeps list 0's 14-bit block in registers while list 1
// goes through the same LDS, then averages.  Waves synchronise with themselves only; a workgroup is four independent waves.
// Still the caller's: the PROF conditions on SPS / picture-header flags, m_skipPROF and equal picture sizes; BCW / explicit weighted prediction.
#include <algorithm>
#include <string.h>
#include "common.h"

namespace {

// m_lumaFilter4x4 without its two outer (zero) taps, phases 0..8; row 16 - p is row p reversed (InterpolationFilter.cpp:64-142)
__constant__ int8_t cALuma6[9][6] = {
  { 0, 0, 64, 0, 0, 0 }, { 1, -3, 63, 4, -2, 1 }, { 1, -5, 62, 8, -3, 1 }, { 2, -8, 60, 13, -4, 1 }, { 3, -10, 58, 17, -5, 1 },
  { 3, -11, 52, 26, -8, 2 }, { 2, -9, 47, 31, -10, 3 }, { 3, -11, 45, 34, -10, 3 }, { 3, -11, 40, 40, -11, 3 } };
__constant__ int8_t cAChroma4[17][4] = {
  { 0, 64, 0, 0 }, { -1, 63, 2, 0 }, { -2, 62, 4, 0 }, { -2, 60, 7, -1 }, { -2, 58, 10, -2 }, { -3, 57, 12, -2 }, { -4, 56, 14, -2 }, { -4, 55, 15, -2 }, { -4, 54, 16, -2 },
  { -5, 53, 18, -2 }, { -6, 52, 20, -2 }, { -6, 49, 24, -3 }, { -6, 46, 28, -4 }, { -5, 44, 29, -4 }, { -4, 42, 30, -4 }, { -4, 39, 33, -4 }, { -4, 36, 36, -4 } };

// ---- the schedule the host uploads ----
struct __attribute__( ( aligned( 16 ) ) ) AffDev      // one component block of one affine CU with the plane table resolved
{
  const int16_t* ref[2];         // the block's own (zero-vector) position per list; null = list not used
  int32_t stride[2];
  int32_t dstOff, orgOff;
  int32_t cpmv[2][3][2];
  int16_t cuX, cuY;
  uint8_t log2W, log2H;          // the CU in luma samples
  uint8_t chroma, six, prof, pad[5];
};
struct AffSub  { int32_t item; int16_t x0, y0; };      // one tile of a block, origin in samples of the component
struct AffUnit { int32_t firstSub; int16_t nSub; uint8_t log2Sb, log2SbW, chroma, pad[7]; };      // what one wave does: nSub tiles of 1 << log2Sb sub-blocks, 1 << log2SbW in a row
static_assert( sizeof( AffDev ) == 96 && sizeof( AffSub ) == 8 && sizeof( AffUnit ) == 16, "schedule records" );

struct AffArgs
{
  const AffDev* items; const AffSub* subs; const AffUnit* units;
  int nUnits, bitDepth, picW, picH, ctu;
  int16_t* pred; int predStride;
  const int16_t* org; int orgStride;
  int16_t* resi;
};

#define AFF_WAVE_SYNC() { __builtin_amdgcn_fence( __ATOMIC_ACQ_REL, "wavefront" ); __builtin_amdgcn_wave_barrier(); }
#define AFF_QUAD_UP   0x90     /* quad_perm [0,0,1,2]: lane r reads lane r - 1 */
#define AFF_QUAD_DOWN 0xF9     /* quad_perm [1,2,3,3]: lane r reads lane r + 1 */

__host__ __device__ inline int affClamp( int v, int lo, int hi ) { return v < lo ? lo : ( v > hi ? hi : v ); }
__host__ __device__ inline int affRound( int v, int shift ) { return ( v + ( 1 << ( shift - 1 ) ) - ( v >= 0 ? 1 : 0 ) ) >> shift; }      // roundAffineMv, one component
__host__ __device__ inline int affMax4( int a, int b, int c, int d ) { const int x = a > b ? a : b, y = c > d ? c : d; return x > y ? x : y; }
__host__ __device__ inline int affMin4( int a, int b, int c, int d ) { const int x = a < b ? a : b, y = c < d ? c : d; return x < y ? x : y; }

// isSubblockVectorSpreadOverLimit :1457-1495 ( a, b = horizontal delta x, y; c, d = vertical delta x, y )
__host__ __device__ inline bool affSpreadOverLimit( int a, int b, int c, int d, bool bothLists )
{
  const int s4 = 4 << 11, tap = 6;
  if( bothLists )
  {
    int rw = affMax4( 0, 4 * a + s4, 4 * c, 4 * a + 4 * c + s4 ) - affMin4( 0, 4 * a + s4, 4 * c, 4 * a + 4 * c + s4 );
    int rh = affMax4( 0, 4 * b, 4 * d + s4, 4 * b + 4 * d + s4 ) - affMin4( 0, 4 * b, 4 * d + s4, 4 * b + 4 * d + s4 );
    rw = ( rw >> 11 ) + tap + 3; rh = ( rh >> 11 ) + tap + 3;
    return rw * rh > ( tap + 9 ) * ( tap + 9 );
  }
  int rw = ( 4 * a + s4 > 0 ? 4 * a + s4 : 0 ) - ( 4 * a + s4 < 0 ? 4 * a + s4 : 0 ), rh = ( 4 * b > 0 ? 4 * b : 0 ) - ( 4 * b < 0 ? 4 * b : 0 );
  rw = ( rw >> 11 ) + tap + 3; rh = ( rh >> 11 ) + tap + 3;
  if( rw * rh > ( tap + 9 ) * ( tap + 5 ) ) return true;
  rw = ( 4 * c > 0 ? 4 * c : 0 ) - ( 4 * c < 0 ? 4 * c : 0 ); rh = ( 4 * d + s4 > 0 ? 4 * d + s4 : 0 ) - ( 4 * d + s4 < 0 ? 4 * d + s4 : 0 );
  rw = ( rw >> 11 ) + tap + 3; rh = ( rh >> 11 ) + tap + 3;
  return rw * rh > ( tap + 5 ) * ( tap + 9 );
}

// taps of one direction as c[k] * sample[pos - lo + k]; a zero fraction is the one-tap set { 64 } at lo = 0
template<int NT>
__device__ __forceinline__ void affTaps( int ( &c )[NT], int& lo, int frac )
{
#pragma unroll
  for( int k = 0; k < NT; k++ ) c[k] = 0;
  lo = 0;
  if( frac == 0 ) { c[0] = 64; return; }
  lo = NT / 2 - 1;
  if( NT == 6 )
  {
    const int p = frac <= 8 ? frac : 16 - frac;
#pragma unroll
    for( int k = 0; k < NT; k++ ) c[k] = cALuma6[p][frac <= 8 ? k : 5 - k];
  }
  else
  {
#pragma unroll
    for( int k = 0; k < NT; k++ ) c[k] = frac <= 16 ? cAChroma4[frac][k & 3] : cAChroma4[32 - frac][3 - ( k & 3 )];
  }
}

struct __attribute__( ( aligned( 8 ) ) ) Row4 { int16_t v[4]; };

// what a lane knows about its sub-block
struct AffLane
{
  bool on;
  const int16_t* ref[2]; int stride[2];
  int cp[2][3][2];
  int cuX, cuY, log2W, log2H, six, prof;
  int sx, sy;                    // the sub-block's origin inside the block, in samples of the component
  int r;                         // the lane's row
  int16_t* tmp;                  // the quad's first-pass block in LDS: ( 4 + NT - 1 ) rows of 4
  int16_t* dst; int dstPitch;    // block origin in the prediction buffer
  const int16_t* org; int orgPitch;
  int16_t* res;
};

// NT = 6: luma (1/16 sample), NT = 4: 4:2:0 chroma (1/32 sample)
template<int NT>
__device__ __forceinline__ void affBody( const AffLane& L, const AffArgs& a )
{
  constexpr bool CHROMA = NT == 4;
  constexpr int ND = ( 4 + NT ) / 2 + 1;      // ND dwords hold a row's 4 + NT - 1 window samples at either alignment
  const int bitDepth = a.bitDepth, hr = 14 - bitDepth > 2 ? 14 - bitDepth : 2, maxv = ( 1 << bitDepth ) - 1;
  const bool bi = L.ref[0] != nullptr && L.ref[1] != nullptr;
  // picture clip :1545-1550
  const int horMax = ( a.picW + 8 - L.cuX - 1 ) << 4, horMin = ( -a.ctu - 8 - L.cuX + 1 ) * 16;
  const int verMax = ( a.picH + 8 - L.cuY - 1 ) << 4, verMin = ( -a.ctu - 8 - L.cuY + 1 ) * 16;
  int first[4], acc[4];
#pragma unroll
  for( int j = 0; j < 4; j++ ) first[j] = acc[j] = 0;

#pragma unroll
  for( int l = 0; l < 2; l++ )
  {
    const bool use = L.on && L.ref[l] != nullptr;
    // ---- the model :1528-1542 (always the luma quantities), the sub-block's vector :1697-1765
    const int dHorX = ( L.cp[l][1][0] - L.cp[l][0][0] ) * ( 1 << ( 7 - L.log2W ) ), dHorY = ( L.cp[l][1][1] - L.cp[l][0][1] ) * ( 1 << ( 7 - L.log2W ) );
    const int dVerX = L.six ? ( L.cp[l][2][0] - L.cp[l][0][0] ) * ( 1 << ( 7 - L.log2H ) ) : -dHorY, dVerY = L.six ? ( L.cp[l][2][1] - L.cp[l][0][1] ) * ( 1 << ( 7 - L.log2H ) ) : dHorX;
    const int baseX = L.cp[l][0][0] * 128, baseY = L.cp[l][0][1] * 128;
    const bool spread = affSpreadOverLimit( dHorX, dHorY, dVerX, dVerY, bi );
    int mvx, mvy;
    if( !CHROMA )
    {
      const int px = spread ? ( 1 << L.log2W ) >> 1 : 2 + L.sx, py = spread ? ( 1 << L.log2H ) >> 1 : 2 + L.sy;
      mvx = affClamp( affRound( baseX + dHorX * px + dVerX * py, 7 ), -( 1 << 17 ), ( 1 << 17 ) - 1 );
      mvy = affClamp( affRound( baseY + dHorY * px + dVerY * py, 7 ), -( 1 << 17 ), ( 1 << 17 ) - 1 );
    }
    else
    {
      // the stored vectors of the top-left and the bottom-right luma sub-block under this chroma sub-block :1729-1739
      const int px0 = spread ? ( 1 << L.log2W ) >> 1 : 2 + 2 * L.sx, py0 = spread ? ( 1 << L.log2H ) >> 1 : 2 + 2 * L.sy;
      const int px1 = spread ? px0 : px0 + 4, py1 = spread ? py0 : py0 + 4;
      const int ax = affClamp( affRound( baseX + dHorX * px0 + dVerX * py0, 7 ), -( 1 << 17 ), ( 1 << 17 ) - 1 );
      const int ay = affClamp( affRound( baseY + dHorY * px0 + dVerY * py0, 7 ), -( 1 << 17 ), ( 1 << 17 ) - 1 );
      const int bx = affClamp( affRound( baseX + dHorX * px1 + dVerX * py1, 7 ), -( 1 << 17 ), ( 1 << 17 ) - 1 );
      const int by = affClamp( affRound( baseY + dHorY * px1 + dVerY * py1, 7 ), -( 1 << 17 ), ( 1 << 17 ) - 1 );
      mvx = affRound( ax + bx, 1 ); mvy = affRound( ay + by, 1 );
    }
    mvx = affClamp( mvx, horMin, horMax ); mvy = affClamp( mvy, verMin, verMax );
    const int fs = CHROMA ? 5 : 4, fm = ( 1 << fs ) - 1;
    const int xInt = mvx >> fs, yInt = mvy >> fs, fx = mvx & fm, fy = mvy & fm;
    // ---- PROF for this list :1555-1560 (the conditions that depend on the vectors; the others are the caller's)
    bool prof = false;
    if( !CHROMA )
    {
      const bool same = L.cp[l][0][0] == L.cp[l][1][0] && L.cp[l][0][1] == L.cp[l][1][1] && ( !L.six || ( L.cp[l][0][0] == L.cp[l][2][0] && L.cp[l][0][1] == L.cp[l][2][1] ) );
      prof = L.prof != 0 && !same && !spread;
      if( L.prof >= 2 )
      {
        const int thr = 1 << ( 7 + ( L.prof == 3 ? 1 : 0 ) );
        prof = prof && ( dHorX > thr || dHorY > thr || dVerX > thr || dVerY > thr || dHorX < -thr || dHorY < -thr || dVerX < -thr || dVerY < -thr );
      }
    }
    const bool last = !bi && !prof;
    const int16_t* blk = use ? L.ref[l] + ( ptrdiff_t ) ( L.sy + yInt ) * L.stride[l] + ( L.sx + xInt ) : nullptr;      // the sub-block at its integer position

    int ch[NT], cv[NT], loX = 0, loY = 0;
    affTaps<NT>( ch, loX, fx );
    affTaps<NT>( cv, loY, fy );
    // ---- 1. horizontal pass, isFirst && !isLast: ( sum - ( 8192 << s1 ) ) >> s1 with s1 = 6 - headroom; rows - loY .., columns - loX - sh .. as aligned dwords
    if( use )
    {
      const int rows = 4 + ( fy ? NT - 1 : 0 ), cols = 4 + ( fx ? NT - 1 : 0 );
      const int s1 = 6 - hr, off1 = -( 8192 << s1 );
      for( int i = L.r; i < rows; i += 4 )
      {
        const uintptr_t ga = reinterpret_cast<uintptr_t>( blk + ( ptrdiff_t ) ( i - loY ) * L.stride[l] - loX );
        const int sh = ( int ) ( ( ga >> 1 ) & 1 );
        const uint32_t* g32 = reinterpret_cast<const uint32_t*>( ga & ~( uintptr_t ) 3 );
        const int nd = ( cols + sh + 1 ) >> 1;
        uint32_t d[ND];
#pragma unroll
        for( int k = 0; k < ND; k++ ) d[k] = k < nd ? g32[k] : 0u;
        int win[4 + NT];
#pragma unroll
        for( int k = 0; k < ND - 1; k++ )
        {
          const uint32_t s = __builtin_amdgcn_alignbit( d[k + 1], d[k], ( uint32_t ) ( sh << 4 ) );
          win[2 * k] = ( int ) ( int16_t ) ( s & 0xffff ); win[2 * k + 1] = ( int ) ( int16_t ) ( s >> 16 );
        }
        Row4 o;
#pragma unroll
        for( int j = 0; j < 4; j++ )
        {
          int s = 0;
#pragma unroll
          for( int k = 0; k < NT; k++ ) s = __mul24( win[j + k], ch[k] ) + s;       // |sample| < 2^15, |tap| < 2^7: the 24-bit multiply is exact
          o.v[j] = ( int16_t ) ( ( s + off1 ) >> s1 );
        }
        *reinterpret_cast<Row4*>( L.tmp + i * 4 ) = o;
      }
    }
    AFF_WAVE_SYNC();
    // ---- 2. vertical pass, !isFirst: isLast ( + clip ) for a list that is alone without PROF, the 14-bit block otherwise
    if( use )
    {
#pragma unroll
      for( int j = 0; j < 4; j++ ) acc[j] = 0;
      const int nv = fy ? NT : 1;
#pragma unroll
      for( int k = 0; k < NT; k++ )
      {
        if( k < nv )
        {
          const Row4 row = *reinterpret_cast<const Row4*>( L.tmp + ( L.r + k ) * 4 );
#pragma unroll
          for( int j = 0; j < 4; j++ ) acc[j] = __mul24( ( int ) row.v[j], cv[k] ) + acc[j];
        }
      }
      if( last )
      {
        const int s2 = 6 + hr, off2 = ( 1 << ( s2 - 1 ) ) + ( 8192 << 6 );
#pragma unroll
        for( int j = 0; j < 4; j++ ) { const int v = ( int16_t ) ( ( acc[j] + off2 ) >> s2 ); acc[j] = v < 0 ? 0 : ( v > maxv ? maxv : v ); }
      }
      else
      {
#pragma unroll
        for( int j = 0; j < 4; j++ ) acc[j] = ( int16_t ) ( acc[j] >> 6 );
      }
    }
    AFF_WAVE_SYNC();
    // ---- 3. PROF :1583-1630, :1797-1835 — luma only
    if( !CHROMA )
    {
      const bool doProf = use && prof;
      // the ring at the integer position rounded by frac >> 3: ( ref << headroom ) - IF_INTERNAL_OFFS
      int left = 0, right = 0, edge[4] = { 0, 0, 0, 0 };
      if( doProf )
      {
        const int16_t* rp = blk + ( ptrdiff_t ) ( fy >> 3 ) * L.stride[l] + ( fx >> 3 );
        const int16_t* row = rp + ( ptrdiff_t ) L.r * L.stride[l];
        left = ( ( int ) row[-1] << hr ) - 8192; right = ( ( int ) row[4] << hr ) - 8192;
        if( L.r == 0 || L.r == 3 )
        {
          const int16_t* er = rp + ( ptrdiff_t ) ( L.r == 0 ? -1 : 4 ) * L.stride[l];
#pragma unroll
          for( int j = 0; j < 4; j++ ) edge[j] = ( ( int ) er[j] << hr ) - 8192;
        }
      }
      // (the quad permutes run for every lane of the wave: no lane of a quad may be masked off while its neighbours read it)
      int up[4], down[4];
#pragma unroll
      for( int j = 0; j < 4; j++ ) { up[j] = VVHIP_DPP( acc[j], AFF_QUAD_UP ); down[j] = VVHIP_DPP( acc[j], AFF_QUAD_DOWN ); }
      if( doProf )
      {
        int refined[4];
        const int dILimit = 1 << ( bitDepth + 1 > 13 ? bitDepth + 1 : 13 );
        const int sn = hr, off = ( 1 << ( sn - 1 ) ) + 8192;
        // row r of the dMv table: dMv[w + 4 h] = -6 ( hor + ver ) + 4 w hor + 4 h ver, roundAffineMv( ., 8 ), clip to +-31
        const int d0x = -6 * ( dHorX + dVerX ) + 4 * L.r * dVerX, d0y = -6 * ( dHorY + dVerY ) + 4 * L.r * dVerY;
#pragma unroll
        for( int j = 0; j < 4; j++ )
        {
          const int dmx = affClamp( affRound( d0x + 4 * j * dHorX, 8 ), -31, 31 ), dmy = affClamp( affRound( d0y + 4 * j * dHorY, 8 ), -31, 31 );
          const int xl = j == 0 ? left : acc[j > 0 ? j - 1 : 0], xr = j == 3 ? right : acc[j < 3 ? j + 1 : 3];
          const int yu = L.r == 0 ? edge[j] : up[j], yd = L.r == 3 ? edge[j] : down[j];
          const int gx = ( xr >> 6 ) - ( xl >> 6 ), gy = ( yd >> 6 ) - ( yu >> 6 );
          const int dI = affClamp( dmx * gx + dmy * gy, -dILimit, dILimit - 1 );
          refined[j] = ( int16_t ) ( acc[j] + dI );      // (kept apart: the neighbours' gradients read the unrefined block; the Pel store comes before the rounding)
        }
#pragma unroll
        for( int j = 0; j < 4; j++ )
        {
          if( bi ) acc[j] = refined[j];
          else { const int v = ( int16_t ) ( ( refined[j] + off ) >> sn ); acc[j] = v < 0 ? 0 : ( v > maxv ? maxv : v ); }
        }
      }
    }
    if( l == 0 )
    {
#pragma unroll
      for( int j = 0; j < 4; j++ ) first[j] = acc[j];
    }
  }
  if( !L.on ) return;
  if( bi )      // addAvg: ClipPel( ( a + b + offset ) >> shiftNum ), shiftNum = headroom + 1, offset = ( 1 << headroom ) + 2 * IF_INTERNAL_OFFS (Buffer.cpp:129-141, :549-575)
  {
    const int sn = hr + 1, off = ( 1 << hr ) + 2 * 8192;
#pragma unroll
    for( int j = 0; j < 4; j++ ) { const int v = ( first[j] + acc[j] + off ) >> sn; acc[j] = v < 0 ? 0 : ( v > maxv ? maxv : v ); }
  }
  else if( L.ref[1] == nullptr )
  {
#pragma unroll
    for( int j = 0; j < 4; j++ ) acc[j] = first[j];
  }
  const int row = L.sy + L.r, col = L.sx;
  Row4 o;
#pragma unroll
  for( int j = 0; j < 4; j++ ) o.v[j] = ( int16_t ) acc[j];
  int16_t* dp = L.dst + ( ptrdiff_t ) row * L.dstPitch + col;
  if( ( reinterpret_cast<uintptr_t>( dp ) & 7 ) == 0 ) *reinterpret_cast<Row4*>( dp ) = o;
  else
  {
#pragma unroll
    for( int j = 0; j < 4; j++ ) dp[j] = o.v[j];
  }
  if( L.res )
  {
    const int16_t* op = L.org + ( ptrdiff_t ) row * L.orgPitch + col;
    Row4 g;
    if( ( reinterpret_cast<uintptr_t>( op ) & 7 ) == 0 ) g = *reinterpret_cast<const Row4*>( op );
    else
    {
#pragma unroll
      for( int j = 0; j < 4; j++ ) g.v[j] = op[j];
    }
#pragma unroll
    for( int j = 0; j < 4; j++ ) g.v[j] = ( int16_t ) ( g.v[j] - o.v[j] );
    int16_t* rp = L.res + ( ptrdiff_t ) row * L.dstPitch + col;
    if( ( reinterpret_cast<uintptr_t>( rp ) & 7 ) == 0 ) *reinterpret_cast<Row4*>( rp ) = g;
    else
    {
#pragma unroll
      for( int j = 0; j < 4; j++ ) rp[j] = g.v[j];
    }
  }
}

constexpr int AFF_TMP_QUAD = 9 * 4;      // first-pass samples per quad: 9 rows of 4 (chroma uses 7)

// a list of affine CUs of mixed sizes: wave -> unit of the host's schedule (size classes, picture bands per XCD)
__global__ void __launch_bounds__( 256 )
predAffineKernel( AffArgs a )
{
  __shared__ __attribute__( ( aligned( 16 ) ) ) int16_t sAff[4 * 16 * AFF_TMP_QUAD];
  const int wave = __builtin_amdgcn_readfirstlane( ( int ) ( threadIdx.x >> 6 ) ), lane = threadIdx.x & 63;
  const int ui = ( int ) blockIdx.x * 4 + wave;
  if( ui >= a.nUnits ) return;
  const AffUnit u = a.units[ui];
  if( u.nSub == 0 ) return;
  const int quad = lane >> 2, t = quad >> u.log2Sb, s = quad & ( ( 1 << u.log2Sb ) - 1 );
  AffLane L;
  L.on = t < u.nSub;
  L.r = lane & 3;
  L.tmp = sAff + ( wave * 16 + quad ) * AFF_TMP_QUAD;
  const AffSub sb = a.subs[u.firstSub + ( L.on ? t : 0 )];
  const AffDev it = a.items[sb.item];
  L.ref[0] = it.ref[0]; L.ref[1] = it.ref[1]; L.stride[0] = it.stride[0]; L.stride[1] = it.stride[1];
#pragma unroll
  for( int l = 0; l < 2; l++ )
#pragma unroll
    for( int k = 0; k < 3; k++ ) { L.cp[l][k][0] = it.cpmv[l][k][0]; L.cp[l][k][1] = it.cpmv[l][k][1]; }
  L.cuX = it.cuX; L.cuY = it.cuY; L.log2W = it.log2W; L.log2H = it.log2H; L.six = it.six; L.prof = it.prof;
  L.sx = sb.x0 + 4 * ( s & ( ( 1 << u.log2SbW ) - 1 ) ); L.sy = sb.y0 + 4 * ( s >> u.log2SbW );
  const int bw = ( 1 << it.log2W ) >> it.chroma;
  L.dstPitch = a.predStride ? a.predStride : bw;
  L.dst = a.pred + it.dstOff;
  L.org = a.org ? a.org + it.orgOff : nullptr; L.orgPitch = a.orgStride;
  L.res = a.resi ? a.resi + it.dstOff : nullptr;
  if( u.chroma ) affBody<4>( L, a );      // wave-uniform
  else           affBody<6>( L, a );
}

struct AffHead { size_t offItems, offSubs, offUnits; int units; };      // the head of the schedule's blob: where its sections lie, the number of wave units

// validates the list, derives the schedule and uploads it; on success the context's key names the list the device copy belongs to
int affBuildSchedule( vvhip_ctx* ctx, const vvhip_me_plane* planes_host, int n_planes, const vvhip_pred_affine_item* items_host, int n, int pic_width, int pic_height,
                      std::vector<unsigned char>& key )
{
  std::vector<AffDev> dev( n );
  std::vector<ListKeyed> order( n );
  for( int i = 0; i < n; i++ )
  {
    const vvhip_pred_affine_item& it = items_host[i];
    if( !isPow2( it.cu_w ) || !isPow2( it.cu_h ) || it.cu_w < 8 || it.cu_h < 8 || it.cu_w > 128 || it.cu_h > 128 )
      return vvhip_fail( ctx, VVHIP_E_ARG, "vvhip_pred_affine_batch: item %d: CU %dx%d (width and height powers of two, 8..128)", i, it.cu_w, it.cu_h );
    if( it.chroma > 1 || it.six_param > 1 || it.prof > 3 || it.rsv[0] || it.rsv[1] || it.rsv[2] )
      return vvhip_fail( ctx, VVHIP_E_ARG, "vvhip_pred_affine_batch: item %d: chroma %d (0, 1), six_param %d (0, 1), prof %d (0..3) or non-zero reserved bytes", i, it.chroma, it.six_param, it.prof );
    if( it.ref_plane[0] < 0 && it.ref_plane[1] < 0 ) return vvhip_fail( ctx, VVHIP_E_ARG, "vvhip_pred_affine_batch: item %d uses neither reference list", i );
    if( it.cu_x < 0 || it.cu_y < 0 || it.cu_x + it.cu_w > pic_width || it.cu_y + it.cu_h > pic_height )
      return vvhip_fail( ctx, VVHIP_E_ARG, "vvhip_pred_affine_batch: item %d: CU %dx%d at (%d, %d) outside the %dx%d picture", i, it.cu_w, it.cu_h, it.cu_x, it.cu_y, pic_width, pic_height );
    AffDev& d = dev[i];
    memset( &d, 0, sizeof( d ) );
    for( int l = 0; l < 2; l++ )
    {
      if( it.ref_plane[l] < 0 ) continue;
      if( it.ref_plane[l] >= n_planes || !planes_host[it.ref_plane[l]].d_base )
        return vvhip_fail( ctx, VVHIP_E_ARG, "vvhip_pred_affine_batch: item %d: list %d names plane %d of a table of %d", i, l, it.ref_plane[l], n_planes );
      for( int k = 0; k < 3; k++ ) for( int c = 0; c < 2; c++ )
      {
        if( it.cpmv[l][k][c] < -( 1 << 17 ) || it.cpmv[l][k][c] >= ( 1 << 17 ) )
          return vvhip_fail( ctx, VVHIP_E_ARG, "vvhip_pred_affine_batch: item %d: list %d control point %d component %d = %d outside the 18-bit vector range", i, l, k, c, it.cpmv[l][k][c] );
        d.cpmv[l][k][c] = it.cpmv[l][k][c];
      }
      d.ref[l] = planes_host[it.ref_plane[l]].d_base + it.ref_off[l];
      d.stride[l] = planes_host[it.ref_plane[l]].stride;
    }
    d.dstOff = it.dst_off; d.orgOff = it.org_off; d.cuX = it.cu_x; d.cuY = it.cu_y; d.log2W = ( uint8_t ) ilog2i( it.cu_w ); d.log2H = ( uint8_t ) ilog2i( it.cu_h );
    d.chroma = it.chroma; d.six = it.six_param; d.prof = it.chroma ? 0 : it.prof;
    // class: the tile shape (blocks with the most sub-blocks first), component, uni / bi, PROF asked for — a wave never mixes classes; inside a class picture order
    const bool bi = it.ref_plane[0] >= 0 && it.ref_plane[1] >= 0;
    const int sbW = std::min( ( it.cu_w >> it.chroma ) / 4, 4 ), sbH = std::min( ( it.cu_h >> it.chroma ) / 4, 16 / sbW );
    order[i].cls = ( ( uint32_t ) ( 4 - ilog2i( sbW * sbH ) ) << 8 ) | ( ( uint32_t ) ilog2i( sbW ) << 4 ) | ( it.chroma ? 4u : 0u ) | ( d.prof ? 2u : 0u ) | ( bi ? 1u : 0u );
    order[i].pos = ( ( int64_t ) it.cu_y << 20 ) | ( uint32_t ) it.cu_x;
    order[i].idx = i;
  }
  std::sort( order.begin(), order.end() );

  // ---- schedule: per class the tiles in picture order, sixteen sub-blocks per wave, four waves per workgroup, workgroups dealt to the XCDs in bands
  std::vector<AffSub> subs;
  std::vector<AffUnit> units;
  for( int c0 = 0; c0 < n; )
  {
    int c1 = c0; while( c1 < n && order[c1].cls == order[c0].cls ) c1++;
    const int log2SbW = ( int ) ( order[c0].cls >> 4 ) & 15, log2Sb = 4 - ( int ) ( order[c0].cls >> 8 ), chroma = ( order[c0].cls >> 2 ) & 1;
    const int tw = 4 << log2SbW, th = 4 << ( log2Sb - log2SbW ), subsPerWave = 16 >> log2Sb;
    const size_t firstSub = subs.size();
    for( int k = c0; k < c1; k++ )
    {
      const vvhip_pred_affine_item& f = items_host[order[k].idx];
      const int bw = f.cu_w >> chroma, bh = f.cu_h >> chroma;
      for( int y0 = 0; y0 < bh; y0 += th ) for( int x0 = 0; x0 < bw; x0 += tw ) subs.push_back( AffSub{ order[k].idx, ( int16_t ) x0, ( int16_t ) y0 } );
    }
    const int nSubs = ( int ) ( subs.size() - firstSub ), nWaves = ( nSubs + subsPerWave - 1 ) / subsPerWave, nWg = ( nWaves + 3 ) / 4;
    const std::vector<int> perm = predBandOrder( nWg, ( int ) ( units.size() / 4 ) );
    for( int l = 0; l < nWg; l++ ) for( int wv = 0; wv < 4; wv++ )
    {
      const int q = perm[l] * 4 + wv;
      AffUnit u; memset( &u, 0, sizeof( u ) );
      u.log2Sb = ( uint8_t ) log2Sb; u.log2SbW = ( uint8_t ) log2SbW; u.chroma = ( uint8_t ) chroma;
      if( q < nWaves ) { u.firstSub = ( int32_t ) ( firstSub + ( size_t ) q * subsPerWave ); u.nSub = ( int16_t ) std::min( subsPerWave, nSubs - q * subsPerWave ); }
      units.push_back( u );
    }
    c0 = c1;
  }

  // ---- the blob: head, items, tiles, units.  A slot of its own: the schedules of vvhip_pred_inter_batch on the same context are not touched
  AffHead H;
  ListBlob blob( &H, sizeof( H ) );
  H.offItems = blob.add( dev.data(), dev.size() * sizeof( AffDev ) );
  H.offSubs = blob.add( subs.data(), subs.size() * sizeof( AffSub ) );
  H.offUnits = blob.add( units.data(), units.size() * sizeof( AffUnit ) );
  H.units = ( int ) units.size();
  return listUpload( ctx, ctx->list[LIST_AFFINE], blob, &key );
}

} // namespace

extern "C" {

int vvhip_pred_affine_batch( vvhip_ctx* ctx, const vvhip_me_plane* planes_host, int n_planes, const vvhip_pred_affine_item* items_host, int n,
                             int pic_width, int pic_height, int ctu_size, int bit_depth,
                             int16_t* d_pred, int pred_stride, const int16_t* d_org, int org_stride, int16_t* d_resi )
{
  if( !ctx ) return VVHIP_E_ARG;
  if( !planes_host || n_planes < 1 || n_planes > 16 || n < 0 || n > ( 1 << 24 ) || bit_depth < 8 || bit_depth > 12 || pred_stride < 0 || ( n && ( !items_host || !d_pred ) ) || ( d_resi && !d_org ) )
    return vvhip_fail( ctx, VVHIP_E_ARG, "vvhip_pred_affine_batch: %d planes (1..16), %d items, bitDepth %d, prediction %p pitch %d, original %p, residual %p", n_planes, n, bit_depth,
                       ( void* ) d_pred, pred_stride, ( const void* ) d_org, ( void* ) d_resi );
  if( ( ctu_size != 32 && ctu_size != 64 && ctu_size != 128 ) || pic_width < 8 || pic_height < 8 || pic_width > 16384 || pic_height > 16384 )
    return vvhip_fail( ctx, VVHIP_E_ARG, "vvhip_pred_affine_batch: CTU size %d (32, 64, 128), picture %dx%d (8..16384)", ctu_size, pic_width, pic_height );
  for( int p = 0; p < n_planes; p++ )
    if( planes_host[p].d_base && ( planes_host[p].stride < 2 || ( planes_host[p].stride & 1 ) ) )
      return vvhip_fail( ctx, VVHIP_E_ARG, "vvhip_pred_affine_batch: plane %d has stride %d (reference planes need an even row pitch in samples)", p, planes_host[p].stride );
  if( n == 0 ) return VVHIP_OK;

  // ---- a list that is run again (same items, same plane table, same picture) is launched at once: no sort, no upload, no allocation, no wait
  const int head[3] = { n_planes, pic_width, pic_height };
  std::vector<unsigned char> key( sizeof( head ) + ( size_t ) n_planes * sizeof( vvhip_me_plane ) + ( size_t ) n * sizeof( vvhip_pred_affine_item ) );
  memcpy( key.data(), head, sizeof( head ) );
  memcpy( key.data() + sizeof( head ), planes_host, ( size_t ) n_planes * sizeof( vvhip_me_plane ) );
  memcpy( key.data() + sizeof( head ) + ( size_t ) n_planes * sizeof( vvhip_me_plane ), items_host, ( size_t ) n * sizeof( vvhip_pred_affine_item ) );
  HostList& S = ctx->list[LIST_AFFINE];
  bool current = false;
  int rc = listCurrent( ctx, S, key, &current );
  if( rc == VVHIP_OK && !current ) rc = affBuildSchedule( ctx, planes_host, n_planes, items_host, n, pic_width, pic_height, key );
  if( rc ) return rc;
  const AffHead& H = listHead<AffHead>( S );
  const char* base = static_cast<const char*>( S.d );
  AffArgs a;
  a.items = reinterpret_cast<const AffDev*>( base + H.offItems ); a.subs = reinterpret_cast<const AffSub*>( base + H.offSubs ); a.units = reinterpret_cast<const AffUnit*>( base + H.offUnits );
  a.nUnits = H.units; a.bitDepth = bit_depth; a.picW = pic_width; a.picH = pic_height; a.ctu = ctu_size;
  a.pred = d_pred; a.predStride = pred_stride; a.org = d_resi ? d_org : nullptr; a.orgStride = org_stride; a.resi = d_resi;
  hipLaunchKernelGGL( predAffineKernel, dim3( ( unsigned ) ( a.nUnits / 4 ) ), dim3( 256 ), 0, ctx->stream, a );
  VVHIP_LAUNCH_CHECK( ctx );
  return listLaunched( ctx, S );
}

} // extern "C"
