// intra.hip — intra luma mode pre-selection of a list of blocks (gfx950): predict every requested mode of a block from one set of reference lines and score it against the
// original with HAD_2SAD, in the kernel that makes the prediction.
//
// Restates, per requested mode, the arithmetic of IntraSearch::xEstimateLumaRdModeList's decision-free loop (EncoderLib/IntraSearch.cpp:171-335):
//   IntraPrediction::initPredIntraParams   CommonLib/IntraPrediction.cpp:409-496   (non-ISP, non-MIP, non-BDPCM luma block; getWideAngle :335-351)
//   xFilterReferenceSamples                :994-1030                                ([1 2 1], once per item)
//   predIntraAng                           :353-383                                 (xPredIntraPlanar_Core :79-135, xGetPredValDc :302-333, IntraPredSampleFilter_Core :137-157)
//   xPredIntraAng                          :518-681                                 (IntraHorVerPDPC_Core :159-175, IntraAnglePDPC_Core :176-189, IntraPredAngleLuma_Core :191-223)
//   RdCost::xGetHAD2SADs                   CommonLib/RdCost.cpp:1768-1816           (tiles and normalisations: hadtile.h)
//
// One workgroup of four waves per item.  The unfiltered and the filtered lines, the original block and one 8-byte parameter record per requested mode live in LDS.  The
// reference forms a prediction row by row from an extended copy of the main reference (projected side samples in front for negative angles, the last sample replicated behind);
// here a sample is a function of ( mode, x, y ): an index below the main reference's start is answered from the side reference with the projection's own expression, an index
// beyond its end with the last sample.  So any lane can form any sample, and the lanes are laid out for the Hadamard teams: a slot is ( mode, tile, team lane ), a lane forms
// the 8 samples its team position transforms (16 for the 4x4 block), subtracts them from the original in LDS and the team scores the tile.  Slots run mode-major over the four
// waves: large blocks spread one mode over several waves, small blocks put several modes into one wave.  Tile sums and SADs are added per mode with integer LDS atomics
// (they commute: results do not depend on the schedule); a prediction reaches HBM only for pred_mask bits.
#include <string.h>
#include "common.h"
#include "hadtile.h"

namespace {

constexpr int IN_THREADS = 256, IN_MODES = 67, IN_LINE = 136;      // a line: 2 * 64 + 1 + 2 samples, rounded up
constexpr int F_VER = 1, F_FILT = 2, F_CUBIC = 4, F_PDPC = 8, F_PRED = 16;

struct IntraMode { int16_t angle, inv; uint8_t mode, flags; int8_t scale; uint8_t predRank; };      // scale: the PDPC scale of the mode (angular scale, or the H / V scale)
static_assert( sizeof( IntraMode ) == 8, "IntraMode layout" );

struct IntraLds
{
  int16_t   lineU[2][IN_LINE], lineF[2][IN_LINE];      // [0] top row, [1] left row, each from the corner
  int16_t   org[64 * 64];
  IntraMode mp[IN_MODES];
  uint32_t  acc[IN_MODES][2];                          // per requested mode: Hadamard sum, SAD
  uint32_t  cubic[32];                                 // four signed bytes per fraction
  int       dc;
};

__device__ const int16_t kAngTable[32]    = { 0, 1, 2, 3, 4, 6, 8, 10, 12, 14, 16, 18, 20, 23, 26, 29, 32, 35, 39, 45, 51, 57, 64, 73, 86, 102, 128, 171, 256, 341, 512, 1024 };
__device__ const int16_t kInvAngTable[32] = { 0, 16384, 8192, 5461, 4096, 2731, 2048, 1638, 1365, 1170, 1024, 910, 819, 712, 630, 565, 512, 468, 420, 364, 321, 287, 256, 224, 191, 161, 128, 96, 64, 48, 32, 16 };
__device__ const uint8_t kIntraFilter[8]  = { 24, 24, 24, 14, 2, 0, 0, 0 };      // m_aucIntraFilter
__device__ const uint8_t kModeShift[6]    = { 0, 6, 10, 12, 14, 15 };
// the cubic filter by 1/32 fraction (InterpolationFilter::getChromaFilterTable), taps 0..3 in bytes 0..3
#define IN_C4( a, b, c, d ) ( ( uint32_t ) ( uint8_t ) ( int8_t ) ( a ) | ( uint32_t ) ( uint8_t ) ( int8_t ) ( b ) << 8 | ( uint32_t ) ( uint8_t ) ( int8_t ) ( c ) << 16 | ( uint32_t ) ( uint8_t ) ( int8_t ) ( d ) << 24 )
__device__ const uint32_t kCubic[32] = {
  IN_C4( 0, 64, 0, 0 ),    IN_C4( -1, 63, 2, 0 ),   IN_C4( -2, 62, 4, 0 ),   IN_C4( -2, 60, 7, -1 ),  IN_C4( -2, 58, 10, -2 ), IN_C4( -3, 57, 12, -2 ), IN_C4( -4, 56, 14, -2 ), IN_C4( -4, 55, 15, -2 ),
  IN_C4( -4, 54, 16, -2 ), IN_C4( -5, 53, 18, -2 ), IN_C4( -6, 52, 20, -2 ), IN_C4( -6, 49, 24, -3 ), IN_C4( -6, 46, 28, -4 ), IN_C4( -5, 44, 29, -4 ), IN_C4( -4, 42, 30, -4 ), IN_C4( -4, 39, 33, -4 ),
  IN_C4( -4, 36, 36, -4 ), IN_C4( -4, 33, 39, -4 ), IN_C4( -4, 30, 42, -4 ), IN_C4( -4, 29, 44, -5 ), IN_C4( -4, 28, 46, -6 ), IN_C4( -3, 24, 49, -6 ), IN_C4( -2, 20, 52, -6 ), IN_C4( -2, 18, 53, -5 ),
  IN_C4( -2, 16, 54, -4 ), IN_C4( -2, 15, 55, -4 ), IN_C4( -2, 14, 56, -4 ), IN_C4( -2, 12, 57, -3 ), IN_C4( -2, 10, 58, -2 ), IN_C4( -1, 7, 60, -2 ),  IN_C4( 0, 4, 62, -2 ),   IN_C4( 0, 2, 63, -1 ) };
#undef IN_C4

__device__ __forceinline__ int flog2( int v ) { return 31 - __builtin_clz( v ); }

// initPredIntraParams for mode `mode` of a w x h luma block with reference line index mri
__device__ __forceinline__ IntraMode intraParams( int w, int h, int mode, int mri )
{
  IntraMode p; p.angle = 0; p.inv = 0; p.mode = ( uint8_t ) mode; p.flags = 0; p.scale = -1; p.predRank = 0;
  int predMode = mode;
  if( mode > 1 )                                                                         // getWideAngle
  {
    const int ds = kModeShift[abs( flog2( w ) - flog2( h ) )];
    if( w > h && mode < 2 + ds )       predMode += 65;
    else if( h > w && mode > 66 - ds ) predMode -= 65;
  }
  const bool ver = predMode >= 34;
  bool pdpc = mri == 0, refFilter = false, interp = false;
  int absAng = 0;
  if( mode > 1 )
  {
    const int am = ver ? predMode - 50 : -( predMode - 18 ), aam = abs( am );
    absAng = kAngTable[aam];
    p.inv = kInvAngTable[aam];
    p.angle = ( int16_t ) ( am < 0 ? -absAng : absAng );
    if( am < 0 ) pdpc = false;
    else if( am > 0 )
    {
      const int sc = min( 2, flog2( ver ? h : w ) - ( flog2( 3 * p.inv - 2 ) - 8 ) );
      p.scale = ( int8_t ) sc;
      pdpc = pdpc && sc >= 0;
    }
    else p.scale = ( int8_t ) ( ( flog2( w ) + flog2( h ) - 2 ) >> 2 );                  // pure horizontal / vertical: the scale IntraHorVerPDPC is called with
  }
  if( mri || mode == 1 ) {}
  else if( mode == 0 ) refFilter = w * h > 32;
  else
  {
    const int diff = min( abs( predMode - 18 ), abs( predMode - 50 ) );
    if( diff > kIntraFilter[( flog2( w ) + flog2( h ) ) >> 1] ) { const bool integer = ( absAng & 31 ) == 0; refFilter = integer; interp = !integer; }
  }
  p.flags = ( uint8_t ) ( ( ver ? F_VER : 0 ) | ( refFilter ? F_FILT : 0 ) | ( interp ? 0 : F_CUBIC ) | ( pdpc ? F_PDPC : 0 ) );
  return p;
}

struct IntraGeo { int w, h, lw, lh, mri, vmax; };

__device__ __forceinline__ int clipS( int v, int vmax ) { return min( max( v, 0 ), vmax ); }

// IntraPredSampleFilter_Core on one sample
__device__ __forceinline__ int sampleFilter( int v, int top, int left, int x, int y, int scale )
{
  const int wT = 32 >> min( 31, ( y << 1 ) >> scale ), wL = 32 >> min( 31, ( x << 1 ) >> scale );
  return v + ( ( wL * ( left - v ) + wT * ( top - v ) + 32 ) >> 6 );
}

// sample ( x, y ) of the prediction of mode record p
__device__ __forceinline__ int intraSample( const IntraLds& L, const IntraGeo& g, const IntraMode p, int x, int y )
{
  const int16_t* top  = ( p.flags & F_FILT ) ? L.lineF[0] : L.lineU[0];
  const int16_t* left = ( p.flags & F_FILT ) ? L.lineF[1] : L.lineU[1];
  if( p.mode == 0 )
  {
    const int t = top[1 + x], l = left[1 + y], tr = top[g.w + 1], bl = left[g.h + 1];
    const int hor = ( l << g.lw ) + ( x + 1 ) * ( tr - l ), ver = ( t << g.lh ) + ( y + 1 ) * ( bl - t );
    const int v = ( ( hor << g.lh ) + ( ver << g.lw ) + ( 1 << ( g.lw + g.lh ) ) ) >> ( 1 + g.lw + g.lh );
    return sampleFilter( v, t, l, x, y, ( g.lw + g.lh - 2 ) >> 2 );                      // (planar is formed only with reference line 0: PDPC always applies)
  }
  if( p.mode == 1 )
    return ( p.flags & F_PDPC ) ? sampleFilter( L.dc, top[1 + x], left[1 + y], x, y, ( g.lw + g.lh - 2 ) >> 2 ) : L.dc;
  const bool ver = p.flags & F_VER;
  const int xx = ver ? x : y, yy = ver ? y : x, W = ver ? g.w : g.h, H = ver ? g.h : g.w;      // the block as the main direction sees it
  const int16_t* mainL = ver ? top : left;
  const int16_t* sideL = ver ? left : top;
  const int mainLast = 2 * W + g.mri, sideLast = 2 * H + g.mri, angle = p.angle, inv = p.inv;
  // refMain[i] / refSide[j] behind the reference's "compensate for line offset" (:585-586)
  auto M = [&]( int i ) -> int { const int k = i + g.mri; return k < 0 ? ( int ) sideL[min( ( -k * inv + 256 ) >> 9, H )] : ( int ) mainL[min( k, mainLast )]; };
  auto S = [&]( int j ) -> int { return sideL[min( j + g.mri, sideLast )]; };
  int v;
  if( angle == 0 )
  {
    v = M( 1 + xx );
    if( ( p.flags & F_PDPC ) && xx < min( 3 << p.scale, W ) ) v = clipS( v + ( ( ( 32 >> ( ( 2 * xx ) >> p.scale ) ) * ( S( 1 + yy ) - M( 0 ) ) + 32 ) >> 6 ), g.vmax );
    return v;
  }
  const int dpos = angle * ( 1 + g.mri + yy ), dint = dpos >> 5, fr = dpos & 31;
  if( ( abs( angle ) & 31 ) == 0 ) v = M( dint + 1 + xx );
  else
  {
    const int p0 = M( dint + xx ), p1 = M( dint + xx + 1 ), p2 = M( dint + xx + 2 ), p3 = M( dint + xx + 3 );
    if( p.flags & F_CUBIC )
    {
      const uint32_t c = L.cubic[fr];
      v = clipS( ( ( int ) ( int8_t ) c * p0 + ( int ) ( int8_t ) ( c >> 8 ) * p1 + ( int ) ( int8_t ) ( c >> 16 ) * p2 + ( ( int ) c >> 24 ) * p3 + 32 ) >> 6, g.vmax );
    }
    else
    {
      const int hf = fr >> 1;
      v = ( ( 16 - hf ) * p0 + ( 32 - hf ) * p1 + ( 16 + hf ) * p2 + hf * p3 + 32 ) >> 6;
    }
  }
  if( ( p.flags & F_PDPC ) && xx < min( 3 << p.scale, W ) )
  {
    const int lft = S( yy + ( ( 256 + inv * ( xx + 1 ) ) >> 9 ) + 1 );
    v += ( ( 32 >> ( ( 2 * xx ) >> p.scale ) ) * ( lft - v ) + 32 ) >> 6;
  }
  return v;
}

__global__ void __launch_bounds__( IN_THREADS )
intraModesKernel( const vvhip_intra_item* __restrict__ items, const int16_t* __restrict__ ref, const int16_t* __restrict__ org, int16_t* __restrict__ pred, uint32_t* __restrict__ cost )
{
  __shared__ IntraLds L;
  const int tid = threadIdx.x, lane = tid & 63;
  const vvhip_intra_item it = items[blockIdx.x];
  IntraGeo g; g.w = it.w; g.h = it.h; g.lw = flog2( g.w ); g.lh = flog2( g.h ); g.mri = it.multi_ref_idx; g.vmax = ( 1 << it.bit_depth ) - 1;
  const int nt = 2 * g.w + 1 + g.mri, nl = 2 * g.h + 1 + g.mri, nSamples = g.w * g.h;
  const int nModes = __builtin_popcount( it.mode_mask[0] ) + __builtin_popcount( it.mode_mask[1] ) + __builtin_popcount( it.mode_mask[2] );
  if( nModes == 0 ) return;

  // ---- the lines, the original, the tables ----
  for( int i = tid; i < nt + nl; i += IN_THREADS )
  {
    const int16_t v = ref[( size_t ) it.ref_off + i];
    if( i < nt ) L.lineU[0][i] = v; else L.lineU[1][i - nt] = v;
  }
  for( int i = tid; i < nSamples; i += IN_THREADS ) L.org[i] = org[( size_t ) it.org_off + i];
  if( tid < 32 ) L.cubic[tid] = kCubic[tid];
  if( tid < IN_MODES ) { L.acc[tid][0] = 0; L.acc[tid][1] = 0; }
  __syncthreads();

  // ---- once per item: the [1 2 1] filter (reference line 0 only), the DC value, the mode records ----
  if( g.mri == 0 )
  {
    const int tl = ( L.lineU[0][0] + L.lineU[0][1] + L.lineU[1][0] + L.lineU[1][1] + 2 ) >> 2;
    for( int i = tid; i < nt + nl; i += IN_THREADS )
    {
      const int r = i < nt ? 0 : 1, k = r ? i - nt : i, last = r ? 2 * g.h : 2 * g.w;
      const int16_t* u = L.lineU[r];
      L.lineF[r][k] = ( int16_t ) ( k == 0 ? tl : ( k == last ? ( int ) u[k] : ( u[k - 1] + 2 * u[k] + u[k + 1] + 2 ) >> 2 ) );
    }
  }
  if( tid >= IN_THREADS - 64 )                                                           // the last wave, all of it: xGetPredValDc
  {
    uint32_t s = 0;
    for( int i = lane; i < g.w + g.h; i += 64 )
    {
      const bool inTop = i < g.w;
      const int k = g.mri + 1 + ( inTop ? i : i - g.w );
      if( inTop ? g.w >= g.h : g.w <= g.h ) s += ( uint32_t ) L.lineU[inTop ? 0 : 1][k];
    }
    s = vvhipGroupSum32( s, 64, lane );
    const int den = g.w == g.h ? 2 * g.w : max( g.w, g.h );
    if( lane == 0 ) L.dc = ( int ) ( ( s + ( den >> 1 ) ) >> flog2( den ) );
  }
  const vvhip_intra_item* itp = items + blockIdx.x;                                       // (masks indexed per lane are read through the pointer: no private copy of the record)
  if( tid < IN_MODES && ( ( itp->mode_mask[tid >> 5] >> ( tid & 31 ) ) & 1 ) )
  {
    const int wd = tid >> 5; const uint32_t below = ( 1u << ( tid & 31 ) ) - 1;
    int rank = __builtin_popcount( itp->mode_mask[wd] & below ), prank = __builtin_popcount( itp->pred_mask[wd] & below );
    if( wd > 0 ) { rank += __builtin_popcount( it.mode_mask[0] ); prank += __builtin_popcount( it.pred_mask[0] ); }
    if( wd > 1 ) { rank += __builtin_popcount( it.mode_mask[1] ); prank += __builtin_popcount( it.pred_mask[1] ); }
    IntraMode p = intraParams( g.w, g.h, tid, g.mri );
    if( ( itp->pred_mask[wd] >> ( tid & 31 ) ) & 1 ) p.flags |= F_PRED;
    p.predRank = ( uint8_t ) prank;
    L.mp[rank] = p;
  }
  __syncthreads();

  // ---- the slots ----
  const int kind = hadTileKind( g.w, g.h, false );
  int16_t* predItem = pred + ( size_t ) it.pred_off;
  if( kind == TK_4x4 )                                                                   // (only the 4x4 block: 4 x N and N x 4 blocks use the 4x8 / 8x4 tiles) one lane per mode
  {
    if( tid < nModes )
    {
      const IntraMode p = L.mp[tid];
      int d[16]; uint32_t sad = 0;
#pragma unroll
      for( int i = 0; i < 16; i++ )
      {
        const int v = intraSample( L, g, p, i & 3, i >> 2 );
        if( p.flags & F_PRED ) predItem[p.predRank * 16 + i] = ( int16_t ) v;
        d[i] = L.org[i] - v;
        sad += ( uint32_t ) abs( d[i] );
      }
      L.acc[tid][0] = hadamard4x4( d ); L.acc[tid][1] = sad;
    }
  }
  else
  {
    const int PW = tileW( kind ), PH = tileH( kind ), LT = tileLanes( kind ), log2LT = flog2( LT );
    const int log2TX = g.lw - flog2( PW ), log2Slots = g.lw + g.lh - 3, slots = 1 << log2Slots, total = nModes << log2Slots;
    for( int s0 = 0; s0 < total; s0 += IN_THREADS )
    {
      const int sl = s0 + tid;
      const bool valid = sl < total;                                                     // (teams are whole: total is a multiple of the team size)
      const int sv = valid ? sl : 0, mi = sv >> log2Slots, rem = sv & ( slots - 1 ), t = rem >> log2LT, r = rem & ( LT - 1 );
      const IntraMode p = L.mp[mi];
      const int tx = ( t & ( ( 1 << log2TX ) - 1 ) ) * PW, ty = ( t >> log2TX ) * PH;
      // the lane's 8 samples (table in front of hadTeam, hadtile.h): a row of 8, or rows 2r and 2r + 1 of a 4x8 tile
      const int x0 = tx + ( kind == TK_16x8 ? 8 * ( r >> 3 ) : 0 ), y0 = ty + ( kind == TK_16x8 ? ( r & 7 ) : ( kind == TK_4x8 ? 2 * r : r ) );
      int d[8]; uint32_t sad = 0;
#pragma unroll
      for( int i = 0; i < 8; i++ )
      {
        const int x = x0 + ( kind == TK_4x8 ? ( i & 3 ) : i ), y = y0 + ( kind == TK_4x8 ? ( i >> 2 ) : 0 );
        const int v = intraSample( L, g, p, x, y );
        if( valid && ( p.flags & F_PRED ) ) predItem[( size_t ) p.predRank * nSamples + y * g.w + x] = ( int16_t ) v;
        d[i] = L.org[y * g.w + x] - v;
        sad += ( uint32_t ) abs( d[i] );
      }
      const uint32_t sres = hadTeam( d, r, LT, kind, lane );
      sad = vvhipGroupSum32( sad, LT, lane );
      if( valid && r == 0 ) { atomicAdd( &L.acc[mi][0], sres ); atomicAdd( &L.acc[mi][1], sad ); }
    }
  }
  __syncthreads();
  if( tid < nModes )
  {
    const uint32_t hadSum = L.acc[tid][0], s2 = 2 * L.acc[tid][1];
    cost[( size_t ) it.cost_off + L.mp[tid].mode] = min( hadSum, s2 );
  }
}

} // namespace

extern "C" {

int vvhip_intra_luma_modes_batch( vvhip_ctx* ctx, const vvhip_intra_item* items_host, int n, const int16_t* d_ref, const int16_t* d_org, int16_t* d_pred, uint32_t* d_cost )
{
  if( !ctx ) return VVHIP_E_ARG;
  if( n < 0 || ( n > 0 && ( !items_host || !d_ref || !d_org || !d_cost ) ) )
    return vvhip_fail( ctx, VVHIP_E_ARG, "vvhip_intra_luma_modes_batch: %d items (>= 0), items / d_ref / d_org / d_cost missing", n );
  for( int i = 0; i < n; i++ )
  {
    const vvhip_intra_item& q = items_host[i];
    auto sizeOk = []( int v ) { return v == 4 || v == 8 || v == 16 || v == 32 || v == 64; };
    if( !sizeOk( q.w ) || !sizeOk( q.h ) ) return vvhip_fail( ctx, VVHIP_E_ARG, "vvhip_intra_luma_modes_batch: item %d: %dx%d (sides of 4, 8, 16, 32, 64)", i, q.w, q.h );
    if( q.bit_depth < 8 || q.bit_depth > 12 ) return vvhip_fail( ctx, VVHIP_E_ARG, "vvhip_intra_luma_modes_batch: item %d: bit depth %d (8..12)", i, q.bit_depth );
    if( q.multi_ref_idx > 2 ) return vvhip_fail( ctx, VVHIP_E_ARG, "vvhip_intra_luma_modes_batch: item %d: multi_ref_idx %d (0..2)", i, q.multi_ref_idx );
    if( q.rsv ) return vvhip_fail( ctx, VVHIP_E_ARG, "vvhip_intra_luma_modes_batch: item %d: reserved bytes are not zero", i );
    if( ( q.mode_mask[2] | q.pred_mask[2] ) >> 3 ) return vvhip_fail( ctx, VVHIP_E_ARG, "vvhip_intra_luma_modes_batch: item %d: mask bits beyond mode 66", i );
    if( ( q.pred_mask[0] & ~q.mode_mask[0] ) | ( q.pred_mask[1] & ~q.mode_mask[1] ) | ( q.pred_mask[2] & ~q.mode_mask[2] ) )
      return vvhip_fail( ctx, VVHIP_E_ARG, "vvhip_intra_luma_modes_batch: item %d: pred_mask is not a subset of mode_mask", i );
    if( q.multi_ref_idx && ( q.mode_mask[0] & 1u ) ) return vvhip_fail( ctx, VVHIP_E_ARG, "vvhip_intra_luma_modes_batch: item %d: PLANAR with multi_ref_idx %d (formed with reference line 0 only)", i, q.multi_ref_idx );
    if( q.ref_off < 0 || q.org_off < 0 || q.pred_off < 0 || q.cost_off < 0 )
      return vvhip_fail( ctx, VVHIP_E_ARG, "vvhip_intra_luma_modes_batch: item %d: negative offset (ref %d, org %d, pred %d, cost %d)", i, q.ref_off, q.org_off, q.pred_off, q.cost_off );
    if( !d_pred && ( q.pred_mask[0] | q.pred_mask[1] | q.pred_mask[2] ) ) return vvhip_fail( ctx, VVHIP_E_ARG, "vvhip_intra_luma_modes_batch: item %d asks for predictions, d_pred is missing", i );
  }
  if( n == 0 ) return VVHIP_OK;
  HostList& S = ctx->list[LIST_INTRA];
  const int rc = listUpload( ctx, S, ListBlob( items_host, ( size_t ) n * sizeof( vvhip_intra_item ) ) );
  if( rc != VVHIP_OK ) return rc;
  hipLaunchKernelGGL( intraModesKernel, dim3( ( unsigned ) n ), dim3( IN_THREADS ), 0, ctx->stream, ( const vvhip_intra_item* ) S.d, d_ref, d_org, d_pred, d_cost );
  VVHIP_LAUNCH_CHECK( ctx );
  return listLaunched( ctx, S );
}

} // extern "C"
