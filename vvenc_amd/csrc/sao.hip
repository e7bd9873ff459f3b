// sao.hip — sample adaptive offset (SAO) of a picture: vvhip_sao_stats / vvhip_sao_offset (gfx950 only).
//
// SAO sits between deblocking and ALF in the encoder's per-CTU pipeline.  Its data-parallel parts are two:
//   stats  : EncSampleAdaptiveOffset::getBlkStats (EncoderLib/EncSampleAdaptiveOffset.cpp:810-929) with the five calcSaoStatistics*_Core routines
//            (CommonLib/SampleAdaptiveOffset.cpp:281-399) for every CTU of a band of CTU rows and up to three planes, as getStatistics / getCtuStatistics drive it
//   offset : offsetBlock_core (CommonLib/SampleAdaptiveOffset.cpp:64-280) for every CTU of a band from the decided per-CTU parameters, as offsetCTU drives it
// The reference walks a CTU row by row and carries the signs of the previous row in line buffers; that is only a cache: every counted or filtered sample has
// edgeType = sgn( c - a ) + sgn( c - b ) for its two neighbours a, b along the type's direction, and WHICH samples are counted / filtered is a rectangle of the CTU with
// ranges of their own on the first (and, in the filter, the last) row of the two diagonal types.  Both kernels restate exactly those ranges as predicates per sample.
//
// One workgroup of four waves per ( CTU, plane ).  The CTU's source samples and a one-sample frame around them go to LDS once (zero where the picture ends: no such
// sample is ever used, the ranges exclude it); a lane then walks down one column with the 3 x 3 neighbourhood in registers — three LDS reads per sample feed all five
// types.  Statistics: the 20 edge bins x { diff, count } are per-lane register sums, reduced in the wave (DPP) and across the four waves through LDS; the 32 bands go to
// an LDS histogram with integer LDS adds, a lane adding its run of equal bands at once; wave 0 stores the whole 2560-byte record with plain 8-byte vector stores.
// All sums are integers, so their order is free and every run gives the same bits.  The sums inside the kernel are 32-bit: a CTU has at most 128 x 128 samples and
// | org - src | <= 2^12 - 1, and 128 * 128 * ( 2^12 - 1 ) < 2^26 fits with room to spare; they are widened to the record's int64 at the store.
// No global atomics, no pre-zeroed output, no float, no scratch.
#include "common.h"
#include <algorithm>
#include <string.h>

namespace {

constexpr int SAO_THREADS = 256, SAO_WAVES = SAO_THREADS / 64;
constexpr int SAO_PAD = 4;      // LDS column of sample x is SAO_PAD + x: the left frame column sits at SAO_PAD - 1, and rows of 4 samples stay 8-byte aligned

// statistics flags (vvenc_hip.h: VVHIP_SAO_*)
constexpr int F_L = 1, F_A = 2, F_AL = 4, F_R = 8, F_B = 16, F_AR = 32;
// the reference's availability mask of the filter (CommonLib/SampleAdaptiveOffset.h:75-85)
constexpr int M_L = 1, M_R = 2, M_A = 4, M_B = 8, M_AL = 16, M_AR = 32, M_BL = 64, M_BR = 128;

struct SaoStatsPlaneDev  { const int16_t* org; const int16_t* src; int orgStride, srcStride, width, height, ctuW, ctuH, shift, skipR, skipB, pad; };
struct SaoStatsArgs      { SaoStatsPlaneDev pl[3]; const uint8_t* flags; long long* out; int ctusX, ctusY, ctuRow0, nPlanes; };
struct SaoOffsetPlaneDev { const int16_t* src; int16_t* dst; int srcStride, dstStride, width, height, ctuW, ctuH, shift, clipMin, clipMax, pad; };
struct SaoParamDev       { int8_t type; uint8_t avail, band, pad; int16_t offs[5]; int16_t pad2; };      // 16 bytes
struct SaoOffsetArgs     { SaoOffsetPlaneDev pl[3]; const SaoParamDev* params; int ctusX, ctusY, ctuRow0, nPlanes; };

struct __attribute__( ( aligned( 8 ) ) ) SaoSeg4 { int16_t v[4]; };

// the CTU's w x h samples at ( x0, y0 ) of the plane and the frame of one sample around them -> tile (row r = -1 .. h at ( r + 1 ) * pitch, column c = -1 .. w at SAO_PAD + c);
// positions outside the picture become 0.  Rows of 4 samples with 8-byte loads where the plane's base, its pitch and the CTU width allow, single samples otherwise.
__device__ __forceinline__ void saoLoadTile( int16_t* __restrict__ tile, int pitch, const int16_t* __restrict__ src, int stride, int width, int height, int x0, int y0, int w, int h, int ctuW )
{
  const int tid = threadIdx.x;
  const bool vec = ( ( ( uintptr_t ) src | ( ( uintptr_t ) ( unsigned ) stride * 2u ) ) & 7u ) == 0 && ( ( ctuW | w ) & 3 ) == 0;
  if( vec )
  {
    const int q = tid & 31, segs = w >> 2;
    for( int r = ( tid >> 5 ) - 1; r <= h; r += SAO_THREADS / 32 )
    {
      if( q >= segs ) continue;
      const int y = y0 + r;
      SaoSeg4 s = { { 0, 0, 0, 0 } };
      if( y >= 0 && y < height ) s = *reinterpret_cast<const SaoSeg4*>( src + ( ptrdiff_t ) y * stride + x0 + 4 * q );
      *reinterpret_cast<SaoSeg4*>( tile + ( r + 1 ) * pitch + SAO_PAD + 4 * q ) = s;
    }
    // the two frame columns
    for( int i = tid; i < 2 * ( h + 2 ); i += SAO_THREADS )
    {
      const int r = ( i >> 1 ) - 1, c = ( i & 1 ) ? w : -1, y = y0 + r, x = x0 + c;
      tile[( r + 1 ) * pitch + SAO_PAD + c] = ( y >= 0 && y < height && x >= 0 && x < width ) ? src[( ptrdiff_t ) y * stride + x] : ( int16_t ) 0;
    }
  }
  else
  {
    for( int r = ( tid >> 6 ) - 1; r <= h; r += SAO_WAVES )
    {
      const int y = y0 + r;
      for( int c = ( tid & 63 ) - 1; c <= w; c += 64 )
      {
        const int x = x0 + c;
        tile[( r + 1 ) * pitch + SAO_PAD + c] = ( y >= 0 && y < height && x >= 0 && x < width ) ? src[( ptrdiff_t ) y * stride + x] : ( int16_t ) 0;
      }
    }
  }
}

__device__ __forceinline__ int saoSgn( int c, int v ) { return ( int ) ( c > v ) - ( int ) ( c < v ); }

// ---- statistics ------------------------------------------------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__( SAO_THREADS )
saoStatsKernel( const SaoStatsArgs a )
{
  extern __shared__ int16_t saoTile[];
  __shared__ int bo[2][32];                     // [ diff, count ][ band ]
  __shared__ int part[SAO_WAVES][4][2][5];      // [ wave ][ edge type ][ diff, count ][ class ]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, plane = blockIdx.y;
  const SaoStatsPlaneDev& p = a.pl[plane];
  const int cx = ( int ) blockIdx.x % a.ctusX, cy = a.ctuRow0 + ( int ) blockIdx.x / a.ctusX, ctu = cy * a.ctusX + cx;
  const int x0 = cx * p.ctuW, y0 = cy * p.ctuH, w = min( p.ctuW, p.width - x0 ), h = min( p.ctuH, p.height - y0 ), pitch = p.ctuW + 2 * SAO_PAD;
  // availability: the caller's flags, or the picture's borders alone (getStatistics)
  int fl;
  if( a.flags ) fl = a.flags[ctu - a.ctuRow0 * a.ctusX];
  else
  {
    const bool L = cx > 0, A = cy > 0, R = cx < a.ctusX - 1, B = cy < a.ctusY - 1;
    fl = ( L ? F_L : 0 ) | ( A ? F_A : 0 ) | ( L && A ? F_AL : 0 ) | ( R ? F_R : 0 ) | ( B ? F_B : 0 ) | ( A && R ? F_AR : 0 );
  }
  if( tid < 64 ) ( &bo[0][0] )[tid] = 0;
  saoLoadTile( saoTile, pitch, p.src, p.srcStride, p.width, p.height, x0, y0, w, h, p.ctuW );
  __syncthreads();

  // the ranges of getBlkStats: the right skipR columns and the bottom skipB rows wait for the deblocking of the next CTU where there is one
  const bool L = fl & F_L, A = fl & F_A, AL = fl & F_AL, R = fl & F_R, B = fl & F_B, AR = fl & F_AR;
  const int startX = L ? 0 : 1, endX = R ? w - p.skipR : w - 1, endXFull = R ? w - p.skipR : w;
  const int endYFull = B ? h - p.skipB : h, endY = B ? h - p.skipB : h - 1, startY90 = A ? 0 : 1;
  // a lane walks rows [ yBeg, yEnd ) of column x
  const int groups = SAO_THREADS / w, g = tid / w, x = tid - g * w, rowsPer = ( h + groups - 1 ) / groups;
  const int yBeg = g * rowsPer, yEnd = g < groups ? min( h, yBeg + rowsPer ) : 0;
  const bool xIn = x >= startX && x < endX, xInFull = x < endXFull;
  const bool first135 = x >= ( AL ? 0 : 1 ) && x < ( A ? endX : 1 );
  const bool first45 = x >= ( A ? startX : endX ) && x < ( ( !R && AR ) ? w : endX );

  int dif[4][5], cnt[4][5];
#pragma unroll
  for( int t = 0; t < 4; t++ )
#pragma unroll
    for( int k = 0; k < 5; k++ ) { dif[t][k] = 0; cnt[t][k] = 0; }
  int runBand = 0, runDiff = 0, runCnt = 0;

  if( yBeg < yEnd )
  {
    const int16_t* t = saoTile + ( yBeg + 1 ) * pitch + SAO_PAD + x;
    int a0, a1, a2, b0 = t[-pitch - 1], b1 = t[-pitch], b2 = t[-pitch + 1], c0 = t[-1], c1 = t[0], c2 = t[1];
    const int16_t* o = p.org + ( ptrdiff_t ) ( y0 + yBeg ) * p.orgStride + x0 + x;
    // eight rows at a time: the eight loads of the original are in flight together (one dependent load per row made a lane's walk a chain of memory latencies)
    for( int yb = yBeg; yb < yEnd; yb += 8, o += ( ptrdiff_t ) 8 * p.orgStride )
    {
      int ov[8];
#pragma unroll
      for( int k = 0; k < 8; k++ ) ov[k] = yb + k < yEnd ? ( int ) o[( ptrdiff_t ) k * p.orgStride] : 0;
#pragma unroll
      for( int k = 0; k < 8; k++ )
      {
        const int y = yb + k;
        if( y >= yEnd ) break;
        a0 = b0; a1 = b1; a2 = b2; b0 = c0; b1 = c1; b2 = c2;
        c0 = t[pitch - 1]; c1 = t[pitch]; c2 = t[pitch + 1];
        t += pitch;
        const int c = b1, d = ov[k] - c;
        const int e0 = saoSgn( c, b0 ) + saoSgn( c, b2 ) + 2, e90 = saoSgn( c, a1 ) + saoSgn( c, c1 ) + 2;
        const int e135 = saoSgn( c, a0 ) + saoSgn( c, c2 ) + 2, e45 = saoSgn( c, a2 ) + saoSgn( c, c0 ) + 2;
        const bool mid = y < endY && xIn;
        const bool v0 = xIn && y < endYFull, v90 = xInFull && y >= startY90 && y < endY;
        const bool v135 = y == 0 ? first135 : mid, v45 = y == 0 ? first45 : mid, vBo = xInFull && y < endYFull;
#pragma unroll
        for( int cl = 0; cl < 5; cl++ )
        {
          const bool m0 = v0 && e0 == cl, m1 = v90 && e90 == cl, m2 = v135 && e135 == cl, m3 = v45 && e45 == cl;
          cnt[0][cl] += m0; dif[0][cl] += m0 ? d : 0;
          cnt[1][cl] += m1; dif[1][cl] += m1 ? d : 0;
          cnt[2][cl] += m2; dif[2][cl] += m2 ? d : 0;
          cnt[3][cl] += m3; dif[3][cl] += m3 ? d : 0;
        }
        if( vBo )
        {
          const int band = ( c >> p.shift ) & 31;      // operand contract: 0 <= src < 2^bitDepth; the mask only keeps a violation inside the histogram
          if( band != runBand && runCnt )
          {
            atomicAdd( &bo[0][runBand], runDiff ); atomicAdd( &bo[1][runBand], runCnt );
            runDiff = 0; runCnt = 0;
          }
          runBand = band; runDiff += d; runCnt++;
        }
      }
    }
    if( runCnt ) { atomicAdd( &bo[0][runBand], runDiff ); atomicAdd( &bo[1][runBand], runCnt ); }
  }
  // every lane of every wave arrives here: the DPP sums need the whole wave
#pragma unroll
  for( int t = 0; t < 4; t++ )
#pragma unroll
    for( int k = 0; k < 5; k++ )
    {
      const int sd = ( int ) vvhipGroupSum32( ( uint32_t ) dif[t][k], 64, lane ), sc = ( int ) vvhipGroupSum32( ( uint32_t ) cnt[t][k], 64, lane );
      if( lane == 0 ) { part[wave][t][0][k] = sd; part[wave][t][1][k] = sc; }
    }
  __syncthreads();
  if( wave == 0 )
  {
    long long* rec = a.out + ( ( size_t ) ctu * a.nPlanes + plane ) * 320;
    for( int i = lane; i < 320; i += 64 )
    {
      const int t = i >> 6, which = ( i >> 5 ) & 1, bin = i & 31;
      int v = 0;
      if( t == 4 ) v = bo[which][bin];
      else if( bin < 5 )
      {
#pragma unroll
        for( int wv = 0; wv < SAO_WAVES; wv++ ) v += part[wv][t][which][bin];
      }
      rec[i] = ( long long ) v;
    }
  }
}

// ---- offset filter ---------------------------------------------------------------------------------------------------------------------------------------------------------
// the filtered value of sample ( x, y ) of a CTU of type 0..3; t points at the sample in the tile
__device__ __forceinline__ int saoEdgeSample( const int16_t* __restrict__ t, int pitch, int type, int x, int y, int w, int h, int mask, int o0, int o1, int o2, int o3, int o4, int lo, int hi )
{
  const int c = t[0];
  const int startX = ( mask & M_L ) ? 0 : 1, endX = ( mask & M_R ) ? w : w - 1;
  bool on; int na, nb;
  if( type == 0 )      { on = x >= startX && x < endX; na = t[-1]; nb = t[1]; }
  else if( type == 1 ) { on = y >= ( ( mask & M_A ) ? 0 : 1 ) && y < ( ( mask & M_B ) ? h : h - 1 ); na = t[-pitch]; nb = t[pitch]; }
  else if( type == 2 )
  {
    const int sx = y == 0 ? ( ( mask & M_AL ) ? 0 : 1 ) : y == h - 1 ? ( ( mask & M_B ) ? startX : w - 1 ) : startX;
    const int ex = y == 0 ? ( ( mask & M_A ) ? endX : 1 ) : y == h - 1 ? ( ( mask & M_BR ) ? w : w - 1 ) : endX;
    on = x >= sx && x < ex; na = t[-pitch - 1]; nb = t[pitch + 1];
  }
  else
  {
    const int sx = y == 0 ? ( ( mask & M_A ) ? startX : w - 1 ) : y == h - 1 ? ( ( mask & M_BL ) ? 0 : 1 ) : startX;
    const int ex = y == 0 ? ( ( mask & M_AR ) ? w : w - 1 ) : y == h - 1 ? ( ( mask & M_B ) ? endX : 1 ) : endX;
    on = x >= sx && x < ex; na = t[-pitch + 1]; nb = t[pitch - 1];
  }
  if( !on ) return c;
  const int e = saoSgn( c, na ) + saoSgn( c, nb ) + 2;
  const int off = e == 0 ? o0 : e == 1 ? o1 : e == 2 ? o2 : e == 3 ? o3 : o4;
  return min( max( c + off, lo ), hi );
}

__global__ void __launch_bounds__( SAO_THREADS )
saoOffsetKernel( const SaoOffsetArgs a )
{
  extern __shared__ int16_t saoTile[];
  const int tid = threadIdx.x, plane = blockIdx.y;
  const SaoOffsetPlaneDev& p = a.pl[plane];
  const int cx = ( int ) blockIdx.x % a.ctusX, cy = a.ctuRow0 + ( int ) blockIdx.x / a.ctusX, ctu = cy * a.ctusX + cx;
  const int x0 = cx * p.ctuW, y0 = cy * p.ctuH, w = min( p.ctuW, p.width - x0 ), h = min( p.ctuH, p.height - y0 ), pitch = p.ctuW + 2 * SAO_PAD;
  const SaoParamDev prm = a.params[( size_t ) ( ctu - a.ctuRow0 * a.ctusX ) * a.nPlanes + plane];      // the band's records
  const int type = prm.type, mask = prm.avail, band = prm.band, lo = p.clipMin, hi = p.clipMax;
  const int o0 = prm.offs[0], o1 = prm.offs[1], o2 = prm.offs[2], o3 = prm.offs[3], o4 = prm.offs[4];
  saoLoadTile( saoTile, pitch, p.src, p.srcStride, p.width, p.height, x0, y0, w, h, p.ctuW );
  __syncthreads();
  int16_t* dst = p.dst + ( ptrdiff_t ) y0 * p.dstStride + x0;
  const bool vec = ( ( ( uintptr_t ) p.dst | ( ( uintptr_t ) ( unsigned ) p.dstStride * 2u ) ) & 7u ) == 0 && ( ( p.ctuW | w ) & 3 ) == 0;
  const int step = vec ? 4 : 1, perRow = vec ? 32 : 64, xi = ( tid & ( perRow - 1 ) ) * step;
  for( int y = tid / perRow; y < h; y += SAO_THREADS / perRow )
    for( int x = xi; x < w; x += perRow * step )
    {
      const int16_t* t = saoTile + ( y + 1 ) * pitch + SAO_PAD + x;
      SaoSeg4 r = { { 0, 0, 0, 0 } };
#pragma unroll
      for( int k = 0; k < 4; k++ )
        if( k < step )
        {
          const int c = t[k];
          int v = c;
          if( type == 4 )
          {
            const int i = ( ( c >> p.shift ) - band ) & 31;      // operand contract: 0 <= src < 2^bitDepth
            v = min( max( c + ( i == 0 ? o0 : i == 1 ? o1 : i == 2 ? o2 : i == 3 ? o3 : 0 ), lo ), hi );
          }
          else if( type >= 0 ) v = saoEdgeSample( t + k, pitch, type, x + k, y, w, h, mask, o0, o1, o2, o3, o4, lo, hi );
          r.v[k] = ( int16_t ) v;
        }
      if( vec ) *reinterpret_cast<SaoSeg4*>( dst + ( ptrdiff_t ) y * p.dstStride + x ) = r;
      else dst[( ptrdiff_t ) y * p.dstStride + x] = r.v[0];
    }
}

// the geometry rules both entries share; -> the CTU grid
bool saoGrid( int width, int height, int ctuW, int ctuH, int stride, int* ctusX, int* ctusY )
{
  if( width < 2 || height < 2 || ctuW < 8 || ctuW > 128 || ctuH < 8 || ctuH > 128 || stride < width ) return false;
  // a last CTU column / row of one sample has no second row for the diagonal types (the reference reads past its block there)
  if( width % ctuW == 1 || height % ctuH == 1 ) return false;
  *ctusX = ( width + ctuW - 1 ) / ctuW; *ctusY = ( height + ctuH - 1 ) / ctuH;
  return true;
}

} // namespace

extern "C" {

int vvhip_sao_stats( vvhip_ctx* ctx, const vvhip_sao_stats_plane* planes, int n_planes, int ctu_row0, int n_rows, const uint8_t* flags_host, int64_t* d_out )
{
  if( !ctx ) return VVHIP_E_ARG;
  if( !planes || n_planes < 1 || n_planes > 3 || !d_out ) return vvhip_fail( ctx, VVHIP_E_ARG, "vvhip_sao_stats: %d planes (1..3), planes / d_out missing", n_planes );
  SaoStatsArgs A;
  memset( &A, 0, sizeof( A ) );
  int maxW = 0, maxH = 0;
  for( int c = 0; c < n_planes; c++ )
  {
    const vvhip_sao_stats_plane& q = planes[c];
    int gx = 0, gy = 0;
    if( !q.d_org || !q.d_src || q.org_stride < q.width || q.bit_depth < 8 || q.bit_depth > 12 || !saoGrid( q.width, q.height, q.ctu_w, q.ctu_h, q.src_stride, &gx, &gy ) )
      return vvhip_fail( ctx, VVHIP_E_ARG, "vvhip_sao_stats: plane %d: %dx%d, CTU %dx%d (8..128, no last column / row of one sample), strides %d / %d, bitDepth %d (8..12)", c, q.width, q.height,
                         q.ctu_w, q.ctu_h, q.org_stride, q.src_stride, q.bit_depth );
    if( c && ( gx != A.ctusX || gy != A.ctusY ) )
      return vvhip_fail( ctx, VVHIP_E_ARG, "vvhip_sao_stats: plane %d has a CTU grid of %dx%d, plane 0 one of %dx%d", c, gx, gy, A.ctusX, A.ctusY );
    A.ctusX = gx; A.ctusY = gy;
    SaoStatsPlaneDev& p = A.pl[c];
    p.org = q.d_org; p.src = q.d_src; p.orgStride = q.org_stride; p.srcStride = q.src_stride; p.width = q.width; p.height = q.height; p.ctuW = q.ctu_w; p.ctuH = q.ctu_h;
    p.shift = q.bit_depth - 5; p.skipR = q.is_luma ? 5 : 3; p.skipB = q.is_luma ? 4 : 2;
    maxW = std::max( maxW, q.ctu_w ); maxH = std::max( maxH, q.ctu_h );
  }
  if( ctu_row0 < 0 || n_rows < 1 || ctu_row0 > A.ctusY - n_rows )
    return vvhip_fail( ctx, VVHIP_E_ARG, "vvhip_sao_stats: CTU rows [%d, %d + %d) of %d", ctu_row0, ctu_row0, n_rows, A.ctusY );
  const int nCtus = n_rows * A.ctusX;
  if( flags_host )
  {
    const uint8_t* f = flags_host + ( size_t ) ctu_row0 * A.ctusX;
    for( int i = 0; i < nCtus; i++ )
    {
      const int cx = i % A.ctusX, cy = ctu_row0 + i / A.ctusX;
      const bool L = cx > 0, T = cy > 0, R = cx < A.ctusX - 1, B = cy < A.ctusY - 1;
      const int can = ( L ? F_L : 0 ) | ( T ? F_A : 0 ) | ( L && T ? F_AL : 0 ) | ( R ? F_R : 0 ) | ( B ? F_B : 0 ) | ( T && R ? F_AR : 0 );
      if( f[i] & ~can ) return vvhip_fail( ctx, VVHIP_E_ARG, "vvhip_sao_stats: CTU (%d, %d): flags 0x%02x name a neighbour outside the picture (possible 0x%02x)", cx, cy, f[i], can );
    }
    const int rc = listUpload( ctx, ctx->list[LIST_SAO_FLAGS], ListBlob( f, ( size_t ) nCtus ) );
    if( rc != VVHIP_OK ) return rc;
    A.flags = ( const uint8_t* ) ctx->list[LIST_SAO_FLAGS].d;
  }
  A.out = ( long long* ) d_out; A.ctuRow0 = ctu_row0; A.nPlanes = n_planes;
  const size_t lds = ( size_t ) ( maxH + 2 ) * ( maxW + 2 * SAO_PAD ) * sizeof( int16_t );
  hipLaunchKernelGGL( saoStatsKernel, dim3( nCtus, n_planes ), dim3( SAO_THREADS ), lds, ctx->stream, A );
  VVHIP_LAUNCH_CHECK( ctx );
  return flags_host ? listLaunched( ctx, ctx->list[LIST_SAO_FLAGS] ) : VVHIP_OK;
}

int vvhip_sao_offset( vvhip_ctx* ctx, const vvhip_sao_offset_plane* planes, int n_planes, const vvhip_sao_param* params_host, int ctu_row0, int n_rows )
{
  if( !ctx ) return VVHIP_E_ARG;
  if( !planes || n_planes < 1 || n_planes > 3 || !params_host ) return vvhip_fail( ctx, VVHIP_E_ARG, "vvhip_sao_offset: %d planes (1..3), planes / params missing", n_planes );
  SaoOffsetArgs A;
  memset( &A, 0, sizeof( A ) );
  int maxW = 0, maxH = 0;
  for( int c = 0; c < n_planes; c++ )
  {
    const vvhip_sao_offset_plane& q = planes[c];
    int gx = 0, gy = 0;
    if( !q.d_src || !q.d_dst || q.dst_stride < q.width || q.bit_depth < 8 || q.bit_depth > 12 || q.clip_min > q.clip_max || q.clip_min < -32768 || q.clip_max > 32767 ||
        !saoGrid( q.width, q.height, q.ctu_w, q.ctu_h, q.src_stride, &gx, &gy ) )
      return vvhip_fail( ctx, VVHIP_E_ARG, "vvhip_sao_offset: plane %d: %dx%d, CTU %dx%d (8..128, no last column / row of one sample), strides %d / %d, bitDepth %d (8..12), clip [%d, %d]", c, q.width,
                         q.height, q.ctu_w, q.ctu_h, q.src_stride, q.dst_stride, q.bit_depth, q.clip_min, q.clip_max );
    if( c && ( gx != A.ctusX || gy != A.ctusY ) )
      return vvhip_fail( ctx, VVHIP_E_ARG, "vvhip_sao_offset: plane %d has a CTU grid of %dx%d, plane 0 one of %dx%d", c, gx, gy, A.ctusX, A.ctusY );
    A.ctusX = gx; A.ctusY = gy;
    SaoOffsetPlaneDev& p = A.pl[c];
    p.src = q.d_src; p.dst = q.d_dst; p.srcStride = q.src_stride; p.dstStride = q.dst_stride; p.width = q.width; p.height = q.height; p.ctuW = q.ctu_w; p.ctuH = q.ctu_h;
    p.shift = q.bit_depth - 5; p.clipMin = q.clip_min; p.clipMax = q.clip_max;
    maxW = std::max( maxW, q.ctu_w ); maxH = std::max( maxH, q.ctu_h );
  }
  // no source plane may overlap a destination plane
  for( int s = 0; s < n_planes; s++ )
    for( int d = 0; d < n_planes; d++ )
    {
      const int16_t* sb = planes[s].d_src; const int16_t* se = sb + ( size_t ) ( planes[s].height - 1 ) * planes[s].src_stride + planes[s].width;
      const int16_t* db = planes[d].d_dst; const int16_t* de = db + ( size_t ) ( planes[d].height - 1 ) * planes[d].dst_stride + planes[d].width;
      if( ( uintptr_t ) sb < ( uintptr_t ) de && ( uintptr_t ) db < ( uintptr_t ) se )
        return vvhip_fail( ctx, VVHIP_E_ARG, "vvhip_sao_offset: the source of plane %d overlaps the destination of plane %d", s, d );
    }
  if( ctu_row0 < 0 || n_rows < 1 || ctu_row0 > A.ctusY - n_rows )
    return vvhip_fail( ctx, VVHIP_E_ARG, "vvhip_sao_offset: CTU rows [%d, %d + %d) of %d", ctu_row0, ctu_row0, n_rows, A.ctusY );
  const int nCtus = n_rows * A.ctusX;
  std::vector<SaoParamDev> dev( ( size_t ) nCtus * n_planes );
  for( int i = 0; i < nCtus; i++ )
  {
    const int cx = i % A.ctusX, cy = ctu_row0 + i / A.ctusX;
    const bool L = cx > 0, T = cy > 0, R = cx < A.ctusX - 1, B = cy < A.ctusY - 1;
    const int can = ( L ? M_L : 0 ) | ( R ? M_R : 0 ) | ( T ? M_A : 0 ) | ( B ? M_B : 0 ) | ( L && T ? M_AL : 0 ) | ( R && T ? M_AR : 0 ) | ( L && B ? M_BL : 0 ) | ( R && B ? M_BR : 0 );
    for( int c = 0; c < n_planes; c++ )
    {
      const vvhip_sao_param& q = params_host[( ( size_t ) ctu_row0 * A.ctusX + i ) * n_planes + c];
      if( q.type < -1 || q.type > 4 || q.band > 31 || q.rsv || ( q.type >= 0 && ( q.avail & ~can ) ) )
        return vvhip_fail( ctx, VVHIP_E_ARG, "vvhip_sao_offset: CTU (%d, %d) plane %d: type %d (-1..4), band %d (0..31), availability 0x%02x (possible 0x%02x)", cx, cy, c, q.type, q.band, q.avail, can );
      SaoParamDev& o = dev[( size_t ) i * n_planes + c];
      o.type = q.type; o.avail = q.avail; o.band = q.band; o.pad = 0; o.pad2 = 0;
      for( int k = 0; k < 5; k++ ) o.offs[k] = q.offs[k];
    }
  }
  const int rc = listUpload( ctx, ctx->list[LIST_SAO_PARAMS], ListBlob( dev.data(), dev.size() * sizeof( SaoParamDev ) ) );
  if( rc != VVHIP_OK ) return rc;
  A.params = ( const SaoParamDev* ) ctx->list[LIST_SAO_PARAMS].d;
  A.ctuRow0 = ctu_row0; A.nPlanes = n_planes;
  const size_t lds = ( size_t ) ( maxH + 2 ) * ( maxW + 2 * SAO_PAD ) * sizeof( int16_t );
  hipLaunchKernelGGL( saoOffsetKernel, dim3( nCtus, n_planes ), dim3( SAO_THREADS ), lds, ctx->stream, A );
  VVHIP_LAUNCH_CHECK( ctx );
  return listLaunched( ctx, ctx->list[LIST_SAO_PARAMS] );
}

} // extern "C"
