// visact.hip — the visual activity of a picture for perceptual QP adaptation (QPA): vvhip_visact (gfx950 only).
//
// BitAllocation::applyQPAdaptationSlice (EncoderLib/BitAllocation.cpp:508-810) measures, serially at slice initialisation, the visual activity of every CTU of the ORIGINAL
// picture and of the whole chroma planes; PreProcess::xGetVisualActivity (EncoderLib/PreProcess.cpp:312-427) does the same on whole planes.  The data-parallel part is six
// entries of g_pelBufOP (CommonLib/Buffer.cpp:323-435) under calcSpatialVisAct / calcTemporalVisAct (BitAllocation.cpp:84-195) and the sample sum of AreaBuf::getAvg
// (CommonLib/Buffer.h:303-315):
//   spatial   HD: AvgHighPass                  | 12 c - 2 ( l + r + u + d ) - ( ul + ur + dl + dr ) | at 1 <= x <= w - 2, 1 <= y <= h - 2
//             ds: AvgHighPassWithDownsampling  the 6 x 6 kernel around the 2 x 2 cells at even x, y in 2 <= x < w - 2, 2 <= y < h - 2
//   temporal  HD: HDHighPass / HDHighPass2     ( 1 + 3 | c - p1 | ) >> 1  /  | c - 2 p1 + p2 |  at the same positions
//             ds: ...Diff1st / ...Diff2nd      the same on the 2 x 2 cell sums
// Both spatial kernels separate into row sums: HD  s = Q( y ) - P( y - 1 ) - P( y + 1 ) with P = l + 2 c + r, Q = 12 c - 2 ( l + r );
//                                              ds  f = C( y ) + C( y + 1 ) - B( y - 1 ) - B( y + 2 ) - A( y - 2 ) - A( y + 3 ) with, over the row's samples s[-2 .. 3] around the cell,
//                                                  A = s[-1] + s[0] + s[1] + s[2], B = s[-2] + 2 s[-1] + 3 s[0] + 3 s[1] + 2 s[2] + s[3], C = 12 ( s[0] + s[1] ) - 3 ( s[-1] + s[2] ) - s[-2] - s[3].
//
// The host cuts every area — a CTU with its guard frame, a whole plane: one code path — into tiles of VA_TW x VA_TH POSITIONS (a position is a sample of the HD form, a 2 x 2
// cell of the ds form, a sample of the mean rectangle).  One workgroup of four waves per tile: the tile's samples and its halo (1 sample HD, 2 ds) go to LDS once; a lane walks
// down VA_ROWS positions of one column with the row sums of the window in registers (HD: 3 LDS samples per position, ds: 2 rows of 3 dwords per cell); the previous originals
// are read once each, straight from memory, all of a lane's loads in flight together.  A lane's three sums are 32-bit, reduced in the wave by DPP and across the waves through
// LDS; one 32-byte partial record per tile.  A second small launch adds the partials of each area in 64 bits.  No global atomics, no pre-zeroed output, no float, no scratch.
//
// The 32-bit bound, derived for the tile of 64 x 32 positions (VA_TW x VA_TH = 2048, 8 per lane, 512 per wave) and ANY int16 samples (| difference of two samples | <= 65535):
//   per position  HD spatial 24 * 65535, ds spatial 96 * 65535 (the 2 x 2 centre weighs 48, the outer samples -48), temporal 4 * 4 * 65535 (ds, second order), mean 32768
//   per wave      512 * 96 * 65535 = 3.3e9 < 2^32 (unsigned); at the 12 bits of the reference's deepest format, 512 * 96 * 4095 < 2^28
// Anything summed across waves or tiles is 64-bit.
#include "common.h"
#include <algorithm>
#include <string.h>

namespace {

constexpr int VA_THREADS = 256, VA_WAVES = VA_THREADS / 64;
constexpr int VA_TW = 64, VA_TH = 32, VA_ROWS = VA_TH / VA_WAVES;      // positions per tile; a lane's run of rows
constexpr int VA_PITCH = 2 * VA_TW + 4, VA_LDS_ROWS = 2 * VA_TH + 4;   // the ds form's samples: the largest tile image (132 x 68 samples, 17952 bytes)
constexpr int K_HD = 0, K_DS = 1, K_MEAN = 2;

struct VaPlaneDev { const int16_t* cur; const int16_t* p1; const int16_t* p2; int curStride, p1Stride, p2Stride; };
struct VaTile     { int plane, kind, order, sx, sy, pw, ph, pad; };      // ( sx, sy ): the plane sample of the tile image's first sample; pw x ph positions.  32 bytes
struct VaSpan     { int first, count; };                                 // an area's tiles
struct VaArgs     { VaPlaneDev pl[3]; const VaTile* tiles; unsigned long long* part; };

__device__ __forceinline__ int vaLo( int d ) { return ( int ) ( short ) ( d & 0xffff ); }
__device__ __forceinline__ int vaHi( int d ) { return d >> 16; }

// the row sums of the HD form over the three samples at p
__device__ __forceinline__ void vaRowHd( const int16_t* __restrict__ p, int& P, int& Q )
{
  const int l = p[0], c = p[1], r = p[2];
  P = l + 2 * c + r; Q = 12 * c - 2 * ( l + r );
}
// the row sums of the ds form over the six samples at p (4-byte aligned); D = the cell's two samples of the row
__device__ __forceinline__ void vaRowDs( const int16_t* __restrict__ p, int& A, int& B, int& Cc, int& D )
{
  const int* q = reinterpret_cast<const int*>( p );
  const int d0 = q[0], d1 = q[1], d2 = q[2];
  const int sm2 = vaLo( d0 ), sm1 = vaHi( d0 ), s0 = vaLo( d1 ), s1 = vaHi( d1 ), s2 = vaLo( d2 ), s3 = vaHi( d2 );
  D = s0 + s1;
  A = sm1 + D + s2;
  B = sm2 + 2 * ( sm1 + s2 ) + 3 * D + s3;
  Cc = 12 * D - 3 * ( sm1 + s2 ) - sm2 - s3;
}
__device__ __forceinline__ unsigned vaTemporal( int order, int c, int p1, int p2 )
{
  return order == 1 ? ( unsigned ) ( ( 1 + 3 * abs( c - p1 ) ) >> 1 ) : ( unsigned ) abs( c - 2 * p1 + p2 );
}

__global__ void __launch_bounds__( VA_THREADS )
visactTileKernel( const VaArgs a )
{
  __shared__ __attribute__( ( aligned( 16 ) ) ) int16_t tile[VA_LDS_ROWS * VA_PITCH];
  __shared__ unsigned part[VA_WAVES][3];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const VaTile t = a.tiles[blockIdx.x];
  const VaPlaneDev& p = a.pl[t.plane];
  const int c = lane, j0 = wave * VA_ROWS;
  const bool on = c < t.pw && j0 < t.ph;
  unsigned spat = 0, temp = 0;
  int mean = 0;

  if( t.kind == K_MEAN )
  {
    // pw x ph samples at ( sx, sy ): no window, no LDS
    if( on )
    {
      const int16_t* s = p.cur + ( ptrdiff_t ) ( t.sy + j0 ) * p.curStride + t.sx + c;
#pragma unroll
      for( int k = 0; k < VA_ROWS; k++ ) mean += j0 + k < t.ph ? ( int ) s[( ptrdiff_t ) k * p.curStride] : 0;
    }
  }
  else
  {
    const bool ds = t.kind == K_DS;
    // the tile image: ( pw + 2 ) x ( ph + 2 ) samples (HD), ( 2 pw + 4 ) x ( 2 ph + 4 ) (ds) — all of them inside the area
    const int nCols = ds ? 2 * t.pw + 4 : t.pw + 2, nRows = ds ? 2 * t.ph + 4 : t.ph + 2;
    for( int r = wave; r < nRows; r += VA_WAVES )
    {
      const int16_t* s = p.cur + ( ptrdiff_t ) ( t.sy + r ) * p.curStride + t.sx;
      for( int x = lane; x < nCols; x += 64 ) tile[r * VA_PITCH + x] = s[x];
    }
    // the previous originals at the lane's positions: every load is issued before the first is used
    int pv1[VA_ROWS], pv2[VA_ROWS];
#pragma unroll
    for( int k = 0; k < VA_ROWS; k++ ) { pv1[k] = 0; pv2[k] = 0; }
    if( on && t.order )
    {
      if( ds )
      {
        const int x = t.sx + 2 + 2 * c, y = t.sy + 2 + 2 * j0;
        const int16_t* q1 = p.p1 + ( ptrdiff_t ) y * p.p1Stride + x;
#pragma unroll
        for( int k = 0; k < VA_ROWS; k++ )
          if( j0 + k < t.ph )
          {
            const int16_t* q = q1 + ( ptrdiff_t ) ( 2 * k ) * p.p1Stride;
            pv1[k] = ( int ) q[0] + ( int ) q[1] + ( int ) q[p.p1Stride] + ( int ) q[p.p1Stride + 1];
          }
        if( t.order == 2 )
        {
          const int16_t* q2 = p.p2 + ( ptrdiff_t ) y * p.p2Stride + x;
#pragma unroll
          for( int k = 0; k < VA_ROWS; k++ )
            if( j0 + k < t.ph )
            {
              const int16_t* q = q2 + ( ptrdiff_t ) ( 2 * k ) * p.p2Stride;
              pv2[k] = ( int ) q[0] + ( int ) q[1] + ( int ) q[p.p2Stride] + ( int ) q[p.p2Stride + 1];
            }
        }
      }
      else
      {
        const int x = t.sx + 1 + c, y = t.sy + 1 + j0;
#pragma unroll
        for( int k = 0; k < VA_ROWS; k++ )
          if( j0 + k < t.ph ) pv1[k] = p.p1[( ptrdiff_t ) ( y + k ) * p.p1Stride + x];
        if( t.order == 2 )
        {
#pragma unroll
          for( int k = 0; k < VA_ROWS; k++ )
            if( j0 + k < t.ph ) pv2[k] = p.p2[( ptrdiff_t ) ( y + k ) * p.p2Stride + x];
        }
      }
    }
    __syncthreads();
    if( on )
    {
      if( ds )
      {
        // cell ( c, j ) of the tile has its window in image rows 2 j .. 2 j + 5, columns 2 c .. 2 c + 5
        const int16_t* q = tile + ( 2 * j0 ) * VA_PITCH + 2 * c;
        // of the window's rows 0 .. 5 the kernel takes A of rows 0, 5, B of rows 1, 4, C and the cell samples D of rows 2, 3; two new rows per cell
        int A0, A2, A4, A5, B1, B3, B4, B5, C2, C3, C4, C5, D2, D3, D4, D5, u0, u1, u2;
        vaRowDs( q, A0, u0, u1, u2 ); vaRowDs( q + VA_PITCH, u0, B1, u1, u2 ); vaRowDs( q + 2 * VA_PITCH, A2, u0, C2, D2 ); vaRowDs( q + 3 * VA_PITCH, u0, B3, C3, D3 );
#pragma unroll
        for( int k = 0; k < VA_ROWS; k++ )
          if( j0 + k < t.ph )
          {
            vaRowDs( q + ( 2 * k + 4 ) * VA_PITCH, A4, B4, C4, D4 ); vaRowDs( q + ( 2 * k + 5 ) * VA_PITCH, A5, B5, C5, D5 );
            spat += ( unsigned ) abs( C2 + C3 - B1 - B4 - A0 - A5 );
            if( t.order ) temp += vaTemporal( t.order, D2 + D3, pv1[k], pv2[k] );
            A0 = A2; A2 = A4; B1 = B3; B3 = B5; C2 = C4; C3 = C5; D2 = D4; D3 = D5;
          }
      }
      else
      {
        // position ( c, j ) of the tile has its window in image rows j .. j + 2, columns c .. c + 2
        const int16_t* q = tile + j0 * VA_PITCH + c;
        int P0, Q0, P1, Q1, P2, Q2;
        vaRowHd( q, P0, Q0 ); vaRowHd( q + VA_PITCH, P1, Q1 );
#pragma unroll
        for( int k = 0; k < VA_ROWS; k++ )
          if( j0 + k < t.ph )
          {
            vaRowHd( q + ( k + 2 ) * VA_PITCH, P2, Q2 );
            spat += ( unsigned ) abs( Q1 - P0 - P2 );
            if( t.order ) temp += vaTemporal( t.order, q[( k + 1 ) * VA_PITCH + 1], pv1[k], pv2[k] );
            P0 = P1; P1 = P2; Q0 = Q1; Q1 = Q2;
          }
      }
    }
  }
  // every lane of every wave arrives here: the DPP sums need the whole wave
  const unsigned s0 = vvhipGroupSum32( spat, 64, lane ), s1 = vvhipGroupSum32( temp, 64, lane ), s2 = vvhipGroupSum32( ( unsigned ) mean, 64, lane );
  if( lane == 0 ) { part[wave][0] = s0; part[wave][1] = s1; part[wave][2] = s2; }
  __syncthreads();
  if( tid < 4 )
  {
    unsigned long long v;
    if( tid == 3 ) v = t.kind == K_MEAN ? 0ull : ( unsigned long long ) t.pw * ( unsigned long long ) t.ph;
    else if( tid == 2 )
    {
      long long m = 0;
#pragma unroll
      for( int w = 0; w < VA_WAVES; w++ ) m += ( long long ) ( int ) part[w][2];
      v = ( unsigned long long ) m;
    }
    else
    {
      v = 0;
#pragma unroll
      for( int w = 0; w < VA_WAVES; w++ ) v += part[w][tid];
    }
    a.part[( size_t ) blockIdx.x * 4 + tid] = v;
  }
}

// one wave per area: the 64-bit sum of its tiles' partial records.  The cross-lane sum goes through four 16-bit limbs: exact for every 64-bit value.
__global__ void __launch_bounds__( 64 )
visactSumKernel( const VaSpan* __restrict__ spans, const unsigned long long* __restrict__ part, unsigned long long* __restrict__ out )
{
  const int lane = threadIdx.x;
  const VaSpan s = spans[blockIdx.x];
  unsigned long long acc[4] = { 0, 0, 0, 0 };
  for( int i = lane; i < s.count; i += 64 )
  {
    const unsigned long long* r = part + ( size_t ) ( s.first + i ) * 4;
#pragma unroll
    for( int f = 0; f < 4; f++ ) acc[f] += r[f];
  }
  unsigned long long mine = 0;
#pragma unroll
  for( int f = 0; f < 4; f++ )
  {
    unsigned long long v = 0;
#pragma unroll
    for( int l = 0; l < 4; l++ ) v += ( unsigned long long ) vvhipGroupSum32( ( uint32_t ) ( ( acc[f] >> ( 16 * l ) ) & 0xffffull ), 64, lane ) << ( 16 * l );
    if( lane == f ) mine = v;
  }
  if( lane < 4 ) out[( size_t ) blockIdx.x * 4 + lane] = mine;
}

} // namespace

// the tile list of the areas (host): per area its filter tiles, then the tiles of its mean rectangle
static void visactTiles( const vvhip_visact_area* areas, int n, std::vector<VaTile>& tiles, std::vector<VaSpan>& spans )
{
  for( int i = 0; i < n; i++ )
  {
    const vvhip_visact_area& q = areas[i];
    VaSpan s; s.first = ( int ) tiles.size();
    const int halo = q.ds ? 2 : 1, step = q.ds ? 2 : 1;
    const int pw = ( q.w - 2 * halo ) / step, ph = ( q.h - 2 * halo ) / step;
    for( int py = 0; py < ph; py += VA_TH )
      for( int px = 0; px < pw; px += VA_TW )
      {
        VaTile t; t.plane = q.plane; t.kind = q.ds ? K_DS : K_HD; t.order = q.order; t.sx = q.x + step * px; t.sy = q.y + step * py;
        t.pw = std::min( VA_TW, pw - px ); t.ph = std::min( VA_TH, ph - py ); t.pad = 0;
        tiles.push_back( t );
      }
    if( q.mw > 0 )
      for( int py = 0; py < q.mh; py += VA_TH )
        for( int px = 0; px < q.mw; px += VA_TW )
        {
          VaTile t; t.plane = q.plane; t.kind = K_MEAN; t.order = 0; t.sx = q.mx + px; t.sy = q.my + py;
          t.pw = std::min( VA_TW, q.mw - px ); t.ph = std::min( VA_TH, q.mh - py ); t.pad = 0;
          tiles.push_back( t );
        }
    s.count = ( int ) tiles.size() - s.first;
    spans.push_back( s );
  }
}

extern "C" {

int vvhip_visact( vvhip_ctx* ctx, const vvhip_visact_plane* planes, int n_planes, const vvhip_visact_area* areas_host, int n, uint64_t* d_out )
{
  if( !ctx ) return VVHIP_E_ARG;
  if( n < 0 || !planes || n_planes < 1 || n_planes > 3 || ( n > 0 && ( !areas_host || !d_out ) ) )
    return vvhip_fail( ctx, VVHIP_E_ARG, "vvhip_visact: %d areas (>= 0), %d planes (1..3), planes / areas / d_out missing", n, n_planes );
  VaArgs A;
  memset( &A, 0, sizeof( A ) );
  for( int c = 0; c < n_planes; c++ )
  {
    const vvhip_visact_plane& q = planes[c];
    if( !q.d_cur || q.width < 1 || q.height < 1 || q.cur_stride < q.width || q.bit_depth < 8 || q.bit_depth > 16 )
      return vvhip_fail( ctx, VVHIP_E_ARG, "vvhip_visact: plane %d: %dx%d, stride %d, bitDepth %d (8..16), d_cur %s", c, q.width, q.height, q.cur_stride, q.bit_depth, q.d_cur ? "set" : "missing" );
    VaPlaneDev& p = A.pl[c];
    p.cur = q.d_cur; p.p1 = q.d_prev1; p.p2 = q.d_prev2; p.curStride = q.cur_stride; p.p1Stride = q.prev1_stride; p.p2Stride = q.prev2_stride;
  }
  for( int i = 0; i < n; i++ )
  {
    const vvhip_visact_area& q = areas_host[i];
    if( q.plane >= n_planes ) return vvhip_fail( ctx, VVHIP_E_ARG, "vvhip_visact: area %d: plane %d of %d", i, q.plane, n_planes );
    const vvhip_visact_plane& p = planes[q.plane];
    if( q.rsv0 || q.rsv1 ) return vvhip_fail( ctx, VVHIP_E_ARG, "vvhip_visact: area %d: reserved bytes are not zero", i );
    if( q.ds > 1 || q.order > 2 ) return vvhip_fail( ctx, VVHIP_E_ARG, "vvhip_visact: area %d: ds %d (0, 1), order %d (0..2)", i, q.ds, q.order );
    if( q.x < 0 || q.y < 0 || q.w < 1 || q.h < 1 || q.x > p.width - q.w || q.y > p.height - q.h )
      return vvhip_fail( ctx, VVHIP_E_ARG, "vvhip_visact: area %d: %dx%d at (%d, %d) is not inside plane %d (%dx%d)", i, q.w, q.h, q.x, q.y, q.plane, p.width, p.height );
    if( q.mw < 0 || q.mh < 0 || ( q.mw > 0 ) != ( q.mh > 0 ) || ( q.mw > 0 && ( q.mx < 0 || q.my < 0 || q.mx > p.width - q.mw || q.my > p.height - q.mh ) ) )
      return vvhip_fail( ctx, VVHIP_E_ARG, "vvhip_visact: area %d: the mean rectangle %dx%d at (%d, %d) is not inside plane %d (%dx%d)", i, q.mw, q.mh, q.mx, q.my, q.plane, p.width, p.height );
    if( q.ds ? ( q.w < 6 || q.h < 6 || ( ( q.w | q.h ) & 1 ) ) : ( q.w < 3 || q.h < 3 ) )
      return vvhip_fail( ctx, VVHIP_E_ARG, "vvhip_visact: area %d: %dx%d is too small or odd for the %s form (HD: >= 3x3; down-sampling: >= 6x6, even)", i, q.w, q.h, q.ds ? "down-sampling" : "HD" );
    if( ( q.order >= 1 && ( !p.d_prev1 || p.prev1_stride < p.width ) ) || ( q.order == 2 && ( !p.d_prev2 || p.prev2_stride < p.width ) ) )
      return vvhip_fail( ctx, VVHIP_E_ARG, "vvhip_visact: area %d: order %d needs the previous original%s of plane %d (strides %d / %d, width %d)", i, q.order, q.order == 2 ? "s" : "", q.plane,
                         p.prev1_stride, p.prev2_stride, p.width );
  }
  if( n == 0 ) return VVHIP_OK;
  std::vector<VaTile> tiles;
  std::vector<VaSpan> spans;
  visactTiles( areas_host, n, tiles, spans );
  // one blob: the tiles, then the spans right behind them
  const size_t tileBytes = tiles.size() * sizeof( VaTile );
  ListBlob blob( tiles.data(), tileBytes );
  blob.add( spans.data(), spans.size() * sizeof( VaSpan ), 1 );
  HostList& S = ctx->list[LIST_VISACT];
  int rc = listUpload( ctx, S, blob );      // (waits for the last launches of this entry: the partial records below are free then, too)
  if( rc != VVHIP_OK ) return rc;
  // the per-tile partial records: a device-only buffer in a slot of its own, guarded by the list slot's event — every launch that touches it also reads the list
  HostList& P = ctx->list[LIST_VISACT_PART];
  if( ( rc = listReserve( ctx, P, tiles.size() * 4 * sizeof( unsigned long long ) ) ) != VVHIP_OK ) return rc;
  A.tiles = ( const VaTile* ) S.d; A.part = ( unsigned long long* ) P.d;
  hipLaunchKernelGGL( visactTileKernel, dim3( ( unsigned ) tiles.size() ), dim3( VA_THREADS ), 0, ctx->stream, A );
  VVHIP_LAUNCH_CHECK( ctx );
  hipLaunchKernelGGL( visactSumKernel, dim3( ( unsigned ) n ), dim3( 64 ), 0, ctx->stream, ( const VaSpan* ) ( ( const unsigned char* ) S.d + tileBytes ), ( const unsigned long long* ) P.d,
                      ( unsigned long long* ) d_out );
  VVHIP_LAUNCH_CHECK( ctx );
  return listLaunched( ctx, S );
}

} // extern "C"
