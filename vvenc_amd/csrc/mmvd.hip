// mmvd.hip — the MMVD merge candidates of a list of CUs (gfx950): per CU up to 64 candidates ( two base vectors x eight steps x four directions ), each predicted from its
// base vector plus the MMVD delta and scored with the Hadamard sum against the original, in the kernel that makes the prediction.  Only the costs leave the device.
//
// Restates, per requested candidate, the decision-free part of EncCu::addMmvdCandsToPruningList (EncoderLib/EncCu.cpp:2353-2453):
//   MergeCtx::setMmvdMergeCandiInfo, getMmvdDeltaMv, the clips, identical motion      mmvd_cand.h ( shared with the host: vvhip_mmvd_candidate )
//   InterPredInterpolation::xPredInterBlk, xWeightedAverage                           the passes and averages of pred.hip ( luma, 8 taps, 14-bit intermediate )
//   RdCost::xGetHADs<false> / <true>                                                  hadtile.h
//
// One workgroup of four waves per TILE of a CU ( at most 512 samples: 32 x 16, 16 x 32, 8 x 64, 4 x 64; most CUs are one tile ).  The tile's original and, per base vector and
// list, ONE reference window centred on the base vector ( tile + 18 samples per direction: every step of up to four samples lies inside ) are staged in LDS once; the
// requested candidates are dealt to the waves.  A wave derives its candidate's vectors ( uniform ), runs the horizontal pass over th + 7 rows into its own 14-bit rows — from
// the LDS window when the candidate's footprint lies inside it, straight from HBM ( aligned dwords ) when it does not: the far steps, a scaled delta, a clipped vector —, the
// vertical pass, the average with list 0's block for two lists, and scores the tile from LDS with the team transform of hadtile.h at 32-bit differences.  A zero fraction takes
// the same two passes with the one-tap set { 64 } ( pred.hip ).  A CU of one tile stores its costs; the tiles of a larger CU add theirs with integer atomics onto slots a
// small kernel has zeroed in front — integer sums, so the result does not depend on the order.
#include <string.h>
#include "common.h"
#include "hadtile.h"
#include "mmvd_cand.h"

namespace {

constexpr int MM_THREADS = 256, MM_WAVES = 4, MM_TILE = 512, MM_TH_MAX = 64;
constexpr int MM_REACH = 8, MM_RING = 18;                  // the window starts 8 samples left of / above the base position and is tile + 18 samples wide and high
constexpr int MM_WIN_DW = ( 26 * 82 + 12 ) / 2;            // the largest window ( the 8 x 64 tile ) and the slack of the last aligned read, in dwords
constexpr int MM_TMP = 23 * 32 + 8;                        // the largest first-pass block ( 32 x 16: 23 rows )

__constant__ int8_t cMLuma8[9][8] = {
  { 0, 0, 0, 64, 0, 0, 0, 0 }, { 0, 1, -3, 63, 4, -2, 1, 0 }, { -1, 2, -5, 62, 8, -3, 1, 0 }, { -1, 3, -8, 60, 13, -4, 1, 0 }, { -1, 4, -10, 58, 17, -5, 1, 0 },
  { -1, 4, -11, 52, 26, -8, 3, -1 }, { -1, 3, -9, 47, 31, -10, 4, -1 }, { -1, 4, -11, 45, 34, -10, 4, -1 }, { -1, 4, -11, 40, 40, -11, 4, -1 } };
__constant__ int8_t cMAltHpel[8] = { 0, 3, 9, 20, 20, 9, 3, 0 };
__constant__ int8_t cMBcwW1[5]   = { -2, 3, 4, 5, 10 };

struct MmvdTile   { int32_t item; int16_t x0, y0; };
struct MmvdPlanes { const int16_t* p[16]; int32_t stride[16]; };
static_assert( sizeof( MmvdTile ) == 8, "MmvdTile layout" );

typedef short s16x4 __attribute__( ( ext_vector_type( 4 ) ) );

struct __attribute__( ( aligned( 16 ) ) ) MmvdLds
{
  int16_t  org[MM_TILE];
  uint32_t win[4][MM_WIN_DW];              // [base * 2 + list]
  int16_t  tmp[MM_WAVES][MM_TMP];          // a wave's first-pass rows
  int16_t  blk0[MM_WAVES][MM_TILE];        // list 0's 14-bit block of a bi-predicted candidate
  int16_t  pred[MM_WAVES][MM_TILE];
  int      wOn[4], wx[4], wy[4], we[4];    // per window: loaded; its first sample in block coordinates; the same as an element offset from the plane's aligned base
  int      nCand;
  uint8_t  cand[64];
  vvhip_mmvd_item item;                    // the CU's record, read once per workgroup: its per-base fields are indexed with the candidate's base (profiles/merge_mmvd.md
                                           // says why the first form, which indexed the record in global memory, was given up)
};

__host__ __device__ inline int mmTileW( int w ) { return w < 32 ? w : 32; }
__host__ __device__ inline int mmTileH( int w, int h ) { const int m = MM_TILE / mmTileW( w ) < MM_TH_MAX ? MM_TILE / mmTileW( w ) : MM_TH_MAX; return h < m ? h : m; }
__host__ __device__ inline int mmTiles( int w, int h ) { return ( w / mmTileW( w ) ) * ( h / mmTileH( w, h ) ); }

#define MM_WAVE_SYNC() { __builtin_amdgcn_fence( __ATOMIC_ACQ_REL, "wavefront" ); __builtin_amdgcn_wave_barrier(); }

__device__ __forceinline__ void mmTaps( int ( &c )[8], int frac, int alt )
{
#pragma unroll
  for( int k = 0; k < 8; k++ )
  {
    const int p = frac <= 8 ? frac : 16 - frac, kk = frac <= 8 ? k : 7 - k;
    c[k] = ( alt && frac == 8 ) ? cMAltHpel[k] : cMLuma8[p][kk];
  }
}

// first pass ( isFirst, !isLast ): rows x tw samples into tmp from the samples at element e0 + r * strideE + x - 0 .. + 10 of src32 ( aligned dwords; the element offset
// carries the parity )
__device__ __forceinline__ void mmHPass( const uint32_t* src32, int e0, int strideE, int rows, int tw, int log2Segs, const int ( &ch )[8], int s1, int16_t* tmp, int lane )
{
  const int off1 = -( 8192 << s1 ), segs = 1 << log2Segs;
  for( int i = lane; i < ( rows << log2Segs ); i += 64 )
  {
    const int r = i >> log2Segs, x = ( i & ( segs - 1 ) ) * 4;
    const int e = e0 + r * strideE + x;
    const uint32_t* p = src32 + ( e >> 1 );
    const uint32_t sh = ( uint32_t ) ( e & 1 ) << 4;
    uint32_t d[6];
#pragma unroll
    for( int k = 0; k < 6; k++ ) d[k] = p[k];
    int win[11];
#pragma unroll
    for( int k = 0; k < 5; k++ )
    {
      const uint32_t s = __builtin_amdgcn_alignbit( d[k + 1], d[k], sh );
      win[2 * k] = ( int ) ( int16_t ) ( s & 0xffff ); win[2 * k + 1] = ( int ) ( int16_t ) ( s >> 16 );
    }
    win[10] = ( int ) ( int16_t ) ( ( d[5] >> sh ) & 0xffff );
    s16x4 o;
#pragma unroll
    for( int j = 0; j < 4; j++ )
    {
      int s = 0;
#pragma unroll
      for( int k = 0; k < 8; k++ ) s = __mul24( win[j + k], ch[k] ) + s;
      o[j] = ( short ) ( ( s + off1 ) >> s1 );
    }
    *reinterpret_cast<s16x4*>( tmp + r * tw + x ) = o;
  }
}

__global__ void __launch_bounds__( MM_THREADS )
mmvdZeroKernel( const vvhip_mmvd_item* __restrict__ items, int n, uint32_t* __restrict__ cost )
{
  const int i = ( int ) ( blockIdx.x * MM_THREADS + threadIdx.x ) >> 6, s = threadIdx.x & 63;
  if( i >= n ) return;
  const vvhip_mmvd_item& q = items[i];
  if( mmTiles( q.w, q.h ) > 1 && ( ( q.cand_mask[s >> 5] >> ( s & 31 ) ) & 1 ) ) cost[( size_t ) q.cost_off + s] = 0;
}

__global__ void __launch_bounds__( MM_THREADS )
mmvdCostsKernel( const vvhip_mmvd_item* __restrict__ items, const MmvdTile* __restrict__ tiles, const MmvdPlanes P, const int16_t* __restrict__ org, int orgStride,
                 uint32_t* __restrict__ cost, int picW, int picH, int ctu, int bitDepth, int fast, int disFrac )
{
  __shared__ MmvdLds L;
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane( tid >> 6 );
  const MmvdTile T = tiles[blockIdx.x];
  if( tid < ( int ) ( sizeof( vvhip_mmvd_item ) / 4 ) ) reinterpret_cast<uint32_t*>( &L.item )[tid] = reinterpret_cast<const uint32_t*>( items + T.item )[tid];
  __syncthreads();
  const vvhip_mmvd_item& q = L.item;
  const int w = q.w, h = q.h, x0 = T.x0, y0 = T.y0;
  const int tw = mmTileW( w ), th = mmTileH( w, h ), log2tw = 31 - __builtin_clz( tw ), log2Segs = log2tw - 2;
  const int pitch = tw + MM_RING, wrows = th + MM_RING;
  const uint32_t m0 = q.cand_mask[0], m1 = q.cand_mask[1];

  // ---- the original tile, the requested candidates in ascending order, the windows' places ----
  {
    const int16_t* o = org + ( size_t ) q.org_off + ( ptrdiff_t ) y0 * orgStride + x0;
    for( int i = tid; i < tw * th; i += MM_THREADS ) L.org[i] = o[( ptrdiff_t ) ( i >> log2tw ) * orgStride + ( i & ( tw - 1 ) )];
  }
  if( tid < 64 )
  {
    const uint32_t mine = tid < 32 ? m0 : m1;
    if( ( mine >> ( tid & 31 ) ) & 1 )
      L.cand[( tid < 32 ? 0 : __builtin_popcount( m0 ) ) + __builtin_popcount( mine & ( ( 1u << ( tid & 31 ) ) - 1u ) )] = ( uint8_t ) tid;
    if( tid == 0 ) L.nCand = __builtin_popcount( m0 ) + __builtin_popcount( m1 );
  }
  else if( tid < 68 )
  {
    const int k = tid - 64, b = k >> 1, l = k & 1;
    bool on = ( b ? m1 : m0 ) != 0 && q.ref_plane[b][l] >= 0;
    int pwx = 0, pwy = 0, pwe = 0;
    if( on )
    {
      MmvdCand c;
      mmvdDerive( q, b << 5, picW, picH, ctu, disFrac, c, true );
      on = l ? c.used[1] : c.used[0];
      if( on )
      {
        const int pl = q.ref_plane[b][l], stride = P.stride[pl];
        const int bx = ( l ? c.mvx[1] : c.mvx[0] ) >> 4, by = ( l ? c.mvy[1] : c.mvy[0] ) >> 4;
        // inside what a candidate may read ( the entry's read bound ): picture columns -( ctu + 11 ) .. picW + w + 11, rows likewise
        int wx = min( max( q.cu_x + x0 + bx - MM_REACH, -( ctu + 11 ) ), picW + w + 11 - ( pitch - 1 ) ) - q.cu_x;
        const int wy = min( max( q.cu_y + y0 + by - MM_REACH, -( ctu + 11 ) ), picH + h + 11 - ( wrows - 1 ) ) - q.cu_y;
        const int par = ( int ) ( ( reinterpret_cast<uintptr_t>( P.p[pl] ) >> 1 ) & 1 );
        int e = par + q.ref_off[b][l] + wy * stride + wx;
        if( e & 1 ) { e--; wx--; }
        pwx = wx; pwy = wy; pwe = e;
      }
    }
    L.wOn[k] = on; L.wx[k] = pwx; L.wy[k] = pwy; L.we[k] = pwe;      // ( zeros for a window that is not loaded: the candidates read wx / wy next to wOn )
  }
  __syncthreads();
#pragma unroll
  for( int k = 0; k < 4; k++ )
  {
    if( !L.wOn[k] ) continue;
    const int pl = q.ref_plane[k >> 1][k & 1], stride = P.stride[pl], pd = pitch >> 1;
    const uint32_t* src32 = reinterpret_cast<const uint32_t*>( reinterpret_cast<uintptr_t>( P.p[pl] ) & ~( uintptr_t ) 3 );
    const int e = L.we[k], d = tid & 31;
    if( d < pd )
      for( int r = tid >> 5; r < wrows; r += MM_THREADS / 32 ) L.win[k][r * pd + d] = src32[( ptrdiff_t ) ( ( e + r * stride ) >> 1 ) + d];
  }
  __syncthreads();

  // ---- the candidates, one wave each ----
  const int hr = 14 - bitDepth > 2 ? 14 - bitDepth : 2, maxv = ( 1 << bitDepth ) - 1, s1 = 6 - hr;
  const int kind = hadTileKind( w, h, fast != 0 ), nTiles = mmTiles( w, h ), nCand = L.nCand;
  int16_t* tmp = L.tmp[wave]; int16_t* blk0 = L.blk0[wave]; int16_t* pred = L.pred[wave];
  for( int ci = wave; ci < nCand; ci += MM_WAVES )
  {
    const int val = __builtin_amdgcn_readfirstlane( ( int ) L.cand[ci] ), b = val >> 5;
    MmvdCand c;
    mmvdDerive( q, val, picW, picH, ctu, disFrac, c );
    const bool bi = c.used[0] && c.used[1];
    const int alt = q.alt_hpel[b], w1 = cMBcwW1[c.bcw], w0 = 8 - w1;
#pragma unroll
    for( int l = 0; l < 2; l++ )
    {
      if( !c.used[l] ) continue;
      const int mvx = c.mvx[l], mvy = c.mvy[l], ix = mvx >> 4, iy = mvy >> 4;
      int ch[8], cv[8];
      mmTaps( ch, mvx & 15, alt );
      mmTaps( cv, mvy & 15, alt );
      // the footprint's first sample in block coordinates; inside the base vector's window?
      const int fx = x0 + ix - 3, fy = y0 + iy - 3, k = 2 * b + l;
      const int ei = fx - L.wx[k], ri = fy - L.wy[k];
      if( L.wOn[k] && ei >= 0 && ei <= MM_RING - 7 && ri >= 0 && ri <= MM_RING - 7 )
        mmHPass( L.win[k], ri * pitch + ei, pitch, th + 7, tw, log2Segs, ch, s1, tmp, lane );
      else
      {
        const int pl = q.ref_plane[b][l], stride = P.stride[pl];
        const uintptr_t a = reinterpret_cast<uintptr_t>( P.p[pl] );
        mmHPass( reinterpret_cast<const uint32_t*>( a & ~( uintptr_t ) 3 ), ( int ) ( ( a >> 1 ) & 1 ) + q.ref_off[b][l] + fy * stride + fx, stride, th + 7, tw, log2Segs, ch, s1, tmp, lane );
      }
      MM_WAVE_SYNC();
      // second pass ( !isFirst ): the final sample of one list, or the 14-bit block and the weighted average of two ( w0 = w1 = 4: addAvg )
      const int s2 = 6 + hr, off2 = ( 1 << ( s2 - 1 ) ) + ( 8192 << 6 ), shB = hr + 3, offB = ( 1 << ( shB - 1 ) ) + ( 8192 << 3 );
      for( int i = lane; i < ( th << log2Segs ); i += 64 )
      {
        const int y = i >> log2Segs, x = ( i & ( ( 1 << log2Segs ) - 1 ) ) * 4;
        int acc[4] = { 0, 0, 0, 0 };
#pragma unroll
        for( int t = 0; t < 8; t++ )
        {
          const s16x4 row = *reinterpret_cast<const s16x4*>( tmp + ( y + t ) * tw + x );
#pragma unroll
          for( int j = 0; j < 4; j++ ) acc[j] = __mul24( ( int ) row[j], cv[t] ) + acc[j];
        }
        s16x4 o;
        if( !bi )
        {
#pragma unroll
          for( int j = 0; j < 4; j++ ) { const int v = ( int16_t ) ( ( acc[j] + off2 ) >> s2 ); o[j] = ( short ) ( v < 0 ? 0 : ( v > maxv ? maxv : v ) ); }
          *reinterpret_cast<s16x4*>( pred + y * tw + x ) = o;
        }
        else if( l == 0 )
        {
#pragma unroll
          for( int j = 0; j < 4; j++ ) o[j] = ( short ) ( acc[j] >> 6 );
          *reinterpret_cast<s16x4*>( blk0 + y * tw + x ) = o;
        }
        else
        {
          const s16x4 f = *reinterpret_cast<const s16x4*>( blk0 + y * tw + x );
#pragma unroll
          for( int j = 0; j < 4; j++ )
          {
            const int v = ( w0 * ( int ) f[j] + w1 * ( int ) ( int16_t ) ( acc[j] >> 6 ) + offB ) >> shB;
            o[j] = ( short ) ( v < 0 ? 0 : ( v > maxv ? maxv : v ) );
          }
          *reinterpret_cast<s16x4*>( pred + y * tw + x ) = o;
        }
      }
      MM_WAVE_SYNC();
    }
    // ---- the tile's Hadamard sum: teams of lanes per transform tile ( table in front of hadTeam, hadtile.h ) ----
    uint32_t sum = 0;
    const int PW = tileW( kind ), PH = tileH( kind ), LT = tileLanes( kind ), log2LT = 31 - __builtin_clz( LT );
    const int log2TX = log2tw - ( 31 - __builtin_clz( PW ) ), slots = kind == TK_16F ? ( tw * th ) >> 5 : ( tw * th ) >> 3;
    for( int s0 = 0; s0 < slots; s0 += 64 )
    {
      const int sl = s0 + lane;
      const bool valid = sl < slots;                                                     // (teams are whole: slots is a multiple of the team size)
      const int sv = valid ? sl : 0, t = sv >> log2LT, r = sv & ( LT - 1 );
      const int tx = ( t & ( ( 1 << log2TX ) - 1 ) ) * PW, ty = ( t >> log2TX ) * PH;
      int d[8];
      if( kind == TK_16F )                                                               // rows 2r, 2r + 1: the 2x2 averages of original and prediction (RdCost.cpp:1138-1160)
      {
        const int at = ( ty + 2 * r ) * tw + tx;
#pragma unroll
        for( int i = 0; i < 8; i++ )
        {
          const int a = at + 2 * i;
          const int ao = ( ( int ) L.org[a] + L.org[a + 1] + L.org[a + tw] + L.org[a + tw + 1] + 2 ) >> 2;
          const int ap = ( ( int ) pred[a] + pred[a + 1] + pred[a + tw] + pred[a + tw + 1] + 2 ) >> 2;
          d[i] = ao - ap;
        }
      }
      else
      {
        const int xx = tx + ( kind == TK_16x8 ? 8 * ( r >> 3 ) : 0 ), yy = ty + ( kind == TK_16x8 ? ( r & 7 ) : ( kind == TK_4x8 ? 2 * r : r ) );
#pragma unroll
        for( int i = 0; i < 8; i++ )
        {
          const int a = ( yy + ( kind == TK_4x8 ? ( i >> 2 ) : 0 ) ) * tw + xx + ( kind == TK_4x8 ? ( i & 3 ) : i );
          d[i] = ( int ) L.org[a] - ( int ) pred[a];
        }
      }
      const uint32_t sres = hadTeam( d, r, LT, kind, lane );
      if( valid && r == 0 ) sum += sres;
    }
    sum = vvhipGroupSum32( sum, 64, lane );
    if( lane == 0 )
    {
      uint32_t* out = cost + ( size_t ) q.cost_off + val;
      if( nTiles == 1 ) *out = sum; else atomicAdd( out, sum );
    }
    MM_WAVE_SYNC();
  }
}

const char* mmvdCheck( const vvhip_mmvd_item& q, int nPlanes, int picW, int picH, char* msg, size_t len )
{
  if( !mmvdSizeOk( q.w, q.h ) ) { snprintf( msg, len, "%dx%d (powers of two 4..128, w + h >= 12)", q.w, q.h ); return msg; }
  if( q.cu_x < 0 || q.cu_y < 0 || q.cu_x + q.w > picW || q.cu_y + q.h > picH ) { snprintf( msg, len, "the CU at ( %d, %d ) lies outside the %dx%d picture", q.cu_x, q.cu_y, picW, picH ); return msg; }
  if( q.org_off < 0 || q.cost_off < 0 ) { snprintf( msg, len, "a negative org_off or cost_off" ); return msg; }
  if( q.rsv0[0] || q.rsv0[1] ) { snprintf( msg, len, "reserved bytes are not zero" ); return msg; }
  for( int k = 0; k < 14; k++ ) if( q.rsv[k] ) { snprintf( msg, len, "reserved bytes are not zero" ); return msg; }
  for( int b = 0; b < 2; b++ )
  {
    if( q.bcw_idx[b] > 4 ) { snprintf( msg, len, "base %d: bcw_idx %d (0..4)", b, q.bcw_idx[b] ); return msg; }
    if( q.long_term[b] > 3 || q.alt_hpel[b] > 1 ) { snprintf( msg, len, "base %d: long_term %d (bits 0, 1), alt_hpel %d (0, 1)", b, q.long_term[b], q.alt_hpel[b] ); return msg; }
    for( int l = 0; l < 2; l++ )
    {
      if( q.ref_plane[b][l] < -1 || q.ref_plane[b][l] >= nPlanes ) { snprintf( msg, len, "base %d list %d: plane %d outside the table of %d", b, l, q.ref_plane[b][l], nPlanes ); return msg; }
      if( q.ref_plane[b][l] < 0 ) continue;
      if( q.ref_off[b][l] < 0 ) { snprintf( msg, len, "base %d list %d: a negative ref_off", b, l ); return msg; }
      for( int k = 0; k < 2; k++ )
        if( q.mv[b][l][k] < -( 1 << 17 ) || q.mv[b][l][k] > ( 1 << 17 ) - 1 ) { snprintf( msg, len, "base %d list %d: vector component %d outside the 18-bit range", b, l, q.mv[b][l][k] ); return msg; }
    }
    if( q.cand_mask[b] && q.ref_plane[b][0] < 0 && q.ref_plane[b][1] < 0 ) { snprintf( msg, len, "base %d uses neither list and has candidates requested", b ); return msg; }
  }
  return nullptr;
}

} // namespace

extern "C" {

int vvhip_mmvd_candidate( const vvhip_mmvd_item* item, int val, int pic_width, int pic_height, int ctu_size, int dis_frac, vvhip_mmvd_cand* out )
{
  if( !item || !out || val < 0 || val > 63 || !mmvdSizeOk( item->w, item->h ) || ( ctu_size != 32 && ctu_size != 64 && ctu_size != 128 ) ) return VVHIP_E_ARG;
  const int b = val >> 5;
  if( item->ref_plane[b][0] < 0 && item->ref_plane[b][1] < 0 ) return VVHIP_E_ARG;
  MmvdCand c;
  mmvdDerive( *item, val, pic_width, pic_height, ctu_size, dis_frac, c );
  memset( out, 0, sizeof( *out ) );
  for( int l = 0; l < 2; l++ )
  {
    out->mv[l][0] = c.mvx[l]; out->mv[l][1] = c.mvy[l]; out->stored_mv[l][0] = c.stx[l]; out->stored_mv[l][1] = c.sty[l];
    out->ref_plane[l] = c.used[l] ? item->ref_plane[b][l] : ( int8_t ) -1;
  }
  out->bcw_idx = ( uint8_t ) c.bcw;
  out->alt_hpel = item->alt_hpel[b];
  return VVHIP_OK;
}

int vvhip_merge_mmvd_costs_batch( vvhip_ctx* ctx, const vvhip_me_plane* planes_host, int n_planes, const vvhip_mmvd_item* items_host, int n,
                                  int pic_width, int pic_height, int ctu_size, int bit_depth, int func, int dis_frac,
                                  const int16_t* d_org, int org_stride, uint32_t* d_cost )
{
  if( !ctx ) return VVHIP_E_ARG;
  if( n < 0 || ( n > 0 && ( !items_host || !planes_host || !d_org || !d_cost ) ) )
    return vvhip_fail( ctx, VVHIP_E_ARG, "vvhip_merge_mmvd_costs_batch: %d items (>= 0), planes / items / d_org / d_cost missing", n );
  if( n_planes < 0 || n_planes > 16 ) return vvhip_fail( ctx, VVHIP_E_ARG, "vvhip_merge_mmvd_costs_batch: %d planes (at most 16)", n_planes );
  if( bit_depth < 8 || bit_depth > 12 ) return vvhip_fail( ctx, VVHIP_E_ARG, "vvhip_merge_mmvd_costs_batch: bit depth %d (8..12)", bit_depth );
  if( func != VVHIP_DF_HAD && func != VVHIP_DF_HAD_FAST ) return vvhip_fail( ctx, VVHIP_E_ARG, "vvhip_merge_mmvd_costs_batch: func %d (VVHIP_DF_HAD or VVHIP_DF_HAD_FAST)", func );
  if( ctu_size != 32 && ctu_size != 64 && ctu_size != 128 ) return vvhip_fail( ctx, VVHIP_E_ARG, "vvhip_merge_mmvd_costs_batch: ctu_size %d (32, 64, 128)", ctu_size );
  if( pic_width <= 0 || pic_height <= 0 || ( n > 0 && org_stride <= 0 ) ) return vvhip_fail( ctx, VVHIP_E_ARG, "vvhip_merge_mmvd_costs_batch: picture %dx%d, org_stride %d", pic_width, pic_height, org_stride );
  MmvdPlanes P;
  memset( &P, 0, sizeof( P ) );
  for( int i = 0; i < n_planes && n > 0; i++ )
  {
    if( !planes_host[i].d_base || planes_host[i].stride <= 0 || ( planes_host[i].stride & 1 ) )
      return vvhip_fail( ctx, VVHIP_E_ARG, "vvhip_merge_mmvd_costs_batch: plane %d: base missing or row pitch %d (positive and even)", i, planes_host[i].stride );
    P.p[i] = planes_host[i].d_base; P.stride[i] = planes_host[i].stride;
  }
  std::vector<MmvdTile> tiles;
  bool multi = false;
  for( int i = 0; i < n; i++ )
  {
    char msg[160];
    if( mmvdCheck( items_host[i], n_planes, pic_width, pic_height, msg, sizeof( msg ) ) ) return vvhip_fail( ctx, VVHIP_E_ARG, "vvhip_merge_mmvd_costs_batch: item %d: %s", i, msg );
    const vvhip_mmvd_item& q = items_host[i];
    if( !q.cand_mask[0] && !q.cand_mask[1] ) continue;
    const int tw = mmTileW( q.w ), th = mmTileH( q.w, q.h );
    multi = multi || mmTiles( q.w, q.h ) > 1;
    for( int y = 0; y < q.h; y += th )
      for( int x = 0; x < q.w; x += tw ) tiles.push_back( MmvdTile{ i, ( int16_t ) x, ( int16_t ) y } );
  }
  if( tiles.empty() ) return VVHIP_OK;
  HostList& S = ctx->list[LIST_MMVD];
  ListBlob blob( items_host, ( size_t ) n * sizeof( vvhip_mmvd_item ) );
  const size_t tileOff = blob.add( tiles.data(), tiles.size() * sizeof( MmvdTile ) );
  const int rc = listUpload( ctx, S, blob );
  if( rc != VVHIP_OK ) return rc;
  const vvhip_mmvd_item* dItems = ( const vvhip_mmvd_item* ) S.d;
  const MmvdTile* dTiles = ( const MmvdTile* ) ( ( const unsigned char* ) S.d + tileOff );
  if( multi )
  {
    hipLaunchKernelGGL( mmvdZeroKernel, dim3( ( unsigned ) ( ( n + 3 ) / 4 ) ), dim3( MM_THREADS ), 0, ctx->stream, dItems, n, d_cost );
    VVHIP_LAUNCH_CHECK( ctx );
  }
  hipLaunchKernelGGL( mmvdCostsKernel, dim3( ( unsigned ) tiles.size() ), dim3( MM_THREADS ), 0, ctx->stream, dItems, dTiles, P, d_org, org_stride, d_cost,
                      pic_width, pic_height, ctu_size, bit_depth, func == VVHIP_DF_HAD_FAST ? 1 : 0, dis_frac ? 1 : 0 );
  VVHIP_LAUNCH_CHECK( ctx );
  return listLaunched( ctx, S );
}

} // extern "C"
