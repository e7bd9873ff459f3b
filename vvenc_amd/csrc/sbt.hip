// sbt.hip — sub-block transform (SBT) around the fused TU pipeline: vvhip_sbt_parts_batch / vvhip_sbt_tiles / vvhip_sbt_place_batch (gfx950 only).
//
// SBT codes one half or one quarter of an inter CU's residual and takes the rest as zero.  A coded tile is an ordinary TU job on a sub-rectangle of the CU's residual
// (vvhip_tu_rdo_multi_strided reads it in place), so three pieces around the TU lists are all there is, for a LIST of CUs of mixed sizes per launch:
//   parts  : InterSearch::xCalcMinDistSbt (EncoderLib/InterSearch.cpp:3272-3464) — the residual energy of every CU in a grid of up to 4 x 4 parts over Y, Cb and Cr, the
//            estimated minimum distortion of the eight SBT modes and the order in which at most 2 + 2 of them are tried
//   tiles  : CU::getSbtTuSplit (CommonLib/UnitTools.cpp:3388), PartitionerImpl::getSbtTuTiling (CommonLib/UnitPartitioner.cpp:995-1056) and the SBT branch of
//            TrQuant::xSetTrTypes (CommonLib/TrQuant.cpp:435-466) — host arithmetic, no kernel
//   place  : the compact reconstruction of the coded tile back into the CU's block with the other tile zero (tu.noResidual, InterSearch.cpp:3562, :3758-3762) and the
//            CU's SSE per component
// Both kernels follow ict.hip: the host sorts the list into classes (shape and vector widths), a wave never mixes classes, small CUs share a wave, every lane moves segments
// of V samples (8, 4, 2 or 1: the widest vector offsets, pitches, part / tile width and base pointers allow) that never straddle a part or tile boundary, every sum is 64-bit,
// reduced inside the wave and stored once — no atomics, no scratch.
#include "common.h"
#include <algorithm>
#include <initializer_list>
#include <string.h>

namespace {

__host__ __device__ constexpr int ilog2c( int v ) { return v >= 8 ? 3 : v >= 4 ? 2 : v >= 2 ? 1 : 0; }
// the part grid of one side (InterSearch.cpp:3291-3292): 4 parts from 16, one part at 4, two between
__host__ __device__ constexpr int sbtLog2Parts( int log2Side ) { return log2Side >= 4 ? 2 : log2Side == 2 ? 0 : 1; }

struct SbtPartsDev { int32_t off[3], strideY, strideC, idx; uint8_t allowed, pad[3]; };                               // one CU as the parts kernel reads it; idx: its place in the caller's list
struct SbtPlaceDev { int32_t off[3], strideY, strideC, tileOff[3], statsIdx[3], idx; uint8_t mode, pad[3]; };       // one candidate as the placement kernel reads it
struct SbtUnit     { int32_t first; int16_t n; uint8_t log2W, log2H, log2VY, log2VC, log2Lanes, pad; };             // what one wave does: n items of one class from items[first]; n == 0: nothing

template<int V> struct __attribute__( ( aligned( V * 2 ) ) ) SbtSeg { int16_t v[V]; };

#define SBT_WAVE_SYNC() { __builtin_amdgcn_fence( __ATOMIC_ACQ_REL, "wavefront" ); __builtin_amdgcn_wave_barrier(); }

__device__ __forceinline__ SbtUnit sbtUnitOfWave( const SbtUnit* __restrict__ units, int wave )
{
  // one record per wave: the same address in every lane, made scalar so that the class switch and the loop bounds are wave-uniform
  const int32_t* p = reinterpret_cast<const int32_t*>( units + wave );
  const int32_t w0 = __builtin_amdgcn_readfirstlane( p[0] ), w1 = __builtin_amdgcn_readfirstlane( p[1] ), w2 = __builtin_amdgcn_readfirstlane( p[2] );
  SbtUnit u;
  u.first = w0; u.n = ( int16_t ) ( w1 & 0xFFFF ); u.log2W = ( uint8_t ) ( ( w1 >> 16 ) & 0xFF ); u.log2H = ( uint8_t ) ( ( w1 >> 24 ) & 0xFF );
  u.log2VY = ( uint8_t ) ( w2 & 0xFF ); u.log2VC = ( uint8_t ) ( ( w2 >> 8 ) & 0xFF ); u.log2Lanes = ( uint8_t ) ( ( w2 >> 16 ) & 0xFF ); u.pad = 0;
  return u;
}

// ---- parts --------------------------------------------------------------------------------------------------------------------------------------------------------------
// energy of the segments s = sub, sub + L, ... of one part of 2^log2PW x 2^log2PH samples at p
template<int V>
__device__ __forceinline__ unsigned long long sbtEnergy( const int16_t* __restrict__ p, int stride, int log2PW, int log2PH, int sub, int L )
{
  const int log2SegsRow = log2PW - ilog2c( V ), segs = 1 << ( log2PW + log2PH - ilog2c( V ) );
  unsigned long long e = 0;
  for( int s = sub; s < segs; s += L )
  {
    const int y = s >> log2SegsRow, x = ( s & ( ( 1 << log2SegsRow ) - 1 ) ) * V;
    const SbtSeg<V> r = *reinterpret_cast<const SbtSeg<V>*>( p + ( ptrdiff_t ) y * stride + x );
#pragma unroll
    for( int k = 0; k < V; k++ ) e += ( unsigned long long ) ( ( int ) r.v[k] * ( int ) r.v[k] );      // ( -32768 )^2 = 2^30 fits the int
  }
  return e;
}

__device__ __forceinline__ unsigned long long sbtEnergyV( int log2V, const int16_t* __restrict__ p, int stride, int log2PW, int log2PH, int sub, int L )
{
  switch( log2V )
  {
  case 3:  return sbtEnergy<8>( p, stride, log2PW, log2PH, sub, L );
  case 2:  return sbtEnergy<4>( p, stride, log2PW, log2PH, sub, L );
  case 1:  return sbtEnergy<2>( p, stride, log2PW, log2PH, sub, L );
  default: return sbtEnergy<1>( p, stride, log2PW, log2PH, sub, L );
  }
}

// m_estMinDistSbt and m_sbtRdoOrder from the weighted part sums d[j * 4 + i] (cells outside the grid are zero), InterSearch.cpp:3338-3463.  Sums of 64-bit integers wrap
// like the reference's whatever their association, and ( a << 5 ) distributes over them, so column / row totals stand in for the loops over j / i.
__device__ __forceinline__ void sbtEstimate( const unsigned long long ( &d )[16], int npx, int npy, unsigned allowed, unsigned long long ( &est )[9], unsigned char ( &order )[8] )
{
  const unsigned long long MAXD = ~0ull;
  unsigned long long C[4], R[4];
#pragma unroll
  for( int k = 0; k < 4; k++ ) { C[k] = d[k] + d[4 + k] + d[8 + k] + d[12 + k]; R[k] = d[4 * k] + d[4 * k + 1] + d[4 * k + 2] + d[4 * k + 3]; }
  est[8] = C[0] + C[1] + C[2] + C[3];
#pragma unroll
  for( int k = 0; k < 8; k++ ) est[k] = MAXD;
  if( allowed & 2u )      // SBT_VER_HALF
  {
    const unsigned long long resi = npx == 4 ? C[0] + C[1] : C[0], no = npx == 4 ? C[2] + C[3] : C[1];
    est[0] = ( resi >> 5 ) + no; est[1] = ( no >> 5 ) + resi;
  }
  if( allowed & 4u )      // SBT_HOR_HALF
  {
    const unsigned long long resi = npy == 4 ? R[0] + R[1] : R[0], no = npy == 4 ? R[2] + R[3] : R[1];
    est[2] = ( resi >> 5 ) + no; est[3] = ( no >> 5 ) + resi;
  }
  if( allowed & 8u )      // SBT_VER_QUAD
  {
    est[4] = ( C[0] + ( ( C[1] + C[2] + C[3] ) << 5 ) ) >> 5;
    est[5] = ( C[3] + ( ( C[0] + C[1] + C[2] ) << 5 ) ) >> 5;
  }
  if( allowed & 16u )     // SBT_HOR_QUAD
  {
    est[6] = ( R[0] + ( ( R[1] + R[2] + R[3] ) << 5 ) ) >> 5;
    est[7] = ( R[3] + ( ( R[0] + R[1] + R[2] ) << 5 ) ) >> 5;
  }
  // the N best of each kind, strict < : a tie goes to the lower mode (:3427-3463)
  unsigned long long t[8];
#pragma unroll
  for( int k = 0; k < 8; k++ ) { t[k] = est[k]; order[k] = 255; }
  const int nHalf = min( 2 * ( int ) ( ( ( allowed >> 1 ) & 1u ) + ( ( allowed >> 2 ) & 1u ) ), 2 ), nQuad = min( 2 * ( int ) ( ( ( allowed >> 3 ) & 1u ) + ( ( allowed >> 4 ) & 1u ) ), 2 );
#pragma unroll
  for( int kind = 0; kind < 2; kind++ )
  {
    const int num = kind ? nQuad : nHalf, start = kind ? nHalf : 0;
#pragma unroll
    for( int r = 0; r < 2; r++ )
    {
      unsigned long long best = MAXD; int sel = 255;
#pragma unroll
      for( int m = 0; m < 4; m++ ) if( t[4 * kind + m] < best ) { best = t[4 * kind + m]; sel = 4 * kind + m; }
      if( r < num )
      {
#pragma unroll
        for( int m = 0; m < 4; m++ ) if( sel == 4 * kind + m ) t[4 * kind + m] = MAXD;
#pragma unroll
        for( int k = 0; k < 4; k++ ) if( start + r == k ) order[k] = ( unsigned char ) sel;
      }
    }
  }
}

// A CU has 16 part slots of L = 2^log2Lanes lanes each (slot p = j * 4 + i of the 4 x 4 frame; slots outside the CU's grid idle), so a part's lanes are an aligned group and
// a CU takes 16 L lanes of the wave: four, two or one CU per wave.  The part sums go to LDS once, and lane 0 of the CU derives the estimates and the order from them.
__global__ void __launch_bounds__( 256 )
sbtPartsKernel( const SbtPartsDev* __restrict__ items, const SbtUnit* __restrict__ units, const int16_t* __restrict__ resi, const double chromaWeight,
                unsigned long long* __restrict__ parts, unsigned long long* __restrict__ est, unsigned char* __restrict__ order )
{
  __shared__ unsigned long long sums[4][4][48];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const SbtUnit u = sbtUnitOfWave( units, blockIdx.x * 4 + wave );
  if( u.n == 0 ) return;
  const int L = 1 << u.log2Lanes, slot = lane >> ( 4 + u.log2Lanes ), li = lane & ( 16 * L - 1 ), p = li >> u.log2Lanes, sub = li & ( L - 1 );
  const int log2NX = sbtLog2Parts( u.log2W ), log2NY = sbtLog2Parts( u.log2H ), i = p & 3, j = p >> 2;
  const bool active = slot < u.n, valid = active && i < ( 1 << log2NX ) && j < ( 1 << log2NY );
  unsigned long long e[3] = { 0, 0, 0 };
  int idx = 0; unsigned allowed = 0;
  if( active )
  {
    const SbtPartsDev it = items[u.first + slot];
    idx = it.idx; allowed = it.allowed;
    if( valid )
    {
      const int log2PW = u.log2W - log2NX, log2PH = u.log2H - log2NY;
      e[0] = sbtEnergyV( u.log2VY, resi + ( ptrdiff_t ) it.off[0] + ( ( ptrdiff_t ) j << log2PH ) * it.strideY + ( i << log2PW ), it.strideY, log2PW, log2PH, sub, L );
#pragma unroll
      for( int c = 1; c < 3; c++ )
        e[c] = sbtEnergyV( u.log2VC, resi + ( ptrdiff_t ) it.off[c] + ( ( ptrdiff_t ) j << ( log2PH - 1 ) ) * it.strideC + ( i << ( log2PW - 1 ) ), it.strideC, log2PW - 1, log2PH - 1, sub, L );
    }
  }
#pragma unroll
  for( int c = 0; c < 3; c++ )
  {
    e[c] = vvhipGroupSum64( e[c], L, lane );      // (per lane at most 256 samples x 2^30 = 2^38)
    if( active && sub == 0 )
    {
      sums[wave][slot][16 * c + p] = e[c];
      if( parts ) parts[( ( ptrdiff_t ) idx * 3 + c ) * 16 + p] = e[c];
    }
  }
  if( !est && !order ) return;
  SBT_WAVE_SYNC();
  if( active && li == 0 )
  {
    unsigned long long d[16];
#pragma unroll
    for( int k = 0; k < 16; k++ )
    {
      // every component's part sum is weighted on its own: ONE IEEE multiplication, truncated toward zero (InterSearch.cpp:3329-3333)
      const double cb = ( double ) sums[wave][slot][16 + k] * chromaWeight, cr = ( double ) sums[wave][slot][32 + k] * chromaWeight;
      d[k] = sums[wave][slot][k] + ( unsigned long long ) cb + ( unsigned long long ) cr;
    }
    unsigned long long m[9]; unsigned char o[8];
    sbtEstimate( d, 1 << log2NX, 1 << log2NY, allowed, m, o );
    if( est )
    {
#pragma unroll
      for( int k = 0; k < 9; k++ ) est[( ptrdiff_t ) idx * 9 + k] = m[k];
    }
    if( order )
    {
#pragma unroll
      for( int k = 0; k < 8; k++ ) order[( ptrdiff_t ) idx * 8 + k] = o[k];
    }
  }
}

// ---- placement ----------------------------------------------------------------------------------------------------------------------------------------------------------
// the coded tile of a component block of 2^log2W x 2^log2H samples (getSbtTuTiling's factors ( dim * f ) >> 2): mode = 2 * ( sbtIdx - 1 ) + sbtPos
struct SbtRect { int x, y, w, h; };
__host__ __device__ inline SbtRect sbtCodedTile( int w, int h, int mode )
{
  const bool ver = !( ( mode >> 1 ) & 1 ), quad = mode >= 4, pos1 = mode & 1;
  const int side = ver ? w : h, len = ( side * ( quad ? 1 : 2 ) ) >> 2, at = pos1 ? ( side * ( quad ? 3 : 2 ) ) >> 2 : 0;
  SbtRect r;
  r.x = ver ? at : 0; r.y = ver ? 0 : at; r.w = ver ? len : w; r.h = ver ? h : len;
  return r;
}

template<int V>
__device__ __forceinline__ unsigned long long sbtPlaceComp( int16_t* __restrict__ rec, const int16_t* __restrict__ org, const int16_t* __restrict__ tileRec, ptrdiff_t off, int stride,
                                                            int log2W, int log2H, const SbtRect t, bool zero, bool wantSse, int li, int G )
{
  const int log2SegsRow = log2W - ilog2c( V ), segs = 1 << ( log2W + log2H - ilog2c( V ) );
  unsigned long long e = 0;
  for( int s = li; s < segs; s += G )
  {
    const int y = s >> log2SegsRow, x = ( s & ( ( 1 << log2SegsRow ) - 1 ) ) * V;
    const bool inTile = !zero && x >= t.x && x < t.x + t.w && y >= t.y && y < t.y + t.h;
    SbtSeg<V> r;
#pragma unroll
    for( int k = 0; k < V; k++ ) r.v[k] = 0;
    if( inTile ) r = *reinterpret_cast<const SbtSeg<V>*>( tileRec + ( ptrdiff_t ) ( y - t.y ) * t.w + ( x - t.x ) );
    const ptrdiff_t at = off + ( ptrdiff_t ) y * stride + x;
    if( rec ) *reinterpret_cast<SbtSeg<V>*>( rec + at ) = r;
    if( wantSse )
    {
      const SbtSeg<V> o = *reinterpret_cast<const SbtSeg<V>*>( org + at );
#pragma unroll
      for( int k = 0; k < V; k++ ) { const long long a = ( int ) r.v[k] - ( int ) o.v[k]; e += ( unsigned long long ) ( a * a ); }
    }
  }
  return e;
}

__global__ void __launch_bounds__( 256 )
sbtPlaceKernel( const SbtPlaceDev* __restrict__ items, const SbtUnit* __restrict__ units, const int16_t* __restrict__ tileRec, const vvhip_tu_stats* __restrict__ stats,
                int16_t* __restrict__ rec, const int16_t* __restrict__ org, unsigned long long* __restrict__ sse )
{
  const int lane = threadIdx.x & 63;
  const SbtUnit u = sbtUnitOfWave( units, blockIdx.x * 4 + ( threadIdx.x >> 6 ) );
  if( u.n == 0 ) return;
  const int G = 1 << u.log2Lanes, sub = lane >> u.log2Lanes, li = lane & ( G - 1 );
  const bool active = sub < u.n, wantSse = sse != nullptr;
  unsigned long long e[3] = { 0, 0, 0 };
  int idx = 0;
  if( active )
  {
    const SbtPlaceDev it = items[u.first + sub];
    idx = it.idx;
#pragma unroll
    for( int c = 0; c < 3; c++ )
    {
      const int lw = u.log2W - ( c ? 1 : 0 ), lh = u.log2H - ( c ? 1 : 0 ), stride = c ? it.strideC : it.strideY, log2V = c ? u.log2VC : u.log2VY;
      const SbtRect t = sbtCodedTile( 1 << lw, 1 << lh, it.mode );
      // no statistics entry: the caller dropped the component's coefficients; an entry without levels: the tile is all zero and never read (sparse outputs leave it unspecified)
      const bool zero = it.statsIdx[c] < 0 || stats[it.statsIdx[c]].abs_sum == 0;
      const int16_t* tr = tileRec + ( ptrdiff_t ) it.tileOff[c];
      switch( log2V )
      {
      case 3:  e[c] = sbtPlaceComp<8>( rec, org, tr, it.off[c], stride, lw, lh, t, zero, wantSse, li, G ); break;
      case 2:  e[c] = sbtPlaceComp<4>( rec, org, tr, it.off[c], stride, lw, lh, t, zero, wantSse, li, G ); break;
      case 1:  e[c] = sbtPlaceComp<2>( rec, org, tr, it.off[c], stride, lw, lh, t, zero, wantSse, li, G ); break;
      default: e[c] = sbtPlaceComp<1>( rec, org, tr, it.off[c], stride, lw, lh, t, zero, wantSse, li, G ); break;
      }
    }
  }
  if( !wantSse ) return;
#pragma unroll
  for( int c = 0; c < 3; c++ )
  {
    e[c] = vvhipGroupSum64( e[c], G, lane );      // (per lane at most 64 samples x 65535^2 < 2^39)
    if( active && li == 0 ) sse[3 * ( ptrdiff_t ) idx + c] = e[c];
  }
}

// ---- host: validation, size classes, the cached schedule ----------------------------------------------------------------------------------------------------------------
// samples of alignment of an offset / a pointer, capped at 8 (16 bytes)
inline int sbtAlignOf( uint64_t v ) { return v == 0 ? 8 : ( int ) std::min<uint64_t>( 8, v & ( ~v + 1 ) ); }

inline int sbtPtrAlign( std::initializer_list<const void*> ptrs )
{
  int a = 8;
  for( const void* p : ptrs ) if( p ) a = std::min( a, sbtAlignOf( ( uint64_t ) ( uintptr_t ) p >> 1 ) );
  return a;
}

// the geometry every SBT item shares; -> 0 or the failure's code
int sbtCheckCu( vvhip_ctx* ctx, const char* entry, int i, int width, int height, const int32_t ( &off )[3], int strideY, int strideC, unsigned allowed, const uint8_t* rsv, int nRsv )
{
  if( !isPow2( width ) || !isPow2( height ) || width < 4 || height < 4 || width > 64 || height > 64 )
    return vvhip_fail( ctx, VVHIP_E_ARG, "%s: item %d: CU %dx%d (width and height powers of two, 4..64)", entry, i, width, height );
  if( strideY < width || strideC < width / 2 )
    return vvhip_fail( ctx, VVHIP_E_ARG, "%s: item %d: row pitches %d / %d below the widths %d / %d", entry, i, strideY, strideC, width, width / 2 );
  if( off[0] < 0 || off[1] < 0 || off[2] < 0 ) return vvhip_fail( ctx, VVHIP_E_ARG, "%s: item %d: negative offset (Y %d, Cb %d, Cr %d)", entry, i, off[0], off[1], off[2] );
  const unsigned can = ( width >= 8 ? 2u : 0u ) | ( height >= 8 ? 4u : 0u ) | ( width >= 16 ? 8u : 0u ) | ( height >= 16 ? 16u : 0u );
  if( allowed == 0 ) return vvhip_fail( ctx, VVHIP_E_ARG, "%s: item %d: sbt_allowed is 0 (a CU without SBT has no part estimates: its SSE is a distortion list's)", entry, i );
  if( allowed & ~can )
    return vvhip_fail( ctx, VVHIP_E_ARG, "%s: item %d: sbt_allowed 0x%x on a %dx%d CU (half modes need a side of 8, quad modes a side of 16: 0x%x at most)", entry, i, allowed, width, height, can );
  for( int k = 0; k < nRsv; k++ ) if( rsv[k] ) return vvhip_fail( ctx, VVHIP_E_ARG, "%s: item %d: non-zero reserved bytes", entry, i );
  return VVHIP_OK;
}

struct SbtHead { size_t offItems, offUnits; int units; };      // the head of a schedule's blob: where the sorted items and the wave units lie, the number of units
// size class: the most samples first (their waves run longest), then shape and the two vector widths — a wave never mixes classes; inside a class in buffer order
inline uint32_t sbtClass( int log2W, int log2H, int vY, int vC ) { return ( ( uint32_t ) ( 12 - log2W - log2H ) << 12 ) | ( ( uint32_t ) log2W << 8 ) | ( ( uint32_t ) ilog2i( vY ) << 4 ) | ( uint32_t ) ilog2i( vC ); }

// sorts the device items by class, cuts every class into waves and uploads both; on success the slot's key names the list it belongs to
template<class Dev, class LanesOf>
int sbtUploadSchedule( vvhip_ctx* ctx, HostList& S, const std::vector<Dev>& dev, std::vector<ListKeyed>& order, LanesOf log2LanesOf, std::vector<unsigned char>& key )
{
  const int n = ( int ) dev.size();
  std::sort( order.begin(), order.end() );
  std::vector<Dev> sorted( n );
  std::vector<SbtUnit> units;
  for( int c0 = 0; c0 < n; )
  {
    int c1 = c0; while( c1 < n && order[c1].cls == order[c0].cls ) c1++;
    const uint32_t cls = order[c0].cls;
    const int log2W = ( int ) ( ( cls >> 8 ) & 15u ), log2H = 12 - log2W - ( int ) ( cls >> 12 ), log2VY = ( int ) ( ( cls >> 4 ) & 15u ), log2VC = ( int ) ( cls & 15u );
    int log2Lanes = 0;
    const int perWave = log2LanesOf( log2W, log2H, log2VY, &log2Lanes );
    for( int k = c0; k < c1; k++ ) sorted[k] = dev[order[k].idx];
    for( int k = c0; k < c1; k += perWave )
    {
      SbtUnit u; memset( &u, 0, sizeof( u ) );
      u.first = k; u.n = ( int16_t ) std::min( perWave, c1 - k ); u.log2W = ( uint8_t ) log2W; u.log2H = ( uint8_t ) log2H; u.log2VY = ( uint8_t ) log2VY; u.log2VC = ( uint8_t ) log2VC;
      u.log2Lanes = ( uint8_t ) log2Lanes;
      units.push_back( u );
    }
    c0 = c1;
  }
  SbtUnit none; memset( &none, 0, sizeof( none ) );
  while( units.size() & 3 ) units.push_back( none );      // four waves per workgroup

  SbtHead H;
  ListBlob blob( &H, sizeof( H ) );
  H.offItems = blob.add( sorted.data(), sorted.size() * sizeof( Dev ) );
  H.offUnits = blob.add( units.data(), units.size() * sizeof( SbtUnit ) );
  H.units = ( int ) units.size();
  return listUpload( ctx, S, blob, &key );
}

template<class Item>
std::vector<unsigned char> sbtKey( int ptrAlign, const Item* items_host, int n )
{
  std::vector<unsigned char> key( 1 + ( size_t ) n * sizeof( Item ) );
  key[0] = ( unsigned char ) ptrAlign;
  memcpy( key.data() + 1, items_host, ( size_t ) n * sizeof( Item ) );
  return key;
}

} // namespace

extern "C" {

int vvhip_sbt_tiles( const vvhip_sbt_item* cu, int mode, vvhip_sbt_tile* out )
{
  if( !cu || !out || mode < 0 || mode > 7 || !isPow2( cu->width ) || !isPow2( cu->height ) || cu->width < 4 || cu->height < 4 || cu->width > 64 || cu->height > 64 ) return VVHIP_E_ARG;
  const bool ver = !( ( mode >> 1 ) & 1 ), quad = mode >= 4, pos1 = mode & 1;
  if( ( ver ? cu->width : cu->height ) < ( quad ? 16 : 8 ) ) return VVHIP_E_ARG;
  const int32_t off[3] = { cu->y_off, cu->cb_off, cu->cr_off };
  for( int c = 0; c < 3; c++ )
  {
    const int w = cu->width >> ( c ? 1 : 0 ), h = cu->height >> ( c ? 1 : 0 ), stride = c ? cu->stride_c : cu->stride_y;
    const SbtRect t = sbtCodedTile( w, h, mode );
    vvhip_sbt_tile& o = out[c];
    memset( &o, 0, sizeof( o ) );
    o.resi_off = off[c] + t.y * stride + t.x; o.stride = stride;
    o.x = ( int16_t ) t.x; o.y = ( int16_t ) t.y; o.width = ( int16_t ) t.w; o.height = ( int16_t ) t.h;
    o.tr_hor = o.tr_ver = VVHIP_DCT2;
    // TrQuant::xSetTrTypes, the SBT branch (TrQuant.cpp:435-466): luma only; DCT-2 when the tile's side ALONG the split line exceeds MTS_INTER_MAX_CU_SIZE (32) — the height
    // of a vertically split CU's tile, the width of a horizontally split one's; the side across it is at most 32 by construction
    if( c == 0 && ( ver ? t.h : t.w ) <= 32 )
    {
      o.tr_hor = ( int8_t ) ( ver && !pos1 ? VVHIP_DCT8 : VVHIP_DST7 );
      o.tr_ver = ( int8_t ) ( !ver && !pos1 ? VVHIP_DCT8 : VVHIP_DST7 );
    }
  }
  return VVHIP_OK;
}

int vvhip_sbt_parts_batch( vvhip_ctx* ctx, const int16_t* d_resi, const vvhip_sbt_item* items_host, int n, double chroma_weight, uint64_t* d_parts, uint64_t* d_est, uint8_t* d_order )
{
  static const char* const entry = "vvhip_sbt_parts_batch";
  if( !ctx ) return VVHIP_E_ARG;
  if( n < 0 || n > ( 1 << 24 ) || ( n && ( !items_host || !d_resi ) ) || ( ( uintptr_t ) d_resi & 1 ) || ( ( uintptr_t ) d_parts & 7 ) || ( ( uintptr_t ) d_est & 7 ) )
    return vvhip_fail( ctx, VVHIP_E_ARG, "%s: %d items at %p, residual %p (an int16 array), part sums %p, estimates %p (uint64 arrays)", entry, n, ( const void* ) items_host,
                       ( const void* ) d_resi, ( void* ) d_parts, ( void* ) d_est );
  if( !( chroma_weight >= 0.0 ) || chroma_weight > 65536.0 ) return vvhip_fail( ctx, VVHIP_E_ARG, "%s: chroma weight %g (0..65536)", entry, chroma_weight );
  if( n == 0 ) return VVHIP_OK;
  HostList& S = ctx->list[LIST_SBT_PARTS];
  const int ptrAlign = sbtPtrAlign( { d_resi } );
  std::vector<unsigned char> key = sbtKey( ptrAlign, items_host, n );
  bool current = false;
  int rc = listCurrent( ctx, S, key, &current );
  if( rc ) return rc;
  if( !current )
  {
    std::vector<SbtPartsDev> dev( n );
    std::vector<ListKeyed> order( n );
    for( int i = 0; i < n; i++ )
    {
      const vvhip_sbt_item& it = items_host[i];
      const int32_t off[3] = { it.y_off, it.cb_off, it.cr_off };
      if( ( rc = sbtCheckCu( ctx, entry, i, it.width, it.height, off, it.stride_y, it.stride_c, it.sbt_allowed, it.rsv, 3 ) ) ) return rc;
      SbtPartsDev& d = dev[i];
      memset( &d, 0, sizeof( d ) );
      d.off[0] = off[0]; d.off[1] = off[1]; d.off[2] = off[2]; d.strideY = it.stride_y; d.strideC = it.stride_c; d.idx = i; d.allowed = it.sbt_allowed;
      const int log2W = ilog2i( it.width ), log2H = ilog2i( it.height ), partW = it.width >> sbtLog2Parts( log2W );      // a segment never straddles a part boundary
      const int vY = std::min( { partW, ptrAlign, sbtAlignOf( ( uint32_t ) it.y_off ), sbtAlignOf( ( uint32_t ) it.stride_y ) } );
      const int vC = std::min( { partW / 2, ptrAlign, sbtAlignOf( ( uint32_t ) it.cb_off ), sbtAlignOf( ( uint32_t ) it.cr_off ), sbtAlignOf( ( uint32_t ) it.stride_c ) } );
      order[i].cls = sbtClass( log2W, log2H, vY, vC ); order[i].pos = it.y_off; order[i].idx = i;
    }
    // lanes per part: one up to 256 luma samples per CU, two up to 1024, four above — 16 part slots per CU
    rc = sbtUploadSchedule( ctx, S, dev, order, []( int log2W, int log2H, int, int* log2Lanes ) { *log2Lanes = log2W + log2H <= 8 ? 0 : log2W + log2H <= 10 ? 1 : 2; return 4 >> *log2Lanes; }, key );
    if( rc ) return rc;
  }
  const SbtHead& H = listHead<SbtHead>( S );
  const char* base = static_cast<const char*>( S.d );
  hipLaunchKernelGGL( sbtPartsKernel, dim3( ( unsigned ) ( H.units / 4 ) ), dim3( 256 ), 0, ctx->stream, reinterpret_cast<const SbtPartsDev*>( base + H.offItems ),
                      reinterpret_cast<const SbtUnit*>( base + H.offUnits ), d_resi, chroma_weight, reinterpret_cast<unsigned long long*>( d_parts ),
                      reinterpret_cast<unsigned long long*>( d_est ), d_order );
  VVHIP_LAUNCH_CHECK( ctx );
  return listLaunched( ctx, S );
}

int vvhip_sbt_place_batch( vvhip_ctx* ctx, const int16_t* d_tile_rec, const vvhip_sbt_place_item* items_host, int n, const vvhip_tu_stats* d_stats, int16_t* d_rec,
                           const int16_t* d_org_resi, uint64_t* d_sse )
{
  static const char* const entry = "vvhip_sbt_place_batch";
  if( !ctx ) return VVHIP_E_ARG;
  if( n < 0 || n > ( 1 << 24 ) || ( n && !items_host ) || ( d_sse && !d_org_resi ) || ( ( uintptr_t ) d_tile_rec & 1 ) || ( ( uintptr_t ) d_rec & 1 ) || ( ( uintptr_t ) d_org_resi & 1 ) ||
      ( ( uintptr_t ) d_sse & 7 ) )
    return vvhip_fail( ctx, VVHIP_E_ARG, "%s: %d items at %p, tile reconstructions %p, reconstruction %p, original residual %p (int16 arrays), SSEs %p (a uint64 array; SSEs need the original residual)",
                       entry, n, ( const void* ) items_host, ( const void* ) d_tile_rec, ( void* ) d_rec, ( const void* ) d_org_resi, ( void* ) d_sse );
  if( n == 0 ) return VVHIP_OK;
  HostList& S = ctx->list[LIST_SBT_PLACE];
  const int ptrAlign = sbtPtrAlign( { d_tile_rec, d_rec, d_sse ? d_org_resi : nullptr } );
  std::vector<unsigned char> key = sbtKey( ptrAlign, items_host, n );
  key.push_back( ( unsigned char ) ( ( d_stats ? 1 : 0 ) | ( d_tile_rec ? 2 : 0 ) ) );      // (what the validation below depends on beside the items)
  bool current = false;
  int rc = listCurrent( ctx, S, key, &current );
  if( rc ) return rc;
  if( !current )
  {
    std::vector<SbtPlaceDev> dev( n );
    std::vector<ListKeyed> order( n );
    for( int i = 0; i < n; i++ )
    {
      const vvhip_sbt_place_item& it = items_host[i];
      const int32_t off[3] = { it.y_off, it.cb_off, it.cr_off };
      if( ( rc = sbtCheckCu( ctx, entry, i, it.width, it.height, off, it.stride_y, it.stride_c, it.sbt_allowed, it.rsv, 2 ) ) ) return rc;
      if( it.mode > 7 ) return vvhip_fail( ctx, VVHIP_E_ARG, "%s: item %d: SBT mode %d (0..7)", entry, i, it.mode );
      if( !( ( it.sbt_allowed >> ( 1 + ( it.mode >> 1 ) ) ) & 1 ) )
        return vvhip_fail( ctx, VVHIP_E_ARG, "%s: item %d: SBT mode %d is of a type that sbt_allowed 0x%x does not hold", entry, i, it.mode, it.sbt_allowed );
      SbtPlaceDev& d = dev[i];
      memset( &d, 0, sizeof( d ) );
      d.strideY = it.stride_y; d.strideC = it.stride_c; d.idx = i; d.mode = it.mode;
      int v[2] = { 8, 8 };
      for( int c = 0; c < 3; c++ )
      {
        if( it.stats_idx[c] < -1 ) return vvhip_fail( ctx, VVHIP_E_ARG, "%s: item %d: component %d: statistics entry %d (an index, or -1 for a component without coefficients)", entry, i, c, it.stats_idx[c] );
        if( it.stats_idx[c] >= 0 && ( !d_stats || !d_tile_rec ) )
          return vvhip_fail( ctx, VVHIP_E_ARG, "%s: item %d: component %d names statistics entry %d and there are no %s", entry, i, c, it.stats_idx[c], d_stats ? "tile reconstructions" : "statistics" );
        if( it.stats_idx[c] >= 0 && it.tile_off[c] < 0 ) return vvhip_fail( ctx, VVHIP_E_ARG, "%s: item %d: component %d: negative tile offset %d", entry, i, c, it.tile_off[c] );
        d.off[c] = off[c]; d.tileOff[c] = it.stats_idx[c] >= 0 ? it.tile_off[c] : 0; d.statsIdx[c] = it.stats_idx[c];
        const SbtRect t = sbtCodedTile( it.width >> ( c ? 1 : 0 ), it.height >> ( c ? 1 : 0 ), it.mode );      // a segment never straddles the tile's boundary
        v[c ? 1 : 0] = std::min( { v[c ? 1 : 0], t.w, ptrAlign, sbtAlignOf( ( uint32_t ) off[c] ), sbtAlignOf( ( uint32_t ) ( c ? it.stride_c : it.stride_y ) ), sbtAlignOf( ( uint32_t ) d.tileOff[c] ) } );
      }
      order[i].cls = sbtClass( ilog2i( it.width ), ilog2i( it.height ), v[0], v[1] ); order[i].pos = it.y_off; order[i].idx = i;
    }
    rc = sbtUploadSchedule( ctx, S, dev, order, []( int log2W, int log2H, int log2VY, int* log2Lanes ) { *log2Lanes = std::min( 6, log2W + log2H - log2VY ); return 64 >> *log2Lanes; }, key );
    if( rc ) return rc;
  }
  const SbtHead& H = listHead<SbtHead>( S );
  const char* base = static_cast<const char*>( S.d );
  hipLaunchKernelGGL( sbtPlaceKernel, dim3( ( unsigned ) ( H.units / 4 ) ), dim3( 256 ), 0, ctx->stream, reinterpret_cast<const SbtPlaceDev*>( base + H.offItems ),
                      reinterpret_cast<const SbtUnit*>( base + H.offUnits ), d_tile_rec, d_stats, d_rec, d_sse ? d_org_resi : nullptr, reinterpret_cast<unsigned long long*>( d_sse ) );
  VVHIP_LAUNCH_CHECK( ctx );
  return listLaunched( ctx, S );
}

} // extern "C"
