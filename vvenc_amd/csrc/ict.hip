// ict.hip — joint Cb-Cr residual coding (ICT) around the fused TU pipeline: vvhip_ict_fwd_batch / vvhip_ict_inv_batch (gfx950 only).
//
// What TrQuant::fwdTransformICT / invTransformICT do for one chroma TU (CommonLib/TrQuant.cpp:95-164, :350-362), for a LIST of TUs of mixed sizes in one launch:
//   forward : one joint block from the Cb and the Cr residual + the pair distortion ( d1, d2 ) selectICTCandidates compares (:364-410)
//   inverse : both reconstructed residuals from the joint reconstruction + their SSEs against the original residuals (InterSearch.cpp:3896-3935)
// All six non-zero signed modes are ONE arithmetic, its integers derived per item from the mode (ictMode: a, b, sgn and a shift) without a divergent branch:
//   c     = Pel( ( a * cb + b * cr ) / D ),  D = 5 for |m| = 1, 3 and 2 for |m| = 2        — the coded component X (Cb for |m| <= 2, Cr for |m| = 3)
//   other = ( sgn * c ) >> ( |m| != 2 )                                                  — the derived component Y
//   d1    = ( X - c )^2 + ( Y - other )^2
// Elementwise work with two reductions per item: every lane moves segments of V samples (V = 8, 4, 2 or 1: the widest vector the item's offsets, pitch, width and the
// call's base pointers allow), an item's lanes are an aligned group of a wave, reduced with DPP only, then ONE 64-bit store per item and value — no atomics.
#include "common.h"
#include <algorithm>
#include <initializer_list>
#include <string.h>

namespace {

__host__ __device__ constexpr int ilog2c( int v ) { return v >= 8 ? 3 : v >= 4 ? 2 : v >= 2 ? 1 : 0; }

struct IctDev  { int32_t cbOff, crOff, stride, jointOff, statsIdx, idx; int8_t mode; uint8_t pad[3]; };      // one item as the kernels read it; idx: its place in the caller's list (d_dist / d_sse)
struct IctUnit { int32_t first; int16_t n; uint8_t log2W, log2H, log2V, log2Lanes, pad[2]; };               // what one wave does: n items of one class from items[first]; n == 0: nothing

template<int V> struct __attribute__( ( aligned( V * 2 ) ) ) IctSeg { int16_t v[V]; };

struct IctMode { int a, b, sgn, sh; bool five, crCoded, zero; };
__device__ __forceinline__ IctMode ictMode( int m )
{
  IctMode r;
  const int am = m < 0 ? -m : m, s = m < 0 ? -1 : 1;
  r.zero = m == 0; r.crCoded = am == 3; r.five = am != 2; r.sgn = s; r.sh = am != 2 ? 1 : 0;
  r.a = am == 2 ? 1 : am == 3 ? 2 * s : 4;      // weight of cb
  r.b = am == 2 ? s : am == 3 ? 4 : 2 * s;      // weight of cr
  return r;
}

template<int V>
__device__ __forceinline__ void ictFwdBody( const IctDev* __restrict__ items, const IctUnit u, const int lane, const int16_t* __restrict__ resi, int16_t* __restrict__ joint,
                                            int64_t* __restrict__ dist )
{
  const int G = 1 << u.log2Lanes, sub = lane >> u.log2Lanes, li = lane & ( G - 1 );
  const bool active = sub < u.n;
  unsigned long long d1 = 0, d2 = 0;
  int idx = 0;
  if( active )
  {
    const IctDev it = items[u.first + sub];
    const IctMode m = ictMode( it.mode );
    idx = it.idx;
    const int log2SegsRow = u.log2W - ilog2c( V ), segs = 1 << ( u.log2W + u.log2H - ilog2c( V ) ), w = 1 << u.log2W;
    for( int s = li; s < segs; s += G )
    {
      const int y = s >> log2SegsRow, x = ( s & ( ( 1 << log2SegsRow ) - 1 ) ) * V;
      const IctSeg<V> cb = *reinterpret_cast<const IctSeg<V>*>( resi + ( ptrdiff_t ) it.cbOff + ( ptrdiff_t ) y * it.stride + x );
      const IctSeg<V> cr = *reinterpret_cast<const IctSeg<V>*>( resi + ( ptrdiff_t ) it.crOff + ( ptrdiff_t ) y * it.stride + x );
      IctSeg<V> c;
#pragma unroll
      for( int k = 0; k < V; k++ )
      {
        const int cbx = cb.v[k], crx = cr.v[k];
        const int t = m.a * cbx + m.b * crx;
        const int cj = ( int16_t ) ( m.five ? t / 5 : t / 2 );      // Pel( ... ): wraps at the int16 extremes
        c.v[k] = ( int16_t ) cj;
        const int other = ( m.sgn * cj ) >> m.sh;
        const long long ex = ( m.crCoded ? crx : cbx ) - cj, ey = ( m.crCoded ? cbx : crx ) - other;
        d1 += m.zero ? ( unsigned long long ) ( ( long long ) cbx * cbx ) : ( unsigned long long ) ( ex * ex + ey * ey );
        d2 += m.zero ? ( unsigned long long ) ( ( long long ) crx * crx ) : 0ull;
      }
      if( !m.zero ) *reinterpret_cast<IctSeg<V>*>( joint + ( ptrdiff_t ) it.jointOff + ( ptrdiff_t ) y * w + x ) = c;
    }
  }
  if( !dist ) return;
  d1 = vvhipGroupSum64( d1, G, lane );      // (per lane at most 64 samples x 2 x 98303^2 < 2^41)
  d2 = vvhipGroupSum64( d2, G, lane );
  if( active && li == 0 ) { dist[2 * ( ptrdiff_t ) idx] = ( int64_t ) d1; dist[2 * ( ptrdiff_t ) idx + 1] = ( int64_t ) d2; }
}

template<int V>
__device__ __forceinline__ void ictInvBody( const IctDev* __restrict__ items, const IctUnit u, const int lane, const int16_t* __restrict__ jointRec,
                                            const vvhip_tu_stats* __restrict__ stats, int16_t* __restrict__ rec, const int16_t* __restrict__ org, uint64_t* __restrict__ sse )
{
  const int G = 1 << u.log2Lanes, sub = lane >> u.log2Lanes, li = lane & ( G - 1 );
  const bool active = sub < u.n;
  unsigned long long eCb = 0, eCr = 0;
  int idx = 0;
  if( active )
  {
    const IctDev it = items[u.first + sub];
    const IctMode m = ictMode( it.mode );
    idx = it.idx;
    const bool allZero = it.statsIdx >= 0 && stats[it.statsIdx].abs_sum == 0;      // the joint reconstruction is taken as zero and not read (InterSearch.cpp:3896-3899)
    const int log2SegsRow = u.log2W - ilog2c( V ), segs = 1 << ( u.log2W + u.log2H - ilog2c( V ) ), w = 1 << u.log2W;
    for( int s = li; s < segs; s += G )
    {
      const int y = s >> log2SegsRow, x = ( s & ( ( 1 << log2SegsRow ) - 1 ) ) * V;
      const ptrdiff_t pCb = ( ptrdiff_t ) it.cbOff + ( ptrdiff_t ) y * it.stride + x, pCr = ( ptrdiff_t ) it.crOff + ( ptrdiff_t ) y * it.stride + x;
      IctSeg<V> c;
      if( allZero ) { for( int k = 0; k < V; k++ ) c.v[k] = 0; }
      else c = *reinterpret_cast<const IctSeg<V>*>( jointRec + ( ptrdiff_t ) it.jointOff + ( ptrdiff_t ) y * w + x );
      IctSeg<V> o;
#pragma unroll
      for( int k = 0; k < V; k++ ) o.v[k] = ( int16_t ) ( ( m.sgn * ( int ) c.v[k] ) >> m.sh );      // narrowed as the Pel store does: -( -32768 ) wraps
      const IctSeg<V> rCb = m.crCoded ? o : c, rCr = m.crCoded ? c : o;
      if( rec )
      {
        *reinterpret_cast<IctSeg<V>*>( rec + pCb ) = rCb;
        *reinterpret_cast<IctSeg<V>*>( rec + pCr ) = rCr;
      }
      if( sse )
      {
        const IctSeg<V> oCb = *reinterpret_cast<const IctSeg<V>*>( org + pCb ), oCr = *reinterpret_cast<const IctSeg<V>*>( org + pCr );
#pragma unroll
        for( int k = 0; k < V; k++ )
        {
          const long long a = ( int ) rCb.v[k] - ( int ) oCb.v[k], b = ( int ) rCr.v[k] - ( int ) oCr.v[k];
          eCb += ( unsigned long long ) ( a * a ); eCr += ( unsigned long long ) ( b * b );
        }
      }
    }
  }
  if( !sse ) return;
  eCb = vvhipGroupSum64( eCb, G, lane );      // (per lane at most 64 samples x 65535^2 < 2^39)
  eCr = vvhipGroupSum64( eCr, G, lane );
  if( active && li == 0 ) { sse[2 * ( ptrdiff_t ) idx] = eCb; sse[2 * ( ptrdiff_t ) idx + 1] = eCr; }
}

__device__ __forceinline__ IctUnit ictUnitOfWave( const IctUnit* __restrict__ units, int wave )
{
  // one record per wave: the same address in every lane, made scalar so that the class switch and the loop bounds are wave-uniform
  const int32_t* p = reinterpret_cast<const int32_t*>( units + wave );
  const int32_t w0 = __builtin_amdgcn_readfirstlane( p[0] ), w1 = __builtin_amdgcn_readfirstlane( p[1] ), w2 = __builtin_amdgcn_readfirstlane( p[2] );
  IctUnit u;
  u.first = w0; u.n = ( int16_t ) ( w1 & 0xFFFF ); u.log2W = ( uint8_t ) ( ( w1 >> 16 ) & 0xFF ); u.log2H = ( uint8_t ) ( ( w1 >> 24 ) & 0xFF );
  u.log2V = ( uint8_t ) ( w2 & 0xFF ); u.log2Lanes = ( uint8_t ) ( ( w2 >> 8 ) & 0xFF ); u.pad[0] = u.pad[1] = 0;
  return u;
}

__global__ void __launch_bounds__( 256 )
ictFwdKernel( const IctDev* __restrict__ items, const IctUnit* __restrict__ units, const int16_t* __restrict__ resi, int16_t* __restrict__ joint, int64_t* __restrict__ dist )
{
  const int lane = threadIdx.x & 63;
  const IctUnit u = ictUnitOfWave( units, blockIdx.x * 4 + ( threadIdx.x >> 6 ) );
  if( u.n == 0 ) return;
  switch( u.log2V )
  {
  case 3:  ictFwdBody<8>( items, u, lane, resi, joint, dist ); break;
  case 2:  ictFwdBody<4>( items, u, lane, resi, joint, dist ); break;
  case 1:  ictFwdBody<2>( items, u, lane, resi, joint, dist ); break;
  default: ictFwdBody<1>( items, u, lane, resi, joint, dist ); break;
  }
}

__global__ void __launch_bounds__( 256 )
ictInvKernel( const IctDev* __restrict__ items, const IctUnit* __restrict__ units, const int16_t* __restrict__ jointRec, const vvhip_tu_stats* __restrict__ stats,
              int16_t* __restrict__ rec, const int16_t* __restrict__ org, uint64_t* __restrict__ sse )
{
  const int lane = threadIdx.x & 63;
  const IctUnit u = ictUnitOfWave( units, blockIdx.x * 4 + ( threadIdx.x >> 6 ) );
  if( u.n == 0 ) return;
  switch( u.log2V )
  {
  case 3:  ictInvBody<8>( items, u, lane, jointRec, stats, rec, org, sse ); break;
  case 2:  ictInvBody<4>( items, u, lane, jointRec, stats, rec, org, sse ); break;
  case 1:  ictInvBody<2>( items, u, lane, jointRec, stats, rec, org, sse ); break;
  default: ictInvBody<1>( items, u, lane, jointRec, stats, rec, org, sse ); break;
  }
}

// ---- host: validation, size classes, the cached schedule ----------------------------------------------------------------------------------------------------------------
// samples of alignment of an offset / a pointer, capped at 8 (16 bytes)
inline int ictAlignOf( uint64_t v ) { return v == 0 ? 8 : ( int ) std::min<uint64_t>( 8, v & ( ~v + 1 ) ); }

struct IctHead { size_t offItems, offUnits; int units; };      // the head of a schedule's blob: where the sorted items and the wave units lie, the number of units

inline HostList& ictSlot( vvhip_ctx* ctx, int dir ) { return ctx->list[dir ? LIST_ICT_INV : LIST_ICT_FWD]; }

// validates the list, derives the schedule and uploads it; on success the slot's key names the list it belongs to
int ictBuildSchedule( vvhip_ctx* ctx, const char* entry, int dir, const vvhip_ict_item* items_host, int n, int ptrAlign, std::vector<unsigned char>& key )
{
  std::vector<IctDev> dev( n );
  std::vector<ListKeyed> order( n );
  for( int i = 0; i < n; i++ )
  {
    const vvhip_ict_item& it = items_host[i];
    if( !isPow2( it.width ) || !isPow2( it.height ) || it.width < 2 || it.height < 2 || it.width > 64 || it.height > 64 )
      return vvhip_fail( ctx, VVHIP_E_ARG, "%s: item %d: block %dx%d (width and height powers of two, 2..64)", entry, i, it.width, it.height );
    if( it.stride < it.width ) return vvhip_fail( ctx, VVHIP_E_ARG, "%s: item %d: row pitch %d below the width %d", entry, i, it.stride, it.width );
    if( it.cb_off < 0 || it.cr_off < 0 || it.joint_off < 0 )
      return vvhip_fail( ctx, VVHIP_E_ARG, "%s: item %d: negative offset (Cb %d, Cr %d, joint %d)", entry, i, it.cb_off, it.cr_off, it.joint_off );
    if( it.mode < -3 || it.mode > 3 || ( dir == 1 && it.mode == 0 ) )
      return vvhip_fail( ctx, VVHIP_E_ARG, "%s: item %d: ICT mode %d (%s)", entry, i, it.mode, dir == 1 ? "-3..3 without 0: mode 0 codes no joint block" : "-3..3" );
    if( it.rsv[0] || it.rsv[1] || it.rsv[2] ) return vvhip_fail( ctx, VVHIP_E_ARG, "%s: item %d: non-zero reserved bytes", entry, i );
    IctDev& d = dev[i];
    memset( &d, 0, sizeof( d ) );
    d.cbOff = it.cb_off; d.crOff = it.cr_off; d.stride = it.stride; d.jointOff = it.joint_off; d.statsIdx = dir == 1 ? it.stats_idx : -1; d.idx = i; d.mode = it.mode;
    const int v = std::min( { ( int ) it.width, ptrAlign, ictAlignOf( ( uint32_t ) it.cb_off ), ictAlignOf( ( uint32_t ) it.cr_off ), ictAlignOf( ( uint32_t ) it.stride ),
                              ictAlignOf( ( uint32_t ) it.joint_off ) } );
    // size class: the most samples first (their waves run longest), then shape and vector width — a wave never mixes classes; inside a class in buffer order
    order[i].cls = ( ( uint32_t ) ( 12 - ilog2i( it.width ) - ilog2i( it.height ) ) << 8 ) | ( ( uint32_t ) ilog2i( it.width ) << 4 ) | ( uint32_t ) ilog2i( v );
    order[i].pos = it.cb_off;
    order[i].idx = i;
  }
  std::sort( order.begin(), order.end() );

  std::vector<IctDev> sorted( n );
  std::vector<IctUnit> units;
  for( int c0 = 0; c0 < n; )
  {
    int c1 = c0; while( c1 < n && order[c1].cls == order[c0].cls ) c1++;
    const vvhip_ict_item& f = items_host[order[c0].idx];
    const int log2V = ( int ) ( order[c0].cls & 15u ), log2W = ilog2i( f.width ), log2H = ilog2i( f.height );
    const int log2Lanes = std::min( 6, log2W + log2H - log2V ), perWave = 64 >> log2Lanes;
    for( int k = c0; k < c1; k++ ) sorted[k] = dev[order[k].idx];
    for( int k = c0; k < c1; k += perWave )
    {
      IctUnit u; memset( &u, 0, sizeof( u ) );
      u.first = k; u.n = ( int16_t ) std::min( perWave, c1 - k ); u.log2W = ( uint8_t ) log2W; u.log2H = ( uint8_t ) log2H; u.log2V = ( uint8_t ) log2V; u.log2Lanes = ( uint8_t ) log2Lanes;
      units.push_back( u );
    }
    c0 = c1;
  }
  IctUnit none; memset( &none, 0, sizeof( none ) );
  while( units.size() & 3 ) units.push_back( none );      // four waves per workgroup

  IctHead H;
  ListBlob blob( &H, sizeof( H ) );
  H.offItems = blob.add( sorted.data(), sorted.size() * sizeof( IctDev ) );
  H.offUnits = blob.add( units.data(), units.size() * sizeof( IctUnit ) );
  H.units = ( int ) units.size();
  return listUpload( ctx, ictSlot( ctx, dir ), blob, &key );
}

// the list's key: the direction's pointer alignment + the items; -> the schedule is current and ordered in front of the launch on the context's stream
int ictSchedule( vvhip_ctx* ctx, const char* entry, int dir, const vvhip_ict_item* items_host, int n, int ptrAlign )
{
  std::vector<unsigned char> key( 1 + ( size_t ) n * sizeof( vvhip_ict_item ) );
  key[0] = ( unsigned char ) ptrAlign;
  memcpy( key.data() + 1, items_host, ( size_t ) n * sizeof( vvhip_ict_item ) );
  bool current = false;
  const int rc = listCurrent( ctx, ictSlot( ctx, dir ), key, &current );
  return rc || current ? rc : ictBuildSchedule( ctx, entry, dir, items_host, n, ptrAlign, key );
}

inline int ictPtrAlign( std::initializer_list<const void*> ptrs )
{
  int a = 8;
  for( const void* p : ptrs ) if( p ) a = std::min( a, ictAlignOf( ( uint64_t ) ( uintptr_t ) p >> 1 ) );
  return a;
}

} // namespace

extern "C" {

int vvhip_ict_fwd_batch( vvhip_ctx* ctx, const int16_t* d_resi, const vvhip_ict_item* items_host, int n, int16_t* d_joint, int64_t* d_dist )
{
  static const char* const entry = "vvhip_ict_fwd_batch";
  if( !ctx ) return VVHIP_E_ARG;
  if( n < 0 || n > ( 1 << 24 ) || ( n && ( !items_host || !d_resi ) ) || ( ( uintptr_t ) d_resi & 1 ) || ( ( uintptr_t ) d_joint & 1 ) )
    return vvhip_fail( ctx, VVHIP_E_ARG, "%s: %d items at %p, residual %p, joint blocks %p (int16 arrays)", entry, n, ( const void* ) items_host, ( const void* ) d_resi, ( void* ) d_joint );
  if( n == 0 ) return VVHIP_OK;
  if( !d_joint )
    for( int i = 0; i < n; i++ )
      if( items_host[i].mode != 0 ) return vvhip_fail( ctx, VVHIP_E_ARG, "%s: item %d has ICT mode %d and there is no buffer for the joint blocks", entry, i, items_host[i].mode );
  const int rc = ictSchedule( ctx, entry, 0, items_host, n, ictPtrAlign( { d_resi, d_joint } ) );
  if( rc ) return rc;
  HostList& S = ictSlot( ctx, 0 );
  const IctHead& H = listHead<IctHead>( S );
  const char* base = static_cast<const char*>( S.d );
  hipLaunchKernelGGL( ictFwdKernel, dim3( ( unsigned ) ( H.units / 4 ) ), dim3( 256 ), 0, ctx->stream, reinterpret_cast<const IctDev*>( base + H.offItems ),
                      reinterpret_cast<const IctUnit*>( base + H.offUnits ), d_resi, d_joint, d_dist );
  VVHIP_LAUNCH_CHECK( ctx );
  return listLaunched( ctx, S );
}

int vvhip_ict_inv_batch( vvhip_ctx* ctx, const int16_t* d_joint_rec, const vvhip_ict_item* items_host, int n, const vvhip_tu_stats* d_stats, int16_t* d_rec,
                         const int16_t* d_org_resi, uint64_t* d_sse )
{
  static const char* const entry = "vvhip_ict_inv_batch";
  if( !ctx ) return VVHIP_E_ARG;
  if( n < 0 || n > ( 1 << 24 ) || ( n && ( !items_host || !d_joint_rec ) ) || ( d_sse && !d_org_resi ) || ( ( uintptr_t ) d_joint_rec & 1 ) || ( ( uintptr_t ) d_rec & 1 ) ||
      ( ( uintptr_t ) d_org_resi & 1 ) )
    return vvhip_fail( ctx, VVHIP_E_ARG, "%s: %d items at %p, joint reconstruction %p, reconstruction %p, original residual %p, SSEs %p (int16 arrays; SSEs need the original residual)", entry, n,
                       ( const void* ) items_host, ( const void* ) d_joint_rec, ( void* ) d_rec, ( const void* ) d_org_resi, ( void* ) d_sse );
  if( n == 0 ) return VVHIP_OK;
  if( !d_stats )
    for( int i = 0; i < n; i++ )
      if( items_host[i].stats_idx >= 0 ) return vvhip_fail( ctx, VVHIP_E_ARG, "%s: item %d names statistics entry %d and there are no statistics", entry, i, items_host[i].stats_idx );
  const int rc = ictSchedule( ctx, entry, 1, items_host, n, ictPtrAlign( { d_joint_rec, d_rec, d_sse ? d_org_resi : nullptr } ) );
  if( rc ) return rc;
  HostList& S = ictSlot( ctx, 1 );
  const IctHead& H = listHead<IctHead>( S );
  const char* base = static_cast<const char*>( S.d );
  hipLaunchKernelGGL( ictInvKernel, dim3( ( unsigned ) ( H.units / 4 ) ), dim3( 256 ), 0, ctx->stream, reinterpret_cast<const IctDev*>( base + H.offItems ),
                      reinterpret_cast<const IctUnit*>( base + H.offUnits ), d_joint_rec, d_stats, d_rec, d_sse ? d_org_resi : nullptr, d_sse );
  VVHIP_LAUNCH_CHECK( ctx );
  return listLaunched( ctx, S );
}

} // extern "C"
