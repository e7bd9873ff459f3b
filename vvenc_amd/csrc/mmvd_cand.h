// mmvd_cand.h — one MMVD merge candidate of a vvhip_mmvd_item, host and device: the vectors, used lists and BCW index the reference arrives at before it predicts.
// mmvd.hip's kernel, its validation path and vvhip_mmvd_candidate all go through mmvdDerive, so what the host hands to the prediction list is what the kernel scored.
//   MergeCtx::getMmvdDeltaMv           CommonLib/ContextModelling.cpp:261-342
//   MergeCtx::setMmvdMergeCandiInfo    :344-404      (Mv::clipToStorageBitDepth Mv.h:274-278, CU::restrictBiPredMergeCandsOne UnitTools.cpp:3085-3097)
//   CU::getDistScaleFactor             CommonLib/UnitTools.cpp:1354-1371;  Mv::scaleMv  CommonLib/Mv.h:182-187
//   xCheckIdenticalMotion              CommonLib/InterPrediction.cpp:292-324;  clipMv  CommonLib/Mv.cpp:68-80 (at InterPrediction.cpp:382)
#pragma once
#include "../../include/vvenc_hip.h"

#ifndef __HIPCC__
#define __host__
#define __device__
#endif

struct MmvdCand
{
  int  mvx[2], mvy[2];           // after the picture clip
  int  stx[2], sty[2];           // cu.mv: after the storage clip, ( 0, 0 ) for a list the CU does not use
  bool used[2];                  // the lists the prediction reads
  int  bcw;
};

static inline __host__ __device__ int mmvdClip3( int lo, int hi, int v ) { return v < lo ? lo : ( v > hi ? hi : v ); }
static inline __host__ __device__ int mmvdAbs( int v ) { return v < 0 ? -v : v; }

// getDistScaleFactor with iDiffPocB = -pocB, iDiffPocD = -pocD (deltas are reference minus current); the callers below never pass equal or zero distances
static inline __host__ __device__ int mmvdDistScale( int pocB, int pocD )
{
  const int tdb = mmvdClip3( -128, 127, -pocB ), tdd = mmvdClip3( -128, 127, -pocD );
  const int x = ( 0x4000 + mmvdAbs( tdd / 2 ) ) / tdd;
  return mmvdClip3( -4096, 4095, ( tdb * x + 32 ) >> 6 );
}
static inline __host__ __device__ int mmvdScale( int scale, int v )
{
  const int p = scale * v;
  return mmvdClip3( -( 1 << 17 ), ( 1 << 17 ) - 1, ( p + 128 - ( p >= 0 ) ) >> 8 );
}

// the item's candidate val (0..63); the base must use a list.  zeroDelta: the base vector itself through the same clips (the kernel centres its window on it)
static inline __host__ __device__ void mmvdDerive( const vvhip_mmvd_item& q, int val, int picW, int picH, int ctu, int disFrac, MmvdCand& c, bool zeroDelta = false )
{
  const int b = ( val >> 5 ) & 1, step = ( val >> 2 ) & 7, pos = val & 3;
  int offset = 1 << ( step + 2 );
  if( disFrac ) offset <<= 2;
  if( zeroDelta ) offset = 0;
  const int dx = pos == 0 ? offset : ( pos == 1 ? -offset : 0 ), dy = pos == 2 ? offset : ( pos == 3 ? -offset : 0 );
  const bool r0 = q.ref_plane[b][0] >= 0, r1 = q.ref_plane[b][1] >= 0;
  int d0x = 0, d0y = 0, d1x = 0, d1y = 0;
  if( r0 && r1 )
  {
    const int p0 = q.poc_delta[b][0], p1 = q.poc_delta[b][1];
    const bool lt = q.long_term[b] != 0, same = ( long long ) p1 * p0 > 0;
    d0x = dx; d0y = dy;
    if( p0 == p1 ) { d1x = dx; d1y = dy; }
    else if( mmvdAbs( p1 ) > mmvdAbs( p0 ) )
    {
      d1x = dx; d1y = dy;
      if( lt ) { d0x = same ? dx : -dx; d0y = same ? dy : -dy; }
      else { const int s = mmvdDistScale( p0, p1 ); d0x = mmvdScale( s, dx ); d0y = mmvdScale( s, dy ); }
    }
    else
    {
      if( lt ) { d1x = same ? dx : -dx; d1y = same ? dy : -dy; }
      else { const int s = mmvdDistScale( p1, p0 ); d1x = mmvdScale( s, dx ); d1y = mmvdScale( s, dy ); }
    }
  }
  else if( r0 ) { d0x = dx; d0y = dy; }
  else          { d1x = dx; d1y = dy; }
  const int lo = -( 1 << 17 ), hi = ( 1 << 17 ) - 1;
  c.used[0] = r0; c.used[1] = r1;
  c.stx[0] = r0 ? mmvdClip3( lo, hi, q.mv[b][0][0] + d0x ) : 0; c.sty[0] = r0 ? mmvdClip3( lo, hi, q.mv[b][0][1] + d0y ) : 0;
  c.stx[1] = r1 ? mmvdClip3( lo, hi, q.mv[b][1][0] + d1x ) : 0; c.sty[1] = r1 ? mmvdClip3( lo, hi, q.mv[b][1][1] + d1y ) : 0;
  c.bcw = ( r0 && r1 ) ? q.bcw_idx[b] : 2;
  if( r0 && r1 && q.w + q.h == 12 ) { c.used[1] = false; c.stx[1] = c.sty[1] = 0; c.bcw = 2; }                     // restrictBiPredMergeCandsOne
  if( c.used[0] && c.used[1] && q.poc_delta[b][0] == q.poc_delta[b][1] && c.stx[0] == c.stx[1] && c.sty[0] == c.sty[1] )      // xCheckIdenticalMotion: list 0 alone
  { c.used[1] = false; c.bcw = 2; }
  const int horMax = ( picW + 8 - q.cu_x - 1 ) * 16, horMin = ( -ctu - 8 - q.cu_x + 1 ) * 16;
  const int verMax = ( picH + 8 - q.cu_y - 1 ) * 16, verMin = ( -ctu - 8 - q.cu_y + 1 ) * 16;
  c.mvx[0] = mmvdClip3( horMin, horMax, c.stx[0] ) ; c.mvy[0] = mmvdClip3( verMin, verMax, c.sty[0] );
  c.mvx[1] = mmvdClip3( horMin, horMax, c.stx[1] ) ; c.mvy[1] = mmvdClip3( verMin, verMax, c.sty[1] );
}

static inline __host__ __device__ bool mmvdSizeOk( int w, int h )
{
  return w >= 4 && w <= 128 && h >= 4 && h <= 128 && !( w & ( w - 1 ) ) && !( h & ( h - 1 ) ) && w + h >= 12;
}
