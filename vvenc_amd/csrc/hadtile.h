// hadtile.h — the Hadamard tile helpers shared by the kernels that score blocks with the reference's HAD family (me.hip: stages and table calls; intra.hip: the mode list).
// Device code only; include behind common.h.  Everything sits in the including unit's anonymous namespace.
#pragma once
#include "common.h"

namespace {

typedef short s16x2 __attribute__( ( ext_vector_type( 2 ) ) );
__device__ __forceinline__ int lo16( uint32_t v ) { return ( int ) ( int16_t ) ( v & 0xffffu ); }
__device__ __forceinline__ int hi16( uint32_t v ) { return ( int ) ( ( int32_t ) v >> 16 ); }
__device__ __forceinline__ uint32_t pkAdd( uint32_t a, uint32_t b ) { return __builtin_bit_cast( uint32_t, __builtin_bit_cast( s16x2, a ) + __builtin_bit_cast( s16x2, b ) ); }
__device__ __forceinline__ uint32_t pkSub( uint32_t a, uint32_t b ) { return __builtin_bit_cast( uint32_t, __builtin_bit_cast( s16x2, a ) - __builtin_bit_cast( s16x2, b ) ); }
constexpr uint32_t BIAS = 0x80008000u;      // signed int16 pair -> unsigned order (v_sad_u16 on biased operands is |a - b| of the signed values)
// 4x4 Hadamard of 16 differences (xCalcHADs4x4, RdCost.cpp:1028-1124): sum of |coefficients| with the DC a quarter, then ( satd + 1 ) >> 1
__device__ __forceinline__ uint32_t hadamard4x4( int ( &d )[16] )
{
#pragma unroll
  for( int r = 0; r < 4; r++ )
  {
    const int a = d[4 * r], b = d[4 * r + 1], c = d[4 * r + 2], e = d[4 * r + 3];
    const int s0 = a + b, s1 = a - b, s2 = c + e, s3 = c - e;
    d[4 * r] = s0 + s2; d[4 * r + 1] = s1 + s3; d[4 * r + 2] = s0 - s2; d[4 * r + 3] = s1 - s3;
  }
  uint32_t s = 0;
#pragma unroll
  for( int c = 0; c < 4; c++ )
  {
    const int a = d[c], b = d[4 + c], e = d[8 + c], f = d[12 + c];
    const int s0 = a + b, s1 = a - b, s2 = e + f, s3 = e - f;
    const int v0 = s0 + s2, v1 = s1 + s3, v2 = s0 - s2, v3 = s1 - s3;
    s += ( c == 0 ? ( ( uint32_t ) abs( v0 ) >> 2 ) : ( uint32_t ) abs( v0 ) ) + ( uint32_t ) abs( v1 ) + ( uint32_t ) abs( v2 ) + ( uint32_t ) abs( v3 );
  }
  return ( s + 1 ) >> 1;
}

typedef short s16x2h __attribute__( ( ext_vector_type( 2 ) ) );
__device__ __forceinline__ int dot2( uint32_t a, uint32_t b, int c ) { return __builtin_amdgcn_sdot2( __builtin_bit_cast( s16x2h, a ), __builtin_bit_cast( s16x2h, b ), c, false ); }
// ---- Hadamard tiles --------------------------------------------------------------------------------------------------------------------------
// The reference's tile ladder (xGetHADs, RdCost.cpp:1818-1938: first match wins).  Every tile type is scored by a TEAM of LT lanes that hold 8 differences each
// (the tile's 8 x LT = 16, 32, 64 or 128 values): an 8-point Walsh-Hadamard transform in the lane's registers, then log2( LT ) butterfly stages across the lanes with DPP —
//   8x8   lane r = row r                                   16x16_fast  lane r = rows 2r, 2r + 1, 2x2 averages of 16 columns (RdCost.cpp:1126-1223)
//   16x8  lane r = row r & 7, columns 8 ( r >> 3 ) ..      8x16        lane r = row r                      (128 values: 16 lanes)
//   8x4   lane r = row r                                   4x8         lane r = rows 2r, 2r + 1 of 4 columns (the register transform then covers x0, x1, y0)
//   4x4   lane r = rows 2r, 2r + 1
// The pairings (in registers: the three index bits a lane holds; across lanes: i <-> 15 - i, i <-> 7 - i, i ^ 2, i ^ 1) are linearly independent over GF(2), so each is a
// valid Hadamard factorisation: the multiset of |coefficients| is the reference's, and the DC coefficient — the only one treated specially (|DC| >> 2 in every tile type) —
// ends in register 0 of lane 0.  Normalisation per tile type as the reference: RdCost.cpp:1119-1121 (4x4), :1317-1319 (8x8), :1218-1222 (16x16_fast),
// :1467 / :1606 (16x8 / 8x16: ( int ) ( sad / sqrt( 16.0 * 8 ) * 2 ) in IEEE double), :1682 / :1763 (8x4 / 4x8: sqrt( 4.0 * 8 )).
enum { TK_8x8 = 0, TK_16F = 1, TK_16x8 = 2, TK_8x16 = 3, TK_8x4 = 4, TK_4x8 = 5, TK_4x4 = 6, TK_2x2 = 7, TK_ROWS = 8 /* no transform: rows of 8 samples (SAD-scored stages) */ };
__host__ __device__ __forceinline__ int hadTileKind( int w, int h, bool fast )
{
  if( w > h && !( h & 7 ) && !( w & 15 ) ) return TK_16x8;
  if( w < h && !( w & 7 ) && !( h & 15 ) ) return TK_8x16;
  if( w > h && !( h & 3 ) && !( w & 7 ) )  return TK_8x4;
  if( w < h && !( w & 3 ) && !( h & 7 ) )  return TK_4x8;
  if( fast && w == h && !( w & 31 ) )      return TK_16F;
  if( !( w & 7 ) && !( h & 7 ) )           return TK_8x8;
  if( !( w & 3 ) && !( h & 3 ) )           return TK_4x4;
  return TK_2x2;
}
__host__ __device__ __forceinline__ int tileW( int kind ) { return ( kind == TK_16F || kind == TK_16x8 ) ? 16 : ( ( kind == TK_4x8 || kind == TK_4x4 ) ? 4 : ( kind == TK_2x2 ? 2 : 8 ) ); }
__host__ __device__ __forceinline__ int tileH( int kind ) { return ( kind == TK_16F || kind == TK_8x16 ) ? 16 : ( ( kind == TK_8x4 || kind == TK_4x4 ) ? 4 : ( kind == TK_2x2 ? 2 : 8 ) ); }
__host__ __device__ __forceinline__ int tileLanes( int kind ) { return ( kind == TK_16x8 || kind == TK_8x16 ) ? 16 : ( ( kind == TK_8x4 || kind == TK_4x8 ) ? 4 : ( kind == TK_4x4 ? 2 : ( kind == TK_2x2 ? 1 : 8 ) ) ); }

__device__ __forceinline__ uint32_t hadNorm( uint32_t s, int kind )
{
  if( kind == TK_8x8 || kind == TK_16F ) { const uint32_t v = ( s + 2 ) >> 2; return kind == TK_16F ? v << 2 : v; }
  if( kind == TK_4x4 ) return ( s + 1 ) >> 1;
  if( kind == TK_16x8 || kind == TK_8x16 ) return ( uint32_t ) ( int ) ( ( double ) ( int ) s / __builtin_sqrt( 16.0 * 8 ) * 2 );
  if( kind == TK_8x4 || kind == TK_4x8 )   return ( uint32_t ) ( int ) ( ( double ) ( int ) s / __builtin_sqrt( 4.0 * 8 ) * 2 );
  return s;
}

// the team's transform: d = the lane's 8 differences, r = the lane's index inside its team of LT lanes (teams are aligned groups of consecutive lanes).
// Returns the tile's normalised SATD in every lane of the team.  |d| < 2^23 / 128 on entry (differences of <= 12-bit values).
// hadTeamCross: the stages across the lanes + sum, on values the lane has already transformed in its registers
__device__ __forceinline__ uint32_t sadU32( uint32_t a, uint32_t b, uint32_t acc ) { uint32_t r; asm( "v_sad_u32 %0, %1, %2, %3" : "=v"( r ) : "v"( a ), "v"( b ), "v"( acc ) ); return r; }
// `done`: the lane-pair distances ( 8 / 4 / 2 ) whose stage the caller has already run (on packed pairs, hadTeamPkD)
__device__ __forceinline__ uint32_t hadTeamCross( int ( &d )[8], int r, int LT, int kind, int lane, int done = 0 )
{
  // upper lane of a pair: other - own, lower: own + other; |d| < 2^23.  The LAST stage (lane pairs i ^ 1: every team has it) adds 2^31 with its multiply (v_mad_i32_i24):
  // |coefficient| = |biased - 2^31| as unsigned numbers, so the sum of magnitudes is one v_sad_u32 per coefficient instead of subtract + max + add
  constexpr uint32_t B31 = 0x80000000u;
#define ME_VSTAGE( CTRL, BIT ) { const int sgn = ( r & ( BIT ) ) ? -1 : 1; _Pragma( "unroll" ) \
  for( int i = 0; i < 8; i++ ) { const int t = __mul24( d[i], sgn ); d[i] = VVHIP_DPP( d[i], CTRL ) + t; } }
  if( LT >= 16 && !( done & 8 ) ) ME_VSTAGE( VVHIP_DPP_MIRROR, 8 )
  if( LT >= 8 && !( done & 4 ) )  ME_VSTAGE( VVHIP_DPP_HALF_MIRROR, 4 )
  if( LT >= 4 && !( done & 2 ) )  ME_VSTAGE( VVHIP_DPP_XOR2, 2 )
#undef ME_VSTAGE
  {                                                                                   // (LT >= 2 for every tile type that comes here)
    const int sgn = ( r & 1 ) ? -1 : 1;
#pragma unroll
    for( int i = 0; i < 8; i++ )
    {
      int t; asm( "v_mad_i32_i24 %0, %1, %2, %3" : "=v"( t ) : "v"( d[i] ), "v"( sgn ), "s"( B31 ) );      // (written out: the compiler turns a multiply by +-1 plus a constant into four instructions)
      d[i] = ( int ) ( ( uint32_t ) VVHIP_DPP( d[i], VVHIP_DPP_XOR1 ) + ( uint32_t ) t );
    }
  }
  uint32_t s = 0;
#pragma unroll
  for( int i = 0; i < 8; i++ ) s = sadU32( ( uint32_t ) d[i], B31, s );
  if( r == 0 ) { const uint32_t dc = sadU32( ( uint32_t ) d[0], B31, 0u ); s = s - dc + ( dc >> 2 ); }
  s = vvhipGroupSum32( s, LT, lane );
  return hadNorm( s, kind );
}
__device__ __forceinline__ uint32_t hadTeam( int ( &d )[8], int r, int LT, int kind, int lane )
{
#pragma unroll
  for( int len = 1; len < 8; len <<= 1 )
#pragma unroll
    for( int i = 0; i < 8; i += 2 * len )
#pragma unroll
      for( int q = i; q < i + len; q++ ) { const int x = d[q], z = d[q + len]; d[q] = x + z; d[q + len] = x - z; }
  return hadTeamCross( d, r, LT, kind, lane );
}
// the same from the lane's two operand rows as PACKED sample pairs (o - p per 16-bit half): the two register stages that pair whole dwords run on packed pairs
// (v_pk_add_i16 / v_pk_sub_i16: sums of four differences, |d| <= 2^( bitDepth + 1 ) with bitDepth <= 10 -> 14 bits), the stage inside a dword is the unpacking itself
// (lo + hi, lo - hi as dot products with ( 1, 1 ) / ( 1, -1 )): 20 instructions for difference + register transform instead of 32.  The stages of a Hadamard transform commute;
// the all-plus coefficient (DC) still ends in register 0.
// Round 6: the first TWO stages across the lanes run on the packed pairs too — v_mov_b32_dpp + v_pk_mad_i16 ( own * ( +-1, +-1 ) + other ) per dword, 8 instructions per
// stage instead of 16 ( v_mul_i32_i24 + v_add_u32_dpp per value ).  Range: a difference is |o - p| <= 2 ( 2^bitDepth - 1 ) ( o a bi-prediction pattern 2 org - pred, p a
// sample; bitDepth <= 10 is checked at plan creation ) = 2046; two register stages + two lane stages sum 16 of them: 32736 <= 32767 — 16 bits hold every intermediate
// ( tests/test_gpu_corners.py drives exactly these extremes ).
__device__ __forceinline__ uint32_t pkMad( uint32_t a, uint32_t b, uint32_t c ) { uint32_t r; asm( "v_pk_mad_i16 %0, %1, %2, %3" : "=v"( r ) : "v"( a ), "v"( b ), "v"( c ) ); return r; }
__device__ __forceinline__ uint32_t hadTeamPkD( const uint32_t ( &D )[4], int r, int LT, int kind, int lane )
{
  const uint32_t E0 = pkAdd( D[0], D[1] ), E1 = pkSub( D[0], D[1] ), E2 = pkAdd( D[2], D[3] ), E3 = pkSub( D[2], D[3] );
  uint32_t F[4] = { pkAdd( E0, E2 ), pkAdd( E1, E3 ), pkSub( E0, E2 ), pkSub( E1, E3 ) };
#define ME_VSTAGE_PK( CTRL, BIT ) { const uint32_t sg = ( r & ( BIT ) ) ? 0xffffffffu : 0x00010001u; _Pragma( "unroll" ) \
  for( int q = 0; q < 4; q++ ) F[q] = pkMad( F[q], sg, ( uint32_t ) VVHIP_DPP( F[q], CTRL ) ); }
  int done = 0;
  if( LT >= 16 )     { ME_VSTAGE_PK( VVHIP_DPP_MIRROR, 8 ) ME_VSTAGE_PK( VVHIP_DPP_HALF_MIRROR, 4 ) done = 8 | 4; }
  else if( LT >= 8 ) { ME_VSTAGE_PK( VVHIP_DPP_HALF_MIRROR, 4 ) ME_VSTAGE_PK( VVHIP_DPP_XOR2, 2 ) done = 4 | 2; }
  else if( LT >= 4 ) { ME_VSTAGE_PK( VVHIP_DPP_XOR2, 2 ) done = 2; }
#undef ME_VSTAGE_PK
  int d[8];
#pragma unroll
  for( int q = 0; q < 4; q++ ) { d[2 * q] = dot2( F[q], 0x00010001u, 0 ); d[2 * q + 1] = dot2( F[q], 0xffff0001u, 0 ); }
  return hadTeamCross( d, r, LT, kind, lane, done );
}
__device__ __forceinline__ uint32_t hadTeamPk( const uint32_t ( &o )[4], const uint32_t ( &p )[4], int r, int LT, int kind, int lane )
{
  const uint32_t D[4] = { pkSub( o[0], p[0] ), pkSub( o[1], p[1] ), pkSub( o[2], p[2] ), pkSub( o[3], p[3] ) };
  return hadTeamPkD( D, r, LT, kind, lane );
}
// two ints ( each inside 16 bits ) as a packed pair
__device__ __forceinline__ uint32_t pkInts( int lo, int hi ) { return __builtin_amdgcn_perm( ( uint32_t ) hi, ( uint32_t ) lo, 0x05040100u ); }

} // namespace
