// blend_golden_gen.cpp — records what the reference encoder's own BCW and GEO blending computes, for tests/golden/blend.npz (driver: tests/blend_golden_gen.py).
//
// Not part of build() and of no Makefile: compiled and linked by hand against the reference library where its sources and oracle/_ref/libvvenc_core.a
// (made by `make -C oracle/ref core`) exist.  With R = the reference checkout and O = oracle/_ref:
//
//   g++ -std=c++14 -O2 -pthread -w -DTARGET_SIMD_X86=1 -DVVENC_SOURCE -DNDEBUG -I$O/gen -I$R/include -I$R/source/Lib/vvenc -I$R/source/Lib
//       -I$R/source/Lib/CommonLib -I$R/source/Lib/CommonLib/x86 -isystem $R/thirdparty tests/blend_golden_gen.cpp
//       -Wl,--whole-archive $O/libvvenc_core.a -Wl,--no-whole-archive -o <somewhere outside the repository>/blend_golden_gen
//
// Per case the two 14-bit blocks go through
//   kind 1 (BCW): AreaBuf<Pel>::addWeightedAvg( s0, s1, clpRng, bcwIdx )                                  — g_pelBufOP's scalar entries, then its x86 entries
//   kind 2 (GEO): InterpolationFilter::weightedGeoBlk( clpRngs, cu, w, h, comp, splitDir, dst, s0, s1 )  — after initInterpolationFilter( false ), then ( true )
// with a CodingUnit of the case's luma size ( w << chroma ) x ( h << chroma ) in 4:2:0 and comp = Y or Cb.  The GEO tables are the library's own (InitGeoRom).
//
// input  (argv[1]) : int32 n, then per case int32 kind, bitDepth, w, h, chroma, param and the two h x w blocks as int16
// output (argv[2]) : per case the h x w result of the scalar row, then of the x86 row, int16
#include <cstdio>
#include <cstdint>
#include <cstring>
#include <vector>
#include "CommonLib/CommonDef.h"
#include "CommonLib/Unit.h"
#include "CommonLib/Buffer.h"
#include "CommonLib/InterpolationFilter.h"

using namespace vvenc;

int main( int argc, char** argv )
{
  if( argc != 3 ) { fprintf( stderr, "usage: %s in out\n", argv[0] ); return 2; }
  FILE* fi = fopen( argv[1], "rb" ); FILE* fo = fopen( argv[2], "wb" );
  if( !fi || !fo ) return 2;
  InterpolationFilter filt[2];
  filt[0].initInterpolationFilter( false );
  filt[1].initInterpolationFilter( true );
  const PelBufferOps scalarOps;                      // the constructor installs the scalar entries
  g_pelBufOP = scalarOps;
  g_pelBufOP.initPelBufOps( true );
  const PelBufferOps simdOps = g_pelBufOP;
  if( filt[1].m_weightedGeoBlk == filt[0].m_weightedGeoBlk || simdOps.wghtAvg8 == scalarOps.wghtAvg8 ) { fprintf( stderr, "no x86 row on this machine\n" ); return 3; }
  int32_t n = 0;
  if( fread( &n, 4, 1, fi ) != 1 ) return 2;
  for( int i = 0; i < n; i++ )
  {
    int32_t hd[6];
    if( fread( hd, 4, 6, fi ) != 6 ) return 2;
    const int kind = hd[0], bd = hd[1], w = hd[2], h = hd[3], chroma = hd[4], param = hd[5];
    std::vector<int16_t> s[2];
    for( int k = 0; k < 2; k++ )
    {
      s[k].assign( ( size_t ) w * h + 64, 0 );      // slack: the x86 rows read whole vectors
      if( fread( s[k].data(), 2, ( size_t ) w * h, fi ) != ( size_t ) w * h ) return 2;
    }
    ClpRngs clp; clp.bd = bd;
    for( int row = 0; row < 2; row++ )
    {
      std::vector<int16_t> out( ( size_t ) w * h + 64, -1 );
      if( kind == 1 )
      {
        g_pelBufOP = row ? simdOps : scalarOps;
        PelBuf dst( out.data(), w, w, h );
        dst.addWeightedAvg( CPelBuf( s[0].data(), w, w, h ), CPelBuf( s[1].data(), w, w, h ), clp, ( int8_t ) param );
      }
      else
      {
        const ComponentID comp = chroma ? COMP_Cb : COMP_Y;
        const Area luma( 0, 0, w << chroma, h << chroma );
        CodingUnit cu( CHROMA_420, luma );
        PelStorage st[3];
        for( int k = 0; k < 3; k++ ) { st[k].create( CHROMA_420, luma ); st[k].bufs[comp].fill( -1 ); }
        for( int k = 0; k < 2; k++ ) for( int y = 0; y < h; y++ ) memcpy( st[k].bufs[comp].buf + ( ptrdiff_t ) y * st[k].bufs[comp].stride, s[k].data() + ( size_t ) y * w, 2 * ( size_t ) w );
        PelUnitBuf d = st[2], a = st[0], b = st[1];
        filt[row].weightedGeoBlk( clp, cu, w, h, comp, ( uint8_t ) param, d, a, b );
        for( int y = 0; y < h; y++ ) memcpy( out.data() + ( size_t ) y * w, st[2].bufs[comp].buf + ( ptrdiff_t ) y * st[2].bufs[comp].stride, 2 * ( size_t ) w );
        for( int k = 0; k < 3; k++ ) st[k].destroy();
      }
      fwrite( out.data(), 2, ( size_t ) w * h, fo );
    }
  }
  fclose( fi ); fclose( fo );
  return 0;
}
