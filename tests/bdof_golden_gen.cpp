// bdof_golden_gen.cpp — records what the reference encoder's own BDOF code computes, for tests/golden/bdof.npz (driver: tests/bdof_golden_gen.py).
//
// Not part of build() and of no Makefile: compiled and linked by hand against the reference library where its sources and oracle/_ref/libvvenc_core.a
// (made by `make -C oracle/ref core`) exist.  With R = the reference checkout and O = oracle/_ref:
//
//   g++ -std=c++14 -O2 -pthread -w -DTARGET_SIMD_X86=1 -DVVENC_SOURCE -DNDEBUG -I$O/gen -I$R/include -I$R/source/Lib/vvenc -I$R/source/Lib
//       -I$R/source/Lib/CommonLib -I$R/source/Lib/CommonLib/x86 -isystem $R/thirdparty tests/bdof_golden_gen.cpp
//       -Wl,--whole-archive $O/libvvenc_core.a -Wl,--no-whole-archive -o <somewhere outside the repository>/bdof_golden_gen
//
// A subclass exposes the protected members of InterPredInterpolation.  Per case the two ( h + 2 ) x ( w + 2 ) frames — the 14-bit block of each list inside its
// one-sample ring, as xPredInterBlk leaves them — are copied into m_filteredBlockTmp[2] / [3] at the layout xApplyBDOF expects (row pitch w + 4, frame origin at
// pitch + 1), then xApplyBDOF runs: xFpBDOFGradFilter, the padding, xFpBiDirOptFlow.  Once after init( false ) (the scalar row) and once after init( true )
// (the x86 row).
//
// input  (argv[1]) : int32 n, then per case int32 bitDepth, w, h and the two frames as int16
// output (argv[2]) : per case the h x w result of the scalar row, then of the x86 row, int16
#include <cstdio>
#include <cstdint>
#include <cstring>
#include <vector>
#include "CommonLib/CommonDef.h"
#include "CommonLib/Unit.h"
#include "CommonLib/InterPrediction.h"

using namespace vvenc;

struct Probe : public InterPredInterpolation
{
  void run( const int16_t* f0, const int16_t* f1, int w, int h, int bd, int16_t* out )
  {
    const int pitch = w + 4;
    for( int l = 0; l < 2; l++ )
    {
      Pel* t = m_filteredBlockTmp[2 + l][COMP_Y];
      memset( t, 0x55, sizeof( Pel ) * pitch * ( h + 4 ) );
      const int16_t* f = l ? f1 : f0;
      for( int y = 0; y < h + 2; y++ ) memcpy( t + ( y + 1 ) * pitch + 1, f + y * ( w + 2 ), sizeof( Pel ) * ( w + 2 ) );
    }
    PelBuf dst( out, w, w, h );
    ClpRng clp; clp.bd = bd;
    xApplyBDOF( dst, clp );
  }
};

int main( int argc, char** argv )
{
  if( argc != 3 ) { fprintf( stderr, "usage: %s in out\n", argv[0] ); return 2; }
  FILE* fi = fopen( argv[1], "rb" ); FILE* fo = fopen( argv[2], "wb" );
  if( !fi || !fo ) return 2;
  Probe scalar, simd;
  scalar.init( false );
  simd.init( true );
  if( simd.xFpBiDirOptFlow == scalar.xFpBiDirOptFlow || simd.xFpBDOFGradFilter == scalar.xFpBDOFGradFilter ) { fprintf( stderr, "no x86 row on this machine\n" ); return 3; }
  int32_t n = 0;
  if( fread( &n, 4, 1, fi ) != 1 ) return 2;
  for( int i = 0; i < n; i++ )
  {
    int32_t hd[3];
    if( fread( hd, 4, 3, fi ) != 3 ) return 2;
    const int bd = hd[0], w = hd[1], h = hd[2], fe = ( w + 2 ) * ( h + 2 );
    std::vector<int16_t> f0( fe ), f1( fe ), o( w * h );
    if( fread( f0.data(), 2, fe, fi ) != ( size_t ) fe || fread( f1.data(), 2, fe, fi ) != ( size_t ) fe ) return 2;
    scalar.run( f0.data(), f1.data(), w, h, bd, o.data() ); fwrite( o.data(), 2, o.size(), fo );
    simd.run( f0.data(), f1.data(), w, h, bd, o.data() );   fwrite( o.data(), 2, o.size(), fo );
  }
  fclose( fi ); fclose( fo );
  return 0;
}
