// ciip_golden_gen.cpp — records what the reference encoder's own planar intra prediction and CIIP weighting compute, for tests/golden/ciip.npz (driver: tests/ciip_golden_gen.py).
//
// Not part of build() and of no Makefile: compiled and linked by hand against the reference library where its sources and oracle/_ref/libvvenc_core.a
// (made by `make -C oracle/ref core`) exist.  With R = the reference checkout and O = oracle/_ref:
//
//   g++ -std=c++14 -O2 -pthread -w -fno-access-control -DTARGET_SIMD_X86=1 -DVVENC_SOURCE -DNDEBUG -I$O/gen -I$R/include -I$R/source/Lib/vvenc -I$R/source/Lib
//       -I$R/source/Lib/CommonLib -I$R/source/Lib/CommonLib/x86 -isystem $R/thirdparty tests/ciip_golden_gen.cpp
//       -Wl,--whole-archive $O/libvvenc_core.a -Wl,--no-whole-archive -o <somewhere outside the repository>/ciip_golden_gen
//
// (-fno-access-control: xFilterReferenceSamples and the two reference-length members are private.)
// Per case the block's reference line goes into the two rows of a reference buffer as xFillReferenceSamples leaves them — row 0 the top row, row 1 the left row, each
// 2 w + 1 / 2 h + 1 samples long; the samples behind top[w + 2] / left[h + 2], which the case does not have, are filled with a pattern of their own — and then through
//   IntraPrediction::xFilterReferenceSamples     (luma cases only; m_topRefLength = 2 w, m_leftRefLength = 2 h as setReferenceArrayLengths leaves them)
//   IntraPrediction::xPredIntraPlanar            the object's function pointer
//   IntraPrediction::IntraPredSampleFilter       the object's function pointer, where min( w, h ) >= 4 (applyPDPC)
//   g_pelBufOP.weightCiip( inter, intra, w * h, numIntra )
// once with IntraPrediction( false ) and the scalar PelBufferOps, once with IntraPrediction( true ) and the x86 PelBufferOps.
//
// input  (argv[1]) : int32 n, then per case int32 bitDepth, w, h, chroma, numIntra, the line (w + h + 6 int16: top[0 .. w + 2], left[0 .. h + 2]) and the h x w inter block
// output (argv[2]) : per case and row (scalar, x86) the h x w intra block, then the h x w result, int16
#include <cstdio>
#include <cstdint>
#include <cstring>
#include <vector>
#include "CommonLib/CommonDef.h"
#include "CommonLib/Unit.h"
#include "CommonLib/Buffer.h"
#include "CommonLib/Slice.h"
#include "CommonLib/IntraPrediction.h"

using namespace vvenc;

int main( int argc, char** argv )
{
  if( argc != 3 ) { fprintf( stderr, "usage: %s in out\n", argv[0] ); return 2; }
  FILE* fi = fopen( argv[1], "rb" ); FILE* fo = fopen( argv[2], "wb" );
  if( !fi || !fo ) return 2;
  IntraPrediction* ip[2] = { new IntraPrediction( false ), new IntraPrediction( true ) };
  const PelBufferOps scalarOps;                      // the constructor installs the scalar entries
  g_pelBufOP = scalarOps;
  g_pelBufOP.initPelBufOps( true );
  const PelBufferOps simdOps = g_pelBufOP;
  if( ip[1]->xPredIntraPlanar == ip[0]->xPredIntraPlanar || ip[1]->IntraPredSampleFilter == ip[0]->IntraPredSampleFilter || simdOps.weightCiip == scalarOps.weightCiip )
  { fprintf( stderr, "no x86 row on this machine\n" ); return 3; }
  SPS sps;
  int32_t n = 0;
  if( fread( &n, 4, 1, fi ) != 1 ) return 2;
  for( int i = 0; i < n; i++ )
  {
    int32_t hd[5];
    if( fread( hd, 4, 5, fi ) != 5 ) return 2;
    const int bd = hd[0], w = hd[1], h = hd[2], chroma = hd[3], numIntra = hd[4];
    std::vector<int16_t> line( w + h + 6 ), inter( ( size_t ) w * h );
    if( fread( line.data(), 2, line.size(), fi ) != line.size() || fread( inter.data(), 2, inter.size(), fi ) != inter.size() ) return 2;
    const int stride = 2 * ( w > h ? w : h ) + 1, maxv = ( 1 << bd ) - 1;
    std::vector<Pel> unf( 2 * stride + 64, 0 ), flt( 2 * stride + 64, 0 );
    for( int k = 0; k <= 2 * w; k++ ) unf[k]          = k <= w + 2 ? line[k]         : ( Pel ) ( ( 37 * k + 11 * i ) & maxv );
    for( int k = 0; k <= 2 * h; k++ ) unf[stride + k] = k <= h + 2 ? line[w + 3 + k] : ( Pel ) ( ( 53 * k + 7 * i ) & maxv );
    const CompArea area( chroma ? COMP_Cb : COMP_Y, CHROMA_420, Area( 0, 0, w, h ) );
    for( int row = 0; row < 2; row++ )
    {
      const Pel* src = unf.data();
      if( !chroma )
      {
        ip[row]->m_topRefLength = 2 * w; ip[row]->m_leftRefLength = 2 * h;
        ip[row]->xFilterReferenceSamples( unf.data(), flt.data(), area, sps, 0, stride );
        src = flt.data();
      }
      const CPelBuf srcBuf( src, stride, 2 );
      std::vector<Pel> store( 2 * ( ( size_t ) w * h + 64 ) + 32, -1 );      // slack: the x86 rows read and write whole vectors, some of them aligned ones
      Pel* intra = reinterpret_cast<Pel*>( ( reinterpret_cast<uintptr_t>( store.data() ) + 63 ) & ~( uintptr_t ) 63 );
      Pel* res = intra + ( ( size_t ) w * h + 64 );
      PelBuf dst( intra, w, w, h );
      ip[row]->xPredIntraPlanar( dst, srcBuf );
      if( w >= 4 && h >= 4 ) ip[row]->IntraPredSampleFilter( dst, srcBuf );
      memcpy( res, inter.data(), 2 * inter.size() );
      g_pelBufOP = row ? simdOps : scalarOps;
      g_pelBufOP.weightCiip( res, intra, w * h, numIntra );
      fwrite( intra, 2, ( size_t ) w * h, fo );
      fwrite( res, 2, ( size_t ) w * h, fo );
    }
  }
  fclose( fi ); fclose( fo );
  return 0;
}
