// ict_golden_gen.cpp — records what the reference encoder's own joint Cb-Cr transform computes, for tests/golden/ict.npz (driver: tests/ict_golden_gen.py).
//
// Not part of build() and of no Makefile: compiled and linked by hand against the reference library where its sources and oracle/_ref/libvvenc_core.a
// (made by `make -C oracle/ref core`) exist.  With R = the reference checkout and O = oracle/_ref:
//
//   g++ -std=c++14 -O2 -pthread -w -DTARGET_SIMD_X86=1 -DVVENC_SOURCE -DNDEBUG -I$O/gen -I$R/include -I$R/source/Lib/vvenc -I$R/source/Lib
//       -I$R/source/Lib/CommonLib -I$R/source/Lib/CommonLib/x86 -isystem $R/thirdparty tests/ict_golden_gen.cpp
//       -Wl,--whole-archive $O/libvvenc_core.a -Wl,--no-whole-archive -o <somewhere outside the repository>/ict_golden_gen
//
// Per case the two residual blocks go through
//   TrQuant::fwdTransformICT( tu, resCb, resCr, resC1, resC2, cbfMask )     -> the joint block (resC1 for |mode| = 1, 2; resC2 for |mode| = 3) and the pair ( d1, d2 )
//   TrQuant::invTransformICT( tu, resCb, resCr )                            twice: with the joint block as the coded component (the other one preset to a pattern of its
//                                                                            own, which must not survive), and with the case's own INPUT block as the coded component —
//                                                                            that pins the narrowing of the derived component at int16 inputs the forward step never produces
// on a faked TransformUnit whose cs->picHeader->jointCbCrSign and jointCbCr select the signed mode through TU::getICTMode (g_ictModes, Rom.cpp:1453), the way
// oracle/ref/ref_api.cpp fakes one for QuantCore.  These functions have ONE row: TrQuant's constructor installs fwdTransformCbCr<m> / invTransformCbCr<m>
// (TrQuant.cpp:230-247) and initTrQuantX86 replaces neither, so there is no x86 variant to record beside it.
//
// input  (argv[1]) : int32 n, then per case int32 mode, w, h and the h x w Cb block and the h x w Cr block, int16
// output (argv[2]) : per case int64 d1, d2; for mode != 0 then five h x w int16 blocks: joint, Cb and Cr from the joint block, Cb and Cr from the input block
#include <cstdio>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "CommonLib/CommonDef.h"
#include "CommonLib/Unit.h"
#include "CommonLib/Buffer.h"
#include "CommonLib/Slice.h"
#include "CommonLib/CodingStructure.h"
#include "CommonLib/Rom.h"
#include "CommonLib/TrQuant.h"

using namespace vvenc;

int main( int argc, char** argv )
{
  if( argc != 3 ) { fprintf( stderr, "usage: %s in out\n", argv[0] ); return 2; }
  FILE* fi = fopen( argv[1], "rb" ); FILE* fo = fopen( argv[2], "wb" );
  if( !fi || !fo ) return 2;
  TrQuant trq;
  PicHeader ph;
  void* csMem = calloc( 1, sizeof( CodingStructure ) );
  CodingStructure* cs = reinterpret_cast<CodingStructure*>( csMem );
  cs->picHeader = &ph;
  int32_t n = 0;
  if( fread( &n, 4, 1, fi ) != 1 ) return 2;
  for( int i = 0; i < n; i++ )
  {
    int32_t hd[3];
    if( fread( hd, 4, 3, fi ) != 3 ) return 2;
    const int mode = hd[0], w = hd[1], h = hd[2], am = mode < 0 ? -mode : mode;
    const size_t cnt = ( size_t ) w * h;
    std::vector<Pel> cb( cnt ), cr( cnt );
    if( fread( cb.data(), 2, cnt, fi ) != cnt || fread( cr.data(), 2, cnt, fi ) != cnt ) return 2;
    int mask = -1;
    for( int k = 0; k < 4; k++ ) if( g_ictModes[0][k] == am ) mask = k;
    if( mask < 0 || g_ictModes[mode < 0 ? 1 : 0][mask] != mode ) { fprintf( stderr, "case %d: no cbf mask for mode %d\n", i, mode ); return 3; }
    ph.jointCbCrSign = mode < 0;
    TransformUnit tu( CHROMA_420, Area( 0, 0, 2 * w, 2 * h ) );
    tu.cs = cs;
    tu.jointCbCr = ( uint8_t ) mask;
    std::vector<Pel> c1( cnt, 12345 ), c2( cnt, 12345 );
    const PelBuf bCb( cb.data(), w, w, h ), bCr( cr.data(), w, w, h );
    PelBuf bC1( c1.data(), w, w, h ), bC2( c2.data(), w, w, h );
    const std::pair<int64_t, int64_t> d = trq.fwdTransformICT( tu, bCb, bCr, bC1, bC2, mask );
    const int64_t dd[2] = { d.first, d.second };
    fwrite( dd, 8, 2, fo );
    if( mode == 0 ) continue;
    const std::vector<Pel>& joint = am == 3 ? c2 : c1;
    const std::vector<Pel>& idle  = am == 3 ? c1 : c2;
    for( size_t k = 0; k < cnt; k++ ) if( idle[k] != 12345 ) { fprintf( stderr, "case %d: mode %d wrote the other joint buffer\n", i, mode ); return 3; }
    fwrite( joint.data(), 2, cnt, fo );
    for( int pass = 0; pass < 2; pass++ )
    {
      std::vector<Pel> rCb( cnt, -21555 ), rCr( cnt, -21555 );
      ( am == 3 ? rCr : rCb ) = pass == 0 ? joint : ( am == 3 ? cr : cb );
      PelBuf bRCb( rCb.data(), w, w, h ), bRCr( rCr.data(), w, w, h );
      trq.invTransformICT( tu, bRCb, bRCr );
      fwrite( rCb.data(), 2, cnt, fo );
      fwrite( rCr.data(), 2, cnt, fo );
    }
  }
  fclose( fi ); fclose( fo );
  free( csMem );
  return 0;
}
