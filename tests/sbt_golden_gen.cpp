// sbt_golden_gen.cpp — records what the reference encoder's own sub-block transform (SBT) code computes, for tests/golden/sbt.npz (driver: tests/sbt_golden_gen.py).
//
// Not part of build() and of no Makefile: compiled and linked by hand against the reference library where its sources and oracle/_ref/libvvenc_core.a
// (made by `make -C oracle/ref core`) exist.  With R = the reference checkout and O = oracle/_ref:
//
//   g++ -std=c++14 -O2 -pthread -w -DTARGET_SIMD_X86=1 -DVVENC_SOURCE -DNDEBUG -I$O/gen -I$R/include -I$R/source/Lib/vvenc -I$R/source/Lib
//       -I$R/source/Lib/CommonLib -I$R/source/Lib/CommonLib/x86 -isystem $R/thirdparty tests/sbt_golden_gen.cpp
//       -Wl,--whole-archive $O/libvvenc_core.a -Wl,--no-whole-archive -o <somewhere outside the repository>/sbt_golden_gen
//
// Three record kinds, read from argv[1] and answered in argv[2] in the same order:
//   1  a CU: int32 w, h, sbtAllowed, double chromaWeight, double distScale, then the Y ( h x w ), Cb and Cr ( h/2 x w/2 ) residual blocks, int16.
//      InterSearch::xCalcMinDistSbt ITSELF (EncoderLib/InterSearch.cpp:3272-3464; a private member, reached by compiling the class's header with `private` spelled
//      `public`) runs on a faked CodingStructure: it reads cs.pcv, cs.sps->bitDepths, the original and the prediction buffer (org = resi >> 1, pred = org - resi: any int16
//      residual is a difference of two Pels), cu.blocks and m_pcRdCost — an RdCost with both chroma distortion weights = chromaWeight.  "Fast algorithm 1" (:3353-3359) returns
//      before anything is estimated whenever distScale * total < 12 << SCALE_BITS; the estimates are recorded with an INFINITE distortion scale (lambda -> 0: the comparison is
//      false for every total, zero included), then the function runs again with distScale for m_skipSbtAll alone.
//      -> uint64 est[9] (getEstDistSbt), uint8 order[8] (m_sbtRdoOrder), uint8 skip (getSkipSbtAll), then uint64 parts[2][3][16]: the UNWEIGHTED sum of squares of every part
//      per component from the reference's SSE table entry (RdCost::getDistPart( org part, pred part, COMP_Y, DF_SSE )) — [0] the scalar row (RdCost::create( false )), [1]
//      the x86 row (create( true )).
//   2  a tiling: int32 w, h, mode -> for tile 0 and tile 1 and each component int32 x, y, width, height (PartitionerImpl::getSbtTuTiling on CU::getSbtTuSplit's split), then
//      int32 trHor, trVer of the CODED tile's luma TU (TrQuant::xSetTrTypes on a TU of that tile whose CU carries the sbtInfo, sps->MTS on).
//   3  a pair of blocks: int32 w, h, then two h x w int16 blocks -> uint64 sse[2]: the SSE table entry on the pair, scalar row and x86 row.
#include <cmath>
#include <cstdio>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>
#include <array>
#include <map>
#include <list>
#include <string>
#include <sstream>
#include <iostream>
#include <algorithm>
#include <functional>
#include <memory>
#include <mutex>
#include <atomic>
#include <thread>
#include <condition_variable>
#include <unordered_map>
#include <deque>
#include <set>
#include <chrono>
#include <bitset>
#include <fstream>
#include <iomanip>
#include <queue>
#include <stack>
#include <random>
#include <numeric>
#include <cassert>
#include <cstdarg>
#include <climits>
#include <cinttypes>
#include <exception>
#include <utility>
#include <type_traits>
#include <iterator>
#include <tuple>
#include <future>
#define private public
#define protected public
#include "CommonLib/CommonDef.h"
#include "CommonLib/Unit.h"
#include "CommonLib/Buffer.h"
#include "CommonLib/Slice.h"
#include "CommonLib/CodingStructure.h"
#include "CommonLib/Rom.h"
#include "CommonLib/RdCost.h"
#include "CommonLib/TrQuant.h"
#include "CommonLib/UnitTools.h"
#include "CommonLib/UnitPartitioner.h"
#include "EncoderLib/InterSearch.h"
#undef private
#undef protected

using namespace vvenc;

static bool rd( FILE* f, void* p, size_t bytes ) { return fread( p, 1, bytes, f ) == bytes; }

int main( int argc, char** argv )
{
  if( argc != 3 ) { fprintf( stderr, "usage: %s in out\n", argv[0] ); return 2; }
  FILE* fi = fopen( argv[1], "rb" ); FILE* fo = fopen( argv[2], "wb" );
  if( !fi || !fo ) return 2;
  SPS* sps = new SPS; PPS* pps = new PPS;
  sps->chromaFormatIdc = CHROMA_420; sps->CTUSize = 128; sps->MTS = true; sps->MTSInter = false;
  sps->bitDepths.recon[CH_L] = sps->bitDepths.recon[CH_C] = 10;
  const unsigned maxQt[3] = { 128, 128, 128 };
  PreCalcValues* pcv = new PreCalcValues( *sps, *pps, maxQt );
  RdCost* rdRow[2] = { new RdCost, new RdCost };
  rdRow[0]->create( false ); rdRow[1]->create( true );
  InterSearch* is = new InterSearch;
  is->m_pcRdCost = rdRow[1];
  TrQuant* trq = new TrQuant;
  int32_t kind = 0;
  while( rd( fi, &kind, 4 ) )
  {
    if( kind == 1 )
    {
      int32_t hd[3]; double wt[2];
      if( !rd( fi, hd, 12 ) || !rd( fi, wt, 16 ) ) return 2;
      const int w = hd[0], h = hd[1], allowed = hd[2];
      std::vector<Pel> resi[3];
      for( int c = 0; c < 3; c++ ) { resi[c].resize( ( size_t ) ( w >> ( c ? 1 : 0 ) ) * ( h >> ( c ? 1 : 0 ) ) ); if( !rd( fi, resi[c].data(), resi[c].size() * 2 ) ) return 2; }
      void* csMem = calloc( 1, sizeof( CodingStructure ) );
      CodingStructure* cs = reinterpret_cast<CodingStructure*>( csMem );
      const UnitArea area( CHROMA_420, Area( 0, 0, w, h ) );
      new ( &cs->area ) UnitArea( area );
      cs->sps = sps; cs->pcv = pcv;
      new ( &cs->m_pred ) PelStorage;
      cs->m_pred.create( area );
      cs->m_org = new PelStorage;
      cs->m_org->create( area );
      for( int c = 0; c < 3; c++ )
      {
        PelBuf o = cs->m_org->get( ComponentID( c ) ), p = cs->m_pred.get( ComponentID( c ) );
        for( int y = 0; y < ( int ) o.height; y++ )
          for( int x = 0; x < ( int ) o.width; x++ )
          {
            const int r = resi[c][( size_t ) y * o.width + x], og = r >> 1;
            o.at( x, y ) = ( Pel ) og; p.at( x, y ) = ( Pel ) ( og - r );
            if( ( int ) o.at( x, y ) - ( int ) p.at( x, y ) != r ) { fprintf( stderr, "residual %d is no difference of two Pels\n", r ); return 3; }
          }
      }
      CodingUnit* cu = reinterpret_cast<CodingUnit*>( calloc( 1, sizeof( CodingUnit ) ) );
      new ( static_cast<UnitArea*>( cu ) ) UnitArea( area );
      rdRow[1]->setDistortionWeight( COMP_Cb, wt[0] ); rdRow[1]->setDistortionWeight( COMP_Cr, wt[0] );
      if( rdRow[1]->getChromaWeight() != wt[0] ) { fprintf( stderr, "chroma weight %.17g does not survive getChromaWeight\n", wt[0] ); return 3; }
      rdRow[1]->m_DistScaleUnadjusted = std::numeric_limits<double>::infinity();
      is->m_skipSbtAll = false;
      memset( is->m_estMinDistSbt, 0x5a, sizeof( is->m_estMinDistSbt ) ); memset( is->m_sbtRdoOrder, 0x5a, sizeof( is->m_sbtRdoOrder ) );
      is->xCalcMinDistSbt( *cs, *cu, ( uint8_t ) allowed );
      if( is->getSkipSbtAll() ) { fprintf( stderr, "fast algorithm 1 fired with an infinite distortion scale\n" ); return 3; }
      uint64_t est[9]; uint8_t order[8];
      for( int k = 0; k < 9; k++ ) est[k] = is->getEstDistSbt( ( uint8_t ) k );
      memcpy( order, is->m_sbtRdoOrder, 8 );
      rdRow[1]->m_DistScaleUnadjusted = wt[1];
      is->m_skipSbtAll = false;
      is->xCalcMinDistSbt( *cs, *cu, ( uint8_t ) allowed );
      const uint8_t skip = is->getSkipSbtAll() ? 1 : 0;
      fwrite( est, 8, 9, fo ); fwrite( order, 1, 8, fo ); fwrite( &skip, 1, 1, fo );
      const int npx = w >= 16 ? 4 : w == 4 ? 1 : 2, npy = h >= 16 ? 4 : h == 4 ? 1 : 2;
      for( int row = 0; row < 2; row++ )
        for( int c = 0; c < 3; c++ )
        {
          uint64_t parts[16]; memset( parts, 0, sizeof( parts ) );
          const CPelBuf o = cs->m_org->get( ComponentID( c ) ), p = cs->m_pred.get( ComponentID( c ) );
          const int lx = o.width / npx, ly = o.height / npy;
          for( int j = 0; j < npy; j++ )
            for( int i = 0; i < npx; i++ )
              parts[4 * j + i] = rdRow[row]->getDistPart( o.subBuf( i * lx, j * ly, lx, ly ), p.subBuf( i * lx, j * ly, lx, ly ), 10, COMP_Y, DF_SSE );
          fwrite( parts, 8, 16, fo );
        }
      cs->m_pred.destroy(); cs->m_org->destroy(); delete cs->m_org; free( cu ); free( csMem );
    }
    else if( kind == 2 )
    {
      int32_t hd[3];
      if( !rd( fi, hd, 12 ) ) return 2;
      const int w = hd[0], h = hd[1], mode = hd[2];
      const uint8_t sbtIdx = ( uint8_t ) ( 1 + ( mode >> 1 ) ), sbtPos = ( uint8_t ) ( mode & 1 ), sbtInfo = ( uint8_t ) ( sbtIdx + ( sbtPos << 4 ) );      // ( what CU::getSbtIdx / getSbtPos take apart )
      if( CU::getSbtMode( CU::getSbtIdx( sbtInfo ), CU::getSbtPos( sbtInfo ) ) != mode ) { fprintf( stderr, "mode %d is not CU::getSbtMode( %d, %d )\n", mode, sbtIdx, sbtPos ); return 3; }
      const UnitArea area( CHROMA_420, Area( 0, 0, w, h ) );
      UnitArea tiles[2];
      Partitioning dst = tiles;
      void* csMem = calloc( 1, sizeof( CodingStructure ) );
      CodingStructure* cs = reinterpret_cast<CodingStructure*>( csMem );
      cs->sps = sps; cs->pcv = pcv;
      if( PartitionerImpl::getSbtTuTiling( dst, area, *cs, CU::getSbtTuSplit( sbtInfo ) ) != 2 ) return 3;
      for( int t = 0; t < 2; t++ )
        for( int c = 0; c < 3; c++ )
        {
          const CompArea& b = tiles[t].blocks[c];
          const int32_t r[4] = { ( int32_t ) b.x, ( int32_t ) b.y, ( int32_t ) b.width, ( int32_t ) b.height };
          fwrite( r, 4, 4, fo );
        }
      CodingUnit* cu = reinterpret_cast<CodingUnit*>( calloc( 1, sizeof( CodingUnit ) ) );
      new ( static_cast<UnitArea*>( cu ) ) UnitArea( area );
      cu->predMode = MODE_INTER; cu->sbtInfo = sbtInfo;
      const CompArea& coded = tiles[sbtPos].blocks[COMP_Y];
      TransformUnit tu( CHROMA_420, Area( coded.x, coded.y, coded.width, coded.height ) );
      tu.cu = cu; tu.cs = cs; tu.mtsIdx[COMP_Y] = 0;
      int trHor = DCT2, trVer = DCT2;
      trq->xSetTrTypes( tu, COMP_Y, coded.width, coded.height, trHor, trVer );
      const int32_t tr[2] = { trHor, trVer };
      fwrite( tr, 4, 2, fo );
      free( cu ); free( csMem );
    }
    else if( kind == 3 )
    {
      int32_t hd[2];
      if( !rd( fi, hd, 8 ) ) return 2;
      const int w = hd[0], h = hd[1];
      std::vector<Pel> a( ( size_t ) w * h ), b( ( size_t ) w * h );
      if( !rd( fi, a.data(), a.size() * 2 ) || !rd( fi, b.data(), b.size() * 2 ) ) return 2;
      const CPelBuf ba( a.data(), w, w, h ), bb( b.data(), w, w, h );
      const uint64_t s[2] = { rdRow[0]->getDistPart( ba, bb, 10, COMP_Y, DF_SSE ), rdRow[1]->getDistPart( ba, bb, 10, COMP_Y, DF_SSE ) };
      fwrite( s, 8, 2, fo );
    }
    else { fprintf( stderr, "record kind %d\n", kind ); return 2; }
  }
  fclose( fi ); fclose( fo );
  return 0;
}
