// intra_golden_gen.cpp — records what the reference encoder's own intra prediction and HAD_2SAD cost compute, for tests/golden/intra.npz (driver: tests/intra_golden_gen.py).
//
// Not part of build() and of no Makefile: compiled and linked by hand against the reference library where its sources and oracle/_ref/libvvenc_core.a
// (made by `make -C oracle/ref core`) exist.  With R = the reference checkout and O = oracle/_ref:
//
//   g++ -std=c++14 -O2 -pthread -w -fno-access-control -DTARGET_SIMD_X86=1 -DVVENC_SOURCE -DNDEBUG -I$O/gen -I$R/include -I$R/source/Lib/vvenc -I$R/source/Lib
//       -I$R/source/Lib/CommonLib -I$R/source/Lib/CommonLib/x86 -I$R/source/Lib/EncoderLib -isystem $R/thirdparty tests/intra_golden_gen.cpp
//       -Wl,--whole-archive $O/libvvenc_core.a -Wl,--no-whole-archive -o <somewhere outside the repository>/intra_golden_gen
//
// Per block the case's reference lines are written into the IntraPrediction object's unfiltered buffer ( m_refBuffer[COMP_Y][PRED_BUF_UNFILTERED], the layout
// xFillReferenceSamples leaves: CommonLib/IntraPrediction.cpp:755-990 ), m_topRefLength, m_leftRefLength and m_refBufferStride[COMP_Y] are set as setReferenceArrayLengths and
// xFillReferenceSamples set them, and xFilterReferenceSamples (:994-1030) fills the filtered buffer (multi_ref_idx 0 only: the one index initIntraPatternChType can filter for).
// Per mode a CodingUnit is filled by hand ( intraDir[0], multiRefIdx, ispMode, mipFlag, bdpcmM, chromaFormat, the luma block ) and the reference's own initPredIntraParams (:409)
// and predIntraAng (:353) run on it.  predIntraAng reads exactly one thing through the CodingUnit's CodingStructure: cs->slice->clpRngs.  A CodingStructure and a Slice cannot be
// constructed stand-alone, so both are zeroed raw storage of their size with only `slice` and `clpRngs.bd` set; nothing else of them is touched by the two calls.
// The cost is RdCost::setDistParam( org, pred, bitDepth, DF_HAD_2SAD ) and its distFunc, on 32-byte aligned compact blocks (RdCost.cpp:1778).
//
// Everything runs twice: IntraPrediction( false ) with RdCost::create( false ) — the scalar row — and IntraPrediction( true ) with RdCost::create( true ) — the x86 row.  The
// program fails unless the six function pointers of IntraPrediction and the HAD_2SAD entry of the x86 row differ from the scalar ones.  (setDistParam takes the table's second
// row for bit depths above 10, RdCost.cpp:217; that row holds the same HAD_2SAD entry in this reference.)  The driver fails unless the rows agree in every sample and cost.
//
// One list per run, read from argv[1], answered in argv[2]:
//   int32 nBlocks, reps; per block int32 w, h, bitDepth, multiRefIdx, nModes, then nModes int32 modes, the lines ( int16, ( 2w + 1 + mri ) + ( 2h + 1 + mri ) ), the original
//   ( int16, w x h )
//   reps == 0 -> per row ( scalar, x86 ), block and mode: uint32 cost, then the prediction ( int16, w x h )
//   reps  > 0 -> double: the best seconds over the whole list of predict + score per mode with the lines in place, the x86 row, one core (a context figure)
#include <algorithm>
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "CommonLib/CommonDef.h"
#include "CommonLib/Unit.h"
#include "CommonLib/Buffer.h"
#include "CommonLib/Slice.h"
#include "CommonLib/CodingStructure.h"
#include "CommonLib/IntraPrediction.h"
#include "CommonLib/RdCost.h"

using namespace vvenc;

static bool rd( FILE* f, void* p, size_t bytes ) { return fread( p, 1, bytes, f ) == bytes; }

struct Block { int w, h, bitDepth, mri; std::vector<int32_t> modes; std::vector<Pel> lines, org; };

struct Row
{
  IntraPrediction* ip; RdCost* rc;
  CodingStructure* cs; Slice* slice; SPS* sps;
  Pel* org; Pel* pred;          // 32-byte aligned, 64 x 64
};

static void* zeroed( size_t bytes ) { void* p = aligned_alloc( 64, ( bytes + 63 ) & ~( size_t ) 63 ); memset( p, 0, ( bytes + 63 ) & ~( size_t ) 63 ); return p; }

static void setLines( Row& r, const Block& b )
{
  Pel* unf = r.ip->m_refBuffer[COMP_Y][PRED_BUF_UNFILTERED];
  memcpy( unf, b.lines.data(), b.lines.size() * sizeof( Pel ) );
  r.ip->m_topRefLength = 2 * b.w; r.ip->m_leftRefLength = 2 * b.h;
  r.ip->m_refBufferStride[COMP_Y] = 2 * b.w + 1 + b.mri;
  if( b.mri == 0 )
    r.ip->xFilterReferenceSamples( unf, r.ip->m_refBuffer[COMP_Y][PRED_BUF_FILTERED], CompArea( COMP_Y, CHROMA_420, 0, 0, b.w, b.h ), *r.sps, 0 );
  memcpy( r.org, b.org.data(), b.org.size() * sizeof( Pel ) );
  r.slice->clpRngs.bd = b.bitDepth;
}

static uint32_t oneMode( Row& r, const Block& b, int mode )
{
  CodingUnit cu;
  cu.cs = r.cs;
  cu.chromaFormat = CHROMA_420;
  cu.blocks.clear();
  cu.blocks.push_back( CompArea( COMP_Y, CHROMA_420, 0, 0, b.w, b.h ) );
  cu.intraDir[0] = mode; cu.intraDir[1] = 0;
  cu.multiRefIdx = b.mri; cu.ispMode = 0; cu.mipFlag = false; cu.bdpcmM[0] = 0; cu.bdpcmM[1] = 0;
  const CompArea area( COMP_Y, CHROMA_420, 0, 0, b.w, b.h );
  r.ip->initPredIntraParams( cu, area, *r.sps );
  PelBuf pred( r.pred, b.w, b.w, b.h );
  r.ip->predIntraAng( COMP_Y, pred, cu );
  DistParam dp = r.rc->setDistParam( CPelBuf( r.org, b.w, b.w, b.h ), CPelBuf( r.pred, b.w, b.w, b.h ), b.bitDepth, DF_HAD_2SAD );
  return ( uint32_t ) dp.distFunc( dp );
}

int main( int argc, char** argv )
{
  if( argc != 3 ) { fprintf( stderr, "usage: %s in out\n", argv[0] ); return 2; }
  FILE* fi = fopen( argv[1], "rb" ); FILE* fo = fopen( argv[2], "wb" );
  if( !fi || !fo ) return 2;
  int32_t hd[2];
  if( !rd( fi, hd, sizeof( hd ) ) ) return 2;
  const int nBlocks = hd[0], reps = hd[1];
  std::vector<Block> blocks( nBlocks );
  for( Block& b : blocks )
  {
    int32_t g[5];
    if( !rd( fi, g, sizeof( g ) ) ) return 2;
    b.w = g[0]; b.h = g[1]; b.bitDepth = g[2]; b.mri = g[3];
    b.modes.resize( g[4] ); b.lines.resize( ( 2 * b.w + 1 + b.mri ) + ( 2 * b.h + 1 + b.mri ) ); b.org.resize( ( size_t ) b.w * b.h );
    if( !rd( fi, b.modes.data(), b.modes.size() * 4 ) || !rd( fi, b.lines.data(), b.lines.size() * 2 ) || !rd( fi, b.org.data(), b.org.size() * 2 ) ) return 2;
  }

  Row rows[2];
  for( int pass = 0; pass < 2; pass++ )
  {
    Row& r = rows[pass];
    r.ip = new IntraPrediction( pass != 0 );
    r.ip->init( CHROMA_420, 10 );
    r.rc = new RdCost; r.rc->create( pass != 0 );
    r.cs = ( CodingStructure* ) zeroed( sizeof( CodingStructure ) ); r.slice = ( Slice* ) zeroed( sizeof( Slice ) ); r.sps = ( SPS* ) zeroed( sizeof( SPS ) );
    r.cs->slice = r.slice;
    r.org = ( Pel* ) zeroed( 64 * 64 * sizeof( Pel ) ); r.pred = ( Pel* ) zeroed( 64 * 64 * sizeof( Pel ) );
  }
  {
    const IntraPrediction &a = *rows[0].ip, &x = *rows[1].ip;
    if( a.IntraPredAngleLuma == x.IntraPredAngleLuma || a.IntraAnglePDPC == x.IntraAnglePDPC || a.IntraHorVerPDPC == x.IntraHorVerPDPC || a.IntraPredSampleFilter == x.IntraPredSampleFilter ||
        a.xPredIntraPlanar == x.xPredIntraPlanar || rows[0].rc->m_afpDistortFunc[0][DF_HAD_2SAD] == rows[1].rc->m_afpDistortFunc[0][DF_HAD_2SAD] )
    { fprintf( stderr, "this build has no x86 row\n" ); return 3; }
  }
  if( reps > 0 )
  {
    Row& r = rows[1];
    double best = 1e30; uint64_t sink = 0;
    for( int k = 0; k < reps; k++ )
    {
      const auto t0 = std::chrono::steady_clock::now();
      for( const Block& b : blocks ) { setLines( r, b ); for( int m : b.modes ) sink += oneMode( r, b, m ); }
      best = std::min( best, std::chrono::duration<double>( std::chrono::steady_clock::now() - t0 ).count() );
    }
    if( sink == 1 ) fprintf( stderr, " " );
    fwrite( &best, 8, 1, fo );
  }
  else
    for( int pass = 0; pass < 2; pass++ )
      for( const Block& b : blocks )
      {
        setLines( rows[pass], b );
        for( int m : b.modes )
        {
          memset( rows[pass].pred, 0x55, 64 * 64 * sizeof( Pel ) );
          const uint32_t c = oneMode( rows[pass], b, m );
          fwrite( &c, 4, 1, fo );
          fwrite( rows[pass].pred, sizeof( Pel ), ( size_t ) b.w * b.h, fo );
        }
      }
  fclose( fi ); fclose( fo );
  return 0;
}
