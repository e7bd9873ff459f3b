// deblock_golden_gen.cpp — records what the reference encoder's own deblocking filter computes, for tests/golden/deblock.npz (driver: tests/deblock_golden_gen.py).
//
// Not part of build() and of no Makefile: compiled and linked by hand against the reference library where its sources and oracle/_ref/libvvenc_core.a
// (made by `make -C oracle/ref core`) exist.  With R = the reference checkout and O = oracle/_ref:
//
//   g++ -std=c++14 -O2 -pthread -w -DTARGET_SIMD_X86=1 -DVVENC_SOURCE -DNDEBUG -I$O/gen -I$R/include -I$R/source/Lib/vvenc -I$R/source/Lib
//       -I$R/source/Lib/CommonLib -I$R/source/Lib/CommonLib/x86 -isystem $R/thirdparty tests/deblock_golden_gen.cpp
//       -Wl,--whole-archive $O/libvvenc_core.a -Wl,--no-whole-archive -o <somewhere outside the repository>/deblock_golden_gen
//
// LoopFilter::xDeblockArea<EDGE_VER> and <EDGE_HOR> (CommonLib/LoopFilter.cpp:405-462; protected members, reached by compiling the class headers with `private` and
// `protected` spelled `public`) are called THEMSELVES over every CTU of the picture, all of EDGE_VER first, the way EncoderLib/EncSlice.cpp:1020 / :1052 call them.  The
// CodingStructure / Picture / Slice / SPS / PreCalcValues they are handed are filled by hand, only as far as xDeblockArea and the two edge filters read them: the two
// LoopFilterParam maps (m_lfParam) with their size (m_mapSize), the unit scale, picture->cs, the slice's offsets and ClpRng, the SPS' bit depths and CTU size.
// Two objects: LoopFilter( false ) — the scalar row — and LoopFilter( true ) — the x86 row.  Each works on its own copy of the planes, and the two copies sit in DIFFERENT
// pseudo-random surroundings (32 samples on every side), so a result that depended on a sample outside the picture would show as a disagreement; the driver fails unless
// the rows agree.
//
// One picture per run, read from argv[1], answered in argv[2]:
//   int32 width, height, ctuSize, bitDepth, chroma (0: 4:0:0, 1: 4:2:0), clipBitDepth (ClpRng{ bd }: [0, 2^bd - 1], all a ClpRng of the reference can express),
//         betaOffsetDiv2[3], tcOffsetDiv2[3], reps
//   the planes (int16, width x height; with chroma two more of half size), the vertical map, the horizontal map ( height / 4 x width / 4 LoopFilterParam records each )
//   reps == 0 -> per row ( scalar, x86 ): the planes after EDGE_VER alone, then the planes after both passes
//   reps  > 0 -> double: the best seconds of one EDGE_VER + EDGE_HOR pass over the picture, the x86 row, one core (a context figure; the planes are restored between passes)
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
#include "CommonLib/Picture.h"
#include "CommonLib/CodingStructure.h"
#include "CommonLib/LoopFilter.h"
#undef private
#undef protected

using namespace vvenc;

static bool rd( FILE* f, void* p, size_t bytes ) { return fread( p, 1, bytes, f ) == bytes; }

static const int MARGIN = 32;

struct Plane
{
  int width = 0, height = 0, stride = 0;
  std::vector<Pel> store, start;
  Pel* at( int x, int y ) { return store.data() + ( size_t ) ( y + MARGIN ) * stride + MARGIN + x; }
  void set( const std::vector<Pel>& s, int w, int h, int bitDepth, uint32_t seed )
  {
    width = w; height = h; stride = ( ( w + 7 ) & ~7 ) + 2 * MARGIN;
    store.resize( ( size_t ) stride * ( h + 2 * MARGIN ) );
    for( Pel& v : store ) { seed = seed * 1664525u + 1013904223u; v = ( Pel ) ( ( seed >> 16 ) & ( ( 1u << bitDepth ) - 1 ) ); }
    for( int y = 0; y < h; y++ ) memcpy( at( 0, y ), s.data() + ( size_t ) y * w, ( size_t ) w * 2 );
    start = store;
  }
  void write( FILE* f ) { for( int y = 0; y < height; y++ ) fwrite( at( 0, y ), 2, width, f ); }
};

int main( int argc, char** argv )
{
  if( argc != 3 ) { fprintf( stderr, "usage: %s in out\n", argv[0] ); return 2; }
  FILE* fi = fopen( argv[1], "rb" ); FILE* fo = fopen( argv[2], "wb" );
  if( !fi || !fo ) return 2;
  int32_t hd[13];
  if( !rd( fi, hd, sizeof( hd ) ) ) return 2;
  const int width = hd[0], height = hd[1], ctu = hd[2], bitDepth = hd[3], nPlanes = hd[4] ? 3 : 1, reps = hd[12];
  const ChromaFormat fmt = hd[4] ? CHROMA_420 : CHROMA_400;
  std::vector<Pel> src[3];
  for( int c = 0; c < nPlanes; c++ )
  {
    src[c].resize( ( size_t ) ( width >> ( c > 0 ) ) * ( height >> ( c > 0 ) ) );
    if( !rd( fi, src[c].data(), src[c].size() * 2 ) ) return 2;
  }
  const int mapW = width / 4, mapH = height / 4;
  static_assert( sizeof( LoopFilterParam ) == 6, "LoopFilterParam is no longer 6 bytes" );
  std::vector<LoopFilterParam> maps[2];
  for( int d = 0; d < 2; d++ )
  {
    maps[d].resize( ( size_t ) mapW * mapH );
    if( !rd( fi, maps[d].data(), maps[d].size() * sizeof( LoopFilterParam ) ) ) return 2;
  }

  SPS* sps = new SPS;
  PPS* pps = new PPS;
  sps->chromaFormatIdc = fmt; sps->CTUSize = ctu; sps->bitDepths.recon[CH_L] = sps->bitDepths.recon[CH_C] = bitDepth;
  pps->picWidthInLumaSamples = width; pps->picHeightInLumaSamples = height;
  const unsigned maxQt[3] = { ( unsigned ) ctu, ( unsigned ) ctu, ( unsigned ) ctu };
  PreCalcValues* pcv = new PreCalcValues( *sps, *pps, maxQt );
  Slice* slice = new Slice;
  slice->deblockingFilterDisable = false;
  for( int c = 0; c < 3; c++ ) { slice->deblockingFilterBetaOffsetDiv2[c] = hd[6 + c]; slice->deblockingFilterTcOffsetDiv2[c] = hd[9 + c]; }
  slice->clpRngs.bd = hd[5];
  XUCache* cache = new XUCache;
  CodingStructure* cs = new CodingStructure( *cache, nullptr );
  Picture* pic = new Picture;
  cs->picture = pic; pic->cs = cs; cs->slice = slice; cs->sps = sps; cs->pps = pps; cs->pcv = pcv;
  for( int c = 0; c < 3; c++ ) cs->unitScale[c] = UnitScale( 2, 2 );      // LF_PARAM_MAP of luma is what is read: one record per 4 x 4 luma samples
  cs->m_mapSize[0] = Size( mapW, mapH );
  cs->m_lfParam[EDGE_VER] = maps[0].data(); cs->m_lfParam[EDGE_HOR] = maps[1].data();

  LoopFilter* row[2] = { new LoopFilter( false ), new LoopFilter( true ) };
  if( row[0]->xPelFilterLuma == row[1]->xPelFilterLuma || row[0]->xFilteringPandQ == row[1]->xFilteringPandQ ) { fprintf( stderr, "this build has no x86 row\n" ); return 3; }
  Plane pl[2][3];
  for( int r = 0; r < 2; r++ )
    for( int c = 0; c < nPlanes; c++ ) pl[r][c].set( src[c], width >> ( c > 0 ), height >> ( c > 0 ), bitDepth, r ? 99991u + c : 12345u + c );

  auto pass = [&]( int r, DeblockEdgeDir dir )
  {
    PelUnitBuf reco;
    reco.chromaFormat = fmt;
    for( int c = 0; c < nPlanes; c++ ) reco.bufs.push_back( PelBuf( pl[r][c].at( 0, 0 ), pl[r][c].stride, pl[r][c].width, pl[r][c].height ) );
    for( int y = 0; y < height; y += ctu )
      for( int x = 0; x < width; x += ctu )
      {
        const UnitArea ctuArea( fmt, Area( x, y, std::min( ctu, width - x ), std::min( ctu, height - y ) ) );
        if( dir == EDGE_VER ) row[r]->xDeblockArea<EDGE_VER>( *cs, ctuArea, MAX_NUM_CH, reco );
        else                  row[r]->xDeblockArea<EDGE_HOR>( *cs, ctuArea, MAX_NUM_CH, reco );
      }
  };

  if( reps > 0 )
  {
    double best = 1e30;
    for( int k = 0; k < reps; k++ )
    {
      for( int c = 0; c < nPlanes; c++ ) pl[1][c].store = pl[1][c].start;
      const auto t0 = std::chrono::steady_clock::now();
      pass( 1, EDGE_VER ); pass( 1, EDGE_HOR );
      best = std::min( best, std::chrono::duration<double>( std::chrono::steady_clock::now() - t0 ).count() );
    }
    fwrite( &best, 8, 1, fo );
  }
  else
    for( int r = 0; r < 2; r++ )
    {
      pass( r, EDGE_VER );
      for( int c = 0; c < nPlanes; c++ ) pl[r][c].write( fo );
      pass( r, EDGE_HOR );
      for( int c = 0; c < nPlanes; c++ ) pl[r][c].write( fo );
      // nothing outside the picture may have been written
      for( int c = 0; c < nPlanes; c++ )
      {
        Plane& p = pl[r][c];
        for( int y = -MARGIN; y < p.height + MARGIN; y++ )
          for( int x = -MARGIN; x < p.stride - MARGIN; x++ )
            if( ( x < 0 || x >= p.width || y < 0 || y >= p.height ) && *p.at( x, y ) != p.start[( size_t ) ( y + MARGIN ) * p.stride + MARGIN + x] ) { fprintf( stderr, "row %d plane %d: a sample outside the picture was written\n", r, c ); return 4; }
      }
    }
  fclose( fi ); fclose( fo );
  fflush( nullptr );
  _Exit( 0 );      // (the hand-filled structures are not torn down: their destructors would free what they do not own)
}
