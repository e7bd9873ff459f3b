// sao_golden_gen.cpp — records what the reference encoder's own SAO code computes, for tests/golden/sao.npz (driver: tests/sao_golden_gen.py).
//
// Not part of build() and of no Makefile: compiled and linked by hand against the reference library where its sources and oracle/_ref/libvvenc_core.a
// (made by `make -C oracle/ref core`) exist.  With R = the reference checkout and O = oracle/_ref:
//
//   g++ -std=c++14 -O2 -pthread -w -DTARGET_SIMD_X86=1 -DVVENC_SOURCE -DNDEBUG -I$O/gen -I$R/include -I$R/source/Lib/vvenc -I$R/source/Lib
//       -I$R/source/Lib/CommonLib -I$R/source/Lib/CommonLib/x86 -isystem $R/thirdparty tests/sao_golden_gen.cpp
//       -Wl,--whole-archive $O/libvvenc_core.a -Wl,--no-whole-archive -o <somewhere outside the repository>/sao_golden_gen
//
// EncSampleAdaptiveOffset::getBlkStats (EncoderLib/EncSampleAdaptiveOffset.cpp:810-929; a private member) and the offsetBlock table entry (CommonLib/SampleAdaptiveOffset.h:101;
// protected) are called THEMSELVES, reached by compiling the class headers with `private` and `protected` spelled `public`.  Two objects: one whose six table entries are
// those of SampleAdaptiveOffset( false ) — the scalar row — and one as the encoder constructs it — the x86 row.  Every record is answered for both rows; the driver fails
// unless they agree.  The two rows work on copies of the planes that sit in DIFFERENT pseudo-random surroundings (32 samples on every side), so that a result which
// depended on a sample outside the plane would show as a disagreement.
//
// Records, read from argv[1] and answered in argv[2] in the same order:
//   0  planes: int32 isChroma, bitDepth, width, height, then the original and the deblocked plane, int16 — no answer; the planes stay current
//   1  statistics of a CTU: int32 x, y, w, h, flags (bit 0 left, 1 above, 2 above-left, 3 right, 4 below, 5 above-right) -> int64 [2][5][2][32]: SAOStatData[5] of both rows
//   2  offset filter of a CTU: int32 x, y, w, h, type, band, availMask, clipBitDepth, offs[5] -> int16 [2][h][w]: res (a copy of src before the call) of both rows;
//      the clip range is ClpRng{ clipBitDepth } = [0, 2^clipBitDepth - 1], all a ClpRng of the reference can express.
//      offset[] as reconstructBlkSAOParam leaves it: EO offset[k] = offs[k]; BO offset[( band + i ) % 32] = offs[i], i < 4, the rest 0
//   3  timing on the current planes (a context figure, one core): int32 ctuW, ctuH, reps -> double [2]: the best seconds of one pass of getBlkStats over every CTU with the
//      picture's borders as availability, and of one pass of offsetBlock (EO_135, all CTUs on) — the x86 row, as the encoder runs it
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
#include "CommonLib/SampleAdaptiveOffset.h"
#include "EncoderLib/EncSampleAdaptiveOffset.h"
#undef private
#undef protected

using namespace vvenc;

static bool rd( FILE* f, void* p, size_t bytes ) { return fread( p, 1, bytes, f ) == bytes; }

static const int MARGIN = 32;

// like the encoder's picture buffers: 64-byte aligned, line pitch a multiple of 8 samples — the x86 row stores whole aligned vectors (a CTU starts at a multiple of 8
// samples) and, where a width is no multiple of 8, past the block into the margin
struct Planes
{
  int width = 0, height = 0, stride = 0;
  size_t elems = 0;
  Pel* org = nullptr; Pel* src = nullptr; Pel* res = nullptr;
  Pel* at( Pel* b, int x, int y ) { return b + ( size_t ) ( y + MARGIN ) * stride + MARGIN + x; }
  Pel* orgAt( int x, int y ) { return at( org, x, y ); }
  Pel* srcAt( int x, int y ) { return at( src, x, y ); }
  Pel* resAt( int x, int y ) { return at( res, x, y ); }
  void set( const std::vector<Pel>& o, const std::vector<Pel>& s, int w, int h, int bitDepth, uint32_t seed )
  {
    free( org ); free( src ); free( res );
    width = w; height = h; stride = ( ( w + 7 ) & ~7 ) + 2 * MARGIN;
    elems = ( size_t ) stride * ( h + 2 * MARGIN );
    const size_t bytes = ( elems * sizeof( Pel ) + 63 ) & ~( size_t ) 63;
    org = ( Pel* ) aligned_alloc( 64, bytes ); src = ( Pel* ) aligned_alloc( 64, bytes ); res = ( Pel* ) aligned_alloc( 64, bytes );
    for( size_t i = 0; i < elems; i++ )
    {
      seed = seed * 1664525u + 1013904223u; org[i] = ( Pel ) ( ( seed >> 16 ) & ( ( 1u << bitDepth ) - 1 ) );
      seed = seed * 1664525u + 1013904223u; src[i] = ( Pel ) ( ( seed >> 16 ) & ( ( 1u << bitDepth ) - 1 ) );
    }
    for( int y = 0; y < h; y++ ) { memcpy( orgAt( 0, y ), o.data() + ( size_t ) y * w, ( size_t ) w * 2 ); memcpy( srcAt( 0, y ), s.data() + ( size_t ) y * w, ( size_t ) w * 2 ); }
  }
};

int main( int argc, char** argv )
{
  if( argc != 3 ) { fprintf( stderr, "usage: %s in out\n", argv[0] ); return 2; }
  FILE* fi = fopen( argv[1], "rb" ); FILE* fo = fopen( argv[2], "wb" );
  if( !fi || !fo ) return 2;
  SampleAdaptiveOffset scalarTable( false );
  EncSampleAdaptiveOffset* row[2] = { new EncSampleAdaptiveOffset, new EncSampleAdaptiveOffset };
  row[0]->offsetBlock = scalarTable.offsetBlock;
  row[0]->calcSaoStatisticsBo = scalarTable.calcSaoStatisticsBo;   row[0]->calcSaoStatisticsEo0 = scalarTable.calcSaoStatisticsEo0;
  row[0]->calcSaoStatisticsEo90 = scalarTable.calcSaoStatisticsEo90; row[0]->calcSaoStatisticsEo135 = scalarTable.calcSaoStatisticsEo135;
  row[0]->calcSaoStatisticsEo45 = scalarTable.calcSaoStatisticsEo45;
  if( row[1]->offsetBlock == row[0]->offsetBlock || row[1]->calcSaoStatisticsEo0 == row[0]->calcSaoStatisticsEo0 ) { fprintf( stderr, "this build has no x86 row\n" ); return 3; }
  for( int r = 0; r < 2; r++ ) row[r]->SampleAdaptiveOffset::init( CHROMA_420, 128, 128, 0, 0 );
  Planes pl[2];
  int isChroma = 0, bitDepth = 10;
  int32_t kind = 0;
  while( rd( fi, &kind, 4 ) )
  {
    if( kind == 0 )
    {
      int32_t hd[4];
      if( !rd( fi, hd, 16 ) ) return 2;
      isChroma = hd[0]; bitDepth = hd[1];
      std::vector<Pel> o( ( size_t ) hd[2] * hd[3] ), s( o.size() );
      if( !rd( fi, o.data(), o.size() * 2 ) || !rd( fi, s.data(), s.size() * 2 ) ) return 2;
      pl[0].set( o, s, hd[2], hd[3], bitDepth, 12345u ); pl[1].set( o, s, hd[2], hd[3], bitDepth, 99991u );
    }
    else if( kind == 1 )
    {
      int32_t hd[5];
      if( !rd( fi, hd, 20 ) ) return 2;
      for( int r = 0; r < 2; r++ )
      {
        SAOStatData st[5];
        memset( st, 0x5a, sizeof( st ) );
        row[r]->getBlkStats( isChroma ? COMP_Cb : COMP_Y, bitDepth, st, pl[r].srcAt( hd[0], hd[1] ), pl[r].orgAt( hd[0], hd[1] ), pl[r].stride, pl[r].stride, hd[2], hd[3],
                             hd[4] & 1, hd[4] & 8, hd[4] & 2, hd[4] & 16, hd[4] & 4, hd[4] & 32 );
        static_assert( sizeof( st ) == 5 * 2 * 32 * 8, "SAOStatData is no longer { int64 diff[32]; int64 count[32]; }" );
        fwrite( st, sizeof( st ), 1, fo );
      }
    }
    else if( kind == 2 )
    {
      int32_t hd[13];
      if( !rd( fi, hd, 52 ) ) return 2;
      const int x = hd[0], y = hd[1], w = hd[2], h = hd[3], type = hd[4], band = hd[5];
      for( int r = 0; r < 2; r++ )
      {
        int offset[MAX_NUM_SAO_CLASSES];
        memset( offset, 0, sizeof( offset ) );
        if( type == SAO_TYPE_BO ) { for( int i = 0; i < 4; i++ ) offset[( band + i ) % MAX_NUM_SAO_CLASSES] = hd[8 + i]; }
        else                      { for( int i = 0; i < 5; i++ ) offset[i] = hd[8 + i]; }
        memcpy( pl[r].res, pl[r].src, pl[r].elems * sizeof( Pel ) );
        ClpRng clp; clp.bd = hd[7];
        row[r]->offsetBlock( bitDepth, clp, type, offset, band, pl[r].srcAt( x, y ), pl[r].resAt( x, y ), pl[r].stride, pl[r].stride, w, h, ( uint8_t ) hd[6], row[r]->m_signLineBuf1, row[r]->m_signLineBuf2 );
        for( int j = 0; j < h; j++ ) fwrite( pl[r].resAt( x, y + j ), 2, w, fo );
      }
    }
    else if( kind == 3 )
    {
      int32_t hd[3];
      if( !rd( fi, hd, 12 ) ) return 2;
      const int cw = hd[0], ch = hd[1], gx = ( pl[1].width + cw - 1 ) / cw, gy = ( pl[1].height + ch - 1 ) / ch;
      std::vector<SAOStatData> st( ( size_t ) gx * gy * 5 );
      double best[2] = { 1e30, 1e30 };
      for( int rep = 0; rep < hd[2]; rep++ )
        for( int what = 0; what < 2; what++ )
        {
          const auto t0 = std::chrono::steady_clock::now();
          for( int cy = 0; cy < gy; cy++ )
            for( int cx = 0; cx < gx; cx++ )
            {
              const int x = cx * cw, y = cy * ch, w = std::min( cw, pl[1].width - x ), h = std::min( ch, pl[1].height - y );
              const bool L = cx > 0, A = cy > 0, R = cx < gx - 1, B = cy < gy - 1;
              if( what == 0 )
                row[1]->getBlkStats( isChroma ? COMP_Cb : COMP_Y, bitDepth, &st[( size_t ) ( cy * gx + cx ) * 5], pl[1].srcAt( x, y ), pl[1].orgAt( x, y ), pl[1].stride, pl[1].stride, w, h, L, R, A, B, L && A, A && R );
              else
              {
                int offset[MAX_NUM_SAO_CLASSES] = { 3, 1, 0, -1, -3 };
                ClpRng clp; clp.bd = bitDepth;
                const uint8_t m = ( uint8_t ) ( ( L ? 1 : 0 ) | ( R ? 2 : 0 ) | ( A ? 4 : 0 ) | ( B ? 8 : 0 ) | ( L && A ? 16 : 0 ) | ( R && A ? 32 : 0 ) | ( L && B ? 64 : 0 ) | ( R && B ? 128 : 0 ) );
                row[1]->offsetBlock( bitDepth, clp, SAO_TYPE_EO_135, offset, 0, pl[1].srcAt( x, y ), pl[1].resAt( x, y ), pl[1].stride, pl[1].stride, w, h, m,
                                     row[1]->m_signLineBuf1, row[1]->m_signLineBuf2 );
              }
            }
          const double s = std::chrono::duration<double>( std::chrono::steady_clock::now() - t0 ).count();
          best[what] = std::min( best[what], s );
        }
      fwrite( best, 8, 2, fo );
    }
    else { fprintf( stderr, "record kind %d\n", kind ); return 2; }
  }
  fclose( fi ); fclose( fo );
  return 0;
}
