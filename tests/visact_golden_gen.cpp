// visact_golden_gen.cpp — records what the reference encoder's own visual-activity code computes, for tests/golden/visact.npz (driver: tests/visact_golden_gen.py).
//
// Not part of build() and of no Makefile: compiled and linked by hand against the reference library where its sources and oracle/_ref/libvvenc_core.a
// (made by `make -C oracle/ref core`) exist.  With R = the reference checkout and O = oracle/_ref:
//
//   g++ -std=c++14 -O2 -pthread -w -DTARGET_SIMD_X86=1 -DVVENC_SOURCE -DNDEBUG -I$O/gen -I$R/include -I$R/source/Lib/vvenc -I$R/source/Lib
//       -I$R/source/Lib/CommonLib -I$R/source/Lib/CommonLib/x86 -I$R/source/Lib/EncoderLib -isystem $R/thirdparty tests/visact_golden_gen.cpp
//       -Wl,--whole-archive $O/libvvenc_core.a -Wl,--no-whole-archive -o <somewhere outside the repository>/visact_golden_gen
//
// Per area of a list the reference's own calcSpatialVisAct, calcTemporalVisAct, updateVisAct (EncoderLib/BitAllocation.cpp:84-204), filterAndCalculateAverageActivity
// (:206-242) and AreaBuf::getAvg (CommonLib/Buffer.h:303-315) are called on the area's CPelBufs, the way BitAllocation::applyQPAdaptationSlice (:553-573, :610-616) calls
// them; the integer sums behind the doubles are taken from the six g_pelBufOP entries themselves, called with the pointers calcSpatialVisAct / calcTemporalVisAct hand them,
// and the doubles must be those sums over the reference's divisors.  Everything runs twice: with g_pelBufOP as its constructor leaves it — the scalar row — and after
// initPelBufOps( true ) — the x86 row; the planes of the two passes sit in DIFFERENT pseudo-random surroundings and at different strides per pointer, so a result that depended
// on a sample outside the area's plane would show as a disagreement.  The driver fails unless the rows agree.
//
// One list per run, read from argv[1], answered in argv[2]:
//   int32 bitDepth, nRows, nAreas, reps; per table row int32 width, height, flags (1: prev1 present, 2: prev2 present, 4: prev1 IS cur); per row the planes present (int16,
//   width x height: cur, prev1 unless it is cur, prev2); nAreas records of 40 bytes (vvhip_visact_area)
//   reps == 0 -> per row ( scalar, x86 ) and area: uint64 saAct, taAct, getAvg's sum, positions; double hpSpatAct, hpTempAct, hpVisAct; uint32 spatAct, tempAct, minAct,
//                visAct; int64 getAvg (-1: no mean rectangle)
//   reps  > 0 -> double: the best seconds of filterAndCalculateAverageActivity + getAvg over the whole list, the x86 row, one core (a context figure)
// order 1 is handed over as a frame rate of 24, order 2 as one of 32 (hpFrameRate of a picture with force2ndOrder, :532); order 0 is calcSpatialVisAct and updateVisAct alone.
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
#include "EncoderLib/BitAllocation.h"

using namespace vvenc;

static bool rd( FILE* f, void* p, size_t bytes ) { return fread( p, 1, bytes, f ) == bytes; }

static const int MARGIN = 32;

struct Plane
{
  int width = 0, height = 0, stride = 0;
  std::vector<Pel> store;
  const Pel* at( int x, int y ) const { return store.data() + ( size_t ) ( y + MARGIN ) * stride + MARGIN + x; }
  void set( const std::vector<Pel>& s, int w, int h, int bitDepth, int extra, uint32_t seed )
  {
    width = w; height = h; stride = w + 2 * MARGIN + extra;
    store.resize( ( size_t ) stride * ( h + 2 * MARGIN ) );
    for( Pel& v : store ) { seed = seed * 1664525u + 1013904223u; v = ( Pel ) ( ( seed >> 16 ) & ( ( 1u << bitDepth ) - 1 ) ); }
    for( int y = 0; y < h; y++ ) memcpy( store.data() + ( size_t ) ( y + MARGIN ) * stride + MARGIN, s.data() + ( size_t ) y * w, ( size_t ) w * 2 );
  }
};

struct AreaRec { uint8_t plane, ds, order, rsv0; int32_t x, y, w, h, mx, my, mw, mh, rsv1; };
struct Result  { uint64_t sums[4]; double hp[3]; uint32_t ints[4]; int64_t avg; };
static_assert( sizeof( AreaRec ) == 40 && sizeof( Result ) == 80, "record sizes" );

struct Row { Plane cur, p1, p2; bool has1 = false, has2 = false, same = false; };

static Result one( const Row& r, const AreaRec& a, int bitDepth )
{
  Result o; memset( &o, 0, sizeof( o ) );
  const Pel* s0 = r.cur.at( a.x, a.y ); const int st0 = r.cur.stride;
  const Pel* s1 = !r.has1 ? nullptr : r.same ? s0 : r.p1.at( a.x, a.y ); const int st1 = r.same ? st0 : r.p1.stride;
  const Pel* s2 = ( r.has2 && a.order == 2 ) ? r.p2.at( a.x, a.y ) : nullptr; const int st2 = r.p2.stride;
  const bool uhd = a.ds != 0;
  const uint32_t frameRate = a.order == 2 ? 32 : 24;
  VisAct va;
  calcSpatialVisAct( s0, st0, a.h, a.w, bitDepth, uhd, va );
  if( a.order ) calcTemporalVisAct( s0, st0, a.h, a.w, s1, st1, s2, st2, frameRate, bitDepth, uhd, va );
  updateVisAct( va, bitDepth );
  o.hp[0] = va.hpSpatAct; o.hp[1] = va.hpTempAct; o.hp[2] = va.hpVisAct;
  o.ints[0] = va.spatAct; o.ints[1] = va.tempAct; o.ints[2] = va.minAct; o.ints[3] = va.visAct;
  if( a.order )
  {
    unsigned minAct = ~0u, spAct = ~0u;
    const double hp = filterAndCalculateAverageActivity( s0, st0, a.h, a.w, s1, st1, s2, st2, frameRate, bitDepth, uhd, &minAct, &spAct );
    if( memcmp( &hp, &va.hpVisAct, 8 ) || minAct != va.minAct || spAct != va.spatAct ) { fprintf( stderr, "filterAndCalculateAverageActivity differs from its three parts\n" ); exit( 5 ); }
  }
  o.avg = a.mw > 0 ? ( int64_t ) CPelBuf( r.cur.at( a.mx, a.my ), st0, a.mw, a.mh ).getAvg() : -1;
  // the sums themselves: the table entries with the pointers calcSpatialVisAct / calcTemporalVisAct hand them
  const int skip = uhd ? 2 : 1;
  o.sums[0] = uhd ? g_pelBufOP.AvgHighPassWithDownsampling( a.w, a.h, s0 + skip * st0, st0 ) : g_pelBufOP.AvgHighPass( a.w, a.h, s0 + st0, st0 );
  if( a.order == 1 )
    o.sums[1] = uhd ? g_pelBufOP.AvgHighPassWithDownsamplingDiff1st( a.w, a.h, s0 + 2 * st0, s1 + 2 * st1, st0, st1 ) : g_pelBufOP.HDHighPass( a.w, a.h, s0 + st0, s1 + st1, st0, st1 );
  else if( a.order == 2 )
    o.sums[1] = uhd ? g_pelBufOP.AvgHighPassWithDownsamplingDiff2nd( a.w, a.h, s0 + 2 * st0, s1 + 2 * st1, s2 + 2 * st2, st0, st1, st2 )
                    : g_pelBufOP.HDHighPass2( a.w, a.h, s0 + st0, s1 + st1, s2 + st2, st0, st1, st2 );
  o.sums[3] = uhd ? ( uint64_t ) ( ( a.w - 4 ) / 2 ) * ( ( a.h - 4 ) / 2 ) : ( uint64_t ) ( a.w - 2 ) * ( a.h - 2 );
  const double div = uhd ? double( ( a.w - 4 ) * ( a.h - 4 ) ) : double( ( a.w - 2 ) * ( a.h - 2 ) );
  const double sp = double( o.sums[0] ) / div, tp = double( o.sums[1] ) / div;
  const bool bypass = r.same && a.order == 1;
  if( memcmp( &sp, &va.hpSpatAct, 8 ) || ( a.order && !bypass && memcmp( &tp, &va.hpTempAct, 8 ) ) || ( bypass && ( va.hpTempAct != 0.0 || o.sums[1] != 0 ) ) )
  { fprintf( stderr, "a table entry's sum is not the one behind calcSpatialVisAct / calcTemporalVisAct\n" ); exit( 5 ); }
  if( a.mw > 0 )
  {
    int64_t acc = 0;
    for( int y = 0; y < a.mh; y++ ) for( int x = 0; x < a.mw; x++ ) acc += *r.cur.at( a.mx + x, a.my + y );
    o.sums[2] = ( uint64_t ) acc;
    if( ( acc + ( ( ( int64_t ) a.mw * a.mh ) >> 1 ) ) / ( ( int64_t ) a.mw * a.mh ) != o.avg ) { fprintf( stderr, "getAvg is not its accumulator's rounded mean\n" ); exit( 5 ); }
  }
  return o;
}

int main( int argc, char** argv )
{
  if( argc != 3 ) { fprintf( stderr, "usage: %s in out\n", argv[0] ); return 2; }
  FILE* fi = fopen( argv[1], "rb" ); FILE* fo = fopen( argv[2], "wb" );
  if( !fi || !fo ) return 2;
  int32_t hd[4];
  if( !rd( fi, hd, sizeof( hd ) ) ) return 2;
  const int bitDepth = hd[0], nRows = hd[1], nAreas = hd[2], reps = hd[3];
  std::vector<int32_t> geo( 3 * nRows );
  if( !rd( fi, geo.data(), geo.size() * 4 ) ) return 2;
  std::vector<std::vector<Pel>> src( 3 * nRows );
  for( int r = 0; r < nRows; r++ )
  {
    const size_t n = ( size_t ) geo[3 * r] * geo[3 * r + 1];
    const int fl = geo[3 * r + 2];
    const bool want[3] = { true, ( fl & 1 ) && !( fl & 4 ), ( fl & 2 ) != 0 };
    for( int k = 0; k < 3; k++ ) if( want[k] ) { src[3 * r + k].resize( n ); if( !rd( fi, src[3 * r + k].data(), n * 2 ) ) return 2; }
  }
  std::vector<AreaRec> areas( nAreas );
  if( !rd( fi, areas.data(), areas.size() * sizeof( AreaRec ) ) ) return 2;

  PelBufferOps scalar;      // the constructor's entries: the scalar row
  for( int pass = 0; pass < 2; pass++ )
  {
    if( pass == 0 ) g_pelBufOP = scalar;
    else
    {
      g_pelBufOP.initPelBufOps( true );
      if( g_pelBufOP.AvgHighPass == scalar.AvgHighPass || g_pelBufOP.AvgHighPassWithDownsampling == scalar.AvgHighPassWithDownsampling || g_pelBufOP.HDHighPass == scalar.HDHighPass ||
          g_pelBufOP.HDHighPass2 == scalar.HDHighPass2 || g_pelBufOP.AvgHighPassWithDownsamplingDiff1st == scalar.AvgHighPassWithDownsamplingDiff1st ||
          g_pelBufOP.AvgHighPassWithDownsamplingDiff2nd == scalar.AvgHighPassWithDownsamplingDiff2nd ) { fprintf( stderr, "this build has no x86 row\n" ); return 3; }
    }
    if( reps > 0 && pass == 0 ) continue;
    std::vector<Row> rows( nRows );
    for( int r = 0; r < nRows; r++ )
    {
      const int w = geo[3 * r], h = geo[3 * r + 1], fl = geo[3 * r + 2];
      Row& R = rows[r];
      R.has1 = fl & 1; R.has2 = ( fl & 2 ) != 0; R.same = ( fl & 4 ) != 0;
      R.cur.set( src[3 * r], w, h, bitDepth, pass ? 5 : 0, 12345u + 7 * r + 1000 * pass );
      if( R.has1 && !R.same ) R.p1.set( src[3 * r + 1], w, h, bitDepth, pass ? 0 : 11, 23456u + 7 * r + 1000 * pass );
      if( R.has2 ) R.p2.set( src[3 * r + 2], w, h, bitDepth, pass ? 2 : 3, 34567u + 7 * r + 1000 * pass );
    }
    if( reps > 0 )
    {
      double best = 1e30;
      uint64_t sink = 0;
      for( int k = 0; k < reps; k++ )
      {
        const auto t0 = std::chrono::steady_clock::now();
        for( const AreaRec& a : areas )
        {
          const Row& r = rows[a.plane];
          const Pel* s0 = r.cur.at( a.x, a.y );
          unsigned mn = 0, sp = 0;
          const double hp = filterAndCalculateAverageActivity( s0, r.cur.stride, a.h, a.w, r.p1.at( a.x, a.y ), r.p1.stride, a.order == 2 ? r.p2.at( a.x, a.y ) : nullptr, r.p2.stride,
                                                               a.order == 2 ? 32 : 24, bitDepth, a.ds != 0, &mn, &sp );
          sink += ( uint64_t ) hp + mn + sp;
          if( a.mw > 0 ) sink += CPelBuf( r.cur.at( a.mx, a.my ), r.cur.stride, a.mw, a.mh ).getAvg();
        }
        best = std::min( best, std::chrono::duration<double>( std::chrono::steady_clock::now() - t0 ).count() );
      }
      if( sink == 1 ) fprintf( stderr, " " );
      fwrite( &best, 8, 1, fo );
    }
    else
      for( const AreaRec& a : areas )
      {
        const Result o = one( rows[a.plane], a, bitDepth );
        fwrite( &o, sizeof( o ), 1, fo );
      }
  }
  fclose( fi ); fclose( fo );
  return 0;
}
