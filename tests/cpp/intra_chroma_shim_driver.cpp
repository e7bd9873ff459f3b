// intra_chroma_shim_driver.cpp — TEST INFRASTRUCTURE: runs vvhip::IntraChromaOps (the shim's entry to vvhip_intra_chroma_modes_batch) on a list of blocks read from a file
// (tests/test_gpu_intra_chroma_shim.py writes it from the fixture's cases, compiles this file against libvvenc_hip_shim.so and checks the outputs against
// tests/golden/intra_chroma.npz).
//   intra_chroma_shim_driver DIR   DIR/list.bin: int32 nBlocks, lumaWidth, lumaHeight, lumaStride, the luma plane ( lumaHeight x lumaStride samples ); per block int32 width,
//                           height, bitDepth, above, left, aboveRightUnits, leftBelowUnits, firstRow, verCollocated, lumaX, lumaY, refStrideCb, refStrideCr, orgStride, modeMask,
//                           predMask, cand[8], then the Cb and the Cr reference buffer ( refStride + 2 height + 1 samples each: the top row at 0, the left row at refStride ), the
//                           Cb and the Cr original ( height x orgStride samples each )
//   -> DIR/cost.bin: per block uint32 [8] (0 where a slot was not scored); DIR/pred.bin: per block, component and slot of predMask (ascending) the prediction, compact;
//      DIR/sel.bin: per block and reduceIntraChromaModesFullRD in ( false, true ): sortedModes[8], disabled[70]; DIR/flow.txt: one line per step that went as it must
//   intra_chroma_shim_driver --select IN OUT   (no device) IN: int32 n; per entry uint32 cost[8], uint8 cand[8], uint8 reduce -> OUT: per entry sortedModes[8], disabled[70]
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include "../../vvenc_amd/csrc/host/vvenc_hip_shim.h"

static std::vector<char> slurp( const std::string& p )
{
  FILE* f = fopen( p.c_str(), "rb" ); if( !f ) { perror( p.c_str() ); exit( 2 ); }
  fseek( f, 0, SEEK_END ); const long n = ftell( f ); fseek( f, 0, SEEK_SET );
  std::vector<char> b( n ); if( fread( b.data(), 1, n, f ) != ( size_t ) n ) exit( 2 );
  fclose( f ); return b;
}
template<class T> static void dump( const std::string& p, const T* v, size_t n ) { FILE* f = fopen( p.c_str(), "wb" ); fwrite( v, sizeof( T ), n, f ); fclose( f ); }

struct Block
{
  int w, h, bitDepth, above, left, arUnits, lbUnits, firstRow, verColl, lumaX, lumaY, refStride[2], orgStride, modeMask, predMask;
  uint8_t cand[8];
  const vvhip::Pel* ref[2]; const vvhip::Pel* org[2];
};

static int addOne( vvhip::IntraChromaOps& ops, const Block& b )
{
  return ops.add( b.ref[0], b.refStride[0], b.ref[1], b.refStride[1], b.org[0], b.org[1], b.orgStride, b.lumaX, b.lumaY, b.w, b.h, b.bitDepth, b.above != 0, b.left != 0, b.arUnits, b.lbUnits,
                  b.firstRow != 0, b.verColl != 0, b.cand, ( unsigned ) b.modeMask, ( unsigned ) b.predMask );
}

static void collect( const vvhip::IntraChromaOps& ops, const std::vector<Block>& blocks, std::vector<uint32_t>& cost, std::vector<vvhip::Pel>& pred )
{
  cost.clear(); pred.clear();
  for( int i = 0; i < ops.count(); i++ )
  {
    for( int s = 0; s < 8; s++ ) cost.push_back( ops.cost( i, s ) );
    for( int c = 0; c < 2; c++ )
      for( int s = 0; s < 8; s++ )
        if( const vvhip::Pel* p = ops.pred( i, c, s ) ) pred.insert( pred.end(), p, p + ( size_t ) blocks[i].w * blocks[i].h );
  }
}

static int selectOnly( const char* in, const char* out )
{
  const std::vector<char> tb = slurp( in );
  int32_t n; memcpy( &n, tb.data(), 4 );
  if( tb.size() != 4 + ( size_t ) n * 41 ) return 2;
  std::vector<uint8_t> res;
  for( int i = 0; i < n; i++ )
  {
    const char* p = tb.data() + 4 + ( size_t ) i * 41;
    uint32_t cost[8]; uint8_t cand[8], sorted[8]; bool disabled[70];
    memcpy( cost, p, 32 ); memcpy( cand, p + 32, 8 );
    vvhip::IntraChromaOps::select( cost, cand, p[40] != 0, sorted, disabled );
    res.insert( res.end(), sorted, sorted + 8 );
    for( int m = 0; m < 70; m++ ) res.push_back( disabled[m] ? 1 : 0 );
  }
  dump( out, res.data(), res.size() );
  return 0;
}

int main( int argc, char** argv )
{
  if( argc == 4 && !strcmp( argv[1], "--select" ) ) return selectOnly( argv[2], argv[3] );
  if( argc < 2 ) return 2;
  const std::string dir = argv[1];
  try
  {
    const std::vector<char> tb = slurp( dir + "/list.bin" );
    const char* p = tb.data();
    int32_t hd[4]; memcpy( hd, p, sizeof( hd ) ); p += sizeof( hd );
    const int nBlocks = hd[0], lumaW = hd[1], lumaH = hd[2], lumaStride = hd[3];
    const vvhip::Pel* luma = reinterpret_cast<const vvhip::Pel*>( p ); p += ( size_t ) lumaStride * lumaH * sizeof( vvhip::Pel );
    std::vector<Block> blocks( nBlocks );
    for( Block& b : blocks )
    {
      int32_t g[24]; memcpy( g, p, sizeof( g ) ); p += sizeof( g );
      b.w = g[0]; b.h = g[1]; b.bitDepth = g[2]; b.above = g[3]; b.left = g[4]; b.arUnits = g[5]; b.lbUnits = g[6]; b.firstRow = g[7]; b.verColl = g[8]; b.lumaX = g[9]; b.lumaY = g[10];
      b.refStride[0] = g[11]; b.refStride[1] = g[12]; b.orgStride = g[13]; b.modeMask = g[14]; b.predMask = g[15];
      for( int k = 0; k < 8; k++ ) b.cand[k] = ( uint8_t ) g[16 + k];
      for( int c = 0; c < 2; c++ ) { b.ref[c] = reinterpret_cast<const vvhip::Pel*>( p ); p += ( size_t ) ( b.refStride[c] + 2 * b.h + 1 ) * sizeof( vvhip::Pel ); }
      for( int c = 0; c < 2; c++ ) { b.org[c] = reinterpret_cast<const vvhip::Pel*>( p ); p += ( size_t ) b.h * b.orgStride * sizeof( vvhip::Pel ); }
    }
    if( p != tb.data() + tb.size() ) return 2;
    std::string flow;
    vvhip::IntraChromaOps ops;
    ops.begin();
    if( ops.run() || ops.count() != 0 ) return 3;
    flow += "an empty list does not run\n";
    Block bad = blocks[0];
    if( addOne( ops, bad ) >= 0 ) return 3;                                                 // (no luma plane yet, and block 0 asks for modes >= 67)
    ops.setLuma( luma, lumaStride, lumaW, lumaH );
    bad = blocks[0]; bad.w = 12;             if( addOne( ops, bad ) >= 0 ) return 3;
    bad = blocks[0]; bad.bitDepth = 13;      if( addOne( ops, bad ) >= 0 ) return 3;
    bad = blocks[0]; bad.cand[3] = 70;       if( addOne( ops, bad ) >= 0 ) return 3;
    bad = blocks[0]; bad.arUnits = bad.w;    if( addOne( ops, bad ) >= 0 ) return 3;
    bad = blocks[0]; bad.above = 0; bad.arUnits = 1; if( addOne( ops, bad ) >= 0 ) return 3;
    bad = blocks[0]; bad.predMask = 1; bad.modeMask = 0xfe; if( addOne( ops, bad ) >= 0 ) return 3;
    bad = blocks[0]; bad.refStride[1] = 2 * bad.w; if( addOne( ops, bad ) >= 0 ) return 3;
    bad = blocks[0]; bad.left = 1; bad.lumaX = 2; if( addOne( ops, bad ) >= 0 ) return 3;
    bad = blocks[0]; bad.lumaY = lumaH - 2 * bad.h + 1; if( addOne( ops, bad ) >= 0 ) return 3;
    if( ops.count() != 0 ) return 3;
    flow += "a missing luma plane, a side of 12, 13 bits, mode 70, too many above-right units, units without their side, an unscored prediction, a short reference pitch and a footprint outside the plane are refused\n";
    for( const Block& b : blocks ) if( addOne( ops, b ) < 0 ) return 3;
    if( ops.count() != nBlocks || !ops.run() ) return 3;
    std::vector<uint32_t> cost; std::vector<vvhip::Pel> pred;
    collect( ops, blocks, cost, pred );
    dump( dir + "/cost.bin", cost.data(), cost.size() );
    dump( dir + "/pred.bin", pred.data(), pred.size() );
    std::vector<uint8_t> sel;
    for( int i = 0; i < nBlocks; i++ )
      for( int red = 0; red < 2; red++ )
      {
        uint8_t sorted[8]; bool disabled[70];
        ops.select( i, red != 0, sorted, disabled );
        sel.insert( sel.end(), sorted, sorted + 8 );
        for( int m = 0; m < 70; m++ ) sel.push_back( disabled[m] ? 1 : 0 );
      }
    dump( dir + "/sel.bin", sel.data(), sel.size() );
    flow += "the list\n";
    // the list again in reverse order on the same object: a block's results do not depend on its place
    ops.begin();
    ops.setLuma( luma, lumaStride, lumaW, lumaH );
    for( int i = nBlocks - 1; i >= 0; i-- ) if( addOne( ops, blocks[i] ) < 0 ) return 3;
    if( !ops.run() ) return 3;
    size_t at = 0;
    for( int i = 0; i < nBlocks; i++ )
    {
      const int j = nBlocks - 1 - i;
      for( int s = 0; s < 8; s++ ) if( ops.cost( j, s ) != cost[( size_t ) 8 * i + s] || ops.scored( j, s ) != ( ( ( blocks[i].modeMask >> s ) & 1 ) != 0 ) ) return 4;
      for( int c = 0; c < 2; c++ )
        for( int s = 0; s < 8; s++ )
          if( const vvhip::Pel* q = ops.pred( j, c, s ) )
          {
            const size_t n = ( size_t ) blocks[i].w * blocks[i].h;
            if( at + n > pred.size() || memcmp( q, pred.data() + at, n * sizeof( vvhip::Pel ) ) ) return 4;
            at += n;
          }
    }
    if( at != pred.size() ) return 4;
    flow += "the reversed list gives every block the same costs and predictions\n";
    dump( dir + "/flow.txt", flow.data(), flow.size() );
  }
  catch( const std::exception& e ) { fprintf( stderr, "exception: %s\n", e.what() ); return 1; }
  return 0;
}
