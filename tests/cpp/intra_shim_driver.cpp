// intra_shim_driver.cpp — TEST INFRASTRUCTURE: runs vvhip::IntraOps (the shim's entry to vvhip_intra_luma_modes_batch) on a list of blocks read from a file
// (tests/test_gpu_intra_shim.py writes it from the fixture's cases, compiles this file against libvvenc_hip_shim.so and checks the outputs against tests/golden/intra.npz).
//   intra_shim_driver DIR   DIR/list.bin: int32 nBlocks; per block int32 width, height, bitDepth, multiRefIdx, refStride, orgStride, numModes, numPred, then numModes + numPred
//                           int32 modes (intraDir, then predDir), the reference buffer ( refStride + 2 height + 1 + multiRefIdx samples: the top row at 0, the left row at
//                           refStride ), the original ( height x orgStride samples )
//   -> DIR/cost.bin: per block uint32 [67] (0 where a mode was not scored); DIR/pred.bin: per block the predictions of predDir in ascending mode order, compact
//      DIR/flow.txt: one line per step of the protocol that went as it must
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

struct Block { int w, h, bitDepth, mri, refStride, orgStride; std::vector<uint8_t> dir, predDir; const vvhip::Pel* ref; const vvhip::Pel* org; };

static int addAll( vvhip::IntraOps& ops, const std::vector<Block>& blocks )
{
  for( const Block& b : blocks )
    if( ops.add( b.ref, b.refStride, b.org, b.orgStride, b.w, b.h, b.bitDepth, b.mri, b.dir.data(), ( int ) b.dir.size(), b.predDir.data(), ( int ) b.predDir.size() ) < 0 ) return -1;
  return ops.count();
}

static void collect( const vvhip::IntraOps& ops, const std::vector<Block>& blocks, std::vector<uint32_t>& cost, std::vector<vvhip::Pel>& pred )
{
  cost.clear(); pred.clear();
  for( int i = 0; i < ops.count(); i++ )
  {
    for( int m = 0; m < 67; m++ ) cost.push_back( ops.cost( i, m ) );
    for( int m = 0; m < 67; m++ )
      if( const vvhip::Pel* p = ops.pred( i, m ) ) pred.insert( pred.end(), p, p + ( size_t ) blocks[i].w * blocks[i].h );
  }
}

int main( int argc, char** argv )
{
  if( argc < 2 ) return 2;
  const std::string dir = argv[1];
  try
  {
    const std::vector<char> tb = slurp( dir + "/list.bin" );
    const char* p = tb.data();
    int32_t nBlocks; memcpy( &nBlocks, p, 4 ); p += 4;
    std::vector<Block> blocks( nBlocks );
    for( Block& b : blocks )
    {
      int32_t g[8]; memcpy( g, p, sizeof( g ) ); p += sizeof( g );
      b.w = g[0]; b.h = g[1]; b.bitDepth = g[2]; b.mri = g[3]; b.refStride = g[4]; b.orgStride = g[5];
      std::vector<int32_t> m( g[6] + g[7] ); memcpy( m.data(), p, m.size() * 4 ); p += m.size() * 4;
      b.dir.assign( m.begin(), m.begin() + g[6] ); b.predDir.assign( m.begin() + g[6], m.end() );
      b.ref = reinterpret_cast<const vvhip::Pel*>( p ); p += ( size_t ) ( b.refStride + 2 * b.h + 1 + b.mri ) * sizeof( vvhip::Pel );
      b.org = reinterpret_cast<const vvhip::Pel*>( p ); p += ( size_t ) b.h * b.orgStride * sizeof( vvhip::Pel );
    }
    if( p != tb.data() + tb.size() ) return 2;
    std::string flow;
    vvhip::IntraOps ops;
    ops.begin();
    if( ops.run() || ops.count() != 0 ) return 3;
    flow += "an empty list does not run\n";
    const Block& b0 = blocks[0];
    const uint8_t planar[1] = { 0 }, beyond[1] = { 67 }, two[1] = { 2 }, three[1] = { 3 };
    if( ops.add( b0.ref, b0.refStride, b0.org, b0.orgStride, 12, b0.h, b0.bitDepth, 0, two, 1 ) >= 0 || ops.add( b0.ref, b0.refStride, b0.org, b0.orgStride, b0.w, b0.h, 13, 0, two, 1 ) >= 0 ||
        ops.add( b0.ref, b0.refStride, b0.org, b0.orgStride, b0.w, b0.h, b0.bitDepth, 3, two, 1 ) >= 0 || ops.add( b0.ref, 2 * b0.w, b0.org, b0.orgStride, b0.w, b0.h, b0.bitDepth, 0, two, 1 ) >= 0 ||
        ops.add( b0.ref, b0.refStride + 1, b0.org, b0.orgStride, b0.w, b0.h, b0.bitDepth, 1, planar, 1 ) >= 0 || ops.add( b0.ref, b0.refStride, b0.org, b0.orgStride, b0.w, b0.h, b0.bitDepth, 0, beyond, 1 ) >= 0 ||
        ops.add( b0.ref, b0.refStride, b0.org, b0.orgStride, b0.w, b0.h, b0.bitDepth, 0, two, 1, three, 1 ) >= 0 || ops.count() != 0 ) return 3;
    flow += "a side of 12, 13 bits, multiRefIdx 3, a short reference pitch, PLANAR with multiRefIdx 1, mode 67, an unscored predDir are refused\n";
    if( addAll( ops, blocks ) != nBlocks || !ops.run() ) return 3;
    std::vector<uint32_t> cost; std::vector<vvhip::Pel> pred;
    collect( ops, blocks, cost, pred );
    dump( dir + "/cost.bin", cost.data(), cost.size() );
    dump( dir + "/pred.bin", pred.data(), pred.size() );
    flow += "the list\n";
    // the list again in reverse order on the same object: a block's results do not depend on its place
    std::vector<Block> rev( blocks.rbegin(), blocks.rend() );
    ops.begin();
    if( addAll( ops, rev ) != nBlocks || !ops.run() ) return 3;
    for( int i = 0; i < nBlocks; i++ )
      for( int m = 0; m < 67; m++ )
      {
        const int j = nBlocks - 1 - i;
        if( ops.cost( j, m ) != cost[( size_t ) 67 * i + m ] || ops.scored( j, m ) != ( std::find( blocks[i].dir.begin(), blocks[i].dir.end(), ( uint8_t ) m ) != blocks[i].dir.end() ) ) return 4;
      }
    size_t at = 0;
    for( int i = 0; i < nBlocks; i++ )
      for( int m = 0; m < 67; m++ )
        if( const vvhip::Pel* q = ops.pred( nBlocks - 1 - i, m ) )
        {
          const size_t n = ( size_t ) blocks[i].w * blocks[i].h;
          if( at + n > pred.size() || memcmp( q, pred.data() + at, n * sizeof( vvhip::Pel ) ) ) return 4;
          at += n;
        }
    if( at != pred.size() ) return 4;
    flow += "the reversed list gives every block the same costs and predictions\n";
    dump( dir + "/flow.txt", flow.data(), flow.size() );
  }
  catch( const std::exception& e ) { fprintf( stderr, "exception: %s\n", e.what() ); return 1; }
  return 0;
}
