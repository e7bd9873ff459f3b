// visact_shim_driver.cpp — TEST INFRASTRUCTURE: runs vvhip::VisActOps (the shim's entry to vvhip_visact) on planes and an area list read from a file
// (tests/test_gpu_visact_shim.py writes it, compiles this file against libvvenc_hip_shim.so and checks the outputs against tests/golden/visact.npz).
//   visact_shim_driver DIR   DIR/pic.bin: int32 nPlanes, bitDepth, nAreas; per plane int32 width, height, stride[3] (cur, prev1, prev2), flags (1: prev1 present,
//                            2: prev2 present, 4: prev1 IS cur); per plane the planes present (height x stride samples: cur, prev1 unless it is cur, prev2); nAreas
//                            vvhip_visact_area records
//   -> DIR/out.bin: per area uint64 record[4]; double hpSpatAct, hpTempAct, hpVisAct; uint32 spatAct, tempAct, minAct, visAct; int64 getAvg (-1: none)
//      DIR/flow.txt: one line per step of the protocol that went as it must
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

struct Result { uint64_t rec[4]; double hp[3]; uint32_t ints[4]; int64_t avg; };

static std::vector<Result> collect( const vvhip::VisActOps& ops )
{
  std::vector<Result> out( ops.count() );
  for( int i = 0; i < ops.count(); i++ )
  {
    Result& o = out[i];
    memset( &o, 0, sizeof( o ) );
    memcpy( o.rec, ops.record( i ), sizeof( o.rec ) );
    const vvhip::VisAct va = ops.visAct( i );
    o.hp[0] = va.hpSpatAct; o.hp[1] = va.hpTempAct; o.hp[2] = va.hpVisAct;
    o.ints[0] = va.spatAct; o.ints[1] = va.tempAct; o.ints[2] = va.minAct; o.ints[3] = va.visAct;
    o.avg = ops.avg( i );
  }
  return out;
}

int main( int argc, char** argv )
{
  if( argc < 2 ) return 2;
  const std::string dir = argv[1];
  try
  {
    const std::vector<char> tb = slurp( dir + "/pic.bin" );
    const int32_t* hd = reinterpret_cast<const int32_t*>( tb.data() );
    const int nPlanes = hd[0], bitDepth = hd[1], nAreas = hd[2];
    int width[3], height[3], st[3][3], flags[3];
    for( int c = 0; c < nPlanes; c++ ) { const int32_t* g = hd + 3 + 6 * c; width[c] = g[0]; height[c] = g[1]; st[0][c] = g[2]; st[1][c] = g[3]; st[2][c] = g[4]; flags[c] = g[5]; }
    const vvhip::Pel* p = reinterpret_cast<const vvhip::Pel*>( hd + 3 + 6 * nPlanes );
    const vvhip::Pel* pl[3][3] = { { nullptr, nullptr, nullptr }, { nullptr, nullptr, nullptr }, { nullptr, nullptr, nullptr } };
    for( int c = 0; c < nPlanes; c++ )
    {
      pl[0][c] = p; p += ( size_t ) height[c] * st[0][c];
      if( flags[c] & 4 ) pl[1][c] = pl[0][c];
      else if( flags[c] & 1 ) { pl[1][c] = p; p += ( size_t ) height[c] * st[1][c]; }
      if( flags[c] & 2 ) { pl[2][c] = p; p += ( size_t ) height[c] * st[2][c]; }
    }
    std::vector<vvhip_visact_area> areas( nAreas );
    memcpy( areas.data(), p, areas.size() * sizeof( vvhip_visact_area ) );
    std::string flow;
    vvhip::VisActOps ops;
    if( ops.sums( areas.data(), nAreas ) || ops.count() != 0 ) return 3;
    flow += "no sums before a picture\n";
    int narrow[3] = { st[0][0], st[0][1], st[0][2] };
    narrow[0] = width[0] - 1;
    if( ops.picture( nPlanes, pl[0], pl[1], pl[2], narrow, st[1], st[2], width, height, bitDepth ) || ops.picture( 4, pl[0], pl[1], pl[2], st[0], st[1], st[2], width, height, bitDepth ) ||
        ops.picture( nPlanes, pl[0], pl[1], pl[2], st[0], st[1], st[2], width, height, 7 ) ) return 3;
    flow += "a pitch below the width, four planes, seven bits are refused\n";
    if( !ops.picture( nPlanes, pl[0], pl[1], pl[2], st[0], st[1], st[2], width, height, bitDepth ) || ops.sums( areas.data(), 0 ) ) return 3;
    if( !ops.sums( areas.data(), nAreas ) || ops.count() != nAreas ) return 3;
    const std::vector<Result> first = collect( ops );
    dump( dir + "/out.bin", first.data(), first.size() );
    flow += "a picture, then its list\n";
    // a second list on the same upload — the first area alone — and the first list again: the records do not depend on the rest of the list
    if( !ops.sums( areas.data(), 1 ) || ops.count() != 1 || memcmp( collect( ops ).data(), first.data(), sizeof( Result ) ) ) return 4;
    if( !ops.sums( areas.data(), nAreas ) ) return 3;
    const std::vector<Result> again = collect( ops );
    if( memcmp( again.data(), first.data(), first.size() * sizeof( Result ) ) ) return 4;
    flow += "further lists on the resident planes give the same records\n";
    dump( dir + "/flow.txt", flow.data(), flow.size() );
  }
  catch( const std::exception& e ) { fprintf( stderr, "exception: %s\n", e.what() ); return 1; }
  return 0;
}
