// deblock_shim_driver.cpp — TEST INFRASTRUCTURE: runs vvhip::DeblockOps (the shim's entry to vvhip_deblock) band by band on a 4:2:0 picture read from a file
// (tests/test_gpu_deblock_shim.py writes it, compiles this file against libvvenc_hip_shim.so and checks the outputs against tests/golden/deblock.npz).
//   deblock_shim_driver DIR   DIR/pic.bin: int32 width, height, bitDepth, ctuSize, stride[3], dstStride[3], lfpStride, betaOffsetDiv2[3], tcOffsetDiv2[3], then the three
//                             unfiltered planes (height x stride samples each; chroma half size), then the vertical and the horizontal map (height / 4 rows of lfpStride
//                             vvhip_lf_param records each)
//   -> DIR/dst<c>.bin (height x dstStride samples, pre-filled with -7: what lies between the rows must come back untouched),
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

int main( int argc, char** argv )
{
  if( argc < 2 ) return 2;
  const std::string dir = argv[1];
  try
  {
    const std::vector<char> tb = slurp( dir + "/pic.bin" );
    const int32_t* hd = reinterpret_cast<const int32_t*>( tb.data() );
    const int width = hd[0], height = hd[1], bitDepth = hd[2], ctuSize = hd[3], lfpStride = hd[10];
    const int* stride = hd + 4; const int* dstStride = hd + 7; const int* beta = hd + 11; const int* tc = hd + 14;
    const vvhip::Pel* p = reinterpret_cast<const vvhip::Pel*>( hd + 17 );
    const vvhip::Pel* rec[3];
    for( int c = 0; c < 3; c++ ) { rec[c] = p; p += ( size_t ) ( c ? height / 2 : height ) * stride[c]; }
    std::vector<vvhip_lf_param> maps[2];
    for( int d = 0; d < 2; d++ )
    {
      maps[d].resize( ( size_t ) ( height / 4 ) * lfpStride );
      memcpy( maps[d].data(), reinterpret_cast<const char*>( p ) + d * maps[0].size() * sizeof( vvhip_lf_param ), maps[d].size() * sizeof( vvhip_lf_param ) );
    }
    const int rows = ( height + ctuSize - 1 ) / ctuSize;
    std::string flow;
    vvhip::DeblockOps ops;
    std::vector<vvhip::Pel> dst[3];
    vvhip::Pel* d[3];
    for( int c = 0; c < 3; c++ ) { dst[c].assign( ( size_t ) ( c ? height / 2 : height ) * dstStride[c], -7 ); d[c] = dst[c].data(); }
    if( ops.end( d, dstStride ) || ops.band( 0, rec, maps[0].data(), maps[1].data(), lfpStride ) || ops.residentPlane( 0 ) ) return 3;
    flow += "nothing before begin\n";
    const int odd[3] = { width + 4, width / 2, width / 2 };
    if( ops.begin( stride, width + 4, height, bitDepth, ctuSize, beta, tc ) || ops.begin( odd, width, height, bitDepth, 48, beta, tc ) ) return 3;
    if( !ops.begin( stride, width, height, bitDepth, ctuSize, beta, tc ) || ops.bands() != rows ) return 3;
    if( ops.end( d, dstStride ) ) return 3;
    flow += "no end before a band\n";
    if( rows > 1 && ops.band( 1, rec, maps[0].data(), maps[1].data(), lfpStride ) ) return 3;      // top to bottom only
    for( int r = 0; r < rows; r++ )
    {
      if( r > 0 && ops.band( r - 1, rec, maps[0].data(), maps[1].data(), lfpStride ) ) return 3;     // each exactly once
      if( !ops.band( r, rec, maps[0].data(), maps[1].data(), lfpStride ) ) return 3;
      if( r < rows - 1 && ops.end( d, dstStride ) ) return 3;                                       // not before every band was issued
    }
    if( ops.band( rows, rec, maps[0].data(), maps[1].data(), lfpStride ) ) return 3;
    flow += "bands top to bottom, each once, no end before the last\n";
    if( !ops.end( d, dstStride ) || !ops.residentPlane( 2 ) ) return 3;
    for( int c = 0; c < 3; c++ ) dump( dir + "/dst" + std::to_string( c ) + ".bin", dst[c].data(), dst[c].size() );
    // a second picture on the same object, nothing downloaded but one plane: the same result
    std::vector<vvhip::Pel> again( dst[1].size(), -7 );
    vvhip::Pel* only[3] = { nullptr, again.data(), nullptr };
    if( !ops.begin( stride, width, height, bitDepth, ctuSize, beta, tc ) ) return 3;
    for( int r = 0; r < rows; r++ ) if( !ops.band( r, rec, maps[0].data(), maps[1].data(), lfpStride ) ) return 3;
    if( !ops.end( only, dstStride ) || again != dst[1] ) return 4;
    flow += "a second picture on the same object filters alike\n";
    dump( dir + "/flow.txt", flow.data(), flow.size() );
  }
  catch( const std::exception& e ) { fprintf( stderr, "exception: %s\n", e.what() ); return 1; }
  return 0;
}
