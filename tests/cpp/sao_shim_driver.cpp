// sao_shim_driver.cpp — TEST INFRASTRUCTURE: runs vvhip::SaoOps (the shim's entry to vvhip_sao_stats / vvhip_sao_offset) band by band on a 4:2:0 picture read from a file
// (tests/test_gpu_sao_shim.py writes it, compiles this file against libvvenc_hip_shim.so and checks the outputs against tests/golden/sao.npz).
//   sao_shim_driver DIR   DIR/pic.bin: int32 width, height, bitDepth, ctuSize, recStride[3], orgStride[3], dstStride[3], then the three deblocked planes (height x recStride
//                         samples each; chroma half size), the three original planes, then ctus x 3 vvhip_sao_param records
//   -> DIR/stats.bin (ctus x 3 x 320 int64), DIR/dst<c>.bin (height x dstStride samples, pre-filled with -7: what lies between the rows must come back untouched),
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
    const int width = hd[0], height = hd[1], bitDepth = hd[2], ctuSize = hd[3];
    const int* recStride = hd + 4; const int* orgStride = hd + 7; const int* dstStride = hd + 10;
    const vvhip::Pel* p = reinterpret_cast<const vvhip::Pel*>( hd + 13 );
    const vvhip::Pel* rec[3]; const vvhip::Pel* org[3];
    for( int c = 0; c < 3; c++ ) { rec[c] = p; p += ( size_t ) ( c ? height / 2 : height ) * recStride[c]; }
    for( int c = 0; c < 3; c++ ) { org[c] = p; p += ( size_t ) ( c ? height / 2 : height ) * orgStride[c]; }
    const int ctusX = ( width + ctuSize - 1 ) / ctuSize, rows = ( height + ctuSize - 1 ) / ctuSize;
    std::vector<vvhip_sao_param> params( ( size_t ) ctusX * rows * 3 );
    memcpy( params.data(), p, params.size() * sizeof( vvhip_sao_param ) );
    std::string flow;
    vvhip::SaoOps ops;
    const int64_t* out = nullptr;
    vvhip::Pel* none[3] = { nullptr, nullptr, nullptr };
    if( ops.statisticsEnd( &out ) || ops.statisticsBand( 0, rec, org ) || ops.offsetPicture( rec, params.data(), none, dstStride ) ) return 3;
    flow += "nothing before begin\n";
    if( !ops.statisticsBegin( recStride, orgStride, width, height, bitDepth, ctuSize ) || ops.statisticsBands() != rows ) return 3;
    if( ops.statisticsEnd( &out ) ) return 3;
    flow += "no end before a band\n";
    for( int r = rows - 1; r >= 0; r-- )      // last row first: bands may come in any order
    {
      if( !ops.statisticsBand( r, rec, org ) ) return 3;
      if( ops.statisticsBand( r, rec, org ) ) return 3;                 // each exactly once
      if( r > 0 && ops.statisticsEnd( &out ) ) return 3;                // not before every band was issued
    }
    if( ops.statisticsBand( rows, rec, org ) || ops.statisticsBand( -1, rec, org ) ) return 3;
    flow += "no end before every band, no band twice\n";
    if( !ops.statisticsEnd( &out ) || !out ) return 3;
    dump( dir + "/stats.bin", out, ( size_t ) ctusX * rows * 3 * VVHIP_SAO_REC );
    std::vector<vvhip::Pel> dst[3];
    vvhip::Pel* d[3];
    for( int c = 0; c < 3; c++ ) { dst[c].assign( ( size_t ) ( c ? height / 2 : height ) * dstStride[c], -7 ); d[c] = dst[c].data(); }
    if( !ops.offsetPicture( rec, params.data(), d, dstStride ) || !ops.residentPlane( 2 ) ) return 3;      // the planes the bands uploaded
    for( int c = 0; c < 3; c++ ) dump( dir + "/dst" + std::to_string( c ) + ".bin", dst[c].data(), dst[c].size() );
    // the same from planes that are not the resident ones (a copy elsewhere): uploaded, same result
    std::vector<vvhip::Pel> copy[3]; const vvhip::Pel* cp[3];
    std::vector<vvhip::Pel> dst2[3]; vvhip::Pel* d2[3];
    for( int c = 0; c < 3; c++ )
    {
      copy[c].assign( rec[c], rec[c] + ( size_t ) ( c ? height / 2 : height ) * recStride[c] ); cp[c] = copy[c].data();
      dst2[c].assign( dst[c].size(), -7 ); d2[c] = dst2[c].data();
    }
    if( !ops.offsetPicture( cp, params.data(), d2, dstStride ) ) return 3;
    for( int c = 0; c < 3; c++ ) if( dst2[c] != dst[c] ) return 4;
    flow += "resident and uploaded planes filter alike\n";
    dump( dir + "/flow.txt", flow.data(), flow.size() );
  }
  catch( const std::exception& e ) { fprintf( stderr, "exception: %s\n", e.what() ); return 1; }
  return 0;
}
