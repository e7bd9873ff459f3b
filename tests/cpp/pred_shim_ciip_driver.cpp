// pred_shim_ciip_driver.cpp — TEST INFRASTRUCTURE: runs vvhip::InterPredOps::predictList WITH CIIP records (planar intra part and weighting) on planes and a list read
// from files (tests/test_gpu_pred_shim_ciip.py writes them, compiles this file against libvvenc_hip_shim.so and checks the outputs against tests/ciip_ref.py).
//   pred_shim_ciip_driver DIR bitDepth  DIR/planes.bin: int32 count, then per plane int32 width, height, margin, stride + (height + 2 margin) x stride samples
//                                       DIR/items.bin:  int32 n, int32 predElems, int32 orgPlane (-1: none), int32 refPlanes, int32 lineElems, n x vvhip_pred_item,
//                                                       n x vvhip_pred_ext, n x vvhip_pred_blend, n x vvhip_pred_ciip, lineElems reference samples
//   -> DIR/pred.bin, DIR/resi.bin (predElems samples each), DIR/plain.bin (the same list with ciip = nullptr), DIR/again.bin (the list with its CIIP records once more)
#include <cstdio>
#include <cstdlib>
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
static void dump( const std::string& p, const std::vector<vvhip::Pel>& v ) { FILE* f = fopen( p.c_str(), "wb" ); fwrite( v.data(), sizeof( vvhip::Pel ), v.size(), f ); fclose( f ); }

int main( int argc, char** argv )
{
  if( argc < 3 ) return 2;
  const std::string dir = argv[1]; const int bitDepth = atoi( argv[2] );
  try
  {
    vvhip::Device& dev = vvhip::Device::get();
    const std::vector<char> pb = slurp( dir + "/planes.bin" ), ib = slurp( dir + "/items.bin" );
    const int32_t* ph = reinterpret_cast<const int32_t*>( pb.data() );
    const int count = *ph++;
    std::vector<const vvhip::Pel*> origin( count );
    for( int k = 0; k < count; k++ )
    {
      const int w = ph[0], h = ph[1], m = ph[2], stride = ph[3];
      const vvhip::Pel* base = reinterpret_cast<const vvhip::Pel*>( ph + 4 );
      origin[k] = base + ( size_t ) m * stride + m;
      dev.registerPicture( origin[k], stride, w, h, m );
      ph = reinterpret_cast<const int32_t*>( base + ( size_t ) ( h + 2 * m ) * stride );
    }
    const int32_t* ih = reinterpret_cast<const int32_t*>( ib.data() );
    const int n = ih[0], predElems = ih[1], orgPlane = ih[2], refPlanes = ih[3], lineElems = ih[4];
    const vvhip_pred_item* items = reinterpret_cast<const vvhip_pred_item*>( ih + 5 + 1 );      // (one int32 of padding keeps the records 8-byte aligned)
    const vvhip_pred_ext* ext = reinterpret_cast<const vvhip_pred_ext*>( items + n );
    const vvhip_pred_blend* blend = reinterpret_cast<const vvhip_pred_blend*>( ext + n );
    const vvhip_pred_ciip* ciip = reinterpret_cast<const vvhip_pred_ciip*>( blend + n + ( n & 1 ) );      // (likewise after an odd number of 4-byte blend records)
    const vvhip::Pel* lines = reinterpret_cast<const vvhip::Pel*>( ciip + n );
    std::vector<vvhip::Pel> pred( predElems, -7 ), resi( predElems, -7 ), plain( predElems, -7 ), again( predElems, -7 );
    vvhip::InterPredOps ops;
    const vvhip::Pel* org = orgPlane >= 0 ? origin[orgPlane] : nullptr;
    if( !ops.predictList( origin.data(), refPlanes, items, n, bitDepth, pred.data(), predElems, org, org ? resi.data() : nullptr, ext, blend, ciip, lines, lineElems ) )
    { fprintf( stderr, "predictList: a plane is not registered\n" ); return 3; }
    if( !ops.predictList( origin.data(), refPlanes, items, n, bitDepth, plain.data(), predElems, nullptr, nullptr, ext, blend ) ) return 3;
    if( !ops.predictList( origin.data(), refPlanes, items, n, bitDepth, again.data(), predElems, nullptr, nullptr, ext, blend, ciip, lines, lineElems ) ) return 3;
    dump( dir + "/pred.bin", pred ); dump( dir + "/resi.bin", resi ); dump( dir + "/plain.bin", plain ); dump( dir + "/again.bin", again );
  }
  catch( const std::exception& e ) { fprintf( stderr, "exception: %s\n", e.what() ); return 1; }
  return 0;
}
