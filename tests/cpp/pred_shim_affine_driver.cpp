// pred_shim_affine_driver.cpp — TEST INFRASTRUCTURE: runs vvhip::InterPredOps::predictAffineList on planes and a list of affine CU records read from files
// (tests/test_gpu_pred_shim_affine.py writes them, compiles this file against libvvenc_hip_shim.so and checks the outputs against tests/affine_ref.py).
//   pred_shim_affine_driver DIR bitDepth DIR/planes.bin: int32 count, then per plane int32 width, height, margin, stride + (height + 2 margin) x stride samples
//                                        DIR/items.bin:  int32 n, predElems, orgPlane (-1: none), refPlanes, picWidth, picHeight, ctuSize, 0, then n x vvhip_pred_affine_item
//   -> DIR/pred.bin, DIR/resi.bin (predElems samples each); exit 4 when a list that names an unregistered plane is accepted
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
    const int n = ih[0], predElems = ih[1], orgPlane = ih[2], refPlanes = ih[3], picW = ih[4], picH = ih[5], ctu = ih[6];
    const vvhip_pred_affine_item* items = reinterpret_cast<const vvhip_pred_affine_item*>( ih + 8 );
    std::vector<vvhip::Pel> pred( predElems, -7 ), resi( predElems, -7 );
    vvhip::InterPredOps ops;
    if( !ops.predictAffineList( origin.data(), refPlanes, items, n, picW, picH, ctu, bitDepth, pred.data(), predElems, orgPlane >= 0 ? origin[orgPlane] : nullptr, orgPlane >= 0 ? resi.data() : nullptr ) )
    { fprintf( stderr, "predictAffineList: a plane is not registered\n" ); return 3; }
    const vvhip::Pel* stranger = pred.data();
    if( ops.predictAffineList( &stranger, 1, items, n, picW, picH, ctu, bitDepth, pred.data(), predElems ) ) { fprintf( stderr, "predictAffineList accepted an unregistered plane\n" ); return 4; }
    dump( dir + "/pred.bin", pred ); dump( dir + "/resi.bin", resi );
  }
  catch( const std::exception& e ) { fprintf( stderr, "exception: %s\n", e.what() ); return 1; }
  return 0;
}
