// sbt_shim_driver.cpp — TEST INFRASTRUCTURE: runs vvhip::SbtOps::codeList (the shim's entry to vvhip_sbt_parts_batch -> vvhip_tu_rdo_multi_strided -> vvhip_sbt_place_batch)
// on a list of CUs and SBT candidates read from a file (tests/test_gpu_sbt_shim.py writes it, compiles this file against libvvenc_hip_shim.so and checks the outputs against
// the Python chain and tests/sbt_ref.py around the oracle's TU pipeline).
//   sbt_shim_driver DIR   DIR/cus.bin: int32 nCus, nCands, bitDepth, isIRAP, thrVal, double chromaWeight, then nCus x { int32 width, height, strideY, strideC, sbtAllowed },
//                         nCands x { int32 cu, mode, qpY, qpCb, qpCr }, then per CU its Y block (height x strideY samples), its Cb and its Cr block (height / 2 x strideC).
//   -> DIR/parts.bin (nCus x 48 uint64), DIR/est.bin (nCus x 9 uint64), DIR/order.bin (nCus x 8 bytes), DIR/levels.bin, DIR/rec.bin (compact, candidate order),
//      DIR/stats.bin (nCands x 3 vvhip_tu_stats), DIR/sse.bin (nCands x 3 uint64), DIR/again.bin (the SSEs once more, after a parts-only call, with only that output requested)
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
template<class T> static void dump( const std::string& p, const std::vector<T>& v ) { FILE* f = fopen( p.c_str(), "wb" ); fwrite( v.data(), sizeof( T ), v.size(), f ); fclose( f ); }

int main( int argc, char** argv )
{
  if( argc < 2 ) return 2;
  const std::string dir = argv[1];
  try
  {
    const std::vector<char> tb = slurp( dir + "/cus.bin" );
    const int32_t* hd = reinterpret_cast<const int32_t*>( tb.data() );
    const int nCus = hd[0], nCands = hd[1], bitDepth = hd[2], irap = hd[3], thrVal = hd[4];
    double chromaWeight; memcpy( &chromaWeight, hd + 5, 8 );
    const int32_t* rec = hd + 7;
    const vvhip::Pel* blk = reinterpret_cast<const vvhip::Pel*>( rec + 5 * ( nCus + nCands ) );
    std::vector<vvhip::SbtOps::Cu> cus( nCus );
    std::vector<vvhip::SbtOps::Cand> cands( nCands );
    for( int i = 0; i < nCus; i++, rec += 5 )
    {
      vvhip::SbtOps::Cu& c = cus[i];
      c.width = rec[0]; c.height = rec[1]; c.strideY = rec[2]; c.strideC = rec[3]; c.sbtAllowed = rec[4];
      c.y = blk; c.cb = c.y + ( size_t ) c.height * c.strideY; c.cr = c.cb + ( size_t ) ( c.height / 2 ) * c.strideC; blk = c.cr + ( size_t ) ( c.height / 2 ) * c.strideC;
    }
    size_t recElems = 0, levElems = 0;
    for( int k = 0; k < nCands; k++, rec += 5 )
    {
      vvhip::SbtOps::Cand& d = cands[k];
      d.cu = rec[0]; d.mode = rec[1]; d.qp[0] = rec[2]; d.qp[1] = rec[3]; d.qp[2] = rec[4];
      const size_t area = ( size_t ) cus[d.cu].width * cus[d.cu].height;
      recElems += area * 3 / 2; levElems += ( area * 3 / 2 ) / ( d.mode >= 4 ? 4 : 2 );
    }
    std::vector<uint64_t> parts( ( size_t ) nCus * 48, 7 ), est( ( size_t ) nCus * 9, 7 ), sse( ( size_t ) nCands * 3, 7 ), again( ( size_t ) nCands * 3, 7 ), est2( ( size_t ) nCus * 9, 7 );
    std::vector<uint8_t> order( ( size_t ) nCus * 8, 7 );
    std::vector<vvhip::Pel> levels( levElems, -7 ), recon( recElems, -7 );
    std::vector<vvhip_tu_stats> stats( ( size_t ) nCands * 3 );
    vvhip::SbtOps ops;
    if( !ops.codeList( cus.data(), nCus, cands.data(), nCands, chromaWeight, bitDepth, irap != 0, thrVal, parts.data(), est.data(), order.data(), levels.data(), recon.data(), stats.data(), sse.data() ) ) return 3;
    if( !ops.codeList( cus.data(), nCus, nullptr, 0, chromaWeight, bitDepth, irap != 0, thrVal, nullptr, est2.data(), nullptr ) || est2 != est ) return 3;
    if( !ops.codeList( cus.data(), nCus, cands.data(), nCands, chromaWeight, bitDepth, irap != 0, thrVal, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, again.data() ) ) return 3;
    dump( dir + "/parts.bin", parts ); dump( dir + "/est.bin", est ); dump( dir + "/order.bin", order ); dump( dir + "/levels.bin", levels ); dump( dir + "/rec.bin", recon );
    dump( dir + "/stats.bin", stats ); dump( dir + "/sse.bin", sse ); dump( dir + "/again.bin", again );
  }
  catch( const std::exception& e ) { fprintf( stderr, "exception: %s\n", e.what() ); return 1; }
  return 0;
}
