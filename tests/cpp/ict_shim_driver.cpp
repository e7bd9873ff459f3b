// ict_shim_driver.cpp — TEST INFRASTRUCTURE: runs vvhip::JointCbCrOps::codeList (the shim's entry to vvhip_ict_fwd_batch -> vvhip_tu_rdo_multi_strided -> vvhip_ict_inv_batch)
// on a list of chroma TUs read from a file (tests/test_gpu_ict_shim.py writes it, compiles this file against libvvenc_hip_shim.so and checks the outputs against
// tests/ict_ref.py around the oracle's TU pipeline).
//   ict_shim_driver DIR   DIR/tus.bin: int32 n, bitDepth, isIRAP, thrVal, nCand, then n + nCand x { int32 width, height, stride, mode, qp }, then per TU its Cb block and its
//                         Cr block, height x stride samples each.  The first n TUs are the chain's list, the last nCand a candidate list (any mode, distortions only).
//   -> DIR/dist.bin (n x 2 int64), DIR/levels.bin, DIR/rec_cb.bin, DIR/rec_cr.bin (compact, list order), DIR/stats.bin (n x vvhip_tu_stats), DIR/sse.bin (n x 2 uint64),
//      DIR/cand.bin (nCand x 2 int64), DIR/again.bin (the chain's SSEs once more, after the candidate list, with only that output requested)
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
template<class T> static void dump( const std::string& p, const std::vector<T>& v ) { FILE* f = fopen( p.c_str(), "wb" ); fwrite( v.data(), sizeof( T ), v.size(), f ); fclose( f ); }

int main( int argc, char** argv )
{
  if( argc < 2 ) return 2;
  const std::string dir = argv[1];
  try
  {
    const std::vector<char> tb = slurp( dir + "/tus.bin" );
    const int32_t* hd = reinterpret_cast<const int32_t*>( tb.data() );
    const int n = hd[0], bitDepth = hd[1], irap = hd[2], thrVal = hd[3], nCand = hd[4];
    const int32_t* rec = hd + 5;
    const vvhip::Pel* blk = reinterpret_cast<const vvhip::Pel*>( rec + 5 * ( n + nCand ) );
    std::vector<vvhip::JointCbCrOps::Tu> tus( n + nCand );
    size_t elems = 0;
    for( int i = 0; i < n + nCand; i++, rec += 5 )
    {
      vvhip::JointCbCrOps::Tu& t = tus[i];
      t.width = rec[0]; t.height = rec[1]; t.stride = rec[2]; t.mode = rec[3]; t.qp = rec[4];
      t.cb = blk; t.cr = blk + ( size_t ) t.height * t.stride; blk += 2 * ( size_t ) t.height * t.stride;
      if( i < n ) elems += ( size_t ) t.width * t.height;
    }
    std::vector<int64_t> dist( 2 * n, -1 ), cand( 2 * nCand, -1 );
    std::vector<uint64_t> sse( 2 * n, 7 ), again( 2 * n, 7 );
    std::vector<vvhip::Pel> levels( elems, -7 ), recCb( elems, -7 ), recCr( elems, -7 );
    std::vector<vvhip_tu_stats> stats( n );
    vvhip::JointCbCrOps ops;
    if( !ops.codeList( tus.data(), n, bitDepth, irap != 0, thrVal, dist.data(), levels.data(), recCb.data(), recCr.data(), stats.data(), sse.data() ) ) return 3;
    if( !ops.codeList( tus.data() + n, nCand, bitDepth, irap != 0, thrVal, cand.data() ) ) return 3;
    if( !ops.codeList( tus.data(), n, bitDepth, irap != 0, thrVal, nullptr, nullptr, nullptr, nullptr, nullptr, again.data() ) ) return 3;
    dump( dir + "/dist.bin", dist ); dump( dir + "/levels.bin", levels ); dump( dir + "/rec_cb.bin", recCb ); dump( dir + "/rec_cr.bin", recCr );
    dump( dir + "/stats.bin", stats ); dump( dir + "/sse.bin", sse ); dump( dir + "/cand.bin", cand ); dump( dir + "/again.bin", again );
  }
  catch( const std::exception& e ) { fprintf( stderr, "exception: %s\n", e.what() ); return 1; }
  return 0;
}
