// mmvd_shim_driver.cpp — TEST INFRASTRUCTURE: runs vvhip::MergeMmvdOps (the shim's entry to vvhip_merge_mmvd_costs_batch) on a list of CUs read from a file
// (tests/test_gpu_mmvd_shim.py writes it from the case list, compiles this file against libvvenc_hip_shim.so and checks the outputs against the model), and its two pieces of
// host arithmetic without a device (tests/test_mmvd_cpu.py).
//   mmvd_shim_driver DIR   DIR/list.bin: int32 nCus, picWidth, picHeight, ctuSize, margin, stride, bitDepth, curPoc, disFrac, hadFast, nRef; nRef reference planes and the
//                          original, ( picHeight + 2 margin ) x stride samples each; per CU int32 cuX, cuY, width, height, maskLo, maskHi and per base int32 mvHor[2], mvVer[2],
//                          plane[2] ( -1: list unused ), refPoc[2], longTerm[2], bcwIdx, altHpel
//   -> DIR/cost.bin: per CU uint32 [64] (0 where a candidate was not scored); DIR/flow.txt: one line per step that went as it must
//   mmvd_shim_driver --walk IN OUT   (no device) IN: int32 n; per entry uint32 dist[64], double bitsCost[64], double listCost[8], uint64 skip, int32 nList, mmvd, mmvdDisNum,
//                          numValidMergeCand, mrgCnd0, mrgCnd1, maxTrackingNum, 0
//   -> OUT: per entry double bestCostOffset, bestCostMerge, int32 bestDir, count, uint8 tested[64]
//   mmvd_shim_driver --bdof IN OUT   (no device) IN: int32 n; per entry int32 width, height, curPoc, mmvd, bdofEnabled, bcwEnabled and per base int32 used[2], refPoc[2],
//                          longTerm[2], bcwIdx -> OUT: per entry uint64
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

struct WalkIn  { uint32_t dist[64]; double bitsCost[64]; double listCost[8]; uint64_t skip; int32_t nList, mmvd, disNum, numValid, mrgCnd0, mrgCnd1, maxTracking, pad; };
struct WalkOut { double bestCostOffset, bestCostMerge; int32_t bestDir, count; uint8_t tested[64]; };
static_assert( sizeof( WalkIn ) == 256 + 512 + 64 + 8 + 32 && sizeof( WalkOut ) == 88, "packed as the tests write and read them" );

static int walkOnly( const char* in, const char* out )
{
  const std::vector<char> tb = slurp( in );
  int32_t n; memcpy( &n, tb.data(), 4 );
  if( tb.size() != 4 + ( size_t ) n * sizeof( WalkIn ) ) return 2;
  std::vector<WalkOut> res( n );
  for( int i = 0; i < n; i++ )
  {
    WalkIn w; memcpy( &w, tb.data() + 4 + ( size_t ) i * sizeof( WalkIn ), sizeof( WalkIn ) );
    vvhip::MergeMmvdOps::WalkCfg cfg;
    cfg.mmvd = w.mmvd; cfg.mmvdDisNum = w.disNum; cfg.numValidMergeCand = w.numValid; cfg.mrgCnd0 = w.mrgCnd0; cfg.mrgCnd1 = w.mrgCnd1; cfg.maxTrackingNum = w.maxTracking; cfg.skip = w.skip;
    WalkOut& o = res[i];
    memset( &o, 0, sizeof( o ) ); memset( o.tested, 0xff, 64 );
    o.count = vvhip::MergeMmvdOps::walk( w.dist, w.bitsCost, w.listCost, w.nList, cfg, o.tested, &o.bestCostOffset, &o.bestCostMerge, &o.bestDir );
  }
  dump( out, res.data(), res.size() );
  return 0;
}

static int bdofOnly( const char* in, const char* out )
{
  const std::vector<char> tb = slurp( in );
  int32_t n; memcpy( &n, tb.data(), 4 );
  if( tb.size() != 4 + ( size_t ) n * 20 * 4 ) return 2;
  static const vvhip::Pel some = 0;
  std::vector<uint64_t> res( n );
  for( int i = 0; i < n; i++ )
  {
    int32_t g[20]; memcpy( g, tb.data() + 4 + ( size_t ) i * 80, 80 );
    vvhip::MergeMmvdOps::Base base[2];
    for( int b = 0; b < 2; b++ )
      for( int l = 0; l < 2; l++ )
      {
        const int32_t* q = g + 6 + 7 * b;
        base[b].refPlane[l] = q[l] ? &some : nullptr; base[b].refPoc[l] = q[2 + l]; base[b].longTerm[l] = q[4 + l] != 0; base[b].bcwIdx = q[6];
      }
    res[i] = vvhip::MergeMmvdOps::bdofCands( g[0], g[1], base, g[2], g[3], g[4] != 0, g[5] != 0 );
  }
  dump( out, res.data(), res.size() );
  return 0;
}

struct Cu { int32_t x, y, w, h; uint32_t maskLo, maskHi; int32_t base[2][12]; };

int main( int argc, char** argv )
{
  if( argc == 4 && !strcmp( argv[1], "--walk" ) ) return walkOnly( argv[2], argv[3] );
  if( argc == 4 && !strcmp( argv[1], "--bdof" ) ) return bdofOnly( argv[2], argv[3] );
  if( argc < 2 ) return 2;
  const std::string dir = argv[1];
  try
  {
    const std::vector<char> tb = slurp( dir + "/list.bin" );
    const char* p = tb.data();
    int32_t hd[11]; memcpy( hd, p, sizeof( hd ) ); p += sizeof( hd );
    const int nCus = hd[0], picW = hd[1], picH = hd[2], ctu = hd[3], margin = hd[4], stride = hd[5], bitDepth = hd[6], curPoc = hd[7], disFrac = hd[8], hadFast = hd[9], nRef = hd[10];
    const size_t planeElems = ( size_t ) ( picH + 2 * margin ) * stride;
    if( nRef < 1 || nRef > 16 || stride < picW + 2 * margin ) return 2;
    std::vector<const vvhip::Pel*> origin( nRef + 1 );
    for( int k = 0; k <= nRef; k++ ) { origin[k] = reinterpret_cast<const vvhip::Pel*>( p ) + ( size_t ) margin * stride + margin; p += planeElems * sizeof( vvhip::Pel ); }
    std::vector<Cu> cus( nCus );
    for( Cu& c : cus ) { memcpy( &c, p, sizeof( Cu ) ); p += sizeof( Cu ); }
    if( p != tb.data() + tb.size() ) return 2;
    vvhip::Device& dev = vvhip::Device::get();
    for( int k = 0; k <= nRef; k++ ) dev.registerPicture( origin[k], stride, picW, picH, margin );
    auto addOne = [&]( vvhip::MergeMmvdOps& ops, const Cu& c )
    {
      vvhip::MergeMmvdOps::Base base[2];
      for( int b = 0; b < 2; b++ )
      {
        const int32_t* q = c.base[b];
        for( int l = 0; l < 2; l++ )
        {
          base[b].mvHor[l] = q[l]; base[b].mvVer[l] = q[2 + l]; base[b].refPlane[l] = q[4 + l] >= 0 ? origin[q[4 + l]] : nullptr; base[b].refPoc[l] = q[6 + l]; base[b].longTerm[l] = q[8 + l] != 0;
        }
        base[b].bcwIdx = q[10]; base[b].altHpel = q[11] != 0;
      }
      return ops.add( c.x, c.y, c.w, c.h, base, ( uint64_t ) c.maskLo | ( uint64_t ) c.maskHi << 32 );
    };
    std::string flow;
    vvhip::MergeMmvdOps ops;
    const vvhip::Pel* org = origin[nRef];
    ops.begin( picW, picH, ctu, bitDepth, curPoc, disFrac != 0, hadFast != 0, org );
    if( ops.run() || ops.count() != 0 ) return 3;
    flow += "an empty list does not run\n";
    Cu bad = cus[0];
    bad = cus[0]; bad.w = 12;                      if( addOne( ops, bad ) >= 0 ) return 3;
    bad = cus[0]; bad.w = 4; bad.h = 4;            if( addOne( ops, bad ) >= 0 ) return 3;
    bad = cus[0]; bad.x = picW - bad.w + 4;        if( addOne( ops, bad ) >= 0 ) return 3;
    bad = cus[0]; bad.y = -4;                      if( addOne( ops, bad ) >= 0 ) return 3;
    bad = cus[0]; bad.base[0][10] = 5;             if( addOne( ops, bad ) >= 0 ) return 3;
    bad = cus[0]; bad.base[0][4] = bad.base[0][5] = -1; bad.maskLo = 1; if( addOne( ops, bad ) >= 0 ) return 3;
    bad = cus[0]; bad.base[0][0] = 1 << 17; bad.base[0][4] = 0; if( addOne( ops, bad ) >= 0 ) return 3;
    ops.begin( picW, picH, 48, bitDepth, curPoc, disFrac != 0, hadFast != 0, org );   if( addOne( ops, cus[0] ) >= 0 ) return 3;
    ops.begin( picW, picH, ctu, 13, curPoc, disFrac != 0, hadFast != 0, org );        if( addOne( ops, cus[0] ) >= 0 ) return 3;
    ops.begin( picW, picH, ctu, bitDepth, curPoc, disFrac != 0, hadFast != 0, nullptr ); if( addOne( ops, cus[0] ) >= 0 ) return 3;
    if( ops.count() != 0 ) return 3;
    flow += "a side of 12, 4 x 4, a CU outside the picture, bcwIdx 5, a requested base without lists, a vector outside the storage range, CTU 48, 13 bits and a missing original are refused\n";
    static const vvhip::Pel stray[16] = { 0 };
    ops.begin( picW, picH, ctu, bitDepth, curPoc, disFrac != 0, hadFast != 0, stray );
    if( addOne( ops, cus[0] ) < 0 || ops.run() ) return 3;
    flow += "an original that is not registered does not run\n";
    ops.begin( picW, picH, ctu, bitDepth, curPoc, disFrac != 0, hadFast != 0, org );
    for( const Cu& c : cus ) if( addOne( ops, c ) < 0 ) return 3;
    if( ops.count() != nCus || !ops.run() ) return 3;
    std::vector<uint32_t> cost;
    for( int i = 0; i < nCus; i++ ) cost.insert( cost.end(), ops.dists( i ), ops.dists( i ) + 64 );
    dump( dir + "/cost.bin", cost.data(), cost.size() );
    flow += "the list\n";
    // the list again in reverse order on the same object: a CU's results do not depend on its place
    ops.begin( picW, picH, ctu, bitDepth, curPoc, disFrac != 0, hadFast != 0, org );
    for( int i = nCus - 1; i >= 0; i-- ) if( addOne( ops, cus[i] ) < 0 ) return 3;
    if( !ops.run() ) return 3;
    for( int i = 0; i < nCus; i++ )
      for( int v = 0; v < 64; v++ )
      {
        const bool req = ( ( v < 32 ? cus[i].maskLo >> v : cus[i].maskHi >> ( v - 32 ) ) & 1 ) != 0;
        if( ops.dist( nCus - 1 - i, v ) != cost[( size_t ) 64 * i + v] || ops.scored( nCus - 1 - i, v ) != req ) return 4;
      }
    flow += "the reversed list gives every CU the same costs\n";
    dump( dir + "/flow.txt", flow.data(), flow.size() );
  }
  catch( const std::exception& e ) { fprintf( stderr, "exception: %s\n", e.what() ); return 1; }
  return 0;
}
