// mmvd_golden_gen.cpp — records what the reference encoder's own functions compute for the MMVD merge candidates of a CU, for tests/golden/mmvd.npz
// (driver: tests/mmvd_golden_gen.py).
//
// Not part of build() and of no Makefile: compiled and linked by hand against the reference library where its sources and oracle/_ref/libvvenc_core.a
// (made by `make -C oracle/ref core`) exist.  With R = the reference checkout and O = oracle/_ref:
//
//   g++ -std=c++14 -O2 -pthread -w -DTARGET_SIMD_X86=1 -DVVENC_SOURCE -DNDEBUG -I$O/gen -I$R/include -I$R/source/Lib/vvenc -I$R/source/Lib
//       -I$R/source/Lib/CommonLib -I$R/source/Lib/CommonLib/x86 -isystem $R/thirdparty tests/mmvd_golden_gen.cpp
//       -Wl,--whole-archive $O/libvvenc_core.a -Wl,--no-whole-archive -o <somewhere outside the repository>/mmvd_golden_gen
//
// Private members ( InterPredInterpolation::m_if, RdCost::m_afpDistortFunc, EncCu::xCheckMMVDCand, EncCu::m_mergeItemList ) are reached by compiling the classes' headers with
// `private` and `protected` spelled `public`, after every standard header they use has been included as it is.
//
// Candidates ( mmvd_golden_gen IN OUT ).  The set-up is the least the functions read: default-constructed SPS ( BDOF and BCW on ) / PPS / PicHeader / Slice ( a B slice ),
// PreCalcValues from them, a CodingStructure that points at them, per base vector and list one reference Picture whose reconstruction buffer is filled from the case's plane,
// with its POC ( in Picture::poc and in the slice's refPOCList at reference index = base index ) and isLongTerm, a MergeCtx with the case's mmvdBaseMv / interDirNeighbours /
// BcwIdx / mmvdUseAltHpelIf, a CodingUnit of the case's area.  Per candidate of a base that uses a list: MergeCtx::setMmvdMergeCandiInfo( cu, idx ), clipMv on a copy of each
// vector as xPredInterUni applies it; per REQUESTED candidate then InterPrediction::motionCompensation( cu, pred, REF_PIC_LIST_X ) with cu.mcControl = 2 | 1 and the DistParam
// functions RdCost::setDistParam chooses for DF_HAD and DF_HAD_fast, original against prediction.
// Everything runs twice: the scalar row ( read_x86_extension_flags( SCALAR ) before InterPrediction::init, RdCost::create( false ), the default PelBufferOps ) and the x86 row
// ( the machine's level, RdCost::create( true ), g_pelBufOP.initPelBufOpsX86() ).  The program fails unless the x86 row's function pointers differ from the scalar ones, and
// fails when the two rows differ in a vector, a prediction sample or a cost.
// ( Above 10 bits RdCost::setDistParam takes m_afpDistortFunc[1], which initRdCostX86 leaves at the scalar functions: the 12-bit costs are the same function on both rows. )
//
// input  : int32 nSets, nCases; per plane set int32 picW, picH, margin, nRef, then nRef reference planes and the original, ( picH + 2 margin ) x ( picW + 2 margin ) int16 each;
//          per case int32 set, bitDepth, ctu, disFrac, cuX, cuY, w, h, maskLo, maskHi, then per base: mv[2][2], plane[2] ( -1: list unused ), pocDelta[2], longTerm[2], bcw, alt
// output : per case, per base that uses a list, per candidate 0..31 of the base: int32 cu.mv[0] ( hor, ver ), cu.mv[1], refIdx[0], refIdx[1], interDir, BcwIdx, imv,
//          clipped mv[0] ( hor, ver ), clipped mv[1]   ( 13 int32 ); for a requested candidate then int32 bdofOrDmvr ( motionCompensation's return value ), uint32 HAD cost,
//          uint32 HAD_fast cost and the h x w prediction, int16
// Timing ( mmvd_golden_gen --time IN REPS ): the x86 row's setMmvdMergeCandiInfo + motionCompensation + one DistParam function ( DF_HAD_fast ) over every requested candidate of
//          the input, on one core; prints the number of candidates and the best of REPS passes in seconds (a context figure).
// Walk   ( mmvd_golden_gen --walk IN OUT ): the loop of EncCu::addMmvdCandsToPruningList (EncCu.cpp:2361-2447) without its prediction, around EncCu::xCheckMMVDCand ITSELF and the
//          reference's own MergeItemList — records as tests/cpp/mmvd_shim_driver.cpp --walk reads and writes them ( maxTrackingNum 0 is run as 64 + nList: a list that never fills ).
#include <cmath>
#include <cstdio>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>
#include <array>
#include <map>
#include <list>
#include <string>
#include <sstream>
#include <iostream>
#include <algorithm>
#include <functional>
#include <memory>
#include <mutex>
#include <atomic>
#include <thread>
#include <condition_variable>
#include <unordered_map>
#include <deque>
#include <set>
#include <chrono>
#include <bitset>
#include <fstream>
#include <iomanip>
#include <queue>
#include <stack>
#include <random>
#include <numeric>
#include <cassert>
#include <cstdarg>
#include <climits>
#include <cinttypes>
#include <exception>
#include <utility>
#include <type_traits>
#include <iterator>
#include <tuple>
#include <future>
#define private public
#define protected public
#include "CommonLib/CommonDef.h"
#include "CommonLib/Unit.h"
#include "CommonLib/Buffer.h"
#include "CommonLib/Picture.h"
#include "CommonLib/Slice.h"
#include "CommonLib/CodingStructure.h"
#include "CommonLib/ContextModelling.h"
#include "CommonLib/UnitTools.h"
#include "CommonLib/RdCost.h"
#include "CommonLib/InterPrediction.h"
#include "CommonLib/x86/CommonDefX86.h"
#include "EncoderLib/EncCu.h"

using namespace vvenc;

struct Set { int picW, picH, margin, nRef; std::vector<std::vector<int16_t>> planes; };
struct Case { int32_t hd[10]; int32_t bs[2][12]; };
struct Row { InterPrediction* ip; RdCost* rc; };

static bool readAll( FILE* fi, std::vector<Set>& sets, std::vector<Case>& cases )
{
  int32_t n[2];
  if( fread( n, 4, 2, fi ) != 2 ) return false;
  sets.resize( n[0] ); cases.resize( n[1] );
  for( Set& s : sets )
  {
    int32_t g[4];
    if( fread( g, 4, 4, fi ) != 4 ) return false;
    s.picW = g[0]; s.picH = g[1]; s.margin = g[2]; s.nRef = g[3];
    s.planes.resize( s.nRef + 1 );
    for( auto& p : s.planes )
    {
      p.resize( ( size_t ) ( s.picW + 2 * s.margin ) * ( s.picH + 2 * s.margin ) );
      if( fread( p.data(), 2, p.size(), fi ) != p.size() ) return false;
    }
  }
  for( Case& c : cases ) if( fread( c.hd, 4, 10, fi ) != 10 || fread( c.bs, 4, 24, fi ) != 24 ) return false;
  return true;
}

// one reference Picture per ( base, list ) — each has its own POC and isLongTerm —; its reconstruction buffer VIEWS the storage of the plane behind it, which is created
// with the picture margin and filled once per plane
struct RefPic { Picture pic; };

static void fill( RefPic& r, const Set& s, int plane, CodingStructure* cs )
{
  static std::map<const int16_t*, PelStorage*> made;
  const int16_t* src = s.planes[plane].data();
  PelStorage*& st = made[src];
  if( !st )
  {
    st = new PelStorage;
    st->create( CHROMA_420, Area( 0, 0, s.picW, s.picH ), 128, s.margin, MEMORY_ALIGN_DEF_SIZE );
    PelBuf buf = st->bufs[COMP_Y];
    const int m = s.margin, w = s.picW + 2 * m, h = s.picH + 2 * m;
    for( int y = 0; y < h; y++ ) for( int x = 0; x < w; x++ ) buf.buf[( y - m ) * ( ptrdiff_t ) buf.stride + ( x - m )] = ( Pel ) src[( size_t ) y * w + x];
  }
  r.pic.cs = cs;
  PelStorage& view = r.pic.m_picBufs[PIC_RECONSTRUCTION];      // (never created itself: it owns nothing and frees nothing)
  view.chromaFormat = st->chromaFormat;
  view.bufs = st->bufs;
}

// one pass over the cases on one row.  out ( may be NULL ) receives the records; -> the number of requested candidates
static size_t pass( Row& row, const std::vector<Set>& sets, const std::vector<Case>& cases, RefPic ( *pics )[2], std::vector<char>* out, bool timeOnly )
{
  size_t nReq = 0;
  auto put = [out]( const void* p, size_t n ) { if( out ) out->insert( out->end(), ( const char* ) p, ( const char* ) p + n ); };
  for( const Case& cs_ : cases )
  {
    const int32_t* hd = cs_.hd;
    const Set& set = sets[hd[0]];
    const int bd = hd[1], ctu = hd[2], w = hd[6], h = hd[7];
    SPS sps; PPS pps; PicHeader ph; Slice slice;
    sps.chromaFormatIdc = CHROMA_420; sps.CTUSize = ctu; sps.BDOF = true; sps.BCW = true; sps.bitDepths.recon[CH_L] = sps.bitDepths.recon[CH_C] = bd;
    pps.picWidthInLumaSamples = set.picW; pps.picHeightInLumaSamples = set.picH; pps.weightedBiPred = false; pps.weightPred = false;
    ph.disFracMMVD = hd[3] != 0; ph.disBdofFlag = false;
    const unsigned maxQt[3] = { ( unsigned ) ctu, ( unsigned ) ctu, ( unsigned ) ctu };
    PreCalcValues pcv( sps, pps, maxQt );
    XUCache cache;
    CodingStructure cs( cache, nullptr );
    cs.sps = &sps; cs.pps = &pps; cs.picHeader = &ph; cs.pcv = &pcv; cs.slice = &slice;
    slice.picHeader = &ph; slice.poc = 0; slice.sps = &sps; slice.pps = &pps; slice.sliceType = VVENC_B_SLICE; slice.clpRngs.bd = bd;
    slice.numRefIdx[0] = slice.numRefIdx[1] = 2;
    MergeCtx ctx;
    for( int b = 0; b < 2; b++ )
    {
      const int32_t* q = cs_.bs[b];
      for( int l = 0; l < 2; l++ )
      {
        const bool used = q[4 + l] >= 0;
        ctx.mmvdBaseMv[b][l].mv = Mv( q[2 * l], q[2 * l + 1] );
        ctx.mmvdBaseMv[b][l].refIdx = used ? b : -1;
        slice.refPOCList[l][b] = q[6 + l];
        fill( pics[b][l], set, used ? q[4 + l] : 0, &cs );
        pics[b][l].pic.poc = q[6 + l];
        pics[b][l].pic.isLongTerm = q[8 + l] != 0;
        slice.refPicList[l][b] = &pics[b][l].pic;
      }
      ctx.interDirNeighbours[b] = ( q[4] >= 0 ? 1 : 0 ) | ( q[5] >= 0 ? 2 : 0 );
      ctx.BcwIdx[b] = ( uint8_t ) q[10];
      ctx.mmvdUseAltHpelIf[b] = q[11] != 0;
    }
    // the original block, compact
    std::vector<Pel> org( ( size_t ) w * h );
    {
      const std::vector<int16_t>& op = set.planes[set.nRef];
      const int pw = set.picW + 2 * set.margin;
      for( int y = 0; y < h; y++ ) for( int x = 0; x < w; x++ ) org[( size_t ) y * w + x] = op[( size_t ) ( set.margin + hd[5] + y ) * pw + set.margin + hd[4] + x];
    }
    PelStorage dst;
    dst.create( CHROMA_420, Area( 0, 0, w, h ) );
    const CPelBuf orgBuf( org.data(), w, w, h );
    DistParam dp[2] = { row.rc->setDistParam( orgBuf, orgBuf, bd, DF_HAD ), row.rc->setDistParam( orgBuf, orgBuf, bd, DF_HAD_fast ) };
    for( int b = 0; b < 2; b++ )
    {
      if( cs_.bs[b][4] < 0 && cs_.bs[b][5] < 0 ) continue;
      const uint32_t mask = ( uint32_t ) hd[8 + b];
      for( int k = 0; k < 32; k++ )
      {
        const bool req = ( mask >> k ) & 1;
        if( timeOnly && !req ) continue;
        CodingUnit cu( CHROMA_420, Area( hd[4], hd[5], w, h ) );
        cu.cs = &cs; cu.slice = &slice; cu.predMode = MODE_INTER; cu.chType = CH_L;
        MmvdIdx idx; idx.val = ( uint8_t ) ( 32 * b + k );
        ctx.setMmvdMergeCandiInfo( cu, idx );
        if( !timeOnly )
        {
          int32_t rec[13] = { cu.mv[0][0].hor, cu.mv[0][0].ver, cu.mv[1][0].hor, cu.mv[1][0].ver, cu.refIdx[0], cu.refIdx[1], cu.interDir, cu.BcwIdx, cu.imv, 0, 0, 0, 0 };
          for( int l = 0; l < 2; l++ )
          {
            Mv mv = cu.mv[l][0];
            clipMv( mv, cu.lumaPos(), cu.lumaSize(), pcv );
            rec[9 + 2 * l] = mv.hor; rec[10 + 2 * l] = mv.ver;
          }
          put( rec, sizeof( rec ) );
        }
        if( !req ) continue;
        nReq++;
        cu.mcControl = 2 | 1; cu.mvRefine = false;
        PelUnitBuf ub = dst;
        dst.bufs[COMP_Y].fill( -1 );
        const bool refined = row.ip->motionCompensation( cu, ub, REF_PIC_LIST_X );
        uint32_t cost[2];
        for( int f = 0; f < ( timeOnly ? 1 : 2 ); f++ )
        {
          DistParam& d = dp[timeOnly ? 1 : f];
          d.cur = dst.bufs[COMP_Y];
          cost[f] = ( uint32_t ) d.distFunc( d );
        }
        if( !timeOnly )
        {
          const int32_t r = refined ? 1 : 0;
          put( &r, 4 ); put( cost, 8 );
          const PelBuf& pb = dst.bufs[COMP_Y];
          for( int y = 0; y < h; y++ ) put( pb.buf + ( ptrdiff_t ) y * pb.stride, 2 * ( size_t ) w );
        }
      }
    }
    dst.destroy();
  }
  return nReq;
}

struct WalkIn  { uint32_t dist[64]; double bitsCost[64]; double listCost[8]; uint64_t skip; int32_t nList, mmvd, disNum, numValid, mrgCnd0, mrgCnd1, maxTracking, pad; };
struct WalkOut { double bestCostOffset, bestCostMerge; int32_t bestDir, count; uint8_t tested[64]; };

static int walkTraces( const char* in, const char* out )
{
  FILE* fi = fopen( in, "rb" ); FILE* fo = fopen( out, "wb" );
  int32_t n;
  if( !fi || !fo || fread( &n, 4, 1, fi ) != 1 ) return 2;
  EncCu* ec = new EncCu;                                              // (never initialised further and never destroyed: xCheckMMVDCand reads m_pcEncCfg->m_MMVD alone)
  VVEncCfg cfg; memset( &cfg, 0, sizeof( cfg ) );
  ec->m_pcEncCfg = &cfg;
  const int maxSize = 80;
  ec->m_mergeItemList.init( maxSize, 1, CHROMA_400, 8, 8 );
  for( int i = 0; i < n; i++ )
  {
    WalkIn w;
    if( fread( &w, sizeof( w ), 1, fi ) != 1 ) return 2;
    cfg.m_MMVD = w.mmvd; cfg.m_MmvdDisNum = w.disNum;
    MergeItemList& list = ec->m_mergeItemList;
    list.resetList( w.maxTracking > 0 ? w.maxTracking : 64 + w.nList );
    const int mrg[2] = { w.mrgCnd0, w.mrgCnd1 };
    for( int k = 0; k < w.nList; k++ ) { MergeItem* p = list.allocateNewMergeItem(); p->cost = w.listCost[k]; p->mergeIdx = k < 2 ? mrg[k] : 2 + k; list.insertMergeItemToList( p ); }
    if( ( int ) list.size() != w.nList ) return 4;
    // EncCu.cpp:2361-2447 around the reference's own xCheckMMVDCand, its prediction replaced by the ready cost
    WalkOut o; memset( &o, 0, sizeof( o ) ); memset( o.tested, 0xff, 64 );
    int    mmvdTestNum    = w.numValid > 1 ? MmvdIdx::ADD_NUM : MmvdIdx::ADD_NUM >> 1;
    int    bestDir        = 0;
    size_t curListSize    = list.size();
    double bestCostMerge  = list.getMergeItemInList( curListSize - 1 )->cost;
    double bestCostOffset = MAX_DOUBLE;
    int    shiftCandStart = 0;
    if( cfg.m_MMVD == 4 )
    {
      const int cnd1idx = list.size() == 1 ? 0 : 1;
      const int mrgCnd0 = list.getMergeItemInList( 0 )->mergeIdx, mrgCnd1 = list.getMergeItemInList( cnd1idx )->mergeIdx;
      if( mrgCnd0 > 1 && mrgCnd1 > 1 ) mmvdTestNum = 0;
      else if( mrgCnd0 > 1 || mrgCnd1 > 1 )
      {
        const int shiftCand = mrgCnd0 < 2 ? mrgCnd0 : mrgCnd1;
        if( shiftCand ) shiftCandStart = MMVD_MAX_REFINE_NUM; else mmvdTestNum = MMVD_MAX_REFINE_NUM;
      }
    }
    for( int mmvdMergeCand = shiftCandStart; mmvdMergeCand < mmvdTestNum; mmvdMergeCand++ )
    {
      MmvdIdx mmvdIdx; mmvdIdx.val = mmvdMergeCand;
      if( mmvdIdx.pos.step >= cfg.m_MmvdDisNum ) continue;
      if( cfg.m_MMVD > 1 )
      {
        const int checkMMVD = ec->xCheckMMVDCand( mmvdIdx, bestDir, mmvdTestNum, bestCostOffset, bestCostMerge, list.getMergeItemInList( curListSize - 1 )->cost );
        mmvdMergeCand = mmvdIdx.val;
        if( checkMMVD ) { if( checkMMVD == 2 ) break; continue; }
      }
      if( ( w.skip >> mmvdIdx.val ) & 1 ) continue;
      MergeItem* p = list.allocateNewMergeItem();
      p->cost = ( double ) w.dist[mmvdIdx.val] + w.bitsCost[mmvdIdx.val];
      p->mergeIdx = mmvdIdx.val;
      const double cost = p->cost;
      o.tested[o.count++] = mmvdIdx.val;
      list.insertMergeItemToList( p );
      if( cfg.m_MMVD > 1 && cost < bestCostOffset )
      {
        bestCostOffset = cost;
        const int candCur = mmvdIdx.val - MMVD_MAX_REFINE_NUM * mmvdIdx.pos.baseIdx;
        if( candCur < 4 ) bestDir = candCur;
      }
    }
    o.bestCostOffset = bestCostOffset; o.bestCostMerge = bestCostMerge; o.bestDir = bestDir;
    fwrite( &o, sizeof( o ), 1, fo );
  }
  fclose( fi ); fclose( fo );
  return 0;
}

int main( int argc, char** argv )
{
  if( argc == 4 && !strcmp( argv[1], "--walk" ) ) return walkTraces( argv[2], argv[3] );
  const bool timing = argc == 4 && !strcmp( argv[1], "--time" );
  if( argc != 3 && !timing ) { fprintf( stderr, "usage: %s in out | --time in reps | --walk in out\n", argv[0] ); return 2; }
  FILE* fi = fopen( timing ? argv[2] : argv[1], "rb" );
  if( !fi ) return 2;
  std::vector<Set> sets; std::vector<Case> cases;
  if( !readAll( fi, sets, cases ) ) return 2;
  fclose( fi );

  const X86_VEXT best = read_x86_extension_flags();
  const PelBufferOps scalarOps = g_pelBufOP;
  Row rows[2];
  for( int r = 0; r < 2; r++ )
  {
    read_x86_extension_flags( r ? best : x86_simd::SCALAR );
    rows[r].rc = new RdCost; rows[r].rc->create( r != 0 );
    rows[r].ip = new InterPrediction; rows[r].ip->init( rows[r].rc, CHROMA_420, 128 );
  }
  PelBufferOps x86Ops = scalarOps;
  x86Ops.initPelBufOpsX86();
  {
    const InterpolationFilter &a = rows[0].ip->m_if, &x = rows[1].ip->m_if;
    if( a.m_filterHor[0][0][0] == x.m_filterHor[0][0][0] || a.m_filterVer[0][1][1] == x.m_filterVer[0][1][1] || a.m_filter8xH[0][0] == x.m_filter8xH[0][0] || a.m_filter16xH[0][1] == x.m_filter16xH[0][1] ||
        a.m_filterCopy[0][0] == x.m_filterCopy[0][0] || rows[0].rc->m_afpDistortFunc[0][DF_HAD8] == rows[1].rc->m_afpDistortFunc[0][DF_HAD8] ||
        rows[0].rc->m_afpDistortFunc[0][DF_HAD16_fast] == rows[1].rc->m_afpDistortFunc[0][DF_HAD16_fast] || scalarOps.addAvg == x86Ops.addAvg || scalarOps.wghtAvg8 == x86Ops.wghtAvg8 || scalarOps.addAvg16 == x86Ops.addAvg16 )
    { fprintf( stderr, "this build has no x86 row\n" ); return 3; }
  }
  static RefPic pics[2][2];
  if( timing )
  {
    g_pelBufOP = x86Ops;
    double bestT = 1e30; size_t n = 0;
    for( int r = 0; r < atoi( argv[3] ); r++ )
    {
      const auto t0 = std::chrono::steady_clock::now();
      n = pass( rows[1], sets, cases, pics, nullptr, true );
      bestT = std::min( bestT, std::chrono::duration<double>( std::chrono::steady_clock::now() - t0 ).count() );
    }
    printf( "%zu %.6f\n", n, bestT );
    return 0;
  }
  std::vector<char> out[2];
  for( int r = 0; r < 2; r++ )
  {
    g_pelBufOP = r ? x86Ops : scalarOps;
    pass( rows[r], sets, cases, pics, &out[r], false );
  }
  if( out[0] != out[1] ) { fprintf( stderr, "the scalar and the x86 row differ\n" ); return 4; }
  FILE* fo = fopen( argv[2], "wb" );
  if( !fo || fwrite( out[0].data(), 1, out[0].size(), fo ) != out[0].size() ) return 2;
  fclose( fo );
  return 0;
}
