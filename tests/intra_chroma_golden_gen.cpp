// intra_chroma_golden_gen.cpp — records what the reference encoder's own chroma intra prediction (regular modes, CCLM, MDLM) and its SAD / HAD costs compute, for
// tests/golden/intra_chroma.npz (driver: tests/intra_chroma_golden_gen.py).
//
// Not part of build() and of no Makefile: compiled and linked by hand against the reference library where its sources and oracle/_ref/libvvenc_core.a
// (made by `make -C oracle/ref core`) exist.  With R = the reference checkout and O = oracle/_ref:
//
//   g++ -std=c++14 -O2 -pthread -w -fno-access-control -DTARGET_SIMD_X86=1 -DVVENC_SOURCE -DNDEBUG -I$O/gen -I$R/include -I$R/source/Lib/vvenc -I$R/source/Lib
//       -I$R/source/Lib/CommonLib -I$R/source/Lib/CommonLib/x86 -I$R/source/Lib/EncoderLib -isystem $R/thirdparty tests/intra_chroma_golden_gen.cpp
//       -Wl,--whole-archive $O/libvvenc_core.a -Wl,--no-whole-archive -o <somewhere outside the repository>/intra_chroma_golden_gen
//
// The availability functions of the reference walk a CodingStructure, so a real one is built: a 384 x 384 4:2:0 picture whose CodingStructure owns the two CU maps
// ( m_cuPtr[CH_L], m_cuPtr[CH_C] ) over its whole area, a Picture whose reconstruction buffer ( m_picBufs[PIC_RECONSTRUCTION], created with its margin ) holds the case's luma
// window around the block, and the block's CU at luma ( 128, 128 ).  Per case the neighbourhood is laid out with 4 x 4-luma CUs ( 2 x 2 chroma: the availability unit ) entered
// into both maps: the row above over the block's width plus the case's above-right count, the column to the left over its height plus the left-below count.  PreCalcValues
// is made while the SPS' CTUSize is 512 ( maxCUSizeLog2 9 ), so getCURestricted (CodingStructure.cpp:1144) sees one CTU and answers from the maps and the CUs' idx alone; the SPS' CTUSize — which only
// isFirstRowOfCtu (IntraPrediction.cpp:1241) reads here — is 32 for a case on the first row of its CTU and 512 otherwise.  The reference's own isAboveAvailable,
// isLeftAvailable, isAboveRightAvailable and isBelowLeftAvailable are inline and file-local; they are run through xFillReferenceSamples on cu.Cb() (:798-803), whose unit flags
// ( m_neighborFlags ) give the four availability numbers of the answer: the driver fails unless they are the case's flags and counts.
// Per case cu.intraDir[1] = MDLM_L_IDX and loadLMLumaRecPels( cu, cu.Cb() ) run once, as estIntraPredChromaQT does (EncoderLib/IntraSearch.cpp:796-800); the two components'
// reference lines are written into m_refBuffer[COMP_Cb / COMP_Cr][PRED_BUF_UNFILTERED] with m_refBufferStride, m_topRefLength and m_leftRefLength as initIntraPatternChType
// leaves them.  Per requested slot: modes 67..69 run xGetLMParameters (for the record) and predIntraChromaLM; modes 0..66 run initPredIntraParams and predIntraAng on
// cu.Cb() / cu.Cr() with cu.intraDir[1] = the mode.  The cost is min( 2 * DF_SAD, DF_HAD ) of Cb plus the same of Cr through RdCost::setDistParam, on 32-byte aligned
// compact blocks.
//
// Everything runs twice: IntraPrediction( false ), RdCost::create( false ) and the default PelBufferOps — the scalar row — then IntraPrediction( true ), RdCost::create( true )
// and g_pelBufOP.initPelBufOpsX86() — the x86 row.  The program fails unless the function pointers of the x86 row differ from the scalar ones.
//
// One list per run, read from argv[1], answered in argv[2]:
//   int32 nBlocks, reps; per block int32 w, h, bitDepth, flags, nAboveRight, nLeftBelow, modeMask, cand[8], winW, winH, then the luma window ( int16, winH x winW, the area's
//   top-left sample at ( 4, 4 ) ), the Cb and the Cr lines ( int16, 2 x ( 2w + 1 + 2h + 1 ) ), the two originals ( int16, 2 x w x h )
//   reps == 0 -> per row ( scalar, x86 ) and block: int32 above, left, nAboveRight, nLeftBelow as the reference derived them; per requested slot uint32 cost,
//                int32 ( a, b, shift ) of Cb and of Cr ( zeros for a regular mode ), the Cb and the Cr prediction ( int16, w x h each )
//   reps  > 0 -> double: the best seconds over the whole list of loadLMLumaRecPels + predict + score per requested slot, the x86 row, one core (a context figure)
#include <algorithm>
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "CommonLib/CommonDef.h"
#include "CommonLib/Unit.h"
#include "CommonLib/Buffer.h"
#include "CommonLib/Slice.h"
#include "CommonLib/Picture.h"
#include "CommonLib/CodingStructure.h"
#include "CommonLib/IntraPrediction.h"
#include "CommonLib/RdCost.h"

using namespace vvenc;

static bool rd( FILE* f, void* p, size_t bytes ) { return fread( p, 1, bytes, f ) == bytes; }

static const int PIC = 384, POS = 128, WORG = 4;
enum { FL_ABOVE = 1, FL_LEFT = 2, FL_FIRST_ROW = 4, FL_VER_COLLOCATED = 8 };

struct Block { int w, h, bitDepth, flags, nAR, nLB, modeMask, cand[8], winW, winH; std::vector<Pel> luma, lines[2], org[2]; };

struct World
{
  SPS* sps; PPS* pps; PreCalcValues* pcv; Slice* slice; XUCache* cache; CodingStructure* cs; Picture* pic;
  std::vector<CodingUnit*> mapL, mapC;
  std::vector<CodingUnit*> neighbours;
  CodingUnit* cu;
};

static void* zeroed( size_t bytes ) { void* p = aligned_alloc( 64, ( bytes + 63 ) & ~( size_t ) 63 ); memset( p, 0, ( bytes + 63 ) & ~( size_t ) 63 ); return p; }

static World* makeWorld()
{
  World* W = new World;
  W->sps = new SPS; W->pps = new PPS;
  W->sps->chromaFormatIdc = CHROMA_420; W->sps->CTUSize = 512;          // (what PreCalcValues takes its maxCUSizeLog2 from)
  W->pps->picWidthInLumaSamples = PIC; W->pps->picHeightInLumaSamples = PIC;
  const unsigned maxQt[3] = { 128, 128, 128 };
  W->pcv = new PreCalcValues( *W->sps, *W->pps, maxQt );
  W->slice = ( Slice* ) zeroed( sizeof( Slice ) );
  W->cache = new XUCache;
  W->cs = new CodingStructure( *W->cache, nullptr );
  W->pic = new Picture;
  CodingStructure* cs = W->cs;
  cs->picture = W->pic; W->pic->cs = cs; cs->slice = W->slice; cs->sps = W->sps; cs->pps = W->pps; cs->pcv = W->pcv; cs->parent = nullptr;
  cs->area = UnitArea( CHROMA_420, Area( 0, 0, PIC, PIC ) );
  cs->unitScale[COMP_Y] = UnitScale( 2, 2 ); cs->unitScale[COMP_Cb] = cs->unitScale[COMP_Cr] = UnitScale( 1, 1 );
  W->mapL.assign( ( size_t ) ( PIC / 4 ) * ( PIC / 4 ), nullptr ); W->mapC = W->mapL;
  cs->m_cuPtr[CH_L] = W->mapL.data(); cs->m_cuPtr[CH_C] = W->mapC.data();
  W->pic->chromaFormat = CHROMA_420;
  W->pic->m_picBufs[PIC_RECONSTRUCTION].create( CHROMA_420, Area( 0, 0, PIC, PIC ), 128, 16, MEMORY_ALIGN_DEF_SIZE );
  W->cu = new CodingUnit;
  return W;
}

static void place( World* W, CodingUnit* c )
{
  const Area& y = c->blocks[COMP_Y];
  for( int v = y.y / 4; v < ( y.y + ( int ) y.height ) / 4; v++ )
    for( int u = y.x / 4; u < ( y.x + ( int ) y.width ) / 4; u++ ) { W->mapL[( size_t ) v * ( PIC / 4 ) + u] = c; W->mapC[( size_t ) v * ( PIC / 4 ) + u] = c; }
}

static void initCu( World* W, CodingUnit* c, int x, int y, int w, int h, int idx )
{
  static_cast<UnitArea&>( *c ) = UnitArea( CHROMA_420, Area( x, y, w, h ) );
  c->cs = W->cs; c->slice = W->slice; c->chromaFormat = CHROMA_420; c->chType = CH_L; c->treeType = TREE_D; c->idx = idx; c->tileIdx = 0;
  c->multiRefIdx = 0; c->ispMode = 0; c->mipFlag = false; c->bdpcmM[0] = c->bdpcmM[1] = 0; c->intraDir[0] = 0; c->intraDir[1] = 0;
}

// the neighbourhood of a case and its luma window in the reconstruction buffer (the rest of the picture carries a fill that depends on `seed`: the two rows differ in it)
static void setScene( World* W, const Block& b, uint32_t seed )
{
  std::fill( W->mapL.begin(), W->mapL.end(), nullptr ); std::fill( W->mapC.begin(), W->mapC.end(), nullptr );
  for( CodingUnit* c : W->neighbours ) delete c;
  W->neighbours.clear();
  int idx = 1;
  auto unit = [&]( int x, int y ) { CodingUnit* c = new CodingUnit; initCu( W, c, x, y, 4, 4, idx++ ); place( W, c ); W->neighbours.push_back( c ); };
  if( b.flags & FL_ABOVE ) for( int x = 0; x < 2 * ( b.w + b.nAR ); x += 4 ) unit( POS + x, POS - 4 );
  if( b.flags & FL_LEFT )  for( int y = 0; y < 2 * ( b.h + b.nLB ); y += 4 ) unit( POS - 4, POS + y );
  initCu( W, W->cu, POS, POS, 2 * b.w, 2 * b.h, 1 << 20 );
  place( W, W->cu );
  W->sps->CTUSize = ( b.flags & FL_FIRST_ROW ) ? 32 : 512;
  W->sps->verCollocatedChroma = ( b.flags & FL_VER_COLLOCATED ) != 0;
  W->sps->bitDepths.recon[CH_L] = W->sps->bitDepths.recon[CH_C] = b.bitDepth;
  W->slice->clpRngs.bd = b.bitDepth;
  PelBuf reco = W->pic->m_picBufs[PIC_RECONSTRUCTION].bufs[COMP_Y];
  for( int y = 0; y < PIC; y++ )
    for( int x = 0; x < PIC; x++ ) { seed = seed * 1664525u + 1013904223u; reco.buf[( ptrdiff_t ) y * reco.stride + x] = ( Pel ) ( ( seed >> 16 ) & ( ( 1u << b.bitDepth ) - 1 ) ); }
  for( int y = 0; y < b.winH; y++ ) memcpy( reco.buf + ( ptrdiff_t ) ( POS - WORG + y ) * reco.stride + POS - WORG, b.luma.data() + ( size_t ) y * b.winW, ( size_t ) b.winW * sizeof( Pel ) );
}

struct Row { IntraPrediction* ip; RdCost* rc; Pel* org[2]; Pel* pred[2]; };

// the four availability numbers as the reference derives them from the CodingStructure: the availability functions are inline and file-local, so they are run where the
// reference itself runs them for a chroma block with the same arguments — xFillReferenceSamples (:755-804), which leaves one flag per 2-sample unit in m_neighborFlags
// ( left-below ... left | above-left | above ... above-right ).  The counts follow loadLMLumaRecPels' rule: an extension counts only behind a fully available side.
static void availability( World* W, Row& r, const Block& b, int32_t out[4] )
{
  const CodingUnit& cu = *W->cu;
  const CompArea& ca = cu.Cb();
  static Pel lines[4 * MAX_CU_SIZE + 8];
  r.ip->reset();
  r.ip->setReferenceArrayLengths( ca );
  r.ip->xFillReferenceSamples( W->pic->getRecoBuf( ca ), lines, ca, cu );
  const int aboveUnits = b.w / 2, leftUnits = b.h / 2, totalLeft = b.h;          // 2h samples in units of 2
  const bool* f = r.ip->m_neighborFlags;
  int above = 0, left = 0, ar = 0, lb = 0;
  for( int k = 0; k < aboveUnits; k++ ) above += f[totalLeft + 1 + k];
  for( int k = 0; k < aboveUnits; k++ ) ar += f[totalLeft + 1 + aboveUnits + k];
  for( int k = 0; k < leftUnits; k++ )  left += f[totalLeft - 1 - k];
  for( int k = 0; k < leftUnits; k++ )  lb += f[totalLeft - 1 - leftUnits - k];
  out[0] = above == aboveUnits; out[1] = left == leftUnits;
  out[2] = out[0] ? 2 * ar : 0; out[3] = out[1] ? 2 * lb : 0;
}

static void setLines( Row& r, const Block& b )
{
  for( int c = 0; c < 2; c++ )
  {
    const ComponentID id = c ? COMP_Cr : COMP_Cb;
    memcpy( r.ip->m_refBuffer[id][PRED_BUF_UNFILTERED], b.lines[c].data(), b.lines[c].size() * sizeof( Pel ) );
    r.ip->m_refBufferStride[id] = 2 * b.w + 1;
    memcpy( r.org[c], b.org[c].data(), b.org[c].size() * sizeof( Pel ) );
  }
  r.ip->m_topRefLength = 2 * b.w; r.ip->m_leftRefLength = 2 * b.h;
  r.ip->m_ipaParam.refFilterFlag = false;
}

static void loadLuma( World* W, Row& r )
{
  W->cu->intraDir[1] = MDLM_L_IDX;
  r.ip->loadLMLumaRecPels( *W->cu, W->cu->Cb() );
}

// one slot: the two predictions into r.pred, the parameter record into prm[2][3] -> the cost
static uint32_t oneSlot( World* W, Row& r, const Block& b, int mode, int32_t prm[2][3] )
{
  CodingUnit& cu = *W->cu;
  cu.intraDir[1] = mode;
  uint32_t total = 0;
  for( int c = 0; c < 2; c++ )
  {
    const ComponentID id = c ? COMP_Cr : COMP_Cb;
    const CompArea& area = cu.blocks[id];
    PelBuf pred( r.pred[c], b.w, b.w, b.h );
    prm[c][0] = prm[c][1] = prm[c][2] = 0;
    if( mode >= LM_CHROMA_IDX )
    {
      int a, bb, sh;
      r.ip->m_ipaParam.refFilterFlag = false;
      r.ip->xGetLMParameters( cu, id, area, a, bb, sh );
      prm[c][0] = a; prm[c][1] = bb; prm[c][2] = sh;
      r.ip->predIntraChromaLM( id, pred, cu, area, mode );
    }
    else
    {
      r.ip->initPredIntraParams( cu, area, *W->sps );
      r.ip->predIntraAng( id, pred, cu );
    }
    const CPelBuf o( r.org[c], b.w, b.w, b.h ), p( r.pred[c], b.w, b.w, b.h );
    DistParam dSad = r.rc->setDistParam( o, p, b.bitDepth, DF_SAD ), dHad = r.rc->setDistParam( o, p, b.bitDepth, DF_HAD );
    const int64_t sad = ( int64_t ) dSad.distFunc( dSad ) * 2, had = ( int64_t ) dHad.distFunc( dHad );
    total += ( uint32_t ) std::min( sad, had );
  }
  return total;
}

int main( int argc, char** argv )
{
  if( argc != 3 ) { fprintf( stderr, "usage: %s in out\n", argv[0] ); return 2; }
  FILE* fi = fopen( argv[1], "rb" ); FILE* fo = fopen( argv[2], "wb" );
  if( !fi || !fo ) return 2;
  int32_t hd[2];
  if( !rd( fi, hd, sizeof( hd ) ) ) return 2;
  const int nBlocks = hd[0], reps = hd[1];
  std::vector<Block> blocks( nBlocks );
  for( Block& b : blocks )
  {
    int32_t g[17];
    if( !rd( fi, g, sizeof( g ) ) ) return 2;
    b.w = g[0]; b.h = g[1]; b.bitDepth = g[2]; b.flags = g[3]; b.nAR = g[4]; b.nLB = g[5]; b.modeMask = g[6];
    for( int k = 0; k < 8; k++ ) b.cand[k] = g[7 + k];
    b.winW = g[15]; b.winH = g[16];
    b.luma.resize( ( size_t ) b.winW * b.winH );
    if( !rd( fi, b.luma.data(), b.luma.size() * 2 ) ) return 2;
    for( int c = 0; c < 2; c++ ) { b.lines[c].resize( 2 * b.w + 1 + 2 * b.h + 1 ); if( !rd( fi, b.lines[c].data(), b.lines[c].size() * 2 ) ) return 2; }
    for( int c = 0; c < 2; c++ ) { b.org[c].resize( ( size_t ) b.w * b.h ); if( !rd( fi, b.org[c].data(), b.org[c].size() * 2 ) ) return 2; }
    if( b.winW + POS - WORG > PIC || b.winH + POS - WORG > PIC ) return 2;
  }

  World* W = makeWorld();
  Row rows[2];
  const PelBufferOps scalarOps = g_pelBufOP;
  for( int pass = 0; pass < 2; pass++ )
  {
    Row& r = rows[pass];
    r.ip = new IntraPrediction( pass != 0 );
    r.ip->init( CHROMA_420, 10 );
    r.rc = new RdCost; r.rc->create( pass != 0 );
    for( int c = 0; c < 2; c++ ) { r.org[c] = ( Pel* ) zeroed( 64 * 64 * sizeof( Pel ) ); r.pred[c] = ( Pel* ) zeroed( 64 * 64 * sizeof( Pel ) ); }
  }
  PelBufferOps x86Ops = scalarOps;
  x86Ops.initPelBufOpsX86();
  {
    const IntraPrediction &a = *rows[0].ip, &x = *rows[1].ip;
    if( a.IntraPredAngleChroma == x.IntraPredAngleChroma || a.IntraAnglePDPC == x.IntraAnglePDPC || a.IntraHorVerPDPC == x.IntraHorVerPDPC || a.IntraPredSampleFilter == x.IntraPredSampleFilter ||
        a.xPredIntraPlanar == x.xPredIntraPlanar || rows[0].rc->m_afpDistortFunc[0][DF_HAD] == rows[1].rc->m_afpDistortFunc[0][DF_HAD] ||
        rows[0].rc->m_afpDistortFunc[0][DF_SAD] == rows[1].rc->m_afpDistortFunc[0][DF_SAD] || scalarOps.linTf4 == x86Ops.linTf4 || scalarOps.linTf8 == x86Ops.linTf8 )
    { fprintf( stderr, "this build has no x86 row\n" ); return 3; }
  }
  if( reps > 0 )
  {
    Row& r = rows[1];
    g_pelBufOP = x86Ops;
    // (the scene — the CU maps and the reconstruction — is set once per block outside the timed region: an encoder has both in place)
    double best = 1e30; uint64_t sink = 0;
    std::vector<double> per( blocks.size(), 1e30 );
    for( int k = 0; k < reps; k++ )
      for( size_t i = 0; i < blocks.size(); i++ )
      {
        const Block& b = blocks[i];
        setScene( W, b, 12345u );
        const auto t0 = std::chrono::steady_clock::now();
        setLines( r, b ); loadLuma( W, r );
        for( int s = 0; s < 8; s++ ) if( ( b.modeMask >> s ) & 1 ) { int32_t prm[2][3]; sink += oneSlot( W, r, b, b.cand[s], prm ); }
        per[i] = std::min( per[i], std::chrono::duration<double>( std::chrono::steady_clock::now() - t0 ).count() );
      }
    best = 0;
    for( double v : per ) best += v;
    if( sink == 1 ) fprintf( stderr, " " );
    fwrite( &best, 8, 1, fo );
  }
  else
    for( int pass = 0; pass < 2; pass++ )
    {
      g_pelBufOP = pass ? x86Ops : scalarOps;
      for( const Block& b : blocks )
      {
        Row& r = rows[pass];
        setScene( W, b, pass ? 99991u : 12345u );
        int32_t av[4];
        availability( W, r, b, av );
        fwrite( av, 4, 4, fo );
        setLines( r, b ); loadLuma( W, r );
        for( int s = 0; s < 8; s++ )
        {
          if( !( ( b.modeMask >> s ) & 1 ) ) continue;
          for( int c = 0; c < 2; c++ ) memset( r.pred[c], 0x55, 64 * 64 * sizeof( Pel ) );
          int32_t prm[2][3];
          const uint32_t cost = oneSlot( W, r, b, b.cand[s], prm );
          fwrite( &cost, 4, 1, fo );
          fwrite( prm, 4, 6, fo );
          for( int c = 0; c < 2; c++ ) fwrite( r.pred[c], sizeof( Pel ), ( size_t ) b.w * b.h, fo );
        }
      }
    }
  fclose( fi ); fclose( fo );
  fflush( nullptr );
  _Exit( 0 );      // (the hand-filled structures are not torn down: their destructors would free what they do not own)
}
