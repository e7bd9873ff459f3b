// affine_golden_gen.cpp — records what the reference encoder's own xPredAffineBlk computes, for tests/golden/affine.npz (driver: tests/affine_golden_gen.py).
//
// Not part of build() and of no Makefile: compiled and linked by hand against the reference library where its sources and oracle/_ref/libvvenc_core.a
// (made by `make -C oracle/ref core`) exist.  With R = the reference checkout and O = oracle/_ref:
//
//   g++ -std=c++14 -O2 -pthread -w -DTARGET_SIMD_X86=1 -DVVENC_SOURCE -DNDEBUG -I$O/gen -I$R/include -I$R/source/Lib/vvenc -I$R/source/Lib
//       -I$R/source/Lib/CommonLib -I$R/source/Lib/CommonLib/x86 -isystem $R/thirdparty tests/affine_golden_gen.cpp
//       -Wl,--whole-archive $O/libvvenc_core.a -Wl,--no-whole-archive -o <somewhere outside the repository>/affine_golden_gen
//
// A subclass exposes the protected members of InterPredInterpolation.  The set-up is the least xPredAffineBlk reads: default-constructed SPS / PPS / PicHeader / Slice,
// PreCalcValues from them, a CodingStructure that points at them, two reference Pictures whose reconstruction buffers are filled from the input planes (luma and Cb),
// a CodingUnit with affine, affineType, interDir and mcControl = 0.  Per case and per list used: the luma call (which also leaves the stored vectors the chroma call reads),
// then the Cb call; `bi` is true when both lists are used.  The PROF setting of a case maps to the state the function reads: 0: sps.PROF off; 1: on, m_encOnly off;
// 2: m_encOnly on, checkLDC off, m_isBi off; 3: the same with m_isBi on.  Everything once after init( false ) (the scalar row) and once after init( true ) (the x86 row).
//
// input  (argv[1]) : int32 picW, picH, ctu, margin, nCases; two pictures x ( luma plane ( picH + 2 margin ) x ( picW + 2 margin ), Cb plane at half the size ) at 10 bit, int16;
//                    per case int32 bitDepth (8: the planes >> 2), cuX, cuY, cuW, cuH, sixParam, interDir, prof, refPic[2], cpmv[2][3][2]
// output (argv[2]) : per case, per row (scalar, x86), per list used: the cuH x cuW luma block, then the cuH/2 x cuW/2 Cb block, int16
#include <cstdio>
#include <cstdint>
#include <cstring>
#include <vector>
#include "CommonLib/CommonDef.h"
#include "CommonLib/Unit.h"
#include "CommonLib/Picture.h"
#include "CommonLib/Slice.h"
#include "CommonLib/CodingStructure.h"
#include "CommonLib/InterPrediction.h"

using namespace vvenc;

struct Probe : public InterPredInterpolation
{
  void state( int prof ) { m_skipPROF = false; m_ifpLines = 0; m_encOnly = prof >= 2; m_isBi = prof == 3; }
  void run( ComponentID comp, const CodingUnit& cu, const Picture* ref, const Mv* mv, PelUnitBuf& dst, bool bi, const ClpRng& clp, RefPicList l ) { xPredAffineBlk( comp, cu, ref, mv, dst, bi, clp, l ); }
};

int main( int argc, char** argv )
{
  if( argc != 3 ) { fprintf( stderr, "usage: %s in out\n", argv[0] ); return 2; }
  FILE* fi = fopen( argv[1], "rb" ); FILE* fo = fopen( argv[2], "wb" );
  if( !fi || !fo ) return 2;
  Probe probe[2];
  probe[0].init( false );
  probe[1].init( true );
  if( probe[1].xFpApplyPROF == probe[0].xFpApplyPROF || probe[1].xFpProfGradFilter == probe[0].xFpProfGradFilter ) { fprintf( stderr, "no x86 row on this machine\n" ); return 3; }
  int32_t hd[5];
  if( fread( hd, 4, 5, fi ) != 5 ) return 2;
  const int picW = hd[0], picH = hd[1], ctu = hd[2], margin = hd[3], nCases = hd[4];

  SPS sps; PPS pps; PicHeader ph; Slice slice;
  sps.chromaFormatIdc = CHROMA_420; sps.CTUSize = ctu;
  pps.picWidthInLumaSamples = picW; pps.picHeightInLumaSamples = picH;
  ph.disProfFlag = false;
  const unsigned maxQt[3] = { ( unsigned ) ctu, ( unsigned ) ctu, ( unsigned ) ctu };
  PreCalcValues pcv( sps, pps, maxQt );
  XUCache cache;
  CodingStructure cs( cache, nullptr );
  cs.sps = &sps; cs.pps = &pps; cs.picHeader = &ph; cs.pcv = &pcv; cs.slice = &slice;

  // the two reference pictures at 10 bit and at 8 bit (the same planes >> 2)
  Picture pic[2][2];
  for( int p = 0; p < 2; p++ )
  {
    for( int b = 0; b < 2; b++ )
    {
      pic[b][p].m_picBufs[PIC_RECONSTRUCTION].create( CHROMA_420, Area( 0, 0, picW, picH ), ctu, margin, MEMORY_ALIGN_DEF_SIZE );
      pic[b][p].cs = &cs;
    }
    for( int c = 0; c < 2; c++ )
    {
      const int m = margin >> c, w = ( picW >> c ) + 2 * m, h = ( picH >> c ) + 2 * m;
      std::vector<int16_t> plane( ( size_t ) w * h );
      if( fread( plane.data(), 2, plane.size(), fi ) != plane.size() ) return 2;
      for( int b = 0; b < 2; b++ )
      {
        PelBuf buf = pic[b][p].m_picBufs[PIC_RECONSTRUCTION].bufs[c ? COMP_Cb : COMP_Y];
        for( int y = 0; y < h; y++ ) for( int x = 0; x < w; x++ ) buf.buf[( y - m ) * ( ptrdiff_t ) buf.stride + ( x - m )] = ( Pel ) ( plane[( size_t ) y * w + x] >> ( b ? 2 : 0 ) );
      }
    }
  }

  for( int i = 0; i < nCases; i++ )
  {
    int32_t c[22];
    if( fread( c, 4, 22, fi ) != 22 ) return 2;
    const int bd = c[0], cuX = c[1], cuY = c[2], cuW = c[3], cuH = c[4], six = c[5], interDir = c[6], prof = c[7];
    const int32_t* cp = c + 10;
    CodingUnit cu( CHROMA_420, Area( cuX, cuY, cuW, cuH ) );
    cu.cs = &cs; cu.slice = &slice; cu.affine = true; cu.affineType = six ? AFFINEMODEL_6PARAM : AFFINEMODEL_4PARAM; cu.interDir = ( uint8_t ) interDir; cu.mcControl = 0;
    sps.PROF = prof != 0; slice.checkLDC = false;
    ClpRng clp; clp.bd = bd;
    PelStorage dst;
    dst.create( CHROMA_420, Area( 0, 0, cuW, cuH ) );
    for( int row = 0; row < 2; row++ )
    {
      probe[row].state( prof );
      for( int l = 0; l < 2; l++ )
      {
        if( !( interDir & ( 1 << l ) ) ) continue;
        Mv mv[3];
        for( int k = 0; k < 3; k++ ) mv[k] = Mv( cp[( l * 3 + k ) * 2], cp[( l * 3 + k ) * 2 + 1] );
        const Picture* ref = &pic[bd == 8 ? 1 : 0][c[8 + l]];
        PelUnitBuf ub = dst;
        for( int comp = 0; comp < 2; comp++ )
        {
          const ComponentID id = comp ? COMP_Cb : COMP_Y;
          dst.bufs[id].fill( -1 );
          probe[row].run( id, cu, ref, mv, ub, interDir == 3, clp, l ? REF_PIC_LIST_1 : REF_PIC_LIST_0 );
          const PelBuf& b = dst.bufs[id];
          for( int y = 0; y < ( cuH >> comp ); y++ ) fwrite( b.buf + ( ptrdiff_t ) y * b.stride, 2, cuW >> comp, fo );
        }
      }
    }
    dst.destroy();
  }
  fclose( fi ); fclose( fo );
  return 0;
}
