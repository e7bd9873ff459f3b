// common.h — internal declarations shared by the HIP translation units of libvvenc_hip.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <string>
#include <vector>
#include "../../include/vvenc_hip.h"

// ---- host lists on the device -------------------------------------------------------------------------------------------------
// An entry that launches from a host-built array (a sorted schedule, a picture's CTU parameters, a list of items) keeps it in a slot of the context: the device copy, the host
// copy the asynchronous upload reads, and the event recorded behind the last launch that read the device copy.  A cached entry also stores the key of the caller's list the
// array was derived from — a list that is run again is neither sorted nor uploaded again; a per-call entry uploads every time and leaves the key empty.  Every use has a slot of
// its own (ListSlot), so entries that alternate on one context evict nothing of each other's.  What an entry needs to know of its array beside the device pointer (section
// offsets, unit counts) it puts into a header struct of its own at the front of the blob and reads back through listHead: the host copy is valid exactly as long as the device
// copy is, and nothing here knows any entry's layout.  The three operations are in ctx.hip: listCurrent, listUpload, listLaunched.
struct HostList
{
  void*        d         = nullptr;      // device copy
  size_t       bytes     = 0;            // its capacity (grow-only)
  std::vector<unsigned char> blob;       // host copy: the source of the asynchronous upload, rewritten only after the last reader's event has been waited for
  std::vector<unsigned char> key;        // the caller's list the copies belong to; empty: none (a per-call array, or an upload that failed)
  hipStream_t  stream    = nullptr;      // the stream the array was uploaded on; compared only, never used as a handle
  hipEvent_t   event     = nullptr;      // recorded behind every launch that reads the device copy
  bool         eventRecorded = false;
};
enum ListSlot
{
  LIST_PRED, LIST_PRED_BLEND, LIST_PRED_CIIP,      // pred.hip: vvhip_pred_inter_batch[_ex]; ..._blend called with a blend array; ..._ciip called with a CIIP array
  LIST_AFFINE,                                     // predaffine.hip: vvhip_pred_affine_batch
  LIST_ICT_FWD, LIST_ICT_INV,                      // ict.hip: vvhip_ict_fwd_batch, vvhip_ict_inv_batch
  LIST_SBT_PARTS, LIST_SBT_PLACE,                  // sbt.hip: vvhip_sbt_parts_batch, vvhip_sbt_place_batch
  LIST_SAO_FLAGS, LIST_SAO_PARAMS,                 // sao.hip, per call: the CTU flags of vvhip_sao_stats, the CTU parameters of vvhip_sao_offset
  LIST_DEBLOCK,                                    // deblock.hip, per call: the band's loop-filter records of vvhip_deblock
  LIST_VISACT, LIST_VISACT_PART,                   // visact.hip, per call: the tile list and area table of vvhip_visact; its per-tile partial records (device only, see there)
  LIST_INTRA, LIST_INTRA_CHROMA,                   // intra.hip, intrachroma.hip, per call: the items of vvhip_intra_luma_modes_batch, of vvhip_intra_chroma_modes_batch
  LIST_MMVD,                                       // mmvd.hip, per call: the items and tiles of vvhip_merge_mmvd_costs_batch
  LIST_COUNT
};

// the sections of a blob in the order they are added, each starting at a multiple of `align` bytes; the data is copied when the blob is uploaded, so it must live until then
struct ListBlob
{
  struct Sec { const void* data; size_t bytes, off; } sec[8];
  int          n         = 0;
  size_t       size      = 0;
  ListBlob() {}
  ListBlob( const void* data, size_t bytes ) { add( data, bytes ); }      // a blob of one section
  size_t add( const void* data, size_t bytes, size_t align = 256 )      // -> the section's offset
  {
    size = ( size + align - 1 ) / align * align;
    sec[n++] = Sec{ data, bytes, size };
    size += bytes;
    return sec[n - 1].off;
  }
};

// sort key of a list item: size class, position inside the class, list index — a schedule holds the items in this order
struct ListKeyed { uint32_t cls; int64_t pos; int idx; };
inline bool operator<( const ListKeyed& a, const ListKeyed& b ) { return a.cls != b.cls ? a.cls < b.cls : a.pos != b.pos ? a.pos < b.pos : a.idx < b.idx; }

struct vvhip_ctx
{
  int          device     = 0;
  hipStream_t  stream     = nullptr;   // stream every launch goes to
  hipStream_t  ownStream  = nullptr;
  std::string  lastError;

  // ROM in HBM (uploaded once by vvhip_create)
  int16_t*     d_trMat    = nullptr;   // all transform matrices, see trMatOffset()
  uint16_t*    d_scan     = nullptr;   // grouped diagonal scan orders, see scanOffset()
  struct VvhipTuMxOps* d_tuMx = nullptr;   // matrix-core operand records of the fused TU kernel: [type][size 4,8,16,32], see VvhipTuMxOps
  struct VvhipTuMx64Ops* d_tuMx64 = nullptr;   // the 64-point DCT-2 record
  uint16_t*    d_tuMxPos  = nullptr;   // scan position of every (lane, register) of a 32x32 tile, per size: [4][64][16]
  // scratch for vvhip_mctf_motion_estimation (grown on demand)
  void*        d_scratch  = nullptr;
  size_t       scratchBytes = 0;
  // optional per-class events of the last vvhip_mctf_motion_estimation[_async] call (vvhip_mctf_set_timing): tag 0 call start, 1 before a level's candidate scoring, 2 after it,
  // 3 after the neighbour scoring, 4 after the sweep, 5 after the final normalisation, 6 call end
  bool         mctfTiming = false;
  std::vector<hipEvent_t> mctfEv;
  std::vector<int> mctfEvTag;
  unsigned long long* d_mctfStats = nullptr;   // scored-candidate counters of the MCTF search (vvhip_mctf_set_stats): 12 x uint64, null = off
  // scratch of vvhip_subpel_dist_batch: predicted blocks + distortion items (grown on demand)
  void*        d_subpel   = nullptr;
  size_t       subpelBytes = 0;
  // job table of the generic TU pipeline's merged launch (trquant.hip: tuRdoGenMultiKernel) + the host copy of what it holds
  void*        d_tuGen    = nullptr;
  size_t       tuGenBytes = 0;
  std::vector<unsigned char> tuGenLast;
  bool         tuSparse   = false;     // vvhip_tu_set_sparse_outputs: the fused TU launches of vvhip_tu_rdo_multi[_strided] write no levels / reconstruction for TUs whose levels are all zero
  hipStream_t  tuGenStream = nullptr;      // the stream the cached generic-TU job table was uploaded on (trquant.hip: tuRdoMulti); compared only, never used as a handle
  hipEvent_t   tuGenEvent  = nullptr;      // recorded behind every launch that reads the table: a caller that switches streams orders the new stream behind it
  bool         tuGenEventRecorded = false;
  // the host-built arrays the list entries keep on the device, one slot per use (HostList above)
  HostList     list[LIST_COUNT];
  // how the host waits for the stream (vvhip_set_blocking_sync): false = hipStreamSynchronize (the runtime's low-latency wait), true = a blocking event — the calling thread
  // sleeps, which matters when the host's cores are all busy encoding
  bool         blockingSync = false;
  hipEvent_t   syncEvent  = nullptr;
};

// every host wait of the library on a context's stream goes through this
inline hipError_t vvhip_wait_stream( vvhip_ctx* ctx )
{
  if( !ctx->blockingSync ) return hipStreamSynchronize( ctx->stream );
  if( !ctx->syncEvent ) return hipErrorInvalidHandle;      // (created by vvhip_create on the context's device)
  const hipError_t e = hipEventRecord( ctx->syncEvent, ctx->stream );
  return e != hipSuccess ? e : hipEventSynchronize( ctx->syncEvent );
}

int vvhip_fail( vvhip_ctx* ctx, int code, const char* fmt, ... );

// ---- the three operations on a host-list slot (ctx.hip); an entry validates its list BEFORE it calls listUpload, so that a list that fails validation leaves the slot untouched
// -> *current: the slot holds the list named by `key`, ordered in front of the next launch on the context's stream
int listCurrent( vvhip_ctx* ctx, HostList& S, const std::vector<unsigned char>& key, bool* current );
// the blob -> the slot's host copy -> its device copy, asynchronously on the context's stream, after the last launch that read the slot; key: swapped in on success (cached
// entries), or null for a per-call array, which is never current
int listUpload( vvhip_ctx* ctx, HostList& S, const ListBlob& blob, std::vector<unsigned char>* key = nullptr );
// behind the launches that read the slot
int listLaunched( vvhip_ctx* ctx, HostList& S );
// the slot's device buffer holds at least `bytes` (grow-only, contents lost on growth); the caller has waited for the slot's readers (listUpload has)
int listReserve( vvhip_ctx* ctx, HostList& S, size_t bytes );
// the header struct an entry put at the front of its blob
template<class H> inline const H& listHead( const HostList& S ) { return *reinterpret_cast<const H*>( S.blob.data() ); }

#define VVHIP_CHECK_HIP( ctx, expr )                                                        \
  do { hipError_t e_ = ( expr );                                                            \
       if( e_ != hipSuccess ) return vvhip_fail( ctx, VVHIP_E_HIP, "%s: %s (%s:%d)", #expr, \
                                                 hipGetErrorString( e_ ), __FILE__, __LINE__ ); } while( 0 )

#define VVHIP_LAUNCH_CHECK( ctx ) VVHIP_CHECK_HIP( ctx, hipGetLastError() )

// ---- ROM layout -------------------------------------------------------------------------------
// transform matrices: type-major, sizes 2..64; entry (type, log2N) lives at trMatOffset(type, log2N), N*N int16
static inline __host__ __device__ int trMatOffset( int trType, int log2N )
{
  // sum_{l=1}^{log2N-1} 4^l = (4^log2N - 4) / 3 ; each type gets a full 2..64 slot (5460 entries)
  return trType * 5460 + ( ( 1 << ( 2 * log2N ) ) - 4 ) / 3;
}
static const int kTrMatTotal = 3 * 5460;

// scan orders for log2w, log2h in 0..6: entry lives at scanOffset(log2w, log2h), (w*h) uint16
static inline __host__ __device__ int scanOffset( int log2w, int log2h )
{
  // prefix over (lw, lh) in row-major order of 2^(lw+lh): sum_{a<lw} 2^a*(127) + 2^lw * (2^lh - 1)
  return ( ( 1 << log2w ) - 1 ) * 127 + ( 1 << log2w ) * ( ( 1 << log2h ) - 1 );
}
static const int kScanTotal = 127 * 127;

// ---- matrix-core operands of the fused TU kernel (trquant.hip, tuMx*) ---------------------------------------------------------
// A 32x32 tile holds (32/N)^2 TUs of size N side by side; "big" is the block-diagonal 32x32 matrix of 32/N copies of the N-point kernel
// matrix (all entries fit 8 bits).  v_mfma_i32_32x32x32_i8 takes 16 bytes per lane for each operand: lane l = 32*h + r supplies row r (A) /
// column r (B) and K-slots (h, 0..15); result register v of lane l holds row mxHw(h, v), column r.  The data operand of every pass is the
// previous pass's result registers (slot s = register s), so the matrix operand's K-slot (h, s) is bound to index mxHw(h, s); and the
// A-side matrices supply their rows in the order mxSigma, which makes result register (h, v) hold logical row 16h + v — a lane's 16
// registers are 16 consecutive rows of ONE column: one 16-point TU, two 8-point TUs or half a 32-point TU.
static inline __host__ __device__ int mxHw( int h, int s ) { return 8 * ( s >> 2 ) + 4 * h + ( s & 3 ); }
static inline __host__ __device__ int mxSigma( int i )     { return 16 * ( ( i >> 2 ) & 1 ) + 4 * ( i >> 3 ) + ( i & 3 ); }   // mxSigma( mxHw( h, v ) ) == 16h + v
struct VvhipTuMxOps
{
  int8_t  nat[64][16];         // B side, forward rows:     lane l: big[l % 32][16h + s]                   (data slots = samples 16h + s of the lane's row)
  int8_t  rowP[64][16];        // A side, forward columns:  lane l: big[mxSigma(l % 32)][mxHw(h, s)]
  int8_t  natT[64][16];        // B side, inverse columns:  lane l: big[16h + s][l % 32]
  int8_t  colP[64][16];        // A side, inverse rows:     lane l: big[mxHw(h, s)][mxSigma(l % 32)]
  int32_t rowSum[32];          // 128 * sum_x big[r][x]: corrections for the (byte - 128) form of the data's low bytes
  int32_t colSum[32];          // 128 * sum_k big[k][c]
};

// 64-point DCT-2 with its zero-out (only the 32 low frequencies per direction survive, TrQuant.cpp:496-497): one wave per 64x64 TU, the
// residual as two row tiles x two column chunks of 32, every contraction over 64 split into two accumulating products.
struct VvhipTuMx64Ops
{
  int8_t  natX[2][64][16];     // forward rows,    B side, x chunk c:  T[l % 32][32c + 16h + s]
  int8_t  rowPY[2][64][16];    // forward columns, A side, row tile t: T[mxSigma(l % 32)][32t + mxHw(h, s)]
  int8_t  natTY[2][64][16];    // inverse columns, B side, row tile t: T[16h + s][32t + l % 32]
  int8_t  colPX[2][64][16];    // inverse rows,    A side, x chunk c:  T[mxHw(h, s)][32c + mxSigma(l % 32)]
  int32_t rowSum[32];          // 128 * sum_{x < 64} T[k][x]
  int32_t colSum[64];          // 128 * sum_{k < 32} T[k][x]
  uint16_t pos[64][16];        // scan position of coefficient (16h + v, l % 32) inside the 64x64 TU
};

void vvhip_build_tr_matrix( int trType, int log2N, int16_t* out );          // host
void vvhip_build_scan_order( int log2w, int log2h, uint32_t* out );         // host
void vvhip_cg_size( int log2w, int log2h, int* log2CGw, int* log2CGh );     // host

// XCD-aware order of a size class's workgroups (pred.hip), shared by the prediction-list entries
std::vector<int> predBandOrder( int nGroups, int base );

static inline int ilog2i( int v ) { int l = 0; while( ( 1 << ( l + 1 ) ) <= v ) l++; return l; }
static inline bool isPow2( int v ) { return v > 0 && ( v & ( v - 1 ) ) == 0; }

// ---- blending two hypotheses with weights w0 + w1 = 8 (pred.hip: BCW, GEO) --------------------------------------------------
// The weight of hypothesis 0 at sample ( x, y ) of a component block is a clamped line: a BCW block has a = b = 0, c = 8 * w0 and lo = hi = w0; a GEO block has
// lo = 0, hi = 8 and the line of its split direction through the 112 x 112 weight mask, with the CU's offset into the mask, the mirror and the component's scale folded
// into ( a, b, c ) by the host (g_globalGeoWeights is Clip3( 0, 8, ( A * mx + B * my + C ) >> 3 ): Rom.cpp:1320-1342, read at InterpolationFilter.cpp:1024-1062).
static inline __host__ __device__ int vvhipBlendW0( int a, int b, int c, int lo, int hi, int x, int y )
{
  const int w = ( a * x + b * y + c ) >> 3;
  return w < lo ? lo : ( w > hi ? hi : w );
}

// ---- cross-lane helpers (device) ----------------------------------------------------------------------------------------
// Sum over aligned groups of G (2..64, power of two) consecutive lanes using DPP only (no LDS crossbar traffic): quad_perm
// xor-1 / xor-2, row_half_mirror (8 lanes), row_mirror (16 lanes), then v_readlane of the four 16-lane row totals.
// The result is valid in every lane of the group.
#ifdef __HIPCC__
#define VVHIP_DPP( v, ctrl ) __builtin_amdgcn_mov_dpp( ( int ) ( v ), ( ctrl ), 0xf, 0xf, true )
#define VVHIP_DPP_XOR1        0xB1    /* quad_perm [1,0,3,2] */
#define VVHIP_DPP_XOR2        0x4E    /* quad_perm [2,3,0,1] */
#define VVHIP_DPP_HALF_MIRROR 0x141   /* lane i <-> 7-i inside 8 lanes  */
#define VVHIP_DPP_MIRROR      0x140   /* lane i <-> 15-i inside 16 lanes */

__device__ __forceinline__ uint32_t vvhipGroupSum32( uint32_t v, int G, int lane )
{
  if( G >= 2 )  v += ( uint32_t ) VVHIP_DPP( v, VVHIP_DPP_XOR1 );
  if( G >= 4 )  v += ( uint32_t ) VVHIP_DPP( v, VVHIP_DPP_XOR2 );
  if( G >= 8 )  v += ( uint32_t ) VVHIP_DPP( v, VVHIP_DPP_HALF_MIRROR );
  if( G >= 16 ) v += ( uint32_t ) VVHIP_DPP( v, VVHIP_DPP_MIRROR );
  if( G >= 32 )
  {
    const uint32_t r0 = ( uint32_t ) __builtin_amdgcn_readlane( ( int ) v, 0 ),  r1 = ( uint32_t ) __builtin_amdgcn_readlane( ( int ) v, 16 );
    const uint32_t r2 = ( uint32_t ) __builtin_amdgcn_readlane( ( int ) v, 32 ), r3 = ( uint32_t ) __builtin_amdgcn_readlane( ( int ) v, 48 );
    v = G == 64 ? r0 + r1 + r2 + r3 : ( lane < 32 ? r0 + r1 : r2 + r3 );
  }
  return v;
}
#define VVHIP_GROUP_REDUCE( NAME, OP )                                                                                         \
__device__ __forceinline__ uint32_t NAME( uint32_t v, int G, int lane )                                                          \
{                                                                                                                                \
  if( G >= 2 )  { const uint32_t o = ( uint32_t ) VVHIP_DPP( v, VVHIP_DPP_XOR1 ); v = OP; }                                      \
  if( G >= 4 )  { const uint32_t o = ( uint32_t ) VVHIP_DPP( v, VVHIP_DPP_XOR2 ); v = OP; }                                      \
  if( G >= 8 )  { const uint32_t o = ( uint32_t ) VVHIP_DPP( v, VVHIP_DPP_HALF_MIRROR ); v = OP; }                               \
  if( G >= 16 ) { const uint32_t o = ( uint32_t ) VVHIP_DPP( v, VVHIP_DPP_MIRROR ); v = OP; }                                    \
  if( G >= 32 )                                                                                                                  \
  {                                                                                                                              \
    uint32_t r[4] = { ( uint32_t ) __builtin_amdgcn_readlane( ( int ) v, 0 ), ( uint32_t ) __builtin_amdgcn_readlane( ( int ) v, 16 ),       \
                      ( uint32_t ) __builtin_amdgcn_readlane( ( int ) v, 32 ), ( uint32_t ) __builtin_amdgcn_readlane( ( int ) v, 48 ) };    \
    uint32_t a, b;                                                                                                               \
    { const uint32_t v = r[0], o = r[1]; a = OP; } { const uint32_t v = r[2], o = r[3]; b = OP; }                                \
    if( G == 64 ) { const uint32_t v = a, o = b; a = OP; b = a; }                                                                \
    v = lane < 32 ? a : b;                                                                                                       \
  }                                                                                                                              \
  return v;                                                                                                                      \
}
VVHIP_GROUP_REDUCE( vvhipGroupMax32, ( o > v ? o : v ) )
VVHIP_GROUP_REDUCE( vvhipGroupOr32, ( v | o ) )

// exact 64-bit group sum of per-lane values < 2^50 through two 32-bit limbs (24-bit split)
__device__ __forceinline__ unsigned long long vvhipGroupSum64( unsigned long long e, int G, int lane )
{
  const uint32_t lo = vvhipGroupSum32( ( uint32_t ) ( e & 0xFFFFFFull ), G, lane ), hi = vvhipGroupSum32( ( uint32_t ) ( e >> 24 ), G, lane );
  return ( ( unsigned long long ) hi << 24 ) + lo;
}
#endif
