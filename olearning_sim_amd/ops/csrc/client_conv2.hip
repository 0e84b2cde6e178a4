// Client-batched 3x3 convolution, v6 family: padded-input implicit GEMM.
//
// What changed vs client_conv.hip's v5 pipeline (measured on MI355X,
// tools/convbench3.py):
//  - the input (activations for fwd/wgrad, dy for dgrad) arrives with a
//    1-element zero halo per plane ([.., H+2, W+2], F.pad on the host),
//    so the implicit-im2col gather has NO bounds masks, NO clamps and
//    NO float round-trips — each element is one ushort load at a
//    directly-addressed offset (v5 spent ~10 VALU ops per gathered
//    element on decompose+mask+select+cvt; PMC showed the kernels
//    issue-bound on that, MFMA busy <10%);
//  - XCD-aware block mapping: all (m,n)-tiles of one client land on one
//    XCD so the client's operand panels stay in that XCD's 4 MB L2
//    (deep layers re-read x / dy across tiles; dispatch places block b
//    on XCD b%8 — cdna_hip_programming.md T1);
//  - small planes (OW 4/8) hoist the (b,oh) decomposition per sub-row
//    instead of per element (template LG_OW);
//  - stride-2 dgrad is parity-decomposed into 4 dense classes (he,we):
//    output position (2i+he, 2j+we) only receives taps with
//    (he+dh-1)%2==0 / (we+dw-1)%2==0, so each class contracts over
//    K=OC*nh*nw with NO zero rows — v5's masked formulation spent 4x
//    the useful MFMA work (measured 21-29 TF vs ~90 for stride-1).
//
// GEMM structure per (client, m-tile, n-tile) workgroup is v5's:
// BM=64 (4 waves x 16 rows), BN=128, BK=32, A-operand read directly
// from global (16 B/lane/K-step), B tile double-buffered in LDS, one
// barrier per K-step, register-double-buffered gather (loads for step
// k+1 issue before the MFMAs of step k).  The forward kernels also have a
// BM=128 x BN=64 block (TILE, four waves of 32 rows x 64 columns) for
// OC where it adds no padded rows: every B fragment read feeds two MFMAs
// and the block gathers and commits half the columns per MFMA
// (conv3_route.h conv3_tile_v6).  The B tile is k-major with
// transposed fragment reads in the stride-1 fwd / dgrad kernels (KM,
// below) and [n][k+pad] with aligned ds_read_b128 fragments elsewhere.
// fwd_v6 / fwd_v7 / dgrad_v6 are compiled for exactly 4 waves per SIMD
// (amdgpu_waves_per_eu): the residency their LDS and 256-thread blocks
// give anyway.  Without it hipcc splits the 32 accumulators between
// VGPRs and AGPRs, copies them across every K-step (64 v_accvgpr moves)
// and, short of registers, waits for each fragment read before the one
// MFMA that uses it; with it the accumulators stay in VGPRs and the
// fragment reads are issued in batches ahead of the MFMAs.
//
// Replaces the role of MIOpen grouped conv on the simulator's hot path
// (reference delegates all compute to operator subprocesses,
// ols_core/taskMgr/utils/utils_run_task.py:496-514 — no kernels to
// port; this is the MI355X-native design).

#include "common.h"
#include "conv3_route.h"
#include "ols_ops.h"

typedef __attribute__((ext_vector_type(8))) short bf16x8;
typedef __attribute__((ext_vector_type(4))) float f32x4;

#define CV6_BM 64
#define CV6_BN 128
#define CV6_BK 32
#define CV6_PAD 8
#define CONV_THREADS 256

struct ConvGeom6 {
  int B, Hp, Wp;        // padded input plane (Hp = H + 2)
  int OH, OW;           // output plane
  int IC, OC, stride;
  int C, tiles_m, tiles_n;
  int lg_ow, lg_ohw;    // log2(OW), log2(OH*OW) — pow2 planes only
};

// Map a linear block id to (client, tile) with all of one client's
// tiles on one XCD (dispatch: block b -> XCD b%8). The grid is padded
// to ceil(C/8)*8 clients; surplus blocks exit.
__device__ __forceinline__ bool xcd_remap6(int lid, int C, int T,
                                           int& c, int& tile) {
  const int xcd = lid & 7;
  const int s = lid >> 3;
  const int grp = s / T;
  tile = s - grp * T;
  c = xcd + 8 * grp;
  return c < C;
}

// ---------------------------------------------------------------------------
// k-major B tile for the stride-1 kernels (template argument KM).
//
// The [n][k+pad] tile takes one ds_write_b16 per gathered element: a
// thread owns one k and 16 (or 32) consecutive n, so nothing it holds is
// contiguous in that tile.  Stored [k][n] instead, its 16 n are the 32
// bytes the two global loads delivered, committed as two ds_write_b128,
// and ds_read_b64_tr_b16 (gfx950) hands the MFMA the B fragment
// transposed: lane 16g+i gets column i, rows 8g..8g+7 — the operand map
// of the ds_read_b128 it replaces, so the same 8 k enter the same MFMA
// in the same order and results are bit-identical.
//
// Image, in shorts, of a BK x 128 tile (BK*256 bytes, 16-byte aligned):
//   off(row, nt, h) = nt*BK*16 + 16*row' + 8*(h ^ s)
//   row' = row ^ (4 if row & 8),  s = (row' >> 2) & 1
// nt is the 16-column n-tile, h the 16-byte half of its 32-byte row.
// Each n-tile is a dense [BK][16] block, so nt is an immediate offset
// on one base address per read.  Banks, by the rules of
// MI355X_MICROARCH.md (LDS):
//  - ds_read_b64_tr_b16 conflicts per 32-lane half over 64 banks.  A
//    half reads rows {r..r+3} and {r+8..r+11} (r = 0 or 4, +16 for the
//    upper half) of one n-tile, 2 x 128 bytes.  Plain 32-byte rows would
//    put the two blocks 256 bytes apart, on the same banks; row' moves
//    the second block by 128 bytes, so the 32 lanes cover 256 contiguous
//    bytes mod 256: conflict-free.
//  - ds_write_b128 conflicts per 8 consecutive lanes over 32 banks.  The
//    8 lanes hold 8 consecutive k of one n-tile and store the same half:
//    at a 32-byte pitch rows i and i+4 would share banks; s swaps the
//    halves of rows 4..7, so the 8 stores cover 128 contiguous bytes
//    mod 128: conflict-free.
// The 128x64 block tile (template argument TILE of fwd v6 / v7) is the
// same image with four n-tiles instead of eight, and both arguments were
// re-derived for its thread maps.  Read: a wave still reads whole n-tiles
// with km_frag_off, whichever rows it owns, so the per-half address set is
// the one above.  Write: fwd v6 has kk = tid % 32 and 8 columns per
// thread, (nt, h) = (grp >> 1, grp & 1) with grp = tid / 32; fwd v7 has
// kk = tid & 63 and one n-tile per thread, both halves.  Either way 8
// consecutive lanes share grp, so they hold 8 consecutive k (8j .. 8j+7,
// which row' permutes among themselves) of one n-tile and store the same
// half: the 128 contiguous bytes mod 128 of the second argument.
// The transposed read needs EXEC all ones and 8-byte-aligned addresses
// (cdna_hip_programming.md T10, G17): the tiles are aligned(16), every
// lane reads an address inside the tile, and the only exit before the
// main loop is the block-uniform xcd_remap6 return.
typedef __attribute__((ext_vector_type(4))) short bf16x4;
typedef __attribute__((ext_vector_type(4), aligned(2))) ushort u16x4_u;
typedef __attribute__((ext_vector_type(8), aligned(2))) ushort u16x8_u;
typedef __attribute__((address_space(3))) bf16x4 lds_bf16x4;

__device__ __forceinline__ int km_row(int row) {
  return row ^ ((row >> 1) & 4);
}

// NCOL gathered columns of one k, packed as loaded: v[i] holds columns
// 8i .. 8i+7.  The runs are 2-byte aligned (dw shifts them by one
// element); the unaligned vector types keep them single global loads.
template <int NCOL>
struct KmRun {
  uint4 v[NCOL / 8];
  // columns 8i .. 8i+7 from row[0..7]
  __device__ __forceinline__ void load8(int i, const ushort* row) {
    v[i] = __builtin_bit_cast(uint4,
                              *reinterpret_cast<const u16x8_u*>(row));
  }
  // columns 4i .. 4i+3 from row[0..3]
  __device__ __forceinline__ void load4(int i, const ushort* row) {
    const uint2 t =
        __builtin_bit_cast(uint2, *reinterpret_cast<const u16x4_u*>(row));
    if (i & 1) { v[i >> 1].z = t.x; v[i >> 1].w = t.y; }
    else       { v[i >> 1].x = t.x; v[i >> 1].y = t.y; }
  }
};

// commit half h (columns 8h .. 8h+7) of row kk of n-tile nt: one
// ds_write_b128, data as loaded
template <int BK>
__device__ __forceinline__ void km_store_half(short* tile, int kk, int nt,
                                              int h, const uint4& v) {
  const int rp = km_row(kk);
  const int s = (rp >> 2) & 1;
  *reinterpret_cast<uint4*>(tile + nt * (BK * 16) + 16 * rp + 8 * (h ^ s)) = v;
}

// commit row kk of n-tile nt: two ds_write_b128, data as loaded
template <int BK>
__device__ __forceinline__ void km_store(short* tile, int kk, int nt,
                                         const uint4& lo, const uint4& hi) {
  const int rp = km_row(kk);
  const int s = (rp >> 2) & 1;
  short* p = tile + nt * (BK * 16) + 16 * rp;
  *reinterpret_cast<uint4*>(p + 8 * s) = lo;
  *reinterpret_cast<uint4*>(p + 8 * (s ^ 1)) = hi;
}

// per-lane offset (shorts) of the transposed read of rows r0+8g+q
// (lane = 16g+4q+p) inside n-tile 0; r0 = 0 or 4, +32 rows = +512
__device__ __forceinline__ int km_frag_off(int lane, int r0) {
  const int p = lane & 3;
  const int rp = km_row(r0 + 8 * (lane >> 4) + ((lane >> 2) & 3));
  const int s = (rp >> 2) & 1;
  return 16 * rp + 8 * ((p >> 1) ^ s) + 4 * (p & 1);
}

// B fragment of n-tile nt, k rows krow0 .. krow0+31 (krow0 = 0 or 32)
template <int BK>
__device__ __forceinline__ bf16x8 km_frag(const short* tile, int off_lo,
                                          int off_hi, int nt, int krow0) {
  const short* base = tile + nt * (BK * 16) + krow0 * 16;
  bf16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
      (lds_bf16x4*)(base + off_lo));
  bf16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
      (lds_bf16x4*)(base + off_hi));
  return __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
}

// ---------------------------------------------------------------------------
// fwd v6: y[c][oc][n] = sum_k W[c][oc][k] * x_pad[c][ic][b][oh*s+dh][ow*s+dw]
// (k = (ic,dh,dw), dw fastest).
//
// LG_OW: 2 or 3 hoist (b,oh) per sub-row of 4/8 columns; 4 = "OW >= 16",
// whole 16-column segment in one output row.
// KM: k-major B tile (above), stride 1 only; false = the [n][k+pad] tile.
// TILE: 0 = 64x128 block, 16 rows per wave; 1 = 128x64, 32 rows per wave
// (two A fragments, acc[2][4]) and 8 gathered columns per thread, half an
// n-tile: one ds_write_b128.  Same k, same MFMA, same K order per output
// element either way.
template <int LG_OW_T, int STRIDE, bool KM = false, int TILE = 0>
__global__ __launch_bounds__(CONV_THREADS)
__attribute__((amdgpu_waves_per_eu(4, 4))) void k_conv3x3_fwd_v6(
    const __hip_bfloat16* __restrict__ xp, const __hip_bfloat16* __restrict__ w,
    __hip_bfloat16* __restrict__ y, ConvGeom6 g) {
  static_assert(!KM || STRIDE == 1, "k-major staging needs contiguous runs");
  static_assert(TILE == 0 || TILE == 1, "64x128 or 128x64");
  constexpr int BM = TILE ? 128 : CV6_BM, BN = TILE ? 64 : CV6_BN;
  constexpr int MI = BM / 64;               // 16-row A fragments per wave
  constexpr int NTW = BN / 16;              // 16-column n-tiles per wave
  constexpr int NCOL = BN / 8;              // gathered columns per thread
  int c, tile;
  if (!xcd_remap6(blockIdx.x, g.C, g.tiles_m * g.tiles_n, c, tile)) return;
  const int mt = tile / g.tiles_n;
  const int m0 = mt * BM;
  const int n0 = (tile - mt * g.tiles_n) * BN;

  __shared__ __attribute__((aligned(16))) short
      bT_lds[2][BN * (KM ? CV6_BK : CV6_BK + CV6_PAD)];
  const int K = g.IC * 9;
  const int N = g.B * g.OH * g.OW;
  const int HpWp = g.Hp * g.Wp;
  const int64_t planeB = (int64_t)g.B * HpWp;
  const ushort* xc =
      reinterpret_cast<const ushort*>(xp) + (int64_t)c * g.IC * planeB;
  const __hip_bfloat16* wc = w + (int64_t)c * g.OC * K;
  __hip_bfloat16* yc = y + (int64_t)c * g.OC * N;

  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  // wave w owns rows m0 + 16*MI*w .. and all BN columns
  const int wrow0 = 16 * MI * wave;
  const __hip_bfloat16* wrow[MI];
  bool arow_ok[MI];
#pragma unroll
  for (int mi = 0; mi < MI; ++mi) {
    const int arow = m0 + wrow0 + mi * 16 + (lane & 15);
    wrow[mi] = wc + (int64_t)min(arow, g.OC - 1) * K;
    arow_ok[mi] = arow < g.OC;
  }

  f32x4 acc[MI][NTW];
#pragma unroll
  for (int mi = 0; mi < MI; ++mi)
#pragma unroll
    for (int i = 0; i < NTW; ++i) acc[mi][i] = {0.f, 0.f, 0.f, 0.f};

  const int kk = threadIdx.x % CV6_BK;
  const int nn0 = (threadIdx.x / CV6_BK) * NCOL;
  ushort breg[NCOL];                        // !KM
  KmRun<NCOL> brun;                         // KM
  const int foff_lo = km_frag_off(lane, 0), foff_hi = km_frag_off(lane, 4);

  auto gather = [&](int k0) {
    const int k = k0 + kk;                  // < K (K % BK == 0)
    const int ic = k / 9, r = k - ic * 9;
    const int dh = r / 3, dw = r - dh * 3;
    const ushort* plane = xc + (int64_t)ic * planeB;
    if (LG_OW_T >= 4) {
      // whole NCOL-column segment inside one output row
      int n = min(n0 + nn0, N - 1);
      int b = n >> g.lg_ohw;
      int q = n & ((1 << g.lg_ohw) - 1);
      int oh = q >> g.lg_ow;
      int ow0 = min(q & ((1 << g.lg_ow) - 1), g.OW - NCOL);
      const ushort* row = plane + (int64_t)b * HpWp
                          + (oh * STRIDE + dh) * g.Wp + ow0 * STRIDE + dw;
      if constexpr (KM) {
#pragma unroll
        for (int j = 0; j < NCOL / 8; ++j) brun.load8(j, row + 8 * j);
      } else {
#pragma unroll
        for (int j = 0; j < NCOL; ++j) breg[j] = row[j * STRIDE];
      }
    } else {
      // OW = 4 or 8: hoist per sub-row of OW columns
      constexpr int SUBW = 1 << LG_OW_T;
      constexpr int NROW = NCOL / SUBW;
#pragma unroll
      for (int rr = 0; rr < NROW; ++rr) {
        int n = min(n0 + nn0 + rr * SUBW, N - 1);
        int b = n >> g.lg_ohw;
        int q = n & ((1 << g.lg_ohw) - 1);
        int oh = q >> LG_OW_T;
        const ushort* row = plane + (int64_t)b * HpWp
                            + (oh * STRIDE + dh) * g.Wp + dw;
        if constexpr (KM) {
          if (SUBW == 8) brun.load8(rr, row);
          else brun.load4(rr, row);
        } else {
#pragma unroll
          for (int j = 0; j < SUBW; ++j)
            breg[rr * SUBW + j] = row[j * STRIDE];
        }
      }
    }
  };
  auto commit = [&](int buf) {
    if constexpr (KM && NCOL == 16) {
      km_store<CV6_BK>(bT_lds[buf], kk, nn0 / 16, brun.v[0], brun.v[1]);
    } else if constexpr (KM) {
      // 8 columns: one half of n-tile nn0 / 16
      km_store_half<CV6_BK>(bT_lds[buf], kk, nn0 / 16, (nn0 / 8) & 1,
                            brun.v[0]);
    } else {
#pragma unroll
      for (int j = 0; j < NCOL; ++j)
        bT_lds[buf][(nn0 + j) * (CV6_BK + CV6_PAD) + kk] = (short)breg[j];
    }
  };

  // The A fragment of step k+1 is loaded one step ahead, AFTER that
  // step's gather: vmcnt counts in issue order, so the commit waits for
  // the gather alone and the MFMAs never wait for a load issued in their
  // own step (loaded in place, A's wait also drained the gather just
  // issued in front of it).
  auto load_a = [&](int mi, int k0) {
    return *reinterpret_cast<const uint4*>(wrow[mi] + k0 + 8 * (lane >> 4));
  };
  // rows past OC are zeroed at use, so the load is not waited for here
  auto use_a = [&](int mi, uint4 av) {
    if (!arow_ok[mi]) av = make_uint4(0, 0, 0, 0);
    return __builtin_bit_cast(bf16x8, av);
  };

  gather(0);
  uint4 a_next[MI];
#pragma unroll
  for (int mi = 0; mi < MI; ++mi) a_next[mi] = load_a(mi, 0);
  commit(0);
  int cur = 0;
  for (int k0 = 0; k0 < K; k0 += CV6_BK) {
    __syncthreads();
    bf16x8 a[MI];
#pragma unroll
    for (int mi = 0; mi < MI; ++mi) a[mi] = use_a(mi, a_next[mi]);
    if (k0 + CV6_BK < K) {
      gather(k0 + CV6_BK);
#pragma unroll
      for (int mi = 0; mi < MI; ++mi) a_next[mi] = load_a(mi, k0 + CV6_BK);
    }
    // one B fragment read per n-tile feeds the wave's MI MFMAs
#pragma unroll
    for (int nt = 0; nt < NTW; ++nt) {
      bf16x8 b;
      if constexpr (KM)
        b = km_frag<CV6_BK>(bT_lds[cur], foff_lo, foff_hi, nt, 0);
      else
        b = *reinterpret_cast<const bf16x8*>(
            &bT_lds[cur][(nt * 16 + (lane & 15)) * (CV6_BK + CV6_PAD)
                         + 8 * (lane >> 4)]);
#pragma unroll
      for (int mi = 0; mi < MI; ++mi)
        acc[mi][nt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
            a[mi], b, acc[mi][nt], 0, 0, 0);
    }
    if (k0 + CV6_BK < K) commit(cur ^ 1);
    cur ^= 1;
  }

#pragma unroll
  for (int mi = 0; mi < MI; ++mi) {
#pragma unroll
    for (int nt = 0; nt < NTW; ++nt) {
      int n = n0 + nt * 16 + (lane & 15);
      if (n >= N) continue;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        int m = m0 + wrow0 + mi * 16 + (lane >> 4) * 4 + r;
        if (m < g.OC)
          yc[(int64_t)m * N + n] = from_f32<__hip_bfloat16>(acc[mi][nt][r]);
      }
    }
  }
}

// ---------------------------------------------------------------------------
// fwd v7: BK=64 — two MFMA sub-steps per barrier (16 MFMAs/wave/step,
// amortising the stage/barrier latency the BK=32 pipeline pays every
// 8 MFMAs; cdna_hip_programming.md: BK 32->64 = +7..16% on the dense
// GEMM ladder), with s_setprio(1) around the MFMA cluster (T5).
// Requires K % 64 == 0 (IC a multiple of 64); launcher falls back to
// v6 otherwise.  KM as in fwd v6: a thread's 32 columns are two n-tiles,
// four ds_write_b128.  TILE as in fwd v6: on the 128x64 block a thread
// gathers 16 columns, one n-tile, in sub-rows of min(OW, 16).
template <int LG_OW_T, int STRIDE, bool KM = false, int TILE = 0>
__global__ __launch_bounds__(CONV_THREADS)
__attribute__((amdgpu_waves_per_eu(4, 4))) void k_conv3x3_fwd_v7(
    const __hip_bfloat16* __restrict__ xp, const __hip_bfloat16* __restrict__ w,
    __hip_bfloat16* __restrict__ y, ConvGeom6 g) {
  static_assert(!KM || STRIDE == 1, "k-major staging needs contiguous runs");
  constexpr int BK = 64;
  static_assert(TILE == 0 || TILE == 1, "64x128 or 128x64");
  constexpr int BM = TILE ? 128 : CV6_BM, BN = TILE ? 64 : CV6_BN;
  constexpr int MI = BM / 64;               // 16-row A fragments per wave
  constexpr int NTW = BN / 16;              // 16-column n-tiles per wave
  constexpr int NCOL = BN / 4;              // gathered columns per thread
  int c, tile;
  if (!xcd_remap6(blockIdx.x, g.C, g.tiles_m * g.tiles_n, c, tile)) return;
  const int mt = tile / g.tiles_n;
  const int m0 = mt * BM;
  const int n0 = (tile - mt * g.tiles_n) * BN;

  __shared__ __attribute__((aligned(16))) short
      bT_lds[2][BN * (KM ? BK : BK + CV6_PAD)];
  const int K = g.IC * 9;
  const int N = g.B * g.OH * g.OW;
  const int HpWp = g.Hp * g.Wp;
  const int64_t planeB = (int64_t)g.B * HpWp;
  const ushort* xc =
      reinterpret_cast<const ushort*>(xp) + (int64_t)c * g.IC * planeB;
  const __hip_bfloat16* wc = w + (int64_t)c * g.OC * K;
  __hip_bfloat16* yc = y + (int64_t)c * g.OC * N;

  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  // wave w owns rows m0 + 16*MI*w .. and all BN columns
  const int wrow0 = 16 * MI * wave;
  const __hip_bfloat16* wrow[MI];
  bool arow_ok[MI];
#pragma unroll
  for (int mi = 0; mi < MI; ++mi) {
    const int arow = m0 + wrow0 + mi * 16 + (lane & 15);
    wrow[mi] = wc + (int64_t)min(arow, g.OC - 1) * K;
    arow_ok[mi] = arow < g.OC;
  }

  f32x4 acc[MI][NTW];
#pragma unroll
  for (int mi = 0; mi < MI; ++mi)
#pragma unroll
    for (int i = 0; i < NTW; ++i) acc[mi][i] = {0.f, 0.f, 0.f, 0.f};

  const int kk = threadIdx.x & 63;            // staged k-row
  const int nn0 = (threadIdx.x >> 6) * NCOL;  // NCOL cols per thread
  ushort breg[NCOL];                          // !KM
  KmRun<NCOL> brun;                           // KM
  const int foff_lo = km_frag_off(lane, 0), foff_hi = km_frag_off(lane, 4);

  auto gather = [&](int k0) {
    const int k = k0 + kk;
    const int ic = k / 9, r = k - ic * 9;
    const int dh = r / 3, dw = r - dh * 3;
    const ushort* plane = xc + (int64_t)ic * planeB;
    constexpr int SUBW = (1 << LG_OW_T) < NCOL ? (1 << LG_OW_T) : NCOL;
    constexpr int NROW = NCOL / SUBW;
    static_assert(!KM || SUBW >= 8, "k-major runs are whole 8-column loads");
#pragma unroll
    for (int rr = 0; rr < NROW; ++rr) {
      int n = min(n0 + nn0 + rr * SUBW, N - 1);
      int b = n >> g.lg_ohw;
      int q = n & ((1 << g.lg_ohw) - 1);
      int oh = q >> g.lg_ow;
      int ow0 = q & ((1 << g.lg_ow) - 1);
      // sub-row segments are aligned; so is a whole-row run of exactly OW
      if (SUBW < NCOL || LG_OW_T < 5) ow0 = 0;
      else ow0 = min(ow0, g.OW - NCOL);
      const ushort* row = plane + (int64_t)b * HpWp
                          + (oh * STRIDE + dh) * g.Wp + ow0 * STRIDE + dw;
      if constexpr (KM) {
#pragma unroll
        for (int j = 0; j < SUBW / 8; ++j)
          brun.load8(rr * (SUBW / 8) + j, row + 8 * j);
      } else {
#pragma unroll
        for (int j = 0; j < SUBW; ++j)
          breg[rr * SUBW + j] = row[j * STRIDE];
      }
    }
  };
  auto commit = [&](int buf) {
    if constexpr (KM) {
#pragma unroll
      for (int j = 0; j < NCOL / 16; ++j)
        km_store<BK>(bT_lds[buf], kk, nn0 / 16 + j, brun.v[2 * j],
                     brun.v[2 * j + 1]);
    } else {
#pragma unroll
      for (int j = 0; j < NCOL; ++j)
        bT_lds[buf][(nn0 + j) * (BK + CV6_PAD) + kk] = (short)breg[j];
    }
  };

  // A one step ahead and after the gather, as in fwd v6
  auto load_a = [&](int mi, int k0, int sub) {
    return *reinterpret_cast<const uint4*>(
        wrow[mi] + k0 + sub * 32 + 8 * (lane >> 4));
  };
  // rows past OC are zeroed at use, so the load is not waited for here
  auto use_a = [&](int mi, uint4 av) {
    if (!arow_ok[mi]) av = make_uint4(0, 0, 0, 0);
    return __builtin_bit_cast(bf16x8, av);
  };

  struct AStep { uint4 v[MI][2]; };         // [fragment][K half]
  gather(0);
  AStep a_next;
#pragma unroll
  for (int mi = 0; mi < MI; ++mi) {
    a_next.v[mi][0] = load_a(mi, 0, 0);
    a_next.v[mi][1] = load_a(mi, 0, 1);
  }
  commit(0);
  int cur = 0;
  for (int k0 = 0; k0 < K; k0 += BK) {
    __syncthreads();
    const AStep a_cur = a_next;
    if (k0 + BK < K) {
      gather(k0 + BK);
#pragma unroll
      for (int mi = 0; mi < MI; ++mi) {
        a_next.v[mi][0] = load_a(mi, k0 + BK, 0);
        a_next.v[mi][1] = load_a(mi, k0 + BK, 1);
      }
    }
    __builtin_amdgcn_s_setprio(1);
#pragma unroll
    for (int sub = 0; sub < 2; ++sub) {
      bf16x8 a[MI];
#pragma unroll
      for (int mi = 0; mi < MI; ++mi) a[mi] = use_a(mi, a_cur.v[mi][sub]);
      // one B fragment read per n-tile feeds the wave's MI MFMAs
#pragma unroll
      for (int nt = 0; nt < NTW; ++nt) {
        bf16x8 b;
        if constexpr (KM)
          b = km_frag<BK>(bT_lds[cur], foff_lo, foff_hi, nt, sub * 32);
        else
          b = *reinterpret_cast<const bf16x8*>(
              &bT_lds[cur][(nt * 16 + (lane & 15)) * (BK + CV6_PAD)
                           + sub * 32 + 8 * (lane >> 4)]);
#pragma unroll
        for (int mi = 0; mi < MI; ++mi)
          acc[mi][nt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
              a[mi], b, acc[mi][nt], 0, 0, 0);
      }
    }
    __builtin_amdgcn_s_setprio(0);
    if (k0 + BK < K) commit(cur ^ 1);
    cur ^= 1;
  }

#pragma unroll
  for (int mi = 0; mi < MI; ++mi) {
#pragma unroll
    for (int nt = 0; nt < NTW; ++nt) {
      int n = n0 + nt * 16 + (lane & 15);
      if (n >= N) continue;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        int m = m0 + wrow0 + mi * 16 + (lane >> 4) * 4 + r;
        if (m < g.OC)
          yc[(int64_t)m * N + n] = from_f32<__hip_bfloat16>(acc[mi][nt][r]);
      }
    }
  }
}

// ---------------------------------------------------------------------------
// dgrad v6 (stride 1): dX[ic][n] over K=(oc,dh,dw), with the weight
// flip folded into the A staging (A[ic][k] = W[oc][ic][8-(3dh+dw)]) —
// no host-side weight transform, W is read once through L2.
// B gather = fwd's padded gather over dy_pad (output plane = H,W of dX).
// KM: k-major B tile as in fwd v6; the A staging is the same either way.
template <int LG_OW_T, bool KM = false>
__global__ __launch_bounds__(CONV_THREADS)
__attribute__((amdgpu_waves_per_eu(4, 4))) void k_conv3x3_dgrad_v6(
    const __hip_bfloat16* __restrict__ dyp, const __hip_bfloat16* __restrict__ w,
    __hip_bfloat16* __restrict__ dx, ConvGeom6 g) {
  // geometry: OH/OW here are dX's plane (the gather output), Hp/Wp the
  // padded dy plane; IC = output rows (dX channels), OC = contracted.
  int c, tile;
  if (!xcd_remap6(blockIdx.x, g.C, g.tiles_m * g.tiles_n, c, tile)) return;
  const int mt = tile / g.tiles_n;
  const int m0 = mt * CV6_BM;
  const int n0 = (tile - mt * g.tiles_n) * CV6_BN;

  __shared__ __attribute__((aligned(16))) short a_lds[2][CV6_BM * CV6_BK];
  __shared__ __attribute__((aligned(16))) short
      bT_lds[2][CV6_BN * (KM ? CV6_BK : CV6_BK + CV6_PAD)];
  const int K = g.OC * 9;
  const int N = g.B * g.OH * g.OW;
  const int HpWp = g.Hp * g.Wp;
  const int64_t planeB = (int64_t)g.B * HpWp;
  const ushort* dyc =
      reinterpret_cast<const ushort*>(dyp) + (int64_t)c * g.OC * planeB;
  const ushort* wc =
      reinterpret_cast<const ushort*>(w) + (int64_t)c * g.OC * g.IC * 9;
  __hip_bfloat16* dxc = dx + (int64_t)c * g.IC * N;

  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  f32x4 acc[CV6_BN / 16];
#pragma unroll
  for (int i = 0; i < CV6_BN / 16; ++i) acc[i] = {0.f, 0.f, 0.f, 0.f};

  const int kk = threadIdx.x % CV6_BK;
  const int nn0 = (threadIdx.x / CV6_BK) * (CV6_BN / 8);
  const int amm = threadIdx.x / 4;              // A row (ic) staged
  const int ak0 = (threadIdx.x % 4) * 8;
  const int aic = min(m0 + amm, g.IC - 1);
  const bool aic_ok = (m0 + amm) < g.IC;
  ushort breg[CV6_BN / 8];                      // !KM
  KmRun<CV6_BN / 8> brun;                       // KM
  const int foff_lo = km_frag_off(lane, 0), foff_hi = km_frag_off(lane, 4);
  ushort areg[8];

  auto gather = [&](int k0) {
    {
      // A: 8 consecutive k = (oc, 3dh+dw); flip index 8-(3dh+dw) walks
      // backwards inside each oc's contiguous 9-element block
      const int kb = k0 + ak0;
      int oc0 = kb / 9;
      int r0 = kb - oc0 * 9;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        int rr = r0 + j;
        int oc = oc0 + (rr >= 9);
        rr -= (rr >= 9) ? 9 : 0;
        ushort v = wc[((int64_t)oc * g.IC + aic) * 9 + (8 - rr)];
        areg[j] = aic_ok ? v : (ushort)0;
      }
    }
    {
      const int k = k0 + kk;
      const int oc = k / 9, r = k - oc * 9;
      const int dh = r / 3, dw = r - dh * 3;
      const ushort* plane = dyc + (int64_t)oc * planeB;
      if (LG_OW_T >= 4) {
        int n = min(n0 + nn0, N - 1);
        int b = n >> g.lg_ohw;
        int q = n & ((1 << g.lg_ohw) - 1);
        int oh = q >> g.lg_ow;
        int ow0 = min(q & ((1 << g.lg_ow) - 1), g.OW - CV6_BN / 8);
        const ushort* row = plane + (int64_t)b * HpWp + (oh + dh) * g.Wp
                            + ow0 + dw;
        if constexpr (KM) {
          brun.load8(0, row);
          brun.load8(1, row + 8);
        } else {
#pragma unroll
          for (int j = 0; j < CV6_BN / 8; ++j) breg[j] = row[j];
        }
      } else {
        constexpr int SUBW = 1 << LG_OW_T;
        constexpr int NROW = (CV6_BN / 8) / SUBW;
#pragma unroll
        for (int rr = 0; rr < NROW; ++rr) {
          int n = min(n0 + nn0 + rr * SUBW, N - 1);
          int b = n >> g.lg_ohw;
          int q = n & ((1 << g.lg_ohw) - 1);
          int oh = q >> LG_OW_T;
          const ushort* row = plane + (int64_t)b * HpWp + (oh + dh) * g.Wp + dw;
          if constexpr (KM) {
            if (SUBW == 8) brun.load8(rr, row);
            else brun.load4(rr, row);
          } else {
#pragma unroll
            for (int j = 0; j < SUBW; ++j) breg[rr * SUBW + j] = row[j];
          }
        }
      }
    }
  };
  auto commit = [&](int buf) {
#pragma unroll
    for (int j = 0; j < 8; ++j)
      a_lds[buf][amm * CV6_BK + ak0 + j] = (short)areg[j];
    if constexpr (KM) {
      km_store<CV6_BK>(bT_lds[buf], kk, nn0 / 16, brun.v[0], brun.v[1]);
    } else {
#pragma unroll
      for (int j = 0; j < CV6_BN / 8; ++j)
        bT_lds[buf][(nn0 + j) * (CV6_BK + CV6_PAD) + kk] = (short)breg[j];
    }
  };

  gather(0);
  commit(0);
  int cur = 0;
  for (int k0 = 0; k0 < K; k0 += CV6_BK) {
    __syncthreads();
    if (k0 + CV6_BK < K) gather(k0 + CV6_BK);
    bf16x8 a = *reinterpret_cast<const bf16x8*>(
        &a_lds[cur][(wave * 16 + (lane & 15)) * CV6_BK + 8 * (lane >> 4)]);
#pragma unroll
    for (int nt = 0; nt < CV6_BN / 16; ++nt) {
      bf16x8 b;
      if constexpr (KM)
        b = km_frag<CV6_BK>(bT_lds[cur], foff_lo, foff_hi, nt, 0);
      else
        b = *reinterpret_cast<const bf16x8*>(
            &bT_lds[cur][(nt * 16 + (lane & 15)) * (CV6_BK + CV6_PAD)
                         + 8 * (lane >> 4)]);
      acc[nt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, acc[nt], 0, 0, 0);
    }
    if (k0 + CV6_BK < K) commit(cur ^ 1);
    cur ^= 1;
  }

#pragma unroll
  for (int nt = 0; nt < CV6_BN / 16; ++nt) {
    int n = n0 + nt * 16 + (lane & 15);
    if (n >= N) continue;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      int m = m0 + wave * 16 + (lane >> 4) * 4 + r;
      if (m < g.IC)
        dxc[(int64_t)m * N + n] = from_f32<__hip_bfloat16>(acc[nt][r]);
    }
  }
}

// ---------------------------------------------------------------------------
// dgrad/wgrad v7: BK=64 (two MFMA sub-steps per barrier) — the fwd v7
// structure applied to the backward pipelines.  MEASURED NEUTRAL
// (dgrad, +9% only at s1d) to NEGATIVE (wgrad -5..-10%: the 37 KB LDS
// halves residency); kept env-gated (OLSIM_CONV_DW64=1) as the A/B
// record — gpurun_out/dw64.log vs v8_fwd.log baseline columns.
template <int LG_OW_T>
__global__ __launch_bounds__(CONV_THREADS) void k_conv3x3_dgrad_v7(
    const __hip_bfloat16* __restrict__ dyp, const __hip_bfloat16* __restrict__ w,
    __hip_bfloat16* __restrict__ dx, ConvGeom6 g) {
  constexpr int BK = 64;
  int c, tile;
  if (!xcd_remap6(blockIdx.x, g.C, g.tiles_m * g.tiles_n, c, tile)) return;
  const int mt = tile / g.tiles_n;
  const int m0 = mt * CV6_BM;
  const int n0 = (tile - mt * g.tiles_n) * CV6_BN;

  __shared__ short a_lds[2][CV6_BM * BK];
  __shared__ short bT_lds[2][CV6_BN * (BK + CV6_PAD)];
  const int K = g.OC * 9;
  const int N = g.B * g.OH * g.OW;
  const int HpWp = g.Hp * g.Wp;
  const int64_t planeB = (int64_t)g.B * HpWp;
  const ushort* dyc =
      reinterpret_cast<const ushort*>(dyp) + (int64_t)c * g.OC * planeB;
  const ushort* wc =
      reinterpret_cast<const ushort*>(w) + (int64_t)c * g.OC * g.IC * 9;
  __hip_bfloat16* dxc = dx + (int64_t)c * g.IC * N;

  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  f32x4 acc[CV6_BN / 16];
#pragma unroll
  for (int i = 0; i < CV6_BN / 16; ++i) acc[i] = {0.f, 0.f, 0.f, 0.f};

  const int kk = threadIdx.x & 63;            // B k-row
  const int nn0 = (threadIdx.x >> 6) * 32;    // 32 cols / thread
  const int amm = threadIdx.x / 4;            // A row (ic)
  const int ak0 = (threadIdx.x % 4) * 16;     // 16 k / thread
  const int aic = min(m0 + amm, g.IC - 1);
  const bool aic_ok = (m0 + amm) < g.IC;
  ushort breg[32];
  ushort areg[16];

  auto gather = [&](int k0) {
    {
      const int kb = k0 + ak0;
      int oc0 = kb / 9;
      int r0 = kb - oc0 * 9;
#pragma unroll
      for (int j = 0; j < 16; ++j) {
        int rr = r0 + j;
        int carry = (rr >= 18) ? 2 : (rr >= 9 ? 1 : 0);
        int oc = oc0 + carry;
        rr -= 9 * carry;
        ushort v = wc[((int64_t)oc * g.IC + aic) * 9 + (8 - rr)];
        areg[j] = aic_ok ? v : (ushort)0;
      }
    }
    {
      const int k = k0 + kk;
      const int oc = k / 9, r = k - oc * 9;
      const int dh = r / 3, dw = r - dh * 3;
      const ushort* plane = dyc + (int64_t)oc * planeB;
      constexpr int SUBW = 1 << (LG_OW_T < 5 ? LG_OW_T : 5);
      constexpr int NROW = 32 / SUBW;
#pragma unroll
      for (int rr = 0; rr < NROW; ++rr) {
        int n = min(n0 + nn0 + rr * SUBW, N - 1);
        int b = n >> g.lg_ohw;
        int q = n & ((1 << g.lg_ohw) - 1);
        int oh = q >> g.lg_ow;
        int ow0 = q & ((1 << g.lg_ow) - 1);
        if (SUBW < 32) ow0 = 0;
        else ow0 = min(ow0, g.OW - 32);
        const ushort* row = plane + (int64_t)b * HpWp + (oh + dh) * g.Wp
                            + ow0 + dw;
#pragma unroll
        for (int j = 0; j < SUBW; ++j) breg[rr * SUBW + j] = row[j];
      }
    }
  };
  auto commit = [&](int buf) {
#pragma unroll
    for (int j = 0; j < 16; ++j)
      a_lds[buf][amm * BK + ak0 + j] = (short)areg[j];
#pragma unroll
    for (int j = 0; j < 32; ++j)
      bT_lds[buf][(nn0 + j) * (BK + CV6_PAD) + kk] = (short)breg[j];
  };

  gather(0);
  commit(0);
  int cur = 0;
  for (int k0 = 0; k0 < K; k0 += BK) {
    __syncthreads();
    if (k0 + BK < K) gather(k0 + BK);
    __builtin_amdgcn_s_setprio(1);
#pragma unroll
    for (int sub = 0; sub < 2; ++sub) {
      bf16x8 a = *reinterpret_cast<const bf16x8*>(
          &a_lds[cur][(wave * 16 + (lane & 15)) * BK + sub * 32
                      + 8 * (lane >> 4)]);
#pragma unroll
      for (int nt = 0; nt < CV6_BN / 16; ++nt) {
        bf16x8 b = *reinterpret_cast<const bf16x8*>(
            &bT_lds[cur][(nt * 16 + (lane & 15)) * (BK + CV6_PAD)
                         + sub * 32 + 8 * (lane >> 4)]);
        acc[nt] =
            __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, acc[nt], 0, 0, 0);
      }
    }
    __builtin_amdgcn_s_setprio(0);
    if (k0 + BK < K) commit(cur ^ 1);
    cur ^= 1;
  }

#pragma unroll
  for (int nt = 0; nt < CV6_BN / 16; ++nt) {
    int n = n0 + nt * 16 + (lane & 15);
    if (n >= N) continue;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      int m = m0 + wave * 16 + (lane >> 4) * 4 + r;
      if (m < g.IC)
        dxc[(int64_t)m * N + n] = from_f32<__hip_bfloat16>(acc[nt][r]);
    }
  }
}

// ---------------------------------------------------------------------------
// dgrad stride 2, parity-decomposed: one launch per class (HE, WE).
// Output positions (2i+HE, 2j+WE); valid taps dh with (HE+dh-1) even:
// HE=0 -> {1}, HE=1 -> {0,2} (same for WE/dw).  Class-k = (oc, th, tw)
// over K = OC*NH*NW (NH,NW in {1,2}); the dy read offset is
// (i + (HE+dh-1)/2, j + (WE+dw-1)/2) into the padded dy plane.
// Class output plane = OH x OW (= dy's plane: H/2 x W/2).
template <int HE, int WE, int LG_OW_T>
__global__ __launch_bounds__(CONV_THREADS) void k_conv3x3_dgrad_s2(
    const __hip_bfloat16* __restrict__ dyp, const __hip_bfloat16* __restrict__ w,
    __hip_bfloat16* __restrict__ dx, ConvGeom6 g) {
  constexpr int NH = HE ? 2 : 1;
  constexpr int NW = WE ? 2 : 1;
  constexpr int NT = NH * NW;
  // valid dh per class (flip index uses 2-dh); delta = (HE+dh-1)/2
  constexpr int DH0 = HE ? 0 : 1;     // first valid dh
  constexpr int DW0 = WE ? 0 : 1;
  int c, tile;
  if (!xcd_remap6(blockIdx.x, g.C, g.tiles_m * g.tiles_n, c, tile)) return;
  const int mt = tile / g.tiles_n;
  const int m0 = mt * CV6_BM;
  const int n0 = (tile - mt * g.tiles_n) * CV6_BN;

  __shared__ short a_lds[2][CV6_BM * CV6_BK];
  __shared__ short bT_lds[2][CV6_BN * (CV6_BK + CV6_PAD)];
  const int K = g.OC * NT;
  const int N = g.B * g.OH * g.OW;          // class grid = dy plane
  const int HpWp = g.Hp * g.Wp;
  const int64_t planeB = (int64_t)g.B * HpWp;
  const ushort* dyc =
      reinterpret_cast<const ushort*>(dyp) + (int64_t)c * g.OC * planeB;
  const ushort* wc =
      reinterpret_cast<const ushort*>(w) + (int64_t)c * g.OC * g.IC * 9;
  const int H = 2 * g.OH, W = 2 * g.OW;     // dX plane
  __hip_bfloat16* dxc = dx + (int64_t)c * g.IC * g.B * H * W;

  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  f32x4 acc[CV6_BN / 16];
#pragma unroll
  for (int i = 0; i < CV6_BN / 16; ++i) acc[i] = {0.f, 0.f, 0.f, 0.f};

  const int kk = threadIdx.x % CV6_BK;
  const int nn0 = (threadIdx.x / CV6_BK) * (CV6_BN / 8);
  const int amm = threadIdx.x / 4;
  const int ak0 = (threadIdx.x % 4) * 8;
  const int aic = min(m0 + amm, g.IC - 1);
  const bool aic_ok = (m0 + amm) < g.IC;
  ushort breg[CV6_BN / 8];
  ushort areg[8];

  auto gather = [&](int k0) {
    {
      // A[ic][k=(oc,th,tw)] = W[oc][ic][(2-dh)*3+(2-dw)],
      // dh = DH0 + 2*th, dw = DW0 + 2*tw
      const int kb = k0 + ak0;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        int k = kb + j;
        int oc = k / NT;                    // NT pow2: shift
        int ti = k - oc * NT;
        int th = NW == 2 ? (ti >> 1) : ti;  // ti = th*NW + tw
        int tw = NW == 2 ? (ti & 1) : 0;
        int dh = DH0 + 2 * th;
        int dw = DW0 + 2 * tw;
        ushort v = wc[((int64_t)oc * g.IC + aic) * 9 + (2 - dh) * 3 + (2 - dw)];
        areg[j] = aic_ok ? v : (ushort)0;
      }
    }
    {
      const int k = k0 + kk;
      const int oc = k / NT;
      const int ti = k - oc * NT;
      const int th = NW == 2 ? (ti >> 1) : ti;
      const int tw = NW == 2 ? (ti & 1) : 0;
      const int dh = DH0 + 2 * th;
      const int dw = DW0 + 2 * tw;
      const int deh = (HE + dh - 1) >> 1;   // dy row offset (0 or 1)
      const int dew = (WE + dw - 1) >> 1;
      const ushort* plane = dyc + (int64_t)oc * planeB;
      if (LG_OW_T >= 4) {
        int n = min(n0 + nn0, N - 1);
        int b = n >> g.lg_ohw;
        int q = n & ((1 << g.lg_ohw) - 1);
        int i = q >> g.lg_ow;
        int j0 = min(q & ((1 << g.lg_ow) - 1), g.OW - CV6_BN / 8);
        const ushort* row = plane + (int64_t)b * HpWp + (i + deh + 1) * g.Wp
                            + j0 + dew + 1;
#pragma unroll
        for (int j = 0; j < CV6_BN / 8; ++j) breg[j] = row[j];
      } else {
        constexpr int SUBW = 1 << LG_OW_T;
        constexpr int NROW = (CV6_BN / 8) / SUBW;
#pragma unroll
        for (int rr = 0; rr < NROW; ++rr) {
          int n = min(n0 + nn0 + rr * SUBW, N - 1);
          int b = n >> g.lg_ohw;
          int q = n & ((1 << g.lg_ohw) - 1);
          int i = q >> LG_OW_T;
          const ushort* row = plane + (int64_t)b * HpWp
                              + (i + deh + 1) * g.Wp + dew + 1;
#pragma unroll
          for (int j = 0; j < SUBW; ++j) breg[rr * SUBW + j] = row[j];
        }
      }
    }
  };
  auto commit = [&](int buf) {
#pragma unroll
    for (int j = 0; j < 8; ++j)
      a_lds[buf][amm * CV6_BK + ak0 + j] = (short)areg[j];
#pragma unroll
    for (int j = 0; j < CV6_BN / 8; ++j)
      bT_lds[buf][(nn0 + j) * (CV6_BK + CV6_PAD) + kk] = (short)breg[j];
  };

  gather(0);
  commit(0);
  int cur = 0;
  for (int k0 = 0; k0 < K; k0 += CV6_BK) {
    __syncthreads();
    if (k0 + CV6_BK < K) gather(k0 + CV6_BK);
    bf16x8 a = *reinterpret_cast<const bf16x8*>(
        &a_lds[cur][(wave * 16 + (lane & 15)) * CV6_BK + 8 * (lane >> 4)]);
#pragma unroll
    for (int nt = 0; nt < CV6_BN / 16; ++nt) {
      bf16x8 b = *reinterpret_cast<const bf16x8*>(
          &bT_lds[cur][(nt * 16 + (lane & 15)) * (CV6_BK + CV6_PAD)
                       + 8 * (lane >> 4)]);
      acc[nt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, acc[nt], 0, 0, 0);
    }
    if (k0 + CV6_BK < K) commit(cur ^ 1);
    cur ^= 1;
  }

  // scatter back to the strided class positions (2i+HE, 2j+WE)
#pragma unroll
  for (int nt = 0; nt < CV6_BN / 16; ++nt) {
    int n = n0 + nt * 16 + (lane & 15);
    if (n >= N) continue;
    int b = n >> g.lg_ohw;
    int q = n & ((1 << g.lg_ohw) - 1);
    int i = q >> g.lg_ow;
    int j = q & ((1 << g.lg_ow) - 1);
    int64_t base = ((int64_t)b * H + 2 * i + HE) * W + 2 * j + WE;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      int m = m0 + wave * 16 + (lane >> 4) * 4 + r;
      if (m < g.IC)
        dxc[(int64_t)m * g.B * H * W + base] =
            from_f32<__hip_bfloat16>(acc[nt][r]);
    }
  }
}

// ---------------------------------------------------------------------------
// wgrad v6: dW[oc][k9] = sum_q dY[oc][q] * P[k9][q]; A = dY rows direct
// from global (unpadded, contiguous); B = patch gather from x_pad with
// the per-column offsets (ic*B*HpWp + dh*Wp + dw) hoisted out of the
// q-loop entirely — per step only the (b,oh,ow) base changes.
__global__ __launch_bounds__(CONV_THREADS) void k_conv3x3_wgrad_v6(
    const __hip_bfloat16* __restrict__ xp, const __hip_bfloat16* __restrict__ dy,
    __hip_bfloat16* __restrict__ dw, ConvGeom6 g) {
  int c, tile;
  if (!xcd_remap6(blockIdx.x, g.C, g.tiles_m * g.tiles_n, c, tile)) return;
  const int mt = tile / g.tiles_n;
  const int m0 = mt * CV6_BM;                  // over OC
  const int n0 = (tile - mt * g.tiles_n) * CV6_BN;   // over IC*9
  __shared__ short bT_lds[2][CV6_BN * (CV6_PAD + CV6_BK)];
  const int K9 = g.IC * 9;
  const int NN = g.B * g.OH * g.OW;            // reduction
  const int HpWp = g.Hp * g.Wp;
  const int64_t planeB = (int64_t)g.B * HpWp;
  const ushort* xc =
      reinterpret_cast<const ushort*>(xp) + (int64_t)c * g.IC * planeB;
  const __hip_bfloat16* dyc = dy + (int64_t)c * g.OC * NN;
  __hip_bfloat16* dwc = dw + (int64_t)c * g.OC * K9;

  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int arow = m0 + wave * 16 + (lane & 15);
  const __hip_bfloat16* dyrow = dyc + (int64_t)min(arow, g.OC - 1) * NN;
  const bool arow_ok = arow < g.OC;

  f32x4 acc[CV6_BN / 16];
#pragma unroll
  for (int i = 0; i < CV6_BN / 16; ++i) acc[i] = {0.f, 0.f, 0.f, 0.f};

  const int qq = threadIdx.x % CV6_BK;
  const int nn0 = (threadIdx.x / CV6_BK) * (CV6_BN / 8);
  ushort breg[CV6_BN / 8];

  // per-column gather offsets: off[j] = ic*B*HpWp + dh*Wp + dw (clamped
  // duplicates for the K9 tail; outputs there are write-masked)
  int64_t off[CV6_BN / 8];
#pragma unroll
  for (int j = 0; j < CV6_BN / 8; ++j) {
    int k = min(n0 + nn0 + j, K9 - 1);
    int ic = k / 9, r = k - ic * 9;
    int dh = r / 3, dw2 = r - dh * 3;
    off[j] = (int64_t)ic * planeB + dh * g.Wp + dw2;
  }

  auto gather = [&](int q0) {
    int q = min(q0 + qq, NN - 1);
    int b = q >> g.lg_ohw;
    int p = q & ((1 << g.lg_ohw) - 1);
    int oh = p >> g.lg_ow;
    int ow = p & ((1 << g.lg_ow) - 1);
    const ushort* base = xc + (int64_t)b * HpWp
                         + (oh * g.stride) * g.Wp + ow * g.stride;
#pragma unroll
    for (int j = 0; j < CV6_BN / 8; ++j) breg[j] = base[off[j]];
  };
  auto commit = [&](int buf) {
#pragma unroll
    for (int j = 0; j < CV6_BN / 8; ++j)
      bT_lds[buf][(nn0 + j) * (CV6_BK + CV6_PAD) + qq] = (short)breg[j];
  };

  gather(0);
  commit(0);
  int cur = 0;
  for (int q0 = 0; q0 < NN; q0 += CV6_BK) {
    __syncthreads();
    if (q0 + CV6_BK < NN) gather(q0 + CV6_BK);
    bf16x8 a;
    {
      uint4 av = *reinterpret_cast<const uint4*>(dyrow + q0 + 8 * (lane >> 4));
      a = *reinterpret_cast<const bf16x8*>(&av);
      if (!arow_ok) {
#pragma unroll
        for (int e = 0; e < 8; ++e) a[e] = 0;
      }
    }
#pragma unroll
    for (int nt = 0; nt < CV6_BN / 16; ++nt) {
      bf16x8 b = *reinterpret_cast<const bf16x8*>(
          &bT_lds[cur][(nt * 16 + (lane & 15)) * (CV6_BK + CV6_PAD)
                       + 8 * (lane >> 4)]);
      acc[nt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, acc[nt], 0, 0, 0);
    }
    if (q0 + CV6_BK < NN) commit(cur ^ 1);
    cur ^= 1;
  }

#pragma unroll
  for (int nt = 0; nt < CV6_BN / 16; ++nt) {
    int k = n0 + nt * 16 + (lane & 15);
    if (k >= K9) continue;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      int m = m0 + wave * 16 + (lane >> 4) * 4 + r;
      if (m < g.OC)
        dwc[(int64_t)m * K9 + k] = __float2bfloat16(acc[nt][r]);
    }
  }
}


// ---------------------------------------------------------------------------
// wgrad v8 (stride 1): run-vectorised B gather.  PMC on v6
// (profiles/pmc_final_r02.md): 19% VALU + 26% instruction-wait, MFMA
// busy only 18% — the producer's 16 scalar u16 loads + 16 ds_write_b16
// per thread per step dominate the instruction stream.  Here one
// producer item owns a (ic, dh) "run" x 8 consecutive q: 8 consecutive
// stride-1 q positions stay inside one padded row, so THREE 8-byte
// loads cover the 10 u16 needed for all three dw columns, extracted
// branchlessly (E is always even: Wp, HpWp, planeB and ow are even)
// and committed as one ds_write_b128 per column.
__global__ __launch_bounds__(CONV_THREADS) void k_conv3x3_wgrad_v8(
    const __hip_bfloat16* __restrict__ xp, const __hip_bfloat16* __restrict__ dy,
    __hip_bfloat16* __restrict__ dw, ConvGeom6 g) {
  int c, tile;
  if (!xcd_remap6(blockIdx.x, g.C, g.tiles_m * g.tiles_n, c, tile)) return;
  const int mt = tile / g.tiles_n;
  const int m0 = mt * CV6_BM;                  // over OC
  const int n0 = (tile - mt * g.tiles_n) * CV6_BN;   // over IC*9
  __shared__ short bT_lds[2][CV6_BN * (CV6_PAD + CV6_BK)];
  const int K9 = g.IC * 9;
  const int NN = g.B * g.OH * g.OW;            // reduction
  const int HpWp = g.Hp * g.Wp;
  const int64_t planeB = (int64_t)g.B * HpWp;
  const ushort* xc =
      reinterpret_cast<const ushort*>(xp) + (int64_t)c * g.IC * planeB;
  const __hip_bfloat16* dyc = dy + (int64_t)c * g.OC * NN;
  __hip_bfloat16* dwc = dw + (int64_t)c * g.OC * K9;

  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int arow = m0 + wave * 16 + (lane & 15);
  const __hip_bfloat16* dyrow = dyc + (int64_t)min(arow, g.OC - 1) * NN;
  const bool arow_ok = arow < g.OC;

  f32x4 acc[CV6_BN / 16];
#pragma unroll
  for (int i = 0; i < CV6_BN / 16; ++i) acc[i] = {0.f, 0.f, 0.f, 0.f};

  // producer item = (run, q-octet): run = (ic, dh) pair of the window
  const int runs_lo = n0 / 3;
  const int runs_hi = (min(n0 + CV6_BN, K9) + 2) / 3;
  const int nitems = (runs_hi - runs_lo) * (CV6_BK / 8);
  const bool prod = threadIdx.x < nitems;
  const int run = runs_lo + threadIdx.x / (CV6_BK / 8);
  const int qv = (threadIdx.x % (CV6_BK / 8)) * 8;
  const int ric = run / 3, rdh = run - ric * 3;
  const int64_t runoff = (int64_t)ric * planeB + rdh * g.Wp;

  uint2 r0, r1, r2;
  int tpar = 0;

  auto gather = [&](int q0) {
    if (!prod) return;
    const int q = q0 + qv;
    const int b = q >> g.lg_ohw;
    const int p = q & ((1 << g.lg_ohw) - 1);
    const int oh = p >> g.lg_ow;
    const int ow = p & ((1 << g.lg_ow) - 1);
    const int64_t E = runoff + (int64_t)b * HpWp + oh * g.Wp + ow;
    // clamp so the 12-u16 window never reads past the tensor (only the
    // final element of the final plane can clamp, by exactly 2)
    const int64_t E4 = min(E & ~3LL, (int64_t)g.IC * planeB - 12);
    tpar = (int)(E - E4) >> 1;               // 0 or 1 (E is even)
    const uint2* src = reinterpret_cast<const uint2*>(xc + E4);
    r0 = src[0];
    r1 = src[1];
    r2 = src[2];
  };
  auto commit = [&](int buf) {
    if (!prod) return;
    // s[k] = u32 of u16 elements (E + 2k, E + 2k + 1)
    uint32_t s[5];
    s[0] = tpar ? r0.y : r0.x;
    s[1] = tpar ? r1.x : r0.y;
    s[2] = tpar ? r1.y : r1.x;
    s[3] = tpar ? r2.x : r1.y;
    s[4] = tpar ? r2.y : r2.x;
#pragma unroll
    for (int dw2 = 0; dw2 < 3; ++dw2) {
      const int k9 = run * 3 + dw2;
      const int col = k9 - n0;
      if (col < 0 || col >= CV6_BN || k9 >= K9) continue;
      uint4 o;
      if (dw2 == 0) {
        o.x = s[0]; o.y = s[1]; o.z = s[2]; o.w = s[3];
      } else if (dw2 == 2) {
        o.x = s[1]; o.y = s[2]; o.z = s[3]; o.w = s[4];
      } else {
        o.x = __builtin_amdgcn_alignbit(s[1], s[0], 16);
        o.y = __builtin_amdgcn_alignbit(s[2], s[1], 16);
        o.z = __builtin_amdgcn_alignbit(s[3], s[2], 16);
        o.w = __builtin_amdgcn_alignbit(s[4], s[3], 16);
      }
      *reinterpret_cast<uint4*>(
          &bT_lds[buf][col * (CV6_BK + CV6_PAD) + qv]) = o;
    }
  };

  gather(0);
  commit(0);
  int cur = 0;
  for (int q0 = 0; q0 < NN; q0 += CV6_BK) {
    __syncthreads();
    if (q0 + CV6_BK < NN) gather(q0 + CV6_BK);
    bf16x8 a;
    {
      uint4 av = *reinterpret_cast<const uint4*>(dyrow + q0 + 8 * (lane >> 4));
      a = *reinterpret_cast<const bf16x8*>(&av);
      if (!arow_ok) {
#pragma unroll
        for (int e = 0; e < 8; ++e) a[e] = 0;
      }
    }
#pragma unroll
    for (int nt = 0; nt < CV6_BN / 16; ++nt) {
      bf16x8 b = *reinterpret_cast<const bf16x8*>(
          &bT_lds[cur][(nt * 16 + (lane & 15)) * (CV6_BK + CV6_PAD)
                       + 8 * (lane >> 4)]);
      acc[nt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, acc[nt], 0, 0, 0);
    }
    if (q0 + CV6_BK < NN) commit(cur ^ 1);
    cur ^= 1;
  }

#pragma unroll
  for (int nt = 0; nt < CV6_BN / 16; ++nt) {
    int k = n0 + nt * 16 + (lane & 15);
    if (k >= K9) continue;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      int m = m0 + wave * 16 + (lane >> 4) * 4 + r;
      if (m < g.OC)
        dwc[(int64_t)m * K9 + k] = __float2bfloat16(acc[nt][r]);
    }
  }
}


// wgrad v8s: run-vectorised producer for STRIDE 2 (OW >= 8).  Same
// item structure as v8, but the 8 q positions map to every-2nd input
// pixel, so the 3 dw columns need 17 consecutive u16 (5 8-byte loads)
// and the extraction picks alternate elements with constant-selector
// v_perm after one branchless word-shift.
__global__ __launch_bounds__(CONV_THREADS) void k_conv3x3_wgrad_v8s(
    const __hip_bfloat16* __restrict__ xp, const __hip_bfloat16* __restrict__ dy,
    __hip_bfloat16* __restrict__ dw, ConvGeom6 g) {
  int c, tile;
  if (!xcd_remap6(blockIdx.x, g.C, g.tiles_m * g.tiles_n, c, tile)) return;
  const int mt = tile / g.tiles_n;
  const int m0 = mt * CV6_BM;
  const int n0 = (tile - mt * g.tiles_n) * CV6_BN;
  __shared__ short bT_lds[2][CV6_BN * (CV6_PAD + CV6_BK)];
  const int K9 = g.IC * 9;
  const int NN = g.B * g.OH * g.OW;
  const int HpWp = g.Hp * g.Wp;
  const int64_t planeB = (int64_t)g.B * HpWp;
  const ushort* xc =
      reinterpret_cast<const ushort*>(xp) + (int64_t)c * g.IC * planeB;
  const __hip_bfloat16* dyc = dy + (int64_t)c * g.OC * NN;
  __hip_bfloat16* dwc = dw + (int64_t)c * g.OC * K9;

  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int arow = m0 + wave * 16 + (lane & 15);
  const __hip_bfloat16* dyrow = dyc + (int64_t)min(arow, g.OC - 1) * NN;
  const bool arow_ok = arow < g.OC;

  f32x4 acc[CV6_BN / 16];
#pragma unroll
  for (int i = 0; i < CV6_BN / 16; ++i) acc[i] = {0.f, 0.f, 0.f, 0.f};

  const int runs_lo = n0 / 3;
  const int runs_hi = (min(n0 + CV6_BN, K9) + 2) / 3;
  const int nitems = (runs_hi - runs_lo) * (CV6_BK / 8);
  const bool prod = threadIdx.x < nitems;
  const int run = runs_lo + threadIdx.x / (CV6_BK / 8);
  const int qv = (threadIdx.x % (CV6_BK / 8)) * 8;
  const int ric = run / 3, rdh = run - ric * 3;
  const int64_t runoff = (int64_t)ric * planeB + rdh * g.Wp;

  uint2 r0, r1, r2, r3, r4;
  int tpar = 0;

  auto gather = [&](int q0) {
    if (!prod) return;
    const int q = q0 + qv;
    const int b = q >> g.lg_ohw;
    const int p = q & ((1 << g.lg_ohw) - 1);
    const int oh = p >> g.lg_ow;
    const int ow = p & ((1 << g.lg_ow) - 1);
    const int64_t E = runoff + (int64_t)b * HpWp + (oh * 2) * g.Wp + ow * 2;
    const int64_t E4 = min(E & ~3LL, (int64_t)g.IC * planeB - 20);
    tpar = (int)(E - E4) >> 1;               // 0 or 1 (E is even)
    const uint2* src = reinterpret_cast<const uint2*>(xc + E4);
    r0 = src[0];
    r1 = src[1];
    r2 = src[2];
    r3 = src[3];
    r4 = src[4];
  };
  auto commit = [&](int buf) {
    if (!prod) return;
    uint32_t w[10] = {r0.x, r0.y, r1.x, r1.y, r2.x,
                      r2.y, r3.x, r3.y, r4.x, r4.y};
    // s[k] = u32 of u16 elements (E + 2k, E + 2k + 1), k 0..8
    uint32_t s[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) s[k] = tpar ? w[k + 1] : w[k];
    // col dw needs elements E + dw + 2j (j 0..7): alternate u16s
#pragma unroll
    for (int dw2 = 0; dw2 < 3; ++dw2) {
      const int k9 = run * 3 + dw2;
      const int col = k9 - n0;
      if (col < 0 || col >= CV6_BN || k9 >= K9) continue;
      // o[m] = (elem dw+4m, elem dw+4m+2); dw even -> lo16 halves of
      // s[dw/2+2m], s[dw/2+2m+1]; dw odd -> hi16 halves of s[2m], s[2m+1]
      const int b0 = (dw2 + 1) >> 1;   // 0, 0, 1 -> s-base per pair step
      const uint32_t sel = (dw2 & 1) ? 0x07060302u : 0x05040100u;
      const int base = (dw2 == 2) ? 1 : 0;
      uint4 o;
      o.x = __builtin_amdgcn_perm(s[base + 1], s[base + 0], sel);
      o.y = __builtin_amdgcn_perm(s[base + 3], s[base + 2], sel);
      o.z = __builtin_amdgcn_perm(s[base + 5], s[base + 4], sel);
      o.w = __builtin_amdgcn_perm(s[base + 7], s[base + 6], sel);
      (void)b0;
      *reinterpret_cast<uint4*>(
          &bT_lds[buf][col * (CV6_BK + CV6_PAD) + qv]) = o;
    }
  };

  gather(0);
  commit(0);
  int cur = 0;
  for (int q0 = 0; q0 < NN; q0 += CV6_BK) {
    __syncthreads();
    if (q0 + CV6_BK < NN) gather(q0 + CV6_BK);
    bf16x8 a;
    {
      uint4 av = *reinterpret_cast<const uint4*>(dyrow + q0 + 8 * (lane >> 4));
      a = *reinterpret_cast<const bf16x8*>(&av);
      if (!arow_ok) {
#pragma unroll
        for (int e = 0; e < 8; ++e) a[e] = 0;
      }
    }
#pragma unroll
    for (int nt = 0; nt < CV6_BN / 16; ++nt) {
      bf16x8 b = *reinterpret_cast<const bf16x8*>(
          &bT_lds[cur][(nt * 16 + (lane & 15)) * (CV6_BK + CV6_PAD)
                       + 8 * (lane >> 4)]);
      acc[nt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, acc[nt], 0, 0, 0);
    }
    if (q0 + CV6_BK < NN) commit(cur ^ 1);
    cur ^= 1;
  }

#pragma unroll
  for (int nt = 0; nt < CV6_BN / 16; ++nt) {
    int k = n0 + nt * 16 + (lane & 15);
    if (k >= K9) continue;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      int m = m0 + wave * 16 + (lane >> 4) * 4 + r;
      if (m < g.OC)
        dwc[(int64_t)m * K9 + k] = __float2bfloat16(acc[nt][r]);
    }
  }
}

// ---------------------------------------------------------------------------
// wgrad v7: BK=64 reduction steps (two MFMA sub-steps per barrier),
// int32 gather offsets.  Requires NN % 64 == 0.
__global__ __launch_bounds__(CONV_THREADS) void k_conv3x3_wgrad_v7(
    const __hip_bfloat16* __restrict__ xp, const __hip_bfloat16* __restrict__ dy,
    __hip_bfloat16* __restrict__ dw, ConvGeom6 g) {
  constexpr int BK = 64;
  int c, tile;
  if (!xcd_remap6(blockIdx.x, g.C, g.tiles_m * g.tiles_n, c, tile)) return;
  const int mt = tile / g.tiles_n;
  const int m0 = mt * CV6_BM;                  // over OC
  const int n0 = (tile - mt * g.tiles_n) * CV6_BN;   // over IC*9
  __shared__ short bT_lds[2][CV6_BN * (BK + CV6_PAD)];
  const int K9 = g.IC * 9;
  const int NN = g.B * g.OH * g.OW;            // reduction
  const int HpWp = g.Hp * g.Wp;
  const int64_t planeB = (int64_t)g.B * HpWp;
  const ushort* xc =
      reinterpret_cast<const ushort*>(xp) + (int64_t)c * g.IC * planeB;
  const __hip_bfloat16* dyc = dy + (int64_t)c * g.OC * NN;
  __hip_bfloat16* dwc = dw + (int64_t)c * g.OC * K9;

  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int arow = m0 + wave * 16 + (lane & 15);
  const __hip_bfloat16* dyrow = dyc + (int64_t)min(arow, g.OC - 1) * NN;
  const bool arow_ok = arow < g.OC;

  f32x4 acc[CV6_BN / 16];
#pragma unroll
  for (int i = 0; i < CV6_BN / 16; ++i) acc[i] = {0.f, 0.f, 0.f, 0.f};

  const int qq = threadIdx.x & 63;
  const int nn0 = (threadIdx.x >> 6) * 32;     // 32 K9-cols / thread
  ushort breg[32];

  int off[32];                                 // plane offsets fit int32
#pragma unroll
  for (int j = 0; j < 32; ++j) {
    int k = min(n0 + nn0 + j, K9 - 1);
    int ic = k / 9, r = k - ic * 9;
    int dh = r / 3, dw2 = r - dh * 3;
    off[j] = (int)((int64_t)ic * planeB + dh * g.Wp + dw2);
  }

  auto gather = [&](int q0) {
    int q = min(q0 + qq, NN - 1);
    int b = q >> g.lg_ohw;
    int p = q & ((1 << g.lg_ohw) - 1);
    int oh = p >> g.lg_ow;
    int ow = p & ((1 << g.lg_ow) - 1);
    const ushort* base = xc + (int64_t)b * HpWp
                         + (oh * g.stride) * g.Wp + ow * g.stride;
#pragma unroll
    for (int j = 0; j < 32; ++j) breg[j] = base[off[j]];
  };
  auto commit = [&](int buf) {
#pragma unroll
    for (int j = 0; j < 32; ++j)
      bT_lds[buf][(nn0 + j) * (BK + CV6_PAD) + qq] = (short)breg[j];
  };

  gather(0);
  commit(0);
  int cur = 0;
  for (int q0 = 0; q0 < NN; q0 += BK) {
    __syncthreads();
    if (q0 + BK < NN) gather(q0 + BK);
    __builtin_amdgcn_s_setprio(1);
#pragma unroll
    for (int sub = 0; sub < 2; ++sub) {
      bf16x8 a;
      {
        uint4 av = *reinterpret_cast<const uint4*>(
            dyrow + q0 + sub * 32 + 8 * (lane >> 4));
        a = *reinterpret_cast<const bf16x8*>(&av);
        if (!arow_ok) {
#pragma unroll
          for (int e = 0; e < 8; ++e) a[e] = 0;
        }
      }
#pragma unroll
      for (int nt = 0; nt < CV6_BN / 16; ++nt) {
        bf16x8 b = *reinterpret_cast<const bf16x8*>(
            &bT_lds[cur][(nt * 16 + (lane & 15)) * (BK + CV6_PAD)
                         + sub * 32 + 8 * (lane >> 4)]);
        acc[nt] =
            __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, acc[nt], 0, 0, 0);
      }
    }
    __builtin_amdgcn_s_setprio(0);
    if (q0 + BK < NN) commit(cur ^ 1);
    cur ^= 1;
  }

#pragma unroll
  for (int nt = 0; nt < CV6_BN / 16; ++nt) {
    int k = n0 + nt * 16 + (lane & 15);
    if (k >= K9) continue;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      int m = m0 + wave * 16 + (lane >> 4) * 4 + r;
      if (m < g.OC)
        dwc[(int64_t)m * K9 + k] = __float2bfloat16(acc[nt][r]);
    }
  }
}

// ---------------------------------------------------------------------------
// launchers: route (conv3_route.h), geometry, one switch

// H x W is the unpadded plane the kernel gathers from; OH x OW the plane
// it tiles over.  tiles_m / tiles_n are the caller's.
static inline void fill_geom6(ConvGeom6& g, int C, int IC, int OC, int B,
                              int H, int W, int stride) {
  g.B = B; g.Hp = H + 2; g.Wp = W + 2;
  g.OH = conv3_cdiv(H, stride); g.OW = conv3_cdiv(W, stride);
  g.IC = IC; g.OC = OC; g.stride = stride; g.C = C;
  g.lg_ow = conv3_lg(g.OW);
  g.lg_ohw = conv3_lg(g.OW) + conv3_lg(g.OH);
}

// every v6-family kernel has this signature, block size and no dynamic LDS
typedef void (*ConvKernel6)(const __hip_bfloat16*, const __hip_bfloat16*,
                            __hip_bfloat16*, ConvGeom6);

// grid: XCD-padded (xcd_remap6) over the geometry's tiles
static inline void launch6(ConvKernel6 kernel, const void* in, const void* w,
                           void* out, const ConvGeom6& g,
                           hipStream_t stream) {
  dim3 grid(((g.C + 7) / 8 * 8) * (g.tiles_m * g.tiles_n));
  hipLaunchKernelGGL(kernel, grid, dim3(CONV_THREADS), 0, stream,
                     (const __hip_bfloat16*)in, (const __hip_bfloat16*)w,
                     (__hip_bfloat16*)out, g);
}

extern "C" int ols_conv3x3_v6_ok(int IC, int OC, int B, int H, int W,
                                 int stride) {
  return conv3_v6_ok(IC, OC, B, H, W, stride);
}

extern "C" const char* ols_conv3x3_route(int dir, int IC, int OC, int B,
                                         int H, int W, int stride) {
  return conv3_route_name(conv3_route(dir, IC, OC, B, H, W, stride));
}

extern "C" const char* ols_conv3x3_staging(int dir, int IC, int OC, int B,
                                           int H, int W, int stride) {
  return conv3_kmajor(dir, IC, OC, B, H, W, stride) ? "kmajor" : "nmajor";
}

extern "C" const char* ols_conv3x3_tile(int dir, int IC, int OC, int B,
                                        int H, int W, int stride) {
  return conv3_tile_name(conv3_tile(dir, IC, OC, B, H, W, stride));
}

extern "C" void ols_conv3x3_fwd_p(const void* xp, const void* w, void* y,
                                  int C, int IC, int OC, int B, int H, int W,
                                  int stride, hipStream_t stream) {
  ConvGeom6 g;
  fill_geom6(g, C, IC, OC, B, H, W, stride);
  ConvKernel6 k = nullptr;
  const Conv3Route route = conv3_route_fwd_v6(IC, OC, B, H, W, stride);
  const bool km = conv3_kmajor_v6(0, route);
  const int tile = conv3_tile_v6(route, OC);
  g.tiles_m = conv3_cdiv(OC, tile ? 128 : CV6_BM);
  g.tiles_n = conv3_cdiv(B * g.OH * g.OW, tile ? 64 : CV6_BN);
  // (route, staging, tile) -> instantiation
#define KM_CASE(id, kern, ...)                                              \
  case id: k = km ? kern<__VA_ARGS__, true> : kern<__VA_ARGS__, false>; break;
#define TILE_PICK(kern, km_, ...)                                           \
  (tile ? kern<__VA_ARGS__, km_, 1> : kern<__VA_ARGS__, km_, 0>)
#define TILE_CASE(id, kern, ...)                                            \
  case id: k = TILE_PICK(kern, false, __VA_ARGS__); break;
#define KM_TILE_CASE(id, kern, ...)                                         \
  case id:                                                                  \
    k = km ? TILE_PICK(kern, true, __VA_ARGS__)                             \
           : TILE_PICK(kern, false, __VA_ARGS__);                           \
    break;
  switch (route) {
    KM_TILE_CASE(CV3_FWD_V6_2_1, k_conv3x3_fwd_v6, 2, 1)
    KM_TILE_CASE(CV3_FWD_V6_3_1, k_conv3x3_fwd_v6, 3, 1)
    KM_TILE_CASE(CV3_FWD_V6_4_1, k_conv3x3_fwd_v6, 4, 1)
    TILE_CASE(CV3_FWD_V6_2_2, k_conv3x3_fwd_v6, 2, 2)
    TILE_CASE(CV3_FWD_V6_3_2, k_conv3x3_fwd_v6, 3, 2)
    TILE_CASE(CV3_FWD_V6_4_2, k_conv3x3_fwd_v6, 4, 2)
    // [n][k] only: measured no faster k-major (conv3_kmajor_v6)
    TILE_CASE(CV3_FWD_V7_3_1, k_conv3x3_fwd_v7, 3, 1)
    KM_TILE_CASE(CV3_FWD_V7_4_1, k_conv3x3_fwd_v7, 4, 1)
    KM_TILE_CASE(CV3_FWD_V7_5_1, k_conv3x3_fwd_v7, 5, 1)
    default: return;                    // not a v6-family fwd route
  }
#undef TILE_PICK
#undef TILE_CASE
#undef KM_TILE_CASE
  launch6(k, xp, w, y, g, stream);
}

// the four parity classes (he, we) of the stride-2 dgrad
template <int LG>
static inline void launch_s2(const void* dyp, const void* w, void* dx,
                             const ConvGeom6& g, hipStream_t stream) {
  launch6(k_conv3x3_dgrad_s2<0, 0, LG>, dyp, w, dx, g, stream);
  launch6(k_conv3x3_dgrad_s2<0, 1, LG>, dyp, w, dx, g, stream);
  launch6(k_conv3x3_dgrad_s2<1, 0, LG>, dyp, w, dx, g, stream);
  launch6(k_conv3x3_dgrad_s2<1, 1, LG>, dyp, w, dx, g, stream);
}

extern "C" void ols_conv3x3_dgrad_p(const void* dyp, const void* w, void* dx,
                                    int C, int IC, int OC, int B, int H,
                                    int W, int stride, hipStream_t stream) {
  // The plane gathered from is dy's, the plane tiled over dx's (stride 1,
  // both H x W) or one parity class of it (stride 2, OH x OW = H/2 x W/2,
  // the size of the dy plane): either way the dy plane at stride 1.
  ConvGeom6 g;
  fill_geom6(g, C, IC, OC, B, H / stride, W / stride, 1);
  g.stride = stride;
  g.tiles_m = conv3_cdiv(IC, CV6_BM);
  g.tiles_n = conv3_cdiv(B * g.OH * g.OW, CV6_BN);
  ConvKernel6 k = nullptr;
  const Conv3Route route = conv3_route_dgrad_v6(IC, OC, B, H, W, stride);
  const bool km = conv3_kmajor_v6(1, route);
  switch (route) {
    KM_CASE(CV3_DGRAD_V6_2, k_conv3x3_dgrad_v6, 2)
    KM_CASE(CV3_DGRAD_V6_3, k_conv3x3_dgrad_v6, 3)
    KM_CASE(CV3_DGRAD_V6_4, k_conv3x3_dgrad_v6, 4)
    case CV3_DGRAD_V7_2: k = k_conv3x3_dgrad_v7<2>; break;
    case CV3_DGRAD_V7_3: k = k_conv3x3_dgrad_v7<3>; break;
    case CV3_DGRAD_V7_4: k = k_conv3x3_dgrad_v7<4>; break;
    case CV3_DGRAD_V7_5: k = k_conv3x3_dgrad_v7<5>; break;
    case CV3_DGRAD_S2_2: launch_s2<2>(dyp, w, dx, g, stream); return;
    case CV3_DGRAD_S2_3: launch_s2<3>(dyp, w, dx, g, stream); return;
    case CV3_DGRAD_S2_4: launch_s2<4>(dyp, w, dx, g, stream); return;
    default: return;                    // not a v6-family dgrad route
  }
#undef KM_CASE
  launch6(k, dyp, w, dx, g, stream);
}

extern "C" void ols_conv3x3_wgrad_p(const void* xp, const void* dy, void* dw,
                                    int C, int IC, int OC, int B, int H,
                                    int W, int stride, hipStream_t stream) {
  ConvGeom6 g;
  fill_geom6(g, C, IC, OC, B, H, W, stride);
  g.tiles_m = conv3_cdiv(OC, CV6_BM);
  g.tiles_n = conv3_cdiv(IC * 9, CV6_BN);
  ConvKernel6 k = nullptr;
  switch (conv3_route_wgrad_v6(IC, OC, B, H, W, stride)) {
    case CV3_WGRAD_V6: k = k_conv3x3_wgrad_v6; break;
    case CV3_WGRAD_V7: k = k_conv3x3_wgrad_v7; break;
    case CV3_WGRAD_V8: k = k_conv3x3_wgrad_v8; break;
    case CV3_WGRAD_V8S: k = k_conv3x3_wgrad_v8s; break;
    default: return;                    // not a v6-family wgrad route
  }
  launch6(k, xp, dy, dw, g, stream);
}
