// Flipped-transposed 3x3 weights for the stride-1 dgrad.
//
// A stride-1 dgrad is a stride-1 forward convolution of the padded dy with
//
//   wt[c][ic][oc*9 + r] = w[c][oc][ic][8 - r],   r = 3*dh + dw
//
// i.e. wt viewed as [C, IC, OC, 3, 3] is a forward weight with the channel
// counts swapped, and conv3x3_fwd_p(dy_pad, wt, 1) is dx.  The forward
// kernels read their A operand with one 16-byte load per lane; dgrad_v6
// gathers it from w in 2-byte loads at stride IC*9 (8 global_load_ushort,
// 15 v_cndmask, 4 v_perm per K-step) and is 27-32 % slower per call on the
// same shape (profiles/conv_kmajor_r06.md).
//
// k_conv3_wflip writes wt from w; k_sgd_conv3_wt is the SGD update of w
// that writes wt from the updated values it already holds, so a trainer
// pays for wt with stores alone.  Both are a tiled transpose of 18-byte
// items (the 9 taps of one (oc, ic) pair) with the taps reversed inside
// each item.
//
// Tile: 32 oc x 32 ic of one client.  A row of the tile is 32 items = 288
// contiguous shorts (576 B = 36 uint4) on the read side (row = oc, the ic
// run) and on the write side (row = ic, the oc run); OC, IC multiples of
// 32 keep both 16-byte aligned.  384 threads move the 1152 uint4 of a tile
// in 3 passes each way: 16-byte global loads, LDS image of the tile as
// loaded (18 KB), and per 16-byte global store a gather of 8 shorts,
//
//   out row ic, short p = 8j + e:  oc = p / 9, r = p % 9
//                                  <- lds[oc*288 + ic*9 + 8 - r]
//
// LDS banks (MI355X: ds_write_b128 conflicts per 8 consecutive lanes over
// 32 banks, 2-byte reads per 32-lane half over 32 banks):
//  - fill: chunk i of the tile goes to bytes 16*i, so every 8 lanes cover
//    128 contiguous bytes: conflict-free, and only because the row pitch
//    is exactly 288 shorts.  Any pad that keeps rows 16-byte aligned
//    (pitch 288 + 8k) makes the groups that straddle two rows 2-way.
//  - gather: consecutive lanes are consecutive j of one ic, so oc advances
//    by 8/9 per lane and a half-wave reads ~29 rows at columns within 9
//    shorts of each other.  The row pitch is 144 dwords = 16 mod 32, so
//    even and odd rows alternate between two 5-dword windows: 3.4-way on
//    average, 4 at worst (counted over all 8 e and all half-waves of the
//    tile).  None was found that removes it among the layouts tried, all
//    of this design (16-byte fill, lanes along j): row pitches 288..416 in
//    steps of 8 shorts and per-row chunk rotations; the best reaches
//    2.3-way for a 2-way fill.  Within the design the reason is that 32
//    banks hold 8 chunk positions, 29 rows need 4 of them each, and rows
//    8 apart read the same tap, so they cannot differ inside the chunk
//    either.  Not tried: lanes mapped across ic instead of j (64-byte
//    store segments), a 2-byte scatter on the fill side with wide reads.
//    Left as is because it does not bound the kernel.  Estimate per tile:
//    144 gather instructions x 2 cycles x 3.4 + 18 fills x 13 = ~1200 LDS
//    cycles against ~4500 for a CU's share of HBM to move the tile's 36
//    KB, 5 blocks per CU to overlap the two.  Measured at C=1250, 512 x
//    512 (profiles/dgrad_wt_r07.md): SQ_LDS_IDX_ACTIVE 1128 cycles per
//    tile, 696 of them SQ_LDS_BANK_CONFLICT; that is about a quarter of
//    k_conv3_wflip's duration per CU and a seventh of k_sgd_conv3_wt's,
//    and both kernels spend 62-63 % of their wave cycles in SQ_WAIT_ANY.
//
// Streaming kernel, each byte touched once: no XCD remap.

#include "common.h"
#include "ols_ops.h"

#define WF_TILE 32                      // oc and ic per tile
#define WF_ROW (WF_TILE * 9)            // shorts per tile row
#define WF_CHUNKS (WF_TILE * WF_ROW / 8)  // uint4 per tile
#define WF_THREADS 384
#define WF_PASSES (WF_CHUNKS / WF_THREADS)

static_assert(WF_CHUNKS % WF_THREADS == 0, "whole passes");

// first short of tile row `row` (oc on the read side with R = OC, S = IC;
// ic on the write side with R = IC, S = OC) in a [C][R][S][9] tensor
__device__ __forceinline__ int64_t wf_row_off(int c, int R, int S, int r0,
                                              int row, int s0) {
  return (((int64_t)c * R + r0 + row) * S + s0) * 9;
}

// write side: out chunk j of tile row ic, gathered from the LDS image
__device__ __forceinline__ uint4 wf_gather(const ushort* lds, int ic, int j) {
  int oc = (8 * j) / 9;
  int r = 8 * j - 9 * oc;
  Pack<ushort, 8> v;
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    v.v[e] = lds[oc * WF_ROW + ic * 9 + 8 - r];
    if (++r == 9) { r = 0; ++oc; }
  }
  return __builtin_bit_cast(uint4, v);
}

// SGD = false: wt <- flip(w).  SGD = true: w <- w - lr*g in place (the
// expression of k_sgd_plain, so it contracts the same way), wt <- flip of
// the updated w.
template <bool SGD>
__device__ __forceinline__ void wf_tile(
    __hip_bfloat16* __restrict__ w, const __hip_bfloat16* __restrict__ g,
    __hip_bfloat16* __restrict__ wt, int OC, int IC, float lr) {
  __shared__ __attribute__((aligned(16))) ushort lds[WF_TILE * WF_ROW];
  const int tiles_ic = IC / WF_TILE;
  const int tiles = (OC / WF_TILE) * tiles_ic;
  const int c = blockIdx.x / tiles;
  const int tile = blockIdx.x - c * tiles;
  const int oc0 = (tile / tiles_ic) * WF_TILE;
  const int ic0 = (tile % tiles_ic) * WF_TILE;

  uint4 in[WF_PASSES];
#pragma unroll
  for (int p = 0; p < WF_PASSES; ++p) {
    const int i = threadIdx.x + p * WF_THREADS;
    const int row = i / 36, col = i - row * 36;
    const int64_t off = wf_row_off(c, OC, IC, oc0, row, ic0) + col * 8;
    in[p] = *reinterpret_cast<const uint4*>(w + off);
    if constexpr (SGD) {
      using P8 = Pack<__hip_bfloat16, 8>;
      P8 wv = __builtin_bit_cast(P8, in[p]);
      const P8 gv = *reinterpret_cast<const P8*>(g + off);
#pragma unroll
      for (int k = 0; k < 8; ++k)
        wv.v[k] = from_f32<__hip_bfloat16>(to_f32(wv.v[k]) -
                                           lr * to_f32(gv.v[k]));
      in[p] = __builtin_bit_cast(uint4, wv);
      *reinterpret_cast<uint4*>(w + off) = in[p];
    }
  }
#pragma unroll
  for (int p = 0; p < WF_PASSES; ++p)
    *reinterpret_cast<uint4*>(&lds[(threadIdx.x + p * WF_THREADS) * 8]) =
        in[p];
  __syncthreads();
#pragma unroll
  for (int p = 0; p < WF_PASSES; ++p) {
    const int i = threadIdx.x + p * WF_THREADS;
    const int ic = i / 36, j = i - ic * 36;
    *reinterpret_cast<uint4*>(wt + wf_row_off(c, IC, OC, ic0, ic, oc0) +
                              j * 8) = wf_gather(lds, ic, j);
  }
}

__global__ __launch_bounds__(WF_THREADS) void k_conv3_wflip(
    const __hip_bfloat16* __restrict__ w, __hip_bfloat16* __restrict__ wt,
    int OC, int IC) {
  wf_tile<false>(const_cast<__hip_bfloat16*>(w), nullptr, wt, OC, IC, 0.f);
}

__global__ __launch_bounds__(WF_THREADS) void k_sgd_conv3_wt(
    __hip_bfloat16* __restrict__ w, const __hip_bfloat16* __restrict__ g,
    __hip_bfloat16* __restrict__ wt, int OC, int IC, float lr) {
  wf_tile<true>(w, g, wt, OC, IC, lr);
}

static inline unsigned wf_grid(int C, int OC, int IC) {
  return (unsigned)((int64_t)C * (OC / WF_TILE) * (IC / WF_TILE));
}

extern "C" void ols_conv3_wflip(const void* w, void* wt, int C, int OC,
                                int IC, hipStream_t stream) {
  hipLaunchKernelGGL(k_conv3_wflip, dim3(wf_grid(C, OC, IC)),
                     dim3(WF_THREADS), 0, stream, (const __hip_bfloat16*)w,
                     (__hip_bfloat16*)wt, OC, IC);
}

extern "C" void ols_sgd_conv3_wt(void* w, const void* g, void* wt, int C,
                                 int OC, int IC, float lr,
                                 hipStream_t stream) {
  hipLaunchKernelGGL(k_sgd_conv3_wt, dim3(wf_grid(C, OC, IC)),
                     dim3(WF_THREADS), 0, stream, (__hip_bfloat16*)w,
                     (const __hip_bfloat16*)g, (__hip_bfloat16*)wt, OC, IC,
                     lr);
}
