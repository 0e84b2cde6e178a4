// Device pieces shared by the causal attention kernels of attn.hip (one
// workgroup holds a whole sequence of up to 128 rows) and attn_long.hip
// (129 to 512 rows, streamed in blocks of 128): the bf16 pack and convert
// helpers, the XOR-swizzled 128-row LDS tile with its two fragment reads,
// and the 16-byte row store.  The tile layout and its bank-conflict
// argument are in the header of attn.hip.
#pragma once

#include "common.h"

typedef __attribute__((ext_vector_type(8))) short bf16x8;
typedef __attribute__((ext_vector_type(4))) short bf16x4;
typedef __attribute__((ext_vector_type(4))) float f32x4;
typedef __attribute__((ext_vector_type(4))) int i32x4;
typedef __attribute__((address_space(3))) bf16x4 lds_bf16x4;

#define ATTN_THREADS 256
#define ATTN_ROWS 128
#define ATTN_LOG2E 1.44269504088896341f
#define ATTN_LN2 0.693147180559945309f
#define ATTN_MASKED -1.0e30f

// Compiled without packed fp32 arithmetic (v_pk_*_f32), as lstm.hip: a
// function with another target feature set is not inlined, so everything
// the kernels call is defined here on compiler builtins.
#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute push(__attribute__((target("no-packed-fp32-ops"))), \
                             apply_to = function)
#endif

// round-to-nearest-even bf16 bits of a finite fp32
__device__ __forceinline__ unsigned attn_bits(float v) {
  const unsigned u = __builtin_bit_cast(unsigned, v);
  return (u + 0x7FFFu + ((u >> 16) & 1u)) >> 16;
}
__device__ __forceinline__ int attn_pack2(float lo, float hi) {
  return (int)(attn_bits(lo) | (attn_bits(hi) << 16));
}
__device__ __forceinline__ float attn_val(short s) {
  return __builtin_bit_cast(float, ((unsigned)(unsigned short)s) << 16);
}
// eight k-slots of an operand from the registers of two neighbouring tiles
__device__ __forceinline__ bf16x8 attn_pack8(const f32x4& a, const f32x4& b) {
  const i32x4 v = {attn_pack2(a[0], a[1]), attn_pack2(a[2], a[3]),
                   attn_pack2(b[0], b[1]), attn_pack2(b[2], b[3])};
  return __builtin_bit_cast(bf16x8, v);
}
__device__ __forceinline__ int attn_from(int lane, int v) {
  return __builtin_amdgcn_ds_bpermute(lane << 2, v);
}
__device__ __forceinline__ float attn_from(int lane, float v) {
  return __builtin_bit_cast(float,
                            attn_from(lane, __builtin_bit_cast(int, v)));
}
__device__ __forceinline__ void attn_barrier() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __builtin_amdgcn_s_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}
__device__ __forceinline__ f32x4 attn_mfma(const bf16x8& a, const bf16x8& b,
                                           const f32x4& c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
}

// 8 bf16 of row `row` at column col, zeros past the sequence
__device__ __forceinline__ bf16x8 attn_load8(const short* base, int64_t ld,
                                             int row, int col, int L) {
  bf16x8 v = {0, 0, 0, 0, 0, 0, 0, 0};
  if (row < L) v = *reinterpret_cast<const bf16x8*>(base + row * ld + col);
  return v;
}

// offset in shorts of element (row, d) of a tile (header: LDS)
template <int HD>
__device__ __forceinline__ int attn_off(int row, int d) {
  const int sw = (HD == 64 ? ((row >> 1) & 3) << 1 : ((row >> 2) & 1) << 1) |
                 ((row >> 3) & 1);
  return row * HD + (((d >> 3) ^ sw) << 3) + (d & 7);
}

// rows [0, nrows) of one operand (global row stride ld) into a tile
template <int HD>
__device__ __forceinline__ void attn_stage(short* tile, const short* src,
                                           int64_t ld, int L, int nrows,
                                           int tid) {
  constexpr int CH = HD / 8;
  for (int idx = tid; idx < nrows * CH; idx += ATTN_THREADS) {
    const int c = idx % CH, row = idx / CH;
    *reinterpret_cast<bf16x8*>(&tile[attn_off<HD>(row, 8 * c)]) =
        attn_load8(src, ld, row, 8 * c, L);
  }
}

// fragment with k along HD: row 16*t + (l&15), k 32*kc + 8*(l>>4) .. +7
template <int HD>
__device__ __forceinline__ bf16x8 attn_row_frag(const short* tile, int t,
                                                int kc, int lane) {
  return *reinterpret_cast<const bf16x8*>(
      &tile[attn_off<HD>(16 * t + (lane & 15), 32 * kc + 8 * (lane >> 4))]);
}

// fragment with k along rows: k-slot (g, e) is row rb + 16*(e>>2) + 4g +
// (e&3), the other index is column 16*dt + (l&15).  off = the lane's
// attn_off(4g + q, 16*dt + 4p), lane = 16g + 4q + p; rb a multiple of 32.
// Needs EXEC all ones: called under wave-uniform control flow only.
template <int HD>
__device__ __forceinline__ bf16x8 attn_tr_frag(const short* tile, int off,
                                               int rb) {
  const short* p = tile + rb * HD + off;
  const bf16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_bf16x4*)p);
  const bf16x4 hi =
      __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_bf16x4*)(p + 16 * HD));
  return __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
}

// acc[dt][r] = X[row][16*dt + 4g + r] times mul, as bf16 to rowp[0 .. HD):
// lanes g and g^1 exchange one 4-pack per pair of d-tiles and each stores
// 8 consecutive d.  Every lane takes part; only `valid` ones store.
template <int DT>
__device__ __forceinline__ void attn_store_rows(const f32x4 (&acc)[DT],
                                                float mul, short* rowp,
                                                bool valid, int lane) {
  const int g = lane >> 4;
  const bool odd = g & 1;
#pragma unroll
  for (int u = 0; u < DT / 2; ++u) {
    const f32x4 a = acc[2 * u], b = acc[2 * u + 1];
    const int lo0 = attn_pack2(a[0] * mul, a[1] * mul);
    const int lo1 = attn_pack2(a[2] * mul, a[3] * mul);
    const int hi0 = attn_pack2(b[0] * mul, b[1] * mul);
    const int hi1 = attn_pack2(b[2] * mul, b[3] * mul);
    const int r0 = attn_from(lane ^ 16, odd ? lo0 : hi0);
    const int r1 = attn_from(lane ^ 16, odd ? lo1 : hi1);
    const i32x4 out = odd ? i32x4{r0, r1, hi0, hi1} : i32x4{lo0, lo1, r0, r1};
    const int d0 = odd ? 32 * u + 16 + 4 * (g - 1) : 32 * u + 4 * g;
    if (valid) *reinterpret_cast<i32x4*>(rowp + d0) = out;
  }
}

template <int HD>
struct AttnGeom {
  static constexpr int KC = HD / 32, DT = HD / 16;
  static constexpr float scale = HD == 64 ? 0.125f : 0.176776695296636881f;
};

// rows staged for a sequence of nt tiles: whole pairs of tiles, since a
// k-slot pair reads both of its tiles
__device__ __forceinline__ int attn_rows(int nt) {
  const int r = ((nt + 1) & ~1) * 16;
  return r < ATTN_ROWS ? r : ATTN_ROWS;
}

// p and dS of one recomputed tile: s, dp the accumulators, (i, j) the
// element's query and key per register, lse and D of query i
__device__ __forceinline__ void attn_p_ds(float s, float dp, float scale,
                                          bool live, float lse_i, float d_i,
                                          float& p, float& ds) {
  p = live ? __builtin_amdgcn_exp2f((s * scale - lse_i) * ATTN_LOG2E) : 0.f;
  ds = live ? p * (dp - d_i) : 0.f;
}

#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute pop
#endif
