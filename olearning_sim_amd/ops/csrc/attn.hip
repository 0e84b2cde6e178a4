// Fused causal self-attention of the per-client BERT for gfx950.
//
//   S = scale * Q K^T (causal), P = softmax(S), O = P V
// for one head of one (client, batch row) at a time, read straight from the
// packed qkv [CB, L, 3, heads, HD] that the qkv blinear writes and written
// straight into att [CB, L, heads*HD] for the next blinear; the backward
// writes dqkv packed like qkv.  L <= 128, HD 32 or 64 (attn_route.h).
//
// ONE WORKGROUP OF FOUR WAVES OWNS ONE (cb, head): grid CB*heads, no
// synchronisation between workgroups, no atomics, no global scratch.
// A wave owns 16-row tiles w and 7-w of the sequence, one short and one
// long causal row block, so the triangle is balanced.
//
// Every product is computed TRANSPOSED, so that no probability ever goes
// through LDS.  With v_mfma_f32_16x16x32_bf16 (A: lane l holds row l&15,
// k 8*(l>>4)..+7; B: column l&15, same k; C/D: reg r of lane l is row
// 4*(l>>4)+r, column l&15) the forward computes S^T = K Q^T per 16-key
// tile: lane (i = l&15, g = l>>4) then holds keys 16*kt + 4g + r of ITS
// query i.  The softmax row is in-lane over registers and tiles plus two
// cross-lane steps (xor 16, 32); max, exp2 and sum are exact two-pass, no
// running maximum.  The four registers of two neighbouring key tiles are,
// as they stand, the eight k-slots of a B operand whose k-slot (g, e) is
// key 32*kc + 16*(e>>2) + 4g + (e&3); O^T = V^T P^T takes V^T in the same
// slot order as A operand, which the transposed LDS read delivers from any
// four rows a 16-lane block names.  O^T leaves lane (i, g) with O[i][16*dt
// + 4g + r]: the row sum of query i is in the same lane, and one exchange
// with lane^16 turns two d-tiles' 4-packs into one 16-byte store.
//
// The backward has two phases in the same shape, each recomputing its own
// tiles of P and dS (7 products instead of 5; the kernel is bound by LDS
// and latency, not by MFMA), so P and dS are rounded to bf16 only in
// registers as MFMA operands and nothing needs LDS space or atomics:
//   phase A, wave owns query tiles: S^T = K Q^T and dP^T = V dO^T per key
//     tile, dS^T = P^T (dP^T - D_i) in-lane, dQ^T = K^T dS^T; D_i = dO_i .
//     O_i from the fragments already loaded.  D and lse go to LDS.
//   phase B, wave owns key tiles: S = Q K^T and dP = dO V^T per query tile
//     (lane holds queries 16*it + 4g + r of ITS key j), dV^T = dO^T P,
//     dK^T = Q^T dS.
// The own-tile operand of every product (Q, dO in A; K, V in B) is used by
// one wave only and goes global -> VGPR as B fragments, never through LDS.
//
// LDS: every staged operand is one tile [128][HD] bf16 without padding
// (rows >= L zero), whose 16-byte pack c of row R is stored at pack
//   c ^ sw(R),  sw(R) = 2*((R>>1)&3) + ((R>>3)&1)   (HD 64, 8 packs a row)
//               sw(R) = 2*((R>>2)&1) + ((R>>3)&1)   (HD 32, 4 packs a row)
// and which serves both fragment kinds:
//  - k along ROWS (V in O^T, K in dQ^T, dO and Q in dV^T and dK^T):
//    ds_read_b64_tr_b16, conflicts per 32-lane half over 64 banks.  A half
//    reads 8 consecutive rows x the 32 bytes of one d-tile dt (packs 2dt,
//    2dt+1; bit 0 of sw only swaps them).  Their 32-byte units mod 256
//    are 4*(R&1) + (dt ^ (R>>1)&3) at HD 64 and 2*(R&3) + (dt ^ (R>>2)&1)
//    at HD 32: eight different units, conflict-free.
//  - k along HD (K and V in S^T and dP^T, Q and dO in S and dP): one
//    ds_read_b128 per lane, row 16*t + (l&15), pack 4*kc + (l>>4); taken
//    as the other b128 tiles of this project take it, 16 lanes of one
//    l>>4 at a time over the 256 bytes the 64 banks span.  Their 16 rows
//    have 16-byte slots mod 16 of 8*(R&1) + (c ^ sw(R)) at HD 64, where
//    R&1 and the three bits of sw separate all 16 rows, and 4*(R&3) +
//    (c ^ sw(R)) at HD 32, likewise: conflict-free.
//  - written by ds_write_b128, conflicts per 8 consecutive lanes over 32
//    banks: the 8 lanes hold the 8 packs of one row (HD 64) or the 4 + 4
//    of two consecutive rows (HD 32), 128 contiguous bytes that sw only
//    permutes within each row: conflict-free.
// Forward: K and V tiles, 32 KB at HD 64.  Backward: K and V in phase A,
// restaged with Q and dO for phase B, plus 1 KB of D and lse: 33 KB.

#include <initializer_list>

#include "common.h"
#include "attn_dev.h"
#include "attn_route.h"
#include "ols_ops.h"

// as attn_dev.h: no packed fp32 arithmetic in the kernels either
#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute push(__attribute__((target("no-packed-fp32-ops"))), \
                             apply_to = function)
#endif

// ---------------------------------------------------------------------------
template <int HD>
__global__ __launch_bounds__(ATTN_THREADS) void k_attn_fwd(
    const short* __restrict__ qkv, short* __restrict__ att,
    float* __restrict__ lse, int L, int heads) {
  using G = AttnGeom<HD>;
  constexpr int KC = G::KC, DT = G::DT;
  __shared__ __align__(16) short k_t[ATTN_ROWS * HD];
  __shared__ __align__(16) short v_t[ATTN_ROWS * HD];

  const int tid = __builtin_amdgcn_workitem_id_x();
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int i16 = lane & 15, g = lane >> 4;
  const int bid = __builtin_amdgcn_workgroup_id_x();
  const int cb = bid / heads, head = bid - cb * heads;
  const int H = heads * HD;
  const int64_t ld = 3 * (int64_t)H;
  const short* qg = qkv + (int64_t)cb * L * ld + head * HD;
  const int nt = (L + 15) >> 4;

  attn_stage<HD>(k_t, qg + H, ld, L, attn_rows(nt), tid);
  attn_stage<HD>(v_t, qg + 2 * H, ld, L, attn_rows(nt), tid);
  int troff[DT];
#pragma unroll
  for (int dt = 0; dt < DT; ++dt)
    troff[dt] = attn_off<HD>(4 * g + ((lane >> 2) & 3),
                                16 * dt + 4 * (lane & 3));
  attn_barrier();

  for (int pass = 0; pass < 2; ++pass) {
    const int qt = pass ? 7 - wave : wave;
    if (qt >= nt) continue;
    const int i = 16 * qt + i16;
    bf16x8 qf[KC];
#pragma unroll
    for (int kc = 0; kc < KC; ++kc)
      qf[kc] = attn_load8(qg, ld, i, 32 * kc + 8 * g, L);

    // S^T per key tile, tiles above the diagonal skipped
    f32x4 s[8];
#pragma unroll
    for (int kt = 0; kt < 8; ++kt) {
      s[kt] = {0.f, 0.f, 0.f, 0.f};
      if (kt <= qt) {
#pragma unroll
        for (int kc = 0; kc < KC; ++kc)
          s[kt] = attn_mfma(attn_row_frag<HD>(k_t, kt, kc, lane), qf[kc],
                            s[kt]);
      }
    }
    float m = ATTN_MASKED;
#pragma unroll
    for (int kt = 0; kt < 8; ++kt)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float v =
            16 * kt + 4 * g + r <= i ? s[kt][r] * G::scale : ATTN_MASKED;
        s[kt][r] = v;
        m = __builtin_fmaxf(m, v);
      }
    m = __builtin_fmaxf(m, attn_from(lane ^ 16, m));
    m = __builtin_fmaxf(m, attn_from(lane ^ 32, m));
    float l = 0.f;
#pragma unroll
    for (int kt = 0; kt < 8; ++kt)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float p =
            __builtin_amdgcn_exp2f((s[kt][r] - m) * ATTN_LOG2E);
        s[kt][r] = p;
        l += p;
      }
    l += attn_from(lane ^ 16, l);
    l += attn_from(lane ^ 32, l);

    // O^T = V^T P^T
    f32x4 o[DT];
#pragma unroll
    for (int dt = 0; dt < DT; ++dt) o[dt] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int kc2 = 0; kc2 < 4; ++kc2) {
      if (2 * kc2 <= qt) {
        const bf16x8 pb = attn_pack8(s[2 * kc2], s[2 * kc2 + 1]);
#pragma unroll
        for (int dt = 0; dt < DT; ++dt)
          o[dt] = attn_mfma(attn_tr_frag<HD>(v_t, troff[dt], 32 * kc2), pb,
                            o[dt]);
      }
    }
    attn_store_rows<DT>(o, __builtin_amdgcn_rcpf(l),
                        att + ((int64_t)cb * L + i) * H + head * HD, i < L,
                        lane);
    if (g == 0 && i < L)
      lse[((int64_t)cb * heads + head) * L + i] =
          m + __builtin_amdgcn_logf(l) * ATTN_LN2;
  }
}

template <int HD>
__global__ __launch_bounds__(ATTN_THREADS) void k_attn_bwd(
    const short* __restrict__ qkv, const short* __restrict__ att,
    const short* __restrict__ datt, const float* __restrict__ lse,
    short* __restrict__ dqkv, int L, int heads) {
  using G = AttnGeom<HD>;
  constexpr int KC = G::KC, DT = G::DT;
  __shared__ __align__(16) short t0[ATTN_ROWS * HD];
  __shared__ __align__(16) short t1[ATTN_ROWS * HD];
  __shared__ float lse_l[ATTN_ROWS], d_l[ATTN_ROWS];

  const int tid = __builtin_amdgcn_workitem_id_x();
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int i16 = lane & 15, g = lane >> 4;
  const int bid = __builtin_amdgcn_workgroup_id_x();
  const int cb = bid / heads, head = bid - cb * heads;
  const int H = heads * HD;
  const int64_t ld = 3 * (int64_t)H;
  const int64_t row0 = (int64_t)cb * L;
  const short* qg = qkv + row0 * ld + head * HD;
  const short* og = att + row0 * H + head * HD;
  const short* dog = datt + row0 * H + head * HD;
  short* dqg = dqkv + row0 * ld + head * HD;
  const float* lse_g = lse + ((int64_t)cb * heads + head) * L;
  const int nt = (L + 15) >> 4;
  const int nrows = attn_rows(nt);

  int troff[DT];
#pragma unroll
  for (int dt = 0; dt < DT; ++dt)
    troff[dt] = attn_off<HD>(4 * g + ((lane >> 2) & 3),
                                16 * dt + 4 * (lane & 3));

  // ---- phase A: query tiles, dQ ------------------------------------------
  {
    const short* k_t = t0;
    const short* v_t = t1;
    attn_stage<HD>(t0, qg + H, ld, L, nrows, tid);
    attn_stage<HD>(t1, qg + 2 * H, ld, L, nrows, tid);
    attn_barrier();

    for (int pass = 0; pass < 2; ++pass) {
      const int qt = pass ? 7 - wave : wave;
      if (qt >= nt) continue;
      const int i = 16 * qt + i16;
      bf16x8 qf[KC], dof[KC];
      float d_i = 0.f;
#pragma unroll
      for (int kc = 0; kc < KC; ++kc) {
        qf[kc] = attn_load8(qg, ld, i, 32 * kc + 8 * g, L);
        dof[kc] = attn_load8(dog, H, i, 32 * kc + 8 * g, L);
        const bf16x8 of = attn_load8(og, H, i, 32 * kc + 8 * g, L);
#pragma unroll
        for (int e = 0; e < 8; ++e)
          d_i += attn_val(dof[kc][e]) * attn_val(of[e]);
      }
      d_i += attn_from(lane ^ 16, d_i);
      d_i += attn_from(lane ^ 32, d_i);
      const float lse_i = i < L ? lse_g[i] : 0.f;
      if (g == 0) {
        d_l[i] = d_i;
        lse_l[i] = lse_i;
      }

      f32x4 dq[DT];
#pragma unroll
      for (int dt = 0; dt < DT; ++dt) dq[dt] = {0.f, 0.f, 0.f, 0.f};
      for (int kc2 = 0; 2 * kc2 <= qt; ++kc2) {
        f32x4 dsv[2];
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          const int kt = 2 * kc2 + h;
          f32x4 s = {0.f, 0.f, 0.f, 0.f}, dp = {0.f, 0.f, 0.f, 0.f};
          if (kt <= qt) {
#pragma unroll
            for (int kc = 0; kc < KC; ++kc) {
              s = attn_mfma(attn_row_frag<HD>(k_t, kt, kc, lane), qf[kc], s);
              dp = attn_mfma(attn_row_frag<HD>(v_t, kt, kc, lane), dof[kc],
                             dp);
            }
          }
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            float p, ds;
            attn_p_ds(s[r], dp[r], G::scale, 16 * kt + 4 * g + r <= i, lse_i,
                      d_i, p, ds);
            dsv[h][r] = ds;
          }
        }
        const bf16x8 dsb = attn_pack8(dsv[0], dsv[1]);
#pragma unroll
        for (int dt = 0; dt < DT; ++dt)
          dq[dt] = attn_mfma(attn_tr_frag<HD>(k_t, troff[dt], 32 * kc2), dsb,
                             dq[dt]);
      }
      attn_store_rows<DT>(dq, G::scale, dqg + i * ld, i < L, lane);
    }
  }
  attn_barrier();

  // ---- phase B: key tiles, dK and dV -------------------------------------
  {
    const short* q_t = t0;
    const short* do_t = t1;
    attn_stage<HD>(t0, qg, ld, L, nrows, tid);
    attn_stage<HD>(t1, dog, H, L, nrows, tid);
    attn_barrier();

    for (int pass = 0; pass < 2; ++pass) {
      const int jt = pass ? 7 - wave : wave;
      if (jt >= nt) continue;
      const int j = 16 * jt + i16;
      bf16x8 kf[KC], vf[KC];
#pragma unroll
      for (int kc = 0; kc < KC; ++kc) {
        kf[kc] = attn_load8(qg + H, ld, j, 32 * kc + 8 * g, L);
        vf[kc] = attn_load8(qg + 2 * H, ld, j, 32 * kc + 8 * g, L);
      }
      f32x4 dk[DT], dv[DT];
#pragma unroll
      for (int dt = 0; dt < DT; ++dt) {
        dk[dt] = {0.f, 0.f, 0.f, 0.f};
        dv[dt] = {0.f, 0.f, 0.f, 0.f};
      }
      for (int kc2 = jt >> 1; 2 * kc2 < nt; ++kc2) {
        f32x4 pv[2], dsv[2];
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          const int it = 2 * kc2 + h;
          f32x4 s = {0.f, 0.f, 0.f, 0.f}, dp = {0.f, 0.f, 0.f, 0.f};
          const bool tile_live = it >= jt && it < nt;
          if (tile_live) {
#pragma unroll
            for (int kc = 0; kc < KC; ++kc) {
              s = attn_mfma(attn_row_frag<HD>(q_t, it, kc, lane), kf[kc], s);
              dp = attn_mfma(attn_row_frag<HD>(do_t, it, kc, lane), vf[kc],
                             dp);
            }
          }
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int i = 16 * it + 4 * g + r;
            const bool live = tile_live && j <= i && i < L;
            float p, ds;
            attn_p_ds(s[r], dp[r], G::scale, live, live ? lse_l[i] : 0.f,
                      live ? d_l[i] : 0.f, p, ds);
            pv[h][r] = p;
            dsv[h][r] = ds;
          }
        }
        const bf16x8 pb = attn_pack8(pv[0], pv[1]);
        const bf16x8 dsb = attn_pack8(dsv[0], dsv[1]);
#pragma unroll
        for (int dt = 0; dt < DT; ++dt) {
          dv[dt] = attn_mfma(attn_tr_frag<HD>(do_t, troff[dt], 32 * kc2), pb,
                             dv[dt]);
          dk[dt] = attn_mfma(attn_tr_frag<HD>(q_t, troff[dt], 32 * kc2), dsb,
                             dk[dt]);
        }
      }
      attn_store_rows<DT>(dk, G::scale, dqg + H + j * ld, j < L, lane);
      attn_store_rows<DT>(dv, 1.f, dqg + 2 * H + j * ld, j < L, lane);
    }
  }
}

#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute pop
#endif

// ---------------------------------------------------------------------------
extern "C" const char* ols_attn_route(int L, int HD, int is_bf16,
                                      int aligned) {
  return attn_route_name(attn_route(L, HD, is_bf16 != 0, aligned != 0));
}

static bool attn_aligned(std::initializer_list<const void*> ptrs) {
  for (const void* p : ptrs)
    if (reinterpret_cast<uintptr_t>(p) % 16 != 0) return false;
  return true;
}

extern "C" int ols_attn_fwd(const void* qkv, void* att, float* lse, int CB,
                            int L, int heads, int HD, hipStream_t stream) {
  if (attn_route(L, HD, true, attn_aligned({qkv, att, lse})) != ATTN_FUSED)
    return 1;
  if (CB == 0 || heads == 0) return 0;
  if (HD == 64)
    hipLaunchKernelGGL(k_attn_fwd<64>, dim3(CB * heads), dim3(ATTN_THREADS), 0,
                       stream, (const short*)qkv, (short*)att, lse, L, heads);
  else
    hipLaunchKernelGGL(k_attn_fwd<32>, dim3(CB * heads), dim3(ATTN_THREADS), 0,
                       stream, (const short*)qkv, (short*)att, lse, L, heads);
  return 0;
}

extern "C" int ols_attn_bwd(const void* qkv, const void* att,
                            const void* datt, const float* lse, void* dqkv,
                            int CB, int L, int heads, int HD,
                            hipStream_t stream) {
  if (attn_route(L, HD, true, attn_aligned({qkv, att, datt, lse, dqkv})) !=
      ATTN_FUSED)
    return 1;
  if (CB == 0 || heads == 0) return 0;
  if (HD == 64)
    hipLaunchKernelGGL(k_attn_bwd<64>, dim3(CB * heads), dim3(ATTN_THREADS), 0,
                       stream, (const short*)qkv, (const short*)att,
                       (const short*)datt, lse, (short*)dqkv, L, heads);
  else
    hipLaunchKernelGGL(k_attn_bwd<32>, dim3(CB * heads), dim3(ATTN_THREADS), 0,
                       stream, (const short*)qkv, (const short*)att,
                       (const short*)datt, lse, (short*)dqkv, L, heads);
  return 0;
}
