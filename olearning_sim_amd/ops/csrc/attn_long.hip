// Fused causal self-attention for sequences of 129 to 512 tokens, gfx950.
//
// Same operands as attn.hip (packed qkv [CB, L, 3, heads, HD] in, att [CB,
// L, heads*HD] and lse [CB, heads, L] out, dqkv packed like qkv), same
// transposed products on v_mfma_f32_16x16x32_bf16, same swizzled 128-row LDS
// tile (attn_dev.h; layout and bank argument in the header of attn.hip).
// What is new is the work split: the sequence is cut into nb = ceil(L/128)
// blocks of 128 rows, a workgroup of four waves owns ONE block and streams
// the blocks it meets through the two LDS tiles.  HD 32 or 64, any L in the
// range (attn_route.h); rows past L are staged as zeros and never stored.
//
// FORWARD, k_attn_long_fwd: grid CB*heads*nb, one workgroup per (cb, head,
// query block qb).  The block index counts qb down, so the workgroups with
// the most key blocks (qb + 1 of them) are scheduled first and the short
// ones fill the tail.  Wave w owns query tiles w and 7-w of its block; their
// Q fragments stay in registers as B operands for the whole kernel.  Key
// blocks 0..qb pass through the K and V tiles (32 KB at HD 64).  Blocks
// before qb are unmasked: both query tiles of a wave take all 8 key tiles.
// Block qb is the causal case of attn.hip with L - 128*qb live rows.
//
// Staging overlap: REGISTER PREFETCH, not a second pair of tiles.  Before
// the products of block kb each thread issues the global loads of its share
// of block kb+1 (HD/8 packs of 16 bytes: 32 VGPRs at HD 64) and commits them
// to LDS after the barrier that ends block kb.  A second pair of tiles would
// take 64 KB, the static limit, for the forward and 65 KB, past it, for the
// backward with its lse and D; the registers fit (HD 64: 237 of 512 in the
// forward, two waves a SIMD; docs/KERNEL_NOTES.md), one scheme serves all
// three streaming loops, and a load in flight costs no LDS write port
// until its data is there.
//
// Online softmax in the transposed layout: lane (i = l&15, g = l>>4) holds
// keys 16*kt + 4g + r of ITS query i.  Per key block: the block maximum bm
// in-lane over registers and tiles and two cross-lane steps (xor 16, 32),
//   m_new = max(m, bm),  alpha = exp2((m - m_new) log2e),
//   l = l alpha + sum_j exp2((s_j - m_new) log2e),  O^T = O^T alpha + V^T P^T.
// m starts at the finite ATTN_MASKED (-1e30) and l at 0, so no inf - inf is
// ever formed: the first block always holds key 0 <= i, its alpha is
// exp2(-huge) = 0 and multiplies zeros.  The four lanes of a query share m
// and alpha, so each keeps its partial l and the cross-lane sum is taken
// once at the end.  The O^T accumulators of query i live in the same lane
// as l and are multiplied by the SAME VALUE alpha: whatever error the fast
// exp2 puts into alpha scales numerator and denominator alike and cancels
// in O / l.  It does not cancel in lse = m + log(l), which carries up to
// nb - 1 such factors (tests/attn_long_ref.py).  One division at the end.
//
// BACKWARD: k_attn_long_dsum writes D[cb, head, i] = dO_i . O_i in fp32 (a
// key block needs D of query blocks other workgroups own), then
// k_attn_long_bwd on grid CB*heads*nb.  Workgroup b runs two phases over
// the same 33 KB of LDS, each with the register prefetch of the forward:
//   phase A, query block b: waves own query tiles (Q, dO as B fragments,
//     lse_i and D_i in registers), key blocks 0..b through the K and V
//     tiles: S^T, dP^T per key tile, dS^T = P^T (dP^T - D_i) with P from
//     lse, dQ^T += K^T dS^T in registers, stored once.
//   phase B, key block b: waves own key tiles (K, V as B fragments), query
//     blocks b..nb-1 through the Q and dO tiles with that block's lse and D
//     (1 KB): dV^T += dO^T P, dK^T += Q^T dS in registers, stored once.
// Workgroup b does (b + 1) + (nb - b) = nb + 1 block products whatever b
// is: balanced by construction, no atomics, no scratch but D, deterministic,
// and every element of dqkv is written.  3 launches a layer.

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

// One thread's share of a 128-row block, HD/16 packs, global -> registers.
// src is the block's first row, L the rows the sequence has from there on.
// Pack idx = tid + 256 t is row idx / CH, pack idx % CH, as attn_stage.
template <int HD>
__device__ __forceinline__ void attn_long_fetch(bf16x8 (&r)[HD / 16],
                                                const short* src, int64_t ld,
                                                int L, int tid) {
  constexpr int CH = HD / 8;
#pragma unroll
  for (int t = 0; t < HD / 16; ++t) {
    const int idx = tid + t * ATTN_THREADS;
    r[t] = attn_load8(src, ld, idx / CH, 8 * (idx % CH), L);
  }
}

// ... and registers -> tile
template <int HD>
__device__ __forceinline__ void attn_long_commit(short* tile,
                                                 const bf16x8 (&r)[HD / 16],
                                                 int tid) {
  constexpr int CH = HD / 8;
#pragma unroll
  for (int t = 0; t < HD / 16; ++t) {
    const int idx = tid + t * ATTN_THREADS;
    *reinterpret_cast<bf16x8*>(&tile[attn_off<HD>(idx / CH, 8 * (idx % CH))]) =
        r[t];
  }
}

// ---------------------------------------------------------------------------
template <int HD>
__global__ __launch_bounds__(ATTN_THREADS) void k_attn_long_fwd(
    const short* __restrict__ qkv, short* __restrict__ att,
    float* __restrict__ lse, int L, int heads, int nb, int CBH) {
  using G = AttnGeom<HD>;
  constexpr int KC = G::KC, DT = G::DT;
  __shared__ __align__(16) short k_t[ATTN_ROWS * HD];
  __shared__ __align__(16) short v_t[ATTN_ROWS * HD];

  const int tid = __builtin_amdgcn_workitem_id_x();
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int i16 = lane & 15, g = lane >> 4;
  const int bid = __builtin_amdgcn_workgroup_id_x();
  const int qb = nb - 1 - bid / CBH;          // heaviest query blocks first
  const int ch = bid % CBH;
  const int cb = ch / heads, head = ch - cb * heads;
  const int H = heads * HD;
  const int64_t ld = 3 * (int64_t)H;
  const short* qg = qkv + (int64_t)cb * L * ld + head * HD;

  int troff[DT];
#pragma unroll
  for (int dt = 0; dt < DT; ++dt)
    troff[dt] = attn_off<HD>(4 * g + ((lane >> 2) & 3),
                                16 * dt + 4 * (lane & 3));

  bf16x8 kr[HD / 16], vr[HD / 16];
  attn_long_fetch<HD>(kr, qg + H, ld, L, tid);
  attn_long_fetch<HD>(vr, qg + 2 * H, ld, L, tid);

  // the wave's two query tiles: Q fragments and the running softmax state
  bf16x8 qf[2][KC];
  float m[2], l[2];
  f32x4 o[2][DT];
#pragma unroll
  for (int pass = 0; pass < 2; ++pass) {
    const int qt = pass ? 7 - wave : wave;
#pragma unroll
    for (int kc = 0; kc < KC; ++kc)
      qf[pass][kc] = attn_load8(qg, ld, 128 * qb + 16 * qt + i16,
                                32 * kc + 8 * g, L);
    m[pass] = ATTN_MASKED;
    l[pass] = 0.f;
#pragma unroll
    for (int dt = 0; dt < DT; ++dt) o[pass][dt] = {0.f, 0.f, 0.f, 0.f};
  }
  attn_long_commit<HD>(k_t, kr, tid);
  attn_long_commit<HD>(v_t, vr, tid);
  attn_barrier();

  for (int kb = 0; kb <= qb; ++kb) {
    const bool more = kb < qb, diag = kb == qb;
    if (more) {
      const int r0 = 128 * (kb + 1);
      attn_long_fetch<HD>(kr, qg + H + r0 * ld, ld, L - r0, tid);
      attn_long_fetch<HD>(vr, qg + 2 * H + r0 * ld, ld, L - r0, tid);
    }
#pragma unroll
    for (int pass = 0; pass < 2; ++pass) {
      const int qt = pass ? 7 - wave : wave;
      if (128 * qb + 16 * qt >= L) continue;
      // key tiles and keys (in the block) this query tile sees
      const int ktmax = diag ? qt : 7;
      const int lim = diag ? 16 * qt + i16 : ATTN_ROWS - 1;

      f32x4 s[8];
#pragma unroll
      for (int kt = 0; kt < 8; ++kt) {
        s[kt] = {0.f, 0.f, 0.f, 0.f};
        if (kt <= ktmax) {
#pragma unroll
          for (int kc = 0; kc < KC; ++kc)
            s[kt] = attn_mfma(attn_row_frag<HD>(k_t, kt, kc, lane),
                              qf[pass][kc], s[kt]);
        }
      }
      float bm = ATTN_MASKED;
#pragma unroll
      for (int kt = 0; kt < 8; ++kt)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float v =
              16 * kt + 4 * g + r <= lim ? s[kt][r] * G::scale : ATTN_MASKED;
          s[kt][r] = v;
          bm = __builtin_fmaxf(bm, v);
        }
      bm = __builtin_fmaxf(bm, attn_from(lane ^ 16, bm));
      bm = __builtin_fmaxf(bm, attn_from(lane ^ 32, bm));
      const float m_new = __builtin_fmaxf(m[pass], bm);
      const float alpha =
          __builtin_amdgcn_exp2f((m[pass] - m_new) * ATTN_LOG2E);
      m[pass] = m_new;
      float sum = 0.f;
#pragma unroll
      for (int kt = 0; kt < 8; ++kt)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float p =
              __builtin_amdgcn_exp2f((s[kt][r] - m_new) * ATTN_LOG2E);
          s[kt][r] = p;
          sum += p;
        }
      l[pass] = l[pass] * alpha + sum;
#pragma unroll
      for (int dt = 0; dt < DT; ++dt)
#pragma unroll
        for (int r = 0; r < 4; ++r) o[pass][dt][r] *= alpha;

      // O^T += V^T P^T
#pragma unroll
      for (int kc2 = 0; kc2 < 4; ++kc2) {
        if (2 * kc2 <= ktmax) {
          const bf16x8 pb = attn_pack8(s[2 * kc2], s[2 * kc2 + 1]);
#pragma unroll
          for (int dt = 0; dt < DT; ++dt)
            o[pass][dt] = attn_mfma(
                attn_tr_frag<HD>(v_t, troff[dt], 32 * kc2), pb, o[pass][dt]);
        }
      }
    }
    if (more) {
      attn_barrier();
      attn_long_commit<HD>(k_t, kr, tid);
      attn_long_commit<HD>(v_t, vr, tid);
      attn_barrier();
    }
  }

#pragma unroll
  for (int pass = 0; pass < 2; ++pass) {
    const int qt = pass ? 7 - wave : wave;
    if (128 * qb + 16 * qt >= L) continue;
    const int i = 128 * qb + 16 * qt + i16;
    float lt = l[pass];
    lt += attn_from(lane ^ 16, lt);
    lt += attn_from(lane ^ 32, lt);
    attn_store_rows<DT>(o[pass], __builtin_amdgcn_rcpf(lt),
                        att + ((int64_t)cb * L + i) * H + head * HD, i < L,
                        lane);
    if (g == 0 && i < L)
      lse[((int64_t)cb * heads + head) * L + i] =
          m[pass] + __builtin_amdgcn_logf(lt) * ATTN_LN2;
  }
}

// ---------------------------------------------------------------------------
// D[cb, head, i] = dO_i . O_i.  One thread per 16-byte pack of att, the
// HD/8 lanes of one (row, head) are consecutive and reduce by exchange.
template <int HD>
__global__ __launch_bounds__(ATTN_THREADS) void k_attn_long_dsum(
    const short* __restrict__ att, const short* __restrict__ datt,
    float* __restrict__ dsum, int64_t rows, int L, int heads) {
  constexpr int CH = HD / 8;
  const int tid = __builtin_amdgcn_workitem_id_x();
  const int lane = tid & 63;
  const int64_t p =
      (int64_t)__builtin_amdgcn_workgroup_id_x() * ATTN_THREADS + tid;
  const int ph = heads * CH;                  // packs of one row
  const int64_t row = p / ph;
  const int c = (int)(p - row * ph);
  float acc = 0.f;
  if (row < rows) {
    const bf16x8 of = *reinterpret_cast<const bf16x8*>(att + 8 * p);
    const bf16x8 dof = *reinterpret_cast<const bf16x8*>(datt + 8 * p);
#pragma unroll
    for (int e = 0; e < 8; ++e) acc += attn_val(dof[e]) * attn_val(of[e]);
  }
#pragma unroll
  for (int x = 1; x < CH; x <<= 1) acc += attn_from(lane ^ x, acc);
  if (row < rows && c % CH == 0) {
    const int64_t cb = row / L;
    dsum[(cb * heads + c / CH) * L + (row - cb * L)] = acc;
  }
}

template <int HD>
__global__ __launch_bounds__(ATTN_THREADS) void k_attn_long_bwd(
    const short* __restrict__ qkv, const short* __restrict__ datt,
    const float* __restrict__ lse, const float* __restrict__ dsum,
    short* __restrict__ dqkv, int L, int heads, int nb, int CBH) {
  using G = AttnGeom<HD>;
  constexpr int KC = G::KC, DT = G::DT;
  __shared__ __align__(16) short t0[ATTN_ROWS * HD];
  __shared__ __align__(16) short t1[ATTN_ROWS * HD];
  __shared__ float ld_l[2 * ATTN_ROWS];       // lse | D of a query block

  const int tid = __builtin_amdgcn_workitem_id_x();
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int i16 = lane & 15, g = lane >> 4;
  const int bid = __builtin_amdgcn_workgroup_id_x();
  const int b = bid / CBH;
  const int ch = bid % CBH;
  const int cb = ch / heads, head = ch - cb * heads;
  const int H = heads * HD;
  const int64_t ld = 3 * (int64_t)H;
  const int64_t row0 = (int64_t)cb * L;
  const short* qg = qkv + row0 * ld + head * HD;
  const short* dog = datt + row0 * H + head * HD;
  short* dqg = dqkv + row0 * ld + head * HD;
  const float* lse_g = lse + ((int64_t)cb * heads + head) * L;
  const float* d_g = dsum + ((int64_t)cb * heads + head) * L;

  int troff[DT];
#pragma unroll
  for (int dt = 0; dt < DT; ++dt)
    troff[dt] = attn_off<HD>(4 * g + ((lane >> 2) & 3),
                                16 * dt + 4 * (lane & 3));
  bf16x8 ra[HD / 16], rb[HD / 16];

  // ---- phase A: query block b, key blocks 0..b, dQ ------------------------
  {
    const short* k_t = t0;
    const short* v_t = t1;
    attn_long_fetch<HD>(ra, qg + H, ld, L, tid);
    attn_long_fetch<HD>(rb, qg + 2 * H, ld, L, tid);
    bf16x8 qf[2][KC], dof[2][KC];
    float lse_i[2], d_i[2];
    f32x4 dq[2][DT];
#pragma unroll
    for (int pass = 0; pass < 2; ++pass) {
      const int i = 128 * b + 16 * (pass ? 7 - wave : wave) + i16;
#pragma unroll
      for (int kc = 0; kc < KC; ++kc) {
        qf[pass][kc] = attn_load8(qg, ld, i, 32 * kc + 8 * g, L);
        dof[pass][kc] = attn_load8(dog, H, i, 32 * kc + 8 * g, L);
      }
      lse_i[pass] = i < L ? lse_g[i] : 0.f;
      d_i[pass] = i < L ? d_g[i] : 0.f;
#pragma unroll
      for (int dt = 0; dt < DT; ++dt) dq[pass][dt] = {0.f, 0.f, 0.f, 0.f};
    }
    attn_long_commit<HD>(t0, ra, tid);
    attn_long_commit<HD>(t1, rb, tid);
    attn_barrier();

    for (int kb = 0; kb <= b; ++kb) {
      const bool more = kb < b, diag = kb == b;
      if (more) {
        const int r0 = 128 * (kb + 1);
        attn_long_fetch<HD>(ra, qg + H + r0 * ld, ld, L - r0, tid);
        attn_long_fetch<HD>(rb, qg + 2 * H + r0 * ld, ld, L - r0, tid);
      }
#pragma unroll
      for (int pass = 0; pass < 2; ++pass) {
        const int qt = pass ? 7 - wave : wave;
        if (128 * b + 16 * qt >= L) continue;
        const int ktmax = diag ? qt : 7;
        const int lim = diag ? 16 * qt + i16 : ATTN_ROWS - 1;
        for (int kc2 = 0; 2 * kc2 <= ktmax; ++kc2) {
          f32x4 dsv[2];
#pragma unroll
          for (int h = 0; h < 2; ++h) {
            const int kt = 2 * kc2 + h;
            f32x4 s = {0.f, 0.f, 0.f, 0.f}, dp = {0.f, 0.f, 0.f, 0.f};
            if (kt <= ktmax) {
#pragma unroll
              for (int kc = 0; kc < KC; ++kc) {
                s = attn_mfma(attn_row_frag<HD>(k_t, kt, kc, lane),
                              qf[pass][kc], s);
                dp = attn_mfma(attn_row_frag<HD>(v_t, kt, kc, lane),
                               dof[pass][kc], dp);
              }
            }
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              float p, ds;
              attn_p_ds(s[r], dp[r], G::scale, 16 * kt + 4 * g + r <= lim,
                        lse_i[pass], d_i[pass], p, ds);
              dsv[h][r] = ds;
            }
          }
          const bf16x8 dsb = attn_pack8(dsv[0], dsv[1]);
#pragma unroll
          for (int dt = 0; dt < DT; ++dt)
            dq[pass][dt] = attn_mfma(
                attn_tr_frag<HD>(k_t, troff[dt], 32 * kc2), dsb, dq[pass][dt]);
        }
      }
      attn_barrier();                 // also ends phase A's use of the tiles
      if (more) {
        attn_long_commit<HD>(t0, ra, tid);
        attn_long_commit<HD>(t1, rb, tid);
        attn_barrier();
      }
    }
#pragma unroll
    for (int pass = 0; pass < 2; ++pass) {
      const int qt = pass ? 7 - wave : wave;
      if (128 * b + 16 * qt >= L) continue;
      const int i = 128 * b + 16 * qt + i16;
      attn_store_rows<DT>(dq[pass], G::scale, dqg + i * ld, i < L, lane);
    }
  }

  // ---- phase B: key block b, query blocks b..nb-1, dK and dV --------------
  {
    const short* q_t = t0;
    const short* do_t = t1;
    const float* lse_l = ld_l;
    const float* d_l = ld_l + ATTN_ROWS;
    // thread t < 128 carries lse of row t of the block, the others D
    const float* sc_g = tid < ATTN_ROWS ? lse_g : d_g;
    const int sc_row = tid & (ATTN_ROWS - 1);
    attn_long_fetch<HD>(ra, qg + 128 * b * ld, ld, L - 128 * b, tid);
    attn_long_fetch<HD>(rb, dog + 128 * b * (int64_t)H, H, L - 128 * b, tid);
    float sc = 128 * b + sc_row < L ? sc_g[128 * b + sc_row] : 0.f;

    bf16x8 kf[2][KC], vf[2][KC];
    f32x4 dk[2][DT], dv[2][DT];
#pragma unroll
    for (int pass = 0; pass < 2; ++pass) {
      const int j = 128 * b + 16 * (pass ? 7 - wave : wave) + i16;
#pragma unroll
      for (int kc = 0; kc < KC; ++kc) {
        kf[pass][kc] = attn_load8(qg + H, ld, j, 32 * kc + 8 * g, L);
        vf[pass][kc] = attn_load8(qg + 2 * H, ld, j, 32 * kc + 8 * g, L);
      }
#pragma unroll
      for (int dt = 0; dt < DT; ++dt) {
        dk[pass][dt] = {0.f, 0.f, 0.f, 0.f};
        dv[pass][dt] = {0.f, 0.f, 0.f, 0.f};
      }
    }
    attn_long_commit<HD>(t0, ra, tid);
    attn_long_commit<HD>(t1, rb, tid);
    ld_l[tid] = sc;
    attn_barrier();

    for (int ib = b; ib < nb; ++ib) {
      const bool more = ib + 1 < nb, diag = ib == b;
      if (more) {
        const int r0 = 128 * (ib + 1);
        attn_long_fetch<HD>(ra, qg + r0 * ld, ld, L - r0, tid);
        attn_long_fetch<HD>(rb, dog + r0 * (int64_t)H, H, L - r0, tid);
        sc = r0 + sc_row < L ? sc_g[r0 + sc_row] : 0.f;
      }
      // live 16-row tiles of this query block
      const int left = (L - 128 * ib + 15) >> 4;
      const int ntb = left < 8 ? left : 8;
#pragma unroll
      for (int pass = 0; pass < 2; ++pass) {
        const int jt = pass ? 7 - wave : wave;
        if (128 * b + 16 * jt >= L) continue;
        const int jl = 16 * jt + i16;
        const int it0 = diag ? jt : 0;        // first tile at or below j
        const int jlim = diag ? jl : 0;       // queries (in the block) >= this
        for (int kc2 = it0 >> 1; 2 * kc2 < ntb; ++kc2) {
          f32x4 pv[2], dsv[2];
#pragma unroll
          for (int h = 0; h < 2; ++h) {
            const int it = 2 * kc2 + h;
            f32x4 s = {0.f, 0.f, 0.f, 0.f}, dp = {0.f, 0.f, 0.f, 0.f};
            const bool tile_live = it >= it0 && it < ntb;
            if (tile_live) {
#pragma unroll
              for (int kc = 0; kc < KC; ++kc) {
                s = attn_mfma(attn_row_frag<HD>(q_t, it, kc, lane),
                              kf[pass][kc], s);
                dp = attn_mfma(attn_row_frag<HD>(do_t, it, kc, lane),
                               vf[pass][kc], dp);
              }
            }
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              const int il = 16 * it + 4 * g + r;
              const bool live =
                  tile_live && jlim <= il && 128 * ib + il < L;
              float p, ds;
              attn_p_ds(s[r], dp[r], G::scale, live, live ? lse_l[il] : 0.f,
                        live ? d_l[il] : 0.f, p, ds);
              pv[h][r] = p;
              dsv[h][r] = ds;
            }
          }
          const bf16x8 pb = attn_pack8(pv[0], pv[1]);
          const bf16x8 dsb = attn_pack8(dsv[0], dsv[1]);
#pragma unroll
          for (int dt = 0; dt < DT; ++dt) {
            dv[pass][dt] = attn_mfma(
                attn_tr_frag<HD>(do_t, troff[dt], 32 * kc2), pb, dv[pass][dt]);
            dk[pass][dt] = attn_mfma(
                attn_tr_frag<HD>(q_t, troff[dt], 32 * kc2), dsb, dk[pass][dt]);
          }
        }
      }
      if (more) {
        attn_barrier();
        attn_long_commit<HD>(t0, ra, tid);
        attn_long_commit<HD>(t1, rb, tid);
        ld_l[tid] = sc;
        attn_barrier();
      }
    }
#pragma unroll
    for (int pass = 0; pass < 2; ++pass) {
      const int jt = pass ? 7 - wave : wave;
      if (128 * b + 16 * jt >= L) continue;
      const int j = 128 * b + 16 * jt + i16;
      attn_store_rows<DT>(dk[pass], G::scale, dqg + H + j * ld, j < L, lane);
      attn_store_rows<DT>(dv[pass], 1.f, dqg + 2 * H + j * ld, j < L, lane);
    }
  }
}

#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute pop
#endif

// ---------------------------------------------------------------------------
extern "C" const char* ols_attn_long_route(int L, int HD, int is_bf16,
                                           int aligned) {
  return attn_route_name(attn_long_route(L, HD, is_bf16 != 0, aligned != 0));
}

static bool attn_long_aligned(std::initializer_list<const void*> ptrs) {
  for (const void* p : ptrs)
    if (reinterpret_cast<uintptr_t>(p) % 16 != 0) return false;
  return true;
}

extern "C" int ols_attn_long_fwd(const void* qkv, void* att, float* lse,
                                 int CB, int L, int heads, int HD,
                                 hipStream_t stream) {
  if (attn_long_route(L, HD, true, attn_long_aligned({qkv, att, lse})) !=
      ATTN_LONG)
    return 1;
  const int nb = (L + ATTN_ROWS - 1) / ATTN_ROWS;
  const int64_t grid = (int64_t)CB * heads * nb;
  if (grid >= (int64_t(1) << 31)) return 1;
  if (grid == 0) return 0;
  if (HD == 64)
    hipLaunchKernelGGL(k_attn_long_fwd<64>, dim3((unsigned)grid),
                       dim3(ATTN_THREADS), 0, stream, (const short*)qkv,
                       (short*)att, lse, L, heads, nb, CB * heads);
  else
    hipLaunchKernelGGL(k_attn_long_fwd<32>, dim3((unsigned)grid),
                       dim3(ATTN_THREADS), 0, stream, (const short*)qkv,
                       (short*)att, lse, L, heads, nb, CB * heads);
  return 0;
}

extern "C" int ols_attn_long_bwd(const void* qkv, const void* att,
                                 const void* datt, const float* lse,
                                 float* dsum, void* dqkv, int CB, int L,
                                 int heads, int HD, hipStream_t stream) {
  if (attn_long_route(L, HD, true,
                      attn_long_aligned({qkv, att, datt, lse, dsum, dqkv})) !=
      ATTN_LONG)
    return 1;
  const int nb = (L + ATTN_ROWS - 1) / ATTN_ROWS;
  const int64_t grid = (int64_t)CB * heads * nb;
  const int64_t rows = (int64_t)CB * L;
  const int64_t dgrid =
      (rows * heads * (HD / 8) + ATTN_THREADS - 1) / ATTN_THREADS;
  if (grid >= (int64_t(1) << 31) || dgrid >= (int64_t(1) << 31)) return 1;
  if (grid == 0) return 0;
  if (HD == 64) {
    hipLaunchKernelGGL(k_attn_long_dsum<64>, dim3((unsigned)dgrid),
                       dim3(ATTN_THREADS), 0, stream, (const short*)att,
                       (const short*)datt, dsum, rows, L, heads);
    hipLaunchKernelGGL(k_attn_long_bwd<64>, dim3((unsigned)grid),
                       dim3(ATTN_THREADS), 0, stream, (const short*)qkv,
                       (const short*)datt, lse, (const float*)dsum,
                       (short*)dqkv, L, heads, nb, CB * heads);
  } else {
    hipLaunchKernelGGL(k_attn_long_dsum<32>, dim3((unsigned)dgrid),
                       dim3(ATTN_THREADS), 0, stream, (const short*)att,
                       (const short*)datt, dsum, rows, L, heads);
    hipLaunchKernelGGL(k_attn_long_bwd<32>, dim3((unsigned)grid),
                       dim3(ATTN_THREADS), 0, stream, (const short*)qkv,
                       (const short*)datt, lse, (const float*)dsum,
                       (short*)dqkv, L, heads, nb, CB * heads);
  }
  return 0;
}
