// Fused per-client LSTM recurrence for gfx950.
//
// One layer of models/lstm.py after the input projection has been hoisted:
//   a_t = xp[:, :, t] + h_{t-1} W_hh          (i | f | g | o along 4H)
//   c_t = sig(a_f) c_{t-1} + sig(a_i) tanh(a_g),  h_t = sig(a_o) tanh(c_t)
// The C clients' recurrences are independent, so ONE WORKGROUP OWNS ONE
// CLIENT FOR ALL L TIMESTEPS: grid C, 256 threads, no synchronisation
// between workgroups.  h and c never leave the chip between steps; the
// only per-step HBM/L2 traffic is that client's W_hh, streamed once.
//
// Work split (both directions).  The batch is the M = 16 rows of one MFMA
// tile (rows b >= B are zero in LDS and masked on every global access).
// Wave w owns hidden units [w*H/4, (w+1)*H/4) in JT = H/64 column tiles
// of 16.  With the v_mfma_f32_16x16x32_bf16 C/D map (lane l, reg r -> row
// (l>>4)*4 + r, col l&15) the value of hidden unit j for batch row b sits
// in the same lane and register slot of every tile that has j as its
// column, so the i/f/g/o pre-activations of one (b, j) meet in one lane
// and the whole cell update is register-local; c_t (forward) and dc,
// dh_rec (backward) stay in fp32 VGPRs across all L steps.
//
// Forward, per step: the 4*JT accumulator tiles are seeded with xp[t]
// (step t+1's is prefetched behind the MFMAs), the h_{t-1} A-fragments
// come from LDS (bf16 [16][H], two buffers, one barrier per step), the
// B-fragments from a fragment-major copy of W_hh that k_lstm_wpack writes
// once per call: the native [H][4H] layout is n-contiguous where the MFMA
// wants 8 consecutive k per lane, and each W_hh element is used by
// exactly one wave once per step, so weights go global -> VGPR as one
// coalesced 16-byte load per lane, in double-buffered batches of LSTM_NB
// fragments, never through LDS.
//
// Backward, per step t = L-1 .. 0: dh = dhs[t] + dh_rec, the pointwise
// gate gradients from the saved gates / cs, dgates_t as bf16 to global
// and to LDS ([16][4H], the next GEMM's A operand), then dh_rec =
// dgates_t W_hh^T (M 16, N H, K 4H).  Its B-fragment B[k][j] = W_hh[j][k]
// is contiguous along 4H in the native layout: no packed copy.  The
// kernel produces only dgates, which is at once the gradient of xp and
// the right operand of dW_hh = h_prev^T dgates (one bmm, ops/lstm.py).

#include <initializer_list>

#include "common.h"
#include "lstm_route.h"
#include "ols_ops.h"

typedef __attribute__((ext_vector_type(8))) short bf16x8;
typedef __attribute__((ext_vector_type(4))) float f32x4;

#define LSTM_THREADS 256
#define LSTM_PAD 8   // bf16 of LDS row padding: 16 rows land on 16 banks
#define LSTM_NB 8    // B-fragments per weight batch (32 VGPRs)

// The two recurrence kernels are compiled without packed fp32 arithmetic
// (v_pk_*_f32); the rest of the extension keeps the default target.  A
// function with another target feature set is not inlined into them, so
// everything they call is defined here, on compiler builtins, and nothing
// from the HIP device headers is used between the push and the pop.
#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute push(__attribute__((target("no-packed-fp32-ops"))), \
                             apply_to = function)
#endif

// round-to-nearest-even bf16 bits of a finite or infinite fp32
__device__ __forceinline__ short lstm_bits(float v) {
  const unsigned u = __builtin_bit_cast(unsigned, v);
  return (short)((u + 0x7FFFu + ((u >> 16) & 1u)) >> 16);
}
__device__ __forceinline__ float lstm_val(short s) {
  return __builtin_bit_cast(float, ((unsigned)(unsigned short)s) << 16);
}
// exp2 overflow gives 1/inf = 0: both saturate cleanly
__device__ __forceinline__ float lstm_sig(float x) {
  return __builtin_amdgcn_rcpf(
      1.f + __builtin_amdgcn_exp2f(-1.44269504088896341f * x));
}
// 1 - 2/(1 + e^2x) cancels near 0, where its absolute error of a few
// 2^-24 is a large part of tanh x itself and would end up in the gradient
// of the output gate (dh * tanh c); below 1/4 the odd series to x^7 is
// within 4e-7 of tanh x, relative
__device__ __forceinline__ float lstm_tanh(float x) {
  const float big = 1.f - 2.f * __builtin_amdgcn_rcpf(
                              1.f + __builtin_amdgcn_exp2f(
                                        2.88539008177792681f * x));
  const float x2 = x * x;
  const float small =
      x * (1.f + x2 * (-0.333333333f +
                       x2 * (0.133333333f + x2 * -0.0539682540f)));
  return __builtin_fabsf(x) < 0.25f ? small : big;
}
__device__ __forceinline__ void lstm_barrier() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __builtin_amdgcn_s_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}
// The weight stream does not depend on t, and the compiler would hoist all
// of it out of the time loop into registers and scratch: an offset it
// cannot see through, renewed once per step, keeps the loads in the loop.
__device__ __forceinline__ int lstm_opaque(int off) {
  asm volatile("" : "+v"(off));
  return off;
}

// ---------------------------------------------------------------------------
// w [C][H][4H] -> wp, fragment-major: for client c, wave w, k-chunk kc and
// fragment f = gate*JT + jt, lane l's 8 values are
//   w[c][kc*32 + 8*(l>>4) + e][gate*H + w*H/4 + jt*16 + (l&15)],  e = 0..7
// at wp[((((c*4 + w)*KC + kc)*4*JT + f)*64 + l)*8 + e]: the order in which
// wave w of k_lstm_fwd consumes them, so its stream is one linear read.
__global__ __launch_bounds__(LSTM_THREADS) void k_lstm_wpack(
    const short* __restrict__ w, bf16x8* __restrict__ wp, int H,
    int64_t frags) {
  const int64_t i = (int64_t)__builtin_amdgcn_workgroup_id_x() * LSTM_THREADS +
                    __builtin_amdgcn_workitem_id_x();
  if (i >= frags) return;
  const int JT = H / 64, KC = H / 32, NF = 4 * JT;
  const int l = (int)(i & 63);
  int64_t q = i >> 6;
  const int f = (int)(q % NF);
  q /= NF;
  const int kc = (int)(q % KC);
  q /= KC;
  const int wv = (int)(q & 3);
  const int64_t c = q >> 2;
  const int n = (f / JT) * H + wv * (H / 4) + (f % JT) * 16 + (l & 15);
  const short* src =
      w + ((c * H + kc * 32 + 8 * (l >> 4)) * 4 * (int64_t)H) + n;
  bf16x8 v;
#pragma unroll
  for (int e = 0; e < 8; ++e) v[e] = src[(int64_t)e * 4 * H];
  wp[i] = v;
}

// ---------------------------------------------------------------------------
template <int JT>
__global__ __launch_bounds__(LSTM_THREADS) void k_lstm_fwd(
    const short* __restrict__ xp, const bf16x8* __restrict__ wp,
    short* __restrict__ hs, short* __restrict__ gates, float* __restrict__ cs,
    int B, int L) {
  constexpr int H = 64 * JT, KC = H / 32, NF = 4 * JT, LD = H + LSTM_PAD;
  constexpr int NBATCH = KC * NF / LSTM_NB;
  static_assert(KC * NF % LSTM_NB == 0, "whole weight batches");
  __shared__ __align__(16) short h_lds[2][16 * LD];

  const int c = __builtin_amdgcn_workgroup_id_x();
  const int tid = __builtin_amdgcn_workitem_id_x();
  const int lane = tid & 63, wave = tid >> 6;
  const int col = lane & 15, rq = lane >> 4;
  for (int i = tid; i < 2 * 16 * LD; i += LSTM_THREADS)
    (&h_lds[0][0])[i] = 0;

  // this wave's weight stream, and this lane's hidden unit of tile 0
  const bf16x8* wv = wp + (int64_t)(c * 4 + wave) * KC * NF * 64;
  int wo = lstm_opaque(lane);
  const int j0 = wave * (H / 4) + col;
  // element (c, b, t, j0) of the [.., H] tensors per register row; the
  // [.., 4H] tensors sit at four times that, less 3*j0.  It steps with t,
  // and everything else a step touches is a constant offset from it.
  // Rows b >= B alias row B-1: read like it (finite values whose results
  // are dropped), never written.
  int64_t o1[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int b = rq * 4 + r < B ? rq * 4 + r : B - 1;
    o1[r] = ((int64_t)c * B + b) * L * H + j0;
  }

  f32x4 cst[JT];
#pragma unroll
  for (int jt = 0; jt < JT; ++jt) cst[jt] = {0.f, 0.f, 0.f, 0.f};

  short xn[NF][4];
  auto load_xp = [&](int ahead) {   // of step t + ahead
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
      for (int f = 0; f < NF; ++f)
        xn[f][r] = xp[4 * o1[r] - 3 * j0 + ahead * 4 * H + (f / JT) * H +
                      (f % JT) * 16];
  };
  bf16x8 wr[2][LSTM_NB];
  auto load_w = [&](int bt, int buf) {
#pragma unroll
    for (int i = 0; i < LSTM_NB; ++i)
      wr[buf][i] = wv[wo + (bt * LSTM_NB + i) * 64];
  };
  load_xp(0);
  load_w(0, 0);
  lstm_barrier();

  for (int t = 0; t < L; ++t) {
    f32x4 acc[NF];
#pragma unroll
    for (int f = 0; f < NF; ++f)
#pragma unroll
      for (int r = 0; r < 4; ++r)
        // opaque, or the compiler converts where it loads and so waits
        // for the prefetch ahead of the MFMAs
        acc[f][r] = lstm_val((short)lstm_opaque((int)xn[f][r]));
    if (t + 1 < L) load_xp(1);

    const short* hb = h_lds[t & 1];
    bf16x8 a;
#pragma unroll
    for (int bt = 0; bt < NBATCH; ++bt) {
      // one batch in flight, no more: the fences keep the scheduler from
      // hoisting the whole unrolled stream into registers (it spills)
      __builtin_amdgcn_sched_barrier(0);
      if (bt + 1 < NBATCH) load_w(bt + 1, (bt + 1) & 1);
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int i = 0; i < LSTM_NB; ++i) {
        const int s = bt * LSTM_NB + i, kc = s / NF, f = s % NF;
        if (f == 0)
          a = *reinterpret_cast<const bf16x8*>(
              &hb[col * LD + kc * 32 + 8 * rq]);
        acc[f] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, wr[bt & 1][i],
                                                         acc[f], 0, 0, 0);
      }
    }
    // the next step's first batch flies behind the cell update
    wo = lstm_opaque(wo);
    if (t + 1 < L) load_w(0, 0);

    short* hn = h_lds[(t + 1) & 1];
#pragma unroll
    for (int jt = 0; jt < JT; ++jt)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float gi = lstm_sig(acc[jt][r]);
        const float gf = lstm_sig(acc[JT + jt][r]);
        const float gg = lstm_tanh(acc[2 * JT + jt][r]);
        const float go = lstm_sig(acc[3 * JT + jt][r]);
        const float cc = gf * cst[jt][r] + gi * gg;
        cst[jt][r] = cc;
        const short hv = lstm_bits(go * lstm_tanh(cc));
        const int b = rq * 4 + r, j = jt * 16;
        const bool live = b < B;
        hn[b * LD + j0 + j] = live ? hv : (short)0;
        if (live) {
          short* gp = gates + (4 * o1[r] - 3 * j0);
          gp[j] = lstm_bits(gi);
          gp[H + j] = lstm_bits(gf);
          gp[2 * H + j] = lstm_bits(gg);
          gp[3 * H + j] = lstm_bits(go);
          cs[o1[r] + j] = cc;
          hs[o1[r] + j] = hv;
        }
      }
#pragma unroll
    for (int r = 0; r < 4; ++r) o1[r] += H;
    lstm_barrier();
  }
}

// ---------------------------------------------------------------------------
template <int JT>
__global__ __launch_bounds__(LSTM_THREADS) void k_lstm_bwd(
    const short* __restrict__ dhs, const short* __restrict__ gates,
    const float* __restrict__ cs, const short* __restrict__ w,
    short* __restrict__ dgates, int B, int L) {
  constexpr int H = 64 * JT, K4 = 4 * H, KC = K4 / 32, LD = K4 + LSTM_PAD;
  constexpr int NBATCH = KC * JT / LSTM_NB;
  static_assert(KC * JT % LSTM_NB == 0, "whole weight batches");
  __shared__ __align__(16) short a_lds[16 * LD];

  const int c = __builtin_amdgcn_workgroup_id_x();
  const int tid = __builtin_amdgcn_workitem_id_x();
  const int lane = tid & 63, wave = tid >> 6;
  const int col = lane & 15, rq = lane >> 4;
  const int j0 = wave * (H / 4) + col;
  // B[k][j] = W_hh[j][k]: lane (col, rq) reads 8 consecutive k of row j
  const short* wl = w + (int64_t)c * H * K4;
  int wo = lstm_opaque(j0 * K4 + 8 * rq);
  // element (c, b, t = L-1, j0) of the [.., H] tensors per register row,
  // stepping down with t (k_lstm_fwd's o1)
  int64_t o1[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int b = rq * 4 + r < B ? rq * 4 + r : B - 1;
    o1[r] = (((int64_t)c * B + b) * L + L - 1) * H + j0;
  }

  f32x4 dhr[JT], dc[JT];
#pragma unroll
  for (int jt = 0; jt < JT; ++jt) {
    dhr[jt] = {0.f, 0.f, 0.f, 0.f};
    dc[jt] = {0.f, 0.f, 0.f, 0.f};
  }
  bf16x8 wr[2][LSTM_NB];
  auto load_w = [&](int bt, int buf) {
#pragma unroll
    for (int i = 0; i < LSTM_NB; ++i) {
      const int s = bt * LSTM_NB + i, kc = s / JT, jt = s % JT;
      wr[buf][i] = *reinterpret_cast<const bf16x8*>(
          wl + wo + jt * 16 * K4 + kc * 32);
    }
  };
  load_w(0, 0);

  for (int t = L - 1; t >= 0; --t) {
#pragma unroll
    for (int jt = 0; jt < JT; ++jt)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int b = rq * 4 + r, j = jt * 16;
        short d[4] = {0, 0, 0, 0};
        const short* gp = gates + (4 * o1[r] - 3 * j0);
        const float gi = lstm_val(gp[j]), gf = lstm_val(gp[H + j]);
        const float gg = lstm_val(gp[2 * H + j]);
        const float go = lstm_val(gp[3 * H + j]);
        const float cp = cs[o1[r] + (t > 0 ? j - H : j)];
        const float ct = cs[o1[r] + j];
        const float dh = lstm_val(dhs[o1[r] + j]) + dhr[jt][r];
        if (b < B) {
          const float tc = lstm_tanh(ct);
          const float dcv = dc[jt][r] + dh * go * (1.f - tc * tc);
          dc[jt][r] = dcv * gf;
          d[0] = lstm_bits(dcv * gg * gi * (1.f - gi));
          d[1] = lstm_bits(t > 0 ? dcv * cp * gf * (1.f - gf) : 0.f);
          d[2] = lstm_bits(dcv * gi * (1.f - gg * gg));
          d[3] = lstm_bits(dh * tc * go * (1.f - go));
#pragma unroll
          for (int g = 0; g < 4; ++g)
            dgates[4 * o1[r] - 3 * j0 + g * H + j] = d[g];
        }
#pragma unroll
        for (int g = 0; g < 4; ++g) a_lds[b * LD + g * H + j0 + j] = d[g];
      }
#pragma unroll
    for (int r = 0; r < 4; ++r) o1[r] -= H;
    if (t == 0) break;   // dh_rec of step 0 has no consumer
    lstm_barrier();

#pragma unroll
    for (int jt = 0; jt < JT; ++jt) dhr[jt] = {0.f, 0.f, 0.f, 0.f};
    bf16x8 a;
#pragma unroll
    for (int bt = 0; bt < NBATCH; ++bt) {
      __builtin_amdgcn_sched_barrier(0);
      if (bt + 1 < NBATCH) load_w(bt + 1, (bt + 1) & 1);
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int i = 0; i < LSTM_NB; ++i) {
        const int s = bt * LSTM_NB + i, kc = s / JT, jt = s % JT;
        if (jt == 0)
          a = *reinterpret_cast<const bf16x8*>(
              &a_lds[col * LD + kc * 32 + 8 * rq]);
        dhr[jt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, wr[bt & 1][i],
                                                          dhr[jt], 0, 0, 0);
      }
    }
    wo = lstm_opaque(wo);
    load_w(0, 0);
    lstm_barrier();
  }
}

#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute pop
#endif

// ---------------------------------------------------------------------------
extern "C" const char* ols_lstm_route(int B, int H, int is_bf16,
                                      int aligned) {
  return lstm_route_name(lstm_route(B, H, is_bf16 != 0, aligned != 0));
}

static bool lstm_aligned(std::initializer_list<const void*> ptrs) {
  for (const void* p : ptrs)
    if (reinterpret_cast<uintptr_t>(p) % 16 != 0) return false;
  return true;
}

extern "C" int ols_lstm_fwd(const void* xp, const void* w, void* wpack,
                            void* hs, void* gates, float* cs, int C, int B,
                            int L, int H, hipStream_t stream) {
  if (lstm_route(B, H, true, lstm_aligned({xp, w, wpack, hs, gates, cs})) !=
      LSTM_FUSED)
    return 1;
  if (C == 0 || L == 0) return 0;
  const int64_t frags = (int64_t)C * H * 4 * H / 8;
  hipLaunchKernelGGL(k_lstm_wpack, dim3(ols_grid(frags, LSTM_THREADS)),
                     dim3(LSTM_THREADS), 0, stream, (const short*)w,
                     (bf16x8*)wpack, H, frags);
#define LSTM_FWD(JT)                                                        \
  hipLaunchKernelGGL(k_lstm_fwd<JT>, dim3(C), dim3(LSTM_THREADS), 0,        \
                     stream, (const short*)xp, (const bf16x8*)wpack,        \
                     (short*)hs, (short*)gates, cs, B, L)
  switch (H / 64) {
    case 1: LSTM_FWD(1); break;
    case 2: LSTM_FWD(2); break;
    case 3: LSTM_FWD(3); break;
    default: LSTM_FWD(4); break;
  }
#undef LSTM_FWD
  return 0;
}

extern "C" int ols_lstm_bwd(const void* dhs, const void* gates,
                            const float* cs, const void* w, void* dgates,
                            int C, int B, int L, int H, hipStream_t stream) {
  if (lstm_route(B, H, true, lstm_aligned({dhs, gates, cs, w, dgates})) !=
      LSTM_FUSED)
    return 1;
  if (C == 0 || L == 0) return 0;
#define LSTM_BWD(JT)                                                        \
  hipLaunchKernelGGL(k_lstm_bwd<JT>, dim3(C), dim3(LSTM_THREADS), 0,        \
                     stream, (const short*)dhs, (const short*)gates, cs,    \
                     (const short*)w, (short*)dgates, B, L)
  switch (H / 64) {
    case 1: LSTM_BWD(1); break;
    case 2: LSTM_BWD(2); break;
    case 3: LSTM_BWD(3); break;
    default: LSTM_BWD(4); break;
  }
#undef LSTM_BWD
  return 0;
}
