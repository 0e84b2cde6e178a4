// The tied LM head's cross-entropy between its GEMMs, for gfx950.
//
// models/bert.py _TiedHeadCE walks the vocabulary in slices [s0, s0 + s).
// Per slice a hipBLASLt bmm writes the bf16 logits tile [C, N, s]; what
// follows used to be a dozen library passes over that tile and is here one
// kernel per direction, each reading the tile once:
//   k_head_ce_stats  folds the slice into the per-row online-softmax state
//                    m (running maximum), l (sum of exp(z - m)) and zy (the
//                    label's logit), in place, fp32 [C, N];
//   k_head_ce_grad   turns the recomputed tile into dlogits = bf16(g * (p -
//                    onehot)), p = exp(z - lse), lse = m + log l, and writes
//                    dbias[c, s0 .. s0 + s), the column sums over the N rows.
// z = float(logit) + float(bias[c, s0 + j]) in fp32 throughout, as the torch
// route computes it.
//
// VEC.  A lane moves the tile in packs of VEC elements: 8 (16 bytes) when s
// is a multiple of 8, 2 when it is even, 1 otherwise (head_ce_route.h); the
// tile's base is 16-byte aligned and its rows follow each other without
// padding, so VEC | s puts every row on a pack boundary and makes every pack
// whole: a pack is inside the slice or outside it.  The bias strip bias + c *
// stride + s0 has whatever alignment V, c and s0 leave it (stride 0: one bias
// for every client), and is 1/N of the bytes: it is read in 2-byte elements,
// or 4-byte pairs where the strip starts on one, never in wider packs.
//
// STATS: one workgroup of four waves takes 16 rows of one client, a wave
// four of them; grid (ceil(N / 16), C).  The columns go by in chunks of 128 *
// VEC (two packs a lane).  The workgroup stages the chunk's bias as fp32 in
// LDS, double-buffered so that one barrier a chunk is enough: chunk k + 1 is
// written while chunk k is read, and the barrier that ends k separates both
// from k + 2 and k + 1.  A lane takes its two packs of bias from LDS into
// registers once per chunk and uses them for its wave's four rows, which is
// why a wave owns four rows and not one: the staging (a 2-byte load per
// element) and the LDS reads are shared by 16 and by 4 rows.  Per row a lane
// keeps an online (m, l) pair over its own packs and rescales l once per
// chunk, by exp(m_old - m_new), not per element.  After the last chunk the
// wave reduces (m, l) by butterfly (ds_bpermute), lane 0 merges the result
// with the state of the earlier slices and stores it; the one lane whose pack
// holds column label - s0 has kept that z, and the wave's sum of it (zeros
// elsewhere, so exact) is zy.  The state starts at m = -inf, l = 0: every
// rescale factor is taken as 1 where old and new maximum are equal, so -inf -
// -inf is never formed, and exp2(-inf) = 0 covers a first slice.
//
// GRAD: one workgroup owns one client and one strip of 64 * VEC columns;
// grid (ceil(s / (64 VEC)), C).  A lane holds the bias of its VEC columns and
// VEC fp32 column sums in registers for the whole kernel.  The four waves
// take rows w, w + 4, ..., four at a time so that four loads are in flight
// per lane; m, l and the label of a row are the same address in every lane.
// Each lane reads its own elements before it writes them and no other lane
// touches them, so the output may be the input tile itself.  dbias sums the
// ROUNDED bf16 dlogits (what the torch route's dlogits.sum(dim=1) sums) in
// fp32, rows in ascending order per wave, then the four waves' sums through
// LDS as ((w0 + w1) + w2) + w3: no atomics, bit-identical between runs.
//
// exp and log are the hardware's v_exp_f32 and v_log_f32 (base 2, one ulp)
// with the base change as an fp32 multiplication; the exponent is formed as
// (z - m) * log2e, whose error shrinks with |z - m| and not with |m|.  Tests
// pass intrinsic=True to the bounds.
//
// Sizes: s < 2^30 so that column indices stay in int; C <= 65535 (grid y).
// Every row and element offset is 64-bit.

#include "common.h"
#include "head_ce_route.h"
#include "ols_ops.h"

#define HCE_THREADS 256
#define HCE_WAVES 4
#define HCE_ROWS 4      // stats: rows per wave
#define HCE_PACKS 2     // stats: packs per lane and chunk
#define HCE_UNROLL 4    // grad: rows in flight per wave
#define HCE_LOG2E 1.44269504088896341f
#define HCE_LN2 0.693147180559945309f

// Compiled without packed fp32 arithmetic (v_pk_*_f32), as lstm.hip and
// attn.hip: a function with another target feature set is not inlined, so
// everything the kernels call is defined here on compiler builtins.
#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute push(__attribute__((target("no-packed-fp32-ops"))), \
                             apply_to = function)
#endif

// VEC bf16 as one load or store of 2 * VEC bytes
template <int VEC>
struct __attribute__((aligned(2 * VEC))) HcePack {
  unsigned short e[VEC];
};

__device__ __forceinline__ float hce_val(unsigned short b) {
  return __builtin_bit_cast(float, ((unsigned)b) << 16);
}
// round-to-nearest-even bf16 bits of a finite fp32
__device__ __forceinline__ unsigned short hce_bits(float v) {
  const unsigned u = __builtin_bit_cast(unsigned, v);
  return (unsigned short)((u + 0x7FFFu + ((u >> 16) & 1u)) >> 16);
}
__device__ __forceinline__ float hce_exp(float x) {
  return __builtin_amdgcn_exp2f(x * HCE_LOG2E);
}
// exp(a - b) for a <= b, and 1 where they are equal, -inf included
__device__ __forceinline__ float hce_rescale(float a, float b) {
  return a == b ? 1.f : hce_exp(a - b);
}
__device__ __forceinline__ float hce_xor(float v, int lane, int off) {
  return __builtin_bit_cast(
      float, __builtin_amdgcn_ds_bpermute((lane ^ off) << 2,
                                          __builtin_bit_cast(int, v)));
}
// Both need EXEC all ones: called under wave-uniform control flow only.
__device__ __forceinline__ float hce_wave_max(float v, int lane) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v = fmaxf(v, hce_xor(v, lane, off));
  return v;
}
__device__ __forceinline__ float hce_wave_sum(float v, int lane) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += hce_xor(v, lane, off);
  return v;
}
__device__ __forceinline__ void hce_barrier() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __builtin_amdgcn_s_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}
// label - s0 where the label is in the slice, -1 elsewhere
__device__ __forceinline__ int hce_label(int64_t label, int64_t s0, int s) {
  const int64_t t = label - s0;
  return t >= 0 && t < s ? (int)t : -1;
}

// n elements of the bias strip src as fp32 into dst, by the whole workgroup
__device__ __forceinline__ void hce_stage_bias(const unsigned short* src,
                                               float* dst, int n, bool pairs,
                                               int tid) {
  if (pairs) {      // src on a 4-byte boundary
    for (int j = 2 * tid; j < n; j += 2 * HCE_THREADS) {
      if (j + 1 < n) {
        const unsigned w = *reinterpret_cast<const unsigned*>(src + j);
        dst[j] = __builtin_bit_cast(float, w << 16);
        dst[j + 1] = __builtin_bit_cast(float, w & 0xFFFF0000u);
      } else {
        dst[j] = hce_val(src[j]);
      }
    }
  } else {
    for (int j = tid; j < n; j += HCE_THREADS) dst[j] = hce_val(src[j]);
  }
}

// ---------------------------------------------------------------------------
template <int VEC>
__global__ __launch_bounds__(HCE_THREADS) void k_head_ce_stats(
    const unsigned short* __restrict__ logits,
    const unsigned short* __restrict__ bias, int64_t bias_stride,
    const int64_t* __restrict__ labels, float* __restrict__ m,
    float* __restrict__ l, float* __restrict__ zy, int N, int s, int64_t s0) {
  constexpr int CHUNK = 64 * VEC * HCE_PACKS;
  __shared__ float sbias[2][CHUNK];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int c = blockIdx.y;
  const int row0 = (blockIdx.x * HCE_WAVES + wave) * HCE_ROWS;
  const int64_t rbase = (int64_t)c * N + row0;
  const unsigned short* strip = bias + c * bias_stride + s0;
  const bool pairs = reinterpret_cast<uintptr_t>(strip) % 4 == 0;

  float mr[HCE_ROWS], lr[HCE_ROWS], zr[HCE_ROWS];
  int lab[HCE_ROWS];
#pragma unroll
  for (int i = 0; i < HCE_ROWS; ++i) {
    mr[i] = -INFINITY;
    lr[i] = 0.f;
    zr[i] = 0.f;
    lab[i] = row0 + i < N ? hce_label(labels[rbase + i], s0, s) : -1;
  }

  const int nchunks = (s + CHUNK - 1) / CHUNK;
  hce_stage_bias(strip, sbias[0], min(CHUNK, s), pairs, tid);
  hce_barrier();
  for (int k = 0; k < nchunks; ++k) {
    const int c0 = k * CHUNK;
    if (k + 1 < nchunks)
      hce_stage_bias(strip + c0 + CHUNK, sbias[(k + 1) & 1],
                     min(CHUNK, s - c0 - CHUNK), pairs, tid);
    int col[HCE_PACKS];
    bool ok[HCE_PACKS];
    float bv[HCE_PACKS][VEC];
#pragma unroll
    for (int u = 0; u < HCE_PACKS; ++u) {
      const int at = (u * 64 + lane) * VEC;
      col[u] = c0 + at;
      ok[u] = col[u] < s;
#pragma unroll
      for (int j = 0; j < VEC; ++j) bv[u][j] = ok[u] ? sbias[k & 1][at + j] : 0.f;
    }
#pragma unroll
    for (int i = 0; i < HCE_ROWS; ++i) {
      if (row0 + i >= N) continue;                       // wave-uniform
      const unsigned short* rp = logits + (rbase + i) * s;
      HcePack<VEC> raw[HCE_PACKS];
#pragma unroll
      for (int u = 0; u < HCE_PACKS; ++u)
        if (ok[u]) raw[u] = *reinterpret_cast<const HcePack<VEC>*>(rp + col[u]);
      float z[HCE_PACKS][VEC];
      float cm = -INFINITY;
#pragma unroll
      for (int u = 0; u < HCE_PACKS; ++u) {
        if (!ok[u]) continue;
#pragma unroll
        for (int j = 0; j < VEC; ++j) {
          z[u][j] = hce_val(raw[u].e[j]) + bv[u][j];
          cm = fmaxf(cm, z[u][j]);
          if (col[u] + j == lab[i]) zr[i] = z[u][j];
        }
      }
      if (ok[0]) {                  // a lane's second pack follows its first
        const float mn = fmaxf(mr[i], cm);
        float sum = 0.f;
#pragma unroll
        for (int u = 0; u < HCE_PACKS; ++u) {
          if (!ok[u]) continue;
#pragma unroll
          for (int j = 0; j < VEC; ++j) sum += hce_exp(z[u][j] - mn);
        }
        lr[i] = lr[i] * hce_rescale(mr[i], mn) + sum;
        mr[i] = mn;
      }
    }
    hce_barrier();
  }

#pragma unroll
  for (int i = 0; i < HCE_ROWS; ++i) {
    if (row0 + i >= N) continue;                         // wave-uniform
    const float mw = hce_wave_max(mr[i], lane);
    const float lw = hce_wave_sum(lr[i] * hce_rescale(mr[i], mw), lane);
    const float zw = hce_wave_sum(zr[i], lane);
    if (lane == 0) {
      const float mg = m[rbase + i], lg = l[rbase + i];
      const float mn = fmaxf(mg, mw);
      l[rbase + i] = lg * hce_rescale(mg, mn) + lw * hce_rescale(mw, mn);
      m[rbase + i] = mn;
      if (lab[i] >= 0) zy[rbase + i] = zw;
    }
  }
}

// ---------------------------------------------------------------------------
// logits and out are the same tile or two tiles apart: no __restrict__
template <int VEC>
__global__ __launch_bounds__(HCE_THREADS) void k_head_ce_grad(
    const unsigned short* logits, unsigned short* out,
    const unsigned short* __restrict__ bias, int64_t bias_stride,
    const int64_t* __restrict__ labels, const float* __restrict__ m,
    const float* __restrict__ l, const float* __restrict__ g,
    unsigned short* __restrict__ dbias, int64_t V, int N, int s, int64_t s0) {
  constexpr int STRIP = 64 * VEC;
  __shared__ float part[HCE_WAVES][STRIP];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int c = blockIdx.y;
  const int col = blockIdx.x * STRIP + lane * VEC;
  const bool ok = col < s;
  const float gg = g[0];

  float bv[VEC], acc[VEC];
#pragma unroll
  for (int j = 0; j < VEC; ++j) {
    bv[j] = ok ? hce_val(bias[c * bias_stride + s0 + col + j]) : 0.f;
    acc[j] = 0.f;
  }

  for (int r0 = wave; r0 < N; r0 += HCE_WAVES * HCE_UNROLL) {
    HcePack<VEC> raw[HCE_UNROLL];
#pragma unroll
    for (int i = 0; i < HCE_UNROLL; ++i) {
      const int r = r0 + HCE_WAVES * i;
      if (r < N && ok)
        raw[i] = *reinterpret_cast<const HcePack<VEC>*>(
            logits + ((int64_t)c * N + r) * s + col);
    }
#pragma unroll
    for (int i = 0; i < HCE_UNROLL; ++i) {
      const int r = r0 + HCE_WAVES * i;
      if (r >= N || !ok) continue;
      const int64_t idx = (int64_t)c * N + r;
      const float lse = m[idx] + __builtin_amdgcn_logf(l[idx]) * HCE_LN2;
      const int lab = hce_label(labels[idx], s0, s);
      HcePack<VEC> d;
#pragma unroll
      for (int j = 0; j < VEC; ++j) {
        const float p = hce_exp(hce_val(raw[i].e[j]) + bv[j] - lse);
        d.e[j] = hce_bits(gg * (p - (col + j == lab ? 1.f : 0.f)));
        acc[j] += hce_val(d.e[j]);
      }
      *reinterpret_cast<HcePack<VEC>*>(out + idx * s + col) = d;
    }
  }

#pragma unroll
  for (int j = 0; j < VEC; ++j) part[wave][lane * VEC + j] = acc[j];
  hce_barrier();
  for (int j = tid; j < STRIP; j += HCE_THREADS) {
    const int cc = blockIdx.x * STRIP + j;
    if (cc < s)
      dbias[c * V + s0 + cc] =
          hce_bits(((part[0][j] + part[1][j]) + part[2][j]) + part[3][j]);
  }
}

#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute pop
#endif

// ---------------------------------------------------------------------------
extern "C" const char* ols_head_ce_route(int64_t s, int is_bf16,
                                         int aligned) {
  return head_ce_route_name(head_ce_route(s, is_bf16 != 0, aligned != 0));
}

static bool hce_aligned(const void* p) {
  return reinterpret_cast<uintptr_t>(p) % 16 == 0;
}

// what the kernels' index arithmetic holds: s below 2^30, C a grid y
static bool hce_sizes_ok(int C, int N, int s) {
  return C >= 0 && C <= 65535 && N >= 1 && s >= 1 && s < (1 << 30);
}

#define HCE_LAUNCH_STATS(VEC)                                               \
  hipLaunchKernelGGL(k_head_ce_stats<VEC>,                                  \
                     dim3((N + HCE_WAVES * HCE_ROWS - 1) /                  \
                              (HCE_WAVES * HCE_ROWS), C),                   \
                     dim3(HCE_THREADS), 0, stream,                          \
                     (const unsigned short*)logits,                         \
                     (const unsigned short*)bias, bias_stride, labels, m, l, \
                     zy, N, s, s0)

extern "C" int ols_head_ce_stats(const void* logits, const void* bias,
                                 int64_t bias_stride, const int64_t* labels,
                                 float* m, float* l, float* zy, int C, int N,
                                 int s, int64_t s0, hipStream_t stream) {
  const HeadCeRoute r = head_ce_route(s, true, hce_aligned(logits));
  if (r == HEAD_CE_TORCH || !hce_sizes_ok(C, N, s)) return 1;
  if (C == 0) return 0;
  if (r == HEAD_CE_FUSED8) HCE_LAUNCH_STATS(8);
  else if (r == HEAD_CE_FUSED2) HCE_LAUNCH_STATS(2);
  else HCE_LAUNCH_STATS(1);
  return 0;
}

#define HCE_LAUNCH_GRAD(VEC)                                                \
  hipLaunchKernelGGL(k_head_ce_grad<VEC>,                                   \
                     dim3((s + 64 * VEC - 1) / (64 * VEC), C),              \
                     dim3(HCE_THREADS), 0, stream,                          \
                     (const unsigned short*)logits, (unsigned short*)out,   \
                     (const unsigned short*)bias, bias_stride, labels, m, l, \
                     g, (unsigned short*)dbias, V, N, s, s0)

extern "C" int ols_head_ce_grad(const void* logits, void* out,
                                const void* bias, int64_t bias_stride,
                                const int64_t* labels, const float* m,
                                const float* l, const float* g, void* dbias,
                                int64_t V, int C, int N, int s, int64_t s0,
                                hipStream_t stream) {
  const HeadCeRoute r =
      head_ce_route(s, true, hce_aligned(logits) && hce_aligned(out));
  if (r == HEAD_CE_TORCH || !hce_sizes_ok(C, N, s) || s0 < 0 || s0 + s > V)
    return 1;
  if (C == 0) return 0;
  if (r == HEAD_CE_FUSED8) HCE_LAUNCH_GRAD(8);
  else if (r == HEAD_CE_FUSED2) HCE_LAUNCH_GRAD(2);
  else HCE_LAUNCH_GRAD(1);
  return 0;
}
