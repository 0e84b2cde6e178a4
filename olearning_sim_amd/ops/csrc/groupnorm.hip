// Fused per-client GroupNorm (+ optional residual add + ReLU), forward
// and backward.
//
// The client-batched ResNet runs GroupNorm(8) after every conv
// (models/resnet.py).  Written as torch ops the normalisation is a
// ~6-kernel forward and ~15-kernel backward chain of large elementwise
// passes per layer — measured >50% of a round's GPU time (see
// profiles/).  Here it is ONE forward kernel and ONE backward kernel.
//
// Layout: x is the channel-grouped activation [B, C*ch, H, W]
// (contiguous), conceptually [B, C, G, ch/G, H, W]; a normalisation
// group (b, c, g) spans cg*HW CONTIGUOUS elements, so every group is a
// coalesced span.  gamma/beta are per-client affine [C, ch].
//
// fwd:  y = gn(x)*gamma + beta  [+ res]  [relu]
//       one workgroup per group (B*C*G workgroups >> 256 CUs);
//       pass 1 reduces sum/sumsq (wave + LDS), pass 2 re-reads x
//       (L1/L2-resident) and writes y; saves mean/rstd per group.
// bwd:  dx = rstd*(dxhat - mean(dxhat) - xhat*mean(dxhat*xhat)),
//       dxhat = relu-masked dy * gamma; per-channel dgamma/dbeta
//       partials reduced in LDS then one fp32 atomicAdd per channel.

#include "common.h"

template <typename T, bool HAS_RES, bool RELU, int LAYOUT>
__global__ __launch_bounds__(OLS_THREADS) void k_gn_fwd(
    const T* __restrict__ x, const T* __restrict__ res, T* __restrict__ y,
    float* __restrict__ mean_out, float* __restrict__ rstd_out,
    const T* __restrict__ gamma, const T* __restrict__ beta,
    int Bn, int C, int ch, int G, int HW, float eps) {
  const int cg = ch / G;
  const int n = cg * HW;
  const int group = blockIdx.x;
  int c, g;
  int64_t base, pstride;
  if (LAYOUT == 0) {          // group = (b, c, g); contiguous cg*HW span
    g = group % G;
    c = (group / G) % C;
    base = (int64_t)group * n;
    pstride = HW;
  } else {                    // group = (c, g, b); planes strided by B*HW
    const int b = group % Bn;
    g = (group / Bn) % G;
    c = group / (Bn * G);
    base = (((int64_t)c * ch + (int64_t)g * cg) * Bn + b) * HW;
    pstride = (int64_t)Bn * HW;
  }
  const T* xg = x + base;
  const T* rg = HAS_RES ? res + base : nullptr;
  T* yg = y + base;

  __shared__ float red[2][OLS_THREADS / WAVE];
  float s1 = 0.f, s2 = 0.f;
  // vector path: 8 elements (16 B) per lane per iteration — scalar bf16
  // loads measure 2-2.5x slower on gfx950 (cdna_hip_programming.md G13);
  // HW is a multiple of 8 for every model plane, so a vector never
  // crosses a plane (LAYOUT 1) or channel boundary
  const bool vec = (HW % 8) == 0;
  if (vec) {
    const int nv = n / 8;
    for (int v8 = threadIdx.x; v8 < nv; v8 += blockDim.x) {
      int i = v8 * 8;
      int64_t idx = (LAYOUT == 0) ? i : ((int64_t)(i / HW) * pstride + i % HW);
      Pack<T, 8> px = *reinterpret_cast<const Pack<T, 8>*>(&xg[idx]);
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        float v = to_f32(px.v[e]);
        s1 += v;
        s2 += v * v;
      }
    }
  } else {
    for (int i = threadIdx.x; i < n; i += blockDim.x) {
      int64_t idx = (LAYOUT == 0) ? i : ((int64_t)(i / HW) * pstride + i % HW);
      float v = to_f32(xg[idx]);
      s1 += v;
      s2 += v * v;
    }
  }
  s1 = wave_sum(s1);
  s2 = wave_sum(s2);
  const int wid = threadIdx.x / WAVE, nw = blockDim.x / WAVE;
  if ((threadIdx.x & (WAVE - 1)) == 0) { red[0][wid] = s1; red[1][wid] = s2; }
  __syncthreads();
  s1 = 0.f; s2 = 0.f;
  for (int w = 0; w < nw; ++w) { s1 += red[0][w]; s2 += red[1][w]; }
  const float mean = s1 / n;
  const float var = fmaxf(s2 / n - mean * mean, 0.f);
  const float rstd = rsqrtf(var + eps);
  if (threadIdx.x == 0) { mean_out[group] = mean; rstd_out[group] = rstd; }

  const T* gam = gamma + (int64_t)c * ch + g * cg;
  const T* bet = beta + (int64_t)c * ch + g * cg;
  if (vec) {
    const int nv = n / 8;
    for (int v8 = threadIdx.x; v8 < nv; v8 += blockDim.x) {
      int i = v8 * 8;
      int chan = i / HW;
      int64_t idx = (LAYOUT == 0) ? i : ((int64_t)chan * pstride + i % HW);
      Pack<T, 8> px = *reinterpret_cast<const Pack<T, 8>*>(&xg[idx]);
      Pack<T, 8> pr;
      if (HAS_RES) pr = *reinterpret_cast<const Pack<T, 8>*>(&rg[idx]);
      Pack<T, 8> py;
      const float ga = to_f32(gam[chan]), be = to_f32(bet[chan]);
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        float v = (to_f32(px.v[e]) - mean) * rstd;
        v = v * ga + be;
        if (HAS_RES) v += to_f32(pr.v[e]);
        if (RELU) v = fmaxf(v, 0.f);
        py.v[e] = from_f32<T>(v);
      }
      *reinterpret_cast<Pack<T, 8>*>(&yg[idx]) = py;
    }
  } else {
    for (int i = threadIdx.x; i < n; i += blockDim.x) {
      int chan = i / HW;                     // channel within the group
      int64_t idx = (LAYOUT == 0) ? i : ((int64_t)chan * pstride + i % HW);
      float v = (to_f32(xg[idx]) - mean) * rstd;
      v = v * to_f32(gam[chan]) + to_f32(bet[chan]);
      if (HAS_RES) v += to_f32(rg[idx]);
      if (RELU) v = fmaxf(v, 0.f);
      yg[idx] = from_f32<T>(v);
    }
  }
}


// One-global-pass forward: x is staged in LDS during the stats pass and
// replayed for the normalize pass (k_gn_fwd reads it twice).
template <typename T, bool HAS_RES, bool RELU, int LAYOUT>
__global__ __launch_bounds__(OLS_THREADS) void k_gn_fwd_lds(
    const T* __restrict__ x, const T* __restrict__ res, T* __restrict__ y,
    float* __restrict__ mean_out, float* __restrict__ rstd_out,
    const T* __restrict__ gamma, const T* __restrict__ beta,
    int Bn, int C, int ch, int G, int HW, float eps) {
  const int cg = ch / G;
  const int n = cg * HW;
  const int group = blockIdx.x;
  int c, g;
  int64_t base, pstride;
  if (LAYOUT == 0) {
    g = group % G;
    c = (group / G) % C;
    base = (int64_t)group * n;
    pstride = HW;
  } else {
    const int b = group % Bn;
    g = (group / Bn) % G;
    c = group / (Bn * G);
    base = (((int64_t)c * ch + (int64_t)g * cg) * Bn + b) * HW;
    pstride = (int64_t)Bn * HW;
  }
  const T* xg = x + base;
  const T* rg = HAS_RES ? res + base : nullptr;
  T* yg = y + base;

  extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
  Pack<T, 8>* xbuf = reinterpret_cast<Pack<T, 8>*>(lds_raw);

  __shared__ float red[2][OLS_THREADS / WAVE];
  float s1 = 0.f, s2 = 0.f;
  const int nv = n / 8;
  for (int v8 = threadIdx.x; v8 < nv; v8 += blockDim.x) {
    int i = v8 * 8;
    int64_t idx = (LAYOUT == 0) ? i : ((int64_t)(i / HW) * pstride + i % HW);
    Pack<T, 8> px = *reinterpret_cast<const Pack<T, 8>*>(&xg[idx]);
    xbuf[v8] = px;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      float v = to_f32(px.v[e]);
      s1 += v;
      s2 += v * v;
    }
  }
  s1 = wave_sum(s1);
  s2 = wave_sum(s2);
  const int wid = threadIdx.x / WAVE, nw = blockDim.x / WAVE;
  if ((threadIdx.x & (WAVE - 1)) == 0) { red[0][wid] = s1; red[1][wid] = s2; }
  __syncthreads();
  s1 = 0.f; s2 = 0.f;
  for (int w = 0; w < nw; ++w) { s1 += red[0][w]; s2 += red[1][w]; }
  const float mean = s1 / n;
  const float var = fmaxf(s2 / n - mean * mean, 0.f);
  const float rstd = rsqrtf(var + eps);
  if (threadIdx.x == 0) { mean_out[group] = mean; rstd_out[group] = rstd; }

  const T* gam = gamma + (int64_t)c * ch + g * cg;
  const T* bet = beta + (int64_t)c * ch + g * cg;
  for (int v8 = threadIdx.x; v8 < nv; v8 += blockDim.x) {
    int i = v8 * 8;
    int chan = i / HW;
    int64_t idx = (LAYOUT == 0) ? i : ((int64_t)chan * pstride + i % HW);
    Pack<T, 8> px = xbuf[v8];
    Pack<T, 8> pr;
    if (HAS_RES) pr = *reinterpret_cast<const Pack<T, 8>*>(&rg[idx]);
    Pack<T, 8> py;
    const float ga = to_f32(gam[chan]), be = to_f32(bet[chan]);
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      float v = (to_f32(px.v[e]) - mean) * rstd;
      v = v * ga + be;
      if (HAS_RES) v += to_f32(pr.v[e]);
      if (RELU) v = fmaxf(v, 0.f);
      py.v[e] = from_f32<T>(v);
    }
    *reinterpret_cast<Pack<T, 8>*>(&yg[idx]) = py;
  }
}

#define MAX_CG 128

template <typename T, bool HAS_RES, bool RELU, int LAYOUT>
__global__ __launch_bounds__(OLS_THREADS) void k_gn_bwd(
    const T* __restrict__ x, const T* __restrict__ y,
    const T* __restrict__ dy, T* __restrict__ dx, T* __restrict__ dres,
    const float* __restrict__ mean_in, const float* __restrict__ rstd_in,
    const T* __restrict__ gamma, float* __restrict__ dgamma,
    float* __restrict__ dbeta, int Bn, int C, int ch, int G, int HW) {
  const int cg = ch / G;
  const int n = cg * HW;
  const int group = blockIdx.x;
  int c, g;
  int64_t base, pstride;
  if (LAYOUT == 0) {
    g = group % G;
    c = (group / G) % C;
    base = (int64_t)group * n;
    pstride = HW;
  } else {
    const int b = group % Bn;
    g = (group / Bn) % G;
    c = group / (Bn * G);
    base = (((int64_t)c * ch + (int64_t)g * cg) * Bn + b) * HW;
    pstride = (int64_t)Bn * HW;
  }
  const T* xg = x + base;
  const T* yg = y + base;
  const T* dyg_in = dy + base;
  T* dxg = dx + base;
  T* drg = HAS_RES ? dres + base : nullptr;
  const float mean = mean_in[group], rstd = rstd_in[group];
  const T* gam = gamma + (int64_t)c * ch + g * cg;

  __shared__ float red[2][OLS_THREADS / WAVE];
  __shared__ float ch_dg[MAX_CG], ch_db[MAX_CG];
  for (int i = threadIdx.x; i < cg; i += blockDim.x) {
    ch_dg[i] = 0.f; ch_db[i] = 0.f;
  }
  __syncthreads();

  const int lane = threadIdx.x & (WAVE - 1);
  float s1 = 0.f, s2 = 0.f;
  // Vector path (HW % 8 == 0, every model plane): 16 B loads per lane,
  // and the per-channel dgamma/dbeta partials are reduced across the
  // lanes that share a channel BEFORE one LDS atomic — the previous
  // per-element atomics serialised up to 256 ways on one address when
  // HW >= the block span.  lpc = lanes per channel: the largest power of
  // two dividing hv, so an aligned group of lpc lanes never straddles a
  // channel (hv itself is not a power of two for e.g. 28x28 or 4x6 planes).
  const bool vec = (HW % 8) == 0;
  if (vec) {
    const int nv = n / 8;
    const int hv = HW / 8;                     // vectors per channel-plane
    const int lpc = min(WAVE, hv & -hv);
    // whole waves iterate together (the shuffle reduce needs every lane
    // of a channel group present; groups of lpc consecutive vectors are
    // always fully active or fully inactive since lpc divides nv)
    for (int v8 = threadIdx.x; v8 - lane < nv; v8 += blockDim.x) {
      const bool active = v8 < nv;
      int i = active ? v8 * 8 : 0;
      int chan = i / HW;
      int64_t idx = (LAYOUT == 0) ? i : ((int64_t)chan * pstride + i % HW);
      float dg = 0.f, db = 0.f;
      if (active) {
        Pack<T, 8> pdy = *reinterpret_cast<const Pack<T, 8>*>(&dyg_in[idx]);
        Pack<T, 8> px = *reinterpret_cast<const Pack<T, 8>*>(&xg[idx]);
        Pack<T, 8> py;
        if (RELU) py = *reinterpret_cast<const Pack<T, 8>*>(&yg[idx]);
        const float ga = to_f32(gam[chan]);
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          float grad = to_f32(pdy.v[e]);
          if (RELU) grad = to_f32(py.v[e]) > 0.f ? grad : 0.f;
          float xhat = (to_f32(px.v[e]) - mean) * rstd;
          float dxhat = grad * ga;
          s1 += dxhat;
          s2 += dxhat * xhat;
          dg += grad * xhat;
          db += grad;
        }
      }
      // reduce over the lpc lanes sharing this channel, one atomic per
      // group (distinct channels land on distinct LDS addresses)
#pragma unroll
      for (int off = 32; off > 0; off >>= 1)
        if (off < lpc) {
          dg += __shfl_xor(dg, off, WAVE);
          db += __shfl_xor(db, off, WAVE);
        }
      if (active && (lane & (lpc - 1)) == 0) {
        atomicAdd(&ch_dg[chan], dg);
        atomicAdd(&ch_db[chan], db);
      }
    }
  } else {
    for (int i = threadIdx.x; i < n; i += blockDim.x) {
      int chan = i / HW;
      int64_t idx = (LAYOUT == 0) ? i : ((int64_t)chan * pstride + i % HW);
      float grad = to_f32(dyg_in[idx]);
      if (RELU) grad = to_f32(yg[idx]) > 0.f ? grad : 0.f;
      float xhat = (to_f32(xg[idx]) - mean) * rstd;
      float dxhat = grad * to_f32(gam[chan]);
      s1 += dxhat;
      s2 += dxhat * xhat;
      atomicAdd(&ch_dg[chan], grad * xhat);
      atomicAdd(&ch_db[chan], grad);
    }
  }
  s1 = wave_sum(s1);
  s2 = wave_sum(s2);
  const int wid = threadIdx.x / WAVE, nw = blockDim.x / WAVE;
  if ((threadIdx.x & (WAVE - 1)) == 0) { red[0][wid] = s1; red[1][wid] = s2; }
  __syncthreads();
  s1 = 0.f; s2 = 0.f;
  for (int w = 0; w < nw; ++w) { s1 += red[0][w]; s2 += red[1][w]; }
  const float m1 = s1 / n, m2 = s2 / n;

  if (vec) {
    const int nv = n / 8;
    for (int v8 = threadIdx.x; v8 < nv; v8 += blockDim.x) {
      int i = v8 * 8;
      int chan = i / HW;
      int64_t idx = (LAYOUT == 0) ? i : ((int64_t)chan * pstride + i % HW);
      Pack<T, 8> pdy = *reinterpret_cast<const Pack<T, 8>*>(&dyg_in[idx]);
      Pack<T, 8> px = *reinterpret_cast<const Pack<T, 8>*>(&xg[idx]);
      Pack<T, 8> py;
      if (RELU) py = *reinterpret_cast<const Pack<T, 8>*>(&yg[idx]);
      const float ga = to_f32(gam[chan]);
      Pack<T, 8> pdx, pdr;
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        float grad = to_f32(pdy.v[e]);
        if (RELU) grad = to_f32(py.v[e]) > 0.f ? grad : 0.f;
        float xhat = (to_f32(px.v[e]) - mean) * rstd;
        float dxhat = grad * ga;
        pdx.v[e] = from_f32<T>(rstd * (dxhat - m1 - xhat * m2));
        if (HAS_RES) pdr.v[e] = from_f32<T>(grad);
      }
      *reinterpret_cast<Pack<T, 8>*>(&dxg[idx]) = pdx;
      if (HAS_RES) *reinterpret_cast<Pack<T, 8>*>(&drg[idx]) = pdr;
    }
  } else {
    for (int i = threadIdx.x; i < n; i += blockDim.x) {
      int chan = i / HW;
      int64_t idx = (LAYOUT == 0) ? i : ((int64_t)chan * pstride + i % HW);
      float grad = to_f32(dyg_in[idx]);
      if (RELU) grad = to_f32(yg[idx]) > 0.f ? grad : 0.f;
      float xhat = (to_f32(xg[idx]) - mean) * rstd;
      float dxhat = grad * to_f32(gam[chan]);
      dxg[idx] = from_f32<T>(rstd * (dxhat - m1 - xhat * m2));
      if (HAS_RES) drg[idx] = from_f32<T>(grad);
    }
  }
  __syncthreads();
  for (int i = threadIdx.x; i < cg; i += blockDim.x) {
    atomicAdd(&dgamma[(int64_t)c * ch + g * cg + i], ch_dg[i]);
    atomicAdd(&dbeta[(int64_t)c * ch + g * cg + i], ch_db[i]);
  }
}


// One-global-pass backward: the group's x and (relu-masked) dy are
// staged in LDS during the stats pass and replayed for the dx pass, so
// x/dy stream from HBM once instead of twice (k_gn_bwd reads them in
// both passes).  Fits when 4*n bytes of dynamic LDS are available
// (n = cg*HW; every model group plane is <= 8K elements = 32 KB).
template <typename T, bool HAS_RES, bool RELU, int LAYOUT>
__global__ __launch_bounds__(OLS_THREADS) void k_gn_bwd_lds(
    const T* __restrict__ x, const T* __restrict__ y,
    const T* __restrict__ dy, T* __restrict__ dx, T* __restrict__ dres,
    const float* __restrict__ mean_in, const float* __restrict__ rstd_in,
    const T* __restrict__ gamma, float* __restrict__ dgamma,
    float* __restrict__ dbeta, int Bn, int C, int ch, int G, int HW) {
  const int cg = ch / G;
  const int n = cg * HW;
  const int group = blockIdx.x;
  int c, g;
  int64_t base, pstride;
  if (LAYOUT == 0) {
    g = group % G;
    c = (group / G) % C;
    base = (int64_t)group * n;
    pstride = HW;
  } else {
    const int b = group % Bn;
    g = (group / Bn) % G;
    c = group / (Bn * G);
    base = (((int64_t)c * ch + (int64_t)g * cg) * Bn + b) * HW;
    pstride = (int64_t)Bn * HW;
  }
  const T* xg = x + base;
  const T* yg = y + base;
  const T* dyg_in = dy + base;
  T* dxg = dx + base;
  T* drg = HAS_RES ? dres + base : nullptr;
  const float mean = mean_in[group], rstd = rstd_in[group];
  const T* gam = gamma + (int64_t)c * ch + g * cg;

  extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
  Pack<T, 8>* xbuf = reinterpret_cast<Pack<T, 8>*>(lds_raw);
  Pack<T, 8>* gbuf = xbuf + n / 8;

  __shared__ float red[2][OLS_THREADS / WAVE];
  __shared__ float ch_dg[MAX_CG], ch_db[MAX_CG];
  for (int i = threadIdx.x; i < cg; i += blockDim.x) {
    ch_dg[i] = 0.f; ch_db[i] = 0.f;
  }
  __syncthreads();

  const int lane = threadIdx.x & (WAVE - 1);
  float s1 = 0.f, s2 = 0.f;
  const int nv = n / 8;
  const int hv = HW / 8;
  const int lpc = min(WAVE, hv & -hv);   // pow2 divisor of hv (see k_gn_bwd)
  for (int v8 = threadIdx.x; v8 - lane < nv; v8 += blockDim.x) {
    const bool active = v8 < nv;
    int i = active ? v8 * 8 : 0;
    int chan = i / HW;
    int64_t idx = (LAYOUT == 0) ? i : ((int64_t)chan * pstride + i % HW);
    float dg = 0.f, db = 0.f;
    if (active) {
      Pack<T, 8> pdy = *reinterpret_cast<const Pack<T, 8>*>(&dyg_in[idx]);
      Pack<T, 8> px = *reinterpret_cast<const Pack<T, 8>*>(&xg[idx]);
      Pack<T, 8> py;
      if (RELU) py = *reinterpret_cast<const Pack<T, 8>*>(&yg[idx]);
      const float ga = to_f32(gam[chan]);
      Pack<T, 8> pg;
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        float grad = to_f32(pdy.v[e]);
        if (RELU) grad = to_f32(py.v[e]) > 0.f ? grad : 0.f;
        pg.v[e] = RELU ? from_f32<T>(grad) : pdy.v[e];
        float xhat = (to_f32(px.v[e]) - mean) * rstd;
        float dxhat = grad * ga;
        s1 += dxhat;
        s2 += dxhat * xhat;
        dg += grad * xhat;
        db += grad;
      }
      xbuf[v8] = px;
      gbuf[v8] = pg;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1)
      if (off < lpc) {
        dg += __shfl_xor(dg, off, WAVE);
        db += __shfl_xor(db, off, WAVE);
      }
    if (active && (lane & (lpc - 1)) == 0) {
      atomicAdd(&ch_dg[chan], dg);
      atomicAdd(&ch_db[chan], db);
    }
  }
  s1 = wave_sum(s1);
  s2 = wave_sum(s2);
  const int wid = threadIdx.x / WAVE, nw = blockDim.x / WAVE;
  if ((threadIdx.x & (WAVE - 1)) == 0) { red[0][wid] = s1; red[1][wid] = s2; }
  __syncthreads();
  s1 = 0.f; s2 = 0.f;
  for (int w = 0; w < nw; ++w) { s1 += red[0][w]; s2 += red[1][w]; }
  const float m1 = s1 / n, m2 = s2 / n;

  for (int v8 = threadIdx.x; v8 < nv; v8 += blockDim.x) {
    int i = v8 * 8;
    int chan = i / HW;
    int64_t idx = (LAYOUT == 0) ? i : ((int64_t)chan * pstride + i % HW);
    Pack<T, 8> px = xbuf[v8];
    Pack<T, 8> pg = gbuf[v8];
    const float ga = to_f32(gam[chan]);
    Pack<T, 8> pdx;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      float grad = to_f32(pg.v[e]);
      float xhat = (to_f32(px.v[e]) - mean) * rstd;
      float dxhat = grad * ga;
      pdx.v[e] = from_f32<T>(rstd * (dxhat - m1 - xhat * m2));
    }
    *reinterpret_cast<Pack<T, 8>*>(&dxg[idx]) = pdx;
    if (HAS_RES) *reinterpret_cast<Pack<T, 8>*>(&drg[idx]) = pg;
  }
  __syncthreads();
  for (int i = threadIdx.x; i < cg; i += blockDim.x) {
    atomicAdd(&dgamma[(int64_t)c * ch + g * cg + i], ch_dg[i]);
    atomicAdd(&dbeta[(int64_t)c * ch + g * cg + i], ch_db[i]);
  }
}

// ---------------------------------------------------------------------------
// Padded-output family (LAYOUT 1, bf16, ReLU always on).
//
// The v6 3x3 convs gather from activations [C, ch, B, H+2, W+2] carrying
// a 1-element zero halo.  These variants of the LDS-staged kernels write
// that padded image themselves, so no standalone pad pass runs between a
// GroupNorm and the conv that consumes it:
//   fwd: y is written padded (halo zeroed here) and a 1-bit-per-element
//        ReLU mask replaces the saved y for backward;
//   bwd: takes the mask, writes dense dx (wgrad's A operand) and, on
//        request, the same values again as a padded image (dgrad's input).
// The statistics passes are copies of k_gn_fwd_lds / k_gn_bwd_lds (same
// striding, same reduction order), so mean/rstd/dx/dres are bit-identical.
//
// Padded planes are (H+2)*(W+2) elements; with H, W even that is a
// multiple of 4, so every plane base is 8-byte aligned and the store pass
// walks the padded index space in aligned 4-element vectors, picking each
// interior element out of LDS.
//
// Mask layout (private to this pair): per group ceil(n/32) uint32 words;
// bit (i & 31) of word (i >> 5) is y > 0 for group-local dense element
// i = chan*HW + h*W + w, i.e. byte (v8 & 3) of word (v8 >> 2) covers the
// 8-element vector v8 the backward iterates over.

typedef __hip_bfloat16 bf16;

struct __align__(8) Bf4 {
  bf16 v[4];
};

// RES: 0 none, 1 dense residual [C, ch, B, H, W] (staged in LDS with
// aligned 16 B loads), 2 padded residual (same geometry as the padded y).
// PAD_OUT false writes a dense y (the network's last block, whose output
// feeds the pooling) while still accepting a padded residual.
template <int RES, bool PAD_OUT>
__global__ __launch_bounds__(OLS_THREADS) void k_gn_fwd_pad(
    const bf16* __restrict__ x, const bf16* __restrict__ res,
    bf16* __restrict__ y, uint32_t* __restrict__ mask,
    float* __restrict__ mean_out, float* __restrict__ rstd_out,
    const bf16* __restrict__ gamma, const bf16* __restrict__ beta, int Bn,
    int C, int ch, int G, int H, int W, float eps) {
  const int cg = ch / G;
  const int HW = H * W;
  const int n = cg * HW;
  const int PW = W + 2, PHW = (H + 2) * PW;
  const int group = blockIdx.x;
  const int b = group % Bn;
  const int g = (group / Bn) % G;
  const int c = group / (Bn * G);
  const int64_t plane0 = ((int64_t)c * ch + (int64_t)g * cg) * Bn + b;
  const int64_t base = plane0 * HW, pstride = (int64_t)Bn * HW;
  const int64_t pbase = plane0 * PHW, ppstride = (int64_t)Bn * PHW;
  const bf16* xg = x + base;

  extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
  Pack<bf16, 8>* xbuf = reinterpret_cast<Pack<bf16, 8>*>(lds_raw);
  const int nv = n / 8;
  Pack<bf16, 8>* rbuf = xbuf + nv;              // RES == 1 only

  __shared__ float red[2][OLS_THREADS / WAVE];
  float s1 = 0.f, s2 = 0.f;
  for (int v8 = threadIdx.x; v8 < nv; v8 += blockDim.x) {
    int i = v8 * 8;
    int64_t idx = (int64_t)(i / HW) * pstride + i % HW;
    Pack<bf16, 8> px = *reinterpret_cast<const Pack<bf16, 8>*>(&xg[idx]);
    xbuf[v8] = px;
    if (RES == 1)
      rbuf[v8] = *reinterpret_cast<const Pack<bf16, 8>*>(&res[base + idx]);
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      float v = to_f32(px.v[e]);
      s1 += v;
      s2 += v * v;
    }
  }
  s1 = wave_sum(s1);
  s2 = wave_sum(s2);
  const int wid = threadIdx.x / WAVE, nw = blockDim.x / WAVE;
  if ((threadIdx.x & (WAVE - 1)) == 0) { red[0][wid] = s1; red[1][wid] = s2; }
  __syncthreads();
  s1 = 0.f; s2 = 0.f;
  for (int w = 0; w < nw; ++w) { s1 += red[0][w]; s2 += red[1][w]; }
  const float mean = s1 / n;
  const float var = fmaxf(s2 / n - mean * mean, 0.f);
  const float rstd = rsqrtf(var + eps);
  if (threadIdx.x == 0) { mean_out[group] = mean; rstd_out[group] = rstd; }

  const bf16* gam = gamma + (int64_t)c * ch + g * cg;
  const bf16* bet = beta + (int64_t)c * ch + g * cg;
  // element views of the staged x / dense residual; each rounded y is
  // written back over the x it came from (one owner per element) so the
  // mask pass below can read it
  bf16* xe = reinterpret_cast<bf16*>(xbuf);
  const bf16* re = reinterpret_cast<const bf16*>(rbuf);
  if (PAD_OUT) {
    const int nvp = PHW / 4;                    // vectors per padded plane
    const int total = cg * nvp;
    for (int t = threadIdx.x; t < total; t += blockDim.x) {
      const int chan = t / nvp;
      const int q = (t - chan * nvp) * 4;
      int ph = q / PW, pw = q - ph * PW;
      const int64_t off = pbase + (int64_t)chan * ppstride + q;
      Bf4 pr;
      if (RES == 2) pr = *reinterpret_cast<const Bf4*>(&res[off]);
      const float ga = to_f32(gam[chan]), be = to_f32(bet[chan]);
      Bf4 py;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        bf16 o = from_f32<bf16>(0.f);
        if (ph >= 1 && ph <= H && pw >= 1 && pw <= W) {
          const int li = chan * HW + (ph - 1) * W + (pw - 1);
          float v = (to_f32(xe[li]) - mean) * rstd;
          v = v * ga + be;
          if (RES == 1) v += to_f32(re[li]);
          if (RES == 2) v += to_f32(pr.v[e]);
          v = fmaxf(v, 0.f);
          o = from_f32<bf16>(v);
          xe[li] = o;
        }
        py.v[e] = o;
        if (++pw == PW) { pw = 0; ++ph; }
      }
      *reinterpret_cast<Bf4*>(&y[off]) = py;
    }
  } else {
    for (int v8 = threadIdx.x; v8 < nv; v8 += blockDim.x) {
      int i = v8 * 8;
      int chan = i / HW;
      int hw = i - chan * HW;
      int64_t idx = (int64_t)chan * pstride + hw;
      Pack<bf16, 8> px = xbuf[v8];
      Pack<bf16, 8> pr;
      if (RES == 1) pr = rbuf[v8];
      if (RES == 2) {
        const bf16* rp = res + pbase + (int64_t)chan * ppstride;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          int h = (hw + e) / W, w = (hw + e) - h * W;
          pr.v[e] = rp[(h + 1) * PW + (w + 1)];
        }
      }
      Pack<bf16, 8> py;
      const float ga = to_f32(gam[chan]), be = to_f32(bet[chan]);
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        float v = (to_f32(px.v[e]) - mean) * rstd;
        v = v * ga + be;
        if (RES != 0) v += to_f32(pr.v[e]);
        v = fmaxf(v, 0.f);
        py.v[e] = from_f32<bf16>(v);
      }
      xbuf[v8] = py;
      *reinterpret_cast<Pack<bf16, 8>*>(&y[base + idx]) = py;
    }
  }
  __syncthreads();
  const int nwords = (n + 31) / 32;
  uint32_t* mg = mask + (int64_t)group * nwords;
  for (int j = threadIdx.x; j < nwords; j += blockDim.x) {
    uint32_t wv = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int v8 = j * 4 + k;
      if (v8 < nv) {
        Pack<bf16, 8> p = xbuf[v8];
#pragma unroll
        for (int e = 0; e < 8; ++e)
          if (to_f32(p.v[e]) > 0.f) wv |= 1u << (k * 8 + e);
      }
    }
    mg[j] = wv;
  }
}

// Backward from the ReLU bitmask.  dx_pad may be null (no padded image
// wanted).  Passes 1 and 2 are k_gn_bwd_lds<.., RELU=true, LAYOUT=1> with
// the mask bit standing in for y > 0.
template <bool HAS_RES>
__global__ __launch_bounds__(OLS_THREADS) void k_gn_bwd_pad(
    const bf16* __restrict__ x, const uint32_t* __restrict__ mask,
    const bf16* __restrict__ dy, bf16* __restrict__ dx,
    bf16* __restrict__ dx_pad, bf16* __restrict__ dres,
    const float* __restrict__ mean_in, const float* __restrict__ rstd_in,
    const bf16* __restrict__ gamma, float* __restrict__ dgamma,
    float* __restrict__ dbeta, int Bn, int C, int ch, int G, int H, int W) {
  const int cg = ch / G;
  const int HW = H * W;
  const int n = cg * HW;
  const int PW = W + 2, PHW = (H + 2) * PW;
  const int group = blockIdx.x;
  const int b = group % Bn;
  const int g = (group / Bn) % G;
  const int c = group / (Bn * G);
  const int64_t plane0 = ((int64_t)c * ch + (int64_t)g * cg) * Bn + b;
  const int64_t base = plane0 * HW, pstride = (int64_t)Bn * HW;
  const int64_t pbase = plane0 * PHW, ppstride = (int64_t)Bn * PHW;
  const bf16* xg = x + base;
  const bf16* dyg_in = dy + base;
  bf16* dxg = dx + base;
  bf16* drg = HAS_RES ? dres + base : nullptr;
  const float mean = mean_in[group], rstd = rstd_in[group];
  const bf16* gam = gamma + (int64_t)c * ch + g * cg;
  const uint32_t* mg = mask + (int64_t)group * ((n + 31) / 32);

  extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
  Pack<bf16, 8>* xbuf = reinterpret_cast<Pack<bf16, 8>*>(lds_raw);
  Pack<bf16, 8>* gbuf = xbuf + n / 8;

  __shared__ float red[2][OLS_THREADS / WAVE];
  __shared__ float ch_dg[MAX_CG], ch_db[MAX_CG];
  for (int i = threadIdx.x; i < cg; i += blockDim.x) {
    ch_dg[i] = 0.f; ch_db[i] = 0.f;
  }
  __syncthreads();

  const int lane = threadIdx.x & (WAVE - 1);
  float s1 = 0.f, s2 = 0.f;
  const int nv = n / 8;
  const int hv = HW / 8;
  const int lpc = min(WAVE, hv & -hv);   // pow2 divisor of hv (see k_gn_bwd)
  for (int v8 = threadIdx.x; v8 - lane < nv; v8 += blockDim.x) {
    const bool active = v8 < nv;
    int i = active ? v8 * 8 : 0;
    int chan = i / HW;
    int64_t idx = (int64_t)chan * pstride + i % HW;
    float dg = 0.f, db = 0.f;
    if (active) {
      Pack<bf16, 8> pdy = *reinterpret_cast<const Pack<bf16, 8>*>(&dyg_in[idx]);
      Pack<bf16, 8> px = *reinterpret_cast<const Pack<bf16, 8>*>(&xg[idx]);
      const uint32_t mb = mg[v8 >> 2] >> ((v8 & 3) * 8);
      const float ga = to_f32(gam[chan]);
      Pack<bf16, 8> pg;
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        float grad = to_f32(pdy.v[e]);
        grad = ((mb >> e) & 1u) ? grad : 0.f;
        pg.v[e] = from_f32<bf16>(grad);
        float xhat = (to_f32(px.v[e]) - mean) * rstd;
        float dxhat = grad * ga;
        s1 += dxhat;
        s2 += dxhat * xhat;
        dg += grad * xhat;
        db += grad;
      }
      xbuf[v8] = px;
      gbuf[v8] = pg;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1)
      if (off < lpc) {
        dg += __shfl_xor(dg, off, WAVE);
        db += __shfl_xor(db, off, WAVE);
      }
    if (active && (lane & (lpc - 1)) == 0) {
      atomicAdd(&ch_dg[chan], dg);
      atomicAdd(&ch_db[chan], db);
    }
  }
  s1 = wave_sum(s1);
  s2 = wave_sum(s2);
  const int wid = threadIdx.x / WAVE, nw = blockDim.x / WAVE;
  if ((threadIdx.x & (WAVE - 1)) == 0) { red[0][wid] = s1; red[1][wid] = s2; }
  __syncthreads();
  s1 = 0.f; s2 = 0.f;
  for (int w = 0; w < nw; ++w) { s1 += red[0][w]; s2 += red[1][w]; }
  const float m1 = s1 / n, m2 = s2 / n;

  for (int v8 = threadIdx.x; v8 < nv; v8 += blockDim.x) {
    int i = v8 * 8;
    int chan = i / HW;
    int64_t idx = (int64_t)chan * pstride + i % HW;
    Pack<bf16, 8> px = xbuf[v8];
    Pack<bf16, 8> pg = gbuf[v8];
    const float ga = to_f32(gam[chan]);
    Pack<bf16, 8> pdx;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      float grad = to_f32(pg.v[e]);
      float xhat = (to_f32(px.v[e]) - mean) * rstd;
      float dxhat = grad * ga;
      pdx.v[e] = from_f32<bf16>(rstd * (dxhat - m1 - xhat * m2));
    }
    *reinterpret_cast<Pack<bf16, 8>*>(&dxg[idx]) = pdx;
    if (HAS_RES) *reinterpret_cast<Pack<bf16, 8>*>(&drg[idx]) = pg;
    xbuf[v8] = pdx;                   // own slot: replayed padded below
  }
  __syncthreads();
  if (dx_pad != nullptr) {
    const bf16* de = reinterpret_cast<const bf16*>(xbuf);
    const int nvp = PHW / 4;
    const int total = cg * nvp;
    for (int t = threadIdx.x; t < total; t += blockDim.x) {
      const int chan = t / nvp;
      const int q = (t - chan * nvp) * 4;
      int ph = q / PW, pw = q - ph * PW;
      Bf4 po;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        bf16 o = from_f32<bf16>(0.f);
        if (ph >= 1 && ph <= H && pw >= 1 && pw <= W)
          o = de[chan * HW + (ph - 1) * W + (pw - 1)];
        po.v[e] = o;
        if (++pw == PW) { pw = 0; ++ph; }
      }
      *reinterpret_cast<Bf4*>(
          &dx_pad[pbase + (int64_t)chan * ppstride + q]) = po;
    }
  }
  for (int i = threadIdx.x; i < cg; i += blockDim.x) {
    atomicAdd(&dgamma[(int64_t)c * ch + g * cg + i], ch_dg[i]);
    atomicAdd(&dbeta[(int64_t)c * ch + g * cg + i], ch_db[i]);
  }
}

// The padded pair is used only when BOTH directions fit their LDS staging
// (backward: x + masked dy = 4 B per element, which also covers the
// forward with a staged dense residual) and the planes vectorise.
extern "C" int ols_gn_pad_ok(int ch, int G, int H, int W) {
  if (G <= 0 || ch % G != 0 || ch / G > MAX_CG) return 0;
  if (H < 2 || W < 2 || (H & 1) || (W & 1) || (H * W) % 8 != 0) return 0;
  const int64_t n = (int64_t)(ch / G) * H * W;
  return n * 4 <= 65536;
}

extern "C" void ols_groupnorm_fwd_pad(
    const void* x, const void* res, int res_mode, void* y, uint32_t* mask,
    float* mean, float* rstd, const void* gamma, const void* beta, int B,
    int C, int ch, int G, int H, int W, float eps, bool pad_out,
    hipStream_t s) {
  dim3 grid(B * C * G), block(OLS_THREADS);
  const int n = (ch / G) * H * W;
  const size_t lds = (size_t)n * sizeof(bf16) * (res_mode == 1 ? 2 : 1);
#define CASE(RM, PO)                                                          \
  hipLaunchKernelGGL((k_gn_fwd_pad<RM, PO>), grid, block, lds, s,             \
                     (const bf16*)x, (const bf16*)res, (bf16*)y, mask, mean,  \
                     rstd, (const bf16*)gamma, (const bf16*)beta, B, C, ch,   \
                     G, H, W, eps)
  if (pad_out) {
    if (res_mode == 0) CASE(0, true);
    else if (res_mode == 1) CASE(1, true);
    else CASE(2, true);
  } else {
    if (res_mode == 0) CASE(0, false);
    else if (res_mode == 1) CASE(1, false);
    else CASE(2, false);
  }
#undef CASE
}

extern "C" void ols_groupnorm_bwd_pad(
    const void* x, const uint32_t* mask, const void* dy, void* dx,
    void* dx_pad, void* dres, const float* mean, const float* rstd,
    const void* gamma, float* dgamma, float* dbeta, int B, int C, int ch,
    int G, int H, int W, hipStream_t s) {
  dim3 grid(B * C * G), block(OLS_THREADS);
  const int n = (ch / G) * H * W;
  const size_t lds = (size_t)n * 2 * sizeof(bf16);
  if (dres != nullptr)
    hipLaunchKernelGGL((k_gn_bwd_pad<true>), grid, block, lds, s,
                       (const bf16*)x, mask, (const bf16*)dy, (bf16*)dx,
                       (bf16*)dx_pad, (bf16*)dres, mean, rstd,
                       (const bf16*)gamma, dgamma, dbeta, B, C, ch, G, H, W);
  else
    hipLaunchKernelGGL((k_gn_bwd_pad<false>), grid, block, lds, s,
                       (const bf16*)x, mask, (const bf16*)dy, (bf16*)dx,
                       (bf16*)dx_pad, (bf16*)dres, mean, rstd,
                       (const bf16*)gamma, dgamma, dbeta, B, C, ch, G, H, W);
}

template <typename T>
static void launch_fwd(const T* x, const T* res, T* y, float* mean,
                       float* rstd, const T* gamma, const T* beta, int B,
                       int C, int ch, int G, int HW, float eps, bool relu,
                       int layout, hipStream_t s) {
  dim3 grid(B * C * G), block(OLS_THREADS);
  const bool has_res = res != nullptr;
  const int n = (ch / G) * HW;
  const size_t lds = (size_t)n * sizeof(T);
  const bool use_lds = (HW % 8) == 0 && sizeof(T) == 2 && lds <= 65536;
#define CASE(HR, RL, LY)                                                      \
  do {                                                                        \
    if (use_lds)                                                              \
      hipLaunchKernelGGL((k_gn_fwd_lds<T, HR, RL, LY>), grid, block, lds, s, \
                         x, res, y, mean, rstd, gamma, beta, B, C, ch, G,    \
                         HW, eps);                                           \
    else                                                                      \
      hipLaunchKernelGGL((k_gn_fwd<T, HR, RL, LY>), grid, block, 0, s, x,    \
                         res, y, mean, rstd, gamma, beta, B, C, ch, G, HW,   \
                         eps);                                               \
  } while (0)
#define PICK(LY)                                                              \
  do {                                                                        \
    if (has_res && relu) CASE(true, true, LY);                                \
    else if (has_res) CASE(true, false, LY);                                  \
    else if (relu) CASE(false, true, LY);                                     \
    else CASE(false, false, LY);                                              \
  } while (0)
  if (layout == 0) PICK(0); else PICK(1);
#undef PICK
#undef CASE
}

template <typename T>
static void launch_bwd(const T* x, const T* y, const T* dy, T* dx, T* dres,
                       const float* mean, const float* rstd, const T* gamma,
                       float* dgamma, float* dbeta, int B, int C, int ch,
                       int G, int HW, bool relu, int layout, hipStream_t s) {
  dim3 grid(B * C * G), block(OLS_THREADS);
  const bool has_res = dres != nullptr;
  // one-global-pass variant when the group plane fits in LDS (4 bytes
  // of staging per element; cap 64 KB keeps >= 2 blocks resident)
  const int n = (ch / G) * HW;
  const size_t lds = (size_t)n * 2 * sizeof(T);
  const bool use_lds = (HW % 8) == 0 && sizeof(T) == 2 && lds <= 65536;
#define CASE(HR, RL, LY)                                                      \
  do {                                                                        \
    if (use_lds)                                                              \
      hipLaunchKernelGGL((k_gn_bwd_lds<T, HR, RL, LY>), grid, block, lds, s, \
                         x, y, dy, dx, dres, mean, rstd, gamma, dgamma,      \
                         dbeta, B, C, ch, G, HW);                            \
    else                                                                      \
      hipLaunchKernelGGL((k_gn_bwd<T, HR, RL, LY>), grid, block, 0, s, x, y, \
                         dy, dx, dres, mean, rstd, gamma, dgamma, dbeta, B,  \
                         C, ch, G, HW);                                      \
  } while (0)
#define PICK(LY)                                                              \
  do {                                                                        \
    if (has_res && relu) CASE(true, true, LY);                                \
    else if (has_res) CASE(true, false, LY);                                  \
    else if (relu) CASE(false, true, LY);                                     \
    else CASE(false, false, LY);                                              \
  } while (0)
  if (layout == 0) PICK(0); else PICK(1);
#undef PICK
#undef CASE
}

extern "C" void ols_groupnorm_fwd(const void* x, const void* res, void* y,
                                  float* mean, float* rstd, const void* gamma,
                                  const void* beta, int B, int C, int ch,
                                  int G, int HW, float eps, bool relu,
                                  int layout, int dtype, hipStream_t stream) {
  if (dtype == 0)
    launch_fwd<float>((const float*)x, (const float*)res, (float*)y, mean,
                      rstd, (const float*)gamma, (const float*)beta, B, C, ch,
                      G, HW, eps, relu, layout, stream);
  else
    launch_fwd<__hip_bfloat16>((const __hip_bfloat16*)x,
                               (const __hip_bfloat16*)res, (__hip_bfloat16*)y,
                               mean, rstd, (const __hip_bfloat16*)gamma,
                               (const __hip_bfloat16*)beta, B, C, ch, G, HW,
                               eps, relu, layout, stream);
}

extern "C" void ols_groupnorm_bwd(const void* x, const void* y,
                                  const void* dy, void* dx, void* dres,
                                  const float* mean, const float* rstd,
                                  const void* gamma, float* dgamma,
                                  float* dbeta, int B, int C, int ch, int G,
                                  int HW, bool relu, int layout, int dtype,
                                  hipStream_t stream) {
  if (dtype == 0)
    launch_bwd<float>((const float*)x, (const float*)y, (const float*)dy,
                      (float*)dx, (float*)dres, mean, rstd,
                      (const float*)gamma, dgamma, dbeta, B, C, ch, G, HW,
                      relu, layout, stream);
  else
    launch_bwd<__hip_bfloat16>(
        (const __hip_bfloat16*)x, (const __hip_bfloat16*)y,
        (const __hip_bfloat16*)dy, (__hip_bfloat16*)dx, (__hip_bfloat16*)dres,
        mean, rstd, (const __hip_bfloat16*)gamma, dgamma, dbeta, B, C, ch, G,
        HW, relu, layout, stream);
}
