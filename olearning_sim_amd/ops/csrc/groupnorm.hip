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
// (contiguous, LAYOUT 0), conceptually [B, C, G, ch/G, H, W]; a
// normalisation group (b, c, g) spans cg*HW CONTIGUOUS elements, so every
// group is a coalesced span.  LAYOUT 1 is [C, ch, B, H, W]: the group's
// cg planes are strided by B*HW.  gamma/beta are per-client affine [C, ch].
//
// fwd:  y = gn(x)*gamma + beta  [+ res]  [relu]
//       one workgroup per group (B*C*G workgroups >> 256 CUs);
//       pass 1 reduces sum/sumsq (wave + LDS), pass 2 re-reads x
//       (L1/L2-resident) and writes y; saves mean/rstd per group.
// bwd:  dx = rstd*(dxhat - mean(dxhat) - xhat*mean(dxhat*xhat)),
//       dxhat = relu-masked dy * gamma; per-channel dgamma/dbeta
//       partials reduced in LDS then one fp32 atomicAdd per channel.
//
// Six kernels: k_gn_fwd / k_gn_bwd stream x (and dy) from global in both
// passes; k_gn_fwd_lds / k_gn_bwd_lds stage the group in LDS in pass 1 and
// replay it; k_gn_fwd_pad / k_gn_bwd_pad do that and write the conv's zero
// halo.  All are compositions of the device pieces below.  What an edit of
// a piece must keep for the bits to stay: docs/KERNEL_NOTES.md,
// "GroupNorm: shared pieces".

#include <type_traits>

#include "common.h"
#include "ols_ops.h"

typedef __hip_bfloat16 bf16;

struct __align__(8) Bf4 {
  bf16 v[4];
};

// ==== Shared device pieces

// 8 elements (16 B) per lane per access — scalar bf16 loads measure 2-2.5x
// slower on gfx950 (cdna_hip_programming.md G13).  Taken only where HW is
// a multiple of 8 (every model plane), so a vector never crosses a plane
// (LAYOUT 1) or channel boundary.
template <typename T>
__device__ __forceinline__ Pack<T, 8> ld8(const T* p) {
  return *reinterpret_cast<const Pack<T, 8>*>(p);
}
template <typename T>
__device__ __forceinline__ void st8(T* p, const Pack<T, 8>& v) {
  *reinterpret_cast<Pack<T, 8>*>(p) = v;
}

// dynamic LDS of the staged kernels, in 8-element vectors
template <typename T>
__device__ __forceinline__ Pack<T, 8>* gn_dyn_lds() {
  extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
  return reinterpret_cast<Pack<T, 8>*>(lds_raw);
}

// Where this workgroup works: its group index, client c, norm group g,
// its first element and the stride between its cg planes, and the offset
// of its first channel in the [C, ch] affine tensors.  pbase/ppstride are
// the same in an image of PHW-element planes: LAYOUT 1 with PHW given (the
// padded pair) only, 0 otherwise.
struct GnGroup {
  int group, c, g;
  int64_t base, pstride;
  int64_t pbase, ppstride;
  int64_t aff;
};

template <int LAYOUT>
__device__ __forceinline__ GnGroup gn_decode(int Bn, int C, int ch, int G,
                                             int HW, int PHW) {
  const int cg = ch / G;
  const int group = blockIdx.x;
  GnGroup d;
  d.group = group;
  if (LAYOUT == 0) {          // group = (b, c, g); contiguous cg*HW span
    d.g = group % G;
    d.c = (group / G) % C;
    d.base = (int64_t)group * (cg * HW);
    d.pstride = HW;
    d.pbase = 0;              // no padded LAYOUT 0 image
    d.ppstride = 0;
  } else {                    // group = (c, g, b); planes strided by B*HW
    const int b = group % Bn;
    d.g = (group / Bn) % G;
    d.c = group / (Bn * G);
    const int64_t plane0 = ((int64_t)d.c * ch + (int64_t)d.g * cg) * Bn + b;
    d.base = plane0 * HW;
    d.pstride = (int64_t)Bn * HW;
    d.pbase = plane0 * PHW;
    d.ppstride = (int64_t)Bn * PHW;
  }
  d.aff = (int64_t)d.c * ch + d.g * cg;
  return d;
}

// offset from the group's base of its dense element i, in channel `chan`
template <int LAYOUT>
__device__ __forceinline__ int64_t gn_idx(int i, int chan, int HW,
                                          int64_t pstride) {
  return (LAYOUT == 0) ? i : ((int64_t)chan * pstride + i % HW);
}

// The forward passes' and the backward dx passes' walk over the group's
// n/8 vectors: body(v8, chan, idx).
template <int LAYOUT, typename Body>
__device__ __forceinline__ void gn_for_packs(int n, int HW, int64_t pstride,
                                             Body body) {
  const int nv = n / 8;
  for (int v8 = threadIdx.x; v8 < nv; v8 += blockDim.x) {
    int i = v8 * 8;
    int chan = i / HW;                       // channel within the group
    body(v8, chan, gn_idx<LAYOUT>(i, chan, HW, pstride));
  }
}

// A pair of sums.  How a running sum reaches a helper decides which adds
// the compiler pairs into packed ops and which products it fuses, and with
// that the bits: the forward's travel by value and the backward's by
// reference, each as compiled before (docs/KERNEL_NOTES.md).
struct Sum2 {
  float s1, s2;
};

// Block sum of both, left in every thread: wave butterfly, lane 0 of each
// wave to LDS, then every thread adds the nw waves' partials in order.
// The caller reads nw = blockDim.x / WAVE before its loops: read here,
// after a divergent loop, it costs a vector load and a full wait per block.
__device__ __forceinline__ Sum2 block_sum2(Sum2 s, int nw) {
  __shared__ float red[2][OLS_THREADS / WAVE];
  float s1 = wave_sum(s.s1);
  float s2 = wave_sum(s.s2);
  const int wid = threadIdx.x / WAVE;
  if ((threadIdx.x & (WAVE - 1)) == 0) { red[0][wid] = s1; red[1][wid] = s2; }
  __syncthreads();
  s1 = 0.f; s2 = 0.f;
  for (int w = 0; w < nw; ++w) { s1 += red[0][w]; s2 += red[1][w]; }
  return {s1, s2};
}

__device__ __forceinline__ float gn_xhat(float x, float mean, float rstd) {
  return (x - mean) * rstd;
}

// ---- forward ---------------------------------------------------------------

__device__ __forceinline__ Sum2 gn_stat1(Sum2 s, float v) {
  s.s1 += v;
  s.s2 += v * v;
  return s;
}

struct GnStats {
  float mean, rstd;
};

// Pass 1 of every forward: the group's mean and rstd, saved for backward.
// stage(v8, idx, px) sees each loaded vector first (the LDS-staged kernels
// keep it there); `vec` false takes the scalar form for planes that do
// not vectorise.
template <typename T, int LAYOUT, typename Stage>
__device__ __forceinline__ GnStats gn_fwd_stats(
    const T* xg, int n, int HW, int64_t pstride, bool vec, float eps,
    int group, float* mean_out, float* rstd_out, Stage stage) {
  const int nw = blockDim.x / WAVE;
  Sum2 s = {0.f, 0.f};
  if (vec) {
    // gn_for_packs' walk, written out: a lambda would hold the running
    // sums by reference, which changes what is fused (see Sum2)
    const int nv = n / 8;
    for (int v8 = threadIdx.x; v8 < nv; v8 += blockDim.x) {
      int i = v8 * 8;
      int64_t idx = gn_idx<LAYOUT>(i, i / HW, HW, pstride);
      const Pack<T, 8> px = ld8(&xg[idx]);
      stage(v8, idx, px);
#pragma unroll
      for (int e = 0; e < 8; ++e) s = gn_stat1(s, to_f32(px.v[e]));
    }
  } else {
    for (int i = threadIdx.x; i < n; i += blockDim.x)
      s = gn_stat1(s, to_f32(xg[gn_idx<LAYOUT>(i, i / HW, HW, pstride)]));
  }
  s = block_sum2(s, nw);
  const float mean = s.s1 / n;
  const float var = fmaxf(s.s2 / n - mean * mean, 0.f);
  const float rstd = rsqrtf(var + eps);
  if (threadIdx.x == 0) { mean_out[group] = mean; rstd_out[group] = rstd; }
  return {mean, rstd};
}

// normalise, affine, + residual r, ReLU, round
template <typename T, bool HAS_RES, bool RELU>
__device__ __forceinline__ T gn_apply1(T x, float r, GnStats st, float ga,
                                       float be) {
  float v = gn_xhat(to_f32(x), st.mean, st.rstd);
  v = v * ga + be;
  if (HAS_RES) v += r;
  if (RELU) v = fmaxf(v, 0.f);
  return from_f32<T>(v);
}

template <typename T, bool HAS_RES, bool RELU>
__device__ __forceinline__ Pack<T, 8> gn_apply8(const Pack<T, 8>& px,
                                                const Pack<T, 8>& pr,
                                                GnStats st, float ga,
                                                float be) {
  Pack<T, 8> py;
#pragma unroll
  for (int e = 0; e < 8; ++e)
    py.v[e] = gn_apply1<T, HAS_RES, RELU>(
        px.v[e], HAS_RES ? to_f32(pr.v[e]) : 0.f, st, ga, be);
  return py;
}

// ---- backward --------------------------------------------------------------

// "ReLU kept element e of this vector": always (no ReLU in the forward),
// from the saved y, or from a byte of the padded pair's bitmask.
struct KeepAll {
  static constexpr bool kMasks = false;
  __device__ bool operator()(int) const { return true; }
};
template <typename T>
struct KeepY {
  static constexpr bool kMasks = true;
  Pack<T, 8> py;
  __device__ bool operator()(int e) const { return to_f32(py.v[e]) > 0.f; }
};
struct KeepBits {
  static constexpr bool kMasks = true;
  uint32_t mb;
  __device__ bool operator()(int e) const { return (mb >> e) & 1u; }
};

template <typename T, bool RELU>
__device__ __forceinline__ auto gn_keep_y(const T* yg, int64_t idx) {
  if constexpr (RELU) return KeepY<T>{ld8(&yg[idx])};
  else return KeepAll{};
}

// relu-masked dy: scalar form, and element e of one vector
template <bool RELU, typename T>
__device__ __forceinline__ float gn_grad1(T dy, T y) {
  float grad = to_f32(dy);
  if (RELU) grad = to_f32(y) > 0.f ? grad : 0.f;
  return grad;
}

template <typename T, typename Kept>
__device__ __forceinline__ float gn_grad(const Pack<T, 8>& pdy,
                                         const Kept& kept, int e) {
  float grad = to_f32(pdy.v[e]);
  if (Kept::kMasks) grad = kept(e) ? grad : 0.f;
  return grad;
}

__device__ __forceinline__ float gn_bwd_stat1(float grad, float x, float ga,
                                              GnStats st, float& s1,
                                              float& s2) {
  float xhat = gn_xhat(x, st.mean, st.rstd);
  float dxhat = grad * ga;
  s1 += dxhat;
  s2 += dxhat * xhat;
  return xhat;
}

// one vector's contribution to the group sums and to its channel's
// dgamma/dbeta; returns the masked gradient as stored (dres, and what the
// staged kernels replay in pass 2)
template <typename T, typename Kept>
__device__ __forceinline__ Pack<T, 8> gn_bwd_acc8(
    const Pack<T, 8>& pdy, const Pack<T, 8>& px, float ga, GnStats st,
    const Kept& kept, float& s1, float& s2, float& dg, float& db) {
  Pack<T, 8> pg = pdy;
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    const float grad = gn_grad(pdy, kept, e);
    if (Kept::kMasks) pg.v[e] = from_f32<T>(grad);
    float xhat = gn_bwd_stat1(grad, to_f32(px.v[e]), ga, st, s1, s2);
    dg += grad * xhat;
    db += grad;
  }
  return pg;
}

// Vector pass 1 of every backward.  load_kept(v8, idx) gives the vector's
// ReLU predicate, stage(v8, px, pg) sees x and the masked gradient.  The
// per-channel dgamma/dbeta partials are reduced across the lanes that
// share a channel BEFORE one LDS atomic — per-element atomics serialised
// up to 256 ways on one address when HW >= the block span.  lpc = lanes
// per channel: the largest power of two dividing hv, so an aligned group of
// lpc lanes never straddles a channel (hv itself is not a power of two for
// e.g. 28x28 or 4x6 planes).
template <typename T, int LAYOUT, typename LoadKept, typename Stage>
__device__ __forceinline__ void gn_bwd_pass1(
    const T* xg, const T* dyg, const T* gam, int n, int HW, int64_t pstride,
    GnStats st, float* ch_dg, float* ch_db, float& s1, float& s2,
    LoadKept load_kept, Stage stage) {
  const int lane = threadIdx.x & (WAVE - 1);
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
    int64_t idx = gn_idx<LAYOUT>(i, chan, HW, pstride);
    float dg = 0.f, db = 0.f;
    if (active) {
      const Pack<T, 8> pdy = ld8(&dyg[idx]);
      const Pack<T, 8> px = ld8(&xg[idx]);
      const auto kept = load_kept(v8, idx);
      const float ga = to_f32(gam[chan]);
      stage(v8, px, gn_bwd_acc8(pdy, px, ga, st, kept, s1, s2, dg, db));
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
}

__device__ __forceinline__ float gn_dx1(float grad, float x, float ga,
                                        GnStats st, float m1, float m2) {
  float xhat = gn_xhat(x, st.mean, st.rstd);
  float dxhat = grad * ga;
  return st.rstd * (dxhat - m1 - xhat * m2);
}

// dx of one vector; grad(e) is the masked gradient of element e
template <typename T, typename Grad>
__device__ __forceinline__ Pack<T, 8> gn_dx8(Grad grad, const Pack<T, 8>& px,
                                             float ga, GnStats st, float m1,
                                             float m2) {
  Pack<T, 8> pdx;
#pragma unroll
  for (int e = 0; e < 8; ++e)
    pdx.v[e] = from_f32<T>(gn_dx1(grad(e), to_f32(px.v[e]), ga, st, m1, m2));
  return pdx;
}

// Pass 2 of the LDS-staged backwards: dx (and dres) from the staged x and
// masked gradient.  REPLAY leaves each dx vector in its x slot.
template <typename T, int LAYOUT, bool HAS_RES, bool REPLAY>
__device__ __forceinline__ void gn_bwd_dx_staged(
    Pack<T, 8>* xbuf, const Pack<T, 8>* gbuf, T* dxg, T* drg, const T* gam,
    int n, int HW, int64_t pstride, GnStats st, float m1, float m2) {
  gn_for_packs<LAYOUT>(n, HW, pstride, [&](int v8, int chan, int64_t idx) {
    const Pack<T, 8> px = xbuf[v8];
    const Pack<T, 8> pg = gbuf[v8];
    const float ga = to_f32(gam[chan]);
    const Pack<T, 8> pdx = gn_dx8(
        [&](int e) { return to_f32(pg.v[e]); }, px, ga, st, m1, m2);
    st8(&dxg[idx], pdx);
    if (HAS_RES) st8(&drg[idx], pg);
    if (REPLAY) xbuf[v8] = pdx;
  });
}

// the per-channel dgamma/dbeta partials of one group, in LDS
__device__ __forceinline__ void gn_chan_zero(float* ch_dg, float* ch_db,
                                             int cg) {
  for (int i = threadIdx.x; i < cg; i += blockDim.x) {
    ch_dg[i] = 0.f; ch_db[i] = 0.f;
  }
}

__device__ __forceinline__ void gn_chan_flush(
    float* dgamma, float* dbeta, int64_t aff,
    const float* ch_dg, const float* ch_db, int cg) {
  for (int i = threadIdx.x; i < cg; i += blockDim.x) {
    atomicAdd(&dgamma[aff + i], ch_dg[i]);
    atomicAdd(&dbeta[aff + i], ch_db[i]);
  }
}

// ---- padded image ----------------------------------------------------------

// Writes the group's cg planes of `out` as (H+2) x (W+2) images with a
// zero halo, in aligned 4-element (8-byte) vectors t -> (chan, q, ph, pw).
// vec(chan, off) sets up one vector (off = its offset in the padded
// tensor) and returns elem(li, e): the value of interior element e, whose
// group-local dense index is li.
template <typename Vec>
__device__ __forceinline__ void gn_pad_walk(bf16* out,
                                            const GnGroup& d, int cg, int H,
                                            int W, Vec vec) {
  const int HW = H * W;
  const int PW = W + 2, PHW = (H + 2) * PW;
  const int nvp = PHW / 4;                    // vectors per padded plane
  const int total = cg * nvp;
  for (int t = threadIdx.x; t < total; t += blockDim.x) {
    const int chan = t / nvp;
    const int q = (t - chan * nvp) * 4;
    int ph = q / PW, pw = q - ph * PW;
    const int64_t off = d.pbase + (int64_t)chan * d.ppstride + q;
    auto elem = vec(chan, off);
    Bf4 po;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      bf16 o = from_f32<bf16>(0.f);
      if (ph >= 1 && ph <= H && pw >= 1 && pw <= W)
        o = elem(chan * HW + (ph - 1) * W + (pw - 1), e);
      po.v[e] = o;
      if (++pw == PW) { pw = 0; ++ph; }
    }
    *reinterpret_cast<Bf4*>(&out[off]) = po;
  }
}

// ==== Dense kernels: streaming (STAGED false) and one-global-pass (STAGED true)

template <typename T, bool HAS_RES, bool RELU, int LAYOUT, bool STAGED>
__device__ __forceinline__ void gn_fwd_body(
    const T* x, const T* res, T* y, float* mean_out, float* rstd_out,
    const T* gamma, const T* beta, int Bn, int C, int ch, int G, int HW,
    float eps) {
  const int cg = ch / G;
  const int n = cg * HW;
  const GnGroup d = gn_decode<LAYOUT>(Bn, C, ch, G, HW, /*PHW=*/0);
  const T* xg = x + d.base;
  const T* rg = HAS_RES ? res + d.base : nullptr;
  T* yg = y + d.base;
  Pack<T, 8>* xbuf = nullptr;
  if constexpr (STAGED) xbuf = gn_dyn_lds<T>();

  // the staged kernels are launched only for planes that vectorise
  const bool vec = STAGED || (HW % 8) == 0;
  const GnStats st = gn_fwd_stats<T, LAYOUT>(
      xg, n, HW, d.pstride, vec, eps, d.group, mean_out, rstd_out,
      [&](int v8, int64_t, const Pack<T, 8>& px) {
        if (STAGED) xbuf[v8] = px;
      });

  const T* gam = gamma + d.aff;
  const T* bet = beta + d.aff;
  if (vec) {
    gn_for_packs<LAYOUT>(n, HW, d.pstride, [&](int v8, int chan, int64_t idx) {
      Pack<T, 8> px;
      if (STAGED) px = xbuf[v8]; else px = ld8(&xg[idx]);
      Pack<T, 8> pr;
      if (HAS_RES) pr = ld8(&rg[idx]);
      const float ga = to_f32(gam[chan]), be = to_f32(bet[chan]);
      st8(&yg[idx], gn_apply8<T, HAS_RES, RELU>(px, pr, st, ga, be));
    });
  } else {
    for (int i = threadIdx.x; i < n; i += blockDim.x) {
      int chan = i / HW;
      int64_t idx = gn_idx<LAYOUT>(i, chan, HW, d.pstride);
      yg[idx] = gn_apply1<T, HAS_RES, RELU>(
          xg[idx], HAS_RES ? to_f32(rg[idx]) : 0.f, st, to_f32(gam[chan]),
          to_f32(bet[chan]));
    }
  }
}

template <typename T, bool HAS_RES, bool RELU, int LAYOUT>
__global__ __launch_bounds__(OLS_THREADS) void k_gn_fwd(
    const T* __restrict__ x, const T* __restrict__ res, T* __restrict__ y,
    float* __restrict__ mean_out, float* __restrict__ rstd_out,
    const T* __restrict__ gamma, const T* __restrict__ beta,
    int Bn, int C, int ch, int G, int HW, float eps) {
  gn_fwd_body<T, HAS_RES, RELU, LAYOUT, false>(
      x, res, y, mean_out, rstd_out, gamma, beta, Bn, C, ch, G, HW, eps);
}

// One-global-pass forward: x is staged in LDS during the stats pass and
// replayed for the normalize pass (k_gn_fwd reads it twice).
template <typename T, bool HAS_RES, bool RELU, int LAYOUT>
__global__ __launch_bounds__(OLS_THREADS) void k_gn_fwd_lds(
    const T* __restrict__ x, const T* __restrict__ res, T* __restrict__ y,
    float* __restrict__ mean_out, float* __restrict__ rstd_out,
    const T* __restrict__ gamma, const T* __restrict__ beta,
    int Bn, int C, int ch, int G, int HW, float eps) {
  gn_fwd_body<T, HAS_RES, RELU, LAYOUT, true>(
      x, res, y, mean_out, rstd_out, gamma, beta, Bn, C, ch, G, HW, eps);
}

template <typename T, bool HAS_RES, bool RELU, int LAYOUT, bool STAGED>
__device__ __forceinline__ void gn_bwd_body(
    const T* x, const T* y, const T* dy, T* dx, T* dres,
    const float* mean_in, const float* rstd_in, const T* gamma,
    float* dgamma, float* dbeta, int Bn, int C, int ch, int G, int HW) {
  const int cg = ch / G;
  const int n = cg * HW;
  const GnGroup d = gn_decode<LAYOUT>(Bn, C, ch, G, HW, /*PHW=*/0);
  const T* xg = x + d.base;
  const T* yg = y + d.base;
  const T* dyg = dy + d.base;
  T* dxg = dx + d.base;
  T* drg = HAS_RES ? dres + d.base : nullptr;
  const GnStats st = {mean_in[d.group], rstd_in[d.group]};
  const T* gam = gamma + d.aff;
  Pack<T, 8>* xbuf = nullptr;
  Pack<T, 8>* gbuf = nullptr;
  if constexpr (STAGED) { xbuf = gn_dyn_lds<T>(); gbuf = xbuf + n / 8; }

  const int nw = blockDim.x / WAVE;
  __shared__ float ch_dg[MAX_CG], ch_db[MAX_CG];
  gn_chan_zero(ch_dg, ch_db, cg);
  __syncthreads();

  float s1 = 0.f, s2 = 0.f;
  const bool vec = STAGED || (HW % 8) == 0;
  if (vec) {
    gn_bwd_pass1<T, LAYOUT>(
        xg, dyg, gam, n, HW, d.pstride, st, ch_dg, ch_db, s1, s2,
        [&](int, int64_t idx) { return gn_keep_y<T, RELU>(yg, idx); },
        [&](int v8, const Pack<T, 8>& px, const Pack<T, 8>& pg) {
          if (STAGED) { xbuf[v8] = px; gbuf[v8] = pg; }
        });
  } else {
    for (int i = threadIdx.x; i < n; i += blockDim.x) {
      int chan = i / HW;
      int64_t idx = gn_idx<LAYOUT>(i, chan, HW, d.pstride);
      const float grad = gn_grad1<RELU>(dyg[idx], yg[idx]);
      float xhat = gn_bwd_stat1(grad, to_f32(xg[idx]), to_f32(gam[chan]), st,
                                s1, s2);
      atomicAdd(&ch_dg[chan], grad * xhat);
      atomicAdd(&ch_db[chan], grad);
    }
  }
  const Sum2 s = block_sum2({s1, s2}, nw);
  const float m1 = s.s1 / n, m2 = s.s2 / n;

  if (STAGED) {
    gn_bwd_dx_staged<T, LAYOUT, HAS_RES, false>(
        xbuf, gbuf, dxg, drg, gam, n, HW, d.pstride, st, m1, m2);
  } else if (vec) {
    gn_for_packs<LAYOUT>(n, HW, d.pstride, [&](int, int chan, int64_t idx) {
      const Pack<T, 8> pdy = ld8(&dyg[idx]);
      const Pack<T, 8> px = ld8(&xg[idx]);
      const auto kept = gn_keep_y<T, RELU>(yg, idx);
      const float ga = to_f32(gam[chan]);
      Pack<T, 8> pdr;                  // dres: the masked gradient, rounded
      st8(&dxg[idx], gn_dx8([&](int e) {
            const float grad = gn_grad(pdy, kept, e);
            if (HAS_RES) pdr.v[e] = from_f32<T>(grad);
            return grad;
          }, px, ga, st, m1, m2));
      if (HAS_RES) st8(&drg[idx], pdr);
    });
  } else {
    for (int i = threadIdx.x; i < n; i += blockDim.x) {
      int chan = i / HW;
      int64_t idx = gn_idx<LAYOUT>(i, chan, HW, d.pstride);
      const float grad = gn_grad1<RELU>(dyg[idx], yg[idx]);
      dxg[idx] = from_f32<T>(gn_dx1(grad, to_f32(xg[idx]), to_f32(gam[chan]),
                                    st, m1, m2));
      if (HAS_RES) drg[idx] = from_f32<T>(grad);
    }
  }
  __syncthreads();
  gn_chan_flush(dgamma, dbeta, d.aff, ch_dg, ch_db, cg);
}

template <typename T, bool HAS_RES, bool RELU, int LAYOUT>
__global__ __launch_bounds__(OLS_THREADS) void k_gn_bwd(
    const T* __restrict__ x, const T* __restrict__ y,
    const T* __restrict__ dy, T* __restrict__ dx, T* __restrict__ dres,
    const float* __restrict__ mean_in, const float* __restrict__ rstd_in,
    const T* __restrict__ gamma, float* __restrict__ dgamma,
    float* __restrict__ dbeta, int Bn, int C, int ch, int G, int HW) {
  gn_bwd_body<T, HAS_RES, RELU, LAYOUT, false>(
      x, y, dy, dx, dres, mean_in, rstd_in, gamma, dgamma, dbeta, Bn, C, ch,
      G, HW);
}

// One-global-pass backward: the group's x and (relu-masked) dy are
// staged in LDS during the stats pass and replayed for the dx pass, so
// x/dy stream from HBM once instead of twice (k_gn_bwd reads them in
// both passes).  Fits when 4*n bytes of dynamic LDS are available
// (n = cg*HW; every model group plane is <= 8K elements = 32 KB).
template <typename T, bool HAS_RES, bool RELU, int LAYOUT>
__global__ __launch_bounds__(OLS_THREADS)
__attribute__((amdgpu_waves_per_eu(8))) void k_gn_bwd_lds(
    const T* __restrict__ x, const T* __restrict__ y,
    const T* __restrict__ dy, T* __restrict__ dx, T* __restrict__ dres,
    const float* __restrict__ mean_in, const float* __restrict__ rstd_in,
    const T* __restrict__ gamma, float* __restrict__ dgamma,
    float* __restrict__ dbeta, int Bn, int C, int ch, int G, int HW) {
  gn_bwd_body<T, HAS_RES, RELU, LAYOUT, true>(
      x, y, dy, dx, dres, mean_in, rstd_in, gamma, dgamma, dbeta, Bn, C, ch,
      G, HW);
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
// The statistics passes ARE those of k_gn_fwd_lds / k_gn_bwd_lds — the
// same gn_fwd_stats, gn_bwd_pass1 and gn_bwd_dx_staged, instantiated for
// LAYOUT 1 — so mean/rstd/dx/dres are bit-identical by construction.
//
// Padded planes are (H+2)*(W+2) elements; with H, W even that is a
// multiple of 4, so every plane base is 8-byte aligned and the store pass
// (gn_pad_walk) walks the padded index space in aligned 4-element
// vectors, picking each interior element out of LDS.
//
// Mask layout (private to this pair): per group ceil(n/32) uint32 words;
// bit (i & 31) of word (i >> 5) is y > 0 for group-local dense element
// i = chan*HW + h*W + w, i.e. byte (v8 & 3) of word (v8 >> 2) covers the
// 8-element vector v8 the backward iterates over.

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
  const GnGroup d = gn_decode<1>(Bn, C, ch, G, HW, PHW);
  const int nv = n / 8;
  Pack<bf16, 8>* xbuf = gn_dyn_lds<bf16>();
  Pack<bf16, 8>* rbuf = xbuf + nv;              // RES == 1 only

  const GnStats st = gn_fwd_stats<bf16, 1>(
      x + d.base, n, HW, d.pstride, true, eps, d.group, mean_out, rstd_out,
      [&](int v8, int64_t idx, const Pack<bf16, 8>& px) {
        xbuf[v8] = px;
        if (RES == 1) rbuf[v8] = ld8(&res[d.base + idx]);
      });

  const bf16* gam = gamma + d.aff;
  const bf16* bet = beta + d.aff;
  // element views of the staged x / dense residual; each rounded y is
  // written back over the x it came from (one owner per element) so the
  // mask pass below can read it
  bf16* xe = reinterpret_cast<bf16*>(xbuf);
  const bf16* re = reinterpret_cast<const bf16*>(rbuf);
  if (PAD_OUT) {
    gn_pad_walk(y, d, cg, H, W, [&](int chan, int64_t off) {
      Bf4 pr{};
      if (RES == 2) pr = *reinterpret_cast<const Bf4*>(&res[off]);
      const float ga = to_f32(gam[chan]), be = to_f32(bet[chan]);
      return [=](int li, int e) {
        float r = 0.f;
        if (RES == 1) r = to_f32(re[li]);
        if (RES == 2) r = to_f32(pr.v[e]);
        const bf16 o = gn_apply1<bf16, RES != 0, true>(xe[li], r, st, ga, be);
        xe[li] = o;
        return o;
      };
    });
  } else {
    gn_for_packs<1>(n, HW, d.pstride, [&](int v8, int chan, int64_t idx) {
      const Pack<bf16, 8> px = xbuf[v8];
      Pack<bf16, 8> pr;
      if (RES == 1) pr = rbuf[v8];
      if (RES == 2) {
        const int hw = v8 * 8 - chan * HW;
        const bf16* rp = res + d.pbase + (int64_t)chan * d.ppstride;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          int h = (hw + e) / W, w = (hw + e) - h * W;
          pr.v[e] = rp[(h + 1) * PW + (w + 1)];
        }
      }
      const float ga = to_f32(gam[chan]), be = to_f32(bet[chan]);
      const Pack<bf16, 8> py =
          gn_apply8<bf16, RES != 0, true>(px, pr, st, ga, be);
      xbuf[v8] = py;
      st8(&y[d.base + idx], py);
    });
  }
  __syncthreads();
  const int nwords = (n + 31) / 32;
  uint32_t* mg = mask + (int64_t)d.group * nwords;
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
// wanted).  Passes 1 and 2 are those of k_gn_bwd_lds<.., RELU=true,
// LAYOUT=1> with the mask byte standing in for y > 0.
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
  const GnGroup d = gn_decode<1>(Bn, C, ch, G, HW,
                                 (H + 2) * (W + 2));
  bf16* drg = HAS_RES ? dres + d.base : nullptr;
  const GnStats st = {mean_in[d.group], rstd_in[d.group]};
  const bf16* gam = gamma + d.aff;
  const uint32_t* mg = mask + (int64_t)d.group * ((n + 31) / 32);
  Pack<bf16, 8>* xbuf = gn_dyn_lds<bf16>();
  Pack<bf16, 8>* gbuf = xbuf + n / 8;

  const int nw = blockDim.x / WAVE;
  __shared__ float ch_dg[MAX_CG], ch_db[MAX_CG];
  gn_chan_zero(ch_dg, ch_db, cg);
  __syncthreads();

  float s1 = 0.f, s2 = 0.f;
  gn_bwd_pass1<bf16, 1>(
      x + d.base, dy + d.base, gam, n, HW, d.pstride, st, ch_dg, ch_db, s1,
      s2,
      [&](int v8, int64_t) {
        return KeepBits{mg[v8 >> 2] >> ((v8 & 3) * 8)};
      },
      [&](int v8, const Pack<bf16, 8>& px, const Pack<bf16, 8>& pg) {
        xbuf[v8] = px;
        gbuf[v8] = pg;
      });
  const Sum2 s = block_sum2({s1, s2}, nw);
  const float m1 = s.s1 / n, m2 = s.s2 / n;

  // each dx vector stays in its own x slot: replayed padded below
  gn_bwd_dx_staged<bf16, 1, HAS_RES, true>(
      xbuf, gbuf, dx + d.base, drg, gam, n, HW, d.pstride, st, m1, m2);
  __syncthreads();
  if (dx_pad != nullptr) {
    const bf16* de = reinterpret_cast<const bf16*>(xbuf);
    gn_pad_walk(dx_pad, d, cg, H, W, [&](int, int64_t) {
      return [=](int li, int) { return de[li]; };
    });
  }
  gn_chan_flush(dgamma, dbeta, d.aff, ch_dg, ch_db, cg);
}

// ==== Host side

// "Stage the group in LDS?"  The planes must vectorise (HW % 8 == 0), the
// kernels stage 2-byte types only, and the staging must fit 64 KB, which
// keeps >= 2 blocks resident.
static bool gn_stage_in_lds(int HW, size_t elem_size, size_t lds_bytes) {
  return (HW % 8) == 0 && elem_size == 2 && lds_bytes <= 65536;
}

template <bool V> using BoolC = std::integral_constant<bool, V>;
template <int V> using IntC = std::integral_constant<int, V>;

// (has_res, relu, layout) -> f(BoolC<HAS_RES>, BoolC<RELU>, IntC<LAYOUT>)
template <typename F>
static void gn_dispatch(bool has_res, bool relu, int layout, F f) {
  auto with_layout = [&](auto hr, auto rl) {
    if (layout == 0) f(hr, rl, IntC<0>{}); else f(hr, rl, IntC<1>{});
  };
  if (has_res && relu) with_layout(BoolC<true>{}, BoolC<true>{});
  else if (has_res) with_layout(BoolC<true>{}, BoolC<false>{});
  else if (relu) with_layout(BoolC<false>{}, BoolC<true>{});
  else with_layout(BoolC<false>{}, BoolC<false>{});
}

// The padded pair is used only when BOTH directions fit their LDS staging
// (backward: x + masked dy = 4 B per element, which also covers the
// forward with a staged dense residual) and the planes vectorise.
extern "C" int ols_gn_pad_ok(int ch, int G, int H, int W) {
  if (G <= 0 || ch % G != 0 || ch / G > MAX_CG) return 0;
  if (H < 2 || W < 2 || (H & 1) || (W & 1)) return 0;
  const int64_t n = (int64_t)(ch / G) * H * W;
  return gn_stage_in_lds(H * W, sizeof(bf16), (size_t)n * 2 * sizeof(bf16));
}

extern "C" void ols_groupnorm_fwd_pad(
    const void* x, const void* res, int res_mode, void* y, uint32_t* mask,
    float* mean, float* rstd, const void* gamma, const void* beta, int B,
    int C, int ch, int G, int H, int W, float eps, bool pad_out,
    hipStream_t s) {
  dim3 grid(B * C * G), block(OLS_THREADS);
  const int n = (ch / G) * H * W;
  const size_t lds = (size_t)n * sizeof(bf16) * (res_mode == 1 ? 2 : 1);
  auto launch = [&](auto rm, auto po) {
    hipLaunchKernelGGL(
        (k_gn_fwd_pad<decltype(rm)::value, decltype(po)::value>), grid,
        block, lds, s, (const bf16*)x, (const bf16*)res, (bf16*)y, mask, mean,
        rstd, (const bf16*)gamma, (const bf16*)beta, B, C, ch, G, H, W, eps);
  };
  auto with_pad = [&](auto rm) {
    if (pad_out) launch(rm, BoolC<true>{}); else launch(rm, BoolC<false>{});
  };
  if (res_mode == 0) with_pad(IntC<0>{});
  else if (res_mode == 1) with_pad(IntC<1>{});
  else with_pad(IntC<2>{});
}

extern "C" void ols_groupnorm_bwd_pad(
    const void* x, const uint32_t* mask, const void* dy, void* dx,
    void* dx_pad, void* dres, const float* mean, const float* rstd,
    const void* gamma, float* dgamma, float* dbeta, int B, int C, int ch,
    int G, int H, int W, hipStream_t s) {
  dim3 grid(B * C * G), block(OLS_THREADS);
  const int n = (ch / G) * H * W;
  const size_t lds = (size_t)n * 2 * sizeof(bf16);
  auto launch = [&](auto hr) {
    hipLaunchKernelGGL((k_gn_bwd_pad<decltype(hr)::value>), grid, block, lds,
                       s, (const bf16*)x, mask, (const bf16*)dy, (bf16*)dx,
                       (bf16*)dx_pad, (bf16*)dres, mean, rstd,
                       (const bf16*)gamma, dgamma, dbeta, B, C, ch, G, H, W);
  };
  if (dres != nullptr) launch(BoolC<true>{}); else launch(BoolC<false>{});
}

template <typename T>
static void launch_fwd(const T* x, const T* res, T* y, float* mean,
                       float* rstd, const T* gamma, const T* beta, int B,
                       int C, int ch, int G, int HW, float eps, bool relu,
                       int layout, hipStream_t s) {
  dim3 grid(B * C * G), block(OLS_THREADS);
  const int n = (ch / G) * HW;
  const size_t lds = (size_t)n * sizeof(T);
  const bool use_lds = gn_stage_in_lds(HW, sizeof(T), lds);
  gn_dispatch(res != nullptr, relu, layout, [&](auto hr, auto rl, auto ly) {
    constexpr bool HR = decltype(hr)::value, RL = decltype(rl)::value;
    constexpr int LY = decltype(ly)::value;
    if (use_lds)
      hipLaunchKernelGGL((k_gn_fwd_lds<T, HR, RL, LY>), grid, block, lds, s,
                         x, res, y, mean, rstd, gamma, beta, B, C, ch, G, HW,
                         eps);
    else
      hipLaunchKernelGGL((k_gn_fwd<T, HR, RL, LY>), grid, block, 0, s, x,
                         res, y, mean, rstd, gamma, beta, B, C, ch, G, HW,
                         eps);
  });
}

template <typename T>
static void launch_bwd(const T* x, const T* y, const T* dy, T* dx, T* dres,
                       const float* mean, const float* rstd, const T* gamma,
                       float* dgamma, float* dbeta, int B, int C, int ch,
                       int G, int HW, bool relu, int layout, hipStream_t s) {
  dim3 grid(B * C * G), block(OLS_THREADS);
  // one-global-pass variant when the group plane fits in LDS (4 bytes
  // of staging per element)
  const int n = (ch / G) * HW;
  const size_t lds = (size_t)n * 2 * sizeof(T);
  const bool use_lds = gn_stage_in_lds(HW, sizeof(T), lds);
  gn_dispatch(dres != nullptr, relu, layout, [&](auto hr, auto rl, auto ly) {
    constexpr bool HR = decltype(hr)::value, RL = decltype(rl)::value;
    constexpr int LY = decltype(ly)::value;
    if (use_lds)
      hipLaunchKernelGGL((k_gn_bwd_lds<T, HR, RL, LY>), grid, block, lds, s,
                         x, y, dy, dx, dres, mean, rstd, gamma, dgamma, dbeta,
                         B, C, ch, G, HW);
    else
      hipLaunchKernelGGL((k_gn_bwd<T, HR, RL, LY>), grid, block, 0, s, x, y,
                         dy, dx, dres, mean, rstd, gamma, dgamma, dbeta, B, C,
                         ch, G, HW);
  });
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
    launch_fwd<bf16>((const bf16*)x, (const bf16*)res, (bf16*)y, mean, rstd,
                     (const bf16*)gamma, (const bf16*)beta, B, C, ch, G, HW,
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
    launch_bwd<bf16>((const bf16*)x, (const bf16*)y, (const bf16*)dy,
                     (bf16*)dx, (bf16*)dres, mean, rstd, (const bf16*)gamma,
                     dgamma, dbeta, B, C, ch, G, HW, relu, layout, stream);
}
