// Server optimiser step over the flat fp32 master: FedAvgM and the FedOpt
// family (FedAdagrad, FedAdam, FedYogi; Reddi et al., Algorithm 2, no bias
// correction) in one launch.
//
//   g = d * (1/W) + sigma * z            (z: the round's noise, optional)
//   momentum:  m = b1*m + g;             x += lr*m
//   adagrad:   m = b1*m + (1-b1)*g;  v = v + g^2
//   adam:      same m;               v = b2*v + (1-b2)*g^2
//   yogi:      same m;               v = v - (1-b2)*g^2*sign(v - g^2)
//   adaptive:  x += lr*m / (sqrt(v) + tau)
//
// x, m, v are updated in place; d and z are only read.  Five streams in,
// three out (momentum: three or four in, two out): HBM-bound, so each
// lane moves one 16-byte pack per stream and iteration.  The kind and the
// presence of z are template arguments; a specialisation has no
// per-element branch but Yogi's sign.  sqrtf and / are the correctly
// rounded ones (no fast-math in the build).

#include "common.h"
#include "ols_ops.h"
#include "server_opt_route.h"

struct SoptScalars {
  float inv_w, sigma, lr, b1, omb1, b2, omb2, tau;
};

template <int KIND, bool NOISE>
__device__ __forceinline__ void sopt_elem(float& x, float d, float& m,
                                          float& v, float z,
                                          const SoptScalars& s) {
  float g = d * s.inv_w;
  if (NOISE) g += s.sigma * z;
  if (KIND == SOPT_MOMENTUM) {
    m = s.b1 * m + g;
    x += s.lr * m;
    return;
  }
  m = s.b1 * m + s.omb1 * g;
  const float g2 = g * g;
  if (KIND == SOPT_ADAGRAD) {
    v = v + g2;
  } else if (KIND == SOPT_ADAM) {
    v = s.b2 * v + s.omb2 * g2;
  } else {
    const float diff = v - g2;
    const float sgn = diff > 0.0f ? 1.0f : (diff < 0.0f ? -1.0f : 0.0f);
    v = v - s.omb2 * g2 * sgn;
  }
  x += s.lr * m / (sqrtf(v) + s.tau);
}

// npacks whole packs by grid stride; the n - 4*npacks (< 4) elements after
// them by the first lanes of the last block.
template <int KIND, bool NOISE>
__global__ __launch_bounds__(OLS_THREADS) void k_server_opt_v4(
    float* __restrict__ x, const float* __restrict__ d,
    float* __restrict__ m, float* __restrict__ v,
    const float* __restrict__ z, int64_t npacks, int64_t n, SoptScalars s) {
  constexpr bool HAS_V = KIND != SOPT_MOMENTUM;
  typedef Pack<float, 4> P4;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
       i < npacks; i += stride) {
    P4 px = reinterpret_cast<const P4*>(x)[i];
    const P4 pd = reinterpret_cast<const P4*>(d)[i];
    P4 pm = reinterpret_cast<const P4*>(m)[i];
    P4 pv, pz;
    if (HAS_V) pv = reinterpret_cast<const P4*>(v)[i];
    if (NOISE) pz = reinterpret_cast<const P4*>(z)[i];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      float vk = HAS_V ? pv.v[k] : 0.0f;
      sopt_elem<KIND, NOISE>(px.v[k], pd.v[k], pm.v[k], vk,
                             NOISE ? pz.v[k] : 0.0f, s);
      if (HAS_V) pv.v[k] = vk;
    }
    reinterpret_cast<P4*>(x)[i] = px;
    reinterpret_cast<P4*>(m)[i] = pm;
    if (HAS_V) reinterpret_cast<P4*>(v)[i] = pv;
  }
  const int64_t t = npacks * 4 + threadIdx.x;
  if (blockIdx.x == gridDim.x - 1 && t < n) {
    float vk = HAS_V ? v[t] : 0.0f;
    sopt_elem<KIND, NOISE>(x[t], d[t], m[t], vk, NOISE ? z[t] : 0.0f, s);
    if (HAS_V) v[t] = vk;
  }
}

template <int KIND, bool NOISE>
__global__ __launch_bounds__(OLS_THREADS) void k_server_opt_scalar(
    float* __restrict__ x, const float* __restrict__ d,
    float* __restrict__ m, float* __restrict__ v,
    const float* __restrict__ z, int64_t n, SoptScalars s) {
  constexpr bool HAS_V = KIND != SOPT_MOMENTUM;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += stride) {
    float vk = HAS_V ? v[i] : 0.0f;
    sopt_elem<KIND, NOISE>(x[i], d[i], m[i], vk, NOISE ? z[i] : 0.0f, s);
    if (HAS_V) v[i] = vk;
  }
}

// 256 CUs x 8 resident blocks: past that a memory-bound grid only adds
// launch work, the grid-stride loops take the rest
static constexpr int SOPT_MAX_GRID = 2048;

static inline bool sopt_16b(const void* p) {
  return p == nullptr || reinterpret_cast<uintptr_t>(p) % 16 == 0;
}

template <int KIND, bool NOISE>
static void launch_server_opt(float* x, const float* d, float* m, float* v,
                              const float* z, int64_t n,
                              const SoptScalars& s, hipStream_t stream) {
  const bool aligned = sopt_16b(x) && sopt_16b(d) && sopt_16b(m) &&
                       sopt_16b(v) && sopt_16b(z);
  if (server_opt_route(n, aligned) == SOPT_V4) {
    const int64_t npacks = n / 4;
    int grid = ols_grid(npacks, OLS_THREADS);
    if (grid > SOPT_MAX_GRID) grid = SOPT_MAX_GRID;
    hipLaunchKernelGGL((k_server_opt_v4<KIND, NOISE>), dim3(grid),
                       dim3(OLS_THREADS), 0, stream, x, d, m, v, z, npacks,
                       n, s);
  } else {
    int grid = ols_grid(n, OLS_THREADS);
    if (grid > SOPT_MAX_GRID) grid = SOPT_MAX_GRID;
    hipLaunchKernelGGL((k_server_opt_scalar<KIND, NOISE>), dim3(grid),
                       dim3(OLS_THREADS), 0, stream, x, d, m, v, z, n, s);
  }
}

template <int KIND>
static void launch_server_opt_kind(float* x, const float* d, float* m,
                                   float* v, const float* z, int64_t n,
                                   const SoptScalars& s,
                                   hipStream_t stream) {
  if (z != nullptr)
    launch_server_opt<KIND, true>(x, d, m, v, z, n, s, stream);
  else
    launch_server_opt<KIND, false>(x, d, m, v, nullptr, n, s, stream);
}

extern "C" const char* ols_server_opt_route(int64_t n, int aligned) {
  return server_opt_route_name(server_opt_route(n, aligned != 0));
}

extern "C" void ols_server_opt_step(int kind, float* x, const float* d,
                                    float* m, float* v, const float* z,
                                    int64_t n, float inv_w, float sigma,
                                    float lr, float b1, float b2, float tau,
                                    hipStream_t stream) {
  if (n <= 0) return;
  const SoptScalars s = {inv_w, sigma, lr, b1, 1.0f - b1,
                         b2,    1.0f - b2, tau};
  switch (kind) {
    case SOPT_MOMENTUM:
      launch_server_opt_kind<SOPT_MOMENTUM>(x, d, m, nullptr, z, n, s,
                                            stream);
      break;
    case SOPT_ADAGRAD:
      launch_server_opt_kind<SOPT_ADAGRAD>(x, d, m, v, z, n, s, stream);
      break;
    case SOPT_ADAM:
      launch_server_opt_kind<SOPT_ADAM>(x, d, m, v, z, n, s, stream);
      break;
    default:
      launch_server_opt_kind<SOPT_YOGI>(x, d, m, v, z, n, s, stream);
  }
}
