// Per-client update clipping: the two pieces the aggregation needs
// before it can bound a client's update norm.
//
//   sq[c]   += sum_j (f32(buf[c,j]) - f32(master[j]))^2      (k_delta_sqnorm)
//   s_c      = sq[c] > S^2 ? S / sqrt(sq[c]) : 1             (k_clip_weights)
//   w_eff[c] = w[c] * s_c,   wsum_eff = sum_c w_eff[c]
//
// The clip factor folds into the aggregation weights, so the accumulate
// kernels (aggregate.hip) run unchanged on (w_eff, wsum_eff).
//
// The squared norm subtracts per element in fp32 and is NOT hoisted: the
// replicas sit within lr*grad of the master, so |buf|^2 - 2 buf.m + |m|^2
// would cancel to nothing.  Both kernels are deterministic: no float
// atomics, every sum has one fixed order.

#include "common.h"
#include "ols_ops.h"

// fixed-order sum over the block; the total is valid in thread 0
__device__ __forceinline__ float block_sum(float x) {
  __shared__ float wave_part[OLS_THREADS / WAVE];
  x = wave_sum(x);
  if ((threadIdx.x & (WAVE - 1)) == 0) wave_part[threadIdx.x / WAVE] = x;
  __syncthreads();
  float total = 0.f;
  if (threadIdx.x == 0) {
#pragma unroll
    for (int w = 0; w < OLS_THREADS / WAVE; ++w) total += wave_part[w];
  }
  return total;
}

// grid (tiles, clients): block (t, c) sums elements [t*tile, (t+1)*tile)
// of client c's row.  V elements per lane per load: V*sizeof(T) == 16 on
// the vector path (the host has checked that every row and the master
// start on a 16-byte boundary and V divides n), V == 1 otherwise.  tile
// is a multiple of OLS_THREADS*V.  With one tile per client the block
// adds into sq[c] itself; otherwise it writes part[c*tiles + t] and
// k_sqnorm_finish adds the tiles in order.
template <typename T, int V>
__global__ __launch_bounds__(OLS_THREADS) void k_delta_sqnorm(
    float* __restrict__ sq, float* __restrict__ part,
    const T* __restrict__ buf, const T* __restrict__ master, int64_t n,
    int64_t tile) {
  const int64_t c = blockIdx.y;
  const int64_t j0 = (int64_t)blockIdx.x * tile;
  const int64_t j1 = min(n, j0 + tile);
  const T* row = buf + c * n;
  float acc = 0.f;
#pragma unroll 4
  for (int64_t j = j0 + (int64_t)threadIdx.x * V; j < j1;
       j += (int64_t)OLS_THREADS * V) {
    if constexpr (V == 1) {
      const float d = to_f32(row[j]) - to_f32(master[j]);
      acc += d * d;
    } else {
      const Pack<T, V> p = *reinterpret_cast<const Pack<T, V>*>(&row[j]);
      const Pack<T, V> m = *reinterpret_cast<const Pack<T, V>*>(&master[j]);
#pragma unroll
      for (int e = 0; e < V; ++e) {
        const float d = to_f32(p.v[e]) - to_f32(m.v[e]);
        acc += d * d;
      }
    }
  }
  const float total = block_sum(acc);
  if (threadIdx.x == 0) {
    if (part) part[c * gridDim.x + blockIdx.x] = total;
    else sq[c] += total;
  }
}

__global__ __launch_bounds__(OLS_THREADS) void k_sqnorm_finish(
    float* __restrict__ sq, const float* __restrict__ part, int64_t clients,
    int tiles) {
  const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= clients) return;
  float total = 0.f;
  for (int t = 0; t < tiles; ++t) total += part[c * tiles + t];
  sq[c] += total;
}

// One block: thread t owns clients t, t + 256, ... (fixed order), then the
// fixed block tree.  wsum_eff is summed from the w_eff values as stored.
__global__ __launch_bounds__(OLS_THREADS) void k_clip_weights(
    const float* __restrict__ sq, const float* __restrict__ weights,
    float* __restrict__ w_eff, float* __restrict__ wsum_eff, int64_t clients,
    float clip) {
  const float clip2 = clip * clip;
  float acc = 0.f;
  for (int64_t c = threadIdx.x; c < clients; c += OLS_THREADS) {
    const float q = sq[c];
    const float s = q > clip2 ? clip / sqrtf(q) : 1.f;
    const float we = weights[c] * s;
    w_eff[c] = we;
    acc += we;
  }
  const float total = block_sum(acc);
  if (threadIdx.x == 0) wsum_eff[0] = total;
}

// Elements per tile: enough tiles that clients * tiles fills the chip
// (256 CUs x 8 blocks), but never less than four loads per lane, and a
// multiple of the block's stride so every tile starts vector-aligned.
static int64_t sqnorm_tile(int64_t n, int64_t clients, int vec) {
  const int64_t step = (int64_t)OLS_THREADS * vec;
  const int64_t want = (2048 + clients - 1) / clients;
  const int64_t most = (n + 4 * step - 1) / (4 * step);
  const int64_t tiles = want < most ? want : most;
  const int64_t per = (n + tiles - 1) / tiles;
  return (per + step - 1) / step * step;
}

extern "C" int ols_sqnorm_tiles(int64_t n, int64_t clients, int vec) {
  const int64_t tile = sqnorm_tile(n, clients, vec);
  return (int)((n + tile - 1) / tile);
}

template <typename T, int V>
static void launch_sqnorm(float* sq, float* part, const void* buf,
                          const void* master, int64_t clients, int64_t n,
                          hipStream_t stream) {
  const int64_t tile = sqnorm_tile(n, clients, V);
  dim3 grid((unsigned)((n + tile - 1) / tile), (unsigned)clients);
  hipLaunchKernelGGL((k_delta_sqnorm<T, V>), grid, dim3(OLS_THREADS), 0,
                     stream, sq, grid.x > 1 ? part : nullptr, (const T*)buf,
                     (const T*)master, n, tile);
  if (grid.x > 1)
    hipLaunchKernelGGL(k_sqnorm_finish, dim3(ols_grid(clients, OLS_THREADS)),
                       dim3(OLS_THREADS), 0, stream, sq, part, clients,
                       (int)grid.x);
}

// part: clients * ols_sqnorm_tiles(n, clients, vec) floats of workspace,
// read only when that tile count exceeds 1.  vec: 1, or 16 / itemsize
// when the caller has checked the alignment conditions above.
extern "C" void ols_client_delta_sqnorm(float* sq, float* part,
                                        const void* buf, const void* master,
                                        int64_t clients, int64_t n, int vec,
                                        int dtype, hipStream_t stream) {
  if (clients <= 0 || n <= 0) return;
  switch (dtype) {
    case 0:
      if (vec > 1)
        launch_sqnorm<float, 4>(sq, part, buf, master, clients, n, stream);
      else
        launch_sqnorm<float, 1>(sq, part, buf, master, clients, n, stream);
      break;
    case 1:
      if (vec > 1)
        launch_sqnorm<__hip_bfloat16, 8>(sq, part, buf, master, clients, n,
                                         stream);
      else
        launch_sqnorm<__hip_bfloat16, 1>(sq, part, buf, master, clients, n,
                                         stream);
      break;
    default:
      if (vec > 1)
        launch_sqnorm<__half, 8>(sq, part, buf, master, clients, n, stream);
      else
        launch_sqnorm<__half, 1>(sq, part, buf, master, clients, n, stream);
  }
}

extern "C" void ols_clip_weights(const float* sq, const float* weights,
                                 float* w_eff, float* wsum_eff,
                                 int64_t clients, float clip,
                                 hipStream_t stream) {
  hipLaunchKernelGGL(k_clip_weights, dim3(1), dim3(OLS_THREADS), 0, stream,
                     sq, weights, w_eff, wsum_eff, clients, clip);
}
