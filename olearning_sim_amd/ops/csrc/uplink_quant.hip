// Uplink compression fused into the weighted accumulate: each client's
// update is quantised to k bits per weight (QSGD-style, stochastic, one
// fp32 scale per bucket of 512 elements) as it is read, so the replicas
// are still read once.
//
//   d_q  = f32(buf[c,q]) - f32(master[q])            per element, NOT hoisted
//   a    = max_q |d_q| over the bucket;  a == 0: the bucket adds nothing
//   t_q  = |d_q| * L / a,   L = 2^(b-1) - 1
//   l_q  = min(L, floor(t_q) + [u_q < t_q - floor(t_q)])
//   delta[q] += sum_c w[c] * sign(d_q) * l_q * (a / L)
//
// The kernels of aggregate.hip hoist W * master out of the client loop and
// cannot host this: the quantiser needs the per-element difference (the
// cancellation argument of clip.hip's header) inside the loop.
//
// u_q is 16 bits of a counter hash of (key, client id, element index in
// the flat master), so a draw does not depend on chunking, grid or route:
//
//   ckey = fmix32(fmix32(k0 ^ cid) ^ k1)                  once per client
//   word = fmix32(ckey ^ (p * 0x9E3779B9)),  p = j >> 1   once per PAIR
//   u    = (j even ? word & 0xFFFF : word >> 16) / 65536
//
// One wave owns one bucket and keeps its master fragment and its fp32
// partial sums in registers through the client loop.  v8: a lane owns 8
// consecutive elements (16-byte packs); scalar: lanes stride through the
// bucket, any n, any alignment.  The bucket maximum is a DPP reduction
// inside each row of 16 lanes and four lane reads across the rows, which
// also leaves it wave-uniform for the one division per client.  Client
// tiles of 64 go on grid y once clients >= 64 and add into delta with
// float atomics (as the cpar kernels of aggregate.hip do); below that one
// tile adds with a plain += and the launch is deterministic.
//
// Non-finite inputs are not hidden: the maximum is taken on the bit
// patterns of |d|, where a NaN sorts above infinity, and poisons its
// bucket.  A client of weight 0 is skipped without reading its row.

#include "common.h"
#include "ols_ops.h"
#include "uplink_route.h"

#define UPLINK_UNROLL 4
#define UPLINK_PER_LANE (UPLINK_BUCKET / WAVE)
#define UPLINK_WAVES (OLS_THREADS / WAVE)

static_assert(UPLINK_PER_LANE == 8, "a lane owns 8 elements of a bucket");
static_assert(UPLINK_CTILE <= OLS_THREADS, "one thread stages one client");

__device__ __forceinline__ uint32_t fmix32(uint32_t h) {
  h ^= h >> 16;
  h *= 0x85EBCA6Bu;
  h ^= h >> 13;
  h *= 0xC2B2AE35u;
  h ^= h >> 16;
  return h;
}

template <int CTRL>
__device__ __forceinline__ uint32_t dpp_max_u32(uint32_t x) {
  const uint32_t y = (uint32_t)__builtin_amdgcn_update_dpp(
      0, (int)x, CTRL, 0xF, 0xF, true);
  return x > y ? x : y;
}

// maximum over the wave of 64, the same value in every lane and uniform
// to the compiler.  All 64 lanes must be active.
__device__ __forceinline__ uint32_t wave_max_u32(uint32_t x) {
  x = dpp_max_u32<0xB1>(x);   // quad_perm [1,0,3,2]
  x = dpp_max_u32<0x4E>(x);   // quad_perm [2,3,0,1]
  x = dpp_max_u32<0x141>(x);  // row_half_mirror
  x = dpp_max_u32<0x140>(x);  // row_mirror: every lane has its row's max
  const uint32_t r0 = (uint32_t)__builtin_amdgcn_readlane((int)x, 0);
  const uint32_t r1 = (uint32_t)__builtin_amdgcn_readlane((int)x, 16);
  const uint32_t r2 = (uint32_t)__builtin_amdgcn_readlane((int)x, 32);
  const uint32_t r3 = (uint32_t)__builtin_amdgcn_readlane((int)x, 48);
  const uint32_t m01 = r0 > r1 ? r0 : r1;
  const uint32_t m23 = r2 > r3 ? r2 : r3;
  return m01 > m23 ? m01 : m23;
}

// The 8 elements lane `lane` owns of the bucket starting at b0: element e
// is q = first + e * step.
template <bool VEC>
__device__ __forceinline__ int64_t lane_first(int64_t b0, int lane) {
  return VEC ? b0 + (int64_t)lane * UPLINK_PER_LANE : b0 + lane;
}
template <bool VEC>
__device__ __forceinline__ int lane_step() {
  return VEC ? 1 : WAVE;
}

// A lane's 8 elements of a row; elements at or past n read as zero, in
// the master fragment too, so their difference is zero.
template <typename T, bool VEC>
__device__ __forceinline__ void load_frag(Pack<T, 8>& f,
                                          const T* __restrict__ row,
                                          int64_t first, int64_t n) {
  if constexpr (VEC) {
    // n % 8 == 0: a lane's pack lies inside the row or wholly past it
    if (first < n) {
      f = *reinterpret_cast<const Pack<T, 8>*>(&row[first]);
    } else {
#pragma unroll
      for (int e = 0; e < 8; ++e) f.v[e] = from_f32<T>(0.f);
    }
  } else {
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const int64_t q = first + (int64_t)e * WAVE;
      f.v[e] = q < n ? row[q] : from_f32<T>(0.f);
    }
  }
}

// PAIRED: VEC with an even elem_base, where a lane's 8 elements are 4
// whole pairs and one hash serves two of them.  Otherwise every element
// hashes its own pair's word and takes its half.
template <typename T, bool VEC, bool PAIRED>
__global__ __launch_bounds__(OLS_THREADS) void k_delta_accum_quant(
    float* __restrict__ delta, const T* __restrict__ buf,
    const T* __restrict__ master, const float* __restrict__ weights,
    const int64_t* __restrict__ cids, int64_t clients, int64_t n,
    int64_t elem_base, int levels, uint32_t k0, uint32_t k1) {
  static_assert(VEC || !PAIRED, "pairs need consecutive elements");
  __shared__ float w_lds[UPLINK_CTILE];
  __shared__ uint32_t key_lds[UPLINK_CTILE];
  const int64_t c0 = (int64_t)blockIdx.y * UPLINK_CTILE;
  const int tile = (int)min((int64_t)UPLINK_CTILE, clients - c0);
  if ((int)threadIdx.x < tile) {
    w_lds[threadIdx.x] = weights[c0 + threadIdx.x];
    key_lds[threadIdx.x] =
        fmix32(fmix32(k0 ^ (uint32_t)cids[c0 + threadIdx.x]) ^ k1);
  }
  __syncthreads();

  const int lane = threadIdx.x & (WAVE - 1);
  const int64_t b0 =
      ((int64_t)blockIdx.x * UPLINK_WAVES + threadIdx.x / WAVE) *
      UPLINK_BUCKET;
  if (b0 >= n) return;  // the whole wave: no lane of it has an element
  const int64_t first = lane_first<VEC>(b0, lane);
  constexpr int step = VEC ? 1 : WAVE;

  Pack<T, 8> mf;
  load_frag<T, VEC>(mf, master, first, n);
  float m[8], acc[8];
  // client-independent half of the hash argument, and which half of the
  // word an element takes (bit e of odd)
  uint32_t pm[PAIRED ? 4 : 8];
  uint32_t odd = 0;
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    m[e] = to_f32(mf.v[e]);
    acc[e] = 0.f;
    const uint64_t j = (uint64_t)elem_base + (uint64_t)(first + e * step);
    if constexpr (PAIRED) {
      if ((e & 1) == 0) pm[e >> 1] = (uint32_t)(j >> 1) * 0x9E3779B9u;
    } else {
      pm[e] = (uint32_t)(j >> 1) * 0x9E3779B9u;
      odd |= (uint32_t)(j & 1) << e;
    }
  }
  const float Lf = (float)levels;

  for (int c = 0; c < tile; c += UPLINK_UNROLL) {
    // the rows of the next clients are requested before the first of
    // them is reduced
    Pack<T, 8> r[UPLINK_UNROLL];
    float w[UPLINK_UNROLL];
#pragma unroll
    for (int u = 0; u < UPLINK_UNROLL; ++u) {
      const float wl = c + u < tile ? w_lds[min(c + u, tile - 1)] : 0.f;
      w[u] = __int_as_float(
          __builtin_amdgcn_readfirstlane(__float_as_int(wl)));
      if (w[u] != 0.f)
        load_frag<T, VEC>(r[u], buf + (c0 + c + u) * n, first, n);
    }
#pragma unroll
    for (int u = 0; u < UPLINK_UNROLL; ++u) {
      if (w[u] == 0.f) continue;  // wave-uniform
      const uint32_t ckey = (uint32_t)__builtin_amdgcn_readfirstlane(
          (int)key_lds[min(c + u, tile - 1)]);
      float d[8];
      uint32_t am = 0;
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        d[e] = to_f32(r[u].v[e]) - m[e];
        const uint32_t bits = __float_as_uint(d[e]) & 0x7FFFFFFFu;
        am = bits > am ? bits : am;
      }
      const float a = __uint_as_float(wave_max_u32(am));
      if (a == 0.f) continue;  // wave-uniform; a NaN goes on
      const float inv = Lf / a;
      const float s = w[u] * a / Lf;
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        uint32_t k;
        if constexpr (PAIRED) {
          const uint32_t word = fmix32(ckey ^ pm[e >> 1]);
          k = (e & 1) ? word >> 16 : word & 0xFFFFu;
        } else {
          const uint32_t word = fmix32(ckey ^ pm[e]);
          k = (odd >> e) & 1 ? word >> 16 : word & 0xFFFFu;
        }
        const float ad = fabsf(d[e]);
        const float t = ad * inv;
        const float fl = floorf(t);
        // t - fl and its scaling by 2^16 are exact in fp32
        float lvl = fl + ((float)k < (t - fl) * 65536.f ? 1.f : 0.f);
        lvl = lvl > Lf ? Lf : lvl;  // keeps a NaN
        // the bucket's maximum is level L whatever a * (L / a) rounds to
        lvl = ad == a ? Lf : lvl;
        acc[e] = fmaf(s, copysignf(lvl, d[e]), acc[e]);
      }
    }
  }

  const bool tiles = gridDim.y > 1;
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    const int64_t q = first + (int64_t)e * step;
    if (q < n) {
      if (tiles) atomicAdd(&delta[q], acc[e]);
      else delta[q] += acc[e];
    }
  }
}

extern "C" const char* ols_delta_accum_quant_route(int64_t n, int64_t clients,
                                                   int dtype, int master_16b,
                                                   int buf_16b) {
  return uplink_route_name(uplink_quant_route(n, clients, dtype,
                                              master_16b != 0, buf_16b != 0));
}

template <typename T>
static void launch_quant(float* delta, const void* buf, const void* master,
                         const float* weights, const int64_t* cids,
                         int64_t clients, int64_t n, int64_t elem_base,
                         int levels, uint32_t k0, uint32_t k1,
                         UplinkRoute route, hipStream_t stream) {
  const int64_t buckets = (n + UPLINK_BUCKET - 1) / UPLINK_BUCKET;
  dim3 grid((unsigned)((buckets + UPLINK_WAVES - 1) / UPLINK_WAVES),
            (unsigned)uplink_client_tiles(clients));
  dim3 block(OLS_THREADS);
#define OLS_QUANT_LAUNCH(VEC, PAIRED)                                        \
  hipLaunchKernelGGL((k_delta_accum_quant<T, VEC, PAIRED>), grid, block, 0,  \
                     stream, delta, (const T*)buf, (const T*)master, weights, \
                     cids, clients, n, elem_base, levels, k0, k1)
  if (route == UPLINK_V8) {
    if (elem_base % 2 == 0) OLS_QUANT_LAUNCH(true, true);
    else OLS_QUANT_LAUNCH(true, false);
  } else {
    OLS_QUANT_LAUNCH(false, false);
  }
#undef OLS_QUANT_LAUNCH
}

extern "C" void ols_delta_accum_quant(float* delta, const void* buf,
                                      const void* master,
                                      const float* weights,
                                      const int64_t* cids, int64_t clients,
                                      int64_t n, int64_t elem_base, int bits,
                                      uint32_t k0, uint32_t k1, int dtype,
                                      hipStream_t stream) {
  const int levels = uplink_levels(bits);
  if (clients <= 0 || n <= 0 || levels == 0) return;
  const UplinkRoute route = uplink_quant_route(
      n, clients, dtype, reinterpret_cast<uintptr_t>(master) % 16 == 0,
      reinterpret_cast<uintptr_t>(buf) % 16 == 0);
  switch (dtype) {
    case 0:
      launch_quant<float>(delta, buf, master, weights, cids, clients, n,
                          elem_base, levels, k0, k1, route, stream);
      break;
    case 1:
      launch_quant<__hip_bfloat16>(delta, buf, master, weights, cids, clients,
                                   n, elem_base, levels, k0, k1, route,
                                   stream);
      break;
    default:
      launch_quant<__half>(delta, buf, master, weights, cids, clients, n,
                           elem_base, levels, k0, k1, route, stream);
  }
}
