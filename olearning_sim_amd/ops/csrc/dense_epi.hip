// What stands between the GEMMs of one BertLM encoder layer, for gfx950:
// bias + GELU after ffn_in, and bias + residual + LayerNorm after attn_out
// and ffn_out.  The GEMMs run without bias (blinear(x, w, None)) and these
// kernels read their bf16 output z once:
//   k_bias_gelu_fwd   y = bf16(gelu(z + b)), exact erf form;
//   k_bias_gelu_bwd   dz = bf16(dy * gelu'(z + b)), z + b recomputed, and the
//                     column sums of dz per row block;
//   k_brln_fwd        s = bf16(z + b + res), y = LayerNorm(s) * gamma + beta,
//                     mean and rstd of s;
//   k_brln_bwd        ds (the gradient of z and of res alike), and per row
//                     block the column sums that make dgamma, dbeta and db;
//   k_colsum_finish   adds the row blocks' strips in index order: bf16 sums.
// bf16 only, fp32 arithmetic in registers, every global access of a row
// operand a 16-byte pack of 8.  No atomics: every sum has one fixed order, so
// two runs give the same bits.
//
// Who owns what.  A lane owns columns: pack u of lane l covers columns
// (u * 64 + l) * 8 .. + 8 of its workgroup's column range, for every row the
// lane's wave touches.  What belongs to columns (the bias, gamma, beta, the
// column sums) therefore lives in that lane's registers for the whole kernel
// and costs one load per workgroup, not one per row.  A workgroup of four
// waves owns one client and one block of consecutive rows, so a block never
// straddles clients and the last block of a client may be short; wave w takes
// rows w, w + 4, ... of the block.
//
// GELU kernels: grid (column chunk of 512 = 64 lanes x 8, row block, client),
// one pack per lane and row, four rows in flight per wave.  u = f32(z) +
// f32(b) is never rounded.  With t = |u| / sqrt 2 and e0 = exp(-t^2) (one
// v_exp_f32, shared by both), Phi(u) comes from erf(t) = t (2/sqrt pi + t^2
// P(t^2)) for t <= 1 and from erfc(t) = e0 R(1/t) / t for t > 1, where the
// negative tail keeps its relative accuracy (Phi = erfc / 2, no 1 - 1
// cancellation), and phi(u) = e0 / sqrt(2 pi).  P and R are least-squares
// Chebyshev fits (degree 5 on [0, 1], degree 10 on [0.1, 1]); evaluated in
// fp32 they are within 1.5e-7 absolute (erf) and 2e-7 relative (erfc) of the
// functions; past t = 10 e0 is zero.  db sums the ROUNDED dz, the values the
// weight-gradient GEMM sees, rows in ascending order per wave.
//
// LayerNorm kernels: one wave per row, the whole row in registers: NP = 1, 2
// or 3 packs per lane for H up to 512, 1024, 1536 (a template parameter, so
// the register arrays are static); lanes past H / 8 packs idle.  Forward:
// grid (ceil(N / 16), client), a wave four rows.  Mean and variance are
// taken over the rounded s, the variance as the mean of (s - mean)^2 since
// the row is resident: y is the LayerNorm of exactly the tensor the backward
// reads.  Backward: grid (row block, client); per row two wave reductions
// (the means of dy gamma and of dy gamma xhat), ds stored once, and three
// fp32 partial sums per owned column: dy xhat, dy and the rounded ds.
//
// Combining the waves.  The four waves' column sums meet in one LDS strip, in
// wave order: wave 0 stores, waves 1 and 2 add to their own lanes' slots,
// wave 3 adds and writes the strip to the scratch [C, row_blocks, K, W]
// (K = 1: db of the GELU; K = 3: dgamma, dbeta, db).  k_colsum_finish then
// reduces over row_blocks into a bf16 [K, C, W].
//
// 1/sqrt is v_rsq_f32 and exp is v_exp_f32 (one ulp each): tests pass
// intrinsic=True to the bounds.
//
// Sizes: widths below 2^30, C and (for the GELU) the number of row blocks at
// most 65535 (grid y and z).  Every row and element offset is 64-bit.

#include <initializer_list>

#include "common.h"
#include "dense_epi_route.h"
#include "ols_ops.h"

#define DE_THREADS 256
#define DE_WAVES 4
#define DE_CHUNK 512      // columns of one GELU workgroup
#define DE_UNROLL 4       // GELU: rows in flight per wave
#define DE_LN_FWD_ROWS 16 // LayerNorm forward: rows per workgroup
#define DE_LOG2E 1.44269504088896341f
#define DE_RSQRT2 0.707106781186547524f
#define DE_RSQRT2PI 0.398942280401432678f
#define DE_2RSQRTPI 1.12837916709551257f

// Compiled without packed fp32 arithmetic (v_pk_*_f32), as head_ce.hip: a
// function with another target feature set is not inlined, so everything the
// kernels call is defined here on compiler builtins.
#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute push(__attribute__((target("no-packed-fp32-ops"))), \
                             apply_to = function)
#endif

// 8 bf16 as one 16-byte load or store
struct __attribute__((aligned(16))) DePack {
  unsigned short e[8];
};
struct __attribute__((aligned(16))) DeFloat4 {
  float v[4];
};
struct __attribute__((aligned(8))) DeHalfPack {
  unsigned short e[4];
};

__device__ __forceinline__ float de_val(unsigned short b) {
  return __builtin_bit_cast(float, ((unsigned)b) << 16);
}
// round-to-nearest-even bf16 bits of an fp32, NaN kept a NaN
__device__ __forceinline__ unsigned short de_bits(float v) {
  const unsigned u = __builtin_bit_cast(unsigned, v);
  if (v != v) return 0x7FC0u;
  return (unsigned short)((u + 0x7FFFu + ((u >> 16) & 1u)) >> 16);
}
__device__ __forceinline__ DePack de_load(const unsigned short* p) {
  return *reinterpret_cast<const DePack*>(p);
}
__device__ __forceinline__ void de_store(unsigned short* p, const DePack& v) {
  *reinterpret_cast<DePack*>(p) = v;
}
// Needs EXEC all ones: called under wave-uniform control flow only.
__device__ __forceinline__ float de_wave_sum(float v, int lane) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1)
    v += __builtin_bit_cast(
        float, __builtin_amdgcn_ds_bpermute((lane ^ off) << 2,
                                            __builtin_bit_cast(int, v)));
  return v;
}
__device__ __forceinline__ void de_barrier() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __builtin_amdgcn_s_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

// Phi(u), the normal distribution function, and phi(u), its density
__device__ __forceinline__ void de_normal(float u, float& Phi, float& phi) {
  const float t = __builtin_fabsf(u) * DE_RSQRT2;
  const float s = t * t;
  const float e0 = __builtin_amdgcn_exp2f(-s * DE_LOG2E);
  float half;               // erf(t) / 2 or erfc(t) / 2
  if (t <= 1.f) {
    float p = 8.386720583e-05f;
    p = __builtin_fmaf(p, s, -8.163732127e-04f);
    p = __builtin_fmaf(p, s, 5.204732064e-03f);
    p = __builtin_fmaf(p, s, -2.686175518e-02f);
    p = __builtin_fmaf(p, s, 1.128375456e-01f);
    p = __builtin_fmaf(p, s, -3.761263788e-01f);
    half = 0.5f * (t * __builtin_fmaf(p, s, DE_2RSQRTPI));
    Phi = u < 0.f ? 0.5f - half : 0.5f + half;
  } else {
    const float w = __builtin_amdgcn_rcpf(t);
    float r = -4.841774330e-02f;
    r = __builtin_fmaf(r, w, 2.366587967e-01f);
    r = __builtin_fmaf(r, w, -4.065380692e-01f);
    r = __builtin_fmaf(r, w, 1.043805927e-01f);
    r = __builtin_fmaf(r, w, 6.741221547e-01f);
    r = __builtin_fmaf(r, w, -1.163484573e+00f);
    r = __builtin_fmaf(r, w, 8.207785487e-01f);
    r = __builtin_fmaf(r, w, -8.133351803e-02f);
    r = __builtin_fmaf(r, w, -2.721191049e-01f);
    r = __builtin_fmaf(r, w, -6.721213576e-04f);
    r = __builtin_fmaf(r, w, 5.642085671e-01f);
    half = 0.5f * (w * r * e0);
    Phi = u < 0.f ? half : 1.f - half;
  }
  phi = e0 * DE_RSQRT2PI;
}

// The waves' column sums acc[n] (column slot0 + j of the strip for acc[j])
// added in wave order through `strip`; the last wave's lanes hold the total
// on return (the others' acc is unchanged).  All four waves call it.
template <int NACC>
__device__ __forceinline__ void de_combine(float* strip, float (&acc)[NACC],
                                           int slot0, int wave) {
#pragma unroll
  for (int w = 0; w < DE_WAVES; ++w) {
    if (wave == w) {                                     // wave-uniform
#pragma unroll
      for (int j = 0; j < NACC; ++j) {
        if (w > 0) acc[j] += strip[slot0 + j];
        if (w < DE_WAVES - 1) strip[slot0 + j] = acc[j];
      }
    }
    if (w < DE_WAVES - 1) de_barrier();
  }
}

// ---------------------------------------------------------------------------
__global__ __launch_bounds__(DE_THREADS) void k_bias_gelu_fwd(
    const unsigned short* __restrict__ z, const unsigned short* __restrict__ b,
    unsigned short* __restrict__ y, int N, int F, int row_block) {
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int c = blockIdx.z;
  const int col = blockIdx.x * DE_CHUNK + lane * 8;
  if (col >= F) return;
  const int r0 = blockIdx.y * row_block;
  const int r1 = r0 + row_block < N ? r0 + row_block : N;

  float bv[8];
  {
    const DePack pb = de_load(b + (int64_t)c * F + col);
#pragma unroll
    for (int j = 0; j < 8; ++j) bv[j] = de_val(pb.e[j]);
  }
  for (int ra = r0 + wave; ra < r1; ra += DE_WAVES * DE_UNROLL) {
    DePack raw[DE_UNROLL];
#pragma unroll
    for (int i = 0; i < DE_UNROLL; ++i) {
      const int r = ra + DE_WAVES * i;
      if (r < r1) raw[i] = de_load(z + ((int64_t)c * N + r) * F + col);
    }
#pragma unroll
    for (int i = 0; i < DE_UNROLL; ++i) {
      const int r = ra + DE_WAVES * i;
      if (r >= r1) continue;
      DePack o;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float u = de_val(raw[i].e[j]) + bv[j];
        float Phi, phi;
        de_normal(u, Phi, phi);
        o.e[j] = de_bits(u * Phi);
      }
      de_store(y + ((int64_t)c * N + r) * F + col, o);
    }
  }
}

// part [C, gridDim.y, F] fp32: the column sums of dz over this row block
__global__ __launch_bounds__(DE_THREADS) void k_bias_gelu_bwd(
    const unsigned short* __restrict__ z, const unsigned short* __restrict__ b,
    const unsigned short* __restrict__ dy, unsigned short* __restrict__ dz,
    float* __restrict__ part, int N, int F, int row_block) {
  __shared__ float strip[DE_CHUNK];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int c = blockIdx.z;
  const int col = blockIdx.x * DE_CHUNK + lane * 8;
  const bool ok = col < F;
  const int r0 = blockIdx.y * row_block;
  const int r1 = r0 + row_block < N ? r0 + row_block : N;

  float bv[8], acc[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) bv[j] = acc[j] = 0.f;
  if (ok) {
    const DePack pb = de_load(b + (int64_t)c * F + col);
#pragma unroll
    for (int j = 0; j < 8; ++j) bv[j] = de_val(pb.e[j]);
    for (int ra = r0 + wave; ra < r1; ra += DE_WAVES * DE_UNROLL) {
      DePack rz[DE_UNROLL], rd[DE_UNROLL];
#pragma unroll
      for (int i = 0; i < DE_UNROLL; ++i) {
        const int r = ra + DE_WAVES * i;
        if (r < r1) {
          const int64_t at = ((int64_t)c * N + r) * F + col;
          rz[i] = de_load(z + at);
          rd[i] = de_load(dy + at);
        }
      }
#pragma unroll
      for (int i = 0; i < DE_UNROLL; ++i) {
        const int r = ra + DE_WAVES * i;
        if (r >= r1) continue;
        DePack o;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const float u = de_val(rz[i].e[j]) + bv[j];
          float Phi, phi;
          de_normal(u, Phi, phi);
          o.e[j] = de_bits(de_val(rd[i].e[j]) * __builtin_fmaf(u, phi, Phi));
          acc[j] += de_val(o.e[j]);
        }
        de_store(dz + ((int64_t)c * N + r) * F + col, o);
      }
    }
  }
  de_combine<8>(strip, acc, lane * 8, wave);
  if (wave == DE_WAVES - 1 && ok) {
    float* dst = part + ((int64_t)c * gridDim.y + blockIdx.y) * F + col;
#pragma unroll
    for (int q = 0; q < 2; ++q)
      *reinterpret_cast<DeFloat4*>(dst + 4 * q) =
          DeFloat4{{acc[4 * q], acc[4 * q + 1], acc[4 * q + 2],
                    acc[4 * q + 3]}};
  }
}

// ---------------------------------------------------------------------------
template <int NP>
__global__ __launch_bounds__(DE_THREADS) void k_brln_fwd(
    const unsigned short* __restrict__ z, const unsigned short* __restrict__ b,
    const unsigned short* __restrict__ res,
    const unsigned short* __restrict__ gamma,
    const unsigned short* __restrict__ beta, unsigned short* __restrict__ y,
    unsigned short* __restrict__ s_out, float* __restrict__ mean_out,
    float* __restrict__ rstd_out, int N, int H, float eps) {
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int c = blockIdx.y;
  const int r0 = blockIdx.x * DE_LN_FWD_ROWS;
  const float inv_h = 1.f / (float)H;

  int col[NP];
  bool ok[NP];
  DePack pb[NP], pg[NP], pe[NP];
#pragma unroll
  for (int u = 0; u < NP; ++u) {
    col[u] = (u * 64 + lane) * 8;
    ok[u] = col[u] < H;
    if (ok[u]) {
      pb[u] = de_load(b + (int64_t)c * H + col[u]);
      pg[u] = de_load(gamma + (int64_t)c * H + col[u]);
      pe[u] = de_load(beta + (int64_t)c * H + col[u]);
    }
  }
  for (int r = r0 + wave; r < r0 + DE_LN_FWD_ROWS && r < N; r += DE_WAVES) {
    const int64_t row = (int64_t)c * N + r;
    DePack pz[NP], pr[NP];
#pragma unroll
    for (int u = 0; u < NP; ++u)
      if (ok[u]) {
        pz[u] = de_load(z + row * H + col[u]);
        pr[u] = de_load(res + row * H + col[u]);
      }
    float sv[NP][8];
    float sum = 0.f;
#pragma unroll
    for (int u = 0; u < NP; ++u) {
      if (!ok[u]) continue;
      DePack ps;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        ps.e[j] = de_bits(de_val(pz[u].e[j]) + de_val(pb[u].e[j]) +
                          de_val(pr[u].e[j]));
        sv[u][j] = de_val(ps.e[j]);
        sum += sv[u][j];
      }
      de_store(s_out + row * H + col[u], ps);
    }
    const float mean = de_wave_sum(sum, lane) * inv_h;
    float sq = 0.f;
#pragma unroll
    for (int u = 0; u < NP; ++u) {
      if (!ok[u]) continue;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        sv[u][j] -= mean;
        sq = __builtin_fmaf(sv[u][j], sv[u][j], sq);
      }
    }
    const float rstd =
        __builtin_amdgcn_rsqf(de_wave_sum(sq, lane) * inv_h + eps);
    if (lane == 0) {
      mean_out[row] = mean;
      rstd_out[row] = rstd;
    }
#pragma unroll
    for (int u = 0; u < NP; ++u) {
      if (!ok[u]) continue;
      DePack o;
#pragma unroll
      for (int j = 0; j < 8; ++j)
        o.e[j] = de_bits(__builtin_fmaf(sv[u][j] * rstd, de_val(pg[u].e[j]),
                                        de_val(pe[u].e[j])));
      de_store(y + row * H + col[u], o);
    }
  }
}

// part [C, gridDim.x, 3, H] fp32: this row block's column sums of dy * xhat
// (dgamma), dy (dbeta) and the rounded ds (db)
template <int NP>
__global__ __launch_bounds__(DE_THREADS) void k_brln_bwd(
    const unsigned short* __restrict__ s, const unsigned short* __restrict__ dy,
    const unsigned short* __restrict__ gamma, const float* __restrict__ mean_in,
    const float* __restrict__ rstd_in, unsigned short* __restrict__ ds,
    float* __restrict__ part, int N, int H, int row_block) {
  __shared__ float strip[3 * NP * 512];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int c = blockIdx.y;
  const int r0 = blockIdx.x * row_block;
  const int r1 = r0 + row_block < N ? r0 + row_block : N;
  const float inv_h = 1.f / (float)H;

  int col[NP];
  bool ok[NP];
  DePack pg[NP];
  float acc[3 * NP * 8];    // [k][u][j]
#pragma unroll
  for (int i = 0; i < 3 * NP * 8; ++i) acc[i] = 0.f;
#pragma unroll
  for (int u = 0; u < NP; ++u) {
    col[u] = (u * 64 + lane) * 8;
    ok[u] = col[u] < H;
    if (ok[u]) pg[u] = de_load(gamma + (int64_t)c * H + col[u]);
  }
  for (int r = r0 + wave; r < r1; r += DE_WAVES) {
    const int64_t row = (int64_t)c * N + r;
    DePack px[NP], pd[NP];
#pragma unroll
    for (int u = 0; u < NP; ++u)
      if (ok[u]) {
        px[u] = de_load(s + row * H + col[u]);
        pd[u] = de_load(dy + row * H + col[u]);
      }
    const float mean = mean_in[row], rstd = rstd_in[row];
    float xh[NP][8], dxh[NP][8];
    float s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int u = 0; u < NP; ++u) {
      if (!ok[u]) continue;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float g = de_val(pd[u].e[j]);
        xh[u][j] = (de_val(px[u].e[j]) - mean) * rstd;
        dxh[u][j] = g * de_val(pg[u].e[j]);
        s1 += dxh[u][j];
        s2 = __builtin_fmaf(dxh[u][j], xh[u][j], s2);
        acc[(0 * NP + u) * 8 + j] =
            __builtin_fmaf(g, xh[u][j], acc[(0 * NP + u) * 8 + j]);
        acc[(1 * NP + u) * 8 + j] += g;
      }
    }
    const float m1 = de_wave_sum(s1, lane) * inv_h;
    const float m2 = de_wave_sum(s2, lane) * inv_h;
#pragma unroll
    for (int u = 0; u < NP; ++u) {
      if (!ok[u]) continue;
      DePack o;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        o.e[j] = de_bits(rstd * (dxh[u][j] - m1 - xh[u][j] * m2));
        acc[(2 * NP + u) * 8 + j] += de_val(o.e[j]);
      }
      de_store(ds + row * H + col[u], o);
    }
  }
  // a lane's slots: 3 * NP * 8 consecutive floats of the strip
  de_combine<3 * NP * 8>(strip, acc, lane * (3 * NP * 8), wave);
  if (wave == DE_WAVES - 1) {
    float* dst = part + ((int64_t)c * gridDim.x + blockIdx.x) * 3 * H;
#pragma unroll
    for (int k = 0; k < 3; ++k)
#pragma unroll
      for (int u = 0; u < NP; ++u) {
        if (!ok[u]) continue;
        const float* a = acc + (k * NP + u) * 8;
#pragma unroll
        for (int q = 0; q < 2; ++q)
          *reinterpret_cast<DeFloat4*>(dst + (int64_t)k * H + col[u] + 4 * q) =
              DeFloat4{{a[4 * q], a[4 * q + 1], a[4 * q + 2], a[4 * q + 3]}};
      }
  }
}

// out[k, c, :] = bf16(sum over rb, in index order, of part[c, rb, k, :]); a
// thread takes four columns.  W % 4 == 0.
__global__ __launch_bounds__(DE_THREADS) void k_colsum_finish(
    const float* __restrict__ part, unsigned short* __restrict__ out, int C,
    int row_blocks, int K, int W) {
  const int wq = W / 4;
  const int64_t idx = (int64_t)blockIdx.x * DE_THREADS + threadIdx.x;
  if (idx >= (int64_t)C * K * wq) return;
  const int q = (int)(idx % wq);
  const int ck = (int)(idx / wq);
  const int k = ck % K, c = ck / K;
  float sum[4] = {0.f, 0.f, 0.f, 0.f};
  for (int rb = 0; rb < row_blocks; ++rb) {
    const DeFloat4 v = *reinterpret_cast<const DeFloat4*>(
        part + (((int64_t)c * row_blocks + rb) * K + k) * W + 4 * q);
#pragma unroll
    for (int j = 0; j < 4; ++j) sum[j] += v.v[j];
  }
  DeHalfPack o;
#pragma unroll
  for (int j = 0; j < 4; ++j) o.e[j] = de_bits(sum[j]);
  *reinterpret_cast<DeHalfPack*>(out + ((int64_t)k * C + c) * W + 4 * q) = o;
}

#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute pop
#endif

// ---------------------------------------------------------------------------
extern "C" const char* ols_dense_epi_route(int64_t width, int is_bf16,
                                           int aligned, int layernorm) {
  return dense_epi_route_name(
      dense_epi_route(width, is_bf16 != 0, aligned != 0, layernorm != 0));
}

static bool de_aligned(std::initializer_list<const void*> ptrs) {
  for (const void* p : ptrs)
    if (p == nullptr || reinterpret_cast<uintptr_t>(p) % 16 != 0) return false;
  return true;
}

// what the kernels' index arithmetic and grids hold
static bool de_sizes_ok(int C, int N, int row_block) {
  return C >= 1 && C <= 65535 && N >= 1 && row_block >= 1;
}

static int de_row_blocks(int N, int row_block) {
  return (N + row_block - 1) / row_block;
}

extern "C" int ols_dense_epi_row_blocks(int N, int row_block) {
  return N >= 1 && row_block >= 1 ? de_row_blocks(N, row_block) : 0;
}

extern "C" int ols_bias_gelu_fwd(const void* z, const void* b, void* y, int C,
                                 int N, int F, int row_block,
                                 hipStream_t stream) {
  if (dense_epi_route(F, true, de_aligned({z, b, y}), false) ==
          DENSE_EPI_TORCH ||
      !de_sizes_ok(C, N, row_block) || de_row_blocks(N, row_block) > 65535)
    return 1;
  hipLaunchKernelGGL(
      k_bias_gelu_fwd,
      dim3((F + DE_CHUNK - 1) / DE_CHUNK, de_row_blocks(N, row_block), C),
      dim3(DE_THREADS), 0, stream, (const unsigned short*)z,
      (const unsigned short*)b, (unsigned short*)y, N, F, row_block);
  return 0;
}

extern "C" int ols_bias_gelu_bwd(const void* z, const void* b, const void* dy,
                                 void* dz, float* part, int C, int N, int F,
                                 int row_block, hipStream_t stream) {
  if (dense_epi_route(F, true, de_aligned({z, b, dy, dz, part}), false) ==
          DENSE_EPI_TORCH ||
      !de_sizes_ok(C, N, row_block) || de_row_blocks(N, row_block) > 65535)
    return 1;
  hipLaunchKernelGGL(
      k_bias_gelu_bwd,
      dim3((F + DE_CHUNK - 1) / DE_CHUNK, de_row_blocks(N, row_block), C),
      dim3(DE_THREADS), 0, stream, (const unsigned short*)z,
      (const unsigned short*)b, (const unsigned short*)dy,
      (unsigned short*)dz, part, N, F, row_block);
  return 0;
}

#define DE_LAUNCH_LN_FWD(NP)                                                 \
  hipLaunchKernelGGL(k_brln_fwd<NP>,                                         \
                     dim3(de_row_blocks(N, DE_LN_FWD_ROWS), C),              \
                     dim3(DE_THREADS), 0, stream, (const unsigned short*)z,  \
                     (const unsigned short*)b, (const unsigned short*)res,   \
                     (const unsigned short*)gamma,                           \
                     (const unsigned short*)beta, (unsigned short*)y,        \
                     (unsigned short*)s, mean, rstd, N, H, eps)

extern "C" int ols_brln_fwd(const void* z, const void* b, const void* res,
                            const void* gamma, const void* beta, void* y,
                            void* s, float* mean, float* rstd, int C, int N,
                            int H, float eps, hipStream_t stream) {
  if (dense_epi_route(H, true, de_aligned({z, b, res, gamma, beta, y, s}),
                      true) == DENSE_EPI_TORCH ||
      !de_sizes_ok(C, N, 1) || mean == nullptr || rstd == nullptr)
    return 1;
  if (H <= 512) DE_LAUNCH_LN_FWD(1);
  else if (H <= 1024) DE_LAUNCH_LN_FWD(2);
  else DE_LAUNCH_LN_FWD(3);
  return 0;
}

#define DE_LAUNCH_LN_BWD(NP)                                                 \
  hipLaunchKernelGGL(k_brln_bwd<NP>, dim3(de_row_blocks(N, row_block), C),   \
                     dim3(DE_THREADS), 0, stream, (const unsigned short*)s,  \
                     (const unsigned short*)dy, (const unsigned short*)gamma, \
                     mean, rstd, (unsigned short*)ds, part, N, H, row_block)

extern "C" int ols_brln_bwd(const void* s, const void* dy, const void* gamma,
                            const float* mean, const float* rstd, void* ds,
                            float* part, int C, int N, int H, int row_block,
                            hipStream_t stream) {
  if (dense_epi_route(H, true, de_aligned({s, dy, gamma, ds, part}), true) ==
          DENSE_EPI_TORCH ||
      !de_sizes_ok(C, N, row_block) || mean == nullptr || rstd == nullptr)
    return 1;
  if (H <= 512) DE_LAUNCH_LN_BWD(1);
  else if (H <= 1024) DE_LAUNCH_LN_BWD(2);
  else DE_LAUNCH_LN_BWD(3);
  return 0;
}

extern "C" int ols_colsum_finish(const float* part, void* out, int C,
                                 int row_blocks, int K, int W,
                                 hipStream_t stream) {
  if (!de_aligned({part, out}) || C < 1 || row_blocks < 1 || K < 1 ||
      W < 8 || W % 8 != 0)
    return 1;
  const int64_t threads = (int64_t)C * K * (W / 4);
  hipLaunchKernelGGL(k_colsum_finish,
                     dim3((unsigned)((threads + DE_THREADS - 1) / DE_THREADS)),
                     dim3(DE_THREADS), 0, stream, part, (unsigned short*)out,
                     C, row_blocks, K, W);
  return 0;
}
