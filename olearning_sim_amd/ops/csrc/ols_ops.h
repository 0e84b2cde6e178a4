// Every extern "C" launcher of the extension, declared once.  Included by
// bindings.cpp and by each .hip file that defines one, so an argument
// list that drifts between the two fails to compile as a conflicting
// C-linkage declaration, where it used to link and run with garbage.
#pragma once

#include <hip/hip_runtime.h>
#include <cstdint>

// Largest ch/G (channels per normalisation group): the GroupNorm backward
// kernels keep per-channel dgamma/dbeta partials in LDS arrays of this
// length, and the torch wrappers refuse anything larger.
#define MAX_CG 128

extern "C" void ols_fused_sgd_update_flat(
    void* buf, const void* grad, const void* master, const int64_t* offs,
    int nblocks, int64_t clients, int64_t total, float lr, float mu,
    int dtype, hipStream_t stream);

extern "C" void ols_weighted_delta_accum_flat(
    float* delta, const void* buf, const void* master, const float* weights,
    const int64_t* offs, int nblocks, int64_t clients, int64_t pglobal,
    float wsum, const float* wsum_dev, int dtype, hipStream_t stream);

// "cpar_s", "cpar", "v8" or "block_table": the kernel that launch runs for
// nblocks blocks of n master elements in all (delta_route.h), given
// whether master and buf start on 16-byte boundaries
extern "C" const char* ols_delta_accum_route(int nblocks, int64_t n,
                                             int64_t clients, int dtype,
                                             int master_16b, int buf_16b);

// clip.hip: per-client squared update norm and clipped aggregation weights
extern "C" int ols_sqnorm_tiles(int64_t n, int64_t clients, int vec);
extern "C" void ols_client_delta_sqnorm(float* sq, float* part,
                                        const void* buf, const void* master,
                                        int64_t clients, int64_t n, int vec,
                                        int dtype, hipStream_t stream);
extern "C" void ols_clip_weights(const float* sq, const float* weights,
                                 float* w_eff, float* wsum_eff,
                                 int64_t clients, float clip,
                                 hipStream_t stream);

// uplink_quant.hip: delta[q] += sum_c weights[c] * Q_bits(buf[c,q] -
// master[q]) over one parameter tensor of n elements, Q the stochastic
// bucketed quantiser with 2^(bits-1) - 1 levels per sign (bits 2, 4 or
// 8).  cids: the clients' ids, elem_base: the tensor's offset in the flat
// master; with the key (k0, k1) they index the uniform draws, and every
// cid and (elem_base + n) / 2 must be below 2^32.
extern "C" void ols_delta_accum_quant(float* delta, const void* buf,
                                      const void* master,
                                      const float* weights,
                                      const int64_t* cids, int64_t clients,
                                      int64_t n, int64_t elem_base, int bits,
                                      uint32_t k0, uint32_t k1, int dtype,
                                      hipStream_t stream);
// "v8" or "scalar": the kernel that launch runs (uplink_route.h), given
// whether master and buf start on 16-byte boundaries
extern "C" const char* ols_delta_accum_quant_route(int64_t n, int64_t clients,
                                                   int dtype, int master_16b,
                                                   int buf_16b);

// server_opt.hip: one server optimiser step over the flat fp32 master.
// kind 0 momentum, 1 adagrad, 2 adam, 3 yogi (server_opt_route.h);
// x, m, v in place, v unused (may be null) for momentum, z null for no
// noise: g = d*inv_w + sigma*z
extern "C" void ols_server_opt_step(int kind, float* x, const float* d,
                                    float* m, float* v, const float* z,
                                    int64_t n, float inv_w, float sigma,
                                    float lr, float b1, float b2, float tau,
                                    hipStream_t stream);
// "v4" or "scalar": the kernel that step runs for n elements, given
// whether every operand starts on a 16-byte boundary
extern "C" const char* ols_server_opt_route(int64_t n, int aligned);

extern "C" void ols_cross_entropy_fwd_bwd(
    const void* logits, const int64_t* labels, float* loss, void* dlogits,
    int64_t nrows, int64_t K, float inv_n, int dtype, hipStream_t stream);

extern "C" void ols_groupnorm_fwd(const void* x, const void* res, void* y,
                                  float* mean, float* rstd, const void* gamma,
                                  const void* beta, int B, int C, int ch,
                                  int G, int HW, float eps, bool relu,
                                  int layout, int dtype, hipStream_t stream);

extern "C" void ols_mfma_selftest(const void* A, const void* B, float* D,
                                  hipStream_t stream);

extern "C" void ols_conv3x3_fwd(const void* x, const void* w, void* y, int C,
                                int IC, int OC, int B, int H, int W,
                                int stride, hipStream_t stream);
extern "C" void ols_conv3x3_dgrad(const void* dy, const void* w, void* dx,
                                  int C, int IC, int OC, int B, int H, int W,
                                  int stride, hipStream_t stream);
extern "C" void ols_conv3x3_wgrad(const void* x, const void* dy, void* dw,
                                  int C, int IC, int OC, int B, int H, int W,
                                  int stride, hipStream_t stream);

extern "C" int ols_conv3x3_v6_ok(int IC, int OC, int B, int H, int W,
                                 int stride);
// dir: 0 fwd, 1 dgrad, 2 wgrad; the kernel's name with its template
// arguments (conv3_route.h), family decision included
extern "C" const char* ols_conv3x3_route(int dir, int IC, int OC, int B,
                                         int H, int W, int stride);
// "kmajor" or "nmajor": the B-tile staging of the kernel that route runs
extern "C" const char* ols_conv3x3_staging(int dir, int IC, int OC, int B,
                                           int H, int W, int stride);
// "64x128" or "128x64": the block tile of the kernel that route runs
extern "C" const char* ols_conv3x3_tile(int dir, int IC, int OC, int B,
                                        int H, int W, int stride);
extern "C" void ols_conv3x3_fwd_p(const void* xp, const void* w, void* y,
                                  int C, int IC, int OC, int B, int H, int W,
                                  int stride, hipStream_t stream);
extern "C" void ols_conv3x3_dgrad_p(const void* dyp, const void* w, void* dx,
                                    int C, int IC, int OC, int B, int H,
                                    int W, int stride, hipStream_t stream);
extern "C" void ols_conv3x3_wgrad_p(const void* xp, const void* dy, void* dw,
                                    int C, int IC, int OC, int B, int H,
                                    int W, int stride, hipStream_t stream);

// w [C, OC, IC, 3, 3] -> wt [C, IC, OC, 3, 3], taps reversed: the forward
// weight of the stride-1 dgrad (conv3_wflip.hip).  OC, IC multiples of 32.
extern "C" void ols_conv3_wflip(const void* w, void* wt, int C, int OC,
                                int IC, hipStream_t stream);
// w -= lr * g in place and wt <- wflip(updated w), one pass
extern "C" void ols_sgd_conv3_wt(void* w, const void* g, void* wt, int C,
                                 int OC, int IC, float lr,
                                 hipStream_t stream);

extern "C" void ols_conv5x5_fwd(const void* x, const void* w, const void* b,
                                void* y, const int* ntab, int C, int IC,
                                int OC, int B, int H, int W, int relu,
                                hipStream_t stream);
extern "C" void ols_conv5x5_dgrad(const void* dyp, const void* w, void* dx,
                                  const int* ntab, int C, int IC, int OC,
                                  int B, int H, int W, hipStream_t stream);
extern "C" int ols_conv5x5_route(int dir, int IC, int OC, int H, int W);
extern "C" void ols_conv5x5_wgrad(const void* x, const void* dy, void* dw,
                                  const int* ntab, int C, int IC, int OC,
                                  int B, int H, int W, hipStream_t stream);

extern "C" void ols_pool2x2_fwd(const void* x, void* y, unsigned char* arg,
                                int64_t planes, int OH, int OW, int dtype,
                                hipStream_t stream);
extern "C" void ols_pool2x2_bwd(const void* dy, const unsigned char* arg,
                                void* dx, int64_t planes, int OH, int OW,
                                int dtype, hipStream_t stream);

extern "C" void ols_subsample2_fwd(const void* x, void* y, int64_t planes,
                                   int OH, int OW, int dtype,
                                   hipStream_t stream);
extern "C" void ols_subsample2_bwd(const void* dy, void* dx, int64_t planes,
                                   int H, int W, int dtype,
                                   hipStream_t stream);

extern "C" void ols_transpose2d(const void* in, void* out, int64_t B, int M,
                                int N, int dtype, hipStream_t stream);

extern "C" void ols_pad2d(const void* in, void* out, int64_t planes, int H,
                          int W, int pad, int dtype, hipStream_t stream);

extern "C" void ols_replicate(const void* src, void* dst, int64_t clients,
                              int64_t n, int dtype, hipStream_t stream);

extern "C" void ols_synth_batch(const float* x, const int64_t* y, void* out,
                                int64_t rows, int64_t batch, int64_t n,
                                float s, float t, hipStream_t stream);

extern "C" void ols_relu_mask(const void* dy, const void* y, void* out,
                              int64_t n, int dtype, hipStream_t stream);

extern "C" void ols_layernorm_fwd(const void* x, const void* gamma,
                                  const void* beta, void* y, float* mean,
                                  float* rstd, int64_t rows, int H,
                                  int64_t rows_per_client, float eps,
                                  int dtype, hipStream_t stream);
extern "C" void ols_layernorm_bwd(const void* x, const void* dy,
                                  const void* gamma, const float* mean,
                                  const float* rstd, void* dx, float* dgamma,
                                  float* dbeta, int64_t rows, int H,
                                  int64_t rows_per_client, int dtype,
                                  hipStream_t stream);

extern "C" void ols_groupnorm_bwd(const void* x, const void* y,
                                  const void* dy, void* dx, void* dres,
                                  const float* mean, const float* rstd,
                                  const void* gamma, float* dgamma,
                                  float* dbeta, int B, int C, int ch, int G,
                                  int HW, bool relu, int layout, int dtype,
                                  hipStream_t stream);

extern "C" int ols_gn_pad_ok(int ch, int G, int H, int W);
extern "C" void ols_groupnorm_fwd_pad(
    const void* x, const void* res, int res_mode, void* y, uint32_t* mask,
    float* mean, float* rstd, const void* gamma, const void* beta, int B,
    int C, int ch, int G, int H, int W, float eps, bool pad_out,
    hipStream_t stream);
extern "C" void ols_groupnorm_bwd_pad(
    const void* x, const uint32_t* mask, const void* dy, void* dx,
    void* dx_pad, void* dres, const float* mean, const float* rstd,
    const void* gamma, float* dgamma, float* dbeta, int B, int C, int ch,
    int G, int H, int W, hipStream_t stream);
extern "C" void ols_subsample2p_fwd(const void* xp, void* y, int64_t planes,
                                    int OH, int OW, int dtype,
                                    hipStream_t stream);
