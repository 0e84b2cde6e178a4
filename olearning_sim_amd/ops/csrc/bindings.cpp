// Torch bindings for the olearning_sim_amd gfx950 kernels.
// Registered as torch.ops.olsim_hip.* (loaded from the in-tree .so by
// olearning_sim_amd/ops/fused.py).

#include <torch/extension.h>
#include <ATen/cuda/CUDAContext.h>
#include <hip/hip_runtime.h>

#include "ols_ops.h"

namespace {

int dtype_code(const at::Tensor& t) {
  switch (t.scalar_type()) {
    case at::kFloat: return 0;
    case at::kBFloat16: return 1;
    case at::kHalf: return 2;
    default:
      TORCH_CHECK(false, "olsim_hip: unsupported dtype ", t.scalar_type());
  }
}

void fused_sgd_update_flat(at::Tensor buf, at::Tensor grad,
                           at::Tensor global_flat, at::Tensor offsets,
                           int64_t clients, double lr, double mu) {
  TORCH_CHECK(buf.is_cuda() && buf.is_contiguous(), "buf must be GPU+contig");
  TORCH_CHECK(grad.sizes() == buf.sizes() && grad.scalar_type() == buf.scalar_type());
  const bool prox = mu != 0.0 && global_flat.numel() > 0;
  if (prox) {
    TORCH_CHECK(offsets.numel() >= 2 && offsets.scalar_type() == at::kLong);
    TORCH_CHECK(global_flat.scalar_type() == buf.scalar_type());
  }
  auto stream = at::cuda::getCurrentCUDAStream();
  ols_fused_sgd_update_flat(
      buf.data_ptr(), grad.data_ptr(),
      prox ? global_flat.data_ptr() : nullptr,
      prox ? offsets.data_ptr<int64_t>() : nullptr,
      prox ? (int)(offsets.numel() - 1) : 0, clients, buf.numel(),
      (float)lr, (float)mu, dtype_code(buf), stream.stream());
}

// wsum_dev: null, or one float on the device that replaces wsum
void delta_accum_impl(at::Tensor& delta, at::Tensor& buf,
                      at::Tensor& global_flat, at::Tensor& weights,
                      at::Tensor& offsets, int64_t clients, double wsum,
                      const float* wsum_dev) {
  TORCH_CHECK(delta.is_cuda() && delta.scalar_type() == at::kFloat &&
              delta.is_contiguous());
  TORCH_CHECK(buf.is_contiguous() && global_flat.is_contiguous());
  TORCH_CHECK(buf.scalar_type() == global_flat.scalar_type());
  TORCH_CHECK(weights.scalar_type() == at::kFloat && weights.numel() == clients);
  TORCH_CHECK(offsets.scalar_type() == at::kLong && offsets.numel() >= 2);
  TORCH_CHECK(buf.numel() == clients * global_flat.numel());
  auto stream = at::cuda::getCurrentCUDAStream();
  ols_weighted_delta_accum_flat(
      delta.data_ptr<float>(), buf.data_ptr(), global_flat.data_ptr(),
      weights.data_ptr<float>(), offsets.data_ptr<int64_t>(),
      (int)(offsets.numel() - 1), clients, global_flat.numel(), (float)wsum,
      wsum_dev, dtype_code(buf), stream.stream());
}

void weighted_delta_accum_flat(at::Tensor delta, at::Tensor buf,
                               at::Tensor global_flat, at::Tensor weights,
                               at::Tensor offsets, int64_t clients,
                               double wsum) {
  delta_accum_impl(delta, buf, global_flat, weights, offsets, clients, wsum,
                   nullptr);
}

// the same reduction with sum_c w_c read from the device (clip_weights'
// wsum_eff): no host round trip between the two
void weighted_delta_accum_flat_dw(at::Tensor delta, at::Tensor buf,
                                  at::Tensor global_flat, at::Tensor weights,
                                  at::Tensor offsets, int64_t clients,
                                  at::Tensor wsum) {
  TORCH_CHECK(wsum.is_cuda() && wsum.device() == delta.device() &&
                  wsum.scalar_type() == at::kFloat && wsum.numel() == 1,
              "weighted_delta_accum_flat_dw: wsum must be one fp32 on the "
              "GPU of delta");
  TORCH_CHECK(weights.is_cuda() && weights.is_contiguous());
  delta_accum_impl(delta, buf, global_flat, weights, offsets, clients, 0.0,
                   wsum.data_ptr<float>());
}

// The kernel one accumulate launch runs: "cpar_s", "cpar", "v8" or
// "block_table".  dtype 0 fp32, 1 bf16, 2 fp16; the two flags say whether
// master and buf start on a 16-byte boundary.  Same host function the
// launcher switches on (delta_route.h), which reads the flags off the
// pointers it is given.
std::string delta_accum_route(int64_t nblocks, int64_t n, int64_t clients,
                              int64_t dtype, bool master_aligned,
                              bool buf_aligned) {
  TORCH_CHECK(nblocks >= 1 && n >= 0 && clients >= 1 && dtype >= 0 &&
                  dtype <= 2,
              "delta_accum_route: nblocks >= 1, clients >= 1, dtype 0..2");
  return ols_delta_accum_route((int)nblocks, n, clients, (int)dtype,
                               master_aligned, buf_aligned);
}

// ---- per-client update clipping (clip.hip) ------------------------------

// 16 / itemsize when every row of buf [clients, n] and master start on a
// 16-byte boundary and n is a whole number of 16-byte packs, else 1
int sqnorm_vec(const at::Tensor& buf, const at::Tensor& master, int64_t n) {
  const int v = 16 / (int)buf.element_size();
  const bool aligned =
      n % v == 0 &&
      reinterpret_cast<uintptr_t>(buf.data_ptr()) % 16 == 0 &&
      reinterpret_cast<uintptr_t>(master.data_ptr()) % 16 == 0;
  return aligned ? v : 1;
}

// sq[c] += sum_j (f32(buf[c,j]) - f32(master[j]))^2, deterministic
void client_delta_sqnorm(at::Tensor sq, at::Tensor buf, at::Tensor master,
                         int64_t clients) {
  TORCH_CHECK(sq.is_cuda() && sq.scalar_type() == at::kFloat &&
                  sq.is_contiguous() && sq.numel() == clients,
              "client_delta_sqnorm: sq must be contiguous fp32 [clients] on "
              "the GPU");
  TORCH_CHECK(buf.is_cuda() && master.is_cuda() &&
                  buf.device() == sq.device() &&
                  master.device() == sq.device() && buf.is_contiguous() &&
                  master.is_contiguous() &&
                  buf.scalar_type() == master.scalar_type(),
              "client_delta_sqnorm: buf and master must be contiguous, of "
              "one dtype, on the GPU of sq");
  // clients is the grid's y dimension
  TORCH_CHECK(clients >= 1 && clients <= 65535,
              "client_delta_sqnorm: clients ", clients, " outside 1..65535");
  const int64_t n = master.numel();
  TORCH_CHECK(buf.numel() == clients * n, "client_delta_sqnorm: buf has ",
              buf.numel(), " elements, expected ", clients, " x ", n);
  const int dt = dtype_code(buf);
  if (n == 0) return;
  const int vec = sqnorm_vec(buf, master, n);
  const int tiles = ols_sqnorm_tiles(n, clients, vec);
  at::Tensor part;
  if (tiles > 1) part = at::empty({clients * tiles}, sq.options());
  ols_client_delta_sqnorm(sq.data_ptr<float>(),
                          tiles > 1 ? part.data_ptr<float>() : nullptr,
                          buf.data_ptr(), master.data_ptr(), clients, n, vec,
                          dt, at::cuda::getCurrentCUDAStream().stream());
}

// tiles one client's row of n elements is split over (vec: 1 for the
// scalar path, 16 / itemsize for the vector path)
int64_t sqnorm_tiles(int64_t n, int64_t clients, int64_t vec) {
  TORCH_CHECK(n >= 1 && clients >= 1 && vec >= 1);
  return ols_sqnorm_tiles(n, clients, (int)vec);
}

std::tuple<at::Tensor, at::Tensor> clip_weights(at::Tensor sq,
                                                at::Tensor weights,
                                                double clip_norm) {
  TORCH_CHECK(sq.is_cuda() && weights.is_cuda() &&
                  sq.device() == weights.device() &&
                  sq.scalar_type() == at::kFloat &&
                  weights.scalar_type() == at::kFloat &&
                  sq.is_contiguous() && weights.is_contiguous() &&
                  sq.dim() == 1 && sq.sizes() == weights.sizes(),
              "clip_weights: sq and weights must be contiguous fp32 [C] on "
              "one GPU");
  TORCH_CHECK(clip_norm > 0.0, "clip_weights: clip_norm must be positive");
  auto w_eff = at::empty_like(weights);
  auto wsum_eff = at::empty({1}, weights.options());
  ols_clip_weights(sq.data_ptr<float>(), weights.data_ptr<float>(),
                   w_eff.data_ptr<float>(), wsum_eff.data_ptr<float>(),
                   sq.numel(), (float)clip_norm,
                   at::cuda::getCurrentCUDAStream().stream());
  return {w_eff, wsum_eff};
}

// ---- uplink compression (uplink_quant.hip) ------------------------------

// delta[q] += sum_c weights[c] * Q(buf[c,q] - master[q]) for one parameter
// tensor: Q quantises each client's update to `bits` bits per weight,
// stochastically and per bucket of 512 elements.  client_ids [clients]
// int64 and elem_base (the tensor's offset in the flat master) index the
// uniform draws of key (k0, k1).  The ids' range is checked here, which
// reads them back (a device sync), unless the caller has checked it:
// fused.weighted_delta_accum_quant does so once for all its launches.
void delta_accum_quant(at::Tensor delta, at::Tensor buf, at::Tensor master,
                       at::Tensor weights, at::Tensor client_ids,
                       int64_t clients, int64_t bits, int64_t k0, int64_t k1,
                       int64_t elem_base, bool ids_checked) {
  TORCH_CHECK(bits == 2 || bits == 4 || bits == 8,
              "delta_accum_quant: bits ", bits, " not one of 2, 4, 8");
  TORCH_CHECK(delta.is_cuda() && delta.scalar_type() == at::kFloat &&
                  delta.is_contiguous(),
              "delta_accum_quant: delta must be contiguous fp32 on the GPU");
  TORCH_CHECK(buf.is_cuda() && master.is_cuda() &&
                  buf.device() == delta.device() &&
                  master.device() == delta.device() && buf.is_contiguous() &&
                  master.is_contiguous() &&
                  buf.scalar_type() == master.scalar_type(),
              "delta_accum_quant: buf and master must be contiguous, of one "
              "dtype, on the GPU of delta");
  // client tiles of 64 are the grid's y dimension
  TORCH_CHECK(clients >= 1 && clients <= 65535 * 64,
              "delta_accum_quant: clients ", clients, " outside 1..",
              65535 * 64);
  TORCH_CHECK(weights.is_cuda() && weights.device() == delta.device() &&
                  weights.scalar_type() == at::kFloat &&
                  weights.is_contiguous() && weights.numel() == clients,
              "delta_accum_quant: weights must be contiguous fp32 [clients] "
              "on the GPU of delta");
  TORCH_CHECK(client_ids.is_cuda() && client_ids.device() == delta.device() &&
                  client_ids.scalar_type() == at::kLong &&
                  client_ids.is_contiguous() &&
                  client_ids.numel() == clients,
              "delta_accum_quant: client_ids must be contiguous int64 "
              "[clients] on the GPU of delta");
  const int64_t n = master.numel();
  TORCH_CHECK(delta.numel() == n, "delta_accum_quant: delta has ",
              delta.numel(), " elements, master ", n);
  TORCH_CHECK(buf.numel() == clients * n, "delta_accum_quant: buf has ",
              buf.numel(), " elements, expected ", clients, " x ", n);
  const int64_t lim = (int64_t)1 << 32;
  TORCH_CHECK(k0 >= 0 && k0 < lim && k1 >= 0 && k1 < lim,
              "delta_accum_quant: k0 and k1 must be 32-bit words");
  // the pair index (elem_base + q) / 2 is hashed as a 32-bit word
  TORCH_CHECK(elem_base >= 0 && elem_base <= 2 * lim - n,
              "delta_accum_quant: elem_base ", elem_base, " + n ", n,
              " outside 0..2^33");
  TORCH_CHECK(buf.scalar_type() == at::kFloat ||
                  buf.scalar_type() == at::kBFloat16 ||
                  buf.scalar_type() == at::kHalf,
              "delta_accum_quant: buf must be fp32, bf16 or fp16, got ",
              buf.scalar_type());
  const int dt = dtype_code(buf);
  if (!ids_checked) {
    const auto [lo, hi] = at::aminmax(client_ids);
    TORCH_CHECK(lo.item<int64_t>() >= 0 && hi.item<int64_t>() < lim,
                "delta_accum_quant: client ids must lie in 0..2^32-1");
  }
  if (n == 0) return;
  ols_delta_accum_quant(delta.data_ptr<float>(), buf.data_ptr(),
                        master.data_ptr(), weights.data_ptr<float>(),
                        client_ids.data_ptr<int64_t>(), clients, n, elem_base,
                        (int)bits, (uint32_t)k0, (uint32_t)k1, dt,
                        at::cuda::getCurrentCUDAStream().stream());
}

// "v8" or "scalar": the kernel one quantised accumulate over n elements
// runs.  dtype 0 fp32, 1 bf16, 2 fp16; the two flags say whether master
// and buf start on a 16-byte boundary.  Same host function the launcher
// switches on (uplink_route.h).
std::string delta_accum_quant_route(int64_t n, int64_t clients, int64_t dtype,
                                    bool master_aligned, bool buf_aligned) {
  TORCH_CHECK(n >= 0 && clients >= 1 && dtype >= 0 && dtype <= 2,
              "delta_accum_quant_route: n >= 0, clients >= 1, dtype 0..2");
  return ols_delta_accum_quant_route(n, clients, (int)dtype, master_aligned,
                                     buf_aligned);
}

// ---- server optimiser step (server_opt.hip) ------------------------------
// kind 0 momentum, 1 adagrad, 2 adam, 3 yogi.  x (master), m and v are
// updated in place; momentum has no v and takes an empty one.  z is the
// round's noise or None: g = d / total_weight + sigma * z.

void server_opt_step(int64_t kind, at::Tensor x, at::Tensor d, at::Tensor m,
                     at::Tensor v, const c10::optional<at::Tensor>& z,
                     double total_weight, double sigma, double lr,
                     double beta1, double beta2, double tau) {
  TORCH_CHECK(kind >= 0 && kind <= 3, "server_opt_step: kind ", kind,
              " outside 0..3 (momentum, adagrad, adam, yogi)");
  TORCH_CHECK(total_weight > 0.0,
              "server_opt_step: total_weight must be positive, got ",
              total_weight);
  TORCH_CHECK(x.is_cuda(), "server_opt_step: x must be on the GPU");
  const bool has_z = z.has_value() && z->defined();
  auto check = [&](const at::Tensor& t, const char* name) {
    TORCH_CHECK(t.is_cuda() && t.device() == x.device() &&
                    t.scalar_type() == at::kFloat && t.is_contiguous(),
                "server_opt_step: ", name,
                " must be contiguous fp32 on the GPU of x");
  };
  check(x, "x");
  check(d, "d");
  check(m, "m");
  check(v, "v");
  if (has_z) check(*z, "z");
  const int64_t n = x.numel();
  TORCH_CHECK(d.numel() == n && m.numel() == n &&
                  (!has_z || z->numel() == n),
              "server_opt_step: x, d, m and z must have one numel, got ", n,
              ", ", d.numel(), ", ", m.numel(), ", ",
              has_z ? z->numel() : n);
  TORCH_CHECK(v.numel() == n || (kind == 0 && v.numel() == 0),
              "server_opt_step: v has ", v.numel(), " elements, expected ",
              n, kind == 0 ? " or none" : "");
  if (n == 0) return;
  ols_server_opt_step((int)kind, x.data_ptr<float>(), d.data_ptr<float>(),
                      m.data_ptr<float>(),
                      kind == 0 ? nullptr : v.data_ptr<float>(),
                      has_z ? z->data_ptr<float>() : nullptr, n,
                      (float)(1.0 / total_weight), (float)sigma, (float)lr,
                      (float)beta1, (float)beta2, (float)tau,
                      at::cuda::getCurrentCUDAStream().stream());
}

// "v4" or "scalar": the kernel a step over n elements runs, given whether
// every operand starts on a 16-byte boundary.  Same host function the
// launcher switches on (server_opt_route.h), which reads the flag off the
// pointers it is given.
std::string server_opt_route(int64_t n, bool aligned) {
  TORCH_CHECK(n >= 0, "server_opt_route: n >= 0");
  return ols_server_opt_route(n, aligned);
}

std::tuple<at::Tensor, at::Tensor> cross_entropy_fwd_bwd(at::Tensor logits,
                                                         at::Tensor labels) {
  TORCH_CHECK(logits.is_cuda() && logits.dim() == 2 && logits.is_contiguous());
  TORCH_CHECK(labels.scalar_type() == at::kLong &&
              labels.numel() == logits.size(0));
  int64_t n = logits.size(0), k = logits.size(1);
  auto loss = at::empty({n}, logits.options().dtype(at::kFloat));
  auto dlogits = at::empty_like(logits);
  auto stream = at::cuda::getCurrentCUDAStream();
  ols_cross_entropy_fwd_bwd(
      logits.data_ptr(), labels.contiguous().data_ptr<int64_t>(),
      loss.data_ptr<float>(), dlogits.data_ptr(), n, k, 1.0f / (float)n,
      dtype_code(logits), stream.stream());
  return {loss, dlogits};
}

int gn_dtype(const at::Tensor& t) {
  TORCH_CHECK(t.scalar_type() == at::kFloat || t.scalar_type() == at::kBFloat16,
              "groupnorm: f32/bf16 only");
  return t.scalar_type() == at::kFloat ? 0 : 1;
}

// Shape of a GroupNorm input, for all four wrappers.  4-D x is
// [B, C*ch, H, W] (layout 0), 5-D x is [C, ch, B, H, W] (layout 1);
// ngroups = B*C*G workgroups of n = (ch/G)*H*W elements each.
struct GnDims {
  int layout;
  int64_t B, ch, H, W, HW, ngroups, n;
};

GnDims gn_dims(const at::Tensor& x, int64_t clients, int64_t groups) {
  TORCH_CHECK(x.is_cuda() && x.is_contiguous() &&
                  (x.dim() == 4 || x.dim() == 5),
              "groupnorm: x must be a contiguous 4-D or 5-D device tensor");
  TORCH_CHECK(clients > 0 && groups > 0);
  GnDims d;
  d.layout = x.dim() == 4 ? 0 : 1;
  if (d.layout == 0) {
    TORCH_CHECK(x.size(1) % clients == 0);
    d.B = x.size(0); d.ch = x.size(1) / clients;
  } else {
    TORCH_CHECK(x.size(0) == clients);
    d.ch = x.size(1); d.B = x.size(2);
  }
  d.H = x.size(-2); d.W = x.size(-1); d.HW = d.H * d.W;
  TORCH_CHECK(d.ch % groups == 0);
  TORCH_CHECK(d.ch / groups <= MAX_CG, "groupnorm: ch/G > ", MAX_CG,
              " unsupported");
  d.ngroups = d.B * clients * groups;
  d.n = (d.ch / groups) * d.HW;
  return d;
}

std::tuple<at::Tensor, at::Tensor, at::Tensor> groupnorm_fwd(
    at::Tensor x, at::Tensor res, at::Tensor gamma, at::Tensor beta,
    int64_t clients, int64_t groups, double eps, bool relu) {
  const GnDims d = gn_dims(x, clients, groups);
  TORCH_CHECK(gamma.is_contiguous() && beta.is_contiguous());
  const bool has_res = res.numel() > 0;
  if (has_res) TORCH_CHECK(res.is_contiguous() && res.sizes() == x.sizes());
  auto y = at::empty_like(x);
  auto mean = at::empty({d.ngroups}, x.options().dtype(at::kFloat));
  auto rstd = at::empty({d.ngroups}, x.options().dtype(at::kFloat));
  auto stream = at::cuda::getCurrentCUDAStream();
  ols_groupnorm_fwd(x.data_ptr(), has_res ? res.data_ptr() : nullptr,
                    y.data_ptr(), mean.data_ptr<float>(),
                    rstd.data_ptr<float>(), gamma.data_ptr(), beta.data_ptr(),
                    (int)d.B, (int)clients, (int)d.ch, (int)groups,
                    (int)d.HW, (float)eps, relu, d.layout, gn_dtype(x),
                    stream.stream());
  return {y, mean, rstd};
}

std::tuple<at::Tensor, at::Tensor, at::Tensor, at::Tensor> groupnorm_bwd(
    at::Tensor x, at::Tensor y, at::Tensor dy, at::Tensor mean,
    at::Tensor rstd, at::Tensor gamma, int64_t clients, int64_t groups,
    bool has_res, bool relu) {
  const GnDims d = gn_dims(x, clients, groups);
  TORCH_CHECK(y.is_contiguous() && y.sizes() == x.sizes() &&
              y.scalar_type() == x.scalar_type());
  TORCH_CHECK(dy.sizes() == x.sizes() &&
              dy.scalar_type() == x.scalar_type());
  TORCH_CHECK(mean.numel() == d.ngroups && rstd.numel() == d.ngroups);
  auto dyc = dy.contiguous();
  auto dx = at::empty_like(x);
  auto dres = has_res ? at::empty_like(x)
                      : at::empty({0}, x.options());
  auto dgamma = at::zeros({clients, d.ch}, x.options().dtype(at::kFloat));
  auto dbeta = at::zeros({clients, d.ch}, x.options().dtype(at::kFloat));
  auto stream = at::cuda::getCurrentCUDAStream();
  ols_groupnorm_bwd(x.data_ptr(), y.data_ptr(), dyc.data_ptr(),
                    dx.data_ptr(), has_res ? dres.data_ptr() : nullptr,
                    mean.data_ptr<float>(), rstd.data_ptr<float>(),
                    gamma.data_ptr(), dgamma.data_ptr<float>(),
                    dbeta.data_ptr<float>(), (int)d.B, (int)clients,
                    (int)d.ch, (int)groups, (int)d.HW, relu, d.layout,
                    gn_dtype(x), stream.stream());
  return {dx, dres, dgamma, dbeta};
}

at::Tensor mfma_selftest(at::Tensor A, at::Tensor B) {
  TORCH_CHECK(A.is_cuda() && A.scalar_type() == at::kBFloat16);
  TORCH_CHECK(A.sizes() == at::IntArrayRef({16, 32}) &&
              B.sizes() == at::IntArrayRef({32, 16}));
  auto D = at::empty({16, 16}, A.options().dtype(at::kFloat));
  ols_mfma_selftest(A.contiguous().data_ptr(), B.contiguous().data_ptr(),
                    D.data_ptr<float>(),
                    at::cuda::getCurrentCUDAStream().stream());
  return D;
}

// ---- client-batched convolutions -----------------------------------------

// Shape of one k x k conv call (k = 3: pad 1, stride 1 or 2; k = 5: valid,
// stride 1), for all nine wrappers.  A call has two of the three operands
//   x  [C, IC, B, H + 2*x_halo, W + 2*x_halo]
//   dy [C, OC, B, OH + 2*dy_halo, OW + 2*dy_halo]
//   w  [C, OC, IC, k, k]
// and passes an undefined tensor for the third; H, W are read from x, or
// given when x is absent (dgrad).  Every operand must be a contiguous 5-D
// bf16 tensor on one device (the kernels reinterpret everything as bf16)
// of exactly the size above, so C, IC, OC, B and the planes the kernels
// index agree across the call.
struct ConvDims {
  int C, IC, OC, B, H, W, OH, OW;
};

ConvDims conv_dims(int k, const at::Tensor& x, int x_halo,
                   const at::Tensor& dy, int dy_halo, const at::Tensor& w,
                   int64_t H, int64_t W, int64_t stride) {
  const at::Tensor& first = x.defined() ? x : dy;
  for (const at::Tensor* t : {&x, &dy, &w}) {
    if (!t->defined()) continue;
    TORCH_CHECK(t->is_cuda() && t->is_contiguous() && t->dim() == 5 &&
                    t->scalar_type() == at::kBFloat16 &&
                    t->device() == first.device(),
                "conv", k, "x", k, ": operands must be contiguous 5-D bf16 "
                "tensors on one GPU");
  }
  TORCH_CHECK(stride == 1 || (k == 3 && stride == 2), "conv", k, "x", k,
              ": stride ", stride, " unsupported");
  if (x.defined()) {
    H = x.size(3) - 2 * x_halo;
    W = x.size(4) - 2 * x_halo;
  }
  const int64_t C = first.size(0), B = first.size(2);
  const int64_t IC = x.defined() ? x.size(1) : w.size(2);
  const int64_t OC = dy.defined() ? dy.size(1) : w.size(1);
  const int64_t OH = k == 3 ? (H + stride - 1) / stride : H - 4;
  const int64_t OW = k == 3 ? (W + stride - 1) / stride : W - 4;
  TORCH_CHECK(C > 0 && IC > 0 && OC > 0 && B > 0 && OH > 0 && OW > 0,
              "conv", k, "x", k, ": empty operand or plane");
  auto expect = [&](const at::Tensor& t, const char* name,
                    std::vector<int64_t> sizes) {
    TORCH_CHECK(!t.defined() || t.sizes() == at::IntArrayRef(sizes), "conv",
                k, "x", k, ": ", name, " is ", t.sizes(), ", expected ",
                at::IntArrayRef(sizes));
  };
  expect(x, "x", {C, IC, B, H + 2 * x_halo, W + 2 * x_halo});
  expect(dy, "dy", {C, OC, B, OH + 2 * dy_halo, OW + 2 * dy_halo});
  expect(w, "w", {C, OC, IC, k, k});
  return {(int)C, (int)IC, (int)OC, (int)B, (int)H, (int)W, (int)OH, (int)OW};
}

// ---- 3x3, v5 family (client_conv.hip): dense operands ----------------------

at::Tensor conv3x3_fwd(at::Tensor x, at::Tensor w, int64_t stride) {
  const ConvDims d = conv_dims(3, x, 0, {}, 0, w, 0, 0, stride);
  auto y = at::empty({d.C, d.OC, d.B, d.OH, d.OW}, x.options());
  ols_conv3x3_fwd(x.data_ptr(), w.data_ptr(), y.data_ptr(), d.C, d.IC, d.OC,
                  d.B, d.H, d.W, (int)stride,
                  at::cuda::getCurrentCUDAStream().stream());
  return y;
}

at::Tensor conv3x3_dgrad(at::Tensor dy, at::Tensor w, int64_t H, int64_t W,
                         int64_t stride) {
  const ConvDims d = conv_dims(3, {}, 0, dy, 0, w, H, W, stride);
  auto dx = at::empty({d.C, d.IC, d.B, d.H, d.W}, dy.options());
  ols_conv3x3_dgrad(dy.data_ptr(), w.data_ptr(), dx.data_ptr(), d.C, d.IC,
                    d.OC, d.B, d.H, d.W, (int)stride,
                    at::cuda::getCurrentCUDAStream().stream());
  return dx;
}

at::Tensor conv3x3_wgrad(at::Tensor x, at::Tensor dy, int64_t stride) {
  const ConvDims d = conv_dims(3, x, 0, dy, 0, {}, 0, 0, stride);
  auto dw = at::empty({d.C, d.OC, d.IC, 3, 3}, x.options());
  ols_conv3x3_wgrad(x.data_ptr(), dy.data_ptr(), dw.data_ptr(), d.C, d.IC,
                    d.OC, d.B, d.H, d.W, (int)stride,
                    at::cuda::getCurrentCUDAStream().stream());
  return dw;
}

// ---- 3x3, v6 padded family (client_conv2.hip) ------------------------------
// x_pad and dy_pad carry a 1-element zero halo per plane

bool conv3x3_v6_ok(int64_t IC, int64_t OC, int64_t B, int64_t H, int64_t W,
                   int64_t stride) {
  return ols_conv3x3_v6_ok((int)IC, (int)OC, (int)B, (int)H, (int)W,
                           (int)stride) != 0;
}

// The kernel, with its template arguments, that x [*, IC, B, H, W] and OC
// output channels run in direction dir ("fwd", "dgrad", "wgrad"), e.g.
// "fwd_v7<5,1>".  Same host functions the launchers switch on, family
// decision included; reads the OLSIM_CONV_* variables on every call.
std::string conv3x3_route(std::string dir, int64_t IC, int64_t OC, int64_t B,
                          int64_t H, int64_t W, int64_t stride) {
  int d = dir == "fwd" ? 0 : dir == "dgrad" ? 1 : dir == "wgrad" ? 2 : -1;
  TORCH_CHECK(d >= 0, "conv3x3_route: dir must be fwd, dgrad or wgrad");
  TORCH_CHECK(stride == 1 || stride == 2, "conv3x3_route: stride 1 or 2");
  return ols_conv3x3_route(d, (int)IC, (int)OC, (int)B, (int)H, (int)W,
                           (int)stride);
}

// "kmajor" or "nmajor": how the kernel conv3x3_route names stages its B
// tile (conv3_route.h conv3_kmajor; OLSIM_CONV_NMAJOR forces "nmajor").
std::string conv3x3_staging(std::string dir, int64_t IC, int64_t OC,
                            int64_t B, int64_t H, int64_t W, int64_t stride) {
  int d = dir == "fwd" ? 0 : dir == "dgrad" ? 1 : dir == "wgrad" ? 2 : -1;
  TORCH_CHECK(d >= 0, "conv3x3_staging: dir must be fwd, dgrad or wgrad");
  TORCH_CHECK(stride == 1 || stride == 2, "conv3x3_staging: stride 1 or 2");
  return ols_conv3x3_staging(d, (int)IC, (int)OC, (int)B, (int)H, (int)W,
                             (int)stride);
}

// "64x128" or "128x64": the block tile of the kernel conv3x3_route names
// (conv3_route.h conv3_tile; OLSIM_CONV_BM64 forces "64x128").  The
// flipped-weight dgrad runs the forward of (OC, IC): ask for that.
std::string conv3x3_tile(std::string dir, int64_t IC, int64_t OC, int64_t B,
                         int64_t H, int64_t W, int64_t stride) {
  int d = dir == "fwd" ? 0 : dir == "dgrad" ? 1 : dir == "wgrad" ? 2 : -1;
  TORCH_CHECK(d >= 0, "conv3x3_tile: dir must be fwd, dgrad or wgrad");
  TORCH_CHECK(stride == 1 || stride == 2, "conv3x3_tile: stride 1 or 2");
  return ols_conv3x3_tile(d, (int)IC, (int)OC, (int)B, (int)H, (int)W,
                          (int)stride);
}

void check_v6(const ConvDims& d, int64_t stride) {
  TORCH_CHECK(ols_conv3x3_v6_ok(d.IC, d.OC, d.B, d.H, d.W, (int)stride),
              "shape unsupported by the v6 conv path");
}

at::Tensor conv3x3_fwd_p(at::Tensor xp, at::Tensor w, int64_t stride) {
  const ConvDims d = conv_dims(3, xp, 1, {}, 0, w, 0, 0, stride);
  check_v6(d, stride);
  auto y = at::empty({d.C, d.OC, d.B, d.OH, d.OW}, xp.options());
  ols_conv3x3_fwd_p(xp.data_ptr(), w.data_ptr(), y.data_ptr(), d.C, d.IC,
                    d.OC, d.B, d.H, d.W, (int)stride,
                    at::cuda::getCurrentCUDAStream().stream());
  return y;
}

at::Tensor conv3x3_dgrad_p(at::Tensor dyp, at::Tensor w, int64_t H, int64_t W,
                           int64_t stride) {
  const ConvDims d = conv_dims(3, {}, 0, dyp, 1, w, H, W, stride);
  check_v6(d, stride);
  auto dx = at::empty({d.C, d.IC, d.B, d.H, d.W}, dyp.options());
  ols_conv3x3_dgrad_p(dyp.data_ptr(), w.data_ptr(), dx.data_ptr(), d.C, d.IC,
                      d.OC, d.B, d.H, d.W, (int)stride,
                      at::cuda::getCurrentCUDAStream().stream());
  return dx;
}

at::Tensor conv3x3_wgrad_p(at::Tensor xp, at::Tensor dy, int64_t stride) {
  const ConvDims d = conv_dims(3, xp, 1, dy, 0, {}, 0, 0, stride);
  check_v6(d, stride);
  auto dw = at::empty({d.C, d.OC, d.IC, 3, 3}, xp.options());
  ols_conv3x3_wgrad_p(xp.data_ptr(), dy.data_ptr(), dw.data_ptr(), d.C, d.IC,
                      d.OC, d.B, d.H, d.W, (int)stride,
                      at::cuda::getCurrentCUDAStream().stream());
  return dw;
}

// ---- flipped-transposed 3x3 weights (conv3_wflip.hip) ----------------------
// wt [C, IC, OC, 3, 3] with wt[c][ic][oc][r] = w[c][oc][ic][8 - r]:
// conv3x3_fwd_p(dy_pad, wt, 1) is the stride-1 dgrad of w.

struct WflipDims {
  int C, OC, IC;
};

// w, and every further operand, a contiguous bf16 [C, OC, IC, 3, 3] on one
// GPU with OC and IC multiples of the kernels' 32 x 32 tile (what
// conv3_v6_ok admits at stride 1); wt the same with OC and IC swapped
WflipDims wflip_dims(const at::Tensor& w, const at::Tensor& g,
                     const at::Tensor& wt) {
  TORCH_CHECK(w.is_cuda() && w.is_contiguous() && w.dim() == 5 &&
                  w.scalar_type() == at::kBFloat16 && w.size(3) == 3 &&
                  w.size(4) == 3,
              "conv3x3_wflip: w must be a contiguous bf16 [C, OC, IC, 3, 3] "
              "GPU tensor, got ", w.scalar_type(), " ", w.sizes());
  const int64_t C = w.size(0), OC = w.size(1), IC = w.size(2);
  TORCH_CHECK(C > 0 && OC > 0 && IC > 0 && OC % 32 == 0 && IC % 32 == 0,
              "conv3x3_wflip: OC and IC must be multiples of 32, got ",
              w.sizes());
  TORCH_CHECK(C * (OC / 32) * (IC / 32) <= INT32_MAX,
              "conv3x3_wflip: too many tiles");
  for (const at::Tensor* t : {&w, &g, &wt}) {
    if (!t->defined()) continue;
    TORCH_CHECK(t->is_cuda() && t->is_contiguous() &&
                    t->scalar_type() == at::kBFloat16 &&
                    t->device() == w.device() &&
                    reinterpret_cast<uintptr_t>(t->data_ptr()) % 16 == 0,
                "conv3x3_wflip: operands must be contiguous, 16-byte "
                "aligned bf16 tensors on one GPU");
  }
  TORCH_CHECK(!g.defined() || g.sizes() == w.sizes(),
              "sgd_conv3_wt: g is ", g.sizes(), ", expected ", w.sizes());
  TORCH_CHECK(!wt.defined() ||
                  wt.sizes() == at::IntArrayRef({C, IC, OC, 3, 3}),
              "sgd_conv3_wt: wt is ", wt.sizes(), ", expected [", C, ", ",
              IC, ", ", OC, ", 3, 3]");
  return {(int)C, (int)OC, (int)IC};
}

at::Tensor conv3x3_wflip(at::Tensor w) {
  const WflipDims d = wflip_dims(w, {}, {});
  auto wt = at::empty({d.C, d.IC, d.OC, 3, 3}, w.options());
  ols_conv3_wflip(w.data_ptr(), wt.data_ptr(), d.C, d.OC, d.IC,
                  at::cuda::getCurrentCUDAStream().stream());
  return wt;
}

void sgd_conv3_wt(at::Tensor w, at::Tensor g, at::Tensor wt, double lr) {
  const WflipDims d = wflip_dims(w, g, wt);
  // the three tensors have the same byte size; wt must overlap neither
  const char* wtp = static_cast<const char*>(wt.data_ptr());
  const int64_t nbytes = (int64_t)wt.numel() * 2;
  for (const at::Tensor* t : {&w, &g}) {
    const char* p = static_cast<const char*>(t->data_ptr());
    TORCH_CHECK(p + nbytes <= wtp || wtp + nbytes <= p,
                "sgd_conv3_wt: wt must not overlap w or g");
  }
  ols_sgd_conv3_wt(w.data_ptr(), g.data_ptr(), wt.data_ptr(), d.C, d.OC,
                   d.IC, (float)lr,
                   at::cuda::getCurrentCUDAStream().stream());
}

// ---- 5x5 VALID family (client_conv5.hip, LeNet) -------------------------
// ntab: int32 [B*OH*OW] plane offsets (b*H*W + oh*W + ow) built host-side

// Which kernel a [*, IC, *, H, W] x and OC output channels run in
// direction dir ("fwd", "dgrad", "wgrad"): "direct" or "mfma".  Same host
// functions the launchers branch on; reads OLSIM_CONV5 on every call.
std::string conv5x5_route(std::string dir, int64_t IC, int64_t OC, int64_t H,
                          int64_t W) {
  int d = dir == "fwd" ? 0 : dir == "dgrad" ? 1 : dir == "wgrad" ? 2 : -1;
  TORCH_CHECK(d >= 0, "conv5x5_route: dir must be fwd, dgrad or wgrad");
  int r = ols_conv5x5_route(d, (int)IC, (int)OC, (int)H, (int)W);
  return r == 0 ? "direct" : "mfma";
}

// ntab has one int32 per position of the plane the kernel tiles over
void check_ntab(const at::Tensor& ntab, const at::Tensor& on, int64_t n) {
  TORCH_CHECK(ntab.is_cuda() && ntab.device() == on.device() &&
                  ntab.scalar_type() == at::kInt && ntab.is_contiguous() &&
                  ntab.numel() == n,
              "conv5x5: ntab must be ", n, " contiguous int32 on the GPU");
}

at::Tensor conv5x5_fwd(at::Tensor x, at::Tensor w, at::Tensor bias,
                       at::Tensor ntab, bool relu) {
  const ConvDims d = conv_dims(5, x, 0, {}, 0, w, 0, 0, 1);
  TORCH_CHECK(d.OC <= 16);
  check_ntab(ntab, x, (int64_t)d.B * d.OH * d.OW);
  TORCH_CHECK(bias.is_cuda() && bias.scalar_type() == at::kBFloat16 &&
              bias.numel() == (int64_t)d.C * d.OC);
  auto y = at::empty({d.C, d.OC, d.B, d.OH, d.OW}, x.options());
  ols_conv5x5_fwd(x.data_ptr(), w.data_ptr(), bias.contiguous().data_ptr(),
                  y.data_ptr(), ntab.data_ptr<int>(), d.C, d.IC, d.OC, d.B,
                  d.H, d.W, relu ? 1 : 0,
                  at::cuda::getCurrentCUDAStream().stream());
  return y;
}

// dyp: dy padded by 4, [C, OC, B, H+4, W+4]; returns dx [C, IC, B, H, W]
at::Tensor conv5x5_dgrad(at::Tensor dyp, at::Tensor w, at::Tensor ntab,
                         int64_t H, int64_t W) {
  const ConvDims d = conv_dims(5, {}, 0, dyp, 4, w, H, W, 1);
  TORCH_CHECK(d.IC <= 16);
  check_ntab(ntab, dyp, (int64_t)d.B * d.H * d.W);
  auto dx = at::empty({d.C, d.IC, d.B, d.H, d.W}, dyp.options());
  ols_conv5x5_dgrad(dyp.data_ptr(), w.data_ptr(), dx.data_ptr(),
                    ntab.data_ptr<int>(), d.C, d.IC, d.OC, d.B, d.H, d.W,
                    at::cuda::getCurrentCUDAStream().stream());
  return dx;
}

at::Tensor conv5x5_wgrad(at::Tensor x, at::Tensor dy, at::Tensor ntab) {
  const ConvDims d = conv_dims(5, x, 0, dy, 0, {}, 0, 0, 1);
  const int64_t nq = (int64_t)d.B * d.OH * d.OW;
  TORCH_CHECK(d.OC <= 16 && nq % 32 == 0);
  check_ntab(ntab, x, nq);
  auto dw = at::empty({d.C, d.OC, d.IC, 5, 5}, x.options());
  ols_conv5x5_wgrad(x.data_ptr(), dy.data_ptr(), dw.data_ptr(),
                    ntab.data_ptr<int>(), d.C, d.IC, d.OC, d.B, d.H, d.W,
                    at::cuda::getCurrentCUDAStream().stream());
  return dw;
}

// ---- 2x2 max pool (pool2x2.hip) -----------------------------------------
// x: [..., H, W] with H, W even; pooled over the last two dims

std::tuple<at::Tensor, at::Tensor> pool2x2_fwd(at::Tensor x) {
  TORCH_CHECK(x.is_cuda() && x.is_contiguous() && x.dim() >= 2);
  int H = x.size(-2), W = x.size(-1);
  TORCH_CHECK(H % 2 == 0 && W % 2 == 0);
  int64_t planes = x.numel() / ((int64_t)H * W);
  auto sizes = x.sizes().vec();
  sizes[sizes.size() - 2] = H / 2;
  sizes[sizes.size() - 1] = W / 2;
  auto y = at::empty(sizes, x.options());
  auto arg = at::empty(sizes, x.options().dtype(at::kByte));
  int dt = x.scalar_type() == at::kBFloat16 ? 1 : 0;
  ols_pool2x2_fwd(x.data_ptr(), y.data_ptr(),
                  (unsigned char*)arg.data_ptr(), planes, H / 2, W / 2, dt,
                  at::cuda::getCurrentCUDAStream().stream());
  return {y, arg};
}

at::Tensor pool2x2_bwd(at::Tensor dy, at::Tensor arg) {
  TORCH_CHECK(dy.is_cuda() && dy.is_contiguous() && dy.dim() >= 2);
  int OH = dy.size(-2), OW = dy.size(-1);
  int64_t planes = dy.numel() / ((int64_t)OH * OW);
  auto sizes = dy.sizes().vec();
  sizes[sizes.size() - 2] = OH * 2;
  sizes[sizes.size() - 1] = OW * 2;
  auto dx = at::empty(sizes, dy.options());
  int dt = dy.scalar_type() == at::kBFloat16 ? 1 : 0;
  ols_pool2x2_bwd(dy.data_ptr(), (unsigned char*)arg.contiguous().data_ptr(),
                  dx.data_ptr(), planes, OH, OW, dt,
                  at::cuda::getCurrentCUDAStream().stream());
  return dx;
}

// ---- per-client LayerNorm (layernorm.hip) -------------------------------
// x [C, N, H] (N rows per client); gamma/beta [C, H]

std::tuple<at::Tensor, at::Tensor, at::Tensor> layernorm_fwd(
    at::Tensor x, at::Tensor gamma, at::Tensor beta, double eps) {
  TORCH_CHECK(x.is_cuda() && x.is_contiguous() && x.dim() == 3);
  TORCH_CHECK(gamma.is_contiguous() && beta.is_contiguous());
  int64_t C = x.size(0), N = x.size(1);
  int H = x.size(2);
  TORCH_CHECK(H % 8 == 0 && N % 4 == 0, "layernorm_fwd: H%8, N%4");
  int64_t rows = C * N;
  auto y = at::empty_like(x);
  auto mean = at::empty({rows}, x.options().dtype(at::kFloat));
  auto rstd = at::empty({rows}, x.options().dtype(at::kFloat));
  int dt = x.scalar_type() == at::kBFloat16 ? 1 : 0;
  ols_layernorm_fwd(x.data_ptr(), gamma.data_ptr(), beta.data_ptr(),
                    y.data_ptr(), mean.data_ptr<float>(),
                    rstd.data_ptr<float>(), rows, H, N, (float)eps, dt,
                    at::cuda::getCurrentCUDAStream().stream());
  return {y, mean, rstd};
}

std::tuple<at::Tensor, at::Tensor, at::Tensor> layernorm_bwd(
    at::Tensor x, at::Tensor dy, at::Tensor gamma, at::Tensor mean,
    at::Tensor rstd) {
  TORCH_CHECK(x.is_cuda() && x.is_contiguous() && dy.is_contiguous());
  int64_t C = x.size(0), N = x.size(1);
  int H = x.size(2);
  int64_t rows = C * N;
  auto dx = at::empty_like(x);
  auto dgamma = at::zeros({C, (int64_t)H}, x.options().dtype(at::kFloat));
  auto dbeta = at::zeros({C, (int64_t)H}, x.options().dtype(at::kFloat));
  int dt = x.scalar_type() == at::kBFloat16 ? 1 : 0;
  ols_layernorm_bwd(x.data_ptr(), dy.data_ptr(),
                    gamma.contiguous().data_ptr(), mean.data_ptr<float>(),
                    rstd.data_ptr<float>(), dx.data_ptr(),
                    dgamma.data_ptr<float>(), dbeta.data_ptr<float>(), rows,
                    H, N, dt, at::cuda::getCurrentCUDAStream().stream());
  return {dx, dgamma, dbeta};
}

// ---- 2x stride subsample (pool2x2.hip) ----------------------------------

at::Tensor subsample2(at::Tensor x) {
  TORCH_CHECK(x.is_cuda() && x.is_contiguous() && x.dim() >= 2);
  int H = x.size(-2), W = x.size(-1);
  TORCH_CHECK(H % 2 == 0 && W % 4 == 0);
  TORCH_CHECK(x.scalar_type() == at::kBFloat16 ||
              x.scalar_type() == at::kFloat);
  int64_t planes = x.numel() / ((int64_t)H * W);
  auto sizes = x.sizes().vec();
  sizes[sizes.size() - 2] = H / 2;
  sizes[sizes.size() - 1] = W / 2;
  auto y = at::empty(sizes, x.options());
  int dt = x.scalar_type() == at::kBFloat16 ? 1 : 0;
  ols_subsample2_fwd(x.data_ptr(), y.data_ptr(), planes, H / 2, W / 2, dt,
                     at::cuda::getCurrentCUDAStream().stream());
  return y;
}

at::Tensor subsample2_bwd(at::Tensor dy, int64_t H, int64_t W) {
  TORCH_CHECK(dy.is_cuda() && dy.is_contiguous() && dy.dim() >= 2);
  TORCH_CHECK(dy.size(-2) == H / 2 && dy.size(-1) == W / 2);
  int64_t planes = dy.numel() / ((int64_t)(H / 2) * (W / 2));
  auto sizes = dy.sizes().vec();
  sizes[sizes.size() - 2] = H;
  sizes[sizes.size() - 1] = W;
  auto dx = at::empty(sizes, dy.options());
  int dt = dy.scalar_type() == at::kBFloat16 ? 1 : 0;
  ols_subsample2_bwd(dy.data_ptr(), dx.data_ptr(), planes, (int)H, (int)W,
                     dt, at::cuda::getCurrentCUDAStream().stream());
  return dx;
}

// ---- padded-output GroupNorm pair (groupnorm.hip) -----------------------
// x: [C, ch, B, H, W] bf16.  y is [C, ch, B, H+2, W+2] with a zero halo
// (pad_out) or dense; mask is the 1-bit ReLU mask the backward consumes.
// res: empty, dense (x's shape) or padded (y's padded shape).  ReLU is
// always applied.

bool gn_pad_ok(int64_t ch, int64_t groups, int64_t H, int64_t W) {
  return ols_gn_pad_ok((int)ch, (int)groups, (int)H, (int)W) != 0;
}

std::tuple<at::Tensor, at::Tensor, at::Tensor, at::Tensor> groupnorm_fwd_pad(
    at::Tensor x, at::Tensor res, at::Tensor gamma, at::Tensor beta,
    int64_t clients, int64_t groups, double eps, bool pad_out) {
  TORCH_CHECK(x.dim() == 5);
  TORCH_CHECK(x.scalar_type() == at::kBFloat16 &&
              gamma.scalar_type() == at::kBFloat16 &&
              beta.scalar_type() == at::kBFloat16);
  const GnDims d = gn_dims(x, clients, groups);
  const int64_t ch = d.ch, B = d.B, H = d.H, W = d.W;
  TORCH_CHECK(ols_gn_pad_ok((int)ch, (int)groups, (int)H, (int)W),
              "shape unsupported by the padded GroupNorm path");
  TORCH_CHECK(gamma.is_contiguous() && beta.is_contiguous() &&
              gamma.numel() == clients * ch && beta.numel() == clients * ch);
  std::vector<int64_t> psizes = {clients, ch, B, H + 2, W + 2};
  int res_mode = 0;
  if (res.numel() > 0) {
    TORCH_CHECK(res.is_cuda() && res.is_contiguous() &&
                res.scalar_type() == at::kBFloat16);
    if (res.sizes() == x.sizes()) res_mode = 1;
    else if (res.sizes() == at::IntArrayRef(psizes)) res_mode = 2;
    else TORCH_CHECK(false, "groupnorm_fwd_pad: residual shape mismatch");
  }
  auto y = pad_out ? at::empty(psizes, x.options()) : at::empty_like(x);
  auto mask = at::empty({d.ngroups, (d.n + 31) / 32},
                        x.options().dtype(at::kInt));
  auto mean = at::empty({d.ngroups}, x.options().dtype(at::kFloat));
  auto rstd = at::empty({d.ngroups}, x.options().dtype(at::kFloat));
  ols_groupnorm_fwd_pad(
      x.data_ptr(), res_mode ? res.data_ptr() : nullptr, res_mode,
      y.data_ptr(), reinterpret_cast<uint32_t*>(mask.data_ptr<int>()),
      mean.data_ptr<float>(), rstd.data_ptr<float>(), gamma.data_ptr(),
      beta.data_ptr(), (int)B, (int)clients, (int)ch, (int)groups, (int)H,
      (int)W, (float)eps, pad_out,
      at::cuda::getCurrentCUDAStream().stream());
  return {y, mask, mean, rstd};
}

// returns (dx dense, dx_pad or empty, dres dense or empty, dgamma, dbeta)
std::tuple<at::Tensor, at::Tensor, at::Tensor, at::Tensor, at::Tensor>
groupnorm_bwd_pad(at::Tensor x, at::Tensor mask, at::Tensor dy,
                  at::Tensor mean, at::Tensor rstd, at::Tensor gamma,
                  int64_t clients, int64_t groups, bool has_res,
                  bool want_pad) {
  TORCH_CHECK(x.dim() == 5);
  TORCH_CHECK(x.scalar_type() == at::kBFloat16 &&
              dy.scalar_type() == at::kBFloat16 && dy.sizes() == x.sizes());
  const GnDims d = gn_dims(x, clients, groups);
  const int64_t ch = d.ch, B = d.B, H = d.H, W = d.W;
  TORCH_CHECK(ols_gn_pad_ok((int)ch, (int)groups, (int)H, (int)W));
  TORCH_CHECK(mask.is_contiguous() && mask.scalar_type() == at::kInt &&
              mask.numel() == d.ngroups * ((d.n + 31) / 32));
  TORCH_CHECK(mean.numel() == d.ngroups && rstd.numel() == d.ngroups);
  auto dyc = dy.contiguous();
  auto dx = at::empty_like(x);
  auto dx_pad = want_pad ? at::empty({clients, ch, B, H + 2, W + 2},
                                     x.options())
                         : at::empty({0}, x.options());
  auto dres = has_res ? at::empty_like(x) : at::empty({0}, x.options());
  auto dgamma = at::zeros({clients, ch}, x.options().dtype(at::kFloat));
  auto dbeta = at::zeros({clients, ch}, x.options().dtype(at::kFloat));
  ols_groupnorm_bwd_pad(
      x.data_ptr(), reinterpret_cast<const uint32_t*>(mask.data_ptr<int>()),
      dyc.data_ptr(), dx.data_ptr(), want_pad ? dx_pad.data_ptr() : nullptr,
      has_res ? dres.data_ptr() : nullptr, mean.data_ptr<float>(),
      rstd.data_ptr<float>(), gamma.data_ptr(), dgamma.data_ptr<float>(),
      dbeta.data_ptr<float>(), (int)B, (int)clients, (int)ch, (int)groups,
      (int)H, (int)W, at::cuda::getCurrentCUDAStream().stream());
  return {dx, dx_pad, dres, dgamma, dbeta};
}

// padded-input subsample: xp [.., H+2, W+2] -> [.., H/2, W/2]
at::Tensor subsample2_p(at::Tensor xp) {
  TORCH_CHECK(xp.is_cuda() && xp.is_contiguous() && xp.dim() >= 2);
  int H = xp.size(-2) - 2, W = xp.size(-1) - 2;
  TORCH_CHECK(H >= 2 && H % 2 == 0 && W % 4 == 0);
  TORCH_CHECK(xp.scalar_type() == at::kBFloat16 ||
              xp.scalar_type() == at::kFloat);
  int64_t planes = xp.numel() / ((int64_t)(H + 2) * (W + 2));
  auto sizes = xp.sizes().vec();
  sizes[sizes.size() - 2] = H / 2;
  sizes[sizes.size() - 1] = W / 2;
  auto y = at::empty(sizes, xp.options());
  int dt = xp.scalar_type() == at::kBFloat16 ? 1 : 0;
  ols_subsample2p_fwd(xp.data_ptr(), y.data_ptr(), planes, H / 2, W / 2, dt,
                      at::cuda::getCurrentCUDAStream().stream());
  return y;
}

// ---- client replica broadcast (replicate.hip) ---------------------------

at::Tensor replicate(at::Tensor src, int64_t clients) {
  TORCH_CHECK(src.is_cuda() && src.is_contiguous() && clients >= 1);
  TORCH_CHECK(src.numel() % 8 == 0);
  TORCH_CHECK(src.scalar_type() == at::kBFloat16 ||
              src.scalar_type() == at::kFloat);
  // k_replicate reads src as 16-byte packs; a view into a flat buffer
  // can start anywhere (replicate_params clones those instead)
  TORCH_CHECK(reinterpret_cast<uintptr_t>(src.data_ptr()) % 16 == 0,
              "replicate: src must start on a 16-byte boundary");
  auto sizes = src.sizes().vec();
  sizes.insert(sizes.begin(), clients);
  auto dst = at::empty(sizes, src.options());
  int dt = src.scalar_type() == at::kBFloat16 ? 1 : 0;
  ols_replicate(src.data_ptr(), dst.data_ptr(), clients, src.numel(), dt,
                at::cuda::getCurrentCUDAStream().stream());
  return dst;
}

at::Tensor synth_batch(at::Tensor x, at::Tensor y, double s, double t) {
  // x [B, n] fp32, y [rows] int64 (rows = C*B) -> out [rows, n] bf16
  TORCH_CHECK(x.is_cuda() && x.is_contiguous() && x.dim() == 2);
  TORCH_CHECK(x.scalar_type() == at::kFloat && x.size(1) % 8 == 0);
  TORCH_CHECK(y.is_cuda() && y.is_contiguous() &&
              y.scalar_type() == at::kLong);
  int64_t rows = y.numel(), batch = x.size(0), n = x.size(1);
  TORCH_CHECK(rows % batch == 0);
  auto out = at::empty({rows, n}, x.options().dtype(at::kBFloat16));
  ols_synth_batch(x.data_ptr<float>(), y.data_ptr<int64_t>(),
                  out.data_ptr(), rows, batch, n, (float)s, (float)t,
                  at::cuda::getCurrentCUDAStream().stream());
  return out;
}

// ---- fused relu-mask backward (replicate.hip) ---------------------------

at::Tensor relu_mask(at::Tensor dy, at::Tensor y) {
  TORCH_CHECK(dy.is_cuda() && dy.is_contiguous() && y.is_contiguous());
  TORCH_CHECK(dy.sizes() == y.sizes() && dy.scalar_type() == y.scalar_type());
  TORCH_CHECK(dy.numel() % 8 == 0);
  TORCH_CHECK(dy.scalar_type() == at::kBFloat16 ||
              dy.scalar_type() == at::kFloat);
  auto out = at::empty_like(dy);
  int dt = dy.scalar_type() == at::kBFloat16 ? 1 : 0;
  ols_relu_mask(dy.data_ptr(), y.data_ptr(), out.data_ptr(), dy.numel(), dt,
                at::cuda::getCurrentCUDAStream().stream());
  return out;
}

// ---- zero-pad trailing 2 dims (pad2d.hip) -------------------------------

at::Tensor pad2d(at::Tensor x, int64_t pad) {
  TORCH_CHECK(x.is_cuda() && x.is_contiguous() && x.dim() >= 2);
  TORCH_CHECK(x.scalar_type() == at::kBFloat16 ||
              x.scalar_type() == at::kHalf);
  int H = x.size(-2), W = x.size(-1);
  TORCH_CHECK(W % 2 == 0 && pad >= 1);
  int64_t planes = x.numel() / ((int64_t)H * W);
  auto sizes = x.sizes().vec();
  sizes[sizes.size() - 2] = H + 2 * pad;
  sizes[sizes.size() - 1] = W + 2 * pad;
  auto y = at::empty(sizes, x.options());
  int dt = x.scalar_type() == at::kBFloat16 ? 1 : 2;
  ols_pad2d(x.data_ptr(), y.data_ptr(), planes, H, W, (int)pad, dt,
            at::cuda::getCurrentCUDAStream().stream());
  return y;
}

// ---- batched 2-D transpose (transpose.hip) ------------------------------

at::Tensor transpose2d(at::Tensor x) {
  TORCH_CHECK(x.is_cuda() && x.is_contiguous() && x.dim() == 3);
  TORCH_CHECK(x.scalar_type() == at::kBFloat16 ||
              x.scalar_type() == at::kFloat);
  int64_t B = x.size(0);
  int M = x.size(1), N = x.size(2);
  // the batch is the grid's z dimension in both kernels
  TORCH_CHECK(B <= 65535, "transpose2d: batch ", B, " exceeds 65535");
  auto y = at::empty({B, (int64_t)N, (int64_t)M}, x.options());
  int dt = x.scalar_type() == at::kBFloat16 ? 1 : 0;
  ols_transpose2d(x.data_ptr(), y.data_ptr(), B, M, N, dt,
                  at::cuda::getCurrentCUDAStream().stream());
  return y;
}

}  // namespace

TORCH_LIBRARY(olsim_hip, m) {
  m.def("fused_sgd_update_flat(Tensor(a!) buf, Tensor grad, Tensor global_flat, "
        "Tensor offsets, int clients, float lr, float mu) -> ()");
  m.def("weighted_delta_accum_flat(Tensor(a!) delta, Tensor buf, "
        "Tensor global_flat, Tensor weights, Tensor offsets, int clients, float wsum) -> ()");
  m.def("weighted_delta_accum_flat_dw(Tensor(a!) delta, Tensor buf, "
        "Tensor global_flat, Tensor weights, Tensor offsets, int clients, "
        "Tensor wsum) -> ()");
  m.def("delta_accum_route(int nblocks, int n, int clients, int dtype, "
        "bool master_aligned, bool buf_aligned) -> str", &delta_accum_route);
  m.def("client_delta_sqnorm(Tensor(a!) sq, Tensor buf, Tensor master, "
        "int clients) -> ()");
  m.def("sqnorm_tiles(int n, int clients, int vec) -> int", &sqnorm_tiles);
  m.def("clip_weights(Tensor sq, Tensor weights, float clip_norm) -> "
        "(Tensor, Tensor)");
  m.def("delta_accum_quant(Tensor(a!) delta, Tensor buf, Tensor master, "
        "Tensor weights, Tensor client_ids, int clients, int bits, int k0, "
        "int k1, int elem_base, bool ids_checked=False) -> ()");
  m.def("delta_accum_quant_route(int n, int clients, int dtype, "
        "bool master_aligned, bool buf_aligned) -> str",
        &delta_accum_quant_route);
  m.def("server_opt_step(int kind, Tensor(a!) x, Tensor d, Tensor(b!) m, "
        "Tensor(c!) v, Tensor? z, float total_weight, float sigma, float lr, "
        "float beta1, float beta2, float tau) -> ()");
  m.def("server_opt_route(int n, bool aligned) -> str", &server_opt_route);
  m.def("cross_entropy_fwd_bwd(Tensor logits, Tensor labels) -> (Tensor, Tensor)");
  m.def("groupnorm_fwd(Tensor x, Tensor res, Tensor gamma, Tensor beta, "
        "int clients, int groups, float eps, bool relu) -> (Tensor, Tensor, Tensor)");
  m.def("groupnorm_bwd(Tensor x, Tensor y, Tensor dy, Tensor mean, "
        "Tensor rstd, Tensor gamma, int clients, int groups, bool has_res, "
        "bool relu) -> (Tensor, Tensor, Tensor, Tensor)");
  m.def("mfma_selftest(Tensor A, Tensor B) -> Tensor");
  m.def("conv3x3_fwd(Tensor x, Tensor w, int stride) -> Tensor");
  m.def("conv3x3_dgrad(Tensor dy, Tensor w, int H, int W, int stride) -> Tensor");
  m.def("conv3x3_wgrad(Tensor x, Tensor dy, int stride) -> Tensor");
  m.def("conv3x3_v6_ok(int IC, int OC, int B, int H, int W, int stride) -> bool",
        &conv3x3_v6_ok);
  m.def("conv3x3_route(str dir, int IC, int OC, int B, int H, int W, "
        "int stride) -> str", &conv3x3_route);
  m.def("conv3x3_staging(str dir, int IC, int OC, int B, int H, int W, "
        "int stride) -> str", &conv3x3_staging);
  m.def("conv3x3_tile(str dir, int IC, int OC, int B, int H, int W, "
        "int stride) -> str", &conv3x3_tile);
  m.def("conv3x3_fwd_p(Tensor xp, Tensor w, int stride) -> Tensor");
  m.def("conv3x3_dgrad_p(Tensor dyp, Tensor w, int H, int W, int stride) -> Tensor");
  m.def("conv3x3_wgrad_p(Tensor xp, Tensor dy, int stride) -> Tensor");
  m.def("conv3x3_wflip(Tensor w) -> Tensor");
  m.def("sgd_conv3_wt(Tensor(a!) w, Tensor g, Tensor(b!) wt, float lr) -> ()");
  m.def("conv5x5_route(str dir, int IC, int OC, int H, int W) -> str",
        &conv5x5_route);
  m.def("conv5x5_fwd(Tensor x, Tensor w, Tensor bias, Tensor ntab, bool relu) -> Tensor");
  m.def("conv5x5_dgrad(Tensor dyp, Tensor w, Tensor ntab, int H, int W) -> Tensor");
  m.def("conv5x5_wgrad(Tensor x, Tensor dy, Tensor ntab) -> Tensor");
  m.def("pool2x2_fwd(Tensor x) -> (Tensor, Tensor)");
  m.def("pool2x2_bwd(Tensor dy, Tensor arg) -> Tensor");
  m.def("transpose2d(Tensor x) -> Tensor");
  m.def("pad2d(Tensor x, int pad) -> Tensor");
  m.def("relu_mask(Tensor dy, Tensor y) -> Tensor");
  m.def("replicate(Tensor src, int clients) -> Tensor");
  m.def("subsample2(Tensor x) -> Tensor");
  m.def("subsample2_bwd(Tensor dy, int H, int W) -> Tensor");
  m.def("subsample2_p(Tensor xp) -> Tensor");
  m.def("gn_pad_ok(int ch, int groups, int H, int W) -> bool", &gn_pad_ok);
  m.def("groupnorm_fwd_pad(Tensor x, Tensor res, Tensor gamma, Tensor beta, "
        "int clients, int groups, float eps, bool pad_out) -> "
        "(Tensor, Tensor, Tensor, Tensor)");
  m.def("groupnorm_bwd_pad(Tensor x, Tensor mask, Tensor dy, Tensor mean, "
        "Tensor rstd, Tensor gamma, int clients, int groups, bool has_res, "
        "bool want_pad) -> (Tensor, Tensor, Tensor, Tensor, Tensor)");
  m.def("synth_batch(Tensor x, Tensor y, float s, float t) -> Tensor");
  m.def("layernorm_fwd(Tensor x, Tensor gamma, Tensor beta, float eps) -> (Tensor, Tensor, Tensor)");
  m.def("layernorm_bwd(Tensor x, Tensor dy, Tensor gamma, Tensor mean, Tensor rstd) -> (Tensor, Tensor, Tensor)");
}

TORCH_LIBRARY_IMPL(olsim_hip, CUDA, m) {
  m.impl("fused_sgd_update_flat", &fused_sgd_update_flat);
  m.impl("weighted_delta_accum_flat", &weighted_delta_accum_flat);
  m.impl("weighted_delta_accum_flat_dw", &weighted_delta_accum_flat_dw);
  m.impl("client_delta_sqnorm", &client_delta_sqnorm);
  m.impl("clip_weights", &clip_weights);
  m.impl("delta_accum_quant", &delta_accum_quant);
  m.impl("server_opt_step", &server_opt_step);
  m.impl("cross_entropy_fwd_bwd", &cross_entropy_fwd_bwd);
  m.impl("groupnorm_fwd", &groupnorm_fwd);
  m.impl("groupnorm_bwd", &groupnorm_bwd);
  m.impl("mfma_selftest", &mfma_selftest);
  m.impl("conv3x3_fwd", &conv3x3_fwd);
  m.impl("conv3x3_dgrad", &conv3x3_dgrad);
  m.impl("conv3x3_wgrad", &conv3x3_wgrad);
  m.impl("conv3x3_fwd_p", &conv3x3_fwd_p);
  m.impl("conv3x3_dgrad_p", &conv3x3_dgrad_p);
  m.impl("conv3x3_wgrad_p", &conv3x3_wgrad_p);
  m.impl("conv3x3_wflip", &conv3x3_wflip);
  m.impl("sgd_conv3_wt", &sgd_conv3_wt);
  m.impl("conv5x5_fwd", &conv5x5_fwd);
  m.impl("conv5x5_dgrad", &conv5x5_dgrad);
  m.impl("conv5x5_wgrad", &conv5x5_wgrad);
  m.impl("pool2x2_fwd", &pool2x2_fwd);
  m.impl("pool2x2_bwd", &pool2x2_bwd);
  m.impl("transpose2d", &transpose2d);
  m.impl("pad2d", &pad2d);
  m.impl("relu_mask", &relu_mask);
  m.impl("replicate", &replicate);
  m.impl("subsample2", &subsample2);
  m.impl("subsample2_bwd", &subsample2_bwd);
  m.impl("subsample2_p", &subsample2_p);
  m.impl("groupnorm_fwd_pad", &groupnorm_fwd_pad);
  m.impl("groupnorm_bwd_pad", &groupnorm_bwd_pad);
  m.impl("synth_batch", &synth_batch);
  m.impl("layernorm_fwd", &layernorm_fwd);
  m.impl("layernorm_bwd", &layernorm_bwd);
}
