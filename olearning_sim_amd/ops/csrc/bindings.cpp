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

// ---- fused LSTM recurrence (lstm.hip) --------------------------------------
// xp [C, B, L, 4H] (input projection, bias included) and w_hh [C, H, 4H];
// hs [C, B, L, H], gates [C, B, L, 4H] (post-nonlinearity, i|f|g|o) and
// cs [C, B, L, H] fp32 are written.  The outputs are arguments so that a
// caller decides where they live.  Everything but cs is bf16; every
// operand is contiguous, on one GPU and on a 16-byte boundary, and the
// shape is one lstm_route() calls "fused": anything else is an error here,
// never a quiet detour.

struct LstmDims {
  int C, B, L, H;
};

LstmDims lstm_dims(const char* op, const at::Tensor& w,
                   std::initializer_list<std::pair<const at::Tensor*, int>>
                       acts,
                   const at::Tensor& cs) {
  TORCH_CHECK(w.is_cuda() && w.dim() == 3 && w.size(2) == 4 * w.size(1), op,
              ": w_hh must be a [C, H, 4H] GPU tensor, got ", w.sizes());
  const int64_t C = w.size(0), H = w.size(1);
  const at::Tensor& first = *acts.begin()->first;
  TORCH_CHECK(first.dim() == 4, op, ": activations must be 4-D");
  const int64_t B = first.size(1), L = first.size(2);
  auto check = [&](const at::Tensor& t, int mult, at::ScalarType dt) {
    TORCH_CHECK(t.is_cuda() && t.device() == w.device() &&
                    t.is_contiguous() && t.scalar_type() == dt &&
                    reinterpret_cast<uintptr_t>(t.data_ptr()) % 16 == 0,
                op, ": operands must be contiguous, 16-byte aligned, on "
                "w_hh's GPU, bf16 (cs: fp32)");
    TORCH_CHECK(t.sizes() == at::IntArrayRef({C, B, L, mult * H}), op,
                ": operand is ", t.sizes(), ", expected ",
                at::IntArrayRef({C, B, L, mult * H}));
  };
  TORCH_CHECK(w.is_contiguous() && w.scalar_type() == at::kBFloat16 &&
                  reinterpret_cast<uintptr_t>(w.data_ptr()) % 16 == 0,
              op, ": w_hh must be contiguous, 16-byte aligned bf16");
  for (const auto& a : acts) check(*a.first, a.second, at::kBFloat16);
  check(cs, 1, at::kFloat);
  TORCH_CHECK(std::string(ols_lstm_route((int)B, (int)H, 1, 1)) == "fused",
              op, ": B = ", B, ", H = ", H, " is not a fused shape (1 <= B "
              "<= 16, H a multiple of 64 up to 256)");
  TORCH_CHECK(C * B * L * 4 * H < (int64_t(1) << 40) && C < (1 << 24), op,
              ": problem too large");
  return {(int)C, (int)B, (int)L, (int)H};
}

void lstm_fwd(at::Tensor xp, at::Tensor w_hh, at::Tensor hs, at::Tensor gates,
              at::Tensor cs) {
  const LstmDims d =
      lstm_dims("lstm_fwd", w_hh, {{&xp, 4}, {&hs, 1}, {&gates, 4}}, cs);
  auto wpack = at::empty_like(w_hh);
  const int rc = ols_lstm_fwd(xp.data_ptr(), w_hh.data_ptr(),
                              wpack.data_ptr(), hs.data_ptr(),
                              gates.data_ptr(), cs.data_ptr<float>(), d.C,
                              d.B, d.L, d.H,
                              at::cuda::getCurrentCUDAStream().stream());
  TORCH_CHECK(rc == 0, "lstm_fwd: launcher refused the operands");
}

void lstm_bwd(at::Tensor dhs, at::Tensor gates, at::Tensor cs,
              at::Tensor w_hh, at::Tensor dgates) {
  const LstmDims d =
      lstm_dims("lstm_bwd", w_hh, {{&dhs, 1}, {&gates, 4}, {&dgates, 4}}, cs);
  const int rc = ols_lstm_bwd(dhs.data_ptr(), gates.data_ptr(),
                              cs.data_ptr<float>(), w_hh.data_ptr(),
                              dgates.data_ptr(), d.C, d.B, d.L, d.H,
                              at::cuda::getCurrentCUDAStream().stream());
  TORCH_CHECK(rc == 0, "lstm_bwd: launcher refused the operands");
}

// "fused" or "torch": the path a layer of batch B and hidden size H takes
// (lstm_route.h), given its dtype and whether every operand is contiguous
// and starts on a 16-byte boundary
std::string lstm_route(int64_t B, int64_t H, bool is_bf16, bool aligned) {
  TORCH_CHECK(B >= 0 && H >= 0 && B < (1 << 30) && H < (1 << 30),
              "lstm_route: B, H out of range");
  return ols_lstm_route((int)B, (int)H, is_bf16, aligned);
}

// ---- fused causal self-attention (attn.hip) --------------------------------
// qkv [C, B, L, 3H] as the qkv blinear packs it (q | k | v along 3H, each
// heads x HD), att and datt [C, B, L, H], lse [C*B, heads, L] fp32, dqkv
// like qkv.  The outputs are arguments so that a caller decides where they
// live.  Every operand is contiguous, on one GPU and on a 16-byte
// boundary, bf16 but for lse, and the shape is one attn_route() calls
// "fused": anything else is an error here, never a quiet detour.

struct AttnDims {
  int CB, L, heads, HD;
};

AttnDims attn_dims(const char* op, const at::Tensor& qkv, int64_t heads,
                   std::initializer_list<const at::Tensor*> like_qkv,
                   std::initializer_list<const at::Tensor*> like_att,
                   const at::Tensor& lse, bool long_seq = false) {
  TORCH_CHECK(qkv.is_cuda() && qkv.dim() == 4 && heads >= 1 &&
                  qkv.size(3) % (3 * heads) == 0,
              op, ": qkv must be a [C, B, L, 3*heads*HD] GPU tensor, got ",
              qkv.sizes(), " for ", heads, " heads");
  const int64_t C = qkv.size(0), B = qkv.size(1), L = qkv.size(2);
  const int64_t H = qkv.size(3) / 3, HD = H / heads;
  auto check = [&](const at::Tensor& t, at::ScalarType dt,
                   at::IntArrayRef shape) {
    TORCH_CHECK(t.is_cuda() && t.device() == qkv.device() &&
                    t.is_contiguous() && t.scalar_type() == dt &&
                    reinterpret_cast<uintptr_t>(t.data_ptr()) % 16 == 0,
                op, ": operands must be contiguous, 16-byte aligned, on "
                "qkv's GPU, bf16 (lse: fp32)");
    TORCH_CHECK(t.sizes() == shape, op, ": operand is ", t.sizes(),
                ", expected ", shape);
  };
  for (const at::Tensor* t : like_qkv) check(*t, at::kBFloat16, {C, B, L, 3 * H});
  for (const at::Tensor* t : like_att) check(*t, at::kBFloat16, {C, B, L, H});
  check(lse, at::kFloat, {C * B, heads, L});
  TORCH_CHECK(L < (1 << 30) && HD < (1 << 30), op, ": L, HD out of range");
  if (long_seq) {
    TORCH_CHECK(std::string(ols_attn_long_route((int)L, (int)HD, 1, 1)) ==
                    "long",
                op, ": L = ", L, ", HD = ", HD, " is not a long shape (129 <= "
                "L <= 512, HD 32 or 64)");
  } else {
    TORCH_CHECK(std::string(ols_attn_route((int)L, (int)HD, 1, 1)) == "fused",
                op, ": L = ", L, ", HD = ", HD, " is not a fused shape (1 <= "
                "L <= 128, HD 32 or 64)");
  }
  TORCH_CHECK(C * B * heads < (int64_t(1) << 31) &&
                  C * B * L * 3 * H < (int64_t(1) << 40),
              op, ": problem too large");
  return {(int)(C * B), (int)L, (int)heads, (int)HD};
}

void attn_fwd(at::Tensor qkv, at::Tensor att, at::Tensor lse, int64_t heads) {
  const AttnDims d = attn_dims("attn_fwd", qkv, heads, {&qkv}, {&att}, lse);
  const int rc = ols_attn_fwd(qkv.data_ptr(), att.data_ptr(),
                              lse.data_ptr<float>(), d.CB, d.L, d.heads, d.HD,
                              at::cuda::getCurrentCUDAStream().stream());
  TORCH_CHECK(rc == 0, "attn_fwd: launcher refused the operands");
}

void attn_bwd(at::Tensor qkv, at::Tensor att, at::Tensor datt, at::Tensor lse,
              at::Tensor dqkv, int64_t heads) {
  const AttnDims d =
      attn_dims("attn_bwd", qkv, heads, {&qkv, &dqkv}, {&att, &datt}, lse);
  const int rc = ols_attn_bwd(qkv.data_ptr(), att.data_ptr(), datt.data_ptr(),
                              lse.data_ptr<float>(), dqkv.data_ptr(), d.CB,
                              d.L, d.heads, d.HD,
                              at::cuda::getCurrentCUDAStream().stream());
  TORCH_CHECK(rc == 0, "attn_bwd: launcher refused the operands");
}

// "fused" or "torch": the path a layer of sequence length L and head size
// HD takes (attn_route.h), given its dtype and whether every operand is
// contiguous and starts on a 16-byte boundary
std::string attn_route(int64_t L, int64_t HD, bool is_bf16, bool aligned) {
  TORCH_CHECK(L >= 0 && HD >= 0 && L < (1 << 30) && HD < (1 << 30),
              "attn_route: L, HD out of range");
  return ols_attn_route((int)L, (int)HD, is_bf16, aligned);
}

// ---- the same for 129 <= L <= 512 (attn_long.hip) --------------------------
// Operands and checks as above; dsum [C*B, heads, L] fp32, shaped like lse,
// is the backward's scratch for dO_i . O_i.

void attn_long_fwd(at::Tensor qkv, at::Tensor att, at::Tensor lse,
                   int64_t heads) {
  const AttnDims d =
      attn_dims("attn_long_fwd", qkv, heads, {&qkv}, {&att}, lse, true);
  const int rc = ols_attn_long_fwd(qkv.data_ptr(), att.data_ptr(),
                                   lse.data_ptr<float>(), d.CB, d.L, d.heads,
                                   d.HD,
                                   at::cuda::getCurrentCUDAStream().stream());
  TORCH_CHECK(rc == 0, "attn_long_fwd: launcher refused the operands");
}

void attn_long_bwd(at::Tensor qkv, at::Tensor att, at::Tensor datt,
                   at::Tensor lse, at::Tensor dsum, at::Tensor dqkv,
                   int64_t heads) {
  const AttnDims d = attn_dims("attn_long_bwd", qkv, heads, {&qkv, &dqkv},
                               {&att, &datt}, lse, true);
  attn_dims("attn_long_bwd", qkv, heads, {}, {}, dsum, true);
  const int rc = ols_attn_long_bwd(
      qkv.data_ptr(), att.data_ptr(), datt.data_ptr(), lse.data_ptr<float>(),
      dsum.data_ptr<float>(), dqkv.data_ptr(), d.CB, d.L, d.heads, d.HD,
      at::cuda::getCurrentCUDAStream().stream());
  TORCH_CHECK(rc == 0, "attn_long_bwd: launcher refused the operands");
}

std::string attn_long_route(int64_t L, int64_t HD, bool is_bf16,
                            bool aligned) {
  TORCH_CHECK(L >= 0 && HD >= 0 && L < (1 << 30) && HD < (1 << 30),
              "attn_long_route: L, HD out of range");
  return ols_attn_long_route((int)L, (int)HD, is_bf16, aligned);
}

// ---- tied-head cross-entropy between the GEMMs (head_ce.hip) ---------------
// One vocab slice [s0, s0 + s): logits [C, N, s] as the bmm wrote it, bias
// [C, V] with unit column stride and any client stride (0 for an expanded
// 1-D bias), labels [C, N] int64, the per-row state m, l, zy [C, N] fp32.
// The tile is bf16, contiguous and on a 16-byte boundary, everything is on
// one GPU, and the slice lies inside V: anything else is an error here,
// never a quiet detour.

struct HeadCeDims {
  int C, N, s;
  int64_t V, bias_stride;
};

HeadCeDims head_ce_dims(const char* op, const at::Tensor& logits,
                        const at::Tensor& bias, const at::Tensor& labels,
                        int64_t s0,
                        std::initializer_list<const at::Tensor*> state) {
  TORCH_CHECK(logits.is_cuda() && logits.dim() == 3 &&
                  logits.scalar_type() == at::kBFloat16 &&
                  logits.is_contiguous(),
              op, ": logits must be a contiguous bf16 [C, N, s] GPU tensor, "
              "got ", logits.sizes());
  const int64_t C = logits.size(0), N = logits.size(1), s = logits.size(2);
  TORCH_CHECK(C >= 1 && C <= 65535 && N >= 1 && N < (int64_t(1) << 31) &&
                  s >= 1 && s < (int64_t(1) << 30),
              op, ": C = ", C, ", N = ", N, ", s = ", s, " out of range");
  const bool aligned =
      reinterpret_cast<uintptr_t>(logits.data_ptr()) % 16 == 0;
  TORCH_CHECK(std::string(ols_head_ce_route(s, 1, aligned)) != "torch", op,
              ": logits must start on a 16-byte boundary");
  TORCH_CHECK(bias.is_cuda() && bias.device() == logits.device() &&
                  bias.dim() == 2 && bias.size(0) == C &&
                  bias.scalar_type() == at::kBFloat16 &&
                  (bias.size(1) == 1 || bias.stride(1) == 1) &&
                  bias.stride(0) >= 0,
              op, ": bias must be a bf16 [C, V] tensor on the logits' GPU "
              "with unit column stride, got ", bias.sizes());
  const int64_t V = bias.size(1);
  TORCH_CHECK(s0 >= 0 && s0 + s <= V, op, ": slice [", s0, ", ", s0 + s,
              ") is outside V = ", V);
  auto rows = [&](const at::Tensor& t, at::ScalarType dt, const char* what) {
    TORCH_CHECK(t.is_cuda() && t.device() == logits.device() &&
                    t.is_contiguous() && t.scalar_type() == dt &&
                    t.sizes() == at::IntArrayRef({C, N}),
                op, ": ", what, " must be contiguous [C, N] on the logits' "
                "GPU (labels int64, m, l, zy fp32), got ", t.sizes());
  };
  rows(labels, at::kLong, "labels");
  for (const at::Tensor* t : state) rows(*t, at::kFloat, "m, l, zy");
  return {(int)C, (int)N, (int)s, V, bias.stride(0)};
}

// m, l, zy <- the online-softmax merge of this slice into them
void head_ce_stats(at::Tensor logits, at::Tensor bias, at::Tensor labels,
                   int64_t s0, at::Tensor m, at::Tensor l, at::Tensor zy) {
  const HeadCeDims d =
      head_ce_dims("head_ce_stats", logits, bias, labels, s0, {&m, &l, &zy});
  const int rc = ols_head_ce_stats(
      logits.data_ptr(), bias.data_ptr(), d.bias_stride,
      labels.data_ptr<int64_t>(), m.data_ptr<float>(), l.data_ptr<float>(),
      zy.data_ptr<float>(), d.C, d.N, d.s, s0,
      at::cuda::getCurrentCUDAStream().stream());
  TORCH_CHECK(rc == 0, "head_ce_stats: launcher refused the operands");
}

// out <- bf16(g * (exp(z - m - log l) - onehot)), dbias[:, s0 : s0 + s] <-
// its column sums.  out MAY BE logits ITSELF: every thread reads its own
// elements before it writes them.  Any other overlap of the two is refused.
void head_ce_grad(at::Tensor logits, at::Tensor bias, at::Tensor labels,
                  int64_t s0, at::Tensor m, at::Tensor l, at::Tensor g,
                  at::Tensor dbias, at::Tensor out) {
  const HeadCeDims d =
      head_ce_dims("head_ce_grad", logits, bias, labels, s0, {&m, &l});
  TORCH_CHECK(out.is_cuda() && out.device() == logits.device() &&
                  out.scalar_type() == at::kBFloat16 && out.is_contiguous() &&
                  out.sizes() == logits.sizes() &&
                  reinterpret_cast<uintptr_t>(out.data_ptr()) % 16 == 0,
              "head_ce_grad: out must be like logits: contiguous bf16 on a "
              "16-byte boundary");
  const char* lo = static_cast<const char*>(logits.data_ptr());
  const char* oo = static_cast<const char*>(out.data_ptr());
  const int64_t nbytes = logits.numel() * 2;
  TORCH_CHECK(oo == lo || oo + nbytes <= lo || lo + nbytes <= oo,
              "head_ce_grad: out must be logits itself or not overlap it");
  TORCH_CHECK(g.is_cuda() && g.device() == logits.device() &&
                  g.scalar_type() == at::kFloat && g.numel() == 1,
              "head_ce_grad: g must be one fp32 element on the logits' GPU");
  TORCH_CHECK(dbias.is_cuda() && dbias.device() == logits.device() &&
                  dbias.scalar_type() == at::kBFloat16 &&
                  dbias.is_contiguous() &&
                  dbias.sizes() == at::IntArrayRef({d.C, d.V}),
              "head_ce_grad: dbias must be contiguous bf16 [C, V], got ",
              dbias.sizes());
  const int rc = ols_head_ce_grad(
      logits.data_ptr(), out.data_ptr(), bias.data_ptr(), d.bias_stride,
      labels.data_ptr<int64_t>(), m.data_ptr<float>(), l.data_ptr<float>(),
      g.data_ptr<float>(), dbias.data_ptr(), d.V, d.C, d.N, d.s, s0,
      at::cuda::getCurrentCUDAStream().stream());
  TORCH_CHECK(rc == 0, "head_ce_grad: launcher refused the operands");
}

// "fused8", "fused2", "fused1" or "torch": the path a slice of s columns
// takes (head_ce_route.h), given the tile's dtype and whether it is
// contiguous and starts on a 16-byte boundary
std::string head_ce_route(int64_t s, bool is_bf16, bool aligned) {
  TORCH_CHECK(s >= 0, "head_ce_route: s >= 0");
  return ols_head_ce_route(s, is_bf16, aligned);
}

// ---- bias + GELU, bias + residual + LayerNorm (dense_epi.hip) --------------
// Row operands (z, res, dy and every row output) are contiguous bf16
// [C, N, W] on one GPU and on 16-byte boundaries, column operands (b, gamma,
// beta) contiguous bf16 [C, W] likewise, mean and rstd fp32 [C, N]; the
// width passes dense_epi_route.h.  Anything else is an error here, never a
// quiet detour.  Outputs are passed in.

struct DenseEpiDims {
  int C, N, W;
};

DenseEpiDims dense_epi_dims(const char* op, const at::Tensor& z,
                            bool layernorm,
                            std::initializer_list<const at::Tensor*> rows,
                            std::initializer_list<const at::Tensor*> cols,
                            std::initializer_list<const at::Tensor*> stats) {
  TORCH_CHECK(z.is_cuda() && z.dim() == 3, op,
              ": the first operand must be a [C, N, W] GPU tensor, got ",
              z.sizes());
  const int64_t C = z.size(0), N = z.size(1), W = z.size(2);
  TORCH_CHECK(C >= 1 && C <= 65535 && N >= 1 && N < (int64_t(1) << 31) &&
                  W >= 1 && W < (int64_t(1) << 30),
              op, ": C = ", C, ", N = ", N, ", W = ", W, " out of range");
  bool aligned = true;
  auto check = [&](const at::Tensor& t, at::IntArrayRef shape,
                   at::ScalarType dt, const char* what) {
    TORCH_CHECK(t.is_cuda() && t.device() == z.device() &&
                    t.scalar_type() == dt && t.is_contiguous() &&
                    t.sizes() == shape,
                op, ": ", what, " on the first operand's GPU expected, got ",
                t.sizes());
    aligned = aligned && reinterpret_cast<uintptr_t>(t.data_ptr()) % 16 == 0;
  };
  for (const at::Tensor* t : rows)
    check(*t, {C, N, W}, at::kBFloat16, "a contiguous bf16 [C, N, W] tensor");
  for (const at::Tensor* t : cols)
    check(*t, {C, W}, at::kBFloat16, "a contiguous bf16 [C, W] tensor");
  for (const at::Tensor* t : stats)
    check(*t, {C, N}, at::kFloat, "a contiguous fp32 [C, N] tensor");
  TORCH_CHECK(std::string(ols_dense_epi_route(W, 1, aligned, layernorm)) !=
                  "torch",
              op, ": width ", W, " or an operand off a 16-byte boundary is "
              "not served (dense_epi_route)");
  return {(int)C, (int)N, (int)W};
}

// fp32 scratch [C, row_blocks, K, W] and its reduction into cols [K, C, W]
at::Tensor dense_epi_scratch(const at::Tensor& z, const DenseEpiDims& d,
                             int64_t row_block, int K) {
  TORCH_CHECK(row_block >= 1 && row_block <= 1024, "row_block in 1..1024");
  return at::empty({d.C, ols_dense_epi_row_blocks(d.N, (int)row_block), K,
                    d.W},
                   z.options().dtype(at::kFloat));
}

void dense_epi_finish(const char* op, const at::Tensor& part,
                      const at::Tensor& cols, const DenseEpiDims& d, int K) {
  TORCH_CHECK(cols.is_cuda() && cols.device() == part.device() &&
                  cols.scalar_type() == at::kBFloat16 &&
                  cols.is_contiguous() &&
                  cols.sizes() == at::IntArrayRef({K, d.C, d.W}),
              op, ": the column sums must be contiguous bf16 [", K,
              ", C, W], got ", cols.sizes());
  const int rc = ols_colsum_finish(
      part.data_ptr<float>(), cols.data_ptr(), d.C, (int)part.size(1), K, d.W,
      at::cuda::getCurrentCUDAStream().stream());
  TORCH_CHECK(rc == 0, op, ": colsum_finish refused the operands");
}

// y <- bf16(gelu(z + b)), erf form
void bias_gelu_fwd(at::Tensor z, at::Tensor b, at::Tensor y,
                   int64_t row_block) {
  const DenseEpiDims d =
      dense_epi_dims("bias_gelu_fwd", z, false, {&z, &y}, {&b}, {});
  TORCH_CHECK(row_block >= 1 && row_block <= 1024, "row_block in 1..1024");
  const int rc = ols_bias_gelu_fwd(
      z.data_ptr(), b.data_ptr(), y.data_ptr(), d.C, d.N, d.W, (int)row_block,
      at::cuda::getCurrentCUDAStream().stream());
  TORCH_CHECK(rc == 0, "bias_gelu_fwd: launcher refused the operands");
}

// dz <- bf16(dy * gelu'(z + b)), db [1, C, F] <- its column sums over N
void bias_gelu_bwd(at::Tensor z, at::Tensor b, at::Tensor dy, at::Tensor dz,
                   at::Tensor db, int64_t row_block) {
  const DenseEpiDims d =
      dense_epi_dims("bias_gelu_bwd", z, false, {&z, &dy, &dz}, {&b}, {});
  at::Tensor part = dense_epi_scratch(z, d, row_block, 1);
  const int rc = ols_bias_gelu_bwd(
      z.data_ptr(), b.data_ptr(), dy.data_ptr(), dz.data_ptr(),
      part.data_ptr<float>(), d.C, d.N, d.W, (int)row_block,
      at::cuda::getCurrentCUDAStream().stream());
  TORCH_CHECK(rc == 0, "bias_gelu_bwd: launcher refused the operands");
  dense_epi_finish("bias_gelu_bwd", part, db, d, 1);
}

// s <- bf16(z + b + res), y <- LayerNorm(s) * gamma + beta, mean, rstd of s
void brln_fwd(at::Tensor z, at::Tensor b, at::Tensor res, at::Tensor gamma,
              at::Tensor beta, double eps, at::Tensor y, at::Tensor s,
              at::Tensor mean, at::Tensor rstd) {
  const DenseEpiDims d =
      dense_epi_dims("brln_fwd", z, true, {&z, &res, &y, &s},
                     {&b, &gamma, &beta}, {&mean, &rstd});
  const int rc = ols_brln_fwd(
      z.data_ptr(), b.data_ptr(), res.data_ptr(), gamma.data_ptr(),
      beta.data_ptr(), y.data_ptr(), s.data_ptr(), mean.data_ptr<float>(),
      rstd.data_ptr<float>(), d.C, d.N, d.W, (float)eps,
      at::cuda::getCurrentCUDAStream().stream());
  TORCH_CHECK(rc == 0, "brln_fwd: launcher refused the operands");
}

// ds <- the gradient of s; cols [3, C, H] <- dgamma, dbeta, db
void brln_bwd(at::Tensor s, at::Tensor dy, at::Tensor gamma, at::Tensor mean,
              at::Tensor rstd, at::Tensor ds, at::Tensor cols,
              int64_t row_block) {
  const DenseEpiDims d = dense_epi_dims("brln_bwd", s, true, {&s, &dy, &ds},
                                        {&gamma}, {&mean, &rstd});
  at::Tensor part = dense_epi_scratch(s, d, row_block, 3);
  const int rc = ols_brln_bwd(
      s.data_ptr(), dy.data_ptr(), gamma.data_ptr(), mean.data_ptr<float>(),
      rstd.data_ptr<float>(), ds.data_ptr(), part.data_ptr<float>(), d.C, d.N,
      d.W, (int)row_block, at::cuda::getCurrentCUDAStream().stream());
  TORCH_CHECK(rc == 0, "brln_bwd: launcher refused the operands");
  dense_epi_finish("brln_bwd", part, cols, d, 3);
}

// "fused" or "torch": the path a row width takes (dense_epi_route.h), given
// the dtype and whether every operand is contiguous and on a 16-byte boundary
std::string dense_epi_route(int64_t width, bool is_bf16, bool aligned,
                            bool layernorm) {
  TORCH_CHECK(width >= 0, "dense_epi_route: width >= 0");
  return ols_dense_epi_route(width, is_bf16, aligned, layernorm);
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
  m.def("lstm_fwd(Tensor xp, Tensor w_hh, Tensor(a!) hs, Tensor(b!) gates, "
        "Tensor(c!) cs) -> ()");
  m.def("lstm_bwd(Tensor dhs, Tensor gates, Tensor cs, Tensor w_hh, "
        "Tensor(a!) dgates) -> ()");
  m.def("lstm_route(int B, int H, bool is_bf16, bool aligned) -> str",
        &lstm_route);
  m.def("attn_fwd(Tensor qkv, Tensor(a!) att, Tensor(b!) lse, int heads) -> ()");
  m.def("attn_bwd(Tensor qkv, Tensor att, Tensor datt, Tensor lse, "
        "Tensor(a!) dqkv, int heads) -> ()");
  m.def("attn_route(int L, int HD, bool is_bf16, bool aligned) -> str",
        &attn_route);
  m.def("attn_long_fwd(Tensor qkv, Tensor(a!) att, Tensor(b!) lse, int heads) "
        "-> ()");
  m.def("attn_long_bwd(Tensor qkv, Tensor att, Tensor datt, Tensor lse, "
        "Tensor(a!) dsum, Tensor(b!) dqkv, int heads) -> ()");
  m.def("attn_long_route(int L, int HD, bool is_bf16, bool aligned) -> str",
        &attn_long_route);
  m.def("head_ce_stats(Tensor logits, Tensor bias, Tensor labels, int s0, "
        "Tensor(a!) m, Tensor(b!) l, Tensor(c!) zy) -> ()");
  m.def("head_ce_grad(Tensor logits, Tensor bias, Tensor labels, int s0, "
        "Tensor m, Tensor l, Tensor g, Tensor(a!) dbias, Tensor(b!) out) "
        "-> ()");
  m.def("head_ce_route(int s, bool is_bf16, bool aligned) -> str",
        &head_ce_route);
  m.def("bias_gelu_fwd(Tensor z, Tensor b, Tensor(a!) y, int row_block) "
        "-> ()");
  m.def("bias_gelu_bwd(Tensor z, Tensor b, Tensor dy, Tensor(a!) dz, "
        "Tensor(b!) db, int row_block) -> ()");
  m.def("brln_fwd(Tensor z, Tensor b, Tensor res, Tensor gamma, Tensor beta, "
        "float eps, Tensor(a!) y, Tensor(b!) s, Tensor(c!) mean, "
        "Tensor(d!) rstd) -> ()");
  m.def("brln_bwd(Tensor s, Tensor dy, Tensor gamma, Tensor mean, "
        "Tensor rstd, Tensor(a!) ds, Tensor(b!) cols, int row_block) -> ()");
  m.def("dense_epi_route(int width, bool is_bf16, bool aligned, "
        "bool layernorm) -> str", &dense_epi_route);
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
  m.impl("lstm_fwd", &lstm_fwd);
  m.impl("lstm_bwd", &lstm_bwd);
  m.impl("attn_fwd", &attn_fwd);
  m.impl("attn_bwd", &attn_bwd);
  m.impl("attn_long_fwd", &attn_long_fwd);
  m.impl("attn_long_bwd", &attn_long_bwd);
  m.impl("head_ce_stats", &head_ce_stats);
  m.impl("head_ce_grad", &head_ce_grad);
  m.impl("bias_gelu_fwd", &bias_gelu_fwd);
  m.impl("bias_gelu_bwd", &bias_gelu_bwd);
  m.impl("brln_fwd", &brln_fwd);
  m.impl("brln_bwd", &brln_bwd);
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
