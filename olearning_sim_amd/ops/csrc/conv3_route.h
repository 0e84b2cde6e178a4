// Which conv3x3 kernel, with which template arguments, a shape runs.
// One function per family and direction; the launchers in client_conv.hip
// and client_conv2.hip switch on the result and the binding's
// conv3x3_route() reports its name, so a test can assert the kernel a
// shape reaches.  Plain C++ on ints: no HIP types, compiles on any host.
#pragma once

#include <cstdlib>
#include <cstring>

// name<template arguments> as conv3x3_route() spells it.  fwd_v6/v7
// carry <LG_OW, STRIDE>, dgrad_v6/v7 <LG_OW>, dgrad_s2 <LG_OW> (its four
// parity-class launches share it), fwd_v5 <ROW_HOIST>, dgrad_v5 <STRIDE>.
#define CONV3_ROUTES(X)                                                     \
  X(FWD_V2, "fwd_v2")                                                       \
  X(FWD_V5_TRUE, "fwd_v5<true>") X(FWD_V5_FALSE, "fwd_v5<false>")           \
  X(DGRAD_GENERIC, "dgrad_generic")                                         \
  X(DGRAD_V5_1, "dgrad_v5<1>") X(DGRAD_V5_2, "dgrad_v5<2>")                 \
  X(WGRAD_GENERIC, "wgrad_generic") X(WGRAD_V5, "wgrad_v5")                 \
  X(FWD_V6_2_1, "fwd_v6<2,1>") X(FWD_V6_3_1, "fwd_v6<3,1>")                 \
  X(FWD_V6_4_1, "fwd_v6<4,1>") X(FWD_V6_2_2, "fwd_v6<2,2>")                 \
  X(FWD_V6_3_2, "fwd_v6<3,2>") X(FWD_V6_4_2, "fwd_v6<4,2>")                 \
  X(FWD_V7_3_1, "fwd_v7<3,1>") X(FWD_V7_4_1, "fwd_v7<4,1>")                 \
  X(FWD_V7_5_1, "fwd_v7<5,1>")                                              \
  X(DGRAD_V6_2, "dgrad_v6<2>") X(DGRAD_V6_3, "dgrad_v6<3>")                 \
  X(DGRAD_V6_4, "dgrad_v6<4>")                                              \
  X(DGRAD_V7_2, "dgrad_v7<2>") X(DGRAD_V7_3, "dgrad_v7<3>")                 \
  X(DGRAD_V7_4, "dgrad_v7<4>") X(DGRAD_V7_5, "dgrad_v7<5>")                 \
  X(DGRAD_S2_2, "dgrad_s2<2>") X(DGRAD_S2_3, "dgrad_s2<3>")                 \
  X(DGRAD_S2_4, "dgrad_s2<4>")                                              \
  X(WGRAD_V6, "wgrad_v6") X(WGRAD_V7, "wgrad_v7")                           \
  X(WGRAD_V8, "wgrad_v8") X(WGRAD_V8S, "wgrad_v8s")

enum Conv3Route {
#define X(id, name) CV3_##id,
  CONV3_ROUTES(X)
#undef X
};

static inline const char* conv3_route_name(Conv3Route r) {
  static const char* const names[] = {
#define X(id, name) name,
      CONV3_ROUTES(X)
#undef X
  };
  return names[r];
}

// The five A/B switches, read on every call.  OLSIM_CONV_V=5 sends every
// shape to the v5 family; the other four act on presence, whatever the
// value (OLSIM_CONV_DW8=0 restores the scalar wgrad gather because it is
// set): OLSIM_CONV_DW64 the BK=64 dgrad_v7 / wgrad_v7,
// OLSIM_CONV_DW8 no run-vectorised wgrad_v8 / v8s,
// OLSIM_CONV_NMAJOR the [n][k] B tile in every fwd / dgrad kernel,
// OLSIM_CONV_BM64 the 64x128 block tile in every forward kernel.
struct Conv3Env {
  bool v5, dw64, no_dw8, nmajor, bm64;
};

static inline Conv3Env conv3_env() {
  const char* v = getenv("OLSIM_CONV_V");
  return {v != nullptr && strcmp(v, "5") == 0,
          getenv("OLSIM_CONV_DW64") != nullptr,
          getenv("OLSIM_CONV_DW8") != nullptr,
          getenv("OLSIM_CONV_NMAJOR") != nullptr,
          getenv("OLSIM_CONV_BM64") != nullptr};
}

static inline int conv3_cdiv(int a, int b) { return (a + b - 1) / b; }
static inline bool conv3_is_p2(int v) { return v > 0 && (v & (v - 1)) == 0; }
static inline int conv3_lg(int v) {
  int l = 0;
  while ((1 << l) < v) ++l;
  return l;
}
// LG_OW template argument of a kernel instantiated for lo..hi
static inline int conv3_clamp(int v, int lo, int hi) {
  return v < lo ? lo : v > hi ? hi : v;
}

// ---- v5 family (client_conv.hip): any shape, dense operands ---------------

static inline Conv3Route conv3_route_fwd_v5(int IC, int OC, int B, int H,
                                            int W, int stride) {
  const int OH = conv3_cdiv(H, stride), OW = conv3_cdiv(W, stride);
  const bool v5_ok = conv3_is_p2(OW) && conv3_is_p2(OH) && (IC * 9) % 32 == 0;
  if (!v5_ok) return CV3_FWD_V2;
  // ROW_HOIST: a 16-column segment lies inside one output row
  return OW >= 16 ? CV3_FWD_V5_TRUE : CV3_FWD_V5_FALSE;
}

static inline Conv3Route conv3_route_dgrad_v5(int IC, int OC, int B, int H,
                                              int W, int stride) {
  const int OH = conv3_cdiv(H, stride), OW = conv3_cdiv(W, stride);
  // dgrad_v5 decomposes n with log2(W) = log2(OW * stride) and H == W:
  // an odd plane at stride 2 (OH = ceil(H/2)) takes the generic kernel
  const bool v5_ok = conv3_is_p2(OW) && conv3_is_p2(OH) && (OC * 9) % 32 == 0
                     && (stride == 1 || stride == 2) && H == W
                     && H == OH * stride;
  if (!v5_ok) return CV3_DGRAD_GENERIC;
  return stride == 1 ? CV3_DGRAD_V5_1 : CV3_DGRAD_V5_2;
}

static inline Conv3Route conv3_route_wgrad_v5(int IC, int OC, int B, int H,
                                              int W, int stride) {
  const int OH = conv3_cdiv(H, stride), OW = conv3_cdiv(W, stride);
  const bool v5_ok = conv3_is_p2(OW) && conv3_is_p2(OH)
                     && (B * OH * OW) % 32 == 0;
  return v5_ok ? CV3_WGRAD_V5 : CV3_WGRAD_GENERIC;
}

// ---- v6 family (client_conv2.hip): padded operands ------------------------

// true when the v6 padded path supports the shape (pow2 planes, K%32==0)
static inline bool conv3_v6_ok(int IC, int OC, int B, int H, int W,
                               int stride) {
  const int OH = conv3_cdiv(H, stride), OW = conv3_cdiv(W, stride);
  if (!conv3_is_p2(OH) || !conv3_is_p2(OW) || OW < 4) return false;
  // stride-2 dgrad scatters into a 2*OH x 2*OW dX plane: odd H or W
  // (7 -> 4) would index dy_pad and dx with the wrong plane sizes
  if (stride == 2 && ((H | W) & 1)) return false;
  if ((IC * 9) % 32 != 0) return false;             // fwd K
  if ((OC * 9) % 32 != 0) return false;             // dgrad K (s=1)
  if (stride == 2 && OC % 32 != 0) return false;    // smallest s2 class K=OC
  if (stride != 1 && stride != 2) return false;
  if ((B * OH * OW) % 32 != 0) return false;        // wgrad A-direct rows
  return true;
}

// The shapes below passed conv3_v6_ok: stride is 1 or 2, planes are pow2.

static inline Conv3Route conv3_route_fwd_v6(int IC, int OC, int B, int H,
                                            int W, int stride) {
  static const Conv3Route v6[2][3] = {
      {CV3_FWD_V6_2_1, CV3_FWD_V6_3_1, CV3_FWD_V6_4_1},
      {CV3_FWD_V6_2_2, CV3_FWD_V6_3_2, CV3_FWD_V6_4_2}};
  static const Conv3Route v7[3] = {CV3_FWD_V7_3_1, CV3_FWD_V7_4_1,
                                   CV3_FWD_V7_5_1};
  const int lg_ow = conv3_lg(conv3_cdiv(W, stride));
  // BK=64 (v7) wins +5..10% at OW >= 8 stride 1 (A/B at C=250); the
  // 4x4-plane deep layers and stride 2 measured flat-to-worse, so they
  // stay on BK=32.
  if ((IC * 9) % 64 == 0 && stride == 1 && lg_ow >= 3)
    return v7[conv3_clamp(lg_ow, 3, 5) - 3];
  return v6[stride != 1][conv3_clamp(lg_ow, 2, 4) - 2];
}

static inline Conv3Route conv3_route_dgrad_v6(int IC, int OC, int B, int H,
                                              int W, int stride) {
  static const Conv3Route v6[3] = {CV3_DGRAD_V6_2, CV3_DGRAD_V6_3,
                                   CV3_DGRAD_V6_4};
  static const Conv3Route v7[4] = {CV3_DGRAD_V7_2, CV3_DGRAD_V7_3,
                                   CV3_DGRAD_V7_4, CV3_DGRAD_V7_5};
  static const Conv3Route s2[3] = {CV3_DGRAD_S2_2, CV3_DGRAD_S2_3,
                                   CV3_DGRAD_S2_4};
  const int lg_ow = conv3_lg(conv3_cdiv(W, stride));
  // stride 2: four parity classes, each a dense GEMM over the dy plane
  if (stride != 1) return s2[conv3_clamp(lg_ow, 2, 4) - 2];
  if (conv3_env().dw64 && (OC * 9) % 64 == 0)
    return v7[conv3_clamp(lg_ow, 2, 5) - 2];
  return v6[conv3_clamp(lg_ow, 2, 4) - 2];
}

static inline Conv3Route conv3_route_wgrad_v6(int IC, int OC, int B, int H,
                                              int W, int stride) {
  const int OH = conv3_cdiv(H, stride), OW = conv3_cdiv(W, stride);
  const Conv3Env env = conv3_env();
  // run-vectorised producer (v8 / v8s): 8 consecutive q stay in one
  // padded row; OLSIM_CONV_DW8 restores the scalar gather
  if (OW >= 8 && !env.no_dw8)
    return stride == 1 ? CV3_WGRAD_V8 : CV3_WGRAD_V8S;
  if (env.dw64 && (B * OH * OW) % 64 == 0) return CV3_WGRAD_V7;
  return CV3_WGRAD_V6;
}

// B-tile staging of a v6-family fwd (dir 0) or dgrad (dir 1) route: true
// = k-major tile, 16-byte LDS stores and transposed fragment reads; false
// = the [n][k+pad] tile and 2-byte stores.  The kernel name and its
// <LG_OW, STRIDE> stay the route's; the staging is one more template
// argument.  Only the stride-1 fwd_v6 / fwd_v7 / dgrad_v6 kernels have the
// k-major form: at stride 2 a thread's columns are alternate elements,
// and dgrad_v7 is a record kept as it was measured.
// fwd_v7<3,1> (OW = 8, the 256-channel stage) stays [n][k]: k-major
// measured 1.3 % slower there (0.850 vs 0.839 ms at C=250,
// profiles/conv_kmajor_r06.md), so it has no k-major instantiation.
// Re-measured on the 128x64 tile, where it commits half as many 2-byte
// stores: 0.777 ms either way (profiles/conv_tile_r08.md), so still none.
static inline bool conv3_kmajor_v6(int dir, Conv3Route r) {
  if (conv3_env().nmajor) return false;
  if (dir == 0)
    return r == CV3_FWD_V6_2_1 || r == CV3_FWD_V6_3_1 || r == CV3_FWD_V6_4_1
           || r == CV3_FWD_V7_4_1 || r == CV3_FWD_V7_5_1;
  if (dir == 1)
    return r == CV3_DGRAD_V6_2 || r == CV3_DGRAD_V6_3 || r == CV3_DGRAD_V6_4;
  return false;
}

// Block tile of a v6-family forward route: 0 = 64x128 (four waves of 16
// rows x 128 columns), 1 = 128x64 (four waves of 32 rows x 64 columns, each
// B fragment read feeding two MFMAs, half the gather and half the B commits
// per MFMA).  Like the staging, one more template argument that the route
// name does not carry.  fwd_v6<*,1>, fwd_v6<*,2> and fwd_v7<*,1> take the
// taller tile when it adds no padded rows (OC = 96, 128, 256, 512 ...; not
// 64 or 192); the dgrad / wgrad kernels have the one tile.  The
// flipped-weight dgrad runs the forward of (OC, IC) and so gets that
// forward's tile.
// All nine instantiations measured faster on the taller tile (C=250, B=16,
// OLSIM_CONV_BM64 set against unset, profiles/conv_tile_r08.md): stride 2
// +30 %, fwd_v7<3,1> +7.2 %, fwd_v7<4,1> +4.7 %, fwd_v7<5,1> +3.8 %,
// fwd_v6<2,1> +2.9 %, fwd_v6<3,1> / <4,1> +16 / +5.5 % off the flagship;
// none is gated back.  Where it does not fit (OC = 64), the same 32x64
// wave tile as a 2x2 wave grid inside the 64x128 block measured 10-25 %
// slower (the two waves of a row pair load the same A) and is not built.
static inline int conv3_tile_v6(Conv3Route r, int OC) {
  if (conv3_env().bm64) return 0;
  if (conv3_cdiv(OC, 128) * 128 != conv3_cdiv(OC, 64) * 64) return 0;
  switch (r) {
    case CV3_FWD_V6_2_1: case CV3_FWD_V6_3_1: case CV3_FWD_V6_4_1:
    case CV3_FWD_V6_2_2: case CV3_FWD_V6_3_2: case CV3_FWD_V6_4_2:
    case CV3_FWD_V7_3_1: case CV3_FWD_V7_4_1: case CV3_FWD_V7_5_1:
      return 1;
    default:
      return 0;
  }
}

static inline const char* conv3_tile_name(int tile) {
  return tile == 1 ? "128x64" : "64x128";
}

// dir: 0 fwd, 1 dgrad, 2 wgrad.  Includes the family decision the Python
// dispatcher makes (ops/conv.py _v6_ok): v6 unless OLSIM_CONV_V=5 or the
// shape is outside conv3_v6_ok.
static inline Conv3Route conv3_route(int dir, int IC, int OC, int B, int H,
                                     int W, int stride) {
  const bool v6 = !conv3_env().v5 && conv3_v6_ok(IC, OC, B, H, W, stride);
  if (dir == 0)
    return v6 ? conv3_route_fwd_v6(IC, OC, B, H, W, stride)
              : conv3_route_fwd_v5(IC, OC, B, H, W, stride);
  if (dir == 1)
    return v6 ? conv3_route_dgrad_v6(IC, OC, B, H, W, stride)
              : conv3_route_dgrad_v5(IC, OC, B, H, W, stride);
  return v6 ? conv3_route_wgrad_v6(IC, OC, B, H, W, stride)
            : conv3_route_wgrad_v5(IC, OC, B, H, W, stride);
}

// staging of the kernel conv3_route() names for the shape (v5-family and
// wgrad routes have no k-major form)
static inline bool conv3_kmajor(int dir, int IC, int OC, int B, int H, int W,
                                int stride) {
  return conv3_kmajor_v6(dir, conv3_route(dir, IC, OC, B, H, W, stride));
}

// block tile of the kernel conv3_route() names for the shape
static inline int conv3_tile(int dir, int IC, int OC, int B, int H, int W,
                             int stride) {
  if (dir != 0) return 0;
  return conv3_tile_v6(conv3_route(dir, IC, OC, B, H, W, stride), OC);
}
