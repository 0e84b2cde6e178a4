// Which quantised-accumulate kernel one launch runs, and the constants of
// the uplink quantiser that the host and the device share.  The launcher
// in uplink_quant.hip switches on the result and the binding's
// delta_accum_quant_route() reports its name, so a test can assert the
// kernel an operand reaches.  Plain C++ on ints: no HIP types, compiles
// on any host.
#pragma once

#include <cstdint>

// elements per quantisation bucket, counted from a tensor's element 0
#define UPLINK_BUCKET 512
// clients per grid-y tile once clients >= UPLINK_CTILE; below that one
// tile holds them all and the launch is deterministic
#define UPLINK_CTILE 64

#define UPLINK_ROUTES(X) X(V8, "v8") X(SCALAR, "scalar")

enum UplinkRoute {
#define X(id, name) UPLINK_##id,
  UPLINK_ROUTES(X)
#undef X
};

static inline const char* uplink_route_name(UplinkRoute r) {
  static const char* const names[] = {
#define X(id, name) name,
      UPLINK_ROUTES(X)
#undef X
  };
  return names[r];
}

// n master elements, dtype 0 fp32 / 1 bf16 / 2 fp16.  The v8 kernel gives
// every lane 8 consecutive elements and reads them from master and from
// each replica row (row length n) as 16-byte packs: n must be a multiple
// of 8 and both base addresses multiples of 16.  The engine's master is a
// view into the flat cast at any element offset, so an operand that is
// not goes to the scalar kernel, which takes any n and any alignment.
// clients does not pick the kernel, only its grid (client tiles on y).
static inline UplinkRoute uplink_quant_route(int64_t n, int64_t clients,
                                             int dtype, bool master_16b,
                                             bool buf_16b) {
  (void)clients;
  (void)dtype;
  return n % 8 == 0 && master_16b && buf_16b ? UPLINK_V8 : UPLINK_SCALAR;
}

static inline int64_t uplink_client_tiles(int64_t clients) {
  return clients >= UPLINK_CTILE ? (clients + UPLINK_CTILE - 1) / UPLINK_CTILE
                                 : 1;
}

// levels per sign for b bits per weight, 0 for an unsupported b
static inline int uplink_levels(int bits) {
  return bits == 2 || bits == 4 || bits == 8 ? (1 << (bits - 1)) - 1 : 0;
}
