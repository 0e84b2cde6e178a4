// Which weighted-delta kernel one accumulate launch runs.  The launcher in
// aggregate.hip switches on the result and the binding's
// delta_accum_route() reports its name, so a test can assert the kernel
// an operand reaches.  Plain C++ on ints: no HIP types, compiles on any
// host.
#pragma once

#include <cstdint>

#define DELTA_ROUTES(X)                                                     \
  X(CPAR_S, "cpar_s") X(CPAR, "cpar") X(V8, "v8") X(BLOCK_TABLE, "block_table")

enum DeltaRoute {
#define X(id, name) DELTA_##id,
  DELTA_ROUTES(X)
#undef X
};

static inline const char* delta_route_name(DeltaRoute r) {
  static const char* const names[] = {
#define X(id, name) name,
      DELTA_ROUTES(X)
#undef X
  };
  return names[r];
}

// nblocks parameter blocks of n master elements in all, dtype 0 fp32 /
// 1 bf16 / 2 fp16.  k_delta_accum_v8 and k_delta_accum_cpar read master
// and every replica row (row length n, a multiple of 8) as 16-byte
// packs: both base addresses must be multiples of 16.  The engine's
// master is a view into the flat cast at any element offset, so an
// operand that is not goes to the scalar kernel of the same shape of
// grid: cpar -> cpar_s, v8 -> block_table.  Both take any n.
static inline DeltaRoute delta_accum_route(int nblocks, int64_t n,
                                           int64_t clients, int dtype,
                                           bool master_16b, bool buf_16b) {
  const bool single = nblocks == 1;
  const bool packs = n % 8 == 0 && master_16b && buf_16b;
  // small bf16 param at many clients: client-parallel tiles (fills the
  // chip; the j-only kernels would be a serial latency chain on a
  // handful of lanes)
  if (single && dtype == 1 && n < 131072 && clients >= 64)
    return packs ? DELTA_CPAR : DELTA_CPAR_S;
  if (single && dtype != 0 && packs) return DELTA_V8;
  return DELTA_BLOCK_TABLE;
}
