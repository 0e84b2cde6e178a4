// Which server-optimiser kernel one step launches.  The launcher in
// server_opt.hip switches on the result and the binding's
// server_opt_route() reports its name, so a test can assert the kernel an
// operand reaches.  Plain C++ on ints: no HIP types, compiles on any host.
#pragma once

#include <cstdint>

enum ServerOptKind {
  SOPT_MOMENTUM = 0,
  SOPT_ADAGRAD = 1,
  SOPT_ADAM = 2,
  SOPT_YOGI = 3,
  SOPT_KINDS = 4
};

enum ServerOptRoute { SOPT_V4, SOPT_SCALAR };

static inline const char* server_opt_route_name(ServerOptRoute r) {
  return r == SOPT_V4 ? "v4" : "scalar";
}

// k_server_opt_v4 reads x, d, m, v and z as 16-byte packs of four floats:
// every operand of the step must start on a 16-byte boundary (aligned)
// and there must be one whole pack at least.  The engine's tensors are
// whole allocations, but a caller may hand in a view at any element
// offset; that goes to the scalar kernel, which takes any n.
static inline ServerOptRoute server_opt_route(int64_t n, bool aligned) {
  return n >= 4 && aligned ? SOPT_V4 : SOPT_SCALAR;
}
