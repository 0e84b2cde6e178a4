// Which path one vocab slice of the tied-head cross-entropy takes between
// its GEMMs.  ops/head_ce.py asks the binding's head_ce_route() for every
// slice and the launchers in head_ce.hip refuse what this refuses, so a test
// can assert the path a slice width reaches.  Plain C++ on ints: no HIP
// types, compiles on any host.
#pragma once

enum HeadCeRoute { HEAD_CE_FUSED8, HEAD_CE_FUSED2, HEAD_CE_FUSED1,
                   HEAD_CE_TORCH };

static inline const char* head_ce_route_name(HeadCeRoute r) {
  return r == HEAD_CE_FUSED8   ? "fused8"
         : r == HEAD_CE_FUSED2 ? "fused2"
         : r == HEAD_CE_FUSED1 ? "fused1"
                               : "torch";
}

// elements per lane and load (the kernels' VEC), 0 for the torch route
static inline int head_ce_vec(HeadCeRoute r) {
  return r == HEAD_CE_FUSED8 ? 8 : r == HEAD_CE_FUSED2 ? 2
         : r == HEAD_CE_FUSED1 ? 1 : 0;
}

// k_head_ce_stats / k_head_ce_grad read a bf16 tile [C, N, s] whose rows
// follow each other without padding, in packs of VEC elements.  The base is
// on a 16-byte boundary (aligned), so a row starts on a pack boundary when
// VEC divides s: 16-byte packs of 8 when s is a multiple of 8, 4-byte pairs
// when it is even, single elements otherwise.  fp32 tiles, tiles that are
// not contiguous or not aligned, and empty slices go to torch.
static inline HeadCeRoute head_ce_route(long long s, bool is_bf16,
                                        bool aligned) {
  if (!is_bf16 || !aligned || s < 1) return HEAD_CE_TORCH;
  return s % 8 == 0 ? HEAD_CE_FUSED8 : s % 2 == 0 ? HEAD_CE_FUSED2
                                                  : HEAD_CE_FUSED1;
}
