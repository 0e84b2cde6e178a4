// Which path the epilogue of one of BertLM's dense layers takes: the fused
// kernels of dense_epi.hip or the library.  ops/dense_epi.py asks the
// binding's dense_epi_route() before every call and the launchers in
// dense_epi.hip refuse what this refuses, so a test can assert the path a
// shape reaches.  Plain C++ on ints: no HIP types, compiles on any host.
#pragma once

enum DenseEpiRoute { DENSE_EPI_FUSED, DENSE_EPI_TORCH };

static inline const char* dense_epi_route_name(DenseEpiRoute r) {
  return r == DENSE_EPI_FUSED ? "fused" : "torch";
}

// the LayerNorm form keeps a whole row in one wave's registers: at most
// DENSE_EPI_LN_PACKS 16-byte packs of each operand per lane
#define DENSE_EPI_LN_PACKS 3
#define DENSE_EPI_LN_MAX_H (64 * 8 * DENSE_EPI_LN_PACKS)

// The kernels move bf16 rows of `width` elements in 16-byte packs of 8: the
// width is a multiple of 8, and every operand is contiguous and starts on a
// 16-byte boundary (aligned), so every pack of every row is whole.  With a
// residual (the LayerNorm form) the width is at most DENSE_EPI_LN_MAX_H.
// fp32, odd widths, strided or misaligned operands go to torch.
static inline DenseEpiRoute dense_epi_route(long long width, bool is_bf16,
                                            bool aligned, bool layernorm) {
  if (!is_bf16 || !aligned || width < 8 || width % 8 != 0 ||
      width >= (1LL << 30))
    return DENSE_EPI_TORCH;
  if (layernorm && width > DENSE_EPI_LN_MAX_H) return DENSE_EPI_TORCH;
  return DENSE_EPI_FUSED;
}
