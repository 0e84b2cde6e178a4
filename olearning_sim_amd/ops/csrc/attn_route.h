// Which path one layer's causal self-attention takes.  ops/attn.py asks the
// binding's attn_route() before every layer and the launchers in attn.hip
// refuse what this refuses, so a test can assert the path a shape reaches.
// Plain C++ on ints: no HIP types, compiles on any host.
#pragma once

enum AttnRoute { ATTN_FUSED, ATTN_TORCH, ATTN_LONG };

static inline const char* attn_route_name(AttnRoute r) {
  return r == ATTN_FUSED ? "fused" : r == ATTN_LONG ? "long" : "torch";
}

// k_attn_fwd / k_attn_bwd give one workgroup of four waves to one (client x
// batch row, head) pair and keep that head's whole sequence in LDS tiles of
// 128 rows: 1 <= L <= 128.  The head dimension is the K of the score MFMAs
// in chunks of 32 and a template argument: HD 32 or 64.  The kernels
// reinterpret every 2-byte operand as bf16 and move it in 16-byte packs of
// 8 along HD: bf16 only, every operand contiguous and on a 16-byte
// boundary (aligned).
static inline AttnRoute attn_route(int L, int HD, bool is_bf16, bool aligned) {
  return is_bf16 && aligned && L >= 1 && L <= 128 && (HD == 32 || HD == 64)
             ? ATTN_FUSED
             : ATTN_TORCH;
}

// k_attn_long_fwd / k_attn_long_bwd (attn_long.hip) cut the sequence into
// blocks of 128 rows, give a workgroup one block and stream the others
// through the same LDS tiles: 129 <= L <= 512, any value in between.  The
// upper end is where the kernels were measured and tested, not a limit of
// the scheme.  Everything else as above.  ops/attn.py asks this after
// attn_route() has said "torch".
static inline AttnRoute attn_long_route(int L, int HD, bool is_bf16,
                                        bool aligned) {
  return is_bf16 && aligned && L >= 129 && L <= 512 && (HD == 32 || HD == 64)
             ? ATTN_LONG
             : ATTN_TORCH;
}
