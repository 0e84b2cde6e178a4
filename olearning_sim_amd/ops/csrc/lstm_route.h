// Which path one LSTM layer's recurrence takes.  ops/lstm.py asks the
// binding's lstm_route() before every layer and the launchers in lstm.hip
// refuse what this refuses, so a test can assert the path a shape reaches.
// Plain C++ on ints: no HIP types, compiles on any host.
#pragma once

enum LstmRoute { LSTM_FUSED, LSTM_TORCH };

static inline const char* lstm_route_name(LstmRoute r) {
  return r == LSTM_FUSED ? "fused" : "torch";
}

// k_lstm_fwd / k_lstm_bwd give one workgroup of four waves to one client.
// The batch is the M = 16 rows of one MFMA tile: 1 <= B <= 16.  Wave w
// owns hidden units [w*H/4, (w+1)*H/4) in column tiles of 16, so H must
// be a multiple of 4 * 16 = 64, and JT = H/64 tiles per gate; the forward
// keeps 4*JT accumulator tiles plus the cell state in registers, which
// JT <= 4 (H <= 256) bounds at 80 VGPRs.  The kernels reinterpret every
// 2-byte operand as bf16 and read the weights as 16-byte packs: bf16
// only, every operand contiguous and on a 16-byte boundary (aligned).
static inline LstmRoute lstm_route(int B, int H, bool is_bf16, bool aligned) {
  return is_bf16 && aligned && B >= 1 && B <= 16 && H >= 64 && H <= 256 &&
                 H % 64 == 0
             ? LSTM_FUSED
             : LSTM_TORCH;
}
