// The forward of the flagship 2x128 bf16 Q-net (224 -> 128 -> 128 -> 16, models/qnet.py) with every weight in
// VGPRs: the one definition that the batched server (qserve.hip) and the backtest (qrollout.hip) both run, so the
// two kernels cannot drift apart.  A wave owns MT 16-unit m-tiles of both hidden layers (hidden units m0 ..
// m0 + 16 MT - 1) plus the output-layer fragments; a workgroup works on NET 16-row tiles of activations in LDS
// (bf16, row strides SX / SH).  The callers keep their data movement: how the feature rows get into sX, their
// barrier, and what they do with a row's Q values and greedy action.
//
// Three pieces are statements that each kernel includes in place, not functions (why: see the files and
// profiles/qnet_shared_forward.md): qnet_weights.h, the weight prologue (declares aW0, aW1, aW2, bb, b2);
// qnet_layers.h, the two hidden layers (sX -> sH1 -> sH2); qnet_head.h, the output MFMA on the wave's 16-row tile
// (declares acc).  This file holds the constants they share and the row arithmetic of the Q head.
#pragma once
#include "common.h"
#include "trade_rule.h"   // argmax3

namespace st {
namespace qnet {

constexpr int INP = 224, HP = 128, OUTP = 16;   // padded dims of the flagship layout (W2 is [OUTP][HP]: 3 rows used)
constexpr int KS0 = INP / 32, KS1 = HP / 32;    // k-steps of v_mfma_f32_16x16x32_bf16
constexpr int SX = INP + 16, SH = HP + 16;      // activation row strides (bf16)

// the Q head of one row from the output MFMA's accumulator (qnet_head.h), on a lane g4 == 0: q[0..2] (+ b2, the
// output ReLU under reference_compat); returns the greedy action (first max, like TF ArgMax)
ST_DEV int q_head_row(f4v acc, const float (&b2)[3], int output_relu, float (&q)[3]) {
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    q[j] = acc[j] + b2[j];
    if (output_relu) q[j] = fmaxf(q[j], 0.f);
  }
  return argmax3(q[0], q[1], q[2]);
}

}  // namespace qnet
}  // namespace st
