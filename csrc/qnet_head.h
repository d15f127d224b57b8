// The output MFMA of the 2x128 Q-net kernels (csrc/qnet_common.h) on one 16-row tile, as statements: the server
// (qserve.hip) and the backtest (qrollout.hip) include this at the top of their output phase, inside `if (wave <
// NET)`, run by the whole wave; under their lane test they then call q_head_row (qnet_common.h) for the row's Q
// values and greedy action.  Included in place and not a function: with the MFMA in a force-inlined function the
// backtest's output phase compiled to another instruction stream and its launch was 0.8 % slower
// (profiles/qnet_shared_forward.md); included, with the row arithmetic a function, all three kernels compile to
// what they were when each carried a copy.  No `#pragma once`: plain statements.
// In scope at the point of inclusion: aW2 (qnet_weights.h); sH2 [.][SH], layer 2's activations, complete; wave
// (= the 16-row tile this wave takes), l16, g4.
// Declares: acc.  Lanes g4 == 0 hold the first four (padded) outputs of row 16 wave + l16, before b2.

      f4v acc = zero4();
#pragma unroll
      for (int ks = 0; ks < KS1; ++ks)
        acc = mfma32(aW2[ks], lds_ld8(sH2 + (16 * wave + l16) * SH + ks * 32 + 8 * g4), acc);
