// The two hidden layers of the 2x128 Q-net kernels (csrc/qnet_common.h) on the workgroup's NET 16-row tiles, as
// statements: the server (qserve.hip) includes this once per 64-row tile, the backtest (qrollout.hip) once per day.
// Included in place and not functions, for the reason given in qnet_weights.h (as function templates: 242 VGPRs
// against 219 in the register-gather server, that build and the backtest 1 % slower; profiles/qnet_shared_forward.md).
// No `#pragma once`: plain statements.
// In scope at the point of inclusion: aW0, aW1, bb (qnet_weights.h); MT, NET (constexpr); the LDS tiles sX [.][SX]
// (the feature rows, complete: a barrier went before), sH1 [.][SH] and sH2 [.][SH] (the callers put it over sX);
// m0, l16, g4; bar(), the caller's workgroup barrier.
// Leaves layer 2's activations in sH2, complete (the last statement is a bar()).

    // P1: layer 1 (the bias is the constant-1 input column) -> ReLU -> bf16 H1
    {
      f4v acc[MT][NET];
#pragma unroll
      for (int i = 0; i < MT; ++i)
#pragma unroll
        for (int n = 0; n < NET; ++n) acc[i][n] = zero4();
#pragma unroll
      for (int ks = 0; ks < KS0; ++ks) {
        s8v b[NET];
#pragma unroll
        for (int n = 0; n < NET; ++n) b[n] = lds_ld8(sX + (16 * n + l16) * SX + ks * 32 + 8 * g4);
#pragma unroll
        for (int i = 0; i < MT; ++i)
#pragma unroll
          for (int n = 0; n < NET; ++n) acc[i][n] = mfma32(aW0[i][ks], b[n], acc[i][n]);
      }
#pragma unroll
      for (int i = 0; i < MT; ++i)
#pragma unroll
        for (int n = 0; n < NET; ++n) {
          const f4v v = acc[i][n];
          lds_st4(sH1 + (16 * n + l16) * SH + m0 + 16 * i + 4 * g4, fmaxf(v[0], 0.f), fmaxf(v[1], 0.f),
                  fmaxf(v[2], 0.f), fmaxf(v[3], 0.f));
        }
    }
    bar();
    // P2: layer 2 + b1 -> ReLU -> bf16 H2 (over X)
    {
      f4v acc[MT][NET];
#pragma unroll
      for (int i = 0; i < MT; ++i)
#pragma unroll
        for (int n = 0; n < NET; ++n) acc[i][n] = zero4();
#pragma unroll
      for (int ks = 0; ks < KS1; ++ks) {
        s8v b[NET];
#pragma unroll
        for (int n = 0; n < NET; ++n) b[n] = lds_ld8(sH1 + (16 * n + l16) * SH + ks * 32 + 8 * g4);
#pragma unroll
        for (int i = 0; i < MT; ++i)
#pragma unroll
          for (int n = 0; n < NET; ++n) acc[i][n] = mfma32(aW1[i][ks], b[n], acc[i][n]);
      }
#pragma unroll
      for (int i = 0; i < MT; ++i)
#pragma unroll
        for (int n = 0; n < NET; ++n) {
          const f4v v = acc[i][n];
          lds_st4(sH2 + (16 * n + l16) * SH + m0 + 16 * i + 4 * g4, fmaxf(v[0] + bb[i][0], 0.f),
                  fmaxf(v[1] + bb[i][1], 0.f), fmaxf(v[2] + bb[i][2], 0.f), fmaxf(v[3] + bb[i][3], 0.f));
        }
    }
    bar();
