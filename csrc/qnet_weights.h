// The weight prologue of the 2x128 Q-net kernels (csrc/qnet_common.h), as statements: the server (qserve.hip) and the
// backtest (qrollout.hip) include this once, before their tile loop.  Included in place and not a function: as a
// force-inlined function template the weights' loads were scheduled and their registers assigned differently, and
// with the layers as functions too the register-gather server and the backtest ran 1 % slower
// (profiles/qnet_shared_forward.md); included, the kernels compile to what they were when each carried a copy.  No
// `#pragma once`: plain statements.
// In scope at the point of inclusion: p with wq, wf and the off_* of the engine layout; MT (16-unit m-tiles per
// wave, constexpr); m0 (the wave's first hidden unit), l16, g4.
// Declares: aW0, aW1 (A fragments of this wave's m-tiles, MT x (7 + 4) k-steps), aW2 (the output layer's, 4
// k-steps), bb (b1 of the accumulator rows this lane holds), b2.

  s8v aW0[MT][KS0], aW1[MT][KS1], aW2[KS1];
#pragma unroll
  for (int i = 0; i < MT; ++i) {
    const bf16_t* w0 = p.wq + p.off_w0 + (size_t)(m0 + 16 * i + l16) * INP + 8 * g4;
#pragma unroll
    for (int ks = 0; ks < KS0; ++ks) aW0[i][ks] = *reinterpret_cast<const s8v*>(w0 + ks * 32);
    const bf16_t* w1 = p.wq + p.off_w1 + (size_t)(m0 + 16 * i + l16) * HP + 8 * g4;
#pragma unroll
    for (int ks = 0; ks < KS1; ++ks) aW1[i][ks] = *reinterpret_cast<const s8v*>(w1 + ks * 32);
  }
  {
    const bf16_t* w2 = p.wq + p.off_w2 + (size_t)l16 * HP + 8 * g4;
#pragma unroll
    for (int ks = 0; ks < KS1; ++ks) aW2[ks] = *reinterpret_cast<const s8v*>(w2 + ks * 32);
  }
  float bb[MT][4];
#pragma unroll
  for (int i = 0; i < MT; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) bb[i][j] = p.wf[p.off_b1 + m0 + 16 * i + 4 * g4 + j];
  float b2[3];
#pragma unroll
  for (int j = 0; j < 3; ++j) b2[j] = p.wf[p.off_b2 + j];
