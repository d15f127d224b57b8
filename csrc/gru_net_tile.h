// The net of the GRU(256) policy on ONE 16-env tile n of a chunk: gates from x (bf16 16x16x32, W_ih from LDS) and
// h (MX-fp8 16x16x128, two K steps over the 256 hidden units), the GRU update of hrt[.][n] in registers (lane:
// units u0 .. u0+3 of tile m, env 16n + l16), and this wave's Q partials -> sQp.  One tile at a time keeps the
// accumulators at 32 VGPRs (W_hh holds 108).
//
// This is the one definition of the bar's arithmetic, as statements: the two actors (gru.hip), the backtest
// (gru_rollout.hip), the server (gru_serve.hip) and the learner's forward (gru_seq_fwd_kernel, gru_learn.hip), which
// evaluates the function the actors act with, include it inside their `for (n = 0; n < 2; ++n)` loop.  It is
// not a function because the same text as a force-inlined function is simplified on its own before it is
// inlined, and the step loops of the pair actor and the backtest then issued one LDS read of the tile 0 -> 1
// hand-over later and ran 0.5 to 0.8 % slower (profiles/gru_shared_bar.md); included in place, the loops are the
// ones the kernels had when each carried a copy.
// No `#pragma once`: plain statements, included once per kernel.
// In scope at the point of inclusion: n; Wh, Ws4, myWx, WqA (gru_weights.h); cX / cH / cS, the x rows, the fp8
// h tile and its scales the step reads; sB, sQp ([RW][3][RN] floats); hrt, a float (&)[2][2][4] on the chunk's h;
// wave, l16, g4; and the macro GRU_TILE_STAMP: a statement run after the tile's MFMAs (the single actor's debug
// stamp), or empty.
// Optional, for the learner, which keeps the gates for its backward (without a definition nothing is kept):
// GRU_TILE_SAVE(m, i, r, z, nn, gh_n, h_prev), statements run for unit (m, i) once its gates are formed and before
// its h is overwritten (gh_n is the pre-scaled accumulator), and GRU_TILE_SAVED, a statement run after the tile's
// GRU update and before its Q MFMA: there the learner stores what it kept.  After the Q partials the same stores
// cost the learner's forward 4.5 % (profiles/gru_learn_shared_bar.md).
#ifndef GRU_TILE_SAVE
#define GRU_TILE_SAVE(m, i, r, z, nn, gh_n, h_prev)
#endif
#ifndef GRU_TILE_SAVED
#define GRU_TILE_SAVED
#endif
  f4v ar[2], az[2], anx[2], anh[2];   // accumulators start at the biases (b_ir+b_hr, b_iz+b_hz, b_in, b_hn)
#pragma unroll
  for (int m = 0; m < 2; ++m) {
    const int u0 = 32 * wave + 16 * m + 4 * g4;
    ar[m] = *reinterpret_cast<const f4v*>(sB + u0);
    az[m] = *reinterpret_cast<const f4v*>(sB + RH + u0);
    anx[m] = *reinterpret_cast<const f4v*>(sB + 2 * RH + u0);
    anh[m] = *reinterpret_cast<const f4v*>(sB + 3 * RH + u0);
  }
  const int row = 16 * n + l16;
  {
    const s8v xb = lds_ld8(cX + row * XS + 8 * g4);
#pragma unroll
    for (int m = 0; m < 2; ++m) {
      ar[m] = mfma32(myWx[(0 * 2 + m) * 64], xb, ar[m]);
      az[m] = mfma32(myWx[(1 * 2 + m) * 64], xb, az[m]);
      anx[m] = mfma32(myWx[(2 * 2 + m) * 64], xb, anx[m]);
    }
  }
#pragma unroll
  for (int ks = 0; ks < 2; ++ks) {
    // bytes 0..15: units 128ks + 16g4 + [0,16); bytes 16..31: units 128ks + 64 + 16g4 + [0,16)
    const uint4 h0 = *reinterpret_cast<const uint4*>(cH + row * HS + 128 * ks + 16 * g4);
    const uint4 h1 = *reinterpret_cast<const uint4*>(cH + row * HS + 128 * ks + 64 + 16 * g4);
    i8v hb;
    hb[0] = (int)h0.x; hb[1] = (int)h0.y; hb[2] = (int)h0.z; hb[3] = (int)h0.w;
    hb[4] = (int)h1.x; hb[5] = (int)h1.y; hb[6] = (int)h1.z; hb[7] = (int)h1.w;
    const int sc = cS[row * SCS + 4 * ks + g4];   // scale of K-block g4 = units of wave 4ks + g4
#define ST_MX3(M, KS)                                                              \
  ar[M] = mx_mfma_sel<2 * (M) + (KS)>(Wh[0][M][KS], hb, ar[M], Ws4[0], sc);          \
  az[M] = mx_mfma_sel<2 * (M) + (KS)>(Wh[1][M][KS], hb, az[M], Ws4[1], sc);          \
  anh[M] = mx_mfma_sel<2 * (M) + (KS)>(Wh[2][M][KS], hb, anh[M], Ws4[2], sc);
    if (ks == 0) { ST_MX3(0, 0) ST_MX3(1, 0) } else { ST_MX3(0, 1) ST_MX3(1, 1) }
#undef ST_MX3
  }
  GRU_TILE_STAMP
#pragma unroll
  for (int m = 0; m < 2; ++m)
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const float r = sigm_ps(ar[m][i]);
      const float z = sigm_ps(az[m][i]);
      const float nn = tanh_ps(__builtin_fmaf(r, anh[m][i], anx[m][i]));
      GRU_TILE_SAVE(m, i, r, z, nn, anh[m][i], hrt[m][n][i])
      hrt[m][n][i] = __builtin_fmaf(z, hrt[m][n][i] - nn, nn);
    }
  GRU_TILE_SAVED
  // Q partials of this wave's units: one MFMA, h' (bf16) taken straight from the accumulator layout
  s8v hb;
  const uint32_t p0 = pack_bf2(hrt[0][n][0], hrt[0][n][1]), p1 = pack_bf2(hrt[0][n][2], hrt[0][n][3]);
  const uint32_t p2 = pack_bf2(hrt[1][n][0], hrt[1][n][1]), p3 = pack_bf2(hrt[1][n][2], hrt[1][n][3]);
  hb[0] = (short)(p0 & 0xFFFF); hb[1] = (short)(p0 >> 16); hb[2] = (short)(p1 & 0xFFFF); hb[3] = (short)(p1 >> 16);
  hb[4] = (short)(p2 & 0xFFFF); hb[5] = (short)(p2 >> 16); hb[6] = (short)(p3 & 0xFFFF); hb[7] = (short)(p3 >> 16);
  const f4v qp = mfma32(WqA, hb, zero4());
  if (g4 == 0) {   // rows a = 0..2 of the 16x16 result live in lanes 0..15, registers 0..2
    sQp[(wave * 3 + 0) * RN + row] = qp[0];
    sQp[(wave * 3 + 1) * RN + row] = qp[1];
    sQp[(wave * 3 + 2) * RN + row] = qp[2];
  }
