// The weight prologue of the GRU(256) policy kernels, as statements: the two actors (gru.hip), the backtest
// (gru_rollout.hip), the server (gru_serve.hip) and the learner's forward (gru_seq_fwd_kernel, gru_learn.hip, on its
// block's net: online or target) include this once, before their first barrier.  Like gru_net_tile.h it is
// included in place and is not a function: through force-inlined functions the resident W_hh fragments landed in
// other registers and the backtest's launch was 1.1 % slower (profiles/gru_shared_bar.md); included, the kernels
// compile to what they were when each carried a copy.  No `#pragma once`: plain statements.
// In scope at the point of inclusion: p, a GruNetW (gru_common.h) or a launch struct derived from it; the LDS
// carves sWx (const s8v*, RW*6*64 fragments), sB and sWq (float [4*RH] each); tid, lane, l16, g4, wave.
// Declares: Wh, Ws4, myWx, WqA.  A workgroup barrier must follow before the staged LDS data is read.

  // W_ih fragments, the gate biases and W_q rows + b_q into LDS, by every thread
  for (int i = tid; i < RW * 6 * 64; i += RT) const_cast<s8v*>(sWx)[i] = p.wih[i];
  for (int i = tid; i < 4 * RH; i += RT) {
    sB[i] = p.bias4[i];
    sWq[i] = p.wq[i];
  }
  // resident MX-fp8 W_hh fragments of this wave's 32 units x 3 gates (96 VGPRs + 12 scales)
  i8v Wh[3][2][2];
  int Ws4[3] = {0, 0, 0};   // 12 E8M0 scales packed 4 per VGPR: (g, m, ks) -> reg g, byte 2m + ks
#pragma unroll
  for (int g = 0; g < 3; ++g)
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
      for (int ks = 0; ks < 2; ++ks) {
        const int idx = (((wave * 3 + g) * 2 + m) * 2 + ks) * 64 + lane;
        Wh[g][m][ks] = p.whh8[idx];
        Ws4[g] |= (p.whhs[idx] & 0xFF) << (8 * (2 * m + ks));
      }
  const s8v* myWx = sWx + wave * 6 * 64 + lane;   // this wave's W_ih fragments in LDS
  // Q head as one bf16 MFMA per env tile: A = W_q rows (a < 3, zero-padded to 16) over this wave's 32 units, K
  // ordered like the GRU accumulators the B operand is built from: element j of lane group q <-> unit
  // 32w + (j < 4 ? 4q + j : 16 + 4q + j - 4)
  s8v WqA;
  {
    const int a = l16;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int u = 32 * wave + (j < 4 ? 4 * g4 + j : 16 + 4 * g4 + j - 4);
      WqA[j] = (short)f2bf(a < 3 ? p.wq[a * RH + u] : 0.f);
    }
  }
