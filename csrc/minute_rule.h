// The minute-bar trading env (BASELINE config 5) as functions of scalars: the position / reward step and the
// env half of the x row.  Host mirror: sharetrade/env/minute.py (same float32 operations in the same order;
// the build keeps -ffp-contract=off, so nothing here fuses).  Used by the actors of csrc/gru.hip, the backtest
// (csrc/gru_rollout.hip) and the server (csrc/gru_serve.hip).
#pragma once
#include "common.h"

namespace st {

struct MinuteMove {
  int position;   // after the action: 0 flat / 1 long
  float entry;    // close of the bar a long was opened at (unchanged by Sell / Hold)
  float reward;   // position' * ret_t - cost * [position changed]
  bool trade;
};

// action 0 Buy -> long, 1 Sell -> flat, 2 Hold -> keep; c = close[t], r = ret[t] = (close[t+1] / c - 1) * 100
ST_DEV MinuteMove minute_move(int a, int position, float entry, float c, float r, float cost) {
  MinuteMove m;
  m.position = a == 0 ? 1 : (a == 1 ? 0 : position);
  m.trade = m.position != position;
  m.entry = (m.trade && m.position == 1) ? c : entry;
  m.reward = (float)m.position * r - (m.trade ? cost : 0.f);
  return m;
}

// columns 8 .. 15 of the x row (bf16): position, unrealised pnl %, elapsed fraction of the episode, 1, zeros
ST_DEV uint4 minute_x_env(int position, float entry, float c, int elapsed, float inv_ep_len) {
  const float upnl = position ? (c / entry - 1.f) * 100.f : 0.f;
  uint4 w;
  w.x = pack_bf2((float)position, upnl);
  w.y = pack_bf2((float)elapsed * inv_ep_len, 1.f);
  w.z = 0u;
  w.w = 0u;
  return w;
}

// the whole x row (bf16 [32]): the bar's 8 market features, the env columns, zero padding
ST_DEV void minute_x_row(bf16_t* row, uint4 bar_feat, uint4 env_cols) {
  const uint4 z = {0u, 0u, 0u, 0u};
  uint4* d = reinterpret_cast<uint4*>(row);
  d[0] = bar_feat; d[1] = env_cols; d[2] = z; d[3] = z;
}

// first maximum of three (the select chain of the actors: no indexed register array)
ST_DEV int first_max3(float q0, float q1, float q2) {
  int g = 0;
  const float qg = q1 > q0 ? q1 : q0;
  if (q1 > q0) g = 1;
  if (q2 > qg) g = 2;
  return g;
}

}  // namespace st
