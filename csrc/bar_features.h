// One raw OHLCV minute bar -> the GRU(256) policy's 8 market features, as a function of scalars and a 32-byte
// per-series state.  The definition is causal (a bar's row depends on that bar and the state alone), so the same
// function serves whole histories (csrc/bar_features.hip: bar_features_kernel / bar_features_naive_kernel) and
// one bar per session (bar_features_sessions_kernel); its operation order is the synthetic generator's
// (csrc/gru.hip minute_bars_kernel), so replaying the generator's own bars recovers the generator's features:
// the latent sigma through a GARCH(1,1) *filter* -- the generator's variance recursion driven by the observed
// return.  Host mirror: sharetrade/data/ohlcv.py featurise_numpy (same float32 operations in the same order).
//
// The function is inlined into kernels that must agree bit for bit, so fp contraction is off inside it whatever
// the build's flags are: every inlining site rounds alike.
#pragma once
#include "common.h"

namespace st {

constexpr int BF_NF = 8;      // features per bar
constexpr int BF_STATE = 8;   // fp32 words of state per series

struct BarState {
  float prev_close;   // 0: no bar yet (var then starts at sigma^2)
  float r1, r2, r3, r4;   // the previous four log returns (5-bar momentum)
  float var;          // GARCH(1,1) variance of the de-seasonalised return, for the next bar
  float sigma;        // long-run per-bar volatility of the series (fitted, constant)
  float vol_scale;    // the series' volume unit (fitted, constant)
};

ST_DEV BarState bar_state_load(const float* p) {
  const float4 a = *reinterpret_cast<const float4*>(p), b = *reinterpret_cast<const float4*>(p + 4);
  BarState s;
  s.prev_close = a.x; s.r1 = a.y; s.r2 = a.z; s.r3 = a.w;
  s.r4 = b.x; s.var = b.y; s.sigma = b.z; s.vol_scale = b.w;
  return s;
}

ST_DEV void bar_state_store(float* p, const BarState& s) {
  *reinterpret_cast<float4*>(p) = make_float4(s.prev_close, s.r1, s.r2, s.r3);
  *reinterpret_cast<float4*>(p + 4) = make_float4(s.r4, s.var, s.sigma, s.vol_scale);
}

// A bar splits into a part that needs no recurrence and a thin recurrence.  bar_features_pre is a function of the
// bar, the previous close (data, not a computed value) and the series' volume unit: features 0 .. 5 and the three
// values the recurrence consumes.  bar_features_rec advances the state (GARCH variance, the four stored returns)
// and gives features 6 and 7.  bar_features_step is one after the other; a kernel may run the two parts in
// different threads (csrc/bar_features.hip: the tiled kernel) and still round exactly as bar_features_step does,
// because every operation is the same IEEE operation on the same values.
struct BarPre {
  float ret;   // log(close / reference price)
  float ush;   // intraday U-shape 1 + 0.8 x^2
  float dsr;   // de-seasonalised return: the U-shape must not feed the GARCH recursion
};

// minute: the bar's index within its session, 0 .. day - 1.  f[0..5]: return %, high-low range %, close position in
// the range, log volume, sin / cos time of day.  prev_close == 0: no bar yet.
ST_DEV BarPre bar_features_pre(float prev_close, float o, float h, float l, float c, float v, int minute, int day,
                               float vol_scale, float (&f)[BF_NF]) {
#pragma clang fp contract(off)
  const float ref = (minute == 0 || prev_close == 0.f) ? o : prev_close;   // no overnight gap enters a return
  const float x = (2.f * (float)minute / (float)day) - 1.f;
  BarPre p;
  p.ush = 1.f + 0.8f * x * x;
  p.ret = logf(c / ref);
  p.dsr = p.ret / p.ush;
  const float ang = 6.2831853f * (float)minute / (float)day;
  f[0] = p.ret * 100.f;
  f[1] = (h - l) / c * 100.f;
  f[2] = (c - l) / fmaxf(h - l, 1e-12f) - 0.5f;
  f[3] = logf(fmaxf(v / vol_scale, 1e-6f));
  f[4] = sinf(ang);
  f[5] = cosf(ang);
  return p;
}

// f[6]: 5-bar momentum %, f[7]: sigma % (before the variance advances).  Episode ends do not touch the state.
ST_DEV void bar_features_rec(BarState& s, const BarPre& p, float c, float alpha, float beta, float (&f)[BF_NF]) {
#pragma clang fp contract(off)
  const float var = s.prev_close == 0.f ? s.sigma * s.sigma : s.var;
  const float omega = s.sigma * s.sigma * (1.f - alpha - beta);
  const float sig = sqrtf(var) * p.ush;
  s.var = omega + alpha * p.dsr * p.dsr + beta * var;
  const float mom = p.ret + s.r1 + s.r2 + s.r3 + s.r4;
  s.r4 = s.r3; s.r3 = s.r2; s.r2 = s.r1; s.r1 = p.ret;
  s.prev_close = c;
  f[6] = mom * 100.f;
  f[7] = sig * 100.f;
}

ST_DEV void bar_features_step(BarState& s, float o, float h, float l, float c, float v, int minute, int day,
                              float alpha, float beta, float (&f)[BF_NF]) {
  const BarPre p = bar_features_pre(s.prev_close, o, h, l, c, v, minute, day, s.vol_scale, f);
  bar_features_rec(s, p, c, alpha, beta, f);
}

// the bf16 row of a bar (16 bytes, the layout of the generator's feat rows)
ST_DEV uint4 bar_features_pack(const float (&f)[BF_NF]) {
  uint4 w;
  w.x = pack_bf2(f[0], f[1]);
  w.y = pack_bf2(f[2], f[3]);
  w.z = pack_bf2(f[4], f[5]);
  w.w = pack_bf2(f[6], f[7]);
  return w;
}

}  // namespace st
