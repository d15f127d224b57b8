// The trading rule of one engine step, defined once for every step kernel: the epsilon-greedy choice
// (argmax, Philox draw, exploit ramp, random action), the Buy/Sell/Hold transition
// (TrainerChildActor.scala:118-146) with its reward modes, the input features of budget / shares / prices,
// and the TD target (QDecisionPolicyActor.scala:67-71) with its learning knobs.  The torch oracle of all of
// it is sharetrade/env/trading.py (env_transition / engine_step_ref).
//
// Functions of scalars only: every kernel keeps its own data movement (where the values live, which lane
// owns an env) and calls these for the arithmetic.  The _rn forms pin each rounding point.
#pragma once
#include "common.h"

namespace st {

// ----------------------------------------------------------------- epsilon-greedy
// index of the largest of three Q values (the first one on ties); best = that value
ST_DEV int argmax3(float q0, float q1, float q2, float& best) {
  int a = 0;
  best = q0;
  if (q1 > best) { best = q1; a = 1; }
  if (q2 > best) { best = q2; a = 2; }
  return a;
}
ST_DEV int argmax3(float q0, float q1, float q2) {
  float best;
  return argmax3(q0, q1, q2, best);
}

// the per-env draw of a step: Philox4x32-10 over the counter (id, step lo, step hi, stream), id = the env's
// global index (env_offset + e); stream 0 is the step kernels'.  r1 decides explore / exploit, r2 the random action.
ST_DEV void policy_bits(uint32_t id, unsigned long long step, uint32_t key0, uint32_t key1, uint32_t& r1, uint32_t& r2,
                        uint32_t stream = 0u) {
  uint32_t c0 = id, c1 = (uint32_t)(step & 0xFFFFFFFFull), c2 = (uint32_t)(step >> 32), c3 = stream;
  philox4x32(c0, c1, c2, c3, key0, key1);
  r1 = c0;
  r2 = c1;
}
// ... as two uniforms in [0, 1)
ST_DEV void policy_draw(uint32_t id, unsigned long long step, uint32_t key0, uint32_t key1, float& u1, float& u2,
                        uint32_t stream = 0u) {
  uint32_t r1, r2;
  policy_bits(id, step, key0, key1, r1, r2, stream);
  u1 = u24(r1);
  u2 = u24(r2);
}
// the exploit probability ramps up to eps with ramp_pos (the episode position, or the step count)
ST_DEV bool exploits(float u1, float eps, float ramp_pos, float inv_ramp) {
  return u1 < fminf(eps, __fmul_rn(ramp_pos, inv_ramp));
}
ST_DEV int random_action(float u2) {
  int rnd = (int)(u2 * 3.0f);
  rnd = rnd > 2 ? 2 : rnd;
  return rnd;
}

// ----------------------------------------------------------------- Buy / Sell / Hold
struct Holding {
  float budget;
  int shares;
};
// the budget and shares a trade starts from: compat_env reproduces the reference, whose child actor trades
// from its initial budget and shares on every step
ST_DEV Holding trade_base(float b, int s, int compat_env, float b0, int s0) {
  Holding h;
  h.budget = compat_env ? b0 : b;
  h.shares = compat_env ? s0 : s;
  return h;
}
// action 0 buys one share at vnew if the budget covers it, 1 sells one if there is one, anything else holds
ST_DEV Holding trade(int a, Holding h, float vnew) {
  const float bd = h.budget;
  const int sd = h.shares;
  const bool buy = (a == 0) && (bd >= vnew);
  const bool sell = (a == 1) && (sd > 0);
  Holding r;
  r.budget = buy ? __fsub_rn(bd, vnew) : (sell ? __fadd_rn(bd, vnew) : bd);
  r.shares = buy ? sd + 1 : (sell ? sd - 1 : sd);
  return r;
}
// reward_mode 0: the change of portfolio value (b + s * vprev -> b2 + s2 * vnew); 1: its one-step return
// (change / previous, 0 where the previous value is not positive); 2: growth, log1p of the return to 2nd order
ST_DEV float reward(float b, int s, float vprev, float b2, int s2, float vnew, int reward_mode) {
  const float cur = __fadd_rn(b, __fmul_rn((float)s, vprev));
  const float nw = __fadd_rn(b2, __fmul_rn((float)s2, vnew));
  float rew = __fsub_rn(nw, cur);
  if (reward_mode) rew = cur > 0.f ? __fdiv_rn(rew, cur) : 0.f;
  if (reward_mode == 2) rew = __fsub_rn(rew, __fmul_rn(__fmul_rn(rew, 0.5f), rew));
  return rew;
}

// ----------------------------------------------------------------- input features (mode 1: relative)
ST_DEV float feat_price(float w, float inv, int mode) {
  return mode ? __fsub_rn(__fmul_rn(w, inv), 1.0f) : w;
}
ST_DEV float feat_budget(float b, float inv_b0, int mode) { return mode ? __fmul_rn(b, inv_b0) : b; }
ST_DEV float feat_shares(int s, float last, float inv_b0, int mode) {
  return mode ? __fmul_rn(__fmul_rn((float)s, last), inv_b0) : (float)s;
}

// ----------------------------------------------------------------- TD target
// value of the next state given a target net's row (t0, t1, t2) = Q_target(x'): its max, or (compat slot,
// Double DQN: of_online_argmax) the entry of the online net's argmax am.  Without a target net the value is
// the online net's max.
ST_DEV float target_value(float t0, float t1, float t2, int am, bool of_online_argmax) {
  return of_online_argmax ? (am == 0 ? t0 : (am == 1 ? t1 : t2)) : fmaxf(fmaxf(t0, t1), t2);
}
ST_DEV float td_target(float rew, float reward_scale, float gamma, float vnext) {
  const float rs = reward_scale != 1.0f ? __fmul_rn(rew, reward_scale) : rew;
  return __fadd_rn(rs, __fmul_rn(gamma, vnext));
}
// dL/dq of the trained slot: coef * (qs - y), the error clamped to [-td_clip, td_clip] when td_clip > 0
// (Huber loss), and no gradient through an output ReLU that is off.  diff = the unclipped error (the loss).
ST_DEV float td_dq(float qs, float y, float coef, float td_clip, int output_relu, float& diff) {
  diff = __fsub_rn(qs, y);
  float dq = coef * (td_clip > 0.f ? fminf(fmaxf(diff, -td_clip), td_clip) : diff);
  if (output_relu && !(qs > 0.f)) dq = 0.f;
  return dq;
}

}  // namespace st
