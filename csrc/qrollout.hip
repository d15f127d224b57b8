// Backtest of a frozen policy on CDNA4 (gfx950): whole episodes of the Buy/Sell/Hold env in one launch.
//
// For env e and day t = start .. start + steps - 1 the rule is the engine's (csrc/trade_rule.h, oracle
// sharetrade/serve/rollout.py::reference_rollout): window prices[e, t : t+H] -> features -> the flagship
// 2x128 bf16 Q-net (224 -> 128 -> 128 -> 16: csrc/qnet_common.h, shared with qserve.hip) -> argmax -> epsilon-greedy
// (Philox stream 4, exploit ramp on the day t) -> trade at v = prices[e, t+H].  Only the budget and the
// shares of the 203 inputs depend on earlier actions, and consecutive windows share H - 1 prices, so a
// workgroup owns its envs for the whole launch:
//  * every weight lives in VGPRs (a wave owns 32 hidden units of both hidden layers plus the output
//    fragments: 104 registers per lane), loaded once per workgroup;
//  * the env state (budget, shares, trade counts) lives in the registers of the lane that ends up with
//    the env's Q row (waves 0 .. NET-1, lanes 0 .. 15);
//  * prices sit in LDS in a ring of 256 values per env: the first block loads H + D of them, every later
//    block of D days loads the D new ones (prefetched into registers a block ahead), so each price is read
//    from HBM once; 1 / last of a block's D windows is computed once per block;
//  * per day: features of the 32 envs (one row per wave pass, lanes along the columns) -> layer 1 ->
//    layer 2 -> output + trade, four LDS-only barriers, no global load on the chain.
// 32 envs per workgroup keep the LDS at 61 KB: two workgroups (four independent 16-env tiles) per CU, one
// workgroup's serial chain under the other's MFMA phases.
//
// The kernel is a template on LEDGER, so the day loop is defined once and the plain instance
// (qrollout_kernel<false>, st_qrollout_launch) carries none of the ledger's work.  The ledger instance
// (qrollout_kernel<true>, st_qrollout_ledger_launch) also keeps, per env and in the owner lane's trade phase, one
// cumulative risk record of 24 words (struct LedgerOut below: equity curve, drawdowns, position and price sums,
// action counts) and, per 16-env chunk and day, the sum of the envs' gains, which qrollout_curve_reduce_kernel
// adds over the chunks to the portfolio curve.  The record lives in LDS (one row per env, 3.5 KB behind the plain
// layout) and is read and written back by six 128-bit accesses a day: only the owner lane touches its row, in
// phase P3, so no further barrier is needed and the instance needs no registers across the day loop.  All of it
// is fp32 in day order with unfused operations.  Oracle: sharetrade/serve/rollout.py::ledger_from_trace.
#include <type_traits>

#include "qnet_common.h"

namespace st {
namespace rollout {
using namespace qnet;   // padded dims, q_head_row; the kernel includes qnet_weights.h, qnet_layers.h, qnet_head.h

constexpr int C = 32;                           // envs per workgroup
constexpr int NW = 4, NT = 64 * NW;
constexpr int NET = C / 16;                     // 16-env tiles per workgroup
constexpr int MT = HP / (16 * NW);              // 16-unit m-tiles per wave
constexpr int D = 32;                           // days per price block
constexpr int RING = 256, SP = RING + 1;        // price ring per env (floats), padded row stride
constexpr int RPW = C / NW;                     // feature rows per wave
static_assert(INP - 3 + D <= RING, "a block's windows and trade prices must fit the ring");
static_assert(C * D == 4 * NT && NT / D == 8, "block loader: 4 values per thread, 8 rows per pass");

constexpr int OFF_X = 0;                            // bf16 [C][SX]; H2 [C][SH] over it
constexpr int OFF_H1 = OFF_X + C * SX * 2;          // bf16 [C][SH]
constexpr int OFF_P = OFF_H1 + C * SH * 2;          // fp32 [C][SP] price ring: price j at column j % RING
constexpr int OFF_INV = OFF_P + C * SP * 4;         // fp32 [C][D] 1 / last price of the block's windows
constexpr int OFF_FB = OFF_INV + C * D * 4;         // fp32 [C] budget feature of the coming day
constexpr int OFF_FS = OFF_FB + C * 4;              // fp32 [C] shares feature of the coming day
constexpr int LDS_BYTES = OFF_FS + C * 4;
static_assert(OFF_H1 % 16 == 0 && OFF_P % 16 == 0 && OFF_INV % 16 == 0 && OFF_FB % 16 == 0, "16-byte carves");
constexpr int LW = 24;                              // words of an env's ledger record
constexpr int CH = 16;                              // envs per chunk of the portfolio curve (a tile of a wave)
constexpr int LS = LW + 4;                          // record stride: 16 lanes' 128-bit accesses cover the 64 banks once
constexpr int OFF_LG = LDS_BYTES;                   // u32 [C][LS] ledger records (ledger instance)
constexpr int LDS_BYTES_LEDGER = OFF_LG + C * LS * 4;
static_assert(OFF_LG % 16 == 0 && 2 * LDS_BYTES_LEDGER <= 160 * 1024, "two ledger workgroups per CU");

// the barriers order LDS traffic and leave the trace stores and the price prefetch in flight
ST_DEV void bar() { lds_barrier(); }

struct RolloutParams {
  const float* prices;     // [E][ld] fp32, T valid values per row
  const bf16_t* wq;        // bf16 flat params (engine layout)
  const float* wf;         // fp32 flat params (biases)
  const float* budget;     // [E] initial budget, or null = b0
  const int* shares;       // [E] initial shares, or null = s0
  float* out_budget;       // [E]
  int* out_shares;         // [E]
  float* out_portfolio;    // [E] budget + shares * last trade price
  int* out_buys;           // [E] executed buys
  int* out_sells;          // [E] executed sells
  signed char* tr_actions; // [E][steps] or null
  float* tr_q;             // [E][steps][3] or null
  float* tr_equity;        // [E][steps] or null: the portfolio after each day's trade
  int E, ld, T, H, start, steps;
  int off_w0, off_w1, off_b1, off_w2, off_b2;
  int feat_mode, output_relu, compat_env;
  int s0;
  float b0, inv_b0, eps, inv_ramp;   // eps = inf: greedy
  uint32_t key0, key1, env_offset;   // draw counter: (env_offset + e, day, 0, stream 4)
};

// What the ledger instance writes besides RolloutParams' outputs.  state_in null = a fresh ledger; with state_in
// the host also passes the budget / shares the piece before ended with.  {part, curve} are given together or not
// at all.  A record is the ledger of the whole run so far (pieces reproduce the whole bit for bit), 24 words:
//   word  0 eq_prev     fp32  equity b + s * v after the last day (eq0 before the first)
//         1 eq0         fp32  b_in + s_in * v0 of a fresh ledger
//         2 v0          fp32  prices[e][start + H - 1] of a fresh ledger (the last price of the first window)
//         3 v_last      fp32  the last trade price
//         4 peak        fp32  max(eq0, every eq)
//         5 max_dd      fp32  the largest peak - eq
//         6 sumsq       fp32  sum of (eq - eq_prev)^2
//         7 sum_d       fp32  sum of d = v - v0
//         8 sum_d2      fp32  sum of d * d
//         9 sum_sd      fp32  sum of float(s) * d, s after the trade
//        10 run         int32 days since eq < peak began (0 at a peak)
//        11 dd_days     int32 the longest run
//        12 days        int32
//        13 chose_buy   int32 days with action 0
//        14 chose_sell  int32 days with action 1
//        15 refused_buy int32 Buys that left the shares unchanged
//        16 refused_sell int32
//        17 flat_days   int32 days ending with 0 shares
//        18 max_shares  int32
//        19 0 (pad)
//    20, 21 sum_s       int64 (low word first) sum of s after the trade
//    22, 23 sum_s2      int64 sum of s * s
struct LedgerOut {
  const uint32_t* state_in;    // [E][24] records of the piece before, or null
  uint32_t* state_out;         // [E][24]
  float* part;                 // [ceil(E / 16)][part_stride] per-day sum of a 16-env chunk's gains eq - eq0
  double* curve;               // [steps] sum of part over the chunks in ascending order
  int part_stride, pad_;       // steps rounded up to 32
};

struct RolloutLedger {
  RolloutParams r;
  LedgerOut l;
};

enum LedgerWord {
  LG_EQ_PREV, LG_EQ0, LG_V0, LG_V_LAST, LG_PEAK, LG_MAX_DD, LG_SUMSQ, LG_SUM_D, LG_SUM_D2, LG_SUM_SD,
  LG_RUN, LG_DD_DAYS, LG_DAYS, LG_CHOSE_BUY, LG_CHOSE_SELL, LG_REFUSED_BUY, LG_REFUSED_SELL, LG_FLAT_DAYS,
  LG_MAX_SHARES, LG_PAD, LG_SUM_S, LG_SUM_S_HI, LG_SUM_S2, LG_SUM_S2_HI
};
static_assert(LG_SUM_S2_HI == LW - 1 && LG_SUM_S % 2 == 0, "24 words, the int64 sums on even words");

// Sum over the 16 lanes of a DPP row by the fixed tree of ledger_from_trace's chunk_sums: the pairs 8, 4, 2, 1
// lanes apart, lane l taking l + w at every level (row_shl; lanes past the row read 0).  Lane 0 of the row holds
// the sum.  Called by whole rows only.
ST_DEV float row_tree_sum(float v) {
  v = __fadd_rn(v, __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(v), 0x108, 0xF, 0xF, true)));   // row_shl:8
  v = __fadd_rn(v, __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(v), 0x104, 0xF, 0xF, true)));
  v = __fadd_rn(v, __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(v), 0x102, 0xF, 0xF, true)));
  v = __fadd_rn(v, __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(v), 0x101, 0xF, 0xF, true)));
  return v;
}

// the launch struct of an instance, and its two halves
template <bool LEDGER> struct ArgsOf { using type = RolloutParams; };
template <> struct ArgsOf<true> { using type = RolloutLedger; };
ST_DEV const RolloutParams& plain_of(const RolloutParams& q) { return q; }
ST_DEV const RolloutParams& plain_of(const RolloutLedger& q) { return q.r; }
ST_DEV LedgerOut ledger_of(const RolloutParams&) { return LedgerOut{}; }
ST_DEV const LedgerOut& ledger_of(const RolloutLedger& q) { return q.l; }

template <bool LEDGER>
__global__ void __launch_bounds__(NT, 2) qrollout_kernel(typename ArgsOf<LEDGER>::type q) {
  const RolloutParams& p = plain_of(q);
  const LedgerOut& L = ledger_of(q);   // (read by the ledger instance only)
  extern __shared__ __attribute__((aligned(16))) char smem[];
  bf16_t* sX = reinterpret_cast<bf16_t*>(smem + OFF_X);
  bf16_t* sH1 = reinterpret_cast<bf16_t*>(smem + OFF_H1);
  bf16_t* sH2 = sX;
  float* sP = reinterpret_cast<float*>(smem + OFF_P);
  float* sInv = reinterpret_cast<float*>(smem + OFF_INV);
  float* sFB = reinterpret_cast<float*>(smem + OFF_FB);
  float* sFS = reinterpret_cast<float*>(smem + OFF_FS);
  uint32_t* sLg = reinterpret_cast<uint32_t*>(smem + OFF_LG);   // (ledger instance: beyond the plain one's LDS)
  const int tid = threadIdx.x, lane = tid & 63, l16 = lane & 15, g4 = lane >> 4;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int m0 = 16 * MT * wave;
  const int H = p.H, mode = p.feat_mode;
  const bool greedy = __builtin_isinf(p.eps);

  // ---------------------------------------------------------------- weights -> VGPRs (once)
#include "qnet_weights.h"

  const int tend = p.start + p.steps;
  const int ntiles = (p.E + C - 1) / C;
  // block loader: thread = (column tid % D of the block, rows tid / D + 8 k); rows past E re-read row E - 1
  const int lc = tid & (D - 1), lr = tid / D;

  for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int r0 = tile * C;
    // the env of this lane: waves 0 .. NET-1, lanes 0 .. 15 (where the output MFMA leaves q[0..2])
    const bool owner = wave < NET && g4 == 0;
    const int myrow = owner ? 16 * wave + l16 : 0;
    const int env = r0 + myrow;
    const bool live = owner && env < p.E;
    float b = p.b0, vlast = 0.f;
    int s = p.s0, nbuy = 0, nsell = 0;
    if (owner) {
      const int ec = min(env, p.E - 1);
      if (p.budget != nullptr) b = p.budget[ec];
      if (p.shares != nullptr) s = p.shares[ec];
    }
    // ------------------------------------------------------------ first block: prices start .. start+H+D-1
#pragma unroll 1
    for (int i = 0; i < RPW; ++i) {
      const int r = wave * RPW + i;
      const float* row = p.prices + (size_t)min(r0 + r, p.E - 1) * (size_t)p.ld;
      for (int c = lane; c < H + D; c += 64) {
        const int j = p.start + c;
        sP[r * SP + (j & (RING - 1))] = row[min(j, p.T - 1)];
      }
    }
    bar();
    if (owner) {
      const float last = sP[myrow * SP + ((p.start + H - 1) & (RING - 1))];
      sFB[myrow] = feat_budget(b, p.inv_b0, mode);
      sFS[myrow] = feat_shares(s, last, p.inv_b0, mode);
      if constexpr (LEDGER) {
        // the env's record: carried in, or fresh from the holding and the price the env starts from
        uint32_t* lg = sLg + myrow * LS;
        if (L.state_in != nullptr) {
          const uint32_t* src = L.state_in + (size_t)min(env, p.E - 1) * LW;
#pragma unroll
          for (int w = 0; w < LW; ++w) lg[w] = src[w];
        } else {
          const uint32_t eq0 = __float_as_uint(__fadd_rn(b, __fmul_rn((float)s, last)));
#pragma unroll
          for (int w = 0; w < LW; ++w) lg[w] = 0u;
          lg[LG_EQ_PREV] = eq0;
          lg[LG_EQ0] = eq0;
          lg[LG_PEAK] = eq0;
          lg[LG_V0] = __float_as_uint(last);
        }
      }
    }
    float pb = 0.f;   // (ledger instance) lane l16: the chunk's gain of day l16 of the current 16 days

#pragma unroll 1
    for (int t0 = p.start; t0 < tend; t0 += D) {
      // 1 / last of the block's windows (torch: 1.0 / last, one correctly rounded division per env and day)
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int r = lr + 8 * k;
        const float last = sP[r * SP + ((t0 + lc + H - 1) & (RING - 1))];
        sInv[r * D + lc] = mode ? __fdiv_rn(1.0f, last) : 1.0f;
      }
      // the next block's D new prices, in flight through this block's days
      const bool more = t0 + D < tend;
      float pf[4] = {0.f, 0.f, 0.f, 0.f};
      const int jn = t0 + H + D + lc;
      if (more) {
#pragma unroll
        for (int k = 0; k < 4; ++k)
          pf[k] = p.prices[(size_t)min(r0 + lr + 8 * k, p.E - 1) * (size_t)p.ld + (size_t)min(jn, p.T - 1)];
      }
      bar();
      const int nd = min(D, tend - t0);
#pragma unroll 1
      for (int d = 0; d < nd; ++d) {
        const int t = t0 + d;
        // ---------------------------------------------------------- P0: ring -> features (bf16)
        // a wave builds its RPW rows one after the other, lane = column pair (2 l, 2 l + 1) of 112
        // (columns 0 .. 127 and 128 .. 223).  Every load is unconditional (columns past the window re-read its
        // last price) and the four ring columns of a lane are the same for all its rows: loads under per-element
        // branches were issued one LDS round trip at a time.  The feature mode is compile-time in the body (one
        // uniform branch per day picks the instance), and the low 64 pairs are prices only (host: H >= 128).
        auto p0 = [&](auto mode_c) {
          constexpr int md = decltype(mode_c)::value;
          int rc[2][2];   // ring column of (pair jj, element q) on day t
#pragma unroll
          for (int jj = 0; jj < 2; ++jj)
#pragma unroll
            for (int q = 0; q < 2; ++q) rc[jj][q] = (t + min(2 * (lane + 64 * jj) + q, H - 1)) & (RING - 1);
          float w[RPW][2][2], inv[RPW], fb[RPW], fs[RPW];
#pragma unroll
          for (int i = 0; i < RPW; ++i) {
            const int r = wave * RPW + i;
            inv[i] = sInv[r * D + d];
            fb[i] = sFB[r];
            fs[i] = sFS[r];
#pragma unroll
            for (int jj = 0; jj < 2; ++jj)
#pragma unroll
              for (int q = 0; q < 2; ++q) w[i][jj][q] = sP[r * SP + rc[jj][q]];
          }
#pragma unroll
          for (int i = 0; i < RPW; ++i) {
            const int r = wave * RPW + i;
#pragma unroll
            for (int jj = 0; jj < 2; ++jj) {
              const int c = 2 * (lane + 64 * jj);
              float x[2];
#pragma unroll
              for (int q = 0; q < 2; ++q) {
                const int k = c + q;
                x[q] = feat_price(w[i][jj][q], inv[i], md);
                if (jj == 1) {   // pairs that can reach column H: budget, shares, the constant 1, padding
                  x[q] = k == H ? fb[i] : x[q];
                  x[q] = k == H + 1 ? fs[i] : x[q];
                  x[q] = k == H + 2 ? 1.0f : x[q];
                  x[q] = k > H + 2 ? 0.0f : x[q];
                }
              }
              if (c < INP) *reinterpret_cast<uint32_t*>(sX + r * SX + c) = pack_bf2(x[0], x[1]);
            }
          }
        };
        if (mode) p0(std::integral_constant<int, 1>{});
        else p0(std::integral_constant<int, 0>{});
        bar();
        // ---------------------------------------------------------- P1, P2: layers 1 and 2 -> H2 (over X)
#include "qnet_layers.h"
        // ---------------------------------------------------------- P3: output, policy, trade
        if (wave < NET) {
#include "qnet_head.h"   // wave w: 16-env tile w; lanes g4 == 0 end up with the outputs of env 16 w + l16 in acc
          if (g4 == 0) {
            float q[3];
            int a = q_head_row(acc, b2, p.output_relu, q);
            if (!greedy) {
              float u1, u2;
              policy_draw(p.env_offset + (uint32_t)env, (unsigned long long)t, p.key0, p.key1, u1, u2, 4u);
              a = exploits(u1, p.eps, (float)t, p.inv_ramp) ? a : random_action(u2);
            }
            const float v = sP[myrow * SP + ((t + H) & (RING - 1))];
            const Holding h = trade_base(b, s, p.compat_env, p.b0, p.s0);
            const Holding r = trade(a, h, v);
            nbuy += r.shares > h.shares;
            nsell += r.shares < h.shares;
            b = r.budget;
            s = r.shares;
            vlast = v;
            // tomorrow's window ends at today's trade price
            sFB[myrow] = feat_budget(b, p.inv_b0, mode);
            sFS[myrow] = feat_shares(s, v, p.inv_b0, mode);
            if (live) {
              const size_t o = (size_t)env * (size_t)p.steps + (size_t)(t - p.start);
              if (p.tr_actions != nullptr) p.tr_actions[o] = (signed char)a;
              if (p.tr_q != nullptr) {
                p.tr_q[3 * o + 0] = q[0];
                p.tr_q[3 * o + 1] = q[1];
                p.tr_q[3 * o + 2] = q[2];
              }
              if (p.tr_equity != nullptr) p.tr_equity[o] = __fadd_rn(b, __fmul_rn((float)s, v));
            }
            if constexpr (LEDGER) {
              uint4* row = reinterpret_cast<uint4*>(sLg + myrow * LS);
              uint32_t lg[LW];
#pragma unroll
              for (int w = 0; w < LW; w += 4) {
                const uint4 x = row[w / 4];
                lg[w] = x.x; lg[w + 1] = x.y; lg[w + 2] = x.z; lg[w + 3] = x.w;
              }
              auto ldf = [&](int w) { return __uint_as_float(lg[w]); };
              auto stf = [&](int w, float x) { lg[w] = __float_as_uint(x); };
              auto inc = [&](int w, bool c) { lg[w] += c ? 1u : 0u; };
              // equity curve
              const float eq = __fadd_rn(b, __fmul_rn((float)s, v));
              const float pnl = __fsub_rn(eq, ldf(LG_EQ_PREV));
              stf(LG_SUMSQ, __fadd_rn(ldf(LG_SUMSQ), __fmul_rn(pnl, pnl)));
              stf(LG_EQ_PREV, eq);
              float peak = ldf(LG_PEAK);
              peak = eq > peak ? eq : peak;
              stf(LG_PEAK, peak);
              const float dd = __fsub_rn(peak, eq), mdd = ldf(LG_MAX_DD);
              stf(LG_MAX_DD, dd > mdd ? dd : mdd);
              const int run = eq < peak ? (int)lg[LG_RUN] + 1 : 0;
              lg[LG_RUN] = (uint32_t)run;
              lg[LG_DD_DAYS] = (uint32_t)max((int)lg[LG_DD_DAYS], run);
              // price and position sums (s after the trade)
              const float dv = __fsub_rn(v, ldf(LG_V0));
              stf(LG_SUM_D, __fadd_rn(ldf(LG_SUM_D), dv));
              stf(LG_SUM_D2, __fadd_rn(ldf(LG_SUM_D2), __fmul_rn(dv, dv)));
              stf(LG_SUM_SD, __fadd_rn(ldf(LG_SUM_SD), __fmul_rn((float)s, dv)));
              const unsigned long long ss =
                  (((unsigned long long)lg[LG_SUM_S_HI] << 32) | lg[LG_SUM_S]) + (unsigned long long)(long long)s;
              lg[LG_SUM_S] = (uint32_t)ss;
              lg[LG_SUM_S_HI] = (uint32_t)(ss >> 32);
              const unsigned long long s2 = (((unsigned long long)lg[LG_SUM_S2_HI] << 32) | lg[LG_SUM_S2]) +
                                            (unsigned long long)((long long)s * (long long)s);
              lg[LG_SUM_S2] = (uint32_t)s2;
              lg[LG_SUM_S2_HI] = (uint32_t)(s2 >> 32);
              // counts (h.shares: the shares before the trade)
              inc(LG_DAYS, true);
              inc(LG_CHOSE_BUY, a == 0);
              inc(LG_CHOSE_SELL, a == 1);
              inc(LG_REFUSED_BUY, a == 0 && s == h.shares);
              inc(LG_REFUSED_SELL, a == 1 && s == h.shares);
              inc(LG_FLAT_DAYS, s == 0);
              lg[LG_MAX_SHARES] = (uint32_t)max((int)lg[LG_MAX_SHARES], s);
              stf(LG_V_LAST, v);
#pragma unroll
              for (int w = 0; w < LW; w += 4) row[w / 4] = make_uint4(lg[w], lg[w + 1], lg[w + 2], lg[w + 3]);
              // portfolio curve: the chunk's sum of the day's gains (rows past E contribute 0); lane i & 15 keeps
              // day i's and 16 days go out at once.  Chunk 2 tile + wave exists when its first row does.
              if (L.part != nullptr) {
                const int i = t - p.start;
                const float sum = row_tree_sum(live ? __fsub_rn(eq, ldf(LG_EQ0)) : 0.f);
                const float sum0 = __uint_as_float(__builtin_amdgcn_readfirstlane(__float_as_uint(sum)));
                pb = l16 == (i & 15) ? sum0 : pb;
                if (((i & 15) == 15 || t == tend - 1) && l16 <= (i & 15) && r0 + CH * wave < p.E)
                  L.part[(size_t)((r0 + CH * wave) / CH) * (size_t)L.part_stride + (size_t)((i & ~15) + l16)] = pb;
              }
            }
          }
        }
        bar();   // the next day's features overwrite X / H2; every read of this day's ring columns is done
      }
      if (more) {
#pragma unroll
        for (int k = 0; k < 4; ++k) sP[(lr + 8 * k) * SP + (jn & (RING - 1))] = pf[k];
        bar();
      }
    }
    if (live) {
      p.out_budget[env] = b;
      p.out_shares[env] = s;
      p.out_portfolio[env] = __fadd_rn(b, __fmul_rn((float)s, vlast));
      p.out_buys[env] = nbuy;
      p.out_sells[env] = nsell;
      if constexpr (LEDGER) {
        uint4* dst = reinterpret_cast<uint4*>(L.state_out + (size_t)env * LW);
        const uint4* row = reinterpret_cast<const uint4*>(sLg + myrow * LS);
#pragma unroll
        for (int w = 0; w < LW; w += 4) dst[w / 4] = row[w / 4];
      }
    }
  }
}

// curve[day] = sum over the chunks, in ascending order from 0, of (double)part[chunk][day]: one thread per day
// (float64: at 65,536 envs the book's gain exceeds fp32's integer range)
__global__ void __launch_bounds__(256) qrollout_curve_reduce_kernel(const float* __restrict__ part,
                                                                    double* __restrict__ curve, int nchunks,
                                                                    int steps, int part_stride) {
  const int s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= steps) return;
  double acc = 0.0;
  for (int c = 0; c < nchunks; ++c) acc += (double)part[(size_t)c * (size_t)part_stride + (size_t)s];
  curve[s] = acc;
}

}  // namespace rollout
}  // namespace st

extern "C" int st_qrollout_lds_bytes() { return st::rollout::LDS_BYTES; }
extern "C" int st_qrollout_day_block() { return st::rollout::D; }

namespace {

// the checks both launches share (below)
bool rollout_ok(const st::rollout::RolloutParams* p) {
  using namespace st::rollout;
  return !(p->H < 128 || p->H + 3 > INP || p->T < p->H + 1 || p->ld < p->T || p->start < 0 || p->steps < 1 ||
      (long long)p->start + p->steps > (long long)p->T - p->H || p->prices == nullptr || p->wq == nullptr ||
      p->wf == nullptr || p->out_budget == nullptr || p->out_shares == nullptr || p->out_portfolio == nullptr ||
      p->out_buys == nullptr || p->out_sells == nullptr);
}

// the dynamic-LDS limit is a per-device attribute of the function: set once on every device launched on
hipError_t rollout_lds_attr(const void* fn, bool* attr, int bytes) {
  int dev = 0;
  hipError_t e = hipGetDevice(&dev);
  if (e != hipSuccess) return e;
  if (dev < 0 || dev >= 64 || !attr[dev]) {
    e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
    if (e != hipSuccess) return e;
    if (dev >= 0 && dev < 64) attr[dev] = true;
  }
  return hipSuccess;
}

}  // namespace

// grid <= 0: one workgroup per 32-env tile.  Pre-launch checks as st_qserve_launch (fixed padded dims 224 /
// 128 / 16, H + 3 <= 224) plus H >= 128 (any layout that pads to 224 inputs has H >= 190; the feature phase
// takes columns 0 .. 127 as prices) and the episode's bounds: days start .. start + steps - 1 need prices up
// to index start + steps - 1 + H <= T - 1 <= ld - 1.
extern "C" hipError_t st_qrollout_launch(const st::rollout::RolloutParams* p, int grid, hipStream_t stream) {
  using namespace st::rollout;
  if (p->E <= 0) return hipSuccess;
  if (!rollout_ok(p)) return hipErrorInvalidValue;
  static bool attr[64] = {};
  const hipError_t e = rollout_lds_attr((const void*)qrollout_kernel<false>, attr, LDS_BYTES);
  if (e != hipSuccess) return e;
  const int ntiles = (p->E + C - 1) / C;
  if (grid <= 0 || grid > ntiles) grid = ntiles;
  hipLaunchKernelGGL(qrollout_kernel<false>, dim3(grid), dim3(NT), LDS_BYTES, stream, *p);
  return hipGetLastError();
}

// The ledger instance and, with a curve, its reduction on the same stream.  Writes every output of the plain
// launch as well.  compat_env trades from the initial holding every day, so a position ledger means nothing under
// it: refused.  part_stride must be the value the kernel indexes with (steps rounded up to 32).
extern "C" hipError_t st_qrollout_ledger_launch(const st::rollout::RolloutLedger* q, int grid, hipStream_t stream) {
  using namespace st::rollout;
  const RolloutParams* p = &q->r;
  const LedgerOut& l = q->l;
  if (p->E <= 0) return hipSuccess;
  if (!rollout_ok(p) || p->compat_env != 0 || l.state_out == nullptr) return hipErrorInvalidValue;
  const bool crv = l.curve != nullptr;
  if ((l.part != nullptr) != crv) return hipErrorInvalidValue;
  if (crv && l.part_stride != ((p->steps + 31) & ~31)) return hipErrorInvalidValue;
  static bool attr[64] = {};
  const hipError_t e = rollout_lds_attr((const void*)qrollout_kernel<true>, attr, LDS_BYTES_LEDGER);
  if (e != hipSuccess) return e;
  const int ntiles = (p->E + C - 1) / C;
  if (grid <= 0 || grid > ntiles) grid = ntiles;
  hipLaunchKernelGGL(qrollout_kernel<true>, dim3(grid), dim3(NT), LDS_BYTES_LEDGER, stream, *q);
  const hipError_t r = hipGetLastError();
  if (r != hipSuccess || !crv) return r;
  hipLaunchKernelGGL(qrollout_curve_reduce_kernel, dim3((p->steps + 255) / 256), dim3(256), 0, stream, l.part, l.curve,
                     (p->E + CH - 1) / CH, p->steps, l.part_stride);
  return hipGetLastError();
}

// struct sizes of this file's launch ABI, for the host mirror's check (no HIP call)
extern "C" int st_abi_qrollout(int* out, int n) {
  const int sz[] = {(int)sizeof(st::rollout::RolloutParams)};
  const int m = (int)(sizeof(sz) / sizeof(sz[0]));
  for (int i = 0; i < n && i < m; ++i) out[i] = sz[i];
  return m;
}

extern "C" int st_abi_qrollout_ledger(int* out, int n) {
  const int sz[] = {(int)sizeof(st::rollout::RolloutLedger), (int)sizeof(st::rollout::LedgerOut)};
  const int m = (int)(sizeof(sz) / sizeof(sz[0]));
  for (int i = 0; i < n && i < m; ++i) out[i] = sz[i];
  return m;
}
