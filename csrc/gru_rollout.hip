// Backtest of a frozen GRU(256) policy on CDNA4 (gfx950): whole episodes of the minute-bar env in one launch.
//
// For env e and bar t = start .. start + steps - 1 the arithmetic of a bar is the actors' (csrc/gru.hip) on the
// weights st_gru_pack produced, from the same source: the statements of gru_weights.h and gru_net_tile.h,
// gru_q_row / quant_h of gru_common.h and the trading rule of minute_rule.h; no rounding point of its own.
// What differs is what surrounds it:
//  * a workgroup (8 waves, 32 envs) owns its envs for the whole launch: h (fp32, accumulator layout), the
//    position, entry price and running return never leave the chip; the weights are loaded once;
//  * every env is at the same bar, so episode ends (consecutive ep_len-bar stretches from `origin`) are
//    uniform: no done flags, no restart draws, the next bar is always t + 1 and is prefetched one env
//    phase ahead; each bar is read from HBM once;
//  * nothing is written per bar unless a trace is asked for; greedy runs make no Philox draws;
//  * the barriers wait for LDS traffic only: the prefetch and the trace stores stay in flight across them.
// Oracle: sharetrade/serve/gru_rollout.py::reference_gru_rollout.
//
// The kernel is a template on LEDGER, so the bar loop is defined once and the plain instance
// (gru_rollout_kernel<false>, st_gru_rollout_launch) carries none of the ledger's registers.  The ledger instance
// (gru_rollout_kernel<true>, st_gru_rollout_ledger_launch) also keeps, per env and in wave 0's env phase, the
// running equity curve (peak, deepest and longest drawdown, sum of squared rewards), the return and trades of
// every episode, the round trips (count, wins, sums of winning and losing trips) and, per bar, the sum of the
// rewards of the chunk's envs, which gru_curve_reduce_kernel adds over the chunks to the portfolio curve.  All of
// it is fp32 in bar order with unfused operations.  Oracle: ...::ledger_from_trace.
#include "gru_common.h"
#include "minute_rule.h"

namespace st {
namespace grollout {

struct GruRollout : GruNetW {  // the packed weights first (gru_common.h)
  const bf16_t* feat;          // [E][T][RMF]
  const float* close;          // [E][T]
  const float* ret;            // [E][T]
  const float* h0;             // [E][RH] or null = 0
  const int* position;         // [E] or null = flat
  const float* entry;          // [E] or null = 0
  float* out_ret;              // [E] sum of rewards in bar order
  int* out_trades;             // [E] position changes
  int* out_long;               // [E] bars held long
  int* out_position;           // [E]
  float* out_entry;            // [E]
  float* out_h;                // [E][RH] or null
  signed char* tr_actions;     // [E][steps] or null
  float* tr_q;                 // [E][steps][3] or null
  float* tr_reward;            // [E][steps] or null
  int E, T, start, steps, origin, ep_len;
  float eps, cost, inv_ep_len; // eps = inf: greedy, no draws
  uint32_t key0, key1, env_offset;   // draw counter: (env_offset + e, t, 0, "GRB1")
};
ST_FOLLOWS_NETW(GruRollout, feat)

// What the ledger instance writes besides GruRollout's outputs.  {ep_ret, ep_trades, state_out, stats} are given
// together or not at all, and so are {part, curve}; state_in null = a fresh ledger (zeros).
struct GruLedgerOut {
  float* ep_ret;               // [E][n_ep] return of episode column k (the first and last may be partial)
  int* ep_trades;              // [E][n_ep]
  const uint4* state_in;       // [E][2] {cum, peak, trip, ep | run, ep_tr, 0, 0} of the piece before, or null
  uint4* state_out;            // [E][2]
  uint4* stats;                // [E][2] {max_dd, sumsq, win_sum, loss_sum | dd_bars, trips, wins, 0} of this piece
  float* part;                 // [chunks][part_stride] per-bar sum of a chunk's rewards
  float* curve;                // [steps] sum of part over the chunks in ascending order
  int n_ep, part_stride;       // (start + steps - 1 - es0) / ep_len + 1; steps rounded up to 32
};

struct GruRolloutLedger {
  GruRollout r;
  GruLedgerOut l;
};

struct Lds {
  static constexpr int WX = 0;                                   // RW*6*64 s8v
  static constexpr int X = WX + RW * 6 * 64 * 16;                // [2][RN*XS] bf16
  static constexpr int H8 = X + 2 * RN * XS * 2;                 // [2][RN*HS] bytes
  static constexpr int SC = H8 + 2 * RN * HS;                    // [2][RN*SCS] int
  static constexpr int B = SC + 2 * RN * SCS * 4;                // [4*RH] float
  static constexpr int WQ = B + 4 * RH * 4;                      // [4*RH] float
  static constexpr int QP = WQ + 4 * RH * 4;                     // [RW][3][RN] float
  static constexpr int BYTES = QP + RW * 3 * RN * 4;
};
static_assert(Lds::BYTES <= 160 * 1024, "rollout LDS");
static_assert(Lds::X % 16 == 0 && Lds::H8 % 16 == 0 && Lds::SC % 16 == 0 && Lds::B % 16 == 0, "16-byte carves");

// Sum over the 32 lanes of a half of the wave by the fixed tree of ledger_from_trace's chunk_sums: the pairs 16,
// 8, 4, 2, 1 lanes apart, lane l taking l + w at every level.  On the VALU (a row swap, then DPP row_shl adds: no
// LDS round trip); lane 0 holds the sum and it is returned wave-uniform.  The wave's halves carry the same envs.
ST_DEV float half_tree_sum(float v) {
  const uint32_t b = __float_as_uint(v);
  const auto r16 = __builtin_amdgcn_permlane16_swap(b, b, false, false);
  v = __fadd_rn(__uint_as_float((uint32_t)r16[0]), __uint_as_float((uint32_t)r16[1]));   // rows 0 + 1 (2 + 3)
  v = __fadd_rn(v, __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(v), 0x108, 0xF, 0xF, true)));   // row_shl:8
  v = __fadd_rn(v, __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(v), 0x104, 0xF, 0xF, true)));
  v = __fadd_rn(v, __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(v), 0x102, 0xF, 0xF, true)));
  v = __fadd_rn(v, __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(v), 0x101, 0xF, 0xF, true)));
  return __uint_as_float(__builtin_amdgcn_readfirstlane(__float_as_uint(v)));
}

// the launch struct of an instance, and its two halves
template <bool LEDGER> struct ArgsOf { using type = GruRollout; };
template <> struct ArgsOf<true> { using type = GruRolloutLedger; };
ST_DEV const GruRollout& plain_of(const GruRollout& q) { return q; }
ST_DEV const GruRollout& plain_of(const GruRolloutLedger& q) { return q.r; }
ST_DEV GruLedgerOut ledger_of(const GruRollout&) { return GruLedgerOut{}; }
ST_DEV const GruLedgerOut& ledger_of(const GruRolloutLedger& q) { return q.l; }

template <bool LEDGER>
__global__ void __launch_bounds__(RT, 1) gru_rollout_kernel(typename ArgsOf<LEDGER>::type q) {
  const GruRollout& p = plain_of(q);
  const GruLedgerOut& L = ledger_of(q);   // (read by the ledger instance only)
  extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
  const s8v* sWx = reinterpret_cast<const s8v*>(lds + Lds::WX);
  bf16_t* sX = reinterpret_cast<bf16_t*>(lds + Lds::X);
  unsigned char* sH8 = lds + Lds::H8;
  int* sSc = reinterpret_cast<int*>(lds + Lds::SC);
  float* sB = reinterpret_cast<float*>(lds + Lds::B);
  float* sWq = reinterpret_cast<float*>(lds + Lds::WQ);
  float* sQp = reinterpret_cast<float*>(lds + Lds::QP);

  const int tid = threadIdx.x, lane = tid & 63, l16 = lane & 15, g4 = lane >> 4;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
#include "gru_weights.h"
  const bool greedy = __builtin_isinf(p.eps);
  const int nchunks = (p.E + RN - 1) / RN, steps = p.steps;
  // start of the episode that holds bar `start` (origin <= start)
  const int es0 = p.origin + (int)(((long long)p.start - p.origin) / p.ep_len) * p.ep_len;
  __syncthreads();

  for (int chunk = blockIdx.x; chunk < nchunks; chunk += gridDim.x) {
    const int e0 = chunk * RN;
    float hr[2][2][4];
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
      for (int n = 0; n < 2; ++n) {
        const int e = min(e0 + 16 * n + l16, p.E - 1), u0 = 32 * wave + 16 * m + 4 * g4;
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (p.h0 != nullptr) v = *reinterpret_cast<const float4*>(p.h0 + (size_t)e * RH + u0);
        hr[m][n][0] = v.x; hr[m][n][1] = v.y; hr[m][n][2] = v.z; hr[m][n][3] = v.w;
      }
    quant_h(hr, sH8, sSc, wave, l16, g4);
    // env state lives in wave 0: lanes l and l + 32 both carry env e0 + (l & 31); rows past E re-read
    // env E - 1 and store nothing
    const int row_ = lane & (RN - 1);
    const int me = min(e0 + row_, p.E - 1);
    const bool writer = lane < RN;
    const bool live = writer && e0 + lane < p.E;
    int pz_ = 0, ntr_ = 0, nlong_ = 0;
    float en_ = 0.f, sum_ = 0.f;
    float cA = 0.f, cB = 0.f, rA = 0.f, rB = 0.f;   // close / ret of bars t, t + 1
    uint4 fB = {0u, 0u, 0u, 0u};                     // features of bar t + 1
    // the ledger (LEDGER instance, wave 0): carried from piece to piece ...
    float cum_ = 0.f, peak_ = 0.f, trip_ = 0.f, ep_ = 0.f;
    int run_ = 0, eptr_ = 0;
    // ... and of this piece alone
    float mdd_ = 0.f, ssq_ = 0.f, wsum_ = 0.f, lsum_ = 0.f, pb_ = 0.f;
    int ddb_ = 0, trips_ = 0, wins_ = 0;
    if (wave == 0) {
      if constexpr (LEDGER) {
        if (L.state_in != nullptr) {
          const uint4 a = L.state_in[2 * (size_t)me], b = L.state_in[2 * (size_t)me + 1];
          cum_ = __uint_as_float(a.x); peak_ = __uint_as_float(a.y);
          trip_ = __uint_as_float(a.z); ep_ = __uint_as_float(a.w);
          run_ = (int)b.x; eptr_ = (int)b.y;
        }
      }
      if (p.position != nullptr) pz_ = p.position[me];
      if (p.entry != nullptr) en_ = p.entry[me];
      const size_t o = (size_t)me * p.T + p.start;   // start + 1 <= T - 1 (launcher)
      cA = p.close[o];
      cB = p.close[o + 1];
      rA = p.ret[o];
      rB = p.ret[o + 1];
      fB = *reinterpret_cast<const uint4*>(p.feat + (o + 1) * RMF);
      const uint4 f0 = *reinterpret_cast<const uint4*>(p.feat + o * RMF);
      if (writer) minute_x_row(sX + lane * XS, f0, minute_x_env(pz_, en_, cA, p.start - es0, p.inv_ep_len));
    }
    lds_barrier();

    int es = es0, k = 0;   // k: episode column of bar t
#pragma unroll 1
    for (int s = 0; s < steps; ++s) {
      const int cur = s & 1, nxt = cur ^ 1;
      const int t = p.start + s;
      const bool done = (t + 1 - es) >= p.ep_len;   // uniform: every env is at bar t
      const bf16_t* cX = sX + cur * RN * XS;
      const unsigned char* cH = sH8 + cur * RN * HS;
      const int* cS = sSc + cur * RN * SCS;
#pragma unroll
      for (int n = 0; n < 2; ++n) {
        float (&hrt)[2][2][4] = hr;
#define GRU_TILE_STAMP
#include "gru_net_tile.h"
#undef GRU_TILE_STAMP
      }
      // an episode's last bar: the next one starts from h = 0 (Q of this bar is already taken)
      if (done) {
#pragma unroll
        for (int m = 0; m < 2; ++m)
#pragma unroll
          for (int n = 0; n < 2; ++n)
#pragma unroll
            for (int i = 0; i < 4; ++i) hr[m][n][i] = 0.f;
      }
      quant_h(hr, sH8 + nxt * RN * HS, sSc + nxt * RN * SCS, wave, l16, g4);
      lds_barrier();
      // ---------------------------------------------------------- env step (wave 0)
      if (wave == 0) {
        float q[3];
        gru_q_row(sWq, sQp, row_, q);
        int a = first_max3(q[0], q[1], q[2]);
        if (!greedy) a = eps_greedy_draw(a, p.env_offset + (uint32_t)(e0 + row_), (uint32_t)t, p.key0, p.key1, p.eps);
        const MinuteMove mv = minute_move(a, pz_, en_, cA, rA, p.cost);
        sum_ += mv.reward;
        ntr_ += mv.trade ? 1 : 0;
        nlong_ += mv.position;
        if constexpr (LEDGER) {
          const float rw = mv.reward;
          const bool last = s == steps - 1;
          // running curve
          cum_ = __fadd_rn(cum_, rw);
          peak_ = cum_ > peak_ ? cum_ : peak_;
          const float dd = __fsub_rn(peak_, cum_);
          mdd_ = dd > mdd_ ? dd : mdd_;
          run_ = cum_ < peak_ ? run_ + 1 : 0;
          ddb_ = max(ddb_, run_);
          ssq_ = __fadd_rn(ssq_, __fmul_rn(rw, rw));
          // episode ledger
          ep_ = __fadd_rn(ep_, rw);
          eptr_ += mv.trade ? 1 : 0;
          if ((done || last) && live && L.ep_ret != nullptr) {
            const size_t o = (size_t)(e0 + lane) * (size_t)L.n_ep + (size_t)k;
            L.ep_ret[o] = ep_;
            L.ep_trades[o] = eptr_;
          }
          if (done) { ep_ = 0.f; eptr_ = 0; }
          // round trips (pz_ is still the position before this bar's action)
          if (mv.trade && mv.position == 1) trip_ = rw;
          else if (pz_ != 0) trip_ = __fadd_rn(trip_, rw);
          if ((mv.trade && mv.position == 0) || (done && mv.position == 1)) {
            const bool won = trip_ > 0.f;
            ++trips_;
            wins_ += won ? 1 : 0;
            wsum_ = won ? __fadd_rn(wsum_, trip_) : wsum_;
            lsum_ = won ? lsum_ : __fadd_rn(lsum_, trip_);
            trip_ = 0.f;
          }
          // portfolio curve: the chunk's sum of this bar's rewards (rows past E contribute 0); lane s & 31 keeps
          // it and a full 128-byte row of 32 bars goes out at once
          if (L.part != nullptr) {
            const float v = half_tree_sum(e0 + row_ < p.E ? rw : 0.f);
            pb_ = row_ == (s & 31) ? v : pb_;
            if (((s & 31) == 31 || last) && writer && lane <= (s & 31))
              L.part[(size_t)chunk * (size_t)L.part_stride + (size_t)((s & ~31) + lane)] = pb_;
          }
        }
        // after an episode's last bar: flat at no cost, entry cleared
        pz_ = done ? 0 : mv.position;
        en_ = done ? 0.f : mv.entry;
        if (writer)
          minute_x_row(sX + nxt * RN * XS + lane * XS, fB,
                       minute_x_env(pz_, en_, cB, done ? 0 : t + 1 - es, p.inv_ep_len));
        if (live) {
          const size_t o = (size_t)(e0 + lane) * (size_t)steps + (size_t)s;
          if (p.tr_actions != nullptr) p.tr_actions[o] = (signed char)a;
          if (p.tr_q != nullptr) {
            p.tr_q[3 * o + 0] = q[0];
            p.tr_q[3 * o + 1] = q[1];
            p.tr_q[3 * o + 2] = q[2];
          }
          if (p.tr_reward != nullptr) p.tr_reward[o] = mv.reward;
        }
        // bar t + 2 for the next env phase (issued last: a whole MFMA phase to land)
        cA = cB;
        rA = rB;
        const size_t o1 = (size_t)me * p.T + min(t + 2, p.T - 1);
        cB = p.close[o1];
        rB = p.ret[o1];
        fB = *reinterpret_cast<const uint4*>(p.feat + o1 * RMF);
      }
      lds_barrier();
      if (done) { es = t + 1; ++k; }
    }
    // results
    if (p.out_h != nullptr) {
#pragma unroll
      for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int n = 0; n < 2; ++n) {
          const int e = e0 + 16 * n + l16, u0 = 32 * wave + 16 * m + 4 * g4;
          if (e < p.E)
            *reinterpret_cast<float4*>(p.out_h + (size_t)e * RH + u0) =
                make_float4(hr[m][n][0], hr[m][n][1], hr[m][n][2], hr[m][n][3]);
        }
    }
    if (wave == 0 && live) {
      const int e = e0 + lane;
      p.out_ret[e] = sum_;
      p.out_trades[e] = ntr_;
      p.out_long[e] = nlong_;
      p.out_position[e] = pz_;
      p.out_entry[e] = en_;
      if constexpr (LEDGER) {
        if (L.stats != nullptr) {
          L.state_out[2 * (size_t)e] = make_uint4(__float_as_uint(cum_), __float_as_uint(peak_),
                                                  __float_as_uint(trip_), __float_as_uint(ep_));
          L.state_out[2 * (size_t)e + 1] = make_uint4((uint32_t)run_, (uint32_t)eptr_, 0u, 0u);
          L.stats[2 * (size_t)e] = make_uint4(__float_as_uint(mdd_), __float_as_uint(ssq_),
                                              __float_as_uint(wsum_), __float_as_uint(lsum_));
          L.stats[2 * (size_t)e + 1] = make_uint4((uint32_t)ddb_, (uint32_t)trips_, (uint32_t)wins_, 0u);
        }
      }
    }
    lds_barrier();
  }
}

// curve[s] = sum over the chunks, in ascending order from 0.f, of part[chunk][s]: one thread per bar
__global__ void __launch_bounds__(256) gru_curve_reduce_kernel(const float* __restrict__ part,
                                                               float* __restrict__ curve, int nchunks, int steps,
                                                               int part_stride) {
  const int s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= steps) return;
  float acc = 0.f;
  for (int c = 0; c < nchunks; ++c) acc = __fadd_rn(acc, part[(size_t)c * (size_t)part_stride + (size_t)s]);
  curve[s] = acc;
}

}  // namespace grollout
}  // namespace st

extern "C" int st_gru_rollout_lds_bytes() { return st::grollout::Lds::BYTES; }
// nothing is staged per block of bars (the draws are made in the env phase of their bar)
extern "C" int st_gru_rollout_block() { return 0; }

namespace {

// Every reward needs close[t + 1]: start + steps <= T - 1.
bool rollout_ok(const st::grollout::GruRollout* p) {
  return !(p->E < 1 || p->steps < 1 || p->ep_len < 1 || p->origin > p->start || p->start < 0 ||
           (long long)p->start + p->steps > (long long)p->T - 1 || !st::net_ok(*p) || p->feat == nullptr ||
           p->close == nullptr || p->ret == nullptr || p->out_ret == nullptr || p->out_trades == nullptr ||
           p->out_long == nullptr || p->out_position == nullptr || p->out_entry == nullptr);
}

// the dynamic-LDS limit is a per-device attribute of the function: set once on every device launched on
hipError_t rollout_lds_attr(const void* fn, bool* attr) {
  int dev = 0;
  hipError_t e = hipGetDevice(&dev);
  if (e != hipSuccess) return e;
  if (dev < 0 || dev >= 64 || !attr[dev]) {
    e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, st::grollout::Lds::BYTES);
    if (e != hipSuccess) return e;
    if (dev >= 0 && dev < 64) attr[dev] = true;
  }
  return hipSuccess;
}

}  // namespace

// grid <= 0: one workgroup per 32-env chunk.
extern "C" hipError_t st_gru_rollout_launch(const st::grollout::GruRollout* p, int grid, hipStream_t stream) {
  using namespace st::grollout;
  if (!rollout_ok(p)) return hipErrorInvalidValue;
  static bool attr[64] = {};
  const hipError_t e = rollout_lds_attr((const void*)gru_rollout_kernel<false>, attr);
  if (e != hipSuccess) return e;
  const int nchunks = (p->E + st::RN - 1) / st::RN;
  if (grid <= 0 || grid > nchunks) grid = nchunks;
  hipLaunchKernelGGL(gru_rollout_kernel<false>, dim3(grid), dim3(st::RT), Lds::BYTES, stream, *p);
  return hipGetLastError();
}

// The ledger instance and, with a curve, its reduction on the same stream.  Writes every output of the plain
// launch as well.  n_ep and part_stride must be the values the kernel indexes with.
extern "C" hipError_t st_gru_rollout_ledger_launch(const st::grollout::GruRolloutLedger* q, int grid,
                                                   hipStream_t stream) {
  using namespace st::grollout;
  const GruRollout* p = &q->r;
  const GruLedgerOut& l = q->l;
  if (!rollout_ok(p)) return hipErrorInvalidValue;
  const bool led = l.stats != nullptr, crv = l.curve != nullptr;
  if ((l.ep_ret != nullptr) != led || (l.ep_trades != nullptr) != led || (l.state_out != nullptr) != led ||
      (l.part != nullptr) != crv)
    return hipErrorInvalidValue;
  const long long es0 = p->origin + ((long long)p->start - p->origin) / p->ep_len * p->ep_len;
  if (led && l.n_ep != (int)(((long long)p->start + p->steps - 1 - es0) / p->ep_len + 1)) return hipErrorInvalidValue;
  if (crv && l.part_stride != ((p->steps + 31) & ~31)) return hipErrorInvalidValue;
  static bool attr[64] = {};
  const hipError_t e = rollout_lds_attr((const void*)gru_rollout_kernel<true>, attr);
  if (e != hipSuccess) return e;
  const int nchunks = (p->E + st::RN - 1) / st::RN;
  if (grid <= 0 || grid > nchunks) grid = nchunks;
  hipLaunchKernelGGL(gru_rollout_kernel<true>, dim3(grid), dim3(st::RT), Lds::BYTES, stream, *q);
  hipError_t r = hipGetLastError();
  if (r != hipSuccess || !crv) return r;
  hipLaunchKernelGGL(gru_curve_reduce_kernel, dim3((p->steps + 255) / 256), dim3(256), 0, stream, l.part, l.curve,
                     nchunks, p->steps, l.part_stride);
  return hipGetLastError();
}

// struct sizes of this file's launch ABI, for the host mirror's check (no HIP call)
extern "C" int st_abi_gru_rollout(int* out, int n) {
  const int sz[] = {(int)sizeof(st::grollout::GruRollout)};
  const int m = (int)(sizeof(sz) / sizeof(sz[0]));
  for (int i = 0; i < n && i < m; ++i) out[i] = sz[i];
  return m;
}

extern "C" int st_abi_gru_rollout_ledger(int* out, int n) {
  const int sz[] = {(int)sizeof(st::grollout::GruRolloutLedger), (int)sizeof(st::grollout::GruLedgerOut)};
  const int m = (int)(sizeof(sz) / sizeof(sz[0]));
  for (int i = 0; i < n && i < m; ++i) out[i] = sz[i];
  return m;
}
