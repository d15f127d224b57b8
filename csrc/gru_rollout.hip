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
#include "gru_common.h"
#include "minute_rule.h"

namespace st {
namespace grollout {

struct GruRollout {
  const i8v* whh8;             // packed weights (GruPack)
  const int* whhs;
  const s8v* wih;
  const float* bias4;
  const float* wq;
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

__global__ void __launch_bounds__(RT, 1) gru_rollout_kernel(GruRollout p) {
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
    if (wave == 0) {
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

    int es = es0;
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
      if (done) es = t + 1;
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
    }
    lds_barrier();
  }
}

}  // namespace grollout
}  // namespace st

extern "C" int st_gru_rollout_lds_bytes() { return st::grollout::Lds::BYTES; }
// nothing is staged per block of bars (the draws are made in the env phase of their bar)
extern "C" int st_gru_rollout_block() { return 0; }

// grid <= 0: one workgroup per 32-env chunk.  Every reward needs close[t + 1]: start + steps <= T - 1.
extern "C" hipError_t st_gru_rollout_launch(const st::grollout::GruRollout* p, int grid, hipStream_t stream) {
  using namespace st::grollout;
  if (p->E < 1 || p->steps < 1 || p->ep_len < 1 || p->origin > p->start || p->start < 0 ||
      (long long)p->start + p->steps > (long long)p->T - 1 || p->whh8 == nullptr || p->whhs == nullptr ||
      p->wih == nullptr || p->bias4 == nullptr || p->wq == nullptr || p->feat == nullptr || p->close == nullptr ||
      p->ret == nullptr || p->out_ret == nullptr || p->out_trades == nullptr || p->out_long == nullptr ||
      p->out_position == nullptr || p->out_entry == nullptr)
    return hipErrorInvalidValue;
  // the dynamic-LDS limit is a per-device attribute of the function: set once on every device launched on
  static bool attr[64] = {};
  int dev = 0;
  hipError_t e = hipGetDevice(&dev);
  if (e != hipSuccess) return e;
  if (dev < 0 || dev >= 64 || !attr[dev]) {
    e = hipFuncSetAttribute((const void*)gru_rollout_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, Lds::BYTES);
    if (e != hipSuccess) return e;
    if (dev >= 0 && dev < 64) attr[dev] = true;
  }
  const int nchunks = (p->E + st::RN - 1) / st::RN;
  if (grid <= 0 || grid > nchunks) grid = nchunks;
  hipLaunchKernelGGL(gru_rollout_kernel, dim3(grid), dim3(st::RT), Lds::BYTES, stream, *p);
  return hipGetLastError();
}

// struct sizes of this file's launch ABI, for the host mirror's check (no HIP call)
extern "C" int st_abi_gru_rollout(int* out, int n) {
  const int sz[] = {(int)sizeof(st::grollout::GruRollout)};
  const int m = (int)(sizeof(sz) / sizeof(sz[0]));
  for (int i = 0; i < n && i < m; ++i) out[i] = sz[i];
  return m;
}
