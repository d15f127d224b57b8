// Raw OHLCV minute bars -> the GRU(256) policy's feature rows (bar_features.h), MI355X-native.
//
//   * bar_features_kernel: whole histories.  The recurrence is sequential in time per series and stays so (the
//     streaming form must reproduce it bit for bit); the parallelism is over series.  A workgroup of 8 waves owns
//     64 series and moves 64-bar x 64-series tiles through LDS: global loads and the bf16 row stores run along
//     time (a wave instruction reads 256 contiguous bytes of one series, writes 1 KiB of feature rows), the
//     compute phases read the tile transposed (lane = series).  A tile plane is [64 series][65] dwords: the loads
//     write bank (s + t) with t = lane (consecutive), the compute phases read it with s = lane (consecutive too),
//     so neither side conflicts.  Most of a bar needs no recurrence (bar_features.h: bar_features_pre -- the two
//     logs, sin, cos, all seven divisions): the 8 waves share it, each taking every 8th bar of the tile;
//     then wave 0 alone walks the tile's bars in order through the thin recurrence (bar_features_rec: the GARCH
//     variance, a square root, the momentum sum).  The feature row of a bar overwrites the bar's own inputs in the
//     tile and the close plane is the close output, so one tile is 7 planes = 116,480 bytes.  Waves wait for each
//     other only inside their workgroup; no workgroup waits on another.
//   * bar_features_naive_kernel: one thread per series walking its row with stride T.  The path of N < 64 and the
//     A/B partner of benchmarks/bench_bar_features.py.
//   * bar_features_sessions_kernel: serving.  One thread per request row gathers its session's state by slot,
//     applies the same function to one bar and scatters the state back; its outputs are the feat / close tensors
//     the serve kernel (csrc/gru_serve.hip) takes, on the same stream ahead of it.
//   * minute_bars_ohlcv_kernel: the synthetic generator of csrc/gru.hip (same Philox counters, same operations)
//     that also writes the open, high, low and volume planes: test data for the above.
#include "bar_features.h"

namespace st {
namespace barf {

constexpr int TB = 64;             // bars per tile
constexpr int TS = 64;             // series per tile = lanes of the wave
constexpr int LD = TB + 1;         // dwords per series row of a plane (odd: see the header comment)
constexpr int PLANE = TS * LD;
constexpr int TW = 8;              // waves per workgroup (two per SIMD)
constexpr int NPLANE = 7;          // open, high, low, close, volume, minute, the intraday U-shape
constexpr int LDS_BYTES = NPLANE * PLANE * 4;

struct BarFeatures {
  const float* open;       // [N][T]
  const float* high;
  const float* low;
  const float* close_in;
  const float* volume;
  const int16_t* minute;   // [N][T]: index of the bar within its session, 0 .. day - 1
  const float* state_in;   // [N][8] (BarState)
  bf16_t* feat;            // [N][T][8]
  float* close;            // [N][T]
  float* state_out;        // [N][8]
  float* feat32;           // [N][T][8] fp32 or null (tests)
  int N, T, day;
  float alpha, beta;
};

struct BarSessions {
  const int* slot;         // [B], -1 (or any slot outside the table) = a padding row
  const float* ohlcv;      // [B][5]
  const int* minute;       // [B]
  float* state;            // [S][8] (BarState)
  bf16_t* feat;            // [B][8]
  float* close;            // [B]
  int B, S, day;
  float alpha, beta;
};

struct MinuteBarsOhlcv {
  float* close;            // [E][T]
  bf16_t* feat;            // [E][T][8]
  float* open;             // [E][T]
  float* high;
  float* low;
  float* volume;
  int E, T, day;
  float sigma, phi, alpha, beta, p0;
  uint32_t key0, key1;
};

ST_DEV void store_feat32(float* p, const float (&f)[BF_NF]) {
  *reinterpret_cast<float4*>(p) = make_float4(f[0], f[1], f[2], f[3]);
  *reinterpret_cast<float4*>(p + 4) = make_float4(f[4], f[5], f[6], f[7]);
}

__global__ void __launch_bounds__(TW * TS) bar_features_kernel(BarFeatures g) {
  extern __shared__ __attribute__((aligned(16))) float tile[];
  float* pO = tile;                  // open   -> row dword 0 (features 0, 1)
  float* pH = tile + PLANE;          // high   -> row dword 1 (features 2, 3)
  float* pL = tile + 2 * PLANE;      // low    -> row dword 2 (features 4, 5)
  float* pC = tile + 3 * PLANE;      // close  (never overwritten: the close output, and the next bar's reference)
  float* pV = tile + 4 * PLANE;      // volume -> the return -> row dword 3 (features 6, 7)
  float* pM = tile + 5 * PLANE;      // minute (int) -> the de-seasonalised return
  float* pU = tile + 6 * PLANE;      // the intraday U-shape
  // (packed bf16 pairs and the minute pass through the float planes as bit patterns: one type per address)
  const int lane = threadIdx.x & (TS - 1);
  const int w = threadIdx.x / TS;              // wave of the workgroup
  const int n0 = blockIdx.x * TS;
  const int rows = min(TS, g.N - n0);          // series of this workgroup (uniform)
  const bool live = lane < rows;               // lane = series in the two compute phases
  const size_t mine = (size_t)(n0 + lane);
  BarState st = {};
  if (live) st = bar_state_load(g.state_in + mine * BF_STATE);   // every wave: prev_close and vol_scale; wave 0: all
  float carry = st.prev_close;                 // the close before the tile's first bar
  const int base = lane * LD;
  for (int t0 = 0; t0 < g.T; t0 += TB) {
    const int nt = min(TB, g.T - t0);          // bars of this tile (uniform)
    // in: lane = bar, a wave takes every TW-th series
    if (lane < nt) {
#pragma unroll 2
      for (int s = w; s < rows; s += TW) {
        const size_t src = (size_t)(n0 + s) * g.T + t0 + lane;
        const int d = s * LD + lane;
        pO[d] = g.open[src];
        pH[d] = g.high[src];
        pL[d] = g.low[src];
        pC[d] = g.close_in[src];
        pV[d] = g.volume[src];
        pM[d] = __int_as_float((int)g.minute[src]);
      }
    }
    __syncthreads();
    // what needs no recurrence: lane = series, a wave takes every TW-th bar
    if (live) {
      for (int t = w; t < nt; t += TW) {
        const int d = base + t;
        const float prev = t > 0 ? pC[d - 1] : carry;
        float f[BF_NF];
        const BarPre p = bar_features_pre(prev, pO[d], pH[d], pL[d], pC[d], pV[d], __float_as_int(pM[d]), g.day, st.vol_scale, f);
        pO[d] = __uint_as_float(pack_bf2(f[0], f[1]));
        pH[d] = __uint_as_float(pack_bf2(f[2], f[3]));
        pL[d] = __uint_as_float(pack_bf2(f[4], f[5]));
        pV[d] = p.ret;
        pM[d] = p.dsr;
        pU[d] = p.ush;
        if (g.feat32 != nullptr) {
          float* o32 = g.feat32 + (mine * g.T + t0 + t) * BF_NF;
          *reinterpret_cast<float4*>(o32) = make_float4(f[0], f[1], f[2], f[3]);
          *reinterpret_cast<float2*>(o32 + 4) = make_float2(f[4], f[5]);
        }
      }
      carry = pC[base + nt - 1];
    }
    __syncthreads();
    // the recurrence, sequential in time: wave 0, lane = series
    if (w == 0 && live) {
      for (int t = 0; t < nt; ++t) {
        const int d = base + t;
        BarPre p;
        p.ret = pV[d]; p.dsr = pM[d]; p.ush = pU[d];
        float f[BF_NF];
        bar_features_rec(st, p, pC[d], g.alpha, g.beta, f);
        pV[d] = __uint_as_float(pack_bf2(f[6], f[7]));
        if (g.feat32 != nullptr)
          *reinterpret_cast<float2*>(g.feat32 + (mine * g.T + t0 + t) * BF_NF + 6) = make_float2(f[6], f[7]);
      }
    }
    __syncthreads();
    // out: lane = bar
    if (lane < nt) {
#pragma unroll 2
      for (int s = w; s < rows; s += TW) {
        const size_t dst = (size_t)(n0 + s) * g.T + t0 + lane;
        const int d = s * LD + lane;
        uint4 q;
        q.x = __float_as_uint(pO[d]); q.y = __float_as_uint(pH[d]);
        q.z = __float_as_uint(pL[d]); q.w = __float_as_uint(pV[d]);
        *reinterpret_cast<uint4*>(g.feat + dst * BF_NF) = q;
        g.close[dst] = pC[d];
      }
    }
    __syncthreads();
  }
  if (w == 0 && live) bar_state_store(g.state_out + mine * BF_STATE, st);
}

__global__ void __launch_bounds__(TS) bar_features_naive_kernel(BarFeatures g) {
  const int n = blockIdx.x * blockDim.x + threadIdx.x;
  if (n >= g.N) return;
  BarState st = bar_state_load(g.state_in + (size_t)n * BF_STATE);
  for (int t = 0; t < g.T; ++t) {
    const size_t o = (size_t)n * g.T + t;
    const float c = g.close_in[o];
    float f[BF_NF];
    bar_features_step(st, g.open[o], g.high[o], g.low[o], c, g.volume[o], (int)g.minute[o], g.day, g.alpha, g.beta,
                      f);
    *reinterpret_cast<uint4*>(g.feat + o * BF_NF) = bar_features_pack(f);
    g.close[o] = c;
    if (g.feat32 != nullptr) store_feat32(g.feat32 + o * BF_NF, f);
  }
  bar_state_store(g.state_out + (size_t)n * BF_STATE, st);
}

__global__ void __launch_bounds__(256) bar_features_sessions_kernel(BarSessions g) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= g.B) return;
  const int sl = g.slot[b];
  if (sl < 0 || sl >= g.S) return;   // a padding row: nothing read, nothing written
  float* sp = g.state + (size_t)sl * BF_STATE;
  BarState st = bar_state_load(sp);
  const float* x = g.ohlcv + (size_t)b * 5;
  const float c = x[3];
  float f[BF_NF];
  bar_features_step(st, x[0], x[1], x[2], c, x[4], g.minute[b], g.day, g.alpha, g.beta, f);
  bar_state_store(sp, st);
  *reinterpret_cast<uint4*>(g.feat + (size_t)b * BF_NF) = bar_features_pack(f);
  g.close[b] = c;
}

// csrc/gru.hip minute_bars_kernel with the bar's open, high, low and volume written out as well
__global__ void __launch_bounds__(256) minute_bars_ohlcv_kernel(MinuteBarsOhlcv g) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= g.E) return;
  uint32_t c0 = (uint32_t)e, c1 = 0xFFFFFFFFu, c2 = 0u, c3 = 0x4D424152u;
  philox4x32(c0, c1, c2, c3, g.key0, g.key1);
  float c = g.p0 * (0.5f + u24(c0));
  float var = g.sigma * g.sigma, rprev = 0.f;
  const float omega = g.sigma * g.sigma * (1.f - g.alpha - g.beta);
  float r1 = 0.f, r2 = 0.f, r3 = 0.f, r4 = 0.f;
  for (int t = 0; t < g.T; ++t) {
    uint32_t a0 = (uint32_t)e, a1 = (uint32_t)t, a2 = 0u, a3 = 0x4D424152u;
    philox4x32(a0, a1, a2, a3, g.key0, g.key1);
    const float u0 = fmaxf(u24(a0), 1e-7f), u1 = u24(a1), u2 = fmaxf(u24(a2), 1e-7f), u3 = u24(a3);
    const float rad0 = sqrtf(-2.f * logf(u0)), rad1 = sqrtf(-2.f * logf(u2));
    const float n1 = rad0 * cosf(6.2831853f * u1), n2 = rad0 * sinf(6.2831853f * u1);
    const float n3 = rad1 * cosf(6.2831853f * u3), n4 = rad1 * sinf(6.2831853f * u3);
    const int tod = t % g.day;
    const float x = (2.f * (float)tod / (float)g.day) - 1.f;
    const float ush = 1.f + 0.8f * x * x;
    const float sig = sqrtf(var) * ush;
    const float ret = g.phi * rprev + sig * n1;
    const float open = c;
    c = open * expf(ret);
    const float hi = fmaxf(open, c) * expf(0.5f * sig * fabsf(n2));
    const float lo = fminf(open, c) * expf(-0.5f * sig * fabsf(n3));
    const float vol = expf(0.5f * n4) * ush;
    const float dsr = ret / ush;
    var = omega + g.alpha * dsr * dsr + g.beta * var;
    const float mom = ret + r1 + r2 + r3 + r4;
    r4 = r3; r3 = r2; r2 = r1; r1 = ret;
    rprev = ret;
    const float ang = 6.2831853f * (float)tod / (float)g.day;
    const size_t o = (size_t)e * g.T + t;
    g.close[o] = c;
    g.open[o] = open;
    g.high[o] = hi;
    g.low[o] = lo;
    g.volume[o] = vol;
    uint4 w;
    w.x = pack_bf2(ret * 100.f, (hi - lo) / c * 100.f);
    w.y = pack_bf2((c - lo) / fmaxf(hi - lo, 1e-12f) - 0.5f, logf(vol));
    w.z = pack_bf2(sinf(ang), cosf(ang));
    w.w = pack_bf2(mom * 100.f, sig * 100.f);
    *reinterpret_cast<uint4*>(g.feat + o * BF_NF) = w;
  }
}

}  // namespace barf
}  // namespace st

extern "C" int st_bar_features_lds_bytes() { return st::barf::LDS_BYTES; }

// variant 0: the tiled kernel from 64 series on, else one thread per series; 1: one thread per series; 2: tiled
extern "C" hipError_t st_bar_features_launch(const st::barf::BarFeatures* p, int variant, hipStream_t stream) {
  using namespace st::barf;
  if (p == nullptr || p->N < 1 || p->T < 1 || p->day < 1 || variant < 0 || variant > 2 || p->open == nullptr ||
      p->high == nullptr || p->low == nullptr || p->close_in == nullptr || p->volume == nullptr ||
      p->minute == nullptr || p->state_in == nullptr || p->feat == nullptr || p->close == nullptr ||
      p->state_out == nullptr)
    return hipErrorInvalidValue;
  const int grid = (p->N + TS - 1) / TS;
  const bool tiled = variant == 2 || (variant == 0 && p->N >= TS);
  if (!tiled) {
    hipLaunchKernelGGL(bar_features_naive_kernel, dim3(grid), dim3(TS), 0, stream, *p);
    return hipGetLastError();
  }
  // the dynamic-LDS limit is a per-device attribute of the function: set once on every device launched on
  static bool attr[64] = {};
  int dev = 0;
  hipError_t e = hipGetDevice(&dev);
  if (e != hipSuccess) return e;
  const bool slot = dev >= 0 && dev < 64;
  if (!slot || !attr[dev]) {
    e = hipFuncSetAttribute((const void*)bar_features_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, LDS_BYTES);
    if (e != hipSuccess) return e;
    if (slot) attr[dev] = true;
  }
  hipLaunchKernelGGL(bar_features_kernel, dim3(grid), dim3(TW * TS), LDS_BYTES, stream, *p);
  return hipGetLastError();
}

extern "C" hipError_t st_bar_features_sessions(const st::barf::BarSessions* p, hipStream_t stream) {
  using namespace st::barf;
  if (p == nullptr || p->B < 1 || p->S < 1 || p->day < 1 || p->slot == nullptr || p->ohlcv == nullptr ||
      p->minute == nullptr || p->state == nullptr || p->feat == nullptr || p->close == nullptr)
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(bar_features_sessions_kernel, dim3((p->B + 255) / 256), dim3(256), 0, stream, *p);
  return hipGetLastError();
}

extern "C" hipError_t st_minute_bars_ohlcv(const st::barf::MinuteBarsOhlcv* g, hipStream_t s) {
  using namespace st::barf;
  if (g == nullptr || g->E < 1 || g->T < 1 || g->day < 1 || g->close == nullptr || g->feat == nullptr ||
      g->open == nullptr || g->high == nullptr || g->low == nullptr || g->volume == nullptr)
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(minute_bars_ohlcv_kernel, dim3((g->E + 255) / 256), dim3(256), 0, s, *g);
  return hipGetLastError();
}

// struct sizes of this file's launch ABI, for the host mirrors' check (no HIP call)
extern "C" int st_abi_bar_features(int* out, int n) {
  const int sz[] = {(int)sizeof(st::barf::BarFeatures), (int)sizeof(st::barf::BarSessions),
                    (int)sizeof(st::barf::MinuteBarsOhlcv)};
  const int m = (int)(sizeof(sz) / sizeof(sz[0]));
  for (int i = 0; i < n && i < m; ++i) out[i] = sz[i];
  return m;
}
