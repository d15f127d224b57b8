// Serving a frozen GRU(256) policy on CDNA4 (gfx950): one launch advances B sessions by one bar each.
//
// A session is a slot of a device-resident table: h [S][RH] fp32 and one 64-byte scalar record per slot
// (ServeRec).  A request row names its slot and brings the bar (8 bf16 features, close).  The arithmetic of a
// row is exactly one bar of gru_rollout_kernel (csrc/gru_rollout.hip) on the weights st_gru_pack produced -- the
// same source (gru_weights.h, gru_net_tile.h, gru_common.h, the trading rule of minute_rule.h), no rounding point
// of its own.
// What differs is what surrounds the bar:
//  * h and the scalars are gathered by slot and scattered back to it; a row whose slot is outside [0, S) (-1 is
//    the padding value) or past B loads nothing from the table, stores nothing and answers action -1;
//  * the episode state is per row: done = elapsed + 1 >= ep_len flattens that row at no cost, clears its entry,
//    stores h = 0 and returns elapsed to 0; flag bit 0 starts the row fresh before its bar;
//  * the next close is not known, so a bar's reward is realised when the session's next bar arrives:
//    (float)pend_pos * ((close / last_close - 1) * 100) - pend_fee, the operation order of bar_returns +
//    minute_move;
//  * the draw counter is (draw_id, bars served, 0, "GRB1") under the actors' key; eps = inf is greedy, no draws.
// Staging: registers.  While a chunk's MFMA phase runs, the next chunk's h rows (16 VGPRs a lane), records,
// bars and flags and the slots of the chunk after it are in flight; the barriers wait for LDS traffic only.
// Two rows of one launch naming the same slot race; the host refuses such a batch.
// Oracle: sharetrade/serve/gru_serve.py::reference_gru_serve.
#include "gru_common.h"
#include "minute_rule.h"

namespace st {
namespace gserve {

struct GruServe : GruNetW {    // the packed weights first (gru_common.h)
  const int* slot;             // [B]
  const bf16_t* feat;          // [B][RMF]
  const float* close;          // [B]
  const unsigned char* flags;  // [B] or null; bit 0: a new episode starts at this bar
  float* h;                    // [S][RH] session table
  int* rec;                    // [S][REC] session table (ServeRec)
  signed char* action;         // [B]; -1 on a padding row
  int* position;               // [B] after the action (before any end-of-episode flattening)
  float* reward;               // [B] realised reward of the session's previous bar
  float* q;                    // [B][3] or null
  int B, S, ep_len;
  float eps, cost, inv_ep_len; // eps = inf: greedy, no draws
  uint32_t key0, key1;
};
ST_FOLLOWS_NETW(GruServe, slot)

// the scalar record of a slot, 16 dwords (the first 11 in use)
constexpr int REC = 16;
struct ServeRec {
  int position;
  float entry;
  int elapsed;         // bars into the episode
  float last_close;    // 0 = none yet
  int pend_pos;        // the pending reward: pend_pos * r - pend_fee once the next close is known
  float pend_fee;
  float ret;           // running sum of realised rewards
  int trades;
  int nlong;
  uint32_t bars;       // bars served: word 1 of the draw counter
  uint32_t draw_id;    // word 0 of the draw counter
};
static_assert(sizeof(ServeRec) == 44 && sizeof(ServeRec) <= REC * 4, "record layout");

struct Lds {
  static constexpr int WX = 0;                                   // RW*6*64 s8v
  static constexpr int X = WX + RW * 6 * 64 * 16;                // [RN*XS] bf16
  static constexpr int H8 = X + RN * XS * 2;                     // [RN*HS] bytes
  static constexpr int SC = H8 + RN * HS;                        // [RN*SCS] int
  static constexpr int B = SC + RN * SCS * 4;                    // [4*RH] float
  static constexpr int WQ = B + 4 * RH * 4;                      // [4*RH] float
  static constexpr int QP = WQ + 4 * RH * 4;                     // [RW][3][RN] float
  static constexpr int DN = QP + RW * 3 * RN * 4;                // [RN] int: the row's episode ends at this bar
  static constexpr int BYTES = DN + RN * 4;
};
static_assert(Lds::BYTES <= 160 * 1024, "serve LDS");
static_assert(Lds::X % 16 == 0 && Lds::H8 % 16 == 0 && Lds::SC % 16 == 0 && Lds::B % 16 == 0, "16-byte carves");

// a chunk's request rows and table rows as the lanes hold them
struct Stage {
  float4 h[2][2];     // [m][n]: units 32 wave + 16 m + 4 g4 .. of row 16 n + l16
  int fl[2];          // flags of rows 16 n + l16
  uint4 r0, r1, r2;   // wave 0: the record of row lane & 31
  uint4 ft;           // wave 0: the bar's features
  float cl;           // wave 0: close
  int fle;            // wave 0: flags
};

// (64-bit row: two grid strides past the last chunk of a large batch do not wrap)
ST_DEV int load_slot(const GruServe& p, long long row) { return row < (long long)p.B ? p.slot[row] : -1; }
ST_DEV bool slot_ok(const GruServe& p, int s) { return (unsigned)s < (unsigned)p.S; }

ST_DEV void load_stage(const GruServe& p, Stage& st, long long r0, const int (&sl)[2], int sle, int wave, int lane,
                       int l16, int g4) {
  const uint4 z4 = {0u, 0u, 0u, 0u};
#pragma unroll
  for (int n = 0; n < 2; ++n) {
    const bool ok = slot_ok(p, sl[n]);
    st.fl[n] = (ok && p.flags != nullptr) ? (int)p.flags[r0 + 16 * n + l16] : 0;
#pragma unroll
    for (int m = 0; m < 2; ++m) {
      const int u0 = 32 * wave + 16 * m + 4 * g4;
      st.h[m][n] = ok ? *reinterpret_cast<const float4*>(p.h + (size_t)sl[n] * RH + u0) : make_float4(0.f, 0.f, 0.f, 0.f);
    }
  }
  st.r0 = z4; st.r1 = z4; st.r2 = z4; st.ft = z4;
  st.cl = 0.f;
  st.fle = 0;
  if (wave == 0 && slot_ok(p, sle)) {
    const long long row = r0 + (lane & (RN - 1));   // < B: the slot of a row past B is -1
    const uint4* rp = reinterpret_cast<const uint4*>(p.rec + (size_t)sle * REC);
    st.r0 = rp[0];
    st.r1 = rp[1];
    st.r2 = rp[2];
    st.ft = *reinterpret_cast<const uint4*>(p.feat + (size_t)row * RMF);
    st.cl = p.close[row];
    st.fle = p.flags != nullptr ? (int)p.flags[row] : 0;
  }
}

__global__ void __launch_bounds__(RT, 1) gru_serve_kernel(GruServe p) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
  const s8v* sWx = reinterpret_cast<const s8v*>(lds + Lds::WX);
  bf16_t* sX = reinterpret_cast<bf16_t*>(lds + Lds::X);
  unsigned char* sH8 = lds + Lds::H8;
  int* sSc = reinterpret_cast<int*>(lds + Lds::SC);
  float* sB = reinterpret_cast<float*>(lds + Lds::B);
  float* sWq = reinterpret_cast<float*>(lds + Lds::WQ);
  float* sQp = reinterpret_cast<float*>(lds + Lds::QP);
  int* sDn = reinterpret_cast<int*>(lds + Lds::DN);

  const int tid = threadIdx.x, lane = tid & 63, l16 = lane & 15, g4 = lane >> 4;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
#include "gru_weights.h"
  const bool greedy = __builtin_isinf(p.eps);
  const int nchunks = (p.B + RN - 1) / RN;
  const int row_ = lane & (RN - 1);
  const bool writer = lane < RN;

  // the first chunk's rows, and the slots of the one after it (a chunk past the end has slot -1 everywhere)
  int sl[2], sle, nsl[2], nsle;
  Stage cur, nxt;
  {
    const long long r0 = (long long)blockIdx.x * RN, r1 = r0 + (long long)gridDim.x * RN;
    sl[0] = load_slot(p, r0 + l16);
    sl[1] = load_slot(p, r0 + 16 + l16);
    sle = load_slot(p, r0 + row_);
    nsl[0] = load_slot(p, r1 + l16);
    nsl[1] = load_slot(p, r1 + 16 + l16);
    nsle = load_slot(p, r1 + row_);
    load_stage(p, cur, r0, sl, sle, wave, lane, l16, g4);
  }
  // everything loaded so far has landed (vmcnt(0)): inside the loop only the prefetch is outstanding, so the
  // first use of `cur` there waits for nothing
  __builtin_amdgcn_s_waitcnt(0x0F70);
  __syncthreads();

#pragma unroll 1
  for (int chunk = blockIdx.x; chunk < nchunks; chunk += gridDim.x) {
    const int r0 = chunk * RN;
    // ------------------------------------------------ next chunk's rows, and the slots of the one after
    int fsl[2], fsle;
    {
      const long long r1 = r0 + (long long)gridDim.x * RN, r2 = r1 + (long long)gridDim.x * RN;
      load_stage(p, nxt, r1, nsl, nsle, wave, lane, l16, g4);
      fsl[0] = load_slot(p, r2 + l16);
      fsl[1] = load_slot(p, r2 + 16 + l16);
      fsle = load_slot(p, r2 + row_);
    }
    // ------------------------------------------------ before the bar: fresh episodes, the realised reward, x
    float hr[2][2][4];
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
      for (int n = 0; n < 2; ++n) {
        const bool fresh = (cur.fl[n] & 1) != 0;
        hr[m][n][0] = fresh ? 0.f : cur.h[m][n].x;
        hr[m][n][1] = fresh ? 0.f : cur.h[m][n].y;
        hr[m][n][2] = fresh ? 0.f : cur.h[m][n].z;
        hr[m][n][3] = fresh ? 0.f : cur.h[m][n].w;
      }
    quant_h(hr, sH8, sSc, wave, l16, g4);
    int pz_ = 0, el_ = 0, ntr_ = 0, nlong_ = 0;
    uint32_t bars_ = 0u, draw_ = 0u;
    float en_ = 0.f, sum_ = 0.f, rew_ = 0.f, c_ = 0.f;
    bool done_ = false;
    if (wave == 0) {
      pz_ = (int)cur.r0.x;
      en_ = __uint_as_float(cur.r0.y);
      el_ = (int)cur.r0.z;
      float lc = __uint_as_float(cur.r0.w);
      const int ppos = (int)cur.r1.x;
      const float pfee = __uint_as_float(cur.r1.y);
      sum_ = __uint_as_float(cur.r1.z);
      ntr_ = (int)cur.r1.w;
      nlong_ = (int)cur.r2.x;
      bars_ = cur.r2.y;
      draw_ = cur.r2.z;
      c_ = cur.cl;
      if (cur.fle & 1) {   // a new episode: flat, no entry, the pending reward dropped; the counters stay
        pz_ = 0;
        en_ = 0.f;
        el_ = 0;
        lc = 0.f;
      }
      if (lc > 0.f) {
        const float r = (c_ / lc - 1.f) * 100.f;
        rew_ = (float)ppos * r - pfee;
        sum_ += rew_;
      }
      done_ = el_ + 1 >= p.ep_len;
      if (writer) {
        minute_x_row(sX + lane * XS, cur.ft, minute_x_env(pz_, en_, c_, el_, p.inv_ep_len));
        sDn[lane] = done_ ? 1 : 0;
      }
    }
    lds_barrier();

    // ------------------------------------------------ the bar's net
    const bf16_t* cX = sX;
    const unsigned char* cH = sH8;
    const int* cS = sSc;
#pragma unroll
    for (int n = 0; n < 2; ++n) {
      float (&hrt)[2][2][4] = hr;
#define GRU_TILE_STAMP
#include "gru_net_tile.h"
#undef GRU_TILE_STAMP
    }
    // The prefetch has had the whole net phase to land, and this chunk's stores are not issued yet: wait for
    // it here (vmcnt(0)), so that the stores below are never waited for before they too have had a net phase
    // (the next wait of this kind is one chunk away).
    __builtin_amdgcn_s_waitcnt(0x0F70);
    // scatter h' to the rows' slots; an episode's last bar stores 0 (Q of this bar is already taken)
#pragma unroll
    for (int n = 0; n < 2; ++n)
      if (slot_ok(p, sl[n])) {
        const bool dn = sDn[16 * n + l16] != 0;
#pragma unroll
        for (int m = 0; m < 2; ++m) {
          const int u0 = 32 * wave + 16 * m + 4 * g4;
          *reinterpret_cast<float4*>(p.h + (size_t)sl[n] * RH + u0) =
              dn ? make_float4(0.f, 0.f, 0.f, 0.f) : make_float4(hr[m][n][0], hr[m][n][1], hr[m][n][2], hr[m][n][3]);
        }
      }
    lds_barrier();
    // ------------------------------------------------ env step (wave 0)
    if (wave == 0) {
      float q[3];
      gru_q_row(sWq, sQp, row_, q);
      int a = first_max3(q[0], q[1], q[2]);
      if (!greedy) a = eps_greedy_draw(a, draw_, bars_, p.key0, p.key1, p.eps);
      // the move alone: this bar's reward waits for the next close
      const MinuteMove mv = minute_move(a, pz_, en_, c_, 0.f, p.cost);
      const int row = r0 + lane;
      if (writer && slot_ok(p, sle)) {
        uint4 w0, w1, w2;
        w0.x = (uint32_t)(done_ ? 0 : mv.position);
        w0.y = __float_as_uint(done_ ? 0.f : mv.entry);
        w0.z = (uint32_t)(done_ ? 0 : el_ + 1);
        w0.w = __float_as_uint(c_);
        w1.x = (uint32_t)mv.position;
        w1.y = __float_as_uint(mv.trade ? p.cost : 0.f);
        w1.z = __float_as_uint(sum_);
        w1.w = (uint32_t)(ntr_ + (mv.trade ? 1 : 0));
        w2.x = (uint32_t)(nlong_ + mv.position);
        w2.y = bars_ + 1u;
        w2.z = draw_;
        w2.w = 0u;
        uint4* rp = reinterpret_cast<uint4*>(p.rec + (size_t)sle * REC);
        rp[0] = w0;
        rp[1] = w1;
        rp[2] = w2;
        p.action[row] = (signed char)a;
        p.position[row] = mv.position;
        p.reward[row] = rew_;
        if (p.q != nullptr) {
          p.q[3 * (size_t)row + 0] = q[0];
          p.q[3 * (size_t)row + 1] = q[1];
          p.q[3 * (size_t)row + 2] = q[2];
        }
      } else if (writer && row < p.B) {   // a padding row
        p.action[row] = (signed char)-1;
        p.position[row] = 0;
        p.reward[row] = 0.f;
        if (p.q != nullptr) {
          p.q[3 * (size_t)row + 0] = 0.f;
          p.q[3 * (size_t)row + 1] = 0.f;
          p.q[3 * (size_t)row + 2] = 0.f;
        }
      }
    }
    // the next lds_barrier() (after the next chunk's x row and fp8 tile are written) orders this phase's LDS reads
    // before the next net phase's writes; the tile and x row themselves were last read before the barrier above
    cur = nxt;
    sl[0] = nsl[0]; sl[1] = nsl[1]; sle = nsle;
    nsl[0] = fsl[0]; nsl[1] = fsl[1]; nsle = fsle;
  }
}

}  // namespace gserve
}  // namespace st

extern "C" int st_gru_serve_lds_bytes() { return st::gserve::Lds::BYTES; }

// grid <= 0 (or more than the chunks): one workgroup per 32-row chunk up to one per CU, then the fewest that
// finish the chunks in the same number of rounds (GruPolicy._auto_grid)
extern "C" hipError_t st_gru_serve_launch(const st::gserve::GruServe* p, int grid, hipStream_t stream) {
  using namespace st::gserve;
  if (p == nullptr || p->B < 1 || p->S < 1 || p->ep_len < 1 || !st::net_ok(*p) || p->slot == nullptr ||
      p->feat == nullptr || p->close == nullptr || p->h == nullptr || p->rec == nullptr || p->action == nullptr ||
      p->position == nullptr || p->reward == nullptr)
    return hipErrorInvalidValue;
  // the dynamic-LDS limit is a per-device attribute of the function: set once on every device launched on
  static bool attr[64] = {};
  static int cus[64] = {};
  int dev = 0;
  hipError_t e = hipGetDevice(&dev);
  if (e != hipSuccess) return e;
  const bool slot = dev >= 0 && dev < 64;
  int ncu = slot ? cus[dev] : 0;
  if (!slot || !attr[dev]) {
    e = hipFuncSetAttribute((const void*)gru_serve_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, Lds::BYTES);
    if (e != hipSuccess) return e;
    e = hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, dev);
    if (e != hipSuccess) return e;
    if (ncu < 1) ncu = 1;
    if (slot) {
      cus[dev] = ncu;
      attr[dev] = true;
    }
  }
  const int nchunks = (p->B + st::RN - 1) / st::RN;
  if (grid <= 0 || grid > nchunks) {
    const int rounds = (nchunks + ncu - 1) / ncu;
    grid = (nchunks + rounds - 1) / rounds;
  }
  hipLaunchKernelGGL(gru_serve_kernel, dim3(grid), dim3(st::RT), Lds::BYTES, stream, *p);
  return hipGetLastError();
}

// struct sizes of this file's launch ABI, for the host mirror's check (no HIP call)
extern "C" int st_abi_gru_serve(int* out, int n) {
  const int sz[] = {(int)sizeof(st::gserve::GruServe), (int)sizeof(st::gserve::ServeRec), st::gserve::REC * 4};
  const int m = (int)(sizeof(sz) / sizeof(sz[0]));
  for (int i = 0; i < n && i < m; ++i) out[i] = sz[i];
  return m;
}
