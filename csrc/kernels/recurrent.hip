// recurrent.hip - LSTM / RNN time-step kernels on the bf16 MFMA
// (v_mfma_f32_16x16x32_bf16, f32 accumulation; docs/OPS.md "Recurrent
// layers"):
//   hvk_lstm_step_fwd  acc[B][NG*H] = h_prev . Wh^T with the whole cell in the
//                      epilogue; the pre-activations are never written;
//   hvk_lstm_step_bwd  acc[B][H] = dG_next . Wh (from a transposed copy of
//                      Wh) with the cell's backward in the epilogue.
// One launch is one time step; the stream orders the steps.  No kernel waits
// for another workgroup, nothing is atomic.  The ...2 entry points advance the
// two independent chains of a bidirectional layer in ONE launch: grid.z is the
// direction, a workgroup picks its direction's argument block and runs the
// same body as the one-direction kernel (docs/OPS.md "Bidirectional").
//
// Tile: a workgroup owns 16 hidden units x 32 batch rows and, forward, all
// NG gates of those units (NG = 4 LSTM, gate order i f g o; NG = 1 RNN).
// The weights are the A operand (hidden unit on the accumulator ROW), the
// activations the B operand (batch row on the COLUMN = lane & 15): a lane
// then holds 4 consecutive hidden units of one batch row for every gate, so
// the cell is lane-local and every epilogue access is a 16-B / 8-B vector.
// The weights stay [NG*H][pitch]: gate g of the tile is the row range
// g*H + j0 ...
// A step has few tiles and a short K, so its time is latency: the 4 waves of
// a workgroup split K (wave w takes the 32-wide chunks w, w + 4, ...), each
// feeding the MFMA straight from 16-B global loads held one chunk ahead, and
// their partial sums meet in LDS, added in wave order (fixed: reruns are
// bit-identical).  Waves 0 and 1 then run the cell for 16 batch rows each.
#include "hvk_api.h"
#include "hvk_common.h"

using namespace hvk;

namespace {

constexpr int NTHR = 256;
constexpr int NW = NTHR / WAVE;   // waves = K splits of a workgroup
constexpr int TH = 16;            // hidden units per tile
constexpr int BSUB = 2;           // 16-row batch sub-tiles per tile
constexpr int TB = 16 * BSUB;     // batch rows per tile
constexpr int BK = 32;            // K of one MFMA

enum { CELL_LSTM = 0, CELL_RNN = 1 };

// plain logistic function and tanh; +-inf arguments of the division give
// exactly 0 / 1, tanhf saturates to +-1
__device__ __forceinline__ float sigm(float x) {
  return 1.f / (1.f + __expf(-x));
}
__device__ __forceinline__ float tanh_(float x) { return tanhf(x); }

// The 8 bf16 [row][k .. k + 7] of a K-major operand, 0 outside rows x K.  The
// load is unconditional (an outside fragment reads the operand's first
// element and is replaced by 0 after): a load under a branch makes hipcc wait
// for it where the branches join.  VEC: base and pitch on the 16-B grid and
// K % 8 == 0, so a fragment is inside or outside as a whole.
template <bool VEC>
__device__ __forceinline__ bf16x8 ldfrag(const uint16_t* __restrict__ p,
                                         long long ld, int row, int rows,
                                         int k, int K) {
  uint4 v;
  if constexpr (VEC) {
    const bool in = row < rows && k < K;
    v = *(const uint4*)(in ? p + row * ld + k : p);
    if (!in) v = make_uint4(0, 0, 0, 0);
  } else {
    uint32_t e[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const bool in = row < rows && k + j < K;
      const uint16_t x = *(in ? p + row * ld + k + j : p);
      e[j] = in ? x : 0u;
    }
    v = make_uint4(e[0] | e[1] << 16, e[2] | e[3] << 16, e[4] | e[5] << 16,
                   e[6] | e[7] << 16);
  }
  return __builtin_bit_cast(bf16x8, v);
}

// acc[g][s] (rows: hidden units j0 .., columns: batch rows b0 + 16 s ..) =
// sum over this wave's K chunks of W[g*H + j][k] * A[b][k]
template <int NG, bool VEC>
__device__ __forceinline__ void product(f32x4 (&acc)[NG][BSUB],
                                        const uint16_t* __restrict__ W,
                                        long long ldw, int H, int j0,
                                        const uint16_t* __restrict__ A,
                                        long long lda, int B, int b0, int K,
                                        int lane, int wid) {
  const int fr = lane & 15, fq = lane >> 4;
  const int nkc = (K + BK - 1) / BK;
  bf16x8 wf[NG], af[BSUB];
  auto load = [&](int kc) {
    const int k = kc * BK + fq * 8;   // past K in the chunk after the last
#pragma unroll
    for (int g = 0; g < NG; ++g)
      wf[g] = ldfrag<VEC>(W + (long long)g * H * ldw, ldw, j0 + fr, H, k, K);
#pragma unroll
    for (int s = 0; s < BSUB; ++s)
      af[s] = ldfrag<VEC>(A, lda, b0 + 16 * s + fr, B, k, K);
  };
  load(wid);
  for (int kc = wid; kc < nkc; kc += NW) {
    bf16x8 wc[NG], ac[BSUB];
#pragma unroll
    for (int g = 0; g < NG; ++g) wc[g] = wf[g];
#pragma unroll
    for (int s = 0; s < BSUB; ++s) ac[s] = af[s];
    load(kc + NW);
#pragma unroll
    for (int g = 0; g < NG; ++g)
#pragma unroll
      for (int s = 0; s < BSUB; ++s)
        acc[g][s] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wc[g], ac[s],
                                                            acc[g][s], 0, 0, 0);
  }
}

// The waves' partial sums through LDS; wave s < BSUB returns with the sums of
// batch sub-tile s in out[g], added in wave order.
template <int NG>
__device__ __forceinline__ void reduce(const f32x4 (&acc)[NG][BSUB],
                                       f32x4 (&out)[NG], float4* red,
                                       int lane, int wid) {
#pragma unroll
  for (int g = 0; g < NG; ++g)
#pragma unroll
    for (int s = 0; s < BSUB; ++s) {
      const f32x4 a = acc[g][s];
      red[((wid * NG + g) * BSUB + s) * WAVE + lane] =
          make_float4(a[0], a[1], a[2], a[3]);
    }
  __syncthreads();
  if (wid >= BSUB) return;
#pragma unroll
  for (int g = 0; g < NG; ++g) {
    float4 t = red[(g * BSUB + wid) * WAVE + lane];
#pragma unroll
    for (int w = 1; w < NW; ++w) {
      const float4 u = red[((w * NG + g) * BSUB + wid) * WAVE + lane];
      t.x += u.x; t.y += u.y; t.z += u.z; t.w += u.w;
    }
    out[g] = f32x4{t.x, t.y, t.z, t.w};
  }
}

// 4 consecutive elements at p (nullptr: zeros); VEC: one vector access, else
// the first n of them one by one
template <bool VEC>
__device__ __forceinline__ void ld4f(const float* p, int n, float* v) {
  if constexpr (VEC) {
    const float4 f = *(const float4*)p;
    v[0] = f.x; v[1] = f.y; v[2] = f.z; v[3] = f.w;
  } else {
#pragma unroll
    for (int r = 0; r < 4; ++r) v[r] = r < n ? p[r] : 0.f;
  }
}
template <bool VEC>
__device__ __forceinline__ void ld4h(const uint16_t* p, int n, float* v) {
  if constexpr (VEC) {
    const uint2 u = *(const uint2*)p;
    v[0] = __uint_as_float(u.x << 16);
    v[1] = __uint_as_float(u.x & 0xffff0000u);
    v[2] = __uint_as_float(u.y << 16);
    v[3] = __uint_as_float(u.y & 0xffff0000u);
  } else {
#pragma unroll
    for (int r = 0; r < 4; ++r) v[r] = r < n ? bf2f(p[r]) : 0.f;
  }
}
template <bool VEC>
__device__ __forceinline__ void st4f(float* p, int n, const float* v) {
  if constexpr (VEC) {
    *(float4*)p = make_float4(v[0], v[1], v[2], v[3]);
  } else {
#pragma unroll
    for (int r = 0; r < 4; ++r)
      if (r < n) p[r] = v[r];
  }
}
template <bool VEC>
__device__ __forceinline__ void st4h(uint16_t* p, int n, const float* v) {
  if constexpr (VEC) {
    *(uint2*)p = make_uint2(pack_bf16x2(v[0], v[1]), pack_bf16x2(v[2], v[3]));
  } else {
#pragma unroll
    for (int r = 0; r < 4; ++r)
      if (r < n) p[r] = f2bf(v[r]);
  }
}

// the argument blocks of a paired launch, indexed by blockIdx.z (a scalar
// offset into the kernel arguments: no vector registers)
template <class A>
struct Pair {
  A d[2];
};

struct FwdArgs {
  const uint16_t* h_prev;   // [B][H] bf16, nullptr at step 0
  const uint16_t* Wh;       // [NG*H][H] bf16
  const float* xg;          // [B][NG*H] f32: x_t . Wx^T + bias
  const float* c_prev;      // [B][H] f32, nullptr: zeros (LSTM)
  float* c;                 // [B][H] f32 (LSTM)
  uint16_t* h;              // [B][H] bf16
  uint16_t* gates;          // [B][NG*H] bf16 post-activation, may be nullptr
  long long ld_hp, ld_w, ld_xg, ld_cp, ld_c, ld_h, ld_g;
  int B, H;
};

template <int NG, bool VEC>
__device__ __forceinline__ void step_fwd_body(const FwdArgs& a, float4* red) {
  const int j0 = blockIdx.x * TH, b0 = blockIdx.y * TB;
  const int t = threadIdx.x, lane = t & 63, wid = t >> 6;
  const int B = a.B, H = a.H;
  f32x4 sum[NG];
#pragma unroll
  for (int g = 0; g < NG; ++g) sum[g] = f32x4{0, 0, 0, 0};
  if (a.h_prev) {   // uniform over the workgroup's direction
    f32x4 acc[NG][BSUB];
#pragma unroll
    for (int g = 0; g < NG; ++g)
#pragma unroll
      for (int s = 0; s < BSUB; ++s) acc[g][s] = f32x4{0, 0, 0, 0};
    product<NG, VEC>(acc, a.Wh, a.ld_w, H, j0, a.h_prev, a.ld_hp, B, b0, H,
                     lane, wid);
    reduce<NG>(acc, sum, red, lane, wid);
  }
  if (wid >= BSUB) return;
  const int b = b0 + 16 * wid + (lane & 15);
  const int j = j0 + 4 * (lane >> 4);
  if (b >= B || j >= H) return;
  const int n = min(4, H - j);   // VEC: H % 8 == 0, so n = 4
  float pre[NG][4];
#pragma unroll
  for (int g = 0; g < NG; ++g) {
    ld4f<VEC>(a.xg + b * a.ld_xg + (long long)g * H + j, n, pre[g]);
#pragma unroll
    for (int r = 0; r < 4; ++r) pre[g][r] += sum[g][r];
  }
  float hv[4];
  if constexpr (NG == 4) {
    float cp[4], cv[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) cp[r] = 0.f;
    if (a.c_prev) ld4f<VEC>(a.c_prev + b * a.ld_cp + j, n, cp);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      pre[0][r] = sigm(pre[0][r]);
      pre[1][r] = sigm(pre[1][r]);
      pre[2][r] = tanh_(pre[2][r]);
      pre[3][r] = sigm(pre[3][r]);
      cv[r] = fmaf(pre[1][r], cp[r], pre[0][r] * pre[2][r]);
      hv[r] = pre[3][r] * tanh_(cv[r]);
    }
    st4f<VEC>(a.c + b * a.ld_c + j, n, cv);
    if (a.gates) {
#pragma unroll
      for (int g = 0; g < NG; ++g)
        st4h<VEC>(a.gates + b * a.ld_g + (long long)g * H + j, n, pre[g]);
    }
  } else {
#pragma unroll
    for (int r = 0; r < 4; ++r) hv[r] = tanh_(pre[0][r]);
  }
  st4h<VEC>(a.h + b * a.ld_h + j, n, hv);
}

template <int NG, bool VEC>
__global__ void __launch_bounds__(NTHR) step_fwd_kernel(const FwdArgs a) {
  __shared__ __attribute__((aligned(16))) float4 red[NW * NG * BSUB * WAVE];
  step_fwd_body<NG, VEC>(a, red);
}

// both directions in one launch: blockIdx.z indexes the argument blocks
template <int NG, bool VEC>
__global__ void __launch_bounds__(NTHR)
step_fwd2_kernel(const Pair<FwdArgs> p) {
  __shared__ __attribute__((aligned(16))) float4 red[NW * NG * BSUB * WAVE];
  step_fwd_body<NG, VEC>(p.d[blockIdx.z], red);
}

struct BwdArgs {
  const uint16_t* dg_next;  // [B][NG*H] bf16: dG of step t + 1, or nullptr
  const uint16_t* WhT;      // [H][NG*H] bf16: Wh transposed
  const uint16_t* err;      // [B][H] bf16: error from above, or nullptr
  const uint16_t* gates;    // LSTM: [B][4H] saved gates; RNN: h_t [B][H]
  const float* c_prev;      // [B][H] f32, nullptr at t = 0 (LSTM)
  const float* c;           // [B][H] f32 (LSTM)
  const float* dc_in;       // [B][H] f32 carried dc_t, nullptr: zeros
  float* dc_out;            // [B][H] f32 dc_{t-1} (may alias dc_in)
  uint16_t* dg;             // [B][NG*H] bf16
  long long ld_dgn, ld_wt, ld_e, ld_g, ld_cp, ld_c, ld_dci, ld_dco, ld_dg;
  int B, H;
};

template <int NG, bool VEC>
__device__ __forceinline__ void step_bwd_body(const BwdArgs& a, float4* red) {
  const int j0 = blockIdx.x * TH, b0 = blockIdx.y * TB;
  const int t = threadIdx.x, lane = t & 63, wid = t >> 6;
  const int B = a.B, H = a.H;
  f32x4 sum[1] = {f32x4{0, 0, 0, 0}};
  if (a.dg_next) {   // uniform over the workgroup's direction
    f32x4 acc[1][BSUB];
#pragma unroll
    for (int s = 0; s < BSUB; ++s) acc[0][s] = f32x4{0, 0, 0, 0};
    product<1, VEC>(acc, a.WhT, a.ld_wt, H, j0, a.dg_next, a.ld_dgn, B, b0,
                    NG * H, lane, wid);
    reduce<1>(acc, sum, red, lane, wid);
  }
  if (wid >= BSUB) return;
  const int b = b0 + 16 * wid + (lane & 15);
  const int j = j0 + 4 * (lane >> 4);
  if (b >= B || j >= H) return;
  const int n = min(4, H - j);
  float dh[4], gt[NG][4], d[NG][4];
#pragma unroll
  for (int r = 0; r < 4; ++r) dh[r] = 0.f;
  if (a.err) ld4h<VEC>(a.err + b * a.ld_e + j, n, dh);
#pragma unroll
  for (int r = 0; r < 4; ++r) dh[r] += sum[0][r];
#pragma unroll
  for (int g = 0; g < NG; ++g)
    ld4h<VEC>(a.gates + b * a.ld_g + (long long)g * H + j, n, gt[g]);
  if constexpr (NG == 4) {
    float cp[4], cv[4], dc[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) cp[r] = dc[r] = 0.f;
    if (a.c_prev) ld4f<VEC>(a.c_prev + b * a.ld_cp + j, n, cp);
    if (a.dc_in) ld4f<VEC>(a.dc_in + b * a.ld_dci + j, n, dc);
    ld4f<VEC>(a.c + b * a.ld_c + j, n, cv);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const float gi = gt[0][r], gf = gt[1][r], gg = gt[2][r], go = gt[3][r];
      const float tc = tanh_(cv[r]);
      const float dcr = fmaf(dh[r] * go, 1.f - tc * tc, dc[r]);
      d[0][r] = dcr * gg * gi * (1.f - gi);
      d[1][r] = dcr * cp[r] * gf * (1.f - gf);
      d[2][r] = dcr * gi * (1.f - gg * gg);
      d[3][r] = dh[r] * tc * go * (1.f - go);
      dc[r] = dcr * gf;
    }
    st4f<VEC>(a.dc_out + b * a.ld_dco + j, n, dc);
  } else {
#pragma unroll
    for (int r = 0; r < 4; ++r)
      d[0][r] = dh[r] * (1.f - gt[0][r] * gt[0][r]);
  }
#pragma unroll
  for (int g = 0; g < NG; ++g)
    st4h<VEC>(a.dg + b * a.ld_dg + (long long)g * H + j, n, d[g]);
}

template <int NG, bool VEC>
__global__ void __launch_bounds__(NTHR) step_bwd_kernel(const BwdArgs a) {
  __shared__ __attribute__((aligned(16))) float4 red[NW * BSUB * WAVE];
  step_bwd_body<NG, VEC>(a, red);
}

// both directions in one launch: blockIdx.z indexes the argument blocks
template <int NG, bool VEC>
__global__ void __launch_bounds__(NTHR)
step_bwd2_kernel(const Pair<BwdArgs> p) {
  __shared__ __attribute__((aligned(16))) float4 red[NW * BSUB * WAVE];
  step_bwd_body<NG, VEC>(p.d[blockIdx.z], red);
}

// y[i] = the cell's own logistic function (kind 0) / tanh (kind 1) of x[i]:
// lets a test measure the device functions the epilogues use
__global__ void __launch_bounds__(NTHR)
recurrent_fn_kernel(const float* __restrict__ x, float* __restrict__ y,
                    long long n, int kind) {
  const long long i = (long long)blockIdx.x * NTHR + threadIdx.x;
  if (i < n) y[i] = kind == 0 ? sigm(x[i]) : tanh_(x[i]);
}

inline bool on_grid(const void* p, long long ld) {
  return ((uintptr_t)p & 15) == 0 && ld % 8 == 0;
}

// directions of a launch: one argument block, or a Pair of them
template <class A>
constexpr unsigned ndirs(const A&) { return 1; }
template <class A>
constexpr unsigned ndirs(const Pair<A>&) { return 2; }

// Launches step kernel k on its argument block(s) over the tile grid of one
// step: ceil(H / TH) x ceil(B / TB) x directions.  Refuses a batch with more
// tiles than grid.y holds.
template <class A>
int launch_step(void (*k)(const A), const A& a, int B, int H, hipStream_t s) {
  const dim3 grid((unsigned)((H + TH - 1) / TH), (unsigned)((B + TB - 1) / TB),
                  ndirs(a));
  if (grid.y > 65535u) return -1;
  hipLaunchKernelGGL(k, grid, dim3(NTHR), 0, s, a);
  return (int)launch_status(s);
}

// the step kernel that takes one argument block / a Pair of them
template <int NG, bool VEC>
constexpr auto fwd_kernel(const FwdArgs&) { return step_fwd_kernel<NG, VEC>; }
template <int NG, bool VEC>
constexpr auto fwd_kernel(const Pair<FwdArgs>&) {
  return step_fwd2_kernel<NG, VEC>;
}
template <int NG, bool VEC>
constexpr auto bwd_kernel(const BwdArgs&) { return step_bwd_kernel<NG, VEC>; }
template <int NG, bool VEC>
constexpr auto bwd_kernel(const Pair<BwdArgs>&) {
  return step_bwd2_kernel<NG, VEC>;
}

// (cell, vec) -> instantiation, for one direction and for a Pair alike
template <class A>
int launch_fwd(const A& a, bool lstm, bool vec, int B, int H, hipStream_t s) {
  if (lstm)
    return vec ? launch_step(fwd_kernel<4, true>(a), a, B, H, s)
               : launch_step(fwd_kernel<4, false>(a), a, B, H, s);
  return vec ? launch_step(fwd_kernel<1, true>(a), a, B, H, s)
             : launch_step(fwd_kernel<1, false>(a), a, B, H, s);
}

template <class A>
int launch_bwd(const A& a, bool lstm, bool vec, int B, int H, hipStream_t s) {
  if (lstm)
    return vec ? launch_step(bwd_kernel<4, true>(a), a, B, H, s)
               : launch_step(bwd_kernel<4, false>(a), a, B, H, s);
  return vec ? launch_step(bwd_kernel<1, true>(a), a, B, H, s)
             : launch_step(bwd_kernel<1, false>(a), a, B, H, s);
}

}  // namespace

// One forward time step.  cell 0 (LSTM, NG = 4, gate order i f g o):
//   pre = xg + h_prev . Wh^T;  i, f, o = sigmoid, g = tanh;
//   c = f c_prev + i g;  h = o tanh(c)
// cell 1 (RNN, NG = 1): h = tanh(xg + h_prev . Wh^T); c / c_prev / gates
// unused.  h_prev nullptr: step 0, no product.  c_prev nullptr: zeros.  gates
// nullptr: not stored.  Every operand has its own row pitch in elements, so a
// step of a batch-major [B][T][.] tensor is a strided view.
namespace {

// Checks one direction's operands and fills its argument block; false:
// refuse.  vec: every operand on the 16-B grid.
bool fwd_args(FwdArgs& a, bool& vec, int cell, int B, int H,
              const void* h_prev, long long ld_hp, const void* Wh,
              long long ld_w, const float* xg, long long ld_xg,
              const float* c_prev, long long ld_cp, float* c, long long ld_c,
              void* h, long long ld_h, void* gates, long long ld_g) {
  const bool lstm = cell == CELL_LSTM;
  if ((cell != CELL_LSTM && cell != CELL_RNN) || B < 1 || H < 1 || !xg ||
      !h || (h_prev && !Wh) || (lstm && !c))
    return false;
  const int ng = lstm ? 4 : 1;
  if (ld_xg < (long long)ng * H || ld_h < H || (h_prev && ld_hp < H) ||
      (h_prev && ld_w < H) || (lstm && ld_c < H) ||
      (lstm && c_prev && ld_cp < H) || (lstm && gates && ld_g < 4ll * H))
    return false;
  a.h_prev = (const uint16_t*)h_prev;
  a.Wh = (const uint16_t*)Wh;
  a.xg = xg;
  a.c_prev = lstm ? c_prev : nullptr;
  a.c = c;
  a.h = (uint16_t*)h;
  a.gates = lstm ? (uint16_t*)gates : nullptr;
  a.ld_hp = ld_hp; a.ld_w = ld_w; a.ld_xg = ld_xg; a.ld_cp = ld_cp;
  a.ld_c = ld_c; a.ld_h = ld_h; a.ld_g = ld_g;
  a.B = B; a.H = H;
  vec = H % 8 == 0 && on_grid(xg, ld_xg) && on_grid(h, ld_h) &&
        (!h_prev || (on_grid(h_prev, ld_hp) && on_grid(Wh, ld_w))) &&
        (!lstm || on_grid(c, ld_c)) &&
        (!a.c_prev || on_grid(c_prev, ld_cp)) &&
        (!a.gates || on_grid(gates, ld_g));
  return true;
}

}  // namespace

HVK_API int hvk_lstm_step_fwd(int cell, int B, int H, const void* h_prev,
                              long long ld_hp, const void* Wh, long long ld_w,
                              const float* xg, long long ld_xg,
                              const float* c_prev, long long ld_cp, float* c,
                              long long ld_c, void* h, long long ld_h,
                              void* gates, long long ld_g, hipStream_t s) {
  FwdArgs a;
  bool vec;
  if (!fwd_args(a, vec, cell, B, H, h_prev, ld_hp, Wh, ld_w, xg, ld_xg,
                c_prev, ld_cp, c, ld_c, h, ld_h, gates, ld_g))
    return -1;
  return launch_fwd(a, cell == CELL_LSTM, vec, B, H, s);
}

// One forward time step of BOTH directions of a bidirectional layer in one
// launch (grid.z = 2): the operand list of hvk_lstm_step_fwd once per
// direction (0: forward chain, 1: reverse chain; each at its own time step).
// Per direction the launch does exactly what hvk_lstm_step_fwd does, bit for
// bit; null operands are per direction.  The vector path needs every operand
// of both directions on the 16-B grid.
HVK_API int hvk_lstm_step_fwd2(
    int cell, int B, int H, const void* h_prev0, long long ld_hp0,
    const void* Wh0, long long ld_w0, const float* xg0, long long ld_xg0,
    const float* c_prev0, long long ld_cp0, float* c0, long long ld_c0,
    void* h0, long long ld_h0, void* gates0, long long ld_g0,
    const void* h_prev1, long long ld_hp1, const void* Wh1, long long ld_w1,
    const float* xg1, long long ld_xg1, const float* c_prev1,
    long long ld_cp1, float* c1, long long ld_c1, void* h1, long long ld_h1,
    void* gates1, long long ld_g1, hipStream_t s) {
  Pair<FwdArgs> p;
  FwdArgs &a0 = p.d[0], &a1 = p.d[1];
  bool vec0, vec1;
  if (!fwd_args(a0, vec0, cell, B, H, h_prev0, ld_hp0, Wh0, ld_w0, xg0,
                ld_xg0, c_prev0, ld_cp0, c0, ld_c0, h0, ld_h0, gates0,
                ld_g0) ||
      !fwd_args(a1, vec1, cell, B, H, h_prev1, ld_hp1, Wh1, ld_w1, xg1,
                ld_xg1, c_prev1, ld_cp1, c1, ld_c1, h1, ld_h1, gates1, ld_g1))
    return -1;
  return launch_fwd(p, cell == CELL_LSTM, vec0 && vec1, B, H, s);
}

// One backward time step: dh = err + dg_next . Wh (either may be absent),
// then, LSTM, from the saved gates, c_prev, c and the carried dc_in:
//   dc = dc_in + dh o (1 - tanh(c)^2)
//   dG = (dc g i(1-i), dc c_prev f(1-f), dc i (1-g^2), dh tanh(c) o(1-o))
//   dc_out = dc f
// RNN (gates = h_t): dG = dh (1 - h^2).  WhT is [H][NG*H], Wh transposed.
namespace {

bool bwd_args(BwdArgs& a, bool& vec, int cell, int B, int H,
              const void* dg_next, long long ld_dgn, const void* WhT,
              long long ld_wt, const void* err, long long ld_e,
              const void* gates, long long ld_g, const float* c_prev,
              long long ld_cp, const float* c, long long ld_c,
              const float* dc_in, long long ld_dci, float* dc_out,
              long long ld_dco, void* dg, long long ld_dg) {
  const bool lstm = cell == CELL_LSTM;
  if ((cell != CELL_LSTM && cell != CELL_RNN) || B < 1 || H < 1 || !gates ||
      !dg || (dg_next && !WhT) || (lstm && (!c || !dc_out)))
    return false;
  const long long gh = (lstm ? 4ll : 1ll) * H;
  if (ld_dg < gh || ld_g < gh || (dg_next && (ld_dgn < gh || ld_wt < gh)) ||
      (err && ld_e < H) ||
      (lstm && (ld_c < H || ld_dco < H || (c_prev && ld_cp < H) ||
                (dc_in && ld_dci < H))))
    return false;
  a.dg_next = (const uint16_t*)dg_next;
  a.WhT = (const uint16_t*)WhT;
  a.err = (const uint16_t*)err;
  a.gates = (const uint16_t*)gates;
  a.c_prev = lstm ? c_prev : nullptr;
  a.c = c;
  a.dc_in = lstm ? dc_in : nullptr;
  a.dc_out = dc_out;
  a.dg = (uint16_t*)dg;
  a.ld_dgn = ld_dgn; a.ld_wt = ld_wt; a.ld_e = ld_e; a.ld_g = ld_g;
  a.ld_cp = ld_cp; a.ld_c = ld_c; a.ld_dci = ld_dci; a.ld_dco = ld_dco;
  a.ld_dg = ld_dg;
  a.B = B; a.H = H;
  vec = H % 8 == 0 && on_grid(dg, ld_dg) && on_grid(gates, ld_g) &&
        (!dg_next || (on_grid(dg_next, ld_dgn) && on_grid(WhT, ld_wt))) &&
        (!err || on_grid(err, ld_e)) &&
        (!lstm || (on_grid(c, ld_c) && on_grid(dc_out, ld_dco))) &&
        (!a.c_prev || on_grid(c_prev, ld_cp)) &&
        (!a.dc_in || on_grid(dc_in, ld_dci));
  return true;
}

}  // namespace

HVK_API int hvk_lstm_step_bwd(int cell, int B, int H, const void* dg_next,
                              long long ld_dgn, const void* WhT,
                              long long ld_wt, const void* err,
                              long long ld_e, const void* gates,
                              long long ld_g, const float* c_prev,
                              long long ld_cp, const float* c, long long ld_c,
                              const float* dc_in, long long ld_dci,
                              float* dc_out, long long ld_dco, void* dg,
                              long long ld_dg, hipStream_t s) {
  BwdArgs a;
  bool vec;
  if (!bwd_args(a, vec, cell, B, H, dg_next, ld_dgn, WhT, ld_wt, err, ld_e,
                gates, ld_g, c_prev, ld_cp, c, ld_c, dc_in, ld_dci, dc_out,
                ld_dco, dg, ld_dg))
    return -1;
  return launch_bwd(a, cell == CELL_LSTM, vec, B, H, s);
}

// One backward time step of both directions in one launch (grid.z = 2): the
// operand list of hvk_lstm_step_bwd once per direction, null operands per
// direction, bit for bit what hvk_lstm_step_bwd does on either.
HVK_API int hvk_lstm_step_bwd2(
    int cell, int B, int H, const void* dg_next0, long long ld_dgn0,
    const void* WhT0, long long ld_wt0, const void* err0, long long ld_e0,
    const void* gates0, long long ld_g0, const float* c_prev0,
    long long ld_cp0, const float* c0, long long ld_c0, const float* dc_in0,
    long long ld_dci0, float* dc_out0, long long ld_dco0, void* dg0,
    long long ld_dg0, const void* dg_next1, long long ld_dgn1,
    const void* WhT1, long long ld_wt1, const void* err1, long long ld_e1,
    const void* gates1, long long ld_g1, const float* c_prev1,
    long long ld_cp1, const float* c1, long long ld_c1, const float* dc_in1,
    long long ld_dci1, float* dc_out1, long long ld_dco1, void* dg1,
    long long ld_dg1, hipStream_t s) {
  Pair<BwdArgs> p;
  BwdArgs &a0 = p.d[0], &a1 = p.d[1];
  bool vec0, vec1;
  if (!bwd_args(a0, vec0, cell, B, H, dg_next0, ld_dgn0, WhT0, ld_wt0, err0,
                ld_e0, gates0, ld_g0, c_prev0, ld_cp0, c0, ld_c0, dc_in0,
                ld_dci0, dc_out0, ld_dco0, dg0, ld_dg0) ||
      !bwd_args(a1, vec1, cell, B, H, dg_next1, ld_dgn1, WhT1, ld_wt1, err1,
                ld_e1, gates1, ld_g1, c_prev1, ld_cp1, c1, ld_c1, dc_in1,
                ld_dci1, dc_out1, ld_dco1, dg1, ld_dg1))
    return -1;
  return launch_bwd(p, cell == CELL_LSTM, vec0 && vec1, B, H, s);
}

HVK_API int hvk_recurrent_fn(int kind, const float* x, float* y, long long n,
                             hipStream_t s) {
  if (!x || !y || n < 1 || (kind != 0 && kind != 1)) return -1;
  hipLaunchKernelGGL(recurrent_fn_kernel,
                     dim3((unsigned)((n + NTHR - 1) / NTHR)), dim3(NTHR), 0, s,
                     x, y, n, kind);
  return (int)launch_status(s);
}

// ---------------------------------------------------------------- GRU
// (docs/OPS.md "GRU").  Gate order r, z, n along the 3H axis:
//   r = sigmoid(xg_r + h_prev . Whr^T),  z = sigmoid(xg_z + h_prev . Whz^T)
//   hn = h_prev . Whn^T + b_hn,  n = tanh(xg_n + r hn)
//   h = (1 - z) n + z h_prev
// The reset gate multiplies the hidden-side product alone, so the step has
// two gate gradients (input side dGx, hidden side dGh) and h is carried in
// float32 (hf) next to the bf16 copy the MFMA reads.  Same tile, K split and
// ordered reduction as above.
namespace {

struct GruFwdArgs {
  const uint16_t* h_prev;   // [B][H] bf16, nullptr at step 0
  const uint16_t* Wh;       // [3H][H] bf16
  const float* xg;          // [B][3H] f32: x_t . Wx^T + (b_r, b_z, b_n)
  const float* bhn;         // [H] f32 or nullptr: zeros
  const float* hf_prev;     // [B][H] f32, nullptr: zeros
  float* hf;                // [B][H] f32: h_t unrounded
  float* hn;                // [B][H] f32
  uint16_t* h;              // [B][H] bf16
  uint16_t* gates;          // [B][3H] bf16 post-activation r z n, or nullptr
  long long ld_hp, ld_w, ld_xg, ld_hfp, ld_hf, ld_hn, ld_h, ld_g;
  int B, H;
};

template <bool VEC>
__device__ __forceinline__ void gru_fwd_body(const GruFwdArgs& a, float4* red) {
  const int j0 = blockIdx.x * TH, b0 = blockIdx.y * TB;
  const int t = threadIdx.x, lane = t & 63, wid = t >> 6;
  const int B = a.B, H = a.H;
  f32x4 sum[3];
#pragma unroll
  for (int g = 0; g < 3; ++g) sum[g] = f32x4{0, 0, 0, 0};
  if (a.h_prev) {   // uniform over the workgroup's direction
    f32x4 acc[3][BSUB];
#pragma unroll
    for (int g = 0; g < 3; ++g)
#pragma unroll
      for (int s = 0; s < BSUB; ++s) acc[g][s] = f32x4{0, 0, 0, 0};
    product<3, VEC>(acc, a.Wh, a.ld_w, H, j0, a.h_prev, a.ld_hp, B, b0, H,
                    lane, wid);
    reduce<3>(acc, sum, red, lane, wid);
  }
  const int b = b0 + 16 * wid + (lane & 15);
  const int j = j0 + 4 * (lane >> 4);
  if (wid >= BSUB || b >= B || j >= H) return;
  const int n = min(4, H - j);   // VEC: H % 8 == 0, so n = 4
  float pre[3][4], bh[4], hp[4], hnv[4], hv[4];
#pragma unroll
  for (int g = 0; g < 3; ++g)
    ld4f<VEC>(a.xg + b * a.ld_xg + (long long)g * H + j, n, pre[g]);
#pragma unroll
  for (int r = 0; r < 4; ++r) bh[r] = hp[r] = 0.f;
  if (a.bhn) ld4f<VEC>(a.bhn + j, n, bh);
  if (a.hf_prev) ld4f<VEC>(a.hf_prev + b * a.ld_hfp + j, n, hp);
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const float gr = sigm(pre[0][r] + sum[0][r]);
    const float gz = sigm(pre[1][r] + sum[1][r]);
    hnv[r] = sum[2][r] + bh[r];
    const float gn = tanh_(fmaf(gr, hnv[r], pre[2][r]));
    // z = 1 gives h_prev exactly, z = 0 gives n exactly
    hv[r] = fmaf(gz, hp[r], (1.f - gz) * gn);
    pre[0][r] = gr; pre[1][r] = gz; pre[2][r] = gn;
  }
  st4f<VEC>(a.hf + b * a.ld_hf + j, n, hv);
  st4f<VEC>(a.hn + b * a.ld_hn + j, n, hnv);
  st4h<VEC>(a.h + b * a.ld_h + j, n, hv);
  if (a.gates) {
#pragma unroll
    for (int g = 0; g < 3; ++g)
      st4h<VEC>(a.gates + b * a.ld_g + (long long)g * H + j, n, pre[g]);
  }
}

template <bool VEC>
__global__ void __launch_bounds__(NTHR) gru_fwd_kernel(const GruFwdArgs a) {
  __shared__ __attribute__((aligned(16))) float4 red[NW * 3 * BSUB * WAVE];
  gru_fwd_body<VEC>(a, red);
}

// both directions in one launch: blockIdx.z indexes the argument blocks
template <bool VEC>
__global__ void __launch_bounds__(NTHR)
gru_fwd2_kernel(const Pair<GruFwdArgs> p) {
  __shared__ __attribute__((aligned(16))) float4 red[NW * 3 * BSUB * WAVE];
  gru_fwd_body<VEC>(p.d[blockIdx.z], red);
}

struct GruBwdArgs {
  const uint16_t* dgh_next; // [B][3H] bf16: dGh of step t + 1, or nullptr
  const uint16_t* WhT;      // [H][3H] bf16: Wh transposed
  const uint16_t* err;      // [B][H] bf16: error from above, or nullptr
  const uint16_t* gates;    // [B][3H] bf16 saved r z n
  const float* hn;          // [B][H] f32
  const float* hf_prev;     // [B][H] f32 h_{t-1}, nullptr at t = 0
  const float* dc_in;       // [B][H] f32 dh_{t+1} z_{t+1}, nullptr: zeros
  float* dc_out;            // [B][H] f32 dh_t z_t
  uint16_t* dgx;            // [B][3H] bf16 (dr, dz, dn)
  uint16_t* dgh;            // [B][3H] bf16 (dr, dz, dn r)
  long long ld_dgn, ld_wt, ld_e, ld_g, ld_hn, ld_hfp, ld_dci, ld_dco, ld_dgx,
      ld_dgh;
  int B, H;
};

template <bool VEC>
__device__ __forceinline__ void gru_bwd_body(const GruBwdArgs& a, float4* red) {
  const int j0 = blockIdx.x * TH, b0 = blockIdx.y * TB;
  const int t = threadIdx.x, lane = t & 63, wid = t >> 6;
  const int B = a.B, H = a.H;
  f32x4 sum[1] = {f32x4{0, 0, 0, 0}};
  if (a.dgh_next) {   // uniform over the workgroup's direction
    f32x4 acc[1][BSUB];
#pragma unroll
    for (int s = 0; s < BSUB; ++s) acc[0][s] = f32x4{0, 0, 0, 0};
    product<1, VEC>(acc, a.WhT, a.ld_wt, H, j0, a.dgh_next, a.ld_dgn, B, b0,
                    3 * H, lane, wid);
    reduce<1>(acc, sum, red, lane, wid);
  }
  if (wid >= BSUB) return;
  const int b = b0 + 16 * wid + (lane & 15);
  const int j = j0 + 4 * (lane >> 4);
  if (b >= B || j >= H) return;
  const int n = min(4, H - j);
  float dh[4], gt[3][4], hnv[4], hp[4], dc[4], dx[3][4], dnr[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) dh[r] = hp[r] = dc[r] = 0.f;
  if (a.err) ld4h<VEC>(a.err + b * a.ld_e + j, n, dh);
  if (a.hf_prev) ld4f<VEC>(a.hf_prev + b * a.ld_hfp + j, n, hp);
  if (a.dc_in) ld4f<VEC>(a.dc_in + b * a.ld_dci + j, n, dc);
  ld4f<VEC>(a.hn + b * a.ld_hn + j, n, hnv);
#pragma unroll
  for (int g = 0; g < 3; ++g)
    ld4h<VEC>(a.gates + b * a.ld_g + (long long)g * H + j, n, gt[g]);
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const float gr = gt[0][r], gz = gt[1][r], gn = gt[2][r];
    const float d = dh[r] + sum[0][r] + dc[r];
    const float dn = d * (1.f - gz) * (1.f - gn * gn);
    dx[0][r] = dn * hnv[r] * gr * (1.f - gr);
    dx[1][r] = d * (hp[r] - gn) * gz * (1.f - gz);
    dx[2][r] = dn;
    dnr[r] = dn * gr;
    dc[r] = d * gz;
  }
  st4f<VEC>(a.dc_out + b * a.ld_dco + j, n, dc);
#pragma unroll
  for (int g = 0; g < 3; ++g)
    st4h<VEC>(a.dgx + b * a.ld_dgx + (long long)g * H + j, n, dx[g]);
  st4h<VEC>(a.dgh + b * a.ld_dgh + j, n, dx[0]);
  st4h<VEC>(a.dgh + b * a.ld_dgh + (long long)H + j, n, dx[1]);
  st4h<VEC>(a.dgh + b * a.ld_dgh + 2ll * H + j, n, dnr);
}

template <bool VEC>
__global__ void __launch_bounds__(NTHR) gru_bwd_kernel(const GruBwdArgs a) {
  __shared__ __attribute__((aligned(16))) float4 red[NW * BSUB * WAVE];
  gru_bwd_body<VEC>(a, red);
}

// both directions in one launch: blockIdx.z indexes the argument blocks
template <bool VEC>
__global__ void __launch_bounds__(NTHR)
gru_bwd2_kernel(const Pair<GruBwdArgs> p) {
  __shared__ __attribute__((aligned(16))) float4 red[NW * BSUB * WAVE];
  gru_bwd_body<VEC>(p.d[blockIdx.z], red);
}

// as fwd_kernel / launch_fwd above
template <bool VEC>
constexpr auto gru_fwd_k(const GruFwdArgs&) { return gru_fwd_kernel<VEC>; }
template <bool VEC>
constexpr auto gru_fwd_k(const Pair<GruFwdArgs>&) {
  return gru_fwd2_kernel<VEC>;
}
template <bool VEC>
constexpr auto gru_bwd_k(const GruBwdArgs&) { return gru_bwd_kernel<VEC>; }
template <bool VEC>
constexpr auto gru_bwd_k(const Pair<GruBwdArgs>&) {
  return gru_bwd2_kernel<VEC>;
}

template <class A>
int launch_gru_fwd(const A& a, bool vec, int B, int H, hipStream_t s) {
  return vec ? launch_step(gru_fwd_k<true>(a), a, B, H, s)
             : launch_step(gru_fwd_k<false>(a), a, B, H, s);
}

template <class A>
int launch_gru_bwd(const A& a, bool vec, int B, int H, hipStream_t s) {
  return vec ? launch_step(gru_bwd_k<true>(a), a, B, H, s)
             : launch_step(gru_bwd_k<false>(a), a, B, H, s);
}

}  // namespace

// One forward GRU time step (equations above).  h_prev nullptr: step 0, no
// product, hn = b_hn.  hf_prev nullptr: zeros.  bhn nullptr: zeros.  gates
// nullptr: not stored.  Every [B][.] operand has its own row pitch in
// elements.
namespace {

bool gru_fwd_args(GruFwdArgs& a, bool& vec, int B, int H, const void* h_prev,
                  long long ld_hp, const void* Wh, long long ld_w,
                  const float* xg, long long ld_xg, const float* hf_prev,
                  long long ld_hfp, float* hf, long long ld_hf, float* hn,
                  long long ld_hn, void* h, long long ld_h, void* gates,
                  long long ld_g, const float* bhn) {
  if (B < 1 || H < 1 || !xg || !h || !hf || !hn || (h_prev && !Wh))
    return false;
  if (ld_xg < 3ll * H || ld_h < H || ld_hf < H || ld_hn < H ||
      (h_prev && (ld_hp < H || ld_w < H)) || (hf_prev && ld_hfp < H) ||
      (gates && ld_g < 3ll * H))
    return false;
  a.h_prev = (const uint16_t*)h_prev;
  a.Wh = (const uint16_t*)Wh;
  a.xg = xg;
  a.bhn = bhn;
  a.hf_prev = hf_prev;
  a.hf = hf;
  a.hn = hn;
  a.h = (uint16_t*)h;
  a.gates = (uint16_t*)gates;
  a.ld_hp = ld_hp; a.ld_w = ld_w; a.ld_xg = ld_xg; a.ld_hfp = ld_hfp;
  a.ld_hf = ld_hf; a.ld_hn = ld_hn; a.ld_h = ld_h; a.ld_g = ld_g;
  a.B = B; a.H = H;
  vec = H % 8 == 0 && on_grid(xg, ld_xg) && on_grid(h, ld_h) &&
        on_grid(hf, ld_hf) && on_grid(hn, ld_hn) &&
        (!h_prev || (on_grid(h_prev, ld_hp) && on_grid(Wh, ld_w))) &&
        (!hf_prev || on_grid(hf_prev, ld_hfp)) &&
        (!bhn || on_grid(bhn, 8)) && (!gates || on_grid(gates, ld_g));
  return true;
}

}  // namespace

HVK_API int hvk_gru_step_fwd(int B, int H, const void* h_prev,
                             long long ld_hp, const void* Wh, long long ld_w,
                             const float* xg, long long ld_xg,
                             const float* hf_prev, long long ld_hfp,
                             float* hf, long long ld_hf, float* hn,
                             long long ld_hn, void* h, long long ld_h,
                             void* gates, long long ld_g, const float* bhn,
                             hipStream_t s) {
  GruFwdArgs a;
  bool vec;
  if (!gru_fwd_args(a, vec, B, H, h_prev, ld_hp, Wh, ld_w, xg, ld_xg, hf_prev,
                    ld_hfp, hf, ld_hf, hn, ld_hn, h, ld_h, gates, ld_g, bhn))
    return -1;
  return launch_gru_fwd(a, vec, B, H, s);
}

// One forward GRU time step of both directions in one launch (grid.z = 2):
// the operand list of hvk_gru_step_fwd once per direction, null operands per
// direction, bit for bit what hvk_gru_step_fwd does on either.
HVK_API int hvk_gru_step_fwd2(
    int B, int H, const void* h_prev0, long long ld_hp0, const void* Wh0,
    long long ld_w0, const float* xg0, long long ld_xg0,
    const float* hf_prev0, long long ld_hfp0, float* hf0, long long ld_hf0,
    float* hn0, long long ld_hn0, void* h0, long long ld_h0, void* gates0,
    long long ld_g0, const float* bhn0, const void* h_prev1,
    long long ld_hp1, const void* Wh1, long long ld_w1, const float* xg1,
    long long ld_xg1, const float* hf_prev1, long long ld_hfp1, float* hf1,
    long long ld_hf1, float* hn1, long long ld_hn1, void* h1, long long ld_h1,
    void* gates1, long long ld_g1, const float* bhn1, hipStream_t s) {
  Pair<GruFwdArgs> p;
  GruFwdArgs &a0 = p.d[0], &a1 = p.d[1];
  bool vec0, vec1;
  if (!gru_fwd_args(a0, vec0, B, H, h_prev0, ld_hp0, Wh0, ld_w0, xg0, ld_xg0,
                    hf_prev0, ld_hfp0, hf0, ld_hf0, hn0, ld_hn0, h0, ld_h0,
                    gates0, ld_g0, bhn0) ||
      !gru_fwd_args(a1, vec1, B, H, h_prev1, ld_hp1, Wh1, ld_w1, xg1, ld_xg1,
                    hf_prev1, ld_hfp1, hf1, ld_hf1, hn1, ld_hn1, h1, ld_h1,
                    gates1, ld_g1, bhn1))
    return -1;
  return launch_gru_fwd(p, vec0 && vec1, B, H, s);
}

// One backward GRU time step from the saved gates (r, z, n), hn and the
// float32 h_{t-1}:
//   dh = err + dgh_next . Wh + dc_in            (each may be absent)
//   dn = dh (1 - z)(1 - n^2),  dz = dh (h_prev - n) z(1 - z)
//   dr = dn hn r(1 - r)
//   dgx = (dr, dz, dn),  dgh = (dr, dz, dn r),  dc_out = dh z
// WhT is [H][3H], Wh transposed.  dc_out may alias dc_in.
namespace {

bool gru_bwd_args(GruBwdArgs& a, bool& vec, int B, int H,
                  const void* dgh_next, long long ld_dgn, const void* WhT,
                  long long ld_wt, const void* err, long long ld_e,
                  const void* gates, long long ld_g, const float* hn,
                  long long ld_hn, const float* hf_prev, long long ld_hfp,
                  const float* dc_in, long long ld_dci, float* dc_out,
                  long long ld_dco, void* dgx, long long ld_dgx, void* dgh,
                  long long ld_dgh) {
  if (B < 1 || H < 1 || !gates || !hn || !dc_out || !dgx || !dgh ||
      (dgh_next && !WhT))
    return false;
  const long long gh = 3ll * H;
  if (ld_dgx < gh || ld_dgh < gh || ld_g < gh || ld_hn < H || ld_dco < H ||
      (dgh_next && (ld_dgn < gh || ld_wt < gh)) || (err && ld_e < H) ||
      (hf_prev && ld_hfp < H) || (dc_in && ld_dci < H))
    return false;
  a.dgh_next = (const uint16_t*)dgh_next;
  a.WhT = (const uint16_t*)WhT;
  a.err = (const uint16_t*)err;
  a.gates = (const uint16_t*)gates;
  a.hn = hn;
  a.hf_prev = hf_prev;
  a.dc_in = dc_in;
  a.dc_out = dc_out;
  a.dgx = (uint16_t*)dgx;
  a.dgh = (uint16_t*)dgh;
  a.ld_dgn = ld_dgn; a.ld_wt = ld_wt; a.ld_e = ld_e; a.ld_g = ld_g;
  a.ld_hn = ld_hn; a.ld_hfp = ld_hfp; a.ld_dci = ld_dci; a.ld_dco = ld_dco;
  a.ld_dgx = ld_dgx; a.ld_dgh = ld_dgh;
  a.B = B; a.H = H;
  vec = H % 8 == 0 && on_grid(dgx, ld_dgx) && on_grid(dgh, ld_dgh) &&
        on_grid(gates, ld_g) && on_grid(hn, ld_hn) &&
        on_grid(dc_out, ld_dco) &&
        (!dgh_next || (on_grid(dgh_next, ld_dgn) && on_grid(WhT, ld_wt))) &&
        (!err || on_grid(err, ld_e)) &&
        (!hf_prev || on_grid(hf_prev, ld_hfp)) &&
        (!dc_in || on_grid(dc_in, ld_dci));
  return true;
}

}  // namespace

HVK_API int hvk_gru_step_bwd(int B, int H, const void* dgh_next,
                             long long ld_dgn, const void* WhT,
                             long long ld_wt, const void* err, long long ld_e,
                             const void* gates, long long ld_g,
                             const float* hn, long long ld_hn,
                             const float* hf_prev, long long ld_hfp,
                             const float* dc_in, long long ld_dci,
                             float* dc_out, long long ld_dco, void* dgx,
                             long long ld_dgx, void* dgh, long long ld_dgh,
                             hipStream_t s) {
  GruBwdArgs a;
  bool vec;
  if (!gru_bwd_args(a, vec, B, H, dgh_next, ld_dgn, WhT, ld_wt, err, ld_e,
                    gates, ld_g, hn, ld_hn, hf_prev, ld_hfp, dc_in, ld_dci,
                    dc_out, ld_dco, dgx, ld_dgx, dgh, ld_dgh))
    return -1;
  return launch_gru_bwd(a, vec, B, H, s);
}

// One backward GRU time step of both directions in one launch (grid.z = 2):
// the operand list of hvk_gru_step_bwd once per direction, null operands per
// direction, bit for bit what hvk_gru_step_bwd does on either.
HVK_API int hvk_gru_step_bwd2(
    int B, int H, const void* dgh_next0, long long ld_dgn0, const void* WhT0,
    long long ld_wt0, const void* err0, long long ld_e0, const void* gates0,
    long long ld_g0, const float* hn0, long long ld_hn0,
    const float* hf_prev0, long long ld_hfp0, const float* dc_in0,
    long long ld_dci0, float* dc_out0, long long ld_dco0, void* dgx0,
    long long ld_dgx0, void* dgh0, long long ld_dgh0, const void* dgh_next1,
    long long ld_dgn1, const void* WhT1, long long ld_wt1, const void* err1,
    long long ld_e1, const void* gates1, long long ld_g1, const float* hn1,
    long long ld_hn1, const float* hf_prev1, long long ld_hfp1,
    const float* dc_in1, long long ld_dci1, float* dc_out1,
    long long ld_dco1, void* dgx1, long long ld_dgx1, void* dgh1,
    long long ld_dgh1, hipStream_t s) {
  Pair<GruBwdArgs> p;
  GruBwdArgs &a0 = p.d[0], &a1 = p.d[1];
  bool vec0, vec1;
  if (!gru_bwd_args(a0, vec0, B, H, dgh_next0, ld_dgn0, WhT0, ld_wt0, err0,
                    ld_e0, gates0, ld_g0, hn0, ld_hn0, hf_prev0, ld_hfp0,
                    dc_in0, ld_dci0, dc_out0, ld_dco0, dgx0, ld_dgx0, dgh0,
                    ld_dgh0) ||
      !gru_bwd_args(a1, vec1, B, H, dgh_next1, ld_dgn1, WhT1, ld_wt1, err1,
                    ld_e1, gates1, ld_g1, hn1, ld_hn1, hf_prev1, ld_hfp1,
                    dc_in1, ld_dci1, dc_out1, ld_dco1, dgx1, ld_dgx1, dgh1,
                    ld_dgh1))
    return -1;
  return launch_gru_bwd(p, vec0 && vec1, B, H, s);
}
