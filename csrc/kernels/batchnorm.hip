// batchnorm.hip - batch normalisation over the last (channel) axis of a
// [P][C] bf16 tensor (NHWC [N,H,W,C], FC [B,C], recurrent [B,T,H]); gfx950.
//
//   hvk_bn_stats   partial + finish: per-channel mean / invstd, the running
//                  statistics, and the folded table scale = gamma * invstd,
//                  shift = beta - mean * scale
//   hvk_bn_fold    the same table from the running statistics (inference)
//   hvk_bn_apply   y = act(x * scale_c + shift_c)
//   hvk_bn_bwd     partial + finish: dbeta = sum g, dgamma = sum g * xhat and
//                  the coefficients of dx; then the dx pass
//
// Tiling.  A lane owns NV channels (8 on the vector path: one 16-byte load;
// 1 on the guarded element path) and keeps its per-channel constants in
// registers.  A workgroup of 256 lanes is TX channel groups wide and RY rows
// high (bn_geom); workgroups are laid out (channel tile, row slice) and
// stride over the rows.
//
// Reductions are two launches with no atomics and no workgroup waiting for
// another: a workgroup adds its RY row-lanes through LDS in row order and
// writes ONE partial per channel to ws[quantity][channel][slice]; the finish
// kernel gives a wave to a channel, lane j adds slices j, j + 64, ... in
// index order and the wave adds its lanes in a fixed tree.  The number of
// slices is a function of (P, C, path) only (hvk_bn_partials), so the bits
// of a result do not depend on the device, and a rerun repeats them.
//
// Variance: sums of (x - K_c) and (x - K_c)^2 with the shift K_c = the mean
// of channel c over the first min(P, 8) rows (bn_shift), the same bits in
// every lane, so partials add plainly:
//   mean = K + S1 / P,  var = (S2 - S1 * S1 / P) / P.
// E[x^2] - mean^2 would lose mean^2 / var of its digits; here the loss is
// (K - mean)^2 / var: about 1 / 8 when the first rows are typical of the
// channel, and up to (outlier / 8)^2 / var when one of them is not.
#include "hvk_common.h"

using namespace hvk;

namespace {

constexpr int BN_THREADS = 256;
constexpr int BN_MIN_ROWS = 4;      // rows per lane before a new slice opens
constexpr int BN_MAX_WGS = 1024;    // workgroups of a partial kernel
constexpr int BN_APPLY_WGS = 2048;  // workgroups of an elementwise pass
constexpr int BN_FINISH_LANES = 64; // lanes that share a channel's slices

struct BnGeom {
  int CG;   // channel groups of NV channels
  int NTX;  // channel tiles (grid.x)
  int TX;   // channel groups per workgroup, <= 64
  int RY;   // rows per workgroup pass, >= 4
  int G;    // row slices of a reduction (grid.y) = partials per channel
  int GA;   // row slices of an elementwise pass
};

inline BnGeom bn_geom(long long P, int C, bool vec) {
  BnGeom g;
  g.CG = vec ? C / 8 : C;
  g.NTX = (g.CG + 63) / 64;
  g.TX = (g.CG + g.NTX - 1) / g.NTX;
  g.RY = BN_THREADS / g.TX;
  const long long per = (long long)g.RY * BN_MIN_ROWS;
  long long s = (P + per - 1) / per;
  const long long cap = BN_MAX_WGS / g.NTX > 0 ? BN_MAX_WGS / g.NTX : 1;
  g.G = (int)(s < cap ? s : cap);
  if (g.G < 1) g.G = 1;
  s = (P + g.RY - 1) / g.RY;
  const long long capa = BN_APPLY_WGS / g.NTX > 0 ? BN_APPLY_WGS / g.NTX : 1;
  g.GA = (int)(s < capa ? s : capa);
  if (g.GA < 1) g.GA = 1;
  return g;
}

// NV bf16 values at p -> float
template <bool VEC>
__device__ __forceinline__ void bn_load(const uint16_t* p, float* v) {
  if constexpr (VEC) {
    const uint4 u = *(const uint4*)p;
    const uint32_t w[4] = {u.x, u.y, u.z, u.w};
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      v[2 * q] = __uint_as_float(w[q] << 16);
      v[2 * q + 1] = __uint_as_float(w[q] & 0xffff0000u);
    }
  } else {
    v[0] = bf2f(*p);
  }
}
template <bool VEC>
__device__ __forceinline__ void bn_store(uint16_t* p, const float* v) {
  if constexpr (VEC) {
    *(uint4*)p = pack_bf16x8(v);
  } else {
    *p = f2bf(v[0]);
  }
}
// NV floats of a per-channel table
template <bool VEC>
__device__ __forceinline__ void bn_loadf(const float* p, float* v) {
  if constexpr (VEC) {
    const float4 a = ((const float4*)p)[0], b = ((const float4*)p)[1];
    v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w;
    v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
  } else {
    v[0] = *p;
  }
}

constexpr int BN_SHIFT_ROWS = 8;
// The shift of NV channels at xc: their mean over the first rows, added in
// row order (every caller gets the same bits)
template <bool VEC>
__device__ __forceinline__ void bn_shift(const uint16_t* xc, long long ldx,
                                         long long P, float* K) {
  constexpr int NV = VEC ? 8 : 1;
  const int n = P < BN_SHIFT_ROWS ? (int)P : BN_SHIFT_ROWS;
#pragma unroll
  for (int k = 0; k < NV; ++k) K[k] = 0.f;
  for (int r = 0; r < n; ++r) {
    float v[NV];
    bn_load<VEC>(xc + r * ldx, v);
#pragma unroll
    for (int k = 0; k < NV; ++k) K[k] += v[k];
  }
  const float inv = 1.f / (float)n;
#pragma unroll
  for (int k = 0; k < NV; ++k) K[k] *= inv;
}

// lane -> (channel group, row lane); false for a lane outside the tile
struct BnLane {
  int cg, ty;
  bool on;
};
__device__ __forceinline__ BnLane bn_lane(int CG, int TX, int RY) {
  BnLane l;
  const int tx = threadIdx.x % TX;
  l.ty = threadIdx.x / TX;
  l.cg = blockIdx.x * TX + tx;
  l.on = l.ty < RY && l.cg < CG;
  return l;
}

// The workgroup's two per-channel sums -> ws[q][c][slice].  red: 2 * 256 *
// NV floats.  Every lane with ty < RY stores (zeros when it is outside the
// tensor), then lane j adds channel j's RY row-lanes in row order.
template <int NV>
__device__ __forceinline__ void bn_block_partials(const float* a1,
                                                  const float* a2, float* red,
                                                  int TX, int RY, int C,
                                                  float* ws, int G) {
  const int tx = threadIdx.x % TX, ty = threadIdx.x / TX;
  const int W = TX * NV;
  if (ty < RY) {
#pragma unroll
    for (int k = 0; k < NV; ++k) {
      red[ty * W + tx * NV + k] = a1[k];
      red[(RY + ty) * W + tx * NV + k] = a2[k];
    }
  }
  __syncthreads();
  for (int j = threadIdx.x; j < W; j += BN_THREADS) {
    const int c = blockIdx.x * W + j;
    if (c >= C) continue;
    float s1 = 0.f, s2 = 0.f;
    for (int r = 0; r < RY; ++r) {
      s1 += red[r * W + j];
      s2 += red[(RY + r) * W + j];
    }
    ws[(size_t)c * G + blockIdx.y] = s1;
    ws[((size_t)C + c) * G + blockIdx.y] = s2;
  }
}

// sum of ws[0 .. G) over the wave: lane j takes j, j + 64, ... in order
__device__ __forceinline__ float bn_wave_total(const float* ws, int G) {
  float s = 0.f;
  for (int i = threadIdx.x & 63; i < G; i += BN_FINISH_LANES) s += ws[i];
  return wave_sum(s);
}

// ------------------------------------------------------------- statistics
template <bool VEC>
__global__ void __launch_bounds__(BN_THREADS)
bn_stats_partial_kernel(const uint16_t* __restrict__ x, long long ldx,
                        long long P, int C, int CG, int TX, int RY,
                        float* __restrict__ ws) {
  constexpr int NV = VEC ? 8 : 1;
  __shared__ float red[2 * BN_THREADS * NV];
  const BnLane l = bn_lane(CG, TX, RY);
  float a1[NV], a2[NV], K[NV];
#pragma unroll
  for (int k = 0; k < NV; ++k) a1[k] = a2[k] = 0.f;
  if (l.on) {
    const uint16_t* xc = x + (long long)l.cg * NV;
    bn_shift<VEC>(xc, ldx, P, K);
    const long long step = (long long)gridDim.y * RY;
#pragma unroll 4
    for (long long r = (long long)blockIdx.y * RY + l.ty; r < P; r += step) {
      float v[NV];
      bn_load<VEC>(xc + r * ldx, v);
#pragma unroll
      for (int k = 0; k < NV; ++k) {
        const float d = v[k] - K[k];
        a1[k] += d;
        a2[k] = __builtin_fmaf(d, d, a2[k]);
      }
    }
  }
  bn_block_partials<NV>(a1, a2, red, TX, RY, C, ws, gridDim.y);
}

// table: [2][C] = scale, shift
__device__ __forceinline__ void bn_fold_one(float g, float b, float mean,
                                            float invstd, float* table, int C,
                                            int c) {
  const float sc = g * invstd;
  table[c] = sc;
  table[C + c] = __builtin_fmaf(-mean, sc, b);
}

__global__ void __launch_bounds__(BN_THREADS)
bn_stats_finish_kernel(const uint16_t* __restrict__ x, long long ldx,
                       const float* __restrict__ ws, int G, long long P, int C,
                       const float* __restrict__ gamma,
                       const float* __restrict__ beta, float* running_mean,
                       float* running_var, float eps, float momentum,
                       float* __restrict__ mean, float* __restrict__ invstd,
                       float* __restrict__ table) {
  const int c = blockIdx.x * (BN_THREADS / 64) + (threadIdx.x >> 6);
  if (c >= C) return;
  const float s1 = bn_wave_total(ws + (size_t)c * G, G);
  const float s2 = bn_wave_total(ws + ((size_t)C + c) * G, G);
  if ((threadIdx.x & 63) != 0) return;
  const float n = (float)P;
  float K;
  bn_shift<false>(x + c, ldx, P, &K);
  const float m = K + s1 / n;
  const float var = fmaxf((s2 - s1 * (s1 / n)) / n, 0.f);
  const float is = 1.f / sqrtf(var + eps);
  mean[c] = m;
  invstd[c] = is;
  running_mean[c] = (1.f - momentum) * running_mean[c] + momentum * m;
  running_var[c] = (1.f - momentum) * running_var[c] +
                   momentum * (var * (n / (n - 1.f)));
  bn_fold_one(gamma[c], beta[c], m, is, table, C, c);
}

__global__ void __launch_bounds__(BN_THREADS)
bn_fold_kernel(const float* __restrict__ gamma, const float* __restrict__ beta,
               const float* __restrict__ running_mean,
               const float* __restrict__ running_var, int C, float eps,
               float* __restrict__ table) {
  const int c = blockIdx.x * BN_THREADS + threadIdx.x;
  if (c >= C) return;
  bn_fold_one(gamma[c], beta[c], running_mean[c],
              1.f / sqrtf(running_var[c] + eps), table, C, c);
}

// ------------------------------------------------------------------ apply
template <int ACT, bool VEC>
__global__ void __launch_bounds__(BN_THREADS)
bn_apply_kernel(const uint16_t* __restrict__ x, long long ldx,
                uint16_t* __restrict__ y, long long ldy, long long P, int C,
                int CG, int TX, int RY, const float* __restrict__ table) {
  constexpr int NV = VEC ? 8 : 1;
  const BnLane l = bn_lane(CG, TX, RY);
  if (!l.on) return;
  const long long c0 = (long long)l.cg * NV;
  float sc[NV], sh[NV];
  bn_loadf<VEC>(table + c0, sc);
  bn_loadf<VEC>(table + C + c0, sh);
  const long long step = (long long)gridDim.y * RY;
#pragma unroll 4
  for (long long r = (long long)blockIdx.y * RY + l.ty; r < P; r += step) {
    float v[NV];
    bn_load<VEC>(x + r * ldx + c0, v);
#pragma unroll
    for (int k = 0; k < NV; ++k) v[k] = __builtin_fmaf(v[k], sc[k], sh[k]);
    act_fwd_n<NV>(v, ACT);
    bn_store<VEC>(y + r * ldy + c0, v);
  }
}

// --------------------------------------------------------------- backward
// g = err * f'(y) (act != 0: y is read), xhat = (x - mean) * invstd
template <bool VEC>
__global__ void __launch_bounds__(BN_THREADS)
bn_bwd_partial_kernel(const uint16_t* __restrict__ x, long long ldx,
                      const uint16_t* __restrict__ err, long long lde,
                      const uint16_t* __restrict__ y, long long ldy, int act,
                      long long P, int C, int CG, int TX, int RY,
                      const float* __restrict__ mean,
                      const float* __restrict__ invstd,
                      float* __restrict__ ws) {
  constexpr int NV = VEC ? 8 : 1;
  __shared__ float red[2 * BN_THREADS * NV];
  const BnLane l = bn_lane(CG, TX, RY);
  float a1[NV], a2[NV];
#pragma unroll
  for (int k = 0; k < NV; ++k) a1[k] = a2[k] = 0.f;
  if (l.on) {
    const long long c0 = (long long)l.cg * NV;
    float mu[NV], is[NV];
    bn_loadf<VEC>(mean + c0, mu);
    bn_loadf<VEC>(invstd + c0, is);
    const long long step = (long long)gridDim.y * RY;
#pragma unroll 2
    for (long long r = (long long)blockIdx.y * RY + l.ty; r < P; r += step) {
      float v[NV], g[NV];
      bn_load<VEC>(x + r * ldx + c0, v);
      bn_load<VEC>(err + r * lde + c0, g);
      if (act) {
        float yv[NV];
        bn_load<VEC>(y + r * ldy + c0, yv);
        act_bwd_mul_n<NV>(g, yv, act);
      }
#pragma unroll
      for (int k = 0; k < NV; ++k) {
        a1[k] += g[k];
        a2[k] = __builtin_fmaf(g[k], (v[k] - mu[k]) * is[k], a2[k]);
      }
    }
  }
  bn_block_partials<NV>(a1, a2, red, TX, RY, C, ws, gridDim.y);
}

// coef: [3][C]: dx = A g + B (x - mean) + D with A = gamma invstd,
// B = -A invstd dgamma / P, D = -A dbeta / P
__global__ void __launch_bounds__(BN_THREADS)
bn_bwd_finish_kernel(const float* __restrict__ ws, int G, long long P, int C,
                     const float* __restrict__ gamma,
                     const float* __restrict__ invstd, float* dgamma,
                     float* dbeta, int accumulate, float* __restrict__ coef) {
  const int c = blockIdx.x * (BN_THREADS / 64) + (threadIdx.x >> 6);
  if (c >= C) return;
  const float db = bn_wave_total(ws + (size_t)c * G, G);
  const float dg = bn_wave_total(ws + ((size_t)C + c) * G, G);
  if ((threadIdx.x & 63) != 0) return;
  dbeta[c] = accumulate ? dbeta[c] + db : db;
  dgamma[c] = accumulate ? dgamma[c] + dg : dg;
  const float n = (float)P;
  const float A = gamma[c] * invstd[c];
  coef[c] = A;
  coef[C + c] = -A * invstd[c] * (dg / n);
  coef[2 * C + c] = -A * (db / n);
}

template <bool VEC>
__global__ void __launch_bounds__(BN_THREADS)
bn_bwd_apply_kernel(const uint16_t* __restrict__ x, long long ldx,
                    const uint16_t* __restrict__ err, long long lde,
                    const uint16_t* __restrict__ y, long long ldy, int act,
                    const uint16_t* __restrict__ aux, long long lda,
                    int aux_act, uint16_t* __restrict__ dx, long long lddx,
                    long long P, int C, int CG, int TX, int RY,
                    const float* __restrict__ mean,
                    const float* __restrict__ coef) {
  constexpr int NV = VEC ? 8 : 1;
  const BnLane l = bn_lane(CG, TX, RY);
  if (!l.on) return;
  const long long c0 = (long long)l.cg * NV;
  float mu[NV], A[NV], B[NV], D[NV];
  bn_loadf<VEC>(mean + c0, mu);
  bn_loadf<VEC>(coef + c0, A);
  bn_loadf<VEC>(coef + C + c0, B);
  bn_loadf<VEC>(coef + 2 * (long long)C + c0, D);
  const long long step = (long long)gridDim.y * RY;
#pragma unroll 2
  for (long long r = (long long)blockIdx.y * RY + l.ty; r < P; r += step) {
    float v[NV], g[NV];
    bn_load<VEC>(x + r * ldx + c0, v);
    bn_load<VEC>(err + r * lde + c0, g);
    if (act) {
      float yv[NV];
      bn_load<VEC>(y + r * ldy + c0, yv);
      act_bwd_mul_n<NV>(g, yv, act);
    }
#pragma unroll
    for (int k = 0; k < NV; ++k)
      v[k] = __builtin_fmaf(A[k], g[k],
                            __builtin_fmaf(B[k], v[k] - mu[k], D[k]));
    if (aux_act) {
      float av[NV];
      bn_load<VEC>(aux + r * lda + c0, av);
      act_bwd_mul_n<NV>(v, av, aux_act);
    }
    bn_store<VEC>(dx + r * lddx + c0, v);
  }
}

inline bool bn_shape_ok(long long P, int C) {
  return P >= 1 && C >= 1 && P <= ((1ll << 31) - 1) / C;
}
inline bool on16(const void* p, long long ld) {
  return p == nullptr || ((((uintptr_t)p) & 15) == 0 && ld % 8 == 0);
}
inline bool pitch_ok(const void* p, long long ld, int C) {
  return p == nullptr || ld >= C;
}

template <bool VEC>
void bn_apply_launch(int act, dim3 grid, hipStream_t s, const uint16_t* x,
                     long long ldx, uint16_t* y, long long ldy, long long P,
                     int C, const BnGeom& g, const float* table) {
#define HVK_BN_APPLY(A)                                                      \
  hipLaunchKernelGGL((bn_apply_kernel<A, VEC>), grid, dim3(BN_THREADS), 0, s, \
                     x, ldx, y, ldy, P, C, g.CG, g.TX, g.RY, table)
  switch (act) {
    case ACT_TANH: HVK_BN_APPLY(ACT_TANH); break;
    case ACT_RELU: HVK_BN_APPLY(ACT_RELU); break;
    case ACT_STRICT_RELU: HVK_BN_APPLY(ACT_STRICT_RELU); break;
    case ACT_SIGMOID: HVK_BN_APPLY(ACT_SIGMOID); break;
    default: HVK_BN_APPLY(ACT_LINEAR); break;
  }
#undef HVK_BN_APPLY
}

}  // namespace

// Partials per channel of the two reductions over a [P][C] tensor: a
// function of the shape and of the path (vec: 8 channels per lane) only.
// The workspaces of hvk_bn_stats and hvk_bn_bwd hold 2 * C * this floats.
HVK_API int hvk_bn_partials(long long P, int C, int vec) {
  if (!bn_shape_ok(P, C) || (vec && C % 8)) return -1;
  return bn_geom(P, C, vec != 0).G;
}

// 1 when a [P][C] tensor at x with row pitch ldx (elements) takes the
// vector path
HVK_API int hvk_bn_vec(const void* x, long long ldx, int C) {
  return C % 8 == 0 && on16(x, ldx) ? 1 : 0;
}

// Training statistics of x[P][C] (bf16, row pitch ldx elements, P >= 2):
// mean, invstd [C]; running_mean / running_var updated in place with the
// unbiased variance; table [2][C] = gamma * invstd, beta - mean * that.
// vec: the caller's path (hvk_bn_vec of every tensor of the layer), which
// fixed the size of ws.
HVK_API int hvk_bn_stats(const void* x, long long ldx, long long P, int C,
                         int vec, const float* gamma, const float* beta,
                         float* running_mean, float* running_var, float eps,
                         float momentum, float* mean, float* invstd,
                         float* table, float* ws, hipStream_t s) {
  if (!x || !gamma || !beta || !running_mean || !running_var || !mean ||
      !invstd || !table || !ws || !bn_shape_ok(P, C) || P < 2 || ldx < C ||
      (vec && !hvk_bn_vec(x, ldx, C)))
    return -1;
  const BnGeom g = bn_geom(P, C, vec != 0);
  const dim3 grid(g.NTX, g.G);
  const uint16_t* xp = (const uint16_t*)x;
  if (vec)
    hipLaunchKernelGGL(bn_stats_partial_kernel<true>, grid, dim3(BN_THREADS),
                       0, s, xp, ldx, P, C, g.CG, g.TX, g.RY, ws);
  else
    hipLaunchKernelGGL(bn_stats_partial_kernel<false>, grid, dim3(BN_THREADS),
                       0, s, xp, ldx, P, C, g.CG, g.TX, g.RY, ws);
  hipLaunchKernelGGL(bn_stats_finish_kernel, dim3((C + 3) / 4),
                     dim3(BN_THREADS), 0, s, xp, ldx, ws, g.G, P, C, gamma,
                     beta, running_mean, running_var, eps, momentum, mean,
                     invstd, table);
  return (int)launch_status(s);
}

HVK_API int hvk_bn_fold(const float* gamma, const float* beta,
                        const float* running_mean, const float* running_var,
                        int C, float eps, float* table, hipStream_t s) {
  if (!gamma || !beta || !running_mean || !running_var || !table || C < 1)
    return -1;
  hipLaunchKernelGGL(bn_fold_kernel, dim3((C + BN_THREADS - 1) / BN_THREADS),
                     dim3(BN_THREADS), 0, s, gamma, beta, running_mean,
                     running_var, C, eps, table);
  return (int)launch_status(s);
}

// y = act(x * table[0][c] + table[1][c]); bf16 [P][C] with row pitches
HVK_API int hvk_bn_apply(const void* x, long long ldx, void* y, long long ldy,
                         long long P, int C, const float* table, int act,
                         hipStream_t s) {
  if (!x || !y || !table || !bn_shape_ok(P, C) || ldx < C || ldy < C ||
      act < 0 || act > 4)
    return -1;
  const bool vec = C % 8 == 0 && on16(x, ldx) && on16(y, ldy);
  const BnGeom g = bn_geom(P, C, vec);
  const dim3 grid(g.NTX, g.GA);
  if (vec)
    bn_apply_launch<true>(act, grid, s, (const uint16_t*)x, ldx, (uint16_t*)y,
                          ldy, P, C, g, table);
  else
    bn_apply_launch<false>(act, grid, s, (const uint16_t*)x, ldx,
                           (uint16_t*)y, ldy, P, C, g, table);
  return (int)launch_status(s);
}

// Backward of the training forward.  g = err * f'(y) when act != 0 (y may be
// null otherwise); dgamma / dbeta written or added to (accumulate); dx
// (null: not wanted) = gamma invstd (g - dbeta / P - xhat dgamma / P), times
// f'(aux) when aux_act != 0.  coef: [3][C], ws: 2 * C * hvk_bn_partials.
HVK_API int hvk_bn_bwd(const void* x, long long ldx, const void* err,
                       long long lde, const void* y, long long ldy,
                       const void* aux, long long lda, void* dx,
                       long long lddx, long long P, int C, int vec,
                       const float* gamma, const float* mean,
                       const float* invstd, float* dgamma, float* dbeta,
                       int accumulate, int act, int aux_act, float* coef,
                       float* ws, hipStream_t s) {
  if (!x || !err || !gamma || !mean || !invstd || !dgamma || !dbeta ||
      !coef || !ws || !bn_shape_ok(P, C) || act < 0 || act > 4 ||
      aux_act < 0 || aux_act > 4 || (act && !y) || (aux_act && !aux) ||
      ldx < C || lde < C || !pitch_ok(act ? y : nullptr, ldy, C) ||
      !pitch_ok(aux_act ? aux : nullptr, lda, C) || !pitch_ok(dx, lddx, C))
    return -1;
  if (!act) y = nullptr;
  if (!aux_act) aux = nullptr;
  if (vec && !(C % 8 == 0 && on16(x, ldx) && on16(err, lde) && on16(y, ldy) &&
               on16(aux, lda) && on16(dx, lddx)))
    return -1;
  const BnGeom g = bn_geom(P, C, vec != 0);
  const dim3 grid(g.NTX, g.G), grida(g.NTX, g.GA);
  const uint16_t *xp = (const uint16_t*)x, *ep = (const uint16_t*)err,
                 *yp = (const uint16_t*)y, *ap = (const uint16_t*)aux;
  if (vec)
    hipLaunchKernelGGL(bn_bwd_partial_kernel<true>, grid, dim3(BN_THREADS), 0,
                       s, xp, ldx, ep, lde, yp, ldy, act, P, C, g.CG, g.TX,
                       g.RY, mean, invstd, ws);
  else
    hipLaunchKernelGGL(bn_bwd_partial_kernel<false>, grid, dim3(BN_THREADS),
                       0, s, xp, ldx, ep, lde, yp, ldy, act, P, C, g.CG, g.TX,
                       g.RY, mean, invstd, ws);
  hipLaunchKernelGGL(bn_bwd_finish_kernel, dim3((C + 3) / 4),
                     dim3(BN_THREADS), 0, s, ws, g.G, P, C, gamma, invstd,
                     dgamma, dbeta, accumulate, coef);
  if (dx) {
    if (vec)
      hipLaunchKernelGGL(bn_bwd_apply_kernel<true>, grida, dim3(BN_THREADS),
                         0, s, xp, ldx, ep, lde, yp, ldy, act, ap, lda,
                         aux_act, (uint16_t*)dx, lddx, P, C, g.CG, g.TX, g.RY,
                         mean, coef);
    else
      hipLaunchKernelGGL(bn_bwd_apply_kernel<false>, grida, dim3(BN_THREADS),
                         0, s, xp, ldx, ep, lde, yp, ldy, act, ap, lda,
                         aux_act, (uint16_t*)dx, lddx, P, C, g.CG, g.TX, g.RY,
                         mean, coef);
  }
  return (int)launch_status(s);
}
