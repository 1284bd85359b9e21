// layernorm.hip - layer normalisation over the last axis of a [P][C] bf16
// tensor ([B][T][E], [B][C], NHWC), with an optional fused residual add, and
// the plain residual add; gfx950.
//
//   hvk_ln_fwd   s = x (+ r), mean / invstd per row (float32 [P]),
//                y = gamma (s - mean) invstd + beta; one launch
//   hvk_ln_bwd   dx = invstd (gh - mean_C(gh) - sh mean_C(gh sh)) with
//                gh = err gamma, sh = (s - mean) invstd; dbeta = sum_P err,
//                dgamma = sum_P err sh in two launches
//   hvk_add      out = bf16(float(a) + float(b))
//
// Row ownership.  A row belongs to L lanes: 16, 32 or 64 lanes of one wave,
// or the 256 lanes of a workgroup; a workgroup of 256 lanes works on 256 / L
// rows at a time and strides over the rows.  A lane keeps K groups of NV
// values of its row (NV = 8 on the vector path: one 16-byte access; 1 on the
// guarded element path) in registers from the load to the store; element
// rows of 1025 .. 8192 columns are kept in LDS instead (32 values per lane
// in registers made the compiler spill scalar registers).  Either way x
// (and r) are read ONCE for C <= LN_REG_C = 8192.  Wider rows take the
// re-reading kernels: the forward reads its inputs three times (mean,
// variance, apply), the backward's dx kernel twice.
//
// Statistics: mean = sum s / C, then var = sum (s - mean)^2 / C on the
// registers (on the re-read path: on the second read), never E[s^2] -
// mean^2.  With a residual s = float(x) + float(r) in float32 is never
// stored: the backward adds the two again.
//
// Lanes are combined by xor exchanges at fixed distances (wave_sum's
// pattern, cut to L lanes) and, for a workgroup row, the four waves' sums
// through LDS in wave order, so a rerun repeats its bits.
//
// dgamma / dbeta are column sums over P: no atomics, no workgroup waiting
// for another.  Workgroup b keeps the column sums of its rows in registers,
// adds its 256 / L row groups through LDS in group order and writes ONE
// partial per column to ws[quantity][b][c]; the finish kernel adds the G
// slices of a column: 16 lanes take slices j, j + 16, ... in index order,
// then the 16 in lane order.  G is a function of (P, C, path) only
// (hvk_ln_partials).  The partials are taken inside the dx kernel (6 B per
// element: x, err read, dx written), not in a read pass of their own as in
// bn_bwd (10 B per element): see ln_cols_fused.  The separate pass stays
// behind hvk_ln_colsum for the A/B, and serves a backward without dx.
#include "hvk_common.h"

using namespace hvk;

namespace {

constexpr int LN_THREADS = 256;
constexpr int LN_REG_C = 8192;     // widest row kept in registers
constexpr int LN_FWD_WGS = 2048;   // workgroups of the forward / dx-only pass
constexpr int LN_MIN_ROWS = 4;     // rows per row group before a slice opens
constexpr int LN_MAX_SLICES = 1024;  // workgroups of a pass with column sums
constexpr int LN_FIN_CH = 16;      // finish: columns per workgroup
constexpr int LN_FIN_GR = LN_THREADS / LN_FIN_CH;  // lanes per column
constexpr int LN_FIN_BATCH = 16;   // finish: loads in flight per quantity
constexpr int LN_ADD_WGS_X = 2048, LN_ADD_WGS_Y = 1024;

// -1: ln_cols_fused decides; 0: always a separate pass; 1: always fused.
// A measuring switch for tools/bench_layernorm.py and the tests only: one
// plain int for the whole process, not guarded against concurrent callers
// and not meant for a training run (results do not depend on it: the slices
// are the same either way).
int g_ln_colsum = -1;

struct LnPath {
  int L, K;   // lanes per row, groups per lane; K = 0: the column-loop
              // kernels (staged in LDS, or re-reading past LN_REG_C)
  int CG;     // groups of NV columns
  int RPB;    // rows per workgroup pass
};

inline LnPath ln_path(int C, bool vec) {
  LnPath p;
  p.CG = vec ? C / 8 : C;
  if (C > LN_REG_C) { p.L = 256; p.K = 0; }
  else if (vec) {
    if (p.CG <= 16) { p.L = 16; p.K = 1; }
    else if (p.CG <= 32) { p.L = 32; p.K = 1; }
    else if (p.CG <= 64) { p.L = 64; p.K = 1; }
    else if (p.CG <= 128) { p.L = 64; p.K = 2; }
    else if (p.CG <= 256) { p.L = 64; p.K = 4; }
    else if (p.CG <= 512) { p.L = 256; p.K = 2; }
    else { p.L = 256; p.K = 4; }
  } else {
    if (p.CG <= 16) { p.L = 16; p.K = 1; }
    else if (p.CG <= 64) { p.L = 64; p.K = 1; }
    else if (p.CG <= 256) { p.L = 64; p.K = 4; }
    else if (p.CG <= 1024) { p.L = 256; p.K = 4; }
    else { p.L = 256; p.K = 0; }   // staged in LDS up to LN_REG_C
  }
  p.RPB = LN_THREADS / p.L;
  return p;
}

inline int ln_slices(long long P, const LnPath& p) {
  const long long per = (long long)p.RPB * LN_MIN_ROWS;
  const long long s = (P + per - 1) / per;
  return (int)(s < LN_MAX_SLICES ? (s < 1 ? 1 : s) : LN_MAX_SLICES);
}

// The column sums ride in the dx kernel (2 * K * NV accumulators per lane):
// faster than a read pass of their own at every shape of the same-process
// A/B (docs/OPS.md, profiles/layernorm/ab_bwd_colsum.txt).  Every
// instantiation of ln_path has K * NV <= 32, the widest that was measured; a
// wider one takes the separate pass until it is measured too.
inline bool ln_cols_fused(const LnPath& p, bool vec) {
  if (g_ln_colsum >= 0) return g_ln_colsum != 0;
  return p.K * (vec ? 8 : 1) <= 32;
}

template <bool VEC>
__device__ __forceinline__ void ln_load(const uint16_t* p, float* v) {
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
__device__ __forceinline__ void ln_store(uint16_t* p, const float* v) {
  if constexpr (VEC) {
    *(uint4*)p = pack_bf16x8(v);
  } else {
    *p = f2bf(v[0]);
  }
}
template <bool VEC>
__device__ __forceinline__ void ln_loadf(const float* p, float* v) {
  if constexpr (VEC) {
    const float4 a = ((const float4*)p)[0], b = ((const float4*)p)[1];
    v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w;
    v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
  } else {
    v[0] = *p;
  }
}
template <bool VEC>
__device__ __forceinline__ void ln_storef(float* p, const float* v) {
  if constexpr (VEC) {
    ((float4*)p)[0] = make_float4(v[0], v[1], v[2], v[3]);
    ((float4*)p)[1] = make_float4(v[4], v[5], v[6], v[7]);
  } else {
    *p = v[0];
  }
}
// s = float(x) (+ float(r)) of NV columns
template <bool VEC>
__device__ __forceinline__ void ln_load_s(const uint16_t* x,
                                          const uint16_t* r, float* v) {
  constexpr int NV = VEC ? 8 : 1;
  ln_load<VEC>(x, v);
  if (r) {
    float t[NV];
    ln_load<VEC>(r, t);
#pragma unroll
    for (int j = 0; j < NV; ++j) v[j] += t[j];
  }
}

// The sum of v over the L lanes of a row, the same bits in every one of
// them.  L = 256: red holds 4 floats, and every lane of the workgroup calls
// (one barrier; the caller alternates between two red arrays).
template <int L>
__device__ __forceinline__ float ln_group_sum(float v, float* red) {
#pragma unroll
  for (int o = (L < 64 ? L : 64) / 2; o > 0; o >>= 1)
    v += __shfl_xor(v, o, 64);
  if constexpr (L == 256) {
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    v = ((red[0] + red[1]) + red[2]) + red[3];
  }
  return v;
}

// ---------------------------------------------------------------- forward
template <bool VEC, int K, int L>
__global__ void __launch_bounds__(LN_THREADS)
ln_fwd_kernel(const uint16_t* __restrict__ x, long long ldx,
              const uint16_t* __restrict__ r, long long ldr,
              uint16_t* __restrict__ y, long long ldy, long long P, int C,
              int CG, const float* __restrict__ gamma,
              const float* __restrict__ beta, float eps,
              float* __restrict__ mean, float* __restrict__ invstd) {
  constexpr int NV = VEC ? 8 : 1, RPB = LN_THREADS / L;
  __shared__ float red[2][4];
  const int sub = threadIdx.x / L, lane = threadIdx.x % L;
  const float n = (float)C;
  const long long step = (long long)gridDim.x * RPB;
  for (long long base = (long long)blockIdx.x * RPB; base < P; base += step) {
    const long long row = base + sub;
    const bool on = row < P;
    float v[K][NV];
    float s = 0.f;
#pragma unroll
    for (int k = 0; k < K; ++k) {
      const int cg = lane + L * k;
      if (on && cg < CG) {
        const long long c0 = (long long)cg * NV;
        ln_load_s<VEC>(x + row * ldx + c0, r ? r + row * ldr + c0 : nullptr,
                       v[k]);
      } else {
#pragma unroll
        for (int j = 0; j < NV; ++j) v[k][j] = 0.f;
      }
#pragma unroll
      for (int j = 0; j < NV; ++j) s += v[k][j];
    }
    const float mu = ln_group_sum<L>(s, red[0]) / n;
    float q = 0.f;
#pragma unroll
    for (int k = 0; k < K; ++k) {
      if (lane + L * k < CG) {
#pragma unroll
        for (int j = 0; j < NV; ++j) {
          v[k][j] -= mu;
          q = __builtin_fmaf(v[k][j], v[k][j], q);
        }
      }
    }
    const float var = ln_group_sum<L>(q, red[1]) / n;
    const float is = 1.f / sqrtf(var + eps);
#pragma unroll
    for (int k = 0; k < K; ++k) {
      const int cg = lane + L * k;
      if (on && cg < CG) {
        const long long c0 = (long long)cg * NV;
        float g[NV], b[NV];
        ln_loadf<VEC>(gamma + c0, g);
        ln_loadf<VEC>(beta + c0, b);
#pragma unroll
        for (int j = 0; j < NV; ++j)
          v[k][j] = __builtin_fmaf(v[k][j] * is, g[j], b[j]);
        ln_store<VEC>(y + row * ldy + c0, v[k]);
      }
    }
    if (on && lane == 0) {
      mean[row] = mu;
      invstd[row] = is;
    }
  }
}

// A workgroup per row, a column loop per lane.  STAGE (element path, C <=
// LN_REG_C): the row is read once and s kept in LDS, each lane reading back
// what it wrote; otherwise (C > LN_REG_C) three reads.
template <bool VEC, bool STAGE>
__global__ void __launch_bounds__(LN_THREADS)
ln_fwd_rr_kernel(const uint16_t* __restrict__ x, long long ldx,
                 const uint16_t* __restrict__ r, long long ldr,
                 uint16_t* __restrict__ y, long long ldy, long long P, int C,
                 int CG, const float* __restrict__ gamma,
                 const float* __restrict__ beta, float eps,
                 float* __restrict__ mean, float* __restrict__ invstd) {
  static_assert(!(VEC && STAGE), "the staged rows are the element path's");
  constexpr int NV = VEC ? 8 : 1;
  __shared__ float red[2][4];
  __shared__ float sm[STAGE ? LN_REG_C : 1];
  const float n = (float)C;
  for (long long row = blockIdx.x; row < P; row += gridDim.x) {
    const uint16_t* xr = x + row * ldx;
    const uint16_t* rr = r ? r + row * ldr : nullptr;
    float s = 0.f;
    for (int cg = threadIdx.x; cg < CG; cg += LN_THREADS) {
      float v[NV];
      ln_load_s<VEC>(xr + (long long)cg * NV, rr ? rr + (long long)cg * NV
                                                  : nullptr, v);
      if constexpr (STAGE) sm[cg] = v[0];
#pragma unroll
      for (int j = 0; j < NV; ++j) s += v[j];
    }
    const float mu = ln_group_sum<256>(s, red[0]) / n;
    float q = 0.f;
    for (int cg = threadIdx.x; cg < CG; cg += LN_THREADS) {
      float v[NV];
      if constexpr (STAGE)
        v[0] = sm[cg];
      else
        ln_load_s<VEC>(xr + (long long)cg * NV, rr ? rr + (long long)cg * NV
                                                    : nullptr, v);
#pragma unroll
      for (int j = 0; j < NV; ++j) {
        const float d = v[j] - mu;
        q = __builtin_fmaf(d, d, q);
      }
    }
    const float var = ln_group_sum<256>(q, red[1]) / n;
    const float is = 1.f / sqrtf(var + eps);
    for (int cg = threadIdx.x; cg < CG; cg += LN_THREADS) {
      const long long c0 = (long long)cg * NV;
      float v[NV], g[NV], b[NV];
      if constexpr (STAGE)
        v[0] = sm[cg];
      else
        ln_load_s<VEC>(xr + c0, rr ? rr + c0 : nullptr, v);
      ln_loadf<VEC>(gamma + c0, g);
      ln_loadf<VEC>(beta + c0, b);
#pragma unroll
      for (int j = 0; j < NV; ++j)
        v[j] = __builtin_fmaf((v[j] - mu) * is, g[j], b[j]);
      ln_store<VEC>(y + row * ldy + c0, v);
    }
    if (threadIdx.x == 0) {
      mean[row] = mu;
      invstd[row] = is;
    }
  }
}

// --------------------------------------------------------------- backward
// One quantity's column sums of a lane's group k: the RPB row groups of the
// workgroup are added in group order through comb ([RPB - 1][NV][L]) and
// group 0 writes the slice.
template <bool VEC, int L>
__device__ __forceinline__ void ln_cols_out(float* a, float* comb, int sub,
                                            int lane, int cg, int CG,
                                            float* wsq) {
  constexpr int NV = VEC ? 8 : 1, RPB = LN_THREADS / L;
  if constexpr (RPB > 1) {
    if (sub > 0) {
#pragma unroll
      for (int j = 0; j < NV; ++j)
        comb[((sub - 1) * NV + j) * L + lane] = a[j];
    }
    __syncthreads();
    if (sub == 0) {
      for (int t = 0; t < RPB - 1; ++t) {
#pragma unroll
        for (int j = 0; j < NV; ++j) a[j] += comb[(t * NV + j) * L + lane];
      }
    }
    __syncthreads();
  }
  if (sub == 0 && cg < CG) ln_storef<VEC>(wsq + (long long)cg * NV, a);
}

// DX: write dx; COLS: write this workgroup's slice of ws[2][G][C]
// (G = gridDim.x): [0] sums of err, [1] sums of err * sh
template <bool VEC, int K, int L, bool DX, bool COLS>
__global__ void __launch_bounds__(LN_THREADS)
ln_bwd_kernel(const uint16_t* __restrict__ err, long long lde,
              const uint16_t* __restrict__ x, long long ldx,
              const uint16_t* __restrict__ r, long long ldr,
              uint16_t* __restrict__ dx, long long lddx, long long P, int C,
              int CG, const float* __restrict__ gamma,
              const float* __restrict__ mean,
              const float* __restrict__ invstd, float* __restrict__ ws) {
  constexpr int NV = VEC ? 8 : 1, RPB = LN_THREADS / L;
  __shared__ float red[2][4];
  __shared__ float comb[COLS && RPB > 1 ? (RPB - 1) * NV * L : 1];
  const int sub = threadIdx.x / L, lane = threadIdx.x % L;
  const float n = (float)C;
  float a1[COLS ? K : 1][NV], a2[COLS ? K : 1][NV];
  if constexpr (COLS) {
#pragma unroll
    for (int k = 0; k < K; ++k)
#pragma unroll
      for (int j = 0; j < NV; ++j) a1[k][j] = a2[k][j] = 0.f;
  }
  const long long step = (long long)gridDim.x * RPB;
  for (long long base = (long long)blockIdx.x * RPB; base < P; base += step) {
    const long long row = base + sub;
    const bool on = row < P;
    const float mu = on ? mean[row] : 0.f, is = on ? invstd[row] : 0.f;
    float v[K][NV], g[K][NV];
    float c1 = 0.f, c2 = 0.f;
#pragma unroll
    for (int k = 0; k < K; ++k) {
      const int cg = lane + L * k;
      if (on && cg < CG) {
        const long long c0 = (long long)cg * NV;
        ln_load_s<VEC>(x + row * ldx + c0, r ? r + row * ldr + c0 : nullptr,
                       v[k]);
        ln_load<VEC>(err + row * lde + c0, g[k]);
#pragma unroll
        for (int j = 0; j < NV; ++j) v[k][j] = (v[k][j] - mu) * is;
        if constexpr (COLS) {
#pragma unroll
          for (int j = 0; j < NV; ++j) {
            a1[k][j] += g[k][j];
            a2[k][j] = __builtin_fmaf(g[k][j], v[k][j], a2[k][j]);
          }
        }
        if constexpr (DX) {
          float gm[NV];
          ln_loadf<VEC>(gamma + c0, gm);
#pragma unroll
          for (int j = 0; j < NV; ++j) {
            g[k][j] *= gm[j];
            c1 += g[k][j];
            c2 = __builtin_fmaf(g[k][j], v[k][j], c2);
          }
        }
      }
    }
    if constexpr (DX) {
      c1 = ln_group_sum<L>(c1, red[0]) / n;
      c2 = ln_group_sum<L>(c2, red[1]) / n;
#pragma unroll
      for (int k = 0; k < K; ++k) {
        const int cg = lane + L * k;
        if (on && cg < CG) {
#pragma unroll
          for (int j = 0; j < NV; ++j)
            g[k][j] = is * (g[k][j] - c1 - v[k][j] * c2);
          ln_store<VEC>(dx + row * lddx + (long long)cg * NV, g[k]);
        }
      }
    }
  }
  if constexpr (COLS) {
    float* w1 = ws + (long long)blockIdx.x * C;
    float* w2 = ws + ((long long)gridDim.x + blockIdx.x) * C;
#pragma unroll
    for (int k = 0; k < K; ++k) {
      const int cg = lane + L * k;
      ln_cols_out<VEC, L>(a1[k], comb, sub, lane, cg, CG, w1);
      ln_cols_out<VEC, L>(a2[k], comb, sub, lane, cg, CG, w2);
    }
  }
}

// dx of a workgroup row.  STAGE (element path, C <= LN_REG_C): one read, sh
// and gh kept in LDS; otherwise two reads of err, x (and r)
template <bool VEC, bool STAGE>
__global__ void __launch_bounds__(LN_THREADS)
ln_bwd_rr_dx_kernel(const uint16_t* __restrict__ err, long long lde,
                    const uint16_t* __restrict__ x, long long ldx,
                    const uint16_t* __restrict__ r, long long ldr,
                    uint16_t* __restrict__ dx, long long lddx, long long P,
                    int C, int CG, const float* __restrict__ gamma,
                    const float* __restrict__ mean,
                    const float* __restrict__ invstd) {
  static_assert(!(VEC && STAGE), "the staged rows are the element path's");
  constexpr int NV = VEC ? 8 : 1;
  __shared__ float red[2][4];
  __shared__ float sv[STAGE ? LN_REG_C : 1], sg[STAGE ? LN_REG_C : 1];
  const float n = (float)C;
  for (long long row = blockIdx.x; row < P; row += gridDim.x) {
    const uint16_t* xr = x + row * ldx;
    const uint16_t* rr = r ? r + row * ldr : nullptr;
    const uint16_t* er = err + row * lde;
    const float mu = mean[row], is = invstd[row];
    float c1 = 0.f, c2 = 0.f;
    for (int cg = threadIdx.x; cg < CG; cg += LN_THREADS) {
      const long long c0 = (long long)cg * NV;
      float v[NV], g[NV], gm[NV];
      ln_load_s<VEC>(xr + c0, rr ? rr + c0 : nullptr, v);
      ln_load<VEC>(er + c0, g);
      ln_loadf<VEC>(gamma + c0, gm);
#pragma unroll
      for (int j = 0; j < NV; ++j) {
        const float gh = g[j] * gm[j], sh = (v[j] - mu) * is;
        if constexpr (STAGE) {
          sv[cg] = sh;
          sg[cg] = gh;
        }
        c1 += gh;
        c2 = __builtin_fmaf(gh, sh, c2);
      }
    }
    c1 = ln_group_sum<256>(c1, red[0]) / n;
    c2 = ln_group_sum<256>(c2, red[1]) / n;
    for (int cg = threadIdx.x; cg < CG; cg += LN_THREADS) {
      const long long c0 = (long long)cg * NV;
      float v[NV], g[NV], gm[NV];
      if constexpr (STAGE) {
        g[0] = is * (sg[cg] - c1 - sv[cg] * c2);
      } else {
        ln_load_s<VEC>(xr + c0, rr ? rr + c0 : nullptr, v);
        ln_load<VEC>(er + c0, g);
        ln_loadf<VEC>(gamma + c0, gm);
#pragma unroll
        for (int j = 0; j < NV; ++j)
          g[j] = is * (g[j] * gm[j] - c1 - ((v[j] - mu) * is) * c2);
      }
      ln_store<VEC>(dx + row * lddx + c0, g);
    }
  }
}

// rows wider than LN_REG_C: the column sums of rows b, b + G, ... (one read)
template <bool VEC>
__global__ void __launch_bounds__(LN_THREADS)
ln_bwd_rr_cols_kernel(const uint16_t* __restrict__ err, long long lde,
                      const uint16_t* __restrict__ x, long long ldx,
                      const uint16_t* __restrict__ r, long long ldr,
                      long long P, int C, int CG,
                      const float* __restrict__ mean,
                      const float* __restrict__ invstd,
                      float* __restrict__ ws) {
  constexpr int NV = VEC ? 8 : 1;
  for (int cg = threadIdx.x; cg < CG; cg += LN_THREADS) {
    const long long c0 = (long long)cg * NV;
    float a1[NV], a2[NV];
#pragma unroll
    for (int j = 0; j < NV; ++j) a1[j] = a2[j] = 0.f;
    for (long long row = blockIdx.x; row < P; row += gridDim.x) {
      float v[NV], g[NV];
      ln_load_s<VEC>(x + row * ldx + c0, r ? r + row * ldr + c0 : nullptr, v);
      ln_load<VEC>(err + row * lde + c0, g);
      const float mu = mean[row], is = invstd[row];
#pragma unroll
      for (int j = 0; j < NV; ++j) {
        a1[j] += g[j];
        a2[j] = __builtin_fmaf(g[j], (v[j] - mu) * is, a2[j]);
      }
    }
    ln_storef<VEC>(ws + (long long)blockIdx.x * C + c0, a1);
    ln_storef<VEC>(ws + ((long long)gridDim.x + blockIdx.x) * C + c0, a2);
  }
}

// ws[2][G][C] -> dbeta, dgamma: lane group t of a column adds slices t,
// t + 16, ... in index order, then the 16 are added in order.  The loads of
// LN_FIN_BATCH slices are issued before their sums are taken (the pass is
// bound by the latency of a load, not by its bytes).
__global__ void __launch_bounds__(LN_THREADS)
ln_bwd_finish_kernel(const float* __restrict__ ws, int G, int C,
                     float* dgamma, float* dbeta, int accumulate) {
  __shared__ float fin[2][LN_FIN_GR][LN_FIN_CH];
  const int tx = threadIdx.x % LN_FIN_CH, t = threadIdx.x / LN_FIN_CH;
  const int c = blockIdx.x * LN_FIN_CH + tx;
  float s1 = 0.f, s2 = 0.f;
  if (c < C) {
    const float* w1 = ws + c;
    const float* w2 = ws + (long long)G * C + c;
    for (int g0 = t; g0 < G; g0 += LN_FIN_GR * LN_FIN_BATCH) {
      float u1[LN_FIN_BATCH], u2[LN_FIN_BATCH];
#pragma unroll
      for (int i = 0; i < LN_FIN_BATCH; ++i) {
        const int g = g0 + i * LN_FIN_GR;
        u1[i] = g < G ? w1[(long long)g * C] : 0.f;
        u2[i] = g < G ? w2[(long long)g * C] : 0.f;
      }
#pragma unroll
      for (int i = 0; i < LN_FIN_BATCH; ++i) {
        s1 += u1[i];
        s2 += u2[i];
      }
    }
  }
  fin[0][t][tx] = s1;
  fin[1][t][tx] = s2;
  __syncthreads();
  if (t != 0 || c >= C) return;
  float db = 0.f, dg = 0.f;
#pragma unroll
  for (int i = 0; i < LN_FIN_GR; ++i) {
    db += fin[0][i][tx];
    dg += fin[1][i][tx];
  }
  dbeta[c] = accumulate ? dbeta[c] + db : db;
  dgamma[c] = accumulate ? dgamma[c] + dg : dg;
}

// -------------------------------------------------------------------- add
template <bool VEC>
__global__ void __launch_bounds__(LN_THREADS)
ln_add_kernel(const uint16_t* a, long long lda, const uint16_t* b,
              long long ldb, uint16_t* out, long long ldo, long long P,
              long long CG) {   // out may be a or b: no __restrict__
  constexpr int NV = VEC ? 8 : 1;
  const long long stepx = (long long)gridDim.x * LN_THREADS;
  for (long long row = blockIdx.y; row < P; row += gridDim.y) {
    for (long long cg = (long long)blockIdx.x * LN_THREADS + threadIdx.x;
         cg < CG; cg += stepx) {
      const long long c0 = cg * NV;
      float u[NV], v[NV];
      ln_load<VEC>(a + row * lda + c0, u);
      ln_load<VEC>(b + row * ldb + c0, v);
#pragma unroll
      for (int j = 0; j < NV; ++j) u[j] += v[j];
      ln_store<VEC>(out + row * ldo + c0, u);
    }
  }
}

inline bool ln_shape_ok(long long P, int C) {
  return P >= 1 && C >= 1 && P <= ((1ll << 31) - 1) / C;
}
inline bool ln_on16(const void* p, long long ld) {
  return p == nullptr || ((((uintptr_t)p) & 15) == 0 && ld % 8 == 0);
}

struct LnFwdArgs {
  const uint16_t *x, *r;
  uint16_t* y;
  long long ldx, ldr, ldy, P;
  int C;
  const float *gamma, *beta;
  float eps;
  float *mean, *invstd;
};

template <bool VEC, int K, int L>
void ln_fwd_launch(const LnFwdArgs& a, const LnPath& p, hipStream_t s) {
  const long long wgs = (a.P + p.RPB - 1) / p.RPB;
  const dim3 grid((unsigned)(wgs < LN_FWD_WGS ? wgs : LN_FWD_WGS));
  hipLaunchKernelGGL((ln_fwd_kernel<VEC, K, L>), grid, dim3(LN_THREADS), 0, s,
                     a.x, a.ldx, a.r, a.ldr, a.y, a.ldy, a.P, a.C, p.CG,
                     a.gamma, a.beta, a.eps, a.mean, a.invstd);
}

struct LnBwdArgs {
  const uint16_t *err, *x, *r;
  uint16_t* dx;
  long long lde, ldx, ldr, lddx, P;
  int C;
  const float *gamma, *mean, *invstd;
  float* ws;
};

// mode 0: dx only; 1: dx + column sums; 2: column sums only
template <bool VEC, int K, int L>
void ln_bwd_launch(const LnBwdArgs& a, const LnPath& p, int mode, int G,
                   hipStream_t s) {
  const long long wgs = (a.P + p.RPB - 1) / p.RPB;
  const dim3 gdx((unsigned)(wgs < LN_FWD_WGS ? wgs : LN_FWD_WGS)), gs(G);
#define HVK_LN_BWD(DX, COLS, GRID)                                           \
  hipLaunchKernelGGL((ln_bwd_kernel<VEC, K, L, DX, COLS>), GRID,             \
                     dim3(LN_THREADS), 0, s, a.err, a.lde, a.x, a.ldx, a.r,  \
                     a.ldr, a.dx, a.lddx, a.P, a.C, p.CG, a.gamma, a.mean,   \
                     a.invstd, a.ws)
  if (mode == 0) HVK_LN_BWD(true, false, gdx);
  else if (mode == 1) HVK_LN_BWD(true, true, gs);
  else HVK_LN_BWD(false, true, gs);
#undef HVK_LN_BWD
}

// the (K, L) instantiations of ln_path, per path
#define HVK_LN_DISPATCH_VEC(FN, ...)                              \
  switch (p.L * 100 + p.K) {                                      \
    case 1601: FN<true, 1, 16>(__VA_ARGS__); break;               \
    case 3201: FN<true, 1, 32>(__VA_ARGS__); break;               \
    case 6401: FN<true, 1, 64>(__VA_ARGS__); break;               \
    case 6402: FN<true, 2, 64>(__VA_ARGS__); break;               \
    case 6404: FN<true, 4, 64>(__VA_ARGS__); break;               \
    case 25602: FN<true, 2, 256>(__VA_ARGS__); break;             \
    default: FN<true, 4, 256>(__VA_ARGS__); break;                \
  }
#define HVK_LN_DISPATCH_ELEM(FN, ...)                             \
  switch (p.L * 100 + p.K) {                                      \
    case 1601: FN<false, 1, 16>(__VA_ARGS__); break;              \
    case 6401: FN<false, 1, 64>(__VA_ARGS__); break;              \
    case 6404: FN<false, 4, 64>(__VA_ARGS__); break;              \
    default: FN<false, 4, 256>(__VA_ARGS__); break;               \
  }

}  // namespace

// Slices per column of the backward's column sums over a [P][C] tensor: a
// function of the shape and of the path (vec: 8 columns per lane) only.
// The workspace of hvk_ln_bwd holds 2 * C * this floats.
HVK_API int hvk_ln_partials(long long P, int C, int vec) {
  if (!ln_shape_ok(P, C) || (vec && C % 8)) return -1;
  return ln_slices(P, ln_path(C, vec != 0));
}

// 1 when a [P][C] tensor at x with row pitch ldx (elements) takes the
// vector path
HVK_API int hvk_ln_vec(const void* x, long long ldx, int C) {
  return C % 8 == 0 && ln_on16(x, ldx) ? 1 : 0;
}

// A/B switch of the backward's column sums: -1 the default rule, 0 a pass
// of their own, 1 inside the dx kernel; returns the old value.  For
// tools/bench_layernorm.py and the tests, see g_ln_colsum.
HVK_API int hvk_ln_colsum(int mode) {
  const int old = g_ln_colsum;
  if (mode >= -1 && mode <= 1) g_ln_colsum = mode;
  return old;
}

// y = gamma (s - mean) invstd + beta over the rows of s = x (+ r, null: no
// residual); bf16 [P][C] with row pitches (elements); gamma, beta float32
// [C]; mean, invstd float32 [P] out.
HVK_API int hvk_ln_fwd(const void* x, long long ldx, const void* r,
                       long long ldr, void* y, long long ldy, long long P,
                       int C, const float* gamma, const float* beta, float eps,
                       float* mean, float* invstd, hipStream_t s) {
  if (!x || !y || !gamma || !beta || !mean || !invstd || !ln_shape_ok(P, C) ||
      ldx < C || ldy < C || (r && ldr < C))
    return -1;
  const bool vec = C % 8 == 0 && ln_on16(x, ldx) && ln_on16(r, ldr) &&
                   ln_on16(y, ldy) && ln_on16(gamma, 8) && ln_on16(beta, 8);
  const LnPath p = ln_path(C, vec);
  const LnFwdArgs a = {(const uint16_t*)x, (const uint16_t*)r, (uint16_t*)y,
                       ldx, ldr, ldy, P, C, gamma, beta, eps, mean, invstd};
  if (p.K == 0) {
    const dim3 grid((unsigned)(P < LN_FWD_WGS ? P : LN_FWD_WGS));
#define HVK_LN_FWD_RR(V, ST)                                                \
  hipLaunchKernelGGL((ln_fwd_rr_kernel<V, ST>), grid, dim3(LN_THREADS), 0, s, \
                     a.x, ldx, a.r, ldr, a.y, ldy, P, C, p.CG, gamma, beta,  \
                     eps, mean, invstd)
    if (vec) HVK_LN_FWD_RR(true, false);
    else if (C <= LN_REG_C) HVK_LN_FWD_RR(false, true);
    else HVK_LN_FWD_RR(false, false);
#undef HVK_LN_FWD_RR
  } else if (vec) {
    HVK_LN_DISPATCH_VEC(ln_fwd_launch, a, p, s)
  } else {
    HVK_LN_DISPATCH_ELEM(ln_fwd_launch, a, p, s)
  }
  return (int)launch_status(s);
}

// Backward of hvk_ln_fwd: dgamma / dbeta written or added to (accumulate);
// dx (need_dx) = invstd (gh - mean_C(gh) - sh mean_C(gh sh)).  vec: the
// caller's path (hvk_ln_vec of every bf16 tensor and of gamma), which fixed
// the size of ws: 2 * C * hvk_ln_partials floats.
HVK_API int hvk_ln_bwd(const void* err, long long lde, const void* x,
                       long long ldx, const void* r, long long ldr, void* dx,
                       long long lddx, long long P, int C, int vec,
                       const float* gamma, const float* mean,
                       const float* invstd, float* dgamma, float* dbeta,
                       int accumulate, int need_dx, float* ws, hipStream_t s) {
  if (!err || !x || !gamma || !mean || !invstd || !dgamma || !dbeta || !ws ||
      !ln_shape_ok(P, C) || lde < C || ldx < C || (r && ldr < C) ||
      (need_dx && (!dx || lddx < C)))
    return -1;
  if (!need_dx) dx = nullptr;
  if (vec && !(C % 8 == 0 && ln_on16(err, lde) && ln_on16(x, ldx) &&
               ln_on16(r, ldr) && ln_on16(dx, lddx) && ln_on16(gamma, 8) &&
               ln_on16(ws, 8)))
    return -1;
  const LnPath p = ln_path(C, vec != 0);
  const int G = ln_slices(P, p);
  const LnBwdArgs a = {(const uint16_t*)err, (const uint16_t*)x,
                       (const uint16_t*)r, (uint16_t*)dx, lde, ldx, ldr, lddx,
                       P, C, gamma, mean, invstd, ws};
  if (p.K == 0) {
    if (vec)
      hipLaunchKernelGGL(ln_bwd_rr_cols_kernel<true>, dim3(G),
                         dim3(LN_THREADS), 0, s, a.err, lde, a.x, ldx, a.r,
                         ldr, P, C, p.CG, mean, invstd, ws);
    else
      hipLaunchKernelGGL(ln_bwd_rr_cols_kernel<false>, dim3(G),
                         dim3(LN_THREADS), 0, s, a.err, lde, a.x, ldx, a.r,
                         ldr, P, C, p.CG, mean, invstd, ws);
    if (dx) {
      const dim3 grid((unsigned)(P < LN_FWD_WGS ? P : LN_FWD_WGS));
#define HVK_LN_DX_RR(V, ST)                                                 \
  hipLaunchKernelGGL((ln_bwd_rr_dx_kernel<V, ST>), grid, dim3(LN_THREADS), 0, \
                     s, a.err, lde, a.x, ldx, a.r, ldr, a.dx, lddx, P, C,    \
                     p.CG, gamma, mean, invstd)
      if (vec) HVK_LN_DX_RR(true, false);
      else if (C <= LN_REG_C) HVK_LN_DX_RR(false, true);
      else HVK_LN_DX_RR(false, false);
#undef HVK_LN_DX_RR
    }
  } else {
    // 1: one kernel for dx and the column sums; else 2 (+ 0 when dx is
    // wanted)
    const bool fused = dx && ln_cols_fused(p, vec != 0);
    const int first = fused ? 1 : 2;
    if (vec) {
      HVK_LN_DISPATCH_VEC(ln_bwd_launch, a, p, first, G, s)
    } else {
      HVK_LN_DISPATCH_ELEM(ln_bwd_launch, a, p, first, G, s)
    }
    if (dx && !fused) {
      if (vec) {
        HVK_LN_DISPATCH_VEC(ln_bwd_launch, a, p, 0, G, s)
      } else {
        HVK_LN_DISPATCH_ELEM(ln_bwd_launch, a, p, 0, G, s)
      }
    }
  }
  hipLaunchKernelGGL(ln_bwd_finish_kernel,
                     dim3((C + LN_FIN_CH - 1) / LN_FIN_CH), dim3(LN_THREADS),
                     0, s, ws, G, C, dgamma, dbeta, accumulate);
  return (int)launch_status(s);
}

// out = bf16(float(a) + float(b)); bf16 [P][C] with row pitches (elements)
HVK_API int hvk_add(const void* a, long long lda, const void* b,
                    long long ldb, void* out, long long ldo, long long P,
                    int C, hipStream_t s) {
  if (!a || !b || !out || !ln_shape_ok(P, C) || lda < C || ldb < C || ldo < C)
    return -1;
  const bool vec = C % 8 == 0 && ln_on16(a, lda) && ln_on16(b, ldb) &&
                   ln_on16(out, ldo);
  long long rows = P, cols = C;
  if (lda == C && ldb == C && ldo == C) {   // one long row
    cols = P * C;
    rows = 1;
    lda = ldb = ldo = cols;
  }
  const long long CG = vec ? cols / 8 : cols;
  const long long gx = (CG + LN_THREADS - 1) / LN_THREADS;
  const dim3 grid((unsigned)(gx < LN_ADD_WGS_X ? gx : LN_ADD_WGS_X),
                  (unsigned)(rows < LN_ADD_WGS_Y ? rows : LN_ADD_WGS_Y));
  if (vec)
    hipLaunchKernelGGL(ln_add_kernel<true>, grid, dim3(LN_THREADS), 0, s,
                       (const uint16_t*)a, lda, (const uint16_t*)b, ldb,
                       (uint16_t*)out, ldo, rows, CG);
  else
    hipLaunchKernelGGL(ln_add_kernel<false>, grid, dim3(LN_THREADS), 0, s,
                       (const uint16_t*)a, lda, (const uint16_t*)b, ldb,
                       (uint16_t*)out, ldo, rows, CG);
  return (int)launch_status(s);
}
