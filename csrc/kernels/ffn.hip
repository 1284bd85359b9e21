// ffn.hip - the two element-wise passes of the position-wise feed-forward
// layer  u = x W1^T + b1,  h = a(u),  y = h W2^T + b2  over [P][F] bf16
// tensors with row pitches (elements); gfx950.  The matrix products are the
// GEMM family's (ops.ffn_fwd / ops.ffn_bwd).
//
//   hvk_ffn_act_fwd   h = a(u); h may be u
//   hvk_ffn_act_bwd   du = bf16(dh a'(u)) (du may be dh), du^T [F][P] when
//                     asked, db1 (+)= sum_P of the ROUNDED du in two launches
//
// a: 0 "gelu" u Phi(u), 1 "gelu_tanh" u s(2 c (u + 0.044715 u^3)) with s the
// logistic function (= 0.5 u (1 + tanh(c (u + 0.044715 u^3)))), 2 "str"
// max(u, 0).  a' is a function of u, not of h: GELU is not monotonic.
//
// Evaluation (float32; budget of a memory-bound pass: about 50 VALU
// lane-instructions per element forward, 100 backward, docs/OPS.md):
//   Phi(u) = u < 0 ? e : 1 - e with e = 0.5 erfc(|u| / sqrt 2) and x = |u| /
//   sqrt 2: x < 1: e = 0.5 - 0.5 x Q(x^2), Q a degree-7 fit of erf(x) / x on
//   [0, 1] (absolute error below 2e-8); x >= 1: e = t exp(R(t) - x^2 - ln 2),
//   t = 1 / (1 + x / 2), R the degree-9 Chebyshev fit of Numerical Recipes'
//   erfcc (relative error below 1.2e-7 of a value below 0.16).  Both are
//   evaluated for every lane and one is selected: no divergent branch.  The
//   backward's phi(u) = exp(-x^2) / sqrt(2 pi) costs one more v_exp.
//   gelu_tanh: s = 1 / (1 + E), E = exp(min(-2z, 80)); 1 - s is taken as
//   E s (no cancellation near s = 1), and the clamp keeps E finite.
// One v_rcp and one (backward: two) v_exp per element, the rest FMAs.
//
// Backward paths:
//   tile    du^T wanted (P % 64 == F % 64 == 0, 16-byte bases and pitches):
//           64 x 64 tiles through padded LDS as transpose_colsum_bf16_kernel
//           (elementwise.hip), 8 B per element.  A slab is RT = 4 (P % 256
//           == 0) or 1 row tiles; its column sums are taken from the LDS tile
//           in that kernel's order, so db1 has the bits of a plain backward
//           followed by hvk_transpose_colsum.
//   row     vector (F % 8 == 0, bases and pitches on the 16-byte grid: NV = 8
//           columns per lane) or guarded element (NV = 1): a workgroup is 8
//           rows x 32 lanes, strides over the rows and keeps its column sums
//           in registers; the 8 rows are added in order through LDS.
// Column sums: no atomics, no workgroup waits for another; slab b writes
// ws[b][F], the finish kernel adds the slabs of a column in index order.
// The slab count is a function of (P, F, path) only (hvk_ffn_act_partials).
#include "hvk_common.h"

using namespace hvk;

namespace {

constexpr int FFN_THREADS = 256;
constexpr int FFN_FWD_WGS_X = 2048, FFN_FWD_WGS_Y = 1024;  // forward grid caps
constexpr int FFN_ROW_SUBS = 8;      // rows of a row-path workgroup pass
constexpr int FFN_ROW_LANES = FFN_THREADS / FFN_ROW_SUBS;   // 32
constexpr int FFN_ROW_MIN = 4;       // rows per lane before a slab opens
constexpr int FFN_ROW_SLABS = 256;   // most slabs (= grid rows) of the row path
constexpr int FFN_TILE_WGS_Y = 512;  // most grid rows of the tile path
constexpr int FFN_FIN_BATCH = 16;    // finish: loads in flight

enum { FFN_GELU = 0, FFN_GELU_TANH = 1, FFN_STR = 2 };

// e = 0.5 erfc(x), x >= 0; x2 = x * x.  r: R(t); q: Q(x2) = erf(x) / x
__device__ __forceinline__ float ffn_half_erfc(float x, float x2) {
  const float t = __builtin_amdgcn_rcpf(__builtin_fmaf(0.5f, x, 1.f));
  float r = 0.17087277f;
  r = __builtin_fmaf(r, t, -0.82215223f);
  r = __builtin_fmaf(r, t, 1.48851587f);
  r = __builtin_fmaf(r, t, -1.13520398f);
  r = __builtin_fmaf(r, t, 0.27886807f);
  r = __builtin_fmaf(r, t, -0.18628806f);
  r = __builtin_fmaf(r, t, 0.09678418f);
  r = __builtin_fmaf(r, t, 0.37409196f);
  r = __builtin_fmaf(r, t, 1.00002368f);
  r = __builtin_fmaf(r, t, -1.26551223f);
  const float big = t * __expf(r - x2 - 0.69314718f);
  float q = -9.673590048e-06f;
  q = __builtin_fmaf(q, x2, 1.126825363e-04f);
  q = __builtin_fmaf(q, x2, -8.484396514e-04f);
  q = __builtin_fmaf(q, x2, 5.221053410e-03f);
  q = __builtin_fmaf(q, x2, -2.686543831e-02f);
  q = __builtin_fmaf(q, x2, 1.128378262e-01f);
  q = __builtin_fmaf(q, x2, -3.761263848e-01f);
  q = __builtin_fmaf(q, x2, 1.128379167e+00f);
  const float small = 0.5f - (0.5f * x) * q;
  return x < 1.f ? small : big;
}

constexpr float FFN_2C = 1.5957691216057308f;               // 2 sqrt(2 / pi)
constexpr float FFN_2CK = 0.044715f * 1.5957691216057308f;

template <int ACT>
__device__ __forceinline__ float ffn_act(float u) {
  if constexpr (ACT == FFN_GELU) {
    const float x = fabsf(u) * 0.70710678118654752f;
    const float e = ffn_half_erfc(x, x * x);
    return u * (u < 0.f ? e : 1.f - e);
  } else if constexpr (ACT == FFN_GELU_TANH) {
    const float z2 = u * __builtin_fmaf(u * u, FFN_2CK, FFN_2C);
    const float E = __expf(fminf(-z2, 80.f));
    return u * __builtin_amdgcn_rcpf(1.f + E);
  } else {
    return u > 0.f ? u : 0.f;
  }
}

// dh * a'(u)
template <int ACT>
__device__ __forceinline__ float ffn_dact(float dh, float u) {
  if constexpr (ACT == FFN_GELU) {
    const float x = fabsf(u) * 0.70710678118654752f;
    const float x2 = x * x;
    const float e = ffn_half_erfc(x, x2);
    const float Phi = u < 0.f ? e : 1.f - e;
    const float phi = __expf(-x2) * 0.3989422804014327f;
    return dh * __builtin_fmaf(u, phi, Phi);
  } else if constexpr (ACT == FFN_GELU_TANH) {
    const float u2 = u * u;
    const float z2 = u * __builtin_fmaf(u2, FFN_2CK, FFN_2C);
    const float E = __expf(fminf(-z2, 80.f));
    const float s = __builtin_amdgcn_rcpf(1.f + E);
    const float w = (E * s) * s;                       // s (1 - s)
    const float dz = __builtin_fmaf(u2, 3.f * FFN_2CK, FFN_2C);
    return dh * __builtin_fmaf(u * dz, w, s);
  } else {
    return u > 0.f ? dh : 0.f;
  }
}

__device__ __forceinline__ void ffn_unpack8(const uint4 p, float* v) {
  const uint32_t w[4] = {p.x, p.y, p.z, p.w};
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    v[2 * q] = __uint_as_float(w[q] << 16);
    v[2 * q + 1] = __uint_as_float(w[q] & 0xffff0000u);
  }
}

// ---------------------------------------------------------------- forward
template <bool VEC, int ACT>
__global__ void __launch_bounds__(FFN_THREADS)
ffn_fwd_kernel(const uint16_t* u, long long ldu, uint16_t* h, long long ldh,
               long long P, long long CG) {   // h may be u: no __restrict__
  constexpr int NV = VEC ? 8 : 1;
  const long long stepx = (long long)gridDim.x * FFN_THREADS;
  for (long long row = blockIdx.y; row < P; row += gridDim.y) {
    for (long long cg = (long long)blockIdx.x * FFN_THREADS + threadIdx.x;
         cg < CG; cg += stepx) {
      const long long c0 = cg * NV;
      if constexpr (VEC) {
        float v[8];
        ffn_unpack8(*(const uint4*)(u + row * ldu + c0), v);
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = ffn_act<ACT>(v[j]);
        *(uint4*)(h + row * ldh + c0) = pack_bf16x8(v);
      } else {
        h[row * ldh + c0] = f2bf(ffn_act<ACT>(bf2f(u[row * ldu + c0])));
      }
    }
  }
}

// --------------------------------------------------------------- backward
// Row path.  Workgroup (bx, by): column groups bx * 32 .. + 31, rows by * 8 +
// sub, + 8 gridDim.y, ...; ws[by][F] gets its column sums of the rounded du.
template <bool VEC, int ACT>
__global__ void __launch_bounds__(FFN_THREADS)
ffn_bwd_row_kernel(const uint16_t* dh, long long lddh,
                   const uint16_t* __restrict__ u, long long ldu,
                   uint16_t* du, long long lddu, long long P, int F, int CG,
                   float* __restrict__ ws) {   // du may be dh
  constexpr int NV = VEC ? 8 : 1;
  __shared__ float comb[FFN_ROW_SUBS - 1][NV][FFN_ROW_LANES];
  const int sub = threadIdx.x / FFN_ROW_LANES;
  const int lane = threadIdx.x % FFN_ROW_LANES;
  const long long cg = (long long)blockIdx.x * FFN_ROW_LANES + lane;
  const bool on = cg < CG;
  const long long c0 = cg * NV;
  float acc[NV];
#pragma unroll
  for (int j = 0; j < NV; ++j) acc[j] = 0.f;
  if (on) {
    const long long step = (long long)gridDim.y * FFN_ROW_SUBS;
    for (long long row = (long long)blockIdx.y * FFN_ROW_SUBS + sub; row < P;
         row += step) {
      if constexpr (VEC) {
        float g[8], v[8];
        ffn_unpack8(*(const uint4*)(dh + row * lddh + c0), g);
        ffn_unpack8(*(const uint4*)(u + row * ldu + c0), v);
#pragma unroll
        for (int j = 0; j < 8; ++j) g[j] = ffn_dact<ACT>(g[j], v[j]);
        const uint4 p = pack_bf16x8(g);
        *(uint4*)(du + row * lddu + c0) = p;
        ffn_unpack8(p, g);
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[j] += g[j];
      } else {
        const uint16_t p = f2bf(ffn_dact<ACT>(bf2f(dh[row * lddh + c0]),
                                              bf2f(u[row * ldu + c0])));
        du[row * lddu + c0] = p;
        acc[0] += bf2f(p);
      }
    }
  }
  if (sub > 0) {
#pragma unroll
    for (int j = 0; j < NV; ++j) comb[sub - 1][j][lane] = acc[j];
  }
  __syncthreads();
  if (sub == 0 && on) {
    for (int t = 0; t < FFN_ROW_SUBS - 1; ++t) {
#pragma unroll
      for (int j = 0; j < NV; ++j) acc[j] += comb[t][j][lane];
    }
    float* w = ws + (long long)blockIdx.y * F + c0;
    if constexpr (VEC) {
      ((float4*)w)[0] = make_float4(acc[0], acc[1], acc[2], acc[3]);
      ((float4*)w)[1] = make_float4(acc[4], acc[5], acc[6], acc[7]);
    } else {
      *w = acc[0];
    }
  }
}

// Tile path.  Workgroup (bx, by): columns bx * 64 .. + 63, slabs by, by +
// gridDim.y, ...; slab s is the row tiles s * RT .. + RT - 1 and writes
// ws[s][F].  A lane computes 16 adjacent columns of a row, stores them to du
// and to the LDS tile, then reads 16 rows of one column back: a 32-byte run
// of a du^T row, summed in transpose_colsum_bf16_kernel's order.
template <int ACT, int RT>
__global__ void __launch_bounds__(FFN_THREADS)
ffn_bwd_tile_kernel(const uint16_t* dh, long long lddh,
                    const uint16_t* __restrict__ u, long long ldu,
                    uint16_t* du, long long lddu,
                    uint16_t* __restrict__ dut, long long lddut, int slabs,
                    int F, float* __restrict__ ws) {   // du may be dh
  __shared__ uint16_t tile[64][64 + 8];
  const int c0 = blockIdx.x * 64, t = threadIdx.x;
  const int col = t >> 2, rr = (t & 3) * 16;
  bool first = true;
  for (int sl = blockIdx.y; sl < slabs; sl += gridDim.y) {
    float sum = 0.f;
    for (int rt = 0; rt < RT; ++rt) {
      const long long r0 = ((long long)sl * RT + rt) * 64;
      const long long row = r0 + (t >> 2);
      const uint4* pg = (const uint4*)(dh + row * lddh + c0 + rr);
      const uint4* pu = (const uint4*)(u + row * ldu + c0 + rr);
      const uint4 g0 = pg[0], g1 = pg[1], u0 = pu[0], u1 = pu[1];
      float g[16], v[16];
      ffn_unpack8(g0, g);
      ffn_unpack8(g1, g + 8);
      ffn_unpack8(u0, v);
      ffn_unpack8(u1, v + 8);
#pragma unroll
      for (int j = 0; j < 16; ++j) g[j] = ffn_dact<ACT>(g[j], v[j]);
      const uint4 a = pack_bf16x8(g), b = pack_bf16x8(g + 8);
      uint4* pd = (uint4*)(du + row * lddu + c0 + rr);
      pd[0] = a;
      pd[1] = b;
      if (!first) __syncthreads();   // the last tile's reads
      first = false;
      *(uint4*)&tile[t >> 2][rr] = a;
      *(uint4*)&tile[t >> 2][rr + 8] = b;
      __syncthreads();
      uint32_t w[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const uint16_t lo = tile[rr + 2 * j][col];
        const uint16_t hi = tile[rr + 2 * j + 1][col];
        sum += bf2f(lo);
        sum += bf2f(hi);
        w[j] = (uint32_t)lo | ((uint32_t)hi << 16);
      }
      uint4* dst = (uint4*)(dut + (long long)(c0 + col) * lddut + r0 + rr);
      dst[0] = make_uint4(w[0], w[1], w[2], w[3]);
      dst[1] = make_uint4(w[4], w[5], w[6], w[7]);
    }
    // over the four lanes of the column (a fixed order)
    sum += __shfl_xor(sum, 1);
    sum += __shfl_xor(sum, 2);
    if ((t & 3) == 0) ws[(long long)sl * F + c0 + col] = sum;
  }
}

// db1[c] (+)= the slabs of ws[G][F] in index order.  FFN_FIN_BATCH loads are
// issued before their sums are taken: the pass is bound by a load's latency.
__global__ void __launch_bounds__(FFN_THREADS)
ffn_finish_kernel(const float* __restrict__ ws, int G, int F, float* db1,
                  int accumulate) {
  const int c = blockIdx.x * FFN_THREADS + threadIdx.x;
  if (c >= F) return;
  float sum = 0.f;
  for (int g0 = 0; g0 < G; g0 += FFN_FIN_BATCH) {
    float v[FFN_FIN_BATCH];
#pragma unroll
    for (int i = 0; i < FFN_FIN_BATCH; ++i)
      v[i] = g0 + i < G ? ws[(long long)(g0 + i) * F + c] : 0.f;
#pragma unroll
    for (int i = 0; i < FFN_FIN_BATCH; ++i)
      if (g0 + i < G) sum += v[i];
  }
  db1[c] = accumulate ? db1[c] + sum : sum;
}

inline bool ffn_shape_ok(long long P, int F) {
  return P >= 1 && F >= 1 && P <= ((1ll << 31) - 1) / F;
}
// a [P][F] tensor with pitch ld stays below 2^31 elements from its base
inline bool ffn_pitch_ok(long long P, int F, long long ld) {
  return ld >= F && (P - 1) * ld + F < (1ll << 31);
}
inline bool ffn_on16(const void* p, long long ld) {
  return p == nullptr || ((((uintptr_t)p) & 15) == 0 && ld % 8 == 0);
}
inline int ffn_tile_rt(long long P) { return P % 256 == 0 ? 4 : 1; }
inline int ffn_row_slabs(long long P) {
  const long long per = (long long)FFN_ROW_SUBS * FFN_ROW_MIN;
  const long long s = (P + per - 1) / per;
  return (int)(s < FFN_ROW_SLABS ? s : FFN_ROW_SLABS);
}

}  // namespace

// Slabs per column of hvk_ffn_act_bwd's column sums over [P][F]: a function
// of the shape and of whether du^T is written (the tile path) only.  ws
// holds F * this floats.  -1: no such grid (transposed needs P % 64 == F %
// 64 == 0).
HVK_API int hvk_ffn_act_partials(long long P, int F, int transposed) {
  if (!ffn_shape_ok(P, F)) return -1;
  if (!transposed) return ffn_row_slabs(P);
  if (P % 64 || F % 64) return -1;
  return (int)(P / (64 * ffn_tile_rt(P)));
}

// h = a(u) over bf16 [P][F] with row pitches (elements); h may be u.
HVK_API int hvk_ffn_act_fwd(const void* u, long long ldu, void* h,
                            long long ldh, long long P, int F, int act,
                            hipStream_t s) {
  if (!u || !h || !ffn_shape_ok(P, F) || !ffn_pitch_ok(P, F, ldu) ||
      !ffn_pitch_ok(P, F, ldh) || act < 0 || act > 2)
    return -1;
  const bool vec = F % 8 == 0 && ffn_on16(u, ldu) && ffn_on16(h, ldh);
  long long rows = P, cols = F;
  if (ldu == F && ldh == F) {   // one long row
    cols = P * F;
    rows = 1;
    ldu = ldh = cols;
  }
  const long long CG = vec ? cols / 8 : cols;
  const long long gx = (CG + FFN_THREADS - 1) / FFN_THREADS;
  const dim3 grid((unsigned)(gx < FFN_FWD_WGS_X ? gx : FFN_FWD_WGS_X),
                  (unsigned)(rows < FFN_FWD_WGS_Y ? rows : FFN_FWD_WGS_Y));
#define HVK_FFN_FWD(V, A)                                                    \
  hipLaunchKernelGGL((ffn_fwd_kernel<V, A>), grid, dim3(FFN_THREADS), 0, s,  \
                     (const uint16_t*)u, ldu, (uint16_t*)h, ldh, rows, CG)
  if (vec) {
    if (act == FFN_GELU) HVK_FFN_FWD(true, FFN_GELU);
    else if (act == FFN_GELU_TANH) HVK_FFN_FWD(true, FFN_GELU_TANH);
    else HVK_FFN_FWD(true, FFN_STR);
  } else {
    if (act == FFN_GELU) HVK_FFN_FWD(false, FFN_GELU);
    else if (act == FFN_GELU_TANH) HVK_FFN_FWD(false, FFN_GELU_TANH);
    else HVK_FFN_FWD(false, FFN_STR);
  }
#undef HVK_FFN_FWD
  return (int)launch_status(s);
}

// du = bf16(dh a'(u)) over bf16 [P][F] with row pitches (du may be dh);
// dut (null: not wanted) = du^T [F][P] with pitch lddut; ws: F *
// hvk_ffn_act_partials(P, F, dut != null) floats; db1 (null: the slabs stay
// in ws) float32 [F], written or added to (accumulate) from the rounded du.
HVK_API int hvk_ffn_act_bwd(const void* dh, long long lddh, const void* u,
                            long long ldu, void* du, long long lddu, void* dut,
                            long long lddut, long long P, int F, int act,
                            float* db1, int accumulate, float* ws,
                            hipStream_t s) {
  if (!dh || !u || !du || !ws || !ffn_shape_ok(P, F) ||
      !ffn_pitch_ok(P, F, lddh) || !ffn_pitch_ok(P, F, ldu) ||
      !ffn_pitch_ok(P, F, lddu) || act < 0 || act > 2)
    return -1;
  const bool vec = F % 8 == 0 && ffn_on16(dh, lddh) && ffn_on16(u, ldu) &&
                   ffn_on16(du, lddu) && ffn_on16(ws, 8);
  int G;
  if (dut) {
    if (P % 64 || F % 64 || !vec || !ffn_on16(dut, lddut) || lddut < P ||
        (F - 1) * lddut + P >= (1ll << 31))
      return -1;
    const int rt = ffn_tile_rt(P);
    G = (int)(P / (64 * rt));
    const dim3 grid(F / 64, G < FFN_TILE_WGS_Y ? G : FFN_TILE_WGS_Y);
#define HVK_FFN_TILE(A, RT)                                                  \
  hipLaunchKernelGGL((ffn_bwd_tile_kernel<A, RT>), grid, dim3(FFN_THREADS),  \
                     0, s, (const uint16_t*)dh, lddh, (const uint16_t*)u,    \
                     ldu, (uint16_t*)du, lddu, (uint16_t*)dut, lddut, G, F,  \
                     ws)
#define HVK_FFN_TILE_A(A)                    \
  if (rt == 4) HVK_FFN_TILE(A, 4);           \
  else HVK_FFN_TILE(A, 1)
    if (act == FFN_GELU) { HVK_FFN_TILE_A(FFN_GELU); }
    else if (act == FFN_GELU_TANH) { HVK_FFN_TILE_A(FFN_GELU_TANH); }
    else { HVK_FFN_TILE_A(FFN_STR); }
#undef HVK_FFN_TILE_A
#undef HVK_FFN_TILE
  } else {
    G = ffn_row_slabs(P);
    const int CG = vec ? F / 8 : F;
    const dim3 grid((CG + FFN_ROW_LANES - 1) / FFN_ROW_LANES, G);
#define HVK_FFN_ROW(V, A)                                                    \
  hipLaunchKernelGGL((ffn_bwd_row_kernel<V, A>), grid, dim3(FFN_THREADS), 0, \
                     s, (const uint16_t*)dh, lddh, (const uint16_t*)u, ldu,  \
                     (uint16_t*)du, lddu, P, F, CG, ws)
    if (vec) {
      if (act == FFN_GELU) HVK_FFN_ROW(true, FFN_GELU);
      else if (act == FFN_GELU_TANH) HVK_FFN_ROW(true, FFN_GELU_TANH);
      else HVK_FFN_ROW(true, FFN_STR);
    } else {
      if (act == FFN_GELU) HVK_FFN_ROW(false, FFN_GELU);
      else if (act == FFN_GELU_TANH) HVK_FFN_ROW(false, FFN_GELU_TANH);
      else HVK_FFN_ROW(false, FFN_STR);
    }
#undef HVK_FFN_ROW
  }
  if (db1)
    hipLaunchKernelGGL(ffn_finish_kernel,
                       dim3((F + FFN_THREADS - 1) / FFN_THREADS),
                       dim3(FFN_THREADS), 0, s, (const float*)ws, G, F, db1,
                       accumulate);
  return (int)launch_status(s);
}
