// rbm.hip - restricted Boltzmann machine kernels on the bf16 MFMA
// (v_mfma_f32_16x16x32_bf16, f32 accumulation; docs/OPS.md "Restricted
// Boltzmann machines"):
//   hvk_rbm_sample  one half of a Gibbs step: P = sigmoid(x . w^T + bias)
//                   (or x . w, from the SAME weights) and the Bernoulli draw
//                   S = (u < P) in the epilogue; the pre-activations are
//                   never written;
//   hvk_rbm_grad    the CD statistic h0^T.v0 - hk^T.vk and both bias sums as
//                   ONE product over K = 2n batch rows, written over the
//                   trainer's flat gradient buffer [W | hbias | vbias].
// No kernel waits for another workgroup, nothing is atomic.
//
// hvk_rbm_sample has the tile of recurrent.hip: a workgroup owns 16 units x
// 32 batch rows, the weights are the A operand (unit on the accumulator ROW),
// the activations the B operand (batch row on the COLUMN = lane & 15), so a
// lane holds 4 consecutive units of one batch row: one float4 of bias, four
// consecutive counters, one 8-B store per output.  The 4 waves split K (wave
// w takes the 32-wide chunks w, w + 4, ...) and their partial sums meet in
// LDS, added in wave order.  x is K-major in both directions and feeds the
// MFMA straight from 16-B global loads.  w [H][V] is K-major for x . w^T
// (direct loads too) and MN-major for x . w: there each wave stages its
// [32 k][16 units] chunk in LDS as it lies in memory and reads the fragment
// with the transposed read.
//
// The transposed read needs EXEC all ones: no lane is masked and nothing
// returns before the last one; partial tiles are padded with zeros.  Global
// loads are unconditional from clamped addresses and zeroed afterwards.
#include "hvk_api.h"
#include "hvk_common.h"

using namespace hvk;

namespace {

typedef __attribute__((address_space(3))) s16x4 lds_s16x4;

constexpr int NTHR = 256;
constexpr int NW = NTHR / WAVE;   // waves = K splits of a sampling workgroup
constexpr int TU = 16;            // units per sampling tile
constexpr int BSUB = 2;           // 16-row batch sub-tiles per sampling tile
constexpr int TB = 16 * BSUB;     // batch rows per sampling tile
constexpr int BK = 32;            // K of one MFMA

// the counter hash of elementwise.hip (dropout, stochastic pooling)
__device__ __forceinline__ uint32_t hash32(uint32_t x, uint32_t seed) {
  x ^= seed * 0x9E3779B9u;
  x ^= x >> 16; x *= 0x7feb352du;
  x ^= x >> 15; x *= 0x846ca68bu;
  x ^= x >> 16;
  return x;
}

// plain logistic function; +-inf arguments of the division give exactly 0 / 1
__device__ __forceinline__ float sigm(float x) {
  return 1.f / (1.f + __expf(-x));
}

// The 8 bf16 [row][c .. c + 7] of a row-major operand, 0 outside rows x cols.
// Unconditional loads (an outside element reads the operand's first element
// and is replaced by 0 after).  VEC: base and pitch on the 16-B grid and
// cols % 8 == 0, so a chunk is inside or outside as a whole.
template <bool VEC>
__device__ __forceinline__ uint4 ldchunk(const uint16_t* __restrict__ p,
                                         long long ld, int row, int rows,
                                         int c, int cols) {
  uint4 v;
  if constexpr (VEC) {
    const bool in = row < rows && c < cols;
    v = *(const uint4*)(in ? p + row * ld + c : p);
    if (!in) v = make_uint4(0, 0, 0, 0);
  } else {
    uint32_t e[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const bool in = row < rows && c + j < cols;
      const uint16_t x = *(in ? p + row * ld + c + j : p);
      e[j] = in ? x : 0u;
    }
    v = make_uint4(e[0] | e[1] << 16, e[2] | e[3] << 16, e[4] | e[5] << 16,
                   e[6] | e[7] << 16);
  }
  return v;
}

// two transposed 8-B reads (k rows q .. q + 3 and + 4 of this lane's column)
// -> one 16x16x32 operand fragment
__device__ __forceinline__ bf16x8 tr_read(const uint16_t* p0,
                                          const uint16_t* p1) {
  s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)p0);
  s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)p1);
  typedef __attribute__((ext_vector_type(8))) short s16x8;
  s16x8 v = __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
  return __builtin_bit_cast(bf16x8, v);
}

// ---------------------------------------------------------------- sampling
struct SampleArgs {
  const uint16_t* x;      // [rows][K] bf16
  const uint16_t* w;      // [H][V] bf16: [U][K] (TR = false) or [K][U]
  const float* bias;      // [U]
  uint16_t* probs;        // [rows][U] bf16 or nullptr
  uint16_t* sample;       // [rows][U] bf16 or nullptr
  const uint32_t* seed_dev;
  long long ldx, ldw, ldp, lds;
  uint32_t seed, base;
  int n, K, U;
};

// LDS image of a wave's [32 k][16 units] chunk: k row r at row slot
// r ^ ((r >> 3 & 1) << 2), so the 8 rows one transposed read of a 32-lane
// half touches (r .. r + 3 and r + 8 .. r + 11) cover the 64 banks once
__device__ __forceinline__ int wslot(int r) { return r ^ (((r >> 3) & 1) << 2); }

template <bool TR, bool VEC>
__global__ void __launch_bounds__(NTHR) rbm_sample_kernel(const SampleArgs a) {
  __shared__ __attribute__((aligned(16))) float4 red[NW * BSUB * WAVE];
  __shared__ __attribute__((aligned(16))) uint16_t wt[TR ? NW * 2 * BK * TU : 8];
  const int u0 = blockIdx.x * TU, b0 = blockIdx.y * TB;
  const int t = threadIdx.x, lane = t & 63, wid = t >> 6;
  const int fr = lane & 15, fq = lane >> 4;
  const int n = a.n, K = a.K, U = a.U;
  const int nkc = (K + BK - 1) / BK;
  // the same trip count in every wave: the waves meet at the barriers
  const int nit = (nkc + NW - 1) / NW;

  f32x4 acc[BSUB];
#pragma unroll
  for (int s = 0; s < BSUB; ++s) acc[s] = f32x4{0, 0, 0, 0};

  uint4 wr, xr[BSUB];
  auto load = [&](int kc) {   // past K: zeros
    const int k = kc * BK + fq * 8;
    if constexpr (TR)
      wr = ldchunk<VEC>(a.w, a.ldw, kc * BK + (lane >> 1), K,
                        u0 + (lane & 1) * 8, U);
    else
      wr = ldchunk<VEC>(a.w, a.ldw, u0 + fr, U, k, K);
#pragma unroll
    for (int s = 0; s < BSUB; ++s)
      xr[s] = ldchunk<VEC>(a.x, a.ldx, b0 + 16 * s + fr, n, k, K);
  };
  load(wid);
  for (int it = 0; it < nit; ++it) {
    const uint4 wc = wr;
    uint4 xc[BSUB];
#pragma unroll
    for (int s = 0; s < BSUB; ++s) xc[s] = xr[s];
    load((it + 1) * NW + wid);
    bf16x8 wf;
    if constexpr (TR) {
      uint16_t* img = wt + (wid * 2 + (it & 1)) * (BK * TU);
      *(uint4*)(img + wslot(lane >> 1) * TU + (lane & 1) * 8) = wc;
      __syncthreads();
      const int r = fq * 8 + (fr >> 2);
      wf = tr_read(img + wslot(r) * TU + (fr & 3) * 4,
                   img + wslot(r + 4) * TU + (fr & 3) * 4);
    } else {
      wf = __builtin_bit_cast(bf16x8, wc);
    }
#pragma unroll
    for (int s = 0; s < BSUB; ++s)
      acc[s] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
          wf, __builtin_bit_cast(bf16x8, xc[s]), acc[s], 0, 0, 0);
  }

  // the waves' partial sums through LDS, added in wave order
#pragma unroll
  for (int s = 0; s < BSUB; ++s)
    red[(wid * BSUB + s) * WAVE + lane] =
        make_float4(acc[s][0], acc[s][1], acc[s][2], acc[s][3]);
  __syncthreads();
  if (wid >= BSUB) return;
  float4 sum = red[wid * WAVE + lane];
#pragma unroll
  for (int w = 1; w < NW; ++w) {
    const float4 o = red[(w * BSUB + wid) * WAVE + lane];
    sum.x += o.x; sum.y += o.y; sum.z += o.z; sum.w += o.w;
  }

  const int b = b0 + 16 * wid + fr;
  const int u = u0 + 4 * fq;
  if (b >= n || u >= U) return;
  const int nu = min(4, U - u);   // VEC: U % 8 == 0, so 4
  float bs[4];
  if constexpr (VEC) {
    const float4 f = *(const float4*)(a.bias + u);
    bs[0] = f.x; bs[1] = f.y; bs[2] = f.z; bs[3] = f.w;
  } else {
#pragma unroll
    for (int r = 0; r < 4; ++r) bs[r] = r < nu ? a.bias[u + r] : 0.f;
  }
  const uint32_t seed = a.seed_dev ? a.seed_dev[0] : a.seed;
  const uint32_t cnt = a.base + (uint32_t)b * (uint32_t)U + (uint32_t)u;
  const float pre[4] = {sum.x + bs[0], sum.y + bs[1], sum.z + bs[2],
                        sum.w + bs[3]};
  float p[4], sm[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    p[r] = sigm(pre[r]);
    const float uf = (float)(hash32(cnt + r, seed) >> 8) * 0x1p-24f;
    sm[r] = uf < p[r] ? 1.f : 0.f;
  }
  if constexpr (VEC) {
    if (a.probs)
      *(uint2*)(a.probs + b * a.ldp + u) =
          make_uint2(pack_bf16x2(p[0], p[1]), pack_bf16x2(p[2], p[3]));
    if (a.sample)
      *(uint2*)(a.sample + b * a.lds + u) =
          make_uint2(pack_bf16x2(sm[0], sm[1]), pack_bf16x2(sm[2], sm[3]));
  } else {
#pragma unroll
    for (int r = 0; r < 4; ++r)
      if (r < nu) {
        if (a.probs) a.probs[b * a.ldp + u + r] = f2bf(p[r]);
        if (a.sample) a.sample[b * a.lds + u + r] = f2bf(sm[r]);
      }
  }
}

// ---------------------------------------------------------------- gradient
// acc[h][v] = sum over K = 2n of A[k][h] B[k][v]: k < n from (h0, v0), then
// from (hk, vk) with the sign bits of the A fragments flipped (exact).  Both
// operands are MN-major [k][.]: a K tile of 32 batch rows is staged as it
// lies, [32 k][64] bf16 per operand, and read with the transposed read.
// Tile 64 x 64, 4 waves of 32 x 32.  The bias sums are MFMAs against a ones
// operand in the tiles of the first tile column (hbias) / row (vbias).
constexpr int GT = 64;                 // h and v per tile
constexpr int GIMG = BK * GT;          // bf16 of one staged operand tile
constexpr int G_TARGET_WGS = 512;

struct GradArgs {
  const uint16_t *h0, *v0, *hk, *vk;   // [rows][H] / [rows][V] bf16
  long long ld_h0, ld_v0, ld_hk, ld_vk;
  float* out;        // splits == 1: the gradient; else the slice workspace
  long long off_hb, off_vb, total;
  float scale;
  int n, V, H, nk, kps, tiles_v;
};

// 16-column block b of k row r sits at block b ^ gsw(r): the 8 rows of one
// transposed read of a 32-lane half (r .. r + 3, r + 8 .. r + 11; a row is
// 128 B, so parity picks the bank half) then cover the 64 banks once
__device__ __forceinline__ int gsw(int r) {
  return ((r >> 1) & 1) | (((r >> 3) & 1) << 1);
}

__device__ __forceinline__ bf16x8 gfrag(const uint16_t* s, int b, int fr,
                                        int fq) {
  const int r = fq * 8 + (fr >> 2);
  return tr_read(s + r * GT + ((b ^ gsw(r)) << 4) + (fr & 3) * 4,
                 s + (r + 4) * GT + ((b ^ gsw(r + 4)) << 4) + (fr & 3) * 4);
}

template <bool VEC, bool DIRECT>
__global__ void __launch_bounds__(NTHR) rbm_grad_kernel(const GradArgs a) {
  __shared__ __attribute__((aligned(16))) uint16_t sm[2 * 2 * GIMG];
  const int th = blockIdx.x / a.tiles_v, tv = blockIdx.x - th * a.tiles_v;
  const int split = blockIdx.y;
  const int h0t = th * GT, v0t = tv * GT;
  const int t = threadIdx.x, lane = t & 63, wid = t >> 6;
  const int wm = wid >> 1, wn = wid & 1;
  const int fr = lane & 15, fq = lane >> 4;
  const int n = a.n, V = a.V, H = a.H, nk = a.nk;
  const int kt0 = split * a.kps, kt1 = min(2 * nk, kt0 + a.kps);
  const int kr = t >> 3, kc = t & 7;
  const int soff = kr * GT + (((kc >> 1) ^ gsw(kr)) << 4) + (kc & 1) * 8;

  f32x4 acc[2][2], ahb[2], avb[2];
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    ahb[i] = avb[i] = f32x4{0, 0, 0, 0};
#pragma unroll
    for (int j = 0; j < 2; ++j) acc[i][j] = f32x4{0, 0, 0, 0};
  }
  const bool do_hb = tv == 0 && wn == 0, do_vb = th == 0 && wm == 0;

  uint4 ra, rb;
  auto load = [&](int kt) {   // past the last K tile: zeros
    const bool neg = kt >= nk;
    const int r = (neg ? kt - nk : kt) * BK + kr;
    ra = ldchunk<VEC>(neg ? a.hk : a.h0, neg ? a.ld_hk : a.ld_h0, r,
                      kt < 2 * nk ? n : 0, h0t + kc * 8, H);
    rb = ldchunk<VEC>(neg ? a.vk : a.v0, neg ? a.ld_vk : a.ld_v0, r,
                      kt < 2 * nk ? n : 0, v0t + kc * 8, V);
  };
  load(kt0);
  *(uint4*)(sm + soff) = ra;
  *(uint4*)(sm + GIMG + soff) = rb;
  __syncthreads();
  int cur = 0;
  for (int kt = kt0; kt < kt1; ++kt) {
    load(kt + 1);
    __builtin_amdgcn_sched_barrier(0);
    const uint16_t* sA = sm + cur * 2 * GIMG;
    const uint16_t* sB = sA + GIMG;
    const uint32_t flip = kt >= nk ? 0x80008000u : 0u;
    bf16x8 af[2], bf[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      uint4 q = __builtin_bit_cast(uint4, gfrag(sA, wm * 2 + i, fr, fq));
      q.x ^= flip; q.y ^= flip; q.z ^= flip; q.w ^= flip;
      af[i] = __builtin_bit_cast(bf16x8, q);
      bf[i] = gfrag(sB, wn * 2 + i, fr, fq);
    }
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j)
        acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[i], bf[j],
                                                            acc[i][j], 0, 0, 0);
    if (do_hb || do_vb) {   // wave-uniform
      const uint32_t o = 0x3f803f80u, m = o ^ flip;
      const bf16x8 ones = __builtin_bit_cast(bf16x8, make_uint4(o, o, o, o));
      const bf16x8 sgn = __builtin_bit_cast(bf16x8, make_uint4(m, m, m, m));
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        if (do_hb)
          ahb[i] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[i], ones, ahb[i],
                                                           0, 0, 0);
        if (do_vb)
          avb[i] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(sgn, bf[i], avb[i],
                                                           0, 0, 0);
      }
    }
    __builtin_amdgcn_sched_barrier(0);
    // also after the last tile (zeros, into the buffer nobody reads)
    *(uint4*)(sm + (cur ^ 1) * 2 * GIMG + soff) = ra;
    *(uint4*)(sm + (cur ^ 1) * 2 * GIMG + GIMG + soff) = rb;
    __syncthreads();
    cur ^= 1;
  }

  float* out = a.out + (DIRECT ? 0 : (long long)split * a.total);
  const float sc = DIRECT ? a.scale : 1.f;
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int h = h0t + wm * 32 + i * 16 + 4 * fq + r;
      if (h >= H) continue;
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const int v = v0t + wn * 32 + j * 16 + fr;
        if (v < V) out[(long long)h * V + v] = sc * acc[i][j][r];
      }
      // every column of ahb holds the row sum
      if (do_hb && fr == 0) out[a.off_hb + h] = sc * ahb[i][r];
    }
  if (do_vb && fq == 0) {   // every row of avb holds the column sum
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int v = v0t + wn * 32 + j * 16 + fr;
      if (v < V) out[a.off_vb + v] = sc * avb[j][0];
    }
  }
  if constexpr (DIRECT) {
    // the padding between the segments, once
    if (blockIdx.x == 0 && t < 48) {
      const long long hv = (long long)H * V;
      const long long e = t < 16 ? hv + t
                        : t < 32 ? a.off_hb + H + (t - 16)
                                 : a.off_vb + V + (t - 32);
      const long long end = t < 16 ? a.off_hb : t < 32 ? a.off_vb : a.total;
      if (e < end) out[e] = 0.f;
    }
  }
}

// grad[e] = scale * (slice 0 + slice 1 + ...) in split order; 0 in the
// padding between the segments
__global__ void __launch_bounds__(NTHR)
rbm_grad_finish(float* grad, const float* __restrict__ ws, long long hv,
                long long off_hb, int H, long long off_vb, int V,
                long long total, int splits, float scale) {
  const long long e = (long long)blockIdx.x * NTHR + threadIdx.x;
  if (e >= total) return;
  const bool in = e < hv || (e >= off_hb && e < off_hb + H) ||
                  (e >= off_vb && e < off_vb + V);
  float s = 0.f;
  if (in) {
    s = ws[e];
    for (int i = 1; i < splits; ++i) s += ws[i * total + e];
    s *= scale;
  }
  grad[e] = s;
}

inline bool on_grid(const void* p, long long ld) {
  return ((uintptr_t)p & 15) == 0 && ld % 8 == 0;
}
inline long long r16(long long n) { return (n + 15) / 16 * 16; }

}  // namespace

// probs / sample [n][U] = sigmoid(x . w^T + bias) (transposed = 0: x [n][V],
// U = H) or sigmoid(x . w + bias) (transposed = 1: x [n][H], U = V) from the
// same w [H][V], and sample = (u < probs) with u = (hash32(base + b U + j,
// seed) >> 8) 2^-24 for element (b, j), in f32 before the bf16 rounding.
// Either output may be nullptr.  seed_dev (uint32 [1]) replaces seed when
// given.  Every operand has its own row pitch in elements.
HVK_API int hvk_rbm_sample(int transposed, int n, int V, int H, const void* x,
                           long long ldx, const void* w, long long ldw,
                           const float* bias, void* probs, long long ldp,
                           void* sample, long long lds, unsigned seed,
                           const void* seed_dev, long long base,
                           hipStream_t s) {
  if (n < 1 || V < 1 || H < 1 || !x || !w || !bias || (!probs && !sample) ||
      (transposed != 0 && transposed != 1))
    return -1;
  const int K = transposed ? H : V, U = transposed ? V : H;
  if (ldx < K || ldw < V || (probs && ldp < U) || (sample && lds < U))
    return -1;
  SampleArgs a;
  a.x = (const uint16_t*)x;
  a.w = (const uint16_t*)w;
  a.bias = bias;
  a.probs = (uint16_t*)probs;
  a.sample = (uint16_t*)sample;
  a.seed_dev = (const uint32_t*)seed_dev;
  a.ldx = ldx; a.ldw = ldw; a.ldp = ldp; a.lds = lds;
  a.seed = seed;
  a.base = (uint32_t)(unsigned long long)base;
  a.n = n; a.K = K; a.U = U;
  const bool vec = K % 8 == 0 && U % 8 == 0 && on_grid(x, ldx) &&
                   on_grid(w, ldw) && ((uintptr_t)bias & 15) == 0 &&
                   (!probs || on_grid(probs, ldp)) &&
                   (!sample || on_grid(sample, lds));
  const dim3 grid((unsigned)((U + TU - 1) / TU), (unsigned)((n + TB - 1) / TB));
  if (grid.y > 65535u) return -1;
#define HVK_RBM_SAMPLE(TR, VEC) \
  hipLaunchKernelGGL((rbm_sample_kernel<TR, VEC>), grid, dim3(NTHR), 0, s, a)
  if (transposed) {
    if (vec) HVK_RBM_SAMPLE(true, true);
    else HVK_RBM_SAMPLE(true, false);
  } else {
    if (vec) HVK_RBM_SAMPLE(false, true);
    else HVK_RBM_SAMPLE(false, false);
  }
#undef HVK_RBM_SAMPLE
  return (int)launch_status(s);
}

// Number of batch slices hvk_rbm_grad uses for (n, V, H) and a requested
// count (0: chosen): the workspace holds that many slices of the flat buffer.
HVK_API int hvk_rbm_grad_splits(int n, int V, int H, int splits) {
  if (n < 1 || V < 1 || H < 1 || splits < 0) return -1;
  const long long tiles =
      (long long)((H + GT - 1) / GT) * ((V + GT - 1) / GT);
  const int nk2 = 2 * ((n + BK - 1) / BK);
  long long sp = splits;
  if (sp == 0) {
    sp = G_TARGET_WGS / tiles;
    if (sp > nk2 / 8) sp = nk2 / 8;
  }
  sp = sp < 1 ? 1 : sp > nk2 ? nk2 : sp;
  const int kps = (int)((nk2 + sp - 1) / sp);
  return (nk2 + kps - 1) / kps;
}

// grad = scale * [h0^T.v0 - hk^T.vk | sum_b (h0 - hk) | sum_b (v0 - vk)] over
// the first n rows, OVERWRITING the flat f32 buffer whose segments W [H][V],
// hbias [H], vbias [V] each start on a 16-element boundary (the padding is
// set to 0).  ws: hvk_rbm_grad_splits(...) slices of the buffer's length
// (unused with one slice).
HVK_API int hvk_rbm_grad(int n, int V, int H, const void* v0, long long ld_v0,
                         const void* h0, long long ld_h0, const void* vk,
                         long long ld_vk, const void* hk, long long ld_hk,
                         float* grad, float scale, float* ws, int splits,
                         hipStream_t s) {
  if (n < 1 || V < 1 || H < 1 || !v0 || !h0 || !vk || !hk || !grad ||
      splits < 0 || ld_v0 < V || ld_vk < V || ld_h0 < H || ld_hk < H ||
      (long long)H * V >= (1ll << 31))
    return -1;
  const int sp = hvk_rbm_grad_splits(n, V, H, splits);
  if (sp < 1 || sp > 65535 || (sp > 1 && !ws)) return -1;
  GradArgs a;
  a.h0 = (const uint16_t*)h0; a.v0 = (const uint16_t*)v0;
  a.hk = (const uint16_t*)hk; a.vk = (const uint16_t*)vk;
  a.ld_h0 = ld_h0; a.ld_v0 = ld_v0; a.ld_hk = ld_hk; a.ld_vk = ld_vk;
  a.off_hb = r16((long long)H * V);
  a.off_vb = a.off_hb + r16(H);
  a.total = a.off_vb + r16(V);
  a.scale = scale;
  a.out = sp == 1 ? grad : ws;
  a.n = n; a.V = V; a.H = H;
  a.nk = (n + BK - 1) / BK;
  a.kps = (2 * a.nk + sp - 1) / sp;
  a.tiles_v = (V + GT - 1) / GT;
  const long long tiles = (long long)((H + GT - 1) / GT) * a.tiles_v;
  if (tiles >= (1ll << 31)) return -1;
  const bool vec = V % 8 == 0 && H % 8 == 0 && on_grid(v0, ld_v0) &&
                   on_grid(vk, ld_vk) && on_grid(h0, ld_h0) &&
                   on_grid(hk, ld_hk);
  const dim3 grid((unsigned)tiles, (unsigned)sp);
#define HVK_RBM_GRAD(VEC, DIRECT) \
  hipLaunchKernelGGL((rbm_grad_kernel<VEC, DIRECT>), grid, dim3(NTHR), 0, s, a)
  if (sp == 1) {
    if (vec) HVK_RBM_GRAD(true, true);
    else HVK_RBM_GRAD(false, true);
  } else {
    if (vec) HVK_RBM_GRAD(true, false);
    else HVK_RBM_GRAD(false, false);
    hipLaunchKernelGGL(rbm_grad_finish,
                       dim3((unsigned)((a.total + NTHR - 1) / NTHR)),
                       dim3(NTHR), 0, s, grad, ws, (long long)H * V, a.off_hb,
                       H, a.off_vb, V, a.total, sp, scale);
  }
#undef HVK_RBM_GRAD
  return (int)launch_status(s);
}
