// attention.hip - multi-head scaled dot-product self-attention, flash style
// (no [T][T] tensor in memory); gfx950, v_mfma_f32_32x32x16_bf16.
//
//   hvk_attn_fwd        o = softmax(q k^T / sqrt(D)) v, lse = ln sum exp(score)
//   hvk_attn_bwd_delta  delta = rowsum(do * o)
//   hvk_attn_bwd_dkv    dk, dv: a workgroup owns 128 keys, sweeps the queries
//   hvk_attn_bwd_dq     dq:     a workgroup owns 128 queries, sweeps the keys
//
// Operands are [B][T][NH*D] bf16 views with a row pitch each (head h at
// columns h*D ..), lse / delta are float32 [B][NH][T].  D is 32, 64 or 128.
//
// Tiling.  A workgroup is 4 waves and owns AT_OWN = 128 rows (queries in
// fwd / dq, keys in dkv) of one (batch, head), 32 per wave, ONE ROW PER LANE
// PAIR (lane & 31; the lane halves split the other index).  It sweeps the
// other index in tiles of AT_SWEEP = 32 rows that all four waves read from
// one LDS copy.  The first product of a tile is oriented so that the swept
// index is the accumulator's row (its 16 registers) and the owned row its
// column (the lane):
//   fwd, dq:  S^T = K Q^T, dP^T = V dO^T      (query on the lane)
//   dkv:      S = Q K^T,   dP = dO V^T        (key on the lane)
// so the softmax statistics (fwd) and lse / delta (dq) are lane-local, and
// the packed bf16 accumulators are the B operand of the second product,
// which sums over the swept index, with no LDS round trip:
//   O^T += V^T P^T,  dQ^T += K^T dS^T,  dV^T += dO^T P,  dK^T += Q^T dS.
// Registers 8s .. 8s+7 of the accumulator are k-step s; element j of lane
// half h is swept row 16s + 8(j >> 2) + 4h + (j & 3), so the A operand of the
// second product (the swept tile TRANSPOSED) is staged in that k order
// (at_trpos): a lane's 8 elements are 16 contiguous bytes of LDS.
//
// LDS images of a 32-row tile.  Row image [32][D]: 16-byte chunks XOR-ed with
// the row (A operand of the first product, one ds_read_b128 per k-step).
// Transposed image [D][AT_TRP]: written once per workgroup with 2-byte
// stores at staging, read with one ds_read_b128 per (32 columns, k-step).
//
// dq and dkv recompute S and dP each (7 products per tile pair instead of 5):
// no atomics and no workgroup waiting for another, so results repeat bit for
// bit (docs/OPS.md "Attention").
//
// Masking: rows past T are loaded from the clamped row T-1 and masked to an
// exact 0 in P; stores are guarded.  Every query row sees key 0 in the first
// tile it visits, so the running maximum is finite from then on.
#include "hvk_common.h"

using namespace hvk;

namespace {

constexpr int AT_THREADS = 256;
constexpr int AT_OWN = 128;    // rows a workgroup owns (32 per wave)
constexpr int AT_SWEEP = 32;   // rows of a swept tile
constexpr int AT_TRP = 40;     // row pitch of a transposed image (elements)
constexpr float AT_LOG2E = 1.4426950408889634f;
constexpr float AT_LN2 = 0.6931471805599453f;

template <int D>
constexpr int at_sw() { return (D / 8 < 8 ? D / 8 : 8) - 1; }

// 8 consecutive bf16 at p
template <bool VEC>
__device__ __forceinline__ uint4 at_ld8(const uint16_t* __restrict__ p) {
  if constexpr (VEC) {
    return *(const uint4*)p;
  } else {
    uint32_t e[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) e[j] = p[j];
    return make_uint4(e[0] | e[1] << 16, e[2] | e[3] << 16, e[4] | e[5] << 16,
                      e[6] | e[7] << 16);
  }
}
// 4 floats -> 4 consecutive bf16 at p
template <bool VEC>
__device__ __forceinline__ void at_st4(uint16_t* __restrict__ p, float a,
                                       float b, float c, float d) {
  const uint32_t lo = pack_bf16x2(a, b), hi = pack_bf16x2(c, d);
  if constexpr (VEC) {
    *(uint2*)p = make_uint2(lo, hi);
  } else {
    p[0] = (uint16_t)lo;
    p[1] = (uint16_t)(lo >> 16);
    p[2] = (uint16_t)hi;
    p[3] = (uint16_t)(hi >> 16);
  }
}

// position of swept row kk inside a row of a transposed image: k-step
// s = kk >> 4, lane half h = (kk >> 2) & 1, element j = ((kk >> 3) & 1) * 4 +
// (kk & 3); slot (s, h) holds its 8 elements contiguously
__device__ __forceinline__ int at_trpos(int kk) {
  return (((kk >> 4) * 2 + ((kk >> 2) & 1)) << 3) + (((kk >> 3) & 1) << 2) +
         (kk & 3);
}

// Rows r0 .. r0 + 31 (clamped to T - 1) of src [T][D] -> the row image and /
// or the transposed image.  Consecutive lanes take consecutive rows of one
// 8-column chunk: the 2-byte stores of a wave then fall into 16 banks.
template <int D, bool VEC, bool ROW, bool TR>
__device__ __forceinline__ void at_stage(const uint16_t* __restrict__ src,
                                         long long ld, int r0, int T,
                                         uint16_t* rowimg, uint16_t* trimg) {
#pragma unroll
  for (int c = threadIdx.x; c < 32 * (D / 8); c += AT_THREADS) {
    const int row = c & 31, ch = c >> 5;
    const int t = min(r0 + row, T - 1);
    const uint4 u = at_ld8<VEC>(src + (long long)t * ld + ch * 8);
    if constexpr (ROW)
      *(uint4*)(rowimg + row * D + ((ch ^ (row & at_sw<D>())) << 3)) = u;
    if constexpr (TR) {
      const uint32_t w[4] = {u.x, u.y, u.z, u.w};
      const int pos = at_trpos(row);
#pragma unroll
      for (int e = 0; e < 8; ++e)
        trimg[(ch * 8 + e) * AT_TRP + pos] =
            (uint16_t)(w[e >> 1] >> ((e & 1) * 16));
    }
  }
}

// A fragment of the first product: row r, columns 8 * chunk .. + 7
template <int D>
__device__ __forceinline__ bf16x8 at_rowfrag(const uint16_t* img, int r,
                                             int chunk) {
  return __builtin_bit_cast(
      bf16x8, *(const uint4*)(img + r * D + ((chunk ^ (r & at_sw<D>())) << 3)));
}
// A fragment of the second product: column d of the tile, slot = 2 s + h
__device__ __forceinline__ bf16x8 at_trfrag(const uint16_t* img, int d,
                                            int slot) {
  return __builtin_bit_cast(bf16x8,
                            *(const uint4*)(img + d * AT_TRP + slot * 8));
}
__device__ __forceinline__ bf16x8 at_pack8(const float* v) {
  return __builtin_bit_cast(bf16x8, pack_bf16x8(v));
}
__device__ __forceinline__ f32x16 at_mfma(bf16x8 a, bf16x8 b, f32x16 c) {
  return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0);
}
__device__ __forceinline__ f32x16 at_zero() {
  f32x16 z;
#pragma unroll
  for (int i = 0; i < 16; ++i) z[i] = 0.f;
  return z;
}
// swept row of accumulator register i in lane half hh
__device__ __forceinline__ int at_accrow(int i, int hh) {
  return (i & 3) + 8 * (i >> 2) + 4 * hh;
}

struct AtIds {
  int tile, b, h, bh;
};
// later_first: under the causal mask the later query tiles carry more work
// (fwd, dq), so they are launched first
__device__ __forceinline__ AtIds at_ids(int ntiles, int NH, bool later_first) {
  AtIds a;
  const int bid = blockIdx.x;
  const int t = bid % ntiles;
  a.tile = later_first ? ntiles - 1 - t : t;
  a.bh = bid / ntiles;
  a.h = a.bh % NH;
  a.b = a.bh / NH;
  return a;
}

// accumulators [column d of the head][owned row on the lane] -> dst[row][d]
template <int D, bool VEC>
__device__ __forceinline__ void at_store_t(uint16_t* __restrict__ dst,
                                           long long ld, int row, int hh,
                                           const f32x16* acc, float mul) {
#pragma unroll
  for (int db = 0; db < D / 32; ++db)
#pragma unroll
    for (int g = 0; g < 4; ++g)
      at_st4<VEC>(dst + (long long)row * ld + db * 32 + 8 * g + 4 * hh,
                  acc[db][4 * g] * mul, acc[db][4 * g + 1] * mul,
                  acc[db][4 * g + 2] * mul, acc[db][4 * g + 3] * mul);
}

// ---------------------------------------------------------------- forward
template <int D, bool VEC>
__global__ void __launch_bounds__(AT_THREADS)
attn_fwd_kernel(const uint16_t* __restrict__ q, long long ldq,
                const uint16_t* __restrict__ k, long long ldk,
                const uint16_t* __restrict__ v, long long ldv,
                uint16_t* __restrict__ o, long long ldo,
                float* __restrict__ lse, int T, int NH, int ntiles, int causal,
                float c2) {
  __shared__ __attribute__((aligned(16))) uint16_t kimg[32 * D];
  __shared__ __attribute__((aligned(16))) uint16_t vtimg[D * AT_TRP];
  const AtIds id = at_ids(ntiles, NH, true);
  const long long row0 = (long long)id.b * T;
  q += row0 * ldq + id.h * D;
  k += row0 * ldk + id.h * D;
  v += row0 * ldv + id.h * D;
  o += row0 * ldo + id.h * D;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int r = lane & 31, hh = lane >> 5;
  const int q0 = id.tile * AT_OWN, wq0 = q0 + 32 * w, qi = wq0 + r;
  const bool wave_on = wq0 < T;
  const int qc = min(qi, T - 1);
  bf16x8 qf[D / 16];
#pragma unroll
  for (int s = 0; s < D / 16; ++s)
    qf[s] = __builtin_bit_cast(
        bf16x8, at_ld8<VEC>(q + (long long)qc * ldq + 16 * s + 8 * hh));
  f32x16 oacc[D / 32];
#pragma unroll
  for (int db = 0; db < D / 32; ++db) oacc[db] = at_zero();
  float m = -INFINITY, l = 0.f;
  const int klast = causal ? min(T - 1, q0 + AT_OWN - 1) : T - 1;
  const int nkt = klast / AT_SWEEP + 1;
  for (int kt = 0; kt < nkt; ++kt) {
    const int k0 = kt * AT_SWEEP;
    if (kt) __syncthreads();
    at_stage<D, VEC, true, false>(k, ldk, k0, T, kimg, nullptr);
    at_stage<D, VEC, false, true>(v, ldv, k0, T, nullptr, vtimg);
    __syncthreads();
    if (!wave_on || (causal && k0 > wq0)) continue;   // wave-uniform
    f32x16 sacc = at_zero();
#pragma unroll
    for (int s = 0; s < D / 16; ++s)
      sacc = at_mfma(at_rowfrag<D>(kimg, r, 2 * s + hh), qf[s], sacc);
    const bool edge = k0 + AT_SWEEP > T || (causal && k0 == wq0);
    float p[16];
    float mx = -INFINITY;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      float sv = sacc[i] * c2;
      if (edge) {
        const int key = k0 + at_accrow(i, hh);
        if (key >= T || (causal && key > qi)) sv = -INFINITY;
      }
      p[i] = sv;
      mx = fmaxf(mx, sv);
    }
    mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
    const float mn = fmaxf(m, mx);
    const float alpha = __builtin_amdgcn_exp2f(m - mn);
    float sum = 0.f;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      p[i] = __builtin_amdgcn_exp2f(p[i] - mn);
      sum += p[i];
    }
    sum += __shfl_xor(sum, 32, 64);
    l = l * alpha + sum;
    m = mn;
#pragma unroll
    for (int db = 0; db < D / 32; ++db)
#pragma unroll
      for (int i = 0; i < 16; ++i) oacc[db][i] *= alpha;
    const bf16x8 pb[2] = {at_pack8(p), at_pack8(p + 8)};
#pragma unroll
    for (int db = 0; db < D / 32; ++db)
#pragma unroll
      for (int s = 0; s < 2; ++s)
        oacc[db] = at_mfma(at_trfrag(vtimg, db * 32 + r, 2 * s + hh), pb[s],
                           oacc[db]);
  }
  if (wave_on && qi < T) {
    at_store_t<D, VEC>(o, ldo, qi, hh, oacc, 1.f / l);
    if (hh == 0) lse[(long long)id.bh * T + qi] = m * AT_LN2 + logf(l);
  }
}

// ------------------------------------------------------------------ delta
// delta[b][h][t] = sum_d do[b][t][h*D + d] * o[b][t][h*D + d]; D / 8 lanes
// share a row (8 columns each) and add up in a fixed tree
template <int D, bool VEC>
__global__ void __launch_bounds__(AT_THREADS)
attn_delta_kernel(const uint16_t* __restrict__ dout, long long lddo,
                  const uint16_t* __restrict__ o, long long ldo,
                  float* __restrict__ delta, int T, int NH, long long rows) {
  constexpr int G = D / 8;
  const long long gid = (long long)blockIdx.x * AT_THREADS + threadIdx.x;
  const long long row = gid / G;
  const int c = (int)(gid % G);
  const long long rc = row < rows ? row : rows - 1;
  const long long bt = rc / NH;
  const int h = (int)(rc % NH);
  const uint4 a = at_ld8<VEC>(dout + bt * lddo + h * D + c * 8);
  const uint4 b = at_ld8<VEC>(o + bt * ldo + h * D + c * 8);
  const uint32_t aw[4] = {a.x, a.y, a.z, a.w}, bw[4] = {b.x, b.y, b.z, b.w};
  float s = 0.f;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    s = __builtin_fmaf(__uint_as_float(aw[j] << 16),
                       __uint_as_float(bw[j] << 16), s);
    s = __builtin_fmaf(__uint_as_float(aw[j] & 0xffff0000u),
                       __uint_as_float(bw[j] & 0xffff0000u), s);
  }
#pragma unroll
  for (int off = G / 2; off > 0; off >>= 1) s += __shfl_xor(s, off, 64);
  if (row < rows && c == 0) {
    const long long b_ = bt / T, t = bt % T;
    delta[(b_ * NH + h) * T + t] = s;
  }
}

// --------------------------------------------------------------------- dq
template <int D, bool VEC>
__global__ void __launch_bounds__(AT_THREADS)
attn_dq_kernel(const uint16_t* __restrict__ q, long long ldq,
               const uint16_t* __restrict__ k, long long ldk,
               const uint16_t* __restrict__ v, long long ldv,
               const uint16_t* __restrict__ dout, long long lddo,
               const float* __restrict__ lse, const float* __restrict__ delta,
               uint16_t* __restrict__ dq, long long lddq, int T, int NH,
               int ntiles, int causal, float c2, float scale) {
  __shared__ __attribute__((aligned(16))) uint16_t kimg[32 * D];
  __shared__ __attribute__((aligned(16))) uint16_t vimg[32 * D];
  __shared__ __attribute__((aligned(16))) uint16_t ktimg[D * AT_TRP];
  const AtIds id = at_ids(ntiles, NH, true);
  const long long row0 = (long long)id.b * T;
  q += row0 * ldq + id.h * D;
  k += row0 * ldk + id.h * D;
  v += row0 * ldv + id.h * D;
  dout += row0 * lddo + id.h * D;
  dq += row0 * lddq + id.h * D;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int r = lane & 31, hh = lane >> 5;
  const int q0 = id.tile * AT_OWN, wq0 = q0 + 32 * w, qi = wq0 + r;
  const bool wave_on = wq0 < T;
  const int qc = min(qi, T - 1);
  bf16x8 qf[D / 16], dof[D / 16];
#pragma unroll
  for (int s = 0; s < D / 16; ++s) {
    qf[s] = __builtin_bit_cast(
        bf16x8, at_ld8<VEC>(q + (long long)qc * ldq + 16 * s + 8 * hh));
    dof[s] = __builtin_bit_cast(
        bf16x8, at_ld8<VEC>(dout + (long long)qc * lddo + 16 * s + 8 * hh));
  }
  const float lse2 = lse[(long long)id.bh * T + qc] * AT_LOG2E;
  const float dl = delta[(long long)id.bh * T + qc];
  f32x16 acc[D / 32];
#pragma unroll
  for (int db = 0; db < D / 32; ++db) acc[db] = at_zero();
  const int klast = causal ? min(T - 1, q0 + AT_OWN - 1) : T - 1;
  const int nkt = klast / AT_SWEEP + 1;
  for (int kt = 0; kt < nkt; ++kt) {
    const int k0 = kt * AT_SWEEP;
    if (kt) __syncthreads();
    at_stage<D, VEC, true, true>(k, ldk, k0, T, kimg, ktimg);
    at_stage<D, VEC, true, false>(v, ldv, k0, T, vimg, nullptr);
    __syncthreads();
    if (!wave_on || (causal && k0 > wq0)) continue;   // wave-uniform
    f32x16 sacc = at_zero(), pacc = at_zero();
#pragma unroll
    for (int s = 0; s < D / 16; ++s) {
      sacc = at_mfma(at_rowfrag<D>(kimg, r, 2 * s + hh), qf[s], sacc);
      pacc = at_mfma(at_rowfrag<D>(vimg, r, 2 * s + hh), dof[s], pacc);
    }
    const bool edge = k0 + AT_SWEEP > T || (causal && k0 == wq0);
    float ds[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      float pv = __builtin_amdgcn_exp2f(sacc[i] * c2 - lse2);
      if (edge) {
        const int key = k0 + at_accrow(i, hh);
        if (key >= T || (causal && key > qi)) pv = 0.f;
      }
      ds[i] = pv * (pacc[i] - dl) * scale;
    }
    const bf16x8 dsb[2] = {at_pack8(ds), at_pack8(ds + 8)};
#pragma unroll
    for (int db = 0; db < D / 32; ++db)
#pragma unroll
      for (int s = 0; s < 2; ++s)
        acc[db] = at_mfma(at_trfrag(ktimg, db * 32 + r, 2 * s + hh), dsb[s],
                          acc[db]);
  }
  if (wave_on && qi < T) at_store_t<D, VEC>(dq, lddq, qi, hh, acc, 1.f);
}

// -------------------------------------------------------------------- dkv
template <int D, bool VEC>
__global__ void __launch_bounds__(AT_THREADS)
attn_dkv_kernel(const uint16_t* __restrict__ q, long long ldq,
                const uint16_t* __restrict__ k, long long ldk,
                const uint16_t* __restrict__ v, long long ldv,
                const uint16_t* __restrict__ dout, long long lddo,
                const float* __restrict__ lse, const float* __restrict__ delta,
                uint16_t* __restrict__ dk, long long lddk,
                uint16_t* __restrict__ dv, long long lddv, int T, int NH,
                int ntiles, int causal, float c2, float scale) {
  __shared__ __attribute__((aligned(16))) uint16_t qimg[32 * D];
  __shared__ __attribute__((aligned(16))) uint16_t doimg[32 * D];
  __shared__ __attribute__((aligned(16))) uint16_t qtimg[D * AT_TRP];
  __shared__ __attribute__((aligned(16))) uint16_t dotimg[D * AT_TRP];
  __shared__ float rowc[2][AT_SWEEP];   // lse * log2(e), delta of the tile
  const AtIds id = at_ids(ntiles, NH, false);
  const long long row0 = (long long)id.b * T;
  q += row0 * ldq + id.h * D;
  k += row0 * ldk + id.h * D;
  v += row0 * ldv + id.h * D;
  dout += row0 * lddo + id.h * D;
  dk += row0 * lddk + id.h * D;
  dv += row0 * lddv + id.h * D;
  lse += (long long)id.bh * T;
  delta += (long long)id.bh * T;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int r = lane & 31, hh = lane >> 5;
  const int kb0 = id.tile * AT_OWN, wk0 = kb0 + 32 * w, kj = wk0 + r;
  const bool wave_on = wk0 < T;
  const int kc = min(kj, T - 1);
  bf16x8 kf[D / 16], vf[D / 16];
#pragma unroll
  for (int s = 0; s < D / 16; ++s) {
    kf[s] = __builtin_bit_cast(
        bf16x8, at_ld8<VEC>(k + (long long)kc * ldk + 16 * s + 8 * hh));
    vf[s] = __builtin_bit_cast(
        bf16x8, at_ld8<VEC>(v + (long long)kc * ldv + 16 * s + 8 * hh));
  }
  f32x16 dkacc[D / 32], dvacc[D / 32];
#pragma unroll
  for (int db = 0; db < D / 32; ++db) dkacc[db] = dvacc[db] = at_zero();
  const int nqt = (T - 1) / AT_SWEEP + 1;
  const int qt_first = causal ? kb0 / AT_SWEEP : 0;
  for (int qt = qt_first; qt < nqt; ++qt) {
    const int qt0 = qt * AT_SWEEP;
    if (qt != qt_first) __syncthreads();
    at_stage<D, VEC, true, true>(q, ldq, qt0, T, qimg, qtimg);
    at_stage<D, VEC, true, true>(dout, lddo, qt0, T, doimg, dotimg);
    if (threadIdx.x < 2 * AT_SWEEP) {
      const int t = min(qt0 + (int)(threadIdx.x & 31), T - 1);
      rowc[threadIdx.x >> 5][threadIdx.x & 31] =
          threadIdx.x < AT_SWEEP ? lse[t] * AT_LOG2E : delta[t];
    }
    __syncthreads();
    if (!wave_on || (causal && qt0 < wk0)) continue;   // wave-uniform
    f32x16 sacc = at_zero(), pacc = at_zero();
#pragma unroll
    for (int s = 0; s < D / 16; ++s) {
      sacc = at_mfma(at_rowfrag<D>(qimg, r, 2 * s + hh), kf[s], sacc);
      pacc = at_mfma(at_rowfrag<D>(doimg, r, 2 * s + hh), vf[s], pacc);
    }
    const bool edge = qt0 + AT_SWEEP > T || wk0 + 32 > T ||
                      (causal && qt0 == wk0);
    float p[16], ds[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int qr = at_accrow(i, hh);
      float pv = __builtin_amdgcn_exp2f(sacc[i] * c2 - rowc[0][qr]);
      if (edge) {
        const int qrow = qt0 + qr;
        if (qrow >= T || kj >= T || (causal && kj > qrow)) pv = 0.f;
      }
      p[i] = pv;
      ds[i] = pv * (pacc[i] - rowc[1][qr]) * scale;
    }
    const bf16x8 pb[2] = {at_pack8(p), at_pack8(p + 8)};
    const bf16x8 dsb[2] = {at_pack8(ds), at_pack8(ds + 8)};
#pragma unroll
    for (int db = 0; db < D / 32; ++db)
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        dvacc[db] = at_mfma(at_trfrag(dotimg, db * 32 + r, 2 * s + hh), pb[s],
                            dvacc[db]);
        dkacc[db] = at_mfma(at_trfrag(qtimg, db * 32 + r, 2 * s + hh), dsb[s],
                            dkacc[db]);
      }
  }
  if (wave_on && kj < T) {
    at_store_t<D, VEC>(dk, lddk, kj, hh, dkacc, 1.f);
    at_store_t<D, VEC>(dv, lddv, kj, hh, dvacc, 1.f);
  }
}

// ------------------------------------------------------------ host checks
inline bool at_view_ok(const void* p, long long ld, long long rows, int E) {
  return p != nullptr && (((uintptr_t)p) & 1) == 0 && ld >= E &&
         rows * ld < (1ll << 31);
}
inline bool at_on16(const void* p, long long ld) {
  return (((uintptr_t)p) & 15) == 0 && ld % 8 == 0;
}
inline bool at_shape_ok(int B, int T, int NH, int D) {
  if (B < 1 || T < 1 || NH < 1 || (D != 32 && D != 64 && D != 128))
    return false;
  const long long rows = (long long)B * T;
  const long long tiles = (T + AT_OWN - 1) / AT_OWN;
  return rows < (1ll << 31) / ((long long)NH * D) &&
         tiles * B * NH < (1ll << 31);
}
inline float at_scale(int D) { return 1.f / sqrtf((float)D); }

#define HVK_AT_DISPATCH(KERNEL, grid, ...)                                   \
  do {                                                                       \
    if (vec) {                                                               \
      if (D == 32)                                                           \
        hipLaunchKernelGGL((KERNEL<32, true>), grid, dim3(AT_THREADS), 0, s, \
                           __VA_ARGS__);                                     \
      else if (D == 64)                                                      \
        hipLaunchKernelGGL((KERNEL<64, true>), grid, dim3(AT_THREADS), 0, s, \
                           __VA_ARGS__);                                     \
      else                                                                   \
        hipLaunchKernelGGL((KERNEL<128, true>), grid, dim3(AT_THREADS), 0,   \
                           s, __VA_ARGS__);                                  \
    } else {                                                                 \
      if (D == 32)                                                           \
        hipLaunchKernelGGL((KERNEL<32, false>), grid, dim3(AT_THREADS), 0,   \
                           s, __VA_ARGS__);                                  \
      else if (D == 64)                                                      \
        hipLaunchKernelGGL((KERNEL<64, false>), grid, dim3(AT_THREADS), 0,   \
                           s, __VA_ARGS__);                                  \
      else                                                                   \
        hipLaunchKernelGGL((KERNEL<128, false>), grid, dim3(AT_THREADS), 0,  \
                           s, __VA_ARGS__);                                  \
    }                                                                        \
  } while (0)

}  // namespace

// Rows a workgroup owns (which = 0) and rows of a swept tile (which = 1):
// the tile edges the tests are built around
HVK_API int hvk_attn_tile(int which) { return which ? AT_SWEEP : AT_OWN; }

// o [B][T][NH*D] = softmax(q k^T / sqrt(D), keys j <= i when causal) v per
// (batch, head); lse [B][NH][T] = ln sum_j exp(score).  Row pitches in
// elements.  Returns -1 on a bad argument before any launch.
HVK_API int hvk_attn_fwd(const void* q, long long ldq, const void* k,
                         long long ldk, const void* v, long long ldv, void* o,
                         long long ldo, float* lse, int B, int T, int NH,
                         int D, int causal, hipStream_t s) {
  if (!at_shape_ok(B, T, NH, D) || !lse) return -1;
  const long long rows = (long long)B * T;
  const int E = NH * D;
  if (!at_view_ok(q, ldq, rows, E) || !at_view_ok(k, ldk, rows, E) ||
      !at_view_ok(v, ldv, rows, E) || !at_view_ok(o, ldo, rows, E))
    return -1;
  const bool vec = at_on16(q, ldq) && at_on16(k, ldk) && at_on16(v, ldv) &&
                   at_on16(o, ldo);
  const int ntiles = (T + AT_OWN - 1) / AT_OWN;
  const dim3 grid((unsigned)((long long)ntiles * B * NH));
  HVK_AT_DISPATCH(attn_fwd_kernel, grid, (const uint16_t*)q, ldq,
                  (const uint16_t*)k, ldk, (const uint16_t*)v, ldv,
                  (uint16_t*)o, ldo, lse, T, NH, ntiles, causal != 0,
                  at_scale(D) * AT_LOG2E);
  return (int)launch_status(s);
}

// delta [B][NH][T] = rowsum over a head's columns of do * o
HVK_API int hvk_attn_bwd_delta(const void* dout, long long lddo,
                               const void* o, long long ldo, float* delta,
                               int B, int T, int NH, int D, hipStream_t s) {
  if (!at_shape_ok(B, T, NH, D) || !delta) return -1;
  const long long rows = (long long)B * T;
  const int E = NH * D;
  if (!at_view_ok(dout, lddo, rows, E) || !at_view_ok(o, ldo, rows, E))
    return -1;
  const bool vec = at_on16(dout, lddo) && at_on16(o, ldo);
  const long long nrows = rows * NH;
  const long long threads = nrows * (D / 8);
  const dim3 grid((unsigned)((threads + AT_THREADS - 1) / AT_THREADS));
  HVK_AT_DISPATCH(attn_delta_kernel, grid, (const uint16_t*)dout, lddo,
                  (const uint16_t*)o, ldo, delta, T, NH, nrows);
  return (int)launch_status(s);
}

// dk, dv from q, k, v, do and the forward's lse and hvk_attn_bwd_delta's
// delta
HVK_API int hvk_attn_bwd_dkv(const void* q, long long ldq, const void* k,
                             long long ldk, const void* v, long long ldv,
                             const void* dout, long long lddo,
                             const float* lse, const float* delta, void* dk,
                             long long lddk, void* dv, long long lddv, int B,
                             int T, int NH, int D, int causal, hipStream_t s) {
  if (!at_shape_ok(B, T, NH, D) || !lse || !delta) return -1;
  const long long rows = (long long)B * T;
  const int E = NH * D;
  if (!at_view_ok(q, ldq, rows, E) || !at_view_ok(k, ldk, rows, E) ||
      !at_view_ok(v, ldv, rows, E) || !at_view_ok(dout, lddo, rows, E) ||
      !at_view_ok(dk, lddk, rows, E) || !at_view_ok(dv, lddv, rows, E))
    return -1;
  const bool vec = at_on16(q, ldq) && at_on16(k, ldk) && at_on16(v, ldv) &&
                   at_on16(dout, lddo) && at_on16(dk, lddk) &&
                   at_on16(dv, lddv);
  const int ntiles = (T + AT_OWN - 1) / AT_OWN;
  const dim3 grid((unsigned)((long long)ntiles * B * NH));
  HVK_AT_DISPATCH(attn_dkv_kernel, grid, (const uint16_t*)q, ldq,
                  (const uint16_t*)k, ldk, (const uint16_t*)v, ldv,
                  (const uint16_t*)dout, lddo, lse, delta, (uint16_t*)dk, lddk,
                  (uint16_t*)dv, lddv, T, NH, ntiles, causal != 0,
                  at_scale(D) * AT_LOG2E, at_scale(D));
  return (int)launch_status(s);
}

// dq from the same operands
HVK_API int hvk_attn_bwd_dq(const void* q, long long ldq, const void* k,
                            long long ldk, const void* v, long long ldv,
                            const void* dout, long long lddo, const float* lse,
                            const float* delta, void* dq, long long lddq,
                            int B, int T, int NH, int D, int causal,
                            hipStream_t s) {
  if (!at_shape_ok(B, T, NH, D) || !lse || !delta) return -1;
  const long long rows = (long long)B * T;
  const int E = NH * D;
  if (!at_view_ok(q, ldq, rows, E) || !at_view_ok(k, ldk, rows, E) ||
      !at_view_ok(v, ldv, rows, E) || !at_view_ok(dout, lddo, rows, E) ||
      !at_view_ok(dq, lddq, rows, E))
    return -1;
  const bool vec = at_on16(q, ldq) && at_on16(k, ldk) && at_on16(v, ldv) &&
                   at_on16(dout, lddo) && at_on16(dq, lddq);
  const int ntiles = (T + AT_OWN - 1) / AT_OWN;
  const dim3 grid((unsigned)((long long)ntiles * B * NH));
  HVK_AT_DISPATCH(attn_dq_kernel, grid, (const uint16_t*)q, ldq,
                  (const uint16_t*)k, ldk, (const uint16_t*)v, ldv,
                  (const uint16_t*)dout, lddo, lse, delta, (uint16_t*)dq, lddq,
                  T, NH, ntiles, causal != 0, at_scale(D) * AT_LOG2E,
                  at_scale(D));
  return (int)launch_status(s);
}
