// kohonen.hip - Kohonen (self-organising) map kernels on the exact f32 MFMA
// (v_mfma_f32_16x16x4_f32, bit-for-bit an fmaf chain; docs/OPS.md "Kohonen
// maps"):
//   hvk_kohonen_argmin  winner search: a [neurons] x [samples] product with
//                       a lexicographic (value, index) arg-min epilogue; the
//                       distance matrix is never written;
//   hvk_kohonen_update  neighbourhood update: dW = G^T . X over the batch,
//                       the gravity operand G computed in registers, applied
//                       to W in place.
// Both use the staging of gemm_f32.hip (register-staged global -> LDS, K
// tile = one 128-B LDS row of 32 f32, 16-B chunk swizzle c ^ (row & 7)) on a
// 128 x 64 tile: 128 neurons (the A operand) by 64 samples / input features
// (the B operand), 4 waves of 64 x 32.  The tile is half of gemm_f32's so
// that three workgroups share a CU (50 KiB of LDS, < 170 registers): with
// one wave per SIMD nothing covers the wait for a staged tile.  A lane reads
// 16 B of its row per fragment and feeds element j to MFMA j (lane quad q
// covers k = 4q + j, the same for both operands).  Work is spread over more
// workgroups by slices: a split writes its partial result to its own slice
// of a workspace and a finishing kernel merges the slices in split order, so
// the result does not depend on scheduling (no float atomics, no atomics in
// the arg-min).
#include <limits.h>

#include "conv_geom.h"
#include "hvk_api.h"

using namespace hvk;

namespace {

constexpr int BT = 128;    // A-operand rows of a tile (neurons)
constexpr int BX = 64;     // B-operand rows of a tile (samples / features)
constexpr int BK = 32;     // f32 per 128-B LDS row
constexpr int NTHR = 256;
constexpr int TILE_A = BT * BK, TILE_B = BX * BK;
constexpr int TARGET_WGS = 512;   // two workgroups per CU before splitting

__device__ __forceinline__ float ld1(const float* p) { return *p; }
__device__ __forceinline__ float ld1(const uint16_t* p) { return bf2f(*p); }
__device__ __forceinline__ void ld4(const float* p, float* v) {
  const float4 f = *(const float4*)p;
  v[0] = f.x; v[1] = f.y; v[2] = f.z; v[3] = f.w;
}
// bf16 -> f32 is exact: the 16 bits become the high half of the f32
__device__ __forceinline__ void ld4(const uint16_t* p, float* v) {
  const uint2 u = *(const uint2*)p;
  v[0] = __uint_as_float(u.x << 16);
  v[1] = __uint_as_float(u.x & 0xffff0000u);
  v[2] = __uint_as_float(u.y << 16);
  v[3] = __uint_as_float(u.y & 0xffff0000u);
}

// NI 16-B LDS chunks per thread per K tile: one per (row, chunk) of a K-major
// source (32 NI rows), one per (k, row chunk) of a source stored [K][rows]
// (NI = 2: 64 rows).  Elements outside [rows] x [K] are staged as 0.
template <int NI>
struct Stage {
  float v[NI][4];
  unsigned ok;   // bit 4 i + j: element j of chunk i is inside the operand
  // The loads are unconditional (an out-of-range element reads p[0] and is
  // replaced by 0 when it is stored to LDS, not before: a use right after
  // the load is a wait right after the load): a load under a branch makes
  // hipcc wait vmcnt(0) where the branches join, once per chunk, and the K
  // loop then pays a memory round trip per chunk instead of overlapping the
  // loads with the MFMAs.
  // VEC: 16-B chunks (base aligned, ld and K multiples of 4: a chunk is
  // inside the row or outside it as a whole).
  template <bool VEC, typename T>
  __device__ __forceinline__ void load_rows(const T* p, int rows, int K,
                                            long long ld, int r0, int k0,
                                            int t) {
    ok = 0;
#pragma unroll
    for (int i = 0; i < NI; ++i) {
      const int r = r0 + (t >> 3) + 32 * i, k = k0 + (t & 7) * 4;
      const T* q = p + (long long)r * ld + k;
      if constexpr (VEC) {
        const bool in = r < rows && k < K;
        ld4(in ? q : p, v[i]);
        ok |= in ? 15u << (4 * i) : 0u;
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const bool in = r < rows && k + j < K;
          v[i][j] = ld1(in ? q + j : p);
          ok |= in ? 1u << (4 * i + j) : 0u;
        }
      }
    }
  }
  // 64 rows x 32 k of a source stored [K][rows] (NI = 2)
  template <bool VEC, typename T>
  __device__ __forceinline__ void load_cols(const T* p, int rows, int K,
                                            long long ld, int r0, int k0,
                                            int t) {
    ok = 0;
#pragma unroll
    for (int i = 0; i < NI; ++i) {
      const int k = k0 + (t >> 4) + 16 * i, r = r0 + (t & 15) * 4;
      const T* q = p + (long long)k * ld + r;
      if constexpr (VEC) {
        const bool in = k < K && r < rows;
        ld4(in ? q : p, v[i]);
        ok |= in ? 15u << (4 * i) : 0u;
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const bool in = k < K && r + j < rows;
          v[i][j] = ld1(in ? q + j : p);
          ok |= in ? 1u << (4 * i + j) : 0u;
        }
      }
    }
  }
  __device__ __forceinline__ float at(int i, int j) const {
    return (ok >> (4 * i + j)) & 1u ? v[i][j] : 0.f;
  }
  // LDS image: [rows][32] with chunk c of row r at (c ^ (r & 7))
  __device__ __forceinline__ void store_rows(float* s, int t) const {
#pragma unroll
    for (int i = 0; i < NI; ++i) {
      const int r = (t >> 3) + 32 * i, c = t & 7;
      *(float4*)(s + r * BK + ((c ^ (r & 7)) * 4)) =
          make_float4(at(i, 0), at(i, 1), at(i, 2), at(i, 3));
    }
  }
  __device__ __forceinline__ void store_cols(float* s, int t) const {
#pragma unroll
    for (int i = 0; i < NI; ++i) {
      const int k = (t >> 4) + 16 * i, r0 = (t & 15) * 4;
      const int c = k >> 2, e = k & 3;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int r = r0 + j;
        s[r * BK + ((c ^ (r & 7)) * 4) + e] = at(i, j);
      }
    }
  }
};

// the 4 consecutive k of chunk 4g + (lane >> 4) of row rowbase + (lane & 15)
__device__ __forceinline__ float4 frag(const float* s, int rowbase, int g,
                                       int lane) {
  const int row = rowbase + (lane & 15);
  const int c = 4 * g + (lane >> 4);
  return *(const float4*)(s + row * BK + ((c ^ (row & 7)) * 4));
}

__device__ __forceinline__ float f4at(const float4& f, int j) {
  return j == 0 ? f.x : j == 1 ? f.y : j == 2 ? f.z : f.w;
}

// (v, i) < (bv, bi) in lexicographic order; a NaN v never wins
__device__ __forceinline__ bool lex_less(float v, int i, float bv, int bi) {
  return v < bv || (v == bv && i < bi);
}

// ---------------------------------------------------------------- winners
// A = W tile (neurons on the accumulator rows), B = X tile (samples on the
// columns = lanes), so a sample's candidates sit in one lane's registers and
// in the 4 lane quads of its column.  LDS: 2 x (W tile, X tile), then the
// tile's 128 squared norms, then the cross-wave (value, index) exchange.
template <typename XT, bool VEC>
__global__ void __launch_bounds__(NTHR)
kohonen_argmin_kernel(const XT* __restrict__ X, const float* __restrict__ W,
                      int B, int NN, int D, int ldx, float* ws_val,
                      int* ws_idx, float* ws_x2, int tps, int nt) {
  constexpr int BUF = TILE_A + TILE_B;
  __shared__ __attribute__((aligned(16))) float smem[2 * BUF + BT + 4 * BX];
  float* snorm = smem + 2 * BUF;
  float* sred_v = snorm + BT;
  int* sred_i = (int*)(sred_v + 2 * BX);

  const int b0 = blockIdx.x * BX;
  const int split = blockIdx.y;
  const int t = threadIdx.x, lane = t & 63, wid = t >> 6;
  const int wm = wid >> 1, wn = wid & 1;
  const int fr = lane & 15, fq = lane >> 4;
  const int t0 = split * tps, t1 = min(nt, t0 + tps);
  const int nk = (D + BK - 1) / BK;

  float bv[2];
  int bi[2];
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    bv[j] = __builtin_inff();
    bi[j] = INT_MAX;
  }

  for (int ti = t0; ti < t1; ++ti) {
    const int n0 = ti * BT;
    const bool first = ti == t0;
    f32x4 acc[4][2];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j) acc[i][j] = f32x4{0, 0, 0, 0};
    float nrm = 0.f;  // t < 128: |W[n0 + t]|^2; t < 192: |X[b0 + t - 128]|^2

    Stage<4> ra;
    Stage<2> rb;
    ra.load_rows<VEC>(W, NN, D, D, n0, 0, t);
    rb.load_rows<VEC>(X, B, D, ldx, b0, 0, t);
    ra.store_rows(smem, t);
    rb.store_rows(smem + TILE_A, t);
    __syncthreads();
    int cur = 0;
    for (int kt = 0; kt < nk; ++kt) {
      // the next tile's loads, also after the last tile (all out of
      // range then: they read element 0), so that nothing loaded joins a
      // branch
      ra.load_rows<VEC>(W, NN, D, D, n0, (kt + 1) * BK, t);
      rb.load_rows<VEC>(X, B, D, ldx, b0, (kt + 1) * BK, t);
      // issue them all before the first MFMA
      __builtin_amdgcn_sched_barrier(0);
      const float* sA = smem + cur * BUF;
      const float* sB = sA + TILE_A;
#pragma unroll
      for (int g = 0; g < 2; ++g) {
        float4 af[4], bf[2];
#pragma unroll
        for (int i = 0; i < 4; ++i) af[i] = frag(sA, wm * 64 + i * 16, g, lane);
#pragma unroll
        for (int i = 0; i < 2; ++i) bf[i] = frag(sB, wn * 32 + i * 16, g, lane);
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
          for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int jj = 0; jj < 2; ++jj)
              acc[i][jj] = __builtin_amdgcn_mfma_f32_16x16x4f32(
                  f4at(af[i], j), f4at(bf[jj], j), acc[i][jj], 0, 0, 0);
      }
      // squared norms from the staged rows.  |W[n]|^2: one fmaf chain in k
      // order, like the MFMA's.  |x_b|^2 (only the quantisation error reads
      // it): a chain per K tile, the tile sums then added up - a single
      // chain over same-sign bf16 data adds a multiple of half an ulp to
      // an even sum at every step and every tie rounds down (-0.75 at
      // |x|^2 = 1e5, D = 1000)
      if (t < BT || (first && t < BT + BX)) {
        const int row = t < BT ? t : t - BT;
        const float* s = (t < BT ? sA : sB) + row * BK;
        float part = t < BT ? nrm : 0.f;
#pragma unroll
        for (int c = 0; c < 8; ++c) {
          const float4 f = *(const float4*)(s + ((c ^ (row & 7)) * 4));
          part = fmaf(f.x, f.x, part);
          part = fmaf(f.y, f.y, part);
          part = fmaf(f.z, f.z, part);
          part = fmaf(f.w, f.w, part);
        }
        nrm = t < BT ? part : nrm + part;
      }
      // also after the last tile (zeros, into the buffer nobody reads): a
      // store under a branch would take its loads along.  The barrier keeps
      // the stores, the loads' first use, below the MFMAs.
      __builtin_amdgcn_sched_barrier(0);
      ra.store_rows(smem + (cur ^ 1) * BUF, t);
      rb.store_rows(smem + (cur ^ 1) * BUF + TILE_A, t);
      __syncthreads();
      cur ^= 1;
    }
    if (t < BT) {
      snorm[t] = nrm;
    } else if (first && split == 0 && t < BT + BX && b0 + t - BT < B) {
      ws_x2[b0 + t - BT] = nrm;
    }
    __syncthreads();
    // s = |W[n]|^2 - 2 x.W[n]; a lane walks its rows in ascending n
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = wm * 64 + i * 16 + 4 * fq + r;
        const int n = n0 + row;
        const float w2 = snorm[row];
#pragma unroll
        for (int j = 0; j < 2; ++j) {
          const float s =
              n < NN ? fmaf(-2.f, acc[i][j][r], w2) : __builtin_inff();
          if (lex_less(s, n, bv[j], bi[j])) {
            bv[j] = s;
            bi[j] = n;
          }
        }
      }
    // snorm is next written after a barrier of the next tile's K loop
  }

  // across the 4 lane quads of a column, then across the two row waves
#pragma unroll
  for (int j = 0; j < 2; ++j) {
#pragma unroll
    for (int o = 16; o <= 32; o <<= 1) {
      const float ov = __shfl_xor(bv[j], o, 64);
      const int oi = __shfl_xor(bi[j], o, 64);
      if (lex_less(ov, oi, bv[j], bi[j])) {
        bv[j] = ov;
        bi[j] = oi;
      }
    }
    if (fq == 0) {
      sred_v[wm * BX + wn * 32 + j * 16 + fr] = bv[j];
      sred_i[wm * BX + wn * 32 + j * 16 + fr] = bi[j];
    }
  }
  __syncthreads();
  if (t < BX && b0 + t < B) {
    float v = sred_v[t];
    int i = sred_i[t];
    if (lex_less(sred_v[BX + t], sred_i[BX + t], v, i)) {
      v = sred_v[BX + t];
      i = sred_i[BX + t];
    }
    ws_val[(long long)split * B + b0 + t] = v;
    ws_idx[(long long)split * B + b0 + t] = i;
  }
}

__global__ void __launch_bounds__(NTHR)
kohonen_argmin_finish(const float* __restrict__ ws_val,
                      const int* __restrict__ ws_idx,
                      const float* __restrict__ ws_x2, int B, int NN,
                      int splits, int* argmin, float* qerr, int* winners) {
  const int b = blockIdx.x * NTHR + threadIdx.x;
  if (b >= B) return;
  float v = ws_val[b];
  int i = ws_idx[b];
  for (int s = 1; s < splits; ++s) {
    const float ov = ws_val[(long long)s * B + b];
    const int oi = ws_idx[(long long)s * B + b];
    if (lex_less(ov, oi, v, i)) {
      v = ov;
      i = oi;
    }
  }
  i = min(max(i, 0), NN - 1);  // a row of NaNs leaves INT_MAX
  argmin[b] = i;
  if (qerr) qerr[b] = fmaxf(0.f, ws_x2[b] + v);
  if (winners) atomicAdd(winners + i, 1);
}

// ----------------------------------------------------------------- update
// dW[n][d] = sum_b G[b][n] X[b][d]: A = G^T (neurons on the rows, computed in
// registers from the lane's own neuron coords and the K tile's winner
// coords), B = X stored [K = b][rows = d].  LDS: 2 X tiles, 2 x 32 winner
// records (x, y, valid, -), 128 row sums.
template <typename XT, bool DIRECT, bool VEC>
__global__ void __launch_bounds__(NTHR)
kohonen_update_kernel(const XT* __restrict__ X, float* W,
                      const float* __restrict__ coords,
                      const int* __restrict__ argmin, int B, int NN, int D,
                      int ldx, float inv2s2, float gmult, float* ws, int kps,
                      int nk, int tiles_d) {
  __shared__ __attribute__((aligned(16)))
      float smem[2 * TILE_B + 2 * 4 * BK + BT];
  float4* swin = (float4*)(smem + 2 * TILE_B);
  float* srs = smem + 2 * TILE_B + 2 * 4 * BK;

  const int tm = blockIdx.x / tiles_d, td = blockIdx.x - tm * tiles_d;
  const int split = blockIdx.y;
  const int m0 = tm * BT, d0 = td * BX;
  const int t = threadIdx.x, lane = t & 63, wid = t >> 6;
  const int wm = wid >> 1, wn = wid & 1;
  const int fr = lane & 15, fq = lane >> 4;
  const int kt0 = split * kps, kt1 = min(nk, kt0 + kps);

  float nx[4], ny[4], rs[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int n = m0 + wm * 64 + i * 16 + fr;
    nx[i] = n < NN ? coords[2 * n] : 0.f;
    ny[i] = n < NN ? coords[2 * n + 1] : 0.f;
    rs[i] = 0.f;
  }
  f32x4 acc[4][2];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) acc[i][j] = f32x4{0, 0, 0, 0};

  // Winner records of a K tile: (coords[argmin[b]], valid); rows past B carry
  // valid = 0, an index outside the map is clamped into it.  The index of
  // tile kt + 3 is fetched while the coords of tile kt + 2 are, a tile
  // ahead of their use (two dependent loads in one step would expose two
  // memory round trips per K tile); unconditional loads from clamped
  // addresses, as in Stage.
  const int tb = t & (BK - 1);
  auto index = [&](int kt) {
    return argmin[min(kt * BK + tb, B - 1)];
  };
  auto record = [&](int kt, int a) {
    a = min(max(a, 0), NN - 1);
    return make_float4(coords[2 * a], coords[2 * a + 1],
                       kt * BK + tb < B ? 1.f : 0.f, 0.f);
  };

  Stage<2> rb;
  rb.load_cols<VEC>(X, D, B, ldx, d0, kt0 * BK, t);
  float4 rw = record(kt0, index(kt0));
  rb.store_cols(smem, t);
  if (t < BK) swin[t] = rw;
  rw = record(kt0 + 1, index(kt0 + 1));
  int ai = index(kt0 + 2);
  __syncthreads();
  int cur = 0;
  for (int kt = kt0; kt < kt1; ++kt) {
    // unconditional, as in the winner search (past this split's last tile
    // they read the next split's rows or element 0, and are dropped)
    rb.load_cols<VEC>(X, D, B, ldx, d0, (kt + 1) * BK, t);
    // keep the loads above the MFMAs: hipcc otherwise sinks them to their
    // first use, the LDS stores below, and the wave waits for them there
    __builtin_amdgcn_sched_barrier(0);
    const float* sB = smem + cur * TILE_B;
    const float4* sW = swin + cur * BK;
#pragma unroll
    for (int g = 0; g < 2; ++g) {
      float4 bf[2];
#pragma unroll
      for (int i = 0; i < 2; ++i) bf[i] = frag(sB, wn * 32 + i * 16, g, lane);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float4 c = sW[16 * g + 4 * fq + j];
        float a[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const float dx = nx[i] - c.x, dy = ny[i] - c.y;
          const float d2 = fmaf(dx, dx, dy * dy);
          a[i] = c.z * __expf(-d2 * inv2s2);
          rs[i] += a[i];
        }
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
          for (int jj = 0; jj < 2; ++jj)
            acc[i][jj] = __builtin_amdgcn_mfma_f32_16x16x4f32(
                a[i], f4at(bf[jj], j), acc[i][jj], 0, 0, 0);
      }
    }
    // ... and their first use below them
    __builtin_amdgcn_sched_barrier(0);
    rb.store_cols(smem + (cur ^ 1) * TILE_B, t);
    swin[(cur ^ 1) * BK + tb] = rw;   // 8 threads per record, same value
    // the records of tile kt + 2 and the indices of tile kt + 3 stay in
    // flight over the next tile's MFMAs
    rw = record(kt + 2, ai);
    ai = index(kt + 3);
    __syncthreads();
    cur ^= 1;
  }

  // row sums: the 4 lane quads hold disjoint k of the same 16 neurons
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    rs[i] += __shfl_xor(rs[i], 16, 64);
    rs[i] += __shfl_xor(rs[i], 32, 64);
    if (wn == 0 && fq == 0) srs[wm * 64 + i * 16 + fr] = rs[i];
  }
  __syncthreads();

#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = wm * 64 + i * 16 + 4 * fq + r;
      const int n = m0 + row;
      if (n >= NN) continue;
      const float rn = srs[row];
      if constexpr (!DIRECT) {
        if (td == 0 && wn == 0 && fr == 0)
          ws[((long long)split * NN + n) * (D + 1) + D] = rn;
      }
#pragma unroll
      for (int jj = 0; jj < 2; ++jj) {
        const int d = d0 + wn * 32 + jj * 16 + fr;
        if (d >= D) continue;
        if constexpr (DIRECT) {
          float* p = W + (long long)n * D + d;
          const float w = *p;
          *p = fmaf(gmult, fmaf(-rn, w, acc[i][jj][r]), w);
        } else {
          ws[((long long)split * NN + n) * (D + 1) + d] = acc[i][jj][r];
        }
      }
    }
}

__global__ void __launch_bounds__(NTHR)
kohonen_update_finish(float* W, const float* __restrict__ ws, int NN, int D,
                      int splits, float gmult) {
  const long long e = (long long)blockIdx.x * NTHR + threadIdx.x;
  if (e >= (long long)NN * D) return;
  const long long n = e / D;
  const int d = (int)(e - n * D);
  const long long slice = (long long)NN * (D + 1);
  const float* p = ws + n * (D + 1);
  float dw = p[d], rn = p[D];
  for (int s = 1; s < splits; ++s) {
    dw += p[s * slice + d];
    rn += p[s * slice + D];
  }
  const float w = W[e];
  W[e] = fmaf(gmult, fmaf(-rn, w, dw), w);
}

inline bool aligned_to(const void* p, size_t a) {
  return ((uintptr_t)p & (a - 1)) == 0;
}

}  // namespace

// argmin[b] = argmin_n (|W[n]|^2 - 2 X[b].W[n]) (ties: lowest n), qerr[b] =
// max(0, |X[b]|^2 + that minimum), winners[argmin[b]] += 1.  X is [B][ldx]
// f32 or bf16, W is [NN][D] f32.  ws: (2 * splits + 1) * B 4-byte words.
// splits = 0: chosen here; > 0: forced (clamped to the neuron tile count).
HVK_API int hvk_kohonen_argmin(const void* X, int x_dt, const float* W, int B,
                               int NN, int D, int ldx, int* argmin,
                               float* qerr, int* winners, void* ws, int splits,
                               hipStream_t s) {
  if (!X || !W || !argmin || !ws || B < 1 || NN < 1 || D < 1 || ldx < D ||
      splits < 0 || (x_dt != HVK_F32 && x_dt != HVK_BF16))
    return -1;
  const int tb = (B + BX - 1) / BX, nt = (NN + BT - 1) / BT;
  int sp = splits > 0 ? splits : TARGET_WGS / tb;
  sp = sp < 1 ? 1 : sp > nt ? nt : sp;
  const int tps = (nt + sp - 1) / sp;
  sp = (nt + tps - 1) / tps;
  float* ws_val = (float*)ws;
  int* ws_idx = (int*)ws + (long long)sp * B;
  float* ws_x2 = (float*)ws + 2ll * sp * B;
  // 16-B chunks need every row of both operands on the 4-element grid
  const size_t xa = x_dt == HVK_F32 ? 16 : 8;
  const bool vec = aligned_to(W, 16) && aligned_to(X, xa) && D % 4 == 0 &&
                   ldx % 4 == 0;
  const dim3 grid((unsigned)tb, (unsigned)sp);
#define HVK_KOH_ARGMIN(XT, VEC)                                              \
  hipLaunchKernelGGL((kohonen_argmin_kernel<XT, VEC>), grid, dim3(NTHR), 0,  \
                     s, (const XT*)X, W, B, NN, D, ldx, ws_val, ws_idx,      \
                     ws_x2, tps, nt)
  if (x_dt == HVK_F32) {
    if (vec) HVK_KOH_ARGMIN(float, true);
    else HVK_KOH_ARGMIN(float, false);
  } else {
    if (vec) HVK_KOH_ARGMIN(uint16_t, true);
    else HVK_KOH_ARGMIN(uint16_t, false);
  }
#undef HVK_KOH_ARGMIN
  hipLaunchKernelGGL(kohonen_argmin_finish, dim3((unsigned)((B + NTHR - 1) /
                                                            NTHR)),
                     dim3(NTHR), 0, s, ws_val, ws_idx, ws_x2, B, NN, sp,
                     argmin, qerr, winners);
  return (int)launch_status(s);
}

// W[n] += gmult * sum_b G[b][n] (X[b] - W[n]) with G[b][n] = exp(-|coords[n]
// - coords[argmin[b]]|^2 * inv2sigma2), in place.  ws: splits * NN * (D + 1)
// floats (unused with one split).  splits = 0: chosen here; > 0: forced
// (clamped to the batch's K tile count).
HVK_API int hvk_kohonen_update(const void* X, int x_dt, float* W,
                               const float* coords, const int* argmin, int B,
                               int NN, int D, int ldx, float inv2sigma2,
                               float gmult, float* ws, int splits,
                               hipStream_t s) {
  if (!X || !W || !coords || !argmin || B < 1 || NN < 1 || D < 1 || ldx < D ||
      splits < 0 || (x_dt != HVK_F32 && x_dt != HVK_BF16))
    return -1;
  const int tiles_d = (D + BX - 1) / BX;
  const int tiles = ((NN + BT - 1) / BT) * tiles_d;
  const int nk = (B + BK - 1) / BK;
  int sp = splits;
  if (sp == 0) {
    sp = TARGET_WGS / tiles;
    if (sp > nk / 4) sp = nk / 4;
  }
  sp = sp < 1 ? 1 : sp > nk ? nk : sp;
  const int kps = (nk + sp - 1) / sp;
  sp = (nk + kps - 1) / kps;
  if (sp > 1 && !ws) return -1;
  const dim3 grid((unsigned)tiles, (unsigned)sp);
#define HVK_KOH_UPD(XT, DIRECT, VEC)                                         \
  hipLaunchKernelGGL((kohonen_update_kernel<XT, DIRECT, VEC>), grid,         \
                     dim3(NTHR), 0, s, (const XT*)X, W, coords, argmin, B,   \
                     NN, D, ldx, inv2sigma2, gmult, ws, kps, nk, tiles_d)
#define HVK_KOH_UPD2(XT, VEC)                                                \
  do {                                                                       \
    if (sp == 1) HVK_KOH_UPD(XT, true, VEC);                                 \
    else HVK_KOH_UPD(XT, false, VEC);                                        \
  } while (0)
  const size_t xa = x_dt == HVK_F32 ? 16 : 8;
  const bool vec = aligned_to(X, xa) && D % 4 == 0 && ldx % 4 == 0;
  if (x_dt == HVK_F32) {
    if (vec) HVK_KOH_UPD2(float, true);
    else HVK_KOH_UPD2(float, false);
  } else {
    if (vec) HVK_KOH_UPD2(uint16_t, true);
    else HVK_KOH_UPD2(uint16_t, false);
  }
#undef HVK_KOH_UPD2
#undef HVK_KOH_UPD
  if (sp > 1) {
    const long long n = (long long)NN * D;
    hipLaunchKernelGGL(kohonen_update_finish,
                       dim3((unsigned)((n + NTHR - 1) / NTHR)), dim3(NTHR), 0,
                       s, W, ws, NN, D, sp, gmult);
  }
  return (int)launch_status(s);
}
