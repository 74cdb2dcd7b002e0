// Kernels of the batch softmax loss (mhte_bsm_core.h: the formula, the deviation, the plan, the workspace).
//
//   bsm_prep_kernel        a wavefront per row: both operands' sum of squares and inv, Q^ / temperature and I^
//                          zero padded to kp, c_j, the diagonal z_ii as one fp32 row dot in a fixed order
//   bsm_row_kernel         a workgroup owns one row block of Q^ and one chunk of I^ tiles; forward: the (m, l)
//                          partial per row and chunk; gradient form: the chunk's partial of G . I^
//   bsm_col_kernel         the mirror image: a column block of I^ against a chunk of Q^ tiles, partial of G^T . Q^
//   bsm_final_kernel       one workgroup: the (m, l) partials merged in chunk order into lse_i, the loss summed in
//                          fp64 in a fixed order, rounded once
//   bsm_final_grad_kernel  a wavefront per row: the chunk partials added in chunk order, the normalisation
//                          backward, the upstream gradient
//
// Every product is v_mfma_f32_32x32x2_f32: exact fp32, an fmaf chain of k' terms in a fixed permuted order (lane
// half h fetches the four floats at 8t + 4h, so step e of group t adds the terms k = 8t + e and 8t + 4 + e: within
// each group of 8 the order is 0, 4, 1, 5, 2, 6, 3, 7; the same in every sweep).  The three sweeps are one body,
// bsm_sweep.  The tile product is taken TRANSPOSED, T = (streamed tile) . (owned block)^T, so that in the result
// (column on the lane, rows in the 16 registers) a lane holds 16 streamed elements of ONE owned row: the row's
// maximum and sum are in-lane work plus one exchange between the two lane halves at the end of the chunk, and the
// tile of G is at once the A operand of the second product, which sums over the streamed index: register reg of
// lane half h is k-slot h of step reg, the B operand reads the streamed tile's row bsm_acc_row(reg, h) from LDS.
// No accumulator tile moves between lanes.  The backward takes the tile product twice (once per gradient) by
// design: a single pass would need the G tile in both orientations and atomics or a second partial array of the
// other operand per row block.
//
// No atomics; plain loads and stores; every workspace index is below the plan's padded extents: the owned block
// and the streamed tile are read from arrays of bp rows (bp a multiple of the row block, the tiles end at or below
// it), user arrays (r) are read below B only, the partials have bp rows per chunk.
#ifndef MHTE_BSM_KERNELS_H_
#define MHTE_BSM_KERNELS_H_

#include "mhte_bsm_core.h"

namespace mhte {

typedef float bsm_f16 __attribute__((ext_vector_type(16)));

// the sum of v over the wavefront in a fixed order: every lane gets the same bits
__device__ __forceinline__ float bsm_wave_sum(float v) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d);
  return v;
}

struct BsmPrepArgs {
  const float* query;
  const float* item;
  const float* interval;
  float *inv_q, *inv_i, *ss_q, *ss_i, *c, *zd, *qs, *is;
  uint32_t B, bp;
  int k, kp, normalize;
  float temperature;
};

__global__ __launch_bounds__(256) void bsm_prep_kernel(BsmPrepArgs a) {
  const uint32_t row = blockIdx.x * 4u + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (row >= a.bp) return;
  const bool valid = row < a.B;
  float q[4], it[4];
  float sq = 0.f, si = 0.f;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const int kk = lane + 64 * e;
    const bool in = valid && kk < a.k;
    q[e] = in ? a.query[size_t(row) * a.k + kk] : 0.f;
    it[e] = in ? a.item[size_t(row) * a.k + kk] : 0.f;
    sq = fmaf(q[e], q[e], sq);
    si = fmaf(it[e], it[e], si);
  }
  sq = bsm_wave_sum(sq);
  si = bsm_wave_sum(si);
  const float invq = a.normalize ? bsm_inv(sq) : 1.f;
  const float invi = a.normalize ? bsm_inv(si) : 1.f;
  float d = 0.f;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const int kk = lane + 64 * e;
    const float x = (q[e] * invq) / a.temperature;
    const float y = it[e] * invi;
    d = fmaf(x, y, d);
    if (kk < a.kp) {
      a.qs[size_t(row) * a.kp + kk] = x;
      a.is[size_t(row) * a.kp + kk] = y;
    }
  }
  d = bsm_wave_sum(d);
  if (lane == 0) {
    const float c = valid ? bsm_c(a.interval[row]) : 0.f;
    a.inv_q[row] = invq;
    a.inv_i[row] = invi;
    a.ss_q[row] = sq;
    a.ss_i[row] = si;
    a.c[row] = c;
    a.zd[row] = d + c;
  }
}

struct BsmSweepArgs {
  const float* own;   // [bp][kp]: the operand whose block the workgroup owns (Q^ / T for a row sweep, I^ for col)
  const float* str;   // [bp][kp]: the streamed operand
  const float* c;     // [bp]
  const float* r;     // [B], the caller's
  const float* lse;   // [bp], rows below B written
  float* ml_m;        // [chunks][bp]
  float* ml_l;
  float* part;        // [chunks][bp][kp]
  uint32_t B, bp, tiles, tiles_per_chunk;
  int kp;
};

enum BsmMode : int { kBsmRowFwd = 0, kBsmRowGrad = 1, kBsmColGrad = 2 };

template <int MODE, int NB>
__device__ __forceinline__ void bsm_sweep(const BsmSweepArgs& a) {
  constexpr int RB = bsm_row_block(NB);
  constexpr int SMAX = NB * 32 + 4;
  __shared__ __attribute__((aligned(16))) float Os[RB * SMAX];
  __shared__ __attribute__((aligned(16))) float Ts[kBsmTile * SMAX];
  __shared__ float sa[kBsmTile];
  __shared__ float sb[kBsmTile];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, li = lane & 31, h = lane >> 5;
  const int kp = a.kp, stride = kp + 4, kq = kp >> 2;
  const uint32_t row0 = blockIdx.x * uint32_t(RB), chunk = blockIdx.y;
  const uint32_t gi = row0 + uint32_t(32 * w + li);   // the owned row of this lane (< bp)

  for (int e = tid; e < RB * kq; e += 2 * RB) {
    const int rr = e / kq, qd = e - rr * kq;
    *reinterpret_cast<float4*>(Os + rr * stride + 4 * qd) =
        *reinterpret_cast<const float4*>(a.own + size_t(row0 + uint32_t(rr)) * kp + 4 * qd);
  }
  float o_a = 0.f, o_b = 0.f;   // row gradient: lse_i, r_i;  col: c_j
  if (MODE == kBsmRowGrad) {
    o_a = gi < a.B ? a.lse[gi] : 0.f;
    o_b = gi < a.B ? a.r[gi] : 0.f;
  } else if (MODE == kBsmColGrad) {
    o_a = a.c[gi];
  }
  BsmML ml = bsm_empty();
  bsm_f16 dacc[NB];
#pragma unroll
  for (int nb = 0; nb < NB; ++nb)
#pragma unroll
    for (int r = 0; r < 16; ++r) dacc[nb][r] = 0.f;

  const uint32_t t0 = chunk * a.tiles_per_chunk;
  const uint32_t t1 = t0 + a.tiles_per_chunk < a.tiles ? t0 + a.tiles_per_chunk : a.tiles;
  for (uint32_t t = t0; t < t1; ++t) {
    const uint32_t s0 = t * uint32_t(kBsmTile);   // s0 + 31 < bp
    __syncthreads();   // the previous tile is read (and, the first time, nothing is pending)
    for (int e = tid; e < kBsmTile * kq; e += 2 * RB) {
      const int rr = e / kq, qd = e - rr * kq;
      *reinterpret_cast<float4*>(Ts + rr * stride + 4 * qd) =
          *reinterpret_cast<const float4*>(a.str + size_t(s0 + uint32_t(rr)) * kp + 4 * qd);
    }
    if (tid < kBsmTile) {
      const uint32_t gs = s0 + uint32_t(tid);
      if (MODE == kBsmColGrad) {   // the streamed index is the row i: lse_i (+inf beyond B: exp gives 0), r_i
        sa[tid] = gs < a.B ? a.lse[gs] : INFINITY;
        sb[tid] = gs < a.B ? a.r[gs] : 0.f;
      } else {                     // the streamed index is the column j: c_j, -inf beyond B (the mask)
        sa[tid] = gs < a.B ? a.c[gs] : -INFINITY;
      }
    }
    __syncthreads();

    bsm_f16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    const float* ap = Ts + li * stride + 4 * h;
    const float* bp = Os + (32 * w + li) * stride + 4 * h;
    for (int kk = 0; kk < kp; kk += 8) {
      const float4 x = *reinterpret_cast<const float4*>(ap + kk);
      const float4 y = *reinterpret_cast<const float4*>(bp + kk);
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(x.x, y.x, acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(x.y, y.y, acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(x.z, y.z, acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(x.w, y.w, acc, 0, 0, 0);
    }

    if (MODE == kBsmRowFwd) {
      float z[16];
      float tmax = -INFINITY;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        z[r] = acc[r] + sa[bsm_acc_row(r, h)];
        tmax = fmaxf(tmax, z[r]);
      }
      if (tmax > -INFINITY) {
        const float mn = fmaxf(ml.m, tmax);
        float s = 0.f;
#pragma unroll
        for (int r = 0; r < 16; ++r) s += expf(z[r] - mn);
        ml.l = ml.l * expf(ml.m - mn) + s;
        ml.m = mn;
      }
    } else {
      float g[16];
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int j = bsm_acc_row(r, h);
        const float delta = gi == s0 + uint32_t(j) ? 1.f : 0.f;
        if (MODE == kBsmRowGrad)
          g[r] = o_b * (expf((acc[r] + sa[j]) - o_a) - delta);
        else
          g[r] = sb[j] * (expf((acc[r] + o_a) - sa[j]) - delta);
      }
#pragma unroll
      for (int nb = 0; nb < NB; ++nb) {
        if (nb * 32 < kp) {
          const int n = nb * 32 + li < kp ? nb * 32 + li : kp - 1;   // (columns at and beyond kp are not stored)
          const float* tp = Ts + n;
#pragma unroll
          for (int r = 0; r < 16; ++r)
            dacc[nb] = __builtin_amdgcn_mfma_f32_32x32x2f32(g[r], tp[bsm_acc_row(r, h) * stride], dacc[nb], 0, 0, 0);
        }
      }
    }
  }

  if (MODE == kBsmRowFwd) {
    BsmML other;
    other.m = __shfl_xor(ml.m, 32);
    other.l = __shfl_xor(ml.l, 32);
    if (h == 0) {
      const BsmML both = bsm_merge(ml, other);
      a.ml_m[size_t(chunk) * a.bp + gi] = both.m;
      a.ml_l[size_t(chunk) * a.bp + gi] = both.l;
    }
  } else {
#pragma unroll
    for (int nb = 0; nb < NB; ++nb) {
      const int n = nb * 32 + li;
      if (n < kp) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const uint32_t row = row0 + uint32_t(32 * w + bsm_acc_row(r, h));
          a.part[(size_t(chunk) * a.bp + row) * kp + n] = dacc[nb][r];
        }
      }
    }
  }
}

template <bool GRAD, int NB>
__global__ __launch_bounds__(2 * bsm_row_block(NB)) void bsm_row_kernel(BsmSweepArgs a) {
  bsm_sweep<GRAD ? kBsmRowGrad : kBsmRowFwd, NB>(a);
}
template <int NB>
__global__ __launch_bounds__(2 * bsm_row_block(NB)) void bsm_col_kernel(BsmSweepArgs a) {
  bsm_sweep<kBsmColGrad, NB>(a);
}

struct BsmFinalArgs {
  const float* ml_m;
  const float* ml_l;
  const float* zd;
  const float* r;
  float* lse;
  float* loss;   // or null
  uint32_t B, bp, chunks;
};

__global__ __launch_bounds__(kBsmFinalThreads) void bsm_final_kernel(BsmFinalArgs a) {
  __shared__ double sh[kBsmFinalThreads];
  const uint32_t tid = threadIdx.x;
  double sum = 0.0;
  for (uint32_t i = tid; i < a.B; i += uint32_t(kBsmFinalThreads)) {
    BsmML x{a.ml_m[i], a.ml_l[i]};
    for (uint32_t c = 1; c < a.chunks; ++c)
      x = bsm_merge(x, BsmML{a.ml_m[size_t(c) * a.bp + i], a.ml_l[size_t(c) * a.bp + i]});
    const float lse = bsm_lse(x);
    a.lse[i] = lse;
    if (a.loss) sum += double(a.r[i]) * (double(a.zd[i]) - double(lse));
  }
  if (!a.loss) return;   // (uniform)
  sh[tid] = sum;
  __syncthreads();
  for (uint32_t d = uint32_t(kBsmFinalThreads) / 2; d >= 1; d >>= 1) {
    if (tid < d) sh[tid] += sh[tid + d];
    __syncthreads();
  }
  if (tid == 0) *a.loss = bsm_pos_zero(-float(sh[0]));
}

struct BsmFinalGradArgs {
  const float* x[2];      // query, item: the caller's
  const float* part[2];   // [chunks][bp][kp]
  const float* inv[2];
  const float* ss[2];
  float* out[2];          // dquery, ditem; either may be null
  const float* grad_dev;
  float grad, temperature;
  uint32_t B, bp, chunks;
  int k, kp, normalize;
};

__global__ __launch_bounds__(256) void bsm_final_grad_kernel(BsmFinalGradArgs a) {
  const int op = blockIdx.y;
  float* out = a.out[op];
  const uint32_t row = blockIdx.x * 4u + (threadIdx.x >> 6);
  if (!out || row >= a.B) return;
  const int lane = threadIdx.x & 63;
  const float up = a.grad_dev ? *a.grad_dev : a.grad;
  const float inv = a.inv[op][row];
  float g[4], xh[4];
  float dot = 0.f;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const int kk = lane + 64 * e;
    g[e] = 0.f;
    xh[e] = 0.f;
    if (kk < a.k) {
      float s = a.part[op][size_t(row) * a.kp + kk];
      for (uint32_t c = 1; c < a.chunks; ++c) s += a.part[op][(size_t(c) * a.bp + row) * a.kp + kk];
      g[e] = op == 0 ? s / a.temperature : s;
      xh[e] = a.x[op][size_t(row) * a.k + kk] * inv;
    }
    dot = fmaf(xh[e], g[e], dot);
  }
  dot = bsm_wave_sum(dot);
  const bool eps = bsm_eps_branch(a.ss[op][row]);
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const int kk = lane + 64 * e;
    if (kk < a.k) {
      const float dx = a.normalize ? bsm_dx(g[e], xh[e], dot, inv, eps) : g[e];
      out[size_t(row) * a.k + kk] = bsm_pos_zero(dx * up);
    }
  }
}

}  // namespace mhte
#endif  // MHTE_BSM_KERNELS_H_
