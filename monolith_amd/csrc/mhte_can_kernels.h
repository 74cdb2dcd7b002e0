// Kernels of the CAN co-action unit (mhte_can_core.h: the formulas, the limits, the index map, the plan).
//
// A workgroup is one wavefront and owns ONE sample: it stages the sample's item row once into LDS (W_i zero padded to
// PD x PD with a row stride of PD + 1 floats, then b_i), walks the sample's row tiles (PD rows, lane = row) in
// ascending order and keeps every sum of the sample in its own registers.  PD is 16 (v_mfma_f32_16x16x4_f32) or 32
// (v_mfma_f32_32x32x2_f32); a lane is (lr, q) = (lane % PD, lane / PD) and holds NR = PD PD / 64 values of a tile.
//
// Every product is taken transposed, h_{i+1}^T = W_i^T h_i^T: A = W_i^T (lane lr = output column, read from LDS
// down a column of W_i), B = h_i^T (lane lr = row).  The accumulator then holds in lane (row, q), register r, the
// output column can_kidx(r, q); with the reduction index of k-slot q at step s ALSO can_kidx(s, q), register s of a
// layer's accumulator is step s of the next layer's B operand.  The MLP chains in registers: no transposition and
// no barrier between layers.  The bias is the accumulator's initial value, the activation a select in registers.
//   can_fwd_kernel   the chain per tile, then the sum over T: the tile of h_L goes through LDS once ([row][column]),
//                    lane j < d of lane group 0 adds its column down the tile's rows in ascending order, writes a
//                    feature when its last row is met and carries an unfinished feature into the next tile; padding
//                    rows are never read.  T == 1 has no sum: h_L is stored from the registers.
//   can_bwd_kernel   recomputes h_1 .. h_L of the tile into registers, starts from dh_L = dout[b, f(row)] (0 on a
//                    padding row, which keeps every padding row out of every sum) and walks the layers down:
//                    dpre = dh masked by h_{i+1} > 0;  dh_i^T = W_i dpre^T with A = W_i as stored (lane lr = k, read
//                    along a row) and B = dpre's registers: the same chaining.  dW_i = h_i^T dpre reduces over rows,
//                    the lane index: h_i and dpre go through LDS ([row][column]) and come back as A (lane lr = k) and
//                    B (lane lr = j) of one more MFMA chain whose accumulator, kept over the sample's tiles, is
//                    dW_i[can_kidx(r, q)][lr]; db_i is the same B against A = 1 in row 0.  ditem is written once per
//                    sample, in runs of d floats; duser once per tile.  Either half is skipped when not asked for.
// The barriers are __syncthreads() of a 64-thread workgroup: wavefront-local.
//
// No atomics; plain loads and stores; every user array is read and written below its extent only.
#ifndef MHTE_CAN_KERNELS_H_
#define MHTE_CAN_KERNELS_H_

#include "mhte_can_core.h"
#include "mhte_cin_kernels.h"

namespace mhte {

typedef float can_f4 __attribute__((ext_vector_type(4)));

template <int PD> struct CanAcc;
template <> struct CanAcc<16> { typedef can_f4 type; };
template <> struct CanAcc<32> { typedef cin_f16 type; };

struct CanArgs {
  const float* user;   // [B, R, d]
  const float* item;   // [B, P]
  const float* dout;   // [B, F, d]
  float* out;          // [B, F, d]
  float* duser;        // or null
  float* ditem;        // or null
  int64_t P;
  int R, T, d, L, act;
};

template <int PD>
__device__ __forceinline__ typename CanAcc<PD>::type can_mfma(float av, float bv, typename CanAcc<PD>::type c) {
  if constexpr (PD == 16)
    return __builtin_amdgcn_mfma_f32_16x16x4f32(av, bv, c, 0, 0, 0);
  else
    return __builtin_amdgcn_mfma_f32_32x32x2f32(av, bv, c, 0, 0, 0);
}

// the sample's item row into LDS: Ws [L][PD][PD + 1] zero padded, Bs [L][PD] zero padded; lanes read runs of d floats
template <int PD>
__device__ __forceinline__ void can_stage(const CanArgs& a, const float* item, float* Ws, float* Bs, int lane) {
  const int d = a.d, per = d * (d + 1);
  for (int e = lane; e < a.L * PD * PD; e += 64) {
    const int i = e / (PD * PD), k = (e / PD) % PD, j = e % PD;
    Ws[(i * PD + k) * (PD + 1) + j] = k < d && j < d ? item[i * per + k * d + j] : 0.f;
  }
  for (int e = lane; e < a.L * PD; e += 64) {
    const int i = e / PD, j = e % PD;
    Bs[e] = j < d ? item[i * per + d * d + j] : 0.f;
  }
}

// one layer: act(W_i^T h^T + b_i) in the accumulator layout, which is the operand layout
template <int PD>
__device__ __forceinline__ typename CanAcc<PD>::type can_layer(const float* Wi, const float* Bi,
                                                               typename CanAcc<PD>::type h, int lr, int q, int act) {
  constexpr int NR = PD * PD / 64, WS = PD + 1;
  typename CanAcc<PD>::type acc;
#pragma unroll
  for (int r = 0; r < NR; ++r) acc[r] = Bi[can_kidx<PD>(r, q)];
#pragma unroll
  for (int s = 0; s < NR; ++s) acc = can_mfma<PD>(Wi[can_kidx<PD>(s, q) * WS + lr], h[s], acc);
  if (act) {
#pragma unroll
    for (int r = 0; r < NR; ++r) acc[r] = acc[r] > 0.f ? acc[r] : 0.f;
  }
  return acc;
}

// the tile's rows of user (or a gradient's target) as this lane sees them: row rg, columns can_kidx(s, q)
template <int PD>
__device__ __forceinline__ typename CanAcc<PD>::type can_load_rows(const float* p, bool rok, int d, int q) {
  constexpr int NR = PD * PD / 64;
  typename CanAcc<PD>::type h;
#pragma unroll
  for (int s = 0; s < NR; ++s) {
    const int k = can_kidx<PD>(s, q);
    h[s] = rok && k < d ? p[k] : 0.f;
  }
  return h;
}

template <int PD>
__global__ __launch_bounds__(64) void can_fwd_kernel(CanArgs a) {
  constexpr int NR = PD * PD / 64, WS = PD + 1;
  typedef typename CanAcc<PD>::type V;
  extern __shared__ float can_lds[];
  float* Ws = can_lds;
  float* Bs = Ws + a.L * PD * WS;
  float* Ts = Bs + a.L * PD;   // [row][column]: the tile of h_L
  const int lane = threadIdx.x, lr = lane % PD, q = lane / PD, d = a.d;
  const int64_t b = blockIdx.x;
  can_stage<PD>(a, a.item + b * a.P, Ws, Bs, lane);
  __syncthreads();
  const float* up = a.user + b * a.R * d;
  float* op = a.out + b * (a.R / a.T) * d;
  float run = 0.f;   // lane j < d of group 0: the unfinished feature's sum of column j
  for (int r0 = 0; r0 < a.R; r0 += PD) {
    const int rg = r0 + lr;
    const bool rok = rg < a.R;
    V h = can_load_rows<PD>(up + int64_t(rok ? rg : 0) * d, rok, d, q);
    for (int i = 0; i < a.L; ++i) h = can_layer<PD>(Ws + i * PD * WS, Bs + i * PD, h, lr, q, a.act);
    if (a.T == 1) {   // (uniform) out = h_L
#pragma unroll
      for (int s = 0; s < NR; ++s) {
        const int k = can_kidx<PD>(s, q);
        if (rok && k < d) op[int64_t(rg) * d + k] = h[s] + 0.f;
      }
      continue;
    }
    __syncthreads();   // the previous tile is read
#pragma unroll
    for (int s = 0; s < NR; ++s) Ts[lr * WS + can_kidx<PD>(s, q)] = h[s];
    __syncthreads();
    if (q == 0 && lr < d) {
      const int n = a.R - r0 < PD ? a.R - r0 : PD;
      int f = r0 / a.T, t = r0 - f * a.T;
      for (int r = 0; r < n; ++r) {
        run += Ts[r * WS + lr];
        if (++t == a.T) {
          op[int64_t(f) * d + lr] = run + 0.f;
          run = 0.f, t = 0, ++f;
        }
      }
    }
  }
}

template <int PD, int LC>
__global__ __launch_bounds__(64) void can_bwd_kernel(CanArgs a) {
  constexpr int NR = PD * PD / 64, WS = PD + 1;
  typedef typename CanAcc<PD>::type V;
  extern __shared__ float can_lds[];
  float* Ws = can_lds;
  float* Bs = Ws + a.L * PD * WS;
  float* Hs = Bs + a.L * PD;   // [row][k]: the tile of h_i
  float* Ds = Hs + PD * WS;    // [row][j]: the tile of dpre_i
  const int lane = threadIdx.x, lr = lane % PD, q = lane / PD, d = a.d;
  const int64_t b = blockIdx.x;
  can_stage<PD>(a, a.item + b * a.P, Ws, Bs, lane);
  __syncthreads();
  const float* up = a.user + b * a.R * d;
  const float* gp = a.dout + b * (a.R / a.T) * d;
  const float one = lr == 0 ? 1.f : 0.f;   // A of the bias gradient: row 0 sums the tile's rows
  V dw[LC];
  float db[LC];
#pragma unroll
  for (int i = 0; i < LC; ++i) {
    db[i] = 0.f;
#pragma unroll
    for (int r = 0; r < NR; ++r) dw[i][r] = 0.f;
  }
  for (int r0 = 0; r0 < a.R; r0 += PD) {
    const int rg = r0 + lr;
    const bool rok = rg < a.R;
    V h[LC + 1];
    h[0] = can_load_rows<PD>(up + int64_t(rok ? rg : 0) * d, rok, d, q);
#pragma unroll
    for (int i = 0; i < LC; ++i)
      if (i < a.L) h[i + 1] = can_layer<PD>(Ws + i * PD * WS, Bs + i * PD, h[i], lr, q, a.act);
    V dh = can_load_rows<PD>(gp + int64_t(rok ? rg / a.T : 0) * d, rok, d, q);
#pragma unroll
    for (int i = LC - 1; i >= 0; --i) {
      if (i >= a.L) continue;   // (uniform)
      V dp = dh;
      if (a.act) {
#pragma unroll
        for (int r = 0; r < NR; ++r) dp[r] = h[i + 1][r] > 0.f ? dh[r] : 0.f;
      }
      if (a.ditem) {
        __syncthreads();   // the previous layer's tiles are read
#pragma unroll
        for (int s = 0; s < NR; ++s) {
          Hs[lr * WS + can_kidx<PD>(s, q)] = h[i][s];
          Ds[lr * WS + can_kidx<PD>(s, q)] = dp[s];
        }
        __syncthreads();
        V sum;
#pragma unroll
        for (int r = 0; r < NR; ++r) sum[r] = 0.f;
#pragma unroll
        for (int s = 0; s < NR; ++s) {
          const int row = can_kidx<PD>(s, q);
          const float dv = Ds[row * WS + lr];
          dw[i] = can_mfma<PD>(Hs[row * WS + lr], dv, dw[i]);
          sum = can_mfma<PD>(one, dv, sum);
        }
        db[i] += sum[0];   // (lane group 0: register 0 is row 0)
      }
      if (i > 0 || a.duser) {
        const float* Wi = Ws + (i * PD + lr) * WS;
#pragma unroll
        for (int r = 0; r < NR; ++r) dh[r] = 0.f;
#pragma unroll
        for (int s = 0; s < NR; ++s) dh = can_mfma<PD>(Wi[can_kidx<PD>(s, q)], dp[s], dh);
      }
    }
    if (a.duser) {
#pragma unroll
      for (int s = 0; s < NR; ++s) {
        const int k = can_kidx<PD>(s, q);
        if (rok && k < d) a.duser[(b * a.R + rg) * d + k] = dh[s] + 0.f;
      }
    }
  }
  if (!a.ditem || lr >= d) return;
  float* ip = a.ditem + b * a.P;
  const int per = d * (d + 1);
#pragma unroll
  for (int i = 0; i < LC; ++i) {
    if (i >= a.L) continue;
#pragma unroll
    for (int r = 0; r < NR; ++r) {
      const int k = can_kidx<PD>(r, q);
      if (k < d) ip[i * per + k * d + lr] = dw[i][r] + 0.f;
    }
    if (q == 0) ip[i * per + d * d + lr] = db[i] + 0.f;
  }
}

}  // namespace mhte
#endif  // MHTE_CAN_KERNELS_H_
