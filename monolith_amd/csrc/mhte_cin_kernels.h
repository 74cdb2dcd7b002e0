// Kernels of the CIN layer (mhte_cin_core.h: the formulas, the limits, the plan).
//
//   cin_fwd_kernel       a workgroup owns 128 GEMM rows (whole b's) against 32 col_tiles columns of U; a wavefront
//                        owns one 32-row tile and col_tiles accumulator tiles.  The x0 slab of the block stays in
//                        LDS; per K chunk the xl values and the weight rows are staged.  A lane holds one row and
//                        one k-slot of a step: lane half 0 the even j, half 1 the odd j; A = xl[r, h] * x0[r, j] is
//                        one multiply, used for every column tile.  Epilogue per column tile through LDS: bias,
//                        activation, xnext in runs along d, pooled as the sum over d ascending.
//   cin_dx_kernel        a wavefront owns 32 rows and keeps their g in registers as the B operand; the tile product
//                        is taken transposed, T = w[k tile] . g^T, so a lane holds 16 k-values of ONE row (as
//                        bsm_sweep does).  dxl: in-lane sums per h, carried across tiles, the two lane halves added
//                        (half 0 + half 1) when an h is complete.  dx0: per lane-half accumulators in LDS, added in
//                        the same order at the end.
//   cin_dw_kernel        a workgroup owns 128 K rows (K row H m is the bias gradient: z = 1) against 32 col_tiles
//                        columns over one slab of rows; per 32-row chunk g, x0 and the needed xl columns are staged
//                        in LDS, z is formed by the lane that owns the K row.
//   cin_slab_sum_kernel  the slab partials added in slab order (fi_slab_sum)
//   cin_zero_kernel      +0 into dw / dbias for B == 0
//
// No atomics; plain loads and stores; every user array is read and written below its extent only.
#ifndef MHTE_CIN_KERNELS_H_
#define MHTE_CIN_KERNELS_H_

#include "mhte_cin_core.h"

namespace mhte {

typedef float cin_f16 __attribute__((ext_vector_type(16)));

constexpr int kCinWS = 160;    // floats between two staged weight rows of the forward: the lane halves on other banks
constexpr int kCinES = 129;    // ... between two columns of the forward's epilogue tile
constexpr int kCinGS = 161;    // ... between two staged g rows of the weight gradient
constexpr int kCinXS = 65;     // ... x0 rows
constexpr int kCinLS = 131;    // ... xl rows: at most 128 / m + 2 <= 130 columns of xl meet one block of 128 K rows
constexpr int kCinTS = 132;    // ... between two weight rows of the input gradient's tile (float4 reads)

struct CinFwdArgs {
  const float* x0;
  const float* xl;
  const float* w;
  const float* bias;
  float* xnext;   // or null
  float* pooled;
  int64_t B;
  int m, D, H, U, act, bpb, mp2, hc, jc, parts;
};

template <int NT, int MP>
__global__ __launch_bounds__(256) void cin_fwd_kernel(CinFwdArgs a) {
  __shared__ float X0s[MP * kCinRowBlock];   // [j][row], the row rotated by 32 for odd j
  __shared__ float Ws[2 * kCinSteps * kCinWS];
  __shared__ float XLs[kCinSteps * kCinRowBlock];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, li = lane & 31, h = lane >> 5;
  const int64_t b0 = int64_t(blockIdx.x) * a.bpb;
  const int c0 = int(blockIdx.y) * (NT * kCinTile);
  const int rows = a.bpb * a.D;   // the rows of the block that belong to a b

  for (int e = tid; e < 2 * a.mp2 * kCinRowBlock; e += 256) {
    const int j = e >> 7, lr = e & 127;
    float v = 0.f;
    if (j < a.m && lr < rows) {
      const int bl = lr / a.D, d = lr - bl * a.D;
      if (b0 + bl < a.B) v = a.x0[((b0 + bl) * a.m + j) * a.D + d];
    }
    X0s[j * kCinRowBlock + ((lr + 32 * (j & 1)) & 127)] = v;
  }
  // the row this thread stages xl for, and the column and k-slot it stages weights for
  const int lr_s = tid & 127, half_s = tid >> 7;
  const int bl_s = lr_s / a.D, d_s = lr_s - bl_s * a.D;
  const bool valid_s = lr_s < rows && b0 + bl_s < a.B;
  const float* xlp = a.xl + (valid_s ? ((b0 + bl_s) * a.H) * a.D + d_s : 0);
  const bool col_s = lr_s < NT * kCinTile && c0 + lr_s < a.U;
  const int lrw = 32 * w + li;

  cin_f16 acc[NT];
#pragma unroll
  for (int nt = 0; nt < NT; ++nt)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[nt][r] = 0.f;

  for (int hh0 = 0; hh0 < a.H; hh0 += a.hc) {
    const int nh = a.H - hh0 < a.hc ? a.H - hh0 : a.hc;
    for (int p = 0; p < a.parts; ++p) {
      const int jp0 = p * kCinSteps;
      const int nj = a.mp2 - jp0 < a.jc ? a.mp2 - jp0 : a.jc;
      __syncthreads();   // the previous chunk is read (the first time: the x0 slab is written)
      for (int hl = half_s; hl < nh; hl += 2) XLs[hl * kCinRowBlock + lr_s] = valid_s ? xlp[int64_t(hh0 + hl) * a.D] : 0.f;
      {
        int hl = 0, jl = 0;
        for (int sl = 0; sl < nh * nj; ++sl) {
          const int j = 2 * (jp0 + jl) + half_s;
          float v = 0.f;
          if (col_s && j < a.m) v = a.w[(int64_t(hh0 + hl) * a.m + j) * a.U + c0 + lr_s];
          Ws[(2 * sl + half_s) * kCinWS + lr_s] = v;
          if (++jl == nj) jl = 0, ++hl;
        }
      }
      __syncthreads();
      for (int hl = 0; hl < nh; ++hl) {
        const float xv = XLs[hl * kCinRowBlock + lrw];
        for (int jl = 0; jl < nj; ++jl) {
          const int j = 2 * (jp0 + jl) + h;
          const float av = xv * X0s[j * kCinRowBlock + ((lrw + 32 * h) & 127)];
          const float* bp = Ws + (2 * (hl * nj + jl) + h) * kCinWS + li;
#pragma unroll
          for (int nt = 0; nt < NT; ++nt)
            acc[nt] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, bp[nt * kCinTile], acc[nt], 0, 0, 0);
        }
      }
    }
  }

  float* Es = Ws;   // [column][row] of one column tile: 32 * 129 floats
#pragma unroll
  for (int nt = 0; nt < NT; ++nt) {
    const int ct = c0 + nt * kCinTile;
    const int ncols = a.U - ct < kCinTile ? a.U - ct : kCinTile;
    if (ncols <= 0) break;   // (uniform)
    __syncthreads();   // the chunk, or the previous column tile, is read
    const float bv = li < ncols ? a.bias[ct + li] : 0.f;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      float v = acc[nt][r] + bv;
      if (a.act) v = v > 0.f ? v : 0.f;
      Es[li * kCinES + 32 * w + cin_acc_row(r, h)] = v;
    }
    __syncthreads();
    if (a.xnext) {   // for one b the tile's columns are ncols * D consecutive floats of xnext
      const int per_b = ncols * a.D;
      for (int e = tid; e < a.bpb * per_b; e += 256) {
        const int bl = e / per_b, rem = e - bl * per_b;
        const int c = rem / a.D, d = rem - c * a.D;
        if (b0 + bl < a.B) a.xnext[((b0 + bl) * a.U + ct) * a.D + rem] = Es[c * kCinES + bl * a.D + d];
      }
    }
    for (int t = tid; t < a.bpb * ncols; t += 256) {
      const int bl = t / ncols, c = t - bl * ncols;
      if (b0 + bl < a.B) {
        const float* ep = Es + c * kCinES + bl * a.D;
        float s = 0.f;
        for (int d = 0; d < a.D; ++d) s += ep[d];
        a.pooled[(b0 + bl) * a.U + ct + c] = s;
      }
    }
  }
}

struct CinGradArgs {
  const float* dxnext;   // [B, U, D] or null
  const float* dpooled;  // [B, U]
  const float* x0;
  const float* xl;
  const float* w;
  const float* xnext;    // [B, U, D], read with relu only
  float* dx0;            // or null
  float* dxl;            // or null
  float* dw;             // or null
  float* dbias;          // or null
  float* part;           // [slabs][H m + 1][U], or null with one slab
  int64_t R, slab_rows;  // R = B D
  int m, D, H, U, K, act;
};

// g[r, u] of a row below R
__device__ __forceinline__ float cin_g(const CinGradArgs& a, int64_t b, int d, int u) {
  const int64_t i = (b * a.U + u) * a.D + d;
  float g = a.dpooled[b * a.U + u];
  if (a.dxnext) g = a.dxnext[i] + g;
  if (a.act) g = a.xnext[i] > 0.f ? g : 0.f;
  return g;
}

template <int MP, int WAVES>
__global__ __launch_bounds__(64 * WAVES) void cin_dx_kernel(CinGradArgs a) {
  constexpr int THREADS = 64 * WAVES;
  __shared__ __attribute__((aligned(16))) float Wt[kCinTile * kCinTS];
  __shared__ int kmap[kCinTile];
  __shared__ float DA[WAVES * 2 * MP * kCinTile];   // [wavefront][lane half][j][row]: the partials of dx0
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, li = lane & 31, h = lane >> 5;
  const int64_t r = int64_t(blockIdx.x) * (kCinTile * WAVES) + 32 * w + li;
  const bool valid = r < a.R;
  const int64_t b = valid ? r / a.D : 0;
  const int d = valid ? int(r - b * a.D) : 0;
  const int nub = (a.U + 127) >> 7, tiles = (a.K + kCinTile - 1) / kCinTile;
  float* da = DA + (w * 2 + h) * MP * kCinTile + li;
  for (int j = 0; j < MP; ++j) da[j * kCinTile] = 0.f;

  float gq[64];   // g[r, ub 128 + 8 t + 4 h + e] at [4 t + e]: the k-slots of this lane half
  auto load_g = [&](int ub) {
#pragma unroll
    for (int q = 0; q < 64; ++q) {
      const int u = ub * 128 + 8 * (q >> 2) + 4 * h + (q & 3);
      gq[q] = valid && u < a.U ? cin_g(a, b, d, u) : 0.f;
    }
  };
  if (nub == 1) load_g(0);

  int cur_hh = -1;
  float s = 0.f;
  for (int t = 0; t < tiles; ++t) {
    const int k0 = t * kCinTile;
    cin_f16 acc;
#pragma unroll
    for (int q = 0; q < 16; ++q) acc[q] = 0.f;
    for (int ub = 0; ub < nub; ++ub) {
      __syncthreads();   // the previous tile and its kmap are read
      for (int e = tid; e < kCinTile * 128; e += THREADS) {
        const int kl = e >> 7, ul = e & 127;
        const int k = k0 + kl, u = ub * 128 + ul;
        Wt[kl * kCinTS + ul] = k < a.K && u < a.U ? a.w[int64_t(k) * a.U + u] : 0.f;
      }
      if (ub == 0 && tid < kCinTile) {
        const int k = k0 + tid;
        kmap[tid] = k < a.K ? (((k / a.m) << 8) | (k % a.m)) : -1;
      }
      if (nub > 1) load_g(ub);
      __syncthreads();
      const float* ap = Wt + li * kCinTS + 4 * h;
#pragma unroll
      for (int t8 = 0; t8 < 16; ++t8) {
        const float4 x = *reinterpret_cast<const float4*>(ap + 8 * t8);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(x.x, gq[4 * t8 + 0], acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(x.y, gq[4 * t8 + 1], acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(x.z, gq[4 * t8 + 2], acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(x.w, gq[4 * t8 + 3], acc, 0, 0, 0);
      }
    }
    // acc[q] = dz[r, k0 + cin_acc_row(q, h)]: the in-lane part
    float tx[16];
    int hr[16];
#pragma unroll
    for (int q = 0; q < 16; ++q) {
      const int pk = kmap[cin_acc_row(q, h)];
      const bool ok = pk >= 0 && valid;
      const int hh = ok ? pk >> 8 : 0, j = ok ? pk & 255 : 0;
      const float x0v = ok ? a.x0[(b * a.m + j) * a.D + d] : 0.f;
      const float xlv = ok ? a.xl[(b * a.H + hh) * a.D + d] : 0.f;
      tx[q] = acc[q] * x0v;
      hr[q] = pk >= 0 ? pk >> 8 : -1;
      if (ok && a.dx0) da[j * kCinTile] += acc[q] * xlv;
    }
    if (a.dxl) {
      const int kend = k0 + kCinTile < a.K ? k0 + kCinTile : a.K;
      const int hh_last = (kend - 1) / a.m;
      for (int hq = k0 / a.m; hq <= hh_last; ++hq) {
        float v = 0.f;
#pragma unroll
        for (int q = 0; q < 16; ++q) v = hr[q] == hq ? v + tx[q] : v;
        if (hq == cur_hh) {
          s += v;
        } else {
          s = v;
          cur_hh = hq;
        }
        if ((hq + 1) * a.m <= kend) {   // every k of this h is summed: half 0 + half 1
          const float o = __shfl_xor(s, 32);
          const float tot = h == 0 ? s + o : o + s;
          if (h == 0 && valid) a.dxl[(b * a.H + hq) * a.D + d] = tot + 0.f;
        }
      }
    }
  }
  if (a.dx0) {
    __syncthreads();
    const float* d0 = DA + (w * 2) * MP * kCinTile + li;
    for (int j = h; j < a.m; j += 2)
      if (valid) a.dx0[(b * a.m + j) * a.D + d] = (d0[j * kCinTile] + d0[(MP + j) * kCinTile]) + 0.f;
  }
}

template <int NT>
__global__ __launch_bounds__(256) void cin_dw_kernel(CinGradArgs a) {
  __shared__ float Gs[kCinTile * kCinGS];
  __shared__ float X0s[kCinTile * kCinXS];
  __shared__ float XLs[kCinTile * kCinLS];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, li = lane & 31, h = lane >> 5;
  const int k0 = int(blockIdx.x) * kCinRowBlock, c0 = int(blockIdx.y) * (NT * kCinTile);
  const int64_t r_lo = int64_t(blockIdx.z) * a.slab_rows;
  const int64_t r_hi = r_lo + a.slab_rows < a.R ? r_lo + a.slab_rows : a.R;
  const int kw = k0 + 32 * w + li;   // the K row of this lane: z[., kw] is its A operand
  const bool is_bias = kw == a.K, is_k = kw < a.K;
  const int hh_base = k0 / a.m;
  const int hh_end = (k0 + kCinRowBlock - 1) / a.m + 1 < a.H ? (k0 + kCinRowBlock - 1) / a.m + 1 : a.H;
  const int nhl = hh_end - hh_base;   // (<= 0 for the block that holds the bias row alone)
  const int hhl = is_k ? kw / a.m - hh_base : 0, jw = is_k ? kw % a.m : 0;
  const int rl_s = tid & 31, q_s = tid >> 5;   // the chunk row this thread stages, and its first column

  cin_f16 acc[NT];
#pragma unroll
  for (int nt = 0; nt < NT; ++nt)
#pragma unroll
    for (int q = 0; q < 16; ++q) acc[nt][q] = 0.f;

  for (int64_t rc = r_lo; rc < r_hi; rc += kCinTile) {
    const int64_t rs = rc + rl_s;
    const bool valid = rs < r_hi;
    const int64_t b = valid ? rs / a.D : 0;
    const int d = valid ? int(rs - b * a.D) : 0;
    __syncthreads();   // the previous chunk is read
    for (int c = q_s; c < NT * kCinTile; c += 8)
      Gs[rl_s * kCinGS + c] = valid && c0 + c < a.U ? cin_g(a, b, d, c0 + c) : 0.f;
    for (int j = q_s; j < a.m; j += 8) X0s[rl_s * kCinXS + j] = valid ? a.x0[(b * a.m + j) * a.D + d] : 0.f;
    for (int hl = q_s; hl < nhl; hl += 8)
      XLs[rl_s * kCinLS + hl] = valid ? a.xl[(b * a.H + hh_base + hl) * a.D + d] : 0.f;
    __syncthreads();
#pragma unroll 4
    for (int st = 0; st < kCinSteps; ++st) {
      const int rl = 2 * st + h;
      float zv = is_bias ? 1.f : 0.f;
      if (is_k) zv = XLs[rl * kCinLS + hhl] * X0s[rl * kCinXS + jw];
      const float* bp = Gs + rl * kCinGS + li;
#pragma unroll
      for (int nt = 0; nt < NT; ++nt)
        acc[nt] = __builtin_amdgcn_mfma_f32_32x32x2f32(zv, bp[nt * kCinTile], acc[nt], 0, 0, 0);
    }
  }

  const int64_t K1 = int64_t(a.K) + 1;
#pragma unroll
  for (int nt = 0; nt < NT; ++nt) {
    const int u = c0 + nt * kCinTile + li;
    if (u >= a.U) continue;
#pragma unroll
    for (int q = 0; q < 16; ++q) {
      const int k = k0 + 32 * w + cin_acc_row(q, h);
      if (k > a.K) continue;
      const float v = acc[nt][q] + 0.f;
      if (a.part) {
        a.part[(int64_t(blockIdx.z) * K1 + k) * a.U + u] = v;
      } else if (k < a.K) {
        if (a.dw) a.dw[int64_t(k) * a.U + u] = v;
      } else if (a.dbias) {
        a.dbias[u] = v;
      }
    }
  }
}

// dw [K, U] and dbias [U] from the partials [slabs][K + 1][U]; either may be null
__global__ __launch_bounds__(256) void cin_slab_sum_kernel(const float* part, float* dw, float* dbias, int64_t ku,
                                                           int64_t n, int slabs) {
  for (int64_t i = int64_t(blockIdx.x) * 256 + threadIdx.x; i < n; i += int64_t(gridDim.x) * 256) {
    const float v = fi_slab_sum(part + i, n, slabs);
    if (i < ku) {
      if (dw) dw[i] = v;
    } else if (dbias) {
      dbias[i - ku] = v;
    }
  }
}

__global__ __launch_bounds__(256) void cin_zero_kernel(float* p, int64_t n) {
  for (int64_t i = int64_t(blockIdx.x) * 256 + threadIdx.x; i < n; i += int64_t(gridDim.x) * 256) p[i] = 0.f;
}

}  // namespace mhte
#endif  // MHTE_CIN_KERNELS_H_
