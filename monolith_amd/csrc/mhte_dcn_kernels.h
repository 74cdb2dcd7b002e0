// Kernels of the DCN cross layer (mhte_dcn_core.h: the formulas, the limits, the plan).
//
// The matrix form is three GEMMs over one tile scheme: a workgroup owns 128 rows against 32 col_tiles columns, a
// wavefront one 32-row tile and col_tiles accumulator tiles; the reduction runs in chunks of 32 (16 steps of
// v_mfma_f32_32x32x2_f32).  Both operand tiles of the next chunk are fetched into registers before the MFMAs of
// this chunk are issued and stored to LDS after them, so the global loads fly under the matrix pipe.  A tile lies
// in LDS either [row][k] (33 floats apart: lanes on consecutive rows meet different banks) or [k][column] (160
// apart: the two lane halves on other banks); each GEMM takes the layout in which its global reads are coalesced.
//   dcn_mat_fwd_kernel   A = xl [row][k], B = w as stored [k][column].  Epilogue in the accumulator layout (lane =
//                        column): u = acc + bias, stored when aux is asked for, xnext = x0 u + xl.
//   dcn_mat_dx_kernel    A = du = g x0, formed while fetching, [row][j]; B = w^T read as rows of w, [column][j].
//                        Epilogue: dxl = acc + g, dx0 = dx0_acc + g u (+ dxl for a first layer, which writes no dxl).
//                        Without dxl and first there is no product: the launch is the elementwise dx0 alone.
//   dcn_mat_dw_kernel    rows are the K rows of dw, row d is dbias; A = xl [b][k] with 1 in column d, B = du [b][j];
//                        the reduction runs over one slab of batch rows; partials [slab][d + 1][d], or dw / dbias
//                        directly with one slab.
// The vector form has no matrix product: a row dot bound by bandwidth.  lanes = min(64, next power of two of d)
// lanes own a row, a lane the columns c, c + lanes, ... (at most VPL of them); a wavefront holds 64 / lanes rows at a
// time.  The dot is an in-lane chain over the lane's columns ascending, then a butterfly over the row's lanes.
//   dcn_vec_fwd_kernel   64 rows per workgroup; s, xnext = (x0 s + bias) + xl, s stored when aux is asked for
//   dcn_vec_grad_kernel  a workgroup owns one slab of rows, wavefront v the rows v, v + 4, ... (times 64 / lanes);
//                        ds by the butterfly, dxl and dx0 written per row, the column sums of dw and dbias carried
//                        in registers, then added over the wavefront's row groups (butterfly) and over the four
//                        wavefronts in wavefront order through LDS.
// cin_slab_sum_kernel adds the partials of either form in slab order, cin_zero_kernel clears dw / dbias for B == 0.
//
// No atomics; plain loads and stores; every user array is read and written below its extent only.
#ifndef MHTE_DCN_KERNELS_H_
#define MHTE_DCN_KERNELS_H_

#include "mhte_cin_kernels.h"
#include "mhte_dcn_core.h"

namespace mhte {

constexpr int kDcnTS = 33;    // floats between two rows of a [row][k] tile
constexpr int kDcnNS = 160;   // ... of a [k][column] tile

struct DcnArgs {
  const float* x0;
  const float* xl;
  const float* w;
  const float* bias;
  const float* g;         // dxnext
  const float* aux_in;    // the forward's aux, read by the gradient
  const float* dx0_acc;   // or null; may be dx0 itself
  float* xnext;
  float* aux;             // or null
  float* dx0;             // or null
  float* dxl;             // or null
  float* dw;              // or null
  float* dbias;           // or null
  float* part;            // the slab partials, or null with one slab
  int64_t B, slab_rows;
  int d, first, lanes, lane_shift;
};

// 16 MFMA steps of one chunk: the A value of step st is ap[st a_step], the B value of column tile nt is
// bp[st b_step + nt b_tile]
template <int NT>
__device__ __forceinline__ void dcn_mma(cin_f16 (&acc)[NT], const float* ap, int a_step, const float* bp, int b_step,
                                        int b_tile) {
#pragma unroll
  for (int st = 0; st < kDcnSteps; ++st) {
    const float av = ap[st * a_step];
#pragma unroll
    for (int nt = 0; nt < NT; ++nt)
      acc[nt] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, bp[st * b_step + nt * b_tile], acc[nt], 0, 0, 0);
  }
}

template <int NT>
__device__ __forceinline__ void dcn_acc_clear(cin_f16 (&acc)[NT]) {
#pragma unroll
  for (int nt = 0; nt < NT; ++nt)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[nt][r] = 0.f;
}

template <int NT>
__global__ __launch_bounds__(256) void dcn_mat_fwd_kernel(DcnArgs a) {
  constexpr int SPAN = NT * kDcnTile, NB = 4 * NT;
  __shared__ float As[kDcnRowBlock * kDcnTS];   // xl [row][k]
  __shared__ float Bs[kDcnChunk * kDcnNS];      // w [k][column]
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, li = lane & 31, h = lane >> 5;
  const int64_t b0 = int64_t(blockIdx.x) * kDcnRowBlock;
  const int c0 = int(blockIdx.y) * SPAN, d = a.d;
  const int ar = tid >> 5, ak = tid & 31;   // the row (+ 8 i) and the k this thread stages of A

  float pa[16], pb[NB];
  auto fetch = [&](int k0) {
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int64_t b = b0 + ar + 8 * i;
      pa[i] = b < a.B && k0 + ak < d ? a.xl[b * d + k0 + ak] : 0.f;
    }
#pragma unroll
    for (int i = 0; i < NB; ++i) {
      const int e = tid + 256 * i, kk = e / SPAN, c = e % SPAN;
      pb[i] = k0 + kk < d && c0 + c < d ? a.w[int64_t(k0 + kk) * d + c0 + c] : 0.f;
    }
  };
  cin_f16 acc[NT];
  dcn_acc_clear<NT>(acc);
  fetch(0);
  for (int k0 = 0; k0 < d; k0 += kDcnChunk) {
    __syncthreads();   // the previous chunk is read
#pragma unroll
    for (int i = 0; i < 16; ++i) As[(ar + 8 * i) * kDcnTS + ak] = pa[i];
#pragma unroll
    for (int i = 0; i < NB; ++i) {
      const int e = tid + 256 * i;
      Bs[(e / SPAN) * kDcnNS + e % SPAN] = pb[i];
    }
    __syncthreads();
    if (k0 + kDcnChunk < d) fetch(k0 + kDcnChunk);
    dcn_mma<NT>(acc, As + (32 * w + li) * kDcnTS + h, 2, Bs + h * kDcnNS + li, 2 * kDcnNS, kDcnTile);
  }

#pragma unroll
  for (int nt = 0; nt < NT; ++nt) {
    const int j = c0 + nt * kDcnTile + li;
    if (j >= d) continue;
    const float bv = a.bias[j];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int64_t b = b0 + 32 * w + cin_acc_row(r, h);
      if (b >= a.B) continue;
      const int64_t i = b * d + j;
      const float u = acc[nt][r] + bv;
      if (a.aux) a.aux[i] = u;
      a.xnext[i] = (a.x0[i] * u + a.xl[i]) + 0.f;
    }
  }
}

template <int NT>
__global__ __launch_bounds__(256) void dcn_mat_dx_kernel(DcnArgs a) {
  constexpr int SPAN = NT * kDcnTile, NB = 4 * NT;
  __shared__ float As[kDcnRowBlock * kDcnTS];   // du [row][j]
  __shared__ float Bt[SPAN * kDcnTS];           // w [column k][j]: w^T without a transposed copy
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, li = lane & 31, h = lane >> 5;
  const int64_t b0 = int64_t(blockIdx.x) * kDcnRowBlock;
  const int c0 = int(blockIdx.y) * SPAN, d = a.d;
  const int ar = tid >> 5, ak = tid & 31;
  const int jn = a.dxl || a.first ? d : 0;   // without dxl there is no product

  float pa[16], pb[NB];
  auto fetch = [&](int j0) {
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int64_t b = b0 + ar + 8 * i;
      const bool ok = b < a.B && j0 + ak < d;
      const int64_t x = ok ? b * d + j0 + ak : 0;
      pa[i] = ok ? a.g[x] * a.x0[x] : 0.f;
    }
#pragma unroll
    for (int i = 0; i < NB; ++i) {
      const int c = ar + 8 * i;
      pb[i] = c0 + c < d && j0 + ak < d ? a.w[int64_t(c0 + c) * d + j0 + ak] : 0.f;
    }
  };
  cin_f16 acc[NT];
  dcn_acc_clear<NT>(acc);
  if (jn) fetch(0);
  for (int j0 = 0; j0 < jn; j0 += kDcnChunk) {
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 16; ++i) As[(ar + 8 * i) * kDcnTS + ak] = pa[i];
#pragma unroll
    for (int i = 0; i < NB; ++i) Bt[(ar + 8 * i) * kDcnTS + ak] = pb[i];
    __syncthreads();
    if (j0 + kDcnChunk < jn) fetch(j0 + kDcnChunk);
    dcn_mma<NT>(acc, As + (32 * w + li) * kDcnTS + h, 2, Bt + li * kDcnTS + h, 2, kDcnTile * kDcnTS);
  }

#pragma unroll
  for (int nt = 0; nt < NT; ++nt) {
    const int k = c0 + nt * kDcnTile + li;
    if (k >= d) continue;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int64_t b = b0 + 32 * w + cin_acc_row(r, h);
      if (b >= a.B) continue;
      const int64_t i = b * d + k;
      const float gv = a.g[i];
      const float dxl = acc[nt][r] + gv;
      if (a.dx0) {
        float v = gv * a.aux_in[i];
        if (a.dx0_acc) v = a.dx0_acc[i] + v;
        if (a.first) v = v + dxl;
        a.dx0[i] = v + 0.f;
      }
      if (a.dxl && !a.first) a.dxl[i] = dxl;
    }
  }
}

template <int NT>
__global__ __launch_bounds__(256) void dcn_mat_dw_kernel(DcnArgs a) {
  constexpr int SPAN = NT * kDcnTile, NB = 4 * NT;
  __shared__ float As[kDcnChunk * kDcnNS];   // xl [b][k], 1 in column d
  __shared__ float Bs[kDcnChunk * kDcnNS];   // du [b][j]
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, li = lane & 31, h = lane >> 5;
  const int k0 = int(blockIdx.x) * kDcnRowBlock, c0 = int(blockIdx.y) * SPAN, d = a.d;
  const int64_t r_lo = int64_t(blockIdx.z) * a.slab_rows;
  const int64_t r_hi = r_lo + a.slab_rows < a.B ? r_lo + a.slab_rows : a.B;
  const int ab = tid >> 7, ak = tid & 127;   // the batch row (+ 2 i) and the K row this thread stages of A

  float pa[16], pb[NB];
  auto fetch = [&](int64_t rc) {
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int64_t b = rc + ab + 2 * i;
      float v = 0.f;
      if (b < r_hi) {
        if (k0 + ak < d) v = a.xl[b * d + k0 + ak];
        if (k0 + ak == d) v = 1.f;
      }
      pa[i] = v;
    }
#pragma unroll
    for (int i = 0; i < NB; ++i) {
      const int e = tid + 256 * i, bb = e / SPAN, c = e % SPAN;
      const bool ok = rc + bb < r_hi && c0 + c < d;
      const int64_t x = ok ? (rc + bb) * d + c0 + c : 0;
      pb[i] = ok ? a.g[x] * a.x0[x] : 0.f;
    }
  };
  cin_f16 acc[NT];
  dcn_acc_clear<NT>(acc);
  fetch(r_lo);
  for (int64_t rc = r_lo; rc < r_hi; rc += kDcnChunk) {
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 16; ++i) As[(ab + 2 * i) * kDcnNS + ak] = pa[i];
#pragma unroll
    for (int i = 0; i < NB; ++i) {
      const int e = tid + 256 * i;
      Bs[(e / SPAN) * kDcnNS + e % SPAN] = pb[i];
    }
    __syncthreads();
    if (rc + kDcnChunk < r_hi) fetch(rc + kDcnChunk);
    dcn_mma<NT>(acc, As + h * kDcnNS + 32 * w + li, 2 * kDcnNS, Bs + h * kDcnNS + li, 2 * kDcnNS, kDcnTile);
  }

#pragma unroll
  for (int nt = 0; nt < NT; ++nt) {
    const int j = c0 + nt * kDcnTile + li;
    if (j >= d) continue;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int k = k0 + 32 * w + cin_acc_row(r, h);
      if (k > d) continue;
      const float v = acc[nt][r] + 0.f;
      if (a.part) {
        a.part[(int64_t(blockIdx.z) * (d + 1) + k) * d + j] = v;
      } else if (k < d) {
        if (a.dw) a.dw[int64_t(k) * d + j] = v;
      } else if (a.dbias) {
        a.dbias[j] = v;
      }
    }
  }
}

// the sum of p over the lanes of one row (a butterfly: every lane ends with the same bits)
__device__ __forceinline__ float dcn_row_sum(float p, int lanes) {
  for (int off = lanes >> 1; off >= 1; off >>= 1) p += __shfl_xor(p, off);
  return p;
}

template <int VPL>
__global__ __launch_bounds__(256) void dcn_vec_fwd_kernel(DcnArgs a) {
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, d = a.d;
  const int cl = lane & (a.lanes - 1), sub = lane >> a.lane_shift, rpw = 64 >> a.lane_shift;
  const int64_t r_lo = int64_t(blockIdx.x) * kDcnVecRows + w * (kDcnVecRows / 4);
  const int64_t r_hi = r_lo + kDcnVecRows / 4 < a.B ? r_lo + kDcnVecRows / 4 : a.B;
  float wv[VPL];
#pragma unroll
  for (int i = 0; i < VPL; ++i) {
    const int c = cl + a.lanes * i;
    wv[i] = c < d ? a.w[c] : 0.f;
  }
  for (int64_t rb = r_lo; rb < r_hi; rb += rpw) {   // (uniform in the wavefront)
    const int64_t r = rb + sub;
    const bool ok = r < r_hi;
    const int64_t base = ok ? r * d : 0;
    float xv[VPL];
    float p = 0.f;
#pragma unroll
    for (int i = 0; i < VPL; ++i) {
      const int c = cl + a.lanes * i;
      xv[i] = ok && c < d ? a.xl[base + c] : 0.f;
      p += xv[i] * wv[i];
    }
    const float s = dcn_row_sum(p, a.lanes);
    if (!ok) continue;
    if (a.aux && cl == 0) a.aux[r] = s;
#pragma unroll
    for (int i = 0; i < VPL; ++i) {
      const int c = cl + a.lanes * i;
      if (c < d) a.xnext[base + c] = ((a.x0[base + c] * s + a.bias[c]) + xv[i]) + 0.f;
    }
  }
}

template <int VPL>
__global__ __launch_bounds__(256) void dcn_vec_grad_kernel(DcnArgs a) {
  __shared__ float Red[64 * VPL];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, d = a.d;
  const int cl = lane & (a.lanes - 1), sub = lane >> a.lane_shift, rpw = 64 >> a.lane_shift;
  const int64_t r_lo = int64_t(blockIdx.x) * a.slab_rows;
  const int64_t r_hi = r_lo + a.slab_rows < a.B ? r_lo + a.slab_rows : a.B;
  const bool sums = a.dw || a.dbias;
  float aw[VPL], ab[VPL];
#pragma unroll
  for (int i = 0; i < VPL; ++i) aw[i] = ab[i] = 0.f;

  for (int64_t rb = r_lo + w * rpw; rb < r_hi; rb += 4 * rpw) {   // (uniform in the wavefront)
    const int64_t r = rb + sub;
    const bool ok = r < r_hi;
    const int64_t base = ok ? r * d : 0;
    float gv[VPL];
    float p = 0.f;
#pragma unroll
    for (int i = 0; i < VPL; ++i) {
      const int c = cl + a.lanes * i;
      const bool in = ok && c < d;
      gv[i] = in ? a.g[base + c] : 0.f;
      p += gv[i] * (in ? a.x0[base + c] : 0.f);
    }
    const float ds = dcn_row_sum(p, a.lanes);
    const float s = ok && a.dx0 ? a.aux_in[r] : 0.f;
#pragma unroll
    for (int i = 0; i < VPL; ++i) {
      const int c = cl + a.lanes * i;
      if (!(ok && c < d)) continue;
      const float dxl = ds * a.w[c] + gv[i];
      if (a.dx0) {
        float v = gv[i] * s;
        if (a.dx0_acc) v = a.dx0_acc[base + c] + v;
        if (a.first) v = v + dxl;
        a.dx0[base + c] = v + 0.f;
      }
      if (a.dxl && !a.first) a.dxl[base + c] = dxl + 0.f;
      if (sums) {
        aw[i] += ds * a.xl[base + c];
        ab[i] += gv[i];
      }
    }
  }
  if (!sums) return;   // (uniform)

  // the row groups of the wavefront, then the wavefronts in their order
#pragma unroll
  for (int i = 0; i < VPL; ++i)
    for (int off = a.lanes; off < 64; off <<= 1) {
      aw[i] += __shfl_xor(aw[i], off);
      ab[i] += __shfl_xor(ab[i], off);
    }
  for (int q = 0; q < 2; ++q)
    for (int v = 1; v < 4; ++v) {
      __syncthreads();   // the previous round is read
      if (w == v) {
#pragma unroll
        for (int i = 0; i < VPL; ++i) Red[i * 64 + lane] = q ? ab[i] : aw[i];
      }
      __syncthreads();
      if (w == 0) {
#pragma unroll
        for (int i = 0; i < VPL; ++i) {
          if (q)
            ab[i] += Red[i * 64 + lane];
          else
            aw[i] += Red[i * 64 + lane];
        }
      }
    }
  if (w != 0 || sub != 0) return;
#pragma unroll
  for (int i = 0; i < VPL; ++i) {
    const int c = cl + a.lanes * i;
    if (c >= d) continue;
    if (a.part) {
      a.part[int64_t(blockIdx.x) * 2 * d + c] = aw[i];
      a.part[int64_t(blockIdx.x) * 2 * d + d + c] = ab[i];
    } else {
      if (a.dw) a.dw[c] = aw[i];
      if (a.dbias) a.dbias[c] = ab[i];
    }
  }
}

}  // namespace mhte
#endif  // MHTE_DCN_KERNELS_H_
