// The FFM feature cross on the device: forward (multiply, dot) and the gradient of both operands in one launch.
// The arithmetic, the shapes and the choice of form are mhte_ffm_core.h's; reference: FFMKernelMultiply /
// FFMKernelDot / FFMGradKernelMultiply / FFMGradKernelDot, native_training/layers/kernels/ffm_kernels.cu.cc:34-168,
// which give one thread a whole batch row.  Included by mhte.hip.
//
// Every kernel comes as VEC = 4 (16-byte global and LDS accesses; D % 4 == 0, the pointers 16-byte aligned, the
// row widths multiples of 4 floats) and VEC = 1 (4-byte accesses of the same elements, same bits), as the table
// kernels do, and as an LDS form and a direct form:
//   forward, LDS form    a workgroup takes a tile of batch rows by grid stride, stages the tile's (L + R) D input
//                        floats in LDS with coalesced loads, then lays its lanes over the tile's OUTPUT, which is
//                        one contiguous run of memory (out_cols is exactly L R D resp. L R): consecutive lanes
//                        store consecutive 16-byte (multiply, VEC = 4) or 4-byte words.  Every input float comes
//                        from HBM once and is reused R resp. L times from LDS.  multiply is a write stream: its
//                        stores are nontemporal.  dot reads its 2 D floats per output as 16-byte LDS reads.
//   gradient, LDS form   a workgroup stages a tile's slabs of grad (L R D floats per row for multiply, L R for
//                        dot; nontemporal 16-byte loads: grad is read once) and its rows of left and right, then
//                        lays its lanes over the tile's left_grad and right_grad rows, trailing columns (+0)
//                        included: a lane sums its R resp. L terms from LDS, walking the slab with stride D resp.
//                        R D.  grad comes from HBM once for both outputs.
//   direct forms         a row whose operands do not fit the LDS budget (mhte_ffm_core.h): the lanes are laid over
//                        the whole output in the same way and read every operand where it lies; the gradient then
//                        reads grad twice.
// Index widths: a tile's element counts fit 32 bits (the LDS budget bounds them); rows and whole-tensor offsets
// are 64-bit.  The host has checked that every row width and L R D are below 2^31 and batch * width below 2^62.
#ifndef MHTE_FFM_KERNELS_H_
#define MHTE_FFM_KERNELS_H_

#include "../../include/monolith_amd_hash_table.h"
#include "mhte_ffm_core.h"
#include "mhte_kernels.h"

namespace mhte {

template <int VEC> struct FfmVec;
template <> struct FfmVec<1> { typedef float type; };
template <> struct FfmVec<4> { typedef FfmF4 type; };

struct FfmFwdArgs {
  const float* left;
  const float* right;
  float* out;
  long long left_cols, right_cols, batch;
  uint32_t L, R, D, tile_rows;
};
struct FfmGradArgs {
  const float* grad;
  const float* left;
  const float* right;
  float* left_grad;
  float* right_grad;
  long long grad_cols, left_cols, right_cols, batch;
  uint32_t L, R, D, tile_rows;
};

// T (float or FfmF4) at p in global memory
template <class T>
__device__ __forceinline__ T ffm_ld(const float* p) { return *(const MHTE_GLOBAL T*)(p); }
template <class T>
__device__ __forceinline__ T ffm_ld_once(const float* p) {   // read once: past L1
  return __builtin_nontemporal_load((const MHTE_GLOBAL T*)(p));
}
template <class T>
__device__ __forceinline__ void ffm_st(float* p, T v) { *(MHTE_GLOBAL T*)(p) = v; }
template <class T>
__device__ __forceinline__ void ffm_st_stream(float* p, T v) { __builtin_nontemporal_store(v, (MHTE_GLOBAL T*)(p)); }

// Stages rows x n T's (float or FfmF4) into LDS: row i of dst is the first n T's of src's row i, src_cols floats
// apart.  Eight loads per thread are issued before the first of them is written to LDS: with two to five
// workgroups per CU it is the loads in flight per thread that cover the HBM latency.  ONCE: nontemporal loads.
template <class T, bool ONCE>
__device__ __forceinline__ void ffm_stage(T* dst, const float* src, long long src_cols, uint32_t rows, uint32_t n,
                                          uint32_t t) {
  constexpr int U = 8;
  constexpr int TV = int(sizeof(T) / 4);
  const uint32_t total = rows * n;
  uint32_t i = t;
  for (; i + (U - 1) * kFfmThreads < total; i += U * kFfmThreads) {
    T v[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const uint32_t k = i + u * kFfmThreads, row = k / n, c = k % n;
      const float* p = src + row * src_cols + (long long)(c) * TV;
      v[u] = ONCE ? ffm_ld_once<T>(p) : ffm_ld<T>(p);
    }
#pragma unroll
    for (int u = 0; u < U; ++u) dst[i + u * kFfmThreads] = v[u];
  }
  for (; i < total; i += kFfmThreads) {
    const uint32_t row = i / n, c = i % n;
    const float* p = src + row * src_cols + (long long)(c) * TV;
    dst[i] = ONCE ? ffm_ld_once<T>(p) : ffm_ld<T>(p);
  }
}

// ---- forward ----------------------------------------------------------------------------------------------
// One output element j of a run of rows.  left_at(row) / right_at(row): the row's L D resp. R D floats as V.
// multiply: j counts V's, j = (row L + l) (R Dv) + r Dv + kv; dot: j counts floats, j = row (L R) + l R + r.
template <int VEC, bool DOT, bool LDS>
__global__ __launch_bounds__(kFfmThreads) void ffm_fwd_kernel(FfmFwdArgs A) {
  typedef typename FfmVec<VEC>::type V;
  const uint32_t t = threadIdx.x;
  const uint32_t Dv = A.D / VEC, LDv = A.L * Dv, RDv = A.R * Dv, LR = A.L * A.R;
  const uint32_t OV = DOT ? LR : LR * Dv;   // output elements per row: floats (dot) or V's (multiply)
  if constexpr (LDS) {
    __shared__ FfmF4 sm[kFfmFwdLdsFloats / 4];
    V* const sl = reinterpret_cast<V*>(sm);   // [tile_rows][LDv]
    V* const sr = sl + A.tile_rows * LDv;     // [tile_rows][RDv]
    const long long n_tiles = (A.batch + A.tile_rows - 1) / A.tile_rows;
    for (long long tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
      const long long b0 = tile * A.tile_rows;
      const uint32_t rows = uint32_t(A.batch - b0 < (long long)(A.tile_rows) ? A.batch - b0 : A.tile_rows);
      ffm_stage<V, false>(sl, A.left + b0 * A.left_cols, A.left_cols, rows, LDv, t);
      ffm_stage<V, false>(sr, A.right + b0 * A.right_cols, A.right_cols, rows, RDv, t);
      __syncthreads();
      float* const out0 = A.out + b0 * (long long)(OV) * (DOT ? 1 : VEC);   // the tile's outputs: one run
      const uint32_t n_out = rows * OV;
      for (uint32_t j = t; j < n_out; j += kFfmThreads) {
        if constexpr (DOT) {
          const uint32_t row = j / LR, lr = j % LR, l = lr / A.R, r = lr % A.R;
          ffm_st<float>(out0 + j, ffm_dot_elem(sl + row * LDv + l * Dv, sr + row * RDv + r * Dv, int(Dv)));
        } else {
          const uint32_t rl = j / RDv, rem = j % RDv, row = rl / A.L, kv = rem % Dv;
          ffm_st_stream<V>(out0 + (long long)(j) * VEC, ffm_mul(sl[rl * Dv + kv], sr[row * RDv + rem]));
        }
      }
      __syncthreads();   // (the next tile overwrites what the slower waves still read)
    }
  } else {
    const long long total = A.batch * (long long)(OV);
    for (long long j = (long long)(blockIdx.x) * kFfmThreads + t; j < total; j += (long long)(gridDim.x) * kFfmThreads) {
      const long long b = j / OV;
      const uint32_t o = uint32_t(j % OV);
      const MHTE_GLOBAL V* lrow = (const MHTE_GLOBAL V*)(A.left + b * A.left_cols);
      const MHTE_GLOBAL V* rrow = (const MHTE_GLOBAL V*)(A.right + b * A.right_cols);
      if constexpr (DOT) {
        const uint32_t l = o / A.R, r = o % A.R;
        ffm_st<float>(A.out + j, ffm_dot_elem(lrow + l * Dv, rrow + r * Dv, int(Dv)));
      } else {
        const uint32_t l = o / RDv, rem = o % RDv, kv = rem % Dv;
        ffm_st_stream<V>(A.out + j * VEC, ffm_mul(lrow[l * Dv + kv], rrow[rem]));
      }
    }
  }
}

// ---- gradient ---------------------------------------------------------------------------------------------
// One output V of a row: c < Lcv is left_grad's V c, else right_grad's V c - Lcv; columns beyond L D / R D get
// +0.  g, lrow, rrow: the row's slab of grad (float for dot, V for multiply), its L D and its R D floats as V.
template <int VEC, bool DOT, class PG, class PV>
__device__ __forceinline__ void ffm_grad_one(const FfmGradArgs& A, long long b, uint32_t c, uint32_t Lcv, PG g,
                                             PV lrow, PV rrow) {
  typedef typename FfmVec<VEC>::type V;
  const uint32_t Dv = A.D / VEC, LDv = A.L * Dv, RDv = A.R * Dv;
  V v = V{};
  if (c < Lcv) {
    if (c < LDv) {
      const uint32_t l = c / Dv, kv = c % Dv;
      if constexpr (DOT)
        v = ffm_grad_elem<V>(g + l * A.R, 1, rrow + kv, Dv, int(A.R));
      else
        v = ffm_grad_elem<V>(g + l * RDv + kv, Dv, rrow + kv, Dv, int(A.R));
    }
    ffm_st<V>(A.left_grad + b * A.left_cols + (long long)(c) * VEC, v);
  } else {
    c -= Lcv;
    if (c < RDv) {
      const uint32_t r = c / Dv, kv = c % Dv;
      if constexpr (DOT)
        v = ffm_grad_elem<V>(g + r, A.R, lrow + kv, Dv, int(A.L));
      else
        v = ffm_grad_elem<V>(g + r * Dv + kv, RDv, lrow + kv, Dv, int(A.L));
    }
    ffm_st<V>(A.right_grad + b * A.right_cols + (long long)(c) * VEC, v);
  }
}

template <int VEC, bool DOT, bool LDS>
__global__ __launch_bounds__(kFfmThreads) void ffm_grad_kernel(FfmGradArgs A) {
  typedef typename FfmVec<VEC>::type V;
  typedef typename FfmVec<DOT ? 1 : VEC>::type GV;   // what grad is read as
  constexpr int GVEC = DOT ? 1 : VEC;
  const uint32_t t = threadIdx.x;
  const uint32_t Dv = A.D / VEC, LDv = A.L * Dv, RDv = A.R * Dv, LR = A.L * A.R;
  const uint32_t Gs = DOT ? LR : LR * Dv;   // the slab of one row, in GV's
  const uint32_t Lcv = uint32_t(A.left_cols / VEC), Rcv = uint32_t(A.right_cols / VEC);
  if constexpr (LDS) {
    __shared__ FfmF4 sm[kFfmGradLdsFloats / 4];
    GV* const sg = reinterpret_cast<GV*>(sm);   // [tile_rows][Gs]
    const uint32_t g_floats = (A.tile_rows * Gs * GVEC + 3u) & ~3u;
    V* const sl = reinterpret_cast<V*>(reinterpret_cast<float*>(sm) + g_floats);   // [tile_rows][LDv]
    V* const sr = sl + A.tile_rows * LDv;                                          // [tile_rows][RDv]
    const uint32_t Ocv = Lcv + Rcv;   // (the trailing columns are fewer than D: a tile's counts stay small)
    const long long n_tiles = (A.batch + A.tile_rows - 1) / A.tile_rows;
    for (long long tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
      const long long b0 = tile * A.tile_rows;
      const uint32_t rows = uint32_t(A.batch - b0 < (long long)(A.tile_rows) ? A.batch - b0 : A.tile_rows);
      ffm_stage<GV, true>(sg, A.grad + b0 * A.grad_cols, A.grad_cols, rows, Gs, t);
      ffm_stage<V, false>(sl, A.left + b0 * A.left_cols, A.left_cols, rows, LDv, t);
      ffm_stage<V, false>(sr, A.right + b0 * A.right_cols, A.right_cols, rows, RDv, t);
      __syncthreads();
      for (uint32_t j = t; j < rows * Ocv; j += kFfmThreads) {
        const uint32_t row = j / Ocv, c = j % Ocv;
        ffm_grad_one<VEC, DOT>(A, b0 + row, c, Lcv, sg + row * Gs, sl + row * LDv, sr + row * RDv);
      }
      __syncthreads();   // (the next tile overwrites what the slower waves still read)
    }
  } else {
    const long long Ocv = (long long)(Lcv) + Rcv;
    const long long total = A.batch * Ocv;
    for (long long j = (long long)(blockIdx.x) * kFfmThreads + t; j < total; j += (long long)(gridDim.x) * kFfmThreads) {
      const long long b = j / Ocv;
      const uint32_t c = uint32_t(j % Ocv);
      ffm_grad_one<VEC, DOT>(A, b, c, Lcv, (const MHTE_GLOBAL GV*)(A.grad + b * A.grad_cols),
                             (const MHTE_GLOBAL V*)(A.left + b * A.left_cols),
                             (const MHTE_GLOBAL V*)(A.right + b * A.right_cols));
    }
  }
}

}  // namespace mhte
#endif  // MHTE_FFM_KERNELS_H_
