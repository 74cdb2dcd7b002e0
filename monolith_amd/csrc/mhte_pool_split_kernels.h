// The pooling of the feature-column path: ragged sum of every feature's rows per batch row, written
// straight into the column slices the dense model takes, and the gradient of that — ONE launch each for
// all features.  Reference: MonolithFusedReduceAndSplitGPU / ...GPUGrad, runtime/ops/reduce_op.cu.cc
// :290-379 (forward kernel), :477-534 (gradient kernel), :392-475 (the op's plan); on the CPU
// MonolithFusedReduceSumAndSplit, runtime/ops/reduce_op.cc:231-321.  Included by mhte.hip.
//
// The reference gives one thread one output ELEMENT (a column of a batch row) and lets it walk the row's
// ids alone, and its gradient finds every element's batch row by binary search.  Here a lane group takes
// one (feature, batch row): a lane keeps one float4 column (or one float where the feature's shape or a
// pointer does not allow 16-byte accesses), the rows of the range are fetched 4 (16 in a long range) at a time and ADDED in
// row order into an accumulator that starts at +0 — the reference's `sum = T(0); sum += ...` chain
// (:308-316) bit for bit, a row of -0.0 alone gives +0.0 — and a row of any length stays one chain (the
// order is the contract; the reference says the same of itself at :348-350).  The gradient's group reads
// its gradient row once and stores it to every row of its range; rows of the feature outside every range
// are zeroed by the same launch.
#ifndef MHTE_POOL_SPLIT_KERNELS_H_
#define MHTE_POOL_SPLIT_KERNELS_H_

#include "mhte_kernels.h"

namespace mhte {

// One row of the grid (blockIdx.y): up to 64 lane columns of one feature.  A block reads its unit with
// wave-uniform loads (scalar registers); a feature wider than 64 lane columns is several units.
struct SplitUnit {
  float* emb;          // forward: the feature's rows [n_rows, dim] (read); gradient: their gradient (written)
  long long n_rows;
  int32_t rs_off;      // where the feature's bs + 1 row splits begin in the concatenated array
  int32_t dim;         // floats per row of emb
  int32_t col0, width; // the unit's columns [col0, col0 + width) of the feature
  int32_t slice0, n_slices;   // the feature's slices in the slice table, by ascending first column
  int32_t vec;         // 1: float4 columns (dim, every slice start and length multiples of 4, pointers aligned)
  int32_t log2g;       // lanes per batch row = 1 << log2g (>= the unit's lane columns)
};
struct SplitSlice {
  float* out;          // forward: the slice's output [bs, dim] (written); gradient: its gradient (read)
  int32_t start, dim;  // first column inside the feature, width
};
constexpr int kSplitInlineUnits = 32, kSplitInlineSlices = 96;   // beyond: the tables are uploaded per call
constexpr int kSplitUnitCols = 64;
constexpr int kSplitDeep = 16;   // rows of a long range in flight per lane
struct SplitArgs {
  const int32_t* row_splits;
  const SplitUnit* x_units;     // EXT: the tables in device memory
  const SplitSlice* x_slices;
  int32_t bs, unit_base;
  SplitUnit units[kSplitInlineUnits];
  SplitSlice slices[kSplitInlineSlices];
};

// (the tables of an EXT launch are read through pointers that are global by type, member by member)
__device__ __forceinline__ SplitUnit split_load(const MHTE_GLOBAL SplitUnit* p) {
  SplitUnit u;
  u.emb = p->emb;
  u.n_rows = p->n_rows;
  u.rs_off = p->rs_off;
  u.dim = p->dim;
  u.col0 = p->col0;
  u.width = p->width;
  u.slice0 = p->slice0;
  u.n_slices = p->n_slices;
  u.vec = p->vec;
  u.log2g = p->log2g;
  return u;
}
__device__ __forceinline__ SplitSlice split_load(const MHTE_GLOBAL SplitSlice* p) {
  SplitSlice s;
  s.out = p->out;
  s.start = p->start;
  s.dim = p->dim;
  return s;
}

template <int VEC>
__device__ __forceinline__ void split_store(float* p, const Vec<VEC>& v);
template <>
__device__ __forceinline__ void split_store<4>(float* p, const Vec<4>& v) {
  Vec<4>::f32x4 t;
  t.x = v.v[0]; t.y = v.v[1]; t.z = v.v[2]; t.w = v.v[3];
  __builtin_nontemporal_store(t, (MHTE_GLOBAL Vec<4>::f32x4*)(p));
}
template <>
__device__ __forceinline__ void split_store<1>(float* p, const Vec<1>& v) {
  __builtin_nontemporal_store(v.v[0], (MHTE_GLOBAL float*)(p));
}

// a row split as the kernels use it: inside [lo, n] whatever the array holds (a malformed row_splits
// reads no row outside the feature)
__device__ __forceinline__ int32_t split_clamp(int32_t x, int32_t lo, int32_t n) { return min(max(x, lo), n); }

template <int VEC>
__device__ __forceinline__ void reduce_split_rows(const SplitUnit& u, const SplitSlice& s, int32_t c,
                                                  const MHTE_GLOBAL int32_t* rs, int32_t bs, int64_t b,
                                                  int64_t stride) {
  if (b >= bs) return;
  const int32_t n = int32_t(min(u.n_rows, (long long)INT32_MAX));
  const float* src = u.emb + c;
  float* dst = s.out + (c - s.start);
  int32_t s0 = split_clamp(rs[b], 0, n), s1 = split_clamp(rs[b + 1], s0, n);
  for (;;) {
    const int64_t nb = b + stride;   // the next row's splits travel while this row is summed
    int32_t n0 = 0, n1 = 0;
    if (nb < bs) {
      n0 = rs[nb];
      n1 = rs[nb + 1];
    }
    Vec<VEC> acc;
    vec_zero(acc);
    int32_t i = s0;
    // a long row is one chain of round trips: 16 rows per trip while 16 are left (a row of 3 000 ids alone
    // otherwise outlasts the rest of the launch), the adds still one after the other
    for (; i + kSplitDeep <= s1; i += kSplitDeep) {
      Vec<VEC> w[kSplitDeep];
#pragma unroll
      for (int t = 0; t < kSplitDeep; ++t) w[t].load(src + int64_t(i + t) * u.dim);
#pragma unroll
      for (int t = 0; t < kSplitDeep; ++t) {
#pragma unroll
        for (int k = 0; k < VEC; ++k) acc.v[k] = acc.v[k] + w[t].v[k];
      }
    }
    for (; i < s1; i += 4) {                 // 4 rows in flight (fetched from a row of the range whatever
      Vec<VEC> v[4];                         // i + t is, masked at the add), added in order
#pragma unroll
      for (int t = 0; t < 4; ++t) v[t].load(src + int64_t(min(i + t, s1 - 1)) * u.dim);
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        if (i + t < s1) {
#pragma unroll
          for (int k = 0; k < VEC; ++k) acc.v[k] = acc.v[k] + v[t].v[k];
        }
      }
    }
    split_store<VEC>(dst + b * int64_t(s.dim), acc);
    if (nb >= bs) break;
    b = nb;
    s0 = split_clamp(n0, 0, n);
    s1 = split_clamp(n1, s0, n);
  }
}

template <int VEC>
__device__ __forceinline__ void reduce_split_grad_rows(const SplitUnit& u, const SplitSlice& s, int32_t c,
                                                       const MHTE_GLOBAL int32_t* rs, int32_t bs, int64_t b,
                                                       int64_t stride) {
  const int32_t n = int32_t(min(u.n_rows, (long long)INT32_MAX));
  float* dst = u.emb + c;
  const float* src = s.out + (c - s.start);
  // rows no range covers: [0, rs[0]) and [rs[bs], n_rows), shared out over the unit's groups
  {
    const int64_t first = split_clamp(rs[0], 0, n), last = split_clamp(rs[bs], int32_t(first), n);
    const int64_t n_out = first + (u.n_rows - last);
    Vec<VEC> z;
    vec_zero(z);
    for (int64_t r = b; r < n_out; r += stride)
      split_store<VEC>(dst + (r < first ? r : last + (r - first)) * u.dim, z);
  }
  if (b >= bs) return;
  int32_t s0 = split_clamp(rs[b], 0, n), s1 = split_clamp(rs[b + 1], s0, n);
  for (;;) {
    const int64_t nb = b + stride;
    int32_t n0 = 0, n1 = 0;
    if (nb < bs) {
      n0 = rs[nb];
      n1 = rs[nb + 1];
    }
    if (s0 < s1) {
      Vec<VEC> g;
      g.load(src + b * int64_t(s.dim));
      for (int32_t r = s0; r < s1; ++r) split_store<VEC>(dst + int64_t(r) * u.dim, g);
    }
    if (nb >= bs) break;
    b = nb;
    s0 = split_clamp(n0, 0, n);
    s1 = split_clamp(n1, s0, n);
  }
}

// grid (row blocks, units).  EXT: unit and slice tables in device memory (any number of features and
// slices); otherwise in the kernel arguments.
template <bool EXT, bool FWD>
__global__ __launch_bounds__(256) void reduce_split_kernel(SplitArgs A) {
  const int32_t ui = A.unit_base + int32_t(blockIdx.y);
  const MHTE_GLOBAL SplitUnit* xu = (const MHTE_GLOBAL SplitUnit*)(A.x_units);
  const MHTE_GLOBAL SplitSlice* xs = (const MHTE_GLOBAL SplitSlice*)(A.x_slices);
  const SplitUnit u = EXT ? split_load(xu + ui) : A.units[ui];
  const int32_t g = 1 << u.log2g;
  const int32_t j = int32_t(threadIdx.x) & (g - 1);
  const int32_t lane_cols = u.vec ? 4 : 1;
  if (j * lane_cols >= u.width) return;
  const int32_t c = u.col0 + j * lane_cols;   // the lane's first column inside the feature
  // the slice that holds it: the last one that starts at or before c
  int32_t lo = u.slice0, hi = u.slice0 + u.n_slices - 1;
  while (lo < hi) {
    const int32_t mid = (lo + hi + 1) >> 1;
    const int32_t start = EXT ? xs[mid].start : A.slices[mid].start;
    if (start <= c) lo = mid; else hi = mid - 1;
  }
  const SplitSlice s = EXT ? split_load(xs + lo) : A.slices[lo];
  const int64_t groups = 256 >> u.log2g;
  const int64_t b = int64_t(blockIdx.x) * groups + (threadIdx.x >> u.log2g);
  const int64_t stride = int64_t(gridDim.x) * groups;
  const MHTE_GLOBAL int32_t* rs = (const MHTE_GLOBAL int32_t*)(A.row_splits) + u.rs_off;
  if (u.vec) {
    if (FWD) reduce_split_rows<4>(u, s, c, rs, A.bs, b, stride);
    else reduce_split_grad_rows<4>(u, s, c, rs, A.bs, b, stride);
  } else {
    if (FWD) reduce_split_rows<1>(u, s, c, rs, A.bs, b, stride);
    else reduce_split_grad_rows<1>(u, s, c, rs, A.bs, b, stride);
  }
}

}  // namespace mhte
#endif  // MHTE_POOL_SPLIT_KERNELS_H_
