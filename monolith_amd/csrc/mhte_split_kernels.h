// Split by indices: MonolithSplitByIndices, its gradient and MonolithRaggedSplitByIndices
// (runtime/ops/split_by_indices_op.cc:28-118, :188-243) — the shard split of the parameter-server path.
//
// The reference walks the elements in order, so inside a split they keep their input order.  Here that order
// is the stable permutation pos[]: split after split, and inside a split the input positions ascending.  It is
// ONE digit pass of the stable radix sort (mhte_group_kernels.h) in its SPLIT form — histogram columns per tile,
// a row scan per bin, the in-order walk with ballot ranking; no atomic decides an order — with the split index
// as the digit (<= 10 bits: kGsMaxBins splits).  An index outside [0, num_splits) is no key of the pass: it is
// counted nowhere but in n_bad and stored nowhere.
//
//   split_finish_kernel   sizes[] and n_bad from the pass's bin totals; pos[] behind the last placed element
//                         <- -1; with a ragged input, the boundary table: entry [s][t] is the number of elements
//                         of split s whose position is < row_splits[t] — positions ascend inside a split, so a
//                         lower bound inside the split's range of pos[] finds it
//   split_rows_kernel     packed[q, :] = input[pos[q], :]
//   split_grad_kernel     input_grads[pos[q], :] = grads[s][q - off[s], :], s found in the scan of sizes[]
// The movers copy rows as 4-byte words or, when the row is whole 16-byte words and every buffer is 16-byte
// aligned, as those; the bits are the same.  An entry of pos[] outside [0, n) moves nothing.
#ifndef MHTE_SPLIT_KERNELS_H_
#define MHTE_SPLIT_KERNELS_H_

#include "mhte_group_kernels.h"

namespace mhte {

// launch counters (mhte_split_launch_counts), index:
enum { kSplitRows1 = 0, kSplitRows4, kSplitGrad1, kSplitGrad4, kSplitPlan, kSplitPlanRagged, kSplitCounters };

struct SplitFinishArgs {
  const uint32_t* tot;          // [bins]: the pass's bin totals (bins >= num_splits: the bins beyond hold 0)
  uint32_t bins, num_splits, n;
  const int64_t* row_splits;    // [n_row_splits] on the device, or null
  uint32_t n_row_splits;
  int64_t* pos;                 // [n]
  int64_t* sizes;               // [num_splits]
  int64_t* split_row_splits;    // [num_splits][n_row_splits]
  int64_t* n_bad;               // [1]
};

__global__ __launch_bounds__(kGsThreads) void split_finish_kernel(SplitFinishArgs A) {
  __shared__ uint32_t off[kGsMaxBins + 1];
  __shared__ uint32_t wsum[kGsWaves];
  gs_bin_starts(A.tot, A.bins, off, wsum);
  __syncthreads();
  uint32_t placed = 0;
#pragma unroll
  for (int x = 0; x < kGsWaves; ++x) placed += wsum[x];
  if (threadIdx.x == 0) off[A.bins] = placed;   // (off[num_splits .. bins] all equal `placed`)
  __syncthreads();
  if (blockIdx.x == 0) {
    for (uint32_t s = threadIdx.x; s < A.num_splits; s += kGsThreads) A.sizes[s] = int64_t(off[s + 1] - off[s]);
    if (threadIdx.x == 0) A.n_bad[0] = int64_t(A.n - placed);
  }
  const uint32_t tid = blockIdx.x * kGsThreads + threadIdx.x, nthreads = gridDim.x * kGsThreads;
  // (n < 2^31 and nthreads <= 2^18: the sums below stay in 32 bits)
  for (uint32_t q = placed + tid; q < A.n; q += nthreads) A.pos[q] = -1;
  const uint32_t entries = A.num_splits * A.n_row_splits;
  for (uint32_t e = tid; e < entries; e += nthreads) {
    const uint32_t s = e / A.n_row_splits, t = e - s * A.n_row_splits;
    const int64_t edge = A.row_splits[t];
    uint32_t lo = off[s], hi = off[s + 1];
    while (lo < hi) {
      const uint32_t mid = lo + (hi - lo) / 2u;
      if (A.pos[mid] < edge) lo = mid + 1u; else hi = mid;
    }
    A.split_row_splits[e] = int64_t(lo - off[s]);
  }
}

struct SplitRowsArgs {
  const void* src;       // [n][chunks] words of W
  void* dst;             // [n][chunks]
  const int64_t* pos;    // [n]
  uint32_t n, chunks;
  uint32_t total;        // n * chunks (the host keeps it below 2^32)
};

template <class W>
__global__ __launch_bounds__(kGsThreads) void split_rows_kernel(SplitRowsArgs A) {
  const uint32_t idx = blockIdx.x * kGsThreads + threadIdx.x;
  if (idx >= A.total) return;
  const uint32_t q = idx / A.chunks, c = idx - q * A.chunks;
  const int64_t p = A.pos[q];
  if (uint64_t(p) >= uint64_t(A.n)) return;
  static_cast<W*>(A.dst)[idx] = static_cast<const W*>(A.src)[size_t(p) * A.chunks + c];
}

struct SplitGradArgs {
  const void* const* grads;   // [num_splits] device pointers, on the device: split s is [sizes[s]][chunks] words
  const int64_t* sizes;       // [num_splits]
  uint32_t num_splits;
  void* dst;                  // [n][chunks]
  const int64_t* pos;         // [n]
  uint32_t n, chunks;
  uint32_t total;             // n * chunks
};

template <class W>
__global__ __launch_bounds__(kGsThreads) void split_grad_kernel(SplitGradArgs A) {
  __shared__ uint32_t off[kGsMaxBins + 1];
  __shared__ uint32_t wsum[kGsWaves];
  gs_bin_starts(A.sizes, A.num_splits, off, wsum);
  __syncthreads();
  if (threadIdx.x == 0) off[A.num_splits] = wsum[0] + wsum[1] + wsum[2] + wsum[3];
  __syncthreads();
  static_assert(kGsWaves == 4, "the sum above");
  const uint32_t idx = blockIdx.x * kGsThreads + threadIdx.x;
  if (idx >= A.total) return;
  const uint32_t q = idx / A.chunks, c = idx - q * A.chunks;
  if (q >= off[A.num_splits]) return;   // behind the last placed element
  uint32_t lo = 0, hi = A.num_splits - 1u;   // the split s with off[s] <= q < off[s + 1]
  while (lo < hi) {
    const uint32_t mid = (lo + hi) / 2u;
    if (off[mid + 1] <= q) lo = mid + 1u; else hi = mid;
  }
  const int64_t p = A.pos[q];
  if (uint64_t(p) >= uint64_t(A.n)) return;
  const W* g = static_cast<const W*>(A.grads[lo]);
  static_cast<W*>(A.dst)[size_t(p) * A.chunks + c] = g[size_t(q - off[lo]) * A.chunks + c];
}

}  // namespace mhte
#endif  // MHTE_SPLIT_KERNELS_H_
