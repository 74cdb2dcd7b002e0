// Kernels of the in-batch AUC loss (mhte_auc_core.h: the contract, the split, the plan).
//
//   auc_count_kernel    classes per tile of kAucScanTile elements
//   auc_scan_kernel     one workgroup: the tiles' offsets, and P and N into two device words
//   auc_scatter_kernel  the positives' and the negatives' logits compacted in element order, every element's rank
//   auc_pair_kernel     every (positive, negative) pair: a tile of one class in registers against a chunk of the
//                       other in LDS; fp64 partial sums per element and chunk, an fp64 loss partial per work item
//   auc_final_kernel    the partials added in chunk / item order, rounded once
//
// The pair kernel makes one sweep for the loss and the positives' sums (positives in registers) and, when a
// gradient is asked for, a second one for the negatives' sums (negatives in registers), both in one launch.  The
// alternative, one sweep with each s reduced across the 64 lanes that hold a negative's positives, costs six
// cross-lane steps of an fp64 add and two moves per wavefront and negative, about as much as the terms
// themselves, and leaves the column sum's order tied to the lane layout; the second sweep repeats the terms,
// needs no cross-lane traffic at all and gives both sums by the same code.
//
// No atomics; nothing but plain loads and stores; every buffer index is bounded by the counts read from the
// device words (P + N <= n) and by the plan's budget (mhte_auc_core.h, auc_split).
#ifndef MHTE_AUC_KERNELS_H_
#define MHTE_AUC_KERNELS_H_

#include "mhte_auc_core.h"

namespace mhte {

// the classes of a thread's four elements, counted into one word: positives low, negatives high (a tile holds
// 1024 elements: neither half overflows its 16 bits)
__device__ __forceinline__ uint32_t auc_pack4(const float* label, uint32_t n, uint32_t e0, int* cls) {
  uint32_t v = 0;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const uint32_t e = e0 + uint32_t(k);
    cls[k] = e < n ? auc_classify(label[e]) : int(kAucIgnored);
    v += cls[k] == kAucPositive ? 1u : (cls[k] == kAucNegative ? 0x10000u : 0u);
  }
  return v;
}

// -> the exclusive prefix of v over the workgroup's threads; *total: the sum.  sh: 2 * kAucThreads words.
__device__ __forceinline__ uint32_t auc_block_scan(uint32_t v, uint32_t* sh, uint32_t* total) {
  const uint32_t tid = threadIdx.x;
  uint32_t* a = sh;
  uint32_t* b = sh + kAucThreads;
  a[tid] = v;
  __syncthreads();
  for (uint32_t d = 1; d < uint32_t(kAucThreads); d <<= 1) {
    b[tid] = a[tid] + (tid >= d ? a[tid - d] : 0u);
    __syncthreads();
    uint32_t* t = a;
    a = b;
    b = t;
  }
  const uint32_t incl = a[tid];
  *total = a[kAucThreads - 1];
  __syncthreads();   // (sh is free again)
  return incl - v;
}

__global__ __launch_bounds__(kAucThreads) void auc_count_kernel(const float* __restrict__ label, uint32_t n,
                                                                uint32_t* __restrict__ tile_counts) {
  __shared__ uint32_t sh[2 * kAucThreads];
  const uint32_t tile = blockIdx.x;   // (the grid is the number of tiles)
  int cls[4];
  const uint32_t v = auc_pack4(label, n, tile * uint32_t(kAucScanTile) + threadIdx.x * 4u, cls);
  uint32_t total;
  (void)auc_block_scan(v, sh, &total);
  if (threadIdx.x == 0) {
    tile_counts[2 * tile] = total & 0xffffu;
    tile_counts[2 * tile + 1] = total >> 16;
  }
}

// One workgroup.  Thread t owns the tiles [t * per, (t + 1) * per): their sums, a scan over the threads, then
// the tiles' exclusive offsets.  counts[0] = P, counts[1] = N.
__global__ __launch_bounds__(kAucThreads) void auc_scan_kernel(const uint32_t* __restrict__ tile_counts, uint32_t tiles,
                                                               uint32_t* __restrict__ tile_offsets,
                                                               uint32_t* __restrict__ counts) {
  __shared__ uint32_t sh[2 * kAucThreads];
  const uint32_t per = (tiles + uint32_t(kAucThreads) - 1) / uint32_t(kAucThreads);
  const uint32_t lo = min(tiles, threadIdx.x * per), hi = min(tiles, lo + per);
  uint32_t p = 0, q = 0;
  for (uint32_t i = lo; i < hi; ++i) {
    p += tile_counts[2 * i];
    q += tile_counts[2 * i + 1];
  }
  uint32_t ptotal, qtotal;
  uint32_t pbase = auc_block_scan(p, sh, &ptotal);
  uint32_t qbase = auc_block_scan(q, sh, &qtotal);
  for (uint32_t i = lo; i < hi; ++i) {
    tile_offsets[2 * i] = pbase;
    tile_offsets[2 * i + 1] = qbase;
    pbase += tile_counts[2 * i];
    qbase += tile_counts[2 * i + 1];
  }
  if (threadIdx.x == 0) {
    counts[0] = ptotal;
    counts[1] = qtotal;
  }
}

// pos[r] / neg[r]: the logit of the r-th positive / negative in element order; rank[e] = r (0 for an ignored e).
__global__ __launch_bounds__(kAucThreads) void auc_scatter_kernel(const float* __restrict__ label,
                                                                  const float* __restrict__ logit, uint32_t n,
                                                                  const uint32_t* __restrict__ tile_offsets,
                                                                  float* __restrict__ pos, float* __restrict__ neg,
                                                                  uint32_t* __restrict__ rank) {
  __shared__ uint32_t sh[2 * kAucThreads];
  const uint32_t tile = blockIdx.x;
  const uint32_t e0 = tile * uint32_t(kAucScanTile) + threadIdx.x * 4u;
  int cls[4];
  const uint32_t v = auc_pack4(label, n, e0, cls);
  uint32_t total;
  const uint32_t excl = auc_block_scan(v, sh, &total);
  uint32_t p = tile_offsets[2 * tile] + (excl & 0xffffu);
  uint32_t q = tile_offsets[2 * tile + 1] + (excl >> 16);
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const uint32_t e = e0 + uint32_t(k);
    if (e >= n) break;
    // (p < P and q < N here, P + N <= n: the offsets count this element)
    if (cls[k] == kAucPositive) {
      pos[p] = logit[e];
      rank[e] = p++;
    } else if (cls[k] == kAucNegative) {
      neg[q] = logit[e];
      rank[e] = q++;
    } else {
      rank[e] = 0;
    }
  }
}

struct AucPairArgs {
  const float* pos;          // [P] compacted logits
  const float* neg;          // [N]
  const uint32_t* counts;    // P, N
  double* row_part;          // [chunks of the negatives][stride of the positives]
  double* col_part;          // [chunks of the positives][stride of the negatives]
  double* loss_part;         // [work items of the first sweep]
  unsigned long long budget; // doubles of row_part and of col_part
};

// One stage: the thread's element a against cnt staged elements of the other class (cnt a multiple of 4; the
// stage's tail holds NaN, whose terms are +0).  SWAP: a is the negative.  Sums in ascending order of the stage.
template <bool SWAP, bool LOSS>
__device__ __forceinline__ void auc_stage(float a, const float* sb, uint32_t cnt, double* ts, double* ss) {
  double t_acc = *ts, s_acc = *ss;
  for (uint32_t j = 0; j < cnt; j += 4) {
    float t[4], s[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const float b = sb[j + uint32_t(k)];
      auc_terms(SWAP ? b - a : a - b, &t[k], &s[k]);
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      if (LOSS) t_acc += double(t[k]);
      s_acc += double(s[k]);
    }
  }
  *ts = t_acc;
  *ss = s_acc;
}

// LOSS: the first sweep leaves a loss partial per work item.  GRAD: the first sweep stores the positives' partial
// sums, and a second sweep, the classes' roles swapped, the negatives'.  At least one of the two.
template <bool LOSS, bool GRAD>
__global__ __launch_bounds__(kAucThreads) void auc_pair_kernel(AucPairArgs A) {
  __shared__ float sb[kAucStage];
  __shared__ double red[kAucThreads];
  const uint32_t tid = threadIdx.x;
  const uint32_t P = A.counts[0], N = A.counts[1];
  const AucSplit s0 = auc_split(P, N, A.budget);
  const AucSplit s1 = auc_split(N, P, A.budget);
  const uint64_t items0 = auc_items(s0);
  const uint64_t items = items0 + (GRAD ? auc_items(s1) : 0ull);
  for (uint64_t it = blockIdx.x; it < items; it += gridDim.x) {
    const bool swap = it >= items0;   // (the same in every thread of the workgroup)
    const AucSplit s = swap ? s1 : s0;
    const uint64_t k = swap ? it - items0 : it;
    const uint32_t c = uint32_t(k / s.a_tiles), at = uint32_t(k % s.a_tiles);
    const float* ra = swap ? A.neg : A.pos;
    const float* rb = swap ? A.pos : A.neg;
    const uint32_t na = swap ? N : P, nb = swap ? P : N;
    const uint32_t ai = at * uint32_t(kAucTile) + tid;
    const float a = ai < na ? ra[ai] : __builtin_nanf("");   // (a NaN element's terms are +0)
    const uint32_t b0 = c * s.chunk_len;                      // (c < chunks: b0 < nb)
    const uint32_t b1 = min(nb, b0 + s.chunk_len);
    double ts = 0.0, ss = 0.0;
    for (uint32_t base = b0; base < b1; base += uint32_t(kAucStage)) {
      const uint32_t cnt = min(uint32_t(kAucStage), (b1 - base + 3u) & ~3u);
      __syncthreads();   // (the stage before is read)
      for (uint32_t j = tid; j < cnt; j += uint32_t(kAucThreads)) sb[j] = base + j < b1 ? rb[base + j] : __builtin_nanf("");
      __syncthreads();
      if (swap) auc_stage<true, false>(a, sb, cnt, &ts, &ss);
      else auc_stage<false, LOSS>(a, sb, cnt, &ts, &ss);
    }
    if (GRAD && ai < na) (swap ? A.col_part : A.row_part)[uint64_t(c) * s.stride + ai] = ss;   // (< chunks * stride <= budget)
    if (LOSS && !swap) {   // the workgroup's 256 sums, one fixed tree
      red[tid] = ts;
      __syncthreads();
      for (uint32_t d = uint32_t(kAucThreads) / 2; d > 0; d >>= 1) {
        if (tid < d) red[tid] += red[tid + d];
        __syncthreads();
      }
      if (tid == 0) A.loss_part[k] = red[0];   // (k < items0 <= budget / kAucTile)
    }
  }
}

struct AucFinalArgs {
  const float* label;
  const uint32_t* rank;
  const uint32_t* counts;
  const double* row_part;
  const double* col_part;
  const double* loss_part;
  float* loss;             // LOSS
  float* grad_out;         // GRAD: [n]
  uint32_t n;
  float grad;
  const float* grad_dev;   // replaces grad when not null
  float neg_weight;
  unsigned long long budget;
};

// Workgroup 0 adds the loss partials in item order (thread t the items t, t + 256, ..., then one tree); every
// workgroup adds its elements' partials in chunk order.
template <bool LOSS, bool GRAD>
__global__ __launch_bounds__(kAucThreads) void auc_final_kernel(AucFinalArgs A) {
  __shared__ double red[kAucThreads];
  const uint32_t tid = threadIdx.x;
  const uint32_t P = A.counts[0], N = A.counts[1];
  const AucSplit s0 = auc_split(P, N, A.budget);
  if (LOSS && blockIdx.x == 0) {
    const uint64_t items0 = auc_items(s0);
    double acc = 0.0;
    for (uint64_t i = tid; i < items0; i += uint64_t(kAucThreads)) acc += A.loss_part[i];
    red[tid] = acc;
    __syncthreads();
    for (uint32_t d = uint32_t(kAucThreads) / 2; d > 0; d >>= 1) {
      if (tid < d) red[tid] += red[tid + d];
      __syncthreads();
    }
    if (tid == 0) A.loss[0] = float(red[0]);
  }
  if (GRAD) {
    const AucSplit s1 = auc_split(N, P, A.budget);
    const double g = double(A.grad_dev ? A.grad_dev[0] : A.grad);
    const double gneg = -(g * double(A.neg_weight));
    for (uint64_t e = uint64_t(blockIdx.x) * uint64_t(kAucThreads) + tid; e < A.n;
         e += uint64_t(gridDim.x) * uint64_t(kAucThreads)) {
      const int cls = auc_classify(A.label[e]);
      float out = 0.f;
      if (cls != kAucIgnored && P != 0 && N != 0) {
        const bool isp = cls == kAucPositive;
        const AucSplit s = isp ? s0 : s1;
        const double* part = (isp ? A.row_part : A.col_part) + A.rank[e];   // (rank < the class's count <= stride)
        double sum = 0.0;
        for (uint32_t c = 0; c < s.chunks; ++c) sum += part[uint64_t(c) * s.stride];
        out = auc_grad_round(sum, isp ? g : gneg);
      }
      A.grad_out[e] = out;
    }
  }
}

}  // namespace mhte
#endif  // MHTE_AUC_KERNELS_H_
