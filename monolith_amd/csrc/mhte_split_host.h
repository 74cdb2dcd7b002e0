// Host side of split by indices (mhte_split_kernels.h): the checks of the entry points, the one partition pass
// in the workspace's scratch (AuxWs: the histogram of the group sort, the caller's row_splits, the gradient's
// pointer table), the choice of the movers' form and the launch counters.  Included by mhte.hip behind
// mhte_aux_host.h.
#ifndef MHTE_SPLIT_HOST_H_
#define MHTE_SPLIT_HOST_H_

#include "mhte_split_kernels.h"

namespace mhte {

// launches by kernel form, process-wide, read by mhte_split_launch_counts
static std::atomic<int64_t> g_split_launches[kSplitCounters];

static void split_check_ptr(const char* op, const char* name, const void* p, bool needed, unsigned align) {
  if (needed && !p) arg_bad(op, std::string("null argument: ") + name);
  if (reinterpret_cast<uintptr_t>(p) & (align - 1u))
    arg_bad(op, std::string(name) + " must be " + std::to_string(align) + "-byte aligned");
}
static void split_check_n(const char* op, int64_t n) {
  if (n < 0) arg_bad(op, "n must be >= 0, got " + std::to_string(n));
  if (n >= (1ll << 31) - 1) arg_bad(op, "n must be below 2^31 - 1, got " + std::to_string(n));
}
static void split_check_num_splits(const char* op, int32_t num_splits) {
  if (num_splits < 1 || num_splits > kGsMaxBins)
    arg_bad(op, "num_splits must be in [1, " + std::to_string(kGsMaxBins) + "], got " + std::to_string(num_splits));
}

// pos / sizes / split_row_splits / n_bad of one partition: 4 launches (none of the pass for n == 0), no wait
// unless host_out is given
static void split_plan(const int64_t* indices, int64_t n, int32_t num_splits, const int64_t* row_splits,
                       int32_t n_row_splits, int64_t* pos, int64_t* sizes, int64_t* split_row_splits,
                       int64_t* n_bad, int64_t* host_out, void* stream) {
  const char* op = "split_plan";
  split_check_n(op, n);
  split_check_num_splits(op, num_splits);
  if (n_row_splits < 0) arg_bad(op, "n_row_splits must be >= 0, got " + std::to_string(n_row_splits));
  if (!row_splits && n_row_splits) arg_bad(op, "null argument: row_splits");
  if (row_splits && n_row_splits < 1) arg_bad(op, "row_splits needs at least one entry");
  split_check_ptr(op, "indices", indices, n > 0, 8);
  split_check_ptr(op, "pos", pos, n > 0, 8);
  split_check_ptr(op, "sizes", sizes, true, 8);
  split_check_ptr(op, "split_row_splits", split_row_splits, n_row_splits > 0, 8);
  split_check_ptr(op, "n_bad", n_bad, true, 8);
  if (row_splits) {   // (split_by_indices_op.cc:224-238: the boundaries walk 0 .. n without stepping back)
    bool ok = row_splits[0] == 0 && row_splits[n_row_splits - 1] == n;
    for (int32_t t = 1; ok && t < n_row_splits; ++t) ok = row_splits[t] >= row_splits[t - 1];
    if (!ok) arg_bad(op, "The input ragged tensor is invalid.");
  }
  need_device();
  hipStream_t st = S(stream);
  const size_t table = size_t(num_splits) * size_t(n_row_splits);
  if (n == 0) {
    HIP_OK(hipMemsetAsync(sizes, 0, size_t(num_splits) * 8, st));
    if (table) HIP_OK(hipMemsetAsync(split_row_splits, 0, table * 8, st));
    HIP_OK(hipMemsetAsync(n_bad, 0, 8, st));
  } else {
    AuxWs& ws = AuxWs::of(current_device());
    std::lock_guard<std::mutex> g(ws.mu);
    AuxWs::Use use_(ws, st);
    GsPass P{};
    P.limit = uint32_t(num_splits);
    ws.gs_tiles(P, n);
    P.k64 = indices;
    P.pout64 = pos;
    P.shift = 0;
    P.bits = 1;
    while ((1u << P.bits) < P.limit) ++P.bits;
    gs_hist_kernel<true><<<dim3(P.ntiles), kGsThreads, 0, st>>>(P);
    gs_rowscan_kernel<<<dim3(1u << P.bits), 64, 0, st>>>(P);
    gs_scatter_kernel<true><<<dim3(P.ntiles), kGsThreads, 0, st>>>(P);
    HIP_OK(hipGetLastError());
    const int64_t* rs_dev = nullptr;
    if (n_row_splits) {
      ws.split_row_splits.reserve(size_t(n_row_splits));
      PinnedStage::of(current_device()).upload(ws.split_row_splits.p, row_splits, size_t(n_row_splits) * 8, st);
      rs_dev = ws.split_row_splits.p;
    }
    const SplitFinishArgs A{P.tot, 1u << P.bits, uint32_t(num_splits), uint32_t(n), rs_dev, uint32_t(n_row_splits),
                            pos, sizes, split_row_splits, n_bad};
    const uint32_t grid = uint32_t(std::max<size_t>(1, std::min<size_t>((table + kGsThreads - 1) / kGsThreads, 1024)));
    split_finish_kernel<<<grid, kGsThreads, 0, st>>>(A);
    HIP_OK(hipGetLastError());
    g_split_launches[kSplitPlan].fetch_add(1, std::memory_order_relaxed);
    if (n_row_splits) g_split_launches[kSplitPlanRagged].fetch_add(1, std::memory_order_relaxed);
  }
  if (host_out) {   // sizes | split_row_splits | n_bad
    HIP_OK(hipMemcpyAsync(host_out, sizes, size_t(num_splits) * 8, hipMemcpyDeviceToHost, st));
    if (table)
      HIP_OK(hipMemcpyAsync(host_out + num_splits, split_row_splits, table * 8, hipMemcpyDeviceToHost, st));
    HIP_OK(hipMemcpyAsync(host_out + num_splits + table, n_bad, 8, hipMemcpyDeviceToHost, st));
    HIP_OK(hipStreamSynchronize(st));
  }
}

// the words of a row and of the whole tensor, checked
struct SplitRowShape {
  uint32_t row_words;   // 4-byte words per row
  bool whole16;         // the row is whole 16-byte words
};
static SplitRowShape split_row_shape(const char* op, int64_t n, int64_t element_size, int32_t elem_bytes) {
  split_check_n(op, n);
  if (element_size < 1) arg_bad(op, "element_size must be >= 1, got " + std::to_string(element_size));
  if (elem_bytes != 4 && elem_bytes != 8)
    arg_bad(op, "elem_bytes must be 4 (float32) or 8 (int64), got " + std::to_string(elem_bytes));
  const long long lim = (1ll << 32) - 1;
  if (element_size > lim) arg_bad(op, "element_size must be below 2^32, got " + std::to_string(element_size));
  const long long words = element_size * (elem_bytes / 4);
  // n < 2^31 and words < 2^33: the product is below 2^64
  if (words > lim || (unsigned long long)n * (unsigned long long)words > (unsigned long long)lim)
    arg_bad(op, "n * element_size * elem_bytes / 4 = " + std::to_string(n) + " * " + std::to_string(words) +
                    " overflows the kernels' 32-bit word index");
  return SplitRowShape{uint32_t(words), (words & 3) == 0};
}
static inline bool split_ptr16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

static void split_rows(const void* input, int64_t n, int64_t element_size, int32_t elem_bytes, const int64_t* pos,
                       void* packed, void* stream) {
  const char* op = "split_rows";
  const SplitRowShape s = split_row_shape(op, n, element_size, elem_bytes);
  split_check_ptr(op, "input", input, n > 0, 4);
  split_check_ptr(op, "packed", packed, n > 0, 4);
  split_check_ptr(op, "pos", pos, n > 0, 8);
  need_device();
  if (n == 0) return;
  const bool wide = s.whole16 && split_ptr16(input) && split_ptr16(packed);
  const uint32_t chunks = wide ? s.row_words / 4u : s.row_words;
  const SplitRowsArgs A{input, packed, pos, uint32_t(n), chunks, uint32_t(n) * chunks};
  const uint32_t grid = (A.total + kGsThreads - 1) / kGsThreads;
  hipStream_t st = S(stream);
  if (wide) split_rows_kernel<uint4><<<grid, kGsThreads, 0, st>>>(A);
  else split_rows_kernel<uint32_t><<<grid, kGsThreads, 0, st>>>(A);
  HIP_OK(hipGetLastError());
  g_split_launches[wide ? kSplitRows4 : kSplitRows1].fetch_add(1, std::memory_order_relaxed);
}

static void split_rows_grad(const void* const* grads, const int64_t* sizes, int32_t num_splits, int64_t n,
                            int64_t element_size, int32_t elem_bytes, const int64_t* pos, void* input_grads,
                            void* stream) {
  const char* op = "split_rows_grad";
  const SplitRowShape s = split_row_shape(op, n, element_size, elem_bytes);
  split_check_num_splits(op, num_splits);
  if (!grads) arg_bad(op, "null argument: grads");
  split_check_ptr(op, "sizes", sizes, true, 8);
  split_check_ptr(op, "pos", pos, n > 0, 8);
  split_check_ptr(op, "input_grads", input_grads, n > 0, 4);
  bool wide = s.whole16 && split_ptr16(input_grads);
  for (int32_t i = 0; i < num_splits; ++i) {
    split_check_ptr(op, "grads[i]", grads[i], false, 4);
    wide = wide && split_ptr16(grads[i]);
  }
  need_device();
  if (n == 0) return;
  hipStream_t st = S(stream);
  AuxWs& ws = AuxWs::of(current_device());
  std::lock_guard<std::mutex> g(ws.mu);
  AuxWs::Use use_(ws, st);
  ws.split_table.reserve(size_t(num_splits) * sizeof(void*));
  PinnedStage::of(current_device()).upload(ws.split_table.p, grads, size_t(num_splits) * sizeof(void*), st);
  const uint32_t chunks = wide ? s.row_words / 4u : s.row_words;
  const SplitGradArgs A{reinterpret_cast<const void* const*>(ws.split_table.p), sizes, uint32_t(num_splits),
                        input_grads, pos, uint32_t(n), chunks, uint32_t(n) * chunks};
  const uint32_t grid = (A.total + kGsThreads - 1) / kGsThreads;
  if (wide) split_grad_kernel<uint4><<<grid, kGsThreads, 0, st>>>(A);
  else split_grad_kernel<uint32_t><<<grid, kGsThreads, 0, st>>>(A);
  HIP_OK(hipGetLastError());
  g_split_launches[wide ? kSplitGrad4 : kSplitGrad1].fetch_add(1, std::memory_order_relaxed);
}

}  // namespace mhte
#endif  // MHTE_SPLIT_HOST_H_
