// Host side of FeatureInsight (mhte_fi_kernels.h): the checks of the entry points, the plan (mhte_fi_core.h: a
// function of the shape alone), the cut of the segment list into launches, the workspace of the weight gradient and
// the launch counters.  Included by mhte.hip behind mhte_aux_host.h.
#ifndef MHTE_FI_HOST_H_
#define MHTE_FI_HOST_H_

#include "mhte_fi_kernels.h"

namespace mhte {

// launches by kernel form, process-wide, read by mhte_feature_insight_launch_counts (index: FiCounter)
static std::atomic<int64_t> g_fi_launches[kFiCounters];
static inline void fi_counted(int i) { g_fi_launches[i].fetch_add(1, std::memory_order_relaxed); }

constexpr int64_t kFiMaxCols = int64_t(kFiTile) * 65535;   // in_cols and k: their tiles are a grid's z extent

static void fi_check_ptr(const char* op, const char* name, const void* p, bool needed) {
  if (needed && !p) arg_bad(op, std::string("null argument: ") + name);
  if (reinterpret_cast<uintptr_t>(p) & 3u) arg_bad(op, std::string(name) + " must be 4-byte aligned");
}
static void fi_check_extents(const char* op, int64_t batch, int64_t in_cols, int32_t k, int32_t n_segments) {
  if (batch < 0) arg_bad(op, "batch must be >= 0, got " + std::to_string(batch));
  if (batch > kFiMaxExtent) arg_bad(op, "batch must be at most 2^30 - 64, got " + std::to_string(batch));
  if (in_cols < 0 || in_cols > kFiMaxCols)
    arg_bad(op, "in_cols must be in [0, " + std::to_string(kFiMaxCols) + "], got " + std::to_string(in_cols));
  if (k < 1 || k > kFiMaxCols)
    arg_bad(op, "k must be in [1, " + std::to_string(kFiMaxCols) + "], got " + std::to_string(k));
  if (n_segments < 1 || n_segments > kFiMaxSegments)
    arg_bad(op, "n_segments must be in [1, " + std::to_string(kFiMaxSegments) + "], got " +
                    std::to_string(n_segments));
  // every element offset is a 64-bit product of these: the largest array is batch x (n_segments k)
  const int64_t fk = int64_t(n_segments) * k;
  if (batch > 0 && fk > (int64_t(1) << 60) / batch)
    arg_bad(op, "batch * n_segments * k must fit 2^60 elements, got " + std::to_string(batch) + " * " +
                    std::to_string(fk));
}
static void fi_check_segments(const char* op, const int32_t* segment_sizes, int32_t n_segments, int64_t in_cols) {
  if (!segment_sizes) arg_bad(op, "null argument: segment_sizes");
  int64_t sum = 0;
  for (int32_t f = 0; f < n_segments; ++f) {
    if (segment_sizes[f] < 0)
      arg_bad(op, "segment_sizes[" + std::to_string(f) + "] must be >= 0, got " + std::to_string(segment_sizes[f]));
    sum += segment_sizes[f];
  }
  if (sum != in_cols)
    arg_bad(op, "the sum of segment_sizes must be in_cols = " + std::to_string(in_cols) + ", got " +
                    std::to_string(sum));
}

// One launch per group of kFiInline consecutive segments; launch(args, longest segment of the group).
template <class LAUNCH>
static void fi_groups(FiArgs& A, const int32_t* segment_sizes, int32_t n_segments, LAUNCH launch) {
  int64_t o = 0;
  for (int32_t g0 = 0; g0 < n_segments; g0 += kFiInline) {
    const int32_t n = std::min<int32_t>(kFiInline, n_segments - g0);
    A.segs.n = n;
    A.segs.first = g0;
    int32_t longest = 0;
    for (int32_t i = 0; i < n; ++i) {
      A.segs.off[i] = int32_t(o);
      o += segment_sizes[g0 + i];
      longest = std::max(longest, segment_sizes[g0 + i]);
    }
    A.segs.off[n] = int32_t(o);
    launch(A, longest);
  }
}
static inline unsigned fi_tiles(int64_t n) { return unsigned((n + kFiTile - 1) / kFiTile); }

static void fi_forward(const float* input, const float* weight, int64_t batch, int64_t in_cols, int32_t k,
                       const int32_t* segment_sizes, int32_t n_segments, int32_t aggregate, float* out,
                       int64_t out_cols, void* stream) {
  const char* op = "feature_insight";
  fi_check_extents(op, batch, in_cols, k, n_segments);
  fi_check_segments(op, segment_sizes, n_segments, in_cols);
  if (aggregate != 0 && aggregate != 1) arg_bad(op, "aggregate must be 0 or 1, got " + std::to_string(aggregate));
  const int64_t want_cols = aggregate ? int64_t(n_segments) : int64_t(n_segments) * k;
  if (out_cols != want_cols)
    arg_bad(op, "out_cols must be " + std::to_string(want_cols) + (aggregate ? " (n_segments)" : " (n_segments * k)") +
                    ", got " + std::to_string(out_cols));
  fi_check_ptr(op, "input", input, batch > 0 && in_cols > 0);
  fi_check_ptr(op, "weight", weight, in_cols > 0);
  fi_check_ptr(op, "out", out, batch > 0);
  need_device();
  if (batch == 0) return;   // nothing to write
  hipStream_t st = S(stream);
  FiArgs A{};
  A.input = input;
  A.weight = weight;
  A.dst = out;
  A.B = batch, A.E = in_cols, A.K = k, A.FK = int64_t(n_segments) * k, A.F = n_segments;
  fi_groups(A, segment_sizes, n_segments, [&](const FiArgs& a, int32_t) {
    if (aggregate) {
      fi_forward_kernel<true><<<dim3(fi_tiles(batch) * a.segs.n, 1, 1), kFiThreads, 0, st>>>(a);
      fi_counted(kFiCntAggregate);
    } else {
      fi_forward_kernel<false><<<dim3(fi_tiles(batch) * a.segs.n, 1, fi_tiles(k)), kFiThreads, 0, st>>>(a);
      fi_counted(kFiCntForward);
    }
  });
  HIP_OK(hipGetLastError());
}

static void fi_gradient(const float* grad, int64_t grad_cols, const float* input, const float* weight, int64_t batch,
                        int64_t in_cols, int32_t k, const int32_t* segment_sizes, int32_t n_segments,
                        float* input_grad, float* weight_grad, void* stream) {
  const char* op = "feature_insight_grad";
  fi_check_extents(op, batch, in_cols, k, n_segments);
  fi_check_segments(op, segment_sizes, n_segments, in_cols);
  const int64_t fk = int64_t(n_segments) * k;
  if (grad_cols != fk)
    arg_bad(op, "grad_cols must be " + std::to_string(fk) + " (n_segments * k), got " + std::to_string(grad_cols));
  fi_check_ptr(op, "grad", grad, batch > 0);
  fi_check_ptr(op, "input", input, batch > 0 && in_cols > 0);
  fi_check_ptr(op, "weight", weight, in_cols > 0);
  fi_check_ptr(op, "input_grad", input_grad, false);
  fi_check_ptr(op, "weight_grad", weight_grad, false);
  if (!input_grad && !weight_grad && in_cols > 0)   // (with in_cols == 0 both are empty: no pointer to ask for)
    arg_bad(op, "null argument: input_grad and weight_grad (at least one is needed)");
  need_device();
  hipStream_t st = S(stream);
  if (in_cols == 0) return;   // both gradients are empty
  if (batch == 0) {           // the sum over no row
    if (weight_grad) HIP_OK(hipMemsetAsync(weight_grad, 0, size_t(in_cols) * size_t(k) * 4, st));
    return;
  }
  const FiPlan p = fi_plan(batch, in_cols, k, n_segments);
  FiArgs A{};
  A.input = input;
  A.weight = weight;
  A.grad = grad;
  A.B = batch, A.E = in_cols, A.K = k, A.FK = fk, A.F = n_segments;
  A.slab_rows = p.slab_rows, A.slabs = p.slabs;
  if (input_grad) {
    A.dst = input_grad;
    fi_groups(A, segment_sizes, n_segments, [&](const FiArgs& a, int32_t longest) {
      if (!longest) return;
      fi_input_grad_kernel<<<dim3(fi_tiles(batch) * a.segs.n, 1, fi_tiles(longest)), kFiThreads, 0, st>>>(a);
      fi_counted(kFiCntInputGrad);
    });
  }
  if (weight_grad) {
    // the partials of the slabs live in the per-device workspace, which grows on the first call of a size (the
    // only allocation) and is then reused in stream order
    AuxWs& ws = AuxWs::of(current_device());
    std::lock_guard<std::mutex> g(ws.mu);
    if (p.slabs > 1) ws.fi.reserve(size_t(p.grad_bytes));
    AuxWs::Use use_(ws, st);
    float* part = p.slabs > 1 ? reinterpret_cast<float*>(ws.fi.p) : weight_grad;
    A.dst = part;
    const unsigned gx = unsigned(p.slabs) * fi_tiles(k);
    fi_groups(A, segment_sizes, n_segments, [&](const FiArgs& a, int32_t longest) {
      if (!longest) return;
      fi_weight_grad_kernel<<<dim3(gx * a.segs.n, 1, fi_tiles(longest)), kFiThreads, 0, st>>>(a);
      fi_counted(kFiCntWeightGrad);
    });
    if (p.slabs > 1) {
      const int64_t n = in_cols * int64_t(k);
      const unsigned blocks = unsigned(std::min<int64_t>((n + kFiThreads - 1) / kFiThreads, 4096));
      fi_slab_sum_kernel<<<blocks, kFiThreads, 0, st>>>(part, weight_grad, n, int(p.slabs));
      fi_counted(kFiCntSlabSum);
    }
  }
  HIP_OK(hipGetLastError());
}

static void fi_plan_out(int64_t batch, int64_t in_cols, int32_t k, int32_t n_segments, int64_t* out, int32_t n) {
  const char* op = "feature_insight_plan";
  fi_check_extents(op, batch, in_cols, k, n_segments);
  if (!out) arg_bad(op, "null argument: out");
  if (n != 9) arg_bad(op, "n must be 9, got " + std::to_string(n));
  const FiPlan p = fi_plan(batch, in_cols, k, n_segments);
  out[0] = p.row_block;
  out[1] = p.col_tile;
  out[2] = p.stage;
  out[3] = p.inline_segments;
  out[4] = p.groups;
  out[5] = p.slab_rows;
  out[6] = p.slabs;
  out[7] = int64_t(p.forward_bytes);
  out[8] = int64_t(p.grad_bytes);
}

}  // namespace mhte
#endif  // MHTE_FI_HOST_H_
