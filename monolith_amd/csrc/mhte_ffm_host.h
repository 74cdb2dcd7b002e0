// Host side of the FFM feature cross (mhte_ffm_kernels.h): the checks of the entry points, the choice of form
// (mhte_ffm_core.h), the launch and the launch counters.  Included by mhte.hip behind mhte_aux_host.h.
#ifndef MHTE_FFM_HOST_H_
#define MHTE_FFM_HOST_H_

#include "mhte_ffm_kernels.h"

namespace mhte {

// launches by kernel form, process-wide, read by mhte_ffm_launch_counts (index: ffm_counter_index)
static std::atomic<int64_t> g_ffm_launches[kFfmCounters];

// The shapes of a call, checked: InvalidArgument before any device call.
struct FfmShape {
  long long L, R, D, lrd;   // lrd = L R D
  bool dot;
};
static inline bool ffm_aligned4(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 3u) == 0; }
static FfmShape ffm_check_shape(const char* op, int64_t left_cols, int64_t right_cols, int64_t batch,
                                int32_t dim_size, int32_t int_type) {
  if (batch < 0) arg_bad(op, "batch must be >= 0, got " + std::to_string(batch));
  if (left_cols < 0) arg_bad(op, "left_cols must be >= 0, got " + std::to_string(left_cols));
  if (right_cols < 0) arg_bad(op, "right_cols must be >= 0, got " + std::to_string(right_cols));
  if (dim_size < 1) arg_bad(op, "dim_size must be >= 1, got " + std::to_string(dim_size));
  if (int_type != 0 && int_type != 1)
    arg_bad(op, "int_type must be 0 (multiply) or 1 (dot), got " + std::to_string(int_type));
  const long long lim = (1ll << 31) - 1;
  if (batch > lim) arg_bad(op, "batch must be below 2^31, got " + std::to_string(batch));
  if (left_cols > lim) arg_bad(op, "left_cols must be below 2^31, got " + std::to_string(left_cols));
  if (right_cols > lim) arg_bad(op, "right_cols must be below 2^31, got " + std::to_string(right_cols));
  FfmShape s;
  s.D = dim_size;
  s.L = left_cols / dim_size;
  s.R = right_cols / dim_size;
  s.dot = int_type == 1;
  // L D and R D are below 2^31 each, so L R D is below 2^62
  s.lrd = s.L * s.R * s.D;
  if (s.lrd > lim)
    arg_bad(op, "(left_cols / dim_size) * (right_cols / dim_size) * dim_size = " + std::to_string(s.lrd) +
                    " overflows the kernels' 32-bit row index: left_cols, right_cols");
  return s;
}
static void ffm_check_ptr(const char* op, const char* name, const void* p, bool needed) {
  if (needed && !p) arg_bad(op, std::string("null argument: ") + name);
  if (!ffm_aligned4(p)) arg_bad(op, std::string(name) + " must be 4-byte aligned");
}
static inline bool ffm_ptr16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

template <bool DOT, bool LDS>
static void ffm_fwd_go(int vec, uint32_t grid, const FfmFwdArgs& A, hipStream_t st) {
  if (vec == 4) ffm_fwd_kernel<4, DOT, LDS><<<grid, kFfmThreads, 0, st>>>(A);
  else ffm_fwd_kernel<1, DOT, LDS><<<grid, kFfmThreads, 0, st>>>(A);
}
template <bool DOT, bool LDS>
static void ffm_grad_go(int vec, uint32_t grid, const FfmGradArgs& A, hipStream_t st) {
  if (vec == 4) ffm_grad_kernel<4, DOT, LDS><<<grid, kFfmThreads, 0, st>>>(A);
  else ffm_grad_kernel<1, DOT, LDS><<<grid, kFfmThreads, 0, st>>>(A);
}
// workgroups of a launch: one per tile (LDS form) or per 256 output elements (direct form), capped
static uint32_t ffm_grid(const FfmForm& f, long long batch, long long per_row, int cap) {
  const long long work = f.lds ? (batch + f.tile_rows - 1) / f.tile_rows : (batch * per_row + kFfmThreads - 1) / kFfmThreads;
  return uint32_t(std::max<long long>(1, std::min<long long>(work, cap)));
}

// One launch; none for an empty problem.
static void ffm_forward(const float* left, int64_t left_cols, const float* right, int64_t right_cols, int64_t batch,
                        int32_t dim_size, int32_t int_type, float* out, int64_t out_cols, void* stream) {
  const char* op = "ffm";
  const FfmShape s = ffm_check_shape(op, left_cols, right_cols, batch, dim_size, int_type);
  const long long want = s.dot ? s.L * s.R : s.lrd;
  if (out_cols != want)
    arg_bad(op, "out_cols must be " + std::to_string(want) + " (" + (s.dot ? "L * R" : "L * R * dim_size") + "), got " +
                    std::to_string(out_cols));
  ffm_check_ptr(op, "left", left, batch > 0 && left_cols > 0);
  ffm_check_ptr(op, "right", right, batch > 0 && right_cols > 0);
  ffm_check_ptr(op, "out", out, batch > 0 && out_cols > 0);
  need_device();
  if (batch == 0 || s.L == 0 || s.R == 0) return;
  // 16-byte accesses: left and right (staging loads), and out for multiply (dot stores single floats)
  const bool aligned = ffm_ptr16(left) && ffm_ptr16(right) && ((left_cols | right_cols) & 3) == 0 &&
                       (s.dot || ffm_ptr16(out));
  const FfmForm f = ffm_forward_form(s.L, s.R, s.D, aligned);
  const FfmFwdArgs A{left, right, out, left_cols, right_cols, batch,
                     uint32_t(s.L), uint32_t(s.R), uint32_t(s.D), uint32_t(f.tile_rows)};
  const uint32_t grid = ffm_grid(f, batch, want / (s.dot ? 1 : f.vec), kFfmFwdMaxGroups);
  hipStream_t st = S(stream);
  if (s.dot) { if (f.lds) ffm_fwd_go<true, true>(f.vec, grid, A, st); else ffm_fwd_go<true, false>(f.vec, grid, A, st); }
  else { if (f.lds) ffm_fwd_go<false, true>(f.vec, grid, A, st); else ffm_fwd_go<false, false>(f.vec, grid, A, st); }
  HIP_OK(hipGetLastError());
  g_ffm_launches[ffm_counter_index(kFfmForward, s.dot, f)].fetch_add(1, std::memory_order_relaxed);
}

// One launch for both outputs; an empty cross (L == 0 or R == 0) only clears them, without a kernel.
static void ffm_gradient(const float* grad, int64_t grad_cols, const float* left, int64_t left_cols,
                         const float* right, int64_t right_cols, int64_t batch, int32_t dim_size, int32_t int_type,
                         float* left_grad, float* right_grad, void* stream) {
  const char* op = "ffm_grad";
  const FfmShape s = ffm_check_shape(op, left_cols, right_cols, batch, dim_size, int_type);
  if (grad_cols < 0) arg_bad(op, "grad_cols must be >= 0, got " + std::to_string(grad_cols));
  if (grad_cols > (1ll << 31) - 1) arg_bad(op, "grad_cols must be below 2^31, got " + std::to_string(grad_cols));
  const long long feats = s.dot ? grad_cols : grad_cols / dim_size;
  if (feats != s.L * s.R)
    arg_bad(op, "the in/out shape not match: grad_cols gives " + std::to_string(feats) + " features, left_cols and "
                "right_cols give " + std::to_string(s.L) + " * " + std::to_string(s.R));
  ffm_check_ptr(op, "grad", grad, batch > 0 && grad_cols > 0);
  ffm_check_ptr(op, "left", left, batch > 0 && left_cols > 0);
  ffm_check_ptr(op, "right", right, batch > 0 && right_cols > 0);
  ffm_check_ptr(op, "left_grad", left_grad, batch > 0 && left_cols > 0);
  ffm_check_ptr(op, "right_grad", right_grad, batch > 0 && right_cols > 0);
  need_device();
  if (batch == 0 || left_cols + right_cols == 0) return;
  hipStream_t st = S(stream);
  if (s.L == 0 || s.R == 0) {   // no term reaches any element: the reference's setZero is all there is
    if (left_cols) HIP_OK(hipMemsetAsync(left_grad, 0, size_t(batch) * size_t(left_cols) * 4, st));
    if (right_cols) HIP_OK(hipMemsetAsync(right_grad, 0, size_t(batch) * size_t(right_cols) * 4, st));
    return;
  }
  // 16-byte accesses: left, right and both outputs, and grad for multiply (dot reads single floats of it)
  const bool aligned = ffm_ptr16(left) && ffm_ptr16(right) && ffm_ptr16(left_grad) && ffm_ptr16(right_grad) &&
                       ((left_cols | right_cols) & 3) == 0 && (s.dot || (ffm_ptr16(grad) && (grad_cols & 3) == 0));
  const FfmForm f = ffm_grad_form(s.L, s.R, s.D, s.dot, aligned);
  const FfmGradArgs A{grad, left, right, left_grad, right_grad, grad_cols, left_cols, right_cols, batch,
                      uint32_t(s.L), uint32_t(s.R), uint32_t(s.D), uint32_t(f.tile_rows)};
  const uint32_t grid = ffm_grid(f, batch, (left_cols + right_cols) / f.vec, kFfmGradMaxGroups);
  if (s.dot) { if (f.lds) ffm_grad_go<true, true>(f.vec, grid, A, st); else ffm_grad_go<true, false>(f.vec, grid, A, st); }
  else { if (f.lds) ffm_grad_go<false, true>(f.vec, grid, A, st); else ffm_grad_go<false, false>(f.vec, grid, A, st); }
  HIP_OK(hipGetLastError());
  g_ffm_launches[ffm_counter_index(kFfmGradient, s.dot, f)].fetch_add(1, std::memory_order_relaxed);
}

}  // namespace mhte
#endif  // MHTE_FFM_HOST_H_
