// Host side of AutoInt (mhte_autoint_kernels.h): the checks of the entry points, the plan (mhte_autoint_core.h: a
// function of the shape alone), the choice of the kernel instance, its dynamic-LDS attribute and the launch
// counters.  There is no workspace.  Included by mhte.hip behind mhte_can_host.h.
#ifndef MHTE_AUTOINT_HOST_H_
#define MHTE_AUTOINT_HOST_H_

#include "mhte_autoint_kernels.h"

namespace mhte {

// launches by kernel, process-wide, read by mhte_autoint_launch_counts (index: AutoIntCounter)
static std::atomic<int64_t> g_autoint_launches[kAutoIntCounters];

static void autoint_check_extents(const char* op, int64_t B, int32_t n, int32_t k, int32_t L) {
  cin_check_dim(op, "n", n, kAutoIntMaxN);
  cin_check_dim(op, "k", k, kAutoIntMaxK);
  cin_check_dim(op, "layer_num", L, kAutoIntMaxLayers);
  if (B < 0) arg_bad(op, "B must be >= 0, got " + std::to_string(B));
  if (B > kAutoIntMaxBatch) arg_bad(op, "B must be below 2^31, got " + std::to_string(B));
}

// A launch with more than 64 KiB of dynamic LDS needs the attribute on its function: set once per instance and
// device, to the most any plan asks for.
template <typename K>
static void autoint_allow_lds(K kernel, std::atomic<uint64_t>& done) {
  int dev = 0;
  HIP_OK(hipGetDevice(&dev));
  const uint64_t bit = 1ull << (dev & 63);
  if (done.load(std::memory_order_relaxed) & bit) return;
  HIP_OK(hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                             int(kAutoIntMaxLds)));
  done.fetch_or(bit, std::memory_order_relaxed);
}

template <int T, int RT>
static void autoint_launch(bool grad, const AutoIntArgs& A, size_t lds, hipStream_t st) {
  static std::atomic<uint64_t> done[2];
  if (grad) {
    autoint_allow_lds(autoint_bwd_kernel<T, RT>, done[1]);
    autoint_bwd_kernel<T, RT><<<unsigned(A.B), 64 * RT, lds, st>>>(A);
  } else {
    autoint_allow_lds(autoint_fwd_kernel<T, RT>, done[0]);
    autoint_fwd_kernel<T, RT><<<unsigned(A.B), 64 * RT, lds, st>>>(A);
  }
}

// the instance for the plan's tile and row tiles
static void autoint_dispatch(bool grad, const AutoIntPlan& p, const AutoIntArgs& A, hipStream_t st) {
  const size_t lds = grad ? p.lds_grad : p.lds_fwd;
  if (p.tile == 16) return autoint_launch<16, 1>(grad, A, lds, st);
  switch (p.row_tiles) {
    case 1: return autoint_launch<32, 1>(grad, A, lds, st);
    case 2: return autoint_launch<32, 2>(grad, A, lds, st);
    case 3: return autoint_launch<32, 3>(grad, A, lds, st);
    default: return autoint_launch<32, 4>(grad, A, lds, st);
  }
}

static void autoint_forward(const float* x, int64_t B, int32_t n, int32_t k, int32_t L, float* out, float* states,
                            void* stream) {
  const char* op = "autoint_forward";
  autoint_check_extents(op, B, n, k, L);
  fi_check_ptr(op, "x", x, B > 0);
  fi_check_ptr(op, "out", out, B > 0);
  fi_check_ptr(op, "states", states, false);
  need_device();
  if (B == 0) return;   // nothing to write
  AutoIntArgs A{};
  A.x = x, A.out = out, A.states = L > 1 ? states : nullptr;
  A.B = B, A.n = n, A.k = k, A.L = L;
  autoint_dispatch(false, autoint_plan(B, n, k, L), A, S(stream));
  g_autoint_launches[kAutoIntCntForward].fetch_add(1, std::memory_order_relaxed);
  HIP_OK(hipGetLastError());
}

static void autoint_gradient(const float* dout, const float* x, const float* states, const float* out, int64_t B,
                             int32_t n, int32_t k, int32_t L, float* dx, void* stream) {
  const char* op = "autoint_grad";
  autoint_check_extents(op, B, n, k, L);
  if (L == 1 && states) arg_bad(op, "states must be NULL when layer_num is 1");
  fi_check_ptr(op, "dout", dout, B > 0);
  fi_check_ptr(op, "x", x, B > 0);
  fi_check_ptr(op, "states", states, B > 0 && L > 1);
  fi_check_ptr(op, "out", out, B > 0);
  fi_check_ptr(op, "dx", dx, B > 0);
  need_device();
  if (B == 0) return;   // the gradient is empty
  AutoIntArgs A{};
  A.dout = dout, A.x = x, A.statesc = states, A.dx = dx;   // (out is not read: mhte_autoint_core.h)
  A.B = B, A.n = n, A.k = k, A.L = L;
  autoint_dispatch(true, autoint_plan(B, n, k, L), A, S(stream));
  g_autoint_launches[kAutoIntCntGrad].fetch_add(1, std::memory_order_relaxed);
  HIP_OK(hipGetLastError());
}

static void autoint_plan_out(int64_t B, int32_t n, int32_t k, int32_t L, int64_t* out, int32_t n_out) {
  const char* op = "autoint_plan";
  autoint_check_extents(op, B, n, k, L);
  if (!out) arg_bad(op, "null argument: out");
  if (n_out != 7) arg_bad(op, "n_out must be 7, got " + std::to_string(n_out));
  const AutoIntPlan p = autoint_plan(B, n, k, L);
  out[0] = p.tile;
  out[1] = p.row_tiles;
  out[2] = p.padded_k;
  out[3] = p.samples_per_workgroup;
  out[4] = int64_t(p.lds_fwd);
  out[5] = int64_t(p.lds_grad);
  out[6] = int64_t(p.ws_bytes);
}

}  // namespace mhte
#endif  // MHTE_AUTOINT_HOST_H_
