// Host side of the CAN co-action unit (mhte_can_kernels.h): the checks of the entry points, the plan
// (mhte_can_core.h: a function of the shape alone), the choice of the kernel instance and the launch counters.
// There is no workspace.  Included by mhte.hip behind mhte_dcn_host.h.
#ifndef MHTE_CAN_HOST_H_
#define MHTE_CAN_HOST_H_

#include "mhte_can_kernels.h"

namespace mhte {

// launches by kernel, process-wide, read by mhte_can_launch_counts (index: CanCounter)
static std::atomic<int64_t> g_can_launches[kCanCounters];

static void can_check_extents(const char* op, int64_t B, int32_t F, int32_t T, int32_t d, int32_t L) {
  cin_check_dim(op, "d", d, kCanMaxD);
  cin_check_dim(op, "layer_num", L, kCanMaxLayers);
  if (F < 1) arg_bad(op, "F must be >= 1, got " + std::to_string(F));
  if (T < 1) arg_bad(op, "T must be >= 1, got " + std::to_string(T));
  if (int64_t(F) * T > kCanMaxRows)
    arg_bad(op, "F * T must be at most 2^30, got " + std::to_string(F) + " * " + std::to_string(T));
  if (B < 0) arg_bad(op, "B must be >= 0, got " + std::to_string(B));
  if (B > kCanMaxBatch) arg_bad(op, "B must be below 2^31, got " + std::to_string(B));
}

// f(PD, LC): the instance for the plan's padded width and the smallest layer capacity that holds L
#define MHTE_CAN_INSTANCE(pd, L, ...)           \
  do {                                          \
    if ((pd) == 16) {                           \
      constexpr int PD = 16;                    \
      MHTE_CAN_LAYERS(L, __VA_ARGS__);          \
    } else {                                    \
      constexpr int PD = 32;                    \
      MHTE_CAN_LAYERS(L, __VA_ARGS__);          \
    }                                           \
  } while (0)
#define MHTE_CAN_LAYERS(L, ...)                 \
  do {                                          \
    if ((L) <= 2) {                             \
      constexpr int LC = 2;                     \
      __VA_ARGS__;                              \
    } else if ((L) <= 4) {                      \
      constexpr int LC = 4;                     \
      __VA_ARGS__;                              \
    } else {                                    \
      constexpr int LC = 8;                     \
      __VA_ARGS__;                              \
    }                                           \
  } while (0)

static CanArgs can_args(const float* user, const float* item, int32_t F, int32_t T, int32_t d, int32_t L,
                        int32_t activation) {
  CanArgs A{};
  A.user = user, A.item = item;
  A.P = int64_t(L) * d * (d + 1);
  A.R = F * T, A.T = T, A.d = d, A.L = L, A.act = activation;
  return A;
}

static void can_forward(const float* user, const float* item, int64_t B, int32_t F, int32_t T, int32_t d, int32_t L,
                        int32_t activation, float* out, void* stream) {
  const char* op = "can_forward";
  can_check_extents(op, B, F, T, d, L);
  cin_check_act(op, activation);
  fi_check_ptr(op, "user", user, B > 0);
  fi_check_ptr(op, "item", item, B > 0);
  fi_check_ptr(op, "out", out, B > 0);
  need_device();
  if (B == 0) return;   // nothing to write
  const CanPlan p = can_plan(B, F, T, d, L);
  CanArgs A = can_args(user, item, F, T, d, L, activation);
  A.out = out;
  hipStream_t st = S(stream);
  if (p.padded_d == 16)
    can_fwd_kernel<16><<<unsigned(B), 64, p.lds_bytes, st>>>(A);
  else
    can_fwd_kernel<32><<<unsigned(B), 64, p.lds_bytes, st>>>(A);
  g_can_launches[kCanCntForward].fetch_add(1, std::memory_order_relaxed);
  HIP_OK(hipGetLastError());
}

static void can_gradient(const float* dout, const float* user, const float* item, int64_t B, int32_t F, int32_t T,
                         int32_t d, int32_t L, int32_t activation, float* duser, float* ditem, void* stream) {
  const char* op = "can_grad";
  can_check_extents(op, B, F, T, d, L);
  cin_check_act(op, activation);
  if (!duser && !ditem) arg_bad(op, "null argument: duser and ditem (at least one is needed)");
  fi_check_ptr(op, "dout", dout, B > 0);
  fi_check_ptr(op, "user", user, B > 0);
  fi_check_ptr(op, "item", item, B > 0);
  fi_check_ptr(op, "duser", duser, false);
  fi_check_ptr(op, "ditem", ditem, false);
  need_device();
  if (B == 0) return;   // both gradients are empty
  const CanPlan p = can_plan(B, F, T, d, L);
  CanArgs A = can_args(user, item, F, T, d, L, activation);
  A.dout = dout, A.duser = duser, A.ditem = ditem;
  hipStream_t st = S(stream);
  MHTE_CAN_INSTANCE(p.padded_d, L, { can_bwd_kernel<PD, LC><<<unsigned(B), 64, p.lds_bytes, st>>>(A); });
  g_can_launches[kCanCntGrad].fetch_add(1, std::memory_order_relaxed);
  HIP_OK(hipGetLastError());
}

static void can_plan_out(int64_t B, int32_t F, int32_t T, int32_t d, int32_t L, int64_t* out, int32_t n) {
  const char* op = "can_plan";
  can_check_extents(op, B, F, T, d, L);
  if (!out) arg_bad(op, "null argument: out");
  if (n != 6) arg_bad(op, "n must be 6, got " + std::to_string(n));
  const CanPlan p = can_plan(B, F, T, d, L);
  out[0] = p.rows_per_tile;
  out[1] = p.padded_d;
  out[2] = p.tiles_per_sample;
  out[3] = p.samples_per_workgroup;
  out[4] = int64_t(p.lds_bytes);
  out[5] = int64_t(p.ws_bytes);
}

}  // namespace mhte
#endif  // MHTE_CAN_HOST_H_
