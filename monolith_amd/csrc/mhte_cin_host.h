// Host side of the CIN layer (mhte_cin_kernels.h): the checks of the entry points, the plan (mhte_cin_core.h: a
// function of the shape alone), the choice of the kernel instance, the workspace of the weight gradient and the
// launch counters.  Included by mhte.hip behind mhte_fi_host.h.
#ifndef MHTE_CIN_HOST_H_
#define MHTE_CIN_HOST_H_

#include "mhte_cin_kernels.h"

namespace mhte {

// launches by kernel form, process-wide, read by mhte_cin_launch_counts (index: CinCounter)
static std::atomic<int64_t> g_cin_launches[kCinCounters];
static inline void cin_counted(int i) { g_cin_launches[i].fetch_add(1, std::memory_order_relaxed); }

static void cin_check_dim(const char* op, const char* name, int64_t v, int64_t hi) {
  if (v < 1 || v > hi)
    arg_bad(op, std::string(name) + " must be in [1, " + std::to_string(hi) + "], got " + std::to_string(v));
}
static void cin_check_extents(const char* op, int64_t B, int32_t m, int32_t D, int32_t H, int32_t U) {
  cin_check_dim(op, "m", m, kCinMaxM);
  cin_check_dim(op, "D", D, kCinMaxD);
  cin_check_dim(op, "H", H, kCinMaxH);
  cin_check_dim(op, "U", U, kCinMaxU);
  if (B < 0) arg_bad(op, "B must be >= 0, got " + std::to_string(B));
  if (B > kCinMaxRows / D) arg_bad(op, "B * D must be at most 2^30, got " + std::to_string(B) + " * " + std::to_string(D));
}
static void cin_check_act(const char* op, int32_t activation) {
  if (activation != 0 && activation != 1)
    arg_bad(op, "activation must be 0 (identity) or 1 (relu), got " + std::to_string(activation));
}

// f(NT): the instance for the plan's column tiles
#define MHTE_CIN_NT(nt, ...)                    \
  do {                                          \
    if ((nt) == 1) {                            \
      constexpr int NT = 1;                     \
      __VA_ARGS__;                              \
    } else if ((nt) == 2) {                     \
      constexpr int NT = 2;                     \
      __VA_ARGS__;                              \
    } else {                                    \
      constexpr int NT = 4;                     \
      __VA_ARGS__;                              \
    }                                           \
  } while (0)

static void cin_forward(const float* x0, const float* xl, const float* w, const float* bias, int64_t B, int32_t m,
                        int32_t D, int32_t H, int32_t U, int32_t activation, float* xnext, float* pooled,
                        void* stream) {
  const char* op = "cin_layer";
  cin_check_extents(op, B, m, D, H, U);
  cin_check_act(op, activation);
  fi_check_ptr(op, "x0", x0, B > 0);
  fi_check_ptr(op, "xl", xl, B > 0);
  fi_check_ptr(op, "w", w, true);
  fi_check_ptr(op, "bias", bias, true);
  fi_check_ptr(op, "xnext", xnext, false);
  fi_check_ptr(op, "pooled", pooled, B > 0);
  need_device();
  if (B == 0) return;   // nothing to write
  const CinPlan p = cin_plan(B, m, D, H, U);
  CinFwdArgs A{x0, xl, w, bias, xnext, pooled, B, m, D, H, U, activation, p.b_per_block, p.mp2, p.hc, p.jc, p.parts};
  const dim3 grid(unsigned(fi_ceil(B, p.b_per_block)), unsigned(p.ublocks), 1);
  hipStream_t st = S(stream);
  MHTE_CIN_NT(p.col_tiles, {
    if (m <= 32)
      cin_fwd_kernel<NT, 32><<<grid, 256, 0, st>>>(A);
    else
      cin_fwd_kernel<NT, 64><<<grid, 256, 0, st>>>(A);
  });
  cin_counted(xnext ? kCinCntForward : kCinCntForwardLast);
  HIP_OK(hipGetLastError());
}

static void cin_gradient(const float* dxnext, const float* dpooled, const float* x0, const float* xl, const float* w,
                         const float* xnext, int64_t B, int32_t m, int32_t D, int32_t H, int32_t U,
                         int32_t activation, float* dx0, float* dxl, float* dw, float* dbias, void* stream) {
  const char* op = "cin_layer_grad";
  cin_check_extents(op, B, m, D, H, U);
  cin_check_act(op, activation);
  if (!dx0 && !dxl && !dw && !dbias) arg_bad(op, "null argument: dx0, dxl, dw and dbias (at least one is needed)");
  if (activation == 1 && !xnext && B > 0) arg_bad(op, "null argument: xnext (relu needs the saved output)");
  fi_check_ptr(op, "dxnext", dxnext, false);
  fi_check_ptr(op, "dpooled", dpooled, B > 0);
  fi_check_ptr(op, "x0", x0, B > 0);
  fi_check_ptr(op, "xl", xl, B > 0);
  fi_check_ptr(op, "w", w, (dx0 || dxl) && B > 0);
  fi_check_ptr(op, "xnext", xnext, false);
  fi_check_ptr(op, "dx0", dx0, false);
  fi_check_ptr(op, "dxl", dxl, false);
  fi_check_ptr(op, "dw", dw, false);
  fi_check_ptr(op, "dbias", dbias, false);
  need_device();
  hipStream_t st = S(stream);
  const int64_t K = int64_t(H) * m;
  if (B == 0) {   // the sums over no row
    if (dw) cin_zero_kernel<<<unsigned(std::min<int64_t>(fi_ceil(K * U, 256), 4096)), 256, 0, st>>>(dw, K * U);
    if (dbias) cin_zero_kernel<<<1, 256, 0, st>>>(dbias, U);
    HIP_OK(hipGetLastError());
    return;
  }
  const CinPlan p = cin_plan(B, m, D, H, U);
  CinGradArgs A{};
  A.dxnext = dxnext, A.dpooled = dpooled, A.x0 = x0, A.xl = xl, A.w = w, A.xnext = xnext;
  A.dx0 = dx0, A.dxl = dxl, A.dw = dw, A.dbias = dbias;
  A.R = B * D, A.slab_rows = p.slab_rows;
  A.m = m, A.D = D, A.H = H, A.U = U, A.K = int(K), A.act = activation;
  if (dx0 || dxl) {
    if (m <= 32)
      cin_dx_kernel<32, 4><<<unsigned(fi_ceil(A.R, 128)), 256, 0, st>>>(A);
    else
      cin_dx_kernel<64, 2><<<unsigned(fi_ceil(A.R, 64)), 128, 0, st>>>(A);
    cin_counted(kCinCntDx);
  }
  if (dw || dbias) {
    // the partials of the slabs live in the per-device workspace, which grows on the first call of a size (the
    // only allocation) and is then reused in stream order
    AuxWs& ws = AuxWs::of(current_device());
    std::lock_guard<std::mutex> g(ws.mu);
    if (p.slabs > 1) ws.cin.reserve(size_t(p.ws_bytes));
    AuxWs::Use use_(ws, st);
    A.part = p.slabs > 1 ? reinterpret_cast<float*>(ws.cin.p) : nullptr;
    const dim3 grid(unsigned(p.kblocks), unsigned(p.ublocks), unsigned(p.slabs));
    MHTE_CIN_NT(p.col_tiles, { cin_dw_kernel<NT><<<grid, 256, 0, st>>>(A); });
    cin_counted(kCinCntDw);
    if (p.slabs > 1) {
      const int64_t n = (K + 1) * U;
      cin_slab_sum_kernel<<<unsigned(std::min<int64_t>(fi_ceil(n, 256), 4096)), 256, 0, st>>>(A.part, dw, dbias, K * U,
                                                                                              n, int(p.slabs));
      cin_counted(kCinCntSlabSum);
    }
  }
  HIP_OK(hipGetLastError());
}

static void cin_plan_out(int64_t B, int32_t m, int32_t D, int32_t H, int32_t U, int64_t* out, int32_t n) {
  const char* op = "cin_plan";
  cin_check_extents(op, B, m, D, H, U);
  if (!out) arg_bad(op, "null argument: out");
  if (n != 6) arg_bad(op, "n must be 6, got " + std::to_string(n));
  const CinPlan p = cin_plan(B, m, D, H, U);
  out[0] = p.row_block;
  out[1] = p.col_tiles;
  out[2] = p.k_chunk;
  out[3] = p.slab_rows;
  out[4] = p.slabs;
  out[5] = int64_t(p.ws_bytes);
}

}  // namespace mhte
#endif  // MHTE_CIN_HOST_H_
