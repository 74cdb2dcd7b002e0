// Host side of the DCN cross layer (mhte_dcn_kernels.h): the checks of the entry points, the plan
// (mhte_dcn_core.h: a function of the shape alone), the choice of the kernel instance, the workspace of the slab
// partials and the launch counters.  Included by mhte.hip behind mhte_cin_host.h.
#ifndef MHTE_DCN_HOST_H_
#define MHTE_DCN_HOST_H_

#include "mhte_dcn_kernels.h"

namespace mhte {

// launches by kernel form, process-wide, read by mhte_dcn_launch_counts (index: DcnCounter)
static std::atomic<int64_t> g_dcn_launches[kDcnCounters];
static inline void dcn_counted(int i) { g_dcn_launches[i].fetch_add(1, std::memory_order_relaxed); }

static void dcn_check_extents(const char* op, int64_t B, int32_t d, int32_t type) {
  cin_check_dim(op, "d", d, kDcnMaxD);
  if (B < 0) arg_bad(op, "B must be >= 0, got " + std::to_string(B));
  if (B > kDcnMaxElems / d) arg_bad(op, "B * d must be at most 2^31, got " + std::to_string(B) + " * " + std::to_string(d));
  if (type != kDcnVector && type != kDcnMatrix)
    arg_bad(op, "type must be 0 (vector) or 1 (matrix), got " + std::to_string(type));
}

// f(NT): the matrix instance for the plan's column tiles;  f(VPL): the vector instance for its values per lane
#define MHTE_DCN_VPL(vpl, ...)                  \
  do {                                          \
    if ((vpl) == 1) {                           \
      constexpr int VPL = 1;                    \
      __VA_ARGS__;                              \
    } else if ((vpl) == 4) {                    \
      constexpr int VPL = 4;                    \
      __VA_ARGS__;                              \
    } else if ((vpl) == 16) {                   \
      constexpr int VPL = 16;                   \
      __VA_ARGS__;                              \
    } else {                                    \
      constexpr int VPL = 64;                   \
      __VA_ARGS__;                              \
    }                                           \
  } while (0)

static int dcn_shift(int lanes) {
  int s = 0;
  while ((1 << s) < lanes) ++s;
  return s;
}

static void dcn_forward(const float* x0, const float* xl, const float* w, const float* bias, int64_t B, int32_t d,
                        int32_t type, float* xnext, float* aux, void* stream) {
  const char* op = "dcn_layer";
  dcn_check_extents(op, B, d, type);
  fi_check_ptr(op, "x0", x0, B > 0);
  fi_check_ptr(op, "xl", xl, B > 0);
  fi_check_ptr(op, "w", w, true);
  fi_check_ptr(op, "bias", bias, true);
  fi_check_ptr(op, "xnext", xnext, B > 0);
  fi_check_ptr(op, "aux", aux, false);
  need_device();
  if (B == 0) return;   // nothing to write
  const DcnPlan p = dcn_plan(B, d, type);
  DcnArgs A{};
  A.x0 = x0, A.xl = xl, A.w = w, A.bias = bias, A.xnext = xnext, A.aux = aux;
  A.B = B, A.d = d, A.lanes = p.lanes, A.lane_shift = dcn_shift(p.lanes);
  hipStream_t st = S(stream);
  if (type == kDcnMatrix) {
    const dim3 grid(unsigned(fi_ceil(B, kDcnRowBlock)), unsigned(p.cblocks), 1);
    MHTE_CIN_NT(p.col_tiles, { dcn_mat_fwd_kernel<NT><<<grid, 256, 0, st>>>(A); });
    dcn_counted(aux ? kDcnCntMatForward : kDcnCntMatForwardNoAux);
  } else {
    const unsigned grid = unsigned(fi_ceil(B, kDcnVecRows));
    MHTE_DCN_VPL(p.vpl, { dcn_vec_fwd_kernel<VPL><<<grid, 256, 0, st>>>(A); });
    dcn_counted(aux ? kDcnCntVecForward : kDcnCntVecForwardNoAux);
  }
  HIP_OK(hipGetLastError());
}

static void dcn_gradient(const float* dxnext, const float* x0, const float* xl, const float* w, const float* aux,
                         int64_t B, int32_t d, int32_t type, int32_t first, const float* dx0_acc, float* dx0,
                         float* dxl, float* dw, float* dbias, void* stream) {
  const char* op = "dcn_layer_grad";
  dcn_check_extents(op, B, d, type);
  if (!dx0 && !dxl && !dw && !dbias) arg_bad(op, "null argument: dx0, dxl, dw and dbias (at least one is needed)");
  if (dx0 && !aux && B > 0) arg_bad(op, "null argument: aux (dx0 needs what the forward saved)");
  if (first && !dx0) arg_bad(op, "null argument: dx0 (a first layer's input gradient is dx0)");
  fi_check_ptr(op, "dxnext", dxnext, B > 0);
  fi_check_ptr(op, "x0", x0, B > 0);
  fi_check_ptr(op, "xl", xl, B > 0);
  fi_check_ptr(op, "w", w, B > 0);
  fi_check_ptr(op, "aux", aux, false);
  fi_check_ptr(op, "dx0_acc", dx0_acc, false);
  fi_check_ptr(op, "dx0", dx0, false);
  fi_check_ptr(op, "dxl", dxl, false);
  fi_check_ptr(op, "dw", dw, false);
  fi_check_ptr(op, "dbias", dbias, false);
  need_device();
  hipStream_t st = S(stream);
  const int64_t nw = type == kDcnMatrix ? int64_t(d) * d : d;
  if (B == 0) {   // the sums over no row
    if (dw) cin_zero_kernel<<<unsigned(std::min<int64_t>(fi_ceil(nw, 256), 4096)), 256, 0, st>>>(dw, nw);
    if (dbias) cin_zero_kernel<<<unsigned(fi_ceil(d, 256)), 256, 0, st>>>(dbias, d);
    HIP_OK(hipGetLastError());
    return;
  }
  const DcnPlan p = dcn_plan(B, d, type);
  DcnArgs A{};
  A.g = dxnext, A.x0 = x0, A.xl = xl, A.w = w, A.aux_in = aux, A.dx0_acc = dx0_acc;
  A.dx0 = dx0, A.dxl = dxl, A.dw = dw, A.dbias = dbias;
  A.B = B, A.slab_rows = p.slab_rows, A.d = d, A.first = first != 0;
  A.lanes = p.lanes, A.lane_shift = dcn_shift(p.lanes);
  const bool sums = dw || dbias;
  if (type == kDcnMatrix && (dx0 || dxl)) {
    const dim3 grid(unsigned(fi_ceil(B, kDcnRowBlock)), unsigned(p.cblocks), 1);
    MHTE_CIN_NT(p.col_tiles, { dcn_mat_dx_kernel<NT><<<grid, 256, 0, st>>>(A); });
    dcn_counted(kDcnCntMatDx);
  }
  if (sums || type == kDcnVector) {
    // the partials of the slabs live in the per-device workspace, which grows on the first call of a size (the
    // only allocation) and is then reused in stream order
    AuxWs& ws = AuxWs::of(current_device());
    std::lock_guard<std::mutex> g(ws.mu);
    const bool parted = sums && p.slabs > 1;
    if (parted) ws.dcn.reserve(size_t(p.ws_bytes));
    AuxWs::Use use_(ws, st);
    A.part = parted ? reinterpret_cast<float*>(ws.dcn.p) : nullptr;
    if (type == kDcnMatrix) {
      const dim3 grid(unsigned(p.kblocks), unsigned(p.cblocks), unsigned(p.slabs));
      MHTE_CIN_NT(p.col_tiles, { dcn_mat_dw_kernel<NT><<<grid, 256, 0, st>>>(A); });
      dcn_counted(kDcnCntMatDw);
    } else {
      MHTE_DCN_VPL(p.vpl, { dcn_vec_grad_kernel<VPL><<<unsigned(p.slabs), 256, 0, st>>>(A); });
      dcn_counted(kDcnCntVecGrad);
    }
    if (parted) {
      const int64_t n = nw + d;
      cin_slab_sum_kernel<<<unsigned(std::min<int64_t>(fi_ceil(n, 256), 4096)), 256, 0, st>>>(A.part, dw, dbias, nw, n,
                                                                                              int(p.slabs));
      dcn_counted(type == kDcnMatrix ? kDcnCntMatSlabSum : kDcnCntVecSlabSum);
    }
  }
  HIP_OK(hipGetLastError());
}

static void dcn_plan_out(int64_t B, int32_t d, int32_t type, int64_t* out, int32_t n) {
  const char* op = "dcn_plan";
  dcn_check_extents(op, B, d, type);
  if (!out) arg_bad(op, "null argument: out");
  if (n != 6) arg_bad(op, "n must be 6, got " + std::to_string(n));
  const DcnPlan p = dcn_plan(B, d, type);
  out[0] = p.row_block;
  out[1] = p.col_span;
  out[2] = p.k_chunk;
  out[3] = p.slab_rows;
  out[4] = p.slabs;
  out[5] = int64_t(p.ws_bytes);
}

}  // namespace mhte
#endif  // MHTE_DCN_HOST_H_
