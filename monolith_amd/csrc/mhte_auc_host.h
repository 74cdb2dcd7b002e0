// Host side of the in-batch AUC loss (mhte_auc_kernels.h): the checks of the entry points, the plan
// (mhte_auc_core.h: a function of n alone), the workspace, the launches and the launch counters.  Included by
// mhte.hip behind mhte_aux_host.h.
#ifndef MHTE_AUC_HOST_H_
#define MHTE_AUC_HOST_H_

#include "mhte_auc_kernels.h"

namespace mhte {

// launches by kernel form, process-wide, read by mhte_inbatch_auc_launch_counts (index: AucCounter)
static std::atomic<int64_t> g_auc_launches[kAucCounters];
static inline void auc_counted(int i) { g_auc_launches[i].fetch_add(1, std::memory_order_relaxed); }

static void auc_check_ptr(const char* op, const char* name, const void* p, bool needed) {
  if (needed && !p) arg_bad(op, std::string("null argument: ") + name);
  if (reinterpret_cast<uintptr_t>(p) & 3u) arg_bad(op, std::string(name) + " must be 4-byte aligned");
}
static void auc_check(const char* op, const float* label, const float* logit, int64_t n, float neg_weight) {
  if (n < 0) arg_bad(op, "n must be >= 0, got " + std::to_string(n));
  if (n > (1ll << 31) - 1) arg_bad(op, "n must be below 2^31, got " + std::to_string(n));
  // (the reference's forward CHECKs it and its gradient does not: both entry points refuse it here)
  if (!(neg_weight > 0.f && neg_weight <= 1.f))
    arg_bad(op, "neg_weight must be in (0, 1], got " + std::to_string(neg_weight));
  auc_check_ptr(op, "label", label, n > 0);
  auc_check_ptr(op, "logit", logit, n > 0);
}

// The launches of one call.  loss and / or grad_out; the compaction, the pair kernel, the final pass: five
// launches.  The workspace grows on the first call of a size (the only allocation) and is then reused in stream
// order.
static void auc_launch(const float* label, const float* logit, int64_t n, float neg_weight, float grad,
                       const float* grad_dev, float* loss, float* grad_out, hipStream_t st) {
  const AucPlan p = auc_plan(n);
  AuxWs& ws = AuxWs::of(current_device());
  std::lock_guard<std::mutex> g(ws.mu);
  ws.auc.reserve(size_t(p.bytes));
  AuxWs::Use use_(ws, st);
  char* w = ws.auc.p;
  uint32_t* counts = reinterpret_cast<uint32_t*>(w + p.off_counts);
  uint32_t* tile_counts = reinterpret_cast<uint32_t*>(w + p.off_tile_counts);
  uint32_t* tile_offsets = reinterpret_cast<uint32_t*>(w + p.off_tile_offsets);
  float* pos = reinterpret_cast<float*>(w + p.off_pos);
  float* neg = reinterpret_cast<float*>(w + p.off_neg);
  uint32_t* rank = reinterpret_cast<uint32_t*>(w + p.off_rank);
  double* loss_part = reinterpret_cast<double*>(w + p.off_loss_part);
  double* row_part = reinterpret_cast<double*>(w + p.off_row_part);
  double* col_part = reinterpret_cast<double*>(w + p.off_col_part);
  const uint32_t un = uint32_t(n);

  auc_count_kernel<<<p.scan_tiles, kAucThreads, 0, st>>>(label, un, tile_counts);
  auc_counted(kAucCntCount);
  auc_scan_kernel<<<1, kAucThreads, 0, st>>>(tile_counts, p.scan_tiles, tile_offsets, counts);
  auc_counted(kAucCntScan);
  auc_scatter_kernel<<<p.scan_tiles, kAucThreads, 0, st>>>(label, logit, un, tile_offsets, pos, neg, rank);
  auc_counted(kAucCntScatter);

  const AucPairArgs A{pos, neg, counts, row_part, col_part, loss_part, p.budget};
  const AucFinalArgs F{label, rank, counts, row_part, col_part, loss_part, loss, grad_out, un, grad, grad_dev,
                       neg_weight, p.budget};
  if (loss && grad_out) {
    auc_pair_kernel<true, true><<<p.pair_groups, kAucThreads, 0, st>>>(A);
    auc_counted(kAucCntPairLossGrad);
    auc_final_kernel<true, true><<<p.final_groups, kAucThreads, 0, st>>>(F);
    auc_counted(kAucCntFinalLossGrad);
  } else if (loss) {
    auc_pair_kernel<true, false><<<p.pair_groups, kAucThreads, 0, st>>>(A);
    auc_counted(kAucCntPairLoss);
    auc_final_kernel<true, false><<<1, kAucThreads, 0, st>>>(F);
    auc_counted(kAucCntFinalLoss);
  } else {
    auc_pair_kernel<false, true><<<p.pair_groups, kAucThreads, 0, st>>>(A);
    auc_counted(kAucCntPairGrad);
    auc_final_kernel<false, true><<<p.final_groups, kAucThreads, 0, st>>>(F);
    auc_counted(kAucCntFinalGrad);
  }
  HIP_OK(hipGetLastError());
}

static void auc_forward(const float* label, const float* logit, int64_t n, float neg_weight, float* loss,
                        float* unit_grad, void* stream) {
  const char* op = "inbatch_auc_loss";
  auc_check(op, label, logit, n, neg_weight);
  auc_check_ptr(op, "loss", loss, true);
  auc_check_ptr(op, "unit_grad", unit_grad, false);
  need_device();
  hipStream_t st = S(stream);
  if (n == 0) {   // no launch: the loss of no pair
    HIP_OK(hipMemsetAsync(loss, 0, 4, st));
    return;
  }
  auc_launch(label, logit, n, neg_weight, 1.f, nullptr, loss, unit_grad, st);
}

static void auc_gradient(const float* label, const float* logit, int64_t n, float grad, const float* grad_dev,
                         float neg_weight, float* logit_grad, void* stream) {
  const char* op = "inbatch_auc_loss_grad";
  auc_check(op, label, logit, n, neg_weight);
  auc_check_ptr(op, "grad_dev", grad_dev, false);
  auc_check_ptr(op, "logit_grad", logit_grad, n > 0);
  need_device();
  if (n == 0) return;
  auc_launch(label, logit, n, neg_weight, grad, grad_dev, nullptr, logit_grad, S(stream));
}

}  // namespace mhte
#endif  // MHTE_AUC_HOST_H_
