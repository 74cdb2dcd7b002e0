// Host side of the batch softmax loss (mhte_bsm_kernels.h): the checks of the entry points, the plan
// (mhte_bsm_core.h: a function of batch and dim alone), the workspace, the launches and the launch counters.
// Included by mhte.hip behind mhte_aux_host.h.
#ifndef MHTE_BSM_HOST_H_
#define MHTE_BSM_HOST_H_

#include "mhte_bsm_kernels.h"

namespace mhte {

// launches by kernel form, process-wide, read by mhte_batch_softmax_launch_counts (index: BsmCounter)
static std::atomic<int64_t> g_bsm_launches[kBsmCounters];
static inline void bsm_counted(int i) { g_bsm_launches[i].fetch_add(1, std::memory_order_relaxed); }

static void bsm_check_ptr(const char* op, const char* name, const void* p, bool needed) {
  if (needed && !p) arg_bad(op, std::string("null argument: ") + name);
  if (reinterpret_cast<uintptr_t>(p) & 3u) arg_bad(op, std::string(name) + " must be 4-byte aligned");
}
static void bsm_check_shape(const char* op, int64_t batch, int32_t dim) {
  if (batch < 0) arg_bad(op, "batch must be >= 0, got " + std::to_string(batch));
  if (batch >= kBsmMaxBatch) arg_bad(op, "batch must be below 2^24, got " + std::to_string(batch));
  if (dim < 1 || dim > kBsmMaxDim)
    arg_bad(op, "dim must be in [1, " + std::to_string(kBsmMaxDim) + "], got " + std::to_string(dim));
}
static void bsm_check(const char* op, const float* query, const float* item, const float* interval, const float* r,
                      int64_t batch, int32_t dim, int32_t normalize, float temperature) {
  bsm_check_shape(op, batch, dim);
  if (!(temperature > 0.f)) arg_bad(op, "temperature must be > 0, got " + std::to_string(temperature));
  if (normalize != 0 && normalize != 1) arg_bad(op, "normalize must be 0 or 1, got " + std::to_string(normalize));
  bsm_check_ptr(op, "query", query, batch > 0);
  bsm_check_ptr(op, "item", item, batch > 0);
  bsm_check_ptr(op, "item_step_interval", interval, batch > 0);
  bsm_check_ptr(op, "r", r, batch > 0);
}

template <int NB>
static void bsm_launch_sweeps(const BsmPlan& p, BsmSweepArgs R, BsmSweepArgs Cc, bool fwd, bool dq, bool di,
                              hipStream_t st) {
  const dim3 grid(p.blocks, p.chunks);
  const int threads = 2 * p.row_block;
  if (fwd) {
    bsm_row_kernel<false, NB><<<grid, threads, 0, st>>>(R);
    bsm_counted(kBsmCntRowFwd);
    return;
  }
  if (dq) {
    bsm_row_kernel<true, NB><<<grid, threads, 0, st>>>(R);
    bsm_counted(kBsmCntRowGrad);
  }
  if (di) {
    bsm_col_kernel<NB><<<grid, threads, 0, st>>>(Cc);
    bsm_counted(kBsmCntCol);
  }
}
static void bsm_sweeps(const BsmPlan& p, const BsmSweepArgs& R, const BsmSweepArgs& Cc, bool fwd, bool dq, bool di,
                       hipStream_t st) {
  switch (p.nb) {
    case 1: bsm_launch_sweeps<1>(p, R, Cc, fwd, dq, di, st); break;
    case 2: bsm_launch_sweeps<2>(p, R, Cc, fwd, dq, di, st); break;
    case 4: bsm_launch_sweeps<4>(p, R, Cc, fwd, dq, di, st); break;
    default: bsm_launch_sweeps<8>(p, R, Cc, fwd, dq, di, st); break;
  }
}

// The launches of one call, batch > 0.  loss and / or the gradients: prep, row (forward), final; then one sweep per
// gradient and the final gradient pass.  The workspace grows on the first call of a size (the only allocation) and
// is then reused in stream order.
static void bsm_launch(const float* query, const float* item, const float* interval, const float* r, int64_t batch,
                       int32_t dim, int32_t normalize, float temperature, float grad, const float* grad_dev,
                       float* loss, float* dquery, float* ditem, hipStream_t st) {
  const BsmPlan p = bsm_plan(batch, dim);
  AuxWs& ws = AuxWs::of(current_device());
  std::lock_guard<std::mutex> g(ws.mu);
  ws.bsm.reserve(size_t(p.bytes));
  AuxWs::Use use_(ws, st);
  char* w = ws.bsm.p;
  auto at = [w](uint64_t off) { return reinterpret_cast<float*>(w + off); };
  const uint32_t B = uint32_t(batch), bp = uint32_t(p.bp);

  const BsmPrepArgs P{query, item, interval, at(p.off_inv_q), at(p.off_inv_i), at(p.off_ss_q), at(p.off_ss_i),
                      at(p.off_c), at(p.off_zd), at(p.off_qs), at(p.off_is), B, bp, dim, p.kp, normalize,
                      temperature};
  bsm_prep_kernel<<<(bp + 3) / 4, 256, 0, st>>>(P);
  bsm_counted(kBsmCntPrep);

  const BsmSweepArgs R{at(p.off_qs), at(p.off_is), at(p.off_c), r, at(p.off_lse), at(p.off_ml_m), at(p.off_ml_l),
                       at(p.off_dq_part), B, bp, p.tiles, p.tiles_per_chunk, p.kp};
  const BsmSweepArgs Cc{at(p.off_is), at(p.off_qs), at(p.off_c), r, at(p.off_lse), at(p.off_ml_m), at(p.off_ml_l),
                        at(p.off_di_part), B, bp, p.tiles, p.tiles_per_chunk, p.kp};
  bsm_sweeps(p, R, Cc, true, false, false, st);

  const BsmFinalArgs F{at(p.off_ml_m), at(p.off_ml_l), at(p.off_zd), r, at(p.off_lse), loss, B, bp, p.chunks};
  bsm_final_kernel<<<1, kBsmFinalThreads, 0, st>>>(F);
  bsm_counted(kBsmCntFinalLse);

  if (dquery || ditem) {
    bsm_sweeps(p, R, Cc, false, dquery != nullptr, ditem != nullptr, st);
    const BsmFinalGradArgs G{{query, item},
                             {at(p.off_dq_part), at(p.off_di_part)},
                             {at(p.off_inv_q), at(p.off_inv_i)},
                             {at(p.off_ss_q), at(p.off_ss_i)},
                             {dquery, ditem},
                             grad_dev,
                             grad,
                             temperature,
                             B,
                             bp,
                             p.chunks,
                             dim,
                             p.kp,
                             normalize};
    bsm_final_grad_kernel<<<dim3((B + 3) / 4, 2), 256, 0, st>>>(G);
    bsm_counted(kBsmCntFinalGrad);
  }
  HIP_OK(hipGetLastError());
}

static void bsm_forward(const float* query, const float* item, const float* interval, const float* r, int64_t batch,
                        int32_t dim, int32_t normalize, float temperature, float* loss, float* unit_dquery,
                        float* unit_ditem, void* stream) {
  const char* op = "batch_softmax_loss";
  bsm_check(op, query, item, interval, r, batch, dim, normalize, temperature);
  bsm_check_ptr(op, "loss", loss, true);
  bsm_check_ptr(op, "unit_dquery", unit_dquery, false);
  bsm_check_ptr(op, "unit_ditem", unit_ditem, false);
  need_device();
  hipStream_t st = S(stream);
  if (batch == 0) {   // no launch: the loss of no row
    HIP_OK(hipMemsetAsync(loss, 0, 4, st));
    return;
  }
  bsm_launch(query, item, interval, r, batch, dim, normalize, temperature, 1.f, nullptr, loss, unit_dquery,
             unit_ditem, st);
}

static void bsm_gradient(const float* query, const float* item, const float* interval, const float* r, int64_t batch,
                         int32_t dim, int32_t normalize, float temperature, float grad, const float* grad_dev,
                         float* dquery, float* ditem, void* stream) {
  const char* op = "batch_softmax_loss_grad";
  bsm_check(op, query, item, interval, r, batch, dim, normalize, temperature);
  bsm_check_ptr(op, "grad_dev", grad_dev, false);
  bsm_check_ptr(op, "dquery", dquery, false);
  bsm_check_ptr(op, "ditem", ditem, false);
  if (!dquery && !ditem) arg_bad(op, "null argument: dquery and ditem (at least one is needed)");
  need_device();
  if (batch == 0) return;
  bsm_launch(query, item, interval, r, batch, dim, normalize, temperature, grad, grad_dev, nullptr, dquery, ditem,
             S(stream));
}

static void bsm_plan_out(int64_t batch, int32_t dim, int64_t* out, int32_t n) {
  const char* op = "batch_softmax_plan";
  bsm_check_shape(op, batch, dim);
  if (!out) arg_bad(op, "null argument: out");
  if (n != 5) arg_bad(op, "n must be 5, got " + std::to_string(n));
  const BsmPlan p = bsm_plan(batch, dim);
  out[0] = p.row_block;
  out[1] = p.tile;
  out[2] = p.chunks;   // per row block
  out[3] = p.chunks;   // per column block: the batch is both extents
  out[4] = int64_t(p.bytes);
}

}  // namespace mhte
#endif  // MHTE_BSM_HOST_H_
