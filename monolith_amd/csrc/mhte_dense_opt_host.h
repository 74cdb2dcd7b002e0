// Host side of the dense optimizers (mhte_dense_opt_kernels.h): the checks of the entry points, the table and
// the launch.  Included by mhte.hip behind mhte_aux_host.h and mhte_flat_host.h.
#ifndef MHTE_DENSE_OPT_HOST_H_
#define MHTE_DENSE_OPT_HOST_H_

#include "mhte_dense_opt_kernels.h"

namespace mhte {

// What the two entry points share.  c_needed: Adamom.
struct DenseOptCall {
  float* const* vars;
  const int64_t* lens;
  int32_t n, align_elems;
  float* m;
  float* v;
  float* c;
  int64_t slot_elems;
  const float* const* grads;
  const void* grads_flat;
  int32_t wire;
  const float* grad_scale_dev;
  const float* lr_dev;
  int32_t update_slots, use_v2;
};

// The variables that take part (ChunkTable: inline up to kDenseOptInline, uploaded beyond).
typedef ChunkTable<DenseOptArgs> DenseOptTable;

// InvalidArgument before any device call; builds the table.
static void dense_opt_check(const char* op, const DenseOptCall& q, bool c_needed, DenseOptTable& T) {
  if (!q.vars) arg_bad(op, "null argument: vars");
  if (!q.lens) arg_bad(op, "null argument: lens");
  check_lens(op, "variable", q.lens, q.n);
  for (int32_t i = 0; i < q.n; ++i)
    if (q.lens[i] != 0 && !q.vars[i]) arg_bad(op, "null argument: vars[" + std::to_string(i) + "]");
  if ((q.grads != nullptr) == (q.grads_flat != nullptr))
    arg_bad(op, "exactly one of grads and grads_flat must be given");
  if (q.wire != 0 && q.wire != 1) arg_bad(op, "wire must be 0 (fp32) or 1 (fp16), got " + std::to_string(q.wire));
  if (q.grads && q.wire == 1) arg_bad(op, "the gradient list is fp32: wire 1 needs grads_flat");
  flat_check_align(op, q.align_elems);
  const int64_t total = flat_offsets(op, q.lens, q.n, q.align_elems, nullptr);
  if (q.slot_elems != total)
    arg_bad(op, "slot_elems must be the aligned total " + std::to_string(total) + ", got " +
                    std::to_string(q.slot_elems));
  if (total) {
    if (!q.m) arg_bad(op, "null argument: m");
    if (!q.v) arg_bad(op, "null argument: v");
    if (c_needed && !q.c) arg_bad(op, "null argument: c");
  }
  if (!aligned16(q.m) || !aligned16(q.v) || (c_needed && !aligned16(q.c)))
    arg_bad(op, "the slot buffers must be 16-byte aligned");
  if (q.grads_flat && !aligned16(q.grads_flat)) arg_bad(op, "grads_flat must be 16-byte aligned");
  if (q.update_slots != 0 && q.update_slots != 1)
    arg_bad(op, "update_slots must be 0 or 1, got " + std::to_string(q.update_slots));
  if (q.use_v2 != 0 && q.use_v2 != 1) arg_bad(op, "use_v2 must be 0 or 1, got " + std::to_string(q.use_v2));
  if (!dense_opt_table(q.vars, q.grads, q.lens, q.n, q.align_elems, T))
    arg_bad(op, "more than 2^31 chunks of 4096 elements in one call");
}

template <bool EXT, int KIND>
static void dense_opt_go(const DenseOptTable& T, const DenseOptCall& q, const DenseOptHyper& h, hipStream_t st) {
  const uint32_t grid = std::max<uint32_t>(1, std::min<uint32_t>(T.A.k.n_chunks, kDenseOptMaxGroups));
  const DenseOptBufs B{q.m, q.v, q.c, q.grads_flat};
  const int32_t flags = (q.update_slots ? kDenseUpdateSlots : 0) | (q.use_v2 ? kDenseV2 : 0);
  if (q.grads)
    dense_opt_kernel<EXT, KIND, kDenseGradList><<<grid, kDenseOptThreads, 0, st>>>(T.A, B, h, q.grad_scale_dev,
                                                                                   q.lr_dev, flags);
  else if (q.wire == 0)
    dense_opt_kernel<EXT, KIND, kDenseGradFlat32><<<grid, kDenseOptThreads, 0, st>>>(T.A, B, h, q.grad_scale_dev,
                                                                                     q.lr_dev, flags);
  else
    dense_opt_kernel<EXT, KIND, kDenseGradFlat16><<<grid, kDenseOptThreads, 0, st>>>(T.A, B, h, q.grad_scale_dev,
                                                                                     q.lr_dev, flags);
}
// One launch (none without elements that take part).
template <int KIND>
static void dense_opt_launch(DenseOptTable& T, const DenseOptCall& q, const DenseOptHyper& h, hipStream_t st) {
  if (T.A.k.n_chunks == 0) return;
  chunk_launch(&AuxWs::dense_opt_table, T, st, [&](auto ext) {
    dense_opt_go<decltype(ext)::value, KIND>(T, q, h, st);
  });
  HIP_OK(hipGetLastError());
}

}  // namespace mhte
#endif  // MHTE_DENSE_OPT_HOST_H_
