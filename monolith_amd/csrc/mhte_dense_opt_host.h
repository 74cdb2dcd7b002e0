// Host side of the dense optimizers (mhte_dense_opt_kernels.h): the checks of the entry points, the table and
// the launch.  Included by mhte.hip behind mhte_flat_host.h.
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

// The variables that take part: up to kDenseOptInline of them travel in the kernel arguments; a longer table
// is uploaded (dense_opt_upload).
struct DenseOptTable {
  DenseOptArgs A{};
  std::vector<DenseOptEntry> entries;
  bool ext() const { return entries.size() > size_t(kDenseOptInline); }
};

// InvalidArgument before any device call; builds the table.
static void dense_opt_check(const char* op, const DenseOptCall& q, bool c_needed, DenseOptTable& T) {
  if (!q.vars) clip_bad(op, "null argument: vars");
  if (!q.lens) clip_bad(op, "null argument: lens");
  if (q.n < 0) clip_bad(op, "n must be >= 0, got " + std::to_string(q.n));
  for (int32_t i = 0; i < q.n; ++i)
    if (q.lens[i] < 0)
      clip_bad(op, "variable " + std::to_string(i) + " has the negative length " + std::to_string(q.lens[i]));
  for (int32_t i = 0; i < q.n; ++i)
    if (q.lens[i] != 0 && !q.vars[i]) clip_bad(op, "null argument: vars[" + std::to_string(i) + "]");
  if ((q.grads != nullptr) == (q.grads_flat != nullptr))
    clip_bad(op, "exactly one of grads and grads_flat must be given");
  if (q.wire != 0 && q.wire != 1) clip_bad(op, "wire must be 0 (fp32) or 1 (fp16), got " + std::to_string(q.wire));
  if (q.grads && q.wire == 1) clip_bad(op, "the gradient list is fp32: wire 1 needs grads_flat");
  flat_check_align(op, q.align_elems);
  const int64_t total = flat_offsets(op, q.lens, q.n, q.align_elems, nullptr);
  if (q.slot_elems != total)
    clip_bad(op, "slot_elems must be the aligned total " + std::to_string(total) + ", got " +
                     std::to_string(q.slot_elems));
  if (total) {
    if (!q.m) clip_bad(op, "null argument: m");
    if (!q.v) clip_bad(op, "null argument: v");
    if (c_needed && !q.c) clip_bad(op, "null argument: c");
  }
  if (!aligned16(q.m) || !aligned16(q.v) || (c_needed && !aligned16(q.c)))
    clip_bad(op, "the slot buffers must be 16-byte aligned");
  if (q.grads_flat && !aligned16(q.grads_flat)) clip_bad(op, "grads_flat must be 16-byte aligned");
  if (q.update_slots != 0 && q.update_slots != 1)
    clip_bad(op, "update_slots must be 0 or 1, got " + std::to_string(q.update_slots));
  if (q.use_v2 != 0 && q.use_v2 != 1) clip_bad(op, "use_v2 must be 0 or 1, got " + std::to_string(q.use_v2));
  uint32_t chunks = 0;
  if (!dense_opt_table(q.vars, q.grads, q.lens, q.n, q.align_elems, T.entries, &chunks))
    clip_bad(op, "more than 2^31 chunks of 4096 elements in one call");
  T.A.n_tensors = uint32_t(T.entries.size());
  T.A.n_chunks = chunks;
  if (!T.ext()) {
    for (size_t i = 0; i < T.entries.size(); ++i) {
      const DenseOptEntry& e = T.entries[i];
      T.A.var[i] = e.var;
      T.A.grad[i] = e.grad;
      T.A.len[i] = e.len;
      T.A.off[i] = e.off;
      T.A.chunk0[i] = e.chunk0;
    }
  }
}

// more than kDenseOptInline variables: the table goes to the workspace's buffer (the caller holds ws.mu and
// has entered the stream), through pinned staging — no wait for the stream
static void dense_opt_upload(AuxWs& ws, DenseOptTable& T, hipStream_t st) {
  const size_t m = T.entries.size();
  const size_t total = m * (4 * 8 + 4);
  ws.dense_opt_table.reserve(total);
  std::vector<char> h(total);
  char* hv = h.data();
  for (size_t i = 0; i < m; ++i) {
    const DenseOptEntry& e = T.entries[i];
    memcpy(hv + i * 8, &e.var, 8);
    memcpy(hv + m * 8 + i * 8, &e.grad, 8);
    memcpy(hv + m * 16 + i * 8, &e.len, 8);
    memcpy(hv + m * 24 + i * 8, &e.off, 8);
    memcpy(hv + m * 32 + i * 4, &e.chunk0, 4);
  }
  PinnedStage::of(current_device()).upload(ws.dense_opt_table.p, hv, total, st);
  char* d = ws.dense_opt_table.p;
  T.A.x_var = reinterpret_cast<float* const*>(d);
  T.A.x_grad = reinterpret_cast<const float* const*>(d + m * 8);
  T.A.x_len = reinterpret_cast<const long long*>(d + m * 16);
  T.A.x_off = reinterpret_cast<const long long*>(d + m * 24);
  T.A.x_chunk0 = reinterpret_cast<const uint32_t*>(d + m * 32);
}

template <bool EXT, int KIND>
static void dense_opt_go(const DenseOptTable& T, const DenseOptCall& q, const DenseOptHyper& h, hipStream_t st) {
  const uint32_t grid = std::max<uint32_t>(1, std::min<uint32_t>(T.A.n_chunks, kDenseOptMaxGroups));
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
  if (T.A.n_chunks == 0) return;
  if (T.ext()) {
    AuxWs& ws = AuxWs::of(current_device());
    std::lock_guard<std::mutex> g(ws.mu);
    AuxWs::Use use_(ws, st);
    dense_opt_upload(ws, T, st);
    dense_opt_go<true, KIND>(T, q, h, st);
  } else {
    dense_opt_go<false, KIND>(T, q, h, st);
  }
  HIP_OK(hipGetLastError());
}

}  // namespace mhte
#endif  // MHTE_DENSE_OPT_HOST_H_
