// Host side of fused_embedding_to_layout (mhte_layout_kernels.h): plan the call (mhte_layout_plan.h: every check
// and every decision, before anything is enqueued), zero-fill, then either the grouped gradient or the planned
// launches.  What is decided here is grid sizes only.  Included by mhte.hip behind mhte_aux_host.h.
#ifndef MHTE_LAYOUT_HOST_H_
#define MHTE_LAYOUT_HOST_H_

#include "mhte_layout_kernels.h"

namespace mhte {

// SetZeroFunctor: rows without fids stay zero.  One launch per kLayoutZeroBufs buffers; `skip`: buffers a rows
// launch writes in full.
static void layout_zero_buffers(float* const* bufs, const int64_t* lens, int32_t n, const std::vector<char>* skip,
                                hipStream_t st) {
  LayoutZeroArgs Z{};
  int32_t m = 0;
  uint64_t longest = 0;
  auto flush = [&] {
    if (m > 0 && longest > 0) {
      const uint32_t gx = uint32_t(std::min<uint64_t>(512, (longest + 4095) / 4096));
      layout_zero_args_kernel<<<dim3(gx, uint32_t(m)), 256, 0, st>>>(Z);
      HIP_OK(hipGetLastError());
    }
    m = 0;
    longest = 0;
  };
  for (int32_t i = 0; i < n; ++i) {
    if (lens[i] <= 0 || (skip && (*skip)[size_t(i)])) continue;
    Z.p[m] = bufs[i];
    Z.len[m] = uint64_t(lens[i]);
    longest = std::max(longest, Z.len[m]);
    if (++m == kLayoutZeroBufs) flush();
  }
  flush();
}

// More matrices or outputs than the kernel arguments hold: the four pointer tables go to the device for the call
// (A.x_*), and the fill reads the written side's pointers and lengths from them.
static void layout_upload_tables(const LayoutCall& c, const float* const* embeddings, float* const* outputs,
                                 StreamTmp& blob, LayoutArgs& A, hipStream_t st) {
  const size_t n_emb = size_t(c.n_emb), n_out = size_t(c.n_outputs);
  const size_t o_emb = 0, o_out = o_emb + n_emb * 8, o_len = o_out + n_out * 8,
               o_str = o_len + std::max(n_emb, n_out) * 8, o_cnt = o_str + n_emb * 4, total = o_cnt + n_emb * 4;
  std::vector<char> h(total, 0);
  memcpy(h.data() + o_emb, embeddings, n_emb * 8);
  memcpy(h.data() + o_out, outputs, n_out * 8);
  uint64_t* len = reinterpret_cast<uint64_t*>(h.data() + o_len);
  uint32_t* str = reinterpret_cast<uint32_t*>(h.data() + o_str);
  uint32_t* cnt = reinterpret_cast<uint32_t*>(h.data() + o_cnt);
  const int64_t* zlen = c.forward ? c.output_len : c.emb_count;
  const int32_t nz = c.forward ? c.n_outputs : c.n_emb;
  uint64_t longest = 0;
  for (int32_t i = 0; i < nz; ++i) longest = std::max(longest, len[i] = uint64_t(std::max<int64_t>(0, zlen[i])));
  for (int32_t i = 0; i < c.n_emb; ++i) {
    str[i] = uint32_t(c.emb_stride[i]);
    cnt[i] = uint32_t(c.emb_count[i]);
  }
  char* d = blob.alloc(total);
  PinnedStage::of(current_device()).upload(d, h.data(), total, st);   // (no wait for the stream)
  A.x_emb = reinterpret_cast<const float* const*>(d + o_emb);
  A.x_out = reinterpret_cast<float* const*>(d + o_out);
  A.x_stride = reinterpret_cast<const uint32_t*>(d + o_str);
  A.x_count = reinterpret_cast<const uint32_t*>(d + o_cnt);
  if (nz > 0 && longest > 0) {
    const uint32_t gx = uint32_t(std::min<uint64_t>(64, (longest + 1023) / 1024));
    layout_zero_kernel<<<dim3(gx, uint32_t(nz)), 256, 0, st>>>(
        reinterpret_cast<float* const*>(d + (c.forward ? o_out : o_emb)), reinterpret_cast<const uint64_t*>(d + o_len));
    HIP_OK(hipGetLastError());
  }
}

// The gradient without float atomics (general form; MHTE_POOL_ATOMICS=1 keeps the atomic one): the fids grouped by
// embedding row, every row's contributions added in the reference's CPU order.
static void layout_grouped_grad(const LayoutArgs& A, const LayoutPlan& P, hipStream_t st) {
  const int64_t n_fid = A.n_fid;
  const size_t nf = size_t(n_fid);
  const size_t o_task = 0, o_off = o_task + P.tasks.size() * sizeof(LayoutTask), o_idx = o_off + P.t_off.size() * 4,
               o_qf = (o_idx + P.t_idx.size() * 4 + 15) & ~size_t(15), o_qseq = o_qf + nf * 4, o_fnfl = o_qseq + nf * 4,
               o_kflag = o_fnfl + size_t(std::max(1, A.n_feature)) * 4,   // (zeroed from here)
               o_nheavy = o_kflag + nf * 4, o_heavy = o_nheavy + 16, o_cpos = o_heavy + nf * 4, total = o_cpos + nf * 4;
  StreamTmp tmp(st);   // (freed in stream order behind the kernels that read it)
  char* d = tmp.alloc(total);
  std::vector<char> h(o_qf, 0);
  memcpy(h.data() + o_task, P.tasks.data(), P.tasks.size() * sizeof(LayoutTask));
  memcpy(h.data() + o_off, P.t_off.data(), P.t_off.size() * 4);
  if (!P.t_idx.empty()) memcpy(h.data() + o_idx, P.t_idx.data(), P.t_idx.size() * 4);
  PinnedStage::of(current_device()).upload(d, h.data(), o_qf, st);   // (no wait for the stream)
  HIP_OK(hipMemsetAsync(d + o_qf, 0xff, o_kflag - o_qf, st));   // qf = -1, fnfl = ~0
  HIP_OK(hipMemsetAsync(d + o_kflag, 0, o_heavy - o_kflag, st));   // kflag, n_heavy
  AuxWs& ws = AuxWs::of(current_device());
  std::lock_guard<std::mutex> g(ws.mu);
  AuxWs::Use use_(ws, st);
  ws.group(reinterpret_cast<const int64_t*>(A.fid_offset), n_fid, st);
  LayoutLists X{};
  X.tasks = reinterpret_cast<const LayoutTask*>(d + o_task);
  X.nfl_task_off = reinterpret_cast<const uint32_t*>(d + o_off);
  X.nfl_tasks = reinterpret_cast<const uint32_t*>(d + o_idx);
  X.qf = reinterpret_cast<int32_t*>(d + o_qf);
  X.qseq = reinterpret_cast<uint32_t*>(d + o_qseq);
  X.fnfl = reinterpret_cast<uint32_t*>(d + o_fnfl);
  X.ukeys = ws.uids.p;
  X.nu = ws.nu.p;
  X.seg_off = ws.seg_off.p;
  X.seg_pos = ws.seg_pos.p;
  X.inverse = ws.inverse.p;
  X.kflag = reinterpret_cast<uint32_t*>(d + o_kflag);
  X.n_heavy = reinterpret_cast<uint32_t*>(d + o_nheavy);
  X.heavy = reinterpret_cast<uint32_t*>(d + o_heavy);
  X.cpos = reinterpret_cast<uint32_t*>(d + o_cpos);
  const int64_t inst = int64_t(A.n_nfl) * A.batch;
  if (inst > 0) layout_qmap_kernel<<<dim3(uint32_t((inst + 255) / 256)), 256, 0, st>>>(A, X);
  layout_heavy_select_kernel<<<dim3(uint32_t((n_fid + 255) / 256)), 256, 0, st>>>(A, X);
  layout_grad_lists_kernel<<<dim3(uint32_t((n_fid * 16 + 255) / 256)), 256, 0, st>>>(A, X);
  // (heavy rows: persistent workgroups over the list the select kernel made; rows are disjoint
  // from the light ones, so the two launches' order does not matter)
  int cus = 0;
  if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, current_device()) != hipSuccess || cus <= 0)
    cus = 256;
  layout_grad_heavy_kernel<<<dim3(uint32_t(std::min<int64_t>(2 * cus, n_fid / kLayoutLight + 64))), 1024, 0, st>>>(A, X);
  HIP_OK(hipGetLastError());
}

template <bool FORWARD>
static void layout_run_launch(LayoutArgs& A, const LayoutLaunch& L, hipStream_t st) {
  if (L.zero_missing != 0 && L.form != kLayoutFormRows)
    throw Error(MHTE_INTERNAL, "layout: the launch that was to write whole output rows cannot run");
  std::copy(L.task, L.task + L.n_tasks, A.task);
  std::copy(L.unit, L.unit + L.n_units, A.unit);
  A.n_units = L.n_units;
  A.zero_missing = L.zero_missing;
  const dim3 grid(uint32_t((int64_t(A.batch) * 16 + 255) / 256), uint32_t(L.n_units));   // a lane group per (unit, row)
  const dim3 rgrid(uint32_t((int64_t(A.batch) + kLayoutRowsR - 1) / kLayoutRowsR));
  if (L.form == kLayoutFormRows) layout_rows_kernel<FORWARD><<<rgrid, 256, 0, st>>>(A);
  else if (L.form == kLayoutFormCopy) layout_copy_kernel<FORWARD><<<grid, 256, 0, st>>>(A);
  else layout_kernel<FORWARD><<<grid, 256, 0, st>>>(A);
  HIP_OK(hipGetLastError());
}

// forward: embeddings read, outputs written; gradient: `embeddings` the gradient buffers (written), `outputs` the
// output gradients (read)
static void embedding_to_layout(bool forward, const float* const* embeddings, const int32_t* emb_stride,
                                const int64_t* emb_count, int32_t n_emb, const unsigned long long* fid_offset,
                                int64_t n_fid, const int32_t* feature_offset, int64_t n_feature,
                                const uint32_t* nfl_offset, int32_t n_nfl, int32_t batch,
                                const mhte_layout_slice* slices, int32_t n_slices, float* const* outputs,
                                const int64_t* output_len, int32_t n_outputs, int32_t flags, hipStream_t st) {
  static const bool rows_form = !(getenv("MHTE_LAYOUT_ROWS") && atoi(getenv("MHTE_LAYOUT_ROWS")) == 0);
  const LayoutCall c{forward, emb_stride, emb_count, n_emb, reinterpret_cast<const void* const*>(embeddings),
                     reinterpret_cast<const void* const*>(outputs), n_fid, n_feature, n_nfl, batch, slices, n_slices,
                     output_len, n_outputs, flags, rows_form, pool_atomics()};
  LayoutPlan P;
  const std::string bad = layout_plan(c, P);
  if (!bad.empty()) throw Error(MHTE_INVALID_ARGUMENT, bad);
  LayoutArgs A{};
  StreamTmp blob(st);
  if (P.ext) {
    layout_upload_tables(c, embeddings, outputs, blob, A, st);
  } else {
    if (forward) layout_zero_buffers(outputs, output_len, n_outputs, &P.skip_fill, st);
    else layout_zero_buffers(const_cast<float* const*>(embeddings), emb_count, n_emb, nullptr, st);
    for (int32_t i = 0; i < n_emb; ++i) {
      A.emb[i] = embeddings[i];
      A.emb_stride[i] = uint32_t(emb_stride[i]);
      A.emb_count[i] = uint32_t(emb_count[i]);
    }
    for (int32_t i = 0; i < n_outputs; ++i) A.out[i] = outputs[i];
  }
  A.fid_offset = fid_offset;
  A.feature_offset = feature_offset;
  A.nfl_offset = nfl_offset;
  A.n_fid = int32_t(n_fid);
  A.n_feature = int32_t(n_feature);
  A.n_nfl = n_nfl;
  A.batch = batch;
  A.n_emb = n_emb;
  if (P.grouped) layout_grouped_grad(A, P, st);
  for (const LayoutLaunch& L : P.launches) {
    if (forward) layout_run_launch<true>(A, L, st);
    else layout_run_launch<false>(A, L, st);
  }
}

}  // namespace mhte
#endif  // MHTE_LAYOUT_HOST_H_
