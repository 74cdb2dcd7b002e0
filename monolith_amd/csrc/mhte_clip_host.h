// Host side of clip by global norm (mhte_clip_kernels.h): the checks of the entry points, the tensor table
// and the launches.  Included by mhte.hip behind mhte_aux_host.h.
#ifndef MHTE_CLIP_HOST_H_
#define MHTE_CLIP_HOST_H_

#include "mhte_clip_kernels.h"

namespace mhte {

// InvalidArgument before any device call.  outputs: NULL for an entry point that has none.  The caller has
// already refused its own null arguments (the lists, result, a device scalar).
static void clip_check(const char* op, const float* const* inputs, const char* in_name, float* const* outputs,
                       const int64_t* lens, int32_t n, bool has_clip_norm, float clip_norm) {
  check_lens(op, "tensor", lens, n);
  for (int32_t i = 0; i < n; ++i) {
    if (lens[i] == 0) continue;
    if (!inputs[i]) arg_bad(op, std::string("null argument: ") + in_name + "[" + std::to_string(i) + "]");
    if (outputs && !outputs[i]) arg_bad(op, "null argument: outputs[" + std::to_string(i) + "]");
  }
  if (has_clip_norm && !(clip_norm >= 0.f))
    arg_bad(op, "clip_norm must be >= 0 and not NaN, got " + std::to_string(clip_norm));
}

// The non-empty tensors of a call, in list order (ChunkTable: inline up to kClipInline, uploaded beyond).
struct ClipTable : ChunkTable<ClipArgs> {
  bool all_inplace = true;
};
// skip_inplace: tensors whose output is their input are left out (the host knows that nothing is clipped)
static void clip_entries(ClipTable& T, const char* op, const float* const* inputs, float* const* outputs,
                         const int64_t* lens, int32_t n, bool skip_inplace) {
  for (int32_t i = 0; i < n; ++i) {
    if (lens[i] == 0) continue;
    float* o = outputs ? outputs[i] : nullptr;
    const bool inplace = o == inputs[i];
    if (skip_inplace && inplace) continue;
    if (outputs && !inplace) T.all_inplace = false;
    const void* const p[2] = {inputs[i], o};
    if (!T.add(p, lens[i])) arg_bad(op, "more than 2^31 chunks of 4096 floats in one call");
  }
}

static uint32_t clip_scale_grid(const ClipTable& T) {
  return std::max<uint32_t>(1, std::min<uint32_t>(T.A.k.n_chunks, kClipScaleGroups));
}

// The norm: the partials launch, then the finish as a launch of its own (fused == false; result gets
// [sum, norm, scale, 0]) or as the prologue of the scale launch.  Two launches, nothing allocated after the
// first call, no wait.
static void clip_norm_launch(ClipTable& T, float clip_norm, float* result, bool fused, hipStream_t st) {
  AuxWs& ws = AuxWs::of(current_device());
  std::lock_guard<std::mutex> g(ws.mu);   // (for the partials, whether or not the table is uploaded)
  AuxWs::Use use_(ws, st);
  ws.clip_partials.reserve(kClipGroups);
  if (T.ext()) chunk_upload(ws.clip_table, T, st);
  with_flag(T.ext(), [&](auto ext) {
    constexpr bool EXT = decltype(ext)::value;
    clip_partials_kernel<EXT><<<kClipGroups, kClipThreads, 0, st>>>(T.A, ws.clip_partials.p);
    if (!fused)
      clip_finish_kernel<<<1, kClipThreads, 0, st>>>(ws.clip_partials.p, clip_norm, result);
    else
      clip_scale_kernel<EXT><<<clip_scale_grid(T), kClipThreads, 0, st>>>(
          T.A, kClipScalePartials, 1.f, ws.clip_partials.p, clip_norm, result, T.all_inplace ? 1 : 0);
  });
  HIP_OK(hipGetLastError());
}

// The multiply alone: one launch (none without elements).
static void clip_scale_launch(ClipTable& T, int32_t mode, float scale, const float* src, float clip_norm,
                              hipStream_t st) {
  if (T.A.k.n_chunks == 0) return;
  chunk_launch(&AuxWs::clip_table, T, st, [&](auto ext) {
    clip_scale_kernel<decltype(ext)::value><<<clip_scale_grid(T), kClipThreads, 0, st>>>(
        T.A, mode, scale, src, clip_norm, nullptr, T.all_inplace ? 1 : 0);
  });
  HIP_OK(hipGetLastError());
}

}  // namespace mhte
#endif  // MHTE_CLIP_HOST_H_
