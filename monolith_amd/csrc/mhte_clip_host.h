// Host side of clip by global norm (mhte_clip_kernels.h): the checks of the entry points, the tensor table
// and the launches.  Included by mhte.hip behind AuxWs and PinnedStage.
#ifndef MHTE_CLIP_HOST_H_
#define MHTE_CLIP_HOST_H_

#include "mhte_clip_kernels.h"

namespace mhte {

[[noreturn]] static void clip_bad(const char* op, const std::string& m) {
  throw Error(MHTE_INVALID_ARGUMENT, std::string(op) + ": " + m);
}

// InvalidArgument before any device call.  outputs: NULL for an entry point that has none.  The caller has
// already refused its own null arguments (the lists, result, a device scalar).
static void clip_check(const char* op, const float* const* inputs, const char* in_name, float* const* outputs,
                       const int64_t* lens, int32_t n, bool has_clip_norm, float clip_norm) {
  if (n < 0) clip_bad(op, "n must be >= 0, got " + std::to_string(n));
  for (int32_t i = 0; i < n; ++i)
    if (lens[i] < 0) clip_bad(op, "tensor " + std::to_string(i) + " has the negative length " + std::to_string(lens[i]));
  for (int32_t i = 0; i < n; ++i) {
    if (lens[i] == 0) continue;
    if (!inputs[i]) clip_bad(op, std::string("null argument: ") + in_name + "[" + std::to_string(i) + "]");
    if (outputs && !outputs[i]) clip_bad(op, "null argument: outputs[" + std::to_string(i) + "]");
  }
  if (has_clip_norm && !(clip_norm >= 0.f))
    clip_bad(op, "clip_norm must be >= 0 and not NaN, got " + std::to_string(clip_norm));
}
static void clip_need_device() {
  static std::atomic<bool> seen{false};   // (a device, once seen, is not asked for again: these calls sit in the step)
  if (seen.load(std::memory_order_relaxed)) return;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) {
    (void)hipGetLastError();
    throw Error(MHTE_UNAVAILABLE, "no HIP device: the MI355X engine has no CPU fallback");
  }
  seen.store(true, std::memory_order_relaxed);
}

// The non-empty tensors of a call, in list order: up to kClipInline of them are written straight into the
// kernel arguments (no allocation); a longer list is kept whole in the vectors and uploaded (clip_upload).
struct ClipTable {
  ClipArgs A{};
  std::vector<const float*> in;
  std::vector<float*> out;
  std::vector<long long> len;
  std::vector<uint32_t> chunk0;
  bool all_inplace = true;
  bool ext() const { return A.n_tensors > uint32_t(kClipInline); }
};
// skip_inplace: tensors whose output is their input are left out (the host knows that nothing is clipped)
static void clip_build(ClipTable& T, const char* op, const float* const* inputs, float* const* outputs,
                       const int64_t* lens, int32_t n, bool skip_inplace) {
  uint64_t chunks = 0;
  uint32_t m = 0;
  for (int32_t i = 0; i < n; ++i) {
    if (lens[i] == 0) continue;
    float* o = outputs ? outputs[i] : nullptr;
    const bool inplace = o == inputs[i];
    if (skip_inplace && inplace) continue;
    if (outputs && !inplace) T.all_inplace = false;
    if (m < uint32_t(kClipInline)) {
      T.A.in[m] = inputs[i];
      T.A.out[m] = o;
      T.A.len[m] = lens[i];
      T.A.chunk0[m] = uint32_t(chunks);
    } else {
      if (m == uint32_t(kClipInline)) {   // the list outgrows the arguments: the vectors take all of it
        T.in.assign(T.A.in, T.A.in + kClipInline);
        T.out.assign(T.A.out, T.A.out + kClipInline);
        T.len.assign(T.A.len, T.A.len + kClipInline);
        T.chunk0.assign(T.A.chunk0, T.A.chunk0 + kClipInline);
      }
      T.in.push_back(inputs[i]);
      T.out.push_back(o);
      T.len.push_back(lens[i]);
      T.chunk0.push_back(uint32_t(chunks));
    }
    ++m;
    chunks += (uint64_t(lens[i]) + kClipChunk - 1) / kClipChunk;
    if (chunks >= (uint64_t(1) << 31)) clip_bad(op, "more than 2^31 chunks of 4096 floats in one call");
  }
  T.A.n_tensors = m;
  T.A.n_chunks = uint32_t(chunks);
}
// more than kClipInline tensors: the table goes to the workspace's buffer (the caller holds ws.mu and has
// entered the stream), through pinned staging — no wait for the stream
static void clip_upload(AuxWs& ws, ClipTable& T, hipStream_t st) {
  const size_t m = T.in.size();
  const size_t total = m * (3 * 8 + 4);
  ws.clip_table.reserve(total);
  std::vector<char> h(total);
  memcpy(h.data(), T.in.data(), m * 8);
  memcpy(h.data() + m * 8, T.out.data(), m * 8);
  memcpy(h.data() + m * 16, T.len.data(), m * 8);
  memcpy(h.data() + m * 24, T.chunk0.data(), m * 4);
  PinnedStage::of(current_device()).upload(ws.clip_table.p, h.data(), total, st);
  char* d = ws.clip_table.p;
  T.A.x_in = reinterpret_cast<const float* const*>(d);
  T.A.x_out = reinterpret_cast<float* const*>(d + m * 8);
  T.A.x_len = reinterpret_cast<const long long*>(d + m * 16);
  T.A.x_chunk0 = reinterpret_cast<const uint32_t*>(d + m * 24);
}

static uint32_t clip_scale_grid(const ClipTable& T) {
  return std::max<uint32_t>(1, std::min<uint32_t>(T.A.n_chunks, kClipScaleGroups));
}

// The norm: the partials launch, then the finish as a launch of its own (fused == false; result gets
// [sum, norm, scale, 0]) or as the prologue of the scale launch.  Two launches, nothing allocated after the
// first call, no wait.
static void clip_norm_launch(ClipTable& T, float clip_norm, float* result, bool fused, hipStream_t st) {
  AuxWs& ws = AuxWs::of(current_device());
  std::lock_guard<std::mutex> g(ws.mu);
  AuxWs::Use use_(ws, st);
  ws.clip_partials.reserve(kClipGroups);
  if (T.ext()) {
    clip_upload(ws, T, st);
    clip_partials_kernel<true><<<kClipGroups, kClipThreads, 0, st>>>(T.A, ws.clip_partials.p);
  } else {
    clip_partials_kernel<false><<<kClipGroups, kClipThreads, 0, st>>>(T.A, ws.clip_partials.p);
  }
  if (!fused) {
    clip_finish_kernel<<<1, kClipThreads, 0, st>>>(ws.clip_partials.p, clip_norm, result);
  } else if (T.ext()) {
    clip_scale_kernel<true><<<clip_scale_grid(T), kClipThreads, 0, st>>>(
        T.A, kClipScalePartials, 1.f, ws.clip_partials.p, clip_norm, result, T.all_inplace ? 1 : 0);
  } else {
    clip_scale_kernel<false><<<clip_scale_grid(T), kClipThreads, 0, st>>>(
        T.A, kClipScalePartials, 1.f, ws.clip_partials.p, clip_norm, result, T.all_inplace ? 1 : 0);
  }
  HIP_OK(hipGetLastError());
}

// The multiply alone: one launch (none without elements).
static void clip_scale_launch(ClipTable& T, int32_t mode, float scale, const float* src, float clip_norm,
                              hipStream_t st) {
  if (T.A.n_chunks == 0) return;
  if (T.ext()) {
    AuxWs& ws = AuxWs::of(current_device());
    std::lock_guard<std::mutex> g(ws.mu);
    AuxWs::Use use_(ws, st);
    clip_upload(ws, T, st);
    clip_scale_kernel<true><<<clip_scale_grid(T), kClipThreads, 0, st>>>(T.A, mode, scale, src, clip_norm, nullptr,
                                                                        T.all_inplace ? 1 : 0);
  } else {
    clip_scale_kernel<false><<<clip_scale_grid(T), kClipThreads, 0, st>>>(T.A, mode, scale, src, clip_norm, nullptr,
                                                                         T.all_inplace ? 1 : 0);
  }
  HIP_OK(hipGetLastError());
}

}  // namespace mhte
#endif  // MHTE_CLIP_HOST_H_
