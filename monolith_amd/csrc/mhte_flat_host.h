// Host side of the aligned flat concat / split (mhte_flat_kernels.h): the layout rule, the checks of the entry
// points, the tensor table and the launches.  Included by mhte.hip behind mhte_clip_host.h.
#ifndef MHTE_FLAT_HOST_H_
#define MHTE_FLAT_HOST_H_

#include "mhte_flat_kernels.h"

namespace mhte {

static void flat_check_align(const char* op, int32_t align_elems) {
  if (align_elems < kFlatMinAlign || align_elems > kFlatMaxAlign || (align_elems & (align_elems - 1)) != 0)
    clip_bad(op, "align_elems must be a power of two in [4, 1024], got " + std::to_string(align_elems));
}
// FusedAlignedOutputAllocator's rule (alloc_utils.h:55-58, :88-94): offsets[i] = the sum of round_up(lens[j], A)
// over j < i, offsets[n] the aligned total.  offsets == NULL: the total alone.  The caller has checked n, lens
// and align_elems.
static int64_t flat_offsets(const char* op, const int64_t* lens, int32_t n, int32_t align_elems, int64_t* offsets) {
  const int64_t mask = int64_t(align_elems) - 1;
  int64_t total = 0;
  for (int32_t i = 0; i < n; ++i) {
    if (offsets) offsets[i] = total;
    if (lens[i] > INT64_MAX - mask - total) clip_bad(op, "the aligned total does not fit into 64 bits");
    total += (lens[i] + mask) & ~mask;
  }
  if (offsets) offsets[n] = total;
  return total;
}

// The non-empty tensors of a call, in list order: up to kFlatInline of them are written straight into the
// kernel arguments (no allocation); a longer list is kept whole in the vectors and uploaded (flat_upload).
struct FlatTable {
  FlatArgs A{};
  std::vector<const float*> in;
  std::vector<long long> len, off;
  std::vector<uint32_t> chunk0;
  bool ext() const { return A.n_tensors > uint32_t(kFlatInline); }
};
static void flat_build(FlatTable& T, const char* op, const float* const* inputs, const int64_t* lens, int32_t n,
                       int32_t align_elems) {
  const int64_t mask = int64_t(align_elems) - 1;
  uint64_t chunks = 0;
  uint32_t m = 0;
  int64_t off = 0;
  for (int32_t i = 0; i < n; ++i) {
    if (lens[i] == 0) continue;   // (an empty tensor occupies nothing)
    if (m < uint32_t(kFlatInline)) {
      T.A.in[m] = inputs[i];
      T.A.len[m] = lens[i];
      T.A.off[m] = off;
      T.A.chunk0[m] = uint32_t(chunks);
    } else {
      if (m == uint32_t(kFlatInline)) {   // the list outgrows the arguments: the vectors take all of it
        T.in.assign(T.A.in, T.A.in + kFlatInline);
        T.len.assign(T.A.len, T.A.len + kFlatInline);
        T.off.assign(T.A.off, T.A.off + kFlatInline);
        T.chunk0.assign(T.A.chunk0, T.A.chunk0 + kFlatInline);
      }
      T.in.push_back(inputs[i]);
      T.len.push_back(lens[i]);
      T.off.push_back(off);
      T.chunk0.push_back(uint32_t(chunks));
    }
    ++m;
    off += (lens[i] + mask) & ~mask;
    // (A divides 4096: the span round_up(len, A) has as many chunks as the tensor)
    chunks += (uint64_t(lens[i]) + kFlatChunk - 1) / kFlatChunk;
    if (chunks >= (uint64_t(1) << 31)) clip_bad(op, "more than 2^31 chunks of 4096 elements in one call");
  }
  T.A.n_tensors = m;
  T.A.n_chunks = uint32_t(chunks);
  T.A.align_mask = uint32_t(mask);
}
// more than kFlatInline tensors: the table goes to the workspace's buffer (the caller holds ws.mu and has
// entered the stream), through pinned staging — no wait for the stream
static void flat_upload(AuxWs& ws, FlatTable& T, hipStream_t st) {
  const size_t m = T.in.size();
  const size_t total = m * (3 * 8 + 4);
  ws.flat_table.reserve(total);
  std::vector<char> h(total);
  memcpy(h.data(), T.in.data(), m * 8);
  memcpy(h.data() + m * 8, T.len.data(), m * 8);
  memcpy(h.data() + m * 16, T.off.data(), m * 8);
  memcpy(h.data() + m * 24, T.chunk0.data(), m * 4);
  PinnedStage::of(current_device()).upload(ws.flat_table.p, h.data(), total, st);
  char* d = ws.flat_table.p;
  T.A.x_in = reinterpret_cast<const float* const*>(d);
  T.A.x_len = reinterpret_cast<const long long*>(d + m * 8);
  T.A.x_off = reinterpret_cast<const long long*>(d + m * 16);
  T.A.x_chunk0 = reinterpret_cast<const uint32_t*>(d + m * 24);
}

template <bool EXT>
static void flat_concat_go(const FlatTable& T, int32_t mode, float scale, const float* scale_dev, int32_t wire,
                           void* out, hipStream_t st) {
  const uint32_t grid = std::max<uint32_t>(1, std::min<uint32_t>(T.A.n_chunks, kFlatGroups));
  if (wire == 0)
    flat_concat_kernel<EXT, float><<<grid, kFlatThreads, 0, st>>>(T.A, mode, scale, scale_dev, static_cast<float*>(out));
  else
    flat_concat_kernel<EXT, _Float16><<<grid, kFlatThreads, 0, st>>>(T.A, mode, scale, scale_dev,
                                                                    static_cast<_Float16*>(out));
}
// One launch (none without elements).
static void flat_concat_launch(FlatTable& T, float scale, const float* scale_dev, int32_t wire, void* out,
                               hipStream_t st) {
  if (T.A.n_chunks == 0) return;
  const int32_t mode = scale_dev ? kClipScaleWord : kClipScaleArg;
  if (T.ext()) {
    AuxWs& ws = AuxWs::of(current_device());
    std::lock_guard<std::mutex> g(ws.mu);
    AuxWs::Use use_(ws, st);
    flat_upload(ws, T, st);
    flat_concat_go<true>(T, mode, scale, scale_dev, wire, out, st);
  } else {
    flat_concat_go<false>(T, mode, scale, scale_dev, wire, out, st);
  }
  HIP_OK(hipGetLastError());
}

static void flat_decode_launch(const void* flat, int32_t wire, int64_t n, float post_scale, float* out,
                               hipStream_t st) {
  if (n == 0) return;
  // 4 elements per access: 16 bytes of fp32, 8 bytes of fp16
  const uintptr_t in_mask = wire == 0 ? 15u : 7u;
  const int32_t vec = ((reinterpret_cast<uintptr_t>(flat) & in_mask) | (reinterpret_cast<uintptr_t>(out) & 15u)) == 0;
  const uint64_t per_group = uint64_t(kFlatThreads) * 16;   // four groups of 4 elements per thread and pass
  const uint32_t grid = uint32_t(std::max<uint64_t>(1, std::min<uint64_t>((uint64_t(n) + per_group - 1) / per_group,
                                                                         uint64_t(kFlatGroups))));
  if (wire == 0)
    flat_decode_kernel<float><<<grid, kFlatThreads, 0, st>>>(static_cast<const float*>(flat), (long long)n, post_scale,
                                                            out, vec);
  else
    flat_decode_kernel<_Float16><<<grid, kFlatThreads, 0, st>>>(static_cast<const _Float16*>(flat), (long long)n,
                                                               post_scale, out, vec);
  HIP_OK(hipGetLastError());
}

}  // namespace mhte
#endif  // MHTE_FLAT_HOST_H_
