// Host side of the aligned flat concat / split (mhte_flat_kernels.h): the layout rule, the checks of the entry
// points, the tensor table and the launches.  Included by mhte.hip behind mhte_aux_host.h.
#ifndef MHTE_FLAT_HOST_H_
#define MHTE_FLAT_HOST_H_

#include "mhte_flat_kernels.h"

namespace mhte {

static void flat_check_align(const char* op, int32_t align_elems) {
  if (align_elems < kFlatMinAlign || align_elems > kFlatMaxAlign || (align_elems & (align_elems - 1)) != 0)
    arg_bad(op, "align_elems must be a power of two in [4, 1024], got " + std::to_string(align_elems));
}
// FusedAlignedOutputAllocator's rule (alloc_utils.h:55-58, :88-94): offsets[i] = the sum of round_up(lens[j], A)
// over j < i, offsets[n] the aligned total.  offsets == NULL: the total alone.  The caller has checked n, lens
// and align_elems.
static int64_t flat_offsets(const char* op, const int64_t* lens, int32_t n, int32_t align_elems, int64_t* offsets) {
  const int64_t mask = int64_t(align_elems) - 1;
  int64_t total = 0;
  for (int32_t i = 0; i < n; ++i) {
    if (offsets) offsets[i] = total;
    if (lens[i] > INT64_MAX - mask - total) arg_bad(op, "the aligned total does not fit into 64 bits");
    total += (lens[i] + mask) & ~mask;
  }
  if (offsets) offsets[n] = total;
  return total;
}

// The non-empty tensors of a call, in list order (ChunkTable: inline up to kFlatInline, uploaded beyond), each
// at its offset by the rule above (an empty tensor occupies nothing).
typedef ChunkTable<FlatArgs> FlatTable;
static void flat_entries(FlatTable& T, const char* op, const float* const* inputs, const int64_t* lens, int32_t n,
                         int32_t align_elems) {
  const int64_t mask = int64_t(align_elems) - 1;
  int64_t off = 0;
  for (int32_t i = 0; i < n; ++i) {
    if (lens[i] == 0) continue;
    const void* const p[1] = {inputs[i]};
    // (A divides 4096: the span round_up(len, A) has as many chunks as the tensor)
    if (!T.add(p, lens[i], off)) arg_bad(op, "more than 2^31 chunks of 4096 elements in one call");
    off += (lens[i] + mask) & ~mask;
  }
  T.A.k.align_mask = uint32_t(mask);
}

template <bool EXT>
static void flat_concat_go(const FlatTable& T, int32_t mode, float scale, const float* scale_dev, int32_t wire,
                           void* out, hipStream_t st) {
  const uint32_t grid = std::max<uint32_t>(1, std::min<uint32_t>(T.A.k.n_chunks, kFlatGroups));
  if (wire == 0)
    flat_concat_kernel<EXT, float><<<grid, kFlatThreads, 0, st>>>(T.A, mode, scale, scale_dev, static_cast<float*>(out));
  else
    flat_concat_kernel<EXT, _Float16><<<grid, kFlatThreads, 0, st>>>(T.A, mode, scale, scale_dev,
                                                                    static_cast<_Float16*>(out));
}
// One launch (none without elements).
static void flat_concat_launch(FlatTable& T, float scale, const float* scale_dev, int32_t wire, void* out,
                               hipStream_t st) {
  if (T.A.k.n_chunks == 0) return;
  const int32_t mode = scale_dev ? kClipScaleWord : kClipScaleArg;
  chunk_launch(&AuxWs::flat_table, T, st, [&](auto ext) {
    flat_concat_go<decltype(ext)::value>(T, mode, scale, scale_dev, wire, out, st);
  });
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
