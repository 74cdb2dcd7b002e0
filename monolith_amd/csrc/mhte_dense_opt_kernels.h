// Dense optimizers on the device: Adamom and RMSprop (V1 / V2) applied to ALL variables in one launch, the
// gradient read where the allreduce left it (a flat fp32 or fp16 buffer) or from a list of fp32 tensors, the
// gradient scale and the learning rate read where the clip and the schedule left them (device words).  The
// arithmetic is mhte_dense_opt_core.h's; reference: ResourceApplyAdamom / ResourceApplyRmsprop,
// native_training/optimizers/cc/kernels/training_ops{.cc,_gpu.cu.cc}.  Included by mhte.hip.
//
// The walk is over the chunk table of mhte_chunk_table.h:
//   * every variable that takes part is cut into chunks of 4096 elements, numbered in list order; the table
//     gives (var pointer, gradient pointer or none, length, offset, chunk0) per variable;
//   * workgroups of 256 threads take chunks by grid stride; in a chunk thread t owns the four groups of 4
//     elements at 4 * (256 * r + t), r = 0..3;
//   * the slots m, v (and c) are flat fp32 buffers in the aligned layout: element k of variable i lives at
//     off[i] + k, always 16-byte aligned at a group's start; a group that lies inside the variable takes 16-byte
//     accesses, the variable's ragged last group 4-byte ones: the padding is never read or written;
//   * var and a list gradient take 16-byte accesses where their pointer is 16-byte aligned, 4-byte accesses of
//     the same elements otherwise (same bits); an fp16 flat gradient takes packed 8-byte loads.
// Registers: Adamom holds 5 input streams per element, 80 VGPRs for a thread's 16 elements; fetching the whole
// next chunk ahead, as the concat does with its one stream, would double that.  kDenseOptGroups (groups of 4
// per thread and pass: 4 = the whole chunk, 2 = half of it) and kDenseOptAhead (issue the next pass's loads
// before this pass's stores) are the two knobs; DESIGN.md §4.12b says which setting was kept and why.
#ifndef MHTE_DENSE_OPT_KERNELS_H_
#define MHTE_DENSE_OPT_KERNELS_H_

#include "../../include/monolith_amd_hash_table.h"
#include "mhte_dense_opt_core.h"
#include "mhte_flat_kernels.h"

namespace mhte {

constexpr int kDenseOptThreads = 256;
constexpr int kDenseOptMaxGroups = 2048;     // workgroups at most (grid stride over the chunks)
static_assert(kDenseOptInline == MHTE_DENSE_OPT_INLINE, "the public header states the kernel's constant");
static_assert(kChunkElems == 4 * 4 * kDenseOptThreads, "a thread owns four groups of 4 elements of a chunk");
#ifndef MHTE_DENSE_OPT_GROUPS
#define MHTE_DENSE_OPT_GROUPS 1
#endif
#ifndef MHTE_DENSE_OPT_AHEAD
#define MHTE_DENSE_OPT_AHEAD 1
#endif
constexpr int kDenseOptGroups = MHTE_DENSE_OPT_GROUPS;   // groups of 4 elements per thread and pass: 4, 2 or 1
constexpr int kDenseOptPasses = 4 / kDenseOptGroups;     // passes per chunk
constexpr bool kDenseOptAhead = MHTE_DENSE_OPT_AHEAD != 0;
static_assert(kDenseOptGroups == 4 || kDenseOptGroups == 2 || kDenseOptGroups == 1, "groups per pass");

enum DenseOptKind : int { kDenseAdamom = 0, kDenseRmsprop = 1 };
enum DenseOptSource : int { kDenseGradList = 0, kDenseGradFlat32 = 1, kDenseGradFlat16 = 2 };
enum DenseOptFlags : int32_t { kDenseUpdateSlots = 1, kDenseV2 = 2 };

// The variables of a call that take part: (var, list gradient — not read with a flat source —, length, offset,
// first chunk).
struct DenseOptArgs : ChunkArgs<kDenseOptInline, 2, true> {};
// the flat buffers of a call
struct DenseOptBufs {
  float* m;
  float* v;
  float* c;                 // Adamom only
  const void* grads_flat;   // a flat source only: fp32 or fp16
};
static_assert(sizeof(DenseOptArgs) + sizeof(DenseOptBufs) + sizeof(DenseOptHyper) + 2 * sizeof(void*) + 8 < 4096,
              "the kernel's argument block stays under 4 KB");

// One chunk's place, uniform over the workgroup.
struct DenseChunk {
  float* var;          // the chunk's first element of the variable
  const float* grad;   // ... of its list gradient
  long long off;       // ... and its place in the slot buffers and the flat gradient (a multiple of 4)
  long long rem;       // elements from the chunk's start to the variable's end (> 0)
  bool var_vec, grad_vec;
};
template <bool EXT, int SRC>
__device__ __forceinline__ DenseChunk dense_chunk_at(const DenseOptArgs& A, uint32_t c, uint32_t ti) {
  const long long skip = (long long)(c - tensor_chunk0<EXT>(A, ti)) * kChunkElems;
  float* var = chunk_ptr<EXT, float>(A, 0, ti);
  const long long len = chunk_len<EXT>(A, ti);
  const long long off = chunk_off<EXT>(A, ti);
  DenseChunk k;
  k.var = var + skip;
  k.var_vec = (reinterpret_cast<uintptr_t>(k.var) & 15u) == 0;
  k.grad = nullptr;
  k.grad_vec = true;
  if constexpr (SRC == kDenseGradList) {
    const float* grad = chunk_ptr<EXT, const float>(A, 1, ti);
    k.grad = grad + skip;
    k.grad_vec = (reinterpret_cast<uintptr_t>(k.grad) & 15u) == 0;
  }
  k.off = off + skip;
  k.rem = len - skip;
  return k;
}

// four elements at p: one 16-byte access when vec (the caller knows the address is aligned and all four lie
// inside the variable), else the first nv of them one by one
__device__ __forceinline__ void dense_load4(const float* p, bool vec, int nv, float (&x)[4]) {
  if (vec) {
    const clip_f32x4 q = *(const MHTE_GLOBAL clip_f32x4*)(p);
    x[0] = q.x; x[1] = q.y; x[2] = q.z; x[3] = q.w;
  } else {
    const MHTE_GLOBAL float* s = (const MHTE_GLOBAL float*)(p);
#pragma unroll
    for (int j = 0; j < 4; ++j) x[j] = j < nv ? s[j] : 0.f;
  }
}
__device__ __forceinline__ void dense_load4_f16(const _Float16* p, bool vec, int nv, float (&x)[4]) {
  if (vec) {
    const flat_f16x4 q = *(const MHTE_GLOBAL flat_f16x4*)(p);
    x[0] = float(q.x); x[1] = float(q.y); x[2] = float(q.z); x[3] = float(q.w);
  } else {
    const MHTE_GLOBAL _Float16* s = (const MHTE_GLOBAL _Float16*)(p);
#pragma unroll
    for (int j = 0; j < 4; ++j) x[j] = j < nv ? float(s[j]) : 0.f;
  }
}
__device__ __forceinline__ void dense_store4(float* p, bool vec, int nv, const float (&x)[4]) {
  if (vec) {
    clip_f32x4 q;
    q.x = x[0]; q.y = x[1]; q.z = x[2]; q.w = x[3];
    *(MHTE_GLOBAL clip_f32x4*)(p) = q;
  } else {
    MHTE_GLOBAL float* d = (MHTE_GLOBAL float*)(p);
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (j < nv) d[j] = x[j];
  }
}

// a thread's elements of one pass: [stream][group][element]; streams: var, gradient, m, v (, c)
template <int KIND>
struct DenseRegs {
  static constexpr int kStreams = KIND == kDenseAdamom ? 5 : 4;
  float x[kStreams][kDenseOptGroups][4];
};

// the first element of thread t's group r of pass p, relative to the chunk's start
__device__ __forceinline__ int dense_group_at(int p, int r, uint32_t t) {
  return 4 * (kDenseOptThreads * (p * kDenseOptGroups + r) + int(t));
}

template <int KIND, int SRC>
__device__ __forceinline__ void dense_load(const DenseChunk& k, const DenseOptBufs& B, int p, uint32_t t,
                                           DenseRegs<KIND>& x) {
#pragma unroll
  for (int r = 0; r < kDenseOptGroups; ++r) {
    const int g = dense_group_at(p, r, t);
    if (g >= k.rem) continue;   // (nothing of this group belongs to the variable)
    const bool full = g + 4 <= k.rem;
    const int nv = full ? 4 : int(k.rem - g);
    dense_load4(k.var + g, full && k.var_vec, nv, x.x[0][r]);
    if constexpr (SRC == kDenseGradList)
      dense_load4(k.grad + g, full && k.grad_vec, nv, x.x[1][r]);
    else if constexpr (SRC == kDenseGradFlat32)
      dense_load4(static_cast<const float*>(B.grads_flat) + k.off + g, full, nv, x.x[1][r]);
    else
      dense_load4_f16(static_cast<const _Float16*>(B.grads_flat) + k.off + g, full, nv, x.x[1][r]);
    dense_load4(B.m + k.off + g, full, nv, x.x[2][r]);
    dense_load4(B.v + k.off + g, full, nv, x.x[3][r]);
    if constexpr (KIND == kDenseAdamom) dense_load4(B.c + k.off + g, full, nv, x.x[4][r]);
  }
}

// UPDATE_SLOTS and V2 are compile-time here: one straight-line body per form, none computes the other's
// division and square root beside its own
template <int KIND, bool UPDATE_SLOTS, bool V2>
__device__ __forceinline__ void dense_apply_store_as(const DenseChunk& k, const DenseOptBufs& B, int p, uint32_t t,
                                                     DenseRegs<KIND>& x, const DenseOptHyper& h) {
#pragma unroll
  for (int r = 0; r < kDenseOptGroups; ++r) {
    const int g = dense_group_at(p, r, t);
    if (g >= k.rem) continue;
    const bool full = g + 4 <= k.rem;
    const int nv = full ? 4 : int(k.rem - g);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if constexpr (KIND == kDenseAdamom)
        dense_adamom_step(x.x[0][r][j], x.x[2][r][j], x.x[3][r][j], x.x[4][r][j], x.x[1][r][j], h, UPDATE_SLOTS, V2);
      else
        dense_rmsprop_step(x.x[0][r][j], x.x[2][r][j], x.x[3][r][j], x.x[1][r][j], h, V2);
    }
    dense_store4(k.var + g, full && k.var_vec, nv, x.x[0][r]);
    if constexpr (KIND == kDenseRmsprop || UPDATE_SLOTS) {   // (Adamom without update_slots: the slots keep their bits)
      dense_store4(B.m + k.off + g, full, nv, x.x[2][r]);
      dense_store4(B.v + k.off + g, full, nv, x.x[3][r]);
      if constexpr (KIND == kDenseAdamom) dense_store4(B.c + k.off + g, full, nv, x.x[4][r]);
    }
  }
}
// (flags is uniform over the launch; RMSprop is never launched without update_slots)
template <int KIND>
__device__ __forceinline__ void dense_apply_store(const DenseChunk& k, const DenseOptBufs& B, int p, uint32_t t,
                                                  DenseRegs<KIND>& x, const DenseOptHyper& h, int32_t flags) {
  const bool v2 = (flags & kDenseV2) != 0;
  if (KIND == kDenseRmsprop || (flags & kDenseUpdateSlots) != 0) {
    if (v2) dense_apply_store_as<KIND, true, true>(k, B, p, t, x, h);
    else dense_apply_store_as<KIND, true, false>(k, B, p, t, x, h);
  } else {
    if (v2) dense_apply_store_as<KIND, false, true>(k, B, p, t, x, h);
    else dense_apply_store_as<KIND, false, false>(k, B, p, t, x, h);
  }
}

// grad_scale_dev / lr_dev != NULL: the device word replaces the argument, one uniform load each.
template <bool EXT, int KIND, int SRC>
__global__ __launch_bounds__(kDenseOptThreads) void dense_opt_kernel(DenseOptArgs A, DenseOptBufs B, DenseOptHyper h,
                                                                     const float* __restrict__ grad_scale_dev,
                                                                     const float* __restrict__ lr_dev,
                                                                     int32_t flags) {
  const uint32_t t = threadIdx.x;
  if (grad_scale_dev) h.grad_scale = *(const MHTE_GLOBAL float*)(grad_scale_dev);
  if (lr_dev) h.lr = *(const MHTE_GLOBAL float*)(lr_dev);
  const uint32_t C = A.k.n_chunks;
  uint32_t c = blockIdx.x;
  if (c >= C) return;
  uint32_t ti = chunk_tensor_of<EXT>(A, c, 0);
  DenseChunk kc = dense_chunk_at<EXT, SRC>(A, c, ti);
  int p = 0;
  DenseRegs<KIND> cur;
  dense_load<KIND, SRC>(kc, B, p, t, cur);
  for (;;) {   // (C < 2^31, the host checks: c + gridDim.x does not wrap)
    DenseChunk kn = kc;
    int pn = p + 1;
    bool more = true;
    if (pn == kDenseOptPasses) {   // the workgroup's next chunk; the variable index only moves forward
      pn = 0;
      const uint32_t cn = c + gridDim.x;
      more = cn < C;
      if (more) {
        ti = chunk_advance<EXT>(A, ti, cn);
        kn = dense_chunk_at<EXT, SRC>(A, cn, ti);
        c = cn;
      }
    }
    DenseRegs<KIND> nxt;
    if (kDenseOptAhead && more) dense_load<KIND, SRC>(kn, B, pn, t, nxt);
    dense_apply_store<KIND>(kc, B, p, t, cur, h, flags);
    if (!more) break;
    if (!kDenseOptAhead) dense_load<KIND, SRC>(kn, B, pn, t, nxt);
    kc = kn;
    p = pn;
    cur = nxt;
  }
}

}  // namespace mhte
#endif  // MHTE_DENSE_OPT_KERNELS_H_
