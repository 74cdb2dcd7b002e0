// Aligned flat concat / split: the allreduce side of the deferred clip.  Reference: MonolithAlignedFlatConcat
// and MonolithAlignedFlatSplit, runtime/ops/aligned_concat_split.cu.cc:32-57, :63-128, with the layout rule of
// FusedAlignedOutputAllocator (runtime/ops/alloc_utils.h:50-95); native_training/feature_utils.py:48-99
// (allreduce_cond, fusion 'one') and :251-264 (cond_defer_clip).  Included by mhte.hip.
//
// Layout: tensor i starts at element off[i] = sum over j < i of round_up(len[j], A), A a power of two in
// [4, 1024]; [off[i], off[i] + len[i]) holds in[i][k] * scale — ONE fp32 product, rounded once, then (fp16
// wire) one IEEE conversion to nearest-even — and [off[i] + len[i], off[i + 1]) holds +0 (the reference's
// `out[id] = 0.0f`), whatever the scale is.  The reference's kernel walks the elements and looks every one up
// in the offsets; here the walk is over the chunk table of mhte_chunk_table.h:
//   * every non-empty tensor's OUTPUT span of round_up(len, A) elements is cut into chunks of 4096 elements,
//     numbered in tensor order; a chunk never straddles two tensors, and a tensor's last chunk carries its
//     padding (A divides 4096: a span has as many chunks as its tensor);
//   * workgroups of 256 threads take chunks by grid stride; in a chunk thread t owns the four groups of 4
//     elements at 4 * (256 * r + t), r = 0..3;
//   * the store side is always vector-aligned (out is 16-byte aligned, A >= 4): 16-byte stores for fp32,
//     packed 8-byte stores for fp16; the load side takes 16-byte loads where the source pointer is 16-byte
//     aligned and the group lies inside the tensor, 4-byte loads of the same elements otherwise (same bits);
//   * the next chunk's loads are issued before this chunk's stores.
// The scale is a kernel argument or a device word (result + 2 of mhte_global_l2_reduce), read with one uniform
// load at the top of the kernel: nothing comes back to the host.
#ifndef MHTE_FLAT_KERNELS_H_
#define MHTE_FLAT_KERNELS_H_

#include "mhte_clip_kernels.h"

namespace mhte {

constexpr int kFlatThreads = kClipThreads;
constexpr int kFlatInline = kClipInline;   // tensors in the kernel arguments; beyond: the table is uploaded per call
constexpr int kFlatGroups = 2048;          // workgroups at most (grid stride over the chunks)
constexpr int kFlatMinAlign = 4, kFlatMaxAlign = 1024;

// The non-empty tensors of a call: (pointer, length, first output element, first chunk), and A - 1.
struct FlatCounts : ChunkCounts {
  uint32_t align_mask;   // A - 1
};
struct FlatArgs : ChunkArgs<kFlatInline, 1, true, FlatCounts> {};
static_assert(sizeof(FlatArgs) + 4 * 8 < 4096, "the concat kernel's argument block stays under 4 KB");

// One chunk's place, uniform over the workgroup.
struct FlatChunk {
  const float* in;   // the chunk's first source element
  long long out;     // ... and its place in the flat buffer (a multiple of 4)
  long long rem;     // source elements from the chunk's start to the tensor's end (> 0)
  int n_out;         // output elements of the chunk, padding included: a multiple of A, <= 4096
};
template <bool EXT>
__device__ __forceinline__ FlatChunk flat_chunk_at(const FlatArgs& A, uint32_t c, uint32_t ti) {
  const long long skip = (long long)(c - tensor_chunk0<EXT>(A, ti)) * kChunkElems;
  const float* in = chunk_ptr<EXT, const float>(A, 0, ti);
  const long long len = chunk_len<EXT>(A, ti);
  const long long off = chunk_off<EXT>(A, ti);
  FlatChunk k;
  k.in = in + skip;
  k.out = off + skip;
  k.rem = len - skip;
  const long long span = ((len + A.k.align_mask) & ~(long long)(A.k.align_mask)) - skip;
  k.n_out = span < kChunkElems ? int(span) : kChunkElems;
  return k;
}

typedef _Float16 flat_f16x4 __attribute__((ext_vector_type(4)));

// a thread's 16 source floats of a chunk: v[r][j] = element 4 * (256 * r + t) + j, +0 past the tensor's end
__device__ __forceinline__ void flat_load(const FlatChunk& k, uint32_t t, ClipRegs& x) {
  const bool vec = (reinterpret_cast<uintptr_t>(k.in) & 15u) == 0;
  const MHTE_GLOBAL float* p = (const MHTE_GLOBAL float*)(k.in);
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int g = 4 * (kFlatThreads * r + int(t));
    if (vec && g + 4 <= k.rem) {
      const clip_f32x4 q = *(const MHTE_GLOBAL clip_f32x4*)(k.in + g);
      x.v[r][0] = q.x; x.v[r][1] = q.y; x.v[r][2] = q.z; x.v[r][3] = q.w;
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j) x.v[r][j] = g + j < k.rem ? p[g + j] : 0.f;
    }
  }
}

// The fp32 product on its way to fp16.  For (_Float16)(a * b) the compiler selects v_fma_mixlo_f16, which
// rounds the EXACT product to fp16 once: where the fp32 product lands on a tie between two fp16 neighbours
// that is the other neighbour about every second time (seen on the device, tests/test_flat_concat_gpu.py).
// The contract is the reference's — an fp32 product, then the compressor's cast — so the product passes
// through an empty asm (no instruction) and multiply and conversion stay two instructions.
__device__ __forceinline__ float flat_rounded_f32(float y) {
  asm volatile("" : "+v"(y));
  return y;
}

// the chunk's stores: the product inside the tensor, +0 in the padding, nothing past the span
template <typename WIRE>
__device__ __forceinline__ void flat_store(const FlatChunk& k, uint32_t t, const ClipRegs& x, float scale,
                                           WIRE* __restrict__ out) {
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int g = 4 * (kFlatThreads * r + int(t));
    if (g >= k.n_out) continue;
    float y[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) y[j] = g + j < k.rem ? __fmul_rn(x.v[r][j], scale) : 0.f;
    if constexpr (sizeof(WIRE) == 4) {
      clip_f32x4 q;
      q.x = y[0]; q.y = y[1]; q.z = y[2]; q.w = y[3];
      *(MHTE_GLOBAL clip_f32x4*)(out + k.out + g) = q;
    } else {
      flat_f16x4 h;   // (the conversion rounds to nearest-even, overflows to inf and keeps subnormals)
      h.x = (_Float16)flat_rounded_f32(y[0]); h.y = (_Float16)flat_rounded_f32(y[1]);
      h.z = (_Float16)flat_rounded_f32(y[2]); h.w = (_Float16)flat_rounded_f32(y[3]);
      *(MHTE_GLOBAL flat_f16x4*)(out + k.out + g) = h;
    }
  }
}

// WIRE: float or _Float16.  mode: kClipScaleArg or kClipScaleWord (src: the device word).
template <bool EXT, typename WIRE>
__global__ __launch_bounds__(kFlatThreads) void flat_concat_kernel(FlatArgs A, int32_t mode, float scale_arg,
                                                                   const float* __restrict__ src,
                                                                   WIRE* __restrict__ out) {
  const uint32_t t = threadIdx.x;
  float scale = scale_arg;
  if (mode == kClipScaleWord) scale = *(const MHTE_GLOBAL float*)(src);
  const uint32_t C = A.k.n_chunks;
  uint32_t c = blockIdx.x;
  if (c >= C) return;
  uint32_t ti = chunk_tensor_of<EXT>(A, c, 0);
  FlatChunk kc = flat_chunk_at<EXT>(A, c, ti);
  ClipRegs cur;
  flat_load(kc, t, cur);
  for (;;) {   // (C < 2^31, the host checks: c + gridDim.x does not wrap)
    const uint32_t cn = c + gridDim.x;
    FlatChunk kn = kc;
    ClipRegs nxt;
    if (cn < C) {
      ti = chunk_advance<EXT>(A, ti, cn);
      kn = flat_chunk_at<EXT>(A, cn, ti);
      flat_load(kn, t, nxt);
    }
    flat_store<WIRE>(kc, t, cur, scale, out);
    if (cn >= C) break;
    c = cn;
    kc = kn;
    cur = nxt;
  }
}

// out[k] = float(flat[k]) * post_scale over n elements; out == flat is allowed for fp32.  Groups of 4
// elements by grid stride where both pointers allow vector accesses, single elements otherwise and in the tail.
template <typename WIRE>
__global__ __launch_bounds__(kFlatThreads) void flat_decode_kernel(const WIRE* flat, long long n, float post_scale,
                                                                   float* out, int32_t vec) {
  const long long tid = (long long)blockIdx.x * kFlatThreads + threadIdx.x;
  const long long stride = (long long)gridDim.x * kFlatThreads;
  const MHTE_GLOBAL WIRE* pi = (const MHTE_GLOBAL WIRE*)(flat);
  MHTE_GLOBAL float* po = (MHTE_GLOBAL float*)(out);
  long long done = 0;
  if (vec) {
    typedef WIRE wire_x4 __attribute__((ext_vector_type(4)));
    const long long groups = n >> 2;
    for (long long g0 = tid; g0 < groups; g0 += 4 * stride) {
      wire_x4 q[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const long long g = g0 + u * stride;
        if (g < groups) q[u] = *(const MHTE_GLOBAL wire_x4*)(pi + 4 * g);
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const long long g = g0 + u * stride;
        if (g >= groups) continue;
        clip_f32x4 y;
        y.x = __fmul_rn(float(q[u].x), post_scale); y.y = __fmul_rn(float(q[u].y), post_scale);
        y.z = __fmul_rn(float(q[u].z), post_scale); y.w = __fmul_rn(float(q[u].w), post_scale);
        *(MHTE_GLOBAL clip_f32x4*)(po + 4 * g) = y;
      }
    }
    done = groups << 2;
  }
  for (long long e = done + tid; e < n; e += stride) po[e] = __fmul_rn(float(pi[e]), post_scale);
}

}  // namespace mhte
#endif  // MHTE_FLAT_KERNELS_H_
