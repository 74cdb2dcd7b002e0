// Clip by global norm on the device: the L2 norm over a list of fp32 tensors, the clip scale
// min(clip_norm / norm, 1) kept in HBM, and the multiply.  Reference: GlobalL2Reduce and
// MonolithClipByGlobalNorm(+Fused), runtime/ops/clip_by_global_norm.h:31-60, clip_by_global_norm.cu.cc,
// clip_by_global_norm_fused.cu.cc:37-165; native_training/clip_ops.py.  Included by mhte.hip.
//
// The reference's GPU form adds its blocks' sums with a float atomicAdd (a different sum every run) and
// waits for the stream before the multiply (clip_by_global_norm_fused.cu.cc:150).  Here the sum of squares
// is ONE FIXED TREE, a function of the tensors' contents and lengths alone — not of the grid, the device or
// the run — and nothing comes back to the host:
//   * every non-empty tensor is cut into chunks of 4096 consecutive floats (the last one short, read as if
//     padded with +0), numbered in tensor order c = 0 .. C-1: the chunk table of mhte_chunk_table.h;
//   * clip_partials_kernel, always 1024 workgroups of 256 threads: workgroup w takes chunks w, w + 1024, ...
//     in that order; in a chunk thread t owns elements 4 * (256 * r + t) + k, r = 0..3, k = 0..3, and adds
//     them into ONE accumulator that starts at +0 in (chunk, r, k) order, acc = acc + v * v with product and
//     sum rounded to fp32 separately (no FMA); the 256 accumulators are halved, a[t] = a[t] + a[t + s] for
//     t < s, s = 128 .. 1; partial[w] is stored by every workgroup (+0 without chunks);
//   * clip_finish: the 1024 partials halved the same way, s = 512 .. 1, norm = sqrt(sum), scale =
//     norm > clip_norm ? clip_norm / norm : 1 (clip_by_global_norm.h:42-43) with IEEE square root and divide.
// No workgroup hands anything to another inside a launch: the partials cross a launch boundary, and the
// scale kernel sums the 4 KB of partials in EVERY workgroup's prologue (the tree is fixed, so all of them
// get the same scale).  16-byte loads where a chunk is full and its address aligned, 4-byte loads otherwise:
// the same elements in the same order, the same bits.
#ifndef MHTE_CLIP_KERNELS_H_
#define MHTE_CLIP_KERNELS_H_

#include "mhte_chunk_table.h"
#include "mhte_kernels.h"

namespace mhte {

constexpr int kClipGroups = 1024;      // workgroups of the partials launch = number of partials
constexpr int kClipThreads = 256;
constexpr int kClipInline = 128;       // tensors in the kernel arguments; beyond: the table is uploaded per call
constexpr int kClipScaleGroups = 2048; // workgroups of the scale launch at most (grid stride over the chunks)

// where the scale kernel takes its factor from (workgroup-uniform)
enum ClipScaleMode : int32_t {
  kClipScaleArg = 0,       // the kernel argument
  kClipScaleWord = 1,      // a device word: the scale itself
  kClipScaleNorm = 2,      // a device word: the global norm, with clip_norm
  kClipScalePartials = 3,  // the partials of clip_partials_kernel, with clip_norm (the fused form)
};

// The non-empty tensors of a call: (in, out, length, first chunk); the partials launch does not read out.
struct ClipArgs : ChunkArgs<kClipInline, 2, false> {};
static_assert(sizeof(ClipArgs) + 6 * 8 < 4096, "the scale kernel's argument block stays under 4 KB");

// One chunk's place, uniform over the workgroup.
struct ClipChunk {
  const float* in;
  float* out;
  long long rem;   // floats from the chunk's start to the tensor's end (> 0)
};
template <bool EXT>
__device__ __forceinline__ ClipChunk clip_chunk_at(const ClipArgs& A, uint32_t c, uint32_t ti) {
  const long long skip = (long long)(c - tensor_chunk0<EXT>(A, ti)) * kChunkElems;
  ClipChunk k;
  const float* in = chunk_ptr<EXT, const float>(A, 0, ti);
  float* out = chunk_ptr<EXT, float>(A, 1, ti);
  const long long len = chunk_len<EXT>(A, ti);
  k.in = in + skip;
  k.out = out ? out + skip : nullptr;
  k.rem = len - skip;
  return k;
}

typedef float clip_f32x4 __attribute__((ext_vector_type(4)));

// a thread's 16 floats of a chunk: v[r][k] = element 4 * (256 * r + t) + k, +0 past the tensor's end
struct ClipRegs {
  float v[4][4];
};
__device__ __forceinline__ void clip_load(const ClipChunk& k, uint32_t t, ClipRegs& x) {
  if (k.rem >= kChunkElems && (reinterpret_cast<uintptr_t>(k.in) & 15u) == 0) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const clip_f32x4 q = *(const MHTE_GLOBAL clip_f32x4*)(k.in + 4 * (kClipThreads * r + int(t)));
      x.v[r][0] = q.x; x.v[r][1] = q.y; x.v[r][2] = q.z; x.v[r][3] = q.w;
    }
    return;
  }
  const MHTE_GLOBAL float* p = (const MHTE_GLOBAL float*)(k.in);
#pragma unroll
  for (int r = 0; r < 4; ++r) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const long long e = 4 * (kClipThreads * r + (long long)(t)) + j;
      x.v[r][j] = e < k.rem ? p[e] : 0.f;
    }
  }
}

// a[t] = a[t] + a[t + s] for t < s, s = 128 .. 1, over the workgroup's 256 values: strides 128 and 64
// through LDS, 32 and below inside wavefront 0 (lane t takes lane t + s: the same pairing).  Thread 0
// returns the sum.
__device__ __forceinline__ float clip_reduce_256(float a, float* lds, uint32_t t) {
  lds[t] = a;
  __syncthreads();
  if (t < 128) lds[t] = __fadd_rn(lds[t], lds[t + 128]);
  __syncthreads();
  float v = 0.f;
  if (t < 64) {
    v = __fadd_rn(lds[t], lds[t + 64]);
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) v = __fadd_rn(v, __shfl_down(v, s, 64));
  }
  return v;
}

template <bool EXT>
__global__ __launch_bounds__(kClipThreads) void clip_partials_kernel(ClipArgs A, float* __restrict__ partials) {
  __shared__ float lds[kClipThreads];
  const uint32_t t = threadIdx.x, w = blockIdx.x;
  const uint32_t C = A.k.n_chunks;
  float acc = 0.f;
  if (w < C) {
    // the next chunk's loads travel while this chunk is added; the tensor index only moves forward
    uint32_t ti = chunk_tensor_of<EXT>(A, w, 0);
    ClipRegs cur;
    clip_load(clip_chunk_at<EXT>(A, w, ti), t, cur);
    for (uint32_t c = w;; c += kClipGroups) {   // (C < 2^31, the host checks: c + 1024 does not wrap)
      const uint32_t cn = c + kClipGroups;
      ClipRegs nxt;
      if (cn < C) {
        ti = chunk_advance<EXT>(A, ti, cn);
        clip_load(clip_chunk_at<EXT>(A, cn, ti), t, nxt);
      }
#pragma unroll
      for (int r = 0; r < 4; ++r) {
#pragma unroll
        for (int j = 0; j < 4; ++j) acc = __fadd_rn(acc, __fmul_rn(cur.v[r][j], cur.v[r][j]));
      }
      if (cn >= C) break;
      cur = nxt;
    }
  }
  const float s = clip_reduce_256(acc, lds, t);
  if (t == 0) ((MHTE_GLOBAL float*)partials)[w] = s;
}

// The 1024 partials -> (sum, norm, scale); every thread of the workgroup returns the scale.  store: this
// workgroup writes the result block [sum, norm, scale, 0].
__device__ __forceinline__ float clip_finish(const float* partials, float clip_norm, float* result, bool store,
                                             float* lds, uint32_t t) {
  const MHTE_GLOBAL float* p = (const MHTE_GLOBAL float*)(partials);
  // s = 512: entries t and t + 256 of the halved array; s = 256: their sum
  const float x0 = __fadd_rn(p[t], p[t + 512]);
  const float x1 = __fadd_rn(p[t + 256], p[t + 768]);
  const float sum = clip_reduce_256(__fadd_rn(x0, x1), lds, t);
  __shared__ float s_scale;
  if (t == 0) {
    // (sqrtf and / are the correctly rounded forms here; __fsqrt_rn is the native approximation on this stack)
    const float norm = sqrtf(sum);
    const float scale = norm > clip_norm ? clip_norm / norm : 1.0f;
    s_scale = scale;
    if (store) {
      MHTE_GLOBAL float* r = (MHTE_GLOBAL float*)(result);
      r[0] = sum;
      r[1] = norm;
      r[2] = scale;
      r[3] = 0.f;
    }
  }
  __syncthreads();
  return s_scale;
}

// the norm-only entry: one workgroup
__global__ __launch_bounds__(kClipThreads) void clip_finish_kernel(const float* __restrict__ partials,
                                                                   float clip_norm, float* __restrict__ result) {
  __shared__ float lds[kClipThreads];
  (void)clip_finish(partials, clip_norm, result, true, lds, threadIdx.x);
}

// out[i][j] = in[i][j] * scale over the chunk table, by grid stride.  A tensor that is in place is left
// alone when the scale is exactly 1 (the reference's "no clip: the outputs are the inputs"), and a call
// whose tensors are all in place then ends after its prologue; a tensor that is not is copied.
template <bool EXT>
__global__ __launch_bounds__(kClipThreads) void clip_scale_kernel(ClipArgs A, int32_t mode, float scale_arg,
                                                                  const float* __restrict__ src, float clip_norm,
                                                                  float* __restrict__ result, int32_t all_inplace) {
  __shared__ float lds[kClipThreads];
  const uint32_t t = threadIdx.x;
  float scale = scale_arg;
  if (mode == kClipScaleWord) {
    scale = *(const MHTE_GLOBAL float*)(src);
  } else if (mode == kClipScaleNorm) {
    const float norm = *(const MHTE_GLOBAL float*)(src);
    scale = norm > clip_norm ? clip_norm / norm : 1.0f;
  } else if (mode == kClipScalePartials) {
    scale = clip_finish(src, clip_norm, result, blockIdx.x == 0, lds, t);
  }
  const bool one = scale == 1.0f;
  if (one && all_inplace) return;
  const uint32_t C = A.k.n_chunks;
  uint32_t ti = 0;
  for (uint32_t c = blockIdx.x; c < C; c += gridDim.x) {   // (C < 2^31: no wrap)
    ti = chunk_advance<EXT>(A, ti, c);
    const ClipChunk k = clip_chunk_at<EXT>(A, c, ti);
    if (one && k.in == k.out) continue;
    if (k.rem >= kChunkElems && ((reinterpret_cast<uintptr_t>(k.in) | reinterpret_cast<uintptr_t>(k.out)) & 15u) == 0) {
      clip_f32x4 q[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) q[r] = *(const MHTE_GLOBAL clip_f32x4*)(k.in + 4 * (kClipThreads * r + int(t)));
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        if (!one) {
          q[r].x = __fmul_rn(q[r].x, scale); q[r].y = __fmul_rn(q[r].y, scale);
          q[r].z = __fmul_rn(q[r].z, scale); q[r].w = __fmul_rn(q[r].w, scale);
        }
        *(MHTE_GLOBAL clip_f32x4*)(k.out + 4 * (kClipThreads * r + int(t))) = q[r];
      }
      continue;
    }
    const MHTE_GLOBAL float* pi = (const MHTE_GLOBAL float*)(k.in);
    MHTE_GLOBAL float* po = (MHTE_GLOBAL float*)(k.out);
    const long long n = k.rem < kChunkElems ? k.rem : (long long)kChunkElems;
    for (long long e = t; e < n; e += kClipThreads) {
      const float x = pi[e];
      po[e] = one ? x : __fmul_rn(x, scale);
    }
  }
}

}  // namespace mhte
#endif  // MHTE_CLIP_KERNELS_H_
