// The FFM feature cross (multiply and dot) and its gradient: the arithmetic contract, the shapes and the
// host's choice of kernel form — one source for host and device.
// Reference: FFMOp / FFMGradOp, native_training/layers/ops/ffm_ops.cc and layers/kernels/ffm_kernels.h:46-157
// (the shapes), ffm_kernels.cc:28-103 and ffm_kernels.cu.cc:34-168 (the loops); the Python side is
// layers/layer_ops.py:24-46 and its only caller the GroupInt / FFM layer, layers/feature_cross.py:69-146.
//
// With L = left_cols / D, R = right_cols / D (integer division) and D = dim_size, everything fp32 and every
// operation ONE operation rounded on its own (no FMA):
//   multiply   out[b, (l R + r) D + k] = left[b, l D + k] * right[b, r D + k]
//   dot        out[b, l R + r]         = (((+0 + p_0) + p_1) + ... + p_{D-1}),  p_k = left[b, l D + k] * right[b, r D + k]
//              (the sum STARTS from +0: 0 + (-0) is +0, an accumulator that starts with p_0 gives other bits)
//   gradient   left_grad[b, l D + k]  = ((+0 + g(l,0,k) right[b, 0 D + k]) + ... + g(l,R-1,k) right[b, (R-1) D + k])
//              right_grad[b, r D + k] = ((+0 + g(0,r,k) left[b, 0 D + k])  + ... + g(L-1,r,k) left[b, (L-1) D + k])
//              g(l,r,k) = grad[b, (l R + r) D + k] for multiply, grad[b, l R + r] for dot
// — the order in which both the CPU and the CUDA loops of the reference reach every element.  Columns of left /
// right beyond L D / R D are not read; the gradients have the inputs' full widths and hold +0 there.
// tests/ffm_truth.py restates all of it.
//
// Compiled by hipcc inside mhte.hip and, for the CPU suite (tests/ffm_host_driver.cc), by g++ with
// MHTE_HOST_ONLY defined.
#ifndef MHTE_FFM_CORE_H_
#define MHTE_FFM_CORE_H_

#include <stdint.h>

#if defined(MHTE_HOST_ONLY)
#ifndef MHTE_HD
#define MHTE_HD
#endif
#else
#include <hip/hip_runtime.h>
#ifndef MHTE_HD
#define MHTE_HD __host__ __device__ __forceinline__
#endif
#endif

namespace mhte {

constexpr int kFfmThreads = 256;
// LDS a workgroup declares, in floats.  Forward: 32 KiB for the (L + R) D input floats of a tile of batch rows
// (five workgroups fit a CU's 160 KiB).  Gradient: 64 KiB for the tile's slabs of grad and its rows of left and
// right: two workgroups per CU, each of them wide enough for a 13 x 13 x 16 slab times five rows.
constexpr int kFfmFwdLdsFloats = 8192;
constexpr int kFfmGradLdsFloats = 16384;
constexpr int kFfmTileRowsMax = 64;      // batch rows per tile at most
constexpr int kFfmFwdMaxGroups = 1024;   // workgroups at most: the grid strides over the tiles beyond
constexpr int kFfmGradMaxGroups = 512;   // (2 per CU, what the gradient's LDS admits)

// four floats that move as one 16-byte access (g++ and hipcc both know vector_size)
typedef float FfmF4 __attribute__((vector_size(16)));

// one rounded product / sum (the build passes -ffp-contract=off; on the device the intrinsics say it again)
MHTE_HD float ffm_mul(float a, float b) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __fmul_rn(a, b);
#else
  return a * b;
#endif
}
MHTE_HD float ffm_add(float a, float b) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __fadd_rn(a, b);
#else
  return a + b;
#endif
}
MHTE_HD FfmF4 ffm_mul(FfmF4 a, FfmF4 b) {
  FfmF4 r;
  r[0] = ffm_mul(a[0], b[0]); r[1] = ffm_mul(a[1], b[1]); r[2] = ffm_mul(a[2], b[2]); r[3] = ffm_mul(a[3], b[3]);
  return r;
}
MHTE_HD FfmF4 ffm_mul(float a, FfmF4 b) {   // (dot's gradient: one g for the D elements of a feature pair)
  FfmF4 r;
  r[0] = ffm_mul(a, b[0]); r[1] = ffm_mul(a, b[1]); r[2] = ffm_mul(a, b[2]); r[3] = ffm_mul(a, b[3]);
  return r;
}
MHTE_HD FfmF4 ffm_add(FfmF4 a, FfmF4 b) {
  FfmF4 r;
  r[0] = ffm_add(a[0], b[0]); r[1] = ffm_add(a[1], b[1]); r[2] = ffm_add(a[2], b[2]); r[3] = ffm_add(a[3], b[3]);
  return r;
}
// the next one (four) of a dot output's terms, in ascending k
MHTE_HD float ffm_dot_step(float acc, float a, float b) { return ffm_add(acc, ffm_mul(a, b)); }
MHTE_HD float ffm_dot_step(float acc, FfmF4 a, FfmF4 b) {
  const FfmF4 p = ffm_mul(a, b);
  return ffm_add(ffm_add(ffm_add(ffm_add(acc, p[0]), p[1]), p[2]), p[3]);
}

// ---- the element functions ------------------------------------------------------------------------------
// PA, PB, PG, PO: pointers to float or FfmF4 in any address space (the kernels pass LDS and global ones).

// One dot output: a and b are the feature's D floats of left and right, n = D (float) or D / 4 (FfmF4) steps.
template <class PA, class PB>
MHTE_HD float ffm_dot_elem(PA a, PB b, int n) {
  float acc = 0.f;
  int i = 0;
  for (; i + 4 <= n; i += 4)   // (four steps per trip: their operands can be fetched together; the sums keep their order)
    acc = ffm_dot_step(ffm_dot_step(ffm_dot_step(ffm_dot_step(acc, a[i], b[i]), a[i + 1], b[i + 1]), a[i + 2], b[i + 2]),
                       a[i + 3], b[i + 3]);
  for (; i < n; ++i) acc = ffm_dot_step(acc, a[i], b[i]);
  return acc;
}

// One gradient element (T float) or four neighbours in k (T FfmF4): +0, then the n terms g[i gs] * o[i os] in
// ascending i.  g: the strided run of upstream gradients, o: the other operand's row.
//   left_grad[l D + k]:   multiply  g = grad + (l R) D + k, gs = D;   dot  g = grad + l R, gs = 1;  o = right + k, os = D, n = R
//   right_grad[r D + k]:  multiply  g = grad + r D + k, gs = R D;     dot  g = grad + r, gs = R;    o = left + k,  os = D, n = L
// (strides in elements of what the pointers point to).
template <class T, class PG, class PO>
MHTE_HD T ffm_grad_elem(PG g, long long gs, PO o, long long os, int n) {
  T acc = T{};
  int i = 0;
  for (; i + 4 <= n; i += 4) {   // (as in ffm_dot_elem)
    acc = ffm_add(acc, ffm_mul(g[i * gs], o[i * os]));
    acc = ffm_add(acc, ffm_mul(g[(i + 1) * gs], o[(i + 1) * os]));
    acc = ffm_add(acc, ffm_mul(g[(i + 2) * gs], o[(i + 2) * os]));
    acc = ffm_add(acc, ffm_mul(g[(i + 3) * gs], o[(i + 3) * os]));
  }
  for (; i < n; ++i) acc = ffm_add(acc, ffm_mul(g[i * gs], o[i * os]));
  return acc;
}

// ---- the host's choice of form ----------------------------------------------------------------------------
enum FfmKernel : int { kFfmForward = 0, kFfmGradient = 1 };
// The kernel form of a call.  vec: 4 (16-byte accesses) or 1.  lds: the tile's operands are staged in LDS
// (tile_rows batch rows per tile); otherwise the direct form, every operand read where it lies.
struct FfmForm {
  int vec, lds, tile_rows;
};
// the launch counter of a form: mhte_ffm_launch_counts' index
constexpr int kFfmCounters = 16;
inline int ffm_counter_index(int kernel, int dot, const FfmForm& f) {
  return kernel * 8 + (dot ? 4 : 0) + (f.vec == 4 ? 0 : 2) + (f.lds ? 0 : 1);
}

// aligned: every pointer the form moves 16 bytes through is 16-byte aligned and every row width it strides by
// is a multiple of 4 floats (the caller ORs them together; which ones count: mhte_ffm_host.h).
// L, R >= 1, D >= 1, L R D < 2^31 (the caller has checked).
inline FfmForm ffm_forward_form(long long L, long long R, long long D, bool aligned) {
  FfmForm f;
  f.vec = (D % 4 == 0 && aligned) ? 4 : 1;
  const long long row = (L + R) * D;   // floats of one batch row in LDS
  long long rows = kFfmFwdLdsFloats / row;
  if (rows > kFfmTileRowsMax) rows = kFfmTileRowsMax;
  f.lds = rows >= 1;
  f.tile_rows = int(rows);
  return f;
}
// floats of grad one batch row stages: the slab
inline long long ffm_grad_slab(long long L, long long R, long long D, bool dot) { return dot ? L * R : L * R * D; }
// LDS layout of a tile: [tile_rows][slab] of grad, rounded up to 4 floats, then [tile_rows][L D] of left, then
// [tile_rows][R D] of right.
inline FfmForm ffm_grad_form(long long L, long long R, long long D, bool dot, bool aligned) {
  FfmForm f;
  f.vec = (D % 4 == 0 && aligned) ? 4 : 1;
  const long long row = ffm_grad_slab(L, R, D, dot) + (L + R) * D;
  long long rows = (kFfmGradLdsFloats - 3) / row;   // (- 3: the rounding of the slab block)
  if (rows > kFfmTileRowsMax) rows = kFfmTileRowsMax;
  f.lds = rows >= 1;
  f.tile_rows = int(rows);
  return f;
}

}  // namespace mhte
#endif  // MHTE_FFM_CORE_H_
