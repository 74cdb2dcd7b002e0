// FeatureInsight, its gradient and the fused aggregate: the per-element arithmetic, the tile constants and the
// launch plan — one source for host and device.
// Reference: native_training/layers/ops/feature_insight_ops.cc, layers/kernels/feature_insight_kernels.cc:70-83
// (forward) and :148-160 (gradient), layers/layer_ops.py:49-85.
//
// input [B, E], weight [E, K], segment f covers columns o_f .. o_f + s_f - 1 of input and the same rows of weight:
//   out[b, f K + k]    = sum_{j in seg f} input[b, j] * weight[j, k]                        [B, F K]
//   input_grad[b, j]   = sum_k grad[b, f(j) K + k] * weight[j, k]                           [B, E]
//   weight_grad[j, k]  = sum_b grad[b, f(j) K + k] * input[b, j]                            [E, K]
//   agg[b, f]          = sum_k out[b, f K + k]^2                                            [B, F]
//
// THE fp32 DEFINITION (what tests/feature_insight_truth.py restates bit for bit).  Every sum is a chain
//   acc = +0;  acc = fmaf(a_t, b_t, acc)  for t ascending                                   (fi_chain)
// over the segment's columns (out), over k (input_grad), over the rows of one batch slab (weight_grad).  The slabs
// of weight_grad are rows [i * slab_rows, min(B, (i + 1) * slab_rows)); their partials are added in slab order,
// starting from the first (fi_slab_sum).  agg squares the rounded out values: kFiLanes = 16 lane chains, lane l
// over k = l, l + 16, l + 32, ... ascending with p = fmaf(out, out, p) from +0, then the 16 lane sums are added in
// lane order starting from lane 0 (fi_agg).  A chain that starts at +0 never yields -0: every zero is +0.
//
// The plan is a function of (B, E, K, F) alone:
//   row_block     kFiTile = 64 rows of input / out / grad one workgroup owns (forward, input gradient)
//   col_tile      kFiTile = 64 output columns of one workgroup
//   stage         kFiStage = 32 terms of a chain per LDS stage; a longer chain loops
//   slabs         the batch slabs of the weight gradient: wanted = clamp(ceil(kFiTargetGroups / tiles), 1,
//                 kFiMaxSlabs) with tiles = max(F, ceil(E / 64)) * ceil(K / 64) (the output tiles the gradient has at
//                 least), slab_rows = ceil(B / wanted) rounded up to kFiTile, slabs = ceil(B / slab_rows)
//   grad_bytes    the workspace of the gradient: slabs * E * K * 4 for slabs > 1 (the partials), else 0
//   forward_bytes 0, in both modes
// A list of more than kFiInline segments is cut into groups of kFiInline consecutive segments, one launch per group:
// the offsets of a launch always ride in its kernel arguments (nothing is uploaded, nothing can go stale).
//
// Compiled by hipcc inside mhte.hip and, for the CPU suite (tests/fi_host_driver.cc), by g++ with MHTE_HOST_ONLY.
#ifndef MHTE_FI_CORE_H_
#define MHTE_FI_CORE_H_

#include <math.h>
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

constexpr int kFiTile = 64;            // rows and columns of an output tile
constexpr int kFiStage = 32;           // chain terms per LDS stage
constexpr int kFiLanes = 16;           // lane chains of the aggregate; column c of a tile belongs to lane c % 16
constexpr int kFiInline = 128;         // segments whose offsets ride in one launch's arguments
constexpr int kFiMaxSegments = 4096;   // the cap on n_segments: 32 launches
constexpr int kFiMaxSlabs = 64;
constexpr int kFiTargetGroups = 2048;  // workgroups the weight gradient aims at: eight per CU
constexpr long long kFiMaxExtent = (1ll << 30) - kFiTile;   // batch, inclusive: row blocks * kFiInline is a grid's x

// ---- the per-element arithmetic ------------------------------------------------------------------------------
MHTE_HD float fi_fma(float a, float b, float acc) { return fmaf(a, b, acc); }

// sum_{t < n} a[t * sa] * b[t * sb], the chain of the definition
MHTE_HD float fi_chain(const float* a, long long sa, const float* b, long long sb, long long n) {
  float acc = 0.f;
  for (long long t = 0; t < n; ++t) acc = fi_fma(a[t * sa], b[t * sb], acc);
  return acc;
}
// the partials of the slabs, in slab order
MHTE_HD float fi_slab_sum(const float* part, long long stride, int slabs) {
  float t = part[0];
  for (int i = 1; i < slabs; ++i) t += part[i * stride];
  return t;
}
// the aggregate of one (row, feature) from its K rounded out values
MHTE_HD float fi_agg(const float* out, int k) {
  float lane[kFiLanes];
  for (int l = 0; l < kFiLanes; ++l) {
    float p = 0.f;
    for (int c = l; c < k; c += kFiLanes) p = fi_fma(out[c], out[c], p);
    lane[l] = p;
  }
  float t = lane[0];
  for (int l = 1; l < kFiLanes; ++l) t += lane[l];
  return t;
}

// ---- the plan -------------------------------------------------------------------------------------------------
struct FiPlan {
  int row_block, col_tile, stage, inline_segments;
  long long slab_rows, slabs, groups;
  unsigned long long forward_bytes, grad_bytes;
};
inline long long fi_ceil(long long a, long long b) { return (a + b - 1) / b; }
// 0 <= B <= kFiMaxExtent, 0 <= E, 1 <= K, 1 <= F
inline FiPlan fi_plan(long long B, long long E, long long K, long long F) {
  FiPlan p;
  p.row_block = kFiTile;
  p.col_tile = kFiTile;
  p.stage = kFiStage;
  p.inline_segments = kFiInline;
  p.groups = fi_ceil(F, kFiInline);
  const long long etiles = fi_ceil(E, kFiTile);
  const long long tiles = (F > etiles ? F : etiles) * fi_ceil(K, kFiTile);
  long long wanted = fi_ceil(kFiTargetGroups, tiles);
  if (wanted > kFiMaxSlabs) wanted = kFiMaxSlabs;
  if (wanted < 1) wanted = 1;
  p.slab_rows = fi_ceil(fi_ceil(B, wanted), kFiTile) * kFiTile;
  if (p.slab_rows < kFiTile) p.slab_rows = kFiTile;
  p.slabs = B > 0 ? fi_ceil(B, p.slab_rows) : 1;
  p.forward_bytes = 0;
  p.grad_bytes = p.slabs > 1 ? 4ull * (unsigned long long)p.slabs * (unsigned long long)E * (unsigned long long)K : 0;
  return p;
}

// ---- the launch counters: mhte_feature_insight_launch_counts' index ---------------------------------------------
enum FiCounter : int {
  kFiCntForward = 0,      // fi_forward_kernel, plain: one per group of kFiInline segments
  kFiCntAggregate = 1,    // fi_forward_kernel, aggregate: the same
  kFiCntInputGrad = 2,    // fi_input_grad_kernel: the same
  kFiCntWeightGrad = 3,   // fi_weight_grad_kernel: the same
  kFiCntSlabSum = 4,      // fi_slab_sum_kernel: one when the plan has more than one slab
  kFiCounters = 5
};

}  // namespace mhte
#endif  // MHTE_FI_CORE_H_
