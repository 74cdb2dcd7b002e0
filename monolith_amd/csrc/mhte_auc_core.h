// The in-batch AUC loss and its gradient: the classification of the labels, the two term functions with their
// branches, the tile and chunk constants and the launch plan — one source for host and device.
// Reference: InbatchAucLoss / InbatchAucLossGrad, runtime/ops/inbatch_auc_loss.cc:30-138 (CPU only, two nested
// loops, one float accumulator); the Python side is native_training/losses/inbatch_auc_loss.py, its test
// losses/inbatch_auc_loss_test.py.
//
// label and logit are fp32 with equal element counts.  Element i is POSITIVE if label[i] > 0, NEGATIVE if it is
// not positive and label[i] > -10000, IGNORED otherwise (a NaN label is ignored).  For every positive i and
// negative j, diff = logit[i] - logit[j] (one fp32 subtraction) and
//   -87 < diff < 88:  t = diff - log(1 + exp(diff)) = log sigmoid(diff),  s = 1 - 1 / (1 + exp(-diff)) = sigmoid(-diff)
//   diff <= -87:      t = diff,                                            s = 1
//   otherwise (diff >= 88, or NaN):  t = 0,                                s = 0
//   loss = sum t_ij (<= 0: the reference's sign, callers negate)
//   logit_grad[i] = grad * sum_j s_ij (positive),  logit_grad[j] = -grad * neg_weight * sum_i s_ij (negative),
//   +0 for an ignored element, for every element when there is no positive or no negative, and wherever the
//   product is a zero of either sign.
// The reference evaluates the middle branch in double; here it is fp32 in the form that cancels nothing: with
// e = exp(-|diff|):  t = -log1p(e) (diff >= 0), diff - log1p(e) (diff < 0);  s = e / (1 + e) (diff >= 0),
// 1 / (1 + e) (diff < 0).  Every sum is fp64 in an order fixed by n, the number of positives and the number of
// negatives, and is rounded to fp32 once (the gradient after its multiplication by neg_weight and grad).
// tests/inbatch_auc_truth.py restates all of it.
//
// Compiled by hipcc inside mhte.hip and, for the CPU suite (tests/auc_host_driver.cc), by g++ with
// MHTE_HOST_ONLY defined.
#ifndef MHTE_AUC_CORE_H_
#define MHTE_AUC_CORE_H_

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

constexpr int kAucThreads = 256;
// The pair kernel's work item: kAucTile elements of one class in registers (one per thread) against one chunk of
// the other class, which passes through LDS kAucStage floats at a time and is read there as broadcasts.  A chunk
// is a multiple of kAucChunk elements.
constexpr int kAucTile = 256;
constexpr int kAucChunk = 256;
constexpr int kAucStage = 1024;
constexpr int kAucScanTile = 1024;    // elements per workgroup of the compaction (4 per thread)
constexpr int kAucMaxGroups = 2048;   // workgroups of the pair kernel at most (8 per CU): the grid strides beyond
constexpr int kAucGroupElems = 64;    // ... and one per this many elements of the batch below that
// doubles of per-chunk partial sums per side at least: 2048 work items of kAucTile rows (4 MiB)
constexpr long long kAucMinBudget = 1ll << 19;

// ---- classification -----------------------------------------------------------------------------------------
enum AucClass : int { kAucIgnored = 0, kAucPositive = 1, kAucNegative = 2 };
MHTE_HD int auc_classify(float label) {
  return label > 0.f ? kAucPositive : (label > -10000.f ? kAucNegative : kAucIgnored);
}

// ---- the terms ----------------------------------------------------------------------------------------------
// log1p(e) for e in [0, 1]: the logarithm of the rounded u = 1 + e, plus what the rounding of u lost, (e - (u - 1)) / u
// (both differences are exact; the correction is below half an ulp of u, so an approximate reciprocal serves it).
// logf is within 1 ulp and the sum adds half of one: within the 2 ulp a library log1pf is allowed, at far fewer
// instructions than the device library's, which works in double-float arithmetic.
MHTE_HD float auc_log1p_unit(float e) {
  const float u = 1.f + e;
  const float lost = e - (u - 1.f);
#if defined(__HIP_DEVICE_COMPILE__)
  const float c = lost * __builtin_amdgcn_rcpf(u);
#else
  const float c = lost / u;
#endif
  return logf(u) + c;
}

// t and s of one pair; they share e.  Selects, no branches: a NaN diff fails every comparison and gives (0, 0).
MHTE_HD void auc_terms(float diff, float* t, float* s) {
  const float e = expf(-fabsf(diff));
  const float l = auc_log1p_unit(e);
  const bool up = diff >= 0.f;
  const float tm = up ? -l : diff - l;
  const float sm = (up ? e : 1.f) / (1.f + e);
  const bool mid = diff > -87.f && diff < 88.f;
  const bool low = diff <= -87.f;
  *t = mid ? tm : (low ? diff : 0.f);
  *s = mid ? sm : (low ? 1.f : 0.f);
}
MHTE_HD float auc_loss_term(float diff) {
  float t, s;
  auc_terms(diff, &t, &s);
  return t;
}
MHTE_HD float auc_grad_weight(float diff) {
  float t, s;
  auc_terms(diff, &t, &s);
  return s;
}
// The rounding of a gradient element: sum is the fp64 sum of its s, scale = grad (positive) or
// -grad * neg_weight (negative) in fp64; a zero of either sign is +0.
MHTE_HD float auc_grad_round(double sum, double scale) {
  const float g = float(sum * scale);
  return g == 0.f ? 0.f : g;
}

// ---- the split of one sweep, computed on the device from the counts -----------------------------------------
// A sweep holds the A elements of one class in registers, a_tiles tiles of kAucTile, and cuts the B elements of
// the other class into `chunks` chunks of chunk_len (the last one shorter).  Work item k = c * a_tiles + a_tile.
// The partial sum of element a over chunk c lies at part[c * stride + a]: chunks * stride <= budget.
struct AucSplit {
  uint32_t a_tiles, chunks, chunk_len;
  uint64_t stride;
};
MHTE_HD AucSplit auc_split(uint32_t A, uint32_t B, uint64_t budget) {
  AucSplit s;
  s.a_tiles = (A + uint32_t(kAucTile) - 1) / uint32_t(kAucTile);
  s.stride = uint64_t(s.a_tiles) * uint64_t(kAucTile);
  s.chunks = 0;
  s.chunk_len = uint32_t(kAucChunk);
  if (A == 0 || B == 0) return s;
  uint64_t cmax = budget / s.stride;   // (the plan's budget holds one chunk of any A <= n)
  if (cmax < 1) cmax = 1;
  const uint64_t minis = (uint64_t(B) + uint64_t(kAucChunk) - 1) / uint64_t(kAucChunk);
  const uint64_t c = cmax < minis ? cmax : minis;
  const uint64_t per = (minis + c - 1) / c;
  s.chunk_len = uint32_t(per * uint64_t(kAucChunk));
  s.chunks = uint32_t((minis + per - 1) / per);
  return s;
}
MHTE_HD uint64_t auc_items(const AucSplit& s) { return uint64_t(s.a_tiles) * uint64_t(s.chunks); }

// ---- the host's launch plan: a function of n alone (P and N never reach the host) ---------------------------
struct AucPlan {
  uint32_t scan_tiles;    // workgroups of the count and the scatter kernel
  uint32_t pair_groups;   // workgroups of the pair kernel
  uint32_t final_groups;  // workgroups of the final pass with a gradient (the loss alone: one)
  uint64_t budget;        // doubles of partial sums per side
  uint64_t loss_slots;    // per-item loss partials: items of one sweep at most
  // the workspace: byte offsets of its arrays (256-byte aligned) and its size
  uint64_t off_counts, off_tile_counts, off_tile_offsets, off_pos, off_neg, off_rank, off_loss_part, off_row_part,
      off_col_part, bytes;
};
inline uint64_t auc_up(uint64_t x, uint64_t a) { return (x + a - 1) / a * a; }
// 0 < n < 2^31
inline AucPlan auc_plan(long long n) {
  AucPlan p;
  const uint64_t un = uint64_t(n);
  p.scan_tiles = uint32_t((un + kAucScanTile - 1) / kAucScanTile);
  const uint64_t g = (un + kAucGroupElems - 1) / kAucGroupElems;
  p.pair_groups = uint32_t(g < 1 ? 1 : (g > uint64_t(kAucMaxGroups) ? uint64_t(kAucMaxGroups) : g));
  const uint64_t f = (un + kAucThreads - 1) / kAucThreads;
  p.final_groups = uint32_t(f > uint64_t(kAucMaxGroups) ? uint64_t(kAucMaxGroups) : f);
  const uint64_t one = auc_up(un, kAucTile);   // one chunk of every element
  p.budget = one > uint64_t(kAucMinBudget) ? one : uint64_t(kAucMinBudget);
  p.loss_slots = p.budget / kAucTile;
  uint64_t o = 0;
  auto take = [&o](uint64_t bytes) {
    const uint64_t at = o;
    o += auc_up(bytes, 256);
    return at;
  };
  p.off_counts = take(16);
  p.off_tile_counts = take(8ull * p.scan_tiles);
  p.off_tile_offsets = take(8ull * p.scan_tiles);
  p.off_pos = take(4 * un);
  p.off_neg = take(4 * un);
  p.off_rank = take(4 * un);
  p.off_loss_part = take(8 * p.loss_slots);
  p.off_row_part = take(8 * p.budget);
  p.off_col_part = take(8 * p.budget);
  p.bytes = o;
  return p;
}

// ---- the launch counters: mhte_inbatch_auc_launch_counts' index ----------------------------------------------
enum AucCounter : int {
  kAucCntCount = 0,        // compaction: classes per tile
  kAucCntScan = 1,         // ... their scan, P and N
  kAucCntScatter = 2,      // ... the stable scatter
  kAucCntPairLoss = 3,     // pair kernel: loss alone (one sweep)
  kAucCntPairLossGrad = 4, // ... loss and both sums (two sweeps in one launch)
  kAucCntPairGrad = 5,     // ... both sums, no loss
  kAucCntFinalLoss = 6,    // final pass, the same three
  kAucCntFinalLossGrad = 7,
  kAucCntFinalGrad = 8,
  kAucCounters = 9
};

}  // namespace mhte
#endif  // MHTE_AUC_CORE_H_
