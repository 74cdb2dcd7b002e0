// AutoInt, the parameter-free self-attention stack over the fields of a sample, and its gradient: the limits, the
// launch plan and the counters — one source for host and device.
// Reference: native_training/layers/feature_trans.py:31-93 (AutoInt.call).
//
// x [B, n, k], out [B, n, k], states [L - 1, B, n, k] (X_1 .. X_{L-1}, only when a gradient is wanted and L > 1).
// Per sample and layer l < L, with X_0 = x[b]:
//   S = X_l X_l^T  [n, n]        P = softmax(S, axis = -1)        X_{l+1} = P X_l        out[b] = X_L
// Gradient, walking the layers last to first with dO = dX_{l+1}, O = X_{l+1}, X = X_l:
//   delta_i = dO_i . O_i      dP = dO X^T      dS = P * (dP - delta)      dX = (dS + dS^T) X + P^T dO
//
// Everything is fp32; every product is an fp32 MFMA; no atomics; the order of every sum is a function of the shape
// alone.  S and P exist in registers only.
//
// The softmax is the exact two-pass one: the row maximum m_i is subtracted, p = e / sum e.  The exponential is
// __expf (v_exp_f32 of the argument times log2 e); its argument is <= 0.  The gradient kernel keeps per row the pair
// (m_i, 1 / sum_i) rather than the log-sum: exp(s - m_i) * (1 / sum_i) is then the forward's P_ij bit for bit, and no
// logarithm of a sum enters the argument of an exponential.  delta_i = dO_i . O_i is taken in its equal form
// sum_j P_ij dP_ij from the P and dP the kernel has anyway: where the softmax saturates (P one-hot) dP_ii - delta_i
// is then exactly 0, as it is in a softmax gradient composed from library calls, while dO_i . O_i summed in another
// order leaves a rounding residue that the following product with X magnifies.  So O is neither staged nor read:
// the gradient entry's out argument is checked and not used, and LDS holds three state buffers.
//
// The plan is a function of (B, n, k, L) alone:
//   tile                   16 for n <= 16 (v_mfma_f32_16x16x4_f32), else 32 (v_mfma_f32_32x32x2_f32)
//   row_tiles              ceil(n / tile) <= 4: the wavefronts of a workgroup; wavefront I owns rows
//                          [I tile, (I + 1) tile) of the sample through all layers
//   padded_k               ceil(k / tile) tile: k is an MFMA's output dimension in P X (tile rows per step) and its
//                          reduction dimension in X X^T (64 / tile per step, which divides tile)
//   samples_per_workgroup  1
//   lds_bytes_forward      4 * 2 * row_tiles tile (padded_k + 1): two state buffers, row stride padded_k + 1 floats
//   lds_bytes_grad         4 * (3 row_tiles tile (padded_k + 1) + 3 row_tiles tile): X_l, dO, dX and the row
//                          statistics (m, 1 / sum, delta)
//   workspace_bytes        0
// Both LDS sizes are at most kAutoIntMaxLds = 163840 at every admitted shape (the largest, n = 128, k = 64:
// 66560 and 101376); above 64 KiB a launch needs the dynamic-LDS attribute, which the host sets once per instance.
//
// Compiled by hipcc inside mhte.hip; on the host alone with MHTE_HOST_ONLY.
#ifndef MHTE_AUTOINT_CORE_H_
#define MHTE_AUTOINT_CORE_H_

#include "mhte_can_core.h"

namespace mhte {

constexpr int kAutoIntMaxN = 128;
constexpr int kAutoIntMaxK = 64;
constexpr int kAutoIntMaxLayers = 8;
constexpr int kAutoIntMaxRowTiles = 4;
constexpr long long kAutoIntMaxBatch = (1ll << 31) - 1;   // the grid's x
constexpr unsigned long long kAutoIntMaxLds = 163840;     // a CU's LDS on gfx950

struct AutoIntPlan {
  int tile, row_tiles, padded_k, samples_per_workgroup;
  unsigned long long lds_fwd, lds_grad, ws_bytes;
};

// 0 <= B, 1 <= n <= 128, 1 <= k <= 64, 1 <= L <= 8
inline AutoIntPlan autoint_plan(long long B, int n, int k, int L) {
  (void)B, (void)L;
  AutoIntPlan p;
  p.tile = n <= 16 ? 16 : 32;
  p.row_tiles = int(fi_ceil(n, p.tile));
  p.padded_k = int(fi_ceil(k, p.tile)) * p.tile;
  p.samples_per_workgroup = 1;
  const unsigned long long rows = (unsigned long long)p.row_tiles * p.tile, stride = p.padded_k + 1;
  p.lds_fwd = 4ull * 2 * rows * stride;
  p.lds_grad = 4ull * (3 * rows * stride + 3 * rows);
  p.ws_bytes = 0;
  return p;
}

// ---- the launch counters: mhte_autoint_launch_counts' index -----------------------------------------------------
enum AutoIntCounter : int {
  kAutoIntCntForward = 0,   // autoint_fwd_kernel
  kAutoIntCntGrad = 1,      // autoint_bwd_kernel
  kAutoIntCounters = 2
};

}  // namespace mhte
#endif  // MHTE_AUTOINT_CORE_H_
