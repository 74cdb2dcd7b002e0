// The CAN co-action unit (Co-Action Network) and its gradients: the limits, the MFMA index maps and the launch
// plan — one source for host and device.
// Reference: native_training/layers/feature_cross.py:345-440 (CAN.call, its four input forms).
//
// user [B, F, T, d] (R = F T rows per sample), item [B, P], P = L d (d + 1), out [B, F, d].  Per sample b and
// layer i < L:   W_i[k][j] = item[b, i d (d + 1) + k d + j]      b_i[j] = item[b, i d (d + 1) + d d + j]
//   h_0 = user[b]        h_{i+1} = act(h_i W_i + b_i)   (on EVERY layer)        out[b, f] = sum_t h_L[f T + t]
//   dh_L[f T + t] = dout[b, f]     dpre_i = dh_{i+1} * (h_{i+1} > 0)  (relu; else dh_{i+1})
//   dh_i = dpre_i W_i^T            dW_i = sum_rows h_i^T dpre_i            db_i = sum_rows dpre_i
// duser = dh_0, ditem [B, P] holds (dW_i, db_i) where item holds (W_i, b_i).
//
// Everything is fp32; every product is an fp32 MFMA; no atomics; the order of every sum is a function of the shape
// alone.
//
// The plan is a function of (B, F, T, d, L) alone.
//   padded_d               16 for d <= 16 (v_mfma_f32_16x16x4_f32), else 32 (v_mfma_f32_32x32x2_f32); the padding
//                          lives in registers and LDS only
//   rows_per_tile          = padded_d: the rows one MFMA chain carries, lane = row
//   tiles_per_sample       ceil(R / rows_per_tile), walked in ascending order by the sample's wavefront
//   samples_per_workgroup  kCanSamples = 1: a workgroup is ONE wavefront, so that its barriers around the LDS
//                          transpositions are wavefront-local and cost nothing
//   lds_bytes              4 (L padded_d (padded_d + 1)   the sample's W_i, zero padded, row stride padded_d + 1
//                             + L padded_d                ... b_i
//                             + 2 padded_d (padded_d + 1)) the two transposition tiles (the forward uses one)
//   workspace_bytes        0: a sample's gradient sums stay in its wavefront's registers
//
// Compiled by hipcc inside mhte.hip; on the host alone with MHTE_HOST_ONLY.
#ifndef MHTE_CAN_CORE_H_
#define MHTE_CAN_CORE_H_

#include "mhte_cin_core.h"

namespace mhte {

constexpr int kCanMaxD = 32;
constexpr int kCanMaxLayers = 8;
constexpr int kCanSamples = 1;                  // samples (wavefronts) of a workgroup
constexpr long long kCanMaxRows = 1ll << 30;    // F T
constexpr long long kCanMaxBatch = (1ll << 31) - 1;   // the grid's x

// The reduction index of k-slot q at MFMA step s, which is also the output row of accumulator register s in lane
// group q: PD == 16 (16x16x4, q < 4, s < 4): 4 q + s;  PD == 32 (32x32x2, q < 2, s < 16): cin_acc_row(s, q).
// With this one map on both operands a layer's accumulator IS the next layer's B operand.
template <int PD>
MHTE_HD int can_kidx(int s, int q) {
  return PD == 16 ? 4 * q + s : cin_acc_row(s, q);
}

struct CanPlan {
  int rows_per_tile, padded_d, samples_per_workgroup;
  long long tiles_per_sample;
  unsigned long long lds_bytes, ws_bytes;
};

// 0 <= B, 1 <= F, T, F T <= 2^30, 1 <= d <= 32, 1 <= L <= 8
inline CanPlan can_plan(long long B, long long F, long long T, int d, int L) {
  (void)B;
  CanPlan p;
  p.padded_d = d <= 16 ? 16 : 32;
  p.rows_per_tile = p.padded_d;
  p.samples_per_workgroup = kCanSamples;
  p.tiles_per_sample = fi_ceil(F * T, p.rows_per_tile);
  const unsigned long long pd = (unsigned long long)p.padded_d;
  p.lds_bytes = 4ull * ((unsigned long long)L * pd * (pd + 1) + (unsigned long long)L * pd + 2 * pd * (pd + 1));
  p.ws_bytes = 0;
  return p;
}

// ---- the launch counters: mhte_can_launch_counts' index ---------------------------------------------------------
enum CanCounter : int {
  kCanCntForward = 0,   // can_fwd_kernel
  kCanCntGrad = 1,      // can_bwd_kernel
  kCanCounters = 2
};

}  // namespace mhte
#endif  // MHTE_CAN_CORE_H_
