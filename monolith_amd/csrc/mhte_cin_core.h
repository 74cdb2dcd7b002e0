// The CIN layer (xDeepFM's compressed interaction network) and its gradients: the limits, the tile constants and
// the launch plan — one source for host and device.
// Reference: native_training/layers/feature_cross.py:694-794 (CIN.call).
//
// x0 [B, m, D] as the user gives it, xl / xnext [B, H, D] / [B, U, D] (feature-major, so that the first layer's
// xl is x0 itself), w [H m, U] with the channel index k = h m + j (h-major), bias [U].  A GEMM row is r = b D + d.
//   out[r, u]     = act( sum_{h, j} xl[r, h] x0[r, j] w[h m + j, u] + bias[u] )           xnext[b, u, d]
//   pooled[b, u]  = sum_d out[b D + d, u]                                                 [B, U]
//   g[r, u]       = (dxnext[r, u] + dpooled[b, u]) act'(out[r, u])
//   dz[r, k]      = sum_u g[r, u] w[k, u]                       (never stored)
//   dxl[r, h]     = sum_j dz[r, h m + j] x0[r, j]     dx0[r, j] = sum_h dz[r, h m + j] xl[r, h]
//   dw[k, u]      = sum_r xl[r, h] x0[r, j] g[r, u]   dbias[u]  = sum_r g[r, u]
// The outer product z[r, k] = xl[r, h] x0[r, j] ([B, D, H m] in the reference) exists in registers only.
//
// Every product is v_mfma_f32_32x32x2_f32 (exact fp32); no atomics; the order of every sum is a function of the
// shape alone.
//
// The plan is a function of (B, m, D, H, U) alone:
//   row_block   kCinRowBlock = 128 GEMM rows of a forward workgroup, four wavefronts of one 32-row tile each.  A block
//               holds b_per_block = 128 / D whole b's; its rows beyond b_per_block D are zero rows.
//   col_tiles   32-column tiles of U one wavefront accumulates: 1, 2 or 4; U beyond 32 col_tiles is the grid's y
//   K chunks    the forward enumerates K as (h, pair of j) with m padded to even (mp2 = ceil(m / 2) pairs, the odd
//               slot of the last pair of an odd m is a zero weight row); one MFMA step is one pair.  A chunk is at most
//               kCinSteps = 16 steps: hc = 16 / mp2 whole h's for mp2 <= 16, else one h in two parts of at most 16
//               pairs.  k_chunk = the K rows of a full chunk: hc m, or 32 where an h is cut.
//   slabs       the row slabs of the weight gradient, FeatureInsight's scheme (mhte_fi_core.h): wanted =
//               clamp(ceil(kFiTargetGroups / tiles), 1, kFiMaxSlabs) with tiles = ceil((H m + 1) / 128) *
//               ceil(U / (32 col_tiles)), slab_rows = ceil(B D / wanted) rounded up to 32, slabs = ceil(B D / slab_rows)
//   ws_bytes    slabs (H m + 1) U 4 for slabs > 1 (the partials of dw and, as row H m, of dbias), else 0
//
// Compiled by hipcc inside mhte.hip; on the host alone with MHTE_HOST_ONLY.
#ifndef MHTE_CIN_CORE_H_
#define MHTE_CIN_CORE_H_

#include "mhte_fi_core.h"

namespace mhte {

constexpr int kCinTile = 32;         // rows and columns of an MFMA tile
constexpr int kCinRowBlock = 128;    // GEMM rows of a forward workgroup; K rows of a weight-gradient workgroup
constexpr int kCinSteps = 16;        // MFMA steps (pairs of K rows) per forward chunk; row pairs per dw chunk
constexpr int kCinMaxM = 64;
constexpr int kCinMaxD = 128;
constexpr int kCinMaxH = 512;
constexpr int kCinMaxU = 512;
constexpr long long kCinMaxRows = 1ll << 30;   // B D

// row of the 32x32 accumulator that register reg of lane half h holds (the column is the lane)
MHTE_HD int cin_acc_row(int reg, int h) { return (reg & 3) + 8 * (reg >> 2) + 4 * h; }

struct CinPlan {
  int row_block, b_per_block, col_tiles, mp2, hc, jc, parts;
  long long k_chunk, chunks, slab_rows, slabs, kblocks, ublocks;
  unsigned long long ws_bytes;
};
constexpr int cin_col_tiles(int U) { return U <= 32 ? 1 : (U <= 64 ? 2 : 4); }

// 0 <= B, 1 <= m <= 64, 1 <= D <= 128, 1 <= H <= 512, 1 <= U <= 512, B D <= 2^30
inline CinPlan cin_plan(long long B, int m, int D, int H, int U) {
  CinPlan p;
  p.row_block = kCinRowBlock;
  p.b_per_block = kCinRowBlock / D;
  p.col_tiles = cin_col_tiles(U);
  p.mp2 = (m + 1) / 2;
  p.hc = p.mp2 <= kCinSteps ? kCinSteps / p.mp2 : 1;
  p.jc = p.mp2 <= kCinSteps ? p.mp2 : kCinSteps;
  p.parts = p.mp2 <= kCinSteps ? 1 : 2;
  p.k_chunk = p.parts == 1 ? (long long)p.hc * m : 2 * kCinSteps;
  p.chunks = fi_ceil(H, p.hc) * p.parts;
  const long long K1 = (long long)H * m + 1, R = B * D;
  p.kblocks = fi_ceil(K1, kCinRowBlock);
  p.ublocks = fi_ceil(U, kCinTile * p.col_tiles);
  long long wanted = fi_ceil(kFiTargetGroups, p.kblocks * p.ublocks);
  if (wanted > kFiMaxSlabs) wanted = kFiMaxSlabs;
  if (wanted < 1) wanted = 1;
  p.slab_rows = fi_ceil(fi_ceil(R, wanted), kCinTile) * kCinTile;
  if (p.slab_rows < kCinTile) p.slab_rows = kCinTile;
  p.slabs = R > 0 ? fi_ceil(R, p.slab_rows) : 1;
  p.ws_bytes = p.slabs > 1 ? 4ull * (unsigned long long)p.slabs * (unsigned long long)K1 * (unsigned long long)U : 0;
  return p;
}

// ---- the launch counters: mhte_cin_launch_counts' index ---------------------------------------------------------
enum CinCounter : int {
  kCinCntForward = 0,      // cin_fwd_kernel writing xnext and pooled
  kCinCntForwardLast = 1,  // cin_fwd_kernel without xnext (a last layer)
  kCinCntDx = 2,           // cin_dx_kernel
  kCinCntDw = 3,           // cin_dw_kernel
  kCinCntSlabSum = 4,      // cin_slab_sum_kernel: one when the plan has more than one slab
  kCinCounters = 5
};

}  // namespace mhte
#endif  // MHTE_CIN_CORE_H_
