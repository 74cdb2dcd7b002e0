// The DCN cross layer (Deep & Cross Network, vector and matrix form) and its gradients: the limits, the tile
// constants and the launch plan — one source for host and device.
// Reference: native_training/layers/feature_cross.py:445-690 (DCN.call, the Vector and Matrix branches).
//
// x0, xl, xnext, g = dxnext are [B, d]; bias [d].
//   vector (type 0), w [d]:      s[b]    = sum_k xl[b, k] w[k]               xnext = (x0 s[b] + bias) + xl
//                                ds[b]   = sum_j g[b, j] x0[b, j]            dxl = ds[b] w + g     dx0 += g s[b]
//                                dw[k]   = sum_b ds[b] xl[b, k]              dbias[j] = sum_b g[b, j]
//   matrix (type 1), w [d, d]:   u[b, j] = sum_k xl[b, k] w[k, j] + bias[j]  xnext = x0 u + xl
//                                du      = g x0  (never stored)              dxl = du w^T + g      dx0 += g u
//                                dw[k, j] = sum_b xl[b, k] du[b, j]          dbias[j] = sum_b du[b, j]
// aux is what the gradient needs of the forward: s [B] (vector), u [B, d] (matrix).
//
// Everything is fp32; every product of the matrix form is v_mfma_f32_32x32x2_f32; no atomics; the order of every sum
// is a function of the shape alone.
//
// The plan is a function of (B, d, type) alone.
//   matrix  row_block   kDcnRowBlock = 128 rows of a workgroup (forward and input gradient: rows of the batch; weight
//                       gradient: K rows of dw, K row d being dbias), four wavefronts of one 32-row tile each
//           col_tiles   32-column tiles one wavefront accumulates: 1, 2 or 4; col_span = 32 col_tiles columns of a
//                       workgroup, more of d is the grid's y
//           k_chunk     kDcnChunk = 32 rows of the reduction staged at a time (16 MFMA steps)
//           slabs       the row slabs of the weight gradient, FeatureInsight's scheme (mhte_fi_core.h): wanted =
//                       clamp(ceil(kFiTargetGroups / tiles), 1, kFiMaxSlabs), tiles = ceil((d + 1) / 128) *
//                       ceil(d / col_span), slab_rows = ceil(B / wanted) rounded up to 32, slabs = ceil(B / slab_rows)
//           ws_bytes    slabs (d + 1) d 4 for slabs > 1 (the partials of dw and, as K row d, of dbias), else 0
//   vector  row_block   kDcnVecRows = 64 rows of a forward workgroup, 16 per wavefront
//           k_chunk     64: the lanes of a wavefront; a row of d <= 32 takes lanes = the next power of two and a
//                       wavefront holds 64 / lanes rows at a time
//           col_span    64 vpl: the columns the kernel instance keeps in registers, vpl (values per lane) the
//                       smallest of 1, 4, 16, 64 that covers d
//           slabs       the row slabs of the gradient, one workgroup each: slab_rows = ceil(B / kDcnVecMaxSlabs) rounded
//                       up to 64, slabs = ceil(B / slab_rows)
//           ws_bytes    slabs 2 d 4 for slabs > 1 (the partials of dw, then of dbias), else 0
//
// Compiled by hipcc inside mhte.hip; on the host alone with MHTE_HOST_ONLY.
#ifndef MHTE_DCN_CORE_H_
#define MHTE_DCN_CORE_H_

#include "mhte_cin_core.h"

namespace mhte {

constexpr int kDcnVector = 0, kDcnMatrix = 1;   // the ABI's type
constexpr int kDcnTile = 32;          // rows and columns of an MFMA tile
constexpr int kDcnRowBlock = 128;     // rows of a matrix workgroup
constexpr int kDcnChunk = 32;         // reduction rows per staged chunk
constexpr int kDcnSteps = kDcnChunk / 2;
constexpr int kDcnVecRows = 64;       // rows of a vector forward workgroup; the unit of the vector slabs
constexpr int kDcnVecMaxSlabs = 512;
constexpr int kDcnMaxD = 4096;
constexpr long long kDcnMaxElems = 1ll << 31;   // B d

struct DcnPlan {
  int row_block, col_tiles, col_span, k_chunk, lanes, vpl;
  long long slab_rows, slabs, kblocks, cblocks;
  unsigned long long ws_bytes;
};

// 0 <= B, 1 <= d <= 4096, B d <= 2^31, type 0 or 1
inline DcnPlan dcn_plan(long long B, int d, int type) {
  DcnPlan p;
  if (type == kDcnMatrix) {
    p.row_block = kDcnRowBlock;
    p.col_tiles = d <= 32 ? 1 : (d <= 64 ? 2 : 4);
    p.col_span = kDcnTile * p.col_tiles;
    p.k_chunk = kDcnChunk;
    p.lanes = 64, p.vpl = 0;
    p.kblocks = fi_ceil(d + 1, kDcnRowBlock);
    p.cblocks = fi_ceil(d, p.col_span);
    long long wanted = fi_ceil(kFiTargetGroups, p.kblocks * p.cblocks);
    if (wanted > kFiMaxSlabs) wanted = kFiMaxSlabs;
    if (wanted < 1) wanted = 1;
    p.slab_rows = fi_ceil(fi_ceil(B, wanted), kDcnTile) * kDcnTile;
    if (p.slab_rows < kDcnTile) p.slab_rows = kDcnTile;
    p.slabs = B > 0 ? fi_ceil(B, p.slab_rows) : 1;
    p.ws_bytes = p.slabs > 1 ? 4ull * (unsigned long long)p.slabs * (unsigned long long)(d + 1) * (unsigned long long)d : 0;
  } else {
    p.row_block = kDcnVecRows;
    p.col_tiles = 0;
    p.lanes = 64;
    while (p.lanes / 2 >= d) p.lanes /= 2;
    p.vpl = d <= 64 ? 1 : (d <= 256 ? 4 : (d <= 1024 ? 16 : 64));
    p.col_span = 64 * p.vpl;
    p.k_chunk = 64;
    p.kblocks = p.cblocks = 1;
    p.slab_rows = fi_ceil(fi_ceil(B, kDcnVecMaxSlabs), kDcnVecRows) * kDcnVecRows;
    if (p.slab_rows < kDcnVecRows) p.slab_rows = kDcnVecRows;
    p.slabs = B > 0 ? fi_ceil(B, p.slab_rows) : 1;
    p.ws_bytes = p.slabs > 1 ? 8ull * (unsigned long long)p.slabs * (unsigned long long)d : 0;
  }
  return p;
}

// ---- the launch counters: mhte_dcn_launch_counts' index ---------------------------------------------------------
enum DcnCounter : int {
  kDcnCntMatForward = 0,      // dcn_mat_fwd_kernel writing u
  kDcnCntMatForwardNoAux = 1, // ... without (inference)
  kDcnCntMatDx = 2,           // dcn_mat_dx_kernel
  kDcnCntMatDw = 3,           // dcn_mat_dw_kernel
  kDcnCntMatSlabSum = 4,      // cin_slab_sum_kernel over the matrix partials
  kDcnCntVecForward = 5,      // dcn_vec_fwd_kernel writing s
  kDcnCntVecForwardNoAux = 6, // ... without
  kDcnCntVecGrad = 7,         // dcn_vec_grad_kernel: dxl, dx0 and the partials of dw and dbias in one launch
  kDcnCntVecSlabSum = 8,      // cin_slab_sum_kernel over the vector partials
  kDcnCounters = 9
};

}  // namespace mhte
#endif  // MHTE_DCN_CORE_H_
