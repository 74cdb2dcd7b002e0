// The sampling-bias-corrected in-batch softmax loss and its gradients: the per-element arithmetic, the tile
// constants and the launch plan — one source for host and device.
// Reference: native_training/losses/batch_softmax_loss.py:18-57; the only consumer of the interval that
// BatchSoftmaxOptimizer (MHTE_OPT_BATCH_SOFTMAX, batch_softmax_step in mhte_core.h) keeps per item id.
//
// query, item [B, k], item_step_interval [B], r [B], all fp32:
//   q^_i = q_i * rsqrt(max(sum q_i^2, 1e-12))        (tf.linalg.l2_normalize; likewise i^_j; identity if !normalize)
//   c_j  = log(max(item_step_interval_j, 1))         (= -log(item_frequency_j))
//   z_ij = (q^_i . i^_j) / temperature + c_j
//   lse_i = m_i + log sum_j exp(z_ij - m_i),  m_i = max_j z_ij
//   loss = - sum_i r_i * (z_ii - lse_i)
// THE ONE DEFINED DEVIATION: the reference takes exp of the unshifted similarity and divides
// (exp(z_ii) / sum_j exp(z_ij), then log), which overflows in fp32 (normalised inputs at temperature 0.01:
// exp(100) = inf, inf / inf = NaN).  Wherever the reference's own fp32 evaluation is finite this is the same
// value; where it overflows, this stays finite.
// Gradients for query and item only, with G_ij = r_i * (exp(z_ij - lse_i) - [i == j]):
//   g_q^ = G . I^ / temperature,   g_i^ = G^T . Q^ / temperature
//   through the normalisation of a row x with s = sum x^2, inv = rsqrt(max(s, 1e-12)), x^ = x * inv:
//     s >= 1e-12: dx = (g - x^ * (x^ . g)) * inv        s < 1e-12: dx = g * inv  (= g * 1e6)
//
// The plan is a pure function of (B, k):
//   kp          k padded with zeros to a multiple of kBsmKPad = 8 (four K steps of v_mfma_f32_32x32x2_f32: a lane
//               fetches its operand as one 16-byte LDS read per four instructions)
//   nb          the kernel form: 1, 2, 4 or 8 blocks of 32 output columns, the smallest with 32 * nb >= kp
//   row_block   rows (columns for the item gradient) one workgroup owns: 128 for nb <= 2, 64 beyond (LDS)
//   tile        kBsmTile = 32 rows of the streamed operand per step
//   bp          B rounded up to row_block: every per-row array of the workspace has bp rows, the padding is zero
//   tiles       ceil(B / 32);  tiles_per_chunk = ceil(tiles / wanted),  chunks = ceil(tiles / tiles_per_chunk) with
//               wanted = clamp(ceil(kBsmTargetGroups / (bp / row_block)), 1, min(tiles, kBsmMaxChunks)): the grid
//               (bp / row_block) x chunks is of the order of twice the CU count for any B; chunk c streams the
//               tiles [c * tiles_per_chunk, min(tiles, (c + 1) * tiles_per_chunk))
// Workspace, in floats (every array starts at a multiple of 256 bytes):
//   6 bp                   inv and sum of squares of both operands, c, the diagonal z_ii
//   2 bp kp                Q^ / temperature and I^, zero padded
//   2 chunks bp + bp       the (m, l) partials and lse
//   2 chunks bp kp         the per-chunk partials of G . I^ and G^T . Q^
// B = 65536, k = 64: one chunk, 2 * 16 MiB + 2 * 16 MiB + 2.25 MiB = 66.25 MiB (69 468 160 bytes).  While there is
// more than one chunk, chunks * bp is about kBsmTargetGroups * row_block, so the two partial arrays together stay
// near 2 * 512 * row_block * kp * 4 bytes: 32 MiB at k = 64 (16 chunks up to B = 4096), 64 MiB at k = 256 (16 chunks
// up to B = 2048, 8 at B = 4096); with one chunk they grow as 8 bp kp bytes.
// LDS per workgroup, static: (row_block + 32) * (32 nb + 4) * 4 + 256 bytes: 22.8 KB (nb = 1), 42.8 KB (nb = 2),
// 49.8 KB (nb = 4), 97.8 KB (nb = 8, k' > 128).  The last is above the 64 KB of most targets; gfx950 has 160 KB per
// CU, on which it leaves room for ONE 128-thread workgroup per CU (two wavefronts): k' > 128 runs at that
// occupancy.  Nothing was measured at k > 64.
//
// Compiled by hipcc inside mhte.hip and, for the CPU suite (tests/bsm_host_driver.cc), by g++ with
// MHTE_HOST_ONLY defined.
#ifndef MHTE_BSM_CORE_H_
#define MHTE_BSM_CORE_H_

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

constexpr int kBsmMaxDim = 256;
constexpr long long kBsmMaxBatch = 1ll << 24;   // exclusive
constexpr int kBsmKPad = 8;
constexpr int kBsmTile = 32;
constexpr int kBsmMaxChunks = 16;
constexpr int kBsmTargetGroups = 512;     // workgroups of a sweep the plan aims at: two per CU
constexpr int kBsmFinalThreads = 1024;    // the one workgroup that merges the (m, l) partials and sums the loss
constexpr float kBsmNormEps = 1e-12f;

// ---- the per-element arithmetic ------------------------------------------------------------------------------
MHTE_HD float bsm_inv(float sumsq) { return 1.f / sqrtf(fmaxf(sumsq, kBsmNormEps)); }
MHTE_HD bool bsm_eps_branch(float sumsq) { return sumsq < kBsmNormEps; }
MHTE_HD float bsm_c(float interval) { return logf(fmaxf(interval, 1.f)); }

// the running maximum m and the sum l of exp(z - m) over a set of z; the empty set is (-inf, 0)
struct BsmML {
  float m, l;
};
MHTE_HD BsmML bsm_empty() { return BsmML{-INFINITY, 0.f}; }
// a then b: the order is part of the result's bits
MHTE_HD BsmML bsm_merge(BsmML a, BsmML b) {
  const float m = fmaxf(a.m, b.m);
  if (!(m > -INFINITY)) return bsm_empty();
  return BsmML{m, a.l * expf(a.m - m) + b.l * expf(b.m - m)};
}
MHTE_HD float bsm_lse(BsmML x) { return x.m + logf(x.l); }

// the normalisation backward of one element: g the gradient at x^, dot = x^ . g over the row
MHTE_HD float bsm_dx(float g, float xhat, float dot, float inv, bool eps_branch) {
  return eps_branch ? g * inv : (g - xhat * dot) * inv;
}
// a zero of either sign is written as +0
MHTE_HD float bsm_pos_zero(float x) { return x == 0.f ? 0.f : x; }

// the row of a 32x32 MFMA result that register reg of a lane of half h (lane >> 5) holds; its column is lane & 31
MHTE_HD int bsm_acc_row(int reg, int h) { return (reg & 3) + 8 * (reg >> 2) + 4 * h; }

// ---- the plan -------------------------------------------------------------------------------------------------
MHTE_HD int bsm_kp(int k) { return (k + kBsmKPad - 1) / kBsmKPad * kBsmKPad; }
MHTE_HD int bsm_nb(int kp) { return kp <= 32 ? 1 : (kp <= 64 ? 2 : (kp <= 128 ? 4 : 8)); }
constexpr int bsm_row_block(int nb) { return nb <= 2 ? 128 : 64; }

struct BsmPlan {
  int kp, nb, row_block, tile;
  uint32_t blocks;            // bp / row_block: grid.x of a sweep
  uint32_t tiles, tiles_per_chunk, chunks;   // chunks: grid.y of a sweep
  uint64_t bp;
  // the workspace: byte offsets of its arrays (256-byte aligned) and its size
  uint64_t off_inv_q, off_inv_i, off_ss_q, off_ss_i, off_c, off_zd, off_qs, off_is, off_ml_m, off_ml_l, off_lse,
      off_dq_part, off_di_part, bytes;
};
inline uint64_t bsm_up(uint64_t x, uint64_t a) { return (x + a - 1) / a * a; }
// 0 <= B < 2^24, 1 <= k <= 256
inline BsmPlan bsm_plan(long long B, int k) {
  BsmPlan p;
  p.kp = bsm_kp(k);
  p.nb = bsm_nb(p.kp);
  p.row_block = bsm_row_block(p.nb);
  p.tile = kBsmTile;
  const uint64_t ub = uint64_t(B);
  p.bp = bsm_up(ub, uint64_t(p.row_block));
  p.blocks = uint32_t(p.bp / uint64_t(p.row_block));
  p.tiles = uint32_t((ub + kBsmTile - 1) / kBsmTile);
  uint64_t wanted = p.blocks ? (uint64_t(kBsmTargetGroups) + p.blocks - 1) / p.blocks : 1;
  if (wanted > uint64_t(kBsmMaxChunks)) wanted = uint64_t(kBsmMaxChunks);
  if (wanted > p.tiles) wanted = p.tiles;
  if (wanted < 1) wanted = 1;
  p.tiles_per_chunk = uint32_t((p.tiles + wanted - 1) / wanted);
  if (p.tiles_per_chunk < 1) p.tiles_per_chunk = 1;
  p.chunks = p.tiles ? (p.tiles + p.tiles_per_chunk - 1) / p.tiles_per_chunk : 1;
  uint64_t o = 0;
  auto take = [&o](uint64_t floats) {
    const uint64_t at = o;
    o += bsm_up(4 * floats, 256);
    return at;
  };
  const uint64_t rows = p.bp, mat = p.bp * uint64_t(p.kp);
  p.off_inv_q = take(rows);
  p.off_inv_i = take(rows);
  p.off_ss_q = take(rows);
  p.off_ss_i = take(rows);
  p.off_c = take(rows);
  p.off_zd = take(rows);
  p.off_qs = take(mat);
  p.off_is = take(mat);
  p.off_ml_m = take(p.chunks * rows);
  p.off_ml_l = take(p.chunks * rows);
  p.off_lse = take(rows);
  p.off_dq_part = take(p.chunks * mat);
  p.off_di_part = take(p.chunks * mat);
  p.bytes = o;
  return p;
}

// ---- the launch counters: mhte_batch_softmax_launch_counts' index ---------------------------------------------
enum BsmCounter : int {
  kBsmCntPrep = 0,       // bsm_prep_kernel
  kBsmCntRowFwd = 1,     // bsm_row_kernel, forward: the (m, l) partials
  kBsmCntRowGrad = 2,    // bsm_row_kernel, gradient form: the partials of G . I^
  kBsmCntCol = 3,        // bsm_col_kernel: the partials of G^T . Q^
  kBsmCntFinalLse = 4,   // bsm_final_kernel: lse and, when asked for, the loss
  kBsmCntFinalGrad = 5,  // bsm_final_grad_kernel: dquery and / or ditem
  kBsmCounters = 6
};
// launches of one call: loss alone 3 (prep, row, final); with gradients 4 + one sweep per gradient asked for
// (prep, row, final, [row gradient], [col], final gradient): 6 with both.  The grad entry launches the same.

}  // namespace mhte
#endif  // MHTE_BSM_CORE_H_
