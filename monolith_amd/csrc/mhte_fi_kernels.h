// The kernels of FeatureInsight (mhte_fi_core.h has the formulas, the fp32 definition and the plan).
//
// Every product of the op is a 64 x 64 output tile of C = A . B with its own chain length R, computed by one
// workgroup of 256 threads on the vector ALU: thread (ty, tx) = (tid / 16, tid % 16) owns the rows ty, ty + 16,
// ty + 32, ty + 48 and the columns tx, tx + 16, tx + 32, tx + 48 of the tile (a row of 16 lanes stores 16
// consecutive floats: the stores are coalesced whatever the alignment of the operands, which are only 4-byte
// aligned), and walks the chain in LDS stages of kFiStage terms, one fmaf per term and output, t ascending: the chain
// of the definition, whatever the tiling; the next stage's loads are issued into registers before this stage is
// multiplied.  (Skipping the groups of 16 rows or columns that a short segment leaves empty was measured: the
// branches in the inner loop cost every tile more than they saved.)  Workgroups are numbered with the SEGMENT
// fastest: those in flight together touch adjacent 256-byte pieces of the same rows of out / grad.  What differs
// between the three products is where A and B come from:
//   forward       A = input[b, o + t]       B = weight[o + t, k]        R = s_f     C -> out[b, f K + k]
//   input grad    A = grad[b, f K + t]      B = weight[o + j, t]        R = K       C -> input_grad[b, o + j]
//   weight grad   A = input[b0 + t, o + j]  B = grad[b0 + t, f K + k]   R = slab    C -> weight_grad or its partial
// The aggregate form of the forward keeps a row block of one feature, walks all column tiles, squares into four
// registers per thread (lane tx's chain of the definition) and adds the 16 lanes of a row in lane order: no
// intermediate, no workspace.
// The segment offsets of a launch ride in its arguments (FiSegs); a longer list is more launches.
#ifndef MHTE_FI_KERNELS_H_
#define MHTE_FI_KERNELS_H_

#include "mhte_fi_core.h"

namespace mhte {

constexpr int kFiThreads = 256;
constexpr int kFiAPad = kFiStage + 1;   // LDS row strides: both tiles are written and read without bank conflicts
constexpr int kFiBPad = kFiTile + 1;

struct FiSegs {
  int32_t n;                     // segments of this launch
  int32_t first;                 // the index of its first segment in the whole list
  int32_t off[kFiInline + 1];    // their first columns, and the end of the last
};

struct FiArgs {
  const float* input;    // [B, E]
  const float* weight;   // [E, K]
  const float* grad;     // [B, F K] (gradient kernels)
  float* dst;            // out, agg, input_grad, or weight_grad / the slab partials
  long long B, E, K, FK, F;
  long long slab_rows, slabs;
  FiSegs segs;
};

// One tile: acc[i][c] += sum_t A(ty + 16 i, t) * B(t, tx + 16 c), t ascending.  A(m, t) = Ap[m a_sm + t a_sr] for
// m < Mv, B(t, n) = Bp[t b_sr + n b_sn] for n < Nv; rows and columns beyond are zeros that are never stored.
// A_TFAST / B_NFAST: the index that is contiguous in memory, which the loader's lanes follow.
template <bool A_TFAST, bool B_NFAST>
__device__ __forceinline__ void fi_tile(float (&acc)[4][4], const float* __restrict__ Ap, long long a_sm,
                                        long long a_sr, const float* __restrict__ Bp, long long b_sr, long long b_sn,
                                        int Mv, int Nv, long long R, float (*As)[kFiAPad], float (*Bs)[kFiBPad]) {
  constexpr int kSlots = kFiTile * kFiStage / kFiThreads;   // elements of each operand a thread moves per stage
  const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
  float ra[kSlots], rb[kSlots];
  // the stage that starts at term t0, from memory into registers (zeros beyond the valid rows, columns and terms)
  auto fetch = [&](long long t0) {
    const int tv = int(R - t0 < kFiStage ? R - t0 : kFiStage);
#pragma unroll
    for (int q = 0; q < kSlots; ++q) {
      const int idx = tid + kFiThreads * q;
      const int ta = A_TFAST ? (idx & (kFiStage - 1)) : (idx >> 6), m = A_TFAST ? (idx >> 5) : (idx & (kFiTile - 1));
      ra[q] = (m < Mv && ta < tv) ? Ap[m * a_sm + (t0 + ta) * a_sr] : 0.f;
      const int tb = B_NFAST ? (idx >> 6) : (idx & (kFiStage - 1)), n = B_NFAST ? (idx & (kFiTile - 1)) : (idx >> 5);
      rb[q] = (n < Nv && tb < tv) ? Bp[(t0 + tb) * b_sr + n * b_sn] : 0.f;
    }
  };
  if (R > 0) fetch(0);
  for (long long t0 = 0; t0 < R; t0 += kFiStage) {
    const int tv = int(R - t0 < kFiStage ? R - t0 : kFiStage);
#pragma unroll
    for (int q = 0; q < kSlots; ++q) {
      const int idx = tid + kFiThreads * q;
      As[A_TFAST ? (idx >> 5) : (idx & (kFiTile - 1))][A_TFAST ? (idx & (kFiStage - 1)) : (idx >> 6)] = ra[q];
      Bs[B_NFAST ? (idx >> 6) : (idx & (kFiStage - 1))][B_NFAST ? (idx & (kFiTile - 1)) : (idx >> 5)] = rb[q];
    }
    __syncthreads();
    if (t0 + kFiStage < R) fetch(t0 + kFiStage);   // the next stage's loads fly while this one is multiplied
#pragma unroll 4
    for (int t = 0; t < tv; ++t) {
      float a[4], b[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) a[i] = As[ty + 16 * i][t];
#pragma unroll
      for (int c = 0; c < 4; ++c) b[c] = Bs[t][tx + 16 * c];
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int c = 0; c < 4; ++c) acc[i][c] = fi_fma(a[i], b[c], acc[i][c]);
    }
    __syncthreads();
  }
}

__device__ __forceinline__ void fi_clear(float (&acc)[4][4]) {
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int c = 0; c < 4; ++c) acc[i][c] = 0.f;
}
// rows m < Mv, columns n < Nv of the tile to Cp[m c_sm + n]
__device__ __forceinline__ void fi_store(const float (&acc)[4][4], float* __restrict__ Cp, long long c_sm, int Mv,
                                         int Nv) {
  const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int m = ty + 16 * i;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const int n = tx + 16 * c;
      if (m < Mv && n < Nv) Cp[m * c_sm + n] = acc[i][c];
    }
  }
}

// grid: (row blocks * segments of the launch [segment fastest], 1, column tiles [plain] or 1 [aggregate])
template <bool AGG>
__global__ __launch_bounds__(kFiThreads) void fi_forward_kernel(const FiArgs a) {
  __shared__ float As[kFiTile][kFiAPad];
  __shared__ float Bs[kFiStage][kFiBPad];
  const unsigned seg = blockIdx.x % unsigned(a.segs.n);
  const long long o = a.segs.off[seg], s = a.segs.off[seg + 1] - o;
  const long long f = a.segs.first + (long long)seg;
  const long long r0 = (long long)(blockIdx.x / unsigned(a.segs.n)) * kFiTile;
  const int Mv = int(a.B - r0 < kFiTile ? a.B - r0 : kFiTile);
  const float* Ap = a.input + r0 * a.E + o;
  float acc[4][4];
  if (!AGG) {
    const long long k0 = (long long)blockIdx.z * kFiTile;
    const int Nv = int(a.K - k0 < kFiTile ? a.K - k0 : kFiTile);
    fi_clear(acc);
    fi_tile<true, true>(acc, Ap, a.E, 1, a.weight + o * a.K + k0, a.K, 1, Mv, Nv, s, As, Bs);
    fi_store(acc, a.dst + r0 * a.FK + f * a.K + k0, a.FK, Mv, Nv);
  } else {
    __shared__ float red[kFiTile][kFiLanes + 1];
    float sq[4] = {0.f, 0.f, 0.f, 0.f};
    for (long long k0 = 0; k0 < a.K; k0 += kFiTile) {
      const int Nv = int(a.K - k0 < kFiTile ? a.K - k0 : kFiTile);
      fi_clear(acc);
      fi_tile<true, true>(acc, Ap, a.E, 1, a.weight + o * a.K + k0, a.K, 1, Mv, Nv, s, As, Bs);
      // (a column beyond K holds +0 and fmaf(0, 0, p) = p: the padding is not part of the chain)
#pragma unroll
      for (int c = 0; c < 4; ++c)
#pragma unroll
        for (int i = 0; i < 4; ++i) sq[i] = fi_fma(acc[i][c], acc[i][c], sq[i]);
    }
    const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
#pragma unroll
    for (int i = 0; i < 4; ++i) red[ty + 16 * i][tx] = sq[i];
    __syncthreads();
    if (int(threadIdx.x) < Mv) {
      float t = red[threadIdx.x][0];
#pragma unroll
      for (int l = 1; l < kFiLanes; ++l) t += red[threadIdx.x][l];
      a.dst[(r0 + threadIdx.x) * a.F + f] = t;
    }
  }
}

// grid: (row blocks * segments of the launch [segment fastest], 1, tiles of 64 columns of the longest segment)
__global__ __launch_bounds__(kFiThreads) void fi_input_grad_kernel(const FiArgs a) {
  __shared__ float As[kFiTile][kFiAPad];
  __shared__ float Bs[kFiStage][kFiBPad];
  const unsigned seg = blockIdx.x % unsigned(a.segs.n);
  const long long o = a.segs.off[seg], s = a.segs.off[seg + 1] - o;
  const long long n0 = (long long)blockIdx.z * kFiTile;
  if (n0 >= s) return;   // the whole workgroup: a shorter segment than the launch's longest
  const long long f = a.segs.first + (long long)seg;
  const long long r0 = (long long)(blockIdx.x / unsigned(a.segs.n)) * kFiTile;
  const int Mv = int(a.B - r0 < kFiTile ? a.B - r0 : kFiTile);
  const int Nv = int(s - n0 < kFiTile ? s - n0 : kFiTile);
  float acc[4][4];
  fi_clear(acc);
  fi_tile<true, false>(acc, a.grad + r0 * a.FK + f * a.K, a.FK, 1, a.weight + (o + n0) * a.K, 1, a.K, Mv, Nv, a.K,
                       As, Bs);
  fi_store(acc, a.dst + r0 * a.E + o + n0, a.E, Mv, Nv);
}

// grid: (slabs * column tiles * segments of the launch [segment fastest], 1, tiles of 64 rows of the longest segment)
__global__ __launch_bounds__(kFiThreads) void fi_weight_grad_kernel(const FiArgs a) {
  __shared__ float As[kFiTile][kFiAPad];
  __shared__ float Bs[kFiStage][kFiBPad];
  const unsigned seg = blockIdx.x % unsigned(a.segs.n), rest = blockIdx.x / unsigned(a.segs.n);
  const long long o = a.segs.off[seg], s = a.segs.off[seg + 1] - o;
  const long long m0 = (long long)blockIdx.z * kFiTile;
  if (m0 >= s) return;
  const long long f = a.segs.first + (long long)seg;
  const long long ktiles = (a.K + kFiTile - 1) / kFiTile;
  const long long slab = (long long)rest / ktiles, k0 = ((long long)rest % ktiles) * kFiTile;
  const long long b0 = slab * a.slab_rows;
  const long long R = a.B - b0 < a.slab_rows ? a.B - b0 : a.slab_rows;
  const int Mv = int(s - m0 < kFiTile ? s - m0 : kFiTile);
  const int Nv = int(a.K - k0 < kFiTile ? a.K - k0 : kFiTile);
  float acc[4][4];
  fi_clear(acc);
  fi_tile<false, true>(acc, a.input + b0 * a.E + o + m0, 1, a.E, a.grad + b0 * a.FK + f * a.K + k0, a.FK, 1, Mv, Nv,
                       R, As, Bs);
  float* dst = a.dst + (a.slabs > 1 ? slab * a.E * a.K : 0);
  fi_store(acc, dst + (o + m0) * a.K + k0, a.K, Mv, Nv);
}

// weight_grad[i] = the partials of element i in slab order, i < n = E K
__global__ __launch_bounds__(kFiThreads) void fi_slab_sum_kernel(const float* __restrict__ part,
                                                                 float* __restrict__ weight_grad, long long n,
                                                                 int slabs) {
  for (long long i = (long long)blockIdx.x * kFiThreads + threadIdx.x; i < n; i += (long long)gridDim.x * kFiThreads)
    weight_grad[i] = fi_slab_sum(part + i, n, slabs);
}

}  // namespace mhte
#endif  // MHTE_FI_KERNELS_H_
