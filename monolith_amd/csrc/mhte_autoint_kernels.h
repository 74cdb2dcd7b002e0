// Kernels of AutoInt (mhte_autoint_core.h: the formulas, the limits, the plan, the choice of exp).
//
// A workgroup is ONE sample and has RT = row_tiles wavefronts; wavefront I owns the rows [I T, (I + 1) T) of the
// sample through all layers.  T is 16 (v_mfma_f32_16x16x4_f32) or 32 (v_mfma_f32_32x32x2_f32); a lane is
// (lr, q) = (lane % T, lane / T), Q = 64 / T lane groups, and holds NR = T T / 64 values of a tile.  The sample's
// state lives in LDS as [RT T][padded_k + 1] floats, zero in its padding rows and columns.
//
// Scores are taken transposed: S^T[J, I] = X_J X_I^T with A = X_J (lane lr = row j), B = X_I (lane lr = row i).
// The accumulator then holds in lane (i, q), register r, the score of row i against j = J T + can_kidx(r, q): a row
// of S is one lane's registers over all J plus the same registers of the other Q - 1 lane groups.  The softmax's
// max and sum are in-lane chains over the registers and one exchange between the lane groups (ai_xmax, ai_xsum);
// j >= n is left out of both.  All RT score tiles stay in registers (RT NR <= 64).
// With the reduction index of k-slot q at step s taken as j = J T + can_kidx(s, q), register s of P^T[J, I] IS step
// s of the B operand of X_{l+1}^T[:, I] += X_l^T[:, J] P^T[J, I] (A = X_l read down a column block, lane lr = c).
// The result, lane (i, q) register r = column can_kidx(r, q) of row i, goes to the other LDS state buffer; after
// the layer's barrier (wavefront-local when RT == 1) the workgroup copies it to memory in row-major runs where a
// layer's state is wanted there (out; states when a gradient follows).
//   autoint_fwd_kernel   the whole stack, x read once, out written once.
//   autoint_bwd_kernel   the layers last to first.  LDS: X_l, dO, and a third buffer that receives dX_l.
//                        Phase 1, wavefront I: the score tiles as in the forward, (m_i, 1 / sum_i) and
//                        delta_i = sum_j P_ij dP_ij of its rows, into LDS arrays.
//                        Phase 2, wavefront I alone produces dX[I, :]: per J ascending, from the score tile it kept,
//                        P_ij = exp(s - m_i) / sum_i (lane statistics) and P_ji = exp(s - m_j) / sum_j (register-row
//                        statistics, LDS broadcasts), dP_ij from X_J dO_I^T and dP_ji from dO_J X_I^T (one pass over
//                        the columns), G^T = P_ij (dP_ij - delta_i) + P_ji (dP_ji - delta_j), and
//                        dX^T[:, I] += X^T[:, J] G^T + dO^T[:, J] P_ji^T with the same register chaining.
// No atomics; plain 4-byte loads and stores; every user array is read and written below its extent only.
#ifndef MHTE_AUTOINT_KERNELS_H_
#define MHTE_AUTOINT_KERNELS_H_

#include "mhte_autoint_core.h"
#include "mhte_can_kernels.h"

namespace mhte {

struct AutoIntArgs {
  const float* x;        // [B, n, k]
  const float* dout;     // [B, n, k]
  const float* statesc;  // the gradient's states
  float* out;            // [B, n, k]
  float* states;         // [L - 1, B, n, k] or null
  float* dx;             // [B, n, k]
  int64_t B;
  int n, k, L;
};

template <int T>
__device__ __forceinline__ float ai_xmax(float v) {
  v = fmaxf(v, __shfl_xor(v, 32));
  if constexpr (T == 16) v = fmaxf(v, __shfl_xor(v, 16));
  return v;
}
// (a + b is commutative, so every lane group ends with the same bits)
template <int T>
__device__ __forceinline__ float ai_xsum(float v) {
  if constexpr (T == 16) v += __shfl_xor(v, 16);
  v += __shfl_xor(v, 32);
  return v;
}

// [n, k] of memory -> [np][xs] of LDS, zero padded to pk columns
__device__ __forceinline__ void ai_stage(float* dst, const float* src, int n, int k, int np, int pk, int xs, int tid,
                                         int nt) {
  for (int e = tid; e < np * pk; e += nt) {
    const int r = e / pk, c = e - r * pk;
    dst[r * xs + c] = r < n && c < k ? src[r * k + c] : 0.f;
  }
}

__device__ __forceinline__ void ai_store(float* dst, const float* src, int n, int k, int xs, int tid, int nt) {
  for (int e = tid; e < n * k; e += nt) {
    const int r = e / k, c = e - r * k;
    dst[e] = src[r * xs + c];
  }
}

// S[J] = S^T[J, I] for every J, then the softmax statistics of the lane's row: m and 1 / sum
template <int T, int RT>
__device__ __forceinline__ void ai_scores(const float* X, int xs, int n, int k, int I, int lr, int q,
                                          typename CanAcc<T>::type (&S)[RT], float& m, float& inv, bool normalise) {
  constexpr int NR = T * T / 64, Q = 64 / T;
#pragma unroll
  for (int J = 0; J < RT; ++J)
#pragma unroll
    for (int r = 0; r < NR; ++r) S[J][r] = 0.f;
  const float* xi = X + (I * T + lr) * xs + q;
  const int steps = (k + Q - 1) / Q;
  for (int s = 0; s < steps; ++s) {
    const float bv = xi[s * Q];
#pragma unroll
    for (int J = 0; J < RT; ++J) S[J] = can_mfma<T>(X[(J * T + lr) * xs + s * Q + q], bv, S[J]);
  }
  m = -INFINITY;
#pragma unroll
  for (int J = 0; J < RT; ++J)
#pragma unroll
    for (int r = 0; r < NR; ++r)
      if (J * T + can_kidx<T>(r, q) < n) m = fmaxf(m, S[J][r]);
  m = ai_xmax<T>(m);
  float sum = 0.f;
#pragma unroll
  for (int J = 0; J < RT; ++J)
#pragma unroll
    for (int r = 0; r < NR; ++r) {
      const float e = J * T + can_kidx<T>(r, q) < n ? __expf(S[J][r] - m) : 0.f;
      if (normalise) S[J][r] = e;
      sum += e;
    }
  inv = 1.f / ai_xsum<T>(sum);
  if (normalise) {
#pragma unroll
    for (int J = 0; J < RT; ++J)
#pragma unroll
      for (int r = 0; r < NR; ++r) S[J][r] *= inv;
  }
}

// the wavefront's rows of a new state, lane (i, q) register r of tile ct = column ct T + can_kidx(r, q), into LDS;
// padding rows become zero rows
template <int T>
__device__ __forceinline__ void ai_put(float* dst, int xs, int row, bool rok, int kt, int q,
                                       const typename CanAcc<T>::type (&acc)[64 / T]) {
  constexpr int NR = T * T / 64, KTM = 64 / T;
#pragma unroll
  for (int ct = 0; ct < KTM; ++ct)
    if (ct < kt) {
#pragma unroll
      for (int r = 0; r < NR; ++r) dst[row * xs + ct * T + can_kidx<T>(r, q)] = rok ? acc[ct][r] : 0.f;
    }
}

template <int T, int RT>
__global__ __launch_bounds__(64 * RT) void autoint_fwd_kernel(AutoIntArgs a) {
  constexpr int NR = T * T / 64, KTM = 64 / T, NT = 64 * RT, NP = RT * T;
  typedef typename CanAcc<T>::type V;
  extern __shared__ float ai_lds[];
  const int tid = threadIdx.x, I = tid / 64, lane = tid % 64, lr = lane % T, q = lane / T;
  const int n = a.n, k = a.k, kt = (k + T - 1) / T, pk = kt * T, xs = pk + 1;
  const int64_t b = blockIdx.x, nk = int64_t(n) * k;
  float* cur = ai_lds;
  float* nxt = cur + NP * xs;
  ai_stage(cur, a.x + b * nk, n, k, NP, pk, xs, tid, NT);
  __syncthreads();
  const int row = I * T + lr;
  for (int l = 0; l < a.L; ++l) {
    V P[RT];
    float m, inv;
    ai_scores<T, RT>(cur, xs, n, k, I, lr, q, P, m, inv, true);
    V acc[KTM];
#pragma unroll
    for (int ct = 0; ct < KTM; ++ct)
#pragma unroll
      for (int r = 0; r < NR; ++r) acc[ct][r] = 0.f;
#pragma unroll
    for (int J = 0; J < RT; ++J)
#pragma unroll
      for (int s = 0; s < NR; ++s) {
        const float* xj = cur + (J * T + can_kidx<T>(s, q)) * xs + lr;
#pragma unroll
        for (int ct = 0; ct < KTM; ++ct)
          if (ct < kt) acc[ct] = can_mfma<T>(xj[ct * T], P[J][s], acc[ct]);
      }
    ai_put<T>(nxt, xs, row, row < n, kt, q, acc);
    __syncthreads();   // X_{l+1} is whole; X_l is read
    if (l == a.L - 1)
      ai_store(a.out + b * nk, nxt, n, k, xs, tid, NT);
    else if (a.states)
      ai_store(a.states + (l * a.B + b) * nk, nxt, n, k, xs, tid, NT);
    float* t = cur;
    cur = nxt, nxt = t;
  }
}

template <int T, int RT>
__global__ __launch_bounds__(64 * RT) void autoint_bwd_kernel(AutoIntArgs a) {
  constexpr int NR = T * T / 64, Q = 64 / T, KTM = 64 / T, NT = 64 * RT, NP = RT * T;
  typedef typename CanAcc<T>::type V;
  extern __shared__ float ai_lds[];
  const int tid = threadIdx.x, I = tid / 64, lane = tid % 64, lr = lane % T, q = lane / T;
  const int n = a.n, k = a.k, kt = (k + T - 1) / T, pk = kt * T, xs = pk + 1;
  const int64_t b = blockIdx.x, nk = int64_t(n) * k;
  float* Xs = ai_lds;
  float* Dc = Xs + NP * xs;   // dO
  float* Dn = Dc + NP * xs;   // dX
  float* Ms = Xs + 3 * NP * xs;
  float* Is = Ms + NP;
  float* Es = Is + NP;        // delta
  ai_stage(Dc, a.dout + b * nk, n, k, NP, pk, xs, tid, NT);
  const int row = I * T + lr;
  const int steps = (k + Q - 1) / Q;
  for (int l = a.L - 1; l >= 0; --l) {
    const float* xg = l == 0 ? a.x + b * nk : a.statesc + ((l - 1) * a.B + b) * nk;
    ai_stage(Xs, xg, n, k, NP, pk, xs, tid, NT);
    __syncthreads();
    // phase 1: the statistics of the wavefront's rows
    V S[RT];
    float mi, invi;
    ai_scores<T, RT>(Xs, xs, n, k, I, lr, q, S, mi, invi, false);
    float di = 0.f;   // delta_i = sum_j P_ij dP_ij
#pragma unroll
    for (int J = 0; J < RT; ++J) {
      V pa;
#pragma unroll
      for (int r = 0; r < NR; ++r) pa[r] = 0.f;
      for (int s = 0; s < steps; ++s) {
        const int c = s * Q + q;
        pa = can_mfma<T>(Xs[(J * T + lr) * xs + c], Dc[row * xs + c], pa);
      }
#pragma unroll
      for (int r = 0; r < NR; ++r)
        if (J * T + can_kidx<T>(r, q) < n) di += __expf(S[J][r] - mi) * invi * pa[r];
    }
    di = ai_xsum<T>(di);
    if (q == 0) Ms[row] = mi, Is[row] = invi, Es[row] = di;
    __syncthreads();   // every row's statistics are there
    // phase 2: dX[I, :]
    V acc[KTM];
#pragma unroll
    for (int ct = 0; ct < KTM; ++ct)
#pragma unroll
      for (int r = 0; r < NR; ++r) acc[ct][r] = 0.f;
#pragma unroll
    for (int J = 0; J < RT; ++J) {
      V pa, pb;   // dP_ij = X_j . dO_i and dP_ji = dO_j . X_i at (j, i)
#pragma unroll
      for (int r = 0; r < NR; ++r) pa[r] = 0.f, pb[r] = 0.f;
      for (int s = 0; s < steps; ++s) {
        const int c = s * Q + q;
        pa = can_mfma<T>(Xs[(J * T + lr) * xs + c], Dc[row * xs + c], pa);
        pb = can_mfma<T>(Dc[(J * T + lr) * xs + c], Xs[row * xs + c], pb);
      }
#pragma unroll
      for (int r = 0; r < NR; ++r) {
        const int j = J * T + can_kidx<T>(r, q);
        const bool jok = j < n;
        const float s = S[J][r];
        const float pij = jok ? __expf(s - mi) * invi : 0.f;
        const float pji = jok ? __expf(s - Ms[j]) * Is[j] : 0.f;
        pa[r] = pij * (pa[r] - di) + pji * (pb[r] - Es[j]);   // G^T[j, i]
        pb[r] = pji;
      }
#pragma unroll
      for (int s = 0; s < NR; ++s) {
        const int o = (J * T + can_kidx<T>(s, q)) * xs + lr;
#pragma unroll
        for (int ct = 0; ct < KTM; ++ct)
          if (ct < kt) {
            acc[ct] = can_mfma<T>(Xs[o + ct * T], pa[s], acc[ct]);
            acc[ct] = can_mfma<T>(Dc[o + ct * T], pb[s], acc[ct]);
          }
      }
    }
    ai_put<T>(Dn, xs, row, row < n, kt, q, acc);
    __syncthreads();   // dX_l is whole; X_l and dO are read
    if (l == 0) ai_store(a.dx + b * nk, Dn, n, k, xs, tid, NT);
    float* t = Dc;
    Dc = Dn, Dn = t;
  }
}

}  // namespace mhte
#endif  // MHTE_AUTOINT_KERNELS_H_
