// Dense optimizers, the arithmetic contract and which variables enter the chunk table: one source for host and
// device.
// Reference: ResourceApplyAdamom (CPU only) and ResourceApplyRmsprop (V1 / V2, CPU and GPU),
// native_training/optimizers/{adamom,rmsprop}.py, optimizers/cc/training_ops.cc and
// optimizers/cc/kernels/training_ops{.h,.cc,_gpu.cu.cc} — the expression trees are those of
// kernels/training_ops.cc:34-121.
//
// The reference does not pin the bits: its CPU build goes through Eigen's packet rsqrt, its GPU build through
// rsqrtf with nvcc free to contract products into FMAs.  Here every operation is ONE fp32 operation rounded on
// its own, no FMA; sqrt and / are the correctly rounded ones and rsqrt(x) := 1.0f / sqrt(x).  g0 is the
// gradient element as it lies in memory (fp32, or fp16 converted exactly):
//   grad = g0 * grad_scale                        (always one rounded product, also for a scale of 1)
//   g    = (wd * var) + grad
//   Adamom (slots m, v, c):  if update_slots:  m = (mom * m) + ((1 - mom) * g)
//                                              v = (ada * v) + (g * g)
//                                              c = (ada * c) + 1
//                            v1:  var = var - ((m * lr) * rsqrt((v / c) + eps))
//                            v2:  var = var - ((m * lr) / (sqrt(v / c) + eps))
//   RMSprop (slots m, v):    v1:  v = v + (((g * g) - v) * (1 - beta2))
//                                 m = (beta1 * m) + ((g * lr) * rsqrt(v + eps))
//                            v2:  v = (beta2 * v) + (g * g)
//                                 m = (beta1 * m) + ((g * lr) / (sqrt(v) + eps))
//                            var = var - m
// Adamom without update_slots still moves var (with fresh slots that is 0 / 0: NaN, no guard); RMSprop without
// update_slots changes nothing and the host launches nothing.  tests/dense_opt_truth.py restates all of it.
//
// This is NOT the sparse per-row kOptRmsprop of mhte_core.h (hash_table/optimizer/rmsprop_optimizer.cc: double
// arithmetic, one accumulator): the two stay apart.
//
// Compiled by hipcc inside mhte.hip and, for the CPU suite (tests/dense_opt_host_driver.cc), by g++ with
// MHTE_HOST_ONLY defined.
#ifndef MHTE_DENSE_OPT_CORE_H_
#define MHTE_DENSE_OPT_CORE_H_

#include "mhte_chunk_table.h"   // (MHTE_HD, and hip_runtime.h unless MHTE_HOST_ONLY)

#if defined(MHTE_HOST_ONLY)
#include <math.h>
#endif

namespace mhte {

// one rounded product / sum (the build passes -ffp-contract=off; on the device the intrinsics say it again)
MHTE_HD float dense_mul(float a, float b) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __fmul_rn(a, b);
#else
  return a * b;
#endif
}
MHTE_HD float dense_add(float a, float b) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __fadd_rn(a, b);
#else
  return a + b;
#endif
}
MHTE_HD float dense_sub(float a, float b) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __fsub_rn(a, b);
#else
  return a - b;
#endif
}
MHTE_HD float dense_rsqrt(float x) { return 1.0f / sqrtf(x); }

// The hyper-parameters of a call.  a, b: Adamom's (ada_decay, mom_decay), RMSprop's (beta1, beta2).
struct DenseOptHyper {
  float grad_scale, lr, a, b, eps, wd;
};

MHTE_HD float dense_grad_after_decay(float var, float g0, const DenseOptHyper& h) {
  const float grad = dense_mul(g0, h.grad_scale);
  return dense_add(dense_mul(h.wd, var), grad);
}

MHTE_HD void dense_adamom_step(float& var, float& m, float& v, float& c, float g0, const DenseOptHyper& h,
                               bool update_slots, bool v2) {
  const float g = dense_grad_after_decay(var, g0, h);
  if (update_slots) {
    m = dense_add(dense_mul(h.b, m), dense_mul(dense_sub(1.0f, h.b), g));
    v = dense_add(dense_mul(h.a, v), dense_mul(g, g));
    c = dense_add(dense_mul(h.a, c), 1.0f);
  }
  const float ml = dense_mul(m, h.lr);
  const float q = v / c;
  const float step = v2 ? ml / dense_add(sqrtf(q), h.eps) : dense_mul(ml, dense_rsqrt(dense_add(q, h.eps)));
  var = dense_sub(var, step);
}

// (update_slots == false is the host's business: nothing is launched)
MHTE_HD void dense_rmsprop_step(float& var, float& m, float& v, float g0, const DenseOptHyper& h, bool v2) {
  const float g = dense_grad_after_decay(var, g0, h);
  const float gl = dense_mul(g, h.lr);
  float step;
  if (v2) {
    v = dense_add(dense_mul(h.b, v), dense_mul(g, g));
    step = gl / dense_add(sqrtf(v), h.eps);
  } else {
    v = dense_add(v, dense_mul(dense_sub(dense_mul(g, g), v), dense_sub(1.0f, h.b)));
    step = dense_mul(gl, dense_rsqrt(dense_add(v, h.eps)));
  }
  m = dense_add(dense_mul(h.a, m), step);
  var = dense_sub(var, m);
}

// ---- the chunk table ----------------------------------------------------------------------------------
constexpr int kDenseOptInline = 96;   // variables in the kernel arguments; beyond: the table is uploaded

// Variable i owns [off[i], off[i] + len[i]) of every slot buffer (and of a flat gradient buffer), off[i] =
// the sum of round_up(len[j], A) over j < i — the rule of mhte_aligned_flat_offsets, over ALL variables of
// the optimizer.  A variable takes part in a call when it is not empty and, with the list source, has a
// gradient; the ones that take part enter the chunk table (mhte_chunk_table.h) in list order, each with the
// pointers (var, gradient — NULL with a flat source: the gradient lies at off in the flat buffer).
// grads == NULL: the flat source.  -> false when the call has 2^31 or more chunks (the table is then
// incomplete).  The caller has checked n, lens and align_elems.
template <class TABLE>
inline bool dense_opt_table(float* const* vars, const float* const* grads, const int64_t* lens, int32_t n,
                            int32_t align_elems, TABLE& T) {
  const long long mask = (long long)(align_elems) - 1;
  long long off = 0;
  for (int32_t i = 0; i < n; ++i) {
    const long long len = lens[i];
    if (len != 0 && (!grads || grads[i])) {
      const void* const p[2] = {vars[i], grads ? grads[i] : nullptr};
      if (!T.add(p, len, off)) return false;
    }
    off += (len + mask) & ~mask;
  }
  return true;
}

// The same table as a list of entries, for a caller that wants to look at it (tests/dense_opt_host_driver.cc).
struct DenseOptEntry {
  float* var;
  const float* grad;   // NULL with a flat source
  long long len, off;
  uint32_t chunk0;
};
inline bool dense_opt_table(float* const* vars, const float* const* grads, const int64_t* lens, int32_t n,
                            int32_t align_elems, std::vector<DenseOptEntry>& entries, uint32_t* n_chunks) {
  ChunkTable<ChunkArgs<kDenseOptInline, 2, true>> T;
  entries.clear();
  if (!dense_opt_table(vars, grads, lens, n, align_elems, T)) return false;
  for (uint32_t i = 0; i < T.A.k.n_tensors; ++i)
    entries.push_back(DenseOptEntry{static_cast<float*>(T.ptr_at(0, i)), static_cast<const float*>(T.ptr_at(1, i)),
                                    T.num_at(0, i), T.num_at(1, i), T.chunk0_at(i)});
  *n_chunks = T.A.k.n_chunks;
  return true;
}

}  // namespace mhte
#endif  // MHTE_DENSE_OPT_CORE_H_
