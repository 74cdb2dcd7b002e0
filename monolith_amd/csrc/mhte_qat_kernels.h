// Quantization-aware training: the segment retrievers of a TRAINING table.  Included by
// mhte_kernels.h only.
//
// The reference's EntryAccessor reads a row through a retriever picked per segment from the
// segment's comp_config (entry_accessor.cc:283-302): fixed_r8 -> FakeQuantRetriever (lookups return
// the int8-quantized weight), one_bit -> HashNetRetriever (lookups return amplitude * tanh(scale * w),
// the update first scales the gradient by the derivative), anything else -> the raw retriever.  Rows
// stay fp32 in HBM: the transforms run in registers between the row load and the store (lookups) and
// between the gradient load and the optimizer (updates).  Save / LookupEntry / dump read the stored
// weights (GetNum, entry_accessor.cc:225-232) and never come here.
#ifndef MHTE_QAT_KERNELS_H_
#define MHTE_QAT_KERNELS_H_

#include "mhte_core.h"

namespace mhte {

// (the values of MHTE_RETRIEVER_* in the public header)
enum RetrieverType : int32_t { kRetRaw = 0, kRetFakeQuant = 1, kRetHashNet = 2 };

// The kernel instance a table's retrievers select (template parameter RT): the one-segment forms
// know their transform at compile time, kRtMixed selects per column from the uniform descriptors.
// kRtRaw is every instance that existed before the retrievers did: no descriptor argument, the
// same code.
enum RetrieverInstance : int { kRtRaw = 0, kRtFakeQuant = 1, kRtHashNet = 2, kRtMixed = 3 };

// The retriever descriptors of one table, a kernel argument of its own of the retriever instances
// (SegDesc / TableView, which every hot kernel takes by value, do not grow).
struct RetrieverArgs {
  uint32_t nseg;
  uint32_t update;                // bit k: this call's Backward moves segment k's scale to cand[k]
  int32_t type[kMaxSegments];     // RetrieverType
  uint32_t w_off[kMaxSegments];   // first column of the segment (SegDesc::w_off)
  float p0[kMaxSegments];         // fake quant: step = r / 128        hash net: amplitude
  float p1[kMaxSegments];         // fake quant: half_step = step / 2
  float cand[kMaxSegments];       // hash net: the scale of this call's global_step (host: powf)
  float* scale;                   // hash net: [kMaxSegments] live scales in device memory
};

// FakeQuantizer::Quantize (compressor/fake_quantizer.h:26-70): round to the nearest of 256 slots
// of width r / 128, through an integer — a negative input that rounds to slot 0 gives +0.0 as
// (float)(int) does, where truncf would give -0.0.  The division is the correctly rounded one
// (no reciprocal multiply: a quotient that is exactly integral must stay so).  The reference
// converts an out-of-range quotient (|f| beyond 2^31 steps, +-inf) to int, which is undefined
// there; here it saturates by sign: +127 * step, -128 * step.  NaN -> 0.
__device__ __forceinline__ float fake_quant(float f, float step, float half_step) {
  if (f != f) return 0.f;
  f = (f >= 0.f) ? f + half_step : f - half_step;
  const float q = f / step;
  const int nstep = static_cast<int>(fminf(fmaxf(q, -128.f), 127.f));
  return static_cast<float>(nstep) * step;
}

// HashNetQuantizer::Forward (compressor/hash_net_quantizer.h:42-44)
__device__ __forceinline__ float hash_net_forward(float w, float scale, float amplitude) {
  return amplitude * tanhf(scale * w);
}
// HashNetQuantizer::Backward (:46-58) behind its scale update: the factor of the gradient at the
// stored weight w
__device__ __forceinline__ float hash_net_backward(float w, float g, float scale, float amplitude) {
  const float y = tanhf(scale * w);
  return g * (amplitude * scale * (1.f - y * y));
}

// the descriptor of column `col` of a multi-segment row: a chain of selects over the (uniform)
// descriptors, no indexed read of the kernel arguments
struct RetrieverCol {
  int32_t type;
  uint32_t k;
  float p0, p1;
};
__device__ __forceinline__ RetrieverCol retriever_of(const RetrieverArgs& ra, uint32_t col) {
  RetrieverCol c{ra.type[0], 0u, ra.p0[0], ra.p1[0]};
#pragma unroll
  for (uint32_t k = 1; k < uint32_t(kMaxSegments); ++k) {
    const bool in = k < ra.nseg && col >= ra.w_off[k];
    c.type = in ? ra.type[k] : c.type;
    c.k = in ? k : c.k;
    c.p0 = in ? ra.p0[k] : c.p0;
    c.p1 = in ? ra.p1[k] : c.p1;
  }
  return c;
}

// The scale a Backward of this call uses for segment k: the call's candidate where the call moves
// the scale (every lane that stores it stores the same value, and nobody reads the device word in
// such a launch), the live device value otherwise.
__device__ __forceinline__ float hash_net_scale_bwd(const RetrieverArgs& ra, uint32_t k, float cand) {
  return ((ra.update >> k) & 1u) ? cand : ra.scale[k];
}

// Retrieve on the VEC weights a lane holds of a resident row, columns e .. e + VEC - 1
// (RetrieverInterface::Retrieve, entry_accessor.cc:169-171)
template <int RT, int VEC>
__device__ __forceinline__ void retrieve_lane(float (&v)[VEC], uint32_t e, const RetrieverArgs& ra) {
  if constexpr (RT == kRtFakeQuant) {
#pragma unroll
    for (int c = 0; c < VEC; ++c) v[c] = fake_quant(v[c], ra.p0[0], ra.p1[0]);
  } else if constexpr (RT == kRtHashNet) {
    const float scale = ra.scale[0];
#pragma unroll
    for (int c = 0; c < VEC; ++c) v[c] = hash_net_forward(v[c], scale, ra.p0[0]);
  } else if constexpr (RT == kRtMixed) {
#pragma unroll
    for (int c = 0; c < VEC; ++c) {
      const RetrieverCol d = retriever_of(ra, e + uint32_t(c));
      if (d.type == kRetFakeQuant) v[c] = fake_quant(v[c], d.p0, d.p1);
      else if (d.type == kRetHashNet) v[c] = hash_net_forward(v[c], ra.scale[d.k], d.p0);
    }
  }
}

// Backward on the VEC gradients g a lane is about to hand to the optimizer, at the weights w it
// holds in registers (RetrieverInterface::Backward, entry_accessor.cc:187-195; the fake-quant
// retriever's is a no-op, retriever/fake_quant_retriever.cc:38-39).  The caller's gradient buffer is
// not written (the reference scales it in place through a const_cast).
template <int RT, int VEC>
__device__ __forceinline__ void backward_lane(float (&g)[VEC], const float (&w)[VEC], uint32_t e,
                                              const RetrieverArgs& ra) {
  if constexpr (RT == kRtHashNet) {
    const float scale = hash_net_scale_bwd(ra, 0u, ra.cand[0]);
#pragma unroll
    for (int c = 0; c < VEC; ++c) g[c] = hash_net_backward(w[c], g[c], scale, ra.p0[0]);
  } else if constexpr (RT == kRtMixed) {
#pragma unroll
    for (int c = 0; c < VEC; ++c) {
      const RetrieverCol d = retriever_of(ra, e + uint32_t(c));
      if (d.type == kRetHashNet) {
        float cand = ra.cand[0];
#pragma unroll
        for (uint32_t k = 1; k < uint32_t(kMaxSegments); ++k) cand = (d.k == k) ? ra.cand[k] : cand;
        g[c] = hash_net_backward(w[c], g[c], hash_net_scale_bwd(ra, d.k, cand), d.p0);
      }
    }
  }
}

// The scale update of HashNetQuantizer::Backward (:47-54), by ONE lane of a lane group whose id
// reached the optimizer: a call in which no id does leaves the scale alone.  A vector store.
__device__ __forceinline__ void hash_net_store_scales(const RetrieverArgs& ra) {
#pragma unroll
  for (uint32_t k = 0; k < uint32_t(kMaxSegments); ++k)
    if (k < ra.nseg && ((ra.update >> k) & 1u)) ra.scale[k] = ra.cand[k];
}

}  // namespace mhte
#endif  // MHTE_QAT_KERNELS_H_
