// The chunk table: how a kernel walks a LIST of tensors as one range of equal pieces.  Shared by clip by global
// norm (mhte_clip_kernels.h), the aligned flat concat (mhte_flat_kernels.h) and the dense optimizers
// (mhte_dense_opt_kernels.h); what a chunk MEANS — which elements are loaded, what is stored — stays with them.
//   * the tensors that take part in a call (the caller decides which) are cut into chunks of 4096 elements,
//     the last one of a tensor short, numbered in list order c = 0 .. n_chunks - 1; a chunk never straddles
//     two tensors;
//   * per tensor the table holds one or two pointers, the length, an offset where the op has one, and the
//     tensor's first chunk, chunk0[] ascending: tensor i's chunks are chunk0[i] .. chunk0[i + 1] - 1;
//   * a list of up to N tensors rides in the kernel arguments (no allocation, no copy); a longer one is kept
//     whole in host vectors, packed into one block and uploaded, and the kernel's EXT instance reads the same
//     columns from device memory;
//   * on the device a chunk's tensor is found by binary search over chunk0[]; a workgroup that takes chunks by
//     grid stride carries a cursor that only moves forward (chunk_advance), so the next chunk's place is known,
//     and its loads in flight, while this chunk is worked on.
// Compiled by hipcc inside mhte.hip and, for the CPU suite (tests/chunk_table_host_driver.cc,
// tests/dense_opt_host_driver.cc), by g++ with MHTE_HOST_ONLY defined: the driver runs the very functions the
// kernels call.
#ifndef MHTE_CHUNK_TABLE_H_
#define MHTE_CHUNK_TABLE_H_

#include <stdint.h>
#include <string.h>

#include <vector>

#if defined(MHTE_HOST_ONLY)
#ifndef MHTE_HD
#define MHTE_HD
#endif
#ifndef MHTE_GLOBAL
#define MHTE_GLOBAL
#endif
#else
#include <hip/hip_runtime.h>
#ifndef MHTE_HD
#define MHTE_HD __host__ __device__ __forceinline__
#endif
#ifndef MHTE_GLOBAL
#define MHTE_GLOBAL __attribute__((address_space(1)))
#endif
#endif

namespace mhte {

constexpr int kChunkElems = 4096;   // elements per chunk

// the words between the EXT pointers and the columns; an op that carries a word of its own derives from it
struct ChunkCounts {
  uint32_t n_tensors, n_chunks;
};

// The kernel-argument block.  N: tensors that fit inline; NPTR: pointer columns (1 or 2); OFF: an offset column
// beside the lengths.  Every column exists twice: inline, and (EXT) as a pointer to the same array in device
// memory.  An op's own struct derives from its instance (the kernels keep their argument types' names).
template <int N, int NPTR, bool OFF, class COUNTS = ChunkCounts>
struct ChunkArgs {
  static_assert(NPTR == 1 || NPTR == 2, "one or two pointer columns");
  static constexpr int kInline = N, kPtrs = NPTR, kNums = OFF ? 2 : 1;
  static constexpr size_t kEntryBytes = 8 * (kPtrs + kNums) + 4;   // of the uploaded block, per tensor
  void* const* x_ptr[NPTR];       // EXT
  const long long* x_num[kNums];
  const uint32_t* x_chunk0;
  COUNTS k;
  void* ptr[NPTR][N];
  long long num[kNums][N];        // the lengths, then the offsets
  uint32_t chunk0[N];
};

// ---- reading a column, on the device and on the host ---------------------------------------------------
template <bool EXT, class A>
MHTE_HD uint32_t tensor_chunk0(const A& a, uint32_t i) {
  return EXT ? ((const MHTE_GLOBAL uint32_t*)(a.x_chunk0))[i] : a.chunk0[i];
}
template <bool EXT, class T, class A>
MHTE_HD T* chunk_ptr(const A& a, int col, uint32_t i) {
  typedef void* any_ptr;
  return static_cast<T*>(EXT ? ((const MHTE_GLOBAL any_ptr*)(a.x_ptr[col]))[i] : a.ptr[col][i]);
}
template <bool EXT, class A>
MHTE_HD long long chunk_num(const A& a, int col, uint32_t i) {
  return EXT ? ((const MHTE_GLOBAL long long*)(a.x_num[col]))[i] : a.num[col][i];
}
template <bool EXT, class A>
MHTE_HD long long chunk_len(const A& a, uint32_t i) { return chunk_num<EXT>(a, 0, i); }
template <bool EXT, class A>
MHTE_HD long long chunk_off(const A& a, uint32_t i) { return chunk_num<EXT>(a, 1, i); }

// the tensor that holds chunk c: the last one whose first chunk is <= c, searched in [lo, n_tensors)
template <bool EXT, class A>
MHTE_HD uint32_t chunk_tensor_of(const A& a, uint32_t c, uint32_t lo) {
  uint32_t hi = a.k.n_tensors - 1;
  while (lo < hi) {
    const uint32_t mid = (lo + hi + 1) >> 1;
    if (tensor_chunk0<EXT>(a, mid) <= c) lo = mid; else hi = mid - 1;
  }
  return lo;
}
// The cursor: tensor ti holds a chunk <= cn < n_chunks; -> the tensor that holds cn.  One compare while cn is
// still inside ti, a search over the tensors behind it otherwise: the index only moves forward.
template <bool EXT, class A>
MHTE_HD uint32_t chunk_advance(const A& a, uint32_t ti, uint32_t cn) {
  if (ti + 1 < a.k.n_tensors && cn >= tensor_chunk0<EXT>(a, ti + 1)) ti = chunk_tensor_of<EXT>(a, cn, ti + 1);
  return ti;
}

// ---- the host builder (no HIP) --------------------------------------------------------------------------
// The tensors of a call in list order: up to N of them are written straight into the kernel arguments; a
// longer list is kept whole in the vectors until pack() lays it out for the upload.
template <class ARGS>
struct ChunkTable {
  ARGS A{};
  std::vector<void*> ptr[ARGS::kPtrs];
  std::vector<long long> num[ARGS::kNums];
  std::vector<uint32_t> chunk0;
  bool ext() const { return A.k.n_tensors > uint32_t(ARGS::kInline); }
  // Appends a tensor of len > 0 elements (p: its kPtrs pointers).  -> false when the call reaches 2^31 chunks
  // (the kernels' chunk numbers are 32-bit and c + grid must not wrap); the table is then not to be used.
  bool add(const void* const* p, long long len, long long off = 0) {
    constexpr uint32_t N = uint32_t(ARGS::kInline);
    const uint32_t m = A.k.n_tensors;
    const long long nums[2] = {len, off};
    if (m < N) {
      for (int j = 0; j < ARGS::kPtrs; ++j) A.ptr[j][m] = const_cast<void*>(p[j]);
      for (int j = 0; j < ARGS::kNums; ++j) A.num[j][m] = nums[j];
      A.chunk0[m] = A.k.n_chunks;
    } else {
      if (m == N) {   // the list outgrows the arguments: the vectors take all of it
        for (int j = 0; j < ARGS::kPtrs; ++j) ptr[j].assign(A.ptr[j], A.ptr[j] + N);
        for (int j = 0; j < ARGS::kNums; ++j) num[j].assign(A.num[j], A.num[j] + N);
        chunk0.assign(A.chunk0, A.chunk0 + N);
      }
      for (int j = 0; j < ARGS::kPtrs; ++j) ptr[j].push_back(const_cast<void*>(p[j]));
      for (int j = 0; j < ARGS::kNums; ++j) num[j].push_back(nums[j]);
      chunk0.push_back(A.k.n_chunks);
    }
    A.k.n_tensors = m + 1;
    const uint64_t chunks = A.k.n_chunks + (uint64_t(len) + kChunkElems - 1) / kChunkElems;
    if (chunks >= (uint64_t(1) << 31)) return false;
    A.k.n_chunks = uint32_t(chunks);
    return true;
  }
  // a built table read back on the host, wherever its columns are
  void* ptr_at(int j, uint32_t i) const { return ext() ? ptr[j][i] : A.ptr[j][i]; }
  long long num_at(int j, uint32_t i) const { return ext() ? num[j][i] : A.num[j][i]; }
  uint32_t chunk0_at(uint32_t i) const { return ext() ? chunk0[i] : A.chunk0[i]; }
  // ext() only.  The block of the upload: the pointer columns, then the lengths (and offsets), then chunk0,
  // each n_tensors long.  Written to dst (host memory); the EXT pointers are set for a copy of it at `at`.
  size_t packed_bytes() const { return size_t(A.k.n_tensors) * ARGS::kEntryBytes; }
  void pack(char* dst, char* at) {
    const size_t m = A.k.n_tensors;
    size_t o = 0;
    for (int j = 0; j < ARGS::kPtrs; ++j, o += m * 8) {
      memcpy(dst + o, ptr[j].data(), m * 8);
      A.x_ptr[j] = reinterpret_cast<void* const*>(at + o);
    }
    for (int j = 0; j < ARGS::kNums; ++j, o += m * 8) {
      memcpy(dst + o, num[j].data(), m * 8);
      A.x_num[j] = reinterpret_cast<const long long*>(at + o);
    }
    memcpy(dst + o, chunk0.data(), m * 4);
    A.x_chunk0 = reinterpret_cast<const uint32_t*>(at + o);
  }
};

}  // namespace mhte
#endif  // MHTE_CHUNK_TABLE_H_
