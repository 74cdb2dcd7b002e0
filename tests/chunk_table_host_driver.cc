// Host driver of tests/test_chunk_table_cpu.py: the argument block, the accessors, the search, the cursor and
// the builder of monolith_amd/csrc/mhte_chunk_table.h, compiled by g++ with MHTE_HOST_ONLY (no HIP).  The
// functions run here are the ones the kernels call.
//   <shape> <N> build <skip> <len> ...
//   <shape> <N> lookup <len> ...
//   <shape> <N> cursor <G> <len> ...
// shape: p1o (one pointer, offsets: the flat concat's), p2 (two pointers: the clip's), p2o (two pointers,
// offsets: the dense optimizers'); N: the inline capacity, 4 or the op's own (128, 128, 96).
// Entry i of the list has the pointers (i + 1) + j * 2^20, j = 0, 1, and the offset sum of round_up(len, 16) over
// the entries before it; entries of length 0 and the entry <skip> (-1: none) take no part but keep their span.
// A table that outgrows N is packed into a host buffer and read back through the EXT accessors.
//   build:   "n_tensors n_chunks ext", then per tensor "index len off chunk0 ok" (off -1 without offsets; ok:
//            every pointer column carries the entry's own pointer); with ext one more line, "cols" and the byte
//            offset of every column in the packed block (pointers, len, off, chunk0) and the block's size.
//            "too many chunks" when the builder refuses.
//   lookup:  per chunk c one line: chunk_tensor_of(c, lo) for lo = 0 .. chunk_tensor_of(c, 0).
//   cursor:  per start chunk w < min(G, n_chunks) one line of "chunk:tensor" pairs: the walk w, w + G, ... with
//            chunk_advance.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <type_traits>
#include <vector>

#include "mhte_chunk_table.h"

using namespace mhte;

template <class ARGS>
static bool build(ChunkTable<ARGS>& T, const std::vector<long long>& lens, int skip) {
  long long off = 0;
  for (size_t i = 0; i < lens.size(); ++i) {
    if (lens[i] != 0 && int(i) != skip) {
      const void* p[2] = {reinterpret_cast<const void*>(uintptr_t(i + 1)),
                          reinterpret_cast<const void*>(uintptr_t(i + 1) + (uintptr_t(1) << 20))};
      if (!T.add(p, lens[i], off)) return false;
    }
    off += (lens[i] + 15) & ~15ll;
  }
  return true;
}

// f(EXT flag) on the table as a kernel would see it
template <class ARGS, class F>
static void view(ChunkTable<ARGS>& T, std::vector<char>& block, F&& f) {
  if (T.ext()) {
    block.resize(T.packed_bytes());
    T.pack(block.data(), block.data());
    f(std::true_type{});
  } else {
    f(std::false_type{});
  }
}

template <class ARGS>
static int run(int argc, char** argv) {
  const char* mode = argv[3];
  int first = 4, skip = -1;
  uint32_t G = 0;
  if (!strcmp(mode, "build")) skip = atoi(argv[first++]);
  if (!strcmp(mode, "cursor")) G = uint32_t(atoll(argv[first++]));
  std::vector<long long> lens;
  for (int i = first; i < argc; ++i) lens.push_back(atoll(argv[i]));
  ChunkTable<ARGS> T;
  if (!build(T, lens, skip)) {
    printf("too many chunks\n");
    return 0;
  }
  std::vector<char> block;
  const ARGS& A = T.A;
  view(T, block, [&](auto ext) {
    constexpr bool EXT = decltype(ext)::value;
    const uint32_t n = A.k.n_tensors, C = A.k.n_chunks;
    if (!strcmp(mode, "build")) {
      printf("%u %u %d\n", n, C, EXT ? 1 : 0);
      for (uint32_t i = 0; i < n; ++i) {
        const uintptr_t p0 = uintptr_t(chunk_ptr<EXT, const char>(A, 0, i));
        bool ok = true;
        for (int j = 1; j < ARGS::kPtrs; ++j)
          ok = ok && uintptr_t(chunk_ptr<EXT, const char>(A, j, i)) == p0 + (uintptr_t(j) << 20);
        printf("%lld %lld %lld %u %d\n", (long long)(p0 - 1), chunk_len<EXT>(A, i),
               ARGS::kNums == 2 ? chunk_num<EXT>(A, ARGS::kNums - 1, i) : -1ll, tensor_chunk0<EXT>(A, i), ok ? 1 : 0);
      }
      if (EXT) {
        printf("cols");
        for (int j = 0; j < ARGS::kPtrs; ++j) printf(" %td", reinterpret_cast<const char*>(A.x_ptr[j]) - block.data());
        for (int j = 0; j < ARGS::kNums; ++j) printf(" %td", reinterpret_cast<const char*>(A.x_num[j]) - block.data());
        printf(" %td %zu\n", reinterpret_cast<const char*>(A.x_chunk0) - block.data(), block.size());
      }
    } else if (!strcmp(mode, "lookup")) {
      for (uint32_t c = 0; c < C; ++c) {
        const uint32_t ti = chunk_tensor_of<EXT>(A, c, 0);
        for (uint32_t lo = 0; lo <= ti; ++lo) printf("%u ", chunk_tensor_of<EXT>(A, c, lo));
        printf("\n");
      }
    } else {
      for (uint32_t w = 0; w < G && w < C; ++w) {
        uint32_t ti = chunk_tensor_of<EXT>(A, w, 0);
        printf("%u:%u", w, ti);
        for (uint32_t c = w; c + G < C; c += G) {   // (the kernels' loop: the next chunk while this one is worked on)
          ti = chunk_advance<EXT>(A, ti, c + G);
          printf(" %u:%u", c + G, ti);
        }
        printf("\n");
      }
    }
  });
  return 0;
}

int main(int argc, char** argv) {
  if (argc >= 4) {
    const char* shape = argv[1];
    const int N = atoi(argv[2]);
    if (!strcmp(shape, "p1o") && N == 4) return run<ChunkArgs<4, 1, true>>(argc, argv);
    if (!strcmp(shape, "p1o") && N == 128) return run<ChunkArgs<128, 1, true>>(argc, argv);
    if (!strcmp(shape, "p2") && N == 4) return run<ChunkArgs<4, 2, false>>(argc, argv);
    if (!strcmp(shape, "p2") && N == 128) return run<ChunkArgs<128, 2, false>>(argc, argv);
    if (!strcmp(shape, "p2o") && N == 4) return run<ChunkArgs<4, 2, true>>(argc, argv);
    if (!strcmp(shape, "p2o") && N == 96) return run<ChunkArgs<96, 2, true>>(argc, argv);
  }
  fprintf(stderr, "usage: %s p1o|p2|p2o <N> build <skip> <len> ... | lookup <len> ... | cursor <G> <len> ...\n", argv[0]);
  return 1;
}
