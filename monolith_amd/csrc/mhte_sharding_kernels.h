// The fused-layout packer on the device: ShardingSparseFids at op version 2 (the reference's host op,
// native_training/data/kernels/parse_sparse_feature.cc:187-240 FillFidList, :259-424 CreateOffsetTensor,
// parse_sparse_feature.h:620-990 FeatureParallelParse) for ids that are already parsed and already on the device.
//
// Every id of every feature gets a position g in ONE numbering (feature after feature, sorted-name order), and one
// launch sequence serves all features:
//   sh_keys      id, pre-output index `full` and the sort key of every position.  The sort key is PS-major,
//                sk = shard * F + (the feature's place in table-major order): the sorted ids are then, PS after
//                PS, exactly the ragged tensor a PS's raw lookup takes — table after table, feature after feature.
//   (unique)     sh_insert / sh_first: an open-addressing table of POSITIONS keyed by (full, id).  A slot is
//                claimed with a compare-and-swap and then only ever lowered with atomicMin over positions of the
//                same key, so when the launch is over it holds the key's FIRST position, whichever wavefront came
//                first: the atomics decide where a key lives, never a value that leaves the kernel.  Later
//                occurrences take the key n_pre and sort behind everything.
//   group sort   the stable digit passes of mhte_group_kernels.h over (sk, g): ranks by ballot, no atomics.
//   sh_starts    key_start[sk] = the lower bound of sk among the sorted keys -> every list's row_splits and bounds.
//   sh_emit      slot o of the sorted order: rank = o - key_start[sk]; fid_list[o] = id, fid_offset[g] = full|rank.
//   (unique)     sh_dups: a later occurrence copies the word of its first.
//   sh_offsets   feature_offset, nfl_offset, and the check of the caller's row_splits (a flag, OR-ed).
// The same input gives the same bits on every run.
#ifndef MHTE_SHARDING_KERNELS_H_
#define MHTE_SHARDING_KERNELS_H_

#include "mhte_group_kernels.h"
#include "mhte_sharding_plan.h"

namespace mhte {

constexpr int kShThreads = 256;
constexpr uint32_t kShEmpty = 0xffffffffu;
constexpr unsigned long long kShBadRowSplits = 1ull;

struct ShFeat {   // a feature as the kernels see it, sorted-name order
  const int64_t* values;
  const int64_t* row_splits;
  uint32_t id_base, row_base;   // its first id / row in the call's numbering
  uint32_t n_ids, n_rows;
  uint32_t ft;                  // its place in table-major order
  uint32_t full_base;           // pre_output_index + feature_in_table_index
  uint32_t tfc;                 // table_feature_count
  uint32_t shared;
};

struct ShArgs {
  const ShFeat* feat;       // [F]
  const ShardSlot* slot;    // [F] by ft
  uint32_t F, ps, n, rows, n_pre;
  int64_t* ids;             // [n] scratch: the ids, gathered
  uint32_t* full;           // [n] scratch
  uint2* kv;                // [n] scratch: (sort key, g), the group sort's input
  uint32_t* slots;          // [mask + 1] scratch of the unique form
  uint32_t mask;
  uint32_t* first;          // [n] scratch of the unique form: the first position of g's (feature, id)
  const uint32_t* skey;     // [n] the sorted keys | their positions
  const uint32_t* spos;
  unsigned long long* fid_offset;   // [n]
  int32_t* feature_offset;          // [rows + 1]
  uint32_t* nfl_offset;             // [F + 1]
  int64_t* fid_list;                // [n]
  int64_t* key_start;               // [n_pre + 2]: lower bounds, then the status word
  int64_t* row_splits_flat;         // [n_pre + n_lists]
  int64_t* list_bounds;             // [n_lists][2]: start, size
};

// the feature that holds id position g < n (ROWS: row r < rows): the last one whose base is <= g
template <bool ROWS>
__device__ __forceinline__ uint32_t sh_feature_of(const ShArgs& A, uint32_t g) {
  uint32_t lo = 0, hi = A.F;
  while (lo + 1 < hi) {
    const uint32_t mid = (lo + hi) >> 1;
    const uint32_t base = ROWS ? A.feat[mid].row_base : A.feat[mid].id_base;
    if (base <= g) lo = mid;
    else hi = mid;
  }
  return lo;
}

__device__ __forceinline__ uint32_t sh_hash(int64_t id, uint32_t full) {
  unsigned long long x = (unsigned long long)id ^ ((unsigned long long)full * 0x9e3779b97f4a7c15ull);
  x ^= x >> 33;
  x *= 0xff51afd7ed558ccdull;
  x ^= x >> 33;
  x *= 0xc4ceb9fe1a85ec53ull;
  x ^= x >> 33;
  return uint32_t(x);
}

__global__ __launch_bounds__(kShThreads) void sh_keys_kernel(ShArgs A) {
  const uint32_t g = blockIdx.x * kShThreads + threadIdx.x;
  if (g >= A.n) return;
  const ShFeat f = A.feat[sh_feature_of<false>(A, g)];
  const int64_t id = f.values[g - f.id_base];
  const uint32_t shard = uint32_t((unsigned long long)id % A.ps);   // (unsigned, as FillFidList's value % ps_num_)
  A.ids[g] = id;
  A.full[g] = f.full_base + shard * f.tfc;
  A.kv[g] = make_uint2(shard * A.F + f.ft, g);
}

__global__ __launch_bounds__(kShThreads) void sh_insert_kernel(ShArgs A) {
  const uint32_t g = blockIdx.x * kShThreads + threadIdx.x;
  if (g >= A.n) return;
  const int64_t id = A.ids[g];
  const uint32_t full = A.full[g];
  uint32_t h = sh_hash(id, full) & A.mask;
  for (;;) {
    uint32_t cur = __atomic_load_n(&A.slots[h], __ATOMIC_RELAXED);
    if (cur == kShEmpty) {
      cur = atomicCAS(&A.slots[h], kShEmpty, g);
      if (cur == kShEmpty) return;
    }
    // (a claimed slot only moves between positions of ONE key: whichever of them is read, the comparison holds)
    if (A.full[cur] == full && A.ids[cur] == id) {
      atomicMin(&A.slots[h], g);
      return;
    }
    h = (h + 1u) & A.mask;
  }
}

__global__ __launch_bounds__(kShThreads) void sh_first_kernel(ShArgs A) {
  const uint32_t g = blockIdx.x * kShThreads + threadIdx.x;
  if (g >= A.n) return;
  const int64_t id = A.ids[g];
  const uint32_t full = A.full[g];
  uint32_t h = sh_hash(id, full) & A.mask;
  uint32_t cur = A.slots[h];
  // (every key was inserted by the launch before: the walk ends at its slot; an empty slot cannot come first)
  while (cur != kShEmpty && !(A.full[cur] == full && A.ids[cur] == id)) {
    h = (h + 1u) & A.mask;
    cur = A.slots[h];
  }
  if (cur == kShEmpty) cur = g;
  A.first[g] = cur;
  if (cur != g) A.kv[g].x = A.n_pre;
}

__device__ __forceinline__ uint32_t sh_lower_bound(const uint32_t* __restrict__ skey, uint32_t n, uint32_t key) {
  uint32_t lo = 0, hi = n;
  while (lo < hi) {
    const uint32_t mid = lo + ((hi - lo) >> 1);
    if (skey[mid] < key) lo = mid + 1u;
    else hi = mid;
  }
  return lo;
}

// one thread per sort key, and one for n_pre (the number of ids that were placed)
__global__ __launch_bounds__(kShThreads) void sh_starts_kernel(ShArgs A) {
  const uint32_t sk = blockIdx.x * kShThreads + threadIdx.x;
  if (sk > A.n_pre) return;
  const uint32_t mine = sh_lower_bound(A.skey, A.n, sk);
  A.key_start[sk] = int64_t(mine);
  if (sk == A.n_pre) return;
  const uint32_t s = sk / A.F, ft = sk - s * A.F;
  const ShardSlot q = A.slot[ft];
  const uint32_t b0 = q.j ? sh_lower_bound(A.skey, A.n, sk - q.j) : mine;
  const uint32_t list = q.t * A.ps + s;   // (fid_list / fid_list_row_splits index, parse_sparse_feature.h:853-855)
  int64_t* rs = A.row_splits_flat + (size_t(q.pre) + size_t(s) * q.tfc + list);
  rs[q.j] = int64_t(mine - b0);
  if (q.j == q.tfc - 1u) {
    const uint32_t e = sh_lower_bound(A.skey, A.n, sk + 1u);
    rs[q.tfc] = int64_t(e - b0);
    A.list_bounds[2 * size_t(list)] = int64_t(b0);
    A.list_bounds[2 * size_t(list) + 1] = int64_t(e - b0);
  }
}

__global__ __launch_bounds__(kShThreads) void sh_emit_kernel(ShArgs A) {
  const uint32_t o = blockIdx.x * kShThreads + threadIdx.x;
  if (o >= A.n) return;
  const uint32_t sk = A.skey[o];
  if (sk >= A.n_pre) return;   // (a later occurrence of the unique form)
  const uint32_t g = A.spos[o];
  const uint32_t rank = o - uint32_t(A.key_start[sk]);
  A.fid_list[o] = A.ids[g];
  A.fid_offset[g] = ((unsigned long long)A.full[g] << 32) | rank;
}

__global__ __launch_bounds__(kShThreads) void sh_dups_kernel(ShArgs A) {
  const uint32_t g = blockIdx.x * kShThreads + threadIdx.x;
  if (g >= A.n) return;
  const uint32_t f = A.first[g];
  if (f != g) A.fid_offset[g] = A.fid_offset[f];
}

// one thread per entry of feature_offset and of nfl_offset
__global__ __launch_bounds__(kShThreads) void sh_offsets_kernel(ShArgs A) {
  const uint32_t i = blockIdx.x * kShThreads + threadIdx.x;
  if (i < A.rows) {
    const ShFeat f = A.feat[sh_feature_of<true>(A, i)];
    const uint32_t r = i - f.row_base;
    const int64_t a = f.row_splits[r], b = f.row_splits[r + 1u];
    if (a < 0 || b < a || b > int64_t(f.n_ids) || (r == 0 && a != 0) || (r == f.n_rows - 1u && b != int64_t(f.n_ids)))
      atomicOr(reinterpret_cast<unsigned long long*>(A.key_start + A.n_pre + 1), kShBadRowSplits);
    const int64_t c = a < 0 ? 0 : (a > int64_t(f.n_ids) ? int64_t(f.n_ids) : a);
    A.feature_offset[i] = int32_t(f.id_base + uint32_t(c));
  } else if (i == A.rows) {
    A.feature_offset[i] = int32_t(A.n);
  }
  if (i < A.F) {
    const ShFeat f = A.feat[i];
    A.nfl_offset[i] = f.row_base | (f.shared ? 0x80000000u : 0u);
  } else if (i == A.F) {
    A.nfl_offset[i] = A.rows + 1u;   // (parse_sparse_feature.cc:321: the entries of feature_offset)
  }
}

}  // namespace mhte
#endif  // MHTE_SHARDING_KERNELS_H_
