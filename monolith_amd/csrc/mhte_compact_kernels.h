// Table compaction (Table::compact, mhte.hip): the rows of the live entries move into the lowest row
// handles, so that the slabs above them can be released.  Included by mhte.hip only.
//
// A = row handles in use (the bump counter), L = live entries (the side slot's row included).  Keys,
// bucket positions and timestamps stay; only the `row` word of the slots changes.
//   compact_mark        bucket scan: one bit per live handle < L; per 1024-slot tile, the slots whose
//                       handle is >= L (the movers)
//   compact_hole_count  per 256-word tile of the bitmap: its zero bits (the holes)
//   compact_hole_emit   the holes, ascending                      (offsets: host scan of the counts)
//   compact_mover_emit  (slot, handle) of the movers, slot order  (offsets: host scan of the counts)
//   compact_move        mover i takes hole i: the row is copied, the slot's row word rewritten
//   compact_counters    next handle <- L; the keys counted ahead for row reservations go back
// Sources are all >= L and destinations all < L: no copy reads what another one writes.  Holes and
// movers are equal in number when the handles in the buckets are distinct and the counters true; the
// host checks that before the first row moves.
// Persistent workgroups, grid-stride over tiles, as the other full-table scans (evict_kernel); the
// only atomics are the bitmap's ORs.
#ifndef MHTE_COMPACT_KERNELS_H_
#define MHTE_COMPACT_KERNELS_H_

#include <type_traits>

#include "mhte_kernels.h"

namespace mhte {

constexpr uint32_t kCompactTileSlots = 1024;   // bucket slots per tile of the two scans (4 per thread)
constexpr uint32_t kCompactTileWords = 256;    // bitmap words per tile of the hole passes (1 per thread)

// occupied slot t -> its row handle; kNoRow for an empty slot or one past the table
__device__ __forceinline__ uint32_t compact_slot_row(const TableView& tv, uint64_t t, uint64_t nslots, bool& occ) {
  occ = false;
  if (t >= nslots) return kNoRow;
  const GBucket* b = global_bucket(tv.buckets) + (t >> 2);
  const int s = int(t & 3);
  if (b->key[s] == kEmptyKey) return kNoRow;
  occ = true;
  return b->row[s];
}

__global__ __launch_bounds__(256) void compact_mark_kernel(TableView tv, uint32_t L, uint64_t ntiles,
                                                           uint32_t* __restrict__ bitmap,
                                                           uint32_t* __restrict__ tile_movers) {
  __shared__ uint32_t wsum[4];
  const uint64_t nslots = (uint64_t(1) << tv.hp) * kSlots;
#pragma unroll 1
  for (uint64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    uint32_t c = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const uint64_t t = tile * kCompactTileSlots + uint64_t(k) * 256 + threadIdx.x;
      bool occ;
      const uint32_t r = compact_slot_row(tv, t, nslots, occ);
      if (occ) {
        if (r < L) atomicOr(&bitmap[r >> 5], 1u << (r & 31u));
        else ++c;
      }
    }
    for (int o = 32; o > 0; o >>= 1) c += __shfl_down(c, o);
    if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0) tile_movers[tile] = wsum[0] + wsum[1] + wsum[2] + wsum[3];
    __syncthreads();
  }
  if (blockIdx.x == 0 && threadIdx.x == 0 && tv.ctr->special_state == 1) {
    const uint32_t r = tv.ctr->special_row;
    if (r < L) atomicOr(&bitmap[r >> 5], 1u << (r & 31u));
  }
}

// the zero bits of bitmap word w that stand for handles < L
__device__ __forceinline__ uint32_t compact_free_bits(const uint32_t* __restrict__ bitmap, uint64_t w,
                                                      uint32_t nwords, uint32_t L) {
  if (w >= nwords) return 0u;
  uint32_t free_bits = ~bitmap[w];
  if (w == nwords - 1 && (L & 31u)) free_bits &= (1u << (L & 31u)) - 1u;
  return free_bits;
}

__global__ __launch_bounds__(256) void compact_hole_count_kernel(const uint32_t* __restrict__ bitmap,
                                                                 uint32_t nwords, uint32_t L, uint32_t ntiles,
                                                                 uint32_t* __restrict__ tile_holes) {
  __shared__ uint32_t wsum[4];
#pragma unroll 1
  for (uint32_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    uint32_t c = uint32_t(__popc(compact_free_bits(bitmap, uint64_t(tile) * kCompactTileWords + threadIdx.x, nwords, L)));
    for (int o = 32; o > 0; o >>= 1) c += __shfl_down(c, o);
    if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0) tile_holes[tile] = wsum[0] + wsum[1] + wsum[2] + wsum[3];
    __syncthreads();
  }
}

// tile_off: exclusive scan of tile_holes; holes [n_holes]
__global__ __launch_bounds__(256) void compact_hole_emit_kernel(const uint32_t* __restrict__ bitmap,
                                                                uint32_t nwords, uint32_t L, uint32_t ntiles,
                                                                const uint32_t* __restrict__ tile_off,
                                                                uint32_t* __restrict__ holes, uint32_t n_holes) {
  __shared__ uint32_t wsum[4];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll 1
  for (uint32_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const uint64_t word = uint64_t(tile) * kCompactTileWords + threadIdx.x;
    uint32_t free_bits = compact_free_bits(bitmap, word, nwords, L);
    const uint32_t c = uint32_t(__popc(free_bits));
    // exclusive scan of c over the workgroup (thread order == handle order)
    uint32_t incl = c;
    for (int o = 1; o < 64; o <<= 1) {
      const uint32_t v = __shfl_up(incl, o);
      if (lane >= o) incl += v;
    }
    if (lane == 63) wsum[w] = incl;
    __syncthreads();
    uint32_t woff = 0;
    for (int i = 0; i < w; ++i) woff += wsum[i];
    uint32_t o = tile_off[tile] + woff + (incl - c);
    while (free_bits) {
      const uint32_t bit = uint32_t(__ffs(int(free_bits))) - 1u;
      free_bits &= free_bits - 1u;
      if (o < n_holes) holes[o] = uint32_t(word) * 32u + bit;
      ++o;
    }
    __syncthreads();
  }
}

// tile_off: exclusive scan of tile_movers; mv_slot, mv_src [n_movers]
__global__ __launch_bounds__(256) void compact_mover_emit_kernel(TableView tv, uint32_t L, uint64_t ntiles,
                                                                 const uint32_t* __restrict__ tile_off,
                                                                 uint64_t* __restrict__ mv_slot,
                                                                 uint32_t* __restrict__ mv_src, uint32_t n_movers) {
  __shared__ uint32_t wsum[4];
  const uint64_t nslots = (uint64_t(1) << tv.hp) * kSlots;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll 1
  for (uint64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    uint32_t run = tile_off[tile];
#pragma unroll 1
    for (int k = 0; k < 4; ++k) {   // (256 consecutive slots a trip: rank order == slot order)
      const uint64_t t = tile * kCompactTileSlots + uint64_t(k) * 256 + threadIdx.x;
      bool occ;
      const uint32_t r = compact_slot_row(tv, t, nslots, occ);
      const bool mover = occ && r >= L;
      const uint64_t bal = __ballot(mover);
      if (lane == 0) wsum[w] = uint32_t(__popcll(bal));
      __syncthreads();
      uint32_t woff = 0, tot = 0;
      for (int i = 0; i < 4; ++i) {
        if (i < w) woff += wsum[i];
        tot += wsum[i];
      }
      if (mover) {
        const uint32_t o = run + woff + uint32_t(__popcll(bal & ((uint64_t(1) << lane) - 1)));
        if (o < n_movers) {
          mv_slot[o] = t;
          mv_src[o] = r;
        }
      }
      run += tot;
      __syncthreads();
    }
  }
}

// Mover i (slot movers first, then the side slot's row when special_src != kNoRow) takes holes[i].  A group
// of G lanes (a power of two <= 64) copies one row: float4 units when VEC == 4 (row_floats a multiple
// of 4: slab bases are allocation-aligned, so both rows then start on 16 bytes), floats otherwise; four
// units in flight per lane.  row_cap: rows the slabs hold.
template <int VEC>
__global__ __launch_bounds__(256) void compact_move_kernel(TableView tv, const uint64_t* __restrict__ mv_slot,
                                                           const uint32_t* __restrict__ mv_src,
                                                           const uint32_t* __restrict__ holes,
                                                           uint32_t n_slot_movers, uint32_t special_src,
                                                           uint32_t L, uint64_t row_cap, uint32_t G) {
  typedef float f32x4 __attribute__((ext_vector_type(4)));
  typedef typename std::conditional<VEC == 4, f32x4, float>::type unit_t;
  typedef MHTE_GLOBAL unit_t gunit_t;
  const uint32_t n_movers = n_slot_movers + (special_src != kNoRow ? 1u : 0u);
  const uint32_t units = tv.row_floats / VEC;
  const uint32_t j = threadIdx.x & (G - 1u);
  const uint64_t ngroups = uint64_t(gridDim.x) * 256 / G;
#pragma unroll 1
  for (uint64_t i = (uint64_t(blockIdx.x) * 256 + threadIdx.x) / G; i < n_movers; i += ngroups) {
    const bool spec = i >= n_slot_movers;
    const uint32_t src = spec ? special_src : mv_src[i];
    const uint32_t dst = holes[i];
    if (uint64_t(src) >= row_cap || dst >= L) continue;   // (never, with true counters: no wild copy)
    const gunit_t* sp = (const gunit_t*)row_ptr(tv, src);
    gunit_t* dp = (gunit_t*)row_ptr(tv, dst);
#pragma unroll 1
    for (uint32_t e = j; e < units; e += 4u * G) {
      unit_t v[4];
#pragma unroll
      for (int q = 0; q < 4; ++q)
        if (e + uint32_t(q) * G < units) v[q] = sp[e + uint32_t(q) * G];
#pragma unroll
      for (int q = 0; q < 4; ++q)
        if (e + uint32_t(q) * G < units) dp[e + uint32_t(q) * G] = v[q];
    }
    if (j == 0) {
      if (spec) {
        tv.ctr->special_row = dst;
      } else {
        const uint64_t t = mv_slot[i];
        global_bucket(tv.buckets)[t >> 2].row[t & 3] = dst;
      }
    }
  }
}

// the bump counter starts over at L; keys counted ahead for row reservations that no update has
// consumed (Counters::reserved) go back: those reservations are void from here on
__global__ void compact_counters_kernel(Counters* __restrict__ c, uint32_t L) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  const unsigned long long live = (c->alloc >> 32) - c->reserved;
  c->alloc = (live << 32) | L;
  c->reserved = 0;
}

}  // namespace mhte

#endif  // MHTE_COMPACT_KERNELS_H_
