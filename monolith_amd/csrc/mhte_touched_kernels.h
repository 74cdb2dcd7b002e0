// Device-resident touched-key set: the keys (int64 fid, int32 tag) that an update path changed since
// the last GetAndClear (hopscotch_hash_set.cc:104-122,173-195 restated for whole batches; DESIGN.md,
// "Touched-key set").  gfx950.
//
// Table: open addressing, linear probing with wrap, 16-byte slots, a power of two >= 2 * (C + 1 +
// max_insert) of them, so the load stays under one half even before a cut is applied.
//   slot.fid  int64
//   slot.w    uint64 = state << 32 | stamp
//             state  0 EMPTY, 1 BUSY (claimed, fid not yet written), tag + 2 live
//             stamp  epoch << 22 | smallest position of the key in the call that inserted it; the
//                    epoch (0..1022, a device counter) tells a key that is new in THIS call from an
//                    older one without a reset between calls; 0xffffffff = no stamp
// A 128-bit key cannot be claimed by one CAS: w goes EMPTY -> BUSY by CAS, the winner stores fid and
// release-stores the live w in the same loop iteration; a prober that meets BUSY reads the slot again
// on its next trip of the ONE probe loop (no spin inside a divergent branch).
//
// One insert call = at most kTkMaxPositions positions (segment-major, then index-minor) and five
// launches, of which the last four leave at once unless the call overflows the capacity:
//   tk_insert    every valid position finds or claims its key; new keys are counted
//   tk_mark      (size0 + n_new > C only) one bit per first-occurrence position of a new key
//   tk_select    one workgroup: finds the cut c (the position in front of which the sequential rule
//                clears), settles size / dropped / clears, advances the epoch, zeroes the bitmap
//   tk_clear     (cut only) empties the table; (epoch wrap only) resets the stamps
//   tk_reinsert  (cut only) inserts the positions >= c
// All counts stay on the device; nothing here allocates or synchronises with the host.
#ifndef MHTE_TOUCHED_KERNELS_H_
#define MHTE_TOUCHED_KERNELS_H_

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mhte_core.h"

namespace mhte {

constexpr uint32_t kTkPosBits = 22;
constexpr uint32_t kTkMaxPositions = (1u << kTkPosBits) - 1u;   // per insert call
constexpr uint32_t kTkEpochs = 1023;                           // epoch field 1023 = "no stamp"
constexpr uint32_t kTkNoStamp = 0xffffffffu;
constexpr uint32_t kTkNoCut = 0xffffffffu;
constexpr uint32_t kTkEmpty = 0, kTkBusy = 1;
constexpr int kTkBlock = 256;
constexpr int kTkSelectBlock = 1024;

struct TkSlot {
  int64_t fid;
  unsigned long long w;
};
static_assert(sizeof(TkSlot) == 16, "TkSlot");

struct TkCtl {
  unsigned long long dropped;   // keys dropped by clears
  unsigned long long clears;
  uint32_t size;                // keys in the set
  uint32_t epoch;               // 0..kTkEpochs-1
  uint32_t n_new;               // keys tk_insert added in the running call
  uint32_t last_p1;             // 1 + the largest valid position of the running call (0: empty call)
  uint32_t cut;                 // kTkNoCut or c
  uint32_t sweep;               // the epoch wrapped: tk_clear resets the stamps
  uint32_t steal_n;             // tk_steal's output cursor
};

// one ragged segment of a call: positions base .. base + n_max - 1 stand for ids[start + i]; valid are
// those with start + i < min(*n_dev, start + n_max) (n_dev NULL: all) and keep[start + i] != 0 (keep
// NULL: all)
struct TkDesc {
  const int64_t* ids;
  const uint32_t* n_dev;
  const int32_t* keep;
  uint32_t start;
  uint32_t n_max;
  int32_t tag;
  uint32_t pad;
};

struct TkDescs {
  const TkDesc* dev;   // device-resident array, or NULL: `one`
  TkDesc one;
  uint32_t nseg;
  uint32_t total;      // sum of n_max
  uint64_t skip[2];    // bit s set: segment s (< 128) holds nothing in this call
};

struct TkView {
  TkSlot* slots;
  TkCtl* ctl;
  uint32_t* bitmap;    // [(max positions + 31) / 32 + 1]
  uint32_t mask;       // slots - 1
  uint32_t capacity;   // C
};

__device__ __forceinline__ unsigned long long tk_load_w(const unsigned long long* p) {
  return __hip_atomic_load(p, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ uint32_t tk_hash(int64_t fid, int32_t tag) {
  return uint32_t(hash_key(fid ^ static_cast<int64_t>(uint64_t(uint32_t(tag)) * 0x9E3779B97F4A7C15ull)) >> 17);
}

// position -> (fid, tag); false when the position holds nothing
__device__ __forceinline__ bool tk_position(const TkDescs& ds, uint32_t p, int64_t* fid, int32_t* tag) {
  if (p >= ds.total) return false;
  uint32_t base = 0;
  for (uint32_t s = 0; s < ds.nseg; ++s) {
    const TkDesc d = ds.dev ? ds.dev[s] : ds.one;
    if (p - base < d.n_max) {
      if (s < 128 && ((ds.skip[s >> 6] >> (s & 63)) & 1ull)) return false;
      const uint32_t i = p - base;
      if (d.n_dev) {
        const uint32_t n = *d.n_dev;
        if (n <= d.start || i >= n - d.start) return false;
      }
      if (d.keep && d.keep[size_t(d.start) + i] == 0) return false;
      *fid = d.ids[size_t(d.start) + i];
      *tag = d.tag;
      return true;
    }
    base += d.n_max;
  }
  return false;
}

// Finds or claims (fid, tag).  stamp: what a claiming thread publishes; epoch < kTkEpochs: a key whose
// stamp carries this epoch takes atomicMin(stamp).  Returns true when the key was absent.
__device__ __forceinline__ bool tk_find_or_claim(const TkView& v, int64_t fid, int32_t tag, uint32_t stamp,
                                                 uint32_t epoch) {
  const unsigned long long live = static_cast<unsigned long long>(uint32_t(tag) + 2u);
  uint32_t h = tk_hash(fid, tag) & v.mask;
  bool done = false, claimed = false;
  // ONE loop with ONE exit behind it: the claiming block falls through to the loop's latch like every other,
  // so a lane of the same wavefront that waits on BUSY always sees the publication on its next trip.
  // (bounded: the load stays under one half, so an EMPTY slot ends every probe sequence; the bound only keeps
  // a corrupted table from hanging the device)
  for (uint64_t trips = 0; !done && trips < (uint64_t(v.mask) + 1u) * 4u; ++trips) {
    TkSlot* s = v.slots + h;
    const unsigned long long w = tk_load_w(&s->w);
    const uint32_t st = uint32_t(w >> 32);
    if (st == kTkEmpty) {
      const unsigned long long old =
          atomicCAS(&s->w, 0ull, (static_cast<unsigned long long>(kTkBusy) << 32) | kTkNoStamp);
      if (old == 0ull) {
        __hip_atomic_store(&s->fid, fid, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(&s->w, (live << 32) | stamp, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
        claimed = true;
        done = true;
      }
      // lost the race: read the same slot again
    } else if (st != kTkBusy) {
      const int64_t f = __hip_atomic_load(&s->fid, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (st == uint32_t(live) && f == fid) {
        if (epoch < kTkEpochs && (uint32_t(w) >> kTkPosBits) == epoch)
          atomicMin(reinterpret_cast<uint32_t*>(&s->w), stamp);   // (little endian: the low word)
        done = true;
      } else {
        h = (h + 1u) & v.mask;
      }
    }
    // BUSY: the claimer publishes in the trip of its CAS; read again
  }
  return claimed;
}

// slot index of a key that is in the table (tk_mark); mask + 1 when absent
__device__ __forceinline__ uint32_t tk_find(const TkView& v, int64_t fid, int32_t tag) {
  const uint32_t live = uint32_t(tag) + 2u;
  uint32_t h = tk_hash(fid, tag) & v.mask;
  for (uint32_t trips = 0; trips <= v.mask; ++trips) {
    const TkSlot s = v.slots[h];
    const uint32_t st = uint32_t(s.w >> 32);
    if (st == kTkEmpty) break;
    if (st == live && s.fid == fid) return h;
    h = (h + 1u) & v.mask;
  }
  return v.mask + 1u;
}

__device__ __forceinline__ uint32_t tk_block_sum(uint32_t x, uint32_t* sh) {
  for (int o = 32; o > 0; o >>= 1) x += __shfl_down(x, o);
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = x;
  __syncthreads();
  uint32_t r = 0;
  for (int w = 0; w < int(blockDim.x >> 6); ++w) r += sh[w];
  __syncthreads();
  return r;
}
__device__ __forceinline__ uint32_t tk_block_max(uint32_t x, uint32_t* sh) {
  for (int o = 32; o > 0; o >>= 1) x = max(x, uint32_t(__shfl_down(x, o)));
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = x;
  __syncthreads();
  uint32_t r = 0;
  for (int w = 0; w < int(blockDim.x >> 6); ++w) r = max(r, sh[w]);
  __syncthreads();
  return r;
}

__global__ __launch_bounds__(kTkBlock) void tk_insert_kernel(TkView v, TkDescs ds) {
  __shared__ uint32_t sh[kTkBlock / 64];
  const uint32_t p = blockIdx.x * kTkBlock + threadIdx.x;
  const uint32_t epoch = v.ctl->epoch;   // (written by tk_select of the call before: a launch boundary)
  int64_t fid = 0;
  int32_t tag = 0;
  const bool valid = tk_position(ds, p, &fid, &tag);
  uint32_t isnew = 0;
  if (valid) isnew = tk_find_or_claim(v, fid, tag, (epoch << kTkPosBits) | p, epoch) ? 1u : 0u;
  const uint32_t n_new = tk_block_sum(isnew, sh);
  const uint32_t last = tk_block_max(valid ? p + 1u : 0u, sh);
  if (threadIdx.x == 0) {
    if (n_new) atomicAdd(&v.ctl->n_new, n_new);
    if (last) atomicMax(&v.ctl->last_p1, last);
  }
}

__global__ __launch_bounds__(kTkBlock) void tk_mark_kernel(TkView v, TkDescs ds) {
  const TkCtl* c = v.ctl;
  const uint32_t size0 = c->size;
  if (size0 > v.capacity || size0 + c->n_new <= v.capacity) return;   // cut at 0, or no cut
  const uint32_t p = blockIdx.x * kTkBlock + threadIdx.x;
  int64_t fid = 0;
  int32_t tag = 0;
  if (!tk_position(ds, p, &fid, &tag)) return;
  const uint32_t h = tk_find(v, fid, tag);
  if (h > v.mask) return;
  if (uint32_t(v.slots[h].w) == ((c->epoch << kTkPosBits) | p)) atomicOr(&v.bitmap[p >> 5], 1u << (p & 31));
}

// one workgroup
__global__ __launch_bounds__(kTkSelectBlock) void tk_select_kernel(TkView v, uint32_t total) {
  __shared__ uint32_t cnt[kTkSelectBlock];
  __shared__ uint32_t found;
  TkCtl* c = v.ctl;
  const uint32_t size0 = c->size, n_new = c->n_new, last_p1 = c->last_p1;
  const uint32_t C = v.capacity;
  const bool over0 = size0 > C;
  const bool scan = !over0 && last_p1 && size0 + n_new > C;   // (uniform)
  uint32_t f = kTkNoCut;   // first-occurrence position of the (C + 1 - size0)-th new key
  if (scan) {
    const uint32_t K = C + 1u - size0;   // 1 <= K <= n_new
    const uint32_t words = (total + 31u) / 32u;
    const uint32_t per = (words + kTkSelectBlock - 1u) / kTkSelectBlock;
    const uint32_t w0 = min(words, threadIdx.x * per), w1 = min(words, w0 + per);
    uint32_t mine = 0;
    for (uint32_t w = w0; w < w1; ++w) mine += __popc(v.bitmap[w]);
    cnt[threadIdx.x] = mine;
    if (threadIdx.x == 0) found = kTkNoCut;
    __syncthreads();
    if (threadIdx.x == 0) {   // exclusive scan of 1024 counts
      uint32_t run = 0;
      for (int i = 0; i < kTkSelectBlock; ++i) {
        const uint32_t x = cnt[i];
        cnt[i] = run;
        run += x;
      }
    }
    __syncthreads();
    const uint32_t before = cnt[threadIdx.x];
    if (before < K && K <= before + mine) {   // exactly one thread
      uint32_t need = K - before;
      for (uint32_t w = w0; w < w1; ++w) {
        uint32_t bits = v.bitmap[w];
        const uint32_t pc = __popc(bits);
        if (need <= pc) {
          for (uint32_t k = 1; k < need; ++k) bits &= bits - 1u;
          found = w * 32u + uint32_t(__ffs(int(bits)) - 1);
          break;
        }
        need -= pc;
      }
    }
    __syncthreads();
    f = found;
    for (uint32_t w = w0; w < w1; ++w) v.bitmap[w] = 0;   // clean for the next call
  }
  if (threadIdx.x != 0) return;
  uint32_t cut = kTkNoCut;
  if (last_p1) {
    if (over0) {
      cut = 0;
      c->dropped += size0;
    } else if (f != kTkNoCut && f + 1u < last_p1) {   // a valid position follows the key that filled the set
      cut = f + 1u;
      c->dropped += uint64_t(size0) + (C + 1u - size0);
    }
  }
  if (cut != kTkNoCut) {
    c->clears += 1;
    c->size = 0;   // tk_reinsert counts
  } else {
    c->size = size0 + n_new;
  }
  c->cut = cut;
  c->n_new = 0;
  c->last_p1 = 0;
  const uint32_t e = c->epoch + 1u;
  c->epoch = e >= kTkEpochs ? 0u : e;
  c->sweep = (e >= kTkEpochs && cut == kTkNoCut) ? 1u : 0u;
}

// mode 0: after tk_select (clears on a cut, sweeps the stamps on an epoch wrap); 1: unconditional
__global__ __launch_bounds__(kTkBlock) void tk_clear_kernel(TkView v, int mode) {
  const bool cut = mode == 1 || v.ctl->cut != kTkNoCut;
  const bool sweep = !cut && v.ctl->sweep != 0;
  if (!cut && !sweep) return;
  const uint32_t n = v.mask + 1u;
  for (uint32_t i = blockIdx.x * kTkBlock + threadIdx.x; i < n; i += gridDim.x * kTkBlock) {
    if (cut) {
      v.slots[i].fid = 0;
      v.slots[i].w = 0ull;
    } else if (uint32_t(v.slots[i].w >> 32) >= 2u) {   // (an EMPTY slot stays all zero: the claim's CAS expects it)
      v.slots[i].w |= static_cast<unsigned long long>(kTkNoStamp);
    }
  }
  if (mode == 1 && blockIdx.x == 0 && threadIdx.x == 0) v.ctl->size = 0;
}

__global__ __launch_bounds__(kTkBlock) void tk_reinsert_kernel(TkView v, TkDescs ds) {
  __shared__ uint32_t sh[kTkBlock / 64];
  const uint32_t cut = v.ctl->cut;
  if (cut == kTkNoCut) return;
  const uint32_t p = blockIdx.x * kTkBlock + threadIdx.x;
  int64_t fid = 0;
  int32_t tag = 0;
  const bool valid = p >= cut && tk_position(ds, p, &fid, &tag);
  uint32_t isnew = 0;
  if (valid) isnew = tk_find_or_claim(v, fid, tag, kTkNoStamp, kTkEpochs) ? 1u : 0u;
  const uint32_t n_new = tk_block_sum(isnew, sh);
  if (threadIdx.x == 0 && n_new) atomicAdd(&v.ctl->size, n_new);
}

// compaction of the live slots into (ids, tags); the order is unspecified.  cap bounds the writes.
__global__ __launch_bounds__(kTkBlock) void tk_steal_kernel(TkView v, int64_t* __restrict__ ids,
                                                            int32_t* __restrict__ tags, uint32_t cap) {
  const uint32_t n = v.mask + 1u;   // (a multiple of 64: whole wavefronts run the same trips)
  for (uint32_t i = blockIdx.x * kTkBlock + threadIdx.x; i < n; i += gridDim.x * kTkBlock) {
    const TkSlot s = v.slots[i];
    const uint32_t st = uint32_t(s.w >> 32);
    const bool live = st >= 2u;
    const unsigned long long m = __ballot(live);
    uint32_t base = 0;
    const uint32_t lane = threadIdx.x & 63u;
    if (m) {
      const int leader = __ffsll(static_cast<long long>(m)) - 1;
      if (int(lane) == leader) base = atomicAdd(&v.ctl->steal_n, uint32_t(__popcll(m)));
      base = __shfl(base, leader);
    }
    if (live) {
      const uint32_t o = base + uint32_t(__popcll(m & ((1ull << lane) - 1ull)));
      if (o < cap) {
        ids[o] = s.fid;
        if (tags) tags[o] = int32_t(st - 2u);
      }
    }
  }
}

}  // namespace mhte

#endif  // MHTE_TOUCHED_KERNELS_H_
