// libmhte.so — MI355X-native MultiHashTable engine: host side + C ABI (include/monolith_amd_hash_table.h).
//
// Host responsibilities (everything else is in mhte_kernels.h):
//   * table geometry in HBM: bucket array (2^hp x 64 B), row slabs, counters
//   * proactive doubling (load factor <= max_load_factor) so the fast insert path never needs the
//     reference's "double when displacement fails" (cuckoohash_map.hpp:1296-1299) mid-kernel
//   * the MultiHashTable op loop over tables sorted by name
//     (RT/ops/multi_hash_table_{lookup,update}_op.cc), argument checks and status mapping
// Build: hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -shared -fPIC mhte.hip
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>
#include <hip/hip_fp16.h>

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <atomic>
#include <exception>
#include <mutex>
#include <future>
#include <initializer_list>
#include <thread>
#include <type_traits>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/monolith_amd_hash_table.h"
#include <unistd.h>
#include <dirent.h>
#include <ctype.h>

#include "mhte_ckpt_parts.h"
#include "mhte_proto_config.h"
#include <map>
#include "mhte_pool_kernels.h"
#include "mhte_pool_split_kernels.h"
#include "mhte_clip_kernels.h"
#include "mhte_flat_kernels.h"
#include "mhte_dense_opt_kernels.h"
#include "mhte_ffm_kernels.h"
#include "mhte_auc_kernels.h"
#include "mhte_bsm_kernels.h"
#include "mhte_fi_kernels.h"
#include "mhte_group_kernels.h"
#include "mhte_split_kernels.h"
#include "mhte_sharding_kernels.h"
#include "mhte_layout_kernels.h"
#include "mhte_step_kernels.h"
#include "mhte_mstep_kernels.h"
#include "mhte_shard_kernels.h"
#include "mhte_compact_kernels.h"
#include "mhte_gemm_kernels.h"

namespace mhte {

// ------------------------------------------------------------------------------------------ errors
static thread_local std::string g_last_error;

#define HIP_OK(expr)                                                                          \
  do {                                                                                        \
    hipError_t e__ = (expr);                                                                  \
    if (e__ != hipSuccess) {                                                                  \
      throw Error(e__ == hipErrorOutOfMemory ? MHTE_RESOURCE_EXHAUSTED : MHTE_UNAVAILABLE,    \
                  std::string(#expr) + ": " + hipGetErrorString(e__));                        \
    }                                                                                         \
  } while (0)

static inline hipStream_t S(void* s) { return reinterpret_cast<hipStream_t>(s); }

template <class T>
struct DevBuf {
  T* p = nullptr;
  size_t cap = 0;
  ~DevBuf() { if (p) (void)hipFree(p); }
  void reserve(size_t n) {
    if (n <= cap) return;
    if (p) {
      HIP_OK(hipDeviceSynchronize());
      HIP_OK(hipFree(p));
      p = nullptr;
    }
    size_t want = std::max<size_t>(n, cap * 2);
    HIP_OK(hipMalloc(&p, want * sizeof(T)));
    cap = want;
  }
};

// pinned host staging (device <-> host copies at link speed, not through a pageable bounce buffer)
template <class T>
struct HostBuf {
  T* p = nullptr;
  size_t cap = 0;
  ~HostBuf() { if (p) (void)hipHostFree(p); }
  void reserve(size_t n) {
    if (n <= cap) return;
    if (p) {
      HIP_OK(hipHostFree(p));
      p = nullptr;
    }
    size_t want = std::max<size_t>(n, cap * 2);
    HIP_OK(hipHostMalloc(reinterpret_cast<void**>(&p), want * sizeof(T), hipHostMallocDefault));
    cap = want;
  }
};

static inline uint32_t ceil_log2(uint64_t n) {
  uint32_t l = 0;
  while ((uint64_t(1) << l) < n) ++l;
  return l;
}


// ------------------------------------------------------------------------------------------ timing
// Kernel-exact timing of the step kernels (mhte_profile_arm / mhte_profile_read): while armed, a
// hot launch goes through hipExtLaunchKernelGGL, whose start/stop events are stamped with the
// kernel's own begin and end on its queue — the same interval rocprofv3 --kernel-trace reports —
// instead of events recorded around the launch, which also contain the dispatch gap.
enum ProfTag : int32_t {
  kTagLookup = 1, kTagSumApply = 2,
  kTagSlowpath = 6, kTagDedup = 7, kTagUpsert = 8, kTagStepFwd = 9, kTagStepBwd = 10,
  kTagMStepFwd = 11, kTagMStepBwd = 12,
  kTagShardBuild = 13, kTagShardLookup = 14, kTagShardGather = 15, kTagShardUpsert = 16,
  kTagShardPush = 17, kTagShardWait = 18, kTagGemm = 19
};

// Per-wavefront timeline of the step kernels (mhte_trace_begin / mhte_trace_end): each traced
// launch gets a region of kTraceWords words per wavefront in the caller's device buffer.
struct TraceLaunch {
  int32_t tag, grid, block;
  int64_t offset;  // first record (in records of 3 words)
};
struct Trace {
  unsigned long long* buf = nullptr;
  int64_t cap = 0, cursor = 0;
  std::vector<TraceLaunch> launches;
};
static thread_local Trace g_trace;
static unsigned long long* trace_region(int32_t tag, uint32_t grid, uint32_t block) {
  if (!g_trace.buf) return nullptr;
  const int64_t waves = int64_t(grid) * ((block + 63) / 64);
  if (g_trace.cursor + waves > g_trace.cap) return nullptr;
  unsigned long long* p = g_trace.buf + size_t(kTraceWords) * g_trace.cursor;
  g_trace.launches.push_back(TraceLaunch{tag, int32_t(grid), int32_t(block), g_trace.cursor});
  g_trace.cursor += waves;
  return p;
}
struct Prof {
  std::vector<hipEvent_t> ev;  // 2 per recorded launch, created when the pass is armed (creating them at the
                               // launch made the timed launches the slowest to enqueue: on a slow host the
                               // queue drained between them and the kernels themselves ran slower)
  std::vector<int32_t> tag;
  int32_t armed = 0;
};
static thread_local Prof g_prof;

// Where the HOST's time goes in a call of the pipelined step (MHTE_HOST_PROF=1; VERDICT r5 weak #7: a plain C
// loop over mhte_table_step_forward / _backward is host-bound on a slow box): per entry point the calls, the
// time inside the call, the part of it before the table lock is held (argument checks, hipSetDevice, the lock)
// and the part inside the launch expressions (the HIP runtime's: kernarg copy, packet, doorbell) — the rest is
// this library's own bookkeeping.  Printed at exit (stderr, or the file MHTE_HOST_PROF_OUT names).
struct HostProfSec {
  const char* name;
  uint64_t calls = 0, total_ns = 0, pre_ns = 0, launch_ns = 0, launches = 0;
};
static HostProfSec g_hp[2] = {{"mhte_table_step_forward"}, {"mhte_table_step_backward"}};
static thread_local HostProfSec* t_hp = nullptr;
static inline uint64_t now_ns() {
  return uint64_t(std::chrono::duration_cast<std::chrono::nanoseconds>(
                      std::chrono::steady_clock::now().time_since_epoch()).count());
}
static void host_prof_dump() {
  FILE* f = stderr;
  if (const char* p = getenv("MHTE_HOST_PROF_OUT")) {
    FILE* g = fopen(p, "a");
    if (g) f = g;
  }
  fprintf(f, "| entry point | calls | us per call | before the lock | in launch expressions (HIP runtime) | launches per call | the rest (this library) |\n|---|---|---|---|---|---|---|\n");
  for (const HostProfSec& s : g_hp) {
    if (!s.calls) continue;
    const double c = double(s.calls);
    fprintf(f, "| %s | %llu | %.2f | %.2f | %.2f | %.2f | %.2f |\n", s.name, (unsigned long long)s.calls,
            s.total_ns / c / 1e3, s.pre_ns / c / 1e3, s.launch_ns / c / 1e3, s.launches / c,
            (double(s.total_ns) - double(s.pre_ns) - double(s.launch_ns)) / c / 1e3);
  }
  if (f != stderr) fclose(f);
}
static bool host_prof_on() {
  static const bool on = [] {
    const bool v = getenv("MHTE_HOST_PROF") != nullptr && atoi(getenv("MHTE_HOST_PROF")) != 0;
    if (v) atexit(host_prof_dump);
    return v;
  }();
  return on;
}
struct HostProfScope {
  HostProfSec* s = nullptr;
  uint64_t t0 = 0;
  explicit HostProfScope(int which) {
    if (host_prof_on()) {
      s = &g_hp[which];
      t_hp = s;
      t0 = now_ns();
    }
  }
  void locked() { if (s) s->pre_ns += now_ns() - t0; }
  ~HostProfScope() {
    if (s) {
      s->total_ns += now_ns() - t0;
      ++s->calls;
      t_hp = nullptr;
    }
  }
};

#define LAUNCH_HOT(TAG, KERNEL, GRID, BLOCK, ST, ...)                                          \
  do {                                                                                         \
    if (g_prof.armed > 0) {                                                                    \
      const size_t i__ = g_prof.tag.size();                                                    \
      hipExtLaunchKernelGGL((KERNEL), dim3(GRID), dim3(BLOCK), 0, (ST), g_prof.ev[2 * i__],    \
                            g_prof.ev[2 * i__ + 1], 0, __VA_ARGS__);                           \
      g_prof.tag.push_back(TAG);                                                               \
      --g_prof.armed;                                                                          \
    } else if (t_hp) {                                                                         \
      const uint64_t t0__ = now_ns();                                                          \
      (KERNEL)<<<dim3(GRID), dim3(BLOCK), 0, (ST)>>>(__VA_ARGS__);                             \
      t_hp->launch_ns += now_ns() - t0__;                                                      \
      ++t_hp->launches;                                                                        \
    } else {                                                                                   \
      (KERNEL)<<<dim3(GRID), dim3(BLOCK), 0, (ST)>>>(__VA_ARGS__);                             \
    }                                                                                          \
  } while (0)

// tables alive in this process, by their device counter block AND a serial number: a dedup
// workspace that holds row reservations (ProbeOut.spec) gives their keys back when its batch is
// dropped — unless the table went first.  (The address alone is not an identity: a table created
// after another was closed gets the freed counter block back, and a workspace of the old table
// would take its reservations off the NEW table's counts — seen as a size of keys - 2^32.)
static std::mutex g_ctr_mu;
static std::vector<std::pair<const void*, uint64_t>> g_live_ctrs;
static uint64_t g_table_serial = 0;
static uint64_t register_counters(const void* p) {
  std::lock_guard<std::mutex> g(g_ctr_mu);
  g_live_ctrs.emplace_back(p, ++g_table_serial);
  return g_table_serial;
}
static void unregister_counters(const void* p, uint64_t serial) {
  std::lock_guard<std::mutex> g(g_ctr_mu);
  auto it = std::find(g_live_ctrs.begin(), g_live_ctrs.end(), std::make_pair(p, serial));
  if (it != g_live_ctrs.end()) g_live_ctrs.erase(it);
}
static bool table_counters_alive(const void* p, uint64_t serial) {
  std::lock_guard<std::mutex> g(g_ctr_mu);
  return std::find(g_live_ctrs.begin(), g_live_ctrs.end(), std::make_pair(p, serial)) != g_live_ctrs.end();
}

// ------------------------------------------------------------------------------------------ dedup ws
struct Table;
struct DedupWs {
  int device = 0;
  DevBuf<int64_t> hkey;
  DevBuf<uint32_t> hmin, hcnt, huidx, hcur, hstart, slot_of, seg_tmp, work, tile_a, tile_b, heavy,
      heavy_n;
  DevBuf<uint32_t> arrive;     // per-list arrival counters of the fused backward, kept zeroed
  size_t arrive_clean = 0;     // arrive[0, arrive_clean) is known to be zero
  int64_t last_n = -1;         // n of the most recent unique(): seg_u describes that batch
  uint32_t clean_cap = 0;  // hash scratch [0, clean_cap] is in the all-empty state
  DevBuf<float> part;
  DevBuf<uint32_t> last_u;

  DedupView view(int64_t n, hipStream_t st) {
    uint32_t C = 1u << std::max<uint32_t>(10, ceil_log2(uint64_t(2) * n));
    const int64_t* old_key = hkey.p;
    hkey.reserve(size_t(C) + 2);
    hmin.reserve(size_t(C) + 2);
    hcnt.reserve(size_t(C) + 2);
    huidx.reserve(size_t(C) + 2);
    hcur.reserve(size_t(C) + 2);
    hstart.reserve(size_t(C) + 2);
    slot_of.reserve(n + 1);
    seg_tmp.reserve(n + 1);
    work.reserve(2 * (size_t(n) / kChunk + size_t(n) / (kLightMax + 1) + 2));
    size_t ntiles = (n + kDdTile - 1) / kDdTile + 1;
    tile_a.reserve(ntiles);
    tile_b.reserve(ntiles);
    heavy.reserve(n / (kLightMax + 1) + 2);
    const uint32_t* old_ctr = heavy_n.p;
    heavy_n.reserve(4);
    DedupView d;
    d.hstart = hstart.p;
    d.hkey = hkey.p; d.hmin = hmin.p; d.hcnt = hcnt.p; d.huidx = huidx.p; d.hcur = hcur.p;
    d.slot_of = slot_of.p; d.tile_a = tile_a.p; d.tile_b = tile_b.p; d.heavy = heavy.p;
    d.heavy_n = heavy_n.p; d.cap_mask = C - 1; d.seg_tmp = seg_tmp.p; d.work = work.p;
    if (hkey.p != old_key || heavy_n.p != old_ctr || C > clean_cap) {
      // scratch was (re)allocated or never cleared this far: one clear pass; afterwards every
      // dedup leaves the slots it touched empty again (dd_finish_kernel)
      dd_clear_kernel<<<(C + 2 + 255) / 256, 256, 0, st>>>(d);
      clean_cap = C;
    }
    return d;
  }

  // the arrival counters of a batch of n positions: large enough and known to be zero (every kernel that
  // counts arrivals leaves them zero again)
  uint32_t* zeroed_arrive(size_t n, hipStream_t st) {
    const uint32_t* old = arrive.p;
    arrive.reserve(n + 2);
    if (arrive.p != old) arrive_clean = 0;
    if (arrive_clean < n + 2) {
      HIP_OK(hipMemsetAsync(arrive.p, 0, arrive.cap * sizeof(uint32_t), st));
      arrive_clean = arrive.cap;
    }
    return arrive.p;
  }
  // scratch of the fused backward (sum_apply_kernel): block partial rows + zeroed arrival counters
  void backward_scratch(int64_t n, uint32_t dim, uint32_t nblk_b, hipStream_t st) {
    part.reserve(size_t(nblk_b) * 2 * dim + 16);
    zeroed_arrive(size_t(n), st);
  }

  void unique(const int64_t* ids, int64_t n, int64_t* uids, uint32_t* inverse, uint32_t* seg_off,
              uint32_t* seg_pos, uint32_t* n_unique_dev, hipStream_t st) {
    if (n < 0 || n > (int64_t(1) << 31) - 4096)
      throw Error(MHTE_INVALID_ARGUMENT, "unique: n out of range");
    last_n = n;
    if (n == 0) {
      HIP_OK(hipMemsetAsync(n_unique_dev, 0, sizeof(uint32_t), st));
      HIP_OK(hipMemsetAsync(seg_off, 0, sizeof(uint32_t), st));
      return;
    }
    DedupView d = view(n, st);
    const uint32_t un = uint32_t(n);
    const uint32_t ntiles = (un + kDdTile - 1) / kDdTile;
    dd_insert_kernel<<<(un + kDdBlock - 1) / kDdBlock, kDdBlock, 0, st>>>(d, ids, un);
    dd_tile_kernel<<<ntiles, 256, 0, st>>>(d, un);
    dd_emit_kernel<<<ntiles, 256, 0, st>>>(d, ids, un, uids, seg_off, n_unique_dev);
    dd_place_kernel<<<(un + kDdBlock - 1) / kDdBlock, kDdBlock, 0, st>>>(d, un, seg_off, inverse);
    const uint32_t nb_rank = (un + 1023) / 1024;
    const uint32_t hgrid = std::min<uint32_t>(256, un / (kLightMax + 1) + 1);
    static const bool split_finish = getenv("MHTE_SPLIT_FINISH") != nullptr;  // profiling aid
    if (split_finish) {
      dd_finish_kernel<<<nb_rank, 1024, 0, st>>>(d, un, nb_rank, inverse, seg_off, seg_off + 1,
                                                 seg_pos, 1, n_unique_dev);
      dd_finish_kernel<<<hgrid, 1024, 0, st>>>(d, un, 0, inverse, seg_off, seg_off + 1, seg_pos, 1,
                                               n_unique_dev);
    } else {
      dd_finish_kernel<<<nb_rank + hgrid, 1024, 0, st>>>(d, un, nb_rank, inverse, seg_off,
                                                         seg_off + 1, seg_pos, 1, n_unique_dev);
    }
    hipError_t le = hipGetLastError();
    if (le != hipSuccess) {
      clean_cap = 0;  // scratch state unknown: force a clear next time
      HIP_OK(le);
    }
  }

  // --- run dedup of the pipelined step (mhte_step_kernels.h); own scratch, independent of the
  // list-building dedup above
  DevBuf<RdSlot> r_hs;
  DevBuf<int64_t> r_btab_key;
  DevBuf<uint32_t> r_hlist, r_uslot, r_ucnt, r_upos, r_btab_val, r_item_runs, r_ctr;
  DevBuf<uint16_t> r_seg;
  DevBuf<ItemHdr> r_item_hdr;
  DevBuf<uint32_t> r_cursor;   // shard packing cursors
  DevBuf<URec> r_urec;         // ProbeOut of the numbered batch: per unique index, what the update
                               // needs in one load — incl. the row handle / slot of an id the table
                               // held when the batch was numbered, or a row reserved for it
  void probe_out_reserve(int64_t n) {
    const URec* old = r_urec.p;
    r_urec.reserve(size_t(n) + 1);
    // (the update reads records past the unique count before it knows the count: never-written
    // memory must at least be well-formed)
    if (r_urec.p != old) HIP_OK(hipMemset(r_urec.p, 0, r_urec.cap * sizeof(URec)));
  }
  uint32_t r_clean_cap = 0;  // run scratch [0, r_clean_cap] is all-empty
  int r_stage = 0;           // 0 idle, 1 dedup enqueued, 2 work list enqueued (ready for apply)
  RunView rv{};

  // --- the probe of the numbered batch.  A probe (r_urec) belongs to ONE table, named by its counter
  // block AND its serial number: for any other — another table, or the same one after a clear — it is
  // void.  Its row reservations go back to that table when the batch is dropped instead of applied,
  // unless the table went first.  r_stage and the four fields below are written by the transitions
  // that follow and by begin_run_dedup / build_work_list, nowhere else.
 private:
  bool r_hints = false;            // r_urec describes the numbered batch
  bool r_prealloc = false;         // ... and holds row reservations for it
  Counters* r_res_ctr = nullptr;   // the table the probe is of ...
  uint64_t r_res_serial = 0;       // ... and its serial number (register_counters)
 public:
  bool probed() const { return r_hints; }
  bool holds_reservations() const { return r_prealloc && r_stage == 2 && r_res_ctr; }
  inline bool probe_is_of(const Table& tb) const;
  // the batch was numbered and probed against tb (reserved: with row reservations): ready for the apply
  inline void adopt_probe(const Table& tb, bool reserved);
  // a probe of another table, or of this one before it was cleared: its row handles and reservations
  // mean nothing to the table about to be updated — forget them, in the heavy items' headers as well
  void void_probe(hipStream_t st) {
    r_hints = false;
    r_prealloc = false;
    r_res_ctr = nullptr;
    HIP_OK(hipMemsetAsync(rv.ctr + 3, 0, sizeof(uint32_t), st));   // (its reservation count)
    if (r_stage == 2) rd_items_unhint_kernel<<<8, 256, 0, st>>>(rv);
  }
  // the apply takes the probe: true if rows were reserved (and their room made) when it was taken
  bool consume_probe() {
    const bool prealloc = r_prealloc;
    r_prealloc = false;
    r_hints = false;
    r_res_ctr = nullptr;
    return prealloc;
  }
  void applied() { r_stage = 0; }   // the apply leaves the scratch all-empty
  // reservations of a numbered batch that is dropped instead of applied: the keys go back
  void drop_reservations(hipStream_t st) {
    if (holds_reservations() && table_counters_alive(r_res_ctr, r_res_serial))
      // (the count is the workspace's own counter, ctr[0] — the user's n_unique buffer of the dropped batch
      // may be gone by now)
      rd_unreserve_kernel<<<32, 256, 0, st>>>(r_urec.p, rv.ctr, rv.n, r_res_ctr);
    (void)consume_probe();
  }

  // items of a list of c occurrences < c / target + 1 (rd_item_blocks), lists > kLightMax
  static uint32_t max_items(int64_t n) {
    return uint32_t(2 * n / item_target() + n / (kStepLightMax + 1) + 2);
  }
  static uint32_t item_target() { return kItemTarget; }
  // Entries of the preallocated item list.  The item workgroups (rd_apply_role, rd_gather_role) fetch entry w
  // — header and run descriptors — BEFORE they compare w with the item count, and w advances by the number of
  // item workgroups, which is at most max_items(n): the last fetch of a workgroup lies below items + max_items.
  // (A list of max_items entries was read up to 61 KB past its end by a batch of 300 lists of 33 in 9900
  // positions — 300 items, 320 item workgroups, 379 entries: an illegal memory access,
  // tests/test_run_dedup_forms_gpu.py "edge-300x33".)
  static size_t item_list_entries(int64_t n) { return 2 * size_t(max_items(n)); }

  // Arguments of a run dedup of ids[0, n), n <= 65 536; the caller enqueues rd_dedup (on its own or
  // inside step_fwd).  A dedup that was never built leaves the scratch dirty: clear first (the
  // build role resets the scratch; the apply only consumes the dense arrays).
  RunView begin_run_dedup(const int64_t* ids, int64_t n, int64_t* uids, uint32_t* n_unique_dev,
                          hipStream_t st) {
    if (n <= 0 || n > int64_t(kRdMaxBlocks) * kRdBlock)
      throw Error(MHTE_INVALID_ARGUMENT, "step: batch must have 1.." +
                                             std::to_string(kRdMaxBlocks * kRdBlock) + " ids");
    drop_reservations(st);
    const uint32_t C = 1u << std::max<uint32_t>(10, ceil_log2(uint64_t(2) * n));
    const RdSlot* old_key = r_hs.p;
    const uint32_t* old_ctr = r_ctr.p;
    r_hs.reserve(size_t(C) + 2);
    r_hlist.reserve((size_t(C) + 2) * kLightMax);
    r_ctr.reserve(4);
    const uint32_t nblk = uint32_t((n + kRdBlock - 1) / kRdBlock);
    r_uslot.reserve(size_t(n) + 1);
    r_ucnt.reserve(size_t(n) + 1);
    r_upos.reserve(size_t(n) + 1);
    r_btab_key.reserve(size_t(nblk) * kRdStride);
    r_btab_val.reserve(size_t(nblk) * kRdStride);
    r_seg.reserve(size_t(nblk) * kRdBlock);
    r_item_hdr.reserve(item_list_entries(n));
    r_item_runs.reserve(item_list_entries(n) * 64);
    RunView d{};
    d.hs = r_hs.p; d.hlist = r_hlist.p; d.cap_mask = C - 1;
    d.uslot = r_uslot.p; d.ucnt = r_ucnt.p; d.upos = r_upos.p; d.btab_key = r_btab_key.p; d.btab_val = r_btab_val.p; d.seg = r_seg.p;
    d.item_hdr = r_item_hdr.p; d.item_runs = r_item_runs.p; d.ctr = r_ctr.p;
    d.ids = ids; d.n = uint32_t(n); d.nblk = nblk; d.uids = uids; d.n_unique = n_unique_dev;
    d.item_target = item_target();
    if (r_hs.p != old_key || r_ctr.p != old_ctr || C > r_clean_cap || r_stage == 1) {
      rd_clear_kernel<<<(C + 2 + 255) / 256, 256, 0, st>>>(d);
      r_clean_cap = C;
    }
    rv = d;
    r_stage = 1;
    return d;
  }
  // workgroups of the build role: one trip of 256 slots per wavefront, at most 128 workgroups
  static uint32_t build_blocks(const RunView& d) {
    const uint32_t trips = (d.cap_mask + 2u + 64u * kBuildSlotsPerLane - 1) / (64u * kBuildSlotsPerLane);
    return std::max<uint32_t>(1, std::min<uint32_t>(128, (trips + 3) / 4));
  }
  // unique numbering + heavy work list of the deduplicated batch on its own (normally it rides in
  // step_bwd)
  void build_work_list(hipStream_t st) {
    if (r_stage != 1) return;
    rd_build_kernel<<<build_blocks(rv), 256, 0, st>>>(rv, uint32_t(kStepLightMax));
    HIP_OK(hipGetLastError());
    r_stage = 2;
  }

  // Unordered dedup (3 launches): unique ids in unspecified order, list bounds per unique index,
  // positions grouped by list (lists of > kLightMax positions ordered, shorter ones not).
  void unique_unordered(const int64_t* ids, int64_t n, int64_t* uids, uint32_t* inverse,
                        uint32_t* lst_start, uint32_t* lst_end, uint32_t* seg_pos,
                        uint32_t* n_unique_dev, hipStream_t st) {
    if (n < 0 || n > (int64_t(1) << 31) - 4096)
      throw Error(MHTE_INVALID_ARGUMENT, "unique: n out of range");
    last_n = n;
    if (n == 0) {
      HIP_OK(hipMemsetAsync(n_unique_dev, 0, sizeof(uint32_t), st));
      return;
    }
    DedupView d = view(n, st);
    const uint32_t un = uint32_t(n);
    const uint32_t nb = (un + kDdBlock - 1) / kDdBlock;
    LAUNCH_HOT(kTagDedup, dd_insert_fast_kernel, nb, kDdBlock, st, d, ids, un, uids);
    LAUNCH_HOT(kTagDedup, dd_place_fast_kernel, nb, kDdBlock, st, d, un, inverse, lst_start, lst_end,
               seg_pos);
    const uint32_t nb_rank = (un + 1023) / 1024;
    const uint32_t hgrid = std::min<uint32_t>(256, un / (kLightMax + 1) + 1);
    LAUNCH_HOT(kTagDedup, dd_finish_kernel, nb_rank + hgrid, 1024, st, d, un, nb_rank, inverse,
               lst_start, lst_end, seg_pos, 0, n_unique_dev);
    hipError_t le = hipGetLastError();
    if (le != hipSuccess) {
      clean_cap = 0;
      HIP_OK(le);
    }
  }
};

// pick lanes-per-id and vector width for a row of `dim` floats
struct Shape {
  int G;
  int VEC;
};
static Shape pick_shape(uint32_t dim, bool vec_ok) {
  Shape s;
  s.VEC = vec_ok ? 4 : 1;
  uint32_t units = (dim + s.VEC - 1) / s.VEC;
  uint32_t g = 8;
  while (g < units && g < 64) g <<= 1;
  s.G = int(g);
  return s;
}
static inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

// A lane shape as compile-time constants: for_shape(sh, [&](auto g, auto v) { ... kernel<decltype(g)::value,
// decltype(v)::value> ... }) runs the generic lambda's instance for sh — every launch that is compiled per
// (G, VEC) selects its kernel here.  with_flag does the same for one run-time flag.
// MHTE_DEV_FAST (development builds, scripts/dev_build.sh): only the dim-64 float4 shape is
// instantiated, which cuts the compile from minutes to well under one; every other shape throws.
template <int N>
using Const = std::integral_constant<int, N>;
template <class F>
static inline void for_shape(Shape sh, F&& f) {
#ifdef MHTE_DEV_FAST
  if (sh.VEC != 4 || sh.G != 16) throw Error(MHTE_INTERNAL, "MHTE_DEV_FAST build: only G = 16, VEC = 4");
  f(Const<16>{}, Const<4>{});
#else
  auto for_g = [&](auto v) {
    switch (sh.G) {
      case 8: f(Const<8>{}, v); break;
      case 16: f(Const<16>{}, v); break;
      case 32: f(Const<32>{}, v); break;
      default: f(Const<64>{}, v); break;
    }
  };
  if (sh.VEC == 4) for_g(Const<4>{});
  else for_g(Const<1>{});
#endif
}
template <class F>
static inline auto with_flag(bool on, F&& f) {
  return on ? f(std::true_type{}) : f(std::false_type{});
}

// the instance of a retriever kernel for Table::retriever_instance()'s answer (not kRtRaw)
template <class F>
static inline F pick_rt(int rt, F fake_quant, F hash_net, F mixed) {
  return rt == kRtFakeQuant ? fake_quant : (rt == kRtHashNet ? hash_net : mixed);
}

// MHTE_EXACT_ORDER in the step kernels (single-table and multi-table step alike): lists of <= kStepLightMax
// occurrences are summed in occurrence order by the id-major groups in every mode; the heavy ones get their
// strictly sequential sums from a launch in front of the update (`pre`: a workgroup streams a list's rows
// through LDS, one wavefront adds them in order) and the item workgroups only apply them.  `walk`: round 5's
// form, one lane group walking each list — rows wider than 256 floats, or MHTE_EXACT_WALK=1 (A/B; 4.8 ms per
// step at Zipf(1.2)).
struct ExactMode {
  bool pre, walk;
  uint32_t light_max() const { return walk ? 0xffffffffu : uint32_t(kStepLightMax); }
};
static ExactMode exact_mode(bool exact_order, uint32_t dim) {
  static const bool force_walk = getenv("MHTE_EXACT_WALK") != nullptr && atoi(getenv("MHTE_EXACT_WALK")) != 0;
  const bool pre = exact_order && !force_walk && dim <= 256u;
  return ExactMode{pre, exact_order && !pre};
}

// ------------------------------------------------------------------------------------------ clock
// seconds on a monotonic clock (+ the test hook's offset): the eviction cadence
static std::atomic<double> g_clock_offset{0.0};
static double lib_now() {
  return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count() +
         g_clock_offset.load();
}

// ------------------------------------------------------------------------------------------ table
// global_step of the API call being served on this thread (every entry point is synchronous on
// its caller's thread); read by Table::upsert for the one optimizer that uses it (batch softmax)
static thread_local int64_t t_global_step = 0;

// Host-side bound on how full the head split of a sliding filter can be (the role keys_upper plays for
// the table's doubling): every consulting launch adds at most its id count; the window can only have to
// move once the bound reaches the split's capacity, and only then do filter_advance_kernel /
// filter_clear_kernel follow the launch — and the true count is fetched (one asynchronous 16-byte copy of
// the state's first words, where filter_advance_kernel leaves the head split's count; polled, never waited
// for) to start the bound over.  A launch that does not say how many ids it had, or one on another stream
// than the fetch in flight, voids that fetch (its count may or may not include the launch's ids).  Launches recorded into a hipGraph are replayed
// without the host seeing them: a filter that was ever consulted under capture keeps the two launches
// behind every consulting launch, as round 4 did everywhere.
struct FilterBudget {
  std::mutex mu;
  uint32_t split_cap = 0;
  uint64_t head_upper = 0;
  uint64_t adds_since_fetch = 0;
  uint64_t gen = 0, fetch_gen = 0;
  bool known = true, fetching = false, every_launch = false;
  uint32_t* h_state = nullptr;      // pinned: head, head_increment, clear_req, head_elements
  hipStream_t fetch_stream = nullptr;
  hipEvent_t ev = nullptr;
  uint64_t skipped = 0, maintained = 0;   // (statistics)
  FilterBudget() {
    static const bool always = getenv("MHTE_FILTER_MAINTAIN_ALWAYS") != nullptr;   // (A/B: round 4's behaviour)
    every_launch = always;
  }
  ~FilterBudget() {
    if (ev) (void)hipEventDestroy(ev);
    if (h_state) (void)hipHostFree(h_state);
  }
  void invalidate() {   // the device state was rewritten (restore)
    std::lock_guard<std::mutex> g(mu);
    known = false;
    ++gen;
  }
  bool due(uint64_t adds, hipStream_t st) {
    std::lock_guard<std::mutex> g(mu);
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(st, &cs) == hipSuccess && cs != hipStreamCaptureStatusNone) every_launch = true;
    if (every_launch) return true;
    if (fetching && (adds == ~0ull || st != fetch_stream)) {
      ++gen;           // (the fetch in flight cannot be trusted to count this launch)
      known = false;
    }
    if (fetching && hipEventQuery(ev) == hipSuccess) {
      fetching = false;
      if (fetch_gen == gen) {
        head_upper = uint64_t(h_state[3]) + adds_since_fetch;
        known = true;
      }
    }
    if (adds == ~0ull) {
      known = false;   // (a launch that does not say how many ids it had)
    } else {
      head_upper += adds;
      adds_since_fetch += adds;
    }
    const bool need = !known || fetching || head_upper + 1u >= uint64_t(split_cap);
    ++(need ? maintained : skipped);
    return need;
  }
  void refetch(const FilterState* d_state, hipStream_t st) {
    std::lock_guard<std::mutex> g(mu);
    if (every_launch || fetching) return;
    if (!h_state && hipHostMalloc(reinterpret_cast<void**>(&h_state), 16) != hipSuccess) {
      every_launch = true;
      return;
    }
    if (!ev && hipEventCreateWithFlags(&ev, hipEventDisableTiming) != hipSuccess) {
      every_launch = true;
      return;
    }
    static_assert(offsetof(FilterState, head_elements) == 12, "the fetched words");
    if (hipMemcpyAsync(h_state, d_state, 16, hipMemcpyDeviceToHost, st) != hipSuccess ||
        hipEventRecord(ev, st) != hipSuccess) {
      every_launch = true;
      return;
    }
    fetching = true;
    fetch_stream = st;
    fetch_gen = gen;
    adds_since_fetch = 0;
  }
};

struct Table {
  std::string name;
  int device = 0;
  int num_cus = 256;   // compute units of the device (residency budget of the step launches)
  std::vector<mhte_segment_config> segs;
  uint32_t dim = 0, row_floats = 0, nseg = 0;
  bool vec_ok = false;  // every segment boundary (weights and state) is a multiple of 4 floats
  double max_load = 0.5;
  TableView view{};
  uint32_t hp = 0;
  Bucket* buckets = nullptr;
  std::vector<float*> chunks;
  float** d_chunks = nullptr;
  uint32_t max_chunks = 0;
  uint32_t chunk_shift = 0;
  Counters* ctr = nullptr;
  uint64_t ctr_serial = 0;      // identity of this table's counter block (register_counters)
  Counters* h_ctr = nullptr;  // pinned mirror
  uint64_t keys_upper = 0, rows_upper = 0;
  int64_t max_update_ts = 0;
  bool count_hits = false;  // lookup hit counter (the reference only emits hit rate for serving tables)
  int64_t default_expire_days = 36500;
  std::vector<int64_t> expire_slots;
  std::vector<int32_t> expire_days;
  DevBuf<int64_t> d_expire_slots;
  DevBuf<int32_t> d_expire_days;
  DevBuf<uint32_t> pending;         // displacement list: one word per entry (index into the op's ids); two words
                                    // in the segment and shard lists (SegUpsertArgs, ShardOwnerArgs)
  DevBuf<uint32_t> skip;            // first admitted occurrence of deferred ids (admission filter)
  // admission: per-feature-slot occurrence thresholds (SlotOccurrenceThresholdConfig) + the filter
  int32_t occ_default = 0;
  std::vector<int64_t> occ_slots;
  std::vector<int32_t> occ_thr;
  DevBuf<int64_t> d_occ_slots;
  DevBuf<int32_t> d_occ_thr;
  bool has_group_opt = false;       // a segment uses GroupAdaGrad (picks the kernel instantiation)
  // Segment retrievers (quantization-aware training, mhte_qat_kernels.h; mhte_table_set_retriever).
  // params: fake quant {r}; hash net {step_size, init_scale, max_scale, amplitude}.
  struct Retriever {
    int32_t type = kRetRaw;
    float p[4] = {0.f, 0.f, 0.f, 0.f};
  };
  std::vector<Retriever> retrievers;   // one per segment
  bool has_retriever = false;          // a segment's retriever is not the raw one
  bool has_hash_net = false;           // ... is HashNet: the update kernels run its Backward
  float* d_scale = nullptr;            // [kMaxSegments] live HashNet scales (allocated with the first HashNet segment)
  static const char* retriever_name(int32_t type) {
    return type == kRetFakeQuant ? "fake_quant_r8" : (type == kRetHashNet ? "hash_net" : "raw");
  }
  // the fused step kernels and the step objects read rows raw: a table with a retriever is refused there, by name
  void refuse_retriever(const std::string& what) const {
    for (uint32_t k = 0; k < uint32_t(retrievers.size()); ++k)
      if (retrievers[k].type != kRetRaw)
        throw Error(MHTE_INVALID_ARGUMENT,
                    what + ": table " + name + " has a " + retriever_name(retrievers[k].type) + " retriever on segment " +
                        std::to_string(k) + "; the fused step kernels read rows raw — such a table takes the op-level "
                        "lookup and update (mhte_lookup / mhte_table_lookup_n, mhte_optimize / mhte_table_optimize_n / "
                        "mhte_table_sum_optimize_n)");
  }
  void set_retriever(int32_t k, int32_t type, const float* params, int32_t n_params) {
    if (k < 0 || k >= int32_t(nseg))
      throw Error(MHTE_INVALID_ARGUMENT, "set_retriever: table " + name + " has no segment " + std::to_string(k));
    Retriever r;
    r.type = type;
    if (type == kRetFakeQuant) {
      if (!params || n_params != 1)
        throw Error(MHTE_INVALID_ARGUMENT, "set_retriever: fake_quant_r8 takes 1 parameter {r}");
      if (!(params[0] > 0.f) || std::isinf(params[0]))
        throw Error(MHTE_INVALID_ARGUMENT, "set_retriever: fake_quant_r8 needs a finite r > 0");
      r.p[0] = params[0];
    } else if (type == kRetHashNet) {
      if (!params || n_params != 4)
        throw Error(MHTE_INVALID_ARGUMENT,
                    "set_retriever: hash_net takes 4 parameters {step_size, init_scale, max_scale, amplitude}");
      // (global_step % step_size: the reference divides by zero, hash_net_quantizer.h:47)
      if (!(params[0] >= 1.f)) throw Error(MHTE_INVALID_ARGUMENT, "set_retriever: hash_net needs step_size > 0");
      // (it travels as a float: whole numbers up to 2^24 are exact, anything else would be another schedule)
      if (params[0] > 16777216.f || params[0] != floorf(params[0]))
        throw Error(MHTE_INVALID_ARGUMENT, "set_retriever: hash_net step_size must be a whole number <= 2^24");
      if (view.seg[k].opt == kOptGroupAdagrad)
        throw Error(MHTE_INVALID_ARGUMENT, "set_retriever: hash_net on a group_adagrad segment is not implemented "
                                           "(the whole-segment update has no per-element Backward)");
      for (int i = 0; i < 4; ++i) r.p[i] = params[i];
    } else if (type != kRetRaw) {
      throw Error(MHTE_INVALID_ARGUMENT, "set_retriever: unknown retriever type " + std::to_string(type));
    }
    finish_pending(nullptr);
    if (type == kRetHashNet && !d_scale) {
      HIP_OK(hipMalloc(&d_scale, sizeof(float) * kMaxSegments));
      HIP_OK(hipMemset(d_scale, 0, sizeof(float) * kMaxSegments));
    }
    // (the setter has no stream: the device is drained first, so the change is behind all enqueued work of
    // every stream, non-blocking ones included, and in place at return)
    HIP_OK(hipDeviceSynchronize());
    if (type == kRetHashNet) HIP_OK(hipMemcpy(d_scale + k, &r.p[1], sizeof(float), hipMemcpyHostToDevice));
    retrievers[k] = r;
    has_retriever = has_hash_net = false;
    for (const Retriever& x : retrievers) {
      has_retriever = has_retriever || x.type != kRetRaw;
      has_hash_net = has_hash_net || x.type == kRetHashNet;
    }
  }
  // The descriptors of a launch.  global_step (updates): the candidate scale of every HashNet segment whose
  // step_size divides it (HashNetQuantizer::Backward, hash_net_quantizer.h:47-50: powf, then the cap).
  RetrieverArgs retriever_args(bool update, int64_t global_step) const {
    RetrieverArgs ra{};
    ra.nseg = nseg;
    ra.scale = d_scale;
    for (uint32_t k = 0; k < nseg; ++k) {
      const Retriever& r = retrievers[k];
      ra.type[k] = r.type;
      ra.w_off[k] = uint32_t(view.seg[k].w_off);
      if (r.type == kRetFakeQuant) {   // FakeQuantizer's constructor, fake_quantizer.h:28-29
        ra.p0[k] = r.p[0] / 128;
        ra.p1[k] = ra.p0[k] / 2;
      } else if (r.type == kRetHashNet) {
        ra.p0[k] = r.p[3];
        if (update && global_step % int64_t(r.p[0]) == 0) {
          ra.cand[k] = std::min(r.p[1] * powf(1.f + 0.005f * static_cast<float>(global_step), 0.5f), r.p[2]);
          ra.update |= 1u << k;
        }
      }
    }
    return ra;
  }
  // the kernel instance the table's retrievers select: lookups, and (hash net only) updates
  int retriever_instance(bool update) const {
    if (update ? !has_hash_net : !has_retriever) return kRtRaw;
    if (nseg == 1) return retrievers[0].type == kRetFakeQuant ? kRtFakeQuant : kRtHashNet;
    return kRtMixed;
  }
  uint32_t* flt_slots = nullptr;   // owned by the mhte_hash_filter attached to the MultiHashTable
  uint64_t flt_total = 0;
  uint32_t* flt_state = nullptr;
  uint32_t flt_nsplit = 0, flt_stride = 0, flt_cap = 0;
  FilterBudget* flt_budget = nullptr;   // the filter's host-side bound on its head split (sliding filters)
  // after a launch that consulted the filter: move the sliding window on if the head split filled
  // up (filter_advance_kernel) and clear the split that becomes the look-ahead one.  `adds_upper`: how
  // many ids the launch can have added to the filter at most (its id count); with it the two launches
  // are skipped while the head split cannot be full yet (FilterBudget) — they were 2 of the filtered
  // step's 4 launches and did nothing in all but one step of a few hundred.
  void filter_maintain(hipStream_t st, uint64_t adds_upper = ~0ull) {
    if (!flt_slots) return;
    const bool sliding = flt_nsplit != 0u && flt_budget != nullptr;
    if (sliding && !flt_budget->due(adds_upper, st)) return;
    filter_advance_kernel<<<1, 64, 0, st>>>(view);
    filter_clear_kernel<<<256, 256, 0, st>>>(view);
    if (sliding) flt_budget->refetch(reinterpret_cast<const FilterState*>(flt_state), st);
  }
  // in-op grouping scratch (ids not declared unique)
  DedupWs dd;
  DevBuf<int64_t> g_uids;
  DevBuf<uint32_t> g_inverse, g_seg_off, g_seg_pos, g_nu;
  std::mutex mu;

  ~Table() {
    (void)hipSetDevice(device);
    (void)hipDeviceSynchronize();
    if (buckets) (void)hipFree(buckets);
    for (float* c : chunks) (void)hipFree(c);
    if (d_chunks) (void)hipFree(d_chunks);
    if (ctr) {
      unregister_counters(ctr, ctr_serial);
      (void)hipFree(ctr);
    }
    if (h_ctr) (void)hipHostFree(h_ctr);
    if (d_scale) (void)hipFree(d_scale);
  }

  void init(const mhte_table_config& c, int dev) {
    device = dev;
    {
      int cus = 0;
      if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && cus > 0)
        num_cus = cus;
    }
    name = c.name ? c.name : "";
    if (c.n_segments < 1 || c.n_segments > kMaxSegments)
      throw Error(MHTE_INVALID_ARGUMENT, "table " + name + ": n_segments must be 1.." +
                                             std::to_string(kMaxSegments));
    segs.assign(c.segments, c.segments + c.n_segments);
    nseg = c.n_segments;
    retrievers.assign(nseg, Retriever{});
    dim = 0;
    for (auto& s : segs) {
      if (s.dim_size <= 0) throw Error(MHTE_INVALID_ARGUMENT, "segment dim_size must be > 0");
      const int32_t base_opt = s.opt_type & ~int32_t(MHTE_OPT_FLAG_STOCHASTIC_ROUNDING_FP16);
      if (base_opt < MHTE_OPT_SGD || base_opt >= kOptCount)
        throw Error(MHTE_INVALID_ARGUMENT, "unknown optimizer type " + std::to_string(s.opt_type));
      if (base_opt != s.opt_type && base_opt == MHTE_OPT_GROUP_ADAGRAD)
        throw Error(MHTE_INVALID_ARGUMENT, "stochastic_rounding_float16 on a group_adagrad segment is not implemented");
      if (s.init_type < MHTE_INIT_ZEROS || s.init_type > MHTE_INIT_RANDOM_UNIFORM)
        throw Error(MHTE_INVALID_ARGUMENT, "unknown initializer type");
      if (base_opt == MHTE_OPT_BATCH_SOFTMAX && s.dim_size != 1)  // batch_softmax_optimizer.cc:29
        throw Error(MHTE_INVALID_ARGUMENT, "a batch softmax segment has dim_size 1");
      if (base_opt == MHTE_OPT_GROUP_ADAGRAD) has_group_opt = true;
      dim += s.dim_size;
    }
    // row = float num[dim] | ctx(seg0) | ctx(seg1) ... (entry_accessor.cc:113-114)
    uint32_t w = 0, st = dim;
    vec_ok = true;
    for (uint32_t i = 0; i < nseg; ++i) {
      SegDesc& d = view.seg[i];
      d.dim = segs[i].dim_size;
      d.w_off = w;
      d.st_off = st;
      d.opt = segs[i].opt_type & ~int32_t(MHTE_OPT_FLAG_STOCHASTIC_ROUNDING_FP16);
      d.sr16 = (segs[i].opt_type & MHTE_OPT_FLAG_STOCHASTIC_ROUNDING_FP16) ? 1 : 0;
      for (int k = 0; k < 8; ++k) d.p[k] = segs[i].opt_params[k];
      d.init = segs[i].init_type;
      d.init_value = segs[i].init_value;
      d.init_value2 = segs[i].init_value2;
      if ((d.dim % 4) || (d.w_off % 4) || (d.st_off % 4)) vec_ok = false;
      w += d.dim;
      st += uint32_t(opt_state_floats(d.opt, d.dim));
    }
    row_floats = st;
    if (row_floats % 4) vec_ok = false;
    max_load = (c.max_load_factor > 0.f && c.max_load_factor <= 1.f) ? c.max_load_factor : 0.5;
    // (0 = unset -> the proto default; a TTL of zero days — everything expires at the next save /
    // scan, hash_table_ops_test.py:381-395 — is written as a negative value)
    default_expire_days = c.default_expire_days > 0 ? c.default_expire_days : (c.default_expire_days < 0 ? 0 : 36500);
    if (c.n_slot_expire > 0) {
      expire_slots.assign(c.expire_slots, c.expire_slots + c.n_slot_expire);
      expire_days.assign(c.expire_days, c.expire_days + c.n_slot_expire);
      d_expire_slots.reserve(expire_slots.size());
      d_expire_days.reserve(expire_days.size());
      HIP_OK(hipMemcpy(d_expire_slots.p, expire_slots.data(), expire_slots.size() * 8,
                       hipMemcpyHostToDevice));
      HIP_OK(hipMemcpy(d_expire_days.p, expire_days.data(), expire_days.size() * 4,
                       hipMemcpyHostToDevice));
    }
    occ_default = c.default_occurrence_threshold;
    if (c.n_slot_occurrence > 0) {
      occ_slots.assign(c.occurrence_slots, c.occurrence_slots + c.n_slot_occurrence);
      occ_thr.assign(c.occurrence_thresholds, c.occurrence_thresholds + c.n_slot_occurrence);
      d_occ_slots.reserve(occ_slots.size());
      d_occ_thr.reserve(occ_thr.size());
      HIP_OK(hipMemcpy(d_occ_slots.p, occ_slots.data(), occ_slots.size() * 8, hipMemcpyHostToDevice));
      HIP_OK(hipMemcpy(d_occ_thr.p, occ_thr.data(), occ_thr.size() * 4, hipMemcpyHostToDevice));
    }
    evict_enabled = c.enable_feature_eviction != 0;
    evict_every_s = (c.feature_evict_every_n_hours > 0 ? c.feature_evict_every_n_hours : 240) * 3600.0;
    last_evict = last_evict_check = lib_now();
    hp = reserve_calc(c.initial_capacity ? c.initial_capacity : 1);
    if (hp > 34) throw Error(MHTE_INVALID_ARGUMENT, "initial_capacity too large");
    alloc_buckets(hp, &buckets, nullptr);
    // row slabs
    const size_t row_bytes = size_t(row_floats) * 4;
    if (c.reserve_rows > 0) {
      chunk_shift = std::max<uint32_t>(10, ceil_log2(c.reserve_rows));
    } else {
      uint32_t s = 12;
      while (s < 24 && (row_bytes << (s + 1)) <= (size_t(64) << 20)) ++s;
      chunk_shift = s;
    }
    if (chunk_shift > 32) throw Error(MHTE_INVALID_ARGUMENT, "reserve_rows too large");
    max_chunks = chunk_shift >= 32 ? 1u : std::min<uint64_t>(uint64_t(1) << (32 - chunk_shift), 65536);
    HIP_OK(hipMalloc(&d_chunks, sizeof(float*) * max_chunks));
    HIP_OK(hipMemset(d_chunks, 0, sizeof(float*) * max_chunks));
    HIP_OK(hipMalloc(&ctr, sizeof(Counters)));
    HIP_OK(hipMemset(ctr, 0, sizeof(Counters)));
    ctr_serial = register_counters(ctr);
    HIP_OK(hipHostMalloc(&h_ctr, sizeof(Counters), hipHostMallocDefault));
    memset(h_ctr, 0, sizeof(Counters));
    add_chunk();
    refresh_view();
  }

  void alloc_buckets(uint32_t new_hp, Bucket** out, hipStream_t st) {
    const uint64_t nb = uint64_t(1) << new_hp;
    HIP_OK(hipMalloc(out, nb * sizeof(Bucket)));
    clear_buckets_kernel<<<dim3(uint32_t((nb + 255) / 256)), 256, 0, st>>>(*out, nb);
    HIP_OK(hipGetLastError());
  }

  void add_chunk() {
    if (chunks.size() >= max_chunks)
      throw Error(MHTE_RESOURCE_EXHAUSTED, "table " + name + ": row handle space exhausted");
    float* p = nullptr;
    HIP_OK(hipMalloc(&p, (size_t(1) << chunk_shift) * row_floats * sizeof(float)));
    chunks.push_back(p);
    HIP_OK(hipMemcpy(d_chunks + (chunks.size() - 1), &p, sizeof(float*), hipMemcpyHostToDevice));
  }

  // bumped whenever `view` (or count_hits) changes: holders of device copies re-upload
  uint64_t view_version = 0;
  // bumped by everything that may insert, move, or delete a bucket entry (updates, displacement,
  // eviction, doubling, restore): a (row handle, bucket slot) resolved before stays valid only
  // while this stands still (the multi-table step's forward -> backward hints)
  uint64_t mut_epoch = 1;
  void refresh_view() {
    ++view_version;
    view.buckets = buckets;
    view.chunk0 = chunks.empty() ? nullptr : chunks[0];
    view.chunks = d_chunks;
    view.ctr = ctr;
    view.hp = hp;
    view.chunk_shift = chunk_shift;
    view.row_floats = row_floats;
    view.dim = dim;
    view.nseg = nseg;
    view.trace = nullptr;
    view.flt_slots = flt_slots;
    view.flt_total = flt_total;
    view.flt_state = flt_state;
    view.flt_nsplit = flt_nsplit;
    view.flt_stride = flt_stride;
    view.flt_cap = flt_cap;
    view.occ_default = occ_default;
    view.occ_n = int32_t(occ_slots.size());
    view.occ_slots = d_occ_slots.p;
    view.occ_thr = d_occ_thr.p;
  }

  void sync_counters(hipStream_t st) {
    finish_pending(st);
    HIP_OK(hipMemcpyAsync(h_ctr, ctr, sizeof(Counters), hipMemcpyDeviceToHost, st));
    HIP_OK(hipStreamSynchronize(st));
    if (h_ctr->error & 1u) {
      // surfaced once; the reference maps engine exceptions to ResourceExhausted/InvalidArgument
      unsigned int zero = 0;
      HIP_OK(hipMemcpy(&ctr->error, &zero, sizeof(zero), hipMemcpyHostToDevice));
      throw Error(MHTE_RESOURCE_EXHAUSTED,
                  "table " + name + ": " + std::to_string(h_ctr->n_dropped) +
                      " ids dropped: no cuckoo path (raise capacity / lower max_load_factor)");
    }
  }

  // EmbeddingHashTableInterface::Clear (cuckoo_embedding_hash_table.cc:322-326: clear_with_callback +
  // DeallocateAll): no entries, the bucket array keeps its size, row handles start over; the
  // table's max_update_ts stands (it lives in the bridge, tf_bridge.cc:385-398)
  void clear(hipStream_t st) {
    finish_pending(st);
    ++mut_epoch;
    const uint64_t nb = uint64_t(1) << hp;
    clear_buckets_kernel<<<dim3(uint32_t((nb + 255) / 256)), 256, 0, st>>>(buckets, nb);
    HIP_OK(hipGetLastError());
    HIP_OK(hipMemsetAsync(ctr, 0, sizeof(Counters), st));
    HIP_OK(hipStreamSynchronize(st));
    memset(h_ctr, 0, sizeof(Counters));
    keys_upper = rows_upper = 0;
    // the row allocator starts over: a batch that was numbered and probed before (its records hold
    // row handles and reservations of the old numbering) must not be applied with them, and must
    // not give reservations "back" to the new counters — the table is a new one to such a workspace
    unregister_counters(ctr, ctr_serial);
    ctr_serial = register_counters(ctr);
  }

  void double_table(hipStream_t st) {
    ++mut_epoch;
    if (hp >= 34) throw Error(MHTE_RESOURCE_EXHAUSTED, "table " + name + ": hashpower limit");
    Bucket* nb = nullptr;
    const uint64_t n_old = uint64_t(1) << hp;
    HIP_OK(hipMalloc(&nb, n_old * 2 * sizeof(Bucket)));
    split_kernel<<<dim3(uint32_t((n_old + 255) / 256)), 256, 0, st>>>(buckets, nb, hp);
    HIP_OK(hipGetLastError());
    HIP_OK(hipStreamSynchronize(st));
    HIP_OK(hipFree(buckets));
    buckets = nb;
    ++hp;
    refresh_view();
  }

  // Called before every mutating op with the number of ids it may insert.
  // true if ensure_capacity(n) would have to grow the table (a displacement pass still
  // outstanding must be finished first: growing re-hashes)
  // keys in the buckets by the (synchronised) counters: row reservations of a batch that was numbered
  // and probed but not applied yet are counted in `alloc` ahead of their insert
  int64_t live_keys() const { return int64_t(h_ctr->alloc >> 32) - int64_t(h_ctr->reserved); }
  bool would_grow(uint64_t n) const {
    const uint64_t row_cap = uint64_t(chunks.size()) << chunk_shift;
    return double(keys_upper + n) > max_load * double(uint64_t(kSlots) << hp) ||
           rows_upper + n + kSpecSlackRows > row_cap;
  }
  // what: kCapBoth — room for n more keys and rows; kCapRows / kCapKeys — one half of it.  The
  // pipelined step reserves the next batch's ROWS a launch ahead (the build role's probe) and makes
  // room in the BUCKETS when that batch is applied, as before: a doubling a batch early would lower
  // the load factor the caller asked for.
  enum { kCapBoth = 0, kCapRows = 1, kCapKeys = 2 };
  void ensure_capacity(uint64_t n, hipStream_t st, int what = kCapBoth) {
    if (what != kCapRows) keys_upper += n;
    if (what != kCapKeys) rows_upper += n + kSpecSlackRows;
    const uint64_t row_cap = uint64_t(chunks.size()) << chunk_shift;
    const bool need_keys = double(keys_upper) > max_load * double(uint64_t(kSlots) << hp);
    const bool need_rows = rows_upper > row_cap;
    if (!need_keys && !need_rows) return;
    {
      // growing needs the live counts (a host round trip) and possibly a re-hash: not something a
      // stream capture can record
      hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
      if (hipStreamIsCapturing(st, &cs) == hipSuccess && cs != hipStreamCaptureStatusNone)
        throw Error(MHTE_FAILED_PRECONDITION,
                    "table " + name + " must grow, which cannot be captured into a hipGraph: "
                    "reserve capacity (initial_capacity / reserve_rows) before capturing");
    }
    sync_counters(st);
    // (keys counted ahead for row reservations are the batch's own inserts: n covers them)
    keys_upper = uint64_t(live_keys()) + (what != kCapRows ? n : 0);
    rows_upper = (h_ctr->alloc & 0xffffffffull) + (what != kCapKeys ? n + kSpecSlackRows : 0);
    if ((h_ctr->alloc >> 32) == 0) {
      // nothing to migrate: jump straight to the needed hashpower
      uint32_t want = hp;
      while (double(keys_upper) > max_load * double(uint64_t(kSlots) << want)) ++want;
      if (want != hp) {
        if (want > 34) throw Error(MHTE_RESOURCE_EXHAUSTED, "table " + name + ": hashpower limit");
        HIP_OK(hipFree(buckets));
        buckets = nullptr;
        alloc_buckets(want, &buckets, st);
        hp = want;
        ++mut_epoch;
        refresh_view();
      }
    }
    while (double(keys_upper) > max_load * double(uint64_t(kSlots) << hp)) double_table(st);
    if (rows_upper > (uint64_t(1) << 32) - 2)
      throw Error(MHTE_RESOURCE_EXHAUSTED, "table " + name + ": more than 2^32 rows");
    while (rows_upper > (uint64_t(chunks.size()) << chunk_shift)) {
      add_chunk();
      refresh_view();
    }
  }

  // ---------------------------------------------------------------- lookup
  void lookup(const int64_t* ids, int64_t n, const uint32_t* n_dev, float* out, hipStream_t st) {
    finish_pending(st);  // a deferred displacement pass always precedes the next op on the table
    if (n <= 0) return;
    Shape sh = pick_shape(dim, vec_ok && aligned16(out));
    // two ids per lane group, 512-thread workgroups, streaming stores: the fastest shape of the
    // sweep over ids per group x workgroup size x store kind (profiles/r01/f_lookup_sweep.jsonl:
    // 6.9 us for 65 536 ids against 9.4 us for one id per group); else one id per group, 256 threads
    const bool two = sh.VEC == 4 && n >= 4096;
    const int block = two ? 512 : 256;
    const uint32_t grid = uint32_t(((two ? (n + 1) / 2 : n) * sh.G + block - 1) / block);
    TableView v = view;
    v.trace = trace_region(kTagLookup, grid, block);
    // a table with segment retrievers: the retrievers' instance of the form, their descriptors behind the
    // raw kernel's arguments
    const int rt = retriever_instance(false);
    const RetrieverArgs ra = rt != kRtRaw ? retriever_args(false, 0) : RetrieverArgs{};
    auto launch = [&](auto raw, auto retrieve) {
      if (rt == kRtRaw) LAUNCH_HOT(kTagLookup, raw, grid, block, st, v, ids, n, n_dev, out, count_hits ? 1 : 0);
      else LAUNCH_HOT(kTagLookup, retrieve, grid, block, st, v, ids, n, n_dev, out, count_hits ? 1 : 0, ra);
    };
    for_shape(sh, [&](auto g_, auto v_) {
      constexpr int G = decltype(g_)::value, V = decltype(v_)::value;
      if (!two)
        launch(lookup_kernel<G, V>, pick_rt(rt, lookup_retrieve_kernel<G, V, kRtFakeQuant>,
                                            lookup_retrieve_kernel<G, V, kRtHashNet>, lookup_retrieve_kernel<G, V, kRtMixed>));
      else if constexpr (V == 4)   // (the float4 form only)
        launch(lookup_kernel_u<G, 4, 2, 1, 512>, pick_rt(rt, lookup_retrieve_kernel_u<G, kRtFakeQuant>,
                                                         lookup_retrieve_kernel_u<G, kRtHashNet>, lookup_retrieve_kernel_u<G, kRtMixed>));
    });
    HIP_OK(hipGetLastError());
  }

  // ---------------------------------------------------------------- upsert + apply
  // the displacement pass's instance for a lane width (launch_upsert, finish_pending)
  template <int OP>
  static auto slowpath_fn(int vec) {
    return vec == 4 ? slowpath_kernel<4, OP> : slowpath_kernel<1, OP>;
  }

  // ... and the fast path's: the whole-segment optimizer's instance only where the table has one
  template <int G, int V, int OP>
  static auto upsert_instance(bool has_group_opt) {
    return (OP == kOpOptimize && has_group_opt) ? upsert_kernel<G, V, OP, true> : upsert_kernel<G, V, OP>;
  }
  // ... and both kernels' instances for retriever_instance(true): kRtHashNet (the one-segment table), else kRtMixed
  template <int G, int V>
  static auto upsert_backward_instance(int rt, bool has_group_opt) {
    return rt == kRtHashNet ? upsert_backward_kernel<G, V, kRtHashNet, false>
                            : (has_group_opt ? upsert_backward_kernel<G, V, kRtMixed, true>
                                             : upsert_backward_kernel<G, V, kRtMixed, false>);
  }
  static auto slowpath_backward_fn(int vec, int rt) {
    const bool one = rt == kRtHashNet;
    return vec == 4 ? (one ? slowpath_backward_kernel<4, kRtHashNet> : slowpath_backward_kernel<4, kRtMixed>)
                    : (one ? slowpath_backward_kernel<1, kRtHashNet> : slowpath_backward_kernel<1, kRtMixed>);
  }
  // the arguments every update path hands its kernels; a null lrs: zero rates
  ApplyArgs apply_args(const float* lrs, int64_t update_time, int64_t global_step, int sum_dups,
                       int filter_mode) const {
    ApplyArgs a;
    for (int i = 0; i < kMaxSegments; ++i) a.lr[i] = (lrs && i < int(nseg)) ? lrs[i] : 0.f;
    a.ts = static_cast<uint32_t>(update_time);
    a.sum_dups = sum_dups;
    a.filter_mode = filter_mode;
    a.global_step = global_step;
    return a;
  }

  template <int OP>
  void launch_upsert(const int64_t* ids, int64_t n, const uint32_t* n_dev, const float* values,
                     const uint32_t* seg_off, const uint32_t* seg_pos, const ApplyArgs& a,
                     int32_t* status, hipStream_t st) {
    Shape sh = pick_shape(dim, vec_ok && (values == nullptr || aligned16(values)));
    ++mut_epoch;
    pending.reserve(size_t(n) + 1);
    uint32_t* skp = nullptr;
    if (flt_slots && a.filter_mode && seg_off) {
      skip.reserve(size_t(n) + 1);
      skp = skip.p;
    }
    const int64_t threads = n * sh.G;
    const dim3 grid(uint32_t((threads + 255) / 256));
    uint32_t* pend = pending.p;
    // an Optimize on a table with a HashNet segment: the retriever's Backward in front of the optimizer
    // (Assign / AssignAdd / Reinitialize write raw) — the retriever instances of both kernels, which take the
    // descriptors and no `status`
    const int rt = OP == kOpOptimize ? retriever_instance(true) : kRtRaw;
    const RetrieverArgs ra = rt != kRtRaw ? retriever_args(true, a.global_step) : RetrieverArgs{};
    for_shape(sh, [&](auto g_, auto v_) {
      constexpr int G = decltype(g_)::value, V = decltype(v_)::value;
      if (rt == kRtRaw)
        LAUNCH_HOT(kTagUpsert, (upsert_instance<G, V, OP>(has_group_opt)), grid, 256, st, view, ids, n, n_dev,
                   values, seg_off, seg_pos, a, status, pend, skp);
      else
        LAUNCH_HOT(kTagUpsert, (upsert_backward_instance<G, V>(rt, has_group_opt)), grid, 256, st, view, ids, n, n_dev,
                   values, seg_off, seg_pos, a, pend, skp, ra);
    });
    if (rt == kRtRaw) slowpath_fn<OP>(sh.VEC)<<<1, 64, 0, st>>>(view, ids, values, seg_off, seg_pos, a, status, pend, skp);
    else slowpath_backward_fn(sh.VEC, rt)<<<1, 64, 0, st>>>(view, ids, values, seg_off, seg_pos, a, pend, skp, ra);
    if (a.filter_mode) filter_maintain(st, uint64_t(n));
    HIP_OK(hipGetLastError());
  }

  template <int OP>
  void upsert(const int64_t* ids, int64_t n, const uint32_t* n_dev, const float* values,
              const float* lrs, int64_t update_time, int32_t flags, int32_t* status,
              hipStream_t st) {
    finish_pending(st);
    if (n <= 0) return;
    if (n > (int64_t(1) << 31) - 4096) throw Error(MHTE_INVALID_ARGUMENT, "too many ids in one op");
    // admission filter (tf_bridge.cc): Assign / Optimize are guarded by Contains; the multi-table
    // AssignAdd goes through AssignAdd2, which is not (:230-232); Reinitialize never filters
    const ApplyArgs a = apply_args(lrs, update_time, t_global_step, (flags & MHTE_SUM_DUPLICATES) ? 1 : 0,
                                   (OP == kOpReinit) ? 0 : (OP == kOpAssignAdd ? 3 : 1));
    ensure_capacity(uint64_t(n), st);
    if (flags & MHTE_IDS_UNIQUE) {
      launch_upsert<OP>(ids, n, n_dev, values, nullptr, nullptr, a, status, st);
      return;
    }
    if (n_dev) throw Error(MHTE_INVALID_ARGUMENT, "device-side count requires MHTE_IDS_UNIQUE");
    // in-op grouping: unique ids in first-occurrence order + ordered occurrence lists, then each
    // id's occurrences are applied in order by one group (sequential semantics of BatchOptimize)
    g_uids.reserve(n);
    g_inverse.reserve(n);
    g_seg_off.reserve(n + 1);
    g_seg_pos.reserve(n);
    g_nu.reserve(4);
    dd.unique(ids, n, g_uids.p, g_inverse.p, g_seg_off.p, g_seg_pos.p, g_nu.p, st);
    launch_upsert<OP>(g_uids.p, n, g_nu.p, values, g_seg_off.p, g_seg_pos.p, a, status, st);
  }

  // ---------------------------------------------------------------- fused backward
  // duplicate-gradient sum + upsert + optimizer apply of the unique ids of ws's most recent
  // unique() in one launch (sum_apply_kernel); falls back to segment-sum + upsert for wide rows.
  // the fused step kernels take every per-element optimizer (their FULL instantiations beyond SGD /
  // Adagrad / FTRL); the whole-segment GroupAdaGrad stays on the op-level kernels
  bool fusable() const {
    if (has_retriever) return false;   // (the step kernels read rows raw)
    for (uint32_t i = 0; i < nseg; ++i)
      if (view.seg[i].opt == kOptGroupAdagrad) return false;
    return fusable_shape();
  }
  bool fusable_shape() const {   // the row fits one lane group (of float4 lanes, where the row has them)
    Shape sh = pick_shape(dim, vec_ok);
    return dim <= uint32_t(sh.G * sh.VEC);
  }
  // The lane shape of a fused launch (sum_apply / step_fwd / step_bwd) for the buffers of THIS call:
  // float4 lanes need every one of them 16-byte aligned.  The fused kernels give a row ONE lane group
  // and do not loop over its columns, so a float4 table of more than 64 floats per row has no shape
  // for a buffer that is only 4-byte aligned (one float per lane covers columns 0..63).
  struct BufArg {
    const char* name;
    const void* p;
  };
  Shape fused_shape_of(std::initializer_list<BufArg> bufs) const {
    bool vec = vec_ok;
    for (const BufArg& b : bufs) vec = vec && aligned16(b.p);
    return pick_shape(dim, vec);
  }
  bool fused_shape_covers(std::initializer_list<BufArg> bufs) const {
    Shape sh = fused_shape_of(bufs);
    return dim <= uint32_t(sh.G * sh.VEC);
  }
  // ... or MHTE_INVALID_ARGUMENT, naming the buffer (as mhte_step_scatter / mhte_step_sum refuse it)
  Shape fused_shape(const char* what, std::initializer_list<BufArg> bufs) const {
    Shape sh = fused_shape_of(bufs);
    if (dim > uint32_t(sh.G * sh.VEC)) {
      std::string which;
      for (const BufArg& b : bufs)
        if (!aligned16(b.p)) which += std::string(which.empty() ? "" : ", ") + b.name;
      throw Error(MHTE_INVALID_ARGUMENT,
                  std::string(what) + ": rows of more than 64 floats must be 16-byte aligned (" + which +
                      (which.empty() ? "row too wide for the fused step" : " is not") + "; table " + name +
                      ", dim " + std::to_string(dim) + ")");
    }
    return sh;
  }
  bool basic_opts() const {   // SGD / Adagrad / FTRL only: the BASIC kernel instantiations
    for (uint32_t i = 0; i < nseg; ++i)
      if (view.seg[i].opt > kOptFtrl || view.seg[i].sr16) return false;   // (rounding: FULL forms only)
    return true;
  }
  void sum_optimize(DedupWs& ws, const int64_t* uids, int64_t n_max, const uint32_t* n_dev,
                    const float* grads, const uint32_t* lst_start, const uint32_t* lst_end,
                    const uint32_t* seg_pos, int64_t n, float* grad_u, const float* lrs,
                    int64_t update_time, bool exact_order, bool defer_slowpath, hipStream_t st) {
    finish_pending(st);
    if (n <= 0 || n_max <= 0) return;
    if (n != ws.last_n)
      throw Error(MHTE_FAILED_PRECONDITION,
                  "sum_optimize: workspace does not hold the occurrence lists of this batch");
    const ApplyArgs a = apply_args(lrs, update_time, 0, 1, 1);  // (global_step: SGD / Adagrad / FTRL only here)
    ++mut_epoch;
    ensure_capacity(uint64_t(n_max), st);
    Shape sh = fused_shape("sum_optimize", {{"grads", grads}, {"grad_unique", grad_u}});
    pending.reserve(size_t(n_max) + 1);
    // upper bound of the work items dd_finish may have queued (each heavy list has > kLightMax
    // entries and at most one partly filled chunk); surplus blocks exit on the device-side count
    const uint32_t nblk_b =
        exact_order ? 0u : uint32_t(n / kChunk + n / (kLightMax + 1) + 1);
    const uint32_t nblk_a = uint32_t((n_max * sh.G + 255) / 256);
    ws.backward_scratch(n, dim, nblk_b, st);
    const uint32_t light_max = exact_order ? 0xffffffffu : uint32_t(kLightMax);
    uint32_t* pend = pending.p;
    TableView v = view;
    v.trace = trace_region(kTagSumApply, nblk_a + nblk_b, 256);
    for_shape(sh, [&](auto g_, auto v_) {
      constexpr int G = decltype(g_)::value, V = decltype(v_)::value;
      LAUNCH_HOT(kTagSumApply, (sum_apply_kernel<G, V>), nblk_a + nblk_b, 256, st, v, uids, n_dev, n_max, grads,
                 lst_start, lst_end, seg_pos, ws.work.p, ws.heavy_n.p + 3, nblk_b, light_max, ws.part.p,
                 ws.arrive.p, grad_u, a, pend);
    });
    HIP_OK(hipGetLastError());
    queued.queue(uids, grad_u, a, sh.VEC);
    filter_maintain(st, uint64_t(n_max));
    if (!defer_slowpath) finish_pending(st);
  }

  // ---------------------------------------------------------------- pipelined step (2 launches)
  //   step_forward   lookup of this batch | run dedup of the next batch
  //                  | displacement pass of the previous update (gated, usually idle)
  //   step_backward  apply of this batch | heavy work list of the next batch
  // the instances of the two launches for a lane shape (BASIC: SGD / Adagrad / FTRL only)
  template <int G, int V>
  static auto step_fwd_instance(int unr, bool basic) {
    if (unr == 2) return basic ? step_fwd_kernel<G, V, 2, true> : step_fwd_kernel<G, V, 2, false>;
    return basic ? step_fwd_kernel<G, V, 3, true> : step_fwd_kernel<G, V, 3, false>;
  }
  // filt: a table with an admission filter takes the instances that consult it (FILT; the others carry no
  // filter code — with it the headline instance kept 11 spilled registers, without it 2).  optk >= 0: the
  // instance compiled for that optimizer alone (one-segment FULL tables with float4 lanes, no filter:
  // 61 -> 7-17 spilled registers for Adam, and the row fetched ahead as the BASIC instances do).
  template <int G, int V>
  static auto step_bwd_instance(bool basic, bool oneseg, bool filt, int optk) {
    if (filt) {
      if (oneseg) return basic ? step_bwd_kernel<G, V, true, false, -1, true> : step_bwd_kernel<G, V, true, true, -1, true>;
      return basic ? step_bwd_kernel<G, V, false, false, -1, true> : step_bwd_kernel<G, V, false, true, -1, true>;
    }
    if constexpr (V == 4) {
      switch (optk) {
        case kOptMomentum: return step_bwd_kernel<G, 4, true, true, kOptMomentum>;
        case kOptAdadelta: return step_bwd_kernel<G, 4, true, true, kOptAdadelta>;
        case kOptRmsprop: return step_bwd_kernel<G, 4, true, true, kOptRmsprop>;
        case kOptRmspropV2: return step_bwd_kernel<G, 4, true, true, kOptRmspropV2>;
        case kOptAdam: return step_bwd_kernel<G, 4, true, true, kOptAdam>;
        case kOptAmsgrad: return step_bwd_kernel<G, 4, true, true, kOptAmsgrad>;
        default: break;
      }
    }
    if (oneseg) return basic ? step_bwd_kernel<G, V, true> : step_bwd_kernel<G, V, true, true>;
    return basic ? step_bwd_kernel<G, V, false> : step_bwd_kernel<G, V, false, true>;
  }

  void step_forward(const int64_t* ids, int64_t n, float* out, const RunView& nxt, hipStream_t st) {
    if (n <= 0) throw Error(MHTE_INVALID_ARGUMENT, "step_forward: empty batch");
    Shape sh = fused_shape("step_forward", {{"embedding", out}});
    const PendingPass pp = take_pending(sh.VEC, st);
    SlowArgs sp{};
    sp.enabled = pp.valid ? 1 : 0;
    if (pp.valid) {
      sp.uids = pp.uids;
      sp.grad_u = pp.grad;
      sp.pending = pending.p;
      sp.a = pp.args;
    }
    // every workgroup of the launch resident at once (two 1024-thread workgroups per CU); the lookup
    // role covers its groups in grid-stride trips
    const uint32_t others = nxt.nblk + uint32_t(sp.enabled);
    const uint32_t slots = uint32_t(2 * num_cus);
    // (the displacement pass's workgroup leaves within a microsecond: it does not count against the
    // lookups' residency — one workgroup fewer would put 1/512 of the batch on a second trip, the
    // launch's tail)
    const uint32_t held = nxt.nblk;
    const uint32_t room = slots > held + 64 ? slots - held : 64u;
    auto blocks_for = [&](int unr) {
      const int64_t groups = (n + unr - 1) / unr;
      return uint32_t((groups * sh.G + kRdBlock - 1) / kRdBlock);
    };
    // (measured: 2 ids per group with a second trip for a few workgroups has a shorter tail than 3
    // per group in one trip; a wavefront's life is the max over its ids of two dependent misses)
    int unr = 2;
    while (unr < 3 && blocks_for(unr) > 2 * room) ++unr;
    const uint32_t nblk_l = std::min(blocks_for(unr), room);
    const dim3 grid(others + nblk_l);
    TableView v = view;
    v.trace = trace_region(kTagStepFwd, grid.x, kRdBlock);
    const bool basic = basic_opts();   // (the displacement role's update code)
    for_shape(sh, [&](auto g_, auto v_) {
      constexpr int G = decltype(g_)::value, V = decltype(v_)::value;
      LAUNCH_HOT(kTagStepFwd, (step_fwd_instance<G, V>(unr, basic)), grid, kRdBlock, st, nxt, v, ids, n, out,
                 count_hits ? 1 : 0, sp, nblk_l);
    });
    HIP_OK(hipGetLastError());
  }

  // ahead: the run dedup of the batch TWO steps on (DedupWs::begin_run_dedup's RunView; nblk 0: none)
  // rides in this launch
  void step_backward(DedupWs& ws, DedupWs* ws_next, const int64_t* uids, int64_t n_max,
                     const uint32_t* n_dev, const float* grads, int64_t n, float* grad_u,
                     const float* lrs, int64_t update_time, bool exact_order, hipStream_t st,
                     int64_t global_step = 0, const RunView& ahead = RunView{}) {
    finish_pending(st);
    if (n <= 0 || n_max <= 0) throw Error(MHTE_INVALID_ARGUMENT, "step_backward: empty batch");
    const ExactMode exact = exact_mode(exact_order, dim);
    if (ws.r_stage == 0 || int64_t(ws.rv.n) != n || ws.rv.uids != uids || ws.rv.n_unique != n_dev)
      throw Error(MHTE_FAILED_PRECONDITION,
                  "step_backward: workspace does not hold the run dedup of this batch");
    // a probe of another table, or of this one before it was cleared (a restore between two steps): probe again
    if (ws.probed() && !ws.probe_is_of(*this)) ws.void_probe(st);
    // first step of a pipeline (later ones were numbered — and probed — a step ahead, inside the
    // previous update's launch)
    if (ws.r_stage == 1 || !ws.probed()) {
      // (r_stage 2 without a probe: numbered on its own, mhte_step_dedup — the probe alone)
      ws.probe_out_reserve(n);
      const bool reserve = flt_slots == nullptr;
      if (reserve) ensure_capacity(uint64_t(std::min<int64_t>(n_max, n)), st, kCapRows);
      ProbeOut po{ws.r_urec.p, reserve ? 1u : 0u};
      if (ws.r_stage == 1)
        rd_build_probe_kernel<<<DedupWs::build_blocks(ws.rv), 256, 0, st>>>(ws.rv, uint32_t(kStepLightMax), view, po);
      else
        rd_probe_kernel<<<uint32_t(std::min<int64_t>(256, (n + 255) / 256)), 256, 0, st>>>(
            ws.rv, view, po, uint32_t(n), exact.light_max());
      HIP_OK(hipGetLastError());
      ws.adopt_probe(*this, reserve);
    }
    const ApplyArgs a = apply_args(lrs, update_time, global_step /* batch softmax */, 1, 1);
    ++mut_epoch;
    // (prealloc: the rows were reserved — and their room made — when the batch was numbered)
    const bool prealloc = ws.consume_probe();
    ensure_capacity(uint64_t(std::min<int64_t>(n_max, n)), st, prealloc ? kCapKeys : kCapBoth);
    Shape sh = fused_shape("step_backward", {{"grads", grads}, {"grad_unique", grad_u}});
    pending.reserve(size_t(n_max) + 1);
    const uint32_t cap_items = DedupWs::max_items(n);
    ws.part.reserve(size_t(cap_items) * dim + 16);
    ApplyCtl c{};
    c.grads = grads;
    c.grad_u = grad_u;
    c.pending = pending.p;
    c.part = ws.part.p;
    c.arrive = ws.zeroed_arrive(size_t(n), st);
    c.n_max = n_max;
    c.light_max = exact.light_max();
    c.pre_summed = exact.pre ? 1u : 0u;
    c.urow = nullptr;
    c.uloc = nullptr;
    c.uts = nullptr;
    c.urec = ws.r_urec.p;
    c.trusted = 0;   // (an update, a displacement pass, a doubling may lie between probe and use: the
                     // kernel checks every hint against the slot's key)
    // fixed grids with grid-stride loops: item workgroups first (longest chain), sized for the
    // work a Zipf batch has; more ids / items than workgroups just means more trips
    const uint32_t groups_per_wg = uint32_t(256 / sh.G);
    // residency budget: 4 workgroups of 256 threads per CU (launch bounds of step_bwd_kernel)
    const uint32_t slots = uint32_t(kBwdBlocksPerCu * num_cus);
    c.nblk_items = exact.walk ? 0u : std::min<uint32_t>(cap_items, uint32_t(num_cus) * 10 / 8);
    if (exact.pre) {
      const uint32_t gx = std::min<uint32_t>(cap_items, uint32_t(num_cus));
      if (sh.VEC == 4) rd_exact_sum_kernel<4><<<gx, kExactThreads, 0, st>>>(ws.rv, grads, dim, ws.part.p);
      else rd_exact_sum_kernel<1><<<gx, kExactThreads, 0, st>>>(ws.rv, grads, dim, ws.part.p);
      HIP_OK(hipGetLastError());
    }
    c.nblk_ids = std::max<uint32_t>(
        1, std::min<uint32_t>(uint32_t((std::min<int64_t>(n_max, n) + groups_per_wg - 1) / groups_per_wg),
                              slots - c.nblk_items - 128));
    RunView nxt{};
    uint32_t nblk_build = 0;
    ProbeOut po{};
    bool reserve_next = false;
    if (ws_next && ws_next->r_stage == 1) {
      nxt = ws_next->rv;
      nblk_build = DedupWs::build_blocks(nxt);
      // (with the run dedup of the batch two ahead in the launch, the build role gives up as many
      // workgroups as the dedup takes — two trips each instead of one: every workgroup of the launch
      // stays resident from the start; a late starter would be the launch's tail)
      if (ahead.nblk && nblk_build > ahead.nblk) nblk_build = std::max<uint32_t>(nblk_build - ahead.nblk, nblk_build / 2);
      // the next batch is numbered AND probed in this launch: hints and row reservations for its
      // update (room for the rows it may reserve is made now)
      ws_next->probe_out_reserve(int64_t(nxt.n));
      reserve_next = flt_slots == nullptr;
      if (reserve_next) ensure_capacity(uint64_t(nxt.n), st, kCapRows);
      po = ProbeOut{ws_next->r_urec.p, reserve_next ? 1u : 0u};
    }
    DedupArgs da{};
    if (ahead.nblk) {
      da.hs = ahead.hs;
      da.hlist = ahead.hlist;
      da.btab_key = ahead.btab_key;
      da.btab_val = ahead.btab_val;
      da.seg = ahead.seg;
      da.ctr = ahead.ctr;
      da.ids = ahead.ids;
      da.cap_mask = ahead.cap_mask;
      da.n = ahead.n;
      da.nblk = ahead.nblk;
    }
    const dim3 grid(da.nblk + nblk_build + c.nblk_items + c.nblk_ids);
    TableView v = view;
    v.trace = trace_region(kTagStepBwd, grid.x, 256);
    const RunView cur = ws.rv;
    const bool basic = basic_opts(), oneseg = nseg == 1, filt = flt_slots != nullptr;
    static const bool no_optk = getenv("MHTE_NO_OPTK") != nullptr;   // (A/B: the one FULL instance for all)
    const int optk =
        (!basic && oneseg && sh.VEC == 4 && !view.seg[0].sr16 && !no_optk && !filt) ? int(view.seg[0].opt) : -1;
    for_shape(sh, [&](auto g_, auto v_) {
      constexpr int G = decltype(g_)::value, V = decltype(v_)::value;
      LAUNCH_HOT(kTagStepBwd, (step_bwd_instance<G, V>(basic, oneseg, filt, optk)), grid, 256, st, nxt, nblk_build,
                 v, cur, c, a, po, da);
    });
    hipError_t le = hipGetLastError();
    ws.applied();
    if (nblk_build) ws_next->adopt_probe(*this, reserve_next);
    if (le != hipSuccess) {
      ws.r_clean_cap = 0;
      if (ws_next) ws_next->r_clean_cap = 0;
      HIP_OK(le);
    }
    filter_maintain(st, uint64_t(n));
    // the displacement pass rides in the next step_forward (or runs on its own if anything else
    // touches the table first)
    queued.queue(uids, grad_u, a, sh.VEC);
  }

  // The displacement pass for the ids the last fused backward could not place (both buckets full; a no-op
  // kernel when there are none, which is the usual case).  The update queues it; the next step_forward
  // takes it into its own launch, and whatever else touches the table first runs it on its own
  // (finish_pending).
  struct PendingPass {
    bool valid = false;
    const int64_t* uids = nullptr;
    const float* grad = nullptr;
    ApplyArgs args{};
    int vec = 4;   // lane width the update stored the queued gradients for
    void queue(const int64_t* uids_, const float* grad_, const ApplyArgs& args_, int vec_) {
      valid = true;
      uids = uids_;
      grad = grad_;
      args = args_;
      vec = vec_;
    }
    PendingPass take() {
      const PendingPass p = *this;
      valid = false;
      return p;
    }
  };
  PendingPass queued;
  // ... taken by a launch of lane width `vec`.  The update stored the queued gradients for its own lane width,
  // which follows the alignment of ITS buffers: a backward on a misaligned gradient (one float per lane) before
  // a forward into an aligned embedding buffer (float4), or the other way round (rows of <= 64 floats;
  // exercised by tests/test_alignment_forms_gpu.py) — a forward with another lane width runs the pass on its
  // own first, in front of its launch, and carries none.
  PendingPass take_pending(int vec, hipStream_t st) {
    if (queued.valid && queued.vec != vec) finish_pending(st);
    return queued.take();
  }
  // a displacement pass somebody else owes this table (the id-sharded step runs the pass of its last owner
  // update inside its NEXT owner lookup's launch, mhte_shard_host.h): whoever touches the table first — any
  // op, a save, a doubling — makes it happen now
  void (*ext_flush)(void*, hipStream_t) = nullptr;
  void* ext_ctx = nullptr;
  void finish_pending(hipStream_t st, bool skip_ext = false) {
    if (ext_flush && !skip_ext) {
      void (*f)(void*, hipStream_t) = ext_flush;
      f(ext_ctx, st);   // (clears the hook of every table it covers)
    }
    if (!queued.valid) return;
    const PendingPass pp = queued.take();
    ++mut_epoch;
    LAUNCH_HOT(kTagSlowpath, slowpath_fn<kOpOptimize>(pp.vec), 1, 64, st, view, pp.uids, pp.grad,
               nullptr, nullptr, pp.args, nullptr, pending.p, nullptr);
    HIP_OK(hipGetLastError());
  }

  void note_update_time(int64_t update_time) {
    // fuzzy max, tf_bridge.cc:262-263
    max_update_ts = std::max(max_update_ts, update_time);
  }

  // Feature eviction cadence (tf_bridge.cc:73-104: a thread per table wakes every 10 s and runs
  // Evict(max_update_ts) once feature_evict_every_n_hours have passed since the last one).  Called by
  // the update entry points with their stream: the scan is ordered with the table's other work.
  bool evict_enabled = false;
  double evict_every_s = 240 * 3600.0;
  double last_evict = 0, last_evict_check = 0;
  uint64_t evict_runs = 0;
  void maybe_evict(hipStream_t st) {
    if (!evict_enabled) return;
    const double now = lib_now();
    if (now - last_evict_check < 10.0) return;
    last_evict_check = now;
    if (now - last_evict < evict_every_s) return;
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(st, &cs) == hipSuccess && cs != hipStreamCaptureStatusNone) return;
    evict(-1, st);
    last_evict = now;
    ++evict_runs;
  }

  void evict(int64_t max_ts, hipStream_t st) {
    finish_pending(st);
    ++mut_epoch;
    TtlConfig ttl;
    ttl.default_days = default_expire_days;
    ttl.n = int32_t(expire_slots.size());
    ttl.slots = d_expire_slots.p;
    ttl.days = d_expire_days.p;
    const uint64_t nslots = (uint64_t(1) << hp) * kSlots;
    // persistent: 8 workgroups per CU (one atomic pair per workgroup at the end)
    const uint64_t need = (nslots + 255) / 256;
    evict_kernel<<<dim3(uint32_t(std::min<uint64_t>(need, 2048))), 256, 0, st>>>(
        view, max_ts < 0 ? max_update_ts : max_ts, ttl);
    HIP_OK(hipGetLastError());
    // opt-in (mhte_table_set_auto_compact): the scan may have freed enough rows to be worth a compaction.
    // Unset — the default — the scan stays what it was: one launch, no host wait.
    if (auto_compact > 0.0) {
      hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
      if (hipStreamIsCapturing(st, &cs) == hipSuccess && cs != hipStreamCaptureStatusNone) return;
      sync_counters(st);
      const uint64_t in_use = h_ctr->alloc & 0xffffffffull;
      const uint64_t live = uint64_t(live_keys()) + (h_ctr->special_state == 1 ? 1 : 0);
      if (in_use > live && double(in_use - live) >= auto_compact * double(in_use)) {
        int64_t res[4];
        compact(res, st);
      }
    }
  }

  // Compaction: the rows of the live entries move into the lowest row handles (mhte_compact_kernels.h)
  // and the slabs above them are released.  Keys, bucket positions, timestamps, dump order and every
  // row's bits stay; only row handles change.  Everything that holds a handle from before is made void:
  // the epoch moves (the multi-table and the id-sharded step hand their hints over only while it stands
  // still) and the counters are registered anew, as in clear() — to a workspace that was numbered and
  // probed before, the table is another one: it probes again, and the rows it had reserved (handles in
  // no bucket, now possibly given to a survivor) are dropped with their keys taken off the live count.
  // out: handles in use before, after, rows moved, bytes of slabs released.
  double auto_compact = 0.0;   // mhte_table_set_auto_compact: free fraction at which evict() compacts (0: never)
  void compact(int64_t out[4], hipStream_t st) {
    {
      hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
      if (hipStreamIsCapturing(st, &cs) == hipSuccess && cs != hipStreamCaptureStatusNone)
        throw Error(MHTE_FAILED_PRECONDITION,
                    "table " + name + ": a compaction moves rows and releases slabs, which cannot be "
                    "captured into a hipGraph");
    }
    finish_pending(st);
    sync_counters(st);
    ++mut_epoch;
    const uint64_t in_use = h_ctr->alloc & 0xffffffffull;
    const bool spec = h_ctr->special_state == 1;
    const uint64_t live = uint64_t(live_keys()) + (spec ? 1 : 0);
    out[0] = out[1] = int64_t(in_use);
    out[2] = out[3] = 0;
    if (in_use == live) return;
    const uint64_t row_cap = uint64_t(chunks.size()) << chunk_shift;
    if (live > in_use || in_use > row_cap)
      throw Error(MHTE_INTERNAL, "table " + name + ": compact: " + std::to_string(live) + " live entries, " +
                                     std::to_string(in_use) + " row handles in use, room for " +
                                     std::to_string(row_cap));
    const uint32_t L = uint32_t(live);
    uint32_t n_slot_movers = 0, special_src = kNoRow;
    DevBuf<uint32_t> bitmap, tile_movers, tile_holes, holes, mv_src;
    DevBuf<uint64_t> mv_slot;
    if (L > 0) {
      const uint64_t nslots = (uint64_t(1) << hp) * kSlots;
      const uint64_t ntiles = (nslots + kCompactTileSlots - 1) / kCompactTileSlots;
      const uint32_t nwords = (L + 31u) / 32u;
      const uint32_t nhtiles = (nwords + kCompactTileWords - 1) / kCompactTileWords;
      const uint32_t grid_s = uint32_t(std::min<uint64_t>(ntiles, 2048));
      const uint32_t grid_h = std::min<uint32_t>(nhtiles, 2048);
      bitmap.reserve(nwords);
      tile_movers.reserve(ntiles);
      tile_holes.reserve(nhtiles);
      HIP_OK(hipMemsetAsync(bitmap.p, 0, sizeof(uint32_t) * nwords, st));
      compact_mark_kernel<<<grid_s, 256, 0, st>>>(view, L, ntiles, bitmap.p, tile_movers.p);
      HIP_OK(hipGetLastError());
      compact_hole_count_kernel<<<grid_h, 256, 0, st>>>(bitmap.p, nwords, L, nhtiles, tile_holes.p);
      HIP_OK(hipGetLastError());
      std::vector<uint32_t> hm(ntiles), hh(nhtiles);
      HIP_OK(hipMemcpyAsync(hm.data(), tile_movers.p, sizeof(uint32_t) * ntiles, hipMemcpyDeviceToHost, st));
      HIP_OK(hipMemcpyAsync(hh.data(), tile_holes.p, sizeof(uint32_t) * nhtiles, hipMemcpyDeviceToHost, st));
      HIP_OK(hipStreamSynchronize(st));
      // exclusive scans, in place (a cold path, as in dump)
      uint64_t n_m = 0, n_h = 0;
      for (uint32_t& c : hm) {
        const uint32_t v = c;
        c = uint32_t(n_m);
        n_m += v;
      }
      for (uint32_t& c : hh) {
        const uint32_t v = c;
        c = uint32_t(n_h);
        n_h += v;
      }
      if (spec && h_ctr->special_row >= L) special_src = h_ctr->special_row;
      const uint64_t n_movers = n_m + (special_src != kNoRow ? 1 : 0);
      // one hole per mover: holds when the handles in the buckets are distinct and the counters true
      if (n_movers != n_h)
        throw Error(MHTE_INTERNAL, "table " + name + ": compact: " + std::to_string(n_movers) + " rows above handle " +
                                       std::to_string(L) + " but " + std::to_string(n_h) + " free handles below it");
      n_slot_movers = uint32_t(n_m);
      if (n_movers) {
        holes.reserve(n_movers);
        mv_slot.reserve(n_m + 1);
        mv_src.reserve(n_m + 1);
        HIP_OK(hipMemcpyAsync(tile_holes.p, hh.data(), sizeof(uint32_t) * nhtiles, hipMemcpyHostToDevice, st));
        compact_hole_emit_kernel<<<grid_h, 256, 0, st>>>(bitmap.p, nwords, L, nhtiles, tile_holes.p, holes.p,
                                                         uint32_t(n_movers));
        HIP_OK(hipGetLastError());
        if (n_m) {
          HIP_OK(hipMemcpyAsync(tile_movers.p, hm.data(), sizeof(uint32_t) * ntiles, hipMemcpyHostToDevice, st));
          compact_mover_emit_kernel<<<grid_s, 256, 0, st>>>(view, L, ntiles, tile_movers.p, mv_slot.p, mv_src.p,
                                                            n_slot_movers);
          HIP_OK(hipGetLastError());
        }
        // a group of G lanes per row, one copy unit (float4, or a float) per lane and trip
        const bool vec = row_floats % 4 == 0;
        const uint32_t units = vec ? row_floats / 4 : row_floats;
        const uint32_t G = std::min<uint32_t>(64, 1u << ceil_log2(units));
        const uint64_t wgs = (n_movers * G + 255) / 256;
        const uint32_t grid_m = uint32_t(std::min<uint64_t>(wgs, uint64_t(8) * num_cus));
        if (vec)
          compact_move_kernel<4><<<grid_m, 256, 0, st>>>(view, mv_slot.p, mv_src.p, holes.p, n_slot_movers,
                                                         special_src, L, row_cap, G);
        else
          compact_move_kernel<1><<<grid_m, 256, 0, st>>>(view, mv_slot.p, mv_src.p, holes.p, n_slot_movers,
                                                         special_src, L, row_cap, G);
        HIP_OK(hipGetLastError());
      }
    }
    compact_counters_kernel<<<1, 64, 0, st>>>(ctr, L);
    HIP_OK(hipGetLastError());
    // (the stream, then — inside hipFree — the device: a step's side stream has nothing of this table's
    // in flight that outlives that, which is what double_table relies on for the old bucket array)
    HIP_OK(hipStreamSynchronize(st));
    const size_t keep =
        std::max<size_t>(1, size_t((uint64_t(L) + kSpecSlackRows + (uint64_t(1) << chunk_shift) - 1) >> chunk_shift));
    const size_t slab_bytes = (size_t(1) << chunk_shift) * row_floats * sizeof(float);
    size_t released = 0;
    if (chunks.size() > keep) {
      HIP_OK(hipMemset(d_chunks + keep, 0, sizeof(float*) * (chunks.size() - keep)));
      while (chunks.size() > keep) {
        HIP_OK(hipFree(chunks.back()));
        chunks.pop_back();
        released += slab_bytes;
      }
    }
    unregister_counters(ctr, ctr_serial);
    ctr_serial = register_counters(ctr);
    sync_counters(st);
    keys_upper = uint64_t(live_keys());
    rows_upper = h_ctr->alloc & 0xffffffffull;
    refresh_view();
    out[1] = int64_t(L);
    out[2] = int64_t(n_slot_movers) + (special_src != kNoRow ? 1 : 0);
    out[3] = int64_t(released);
  }
};

inline bool DedupWs::probe_is_of(const Table& tb) const {
  return r_res_ctr == tb.view.ctr && r_res_serial == tb.ctr_serial;
}
inline void DedupWs::adopt_probe(const Table& tb, bool reserved) {
  r_stage = 2;
  r_hints = true;
  r_prealloc = reserved;
  r_res_ctr = tb.view.ctr;
  r_res_serial = tb.ctr_serial;
}

// ------------------------------------------------------------------------------------------ multi table
}  // namespace mhte

struct mhte_multi_table {
  int device = 0;
  std::string shared_name;
  mhte::CkptPool ckpt_stages;   // checkpoint staging, one per concurrent shard job, reused across calls
  std::vector<std::unique_ptr<mhte::Table>> tables;  // sorted by name
  // device copies of the tables' views, read by the multi-table launches (mhte_mstep_host.h)
  mhte::DevBuf<mhte::TableView> d_views;
  mhte::DevBuf<mhte::RetrieverArgs> d_rets;   // the tables' retriever descriptors of a fused-op launch (sync_retrievers)
  std::vector<uint64_t> view_uploaded;
  // the attached touched-key set (mhte_touched_host.h); read under a table's mutex, written under all
  mhte_touched_key_set* touched = nullptr;
  // live step objects, under g_touched_link_mu (a filter and a set together refuse a multi step, a set
  // refuses an id-sharded step); destroying the table first unlinks them
  std::vector<mhte_multi_step*> multi_steps;
  std::vector<mhte_shard_step*> shard_steps;
};
struct mhte_dedup_ws {
  mhte::DedupWs ws;
};
// live tables by shared_name (the TF ResourceMgr's role for ReadMonolithMultiHashTable /
// IsHashTableInitialized)
static std::mutex g_registry_mu;
static std::map<std::string, mhte_multi_table*> g_registry;
struct mhte_hash_filter {
  int device = 0;
  uint32_t* slots = nullptr;       // [nsplit][stride]
  uint32_t* state = nullptr;       // FilterState
  uint64_t total = 0;              // hash range of a split = split_capacity * 1.2
  uint64_t capacity = 0;           // the filter's (constructor argument)
  uint32_t nsplit = 0, stride = 0, split_cap = 0, split_num_arg = 0;
  mhte::FilterBudget budget;       // when the window can have to move (sliding filters)
  mhte::TableView view() const {   // (a view that only carries the filter: the filter's own kernels)
    mhte::TableView v{};
    v.flt_slots = slots;
    v.flt_total = total;
    v.flt_state = state;
    v.flt_nsplit = nsplit;
    v.flt_stride = stride;
    v.flt_cap = split_cap;
    return v;
  }
  // SlotOccurrenceThresholdConfig given with the filter (mhte_hash_filter_create_from_proto)
  bool has_occ = false;
  int32_t occ_default = 0;
  std::vector<int64_t> occ_slots;
  std::vector<int32_t> occ_thr;
  ~mhte_hash_filter() {
    if (slots) {
      (void)hipSetDevice(device);
      (void)hipFree(slots);
    }
    if (state) (void)hipFree(state);
  }
};

// the read-only probe (mhte_table_contains; the touched-key set's record of a filtered table)
namespace mhte {
__global__ __launch_bounds__(256) void contains_kernel(TableView tv, const int64_t* __restrict__ ids,
                                                       const uint32_t* __restrict__ n_dev, int64_t n,
                                                       int32_t* __restrict__ out) {
  const int64_t i = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
  if (i >= n) return;
  if (n_dev && i >= int64_t(*n_dev)) {   // (behind the device-side count: not held)
    out[i] = 0;
    return;
  }
  const int64_t id = ids[i];
  if (id == kEmptyKey) {
    out[i] = tv.ctr->special_state == 1;
    return;
  }
  const uint64_t hv = hash_key(id);
  const uint64_t i1 = index_hash(tv.hp, hv);
  const uint64_t i2 = alt_index(tv.hp, partial_key(hv), i1);
  int found = 0;
  for (int s = 0; s < kSlots; ++s) {
    found |= (tv.buckets[i1].key[s] == id);
    found |= (tv.buckets[i2].key[s] == id);
  }
  out[i] = found;
}
}  // namespace mhte

#include "mhte_touched_host.h"

namespace mhte {

template <class F>
static mhte_status guard(F&& f) {
  try {
    f();
    return MHTE_OK;
  } catch (const Error& e) {
    g_last_error = e.what();
    return e.code;
  } catch (const std::exception& e) {
    g_last_error = e.what();
    return MHTE_INTERNAL;
  }
}

static void check_handle(const mhte_multi_table* t) {
  if (!t) throw Error(MHTE_INVALID_ARGUMENT, "null table handle");
}
static Table& table_at(mhte_multi_table* t, int32_t i) {
  check_handle(t);
  if (i < 0 || i >= int32_t(t->tables.size()))
    throw Error(MHTE_INVALID_ARGUMENT, "table index out of range: " + std::to_string(i));
  return *t->tables[i];
}

// ragged (id, id_split) over the tables; multi_hash_table_update_op.cc:34-45 error texts
static void check_split(const mhte_multi_table* t, const int64_t* id_split, int64_t n_split,
                        const char* what) {
  check_handle(t);
  if (!id_split || n_split - 1 != int64_t(t->tables.size()))
    throw Error(MHTE_INVALID_ARGUMENT,
                std::string("The length of tensor `") + what + "` doesn't equal to table num. " +
                    std::to_string(n_split - 1) + "v.s." + std::to_string(t->tables.size()));
  for (int64_t i = 0; i + 1 < n_split; ++i)
    if (id_split[i + 1] < id_split[i]) throw Error(MHTE_INVALID_ARGUMENT, "id_split not monotonic");
}

template <int OP>
static void ragged_upsert(mhte_multi_table* t, const int64_t* id, const int64_t* id_split,
                          int64_t n_split, const float* value, int64_t value_len,
                          const float* learning_rate, int64_t n_lr, int64_t update_time,
                          int32_t flags, void* stream) {
  check_split(t, id_split, n_split, "id");
  HIP_OK(hipSetDevice(t->device));
  int64_t value_offset = 0, lr_offset = 0;
  for (size_t i = 0; i < t->tables.size(); ++i) {
    Table& tb = *t->tables[i];
    const int64_t num_ids = id_split[i + 1] - id_split[i];
    const int64_t value_size = num_ids * tb.dim;
    if (value_offset + value_size > value_len)
      throw Error(MHTE_INVALID_ARGUMENT, "The length of tensor `value` is too short. Currently value" +
                                             std::to_string(value_len));
    const float* lrs = nullptr;
    if (OP == kOpOptimize) {
      lrs = learning_rate + lr_offset;
      lr_offset += tb.nseg;
      if (lr_offset > n_lr)
        throw Error(MHTE_INVALID_ARGUMENT,
                    "The length of tensor `learning_rate` is too short. Currently value" +
                        std::to_string(n_lr));
    }
    std::lock_guard<std::mutex> g(tb.mu);
    tb.note_update_time(update_time);
    tb.upsert<OP>(id + id_split[i], num_ids, nullptr, value + value_offset, lrs, update_time, flags,
                  nullptr, S(stream));
    if (OP == kOpOptimize) tb.maybe_evict(S(stream));
    if (OP == kOpOptimize) tk_record(t, tb, int32_t(i), id + id_split[i], num_ids, nullptr, S(stream));
    value_offset += value_size;
  }
}

}  // namespace mhte

#include "mhte_mstep_host.h"
#include "mhte_shard_host.h"
#include "mhte_gemm_host.h"
#include "mhte_aux_host.h"
#include "mhte_clip_host.h"
#include "mhte_flat_host.h"
#include "mhte_dense_opt_host.h"
#include "mhte_ffm_host.h"
#include "mhte_auc_host.h"
#include "mhte_bsm_host.h"
#include "mhte_fi_host.h"
#include "mhte_split_host.h"
#include "mhte_sharding_host.h"
#include "mhte_ckpt_host.h"

struct mhte_multi_step {
  mhte::MultiStep ms;
  // the touched-key set's segments over the tables' unique ids, per slot, built at creation: one insert
  // call per backward however many tables there are
  std::vector<mhte::TkDesc> h_tk[2];
  mhte::TkDesc* d_tk = nullptr;   // [2][T]
  std::vector<uint8_t> tk_skip;
  ~mhte_multi_step() {
    if (d_tk) {
      (void)hipSetDevice(ms.device);
      (void)hipDeviceSynchronize();
      (void)hipFree(d_tk);
    }
  }
  bool counted = false;   // in mhte_multi_table::multi_steps
};
struct mhte_shard_step {
  mhte::ShardStep ss;
  bool counted = false;   // in mhte_multi_table::shard_steps
};
struct mhte_dense_mlp {
  mhte::DenseMlp m;
};

using namespace mhte;

extern "C" {

const char* mhte_last_error(void) { return g_last_error.c_str(); }
int32_t mhte_abi_version(void) { return MHTE_ABI_VERSION; }

mhte_status mhte_multi_table_create(const mhte_table_config* configs, int32_t n_tables,
                                    int32_t device, const char* shared_name,
                                    mhte_multi_table** out) {
  return guard([&] {
    if (!configs || n_tables <= 0 || !out)
      throw Error(MHTE_INVALID_ARGUMENT, "create: bad arguments");
    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev <= 0)
      throw Error(MHTE_UNAVAILABLE, "no HIP device: the MI355X engine has no CPU fallback");
    if (device < 0 || device >= ndev)
      throw Error(MHTE_INVALID_ARGUMENT, "device ordinal out of range");
    HIP_OK(hipSetDevice(device));
    std::unique_ptr<mhte_multi_table> mt(new mhte_multi_table);
    mt->device = device;
    mt->shared_name = shared_name ? shared_name : "";
    std::vector<int> order(n_tables);
    for (int i = 0; i < n_tables; ++i) order[i] = i;
    std::sort(order.begin(), order.end(), [&](int a, int b) {
      return std::string(configs[a].name ? configs[a].name : "") <
             std::string(configs[b].name ? configs[b].name : "");
    });
    for (int i = 0; i < n_tables; ++i) {
      if (i > 0 && std::string(configs[order[i]].name ? configs[order[i]].name : "") ==
                       std::string(configs[order[i - 1]].name ? configs[order[i - 1]].name : ""))
        throw Error(MHTE_INVALID_ARGUMENT, "duplicate table name");
      std::unique_ptr<Table> tb(new Table);
      tb->init(configs[order[i]], device);
      mt->tables.push_back(std::move(tb));
    }
    HIP_OK(hipDeviceSynchronize());
    *out = mt.release();
    if (!(*out)->shared_name.empty()) {
      std::lock_guard<std::mutex> g(g_registry_mu);
      g_registry[(*out)->shared_name] = *out;
    }
  });
}

void mhte_multi_table_destroy(mhte_multi_table* t) {
  if (t) {
    // (a displacement pass an id-sharded step still owes these tables: run it while they exist — the
    // step's destructor does the same if it goes first)
    try {
      (void)hipSetDevice(t->device);
      for (auto& tb : t->tables)
        if (tb->ext_flush) tb->finish_pending(nullptr);
    } catch (...) {
    }
    {
      std::lock_guard<std::mutex> link(g_touched_link_mu);
      if (t->touched) {
        std::lock_guard<std::mutex> gs(t->touched->mu);
        t->touched->owner = nullptr;
        t->touched = nullptr;
      }
      for (mhte_multi_step* ms : t->multi_steps) ms->counted = false;
      for (mhte_shard_step* ss : t->shard_steps) ss->counted = false;
    }
    std::lock_guard<std::mutex> g(g_registry_mu);
    auto it = g_registry.find(t->shared_name);
    if (it != g_registry.end() && it->second == t) g_registry.erase(it);
  }
  delete t;
}

mhte_multi_table* mhte_multi_table_find(const char* shared_name) {
  if (!shared_name) return nullptr;
  std::lock_guard<std::mutex> g(g_registry_mu);
  auto it = g_registry.find(shared_name);
  return it == g_registry.end() ? nullptr : it->second;
}
int32_t mhte_multi_table_is_initialized(const char* shared_name) {
  return mhte_multi_table_find(shared_name) ? 1 : 0;
}
void mhte_advance_clock_for_testing(double seconds) { g_clock_offset.store(g_clock_offset.load() + seconds); }
int32_t mhte_num_tables(const mhte_multi_table* t) { return t ? int32_t(t->tables.size()) : 0; }
const char* mhte_table_name(const mhte_multi_table* t, int32_t i) {
  return (t && i >= 0 && i < int32_t(t->tables.size())) ? t->tables[i]->name.c_str() : "";
}
int32_t mhte_table_dim(const mhte_multi_table* t, int32_t i) {
  return (t && i >= 0 && i < int32_t(t->tables.size())) ? int32_t(t->tables[i]->dim) : -1;
}
int32_t mhte_table_slice_size(const mhte_multi_table* t, int32_t i) {
  return (t && i >= 0 && i < int32_t(t->tables.size())) ? int32_t(t->tables[i]->nseg) : -1;
}
int32_t mhte_table_row_floats(const mhte_multi_table* t, int32_t i) {
  return (t && i >= 0 && i < int32_t(t->tables.size())) ? int32_t(t->tables[i]->row_floats) : -1;
}
int32_t mhte_table_index(const mhte_multi_table* t, const char* name) {
  if (!t || !name) return -1;
  for (size_t i = 0; i < t->tables.size(); ++i)
    if (t->tables[i]->name == name) return int32_t(i);
  return -1;
}
const char* mhte_shared_name(const mhte_multi_table* t) { return t ? t->shared_name.c_str() : ""; }

mhte_status mhte_lookup(mhte_multi_table* t, const int64_t* id, const int64_t* id_split,
                        int64_t n_split, float* embedding, int64_t embedding_len, void* stream) {
  return guard([&] {
    check_handle(t);
    if (!id_split || n_split != int64_t(t->tables.size()) + 1)
      throw Error(MHTE_INVALID_ARGUMENT, "table size: " + std::to_string(t->tables.size()) +
                                             ". Error id_split size: " + std::to_string(n_split));
    HIP_OK(hipSetDevice(t->device));
    int64_t emb_size = 0;
    for (size_t i = 0; i < t->tables.size(); ++i) {
      if (id_split[i + 1] < id_split[i]) throw Error(MHTE_INVALID_ARGUMENT, "id_split not monotonic");
      emb_size += (id_split[i + 1] - id_split[i]) * t->tables[i]->dim;
    }
    if (emb_size > embedding_len)
      throw Error(MHTE_INVALID_ARGUMENT, "embedding buffer too short: need " +
                                             std::to_string(emb_size));
    int64_t off = 0;
    for (size_t i = 0; i < t->tables.size(); ++i) {
      Table& tb = *t->tables[i];
      const int64_t num_ids = id_split[i + 1] - id_split[i];
      std::lock_guard<std::mutex> g(tb.mu);
      tb.lookup(id + id_split[i], num_ids, nullptr, embedding + off, S(stream));
      off += num_ids * tb.dim;
    }
  });
}

mhte_status mhte_optimize(mhte_multi_table* t, const int64_t* id, const int64_t* id_split,
                          int64_t n_split, const float* value, int64_t value_len,
                          const float* learning_rate, int64_t n_learning_rate, int64_t update_time,
                          int64_t global_step, int32_t flags, void* stream) {
  return guard([&] {
    mhte::t_global_step = global_step;  // (batch softmax)
    if (!learning_rate) throw Error(MHTE_INVALID_ARGUMENT, "learning_rate is null");
    ragged_upsert<kOpOptimize>(t, id, id_split, n_split, value, value_len, learning_rate,
                               n_learning_rate, update_time, flags, stream);
  });
}

mhte_status mhte_assign(mhte_multi_table* t, const int64_t* id, const int64_t* id_split,
                        int64_t n_split, const float* value, int64_t value_len, int64_t update_time,
                        int32_t flags, void* stream) {
  return guard([&] {
    ragged_upsert<kOpAssign>(t, id, id_split, n_split, value, value_len, nullptr, 0, update_time,
                             flags, stream);
  });
}

mhte_status mhte_assign_add(mhte_multi_table* t, const int64_t* id, const int64_t* id_split,
                            int64_t n_split, const float* value, int64_t value_len,
                            int64_t update_time, int32_t flags, void* stream) {
  return guard([&] {
    ragged_upsert<kOpAssignAdd>(t, id, id_split, n_split, value, value_len, nullptr, 0, update_time,
                                flags, stream);
  });
}

mhte_status mhte_reinitialize(mhte_multi_table* t, const char* table_name, const int64_t* id,
                              int64_t n, int32_t* id_status, int64_t now, void* stream) {
  return guard([&] {
    check_handle(t);
    HIP_OK(hipSetDevice(t->device));
    if (n <= 0) return;
    // -1: table_name does not exist (not an error, multi_hash_table_update_op.cc:209-220)
    HIP_OK(hipMemsetAsync(id_status, 0xff, sizeof(int32_t) * n, S(stream)));
    const int32_t idx = mhte_table_index(t, table_name);
    if (idx < 0) {
      fprintf(stderr, "[mhte] table %s does not exist!\n", table_name ? table_name : "(null)");
      return;
    }
    Table& tb = *t->tables[idx];
    if (now == 0) {
      now = std::chrono::duration_cast<std::chrono::seconds>(
                std::chrono::system_clock::now().time_since_epoch()).count();
    }
    std::lock_guard<std::mutex> g(tb.mu);
    tb.upsert<kOpReinit>(id, n, nullptr, nullptr, nullptr, now, 0, id_status, S(stream));
    tk_record(t, tb, idx, id, n, nullptr, S(stream));
  });
}

mhte_status mhte_compute_fused_offsets(const mhte_multi_table* t, const int32_t* fused_slot_size,
                                       int32_t num_of_shards, int32_t* id_offsets,
                                       int32_t* embedding_offsets, int32_t* embedding_splits,
                                       int64_t* total_ids, int64_t* total_embeddings) {
  return guard([&] {
    check_handle(t);
    if (!fused_slot_size || num_of_shards <= 0)
      throw Error(MHTE_INVALID_ARGUMENT, "fused offsets: bad arguments");
    const int T = int(t->tables.size());
    int64_t tk = 0, te = 0, prev = 0;
    if (id_offsets) id_offsets[0] = 0;
    if (embedding_offsets) embedding_offsets[0] = 0;
    for (int s = 0; s < num_of_shards; ++s) {
      for (int k = 0; k < T; ++k) {
        const int idx = T * s + k;
        const int sz = fused_slot_size[idx];
        if (sz < 0) throw Error(MHTE_INVALID_ARGUMENT, "negative fused_slot_size");
        tk += sz;
        te += int64_t(sz) * t->tables[k]->dim;
        if (te > INT32_MAX) throw Error(MHTE_INVALID_ARGUMENT, "fused embedding size exceeds int32");
        if (id_offsets) id_offsets[idx + 1] = int32_t(tk);
        if (embedding_offsets) embedding_offsets[idx + 1] = int32_t(te);
      }
      if (embedding_splits) embedding_splits[s] = int32_t(te - prev);
      prev = te;
    }
    if (total_ids) *total_ids = tk;
    if (total_embeddings) *total_embeddings = te;
  });
}

mhte_status mhte_fused_lookup(mhte_multi_table* t, const int64_t* ids,
                              const int32_t* fused_slot_size, int32_t num_of_shards,
                              int64_t req_time, float* embeddings, int64_t embeddings_len,
                              int32_t* embedding_splits, int32_t* id_offsets,
                              int32_t* embedding_offsets, void* stream) {
  (void)req_time;
  return guard([&] {
    check_handle(t);
    const int T = int(t->tables.size());
    std::vector<int32_t> ko(size_t(T) * num_of_shards + 1), eo(size_t(T) * num_of_shards + 1),
        es(num_of_shards);
    int64_t tk = 0, te = 0;
    mhte_status st = mhte_compute_fused_offsets(t, fused_slot_size, num_of_shards, ko.data(),
                                                eo.data(), es.data(), &tk, &te);
    if (st != MHTE_OK) throw Error(st, g_last_error);
    if (te > embeddings_len)
      throw Error(MHTE_INVALID_ARGUMENT, "embeddings buffer too short: need " + std::to_string(te));
    HIP_OK(hipSetDevice(t->device));
    if (seg_kernels_ok(t) && aligned16(embeddings)) {
      // ONE launch over the [shard][table] segments (mhte_mstep_kernels.h)
      std::vector<std::unique_lock<std::mutex>> locks;
      for (auto& tb : t->tables) locks.emplace_back(tb->mu);
      fused_lookup_segments(t, ids, ko.data(), eo.data(), T * num_of_shards, embeddings, S(stream));
    } else {
      for (int s = 0; s < num_of_shards; ++s) {
        for (int k = 0; k < T; ++k) {
          const int idx = s * T + k;
          Table& tb = *t->tables[k];
          std::lock_guard<std::mutex> g(tb.mu);
          tb.lookup(ids + ko[idx], fused_slot_size[idx], nullptr, embeddings + eo[idx], S(stream));
        }
      }
    }
    if (embedding_splits) memcpy(embedding_splits, es.data(), sizeof(int32_t) * es.size());
    if (id_offsets) memcpy(id_offsets, ko.data(), sizeof(int32_t) * ko.size());
    if (embedding_offsets) memcpy(embedding_offsets, eo.data(), sizeof(int32_t) * eo.size());
  });
}

mhte_status mhte_fused_optimize(mhte_multi_table* t, const int64_t* ids,
                                const int32_t* fused_slot_size, const float* id_grads,
                                int64_t id_grads_len, const int32_t* id_offsets,
                                const int32_t* grad_offsets, const float* learning_rates,
                                int64_t n_learning_rates, int64_t req_time, int64_t global_step,
                                int32_t num_of_shards, int32_t flags, void* stream) {
  return guard([&] {
    mhte::t_global_step = global_step;
    check_handle(t);
    if (!fused_slot_size || !id_offsets || !grad_offsets || !learning_rates)
      throw Error(MHTE_INVALID_ARGUMENT, "fused optimize: null argument");
    const int T = int(t->tables.size());
    int64_t need_lr = 0;
    for (int k = 0; k < T; ++k) need_lr += t->tables[k]->nseg;
    if (need_lr > n_learning_rates)
      throw Error(MHTE_INVALID_ARGUMENT, "learning_rate_tensors too short");
    HIP_OK(hipSetDevice(t->device));
    for (int idx = 0; idx < T * num_of_shards; ++idx) {
      if (fused_slot_size[idx] < 0) throw Error(MHTE_INVALID_ARGUMENT, "negative fused_slot_size");
      if (int64_t(grad_offsets[idx]) + int64_t(fused_slot_size[idx]) * t->tables[idx % T]->dim > id_grads_len)
        throw Error(MHTE_INVALID_ARGUMENT, "id_grads too short");
    }
    bool filtered = false;
    for (auto& tb : t->tables) filtered = filtered || tb->flt_slots != nullptr;
    if ((flags & MHTE_IDS_UNIQUE) && !filtered && seg_kernels_ok(t) && aligned16(id_grads)) {
      // ids distinct inside every segment (the caller's FusedReorderByIndices deduplicated them):
      // ONE upsert launch over the segments + the displacement pass
      std::vector<std::unique_lock<std::mutex>> locks;
      for (auto& tb : t->tables) locks.emplace_back(tb->mu);
      fused_optimize_segments(t, ids, fused_slot_size, id_grads, id_offsets, grad_offsets,
                              learning_rates, req_time, global_step, num_of_shards, S(stream));
      for (int idx = 0; t->touched && idx < T * num_of_shards; ++idx)
        tk_record(t, *t->tables[idx % T], idx % T, ids + id_offsets[idx], fused_slot_size[idx], nullptr,
                  S(stream));
      return;
    }
    for (int s = 0; s < num_of_shards; ++s) {
      int64_t lr_off = 0;  // restarts per shard, multi_hash_table_update_op.cc:285-293
      for (int k = 0; k < T; ++k) {
        const int idx = s * T + k;
        Table& tb = *t->tables[k];
        const float* lrs = learning_rates + lr_off;
        lr_off += tb.nseg;
        const int64_t n = fused_slot_size[idx];
        if (int64_t(grad_offsets[idx]) + n * tb.dim > id_grads_len)
          throw Error(MHTE_INVALID_ARGUMENT, "id_grads too short");
        std::lock_guard<std::mutex> g(tb.mu);
        tb.note_update_time(req_time);
        tb.upsert<kOpOptimize>(ids + id_offsets[idx], n, nullptr, id_grads + grad_offsets[idx], lrs,
                               req_time, flags, nullptr, S(stream));
        if (s == num_of_shards - 1) tb.maybe_evict(S(stream));
        tk_record(t, tb, k, ids + id_offsets[idx], n, nullptr, S(stream));
      }
    }
  });
}

mhte_status mhte_table_size(mhte_multi_table* t, int32_t table, int64_t* size, void* stream) {
  return guard([&] {
    Table& tb = table_at(t, table);
    HIP_OK(hipSetDevice(t->device));
    std::lock_guard<std::mutex> g(tb.mu);
    tb.sync_counters(S(stream));
    *size = tb.live_keys() + (tb.h_ctr->special_state ? 1 : 0);
  });
}


mhte_status mhte_table_contains(mhte_multi_table* t, int32_t table, const int64_t* id, int64_t n,
                                int32_t* out, void* stream) {
  return guard([&] {
    Table& tb = table_at(t, table);
    HIP_OK(hipSetDevice(t->device));
    if (n <= 0) return;
    std::lock_guard<std::mutex> g(tb.mu);
    tb.finish_pending(S(stream));
    contains_kernel<<<dim3(uint32_t((n + 255) / 256)), 256, 0, S(stream)>>>(tb.view, id, nullptr, n, out);
    HIP_OK(hipGetLastError());
  });
}

mhte_status mhte_table_evict(mhte_multi_table* t, int32_t table, int64_t max_update_time,
                             void* stream) {
  return guard([&] {
    Table& tb = table_at(t, table);
    HIP_OK(hipSetDevice(t->device));
    std::lock_guard<std::mutex> g(tb.mu);
    tb.evict(max_update_time, S(stream));
  });
}

mhte_status mhte_table_compact(mhte_multi_table* t, int32_t table, int64_t out[4], void* stream) {
  return guard([&] {
    Table& tb = table_at(t, table);
    if (!out) throw Error(MHTE_INVALID_ARGUMENT, "compact: null argument");
    HIP_OK(hipSetDevice(t->device));
    std::lock_guard<std::mutex> g(tb.mu);
    tb.compact(out, S(stream));
  });
}

mhte_status mhte_table_set_auto_compact(mhte_multi_table* t, int32_t table, double min_free_fraction) {
  return guard([&] {
    Table& tb = table_at(t, table);
    if (!(min_free_fraction >= 0.0 && min_free_fraction <= 1.0))
      throw Error(MHTE_INVALID_ARGUMENT, "set_auto_compact: min_free_fraction must be 0 (never) or in (0, 1]");
    std::lock_guard<std::mutex> g(tb.mu);
    tb.auto_compact = min_free_fraction;
  });
}

mhte_status mhte_table_get_stats(mhte_multi_table* t, int32_t table, mhte_table_stats* out,
                                 void* stream) {
  return guard([&] {
    Table& tb = table_at(t, table);
    HIP_OK(hipSetDevice(t->device));
    std::lock_guard<std::mutex> g(tb.mu);
    tb.sync_counters(S(stream));
    out->size = tb.live_keys() + (tb.h_ctr->special_state ? 1 : 0);
    out->hashpower = int32_t(tb.hp);
    out->rows_allocated = int64_t(tb.h_ctr->alloc & 0xffffffffull);
    out->lookup_hits = int64_t(tb.h_ctr->hits);
    out->dropped = tb.h_ctr->n_dropped;
    out->evicted = tb.h_ctr->n_evicted;
    out->max_update_ts = tb.max_update_ts;
    out->bytes_buckets = int64_t(sizeof(Bucket)) << tb.hp;
    out->bytes_rows = int64_t(tb.chunks.size()) * (int64_t(tb.row_floats) * 4 << tb.chunk_shift);
    unsigned long long zero = 0;
    HIP_OK(hipMemcpy(&tb.ctr->hits, &zero, sizeof(zero), hipMemcpyHostToDevice));
  });
}

mhte_status mhte_table_dump(mhte_multi_table* t, int32_t table, int64_t cap, int64_t* ids,
                            int64_t* positions, uint32_t* ts, float* rows, int64_t* n_out,
                            void* stream) {
  return guard([&] { dump_table(t, table_at(t, table), cap, ids, positions, ts, rows, n_out, S(stream)); });
}

// ---- post-exchange gather + pooling -------------------------------------------------------------
}  // extern "C"
namespace mhte {
// zeroed (gradient only): the caller has just filled `fused` with zeros — the first launch may store without
// reading the destination
template <bool GATHER>
static void fused_gather(float* fused, int32_t n_inputs, const int32_t* const* offsets,
                         const int64_t* n, const int32_t* dims, float* const* rows, float scale,
                         hipStream_t st, int64_t fused_len = int64_t(1) << 31, bool zeroed = false,
                         const float* scale_dev = nullptr) {
  if (n_inputs < 0) throw Error(MHTE_INVALID_ARGUMENT, "n_inputs must be >= 0");
  int key_bits = 1;   // (offsets are int32 and lie inside the fused buffer)
  while (key_bits < 31 && (int64_t(1) << key_bits) < fused_len) ++key_bits;
  for (int32_t i0 = 0; i0 < n_inputs; i0 += kMaxGatherInputs) {
    GatherInputs in{};
    in.n_inputs = std::min<int32_t>(kMaxGatherInputs, n_inputs - i0);
    int64_t acc = 0;
    for (int32_t k = 0; k < in.n_inputs; ++k) {
      if (n[i0 + k] < 0 || dims[i0 + k] <= 0)
        throw Error(MHTE_INVALID_ARGUMENT, "fused gather: bad size or dim of input " + std::to_string(i0 + k));
      in.offsets[k] = offsets[i0 + k];
      in.rows[k] = rows[i0 + k];
      in.dim[k] = dims[i0 + k];
      in.start[k] = acc;
      acc += n[i0 + k];
    }
    in.start[in.n_inputs] = acc;
    in.aligned = aligned16(fused) ? 1 : 0;
    for (int32_t k = 0; k < in.n_inputs; ++k)
      if (!aligned16(in.rows[k])) in.aligned = 0;
    if (acc == 0) continue;
    if (!GATHER && !pool_atomics()) {
      // the gradient without atomics: rows that share an offset are grouped and added in row order
      AuxWs& ws = AuxWs::of(current_device());
      std::lock_guard<std::mutex> g(ws.mu);
      AuxWs::Use use_(ws, st);
      ws.keys.reserve(size_t(acc));
      gather_keys_kernel<<<dim3(uint32_t((acc + 255) / 256)), 256, 0, st>>>(in, ws.keys.p);
      ws.group_sorted(ws.keys.p, acc, key_bits, st);   // (a key is a float offset into the fused buffer)
      bool vec = in.aligned != 0;
      for (int32_t k = 0; k < in.n_inputs; ++k) vec = vec && (in.dim[k] & 3) == 0;
      // (scale_dev: the factor is a device word, read by every workgroup — the same kernels otherwise)
      const dim3 gv(uint32_t(((acc + kGatherGradKeys - 1) / kGatherGradKeys * 16 + 255) / 256)), gs(uint32_t((acc * 8 + 255) / 256));
      const int fresh = (zeroed && i0 == 0) ? 1 : 0;
      if (vec && !scale_dev)
        gather_grad_lists_vec_kernel<false><<<gv, 256, 0, st>>>(
            fused, in, scale, ws.uids.p, ws.nu.p, ws.seg_off.p, ws.seg_pos.p, fresh, nullptr);
      else if (vec)
        gather_grad_lists_vec_kernel<true><<<gv, 256, 0, st>>>(
            fused, in, scale, ws.uids.p, ws.nu.p, ws.seg_off.p, ws.seg_pos.p, fresh, scale_dev);
      else if (!scale_dev)
        gather_grad_lists_kernel<false><<<gs, 256, 0, st>>>(
            fused, in, scale, ws.uids.p, ws.nu.p, ws.seg_off.p, ws.seg_pos.p, nullptr);
      else
        gather_grad_lists_kernel<true><<<gs, 256, 0, st>>>(
            fused, in, scale, ws.uids.p, ws.nu.p, ws.seg_off.p, ws.seg_pos.p, scale_dev);
      HIP_OK(hipGetLastError());
      continue;
    }
    const dim3 grid(uint32_t((acc * 8 + 255) / 256));
    if constexpr (!GATHER) {   // (the forward gather has no scale: no <true, true> instantiation)
      if (scale_dev) {
        fused_gather_kernel<false, true><<<grid, 256, 0, st>>>(fused, in, scale, scale_dev);
        HIP_OK(hipGetLastError());
        continue;
      }
    }
    fused_gather_kernel<GATHER, false><<<grid, 256, 0, st>>>(fused, in, scale, nullptr);
    HIP_OK(hipGetLastError());
  }
}
// scale_dev != NULL: the factor is read on the device (scale is then not used)
static void fused_gather_gradient(float* fused_grad, int64_t fused_len, int32_t n_inputs, const float* const* grads,
                                  const int32_t* const* offsets, const int64_t* n, const int32_t* dims, float scale,
                                  const float* scale_dev, hipStream_t st) {
  if (fused_len < 0) throw Error(MHTE_INVALID_ARGUMENT, "fused_len must be >= 0");
  if (fused_len) {   // (16-byte stores from a full grid: hipMemsetAsync moves a large buffer at 1.3 TB/s)
    LayoutZeroArgs Z{};
    Z.p[0] = fused_grad;
    Z.len[0] = uint64_t(fused_len);
    const uint32_t gx = uint32_t(std::min<uint64_t>(2048, (uint64_t(fused_len) + 4095) / 4096));
    layout_zero_args_kernel<<<dim3(gx, 1), 256, 0, st>>>(Z);
    HIP_OK(hipGetLastError());
  }
  fused_gather<false>(fused_grad, n_inputs, offsets, n, dims, const_cast<float* const*>(grads), scale, st,
                      fused_len > 0 ? fused_len : 1, /*zeroed=*/fused_len > 0, scale_dev);
}
}  // namespace mhte
extern "C" {

mhte_status mhte_fused_gather_embeddings_by_input(const float* fused_embeddings, int32_t n_inputs,
                                                  const int32_t* const* offsets, const int64_t* n,
                                                  const int32_t* dims, float* const* outputs,
                                                  void* stream) {
  return guard([&] {
    fused_gather<true>(const_cast<float*>(fused_embeddings), n_inputs, offsets, n, dims, outputs, 1.f,
                       S(stream));
  });
}

mhte_status mhte_fused_gather_embeddings_by_input_gradient(float* fused_grad, int64_t fused_len,
                                                           int32_t n_inputs,
                                                           const float* const* grads,
                                                           const int32_t* const* offsets,
                                                           const int64_t* n, const int32_t* dims,
                                                           float scale, void* stream) {
  return guard([&] {
    fused_gather_gradient(fused_grad, fused_len, n_inputs, grads, offsets, n, dims, scale, nullptr, S(stream));
  });
}

mhte_status mhte_fused_gather_embeddings_by_input_gradient_dev_scale(float* fused_grad, int64_t fused_len,
                                                                     int32_t n_inputs,
                                                                     const float* const* grads,
                                                                     const int32_t* const* offsets,
                                                                     const int64_t* n, const int32_t* dims,
                                                                     const float* scale_dev, void* stream) {
  return guard([&] {
    if (!scale_dev)
      throw Error(MHTE_INVALID_ARGUMENT, "fused_gather_embeddings_by_input_gradient_dev_scale: null argument: scale_dev");
    fused_gather_gradient(fused_grad, fused_len, n_inputs, grads, offsets, n, dims, 1.f, scale_dev, S(stream));
  });
}

// ---- clip by global norm (csrc/mhte_clip_kernels.h, mhte_clip_host.h) --------------------------------
mhte_status mhte_global_l2_reduce(const float* const* tensors, const int64_t* lens, int32_t n, float clip_norm,
                                  float* result, void* stream) {
  return guard([&] {
    const char* op = "global_l2_reduce";
    if (!tensors) arg_bad(op, "null argument: tensors");
    if (!lens) arg_bad(op, "null argument: lens");
    if (!result) arg_bad(op, "null argument: result");
    clip_check(op, tensors, "tensors", nullptr, lens, n, true, clip_norm);
    need_device();
    ClipTable T;
    clip_entries(T, op, tensors, nullptr, lens, n, false);
    clip_norm_launch(T, clip_norm, result, /*fused=*/false, S(stream));
  });
}

mhte_status mhte_clip_by_global_norm(const float* const* inputs, float* const* outputs, const int64_t* lens,
                                     int32_t n, float global_norm, float clip_norm, void* stream) {
  return guard([&] {
    const char* op = "clip_by_global_norm";
    if (!inputs) arg_bad(op, "null argument: inputs");
    if (!outputs) arg_bad(op, "null argument: outputs");
    if (!lens) arg_bad(op, "null argument: lens");
    clip_check(op, inputs, "inputs", outputs, lens, n, true, clip_norm);
    need_device();
    // clip_by_global_norm.h:42-43 on the host; not clipped: tensors that are in place take no part at all
    const float scale = global_norm > clip_norm ? clip_norm / global_norm : 1.0f;
    ClipTable T;
    clip_entries(T, op, inputs, outputs, lens, n, /*skip_inplace=*/scale == 1.0f);
    clip_scale_launch(T, kClipScaleArg, scale, nullptr, clip_norm, S(stream));
  });
}

mhte_status mhte_clip_by_global_norm_dev(const float* const* inputs, float* const* outputs, const int64_t* lens,
                                         int32_t n, const float* global_norm_dev, float clip_norm, void* stream) {
  return guard([&] {
    const char* op = "clip_by_global_norm_dev";
    if (!inputs) arg_bad(op, "null argument: inputs");
    if (!outputs) arg_bad(op, "null argument: outputs");
    if (!lens) arg_bad(op, "null argument: lens");
    if (!global_norm_dev) arg_bad(op, "null argument: global_norm_dev");
    clip_check(op, inputs, "inputs", outputs, lens, n, true, clip_norm);
    need_device();
    ClipTable T;
    clip_entries(T, op, inputs, outputs, lens, n, false);
    clip_scale_launch(T, kClipScaleNorm, 1.f, global_norm_dev, clip_norm, S(stream));
  });
}

mhte_status mhte_clip_by_global_norm_fused(const float* const* inputs, float* const* outputs, const int64_t* lens,
                                           int32_t n, float clip_norm, float* result, void* stream) {
  return guard([&] {
    const char* op = "clip_by_global_norm_fused";
    if (!inputs) arg_bad(op, "null argument: inputs");
    if (!outputs) arg_bad(op, "null argument: outputs");
    if (!lens) arg_bad(op, "null argument: lens");
    if (!result) arg_bad(op, "null argument: result");
    clip_check(op, inputs, "inputs", outputs, lens, n, true, clip_norm);
    need_device();
    ClipTable T;
    clip_entries(T, op, inputs, outputs, lens, n, false);
    clip_norm_launch(T, clip_norm, result, /*fused=*/true, S(stream));
  });
}

mhte_status mhte_scale_tensors_dev(const float* const* inputs, float* const* outputs, const int64_t* lens,
                                   int32_t n, const float* scale_dev, void* stream) {
  return guard([&] {
    const char* op = "scale_tensors_dev";
    if (!inputs) arg_bad(op, "null argument: inputs");
    if (!outputs) arg_bad(op, "null argument: outputs");
    if (!lens) arg_bad(op, "null argument: lens");
    if (!scale_dev) arg_bad(op, "null argument: scale_dev");
    clip_check(op, inputs, "inputs", outputs, lens, n, false, 0.f);
    need_device();
    ClipTable T;
    clip_entries(T, op, inputs, outputs, lens, n, false);
    clip_scale_launch(T, kClipScaleWord, 1.f, scale_dev, 0.f, S(stream));
  });
}

// ---- aligned flat concat / split (csrc/mhte_flat_kernels.h, mhte_flat_host.h) -------------------------
mhte_status mhte_aligned_flat_offsets(const int64_t* lens, int32_t n, int32_t align_elems, int64_t* offsets) {
  return guard([&] {
    const char* op = "aligned_flat_offsets";
    if (!lens) arg_bad(op, "null argument: lens");
    if (!offsets) arg_bad(op, "null argument: offsets");
    check_lens(op, "tensor", lens, n);
    flat_check_align(op, align_elems);
    (void)flat_offsets(op, lens, n, align_elems, offsets);
  });
}

mhte_status mhte_aligned_flat_concat(const float* const* inputs, const int64_t* lens, int32_t n, int32_t align_elems,
                                     float scale, const float* scale_dev, int32_t wire, void* out, int64_t out_elems,
                                     void* stream) {
  return guard([&] {
    const char* op = "aligned_flat_concat";
    if (!inputs) arg_bad(op, "null argument: inputs");
    if (!lens) arg_bad(op, "null argument: lens");
    clip_check(op, inputs, "inputs", nullptr, lens, n, false, 0.f);
    flat_check_align(op, align_elems);
    if (wire != 0 && wire != 1) arg_bad(op, "wire must be 0 (fp32) or 1 (fp16), got " + std::to_string(wire));
    const int64_t total = flat_offsets(op, lens, n, align_elems, nullptr);
    if (out_elems != total)
      arg_bad(op, "out_elems must be the aligned total " + std::to_string(total) + ", got " + std::to_string(out_elems));
    if (total && !out) arg_bad(op, "null argument: out");
    if (!aligned16(out)) arg_bad(op, "out must be 16-byte aligned");
    FlatTable T;
    flat_entries(T, op, inputs, lens, n, align_elems);
    need_device();
    flat_concat_launch(T, scale, scale_dev, wire, out, S(stream));
  });
}

mhte_status mhte_aligned_flat_decode(const void* flat, int32_t wire, int64_t total_elems, float post_scale, float* out,
                                     void* stream) {
  return guard([&] {
    const char* op = "aligned_flat_decode";
    if (total_elems < 0) arg_bad(op, "total_elems must be >= 0, got " + std::to_string(total_elems));
    if (wire != 0 && wire != 1) arg_bad(op, "wire must be 0 (fp32) or 1 (fp16), got " + std::to_string(wire));
    if (total_elems && !flat) arg_bad(op, "null argument: flat");
    if (total_elems && !out) arg_bad(op, "null argument: out");
    if (wire == 1 && total_elems && static_cast<const void*>(out) == flat)
      arg_bad(op, "an fp16 flat buffer is not decoded in place");
    need_device();
    flat_decode_launch(flat, wire, total_elems, post_scale, out, S(stream));
  });
}

// ---- dense optimizers (csrc/mhte_dense_opt_core.h, mhte_dense_opt_kernels.h, mhte_dense_opt_host.h) ---
mhte_status mhte_dense_apply_adamom(float* const* vars, const int64_t* lens, int32_t n, int32_t align_elems, float* m,
                                    float* v, float* c, int64_t slot_elems, const float* const* grads,
                                    const void* grads_flat, int32_t wire, float grad_scale,
                                    const float* grad_scale_dev, float lr, const float* lr_dev, float ada_decay,
                                    float mom_decay, float epsilon, float weight_decay, int32_t update_slots,
                                    int32_t use_v2, void* stream) {
  return guard([&] {
    const DenseOptCall q{vars, lens, n, align_elems, m, v, c, slot_elems, grads, grads_flat, wire,
                         grad_scale_dev, lr_dev, update_slots, use_v2};
    DenseOptTable T;
    dense_opt_check("dense_apply_adamom", q, /*c_needed=*/true, T);
    need_device();
    const DenseOptHyper h{grad_scale, lr, ada_decay, mom_decay, epsilon, weight_decay};
    dense_opt_launch<kDenseAdamom>(T, q, h, S(stream));
  });
}

mhte_status mhte_dense_apply_rmsprop(float* const* vars, const int64_t* lens, int32_t n, int32_t align_elems, float* m,
                                     float* v, int64_t slot_elems, const float* const* grads, const void* grads_flat,
                                     int32_t wire, float grad_scale, const float* grad_scale_dev, float lr,
                                     const float* lr_dev, float beta1, float beta2, float epsilon, float weight_decay,
                                     int32_t update_slots, int32_t use_v2, void* stream) {
  return guard([&] {
    const DenseOptCall q{vars, lens, n, align_elems, m, v, nullptr, slot_elems, grads, grads_flat, wire,
                         grad_scale_dev, lr_dev, update_slots, use_v2};
    DenseOptTable T;
    dense_opt_check("dense_apply_rmsprop", q, /*c_needed=*/false, T);
    need_device();
    if (!update_slots) return;   // (training_ops.cc:45, :66: without update_slots the op changes nothing)
    const DenseOptHyper h{grad_scale, lr, beta1, beta2, epsilon, weight_decay};
    dense_opt_launch<kDenseRmsprop>(T, q, h, S(stream));
  });
}

// ---- FFM feature cross (csrc/mhte_ffm_core.h, mhte_ffm_kernels.h, mhte_ffm_host.h) ---------------------
mhte_status mhte_ffm(const float* left, int64_t left_cols, const float* right, int64_t right_cols, int64_t batch,
                     int32_t dim_size, int32_t int_type, float* out, int64_t out_cols, void* stream) {
  return guard([&] {
    ffm_forward(left, left_cols, right, right_cols, batch, dim_size, int_type, out, out_cols, stream);
  });
}

mhte_status mhte_ffm_grad(const float* grad, int64_t grad_cols, const float* left, int64_t left_cols,
                          const float* right, int64_t right_cols, int64_t batch, int32_t dim_size, int32_t int_type,
                          float* left_grad, float* right_grad, void* stream) {
  return guard([&] {
    ffm_gradient(grad, grad_cols, left, left_cols, right, right_cols, batch, dim_size, int_type, left_grad,
                 right_grad, stream);
  });
}

mhte_status mhte_ffm_launch_counts(int64_t* out, int32_t n) {
  return guard([&] {
    if (!out) arg_bad("ffm_launch_counts", "null argument: out");
    if (n != kFfmCounters)
      arg_bad("ffm_launch_counts", "n must be " + std::to_string(kFfmCounters) + ", got " + std::to_string(n));
    for (int i = 0; i < kFfmCounters; ++i) out[i] = g_ffm_launches[i].load(std::memory_order_relaxed);
  });
}

// ---- in-batch AUC loss (csrc/mhte_auc_core.h, mhte_auc_kernels.h, mhte_auc_host.h) ---------------------
mhte_status mhte_inbatch_auc_loss(const float* label, const float* logit, int64_t n, float neg_weight, float* loss,
                                  float* unit_grad, void* stream) {
  return guard([&] { auc_forward(label, logit, n, neg_weight, loss, unit_grad, stream); });
}

mhte_status mhte_inbatch_auc_loss_grad(const float* label, const float* logit, int64_t n, float grad,
                                       const float* grad_dev, float neg_weight, float* logit_grad, void* stream) {
  return guard([&] { auc_gradient(label, logit, n, grad, grad_dev, neg_weight, logit_grad, stream); });
}

mhte_status mhte_inbatch_auc_launch_counts(int64_t* out, int32_t n) {
  return guard([&] {
    const char* op = "inbatch_auc_launch_counts";
    if (!out) arg_bad(op, "null argument: out");
    if (n != kAucCounters) arg_bad(op, "n must be " + std::to_string(kAucCounters) + ", got " + std::to_string(n));
    for (int i = 0; i < kAucCounters; ++i) out[i] = g_auc_launches[i].load(std::memory_order_relaxed);
  });
}

// ---- batch softmax loss (csrc/mhte_bsm_core.h, mhte_bsm_kernels.h, mhte_bsm_host.h) ----------------------
mhte_status mhte_batch_softmax_loss(const float* query, const float* item, const float* item_step_interval,
                                    const float* r, int64_t batch, int32_t dim, int32_t normalize, float temperature,
                                    float* loss, float* unit_dquery, float* unit_ditem, void* stream) {
  return guard([&] {
    bsm_forward(query, item, item_step_interval, r, batch, dim, normalize, temperature, loss, unit_dquery, unit_ditem,
                stream);
  });
}

mhte_status mhte_batch_softmax_loss_grad(const float* query, const float* item, const float* item_step_interval,
                                         const float* r, int64_t batch, int32_t dim, int32_t normalize,
                                         float temperature, float grad, const float* grad_dev, float* dquery,
                                         float* ditem, void* stream) {
  return guard([&] {
    bsm_gradient(query, item, item_step_interval, r, batch, dim, normalize, temperature, grad, grad_dev, dquery, ditem,
                 stream);
  });
}

mhte_status mhte_batch_softmax_plan(int64_t batch, int32_t dim, int64_t* out, int32_t n) {
  return guard([&] { bsm_plan_out(batch, dim, out, n); });
}

mhte_status mhte_batch_softmax_launch_counts(int64_t* out, int32_t n) {
  return guard([&] {
    const char* op = "batch_softmax_launch_counts";
    if (!out) arg_bad(op, "null argument: out");
    if (n != kBsmCounters) arg_bad(op, "n must be " + std::to_string(kBsmCounters) + ", got " + std::to_string(n));
    for (int i = 0; i < kBsmCounters; ++i) out[i] = g_bsm_launches[i].load(std::memory_order_relaxed);
  });
}

// ---- FeatureInsight (csrc/mhte_fi_core.h, mhte_fi_kernels.h, mhte_fi_host.h) -----------------------------
mhte_status mhte_feature_insight(const float* input, const float* weight, int64_t batch, int64_t in_cols, int32_t k,
                                 const int32_t* segment_sizes, int32_t n_segments, int32_t aggregate, float* out,
                                 int64_t out_cols, void* stream) {
  return guard([&] {
    fi_forward(input, weight, batch, in_cols, k, segment_sizes, n_segments, aggregate, out, out_cols, stream);
  });
}

mhte_status mhte_feature_insight_grad(const float* grad, int64_t grad_cols, const float* input, const float* weight,
                                      int64_t batch, int64_t in_cols, int32_t k, const int32_t* segment_sizes,
                                      int32_t n_segments, float* input_grad, float* weight_grad, void* stream) {
  return guard([&] {
    fi_gradient(grad, grad_cols, input, weight, batch, in_cols, k, segment_sizes, n_segments, input_grad, weight_grad,
                stream);
  });
}

mhte_status mhte_feature_insight_plan(int64_t batch, int64_t in_cols, int32_t k, int32_t n_segments, int64_t* out,
                                      int32_t n) {
  return guard([&] { fi_plan_out(batch, in_cols, k, n_segments, out, n); });
}

mhte_status mhte_feature_insight_launch_counts(int64_t* out, int32_t n) {
  return guard([&] {
    const char* op = "feature_insight_launch_counts";
    if (!out) arg_bad(op, "null argument: out");
    if (n != kFiCounters) arg_bad(op, "n must be " + std::to_string(kFiCounters) + ", got " + std::to_string(n));
    for (int i = 0; i < kFiCounters; ++i) out[i] = g_fi_launches[i].load(std::memory_order_relaxed);
  });
}

// ---- split by indices (csrc/mhte_split_kernels.h, mhte_split_host.h) -----------------------------------
mhte_status mhte_split_plan(const int64_t* indices, int64_t n, int32_t num_splits, const int64_t* row_splits,
                            int32_t n_row_splits, int64_t* pos, int64_t* sizes, int64_t* split_row_splits,
                            int64_t* n_bad, int64_t* host_out, void* stream) {
  return guard([&] {
    split_plan(indices, n, num_splits, row_splits, n_row_splits, pos, sizes, split_row_splits, n_bad, host_out,
               stream);
  });
}

mhte_status mhte_split_rows(const void* input, int64_t n, int64_t element_size, int32_t elem_bytes,
                            const int64_t* pos, void* packed, void* stream) {
  return guard([&] { split_rows(input, n, element_size, elem_bytes, pos, packed, stream); });
}

mhte_status mhte_split_rows_grad(const void* const* grads, const int64_t* sizes, int32_t num_splits, int64_t n,
                                 int64_t element_size, int32_t elem_bytes, const int64_t* pos, void* input_grads,
                                 void* stream) {
  return guard([&] {
    split_rows_grad(grads, sizes, num_splits, n, element_size, elem_bytes, pos, input_grads, stream);
  });
}

mhte_status mhte_split_launch_counts(int64_t* out, int32_t n) {
  return guard([&] {
    if (!out) arg_bad("split_launch_counts", "null argument: out");
    if (n != kSplitCounters)
      arg_bad("split_launch_counts", "n must be " + std::to_string(kSplitCounters) + ", got " + std::to_string(n));
    for (int i = 0; i < kSplitCounters; ++i) out[i] = g_split_launches[i].load(std::memory_order_relaxed);
  });
}

// ---- the fused-layout packer (csrc/mhte_sharding_plan.h, mhte_sharding_kernels.h, mhte_sharding_host.h) --
mhte_status mhte_sharding_sparse_fids(const mhte_shard_feature* features, int32_t n_features,
                                      const int32_t* table_feature_count, int32_t n_tables, int32_t ps_num,
                                      int32_t unique, uint64_t* fid_offset, int32_t* feature_offset,
                                      uint32_t* nfl_offset, int64_t* fid_list, int64_t* key_start,
                                      int64_t* row_splits_flat, int64_t* list_bounds, int64_t* host_out,
                                      void* stream) {
  return guard([&] {
    sharding_sparse_fids(features, n_features, table_feature_count, n_tables, ps_num, unique, fid_offset,
                         feature_offset, nfl_offset, fid_list, key_start, row_splits_flat, list_bounds, host_out,
                         stream);
  });
}

mhte_status mhte_lookup_gradient(const int64_t* id_indices, int64_t n, int64_t index_cols,
                                 const int64_t* id_values, const float* input_grads, int64_t n_rows,
                                 int32_t dim, int64_t* out_ids, float* out_grads, void* stream) {
  return guard([&] {
    if (n < 0 || index_cols < 1 || n_rows < 0 || dim < 0)
      throw Error(MHTE_INVALID_ARGUMENT, "lookup_gradient: bad shape");
    if (n == 0) return;
    if (!id_indices || !id_values || !out_ids || (dim > 0 && (!input_grads || !out_grads)))
      throw Error(MHTE_INVALID_ARGUMENT, "lookup_gradient: null argument");
    hipStream_t st = S(stream);
    static thread_local DevBuf<uint32_t> flag;
    flag.reserve(1);
    HIP_OK(hipMemsetAsync(flag.p, 0, sizeof(uint32_t), st));
    const int32_t vec4 = (dim % 4 == 0 && aligned16(input_grads) && aligned16(out_grads)) ? 1 : 0;
    const uint32_t grid = uint32_t(std::min<int64_t>((n * 8 + 255) / 256, 1 << 16));
    lookup_gradient_kernel<<<grid, 256, 0, st>>>(id_indices, n, index_cols, id_values, input_grads, n_rows, dim,
                                                 vec4, out_ids, out_grads, flag.p);
    HIP_OK(hipGetLastError());
    uint32_t bad = 0;
    HIP_OK(hipMemcpyAsync(&bad, flag.p, sizeof(bad), hipMemcpyDeviceToHost, st));
    HIP_OK(hipStreamSynchronize(st));
    if (bad) throw Error(MHTE_INVALID_ARGUMENT, "lookup_gradient: id_indices[:, 0] holds a row outside [0, " +
                                                std::to_string(n_rows) + ")");
  });
}

mhte_status mhte_reduce_rows(const int64_t* indices, const float* values, int64_t n, int32_t dim,
                             int64_t batch, int32_t mode, int32_t indices_sorted, float* out,
                             void* stream) {
  return guard([&] {
    if (dim <= 0 || batch < 0 || n < 0 || mode < 0 || mode > 2)
      throw Error(MHTE_INVALID_ARGUMENT, "reduce_rows: bad argument");
    if (batch == 0) return;
    hipStream_t st = S(stream);
    if (indices_sorted) {
      const dim3 grid(uint32_t((batch * 16 + 255) / 256));
      if (dim % 4 == 0 && aligned16(values) && aligned16(out))
        reduce_rows_sorted_kernel<4><<<grid, 256, 0, st>>>(indices, values, n, dim, batch, mode, out);
      else
        reduce_rows_sorted_kernel<1><<<grid, 256, 0, st>>>(indices, values, n, dim, batch, mode, out);
    } else if (!pool_atomics()) {
      // indices in any order, no atomics: rows of one output are grouped and added in index order —
      // the reference's sequential loop, bit for bit.  An output no index names is 0 (sum, square
      // norm) or 0 * (1 / 0) = NaN (mean), as there.
      if (mode == 1) HIP_OK(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(out), 0x7fc00000, size_t(batch) * dim, st));
      else HIP_OK(hipMemsetAsync(out, 0, size_t(batch) * dim * sizeof(float), st));
      if (n) {
        AuxWs& ws = AuxWs::of(current_device());
        std::lock_guard<std::mutex> g(ws.mu);
        AuxWs::Use use_(ws, st);
        int bits = 1;
        while (bits < 31 && (int64_t(1) << bits) < batch) ++bits;   // (an index is a row of `out`: < batch)
        if ((int64_t(1) << bits) >= batch) ws.group_sorted(indices, n, bits, st);
        else ws.group(indices, n, st);
        const dim3 grid(uint32_t((n * 16 + 255) / 256));
        if (dim % 4 == 0 && aligned16(values) && aligned16(out))
          reduce_rows_lists_kernel<4><<<grid, 256, 0, st>>>(ws.uids.p, ws.nu.p, ws.seg_off.p, ws.seg_pos.p, values,
                                                            dim, batch, mode, out);
        else
          reduce_rows_lists_kernel<1><<<grid, 256, 0, st>>>(ws.uids.p, ws.nu.p, ws.seg_off.p, ws.seg_pos.p, values,
                                                            dim, batch, mode, out);
        HIP_OK(hipGetLastError());
      }
    } else {
      HIP_OK(hipMemsetAsync(out, 0, size_t(batch) * dim * sizeof(float), st));
      uint32_t* cnt = nullptr;
      if (mode == 1) {
        HIP_OK(hipMallocAsync(reinterpret_cast<void**>(&cnt), size_t(batch) * 4, st));
        HIP_OK(hipMemsetAsync(cnt, 0, size_t(batch) * 4, st));
      }
      if (n)
        reduce_rows_atomic_kernel<<<dim3(uint32_t((n * 16 + 255) / 256)), 256, 0, st>>>(
            indices, values, n, dim, mode, out, cnt);
      if (mode != 0)
        reduce_rows_finish_kernel<<<dim3(uint32_t((batch * dim + 255) / 256)), 256, 0, st>>>(
            out, cnt, batch, dim, mode);
      if (cnt) HIP_OK(hipFreeAsync(cnt, st));
    }
    HIP_OK(hipGetLastError());
  });
}

// ---- fused ragged reduce-and-split pooling (csrc/mhte_pool_split_kernels.h) ------------------------
}  // extern "C"
namespace mhte {
// Checks the plan on the host (every failure InvalidArgument, before any HIP call), then launches the forward
// (ptrs: embeddings read, slice_ptrs: outputs written) or the gradient (ptrs: embedding gradients written,
// slice_ptrs: slice gradients read).
static void reduce_split_launch(bool forward, const int32_t* row_splits, const int32_t* row_split_splits,
                                float* const* ptrs, const int64_t* emb_rows, const int32_t* emb_dims,
                                int32_t n_features, const int32_t* slice_dims, int32_t n_slices,
                                float* const* slice_ptrs, hipStream_t st) {
  const std::string op = forward ? "fused_reduce_and_split: " : "fused_reduce_and_split_grad: ";
  auto bad = [&](const std::string& m) { throw Error(MHTE_INVALID_ARGUMENT, op + m); };
  if (n_features <= 0) bad("n_features must be > 0, got " + std::to_string(n_features));
  if (n_slices <= 0) bad("n_slices must be > 0, got " + std::to_string(n_slices));
  if (!row_splits) bad("null argument: row_splits");
  if (!row_split_splits) bad("null argument: row_split_splits");
  if (!ptrs) bad(forward ? "null argument: embeddings" : "null argument: embeddings_grad");
  if (!emb_rows) bad("null argument: emb_rows");
  if (!emb_dims) bad("null argument: emb_dims");
  if (!slice_dims) bad("null argument: slice_dims");
  if (!slice_ptrs) bad(forward ? "null argument: outputs" : "null argument: slice_grads");
  int64_t emb_cols = 0, slice_cols = 0;
  for (int32_t i = 0; i < n_features; ++i) {
    if (emb_dims[i] <= 0)
      bad("embedding " + std::to_string(i) + " has the non-positive dim " + std::to_string(emb_dims[i]));
    if (emb_rows[i] < 0)
      bad("embedding " + std::to_string(i) + " has a negative row count " + std::to_string(emb_rows[i]));
    emb_cols += emb_dims[i];
  }
  for (int32_t k = 0; k < n_slices; ++k) {
    if (slice_dims[k] <= 0)
      bad("slice " + std::to_string(k) + " has the non-positive dim " + std::to_string(slice_dims[k]));
    slice_cols += slice_dims[k];
  }
  const int64_t bs64 = int64_t(row_split_splits[1]) - row_split_splits[0] - 1;   // reduce_op.cu.cc:417
  if (bs64 < 0) bad("feature 0 has no row splits (a feature has batch size + 1 of them)");
  for (int32_t i = 0; i < n_features; ++i) {
    const int64_t cnt = int64_t(row_split_splits[i + 1]) - row_split_splits[i];
    if (cnt != bs64 + 1)
      bad("feature " + std::to_string(i) + " has " + std::to_string(cnt) + " row splits, feature 0 has " +
          std::to_string(bs64 + 1) + " (batch size + 1)");
  }
  if (slice_cols != emb_cols)
    bad("sum(slice_dims) = " + std::to_string(slice_cols) + " differs from sum(emb_dims) = " +
        std::to_string(emb_cols));
  const int32_t bs = int32_t(bs64);
  std::vector<SplitSlice> slices(static_cast<size_t>(n_slices));
  std::vector<int32_t> first_slice(size_t(n_features) + 1, 0);
  {
    int32_t k = 0;
    for (int32_t i = 0; i < n_features; ++i) {
      first_slice[size_t(i)] = k;
      int32_t col = 0;
      while (col < emb_dims[i]) {   // (k < n_slices: the sums are equal)
        if (col + int64_t(slice_dims[k]) > emb_dims[i])
          bad("slice " + std::to_string(k) + " (columns " + std::to_string(col) + " to " +
              std::to_string(col + int64_t(slice_dims[k])) + " of feature " + std::to_string(i) +
              ", which has " + std::to_string(emb_dims[i]) + ") straddles features " + std::to_string(i) +
              " and " + std::to_string(i + 1));
        slices[size_t(k)].out = slice_ptrs[k];
        slices[size_t(k)].start = col;
        slices[size_t(k)].dim = slice_dims[k];
        col += slice_dims[k];
        ++k;
      }
    }
    first_slice[size_t(n_features)] = k;
  }
  for (int32_t i = 0; i < n_features; ++i)
    if (!ptrs[i] && emb_rows[i] > 0)
      bad(std::string("null argument: ") + (forward ? "embeddings[" : "embeddings_grad[") + std::to_string(i) + "]");
  for (int32_t k = 0; k < n_slices; ++k)
    if (!slice_ptrs[k] && bs > 0)
      bad(std::string("null argument: ") + (forward ? "outputs[" : "slice_grads[") + std::to_string(k) + "]");
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) {
    (void)hipGetLastError();
    throw Error(MHTE_UNAVAILABLE, "no HIP device: the MI355X engine has no CPU fallback");
  }
  if (forward && bs == 0) return;
  // units: a feature's lane columns (float4s where its shape and pointers allow, else floats) in runs of 64
  std::vector<SplitUnit> units;
  int64_t need = 1;
  for (int32_t i = 0; i < n_features; ++i) {
    if (!forward && emb_rows[i] == 0) continue;
    bool vec = emb_dims[i] % 4 == 0 && aligned16(ptrs[i]);
    for (int32_t k = first_slice[size_t(i)]; vec && k < first_slice[size_t(i) + 1]; ++k)
      vec = ((slices[size_t(k)].start | slices[size_t(k)].dim) & 3) == 0 && aligned16(slices[size_t(k)].out);
    const int32_t per = vec ? 4 : 1, cols = emb_dims[i] / per;
    for (int32_t c0 = 0; c0 < cols; c0 += kSplitUnitCols) {
      SplitUnit u{};
      u.emb = ptrs[i];
      u.n_rows = emb_rows[i];
      u.rs_off = row_split_splits[i];
      u.dim = emb_dims[i];
      u.col0 = c0 * per;
      const int32_t nc = std::min(kSplitUnitCols, cols - c0);
      u.width = nc * per;
      u.slice0 = first_slice[size_t(i)];
      u.n_slices = first_slice[size_t(i) + 1] - first_slice[size_t(i)];
      u.vec = vec ? 1 : 0;
      while ((1 << u.log2g) < nc) ++u.log2g;
      need = std::max(need, (int64_t(bs) + (256 >> u.log2g) - 1) / (256 >> u.log2g));
      units.push_back(u);
    }
  }
  if (units.empty()) return;
  // (row blocks per unit: enough to fill the chip several times over, the rest of the rows by grid stride)
  const int64_t cap = std::min<int64_t>(4096, std::max<int64_t>(64, 32768 / int64_t(units.size())));
  const uint32_t gx = uint32_t(std::min(need, cap));
  SplitArgs A{};
  A.row_splits = row_splits;
  A.bs = bs;
  const bool ext = units.size() > size_t(kSplitInlineUnits) || slices.size() > size_t(kSplitInlineSlices);
  struct Tmp {   // (freed in stream order behind the kernels that read it)
    char* d = nullptr;
    hipStream_t st;
    ~Tmp() {
      if (d && hipFreeAsync(d, st) != hipSuccess) {
        (void)hipGetLastError();
        (void)hipStreamSynchronize(st);
        (void)hipFree(d);
      }
    }
  } tmp;
  tmp.st = st;
  if (ext) {
    const size_t o_slice = units.size() * sizeof(SplitUnit), total = o_slice + slices.size() * sizeof(SplitSlice);
    std::vector<char> h(total);
    memcpy(h.data(), units.data(), o_slice);
    memcpy(h.data() + o_slice, slices.data(), total - o_slice);
    void* d = nullptr;
    if (hipMallocAsync(&d, total, st) != hipSuccess) {
      (void)hipGetLastError();
      HIP_OK(hipMalloc(&d, total));
    }
    tmp.d = static_cast<char*>(d);
    PinnedStage::of(current_device()).upload(tmp.d, h.data(), total, st);   // (no wait for the stream)
    A.x_units = reinterpret_cast<const SplitUnit*>(tmp.d);
    A.x_slices = reinterpret_cast<const SplitSlice*>(tmp.d + o_slice);
  } else {
    std::copy(units.begin(), units.end(), A.units);
    std::copy(slices.begin(), slices.end(), A.slices);
  }
  for (size_t base = 0; base < units.size(); base += 65535) {   // (grid.y holds 65 535 units)
    A.unit_base = int32_t(base);
    const dim3 grid(gx, uint32_t(std::min<size_t>(65535, units.size() - base)));
    if (ext) {
      if (forward) reduce_split_kernel<true, true><<<grid, 256, 0, st>>>(A);
      else reduce_split_kernel<true, false><<<grid, 256, 0, st>>>(A);
    } else {
      if (forward) reduce_split_kernel<false, true><<<grid, 256, 0, st>>>(A);
      else reduce_split_kernel<false, false><<<grid, 256, 0, st>>>(A);
    }
    HIP_OK(hipGetLastError());
  }
}
}  // namespace mhte
extern "C" {

mhte_status mhte_fused_reduce_and_split(const int32_t* row_splits, const int32_t* row_split_splits,
                                        const float* const* embeddings, const int64_t* emb_rows,
                                        const int32_t* emb_dims, int32_t n_features,
                                        const int32_t* slice_dims, int32_t n_slices, float* const* outputs,
                                        void* stream) {
  return guard([&] {
    reduce_split_launch(true, row_splits, row_split_splits, (float* const*)embeddings, emb_rows, emb_dims,
                        n_features, slice_dims, n_slices, outputs, S(stream));
  });
}

mhte_status mhte_fused_reduce_and_split_grad(const int32_t* row_splits, const int32_t* row_split_splits,
                                             const int64_t* emb_rows, const int32_t* emb_dims,
                                             int32_t n_features, const int32_t* slice_dims, int32_t n_slices,
                                             const float* const* slice_grads, float* const* embeddings_grad,
                                             void* stream) {
  return guard([&] {
    reduce_split_launch(false, row_splits, row_split_splits, embeddings_grad, emb_rows, emb_dims, n_features,
                        slice_dims, n_slices, (float* const*)slice_grads, S(stream));
  });
}

// ---- admission filter ---------------------------------------------------------------------------
mhte_status mhte_hash_filter_create(uint64_t capacity, int32_t split_num, int32_t device,
                                    mhte_hash_filter** out) {
  return guard([&] {
    if (!out) throw Error(MHTE_INVALID_ARGUMENT, "null out");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev)
      throw Error(MHTE_UNAVAILABLE, "no such HIP device");
    HIP_OK(hipSetDevice(device));
    // SlidingHashFilter(capacity, split_num), sliding_hash_filter.cc:29-42
    // (the dump's split_num is the constructor ARGUMENT, unclamped — split_num_, :30,160,192 — so a
    // reference-written dump of a filter created with split_num < 5 validates here and vice versa)
    const int32_t split_num_as_given = split_num;
    if (capacity < 300) capacity = 300;
    if (split_num < 5) split_num = 5;
    if (split_num > kFilterMaxSplits)
      throw Error(MHTE_INVALID_ARGUMENT, "hash filter: split_num must be <= " + std::to_string(kFilterMaxSplits));
    std::unique_ptr<mhte_hash_filter> f(new mhte_hash_filter);
    f->device = device;
    f->capacity = capacity;
    f->split_num_arg = uint32_t(split_num_as_given);
    f->nsplit = uint32_t(split_num);
    const uint64_t split_capacity = capacity / uint64_t(split_num - kFilterForward + 1);  // get_split_capacity
    f->split_cap = uint32_t(std::min<uint64_t>(split_capacity, 0xffffffffu));
    f->total = uint64_t(double(split_capacity) * 1.2);   // HashFilter(split_capacity, fill_rate = 1.2)
    if (f->total < 1) f->total = 1;
    if (f->total + kFilterMaxStep > 0xffffffffull)
      throw Error(MHTE_INVALID_ARGUMENT, "hash filter: split too large");
    f->stride = uint32_t(f->total + kFilterMaxStep);
    const size_t words = size_t(f->nsplit) * f->stride;
    HIP_OK(hipMalloc(&f->slots, words * sizeof(uint32_t)));
    HIP_OK(hipMemset(f->slots, 0, words * sizeof(uint32_t)));
    HIP_OK(hipMalloc(&f->state, sizeof(FilterState)));
    HIP_OK(hipMemset(f->state, 0, sizeof(FilterState)));
    f->budget.split_cap = f->split_cap;
    *out = f.release();
  });
}
void mhte_hash_filter_destroy(mhte_hash_filter* f) { delete f; }

mhte_status mhte_multi_table_set_filter(mhte_multi_table* t, mhte_hash_filter* f) {
  return guard([&] {
    check_handle(t);
    if (f && f->device != t->device)
      throw Error(MHTE_INVALID_ARGUMENT, "hash filter lives on another device");
    for (auto& tb : t->tables) {
      std::lock_guard<std::mutex> g(tb->mu);
      tb->flt_slots = f ? f->slots : nullptr;
      tb->flt_total = f ? f->total : 0;
      tb->flt_state = f ? f->state : nullptr;
      tb->flt_nsplit = f ? f->nsplit : 0;
      tb->flt_stride = f ? f->stride : 0;
      tb->flt_cap = f ? f->split_cap : 0;
      tb->flt_budget = f ? &f->budget : nullptr;
      tb->refresh_view();
    }
  });
}

// ---- touched-key set (mhte_touched_host.h) ---------------------------------------------------------
mhte_status mhte_touched_key_set_create(int64_t capacity, int64_t max_insert, int32_t device,
                                        mhte_touched_key_set** out) {
  return guard([&] {
    if (!out) throw Error(MHTE_INVALID_ARGUMENT, "touched-key set: null out");
    if (capacity <= 0 || capacity > int64_t(1) << 30)
      throw Error(MHTE_INVALID_ARGUMENT, "touched-key set: capacity must be 1..2^30");
    if (max_insert < 0) throw Error(MHTE_INVALID_ARGUMENT, "touched-key set: negative max_insert");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
      throw Error(MHTE_UNAVAILABLE, "no HIP device: the MI355X engine has no CPU fallback");
    if (device < 0 || device >= ndev) throw Error(MHTE_INVALID_ARGUMENT, "device ordinal out of range");
    HIP_OK(hipSetDevice(device));
    std::unique_ptr<mhte_touched_key_set> s(new mhte_touched_key_set);
    s->device = device;
    s->capacity = capacity;
    const int64_t limit = std::min<int64_t>(std::min<int64_t>(max_insert ? max_insert : capacity + 1, capacity + 1),
                                            int64_t(kTkMaxPositions));
    s->call_limit = uint32_t(limit);
    const uint64_t nslots = uint64_t(1) << std::max<uint32_t>(8, ceil_log2(2 * uint64_t(capacity + 1 + limit)));
    if (nslots > (uint64_t(1) << 31)) throw Error(MHTE_INVALID_ARGUMENT, "touched-key set: too large (more than 2^31 slots)");
    HIP_OK(hipMalloc(&s->view.slots, nslots * sizeof(TkSlot)));
    HIP_OK(hipMemset(s->view.slots, 0, nslots * sizeof(TkSlot)));
    HIP_OK(hipMalloc(&s->view.ctl, sizeof(TkCtl)));
    HIP_OK(hipMemset(s->view.ctl, 0, sizeof(TkCtl)));
    const size_t words = size_t(limit + 31) / 32 + 1;
    HIP_OK(hipMalloc(&s->view.bitmap, words * sizeof(uint32_t)));
    HIP_OK(hipMemset(s->view.bitmap, 0, words * sizeof(uint32_t)));
    s->view.mask = uint32_t(nslots - 1);
    s->view.capacity = uint32_t(capacity);
    HIP_OK(hipEventCreateWithFlags(&s->ev, hipEventDisableTiming));
    HIP_OK(hipDeviceSynchronize());
    *out = s.release();
  });
}

void mhte_touched_key_set_destroy(mhte_touched_key_set* set) {
  if (!set) return;
  {
    std::lock_guard<std::mutex> link(g_touched_link_mu);
    if (mhte_multi_table* t = set->owner) {
      std::vector<std::unique_lock<std::mutex>> locks;
      for (auto& tb : t->tables) locks.emplace_back(tb->mu);
      t->touched = nullptr;
      set->owner = nullptr;
    }
  }
  delete set;
}

mhte_status mhte_touched_key_set_insert(mhte_touched_key_set* set, const int64_t* ids, int64_t n_max,
                                        const uint32_t* n_dev, int32_t tag, void* stream) {
  return guard([&] {
    if (n_max < 0 || n_max > int64_t(0xffffffffu)) throw Error(MHTE_INVALID_ARGUMENT, "touched-key set: bad n_max");
    if (!set) throw Error(MHTE_INVALID_ARGUMENT, "touched-key set: null handle");
    if (tag < 0) throw Error(MHTE_INVALID_ARGUMENT, "touched-key set: negative tag");
    if (n_max == 0) return;
    if (!ids) throw Error(MHTE_INVALID_ARGUMENT, "touched-key set: null ids");
    HIP_OK(hipSetDevice(set->device));
    std::lock_guard<std::mutex> g(set->mu);
    tk_enter_stream(*set, S(stream));
    TkDesc d{};
    d.ids = ids;
    d.n_dev = n_dev;
    d.n_max = uint32_t(n_max);
    d.tag = tag;
    tk_insert_segments(*set, &d, nullptr, 1, nullptr, S(stream));
  });
}

mhte_status mhte_touched_key_set_stats(mhte_touched_key_set* set, int64_t out[4], void* stream) {
  return guard([&] {
    if (!set || !out) throw Error(MHTE_INVALID_ARGUMENT, "touched-key set: null argument");
    HIP_OK(hipSetDevice(set->device));
    std::lock_guard<std::mutex> g(set->mu);
    tk_enter_stream(*set, S(stream));
    TkCtl h;
    HIP_OK(hipMemcpyAsync(&h, set->view.ctl, sizeof(h), hipMemcpyDeviceToHost, S(stream)));
    HIP_OK(hipStreamSynchronize(S(stream)));
    out[0] = int64_t(h.size);
    out[1] = int64_t(h.dropped);
    out[2] = int64_t(h.clears);
    out[3] = set->capacity;
  });
}

mhte_status mhte_touched_key_set_steal(mhte_touched_key_set* set, int64_t* ids_out, int32_t* tags_out,
                                       int64_t cap, int64_t* n, void* stream) {
  return guard([&] {
    if (!set || !n) throw Error(MHTE_INVALID_ARGUMENT, "touched-key set: null argument");
    if (cap < 0 || (cap > 0 && !ids_out)) throw Error(MHTE_INVALID_ARGUMENT, "touched-key set: bad output buffer");
    HIP_OK(hipSetDevice(set->device));
    std::lock_guard<std::mutex> g(set->mu);
    hipStream_t st = S(stream);
    tk_enter_stream(*set, st);
    TkCtl h;
    HIP_OK(hipMemcpyAsync(&h, set->view.ctl, sizeof(h), hipMemcpyDeviceToHost, st));
    HIP_OK(hipStreamSynchronize(st));
    if (int64_t(h.size) > cap)
      throw Error(MHTE_INVALID_ARGUMENT, "touched-key set: the set holds " + std::to_string(h.size) +
                                             " keys, the output buffers " + std::to_string(cap));
    *n = int64_t(h.size);
    if (h.size == 0) return;
    const TkView v = set->view;
    HIP_OK(hipMemsetAsync(&v.ctl->steal_n, 0, sizeof(uint32_t), st));
    const uint32_t nb = uint32_t(std::min<uint64_t>((uint64_t(v.mask) + 1u) / kTkBlock, 2048));
    tk_steal_kernel<<<nb, kTkBlock, 0, st>>>(v, ids_out, tags_out, uint32_t(std::min<int64_t>(cap, 0xffffffffll)));
    tk_clear_kernel<<<nb, kTkBlock, 0, st>>>(v, 1);
    HIP_OK(hipGetLastError());
    HIP_OK(hipStreamSynchronize(st));
  });
}

mhte_status mhte_multi_table_set_touched_key_set(mhte_multi_table* t, mhte_touched_key_set* set) {
  return guard([&] {
    check_handle(t);
    std::lock_guard<std::mutex> link(g_touched_link_mu);
    if (set) {
      if (set->device != t->device) throw Error(MHTE_INVALID_ARGUMENT, "touched-key set lives on another device");
      if (set->owner && set->owner != t)
        throw Error(MHTE_INVALID_ARGUMENT, "touched-key set is attached to another MultiHashTable");
      if (!t->shard_steps.empty())
        throw Error(MHTE_INVALID_ARGUMENT, "an id-sharded step exists on this MultiHashTable: it does not record "
                                           "on the owner yet");
      if (!t->multi_steps.empty() && tk_any_filter(t))
        throw Error(MHTE_INVALID_ARGUMENT, "a multi step exists on this MultiHashTable and it has an admission "
                                           "filter: the fused step cannot record what the filter admits");
    }
    std::vector<std::unique_lock<std::mutex>> locks;
    for (auto& tb : t->tables) locks.emplace_back(tb->mu);
    if (t->touched && t->touched != set) {
      std::lock_guard<std::mutex> gs(t->touched->mu);
      t->touched->owner = nullptr;
    }
    t->touched = set;
    if (set) {
      std::lock_guard<std::mutex> gs(set->mu);
      set->owner = t;
    }
  });
}

/* seen count of ids (Filter::get, hash_filter.h:109-111): out [dev u32, n] */
mhte_status mhte_hash_filter_get(mhte_hash_filter* f, const int64_t* id, int64_t n, uint32_t* out,
                                 void* stream) {
  return guard([&] {
    if (!f) throw Error(MHTE_INVALID_ARGUMENT, "null argument");
    if (n <= 0) return;
    if (!id || !out) throw Error(MHTE_INVALID_ARGUMENT, "null argument");
    HIP_OK(hipSetDevice(f->device));
    filter_get_kernel<<<dim3(uint32_t((n + 255) / 256)), 256, 0, S(stream)>>>(f->view(), id, n, out);
    HIP_OK(hipGetLastError());
  });
}

// MonolithHashFilterSave / Restore (RT/ops/hash_filter_save_op.cc:35-112, hash_filter_restore_op.cc):
// one TFRecord file per split, <basename>-%05d-of-%05d: a HashFilterSplitMetaDump (with the sliding
// window's SlidingHashFilterMetaDump inside), then HashFilterSplitDataDump records of <= 10 000 slot
// words (hash_filter.cc:27-57; embedding_hash_table.proto:112-137).
namespace mhte {
namespace {
void put_key(std::string& o, uint32_t field, uint32_t wt) { ckpt::put_varint(o, (uint64_t(field) << 3) | wt); }
void put_u(std::string& o, uint32_t field, uint64_t v) { put_key(o, field, 0); ckpt::put_varint(o, v); }
}  // namespace
}  // namespace mhte

mhte_status mhte_hash_filter_stats(mhte_hash_filter* f, int64_t* out, int32_t cap, void* stream) {
  return guard([&] {
    if (!f || !out) throw Error(MHTE_INVALID_ARGUMENT, "filter stats: bad arguments");
    if (cap < 4 + int32_t(f->nsplit)) throw Error(MHTE_INVALID_ARGUMENT, "filter stats: out holds 4 + split count words");
    HIP_OK(hipSetDevice(f->device));
    hipStream_t st = S(stream);
    std::unique_ptr<FilterState> hs_heap(new FilterState);   // (256 KB: not on the stack)
    FilterState& hs = *hs_heap;
    HIP_OK(hipMemcpyAsync(&hs, f->state, sizeof(hs), hipMemcpyDeviceToHost, st));
    HIP_OK(hipStreamSynchronize(st));
    out[0] = hs.head;
    out[1] = hs.head_increment;
    out[2] = int64_t(hs.failure_count);
    out[3] = f->nsplit;
    for (uint32_t sp = 0; sp < f->nsplit; ++sp) out[4 + sp] = filter_split_elements(hs, sp);
  });
}

mhte_status mhte_hash_filter_save(mhte_hash_filter* f, const char* basename, void* stream) {
  return guard([&] {
    if (!f || !basename || !*basename) throw Error(MHTE_INVALID_ARGUMENT, "filter save: bad arguments");
    if (f->nsplit == 0) return;   // probabilistic: split_num() == 0, the save op writes no file
    HIP_OK(hipSetDevice(f->device));
    hipStream_t st = S(stream);
    std::unique_ptr<FilterState> hs_heap(new FilterState);   // (256 KB: not on the stack)
    FilterState& hs = *hs_heap;
    HIP_OK(hipMemcpyAsync(&hs, f->state, sizeof(hs), hipMemcpyDeviceToHost, st));
    std::vector<uint32_t> words(size_t(f->nsplit) * f->stride);
    HIP_OK(hipMemcpyAsync(words.data(), f->slots, words.size() * 4, hipMemcpyDeviceToHost, st));
    HIP_OK(hipStreamSynchronize(st));
    std::string sl;   // SlidingHashFilterMetaDump
    put_u(sl, 1, f->split_num_arg);
    put_u(sl, 2, kFilterForward);
    put_u(sl, 3, f->nsplit - kFilterForward);
    put_u(sl, 4, kFilterProbe);
    put_u(sl, 5, hs.head);
    put_u(sl, 6, hs.head_increment);
    put_u(sl, 7, hs.failure_count);
    for (uint32_t sp = 0; sp < f->nsplit; ++sp) {
      const std::string fn = ckpt::shard_name(basename, "", int(sp), int(f->nsplit));
      const std::string tmp = fn + "-tmp-" + std::to_string(uint64_t(getpid()));
      {
        ckpt::RecordWriter w(tmp, false);
        std::string meta;   // HashFilterSplitMetaDump
        put_u(meta, 1, 0);   // failure_count of the split (hash_filter.h:103: a statistic of exhausted
                             // probe sequences; the engine keeps the sliding filter's total only)
        put_u(meta, 2, f->total);
        put_u(meta, 3, filter_split_elements(hs, uint32_t(sp)));
        put_key(meta, 4, 1);
        const double fill = 1.2;
        meta.append(reinterpret_cast<const char*>(&fill), 8);
        put_key(meta, 5, 2);
        ckpt::put_varint(meta, sl.size());
        meta += sl;
        w.write(meta);
        const uint32_t* split = words.data() + size_t(sp) * f->stride;
        std::string rec;
        for (uint32_t s0 = 0; s0 < f->stride; s0 += 10000) {
          rec.clear();
          put_u(rec, 1, s0);
          const uint32_t s1 = std::min<uint32_t>(f->stride, s0 + 10000);
          for (uint32_t i = s0; i < s1; ++i) put_u(rec, 2, split[i]);   // (proto2 repeated: unpacked)
          w.write(rec);
        }
        w.close();
      }
      if (rename(tmp.c_str(), fn.c_str()) != 0)
        throw Error(MHTE_INTERNAL, "filter save: cannot rename into " + fn);
    }
  });
}

mhte_status mhte_hash_filter_restore(mhte_hash_filter* f, const char* basename, void* stream) {
  return guard([&] {
    if (!f || !basename || !*basename) throw Error(MHTE_INVALID_ARGUMENT, "filter restore: bad arguments");
    if (f->nsplit == 0) return;   // probabilistic: stateless
    HIP_OK(hipSetDevice(f->device));
    hipStream_t st = S(stream);
    std::unique_ptr<FilterState> hs_heap(new FilterState);   // (256 KB: not on the stack)
    FilterState& hs = *hs_heap;
    memset(&hs, 0, sizeof(hs));
    std::vector<uint32_t> words(size_t(f->nsplit) * f->stride, 0u);
    try {
      for (uint32_t sp = 0; sp < f->nsplit; ++sp) {
        ckpt::RecordReader r(ckpt::shard_name(basename, "", int(sp), int(f->nsplit)), false);
        std::string rec;
        if (!r.read(&rec)) throw Error(MHTE_INTERNAL, "filter restore: empty split file");
        {
          pcfg::Msg m(reinterpret_cast<const uint8_t*>(rec.data()), rec.size());
          pcfg::Field fl;
          uint64_t total = 0;
          while (m.next(&fl)) {
            if (fl.num == 2) total = fl.v;
            if (fl.num == 3) hs.num_elements[sp][0] = uint32_t(fl.v);
            if (fl.num == 5 && fl.wt == 2) {
              pcfg::Msg sm(fl.p, fl.n);
              pcfg::Field g;
              while (sm.next(&g)) {
                // SlidingHashFilter::RestoreMetaDump validates the geometry (:181-197)
                auto same = [&](uint64_t want, const char* what) {
                  if (g.v != want)
                    throw Error(MHTE_RESOURCE_EXHAUSTED,
                                std::string(what) + ": " + std::to_string(want) + " does't match with : " +
                                    std::to_string(g.v) + " read from hash filter checkpoint file.");
                };
                if (g.num == 1) same(f->split_num_arg, "split_num");
                if (g.num == 2) same(kFilterForward, "max_forward_step");
                if (g.num == 3) same(f->nsplit - kFilterForward, "max_backward_step");
                if (g.num == 4) same(kFilterProbe, "max_step");
                if (g.num == 5) hs.head = uint32_t(g.v);
                if (g.num == 6) hs.head_increment = uint32_t(g.v);
                if (g.num == 7) hs.failure_count = g.v;
              }
            }
          }
          if (total != f->total)
            throw Error(MHTE_RESOURCE_EXHAUSTED, "filter restore: split size " + std::to_string(total) +
                                                     " does not match this filter's " + std::to_string(f->total));
        }
        uint32_t* split = words.data() + size_t(sp) * f->stride;
        while (r.read(&rec)) {
          pcfg::Msg m(reinterpret_cast<const uint8_t*>(rec.data()), rec.size());
          pcfg::Field fl;
          uint64_t off = 0, i = 0;
          while (m.next(&fl)) {
            if (fl.num == 1) off = fl.v;
            if (fl.num == 2 && fl.wt == 0) {
              if (off + i < f->stride) split[off + i] = uint32_t(fl.v);
              ++i;
            }
            if (fl.num == 2 && fl.wt == 2) {  // (a packed writer)
              const uint8_t* q = fl.p;
              const uint8_t* qe = fl.p + fl.n;
              uint64_t v;
              while (q < qe && ckpt::get_varint(q, qe, &v)) {
                if (off + i < f->stride) split[off + i] = uint32_t(v);
                ++i;
              }
            }
          }
        }
      }
    } catch (const Error&) {
      throw;
    } catch (const std::exception& e) {
      throw Error(MHTE_NOT_FOUND, std::string("filter restore: ") + e.what());
    }
    // A slot word is the reference's uint16: signature << 4 | count (hash_filter.h:33-60).  Dumps
    // written by this engine before ABI 12 carried 28-bit signatures in the same 32-bit words,
    // untagged: restored as they are, no id would ever match its slot again (counts lost, admitted
    // ids filtered anew) — refuse them by name instead.
    for (uint32_t wv : words)
      if (wv > 0xffffu)
        throw Error(MHTE_INVALID_ARGUMENT,
                    "filter restore: slot words wider than 16 bits — a dump written before ABI 12 "
                    "(28-bit signatures); not convertible (the 12-bit signature is a different hash "
                    "slice), re-create the filter");
    HIP_OK(hipMemcpyAsync(f->slots, words.data(), words.size() * 4, hipMemcpyHostToDevice, st));
    HIP_OK(hipMemcpyAsync(f->state, &hs, sizeof(hs), hipMemcpyHostToDevice, st));
    f->budget.invalidate();   // (the head split's fill is whatever the dump says)
    HIP_OK(hipStreamSynchronize(st));
  });
}

// ---- checkpoints in the reference's on-disk format (mhte_ckpt_host.h) ---------------------------
mhte_status mhte_multi_table_save(mhte_multi_table* t, const char* basename, int32_t nshards,
                                  void* stream) {
  return guard([&] {
    check_handle(t);
    ckpt_entry(t, false, basename, [&] { save_tables(t, basename, nshards, S(stream)); });
  });
}

mhte_status mhte_multi_table_restore(mhte_multi_table* t, const char* basename, void* stream) {
  return guard([&] {
    check_handle(t);
    ckpt_entry(t, true, basename, [&] { restore_tables(t, basename, S(stream)); });
  });
}

mhte_status mhte_table_save(mhte_multi_table* t, int32_t table, const char* basename, int32_t nshards,
                            void* stream) {
  return guard([&] {
    table_at(t, table);
    ckpt_entry(t, false, basename, [&] { save_tables(t, basename, nshards, S(stream), table); });
  });
}

mhte_status mhte_table_restore(mhte_multi_table* t, int32_t table, const char* basename, void* stream) {
  return guard([&] {
    table_at(t, table);
    ckpt_entry(t, true, basename, [&] { restore_tables(t, basename, S(stream), table); });
  });
}

mhte_status mhte_table_clear(mhte_multi_table* t, int32_t table, void* stream) {
  return guard([&] {
    Table& tb = table_at(t, table);
    HIP_OK(hipSetDevice(t->device));
    std::lock_guard<std::mutex> g(tb.mu);
    tb.clear(S(stream));
  });
}

// ---- dedup / packing ops ---------------------------------------------------------------------
mhte_status mhte_dedup_ws_create(int32_t device, mhte_dedup_ws** out) {
  return guard([&] {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev)
      throw Error(MHTE_UNAVAILABLE, "no such HIP device");
    mhte_dedup_ws* w = new mhte_dedup_ws;
    w->ws.device = device;
    *out = w;
  });
}
void mhte_dedup_ws_destroy(mhte_dedup_ws* ws) {
  if (ws && ws->ws.holds_reservations()) {
    // a numbered batch that was never applied: its row reservations' keys go back to the table
    // (the table may already be gone: its counters then are freed memory — only while it lives)
    // (the numbering / probe that wrote the records ran on the caller's stream, which the null stream
    // does not wait for: drain the device first, then count)
    (void)hipSetDevice(ws->ws.device);
    (void)hipDeviceSynchronize();
    ws->ws.drop_reservations(nullptr);
    (void)hipDeviceSynchronize();
  }
  delete ws;
}

mhte_status mhte_unique(mhte_dedup_ws* ws, const int64_t* ids, int64_t n, int64_t* unique_ids,
                        uint32_t* inverse, uint32_t* seg_off, uint32_t* seg_pos,
                        uint32_t* n_unique_dev, int64_t* n_unique_host, void* stream) {
  return guard([&] {
    if (!ws) throw Error(MHTE_INVALID_ARGUMENT, "null workspace");
    HIP_OK(hipSetDevice(ws->ws.device));
    ws->ws.unique(ids, n, unique_ids, inverse, seg_off, seg_pos, n_unique_dev, S(stream));
    if (n_unique_host) {
      uint32_t u = 0;
      HIP_OK(hipMemcpyAsync(&u, n_unique_dev, sizeof(u), hipMemcpyDeviceToHost, S(stream)));
      HIP_OK(hipStreamSynchronize(S(stream)));
      *n_unique_host = u;
    }
  });
}

mhte_status mhte_unique_unordered(mhte_dedup_ws* ws, const int64_t* ids, int64_t n,
                                  int64_t* unique_ids, uint32_t* inverse, uint32_t* list_start,
                                  uint32_t* list_end, uint32_t* seg_pos, uint32_t* n_unique_dev,
                                  int64_t* n_unique_host, void* stream) {
  return guard([&] {
    if (!ws) throw Error(MHTE_INVALID_ARGUMENT, "null workspace");
    HIP_OK(hipSetDevice(ws->ws.device));
    ws->ws.unique_unordered(ids, n, unique_ids, inverse, list_start, list_end, seg_pos,
                            n_unique_dev, S(stream));
    if (n_unique_host) {
      uint32_t u = 0;
      HIP_OK(hipMemcpyAsync(&u, n_unique_dev, sizeof(u), hipMemcpyDeviceToHost, S(stream)));
      HIP_OK(hipStreamSynchronize(S(stream)));
      *n_unique_host = u;
    }
  });
}

mhte_status mhte_gather_rows(const float* src, const uint32_t* index, int64_t n, int32_t dim,
                             float* out, void* stream) {
  return guard([&] {
    if (n <= 0) return;
    if (dim <= 0) throw Error(MHTE_INVALID_ARGUMENT, "dim must be > 0");
    Shape sh = pick_shape(uint32_t(dim), dim % 4 == 0 && aligned16(src) && aligned16(out));
    const dim3 grid(uint32_t((n * sh.G + 255) / 256));
    hipStream_t st = S(stream);
    for_shape(sh, [&](auto g_, auto v_) {
      gather_rows_kernel<decltype(g_)::value, decltype(v_)::value><<<grid, 256, 0, st>>>(src, index, n, uint32_t(dim), out);
    });
    HIP_OK(hipGetLastError());
  });
}

mhte_status mhte_segment_sum(mhte_dedup_ws* ws, const float* grads, const uint32_t* inverse,
                             const uint32_t* seg_off, const uint32_t* seg_pos,
                             const uint32_t* n_unique_dev, int64_t n, int32_t dim, float* out,
                             int32_t exact_order, void* stream) {
  return guard([&] {
    if (!ws) throw Error(MHTE_INVALID_ARGUMENT, "null workspace");
    if (n <= 0) return;
    if (dim <= 0) throw Error(MHTE_INVALID_ARGUMENT, "dim must be > 0");
    HIP_OK(hipSetDevice(ws->ws.device));
    hipStream_t st = S(stream);
    Shape sh = pick_shape(uint32_t(dim), dim % 4 == 0 && aligned16(grads) && aligned16(out));
    if (exact_order) {
      const dim3 grid(uint32_t((n * sh.G + 255) / 256));
      for_shape(sh, [&](auto g_, auto v_) {
        segsum_exact_kernel<decltype(g_)::value, decltype(v_)::value><<<grid, 256, 0, st>>>(
            grads, n_unique_dev, seg_off, seg_pos, uint32_t(dim), out);
      });
    } else {
      const int win = sh.G < 16 ? sh.G : 16;
      const int64_t nwin = (n + win - 1) / win;
      ws->ws.part.reserve(size_t(nwin) * 2 * dim + 16);
      ws->ws.last_u.reserve(nwin + 1);
      float* part = ws->ws.part.p;
      uint32_t* last_u = ws->ws.last_u.p;
      const dim3 grid(uint32_t((nwin * sh.G + 255) / 256));
      for_shape(sh, [&](auto g_, auto v_) {
        constexpr int G = decltype(g_)::value, V = decltype(v_)::value;
        segsum_window_kernel<G, V><<<grid, 256, 0, st>>>(grads, inverse, seg_off, seg_pos, uint32_t(n),
                                                         uint32_t(dim), out, part, last_u);
        segsum_combine_kernel<G, V><<<dim3(uint32_t(nwin)), 256, 0, st>>>(seg_off, last_u, uint32_t(dim), out, part);
      });
    }
    HIP_OK(hipGetLastError());
  });
}

mhte_status mhte_table_lookup_n(mhte_multi_table* t, int32_t table, const int64_t* id,
                                int64_t n_max, const uint32_t* n_dev, float* embedding,
                                void* stream) {
  return guard([&] {
    Table& tb = table_at(t, table);
    HIP_OK(hipSetDevice(t->device));
    std::lock_guard<std::mutex> g(tb.mu);
    tb.lookup(id, n_max, n_dev, embedding, S(stream));
  });
}

mhte_status mhte_table_optimize_n(mhte_multi_table* t, int32_t table, const int64_t* id,
                                  int64_t n_max, const uint32_t* n_dev, const float* value,
                                  const float* learning_rate, int64_t n_learning_rate,
                                  int64_t update_time, int64_t global_step, int32_t flags,
                                  void* stream) {
  return guard([&] {
    mhte::t_global_step = global_step;
    Table& tb = table_at(t, table);
    if (!learning_rate || n_learning_rate < int64_t(tb.nseg))
      throw Error(MHTE_INVALID_ARGUMENT, "The length of tensor `learning_rate` is too short.");
    HIP_OK(hipSetDevice(t->device));
    std::lock_guard<std::mutex> g(tb.mu);
    tb.note_update_time(update_time);
    tb.upsert<kOpOptimize>(id, n_max, n_dev, value, learning_rate, update_time, flags, nullptr,
                           S(stream));
    tb.maybe_evict(S(stream));
    tk_record(t, tb, table, id, n_max, n_dev, S(stream));
  });
}

mhte_status mhte_table_sum_optimize_n(mhte_multi_table* t, int32_t table, mhte_dedup_ws* ws,
                                      const int64_t* unique_ids, int64_t n_max,
                                      const uint32_t* n_unique_dev, const float* grads,
                                      const uint32_t* inverse, const uint32_t* list_start,
                                      const uint32_t* list_end, const uint32_t* seg_pos, int64_t n,
                                      float* grad_unique, const float* learning_rate,
                                      int64_t n_learning_rate, int64_t update_time,
                                      int64_t global_step, int32_t flags, void* stream) {
  return guard([&] {
    mhte::t_global_step = global_step;  // (batch softmax, through the op-level update of wide / non-basic tables)
    Table& tb = table_at(t, table);
    if (!ws) throw Error(MHTE_INVALID_ARGUMENT, "null workspace");
    if (!learning_rate || n_learning_rate < int64_t(tb.nseg))
      throw Error(MHTE_INVALID_ARGUMENT, "The length of tensor `learning_rate` is too short.");
    if (!n_unique_dev || !grad_unique)
      throw Error(MHTE_INVALID_ARGUMENT, "sum_optimize: null argument");
    HIP_OK(hipSetDevice(t->device));
    std::lock_guard<std::mutex> g(tb.mu);
    tb.note_update_time(update_time);
    hipStream_t st = S(stream);
    if (tb.flt_slots) {
      // an occurrence filter is attached: the admission decision needs every id's occurrence COUNT
      // (one consultation with count k, tf_bridge.cc:300-310) — the update kernel that walks the
      // occurrence lists, sums them in order and consults the filter (sum_apply_kernel does not)
      if (list_end != list_start + 1)
        throw Error(MHTE_INVALID_ARGUMENT, "a table with an occurrence filter needs the ordered mhte_unique "
                                           "(CSR occurrence lists)");
      tb.finish_pending(st);
      if (n <= 0 || n_max <= 0) return;
      const ApplyArgs a = tb.apply_args(learning_rate, update_time, global_step, 1, 1);
      tb.ensure_capacity(uint64_t(n_max), st);
      tb.launch_upsert<kOpOptimize>(unique_ids, n_max, n_unique_dev, grads, list_start, seg_pos, a, nullptr, st);
      tb.maybe_evict(st);
      tk_record(t, tb, table, unique_ids, n_max, n_unique_dev, st);
      return;
    }
    // (sum_apply_kernel is compiled for SGD / Adagrad / FTRL; a row of more than 64 floats in buffers that are
    // not 16-byte aligned has no fused shape and takes the route of the wide rows below)
    if (tb.fusable() && tb.basic_opts() &&
        tb.fused_shape_covers({{"grads", grads}, {"grad_unique", grad_unique}})) {
      tb.sum_optimize(ws->ws, unique_ids, n_max, n_unique_dev, grads, list_start, list_end,
                      seg_pos, n, grad_unique, learning_rate, update_time,
                      (flags & MHTE_EXACT_ORDER) != 0, (flags & MHTE_DEFER_SLOWPATH) != 0, st);
      if (!(flags & MHTE_DEFER_SLOWPATH)) tb.maybe_evict(st);
      tk_record(t, tb, table, unique_ids, n_max, n_unique_dev, st);
      return;
    }
    // wide rows: segment sum, then the ordinary upsert over the unique ids (needs the CSR form of
    // the ordered dedup: list_end == list_start + 1)
    if (list_end != list_start + 1)
      throw Error(MHTE_INVALID_ARGUMENT,
                  "rows wider than 256 floats, rows of more than 64 floats in buffers that are not 16-byte "
                  "aligned and optimizers beyond SGD / Adagrad / FTRL need the ordered "
                  "mhte_unique (CSR occurrence lists) here; the pipelined step takes them as they are");
    mhte_status s2 = mhte_segment_sum(ws, grads, inverse, list_start, seg_pos, n_unique_dev, n,
                                      int32_t(tb.dim), grad_unique,
                                      (flags & MHTE_EXACT_ORDER) ? 1 : 0, stream);
    if (s2 != MHTE_OK) throw Error(s2, g_last_error);
    tb.upsert<kOpOptimize>(unique_ids, n_max, n_unique_dev, grad_unique, learning_rate, update_time,
                           MHTE_IDS_UNIQUE, nullptr, st);
    tk_record(t, tb, table, unique_ids, n_max, n_unique_dev, st);
  });
}

mhte_status mhte_step_dedup(mhte_dedup_ws* ws, const int64_t* id, int64_t n, int64_t* unique_ids,
                            uint32_t* n_unique_dev, void* stream) {
  return guard([&] {
    if (!ws || !id || !unique_ids || !n_unique_dev)
      throw Error(MHTE_INVALID_ARGUMENT, "step_dedup: null argument");
    HIP_OK(hipSetDevice(ws->ws.device));
    hipStream_t st = S(stream);
    const RunView d = ws->ws.begin_run_dedup(id, n, unique_ids, n_unique_dev, st);
    LAUNCH_HOT(kTagDedup, rd_dedup_kernel, d.nblk, kRdBlock, st, d);
    HIP_OK(hipGetLastError());
    ws->ws.build_work_list(st);
  });
}

extern "C++" {
namespace mhte {
// SCATTER / SUM over the run format of ws's deduplicated + built batch (rd_gather_kernel)
template <bool SCATTER>
static void step_gather(DedupWs& ws, const float* in, const uint32_t* index, int32_t dim, float* out,
                        hipStream_t st) {
  if (ws.r_stage == 1) ws.build_work_list(st);
  if (ws.r_stage != 2)
    throw Error(MHTE_FAILED_PRECONDITION, "workspace holds no deduplicated batch (mhte_step_dedup)");
  if (dim <= 0 || dim > 256) throw Error(MHTE_INVALID_ARGUMENT, "dim must be 1..256");
  if (!in || !out) throw Error(MHTE_INVALID_ARGUMENT, "null argument");
  const bool vec = dim % 4 == 0 && aligned16(in) && aligned16(out);
  Shape sh = pick_shape(uint32_t(dim), vec);
  if (uint32_t(dim) > uint32_t(sh.G * sh.VEC))
    throw Error(MHTE_INVALID_ARGUMENT, "rows of more than 64 floats must be 16-byte aligned and a "
                                       "multiple of 4 floats wide");
  const int64_t n = ws.rv.n;
  const uint32_t cap_items = DedupWs::max_items(n);
  GatherCtl c{};
  c.in = in;
  c.out = out;
  c.index = index;
  c.n_max = n;
  c.dim = uint32_t(dim);
  if (!SCATTER) {
    ws.part.reserve(size_t(cap_items) * dim + 16);
    c.part = ws.part.p;
    c.arrive = ws.zeroed_arrive(size_t(n), st);
  }
  const uint32_t groups_per_wg = uint32_t(256 / sh.G);
  c.nblk_items = std::min<uint32_t>(cap_items, 288);
  c.nblk_ids = std::max<uint32_t>(1, std::min<uint32_t>(uint32_t((n + groups_per_wg - 1) / groups_per_wg), 1024));
  const dim3 grid(c.nblk_items + c.nblk_ids);
  const RunView d = ws.rv;
  for_shape(sh, [&](auto g_, auto v_) {
    rd_gather_kernel<decltype(g_)::value, decltype(v_)::value, SCATTER><<<grid, 256, 0, st>>>(d, c);
  });
  HIP_OK(hipGetLastError());
}
}  // namespace mhte
}  // extern "C++"

mhte_status mhte_step_scatter(mhte_dedup_ws* ws, const float* rows, const uint32_t* index,
                              int32_t dim, float* out, void* stream) {
  return guard([&] {
    if (!ws) throw Error(MHTE_INVALID_ARGUMENT, "null workspace");
    HIP_OK(hipSetDevice(ws->ws.device));
    step_gather<true>(ws->ws, rows, index, dim, out, S(stream));
  });
}

mhte_status mhte_step_sum(mhte_dedup_ws* ws, const float* grads, const uint32_t* index, int32_t dim,
                          float* out, void* stream) {
  return guard([&] {
    if (!ws) throw Error(MHTE_INVALID_ARGUMENT, "null workspace");
    HIP_OK(hipSetDevice(ws->ws.device));
    step_gather<false>(ws->ws, grads, index, dim, out, S(stream));
  });
}

mhte_status mhte_shard_partition(mhte_dedup_ws* ws, const int64_t* ids, int64_t n_max,
                                 const uint32_t* n_dev, int32_t num_shards, int64_t* send_ids,
                                 uint32_t* send_pos, uint32_t* counts, void* stream) {
  return guard([&] {
    if (!ws || !ids || !n_dev || !send_ids || !send_pos || !counts)
      throw Error(MHTE_INVALID_ARGUMENT, "shard_partition: null argument");
    if (num_shards < 1 || num_shards > kMaxShards)
      throw Error(MHTE_INVALID_ARGUMENT, "num_shards must be 1.." + std::to_string(kMaxShards));
    HIP_OK(hipSetDevice(ws->ws.device));
    hipStream_t st = S(stream);
    HIP_OK(hipMemsetAsync(counts, 0, sizeof(uint32_t) * num_shards, st));
    if (n_max <= 0) return;
    ws->ws.r_cursor.reserve(kMaxShards);
    HIP_OK(hipMemsetAsync(ws->ws.r_cursor.p, 0, sizeof(uint32_t) * kMaxShards, st));
    const uint32_t nb = uint32_t((n_max + 1023) / 1024);
    rd_shard_count_kernel<<<nb, 1024, 0, st>>>(ids, n_dev, n_max, uint32_t(num_shards), counts);
    rd_shard_place_kernel<<<nb, 1024, 0, st>>>(ids, n_dev, n_max, uint32_t(num_shards), counts,
                                               ws->ws.r_cursor.p, send_ids, send_pos);
    HIP_OK(hipGetLastError());
  });
}

mhte_status mhte_table_step_forward(mhte_multi_table* t, int32_t table, const int64_t* id,
                                    int64_t n, float* embedding, mhte_dedup_ws* ws_next,
                                    const int64_t* id_next, int64_t n_next,
                                    int64_t* unique_ids_next, uint32_t* n_unique_dev_next,
                                    mhte_dedup_ws* ws_cur, void* stream) {
  return guard([&] {
    HostProfScope hps(0);
    Table& tb = table_at(t, table);
    tb.refuse_retriever("step_forward");
    if (!tb.fusable())
      throw Error(MHTE_INVALID_ARGUMENT, "step_forward: row too wide for the fused step");
    HIP_OK(hipSetDevice(t->device));
    std::lock_guard<std::mutex> g(tb.mu);
    hps.locked();
    // refused before anything changes: the next batch's run dedup is not begun, the displacement pass the
    // previous update left stays queued
    if (n > 0) tb.fused_shape("step_forward", {{"embedding", embedding}});
    hipStream_t st = S(stream);
    RunView nxt{};
    if (ws_next) {
      if (!id_next || !unique_ids_next || !n_unique_dev_next)
        throw Error(MHTE_INVALID_ARGUMENT, "step_forward: null argument for the next batch");
      nxt = ws_next->ws.begin_run_dedup(id_next, n_next, unique_ids_next, n_unique_dev_next, st);
    }
    if (ws_cur && ws_cur == ws_next)
      throw Error(MHTE_INVALID_ARGUMENT, "step_forward: ws_cur must differ from ws_next");
    tb.step_forward(id, n, embedding, nxt, st);
  });
}

mhte_status mhte_table_step_backward(mhte_multi_table* t, int32_t table, mhte_dedup_ws* ws,
                                     mhte_dedup_ws* ws_next, const int64_t* unique_ids,
                                     int64_t n_max, const uint32_t* n_unique_dev,
                                     const float* grads, int64_t n, float* grad_unique,
                                     const float* learning_rate, int64_t n_learning_rate,
                                     int64_t update_time, int64_t global_step, int32_t flags,
                                     void* stream) {
  return mhte_table_step_backward_ahead(t, table, ws, ws_next, unique_ids, n_max, n_unique_dev, grads, n,
                                        grad_unique, learning_rate, n_learning_rate, update_time,
                                        global_step, flags, nullptr, nullptr, 0, nullptr, nullptr, stream);
}

mhte_status mhte_table_step_backward_ahead(mhte_multi_table* t, int32_t table, mhte_dedup_ws* ws,
                                           mhte_dedup_ws* ws_next, const int64_t* unique_ids,
                                           int64_t n_max, const uint32_t* n_unique_dev,
                                           const float* grads, int64_t n, float* grad_unique,
                                           const float* learning_rate, int64_t n_learning_rate,
                                           int64_t update_time, int64_t global_step, int32_t flags,
                                           mhte_dedup_ws* ws_ahead, const int64_t* id_ahead,
                                           int64_t n_ahead, int64_t* unique_ids_ahead,
                                           uint32_t* n_unique_dev_ahead, void* stream) {
  return guard([&] {
    HostProfScope hps(1);
    Table& tb = table_at(t, table);
    // (the lock first: the refusal below reads the attachment, and does not depend on the batch)
    std::lock_guard<std::mutex> g(tb.mu);
    hps.locked();
    tb.refuse_retriever("step_backward");
    if (t->touched && tb.flt_slots)
      throw Error(MHTE_INVALID_ARGUMENT, "step_backward: a table with an admission filter AND a touched-key set "
                                         "takes the op-level update (mhte_table_sum_optimize_n): the fused step "
                                         "decides admission inside its apply role");
    if (!ws || ws == ws_next)
      throw Error(MHTE_INVALID_ARGUMENT, "step_backward needs the batch's workspace, distinct "
                                         "from the next batch's");
    if (ws_ahead && (ws_ahead == ws || ws_ahead == ws_next))
      throw Error(MHTE_INVALID_ARGUMENT, "step_backward: the workspace of the batch two ahead must be "
                                         "a third one");
    if (ws_ahead && (!id_ahead || !unique_ids_ahead || !n_unique_dev_ahead))
      throw Error(MHTE_INVALID_ARGUMENT, "step_backward: null argument for the batch two ahead");
    if (!learning_rate || n_learning_rate < int64_t(tb.nseg))
      throw Error(MHTE_INVALID_ARGUMENT, "The length of tensor `learning_rate` is too short.");
    if (!n_unique_dev || !grad_unique || !unique_ids || !grads)
      throw Error(MHTE_INVALID_ARGUMENT, "step_backward: null argument");
    if (!tb.fusable())
      throw Error(MHTE_INVALID_ARGUMENT, "step_backward: row too wide (or a whole-segment optimizer) "
                                         "for the fused step");
    // refused before anything changes: no update time noted, the run dedup of the batch two ahead not begun,
    // the queued displacement pass and the workspace's probe left as they are
    tb.fused_shape("step_backward", {{"grads", grads}, {"grad_unique", grad_unique}});
    HIP_OK(hipSetDevice(t->device));
    tb.note_update_time(update_time);
    RunView ahead{};
    if (ws_ahead)
      ahead = ws_ahead->ws.begin_run_dedup(id_ahead, n_ahead, unique_ids_ahead, n_unique_dev_ahead, S(stream));
    tb.step_backward(ws->ws, ws_next ? &ws_next->ws : nullptr, unique_ids, n_max, n_unique_dev,
                     grads, n, grad_unique, learning_rate, update_time,
                     (flags & MHTE_EXACT_ORDER) != 0, S(stream), global_step, ahead);
    if (tb.evict_enabled && lib_now() - tb.last_evict >= tb.evict_every_s) {
      // (the scan must not overtake the displacement pass this update left for the next forward)
      tb.finish_pending(S(stream));
      tb.maybe_evict(S(stream));
    }
    tk_record(t, tb, table, unique_ids, n_max, n_unique_dev, S(stream));
  });
}

mhte_status mhte_table_finish_pending(mhte_multi_table* t, int32_t table, void* stream) {
  return guard([&] {
    Table& tb = table_at(t, table);
    HIP_OK(hipSetDevice(t->device));
    std::lock_guard<std::mutex> g(tb.mu);
    tb.finish_pending(S(stream));
  });
}

int32_t mhte_table_fused_backward_ok(const mhte_multi_table* t, int32_t i) {
  if (!(t && i >= 0 && i < int32_t(t->tables.size()) && t->tables[i]->fusable())) return 0;
  return t->tables[i]->basic_opts() ? 1 : 2;
}

mhte_status mhte_table_set_retriever(mhte_multi_table* t, int32_t table, int32_t segment, int32_t type,
                                     const float* params, int32_t n_params) {
  return guard([&] {
    Table& tb = table_at(t, table);
    HIP_OK(hipSetDevice(t->device));
    std::lock_guard<std::mutex> link(g_touched_link_mu);   // (before the table's, as everywhere: the step lists)
    std::lock_guard<std::mutex> g(tb.mu);
    if (type != MHTE_RETRIEVER_RAW && (!t->multi_steps.empty() || !t->shard_steps.empty()))
      throw Error(MHTE_FAILED_PRECONDITION, "set_retriever: a multi-table or id-sharded step exists on this "
                                            "MultiHashTable; its kernels read rows raw");
    tb.set_retriever(segment, type, params, n_params);
  });
}

mhte_status mhte_table_get_retriever(mhte_multi_table* t, int32_t table, int32_t segment, int32_t* type,
                                     float* params, int32_t cap) {
  return guard([&] {
    Table& tb = table_at(t, table);
    if (segment < 0 || segment >= int32_t(tb.nseg) || !type)
      throw Error(MHTE_INVALID_ARGUMENT, "get_retriever: bad segment or null argument");
    std::lock_guard<std::mutex> g(tb.mu);
    const Table::Retriever& r = tb.retrievers[segment];
    *type = r.type;
    const int32_t np = r.type == kRetFakeQuant ? 1 : (r.type == kRetHashNet ? 4 : 0);
    for (int32_t i = 0; params && i < np && i < cap; ++i) params[i] = r.p[i];
  });
}

mhte_status mhte_table_hash_net_scale(mhte_multi_table* t, int32_t table, int32_t segment, float* host_out,
                                      void* stream) {
  return guard([&] {
    Table& tb = table_at(t, table);
    if (!host_out) throw Error(MHTE_INVALID_ARGUMENT, "hash_net_scale: null argument");
    HIP_OK(hipSetDevice(t->device));
    std::lock_guard<std::mutex> g(tb.mu);
    if (segment < 0 || segment >= int32_t(tb.nseg) || tb.retrievers[segment].type != kRetHashNet)
      throw Error(MHTE_INVALID_ARGUMENT, "hash_net_scale: table " + tb.name + " segment " +
                                             std::to_string(segment) + " has no hash_net retriever");
    tb.finish_pending(S(stream));
    HIP_OK(hipMemcpyAsync(host_out, tb.d_scale + segment, sizeof(float), hipMemcpyDeviceToHost, S(stream)));
    HIP_OK(hipStreamSynchronize(S(stream)));
  });
}

mhte_status mhte_value_offsets(const uint32_t* seg_off, const uint32_t* seg_pos,
                               const uint32_t* n_unique_dev, int64_t n, int64_t value_base,
                               int64_t dim, int64_t split_base, int64_t* value_offset,
                               int64_t* value_offset_split, void* stream) {
  return guard([&] {
    if (n <= 0) return;
    hipStream_t st = S(stream);
    offsets_from_positions_kernel<<<dim3(uint32_t((n + 255) / 256)), 256, 0, st>>>(
        seg_pos, uint32_t(n), value_base, dim, value_offset);
    widen_offsets_kernel<<<dim3(uint32_t((n + 1 + 255) / 256)), 256, 0, st>>>(
        seg_off, n_unique_dev, split_base, value_offset_split);
    HIP_OK(hipGetLastError());
  });
}

mhte_status mhte_fill_with_offset_map(const int64_t* pos, int64_t n, const float* value,
                                      const int64_t* value_offset_map,
                                      const int64_t* value_offset_map_split, int32_t dim,
                                      int32_t offsets_vec4, float* value_buffer, void* stream) {
  return guard([&] {
    if (n <= 0) return;
    if (dim <= 0) throw Error(MHTE_INVALID_ARGUMENT, "dim must be > 0");
    Shape sh = pick_shape(uint32_t(dim), offsets_vec4 && dim % 4 == 0 && aligned16(value) &&
                                             aligned16(value_buffer));
    const dim3 grid(uint32_t((n * sh.G + 255) / 256));
    hipStream_t st = S(stream);
    for_shape(sh, [&](auto g_, auto v_) {
      scatter_offsets_kernel<decltype(g_)::value, decltype(v_)::value><<<grid, 256, 0, st>>>(
          pos, n, value, value_offset_map, value_offset_map_split, uint32_t(dim), value_buffer);
    });
    HIP_OK(hipGetLastError());
  });
}

mhte_status mhte_fill_with_offset_map_gradient(const int64_t* pos, int64_t n, const float* grad,
                                               const int64_t* grad_offset_map,
                                               const int64_t* grad_offset_map_split, int32_t dim,
                                               int32_t offsets_vec4, float* backprop_grad,
                                               void* stream) {
  return guard([&] {
    if (n <= 0) return;
    if (dim <= 0) throw Error(MHTE_INVALID_ARGUMENT, "dim must be > 0");
    Shape sh = pick_shape(uint32_t(dim), offsets_vec4 && dim % 4 == 0 && aligned16(grad) &&
                                             aligned16(backprop_grad));
    const dim3 grid(uint32_t((n * sh.G + 255) / 256));
    hipStream_t st = S(stream);
    for_shape(sh, [&](auto g_, auto v_) {
      gather_sum_offsets_kernel<decltype(g_)::value, decltype(v_)::value><<<grid, 256, 0, st>>>(
          pos, n, grad, grad_offset_map, grad_offset_map_split, uint32_t(dim), backprop_grad);
    });
    HIP_OK(hipGetLastError());
  });
}

mhte_status mhte_table_set_count_hits(mhte_multi_table* t, int32_t table, int32_t enable) {
  return guard([&] {
    Table& tb = table_at(t, table);
    std::lock_guard<std::mutex> g(tb.mu);
    tb.count_hits = enable != 0;
    ++tb.view_version;
  });
}

// ---- fused_embedding_to_layout ------------------------------------------------------------------
extern "C++" {
namespace mhte {
static void layout_launch(bool forward, const float* const* embeddings, const int32_t* emb_stride,
                          const int64_t* emb_count, int32_t n_emb, const unsigned long long* fid_offset,
                          int64_t n_fid, const int32_t* feature_offset, int64_t n_feature,
                          const uint32_t* nfl_offset, int32_t n_nfl, int32_t batch,
                          const mhte_layout_slice* slices, int32_t n_slices, float* const* outputs,
                          const int64_t* output_len, int32_t n_outputs, int32_t flags, hipStream_t st) {
  if (n_emb < 0 || n_outputs < 0 || n_emb > (1 << 20) || n_outputs > (1 << 20))
    throw Error(MHTE_INVALID_ARGUMENT, "layout: bad matrix / output count");
  if (batch < 0 || n_slices < 0 || n_fid > INT32_MAX || n_feature > INT32_MAX)
    throw Error(MHTE_INVALID_ARGUMENT, "layout: bad sizes");
  // Few matrices and outputs (a model's tables: the training path) travel in the kernel arguments.
  // More of them (one matrix per (table, shard, feature) as the reference's parameter-server path
  // hands them over: ~1000 in its own test) go through pointer tables uploaded for the call.
  const bool ext = n_emb > kMaxLayoutEmb || n_outputs > kMaxLayoutOut;
  struct Blob {
    char* d = nullptr;
    hipStream_t st;
    ~Blob() {
      if (d && hipFreeAsync(d, st) != hipSuccess) {
        (void)hipGetLastError();
        (void)hipStreamSynchronize(st);
        (void)hipFree(d);
      }
    }
  } blob;
  blob.st = st;
  // ---- forward, copy form, one launch: do the slices (plus zero runs for the columns between them) write
  // every float of their outputs?  Then layout_rows_kernel writes the zeros too and the fill in front
  // of it — a pass over the whole output: 268 MB at configs[4]'s shape — is left out for those outputs.
  static const bool rows_form = !(getenv("MHTE_LAYOUT_ROWS") && atoi(getenv("MHTE_LAYOUT_ROWS")) == 0);
  std::vector<char> out_written(size_t(std::max(n_outputs, 0)), 0);
  std::vector<LayoutTask> zero_runs;
  if (forward && !ext && rows_form && (flags & MHTE_LAYOUT_ONE_FID_UNIQUE_ROWS) != 0 && n_fid == n_feature &&
      n_slices > 0 && n_slices <= kMaxLayoutTasks && batch > 0) {
    bool ok = true;
    int64_t cols = 0;
    for (int32_t i = 0; ok && i < n_slices; ++i) {
      const mhte_layout_slice& sc = slices[i];
      ok = sc.out_type != 2 && sc.pooling != kPoolFirstN && sc.out_index >= 0 && sc.out_index < n_outputs &&
           sc.dim > 0 && sc.start >= 0 && sc.out_offset >= 0 && sc.out_row_floats > 0 &&
           ((sc.start | sc.dim | sc.out_offset | sc.out_row_floats) & 3) == 0 && aligned16(outputs[sc.out_index]);
      cols += sc.dim / 4;
    }
    for (int32_t i = 0; ok && i < n_emb; ++i) ok = (emb_stride[i] & 3) == 0 && aligned16(embeddings[i]);
    std::vector<char> covered(size_t(n_outputs), 0);
    for (int32_t o = 0; ok && o < n_outputs; ++o) {
      std::vector<std::pair<int32_t, int32_t>> runs;   // (offset, width) of the slices of output o
      int32_t stride = 0;
      for (int32_t i = 0; ok && i < n_slices; ++i)
        if (slices[i].out_index == o) {
          if (stride && stride != slices[i].out_row_floats) ok = false;
          stride = slices[i].out_row_floats;
          runs.emplace_back(slices[i].out_offset, slices[i].dim);
        }
      if (!ok || runs.empty()) continue;
      if (output_len[o] != int64_t(batch) * stride) continue;   // (rows beyond the batch: the fill stays)
      std::sort(runs.begin(), runs.end());
      int32_t pos = 0;
      std::vector<LayoutTask> gaps;
      bool tiles = true;
      for (auto& r : runs) {
        if (r.first < pos) { tiles = false; break; }            // overlapping slices: the fill stays
        if (r.first > pos) {
          LayoutTask z{};
          z.nfl_idx = -2;
          z.dim = r.first - pos;
          z.pooling = kPoolZeroFill;
          z.out_index = o;
          z.out_offset = pos;
          z.out_stride = stride;
          gaps.push_back(z);
        }
        pos = r.first + r.second;
      }
      if (!tiles || pos > stride) continue;
      if (pos < stride) {
        LayoutTask z{};
        z.nfl_idx = -2;
        z.dim = stride - pos;
        z.pooling = kPoolZeroFill;
        z.out_index = o;
        z.out_offset = pos;
        z.out_stride = stride;
        gaps.push_back(z);
      }
      int64_t gcols = 0;
      for (auto& z : gaps) gcols += z.dim / 4;
      if (size_t(n_slices) + zero_runs.size() + gaps.size() > size_t(kMaxLayoutTasks) ||
          cols + gcols > kLayoutRowsMaxF)
        continue;
      cols += gcols;
      zero_runs.insert(zero_runs.end(), gaps.begin(), gaps.end());
      covered[size_t(o)] = 1;
    }
    if (ok && cols <= kLayoutRowsMaxF) out_written = covered;
    else zero_runs.clear();
  }
  auto zero_buffers = [&](float* const* bufs, const int64_t* lens, int32_t n, const std::vector<char>* skip) {
    LayoutZeroArgs Z{};
    int32_t m = 0;
    uint64_t longest = 0;
    auto flush = [&] {
      if (m == 0 || longest == 0) { m = 0; longest = 0; return; }
      const uint32_t gx = uint32_t(std::min<uint64_t>(512, (longest + 4095) / 4096));
      layout_zero_args_kernel<<<dim3(gx, uint32_t(m)), 256, 0, st>>>(Z);
      HIP_OK(hipGetLastError());
      m = 0;
      longest = 0;
    };
    for (int32_t i = 0; i < n; ++i) {
      if (lens[i] <= 0 || (skip && (*skip)[size_t(i)])) continue;
      Z.p[m] = bufs[i];
      Z.len[m] = uint64_t(lens[i]);
      longest = std::max(longest, Z.len[m]);
      if (++m == kLayoutZeroBufs) flush();
    }
    flush();
  };
  LayoutArgs A{};
  if (ext) {
    const size_t o_emb = 0, o_out = o_emb + size_t(n_emb) * 8, o_len = o_out + size_t(n_outputs) * 8,
                 o_str = o_len + size_t(std::max(n_emb, n_outputs)) * 8, o_cnt = o_str + size_t(n_emb) * 4,
                 total = o_cnt + size_t(n_emb) * 4;
    std::vector<char> h(total, 0);
    memcpy(h.data() + o_emb, embeddings, size_t(n_emb) * 8);
    memcpy(h.data() + o_out, outputs, size_t(n_outputs) * 8);
    uint64_t* len = reinterpret_cast<uint64_t*>(h.data() + o_len);
    uint32_t* str = reinterpret_cast<uint32_t*>(h.data() + o_str);
    uint32_t* cnt = reinterpret_cast<uint32_t*>(h.data() + o_cnt);
    uint64_t longest = 0;
    if (forward) for (int32_t i = 0; i < n_outputs; ++i) longest = std::max(longest, len[i] = uint64_t(std::max<int64_t>(0, output_len[i])));
    else for (int32_t i = 0; i < n_emb; ++i) longest = std::max(longest, len[i] = uint64_t(std::max<int64_t>(0, emb_count[i])));
    for (int32_t i = 0; i < n_emb; ++i) {
      str[i] = uint32_t(emb_stride[i]);
      cnt[i] = uint32_t(emb_count[i]);
    }
    void* d = nullptr;
    if (hipMallocAsync(&d, total, st) != hipSuccess) {
      (void)hipGetLastError();
      HIP_OK(hipMalloc(&d, total));
    }
    blob.d = static_cast<char*>(d);
    PinnedStage::of(current_device()).upload(blob.d, h.data(), total, st);   // (no wait for the stream)
    A.x_emb = reinterpret_cast<const float* const*>(blob.d + o_emb);
    A.x_out = reinterpret_cast<float* const*>(blob.d + o_out);
    A.x_stride = reinterpret_cast<const uint32_t*>(blob.d + o_str);
    A.x_count = reinterpret_cast<const uint32_t*>(blob.d + o_cnt);
    const int32_t nz = forward ? n_outputs : n_emb;   // SetZeroFunctor: rows without fids stay zero
    if (nz > 0 && longest > 0) {
      const uint32_t gx = uint32_t(std::min<uint64_t>(64, (longest + 1023) / 1024));
      layout_zero_kernel<<<dim3(gx, uint32_t(nz)), 256, 0, st>>>(
          reinterpret_cast<float* const*>(blob.d + (forward ? o_out : o_emb)),
          reinterpret_cast<const uint64_t*>(blob.d + o_len));
      HIP_OK(hipGetLastError());
    }
  } else {
    // SetZeroFunctor: rows without fids stay zero (one launch over all buffers; outputs the copy launch
    // below writes in full are left to it)
    if (forward) zero_buffers(outputs, output_len, n_outputs, &out_written);
    else zero_buffers(const_cast<float* const*>(embeddings), emb_count, n_emb, nullptr);
  }
  if (batch == 0 || n_slices == 0) return;
  if (!ext) {
    for (int32_t i = 0; i < n_emb; ++i) {
      A.emb[i] = embeddings[i];
      A.emb_stride[i] = uint32_t(emb_stride[i]);
      A.emb_count[i] = uint32_t(emb_count[i]);
    }
    for (int32_t i = 0; i < n_outputs; ++i) A.out[i] = outputs[i];
  }
  A.fid_offset = fid_offset;
  A.feature_offset = feature_offset;
  A.nfl_offset = nfl_offset;
  A.n_fid = int32_t(n_fid);
  A.n_feature = int32_t(n_feature);
  A.n_nfl = n_nfl;
  A.batch = batch;
  A.n_emb = n_emb;
  auto check_slice = [&](int32_t i, int32_t first_of_addn) {
    const mhte_layout_slice& sc = slices[i];
    if (sc.out_index < 0 || sc.out_index >= n_outputs || sc.dim <= 0 || sc.out_row_floats <= 0 ||
        int64_t(sc.out_offset) + int64_t(sc.dim) * (sc.pooling == 3 ? std::max(1, sc.max_sequence_length) : 1) >
            sc.out_row_floats ||
        int64_t(batch) * sc.out_row_floats > output_len[sc.out_index])
      throw Error(MHTE_INVALID_ARGUMENT, "layout: slice " + std::to_string(i) + " does not fit its output");
    if (sc.out_type == 2 && sc.pooling == 3)   // CHECK in the op's constructor
      throw Error(MHTE_INVALID_ARGUMENT, "layout: FIRSTN pooling cannot be added (ADDN)");
    if (sc.out_type == 2 && sc.dim != slices[first_of_addn].dim)
      throw Error(MHTE_INVALID_ARGUMENT, "layout: slices of an ADDN layout differ in width");
  };
  auto task_of = [&](const mhte_layout_slice& sc) {
    LayoutTask t{};
    t.nfl_idx = sc.feature_idx;
    t.start = sc.start;
    t.dim = sc.dim;
    t.pooling = sc.pooling;
    t.max_seq = sc.max_sequence_length;
    t.out_index = sc.out_index;
    t.out_offset = sc.out_offset;
    t.out_stride = sc.out_row_floats;
    return t;
  };
  // ---- the gradient without float atomics (general form; MHTE_POOL_ATOMICS=1 keeps the atomic one)
  // The flag's plain stores hold only while no element of a feature's row is named by two slices (the
  // same columns of one feature in a CONCAT and in a STACK layout, say): there the gradient is a sum of
  // two addends, and the call takes the form it would take without the flag.  The forward only reads.
  bool copy_form = (flags & MHTE_LAYOUT_ONE_FID_UNIQUE_ROWS) != 0 && n_fid == n_feature;
  if (!forward && copy_form) {
    std::vector<std::pair<int32_t, int32_t>> order;   // (feature, slice) by feature, then start
    order.reserve(size_t(n_slices));
    for (int32_t i = 0; i < n_slices; ++i) order.emplace_back(slices[i].feature_idx, i);
    std::sort(order.begin(), order.end(), [&](const std::pair<int32_t, int32_t>& a, const std::pair<int32_t, int32_t>& b) {
      return a.first != b.first ? a.first < b.first : slices[a.second].start < slices[b.second].start;
    });
    int64_t end = 0;   // one past the last column a slice of the current feature has named so far
    for (size_t i = 0; copy_form && i < order.size(); ++i) {
      const mhte_layout_slice& sc = slices[order[i].second];
      if (i == 0 || order[i].first != order[i - 1].first) end = INT64_MIN;
      if (int64_t(sc.start) < end) copy_form = false;
      end = std::max(end, int64_t(sc.start) + std::max(sc.dim, 0));
    }
  }
  if (!forward && !copy_form && !pool_atomics() && n_fid > 0) {
    std::vector<LayoutTask> tasks(static_cast<size_t>(n_slices));
    std::vector<uint32_t> t_off(size_t(n_nfl) + 1, 0), t_idx;
    for (int32_t i = 0, first = 0; i < n_slices; ++i) {
      if (i == 0 || slices[i].out_type != 2 || slices[i - 1].out_type != 2 ||
          slices[i].out_index != slices[i - 1].out_index)
        first = i;
      check_slice(i, first);
      tasks[size_t(i)] = task_of(slices[i]);
      if (slices[i].feature_idx >= 0 && slices[i].feature_idx < n_nfl) ++t_off[size_t(slices[i].feature_idx) + 1];
    }
    for (int32_t i = 0; i < n_nfl; ++i) t_off[size_t(i) + 1] += t_off[size_t(i)];
    t_idx.resize(t_off[size_t(n_nfl)]);
    {
      std::vector<uint32_t> cur(t_off.begin(), t_off.end() - 1);
      for (int32_t i = 0; i < n_slices; ++i)
        if (slices[i].feature_idx >= 0 && slices[i].feature_idx < n_nfl)
          t_idx[cur[size_t(slices[i].feature_idx)]++] = uint32_t(i);
    }
    const size_t o_task = 0, o_off = o_task + tasks.size() * sizeof(LayoutTask),
                 o_idx = o_off + t_off.size() * 4, o_qf = (o_idx + t_idx.size() * 4 + 15) & ~size_t(15),
                 o_qseq = o_qf + size_t(n_fid) * 4, o_fnfl = o_qseq + size_t(n_fid) * 4,
                 o_kflag = o_fnfl + size_t(std::max<int64_t>(1, n_feature)) * 4,   // (zeroed from here)
                 o_nheavy = o_kflag + size_t(n_fid) * 4, o_heavy = o_nheavy + 16,
                 o_cpos = o_heavy + size_t(n_fid) * 4, total = o_cpos + size_t(n_fid) * 4;
    struct Tmp {   // (freed in stream order behind the kernels that read it)
      char* d = nullptr;
      hipStream_t st;
      ~Tmp() {
        if (d && hipFreeAsync(d, st) != hipSuccess) {
          (void)hipGetLastError();
          (void)hipStreamSynchronize(st);
          (void)hipFree(d);
        }
      }
    } tmp;
    tmp.st = st;
    void* d = nullptr;
    if (hipMallocAsync(&d, total, st) != hipSuccess) {
      (void)hipGetLastError();
      HIP_OK(hipMalloc(&d, total));
    }
    tmp.d = static_cast<char*>(d);
    std::vector<char> h(o_qf, 0);
    memcpy(h.data() + o_task, tasks.data(), tasks.size() * sizeof(LayoutTask));
    memcpy(h.data() + o_off, t_off.data(), t_off.size() * 4);
    if (!t_idx.empty()) memcpy(h.data() + o_idx, t_idx.data(), t_idx.size() * 4);
    PinnedStage::of(current_device()).upload(tmp.d, h.data(), o_qf, st);   // (no wait for the stream)
    HIP_OK(hipMemsetAsync(tmp.d + o_qf, 0xff, o_kflag - o_qf, st));   // qf = -1, fnfl = ~0
    HIP_OK(hipMemsetAsync(tmp.d + o_kflag, 0, o_heavy - o_kflag, st));   // kflag, n_heavy
    AuxWs& ws = AuxWs::of(current_device());
    std::lock_guard<std::mutex> g(ws.mu);
    AuxWs::Use use_(ws, st);
    ws.group(reinterpret_cast<const int64_t*>(fid_offset), n_fid, st);
    LayoutLists X{};
    X.tasks = reinterpret_cast<const LayoutTask*>(tmp.d + o_task);
    X.nfl_task_off = reinterpret_cast<const uint32_t*>(tmp.d + o_off);
    X.nfl_tasks = reinterpret_cast<const uint32_t*>(tmp.d + o_idx);
    X.qf = reinterpret_cast<int32_t*>(tmp.d + o_qf);
    X.qseq = reinterpret_cast<uint32_t*>(tmp.d + o_qseq);
    X.fnfl = reinterpret_cast<uint32_t*>(tmp.d + o_fnfl);
    X.ukeys = ws.uids.p;
    X.nu = ws.nu.p;
    X.seg_off = ws.seg_off.p;
    X.seg_pos = ws.seg_pos.p;
    X.inverse = ws.inverse.p;
    X.kflag = reinterpret_cast<uint32_t*>(tmp.d + o_kflag);
    X.n_heavy = reinterpret_cast<uint32_t*>(tmp.d + o_nheavy);
    X.heavy = reinterpret_cast<uint32_t*>(tmp.d + o_heavy);
    X.cpos = reinterpret_cast<uint32_t*>(tmp.d + o_cpos);
    const int64_t inst = int64_t(n_nfl) * batch;
    if (inst > 0) layout_qmap_kernel<<<dim3(uint32_t((inst + 255) / 256)), 256, 0, st>>>(A, X);
    layout_heavy_select_kernel<<<dim3(uint32_t((n_fid + 255) / 256)), 256, 0, st>>>(A, X);
    layout_grad_lists_kernel<<<dim3(uint32_t((n_fid * 16 + 255) / 256)), 256, 0, st>>>(A, X);
    // (heavy rows: persistent workgroups over the list the select kernel made; rows are disjoint
    // from the light ones, so the two launches' order does not matter)
    int cus = 0;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, current_device()) != hipSuccess || cus <= 0)
      cus = 256;
    layout_grad_heavy_kernel<<<dim3(uint32_t(std::min<int64_t>(2 * cus, n_fid / kLayoutLight + 64))),
                               1024, 0, st>>>(A, X);
    HIP_OK(hipGetLastError());
    return;
  }
  int32_t k = 0;
  bool addn_open = false;   // the previous launch ended inside an ADDN layout: its next slices add on
  while (k < n_slices) {
    // one launch per kMaxLayoutTasks slices.  An ADDN layout's slices are added in configuration
    // order by one lane group; a layout with more slices than a launch holds continues in the next
    // launch, which starts from the sums the previous one stored (same order, same roundings).
    int32_t nt = 0, nu = 0;
    while (k < n_slices) {
      int32_t span = 1;
      if (slices[k].out_type == 2)
        while (k + span < n_slices && slices[k + span].out_type == 2 &&
               slices[k + span].out_index == slices[k].out_index) ++span;
      const bool cont = addn_open;
      // (forward) a slice that writes floats an earlier slice of this launch writes too starts the next
      // launch: launches run in stream order, so the later slice's values stay, as in the op's own loop
      // (inside one launch the two stores come from different lanes or workgroups, in no order)
      bool clash = false;
      for (int32_t q = 0; forward && !clash && q < nt; ++q) {
        const LayoutTask& t = A.task[q];
        const mhte_layout_slice& sc = slices[k];
        if (t.out_index != sc.out_index) continue;
        const int64_t w0 = int64_t(t.dim) * (t.pooling == kPoolFirstN ? std::max(1, t.max_seq) : 1),
                      w1 = int64_t(sc.dim) * (sc.pooling == kPoolFirstN ? std::max(1, sc.max_sequence_length) : 1);
        clash = t.out_stride != sc.out_row_floats ||
                (int64_t(sc.out_offset) < t.out_offset + w0 && int64_t(t.out_offset) < sc.out_offset + w1);
      }
      if (clash) break;
      if (span > kMaxLayoutTasks) {
        if (nt > 0) break;             // (a long ADDN layout starts its own launch)
        span = kMaxLayoutTasks;
        addn_open = true;
      } else {
        if (nt + span > kMaxLayoutTasks) break;
        addn_open = false;
      }
      for (int32_t q = 0; q < span; ++q) {
        check_slice(k + q, k);
        A.task[nt + q] = task_of(slices[k + q]);
      }
      A.unit[nu].first = uint16_t(nt);
      A.unit[nu].count = uint16_t(span);
      A.unit[nu].addn = slices[k].out_type == 2 ? (cont ? 2 : 1) : 0;
      ++nu;
      nt += span;
      k += span;
    }
    // (the zero runs of outputs this launch writes in full: slices like any other)
    const bool whole_rows = !zero_runs.empty() || std::find(out_written.begin(), out_written.end(), 1) != out_written.end();
    if (whole_rows) {
      for (auto& z : zero_runs) {
        A.task[nt] = z;
        A.unit[nu].first = uint16_t(nt);
        A.unit[nu].count = 1;
        A.unit[nu].addn = 0;
        ++nu;
        ++nt;
      }
      // (one bit per output; whole rows are decided without pointer tables only: at most kMaxLayoutOut outputs)
      uint32_t mask = 0;
      for (size_t o = 0; o < out_written.size() && o < 32; ++o)
        if (out_written[o]) mask |= 1u << o;
      A.zero_missing = int32_t(mask);
    }
    A.n_units = nu;
    const dim3 grid(uint32_t((int64_t(batch) * 16 + 255) / 256), uint32_t(nu));
    // one fid per feature instance (asserted by the caller), copies of float4-aligned slices: the
    // vector copy form, plain stores for the gradient
    bool fast = copy_form;
    for (int32_t q = 0; fast && q < nt; ++q) {
      const LayoutTask& t = A.task[q];
      fast = t.pooling != kPoolFirstN && ((t.start | t.dim | t.out_offset | t.out_stride) & 3) == 0 &&
             aligned16(outputs[t.out_index]);
    }
    for (int32_t q = 0; fast && q < nu; ++q) fast = A.unit[q].count == 1;
    for (int32_t i = 0; fast && i < n_emb; ++i) fast = (emb_stride[i] & 3) == 0 && aligned16(embeddings[i]);
    // ... a workgroup per 16 batch rows over all slices of the launch when a row's float4 columns fit its
    // column table (layout_rows_kernel; MHTE_LAYOUT_ROWS=0: a lane group per (slice, row), round 2's form)
    int64_t cols = 0;
    for (int32_t q = 0; q < nu; ++q) cols += A.task[A.unit[q].first].dim / 4;
    if (fast && rows_form && cols > 0 && cols <= kLayoutRowsMaxF) {
      const dim3 rgrid(uint32_t((int64_t(batch) + kLayoutRowsR - 1) / kLayoutRowsR));
      if (forward) layout_rows_kernel<true><<<rgrid, 256, 0, st>>>(A);
      else layout_rows_kernel<false><<<rgrid, 256, 0, st>>>(A);
    } else if (whole_rows) {
      throw Error(MHTE_INTERNAL, "layout: the launch that was to write whole output rows cannot run");
    } else if (fast) {
      if (forward) layout_copy_kernel<true><<<grid, 256, 0, st>>>(A);
      else layout_copy_kernel<false><<<grid, 256, 0, st>>>(A);
    } else {
      if (forward) layout_kernel<true><<<grid, 256, 0, st>>>(A);
      else layout_kernel<false><<<grid, 256, 0, st>>>(A);
    }
    HIP_OK(hipGetLastError());
  }
}
}  // namespace mhte
}  // extern "C++"

mhte_status mhte_embedding_to_layout(const float* const* embeddings, const int32_t* emb_row_floats,
                                     const int64_t* emb_len, int32_t n_emb, const uint64_t* fid_offset,
                                     int64_t n_fid, const int32_t* feature_offset, int64_t n_feature,
                                     const uint32_t* nfl_offset, int32_t n_nfl, int32_t batch_size,
                                     const mhte_layout_slice* slices, int32_t n_slices,
                                     float* const* outputs, const int64_t* output_len, int32_t n_outputs,
                                     int32_t flags, void* stream) {
  return guard([&] {
    layout_launch(true, embeddings, emb_row_floats, emb_len, n_emb,
                  reinterpret_cast<const unsigned long long*>(fid_offset), n_fid, feature_offset, n_feature,
                  nfl_offset, n_nfl, batch_size, slices, n_slices, outputs, output_len, n_outputs, flags,
                  S(stream));
  });
}

mhte_status mhte_embedding_to_layout_grad(float* const* embeddings_grad, const int32_t* emb_row_floats,
                                          const int64_t* emb_len, int32_t n_emb, const uint64_t* fid_offset,
                                          int64_t n_fid, const int32_t* feature_offset, int64_t n_feature,
                                          const uint32_t* nfl_offset, int32_t n_nfl, int32_t batch_size,
                                          const mhte_layout_slice* slices, int32_t n_slices,
                                          const float* const* tensors_grad, const int64_t* tensor_len,
                                          int32_t n_tensors, int32_t flags, void* stream) {
  return guard([&] {
    layout_launch(false, const_cast<const float* const*>(embeddings_grad), emb_row_floats, emb_len, n_emb,
                  reinterpret_cast<const unsigned long long*>(fid_offset), n_fid, feature_offset, n_feature,
                  nfl_offset, n_nfl, batch_size, slices, n_slices,
                  (float* const*)tensors_grad,
                  tensor_len, n_tensors, flags, S(stream));
  });
}

// ---- boundary completion: proto configs, entry lookup, feature stat -------------------------------
mhte_status mhte_hash_filter_create_from_proto(uint64_t capacity, int32_t split_num,
                                               const void* config, int64_t config_len,
                                               int32_t device, mhte_hash_filter** out) {
  mhte_status st = mhte_hash_filter_create(capacity, split_num, device, out);
  if (st != MHTE_OK) return st;
  return guard([&] {
    try {
      mhte_hash_filter* f = *out;
      if (config && config_len > 0) {
        pcfg::parse_occurrence(config, size_t(config_len), &f->occ_default, &f->occ_slots, &f->occ_thr);
        f->has_occ = true;
      }
    } catch (const ckpt::ProtoError& e) {
      mhte_hash_filter_destroy(*out);
      *out = nullptr;
      throw Error(MHTE_INVALID_ARGUMENT, e.what());
    }
  });
}

// MonolithProbabilisticFilter (ops/hash_filter_op.cc:81-110; probabilistic_filter.{h,cc}): no table
// of counts — admission is a draw per consultation (csrc/mhte_kernels.h prob_consult)
mhte_status mhte_hash_filter_create_probabilistic(int32_t equal_probability, uint64_t seed, const void* config,
                                                  int64_t config_len, int32_t device, mhte_hash_filter** out) {
  return guard([&] {
    if (!out) throw Error(MHTE_INVALID_ARGUMENT, "null out");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev)
      throw Error(MHTE_UNAVAILABLE, "no such HIP device");
    HIP_OK(hipSetDevice(device));
    std::unique_ptr<mhte_hash_filter> f(new mhte_hash_filter);
    f->device = device;
    f->nsplit = 0;                                    // the marker of the probabilistic kind
    f->total = equal_probability ? 1 : 0;
    f->stride = 0;
    HIP_OK(hipMalloc(&f->slots, 64 * sizeof(uint32_t)));   // (never read: "a filter is attached")
    HIP_OK(hipMemset(f->slots, 0, 64 * sizeof(uint32_t)));
    HIP_OK(hipMalloc(&f->state, sizeof(FilterState)));
    std::unique_ptr<FilterState> hs_heap(new FilterState);   // (256 KB: not on the stack)
    FilterState& hs = *hs_heap;
    memset(&hs, 0, sizeof(hs));
    if (seed == 0)   // (the reference seeds with time(0), xorshift.h:29-31)
      seed = uint64_t(std::chrono::steady_clock::now().time_since_epoch().count()) | 1ull;
    hs.failure_count = seed;
    HIP_OK(hipMemcpy(f->state, &hs, sizeof(hs), hipMemcpyHostToDevice));
    if (config && config_len > 0) {
      try {
        pcfg::parse_occurrence(config, size_t(config_len), &f->occ_default, &f->occ_slots, &f->occ_thr);
      } catch (const ckpt::ProtoError& e) {
        throw Error(MHTE_INVALID_ARGUMENT, e.what());
      }
      f->has_occ = true;
    }
    HIP_OK(hipDeviceSynchronize());
    *out = f.release();
  });
}

mhte_status mhte_multi_table_create_from_proto(const void* config, int64_t config_len,
                                               mhte_hash_filter* filter, uint64_t reserve_rows,
                                               float max_load_factor, int32_t device,
                                               const char* shared_name, float* learning_rates_out,
                                               int32_t learning_rates_cap, mhte_multi_table** out) {
  std::vector<pcfg::TableCfg> tabs;
  mhte_status st = guard([&] {
    if (!config || config_len <= 0 || !out) throw Error(MHTE_INVALID_ARGUMENT, "create: bad arguments");
    try {
      tabs = pcfg::parse_multi(config, size_t(config_len));
    } catch (const ckpt::ProtoError& e) {
      throw Error(MHTE_INVALID_ARGUMENT, std::string("Unable to parse config: ") + e.what());
    }
    if (tabs.empty()) throw Error(MHTE_INVALID_ARGUMENT, "config holds no table");
  });
  if (st != MHTE_OK) return st;
  std::vector<std::vector<mhte_segment_config>> segs(tabs.size());
  std::vector<mhte_table_config> cfgs(tabs.size());
  for (size_t i = 0; i < tabs.size(); ++i) {
    const pcfg::TableCfg& t = tabs[i];
    for (const auto& s : t.segs) segs[i].push_back(s.c);
    mhte_table_config& c = cfgs[i];
    memset(&c, 0, sizeof(c));
    c.name = t.name.c_str();
    c.n_segments = int32_t(segs[i].size());
    c.segments = segs[i].data();
    c.initial_capacity = t.initial_capacity;
    c.reserve_rows = reserve_rows;
    c.max_load_factor = max_load_factor;
    c.default_expire_days = t.default_expire == 0 ? -1 : t.default_expire;
    c.n_slot_expire = int32_t(t.expire_slots.size());
    c.expire_slots = t.expire_slots.data();
    c.expire_days = t.expire_days.data();
    if (filter && filter->has_occ) {
      c.default_occurrence_threshold = filter->occ_default;
      c.n_slot_occurrence = int32_t(filter->occ_slots.size());
      c.occurrence_slots = filter->occ_slots.data();
      c.occurrence_thresholds = filter->occ_thr.data();
    }
    c.enable_feature_eviction = t.enable_eviction ? 1 : 0;
    c.feature_evict_every_n_hours = t.evict_every_n_hours;
  }
  st = mhte_multi_table_create(cfgs.data(), int32_t(cfgs.size()), device, shared_name, out);
  if (st != MHTE_OK) return st;
  if (filter) {
    st = mhte_multi_table_set_filter(*out, filter);
    if (st != MHTE_OK) {
      mhte_multi_table_destroy(*out);
      *out = nullptr;
      return st;
    }
  }
  // comp_config -> the segments' retrievers (GenerateObjFromSegments, entry_accessor.cc:283-302)
  for (const auto& t : tabs)
    for (size_t k = 0; k < t.segs.size(); ++k) {
      const pcfg::Segment& s = t.segs[k];
      if (s.retriever == MHTE_RETRIEVER_RAW) continue;
      st = mhte_table_set_retriever(*out, mhte_table_index(*out, t.name.c_str()), int32_t(k), s.retriever,
                                    s.retriever_params, s.retriever == MHTE_RETRIEVER_HASH_NET ? 4 : 1);
      if (st != MHTE_OK) {
        mhte_multi_table_destroy(*out);
        *out = nullptr;
        return st;
      }
    }
  if (learning_rates_out) {  // sorted-name order, like the tables
    int32_t k = 0;
    for (auto& tb : (*out)->tables)
      for (const auto& t : tabs)
        if (t.name == tb->name)
          for (const auto& s : t.segs)
            if (k < learning_rates_cap) learning_rates_out[k++] = s.learning_rate;
  }
  return MHTE_OK;
}

namespace mhte {
// one thread per id: probe, then found flag, timestamp and the whole row (weights | optimizer ctx)
__global__ __launch_bounds__(256) void entry_fetch_kernel(TableView tv, const int64_t* __restrict__ ids,
                                                          int64_t n, int32_t* __restrict__ found,
                                                          uint32_t* __restrict__ ts,
                                                          float* __restrict__ rows) {
  const int64_t i = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int64_t id = ids[i];
  uint32_t r = kNoRow, t = 0;
  if (id == kEmptyKey) {
    if (tv.ctr->special_state == 1) {
      r = tv.ctr->special_row;
      t = tv.ctr->special_ts;
    }
  } else {
    const uint64_t hv = hash_key(id);
    const uint64_t i1 = index_hash(tv.hp, hv);
    const uint64_t i2 = alt_index(tv.hp, partial_key(hv), i1);
    for (int s = 0; s < kSlots; ++s) {
      if (tv.buckets[i1].key[s] == id) { r = tv.buckets[i1].row[s]; t = tv.buckets[i1].ts[s]; }
      if (tv.buckets[i2].key[s] == id) { r = tv.buckets[i2].row[s]; t = tv.buckets[i2].ts[s]; }
    }
  }
  found[i] = r != kNoRow;
  ts[i] = t;
  if (r != kNoRow) {
    const float* rp = row_ptr(tv, r);
    for (uint32_t e = 0; e < tv.row_floats; ++e) rows[i * tv.row_floats + e] = rp[e];
  }
}
}  // namespace mhte

mhte_status mhte_lookup_entry(mhte_multi_table* t, const int64_t* id, const int64_t* id_split,
                              int64_t n_split, char* entries, int64_t cap, int64_t* entry_offsets,
                              int64_t* needed, void* stream) {
  return guard([&] {
    check_handle(t);
    if (!id_split || n_split != int64_t(t->tables.size()) + 1)  // multi_hash_table_lookup_op.cc:101-103
      throw Error(MHTE_INVALID_ARGUMENT, "id_split must be " + std::to_string(t->tables.size() + 1) +
                                             ". Current: " + std::to_string(n_split));
    if (!entry_offsets || !needed) throw Error(MHTE_INVALID_ARGUMENT, "lookup_entry: null argument");
    HIP_OK(hipSetDevice(t->device));
    hipStream_t st = S(stream);
    std::string all, rec;
    std::vector<int64_t> offs;
    offs.push_back(0);
    for (size_t k = 0; k < t->tables.size(); ++k) {
      Table& tb = *t->tables[k];
      const int64_t n = id_split[k + 1] - id_split[k];
      if (n < 0) throw Error(MHTE_INVALID_ARGUMENT, "id_split not monotonic");
      if (n == 0) continue;
      std::lock_guard<std::mutex> g(tb.mu);
      tb.finish_pending(st);
      DevBuf<int32_t> d_found;
      DevBuf<uint32_t> d_ts;
      DevBuf<float> d_rows;
      d_found.reserve(n);
      d_ts.reserve(n);
      d_rows.reserve(size_t(n) * tb.row_floats);
      entry_fetch_kernel<<<dim3(uint32_t((n + 255) / 256)), 256, 0, st>>>(
          tb.view, id + id_split[k], n, d_found.p, d_ts.p, d_rows.p);
      HIP_OK(hipGetLastError());
      std::vector<int64_t> h_ids(n);
      std::vector<int32_t> h_found(n);
      std::vector<uint32_t> h_ts(n);
      std::vector<float> h_rows(size_t(n) * tb.row_floats);
      HIP_OK(hipMemcpyAsync(h_ids.data(), id + id_split[k], n * 8, hipMemcpyDeviceToHost, st));
      HIP_OK(hipMemcpyAsync(h_found.data(), d_found.p, n * 4, hipMemcpyDeviceToHost, st));
      HIP_OK(hipMemcpyAsync(h_ts.data(), d_ts.p, n * 4, hipMemcpyDeviceToHost, st));
      HIP_OK(hipMemcpyAsync(h_rows.data(), d_rows.p, h_rows.size() * 4, hipMemcpyDeviceToHost, st));
      HIP_OK(hipStreamSynchronize(st));
      const std::vector<ckpt::SegLayout> segs = seg_layout(tb);
      for (int64_t i = 0; i < n; ++i) {
        if (h_found[size_t(i)]) {
          ckpt::encode_entry(rec, h_ids[size_t(i)], h_rows.data() + size_t(i) * tb.row_floats, segs,
                             int(tb.dim), h_ts[size_t(i)]);
          all += rec;
        }
        offs.push_back(int64_t(all.size()));
      }
    }
    *needed = int64_t(all.size());
    memcpy(entry_offsets, offs.data(), offs.size() * sizeof(int64_t));
    if (int64_t(all.size()) > cap || (!entries && !all.empty()))
      throw Error(MHTE_INVALID_ARGUMENT, "lookup_entry: entries buffer too small: need " +
                                             std::to_string(all.size()));
    if (!all.empty()) memcpy(entries, all.data(), all.size());
  });
}

mhte_status mhte_table_save_as_tensor(mhte_multi_table* t, int32_t table, int32_t shard_idx,
                                      int32_t num_shards, int64_t limit, int64_t offset, int64_t* new_offset,
                                      char* entries, int64_t cap, int64_t* entry_offsets,
                                      int64_t offsets_cap, int64_t* n_entries, int64_t* needed, void* stream) {
  return guard([&] {
    save_as_tensor(t, table_at(t, table), shard_idx, num_shards, limit, offset, new_offset, entries, cap,
                   entry_offsets, offsets_cap, n_entries, needed, S(stream));
  });
}

mhte_status mhte_feature_stat(const char* basename, char* names, int64_t names_cap, uint64_t* counts,
                              int32_t cap, int32_t* n_out) {
  return guard([&] { feature_stat(basename, names, names_cap, counts, cap, n_out); });
}

// ---- multi-table pipelined step -----------------------------------------------------------------
mhte_status mhte_multi_step_create(mhte_multi_table* t, int64_t max_batch_per_table,
                                   mhte_multi_step** out) {
  return guard([&] {
    check_handle(t);
    if (!out) throw Error(MHTE_INVALID_ARGUMENT, "null out");
    HIP_OK(hipSetDevice(t->device));
    std::lock_guard<std::mutex> link(g_touched_link_mu);   // (before the tables', as everywhere)
    std::vector<std::unique_lock<std::mutex>> locks;
    for (auto& tb : t->tables) locks.emplace_back(tb->mu);
    for (auto& tb : t->tables) tb->refuse_retriever("multi step");
    if (t->touched && tk_any_filter(t))
      throw Error(MHTE_INVALID_ARGUMENT, "multi step: a MultiHashTable with an admission filter AND a touched-key "
                                         "set takes the op-level update: the fused step decides admission inside "
                                         "its apply role");
    std::unique_ptr<mhte_multi_step> s(new mhte_multi_step);
    s->ms.init(t, max_batch_per_table);
    const uint32_t T = s->ms.T;
    for (int sl = 0; sl < 2; ++sl) {
      s->h_tk[sl].assign(T, TkDesc{});
      for (uint32_t k = 0; k < T; ++k) {
        TkDesc& d = s->h_tk[sl][k];
        d.ids = s->ms.h_st[k].rv[sl].uids;
        d.n_dev = s->ms.h_st[k].rv[sl].n_unique;
        d.n_max = uint32_t(max_batch_per_table);
        d.tag = int32_t(k);
      }
    }
    HIP_OK(hipMalloc(&s->d_tk, sizeof(TkDesc) * 2 * T));
    for (int sl = 0; sl < 2; ++sl)
      HIP_OK(hipMemcpy(s->d_tk + size_t(sl) * T, s->h_tk[sl].data(), sizeof(TkDesc) * T, hipMemcpyHostToDevice));
    s->tk_skip.assign(T, 0);
    t->multi_steps.push_back(s.get());   // (behind the last call that can throw)
    s->counted = true;
    *out = s.release();
  });
}
void mhte_multi_step_destroy(mhte_multi_step* s) {
  if (s) {
    std::lock_guard<std::mutex> link(g_touched_link_mu);
    if (s->counted) {   // (false once the table went first: mhte_multi_table_destroy unlinks)
      auto& v = s->ms.mt->multi_steps;
      v.erase(std::remove(v.begin(), v.end(), s), v.end());
    }
  }
  delete s;
}

mhte_status mhte_multi_step_forward(mhte_multi_step* s, const int64_t* id, const int64_t* id_split,
                                    int64_t n_split, float* embedding, int64_t embedding_len,
                                    const int64_t* id_next, const int64_t* id_split_next,
                                    int64_t n_split_next, int32_t prefetched, void* stream) {
  return guard([&] {
    if (!s) throw Error(MHTE_INVALID_ARGUMENT, "null multi step");
    HIP_OK(hipSetDevice(s->ms.device));
    std::vector<std::unique_lock<std::mutex>> locks;
    for (auto& tb : s->ms.mt->tables) locks.emplace_back(tb->mu);
    s->ms.forward(id, id_split, n_split, embedding, embedding_len, id_next, id_split_next,
                  n_split_next, prefetched, S(stream));
  });
}

mhte_status mhte_multi_step_backward(mhte_multi_step* s, const float* value, int64_t value_len,
                                     const float* learning_rate, int64_t n_learning_rate,
                                     int64_t update_time, int64_t global_step, int32_t flags,
                                     void* stream) {
  return guard([&] {
    if (!s) throw Error(MHTE_INVALID_ARGUMENT, "null multi step");
    HIP_OK(hipSetDevice(s->ms.device));
    std::vector<std::unique_lock<std::mutex>> locks;
    for (auto& tb : s->ms.mt->tables) locks.emplace_back(tb->mu);
    mhte_touched_key_set* set = s->ms.mt->touched;
    if (set && tk_any_filter(s->ms.mt))
      throw Error(MHTE_INVALID_ARGUMENT, "multi step: an admission filter AND a touched-key set are attached");
    const int slot = s->ms.cur;
    s->ms.backward(value, value_len, learning_rate, n_learning_rate, update_time,
                   (flags & MHTE_EXACT_ORDER) != 0, S(stream), global_step);
    if (set) {
      const uint32_t T = s->ms.T;
      for (uint32_t k = 0; k < T; ++k) s->tk_skip[k] = s->ms.n_slot[slot][k] ? 0 : 1;
      std::lock_guard<std::mutex> g(set->mu);
      tk_enter_stream(*set, S(stream));
      tk_insert_segments(*set, s->h_tk[slot].data(), s->d_tk + size_t(slot) * T, T, s->tk_skip.data(), S(stream));
    }
  });
}

mhte_status mhte_multi_step_unique_counts(mhte_multi_step* s, int64_t* counts, void* stream) {
  return guard([&] {
    if (!s || !counts) throw Error(MHTE_INVALID_ARGUMENT, "null argument");
    MultiStep& ms = s->ms;
    HIP_OK(hipSetDevice(ms.device));
    if (ms.stage[ms.cur] != 2)
      throw Error(MHTE_FAILED_PRECONDITION, "multi step: the current batch has not been numbered");
    std::vector<uint32_t> h(ms.T, 0);
    for (uint32_t t = 0; t < ms.T; ++t)
      if (ms.n_slot[ms.cur][t])
        HIP_OK(hipMemcpyAsync(&h[t], ms.h_st[t].rv[ms.cur].n_unique, sizeof(uint32_t),
                              hipMemcpyDeviceToHost, S(stream)));
    HIP_OK(hipStreamSynchronize(S(stream)));
    for (uint32_t t = 0; t < ms.T; ++t) counts[t] = h[t];
  });
}

// ---- id-sharded multi-table step (mhte_shard_host.h) -------------------------------------------------
mhte_status mhte_shard_unique_id(void* out128) {
  return guard([&] {
    if (!out128) throw Error(MHTE_INVALID_ARGUMENT, "null out");
    Rccl& R = Rccl::get();
    ncclUniqueId id;
    R.ok(R.GetUniqueId(&id), "GetUniqueId");
    static_assert(sizeof(id) == 128, "ncclUniqueId");
    memcpy(out128, &id, sizeof(id));
  });
}

static std::vector<std::unique_lock<std::mutex>> lock_tables(mhte_shard_step** steps, int32_t n) {
  std::vector<std::unique_lock<std::mutex>> locks;
  for (int32_t r = 0; r < n; ++r)
    for (auto& tb : steps[r]->ss.mt->tables) locks.emplace_back(tb->mu);
  return locks;
}

mhte_status mhte_shard_step_create(mhte_multi_table* t, int64_t max_batch_per_table, int32_t rank,
                                   int32_t world, int64_t ids_per_peer_table, const void* unique_id,
                                   mhte_shard_step** out) {
  return guard([&] {
    check_handle(t);
    if (!out) throw Error(MHTE_INVALID_ARGUMENT, "null out");
    HIP_OK(hipSetDevice(t->device));
    std::lock_guard<std::mutex> link(g_touched_link_mu);   // (before the tables', as everywhere)
    std::vector<std::unique_lock<std::mutex>> locks;
    for (auto& tb : t->tables) locks.emplace_back(tb->mu);
    std::unique_ptr<mhte_shard_step> s(new mhte_shard_step);
    if (t->touched)
      throw Error(MHTE_INVALID_ARGUMENT, "shard step: the MultiHashTable has a touched-key set attached; the "
                                         "id-sharded step does not record on the owner yet");
    s->ss.init(t, max_batch_per_table, rank, world, ids_per_peer_table, unique_id);
    t->shard_steps.push_back(s.get());
    s->counted = true;
    *out = s.release();
  });
}
void mhte_shard_step_destroy(mhte_shard_step* s) {
  if (s) {
    std::lock_guard<std::mutex> link(g_touched_link_mu);
    if (s->counted) {
      auto& v = s->ss.mt->shard_steps;
      v.erase(std::remove(v.begin(), v.end(), s), v.end());
    }
  }
  delete s;
}

mhte_status mhte_shard_step_create_ipc(mhte_multi_table* t, int64_t max_batch_per_table, int32_t rank,
                                       int32_t world, int64_t ids_per_peer_table,
                                       mhte_shard_step** out) {
  return guard([&] {
    check_handle(t);
    if (!out) throw Error(MHTE_INVALID_ARGUMENT, "null out");
    HIP_OK(hipSetDevice(t->device));
    std::lock_guard<std::mutex> link(g_touched_link_mu);   // (before the tables', as everywhere)
    std::vector<std::unique_lock<std::mutex>> locks;
    for (auto& tb : t->tables) locks.emplace_back(tb->mu);
    std::unique_ptr<mhte_shard_step> s(new mhte_shard_step);
    if (t->touched)
      throw Error(MHTE_INVALID_ARGUMENT, "shard step: the MultiHashTable has a touched-key set attached; the "
                                         "id-sharded step does not record on the owner yet");
    s->ss.init(t, max_batch_per_table, rank, world, ids_per_peer_table, nullptr, true);
    t->shard_steps.push_back(s.get());
    s->counted = true;
    *out = s.release();
  });
}

mhte_status mhte_shard_step_ipc_handle(mhte_shard_step* s, void* out128) {
  return guard([&] {
    if (!s || !out128) throw Error(MHTE_INVALID_ARGUMENT, "null argument");
    HIP_OK(hipSetDevice(s->ss.device));
    s->ss.ipc_handle(out128);
  });
}

mhte_status mhte_shard_step_ipc_connect(mhte_shard_step* s, const void* handles, int32_t n_handles) {
  return guard([&] {
    if (!s || !handles) throw Error(MHTE_INVALID_ARGUMENT, "null argument");
    if (n_handles != s->ss.world)
      throw Error(MHTE_INVALID_ARGUMENT, "shard step connect: one handle per rank of the world");
    HIP_OK(hipSetDevice(s->ss.device));
    s->ss.ipc_connect(handles);
  });
}

mhte_status mhte_shard_step_ipc_selftest(mhte_shard_step* s, void* stream) {
  return guard([&] {
    if (!s) throw Error(MHTE_INVALID_ARGUMENT, "null shard step");
    HIP_OK(hipSetDevice(s->ss.device));
    s->ss.ipc_selftest(mhte::S(stream));
  });
}

mhte_status mhte_shard_step_forward(mhte_shard_step* s, const int64_t* id, const int64_t* id_split,
                                    int64_t n_split, float* embedding, int64_t embedding_len,
                                    const int64_t* id_next, const int64_t* id_split_next,
                                    int64_t n_split_next, int32_t prefetched, void* stream) {
  return guard([&] {
    if (!s) throw Error(MHTE_INVALID_ARGUMENT, "null shard step");
    HIP_OK(hipSetDevice(s->ss.device));
    auto locks = lock_tables(&s, 1);
    ShardFwd a;
    a.id = id;
    a.split = id_split;
    a.emb = embedding;
    a.emb_len = embedding_len;
    a.id_next = id_next;
    a.split_next = id_split_next;
    ShardStep* S = &s->ss;
    shard_forward(&S, 1, &a, n_split, n_split_next, prefetched, mhte::S(stream));
  });
}

mhte_status mhte_shard_step_backward(mhte_shard_step* s, const float* value, int64_t value_len,
                                     const float* learning_rate, int64_t n_learning_rate,
                                     int64_t update_time, int64_t global_step, void* stream) {
  return guard([&] {
    if (!s) throw Error(MHTE_INVALID_ARGUMENT, "null shard step");
    HIP_OK(hipSetDevice(s->ss.device));
    auto locks = lock_tables(&s, 1);
    ShardStep* S = &s->ss;
    shard_backward(&S, 1, &value, &value_len, learning_rate, n_learning_rate, update_time, global_step,
                   mhte::S(stream));
  });
}

mhte_status mhte_shard_step_set_overlap(mhte_shard_step* s, int32_t mode) {
  return guard([&] {
    if (!s) throw Error(MHTE_INVALID_ARGUMENT, "null shard step");
    HIP_OK(hipSetDevice(s->ss.device));
    auto locks = lock_tables(&s, 1);
    if (s->ss.aux_pending) HIP_OK(hipStreamSynchronize(s->ss.aux));
    s->ss.set_overlap(mode);
  });
}

mhte_status mhte_shard_step_set_grad_bits(mhte_shard_step* s, int32_t bits) {
  return guard([&] {
    if (!s) throw Error(MHTE_INVALID_ARGUMENT, "null shard step");
    HIP_OK(hipSetDevice(s->ss.device));
    auto locks = lock_tables(&s, 1);
    HIP_OK(hipDeviceSynchronize());
    s->ss.set_grad_bits(bits);
  });
}

mhte_status mhte_shard_step_set_exact_order(mhte_shard_step* s, int32_t on) {
  return guard([&] {
    if (!s) throw Error(MHTE_INVALID_ARGUMENT, "null shard step");
    auto locks = lock_tables(&s, 1);
    s->ss.exact_order = on != 0;
  });
}

mhte_status mhte_shard_step_check(mhte_shard_step* s, void* stream) {
  return guard([&] {
    if (!s) throw Error(MHTE_INVALID_ARGUMENT, "null shard step");
    HIP_OK(hipSetDevice(s->ss.device));
    s->ss.flush_slow(mhte::S(stream));
    HIP_OK(hipStreamSynchronize(mhte::S(stream)));
    if (s->ss.aux) HIP_OK(hipStreamSynchronize(s->ss.aux));
    s->ss.check_flags();
  });
}

mhte_status mhte_shard_step_unique_counts(mhte_shard_step* s, int64_t* counts, void* stream) {
  return guard([&] {
    if (!s || !counts) throw Error(MHTE_INVALID_ARGUMENT, "null argument");
    MultiStep& ms = s->ss.ms;
    HIP_OK(hipSetDevice(ms.device));
    if (ms.stage[ms.cur] != 2)
      throw Error(MHTE_FAILED_PRECONDITION, "shard step: the current batch has not been numbered");
    std::vector<uint32_t> h(ms.T, 0);
    for (uint32_t t = 0; t < ms.T; ++t)
      if (ms.n_slot[ms.cur][t])
        HIP_OK(hipMemcpyAsync(&h[t], ms.h_st[t].rv[ms.cur].n_unique, sizeof(uint32_t),
                              hipMemcpyDeviceToHost, mhte::S(stream)));
    HIP_OK(hipStreamSynchronize(mhte::S(stream)));
    for (uint32_t t = 0; t < ms.T; ++t) counts[t] = h[t];
  });
}

mhte_status mhte_shard_step_info(mhte_shard_step* s, int64_t info[4]) {
  return guard([&] {
    if (!s || !info) throw Error(MHTE_INVALID_ARGUMENT, "null argument");
    info[0] = s->ss.cap;
    info[1] = int64_t(s->ss.x_block(kXIds));
    info[2] = int64_t(s->ss.x_block(kXRows));
    info[3] = s->ss.alias ? 0 : s->ss.ipc ? (s->ss.win_fine ? 3 : 4) : (s->ss.comm ? 1 : 2);
  });
}

mhte_status mhte_shard_step_launches(mhte_shard_step* s, int32_t out[2]) {
  return guard([&] {
    if (!s || !out) throw Error(MHTE_INVALID_ARGUMENT, "null argument");
    out[0] = int32_t(s->ss.launches_fwd);
    out[1] = int32_t(s->ss.launches - s->ss.launches_fwd);
  });
}

mhte_status mhte_shard_step_apply_launches(mhte_shard_step* s, int64_t out[12]) {
  return guard([&] {
    if (!s || !out) throw Error(MHTE_INVALID_ARGUMENT, "null argument");
    for (int i = 0; i < 12; ++i) out[i] = int64_t(s->ss.apply_launches[i]);
  });
}

mhte_status mhte_shard_step_wire_stats(mhte_shard_step* s, int64_t out[4]) {
  return guard([&] {
    if (!s || !out) throw Error(MHTE_INVALID_ARGUMENT, "null argument");
    out[0] = int64_t(s->ss.wire_pairs);
    out[1] = int64_t(s->ss.wire_exchanges);
    out[2] = int64_t(s->ss.wire_pairs_max);
    out[3] = int64_t(s->ss.host_waits);
  });
}

mhte_status mhte_shard_step_comm_ranks(mhte_shard_step* s, int32_t out[2]) {
  return guard([&] {
    if (!s || !out) throw Error(MHTE_INVALID_ARGUMENT, "null argument");
    out[0] = out[1] = 0;
    if (!s->ss.comm) return;   // (identity / peer stores / in-process group: no communicator)
    Rccl& R = Rccl::get();
    if (!R.CommCount || !R.CommUserRank) throw Error(MHTE_UNAVAILABLE, "this RCCL exports no ncclCommCount");
    int n = 0, r = 0;
    R.ok(R.CommCount(s->ss.comm, &n), "CommCount");
    R.ok(R.CommUserRank(s->ss.comm, &r), "CommUserRank");
    out[0] = n;
    out[1] = r;
  });
}

mhte_status mhte_shard_group_forward(mhte_shard_step** steps, int32_t n, const int64_t* const* id,
                                     const int64_t* const* id_split, int64_t n_split,
                                     float* const* embedding, const int64_t* embedding_len,
                                     const int64_t* const* id_next,
                                     const int64_t* const* id_split_next, int64_t n_split_next,
                                     int32_t prefetched, void* stream) {
  return guard([&] {
    if (!steps || n < 1 || n > kMaxShards || !id || !id_split || !embedding || !embedding_len)
      throw Error(MHTE_INVALID_ARGUMENT, "shard group forward: bad arguments");
    for (int32_t r = 0; r < n; ++r)
      if (!steps[r]) throw Error(MHTE_INVALID_ARGUMENT, "null shard step");
    auto locks = lock_tables(steps, n);
    std::vector<ShardStep*> S(size_t(n), nullptr);
    std::vector<ShardFwd> a(size_t(n), ShardFwd{});
    for (int32_t r = 0; r < n; ++r) {
      S[size_t(r)] = &steps[r]->ss;
      a[size_t(r)].id = id[r];
      a[size_t(r)].split = id_split[r];
      a[size_t(r)].emb = embedding[r];
      a[size_t(r)].emb_len = embedding_len[r];
      a[size_t(r)].id_next = id_next ? id_next[r] : nullptr;
      a[size_t(r)].split_next = id_split_next ? id_split_next[r] : nullptr;
    }
    shard_forward(S.data(), n, a.data(), n_split, n_split_next, prefetched, mhte::S(stream));
  });
}

mhte_status mhte_shard_group_backward(mhte_shard_step** steps, int32_t n, const float* const* value,
                                      const int64_t* value_len, const float* learning_rate,
                                      int64_t n_learning_rate, int64_t update_time,
                                      int64_t global_step, void* stream) {
  return guard([&] {
    if (!steps || n < 1 || n > kMaxShards || !value || !value_len)
      throw Error(MHTE_INVALID_ARGUMENT, "shard group backward: bad arguments");
    for (int32_t r = 0; r < n; ++r)
      if (!steps[r]) throw Error(MHTE_INVALID_ARGUMENT, "null shard step");
    auto locks = lock_tables(steps, n);
    std::vector<ShardStep*> S(size_t(n), nullptr);
    for (int32_t r = 0; r < n; ++r) S[size_t(r)] = &steps[r]->ss;
    shard_backward(S.data(), n, value, value_len, learning_rate, n_learning_rate, update_time,
                   global_step, mhte::S(stream));
  });
}

mhte_status mhte_profile_arm(int32_t n) {
  return guard([&] {
    if (n < 0 || n > 65536) throw Error(MHTE_INVALID_ARGUMENT, "profile_arm: n out of range");
    for (hipEvent_t e : g_prof.ev) (void)hipEventDestroy(e);
    g_prof.ev.clear();
    g_prof.tag.clear();
    g_prof.armed = 0;
    g_prof.ev.resize(size_t(2 * n), nullptr);
    for (auto& e : g_prof.ev) HIP_OK(hipEventCreate(&e));
    g_prof.tag.reserve(size_t(n));
    g_prof.armed = n;
  });
}

mhte_status mhte_profile_read(int32_t cap, int32_t* kernel_tag, float* usec, int32_t* n_out) {
  return guard([&] {
    if (!n_out) throw Error(MHTE_INVALID_ARGUMENT, "profile_read: null n_out");
    g_prof.armed = 0;
    const int32_t n = int32_t(g_prof.tag.size());
    *n_out = n;
    for (int32_t i = 0; i < n && i < cap; ++i) {
      HIP_OK(hipEventSynchronize(g_prof.ev[2 * i + 1]));
      float ms = 0.f;
      HIP_OK(hipEventElapsedTime(&ms, g_prof.ev[2 * i], g_prof.ev[2 * i + 1]));
      if (kernel_tag) kernel_tag[i] = g_prof.tag[i];
      if (usec) usec[i] = ms * 1e3f;
    }
  });
}

// ---- dense tower (mhte_gemm_host.h)
mhte_status mhte_dense_mlp_create(const int32_t* widths, int32_t n_widths, int64_t max_batch,
                                  int32_t gpu_ordinal, mhte_dense_mlp** out) {
  return guard([&] {
    if (!widths || !out) throw Error(MHTE_INVALID_ARGUMENT, "dense mlp: null argument");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || gpu_ordinal < 0 || gpu_ordinal >= ndev)
      throw Error(MHTE_UNAVAILABLE, "no such HIP device");
    HIP_OK(hipSetDevice(gpu_ordinal));
    std::unique_ptr<mhte_dense_mlp> m(new mhte_dense_mlp);
    m->m.create(widths, n_widths, max_batch, gpu_ordinal);
    *out = m.release();
  });
}
void mhte_dense_mlp_destroy(mhte_dense_mlp* m) {
  if (!m) return;
  (void)hipSetDevice(m->m.device);
  (void)hipDeviceSynchronize();
  delete m;
}
mhte_status mhte_dense_mlp_set_params(mhte_dense_mlp* m, int32_t layer, const float* weight,
                                      const float* bias, void* stream) {
  return guard([&] {
    if (!m || !weight || !bias) throw Error(MHTE_INVALID_ARGUMENT, "dense mlp: null argument");
    HIP_OK(hipSetDevice(m->m.device));
    m->m.set_params(layer, weight, bias, S(stream));
  });
}
mhte_status mhte_dense_mlp_get_params(mhte_dense_mlp* m, int32_t layer, float* weight, float* bias,
                                      void* stream) {
  return guard([&] {
    if (!m || !weight || !bias) throw Error(MHTE_INVALID_ARGUMENT, "dense mlp: null argument");
    HIP_OK(hipSetDevice(m->m.device));
    m->m.get_params(layer, weight, bias, S(stream));
  });
}
mhte_status mhte_dense_mlp_forward(mhte_dense_mlp* m, const float* x, int64_t batch, float* y,
                                   void* stream) {
  return guard([&] {
    if (!m || !x || !y) throw Error(MHTE_INVALID_ARGUMENT, "dense mlp: null argument");
    HIP_OK(hipSetDevice(m->m.device));
    m->m.forward(x, batch, y, S(stream));
  });
}
mhte_status mhte_dense_mlp_backward(mhte_dense_mlp* m, const float* dy, float* dx,
                                    float learning_rate, void* stream) {
  return guard([&] {
    if (!m || !dy) throw Error(MHTE_INVALID_ARGUMENT, "dense mlp: null argument");
    HIP_OK(hipSetDevice(m->m.device));
    m->m.backward(dy, dx, learning_rate, S(stream));
  });
}
mhte_status mhte_dense_mlp_backward_grads(mhte_dense_mlp* m, const float* dy, float* dx,
                                          float* const* weight_grads, float* const* bias_grads, void* stream) {
  return guard([&] {
    DenseMlp::check_ptr("dense_mlp_backward_grads", "m", m, true);
    DenseMlp::check_ptr("dense_mlp_backward_grads", "dy", dy, true);
    DenseMlp::check_ptr("dense_mlp_backward_grads", "dx", dx, false);
    m->m.check_grads_call(weight_grads, bias_grads);
    HIP_OK(hipSetDevice(m->m.device));
    m->m.backward_grads(dy, dx, weight_grads, bias_grads, S(stream));
  });
}
mhte_status mhte_dense_mlp_load_params(mhte_dense_mlp* m, const float* const* weights,
                                       const float* const* biases, void* stream) {
  return guard([&] {
    DenseMlp::check_ptr("dense_mlp_load_params", "m", m, true);
    m->m.check_load_call(weights, biases);
    HIP_OK(hipSetDevice(m->m.device));
    m->m.load_params(weights, biases, S(stream));
  });
}
mhte_status mhte_dense_mlp_launch_counts(mhte_dense_mlp* m, int64_t out[8]) {
  return guard([&] {
    if (!m || !out) throw Error(MHTE_INVALID_ARGUMENT, "dense mlp: null argument");
    for (int r = 0; r < 4; ++r)
      for (int t = 0; t < 2; ++t) out[2 * r + t] = m->m.launches[r][t];
  });
}

mhte_status mhte_trace_begin(void* dev_buf, int64_t cap_records) {
  return guard([&] {
    g_trace.buf = static_cast<unsigned long long*>(dev_buf);
    g_trace.cap = dev_buf ? cap_records : 0;
    g_trace.cursor = 0;
    g_trace.launches.clear();
  });
}

mhte_status mhte_trace_end(int32_t cap, int32_t* kernel_tag, int32_t* grid, int32_t* block,
                           int64_t* offset, int32_t* n_out) {
  return guard([&] {
    if (!n_out) throw Error(MHTE_INVALID_ARGUMENT, "trace_end: null n_out");
    g_trace.buf = nullptr;
    const int32_t n = int32_t(g_trace.launches.size());
    *n_out = n;
    for (int32_t i = 0; i < n && i < cap; ++i) {
      const TraceLaunch& l = g_trace.launches[size_t(i)];
      if (kernel_tag) kernel_tag[i] = l.tag;
      if (grid) grid[i] = l.grid;
      if (block) block[i] = l.block;
      if (offset) offset[i] = l.offset;
    }
  });
}

}  // extern "C"
