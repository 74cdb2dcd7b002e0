// Host side of the touched-key set (mhte_touched_kernels.h): the resource, the insert call and the
// recording hook of the update entry points.  Included by mhte.hip.
#ifndef MHTE_TOUCHED_HOST_H_
#define MHTE_TOUCHED_HOST_H_

#include "mhte_touched_kernels.h"

struct mhte_touched_key_set {
  int device = 0;
  int64_t capacity = 0;
  uint32_t call_limit = 0;          // positions per device call: min(max_insert, capacity + 1, kTkMaxPositions)
  mhte::TkView view{};
  // own mutex, taken AFTER the tables' (an update entry point holds its table's while it records)
  std::mutex mu;
  hipStream_t last_stream = nullptr;
  bool used = false;
  hipEvent_t ev = nullptr;          // orders consecutive calls that arrive on different streams
  mhte_multi_table* owner = nullptr;
  mhte::DevBuf<int32_t> keep;       // per-id "the table holds it" of a filtered table's op-level update
  ~mhte_touched_key_set() {
    (void)hipSetDevice(device);
    if (view.slots || view.ctl) (void)hipDeviceSynchronize();
    if (view.slots) (void)hipFree(view.slots);
    if (view.ctl) (void)hipFree(view.ctl);
    if (view.bitmap) (void)hipFree(view.bitmap);
    if (ev) (void)hipEventDestroy(ev);
  }
};

namespace mhte {

// attach / detach / destroy of either side
static std::mutex g_touched_link_mu;

// the caller holds set.mu
static void tk_enter_stream(mhte_touched_key_set& set, hipStream_t st) {
  if (set.used && set.last_stream != st) {
    HIP_OK(hipEventRecord(set.ev, set.last_stream));
    HIP_OK(hipStreamWaitEvent(st, set.ev, 0));
  }
  set.last_stream = st;
  set.used = true;
}

static void tk_launch_call(mhte_touched_key_set& set, const TkDescs& ds, hipStream_t st) {
  if (ds.total == 0 || ds.nseg == 0) return;
  const TkView v = set.view;
  const uint32_t nb = (ds.total + kTkBlock - 1) / kTkBlock;
  const uint32_t nclear = uint32_t(std::min<uint64_t>((uint64_t(v.mask) + 1u) / kTkBlock, 2048));
  tk_insert_kernel<<<nb, kTkBlock, 0, st>>>(v, ds);
  tk_mark_kernel<<<nb, kTkBlock, 0, st>>>(v, ds);
  tk_select_kernel<<<1, kTkSelectBlock, 0, st>>>(v, ds.total);
  tk_clear_kernel<<<nclear, kTkBlock, 0, st>>>(v, 0);
  tk_reinsert_kernel<<<nb, kTkBlock, 0, st>>>(v, ds);
  HIP_OK(hipGetLastError());
}

// Inserts the segments descs[0..n) in order.  dev: the same array on the device, or NULL (each segment
// then travels in the kernel arguments).  skip[s] != 0: segment s holds nothing in this call.  Segments
// are grouped into calls of at most call_limit positions; a longer segment is cut.  The caller holds
// set.mu and has entered the stream.
static void tk_insert_segments(mhte_touched_key_set& set, const TkDesc* descs, const TkDesc* dev, uint32_t n,
                               const uint8_t* skip, hipStream_t st) {
  const uint32_t limit = set.call_limit;
  uint32_t s = 0;
  while (s < n) {
    if (skip && skip[s]) {
      ++s;
      continue;
    }
    if (descs[s].n_max == 0) {
      ++s;
      continue;
    }
    if (descs[s].n_max > limit || !dev) {   // one segment per call, cut to the limit
      for (uint32_t off = 0; off < descs[s].n_max; off += limit) {
        TkDescs ds{};
        ds.dev = nullptr;
        ds.one = descs[s];
        ds.one.start = descs[s].start + off;
        ds.one.n_max = std::min<uint32_t>(limit, descs[s].n_max - off);
        ds.nseg = 1;
        ds.total = ds.one.n_max;
        tk_launch_call(set, ds, st);
      }
      ++s;
      continue;
    }
    TkDescs ds{};
    ds.dev = dev + s;
    uint32_t k = 0;
    uint64_t total = 0;
    while (s + k < n && k < 128 && descs[s + k].n_max <= limit && total + descs[s + k].n_max <= limit) {
      if (skip && skip[s + k]) ds.skip[k >> 6] |= 1ull << (k & 63);
      total += descs[s + k].n_max;
      ++k;
    }
    ds.nseg = k;
    ds.total = uint32_t(total);
    tk_launch_call(set, ds, st);
    s += k;
  }
}

// The recording hook of the op-level update entry points; the caller holds tb.mu.  ids [dev, n_max],
// n_dev [dev] or NULL.  With an admission filter on the table only the ids it holds now are recorded
// (ids_after_filter, tf_bridge.cc:236-251,312-336): the read-only probe, in stream order behind the update.
static void tk_record(mhte_multi_table* t, Table& tb, int32_t table, const int64_t* ids, int64_t n_max,
                      const uint32_t* n_dev, hipStream_t st) {
  mhte_touched_key_set* set = t->touched;
  if (!set || n_max <= 0) return;
  if (n_max > int64_t(0xffffffffu)) throw Error(MHTE_INVALID_ARGUMENT, "touched-key set: too many ids in one call");
  std::lock_guard<std::mutex> g(set->mu);
  tk_enter_stream(*set, st);
  TkDesc d{};
  d.ids = ids;
  d.n_dev = n_dev;
  d.n_max = uint32_t(n_max);
  d.tag = table;
  if (tb.flt_slots) {
    tb.finish_pending(st);
    set->keep.reserve(size_t(n_max));
    contains_kernel<<<dim3(uint32_t((n_max + 255) / 256)), 256, 0, st>>>(tb.view, ids, n_dev, n_max, set->keep.p);
    HIP_OK(hipGetLastError());
    d.keep = set->keep.p;
  }
  tk_insert_segments(*set, &d, nullptr, 1, nullptr, st);
}

static bool tk_any_filter(const mhte_multi_table* t) {
  for (auto& tb : t->tables)
    if (tb->flt_slots) return true;
  return false;
}

}  // namespace mhte

#endif  // MHTE_TOUCHED_HOST_H_
