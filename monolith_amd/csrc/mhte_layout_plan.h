// Host plan of fused_embedding_to_layout (mhte_layout_host.h executes it, mhte_layout_kernels.h are the kernels):
// the checks of a call and every decision the host takes for it — pointer tables or inline arguments, which
// outputs the zero fill may skip, the gradient's copy form, the grouped gradient's task lists, and the launches
// with their forms.  Plain host C++, no HIP and no getenv: compiled by hipcc inside mhte.hip and, alone, by
// tests/layout_plan_host_driver.cc (g++, also under the sanitizers).
#ifndef MHTE_LAYOUT_PLAN_H_
#define MHTE_LAYOUT_PLAN_H_

#include <stdint.h>

#include <algorithm>
#include <string>
#include <utility>
#include <vector>

#include "../../include/monolith_amd_hash_table.h"

namespace mhte {

constexpr int kMaxLayoutTasks = 48;   // slices per launch (more: several launches)
constexpr int kMaxLayoutEmb = 64;     // embedding matrices (shard x sub-table) carried in the kernel
constexpr int kMaxLayoutOut = 32;     // arguments, output tensors likewise; more (the reference's own
                                      // test has ~1000 and 153): pointer tables in device memory
constexpr int kLayoutRowsR = 16;        // batch rows per workgroup of layout_rows_kernel
constexpr int kLayoutRowsMaxF = 2048;   // float4 columns of one batch row over the launch's slices

enum LayoutPooling : int32_t { kPoolSum = 0, kPoolMean = 1, kPoolFirstN = 3 };  // example.proto:176-180
constexpr int32_t kPoolZeroFill = 100;   // (internal) a run of output columns no slice writes: layout_rows_kernel zeroes it
constexpr int32_t kLayoutAddn = 2;       // mhte_layout_slice.out_type of an ADDN layout

struct LayoutTask {
  int32_t nfl_idx;       // SliceConfig.feature_idx
  int32_t start, dim;    // slice [start, start + dim) of the feature's embedding
  int32_t pooling;
  int32_t max_seq;       // FIRSTN: rows kept
  int32_t out_index;     // which output tensor
  int32_t out_offset;    // float offset of the slice inside an output row
  int32_t out_stride;    // floats per output row
};
struct LayoutUnit {
  uint16_t first, count; // tasks [first, first + count); count > 1 only for an ADDN layout
  uint16_t addn, pad;    // addn: 1 an ADDN layout, 2 its continuation in a following launch
};

// The call as the plan sees it.  The pointers behind `embeddings` / `outputs` are read for their 16-byte
// alignment only (forward: matrices and output tensors; gradient: gradient buffers and output gradients).
struct LayoutCall {
  bool forward;
  const int32_t* emb_stride;
  const int64_t* emb_count;
  int32_t n_emb;
  const void* const* embeddings;
  const void* const* outputs;
  int64_t n_fid, n_feature;
  int32_t n_nfl, batch;
  const mhte_layout_slice* slices;
  int32_t n_slices;
  const int64_t* output_len;
  int32_t n_outputs, flags;
  bool rows_form, pool_atomics;   // MHTE_LAYOUT_ROWS != 0, MHTE_POOL_ATOMICS=1
};

enum LayoutForm : int32_t { kLayoutFormRows = 0, kLayoutFormCopy = 1, kLayoutFormGeneral = 2 };

struct LayoutLaunch {
  LayoutForm form;
  int32_t n_tasks, n_units;
  int32_t zero_missing;   // LayoutArgs.zero_missing; != 0 (and zero runs among the tasks) only with form rows
  LayoutTask task[kMaxLayoutTasks];
  LayoutUnit unit[kMaxLayoutTasks];
};

struct LayoutPlan {
  bool ext = false;              // pointer tables in device memory (the fill then runs over every buffer)
  std::vector<char> skip_fill;   // [n_outputs], forward without ext: 1 = a rows launch writes every float
  bool grouped = false;          // the gradient without float atomics: the three lists below, no launches
  std::vector<LayoutTask> tasks;       // [n_slices]
  std::vector<uint32_t> t_off, t_idx;  // [n_nfl + 1] / slices by feature, in configuration order
  std::vector<LayoutLaunch> launches;  // in stream order; empty: the fill is all the call does
};

static inline bool layout_aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }
static inline bool layout_one_fid(const LayoutCall& c) {
  return (c.flags & MHTE_LAYOUT_ONE_FID_UNIQUE_ROWS) != 0 && c.n_fid == c.n_feature;
}
static inline bool layout_matrices_aligned(const LayoutCall& c) {
  for (int32_t i = 0; i < c.n_emb; ++i)
    if ((c.emb_stride[i] & 3) != 0 || !layout_aligned16(c.embeddings[i])) return false;
  return true;
}
// floats of an output row a slice writes from out_offset on
static inline int64_t layout_width(int32_t dim, int32_t pooling, int32_t max_seq) {
  return int64_t(dim) * (pooling == kPoolFirstN ? std::max(1, max_seq) : 1);
}
static inline LayoutTask layout_task_of(const mhte_layout_slice& sc) {
  return LayoutTask{sc.feature_idx, sc.start, sc.dim, sc.pooling, sc.max_sequence_length,
                    sc.out_index, sc.out_offset, sc.out_row_floats};
}
// slice i continues the ADDN layout slice i - 1 belongs to
static inline bool layout_same_addn(const mhte_layout_slice* s, int32_t i) {
  return i > 0 && s[i].out_type == kLayoutAddn && s[i - 1].out_type == kLayoutAddn &&
         s[i].out_index == s[i - 1].out_index;
}

// ---- the checks: "" or the message of the InvalidArgument error.  A call that moves nothing (no batch rows or
// no slices) only fills, and its slices are not looked at.
static inline std::string layout_check(const LayoutCall& c) {
  if (c.n_emb < 0 || c.n_outputs < 0 || c.n_emb > (1 << 20) || c.n_outputs > (1 << 20))
    return "layout: bad matrix / output count";
  if (c.batch < 0 || c.n_slices < 0 || c.n_fid > INT32_MAX || c.n_feature > INT32_MAX) return "layout: bad sizes";
  if (c.batch == 0) return "";
  for (int32_t i = 0, first = 0; i < c.n_slices; ++i) {
    const mhte_layout_slice& sc = c.slices[i];
    if (!layout_same_addn(c.slices, i)) first = i;   // (the first slice of the whole ADDN layout)
    if (sc.out_index < 0 || sc.out_index >= c.n_outputs || sc.dim <= 0 || sc.out_row_floats <= 0 ||
        int64_t(sc.out_offset) + layout_width(sc.dim, sc.pooling, sc.max_sequence_length) > sc.out_row_floats ||
        int64_t(c.batch) * sc.out_row_floats > c.output_len[sc.out_index])
      return "layout: slice " + std::to_string(i) + " does not fit its output";
    if (sc.out_type == kLayoutAddn && sc.pooling == kPoolFirstN)   // CHECK in the op's constructor
      return "layout: FIRSTN pooling cannot be added (ADDN)";
    if (sc.out_type == kLayoutAddn && sc.dim != c.slices[first].dim)
      return "layout: slices of an ADDN layout differ in width";
  }
  return "";
}

// ---- decision 1, forward: do the slices of an output (plus zero runs for the columns between and behind them)
// write every float of it?  Then layout_rows_kernel writes the zeros too and the fill in front of it — a pass over
// the whole output: 268 MB at configs[4]'s shape — is left out for that output.  Holds for calls whose slices fit
// one launch in the rows form; fills P.skip_fill and returns the zero runs, which every launch of the call carries.
static inline LayoutTask layout_zero_run(int32_t out, int32_t offset, int32_t end, int32_t stride) {
  return LayoutTask{/*nfl_idx*/ -2, /*start*/ 0, /*dim*/ end - offset, kPoolZeroFill, /*max_seq*/ 0, out, offset, stride};
}
// the zero runs that complete output o's rows, or false: its slices do not tile a [batch, stride] tensor
static inline bool layout_output_gaps(const LayoutCall& c, int32_t o, int32_t stride, std::vector<LayoutTask>& gaps) {
  if (stride == 0 || c.output_len[o] != int64_t(c.batch) * stride) return false;   // (rows beyond the batch: the fill stays)
  std::vector<std::pair<int32_t, int32_t>> runs;   // (offset, width) of the slices of output o
  for (int32_t i = 0; i < c.n_slices; ++i)
    if (c.slices[i].out_index == o) runs.emplace_back(c.slices[i].out_offset, c.slices[i].dim);
  std::sort(runs.begin(), runs.end());
  int32_t pos = 0;
  for (auto& r : runs) {
    if (r.first < pos) return false;   // overlapping slices: the fill stays
    if (r.first > pos) gaps.push_back(layout_zero_run(o, pos, r.first, stride));
    pos = r.first + r.second;
  }
  if (pos < stride) gaps.push_back(layout_zero_run(o, pos, stride, stride));
  return true;
}
static inline std::vector<LayoutTask> layout_whole_rows(const LayoutCall& c, LayoutPlan& P) {
  std::vector<LayoutTask> zero_runs;
  if (!c.forward || P.ext || !c.rows_form || !layout_one_fid(c) || c.n_slices > kMaxLayoutTasks) return zero_runs;
  int64_t cols = 0;
  std::vector<int32_t> stride(size_t(c.n_outputs), 0);   // floats per row of an output, 0: no slice names it
  for (int32_t i = 0; i < c.n_slices; ++i) {
    const mhte_layout_slice& sc = c.slices[i];
    if (sc.out_type == kLayoutAddn || sc.pooling == kPoolFirstN || sc.start < 0 || sc.out_offset < 0 ||
        ((sc.start | sc.dim | sc.out_offset | sc.out_row_floats) & 3) != 0 || !layout_aligned16(c.outputs[sc.out_index]))
      return zero_runs;
    int32_t& st = stride[size_t(sc.out_index)];
    if (st && st != sc.out_row_floats) return zero_runs;   // (two row widths in one output)
    st = sc.out_row_floats;
    cols += sc.dim / 4;
  }
  if (cols > kLayoutRowsMaxF || !layout_matrices_aligned(c)) return zero_runs;
  std::vector<char> covered(size_t(c.n_outputs), 0);
  for (int32_t o = 0; o < c.n_outputs; ++o) {
    std::vector<LayoutTask> gaps;
    const bool tiles = layout_output_gaps(c, o, stride[size_t(o)], gaps);
    int64_t gcols = 0;
    for (auto& z : gaps) gcols += z.dim / 4;
    if (!tiles || size_t(c.n_slices) + zero_runs.size() + gaps.size() > size_t(kMaxLayoutTasks) ||
        cols + gcols > kLayoutRowsMaxF)
      continue;
    cols += gcols;
    zero_runs.insert(zero_runs.end(), gaps.begin(), gaps.end());
    covered[size_t(o)] = 1;
  }
  P.skip_fill = covered;
  return zero_runs;
}

// ---- decision 2: the copy form (float4 copies; the gradient a plain store).  The flag's plain stores hold only
// while no element of a feature's row is named by two slices (the same columns of one feature in a CONCAT and in a
// STACK layout, say): there the gradient is a sum of two addends, and the call takes the form it would take
// without the flag.  The forward only reads.
static inline bool layout_copy_form(const LayoutCall& c) {
  if (!layout_one_fid(c)) return false;
  if (c.forward) return true;
  const mhte_layout_slice* s = c.slices;
  std::vector<int32_t> order(size_t(c.n_slices));   // slices by feature, then start
  for (int32_t i = 0; i < c.n_slices; ++i) order[size_t(i)] = i;
  std::sort(order.begin(), order.end(), [s](int32_t a, int32_t b) {
    if (s[a].feature_idx != s[b].feature_idx) return s[a].feature_idx < s[b].feature_idx;
    return s[a].start != s[b].start ? s[a].start < s[b].start : a < b;
  });
  int64_t end = 0;   // one past the last column a slice of the current feature has named so far
  for (size_t i = 0; i < order.size(); ++i) {
    const mhte_layout_slice& sc = s[order[i]];
    if (i == 0 || sc.feature_idx != s[order[i - 1]].feature_idx) end = INT64_MIN;
    if (int64_t(sc.start) < end) return false;
    end = std::max(end, int64_t(sc.start) + sc.dim);
  }
  return true;
}

// ---- decision 3: the grouped (atomic-free) gradient's tasks and, per named feature list, the slices that read it
static inline void layout_group_tasks(const LayoutCall& c, LayoutPlan& P) {
  const auto named = [&c](int32_t i) { return c.slices[i].feature_idx >= 0 && c.slices[i].feature_idx < c.n_nfl; };
  P.grouped = true;
  P.tasks.resize(size_t(c.n_slices));
  P.t_off.assign(size_t(c.n_nfl) + 1, 0);
  for (int32_t i = 0; i < c.n_slices; ++i) {
    P.tasks[size_t(i)] = layout_task_of(c.slices[i]);
    if (named(i)) ++P.t_off[size_t(c.slices[i].feature_idx) + 1];
  }
  for (int32_t f = 0; f < c.n_nfl; ++f) P.t_off[size_t(f) + 1] += P.t_off[size_t(f)];
  P.t_idx.resize(P.t_off[size_t(c.n_nfl)]);
  std::vector<uint32_t> cur(P.t_off.begin(), P.t_off.end() - 1);
  for (int32_t i = 0; i < c.n_slices; ++i)
    if (named(i)) P.t_idx[cur[size_t(c.slices[i].feature_idx)]++] = uint32_t(i);
}

// ---- decision 4: the launches.  One launch per kMaxLayoutTasks slices.  An ADDN layout's slices are added in
// configuration order by one lane group; a layout with more slices than a launch holds continues in the next
// launch, which starts from the sums the previous one stored (same order, same roundings).
//
// (forward) a slice that writes floats an earlier slice of this launch writes too starts the next launch: launches
// run in stream order, so the later slice's values stay, as in the op's own loop (inside one launch the two stores
// come from different lanes or workgroups, in no order)
static inline bool layout_clashes(const LayoutLaunch& L, const mhte_layout_slice& sc) {
  const int64_t w1 = layout_width(sc.dim, sc.pooling, sc.max_sequence_length);
  for (int32_t q = 0; q < L.n_tasks; ++q) {
    const LayoutTask& t = L.task[q];
    if (t.out_index != sc.out_index) continue;
    if (t.out_stride != sc.out_row_floats || (int64_t(sc.out_offset) < t.out_offset + layout_width(t.dim, t.pooling, t.max_seq) &&
                                              int64_t(t.out_offset) < sc.out_offset + w1))
      return true;
  }
  return false;
}
// the next `count` tasks of the launch, already written behind its last one, become a unit
static inline void layout_add_unit(LayoutLaunch& L, int32_t count, int32_t addn) {
  L.unit[L.n_units++] = LayoutUnit{uint16_t(L.n_tasks), uint16_t(count), uint16_t(addn), 0};
  L.n_tasks += count;
}
// One fid per feature instance (asserted by the caller) and float4-aligned copies: the vector copy form, plain
// stores for the gradient; a workgroup per 16 batch rows over all slices of the launch (rows) when a row's float4
// columns fit the kernel's column table, else a lane group per (slice, row) (copy).
static inline LayoutForm layout_form_of(const LayoutCall& c, const LayoutLaunch& L, bool copy_form) {
  bool fast = copy_form;
  int64_t cols = 0;
  for (int32_t q = 0; fast && q < L.n_tasks; ++q) {
    const LayoutTask& t = L.task[q];
    fast = t.pooling != kPoolFirstN && ((t.start | t.dim | t.out_offset | t.out_stride) & 3) == 0 &&
           layout_aligned16(c.outputs[t.out_index]);
  }
  for (int32_t q = 0; q < L.n_units; ++q) {
    fast = fast && L.unit[q].count == 1;
    cols += L.task[L.unit[q].first].dim / 4;
  }
  if (!fast || !layout_matrices_aligned(c)) return kLayoutFormGeneral;
  return c.rows_form && cols > 0 && cols <= kLayoutRowsMaxF ? kLayoutFormRows : kLayoutFormCopy;
}
static inline void layout_pack(const LayoutCall& c, bool copy_form, const std::vector<LayoutTask>& zero_runs,
                               LayoutPlan& P) {
  uint32_t mask = 0;   // one bit per output written whole (decided without pointer tables: <= kMaxLayoutOut outputs)
  for (size_t o = 0; o < P.skip_fill.size() && o < 32; ++o)
    if (P.skip_fill[o]) mask |= 1u << o;
  int32_t k = 0;
  bool addn_open = false;   // the previous launch ended inside an ADDN layout: its next slices add on
  while (k < c.n_slices) {
    P.launches.emplace_back();
    LayoutLaunch& L = P.launches.back();
    L.n_tasks = L.n_units = 0;
    while (k < c.n_slices) {
      int32_t span = 1;
      while (k + span < c.n_slices && layout_same_addn(c.slices, k + span)) ++span;
      const bool cont = addn_open;
      if (c.forward && layout_clashes(L, c.slices[k])) break;
      if (span > kMaxLayoutTasks) {
        if (L.n_tasks > 0) break;   // (a long ADDN layout starts its own launch)
        span = kMaxLayoutTasks;
        addn_open = true;
      } else {
        if (L.n_tasks + span > kMaxLayoutTasks) break;
        addn_open = false;
      }
      for (int32_t q = 0; q < span; ++q) L.task[L.n_tasks + q] = layout_task_of(c.slices[k + q]);
      layout_add_unit(L, span, c.slices[k].out_type == kLayoutAddn ? (cont ? 2 : 1) : 0);
      k += span;
    }
    // (the zero runs of outputs the call writes in full: slices like any other)
    for (auto& z : zero_runs) {
      L.task[L.n_tasks] = z;
      layout_add_unit(L, 1, 0);
    }
    L.zero_missing = int32_t(mask);
    L.form = layout_form_of(c, L, copy_form);
  }
}

// The whole plan: "" or the message of the InvalidArgument error (then P is not to be used).
static inline std::string layout_plan(const LayoutCall& c, LayoutPlan& P) {
  const std::string bad = layout_check(c);
  if (!bad.empty()) return bad;
  // Few matrices and outputs (a model's tables: the training path) travel in the kernel arguments.  More of them
  // (one matrix per (table, shard, feature) as the reference's parameter-server path hands them over: ~1000 in its
  // own test) go through pointer tables uploaded for the call.
  P.ext = c.n_emb > kMaxLayoutEmb || c.n_outputs > kMaxLayoutOut;
  P.skip_fill.assign(size_t(c.n_outputs), 0);
  if (c.batch == 0 || c.n_slices == 0) return "";
  const std::vector<LayoutTask> zero_runs = layout_whole_rows(c, P);
  const bool copy_form = layout_copy_form(c);
  if (!c.forward && !copy_form && !c.pool_atomics && c.n_fid > 0) layout_group_tasks(c, P);
  else layout_pack(c, copy_form, zero_runs, P);
  return "";
}

}  // namespace mhte
#endif  // MHTE_LAYOUT_PLAN_H_
