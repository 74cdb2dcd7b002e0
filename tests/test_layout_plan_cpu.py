"""fused_embedding_to_layout: the host plan (csrc/mhte_layout_plan.h) without a device.

``mhte_embedding_to_layout(_grad)`` plans a call before it enqueues anything: the checks, pointer tables or
inline arguments, which outputs the zero fill skips, the grouped gradient or the list of launches with their
forms (rows, copy, general).  tests/layout_plan_host_driver.cc prints that plan; this module compares it

  * for every case of tests/test_layout_forms_gpu.py (the builders are shared: tests/layout_cases.py), in both
    directions, with the flag and without where that module uses both, with the sequence its comments promise;
  * at the edges of each decision, and for every error message;
  * once more under AddressSanitizer and UBSan (a stand-alone program: nothing is loaded into Python).

The expected sequences are written out here (``L(...)``: form, the slices of the launch by index, zero runs, mask),
derived by hand from the rules of the plan header's comments; only a task's eight numbers are copied from the
slice it stands for, and the grouped gradient's lists are restated by ``_lists``.
"""
import os
import subprocess

import numpy as np
import pytest

import layout_cases as LC
from monolith_amd import _lib
from monolith_amd.distribution_ops import _layout_plan

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIVER_SRC = os.path.join(ROOT, "tests", "layout_plan_host_driver.cc")
FLAG = _lib.MHTE_LAYOUT_ONE_FID_UNIQUE_ROWS
SUM, FIRSTN = 0, 3
CONCAT, ADDN, NONE = 0, 2, 3
ZERO_FILL = 100   # kPoolZeroFill


# ===================================================================== a call as the driver reads it
def sl(feature, start, dim, out_index, out_offset, row, pooling=SUM, max_seq=0, out_type=NONE):
  return (feature, start, dim, pooling, max_seq, out_type, out_index, out_offset, row)


def as_tuples(slices):
  return [(s.feature_idx, s.start, s.dim, s.pooling, s.max_sequence_length, s.out_type, s.out_index, s.out_offset,
           s.out_row_floats) for s in slices]


def call_text(forward, batch, slices, out_lens, embs, flag=0, n_fid=None, n_feature=None, n_nfl=4, rows=1, atomics=0,
              out_bits=None, n_emb=None, n_outputs=None):
  """``embs``: (row floats, floats, address bits) per matrix; ``n_fid`` / ``n_feature`` default to one fid per
  instance of ``n_nfl`` lists."""
  n_fid = n_nfl * batch if n_fid is None else n_fid
  n_feature = n_fid if n_feature is None else n_feature
  lines = ["call %d %d %d %d %d %d %d %d %d %d" % (forward, batch, n_fid, n_feature, n_nfl, flag, rows, atomics,
                                                 len(embs) if n_emb is None else n_emb,
                                                 len(out_lens) if n_outputs is None else n_outputs)]
  lines += ["emb %d %d %d" % e for e in embs]
  lines += ["out %d %d" % (n, out_bits[i] if out_bits else 0) for i, n in enumerate(out_lens)]
  lines += ["slice " + " ".join(map(str, s)) for s in slices]
  return "\n".join(lines) + "\n"


def case_call(c, forward, flag, atomics=0, rows=1):
  """A case of layout_cases as the raw caller of test_layout_forms_gpu hands it over."""
  slices, shapes = _layout_plan(c["cfgs"], c["batch"])
  lens = [int(np.prod(sh)) for sh in shapes]
  return hand_call(c, forward, flag, as_tuples(slices), lens, atomics, rows)


def hand_call(c, forward, flag, slices, lens, atomics=0, rows=1):
  embs = [(e.shape[1], e.size, 0) for e in c["embs"]]
  text = call_text(forward, c["batch"], slices, lens, embs, flag, len(c["fid_offset"]), len(c["feature_offset"]),
                   len(c["nfl_offset"]), rows, atomics)
  return text, slices


# ===================================================================== a plan as the driver prints it
def task_line(s):
  return "t %d %d %d %d %d %d %d %d" % (s[0], s[1], s[2], s[3], s[4], s[6], s[7], s[8])


def zero_line(out, offset, end, row):
  return "t -2 0 %d %d 0 %d %d %d" % (end - offset, ZERO_FILL, out, offset, row)


def L(form, idx, units=None, zeros=(), mask=0):
  """A launch: its form, the slices it holds (indices), its units as (first task, count, addn) — by default one
  per slice — then one task and unit per zero run (output, offset, end, row floats)."""
  idx = list(idx)
  units = [(q, 1, 0) for q in range(len(idx))] if units is None else list(units)
  return (form, idx, units + [(len(idx) + z, 1, 0) for z in range(len(zeros))], list(zeros), mask)


def plan_text(slices, launches, ext=0, skip=(0,)):
  out = ["ext %d" % ext, " ".join(["skip"] + [str(s) for s in skip])]
  for form, idx, units, zeros, mask in launches:
    out.append("launch %s mask=%x" % (form, mask))
    out += [task_line(slices[i]) for i in idx] + [zero_line(*z) for z in zeros]
    out += ["u %d %d %d" % u for u in units]
  return out


def _lists(slices, n_nfl):
  """t_off / t_idx: per named feature list the slices that read it, in configuration order."""
  by = [[i for i, s in enumerate(slices) if s[0] == f] for f in range(n_nfl)]
  off = [0]
  for b in by:
    off.append(off[-1] + len(b))
  return off, [i for b in by for i in b]


def grouped_text(slices, n_nfl, ext=0, n_outputs=1):
  off, idx = _lists(slices, n_nfl)
  return (["ext %d" % ext, " ".join(["skip"] + ["0"] * n_outputs), "grouped"] + [task_line(s) for s in slices] +
          [" ".join(["t_off"] + [str(v) for v in off]), " ".join(["t_idx"] + [str(v) for v in idx])])


# ===================================================================== the cases of test_layout_forms_gpu
# cid -> (outputs, launches forward with the flag as (skip, launches), launches of the gradient with the flag);
# launches as ranges of slices with the form.  Without the flag: the same ranges in the general form, no fill
# skipped (forward), the grouped gradient.
R = range
LETTERED = {
    # 32 x 64 = 2048 columns, exact width: one rows launch that writes whole rows; the gradient: rows, no mask
    "a": (1, ([1], [L("rows", R(32), mask=1)]), [L("rows", R(32))]),
    # 2049 columns: past the column table -> fill + copy
    "b": (1, ([0], [L("copy", R(33))]), [L("copy", R(33))]),
    # 2067 columns over five outputs, 42 slices: one copy launch
    "bh": (5, ([0] * 5, [L("copy", R(42))]), [L("copy", R(42))]),
    # 2044 columns + a tail of 4 columns = 2048: covered, the zero run rides in the launch
    "c4": (1, ([1], [L("rows", R(32), zeros=[(0, 8176, 8192, 8192)], mask=1)]), [L("rows", R(32))]),
    # ... a tail of 8 columns = 2052: the fill stays, rows launch of the 2044
    "c8": (1, ([0], [L("rows", R(32))]), [L("rows", R(32))]),
    # 48 slices, exact width: one launch, whole rows
    "d": (1, ([1], [L("rows", R(48), mask=1)]), [L("rows", R(48))]),
    # 48 slices + 1 zero run = 49 tasks: fill + rows
    "e": (1, ([0], [L("rows", R(48))]), [L("rows", R(48))]),
    # 49 slices: two rows launches behind the fill
    "f": (1, ([0], [L("rows", R(48)), L("rows", R(48, 49))]), [L("rows", R(48)), L("rows", R(48, 49))]),
    # 48 x 43 = 2064 columns (copy), then 5 x 4 (rows)
    "g": (1, ([0], [L("copy", R(48)), L("rows", R(48, 53))]), [L("copy", R(48)), L("rows", R(48, 53))]),
    # nine slices tile five outputs exactly: whole rows for all five
    "h": (5, ([1] * 5, [L("rows", R(9), mask=0x1f)]), [L("rows", R(9))]),
    # 70 matrices: pointer tables, fill for every output, two rows launches
    "i": (1, ([0], [L("rows", R(48)), L("rows", R(48, 70))]), [L("rows", R(48)), L("rows", R(48, 70))]),
    # widths that are no float4s: the general form; the flagged gradient keeps the launch form (one addend)
    "k": (1, ([0], [L("general", R(7))]), [L("general", R(7))]),
}


def _general(launches):
  return [L("general", idx, units[:len(idx)]) for _, idx, units, _, _ in launches]


def lettered_plans():
  for cid, (n_out, (skip, fwd), grad) in LETTERED.items():
    c = LC.build_case(cid)
    ext = 1 if cid == "i" else 0
    n_nfl = len(c["nfl_offset"])
    for flag in (FLAG, 0):
      text, s = case_call(c, 1, flag)
      yield ("%s-fwd-%d" % (cid, flag), text,
             plan_text(s, fwd, ext, skip) if flag else plan_text(s, _general(fwd), ext, [0] * n_out))
      text, s = case_call(c, 0, flag)
      yield ("%s-grad-%d" % (cid, flag), text,
             plan_text(s, grad, ext, [0] * n_out) if flag else grouped_text(s, n_nfl, ext, n_out))


def hand_plans():
  B = 19
  c = LC._hand_case(B)
  z = [(0, 8, 16, 24)]   # two_outputs: the gap of output 0, carried by every launch of the call
  hand = {
      # a gap and a tail: two zero runs, whole rows
      "gaps": ([1], [L("rows", R(2), zeros=[(0, 16, 32, 64), (0, 48, 64, 64)], mask=1)]),
      # overlapping slices: the fill stays, the later slice takes a launch of its own
      "overlap": ([0], [L("rows", [0]), L("rows", [1])]),
      "overlap_reversed": ([0], [L("rows", [0]), L("rows", [1])]),
      # output_len larger than batch * stride: the fill stays
      "rows_beyond_batch": ([0], [L("rows", [0])]),
      # output 0 tiled with a gap, output 1 overlapping twice: three launches
      "two_outputs": ([1, 0], [L("rows", R(3), zeros=z, mask=1), L("rows", [3], zeros=z, mask=1),
                               L("rows", [4], zeros=z, mask=1)]),
  }
  for hid, (skip, fwd) in hand.items():
    slices, lens = LC.HAND[hid](B)
    for flag in (FLAG, 0):
      text, s = hand_call(c, 1, flag, as_tuples(slices), lens)
      yield ("hand-%s-%d" % (hid, flag), text,
             plan_text(s, fwd, 0, skip) if flag else plan_text(s, _general(fwd), 0, [0] * len(lens)))


def other_case_plans():
  # the same columns of a feature in two layouts: forward whole rows of all three outputs; the flagged gradient is
  # not the copy form: grouped, or one general launch under MHTE_POOL_ATOMICS=1
  c = LC.overlap_case()
  for flag in (FLAG, 0):
    text, s = case_call(c, 1, flag)
    yield ("overlap-fwd-%d" % flag, text,
           plan_text(s, [L("rows", R(9), mask=7)], 0, [1, 1, 1]) if flag else plan_text(s, [L("general", R(9))], 0, [0] * 3))
    text, s = case_call(c, 0, flag)
    yield ("overlap-grad-%d" % flag, text, grouped_text(s, 3, 0, 3))
  text, s = case_call(c, 0, FLAG, atomics=1)
  yield ("overlap-grad-atomics", text, plan_text(s, [L("general", R(9))], 0, [0] * 3))
  # 60-slice ADDN, then a 60-slice CONCAT: the ADDN's first 48 slices (addn 1); its last 12 continue (addn 2: they
  # name the columns the first launch wrote) with 36 CONCAT slices behind them; the last 24
  c = LC.general_case()
  sixty = [L("general", R(48), [(0, 48, 1)]), L("general", R(48, 96), [(0, 12, 2)] + [(q, 1, 0) for q in R(12, 48)]),
           L("general", R(96, 120))]
  text, s = case_call(c, 1, 0)
  yield ("sixty-fwd", text, plan_text(s, sixty, 0, [0, 0]))
  text, s = case_call(c, 0, 0, atomics=1)
  yield ("sixty-grad-atomics", text, plan_text(s, sixty, 0, [0, 0]))
  text, s = case_call(c, 0, 0)
  yield ("sixty-grad", text, grouped_text(s, 60, 0, 2))
  # five features, all four output types, FIRSTN: 12 slices, the four of the ADDN layout one unit
  c = LC.mixed_case()
  mixed = [L("general", R(12), [(0, 4, 1)] + [(q, 1, 0) for q in R(4, 12)])]
  text, s = case_call(c, 1, 0)
  yield ("mixed-fwd", text, plan_text(s, mixed, 0, [0] * 6))
  text, s = case_call(c, 0, 0, atomics=1)
  yield ("mixed-grad-atomics", text, plan_text(s, mixed, 0, [0] * 6))
  text, s = case_call(c, 0, 0)
  yield ("mixed-grad", text, grouped_text(s, 5, 0, 6))


def edge_plans():
  B, E = 19, [(8, 8 * 40, 0)]
  one = [sl(0, 0, 4, 0, 0, 4)]
  # task count, counting zero runs: 46 and 47 slices with a tail run make 47 and 48 tasks (whole rows); 48 make 49
  for n in (46, 47, 48):
    s = [sl(i % 4, 4, 4, 0, 4 * i, 4 * n + 4) for i in range(n)]
    whole = n + 1 <= 48
    yield ("tasks-%d" % (n + 1), call_text(1, B, s, [B * (4 * n + 4)], E, FLAG),
           plan_text(s, [L("rows", R(n), zeros=[(0, 4 * n, 4 * n + 4, 4 * n + 4)] if whole else [], mask=int(whole))],
                     0, [int(whole)]))
  # float4 columns: kLayoutRowsMaxF = 2048 fit the rows kernel's column table, one more does not
  wide = [(8200, 8200 * 40, 0)]
  for dim, form in ((8192, "rows"), (8196, "copy")):
    s = [sl(0, 4, dim, 0, 0, dim)]
    yield ("columns-%d-fwd" % (dim // 4), call_text(1, B, s, [B * dim], wide, FLAG),
           plan_text(s, [L(form, [0], mask=int(form == "rows"))], 0, [int(form == "rows")]))
    yield ("columns-%d-grad" % (dim // 4), call_text(0, B, s, [B * dim], wide, FLAG), plan_text(s, [L(form, [0])]))
  # a FIRSTN slice is no copy: general form
  s = [sl(0, 0, 4, 0, 0, 8, FIRSTN, 2)]
  yield ("firstn", call_text(1, B, s, [B * 8], E, FLAG), plan_text(s, [L("general", [0])]))
  # a matrix, a row stride, an output or a slice start off a 16-byte boundary: general form
  yield ("misaligned-matrix", call_text(1, B, one, [B * 4], [(8, 320, 4)], FLAG), plan_text(one, [L("general", [0])]))
  yield ("misaligned-stride", call_text(1, B, one, [B * 4], [(6, 240, 0)], FLAG), plan_text(one, [L("general", [0])]))
  yield ("misaligned-output", call_text(1, B, one, [B * 4], E, FLAG, out_bits=[4]), plan_text(one, [L("general", [0])]))
  s = [sl(0, 2, 4, 0, 0, 4)]
  yield ("misaligned-start", call_text(1, B, s, [B * 4], E, FLAG), plan_text(s, [L("general", [0])]))
  # the flag without one fid per instance (n_fid != n_feature) is not honoured
  yield ("flag-two-fids", call_text(1, B, one, [B * 4], E, FLAG, n_fid=5 * B, n_feature=4 * B),
         plan_text(one, [L("general", [0])]))
  # MHTE_LAYOUT_ROWS=0: the copy form, and no output is left to a rows launch
  yield ("rows-off", call_text(1, B, one, [B * 4], E, FLAG, rows=0), plan_text(one, [L("copy", [0])]))
  yield ("rows-on", call_text(1, B, one, [B * 4], E, FLAG), plan_text(one, [L("rows", [0], mask=1)], 0, [1]))
  # kMaxLayoutOut = 32 outputs and kMaxLayoutEmb = 64 matrices travel in the arguments, one more: pointer tables
  for n_out in (32, 33):
    yield ("outputs-%d" % n_out, call_text(1, B, one, [B * 4] * n_out, E, FLAG),
           plan_text(one, [L("rows", [0], mask=1 - (n_out > 32))], int(n_out > 32), [int(n_out <= 32)] + [0] * (n_out - 1)))
  for n_emb in (64, 65):
    yield ("matrices-%d" % n_emb, call_text(1, B, one, [B * 4], E * n_emb, FLAG),
           plan_text(one, [L("rows", [0], mask=1 - (n_emb > 64))], int(n_emb > 64), [int(n_emb <= 64)]))
  # nothing to move: the fill only (and the slices are not looked at)
  yield ("batch-0", call_text(1, 0, [sl(0, 0, 0, 7, 0, 0)], [0], E, FLAG), plan_text([], []))
  yield ("slices-0", call_text(1, B, [], [B * 4], E, FLAG), plan_text([], []))
  yield ("slices-0-grad", call_text(0, B, [], [B * 4], E, 0), plan_text([], []))
  # a gradient without fids has nothing to group: the launch form
  yield ("grad-no-fids", call_text(0, B, one, [B * 4], E, 0, n_fid=0, n_feature=0), plan_text(one, [L("general", [0])]))


PLANS = {name: (text, want) for gen in (lettered_plans, hand_plans, other_case_plans, edge_plans)
         for name, text, want in gen()}


# ===================================================================== every error message
def _long_addn(n=60, odd=50):
  """An ADDN layout of more than 48 slices whose slice ``odd`` is 8 wide, the others 4."""
  return [sl(i % 4, 0, 8 if i == odd else 4, 0, 0, 8, out_type=ADDN) for i in range(n)]


def error_calls():
  B, E = 19, [(8, 320, 0)]
  ok = [sl(0, 0, 4, 0, 0, 4)]
  count, sizes = "layout: bad matrix / output count", "layout: bad sizes"
  yield "n_emb<0", call_text(1, B, ok, [B * 4], [], n_emb=-1), count
  yield "n_outputs>2^20", call_text(1, B, ok, [], E, n_outputs=(1 << 20) + 1), count
  yield "batch<0", call_text(1, -1, ok, [B * 4], E, n_fid=0), sizes
  yield "n_fid>int32", call_text(1, B, ok, [B * 4], E, n_fid=1 << 31), sizes
  yield "n_feature>int32", call_text(0, B, ok, [B * 4], E, n_fid=4, n_feature=1 << 31), sizes
  fit = "layout: slice 1 does not fit its output"
  for what, bad in (("out_index", sl(0, 0, 4, 1, 0, 4)), ("out_index<0", sl(0, 0, 4, -1, 0, 4)), ("dim", sl(0, 0, 0, 0, 0, 4)),
                    ("row", sl(0, 0, 4, 0, 0, 0)), ("offset", sl(0, 0, 4, 0, 4, 4)), ("rows", sl(0, 0, 4, 0, 0, 8)),
                    ("firstn", sl(0, 0, 2, 0, 0, 4, FIRSTN, 3))):
    for forward in (1, 0):
      yield "fit-%s-%d" % (what, forward), call_text(forward, B, ok + [bad], [B * 4], E), fit
  yield ("firstn-addn", call_text(1, B, [sl(0, 0, 4, 0, 0, 12, FIRSTN, 3, ADDN)], [B * 12], E),
         "layout: FIRSTN pooling cannot be added (ADDN)")
  width = "layout: slices of an ADDN layout differ in width"
  yield "addn-width", call_text(1, B, [sl(0, 0, 4, 0, 0, 8, out_type=ADDN), sl(1, 0, 8, 0, 0, 8, out_type=ADDN)], [B * 8], E), width
  # slice 50 of a 60-slice ADDN layout is compared with slice 0, not with slice 48 (the first of its launch):
  # refused in both directions, in the grouped and in the launch form of the gradient
  for name, forward, flag, atomics in (("fwd", 1, 0, 0), ("fwd-flag", 1, FLAG, 0), ("grad", 0, 0, 0), ("grad-flag", 0, FLAG, 0),
                                       ("grad-atomics", 0, 0, 1)):
    yield "addn-width-50-" + name, call_text(forward, B, _long_addn(), [B * 8], E, flag, atomics=atomics), width
  # ... and an ADDN layout whose slices 48 .. 59 all differ from slices 0 .. 47 (each launch alike in itself)
  two = [sl(i % 4, 0, 4 if i < 48 else 8, 0, 0, 8, out_type=ADDN) for i in range(60)]
  for forward in (1, 0):
    yield "addn-width-48-%d" % forward, call_text(forward, B, two, [B * 8], E), width


ERRORS = {name: (text, msg) for name, text, msg in error_calls()}


# ===================================================================== the tests
def _compile(exe, extra=()):
  subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", *extra, "-I" + os.path.join(ROOT, "monolith_amd", "csrc"),
                         DRIVER_SRC, "-o", exe])
  return exe


def _run(exe, text):
  return subprocess.run([exe], input=text, capture_output=True, text=True)


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
  return _compile(str(tmp_path_factory.mktemp("layout_plan") / "layout_plan_host"))


@pytest.mark.parametrize("name", sorted(PLANS))
def test_planned_sequence(driver, name):
  text, want = PLANS[name]
  r = _run(driver, text)
  assert r.returncode == 0, (r.returncode, r.stdout[-500:], r.stderr[-500:])   # (1: a whole-rows launch that is not rows)
  assert r.stdout.strip().split("\n") == want


def test_the_cases_are_the_shapes_their_names_say():
  """What the expectations above rely on: slice counts, outputs and the fids-per-instance of the shared cases."""
  assert {cid: len(as_tuples(_layout_plan(LC.build_case(cid)["cfgs"], 19)[0])) for cid in LC.CASES} == {
      "a": 32, "b": 33, "bh": 42, "c4": 32, "c8": 32, "d": 48, "e": 48, "f": 49, "g": 53, "h": 9, "i": 70, "k": 7}
  assert sorted(LETTERED) == sorted(LC.CASES) and sorted(LC.HAND) == sorted(
      ["gaps", "overlap", "overlap_reversed", "rows_beyond_batch", "two_outputs"])
  g = LC.general_case()
  assert len(g["fid_offset"]) != len(g["feature_offset"]) and len(g["embs"]) == 3


@pytest.mark.parametrize("name", sorted(ERRORS))
def test_every_refusal(driver, name):
  text, msg = ERRORS[name]
  r = _run(driver, text)
  assert r.returncode == 0 and r.stdout == "refused: %s\n" % msg, (r.stdout[-500:], r.stderr[-500:])


def test_plan_driver_is_clean_under_asan_and_ubsan(driver, tmp_path):
  flags = ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
  probe = subprocess.run(["g++", "-x", "c++", "-", *flags, "-o", str(tmp_path / "probe")], input="int main() {}\n",
                         capture_output=True, text=True)
  if probe.returncode != 0:
    pytest.skip("the sanitizer runtimes are not installed: " + probe.stderr.strip().split("\n")[-1])
  exe = _compile(str(tmp_path / "layout_plan_host_san"), flags)
  for name, (text, _) in sorted(list(PLANS.items()) + list(ERRORS.items())):
    r = _run(exe, text)
    assert r.returncode == 0, (name, r.stderr[-2000:])
    assert r.stdout == _run(driver, text).stdout, name
