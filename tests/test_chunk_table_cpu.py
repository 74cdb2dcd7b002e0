"""CPU suite of the chunk table (csrc/mhte_chunk_table.h): the argument block at the three shapes the ops use
(one pointer and offsets, two pointers, two pointers and offsets) and at two inline capacities (4, and the ops'
128 / 128 / 96), driven on the host by tests/chunk_table_host_driver.cc — the builder, the packed block of a
table that outgrew the arguments, the binary search and the forward-only cursor are the functions the kernels
call, compared with a numpy restatement (a searchsorted over the cumulative chunk counts).  The driver is run
once more under AddressSanitizer and UndefinedBehaviorSanitizer, stand-alone."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "chunk_table_host_driver.cc")
CHUNK = 4096
# (shape, pointers, offsets?) x capacities
SHAPES = {"p1o": (1, True, (4, 128)), "p2": (2, False, (4, 128)), "p2o": (2, True, (4, 96))}
CASES = [(s, n) for s, (_, _, caps) in SHAPES.items() for n in caps]
IDS = ["%s-%d" % c for c in CASES]
EDGE = [1, 4095, 4096, 4097, 8193, 1, 1, 3 * 4096]
TABLES = {
    "edges": EDGE,
    "edges + 200 one-chunk": EDGE + [1 + (37 * i) % 4096 for i in range(200)],
    "single tensor": [5 * 4096 + 1],
    "last tensor has one chunk": [3 * 4096, 9 * 4096 + 7, 12],
}
STRIDES = [1, 2, 3, 7, 1024, 2048]


def _compile(exe, extra=()):
  subprocess.check_call(["g++", "-O2", "-std=c++17", "-DMHTE_HOST_ONLY", *extra,
                         "-I" + os.path.join(ROOT, "monolith_amd", "csrc"), SRC, "-o", exe])
  return exe


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
  return _compile(str(tmp_path_factory.mktemp("chunk_table") / "chunk_table_host"))


def _run(driver, *args):
  return subprocess.run([driver] + [str(a) for a in args], capture_output=True, text=True, check=True).stdout


def _truth(lens, skip=-1):
  """(index, len, off, chunk0) of the entries that take part, and the number of chunks."""
  rows, chunks, off = [], 0, 0
  for i, n in enumerate(lens):
    if n != 0 and i != skip:
      rows.append((i, n, off, chunks))
      chunks += (n + CHUNK - 1) // CHUNK
    off += (n + 15) // 16 * 16
  return rows, chunks


def _tensor_of(lens):
  """tensor of every chunk: a searchsorted over the cumulative chunk counts"""
  counts = np.array([(n + CHUNK - 1) // CHUNK for n in lens], dtype=np.int64)
  ends = np.cumsum(counts)
  return np.searchsorted(ends, np.arange(ends[-1]), side="right")


# ---- the builder -----------------------------------------------------------------------------------------
def _build_lists(cap):
  lists = {"N - 1": [100 + 4096 * (i % 3) for i in range(cap - 1)],
           "N": [100 + 4096 * (i % 3) for i in range(cap)],
           "N + 1": [100 + 4096 * (i % 3) for i in range(cap + 1)],
           "155": [1 + 511 * i for i in range(155)],
           "none": [],
           "all empty": [0] * 7}
  return lists


@pytest.mark.parametrize("shape,cap", CASES, ids=IDS)
def test_build_equals_numpy(shape, cap, driver):
  nptr, has_off, _ = SHAPES[shape]
  for name, lens in _build_lists(cap).items():
    for skip in ([-1] if len(lens) < 3 else [-1, len(lens) // 2]):
      out = _run(driver, shape, cap, "build", skip, *lens).split("\n")
      rows, chunks = _truth(lens, skip)
      ext = len(rows) > cap
      assert out[0].split() == [str(len(rows)), str(chunks), str(int(ext))], (name, skip)
      got = [tuple(int(x) for x in line.split()) for line in out[1:1 + len(rows)]]
      want = [(i, n, off if has_off else -1, c0, 1) for i, n, off, c0 in rows]
      assert got == want, (name, skip)
      if skip >= 0 and lens[skip]:   # the skipped entry keeps its span: the one behind it keeps its offset
        assert all(r[0] != skip for r in rows)
        nxt = [r for r in rows if r[0] == skip + 1][0]
        assert nxt[2] == sum((n + 15) // 16 * 16 for n in lens[:skip + 1])
      tail = [line for line in out[1 + len(rows):] if line]
      if ext:   # the packed block: the pointer columns, the lengths (, the offsets), chunk0; nothing else
        m, cols8 = len(rows), nptr + 1 + int(has_off)
        assert tail == ["cols " + " ".join(str(8 * m * j) for j in range(cols8 + 1)) + " %d" % (m * (8 * cols8 + 4))]
      else:
        assert tail == []
  # at N the table rides in the arguments, at N + 1 it does not
  assert _run(driver, shape, cap, "build", -1, *([5] * cap)).split("\n")[0].split()[2] == "0"
  assert _run(driver, shape, cap, "build", -1, *([5] * (cap + 1))).split("\n")[0].split()[2] == "1"


@pytest.mark.parametrize("shape,cap", CASES, ids=IDS)
def test_builder_refuses_2_31_chunks(shape, cap, driver):
  assert _run(driver, shape, cap, "build", -1, 2 ** 43).strip() == "too many chunks"
  assert _run(driver, shape, cap, "build", -1, 7, 2 ** 43 - 4096, 5).strip() == "too many chunks"
  # one chunk below the bound is taken
  assert _run(driver, shape, cap, "build", -1, 2 ** 43 - 4096).split("\n")[0].split()[:2] == ["1", str(2 ** 31 - 1)]


# ---- the search ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,cap", CASES, ids=IDS)
@pytest.mark.parametrize("table", ["edges", "edges + 200 one-chunk"])
def test_lookup_equals_the_scan(shape, cap, table, driver):
  lens = TABLES[table]
  want = _tensor_of(lens)
  lines = [line for line in _run(driver, shape, cap, "lookup", *lens).split("\n") if line]
  assert len(lines) == want.size
  for c, line in enumerate(lines):
    got = [int(x) for x in line.split()]
    # from every valid lower bound lo <= answer the search gives the answer
    assert got == [want[c]] * (want[c] + 1), (c, got)


# ---- the cursor ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,cap", CASES, ids=IDS)
@pytest.mark.parametrize("table", sorted(TABLES))
def test_cursor_equals_independent_searches(shape, cap, table, driver):
  lens = TABLES[table]
  of = _tensor_of(lens)
  C = of.size
  jumped = False
  for G in STRIDES:
    lines = [line for line in _run(driver, shape, cap, "cursor", G, *lens).split("\n") if line]
    assert len(lines) == min(G, C)
    for w, line in enumerate(lines):
      got = [tuple(int(x) for x in pair.split(":")) for pair in line.split()]
      want = [(c, of[c]) for c in range(w, C, G)]
      assert got == want, (G, w)
      jumped = jumped or any(b[1] - a[1] > 2 for a, b in zip(want, want[1:]))
  if table == "edges + 200 one-chunk":   # strides that pass over several whole tensors at once
    assert jumped


# ---- the same driver under the sanitizers ----------------------------------------------------------------
def test_driver_is_clean_under_asan_and_ubsan(tmp_path):
  exe = str(tmp_path / "chunk_table_host_san")
  flags = ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
  probe = subprocess.run(["g++", "-x", "c++", "-", *flags, "-o", str(tmp_path / "probe")], input="int main() {}\n",
                         capture_output=True, text=True)
  if probe.returncode != 0:
    pytest.skip("the sanitizer runtimes are not installed: " + probe.stderr.strip().split("\n")[-1])
  _compile(exe, flags)
  big = TABLES["edges + 200 one-chunk"]
  for shape, cap in CASES:
    for args in (["build", -1] + big, ["build", 3] + [5] * (cap + 1), ["build", -1, 2 ** 43], ["lookup"] + big,
                 ["cursor", 7] + big, ["cursor", 1024] + big, ["cursor", 3] + TABLES["single tensor"]):
      r = subprocess.run([exe, shape, str(cap)] + [str(a) for a in args], capture_output=True, text=True)
      assert r.returncode == 0, (shape, cap, args[0], r.stderr[-2000:])
