"""CPU suite: the host-only parts of the checkpoint path (monolith_amd/csrc/mhte_ckpt_parts.h) through
tests/ckpt_host_driver.cc, built by g++ with MHTE_HOST_ONLY: the shard arithmetic, the shard-thread pool,
the read-ahead record stream of a restore, the cut of a batch into runs of distinct ids and the initial
row of a table.  The multi-threaded ones also run in builds of the same stand-alone driver under the
address + undefined-behaviour sanitizers and under the thread sanitizer."""
import math
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import ckpt_proto as P  # noqa: E402

SRC = os.path.join(ROOT, "tests", "ckpt_host_driver.cc")
VARIANTS = {"plain": ["-O2"],
            "asan_ubsan": ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"],
            "tsan": ["-O1", "-g", "-fsanitize=thread"]}
SAN_ENV = {"ASAN_OPTIONS": "detect_leaks=1:halt_on_error=1", "UBSAN_OPTIONS": "halt_on_error=1:print_stacktrace=1",
           "TSAN_OPTIONS": "halt_on_error=1:exitcode=66"}


_built = {}


def _build(tmp_path_factory, variant):
  if variant in _built:
    return _built[variant]
  exe = str(tmp_path_factory.mktemp("ckpt_host_" + variant) / "driver")
  r = subprocess.run(["g++", "-std=c++17", "-DMHTE_HOST_ONLY", "-pthread"] + VARIANTS[variant] + ["-o", exe, SRC],
                     capture_output=True, text=True)
  if r.returncode != 0 and variant != "plain" and any(
      "cannot find" in line and ("asan" in line or "ubsan" in line or "tsan" in line)
      for line in r.stderr.splitlines()):
    pytest.skip("this g++ has no runtime library for the %s build" % variant)
  assert r.returncode == 0, r.stderr
  _built[variant] = exe
  return exe


@pytest.fixture(scope="module")
def plain(tmp_path_factory):
  return _build(tmp_path_factory, "plain")


@pytest.fixture(scope="module", params=list(VARIANTS))
def driver(request, tmp_path_factory):
  """every build of the driver, the sanitizer ones included"""
  return _build(tmp_path_factory, request.param)


def run(exe, *args, code=0):
  r = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True, env=dict(os.environ, **SAN_ENV))
  assert r.returncode == code and "Sanitizer" not in r.stderr, (r.returncode, r.stdout, r.stderr)
  return r.stdout.strip()


# ---------------------------------------------------------------------------------- shard arithmetic
@pytest.mark.parametrize("hp,total", [(hp, t) for hp in (3, 10) for t in (1, 3, 5, 7, 8)] + [(3, 16)])
def test_shard_bucket_ranges_tile_the_table(plain, hp, total):
  got = [tuple(int(x) for x in line.split()) for line in run(plain, "shardrange", hp, total).splitlines()]
  q, r = divmod(1 << hp, total)   # the walk of tests/test_boundary_gpu.py
  want = []
  for shard in range(total):
    begin = shard * q + min(shard, r)
    want.append((begin, begin + q + (1 if shard < r else 0)))
  assert got == want
  assert got[0][0] == 0 and got[-1][1] == 1 << hp
  assert all(a[1] == b[0] for a, b in zip(got, got[1:]))       # no gap, no overlap
  assert all(b <= e for b, e in got)
  if total > 1 << hp:
    assert sum(1 for b, e in got if b == e) == total - (1 << hp)   # more shards than buckets: empty ranges


@pytest.mark.parametrize("entries,requested,want", [
    (0, -1, 1), (999_999, -1, 1), (1_000_000, -1, 1), (4_000_000, -1, 4), (50_000_000, -1, 4),
    (4_000_000, 0, 1), (0, 7, 7), (50_000_000, 7, 7)])
def test_pick_nshards(plain, entries, requested, want):
  assert int(run(plain, "picknshards", entries, requested)) == want


# ---------------------------------------------------------------------------------- record stream
STRETCH = 4096


def _fnv(records):
  h = 1469598103934665603
  for r in records:
    for c in struct.pack("<Q", len(r)) + r:
      h = ((h ^ c) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
  return h


@pytest.fixture(scope="module")
def record_files(tmp_path_factory):
  """1000 records of 0..79 bytes — a zero-length one and one longer than the stretch among them — framed by
  the independent Python writer, plain and as a snappy block stream of small blocks (several per stretch);
  and the same cut in the middle of the last record."""
  rng = np.random.default_rng(5)
  records = [rng.integers(0, 256, int(n), dtype=np.uint8).tobytes() for n in rng.integers(0, 80, 1000)]
  records[10] = b""
  records[500] = rng.integers(0, 256, 2 * STRETCH + 123, dtype=np.uint8).tobytes()
  raw = b"".join(P.frame(r) for r in records)
  d = tmp_path_factory.mktemp("records")
  paths = {}
  for name, data in (("whole", raw), ("cut", raw[:-9])):
    paths[name, 0] = str(d / (name + ".plain"))
    open(paths[name, 0], "wb").write(data)
    paths[name, 1] = str(d / (name + ".snappy"))
    open(paths[name, 1], "wb").write(P.write_tf_snappy(data, block=1500))
  return records, paths


@pytest.mark.parametrize("snappy", (0, 1))
@pytest.mark.parametrize("take", (1, 7, 256, 0))   # 0: more than is left
def test_record_stream_hands_out_every_record_in_order(driver, record_files, snappy, take):
  records, paths = record_files
  out = [int(x) for x in run(driver, "stream", paths["whole", snappy], snappy, STRETCH, 2, take).split()]
  count, total, digest, takes = out[:4]
  # (the driver has also compared every record with a plain RecordReader::read loop over the file)
  assert (count, total, digest) == (len(records), sum(len(r) for r in records), _fnv(records))
  assert takes >= math.ceil(len(records) / (take or len(records)))
  if snappy:   # many stretches long: no single take returns all of it (a plain file is read 1 MiB at a time)
    assert takes > 1
  assert out[4:] == [0, 0, 0]   # at the end take returns 0, and keeps returning 0


@pytest.mark.parametrize("snappy", (0, 1))
def test_record_stream_surfaces_a_cut_file_and_still_joins_its_helper(driver, record_files, snappy):
  _, paths = record_files
  out = run(driver, "stream", paths["cut", snappy], snappy, STRETCH, 2, 7, code=1)
  assert out.startswith("ERROR truncated record"), out


# ---------------------------------------------------------------------------------- distinct runs
I64_MIN = -(1 << 63)


DISTINCT_5000 = [I64_MIN] + [int(x) for x in np.random.default_rng(3).permutation(np.arange(-2500, 2499))]


@pytest.mark.parametrize("ids,want", [
    ([1, 2, 1, 1, 3, 2], [2, 3, 6]),
    ([I64_MIN, -7, I64_MIN, I64_MIN, -3, -7], [2, 3, 6]),
    (DISTINCT_5000, [5000]),
    ([I64_MIN] * 64, list(range(1, 65))),
    ([-9] * 64, list(range(1, 65)))], ids=["example", "example_negative", "distinct_5000", "int64_min_64", "one_id_64"])
def test_next_distinct_run(driver, tmp_path, ids, want):
  assert len(ids) == want[-1] and (want != [5000] or len(set(ids)) == 5000)
  p = tmp_path / "ids"
  p.write_bytes(np.asarray(ids, np.int64).tobytes())
  assert [int(x) for x in run(driver, "runs", p).split()] == want


# ---------------------------------------------------------------------------------- shard-thread pool
def test_shard_pool_runs_every_job_once_on_at_most_16_threads(driver):
  once, most, finished_at_error, error = run(driver, "pool", 40).split(None, 3)
  assert (int(once), int(finished_at_error), error) == (40, -1, "none")
  assert 1 <= int(most) <= 16


def test_shard_pool_reports_the_first_failed_shard_after_all_have_finished(driver):
  once, most, finished_at_error, error = run(driver, "pool", 40, 9, 3).split(None, 3)
  assert int(once) == 40 and 1 <= int(most) <= 16
  assert int(finished_at_error) == 40
  assert error == "job 3 failed as asked"


# ---------------------------------------------------------------------------------- initial row
SGD, ADAGRAD, ADAM, AMSGRAD, GROUP_ADAGRAD = 0, 1, 7, 8, 11
ZEROS, ONES, CONSTANT, RANDOM_UNIFORM = 0, 1, 2, 3


@pytest.mark.parametrize("dim", (1, 5))
def test_initial_row(plain, dim):
  """initializer + optimizer Init as the restore pre-fills a row: weights from the initializer (random-uniform
  starts at 0: the dump always carries the weights), Adagrad's accumulator at its initial value, Adam's and
  AMSGrad's vectors at 0 with beta1, beta2 behind them as the running powers, GroupAdagrad's sum at its
  initial value; the rest of a 4-float slot stays 0."""
  # (opt, init, init value, p0, p1)
  segs = [(SGD, ONES, 0.0, 0.0, 0.0), (ADAGRAD, CONSTANT, 0.25, 0.1, 0.0), (ADAM, RANDOM_UNIFORM, -0.5, 0.9, 0.99),
          (AMSGRAD, ZEROS, 0.0, 0.8, 0.95), (GROUP_ADAGRAD, CONSTANT, -2.0, 0.3, 0.0)]
  args = []
  for opt, init, value, p0, p1 in segs:
    args += [opt, dim, init, value, p0, p1]
  got = np.array(run(plain, "initrow", len(segs), *args).split(), np.float32)
  weights, state = [], []
  for opt, init, value, p0, p1 in segs:
    weights += [{ZEROS: 0.0, ONES: 1.0, CONSTANT: value, RANDOM_UNIFORM: 0.0}[init]] * dim
    if opt == ADAGRAD:
      state += [p0] * dim
    elif opt in (ADAM, AMSGRAD):
      state += [0.0] * ((2 if opt == ADAM else 3) * dim) + [p0, p1, 0.0, 0.0]
    elif opt == GROUP_ADAGRAD:
      state += [p0, 0.0, 0.0, 0.0]
  np.testing.assert_array_equal(got, np.array(weights + state, np.float32))
