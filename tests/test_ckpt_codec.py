"""CPU suite: the checkpoint codec (monolith_amd/csrc/mhte_ckpt.h, compiled host-only with g++)
against (a) the reference's own golden EntryDump (embedding_hash_table_test.h:78-93), (b) the
protobuf runtime on message classes restating the reference's .proto files, (c) the standard
CRC-32C check value, (d) an independent pure-Python TFRecord / TF-snappy reader and writer."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import ckpt_proto as P  # noqa: E402

(SGD, ADAGRAD, FTRL, MOMENTUM, ADADELTA, RMSPROP, RMSPROPV2, ADAM, AMSGRAD, MOVING_AVERAGE,
 BATCH_SOFTMAX, GROUP_ADAGRAD) = range(12)
# (state vectors, scalars) per kind, in the engine's row (scalars sit in a 4-float slot; batch
# softmax keeps its int64 step in the first two words of one)
STATE = {SGD: (0, 0), ADAGRAD: (1, 0), FTRL: (2, 0), MOMENTUM: (1, 0), ADADELTA: (2, 0), RMSPROP: (1, 0),
         RMSPROPV2: (1, 0), ADAM: (2, 2), AMSGRAD: (3, 2), MOVING_AVERAGE: (0, 0), BATCH_SOFTMAX: (0, 2),
         GROUP_ADAGRAD: (0, 1)}


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
  exe = str(tmp_path_factory.mktemp("ckpt") / "ckpt_driver")
  subprocess.check_call(["g++", "-O2", "-std=c++17", "-DMHTE_HOST_ONLY", "-pthread", "-o", exe,
                         os.path.join(ROOT, "tests", "ckpt_host_driver.cc")])
  return exe


def run(exe, *args):
  return subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True,
                        check=True).stdout.strip()


def reference_entry(id_, ts, segs, row, dim, with_id=True, packed=False):
  """EntryAccessor::Save (entry_accessor.cc:218-226) through the protobuf runtime."""
  e = P.EntryDump()
  if with_id:
    e.id = id_
  e.num.extend(row[:dim])
  st = dim
  for kind, d in segs:
    if kind == MOVING_AVERAGE:   # Save() returns an empty OptimizerDump (moving_average_optimizer.cc:54-57)
      continue
    s = e.opt.dump.add()
    if kind == BATCH_SOFTMAX:
      s.batch_softmax.global_step = int(np.array(row[st:st + 2], np.float32).view(np.int64)[0])
    elif kind == GROUP_ADAGRAD:
      s.group_adagrad.grad_square_sum = row[st]
    elif kind == SGD:
      s.sgd.SetInParent()
    elif kind == ADAGRAD:
      s.adagrad.norm.extend(row[st:st + d])
    elif kind == FTRL:
      s.ftrl.norm.extend(row[st:st + d])
      s.ftrl.zero.extend(row[st + d:st + 2 * d])
    elif kind == MOMENTUM:
      s.momentum.n.extend(row[st:st + d])
    elif kind == RMSPROP:
      s.rmsprop.n.extend(row[st:st + d])
    elif kind == RMSPROPV2:
      s.rmspropv2.n.extend(row[st:st + d])
    elif kind == ADADELTA:
      s.adadelta.accum.extend(row[st:st + d])
      s.adadelta.accum_update.extend(row[st + d:st + 2 * d])
    elif kind == ADAM:
      s.adam.m.extend(row[st:st + d])
      s.adam.v.extend(row[st + d:st + 2 * d])
      s.adam.beta1_power, s.adam.beta2_power = row[st + 2 * d], row[st + 2 * d + 1]
    else:
      s.amsgrad.m.extend(row[st:st + d])
      s.amsgrad.v.extend(row[st + d:st + 2 * d])
      s.amsgrad.vhat.extend(row[st + 2 * d:st + 3 * d])
      s.amsgrad.beta1_power, s.amsgrad.beta2_power = row[st + 3 * d], row[st + 3 * d + 1]
    nv, ns = STATE[kind]
    st += nv * d + (4 if ns else 0)
  e.last_update_ts_sec = ts
  return e.SerializeToString()


def test_crc32c_check_value(driver):
  crc, m = run(driver, "crc", "123456789").split()
  assert crc == "e3069283"                       # CRC-32C check value (RFC 3720 B.4)
  assert int(m, 16) == P.masked(b"123456789")
  # the sliced-table form (hosts without SSE4.2) agrees, at lengths around its 8-byte stride
  for text in ("123456789", "", "a", "abcdefg", "abcdefgh", "abcdefghi", "x" * 1000 + "yz"):
    assert run(driver, "crcsoft", text) == run(driver, "crc", text).split()[0]


def test_reference_golden_entry_dump(driver):
  """embedding_hash_table_test.h:78-93: Sgd table, id 1 after AssignAdd -> EntryDump
  {num: 1, opt {dump {sgd {}}}, last_update_ts_sec: 0}; the Save path adds the id (field 1)."""
  golden = bytes.fromhex("150000803f" "1a040a021200" "2000")
  e = P.EntryDump()
  e.num.append(1.0)
  e.opt.dump.add().sgd.SetInParent()
  e.last_update_ts_sec = 0
  assert e.SerializeToString() == golden         # the descriptors restate the .proto faithfully
  got = bytes.fromhex(run(driver, "entry", 7, 0, 1, 1, SGD, 1, 1.0))
  assert got[:9] == b"\x09" + (7).to_bytes(8, "little")
  assert got[9:] == golden


@pytest.mark.parametrize("segs", [[(SGD, 3)], [(ADAGRAD, 4)], [(FTRL, 2)],
                                  [(FTRL, 1), (ADAGRAD, 5), (SGD, 2)], [(MOMENTUM, 3)],
                                  [(ADADELTA, 2)], [(RMSPROP, 2), (RMSPROPV2, 1)], [(ADAM, 4)],
                                  [(AMSGRAD, 2), (ADAM, 1), (SGD, 1)], [(GROUP_ADAGRAD, 3), (ADAGRAD, 2)]])
def test_entry_bytes_equal_protobuf_runtime(driver, segs):
  rng = np.random.default_rng(len(segs) * 11 + segs[0][1])
  dim = sum(d for _, d in segs)
  rf = dim + sum(STATE[k][0] * d + (4 if STATE[k][1] else 0) for k, d in segs)
  row = rng.standard_normal(rf).astype(np.float32)
  for id_, ts in ((-3, 0), (1 << 62, 1700000123), (-(1 << 63), 4294967295)):
    args = ["entry", id_, ts, dim, len(segs)] + [x for s in segs for x in s] + [repr(float(v)) for v in row]
    got = bytes.fromhex(run(driver, *args))
    assert got == reference_entry(id_, ts, segs, row.tolist(), dim)


def test_decode_accepts_unpacked_packed_and_missing_fields(driver, tmp_path):
  segs = [(FTRL, 2), (ADAGRAD, 3)]
  dim, rf = 5, 5 + 4 + 3
  row = (np.arange(rf) * 0.5 + 0.25).astype(np.float32)
  seg_args = [x for s in segs for x in s]
  raw = reference_entry(99, 1234, segs, row.tolist(), dim)
  (tmp_path / "a.hex").write_text(raw.hex())
  out = run(driver, "decode", tmp_path / "a.hex", dim, len(segs), *seg_args).split()
  assert int(out[0]) == 99 and int(out[1]) == 1234
  np.testing.assert_array_equal(np.array(out[2:], np.float32), row)
  # packed repeated floats (a proto3-style writer) decode the same
  def packed(field, vals):
    b = np.asarray(vals, np.float32).tobytes()
    return bytes([(field << 3) | 2]) + P._varint(len(b)) + b
  ftrl = packed(1, row[7:9]) + packed(2, row[5:7])
  ada = packed(1, row[9:12])
  opt = b"".join(b"\x0a" + P._varint(len(m) + 2) + bytes([t]) + P._varint(len(m)) + m
                 for t, m in ((0x1a, ftrl), (0x0a, ada)))
  raw2 = b"\x09" + (99).to_bytes(8, "little") + packed(2, row[:5]) + b"\x1a" + P._varint(len(opt)) + opt
  (tmp_path / "b.hex").write_text(raw2.hex())
  out = run(driver, "decode", tmp_path / "b.hex", dim, len(segs), *seg_args).split()
  assert int(out[0]) == 99 and int(out[1]) == 0     # no timestamp in the dump -> 0 (:384-386)
  np.testing.assert_array_equal(np.array(out[2:], np.float32), row)
  # an entry without optimizer dump keeps the pre-filled state (driver pre-fills -7)
  e = P.EntryDump()
  e.id = 5
  e.num.extend(row[:5].tolist())
  (tmp_path / "c.hex").write_text(e.SerializeToString().hex())
  out = run(driver, "decode", tmp_path / "c.hex", dim, len(segs), *seg_args).split()
  np.testing.assert_array_equal(np.array(out[2:7], np.float32), row[:5])
  assert all(float(x) == -7.0 for x in out[7:])


def test_moving_average_and_batch_softmax_dumps(driver, tmp_path):
  """A segment whose optimizer saves nothing contributes no SingleOptimizerDump (and takes none
  back on restore, optimizer_combination.cc:86-97); batch softmax dumps one int64."""
  segs = [(MOVING_AVERAGE, 2), (BATCH_SOFTMAX, 1), (ADAGRAD, 2), (MOVING_AVERAGE, 1)]
  dim = 6
  rf = dim + 4 + 2
  for step in (0, 5, (1 << 40) + 12345):
    row = (np.arange(rf) * 0.25 + 1.0).astype(np.float32)
    row[dim:dim + 2] = np.array([step], np.int64).view(np.float32)
    row[dim + 2:dim + 4] = 0.0
    seg_args = [x for s_ in segs for x in s_]
    args = ["entry", 42, 77, dim, len(segs)] + seg_args + [repr(float(v)) for v in row]
    got = bytes.fromhex(run(driver, *args))
    ref = reference_entry(42, 77, segs, row, dim)
    assert got == ref
    e = P.EntryDump()
    e.ParseFromString(got)
    assert len(e.opt.dump) == 2 and e.opt.dump[0].batch_softmax.global_step == step
    (tmp_path / "m.hex").write_text(got.hex())
    out = run(driver, "decode", tmp_path / "m.hex", dim, len(segs), *seg_args).split()
    dec = np.array(out[2:], np.float32)
    np.testing.assert_array_equal(dec[:dim], row[:dim])
    assert int(dec[dim:dim + 2].view(np.int64)[0]) == step
    np.testing.assert_array_equal(dec[dim + 4:], row[dim + 4:])


@pytest.mark.parametrize("snappy", [0, 1])
def test_record_files_roundtrip_and_match_python_reader(driver, tmp_path, snappy):
  path = tmp_path / ("f%d" % snappy)
  n, ln = 3000, 300                                 # ~1 MB: several 256 KiB snappy blocks
  run(driver, "write", path, snappy, n, ln)
  cnt, x, total = (int(v) for v in run(driver, "read", path, snappy).split())
  recs = [bytes([i & 0xff]) * (ln + i % 7) for i in range(n)]
  assert cnt == n and total == sum(len(r) for r in recs)
  stream = path.read_bytes()
  raw = P.read_tf_snappy(stream) if snappy else stream
  assert P.unframe(raw) == recs
  # and the other way: a file framed (and compressed WITH copy elements) by the Python writer
  path2 = tmp_path / ("g%d" % snappy)
  raw2 = b"".join(P.frame(r) for r in recs)
  path2.write_bytes(P.write_tf_snappy(raw2) if snappy else raw2)
  if snappy:
    assert len(path2.read_bytes()) < len(raw2) // 4   # copies were emitted
  cnt2, x2, total2 = (int(v) for v in run(driver, "read", path2, snappy).split())
  assert (cnt2, x2, total2) == (cnt, x, total)
  # the restore path's reader: stretches of whole records, snappy blocks unpacked side by side; the
  # stretch size decides where records are cut and carried over, the thread count nothing
  for f in (path, path2):
    for stretch, threads in ((1 << 20, 1), (1 << 20, 4), (300000, 3), (1000, 2), (64 << 20, 8)):
      c, xx, tot, batches = (int(v) for v in run(driver, "readbatch", f, snappy, stretch, threads).split())
      assert (c, xx, tot) == (cnt, x, total), (f, stretch, threads)
      if stretch == 1000 and snappy:   # (a plain file is read a MiB at a time at least)
        assert batches > 3


def _literal_only_stream(raw: bytes) -> bytes:
  """What the engine's writer emits for a record stream (mhte_ckpt.h RecordWriter): blocks of
  <= 256 KiB, each [4-byte big-endian packed length | varint length | literal elements <= 64 KiB]."""
  def varint(v):
    out = bytearray()
    while v >= 0x80:
      out.append((v & 0x7f) | 0x80)
      v >>= 7
    out.append(v)
    return bytes(out)
  out = bytearray()
  for b0 in range(0, len(raw), 262144):
    blk = raw[b0:b0 + 262144]
    body = bytearray(varint(len(blk)))
    for i in range(0, len(blk), 65536):
      lit = blk[i:i + 65536]
      l1 = len(lit) - 1
      if l1 < 60:
        body.append(l1 << 2)
      elif l1 < 256:
        body += bytes([60 << 2, l1])
      else:
        body += bytes([61 << 2, l1 & 0xff, l1 >> 8])
      body += lit
    out += len(body).to_bytes(4, "big") + body
  return bytes(out)


@pytest.mark.parametrize("n,ln", [(1, 5), (397, 660), (3000, 300), (900, 1171), (2, 300000)])
def test_writer_output_is_the_literal_only_block_stream(driver, tmp_path, n, ln):
  """Byte for byte: the writer hands whole blocks to writev() from the caller's buffer and tops
  up partial ones through its own — the file must not depend on how the bytes arrived."""
  path = tmp_path / "w"
  run(driver, "write", path, 1, n, ln)
  recs = [bytes([i & 0xff]) * (ln + i % 7) for i in range(n)]
  raw = b"".join(P.frame(r) for r in recs)
  assert path.read_bytes() == _literal_only_stream(raw)
  run(driver, "write", path, 0, n, ln)
  assert path.read_bytes() == raw
  # the save path's pattern: a few large buffers of framed records
  parts = 5
  raw = b"".join(P.frame(bytes([(p + j) & 0xff]) * (ln + j % 7)) for p in range(parts) for j in range(n))
  run(driver, "writeparts", path, 1, parts, n, ln)
  assert path.read_bytes() == _literal_only_stream(raw)
  run(driver, "writeparts", path, 0, parts, n, ln)
  assert path.read_bytes() == raw


def test_corruption_is_reported(driver, tmp_path):
  path = tmp_path / "c"
  run(driver, "write", path, 1, 50, 100)
  b = bytearray(path.read_bytes())
  b[40] ^= 0x55
  path.write_bytes(bytes(b))
  r = subprocess.run([driver, "read", str(path), "1"], capture_output=True, text=True)
  assert r.returncode == 1 and "ERROR" in r.stdout
  r = subprocess.run([driver, "readbatch", str(path), "1", "4096", "2"], capture_output=True, text=True)
  assert r.returncode == 1 and "ERROR" in r.stdout
  # a block whose varint promises more bytes than its elements deliver
  b = bytearray(path.read_bytes())
  b[40] ^= 0x55          # (undo)
  b[4] ^= 0x01           # uncompressed length of the first block
  path.write_bytes(bytes(b))
  for cmd in (["read", str(path), "1"], ["readbatch", str(path), "1", "4096", "2"]):
    r = subprocess.run([driver] + cmd, capture_output=True, text=True)
    assert r.returncode == 1 and "ERROR" in r.stdout


def test_save_pipeline_hands_chunks_over_in_order(driver):
  """run_pipeline3 (the save path's scan | encode | write): two buffer sets between neighbouring
  stages, every stage in chunk order; a failing stage stops the others and its error comes out."""
  for n in (0, 1, 2, 3, 64):
    assert run(driver, "pipeline", n, -1, 0) == "ok %d" % n
  for end in (0, 1, 2, 9, 40):        # a stage A that says where the stream ends (n: an upper bound)
    assert run(driver, "pipeline", 1000000, -1, 0, end) == "ok %d" % end
  for stage in (0, 1, 2):
    for chunk in (0, 1, 7, 31):
      r = subprocess.run([driver, "pipeline", "32", str(stage), str(chunk)], capture_output=True, text=True)
      assert r.returncode == 1 and "stage failed as asked" in r.stdout, (stage, chunk, r.stdout)


# ---- the reference's own TF-written files (tests/golden/tf_written, made by make_tf_written.py from
# model_export/testdata/saved_model/ps_N/.../assets/MonolithHashTable_*: MonolithHashTableSave's
# single-table layout, uncompressed TFRecord of EntryDump, hash_table_save_op.cc:147-160)
def _tf_written():
  import json
  d = os.path.join(ROOT, "tests", "golden", "tf_written")
  with open(os.path.join(d, "manifest.json")) as f:
    return d, json.load(f)


KIND_OF = {"sgd": SGD, "ftrl": FTRL, "adagrad": ADAGRAD}


@pytest.mark.parametrize("batch", [0, 1])
def test_tf_written_files_decode_and_reencode_byte_identically(driver, tmp_path, batch):
  """Every record TensorFlow wrote (150 across the four table layouts) goes through the C++ codec
  (framing check, crc, decode_entry into a row, encode_entry, framing) and comes out as the same
  bytes: the record codec and the TFRecord framing are pinned to files the reference holds."""
  d, manifest = _tf_written()
  total = 0
  for m in manifest:
    segs = []
    for kind, dim in m["segments"]:
      segs += [KIND_OF[kind], dim]
    files = [m["all_records_file"]] + ["%s-%05d-of-%05d" % (m["basename"], i, 4) for i in range(4)]
    for fn in files:
      src = os.path.join(d, fn)
      out = str(tmp_path / ("re_%d_%s" % (batch, fn)))
      got = run(driver, "recode", src, out, batch, m["dim"], len(m["segments"]), *segs).split()
      raw = open(src, "rb").read()
      assert open(out, "rb").read() == raw, fn
      # the protobuf runtime agrees on what was in there
      recs = P.unframe(raw)
      ids = 0
      for r in recs:
        e = P.EntryDump()
        e.ParseFromString(r)
        ids ^= e.id & 0xFFFFFFFFFFFFFFFF
        assert len(e.num) == m["dim"] and e.HasField("last_update_ts_sec")
      assert (int(got[0]), int(got[1])) == (len(recs), ids), fn
      if fn == m["all_records_file"]:
        assert len(recs) == m["all_records"]
        total += len(recs)
  assert total == 150
