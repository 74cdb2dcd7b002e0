#!/usr/bin/env python
"""bench.py — BASELINE.json's metric on MI355X: embedding lookups+updates/sec, 1B-id universe x
dim 64, Zipf(1.2), batch 65536, fused Adagrad (configs[2]); HBM-BW% through `roofline`.

One "step" = one pass of the sparse hot path over one batch of B ids already resident in HBM:
  dedup -> lookup(unique) -> scatter to B rows | duplicate-grad sum -> Adagrad apply(unique)
(the op sequence of native_training/distributed_ps.py:282-329 + :489-514).  value =
(B lookups + B updates) * steps * n_gpus / wall time, max over ranks, barrier + synchronize on both
sides.  With --gpus N > 1 (launched by torch.distributed.run) every rank feeds its own B ids and the
table is sharded by fid mod N with four all-to-alls per step over RCCL (weak scaling).

Contract: prints ONE JSON line on rank 0; a plain run sets up, warms up, times exactly --steps steps
and prints it.  --dump-outputs DIR writes the embeddings the last timed step returned.  With --full,
extra objects: `roofline` (dominant kernel, HIP-event timed on the launch stream), `cpu_baseline`
(reference map + AVX Adagrad built from the reference's own sources, oracle/_ref, timed on this box's
host cores; N=1 only), `parity_check`, and the other launch modes' windows.
"""
import argparse
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

# The HIP runtime keeps the kernel arguments of an EAGER launch in host memory unless told otherwise (the nodes
# of a hipGraph get theirs in device memory).  The step kernels take ~1.5 KB of arguments each and read them
# with scalar loads: over PCIe those reads made step_bwd 19.8 us instead of 15.7 in the event-timed pass and the
# eager C loop 46.8 us per step instead of 38.4 (profiles/r06/host_enqueue.md).  The runtime's own switch, set
# before it is loaded; a process that embeds the library (the TF shim of INTEGRATION.md) exports the same.  The
# graph-replayed headline does not depend on it.  An explicit setting of the caller wins.
os.environ.setdefault("HIP_FORCE_DEV_KERNARG", "1")

HBM_PEAK_GBPS = 8000.0  # MI355X HBM3E spec peak (MI355X_MICROARCH.md); ~6300 GB/s achievable copy
PROBE_BYTES = 72        # keys+tags of both candidate buckets
DUMP_LIMIT = 64 << 20   # --dump-outputs: bytes of all files together
RING = 1440             # distinct batches of a plain run at most (ring_size): a multiple of 60 = whole graph chunks
                        # of 10 steps and whole turns of the 2- and 3-slot dedup rotation (a replayed lap of graphs
                        # comes back to the state it was captured from)
RING_DLRM = 300         # the same for --config dlrm26 (26 tables: 13.6 MB of ids per step)


def parse():
  p = argparse.ArgumentParser()
  p.add_argument("--gpus", type=int, default=1)
  p.add_argument("--steps", type=int, default=200)
  p.add_argument("--warmup", type=int, default=20)
  p.add_argument("--batch", type=int, default=65536)
  p.add_argument("--dim", type=int, default=64)
  p.add_argument("--universe", type=float, default=1e9)
  p.add_argument("--resident-rows", type=float, default=float(1 << 27),
                 help="rows pre-inserted per GPU (the hottest ranks of this GPU's shard)")
  p.add_argument("--opt", default="adagrad", choices=["adagrad", "sgd"])
  p.add_argument("--config", default="configs2", choices=["configs2", "dlrm26"],
                 help="configs2 (default, the bench line): BASELINE.json configs[2]/[1] single table; "
                      "dlrm26: configs[4]'s shape on one GPU — 26 feature tables of dims 16/32/64, "
                      "batch ids per table and step, online insert + TTL eviction scans, all tables in "
                      "one launch pair per step (a measurement kept under profiles/, not the bench line)")
  p.add_argument("--tables", type=int, default=26, help="dlrm26: number of feature tables")
  p.add_argument("--dims", default="16,32,64", help="dlrm26: table dims, cycled over the tables")
  p.add_argument("--steps-per-second", type=int, default=2000,
                 help="dlrm26: update_time (seconds) advances once per this many steps — a ~0.43 ms "
                      "step is ~2 300 steps per wall-clock second; 1 = a new second every step (the "
                      "timestamp of every touched id changes every step)")
  p.add_argument("--evict-every", type=int, default=100,
                 help="dlrm26: TTL eviction scan of every table each N steps (0: never)")
  p.add_argument("--grad-pool", type=int, default=17,
                 help="gradient buffers rotated by the timed loop (17 x 16.8 MB > the 256 MiB "
                      "Infinity Cache: gradients are read from HBM, not from the LLC)")
  p.add_argument("--no-parity-check", action="store_true")
  p.add_argument("--dense", action="store_true",
                 help="dlrm26: the dense leg too — embeddings -> fused_embedding_to_layout (concat) -> "
                      "bf16 MLP 1024-512-256-1 on MFMA (hipBLASLt through torch) forward + backward + "
                      "SGD, layout gradient -> sparse update; the next batch's dedup runs on a side "
                      "stream beside the GEMMs")
  p.add_argument("--mlp", default="1024,512,256", help="hidden widths of the dense model")
  p.add_argument("--mlp-impl", default="mhte", choices=["mhte", "torch"],
                 help="--dense: the tower through mhte_dense_mlp_* (this repo's bf16 MFMA GEMMs, default) or "
                      "through torch / hipBLASLt (the A/B reference)")
  p.add_argument("--mlp-split", type=int, default=32,
                 help="dense model: weight gradients as a batched GEMM over this many slices of the "
                      "batch (0: torch.nn.Linear under autocast, one GEMM per gradient)")
  p.add_argument("--overlap", action="store_true",
                 help="sharded step: the next batch's dedup / numbering / id dispatch on the step's own "
                      "stream beside the dense leg (mhte_shard_step_set_overlap)")
  p.add_argument("--launch", default="auto", choices=["auto", "eager", "graph"])
  p.add_argument("--lookahead", type=int, default=1, choices=[1, 2],
                 help="batches of look-ahead handed to the step: 1 = the next batch (its run dedup rides in "
                      "the forward launch), 2 = the one after it as well (dedup in the backward launch: "
                      "measured slower on one table of 65 536 ids, DESIGN 4.4 — the backward launch has no "
                      "idle wave slots to hide it in)")
  p.add_argument("--no-cpu-baseline", action="store_true")
  p.add_argument("--no-extra-windows", action="store_true",
                 help="skip the eager_cpp (C-loop enqueue) and exact_order (bit-exact mode) windows that are "
                      "reported under timing_ms_per_step beside the line's own")
  p.add_argument("--cpu-steps", type=int, default=150)
  p.add_argument("--cpu-child", default="", help=argparse.SUPPRESS)   # "i" | "ii": one CPU-baseline
                                                                      # variant in a process of its own
  p.add_argument("--exact-order", action="store_true")
  p.add_argument("--ids-per-peer", type=int, default=0,
                 help="sharded step: id slots per (peer, table) block (0: library default)")
  p.add_argument("--force-sharded", action="store_true",
                 help="N=1 through the id-sharded code path (one-rank process group): the floor of "
                      "the multi-GPU step without any link traffic; a measurement, not the bench line")
  p.add_argument("--dist-backend", default="auto", choices=["auto", "nccl", "gloo", "ipc"],
                 help="torch.distributed backend of the launcher's side channel for --gpus > 1 (rendezvous, "
                      "barriers, the max-over-ranks reduction): auto = nccl (RCCL) with one device per "
                      "rank, gloo when ranks share a device (RCCL cannot place two ranks on one GPU); "
                      "ipc = gloo + --transport ipc")
  p.add_argument("--transport", default="auto", choices=["auto", "ipc", "rccl", "torch"],
                 help="the sharded step's exchanges: ipc = direct peer stores into hipIpc-mapped windows "
                      "(device-sized, works across xGMI and between ranks sharing a GPU); rccl = "
                      "ncclSend / ncclRecv groups; auto = ipc if every rank's self test passes, else "
                      "rccl; torch = round 1's torch.distributed form of the step (functional check)")
  p.add_argument("--trace-out", default="",
                 help="write a per-wavefront timeline (.npz) of three pipelined steps")
  p.add_argument("--no-stage-timing", action="store_true",
                 help="skip the per-kernel HIP-event pass (profiling the overlapped step only)")
  p.add_argument("--full", action="store_true",
                 help="everything beyond the headline as well: the other launch modes' windows (eager, eager_cpp, "
                      "exact_order, the 200-step reference window), the per-kernel HIP-event pass and roofline, "
                      "the parity check against the oracle and the CPU baseline (each still switched off by its "
                      "--no-* option).  Without it a run sets up, warms up, times --steps steps and prints the line")
  p.add_argument("--dump-outputs", default="", metavar="DIR",
                 help="after the timed steps, write the embeddings the last timed step's forward returned as "
                      "DIR/<name>.npy (float32; a fixed seeded sample of rows beyond %d MB in all)" % (DUMP_LIMIT >> 20))
  args = p.parse_args()
  if args.trace_out and not args.full:
    p.error("--trace-out rides in the per-kernel pass: it needs --full")
  if not args.full:
    args.no_cpu_baseline = args.no_extra_windows = args.no_parity_check = args.no_stage_timing = True
  return args


def algorithmic_bytes(B, U, D, S):
  """SURVEY.md §8d / BASELINE.md §3 per step; and per kernel."""
  P = PROBE_BYTES
  lookup = 8 * B + P * U + 4 * D * U + 4 * D * B
  update = 8 * B + 4 * D * B + P * U + (8 * D + 8 * S) * U + 4 * U
  per_kernel = {
      # one probe+gather launch over the B occurrences: distinct buckets and rows are fetched from
      # HBM once (duplicates hit L2) == SURVEY's bytes_lookup
      "lookup_kernel": lookup,
      # fused backward launch (gradient sum + upsert + optimizer) == SURVEY's bytes_update
      "sum_apply_kernel": update,
  }
  return lookup + update, per_kernel


_JSON_FD = None


def stdout_for_the_line_only():
  """Everything else a rank writes to stdout goes to stderr from here on: native libraries print
  there (RCCL's version block when a communicator is made, gloo's "[Gloo] Rank 0 is connected to …"
  at the rendezvous), and the contract is ONE JSON line on stdout."""
  global _JSON_FD
  flush_native_stdout()
  _JSON_FD = os.dup(1)
  os.dup2(2, 1)


def emit_line(obj):
  """The bench's ONE JSON line, the only thing on stdout (stdout_for_the_line_only)."""
  flush_native_stdout()
  data = (json.dumps(obj) + "\n").encode()
  if _JSON_FD is None:
    sys.stdout.write(data.decode())
    sys.stdout.flush()
  else:
    os.write(_JSON_FD, data)


def flush_native_stdout():
  import ctypes
  try:
    ctypes.CDLL(None).fflush(None)
  except OSError:
    pass
  sys.stdout.flush()


def spawn_ranks(n):
  """`python bench.py --gpus N` without a launcher: run the N ranks under torch.distributed.run
  (one process per rank, rendezvous on 127.0.0.1) and pass their output through — rank 0's JSON line
  stays the last line of stdout.  On a box with fewer than N GPUs the ranks share devices and the
  exchanges go through the peer-store transport."""
  import socket
  import subprocess
  s = socket.socket()
  s.bind(("127.0.0.1", 0))
  port = s.getsockname()[1]
  s.close()
  cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(n),
         "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
  env = dict(os.environ)
  env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
  env.setdefault("OMP_NUM_THREADS", "8")
  flush_native_stdout()
  rc = subprocess.call(cmd, env=env)
  if rc:
    raise SystemExit(rc)


def peer_unique_max(ids_host, world):
  """Largest number of distinct ids one batch of `ids_host` [steps, B] sends to one owner
  (owner = id mod world, NT/distributed_ps.py:289)."""
  mx = 0
  for row in ids_host:
    u = np.unique(row)
    mx = max(mx, int(np.bincount(np.mod(u, world).astype(np.int64), minlength=world).max()))
  return mx


def sharded_algorithmic_bytes(B, U, D, S):
  """Per launch of the id-sharded step (csrc/mhte_shard_kernels.h), world 1, one table: the rows of
  the U distinct ids cross a peer block in each direction on top of SURVEY 8d's per-step bytes."""
  P = PROBE_BYTES
  return {
      "shard_lookup_kernel": 8 * U + P * U + 4 * D * U + 4 * D * U,      # ids, probes, rows -> block
      "shard_scatter_kernel": 4 * U + 4 * D * U + 4 * D * B,             # slots, block -> occurrences
      "shard_build_kernel": 4 * D * B + 4 * U + 4 * D * U + 8 * U,       # gradient sums -> block; ids -> block
      "shard_upsert_kernel": 8 * U + 4 * D * U + P * U + (8 * D + 8 * S) * U + 4 * U,
      "dd_kernels": 8 * B,
  }


def pmc_traffic(kernel):
  """HBM bytes per launch of `kernel` from the committed PMC passes (profiles/pmc_traffic.json,
  written by scripts/pmc_traffic.py from separate `rocprofv3 --pmc FETCH_SIZE` / `--pmc WRITE_SIZE`
  runs of this same command; corrections as MI355X_MICROARCH.md prescribes, see that file's
  "method").  bench.py cannot collect counters itself; null when no summary is committed."""
  path = os.path.join(ROOT, "profiles", "pmc_traffic.json")
  try:
    with open(path) as f:
      d = json.load(f)
    k = d["kernels"][kernel]
    return int(k["hbm_bytes_per_launch"]), "profiles/pmc_traffic.json (%s)" % d.get("source", "")
  except Exception:  # pylint: disable=broad-except
    return None, None


def oracle_subset_rows(probe, D, opt, lr, applied, ids_of, grads_of):
  """Rows of the `probe` ids after the update sequence `applied` = [(batch, grad buffer, time)],
  by the CPU oracle restricted to those ids (a row depends on its own id's gradient history only):
  per step first-occurrence dedup, duplicate gradients added in occurrence order, one optimizer
  step — the reference's sequence (unique_mapping_ops.cc:284-329 + multi_hash_table_update_op.cc
  :47-100).  The checker of `parity_check`, never the thing measured."""
  import oracle as O
  seg = O.segment(D, O.OPT_ADAGRAD if opt == "adagrad" else O.OPT_SGD, p=(0.1, 0.0))
  ot = O.Table(seg, 1)
  ps = np.sort(probe)
  for (b, g, t) in applied:
    ids = ids_of(b)
    m = np.isin(ids, ps)
    sub = ids[m]
    if not sub.size:
      continue
    gr = grads_of(g)[m]
    uk, _, vo, vos, _ = O.unique_key_with_value_and_offset(sub, [0, sub.size], [D])
    gu = O.fill_with_offset_map_gradient(np.arange(uk.size), [0, uk.size], gr.ravel(), vo, vos,
                                         [D]).reshape(-1, D)
    ot.optimize(uk, gu, [lr], t)
  return ot.lookup(probe)[0]


def parity_numbers(got, exp):
  diff = np.abs(got.astype(np.float64) - exp.astype(np.float64))
  den = np.maximum(np.abs(exp.astype(np.float64)), 1e-30)
  big = np.abs(exp) > 1e-6
  return {"n": int(got.shape[0]), "max_abs": float(diff.max()) if diff.size else 0.0,
          "max_rel": float((diff[big] / den[big]).max()) if big.any() else 0.0,
          "rows_bit_exact": int((got == exp).all(axis=1).sum()),
          "rel_floor": 1e-6}


def ring_size(n_batches, K, full, ring):
  """Distinct batches of the stream (step s trains batch s mod P).  --full keeps every batch fresh, as each of
  its passes assumes, unless --steps alone passes the ring; a plain run needs n_batches for its own steps only,
  and beyond `ring` its batches come round again (the set-up does not grow with --steps)."""
  return n_batches if (full and K <= ring) else min(n_batches, ring)


def ring_stretches(lo, hi, P):
  """Steps [lo, hi) of a ring of P batches for a loop that reads batch b + 1 ahead of batch b within the ring
  (the C loop, csrc/eager_loop.c): [(first batch, steps)] stretches that end one step short of the ring's end,
  and (batch P - 1, None) for the step whose next batch is the ring's first, enqueued one by one."""
  out, s = [], lo
  while s < hi:
    b = s % P
    e = min(hi, s + (P - 1 - b))
    if e > s:
      out.append((b, e - s))
    if e < hi:
      out.append((e % P, None))
      e += 1
    s = e
  return out


def repeated_steps(lo, hi, P):
  """Steps of [lo, hi) that train a batch an earlier step of the run trained (s >= P)."""
  return max(0, hi - max(lo, P))


def take_outputs(arrays, limit=DUMP_LIMIT):
  """--dump-outputs: host float32 copies of `arrays` ({name: device tensor, rows first}) taken right after the
  timed window, before anything else overwrites the buffers.  Beyond `limit` bytes in all, every array keeps
  the same fraction of its rows, chosen by a fixed seed: the sample depends on the shapes only."""
  import torch
  total = sum(4 * t.numel() for t in arrays.values())
  out = {}
  for name, t in arrays.items():
    if total > limit:
      n = t.shape[0]
      keep = max(1, int(n * (limit / total)))
      rows = np.sort(np.random.default_rng(0).choice(n, keep, replace=False))
      t = t.index_select(0, torch.from_numpy(rows).to(t.device))
    out[name] = t.float().cpu().numpy()
  return out


def write_outputs(d, outs):
  os.makedirs(d, exist_ok=True)
  for name, a in outs.items():
    np.save(os.path.join(d, name + ".npy"), a)


def main_dlrm(args):
  """BASELINE.json configs[4]'s shape on ONE MI355X (the 8-GPU sharding of it is the driver's
  --gpus run of the default config): T feature tables of dims 16 / 32 / 64 (fused Adagrad), B
  Zipf(1.2) ids per table and step, ids inserted online, a TTL eviction scan of every table each
  --evict-every steps — lookups and updates of ALL tables in one launch pair per step
  (mhte_multi_step_forward / _backward)."""
  import torch
  assert torch.cuda.is_available(), "bench.py needs an MI355X (no CPU fallback)"
  torch.cuda.set_device(0)
  dev = torch.device("cuda", 0)
  from monolith_amd import _lib, entry, synthetic as S
  from monolith_amd.fused_step import MultiSparseStep
  from monolith_amd.multi_hash_table_ops import MultiHashTable, Ragged

  T, B = args.tables, args.batch
  K, W = args.steps, args.warmup
  V = int(args.universe) // T                      # ids per feature
  resident = min(int(args.resident_rows) // T, V)  # prefilled rows per table
  dcyc = [int(x) for x in args.dims.split(",")]
  dims = [dcyc[i % len(dcyc)] for i in range(T)]
  names = ["f%02d" % (i + 1) for i in range(T)]    # sorted order == slot order
  reps = min(K, 50) if not args.no_stage_timing else 0
  n_steps = W + K + reps + 4
  P = ring_size(n_steps + 1, K, args.full, RING_DLRM)   # distinct ragged batches: step s trains batch s mod P
  lr = 0.001
  configs = {}
  for i, n in enumerate(names):
    rows_cap = resident + P * 24000 + (1 << 16)   # ~13 k distinct ids per batch, < 40 % new
    slots = 4
    while slots * 0.5 < rows_cap:
      slots *= 2
    configs[n] = entry.make_table_config(
        [entry.CombineAsSegment(dims[i], entry.ZerosInitializer(), entry.AdagradOptimizer(lr, 0.1))],
        entry.CuckooHashTableConfig(initial_capacity=slots, reserve_rows=rows_cap))
  mt = MultiHashTable.from_configs(configs, name_suffix="dlrm")
  splits0 = np.zeros(T + 1, dtype=np.int64)

  # ---- prefill: the `resident` hottest ranks of every feature, rows = initializer ----
  t0 = time.time()
  mult = torch.tensor(0x9E3779B97F4A7C15 - (1 << 64), dtype=torch.int64, device=dev)
  chunk = 1 << 21
  for i, n in enumerate(names):
    zeros = torch.zeros((chunk, dims[i]), dtype=torch.float32, device=dev)
    for r0 in range(1, resident + 1, chunk):
      m = min(chunk, resident + 1 - r0)
      ranks = torch.arange(r0, r0 + m, dtype=torch.int64, device=dev)
      fid = ((ranks * mult) & ((1 << 48) - 1)) | ((i + 1) << 48)
      sp = splits0.copy()
      sp[i + 1:] = m
      _lib.check(mt._lib.mhte_assign(mt.handle, _lib.vp(fid), sp.ctypes.data_as(_lib.C.POINTER(_lib.C.c_int64)),
                                     _lib.C.c_int64(T + 1), _lib.vp(zeros), _lib.C.c_int64(m * dims[i]),
                                     _lib.C.c_int64(S.update_time(0) - 3600),   # (last touched an hour ago)
                                     _lib.C.c_int32(_lib.MHTE_IDS_UNIQUE), None))
    torch.cuda.synchronize()
    del zeros
  torch.cuda.empty_cache()
  prefill_s = time.time() - t0
  size0 = [mt.size(n) for n in names]

  # ---- inputs resident in HBM: one ragged batch per step (tables in slot order), two gradient
  # buffers of sum(B * dim) floats each (2 x 247 MB at 26 tables: beyond the 256 MiB LLC)
  splits = np.arange(T + 1, dtype=np.int64) * B
  ids_host = np.empty((P, T * B), dtype=np.int64)

  def fill(s):
    for i in range(T):
      ids_host[s, i * B:(i + 1) * B] = S.id_batch(s * 64 + i + 1, B, V, "zipf", feature_slot=i + 1)
  with ThreadPoolExecutor(min(16, os.cpu_count() or 1)) as ex:
    list(ex.map(fill, range(P)))
  ids_all = torch.from_numpy(ids_host).to(dev)
  rag = [Ragged(ids_all[s], splits) for s in range(P)]
  gsz = B * sum(dims)
  goff = np.concatenate([[0], np.cumsum([B * d for d in dims])])

  def grad_host(g):
    rng = np.random.Generator(np.random.PCG64(S.SEED0 + 10**9 + g))
    return rng.standard_normal(gsz, dtype=np.float32) * np.float32(0.01)

  NG = 2
  grad_pool = [torch.from_numpy(grad_host(g)).to(dev) for g in range(NG)]
  out = torch.empty(gsz, dtype=torch.float32, device=dev)
  if args.dense:
    os.environ.setdefault("MHTE_MSTEP_SIDE", "1")   # dedup of the next batch beside the GEMMs
  sharded = bool(args.force_sharded)
  if sharded:
    # every table through the id-sharded step with one rank: the floor of the multi-GPU step
    from monolith_amd.distributed_ps_sync import ShardedMultiStep
    # (overlap is a creation-time choice: with the peer-store transport the wire mode is part of what the
    # ranks agree on at connect, and the direct-store form refuses a change behind it)
    step = ShardedMultiStep(mt, B, ids_per_peer_table=args.ids_per_peer,
                            transport="ipc" if args.transport == "ipc" else "auto",
                            overlap=True if args.overlap else None)
  else:
    step = MultiSparseStep(mt, B, exact_order=args.exact_order)
  applied = []
  evictions = [0]
  sps = max(1, int(args.steps_per_second))

  def ut(step):   # update_time of a step: wall-clock seconds
    return S.update_time(step // sps)

  # ---- dense leg: layout (concat of the T features' rows) -> MLP -> layout gradient -------------
  dense = None
  if args.dense:
    from monolith_amd import distribution_ops as DO
    feats = {n: DO.FeatureConfig(n, DO.PoolingType.SUM, [dims[i]]) for i, n in enumerate(names)}
    kin = (sum(dims) + 127) // 128 * 128     # GEMM K padded to a multiple of 128 (zero columns)
    concat = DO.OutConfig([DO.SliceConfig(n, 0, dims[i]) for i, n in enumerate(names)], DO.OutType.CONCAT,
                          [[-1, kin]])
    lcfg = DO.FeatureConfigs(feats, {"concat": concat})
    # one id per feature and sample: fid (t, b) is row b of matrix t (the per-occurrence rows of the
    # step's forward), feature instance t * B + b, named feature list t
    fo = (torch.arange(T, dtype=torch.int64, device=dev).repeat_interleave(B) << 32) | \
         torch.arange(B, dtype=torch.int64, device=dev).repeat(T)
    fe = torch.arange(T * B, dtype=torch.int32, device=dev)
    nf = (torch.arange(T, dtype=torch.int32, device=dev) * B)
    widths = [kin] + [int(w) for w in args.mlp.split(",")] + [1]

    class SplitKLinearFn(torch.autograd.Function):
      """y = x w^T + b in bf16 on MFMA (hipBLASLt through torch).  The weight gradient dW = dy^T x has a
      small output (out x in) and a 65 536-long reduction: as ONE GEMM hipBLASLt launches 25-97
      workgroups on 256 CUs (rocprofv3: 248-357 us per layer, 0.15 of the bf16 peak).  Split along the
      batch into `split` partial products (a batched GEMM: split x (out/256) x (in/256) tiles) and
      summed in fp32, the same arithmetic fills the chip."""

      @staticmethod
      def forward(ctx, x, w, b, split):
        ctx.save_for_backward(x, w)
        ctx.split = split
        return torch.addmm(b, x, w.t())

      @staticmethod
      def backward(ctx, dy):
        x, w = ctx.saved_tensors
        dy = dy.contiguous()
        dx = dy @ w
        M, S = x.shape[0], ctx.split
        if S > 1 and M % S == 0:
          dw = torch.bmm(dy.view(S, M // S, -1).transpose(1, 2), x.view(S, M // S, -1)).float().sum(0)
        else:
          dw = (dy.t() @ x).float()
        return dx, dw, dy.float().sum(0), None

    class Mlp(torch.nn.Module):
      def __init__(self, split):
        super().__init__()
        self.split = split
        self.w = torch.nn.ParameterList()
        self.b = torch.nn.ParameterList()
        for a, b_ in zip(widths[:-1], widths[1:]):
          lin = torch.nn.Linear(a, b_)
          self.w.append(lin.weight)
          self.b.append(lin.bias)

      def forward(self, x):
        h = x.to(torch.bfloat16)
        for i, (w, b) in enumerate(zip(self.w, self.b)):
          h = SplitKLinearFn.apply(h, w.to(torch.bfloat16), b.to(torch.bfloat16),
                                   self.split if w.shape[0] > 1 else 1)
          if i + 1 < len(self.w):
            h = torch.relu(h)
        return h

    dmlp = None
    if args.mlp_impl == "mhte":
      from monolith_amd.dense_mlp import DenseMlp
      dmlp = DenseMlp(widths, max_batch=B)
      for i, (a, b_) in enumerate(zip(widths[:-1], widths[1:])):
        lin = torch.nn.Linear(a, b_)      # (the same initialisation as the torch form)
        dmlp.set_params(i, lin.weight, lin.bias)
      mlp = None
    elif args.mlp_split > 0:
      mlp = Mlp(args.mlp_split).to(dev)
    else:
      layers = []
      for a, b_ in zip(widths[:-1], widths[1:]):
        layers += [torch.nn.Linear(a, b_), torch.nn.ReLU()]
      mlp = torch.nn.Sequential(*layers[:-1]).to(dev)
    opt = torch.optim.SGD(mlp.parameters(), lr=1e-3) if mlp is not None else None
    eoff = np.concatenate([[0], np.cumsum([B * d for d in dims])])
    dense = {"flops_per_step": 6 * B * sum(a * b_ for a, b_ in zip(widths[:-1], widths[1:])), "widths": widths}

    gflat = torch.empty(gsz, dtype=torch.float32, device=dev)
    gviews = [gflat[eoff[i]:eoff[i + 1]].view(B, dims[i]) for i in range(T)]

    ybuf = torch.empty(B, dtype=torch.float32, device=dev)
    dxbuf = torch.empty(B, kin, dtype=torch.float32, device=dev)
    dy_mean = torch.full((B,), 1.0 / B, dtype=torch.float32, device=dev)   # loss = mean of the logits

    def mlp_step(x):
      """forward + backward + SGD of the tower; -> gradient of the loss at x"""
      if dmlp is not None:
        dmlp.forward(x, out=ybuf)
        return dmlp.backward(dy_mean, 1e-3, out=dxbuf)
      x.requires_grad_(True)
      x.grad = None
      if args.mlp_split > 0:
        y = mlp(x)
      else:
        with torch.autocast("cuda", dtype=torch.bfloat16):
          y = mlp(x)
      loss = y.float().mean()
      opt.zero_grad(set_to_none=True)
      loss.backward()
      opt.step()
      return x.grad

    def dense_step(emb_flat):
      embs = [emb_flat[eoff[i]:eoff[i + 1]].view(B, dims[i]) for i in range(T)]
      x = DO.fused_embedding_to_layout(embs, fo, fe, nf, B, lcfg, one_fid_unique_rows=True)[0]
      dx = mlp_step(x)
      DO.fused_embedding_to_layout_grad(embs, fo, fe, nf, B, [dx], lcfg, one_fid_unique_rows=True,
                                        out=gviews)
      return gflat

  def run(lo, hi):
    for s in range(lo, hi):
      b = s % P
      step.forward(rag[b], rag[(s + 1) % P], out=out)
      if dense is not None:
        step.backward(dense_step(out), ut(s))
      else:
        step.backward(grad_pool[b % NG], ut(s))
        applied.append((b, b % NG, ut(s)))
      if args.evict_every and (s + 1) % args.evict_every == 0:
        for n in names:
          mt.evict(n)
        evictions[0] += 1

  import gc
  run(0, W)
  torch.cuda.synchronize()
  evictions[0] = 0
  gc.collect()
  gc.disable()   # (a generation-2 pass of the interpreter inside the timed region is ~40 ms)
  t = time.perf_counter()
  run(W, W + K)
  torch.cuda.synchronize()
  elapsed = time.perf_counter() - t
  gc.enable()
  if args.dump_outputs:   # the step's flat output, one view per table
    outputs = take_outputs({"embeddings_" + n: out[goff[i]:goff[i + 1]].view(B, dims[i])
                            for i, n in enumerate(names)})

  # ---- per-kernel timing: HIP events with the kernels' own begin/end (mhte_profile_arm) ----
  # (--full: a pass of its own behind the timed region)
  roofline, stages, U = None, {}, None
  if reps:
    acc, uniq = {}, []
    _lib.profile_arm(8 * reps)
    for s in range(W + K, W + K + reps):
      b = s % P
      step.forward(rag[b], rag[(s + 1) % P], out=out)
      if s % 10 == 0:
        uniq.append(step.unique_counts())
      if dense is not None:
        step.backward(dense_step(out), ut(s))
      else:
        step.backward(grad_pool[b % NG], ut(s))
        applied.append((b, b % NG, ut(s)))
    torch.cuda.synchronize()
    for name, us in _lib.profile_read():
      a = acc.setdefault(name, [0, 0.0])
      a[0] += 1
      a[1] += us
    U = np.mean(np.stack(uniq), axis=0)              # distinct ids per table and batch
    alg_fwd = alg_bwd = 0
    for i in range(T):
      _, pk = algorithmic_bytes(B, float(U[i]), dims[i], dims[i])
      alg_fwd += pk["lookup_kernel"]
      alg_bwd += pk["sum_apply_kernel"]
    alg = {"mstep_fwd_kernel": alg_fwd, "mstep_bwd_kernel": alg_bwd}
    if sharded:
      alg = {}
      for i in range(T):
        for k, v in sharded_algorithmic_bytes(B, float(U[i]), dims[i], dims[i]).items():
          alg[k] = alg.get(k, 0) + v
      alg.pop("dd_kernels")
    stages = {}
    for name, (cnt, tot) in sorted(acc.items()):
      stages[name] = {"avg_us": round(tot / cnt, 2), "launches_per_step": round(cnt / reps, 2)}
      if name in alg:
        stages[name]["alg_bytes"] = int(alg[name])
        stages[name]["GBps"] = round(alg[name] / (tot / cnt) / 1e3, 1)
    dom = max((k for k in stages if k in alg), key=lambda k: stages[k]["avg_us"])
    a_gbps = alg[dom] / stages[dom]["avg_us"] / 1e3
    step_bytes = alg_fwd + alg_bwd
    # (the committed PMC passes are of the default 26 x 65 536 shape)
    traffic, traffic_src = pmc_traffic(dom) if (T == 26 and B == 65536 and not sharded) else (None, None)
    roofline = {"bound": "hbm", "kernel": dom, "achieved": round(a_gbps, 1), "peak": HBM_PEAK_GBPS,
                "unit": "GB/s", "frac": round(a_gbps / HBM_PEAK_GBPS, 4), "traffic": traffic,
                "traffic_source": traffic_src,
                "alg_bytes_per_launch": int(alg[dom]), "avg_launch_us": stages[dom]["avg_us"],
                "timing": "hipExtLaunchKernelGGL start/stop events on the launch stream, %d launches" % reps,
                "step_alg_bytes": int(step_bytes),
                "step_GBps": round(step_bytes / (elapsed / K) / 1e9, 1),
                "step_frac": round(step_bytes / (elapsed / K) / 1e9 / HBM_PEAK_GBPS, 4)}

  # ---- parity of the benched state against the oracle's replay, three tables (one per dim) ----
  parity = None
  if dense is not None and args.full:
    # the dense leg alone, timed with events on its stream: MFMA roofline of the GEMMs
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(10):
      dense_step(out)
    e1.record()
    torch.cuda.synchronize()
    d_us = e0.elapsed_time(e1) * 1e3 / 10
    xin = torch.randn(B, kin, device=dev)
    for _ in range(3):
      mlp_step(xin)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(10):
      mlp_step(xin)
    e1.record()
    torch.cuda.synchronize()
    m_us = e0.elapsed_time(e1) * 1e3 / 10
    dense.update({"dense_leg_us": round(d_us, 1), "mlp_us": round(m_us, 1),
                  "layout_fwd_bwd_us": round(d_us - m_us, 1),
                  "roofline": {"bound": "mfma", "achieved": round(dense["flops_per_step"] / m_us / 1e6, 1),
                               "peak": 2500.0, "unit": "TFLOP/s",
                               "frac": round(dense["flops_per_step"] / m_us / 1e6 / 2500.0, 4)},
                  "mlp_impl": ("mhte_dense_mlp_* (hand-written bf16 MFMA GEMMs, csrc/mhte_gemm_kernels.h)"
                               if dmlp is not None else "torch / hipBLASLt"),
                  "note": "mlp_us: bf16 MLP forward + backward + SGD incl. its casts, transposes and "
                          "elementwise kernels; flops = 6 * batch * sum(in * out); dense_leg_us adds the "
                          "layout kernels either side"})
  if not args.no_parity_check and dense is None:
    try:
      t0p = time.time()
      parity = {}
      last = applied[-1][0]
      gcache = {}

      def grads_flat(g):
        if g not in gcache:
          gcache[g] = grad_host(g)
        return gcache[g]

      for i in (0, 1, 2):
        sl = slice(i * B, (i + 1) * B)
        probe = np.unique(ids_host[last, sl])
        exp = oracle_subset_rows(
            probe, dims[i], "adagrad", lr, applied, lambda b, sl=sl: ids_host[b, sl],
            lambda g, i=i: grads_flat(g)[goff[i]:goff[i + 1]].reshape(B, dims[i]))
        got = mt.lookup({names[i]: torch.from_numpy(probe).to(dev)})[names[i]].cpu().numpy()
        parity[names[i]] = parity_numbers(got, exp)
      parity["updates_replayed"] = len(applied)
      parity["seconds"] = round(time.time() - t0p, 1)
    except Exception as e:  # pylint: disable=broad-except
      parity = {"failed": repr(e)[:300]}

  # ---- CPU baseline: the reference map + AVX Adagrad (oracle/_ref), one table per dim class ----
  cpu = None
  if not args.no_cpu_baseline:
    try:
      import oracle as O
      cores = os.cpu_count() or 1
      avx = O.ref_available(True)
      per_dim = {}
      for d in (16, 32, 64):
        i = dims.index(d)
        ps = O.RefPs(cores, d, O.OPT_ADAGRAD, 0.1, 0.0, 0.0, 1, avx=avx)
        gh = grad_host(0)[goff[i]:goff[i + 1]].reshape(B, d)
        times = []
        for s in range(5 + 30):
          tt = time.perf_counter()
          ps.step(ids_host[s % P, i * B:(i + 1) * B], gh, lr, ut(s), want_emb=True)
          times.append(time.perf_counter() - tt)
        per_dim[d] = float(np.median(times[5:]))
      t_step = sum(per_dim[d] for d in dims)
      cpu = {"value": round(2 * B * T / t_step, 1), "unit": "lookups+updates/s", "cores": cores,
             "kind": "reference",
             "sample": "30 steps (after 5) of one table per dim class (16/32/64: %.2f / %.2f / %.2f ms "
                       "median), tables grown from empty, summed over the %d tables as the reference's "
                       "loop over tables would run them; PS-style %d single-threaded shards of the "
                       "reference cuckoohash_map + %s Adagrad" %
                       (per_dim[16] * 1e3, per_dim[32] * 1e3, per_dim[64] * 1e3, T, cores,
                        "AVX2" if avx else "scalar")}
    except Exception as e:  # pylint: disable=broad-except
      cpu = {"value": None, "unit": "lookups+updates/s", "cores": os.cpu_count(), "kind": "reference",
             "sample": "failed: %r" % (e,)}

  size1 = [mt.size(n) for n in names]
  value = 2.0 * B * T * K / elapsed
  out_json = {
      "metric": "embedding lookups+updates/sec, %d-feature multi-table step, Zipf(1.2) batch=%d per feature" % (T, B),
      "value": round(value, 1), "unit": "lookups+updates/s", "n_gpus": 1, "steps": K, "warmup": W,
      "ms_per_step": round(elapsed / K * 1e3, 5), "steps_per_sec": round(K / elapsed, 1),
      "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": "f32",
      "data": "synthetic",
      "config": {
          "workload": "configs[4] shape on 1 MI355X: %d feature tables, dims 16/32/64, fused Adagrad, "
                      "Zipf(1.2) over %d ids per feature, batch %d ids per feature and step, online "
                      "insert, TTL eviction scan every %d steps; %s" %
                      (T, V, B, args.evict_every,
                       ("end to end with the dense model (layout + bf16 MLP)" if dense is not None else
                        "sparse path only (no dense model)") +
                       ("; through the id-sharded step with one rank (%s)" % step.info()["transport"]
                        if sharded else "")),
          "tables": T, "dims": dims, "batch_per_table": B, "universe_per_table": V,
          "resident_rows_start": int(sum(size0)), "resident_rows_end": int(sum(size1)),
          "unique_ids_per_batch_mean": None if U is None else float(U.mean()),
          "eviction_scans_in_timed_region": evictions[0], "distinct_batches": P,
          "timed_steps_on_repeated_batches": repeated_steps(W, W + K, P),
          "gradient_bytes_rotated": int(NG * gsz * 4), "prefill_s": round(prefill_s, 2),
          "update_time": "one second per %d steps" % sps,
          "launch": "eager",
          "overlap": bool(args.overlap and sharded),
          "shard_step": step.info() if sharded else None,
      },
      "roofline": roofline, "stages": stages, "cpu_baseline": cpu, "parity_check": parity,
      "dense": dense,
  }
  if cpu and cpu.get("value"):
    out_json["vs_cpu_baseline"] = round(value / cpu["value"], 2)
  if args.dump_outputs:
    write_outputs(args.dump_outputs, outputs)
  emit_line(out_json)


def cpu_child(args):
  """One CPU-baseline variant on this box's host cores; prints one JSON line."""
  import oracle as O
  from monolith_amd import synthetic as S
  B, D, V = args.batch, args.dim, int(args.universe)
  cores = os.cpu_count() or 1
  opt = O.OPT_ADAGRAD if args.opt == "adagrad" else O.OPT_SGD
  avx = O.ref_available(True)
  lr = 0.001 if args.opt == "adagrad" else 0.01
  cw, ck = 20, args.cpu_steps    # (>= 20 warm-up steps, median of >= 100)
  grads_h = [S.grad_batch(s, B, D) for s in range(4)]
  # Variant (ii) starts its ONE shared map at 2^18 slots (65 536 buckets = the reference map's
  # kMaxNumLocks), not at the proto default of 1: below that size the reference's cuckoo_fast_double
  # replaces the locks array at every doubling, and `old_buckets_.swap(buckets_)`
  # (cuckoohash_map.hpp:1814-1815) lets a thread that slept through a doubling pass check_hashpower
  # against a null bucket pointer — round 4's rc -11: 2 of 12 runs with 256 threads on the GPU box,
  # all in the first step (oracle/stress/shared_map_stress.cc, profiles/r05/cpu_baseline_rc11.md).
  # The per-thread shards of variant (i) have one thread per map and keep the default.
  shared = args.cpu_child == "ii"
  ps = O.RefPs(cores, D, opt, 0.1, 0.0, 0.0, (1 << 18) if shared else 1, avx=avx, shared=shared)
  times, phases = [], []
  for s in range(cw + ck):
    ids = S.id_batch(s, B, V, "zipf")
    t = time.perf_counter()
    ps.step(ids, grads_h[s % 4], lr, S.update_time(s), want_emb=True)
    times.append(time.perf_counter() - t)
    phases.append(ps.breakdown())
  med = float(np.median(times[cw:]))
  print(json.dumps({"value": round(2 * B / med, 1), "median_step_ms": round(med * 1e3, 3), "steps": ck,
                    "rows_at_end": ps.size(), "cores": cores, "avx": bool(avx),
                    "initial_capacity": (1 << 18) if shared else 1,
                    "phase_ms_median": {k: round(float(np.median([p_[k] for p_ in phases[cw:]])) * 1e3, 3)
                                        for k in O.RefPs.PHASES}}))


def main():
  args = parse()
  if args.cpu_child:
    return cpu_child(args)
  if args.config == "dlrm26":
    return main_dlrm(args)
  import torch
  import torch.distributed as dist
  world = int(os.environ.get("WORLD_SIZE", "1"))
  rank = int(os.environ.get("RANK", "0"))
  local_rank = int(os.environ.get("LOCAL_RANK", "0"))
  if args.gpus != world and world == 1 and args.gpus > 1:
    return spawn_ranks(args.gpus)   # `python bench.py --gpus N`: launch the N ranks ourselves
  assert torch.cuda.is_available(), "bench.py needs MI355X GPUs (no CPU fallback)"
  stdout_for_the_line_only()
  ndev = torch.cuda.device_count()
  shared_device = world > ndev        # several ranks per GPU (the 1-GPU box)
  local_rank %= ndev
  torch.cuda.set_device(local_rank)
  dev = torch.device("cuda", local_rank)
  sharded = world > 1 or args.force_sharded
  if args.dist_backend == "ipc":
    args.dist_backend, args.transport = "gloo", "ipc"
  if args.dist_backend == "auto":
    args.dist_backend = "gloo" if shared_device else "nccl"
  if shared_device and args.transport == "auto":
    args.transport = "ipc"            # (RCCL refuses two ranks on one device)
  if shared_device:
    args.resident_rows = args.resident_rows / -(-world // ndev)   # the ranks of a device share its HBM
  if world > 1:   # (one rank needs no rendezvous: the sharded step's exchange is the identity)
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ.setdefault("MASTER_PORT", "29533")
    dist.init_process_group(args.dist_backend, rank=rank, world_size=world)

  from monolith_amd import _lib, entry, synthetic as S
  from monolith_amd.fused_step import SparseStep
  from monolith_amd.multi_hash_table_ops import MultiHashTable

  B, D = args.batch, args.dim
  V = int(args.universe) * world  # weak scaling: 1B-id universe per GPU
  K, W = args.steps, args.warmup
  S_state = D if args.opt == "adagrad" else 0
  resident = int(args.resident_rows)

  # ---- inputs resident in HBM before the timed region ----
  # Every launch mode trains FRESH batches (a replay of batches the table has already seen would
  # find every id resident and skip the insert path).  The modes run back to back over one
  # contiguous batch sequence: the last step of a mode deduplicates the first batch of the next
  # mode ahead, exactly as it does inside a mode.  The sequence is a ring of P batches (ring_size):
  # step s trains batch s mod P with gradient buffer (s mod P) mod NG at update_time(s mod P).  --full
  # gets a fresh batch for every step unless --steps alone passes RING; a plain run's batches come
  # round again beyond RING, so that its set-up does not grow with --steps, and the line says how
  # many timed steps trained a repeated batch.
  # launches of the per-kernel timing pass (HIP events): 100 whatever --steps is — the first launches
  # after the queue has drained run slower (the driver's 20-step window averaged 17.9 us for a kernel
  # that takes 15.5-16 us in steady state), so the pass also warms up before it arms the events
  reps = 100
  PROF_WARM = 8
  gchunk = 10                               # steps per captured graph
  Wg = -(-W // gchunk) * gchunk             # the graph mode's warm-up: W rounded up to whole chunks
  # a short --steps window (the driver's 20 steps are 0.7 ms of GPU work) is reported next to a
  # 200-step window of the same mode: `reference_window` in the JSON line
  REFW = 200 if (K < 200 and not sharded and args.full) else 0
  if sharded:
    n_batches = K + W + 24
  elif args.full:
    n_batches = ((W + K) + (Wg + K) + 2 * reps + 14 + PROF_WARM + REFW +
                 (0 if args.no_extra_windows else (W + K + 1) + REFW + 2 * (Wg + K + 8)))
  else:   # warm-up, one eager step, the graph mode's rounded warm-up and the timed steps, + look-ahead
    n_batches = W + min(K, 200) + 1 + Wg + K + 3
  P = ring_size(n_batches, K, args.full, RING)

  def make_table(res):
    # room for a batch of new rows per step: K + W + 8 batches with a fresh batch for every step; when the
    # batches come round, new ids come from the ring's P batches only
    units = K + W + 8 if P == n_batches else min(K + W + 8, RING)
    rows_cap = res + units * B * (2 if sharded else 1) + (1 << 16)
    slots = 4
    while slots * 0.5 < rows_cap:
      slots *= 2
    opt = (entry.AdagradOptimizer(0.001, 0.1) if args.opt == "adagrad" else
           entry.SgdOptimizer(0.01))
    cfg = entry.make_table_config(
        [entry.CombineAsSegment(D, entry.ZerosInitializer(), opt)],
        entry.CuckooHashTableConfig(initial_capacity=slots, reserve_rows=rows_cap))
    return MultiHashTable.from_configs({"emb": cfg}, name_suffix="bench%d_%d" % (rank, res))

  mt = None
  while mt is None:
    try:
      mt = make_table(resident)
    except _lib.MhteError as e:  # out of HBM: halve the resident set and say so
      if e.code != _lib.MHTE_RESOURCE_EXHAUSTED or resident < (1 << 16):
        raise
      resident //= 2
      torch.cuda.empty_cache()

  # ---- prefill: the `resident` hottest ranks of this GPU's shard, rows = initializer (zeros) ----
  t0 = time.time()
  mult = torch.tensor(0x9E3779B97F4A7C15 - (1 << 64), dtype=torch.int64, device=dev)
  chunk = 1 << 22
  zeros = torch.zeros((chunk, D), dtype=torch.float32, device=dev)
  filled, r0 = 0, 1
  while filled < resident:
    ranks = torch.arange(r0, r0 + chunk * world, dtype=torch.int64, device=dev)
    r0 += chunk * world
    fid = ((ranks * mult) & ((1 << 48) - 1)) | (1 << 48)
    if world > 1:
      fid = fid[torch.remainder(fid, world) == rank]
    # (about `chunk` of the chunk * world candidates are this rank's — by chance a few more, and the rows
    # buffer holds `chunk`: they go in pieces.  Taking them in one call read past the buffer: a memory fault
    # waiting for the right neighbour, seen with three ranks)
    for o in range(0, fid.numel(), chunk):
      n = min(fid.numel() - o, chunk, resident - filled)
      if n <= 0:
        break
      part = fid[o:o + n].contiguous()
      rg = mt.get_ragged_id({"emb": part})
      _lib.check(mt._lib.mhte_assign(mt.handle, _lib.vp(part),
                                     rg.row_splits.ctypes.data_as(_lib.C.POINTER(_lib.C.c_int64)),
                                     _lib.C.c_int64(2), _lib.vp(zeros), _lib.C.c_int64(n * D),
                                     _lib.C.c_int64(S.update_time(0)),
                                     _lib.C.c_int32(_lib.MHTE_IDS_UNIQUE), None))
      filled += n
  torch.cuda.synchronize()
  del zeros
  torch.cuda.empty_cache()
  prefill_s = time.time() - t0
  st0 = mt.stats("emb")

  # ---- inputs resident in HBM before the timed region (their number P: above the table) ----
  with ThreadPoolExecutor(min(16, os.cpu_count() or 1)) as ex:
    ids_host = np.stack(list(ex.map(lambda s: S.id_batch(s * world + rank, B, V, "zipf"), range(P))))
  ids_all = torch.from_numpy(ids_host).to(dev)
  NG = max(1, args.grad_pool)
  grad_pool = [torch.from_numpy(S.grad_batch(s, B, D)).to(dev) for s in range(NG)]
  applied = []        # (batch, gradient buffer, update_time) of every update enqueued, in order
  applied_ok = True

  def barrier():
    torch.cuda.synchronize()
    if world > 1:
      dist.barrier()
      torch.cuda.synchronize()

  results = {}
  steps_of = {}
  outputs = {}         # --dump-outputs: what each timed window's last step returned, by window
  window_of = {}       # steps [lo, hi) of each timed window
  extra_windows = {}   # ms per step of the windows that are reported beside the line's own (eager_cpp, exact_order)
  stages, shard_info, shard_roofline, uniq_avg = {}, None, None, None
  graph_err = None
  if not sharded:
    # Steady-state pipeline (fused_step.py): while batch s is looked up and updated, the dedup of
    # batch s+1 — which depends on the ids only — rides in the same launches, as the reference's
    # prefetch queue does.  Every timed step executes exactly one dedup, one lookup and one
    # update: the first timed batch was deduplicated by the last warm-up step, the last timed
    # step deduplicates the batch after it.
    step = SparseStep(mt, "emb", B, exact_order=args.exact_order)

    # --lookahead 2 (default): the batch after the next is handed over as well — its run dedup rides
    # in this step's BACKWARD launch and the next step's forward launch carries lookups only; every
    # timed step still executes exactly one dedup, one numbering + probe, one lookup and one update
    two_ahead = args.lookahead >= 2

    def run_eager(lo, hi, st=None):
      st = st or step
      for s in range(lo, hi):
        b = s % P
        st.forward(ids_all[b], next_ids=ids_all[(s + 1) % P],
                   ahead_ids=ids_all[(s + 2) % P] if two_ahead else None)
        st.backward(grad_pool[b % NG], S.update_time(b))
        applied.append((b, b % NG, S.update_time(b)))

    def run_c_loop(lo, hi):
      # the same steps enqueued by a plain C loop over mhte_table_step_forward / _backward
      # (csrc/eager_loop.c): no interpreter and no hipGraph between the calls.  The loop reads batch
      # s + 1 ahead of step s: a stretch ends one step short of the ring's end, and that step (whose
      # next batch is the ring's first) is enqueued from here
      for b, n in ring_stretches(lo, hi, P):
        if n is None:
          run_eager(b, b + 1)
          continue
        step.c_loop(ids_all, b, b + n, grad_pool, S.update_time(0))
        for b_ in range(b, b + n):
          applied.append((b_, b_ % NG, S.update_time(b_)))

    def timed(name, c, w, k):
      import gc
      run_eager(c, c + w)
      gc.collect()
      gc.disable()   # (a generation-2 pass of the interpreter inside the timed region is ~40 ms)
      barrier()
      t = time.perf_counter()
      run_eager(c + w, c + w + k)
      barrier()
      results[name] = time.perf_counter() - t
      gc.enable()
      steps_of[name] = k
      window_of[name] = (c + w, c + w + k)
      if args.dump_outputs:
        outputs[name] = take_outputs({"embeddings": step.emb})
      return c + w + k

    def capture(st, c0, n):
      """hipGraphs of gc steps each for the steps [c0, c0 + n).  Past the ring's length one turn of it is
      captured: graph i serves steps c0 + i * gc + j * P, which train the same batches (replay())."""
      if n > P:
        assert P % 60 == 0, "a ring of %d batches does not come back to its captured state" % P
        n = P
      gs = []
      for a in range(c0, c0 + n, gc):
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
          run_eager(a, a + gc, st)
        gs.append(g)
      return gs

    def replay(gs, lo, hi):
      """chunks [lo, hi) of the steps captured by capture(): a chunk past the ring replays its turn's graph
      (the parity log then no longer lists every update)"""
      nonlocal applied_ok
      if hi > len(gs):
        applied_ok = False
      for i in range(lo, hi):
        gs[i % len(gs)].replay()

    gc = gchunk
    want_graph = args.launch in ("auto", "graph") and K % gc == 0
    if args.full or not want_graph:
      cur = timed("eager", 0, W, K)          # two launches per step
    else:
      # the line's launch mode alone.  Warm-up: the W steps, then (untimed) the eager window that --full times
      # ahead of the graph mode, at most 200 steps — a short graph window measured straight after a few steps
      # read 33.9 us per step against 30.3 behind that window
      cur = W + min(K, 200)
      run_eager(0, cur)

    # ---- hipGraph replay: the launch-bound loop captured in chunks of `gc` pipelined steps
    # (2 launches per step on one queue).  Each chunk graph reads its batches straight from the
    # resident id array, so nothing is copied or skipped inside the timed region.
    # The warm-up is rounded UP to whole chunks (extra untimed steps); exactly K steps are timed.
    if want_graph:
      graphs = []
      try:
        # one eager step first: leaves batch cur+1 deduplicated ahead and a displacement pass
        # outstanding, the state every chunk starts from
        run_eager(cur, cur + 1)
        cur += 1
        step.quiesce()
        G0 = cur
        # (the reference window below is replayed too: enqueued step by step from the interpreter a
        # window is HOST-bound on a slow host — 41.9 us/step on one box against 30.4 replayed)
        n_ref = (REFW // gc) * gc
        graphs = capture(step, G0, Wg + K + n_ref)
        cur = G0 + Wg + K + n_ref
        torch.cuda.synchronize()
        # capture executed nothing: replay from batch G0
        replay(graphs, 0, Wg // gc)
        barrier()
        t = time.perf_counter()
        replay(graphs, Wg // gc, (Wg + K) // gc)
        barrier()
        results["graph"] = time.perf_counter() - t
        steps_of["graph"] = K
        window_of["graph"] = (G0 + Wg, G0 + Wg + K)
        if args.dump_outputs:
          outputs["graph"] = take_outputs({"embeddings": step.emb})
        if n_ref:
          t = time.perf_counter()
          replay(graphs, (Wg + K) // gc, (Wg + K + n_ref) // gc)
          barrier()
          results["graph_ref_window"] = time.perf_counter() - t
          steps_of["graph_ref_window"] = n_ref
      except Exception as e:  # pylint: disable=broad-except
        graph_err = repr(e)[:300]
        applied_ok = False   # (the aborted capture logged updates that never ran)
        print("graph path failed: %s" % graph_err, file=sys.stderr)
        torch.cuda.synchronize()
        # the aborted capture advanced the host-side pipeline state without executing anything:
        # start the following passes from a fresh pipeline
        step = SparseStep(mt, "emb", B, exact_order=args.exact_order)
        cur += gc * (len(graphs) + 1)
        if "eager" not in results:   # (the graph mode was to be the only one: the line's window enqueued eagerly)
          cur = timed("eager", cur, W, K)
    if REFW and "graph_ref_window" not in results:   # (no graph mode: the long window enqueued step by step)
      cur = timed("eager_ref_window", cur, 0, REFW)
    # ---- two more windows of K steps, reported under timing_ms_per_step, never the line's `value`:
    # (a) eager_cpp: enqueued by a C loop over the C ABI — what a TF OpKernel pair pays per step without a
    #     graph (the interpreter's share of `eager` gone);
    # (b) exact_order: the bit-exact mode (every duplicate list summed strictly in occurrence order),
    #     replayed from hipGraphs like the headline
    if not two_ahead and not args.no_extra_windows:
      try:
        import gc as _gc
        run_eager(cur, cur + 1)            # leaves batch cur + 1 deduplicated ahead
        cur += 1
        run_c_loop(cur, cur + W)
        cur += W
        _gc.collect()
        _gc.disable()
        barrier()
        t = time.perf_counter()
        run_c_loop(cur, cur + K)
        barrier()
        extra_windows["eager_cpp"] = (time.perf_counter() - t) / K * 1e3
        cur += K
        if REFW:
          # (a 20-step window of eager launches is mostly the queue's start-up after a drained device: the same C
          # loop over the reference window's 200 steps — profiles/r06/host_enqueue.md)
          barrier()
          t = time.perf_counter()
          run_c_loop(cur, cur + REFW)
          barrier()
          extra_windows["eager_cpp_%d_steps" % REFW] = (time.perf_counter() - t) / REFW * 1e3
          cur += REFW
        _gc.enable()
      except Exception as e:  # pylint: disable=broad-except
        extra_windows["eager_cpp_error"] = repr(e)[:200]
        print("eager_cpp window failed: %r" % (e,), file=sys.stderr)
      if not args.exact_order and "graph" in results and K % gchunk == 0:
        try:
          step_x = SparseStep(mt, "emb", B, exact_order=True)
          run_eager(cur, cur + 4, step_x)   # (every workspace of the new pipeline allocates outside the capture)
          cur += 4
          step_x.quiesce()
          gx = capture(step_x, cur, Wg + K)
          cur += Wg + K
          torch.cuda.synchronize()
          replay(gx, 0, Wg // gchunk)
          barrier()
          t = time.perf_counter()
          replay(gx, Wg // gchunk, (Wg + K) // gchunk)
          barrier()
          extra_windows["exact_order"] = (time.perf_counter() - t) / K * 1e3
          del gx
        except Exception as e:  # pylint: disable=broad-except
          extra_windows["exact_order_error"] = repr(e)[:200]
          applied_ok = False
          print("exact-order window failed: %r" % (e,), file=sys.stderr)
          for _ in range(2):   # (a failed capture leaves its error for the next launch check to find: absorb it)
            try:
              torch.cuda.synchronize()
              torch.zeros(1, device=dev).add_(1)
            except Exception:  # pylint: disable=broad-except
              pass
          step = SparseStep(mt, "emb", B, exact_order=args.exact_order)
          cur += Wg + K + 8
    P0 = cur
  else:
    # the id-sharded step, enqueued from C++ (csrc/mhte_shard_host.h): kernels + RCCL send / recv
    # groups on this stream; world == 1: the exchange is the identity
    from monolith_amd.distributed_ps_sync import ShardedMultiStep
    from tests.torch_sharded_step import HipBackend, ShardedEmbedding   # (test harness: last-resort fallback)
    from monolith_amd.multi_hash_table_ops import Ragged
    splits1 = np.array([0, B], dtype=np.int64)
    rag = [Ragged(ids_all[s], splits1) for s in range(P)]
    emb_out = torch.empty(B * D, dtype=torch.float32, device=dev)
    impl = os.environ.get("MHTE_BENCH_SHARDED_IMPL", "")   # "torch": round 1's torch.distributed form
    if args.transport == "torch":
      impl = "torch"
    se = None
    if world > 1 and args.transport == "rccl" and impl != "torch":
      # the C++ step over RCCL; if RCCL cannot be bound on any rank (a symmetric failure, before the
      # collective communicator set-up), every rank takes the torch.distributed form instead
      err = None
      try:
        from monolith_amd.distributed_ps_sync import shard_unique_id
        shard_unique_id()
      except Exception as e:  # pylint: disable=broad-except
        err = e
      flag = torch.tensor([1 if err is not None else 0], device=dev if args.dist_backend == "nccl" else "cpu")
      dist.all_reduce(flag, op=dist.ReduceOp.MAX)
      if int(flag.item()):
        if rank == 0:
          print("RCCL could not be bound by the library (%r): torch.distributed form of the step" % (err,),
                file=sys.stderr)
        impl = "torch"
    if world > 1 and impl == "torch":
      # ranks sharing one GPU (the 1-GPU box): RCCL cannot put two ranks on a device, so the N > 1
      # control flow of this file is exercised through round 1's torch.distributed form of the step,
      # its exchanges staged through host memory by gloo — not a scaling number
      class _GlooStep:
        def __init__(self):
          self.se = ShardedEmbedding(HipBackend(mt, "emb"))

        def forward(self, r, nxt, out=None):
          out.copy_(self.se.lookup(r.values, next_ids=nxt.values).view(-1))

        def backward(self, g, t):
          self.se.apply_gradients(g.view(B, D), t)

        def check(self):
          torch.cuda.synchronize()

        def info(self):
          return {"transport": "torch.distributed %s (round 1's Python form of the step)" % args.dist_backend}

        def close(self):
          pass
      se = _GlooStep()
    fallback_note = None
    if se is None:
      # Blocks hold the whole batch by default (no step can overflow one, no id is dropped); the
      # peer-store transport and RCCL's exact form move only their occupied part.  --ids-per-peer is
      # an explicit smaller capacity (fixed-size RCCL blocks).
      # The C++ step, by the transport asked for ("auto": peer stores if every rank's self test over
      # the mapped windows passes, else RCCL send / recv — ShardedMultiStep).  If its creation fails
      # on ANY rank, every rank falls back to round 1's torch.distributed form together, and the
      # line says so: a first run on an N-GPU node must end in a number with its transport named,
      # not in a hang or a traceback.
      err = None
      try:
        se = ShardedMultiStep(mt, B, ids_per_peer_table=args.ids_per_peer,
                              transport=args.transport if (world > 1 or args.transport == "ipc") else "auto")
        if world > 1 and se.info()["transport"] == "rccl":
          n_comm, r_comm = se.comm_ranks()
          assert (n_comm, r_comm) == (world, rank), \
              "RCCL communicator holds %d ranks (this one: %d), launched %d (rank %d)" % (n_comm, r_comm, world, rank)
      except Exception as e:  # pylint: disable=broad-except
        err = e
      if world > 1:
        flag = torch.tensor([1 if err is not None else 0], device=dev if args.dist_backend == "nccl" else "cpu")
        dist.all_reduce(flag, op=dist.ReduceOp.MAX)
        if int(flag.item()):
          fallback_note = "C++ step (%s) failed on a rank: %s" % (args.transport, repr(err)[:200] if err else "a peer's error")
          if rank == 0:
            print(fallback_note + " -> torch.distributed form of the step", file=sys.stderr)
          if se is not None:
            try:
              se.close(collective=False)
            except Exception:  # pylint: disable=broad-except
              pass

          class _TorchStep:
            def __init__(self):
              self.se = ShardedEmbedding(HipBackend(mt, "emb"))

            def forward(self, r, nxt, out=None):
              out.copy_(self.se.lookup(r.values, next_ids=nxt.values).view(-1))

            def backward(self, g, t):
              self.se.apply_gradients(g.view(B, D), t)

            def check(self):
              torch.cuda.synchronize()

            def info(self):
              return {"transport": "torch.distributed %s all_to_all (round 1's Python form of the step)" % args.dist_backend,
                      "transport_note": fallback_note}

            def close(self):
              pass
          se = _TorchStep()
      elif err is not None:
        raise err

    host_us = []   # MHTE_BENCH_STEP_TIMES=1: host time of every step's two calls (stall hunting)
    trace_host = os.environ.get("MHTE_BENCH_STEP_TIMES") == "1"

    def run_sharded(lo, hi):
      for s in range(lo, hi):
        t_a = time.perf_counter() if trace_host else 0.0
        b = s % P
        se.forward(rag[b], rag[(s + 1) % P], out=emb_out)
        t_b = time.perf_counter() if trace_host else 0.0
        se.backward(grad_pool[b % NG].view(-1), S.update_time(b))
        if trace_host:
          host_us.append((s, (t_b - t_a) * 1e6, (time.perf_counter() - t_b) * 1e6))
        applied.append((b, b % NG, S.update_time(b)))

    import gc
    run_sharded(0, W)
    gc.collect()
    gc_was = gc.isenabled()
    if os.environ.get("MHTE_BENCH_KEEP_GC") != "1":
      gc.disable()   # (a generation-2 pass of the interpreter is ~40 ms: 200 us on every step of 200)
    barrier()
    t = time.perf_counter()
    run_sharded(W, W + K)
    barrier()
    results["eager"] = time.perf_counter() - t
    elapsed_local = results["eager"]
    if args.dump_outputs:
      outputs["eager"] = take_outputs({"embeddings": emb_out.view(B, D)})
    if gc_was:
      gc.enable()
    steps_of["eager"] = K
    window_of["eager"] = (W, W + K)
    se.check()
    shard_info = se.info()
    if trace_host:
      top = sorted(host_us, key=lambda x: -(x[1] + x[2]))[:6]
      print("slowest steps (step, forward us, backward us): %s" % [(a, round(b), round(c)) for a, b, c in top],
            file=sys.stderr)
    if not args.no_stage_timing:   # kernel-exact time of every tagged launch of a step (every rank
                                   # runs the same extra steps: they are collective; rank 0 reports its own)
      acc = {}
      nprof = 20
      for s in range(W + K, W + K + nprof):
        _lib.profile_arm(64)
        run_sharded(s, s + 1)
        torch.cuda.synchronize()
        for name, us in _lib.profile_read():
          a = acc.setdefault(name, [0, 0.0])
          a[0] += 1
          a[1] += us
      if nprof > 0:
        uniq_avg = float(np.mean([np.unique(ids_host[s % P]).size for s in range(W + K, W + K + nprof)]))
        salg = sharded_algorithmic_bytes(B, uniq_avg, D, S_state)
        stages = {"note": "kernel-exact HIP-event time of the tagged launches of the sharded step "
                          "(+ 1 untagged displacement launch per peer)"}
        for k, v in acc.items():
          us = v[1] / v[0]
          stages[k] = {"launches_per_step": round(v[0] / nprof, 2), "avg_us": round(us, 2)}
          if k in salg:
            stages[k]["alg_bytes"] = int(salg[k])
            stages[k]["GBps"] = round(salg[k] / us / 1e3, 1)
        cands = [k for k in acc if k in salg and k != "dd_kernels"]
        dom = max(cands, key=lambda k: stages[k]["avg_us"]) if cands else None
        a_gbps = salg[dom] / stages[dom]["avg_us"] / 1e3 if dom else 0.0
        step_bytes, _ = algorithmic_bytes(B, uniq_avg, D, S_state)
        shard_roofline = None if dom is None else {
            "bound": "hbm", "kernel": dom, "achieved": round(a_gbps, 1), "peak": HBM_PEAK_GBPS,
            "unit": "GB/s", "frac": round(a_gbps / HBM_PEAK_GBPS, 4), "traffic": None,
            "alg_bytes_per_launch": int(salg[dom]), "avg_launch_us": stages[dom]["avg_us"],
            "timing": "hipExtLaunchKernelGGL start/stop events on the launch stream, %d launches" % nprof,
            "step_alg_bytes": int(step_bytes),
            "step_GBps": round(step_bytes / (elapsed_local / K) / 1e9, 1),
            "step_frac": round(step_bytes / (elapsed_local / K) / 1e9 / HBM_PEAK_GBPS, 4)}
  REF_KEYS = ("graph_ref_window", "eager_ref_window")
  full = {k: v for k, v in results.items() if steps_of[k] == K and k not in REF_KEYS}   # modes timed over exactly K steps
  launch = min(full, key=full.get) if args.launch == "auto" else (
      args.launch if args.launch in full else "eager")
  elapsed = results[launch]
  if world > 1:
    tt = torch.tensor([elapsed], dtype=torch.float64,
                      device=dev if args.dist_backend == "nccl" else "cpu")
    dist.all_reduce(tt, op=dist.ReduceOp.MAX)
    elapsed = float(tt.item())

  # ---- per-kernel timing (N=1): HIP events stamped with each kernel's own begin/end on the launch
  # stream (mhte_profile_arm -> hipExtLaunchKernelGGL), the interval rocprofv3 --kernel-trace
  # reports.  Pass 1: the pipelined step as timed above (2 launches per step).  Pass 2: the
  # same work as separate launches, which attributes time to lookup / backward / dedup.
  roofline = shard_roofline
  if not sharded and not args.no_stage_timing:
    step.quiesce()
    acc = {}

    def collect():
      torch.cuda.synchronize()
      for name, us in _lib.profile_read():
        a = acc.setdefault(name, [0, 0.0])
        a[0] += 1
        a[1] += us

    run_eager(P0, P0 + 1)   # (first step after a mode switch may use the plain forward launch)
    step.quiesce()
    run_eager(P0 + 1, P0 + 1 + PROF_WARM)   # untimed: clocks and caches as in the timed region
    P0 += PROF_WARM
    _lib.profile_arm(2 * reps)
    run_eager(P0 + 1, P0 + 1 + reps)
    collect()
    pipelined = {k: v[1] / v[0] for k, v in acc.items()}
    pipelined_cnt = {k: v[0] for k, v in acc.items()}
    if args.trace_out:   # per-wavefront timeline of three more pipelined steps
      tcap = 1 << 20
      tbuf = torch.zeros(_lib.TRACE_WORDS * tcap, dtype=torch.int64, device=dev)
      _lib.trace_begin(tbuf, tcap)
      run_eager(P0 + 1 + reps, P0 + 4 + reps)
      torch.cuda.synchronize()
      tl = _lib.trace_end()
      np.savez_compressed(args.trace_out, records=tbuf.cpu().numpy().reshape(-1, _lib.TRACE_WORDS),
                          launches=np.array([(t_[0], t_[1], t_[2], t_[3]) for t_ in tl], dtype=object),
                          allow_pickle=True)
    acc = {}
    us = []
    step.quiesce()
    for s in range(P0 + reps + 5, P0 + 2 * reps + 5):
      b = s % P
      ids = ids_all[b]
      _lib.profile_arm(8)
      step._unique(ids)  # pylint: disable=protected-access
      mt.table_lookup_n(step.idx, ids, None, step.emb, n_max=B)
      mt.table_sum_optimize_n(step.idx, step.ws, step.u, grad_pool[b % NG], step.grad_u, step.lrs,
                              S.update_time(b), 0, exact_order=args.exact_order, n_max=B,
                              defer_slowpath=True)
      mt.table_finish_pending(step.idx)
      applied.append((b, b % NG, S.update_time(b)))
      collect()
      us.append(step.n_unique())
    uniq_avg = float(np.mean(us))
    step_bytes, per_kernel = algorithmic_bytes(B, uniq_avg, D, S_state)
    alg = {"step_fwd_kernel": per_kernel["lookup_kernel"],
           "step_bwd_kernel": per_kernel["sum_apply_kernel"],
           "lookup_kernel": per_kernel["lookup_kernel"], "sum_apply_kernel": per_kernel["sum_apply_kernel"]}
    for name, avg in sorted(pipelined.items()):
      stages[name] = {"avg_us": round(avg, 2),
                      "launches_per_step": round(pipelined_cnt[name] / reps, 2)}
    for name, (cnt, tot) in sorted(acc.items()):
      stages["unzipped:" + name] = {"avg_us": round(tot / cnt, 2), "launches_per_step": cnt // reps}
    for name, st_ in stages.items():
      base = name.split(":")[-1]
      if base in alg:
        st_["alg_bytes"] = int(alg[base])
        st_["GBps"] = round(alg[base] / st_["avg_us"] / 1e3, 1)
    dom = max((k for k in pipelined if k in alg), key=lambda k: pipelined[k])
    a_gbps = alg[dom] / pipelined[dom] / 1e3
    # (the committed PMC passes are of the default workload: not applicable to another shape)
    default_shape = (B == 65536 and D == 64 and args.opt == "adagrad" and int(args.universe) == 10**9)
    traffic, traffic_src = pmc_traffic(dom) if default_shape else (None, None)
    roofline = {"bound": "hbm", "kernel": dom, "achieved": round(a_gbps, 1), "peak": HBM_PEAK_GBPS,
                "unit": "GB/s", "frac": round(a_gbps / HBM_PEAK_GBPS, 4), "traffic": traffic,
                "traffic_source": traffic_src,
                "alg_bytes_per_launch": int(alg[dom]),
                "avg_launch_us": round(pipelined[dom], 2),
                "timing": "hipExtLaunchKernelGGL start/stop events on the launch stream, %d launches of the same "
                          "step in a pass of their own behind the timed region (a graph replay cannot carry "
                          "events), %d untimed steps first" % (reps, PROF_WARM),
                "step_alg_bytes": int(step_bytes),
                "step_GBps": round(step_bytes / (elapsed / K) / 1e9, 1),
                "step_frac": round(step_bytes / (elapsed / K) / 1e9 / HBM_PEAK_GBPS, 4)}

  st1 = mt.stats("emb")

  # ---- parity of the benched state: the rows of >= 10 000 ids of the timed stream, read back
  # after everything above, against the oracle's replay of the same update sequence
  parity = None
  if rank == 0 and not args.no_parity_check:
    if not applied_ok:
      parity = {"skipped": "update log incomplete: a failed graph capture, or graphs replayed more than once "
                           "(more steps than distinct batches)"}
    else:
      try:
        last = applied[-1][0]
        probe = np.unique(np.concatenate([ids_host[last], ids_host[(W + K // 2) % P]]))
        lr = 0.001 if args.opt == "adagrad" else 0.01
        t0p = time.time()
        gcache = {}

        def grads_of(g):
          if g not in gcache:
            gcache[g] = S.grad_batch(g, B, D)
          return gcache[g]

        log, ids_of = applied, (lambda b: ids_host[b])
        if world > 1:
          # rank 0's shard after the run: the ids it owns, updated by EVERY rank's batches — one
          # optimizer application per sender, in rank order (distributed_ps_sync.py:357-479)
          probe = probe[np.mod(probe, world) == 0]
          if probe.size > 12000:
            probe = probe[:: probe.size // 12000 + 1]
          log = [((b, r), g, t) for (b, g, t) in applied for r in range(world)]
          ids_of = lambda br: (ids_host[br[0]] if br[1] == 0 else  # noqa: E731
                               S.id_batch(br[0] * world + br[1], B, V, "zipf"))
        exp = oracle_subset_rows(probe, D, args.opt, lr, log, ids_of, grads_of)
        got = mt.lookup({"emb": torch.from_numpy(probe).to(dev)})["emb"].cpu().numpy()
        parity = parity_numbers(got, exp)
        parity.update({"updates_replayed": len(applied), "seconds": round(time.time() - t0p, 1),
                       "exact_order": bool(args.exact_order),
                       "checker": "oracle/ restricted to the probe ids (sequential sums)"})
      except Exception as e:  # pylint: disable=broad-except
        parity = {"failed": repr(e)[:300]}

  # ---- CPU baseline: the reference's own map + AVX Adagrad on this box's host cores ----
  cpu = None
  if not sharded and rank == 0 and not args.no_cpu_baseline:
    try:
      import oracle as O
      cores = os.cpu_count() or 1
      opt = O.OPT_ADAGRAD if args.opt == "adagrad" else O.OPT_SGD
      avx = O.ref_available(True)
      lr = 0.001 if args.opt == "adagrad" else 0.01
      cw = 20
      grads_h = [S.grad_batch(s, B, D) for s in range(4)]

      def cpu_variant(shared, ck):
        # in a process of its own (a baseline must not take the GPU measurement with it).  Round 4 lost
        # variant (ii) to an rc -11: root cause and cure in cpu_child
        import subprocess
        cmd = [sys.executable, os.path.abspath(__file__), "--cpu-child", "ii" if shared else "i",
               "--cpu-steps", str(ck), "--batch", str(B), "--dim", str(D), "--opt", args.opt,
               "--universe", str(args.universe)]
        r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
        if r.returncode != 0:
          return {"value": None, "failed": "rc %d: %s" % (r.returncode, r.stderr.decode()[-200:])}
        return json.loads(r.stdout.decode().strip().splitlines()[-1])

      v1 = cpu_variant(False, args.cpu_steps)
      v2 = cpu_variant(True, max(20, args.cpu_steps // 2))
      cpu = {"value": v1["value"], "unit": "lookups+updates/s", "cores": cores,
             "kind": "reference",
             "sample": "%d steps (after %d warm-up) of the same Zipf(1.2) stream, batch %d, dim %d, "
                       "%s; CPU table grown on demand from empty (%s rows resident at the end — the GPU "
                       "table of the timed line holds %d rows: the small CPU table favours the "
                       "reference); variant (i) PS-style: "
                       "%d single-threaded shards of the reference cuckoohash_map + %s Adagrad, "
                       "median step %s ms" % (args.cpu_steps, cw, B, D, args.opt, v1.get("rows_at_end"),
                                              int(st1.size), cores, "AVX2" if avx else "scalar",
                                              v1.get("median_step_ms")),
             "variants": {"i_ps_shards": v1, "ii_shared_table": v2},
             "note": "phases: single-threaded worker-side dedup (std::unordered_map) and shard "
                     "partition, then %d threads: lookup, scatter to occurrences, duplicate-gradient "
                     "sum, optimize.  (ii) = ONE reference map shared by the threads, contiguous "
                     "chunks of the distinct ids (the fused ops' Shard() loop)" % cores,
             "single_threaded_ms": (lambda ph: None if not ph else round(
                 sum(ph.get(k, 0.0) for k in ("dedup", "partition")), 3))(v1.get("phase_ms_median")),
             "single_threaded_note": "of variant (i)'s median step, this many ms are the worker-side front end "
                                     "(dedup + shard partition) on ONE thread — the reference's worker does the "
                                     "same on its own (unique_mapping_ops.cc:51-155); the per-shard phases use "
                                     "all %d threads.  The GPU / CPU ratio moves with the box's host "
                                     "(12.8-21.9 M/s over the boxes seen): not a figure of merit" % cores}
    except Exception as e:  # pylint: disable=broad-except
      cpu = {"value": None, "unit": "lookups+updates/s", "cores": os.cpu_count(), "kind": "reference",
             "sample": "failed: %r" % (e,)}

  # ---- what crosses the links per step (N > 1): this rank's distinct ids owned by OTHER ranks — ids
  # out, rows back, gradient sums out — against the xGMI bound of SURVEY 8e (7 links x ~153 GB/s per
  # GPU, point to point); the occupied part of the blocks (peer stores and the exact RCCL form move
  # exactly that; the fixed-size RCCL form moves whole blocks: config.shard_step.id_block_bytes)
  exchange_info = None
  if sharded and world > 1:
    nb = min(K, 16)
    remote = float(np.mean([int((np.unique(ids_host[(W + s) % P]) % world != rank).sum()) for s in range(nb)]))
    egress = remote * (8 + 4 * D)          # ids + gradient sums leave
    ingress = remote * (4 * D)             # rows come back (+ the peers' ids and gradients: symmetric)
    per_step_s = elapsed / K
    XGMI_PEAK = 7 * 153.0
    exchange_info = {
        "remote_unique_ids_per_step": round(remote, 1),
        "egress_bytes_per_step": int(egress), "ingress_row_bytes_per_step": int(ingress),
        "egress_GBps_over_the_step": round(egress / per_step_s / 1e9, 2),
        "xgmi_peak_GBps_per_gpu": XGMI_PEAK,
        "frac_of_xgmi": round(egress / per_step_s / 1e9 / XGMI_PEAK, 5),
        "floor_us_at_xgmi_peak": round(max(egress, ingress + remote * 8) / (XGMI_PEAK * 1e9) * 1e6, 2),
        "note": "rank 0's bytes; the step's three exchanges are latency-bound at this size (SURVEY 8e)"}
  if rank == 0:
    # The line is the --steps window's: a short window (the driver's 20 steps are 0.6 ms of GPU work: two
    # hipGraph replays) is fragile, and --full reports the 200-step window of the same step beside it
    # (reference_window).
    value_window = "%d steps, %s" % (K, launch)
    repeated = repeated_steps(*window_of[launch], P) if launch in window_of else 0
    if repeated:
      value_window += ("; %d of them train batches an earlier step trained (a ring of %d distinct batches): "
                       "their ids are all resident, nothing is inserted" % (repeated, P))
    ref_key = next((k for k in REF_KEYS if k in results), None)
    value = 2.0 * B * K * world / elapsed
    if args.dump_outputs:
      write_outputs(args.dump_outputs, outputs[launch])
    out = {
        "metric": "embedding lookups+updates/sec at 1B ids x dim64, Zipf(1.2) batch=65536",
        "value": round(value, 1),
        "unit": "lookups+updates/s",
        "n_gpus": world,
        "steps": K,
        "warmup": W,
        "ms_per_step": round(elapsed / K * 1e3, 5),
        "higher_is_better": True,
        "scaling": "weak",
        "vs_baseline": None,
        "dtype": "f32",
        "data": "synthetic",
        "config": {
            "workload": ("configs[2]: 1 MI355X, 1B-id universe (per GPU), dim=%d, Zipf(1.2), "
                         "batch=%d/GPU, %s; grow-on-demand table" if world == 1 else
                         "configs[3] shape: %d MI355X, %dB ids sharded by fid mod N (1B-id universe "
                         "per GPU), dim=%%d, Zipf(1.2), batch=%%d/GPU, %%s; all-to-all id dispatch + "
                         "row / gradient return" % (world, world)) %
                        (D, B, "fused Adagrad" if args.opt == "adagrad" else "SGD"),
            "batch_per_gpu": B, "dim": D, "universe_ids": V, "optimizer": args.opt,
            "resident_rows_per_gpu_start": int(st0.size), "resident_rows_per_gpu_end": int(st1.size),
            "row_bytes": 4 * (D + S_state), "hashpower": int(st1.hashpower),
            "table_bytes_per_gpu": int(st1.bytes_buckets + st1.bytes_rows),
            "unique_ids_per_batch": uniq_avg, "launch": launch,
            "distinct_batches": P,
            "distinct_batches_note": "step s trains batch s mod %d of the seeded stream" % P,
            "timed_steps_on_repeated_batches": repeated,
            "launch_note": ("hipGraph replay, %d steps per graph; %d untimed warm-up steps replayed "
                            "(--warmup rounded up to whole graphs), exactly %d steps timed" %
                            (gchunk, Wg, K)) if launch == "graph" else None,
            "parallelism": "1 GPU" if not sharded else
                           "fid mod %d sharding, 3 exchanges/step for all tables (%s)%s" %
                           (world, shard_info["transport"],
                            "; %d ranks share each GPU" % -(-world // ndev) if shared_device else ""),
            "shard_step": shard_info,
            "exchange": exchange_info,
            "prefill_s": round(prefill_s, 2),
        },
        "value_window": value_window,
        "timing_ms_per_step": dict(
            {k: round(v / steps_of[k] * 1e3, 5) for k, v in results.items() if k not in REF_KEYS},
            **{k: (round(v, 5) if isinstance(v, float) else v) for k, v in extra_windows.items()}),
        "timing_note": "eager = two Python calls per step; graph = hipGraph replay (the line's value); eager_cpp = "
                       "the same %d steps enqueued by a plain C loop over mhte_table_step_forward / _backward "
                       "(csrc/eager_loop.c: what a TF OpKernel pair pays without a graph); exact_order = the "
                       "bit-exact mode (MHTE_EXACT_ORDER: every duplicate list summed strictly in occurrence "
                       "order; since round 6 the heavy lists are streamed through LDS by rd_exact_sum_kernel), "
                       "hipGraph replay.  HIP_FORCE_DEV_KERNARG=%s: the runtime's switch for where an eager launch's "
                       "kernel arguments live (1 = device memory, set by this script unless the caller set it)"
                       % (K, os.environ.get("HIP_FORCE_DEV_KERNARG", "")),
        "reference_window": None if not ref_key else {
            "steps": steps_of[ref_key], "launch": ref_key.split("_")[0],
            "ms_per_step": round(results[ref_key] / steps_of[ref_key] * 1e3, 5),
            "note": "the same step timed over a longer window (a %d-step window is %.2f ms of work); "
                    "hipGraph replays like the short window when the graph mode is available — enqueued "
                    "step by step a window measures the host" % (K, elapsed * 1e3)},
        "roofline": roofline,
        "stages": stages,
        "cpu_baseline": cpu,
        "parity_check": parity,
    }
    if cpu and cpu.get("value"):
      out["vs_cpu_baseline"] = round(value / cpu["value"], 2)
    if graph_err:
      out["graph_error"] = graph_err
  # communicators go first: whatever their teardown prints must not follow the JSON line; the
  # other ranks empty their C stdio buffers (RCCL's version block) before rank 0 gets that far
  flush_native_stdout()
  if world > 1:
    barrier()
  if sharded:
    se.close()
  if world > 1:
    dist.destroy_process_group()
  flush_native_stdout()
  if rank == 0:
    emit_line(out)


if __name__ == "__main__":
  main()
