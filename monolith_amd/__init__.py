"""monolith_amd — MI355X-native collisionless embedding-table engine for Monolith's sparse path.

Only the hot path named by BASELINE.json's north_star lives here: the MultiHashTable ops
(lookup / optimize / assign / assign_add / reinitialize / fused_lookup / fused_optimize), the
caller-side dedup and packing ops around them, and the id-sharded all-to-all exchange.  Compute
is hand-written HIP for gfx950 in ``csrc/`` behind the C ABI of
``include/monolith_amd_hash_table.h``; PyTorch is used for device memory, streams and
``torch.distributed`` only.  There is no CPU fallback: without the HIP library or a GPU every op
raises.
"""
from monolith_amd import entry  # noqa: F401
from monolith_amd._lib import build_library, library_path, MhteError  # noqa: F401

_LOSSES = ("inbatch_auc_loss", "inbatch_auc_loss_grad", "inbatch_auc_launch_counts", "batch_softmax_loss",
           "batch_softmax_loss_grad", "batch_softmax_plan", "batch_softmax_launch_counts")

__all__ = ["entry", "build_library", "library_path", "MhteError", "PartitionedHashTable", "losses"] + list(_LOSSES)


def __getattr__(name):
  # (the class needs torch and the library; the package itself imports without either)
  if name == "PartitionedHashTable":
    from monolith_amd.partitioned_hash_table import PartitionedHashTable
    return PartitionedHashTable
  if name == "losses" or name in _LOSSES:
    import importlib
    losses = importlib.import_module("monolith_amd.losses")
    return losses if name == "losses" else getattr(losses, name)
  raise AttributeError("module 'monolith_amd' has no attribute %r" % name)
