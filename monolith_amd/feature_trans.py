"""Feature-transformation layers on MI355X — host-side mirror of monolith/native_training/layers/feature_trans.py.

``AutoInt`` (reference :31-93) is parameter-free self-attention over the fields of a sample, iterated ``layer_num``
times: ``X <- softmax(X X^T, -1) X`` on ``[B, num_feat, emb]``.  It runs over ``layer_ops.autoint``: the whole stack
is one fused fp32 MFMA launch forward and one backward, a workgroup per sample, the ``[B, n, n]`` score and attention
matrices in registers only.  ``n <= 128``, ``emb <= 64``, ``layer_num <= 8``.

``iRazor`` and ``SeNet`` are not built.
"""
import torch

from monolith_amd.layer_ops import AUTOINT_MAX_LAYERS, autoint

OUT_TYPES = ("concat", "stack", None)


class AutoInt(torch.nn.Module):
  """Auto-Interaction (reference :31-93, https://arxiv.org/abs/1810.11921 without its projections, as the reference
  has it).  One launch of ``layer_ops.autoint``'s kernels forward, one backward.  The layer has no parameters.

  Args:
    layer_num: the number of attention layers, 1 to 8.
    out_type: ``'concat'`` -> ``[B, n k]``, ``'stack'`` -> ``[B, n, k]``, None -> the list of ``n`` tensors ``[B, k]``
      (the reference's ``merge_tensor_list`` of one 3-D tensor).
    keep_list: wrap a ``'concat'`` or ``'stack'`` result in a one-element list.

  Input ``embeds`` ``[B, n, k]``.
  """

  def __init__(self, layer_num: int = 1, out_type="concat", keep_list: bool = False):
    super().__init__()
    if not isinstance(layer_num, int) or isinstance(layer_num, bool) or not 1 <= layer_num <= AUTOINT_MAX_LAYERS:
      raise ValueError("AutoInt: layer_num must be an int in [1, %d], got %r" % (AUTOINT_MAX_LAYERS, layer_num))
    if out_type not in OUT_TYPES:
      raise ValueError("AutoInt: out_type must be 'concat', 'stack' or None, got %r" % (out_type,))
    self.layer_num, self.out_type, self.keep_list = layer_num, out_type, bool(keep_list)

  def forward(self, embeds):
    if not isinstance(embeds, torch.Tensor) or embeds.dim() != 3:
      raise ValueError("AutoInt: the input must be a [B, num_feat, emb] tensor")
    out = autoint(embeds, self.layer_num)
    if self.out_type is None:
      return list(torch.unbind(out, dim=1))
    if self.out_type == "concat":
      out = out.reshape(out.shape[0], out.shape[1] * out.shape[2])
    return [out] if self.keep_list else out

  def get_config(self):
    return {"layer_num": self.layer_num, "out_type": self.out_type, "keep_list": self.keep_list}
