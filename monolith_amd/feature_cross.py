"""Feature-cross layers on MI355X — host-side mirror of monolith/native_training/layers/feature_cross.py.

Only ``GroupInt`` (alias ``FFM``, reference :69-146) lives here: the layer between the per-feature outputs of the
layout op and the dense tower.  Its cross is ``layer_ops.ffm``, one hand-written launch forward and one backward.
The attention variant (``use_attention=True``: an MLP over the stacked products) is not built.
"""
from typing import List, Sequence

import torch

from monolith_amd.layer_ops import INT_TYPES, ffm


class GroupInt(torch.nn.Module):
  """Group Interaction: every group embedding of the left list against every one of the right list.

  Args:
    interaction_type: ``'multiply'`` (output ``[B, L R D]``) or ``'dot'`` (output ``[B, L R]``).
    use_attention: admitted with ``'multiply'`` only, as the reference asserts — and not implemented here.
    out_type: kept for the reference's config (``'concat'``, ``'stack'`` or None); the reference's call does not
      read it either.
    keep_list: wrap the output into a one-element list.

  Input: ``(left_fields, right_fields)``, two lists of ``[B, D]`` tensors with one ``D``.
  """

  def __init__(self, interaction_type: str = "multiply", use_attention: bool = False,
               attention_units: List[int] = None, activation="relu", initializer=None, regularizer=None,
               out_type="concat", keep_list: bool = False):
    super().__init__()
    if interaction_type not in INT_TYPES:
      raise ValueError("GroupInt: interaction_type must be 'multiply' or 'dot', got %r" % (interaction_type,))
    if use_attention:
      if interaction_type != "multiply":   # (reference :84-85)
        raise ValueError("GroupInt: use_attention needs interaction_type 'multiply', got %r" % (interaction_type,))
      raise NotImplementedError("GroupInt: use_attention=True (the attention MLP over the stacked products) is "
                                "not implemented")
    self.interaction_type = interaction_type
    self.use_attention = False
    self.attention_units = attention_units
    self.activation = activation
    self.initializer = initializer
    self.regularizer = regularizer
    self.out_type = out_type
    self.keep_list = keep_list

  def forward(self, inputs: Sequence[Sequence[torch.Tensor]]):
    left_fields, right_fields = inputs
    if len(left_fields) == 0 or len(right_fields) == 0:
      raise ValueError("GroupInt: both lists of fields must hold at least one tensor")
    left, right = torch.cat(list(left_fields), dim=1), torch.cat(list(right_fields), dim=1)
    last_dim_size = int(left_fields[0].shape[-1])
    out = ffm(left, right, last_dim_size, self.interaction_type)
    return [out] if self.keep_list else out

  def get_config(self):
    return {"interaction_type": self.interaction_type, "use_attention": self.use_attention,
            "attention_units": self.attention_units, "activation": self.activation,
            "initializer": self.initializer, "regularizer": self.regularizer, "out_type": self.out_type,
            "keep_list": self.keep_list}


FFM = GroupInt
