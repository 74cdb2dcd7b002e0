"""Feature-cross layers on MI355X — host-side mirror of monolith/native_training/layers/feature_cross.py.

``GroupInt`` (alias ``FFM``, reference :69-146) is the layer between the per-feature outputs of the layout op and
the dense tower.  Its cross is ``layer_ops.ffm``, one hand-written launch forward and one backward.  The attention
variant (``use_attention=True``: an MLP over the stacked products) is not built.

``CIN`` (reference :694-794) is xDeepFM's compressed interaction network over ``layer_ops.cin_layer``: one fused
fp32 MFMA launch per layer forward, two or three backward, without the reference's ``[B, D, H m]`` intermediate.

``DCN`` (reference :445-690) is the cross half of a Deep & Cross network, vector and matrix form, over
``layer_ops.dcn_cross``: one fused launch per layer forward, and the whole stack is one autograd node whose backward
carries a single ``dx0`` buffer through the layers.  The ``mixed`` form (low-rank experts), kernel norm and dropout
are not built.

``CAN`` (reference :345-440) is the Co-Action Network's unit over ``layer_ops.can_unit``: every sample's item
embedding is cut into the weights of a small MLP that runs over that sample's user rows; one fused fp32 MFMA launch
forward and one backward, no intermediate in memory.  Activations None and ``'relu'``; ``'tanh'`` and ``'sigmoid'``,
``d > 32`` and ``layer_num > 8`` are not built.  ``AllInt`` and ``CDot`` are not built.
"""
from typing import List, Sequence

import torch

from monolith_amd.layer_ops import (CAN_ACTIVATIONS, CAN_MAX_LAYERS, CIN_ACTIVATIONS, DCN_TYPES, INT_TYPES, can_unit,
                                    cin_layer, dcn_cross, ffm)


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


class CIN(torch.nn.Module):
  """Compressed Interaction Network, the explicit high-order cross of xDeepFM (reference :694-794).

  Layer i is a 1x1 convolution over the outer product of the running state ``[B, H_i, D]`` with the input
  ``[B, m, D]`` (``H_0 = m``, ``H_i = hidden_uints[i - 1]``); every layer's output is summed over ``D`` and the sums
  are concatenated.  Each layer is one launch of ``layer_ops.cin_layer``; the last one has no activation and never
  writes its ``[B, U, D]`` output.

  Args:
    hidden_uints: the filters of each layer (the reference's spelling, so that configs carry over).
    activation: None or ``'relu'``, applied on every layer but the last.
    initializer: ``'glorot_uniform'`` (the only one built).
    regularizer: kept for the config, not applied.

  Input ``[B, m, D]`` -> ``[B, sum(hidden_uints)]``.  Parameters ``kernel_i`` ``[H_i m, U_i]`` and ``bias_i``
  ``[U_i]`` are created from the first input's shape.
  """

  def __init__(self, hidden_uints: Sequence[int], activation=None, initializer="glorot_uniform", regularizer=None):
    super().__init__()
    if activation not in CIN_ACTIVATIONS:
      raise NotImplementedError("CIN: activation must be None or 'relu', got %r" % (activation,))
    if initializer != "glorot_uniform":
      raise NotImplementedError("CIN: initializer must be 'glorot_uniform', got %r" % (initializer,))
    self.hidden_uints = [int(u) for u in hidden_uints]
    if not self.hidden_uints or min(self.hidden_uints) < 1:
      raise ValueError("CIN: hidden_uints must hold at least one int >= 1, got %r" % (hidden_uints,))
    self.activation = activation
    self.initializer = initializer
    self.regularizer = regularizer
    self._built_for = None

  def _build(self, x: torch.Tensor):
    m = int(x.shape[1])
    for i, units in enumerate(self.hidden_uints):
      fan_in = (m if i == 0 else self.hidden_uints[i - 1]) * m
      limit = (6.0 / (fan_in + units)) ** 0.5   # glorot uniform of Conv1D's (1, H m, U) kernel
      kernel = torch.empty((fan_in, units), dtype=torch.float32, device=x.device).uniform_(-limit, limit)
      self.register_parameter("kernel_%d" % i, torch.nn.Parameter(kernel))
      self.register_parameter("bias_%d" % i, torch.nn.Parameter(torch.zeros(units, dtype=torch.float32,
                                                                            device=x.device)))
    self._built_for = (m, int(x.shape[2]))

  def forward(self, inputs: torch.Tensor):
    if not isinstance(inputs, torch.Tensor) or inputs.dim() != 3:
      raise ValueError("CIN: the input must be a [B, m, D] tensor")
    if self._built_for is None:
      self._build(inputs)
    if self._built_for != (int(inputs.shape[1]), int(inputs.shape[2])):
      raise ValueError("CIN: built for [B, %d, %d], got %s" % (self._built_for + (tuple(inputs.shape),)))
    xl, pooled = inputs, []
    last = len(self.hidden_uints) - 1
    for i in range(last + 1):
      xl, p = cin_layer(inputs, xl, getattr(self, "kernel_%d" % i), getattr(self, "bias_%d" % i),
                        None if i == last else self.activation, want_next=i != last)
      pooled.append(p)
    return torch.cat(pooled, dim=1)

  def get_config(self):
    return {"hidden_uints": self.hidden_uints, "activation": self.activation, "initializer": self.initializer,
            "regularizer": self.regularizer}


class DCN(torch.nn.Module):
  """The cross network of Deep & Cross (reference :445-690), ``xl = x0`` and per layer

    vector:  ``xl = x0 * (xl @ kernel_i) + bias_i + xl``      kernel_i ``[d, 1]``
    matrix:  ``xl = x0 * (xl @ kernel_i + bias_i) + xl``      kernel_i ``[d, d]``

  with ``bias_i`` ``[1, d]``; every layer is one launch of ``layer_ops.dcn_cross``'s kernels.

  Args:
    layer_num: the number of cross layers.
    dcn_type: ``'vector'`` or ``'matrix'``; ``'mixed'`` is not built.
    initializer: None (glorot normal: a normal of stddev ``sqrt(2 / (fan_in + fan_out)) / 0.87962566`` truncated at
      two stddev); nothing else is built.
    regularizer, num_experts, low_rank, keep_prob, mode: kept for the config, not applied.
    allow_kernel_norm, use_dropout: must be False.

  Input ``[B, d]`` -> ``[B, d]``.  Parameters are created from the first input's shape.
  """

  def __init__(self, layer_num: int = 1, dcn_type: str = "matrix", initializer=None, regularizer=None,
               num_experts: int = 1, low_rank: int = 0, allow_kernel_norm: bool = False, use_dropout: bool = False,
               keep_prob: float = 0.95, mode: str = "train"):
    super().__init__()
    if dcn_type not in DCN_TYPES:
      raise NotImplementedError("DCN: dcn_type must be 'vector' or 'matrix', got %r" % (dcn_type,))
    if allow_kernel_norm:
      raise NotImplementedError("DCN: allow_kernel_norm=True is not built")
    if use_dropout:
      raise NotImplementedError("DCN: use_dropout=True is not built")
    if initializer is not None:
      raise NotImplementedError("DCN: initializer must be None (glorot normal), got %r" % (initializer,))
    if int(layer_num) < 1:
      raise ValueError("DCN: layer_num must be an int >= 1, got %r" % (layer_num,))
    self.layer_num, self.dcn_type = int(layer_num), dcn_type
    self.initializer, self.regularizer = initializer, regularizer
    self.num_experts, self.low_rank = num_experts, low_rank
    self.allow_kernel_norm, self.use_dropout, self.keep_prob, self.mode = False, False, keep_prob, mode
    self._built_for = None

  def _build(self, x: torch.Tensor):
    d = int(x.shape[1])
    cols = d if self.dcn_type == "matrix" else 1
    std = (2.0 / (d + cols)) ** 0.5 / 0.87962566
    for i in range(self.layer_num):
      kernel = torch.empty((d, cols), dtype=torch.float32, device=x.device)
      torch.nn.init.trunc_normal_(kernel, 0.0, std, -2 * std, 2 * std)
      self.register_parameter("kernel_%d" % i, torch.nn.Parameter(kernel))
      self.register_parameter("bias_%d" % i, torch.nn.Parameter(torch.zeros((1, d), dtype=torch.float32,
                                                                            device=x.device)))
    self._built_for = d

  def forward(self, inputs: torch.Tensor):
    if not isinstance(inputs, torch.Tensor) or inputs.dim() != 2:
      raise ValueError("DCN: the input must be a [B, d] tensor")
    if self._built_for is None:
      self._build(inputs)
    if self._built_for != int(inputs.shape[1]):
      raise ValueError("DCN: built for [B, %d], got %s" % (self._built_for, tuple(inputs.shape)))
    return dcn_cross(inputs, [getattr(self, "kernel_%d" % i) for i in range(self.layer_num)],
                     [getattr(self, "bias_%d" % i) for i in range(self.layer_num)], self.dcn_type)

  def get_config(self):
    return {"layer_num": self.layer_num, "dcn_type": self.dcn_type, "initializer": self.initializer,
            "regularizer": self.regularizer, "num_experts": self.num_experts, "low_rank": self.low_rank,
            "allow_kernel_norm": self.allow_kernel_norm, "use_dropout": self.use_dropout,
            "keep_prob": self.keep_prob, "mode": self.mode}


class CAN(torch.nn.Module):
  """The Co-Action Network's unit (reference :345-440).  The item side is reshaped into the parameters of an MLP,
  per sample ``layer_num`` pairs ``(W_i [d, d], b_i [d])`` in that order, and the user side is its input:
  ``h = activation(h @ W_i + b_i)`` on every layer, then the sum over the sequence axis where there is one.  One
  launch of ``layer_ops.can_unit``'s kernels forward, one backward.

  Args:
    layer_num: the number of layers, 1 to 8.
    activation: None or ``'relu'``; ``'tanh'`` and ``'sigmoid'`` are not built.
    is_seq: the user side has a sequence axis.
    is_stacked: the user side is several features stacked.

  Input ``(user_emb, item_emb)``: ``user_emb`` ``[B, F, T, d]`` / ``[B, F, d]`` / ``[B, T, d]`` / ``[B, d]`` for
  (is_seq, is_stacked) = (T, T) / (F, T) / (T, F) / (F, F), ``d <= 32``; ``item_emb`` ``[B, layer_num d (d + 1)]``
  -> ``[B, F, d]`` when stacked, else ``[B, d]`` (also at ``B = 1``, where the reference's squeeze drops the batch
  axis).  The layer has no parameters.
  """

  def __init__(self, layer_num: int = 2, activation="relu", is_seq: bool = False, is_stacked: bool = True):
    super().__init__()
    if activation not in CAN_ACTIVATIONS:
      raise NotImplementedError("CAN: activation must be None or 'relu', got %r" % (activation,))
    if not isinstance(layer_num, int) or isinstance(layer_num, bool) or not 1 <= layer_num <= CAN_MAX_LAYERS:
      raise ValueError("CAN: layer_num must be an int in [1, %d], got %r" % (CAN_MAX_LAYERS, layer_num))
    self.layer_num, self.activation = layer_num, activation
    self.is_seq, self.is_stacked = bool(is_seq), bool(is_stacked)

  def forward(self, inputs):
    if not isinstance(inputs, (tuple, list)) or len(inputs) != 2:
      raise ValueError("CAN: the input must be (user_emb, item_emb)")
    return can_unit(inputs[0], inputs[1], self.layer_num, self.activation, self.is_seq, self.is_stacked)

  def get_config(self):
    return {"layer_num": self.layer_num, "activation": self.activation, "is_seq": self.is_seq,
            "is_stacked": self.is_stacked}
