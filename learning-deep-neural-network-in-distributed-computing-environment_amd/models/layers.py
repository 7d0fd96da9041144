"""Layer modules whose forward/backward run on the native gfx950 kernels.

They subclass the stock ``torch.nn`` layers, so parameter names, shapes,
``state_dict`` keys and init hooks are exactly those of the reference
(BAR/model.py uses nn.Conv2d / nn.BatchNorm2d / nn.Linear / nn.ReLU); only the
compute path changes.  A layer is bound to the model's FlatParams (bf16
shadow + flat gradient buffer) by ``ldnn.prepare`` / ``FlatParams(model)``.
"""
from __future__ import annotations

import math
import os

import torch
import torch.nn as nn

from ..ops import functional as LF


class Linear(nn.Linear):
    """nn.Linear with an optional fused activation epilogue ('none'|'relu'|'sigmoid')."""

    def __init__(self, in_features, out_features, bias=True, activation: str = "none", device=None, dtype=None):
        super().__init__(in_features, out_features, bias=bias, device=device, dtype=dtype)
        assert activation in LF.ACTS
        self.activation = activation
        self._ldnn_flat = None

    def forward(self, x):
        return LF.linear_act(x, self.weight, self.bias, self.activation, self._ldnn_flat)

    def extra_repr(self):
        return super().extra_repr() + f", activation={self.activation}"


class ReLU(nn.ReLU):
    def forward(self, x):
        return LF.relu(x)


class Sigmoid(nn.Sigmoid):
    def forward(self, x):
        return LF.sigmoid(x)


class Flatten(nn.Flatten):
    pass


class Dropout(nn.Dropout):
    """nn.Dropout whose mask is a counter hash of (seed, module_index, call count, element)
    (``LF.dropout_mask``): one native pass each way on the GPU with no mask stored, the exact twin
    on the CPU.  The state (``LF.DropoutState``) is created lazily on the input's device and kept
    in ``__dict__``: it is neither a parameter nor a buffer, so ``state_dict()``, ``buffers()``,
    broadcasts and averaging never see it.  ``reseed_dropout`` gives it its seed and index; the
    rate is compared on the host before each call and rewritten into the state when ``p`` changed
    (``sync_rate`` does the same for a captured step).  Eval mode and ``p == 0`` are the identity."""

    def __init__(self, p: float = 0.5, inplace: bool = False):
        if inplace:
            raise ValueError("ldnn Dropout: inplace=True is not supported")
        super().__init__(p, False)
        self.__dict__["_ldnn_drop"] = None
        self.__dict__["_ldnn_drop_seed"] = (0, 0)   # (seed, module_index) of the last reseed

    def _state(self, device):
        st = self.__dict__["_ldnn_drop"]
        if st is None or st.words.device != device:
            st = self.__dict__["_ldnn_drop"] = LF.DropoutState(device, *self.__dict__["_ldnn_drop_seed"])
        return st

    def reseed(self, seed: int, module_index: int) -> None:
        self.__dict__["_ldnn_drop_seed"] = (int(seed), int(module_index))
        if self.__dict__["_ldnn_drop"] is not None:
            self.__dict__["_ldnn_drop"].reseed(seed, module_index)

    def sync_rate(self) -> None:
        """Write ``self.p`` into an existing state when it changed (a host compare, no device
        traffic otherwise): the graphed steps call it before a replay."""
        st = self.__dict__["_ldnn_drop"]
        if st is not None:
            st.set_rate(self.p)   # (p == 0: thr 0 and scale 1, the captured launch becomes a copy)

    def forward(self, x):
        if self.inplace:
            raise ValueError("ldnn Dropout: inplace=True is not supported")
        if not self.training or self.p == 0:
            return x
        return LF.dropout(x, self.p, True, self._state(x.device))


def dropout_modules(model) -> list:
    """The model's Dropout modules in ``modules()`` order (through a DataParallel wrapper too)."""
    return [m for m in model.modules() if isinstance(m, Dropout)]


def reseed_dropout(model, seed: int) -> int:
    """Give the k-th Dropout of ``model.modules()`` the index k and ``seed``, and zero its call
    count: the masks that follow are a pure function of (seed, k, calls since, element).  Host
    writes into the modules' persistent states, outside any graph: a captured step follows.
    Returns the number of Dropout modules."""
    mods = dropout_modules(model)
    for k, m in enumerate(mods):
        m.reseed(seed, k)
    return len(mods)


class CrossEntropyLoss(nn.CrossEntropyLoss):
    """Mean cross-entropy (the reference's criterion, BAR/main.py:52) on the fused
    softmax-xent kernel.  Pass ``stats`` to accumulate loss-sum / #correct on device.
    ``label_smoothing`` is torch's, and so is the dispatch on the target: integer class
    indices [B] or floating class probabilities [B, C] (Mixup / CutMix, distillation).  Class
    weights and ``ignore_index`` are refused here as before -- ``WeightedCrossEntropyLoss`` is the
    criterion that takes them -- and so are the sum / none reductions."""

    _ldnn_weighted = False   # (WeightedCrossEntropyLoss: True)

    def __init__(self, weight=None, size_average=None, ignore_index: int = -100, reduce=None,
                 reduction: str = "mean", label_smoothing: float = 0.0):
        super().__init__(weight, size_average, ignore_index, reduce, reduction, label_smoothing)
        if not self._ldnn_weighted:
            if weight is not None:
                raise NotImplementedError("ldnn CrossEntropyLoss: class weights are not implemented here: use "
                                          "WeightedCrossEntropyLoss(weight=...)")
            if ignore_index != -100:
                raise NotImplementedError("ldnn CrossEntropyLoss: ignore_index is not implemented here: use "
                                          "WeightedCrossEntropyLoss(ignore_index=...)")
        if self.reduction != "mean":
            raise NotImplementedError(f"ldnn CrossEntropyLoss: reduction={self.reduction!r} is not implemented "
                                      "(mean only)")

    def forward(self, logits, labels, stats=None):
        return LF.cross_entropy(logits, labels, stats, self.label_smoothing)


class WeightedCrossEntropyLoss(CrossEntropyLoss):
    """``CrossEntropyLoss`` with torch's ``weight`` (one finite value >= 0 per class, kept as the
    fp32 buffer ``weight``) and ``ignore_index``, on the weighted instances of the fused kernel
    (a denominator pre-pass + the loss launch).  ``ops.functional.cross_entropy`` names the two
    departures from torch: an all-ignored batch gives 0, not NaN, and a label that is no class
    counts as ignored on the GPU.  With ``weight=None, ignore_index=-100`` it is ``CrossEntropyLoss``,
    launch for launch.  The sum / none reductions are refused as there."""

    _ldnn_weighted = True

    def __init__(self, weight=None, size_average=None, ignore_index: int = -100, reduce=None,
                 reduction: str = "mean", label_smoothing: float = 0.0):
        if weight is not None:
            weight = torch.as_tensor(weight).detach().to(torch.float32).clone()
            if weight.dim() != 1:
                raise ValueError("ldnn WeightedCrossEntropyLoss: weight must be one value per class, got "
                                 f"{tuple(weight.shape)}")
        super().__init__(weight, size_average, int(ignore_index), reduce, reduction, label_smoothing)

    def set_class_weights(self, values) -> None:
        """Copy ``values`` (one per class) into the ``weight`` buffer in place: a host write to a
        persistent address, outside any graph -- a captured step reads the new values at its next
        replay.  The criterion must have been built with weights (a capture bakes their address in)."""
        if self.weight is None:
            raise ValueError("ldnn WeightedCrossEntropyLoss: built without class weights; pass weight= to the "
                             "constructor")
        v = torch.as_tensor(values, dtype=torch.float32)
        if v.shape != self.weight.shape:
            raise ValueError(f"ldnn WeightedCrossEntropyLoss: {tuple(self.weight.shape)} class weights expected, got "
                             f"{tuple(v.shape)}")
        with torch.no_grad():
            self.weight.copy_(v)

    def forward(self, logits, labels, stats=None):
        w = self.weight
        if w is not None and w.device != logits.device:   # (the buffer follows the logits once, then stays)
            self.weight = w = w.to(logits.device)
        return LF.cross_entropy(logits, labels, stats, self.label_smoothing, w, self.ignore_index)


class FocalLoss(WeightedCrossEntropyLoss):
    """The focal loss of Lin et al. 2017 over integer labels, on the focal instances of the fused kernel:
    a kept row's loss is ``weight[y] (1 - p)^gamma (-log p)`` with ``p = softmax(logits)[y]``, divided by the
    kept rows' weight sum as in ``WeightedCrossEntropyLoss``, whose ``weight``, ``ignore_index``,
    ``set_class_weights`` and departures from torch it keeps.  ``gamma`` (finite, >= 0) is a plain
    attribute; 0 is the weighted cross-entropy, launch for launch.  Label smoothing and class-probability
    targets are refused (no agreed definition), and so are the sum / none reductions."""

    def __init__(self, gamma: float = 2.0, weight=None, ignore_index: int = -100, reduction: str = "mean",
                 label_smoothing: float = 0.0):
        if label_smoothing != 0.0:
            raise ValueError(f"ldnn FocalLoss: label_smoothing={label_smoothing} is not defined for the focal loss")
        gamma = float(gamma)
        if not (gamma >= 0.0 and math.isfinite(gamma)):
            raise ValueError(f"ldnn FocalLoss: gamma must be finite and >= 0, got {gamma}")
        super().__init__(weight, None, ignore_index, None, reduction, 0.0)
        self.gamma = gamma

    def extra_repr(self) -> str:
        return f"gamma={self.gamma}, ignore_index={self.ignore_index}"

    def forward(self, logits, labels, stats=None):
        if labels.is_floating_point():
            raise ValueError("ldnn FocalLoss: class-probability targets (Mixup / CutMix) are not defined for the "
                             f"focal loss, got a {tuple(labels.shape)} {labels.dtype} target")
        w = self.weight
        if w is not None and w.device != logits.device:   # (the buffer follows the logits once, then stays)
            self.weight = w = w.to(logits.device)
        return LF.cross_entropy(logits, labels, stats, 0.0, w, self.ignore_index, self.gamma)


class Conv2d(nn.Conv2d):
    """nn.Conv2d (reference key names and init).  On the GPU the activations flow as
    NHWC bf16 through the native implicit-GEMM conv kernels (conv.hip), with the
    weights read from the FlatParams KRSC bf16 shadow; an optional ReLU is fused
    into the conv epilogue."""

    def __init__(self, *args, activation: str = "none", **kwargs):
        super().__init__(*args, **kwargs)
        assert activation in ("none", "relu")
        self.activation = activation
        self._ldnn_flat = None
        self.__dict__["_ldnn_stats_bn"] = None  # (not a submodule: state_dict keys unchanged)

    def forward(self, x):
        return LF.conv2d(x, self, relu=self.activation == "relu",
                         bn=self._ldnn_stats_bn if FUSE_BN_STATS else None)


# Conv-epilogue BatchNorm statistics (pair_conv_bn) are on by default since the
# finalize became parallel (8 accumulator copies summed into LDS, exchanges batched):
# alternated same-box A/B (scripts/ab_cnn.sh, profiles/cnn_fuse_stats_tapmajor_ab_r2.jsonl)
# with the tap-major conv K order: ResNet-18 b64 3.89 -> 3.82 ms, EnhancedCNN b64
# 2.45 -> 2.42 ms.  (Round 1, with a serial finalize, it lost: 3.80 vs 3.67 ms.)
# LDNN_FUSE_BN_STATS=0 turns it off.
FUSE_BN_STATS = os.environ.get("LDNN_FUSE_BN_STATS", "1") == "1"


def pair_conv_bn(conv: "Conv2d", bn: "BatchNorm2d") -> None:
    """Declare that `bn` consumes exactly `conv`'s output: in training mode the conv
    kernel's epilogue then accumulates and finalizes the BN's batch statistics
    (ldnn_conv_lds.h bn_stats_epilogue) and the BN runs only its apply pass.  Only for
    architectures where that dataflow is fixed (the BN also checks it is handed the
    very buffer the conv wrote before it trusts the statistics)."""
    conv.__dict__["_ldnn_stats_bn"] = bn


class BatchNorm2d(nn.BatchNorm2d):
    """Train-mode batch statistics + running-stat EMA exactly as nn.BatchNorm2d;
    on the GPU fp32 statistics over NHWC bf16 activations in the native kernels,
    with optional residual-add + ReLU fused into the same pass (``act``)."""

    def __init__(self, *args, **kwargs):
        super().__init__(*args, **kwargs)
        self._ldnn_flat = None

    def forward(self, x):
        return LF.batch_norm_act(x, self)

    def act(self, x, residual=None, relu: bool = False):
        """relu?(bn(x) + residual) in one fused pass."""
        return LF.batch_norm_act(x, self, residual, relu)


class GroupNorm(nn.GroupNorm):
    """nn.GroupNorm (its parameter names and init; no buffers) with the surface of
    ``BatchNorm2d``: statistics per sample and channel group, so the result does not depend on
    which samples share a batch and train and eval mode are the same function.  On the GPU fp32
    statistics over NHWC bf16 activations in the native kernels (group_norm.hip), with optional
    residual-add + ReLU fused into the same pass (``act``)."""

    def __init__(self, num_groups, num_channels, eps: float = 1e-5, affine: bool = True, device=None, dtype=None):
        super().__init__(num_groups, num_channels, eps=eps, affine=affine, device=device, dtype=dtype)
        self._ldnn_flat = None

    def forward(self, x):
        return LF.group_norm_act(x, self)

    def act(self, x, residual=None, relu: bool = False):
        """relu?(gn(x) + residual) in one fused pass."""
        return LF.group_norm_act(x, self, residual, relu)


class LayerNorm(nn.LayerNorm):
    """nn.LayerNorm over the last dimension (its parameter names and init; no buffers) for the [B, N]
    activations of the MLPs: statistics per row, so the result does not depend on which samples share
    a batch and train and eval mode are the same function.  On the GPU fp32 statistics over bf16 rows
    in the native kernels (layer_norm.hip), with the layer's activation fused into the same pass
    (``act``)."""

    def __init__(self, normalized_shape: int, eps: float = 1e-5, elementwise_affine: bool = True, device=None,
                 dtype=None):
        if not isinstance(normalized_shape, int):
            raise ValueError("ldnn LayerNorm normalises the last dimension: normalized_shape must be an int, got "
                             f"{normalized_shape!r}")
        super().__init__(normalized_shape, eps=eps, elementwise_affine=elementwise_affine, device=device, dtype=dtype)
        self._ldnn_flat = None

    def forward(self, x):
        return LF.layer_norm_act(x, self)

    def act(self, x, act: str = "none"):
        """act(ln(x)) in one fused pass; ``act`` in none | relu | sigmoid."""
        return LF.layer_norm_act(x, self, act)


# "batch" and "group" are the CNNs' choices (make_norm), "layer" the MLPs' (models/mlp.py)
NORMS = ("batch", "group", "layer")


def make_norm(norm: str, channels: int, gn_groups: int = 32):
    """The normalisation layer of a CNN: ``BatchNorm2d(channels)`` or ``GroupNorm(gn_groups, channels)``."""
    if norm == "batch":
        return BatchNorm2d(channels)
    if norm != "group":
        raise ValueError(f"the normalisation layer of a CNN is 'batch' or 'group', got {norm!r}")
    if gn_groups < 1 or channels % gn_groups:
        raise ValueError(f"gn_groups={gn_groups} does not divide the {channels} channels of a normalised layer")
    return GroupNorm(gn_groups, channels)


class MaxPool2d(nn.MaxPool2d):
    def forward(self, x):
        return LF.pool2d(x, self, True)


class AvgPool2d(nn.AvgPool2d):
    def forward(self, x):
        return LF.pool2d(x, self, False)


class AdaptiveAvgPool2d(nn.AdaptiveAvgPool2d):
    def forward(self, x):
        return LF.adaptive_avg_pool2d(x, self.output_size)
