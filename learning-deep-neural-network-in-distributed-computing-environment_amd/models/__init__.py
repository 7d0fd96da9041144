"""Model zoo: the reference's EnhancedCNNModel (+ its small variant) and the
BASELINE.json configs (mlp2, mlp3, lenet5, resnet18)."""
from __future__ import annotations

import torch.nn as nn

from .cnn import EnhancedCNNModel, EnhancedCNNSmall, LeNet5, ResBlock, SeparableConv2d  # noqa: F401
from .layers import (NORMS, CrossEntropyLoss, Dropout, FocalLoss, GroupNorm, LayerNorm, Linear,  # noqa: F401
                     SqueezeExcite, WeightedCrossEntropyLoss, reseed_dropout)
from .mlp import MLP, mlp2, mlp3  # noqa: F401
from .resnet import ResNet, resnet18  # noqa: F401

# name -> (constructor, input kind for the synthetic dataset)
REGISTRY = {
    "enhanced_cnn": (lambda nc=10, dropout=0.0, **kw: EnhancedCNNModel(nc, dropout=dropout, **kw), "cifar10"),
    "enhanced_cnn_small": (lambda nc=10, dropout=0.0, **kw: EnhancedCNNSmall(nc, dropout=dropout, **kw), "cifar10"),
    "lenet5": (lambda nc=10, dropout=0.0: LeNet5(nc, dropout=dropout), "mnist"),
    "mlp2": (lambda nc=10, dropout=0.0, **norm: mlp2(784, 1024, nc, dropout=dropout, **norm), "mnist"),
    "mlp3": (lambda nc=10, dropout=0.0, **norm: mlp3(784, 4096, nc, dropout=dropout, **norm), "mnist"),
    "mlp3_small": (lambda nc=10, dropout=0.0, **norm: mlp3(784, 1024, nc, dropout=dropout, **norm), "mnist"),
    "resnet18": (lambda nc=1000, dropout=0.0, **norm: resnet18(nc, dropout=dropout, **norm), "imagenet"),
    "resnet18_cifar": (lambda nc=10, dropout=0.0, **norm: resnet18(nc, dropout=dropout, **norm), "cifar10"),
}


# the models that have normalisation layers, hence a ``norm`` choice
NORM_MODELS = ("enhanced_cnn", "enhanced_cnn_small", "resnet18", "resnet18_cifar")
# the models that take a LayerNorm after every hidden Linear (norm="layer")
LAYER_NORM_MODELS = ("mlp2", "mlp3", "mlp3_small")
# the models whose hidden Linear layers take linear_dtype="fp8" / "mxfp8"
FP8_LINEAR_MODELS = ("mlp2", "mlp3", "mlp3_small")
# the models that have a depthwise-separable variant (separable=True)
SEPARABLE_MODELS = ("enhanced_cnn", "enhanced_cnn_small")
# the group widths of a separable variant's 3x3 beside 1 (depthwise): build_model(..., group_width=)
GROUP_WIDTHS = (8, 16, 32)
# the models whose residual blocks take a Squeeze-and-Excitation gate (se_ratio > 0)
SE_MODELS = ("enhanced_cnn", "enhanced_cnn_small")


def build_model(name: str, num_classes: int | None = None, dropout: float = 0.0, norm: str = "batch",
                gn_groups: int = 32, separable: bool = False, linear_dtype: str = "bf16",
                group_width: int = 1, se_ratio: int = 0) -> nn.Module:
    """``dropout``: the rate of the model's Dropout modules (MLPs: after every hidden layer; LeNet-5:
    after fc1 and fc2; the ResNets and EnhancedCNNs: in front of the classifier).  0: none exist.
    ``norm``: "batch" (BatchNorm2d, the default) or "group" (GroupNorm with ``gn_groups`` groups under
    the same attribute names, so the ``weight`` / ``bias`` keys are the BatchNorm model's and there are
    no buffers); the MLPs and LeNet-5 have no normalisation layer and refuse "group".  "layer": the
    MLPs only -- a LayerNorm over the width after every hidden Linear, carrying the activation
    (``norms.{i}.weight`` / ``norms.{i}.bias`` beside the default's keys, no buffers); every other
    model refuses it.
    ``separable``: the EnhancedCNNs with every residual-block 3x3 convolution as a depthwise 3x3 followed
    by a 1x1 (``conv1.dw.weight`` / ``conv1.pw.weight``); every other model refuses it.
    ``group_width``: with ``separable``, the 3x3 mixes this many neighbouring channels (1: depthwise; 8, 16 or 32:
    a grouped convolution, ``dw.weight`` [C, group_width, 3, 3] under the same keys).
    ``linear_dtype``: "bf16" (the default), "fp8" (per-tensor scales) or "mxfp8" (one scale per block of 32): the
    MLPs' hidden Linear layers run their three GEMMs on fp8 codes (the output layer stays bf16; modules and keys are
    the default's); every other model refuses it.
    ``se_ratio``: R > 0 gives every residual block of the EnhancedCNNs a Squeeze-and-Excitation gate with
    max(8, C // R) hidden units (``se.fc1.weight`` / ``se.fc1.bias`` / ``se.fc2.weight`` / ``se.fc2.bias`` beside the
    default's keys); 0, the default, builds none; every other model refuses it."""
    ctor, _ = REGISTRY[name]
    if norm not in NORMS:
        raise ValueError(f"norm must be one of {NORMS}, got {norm!r}")
    kw = {"dropout": dropout} if dropout else {}
    if norm == "group":
        if name not in NORM_MODELS:
            raise ValueError(f"norm='group': {name} has no normalisation layer")
        kw.update(norm=norm, gn_groups=gn_groups)
    elif norm == "layer":
        if name not in LAYER_NORM_MODELS:
            raise ValueError(f"norm='layer': LayerNorm is built for the MLPs ({', '.join(LAYER_NORM_MODELS)}), "
                             f"not for {name}")
        kw.update(norm=norm)
    if group_width != 1:
        if group_width not in GROUP_WIDTHS:
            raise ValueError(f"group_width must be 1 or one of {GROUP_WIDTHS}, got {group_width!r}")
        if not separable:
            raise ValueError(f"group_width={group_width}: the group width is the separable blocks' 3x3; it needs "
                             "separable=True")
        if name not in SEPARABLE_MODELS:
            raise ValueError(f"group_width={group_width}: the separable variant is built for "
                             f"{', '.join(SEPARABLE_MODELS)}, not for {name}")
        kw.update(group_width=group_width)
    if separable:
        if name not in SEPARABLE_MODELS:
            raise ValueError(f"separable=True: the depthwise-separable variant is built for "
                             f"{', '.join(SEPARABLE_MODELS)}, not for {name}")
        kw.update(separable=True)
    if linear_dtype != "bf16":
        if linear_dtype not in ("fp8", "mxfp8"):
            raise ValueError(f"linear_dtype must be 'bf16', 'fp8' or 'mxfp8', got {linear_dtype!r}")
        if name not in FP8_LINEAR_MODELS:
            raise ValueError(f"linear_dtype={linear_dtype!r}: the fp8 Linear is built for the hidden layers of the MLPs "
                             f"({', '.join(FP8_LINEAR_MODELS)}), not for {name}")
        kw.update(linear_dtype=linear_dtype)
    if se_ratio:
        if se_ratio < 0:
            raise ValueError(f"se_ratio must be >= 0, got {se_ratio!r}")
        if name not in SE_MODELS:
            raise ValueError(f"se_ratio={se_ratio}: the Squeeze-and-Excitation blocks are built for "
                             f"{', '.join(SE_MODELS)}, not for {name}")
        kw.update(se_ratio=se_ratio)
    return ctor(**kw) if num_classes is None else ctor(num_classes, **kw)


def dataset_for(name: str) -> str:
    return REGISTRY[name][1]


def xavier_init(model: nn.Module):
    """The reference's init (BAR/main.py:33-37): Xavier-uniform Conv2d/Linear
    weights, zero biases."""
    for m in model.modules():
        if isinstance(m, (nn.Conv2d, nn.Linear)):
            nn.init.xavier_uniform_(m.weight)
            if m.bias is not None:
                nn.init.zeros_(m.bias)
