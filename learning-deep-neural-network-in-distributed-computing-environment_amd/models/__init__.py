"""Model zoo: the reference's EnhancedCNNModel (+ its small variant) and the
BASELINE.json configs (mlp2, mlp3, lenet5, resnet18)."""
from __future__ import annotations

import torch.nn as nn

from .cnn import EnhancedCNNModel, EnhancedCNNSmall, LeNet5, ResBlock  # noqa: F401
from .layers import (NORMS, CrossEntropyLoss, Dropout, FocalLoss, GroupNorm, LayerNorm, Linear,  # noqa: F401
                     WeightedCrossEntropyLoss, reseed_dropout)
from .mlp import MLP, mlp2, mlp3  # noqa: F401
from .resnet import ResNet, resnet18  # noqa: F401

# name -> (constructor, input kind for the synthetic dataset)
REGISTRY = {
    "enhanced_cnn": (lambda nc=10, dropout=0.0, **norm: EnhancedCNNModel(nc, dropout=dropout, **norm), "cifar10"),
    "enhanced_cnn_small": (lambda nc=10, dropout=0.0, **norm: EnhancedCNNSmall(nc, dropout=dropout, **norm), "cifar10"),
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


def build_model(name: str, num_classes: int | None = None, dropout: float = 0.0, norm: str = "batch",
                gn_groups: int = 32) -> nn.Module:
    """``dropout``: the rate of the model's Dropout modules (MLPs: after every hidden layer; LeNet-5:
    after fc1 and fc2; the ResNets and EnhancedCNNs: in front of the classifier).  0: none exist.
    ``norm``: "batch" (BatchNorm2d, the default) or "group" (GroupNorm with ``gn_groups`` groups under
    the same attribute names, so the ``weight`` / ``bias`` keys are the BatchNorm model's and there are
    no buffers); the MLPs and LeNet-5 have no normalisation layer and refuse "group".  "layer": the
    MLPs only -- a LayerNorm over the width after every hidden Linear, carrying the activation
    (``norms.{i}.weight`` / ``norms.{i}.bias`` beside the default's keys, no buffers); every other
    model refuses it."""
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
