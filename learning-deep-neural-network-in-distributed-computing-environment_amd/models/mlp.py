"""Multi-layer perceptrons of the BASELINE.json configs.

* ``mlp2``: 2-layer MLP on MNIST-shaped input (config #1, CPU plumbing).
* ``mlp3``: the flagship 3-layer MLP 784-4096-4096-10 (configs #2/#3), whose
  training step the static engine (train/static_mlp.py) runs on the native
  MFMA kernels with graph capture and overlapped RCCL gradient all-reduce.

Activations are fused into the Linear GEMM epilogue (ReLU or sigmoid, the
two activations BASELINE.json names).  With ``norm="layer"`` every hidden
Linear is followed by a LayerNorm over its width, which then carries the
activation (Linear -> LayerNorm + activation -> Dropout); the default builds
none.
"""
from __future__ import annotations

import torch.nn as nn

from .layers import Dropout, LayerNorm, Linear


class MLP(nn.Module):
    def __init__(self, in_features: int = 784, hidden=(4096, 4096), num_classes: int = 10,
                 activation: str = "relu", dropout: float = 0.0, norm: str = "batch"):
        super().__init__()
        if norm not in ("batch", "layer"):
            raise ValueError(f"MLP: norm must be 'batch' (the default: no normalisation layer) or 'layer', got {norm!r}")
        dims = [in_features, *hidden, num_classes]
        self.in_features = in_features
        self.num_classes = num_classes
        self.activation = activation
        layer_norm = norm == "layer"
        # with LayerNorm the hidden Linears hand their pre-activations on and the norm applies the activation
        self.layers = nn.ModuleList(
            Linear(dims[i], dims[i + 1], activation=activation if i < len(dims) - 2 and not layer_norm else "none")
            for i in range(len(dims) - 1)
        )
        # LayerNorm after every hidden Linear; none is constructed by default, so named_modules(),
        # the state_dict keys and every launch are then those of the model without the keyword
        if layer_norm:
            self.norms = nn.ModuleList(LayerNorm(w) for w in hidden)
        # dropout after every hidden layer's fused activation; none is constructed at rate 0, so
        # named_modules() and every launch are then those of the model without the keyword
        if dropout:
            self.drops = nn.ModuleList(Dropout(dropout) for _ in hidden)

    def forward(self, x):
        x = x.flatten(1)
        norms = getattr(self, "norms", ())
        drops = getattr(self, "drops", ())
        for i, layer in enumerate(self.layers):
            x = layer(x)
            if i < len(norms):
                x = norms[i].act(x, self.activation)
            if i < len(drops):
                x = drops[i](x)
        return x


def mlp2(in_features=784, hidden=1024, num_classes=10, activation="relu", dropout=0.0, norm="batch"):
    return MLP(in_features, (hidden,), num_classes, activation, dropout, norm)


def mlp3(in_features=784, hidden=4096, num_classes=10, activation="relu", dropout=0.0, norm="batch"):
    return MLP(in_features, (hidden, hidden), num_classes, activation, dropout, norm)
