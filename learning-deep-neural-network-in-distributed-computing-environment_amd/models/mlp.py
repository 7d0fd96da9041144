"""Multi-layer perceptrons of the BASELINE.json configs.

* ``mlp2``: 2-layer MLP on MNIST-shaped input (config #1, CPU plumbing).
* ``mlp3``: the flagship 3-layer MLP 784-4096-4096-10 (configs #2/#3), whose
  training step the static engine (train/static_mlp.py) runs on the native
  MFMA kernels with graph capture and overlapped RCCL gradient all-reduce.

Activations are fused into the Linear GEMM epilogue (ReLU or sigmoid, the
two activations BASELINE.json names).  With ``norm="layer"`` every hidden
Linear is followed by a LayerNorm over its width, which then carries the
activation (Linear -> LayerNorm + activation -> Dropout); the default builds
none.  With ``linear_dtype="fp8"`` or ``"mxfp8"`` the hidden Linears run their
GEMMs on fp8 codes with per-tensor or per-block scales
(``layers.Linear(compute_dtype=)``); modules and keys stay as they are.
"""
from __future__ import annotations

import torch.nn as nn

from .layers import Dropout, LayerNorm, Linear


class MLP(nn.Module):
    def __init__(self, in_features: int = 784, hidden=(4096, 4096), num_classes: int = 10,
                 activation: str = "relu", dropout: float = 0.0, norm: str = "batch", linear_dtype: str = "bf16"):
        super().__init__()
        if linear_dtype not in ("bf16", "fp8", "mxfp8"):
            raise ValueError(f"MLP: linear_dtype must be 'bf16', 'fp8' or 'mxfp8', got {linear_dtype!r}")
        if norm not in ("batch", "layer"):
            raise ValueError(f"MLP: norm must be 'batch' (the default: no normalisation layer) or 'layer', got {norm!r}")
        dims = [in_features, *hidden, num_classes]
        self.in_features = in_features
        self.num_classes = num_classes
        self.activation = activation
        layer_norm = norm == "layer"
        # with LayerNorm the hidden Linears hand their pre-activations on and the norm applies the activation
        # linear_dtype="fp8" / "mxfp8": every hidden Linear runs its GEMMs in fp8; the output layer (the fused head and
        # loss paths are built around it) stays bf16
        self.layers = nn.ModuleList(
            Linear(dims[i], dims[i + 1], activation=activation if i < len(dims) - 2 and not layer_norm else "none",
                   compute_dtype=linear_dtype if i < len(dims) - 2 else "bf16")
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


def mlp2(in_features=784, hidden=1024, num_classes=10, activation="relu", dropout=0.0, norm="batch",
         linear_dtype="bf16"):
    return MLP(in_features, (hidden,), num_classes, activation, dropout, norm, linear_dtype)


def mlp3(in_features=784, hidden=4096, num_classes=10, activation="relu", dropout=0.0, norm="batch",
         linear_dtype="bf16"):
    return MLP(in_features, (hidden, hidden), num_classes, activation, dropout, norm, linear_dtype)
