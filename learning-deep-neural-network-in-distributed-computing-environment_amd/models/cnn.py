"""CNN model families of the reference and of the BASELINE.json configs.

* ``EnhancedCNNModel`` -- the reference's CIFAR ResNet-style network
  (BAR/model.py:74-111): prep conv3x3 3->64 + BN + ReLU, four stages of two
  ``ResBlock``s (64->128->256->512->1024, first block stride 2), global average
  pool, fc 1024->10.  44,595,786 parameters; state_dict keys identical to the
  reference (prep.0.weight, layer1.0.conv1.weight, ..., fc.bias).
* ``EnhancedCNNSmall`` -- the commented-out three-stage variant
  (BAR/model.py:4-50): 4,829,258 parameters.
* ``LeNet5`` -- BASELINE.json config #4 (28x28 input).
"""
from __future__ import annotations

import torch.nn as nn

from ..ops import functional as LF
from .layers import (AdaptiveAvgPool2d, AvgPool2d, BatchNorm2d, Conv2d, Dropout, Linear, MaxPool2d, ReLU, make_norm,
                     pair_conv_bn)


class ConvBNReLU(nn.Sequential):
    """Sequential(conv, norm, relu) -- same state_dict keys (prep.0 / prep.1) -- whose
    norm and ReLU run as one fused pass."""

    def __init__(self, *mods):
        super().__init__(*mods)
        if isinstance(self[1], BatchNorm2d):
            pair_conv_bn(self[0], self[1])

    def forward(self, x):
        return self[1].act(self[0](x), relu=True)


class ResBlock(nn.Module):
    """conv3x3(stride)-BN-ReLU-conv3x3-BN + shortcut (1x1 conv + BN when the shape
    changes) -> add -> ReLU; convs without bias (BAR/model.py:52-72).  ``norm="group"``: a
    GroupNorm under every BN's attribute name (bn1, bn2, shortcut.1)."""

    def __init__(self, in_channels, out_channels, stride=1, norm: str = "batch", gn_groups: int = 32):
        super().__init__()
        self.conv1 = Conv2d(in_channels, out_channels, kernel_size=3, stride=stride, padding=1, bias=False)
        self.bn1 = make_norm(norm, out_channels, gn_groups)
        self.conv2 = Conv2d(out_channels, out_channels, kernel_size=3, stride=1, padding=1, bias=False)
        self.bn2 = make_norm(norm, out_channels, gn_groups)
        self.shortcut = nn.Sequential()
        if stride != 1 or in_channels != out_channels:
            self.shortcut = nn.Sequential(
                Conv2d(in_channels, out_channels, kernel_size=1, stride=stride, bias=False),
                make_norm(norm, out_channels, gn_groups),
            )
        self.relu = ReLU()
        self.group_norm = norm == "group"
        if not self.group_norm:
            pair_conv_bn(self.conv1, self.bn1)
            pair_conv_bn(self.conv2, self.bn2)
            if len(self.shortcut):
                pair_conv_bn(self.shortcut[0], self.shortcut[1])

    def forward(self, x):
        if self.group_norm:
            # conv -> gn(+ReLU), conv -> gn(+ residual + ReLU); the shortcut's GroupNorm output is
            # the residual of the main branch's pass.  No twins: autograd sums x's two gradients
            if len(self.shortcut):
                c1, sc = LF.conv2d_pair(x, LF.shortcut_input(x), self.conv1, self.shortcut[0])
                res = self.shortcut[1].act(sc)
            else:
                c1, res = self.conv1(x), LF.shortcut_input(x)
            return self.bn2.act(self.conv2(self.bn1.act(c1, relu=True)), residual=res, relu=True)
        # BAR/model.py:67-72 with BN+ReLU and BN+residual-add+ReLU each fused into one pass;
        # the shortcut reads x's twin (LF.shortcut_input), so the producer of x sums the two
        # branch gradients in its own backward kernels instead of a separate add
        if len(self.shortcut):
            # the 3x3 and the 1x1 shortcut conv of x in one launch, then conv2 and both BNs, the add
            # and the ReLU in one pass
            c1, sc = LF.conv2d_pair(x, LF.shortcut_input(x), self.conv1, self.shortcut[0])
            out = self.bn1.act(c1, relu=True)
            return LF.batch_norm_dual_act(self.conv2(out), self.bn2, sc, self.shortcut[1])
        out = self.bn1.act(self.conv1(x), relu=True)
        return self.bn2.act(self.conv2(out), residual=LF.shortcut_input(x), relu=True)


def _head(x, pool, fc, drop=None):
    """fc(drop(flatten(pool(x)))).  Without an active dropout (none constructed, eval mode or
    rate 0) that is the fused gap_linear launch; with one, pool -> flatten -> dropout -> fc."""
    if drop is None or not drop.training or drop.p == 0:
        return LF.gap_linear(x, pool, fc)   # pool -> view -> fc (one fused launch each way on the GPU)
    y = pool(x)
    return fc(drop(y.reshape(y.size(0), -1)))


class EnhancedCNNModel(nn.Module):
    def __init__(self, num_classes: int = 10, in_channels: int = 3, dropout: float = 0.0, norm: str = "batch",
                 gn_groups: int = 32):
        super().__init__()
        nk = dict(norm=norm, gn_groups=gn_groups)
        self.prep = ConvBNReLU(
            Conv2d(in_channels, 64, kernel_size=3, stride=1, padding=1, bias=False),
            make_norm(norm, 64, gn_groups),
            ReLU(),
        )
        self.layer1 = nn.Sequential(ResBlock(64, 128, stride=2, **nk), ResBlock(128, 128, stride=1, **nk))
        self.layer2 = nn.Sequential(ResBlock(128, 256, stride=2, **nk), ResBlock(256, 256, stride=1, **nk))
        self.layer3 = nn.Sequential(ResBlock(256, 512, stride=2, **nk), ResBlock(512, 512, stride=1, **nk))
        self.layer4 = nn.Sequential(ResBlock(512, 1024, stride=2, **nk), ResBlock(1024, 1024, stride=1, **nk))
        self.pool = AdaptiveAvgPool2d(1)
        self.fc = Linear(1024, num_classes)
        if dropout:   # (none constructed at rate 0: named_modules() stay the reference's)
            self.drop = Dropout(dropout)

    def forward(self, x):
        x = self.prep(x)
        x = self.layer1(x)
        x = self.layer2(x)
        x = self.layer3(x)
        x = self.layer4(x)
        return _head(x, self.pool, self.fc, getattr(self, "drop", None))


class EnhancedCNNSmall(nn.Module):
    """The reference's commented-out smaller model (BAR/model.py:4-50)."""

    def __init__(self, num_classes: int = 10, in_channels: int = 3, dropout: float = 0.0, norm: str = "batch",
                 gn_groups: int = 32):
        super().__init__()
        nk = dict(norm=norm, gn_groups=gn_groups)
        self.prep = ConvBNReLU(
            Conv2d(in_channels, 64, kernel_size=3, stride=1, padding=1, bias=False),
            make_norm(norm, 64, gn_groups),
            ReLU(),
        )
        self.layer1 = ResBlock(64, 128, stride=2, **nk)
        self.layer2 = ResBlock(128, 256, stride=2, **nk)
        self.layer3 = ResBlock(256, 512, stride=2, **nk)
        self.pool = AdaptiveAvgPool2d(1)
        self.fc = Linear(512, num_classes)
        if dropout:
            self.drop = Dropout(dropout)

    def forward(self, x):
        x = self.prep(x)
        x = self.layer3(self.layer2(self.layer1(x)))
        return _head(x, self.pool, self.fc, getattr(self, "drop", None))


class LeNet5(nn.Module):
    """LeNet-5 for 28x28 (MNIST-shaped) input: conv5x5(pad 2)-ReLU-pool, conv5x5-ReLU-pool,
    fc 400-120-84-10 (ReLU activations fused into the Linear epilogues)."""

    def __init__(self, num_classes: int = 10, in_channels: int = 1, pool: str = "max", dropout: float = 0.0):
        super().__init__()
        P = MaxPool2d if pool == "max" else AvgPool2d
        self.features = nn.Sequential(
            Conv2d(in_channels, 6, kernel_size=5, padding=2, activation="relu"), ReLU(), P(2),
            Conv2d(6, 16, kernel_size=5, activation="relu"), ReLU(), P(2),
        )
        # the ReLUs are fused into the conv epilogues; the modules stay for the reference layout
        self.features[1] = nn.Identity()
        self.features[4] = nn.Identity()
        self.features[5].flatten_out = True   # native pool writes NCHW: the flatten below is a view
        self.fc1 = Linear(16 * 5 * 5, 120, activation="relu")
        self.fc2 = Linear(120, 84, activation="relu")
        self.fc3 = Linear(84, num_classes)
        if dropout:   # after fc1 and after fc2
            self.drop1 = Dropout(dropout)
            self.drop2 = Dropout(dropout)

    def forward(self, x):
        x = self.features(x)
        x = x.flatten(1)
        if hasattr(self, "drop1"):
            return self.fc3(self.drop2(self.fc2(self.drop1(self.fc1(x)))))
        return self.fc3(self.fc2(self.fc1(x)))
