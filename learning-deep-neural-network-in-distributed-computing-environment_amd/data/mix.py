"""Batch mixing: Mixup (Zhang et al. 2018) and CutMix (Yun et al. 2019), one plan per batch.

``BatchMix.plan`` draws a host-side plan (``lam``, a permutation of the batch, CutMix's box);
``BatchMix.apply`` turns a batch ``(x [B, C, H, W], y [B])`` into ``(x_mixed, q)`` with dense
soft targets ``q [B, num_classes]`` (fp32) for the soft-target cross-entropy:

    mixup :  x_mixed[i] = lam x[i] + (1 - lam) x[perm[i]]
    cutmix:  x_mixed[i] = x[perm[i]] inside the box, x[i] outside
    q[i]    = lam onehot(y[i]) + (1 - lam) onehot(y[perm[i]])

On the GPU that is one native launch (csrc/kernels/mix.hip); elsewhere the same function in
torch ops on the same plan.  The plan applies to the whole batch, not per sample (timm's
"batch" mode, torchvision's reference transforms).
"""
from __future__ import annotations

import math
from dataclasses import dataclass

import numpy as np
import torch

from ..ops import _ext

MODE_NONE, MODE_MIXUP, MODE_CUTMIX = "none", "mixup", "cutmix"


@dataclass(frozen=True)
class MixPlan:
    """One batch's draws.  ``box`` = (y0, y1, x0, x1): rows [y0, y1) x columns [x0, x1) come from
    the permuted image (empty unless ``mode == 'cutmix'``); ``lam`` weighs the targets (and the
    images under mixup)."""
    mode: str
    lam: float
    perm: np.ndarray
    box: tuple

    @property
    def cutmix(self) -> bool:
        return self.mode == MODE_CUTMIX


def ldq_for(num_classes: int) -> int:
    """Row stride of the soft targets: the class count rounded up to 4 floats (16-byte rows)."""
    return (int(num_classes) + 3) // 4 * 4


class BatchMix:
    """Mixup / CutMix with timm's parameters: ``mixup_alpha`` / ``cutmix_alpha`` > 0 turn the
    modes on (lam ~ Beta(alpha, alpha)), ``prob`` is the probability that a batch is mixed at
    all, ``switch_prob`` the probability of CutMix when both are on."""

    def __init__(self, mixup_alpha: float = 0.0, cutmix_alpha: float = 0.0, prob: float = 1.0,
                 switch_prob: float = 0.5, num_classes: int | None = None):
        mixup_alpha, cutmix_alpha, prob, switch_prob = map(float, (mixup_alpha, cutmix_alpha, prob, switch_prob))
        if not (mixup_alpha >= 0.0 and cutmix_alpha >= 0.0 and math.isfinite(mixup_alpha)
                and math.isfinite(cutmix_alpha)):
            raise ValueError(f"mixup_alpha / cutmix_alpha must be finite and >= 0, got {mixup_alpha}, {cutmix_alpha}")
        if mixup_alpha == 0.0 and cutmix_alpha == 0.0:
            raise ValueError("BatchMix needs mixup_alpha > 0 or cutmix_alpha > 0")
        if not 0.0 <= prob <= 1.0 or not 0.0 <= switch_prob <= 1.0:
            raise ValueError(f"prob and switch_prob must be in [0, 1], got {prob}, {switch_prob}")
        if num_classes is not None and int(num_classes) < 1:
            raise ValueError("BatchMix needs num_classes >= 1 (the width of the soft targets)")
        self.mixup_alpha, self.cutmix_alpha = mixup_alpha, cutmix_alpha
        self.prob, self.switch_prob = prob, switch_prob
        # (None: the DeviceLoader it is given to fills in its dataset's class count)
        self.num_classes = None if num_classes is None else int(num_classes)

    def with_classes(self, num_classes: int) -> "BatchMix":
        """This configuration with the width of the soft targets set."""
        return BatchMix(self.mixup_alpha, self.cutmix_alpha, self.prob, self.switch_prob, num_classes)

    def __repr__(self):
        return (f"BatchMix(mixup_alpha={self.mixup_alpha}, cutmix_alpha={self.cutmix_alpha}, prob={self.prob}, "
                f"switch_prob={self.switch_prob}, num_classes={self.num_classes})")

    def plan(self, batch_seed: int, B: int, H: int, W: int) -> MixPlan:
        """The plan of one batch: a pure function of ``batch_seed`` (and B, H, W).

        All draws come from ``rng = np.random.default_rng(batch_seed)``, in this fixed order (a
        draw is skipped only where stated):

        1. apply?   ``rng.random() < prob``.  If not: lam = 1, no box, the identity
           permutation, and nothing more is drawn.
        2. mode     with both alphas > 0: cutmix if ``rng.random() < switch_prob`` else mixup;
           with one alpha > 0 that mode, and nothing is drawn.
        3. lam      ``rng.beta(a, a)`` with the chosen mode's alpha.
        4. perm     ``rng.permutation(B)``.
        5. box      (cutmix only; timm's rand_bbox) r = sqrt(1 - lam), cut_h = int(H r),
           cut_w = int(W r), ``cy = rng.integers(H)``, ``cx = rng.integers(W)``;
           rows [clip(cy - cut_h // 2, 0, H), clip(cy + cut_h // 2, 0, H)), columns likewise
           from cx and cut_w; then lam = 1 - box_area / (H W)."""
        B, H, W = int(B), int(H), int(W)
        rng = np.random.default_rng(int(batch_seed))
        if not rng.random() < self.prob:
            return MixPlan(MODE_NONE, 1.0, np.arange(B, dtype=np.int64), (0, 0, 0, 0))
        if self.mixup_alpha > 0.0 and self.cutmix_alpha > 0.0:
            cut = bool(rng.random() < self.switch_prob)
        else:
            cut = self.cutmix_alpha > 0.0
        a = self.cutmix_alpha if cut else self.mixup_alpha
        lam = float(rng.beta(a, a))
        perm = rng.permutation(B).astype(np.int64)
        if not cut:
            return MixPlan(MODE_MIXUP, lam, perm, (0, 0, 0, 0))
        r = math.sqrt(1.0 - lam)
        cut_h, cut_w = int(H * r), int(W * r)
        cy, cx = int(rng.integers(H)), int(rng.integers(W))
        y0, y1 = int(np.clip(cy - cut_h // 2, 0, H)), int(np.clip(cy + cut_h // 2, 0, H))
        x0, x1 = int(np.clip(cx - cut_w // 2, 0, W)), int(np.clip(cx + cut_w // 2, 0, W))
        lam = 1.0 - (y1 - y0) * (x1 - x0) / float(H * W)
        return MixPlan(MODE_CUTMIX, lam, perm, (y0, y1, x0, x1))

    def apply(self, x: torch.Tensor, y: torch.Tensor, plan: MixPlan):
        """(x_mixed, q) of one batch under ``plan``; q is the [B, num_classes] view of a
        [B, ldq_for(num_classes)] buffer (zero pad columns, 16-byte rows)."""
        if self.num_classes is None:
            raise ValueError("BatchMix.apply needs num_classes (BatchMix(..., num_classes=C) or with_classes)")
        perm = torch.as_tensor(plan.perm, dtype=torch.long).to(x.device, non_blocking=True)
        if (x.is_cuda and x.dim() == 4 and x.is_contiguous() and x.dtype in (torch.float32, torch.bfloat16)
                and _ext.use_native(x)):
            return mix_native(x, y, perm, plan, self.num_classes)
        return mix_reference(x, y, perm, plan, self.num_classes)


def mix_native(x, y, perm, plan: MixPlan, num_classes: int):
    """One mix.hip launch: the mixed batch and the soft targets."""
    out = torch.empty_like(x)
    q = torch.empty(x.shape[0], ldq_for(num_classes), dtype=torch.float32, device=x.device)
    y0, y1, x0, x1 = plan.box
    _ext.C().batch_mix(x, perm, y, out, q, plan.cutmix, float(plan.lam), y0, y1, x0, x1)
    return out, q[:, :num_classes]


def mix_reference(x, y, perm, plan: MixPlan, num_classes: int):
    """mix_native in torch ops (the CPU twin, and the loader's path off the GPU): fp32
    arithmetic rounded once to x's dtype under mixup, copies under cutmix."""
    B = x.shape[0]
    lam = float(plan.lam)
    if plan.cutmix:
        y0, y1, x0, x1 = plan.box
        out = x.clone()
        out[:, :, y0:y1, x0:x1] = x[perm][:, :, y0:y1, x0:x1]
    elif lam == 1.0:
        out = x.clone()
    else:
        l32 = torch.tensor(lam, dtype=torch.float32)
        out = (l32 * x.float() + (1.0 - l32) * x[perm].float()).to(x.dtype)
    q = torch.zeros(B, ldq_for(num_classes), dtype=torch.float32, device=x.device)
    rows = torch.arange(B, device=x.device)
    yp = y[perm]
    l32 = torch.tensor(lam, dtype=torch.float32, device=x.device)
    q[rows, y] = l32
    q[rows, yp] = torch.where(yp == y, torch.ones_like(l32), 1.0 - l32)
    return out, q[:, :num_classes]
