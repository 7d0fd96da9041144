"""Class weights for the weighted cross-entropy from a shard's label histogram (--class_weights).

Pure NumPy on host labels: no random numbers, no device.  Under the class-skewed partitions
every rank computes the weights of ITS shard, so the ranks' weights differ on purpose."""
from __future__ import annotations

import math

import numpy as np

RULES = ("balanced", "sqrt")


def class_weights_from_labels(labels, num_classes: int, rule: str) -> np.ndarray:
    """fp32 [num_classes] weights of ``labels`` (integers in [0, num_classes)) by ``rule``:

    balanced: n / (C_present * n_c) -- sklearn's ``class_weight="balanced"`` restricted to the
        C_present classes that occur (n samples, n_c of class c).  The mean per-sample weight is 1.
    sqrt: 1 / sqrt(n_c), scaled so that the mean per-sample weight is 1: a milder correction.

    A class that does not occur gets 0 (it cannot appear in a loss over this shard); an empty
    ``labels`` gives all zeros."""
    if rule not in RULES:
        raise ValueError(f"class weights: unknown rule {rule!r} (one of {', '.join(RULES)})")
    num_classes = int(num_classes)
    y = np.asarray(labels).reshape(-1).astype(np.int64)
    if y.size and (y.min() < 0 or y.max() >= num_classes):
        raise ValueError(f"class weights: labels must lie in [0, {num_classes})")
    n_c = np.bincount(y, minlength=num_classes).astype(np.float64)
    present = n_c > 0
    w = np.zeros(num_classes, dtype=np.float64)
    if not present.any():
        return w.astype(np.float32)
    n = float(y.size)
    if rule == "balanced":
        w[present] = n / (present.sum() * n_c[present])
    else:
        w[present] = 1.0 / np.sqrt(n_c[present])
        w *= n / float((w * n_c).sum())   # mean over the samples of w[y] = 1
    return w.astype(np.float32)


def parse_class_weights(spec: str, num_classes: int | None = None):
    """The --class_weights value: None for ``none``, the rule's name for ``balanced`` / ``sqrt``,
    or the fp32 array of a comma-separated list (finite, >= 0, ``num_classes`` long when that is
    given).  A ValueError names what is wrong."""
    spec = str(spec).strip()
    if spec == "none":
        return None
    if spec in RULES:
        return spec
    try:
        vals = [float(v) for v in spec.split(",")]
    except ValueError:
        raise ValueError(f"--class_weights takes none, {', '.join(RULES)} or a comma-separated list of floats, "
                         f"got {spec!r}") from None
    if any(not math.isfinite(v) or v < 0 for v in vals):
        raise ValueError(f"--class_weights: the weights must be finite and >= 0, got {spec!r}")
    if num_classes is not None and len(vals) != int(num_classes):
        raise ValueError(f"--class_weights: {int(num_classes)} weights expected (one per class), got {len(vals)}")
    return np.asarray(vals, dtype=np.float32)
