"""Autograd-aware ops on the native gfx950 kernels (generic, module-driven path).

Each op has two implementations:
  * GPU: the hand-written HIP kernels (bf16 activations, fp32 accumulation,
    weight gradients written straight into the FlatParams gradient buffer --
    autograd never allocates or accumulates a weight gradient tensor);
  * CPU: the plain PyTorch fp32 reference (used by the orchestration tests and
    as the numerics oracle of the GPU tests).

Reference call sites replaced: nn.Linear + F.relu / sigmoid
(K10, K13; BAR/model.py:68-71,100), nn.CrossEntropyLoss fwd/bwd + argmax
bookkeeping (K14, K15; BAR/trainer.py:207-216).
"""
from __future__ import annotations

import math
import os

import torch
import torch.nn.functional as F

from . import _ext

ACTS = {"none": None, "relu": 0, "sigmoid": 1}


def _fire_pre_hooks(mods, x) -> bool:
    """A fused launch that stands in for the __call__ of several modules (conv2d_pair,
    gap_linear) must still run their forward pre-hooks: the sharded DP step cuts its graph
    chain there and waits for the bucket's weight all-gather (GraphedDPStep._on_forward).
    Fires every module's pre-hooks with (x,) and returns True, or returns False without
    firing any when a module carries hooks a fused launch cannot honour (post-forward
    hooks, kwargs pre-hooks, global module hooks): the caller then runs the module calls."""
    from torch.nn.modules import module as _m

    if _m._global_forward_pre_hooks or _m._global_forward_hooks:
        return False
    for mod in mods:
        if mod._forward_hooks or getattr(mod, "_forward_pre_hooks_with_kwargs", None):
            return False
    for mod in mods:
        for hook in tuple(mod._forward_pre_hooks.values()):
            if hook(mod, (x,)) is not None:
                raise RuntimeError(f"a forward pre-hook of {type(mod).__name__} rewrote its input: "
                                   "not supported on the fused launch")
    return True


def _to_bf16(x: torch.Tensor) -> torch.Tensor:
    """The cast alone: strides and memory format stay (a channels_last tensor stays NHWC)."""
    return x if x.dtype == torch.bfloat16 else x.to(torch.bfloat16)


def _from_bf16(t: torch.Tensor, dtype) -> torch.Tensor:
    """A native op's bf16 result (a gradient) in the dtype its consumer handed in."""
    return t if dtype == torch.bfloat16 else t.to(dtype)


def _bf16_rows(x: torch.Tensor) -> torch.Tensor:
    """bf16 with a unit last stride, copying only if needed (GEMM and row-kernel operands)."""
    if x.dtype == torch.bfloat16:
        return x if x.stride(-1) == 1 else x.contiguous()
    return x.to(torch.bfloat16).contiguous()


def _padded_rows_view(g: torch.Tensor, npad: int, zero_pad_guaranteed: bool = True) -> torch.Tensor:
    """[B, N] tensor -> [B, npad] (npad >= N, multiple of 8), copying only if needed.

    A [B, N] view whose row stride is already npad was produced by an ldnn op on
    a padded [B, npad] buffer and is widened in place.  Gradients written by
    ldnn ops have zero padding; forward activations may carry arbitrary (finite)
    values there, which is harmless because the matching weight columns are 0."""
    B, N = g.shape
    if N == npad and g.is_contiguous():
        return g
    if g.stride(1) == 1 and g.stride(0) == npad and g.dtype == torch.bfloat16 and zero_pad_guaranteed:
        return g.as_strided((B, npad), (npad, 1), g.storage_offset())
    out = torch.zeros(B, npad, dtype=torch.bfloat16, device=g.device)
    out[:, :N].copy_(g)
    return out


class _LinearActNative(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias, act, flat):
        C = _ext.C()
        x = _bf16_rows(x)
        w = flat.shadow_storage(weight)
        npad, kpad = w.shape
        K = weight.shape[1]
        assert x.shape[-1] == K, f"Linear expects {K} input features, got {x.shape[-1]}"
        x2 = x.reshape(-1, K)
        if kpad != K:
            # pad columns must be 0 so the weight-gradient pad columns stay exactly 0
            # (the producer's pad may hold e.g. sigmoid(0) = 0.5)
            zp = getattr(x, "_ldnn_zpad", False)
            x2 = _padded_rows_view(x2, kpad)
            if not zp:
                # through .data: the producer saved this buffer for its own backward and
                # its pad columns never influence that backward (their gradient is 0)
                x2.data[:, K:].zero_()
        y = torch.empty(x2.shape[0], npad, dtype=torch.bfloat16, device=x.device)
        if bias is not None:
            b = flat.master_storage(bias)
        else:
            b = torch.zeros(npad, dtype=torch.float32, device=x.device)
        epi = {None: C.EPI_BIAS, 0: C.EPI_BIAS_RELU, 1: C.EPI_BIAS_SIGMOID}[act]
        # (a split-K forward with the in-launch combine for the 64 x 512 -> 1000 classifier
        # measured slower standalone and neutral in the ResNet-18 step: removed in round 4,
        # profiles/r3s3/head_micro.jsonl)
        C.gemm(x2, w, y, True, True, epi, bias=b)
        ctx.save_for_backward(x2, y)
        ctx.act, ctx.flat, ctx.weight, ctx.bias = act, flat, weight, bias
        ctx.xshape = x.shape
        n = weight.shape[0]
        out = y if n == npad else y[:, :n]
        out = out.reshape(*x.shape[:-1], n)
        if act != 1 and n != npad and out.dim() == 2:
            # pad rows of W and pad entries of b are exactly 0 (their gradients are), so the
            # pad columns hold act(0) = 0: a padded consumer skips re-zeroing them
            out._ldnn_zpad = True
        return out

    @staticmethod
    def backward(ctx, gy):
        C = _ext.C()
        x2, y = ctx.saved_tensors
        flat, weight, bias = ctx.flat, ctx.weight, ctx.bias
        npad = y.shape[1]
        g = _padded_rows_view(_bf16_rows(gy.reshape(-1, gy.shape[-1])), npad)
        if ctx.act is not None:
            gz = torch.empty_like(y)
            if bias is not None:   # activation backward + the bias gradient's column sums in one pass
                C.act_bwd_colsum(g.contiguous(), y, gz, flat.grad_storage(bias), ctx.act,
                                 flat.grad_beta(bias) != 0.0)
            else:
                C.act_bwd(g.contiguous(), y, gz, ctx.act)
        else:
            gz = g.contiguous()
            if bias is not None:
                C.colsum(gz, flat.grad_storage(bias), flat.grad_beta(bias) != 0.0)
        # weight grad straight into the flat fp32 gradient buffer (accumulate, or
        # overwrite as the step's first write: FlatParams.grad_beta)
        C.gemm(gz, x2, flat.grad_storage(weight), False, False, beta=flat.grad_beta(weight))
        flat.notify(weight, bias)
        dx = None
        if ctx.needs_input_grad[0]:
            dx = torch.empty(x2.shape, dtype=torch.bfloat16, device=x2.device)
            C.gemm(gz, flat.shadow_storage(weight), dx, True, False)
            K = weight.shape[1]
            if dx.shape[1] != K:
                dx = dx[:, :K]
            dx = dx.reshape(ctx.xshape)
        return dx, None, None, None, None


def linear_act(x, weight, bias=None, act: str = "none", flat=None):
    """y = act(x @ W^T + b); native fused GEMM epilogue on the GPU."""
    a = ACTS[act]
    if _ext.use_native(x):
        if flat is None or flat.shadow is None:
            raise RuntimeError("native Linear needs the model attached to FlatParams (ldnn.prepare(model))")
        return _LinearActNative.apply(x, weight, bias, a, flat)
    y = F.linear(x.float(), weight, bias)
    if a == 0:
        y = F.relu(y)
    elif a == 1:
        y = torch.sigmoid(y)
    return y


def _flat_dense(t: torch.Tensor) -> torch.Tensor | None:
    """A 1-D view over the storage of a dense tensor (row-major or channels_last)."""
    if t.is_contiguous():
        return t.view(-1)
    if t.dim() == 4 and t.is_contiguous(memory_format=torch.channels_last):
        return t.permute(0, 2, 3, 1).reshape(-1)
    return None


class _ActNative(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, act):
        C = _ext.C()
        xb = _to_bf16(x)
        if _flat_dense(xb) is None:
            xb = xb.contiguous()
        y = torch.empty_like(xb)  # keeps the memory format (channels_last stays NHWC)
        C.act_fwd(_flat_dense(xb), _flat_dense(y), act)
        ctx.save_for_backward(y)
        ctx.act = act
        ctx.in_dtype = x.dtype
        return y

    @staticmethod
    def backward(ctx, gy):
        (y,) = ctx.saved_tensors
        g = _to_bf16(gy)
        if g.stride() != y.stride():
            g = g.contiguous(memory_format=torch.channels_last) if y.dim() == 4 and not y.is_contiguous() \
                else g.contiguous()
        dx = torch.empty_like(y)
        _ext.C().act_bwd(_flat_dense(g), _flat_dense(y), _flat_dense(dx), ctx.act)
        return dx.to(ctx.in_dtype), None


def relu(x):
    if _ext.use_native(x):
        return _ActNative.apply(x, 0)
    return F.relu(x)


def sigmoid(x):
    if _ext.use_native(x):
        return _ActNative.apply(x, 1)
    return torch.sigmoid(x)


class _SoftmaxXentNative(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, labels, stats, label_smoothing=0.0, weight=None, ignore_index=-100, focal_gamma=0.0):
        C = _ext.C()
        B, n = logits.shape
        lg = _bf16_rows(logits)
        ld = lg.stride(0)
        dfull = torch.empty(B * ld, dtype=torch.bfloat16, device=lg.device).view(B, ld)
        # one launch: the kernel's last block writes [mean loss, #correct] into `out`
        # and adds [loss sum, #correct] into `stats` (no fill / divide / add kernels)
        out = torch.empty(2, dtype=torch.float32, device=lg.device)
        if labels.dim() == 2:   # class-probability targets (validated by cross_entropy): no gradient for them
            q = labels if labels.dtype == torch.float32 else labels.float()
            if q.stride(1) != 1:
                q = q.contiguous()
            if weight is not None:   # (ignore_index does not apply to probability targets, as in torch)
                C.softmax_xent_soft_w(lg, q, dfull[:, :n], stats, None, n, 1.0 / B, loss_out=out, loss_scale=1.0 / B,
                                      label_smoothing=label_smoothing, weight=weight)
            else:
                C.softmax_xent_soft(lg, q, dfull[:, :n], stats, None, n, 1.0 / B, loss_out=out, loss_scale=1.0 / B,
                                    label_smoothing=label_smoothing)
        elif focal_gamma > 0.0:
            # the weighted pair of launches with the focal instances (labels, no smoothing: cross_entropy checks)
            C.softmax_xent_focal(lg, labels, dfull[:, :n], stats, None, n, gamma=focal_gamma, weight=weight,
                                 ignore_index=ignore_index, loss_out=out)
        elif weight is not None or ignore_index != -100:
            # two launches: the pre-pass sums the kept rows' weights on the device, the loss kernel
            # divides by that (no host divisor: the batch's weight sum is not known here)
            C.softmax_xent_w(lg, labels, dfull[:, :n], stats, None, n, loss_out=out, label_smoothing=label_smoothing,
                             weight=weight, ignore_index=ignore_index)
        else:
            C.softmax_xent(lg, labels, dfull[:, :n], stats, None, n, 1.0 / B, loss_out=out, loss_scale=1.0 / B,
                           label_smoothing=label_smoothing)
        ctx.save_for_backward(dfull)
        ctx.n, ctx.in_dtype = n, logits.dtype
        return out[0]

    @staticmethod
    def backward(ctx, go):
        (dfull,) = ctx.saved_tensors
        if ctx.in_dtype == torch.bfloat16 and getattr(go, "_ldnn_unit", False):
            # the graphed steps' persistent seed is exactly 1 (train.graphed.unit_seed): the
            # forward's d(mean loss)/d(logits) is the gradient as is, no scaling pass
            return dfull[:, : ctx.n], None, None, None, None, None, None
        if ctx.in_dtype == torch.bfloat16 and go.dtype == torch.float32 and go.is_cuda and dfull.numel() % 8 == 0:
            # d = dlogits * grad_output in one pass over the padded rows (pad stays 0)
            full = torch.empty_like(dfull)
            _ext.C().scale_bf16(dfull, go.reshape(1), full)
            return full[:, : ctx.n], None, None, None, None, None, None
        d = dfull[:, : ctx.n]
        d = (d.float() * go).to(torch.bfloat16) if ctx.in_dtype == torch.bfloat16 else d.float() * go
        if ctx.in_dtype == torch.bfloat16 and dfull.stride(0) != ctx.n:
            full = torch.zeros_like(dfull)
            full[:, : ctx.n] = d
            d = full[:, : ctx.n]
        return d, None, None, None, None, None, None


class _FocalFallback(torch.autograd.Function):
    """The focal loss of cross_entropy(focal_gamma > 0) in fp32 torch ops, with the closed-form gradient
    the kernels use: autograd through (1 - p) ** gamma gives NaN at p == 1 for gamma < 1."""

    @staticmethod
    def forward(ctx, lf, labels, weight, ignore_index, gamma):
        ncls = lf.shape[1]
        kept = (labels != ignore_index) & (labels >= 0) & (labels < ncls)
        safe = torch.where(kept, labels, torch.zeros_like(labels))
        hot = F.one_hot(safe, ncls).bool()
        lse = torch.logsumexp(lf, 1)
        xl = lf.gather(1, safe[:, None])[:, 0]
        # q = 1 - p from the other classes' exponentials (no cancellation); a single class has q = 0
        q = (torch.exp(torch.logsumexp(lf.masked_fill(hot, float("-inf")), 1) - lse) if ncls > 1
             else torch.zeros_like(lse))
        p = torch.exp(xl - lse)
        pos = q >= torch.finfo(lf.dtype).tiny   # below: p rounds to 1, the row contributes nothing
        qs = torch.where(pos, q, torch.ones_like(q))
        nlp = torch.where(q < 0.5, -torch.log1p(-q), lse - xl)
        m = torch.where(pos, qs ** gamma, torch.zeros_like(q))
        f = m + (gamma * m) * (p * (nlp / qs))
        a = kept.to(lf.dtype) if weight is None else weight[safe] * kept
        den = a.sum()
        inv = torch.where(den > 0, 1.0 / torch.where(den > 0, den, torch.ones_like(den)), torch.zeros_like(den))
        ctx.save_for_backward((a * f * inv)[:, None] * (torch.softmax(lf, 1) - hot.to(lf.dtype)))
        ctx.mark_non_differentiable(kept)
        return (a * m * nlp).sum() * inv, kept

    @staticmethod
    def backward(ctx, go, _):
        (d,) = ctx.saved_tensors
        return d * go, None, None, None, None


def _soft_target(logits, target) -> bool:
    """torch's dispatch on the target: an integer [B] tensor holds class indices (False), a
    floating [B, C] tensor class probabilities (True); anything else is refused."""
    if not target.is_floating_point() and not target.is_complex() and target.dim() == 1:
        return False
    if logits.dim() == 2 and target.is_floating_point() and target.shape == logits.shape:
        if target.requires_grad:
            raise ValueError("cross_entropy: class-probability targets get no gradient; detach the target")
        return True
    raise ValueError(f"cross_entropy: logits {tuple(logits.shape)} ({logits.dtype}) take class indices "
                     f"[{logits.shape[0]}] (integer) or class probabilities {tuple(logits.shape)} (floating), "
                     f"got a target {tuple(target.shape)} ({target.dtype})")


def cross_entropy(logits, labels, stats: torch.Tensor | None = None, label_smoothing: float = 0.0,
                  weight: torch.Tensor | None = None, ignore_index: int = -100, focal_gamma: float = 0.0):
    """Mean softmax cross-entropy.  `stats` (device fp32, >= 2) accumulates
    [sum of per-sample loss, #correct] without a host sync.  `label_smoothing` in [0, 1]:
    torch's smoothed targets eps / C + (1 - eps) * onehot (the loss, its gradient and the
    accumulated loss sum are the smoothed ones; #correct is unaffected).

    The target is dispatched as torch does: an integer [B] tensor holds class indices, a
    floating [B, C] tensor class probabilities (rows are not normalised; smoothing applies to
    them too).  Under probability targets #correct counts the rows whose logits' argmax is the
    target row's (first-index) argmax: agreement with the dominant label.

    `weight` (fp32 [C], finite and >= 0: the caller's contract) and `ignore_index` are torch's: with
    k_r = 0 for a row whose label is `ignore_index` (else 1) and q' the smoothed target row,
    loss = sum_r k_r sum_c w_c q'_rc (lse_r - x_rc) / sum_r k_r w[y_r] over labels, and
    sum_r sum_c w_c q'_rc (lse_r - x_rc) / B over probability targets (where `ignore_index` does not
    apply).  `stats[0]` gains B * loss, `stats[1]` #correct over the kept rows.  Two departures from
    torch: when nothing is kept, or every kept class has weight 0, the loss and its gradient are 0
    (torch: NaN, which would poison every weight of a replayed step); and on the GPU a label
    outside [0, C) that is not `ignore_index` counts as ignored (torch: a device assert).  With
    `weight=None, ignore_index=-100` (the defaults) the call is the unweighted one, launch for launch.

    `focal_gamma` (finite, >= 0; integer labels only, no label smoothing: ValueError otherwise) turns the
    loss into the focal loss of Lin et al. 2017 on the weighted path: with p = softmax(x_r)[y_r],
    loss = sum_r k_r w[y_r] (1 - p)^gamma (-log p) / sum_r k_r w[y_r], everything else (`weight`,
    `ignore_index`, the divisor, `stats`, the two departures) as above.  A row whose 1 - p underflows
    contributes 0 and gets a zero gradient row.  0 (the default) is the call without it, launch for launch."""
    label_smoothing = float(label_smoothing)
    ignore_index = int(ignore_index)
    focal_gamma = float(focal_gamma)
    if not (focal_gamma >= 0.0 and math.isfinite(focal_gamma)):
        raise ValueError(f"cross_entropy: focal_gamma must be finite and >= 0, got {focal_gamma}")
    if weight is not None and (weight.dim() != 1 or weight.shape[0] != logits.shape[-1]):
        raise ValueError(f"cross_entropy: weight must hold one value per class [{logits.shape[-1]}], got "
                         f"{tuple(weight.shape)}")
    if not 0.0 <= label_smoothing <= 1.0:
        raise ValueError(f"label_smoothing must be in [0, 1], got {label_smoothing}")
    soft = _soft_target(logits, labels)
    if focal_gamma > 0.0 and (soft or label_smoothing > 0.0):
        raise ValueError("cross_entropy: focal_gamma > 0 takes integer labels and label_smoothing == 0 (there is no "
                         "agreed focal loss over class-probability targets or smoothed ones), got "
                         + (f"a {tuple(labels.shape)} {labels.dtype} target" if soft
                            else f"label_smoothing={label_smoothing}"))
    if _ext.use_native(logits):
        if focal_gamma > 0.0:
            return _SoftmaxXentNative.apply(logits, labels, stats, label_smoothing, weight, ignore_index, focal_gamma)
        return _SoftmaxXentNative.apply(logits, labels, stats, label_smoothing, weight, ignore_index)
    lf = logits.float()
    kept = None
    if focal_gamma > 0.0:
        loss, kept = _FocalFallback.apply(lf, labels, None if weight is None else weight.to(lf.device, lf.dtype),
                                          ignore_index, focal_gamma)
    elif weight is None and (soft or ignore_index == -100):
        loss = F.cross_entropy(lf, labels.float() if soft else labels, label_smoothing=label_smoothing)
    elif soft:
        loss = F.cross_entropy(lf, labels.float(), weight=weight.to(lf.device, lf.dtype),
                               label_smoothing=label_smoothing)
    else:
        # torch's weighted mean is its weighted sum over the kept rows' weight sum; dividing here
        # gives 0 (not 0 / 0) when that sum is 0, without reading it on the host
        w = None if weight is None else weight.to(lf.device, lf.dtype)
        kept = labels != ignore_index
        safe = torch.where(kept, labels, torch.zeros_like(labels))
        den = (kept.to(lf.dtype) if w is None else w[safe] * kept).sum()
        tot = F.cross_entropy(lf, labels, weight=w, ignore_index=ignore_index, reduction="sum",
                              label_smoothing=label_smoothing)
        loss = tot / torch.where(den > 0, den, torch.ones_like(den))
    if stats is not None:
        with torch.no_grad():
            hit = lf.argmax(1) == (labels.argmax(1) if soft else labels)
            stats[0] += loss.detach() * labels.shape[0]
            stats[1] += (hit if kept is None else hit & kept).sum()
    return loss


# ------------------------------------------------------------------ conv / BN
def _up8(v: int) -> int:
    return (v + 7) // 8 * 8


def as_nhwc(t: torch.Tensor, cp: int, zero_pad: bool = True) -> torch.Tensor:
    """Logical [N, C, H, W] tensor -> dense NHWC bf16 buffer [N, H, W, cp].

    Channels-last tensors (ours, or torch's channels_last outputs) are widened
    in place when their channel stride already is cp; anything else is copied
    into a zero-padded buffer."""
    N, C, H, W = t.shape
    if (t.dtype == torch.bfloat16 and t.stride(1) == 1 and t.stride(3) == cp and t.stride(2) == W * cp
            and t.stride(0) == H * W * cp):
        buf = t.as_strided((N, H, W, cp), (H * W * cp, W * cp, cp, 1), t.storage_offset())
        if zero_pad and cp > C and not getattr(t, "_ldnn_zpad", False):
            buf.data[..., C:].zero_()
        return buf
    if (cp % 8 == 0 and t.is_contiguous() and t.dtype in (torch.float32, torch.bfloat16)
            and _ext.use_native(t)):
        # one native pass: gather + cast + zeroed pad channels (no fill + permute copy)
        buf = torch.empty(N, H, W, cp, dtype=torch.bfloat16, device=t.device)
        _ext.C().nchw_to_nhwc(t, buf)
        return buf
    buf = torch.zeros(N, H, W, cp, dtype=torch.bfloat16, device=t.device) if cp > C else \
        torch.empty(N, H, W, cp, dtype=torch.bfloat16, device=t.device)
    buf[..., :C].copy_(t.permute(0, 2, 3, 1))
    return buf


def nchw_view(buf: torch.Tensor, c: int) -> torch.Tensor:
    """Dense NHWC buffer -> logical [N, c, H, W] view (channels_last strides)."""
    return buf[..., :c].permute(0, 3, 1, 2)


def _zpad(t: torch.Tensor) -> torch.Tensor:
    """Mark a native op's NHWC output whose pad channels (c .. cp-1) are exactly zero by
    construction (zero weight rows / bias entries, pooling or gradients of zero pads), so
    its consumer's as_nhwc skips the pad-clearing launch."""
    t._ldnn_zpad = True
    return t


def _bn_train_state(mod, dev):
    """(running_mean, running_var, momentum, num_batches tensor) of a training-mode BN
    forward, with the Python-side bookkeeping of one call (num_batches_tracked)."""
    mom = mod.momentum
    nbt = None
    if mod.training and mod.track_running_stats:
        # num_batches_tracked += 1 happens inside the fused BN statistics kernel
        nbt = mod.num_batches_tracked if mod.num_batches_tracked.is_cuda else None
        if nbt is None:
            mod.num_batches_tracked.add_(1)
        mod._ldnn_nbt = getattr(mod, "_ldnn_nbt", 0) + 1
        if mom is None:
            mom = 1.0 / mod._ldnn_nbt
    rm = mod.running_mean if mod.track_running_stats else None
    rv = mod.running_var if mod.track_running_stats else None
    return rm, rv, mom, nbt


def _fused_bn_ok(bn, K: int, kp: int, bias, relu: bool) -> bool:
    return (bn is not None and bn.training and bn.affine and kp == K == bn.num_features and bias is None
            and not relu and getattr(bn, "_ldnn_flat", None) is not None)


# The dgrad of a conv whose input is a training BatchNorm(+ReLU)'s output takes that BN's
# backward statistics in its epilogue (conv2d_dgrad with a BnBwdFuse), and the BN backward runs
# its apply pass alone -- one reduce launch less per such pair (LDNN_CONV_BN_BWD=0: off)
CONV_BN_BWD = os.environ.get("LDNN_CONV_BN_BWD", "1") != "0"
BN_BWD_FUSED = [0]   # BN backwards that found their statistics finalized by a dgrad (tests)


class _BnBwdSrc:
    """What a consumer conv's dgrad needs to take a BN's backward statistics (attached to the
    BN's primary output as ``_ldnn_bnsrc``).  ``twin_used``: the output also feeds a shortcut
    (its gradient arrives in two parts, so only the BN's own reduce sees the sum)."""

    __slots__ = ("mod", "flat", "weight", "bias", "x2", "mask", "smean", "sinv", "ws", "C", "twin_used", "pre")

    def __init__(self, mod, flat, weight, bias, x2, mask, smean, sinv, ws, C):
        self.mod, self.flat, self.weight, self.bias = mod, flat, weight, bias
        self.x2, self.mask, self.smean, self.sinv, self.ws, self.C = x2, mask, smean, sinv, ws, C
        self.twin_used = False
        self.pre = None   # (dx pointer, version) of a dgrad that finalized the statistics

    def dgrad_kwargs(self):
        """conv_dgrad keyword arguments, or None when the BN's gradients accumulate this step
        (the fused finalize only overwrites: a recomputing fallback must be able to redo it)."""
        f = self.flat
        if not (f.grad_fresh(self.weight) and f.grad_fresh(self.bias)):   # (peeks: the BN's backward consumes)
            return None
        C = self.C
        return dict(bn_x=self.x2, bn_mask=self.mask, bn_ws=self.ws, bn_gamma=f.master_storage(self.weight)[:C],
                    bn_save_mean=self.smean, bn_save_invstd=self.sinv, bn_dgamma=f.grad_storage(self.weight)[:C],
                    bn_dbeta=f.grad_storage(self.bias)[:C], bn_assign=True)


def _conv_bn_stats(bn, K: int, dev, C):
    """(conv_fwd's bn_* arguments without the prefix, bookkeeping state) for a conv whose epilogue
    takes the next training BN's statistics (_fused_bn_ok)."""
    ws = _bn_workspace(bn, K, dev, C)
    smean = torch.empty(K, dtype=torch.float32, device=dev)
    sinv = torch.empty(K, dtype=torch.float32, device=dev)
    bflat = bn._ldnn_flat
    snap = (getattr(bn, "_ldnn_nbt", 0), bn.num_batches_tracked.clone()
            if bn.track_running_stats and not bn.num_batches_tracked.is_cuda else None)
    rm, rv, mom, nbt = _bn_train_state(bn, dev)
    args = dict(ws=ws, gamma=bflat.master_storage(bn.weight)[:K], beta=bflat.master_storage(bn.bias)[:K],
                running_mean=rm, running_var=rv, save_mean=smean, save_invstd=sinv, eps=bn.eps,
                momentum=mom or 0.0, num_batches=nbt)
    return args, (smean, sinv, snap)


def _conv_bn_stats_done(bn, done: bool, y, state):
    smean, sinv, snap = state
    if done:
        bn.__dict__["_ldnn_pre"] = (y.data_ptr(), smean, sinv)
    else:  # generic conv path: the BN runs its own statistics pass (undo the bookkeeping)
        bn._ldnn_nbt = snap[0]
        if snap[1] is not None:
            bn.num_batches_tracked.copy_(snap[1])


def _colsum_ws(flat, bias, cols: int, dev) -> torch.Tensor:
    """A conv bias's persistent colsum scratch (cols floats + a ticket, zeroed once; the kernel leaves it
    zero): its column sums over many row groups then take one launch, no zero fill (elementwise.hip)."""
    cache = flat.__dict__.setdefault("_ldnn_colsum_ws", {})
    ws = cache.get(id(bias))
    if ws is None or ws.device != dev or ws.numel() < cols + 1:
        ws = torch.zeros(cols + 1, dtype=torch.float32, device=dev)
        cache[id(bias)] = ws
    return ws


class _Conv2dNative(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias, stride, pad, flat, relu, bn=None):
        C = _ext.C()
        K, Cin, R, S = weight.shape
        w = flat.shadow_storage(weight)  # [Kp][R][S][Cp]
        kp, cp = w.shape[0], w.shape[3]
        xb = as_nhwc(x, cp)
        N, H, W, _ = xb.shape
        P, Q = (H + 2 * pad - R) // stride + 1, (W + 2 * pad - S) // stride + 1
        y = torch.empty(N, P, Q, kp, dtype=torch.bfloat16, device=x.device)
        b = flat.master_storage(bias) if bias is not None else None
        epi = (C.EPI_BIAS_RELU if relu else C.EPI_BIAS) if b is not None else C.EPI_NONE
        if relu and b is None:
            b = torch.zeros(kp, dtype=torch.float32, device=x.device)
            epi = C.EPI_BIAS_RELU
        xs, packed = None, False
        if (epi == C.EPI_NONE and cp == 8 and R == 7 and S == 7 and stride == 2
                and C.stem_s2d_fwd_ok(N, H, W, cp, kp, R, S, stride, pad, Cin)):
            # a 7x7 / 2 stem: the forward runs on the packed space-to-depth image, which the weight
            # gradient then reuses (conv_stem.hip conv_s2d_ws_kernel / stem_s2d_wgrad_kernel) -- the
            # one a graph's input staging wrote along with x (graphed.static_input), or packed here
            img, ver = getattr(x, "_ldnn_s2d", (None, None))
            if (img is not None and ver == x._version and tuple(img.shape) == (N, P + 3, Q + 3, 16)
                    and img.device == x.device):
                xs, packed = img, True
            else:
                xs = torch.empty(N, P + 3, Q + 3, 16, dtype=torch.bfloat16, device=x.device)
        if _fused_bn_ok(bn, K, kp, bias, relu):
            # the conv epilogue accumulates + finalizes the next BN's batch statistics
            args, state = _conv_bn_stats(bn, K, x.device, C)
            done = C.conv_fwd(xb, w, y, stride, pad, b, epi, real_channels=Cin, s2d_xs=xs, s2d_packed=packed,
                              **{"bn_" + k: v for k, v in args.items()})
            _conv_bn_stats_done(bn, done, y, state)
        else:
            C.conv_fwd(xb, w, y, stride, pad, b, epi, real_channels=Cin, s2d_xs=xs, s2d_packed=packed)
        ctx.save_for_backward(xb, y, xs)
        ctx.meta = (stride, pad, flat, weight, bias, relu, Cin, x.dtype)
        src = getattr(x, "_ldnn_bnsrc", None)
        ctx.bnsrc = src if (CONV_BN_BWD and src is not None and stride == 1 and src.C == cp == Cin) else None
        return nchw_view(y, K)

    @staticmethod
    def backward(ctx, gy):
        C = _ext.C()
        xb, y, xs = ctx.saved_tensors
        stride, pad, flat, weight, bias, relu, Cin, in_dtype = ctx.meta
        kp = y.shape[3]
        g = as_nhwc(_to_bf16(gy), kp)
        if relu:
            gz = torch.empty_like(y)
            if bias is not None:   # ReLU backward + the bias gradient's column sums in one pass
                C.act_bwd_colsum(g.contiguous().view(-1, kp), y.view(-1, kp), gz.view(-1, kp),
                                 flat.grad_storage(bias), 0, flat.grad_beta(bias) != 0.0,
                                 ws=_colsum_ws(flat, bias, kp, y.device))
            else:
                C.act_bwd(g.contiguous(), y, gz, 0)
            g = gz
        elif bias is not None:
            C.colsum(g.contiguous().view(-1, kp), flat.grad_storage(bias), flat.grad_beta(bias) != 0.0,
                     ws=_colsum_ws(flat, bias, kp, g.device))
        dw, beta = flat.grad_storage(weight), flat.grad_beta(weight)
        dx = None
        if ctx.needs_input_grad[0]:
            # dgrad + wgrad of the layer: one launch where the kernels allow (conv_bwd)
            dxb = torch.empty_like(xb)
            src = ctx.bnsrc
            kw = src.dgrad_kwargs() if src is not None and not src.twin_used else None
            if C.conv_bwd(g, flat.shadow_storage(weight), dxb, xb, dw, stride, pad, beta, Cin, **(kw or {})) and kw:
                # the BN's backward finds its statistics finalized if this dx reaches it unchanged
                src.pre = (dxb.data_ptr(), dxb._version)
            ctx.bnsrc = None
            dx = _from_bf16(_zpad(nchw_view(dxb, Cin)), in_dtype)   # (weight pad channels are zero)
        else:
            C.conv_wgrad(g, xb, dw, stride, pad, beta, real_channels=Cin, s2d_xs=xs)
        flat.notify(weight, bias)
        return dx, None, None, None, None, None, None, None


class _Conv2dPairNative(torch.autograd.Function):
    """A downsampling residual block's two convolutions of one input -- the 3x3 (conv0 on x) and
    the 1x1 shortcut (conv1 on x's twin xt) -- as ONE forward launch (conv_fwd2: both GEMMs share
    the chip), each with its BN's fused statistics; the backward runs each conv's dgrad + wgrad
    pair and returns the two input gradients separately (the producer sums them)."""

    @staticmethod
    def forward(ctx, x, xt, w0, w1, flat, meta0, meta1):
        C = _ext.C()
        (st0, p0, bn0), (st1, p1, bn1) = meta0, meta1
        sh0, sh1 = flat.shadow_storage(w0), flat.shadow_storage(w1)
        (kp0, cp), kp1 = (sh0.shape[0], sh0.shape[3]), sh1.shape[0]
        K0, Cin, R0, S0 = w0.shape
        K1, _, R1, S1 = w1.shape
        xb = as_nhwc(x, cp)
        N, H, W, _ = xb.shape
        dev = x.device
        ys, args, states = [], [], []
        for (K, kp, R, S, st, pd, bn) in ((K0, kp0, R0, S0, st0, p0, bn0), (K1, kp1, R1, S1, st1, p1, bn1)):
            P, Q = (H + 2 * pd - R) // st + 1, (W + 2 * pd - S) // st + 1
            ys.append(torch.empty(N, P, Q, kp, dtype=torch.bfloat16, device=dev))
            a, stt = _conv_bn_stats(bn, K, dev, C) if _fused_bn_ok(bn, K, kp, None, False) else (None, None)
            args.append(a)
            states.append(stt)
        done = C.conv_fwd2(xb, sh0, ys[0], st0, p0, sh1, ys[1], st1, p1, args[0], args[1])
        for bn, d, y, stt in zip((bn0, bn1), done, ys, states):
            if stt is not None:
                _conv_bn_stats_done(bn, d, y, stt)
        ctx.save_for_backward(xb)
        ctx.meta = (flat, (w0, st0, p0), (w1, st1, p1), Cin, x.dtype)
        return nchw_view(ys[0], K0), nchw_view(ys[1], K1)

    @staticmethod
    def backward(ctx, g0, g1):
        C = _ext.C()
        (xb,) = ctx.saved_tensors
        flat, c0, c1, Cin, in_dtype = ctx.meta
        if g0 is not None and g1 is not None and ctx.needs_input_grad[0] and ctx.needs_input_grad[1]:
            # both convs' dgrads and wgrads in one launch (conv_bwd2)
            job = []
            for g, (weight, st, pd) in ((g0, c0), (g1, c1)):
                sh = flat.shadow_storage(weight)
                gb = as_nhwc(_to_bf16(g), sh.shape[0])
                job.append((gb, sh, torch.empty_like(xb), flat.grad_storage(weight), st, pd, flat.grad_beta(weight)))
            (ga, sa, xa, wa, sta, pa, ba), (gc, sc, xc, wc, stc, pc, bc) = job
            C.conv_bwd2(xb, ga, sa, xa, wa, sta, pa, ba, gc, sc, xc, wc, stc, pc, bc, Cin)
            flat.notify(c0[0], c1[0])
            dxs = [_from_bf16(_zpad(nchw_view(t, Cin)), in_dtype) for t in (xa, xc)]
            return dxs[0], dxs[1], None, None, None, None, None
        dxs = []
        for k, (g, (weight, st, pd)) in enumerate(((g0, c0), (g1, c1))):
            if g is None:
                dxs.append(None)
                continue
            sh = flat.shadow_storage(weight)
            gb = as_nhwc(_to_bf16(g), sh.shape[0])
            dw, beta = flat.grad_storage(weight), flat.grad_beta(weight)
            if ctx.needs_input_grad[k]:
                dxb = torch.empty_like(xb)
                C.conv_bwd(gb, sh, dxb, xb, dw, st, pd, beta, Cin)
                dx = _zpad(nchw_view(dxb, Cin))
                dxs.append(_from_bf16(dx, in_dtype))
            else:
                C.conv_wgrad(gb, xb, dw, st, pd, beta, real_channels=Cin)
                dxs.append(None)
            flat.notify(weight)
        return dxs[0], dxs[1], None, None, None, None, None


def conv2d_pair(x, xt, mod0, mod1):
    """(mod0(x), mod1(xt)) -- a downsampling block's 3x3 conv and 1x1 shortcut conv of one input
    (xt: x's twin, LF.shortcut_input) -- as one native forward launch on the GPU (both bias-free,
    no fused ReLU); otherwise the two module calls."""
    if _ext.use_native(x) and xt.data_ptr() == x.data_ptr():
        flat = getattr(mod0, "_ldnn_flat", None)
        ok = (flat is not None and flat.shadow is not None and getattr(mod1, "_ldnn_flat", None) is flat
              and all(m.groups == 1 and m.dilation == (1, 1) and m.bias is None and m.stride[0] == m.stride[1]
                      and isinstance(m.padding, tuple) and m.padding[0] == m.padding[1]
                      and getattr(m, "activation", None) != "relu" for m in (mod0, mod1))
              and mod0.in_channels == mod1.in_channels)
        if ok and _fire_pre_hooks((mod0, mod1), x):
            bn0 = mod0._ldnn_stats_bn if _layers_fuse_bn_stats() else None
            bn1 = mod1._ldnn_stats_bn if _layers_fuse_bn_stats() else None
            y0, y1 = _Conv2dPairNative.apply(x, xt, mod0.weight, mod1.weight, flat,
                                             (mod0.stride[0], mod0.padding[0], bn0),
                                             (mod1.stride[0], mod1.padding[0], bn1))
            return _zpad(y0), _zpad(y1)
    return mod0(x), mod1(xt)


def _layers_fuse_bn_stats() -> bool:
    from ..models import layers
    return layers.FUSE_BN_STATS


def conv2d(x, mod, relu: bool = False, bn=None):
    """Convolution of module `mod` (nn.Conv2d parameters).  GPU: native implicit-GEMM
    kernels on NHWC bf16 activations and KRSC bf16 weights (groups=1, dilation=1);
    CPU: the fp32 reference."""
    if _ext.use_native(x):
        flat = getattr(mod, "_ldnn_flat", None)
        ok = (flat is not None and flat.shadow is not None and mod.groups == 1 and mod.dilation == (1, 1)
              and mod.stride[0] == mod.stride[1] and mod.padding[0] == mod.padding[1]
              and isinstance(mod.padding, tuple))
        if not ok:
            raise RuntimeError("native conv needs groups=1, dilation=1, square stride/padding and "
                               "the model attached to FlatParams (ldnn.prepare(model))")
        # output pad channels: zero weight rows and bias entries -> exactly 0 (also after ReLU)
        return _zpad(_Conv2dNative.apply(x, mod.weight, mod.bias, mod.stride[0], mod.padding[0], flat, relu, bn))
    y = F.conv2d(x.float(), mod.weight, mod.bias, mod.stride, mod.padding, mod.dilation, mod.groups)
    return F.relu(y) if relu else y


def _module_ws(mod, attr: str, n: int, dev, zero: bool = False) -> torch.Tensor:
    """A norm module's persistent fp32 scratch, kept as ``mod.<attr>``.  It grows with the largest
    call seen, so a captured step -- warmed up at its own shape first -- allocates nothing new.
    ``zero``: zeroed once (the BN kernels keep their accumulators clear: no zero-fill launch per
    call); the GroupNorm / LayerNorm scratch keeps nothing between launches and needs no zeroing."""
    ws = mod.__dict__.get(attr)
    if ws is None or ws.device != dev or ws.numel() < n:
        ws = mod.__dict__[attr] = (torch.zeros if zero else torch.empty)(max(n, 1), dtype=torch.float32, device=dev)
    return ws


def _bn_workspace(mod, C: int, dev, C_) -> torch.Tensor:
    return _module_ws(mod, "_ldnn_bn_ws", C_.bn_workspace_floats(C), dev, zero=True)


def _with_twin(y: torch.Tensor, twin: torch.Tensor) -> torch.Tensor:
    """Native BN / pool outputs come with a twin: a second autograd output over the
    same storage.  A residual block reads its shortcut through the twin
    (``shortcut_input``), so the producer's backward receives the two branch
    gradients separately and sums them inside its own kernels -- no separate
    elementwise add of the gradients (autograd's accumulation of a tensor used twice)."""
    y._ldnn_twin = twin
    return y


def shortcut_input(x: torch.Tensor) -> torch.Tensor:
    """The tensor a residual block's shortcut branch should read (x's twin if it has one)."""
    t = getattr(x, "_ldnn_twin", None)
    src = getattr(x, "_ldnn_bnsrc", None)
    if src is not None:   # the producer BN's gradient arrives in two parts: no dgrad-side statistics
        src.twin_used = True
    return x if t is None else t


def _bn_stats_source(mod, x2, C: int):
    """Where a BN forward over ``x2`` takes its batch statistics from: (running_mean, running_var,
    save_mean, save_invstd, momentum, num_batches, stats_ready).  stats_ready: the producing conv's
    epilogue already accumulated + finalized them for this very buffer (_conv_bn_stats_done; a
    training-mode path); otherwise this BN's own pass, with its bookkeeping (_bn_train_state)."""
    pre = mod.__dict__.pop("_ldnn_pre", None)
    if pre is not None and mod.training and pre[0] == x2.data_ptr():
        return None, None, pre[1], pre[2], 0.0, None, True
    rm, rv, mom, nbt = _bn_train_state(mod, x2.device)
    smean = torch.empty(C, dtype=torch.float32, device=x2.device)
    return rm, rv, smean, torch.empty_like(smean), mom or 0.0, nbt, False


class _BatchNormNative(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias, residual, mod, flat, relu):
        C_ = _ext.C()
        N, C, H, W = x.shape
        xb = as_nhwc(_to_bf16(x), C, zero_pad=False)
        x2 = xb.view(-1, C)
        r2 = None
        if residual is not None:
            r2 = as_nhwc(_to_bf16(residual), C, zero_pad=False).reshape(-1, C)
        y = torch.empty(N, H, W, C, dtype=torch.bfloat16, device=x.device)
        dev = x.device
        ws = _bn_workspace(mod, C, dev, C_)
        gamma = flat.master_storage(weight)[:C] if weight is not None else None
        beta = flat.master_storage(bias)[:C] if bias is not None else None
        training = mod.training or not mod.track_running_stats
        # ReLU as a bit mask for the backward (its reduce and apply passes read 1/16 of
        # y's bytes); only when a backward will run
        mask = (torch.empty(x2.shape[0] * C // 8, dtype=torch.uint8, device=dev)
                if relu and any(ctx.needs_input_grad) and BN_RELU_MASK else None)
        rm, rv, smean, sinv, mom, nbt, ready = _bn_stats_source(mod, x2, C)
        C_.bn_fwd(x2, y.view(-1, C), r2, gamma, beta, rm, rv, smean, sinv, ws, mod.eps, mom, training, relu, nbt,
                  stats_ready=ready, mask=mask)
        ctx.mask = mask
        ctx.save_for_backward(x2, y if mask is None else x2.new_empty(0), smean, sinv)
        ctx.meta = (flat, weight, bias, relu, residual is not None, ws, (N, C, H, W), x.dtype)
        ctx.set_materialize_grads(False)
        out = nchw_view(y, C)
        ctx.bnsrc = None
        if (CONV_BN_BWD and mod.training and weight is not None and bias is not None
                and (mask is not None or not relu) and any(ctx.needs_input_grad)):
            ctx.bnsrc = out._ldnn_bnsrc = _BnBwdSrc(mod, flat, weight, bias, x2, mask, smean, sinv, ws, C)
        return out, nchw_view(y, C)

    @staticmethod
    def backward(ctx, gy, gy_twin):
        C_ = _ext.C()
        x2, y, smean, sinv = ctx.saved_tensors
        flat, weight, bias, relu, has_res, ws, (N, C, H, W), in_dtype = ctx.meta
        if gy is None:
            gy, gy_twin = gy_twin, None
        if gy is None:
            return None, None, None, None, None, None, None
        g2 = as_nhwc(_to_bf16(gy), C, zero_pad=False).contiguous().view(-1, C)
        gt = None
        if gy_twin is not None:   # the shortcut branch's gradient of the same output: summed in the kernels
            gt = as_nhwc(_to_bf16(gy_twin), C, zero_pad=False).contiguous().view(-1, C)
        dx = torch.empty(N, H, W, C, dtype=torch.bfloat16, device=x2.device)
        dres = torch.empty_like(dx) if has_res and ctx.needs_input_grad[3] else None
        gamma = flat.master_storage(weight)[:C] if weight is not None else None
        # first write of the step: the finalize stores dgamma / dbeta instead of adding
        dg, db, assign = flat.affine_grads(weight, bias)
        mask = ctx.mask
        yv = y.view(-1, C) if mask is None else x2   # (y is not read when the mask is given)
        pre = ctx.bnsrc.pre if ctx.bnsrc is not None else None
        ctx.bnsrc = None
        # statistics finalized by the consumer conv's dgrad epilogue, if its dx arrived unchanged
        # (a second consumer's gradient -- an in-place accumulation bumps the version -- or a
        # twin branch gradient sends the BN through its own reduce)
        ready = (pre is not None and gt is None and assign and pre[0] == g2.data_ptr() and pre[1] == gy._version)
        BN_BWD_FUSED[0] += int(ready)
        C_.bn_bwd(x2, yv, g2, dx.view(-1, C), dres.view(-1, C) if dres is not None else None, gamma,
                  smean, sinv, ws, dg, db, relu, mask=mask, grad_assign=assign, dy2=gt, stats_ready=ready)
        flat.notify(weight, bias)
        dresv = nchw_view(dres, C) if dres is not None else None
        return _from_bf16(nchw_view(dx, C), in_dtype), None, None, dresv, None, None, None


class _BatchNormDualNative(torch.autograd.Function):
    """relu(bn_a(x) + bn_b(r)) -- a residual block whose shortcut carries its own BatchNorm
    (1x1 downsample conv + BN) -- as one native pass each way (bn_pool.hip bn_dual_*): the
    shortcut BN's output is never stored, both BNs' backward statistics come from one
    reduce pass over the shared post-ReLU gradient, and one apply pass writes dx and dr."""

    @staticmethod
    def forward(ctx, x, r, wa, ba, wb, bb, mod_a, mod_b, flat):
        C_ = _ext.C()
        N, C, H, W = x.shape
        dev = x.device
        x2 = as_nhwc(_to_bf16(x), C, zero_pad=False).reshape(-1, C)
        r2 = as_nhwc(_to_bf16(r), C, zero_pad=False).reshape(-1, C)
        y = torch.empty(N, H, W, C, dtype=torch.bfloat16, device=dev)
        mask = (torch.empty(x2.shape[0] * C // 8, dtype=torch.uint8, device=dev)
                if any(ctx.needs_input_grad) and BN_RELU_MASK else None)

        def state(mod, t2, w, b):   # one BN's run of bn_dual_fwd's arguments
            rm, rv, mean, invstd, mom, nbt, ready = _bn_stats_source(mod, t2, C)
            return (flat.master_storage(w)[:C], flat.master_storage(b)[:C], rm, rv, mean, invstd,
                    _bn_workspace(mod, C, dev, C_), mod.eps, mom, nbt, ready)

        sa, sb = state(mod_a, x2, wa, ba), state(mod_b, r2, wb, bb)
        C_.bn_dual_fwd(x2, r2, y.view(-1, C), mask, *sa, *sb)
        ctx.mask = mask
        ctx.save_for_backward(x2, r2, y.view(-1, C) if mask is None else x2.new_empty(0), sa[4], sa[5], sb[4], sb[5])
        ctx.meta = (flat, (wa, ba, sa[6]), (wb, bb, sb[6]), (N, C, H, W), x.dtype, r.dtype)
        ctx.set_materialize_grads(False)
        return nchw_view(y, C), nchw_view(y, C)

    @staticmethod
    def backward(ctx, gy, gy_twin):
        C_ = _ext.C()
        x2, r2, y2, mean_a, inv_a, mean_b, inv_b = ctx.saved_tensors
        flat, (wa, ba, ws_a), (wb, bb, ws_b), (N, C, H, W), x_dtype, r_dtype = ctx.meta
        if gy is None:
            gy, gy_twin = gy_twin, None
        if gy is None:
            return (None,) * 9

        def nhwc2(t):
            return as_nhwc(_to_bf16(t), C, zero_pad=False).contiguous().view(-1, C)

        g2 = nhwc2(gy)
        gt = nhwc2(gy_twin) if gy_twin is not None else None
        dx = torch.empty(N, H, W, C, dtype=torch.bfloat16, device=x2.device)
        dr = torch.empty_like(dx)

        C_.bn_dual_bwd(x2, r2, y2 if ctx.mask is None else x2, ctx.mask, g2, gt, dx.view(-1, C), dr.view(-1, C),
                       flat.master_storage(wa)[:C], mean_a, inv_a, ws_a, *flat.affine_grads(wa, ba),
                       flat.master_storage(wb)[:C], mean_b, inv_b, ws_b, *flat.affine_grads(wb, bb))
        flat.notify(wa, ba)
        flat.notify(wb, bb)
        return (_from_bf16(nchw_view(dx, C), x_dtype), _from_bf16(nchw_view(dr, C), r_dtype),
                None, None, None, None, None, None, None)


# y = relu(bn_a(x) + bn_b(r)) in one pass (LDNN_BN_DUAL=0: bn_b's apply + bn_a's residual pass)
BN_DUAL_FUSED = os.environ.get("LDNN_BN_DUAL", "1") != "0"


def batch_norm_dual_act(x, mod_a, r, mod_b):
    """relu(mod_a(x) + mod_b(r)): the tail of a residual block whose shortcut is conv + BN."""
    fa, fb = getattr(mod_a, "_ldnn_flat", None), getattr(mod_b, "_ldnn_flat", None)
    ok = (BN_DUAL_FUSED and _ext.use_native(x) and fa is not None and fa is fb and mod_a.training
          and mod_b.training and mod_a.affine and mod_b.affine and x.dim() == 4 and x.shape == r.shape
          and x.shape[1] % 8 == 0)
    if ok:
        return _with_twin(*_BatchNormDualNative.apply(x, r, mod_a.weight, mod_a.bias, mod_b.weight, mod_b.bias,
                                                      mod_a, mod_b, fa))
    return mod_a.act(x, residual=mod_b(r), relu=True)


# BatchNorm + ReLU keeps a bit mask of the output for its backward (measured A/B in
# profiles/, LDNN_BN_RELU_MASK=0 reads the bf16 output instead)
BN_RELU_MASK = os.environ.get("LDNN_BN_RELU_MASK", "1") != "0"


def batch_norm_act(x, mod, residual=None, relu: bool = False):
    """relu?(BatchNorm2d(x) (+ residual)) -- fused into one native pass on the GPU
    (fp32 statistics over NHWC bf16); the CPU path is the fp32 reference."""
    flat = getattr(mod, "_ldnn_flat", None)
    if _ext.use_native(x) and flat is not None and x.shape[1] % 8 == 0 and mod.affine:
        return _with_twin(*_BatchNormNative.apply(x, mod.weight, mod.bias, residual, mod, flat, relu))
    y = batch_norm2d(x, mod)
    if residual is not None:
        y = y + residual
    return F.relu(y) if relu else y


def batch_norm2d(x, mod):
    training = mod.training or not mod.track_running_stats
    mom = 0.0 if mod.momentum is None else mod.momentum
    if mod.training and mod.track_running_stats and mod.num_batches_tracked is not None:
        mod.num_batches_tracked.add_(1)
        if mod.momentum is None:
            mom = 1.0 / float(mod.num_batches_tracked)
    rm = mod.running_mean if (not mod.training or mod.track_running_stats) else None
    rv = mod.running_var if (not mod.training or mod.track_running_stats) else None
    if x.is_cuda and x.dtype == torch.bfloat16:
        y = F.batch_norm(x.float(), rm, rv, mod.weight, mod.bias, training, mom, mod.eps)
        return y.to(torch.bfloat16)
    return F.batch_norm(x.float(), rm, rv, mod.weight, mod.bias, training, mom, mod.eps)


# ------------------------------------------------------------------ GroupNorm
def _dense_nhwc(t: torch.Tensor) -> bool:
    """A logical [N, C, H, W] bf16 tensor that is a view of a dense, 16-byte aligned NHWC buffer
    (what every native conv / norm / pool op returns)."""
    if t.dtype != torch.bfloat16 or t.dim() != 4:
        return False
    N, C, H, W = t.shape
    want = (H * W * C, 1, W * C, C)
    return (all(sz == 1 or st == w for sz, st, w in zip(t.shape, t.stride(), want))
            and t.numel() > 0 and t.data_ptr() % 16 == 0)


class _GroupNormNative(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias, residual, mod, flat, relu):
        C_ = _ext.C()
        N, C, H, W = x.shape
        G, dev = mod.num_groups, x.device
        xb = x.as_strided((N, H, W, C), (H * W * C, W * C, C, 1), x.storage_offset())
        rb = None
        if residual is not None:
            rb = as_nhwc(_to_bf16(residual), C, zero_pad=False)
        y = torch.empty(N, H, W, C, dtype=torch.bfloat16, device=dev)
        ws = _module_ws(mod, "_ldnn_gn_ws", C_.gn_workspace_floats(N, H * W, C, G), dev)   # (partials + coefficients)
        mean = torch.empty(N * G, dtype=torch.float32, device=dev)
        rstd = torch.empty(N * G, dtype=torch.float32, device=dev)
        gamma = flat.master_storage(weight)[:C] if weight is not None else None
        beta = flat.master_storage(bias)[:C] if bias is not None else None
        # the ReLU leaves a bit mask for the backward (which then never reads y); only when one will run
        mask = (torch.empty(N * H * W * C // 8, dtype=torch.uint8, device=dev)
                if relu and any(ctx.needs_input_grad) else None)
        C_.gn_fwd(xb, y, rb, gamma, beta, mean, rstd, ws, G, mod.eps, relu, mask=mask)
        ctx.save_for_backward(xb, mean, rstd)
        ctx.mask = mask
        ctx.meta = (flat, weight, bias, mod, G, residual is not None, residual.dtype if residual is not None else None)
        ctx.set_materialize_grads(False)
        return _zpad(nchw_view(y, C))

    @staticmethod
    def backward(ctx, gy):
        if gy is None:
            return (None,) * 7
        C_ = _ext.C()
        xb, mean, rstd = ctx.saved_tensors
        flat, weight, bias, mod, G, has_res, res_dtype = ctx.meta
        N, H, W, C = xb.shape
        g = as_nhwc(_to_bf16(gy), C, zero_pad=False).contiguous()
        if g.data_ptr() % 16:
            g = g.clone()
        dx = torch.empty_like(xb)
        dres = torch.empty_like(xb) if has_res and ctx.needs_input_grad[3] else None
        gamma, dg, db, assign = None, None, None, True
        if weight is not None:   # first write of the step: the finalize stores dgamma / dbeta instead of adding
            gamma = flat.master_storage(weight)[:C]
            dg, db, assign = flat.affine_grads(weight, bias)
        ws = _module_ws(mod, "_ldnn_gn_ws", C_.gn_workspace_floats(N, H * W, C, G), xb.device)
        C_.gn_bwd(xb, g, dx, dres, gamma, mean, rstd, ws, dg, db, G, ctx.mask is not None, mask=ctx.mask,
                  grad_assign=assign)
        if weight is not None:
            flat.notify(weight, bias)
        dresv = _from_bf16(nchw_view(dres, C), res_dtype) if dres is not None else None
        return _zpad(nchw_view(dx, C)), None, None, dresv, None, None, None


def group_norm_act(x, mod, residual=None, relu: bool = False):
    """relu?(GroupNorm(x) (+ residual)) with ``mod``'s (nn.GroupNorm) groups, eps and affine
    parameters.  GPU, bf16 activations in the dense NHWC layout the native ops produce,
    C % 8 == 0: the native passes of group_norm.hip (fp32 statistics per sample and group, the add
    and the ReLU fused into the apply pass; gamma / beta read from the FlatParams master, their
    gradients written into the flat gradient buffer).  Everything else -- the CPU, other dtypes or
    layouts, other channel counts, a module not attached to FlatParams -- is F.group_norm in fp32
    plus the add and the ReLU.  Statistics are per sample: train and eval mode are one function."""
    flat = getattr(mod, "_ldnn_flat", None)
    if (_ext.use_native(x) and _dense_nhwc(x) and x.shape[1] % 8 == 0 and x.shape[0] <= 65535
            and (not mod.affine or flat is not None)):
        return _GroupNormNative.apply(x, mod.weight, mod.bias, residual, mod, flat, relu)
    y = F.group_norm(x.float(), mod.num_groups, mod.weight, mod.bias, mod.eps)
    if residual is not None:
        y = y + residual
    if relu:
        y = F.relu(y)
    return y.to(torch.bfloat16) if x.is_cuda and x.dtype == torch.bfloat16 else y


# ------------------------------------------------------------------ LayerNorm
def _ln_ld(t: torch.Tensor) -> int:
    return t.stride(0) if t.shape[0] > 1 else _up8(t.shape[1])   # (a single row's stride is arbitrary)


def _ln_rows(t: torch.Tensor) -> torch.Tensor:
    """``t`` ([B, N] bf16) as an operand of the LayerNorm kernels: itself when it is a view with a unit
    column stride, a row stride that is a multiple of 8 (and no more than twice the row: a column
    slice of a much wider matrix is not worth an output of that stride), a 16-byte aligned base and a
    storage that holds every row's last vector whole -- what an ldnn ``Linear`` hands on, or a dense
    matrix with N % 8 == 0.  Anything else is copied once into the [B, N] view of a [B, up8(N)]
    buffer (whose pad columns may hold anything: the kernels select them away)."""
    B, N = t.shape
    npad, ld = _up8(N), _ln_ld(t)
    if ((t.stride(1) == 1 or N == 1) and ld % 8 == 0 and npad <= ld <= 2 * npad and t.data_ptr() % 16 == 0
            and t.storage_offset() + (B - 1) * ld + npad <= t.untyped_storage().nbytes() // t.element_size()):
        return t
    buf = torch.empty(B, npad, dtype=torch.bfloat16, device=t.device)
    v = buf if npad == N else buf[:, :N]
    v.copy_(t)
    return v


def _ln_out_like(x2: torch.Tensor) -> torch.Tensor:
    """The output operand for ``x2``: the [B, N] view of a fresh buffer with x2's row stride."""
    B, N = x2.shape
    ld = _ln_ld(x2)
    buf = torch.empty(B, ld, dtype=torch.bfloat16, device=x2.device)
    return buf if ld == N else buf[:, :N]


class _LayerNormNative(torch.autograd.Function):
    """layer_norm.hip: the forward saves x, mean and rstd; the backward recomputes the pre-activation."""

    @staticmethod
    def forward(ctx, x, weight, bias, mod, flat, act):
        C_ = _ext.C()
        x2 = _ln_rows(x)
        B, N = x2.shape
        y = _ln_out_like(x2)
        mean = torch.empty(B, dtype=torch.float32, device=x.device)
        rstd = torch.empty(B, dtype=torch.float32, device=x.device)
        # the padded fp32 master storage (up8(N) floats; the kernels use the first N)
        gamma = flat.master_storage(weight) if weight is not None else None
        beta = flat.master_storage(bias) if bias is not None else None
        C_.ln_fwd(x2, y, gamma, beta, mean, rstd, mod.eps, -1 if act is None else act)
        ctx.save_for_backward(x2, mean, rstd)
        ctx.meta = (flat, weight, bias, mod, act)
        if y.stride(0) != N:
            y._ldnn_zpad = True   # the kernel wrote the pad columns' zeros, also under sigmoid
        return y

    @staticmethod
    def backward(ctx, gy):
        C_ = _ext.C()
        x2, mean, rstd = ctx.saved_tensors
        flat, weight, bias, mod, act = ctx.meta
        B, N = x2.shape
        g = _ln_rows(_to_bf16(gy))
        dx = _ln_out_like(x2)
        gamma = beta = dg = db = ws = None
        assign = False
        if weight is not None:
            gamma, beta = flat.master_storage(weight), flat.master_storage(bias)
            # first write of the step: the finalize stores dgamma / dbeta instead of adding
            dg, db, assign = flat.affine_grads(weight, bias)
            ws = _module_ws(mod, "_ldnn_ln_ws", C_.ln_workspace_floats(B, N), x2.device)   # (the partial rows)
        C_.ln_bwd(x2, g, dx, gamma, beta, mean, rstd, ws, dg, db, -1 if act is None else act, grad_assign=assign)
        if weight is not None:
            flat.notify(weight, bias)
        return dx, None, None, None, None, None


_LN_MAX_WIDTH = None


def _ln_max_width() -> int:
    global _LN_MAX_WIDTH
    if _LN_MAX_WIDTH is None:
        _LN_MAX_WIDTH = int(_ext.C().ln_max_width())
    return _LN_MAX_WIDTH


def layer_norm_act(x, mod, act: str = "none"):
    """act(LayerNorm(x)) over the last dimension with ``mod``'s (nn.LayerNorm over one dimension) eps
    and affine parameters; ``act`` in none | relu | sigmoid.  GPU, bf16, a 2-D activation with a unit
    column stride and at most ``ln_max_width()`` columns: the native passes of layer_norm.hip (fp32
    statistics per row, the activation fused; gamma / beta read from the FlatParams master, their
    gradients written into the flat gradient buffer; only mean and rstd are saved).  A [B, N] view of
    a padded buffer -- what an ldnn ``Linear`` hands on -- is processed in place of a copy and the
    result is such a view with the input's row stride and zeroed pad columns, so the next ``Linear``
    widens it without a copy or a fill.  Everything else -- the CPU, other dtypes or ranks, wider
    rows, an affine module not attached to FlatParams -- is F.layer_norm in fp32 plus the activation.
    Statistics are per row: train and eval mode are one function."""
    a = ACTS[act]
    N = x.shape[-1]
    if len(mod.normalized_shape) != 1 or mod.normalized_shape[0] != N:
        raise ValueError(f"layer_norm_act: the module normalises {tuple(mod.normalized_shape)}, the input's last "
                         f"dimension is {N}")
    flat = getattr(mod, "_ldnn_flat", None)
    if (_ext.use_native(x) and x.dtype == torch.bfloat16 and x.dim() == 2 and x.numel() > 0
            and (x.stride(1) == 1 or N == 1) and N <= _ln_max_width()
            and (mod.weight is None or (flat is not None and mod.bias is not None))):
        return _LayerNormNative.apply(x, mod.weight, mod.bias, mod, flat, a)
    y = F.layer_norm(x.float(), (N,), mod.weight, mod.bias, mod.eps)
    if a == 0:
        y = F.relu(y)
    elif a == 1:
        y = torch.sigmoid(y)
    return y.to(torch.bfloat16) if x.is_cuda and x.dtype == torch.bfloat16 else y


# ------------------------------------------------------------------ pooling
class _PoolNative(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, k, stride, pad, is_max):
        C_ = _ext.C()
        N, C, H, W = x.shape
        cp = _up8(C)
        xb = as_nhwc(_to_bf16(x), cp)
        P, Q = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
        y = torch.empty(N, P, Q, cp, dtype=torch.bfloat16, device=x.device)
        am = torch.empty(N, P, Q, cp, dtype=torch.uint8, device=x.device) if is_max else None
        C_.pool_fwd(xb.contiguous(), y, am, k, k, stride, pad, is_max)
        ctx.save_for_backward(am) if is_max else None
        ctx.meta = (k, stride, pad, is_max, (N, C, H, W, cp), x.dtype)
        ctx.set_materialize_grads(False)
        return nchw_view(y, C), nchw_view(y, C)

    @staticmethod
    def backward(ctx, gy, gy_twin):
        C_ = _ext.C()
        k, stride, pad, is_max, (N, C, H, W, cp), in_dtype = ctx.meta
        if gy is None:
            gy, gy_twin = gy_twin, None
        if gy is None:
            return None, None, None, None, None
        am = ctx.saved_tensors[0] if is_max else None
        g = as_nhwc(_to_bf16(gy), cp).contiguous()
        gt = None
        if gy_twin is not None:
            gt = as_nhwc(_to_bf16(gy_twin), cp).contiguous()
        dx = torch.empty(N, H, W, cp, dtype=torch.bfloat16, device=gy.device)
        C_.pool_bwd(g, am, dx, k, k, stride, pad, is_max, dy2=gt)
        out = _zpad(nchw_view(dx, C))   # (pooled gradient of zero pad channels)
        return _from_bf16(out, in_dtype), None, None, None, None


class _BnReluMaxPoolNative(torch.autograd.Function):
    """maxpool3x3/2(relu(BatchNorm2d(x))) in one native pass each way (bn_pool.hip
    bn_maxpool_*): the BN output is never stored, the pool's argmax doubles as the
    ReLU mask and the backward turns the pooled gradient straight into dx."""

    @staticmethod
    def forward(ctx, x, weight, bias, mod, flat, pad):
        C_ = _ext.C()
        N, C, H, W = x.shape
        xb = as_nhwc(_to_bf16(x), C, zero_pad=False).contiguous()
        P, Q = (H + 2 * pad - 3) // 2 + 1, (W + 2 * pad - 3) // 2 + 1
        dev = x.device
        y = torch.empty(N, P, Q, C, dtype=torch.bfloat16, device=dev)
        am = torch.empty(N, P, Q, C, dtype=torch.uint8, device=dev)
        # the BN input at every argmax: the backward statistics read it (pooled size) instead of x
        xam = torch.empty(N, P, Q, C, dtype=torch.bfloat16, device=dev) if BN_POOL_MODE == 1 else None
        ws = _bn_workspace(mod, C, dev, C_)
        gamma = flat.master_storage(weight)[:C] if weight is not None else None
        beta = flat.master_storage(bias)[:C] if bias is not None else None
        rm, rv, smean, sinv, mom, nbt, ready = _bn_stats_source(mod, xb, C)
        C_.bn_pool_fwd(xb, y, am, gamma, beta, rm, rv, smean, sinv, ws, mod.eps, mom, nbt, ready, pad, xam)
        ctx.save_for_backward(xb, am, smean, sinv, xam)
        ctx.meta = (flat, weight, bias, ws, pad, C, x.dtype)
        ctx.set_materialize_grads(False)
        return nchw_view(y, C), nchw_view(y, C)

    @staticmethod
    def backward(ctx, gy, gy_twin):
        C_ = _ext.C()
        xb, am, smean, sinv, xam = ctx.saved_tensors
        flat, weight, bias, ws, pad, C, in_dtype = ctx.meta
        if gy is None:
            gy, gy_twin = gy_twin, None
        if gy is None:
            return None, None, None, None, None, None
        g = as_nhwc(_to_bf16(gy), C, zero_pad=False).contiguous()
        gt = None
        if gy_twin is not None:
            gt = as_nhwc(_to_bf16(gy_twin), C, zero_pad=False).contiguous()
        dx = torch.empty_like(xb)
        gamma = flat.master_storage(weight)[:C] if weight is not None else None
        dg, db, assign = flat.affine_grads(weight, bias)
        C_.bn_pool_bwd(xb, g, am, dx, gamma, smean, sinv, ws, dg, db, assign, gt, pad, xam)
        flat.notify(weight, bias)
        return _from_bf16(nchw_view(dx, C), in_dtype), None, None, None, None, None


# BN + ReLU + max-pool fused (LDNN_BN_POOL=0: the separate BN-apply and pool passes; 1: fused, the
# backward statistics from the pooled side (x at the argmax); 2: fused, the statistics pass reads x)
BN_POOL_MODE = int(os.environ.get("LDNN_BN_POOL", "1"))
BN_POOL_FUSED = BN_POOL_MODE != 0


def bn_relu_maxpool(x, bn, pool):
    """pool(relu(bn(x))) for a 3x3 / stride-2 max-pool: one native pass each way on the
    GPU in training mode (C / 8 dividing 256), else the separate layers."""
    flat = getattr(bn, "_ldnn_flat", None)
    k, st, pad = _sq(pool.kernel_size), _sq(pool.stride if pool.stride is not None else pool.kernel_size), \
        _sq(pool.padding)
    C = x.shape[1] if x.dim() == 4 else 0
    ok = (BN_POOL_FUSED and _ext.use_native(x) and flat is not None and bn.training and bn.affine
          and x.dim() == 4 and C % 8 == 0 and 256 % (C // 8 or 1) == 0 and C // 8 <= 256
          and k == 3 and st == 2 and pad is not None and 0 <= pad <= 1 and _sq(pool.dilation) == 1
          and not getattr(pool, "ceil_mode", False) and not getattr(pool, "return_indices", False))
    if ok:
        return _with_twin(*_BnReluMaxPoolNative.apply(x, bn.weight, bn.bias, bn, flat, pad))
    return pool(bn.act(x, relu=True))


def _sq(v):
    return v if isinstance(v, int) else (v[0] if v[0] == v[1] else None)


class _PoolFlatNative(torch.autograd.Function):
    """A pool whose only consumer flattens it (LeNet-5's last pool -> fc1): the kernel
    writes the dense NCHW output itself, so ``flatten(1)`` is a free view instead of an
    NHWC -> NCHW copy, and the backward reads the flattened gradient in place
    (bn_pool.hip pool_fwd_kernel / pool_bwd_kernel with ``cl`` > 0)."""

    @staticmethod
    def forward(ctx, x, k, stride, pad, is_max):
        C_ = _ext.C()
        N, C, H, W = x.shape
        cp = _up8(C)
        xb = as_nhwc(_to_bf16(x), cp)
        P, Q = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
        y = torch.empty(N, C, P, Q, dtype=torch.bfloat16, device=x.device)
        am = torch.empty(N, P, Q, cp, dtype=torch.uint8, device=x.device) if is_max else None
        C_.pool_fwd(xb.contiguous(), y, am, k, k, stride, pad, is_max, nchw_out=True)
        ctx.save_for_backward(am) if is_max else None
        ctx.meta = (k, stride, pad, is_max, (N, C, H, W, cp), x.dtype)
        return y

    @staticmethod
    def backward(ctx, gy):
        C_ = _ext.C()
        k, stride, pad, is_max, (N, C, H, W, cp), in_dtype = ctx.meta
        am = ctx.saved_tensors[0] if is_max else None
        g = _to_bf16(gy).contiguous()
        dx = torch.empty(N, H, W, cp, dtype=torch.bfloat16, device=gy.device)
        C_.pool_bwd(g, am, dx, k, k, stride, pad, is_max, nchw_dy=True)
        out = _zpad(nchw_view(dx, C))
        return _from_bf16(out, in_dtype), None, None, None, None


def pool2d(x, mod, is_max: bool):
    """Max / average pooling.  ``mod.flatten_out`` (set by a model whose pool feeds a
    flatten, e.g. LeNet-5) makes the native path return a dense NCHW tensor."""
    k, st, pad = _sq(mod.kernel_size), _sq(mod.stride if mod.stride is not None else mod.kernel_size), _sq(mod.padding)
    simple = (None not in (k, st, pad) and not getattr(mod, "ceil_mode", False)
              and (not is_max or _sq(mod.dilation) == 1) and (is_max or getattr(mod, "count_include_pad", True))
              and k * k <= 255)
    if _ext.use_native(x) and simple and x.dim() == 4 and getattr(mod, "flatten_out", False):
        return _PoolFlatNative.apply(x, k, st, pad, is_max)
    if _ext.use_native(x) and simple and x.dim() == 4:
        y, twin = _PoolNative.apply(x, k, st, pad, is_max)   # (the input's pad was zeroed / zero)
        return _with_twin(_zpad(y), _zpad(twin))
    if is_max:
        return F.max_pool2d(x, mod.kernel_size, mod.stride, mod.padding, mod.dilation, mod.ceil_mode)
    return F.avg_pool2d(x, mod.kernel_size, mod.stride, mod.padding, mod.ceil_mode, mod.count_include_pad)


class _GapNative(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        C_ = _ext.C()
        N, C, H, W = x.shape
        cp = _up8(C)
        xb = as_nhwc(_to_bf16(x), cp).contiguous()
        y = torch.empty(N, cp, dtype=torch.bfloat16, device=x.device)
        C_.gap_fwd(xb.view(N, H * W, cp), y)
        ctx.meta = (N, C, H, W, cp, x.dtype)
        return y[:, :C].view(N, C, 1, 1)

    @staticmethod
    def backward(ctx, gy):
        C_ = _ext.C()
        N, C, H, W, cp, in_dtype = ctx.meta
        g2 = gy.reshape(N, C)
        if cp == C and g2.dtype == torch.bfloat16 and g2.is_contiguous():
            g = g2   # (the Linear dgrad's dense output: no zero-pad copy)
        else:
            g = torch.zeros(N, cp, dtype=torch.bfloat16, device=gy.device)
            g[:, :C] = g2
        dx = torch.empty(N, H, W, cp, dtype=torch.bfloat16, device=gy.device)
        C_.gap_bwd(g, dx.view(N, H * W, cp))
        out = nchw_view(dx, C)
        return _from_bf16(out, in_dtype)


def adaptive_avg_pool2d(x, output_size):
    os_ = output_size if isinstance(output_size, int) else (output_size[0] if output_size[0] == output_size[1] else None)
    if _ext.use_native(x) and os_ == 1 and x.dim() == 4:
        return _GapNative.apply(x)
    return F.adaptive_avg_pool2d(x, output_size)


class _GapLinearNative(torch.autograd.Function):
    """AdaptiveAvgPool2d(1) -> flatten -> Linear (<= 16 classes) in one launch each way
    (gap_head.hip): the CNN classifier heads at small batch are pure launch latency."""

    @staticmethod
    def forward(ctx, x, weight, bias, flat):
        C_ = _ext.C()
        N, C, H, W = x.shape
        w = flat.shadow_storage(weight)
        npad = w.shape[0]
        xb = as_nhwc(_to_bf16(x), C).contiguous()
        pooled = torch.empty(N, C, dtype=torch.bfloat16, device=x.device)
        logits = torch.empty(N, npad, dtype=torch.bfloat16, device=x.device)
        b = flat.master_storage(bias) if bias is not None else None
        ncls = weight.shape[0]
        C_.gap_linear_fwd(xb.view(N, H * W, C), w, b, pooled, logits, ncls)
        ctx.save_for_backward(pooled)
        ctx.meta = (N, C, H, W, ncls, x.dtype)
        ctx.flat, ctx.weight, ctx.bias = flat, weight, bias
        return logits[:, :ncls]

    @staticmethod
    def backward(ctx, gy):
        C_ = _ext.C()
        (pooled,) = ctx.saved_tensors
        N, C, H, W, ncls, in_dtype = ctx.meta
        flat, weight, bias = ctx.flat, ctx.weight, ctx.bias
        g = _bf16_rows(gy)
        dx = torch.empty(N, H, W, C, dtype=torch.bfloat16, device=gy.device)
        C_.gap_linear_bwd(g, pooled, flat.shadow_storage(weight), flat.grad_storage(weight),
                          flat.grad_storage(bias) if bias is not None else None, dx.view(N, H * W, C), ncls,
                          beta_w=flat.grad_beta(weight), beta_b=flat.grad_beta(bias) if bias is not None else 0.0)
        flat.notify(weight, bias)
        out = nchw_view(dx, C)
        return _from_bf16(out, in_dtype), None, None, None


# LDNN_GAP_LINEAR=0: the pooled classifier head runs as separate pool + Linear ops (A/B knob)
GAP_LINEAR = os.environ.get("LDNN_GAP_LINEAR", "1") == "1"


def gap_linear(x, pool, fc):
    """fc(flatten(pool(x))) for a global average pool `pool` and an ldnn Linear `fc`; one fused
    launch each way when the shapes allow (<= 16 classes, unpadded features), else the two ops."""
    flat = getattr(fc, "_ldnn_flat", None)
    os_ = pool.output_size if isinstance(pool.output_size, int) else (
        pool.output_size[0] if pool.output_size[0] == pool.output_size[1] else None)
    if (GAP_LINEAR and _ext.use_native(x) and x.dim() == 4 and os_ == 1 and flat is not None
            and flat.shadow is not None and getattr(fc, "activation", "none") == "none"):
        N, C, H, W = x.shape
        w = flat.shadow_storage(fc.weight)
        if (w.shape[1] == C and C == fc.in_features and _ext.C().gap_linear_ok(N, H * W, C, fc.out_features)
                and _fire_pre_hooks((pool, fc), x)):
            return _GapLinearNative.apply(x, fc.weight, fc.bias, flat)
    y = pool(x)
    return fc(y.reshape(y.size(0), -1))


# -------------------------------------------------------------------- dropout
_M32, _M64 = (1 << 32) - 1, (1 << 64) - 1
_DROP_GROUP_MUL = 0xD1B54A32D192ED03
# words of a DropoutState (int32, the device kernel's layout: csrc/kernels/dropout.hip)
DROP_SEED_LO, DROP_SEED_HI, DROP_MODULE, DROP_COUNTER, DROP_THR, DROP_SCALE, DROP_ARRIVE = range(7)


def _i32(v: int) -> int:
    """A 32-bit pattern as the signed value an int32 tensor stores."""
    v &= _M32
    return v - (1 << 32) if v >> 31 else v


def dropout_thr(p: float) -> int:
    """thr = round(p * 65536) of a drop rate 0 <= p <= 1: the realised rate is thr / 65536."""
    p = float(p)
    if not 0.0 <= p <= 1.0:
        raise ValueError(f"dropout probability has to be between 0 and 1, but got {p}")
    return int(round(p * 65536.0))


def dropout_scale(thr: int):
    """The fp32 scale 65536 / (65536 - thr) of the kept elements (0 when everything is dropped)."""
    import numpy as np

    return np.float32(0.0) if thr >= 65536 else np.float32(65536.0) / np.float32(65536 - thr)


def dropout_mask(seed: int, module_index: int, counter: int, thr: int, R: int, N: int):
    """The exact NumPy twin of the dropout kernels' mask (csrc/kernels/dropout.hip): a bool [R, N]
    array, True where the element is DROPPED.

    A tensor is seen as [R, N]: N the last logical dimension, R the product of the rest.  Four
    neighbouring columns of a row share one hash; with G = ceil(N / 4):

        key   = smix(smix(seed64) ^ (module_index << 32 | counter))      all 64-bit, wrapping
        h     = smix(key ^ ((r * G + (c >> 2)) * 0xD1B54A32D192ED03))
        bits  = (h >> (16 * (c & 3))) & 0xFFFF
        drop  = bits < thr        with thr = round(p * 65536), 0 <= thr <= 65536
        scale = 65536.0f / (65536 - thr)   (fp32; thr == 65536: everything is dropped, output 0)
        y     = drop ? 0 : bf16_rne(float(x) * scale)        dx = drop ? 0 : bf16_rne(float(g) * scale)

    smix is data/autoaugment.smix (splitmix64's finaliser).  The mask depends on the logical (r, c)
    only, not on strides, padding or the launch."""
    import numpy as np

    from ..data.autoaugment import smix, smix_np

    key = smix(smix(int(seed) & _M64) ^ (((int(module_index) & _M32) << 32) | (int(counter) & _M32)))
    G = (N + 3) // 4
    u = np.uint64
    with np.errstate(over="ignore"):
        grp = np.arange(R * G, dtype=np.uint64) * u(_DROP_GROUP_MUL)
    h = smix_np(grp ^ u(key)).reshape(R, G)
    bits = (h[:, :, None] >> (np.arange(4, dtype=np.uint64) * u(16))) & u(0xFFFF)
    return (bits.reshape(R, 4 * G)[:, :N] < u(thr))


class DropoutState:
    """The persistent state one Dropout module's calls read: 8 int32 words on the module's device
    (seed low / high, module_index, counter, thr, the scale's fp32 bits, the kernel's arrival
    count).  The host writes it the way the optimizers write the lr: fills into persistent
    addresses, outside any captured graph.  The counter is advanced by the forward itself (on the
    GPU by the launch's last workgroup), so every call, and every replay of a captured call, draws
    a new mask."""

    def __init__(self, device, seed: int = 0, module_index: int = 0):
        self.words = torch.zeros(8, dtype=torch.int32, device=device)
        self.thr = 0   # (with scale 1: a launch before any set_rate copies its input)
        self.words[DROP_SCALE].fill_(_i32(int(dropout_scale(0).view("uint32"))))
        self.reseed(seed, module_index)

    def reseed(self, seed: int, module_index: int) -> None:
        s = int(seed) & _M64
        w = self.words
        w[DROP_SEED_LO].fill_(_i32(s))
        w[DROP_SEED_HI].fill_(_i32(s >> 32))
        w[DROP_MODULE].fill_(_i32(int(module_index)))
        w[DROP_COUNTER].fill_(0)

    def set_rate(self, p: float) -> int:
        """thr of ``p``; rewrites the state's thr and scale only when it differs from the last one."""
        thr = dropout_thr(p)
        if thr != self.thr:
            self.words[DROP_THR].fill_(thr)
            self.words[DROP_SCALE].fill_(_i32(int(dropout_scale(thr).view("uint32"))))
            self.thr = thr
        return thr

    def read(self) -> dict:
        """The state's words as Python ints (a device read: tests and debugging)."""
        w = [v & _M32 for v in self.words.tolist()]
        return dict(seed=w[DROP_SEED_LO] | (w[DROP_SEED_HI] << 32), module_index=w[DROP_MODULE],
                    counter=w[DROP_COUNTER], thr=w[DROP_THR])


def _drop_rows(t: torch.Tensor) -> torch.Tensor:
    """``t`` as a [R, N] operand of the dropout kernels: itself when it is a 2-D tensor with dense rows
    whose storage holds every row whole (a dense matrix, or the [B, N] view of a padded [B, npad]
    buffer an ldnn op handed on), else a dense [numel / N, N] copy."""
    N = t.shape[-1]
    if (t.dim() == 2 and t.stride(1) == 1 and t.stride(0) >= N
            and t.storage_offset() + t.shape[0] * t.stride(0) <= t.untyped_storage().nbytes() // t.element_size()):
        return t
    return t.contiguous().view(-1, N)


def _drop_out_like(x2: torch.Tensor) -> torch.Tensor:
    """The output operand for ``x2``: the [R, N] view of a fresh buffer with x2's row stride."""
    R, N = x2.shape
    buf = torch.empty(R, max(x2.stride(0), N), dtype=torch.bfloat16, device=x2.device)
    return buf if buf.shape[1] == N else buf[:, :N]


class _DropoutNative(torch.autograd.Function):
    """dropout.hip: the forward saves only its 8-word ticket, the backward regenerates the mask."""

    @staticmethod
    def forward(ctx, x, state):
        C = _ext.C()
        x2 = _drop_rows(_to_bf16(x))
        y = _drop_out_like(x2)
        ticket = torch.empty(8, dtype=torch.int32, device=x.device)
        C.dropout_fwd(x2, y, state.words, ticket)
        ctx.save_for_backward(ticket)
        ctx.shape, ctx.in_dtype = x.shape, x.dtype
        if y.stride(0) != y.shape[1] and x.dim() == 2:
            y._ldnn_zpad = True   # the kernel wrote the pad columns' zeros
            return y
        return y.view(x.shape)

    @staticmethod
    def backward(ctx, gy):
        (ticket,) = ctx.saved_tensors
        g2 = _drop_rows(_to_bf16(gy))
        dx = _drop_out_like(g2)
        _ext.C().dropout_bwd(g2, dx, ticket)
        dx = dx if dx.shape == ctx.shape else dx.view(ctx.shape)
        return _from_bf16(dx, ctx.in_dtype), None


def dropout(x, p: float = 0.5, training: bool = True, state: DropoutState | None = None):
    """Inverted dropout whose mask is a pure function of (seed, module_index, call count, element):
    see ``dropout_mask``.  ``state`` carries seed, module_index and the call count, and is advanced
    by the call.  On the GPU one native pass each way (no mask is stored: the backward regenerates
    it); on the CPU the exact twin, so a CPU and a GPU run with equal states drop the same elements.
    ``p == 0`` or ``training == False`` returns ``x`` itself.

    Dtypes: the native path computes in and returns bf16 whatever the input's dtype, like every
    native activation op (``relu``, ``linear_act``), and hands the input's dtype back only in the
    gradient; the CPU path keeps the input's dtype.  On bf16 inputs the two agree bit for bit."""
    thr = dropout_thr(p)
    if not training or thr == 0 or x.numel() == 0:
        return x
    if state is None:
        raise ValueError("dropout: a DropoutState is needed in training mode (models.layers.Dropout keeps one)")
    if state.words.device != x.device:
        raise ValueError(f"dropout: the state lives on {state.words.device}, the input on {x.device}")
    state.set_rate(p)
    if _ext.use_native(x):
        return _DropoutNative.apply(x, state)
    s = state.read()
    N = x.shape[-1]
    drop = torch.from_numpy(dropout_mask(s["seed"], s["module_index"], s["counter"], thr, x.numel() // N, N))
    state.words[DROP_COUNTER] = _i32(s["counter"] + 1)
    drop = drop.view(x.shape).to(x.device)
    return (x.float() * float(dropout_scale(thr))).to(x.dtype).masked_fill(drop, 0.0)
