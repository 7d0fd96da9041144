"""Fused optimizers (reference BAR/main.py:53 uses torch.optim.Adam,
BASELINE configs use SGD-momentum).

They are ``torch.optim.Optimizer`` subclasses (so the reference's
``StepLR(optimizer, step_size=25)`` and ``optimizer.param_groups[..]['lr']``
work unchanged), but when the parameters live in a FlatParams buffer the
update is ONE fused kernel over the whole model (fp32 master + momentum /
moments + bf16 shadow refresh, with the data-parallel 1/N folded in) instead
of a per-tensor loop.  Learning rate and Adam's step count are handed to the
kernel through a small device tensor, so the update can sit inside a captured
hipGraph.  Without FlatParams (or on CPU) the same math runs as torch ops.

``max_grad_norm`` (default None = off) clips by the global L2 norm with
``torch.nn.utils.clip_grad_norm_`` semantics: the gradient is multiplied by
``min(1, max_norm / (total_norm + 1e-6))`` before weight decay and momentum, and a
step whose norm is not finite is SKIPPED (no parameter, momentum / moment, shadow or
Adam step-count change).  On the flat GPU path the norm (``grad_sumsq`` partials +
``clip_finalize``) and the coefficient stay on the device: the fused kernels read them
from a small state tensor, the threshold is written into that tensor by the host like
the learning rate, so the clipped update replays from a hipGraph.  Under
``DataParallel(shard_optimizer=True)`` each rank sums the squares of its own shard
ranges (rank 0 also the replicated tail) and ONE scalar all-reduce makes the norm
global.  Limits: SGD's ``first_step`` flag stays host-driven, so on the fused path a
skipped very first step differs from torch only when ``dampening != 0`` (the next step
then damps the gradient it seeds the momentum with); a sum of squares that overflows
fp32 counts as non-finite; the counters are fp32 device scalars (exact to 2**24) and
are not saved in checkpoints.  The device-only norm needs ONE param group holding one
flat buffer: with several groups (one shared threshold) the norm is taken with torch ops
and its skip flag is read on the host -- a host sync per step, and such an optimizer
cannot be captured into a graph.  A graph captured with clipping on keeps its clipping
kernels: setting ``max_grad_norm`` to None afterwards makes the replays run them with an
infinite threshold (coefficient 1, non-finite steps still skipped); a graph captured with
clipping off never clips, whatever is set later -- capture again.
"""
from __future__ import annotations

import math

import torch

from ..ops import _ext
from ..utils.flat_params import owner_of




def _refuse_partial_sharded(params):
    """A param group that does not map onto one whole FlatParams would take the per-tensor
    update path; on a sharded DataParallel buffer (only this rank's shard of flat.grad is
    reduced, and nothing all-gathers the result) that silently diverges the replicas."""
    for p in params:
        f = owner_of(p)
        if f is not None and getattr(f, "shard_sync", None) is not None:
            raise RuntimeError("DataParallel(shard_optimizer=True): the optimizer's param group must hold "
                               "every parameter of the model's flat buffer (one group, built AFTER the "
                               "DataParallel wrapper)")


# slots of the clipping state tensor (csrc/include/ldnn_kernels.h ClipSlot)
_CLIP_MAX, _CLIP_COEF, _CLIP_SKIP, _CLIP_NORM, _CLIP_STEPS, _CLIP_CLIPPED, _CLIP_SKIPPED, _CLIP_LEN = 0, 1, 2, 3, 4, 5, 6, 8
# device-only entries of _ls(): rebuilt by an eager step, never saved
_TRANSIENT = ("hp", "clip", "clip_scratch", "clip_local")


class _FlatOptimizer(torch.optim.Optimizer):
    def _ls(self) -> dict:
        """Fused (flat-buffer) optimizer state: momentum / moments / step / hp (+ the
        clipping state and scratch)."""
        return self.__dict__.setdefault("_ldnn_state", {})

    def state_dict(self):
        sd = super().state_dict()
        ls = self._ls()
        flat = {k: v for k, v in ls.items() if k not in _TRANSIENT}
        if self._clip_threshold() is not None and "hp" in ls and "exp_avg" in ls:
            # the fused Adam's step count lives on the device: skipped steps did not advance it
            flat["step"] = int(ls["hp"][1].item())
        sd["ldnn_flat_state"] = flat
        return sd

    # ---- global-norm gradient clipping ------------------------------------------------
    def _clip_threshold(self):
        """The clipping threshold (None: off).  One threshold for the whole optimizer."""
        vals = [g.get("max_grad_norm") for g in self.param_groups]
        vals = [None if v is None or float(v) <= 0 else float(v) for v in vals]
        if any(v != vals[0] for v in vals):
            raise ValueError(f"max_grad_norm must be the same in every param group (the norm is global); got {vals}")
        return vals[0] if vals else None

    def _clip_state(self, device, scratch: int = 0):
        """The device clipping state [max_norm, coef, skip, last_norm, steps, clipped, skipped, -]
        (and ``scratch`` partial slots + the 1-element local sum for the native kernels), with
        the current threshold written -- like ``hp``: allocated by an eager step, read by graphs."""
        st = self._ls()
        cl = st.get("clip")
        capturing = getattr(self, "_ldnn_capturing", False)
        if cl is None or cl.device != device:
            if capturing:
                raise RuntimeError("run an eager optimizer step before capturing it into a graph")
            cl = torch.zeros(_CLIP_LEN, dtype=torch.float32, device=device)
            st["clip"] = cl
        if scratch:
            sc = st.get("clip_scratch")
            if sc is None or sc.device != device or sc.numel() < scratch:
                if capturing:
                    raise RuntimeError("run an eager optimizer step before capturing it into a graph")
                st["clip_scratch"] = torch.zeros(scratch, dtype=torch.float32, device=device)
                st["clip_local"] = torch.zeros(1, dtype=torch.float32, device=device)
        if not capturing:
            cl[_CLIP_MAX].fill_(self._clip_threshold())
        return cl

    def grad_clip_stats(self):
        """Device scalars ``last_norm`` / ``steps`` / ``clipped`` / ``skipped`` of the clipped
        steps so far (reading one syncs), or None when clipping is off."""
        if self._clip_threshold() is None:
            return None
        cl = self._ls().get("clip")
        if cl is None:
            ps = self.param_groups[0]["params"]
            cl = self._clip_state(ps[0].device if ps else torch.device("cpu"))
        return {"last_norm": cl[_CLIP_NORM], "steps": cl[_CLIP_STEPS], "clipped": cl[_CLIP_CLIPPED],
                "skipped": cl[_CLIP_SKIPPED]}

    @staticmethod
    def _clip_finalize_torch(cl, total_sq, grad_scale=1.0):
        """clip_finalize's math in torch ops: ``total_sq`` = the sum of squares (0-d / 1-element)."""
        norm = (total_sq.reshape(()).double().sqrt() * grad_scale).float()
        finite = torch.isfinite(norm)
        coef = torch.where(finite, (cl[_CLIP_MAX] / (norm + 1e-6)).clamp(max=1.0), torch.zeros_like(norm))
        cl[_CLIP_COEF] = coef
        cl[_CLIP_SKIP] = (~finite).float()
        cl[_CLIP_NORM] = norm
        cl[_CLIP_STEPS] += 1
        cl[_CLIP_CLIPPED] += (finite & (coef < 1)).float()
        cl[_CLIP_SKIPPED] += (~finite).float()

    def _clip_begin(self):
        """Start of a clipped step: the global norm over EVERY group's gradient, before any
        update.  Returns None (off, or a sharded flat buffer: ``_sharded_step`` does it with
        its scalar all-reduce), else ``(state, skip)`` -- ``skip`` None on the fused path
        (the kernels read the flag on the device), a host bool on the torch paths."""
        if self._clip_threshold() is None:
            return None
        flats = [self._flat_for_group(g) for g in self.param_groups]
        f = flats[0] if len(flats) == 1 else None
        if f is not None and getattr(f, "shard_sync", None) is not None:
            return None
        if f is not None and _ext.use_native(f.master):
            f.finalize_grads()
            C = _ext.C()
            cl = self._clip_state(f.master.device, C.grad_sumsq_parts(f.grad.numel()))
            sc = self._ls()["clip_scratch"]
            C.clip_finalize(sc, C.grad_sumsq(f.grad, sc, 0), cl, f.grad_scale)
            return cl, None
        total, dev = None, None
        for g, fl in zip(self.param_groups, flats):
            if fl is not None:
                fl.finalize_grads()
                terms = [(fl.grad.double() * fl.grad_scale).square().sum()]
            else:
                terms = [p.grad.double().square().sum() for p in g["params"] if p.grad is not None]
            for t in terms:
                dev = t.device if dev is None else dev
                total = t if total is None else total + t.to(dev)
        if total is None:
            return None
        cl = self._clip_state(dev)
        self._clip_finalize_torch(cl, total)
        return cl, bool(cl[_CLIP_SKIP].item())

    def load_state_dict(self, state_dict):
        state_dict = dict(state_dict)
        flat_state = state_dict.pop("ldnn_flat_state", {})
        super().load_state_dict(state_dict)
        ls = self._ls()
        ls.clear()
        for k, v in flat_state.items():
            ls[k] = v.clone() if torch.is_tensor(v) else v
        # re-home buffers onto the parameters' device
        for group in self.param_groups:
            f = self._flat_for_group(group)
            if f is not None:
                for k, v in list(ls.items()):
                    if torch.is_tensor(v):
                        ls[k] = v.to(f.master.device)

    def _flat_for_group(self, group):
        ps = group["params"]
        if not ps:
            return None
        f = owner_of(ps[0])
        if f is None or any(owner_of(p) is not f for p in ps) or len(ps) != len(f.segments):
            _refuse_partial_sharded(ps)
            return None
        return f

    def _hp(self, flat, lr):
        st = self._ls()
        hp = st.get("hp")
        if hp is None or hp.device != flat.master.device:
            if getattr(self, "_ldnn_capturing", False):
                raise RuntimeError("run an eager optimizer step before capturing it into a graph")
            hp = torch.zeros(2, dtype=torch.float32, device=flat.master.device)
            hp[1] = float(st.get("step", 0))
            st["hp"] = hp
        # inside a hipGraph capture the lr write is NOT recorded: the graph reads hp,
        # and GraphedStep refreshes it (sync_hyperparams) whenever the lr changes
        if not getattr(self, "_ldnn_capturing", False):
            hp[0].fill_(lr)
        return hp

    @torch.no_grad()
    def sync_hyperparams(self):
        """Write the current learning rate (and clipping threshold) into the device
        hyper-parameter tensors."""
        hp = self._ls().get("hp")
        if hp is not None:
            hp[0].fill_(self.param_groups[0]["lr"])
        cl = self._ls().get("clip")
        if cl is not None:
            # (clipping switched off after a graph was captured: an infinite threshold makes the
            # captured kernels' coefficient 1; the non-finite guard of that graph stays)
            mx = self._clip_threshold()
            cl[_CLIP_MAX].fill_(mx if mx is not None else float("inf"))

    def _buf(self, name, like):
        st = self._ls()
        b = st.get(name)
        if b is None or b.shape != like.shape or b.device != like.device:
            b = torch.zeros_like(like)
            st[name] = b
        return b

    # ---- range updates (optimizer overlapped with the backward, train/graphed.py) ----
    def range_updater(self):
        """A ``_RangeUpdate`` for ONE step of a single flat-buffer group on the GPU
        (None when the optimizer cannot update by ranges: several groups, no
        FlatParams, CPU).  ``update(lo, hi)`` runs the fused kernel on flat elements
        [lo, hi) on the current stream; ``end()`` closes the step.  Every element must
        be covered exactly once per step."""
        if not self.supports_ranges():
            return None
        group = self.param_groups[0]
        return _RangeUpdate(self, self._flat_for_group(group), group)

    def supports_ranges(self) -> bool:
        if self._clip_threshold() is not None:
            return False   # the whole norm must be known before any range updates
        if len(self.param_groups) != 1 or type(self)._update_range is _FlatOptimizer._update_range:
            return False
        f = self._flat_for_group(self.param_groups[0])
        return f is not None and _ext.use_native(f.master)

    def _begin_ranges(self, f, group, clip=None):  # per-step setup on the current stream (subclasses)
        return {}

    def _update_range(self, f, group, ctx, lo, hi):
        raise NotImplementedError

    def _sharded_step(self, f, group) -> bool:
        """DataParallel(shard_optimizer=True) owns ``f``: update only this rank's flat
        ranges (its shard of every reduce-scattered bucket + the replicated tail), then
        let the data-parallel wrapper start the weight all-gathers.  False otherwise."""
        sh = getattr(f, "shard_sync", None)
        if sh is None:
            return False
        if len(self.param_groups) != 1:
            # the full-replica update below would read flat.grad, of which only this rank's
            # shards hold reduced values, and no weight all-gather would follow: replicas
            # would silently diverge
            raise RuntimeError("DataParallel(shard_optimizer=True) needs ONE param group holding the whole "
                               f"flat buffer; this optimizer has {len(self.param_groups)}")
        f.finalize_grads()
        if self._clip_threshold() is not None:
            return self._sharded_step_clipped(f, group, sh)
        ctx = self._begin_ranges(f, group)
        parts = getattr(sh, "step_parts", None)
        if parts is not None:   # the caller interleaves its own work per bucket (GraphedDPStep capture)
            parts(lambda lo, hi: self._update_range(f, group, ctx, lo, hi) if hi > lo else None)
        else:
            for lo, hi in sh.update_ranges():
                if hi > lo:
                    self._update_range(f, group, ctx, lo, hi)
        st = self._ls()
        st["step"] = st.get("step", 0) + 1
        sh.after_update()
        return True

    def _sharded_step_clipped(self, f, group, sh) -> bool:
        """The sharded step with global-norm clipping, in three phases: ``norm`` (sums of
        squares of this rank's shard ranges -- on rank 0 also of the replicated tail, which
        every rank holds alike, so it is counted once -- into one local scalar), ONE scalar
        all-reduce, ``update`` (finalize the coefficient, then every range update).  Every
        bucket's post_collective has run before.  ``sh.clip_phases(norm, local, update)``: a
        caller that captures the two compute phases into graphs and issues the all-reduce
        itself (GraphedDPStep); else the all-reduce goes through ``sh.comm`` here."""
        native = _ext.use_native(f.master)
        ranges = [(lo, hi) for lo, hi in sh.norm_ranges() if hi > lo]
        st = self._ls()
        if native:
            C = _ext.C()
            cl = self._clip_state(f.master.device, max(1, sum(C.grad_sumsq_parts(hi - lo) for lo, hi in ranges)))
        else:
            cl = self._clip_state(f.master.device)
            if st.get("clip_local") is None or st["clip_local"].device != f.master.device:
                st["clip_local"] = torch.zeros(1, dtype=torch.float32, device=f.master.device)
        local = st["clip_local"]

        def norm():
            if native:
                sc, slot = st["clip_scratch"], 0
                for lo, hi in ranges:
                    slot += C.grad_sumsq(f.grad[lo:hi], sc, slot)
                C.sumsq_total(sc, slot, local)
            else:
                tot = torch.zeros((), dtype=torch.float64, device=f.master.device)
                for lo, hi in ranges:
                    tot = tot + f.grad[lo:hi].double().square().sum()
                local.copy_(tot.reshape(1))

        def update():
            if native:
                C.clip_finalize(st["clip_scratch"], 0, cl, f.grad_scale, ext=local)
                skip = None
            else:
                self._clip_finalize_torch(cl, local, f.grad_scale)
                skip = bool(cl[_CLIP_SKIP].item())
            if skip:   # (torch path: decided on the host; the fused kernels read the flag themselves)
                return
            ctx = self._begin_ranges(f, group, clip=(cl, skip))
            for lo, hi in sh.update_ranges():
                if hi > lo:
                    self._update_range(f, group, ctx, lo, hi)
            st["step"] = st.get("step", 0) + 1

        phases = getattr(sh, "clip_phases", None)
        if phases is not None:
            phases(norm, local, update)
        else:
            norm()
            sh.comm.all_reduce(local)
            update()
        sh.after_update()
        return True

    def zero_grad(self, set_to_none: bool = True):
        for group in self.param_groups:
            f = self._flat_for_group(group)
            if f is not None:
                # (set_to_none: the next backward's first write overwrites instead of a fill)
                f.zero_grad(lazy=set_to_none)
            else:
                for p in group["params"]:
                    if p.grad is not None:
                        if set_to_none and owner_of(p) is None:
                            p.grad = None
                        else:
                            p.grad.zero_()


class SGD(_FlatOptimizer):
    def __init__(self, params, lr=0.01, momentum=0.0, dampening=0.0, weight_decay=0.0, nesterov=False,
                 max_grad_norm=None):
        super().__init__(params, dict(lr=lr, momentum=momentum, dampening=dampening, weight_decay=weight_decay,
                                      nesterov=nesterov, max_grad_norm=max_grad_norm))

    @torch.no_grad()
    def step(self, closure=None, clear_grads: bool = False):
        """clear_grads: the update kernel also zeroes the flat gradient after reading it
        (one pass instead of a later zero_grad fill; on MI355X the zero writes inside
        the bandwidth-bound update cost about what the fill launch does)."""
        loss = closure() if closure is not None else None
        clip = self._clip_begin()
        cl, skip = clip if clip is not None else (None, None)
        for group in self.param_groups:
            lr, mu, damp, wd, nest = (group[k] for k in ("lr", "momentum", "dampening", "weight_decay", "nesterov"))
            f = self._flat_for_group(group)
            if f is not None and self._sharded_step(f, group):
                continue
            if f is not None:
                f.finalize_grads()
                st = self._ls()
                first = st.get("step", 0) == 0
                mom = self._buf("momentum", f.master) if mu != 0 else f.master
                if _ext.use_native(f.master):
                    _ext.C().sgd_step(f.master, f.grad, mom, f.shadow, self._hp(f, lr), f.grad_scale, mu, damp, wd,
                                      nest, first, zero_ranges=[(0, f.grad.numel())] if clear_grads else [],
                                      clip=cl.to(f.master.device) if cl is not None else None)
                else:
                    if not skip:
                        g = f.grad * f.grad_scale
                        self._sgd_torch(f.master, g if cl is None else g * cl[_CLIP_COEF], mom if mu != 0 else None,
                                        lr, mu, damp, wd, nest, first)
                        if f.shadow is not None:
                            f.shadow.copy_(f.master)
                    if clear_grads:
                        f.grad.zero_()
                    if skip:
                        continue
                st["step"] = st.get("step", 0) + 1
            else:
                if skip:
                    continue
                for p in group["params"]:
                    if p.grad is None:
                        continue
                    if cl is not None:
                        p.grad.mul_(cl[_CLIP_COEF].to(p.grad.device))
                    ps = self.state.setdefault(p, {})
                    first = "momentum_buffer" not in ps
                    if mu != 0 and first:
                        ps["momentum_buffer"] = torch.zeros_like(p)
                    self._sgd_torch(p.data, p.grad, ps.get("momentum_buffer"), lr, mu, damp, wd, nest, first)
        return loss

    def _begin_ranges(self, f, group, clip=None):
        mu = group["momentum"]
        hp = self._hp(f, group["lr"]) if _ext.use_native(f.master) else None
        return dict(hp=hp, first=self._ls().get("step", 0) == 0, clip=clip[0] if clip is not None else None,
                    mom=self._buf("momentum", f.master) if mu != 0 else f.master)

    def _update_range(self, f, group, ctx, lo, hi):
        sh = f.shadow[lo:hi] if f.shadow is not None else None
        if not _ext.use_native(f.master):
            mu = group["momentum"]
            g = f.grad[lo:hi] * f.grad_scale
            if ctx["clip"] is not None:
                g = g * ctx["clip"][_CLIP_COEF]
            self._sgd_torch(f.master[lo:hi], g, ctx["mom"][lo:hi] if mu != 0 else None,
                            group["lr"], mu, group["dampening"], group["weight_decay"], group["nesterov"], ctx["first"])
            if sh is not None:
                sh.copy_(f.master[lo:hi])
            return
        _ext.C().sgd_step(f.master[lo:hi], f.grad[lo:hi], ctx["mom"][lo:hi], sh, ctx["hp"], f.grad_scale,
                          group["momentum"], group["dampening"], group["weight_decay"], group["nesterov"],
                          ctx["first"], clip=ctx["clip"])

    @staticmethod
    def _sgd_torch(p, g, buf, lr, mu, damp, wd, nest, first):
        if wd != 0:
            g = g + wd * p
        if mu != 0:
            if first:
                buf.copy_(g)
            else:
                buf.mul_(mu).add_(g, alpha=1 - damp)
            g = g + mu * buf if nest else buf
        p.add_(g, alpha=-lr)


class Adam(_FlatOptimizer):
    decoupled = False

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, max_grad_norm=None):
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay,
                                      max_grad_norm=max_grad_norm))

    @torch.no_grad()
    def step(self, closure=None, clear_grads: bool = False):
        """clear_grads: as SGD.step."""
        loss = closure() if closure is not None else None
        clip = self._clip_begin()
        cl, skip = clip if clip is not None else (None, None)
        for group in self.param_groups:
            lr, (b1, b2), eps, wd = group["lr"], group["betas"], group["eps"], group["weight_decay"]
            f = self._flat_for_group(group)
            if f is not None and self._sharded_step(f, group):
                continue
            if f is not None:
                f.finalize_grads()
                st = self._ls()
                m, v = self._buf("exp_avg", f.master), self._buf("exp_avg_sq", f.master)
                if _ext.use_native(f.master):
                    hp = self._hp(f, lr)
                    dcl = cl.to(f.master.device) if cl is not None else None
                    _ext.C().bump_step(hp, clip=dcl)
                    _ext.C().adam_step(f.master, f.grad, m, v, f.shadow, hp, f.grad_scale, b1, b2, eps, wd,
                                       self.decoupled, zero_ranges=[(0, f.grad.numel())] if clear_grads else [],
                                       clip=dcl)
                    st["step"] = st.get("step", 0) + 1
                else:
                    if not skip:
                        st["step"] = st.get("step", 0) + 1
                        g = f.grad * f.grad_scale
                        self._adam_torch(f.master, g if cl is None else g * cl[_CLIP_COEF], m, v, st["step"], lr, b1,
                                         b2, eps, wd)
                        if f.shadow is not None:
                            f.shadow.copy_(f.master)
                    if clear_grads:
                        f.grad.zero_()
            else:
                if skip:
                    continue
                for p in group["params"]:
                    if p.grad is None:
                        continue
                    if cl is not None:
                        p.grad.mul_(cl[_CLIP_COEF].to(p.grad.device))
                    ps = self.state.setdefault(p, {})
                    if "exp_avg" not in ps:
                        ps["exp_avg"] = torch.zeros_like(p)
                        ps["exp_avg_sq"] = torch.zeros_like(p)
                        ps["step"] = 0
                    ps["step"] += 1
                    self._adam_torch(p.data, p.grad, ps["exp_avg"], ps["exp_avg_sq"], ps["step"], lr, b1, b2, eps,
                                     wd)
        return loss

    def _begin_ranges(self, f, group, clip=None):
        hp = None
        cl = clip[0] if clip is not None else None
        if _ext.use_native(f.master):
            hp = self._hp(f, group["lr"])
            _ext.C().bump_step(hp, clip=cl)   # once per step, before any range reads the step count
        return dict(hp=hp, clip=cl, m=self._buf("exp_avg", f.master), v=self._buf("exp_avg_sq", f.master),
                    t=self._ls().get("step", 0) + 1)

    def _update_range(self, f, group, ctx, lo, hi):
        b1, b2 = group["betas"]
        sh = f.shadow[lo:hi] if f.shadow is not None else None
        if not _ext.use_native(f.master):
            g = f.grad[lo:hi] * f.grad_scale
            if ctx["clip"] is not None:
                g = g * ctx["clip"][_CLIP_COEF]
            self._adam_torch(f.master[lo:hi], g, ctx["m"][lo:hi], ctx["v"][lo:hi],
                             ctx["t"], group["lr"], b1, b2, group["eps"], group["weight_decay"])
            if sh is not None:
                sh.copy_(f.master[lo:hi])
            return
        _ext.C().adam_step(f.master[lo:hi], f.grad[lo:hi], ctx["m"][lo:hi], ctx["v"][lo:hi], sh, ctx["hp"],
                           f.grad_scale, b1, b2, group["eps"], group["weight_decay"], self.decoupled,
                           clip=ctx["clip"])

    def _adam_torch(self, p, g, m, v, t, lr, b1, b2, eps, wd):
        if wd != 0:
            if self.decoupled:
                p.mul_(1 - lr * wd)
            else:
                g = g + wd * p
        m.mul_(b1).add_(g, alpha=1 - b1)
        v.mul_(b2).addcmul_(g, g, value=1 - b2)
        bc1 = 1 - b1 ** t
        bc2 = 1 - b2 ** t
        denom = (v.sqrt() / math.sqrt(bc2)).add_(eps)
        p.addcdiv_(m, denom, value=-lr / bc1)


class AdamW(Adam):
    decoupled = True

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, max_grad_norm=None):
        super().__init__(params, lr, betas, eps, weight_decay, max_grad_norm)


def build_optimizer(name: str, params, lr: float, momentum: float = 0.9, weight_decay: float = 0.0,
                    max_grad_norm: float | None = None):
    """max_grad_norm: clip by the global L2 norm (None or <= 0: off)."""
    name = name.lower()
    if max_grad_norm is not None and max_grad_norm <= 0:
        max_grad_norm = None
    if name == "sgd":
        return SGD(params, lr=lr, momentum=momentum, weight_decay=weight_decay, max_grad_norm=max_grad_norm)
    if name == "adam":
        return Adam(params, lr=lr, weight_decay=weight_decay, max_grad_norm=max_grad_norm)
    if name == "adamw":
        return AdamW(params, lr=lr, weight_decay=weight_decay, max_grad_norm=max_grad_norm)
    raise ValueError(f"unknown optimizer {name!r}")


class _RangeUpdate:
    """One optimizer step applied as several flat-range launches (see
    ``_FlatOptimizer.range_updater``)."""

    def __init__(self, opt, flat, group):
        self.opt, self.flat, self.group = opt, flat, group
        self.ctx = opt._begin_ranges(flat, group)
        self.done = 0

    @torch.no_grad()
    def update(self, lo: int, hi: int):
        if hi > lo:
            self.opt._update_range(self.flat, self.group, self.ctx, lo, hi)
            self.done += hi - lo

    def end(self):
        if self.done != self.flat.numel:
            raise RuntimeError(f"range updates covered {self.done} of {self.flat.numel} flat elements")
        st = self.opt._ls()
        st["step"] = st.get("step", 0) + 1
