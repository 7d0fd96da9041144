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

``SGD(lars_trust=...)`` (default None = off; ``build_optimizer("lars")``) adds LARS: see the
class.  It is the per-tensor form of the same plumbing -- ``seg_sumsq`` + ``lars_finalize``
leave one trust ratio per parameter tensor on the device, the fused SGD looks it up per
64-element block, and the sharded step all-reduces the ``2S`` per-segment sums (clipping's
scalar behind them) in its one extra collective.
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
_TRANSIENT = ("hp", "clip", "clip_scratch", "clip_local", "lars")
# LARS ratio table: one slot per uint16 map value, so every map entry is in bounds; the slots
# past the segments are never written and hold 1 (alignment gaps map to the last one)
_LARS_SLOTS, _LARS_GAP = 65536, 65535
_CAPTURE_MSG = "run an eager optimizer step before capturing it into a graph"


def lars_chunk_table(bounds, ranges, chunk):
    """The seg_sumsq tables (host lists) for segments ``bounds`` = [(begin, end)] restricted to
    the flat ``ranges``: ``chunks`` rows (segment, begin / 64, end / 64, 0) of at most ``chunk``
    elements, never across a segment boundary, a segment's chunks consecutive; ``segs`` rows
    (first chunk, end chunk) per segment.  Everything must lie on 64-element boundaries."""
    for lo, hi in list(ranges) + list(bounds):
        if lo % 64 or hi % 64 or lo < 0 or hi < lo:
            raise ValueError(f"LARS: the flat range [{lo}, {hi}) is not 64-element aligned")
    if chunk <= 0 or chunk % 64:
        raise ValueError(f"LARS: chunk {chunk} must be a positive multiple of 64")
    rs = sorted((lo, hi) for lo, hi in ranges if hi > lo)
    chunks, segs = [], []
    for s, (b, e) in enumerate(bounds):
        first = len(chunks)
        for lo, hi in rs:
            x, y = max(b, lo), min(e, hi)
            while x < y:
                z = min(x + chunk, y)
                chunks.append((s, x // 64, z // 64, 0))
                x = z
        segs.append((first, len(chunks)))
    return chunks, segs


class _Lars:
    """Device state of LARS over one flat buffer (or, ``flat`` None, over loose tensors)."""

    def __init__(self, flat, params, exclude_1d, device):
        self.flat, self.device, self.exclude_1d = flat, device, exclude_1d
        if flat is not None:
            segs = flat.segments
            self.names = [s.name for s in segs]
            self.adapt = [not (exclude_1d and s.param.dim() < 2) for s in segs]
            self.bounds = [(s.offset, s.offset + (s.storage_numel + 63) // 64 * 64) for s in segs]
            if len(segs) >= _LARS_GAP:
                raise ValueError(f"LARS: {len(segs)} parameter tensors exceed the uint16 segment map")
            seg_of = torch.full((flat.numel // 64,), _LARS_GAP, dtype=torch.int64)
            for i, (b, e) in enumerate(self.bounds):
                if b % 64 or e > flat.numel:
                    raise ValueError(f"LARS: segment {self.names[i]} is not 64-element aligned in the flat buffer")
                seg_of[b // 64: e // 64] = i
            self.seg_of = seg_of.to(device)               # torch paths index with it
            self.segmap = seg_of.to(torch.uint16).to(device)   # the fused kernel's map
        else:
            self.names = [f"param{i}" for i in range(len(params))]
            self.adapt = [not (exclude_1d and p.dim() < 2) for p in params]
        self.S = S = len(self.names)
        self.adapt_t = torch.tensor(self.adapt, dtype=torch.bool, device=device)
        self.hdr = torch.zeros(2, dtype=torch.float32, device=device)
        self.ratio = torch.ones(max(_LARS_SLOTS, S + 1), dtype=torch.float32, device=device)
        self.w_norm = torch.zeros(S, dtype=torch.float32, device=device)
        self.g_norm = torch.zeros(S, dtype=torch.float32, device=device)
        self.local = torch.zeros(2 * S + 1, dtype=torch.float32, device=device)   # sharded: [2S] sums + clip's
        self.tables = {}

    def table(self, ranges, capturing):
        """Device chunk tables + partial slots of seg_sumsq over ``ranges`` (built once per set)."""
        key = tuple(ranges)
        t = self.tables.get(key)
        if t is None:
            if capturing:
                raise RuntimeError(_CAPTURE_MSG)
            chunks, segs = lars_chunk_table(self.bounds, ranges, _ext.C().seg_sumsq_chunk())
            segtab = [(a, b, int(ad), 0) for (a, b), ad in zip(segs, self.adapt)]
            i32 = dict(dtype=torch.int32, device=self.device)
            t = dict(ranges=[tuple(r) for r in ranges],
                     chunks=torch.tensor(chunks, **i32).reshape(-1, 4), segtab=torch.tensor(segtab, **i32).reshape(-1, 4),
                     partials=torch.zeros(2 * len(chunks), dtype=torch.float32, device=self.device))
            self.tables[key] = t
        return t

    def elem_ratio(self, lo, hi):
        """The ratio of every element of the flat range [lo, hi) (torch paths)."""
        return self.ratio[self.seg_of[lo // 64: hi // 64]].repeat_interleave(64)


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

    # ---- LARS: per-tensor trust ratios (SGD) -------------------------------------------
    def _lars_conf(self):
        """``(trust_coef, eps, exclude_1d)``, or None when LARS is off.  One setting for the whole
        optimizer; the keys are read with .get, so state saved before they existed loads."""
        vals = []
        for g in self.param_groups:
            t = g.get("lars_trust")
            vals.append(None if t is None else (float(t), float(g.get("lars_eps", 1e-8)),
                                                bool(g.get("lars_exclude_1d", True))))
        if any(v != vals[0] for v in vals):
            raise ValueError(f"lars_trust / lars_eps / lars_exclude_1d must be the same in every param group; got {vals}")
        return vals[0] if vals else None

    def _lars_state(self, flat, params=None, device=None):
        """The LARS device state, with the current trust coefficient and eps written -- like
        ``hp``: allocated by an eager step, read by graphs."""
        trust, eps, excl = self._lars_conf()
        st = self._ls()
        L = st.get("lars")
        device = flat.master.device if flat is not None else device
        capturing = getattr(self, "_ldnn_capturing", False)
        if L is None or L.flat is not flat or L.device != device or L.exclude_1d != excl or \
                (flat is None and L.S != len(params)):
            if capturing:
                raise RuntimeError(_CAPTURE_MSG)
            L = st["lars"] = _Lars(flat, params, excl, device)
        if not capturing:
            L.hdr[0].fill_(trust)
            L.hdr[1].fill_(eps)
        return L

    def lars_stats(self):
        """In segment (flat-buffer) order: the device tensors ``ratio`` / ``w_norm`` / ``g_norm`` of
        the last LARS step, the parameter ``names`` and which tensors are ``adapted`` (reading a
        tensor syncs); None when LARS is off."""
        if self._lars_conf() is None:
            return None
        L = self._ls().get("lars")
        if L is None:
            f = self._flat_for_group(self.param_groups[0]) if len(self.param_groups) == 1 else None
            ps = [p for g in self.param_groups for p in g["params"]]
            L = self._lars_state(f, ps, ps[0].device if ps else torch.device("cpu"))
        return {"ratio": L.ratio[:L.S], "w_norm": L.w_norm, "g_norm": L.g_norm, "names": list(L.names),
                "adapted": list(L.adapt)}

    @staticmethod
    def _lars_sums_torch(L, f, ranges):
        """seg_sumsq in torch ops: [2][S] fp64 sums of squares of master / grad over ``ranges``."""
        out = torch.zeros(2, L.S + 1, dtype=torch.float64, device=L.device)
        for lo, hi in ranges:
            if lo % 64 or hi % 64:
                raise ValueError(f"LARS: the flat range [{lo}, {hi}) is not 64-element aligned")
            if hi <= lo:
                continue
            idx = L.seg_of[lo // 64: hi // 64].clamp(max=L.S)
            for k, buf in enumerate((f.master, f.grad)):
                out[k].index_add_(0, idx, buf[lo:hi].double().square().view(-1, 64).sum(1))
        return out[:, :L.S]

    @staticmethod
    def _lars_finalize_torch(L, sums, gscale, wd):
        """lars_finalize in torch ops; ``gscale`` = grad_scale (* the clip coefficient)."""
        trust, eps = L.hdr.double()
        wn = sums[0].double().sqrt()
        gn = sums[1].double().sqrt() * gscale
        r = trust * wn / (gn + wd * wn + eps)
        over = torch.isinf(sums.float()).any(0)      # (a sum of squares beyond fp32: ratio 0)
        r = torch.where(over, torch.zeros_like(r), r)
        r = torch.where(L.adapt_t & (wn > 0) & (gn > 0), r, torch.ones_like(r))
        L.ratio[:L.S] = r.float()
        L.w_norm.copy_(wn)
        L.g_norm.copy_(gn)

    def _lars_begin(self, f, group, cl):
        """The ratios of an unsharded flat step, before the update: returns the state (its
        ``ratio`` / ``segmap`` feed the fused kernel).  ``cl``: the finalized clip state or None."""
        L = self._lars_state(f)
        wd = group["weight_decay"]
        if _ext.use_native(f.master):
            C = _ext.C()
            t = L.table([(0, f.numel)], getattr(self, "_ldnn_capturing", False))
            C.seg_sumsq(f.master, f.grad, t["chunks"], t["partials"], t["ranges"], [b for b, _ in L.bounds])
            C.lars_finalize(t["partials"], t["segtab"], L.hdr, L.ratio, L.w_norm, L.g_norm, f.grad_scale, wd,
                            clip=cl)
        else:
            coef = cl[_CLIP_COEF].double() if cl is not None else 1.0
            self._lars_finalize_torch(L, self._lars_sums_torch(L, f, [(0, f.numel)]), f.grad_scale * coef, wd)
        return L

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
        """Write the current learning rate (and clipping threshold, LARS trust coefficient and
        eps) into the device hyper-parameter tensors."""
        hp = self._ls().get("hp")
        if hp is not None:
            hp[0].fill_(self.param_groups[0]["lr"])
        cl = self._ls().get("clip")
        if cl is not None:
            # (clipping switched off after a graph was captured: an infinite threshold makes the
            # captured kernels' coefficient 1; the non-finite guard of that graph stays)
            mx = self._clip_threshold()
            cl[_CLIP_MAX].fill_(mx if mx is not None else float("inf"))
        L = self._ls().get("lars")
        conf = self._lars_conf()
        if L is not None and conf is not None:
            L.hdr[0].fill_(conf[0])
            L.hdr[1].fill_(conf[1])

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
        if self._lars_conf() is not None:
            return False   # ... and so must a tensor's whole gradient before any of it moves
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
        if self._clip_threshold() is not None or self._lars_conf() is not None:
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
        """The sharded step with global-norm clipping and / or LARS, in three phases: ``norm``
        (sums of squares of this rank's shard ranges -- on rank 0 also of the replicated tail,
        which every rank holds alike, so it is counted once -- into one local vector), ONE
        all-reduce of that vector, ``update`` (finalize the coefficient / the ratios, then every
        range update).  The vector is the scalar gradient sum with clipping alone; with LARS
        the per-segment [master, grad] sums ``[2S]``, followed by clipping's scalar.  Every
        bucket's post_collective has run before.  ``sh.clip_phases(norm, local, update)``: a
        caller that captures the two compute phases into graphs and issues the all-reduce
        itself (GraphedDPStep); else the all-reduce goes through ``sh.comm`` here."""
        native = _ext.use_native(f.master)
        clipped = self._clip_threshold() is not None
        ranges = [(lo, hi) for lo, hi in sh.norm_ranges() if hi > lo]
        st = self._ls()
        L = self._lars_state(f) if self._lars_conf() is not None else None
        cl = None
        if native:
            C = _ext.C()
            if clipped:
                cl = self._clip_state(f.master.device, max(1, sum(C.grad_sumsq_parts(hi - lo) for lo, hi in ranges)))
            tab = L.table(ranges, getattr(self, "_ldnn_capturing", False)) if L is not None else None
        elif clipped:
            cl = self._clip_state(f.master.device)
            if st.get("clip_local") is None or st["clip_local"].device != f.master.device:
                st["clip_local"] = torch.zeros(1, dtype=torch.float32, device=f.master.device)
        local = st["clip_local"] if L is None else L.local
        clip_local = local[local.numel() - 1:] if clipped else None
        wd = group["weight_decay"]

        def norm():
            if native:
                if clipped:
                    sc, slot = st["clip_scratch"], 0
                    for lo, hi in ranges:
                        slot += C.grad_sumsq(f.grad[lo:hi], sc, slot)
                    C.sumsq_total(sc, slot, clip_local)
                if L is not None:
                    C.seg_sumsq(f.master, f.grad, tab["chunks"], tab["partials"], tab["ranges"],
                                [b for b, _ in L.bounds])
                    C.lars_finalize(tab["partials"], tab["segtab"], L.hdr, L.ratio, L.w_norm, L.g_norm, 1.0, 0.0,
                                    sums_out=local)
            else:
                if clipped:
                    tot = torch.zeros((), dtype=torch.float64, device=f.master.device)
                    for lo, hi in ranges:
                        tot = tot + f.grad[lo:hi].double().square().sum()
                    clip_local.copy_(tot.reshape(1))
                if L is not None:
                    local[:2 * L.S].copy_(self._lars_sums_torch(L, f, ranges).t().reshape(-1))

        def update():
            skip = None
            if native:
                if clipped:
                    C.clip_finalize(st["clip_scratch"], 0, cl, f.grad_scale, ext=clip_local)
                if L is not None:
                    C.lars_finalize(None, tab["segtab"], L.hdr, L.ratio, L.w_norm, L.g_norm, f.grad_scale, wd,
                                    ext=local, clip=cl)
            elif clipped:
                self._clip_finalize_torch(cl, clip_local, f.grad_scale)
                skip = bool(cl[_CLIP_SKIP].item())
            if skip:   # (torch path: decided on the host; the fused kernels read the flag themselves)
                return
            if L is not None and not native:
                coef = cl[_CLIP_COEF].double() if clipped else 1.0
                self._lars_finalize_torch(L, local[:2 * L.S].view(L.S, 2).t(), f.grad_scale * coef, wd)
            kw = {} if L is None else {"lars": L}
            ctx = self._begin_ranges(f, group, clip=(cl, skip) if clipped else None, **kw)
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
    """SGD (momentum / dampening / nesterov / weight decay), optionally with LARS: with
    ``lars_trust`` set (None = off) tensor i's update ``g_i + weight_decay * w_i`` is scaled by
    ``lars_trust * |w_i| / (|g_i| + weight_decay * |w_i| + lars_eps)`` before it enters the
    momentum chain (You, Gitman, Ginsburg 2017); ``g_i`` is the reduced, scaled and -- with
    ``max_grad_norm`` -- clipped gradient.  The ratio is 1 for a tensor whose weight or gradient
    norm is zero and, with ``lars_exclude_1d`` (default), for tensors with ``dim() < 2`` (biases,
    BatchNorm affine).  On the flat GPU path ``seg_sumsq`` + ``lars_finalize`` leave the ratios
    on the device and the fused kernel looks them up per 64-element block; the trust
    coefficient and eps are device scalars written like the lr, so a captured graph follows a
    schedule on them.  No non-finite guard of its own: NaN norms fail the ``> 0`` tests (ratio 1)
    and the NaN elements propagate as in torch; a per-tensor sum of squares that overflows
    fp32 gives that tensor ratio 0.  ``lars_stats()`` reports the last ratios and norms."""

    def __init__(self, params, lr=0.01, momentum=0.0, dampening=0.0, weight_decay=0.0, nesterov=False,
                 max_grad_norm=None, lars_trust=None, lars_eps=1e-8, lars_exclude_1d=True):
        if lars_trust is not None and lars_trust <= 0:
            raise ValueError(f"lars_trust must be positive (None: LARS off); got {lars_trust}")
        super().__init__(params, dict(lr=lr, momentum=momentum, dampening=dampening, weight_decay=weight_decay,
                                      nesterov=nesterov, max_grad_norm=max_grad_norm, lars_trust=lars_trust,
                                      lars_eps=lars_eps, lars_exclude_1d=lars_exclude_1d))

    @torch.no_grad()
    def step(self, closure=None, clear_grads: bool = False):
        """clear_grads: the update kernel also zeroes the flat gradient after reading it
        (one pass instead of a later zero_grad fill; on MI355X the zero writes inside
        the bandwidth-bound update cost about what the fill launch does)."""
        loss = closure() if closure is not None else None
        clip = self._clip_begin()
        cl, skip = clip if clip is not None else (None, None)
        lars = self._lars_conf()
        loose = None   # LARS over tensors outside a flat buffer: [param index, rows of (ratio, wn, gn)]
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
                    dcl = cl.to(f.master.device) if cl is not None else None
                    L = self._lars_begin(f, group, dcl) if lars is not None else None
                    _ext.C().sgd_step(f.master, f.grad, mom, f.shadow, self._hp(f, lr), f.grad_scale, mu, damp, wd,
                                      nest, first, zero_ranges=[(0, f.grad.numel())] if clear_grads else [],
                                      clip=dcl, lars=(L.ratio, L.segmap) if L is not None else None)
                else:
                    if not skip:
                        g = f.grad * f.grad_scale
                        L = self._lars_begin(f, group, cl) if lars is not None else None
                        self._sgd_torch(f.master, g if cl is None else g * cl[_CLIP_COEF], mom if mu != 0 else None,
                                        lr, mu, damp, wd, nest, first,
                                        ratio=L.elem_ratio(0, f.numel) if L is not None else None)
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
                if lars is not None and loose is None:
                    ps_all = [p for g_ in self.param_groups for p in g_["params"]]
                    loose = [0, self._lars_state(None, ps_all, ps_all[0].device)]
                for p in group["params"]:
                    if loose is not None:
                        k = loose[0]
                        loose[0] += 1
                    if p.grad is None:
                        continue
                    if cl is not None:
                        p.grad.mul_(cl[_CLIP_COEF].to(p.grad.device))
                    ps = self.state.setdefault(p, {})
                    first = "momentum_buffer" not in ps
                    if mu != 0 and first:
                        ps["momentum_buffer"] = torch.zeros_like(p)
                    ratio = None
                    if loose is not None:
                        L = loose[1]
                        wn, gn = float(p.detach().double().norm()), float(p.grad.double().norm())
                        ratio = 1.0
                        if L.adapt[k] and wn > 0 and gn > 0:
                            ratio = lars[0] * wn / (gn + wd * wn + lars[1])
                        L.ratio[k], L.w_norm[k], L.g_norm[k] = ratio, wn, gn
                    self._sgd_torch(p.data, p.grad, ps.get("momentum_buffer"), lr, mu, damp, wd, nest, first,
                                    ratio=ratio)
        return loss

    def _begin_ranges(self, f, group, clip=None, lars=None):
        mu = group["momentum"]
        hp = self._hp(f, group["lr"]) if _ext.use_native(f.master) else None
        return dict(hp=hp, first=self._ls().get("step", 0) == 0, clip=clip[0] if clip is not None else None,
                    mom=self._buf("momentum", f.master) if mu != 0 else f.master, lars=lars)

    def _update_range(self, f, group, ctx, lo, hi):
        sh = f.shadow[lo:hi] if f.shadow is not None else None
        L = ctx.get("lars")
        if not _ext.use_native(f.master):
            mu = group["momentum"]
            g = f.grad[lo:hi] * f.grad_scale
            if ctx["clip"] is not None:
                g = g * ctx["clip"][_CLIP_COEF]
            self._sgd_torch(f.master[lo:hi], g, ctx["mom"][lo:hi] if mu != 0 else None,
                            group["lr"], mu, group["dampening"], group["weight_decay"], group["nesterov"], ctx["first"],
                            ratio=L.elem_ratio(lo, hi) if L is not None else None)
            if sh is not None:
                sh.copy_(f.master[lo:hi])
            return
        if L is not None and (lo % 64 or hi % 64):
            raise ValueError(f"LARS: the update range [{lo}, {hi}) is not 64-element aligned")
        _ext.C().sgd_step(f.master[lo:hi], f.grad[lo:hi], ctx["mom"][lo:hi], sh, ctx["hp"], f.grad_scale,
                          group["momentum"], group["dampening"], group["weight_decay"], group["nesterov"],
                          ctx["first"], clip=ctx["clip"],
                          lars=(L.ratio, L.segmap[lo // 64: hi // 64]) if L is not None else None)

    @staticmethod
    def _sgd_torch(p, g, buf, lr, mu, damp, wd, nest, first, ratio=None):
        if wd != 0:
            g = g + wd * p
        if ratio is not None:
            g = g * ratio
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
                    max_grad_norm: float | None = None, **lars):
    """max_grad_norm: clip by the global L2 norm (None or <= 0: off).  "lars": SGD with
    ``lars_trust=0.001``; ``lars_trust`` / ``lars_eps`` / ``lars_exclude_1d`` go to SGD (and
    "sgd" takes them too); Adam and AdamW refuse them."""
    name = name.lower()
    if max_grad_norm is not None and max_grad_norm <= 0:
        max_grad_norm = None
    bad = set(lars) - {"lars_trust", "lars_eps", "lars_exclude_1d"}
    if bad or (lars and name in ("adam", "adamw")):
        raise TypeError(f"build_optimizer({name!r}) got unexpected keyword arguments {sorted(bad or lars)}")
    if name == "lars":
        lars.setdefault("lars_trust", 0.001)
        return SGD(params, lr=lr, momentum=momentum, weight_decay=weight_decay, max_grad_norm=max_grad_norm, **lars)
    if name == "sgd":
        return SGD(params, lr=lr, momentum=momentum, weight_decay=weight_decay, max_grad_norm=max_grad_norm, **lars)
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
