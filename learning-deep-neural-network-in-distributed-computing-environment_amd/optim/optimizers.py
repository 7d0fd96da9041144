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

``Lamb`` (``build_optimizer("lamb")``) is the Adam-side counterpart: see the class.  Its trust
ratio needs the norm of the Adam direction formed from THIS step's moments, so the step has a
second reduce stage (``_FlatStep.moments`` / ``ratios``): ``lamb_moments`` updates the moments and
reduces per tensor, ``lamb_finalize`` leaves the ratios on the device, ``lamb_apply`` writes the
weights; the sharded step all-reduces the ``2S`` sums in a collective of its own after the
moments -- they depend on the clip coefficient, which depends on the first reduction.

``Lion`` (``build_optimizer("lion")``) sits at the other end: one moment, the sign of an interpolated
momentum, no step count and no norm -- one ``lion_step`` launch per range and no stage of its own in
``_FlatStep``; see the class (its NaN behaviour is documented there, beside LAMB's).

``ema_decay`` (default None = off; every optimizer, ``build_optimizer(ema_decay=, ema_warmup=)``) keeps an
exponential moving average of the weights for evaluation: ``_ls()["ema"]``, a flat fp32 buffer shaped
like the master (loose tensors: ``state[p]["ema"]``), created by the first eager step as a copy of the
master BEFORE that step's update and, once per non-skipped step after the weight update, moved by
``e += a_t * (w - e)`` with ``a_t = 1 - d`` or, with ``ema_warmup`` (default), ``max(1 - d, 9 / (10 + c))``
after ``c`` updates.  ``c``, ``d`` and ``a_t`` live in a small device header (``ema_hdr``; the host
writes ``d`` and the warm-up flag like the lr, so a captured step follows ``sync_hyperparams()``), and
the pass rides on ``_FlatStep`` (``ema_begin`` in ``finalize``, ``ema_update`` behind every ``update``),
so the eager, sharded, range and graphed steps average alike and need no extra collective; a step the
non-finite guard skips changes neither ``e`` nor ``c``.  The average is saved by ``state_dict()`` (with
``ema_updates``) and all-gathered by ``gather_master(optimizer)`` with the moments.
``ema_weights()`` swaps it in for evaluation; ``ema_stats()`` reports the count and the last ``a_t``.
Buffers (BatchNorm running statistics) are not averaged -- evaluation under the averaged weights uses
the live ones -- and the end-of-epoch aggregation leaves ``e`` alone: each replica's average follows
its own master, the jump at an aggregation included.  A graph captured with the EMA off never
averages until it is captured again; one captured with it on keeps averaging (with the last decay
written) after ``ema_decay`` is set to None.  Padding and alignment gaps are averaged like everything
else: zero in the master, they stay zero.

``lr_schedule`` (default None = off; every optimizer, ``build_optimizer(lr_schedule=)``) is a per-step
schedule: a plain dict ``{"kind": "constant" | "linear" | "poly" | "cosine", "total_steps": T,
"warmup_steps": W = 0, "warmup_start": ws = 0, "min_ratio": m = 0, "power": q = 2}``, checked at
construction and the same in every param group.  With ``t`` non-skipped steps done and ``u = t + 1``
the step about to run uses ``param_groups[0]["lr"] * s(u)`` -- ``StepLR`` or the user still move the
base, and the two multiply: ``s = ws + (1 - ws) * u / W`` while ``u <= W`` (the last warm-up step runs
at exactly the base); after it, with ``p = min(1, (u - W) / (T - W))``, ``constant``: 1, ``poly``:
``m + (1 - m) * (1 - p)^q`` (``linear``: q = 1), ``cosine``: ``m + (1 - m) * (1 + cos(pi p)) / 2``; beyond
the horizon ``m``.  On the flat GPU path the constants, the base, ``t`` and the last factor live in a
small device header (``sched_hdr``; the host writes constants and base only when one changed) and
``lr_sched``, a one-thread launch in ``_FlatStep.finalize`` behind the norms and before any update,
writes this step's rate into ``hp[0]``: the eager, range, sharded and graphed steps schedule in the
stream and graph link of their updates, a replay needs no host write, and a step the non-finite guard
skips is not counted -- the next one runs at the rate the skipped one would have had.  Sharded
per-step data parallelism needs no collective: every rank sees the same skip flag and computes the same
``t`` (the ranks must be given the same dict: the CLI agrees its default horizon across them); under the weighted mix or gossip each rank counts its own non-skipped steps.  On the CPU, for
loose tensors and with several param groups (each group's own rate times the one factor) the same
math runs on the host in Python floats.  ``state_dict()`` saves ``sched_steps`` (a checkpoint without
it starts at 0), ``lr_schedule_stats()`` reports count, factor and rate.  The count is an fp32 device
scalar (exact to 2**24; longer horizons are refused).  A graph captured with the schedule off never
schedules until it is captured again; one captured with it on keeps its ``lr_sched`` (with the last
constants written, still following the base) after ``lr_schedule`` is set to None.

``prox_mu`` (default None = off, as is 0; SGD, Adam, AdamW and Lion, ``build_optimizer(prox_mu=)``) is FedProx
(Li et al., MLSys 2020): each rank minimises ``F_k(w) + mu / 2 * |w - a|^2`` with the anchor ``a`` the
weights its round started from, so ``mu * (p0 - a)`` -- ``p0`` the weight as loaded, before any decoupled
decay -- is added to the reduced, scaled and clipped gradient where weight decay is added (behind it):
SGD ``g += wd p0; g += mu (p0 - a)``, then the momentum chain; Adam the same before both moments; AdamW
and Lion add it to ``g`` and keep their decay decoupled.  The anchor is ``_ls()["prox_anchor"]``, a flat
fp32 buffer shaped like the master (loose tensors: ``state[p]["prox_anchor"]``); ``set_prox_anchor()``
copies the master into it in place (``train_global`` does at the start of every global epoch, behind the
aggregation), and without a call the first eager step with ``prox_mu > 0`` anchors at the master before
its update.  ``mu`` lives in a small device header (``prox_hdr``) the host writes like the lr, and the
anchor is one more streamed operand of the fused update (``sgd_step`` / ``adam_step`` / ``lion_step``
``prox=``, 4 B per element), cut by the same range as the master: the eager, range, sharded and graphed
steps all apply the term, a captured step follows ``sync_hyperparams()`` and ``set_prox_anchor()`` (a
device copy into the same address, outside the graph), and no collective is added.  Clipping: the global
norm is taken of the loss gradient alone -- the term is a regulariser the optimizer adds, treated
exactly as L2 weight decay is, so the norm, the coefficient and the non-finite guard do not see it, and
a skipped step changes no master, moment, shadow or anchor.  This departs from "penalty in the loss +
``clip_grad_norm_``", where the penalty's gradient is clipped with the rest.  LARS and LAMB refuse
``prox_mu > 0`` (their ratios are defined on ``g + wd w``; there is no agreed form with a proximal term).
Neither anchor nor header is saved (``state_dict()`` keys are unchanged): checkpoints are written at the
end of a global epoch, behind the aggregation, and the next one re-anchors.  ``prox_stats()`` reports
``mu`` and ``|w - a|_2``.  A graph captured with ``prox_mu`` off never applies the term until it is
captured again; one captured with it on runs with ``mu = 0`` after ``prox_mu`` is set to None or 0; a
capture with ``prox_mu > 0`` and no anchor yet asks for an eager step first.
"""
from __future__ import annotations

import contextlib
import math
import numbers

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
_TRANSIENT = ("hp", "clip", "clip_scratch", "clip_local", "lars", "lamb", "ema_hdr", "sched_hdr", "sched_written",
              "sched_last", "prox_anchor", "prox_hdr")
# the FedProx header: [mu, -, -, -]
_PROX_MU, _PROX_LEN = 0, 4
# slots of the weight EMA's header (csrc/include/ldnn_kernels.h EmaSlot)
_EMA_DECAY, _EMA_WARMUP, _EMA_UPDATES, _EMA_ALPHA, _EMA_LEN = 0, 1, 2, 3, 4
# slots of the learning-rate schedule's header (csrc/include/ldnn_kernels.h SchedSlot): the first six
# are ``_sched_consts``' tuple
_SCHED_BASE, _SCHED_STEPS, _SCHED_FACTOR, _SCHED_LEN = 6, 7, 8, 9
_SCHED_KINDS = {"constant": 0, "poly": 1, "linear": 1, "cosine": 2}
_SCHED_KEYS = ("kind", "total_steps", "warmup_steps", "warmup_start", "min_ratio", "power")
# LARS ratio table: one slot per uint16 map value, so every map entry is in bounds; the slots
# past the segments are never written and hold 1 (alignment gaps map to the last one)
_LARS_SLOTS, _LARS_GAP = 65536, 65535
_CAPTURE_MSG = "run an eager optimizer step before capturing it into a graph"
# lengths of the fp32 device vectors of _ls() (clip_scratch: as many slots as the ranges need)
_STATE_LEN = {"hp": 2, "clip": _CLIP_LEN, "clip_local": 1, "ema_hdr": _EMA_LEN, "sched_hdr": _SCHED_LEN,
              "prox_hdr": _PROX_LEN}


def _graph_state(store: dict, key, capturing: bool, make):
    """(Re)build ``store[key]``, device state that an eager step allocates and a captured graph
    reads -- which a capture must not do: it asks for an eager step first."""
    if capturing:
        raise RuntimeError(_CAPTURE_MSG)
    store[key] = v = make()
    return v


def _cut(sl, *ts):
    """``t[sl]`` of every tensor (None stays None); ``sl`` None: the whole buffers, no views to build."""
    return ts if sl is None else tuple(t[sl] if t is not None else None for t in ts)


def _aligned64(who, what, ranges):
    for lo, hi in ranges:
        if lo % 64 or hi % 64 or lo < 0 or hi < lo:
            raise ValueError(f"{who}: the {what} range [{lo}, {hi}) is not 64-element aligned")


def chunk_table(bounds, ranges, chunk, counted=None):
    """The seg_sumsq / lamb_moments tables (host lists) for segments ``bounds`` = [(begin, end)]
    restricted to the flat ``ranges``: ``chunks`` rows (segment, begin / 64, end / 64, counted) of at
    most ``chunk`` elements, never across a segment boundary, a segment's chunks consecutive; ``segs``
    rows (first chunk, end chunk) per segment.  Everything must lie on 64-element boundaries.
    ``counted`` (LAMB; None: LARS's table, fourth field 0): flat ranges whose sums enter this rank's
    norms -- the chunks are cut at their edges so each lies wholly in (fourth field 1, a segment's
    first chunks) or out."""
    who = "LARS" if counted is None else "LAMB"
    _aligned64(who, "counted", counted or ())
    _aligned64(who, "flat", list(ranges) + list(bounds))
    if chunk <= 0 or chunk % 64:
        raise ValueError(f"{who}: chunk {chunk} must be a positive multiple of 64")
    cs = sorted((lo, hi) for lo, hi in counted or () if hi > lo)
    pieces = []          # ``ranges`` cut into (lo, hi, counted) runs
    for lo, hi in sorted((lo, hi) for lo, hi in ranges if hi > lo):
        x = lo
        for a, b in cs:
            a, b = max(a, x), min(b, hi)
            if b <= a:
                continue
            if a > x:
                pieces.append((x, a, 0))
            pieces.append((a, b, 1))
            x = b
        if x < hi:
            pieces.append((x, hi, 0))
    chunks, segs = [], []
    for s, (b, e) in enumerate(bounds):
        first = len(chunks)
        for flag in (1, 0):
            for lo, hi in sorted((lo, hi) for lo, hi, c in pieces if c == flag):
                x, y = max(b, lo), min(e, hi)
                while x < y:
                    z = min(x + chunk, y)
                    chunks.append((s, x // 64, z // 64, flag))
                    x = z
        segs.append((first, len(chunks)))
    return chunks, segs


def lars_chunk_table(bounds, ranges, chunk):
    """``chunk_table`` for seg_sumsq."""
    return chunk_table(bounds, ranges, chunk)


def lamb_chunk_table(bounds, ranges, counted, chunk):
    """``chunk_table`` for lamb_moments."""
    return chunk_table(bounds, ranges, chunk, counted)


class _Lars:
    """Device state of the per-tensor trust ratios over one flat buffer (or, ``flat`` None, over
    loose tensors): segment map, ratio table, norm vectors, chunk tables per set of ranges, and
    ``local``, the [2S] sums a sharded step all-reduces (LARS: with clipping's scalar behind them)."""
    who, local_extra = "LARS", 1

    def __init__(self, flat, params, exclude_1d, device):
        self.flat, self.device, self.exclude_1d = flat, device, exclude_1d
        if flat is not None:
            segs = flat.segments
            self.names = [s.name for s in segs]
            self.adapt = [not (exclude_1d and s.param.dim() < 2) for s in segs]
            self.bounds = [(s.offset, s.offset + (s.storage_numel + 63) // 64 * 64) for s in segs]
            self.offsets = [b for b, _ in self.bounds]
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
        self.local = torch.zeros(2 * S + self.local_extra, dtype=torch.float32, device=device)
        self.tables = {}

    def table(self, ranges, capturing, counted=None):
        """Device chunk tables + partial slots of seg_sumsq (``counted``: of lamb_moments) over
        ``ranges``, built once per set."""
        def make():
            chunks, segs = chunk_table(self.bounds, ranges, _ext.C().seg_sumsq_chunk(), counted)
            segtab = [(a, b, int(ad), 0) for (a, b), ad in zip(segs, self.adapt)]
            i32 = dict(dtype=torch.int32, device=self.device)
            return dict(ranges=[tuple(r) for r in ranges], chunks=torch.tensor(chunks, **i32).reshape(-1, 4),
                        segtab=torch.tensor(segtab, **i32).reshape(-1, 4),
                        partials=torch.zeros(2 * len(chunks), dtype=torch.float32, device=self.device))
        key = tuple(ranges) if counted is None else (tuple(ranges), tuple(counted))
        return self.tables.get(key) or _graph_state(self.tables, key, capturing, make)

    def elem_ratio(self, lo, hi):
        """The ratio of every element of the flat range [lo, hi) (torch paths)."""
        return self.ratio[self.seg_of[lo // 64: hi // 64]].repeat_interleave(64)

    def sums_torch(self, bufs, ranges):
        """seg_sumsq in torch ops: [2][S] fp64 sums of squares of the two flat ``bufs`` over ``ranges``."""
        _aligned64(self.who, "flat", ranges)
        out = torch.zeros(2, self.S + 1, dtype=torch.float64, device=self.device)
        for lo, hi in ranges:
            if hi <= lo:
                continue
            idx = self.seg_of[lo // 64: hi // 64].clamp(max=self.S)
            for k, buf in enumerate(bufs):
                out[k].index_add_(0, idx, buf[lo:hi].double().square().view(-1, 64).sum(1))
        return out[:, :self.S]

    def _set_ratios(self, sums, wn, gn, r):
        over = torch.isinf(sums.float()).any(0)      # (a sum of squares beyond fp32: ratio 0)
        r = torch.where(over, torch.zeros_like(r), r)
        r = torch.where(self.adapt_t & (wn > 0) & (gn > 0), r, torch.ones_like(r))
        self.ratio[:self.S] = r.float()
        self.w_norm.copy_(wn)
        self.g_norm.copy_(gn)

    def finalize_torch(self, sums, gscale, wd):
        """lars_finalize in torch ops; ``gscale`` = grad_scale (* the clip coefficient)."""
        trust, eps = self.hdr.double()
        wn = sums[0].double().sqrt()
        gn = sums[1].double().sqrt() * gscale
        self._set_ratios(sums, wn, gn, trust * wn / (gn + wd * wn + eps))


class _Lamb(_Lars):
    """LAMB's: ``g_norm`` holds |u|, the tables are keyed by (moments ranges, counted ranges), ``local``
    is the [2S] sums alone.  ``u``: the torch paths' Adam direction between moments and update."""
    who, local_extra, u = "LAMB", 0, None

    def finalize_torch(self, sums):
        """lamb_finalize in torch ops."""
        wn, un = sums[0].double().sqrt(), sums[1].double().sqrt()
        self._set_ratios(sums, wn, un, wn / un)


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


def _ema_begin_torch(hdr, skip=False):
    """ema_begin's math in torch ops (fp32, no host read): this step's a_t, and the count."""
    if skip:
        hdr[_EMA_ALPHA] = 0.0
        return
    a = 1.0 - hdr[_EMA_DECAY]
    a = torch.where(hdr[_EMA_WARMUP] != 0, torch.maximum(a, 9.0 / (10.0 + hdr[_EMA_UPDATES])), a)
    hdr[_EMA_ALPHA] = a
    hdr[_EMA_UPDATES] += 1


def _ema_update_torch(e, w, hdr):
    """ema_update in torch ops: e += a_t * (w - e)."""
    e.add_((w - e).mul_(hdr[_EMA_ALPHA].to(e.device)))


def check_prox_mu(mu):
    """``prox_mu`` as the optimizers take it: None (off) or a finite real number >= 0 (0: off too);
    anything else is a ValueError.  Returns None when off, else the float."""
    if mu is None:
        return None
    if isinstance(mu, bool) or not isinstance(mu, numbers.Real) or not 0.0 <= float(mu) < float("inf"):
        raise ValueError(f"prox_mu must be None (off) or a finite number >= 0; got {mu!r}")
    return float(mu) or None


def _whole(what, v):
    """``v`` as an int when it is a whole, finite number (no bool, no string); else a ValueError."""
    if isinstance(v, bool) or not isinstance(v, numbers.Real) or v != v or v in (float("inf"), -float("inf")) \
            or v != int(v):
        raise ValueError(f"lr_schedule: {what} must be a whole number; got {v!r}")
    return int(v)


def _real(what, v):
    if isinstance(v, bool) or not isinstance(v, numbers.Real):
        raise ValueError(f"lr_schedule: {what} must be a number; got {v!r}")
    return float(v)


def _sched_consts(sched):
    """Validate an ``lr_schedule`` dict (every refusal is a ValueError); returns the header constants
    ``(kind code, W, ws, T, m, q)`` (``linear``: poly with q = 1; ``constant`` needs no horizon)."""
    if not isinstance(sched, dict):
        raise ValueError(f"lr_schedule must be None (off) or a dict with the keys {_SCHED_KEYS}; got {sched!r}")
    bad = set(sched) - set(_SCHED_KEYS)
    if bad:
        raise ValueError(f"lr_schedule: unknown keys {sorted(bad, key=str)} (known: {_SCHED_KEYS})")
    kind = sched.get("kind")
    if not isinstance(kind, str) or kind not in _SCHED_KINDS:
        raise ValueError(f"lr_schedule: kind must be one of {sorted(_SCHED_KINDS)}; got {kind!r}")

    def get(key, default):
        return default if sched.get(key) is None else sched[key]

    W = _whole("warmup_steps", get("warmup_steps", 0))
    ws, m = _real("warmup_start", get("warmup_start", 0.0)), _real("min_ratio", get("min_ratio", 0.0))
    q = 1.0 if kind == "linear" else _real("power", get("power", 2.0))
    if W < 0:
        raise ValueError(f"lr_schedule: warmup_steps must be a whole number >= 0; got {W}")
    T = get("total_steps", W + 1 if kind == "constant" else None)
    if T is None:
        raise ValueError(f"lr_schedule: {kind!r} needs total_steps (> warmup_steps = {W})")
    T = _whole("total_steps", T)
    if T <= W:
        raise ValueError(f"lr_schedule: total_steps must be a whole number > warmup_steps ({W}); got {T}")
    if not 0.0 <= ws <= 1.0 or not 0.0 <= m <= 1.0:
        raise ValueError(f"lr_schedule: warmup_start and min_ratio must lie in [0, 1]; got {ws}, {m}")
    if not q > 0 or q == float("inf"):
        raise ValueError(f"lr_schedule: power must be positive and finite; got {q}")
    if T >= 2 ** 24:
        raise ValueError(f"lr_schedule: total_steps {T} exceeds the fp32 step count (2**24)")
    return float(_SCHED_KINDS[kind]), float(W), ws, float(T), m, q


def check_lr_schedule(sched):
    """Validate an ``lr_schedule`` value the way the optimizers' constructors do (ValueError on any
    refusal); returns None for None, else a plain copy of the dict."""
    if sched is None:
        return None
    _sched_consts(sched)
    return dict(sched)


def lr_schedule_factor(sched, u):
    """The schedule's factor ``s(u)`` of step ``u`` = 1, 2, ... in Python floats (what the CPU and
    loose-tensor paths use; ``lr_sched`` is the same expression in fp32).  ``sched``: an
    ``lr_schedule`` dict, or ``_sched_consts``' tuple."""
    kind, W, ws, T, m, q = sched if isinstance(sched, tuple) else _sched_consts(sched)
    if u <= W:
        return ws + (1.0 - ws) * (u / W)
    if kind == 0:
        return 1.0
    p = min(1.0, (u - W) / (T - W))
    return m + (1.0 - m) * ((1.0 - p) ** q if kind == 1 else 0.5 * (1.0 + math.cos(math.pi * p)))


class _FlatStep:
    """ONE optimizer step of one flat buffer ``f``, as the stages every driver runs in this order:

        norm(ranges) -> [all-reduce ``local``] -> finalize(reduced)
            -> moments(update_ranges, counted_ranges) -> [all-reduce ``local2``] -> ratios(reduced)
            -> update(lo, hi) ... -> end()

    The second line exists only for LAMB (``M``): its trust ratios need the norm of the Adam
    direction, which needs this step's moments, which need the clip coefficient of the first
    reduction.  ``moments`` runs over every range this rank updates and counts the sums of those
    inside ``counted_ranges``; ``local2`` (sharded only) is the [2S] vector of per-segment
    [master, direction] sums.

    ``local``: the fp32 vector that must be all-reduced between ``norm`` and ``finalize`` -- None
    unless the buffer is sharded and clipping or LARS is on.  With clipping alone it is the
    1-element sum of squares; with LARS the per-segment [master, grad] sums ``[2S]`` with
    clipping's scalar behind them.  Building the step allocates (an eager step) or looks up (a
    capture) every piece of device state and, when not capturing, writes the hyper-parameters.

    Skipping (a non-finite norm): the native kernels read the flag on the device, so every
    launch is issued and the host step count advances (Adam's device count does not); on the
    torch paths ``skip`` is a host bool after ``finalize`` and nothing changes.

    ``clip``: ``(state, skip)`` of a norm taken outside (several groups / loose tensors).

    The weight EMA (``ema``: the flat average, ``ema_hdr`` its header) rides on two of the stages, so
    every driver averages in the stream and graph link of its updates: ``finalize`` issues
    ``ema_begin`` (this step's a_t and the count; a skipped step gets a_t = 0) and ``update(lo, hi)``
    issues ``ema_update`` on the same range right behind the optimizer's launch.

    The learning-rate schedule rides on ``finalize`` too, behind the norms (the skip flag is known)
    and before the optimizer's prologue and any ``update``: natively ``lr_sched`` turns the header
    ``sched_hdr`` into this step's ``hp[0]``; on the torch paths ``lr`` (what ``_update_torch`` uses)
    becomes ``group["lr"] * s`` in Python floats.  ``sched``: the factor of a schedule stepped
    outside (several groups / loose tensors), already in ``lr``.

    FedProx (``prox``: ``(anchor, header)``; ``prox_mu``: the host's value for the torch paths) adds no
    stage: ``update(lo, hi)`` hands the optimizer's launch the anchor cut like the master.

    The stages hand their results on in the object, so the order is a precondition: when the
    step takes a norm (``normed``: its own clipping, or LARS), ``norm`` comes before ``finalize``;
    ``finalize`` comes before any ``update``.  With neither, ``norm`` may be left out."""

    # what a plain step (no clipping, no LARS) never sets
    own_clip = normed = False
    cl = skip = L = M = hp = local = local2 = tab = mtab = sumsq = ctx = ema = ema_hdr = None
    sched_hdr = sched_host = prox = prox_mu = None
    ranges, counted, nparts = (), (), 0

    def __init__(self, opt, f, group, clip=None, sharded=False, sched=None):
        self.opt, self.f, self.group = opt, f, group
        self.lr = group["lr"] if sched is None else group["lr"] * sched
        opt._refuse_inside_ema("an optimizer step")
        self.st = st = opt._ls()
        self.native = native = _ext.use_native(f.master)
        dev = f.master.device
        thr, lars, lamb = opt._clip_threshold(), opt._lars_conf(), opt._lamb_conf()
        if clip is not None or thr is not None or lars is not None:
            self._norm_state(clip, thr, lars, dev, sharded)
        if lamb is not None:
            self.M = opt._trust_state("lamb", lamb, f)
            self.local2 = self.M.local if sharded else None
        if opt._ema_conf() is not None:
            self.ema, self.ema_hdr = opt._ema_state(f)
        self.prox_mu = opt._prox_conf()
        if self.prox_mu is not None:
            self.prox = opt._prox_state(f)
        if native:
            hp = st.get("hp")
            self.hp = hp if hp is not None and hp.device == dev else opt._state("hp", dev)
        if sched is None:
            conf = opt._sched_conf()
            if conf is not None and native:
                self.sched_hdr = opt._state("sched_hdr", dev)
            else:
                self.sched_host = conf
        if not opt._ldnn_capturing:
            # inside a hipGraph capture the writes are NOT recorded: the graph reads the tensors,
            # and GraphedStep refreshes them (sync_hyperparams) whenever a value changes
            opt._write_hyperparams(self.lr, (thr, lars))

    def _norm_state(self, clip, thr, lars, dev, sharded):
        opt = self.opt
        if clip is not None:
            self.cl, self.skip = (clip[0].to(dev), None) if self.native else clip
        elif thr is not None:
            self.own_clip, self.cl = True, opt._state("clip", dev)
        if lars is not None:
            self.L = opt._trust_state("lars", lars[2], self.f)
        self.normed = self.own_clip or self.L is not None
        if sharded and self.normed:
            self.local = self.L.local if self.L is not None else opt._state("clip_local", dev)

    def prox_arg(self, sl):
        """``prox=`` of a native update over the flat slice ``sl``: the anchor cut like the master."""
        return None if self.prox is None else (_cut(sl, self.prox[0])[0], self.prox[1])

    def prox_term(self, sl, p):
        """The torch paths' ``mu * (p0 - a)`` over the flat slice ``sl`` (None when off); ``p``: the
        master's slice, before the update touches it."""
        return None if self.prox is None else (p - _cut(sl, self.prox[0])[0]).mul_(self.prox_mu)

    def _seg_sums(self):
        L, f = self.L, self.f
        self.tab = t = L.table(self.ranges, self.opt._ldnn_capturing)
        _ext.C().seg_sumsq(f.master, f.grad, t["chunks"], t["partials"], t["ranges"], L.offsets)

    def norm(self, ranges):
        """The sums of squares over ``ranges`` (of a sharded buffer: this rank's shard ranges, on
        rank 0 also the replicated tail, which every rank holds alike and one rank counts):
        clipping's per-workgroup partials, one range after the other in the scratch slots, and --
        where they have to travel (``local``) -- their total and LARS's per-segment sums."""
        if not self.normed:
            return
        f, L, local = self.f, self.L, self.local
        self.ranges = ranges = [(lo, hi) for lo, hi in ranges if hi > lo]
        if self.native:
            C = _ext.C()
            if self.own_clip:
                sc = self.opt._state("clip_scratch", f.master.device,
                                     max(1, sum(C.grad_sumsq_parts(hi - lo) for lo, hi in ranges)))
                self.nparts = 0
                for lo, hi in ranges:
                    g = f.grad if lo == 0 and hi == f.numel else f.grad[lo:hi]    # (the whole buffer: no view to build)
                    self.nparts += C.grad_sumsq(g, sc, self.nparts)
                if local is not None:
                    C.sumsq_total(sc, self.nparts, local[-1:])
            if L is not None and local is not None:
                self._seg_sums()
                C.lars_finalize(self.tab["partials"], self.tab["segtab"], L.hdr, L.ratio, L.w_norm, L.g_norm, 1.0, 0.0,
                                sums_out=local)
            return
        if self.own_clip:
            scale = f.grad_scale if local is None else 1.0    # (a reduced sum is scaled when finalized)
            self.sumsq = torch.zeros((), dtype=torch.float64, device=f.master.device)
            for lo, hi in ranges:
                self.sumsq = self.sumsq + (f.grad[lo:hi].double() * scale).square().sum()
            if local is not None:
                local[-1:].copy_(self.sumsq.reshape(1))
        if L is not None and local is not None:
            local[:2 * L.S].copy_(L.sums_torch((f.master, f.grad), ranges).t().reshape(-1))

    def finalize(self, reduced: bool):
        """The clip state, then the LARS ratios (which use the clip coefficient), then the
        optimizer's per-step prologue.  ``reduced``: the sums come from the all-reduced ``local``;
        else straight from ``norm``'s partials (LARS's are taken here: nothing waited for them)."""
        if self.normed:
            self._finalize_norms(reduced)
        if self.sched_hdr is not None:
            _ext.C().lr_sched(self.sched_hdr, self.hp, clip=self.cl)
        elif self.sched_host is not None:
            self.lr = self.group["lr"] * self.opt._host_sched(self.sched_host, self.group["lr"], bool(self.skip))
        if not self.skip:
            self.ctx = self.opt._begin_ranges(self)
        if self.ema is not None:
            if self.native:
                _ext.C().ema_begin(self.ema_hdr, clip=self.cl)
            else:
                _ema_begin_torch(self.ema_hdr, self.skip)

    def _finalize_norms(self, reduced):
        f, L, cl, local = self.f, self.L, self.cl, self.local
        gs, wd = f.grad_scale, self.group["weight_decay"]
        if self.native:
            C = _ext.C()
            if self.own_clip:
                sc = self.st["clip_scratch"]
                if reduced:
                    C.clip_finalize(sc, 0, cl, gs, ext=local[-1:])
                else:
                    C.clip_finalize(sc, self.nparts, cl, gs)
            if L is not None:
                if reduced:
                    C.lars_finalize(None, self.tab["segtab"], L.hdr, L.ratio, L.w_norm, L.g_norm, gs, wd,
                                    ext=local, clip=cl)
                else:
                    self._seg_sums()
                    C.lars_finalize(self.tab["partials"], self.tab["segtab"], L.hdr, L.ratio, L.w_norm, L.g_norm, gs,
                                    wd, clip=cl)
        else:
            if self.own_clip:
                if reduced:
                    _clip_finalize_torch(cl, local[-1:], gs)
                else:
                    _clip_finalize_torch(cl, self.sumsq)
                self.skip = bool(cl[_CLIP_SKIP].item())
            if self.skip:
                return
            if L is not None:
                sums = local[:2 * L.S].view(L.S, 2).t() if reduced else L.sums_torch((f.master, f.grad), self.ranges)
                L.finalize_torch(sums, gs * (cl[_CLIP_COEF].double() if cl is not None else 1.0), wd)

    def moments(self, ranges, counted):
        """LAMB: the moment update over ``ranges`` and the per-segment sums of squares of master
        and direction over ``counted`` (a subset of ``ranges``); sharded, the sums go to ``local2``."""
        M, f = self.M, self.f
        if M is None or self.skip:
            return
        ranges = [(lo, hi) for lo, hi in ranges if hi > lo]
        counted = [(lo, hi) for lo, hi in counted if hi > lo]
        if self.native:
            C = _ext.C()
            self.mtab = t = M.table(ranges, self.opt._ldnn_capturing, counted)
            g = self.group
            C.lamb_moments(f.master, f.grad, self.ctx[0], self.ctx[1], t["chunks"], t["partials"], self.hp, f.grad_scale,
                           *g["betas"], g["eps"], g["weight_decay"], t["ranges"], M.offsets, clip=self.cl)
            if self.local2 is not None:
                C.lamb_finalize(t["partials"], t["segtab"], M.ratio, M.w_norm, M.g_norm, sums_out=self.local2)
            return
        if M.u is None or M.u.shape != f.master.shape or M.u.device != f.master.device:
            M.u = torch.zeros_like(f.master)
        coef = self.cl[_CLIP_COEF] if self.cl is not None else 1.0
        for lo, hi in ranges:
            M.u[lo:hi] = self.opt._moments_torch(self, f.master[lo:hi], f.grad[lo:hi] * f.grad_scale * coef,
                                                 self.ctx[0][lo:hi], self.ctx[1][lo:hi])
        self.counted = counted
        if self.local2 is not None:
            self.local2.copy_(M.sums_torch((f.master, M.u), counted).t().reshape(-1))

    def ratios(self, reduced: bool):
        """LAMB: the trust ratios from the all-reduced ``local2`` or from ``moments``' own sums."""
        M = self.M
        if M is None or self.skip:
            return
        if self.native:
            t = self.mtab
            if reduced:
                _ext.C().lamb_finalize(None, t["segtab"], M.ratio, M.w_norm, M.g_norm, ext=self.local2, clip=self.cl)
            else:
                _ext.C().lamb_finalize(t["partials"], t["segtab"], M.ratio, M.w_norm, M.g_norm, clip=self.cl)
            return
        M.finalize_torch(self.local2.view(M.S, 2).t() if reduced
                         else M.sums_torch((self.f.master, M.u), self.counted))

    def update(self, lo: int, hi: int, zero=()):
        """Update flat elements [lo, hi): one fused launch (which also zeroes the flat gradient
        ranges ``zero``), or the same math in torch ops."""
        if hi <= lo:
            return
        f, L = self.f, self.L
        sl = None if lo == 0 and hi == f.numel else slice(lo, hi)    # (None: the whole buffer, no views to build)
        if self.native:
            if (L is not None or self.M is not None) and (lo % 64 or hi % 64):
                raise ValueError(f"{'LARS' if L is not None else 'LAMB'}: the update range [{lo}, {hi}) is not "
                                 "64-element aligned")
            self.opt._update_native(self, sl, zero if lo == 0 else [(a - lo, b - lo) for a, b in zero])
            if self.ema is not None:
                _ext.C().ema_update(*_cut(sl, f.master, self.ema), self.ema_hdr)
            return
        if not self.skip:
            p, g, shadow = _cut(sl, f.master, f.grad, f.shadow)
            g = g * f.grad_scale
            if self.cl is not None:
                g = g * self.cl[_CLIP_COEF]
            L = L if L is not None else self.M
            self.opt._update_torch(self, sl, p, g, L.elem_ratio(lo, hi) if L is not None else None)
            if shadow is not None:
                shadow.copy_(p)
            if self.ema is not None:
                _ema_update_torch(_cut(sl, self.ema)[0], p, self.ema_hdr)
        for a, b in zero:
            f.grad[a:b].zero_()

    def end(self):
        if not self.skip:
            st = self.st
            st["step"] = st.get("step", 0) + 1


class _RangeStep(_FlatStep):
    """``range_updater``'s form: driven from outside ``step()``, and its ranges must cover the buffer."""
    done = 0

    @torch.no_grad()
    def update(self, lo: int, hi: int, zero=()):
        self.done += max(hi - lo, 0)
        super().update(lo, hi, zero)

    def end(self):
        if self.done != self.f.numel:
            raise RuntimeError(f"range updates covered {self.done} of {self.f.numel} flat elements")
        super().end()


class _FlatOptimizer(torch.optim.Optimizer):
    def __init__(self, params, defaults):
        super().__init__(params, defaults)
        self._sched_conf()    # (a schedule given per param group: checked, and the same in all)
        self._prox_conf()     # (prox_mu likewise)

    def _ls(self) -> dict:
        """Fused (flat-buffer) optimizer state: momentum / moments / step / hp (+ the
        clipping state and scratch)."""
        return self.__dict__.setdefault("_ldnn_state", {})

    def state_dict(self):
        sd = super().state_dict()
        ls = self._ls()
        flat = {k: v for k, v in ls.items() if k not in _TRANSIENT}
        if self._bumps_step and self._clip_threshold() is not None and "hp" in ls and "exp_avg" in ls:
            # the fused Adam's step count lives on the device: skipped steps did not advance it
            # (Adam / AdamW / Lamb; Lion never bumps hp[1], its count is the host's)
            flat["step"] = int(ls["hp"][1].item())
        if "ema_hdr" in ls:
            # ... and so does the EMA's update count (load_state_dict hands it to the next header)
            flat["ema_updates"] = int(ls["ema_hdr"][_EMA_UPDATES].item())
        if "sched_hdr" in ls:
            # ... and the schedule's count of non-skipped steps (the host paths keep it in ``ls``)
            flat["sched_steps"] = int(ls["sched_hdr"][_SCHED_STEPS].item())
        sd["ldnn_flat_state"] = flat
        if any("prox_anchor" in v for v in sd["state"].values()):
            # (loose tensors: the anchors are not saved either; the dicts are the live ones, so copy)
            sd["state"] = {k: {n: t for n, t in v.items() if n != "prox_anchor"} for k, v in sd["state"].items()}
        return sd

    # ---- device state an eager step allocates and a captured graph reads ---------------
    _ldnn_capturing = False    # set on the instance by GraphedStep / GraphedDPStep around their capture
    _bumps_step = False        # the optimizer's prologue issues bump_step: hp[1] counts the non-skipped steps

    def _state(self, key, device, n=None):
        """The fp32 device vector ``key`` of ``_ls()``, at least ``n`` long: ``hp`` [lr, Adam's
        step count], ``clip`` [max_norm, coef, skip, last_norm, steps, clipped, skipped, -],
        ``clip_scratch`` (grad_sumsq's partial slots), ``clip_local`` (the 1-element local sum),
        ``ema_hdr`` [decay, warm-up flag, EMA updates, last a_t], ``sched_hdr`` [kind, W, ws, T, m,
        q, base, steps, last factor], ``prox_hdr`` [mu, -, -, -]."""
        st = self._ls()
        t = st.get(key)
        n = n or _STATE_LEN[key]
        if t is None or t.device != device or t.numel() < n:
            t = _graph_state(st, key, self._ldnn_capturing, lambda: torch.zeros(n, dtype=torch.float32, device=device))
            if key == "hp":
                t[1] = float(st.get("step", 0))
            elif key == "ema_hdr":
                t[_EMA_UPDATES] = float(st.get("ema_updates", 0))
            elif key == "sched_hdr":
                t[_SCHED_STEPS] = float(st.get("sched_steps", 0))
        return t

    def _trust_state(self, key, excl, flat, params=None, device=None):
        """The LARS / LAMB (``key`` "lars" / "lamb") device state over ``flat`` (None: over the loose ``params``)."""
        st = self._ls()
        device = flat.master.device if flat is not None else device
        T = st.get(key)
        if T is None or T.flat is not flat or T.device != device or T.exclude_1d != excl or \
                (flat is None and T.S != len(params)):
            cls = _Lamb if key == "lamb" else _Lars
            T = _graph_state(st, key, self._ldnn_capturing, lambda: cls(flat, params, excl, device))
        return T

    def _lars_state(self, *args):
        return self._trust_state("lars", *args)

    def _lamb_state(self, *args):
        return self._trust_state("lamb", *args)

    def _trust_stats(self, key, excl, norm2):
        """``lars_stats`` / ``lamb_stats``: the state ``key`` (built when no step has run yet) as a dict."""
        T = self._ls().get(key)
        if T is None:
            f = self._flat_for_group(self.param_groups[0]) if len(self.param_groups) == 1 else None
            ps = [p for g in self.param_groups for p in g["params"]]
            T = self._trust_state(key, excl, f, ps, ps[0].device if ps else torch.device("cpu"))
            if key == "lars":
                self._write_hyperparams()
        return {"ratio": T.ratio[:T.S], "w_norm": T.w_norm, norm2: T.g_norm, "names": list(T.names),
                "adapted": list(T.adapt)}

    def _write_hyperparams(self, lr=None, conf=None):
        """Write the learning rate, the clipping threshold, LARS's trust coefficient and eps, the
        EMA's decay and warm-up flag and FedProx's mu into whichever of their device tensors exist; with a schedule's
        header the rate goes there as the base (``lr_sched`` writes ``hp[0]``).  ``conf``:
        ``(_clip_threshold(), _lars_conf())`` where the caller has them already."""
        st = self._ls()
        hp, cl, L, eh = st.get("hp"), st.get("clip"), st.get("lars"), st.get("ema_hdr")
        lr = self.param_groups[0]["lr"] if lr is None else lr
        sh = st.get("sched_hdr")
        sched = self._sched_conf() if sh is not None else None
        if sh is not None:
            # the schedule's constants and base rate: only the slots whose value changed (all of a new
            # header), so a scheduled step whose base stands issues no host write at all.  (Switched
            # off after a capture: the captured lr_sched keeps the last constants and follows the base.)
            last = st.get("sched_written")
            old = last[1] if last is not None and last[0] is sh else (None,) * (_SCHED_BASE + 1)
            vals = (sched if sched is not None else old[:_SCHED_BASE]) + (float(lr),)
            for i, (v, o) in enumerate(zip(vals, old)):
                if v != o and v is not None:
                    sh[i].fill_(v)
            st["sched_written"] = (sh, vals)
        if hp is not None and sched is None:
            hp[0].fill_(lr)
        if eh is not None:
            ema = self._ema_conf()
            if ema is not None:    # (switched off after a capture: the captured kernels keep the last decay)
                eh[_EMA_DECAY].fill_(ema[0])
                eh[_EMA_WARMUP].fill_(float(ema[1]))
        ph = st.get("prox_hdr")
        if ph is not None:
            # (switched off after a capture: the captured kernels run with mu = 0, the term vanishes)
            ph[_PROX_MU].fill_(self._prox_conf() or 0.0)
        if cl is None and L is None:
            return
        mx, lars = conf if conf is not None else (self._clip_threshold(), self._lars_conf())
        if cl is not None:
            # (clipping switched off after a graph was captured: an infinite threshold makes the
            # captured kernels' coefficient 1; the non-finite guard of that graph stays)
            cl[_CLIP_MAX].fill_(mx if mx is not None else float("inf"))
        if L is not None and lars is not None:
            L.hdr[0].fill_(lars[0])
            L.hdr[1].fill_(lars[1])

    @torch.no_grad()
    def sync_hyperparams(self):
        """Write the current learning rate (and clipping threshold, LARS trust coefficient and
        eps, EMA decay and warm-up flag, the schedule's constants and base rate, FedProx's mu) into the device
        hyper-parameter tensors."""
        self._write_hyperparams()

    def _buf(self, name, like):
        st = self._ls()
        b = st.get(name)
        if b is None or b.shape != like.shape or b.device != like.device:
            b = torch.zeros_like(like)
            st[name] = b
        return b

    # ---- global-norm gradient clipping ------------------------------------------------
    def _same_in_groups(self, read, what):
        """``read(group)``, which must be the same in every param group (None without groups)."""
        groups = self.param_groups
        if not groups:
            return None
        v = read(groups[0])
        for g in groups[1:]:
            if read(g) != v:
                raise ValueError(f"{what}; got {[read(g_) for g_ in groups]}")
        return v

    @staticmethod
    def _group_threshold(g):
        v = g.get("max_grad_norm")
        return None if v is None or float(v) <= 0 else float(v)

    def _clip_threshold(self):
        """The clipping threshold (None: off).  One threshold for the whole optimizer."""
        return self._same_in_groups(self._group_threshold,
                                    "max_grad_norm must be the same in every param group (the norm is global)")

    def grad_clip_stats(self):
        """Device scalars ``last_norm`` / ``steps`` / ``clipped`` / ``skipped`` of the clipped
        steps so far (reading one syncs), or None when clipping is off."""
        if self._clip_threshold() is None:
            return None
        cl = self._ls().get("clip")
        if cl is None:
            ps = self.param_groups[0]["params"]
            cl = self._state("clip", ps[0].device if ps else torch.device("cpu"))
            self._write_hyperparams()
        return {"last_norm": cl[_CLIP_NORM], "steps": cl[_CLIP_STEPS], "clipped": cl[_CLIP_CLIPPED],
                "skipped": cl[_CLIP_SKIPPED]}

    def _loose_clip(self, flats):
        """The clipped step of several groups, or of tensors outside a flat buffer: the global
        norm over EVERY group's gradient in torch ops, before any update.  Returns ``(state,
        skip)`` with the skip flag read on the host (a sync per step; such an optimizer cannot be
        captured), or None when no gradient exists."""
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
        cl = self._state("clip", dev)
        if not self._ldnn_capturing:
            self._write_hyperparams()
        _clip_finalize_torch(cl, total)
        return cl, bool(cl[_CLIP_SKIP].item())

    # ---- LARS: per-tensor trust ratios (SGD) -------------------------------------------
    @staticmethod
    def _group_lars(g):
        t = g.get("lars_trust")
        return None if t is None else (float(t), float(g.get("lars_eps", 1e-8)), bool(g.get("lars_exclude_1d", True)))

    def _lars_conf(self):
        """``(trust_coef, eps, exclude_1d)``, or None when LARS is off.  One setting for the whole
        optimizer; the keys are read with .get, so state saved before they existed loads."""
        if "lars_trust" not in self.defaults:    # (Adam / AdamW take no LARS settings)
            return None
        return self._same_in_groups(self._group_lars,
                                    "lars_trust / lars_eps / lars_exclude_1d must be the same in every param group")

    def lars_stats(self):
        """In segment (flat-buffer) order: the device tensors ``ratio`` / ``w_norm`` / ``g_norm`` of
        the last LARS step, the parameter ``names`` and which tensors are ``adapted`` (reading a
        tensor syncs); None when LARS is off."""
        lars = self._lars_conf()
        return None if lars is None else self._trust_stats("lars", lars[2], "g_norm")

    # ---- LAMB: per-tensor trust ratios (Lamb) -------------------------------------------
    def _lamb_conf(self):
        """``exclude_1d``, or None on every optimizer but Lamb."""
        if "lamb_exclude_1d" not in self.defaults:
            return None
        return self._same_in_groups(lambda g: bool(g.get("lamb_exclude_1d", True)),
                                    "lamb_exclude_1d must be the same in every param group")

    def lamb_stats(self):
        """In segment (flat-buffer) order: the device tensors ``ratio`` / ``w_norm`` / ``u_norm`` of
        the last LAMB step, the parameter ``names`` and which tensors are ``adapted`` (reading a
        tensor syncs); None on the other optimizers."""
        excl = self._lamb_conf()
        return None if excl is None else self._trust_stats("lamb", excl, "u_norm")

    # ---- EMA of the weights (evaluation weights) ----------------------------------------
    _ldnn_in_ema = False    # inside ema_weights(): the master holds the average

    @staticmethod
    def _check_ema_decay(d):
        if d is not None and not 0 < d < 1:
            raise ValueError(f"ema_decay must be None (off) or in (0, 1); got {d}")

    @staticmethod
    def _group_ema(g):
        d = g.get("ema_decay")
        return None if d is None else (float(d), bool(g.get("ema_warmup", True)))

    def _ema_conf(self):
        """``(decay, warmup)``, or None when the EMA is off.  One setting for the whole optimizer; the
        keys are read with .get, so state saved before they existed loads."""
        return self._same_in_groups(self._group_ema, "ema_decay / ema_warmup must be the same in every param group")

    def _ema_state(self, f):
        """``(ema, header)`` of the flat buffer ``f``; the average starts as a copy of the master (the
        first eager step calls this before its update)."""
        st = self._ls()
        e = st.get("ema")
        if e is None or e.shape != f.master.shape or e.device != f.master.device:
            e = _graph_state(st, "ema", self._ldnn_capturing, lambda: f.master.detach().clone())
        return e, self._state("ema_hdr", f.master.device)

    def _refuse_inside_ema(self, what):
        if self._ldnn_in_ema:
            raise RuntimeError(f"{what} inside ema_weights(): the parameters hold the average, not the live weights")

    def _ema_flat(self):
        """The one flat buffer the EMA covers (None: loose tensors); anything between is refused."""
        return self._one_flat("ema_decay")

    def _loose_ema_begin(self):
        """Loose tensors, before the step's updates: every parameter's average (created as a copy of
        it) and the header."""
        ps = [p for g in self.param_groups for p in g["params"]]
        for p in ps:
            if "ema" not in self.state.setdefault(p, {}):
                self.state[p]["ema"] = p.detach().clone()
        hdr = self._state("ema_hdr", ps[0].device if ps else torch.device("cpu"))
        self._write_hyperparams()
        return ps, hdr

    def ema_stats(self):
        """The device scalars ``updates`` (EMA updates so far) and ``a_last`` (the last step's a_t; 0
        after a skipped step) -- reading one syncs -- and ``decay``; None when the EMA is off."""
        conf = self._ema_conf()
        if conf is None:
            return None
        hdr = self._ls().get("ema_hdr")
        if hdr is None:
            ps = self.param_groups[0]["params"]
            hdr = self._state("ema_hdr", ps[0].device if ps else torch.device("cpu"))
            self._write_hyperparams()
        return {"updates": hdr[_EMA_UPDATES], "a_last": hdr[_EMA_ALPHA], "decay": conf[0]}

    @contextlib.contextmanager
    @torch.no_grad()
    def ema_weights(self):
        """Inside the context the parameters (fp32 master and bf16 shadow) hold the EMA and the EMA
        buffer holds the live weights -- an exact exchange, undone bit for bit on leaving.  Buffers
        (BatchNorm running statistics) are not averaged: evaluation uses the live ones.  No
        optimizer step, and no replay of a graph that holds one, may run inside.  Of a sharded
        buffer the average must be whole first: ``gather_master(optimizer)`` on every rank."""
        if self._ema_conf() is None:
            raise RuntimeError("ema_weights(): the EMA is off (ema_decay=None)")
        if self._ldnn_in_ema:
            raise RuntimeError("ema_weights() is already active: the context does not nest")
        f = self._ema_flat()
        if f is not None:
            e = self._ls().get("ema")
            pairs = None
            if e is not None and (e.shape != f.master.shape or e.device != f.master.device):
                e = None
            sh = getattr(f, "shard_sync", None)
            if e is not None and sh is not None and not sh.master_whole:
                raise RuntimeError("ema_weights(): this rank holds only its shards of the average; call "
                                   "gather_master(optimizer) on every rank first")
        else:
            pairs = [(p, self.state.get(p, {}).get("ema")) for g in self.param_groups for p in g["params"]]
            e = None if any(a is None for _, a in pairs) or not pairs else pairs
        if e is None:
            raise RuntimeError("ema_weights(): no optimizer step has run yet, there is no average")

        def swap():
            if pairs is not None:
                for p, _ in pairs:
                    st = self.state[p]
                    p.data, st["ema"] = st["ema"], p.data
            elif _ext.use_native(f.master):
                _ext.C().ema_swap(f.master, e, f.shadow)
                if f.shadow is not None:
                    torch.autograd.graph.increment_version(f.shadow)   # (as refresh_shadow does)
            else:
                tmp = f.master.clone()
                f.master.copy_(e)
                e.copy_(tmp)
                if f.shadow is not None:
                    f.shadow.copy_(f.master)

        swap()
        self._ldnn_in_ema = True
        try:
            yield
        finally:
            self._ldnn_in_ema = False
            swap()

    # ---- FedProx: the proximal term toward the round's start weights ----------------------
    _prox_ok = True    # (Lamb: False)

    def _prox_conf(self):
        """``mu`` > 0, or None when the term is off.  One value for the whole optimizer; the key is
        read with .get, so state saved before it existed loads.  LARS and LAMB refuse it."""
        mu = self._same_in_groups(lambda g: check_prox_mu(g.get("prox_mu")),
                                  "prox_mu must be the same in every param group")
        if mu is not None and (not self._prox_ok or self._lars_conf() is not None):
            raise ValueError("prox_mu: LARS and LAMB take no proximal term (their trust ratios are defined on "
                             "g + weight_decay * w; there is no agreed form with one)")
        return mu

    def _one_flat(self, what):
        """The one flat buffer ``what`` covers (None: loose tensors); anything between is refused."""
        flats = [self._flat_for_group(g) for g in self.param_groups]
        if all(f is None for f in flats):
            return None
        if len(flats) != 1:
            raise ValueError(f"{what} needs ONE param group holding one flat buffer, or loose tensors only")
        return flats[0]

    def _prox_state(self, f):
        """``(anchor, header)`` of the flat buffer ``f``; without a ``set_prox_anchor()`` before it the
        anchor starts as a copy of the master (the first eager step calls this before its update)."""
        st = self._ls()
        a = st.get("prox_anchor")
        if a is None or a.shape != f.master.shape or a.device != f.master.device:
            a = _graph_state(st, "prox_anchor", self._ldnn_capturing, lambda: f.master.detach().clone())
        return a, self._state("prox_hdr", f.master.device)

    def _loose_prox(self, p, mu):
        """Loose tensors: ``mu * (p - a)`` of the parameter ``p`` (None when off); the anchor is created
        as a copy of ``p`` by the first step that needs it."""
        if mu is None:
            return None
        ps = self.state.setdefault(p, {})
        if "prox_anchor" not in ps:
            ps["prox_anchor"] = p.detach().clone()
        return (p.data - ps["prox_anchor"]).mul_(mu)

    @torch.no_grad()
    def set_prox_anchor(self):
        """Anchor FedProx at the current weights: copy the master into the anchor, in place -- the
        address stands, so captured steps follow (the copy itself runs outside any graph).  The first
        call allocates the anchor.  Of a sharded buffer the master must be whole (``gather_master``)."""
        self._refuse_inside_ema("set_prox_anchor()")
        if self._ldnn_capturing:
            raise RuntimeError("set_prox_anchor() during a graph capture: the copy would not be recorded as a "
                               "host-side call; anchor before the capture or between replays")
        if self._prox_conf() is None:
            raise RuntimeError("set_prox_anchor(): the proximal term is off (prox_mu is None or 0)")
        f = self._one_flat("prox_mu")
        if f is None:
            for g in self.param_groups:
                for p in g["params"]:
                    ps = self.state.setdefault(p, {})
                    if "prox_anchor" in ps:
                        ps["prox_anchor"].copy_(p.data)
                    else:
                        ps["prox_anchor"] = p.detach().clone()
            return
        st = self._ls()
        a = st.get("prox_anchor")
        if a is None or a.shape != f.master.shape or a.device != f.master.device:
            st["prox_anchor"] = f.master.detach().clone()
        else:
            a.copy_(f.master)

    def prox_stats(self):
        """``{"mu": float, "drift_norm": float or None}``: ``mu`` (0.0 when off) and ``|w - a|_2`` over
        the flat master (loose tensors: over all of them) in fp64 torch ops, None before any anchor
        exists.  One host sync; meant for once per global epoch."""
        mu = self._prox_conf()
        f = self._one_flat("prox_mu") if mu is not None else None
        sq = None
        if f is not None:
            a = self._ls().get("prox_anchor")
            if a is not None and a.shape == f.master.shape and a.device == f.master.device:
                sq = (f.master.double() - a.double()).square().sum()
        elif mu is not None:
            pairs = [(p, self.state.get(p, {}).get("prox_anchor")) for g in self.param_groups for p in g["params"]]
            if pairs and all(a is not None for _, a in pairs):
                sq = sum((p.detach().double() - a.double()).square().sum().cpu() for p, a in pairs)
        return {"mu": mu or 0.0, "drift_norm": None if sq is None else float(sq.sqrt())}

    # ---- per-step learning-rate schedule -------------------------------------------------
    _check_schedule = staticmethod(check_lr_schedule)

    def _sched_conf(self):
        """``_sched_consts`` of the schedule, or None when it is off.  One schedule for the whole
        optimizer; the key is read with .get, so state saved before it existed loads."""
        sched = self._same_in_groups(lambda g: g.get("lr_schedule"),
                                     "lr_schedule must be the same in every param group")
        if sched is None:
            return None
        # (validated once per value: a step, a sync and a stats call only compare the dict)
        seen = self.__dict__.get("_ldnn_sched_seen")
        if seen is None or seen[0] != sched:
            self._ldnn_sched_seen = seen = (dict(sched), _sched_consts(sched))
        return seen[1]

    def _host_sched(self, conf, base, skip):
        """One step of the schedule on the host (CPU, loose tensors, several groups): the factor of
        the step about to run; the count ``sched_steps`` advances unless the step is skipped."""
        st = self._ls()
        hdr = st.pop("sched_hdr", None)
        if hdr is not None:     # (the buffer moved off the native path: its device count comes along)
            st["sched_steps"] = int(hdr[_SCHED_STEPS].item())
            st.pop("sched_written", None)
        if skip:
            return st.get("sched_last", (0.0, 0.0))[0]
        t = st.get("sched_steps", 0)
        s = lr_schedule_factor(conf, t + 1)
        st["sched_steps"], st["sched_last"] = t + 1, (s, base * s)
        return s

    def lr_schedule_stats(self):
        """The scalars ``steps`` (non-skipped steps the schedule has counted), ``factor`` and ``lr``
        (the last non-skipped step's ``s`` and rate; 0 before the first) -- on the fused path device
        scalars, reading one syncs -- or None when the schedule is off."""
        if self._sched_conf() is None:
            return None
        st = self._ls()
        hdr, hp = st.get("sched_hdr"), st.get("hp")
        if hdr is not None and hp is not None:
            return {"steps": hdr[_SCHED_STEPS], "factor": hdr[_SCHED_FACTOR], "lr": hp[0]}
        s, lr = st.get("sched_last", (0.0, 0.0))
        return {"steps": torch.tensor(float(st.get("sched_steps", 0))), "factor": torch.tensor(s, dtype=torch.float64),
                "lr": torch.tensor(lr, dtype=torch.float64)}

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

    # ---- the step ---------------------------------------------------------------------
    @torch.no_grad()
    def step(self, closure=None, clear_grads: bool = False):
        """clear_grads: the update kernel also zeroes the flat gradient after reading it
        (one pass instead of a later zero_grad fill; on MI355X the zero writes inside
        the bandwidth-bound update cost about what the fill launch does)."""
        loss = closure() if closure is not None else None
        self._refuse_inside_ema("step()")
        groups = self.param_groups
        flats = [self._flat_for_group(g) for g in groups]
        clip = sched = None
        loose_ema = None     # the EMA over loose tensors (a flat buffer's rides on its _FlatStep)
        if self._ema_conf() is not None and self._ema_flat() is None:
            loose_ema = self._loose_ema_begin()
        if self._prox_conf() is not None:
            self._one_flat("prox_mu")     # (one anchor: one flat buffer, or loose tensors only)
        if len(flats) != 1 or flats[0] is None:
            # several groups / loose tensors: one norm over all of them in torch ops; and one LARS
            # setting for every group, or a ValueError, before any update
            if self._clip_threshold() is not None:
                clip = self._loose_clip(flats)
            self._lars_conf()
            # ... and one schedule step on the host for all of them (a single flat buffer's rides
            # on its _FlatStep), each group's own rate times the factor
            conf = self._sched_conf()
            if conf is not None and groups:
                sched = self._host_sched(conf, groups[0]["lr"], clip is not None and clip[1])
        loose = {}           # what the per-tensor updates of this step share
        for group, f in zip(groups, flats):
            if f is not None:
                self._flat_step(f, group, clip, clear_grads, sched)
            elif clip is None or not clip[1]:
                if sched is not None:
                    group = dict(group, lr=group["lr"] * sched)
                self._loose_update(group, clip[0] if clip is not None else None, loose)
        if loose_ema is not None:
            ps, hdr = loose_ema
            skipped = clip is not None and clip[1]
            _ema_begin_torch(hdr, skipped)
            if not skipped:
                for p in ps:
                    _ema_update_torch(self.state[p]["ema"], p.data, hdr)
        return loss

    def _flat_step(self, f, group, clip, clear_grads, sched=None):
        """One ``_FlatStep`` over the whole flat buffer; when DataParallel(shard_optimizer=True)
        owns ``f`` (``f.shard_sync``, a GradBucketer), over this rank's flat ranges (its shard of
        every reduce-scattered bucket + the replicated tail) with ONE all-reduce of ``local``
        between the norm and the update, after which the wrapper starts the weight all-gathers.
        ``shard_sync.step_driver(step)`` replaces the sharded sequence (GraphedDPStep's capture)."""
        sh = getattr(f, "shard_sync", None)
        if sh is not None and len(self.param_groups) != 1:
            # the full-replica update would read flat.grad, of which only this rank's shards hold
            # reduced values, and no weight all-gather would follow: replicas would silently diverge
            raise RuntimeError("DataParallel(shard_optimizer=True) needs ONE param group holding the whole "
                               f"flat buffer; this optimizer has {len(self.param_groups)}")
        f.finalize_grads()
        s = _FlatStep(self, f, group, clip, sh is not None, sched)
        if sh is None:
            n = f.numel
            if s.normed:
                s.norm(((0, n),))
            s.finalize(False)
            if s.M is not None:
                s.moments(((0, n),), ((0, n),))
                s.ratios(False)
            s.update(0, n, ((0, n),) if clear_grads else ())
            s.end()
            return
        if sh.step_driver is not None:
            sh.step_driver(s)
        else:
            if s.local is not None:
                s.norm(sh.norm_ranges())
                sh.comm.all_reduce(s.local)
            s.finalize(reduced=s.local is not None)
            if s.M is not None:
                s.moments(sh.update_ranges(), sh.norm_ranges())
                sh.comm.all_reduce(s.local2)
                s.ratios(reduced=True)
            for lo, hi in sh.update_ranges():
                s.update(lo, hi)
            s.end()
        sh.after_update()

    def range_updater(self):
        """A ``_FlatStep``, finalized, for ONE step of a single flat-buffer group on the GPU
        applied as several range launches (None when the optimizer cannot update by ranges:
        several groups, no FlatParams, CPU, clipping or LARS).  ``update(lo, hi)`` runs the fused
        kernel on flat elements [lo, hi) on the current stream; ``end()`` closes the step.  Every
        element must be covered exactly once per step.  (The sharded step and GraphedDPStep's
        per-bucket optimizer graphs drive the same object.)"""
        if not self.supports_ranges():
            return None
        group = self.param_groups[0]
        s = _RangeStep(self, self._flat_for_group(group), group)
        s.finalize(reduced=False)
        return s

    def supports_ranges(self) -> bool:
        if self._clip_threshold() is not None:
            return False   # the whole norm must be known before any range updates
        if self._lars_conf() is not None or self._lamb_conf() is not None:
            return False   # ... and so must a tensor's whole gradient (LAMB: direction) before any of it moves
        if len(self.param_groups) != 1 or type(self)._update_native is _FlatOptimizer._update_native:
            return False
        f = self._flat_for_group(self.param_groups[0])
        return f is not None and _ext.use_native(f.master)

    # ---- what an optimizer supplies (``s``: the _FlatStep; ``sl``: the flat slice, None = whole) ----
    def _begin_ranges(self, s) -> dict:
        """Per-step prologue on the current stream, before any range: returns ``s.ctx``."""
        return {}

    def _update_native(self, s, sl, zero):
        raise NotImplementedError

    def _update_torch(self, s, sl, p, g, ratio):
        raise NotImplementedError

    def _loose_update(self, group, cl, loose):
        raise NotImplementedError

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
                 max_grad_norm=None, lars_trust=None, lars_eps=1e-8, lars_exclude_1d=True, ema_decay=None,
                 ema_warmup=True, lr_schedule=None, prox_mu=None):
        if lars_trust is not None and lars_trust <= 0:
            raise ValueError(f"lars_trust must be positive (None: LARS off); got {lars_trust}")
        self._check_ema_decay(ema_decay)
        check_prox_mu(prox_mu)
        super().__init__(params, dict(lr=lr, momentum=momentum, dampening=dampening, weight_decay=weight_decay,
                                      nesterov=nesterov, max_grad_norm=max_grad_norm, lars_trust=lars_trust,
                                      lars_eps=lars_eps, lars_exclude_1d=lars_exclude_1d, ema_decay=ema_decay,
                                      ema_warmup=ema_warmup, lr_schedule=self._check_schedule(lr_schedule),
                                      prox_mu=prox_mu))

    def _begin_ranges(self, s):
        # (``first`` is host-driven: the very first step seeds the momentum)
        return s.st.get("step", 0) == 0, self._buf("momentum", s.f.master) if s.group["momentum"] != 0 else s.f.master

    def _update_native(self, s, sl, zero):
        f, g, L = s.f, s.group, s.L
        first, mom = s.ctx
        p, grad, mom, shadow = _cut(sl, f.master, f.grad, mom, f.shadow)
        lars = None
        if L is not None:
            lars = (L.ratio, L.segmap if sl is None else L.segmap[sl.start // 64: sl.stop // 64])
        _ext.C().sgd_step(p, grad, mom, shadow, s.hp, f.grad_scale, g["momentum"], g["dampening"], g["weight_decay"],
                          g["nesterov"], first, zero_ranges=zero, clip=s.cl, lars=lars, prox=s.prox_arg(sl))

    def _update_torch(self, s, sl, p, g_, ratio):
        g, mu = s.group, s.group["momentum"]
        first, mom = s.ctx
        self._sgd_torch(p, g_, _cut(sl, mom)[0] if mu != 0 else None, s.lr, mu, g["dampening"],
                        g["weight_decay"], g["nesterov"], first, ratio=ratio, prox=s.prox_term(sl, p))

    def _loose_update(self, group, cl, loose):
        lr, mu, damp, wd, nest = (group[k] for k in ("lr", "momentum", "dampening", "weight_decay", "nesterov"))
        lars, prox_mu = self._lars_conf(), self._prox_conf()
        if lars is not None and not loose:
            # LARS over tensors outside a flat buffer: the next parameter's index, rows of (ratio, wn, gn)
            ps_all = [p for g_ in self.param_groups for p in g_["params"]]
            loose.update(k=0, L=self._lars_state(lars[2], None, ps_all, ps_all[0].device))
            self._write_hyperparams()
        for p in group["params"]:
            if loose:
                k = loose["k"]
                loose["k"] += 1
            if p.grad is None:
                continue
            if cl is not None:
                p.grad.mul_(cl[_CLIP_COEF].to(p.grad.device))
            ps = self.state.setdefault(p, {})
            first = "momentum_buffer" not in ps
            if mu != 0 and first:
                ps["momentum_buffer"] = torch.zeros_like(p)
            ratio = None
            if loose:
                L = loose["L"]
                wn, gn = float(p.detach().double().norm()), float(p.grad.double().norm())
                ratio = 1.0
                if L.adapt[k] and wn > 0 and gn > 0:
                    ratio = lars[0] * wn / (gn + wd * wn + lars[1])
                L.ratio[k], L.w_norm[k], L.g_norm[k] = ratio, wn, gn
            self._sgd_torch(p.data, p.grad, ps.get("momentum_buffer"), lr, mu, damp, wd, nest, first, ratio=ratio,
                            prox=self._loose_prox(p, prox_mu))

    @staticmethod
    def _sgd_torch(p, g, buf, lr, mu, damp, wd, nest, first, ratio=None, prox=None):
        if wd != 0:
            g = g + wd * p
        if prox is not None:      # mu * (p0 - a)
            g = g + prox
        if ratio is not None:
            g = g * ratio
        if mu != 0:
            if first:
                buf.copy_(g)
            else:
                buf.mul_(mu).add_(g, alpha=1 - damp)
            g = g + mu * buf if nest else buf
        p.add_(g, alpha=-lr)


def _adam_moments(m, v, g, b1, b2):
    m.mul_(b1).add_(g, alpha=1 - b1)
    v.mul_(b2).addcmul_(g, g, value=1 - b2)


class Adam(_FlatOptimizer):
    decoupled = False
    _bumps_step = True

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, max_grad_norm=None,
                 ema_decay=None, ema_warmup=True, lr_schedule=None, prox_mu=None):
        self._check_ema_decay(ema_decay)
        check_prox_mu(prox_mu)
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay,
                                      max_grad_norm=max_grad_norm, ema_decay=ema_decay, ema_warmup=ema_warmup,
                                      lr_schedule=self._check_schedule(lr_schedule), prox_mu=prox_mu))

    def _begin_ranges(self, s):
        if s.native:
            _ext.C().bump_step(s.hp, clip=s.cl)   # once per step, before any range reads the step count
        m = s.f.master
        return self._buf("exp_avg", m), self._buf("exp_avg_sq", m), s.st.get("step", 0) + 1

    def _update_native(self, s, sl, zero):
        f, g = s.f, s.group
        p, grad, m, v, shadow = _cut(sl, f.master, f.grad, s.ctx[0], s.ctx[1], f.shadow)
        _ext.C().adam_step(p, grad, m, v, shadow, s.hp, f.grad_scale, *g["betas"], g["eps"], g["weight_decay"],
                           self.decoupled, zero_ranges=zero, clip=s.cl, prox=s.prox_arg(sl))

    def _update_torch(self, s, sl, p, g_, ratio):
        g = s.group
        m, v = _cut(sl, s.ctx[0], s.ctx[1])
        self._adam_torch(p, g_, m, v, s.ctx[2], s.lr, *g["betas"], g["eps"], g["weight_decay"],
                         prox=s.prox_term(sl, p))

    def _loose_state(self, p, cl):
        """The per-tensor step of a loose ``p`` begins: its gradient clipped, its state (exp_avg,
        exp_avg_sq, step; created on the first step) with the step counted."""
        if cl is not None:
            p.grad.mul_(cl[_CLIP_COEF].to(p.grad.device))
        ps = self.state.setdefault(p, {})
        if "exp_avg" not in ps:
            ps["exp_avg"] = torch.zeros_like(p)
            ps["exp_avg_sq"] = torch.zeros_like(p)
            ps["step"] = 0
        ps["step"] += 1
        return ps

    def _loose_update(self, group, cl, loose):
        lr, (b1, b2), eps, wd = group["lr"], group["betas"], group["eps"], group["weight_decay"]
        prox_mu = self._prox_conf()
        for p in group["params"]:
            if p.grad is not None:
                ps = self._loose_state(p, cl)
                self._adam_torch(p.data, p.grad, ps["exp_avg"], ps["exp_avg_sq"], ps["step"], lr, b1, b2, eps, wd,
                                 prox=self._loose_prox(p, prox_mu))

    def _adam_torch(self, p, g, m, v, t, lr, b1, b2, eps, wd, prox=None):
        """``prox``: mu * (p0 - a), formed by the caller before the decoupled decay below touches p."""
        if wd != 0:
            if self.decoupled:
                p.mul_(1 - lr * wd)
            else:
                g = g + wd * p
        if prox is not None:
            g = g + prox
        _adam_moments(m, v, g, b1, b2)
        bc1 = 1 - b1 ** t
        bc2 = 1 - b2 ** t
        denom = (v.sqrt() / math.sqrt(bc2)).add_(eps)
        p.addcdiv_(m, denom, value=-lr / bc1)


class AdamW(Adam):
    decoupled = True

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, max_grad_norm=None,
                 ema_decay=None, ema_warmup=True, lr_schedule=None, prox_mu=None):
        super().__init__(params, lr, betas, eps, weight_decay, max_grad_norm, ema_decay, ema_warmup, lr_schedule,
                         prox_mu)


class Lamb(_FlatOptimizer):
    """LAMB (You et al. 2020): Adam's direction with a per-tensor trust ratio,

        m = b1 m + (1 - b1) g,  v = b2 v + (1 - b2) g^2
        u = (m / (1 - b1^t)) / (sqrt(v / (1 - b2^t)) + eps) + weight_decay * w
        w -= lr * r_i * u,   r_i = |w_i| / |u_i|  (1 when either norm is 0)

    ``g`` is the reduced, scaled and -- with ``max_grad_norm`` -- clipped gradient; the norms are
    taken before the weight write.  With ``lamb_exclude_1d`` (default) tensors with ``dim() < 2``
    keep ratio 1 (weight decay still applies to them).  No coefficient and no clamp on the ratio.
    On the flat GPU path ``lamb_moments`` updates the moments and reduces |w|, |u| per tensor,
    ``lamb_finalize`` leaves the ratios on the device and ``lamb_apply`` recomputes u from the
    moments and writes the weights and the bf16 shadow; sharded, the [2S] sums travel in one
    all-reduce after the moments (behind clipping's scalar all-reduce, if any).  Edge behaviour is
    LARS's: a per-tensor sum of squares beyond fp32 gives ratio 0, NaN norms give ratio 1 and the
    NaN propagates, and there is no non-finite guard without ``max_grad_norm``.  State keys are
    Adam's (``exp_avg``, ``exp_avg_sq``, ``step``); ``lamb_stats()`` reports the last ratios."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-6, weight_decay=0.0, max_grad_norm=None,
                 lamb_exclude_1d=True, ema_decay=None, ema_warmup=True, lr_schedule=None, prox_mu=None):
        self._check_ema_decay(ema_decay)
        if check_prox_mu(prox_mu) is not None:
            raise ValueError("Lamb takes no prox_mu: its trust ratio is defined on the Adam direction of g + "
                             "weight_decay * w; there is no agreed form with a proximal term")
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay,
                                      max_grad_norm=max_grad_norm, lamb_exclude_1d=lamb_exclude_1d,
                                      ema_decay=ema_decay, ema_warmup=ema_warmup,
                                      lr_schedule=self._check_schedule(lr_schedule)))

    _begin_ranges, _loose_state, _bumps_step, _prox_ok = Adam._begin_ranges, Adam._loose_state, True, False

    def _update_native(self, s, sl, zero):
        f, g, M = s.f, s.group, s.M
        p, grad, m, v, shadow = _cut(sl, f.master, f.grad, s.ctx[0], s.ctx[1], f.shadow)
        _ext.C().lamb_apply(p, grad, m, v, shadow, s.hp, *g["betas"], g["eps"], g["weight_decay"], M.ratio,
                            M.segmap if sl is None else M.segmap[sl.start // 64: sl.stop // 64], zero_ranges=zero,
                            clip=s.cl)

    @staticmethod
    def _direction(p, m, v, t, b1, b2, eps, wd):
        return (m / (1 - b1 ** t)) / ((v / (1 - b2 ** t)).sqrt() + eps) + wd * p

    def _moments_torch(self, s, p, g_, m, v):
        """The moment update of one flat range in torch ops; returns u."""
        g = s.group
        _adam_moments(m, v, g_, *g["betas"])
        return self._direction(p, m, v, s.ctx[2], *g["betas"], g["eps"], g["weight_decay"])

    def _update_torch(self, s, sl, p, g_, ratio):
        p.sub_(s.lr * ratio * _cut(sl, s.M.u)[0])

    def _loose_update(self, group, cl, loose):
        lr, (b1, b2), eps, wd = group["lr"], group["betas"], group["eps"], group["weight_decay"]
        if not loose:
            ps_all = [p for g_ in self.param_groups for p in g_["params"]]
            loose.update(k=0, M=self._lamb_state(self._lamb_conf(), None, ps_all, ps_all[0].device))
        M = loose["M"]
        for p in group["params"]:
            k = loose["k"]
            loose["k"] += 1
            if p.grad is None:
                continue
            ps = self._loose_state(p, cl)
            m, v = ps["exp_avg"], ps["exp_avg_sq"]
            _adam_moments(m, v, p.grad, b1, b2)
            u = self._direction(p.data, m, v, ps["step"], b1, b2, eps, wd)
            wn, un = float(p.detach().double().norm()), float(u.double().norm())
            ratio = wn / un if (M.adapt[k] and wn > 0 and un > 0) else 1.0
            M.ratio[k], M.w_norm[k], M.g_norm[k] = ratio, wn, un
            p.data.add_(u, alpha=-lr * ratio)


class Lion(_FlatOptimizer):
    """Lion (Chen et al. 2023, "evolved sign momentum"): one moment, the update is a sign,

        c = b1 m + (1 - b1) g
        w = w (1 - lr weight_decay) - lr sign(c)      (decoupled decay; no factor when weight_decay == 0)
        m = b2 m + (1 - b2) g                         (from the OLD m, after c)

    ``g`` is the reduced, scaled and -- with ``max_grad_norm`` -- clipped gradient; ``sign`` is +-1, 0 at
    +-0 and NaN at NaN.  There is no step count in the math (no bias correction) and no per-tensor norm,
    so the flat GPU step is ONE ``lion_step`` launch per range (22 B per element: w, g, m read, w, m and
    the bf16 shadow written; Adam moves 30), it updates by ranges like SGD / Adam (``supports_ranges()``;
    with clipping the whole norm comes first, as for Adam) and the sharded step needs no collective of
    its own.  The rate is ``hp[0]``: a captured step follows a changed lr and ``lr_schedule``.  Edge
    behaviour, beside LAMB's: no non-finite guard without ``max_grad_norm`` -- a NaN gradient element
    makes that element's ``m``, ``c``, ``sign(c)`` and ``w`` NaN (``torch.sign`` alone would give 0 there: the
    torch twin puts the NaN back), an infinite one moves ``w`` by ``lr`` and leaves ``m`` infinite; with
    ``max_grad_norm`` such a step is skipped whole (``w``, ``m``, shadow and EMA stay).  State: ``exp_avg``
    (fp32, shaped like the master, zero at first) and the host's ``step``; there is no ``exp_avg_sq``."""

    def __init__(self, params, lr=1e-4, betas=(0.9, 0.99), weight_decay=0.0, max_grad_norm=None, ema_decay=None,
                 ema_warmup=True, lr_schedule=None, prox_mu=None):
        if len(betas) != 2 or not all(0.0 <= b < 1.0 for b in betas):
            raise ValueError(f"Lion: betas must be two numbers in [0, 1); got {betas!r}")
        self._check_ema_decay(ema_decay)
        check_prox_mu(prox_mu)
        super().__init__(params, dict(lr=lr, betas=tuple(betas), weight_decay=weight_decay,
                                      max_grad_norm=max_grad_norm, ema_decay=ema_decay, ema_warmup=ema_warmup,
                                      lr_schedule=self._check_schedule(lr_schedule), prox_mu=prox_mu))

    def _begin_ranges(self, s):
        return self._buf("exp_avg", s.f.master)     # (no launch: nothing counts steps on the device)

    def _update_native(self, s, sl, zero):
        f, g = s.f, s.group
        p, grad, m, shadow = _cut(sl, f.master, f.grad, s.ctx, f.shadow)
        _ext.C().lion_step(p, grad, m, shadow, s.hp, f.grad_scale, *g["betas"], g["weight_decay"], zero_ranges=zero,
                           clip=s.cl, prox=s.prox_arg(sl))

    def _update_torch(self, s, sl, p, g_, ratio):
        g = s.group
        self._lion_torch(p, g_, _cut(sl, s.ctx)[0], s.lr, *g["betas"], g["weight_decay"], prox=s.prox_term(sl, p))

    def _loose_update(self, group, cl, loose):
        lr, (b1, b2), wd = group["lr"], group["betas"], group["weight_decay"]
        prox_mu = self._prox_conf()
        for p in group["params"]:
            if p.grad is None:
                continue
            if cl is not None:
                p.grad.mul_(cl[_CLIP_COEF].to(p.grad.device))
            ps = self.state.setdefault(p, {})
            if "exp_avg" not in ps:
                ps["exp_avg"] = torch.zeros_like(p)
            self._lion_torch(p.data, p.grad, ps["exp_avg"], lr, b1, b2, wd, prox=self._loose_prox(p, prox_mu))

    @staticmethod
    def _lion_torch(p, g, m, lr, b1, b2, wd, prox=None):
        if prox is not None:      # mu * (p0 - a): into c and m alike
            g = g + prox
        c = m * b1 + g * (1 - b1)
        s = torch.where(c != c, c, c.sign())      # (torch.sign(NaN) is 0; the kernel's is NaN)
        if wd != 0:
            p.mul_(1 - lr * wd)
        p.add_(s, alpha=-lr)
        m.mul_(b2).add_(g, alpha=1 - b2)


def build_optimizer(name: str, params, lr: float, momentum: float = 0.9, weight_decay: float = 0.0,
                    max_grad_norm: float | None = None, ema_decay: float | None = None, ema_warmup: bool = True,
                    lr_schedule: dict | None = None, prox_mu: float | None = None, **lars):
    """max_grad_norm: clip by the global L2 norm (None or <= 0: off).  ema_decay / ema_warmup: the
    weight EMA of every optimizer (None: off).  lr_schedule: the per-step schedule of every optimizer
    (a dict, see the module docstring; None: off).  prox_mu: FedProx's mu (None or 0: off; "lars" and
    "lamb" refuse a positive one with a ValueError).  "lars": SGD with
    ``lars_trust=0.001``; ``lars_trust`` / ``lars_eps`` / ``lars_exclude_1d`` go to SGD (and
    "sgd" takes them too); Adam, AdamW and Lion refuse them.  "lamb": Lamb, which takes
    ``lamb_exclude_1d`` (nobody else does) and refuses the ``lars_*`` keywords.  "lion": Lion at its
    default betas (0.9, 0.99); ``momentum`` is ignored, as for Adam."""
    name = name.lower()
    if max_grad_norm is not None and max_grad_norm <= 0:
        max_grad_norm = None
    allowed = {"lamb_exclude_1d"} if name == "lamb" else \
        set() if name in ("adam", "adamw", "lion") else {"lars_trust", "lars_eps", "lars_exclude_1d"}
    bad = set(lars) - allowed
    if bad:
        raise TypeError(f"build_optimizer({name!r}) got unexpected keyword arguments {sorted(bad)}")
    ema = dict(ema_decay=ema_decay, ema_warmup=ema_warmup, lr_schedule=lr_schedule, prox_mu=prox_mu)
    if name == "lamb":
        return Lamb(params, lr=lr, weight_decay=weight_decay, max_grad_norm=max_grad_norm, **ema, **lars)
    if name == "lars":
        lars.setdefault("lars_trust", 0.001)
        return SGD(params, lr=lr, momentum=momentum, weight_decay=weight_decay, max_grad_norm=max_grad_norm, **ema,
                   **lars)
    if name == "sgd":
        return SGD(params, lr=lr, momentum=momentum, weight_decay=weight_decay, max_grad_norm=max_grad_norm, **ema,
                   **lars)
    if name == "adam":
        return Adam(params, lr=lr, weight_decay=weight_decay, max_grad_norm=max_grad_norm, **ema)
    if name == "adamw":
        return AdamW(params, lr=lr, weight_decay=weight_decay, max_grad_norm=max_grad_norm, **ema)
    if name == "lion":
        return Lion(params, lr=lr, weight_decay=weight_decay, max_grad_norm=max_grad_norm, **ema)
    raise ValueError(f"unknown optimizer {name!r}")
