"""LAMB on the GPU: the lamb_moments / lamb_finalize / lamb_apply kernels (csrc/kernels/optim.hip),
their bindings' refusals, the launch budget of ``Lamb.step()`` (unsharded, sharded, captured), and
the LAMB step replayed from hipGraphs (GraphedStep, GraphedDPStep)."""
import os
import socket
import subprocess
import sys
import threading

import pytest
import torch

import ldnn
from ldnn.models import CrossEntropyLoss, build_model, xavier_init
from ldnn.models.mlp import MLP
from ldnn.ops import _ext
from ldnn.ops._ext import C
from ldnn.optim import Lamb
from ldnn.optim.optimizers import _Lars, lamb_chunk_table
from ldnn.parallel.comm import FakeWorld, LocalComm, _Done
from ldnn.parallel.ddp import DataParallel
from ldnn.train.graphed import GraphedDPStep, GraphedStep

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

COEF, SKIP = 1, 2
B1, B2, EPS, WD, GS, T = 0.9, 0.999, 1e-6, 1e-2, 0.5, 3


def _layout(lens, gaps=()):
    """[(begin, end)] of segments ``lens`` long, a 64-element alignment gap after those in ``gaps``."""
    bounds, off = [], 0
    for i, n in enumerate(lens):
        bounds.append((off, off + n))
        off += n + (64 if i in gaps else 0)
    return bounds, off


def _bufs(bounds, n, seed):
    """w, g, m, v: random inside the segments (v >= 0), NaN in the gaps (no chunk may touch them)."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    out = [torch.full((n,), float("nan"), device="cuda") for _ in range(4)]
    for b, e in bounds:
        out[0][b:e] = torch.randn(e - b, device="cuda", generator=g)
        out[1][b:e] = torch.randn(e - b, device="cuda", generator=g) * 3.0
        out[2][b:e] = torch.randn(e - b, device="cuda", generator=g) * 0.5
        out[3][b:e] = torch.rand(e - b, device="cuda", generator=g) * 2.0
    return out


def _bits(t):
    return t.view(torch.int32)


def _moments(bounds, ranges, counted, bufs, adapt, clip=None, slack=0, ext=None, sums=False):
    """lamb_moments on clones of m, v, then lamb_finalize; returns (ratio, wn, un) or the [2S] sums,
    the new m, v and the partials."""
    w, gr, m, v = bufs
    m, v = m.clone(), v.clone()
    S = len(bounds)
    chunks, segs = lamb_chunk_table(bounds, ranges, counted, C().seg_sumsq_chunk())
    i32 = dict(dtype=torch.int32, device="cuda")
    ct = torch.tensor(chunks, **i32).reshape(-1, 4)
    segtab = torch.tensor([(a, b, int(ad), 0) for (a, b), ad in zip(segs, adapt)], **i32).reshape(-1, 4)
    partials = torch.full((2 * len(chunks) + slack,), float("nan"), device="cuda")
    hp = torch.tensor([0.1, float(T)], device="cuda")
    assert C().lamb_moments(w, gr, m, v, ct, partials, hp, GS, B1, B2, EPS, WD, list(ranges), [b for b, _ in bounds],
                            clip=clip) == len(chunks)
    ratio, wn, un = torch.ones(65536, device="cuda"), torch.zeros(S, device="cuda"), torch.zeros(S, device="cuda")
    if sums:
        out = torch.zeros(2 * S, device="cuda")
        C().lamb_finalize(partials, segtab, ratio, wn, un, sums_out=out)
        return out, m, v, partials
    C().lamb_finalize(partials, segtab, ratio, wn, un, ext=ext, clip=clip)
    return (ratio, wn, un), m, v, partials


def _want(bounds, ranges, counted, bufs, adapt, coef=1.0):
    """fp64: the issue's formulas; per-segment norms over ``counted``, new m / v over ``ranges``."""
    w, gr, m, v = (t.double() for t in bufs)
    g = gr * GS * coef
    m2, v2 = m.clone(), v.clone()
    for lo, hi in ranges:
        m2[lo:hi] = B1 * m[lo:hi] + (1 - B1) * g[lo:hi]
        v2[lo:hi] = B2 * v[lo:hi] + (1 - B2) * g[lo:hi] ** 2
    u = (m2 / (1 - B1 ** T)) / ((v2 / (1 - B2 ** T)).sqrt() + EPS) + WD * w
    out = []
    for (b, e), ad in zip(bounds, adapt):
        ws = us = 0.0
        for lo, hi in counted:
            x, y = max(b, lo), min(e, hi)
            if y > x:
                ws += w[x:y].square().sum().item()
                us += u[x:y].square().sum().item()
        wn, un = ws ** 0.5, us ** 0.5
        out.append((wn / un if (ad and wn > 0 and un > 0) else 1.0, wn, un))
    return out, m2, v2


def _worst(got, want):
    ratio, wn, un = (t.cpu().double() for t in got)
    worst = 0.0
    for i, (r, a, b) in enumerate(want):
        for g_, w_ in ((ratio[i].item(), r), (wn[i].item(), a), (un[i].item(), b)):
            err = abs(g_ - w_) / w_ if w_ != 0 else abs(g_)
            assert err <= 1e-5, (i, g_, w_)
            worst = max(worst, err)
    assert bool((got[0][len(want):] == 1).all())     # the slots past the segments stay 1
    return worst


def _check_moments(m, v, m2, v2, bufs, ranges):
    """New moments inside ``ranges`` against fp64; everything else (the gaps' NaN too) bit-untouched."""
    inside = torch.zeros(m.numel(), dtype=torch.bool, device="cuda")
    for lo, hi in ranges:
        inside[lo:hi] = True
    live = ~torch.isnan(bufs[0])
    sel = inside & live
    torch.testing.assert_close(m[sel].double(), m2[sel], rtol=1e-5, atol=1e-6)
    torch.testing.assert_close(v[sel].double(), v2[sel], rtol=1e-5, atol=1e-6)
    for new, old in ((m, bufs[2]), (v, bufs[3])):
        assert torch.equal(_bits(new)[~sel], _bits(old)[~sel])


def test_lamb_moments_and_finalize_match_fp64():
    """Made-up layouts against the fp64 formulas; bound 1e-5 relative on every w_norm, u_norm and
    ratio (tests/test_lars_gpu.py::test_seg_sumsq_and_finalize_match_fp64 holds the same reduction
    structure to it; u adds a handful of fp32 roundings per element).  Measured maximum on MI355X:
    3.6e-6, on u_norm and the ratios -- not rounding in the sums but the bias correction:
    1 - beta2^t is 3.0e-3 at t = 3, and formed in fp32 from float(0.999) it is 6.6e-6 relative off
    the exact value (0.999 is not a float, and the power's rounding is large beside the small
    difference); half of that reaches u through the square root.  adam_kernel forms the same
    quantity the same way, which the apply test's agreement with adam_step relies on.  A
    4-workgroup grid cap and the default give the same bits, as do two runs; NaN in the alignment
    gaps and in the unused partial slots changes nothing and the gaps' m, v are untouched."""
    ch = C().seg_sumsq_chunk()
    assert ch % 64 == 0 and ch >= 1024
    layouts = [
        _layout([64, 128, ch - 64, ch, ch + 64, 3 * ch + 192], gaps=(1, 3)),
        _layout([192]),
        _layout([64] * 300),
    ]
    worst = 0.0
    for li, (bounds, n) in enumerate(layouts):
        S = len(bounds)
        adapt = [i % 4 != 1 for i in range(S)] if S > 1 else [True]
        bufs = _bufs(bounds, n, 30 + li)
        w0 = bufs[0].clone()
        last = bounds[-1]
        sets = [[(0, n)]]
        if li == 0:
            b2, b4 = bounds[2][0], bounds[4][0]
            sets.append([(b2 + 128, b4 + 64), (last[0] + 64, last[0] + 2 * ch + 128)])   # cut inside segments
            sets.append([(last[0] + ch + 64, last[0] + ch + 128)])                        # one 64-element piece
        for ranges in sets:
            chunks = lamb_chunk_table(bounds, ranges, ranges, ch)[0]
            assert all(0 < (e - b) * 64 <= ch and bounds[s][0] <= b * 64 and e * 64 <= bounds[s][1] and c == 1
                       for s, b, e, c in chunks)
            assert [c[0] for c in chunks] == sorted(c[0] for c in chunks)      # a segment's chunks are consecutive
            a, ma, va, _ = _moments(bounds, ranges, ranges, bufs, adapt)
            C().set_opt_max_blocks(4)          # fewer workgroups than chunks: the grid strides over them
            try:
                b, mb, vb, _ = _moments(bounds, ranges, ranges, bufs, adapt, slack=37)
            finally:
                C().set_opt_max_blocks(0)
            c, mc, vc, _ = _moments(bounds, ranges, ranges, bufs, adapt)
            want, m2, v2 = _want(bounds, ranges, ranges, bufs, adapt)
            worst = max(worst, _worst(a, want))
            _check_moments(ma, va, m2, v2, bufs, ranges)
            for other in ((b, mb, vb), (c, mc, vc)):
                for x, y in zip((*a, ma, va), (*other[0], other[1], other[2])):
                    assert torch.equal(_bits(x), _bits(y))
            assert torch.equal(_bits(bufs[0]), _bits(w0))                      # the weights are only read
        if li == 0:
            full = [(0, n)]
            # counted / uncounted: two complementary counted sets over the same moments ranges, their
            # sums added through ext, == the one-range result; the uncounted chunks' m, v still move
            mid = bounds[4][0] + 128
            s1, m1, v1, p1 = _moments(bounds, full, [(0, mid)], bufs, adapt, sums=True)
            s2, m2_, v2_, _ = _moments(bounds, full, [(mid, n)], bufs, adapt, sums=True)
            one, mo, vo, _ = _moments(bounds, full, full, bufs, adapt)
            for x, y in ((m1, mo), (m2_, mo), (v1, vo), (v2_, vo)):
                assert torch.equal(_bits(x), _bits(y))
            assert bool((p1 == 0).any()) and not bool(torch.isnan(p1).any())   # uncounted chunks store 0, 0
            segtab = torch.tensor([(0, 0, int(ad), 0) for ad in adapt], dtype=torch.int32, device="cuda")
            ratio, wn, un = torch.ones(65536, device="cuda"), torch.zeros(S, device="cuda"), torch.zeros(S, device="cuda")
            C().lamb_finalize(None, segtab, ratio, wn, un, ext=s1 + s2)
            for x, y in zip((ratio[:S], wn, un), (one[0][:S], one[1], one[2])):
                assert bool(((x - y).abs() <= 1e-6 * y.abs()).all())
            # the clip state's coefficient scales g only (u_norm is not scaled again); its skip flag
            # writes nothing at all
            st = torch.zeros(8, device="cuda")
            st[COEF] = 0.25
            c, mc, vc, _ = _moments(bounds, full, full, bufs, adapt, clip=st)
            want, m2, v2 = _want(bounds, full, full, bufs, adapt, coef=0.25)
            worst = max(worst, _worst(c, want))
            _check_moments(mc, vc, m2, v2, bufs, full)
            st[SKIP] = 1.0
            d, md, vd, pd = _moments(bounds, full, full, bufs, adapt, clip=st)
            assert bool((d[0] == 1).all()) and bool((d[1] == 0).all()) and bool((d[2] == 0).all())
            assert torch.equal(_bits(md), _bits(bufs[2])) and torch.equal(_bits(vd), _bits(bufs[3]))
            assert bool(torch.isnan(pd).all())
    print(f"lamb_moments + lamb_finalize worst relative error {worst:.3e}")


# ---------------------------------------------------------------- lamb_apply
N_OPT = 8192 + 64
# five segments and a gap; segment 2 spans element 4096, where a 4-workgroup grid's stride wraps
SEGS = [(0, 1024), (1024, 3072), (3072, 5120), (5184, 7232), (7232, N_OPT)]
RATIOS = [0.5, 1.0, 0.25, 1.0, 2.0]     # the gap maps to a slot that holds 1
LR = 0.1


def _apply_bufs(seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    p = torch.randn(N_OPT, device="cuda", generator=g)
    ratio = torch.ones(65536, device="cuda")
    seg_of = torch.full((N_OPT // 64,), 65535, dtype=torch.int64)
    for i, (b, e) in enumerate(SEGS):
        seg_of[b // 64: e // 64] = i
        ratio[i] = RATIOS[i]
    return dict(p=p, g=torch.randn(N_OPT, device="cuda", generator=g),
                m=torch.randn(N_OPT, device="cuda", generator=g) * 0.5,
                v=torch.rand(N_OPT, device="cuda", generator=g) * 2.0 + 0.05, sh=p.bfloat16(), ratio=ratio,
                map=seg_of.to(torch.uint16).cuda(), elem=ratio[seg_of.cuda()].repeat_interleave(64))


def _clone(b):
    return {k: v.clone() for k, v in b.items()}


def _apply(b, clip=None, zero=(), wd=WD, eps=EPS):
    hp = torch.tensor([LR, float(T)], device="cuda")
    C().lamb_apply(b["p"], b["g"], b["m"], b["v"], b["sh"], hp, B1, B2, eps, wd, b["ratio"], b["map"],
                   zero_ranges=list(zero), clip=clip)


def test_lamb_apply():
    """A hand-written ratio table (with 1 and the gap) against the formula in fp64, tolerance of
    tests/test_lars_gpu.py::test_fused_sgd_lars; zero ranges under a 4-workgroup cap (the stride
    wraps inside a segment); shadow == p.bfloat16() bitwise; the skip flag; and ratio 1, weight
    decay 0 == adam_step.  Measured maximum absolute error on MI355X: 5.9e-7."""
    b0 = _apply_bufs(41)
    zero = [(3, 5000), (8190, N_OPT)]
    want_g = b0["g"].clone()
    want_g[3:5000] = 0
    want_g[8190:] = 0
    C().set_opt_max_blocks(4)       # 4 workgroups x 256 threads x 4 elements: the stride wraps at 4096
    try:
        c = _clone(b0)
        _apply(c, zero=zero)
        p, m, v, r = (b0[k].double() for k in ("p", "m", "v", "elem"))
        u = (m / (1 - B1 ** T)) / ((v / (1 - B2 ** T)).sqrt() + EPS) + WD * p
        want = (p - LR * r * u).float()
        torch.testing.assert_close(c["p"], want, rtol=1e-5, atol=1e-6)
        print(f"lamb_apply max abs error {(c['p'].double() - (p - LR * r * u)).abs().max().item():.3e}")
        assert torch.equal(c["sh"], c["p"].bfloat16())
        assert torch.equal(c["g"], want_g)
        assert torch.equal(c["m"], b0["m"]) and torch.equal(c["v"], b0["v"])       # the moments are only read
        # a clip state without the skip flag changes nothing (the coefficient is the moments' business)
        st = torch.zeros(8, device="cuda")
        st[COEF] = 0.25
        c2 = _clone(b0)
        _apply(c2, clip=st, zero=zero)
        for k in ("p", "sh", "g"):
            assert torch.equal(c2[k], c[k]), k
        # the skip flag set: nothing but the zero ranges changes
        st[SKIP] = 1.0
        d = _clone(b0)
        _apply(d, clip=st, zero=zero)
        for k in ("p", "m", "v", "sh"):
            assert torch.equal(d[k], b0[k]), k
        assert torch.equal(d["g"], want_g)
    finally:
        C().set_opt_max_blocks(0)
    # ratio all ones, weight decay 0: the moments adam_step leaves, applied, == adam_step's weights
    e, f = _clone(b0), _clone(b0)
    hp = torch.tensor([LR, float(T)], device="cuda")
    C().adam_step(e["p"], e["g"], e["m"], e["v"], e["sh"], hp, 1.0, B1, B2, EPS, 0.0, False)
    f["m"], f["v"] = e["m"].clone(), e["v"].clone()
    f["ratio"].fill_(1.0)
    _apply(f, wd=0.0)
    torch.testing.assert_close(f["p"], e["p"], rtol=1e-5, atol=1e-6)
    assert not torch.equal(f["p"], b0["p"])


def test_binding_refusals_leave_the_buffers_alone():
    bounds, n = _layout([256, 256])
    bufs = _bufs(bounds, n, 40)
    keep = [t.clone() for t in bufs]
    w, gr, m, v = bufs
    chunks, segs = lamb_chunk_table(bounds, [(0, n)], [(0, n)], C().seg_sumsq_chunk())
    ct = torch.tensor(chunks, dtype=torch.int32, device="cuda").reshape(-1, 4)
    partials = torch.zeros(2 * len(chunks), device="cuda")
    hp = torch.tensor([0.1, 1.0], device="cuda")
    tail = (hp, GS, B1, B2, EPS, WD)
    with pytest.raises(RuntimeError, match="64-element aligned"):
        C().lamb_moments(w, gr, m, v, ct, partials, *tail, [(32, 256)], [0, 256])
    with pytest.raises(RuntimeError, match="multiple of 64"):
        C().lamb_moments(w, gr, m, v, ct, partials, *tail, [(0, n)], [0, 200])
    with pytest.raises(RuntimeError, match="64-element aligned"):
        C().lamb_moments(w, gr, m, v, ct, partials, *tail, [(0, n + 64)], [0, 256])      # past the buffers
    with pytest.raises(RuntimeError, match="2 slots per chunk"):
        C().lamb_moments(w, gr, m, v, ct, partials[:1], *tail, [(0, n)], [0, 256])
    with pytest.raises(RuntimeError):
        C().lamb_moments(w, gr, m.double(), v, ct, partials, *tail, [(0, n)], [0, 256])   # a wrong dtype
    with pytest.raises(RuntimeError):
        C().lamb_moments(w, gr, m, v[:-64], ct, partials, *tail, [(0, n)], [0, 256])      # a short buffer
    with pytest.raises(RuntimeError, match="chunks"):
        C().lamb_moments(w, gr, m, v, ct.to(torch.int32)[:, :3].contiguous(), partials, *tail, [(0, n)], [0, 256])
    with pytest.raises(ValueError, match="64-element aligned"):
        lamb_chunk_table(bounds, [(0, 100)], [(0, 100)], C().seg_sumsq_chunk())
    segtab = torch.tensor([(a, b, 1, 0) for a, b in segs], dtype=torch.int32, device="cuda")
    ratio, wn, un = torch.ones(65536, device="cuda"), torch.zeros(2, device="cuda"), torch.zeros(2, device="cuda")
    with pytest.raises(RuntimeError, match="ratio"):
        C().lamb_finalize(partials, segtab, ratio[:1], wn, un)
    with pytest.raises(RuntimeError, match="sums_out"):
        C().lamb_finalize(partials, segtab, ratio, wn, un, sums_out=torch.zeros(3, device="cuda"))
    for t, k in zip(bufs, keep):
        assert torch.equal(_bits(t), _bits(k))
    assert bool((partials == 0).all()) and bool((ratio == 1).all())
    b = _apply_bufs(42)
    hp = torch.tensor([LR, float(T)], device="cuda")

    def apply(**kw):
        a = dict(b, **kw)
        C().lamb_apply(a["p"], a["g"], a["m"], a["v"], a["sh"], hp, B1, B2, EPS, WD, a["ratio"], a["map"])

    with pytest.raises(RuntimeError, match="64-element aligned"):
        apply(**{k: b[k][:-32] for k in ("p", "g", "m", "v", "sh")})                       # a misaligned range
    with pytest.raises(RuntimeError, match="ratio table"):
        apply(ratio=b["ratio"][:100])                                                      # a short ratio table
    with pytest.raises(RuntimeError, match="map entry"):
        apply(map=b["map"][:-1])                                                           # a short map
    with pytest.raises(RuntimeError):
        apply(map=b["map"].to(torch.int32))
    with pytest.raises(RuntimeError):
        apply(sh=b["sh"].float())
    with pytest.raises(RuntimeError):
        apply(m=b["m"][:-64])
    for k, t in _apply_bufs(42).items():
        assert torch.equal(b[k], t), k


# ---------------------------------------------------------------- launch budget
_HOST_QUERIES = ("grad_sumsq_parts", "seg_sumsq_chunk")
_OPTIMIZER_CALLS = ("bump_step", "grad_sumsq", "sumsq_total", "clip_finalize", "lamb_moments", "lamb_finalize", "lamb_apply",
                    "adam_step", "sgd_step", "seg_sumsq", "lars_finalize")
_KW = (("clip", "clip"), ("ext", "ext"), ("sums_out", "sums_out"), ("zero_ranges", "zero"))

CONFIGS = {
    "lamb": (lambda p: Lamb(p, lr=1e-3, weight_decay=1e-2), {}),
    "lamb_clip": (lambda p: Lamb(p, lr=1e-3, weight_decay=1e-2, max_grad_norm=1.0), {}),
    "lamb_clear": (lambda p: Lamb(p, lr=1e-3), {"clear_grads": True}),
}
UNSHARDED = {
    "lamb": ["bump_step", "lamb_moments", "lamb_finalize", "lamb_apply"],
    "lamb_clip": ["grad_sumsq", "clip_finalize", "bump_step[clip]", "lamb_moments[clip]", "lamb_finalize[clip]",
                  "lamb_apply[clip]"],
    "lamb_clear": ["bump_step", "lamb_moments", "lamb_finalize", "lamb_apply[zero]"],
}
# 2-rank world, two sharded buckets + the replicated tail: (rank 0, rank 1, all-reduces per rank, ranges
# counted by rank 0 / rank 1).  Every rank runs the moments over, and applies, three ranges.
_SH_LAMB = ["bump_step", "lamb_moments", "lamb_finalize[sums_out]", "lamb_finalize[ext]"] + ["lamb_apply"] * 3
_SH_CLIP = ["sumsq_total", "clip_finalize[ext]", "bump_step[clip]", "lamb_moments[clip]", "lamb_finalize[sums_out]",
            "lamb_finalize[clip,ext]"] + ["lamb_apply[clip]"] * 3
SHARDED = {
    "lamb": (_SH_LAMB, _SH_LAMB, 1),
    "lamb_clip": (["grad_sumsq"] * 3 + _SH_CLIP, ["grad_sumsq"] * 2 + _SH_CLIP, 2),
}
GRAPH_LABELS = {"lamb": [None, "lamb"], "lamb_clip": [None, "clip", "lamb"]}


class _Recorder:
    """Stands in for the native module: forwards every call, logs launches per thread."""

    def __init__(self, real):
        self._real, self.logs = real, {}

    def __getattr__(self, name):
        fn = getattr(self._real, name)
        if not callable(fn) or name in _HOST_QUERIES:
            return fn

        def call(*a, **kw):
            tags = [tag for key, tag in _KW if kw.get(key) is not None and not (key == "zero_ranges" and not kw[key])]
            self.logs.setdefault(threading.get_ident(), []).append(name + ("[" + ",".join(tags) + "]" if tags else ""))
            return fn(*a, **kw)
        return call

    def take(self):
        return self.logs.pop(threading.get_ident(), [])


@pytest.fixture
def rec(monkeypatch):
    r = _Recorder(_ext.C())
    monkeypatch.setattr(_ext, "C", lambda: r)
    return r


def _model():
    torch.manual_seed(0)
    m = MLP(70, (33,), 10)
    ldnn.prepare(m, "cuda")
    return m


def _fill_grad(flat, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    flat.grad.copy_(torch.randn(flat.numel, device="cuda", generator=g))


def _flat(opt):
    return opt._flat_for_group(opt.param_groups[0])


def _record_step(rec, opt, kw, comm=None):
    """One warm-up step, then the calls (and all-reduces on ``comm``) of the next one."""
    f = _flat(opt)
    _fill_grad(f, 1)
    opt.step(**kw)
    _fill_grad(f, 2)
    n = [0]
    if comm is not None:
        real = comm.all_reduce
        comm.all_reduce = lambda *a, **k: (n.__setitem__(0, n[0] + 1), real(*a, **k))[1]
    rec.take()
    opt.step(**kw)
    return rec.take(), n[0]


def _sharded_rank(comm, rec, name):
    mk, kw = CONFIGS[name]
    m = _model()
    dp = DataParallel(m, comm, bucket_cap_mb=0.005, shard_optimizer=True)
    assert dp.sharded and [b["sharded"] for b in dp.bucketer.buckets] == [True, True, False]
    opt = mk(m.parameters())
    calls, reduces = _record_step(rec, opt, {}, comm)
    dp.wait_gathers()
    torch.cuda.synchronize()
    keys = list(opt._ls()["lamb"].tables)
    assert len(keys) == 1
    return calls, reduces, len(keys[0][0]), len(keys[0][1])


@pytest.mark.parametrize("name", list(CONFIGS))
def test_unsharded_step_launches(rec, name):
    mk, kw = CONFIGS[name]
    assert _record_step(rec, mk(_model().parameters()), kw)[0] == UNSHARDED[name]


@pytest.mark.parametrize("name", ["lamb", "lamb_clip"])
def test_sharded_step_launches_and_collectives(rec, name):
    res = FakeWorld(2).run(_sharded_rank, rec, name)
    for r in range(2):
        assert res[r][:2] == (SHARDED[name][r], SHARDED[name][2]), r
        assert res[r][2] == 3                        # moments (and applies) over three ranges
    assert res[0][3] == 3 and res[1][3] == 2         # rank 0 also counts the replicated tail


def _state_ids(opt):
    ids = {}
    for k, v in opt._ls().items():
        if torch.is_tensor(v):
            ids[k] = id(v)
        elif isinstance(v, _Lars):
            ids[k] = id(v)
            ids.update({f"{k}.{a}": id(t) for a, t in vars(v).items() if torch.is_tensor(t)})
            for key, tab in v.tables.items():
                ids.update({f"{k}.tables{key}.{a}": id(t) for a, t in tab.items() if torch.is_tensor(t)})
    return ids


@pytest.mark.parametrize("name", list(CONFIGS))
def test_captured_step_issues_the_eager_calls_and_allocates_nothing(rec, name):
    mk, kw = CONFIGS[name]
    opt = mk(_model().parameters())
    f = _flat(opt)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        eager, _ = _record_step(rec, opt, kw)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    before = _state_ids(opt)
    assert any(k.startswith("lamb.tables") for k in before)
    _fill_grad(f, 3)
    graph = torch.cuda.CUDAGraph()
    opt._ldnn_capturing = True
    try:
        with torch.cuda.graph(graph, stream=s):
            opt.step(**kw)
    finally:
        opt._ldnn_capturing = False
    assert rec.take() == eager == UNSHARDED[name]
    assert _state_ids(opt) == before
    master = f.master.clone()
    graph.replay()
    torch.cuda.synchronize()
    assert not torch.equal(master, f.master)     # the graph holds the update


def test_capture_without_an_eager_step_is_refused(rec):
    opt = CONFIGS["lamb_clip"][0](_model().parameters())
    _fill_grad(_flat(opt), 1)
    opt._ldnn_capturing = True
    with pytest.raises(RuntimeError, match="run an eager optimizer step before capturing"):
        opt.step()
    assert not any(torch.is_tensor(v) for k, v in opt._ls().items() if k not in ("exp_avg", "exp_avg_sq"))
    assert "lamb" not in opt._ls()


class _TwoRankEcho(LocalComm):
    """One process standing in for rank 0 of two (as tests/test_graphed_dp_gpu.py does)."""
    world_size = 2

    def reduce_scatter(self, out, inp, async_op=False):
        self.record("reduce_scatter", inp)
        out.copy_(inp[: out.numel()])
        return _Done() if async_op else None

    def all_gather_into(self, out, inp, async_op=False):
        self.record("all_gather_into", out)
        return _Done() if async_op else None


@pytest.mark.parametrize("name", ["lamb", "lamb_clip"])
def test_graphed_dp_capture_drives_the_sharded_step(rec, name):
    """GraphedDPStep's capture runs the sharded LAMB step through ``GradBucketer.step_driver``: the
    calls it captures are rank 0's eager ones, in a moments graph and a "lamb" graph (with clipping:
    a norm graph, a "clip" graph holding the moments, a "lamb" graph), and it allocates nothing."""
    m = _model()
    dp = DataParallel(m, _TwoRankEcho(), bucket_cap_mb=0.005, broadcast_init=False, shard_optimizer=True)
    assert dp.sharded and len(dp.bucketer.buckets) == 3
    opt = CONFIGS[name][0](m.parameters())
    g = torch.Generator(device="cuda").manual_seed(5)
    x = torch.randn(16, 70, device="cuda", generator=g).bfloat16()
    y = torch.randint(0, 10, (16,), device="cuda", generator=g)
    crit = CrossEntropyLoss()
    opt.zero_grad()
    crit(dp(x), y).backward()
    dp.finish_gradient_sync()
    opt.step()
    dp.wait_gathers()
    torch.cuda.synchronize()
    before = _state_ids(opt)
    rec.take()
    gd = GraphedDPStep(dp, crit, opt, x, y)
    calls = [c for c in rec.take() if c.split("[")[0] in _OPTIMIZER_CALLS]
    assert calls == SHARDED[name][0]
    assert _state_ids(opt) == before
    assert [i for _, i in gd.g_opts] == GRAPH_LABELS[name]
    n0 = dp.comm.schedule_digest()[0]
    master = _flat(opt).master.clone()
    gd(x, y)
    dp.wait_gathers()
    torch.cuda.synchronize()
    assert not torch.equal(master, _flat(opt).master)
    ops = dp.comm.schedule_digest()[0] - n0
    gd(x, y)
    dp.wait_gathers()
    torch.cuda.synchronize()
    assert dp.comm.schedule_digest()[0] - n0 == 2 * ops      # the same collectives every replay


# ---------------------------------------------------------------- graphed steps
def _models(name, n):
    torch.manual_seed(0)
    ms = [build_model(name) for _ in range(n)]
    xavier_init(ms[0])
    for m in ms[1:]:
        m.load_state_dict(ms[0].state_dict())
    for m in ms:
        ldnn.prepare(m, "cuda")
    return ms


def test_graphed_step_with_lamb_matches_eager():
    """LeNet-5, batch 8, LAMB with weight decay: 4 replays == 4 eager steps (two eager runs give
    the spread, as tests/test_lars_gpu.py::test_graphed_step_with_lars_matches_eager judges it).
    An adapted tensor moves by exactly lr * |w| (|lr r u| = lr |w|), so the lr a replay applied can
    be read off its update: the lr made 10x smaller between replays 2 and 3 is the one replay 3
    applies (within 1 %)."""
    lr = 2e-3
    m1, m2, m3 = _models("lenet5", 3)
    o1, o2, o3 = (Lamb(m.parameters(), lr=lr, weight_decay=1e-2) for m in (m1, m2, m3))
    crit = CrossEntropyLoss()
    g = torch.Generator(device="cuda").manual_seed(1)
    xs = [torch.randn(8, 1, 28, 28, device="cuda", generator=g).bfloat16() for _ in range(5)]
    ys = [torch.randint(0, 10, (8,), device="cuda", generator=g) for _ in range(5)]
    for m, o in ((m1, o1), (m2, o2), (m3, o3)):
        o.zero_grad()
        crit(m(xs[0]), ys[0]).backward()
        o.step()
    p0 = [q.detach().clone() for q in m2.parameters()]
    gs = GraphedStep(m1, crit, o1, xs[1], ys[1], warmup=0)
    f1 = _flat(o1)
    implied = []
    for i in range(1, 5):
        if i == 3:
            for o in (o1, o2, o3):
                o.param_groups[0]["lr"] = lr / 10
        before = f1.master.clone()
        gs(xs[i], ys[i])
        for m, o in ((m2, o2), (m3, o3)):
            o.zero_grad()
            crit(m(xs[i]), ys[i]).backward()
            o.step()
        st = o1.lamb_stats()
        M = o1._ls()["lamb"]
        moved = []
        for k, ((b, e), ad) in enumerate(zip(M.bounds, st["adapted"])):
            if ad and float(st["w_norm"][k]) > 0:
                moved.append((f1.master[b:e] - before[b:e]).double().norm().item() / float(st["w_norm"][k]))
        implied.append(moved)
        r1, r2 = o1.lamb_stats()["ratio"], o2.lamb_stats()["ratio"]
        assert bool(((r1 - r2).abs() <= 2e-2 * r2.abs()).all()), (i, r1, r2)
    for moved, want in zip(implied, (lr, lr, lr / 10, lr / 10)):
        assert moved and all(abs(v - want) <= 1e-2 * want for v in moved), (moved, want)
    ad = o1.lamb_stats()["adapted"]
    assert any(ad) and not all(ad)
    assert bool((o1.lamb_stats()["ratio"][~torch.tensor(ad, device="cuda")] == 1).all())
    assert bool((o1.lamb_stats()["ratio"][torch.tensor(ad, device="cuda")] != 1).any())
    torch.cuda.synchronize()
    for (n, p), (_, q), (_, s), r in zip(m1.named_parameters(), m2.named_parameters(), m3.named_parameters(), p0):
        d1, d2, d3 = ((t.detach() - r).flatten().double() for t in (p, q, s))
        eg, ee = (d1 - d2).norm().item(), (d3 - d2).norm().item()
        assert eg <= 3.0 * ee + 2e-3 * d2.norm().item(), (n, eg, ee, d2.norm().item())


@pytest.mark.parametrize("clip", [None, 0.5])
def test_graphed_dp_world1_lamb_equals_single_process(clip):
    """GraphedDPStep on a world-1 comm, shard_optimizer on and off, == the single-process graphed
    step, with the odd-batch eager fallback; tolerance of
    tests/test_lars_gpu.py::test_graphed_dp_world1_lars_equals_single_process."""
    shape = (128, 1, 28, 28)
    m1, m2, m3 = _models("lenet5", 3)
    crit = CrossEntropyLoss()
    dps = [DataParallel(m1, LocalComm(), bucket_cap_mb=0.05, broadcast_init=False, shard_optimizer=True),
           DataParallel(m2, LocalComm(), bucket_cap_mb=0.05, broadcast_init=False)]
    opts = [Lamb(m.parameters(), lr=2e-3, weight_decay=1e-2, max_grad_norm=clip) for m in (m1, m2, m3)]
    g = torch.Generator(device="cuda").manual_seed(2)
    xs = [torch.randn(*shape, device="cuda", generator=g).bfloat16() for _ in range(4)]
    ys = [torch.randint(0, 10, (shape[0],), device="cuda", generator=g) for _ in range(4)]
    p0 = [p.detach().clone() for p in m3.parameters()]
    for dp, o in zip(dps, opts):
        o.zero_grad()
        crit(dp(xs[0]), ys[0]).backward()
        dp.finish_gradient_sync()
        o.step()
        dp.wait_gathers()
    opts[2].zero_grad()
    crit(m3(xs[0]), ys[0]).backward()
    opts[2].step()
    gds = [GraphedDPStep(dp, crit, o, xs[0], ys[0]) for dp, o in zip(dps, opts)]
    gs = GraphedStep(m3, crit, opts[2], xs[0], ys[0], warmup=0)
    for i in range(1, 4):
        for s in (*gds, gs):
            s(xs[i], ys[i])
    for s in (*gds, gs):                 # the odd-shaped batch: the eager fallback
        s(xs[0][:50], ys[0][:50])
    dps[0].gather_master(opts[0])
    torch.cuda.synchronize()
    stats = [dict(zip(o.lamb_stats()["names"], o.lamb_stats()["ratio"].tolist())) for o in opts]
    for st in stats[:2]:
        for n, v in stats[2].items():
            assert st[n] == pytest.approx(v, rel=2e-2), n
    assert any(v != 1.0 for v in stats[2].values())
    if clip is not None:
        # (with clipping the saved step is the device count, as for Adam: replays advance it)
        assert all(o.state_dict()["ldnn_flat_state"]["step"] == 5 for o in opts)
        cs = [{k: v.item() for k, v in o.grad_clip_stats().items()} for o in opts]
        assert cs[0]["steps"] == cs[1]["steps"] == cs[2]["steps"] == 5 and cs[0]["skipped"] == 0
    for ma in (m1, m2):
        for a, b, r in zip(ma.parameters(), m3.parameters(), p0):
            da, db = (a.detach() - r).double(), (b.detach() - r).double()
            assert (da - db).norm().item() <= 2e-2 * db.norm().item() + 1e-6


@pytest.mark.parametrize("clip", [None, "0.5"])
def test_graphed_dp_two_ranks_gloo_with_lamb(clip):
    """2 gloo ranks sharing the GPU (scripts/check_graphed_dp.py --optimizer lamb --shard [--clip]):
    the graphed sharded LAMB step == ONE graphed rank on the concatenated batches == the unsharded
    run, the schedule check passes, replicas identical."""
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.join(ROOT, "scripts", "check_graphed_dp.py"), "--optimizer", "lamb",
           "--shard"] + (["--clip", clip] if clip else [])
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    assert "GRAPHED_DP_OK" in r.stdout, r.stdout[-3000:]
