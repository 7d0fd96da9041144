"""Lion on the GPU: the lion_step kernel (csrc/kernels/optim.hip) against fp64 -- bit for bit on a
fixture whose arithmetic is exact in fp32, within bounds on random inputs --, its zero ranges, clip
state and binding refusals, the launch budget of ``Lion.step()`` (eager, by ranges, captured), and the
Lion step replayed from hipGraphs (GraphedStep, GraphedDPStep)."""
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
from ldnn.optim import Lion
from ldnn.parallel.comm import LocalComm
from ldnn.parallel.ddp import DataParallel
from ldnn.train.graphed import GraphedDPStep, GraphedStep

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

COEF, SKIP = 1, 2
N_MAIN = 4 * 4096 + 3      # whole float4s past one sweep of a 4-workgroup grid (4096 elements), and a 3-element tail


def _bits(t):
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def _sign(c):
    return torch.where(c != c, c, torch.sign(c))


def _ref64(w, g, m, lr, b1, b2, wd, gs):
    """One step of the formulas in fp64; returns (w, m, c)."""
    g = g * gs
    c = b1 * m + (1 - b1) * g
    if wd != 0:
        w = w * (1 - lr * wd)
    return w - lr * _sign(c), b2 * m + (1 - b2) * g, c


# ---------------------------------------------------------------- 1. exact fixture
EX = dict(b1=0.5, b2=0.75, lr=2.0 ** -6, gs=0.5)


def _exact_inputs(n, seed):
    g = torch.Generator().manual_seed(seed)
    return [(torch.randint(-64, 65, (n,), generator=g).float() / 16).cuda() for _ in range(3)]


def _run_exact(n, steps, wd, with_shadow, seed, pad=0):
    """``steps`` lion_step calls on multiples of 1/16 in [-4, 4] (the sign of g alternates) against
    the fp64 formulas: w and m bit for bit, the shadow == w.bfloat16(); ``pad``: the n elements are
    the 64-aligned range [pad, pad + n) of NaN-filled buffers that must stay bit-untouched around it.
    Returns the number of elements that met c == 0."""
    w0, g0, m0 = _exact_inputs(n, seed)
    total = n + 3 * pad
    big = [torch.full((total,), float("nan"), device="cuda") for _ in range(3)]
    sh_big = torch.full((total,), float("nan"), device="cuda").bfloat16()
    sl = slice(pad, pad + n)
    for b, t in zip(big, (w0, g0, m0)):
        b[sl] = t
    sh_big[sl] = w0.bfloat16()
    keep = [b.clone() for b in big] + [sh_big.clone()]
    w, g, m = (b[sl] for b in big)
    sh = sh_big[sl] if with_shadow else None
    hp = torch.tensor([EX["lr"], 0.0], device="cuda")
    rw, rm = w0.double(), m0.double()
    zeros = 0
    for k in range(steps):
        gk = g0 if k % 2 == 0 else -g0
        g.copy_(gk)
        C().lion_step(w, g, m, sh, hp, EX["gs"], EX["b1"], EX["b2"], wd)
        rw, rm, c = _ref64(rw, gk.double(), rm, EX["lr"], EX["b1"], EX["b2"], wd, EX["gs"])
        zeros += int((c == 0).sum())
        # the fixture's premise: the fp64 results are fp32 numbers
        assert torch.equal(rw.float().double(), rw) and torch.equal(rm.float().double(), rm)
        assert torch.equal(_bits(w), _bits(rw.float())), (n, k, wd)
        assert torch.equal(_bits(m), _bits(rm.float())), (n, k, wd)
        if with_shadow:
            assert torch.equal(_bits(sh), _bits(w.bfloat16())), (n, k, wd)
        assert torch.equal(_bits(g), _bits(gk))                      # no zero range: the gradient is only read
    assert float(hp[1]) == 0.0
    out = torch.ones(total, dtype=torch.bool, device="cuda")
    out[sl] = False
    for b, k in zip(big + [sh_big], keep):
        assert torch.equal(_bits(b)[out], _bits(k)[out])
    if not with_shadow:
        assert torch.equal(_bits(sh_big), _bits(keep[3]))
    return zeros


@pytest.mark.parametrize("with_shadow", [True, False])
@pytest.mark.parametrize("cap", [0, 4])
def test_exact_fixture_matches_fp64_bit_for_bit(cap, with_shadow):
    """beta1 = 0.5, beta2 = 0.75, lr = 2^-6, grad_scale = 0.5 on multiples of 1/16: every product and
    sum is exact in fp32 for 4 steps without weight decay and for 2 steps with weight_decay = 0.25 (the
    factor 255/256 adds 8 bits a step), so any evaluation order or contraction gives the fp64 bits.
    Default grid and a 4-workgroup cap (the grid-stride loop wraps four times), with and without a
    shadow, n = 4 * 4096 + 3, the tail alone (n = 3), n = 64, and a 64-aligned range of a larger
    NaN-filled buffer.  381 of the fixture's elements meet c == 0; on MI355X no bit differs."""
    C().set_opt_max_blocks(cap)
    try:
        zeros = _run_exact(N_MAIN, 4, 0.0, with_shadow, 11) + _run_exact(N_MAIN, 2, 0.25, with_shadow, 12)
        for n in (3, 64):
            _run_exact(n, 4, 0.0, with_shadow, 13)
            _run_exact(n, 2, 0.25, with_shadow, 14)
        zeros += _run_exact(2 * 4096 + 64, 4, 0.0, with_shadow, 15, pad=128)
        zeros += _run_exact(2 * 4096 + 64, 2, 0.25, with_shadow, 16, pad=128)
    finally:
        C().set_opt_max_blocks(0)
    print(f"exact fixture (cap {cap}, shadow {with_shadow}): {zeros} elements met c == 0; 0 differing bits")
    assert zeros > 0         # sign(0) = 0 is exercised


# ---------------------------------------------------------------- 2. random inputs
B1, B2, WD, GS, LR = 0.9, 0.99, 1e-2, 0.5, 1e-3


def _bufs(n, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return (torch.randn(n, device="cuda", generator=g), torch.randn(n, device="cuda", generator=g) * 3.0,
            torch.randn(n, device="cuda", generator=g) * 0.5)


def test_random_inputs_match_fp64():
    """Seeded normals, betas (0.9, 0.99), weight decay 1e-2, grad_scale 0.5.  m within rtol 1e-5 /
    atol 1e-6 (the bound tests/test_lamb_gpu.py holds the same moment expression to); w within the
    same bound wherever the sign is decided.  An element is undecided when |c| <= 4 * 2^-24 *
    (|beta1 m| + |(1 - beta1) g|), c in fp64 (three fp32 roundings and one to spare): its w must be one
    of the three possible outcomes, and at most 0.01 % of the elements may be undecided.  Measured on
    MI355X: worst |dm| 1.4e-7, worst |dw| 2.3e-7, 0 of 16387 undecided."""
    n = N_MAIN
    w0, g0, m0 = _bufs(n, 21)
    w, g, m = w0.clone(), g0.clone(), m0.clone()
    sh = w.bfloat16()
    hp = torch.tensor([LR, 0.0], device="cuda")
    C().lion_step(w, g, m, sh, hp, GS, B1, B2, WD)
    rw, rm, c = _ref64(w0.double(), g0.double(), m0.double(), LR, B1, B2, WD, GS)
    und = c.abs() <= 4 * 2.0 ** -24 * ((B1 * m0.double()).abs() + ((1 - B1) * g0.double() * GS).abs())
    n_und = int(und.sum())
    assert n_und <= 1e-4 * n, n_und
    tol = lambda ref: 1e-6 + 1e-5 * ref.abs()      # noqa: E731
    em = (m.double() - rm).abs()
    assert bool((em <= tol(rm)).all())
    ew = (w.double() - rw).abs()
    assert bool((ew <= tol(rw))[~und].all())
    if n_und:
        base = w0.double()[und] * (1 - LR * WD)
        ok = torch.zeros(n_und, dtype=torch.bool, device="cuda")
        for s in (-1.0, 0.0, 1.0):
            cand = base - LR * s
            ok |= (w.double()[und] - cand).abs() <= tol(cand)
        assert bool(ok.all())
    assert torch.equal(_bits(sh), _bits(w.bfloat16())) and torch.equal(_bits(g), _bits(g0))
    print(f"lion_step random inputs (n = {n}): worst |dm| {em.max().item():.3e}, worst |dw| (decided) "
          f"{ew[~und].max().item():.3e}, undecided {n_und}")


# ---------------------------------------------------------------- 3. zero ranges
@pytest.mark.parametrize("skip", [False, True])
def test_zero_ranges_are_cleared_and_the_rest_of_the_gradient_is_untouched(skip):
    n = N_MAIN
    w0, g0, m0 = _bufs(n, 22)
    want_g = g0.clone()
    zero = [(3, 5000), (n - 6, n)]        # unaligned edges, across the grid-stride wrap, into the scalar tail
    for a, b in zero:
        want_g[a:b] = 0
    st = torch.zeros(8, device="cuda")
    st[COEF], st[SKIP] = 1.0, float(skip)
    hp = torch.tensor([LR, 0.0], device="cuda")
    for cap in (0, 4):
        w, g, m = w0.clone(), g0.clone(), m0.clone()
        sh = w.bfloat16()
        C().set_opt_max_blocks(cap)
        try:
            C().lion_step(w, g, m, sh, hp, GS, B1, B2, WD, zero_ranges=zero, clip=st)
        finally:
            C().set_opt_max_blocks(0)
        assert torch.equal(_bits(g), _bits(want_g))
        if skip:
            assert torch.equal(_bits(w), _bits(w0)) and torch.equal(_bits(m), _bits(m0))
            assert torch.equal(_bits(sh), _bits(w0.bfloat16()))
        else:
            w2, g2, m2 = w0.clone(), g0.clone(), m0.clone()
            C().lion_step(w2, g2, m2, None, hp, GS, B1, B2, WD, clip=st)       # the same step without ranges
            assert torch.equal(_bits(w), _bits(w2)) and torch.equal(_bits(m), _bits(m2))
            assert torch.equal(_bits(g2), _bits(g0)) and not torch.equal(w, w0)
    # one range, and a skipped step that asks for none: the gradient stays
    w, g, m = w0.clone(), g0.clone(), m0.clone()
    C().lion_step(w, g, m, None, hp, GS, B1, B2, WD, zero_ranges=[(0, n)], clip=st)
    assert bool((g == 0).all())
    if skip:
        g = g0.clone()
        C().lion_step(w, g, m, None, hp, GS, B1, B2, WD, clip=st)
        assert torch.equal(_bits(g), _bits(g0)) and torch.equal(_bits(w), _bits(w0))


# ---------------------------------------------------------------- 4. clip state
def test_clip_coefficient_scales_the_gradient_and_the_skip_flag_stops_the_step():
    n = N_MAIN
    w0, g0, m0 = _bufs(n, 23)
    hp = torch.tensor([LR, 0.0], device="cuda")
    st = torch.zeros(8, device="cuda")
    st[COEF] = 0.25
    a = [t.clone() for t in (w0, g0, m0)] + [w0.bfloat16()]
    b = [t.clone() for t in (w0, g0, m0)] + [w0.bfloat16()]
    C().lion_step(a[0], a[1], a[2], a[3], hp, GS, B1, B2, WD, clip=st)
    C().lion_step(b[0], b[1], b[2], b[3], hp, GS * 0.25, B1, B2, WD)       # (0.5 * 0.25 is exact)
    for x, y in zip(a, b):
        assert torch.equal(_bits(x), _bits(y))
    _, rm, _ = _ref64(w0.double(), g0.double(), m0.double(), LR, B1, B2, WD, GS * 0.25)
    torch.testing.assert_close(a[2].double(), rm, rtol=1e-5, atol=1e-6)
    assert not torch.equal(a[0], w0)
    st[SKIP] = 1.0
    d = [t.clone() for t in (w0, g0, m0)] + [w0.bfloat16()]
    C().lion_step(d[0], d[1], d[2], d[3], hp, GS, B1, B2, WD, clip=st)
    for x, y in zip(d, (w0, g0, m0, w0.bfloat16())):
        assert torch.equal(_bits(x), _bits(y))


# ---------------------------------------------------------------- 5. binding refusals
def test_binding_refusals_leave_the_buffers_alone():
    n = 4096
    w, g, m = _bufs(n, 24)
    sh = w.bfloat16()
    keep = [t.clone() for t in (w, g, m, sh)]
    hp = torch.tensor([LR, 0.0], device="cuda")
    st = torch.zeros(8, device="cuda")

    def call(**kw):
        a = dict(w=w, g=g, m=m, sh=sh, hp=hp, zero=[], clip=None)
        a.update(kw)
        C().lion_step(a["w"], a["g"], a["m"], a["sh"], a["hp"], GS, B1, B2, WD, zero_ranges=a["zero"], clip=a["clip"])

    for kw in (dict(m=m.double()), dict(g=g.half()), dict(w=w.double()),         # a wrong dtype
               dict(sh=sh.float()), dict(hp=hp.double()),
               dict(m=m.cpu()), dict(g=g.cpu()), dict(hp=hp.cpu()), dict(sh=sh.cpu()),   # a wrong device
               dict(clip=st.cpu()),
               dict(m=m[:-64]), dict(g=g[:-4]), dict(sh=sh[:-64]),                # mismatched lengths
               dict(hp=hp[:1]), dict(clip=st[:4]),                                # a short hp / clip state
               dict(m=m[1:], w=w[1:], g=g[1:], sh=sh[1:]),                        # not 16-byte aligned
               dict(m=torch.zeros(2 * n, device="cuda")[::2]),                    # not contiguous
               dict(zero=[(0, n + 1)]), dict(zero=[(5, 3)]), dict(zero=[(0, 1), (1, 2), (2, 3)])):
        with pytest.raises((RuntimeError, TypeError)):
            call(**kw)
    torch.cuda.synchronize()
    for t, k in zip((w, g, m, sh), keep):
        assert torch.equal(_bits(t), _bits(k))
    call()
    assert not torch.equal(w, keep[0])


# ---------------------------------------------------------------- 6. launch budget
_HOST_QUERIES = ("grad_sumsq_parts", "seg_sumsq_chunk")
_KW = (("clip", "clip"), ("ext", "ext"), ("sums_out", "sums_out"), ("zero_ranges", "zero"))
_SCHED = dict(kind="cosine", total_steps=100, warmup_steps=5)

CONFIGS = {
    "lion": (lambda p: Lion(p, lr=1e-3, weight_decay=1e-2), {}),
    "lion_clip": (lambda p: Lion(p, lr=1e-3, weight_decay=1e-2, max_grad_norm=1.0), {}),
    "lion_clear": (lambda p: Lion(p, lr=1e-3), {"clear_grads": True}),
    "lion_ema": (lambda p: Lion(p, lr=1e-3, ema_decay=0.99), {}),
    "lion_all": (lambda p: Lion(p, lr=1e-3, max_grad_norm=1.0, ema_decay=0.99, lr_schedule=_SCHED), {}),
}
UNSHARDED = {
    "lion": ["lion_step"],
    "lion_clip": ["grad_sumsq", "clip_finalize", "lion_step[clip]"],
    "lion_clear": ["lion_step[zero]"],
    "lion_ema": ["ema_begin", "lion_step", "ema_update"],
    "lion_all": ["grad_sumsq", "clip_finalize", "lr_sched[clip]", "ema_begin[clip]", "lion_step[clip]", "ema_update"],
}


class _Recorder:
    """Stands in for the native module: forwards every call, logs launches per thread (as
    tests/test_lamb_gpu.py's does)."""

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


def _record_step(rec, opt, kw):
    """One warm-up step, then the calls of the next one."""
    f = _flat(opt)
    _fill_grad(f, 1)
    opt.step(**kw)
    _fill_grad(f, 2)
    rec.take()
    opt.step(**kw)
    return rec.take()


@pytest.mark.parametrize("name", list(CONFIGS))
def test_unsharded_step_launches(rec, name):
    """One lion_step: no bump_step, no norm kernels without clipping, one ema_update more with the EMA."""
    mk, kw = CONFIGS[name]
    opt = mk(_model().parameters())
    assert _record_step(rec, opt, kw) == UNSHARDED[name]
    ls = opt._ls()
    assert "exp_avg" in ls and "exp_avg_sq" not in ls and float(ls["hp"][1]) == 0.0
    # the saved step count is the host's (hp[1] is never bumped), with clipping too
    assert opt.state_dict()["ldnn_flat_state"]["step"] == 2
    assert opt.supports_ranges() == ("clip" not in name and name != "lion_all")


def test_range_updates_equal_the_whole_step(rec):
    """``range_updater()``: one lion_step per range, and the same bits as the whole-buffer step."""
    ma, mb = _model(), _model()
    oa, ob = (Lion(m.parameters(), lr=1e-3, weight_decay=1e-2) for m in (ma, mb))
    fa, fb = _flat(oa), _flat(ob)
    for seed in (1, 2):
        _fill_grad(fa, seed)
        _fill_grad(fb, seed)
        oa.step()
        rec.take()
        s = ob.range_updater()
        assert s is not None
        cut = (fb.numel // 2) // 64 * 64
        s.update(0, cut)
        s.update(cut, fb.numel)
        s.end()
        assert rec.take() == ["lion_step", "lion_step"]
    torch.cuda.synchronize()
    assert torch.equal(fa.master, fb.master) and torch.equal(oa._ls()["exp_avg"], ob._ls()["exp_avg"])
    assert torch.equal(fa.shadow, fb.shadow) and ob._ls()["step"] == 2


def _state_ids(opt):
    return {k: id(v) for k, v in opt._ls().items() if torch.is_tensor(v)}


@pytest.mark.parametrize("name", list(CONFIGS))
def test_captured_step_issues_the_eager_calls_and_allocates_nothing(rec, name):
    mk, kw = CONFIGS[name]
    opt = mk(_model().parameters())
    f = _flat(opt)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        eager = _record_step(rec, opt, kw)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    before = _state_ids(opt)
    assert "exp_avg" in before and "hp" in before
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
    opt = CONFIGS["lion"][0](_model().parameters())
    _fill_grad(_flat(opt), 1)
    opt._ldnn_capturing = True
    with pytest.raises(RuntimeError, match="run an eager optimizer step before capturing"):
        opt.step()
    assert "lion_step" not in rec.take() and "hp" not in opt._ls()


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


def test_graphed_step_with_lion_matches_eager():
    """LeNet-5, batch 8, Lion without weight decay: 4 replays == 4 eager steps, judged against the
    spread of two eager runs as tests/test_lamb_gpu.py::test_graphed_step_with_lamb_matches_eager
    judges it.  Without weight decay every element of a step moves by 0 or by exactly the rate in
    force (within one fp32 ulp of the weight), so the rate a replay applied can be read off its
    update: the lr made 10x smaller between replays 2 and 3 is the one replay 3 applies."""
    lr = 1e-3
    m1, m2, m3 = _models("lenet5", 3)
    o1, o2, o3 = (Lion(m.parameters(), lr=lr) for m in (m1, m2, m3))
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
        rate = torch.tensor(lr if i < 3 else lr / 10, device="cuda")        # (fp32, as hp[0] holds it)
        after = f1.master
        d = (after.double() - before.double()).abs()
        big = torch.maximum(after.abs(), before.abs())
        ulp = (torch.nextafter(big, torch.full_like(big, float("inf"))) - big).double()
        moved = d != 0
        assert int(moved.sum()) > f1.numel // 4, i
        off = (d - rate.double()).abs()[moved]
        assert bool((off <= ulp[moved]).all()), (i, off.max().item())
    torch.cuda.synchronize()
    worst = 0.0
    for (n, p), (_, q), (_, s), r in zip(m1.named_parameters(), m2.named_parameters(), m3.named_parameters(), p0):
        d1, d2, d3 = ((t.detach() - r).flatten().double() for t in (p, q, s))
        eg, ee = (d1 - d2).norm().item(), (d3 - d2).norm().item()
        worst = max(worst, eg / d2.norm().item())
        assert eg <= 3.0 * ee + 2e-3 * d2.norm().item(), (n, eg, ee, d2.norm().item())
    print(f"graphed Lion vs eager: worst relative update distance {worst:.3e}")


@pytest.mark.parametrize("clip", [None, 0.5])
def test_graphed_dp_world1_lion_equals_single_process(clip):
    """GraphedDPStep on a world-1 comm, shard_optimizer on and off, == the single-process graphed
    step, with the odd-batch eager fallback; tolerance of
    tests/test_lamb_gpu.py::test_graphed_dp_world1_lamb_equals_single_process."""
    shape = (128, 1, 28, 28)
    m1, m2, m3 = _models("lenet5", 3)
    crit = CrossEntropyLoss()
    dps = [DataParallel(m1, LocalComm(), bucket_cap_mb=0.05, broadcast_init=False, shard_optimizer=True),
           DataParallel(m2, LocalComm(), bucket_cap_mb=0.05, broadcast_init=False)]
    opts = [Lion(m.parameters(), lr=1e-4, weight_decay=1e-2, max_grad_norm=clip) for m in (m1, m2, m3)]
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
    if clip is not None:
        cs = [{k: v.item() for k, v in o.grad_clip_stats().items()} for o in opts]
        assert cs[0]["steps"] == cs[1]["steps"] == cs[2]["steps"] == 5 and cs[0]["skipped"] == 0
    for o in opts:
        assert float(o._ls()["hp"][1]) == 0.0 and "exp_avg_sq" not in o._ls()
    for ma in (m1, m2):
        for a, b, r in zip(ma.parameters(), m3.parameters(), p0):
            da, db = (a.detach() - r).double(), (b.detach() - r).double()
            assert db.norm().item() > 0
            assert (da - db).norm().item() <= 2e-2 * db.norm().item() + 1e-6


@pytest.mark.parametrize("clip", [None, "0.5"])
def test_graphed_dp_two_ranks_gloo_with_lion(clip):
    """2 gloo ranks sharing the GPU (scripts/check_graphed_dp.py --optimizer lion --shard [--clip]):
    the graphed sharded Lion step == ONE graphed rank on the concatenated batches == the unsharded
    run, the schedule check passes, replicas identical."""
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.join(ROOT, "scripts", "check_graphed_dp.py"), "--optimizer", "lion",
           "--shard"] + (["--clip", clip] if clip else [])
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    assert "GRAPHED_DP_OK" in r.stdout, r.stdout[-3000:]
