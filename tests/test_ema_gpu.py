"""Weight EMA on the GPU: the three kernels (``ema_begin`` / ``ema_update`` / ``ema_swap``) against
float64 and bit patterns, the bindings' refusals, the flat optimizers with the EMA on (eager,
sharded, captured, ``GraphedStep`` / ``GraphedDPStep``), the launch budget, and a forward under
``ema_weights()``.

Bound (as tests/test_ema.py): after ``T`` updates ``T * 2**-22 * M`` absolute against the float64
EMA of the read-back masters, ``M`` the largest magnitude a master or average element reaches.  Each
check prints its worst error and the bound (``EMA_ERR ...``) before it asserts.

The flat buffer of the MLP 70-33-10 is a multiple of 64 elements and so is every range the sharded
step cuts it into (asserted below): the layout produces no range whose length is not a multiple of
4, so the scalar tail of ``ema_update`` is covered by the kernel-level sizes (67, 193, 4101, ...)
only."""
import threading

import pytest
import torch

import ldnn
from ldnn.models import CrossEntropyLoss
from ldnn.models.mlp import MLP
from ldnn.ops import _ext
from ldnn.optim import SGD, Adam, AdamW, Lamb
from ldnn.optim.optimizers import _CAPTURE_MSG, _Lars
from ldnn.parallel.comm import FakeWorld
from ldnn.parallel.ddp import DataParallel
from ldnn.train.graphed import GraphedDPStep, GraphedStep

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -22
_DECAY, _WARMUP, _UPDATES, _ALPHA = 0, 1, 2, 3     # the header's slots (ldnn_kernels.h EmaSlot)
_HOST_QUERIES = ("grad_sumsq_parts", "seg_sumsq_chunk")
_KW = (("clip", "clip"), ("lars", "lars"), ("ext", "ext"), ("sums_out", "sums_out"), ("zero_ranges", "zero"))
_UPDATES_CALLS = ("sgd_step", "adam_step", "lamb_apply")


def report(name, err, bound):
    print(f"EMA_ERR {name} worst_abs_err={err:.3e} bound={bound:.3e}")


def sweep():
    """Elements one full grid sweep of the flat kernels covers: the binding's grid rule caps the
    grid (``grad_sumsq_parts`` reports it), 256 threads a workgroup, one float4 a thread."""
    return _ext.C().grad_sumsq_parts(1 << 40) * 256 * 4


def bits(t):
    return t.view(torch.int32 if t.element_size() == 4 else torch.int16)


def alpha(d, warmup, c):
    return max(1 - d, 9 / (10 + c)) if warmup else 1 - d


def ema64(start, masters, d, warmup):
    e = start.double().clone()
    M = float(e.abs().max())
    for c, w in enumerate(masters):
        e += alpha(d, warmup, c) * (w.double() - e)
        M = max(M, float(w.abs().max()), float(e.abs().max()))
    return e, M


def assert_ema(name, e, start, masters, d, warmup):
    ref, M = ema64(start, masters, d, warmup)
    err, bound = float((e.double() - ref).abs().max()), len(masters) * EPS * M
    report(name, err, bound)
    assert err <= bound
    assert not torch.equal(e, masters[-1]) and not torch.equal(e, start)


def hdr(d=0.0, warmup=0.0, c=0.0, a=0.0):
    return torch.tensor([d, warmup, c, a], dtype=torch.float32, device="cuda")


# ---- kernels -------------------------------------------------------------------------------
def _sizes():
    return [4, 67, 193, 4101, sweep() + 4101]


@pytest.mark.parametrize("a_t", [0.1, 2.0 ** -10])
@pytest.mark.parametrize("off", [0, 64])
def test_ema_update_against_float64(off, a_t):
    g = torch.Generator(device="cuda").manual_seed(7)
    worst = 0.0
    for n in _sizes():
        wbuf = torch.full((n + 192,), float("nan"), device="cuda")
        ebuf = torch.full((n + 192,), float("nan"), device="cuda")
        w, e = wbuf[off: off + n], ebuf[off: off + n]
        w.copy_(torch.randn(n, device="cuda", generator=g))
        e.copy_(torch.randn(n, device="cuda", generator=g))
        w0, e0, before = wbuf.clone(), e.clone(), bits(ebuf).clone()
        h = hdr(0.9, 0, 3, a_t)
        _ext.C().ema_update(w, e, h)
        a = float(h[_ALPHA])                       # (a_t as fp32 holds it)
        ref = e0.double() + a * (w.double() - e0.double())
        M = max(float(w.abs().max()), float(e0.abs().max()), float(ref.abs().max()))
        err = float((e.double() - ref).abs().max())
        worst = max(worst, err / (EPS * M))
        assert err <= EPS * M, (n, err, EPS * M)
        assert not torch.equal(e, e0)
        # the sentinels around the view, and the master, bit for bit
        outside = torch.ones(n + 192, dtype=torch.bool, device="cuda")
        outside[off: off + n] = False
        assert torch.equal(bits(ebuf)[outside], before[outside]) and bool(ebuf[outside].isnan().all())
        assert torch.equal(bits(wbuf), bits(w0))
        assert torch.equal(h, hdr(0.9, 0, 3, a_t))
        # a_t = 0 (a skipped step): nothing moves
        now = bits(ebuf).clone()
        _ext.C().ema_update(w, e, hdr(0.9, 0, 3, 0.0))
        assert torch.equal(bits(ebuf), now)
    report(f"ema_update[off={off},a_t={a_t:g}] (in units of the one-step bound)", worst, 1.0)


def test_ema_begin_counts_and_warms_up():
    C = _ext.C()
    h = hdr(0.5, 1)
    worst = 0.0
    for c in range(12):
        C.ema_begin(h)
        want = alpha(0.5, True, c)
        assert float(h[_UPDATES]) == c + 1
        rel = abs(float(h[_ALPHA]) - want) / want
        worst = max(worst, rel)
        assert rel <= EPS, (c, float(h[_ALPHA]), want)
    assert float(h[_ALPHA]) == 0.5                 # the warm-up handed over to d (at c = 8)
    report("ema_begin a_t (relative)", worst, EPS)
    # a skipped step: c stays, a_t = 0; an unskipped clip state counts
    clip = torch.zeros(8, device="cuda")
    clip[2] = 1.0
    C.ema_begin(h, clip=clip)
    assert float(h[_UPDATES]) == 12 and float(h[_ALPHA]) == 0.0
    clip[2] = 0.0
    C.ema_begin(h, clip=clip)
    assert float(h[_UPDATES]) == 13 and float(h[_ALPHA]) == 0.5
    assert float(h[_DECAY]) == 0.5 and float(h[_WARMUP]) == 1.0
    # warm-up off: the fp32 value of 1 - d every time
    h = hdr(0.999, 0)
    want = float(torch.tensor(1.0) - torch.tensor(0.999, dtype=torch.float32))
    for c in range(3):
        C.ema_begin(h)
        assert float(h[_ALPHA]) == want and float(h[_UPDATES]) == c + 1


@pytest.mark.parametrize("with_shadow", [True, False])
def test_ema_swap_is_an_exact_exchange(with_shadow):
    g = torch.Generator(device="cuda").manual_seed(8)
    for n in (4101, sweep() + 4101):
        w = torch.randn(n, device="cuda", generator=g)
        e = torch.randn(n, device="cuda", generator=g)
        w[5], e[6], w[n - 1] = float("nan"), float("-inf"), -0.0      # (bit patterns, not values)
        sh = w.to(torch.bfloat16) if with_shadow else None
        w0, e0, s0 = w.clone(), e.clone(), (sh.clone() if with_shadow else None)
        if with_shadow:
            _ext.C().ema_swap(w, e, sh)
        else:
            _ext.C().ema_swap(w, e)
        assert torch.equal(bits(w), bits(e0)) and torch.equal(bits(e), bits(w0))
        if with_shadow:
            assert torch.equal(bits(sh), bits(e0.to(torch.bfloat16)))
        _ext.C().ema_swap(w, e, shadow=sh)
        assert torch.equal(bits(w), bits(w0)) and torch.equal(bits(e), bits(e0))
        if with_shadow:
            assert torch.equal(bits(sh), bits(s0))


def test_bindings_refuse_bad_buffers():
    C = _ext.C()
    buf = torch.zeros(260, device="cuda")
    w, e, h = buf[:128], torch.zeros(128, device="cuda"), hdr(0.9, 0, 0, 0.1)
    for fn, extra in ((C.ema_update, (h,)), (C.ema_swap, ())):
        with pytest.raises(RuntimeError, match="dtype"):
            fn(w.double(), e, *extra)
        with pytest.raises(RuntimeError, match="dtype"):
            fn(w, e.to(torch.bfloat16), *extra)
        with pytest.raises(RuntimeError, match="equally long"):
            fn(w, e[:124], *extra)
        with pytest.raises(RuntimeError, match="16-byte aligned"):
            fn(buf[1:129], e, *extra)
        with pytest.raises(RuntimeError, match="16-byte aligned"):
            fn(w, torch.zeros(132, device="cuda")[1:129], *extra)
        with pytest.raises(RuntimeError, match="contiguous"):
            fn(buf[:256:2], e, *extra)
    with pytest.raises(RuntimeError, match="hdr"):
        C.ema_update(w, e, h[:3])
    with pytest.raises(RuntimeError, match="hdr"):
        C.ema_begin(h[:3])
    with pytest.raises(RuntimeError, match="bad shadow"):
        C.ema_swap(w, e, torch.zeros(64, dtype=torch.bfloat16, device="cuda"))
    assert not buf.any() and not e.any()


# ---- optimizers ------------------------------------------------------------------------------
EMA = dict(ema_decay=0.5)     # (warm-up on: it hands over to d at c = 8; the graphed tests pass it)
CONFIGS = {
    "sgd_momentum": (lambda p, **k: SGD(p, lr=0.05, momentum=0.9, **k), {}),
    "sgd_clip_lars": (lambda p, **k: SGD(p, lr=0.05, momentum=0.9, weight_decay=1e-4, max_grad_norm=1.0,
                                         lars_trust=0.02, **k), {}),
    "adam": (lambda p, **k: Adam(p, lr=1e-3, **k), {}),
    "adamw_clear": (lambda p, **k: AdamW(p, lr=1e-3, **k), {"clear_grads": True}),
    "lamb": (lambda p, **k: Lamb(p, lr=1e-3, weight_decay=0.01, **k), {}),
}
# the parent's sequences (tests/test_optim_launches_gpu.py, tests/test_lamb_gpu.py), as literals
UNSHARDED = {
    "sgd_momentum": ["sgd_step"],
    "sgd_clip_lars": ["grad_sumsq", "clip_finalize", "seg_sumsq", "lars_finalize[clip]", "sgd_step[clip,lars]"],
    "adam": ["bump_step", "adam_step"],
    "adamw_clear": ["bump_step", "adam_step[zero]"],
}
SHARDED = {
    "sgd_momentum": (["sgd_step"] * 3, ["sgd_step"] * 3, 0),
    "sgd_clip_lars": (["grad_sumsq"] * 3 + ["sumsq_total", "seg_sumsq", "lars_finalize[sums_out]",
                                            "clip_finalize[ext]", "lars_finalize[clip,ext]"]
                      + ["sgd_step[clip,lars]"] * 3,
                      ["grad_sumsq"] * 2 + ["sumsq_total", "seg_sumsq", "lars_finalize[sums_out]",
                                            "clip_finalize[ext]", "lars_finalize[clip,ext]"]
                      + ["sgd_step[clip,lars]"] * 3, 1),
    "adam": (["bump_step"] + ["adam_step"] * 3, ["bump_step"] + ["adam_step"] * 3, 0),
    "adamw_clear": (["bump_step"] + ["adam_step"] * 3, ["bump_step"] + ["adam_step"] * 3, 0),
}


def with_ema(parent):
    """The parent's sequence with ``ema_begin`` before the first update launch (it takes the clip
    state the updates take) and ``ema_update`` behind every update launch."""
    out, begun = [], False
    for c in parent:
        if c.split("[")[0] in _UPDATES_CALLS:
            if not begun:
                out.append("ema_begin[clip]" if "clip" in c else "ema_begin")
                begun = True
            out += [c, "ema_update"]
        else:
            out.append(c)
    return out


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


def _eager(name, ema, steps=6):
    mk, kw = CONFIGS[name]
    opt = mk(_model().parameters(), **(EMA if ema else {}))
    f = _flat(opt)
    start, masters = f.master.clone(), []
    for i in range(steps):
        _fill_grad(f, 10 + i)
        opt.step(**kw)
        masters.append(f.master.clone())
    return opt, f, start, masters


@pytest.mark.parametrize("name", list(CONFIGS))
def test_optimizer_ema_matches_float64_and_changes_nothing_else(name):
    on, f, start, masters = _eager(name, True)
    off, f_off, _, masters_off = _eager(name, False)
    assert f.numel % 64 == 0        # (no update range with a length that is not a multiple of 4)
    assert_ema(f"optimizer[{name}]", on._ls()["ema"], start, masters, 0.5, True)
    assert int(on.ema_stats()["updates"]) == 6
    assert float(on.ema_stats()["a_last"]) == pytest.approx(alpha(0.5, True, 5), rel=EPS)
    for a, b in zip(masters, masters_off):
        assert torch.equal(a, b)
    assert torch.equal(f.shadow, f_off.shadow)
    n = 0
    for k in ("momentum", "exp_avg", "exp_avg_sq"):
        if k in off._ls():
            assert torch.equal(on._ls()[k], off._ls()[k]), k
            n += 1
    assert n and off.ema_stats() is None and "ema" not in off._ls() and "ema_hdr" not in off._ls()
    # padding and alignment gaps are zero in the master and stay zero in the average
    used = torch.zeros(f.numel, dtype=torch.bool, device="cuda")
    for s in f.segments:
        used[s.offset: s.offset + s.storage_numel] = True
    if name == "sgd_momentum":      # (a zero gradient there: the random fill above moved the others' padding)
        opt = CONFIGS[name][0](_model().parameters(), **EMA)
        f = _flat(opt)
        for i in range(3):
            _fill_grad(f, 30 + i)
            f.grad[~used] = 0
            opt.step()
        assert not f.master[~used].any() and not opt._ls()["ema"][~used].any()
        assert opt._ls()["ema"][used].any()


def test_skipped_step_on_the_device():
    opt = SGD(_model().parameters(), lr=0.05, momentum=0.9, max_grad_norm=1.0, **EMA)
    f = _flat(opt)
    for i in range(2):
        _fill_grad(f, 40 + i)
        opt.step()
    e = opt._ls()["ema"].clone()
    _fill_grad(f, 42)
    f.grad[77] = float("inf")
    opt.step()
    assert int(opt.grad_clip_stats()["skipped"]) == 1
    assert torch.equal(opt._ls()["ema"], e)
    assert int(opt.ema_stats()["updates"]) == 2 and float(opt.ema_stats()["a_last"]) == 0.0
    _fill_grad(f, 43)
    opt.step()
    assert int(opt.ema_stats()["updates"]) == 3 and not torch.equal(opt._ls()["ema"], e)


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


@pytest.mark.parametrize("name", list(UNSHARDED))
def test_unsharded_launches(rec, name):
    mk, kw = CONFIGS[name]
    assert with_ema(UNSHARDED["adam"]) == ["bump_step", "ema_begin", "adam_step", "ema_update"]
    assert _record_step(rec, mk(_model().parameters(), **EMA), kw)[0] == with_ema(UNSHARDED[name])
    assert _record_step(rec, mk(_model().parameters()), kw)[0] == UNSHARDED[name]      # off: the parent's


def _sharded_rank(comm, rec, name):
    mk, kw = CONFIGS[name]
    m = _model()
    dp = DataParallel(m, comm, bucket_cap_mb=0.005, shard_optimizer=True)
    assert dp.sharded and [b["sharded"] for b in dp.bucketer.buckets] == [True, True, False]
    assert all(lo % 64 == 0 and hi % 64 == 0 for lo, hi in dp.bucketer.update_ranges())
    out = _record_step(rec, mk(m.parameters(), **EMA), kw, comm)
    dp.wait_gathers()
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("name", list(SHARDED))
def test_sharded_launches_and_no_extra_collective(rec, name):
    res = FakeWorld(2).run(_sharded_rank, rec, name)
    for r in range(2):
        assert res[r] == (with_ema(SHARDED[name][r]), SHARDED[name][2]), r
        assert res[r][0].count("ema_update") == 3 and res[r][0].count("ema_begin" + ("[clip]" if "clip" in name
                                                                                   else "")) == 1


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


@pytest.mark.parametrize("name", list(UNSHARDED))
def test_captured_step_issues_the_eager_calls_and_allocates_nothing(rec, name):
    mk, kw = CONFIGS[name]
    opt = mk(_model().parameters(), **EMA)
    f = _flat(opt)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        eager, _ = _record_step(rec, opt, kw)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    before = _state_ids(opt)
    assert "ema" in before and "ema_hdr" in before
    _fill_grad(f, 3)
    graph = torch.cuda.CUDAGraph()
    opt._ldnn_capturing = True
    try:
        with torch.cuda.graph(graph, stream=s):
            opt.step(**kw)
    finally:
        opt._ldnn_capturing = False
    assert rec.take() == eager == with_ema(UNSHARDED[name])
    assert _state_ids(opt) == before
    e, n = opt._ls()["ema"].clone(), int(opt.ema_stats()["updates"])
    graph.replay()
    torch.cuda.synchronize()
    assert not torch.equal(e, opt._ls()["ema"]) and int(opt.ema_stats()["updates"]) == n + 1


def test_capture_that_would_allocate_the_average_is_refused():
    opt = Adam(_model().parameters(), lr=1e-3)
    f = _flat(opt)
    _fill_grad(f, 1)
    opt.step()                                    # every other piece of device state exists now
    opt.param_groups[0]["ema_decay"] = 0.9
    opt._ldnn_capturing = True
    try:
        with pytest.raises(RuntimeError, match=_CAPTURE_MSG):
            opt.step()
    finally:
        opt._ldnn_capturing = False
    assert "ema" not in opt._ls() and "ema_hdr" not in opt._ls()
    # and with no eager step at all
    opt = Adam(_model().parameters(), lr=1e-3, **EMA)
    opt._ldnn_capturing = True
    try:
        with pytest.raises(RuntimeError, match=_CAPTURE_MSG):
            opt.step()
    finally:
        opt._ldnn_capturing = False
    assert not any(torch.is_tensor(v) for v in opt._ls().values())


# ---- graphed steps ---------------------------------------------------------------------------
def _batches(n, seed=5, B=16):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return ([torch.randn(B, 70, device="cuda", generator=g).bfloat16() for _ in range(n)],
            [torch.randint(0, 10, (B,), device="cuda", generator=g) for _ in range(n)])


def test_graphed_step_replays_the_average_and_follows_the_decay():
    m = _model()
    opt = Adam(m.parameters(), lr=1e-2, ema_decay=0.9, ema_warmup=False)
    f = _flat(opt)
    xs, ys = _batches(7)
    start = f.master.clone()
    gs = GraphedStep(m, CrossEntropyLoss(), opt, xs[0], ys[0], warmup=1)     # one eager step, then the capture
    torch.cuda.synchronize()
    masters = [f.master.clone()]
    for i in range(1, 6):
        gs(xs[i], ys[i])
        torch.cuda.synchronize()
        masters.append(f.master.clone())
    assert_ema("GraphedStep", opt._ls()["ema"], start, masters, 0.9, False)
    st = opt.ema_stats()
    assert int(st["updates"]) == 6
    assert float(st["a_last"]) == float(torch.tensor(1.0) - torch.tensor(0.9, dtype=torch.float32))
    opt.param_groups[0]["ema_decay"] = 0.5
    e = opt._ls()["ema"].clone()
    gs(xs[6], ys[6])
    torch.cuda.synchronize()
    assert float(opt.ema_stats()["a_last"]) == 0.5 and int(opt.ema_stats()["updates"]) == 7
    ref = e.double() + 0.5 * (f.master.double() - e.double())
    M = max(float(ref.abs().max()), float(f.master.abs().max()), float(e.abs().max()))
    assert float((opt._ls()["ema"].double() - ref).abs().max()) <= EPS * M


_CAPTURE_LOCK = threading.Lock()


def _graphed_dp_rank(comm):
    m = _model()
    dp = DataParallel(m, comm, bucket_cap_mb=0.005, shard_optimizer=True)
    assert dp.sharded and len(dp.bucketer.buckets) == 3
    f = dp.flat
    opt = SGD(m.parameters(), lr=0.05, momentum=0.9, **EMA)
    xs, ys = _batches(5, seed=50 + comm.rank)
    crit = CrossEntropyLoss()
    start = f.master.clone()
    # the eager step that allocates the state, on a filled-in gradient (the same on both ranks, as
    # a reduced one is): an eager backward would issue its bucket collectives from the autograd
    # engine's one device thread, which the two rank threads share
    _fill_grad(f, 6)
    opt.step()
    dp.gather_master(opt)
    torch.cuda.synchronize()
    masters = [f.master.clone()]
    with _CAPTURE_LOCK:                          # (the ranks are threads: one capture at a time)
        gd = GraphedDPStep(dp, crit, opt, xs[0], ys[0])
        torch.cuda.synchronize()
    for i in range(1, 5):
        gd(xs[i], ys[i])
        dp.gather_master(opt)
        torch.cuda.synchronize()
        masters.append(f.master.clone())
    return start, masters, opt._ls()["ema"].clone(), int(opt.ema_stats()["updates"])


def test_graphed_dp_two_ranks_sharded_average():
    res = FakeWorld(2).run(_graphed_dp_rank)
    (start, masters, e0, n0), (_, masters1, e1, n1) = res
    assert n0 == n1 == 5
    assert torch.equal(e0, e1) and torch.equal(masters[-1], masters1[-1])
    assert_ema("GraphedDPStep[2 ranks, sharded]", e0, start, masters, 0.5, True)


def test_forward_under_ema_weights():
    m = _model()
    opt = Adam(m.parameters(), lr=1e-2, **EMA)
    f = _flat(opt)
    xs, ys = _batches(4, seed=9)
    crit = CrossEntropyLoss()
    for x, y in zip(xs[:3], ys[:3]):
        opt.zero_grad()
        crit(m(x), y).backward()
        opt.step()
    m.eval()
    with torch.no_grad():
        live = m(xs[3]).clone()
        master, shadow = f.master.clone(), f.shadow.clone()
        with opt.ema_weights():
            out = m(xs[3]).clone()
            avg = f.master.clone()
            assert torch.equal(opt._ls()["ema"], master)       # (the live weights wait in the EMA buffer)
        again = m(xs[3]).clone()
    assert torch.equal(bits(f.master), bits(master)) and torch.equal(bits(f.shadow), bits(shadow))
    assert torch.equal(avg, opt._ls()["ema"])
    m2 = MLP(70, (33,), 10)
    f2 = ldnn.prepare(m2, "cuda")
    f2.master.copy_(avg)
    f2.refresh_shadow()
    m2.eval()
    with torch.no_grad():
        ref = m2(xs[3])
    assert torch.equal(bits(out), bits(ref))
    assert torch.equal(bits(again), bits(live)) and not torch.equal(out, live)
