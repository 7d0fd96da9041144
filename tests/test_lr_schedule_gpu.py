"""Per-step learning-rate schedule on the GPU: ``lr_sched`` against the float64 closed form, the
flat optimizers under the device schedule against runs whose rate the test sets by hand (bit for
bit), ``GraphedStep`` replays that follow the schedule with no host write, and a step skipped on
the device.

Kernel bound: ``|s_dev - s_ref64| <= 1e-6`` absolute.  The factor is at most 1 and is built from
fewer than ten fp32 roundings (2**-24 relative each) plus one ``cospif`` / ``powf``, so a few 1e-7
are expected; the reference takes the header's constants as fp32 holds them.  Each check prints its
worst error and the bound (``LR_SCHED_ERR ...``) before it asserts."""
import math

import pytest
import torch

import ldnn
from ldnn.models import CrossEntropyLoss, build_model, xavier_init
from ldnn.models.mlp import MLP
from ldnn.ops import _ext
from ldnn.optim import SGD, Adam, Lamb
from ldnn.train.graphed import GraphedStep

pytestmark = pytest.mark.gpu

BOUND = 1e-6
KIND, WARM, START, TOTAL, MIN, POWER, BASE, STEPS, FACTOR, LEN = range(10)   # ldnn_kernels.h SchedSlot
CODES = {"constant": 0, "poly": 1, "linear": 1, "cosine": 2}


def report(name, err, bound):
    print(f"LR_SCHED_ERR {name} worst_abs_err={err:.3e} bound={bound:.3e}")


def ref64(kind, u, W, T, ws, m, q):
    if u <= W:
        return ws + (1 - ws) * u / W
    if kind == "constant":
        return 1.0
    p = min(1.0, (u - W) / (T - W))
    if kind == "cosine":
        return m + (1 - m) * 0.5 * (1 + math.cos(math.pi * p))
    return m + (1 - m) * (1 - p) ** q


def header(kind, W, T, ws=0.0, m=0.0, q=2.0, base=1.0, t=0.0):
    q = 1.0 if kind == "linear" else q
    return torch.tensor([CODES[kind], W, ws, T, m, q, base, t, 0.0], dtype=torch.float32, device="cuda")


def sched(kind, W, T, **kw):
    return dict(kind=kind, total_steps=T, warmup_steps=W, **kw)


# ---- the kernel ----------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["constant", "linear", "poly", "cosine"])
@pytest.mark.parametrize("ws,m,q,base", [(0.0, 0.0, 2.0, 1.0), (0.1, 0.05, 1.7, 0.3)])
def test_lr_sched_against_float64(kind, ws, m, q, base):
    C = _ext.C()
    h = header(kind, 3, 8, ws, m, q, base)
    hp = torch.tensor([-1.0, 5.0], device="cuda")
    consts = h[:BASE + 1].clone()
    ws32, m32, q32, base32 = (float(h[i]) for i in (START, MIN, POWER, BASE))
    worst = 0.0
    for u in range(1, 12):
        C.lr_sched(h, hp)
        s_dev, want = float(h[FACTOR]), ref64(kind, u, 3, 8, ws32, m32, q32)
        worst = max(worst, abs(s_dev - want))
        assert float(h[STEPS]) == u
        # hp[0] is the fp32 product of base and the factor; the Adam step count beside it is untouched
        assert float(hp[0]) == float(torch.tensor(base32, dtype=torch.float32) * torch.tensor(s_dev, dtype=torch.float32))
        assert float(hp[1]) == 5.0
        if u == 3:
            assert s_dev == 1.0                     # the last warm-up step: exactly the base
    report(f"lr_sched[{kind},ws={ws},m={m},q={q}]", worst, BOUND)
    assert worst <= BOUND
    assert s_dev == (1.0 if kind == "constant" else m32)     # beyond the horizon: the floor
    assert torch.equal(h[:BASE + 1], consts)
    # a skipped step: count, factor and rate stay; a clear flag counts again
    clip = torch.zeros(8, device="cuda")
    clip[2] = 1.0
    before, lr = h.clone(), float(hp[0])
    C.lr_sched(h, hp, clip=clip)
    assert torch.equal(h, before) and float(hp[0]) == lr
    clip[2] = 0.0
    C.lr_sched(h, hp, clip=clip)
    assert float(h[STEPS]) == 12 and float(h[FACTOR]) == s_dev
    assert bool((clip == 0).all())


def test_lr_sched_without_warmup_and_resumed():
    C = _ext.C()
    worst = 0.0
    for kind in ("linear", "poly", "cosine"):
        h, hp = header(kind, 0, 5, t=2.0), torch.zeros(2, device="cuda")      # (a count a checkpoint restored)
        for u in range(3, 8):
            C.lr_sched(h, hp)
            worst = max(worst, abs(float(hp[0]) - ref64(kind, u, 0, 5, 0.0, 0.0, 2.0 if kind == "poly" else 1.0)))
        assert float(h[STEPS]) == 7 and float(hp[0]) == 0.0
    report("lr_sched[W=0, from t=2]", worst, BOUND)
    assert worst <= BOUND


def test_binding_refuses_bad_arguments():
    C = _ext.C()
    h, hp = header("cosine", 3, 8), torch.zeros(2, device="cuda")
    for bad_h, bad_hp, clip in ((h[:LEN - 2], hp, None), (h.double(), hp, None), (h.cpu(), hp, None),
                                (h, hp[:1], None), (h, hp.cpu(), None), (h, hp.double(), None),
                                (torch.zeros(2 * LEN, device="cuda")[::2], hp, None),
                                (h, hp, torch.zeros(4, device="cuda")), (h, hp, torch.zeros(8))):
        with pytest.raises(RuntimeError):
            C.lr_sched(bad_h, bad_hp, clip=clip)
    assert float(h[STEPS]) == 0


# ---- the optimizers, bit for bit ------------------------------------------------------------
SCHED = sched("cosine", 3, 8, warmup_start=0.1, min_ratio=0.05)
CONFIGS = {
    "sgd": lambda p, **kw: SGD(p, lr=0.05, momentum=0.9, weight_decay=1e-3, **kw),
    "adam": lambda p, **kw: Adam(p, lr=1e-3, **kw),
    "lamb": lambda p, **kw: Lamb(p, lr=1e-2, weight_decay=0.01, **kw),
    "lars_clip": lambda p, **kw: SGD(p, lr=0.05, momentum=0.9, weight_decay=1e-4, lars_trust=0.02,
                                     max_grad_norm=1.0, **kw),
}
STATE_KEYS = ("momentum", "exp_avg", "exp_avg_sq")


def _mlp():
    torch.manual_seed(0)
    m = MLP(70, (33,), 10)
    return m, ldnn.prepare(m, "cuda")


@pytest.fixture(scope="module")
def flat_grads():
    _, f = _mlp()
    g = torch.Generator(device="cuda").manual_seed(11)
    return [torch.randn(f.numel, device="cuda", generator=g) for _ in range(11)]


@pytest.mark.parametrize("name", list(CONFIGS))
def test_optimizer_equals_rate_set_by_hand(name, flat_grads):
    ma, fa = _mlp()
    a = CONFIGS[name](ma.parameters(), lr_schedule=SCHED)
    base, start, lrs = a.param_groups[0]["lr"], fa.master.clone(), []
    for u, g in enumerate(flat_grads, 1):
        fa.grad.copy_(g)
        a.step()
        st = a.lr_schedule_stats()
        lrs.append(float(st["lr"]))
        assert int(st["steps"]) == u and a.param_groups[0]["lr"] == base
    want = [base * ref64("cosine", u, 3, 8, 0.1, 0.05, 2.0) for u in range(1, 12)]
    err = max(abs(x - y) for x, y in zip(lrs, want)) / base
    report(f"optimizer[{name}] lr / base", err, BOUND)
    assert err <= BOUND and len(set(lrs)) == 8       # (7 distinct rates, then the floor)
    mb, fb = _mlp()
    b = CONFIGS[name](mb.parameters())
    for lr, g in zip(lrs, flat_grads):
        b.param_groups[0]["lr"] = lr
        fb.grad.copy_(g)
        b.step()
    assert torch.equal(fa.master, fb.master) and not torch.equal(fa.master, start)
    assert fa.shadow is not None and torch.equal(fa.shadow, fb.shadow)
    keys = [k for k in STATE_KEYS if k in a._ls()]
    assert keys and keys == [k for k in STATE_KEYS if k in b._ls()]
    for k in keys:
        assert torch.equal(a._ls()[k], b._ls()[k]), k
    assert a.state_dict()["ldnn_flat_state"]["sched_steps"] == 11
    assert b.lr_schedule_stats() is None and "sched_hdr" not in b._ls()


# ---- graphed steps -------------------------------------------------------------------------
def _lenets(n):
    ms = [build_model("lenet5") for _ in range(n)]
    xavier_init(ms[0])
    for m in ms[1:]:
        m.load_state_dict(ms[0].state_dict())
    for m in ms:
        ldnn.prepare(m, "cuda")
    return ms


def _batches(n, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    xs = [torch.randn(8, 1, 28, 28, device="cuda", generator=g).bfloat16() for _ in range(n)]
    ys = [torch.randint(0, 10, (8,), device="cuda", generator=g) for _ in range(n)]
    return xs, ys


def test_graphed_step_follows_the_schedule_without_host_writes():
    """LeNet-5, batch 8: one eager step, then 8 replays == 9 eager steps (two eager runs give the
    spread, as tests/test_lars_gpu.py::test_graphed_step_with_lars_matches_eager judges it).  The
    param groups stay untouched, yet the rate follows the closed form replay by replay; halving the
    base before replay 5, as StepLR does, is followed by that replay."""
    S = sched("cosine", 2, 8, min_ratio=0.1)
    m1, m2, m3 = _lenets(3)
    o1, o2, o3 = (SGD(m.parameters(), lr=0.05, momentum=0.9, lr_schedule=S) for m in (m1, m2, m3))
    crit = CrossEntropyLoss()
    xs, ys = _batches(9, 1)
    for m, o in ((m1, o1), (m2, o2), (m3, o3)):
        o.zero_grad()
        crit(m(xs[0]), ys[0]).backward()
        o.step()
    p0 = [q.detach().clone() for q in m2.parameters()]
    gs = GraphedStep(m1, crit, o1, xs[1], ys[1], warmup=0)
    groups = [dict(g, params=None) for g in o1.param_groups]
    worst, base = 0.0, 0.05
    for i in range(1, 9):
        if i == 5:
            base = 0.025
            for o in (o1, o2, o3):
                o.param_groups[0]["lr"] = base
            groups = [dict(g, params=None) for g in o1.param_groups]
        gs(xs[i], ys[i])
        for m, o in ((m2, o2), (m3, o3)):
            o.zero_grad()
            crit(m(xs[i]), ys[i]).backward()
            o.step()
        st = o1.lr_schedule_stats()
        assert int(st["steps"]) == i + 1
        worst = max(worst, abs(float(st["lr"]) / base - ref64("cosine", i + 1, 2, 8, 0.0, float(torch.tensor(0.1)), 2.0)))
        assert float(st["lr"]) == float(o2.lr_schedule_stats()["lr"])
        assert [dict(g, params=None) for g in o1.param_groups] == groups
    report("graphed lr / base", worst, BOUND)
    assert worst <= BOUND
    torch.cuda.synchronize()
    for (n, p), (_, q), (_, s), r in zip(m1.named_parameters(), m2.named_parameters(), m3.named_parameters(), p0):
        d1, d2, d3 = ((t.detach() - r).flatten().double() for t in (p, q, s))
        eg, ee = (d1 - d2).norm().item(), (d3 - d2).norm().item()
        assert eg <= 3.0 * ee + 2e-3 * d2.norm().item(), (n, eg, ee, d2.norm().item())
        assert d2.norm().item() > 0


def test_graphed_replay_issues_no_host_write(monkeypatch):
    """Between replays nothing is written from the host: ``fill_`` is not called at all while the
    base and the dict stand, and a changed base costs the one slot."""
    m1, = _lenets(1)
    o1 = SGD(m1.parameters(), lr=0.05, momentum=0.9, lr_schedule=sched("linear", 2, 8))
    crit = CrossEntropyLoss()
    xs, ys = _batches(4, 2)
    o1.zero_grad()
    crit(m1(xs[0]), ys[0]).backward()
    o1.step()
    gs = GraphedStep(m1, crit, o1, xs[1], ys[1], warmup=0)
    fills = []
    real = torch.Tensor.fill_
    monkeypatch.setattr(torch.Tensor, "fill_", lambda t, v: (fills.append(v), real(t, v))[1])
    gs(xs[1], ys[1])
    gs(xs[2], ys[2])
    assert fills == []
    o1.param_groups[0]["lr"] = 0.01
    gs(xs[3], ys[3])
    assert fills == [0.01]
    monkeypatch.undo()
    st = o1.lr_schedule_stats()
    assert int(st["steps"]) == 4
    assert abs(float(st["lr"]) / 0.01 - ref64("linear", 4, 2, 8, 0.0, 0.0, 1.0)) <= BOUND


def _gap_index(f):
    """A flat element between two segments: no backward writes it, the norm reads it."""
    segs = sorted(f.segments, key=lambda s: s.offset)
    for a, nxt in zip(segs, [b.offset for b in segs[1:]] + [f.numel]):
        if nxt > a.offset + a.storage_numel:
            return a.offset + a.storage_numel
    return None


def test_skipped_replay_is_not_counted():
    """Clipping on, one replay with an inf planted in the flat gradient buffer (in an alignment gap,
    which the captured backward does not overwrite and the norm reads): the step is skipped on the
    device, ``steps`` stays, and the next replay runs at the rate the skipped one would have used."""
    m1, = _lenets(1)
    o1 = SGD(m1.parameters(), lr=0.05, momentum=0.9, max_grad_norm=1.0, lr_schedule=sched("linear", 0, 10))
    f = o1._flat_for_group(o1.param_groups[0])
    crit = CrossEntropyLoss()
    xs, ys = _batches(4, 3)
    gap = _gap_index(f)
    assert gap is not None
    o1.zero_grad()
    crit(m1(xs[0]), ys[0]).backward()
    o1.step()
    gs = GraphedStep(m1, crit, o1, xs[1], ys[1], warmup=0)
    gs(xs[1], ys[1])
    torch.cuda.synchronize()
    st = o1.lr_schedule_stats()
    assert int(st["steps"]) == 2 and int(o1.grad_clip_stats()["skipped"]) == 0
    lr2, w = float(st["lr"]), f.master.clone()
    hdr = o1._ls()["sched_hdr"].clone()
    f.grad[gap] = float("inf")
    gs(xs[2], ys[2])
    torch.cuda.synchronize()
    if int(o1.grad_clip_stats()["skipped"]) == 0:
        pytest.fail("the planted inf did not reach the norm: the graph overwrites the gradient buffer")
    assert torch.equal(o1._ls()["sched_hdr"], hdr) and float(o1.lr_schedule_stats()["lr"]) == lr2
    assert torch.equal(f.master, w)
    f.grad[gap] = 0.0
    gs(xs[3], ys[3])
    torch.cuda.synchronize()
    st = o1.lr_schedule_stats()
    assert int(st["steps"]) == 3 and int(o1.grad_clip_stats()["skipped"]) == 1
    assert abs(float(st["lr"]) / 0.05 - ref64("linear", 3, 0, 10, 0.0, 0.0, 1.0)) <= BOUND
    assert float(st["lr"]) < lr2 and not torch.equal(f.master, w)


def test_graphed_dp_world1_sharded_schedules_like_the_single_process_step():
    """GraphedDPStep on a world-1 comm with the sharded optimizer: the captured chain's update link
    schedules like GraphedStep (same header, same kernel: the rates are equal bit for bit), the
    odd-batch eager fallback counts as a step, and the weights agree within the tolerance of
    tests/test_lars_gpu.py::test_graphed_dp_world1_lars_equals_single_process."""
    from ldnn.parallel.comm import LocalComm
    from ldnn.parallel.ddp import DataParallel
    from ldnn.train.graphed import GraphedDPStep

    S = sched("poly", 2, 6, min_ratio=0.1)
    shape = (128, 1, 28, 28)
    m1, m2 = _lenets(2)
    crit = CrossEntropyLoss()
    dp = DataParallel(m1, LocalComm(), bucket_cap_mb=0.05, broadcast_init=False, shard_optimizer=True)
    o1, o2 = (SGD(m.parameters(), lr=0.05, momentum=0.9, lr_schedule=S) for m in (m1, m2))
    g = torch.Generator(device="cuda").manual_seed(5)
    xs = [torch.randn(*shape, device="cuda", generator=g).bfloat16() for _ in range(4)]
    ys = [torch.randint(0, 10, (shape[0],), device="cuda", generator=g) for _ in range(4)]
    p0 = [p.detach().clone() for p in m2.parameters()]
    o1.zero_grad()
    crit(dp(xs[0]), ys[0]).backward()
    dp.finish_gradient_sync()
    o1.step()
    dp.wait_gathers()
    o2.zero_grad()
    crit(m2(xs[0]), ys[0]).backward()
    o2.step()
    gd = GraphedDPStep(dp, crit, o1, xs[0], ys[0])
    gs = GraphedStep(m2, crit, o2, xs[0], ys[0], warmup=0)
    batches = [(xs[i], ys[i]) for i in range(1, 4)] + [(xs[0][:50], ys[0][:50])]      # (the last: eager fallback)
    for u, (x, y) in enumerate(batches, 2):
        gd(x, y)
        gs(x, y)
        a, b = o1.lr_schedule_stats(), o2.lr_schedule_stats()
        assert int(a["steps"]) == int(b["steps"]) == u
        assert float(a["lr"]) == float(b["lr"])
        assert abs(float(a["lr"]) / 0.05 - ref64("poly", u, 2, 6, 0.0, float(torch.tensor(0.1)), 2.0)) <= BOUND
    dp.gather_master(o1)
    torch.cuda.synchronize()
    for a, b, r in zip(m1.parameters(), m2.parameters(), p0):
        da, db = (a.detach() - r).double(), (b.detach() - r).double()
        assert (da - db).norm().item() <= 2e-2 * db.norm().item() + 1e-6
        assert db.norm().item() > 0
