"""Weight EMA of the flat optimizers on the CPU (torch-op) paths: ``e += a_t * (w - e)`` once per
non-skipped step, ``a_t = 1 - d`` or, with warm-up, ``max(1 - d, 9 / (10 + c))`` after ``c`` updates.

The reference is a float64 EMA recomputed from clones of the master taken after every step, with
``a_t`` from the formula.  Bound after ``T`` updates: ``T * 2**-22 * M`` absolute, ``M`` the largest
magnitude any master or average element reaches in the run -- per step the sub, mul and add round at
most ``3 * 2**-24 * M``, and the error carried over is scaled by ``d_t <= 1``.

The model is the bias-carrying MLP 70-33-10 of tests/test_optim_launches_gpu.py: padded segments,
alignment gaps, 1-D tensors."""
import math
import types

import pytest
import torch

import ldnn
from ldnn.models import CrossEntropyLoss
from ldnn.models.mlp import MLP
from ldnn.optim import SGD, Adam, AdamW, Lamb, build_optimizer
from ldnn.optim.optimizers import _TRANSIENT
from ldnn.parallel.comm import FakeWorld
from ldnn.parallel.ddp import DataParallel

CONFIGS = {
    "sgd": (lambda p, **kw: SGD(p, lr=0.05, momentum=0.9, **kw), dict(ema_decay=0.9, ema_warmup=False)),
    "adam": (lambda p, **kw: Adam(p, lr=1e-3, **kw), dict(ema_decay=0.5)),   # warm-up hands over to d at c = 8
    "lamb": (lambda p, **kw: Lamb(p, lr=1e-3, weight_decay=0.01, **kw), dict(ema_decay=0.9)),
}
STATE_KEYS = ("momentum", "exp_avg", "exp_avg_sq")
# a_t as the header holds it: d is rounded to fp32 (2**-25 absolute at most, d < 1), so is the
# difference or quotient (2**-25 again, a_t <= 1)
A_TOL = 2.0 ** -24


def alpha(d, warmup, c):
    return max(1 - d, 9 / (10 + c)) if warmup else 1 - d


def ema64(start, masters, d, warmup, c0=0):
    """The float64 EMA of ``masters`` (one per update) from ``start``, and the magnitude bound M."""
    e = start.double().clone()
    M = float(e.abs().max())
    for c, w in enumerate(masters, c0):
        e += alpha(d, warmup, c) * (w.double() - e)
        M = max(M, float(w.abs().max()), float(e.abs().max()))
    return e, M


def assert_ema(e, start, masters, d, warmup):
    ref, M = ema64(start, masters, d, warmup)
    err = float((e.double() - ref).abs().max())
    assert err <= len(masters) * 2.0 ** -22 * M, (err, len(masters) * 2.0 ** -22 * M)
    # (and it is an average, not a copy of either end)
    assert not torch.equal(e, masters[-1]) and not torch.equal(e, start)


def _model(flat=True):
    torch.manual_seed(0)
    m = MLP(70, (33,), 10)
    return m, (ldnn.prepare(m, "cpu") if flat else None)


def _grads(n, steps, seed=1):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(n, generator=g) for _ in range(steps)]


def _run(name, steps=12, ema=True, grads=None):
    """``steps`` steps on random flat gradients; the masters after every step."""
    mk, kw = CONFIGS[name]
    m, f = _model()
    opt = mk(m.parameters(), **(kw if ema else {}))
    start, masters = f.master.clone(), []
    for g in grads or _grads(f.numel, steps):
        f.grad.copy_(g)
        opt.step()
        masters.append(f.master.clone())
    return opt, f, start, masters, m


@pytest.mark.parametrize("name", list(CONFIGS))
def test_flat_cpu_ema_matches_float64(name):
    opt, f, start, masters, _ = _run(name)
    kw = CONFIGS[name][1]
    e = opt._ls()["ema"]
    assert e.shape == f.master.shape and e.dtype == torch.float32
    assert_ema(e, start, masters, kw["ema_decay"], kw.get("ema_warmup", True))
    st = opt.ema_stats()
    assert int(st["updates"]) == 12 and st["decay"] == kw["ema_decay"]
    assert float(st["a_last"]) == pytest.approx(alpha(kw["ema_decay"], kw.get("ema_warmup", True), 11), abs=A_TOL)
    assert "ema" not in _TRANSIENT and "ema_hdr" in _TRANSIENT


@pytest.mark.parametrize("name", list(CONFIGS))
def test_ema_changes_nothing_else(name):
    on, f_on, _, m_on, _ = _run(name, steps=5)
    off, f_off, _, m_off, _ = _run(name, steps=5, ema=False)
    assert off.ema_stats() is None and "ema" not in off._ls() and "ema_hdr" not in off._ls()
    for a, b in zip(m_on, m_off):
        assert torch.equal(a, b)
    for k in STATE_KEYS:
        assert (k in on._ls()) == (k in off._ls())
        if k in on._ls():
            assert torch.equal(on._ls()[k], off._ls()[k]), k


def test_constructor_arguments():
    m, _ = _model()
    for bad in (0.0, 1.0, -0.1, 1.5):
        for cls in (SGD, Adam, AdamW, Lamb):
            with pytest.raises(ValueError, match="ema_decay"):
                cls(m.parameters(), ema_decay=bad)
    for name in ("sgd", "lars", "adam", "adamw", "lamb"):
        opt = build_optimizer(name, m.parameters(), 0.01, ema_decay=0.99, ema_warmup=False)
        assert opt.param_groups[0]["ema_decay"] == 0.99 and opt.param_groups[0]["ema_warmup"] is False
        assert build_optimizer(name, m.parameters(), 0.01).ema_stats() is None
    ps = list(m.parameters())
    opt = SGD([{"params": ps[:2]}, {"params": ps[2:], "ema_decay": 0.5}], lr=0.1, ema_decay=0.9)
    with pytest.raises(ValueError, match="ema_decay"):
        opt.ema_stats()


def test_ema_weights_swaps_in_and_restores_bit_for_bit():
    opt, f, _, _, m = _run("adam", steps=4)
    f.shadow = f.master.to(torch.bfloat16)      # (a CPU buffer has no shadow: give it one, as on the GPU)
    master, shadow, e = f.master.clone(), f.shadow.clone(), opt._ls()["ema"].clone()
    with opt.ema_weights():
        assert torch.equal(f.master, e) and torch.equal(opt._ls()["ema"], master)
        assert torch.equal(f.shadow, e.to(torch.bfloat16))
        for s in f.segments:
            assert torch.equal(s.param.detach(), f._logical(s, f.storage_view(s, e)))
    assert torch.equal(f.master, master) and torch.equal(f.shadow, shadow) and torch.equal(opt._ls()["ema"], e)
    # an exception inside still swaps back
    with pytest.raises(KeyError):
        with opt.ema_weights():
            raise KeyError("x")
    assert torch.equal(f.master, master) and torch.equal(opt._ls()["ema"], e)


def test_ema_weights_misuse_raises():
    m, f = _model()
    with pytest.raises(RuntimeError, match="EMA is off"):
        with Adam(m.parameters()).ema_weights():
            pass
    opt = Adam(m.parameters(), ema_decay=0.9)
    with pytest.raises(RuntimeError, match="no optimizer step has run"):
        with opt.ema_weights():
            pass
    f.grad.normal_()
    opt.step()
    master = f.master.clone()
    with opt.ema_weights():
        with pytest.raises(RuntimeError, match="does not nest"):
            with opt.ema_weights():
                pass
        with pytest.raises(RuntimeError, match="inside ema_weights"):
            opt.step()
    assert torch.equal(f.master, master)
    opt.step()      # ... and afterwards the optimizer steps again
    # (the fifth case, a sharded average that was not gathered, is in the 2-rank test below)


def _loose(name, ema=True):
    mk, kw = CONFIGS[name]
    m, _ = _model(flat=False)
    return m, mk(m.parameters(), **(kw if ema else {}))


@pytest.mark.parametrize("name", list(CONFIGS))
def test_loose_tensors_ema_per_tensor(name):
    kw = CONFIGS[name][1]
    m, opt = _loose(name)
    m0, off = _loose(name, ema=False)
    ps = list(m.parameters())
    starts, hist = [p.detach().clone() for p in ps], [[] for _ in ps]
    g = torch.Generator().manual_seed(3)
    for _ in range(12):
        for p, q, h in zip(ps, m0.parameters(), hist):
            p.grad = torch.randn(p.shape, generator=g)
            q.grad = p.grad.clone()
        opt.step()
        off.step()
        for p, h in zip(ps, hist):
            h.append(p.detach().clone())
    for p, q, s, h in zip(ps, m0.parameters(), starts, hist):
        assert torch.equal(p, q)                       # the EMA changes nothing else
        assert_ema(opt.state[p]["ema"], s, h, kw["ema_decay"], kw.get("ema_warmup", True))
    assert int(opt.ema_stats()["updates"]) == 12
    before = [p.detach().clone() for p in ps]
    with opt.ema_weights():
        for p, h, s in zip(ps, hist, starts):
            ref, _ = ema64(s, h, kw["ema_decay"], kw.get("ema_warmup", True))
            assert float((p.detach().double() - ref).abs().max()) <= 12 * 2.0 ** -22 * max(1.0, float(ref.abs().max()))
            assert not torch.equal(p.detach(), h[-1])
    for p, b in zip(ps, before):
        assert torch.equal(p.detach(), b)


@pytest.mark.parametrize("flat", [True, False])
def test_skipped_step_leaves_average_and_count(flat):
    m, f = _model(flat)
    opt = SGD(m.parameters(), lr=0.05, momentum=0.9, max_grad_norm=1.0, ema_decay=0.9)
    ps = list(m.parameters())
    g = torch.Generator().manual_seed(4)

    def fill(bad):
        for p in ps:
            p.grad = p.grad if flat else torch.empty_like(p)
            p.grad.copy_(torch.randn(p.shape, generator=g))
        if bad:
            ps[0].grad[0, 3] = float("inf")

    def avg():
        return [opt._ls()["ema"].clone()] if flat else [opt.state[p]["ema"].clone() for p in ps]

    for _ in range(2):
        fill(False)
        opt.step()
    e, w = avg(), [p.detach().clone() for p in ps]
    assert int(opt.ema_stats()["updates"]) == 2
    fill(True)
    opt.step()
    assert int(opt.grad_clip_stats()["skipped"]) == 1
    assert all(torch.equal(a, b) for a, b in zip(avg(), e))
    assert all(torch.equal(p.detach(), b) for p, b in zip(ps, w))
    assert int(opt.ema_stats()["updates"]) == 2 and float(opt.ema_stats()["a_last"]) == 0.0
    fill(False)
    opt.step()
    assert int(opt.ema_stats()["updates"]) == 3
    assert not any(torch.equal(a, b) for a, b in zip(avg(), e))


@pytest.mark.parametrize("name", list(CONFIGS))
def test_state_dict_round_trip(name, tmp_path):
    mk, kw = CONFIGS[name]
    m, f = _model()
    grads = _grads(f.numel, 6)
    straight = _run(name, grads=grads)[0]
    opt, f1, _, _, _ = _run(name, grads=grads[:3])
    sd = opt.state_dict()
    assert sd["ldnn_flat_state"]["ema_updates"] == 3 and "ema_hdr" not in sd["ldnn_flat_state"]
    # through a file, loaded with weights_only=True as the checkpoints are
    # (the whole flat master, not the model's state_dict: the random gradients moved the padding too)
    torch.save({"opt": sd, "master": f1.master}, tmp_path / "c.pt")
    ck = torch.load(tmp_path / "c.pt", weights_only=True)

    def fresh():
        m2, f2 = _model()
        f2.master.copy_(ck["master"])
        return mk(m2.parameters(), **kw), f2

    opt2, f2 = fresh()
    opt2.load_state_dict(ck["opt"])
    for g in grads[3:]:
        f2.grad.copy_(g)
        opt2.step()
    assert torch.equal(f2.master, straight._flat_for_group(straight.param_groups[0]).master)
    assert torch.equal(opt2._ls()["ema"], straight._ls()["ema"])
    assert int(opt2.ema_stats()["updates"]) == 6 == int(straight.ema_stats()["updates"])
    assert opt2.state_dict()["ldnn_flat_state"]["ema_updates"] == 6
    # a checkpoint from before the EMA existed: loads, and the average restarts from the master
    old = {k: v for k, v in ck["opt"].items()}
    old["ldnn_flat_state"] = {k: v for k, v in old["ldnn_flat_state"].items() if not k.startswith("ema")}
    for g_ in old["param_groups"]:
        g_.pop("ema_decay"), g_.pop("ema_warmup")
    opt3, f3 = fresh()
    opt3.load_state_dict(old)
    opt3.param_groups[0].update(kw)          # (the loaded groups carry the old keys only)
    assert "ema" not in opt3._ls()
    start = f3.master.clone()
    f3.grad.copy_(grads[3])
    opt3.step()
    assert int(opt3.ema_stats()["updates"]) == 1
    a0 = alpha(kw["ema_decay"], kw.get("ema_warmup", True), 0)
    ref = start.double() + a0 * (f3.master.double() - start.double())
    assert float((opt3._ls()["ema"].double() - ref).abs().max()) <= 2.0 ** -22 * float(ref.abs().max())


def _sharded_rank(comm):
    torch.manual_seed(0)
    m = MLP(70, (33,), 10)
    ldnn.prepare(m, "cpu")
    dp = DataParallel(m, comm, bucket_cap_mb=0.005, shard_optimizer=True)
    assert dp.sharded and [b["sharded"] for b in dp.bucketer.buckets] == [True, True, False]
    f = dp.flat
    opt = SGD(m.parameters(), lr=0.05, momentum=0.9, ema_decay=0.9)
    g = torch.Generator().manual_seed(20 + comm.rank)
    crit = CrossEntropyLoss()
    start, masters, refused = f.master.clone(), [], None
    for _ in range(5):
        x, y = torch.randn(8, 70, generator=g), torch.randint(0, 10, (8,), generator=g)
        opt.zero_grad()
        crit(dp(x), y).backward()
        dp.finish_gradient_sync()
        opt.step()
        try:
            with opt.ema_weights():
                pass
        except RuntimeError as e:
            refused = str(e)
        dp.gather_master(opt)
        masters.append(f.master.clone())
    with opt.ema_weights():       # whole now
        inside = f.master.clone()
    return start, masters, opt._ls()["ema"].clone(), refused, inside, int(opt.ema_stats()["updates"])


def test_sharded_two_ranks_ema_is_whole_after_gather_master():
    res = FakeWorld(2).run(_sharded_rank)
    (start, masters, e0, refused, inside, n), r1 = res
    assert torch.equal(e0, r1[2]) and torch.equal(masters[-1], r1[1][-1])
    assert n == r1[5] == 5
    assert_ema(e0, start, masters, 0.9, True)
    assert torch.equal(inside, e0)
    for r in res:
        assert r[3] is not None and "gather_master(optimizer)" in r[3]


def test_cli_flags_and_engine(monkeypatch):
    import ldnn.cli as cli
    from ldnn.models.mlp import mlp2

    p = cli.build_parser()
    a = p.parse_args([])
    assert a.ema_decay == 0.0 and a.ema_no_warmup is False
    cpu = torch.device("cpu")
    with monkeypatch.context() as mp:
        mp.setattr(cli, "native_gpu", lambda dev: True)
        a = p.parse_args(["--model", "mlp2", "--engine", "static", "--ema_decay", "0.99"])
        with pytest.raises(SystemExit, match="--ema_decay runs on the autograd path"):
            cli.resolve_engine(a, mlp2(), cpu, 1)
        a = p.parse_args(["--model", "mlp2", "--engine", "auto", "--ema_decay", "0.99"])
        assert cli.resolve_engine(a, mlp2(), cpu, 1) is False
        a = p.parse_args(["--model", "mlp2", "--engine", "static"])
        assert cli.resolve_engine(a, mlp2(), cpu, 1) is True
    for bad in ("1.0", "-0.1"):
        with pytest.raises(SystemExit, match="ema_decay"):
            cli.main(["--ema_decay", bad])


class _Log:
    def __init__(self):
        self.records = []

    def log(self, **kw):
        self.records.append(kw)


def test_trainer_validates_on_the_average(monkeypatch):
    import ldnn.train.trainer as T
    from ldnn.data.loader import get_loaders
    from ldnn.models import xavier_init
    from ldnn.models.mlp import mlp2
    from ldnn.optim import StepLR

    comm = FakeWorld(1).comm(0)
    torch.manual_seed(0)
    model = mlp2(784, 32, 10)
    xavier_init(model)
    flat = ldnn.prepare(model, "cpu")
    tr, va, te, trainset, valset, ti, vi = get_loaders(32, 1, 0, model, "cpu", None, dataset="mnist", comm=comm,
                                                       n_train=320, n_test=64, partition_rule="equal")[:7]
    opt = Adam(model.parameters(), lr=1e-3, ema_decay=0.9)
    steps, seen = [0], []
    real_validate = T.validate

    real_step = opt.step

    def counting_step(self, *a, **k):
        steps[0] += 1
        return real_step(*a, **k)

    # (a bound method, set before the scheduler wraps step: no scheduler-order warning)
    opt.step = types.MethodType(counting_step, opt)
    sch = StepLR(opt, step_size=25)

    def spy(*a, **k):
        seen.append((flat.master.clone(), opt._ls()["ema"].clone(), spy.before))
        return real_validate(*a, **k)

    # what the buffers held just before the trainer entered its evaluation context
    real_ctx = T.ema_eval

    def ctx(o, dp=None):
        spy.before = (flat.master.clone(), o._ls()["ema"].clone())
        return real_ctx(o, dp)

    monkeypatch.setattr(T, "validate", spy)
    monkeypatch.setattr(T, "ema_eval", ctx)
    log = _Log()
    T.train_global(model, tr, va, trainset, valset, ti, vi, CrossEntropyLoss(), opt, sch, "cpu", 0, 1, 2, 1,
                   math.inf, 32, 0.0, 0.0, comm=comm, progress=False, verbose=False, logger=log, repartition=False)
    assert len(seen) == 2 and steps[0] > 0
    for master, avg, (live, ema_before) in seen:
        assert torch.equal(master, ema_before) and torch.equal(avg, live)   # swapped in
        assert not torch.equal(master, live)
    # afterwards the master is the live weights again: it equals what the last validation held aside
    assert torch.equal(flat.master, seen[-1][1]) and torch.equal(opt._ls()["ema"], seen[-1][0])
    rec = [r for r in log.records if r.get("kind") == "global_epoch"]
    assert len(rec) == 1 and rec[0]["ema_updates"] == steps[0]
    assert rec[0]["ema_a_last"] == pytest.approx(alpha(0.9, True, steps[0] - 1), abs=A_TOL)
    assert isinstance(rec[0]["ema_updates"], int) and isinstance(rec[0]["ema_a_last"], float)
