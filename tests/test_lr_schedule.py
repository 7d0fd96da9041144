"""Per-step learning-rate schedule on the host paths (CPU flat buffer, loose tensors): the factor
against the float64 closed form, its edges, composition with a per-epoch change of the base rate,
the constructor's checks, the optimizers against a run whose rate the test sets by hand, the
non-finite guard, checkpoints, the CLI flags and the collective count of a sharded run.

``ref_factor`` below is the closed form as the optimizers' docstring states it, written out
independently; the host paths compute in Python floats too, so the comparison is to a few ulps
(1e-15 absolute: the factor is at most 1)."""
import math

import pytest
import torch

import ldnn
from ldnn.models import CrossEntropyLoss
from ldnn.models.mlp import MLP
from ldnn.optim import SGD, Adam, AdamW, Lamb, StepLR, build_optimizer
from ldnn.optim.optimizers import _TRANSIENT, lr_schedule_factor
from ldnn.parallel.comm import FakeWorld
from ldnn.parallel.ddp import DataParallel

KINDS = ("constant", "linear", "poly", "cosine")
WT = ((0, 5), (3, 8), (3, 4))
STEPS = 11


def ref_factor(kind, u, W, T, ws=0.0, m=0.0, q=2.0):
    if u <= W:
        return ws + (1 - ws) * u / W
    if kind == "constant":
        return 1.0
    p = min(1.0, (u - W) / (T - W))
    if kind == "cosine":
        return m + (1 - m) * 0.5 * (1 + math.cos(math.pi * p))
    return m + (1 - m) * (1 - p) ** (1.0 if kind == "linear" else q)


def sched(kind, W, T, **kw):
    return dict(kind=kind, total_steps=T, warmup_steps=W, **kw)


def _model(flat=True):
    torch.manual_seed(0)
    m = MLP(70, (33,), 10)
    return m, (ldnn.prepare(m, "cpu") if flat else None)


def _fill(ps, g, flat, bad=False):
    for p in ps:
        p.grad = p.grad if flat else torch.empty_like(p)
        p.grad.copy_(torch.randn(p.shape, generator=g))
    if bad:
        ps[0].grad[0, 3] = float("inf")


# ---- the factor ----------------------------------------------------------------------------
@pytest.mark.parametrize("W,T", WT)
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("extra", [{}, dict(warmup_start=0.25, min_ratio=0.1, power=3.0)])
def test_factor_against_closed_form(kind, W, T, extra):
    w = torch.nn.Parameter(torch.ones(3))
    opt = SGD([w], lr=0.5, lr_schedule=sched(kind, W, T, **extra))
    ref = dict(ws=extra.get("warmup_start", 0.0), m=extra.get("min_ratio", 0.0), q=extra.get("power", 2.0))
    for u in range(1, STEPS + 1):
        w.grad = torch.ones(3)
        opt.step()
        want = ref_factor(kind, u, W, T, **ref)
        st = opt.lr_schedule_stats()
        assert int(st["steps"]) == u
        assert abs(float(st["factor"]) - want) <= 1e-15, (u, float(st["factor"]), want)
        assert abs(float(st["lr"]) - 0.5 * want) <= 1e-15
        assert abs(lr_schedule_factor(opt.param_groups[0]["lr_schedule"], u) - want) <= 1e-15
    # the horizon clamp was exercised: beyond T the factor is the floor (constant: 1)
    assert float(st["factor"]) == (1.0 if kind == "constant" else ref["m"])


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("ws", [0.0, 0.1, 0.3])
def test_warmup_edges(kind, ws):
    s = sched(kind, 3, 8, warmup_start=ws, min_ratio=0.2)
    # the last warm-up step runs at exactly the base, and the first step of the decay joins it
    assert lr_schedule_factor(s, 3) == 1.0
    assert lr_schedule_factor(s, 1) > 0.0                     # ws = 0: the first step already moves
    assert lr_schedule_factor(s, 1) == pytest.approx(ws + (1 - ws) / 3, abs=1e-15)
    step = abs(lr_schedule_factor(s, 4) - 1.0)
    assert step <= (1 - 0.2) * (1 / 5) * 2.0 + 1e-15          # no jump: at most the decay's steepest slope
    assert lr_schedule_factor(s, 8) == (1.0 if kind == "constant" else 0.2)


def test_linear_is_poly_with_power_one():
    for u in range(1, STEPS + 1):
        assert lr_schedule_factor(sched("linear", 3, 8, min_ratio=0.1), u) == \
            lr_schedule_factor(sched("poly", 3, 8, min_ratio=0.1, power=1.0), u)
        # ("linear" ignores a power given with it)
        assert lr_schedule_factor(sched("linear", 3, 8, power=5.0), u) == lr_schedule_factor(sched("linear", 3, 8), u)


def test_composes_with_steplr():
    m, f = _model()
    opt = SGD(m.parameters(), lr=0.1, lr_schedule=sched("cosine", 2, 10))
    stepper = StepLR(opt, step_size=1, gamma=0.5)
    g = torch.Generator().manual_seed(2)
    for u in range(1, 9):
        _fill(list(m.parameters()), g, True)
        opt.step()
        base = 0.1 * 0.5 ** ((u - 1) // 4)
        assert opt.param_groups[0]["lr"] == pytest.approx(base, rel=1e-12)
        assert float(opt.lr_schedule_stats()["lr"]) == pytest.approx(base * ref_factor("cosine", u, 2, 10), rel=1e-12)
        if u % 4 == 0:
            stepper.step()        # (an "epoch" of 4 steps)


def test_validation_errors():
    w = [torch.nn.Parameter(torch.ones(3))]
    for bad in (sched("cosine", 3, 3), sched("poly", 5, 2), dict(kind="cosine"), sched("cosine", 0, 5, warmup_start=1.5),
                sched("cosine", 0, 5, warmup_start=-0.1), sched("cosine", 0, 5, min_ratio=1.01),
                sched("cosine", 0, 5, min_ratio=-1.0), sched("exp", 0, 5), sched("poly", 0, 5, power=0.0),
                sched("cosine", -1, 5), dict(kind="cosine", total_steps=5, decay=0.1), "cosine"):
        for mk in (SGD, Adam, AdamW, Lamb):
            with pytest.raises(ValueError, match="lr_schedule"):
                mk(w, lr=0.1, lr_schedule=bad)
        with pytest.raises(ValueError, match="lr_schedule"):
            build_optimizer("lamb", w, 0.1, lr_schedule=bad)
    SGD(w, lr=0.1, lr_schedule=dict(kind="constant", warmup_steps=4))       # (constant needs no horizon)
    a, b = torch.nn.Parameter(torch.ones(3)), torch.nn.Parameter(torch.ones(3))
    with pytest.raises(ValueError, match="same in every param group"):
        SGD([dict(params=[a], lr_schedule=sched("cosine", 0, 5)), dict(params=[b])], lr=0.1)
    with pytest.raises(ValueError, match="same in every param group"):
        SGD([dict(params=[a], lr_schedule=sched("cosine", 0, 5)),
             dict(params=[b], lr_schedule=sched("cosine", 0, 6))], lr=0.1)
    # off by default, and then nothing about it is kept
    opt = SGD([a], lr=0.1)
    a.grad = torch.ones(3)
    opt.step()
    assert opt.lr_schedule_stats() is None
    assert not any(k.startswith("sched") for k in opt._ls()) and "sched_steps" not in opt.state_dict()["ldnn_flat_state"]


# ---- the optimizers ------------------------------------------------------------------------
CONFIGS = {
    "sgd": lambda p, **kw: SGD(p, lr=0.05, momentum=0.9, weight_decay=1e-3, **kw),
    "lamb": lambda p, **kw: Lamb(p, lr=1e-2, weight_decay=0.01, **kw),
    "adamw": lambda p, **kw: build_optimizer("adamw", p, 1e-3, weight_decay=0.01, **kw),
}
SCHED = sched("cosine", 3, 8, warmup_start=0.1, min_ratio=0.05)


@pytest.mark.parametrize("flat", [True, False])
@pytest.mark.parametrize("name", list(CONFIGS))
def test_matches_a_run_with_the_rate_set_by_hand(name, flat):
    ma, _ = _model(flat)
    mb, _ = _model(flat)
    a, b = CONFIGS[name](ma.parameters(), lr_schedule=SCHED), CONFIGS[name](mb.parameters())
    base = b.param_groups[0]["lr"]
    ga, gb = torch.Generator().manual_seed(3), torch.Generator().manual_seed(3)
    for u in range(1, STEPS + 1):
        _fill(list(ma.parameters()), ga, flat)
        _fill(list(mb.parameters()), gb, flat)
        b.param_groups[0]["lr"] = base * lr_schedule_factor(SCHED, u)
        a.step()
        b.step()
        assert a.param_groups[0]["lr"] == base                 # (the schedule leaves the base alone)
        for p, r in zip(ma.parameters(), mb.parameters()):
            assert torch.equal(p.detach(), r.detach()), (name, u)
    start, _ = _model(flat)
    assert not any(torch.equal(p.detach(), s.detach()) for p, s in zip(ma.parameters(), start.parameters()))


@pytest.mark.parametrize("flat", [True, False])
def test_skipped_step_is_not_counted(flat):
    m, _ = _model(flat)
    opt = SGD(m.parameters(), lr=0.05, momentum=0.9, max_grad_norm=1.0, lr_schedule=sched("linear", 4, 9))
    ps, g = list(m.parameters()), torch.Generator().manual_seed(4)
    for _ in range(2):
        _fill(ps, g, flat)
        opt.step()
    before = [p.detach().clone() for p in ps]
    assert int(opt.lr_schedule_stats()["steps"]) == 2
    _fill(ps, g, flat, bad=True)
    opt.step()
    st = opt.lr_schedule_stats()
    assert int(opt.grad_clip_stats()["skipped"]) == 1
    assert int(st["steps"]) == 2 and float(st["factor"]) == ref_factor("linear", 2, 4, 9)
    assert all(torch.equal(p.detach(), b) for p, b in zip(ps, before))
    _fill(ps, g, flat)
    opt.step()                                     # the step the skipped one would have been
    st = opt.lr_schedule_stats()
    assert int(st["steps"]) == 3 and float(st["factor"]) == ref_factor("linear", 3, 4, 9)
    assert not any(torch.equal(p.detach(), b) for p, b in zip(ps, before))


@pytest.mark.parametrize("name", list(CONFIGS))
def test_state_dict_round_trip(name, tmp_path):
    def run(opt, m, grads):
        f = opt._flat_for_group(opt.param_groups[0])
        for g in grads:
            f.grad.copy_(g)
            opt.step()
        return f

    m, f = _model()
    gen = torch.Generator().manual_seed(5)
    grads = [torch.randn(f.numel, generator=gen) for _ in range(6)]
    straight = CONFIGS[name](m.parameters(), lr_schedule=SCHED)
    fs = run(straight, m, grads)
    m1, _ = _model()
    opt = CONFIGS[name](m1.parameters(), lr_schedule=SCHED)
    f1 = run(opt, m1, grads[:3])
    sd = opt.state_dict()
    assert sd["ldnn_flat_state"]["sched_steps"] == 3
    assert not any(k in sd["ldnn_flat_state"] for k in _TRANSIENT)
    torch.save({"opt": sd, "master": f1.master}, tmp_path / "c.pt")
    ck = torch.load(tmp_path / "c.pt", weights_only=True)
    assert ck["opt"]["param_groups"][0]["lr_schedule"] == SCHED
    m2, f2 = _model()
    f2.master.copy_(ck["master"])
    opt2 = CONFIGS[name](m2.parameters(), lr_schedule=SCHED)
    opt2.load_state_dict(ck["opt"])
    assert int(opt2.lr_schedule_stats()["steps"]) == 3
    run(opt2, m2, grads[3:])
    assert torch.equal(f2.master, fs.master)
    assert int(opt2.lr_schedule_stats()["steps"]) == 6 == opt2.state_dict()["ldnn_flat_state"]["sched_steps"]
    # a checkpoint from before the schedule existed: loads, and the schedule starts at 0
    old = dict(ck["opt"])
    old["ldnn_flat_state"] = {k: v for k, v in old["ldnn_flat_state"].items() if k != "sched_steps"}
    for g_ in old["param_groups"]:
        g_.pop("lr_schedule")
    m3, f3 = _model()
    opt3 = CONFIGS[name](m3.parameters())
    opt3.load_state_dict(old)
    assert opt3.lr_schedule_stats() is None
    opt3.param_groups[0]["lr_schedule"] = dict(SCHED)
    f3.grad.copy_(grads[3])
    opt3.step()
    st = opt3.lr_schedule_stats()
    assert int(st["steps"]) == 1 and float(st["factor"]) == lr_schedule_factor(SCHED, 1)


# ---- CLI -----------------------------------------------------------------------------------
def test_cli_flags_and_engine(monkeypatch):
    import ldnn.cli as cli
    from ldnn.models.mlp import mlp2

    p = cli.build_parser()
    a = p.parse_args([])
    assert (a.lr_schedule, a.warmup_steps, a.warmup_start, a.lr_total_steps, a.lr_min_ratio, a.lr_power) == \
        ("none", 0, 0.0, None, 0.0, 2.0)
    assert cli.schedule_from_args(a, 100) is None
    a = p.parse_args(["--lr_schedule", "poly", "--warmup_steps", "5", "--warmup_start", "0.1", "--lr_min_ratio",
                      "0.01", "--lr_power", "1.5"])
    assert cli.schedule_from_args(a, 100) == dict(kind="poly", total_steps=100, warmup_steps=5, warmup_start=0.1,
                                                  min_ratio=0.01, power=1.5)
    a = p.parse_args(["--lr_schedule", "cosine", "--lr_total_steps", "40"])
    d = cli.schedule_from_args(a, 100)
    assert d["total_steps"] == 40
    SGD([torch.nn.Parameter(torch.ones(2))], lr=0.1, lr_schedule=d)
    with pytest.raises(SystemExit):
        p.parse_args(["--lr_schedule", "exponential"])
    cpu = torch.device("cpu")
    with monkeypatch.context() as mp:
        mp.setattr(cli, "native_gpu", lambda dev: True)
        a = p.parse_args(["--model", "mlp2", "--engine", "static", "--lr_schedule", "cosine"])
        with pytest.raises(SystemExit, match="--lr_schedule runs on the autograd path"):
            cli.resolve_engine(a, mlp2(), cpu, 1)
        a = p.parse_args(["--model", "mlp2", "--engine", "auto", "--lr_schedule", "cosine"])
        assert cli.resolve_engine(a, mlp2(), cpu, 1) is False
        a = p.parse_args(["--model", "mlp2", "--engine", "static"])
        assert cli.resolve_engine(a, mlp2(), cpu, 1) is True
    for bad in (["--warmup_start", "1.5"], ["--lr_min_ratio", "-0.5"], ["--lr_power", "0"], ["--warmup_steps", "-2"]):
        with pytest.raises(SystemExit, match="--lr_schedule"):
            cli.main(["--lr_schedule", "cosine"] + bad)


# ---- sharded data parallelism --------------------------------------------------------------
def _sharded_rank(comm, schedule):
    torch.manual_seed(0)
    m = MLP(70, (33,), 10)
    ldnn.prepare(m, "cpu")
    dp = DataParallel(m, comm, bucket_cap_mb=0.005, shard_optimizer=True)
    assert dp.sharded
    opt = SGD(m.parameters(), lr=0.05, momentum=0.9, max_grad_norm=1.0, lr_schedule=schedule)
    g = torch.Generator().manual_seed(20 + comm.rank)
    crit = CrossEntropyLoss()
    lrs = []
    for _ in range(5):
        x, y = torch.randn(8, 70, generator=g), torch.randint(0, 10, (8,), generator=g)
        opt.zero_grad()
        crit(dp(x), y).backward()
        dp.finish_gradient_sync()
        opt.step()
        st = opt.lr_schedule_stats()
        lrs.append(None if st is None else float(st["lr"]))
    dp.gather_master(opt)
    return comm.schedule_digest(), lrs, dp.flat.master.clone()


def test_sharded_two_ranks_need_no_extra_collective():
    on = FakeWorld(2).run(_sharded_rank, sched("cosine", 2, 6))
    off = FakeWorld(2).run(_sharded_rank, None)
    assert on[0][0] == on[1][0] == off[0][0] == off[1][0]        # op count and op / shape / dtype hash
    assert on[0][0][0] > 0
    want = [0.05 * ref_factor("cosine", u, 2, 6) for u in range(1, 6)]
    for r in on:
        assert r[1] == pytest.approx(want, rel=1e-12)
    assert torch.equal(on[0][2], on[1][2]) and not torch.equal(on[0][2], off[0][2])


# ---- the CLI's default horizon -------------------------------------------------------------
def _horizon_rank(comm, sync_every, lengths):
    """One rank of a run whose shards differ in length: the CLI's default horizon, an optimizer built
    from it, and the rates of the lock-step updates."""
    import ldnn.cli as cli

    a = cli.build_parser().parse_args(["--lr_schedule", "cosine", "--warmup_steps", "2", "--epochs_global", "2",
                                       "--epochs_local", "3", "--sync_every", sync_every])
    n = lengths[comm.rank]
    total = cli.default_total_steps(a, n, comm, comm.world_size, torch.device("cpu"))
    w = torch.nn.Parameter(torch.ones(3))
    opt = SGD([w], lr=0.1, lr_schedule=cli.schedule_from_args(a, total))
    lrs = []
    for _ in range(12):
        w.grad = torch.ones(3)
        opt.step()
        lrs.append(float(opt.lr_schedule_stats()["lr"]))
    return total, lrs, comm.schedule_digest()


def test_default_horizon_is_agreed_across_ranks_under_per_step_sync():
    # shards of 7, 10 and 9 batches: a local epoch runs the shortest loader's 7 steps and one tail step
    res = FakeWorld(3).run(_horizon_rank, "step", (7, 10, 9))
    assert [r[0] for r in res] == [2 * 3 * 8] * 3
    assert res[0][1] == res[1][1] == res[2][1] and len(set(res[0][1])) == 12
    assert res[0][1] == pytest.approx([0.1 * ref_factor("cosine", u, 2, 48) for u in range(1, 13)], rel=1e-12)
    assert res[0][2] == res[1][2] == res[2][2] and res[0][2][0] == 1          # one collective, on every rank
    # equal shards: no tail step
    assert [r[0] for r in FakeWorld(2).run(_horizon_rank, "step", (7, 7))] == [2 * 3 * 7] * 2
    # the global-epoch schedule: every rank counts its own steps, no collective
    res = FakeWorld(2).run(_horizon_rank, "global_epoch", (7, 10))
    assert [r[0] for r in res] == [42, 60] and res[0][2][0] == res[1][2][0] == 0
    # one rank: its own loader
    assert FakeWorld(1).run(_horizon_rank, "step", (5,))[0][0] == 30


def test_cli_exits_when_the_default_horizon_is_within_the_warmup():
    import ldnn.cli as cli

    a = cli.build_parser().parse_args(["--lr_schedule", "cosine", "--warmup_steps", "50"])
    with pytest.raises(SystemExit, match=r"--lr_total_steps must be a whole number > --warmup_steps \(50\).*"
                                         r"default horizon of this run is 40 steps"):
        cli.schedule_from_args(a, 40)
    assert cli.schedule_from_args(a, 51)["total_steps"] == 51
    a = cli.build_parser().parse_args(["--lr_schedule", "cosine", "--warmup_steps", "50", "--lr_total_steps", "20"])
    with pytest.raises(SystemExit, match="--lr_total_steps must be a whole number > --warmup_steps"):
        cli.main(["--lr_schedule", "cosine", "--warmup_steps", "50", "--lr_total_steps", "20"])


def test_every_bad_value_is_a_value_error():
    from ldnn.optim import check_lr_schedule

    w = [torch.nn.Parameter(torch.ones(3))]
    for bad in (dict(kind="cosine", total_steps="8"), dict(kind="cosine", total_steps=float("inf")),
                dict(kind="cosine", total_steps=float("nan")), dict(kind="cosine", total_steps=8, warmup_steps="2"),
                dict(kind="cosine", total_steps=8, warmup_steps=2.5), dict(kind="cosine", total_steps=8, power="2"),
                dict(kind="cosine", total_steps=8, min_ratio=[0.1]), dict(kind="cosine", total_steps=True),
                dict(kind=["cosine"], total_steps=8), {1: 2, "kind": "cosine", "total_steps": 8}):
        with pytest.raises(ValueError, match="lr_schedule"):
            check_lr_schedule(bad)
        with pytest.raises(ValueError, match="lr_schedule"):
            Adam(w, lr=0.1, lr_schedule=bad)
    assert check_lr_schedule(None) is None
    d = dict(kind="poly", total_steps=8.0, warmup_steps=2, power=None)       # (whole floats and None defaults pass)
    assert check_lr_schedule(d) == d and check_lr_schedule(d) is not d


def test_schedule_is_validated_once_per_value(monkeypatch):
    import ldnn.optim.optimizers as O

    calls = []
    real = O._sched_consts
    monkeypatch.setattr(O, "_sched_consts", lambda s: (calls.append(1), real(s))[1])
    m, _ = _model()
    opt = SGD(m.parameters(), lr=0.05, lr_schedule=sched("cosine", 2, 8))
    n0 = len(calls)
    g = torch.Generator().manual_seed(6)
    for _ in range(3):
        _fill(list(m.parameters()), g, True)
        opt.step()
        opt.lr_schedule_stats()
    assert len(calls) == n0
    opt.param_groups[0]["lr_schedule"]["total_steps"] = 6          # changed in place: seen, checked once
    _fill(list(m.parameters()), g, True)
    opt.step()
    assert len(calls) == n0 + 1
    assert float(opt.lr_schedule_stats()["factor"]) == ref_factor("cosine", 4, 2, 6)
    opt.param_groups[0]["lr_schedule"]["total_steps"] = 1          # ... and still refused when wrong
    with pytest.raises(ValueError, match="total_steps"):
        opt.step()
