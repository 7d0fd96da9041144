"""Lion (optim/optimizers.py Lion), CPU paths: the torch-op twin against an oracle written out here
(per-tensor fp64 state from the same fp32 gradients), sign(0), the first step, the non-finite guard
with a schedule, the state_dict round trip, ``build_optimizer``, the CLI, sharded == unsharded under
FakeWorld with no extra all-reduce (with clipping: exactly one), and the EMA riding along."""
import json

import pytest
import torch

import ldnn
from ldnn.models import CrossEntropyLoss, build_model, xavier_init
from ldnn.optim import SGD, Adam, AdamW, Lamb, Lion, build_optimizer
from ldnn.parallel.comm import FakeWorld
from ldnn.parallel.ddp import DataParallel

LR, B1, B2, WD = 1e-3, 0.9, 0.99, 1e-2


def _init_state():
    torch.manual_seed(0)
    m = build_model("lenet5")
    xavier_init(m)
    return m.state_dict()


INIT = _init_state()


def _lenet(flat=True):
    m = build_model("lenet5")
    m.load_state_dict(INIT)
    if flat:
        ldnn.prepare(m, "cpu")
    return m


def _batch(g, n=8):
    return torch.randn(n, 1, 28, 28, generator=g), torch.randint(0, 10, (n,), generator=g)


def _backward(mod, opt, x, y, scale=1.0):
    opt.zero_grad()
    (torch.nn.functional.cross_entropy(mod(x), y) * scale).backward()


def _params(m):
    return [p.detach().clone() for p in m.parameters()]


class _Oracle:
    """The formulas per tensor in fp64, fed the fp32 gradients the model under test computed (a sign
    amplifies a last-bit difference between two models' gradients without bound, so the oracle takes
    the very same ones)."""

    def __init__(self, model, lr=LR, wd=WD, b1=B1, b2=B2, max_norm=None):
        self.model, self.lr, self.wd, self.b1, self.b2, self.max_norm = model, lr, wd, b1, b2, max_norm
        self.w = {n: p.detach().double().clone() for n, p in model.named_parameters()}
        self.m = {n: torch.zeros_like(v) for n, v in self.w.items()}
        self.undecided = 0

    def step(self):
        """One step from the model's current .grad (call it before the optimizer's step)."""
        grads = {n: p.grad.detach().clone() for n, p in self.model.named_parameters()}
        if self.max_norm is not None:
            tmp = [torch.nn.Parameter(torch.zeros_like(g)) for g in grads.values()]
            for t, g in zip(tmp, grads.values()):
                t.grad = g
            torch.nn.utils.clip_grad_norm_(tmp, self.max_norm)      # (clips the clones in place)
        for n in self.w:
            g, m = grads[n].double(), self.m[n]
            c = self.b1 * m + (1 - self.b1) * g
            # (an fp32 c this close to 0 could round to the other side: the oracle counts them)
            self.undecided += int(((c != 0) & (c.abs() <= 4 * 2.0 ** -24 * ((self.b1 * m).abs() +
                                                                           ((1 - self.b1) * g).abs()))).sum())
            w = self.w[n]
            if self.wd != 0:
                w = w * (1 - self.lr * self.wd)
            self.w[n] = w - self.lr * torch.sign(c)
            self.m[n] = self.b2 * m + (1 - self.b2) * g

    def check(self, opt, flat):
        assert self.undecided == 0      # (else a sign may legitimately differ: pick another seed)
        for n, p in self.model.named_parameters():
            torch.testing.assert_close(p.detach(), self.w[n].float(), rtol=1e-5, atol=1e-6, msg=n)
        if flat:
            f = opt._flat_for_group(opt.param_groups[0])
            for s in f.segments:
                got = f._logical(s, f.storage_view(s, opt._ls()["exp_avg"]))
                torch.testing.assert_close(got, self.m[s.name].float(), rtol=1e-5, atol=1e-6, msg=s.name)
                assert bool((got != 0).any()), s.name
        else:
            for n, p in self.model.named_parameters():
                assert sorted(opt.state[p]) == ["exp_avg"]
                torch.testing.assert_close(opt.state[p]["exp_avg"], self.m[n].float(), rtol=1e-5, atol=1e-6, msg=n)


# ---------------------------------------------------------------- 1. oracle
@pytest.mark.parametrize("clip", [None, 1.0])
@pytest.mark.parametrize("flat", [True, False])
def test_lion_steps_match_the_oracle(flat, clip):
    """4 steps of LeNet-5 (1-D and 4-D tensors, the padded 10-row head), batch 8, weight decay 1e-2,
    with and without clipping (losses scaled so that it clips): weights and moment within rtol 1e-5 /
    atol 1e-6 of the fp64 oracle -- a flipped sign would be off by 2 lr = 2e-3."""
    m = _lenet(flat)
    o = Lion(m.parameters(), lr=LR, weight_decay=WD, max_grad_norm=clip)
    ora = _Oracle(m, max_norm=clip)
    g = torch.Generator().manual_seed(1)
    for s in (1.0, 20.0, 1.0, 20.0):
        x, y = _batch(g)
        _backward(m, o, x, y, s)
        ora.step()
        o.step()
    ora.check(o, flat)
    if clip is not None:
        assert int(o.grad_clip_stats()["clipped"]) >= 1 and int(o.grad_clip_stats()["steps"]) == 4
    if flat:
        assert sorted(k for k in o._ls() if k not in ("clip",)) == ["exp_avg", "step"] and o._ls()["step"] == 4
        assert o.lars_stats() is None and o.lamb_stats() is None
        assert not o.supports_ranges() and o.range_updater() is None     # (CPU buffers: no range launches)


# ---------------------------------------------------------------- 2. sign(0) and the first step
@pytest.mark.parametrize("flat", [True, False])
def test_sign_of_zero_moves_by_the_decay_only(flat):
    """beta1 = 0.5 and g = -m make c = 0.5 m - 0.5 m exactly 0 in every element: the weights move by
    the decay factor alone, and m becomes 0.75 m - 0.25 m = m / 2 (0.75 m rounds: within one ulp)."""
    lr, wd = 1e-2, 0.25
    m = _lenet(flat)
    o = Lion(m.parameters(), lr=lr, betas=(0.5, 0.75), weight_decay=wd)
    x, y = _batch(torch.Generator().manual_seed(2))
    _backward(m, o, x, y)
    o.step()
    if flat:
        mom = o._ls()["exp_avg"].clone()
        f = o._flat_for_group(o.param_groups[0])
        f.grad.copy_(-mom)
    else:
        mom = [o.state[p]["exp_avg"].clone() for p in m.parameters()]
        for p, b in zip(m.parameters(), mom):
            p.grad = -b
    before = _params(m)
    o.step()
    moved = 0
    for p, q in zip(m.parameters(), before):
        assert torch.equal(p.detach(), q * (1 - lr * wd))
        moved += int((p.detach() != q).sum())
    assert moved > 0
    if flat:
        torch.testing.assert_close(o._ls()["exp_avg"], mom * 0.5, rtol=2.0 ** -23, atol=0)
        assert bool((mom != 0).any())
    else:
        for p, b in zip(m.parameters(), mom):
            torch.testing.assert_close(o.state[p]["exp_avg"], b * 0.5, rtol=2.0 ** -23, atol=0)


@pytest.mark.parametrize("flat", [True, False])
def test_first_step_moves_every_element_by_the_rate(flat):
    m = _lenet(flat)
    o = Lion(m.parameters(), lr=LR)
    x, y = _batch(torch.Generator().manual_seed(3))
    _backward(m, o, x, y)
    before, grads = _params(m), [p.grad.detach().clone() for p in m.parameters()]
    o.step()
    for p, q, g in zip(m.parameters(), before, grads):
        assert torch.equal(p.detach(), q - LR * g.sign())
        assert bool((g != 0).any())
    # a NaN gradient element without clipping: that element's moment and weight become NaN, no other
    _backward(m, o, x, y)
    p0 = next(iter(m.parameters()))
    p0.grad.view(-1)[3] = float("nan")
    o.step()
    bad = torch.isnan(p0.detach().view(-1))
    assert bool(bad[3]) and int(bad.sum()) == 1
    mom = o._ls()["exp_avg"] if flat else o.state[p0]["exp_avg"]
    assert int(torch.isnan(mom).sum()) == 1


# ---------------------------------------------------------------- 3. the non-finite guard and the schedule
@pytest.mark.parametrize("flat", [True, False])
def test_skipped_step_changes_nothing_and_is_not_counted_by_the_schedule(flat):
    """Warm-up over 10 steps from 0: step u runs at lr * u / 10.  Step 1, a non-finite step, then the
    next one, which runs at u = 2 (not 3): with weight decay 0 every moved element moves by the rate."""
    lr = 1e-2
    m = _lenet(flat)
    o = Lion(m.parameters(), lr=lr, max_grad_norm=1.0, ema_decay=0.9,
             lr_schedule=dict(kind="constant", total_steps=100, warmup_steps=10))
    g = torch.Generator().manual_seed(4)

    def moved_by():
        before = _params(m)
        o.step()
        d = torch.cat([(p.detach() - q).abs().flatten() for p, q in zip(m.parameters(), before)])
        return d[d != 0]

    x, y = _batch(g)
    _backward(m, o, x, y)
    d = moved_by()
    assert d.numel() and bool(((d - lr * 0.1).abs() <= 1e-7).all())
    before = _params(m)
    state = ({k: v.clone() for k, v in o._ls().items() if torch.is_tensor(v) and k in ("exp_avg", "ema")} if flat else
             {(i, k): v.clone() for i, p in enumerate(m.parameters()) for k, v in o.state[p].items()})
    x, y = _batch(g)
    _backward(m, o, x, y)
    next(iter(m.parameters())).grad.view(-1)[3] = float("inf")
    o.step()
    assert int(o.grad_clip_stats()["skipped"]) == 1
    for p, q in zip(m.parameters(), before):
        assert torch.equal(p.detach(), q)
    now = (o._ls() if flat else {(i, k): v for i, p in enumerate(m.parameters()) for k, v in o.state[p].items()})
    for k, v in state.items():
        assert torch.equal(now[k], v), k
    assert int(o.lr_schedule_stats()["steps"]) == 1 and int(o.ema_stats()["updates"]) == 1
    x, y = _batch(g)
    _backward(m, o, x, y)
    d = moved_by()
    assert d.numel() and bool(((d - lr * 0.2).abs() <= 1e-7).all())
    assert int(o.lr_schedule_stats()["steps"]) == 2
    assert float(o.lr_schedule_stats()["lr"]) == pytest.approx(lr * 0.2, rel=1e-6)


# ---------------------------------------------------------------- 4. state_dict
@pytest.mark.parametrize("clip", [None, 1.0])
def test_state_dict_round_trip_continues_bit_for_bit(clip):
    ma, mb = _lenet(), _lenet()
    oa = Lion(ma.parameters(), lr=LR, weight_decay=WD, max_grad_norm=clip)
    g = torch.Generator().manual_seed(5)
    batches = [_batch(g) for _ in range(5)]
    for x, y in batches[:2]:
        _backward(ma, oa, x, y, 20.0)
        oa.step()
    sd = oa.state_dict()
    assert sorted(sd["ldnn_flat_state"]) == ["exp_avg", "step"] and sd["ldnn_flat_state"]["step"] == 2
    mb.load_state_dict(ma.state_dict())
    ob = Lion(mb.parameters(), lr=0.5, betas=(0.5, 0.5))
    ob.load_state_dict(sd)
    assert ob.param_groups[0]["lr"] == LR and ob.param_groups[0]["betas"] == (B1, B2)
    for x, y in batches[2:]:
        for mod, opt in ((ma, oa), (mb, ob)):
            _backward(mod, opt, x, y, 20.0)
            opt.step()
    fa, fb = (o._flat_for_group(o.param_groups[0]) for o in (oa, ob))
    assert torch.equal(fa.master, fb.master)
    assert torch.equal(oa._ls()["exp_avg"], ob._ls()["exp_avg"]) and "exp_avg_sq" not in ob._ls()
    assert oa.state_dict()["ldnn_flat_state"]["step"] == ob.state_dict()["ldnn_flat_state"]["step"] == 5


# ---------------------------------------------------------------- 5. interface
def test_build_optimizer_and_refusals():
    m = _lenet()
    sched = dict(kind="cosine", total_steps=50, warmup_steps=5)
    o = build_optimizer("lion", m.parameters(), 3e-4, momentum=0.5, weight_decay=0.1, max_grad_norm=1.0,
                        ema_decay=0.99, ema_warmup=False, lr_schedule=sched)
    g0 = o.param_groups[0]
    assert isinstance(o, Lion) and g0["lr"] == 3e-4 and g0["betas"] == (0.9, 0.99) and g0["weight_decay"] == 0.1
    assert g0["max_grad_norm"] == 1.0 and g0["ema_decay"] == 0.99 and g0["ema_warmup"] is False
    assert g0["lr_schedule"] == sched and "momentum" not in g0 and "eps" not in g0
    d = Lion(m.parameters()).param_groups[0]
    assert d["lr"] == 1e-4 and d["betas"] == (0.9, 0.99) and d["weight_decay"] == 0.0 and d["max_grad_norm"] is None
    assert build_optimizer("LION", m.parameters(), 1e-4, max_grad_norm=0.0).param_groups[0]["max_grad_norm"] is None
    for kw in (dict(lars_trust=0.01), dict(lars_eps=1e-6), dict(lars_exclude_1d=False), dict(lamb_exclude_1d=False)):
        with pytest.raises(TypeError):
            build_optimizer("lion", m.parameters(), 1e-4, **kw)
    for betas in ((1.0, 0.99), (0.9, 1.0), (-0.1, 0.99), (0.9, 1.5), (0.9,)):
        with pytest.raises(ValueError, match="betas"):
            Lion(m.parameters(), betas=betas)
    Lion(m.parameters(), betas=(0.0, 0.0))
    with pytest.raises(ValueError, match="ema_decay"):
        Lion(m.parameters(), ema_decay=1.0)
    with pytest.raises(ValueError, match="lr_schedule"):
        Lion(m.parameters(), lr_schedule=dict(kind="cosine"))
    with pytest.raises(TypeError):
        Lion(m.parameters(), eps=1e-8)
    for Opt in (SGD, Adam, AdamW, Lamb):
        assert Opt._update_native is not Lion._update_native


def test_cli_parser_and_engine_resolution(monkeypatch):
    from ldnn import cli
    from ldnn.models.mlp import mlp2

    assert cli.build_parser().parse_args([]).optimizer == "adam"
    model, dev = mlp2(), torch.device("cpu")
    monkeypatch.setattr(cli, "native_gpu", lambda d: True)   # (as on a GPU host with the extension)
    a = cli.build_parser().parse_args(["--engine", "static", "--optimizer", "lion"])
    assert a.optimizer == "lion"
    with pytest.raises(SystemExit, match="--optimizer lion runs on the autograd path"):
        cli.resolve_engine(a, model, dev, 1)
    a.engine = "auto"
    assert cli.resolve_engine(a, model, dev, 1) is False
    a.optimizer = "adam"
    assert cli.resolve_engine(a, model, dev, 1) is True


def test_cli_metrics_fields(tmp_path):
    from ldnn.cli import main

    main(["--model", "mlp2", "--dataset", "mnist", "--n_train", "400", "--n_test", "80", "--epochs_global", "1",
          "--epochs_local", "1", "--device", "cpu", "--quiet", "--out_dir", str(tmp_path), "--plots", "", "--no_eval",
          "--optimizer", "lion", "--lr", "0.0001", "--weight_decay", "0.1", "--clip_grad_norm", "1.0",
          "--ema_decay", "0.999", "--lr_schedule", "cosine", "--warmup_steps", "2", "--lr_min_ratio", "0.1"])
    recs = [json.loads(l) for l in open(tmp_path / "metrics.rank0.jsonl")]
    ge = [r for r in recs if r.get("kind") == "global_epoch"]
    assert ge
    for r in ge:
        assert {"grad_norm_last", "grad_clipped_steps", "grad_skipped_steps", "ema_updates", "ema_a_last", "lr_last",
                "lr_sched_steps"} <= set(r)
        assert not any(k.startswith(("lamb_", "lars_")) for k in r)
        assert r["ema_updates"] == r["lr_sched_steps"] > 0 and 0 < r["lr_last"] <= 1e-4


# ---------------------------------------------------------------- 6. data parallel (FakeWorld)
def _dp_train(comm, shard, lion, clip, steps=3, batch=6):
    m = build_model("lenet5")
    m.load_state_dict(INIT)
    ldnn.prepare(m, "cpu")
    dp = DataParallel(m, comm, bucket_cap_mb=0.05, shard_optimizer=shard)
    opt = (Lion(m.parameters(), lr=LR, weight_decay=WD, max_grad_norm=clip) if lion else
           Adam(m.parameters(), lr=LR, weight_decay=WD, max_grad_norm=clip))
    g = torch.Generator().manual_seed(10 + comm.rank)
    crit = CrossEntropyLoss()
    n0 = comm.schedule_digest()[0]
    for _ in range(steps):
        x = torch.randn(batch, 1, 28, 28, generator=g)
        y = torch.randint(0, 10, (batch,), generator=g)
        opt.zero_grad()
        (crit(dp(x), y) * 20.0).backward()
        dp.finish_gradient_sync()
        opt.step()
    nops = comm.schedule_digest()[0] - n0
    comm.check_schedule("end of test")
    dp.gather_master(opt)       # (every flat-shaped state tensor comes along: exp_avg is whole afterwards)
    st = {k: v.clone() for k, v in m.state_dict().items()}
    f = opt._flat_for_group(opt.param_groups[0])
    mom = {s.name: f.storage_view(s, opt._ls()["exp_avg"]).clone() for s in f.segments}
    return st, mom, nops


@pytest.mark.parametrize("clip", [None, 1.0])
@pytest.mark.parametrize("world", [2, 3])
def test_sharded_lion_equals_unsharded(world, clip):
    """Weights and the gathered moment; tolerance of tests/test_lamb.py::test_sharded_lamb_equals_unsharded
    (one flipped sign would be off by 2 lr = 2e-3)."""
    sh = FakeWorld(world).run(_dp_train, True, True, clip)
    ref = FakeWorld(world).run(_dp_train, False, True, clip)
    for r in range(world):
        for k, v in ref[r][0].items():
            torch.testing.assert_close(sh[r][0][k].float(), v.float(), rtol=1e-5, atol=1e-6, msg=k)
        for k, v in ref[r][1].items():
            torch.testing.assert_close(sh[r][1][k], v, rtol=1e-5, atol=1e-6, msg=k)
            assert bool((v != 0).any()), k
        for k, v in sh[0][0].items():
            assert torch.equal(sh[r][0][k], v), k              # replicas identical


def test_sharded_lion_adds_no_all_reduce_and_one_with_clipping():
    N, steps = 3, 3
    off = FakeWorld(N).run(_dp_train, True, False, None)
    lion = FakeWorld(N).run(_dp_train, True, True, None)
    both = FakeWorld(N).run(_dp_train, True, True, 1.0)
    unsh_off = FakeWorld(N).run(_dp_train, False, False, None)
    unsh_on = FakeWorld(N).run(_dp_train, False, True, 1.0)
    for r in range(N):
        assert lion[r][2] == off[r][2]                 # no collective of its own (check_schedule passed)
        assert both[r][2] - off[r][2] == steps         # clipping's scalar, nothing else
        assert unsh_on[r][2] == unsh_off[r][2]         # the unsharded path needs none


# ---------------------------------------------------------------- 7. EMA
@pytest.mark.parametrize("flat", [True, False])
def test_ema_rides_along_and_counts_the_non_skipped_steps(flat):
    d = 0.5
    m = _lenet(flat)
    o = Lion(m.parameters(), lr=LR, max_grad_norm=1.0, ema_decay=d, ema_warmup=False)
    g = torch.Generator().manual_seed(6)
    want = [p.detach().double().clone() for p in m.parameters()]
    for i in range(4):
        x, y = _batch(g)
        _backward(m, o, x, y)
        if i == 2:
            next(iter(m.parameters())).grad.view(-1)[0] = float("nan")
        o.step()
        if i != 2:
            want = [e + (1 - d) * (p.detach().double() - e) for e, p in zip(want, m.parameters())]
    assert int(o.ema_stats()["updates"]) == 3 and int(o.grad_clip_stats()["skipped"]) == 1
    live = _params(m)
    with o.ema_weights():
        for p, e in zip(m.parameters(), want):
            torch.testing.assert_close(p.detach(), e.float(), rtol=1e-5, atol=1e-6)
    for p, q in zip(m.parameters(), live):
        assert torch.equal(p.detach(), q)
    if flat:
        assert o.state_dict()["ldnn_flat_state"]["ema_updates"] == 3
