"""FedProx (``prox_mu``: ``mu * (w - anchor)`` added to the gradient inside the optimizers), CPU paths:
the torch-op twins against torch.optim fed the proximal gradient, off == absent, clipping does not see
the term, the refusals, ``train_global``'s anchor and drift metric, sharded == replicated on two gloo
ranks."""
import math
import os
import sys

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import ldnn
from ldnn.data.loader import get_loaders
from ldnn.models import CrossEntropyLoss, build_model, xavier_init
from ldnn.models.mlp import mlp2
from ldnn.optim import SGD, Adam, AdamW, Lamb, Lion, StepLR, build_optimizer
from ldnn.parallel.comm import FakeWorld
from ldnn.train.trainer import train_global
from ldnn.utils.flat_params import FlatParams

from test_sharded_dp import INIT, SHAPES, _port     # (helpers of the sharded-vs-replicated test)

MU = 0.1
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _pair(flat):
    torch.manual_seed(0)
    m, r = mlp2(784, 32, 10), mlp2(784, 32, 10)
    r.load_state_dict(m.state_dict())
    if flat:
        FlatParams(m, "cpu")
    return m, r


def _batch():
    return torch.randn(16, 784), torch.randint(0, 10, (16,))


def _backward(mod, opt, x, y, scale=1.0):
    opt.zero_grad()
    (torch.nn.functional.cross_entropy(mod(x), y) * scale).backward()


# ---------------------------------------------------------------- 1. the torch twins
@pytest.mark.parametrize("Opt,TOpt,kw", [
    (SGD, torch.optim.SGD, dict(lr=0.1, weight_decay=1e-4)),
    (SGD, torch.optim.SGD, dict(lr=0.1, momentum=0.9, weight_decay=1e-4)),
    (SGD, torch.optim.SGD, dict(lr=0.1, momentum=0.9, nesterov=True)),
    (Adam, torch.optim.Adam, dict(lr=1e-2, weight_decay=1e-3)),
    (AdamW, torch.optim.AdamW, dict(lr=1e-2, weight_decay=1e-2)),
], ids=["sgd", "sgd_momentum", "sgd_nesterov", "adam", "adamw"])
@pytest.mark.parametrize("flat", [True, False], ids=["flat", "loose"])
def test_prox_step_matches_torch_fed_the_proximal_gradient(Opt, TOpt, kw, flat):
    """Three steps, mu = 0.1, against torch.optim stepping ``p.grad = g + mu * (p - a)`` with ``a`` the
    initial weights (no explicit anchor: the first step anchors at the master before its update).
    Bound: rtol 1e-5 / atol 1e-6, taken from tests/test_optim_models.py::test_optimizer_matches_torch."""
    m, r = _pair(flat)
    o, ro = Opt(m.parameters(), prox_mu=MU, **kw), TOpt(r.parameters(), **kw)
    anchor = [p.detach().clone() for p in r.parameters()]
    for _ in range(3):
        x, y = _batch()
        _backward(m, o, x, y)
        _backward(r, ro, x, y)
        for p, a in zip(r.parameters(), anchor):
            p.grad.add_(MU * (p.detach() - a))
        o.step()
        ro.step()
    for a, b, a0 in zip(m.parameters(), r.parameters(), anchor):
        torch.testing.assert_close(a.detach(), b.detach(), rtol=1e-5, atol=1e-6)
        assert not torch.equal(b.detach(), a0)
    st = o.prox_stats()
    drift = math.sqrt(sum(float((p.detach().double() - a.double()).square().sum())
                          for p, a in zip(m.parameters(), anchor)))
    assert st["mu"] == MU and st["drift_norm"] == pytest.approx(drift, rel=1e-6) and drift > 0


@pytest.mark.parametrize("wd", [0.0, 1e-2])
@pytest.mark.parametrize("flat", [True, False], ids=["flat", "loose"])
def test_prox_lion_matches_the_fp64_formula(flat, wd):
    """Lion, three steps, mu = 0.1, against the formula in fp64 fed the very fp32 gradients the model
    under test computed: g += mu (p0 - a); c = b1 m + (1 - b1) g; w = w (1 - lr wd) - lr sign(c);
    m = b2 m + (1 - b2) g.  Bound: rtol 1e-5 / atol 1e-6 with no undecided sign, taken from
    tests/test_lion.py::test_lion_steps_match_the_oracle (a flipped sign would be off by 2 lr)."""
    lr, b1, b2 = 1e-3, 0.9, 0.99
    m, _ = _pair(flat)
    o = Lion(m.parameters(), lr=lr, betas=(b1, b2), weight_decay=wd, prox_mu=MU)
    w = [p.detach().double().clone() for p in m.parameters()]
    a = [v.clone() for v in w]
    mom = [torch.zeros_like(v) for v in w]
    undecided = 0
    for _ in range(3):
        x, y = _batch()
        _backward(m, o, x, y)
        for i, p in enumerate(m.parameters()):
            g = p.grad.detach().double() + MU * (w[i] - a[i])
            c = b1 * mom[i] + (1 - b1) * g
            undecided += int(((c != 0) & (c.abs() <= 4 * 2.0 ** -24 * ((b1 * mom[i]).abs() + ((1 - b1) * g).abs()))).sum())
            w[i] = w[i] * (1 - lr * wd) - lr * torch.sign(c)
            mom[i] = b2 * mom[i] + (1 - b2) * g
        o.step()
    assert undecided == 0       # (else a sign may legitimately differ: pick another seed)
    for p, v in zip(m.parameters(), w):
        torch.testing.assert_close(p.detach(), v.float(), rtol=1e-5, atol=1e-6)


def test_set_prox_anchor_moves_the_anchor_in_place():
    m, _ = _pair(True)
    o = SGD(m.parameters(), lr=0.1, prox_mu=MU)
    assert o.prox_stats() == {"mu": MU, "drift_norm": None}
    o.set_prox_anchor()
    a = o._ls()["prox_anchor"]
    f = o._flat_for_group(o.param_groups[0])
    assert a.dtype == torch.float32 and a.shape == f.master.shape and torch.equal(a, f.master)
    _backward(m, o, *_batch())
    o.step()
    assert not torch.equal(a, f.master) and o.prox_stats()["drift_norm"] > 0
    o.set_prox_anchor()
    assert o._ls()["prox_anchor"] is a and torch.equal(a, f.master) and o.prox_stats()["drift_norm"] == 0.0
    o.param_groups[0]["ema_decay"] = 0.9
    _backward(m, o, *_batch())
    o.step()
    with o.ema_weights():
        with pytest.raises(RuntimeError, match="ema_weights"):
            o.set_prox_anchor()
    o._ldnn_capturing = True
    try:
        with pytest.raises(RuntimeError, match="capture"):
            o.set_prox_anchor()
    finally:
        o._ldnn_capturing = False


# ---------------------------------------------------------------- 2. off == absent
@pytest.mark.parametrize("Opt,kw", [(SGD, dict(lr=0.1, momentum=0.9, weight_decay=1e-4)), (Adam, dict(lr=1e-2)),
                                    (AdamW, dict(lr=1e-2)), (Lion, dict(lr=1e-3))],
                         ids=["sgd", "adam", "adamw", "lion"])
@pytest.mark.parametrize("mu", [0, 0.0, None])
@pytest.mark.parametrize("flat", [True, False], ids=["flat", "loose"])
def test_prox_off_is_the_optimizer_without_the_keyword(Opt, kw, mu, flat):
    res = []
    for extra in (dict(prox_mu=mu), {}):
        m, _ = _pair(flat)
        o = Opt(m.parameters(), **kw, **extra)
        torch.manual_seed(3)
        for _ in range(3):
            _backward(m, o, *_batch())
            o.step()
        res.append(([p.detach().clone() for p in m.parameters()], o))
    for a, b in zip(res[0][0], res[1][0]):
        assert torch.equal(a, b)
    on, off = res[0][1], res[1][1]
    assert "prox_anchor" not in on._ls() and "prox_hdr" not in on._ls() and sorted(on._ls()) == sorted(off._ls())
    assert all("prox_anchor" not in st for st in on.state.values())
    sd, sd0 = on.state_dict(), off.state_dict()
    assert sorted(sd) == sorted(sd0) and sorted(sd["ldnn_flat_state"]) == sorted(sd0["ldnn_flat_state"])
    assert on.prox_stats() == {"mu": 0.0, "drift_norm": None}
    with pytest.raises(RuntimeError, match="off"):
        on.set_prox_anchor()


@pytest.mark.parametrize("flat", [True, False], ids=["flat", "loose"])
def test_state_dict_keys_do_not_change_with_prox_on(flat):
    """The anchor is not checkpointed: the next global epoch re-anchors."""
    keys = []
    for extra in (dict(prox_mu=MU), {}):
        m, _ = _pair(flat)
        o = Adam(m.parameters(), lr=1e-2, **extra)
        _backward(m, o, *_batch())
        o.step()
        sd = o.state_dict()
        keys.append((sorted(sd), sorted(sd["ldnn_flat_state"]), sorted(sorted(v) for v in sd["state"].values())))
        if extra and not flat:      # (the live per-tensor state keeps its anchors)
            assert all("prox_anchor" in st for st in o.state.values())
    assert keys[0] == keys[1]


# ---------------------------------------------------------------- 3. clipping
@pytest.mark.parametrize("flat", [True, False], ids=["flat", "loose"])
def test_clip_norm_and_guard_do_not_see_the_proximal_term(flat):
    from ldnn.optim.optimizers import _CLIP_COEF

    stats = []
    for mu in (MU, None):
        m, _ = _pair(flat)
        o = SGD(m.parameters(), lr=0.1, momentum=0.9, max_grad_norm=0.5, prox_mu=mu)
        if mu is not None:
            o.set_prox_anchor()
            anchors = [o._ls()["prox_anchor"]] if flat else [o.state[p]["prox_anchor"] for p in m.parameters()]
            for a in anchors:
                a.add_(1e3)      # a = w + 1e3: the term dwarfs the gradient
        torch.manual_seed(5)
        _backward(m, o, *_batch(), scale=20.0)
        o.step()
        cs = o.grad_clip_stats()
        stats.append((float(cs["last_norm"]), float(o._ls()["clip"][_CLIP_COEF]), int(cs["clipped"])))
    assert stats[0] == stats[1] and stats[0][2] == 1 and stats[0][1] < 1.0
    # (the optimizer with the term: a non-finite gradient changes nothing, the anchor included)
    m, _ = _pair(flat)
    o = SGD(m.parameters(), lr=0.1, momentum=0.9, max_grad_norm=0.5, prox_mu=MU)
    _backward(m, o, *_batch())
    o.step()
    o.set_prox_anchor()
    _backward(m, o, *_batch())
    o.step()

    def snapshot():
        ls = [v.clone() for k, v in sorted(o._ls().items()) if k in ("momentum", "prox_anchor")]
        per = [t.clone() for p in m.parameters() for _, t in sorted(o.state.get(p, {}).items()) if torch.is_tensor(t)]
        return [p.detach().clone() for p in m.parameters()] + ls + per

    before = snapshot()
    assert len(before) >= len(list(m.parameters())) + (2 if flat else 2 * len(list(m.parameters())))
    _backward(m, o, *_batch())
    next(iter(m.parameters())).grad.view(-1)[0] = float("inf")
    o.step()
    assert int(o.grad_clip_stats()["skipped"]) == 1
    for a, b in zip(before, snapshot()):
        assert torch.equal(a, b)


# ---------------------------------------------------------------- 4. refusals
def test_refusals():
    m, _ = _pair(True)
    with pytest.raises(ValueError, match="prox"):
        Lamb(m.parameters(), prox_mu=MU)
    with pytest.raises(ValueError, match="prox"):
        SGD(m.parameters(), lars_trust=0.001, prox_mu=MU)
    with pytest.raises(ValueError, match="prox"):
        build_optimizer("lars", m.parameters(), 0.1, prox_mu=MU)
    with pytest.raises(ValueError, match="prox"):
        build_optimizer("lamb", m.parameters(), 0.1, prox_mu=MU)
    Lamb(m.parameters(), prox_mu=0)
    SGD(m.parameters(), lars_trust=0.001, prox_mu=None)
    for Opt in (SGD, Adam, AdamW, Lion):
        for bad in (-0.1, float("nan"), float("inf"), "0.1", True):
            with pytest.raises(ValueError, match="prox_mu"):
                Opt(m.parameters(), prox_mu=bad)
    for name in ("sgd", "adam", "adamw", "lion"):
        assert build_optimizer(name, m.parameters(), 0.1, prox_mu=MU).param_groups[0]["prox_mu"] == MU
    loose, _ = _pair(False)
    lp = list(loose.parameters())
    with pytest.raises(ValueError, match="same in every param group"):
        SGD([dict(params=lp[:2], prox_mu=0.1), dict(params=lp[2:], prox_mu=0.2)], lr=0.1)
    o = SGD([dict(params=lp[:2]), dict(params=lp[2:])], lr=0.1, prox_mu=MU)
    o.param_groups[1]["prox_mu"] = 0.3
    with pytest.raises(ValueError, match="same in every param group"):
        o.step()


@pytest.mark.parametrize("argv", [["--optimizer", "lars"], ["--optimizer", "lamb"], ["--engine", "static"]],
                         ids=["lars", "lamb", "static"])
def test_cli_refusals(argv, tmp_path):
    from ldnn.cli import main

    with pytest.raises(SystemExit, match="fedprox_mu"):
        main(["--model", "mlp2", "--dataset", "mnist", "--n_train", "200", "--n_test", "40", "--device", "cpu",
              "--quiet", "--out_dir", str(tmp_path), "--plots", "", "--no_eval", "--fedprox_mu", "0.01"] + argv)


@pytest.mark.parametrize("bad", ["-1", "nan", "inf"])
def test_cli_range_check(bad, tmp_path):
    from ldnn.cli import main

    with pytest.raises(SystemExit, match="--fedprox_mu must be finite"):
        main(["--device", "cpu", "--out_dir", str(tmp_path), "--fedprox_mu", bad])


def test_cli_engine_resolution(monkeypatch):
    from ldnn import cli

    assert cli.build_parser().parse_args([]).fedprox_mu == 0.0
    model, dev = mlp2(), torch.device("cpu")
    monkeypatch.setattr(cli, "native_gpu", lambda d: True)   # (as on a GPU host with the extension)
    a = cli.build_parser().parse_args(["--engine", "static", "--optimizer", "sgd", "--fedprox_mu", "0.01"])
    with pytest.raises(SystemExit, match="--fedprox_mu runs on the autograd path"):
        cli.resolve_engine(a, model, dev, 1)
    a.engine = "auto"
    assert cli.resolve_engine(a, model, dev, 1) is False
    a.fedprox_mu = 0.0
    assert cli.resolve_engine(a, model, dev, 1) is True


# ---------------------------------------------------------------- 5. train_global
class _Log:
    def __init__(self):
        self.recs = []

    def log(self, **kw):
        self.recs.append(kw)


def _train_global(mu, Eg=2, El=2):
    comm = FakeWorld(1).comm(0)
    torch.manual_seed(0)
    model = mlp2(784, 32, 10)
    xavier_init(model)
    ldnn.prepare(model, "cpu")
    loaders = get_loaders(32, 1, 0, model, "cpu", None, dataset="mnist", comm=comm, n_train=600, n_test=100,
                          partition_rule="equal")
    tr, va, te, trainset, valset, ti, vi = loaders[:7]
    opt = SGD(model.parameters(), lr=0.05, momentum=0.9, prox_mu=mu)
    calls = []
    orig = opt.set_prox_anchor
    opt.set_prox_anchor = lambda: (calls.append(opt._ls().get("step", 0)), orig())[1]
    log = _Log()
    train_global(model, tr, va, trainset, valset, ti, vi, CrossEntropyLoss(), opt, StepLR(opt, step_size=25), "cpu", 0,
                 1, El, Eg, float("inf"), 32, 0.5, 0.5, 0.5, "equal", "gradients", comm=comm, progress=False,
                 verbose=False, logger=log)
    return [r for r in log.recs if r.get("kind") == "global_epoch"], calls, opt


def test_train_global_anchors_every_global_epoch_and_logs_the_drift():
    weak, calls, opt = _train_global(1e-6)
    strong, calls2, _ = _train_global(1.0)
    assert len(weak) == len(strong) == 2
    steps = opt._ls()["step"]
    assert calls == calls2 == [0, steps // 2]      # once per global epoch, before its first step
    for w, s in zip(weak, strong):
        assert w["prox_mu"] == 1e-6 and s["prox_mu"] == 1.0
        assert math.isfinite(w["prox_drift_norm"]) and math.isfinite(s["prox_drift_norm"])
        assert 0 < s["prox_drift_norm"] < w["prox_drift_norm"]
    off, calls3, _ = _train_global(None)
    assert calls3 == [] and all("prox_mu" not in r and "prox_drift_norm" not in r for r in off)


# ---------------------------------------------------------------- 6. sharded == replicated, two gloo ranks
def _gloo_worker(rank, world, port, out, shard):
    import datetime

    sys.path.insert(0, ROOT)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world, timeout=datetime.timedelta(seconds=60))
    from ldnn.parallel.comm import TorchComm
    from ldnn.parallel.ddp import DataParallel

    name = "lenet5"
    m = build_model(name)
    m.load_state_dict(INIT[name])
    ldnn.prepare(m, "cpu")
    dp = DataParallel(m, TorchComm(), bucket_cap_mb=0.05, shard_optimizer=shard)
    opt = SGD(m.parameters(), lr=0.05, momentum=0.9, prox_mu=MU)
    g = torch.Generator().manual_seed(10 + rank)
    crit = CrossEntropyLoss()
    for _ in range(3):
        x = torch.randn(6, *SHAPES[name], generator=g)
        y = torch.randint(0, 10, (6,), generator=g)
        opt.zero_grad()
        crit(dp(x), y).backward()
        dp.finish_gradient_sync()
        opt.step()
    dp.gather_master(opt)
    torch.save({"model": {k: v.detach().clone() for k, v in m.state_dict().items()},
                "drift": opt.prox_stats()["drift_norm"], "sharded": [b["sharded"] for b in dp.bucketer.buckets]},
               f"{out}.{rank}")
    dist.destroy_process_group()


def test_sharded_prox_step_equals_replicated_two_gloo_ranks(tmp_path):
    """SGD-momentum, mu = 0.1, three steps on LeNet-5.  Bound: rtol 1e-5 / atol 1e-6, the one
    tests/test_sharded_dp.py::test_sharded_step_equals_allreduce_step holds the masters to."""
    world, res = 2, {}
    for shard in (True, False):
        out = str(tmp_path / f"shard{int(shard)}.pt")
        mp.spawn(_gloo_worker, args=(world, _port(), out, shard), nprocs=world, join=True)
        res[shard] = [torch.load(f"{out}.{r}", weights_only=True) for r in range(world)]
    assert sum(res[True][0]["sharded"]) >= 1 and not any(res[False][0]["sharded"])
    for r in range(world):
        for k, v in res[False][r]["model"].items():
            torch.testing.assert_close(res[True][r]["model"][k].float(), v.float(), rtol=1e-5, atol=1e-6, msg=k)
            assert torch.equal(res[True][r]["model"][k], res[True][0]["model"][k]), k      # replicas identical
        assert res[True][r]["drift"] > 0
        assert res[True][r]["drift"] == pytest.approx(res[False][r]["drift"], rel=1e-4)
