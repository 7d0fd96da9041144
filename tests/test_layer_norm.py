"""LayerNorm as the MLPs' normalisation layer (``norm="layer"``): module surface, model layout,
refusals, and the property it exists for -- a result that does not depend on which samples share
a batch -- on the CPU path (F.layer_norm in fp32)."""
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import ldnn
from ldnn.models import CrossEntropyLoss, build_model, xavier_init
from ldnn.models.layers import Dropout, LayerNorm, Linear
from ldnn.models.mlp import MLP, mlp3
from ldnn.optim import SGD, Lamb
from ldnn.parallel.comm import FakeWorld
from ldnn.parallel.ddp import DataParallel

ACT = {"none": lambda t: t, "relu": F.relu, "sigmoid": torch.sigmoid}


@pytest.mark.parametrize("act", ["none", "relu", "sigmoid"])
def test_act_equals_torch_layer_norm(act):
    torch.manual_seed(0)
    ln = LayerNorm(33)
    with torch.no_grad():
        ln.weight.copy_(1 + 0.3 * torch.randn(33))
        ln.bias.copy_(0.2 * torch.randn(33))
    x = torch.randn(5, 33, requires_grad=True)
    y = ln.act(x, act)
    xr = x.detach().clone().requires_grad_()
    w, b = ln.weight.detach().clone().requires_grad_(), ln.bias.detach().clone().requires_grad_()
    yr = ACT[act](F.layer_norm(xr, (33,), w, b, 1e-5))
    torch.testing.assert_close(y, yr, rtol=1e-5, atol=1e-6)
    dy = torch.randn_like(yr)
    y.backward(dy)
    yr.backward(dy)
    for a, e in ((x.grad, xr.grad), (ln.weight.grad, w.grad), (ln.bias.grad, b.grad)):
        torch.testing.assert_close(a, e, rtol=1e-5, atol=1e-6)
    torch.testing.assert_close(ln(x), F.layer_norm(x, (33,), ln.weight, ln.bias, ln.eps), rtol=1e-5, atol=1e-6)


def test_module_surface():
    ln = LayerNorm(16)
    assert isinstance(ln, nn.LayerNorm) and ln.eps == 1e-5 and ln.normalized_shape == (16,)
    assert ln._ldnn_flat is None and list(ln.buffers()) == []
    assert [n for n, _ in ln.named_parameters()] == ["weight", "bias"]
    plain = LayerNorm(8, elementwise_affine=False)
    assert list(plain.parameters()) == []
    x = torch.randn(3, 8)
    torch.testing.assert_close(plain.act(x, "relu"), F.relu(F.layer_norm(x, (8,))), rtol=1e-5, atol=1e-6)
    with pytest.raises(ValueError):
        LayerNorm((4, 8))          # one trailing dimension only
    with pytest.raises(ValueError):
        ln.act(torch.randn(3, 8))  # the wrong width
    with pytest.raises(KeyError):
        ln.act(torch.randn(3, 16), "tanh")


def test_model_layout():
    base = mlp3(784, 64, 10)
    assert [n for n, _ in base.named_modules()] == ["", "layers", "layers.0", "layers.1", "layers.2"]
    keys = ["layers.0.weight", "layers.0.bias", "layers.1.weight", "layers.1.bias", "layers.2.weight",
            "layers.2.bias"]
    assert list(base.state_dict()) == keys
    assert [l.activation for l in base.layers] == ["relu", "relu", "none"]
    assert list(mlp3(784, 64, 10, norm="batch").state_dict()) == keys
    assert list(build_model("mlp3").state_dict()) == keys

    m = mlp3(784, 64, 10, norm="layer")
    assert list(m.buffers()) == []
    assert sorted(m.state_dict()) == sorted(keys + ["norms.0.weight", "norms.0.bias", "norms.1.weight",
                                                    "norms.1.bias"])
    assert [n for n, _ in m.named_modules()] == ["", "layers", "layers.0", "layers.1", "layers.2", "norms",
                                                 "norms.0", "norms.1"]
    assert [l.activation for l in m.layers] == ["none", "none", "none"]   # the norms carry the activation
    assert all(isinstance(n, LayerNorm) and n.normalized_shape == (64,) for n in m.norms)
    for k in keys:
        assert m.state_dict()[k].shape == base.state_dict()[k].shape
    for name in ("mlp2", "mlp3"):
        built = build_model(name, norm="layer")
        assert len(built.norms) == len(built.layers) - 1 and list(built.buffers()) == []
    with pytest.raises(ValueError):
        MLP(70, (33,), 10, norm="group")


def test_forward_is_linear_norm_activation():
    torch.manual_seed(0)
    m = MLP(70, (33,), 10, activation="sigmoid", norm="layer")
    x = torch.randn(6, 70)
    l0, l1, n0 = m.layers[0], m.layers[1], m.norms[0]
    h = torch.sigmoid(F.layer_norm(F.linear(x, l0.weight, l0.bias), (33,), n0.weight, n0.bias, n0.eps))
    torch.testing.assert_close(m(x), F.linear(h, l1.weight, l1.bias), rtol=1e-5, atol=1e-6)


def test_refusals():
    for name in ("enhanced_cnn_small", "enhanced_cnn", "resnet18_cifar", "lenet5"):
        with pytest.raises(ValueError):
            build_model(name, norm="layer")
    with pytest.raises(ValueError):
        build_model("mlp3", norm="instance")
    from ldnn.cli import build_parser, main
    assert build_parser().parse_args(["--norm", "layer"]).norm == "layer"
    for model in ("lenet5", "enhanced_cnn_small"):
        with pytest.raises(SystemExit, match="--norm layer"):
            main(["--norm", "layer", "--model", model, "--device", "cpu"])
    with pytest.raises(SystemExit):
        main(["--engine", "static", "--norm", "layer", "--model", "mlp3", "--device", "cpu"])
    from ldnn.train.static_mlp import StaticMLPEngine
    with pytest.raises(ValueError, match="autograd path"):   # the engine itself, not only the command line
        StaticMLPEngine(mlp3(784, 64, 10, norm="layer"), 8)


def test_static_engine_refuses_layer_norm_and_auto_falls_back():
    import argparse

    from ldnn.cli import resolve_engine

    def args(engine):
        return argparse.Namespace(engine=engine, model="mlp3", grad_comm_dtype="fp32", legacy_gossip=False,
                                  sync_every="global_epoch", topology="allreduce", norm="layer")

    import ldnn.cli as cli
    real = cli.native_gpu
    cli.native_gpu = lambda dev: True   # (the refusal under test comes after the device check)
    try:
        with pytest.raises(SystemExit, match="--norm layer runs on the autograd path"):
            resolve_engine(args("static"), mlp3(784, 64, 10, norm="layer"), torch.device("cpu"), 1)
        assert resolve_engine(args("auto"), mlp3(784, 64, 10, norm="layer"), torch.device("cpu"), 1) is False
    finally:
        cli.native_gpu = real


def _small(**kw):
    return MLP(70, (33,), 10, norm="layer", **kw)


torch.manual_seed(0)
_INIT = _small()
xavier_init(_INIT)
with torch.no_grad():   # (LayerNorm's own init is gamma = 1, beta = 0: move off it)
    _INIT.norms[0].weight.add_(0.3 * torch.randn(33))
    _INIT.norms[0].bias.add_(0.2 * torch.randn(33))
_INIT = _INIT.state_dict()
_G = torch.Generator().manual_seed(3)
_XS = [torch.randn(4, 70, generator=_G) for _ in range(3)]
_YS = [torch.randint(0, 10, (4,), generator=_G) for _ in range(3)]


def _dp_train(comm, shard):
    m = _small()
    m.load_state_dict(_INIT)
    ldnn.prepare(m, "cpu")
    dp = DataParallel(m, comm, bucket_cap_mb=0.005, shard_optimizer=shard)
    opt = SGD(m.parameters(), lr=0.05, momentum=0.9)
    crit = CrossEntropyLoss()
    lo, hi = comm.rank * 2, comm.rank * 2 + 2
    for x, y in zip(_XS, _YS):
        opt.zero_grad()
        crit(dp(x[lo:hi]), y[lo:hi]).backward()
        dp.finish_gradient_sync()
        opt.step()
    dp.gather_master(opt)
    kinds = [b["sharded"] for b in dp.bucketer.buckets]
    tail = [s.name for s in dp.flat.segments if s.param.dim() == 1]
    return kinds, {k: v.clone() for k, v in m.state_dict().items()}, tail


@pytest.mark.parametrize("shard", [False, True])
def test_per_step_dp_on_half_batches_equals_one_process_on_the_whole_batch(shard):
    one = _small()
    one.load_state_dict(_INIT)
    ldnn.prepare(one, "cpu")
    opt = SGD(one.parameters(), lr=0.05, momentum=0.9)
    crit = CrossEntropyLoss()
    for x, y in zip(_XS, _YS):
        opt.zero_grad()
        crit(one(x), y).backward()
        opt.step()
    assert not torch.equal(one.state_dict()["norms.0.weight"], _INIT["norms.0.weight"])
    res = FakeWorld(2).run(_dp_train, shard)
    for r in range(2):
        kinds, sd, tail = res[r]
        if shard:   # LayerNorm affine are 1-D: they sit in the replicated tail bucket
            assert kinds[-1] is False and any(kinds), kinds
            assert "norms.0.weight" in tail and "norms.0.bias" in tail
        for k, v in one.state_dict().items():
            torch.testing.assert_close(sd[k], v, rtol=1e-5, atol=1e-6, msg=k)


def test_checkpoint_round_trip(tmp_path):
    from ldnn.utils.checkpoint import Checkpointer, load_checkpoint

    m = _small()
    m.load_state_dict(_INIT)
    ldnn.prepare(m, "cpu")
    opt = SGD(m.parameters(), lr=0.05, momentum=0.9)
    x, y = _XS[0], _YS[0]
    opt.zero_grad()
    CrossEntropyLoss()(m(x), y).backward()
    opt.step()
    path = Checkpointer(str(tmp_path)).save(1, m, opt)
    m2 = _small()
    ldnn.prepare(m2, "cpu")
    opt2 = SGD(m2.parameters(), lr=0.05, momentum=0.9)
    load_checkpoint(path, m2, opt2)
    assert list(m2.state_dict()) == list(m.state_dict())
    for k, v in m.state_dict().items():
        assert torch.equal(m2.state_dict()[k], v), k
    for o, mm in ((opt, m), (opt2, m2)):   # and the resumed run takes the same next step
        o.zero_grad()
        CrossEntropyLoss()(mm(x), y).backward()
        o.step()
    for k, v in m.state_dict().items():
        torch.testing.assert_close(m2.state_dict()[k], v, rtol=0, atol=0, msg=k)
    with pytest.raises(Exception):   # a checkpoint of the model without norms is not silently accepted
        m2.load_state_dict(MLP(70, (33,), 10).state_dict())


def test_one_d_treatment_under_the_optimizers():
    """LayerNorm affine are 1-D like biases: excluded from LARS / LAMB trust ratios; clipping, weight
    decay and the EMA run; every parameter moves and stays finite."""
    x, y = _XS[0], _YS[0]
    for mk, stats in ((lambda p: SGD(p, lr=0.05, momentum=0.9, weight_decay=5e-4, max_grad_norm=1.0, lars_trust=0.02,
                                     ema_decay=0.9), "lars_stats"),
                      (lambda p: Lamb(p, lr=1e-3, weight_decay=1e-2, max_grad_norm=1.0, ema_decay=0.9), "lamb_stats")):
        m = _small()
        m.load_state_dict(_INIT)
        ldnn.prepare(m, "cpu")
        opt = mk(m.parameters())
        before = [p.detach().clone() for p in m.parameters()]
        for _ in range(2):
            opt.zero_grad()
            CrossEntropyLoss()(m(x), y).backward()
            opt.step()
        for (n, p), b in zip(m.named_parameters(), before):
            assert torch.isfinite(p).all() and not torch.equal(p, b), n
        st = getattr(opt, stats)()
        adapted = dict(zip(st["names"], st["adapted"]))
        assert adapted["norms.0.weight"] is False and adapted["norms.0.bias"] is False
        assert adapted["layers.0.bias"] is False and adapted["layers.0.weight"] is True


def test_train_mode_equals_eval_mode_and_dropout_order():
    torch.manual_seed(0)
    m = _small()
    x = torch.randn(4, 70)
    with torch.no_grad():
        assert torch.equal(m.train()(x), m.eval()(x))
    d = _small(dropout=0.3)
    assert [type(c) for c in (d.layers[0], d.norms[0], d.drops[0])] == [Linear, LayerNorm, Dropout]
    from ldnn.models import reseed_dropout
    reseed_dropout(d, 7)
    seen = []
    d.drops[0].register_forward_hook(lambda mod, inp, out: seen.append((inp[0].detach(), out.detach())))
    d.train()
    CrossEntropyLoss()(d(x), torch.randint(0, 10, (4,))).backward()
    (h, out), = seen
    # dropout sees the normalised, activated rows: Linear -> LayerNorm + ReLU -> Dropout
    l0, n0 = d.layers[0], d.norms[0]
    want = F.relu(F.layer_norm(F.linear(x, l0.weight, l0.bias), (33,), n0.weight, n0.bias, n0.eps))
    torch.testing.assert_close(h, want, rtol=1e-5, atol=1e-6)
    dropped = (out == 0) & (h != 0)
    assert 0 < dropped.float().mean().item() < 0.7
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in d.parameters())
    with torch.no_grad():
        assert torch.equal(d.eval()(x), d.eval()(x))
