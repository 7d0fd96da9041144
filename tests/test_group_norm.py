"""GroupNorm as the CNNs' normalisation layer (``norm="group"``): module surface, model layout,
refusals, and the property it exists for -- a result that does not depend on which samples share
a batch -- on the CPU path (F.group_norm in fp32)."""
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import ldnn
from ldnn.models import CrossEntropyLoss, build_model, xavier_init
from ldnn.models.layers import GroupNorm
from ldnn.optim import SGD, Lamb
from ldnn.parallel.comm import FakeWorld
from ldnn.parallel.ddp import DataParallel

BN_ONLY = ("running_mean", "running_var", "num_batches_tracked")


@pytest.mark.parametrize("relu,res", [(False, False), (True, False), (False, True), (True, True)])
def test_act_equals_torch_group_norm(relu, res):
    torch.manual_seed(0)
    gn = GroupNorm(4, 16)
    with torch.no_grad():
        gn.weight.copy_(1 + 0.3 * torch.randn(16))
        gn.bias.copy_(0.2 * torch.randn(16))
    x = torch.randn(3, 16, 5, 7, requires_grad=True)
    r = torch.randn(3, 16, 5, 7, requires_grad=True) if res else None
    y = gn.act(x, residual=r, relu=relu)
    xr = x.detach().clone().requires_grad_()
    rr = r.detach().clone().requires_grad_() if res else None
    w, b = gn.weight.detach().clone().requires_grad_(), gn.bias.detach().clone().requires_grad_()
    yr = F.group_norm(xr, 4, w, b, gn.eps)
    if res:
        yr = yr + rr
    if relu:
        yr = F.relu(yr)
    torch.testing.assert_close(y, yr, rtol=1e-5, atol=1e-6)
    dy = torch.randn_like(yr)
    y.backward(dy)
    yr.backward(dy)
    for a, e in ((x.grad, xr.grad), (gn.weight.grad, w.grad), (gn.bias.grad, b.grad)) + (((r.grad, rr.grad),) if res else ()):
        torch.testing.assert_close(a, e, rtol=1e-5, atol=1e-6)
    torch.testing.assert_close(gn(x), F.group_norm(x, 4, gn.weight, gn.bias, gn.eps), rtol=1e-5, atol=1e-6)


def test_affine_false_has_no_parameters():
    gn = GroupNorm(2, 8, affine=False)
    assert list(gn.parameters()) == []
    x = torch.randn(2, 8, 3, 3)
    torch.testing.assert_close(gn.act(x, relu=True), F.relu(F.group_norm(x, 2)), rtol=1e-5, atol=1e-6)


@pytest.mark.parametrize("name,n_keys,some", [
    ("enhanced_cnn_small", 62, ("prep.1.weight", "layer1.shortcut.1.bias", "layer3.bn2.weight")),
    ("resnet18_cifar", 122, ("bn1.weight", "layer2.0.downsample.1.weight", "layer4.1.bn2.bias"))])
def test_group_norm_models_keep_names_and_have_no_buffers(name, n_keys, some):
    bn, gn = build_model(name), build_model(name, norm="group")
    assert not any(isinstance(m, nn.BatchNorm2d) for m in gn.modules())
    assert sum(isinstance(m, GroupNorm) for m in gn.modules()) == sum(isinstance(m, nn.BatchNorm2d) for m in bn.modules())
    assert list(gn.buffers()) == []
    keys_bn = list(bn.state_dict())
    assert list(gn.state_dict()) == [k for k in keys_bn if not k.endswith(BN_ONLY)]
    assert [n for n, _ in gn.named_modules()] == [n for n, _ in bn.named_modules()]
    # the default model is the one from before the norm choice existed
    assert len(keys_bn) == n_keys and all(k in keys_bn for k in some)
    assert "prep.1.running_mean" in keys_bn or "bn1.running_mean" in keys_bn
    assert list(build_model(name, norm="batch").state_dict()) == keys_bn
    for m in gn.modules():
        if isinstance(m, GroupNorm):
            assert m.num_groups == 32


def test_refusals():
    with pytest.raises(ValueError, match="gn_groups"):
        build_model("enhanced_cnn_small", norm="group", gn_groups=48)
    for name in ("mlp3", "lenet5"):
        with pytest.raises(ValueError, match="no normalisation layer"):
            build_model(name, norm="group")
        build_model(name, norm="batch")
    with pytest.raises(ValueError):
        build_model("enhanced_cnn_small", norm="layer")
    from ldnn.cli import build_parser, main
    a = build_parser().parse_args([])
    assert (a.norm, a.gn_groups) == ("batch", 32)
    with pytest.raises(SystemExit, match="no normalisation layer"):
        main(["--norm", "group", "--model", "mlp3", "--device", "cpu"])
    with pytest.raises(SystemExit):
        main(["--engine", "static", "--norm", "group", "--model", "mlp3", "--device", "cpu"])
    with pytest.raises(SystemExit, match="gn_groups"):
        main(["--norm", "group", "--gn_groups", "48", "--model", "enhanced_cnn_small", "--device", "cpu"])


def test_static_engine_refuses_group_norm_and_auto_falls_back():
    import argparse

    from ldnn.cli import resolve_engine
    from ldnn.models import mlp3

    def args(engine):
        return argparse.Namespace(engine=engine, model="mlp3", grad_comm_dtype="fp32", legacy_gossip=False,
                                  sync_every="global_epoch", topology="allreduce", norm="group")

    import ldnn.cli as cli
    real = cli.native_gpu
    cli.native_gpu = lambda dev: True   # (the refusal under test comes after the device check)
    try:
        with pytest.raises(SystemExit, match="--norm group runs on the autograd path"):
            resolve_engine(args("static"), mlp3(784, 64, 10), torch.device("cpu"), 1)
        assert resolve_engine(args("auto"), mlp3(784, 64, 10), torch.device("cpu"), 1) is False
    finally:
        cli.native_gpu = real


def _grads(model, x, y):
    model.zero_grad()
    F.cross_entropy(model(x), y).backward()
    return [p.grad.detach().clone() for p in model.parameters()]


def _half_vs_full(norm):
    torch.manual_seed(0)
    m = build_model("enhanced_cnn_small", norm=norm)
    xavier_init(m)
    m.train()
    x, y = torch.randn(8, 3, 32, 32), torch.randint(0, 10, (8,))
    full = _grads(m, x, y)
    h0, h1 = _grads(m, x[:4], y[:4]), _grads(m, x[4:], y[4:])
    return full, [(a + b) / 2 for a, b in zip(h0, h1)]


def test_half_batch_gradients_average_to_the_full_batch_gradient():
    """The mean of two half-batch gradients is the full-batch gradient with GroupNorm (to fp32
    rounding), and is not with BatchNorm: that the same check sees the BatchNorm effect shows it
    can see one."""
    full, halves = _half_vs_full("group")
    for f, h in zip(full, halves):
        torch.testing.assert_close(h, f, rtol=1e-4, atol=1e-6 * f.abs().max().item())
    full, halves = _half_vs_full("batch")
    worst = max(((h - f).abs().max() / f.abs().max()).item() for f, h in zip(full, halves))
    assert worst > 1e-2, worst


def test_train_mode_equals_eval_mode():
    torch.manual_seed(0)
    m = build_model("enhanced_cnn_small", norm="group")
    x = torch.randn(4, 3, 32, 32)
    with torch.no_grad():
        a = m.train()(x)
        b = m.eval()(x)
    assert torch.equal(a, b)


torch.manual_seed(0)
_INIT = build_model("enhanced_cnn_small", norm="group")
xavier_init(_INIT)
_INIT = _INIT.state_dict()
# Small on purpose (batch 4, 16x16): two runs at different batch sizes agree only while no ReLU
# input lies within fp32 rounding of zero (the CPU convolutions pick their algorithm by batch size,
# and a flipped ReLU bit changes every gradient upstream of it by about one part in the number of
# positions); the fewer activations, the rarer that measure-zero event
_G = torch.Generator().manual_seed(3)
_XS = [torch.randn(4, 3, 16, 16, generator=_G) for _ in range(3)]
_YS = [torch.randint(0, 10, (4,), generator=_G) for _ in range(3)]


def _dp_train(comm, shard):
    m = build_model("enhanced_cnn_small", norm="group")
    m.load_state_dict(_INIT)
    ldnn.prepare(m, "cpu")
    dp = DataParallel(m, comm, bucket_cap_mb=0.05, shard_optimizer=shard)
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
    one = build_model("enhanced_cnn_small", norm="group")
    one.load_state_dict(_INIT)
    ldnn.prepare(one, "cpu")
    opt = SGD(one.parameters(), lr=0.05, momentum=0.9)
    crit = CrossEntropyLoss()
    for x, y in zip(_XS, _YS):
        opt.zero_grad()
        crit(one(x), y).backward()
        opt.step()
    res = FakeWorld(2).run(_dp_train, shard)
    for r in range(2):
        kinds, sd, tail = res[r]
        if shard:   # GroupNorm affine are 1-D: they sit in the replicated tail bucket
            assert kinds[-1] is False and any(kinds), kinds
            assert "prep.1.weight" in tail and "layer3.bn2.bias" in tail
        for k, v in one.state_dict().items():
            torch.testing.assert_close(sd[k], v, rtol=1e-5, atol=1e-6, msg=k)


def test_checkpoint_round_trip(tmp_path):
    from ldnn.utils.checkpoint import Checkpointer, load_checkpoint

    torch.manual_seed(0)
    m = build_model("enhanced_cnn_small", norm="group")
    xavier_init(m)
    ldnn.prepare(m, "cpu")
    opt = SGD(m.parameters(), lr=0.05, momentum=0.9)
    x, y = torch.randn(4, 3, 32, 32), torch.randint(0, 10, (4,))
    opt.zero_grad()
    CrossEntropyLoss()(m(x), y).backward()
    opt.step()
    path = Checkpointer(str(tmp_path)).save(1, m, opt)
    m2 = build_model("enhanced_cnn_small", norm="group")
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
    with pytest.raises(Exception):   # a BatchNorm checkpoint is not silently accepted (no conversion)
        bn = build_model("enhanced_cnn_small")
        m2.load_state_dict(bn.state_dict())


def test_one_d_treatment_and_aggregation_without_buffers():
    """GroupNorm affine are 1-D like BatchNorm affine: the same names are excluded from LARS / LAMB
    trust ratios; clipping, weight decay and the EMA run; weight averaging with average_buffers on a
    model that has no buffer at all is the plain weight average."""
    from ldnn.parallel.aggregation import Aggregator

    bn, gn = build_model("enhanced_cnn_small"), build_model("enhanced_cnn_small", norm="group")
    assert [n for n, p in gn.named_parameters() if p.dim() < 2] == [n for n, p in bn.named_parameters() if p.dim() < 2]
    torch.manual_seed(0)
    x, y = torch.randn(4, 3, 32, 32), torch.randint(0, 10, (4,))
    for mk in (lambda p: SGD(p, lr=0.05, momentum=0.9, weight_decay=5e-4, max_grad_norm=1.0, lars_trust=0.02,
                             ema_decay=0.9),
               lambda p: Lamb(p, lr=1e-3, weight_decay=1e-2, max_grad_norm=1.0, ema_decay=0.9)):
        m = build_model("enhanced_cnn_small", norm="group")
        xavier_init(m)
        ldnn.prepare(m, "cpu")
        opt = mk(m.parameters())
        before = [p.detach().clone() for p in m.parameters()]
        for _ in range(2):
            opt.zero_grad()
            CrossEntropyLoss()(m(x), y).backward()
            opt.step()
        for (n, p), b in zip(m.named_parameters(), before):
            assert torch.isfinite(p).all() and not torch.equal(p, b), n

    models = []
    for s in range(2):
        torch.manual_seed(s)
        m = build_model("enhanced_cnn_small", norm="group")
        xavier_init(m)
        ldnn.prepare(m, "cpu")
        models.append(m)
    want = {k: (models[0].state_dict()[k] + models[1].state_dict()[k]) / 2 for k in models[0].state_dict()}

    def body(c):
        Aggregator("allreduce", "equal", "weights", comm=c, average_buffers=True)(models[c.rank])

    FakeWorld(2).run(body)
    for m in models:
        for k, v in m.state_dict().items():
            torch.testing.assert_close(v, want[k], rtol=1e-5, atol=1e-6, msg=k)
