"""Label smoothing of the cross-entropy criterion (torch's ``label_smoothing``, mean reduction):
the CPU path, the argument checks and the command line.  The kernel side is in
test_label_smoothing_gpu.py."""
import pytest
import torch
import torch.nn.functional as F

from ldnn.models import CrossEntropyLoss
from ldnn.ops import functional as LF


def _batch(B=37, C=10, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(B, C, generator=g) * 3, torch.randint(0, C, (B,), generator=g)


def test_criterion_matches_torch_cpu():
    x, y = _batch()
    B = x.shape[0]
    a = x.clone().requires_grad_(True)
    stats = torch.tensor([2.0, 3.0])
    loss = CrossEntropyLoss(label_smoothing=0.1)(a, y, stats)
    loss.backward()
    r = x.clone().requires_grad_(True)
    ref = F.cross_entropy(r, y, label_smoothing=0.1)
    ref.backward()
    plain = F.cross_entropy(x, y)
    torch.testing.assert_close(loss.detach(), ref.detach(), rtol=1e-6, atol=0)
    assert abs(loss.item() - plain.item()) > 1e-3   # (the option used to be dropped silently)
    torch.testing.assert_close(a.grad, r.grad, rtol=1e-6, atol=1e-9)
    correct = float((x.argmax(1) == y).sum())
    torch.testing.assert_close(stats, torch.tensor([2.0 + ref.item() * B, 3.0 + correct]), rtol=1e-6, atol=0)


def test_functional_matches_torch_cpu():
    x, y = _batch(seed=1)
    for eps in (0.1, 0.5, 1.0):
        torch.testing.assert_close(LF.cross_entropy(x, y, None, eps), F.cross_entropy(x, y, label_smoothing=eps),
                                   rtol=1e-6, atol=0)


def test_default_unchanged():
    x, y = _batch(seed=2)
    a, b = x.clone().requires_grad_(True), x.clone().requires_grad_(True)
    la, lb = LF.cross_entropy(a, y), LF.cross_entropy(b, y, label_smoothing=0.0)
    la.backward()
    lb.backward()
    assert torch.equal(la, lb) and torch.equal(a.grad, b.grad)
    assert torch.equal(CrossEntropyLoss()(x, y), la.detach())
    assert CrossEntropyLoss().label_smoothing == 0.0


@pytest.mark.parametrize("eps", [-0.1, 1.5])
def test_bad_smoothing_raises(eps):
    x, y = _batch()
    with pytest.raises(ValueError, match="label_smoothing"):
        LF.cross_entropy(x, y, label_smoothing=eps)
    with pytest.raises(ValueError, match="label_smoothing"):
        CrossEntropyLoss(label_smoothing=eps)(x, y)


@pytest.mark.parametrize("kw", [dict(weight=torch.ones(10)), dict(ignore_index=3), dict(reduction="sum"),
                                dict(reduction="none")], ids=["weight", "ignore_index", "sum", "none"])
def test_unimplemented_options_raise(kw):
    with pytest.raises(NotImplementedError):
        CrossEntropyLoss(**kw)


def test_cli_flag_and_engine(monkeypatch):
    from ldnn.cli import build_parser, resolve_engine
    from ldnn.models.mlp import mlp2

    p = build_parser()
    assert p.parse_args([]).label_smoothing == 0.0
    assert p.parse_args(["--label_smoothing", "0.1"]).label_smoothing == 0.1
    assert "smoothed" in p.format_help()   # (the validation loss is the smoothed one: the help says so)
    cpu = torch.device("cpu")
    # without a GPU every static request fails on the device first: the flag's own message needs
    # a native device, so stand one in
    import ldnn.cli as cli

    with monkeypatch.context() as mp:
        mp.setattr(cli, "native_gpu", lambda dev: True)
        a = p.parse_args(["--model", "mlp2", "--engine", "static", "--label_smoothing", "0.1"])
        with pytest.raises(SystemExit, match="--label_smoothing runs on the autograd path"):
            resolve_engine(a, mlp2(), cpu, 1)
        a = p.parse_args(["--model", "mlp2", "--engine", "auto", "--label_smoothing", "0.1"])
        assert resolve_engine(a, mlp2(), cpu, 1) is False
        # 0.0: as before
        a = p.parse_args(["--model", "mlp2", "--engine", "static", "--label_smoothing", "0.0"])
        assert resolve_engine(a, mlp2(), cpu, 1) is True
        a = p.parse_args(["--model", "mlp2", "--label_smoothing", "0.0"])
        assert resolve_engine(a, mlp2(), cpu, 1) is True
        # the earlier messages keep their precedence
        a = p.parse_args(["--model", "mlp2", "--engine", "static", "--optimizer", "lamb", "--label_smoothing", "0.1"])
        with pytest.raises(SystemExit, match="--optimizer lamb"):
            resolve_engine(a, mlp2(), cpu, 1)
    # on the CPU itself: auto falls back, static exits (as test_engine_adapter.test_resolve_engine_cpu)
    a = p.parse_args(["--model", "mlp2", "--label_smoothing", "0.1"])
    assert resolve_engine(a, mlp2(), cpu, 1) is False
    a = p.parse_args(["--model", "mlp2", "--engine", "static", "--label_smoothing", "0.1"])
    with pytest.raises(SystemExit):
        resolve_engine(a, mlp2(), cpu, 1)


def test_cli_rejects_out_of_range():
    from ldnn.cli import main

    with pytest.raises(SystemExit, match="label_smoothing"):
        main(["--label_smoothing", "1.5"])
