"""Squeeze-and-Excitation on the CPU: the fp32 fallback against float64, structure, refusals, a two-step CLI run."""
import json
import math

import pytest
import torch

from ldnn.models import SqueezeExcite, build_model
from ldnn.ops import functional as LF


def se_reference(u, r, t, params, relu, dtype=torch.float64):
    """The issue's formula in ``dtype`` with autograd: (out, du, dres, dW1, db1, dW2, db2)."""
    u = u.detach().to(dtype).requires_grad_(True)
    r = r.detach().to(dtype).requires_grad_(True) if r is not None else None
    w1, b1, w2, b2 = (p.detach().to(dtype).requires_grad_(True) for p in params)
    h = torch.relu(u.mean((2, 3)) @ w1.T + b1)
    s = torch.sigmoid(h @ w2.T + b2)
    pre = u * s[:, :, None, None] + (r if r is not None else 0)
    out = torch.relu(pre) if relu else pre
    (out * t.to(dtype)).sum().backward()
    return dict(out=out.detach(), pre=pre.detach(), s=s.detach(), du=u.grad, dres=None if r is None else r.grad,
                dw1=w1.grad, db1=b1.grad, dw2=w2.grad, db2=b2.grad)


@pytest.mark.parametrize("relu,residual", [(False, False), (True, False), (True, True)])
def test_fallback_equals_float64(relu, residual):
    g = torch.Generator().manual_seed(0)
    N, C, H, W = 3, 24, 5, 3
    se = SqueezeExcite(C, 4)                                  # Ch = max(8, 6) = 8
    u = (torch.randn(N, C, H, W, generator=g) + torch.randn(1, C, 1, 1, generator=g)).requires_grad_(True)
    r = torch.randn(N, C, H, W, generator=g).requires_grad_(True) if residual else None
    t = torch.randn(N, C, H, W, generator=g)
    params = (se.fc1.weight, se.fc1.bias, se.fc2.weight, se.fc2.bias)
    ref = se_reference(u, r, t, params, relu)
    out = LF.se_scale_act(u, se, r, relu)
    (out * t).sum().backward()
    got = dict(out=out.detach(), du=u.grad, dres=None if r is None else r.grad, dw1=params[0].grad, db1=params[1].grad,
               dw2=params[2].grad, db2=params[3].grad)
    for k, v in got.items():   # fp32 against float64: a few ulp of sums of at most N * H * W * C terms
        if v is None:
            assert ref[k] is None
        else:
            torch.testing.assert_close(v.double(), ref[k], rtol=1e-4, atol=1e-5 * max(1.0, ref[k].abs().max().item()))


@pytest.mark.parametrize("name,blocks", [("enhanced_cnn", [f"layer{i}.{j}" for i in (1, 2, 3, 4) for j in (0, 1)]),
                                         ("enhanced_cnn_small", ["layer1", "layer2", "layer3"])])
def test_structure(name, blocks):
    base, off, se = build_model(name), build_model(name, se_ratio=0), build_model(name, se_ratio=16)
    assert list(base.state_dict()) == list(off.state_dict())
    assert [n for n, _ in base.named_modules()] == [n for n, _ in off.named_modules()]
    extra = [k for k in se.state_dict() if k not in base.state_dict()]
    assert extra == [f"{b}.se.{fc}.{p}" for b in blocks for fc in ("fc1", "fc2") for p in ("weight", "bias")]
    assert [k for k in se.state_dict() if k not in extra] == list(base.state_dict())
    if name == "enhanced_cnn":
        n = sum(p.numel() for p in se.parameters())
        assert n == 44_595_786 + 352_240 == 44_948_026


def test_refusals():
    for name in ("resnet18", "mlp3"):
        with pytest.raises(ValueError, match="se_ratio"):
            build_model(name, se_ratio=16)
    with pytest.raises(ValueError, match="se_ratio"):
        SqueezeExcite(72, 16)
    with pytest.raises(ValueError, match="se_ratio"):
        build_model("enhanced_cnn_small", se_ratio=48)
    from ldnn.cli import main
    with pytest.raises(SystemExit, match="--se_ratio"):
        main(["--se_ratio", "16", "--model", "lenet5", "--device", "cpu"])
    with pytest.raises(SystemExit, match="--se_ratio"):
        main(["--se_ratio", "-1", "--model", "enhanced_cnn_small", "--device", "cpu"])


def test_cli_two_step_cpu_run(tmp_path):
    from ldnn.cli import main

    main(["--model", "enhanced_cnn_small", "--se_ratio", "16", "--separable", "--norm", "group", "--n_train", "16",
          "--n_test", "8", "--batch_size", "8", "--epochs_global", "1", "--epochs_local", "1", "--device", "cpu", "--quiet",
          "--out_dir", str(tmp_path), "--plots", "", "--no_eval", "--no_repartition"])
    ep = [r for r in map(json.loads, open(tmp_path / "metrics.rank0.jsonl")) if r.get("kind") == "global_epoch"][0]
    assert 8 < ep["samples"] <= 16 and math.isfinite(ep["train_loss"])   # (two batches of the training split)
