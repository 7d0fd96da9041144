"""The depthwise-separable EnhancedCNN variant: structure, keys, refusals and a CPU step."""
import pytest
import torch

from ldnn.models import CrossEntropyLoss, build_model


def _dense_keys(stages):
    """The dense model's state_dict keys: prep, the blocks of ``stages`` (prefix list), fc."""
    norm = ["weight", "bias", "running_mean", "running_var", "num_batches_tracked"]
    keys = ["prep.0.weight"] + [f"prep.1.{k}" for k in norm]
    for blk, shortcut in stages:
        keys += [f"{blk}.conv1.weight"] + [f"{blk}.bn1.{k}" for k in norm]
        keys += [f"{blk}.conv2.weight"] + [f"{blk}.bn2.{k}" for k in norm]
        if shortcut:
            keys += [f"{blk}.shortcut.0.weight"] + [f"{blk}.shortcut.1.{k}" for k in norm]
    return keys + ["fc.weight", "fc.bias"]


@pytest.mark.parametrize("name,count,stages", [
    ("enhanced_cnn", 5_662_346, [(f"layer{i}.{j}", j == 0) for i in (1, 2, 3, 4) for j in (0, 1)]),
    ("enhanced_cnn_small", 712_586, [(f"layer{i}", True) for i in (1, 2, 3)])])
def test_separable_structure(name, count, stages):
    m = build_model(name, separable=True)
    assert sum(p.numel() for p in m.parameters()) == count
    assert list(build_model(name).state_dict()) == list(build_model(name, separable=False).state_dict()) \
        == _dense_keys(stages)
    sd, first = m.state_dict(), stages[0][0]
    assert tuple(sd[f"{first}.conv1.dw.weight"].shape) == (64, 1, 3, 3)
    assert tuple(sd[f"{first}.conv1.pw.weight"].shape) == (128, 64, 1, 1)
    assert f"{first}.conv1.weight" not in sd and tuple(sd["prep.0.weight"].shape) == (64, 3, 3, 3)


def test_separable_refusals():
    for name in ("resnet18", "mlp3"):
        with pytest.raises(ValueError, match="separable"):
            build_model(name, separable=True)
    from ldnn.cli import build_parser, main
    assert build_parser().parse_args([]).separable is False
    with pytest.raises(SystemExit, match="--separable"):
        main(["--separable", "--model", "lenet5", "--device", "cpu"])


@pytest.mark.parametrize("norm", ["batch", "group"])
def test_separable_cpu_step_is_finite(norm):
    torch.manual_seed(0)
    m = build_model("enhanced_cnn_small", norm=norm, separable=True)
    loss = CrossEntropyLoss()(m(torch.randn(4, 3, 32, 32)), torch.randint(0, 10, (4,)))
    loss.backward()
    assert torch.isfinite(loss) and all(torch.isfinite(p.grad).all() for p in m.parameters())
