"""The separable EnhancedCNNs with a grouped 3x3 (group_width): structure, counts, refusals and a CPU step."""
import pytest
import torch

from ldnn.models import CrossEntropyLoss, build_model


@pytest.mark.parametrize("name,base,sum_c,first", [("enhanced_cnn", 5_662_346, 6720, "layer1.0"),
                                                   ("enhanced_cnn_small", 712_586, 1344, "layer1")])
@pytest.mark.parametrize("gw", [8, 16, 32])
def test_grouped_separable_structure(name, base, sum_c, first, gw):
    m = build_model(name, separable=True, group_width=gw)
    assert sum(p.numel() for p in m.parameters()) == base + 9 * (gw - 1) * sum_c
    sd = m.state_dict()
    assert list(sd) == list(build_model(name, separable=True, group_width=1).state_dict())
    assert tuple(sd[f"{first}.conv1.dw.weight"].shape) == (64, gw, 3, 3)
    assert tuple(sd[f"{first}.conv2.dw.weight"].shape) == (128, gw, 3, 3)
    assert tuple(sd[f"{first}.conv1.pw.weight"].shape) == (128, 64, 1, 1)


def test_group_width_refusals():
    for kw in (dict(name="enhanced_cnn", separable=True, group_width=4), dict(name="enhanced_cnn", group_width=16),
               dict(name="resnet18", separable=True, group_width=16)):
        with pytest.raises(ValueError, match="group_width"):
            build_model(**kw)
    from ldnn.cli import build_parser, main
    assert build_parser().parse_args([]).group_width == 1
    with pytest.raises(SystemExit, match=r"--group_width.*--separable"):
        main(["--group_width", "16", "--model", "enhanced_cnn_small", "--device", "cpu"])


def test_grouped_separable_cpu_step_is_finite():
    torch.manual_seed(0)
    m = build_model("enhanced_cnn_small", separable=True, group_width=16)
    loss = CrossEntropyLoss()(m(torch.randn(4, 3, 32, 32)), torch.randint(0, 10, (4,)))
    loss.backward()
    assert torch.isfinite(loss) and all(torch.isfinite(p.grad).all() for p in m.parameters())
