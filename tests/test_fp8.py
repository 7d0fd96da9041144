"""The fp8 Linear off the GPU: the torch twin of the recipe against exact math, and the public surface
(Linear(compute_dtype=), MLP / build_model(linear_dtype=), --linear_dtype)."""
import pytest
import torch
import torch.nn.functional as F

from ldnn.models import build_model
from ldnn.models.layers import Linear
from ldnn.models.mlp import mlp3
from ldnn.ops import functional as LF


def test_twin_against_exact_math():
    """Unit-variance operands at (B, K, N) = (32, 4096, 48): the recipe's relative Frobenius error against an fp64
    F.linear of the unquantised tensors measures 0.037 and depends only on the formats.  Above 0.08 the scale or the
    format is wrong; below 0.005 the twin did not quantise."""
    torch.manual_seed(0)
    B, K, N = 32, 4096, 48
    x = torch.randn(B, K, requires_grad=True)
    lin = Linear(K, N, activation="none", compute_dtype="fp8")
    with torch.no_grad():
        lin.weight.copy_(torch.randn(N, K))
        lin.bias.copy_(torch.randn(N))
    gy = torch.randn(B, N)
    y = lin(x)
    y.backward(gy)
    xd, wd = x.detach().double(), lin.weight.detach().double()
    exact = {"y": F.linear(xd, wd, lin.bias.detach().double()), "dx": gy.double() @ wd, "dw": gy.double().t() @ xd}
    got = {"y": y.detach(), "dx": x.grad, "dw": lin.weight.grad}
    for k, ref in exact.items():
        rel = ((got[k].double() - ref).norm() / ref.norm()).item()
        print(k, rel)
        assert 0.005 < rel < 0.08, (k, rel)
    assert torch.allclose(lin.bias.grad, gy.sum(0), rtol=1e-2, atol=1e-1)   # (from the bf16-rounded gz, unquantised)


@pytest.mark.parametrize("fmt", ["e4m3", "e5m2"])
def test_quantize_scale_is_the_largest_power_of_two(fmt):
    fmax = LF.FP8_FORMATS[fmt][1]
    t = torch.tensor([[fmax / 8, -1.0, 0.0, 0.5, 0.25, 0.0, 0.0, 0.0]]).bfloat16()   # the boundary e must include
    codes, codes_t, words = LF.fp8_quantize(t, fmt)
    assert words[:3].tolist() == [fmax / 8, 8.0, 0.125]
    assert codes.shape == (128, 128) and codes_t.shape == (128, 128) and torch.equal(codes.t(), codes_t)
    assert codes[0, 0].item() == (0x7E if fmt == "e4m3" else 0x7B) and codes[1:].sum() == 0   # fmt_max; pad code 0
    _, _, w0 = LF.fp8_quantize(torch.zeros(2, 8).bfloat16(), fmt)
    assert w0[:3].tolist() == [0.0, 1.0, 1.0]
    _, _, wn = LF.fp8_quantize(torch.tensor([[1.0, float("inf")] + [0.0] * 6]).bfloat16(), fmt)
    assert torch.isnan(wn[1:3]).all()


def test_defaults_keep_modules_and_keys():
    ref = build_model("mlp3_small")
    fp8 = build_model("mlp3_small", linear_dtype="fp8")
    assert [n for n, _ in fp8.named_modules()] == [n for n, _ in ref.named_modules()] == \
        ["", "layers", "layers.0", "layers.1", "layers.2"]
    assert list(fp8.state_dict()) == list(ref.state_dict())
    assert [l.compute_dtype for l in ref.layers] == ["bf16"] * 3
    assert [l.compute_dtype for l in fp8.layers] == ["fp8", "fp8", "bf16"]   # the output layer stays bf16
    assert [l.compute_dtype for l in build_model("mlp3_small", norm="layer", linear_dtype="fp8").layers][:2] == ["fp8"] * 2
    assert "compute_dtype" not in repr(ref) and "compute_dtype=fp8" in repr(fp8)


def test_refusals():
    with pytest.raises(ValueError, match="linear_dtype='fp8'"):
        build_model("lenet5", linear_dtype="fp8")
    with pytest.raises(ValueError):
        build_model("mlp3_small", linear_dtype="fp4")
    with pytest.raises(ValueError):
        Linear(8, 8, compute_dtype="fp16")
    from ldnn.cli import build_parser, main
    assert build_parser().parse_args([]).linear_dtype == "bf16"
    for model in ("lenet5", "enhanced_cnn_small"):
        with pytest.raises(SystemExit, match="--linear_dtype fp8"):
            main(["--linear_dtype", "fp8", "--model", model, "--device", "cpu"])
    with pytest.raises(SystemExit):
        main(["--engine", "static", "--linear_dtype", "fp8", "--model", "mlp3", "--device", "cpu"])
    from ldnn.train.static_mlp import StaticMLPEngine
    with pytest.raises(ValueError, match="autograd path"):
        StaticMLPEngine(mlp3(784, 64, 10, linear_dtype="fp8"), 8)
