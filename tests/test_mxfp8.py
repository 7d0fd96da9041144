"""The mxfp8 Linear off the GPU: the torch twin of the block-scaled recipe against exact math, and the public
surface (Linear(compute_dtype=), MLP / build_model(linear_dtype=), --linear_dtype)."""
import pytest
import torch

from ldnn.models import build_model
from ldnn.models.layers import Linear
from ldnn.models.mlp import mlp3
from ldnn.ops import functional as LF

# format -> (2^-(mantissa bits + 1), half a subnormal step of the scaled block = 2^(emin - mantissa bits - 1))
STEP = {"e4m3": (2.0 ** -4, 2.0 ** -10), "e5m2": (2.0 ** -3, 2.0 ** -17)}


def deq(t, fmt):
    """Quantise the rows of t in blocks of 32, decode: (fp64 values, 2^-e per element)."""
    codes, e = LF._mx8_codes(t, fmt)
    inv = torch.ldexp(torch.ones(e.shape, dtype=torch.float64), -e).repeat_interleave(32, dim=1)[:, :t.shape[1]]
    return codes.contiguous().view(LF.FP8_FORMATS[fmt][2]).double() * inv, inv


@pytest.mark.parametrize("fmt", ["e4m3", "e5m2"])
@pytest.mark.parametrize("R,C", [(3, 8), (64, 256), (5, 72)])
def test_twin_quantize_dequantize(R, C, fmt):
    """|deq - t| <= max(2^-4 |t|, 2^-10 2^-e) for e4m3 (three mantissa bits; half a subnormal step of the scaled
    block), 2^-3 and 2^-17 for e5m2; blocks scaled over 2^-8 .. 2^8, so neighbouring blocks differ in e."""
    torch.manual_seed(R + C)
    t = torch.randn(R, C) * torch.ldexp(torch.ones(R, C), torch.randint(-8, 9, (R, -(-C // 32))).repeat_interleave(32, 1)[:, :C])
    t = t.bfloat16()
    d, inv = deq(t, fmt)
    rel, sub = STEP[fmt]
    assert ((d - t.double()).abs() <= torch.maximum(rel * t.double().abs(), sub * inv)).all()
    codes, scales, codes_t, scales_t = LF.mx8_quantize(t, fmt)
    up = lambda v: (v + 127) // 128 * 128
    assert codes.shape == (up(R), up(C)) and scales.shape == (up(R), up(C) // 32)
    assert codes_t.shape == (up(C), up(R)) and scales_t.shape == (up(C), up(R) // 32)
    assert not codes[R:].any() and not codes[:, C:].any() and (scales[R:] == 127).all()
    assert len(scales[:R].unique()) > 1
    b8, bs, _, _ = LF.mx8_quantize(t, "e4m3", transpose=False)   # the fallback GEMM decodes the padded pairs
    out = LF.mx8_gemm(codes, scales, b8, bs, torch.empty(R, R), a_fmt=fmt)
    ref = d @ deq(t, "e4m3")[0].t()
    assert torch.allclose(out.double(), ref, rtol=1e-5, atol=1e-5 * ref.abs().max().item())


def test_outlier_stays_in_its_block():
    """One 1e4 in a [64, 256] randn matrix: the dequantised error outside that element's row-block is bit-identical
    to the error of the matrix without the outlier (a per-tensor scale would flush most of the matrix)."""
    torch.manual_seed(0)
    t = torch.randn(64, 256).bfloat16()
    u = t.clone()
    u[17, 100] = 1e4
    et, eu = deq(t, "e4m3")[0] - t.double(), deq(u, "e4m3")[0] - u.double()
    keep = torch.ones(64, 256, dtype=torch.bool)
    keep[17, 96:128] = False
    assert torch.equal(et[keep], eu[keep]) and et[keep].abs().max() > 0
    assert eu[17, 100].abs() <= 2.0 ** -4 * 1e4


def test_twin_linear_against_exact_math():
    """The twin's three products against fp64 F.linear of the unquantised tensors, with the bounds of test_fp8's
    per-tensor twin: the relative Frobenius error of unit-variance operands depends only on the formats.  Above 0.08
    a scale or a block orientation is wrong; below 0.005 the twin did not quantise."""
    torch.manual_seed(1)
    B, K, N = 40, 200, 48
    x = torch.randn(B, K, requires_grad=True)
    lin = Linear(K, N, activation="none", compute_dtype="mxfp8")
    with torch.no_grad():
        lin.weight.copy_(torch.randn(N, K))
    gy = torch.randn(B, N)
    y = lin(x)
    y.backward(gy)
    xd, wd = x.detach().double(), lin.weight.detach().double()
    gz = gy.double()
    exact = {"y": xd @ wd.t() + lin.bias.detach().double(), "dx": gz @ wd, "dw": gz.t() @ xd}
    for k, got in {"y": y.detach(), "dx": x.grad, "dw": lin.weight.grad}.items():
        rel = ((got.double() - exact[k]).norm() / exact[k].norm()).item()
        assert 0.005 < rel < 0.08, (k, rel)


def test_defaults_keep_modules_and_keys():
    ref = build_model("mlp3_small")
    mx = build_model("mlp3_small", linear_dtype="mxfp8")
    assert [n for n, _ in mx.named_modules()] == [n for n, _ in ref.named_modules()]
    assert list(mx.state_dict()) == list(ref.state_dict())
    assert [l.compute_dtype for l in ref.layers] == ["bf16"] * 3
    assert [l.compute_dtype for l in mx.layers] == ["mxfp8", "mxfp8", "bf16"]   # the output layer stays bf16
    assert [l.compute_dtype for l in build_model("mlp3_small", norm="layer", linear_dtype="mxfp8").layers][:2] == \
        ["mxfp8"] * 2
    assert "compute_dtype" not in repr(ref) and "compute_dtype=mxfp8" in repr(mx)
    assert "mxfp8" in LF.LINEAR_DTYPES


def test_refusals():
    with pytest.raises(ValueError, match="linear_dtype='mxfp8'"):
        build_model("lenet5", linear_dtype="mxfp8")
    with pytest.raises(ValueError):
        LF.linear_act(torch.zeros(2, 8), torch.zeros(8, 8), compute_dtype="mxfp4")
    from ldnn.cli import build_parser, main
    assert build_parser().parse_args([]).linear_dtype == "bf16"
    for model in ("lenet5", "enhanced_cnn_small"):
        with pytest.raises(SystemExit, match="--linear_dtype mxfp8"):
            main(["--linear_dtype", "mxfp8", "--model", model, "--device", "cpu"])
    with pytest.raises(SystemExit):
        main(["--engine", "static", "--linear_dtype", "mxfp8", "--model", "mlp3", "--device", "cpu"])
    from ldnn.train.static_mlp import StaticMLPEngine
    with pytest.raises(ValueError, match="linear_dtype='mxfp8'.*autograd path"):
        StaticMLPEngine(mlp3(784, 64, 10, linear_dtype="mxfp8"), 8)
