"""Grouped 3x3 convolution (gconv.hip) through layers.Conv2d(groups=C // gw) against float64 on the MI355X."""
import pytest
import torch
import torch.nn.functional as F

import ldnn
from ldnn.models.layers import Conv2d

pytestmark = pytest.mark.gpu


def _ref(x, w, b, dy, stride, relu, G):
    """float64 F.conv2d(groups=G) on the bf16-rounded operands: (y, dx, dw, db), then the same convolution
    and gradients of the absolute values (the bounds' A)."""
    pre = F.conv2d(x, w, b, stride, 1, 1, G)
    g = dy * (pre > 0) if relu else dy
    ay = F.conv2d(x.abs(), w.abs(), None if b is None else b.abs(), stride, 1, 1, G)
    grads = []
    for xx, ww, gg in ((x, w, g), (x.abs(), w.abs(), g.abs())):
        xx, ww = xx.clone().requires_grad_(True), ww.clone().requires_grad_(True)
        grads += [*torch.autograd.grad(F.conv2d(xx, ww, None, stride, 1, 1, G), (xx, ww), gg), gg.sum((0, 2, 3))]
    return [pre.relu() if relu else pre, *grads, ay]


# 1x1: all halo, one group in a mostly empty slab; odd sizes at stride 2 with two taps (half-zero fifth MFMA) and one
# tap per MFMA; 96 / 80 channels: a second, partial slab, 19 wide: several tiles both ways; 2x2 and 4x4: several
# images per tile, four taps' worth of width 8; bias + ReLU and the colsum launches
@pytest.mark.parametrize("N,C,gw,H,W,stride,bias,act", [
    (1, 8, 8, 1, 1, 1, False, "none"), (2, 16, 16, 5, 7, 2, False, "none"), (2, 32, 32, 5, 7, 2, False, "none"),
    (3, 96, 32, 19, 19, 1, False, "none"), (2, 80, 16, 19, 17, 2, False, "none"), (5, 64, 8, 2, 2, 1, False, "none"),
    (5, 64, 8, 4, 4, 2, False, "none"), (2, 48, 16, 9, 6, 2, True, "relu")])
def test_grouped_conv_matches_float64(N, C, gw, H, W, stride, bias, act):
    """y, dx within 2^-8 |ref| + 2^-23 T A (one bf16 rounding + a T = 9 gw term fp32 sum), dw (and db) within
    2^-23 L A_w with L = N P Q terms; accumulation, the first write over a poisoned buffer after a lazy
    zero_grad, and run-to-run bit equality."""
    torch.manual_seed(0)
    conv = Conv2d(C, C, 3, stride, padding=1, groups=C // gw, bias=bias, activation=act)
    flat = ldnn.prepare(conv, "cuda")
    x = torch.randn(N, C, H, W).bfloat16()
    xg = x.cuda().requires_grad_(True)
    y = conv(xg)
    dy = torch.randn(y.shape).bfloat16()
    y.backward(dy.cuda())
    ry, rdx, rdw, rdb, adx, adw, adb, ay = _ref(x.double(), conv.weight.detach().cpu().bfloat16().double(),
                                                conv.bias.detach().cpu().double() if bias else None, dy.double(),
                                                stride, act == "relu", C // gw)
    L, T = N * y.shape[2] * y.shape[3], 9 * gw
    gs = flat.grad_storage(conv.weight)   # [C][3][3][gw]
    assert tuple(gs.shape) == (C, 3, 3, gw)
    dw1 = gs.clone()
    for name, got, ref, tol in (("y", y, ry, 2.0 ** -8 * ry.abs() + 2.0 ** -23 * T * ay),
                                ("dx", xg.grad, rdx, 2.0 ** -8 * rdx.abs() + 2.0 ** -23 * T * adx),
                                ("dw", dw1.permute(0, 3, 1, 2), rdw, 2.0 ** -23 * L * adw)):
        err = (got.detach().double().cpu() - ref).abs()
        print(name, "max err", err.max().item(), "max bound", tol.max().item())
        assert (err <= tol).all(), (name, (err - tol).max().item())
    if bias:
        err = (conv.bias.grad.double().cpu() - rdb).abs()
        print("db max err", err.max().item(), "max bound", (2.0 ** -23 * L * adb).max().item())
        assert (err <= 2.0 ** -23 * L * adb).all(), ("db", err.max().item())
    # a second backward accumulates: 2 dw (dw + dw is exact)
    conv(xg).backward(dy.cuda())
    err = (gs.permute(0, 3, 1, 2).double().cpu() - 2 * rdw).abs()
    assert (err <= 2.0 ** -23 * L * 2 * adw).all()
    # lazy zero_grad: the first write stores over whatever the buffer holds; same bits as run 1
    flat.zero_grad(lazy=True)
    gs.fill_(float("nan"))
    conv(xg).backward(dy.cuda())
    assert torch.equal(gs, dw1)
