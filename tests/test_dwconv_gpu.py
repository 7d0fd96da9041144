"""Depthwise 3x3 convolution (dwconv.hip) through layers.Conv2d(groups=C) against float64 on the MI355X."""
import pytest
import torch
import torch.nn.functional as F

import ldnn
from ldnn.models.layers import Conv2d

pytestmark = pytest.mark.gpu


def _ref(x, w, b, dy, stride, relu):
    """float64 F.conv2d(groups=C) on the bf16-rounded operands: (y, dx, dw, db), then the same convolution
    and gradients of the absolute values (the bounds' A)."""
    C = x.shape[1]
    pre = F.conv2d(x, w, b, stride, 1, 1, C)
    g = dy * (pre > 0) if relu else dy
    ay = F.conv2d(x.abs(), w.abs(), None if b is None else b.abs(), stride, 1, 1, C)
    grads = []
    for xx, ww, gg in ((x, w, g), (x.abs(), w.abs(), g.abs())):
        xx, ww = xx.clone().requires_grad_(True), ww.clone().requires_grad_(True)
        grads += [*torch.autograd.grad(F.conv2d(xx, ww, None, stride, 1, 1, C), (xx, ww), gg), gg.sum((0, 2, 3))]
    return [pre.relu() if relu else pre, *grads, ay]


# 1x1: all halo; odd sizes at stride 2; 72 channels: a second, partial channel block, 19 wide: several tiles both
# ways; 2x2 and 4x4: several images per tile; 12 channels: Cp = 16 > C
@pytest.mark.parametrize("N,C,H,W,stride,bias,act", [
    (1, 8, 1, 1, 1, False, "none"), (2, 8, 5, 7, 2, False, "none"), (3, 72, 19, 19, 1, False, "none"),
    (2, 72, 19, 17, 2, False, "none"), (5, 64, 2, 2, 1, False, "none"), (5, 64, 4, 4, 2, False, "none"),
    (2, 12, 6, 6, 1, False, "none"), (2, 12, 9, 6, 2, True, "relu")])
def test_depthwise_conv_matches_float64(N, C, H, W, stride, bias, act):
    """y, dx within 2^-8 |ref| + 2^-20 A (one bf16 rounding + a 9-term fp32 sum), dw (and db) within
    2^-24 L A_w with L = N P Q terms per tap; pad channels and the gradient storage beside the taps exactly 0;
    accumulation, the first write over a poisoned buffer after a lazy zero_grad, and run-to-run bit equality."""
    torch.manual_seed(0)
    conv = Conv2d(C, C, 3, stride, padding=1, groups=C, bias=bias, activation=act)
    flat = ldnn.prepare(conv, "cuda")
    x = torch.randn(N, C, H, W).bfloat16()
    xg = x.cuda().requires_grad_(True)
    hooked = []
    xg.register_hook(hooked.append)
    y = conv(xg)
    dy = torch.randn(y.shape).bfloat16()
    y.backward(dy.cuda())
    relu = act == "relu"
    ry, rdx, rdw, rdb, adx, adw, adb, ay = _ref(x.double(), conv.weight.detach().cpu().bfloat16().double(),
                                                conv.bias.detach().cpu().double() if bias else None, dy.double(),
                                                stride, relu)
    L = N * y.shape[2] * y.shape[3]
    gs = flat.grad_storage(conv.weight)
    dw1 = gs.clone()
    for name, got, ref, tol in (("y", y, ry, 2.0 ** -8 * ry.abs() + 2.0 ** -20 * ay),
                                ("dx", xg.grad, rdx, 2.0 ** -8 * rdx.abs() + 2.0 ** -20 * adx),
                                ("dw", dw1[:C, :, :, 0].unsqueeze(1), rdw, 2.0 ** -24 * L * adw)):
        err = (got.detach().double().cpu() - ref).abs()
        print(name, "max err", err.max().item(), "max bound", tol.max().item())
        assert (err <= tol).all(), (name, (err - tol).max().item())
    if bias:
        err = (conv.bias.grad.double().cpu() - rdb).abs()
        assert (err <= 2.0 ** -24 * L * adb).all(), ("db", err.max().item())
    Cp = gs.shape[0]
    for t in (y, hooked[0]):   # the whole NHWC buffers behind the logical views
        buf = torch.empty(0, dtype=t.dtype, device=t.device).set_(t.untyped_storage()).view(N, -1, Cp)
        assert getattr(t, "_ldnn_zpad", False) and (buf[..., C:] == 0).all()
    assert (gs[..., 1:] == 0).all() and (gs[C:] == 0).all()
    # a second backward accumulates: 2 dw (dw + dw is exact)
    conv(xg).backward(dy.cuda())
    err = (gs[:C, :, :, 0].unsqueeze(1).double().cpu() - 2 * rdw).abs()
    assert (err <= 2.0 ** -24 * L * 2 * adw).all() and (gs[..., 1:] == 0).all()
    # lazy zero_grad: the first write stores over whatever the buffer holds, pads included; same bits as run 1
    flat.zero_grad(lazy=True)
    gs.fill_(float("nan"))
    conv(xg).backward(dy.cuda())
    assert torch.equal(gs, dw1)


def test_other_grouped_convs_are_refused():
    conv = Conv2d(16, 16, 3, padding=1, groups=4, bias=False)
    ldnn.prepare(conv, "cuda")
    with pytest.raises(RuntimeError, match="depthwise"):
        conv(torch.randn(1, 16, 4, 4, device="cuda").bfloat16())
