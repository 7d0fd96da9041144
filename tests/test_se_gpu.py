"""se.hip against float64 on the bf16-rounded inputs; the se_ratio CNNs against fp32 on the CPU and from a graph."""
import copy

import pytest
import torch
import torch.nn.functional as F

import ldnn
from ldnn.models import CrossEntropyLoss, SqueezeExcite, build_model, xavier_init
from ldnn.ops import functional as LF
from test_se import se_reference

pytestmark = pytest.mark.gpu

# (N, C, H, W): the smallest shapes that reach each code path
SHAPES = [
    (2, 8, 1, 1),         # one pixel, one vector per pixel, Ch clamped to 8
    (3, 128, 16, 16),     # EnhancedCNN's layer 1: 16 lanes per pixel, many sweeps
    (2, 1024, 2, 2),      # 128 lanes per pixel, fewer pixels than pixels in flight, Ch = 64
    (5, 72, 5, 3),        # C/8 = 9 does not divide 256, 15 pixels do not fill a sweep; Ch = 9, padded to 16
    (1, 2048, 3, 3),      # the channel-chunk loop
]
MODES = [(False, False), (True, False), (True, True)]   # (relu, residual)


def _cl(x):  # bf16 channels_last copy of a fp32 NCHW tensor
    return x.bfloat16().contiguous(memory_format=torch.channels_last)


def _module(C, seed=1):
    """W1, W2 scaled so that the gate spreads over roughly (0.1, 0.9) for _inputs' z (unit offsets)."""
    g = torch.Generator().manual_seed(seed)
    se = SqueezeExcite(C, 16 if C % 16 == 0 else 8)
    Ch = se.fc1.out_features
    with torch.no_grad():
        se.fc1.weight.copy_(torch.randn(Ch, C, generator=g) / C ** 0.5)
        se.fc1.bias.copy_(0.2 * torch.randn(Ch, generator=g))
        se.fc2.weight.copy_(torch.randn(C, Ch, generator=g) / Ch ** 0.5)
        se.fc2.bias.copy_(0.2 * torch.randn(C, generator=g))
    ldnn.prepare(se, "cuda")
    return se


def _inputs(shape, residual, seed=0):
    N, C, H, W = shape
    g = torch.Generator(device="cuda").manual_seed(seed)
    rnd = lambda *s: torch.randn(*s, device="cuda", generator=g)   # noqa: E731
    u = _cl(rnd(N, C, H, W) + rnd(1, C, 1, 1) + 0.5 * rnd(N, C, 1, 1))   # per-channel offsets: z is not ~ 0
    r = _cl(rnd(N, C, H, W)) if residual else None
    return u, r, _cl(rnd(N, C, H, W))


def _params(se):
    return se.fc1.weight, se.fc1.bias, se.fc2.weight, se.fc2.bias


def _native(u, r, t, se, relu):
    ub = u.clone().requires_grad_(True)
    rb = r.clone().requires_grad_(True) if r is not None else None
    y = se.act(ub, rb, relu)
    (y.float() * t.float()).sum().backward()
    return y.detach(), ub.grad, rb.grad if rb is not None else None


@pytest.mark.parametrize("relu,residual", MODES)
@pytest.mark.parametrize("shape", SHAPES)
def test_se_fused_vs_float64(shape, relu, residual):
    """Bounds: tests/test_group_norm_gpu.py's, with its ReLU boundary band narrowed: the fp32 gate is within 1e-5
    relative of float64's and |s * u| < 10, so only a pre-activation within 1e-4 of zero may sit on the other side of
    the ReLU; such elements (at most 1 % of a case) are left out of the du / dres comparison."""
    se = _module(shape[1])
    u, r, t = _inputs(shape, residual)
    ref = se_reference(u, r, t, _params(se), relu)
    assert ref["s"].std().item() > 0.1                      # (a wrong gate path must not hide behind s ~ 0.5)
    y, du, dres = _native(u, r, t, se, relu)
    assert se.__dict__.get("_ldnn_se_ws") is not None       # (the native path ran)
    assert y.dtype == torch.bfloat16 and y.shape == u.shape and LF._dense_nhwc(y) and du.shape == u.shape
    torch.testing.assert_close(y.double(), ref["out"], rtol=2e-2, atol=3e-2)
    keep = torch.ones_like(ref["pre"], dtype=torch.bool)
    if relu:
        keep = ref["pre"].abs() > 1e-4
        assert 1.0 - keep.float().mean().item() <= 0.01
    for name, got, want in (("du", du, ref["du"]), ("dres", dres, ref["dres"])):
        if want is None:
            assert got is None
            continue
        torch.testing.assert_close(torch.where(keep, got.double(), want), want, rtol=3e-2,
                                   atol=3e-2 * want.abs().max().item())
    for name, p in zip(("dw1", "db1", "dw2", "db2"), _params(se)):
        want = ref[name]
        torch.testing.assert_close(p.grad.double(), want, rtol=2e-2, atol=2e-2 * want.abs().max().item())


def test_second_backward_accumulates_and_lazy_zero_grad_overwrites_poison():
    shape = (5, 72, 5, 3)
    se = _module(shape[1])
    flat, Ch = se._ldnn_flat, se.fc1.out_features
    assert Ch == 9 and tuple(flat.grad_storage(se.fc1.weight).shape) == (16, 72)
    u, r, t = _inputs(shape, True)
    _native(u, r, t, se, True)
    once = [p.grad.clone() for p in _params(se)]
    _native(u, r, t, se, True)                 # no zero_grad: the totals are added
    for p, o in zip(_params(se), once):
        torch.testing.assert_close(p.grad, 2 * o, rtol=1e-6, atol=1e-6 * o.abs().max().item())
    flat.zero_grad(lazy=True)                  # marked zero only: the next backward overwrites
    flat.grad.fill_(float("nan"))
    _native(u, r, t, se, True)
    for p, o in zip(_params(se), once):
        assert torch.equal(p.grad, o)
    assert (flat.grad_storage(se.fc1.weight)[Ch:] == 0).all() and (flat.grad_storage(se.fc1.bias)[Ch:] == 0).all()
    assert (flat.grad_storage(se.fc2.weight)[:, Ch:] == 0).all()


def _cnn(n, **kw):
    """n identical enhanced_cnn_small(se_ratio=16) on the CPU: Xavier, bf16-representable weights, and biases
    0.5 * randn for the reason _inputs offsets u: with beta = 0 the squeeze averages a zero-mean map (|z| ~ 0.04), fc1's
    pre-activations straddle zero and rounding u alone to bf16 in fp32 moves fc1's gradients to a cosine of 0.985."""
    torch.manual_seed(0)
    ms = [build_model("enhanced_cnn_small", se_ratio=16, **kw)]
    xavier_init(ms[0])
    with torch.no_grad():   # (the conv kernels read a bf16 shadow: give both sides the same weights)
        for name, q in ms[0].named_parameters():
            if q.dim() > 1:
                q.copy_(q.bfloat16().float())
            elif name.endswith("bias"):
                q.copy_(0.5 * torch.randn(q.shape))
    return ms + [copy.deepcopy(ms[0]) for _ in range(n - 1)]


@pytest.mark.parametrize("separable", [False, True])
@pytest.mark.parametrize("norm", ["batch", "group"])
def test_se_model_vs_fp32_cpu(norm, separable):
    """Bounds: tests/test_group_norm_gpu.py's model-level ones (logits 5e-2 of max, every gradient's cosine > 0.98)."""
    m, ref = _cnn(2, norm=norm, separable=separable)
    ldnn.prepare(m, "cuda")
    g = torch.Generator().manual_seed(7)
    x, y = torch.randn(4, 3, 32, 32, generator=g).bfloat16(), torch.randint(0, 10, (4,), generator=g)
    out = m(x.cuda())
    CrossEntropyLoss()(out, y.cuda()).backward()
    ro = ref(x.float())
    F.cross_entropy(ro, y).backward()
    assert all(b.se.__dict__.get("_ldnn_se_ws") is not None for b in (m.layer1, m.layer2, m.layer3))
    torch.testing.assert_close(out.float().cpu(), ro.detach(), rtol=5e-2, atol=5e-2 * ro.abs().max().item())
    for (n, p), (_, q) in zip(m.named_parameters(), ref.named_parameters()):
        cos = F.cosine_similarity(p.grad.float().flatten().cpu(), q.grad.flatten(), dim=0).item()
        assert cos > 0.98, (n, cos)


def test_se_graphed_step_equals_eager():
    """Three replays against three eager steps, to tests/test_mxfp8_gpu.py's graphed-vs-eager tolerance."""
    from ldnn.optim import SGD
    from ldnn.train.graphed import GraphedStep

    ms = _cnn(3)
    for m in ms:
        ldnn.prepare(m, "cuda")
    os_ = [SGD(m.parameters(), lr=2e-3, momentum=0.9) for m in ms]
    crit = CrossEntropyLoss()
    gen = torch.Generator(device="cuda").manual_seed(1)
    xs = [torch.randn(8, 3, 32, 32, device="cuda", generator=gen).bfloat16() for _ in range(4)]
    ys = [torch.randint(0, 10, (8,), device="cuda", generator=gen) for _ in range(4)]

    def eager(m, o, i):
        o.zero_grad()
        crit(m(xs[i]), ys[i]).backward()
        o.step()

    for m, o in zip(ms, os_):
        eager(m, o, 0)
    p0 = [q.detach().clone() for q in ms[1].parameters()]
    gs = GraphedStep(ms[0], crit, os_[0], xs[1], ys[1], warmup=0)
    for i in (1, 2, 3):
        gs(xs[i], ys[i])
        eager(ms[1], os_[1], i)
        eager(ms[2], os_[2], i)
    torch.cuda.synchronize()
    for p, q, s, r in zip(*(m.parameters() for m in ms), p0):
        d1, d2, d3 = ((t.detach() - r).flatten().double() for t in (p, q, s))
        assert torch.isfinite(d1).all() and d2.norm() > 0
        assert (d1 - d2).norm().item() <= 3.0 * (d3 - d2).norm().item() + 2e-3 * d2.norm().item()
