"""Native NHWC bf16 GroupNorm (+ residual + ReLU), forward and backward (group_norm.hip), against
F.group_norm in fp32 on the same bf16-rounded inputs; and the GroupNorm CNNs against fp32 torch.nn
twins, eagerly and from a captured step."""
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import ldnn
from ldnn.models import CrossEntropyLoss, build_model, xavier_init
from ldnn.models.layers import GroupNorm
from ldnn.ops import _ext
from ldnn.ops import functional as LF

pytestmark = pytest.mark.gpu

# (N, C, H, W, G): the smallest shapes that reach each way the kernels can go wrong
SHAPES = [
    (2, 64, 4, 4, 32),      # cg = 2, four groups inside one 8-channel vector
    (3, 128, 5, 7, 32),     # cg = 4, odd pixel count, odd N
    (2, 256, 2, 2, 32),     # cg = 8, one vector is one group
    (1, 512, 1, 1, 32),     # one pixel, m = 16: more slabs than pixels must not happen
    (2, 1024, 2, 2, 32),    # cg = 32, a group spans four vectors; EnhancedCNN's last stage
    (2, 64, 3, 3, 1),       # one group: layer norm over C, H, W
    (2, 64, 3, 3, 64),      # cg = 1: instance norm
    (5, 24, 3, 3, 3),       # G not a power of two
    (2, 64, 32, 32, 32),    # several pixel slabs per sample; EnhancedCNN's first layer
]
MODES = [(False, False), (True, False), (True, True)]   # (relu, residual)


def _cl(x):  # bf16 channels_last copy of a fp32 NCHW tensor
    return x.bfloat16().contiguous(memory_format=torch.channels_last)


def _module(C, G, seed, affine=True):
    g = torch.Generator().manual_seed(seed)
    gn = GroupNorm(G, C, affine=affine)
    if affine:
        with torch.no_grad():
            gn.weight.copy_(1 + 0.3 * torch.randn(C, generator=g))
            gn.bias.copy_(0.2 * torch.randn(C, generator=g))
    ldnn.prepare(gn, "cuda")
    return gn


def _inputs(shape, residual, seed=0):
    N, C, H, W, _ = shape
    g = torch.Generator(device="cuda").manual_seed(seed)
    x = _cl(1.5 * torch.randn(N, C, H, W, device="cuda", generator=g) + 0.5)
    r = _cl(torch.randn(N, C, H, W, device="cuda", generator=g)) if residual else None
    dy = _cl(torch.randn(N, C, H, W, device="cuda", generator=g))
    return x, r, dy


def _reference(x, r, dy, gn, G, relu):
    """F.group_norm in fp32 on the bf16-rounded inputs, the fp32 add and ReLU, autograd backward."""
    xf = x.float().requires_grad_(True)
    rf = r.float().requires_grad_(True) if r is not None else None
    w = gn.weight.detach().clone().requires_grad_(True) if gn.affine else None
    b = gn.bias.detach().clone().requires_grad_(True) if gn.affine else None
    pre = F.group_norm(xf, G, w, b, gn.eps)
    if rf is not None:
        pre = pre + rf
    y = F.relu(pre) if relu else pre
    y.backward(dy.float())
    return dict(y=y.detach(), pre=pre.detach(), dx=xf.grad, dres=rf.grad if rf is not None else None,
                dgamma=w.grad if w is not None else None, dbeta=b.grad if b is not None else None)


def _native(x, r, dy, gn, relu):
    xb = x.clone().requires_grad_(True)
    rb = r.clone().requires_grad_(True) if r is not None else None
    y = gn.act(xb, rb, relu)
    y.backward(dy)
    return y.detach(), xb.grad, rb.grad if rb is not None else None


def _check(shape, relu, residual, affine=True):
    N, C, H, W, G = shape
    gn = _module(C, G, seed=1, affine=affine)
    x, r, dy = _inputs(shape, residual)
    ref = _reference(x, r, dy, gn, G, relu)
    y, dx, dres = _native(x, r, dy, gn, relu)
    assert y.dtype == torch.bfloat16 and y.shape == x.shape and LF._dense_nhwc(y) and dx.shape == x.shape
    torch.testing.assert_close(y.float(), ref["y"], rtol=2e-2, atol=3e-2)
    keep = torch.ones_like(ref["pre"], dtype=torch.bool)
    if relu:
        # an element whose reference pre-activation is within 1e-3 of zero may sit on the other side
        # of the ReLU after bf16 rounding: left out of the dx / dres comparison, at most 1 % of a case
        keep = ref["pre"].abs() > 1e-3
        share = 1.0 - keep.float().mean().item()
        print(f"{shape} relu boundary share {share:.4%}")
        assert share <= 0.01, share
    for name, got, want in (("dx", dx, ref["dx"]), ("dres", dres, ref["dres"])):
        if want is None:
            assert got is None
            continue
        err = ((got.float() - want).abs() * keep).max().item()
        print(f"{shape} relu={relu} res={residual} {name}: max err {err:.3e} of max|ref| {want.abs().max().item():.3e}")
        torch.testing.assert_close(torch.where(keep, got.float(), want), want, rtol=3e-2,
                                   atol=3e-2 * want.abs().max().item())
    if affine:
        for name, got, want in (("dgamma", gn.weight.grad, ref["dgamma"]), ("dbeta", gn.bias.grad, ref["dbeta"])):
            print(f"{shape} {name}: max err {(got - want).abs().max().item():.3e} of {want.abs().max().item():.3e}")
            torch.testing.assert_close(got, want, rtol=2e-2, atol=2e-2 * want.abs().max().item())
    return gn


@pytest.mark.parametrize("relu,residual", MODES)
@pytest.mark.parametrize("shape", SHAPES)
def test_group_norm_fused_vs_fp32(shape, relu, residual):
    _check(shape, relu, residual)


def test_slabs_never_exceed_pixels():
    C_ = _ext.C()
    for N, C, H, W, G in SHAPES + [(64, 64, 32, 32, 32), (64, 1024, 2, 2, 32), (64, 64, 56, 56, 32), (256, 64, 112, 112, 32)]:
        s = C_.gn_slabs(N, H * W, C, G)
        assert 1 <= s <= H * W, (N, C, H, W, s)
    assert C_.gn_slabs(1, 1, 512, 32) == 1
    assert C_.gn_slabs(2, 1024, 64, 32) > 1                    # several slabs per sample on the first layer
    assert 64 * C_.gn_slabs(64, 1024, 64, 32) >= 4 * 256       # and enough workgroups for 256 CUs at batch 64


def test_one_pixel_map_is_kept_finite_by_eps():
    """m = cg on a 1x1 map; a constant group has variance 0 and rstd = 1 / sqrt(eps)."""
    gn = _module(64, 32, seed=2)
    x = torch.zeros(2, 64, 1, 1, device="cuda")
    x[:, 0::2] = 3.0
    x[:, 1::2] = 3.0          # every group of two channels is constant
    xb = _cl(x).requires_grad_(True)
    y = gn.act(xb, relu=False)
    # (x - mean) * rstd = 0 * 316: the output is beta, to the forward's tolerance
    torch.testing.assert_close(y.float().flatten(1), gn.bias.detach().expand(2, 64), rtol=2e-2, atol=3e-2)
    y.backward(_cl(torch.ones_like(x)))
    assert torch.isfinite(xb.grad.float()).all() and torch.isfinite(gn.weight.grad).all()
    torch.testing.assert_close(gn.weight.grad, torch.zeros(64, device="cuda"), rtol=0, atol=0)   # xhat = 0


@pytest.mark.parametrize("shape", [(2, 64, 32, 32, 32), (2, 1024, 2, 2, 32)])
def test_two_runs_are_bit_equal(shape):
    out = []
    for _ in range(2):
        gn = _module(shape[1], shape[4], seed=1)
        x, r, dy = _inputs(shape, True)
        y, dx, dres = _native(x, r, dy, gn, True)
        out.append((y, dx, dres, gn.weight.grad.clone(), gn.bias.grad.clone()))
    for a, b in zip(*out):
        assert torch.equal(a, b)


def test_second_backward_accumulates_and_lazy_zero_grad_overwrites():
    shape = (3, 128, 5, 7, 32)
    gn = _module(shape[1], shape[4], seed=1)
    flat = gn._ldnn_flat
    x, r, dy = _inputs(shape, False)
    ref = _reference(x, None, dy, gn, shape[4], True)
    _native(x, None, dy, gn, True)
    once_g, once_b = gn.weight.grad.clone(), gn.bias.grad.clone()
    _native(x, None, dy, gn, True)            # no zero_grad: grad_assign = False, the totals are added
    torch.testing.assert_close(gn.weight.grad, 2 * once_g, rtol=1e-6, atol=1e-6 * once_g.abs().max().item())
    torch.testing.assert_close(gn.bias.grad, 2 * once_b, rtol=1e-6, atol=1e-6 * once_b.abs().max().item())
    flat.zero_grad(lazy=True)                  # marked zero only: the next backward overwrites
    _native(x, None, dy, gn, True)
    assert torch.equal(gn.weight.grad, once_g) and torch.equal(gn.bias.grad, once_b)
    torch.testing.assert_close(once_g, ref["dgamma"], rtol=2e-2, atol=2e-2 * ref["dgamma"].abs().max().item())


def test_mixed_first_write_clears_only_the_fresh_gradient():
    """The weight's gradient already written this step, the bias's still marked zero by the lazy
    zero_grad: the backward adds dgamma onto the written one and clears the stale bias buffer before
    adding dbeta (0 + total: the same bits as the store).  The totals come from one clean backward
    of an identically seeded twin."""
    shape = (3, 128, 5, 7, 32)
    gn, twin = _module(shape[1], shape[4], seed=1), _module(shape[1], shape[4], seed=1)
    flat = gn._ldnn_flat
    x, r, dy = _inputs(shape, False)
    _native(x, None, dy, twin, True)
    dgamma, dbeta = twin.weight.grad.clone(), twin.bias.grad.clone()
    _native(3 * x, None, dy, gn, True)        # native ops write both; their buffers now hold other totals
    flat.zero_grad(lazy=True)
    gn.weight.grad.fill_(1.0)
    assert flat.grad_beta(gn.weight) == 0.0   # a caller wrote the weight's gradient: no longer fresh
    _native(x, None, dy, gn, True)
    torch.testing.assert_close(gn.weight.grad, 1 + dgamma, rtol=1e-6, atol=1e-6 * dgamma.abs().max().item())
    assert torch.equal(gn.bias.grad, dbeta)


def test_affine_false():
    gn = _check((3, 128, 5, 7, 32), True, True, affine=False)
    assert list(gn.parameters()) == []


def test_other_channel_counts_take_the_fallback():
    shape = (2, 20, 3, 3, 5)
    gn = _module(20, 5, seed=1)
    x, r, dy = _inputs(shape, True)
    ref = _reference(x, r, dy, gn, 5, True)
    y, dx, dres = _native(x, r, dy, gn, True)
    torch.testing.assert_close(y.float(), ref["y"], rtol=2e-2, atol=3e-2)
    torch.testing.assert_close(dx.float(), ref["dx"], rtol=3e-2, atol=3e-2 * ref["dx"].abs().max().item())
    torch.testing.assert_close(gn.weight.grad, ref["dgamma"], rtol=2e-2, atol=2e-2 * ref["dgamma"].abs().max().item())
    assert getattr(gn, "_ldnn_gn_ws", None) is None      # (no native call happened)


def test_binding_refuses_bad_arguments():
    C_ = _ext.C()
    N, H, W, C, G = 2, 3, 3, 64, 32
    x = torch.randn(N, H, W, C, device="cuda").bfloat16()
    y = torch.empty_like(x)
    mean, rstd = torch.empty(N * G, device="cuda"), torch.empty(N * G, device="cuda")
    ws = torch.empty(C_.gn_workspace_floats(N, H * W, C, G), device="cuda")
    C_.gn_fwd(x, y, None, None, None, mean, rstd, ws, G, 1e-5, False)
    x8 = torch.zeros(x.numel() + 8, dtype=torch.bfloat16, device="cuda")[4:4 + x.numel()].view(N, H, W, C)
    assert x8.data_ptr() % 16 == 8
    for bad in (lambda: C_.gn_fwd(x, y, None, None, None, mean, rstd, ws, 48, 1e-5, False),        # C % G
                lambda: C_.gn_fwd(x[..., :20].contiguous(), y[..., :20].contiguous(), None, None, None, mean, rstd, ws,
                                  5, 1e-5, False),                                                 # C % 8
                lambda: C_.gn_fwd(x, y[:1], None, None, None, mean, rstd, ws, G, 1e-5, False),     # shape
                lambda: C_.gn_fwd(x, y, None, None, None, mean[:8], rstd, ws, G, 1e-5, False),     # short mean
                lambda: C_.gn_fwd(x, y, None, None, None, mean, rstd, ws[:16], G, 1e-5, False),    # short ws
                lambda: C_.gn_fwd(x8, y, None, None, None, mean, rstd, ws, G, 1e-5, False),       # 8-B aligned x
                lambda: C_.gn_fwd(x, y, None, None, None, mean.cpu(), rstd, ws, G, 1e-5, False),   # device
                lambda: C_.gn_fwd(x, y, None, None, None, mean, rstd, ws, G, 1e-5, False,
                                  mask=torch.empty(x.numel() // 8, dtype=torch.uint8, device="cuda")),   # mask, no relu
                lambda: C_.gn_bwd(x, x.clone(), y, None, None, mean, rstd, ws, None, None, G, True)):   # relu, no mask
        with pytest.raises(RuntimeError):
            bad()
    torch.cuda.synchronize()


def test_padding_is_not_read_and_nothing_outside_is_written():
    """y, dx, dres and the mask between canaries, the bytes behind x, the residual and dy NaN: nothing
    outside an output is written, no poison reaches a result, and the results are those of plain buffers."""
    from strided import assert_no_poison, assert_outside_untouched, poisoned, write_inside

    C_ = _ext.C()
    shape = (3, 128, 5, 7, 32)
    N, C, H, W, G = shape
    rows = N * H * W
    gn = _module(C, G, seed=1)
    flat = gn._ldnn_flat
    gamma, beta = flat.master_storage(gn.weight)[:C], flat.master_storage(gn.bias)[:C]
    xs, rs, dys = (t.permute(0, 2, 3, 1).reshape(rows, C) for t in _inputs(shape, True))

    def run(make_in, make_out):
        x, r, dy = make_in(xs), make_in(rs), make_in(dys)
        y, dx, dres = make_out(torch.bfloat16, C), make_out(torch.bfloat16, C), make_out(torch.bfloat16, C)
        mask = make_out(torch.uint8, C // 8)
        mean, rstd = torch.empty(N * G, device="cuda"), torch.empty(N * G, device="cuda")
        ws = torch.empty(C_.gn_workspace_floats(N, H * W, C, G), device="cuda")
        dg, db = torch.empty(C, device="cuda"), torch.empty(C, device="cuda")
        v = lambda t: t[0].view(N, H, W, C)
        C_.gn_fwd(v(x), v(y), v(r), gamma, beta, mean, rstd, ws, G, gn.eps, True, mask=mask[0].view(-1))
        C_.gn_bwd(v(x), v(dy), v(dx), v(dres), gamma, mean, rstd, ws, dg, db, G, True, mask=mask[0].view(-1),
                  grad_assign=True)
        torch.cuda.synchronize()
        return (y, dx, dres, mask), (dg, db)

    def dense_in(t):
        return (t.clone(), None)

    def dense_out(dtype, cols):
        return (torch.zeros(rows, cols, dtype=dtype, device="cuda"), None)

    def poisoned_in(t):
        v, h = poisoned(rows, C, ld=C, before=3, after=5, dtype=torch.bfloat16, device="cuda", fill="nan", full_rows=True)
        write_inside(v, t)
        return v, h

    def poisoned_out(dtype, cols):
        return poisoned(rows, cols, ld=cols, before=3, after=5, dtype=dtype, device="cuda", fill="sentinel",
                        aligned=dtype != torch.uint8, full_rows=True)

    outs_d, grads_d = run(dense_in, dense_out)
    outs_p, grads_p = run(poisoned_in, poisoned_out)
    for name, (vd, _), (vp, hp) in zip(("y", "dx", "dres", "mask"), outs_d, outs_p):
        assert_outside_untouched(hp, name)
        if vp.dtype.is_floating_point:
            assert_no_poison(vp, name)
        assert torch.equal(vp, vd), name
    for a, b in zip(grads_d, grads_p):
        assert torch.isfinite(a).all() and torch.equal(a, b)


# ---- model level ---------------------------------------------------------------------------

class _RefBlock(nn.Module):
    def __init__(self, cin, cout, stride, short):
        super().__init__()
        self.conv1 = nn.Conv2d(cin, cout, 3, stride, 1, bias=False)
        self.bn1 = nn.GroupNorm(32, cout)
        self.conv2 = nn.Conv2d(cout, cout, 3, 1, 1, bias=False)
        self.bn2 = nn.GroupNorm(32, cout)
        sc = nn.Sequential()
        if stride != 1 or cin != cout:
            sc = nn.Sequential(nn.Conv2d(cin, cout, 1, stride, bias=False), nn.GroupNorm(32, cout))
        setattr(self, short, sc)
        self.short = short

    def forward(self, x):
        out = F.relu(self.bn1(self.conv1(x)))
        return F.relu(self.bn2(self.conv2(out)) + getattr(self, self.short)(x))


class _RefSmall(nn.Module):
    """Plain torch.nn twin of EnhancedCNNSmall(norm="group"): same state_dict keys, no ldnn layer."""

    def __init__(self):
        super().__init__()
        self.prep = nn.Sequential(nn.Conv2d(3, 64, 3, 1, 1, bias=False), nn.GroupNorm(32, 64), nn.ReLU())
        self.layer1, self.layer2 = _RefBlock(64, 128, 2, "shortcut"), _RefBlock(128, 256, 2, "shortcut")
        self.layer3 = _RefBlock(256, 512, 2, "shortcut")
        self.fc = nn.Linear(512, 10)

    def forward(self, x):
        return self.fc(self.layer3(self.layer2(self.layer1(self.prep(x)))).mean((2, 3)))


class _RefResNet18(nn.Module):
    """... of resnet18(norm="group") (torchvision layout; an identity shortcut is ``downsample`` = None
    there, an empty Sequential here: no keys either way)."""

    def __init__(self):
        super().__init__()
        self.conv1 = nn.Conv2d(3, 64, 7, 2, 3, bias=False)
        self.bn1 = nn.GroupNorm(32, 64)
        c = 64
        for i, w in enumerate((64, 128, 256, 512)):
            s = 1 if i == 0 else 2
            setattr(self, f"layer{i + 1}", nn.Sequential(_RefBlock(c, w, s, "downsample"), _RefBlock(w, w, 1, "downsample")))
            c = w
        self.fc = nn.Linear(512, 10)

    def forward(self, x):
        x = F.max_pool2d(F.relu(self.bn1(self.conv1(x))), 3, 2, 1)
        return self.fc(self.layer4(self.layer3(self.layer2(self.layer1(x)))).mean((2, 3)))


_TWINS = {"enhanced_cnn_small": _RefSmall, "resnet18_cifar": _RefResNet18}


def _model_and_twin(name):
    torch.manual_seed(0)
    m = build_model(name, norm="group")
    xavier_init(m)
    ref = _TWINS[name]()
    ref.load_state_dict(m.state_dict())
    with torch.no_grad():   # the bf16-rounded weights the kernels read
        for q in ref.parameters():
            if q.dim() > 1:
                q.copy_(q.bfloat16().float())
    ldnn.prepare(m, "cuda")
    return m, ref.cuda()


def _rel(a, b):
    a, b = a.detach().double().flatten(), b.detach().double().flatten()
    return ((a - b).norm() / b.norm().clamp_min(1e-30)).item()


@pytest.mark.parametrize("name", ["enhanced_cnn_small", "resnet18_cifar"])
def test_group_norm_model_three_sgd_steps_vs_fp32_twin(name):
    """Three eager SGD steps; before each, the twin takes the model's current weights (bf16-rounded
    where the kernels read the bf16 shadow), so every step compares the native forward and backward
    with fp32 at the same weights.  Bounds: tests/test_layers_gpu.py's for its BatchNorm models --
    EnhancedCNNSmall: logits rtol 5e-2 / atol 5e-2 max, loss 5 %, every parameter gradient's cosine
    > 0.98 (test_cnn_native_matches_cpu_fp32); ResNet-18: logits 4e-2, classifier gradients 6e-2 /
    2e-2 in relative L2 (test_cnn_forward_and_head_gradients_vs_fp32_oracle: the deep trunk's
    gradients are not well conditioned at model level in any bf16 implementation).
    A twin that steps on its own drifts away instead: ResNet-18 at 32x32 normalises 1x1 maps in
    groups of 16 values, its trunk gradients carry the bf16 noise into the weights, and two free
    runs at lr 5e-4 measured logits 1.0e-2, 2.4e-2, 3.7e-2 and fc.bias gradient 2.5e-2 apart at
    the third step -- a distance between two trainings, not an error of a pass."""
    from ldnn.optim import SGD

    m, ref = _model_and_twin(name)
    assert not any(isinstance(q, nn.BatchNorm2d) for q in m.modules())
    # (a rate at which the fp32 twin's loss stays where it started over the three steps: at 0.05 the
    # Xavier-initialised GroupNorm nets jump from a loss of 3 to 15 and the comparison is of two blow-ups)
    opt = SGD(m.parameters(), lr=5e-4)
    crit = CrossEntropyLoss()
    g = torch.Generator(device="cuda").manual_seed(7)
    for step in range(3):
        x = torch.randn(8, 3, 32, 32, device="cuda", generator=g).bfloat16()
        y = torch.randint(0, 10, (8,), device="cuda", generator=g)
        opt.zero_grad()
        out = m(x)
        lo = crit(out, y)
        lo.backward()
        with torch.no_grad():
            twin = dict(ref.named_parameters())
            for n, p in m.named_parameters():
                twin[n].copy_(p.bfloat16().float() if p.dim() > 1 else p)
        ref.zero_grad()
        ro = ref(x.float())
        lr_ = F.cross_entropy(ro, y)
        lr_.backward()
        print(f"{name} step {step}: loss {lo.item():.4f} vs {lr_.item():.4f}, logits rel {_rel(out.float(), ro):.3e}")
        assert abs(lo.item() - lr_.item()) < 0.05 * max(1.0, lr_.item())
        if name == "enhanced_cnn_small":
            torch.testing.assert_close(out.float(), ro.detach(), rtol=5e-2, atol=5e-2 * ro.abs().max().item())
            for (n, p), (_, q) in zip(m.named_parameters(), ref.named_parameters()):
                cos = F.cosine_similarity(p.grad.float().flatten(), q.grad.flatten(), dim=0).item()
                assert cos > 0.98, (step, n, cos)
        else:
            assert _rel(out.float(), ro) < 4e-2, _rel(out.float(), ro)
            assert _rel(m.fc.weight.grad, ref.fc.weight.grad) < 6e-2, _rel(m.fc.weight.grad, ref.fc.weight.grad)
            assert _rel(m.fc.bias.grad, ref.fc.bias.grad) < 2e-2, _rel(m.fc.bias.grad, ref.fc.bias.grad)
        opt.step()


@pytest.mark.parametrize("name", ["enhanced_cnn_small", "resnet18_cifar"])
def test_group_norm_graphed_step_matches_eager(name):
    """A GroupNorm step captured once (train.graphed.GraphedStep) and replayed gives the eager
    steps' parameters, through an lr change between replays; bound and construction are
    tests/test_layers_gpu.py test_graphed_step_matches_eager's: within the eager-vs-eager spread of
    the parameter updates plus a rounding-level floor, and pointing the same way."""
    from ldnn.optim import SGD
    from ldnn.train.graphed import GraphedStep

    torch.manual_seed(0)
    ms = [build_model(name, norm="group") for _ in range(3)]
    xavier_init(ms[0])
    for m in ms[1:]:
        m.load_state_dict(ms[0].state_dict())
    for m in ms:
        ldnn.prepare(m, "cuda")
    os_ = [SGD(m.parameters(), lr=2e-3, momentum=0.9) for m in ms]
    crit = CrossEntropyLoss()
    g = torch.Generator(device="cuda").manual_seed(1)
    xs = [torch.randn(8, 3, 32, 32, device="cuda", generator=g).bfloat16() for _ in range(4)]
    ys = [torch.randint(0, 10, (8,), device="cuda", generator=g) for _ in range(4)]
    for m, o in zip(ms, os_):    # one eager step each first (optimizer state and workspaces exist)
        o.zero_grad()
        crit(m(xs[0]), ys[0]).backward()
        o.step()
    p0 = [q.detach().clone() for q in ms[1].parameters()]
    ws0 = {n: q._ldnn_gn_ws.data_ptr() for n, q in ms[0].named_modules() if isinstance(q, GroupNorm)}
    gs = GraphedStep(ms[0], crit, os_[0], xs[1], ys[1], warmup=0)
    for i in range(1, 4):
        if i == 3:
            for o in os_:
                o.param_groups[0]["lr"] *= 0.1
        gs(xs[i], ys[i])
        for m, o in zip(ms[1:], os_[1:]):
            o.zero_grad()
            crit(m(xs[i]), ys[i]).backward()
            o.step()
    torch.cuda.synchronize()
    # the workspaces are the modules' own: capture and replay allocated none
    assert ws0 == {n: q._ldnn_gn_ws.data_ptr() for n, q in ms[0].named_modules() if isinstance(q, GroupNorm)}
    upd = [torch.cat([(t.detach() - r).flatten().double() for t, r in zip(m.parameters(), p0)]) for m in ms]
    for (n, p), (_, q), (_, s), r in zip(*(m.named_parameters() for m in ms), p0):
        d1, d2, d3 = ((t.detach() - r).flatten().double() for t in (p, q, s))
        eg, ee = (d1 - d2).norm().item(), (d3 - d2).norm().item()
        assert eg <= 3.0 * ee + 2e-3 * d2.norm().item(), (n, eg, ee, d2.norm().item())
        if name == "enhanced_cnn_small":
            cos, cos_ee = (F.cosine_similarity(d, d2, dim=0).item() for d in (d1, d3))
            assert cos > (0.9 if cos_ee >= 0.9 else cos_ee - 0.3), (n, cos, cos_ee)
    cos, cos_ee = (F.cosine_similarity(d, upd[1], dim=0).item() for d in (upd[0], upd[2]))
    assert cos > min(0.9, cos_ee - 0.1), (cos, cos_ee)
    assert list(ms[0].buffers()) == []
