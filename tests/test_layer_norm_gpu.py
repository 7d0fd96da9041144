"""Native bf16 LayerNorm with the activation fused, forward and backward (layer_norm.hip), against
F.layer_norm in fp32 on the same bf16-rounded inputs; and the LayerNorm MLPs against fp32 torch.nn
twins, eagerly and from a captured step."""
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import ldnn
from ldnn.models import CrossEntropyLoss, reseed_dropout
from ldnn.models.layers import LayerNorm
from ldnn.models.mlp import MLP
from ldnn.ops import _ext

pytestmark = pytest.mark.gpu

ACTS = ["none", "relu", "sigmoid"]
ACT_FN = {"none": lambda t: t, "relu": F.relu, "sigmoid": torch.sigmoid}
ACT_ID = {"none": -1, "relu": 0, "sigmoid": 1}


def _wmax():
    return int(_ext.C().ln_max_width())


def _shapes():
    """(B, N): the smallest shapes that reach each way the kernels can go wrong."""
    w = _wmax()
    return [
        (2, 1),         # variance 0, y = beta, dx = 0
        (3, 8),         # one vector
        (3, 33),        # tail of 1 in the last vector, odd rows, mostly idle lanes
        (5, 70),        # tail of 6
        (4, 64),        # dense
        (2, 512),       # exactly one vector per lane
        (7, 520),       # a second round with one busy lane
        (3, 4096),      # the flagship width
        (2, w),         # widest native row (above 4096: the parameter sums are a kernel of their own)
        (2, w + 8),     # takes the fallback
        (4100, 16),     # more rows than either grid covers at once (1025 workgroups' worth on 1024 and on 512)
        (1030, 200),    # 258 workgroups' partial rows, the last workgroup with idle waves
    ]


SHAPE_IDS = ["2x1", "3x8", "3x33", "5x70", "4x64", "2x512", "7x520", "3x4096", "2xWmax", "2xWmax+8", "4100x16",
             "1030x200"]

_CACHE = {}


def _case(B, N):
    """Inputs from a CPU generator (so the ReLU boundary shares below could be computed without a GPU)
    and the fp32 reference of the three activations, computed once per shape and left unchanged."""
    key = (B, N)
    if key not in _CACHE:
        g = torch.Generator().manual_seed(0)
        x = (1.5 * torch.randn(B, N, generator=g) + 0.5).bfloat16()
        dy = torch.randn(B, N, generator=g).bfloat16()
        g1 = torch.Generator().manual_seed(1)
        gamma = 1 + 0.3 * torch.randn(N, generator=g1)
        beta = 0.2 * torch.randn(N, generator=g1)
        x, dy, gamma, beta = (t.cuda() for t in (x, dy, gamma, beta))
        ref = {}
        for act in ACTS:
            xf = x.float().requires_grad_(True)
            w, b = gamma.clone().requires_grad_(True), beta.clone().requires_grad_(True)
            pre = F.layer_norm(xf, (N,), w, b, 1e-5)
            y = ACT_FN[act](pre)
            y.backward(dy.float())
            ref[act] = dict(y=y.detach(), pre=pre.detach(), dx=xf.grad, dgamma=w.grad, dbeta=b.grad)
        _CACHE[key] = (x, dy, gamma, beta, ref)
    return _CACHE[key]


def _module(N, gamma=None, beta=None, affine=True):
    ln = LayerNorm(N, elementwise_affine=affine)
    if affine and gamma is not None:
        with torch.no_grad():
            ln.weight.copy_(gamma)
            ln.bias.copy_(beta)
    ldnn.prepare(ln, "cuda")
    return ln


def _native(ln, x, dy, act):
    xb = x.clone().requires_grad_(True)
    y = ln.act(xb, act)
    y.backward(dy)
    return y.detach(), xb.grad


def _compare(tag, act, y, dx, dgamma, dbeta, ref):
    torch.testing.assert_close(y.float(), ref["y"], rtol=2e-2, atol=3e-2)
    keep = torch.ones_like(ref["pre"], dtype=torch.bool)
    if act == "relu":
        # an element whose reference pre-activation is within 1e-3 of zero may sit on the other side
        # of the ReLU after bf16 rounding: left out of the dx comparison, at most 1 % of a case
        keep = ref["pre"].abs() > 1e-3
        share = 1.0 - keep.float().mean().item()
        print(f"{tag} relu boundary share {share:.4%}")
        assert share <= 0.01, share
    want = ref["dx"]
    err = ((dx.float() - want).abs() * keep).max().item()
    print(f"{tag} {act} y: max err {(y.float() - ref['y']).abs().max().item():.3e}; dx: max err {err:.3e} of "
          f"max|ref| {want.abs().max().item():.3e}")
    torch.testing.assert_close(torch.where(keep, dx.float(), want), want, rtol=3e-2, atol=3e-2 * want.abs().max().item())
    for name, got in (("dgamma", dgamma), ("dbeta", dbeta)):
        if got is None:
            continue
        want = ref[name]
        print(f"{tag} {act} {name}: max err {(got - want).abs().max().item():.3e} of {want.abs().max().item():.3e}")
        torch.testing.assert_close(got, want, rtol=2e-2, atol=2e-2 * want.abs().max().item())


@pytest.mark.parametrize("act", ACTS)
@pytest.mark.parametrize("idx", range(12), ids=SHAPE_IDS)
def test_layer_norm_fused_vs_fp32(idx, act):
    B, N = _shapes()[idx]
    x, dy, gamma, beta, ref = _case(B, N)
    ln = _module(N, gamma, beta)
    y, dx = _native(ln, x, dy, act)
    assert y.dtype == torch.bfloat16 and y.shape == x.shape and dx.shape == x.shape and dx.dtype == torch.bfloat16
    _compare(f"({B}, {N})", act, y, dx, ln.weight.grad, ln.bias.grad, ref[act])
    native = N <= _wmax()
    assert (ln.__dict__.get("_ldnn_ln_ws") is not None) == native   # the fallback made no native call
    if N == 1:   # a row of one element: variance 0, xhat = 0, y = act(beta), and dx = 0
        torch.testing.assert_close(y.float(), ACT_FN[act](beta).expand(B, 1), rtol=2e-2, atol=3e-2)
        assert dx.float().abs().max().item() <= 1e-6


@pytest.mark.parametrize("act", ACTS)
def test_no_affine_instance(act):
    B, N = 5, 70
    x, dy, _, _, _ = _case(B, N)
    ln = _module(N, affine=False)
    assert list(ln.parameters()) == []
    xf = x.float().requires_grad_(True)
    pre = F.layer_norm(xf, (N,), None, None, 1e-5)
    yr = ACT_FN[act](pre)
    yr.backward(dy.float())
    y, dx = _native(ln, x, dy, act)
    _compare(f"({B}, {N}) no affine", act, y, dx, None, None, dict(y=yr.detach(), pre=pre.detach(), dx=xf.grad))
    assert ln.__dict__.get("_ldnn_ln_ws") is None    # no parameter sums, no workspace


@pytest.mark.parametrize("shape", [(1030, 200), (3, 4096)])
def test_two_runs_are_bit_equal(shape):
    B, N = shape
    x, dy, gamma, beta, _ = _case(B, N)
    out = []
    for _ in range(2):
        ln = _module(N, gamma, beta)
        y, dx = _native(ln, x, dy, "relu")
        out.append((y, dx, ln.weight.grad.clone(), ln.bias.grad.clone()))
    for a, b in zip(*out):
        assert torch.equal(a, b)


def test_second_backward_accumulates_and_lazy_zero_grad_overwrites():
    B, N = 5, 70
    x, dy, gamma, beta, ref = _case(B, N)
    ln = _module(N, gamma, beta)
    flat = ln._ldnn_flat
    _native(ln, x, dy, "relu")
    once_g, once_b = ln.weight.grad.clone(), ln.bias.grad.clone()
    _native(ln, x, dy, "relu")            # no zero_grad: grad_assign = False, the totals are added
    torch.testing.assert_close(ln.weight.grad, 2 * once_g, rtol=1e-6, atol=1e-6 * once_g.abs().max().item())
    torch.testing.assert_close(ln.bias.grad, 2 * once_b, rtol=1e-6, atol=1e-6 * once_b.abs().max().item())
    flat.zero_grad(lazy=True)              # marked zero only: the next backward overwrites
    _native(ln, x, dy, "relu")
    assert torch.equal(ln.weight.grad, once_g) and torch.equal(ln.bias.grad, once_b)
    torch.testing.assert_close(once_g, ref["relu"]["dgamma"], rtol=2e-2, atol=2e-2 * ref["relu"]["dgamma"].abs().max().item())
    # the storage's pad entries (70 -> 72) are never written
    assert flat.grad_storage(ln.weight)[N:].abs().max().item() == 0


def test_mixed_first_write_clears_only_the_fresh_gradient():
    """The weight's gradient already written this step, the bias's still marked zero by the lazy
    zero_grad: the backward adds dgamma onto the written one and clears the stale bias storage (all
    24 entries of the padded 20) before adding dbeta (0 + total: the same bits as the store).  The
    totals come from one clean backward of an identically seeded twin."""
    B, N = 5, 20
    x, dy, gamma, beta, _ = _case(B, N)
    ln, twin = _module(N, gamma, beta), _module(N, gamma, beta)
    flat = ln._ldnn_flat
    _native(twin, x, dy, "relu")
    dgamma, dbeta = twin.weight.grad.clone(), twin.bias.grad.clone()
    _native(ln, 3 * x, dy, "relu")            # native ops write both; their buffers now hold other totals
    flat.zero_grad(lazy=True)
    ln.weight.grad.fill_(1.0)
    assert flat.grad_beta(ln.weight) == 0.0   # a caller wrote the weight's gradient: no longer fresh
    _native(ln, x, dy, "relu")
    torch.testing.assert_close(ln.weight.grad, 1 + dgamma, rtol=1e-6, atol=1e-6 * dgamma.abs().max().item())
    assert torch.equal(ln.bias.grad, dbeta)
    # the storages' pad entries (20 -> 24) stay zero
    assert flat.grad_storage(ln.weight)[N:].abs().max().item() == 0
    assert flat.grad_storage(ln.bias)[N:].abs().max().item() == 0


def _up8(n):
    return (n + 7) // 8 * 8


def _vec8(t):
    """A [N] fp32 vector in a buffer of N rounded up to 8 floats, NaN behind it (the kernels' operand)."""
    buf = torch.full((_up8(t.numel()),), float("nan"), device="cuda")
    buf[:t.numel()] = t
    return buf


@pytest.mark.parametrize("act", ["relu", "sigmoid"])
@pytest.mark.parametrize("N", [33, 64])
def test_padding_is_not_read_and_nothing_outside_is_written(N, act):
    """x and dy [B, N] views of NaN-filled buffers with ld = up8(N) + 8, 16-byte and not 32-byte aligned;
    y and dx whole rows between sentinel rows: no NaN in any result, the outputs' pad columns exactly 0,
    nothing outside written, everything bit-equal to the call on plain buffers."""
    from strided import assert_no_poison, assert_outside_untouched, poisoned, write_inside

    C_ = _ext.C()
    B = 5
    xs, dys, gamma, beta, ref = _case(B, N) if N == 33 else _case(4, 64)
    B = xs.shape[0]
    ld = _up8(N) + 8
    gm, bt = _vec8(gamma), _vec8(beta)

    def run(make_in, make_out):
        x, dy = make_in(xs), make_in(dys)
        y, dx = make_out(), make_out()
        mean, rstd = torch.empty(B, device="cuda"), torch.empty(B, device="cuda")
        ws = torch.empty(C_.ln_workspace_floats(B, N), device="cuda")
        dg, db = torch.zeros(_up8(N), device="cuda"), torch.zeros(_up8(N), device="cuda")
        C_.ln_fwd(x[0], y[0][:, :N], gm, bt, mean, rstd, 1e-5, ACT_ID[act])
        C_.ln_bwd(x[0], dy[0], dx[0][:, :N], gm, bt, mean, rstd, ws, dg, db, ACT_ID[act], grad_assign=True)
        torch.cuda.synchronize()
        return (y, dx), (mean, rstd, dg, db)

    def plain_in(t):     # the same stride, zeros in the pad columns
        buf = torch.zeros(B, ld, dtype=torch.bfloat16, device="cuda")
        buf[:, :N] = t
        return buf[:, :N], None

    def plain_out():
        return torch.full((B, ld), 7.0, dtype=torch.bfloat16, device="cuda"), None

    def poisoned_in(t):
        v, h = poisoned(B, N, ld=ld, before=3, after=5, dtype=torch.bfloat16, device="cuda", fill="nan")
        write_inside(v, t)
        return v, h

    def poisoned_out():
        return poisoned(B, ld, ld=ld, before=3, after=5, dtype=torch.bfloat16, device="cuda", fill="sentinel",
                        full_rows=True)

    outs_d, vecs_d = run(plain_in, plain_out)
    outs_p, vecs_p = run(poisoned_in, poisoned_out)
    for name, (vd, _), (vp, hp) in zip(("y", "dx"), outs_d, outs_p):
        assert vp.data_ptr() % 16 == 0 and vp.data_ptr() % 32 != 0
        assert_outside_untouched(hp, name)
        assert_no_poison(vp, name)
        assert torch.equal(vp, vd), name
        assert (vp[:, N:].view(torch.int16) == 0).all(), f"{name}: pad columns"     # +0, also under sigmoid
    for name, a, b in zip(("mean", "rstd", "dgamma", "dbeta"), vecs_d, vecs_p):
        assert torch.isfinite(a).all() and torch.equal(a, b), name
    y, dx = outs_p[0][0][:, :N], outs_p[1][0][:, :N]
    _compare(f"strided ({B}, {N})", act, y, dx, vecs_p[2][:N], vecs_p[3][:N], ref[act])
    if N % 8:    # the gradients' pad entries are not written
        assert vecs_p[2][N:].abs().max().item() == 0 and vecs_p[3][N:].abs().max().item() == 0


def test_binding_refuses_bad_arguments():
    C_ = _ext.C()
    B, N = 4, 64
    W = _wmax()
    x = torch.randn(B, N, device="cuda").bfloat16()
    y, dy, dx = torch.empty_like(x), torch.randn(B, N, device="cuda").bfloat16(), torch.empty_like(x)
    mean, rstd = torch.empty(B, device="cuda"), torch.empty(B, device="cuda")
    gm, bt = torch.ones(N, device="cuda"), torch.zeros(N, device="cuda")
    dg, db = torch.zeros(N, device="cuda"), torch.zeros(N, device="cuda")
    ws = torch.empty(C_.ln_workspace_floats(B, N), device="cuda")
    assert ws.numel() >= 2 * N
    C_.ln_fwd(x, y, gm, bt, mean, rstd, 1e-5, 0)
    C_.ln_bwd(x, dy, dx, gm, bt, mean, rstd, ws, dg, db, 0, grad_assign=True)
    x12 = torch.randn(B, 12, device="cuda").bfloat16()                       # row stride 12
    x8 = torch.zeros(x.numel() + 8, dtype=torch.bfloat16, device="cuda")[4:4 + x.numel()].view(B, N)
    assert x8.data_ptr() % 16 == 8
    wide = torch.zeros(2, W + 8, dtype=torch.bfloat16, device="cuda")
    for bad in (lambda: C_.ln_fwd(x12, torch.empty_like(x12), None, None, mean, rstd, 1e-5, 0),       # ld % 8
                lambda: C_.ln_fwd(x8, y, gm, bt, mean, rstd, 1e-5, 0),                                # 8-B aligned x
                lambda: C_.ln_fwd(x, x8, gm, bt, mean, rstd, 1e-5, 0),                                # 8-B aligned y
                lambda: C_.ln_fwd(wide, torch.empty_like(wide), None, None, mean, rstd, 1e-5, 0),     # N > W_max
                lambda: C_.ln_fwd(x, y, gm, bt, mean[:2], rstd, 1e-5, 0),                             # short mean
                lambda: C_.ln_fwd(x, y, gm, bt, mean, rstd[:2], 1e-5, 0),                             # short rstd
                lambda: C_.ln_fwd(x, y[:2], gm, bt, mean, rstd, 1e-5, 0),                             # shape
                lambda: C_.ln_fwd(x, y, gm[:32], bt, mean, rstd, 1e-5, 0),                            # short gamma
                lambda: C_.ln_fwd(x, y, gm, None, mean, rstd, 1e-5, 0),                               # gamma, no beta
                lambda: C_.ln_fwd(x, y.float(), gm, bt, mean, rstd, 1e-5, 0),                         # dtype
                lambda: C_.ln_fwd(x.cpu(), y, gm, bt, mean, rstd, 1e-5, 0),                           # device
                lambda: C_.ln_fwd(x, y, gm, bt, mean.cpu(), rstd, 1e-5, 0),                           # device
                lambda: C_.ln_fwd(x, x, gm, bt, mean, rstd, 1e-5, 0),                                 # in place
                lambda: C_.ln_fwd(x, y, gm, bt, mean, rstd, 1e-5, 2),                                 # act range
                lambda: C_.ln_fwd(x, y, gm, bt, mean, rstd, 1e-5, -2),
                lambda: C_.ln_bwd(x, dy, dx, gm, bt, mean, rstd, ws[:16], dg, db, 0),                 # short workspace
                lambda: C_.ln_bwd(x, dy, dx, gm, bt, mean, rstd, None, dg, db, 0),                    # no workspace
                lambda: C_.ln_bwd(x, dy, x, gm, bt, mean, rstd, ws, dg, db, 0),                       # in place
                lambda: C_.ln_bwd(x, dy, dy, gm, bt, mean, rstd, ws, dg, db, 0),
                lambda: C_.ln_bwd(x, dy, dx, gm, bt, mean, rstd, ws, dg, None, 0),                    # dgamma, no dbeta
                lambda: C_.ln_bwd(x, dy, dx, None, None, mean, rstd, ws, dg, db, 0),                  # dgamma, no gamma
                lambda: C_.ln_bwd(x, dy, dx, gm, bt, mean, rstd, ws, None, None, 0)):                 # gamma, no dgamma
        with pytest.raises(RuntimeError):
            bad()
    # a view whose storage ends before its last row's last vector is refused, not read
    short = torch.zeros(2 * 16 - 4, dtype=torch.bfloat16, device="cuda").as_strided((2, 10), (16, 1))
    with pytest.raises(RuntimeError):
        C_.ln_fwd(short, torch.zeros(2, 16, dtype=torch.bfloat16, device="cuda")[:, :10], None, None, mean, rstd, 1e-5, 0)
    torch.cuda.synchronize()


# ---- model level ---------------------------------------------------------------------------

class _RefMLP(nn.Module):
    """Plain torch.nn twin of MLP(norm="layer"): same state_dict keys, no ldnn layer."""

    def __init__(self, dims, activation):
        super().__init__()
        self.layers = nn.ModuleList(nn.Linear(dims[i], dims[i + 1]) for i in range(len(dims) - 1))
        self.norms = nn.ModuleList(nn.LayerNorm(w) for w in dims[1:-1])
        self.fn = ACT_FN[activation]

    def forward(self, x):
        for i, layer in enumerate(self.layers):
            x = layer(x)
            if i < len(self.norms):
                x = self.fn(self.norms[i](x))
        return x


def _xavier(m):
    for q in m.modules():
        if isinstance(q, nn.Linear):
            nn.init.xavier_uniform_(q.weight)
            nn.init.zeros_(q.bias)
        elif isinstance(q, nn.LayerNorm):
            with torch.no_grad():
                q.weight.add_(0.2 * torch.randn_like(q.weight))
                q.bias.add_(0.1 * torch.randn_like(q.bias))


@pytest.mark.parametrize("activation", ["relu", "sigmoid"])
@pytest.mark.parametrize("dims,batch", [((70, 33, 10), 24), ((784, 256, 10), 256)])
def test_layer_norm_model_three_sgd_steps_vs_fp32_twin(dims, batch, activation):
    """Three eager SGD steps; before each comparison the twin takes the model's current weights
    (bf16-rounded where the kernels read the bf16 shadow), so every step compares the native forward
    and backward with fp32 at the same weights (tests/test_group_norm_gpu.py's construction).  Bounds:
    tests/test_layers_gpu.py's -- loss within 0.05, logits rtol 5e-2 / atol 5e-2 max, every parameter
    gradient's cosine > 0.98."""
    from ldnn.optim import SGD

    torch.manual_seed(0)
    m = MLP(dims[0], dims[1:-1], dims[-1], activation=activation, norm="layer")
    _xavier(m)
    ref = _RefMLP(dims, activation).cuda()
    ldnn.prepare(m, "cuda")
    opt = SGD(m.parameters(), lr=0.05)
    crit = CrossEntropyLoss()
    g = torch.Generator(device="cuda").manual_seed(7)
    for step in range(3):
        x = torch.randn(batch, dims[0], device="cuda", generator=g).bfloat16()
        y = torch.randint(0, dims[-1], (batch,), device="cuda", generator=g)
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
        print(f"{dims} {activation} step {step}: loss {lo.item():.4f} vs {lr_.item():.4f}")
        assert abs(lo.item() - lr_.item()) < 0.05
        torch.testing.assert_close(out.float(), ro.detach(), rtol=5e-2, atol=5e-2 * ro.abs().max().item())
        for (n, p), (_, q) in zip(m.named_parameters(), ref.named_parameters()):
            cos = F.cosine_similarity(p.grad.float().flatten(), q.grad.flatten(), dim=0).item()
            assert cos > 0.98, (step, n, cos)
        opt.step()


def test_layer_norm_graphed_step_matches_eager():
    """A LayerNorm step captured once (train.graphed.GraphedStep) and replayed gives the eager steps'
    parameters, through an lr change between replays; bound and construction are
    tests/test_group_norm_gpu.py test_group_norm_graphed_step_matches_eager's: within the
    eager-vs-eager spread of the parameter updates plus a rounding-level floor, and pointing the same
    way.  The modules' workspaces are untouched by capture and replay."""
    from ldnn.optim import SGD
    from ldnn.train.graphed import GraphedStep

    torch.manual_seed(0)
    ms = [MLP(784, (256, 256), 10, norm="layer") for _ in range(3)]
    _xavier(ms[0])
    for m in ms[1:]:
        m.load_state_dict(ms[0].state_dict())
    for m in ms:
        ldnn.prepare(m, "cuda")
    os_ = [SGD(m.parameters(), lr=2e-2, momentum=0.9) for m in ms]
    crit = CrossEntropyLoss()
    g = torch.Generator(device="cuda").manual_seed(1)
    xs = [torch.randn(64, 784, device="cuda", generator=g).bfloat16() for _ in range(4)]
    ys = [torch.randint(0, 10, (64,), device="cuda", generator=g) for _ in range(4)]
    for m, o in zip(ms, os_):    # one eager step each first (optimizer state and workspaces exist)
        o.zero_grad()
        crit(m(xs[0]), ys[0]).backward()
        o.step()
    p0 = [q.detach().clone() for q in ms[1].parameters()]
    ws0 = [q._ldnn_ln_ws.data_ptr() for q in ms[0].norms]
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
    assert ws0 == [q._ldnn_ln_ws.data_ptr() for q in ms[0].norms]
    upd = [torch.cat([(t.detach() - r).flatten().double() for t, r in zip(m.parameters(), p0)]) for m in ms]
    for (n, p), (_, q), (_, s), r in zip(*(m.named_parameters() for m in ms), p0):
        d1, d2, d3 = ((t.detach() - r).flatten().double() for t in (p, q, s))
        assert d2.norm().item() > 0, n
        eg, ee = (d1 - d2).norm().item(), (d3 - d2).norm().item()
        assert eg <= 3.0 * ee + 2e-3 * d2.norm().item(), (n, eg, ee, d2.norm().item())
        cos, cos_ee = (F.cosine_similarity(d, d2, dim=0).item() for d in (d1, d3))
        assert cos > (0.9 if cos_ee >= 0.9 else cos_ee - 0.3), (n, cos, cos_ee)
    cos, cos_ee = (F.cosine_similarity(d, upd[1], dim=0).item() for d in (upd[0], upd[2]))
    assert cos > min(0.9, cos_ee - 0.1), (cos, cos_ee)
    assert list(ms[0].buffers()) == []


def test_dropout_after_layer_norm_runs_and_drops_what_the_cpu_drops():
    """Linear -> LayerNorm + sigmoid -> Dropout: a GPU step runs, and with equal seeds the CPU path drops
    the same elements (a sigmoid output is never 0, so the dropout output's zeros are the mask)."""
    from ldnn.optim import SGD

    torch.manual_seed(0)
    seen = {}
    models = {}
    x = torch.randn(24, 70).bfloat16()
    y = torch.randint(0, 10, (24,))
    for dev in ("cpu", "cuda"):
        torch.manual_seed(0)
        m = MLP(70, (33,), 10, activation="sigmoid", dropout=0.3, norm="layer")
        ldnn.prepare(m, dev)
        reseed_dropout(m, 11)
        m.drops[0].register_forward_hook(lambda mod, inp, out, dev=dev: seen.__setitem__(dev, out.detach().float().cpu()))
        m.train()
        opt = SGD(m.parameters(), lr=0.05)
        opt.zero_grad()
        loss = CrossEntropyLoss()(m(x.to(dev) if dev == "cuda" else x.float()), y.to(dev))
        loss.backward()
        opt.step()
        assert torch.isfinite(loss).item()
        assert all(torch.isfinite(p).all() for p in m.parameters())
        models[dev] = m
    torch.cuda.synchronize()
    zc, zg = seen["cpu"] == 0, seen["cuda"] == 0
    assert zc.shape == (24, 33) and 0.15 < zc.float().mean().item() < 0.45
    assert torch.equal(zc, zg)


@pytest.mark.parametrize("activation", ["relu", "sigmoid"])
def test_hand_on_from_linear_to_layer_norm_to_linear_is_copy_free(activation):
    """The [B, 33] view of the [B, 40] buffer the first Linear wrote is the LayerNorm kernels' operand,
    and the LayerNorm's output -- such a view again, pad columns zeroed -- is the next Linear's."""
    torch.manual_seed(0)
    m = MLP(70, (33,), 10, activation=activation, norm="layer")
    ldnn.prepare(m, "cuda")
    x = torch.randn(24, 70, device="cuda").bfloat16()
    h = m.layers[0](x)
    assert h.shape == (24, 33) and h.stride() == (40, 1)
    n = m.norms[0].act(h, activation)
    out = m.layers[1](n)
    assert n.shape == (24, 33) and n.stride() == (40, 1) and getattr(n, "_ldnn_zpad", False) is True
    saved = n.grad_fn.saved_tensors[0]                      # the operand the LayerNorm kernels read
    assert saved.untyped_storage().data_ptr() == h.untyped_storage().data_ptr() and saved.stride() == (40, 1)
    nxt = out.grad_fn.saved_tensors[0]                      # the operand the next GEMM read, widened in place
    assert nxt.untyped_storage().data_ptr() == n.untyped_storage().data_ptr() and nxt.shape == (24, 40)
    whole = n.as_strided((24, 40), (40, 1), n.storage_offset())
    assert (whole[:, 33:].view(torch.int16) == 0).all()     # zeros also under sigmoid
    out.float().sum().backward()
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in m.parameters())
