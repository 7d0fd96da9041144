"""Class weights and ignore_index in the fused softmax cross-entropy (xent.hip weighted instances and
the xent_wden pre-pass) against ``F.cross_entropy(logits.float(), target, weight=, ignore_index=,
label_smoothing=)`` on the same bf16 logits and its autograd gradient.

Over labels the kernel's gradient is the mean loss's (the divisor, the kept rows' weight sum, is formed
on the device); over probability targets direct calls use grad_scale = 1 like test_soft_targets_gpu.py.
Tolerances are the project's for this kernel (test_soft_targets_gpu.py): loss rtol 1e-4 / atol 1e-4,
#correct exact (over kept rows), gradient rtol 2e-2 / atol 1e-4, pad columns and ignored rows exactly 0,
bias sums within 1e-6 * sum |d| of the float64 column sums of the stored bf16 gradient.
"""
import pytest
import torch
import torch.nn.functional as F

import ldnn
from ldnn.ops import _ext
from ldnn.ops import functional as LF

pytestmark = pytest.mark.gpu

# (B, C, ld): rows kernel with a partial last workgroup / fewer rows than a wave / the LD = 64 instance /
# wave kernel with 4 rows per block / wave kernel with 16 rows per block and a padded stride
SHAPES = [(300, 10, 16), (5, 3, 8), (257, 64, 64), (64, 1000, 1000), (1100, 65, 72)]


def C():
    return _ext.C()


def _gen(seed):
    return torch.Generator(device="cuda").manual_seed(seed)


def _logits(B, Cc, ld, seed=41):
    return (torch.randn(B, ld, device="cuda", generator=_gen(seed)) * 3).bfloat16()[:, :Cc]


def _weights(Cc, seed=42):
    """fp32 [C] in [0, 3] with one exact 0."""
    w = torch.rand(Cc, device="cuda", generator=_gen(seed)) * 3
    w[1] = 0.0
    return w


def _labels(B, Cc, ignore_index, seed=43):
    """Labels with about a fifth of the rows ignored, row 0 and the last row among them."""
    y = torch.randint(0, Cc, (B,), device="cuda", generator=_gen(seed))
    ign = torch.rand(B, device="cuda", generator=_gen(seed + 1)) < 0.2
    ign[0] = ign[-1] = True
    if B > 2:
        ign[1] = False
    y[ign] = ignore_index
    if ignore_index >= 0:
        ign = y == ignore_index   # (rows that drew the class itself are ignored too, as in torch)
    return y, ign


def _targets(B, Cc, seed=45):
    q = torch.rand(B, Cc, device="cuda", generator=_gen(seed))
    top = torch.randint(0, Cc, (B,), device="cuda", generator=_gen(seed + 1))
    q[torch.arange(B, device="cuda"), top] = 1.25   # (an unambiguous argmax)
    return q / q.sum(1, keepdim=True)


def _oracle(logits, target, w, ignore_index, eps, scale=1.0):
    """(mean loss, d(scale * mean loss)/d logits, #correct over kept rows) in fp32 from torch."""
    lf = logits.float().requires_grad_(True)
    soft = target.dim() == 2
    kw = {} if soft else dict(ignore_index=ignore_index)
    loss = F.cross_entropy(lf, target, weight=w, label_smoothing=eps, **kw)
    (loss * scale).backward()
    hit = lf.detach().argmax(1) == (target.argmax(1) if soft else target)
    if not soft:
        hit &= target != ignore_index
    return loss.detach(), lf.grad, int(hit.sum().item())


def _kernel(logits, target, ld, w, ignore_index=-100, eps=0.0, **kw):
    B, Cc = logits.shape
    dl = torch.full((B, ld), 7.0, device="cuda", dtype=torch.bfloat16)
    stats = torch.zeros(2, device="cuda")
    db = torch.zeros(ld, device="cuda")
    if target.dim() == 2:
        C().softmax_xent_soft_w(logits, target, dl[:, :Cc], stats, dbias=db, num_classes=Cc, grad_scale=1.0,
                                label_smoothing=eps, weight=w, **kw)
    else:
        C().softmax_xent_w(logits, target, dl[:, :Cc], stats, dbias=db, num_classes=Cc, label_smoothing=eps,
                           weight=w, ignore_index=ignore_index, **kw)
    return dl, stats, db


def _check(dl, stats, db, ref, B, Cc, ignored=None):
    loss, grad, correct = ref
    print(f"loss {stats[0].item() / B:.6f} ref {loss.item():.6f}  correct {stats[1].item():.0f} ref {correct}  "
          f"max |dgrad| {(dl[:, :Cc].float() - grad).abs().max().item():.3e} of max |grad| {grad.abs().max().item():.3e}")
    torch.testing.assert_close(stats[0] / B, loss, rtol=1e-4, atol=1e-4)
    assert stats[1].item() == correct
    torch.testing.assert_close(dl[:, :Cc].float(), grad, rtol=2e-2, atol=1e-4)
    if dl.shape[1] > Cc:
        assert dl[:, Cc:].float().abs().max().item() == 0.0
    if ignored is not None and bool(ignored.any()):
        assert dl[ignored].float().abs().max().item() == 0.0
    d64 = dl.double()
    err = (db.double() - d64.sum(0)).abs()
    bound = 1e-6 * d64.abs().sum(0)
    assert bool((err <= bound).all()), (err.max().item(), bound.min().item())


@pytest.mark.parametrize("ignore_index", [-100, 2])
@pytest.mark.parametrize("eps", [0.0, 0.1])
@pytest.mark.parametrize("B,Cc,ld", SHAPES)
def test_weighted_kernel_matches_torch(B, Cc, ld, eps, ignore_index):
    logits, w = _logits(B, Cc, ld), _weights(Cc)
    y, ign = _labels(B, Cc, ignore_index)
    dl, stats, db = _kernel(logits, y, ld, w, ignore_index, eps)
    _check(dl, stats, db, _oracle(logits, y, w, ignore_index, eps), B, Cc, ign)
    den = C().xent_wden_ws(logits)
    # (non-negative terms, at most 5 per thread and then a 10-level tree: ~15 fp32 roundings of the sum)
    torch.testing.assert_close(den[0].double(), w.double()[y[~ign]].sum(), rtol=1e-5, atol=0)
    assert den[2].item() == int((~ign).sum())


@pytest.mark.parametrize("eps", [0.0, 0.1])
@pytest.mark.parametrize("B,Cc,ld", SHAPES)
def test_weighted_soft_kernel_matches_torch(B, Cc, ld, eps):
    logits, w, q = _logits(B, Cc, ld), _weights(Cc), _targets(B, Cc)
    dl, stats, db = _kernel(logits, q, ld, w, eps=eps)
    _check(dl, stats, db, _oracle(logits, q, w, -100, eps, scale=B), B, Cc)


@pytest.mark.parametrize("eps", [0.0, 0.1])
@pytest.mark.parametrize("B,Cc,ld", SHAPES)
def test_unit_weights_reproduce_the_unweighted_op(B, Cc, ld, eps):
    logits = _logits(B, Cc, ld, seed=47)
    y = torch.randint(0, Cc, (B,), device="cuda", generator=_gen(48))
    dl, stats, _ = _kernel(logits, y, ld, torch.ones(Cc, device="cuda"), eps=eps)
    dh = torch.full((B, ld), 7.0, device="cuda", dtype=torch.bfloat16)
    sh = torch.zeros(2, device="cuda")
    C().softmax_xent(logits, y, dh[:, :Cc], sh, dbias=None, num_classes=Cc, grad_scale=1.0 / B, label_smoothing=eps)
    torch.testing.assert_close(stats[0] / B, sh[0] / B, rtol=1e-4, atol=1e-4)
    assert stats[1].item() == sh[1].item()
    torch.testing.assert_close(dl.float(), dh.float(), rtol=2e-2, atol=1e-4)
    # probability targets likewise
    q = _targets(B, Cc, seed=49)
    dl, stats, _ = _kernel(logits, q, ld, torch.ones(Cc, device="cuda"), eps=eps)
    C().softmax_xent_soft(logits, q, dh[:, :Cc], sh.zero_(), dbias=None, num_classes=Cc, grad_scale=1.0,
                          label_smoothing=eps)
    torch.testing.assert_close(stats[0] / B, sh[0] / B, rtol=1e-4, atol=1e-4)
    assert stats[1].item() == sh[1].item()
    torch.testing.assert_close(dl.float(), dh.float(), rtol=2e-2, atol=1e-4)


@pytest.mark.parametrize("B,Cc,ld", SHAPES)
def test_no_weight_with_ignore_index_is_unit_weights(B, Cc, ld):
    logits = _logits(B, Cc, ld, seed=50)
    y, ign = _labels(B, Cc, 2, seed=51)
    a = _kernel(logits, y, ld, None, 2, 0.1)
    b = _kernel(logits, y, ld, torch.ones(Cc, device="cuda"), 2, 0.1)
    assert torch.equal(a[0], b[0])   # the gradient rows: the same arithmetic, bit for bit
    # (the statistics and bias sums are fp32 atomics over the blocks: the order may differ)
    torch.testing.assert_close(a[1][0] / B, b[1][0] / B, rtol=1e-4, atol=1e-4)
    assert a[1][1].item() == b[1][1].item()
    # each bias sum lies within 1e-6 * sum |d| of the exact column sum (_check), so two lie within twice that
    assert bool(((a[2] - b[2]).abs().double() <= 2e-6 * a[0].double().abs().sum(0)).all())
    _check(*a, _oracle(logits, y, None, 2, 0.1), B, Cc, ign)


@pytest.mark.parametrize("B,Cc,ld", SHAPES)
def test_out_of_range_labels_are_ignored(B, Cc, ld):
    """A label that is no class and not ignore_index: no error, treated as ignored, nothing outside
    the weights or the gradient rows is touched (canary words round both)."""
    logits = _logits(B, Cc, ld, seed=52)
    y, ign = _labels(B, Cc, -100, seed=53)
    bad = torch.zeros(B, dtype=torch.bool, device="cuda")
    bad[B // 2] = bad[min(3, B - 2)] = True
    y[B // 2], y[min(3, B - 2)] = Cc, -7
    y[1] = 0   # (a kept row of a class with weight > 0: at B = 5 it is the only kept row, and den must be > 0)
    wbuf = torch.full((Cc + 64,), 1e30, device="cuda")
    wbuf[32: 32 + Cc] = _weights(Cc)
    w = wbuf[32: 32 + Cc]
    dbuf = torch.full((B + 2, ld), 7.0, device="cuda", dtype=torch.bfloat16)
    dl = dbuf[1:-1]
    stats, db = torch.zeros(2, device="cuda"), torch.zeros(ld, device="cuda")
    C().softmax_xent_w(logits, y, dl[:, :Cc], stats, dbias=db, num_classes=Cc, label_smoothing=0.1, weight=w,
                       ignore_index=-100)
    torch.cuda.synchronize()
    assert bool((wbuf[:32] == 1e30).all()) and bool((wbuf[32 + Cc:] == 1e30).all())
    assert bool((dbuf[0].float() == 7.0).all()) and bool((dbuf[-1].float() == 7.0).all())
    yt = torch.where(bad, torch.full_like(y, -100), y)
    _check(dl, stats, db, _oracle(logits, yt, w, -100, 0.1), B, Cc, ign | bad)


@pytest.mark.parametrize("B,Cc,ld", SHAPES)
def test_two_launches_are_bit_identical(B, Cc, ld):
    logits, w = _logits(B, Cc, ld, seed=54), _weights(Cc, seed=55)
    y, _ = _labels(B, Cc, 2, seed=56)
    y[1] = 0   # (a kept row of a class with weight > 0: den > 0 at every shape)
    dl1, _, _ = _kernel(logits, y, ld, w, 2, 0.1)
    den1 = C().xent_wden_ws(logits).clone()
    dl2, _, _ = _kernel(logits, y, ld, w, 2, 0.1)
    den2 = C().xent_wden_ws(logits).clone()
    assert torch.equal(dl1.view(torch.int16), dl2.view(torch.int16))
    assert torch.equal(den1.view(torch.int32), den2.view(torch.int32))
    assert den1[0].item() > 0 and den1[1].item() == pytest.approx(1.0 / den1[0].item(), rel=1e-6)


@pytest.mark.parametrize("B,Cc,ld", SHAPES)
def test_all_ignored_batch_gives_zeros(B, Cc, ld):
    logits, w = _logits(B, Cc, ld, seed=57), _weights(Cc, seed=58)
    out = torch.full((2,), -5.0, device="cuda")
    for y in (torch.full((B,), 2, device="cuda"), torch.full((B,), 1, device="cuda")):   # all ignored / all weight 0
        dl, stats, db = _kernel(logits, y, ld, w, 2, 0.0, loss_out=out)
        assert out.tolist()[0] == 0.0 and stats[0].item() == 0.0
        assert dl.float().abs().max().item() == 0.0 and db.abs().max().item() == 0.0
        assert C().xent_wden_ws(logits)[:2].tolist() == [0.0, 0.0]
    assert out[1].item() == int((logits.float().argmax(1) == 1).sum())   # weight 0 rows are kept rows


@pytest.mark.parametrize("B,Cc,ld", [(300, 10, 16), (64, 1000, 1000)])
def test_weighted_finalize(B, Cc, ld):
    """loss_out: the last block writes [weighted mean loss, #correct], adds [B * mean loss, #correct]
    into stats once and leaves its accumulator zero for the next call (as test_soft_finalize)."""
    eps = 0.1
    logits, w = _logits(B, Cc, ld, seed=59), _weights(Cc, seed=60)
    y, _ = _labels(B, Cc, 2, seed=61)
    ref, _, correct = _oracle(logits, y, w, 2, eps)
    dl = torch.empty(B, ld, device="cuda", dtype=torch.bfloat16)
    stats = torch.tensor([1.0, 2.0], device="cuda")
    for _ in range(2):
        out = torch.full((2,), -5.0, device="cuda")
        C().softmax_xent_w(logits, y, dl[:, :Cc], stats, None, Cc, loss_out=out, label_smoothing=eps, weight=w,
                           ignore_index=2)
        torch.testing.assert_close(out[0], ref, rtol=1e-4, atol=1e-4)   # (a dirty accumulator would double it)
        assert out[1].item() == correct
    torch.testing.assert_close(stats, torch.tensor([1.0 + 2 * ref.item() * B, 2.0 + 2 * correct], device="cuda"),
                               rtol=1e-4, atol=1e-3)
    # probability targets: the host's scale, the unweighted convention
    q = _targets(B, Cc, seed=62)
    ref, _, correct = _oracle(logits, q, w, -100, eps)
    stats = torch.tensor([1.0, 2.0], device="cuda")
    for _ in range(2):
        out = torch.full((2,), -5.0, device="cuda")
        C().softmax_xent_soft_w(logits, q, dl[:, :Cc], stats, None, Cc, 1.0 / B, loss_out=out, loss_scale=1.0 / B,
                                label_smoothing=eps, weight=w)
        torch.testing.assert_close(out[0], ref, rtol=1e-4, atol=1e-4)
        assert out[1].item() == correct
    torch.testing.assert_close(stats, torch.tensor([1.0 + 2 * ref.item() * B, 2.0 + 2 * correct], device="cuda"),
                               rtol=1e-4, atol=1e-3)


def test_binding_refusals():
    B, Cc, ld = 64, 10, 16
    logits = _logits(B, Cc, ld)
    y = torch.randint(0, Cc, (B,), device="cuda")
    q = _targets(B, Cc)
    w = _weights(Cc)
    for target in (y, q):
        with pytest.raises(RuntimeError, match="weight"):
            _kernel(logits, target, ld, w.double())
        with pytest.raises(RuntimeError, match="weight"):
            _kernel(logits, target, ld, torch.ones(Cc + 1, device="cuda"))
        with pytest.raises(RuntimeError, match="weight"):
            _kernel(logits, target, ld, w.cpu())
        with pytest.raises(RuntimeError, match="weight"):
            _kernel(logits, target, ld, torch.ones(2 * Cc, device="cuda")[::2])
        with pytest.raises(RuntimeError, match="label_smoothing"):
            _kernel(logits, target, ld, w, eps=1.5)
    with pytest.raises(RuntimeError, match="labels"):   # xent_launch's own checks still apply
        _kernel(logits, y[:-1], ld, w)


def test_autograd_path():
    from ldnn.models import WeightedCrossEntropyLoss

    B = 96
    buf = _logits(B, 16, 16, seed=63)
    w = _weights(10, seed=64)
    y, _ = _labels(B, 10, 2, seed=65)
    q = _targets(B, 10, seed=66)
    crit = WeightedCrossEntropyLoss(weight=w.cpu(), ignore_index=2, label_smoothing=0.1)   # (the buffer follows the logits)
    for target in (y, q):
        logits = buf[:, :10].detach().requires_grad_(True)
        stats = torch.zeros(2, device="cuda")
        loss = crit(logits, target, stats)
        (B * loss).backward()
        ref, grad, correct = _oracle(buf[:, :10], target, w, 2, 0.1, scale=B)
        torch.testing.assert_close(loss.detach(), ref, rtol=1e-4, atol=1e-4)
        torch.testing.assert_close(logits.grad.float(), grad, rtol=2e-2, atol=2e-4)
        torch.testing.assert_close(stats, torch.tensor([ref.item() * B, float(correct)], device="cuda"),
                                   rtol=1e-4, atol=1e-3)
    assert crit.weight.is_cuda
    # the defaults take the unweighted launch: bit for bit the loss of the call without the keywords
    logits = buf[:, :10].detach()
    assert torch.equal(LF.cross_entropy(logits, y.clamp_min(0), None, 0.1, weight=None, ignore_index=-100),
                       LF.cross_entropy(logits, y.clamp_min(0), None, 0.1))


def test_graphed_step_follows_the_weights_in_place():
    from ldnn.models import CrossEntropyLoss, WeightedCrossEntropyLoss, xavier_init
    from ldnn.models.mlp import MLP
    from ldnn.optim import SGD
    from ldnn.train.graphed import GraphedStep

    torch.manual_seed(67)
    m = MLP(70, (33,), 10)
    xavier_init(m)
    ldnn.prepare(m, "cuda")
    opt = SGD(m.parameters(), lr=0.0, momentum=0.9)
    w1, w2 = _weights(10, seed=68), _weights(10, seed=69)
    crit = WeightedCrossEntropyLoss(weight=w1, ignore_index=2)
    B = 64
    x = (torch.randn(B, 70, device="cuda") * 4).bfloat16()
    y, _ = _labels(B, 10, 2, seed=70)
    gs = GraphedStep(m, crit, opt, x, y)
    with torch.no_grad():
        out = m(x).float()   # lr = 0: the logits of every step
    got1 = gs(x, y).item()
    crit.set_class_weights(w2.cpu())   # in place: the replay reads the new values
    got2 = gs(x, y).item()
    g2 = [p.grad.clone() for p in m.parameters()]
    refs = [F.cross_entropy(out, y, weight=w, ignore_index=2).item() for w in (w1, w2)]
    tols = [1e-4 + 1e-4 * abs(r) for r in refs]
    print(f"replayed {[got1, got2]}  ref {refs}")
    assert abs(got1 - refs[0]) <= tols[0] and abs(got2 - refs[1]) <= tols[1]
    assert abs(got1 - got2) > 10 * max(tols)
    # ... and equals an eager step with the new weights: the same kernels on the same inputs (one loss
    # workgroup: the same bits; the weight gradients may differ by the order of fp32 atomic sums)
    opt.zero_grad()
    loss = WeightedCrossEntropyLoss(weight=w2, ignore_index=2)(m(x), y)
    loss.backward()
    assert loss.item() == got2
    for a, p in zip(g2, m.parameters()):
        torch.testing.assert_close(a, p.grad, rtol=1e-4, atol=1e-6)
    # what the capture baked in must not change behind it
    crit.ignore_index = 3
    with pytest.raises(RuntimeError, match="ignore_index"):
        gs(x, y)
    crit.ignore_index = 2
    gs(x, y)
    old = crit.weight
    crit.weight = w2.clone()
    with pytest.raises(RuntimeError, match="different tensor"):
        gs(x, y)
    crit.weight = None
    with pytest.raises(RuntimeError, match="went away"):
        gs(x, y)
    crit.weight = old
    gs(x, y)
    plain = CrossEntropyLoss()
    gp = GraphedStep(m, plain, opt, x, y.clamp_min(0))
    plain.weight = w1.clone()
    with pytest.raises(RuntimeError, match="appeared"):
        gp(x, y.clamp_min(0))
    torch.cuda.synchronize()
