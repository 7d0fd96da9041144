"""Focal loss in the fused softmax cross-entropy (xent.hip XM_FOCAL instances on the xent_wden pre-pass)
against a float64 autograd oracle on the same bf16 logits.

The oracle (test_focal_loss.focal_oracle) forms q = 1 - p from the other classes' logits, so it stays finite
on the two planted rows of every case: row 0 (label logit +60, all others -60: q underflows in fp32, the
kernel writes a zero gradient row and adds 0 to the loss) and row 1 (label logit -60, all others 0: q = 1,
the modulating factor is ~1).  Every stored gradient element, loss_out and both statistics must be finite.

Tolerances are the project's for this kernel (test_class_weights_gpu.py): loss rtol 1e-4 / atol 1e-4, #correct
exact (over kept rows), gradient rtol 2e-2 / atol 1e-4, pad columns and ignored rows exactly 0, bias sums within
1e-6 * sum |d| of the float64 column sums of the stored bf16 gradient.
"""
import pytest
import torch

import ldnn
from ldnn.ops import _ext
from ldnn.ops import functional as LF
from test_focal_loss import focal_oracle

pytestmark = pytest.mark.gpu

# (B, C, ld): rows kernel with a partial last workgroup / fewer rows than a wave / the LD = 64 instance /
# wave kernel with 4 rows per block / wave kernel with 16 rows per block and a padded stride
SHAPES = [(300, 10, 16), (5, 3, 8), (257, 64, 64), (64, 1000, 1000), (1100, 65, 72)]


def C():
    return _ext.C()


def _gen(seed):
    return torch.Generator(device="cuda").manual_seed(seed)


def _logits(B, Cc, ld, seed=41):
    """bf16 [B, C] view of a [B, ld] buffer with the two planted rows (label 0)."""
    buf = (torch.randn(B, ld, device="cuda", generator=_gen(seed)) * 3).bfloat16()
    buf[0, :Cc] = -60.0
    buf[0, 0] = 60.0
    buf[1, :Cc] = 0.0
    buf[1, 0] = -60.0
    return buf[:, :Cc]


def _weights(Cc, seed=42):
    """fp32 [C] in [0, 3] with one exact 0 (as test_class_weights_gpu._weights); class 0 has weight > 0."""
    w = torch.rand(Cc, device="cuda", generator=_gen(seed)) * 3
    w[1] = 0.0
    w[0] = w[0].clamp_min(0.5)
    return w


def _labels(B, Cc, ignore_index, seed=43):
    """Labels with about a fifth of the rows ignored, the last row among them; rows 0 and 1 (planted) are
    kept rows of class 0."""
    y = torch.randint(0, Cc, (B,), device="cuda", generator=_gen(seed))
    ign = torch.rand(B, device="cuda", generator=_gen(seed + 1)) < 0.2
    ign[-1] = True
    y[ign] = ignore_index
    y[0] = y[1] = 0
    return y, y == ignore_index   # (rows that drew the class itself are ignored too, as in torch)


def _kernel(logits, y, ld, w, ignore_index=-100, gamma=2.0, **kw):
    B, Cc = logits.shape
    dl = torch.full((B, ld), 7.0, device="cuda", dtype=torch.bfloat16)
    stats = torch.zeros(2, device="cuda")
    db = torch.zeros(ld, device="cuda")
    C().softmax_xent_focal(logits, y, dl[:, :Cc], stats, dbias=db, num_classes=Cc, gamma=gamma, weight=w,
                           ignore_index=ignore_index, **kw)
    return dl, stats, db


def _check(dl, stats, db, ref, B, Cc, ignored=None):
    loss, grad, correct = ref
    grad = grad.float()
    print(f"loss {stats[0].item() / B:.6f} ref {loss.item():.6f}  correct {stats[1].item():.0f} ref {correct}  "
          f"max |dgrad| {(dl[:, :Cc].float() - grad).abs().max().item():.3e} of max |grad| {grad.abs().max().item():.3e}")
    for t in (dl.float(), stats, db):
        assert bool(torch.isfinite(t).all())
    torch.testing.assert_close(stats[0] / B, loss.float(), rtol=1e-4, atol=1e-4)
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
@pytest.mark.parametrize("weighted", [True, False], ids=["w", "w=None"])
@pytest.mark.parametrize("gamma", [0.5, 2.0])
@pytest.mark.parametrize("B,Cc,ld", SHAPES)
def test_focal_kernel_matches_the_oracle(B, Cc, ld, gamma, weighted, ignore_index):
    logits = _logits(B, Cc, ld)
    w = _weights(Cc) if weighted else None
    y, ign = _labels(B, Cc, ignore_index)
    out = torch.full((2,), -5.0, device="cuda")
    dl, stats, db = _kernel(logits, y, ld, w, ignore_index, gamma, loss_out=out)
    assert bool(torch.isfinite(out).all())
    ref = focal_oracle(logits, y, w, ignore_index, gamma)
    _check(dl, stats, db, ref, B, Cc, ign)
    torch.testing.assert_close(out[0], ref[0].float(), rtol=1e-4, atol=1e-4)
    assert dl[0].float().abs().max().item() == 0.0   # the saturated row: a zero gradient row
    # row 1: q = 1, the factor is ~1: the label's element is -a / den to bf16 rounding
    den = C().xent_wden_ws(logits)
    a = 1.0 if w is None else w[0].item()
    assert dl[1, 0].item() == pytest.approx(-a / den[0].item(), rel=2 ** -7)
    assert den[2].item() == int((~ign).sum())


@pytest.mark.parametrize("B,Cc,ld", SHAPES)
def test_gamma_zero_is_the_weighted_op(B, Cc, ld):
    logits, w = _logits(B, Cc, ld, seed=50), _weights(Cc, seed=51)
    y, _ = _labels(B, Cc, 2, seed=52)
    a = _kernel(logits, y, ld, w, 2, 0.0)
    dl = torch.full((B, ld), 7.0, device="cuda", dtype=torch.bfloat16)
    stats, db = torch.zeros(2, device="cuda"), torch.zeros(ld, device="cuda")
    C().softmax_xent_w(logits, y, dl[:, :Cc], stats, dbias=db, num_classes=Cc, weight=w, ignore_index=2)
    assert torch.equal(a[0].view(torch.int16), dl.view(torch.int16))   # the same launch: bit for bit
    # (the statistics and bias sums are fp32 atomics over the blocks: the order may differ)
    torch.testing.assert_close(a[1][0] / B, stats[0] / B, rtol=1e-4, atol=1e-4)
    assert a[1][1].item() == stats[1].item()
    # each bias sum lies within 1e-6 * sum |d| of the exact column sum (_check), so two lie within twice that
    assert bool(((a[2] - db).abs().double() <= 2e-6 * dl.double().abs().sum(0)).all())


@pytest.mark.parametrize("B,Cc,ld", SHAPES)
def test_out_of_range_labels_are_ignored(B, Cc, ld):
    """A label that is no class and not ignore_index: no error, treated as ignored, nothing outside
    the weights or the gradient rows is touched (canary words round both)."""
    logits = _logits(B, Cc, ld, seed=53)
    y, ign = _labels(B, Cc, -100, seed=54)
    bad = torch.zeros(B, dtype=torch.bool, device="cuda")
    bad[B // 2] = bad[min(3, B - 2)] = True
    y[B // 2], y[min(3, B - 2)] = Cc, -7
    wbuf = torch.full((Cc + 64,), 1e30, device="cuda")
    wbuf[32: 32 + Cc] = _weights(Cc)
    w = wbuf[32: 32 + Cc]
    dbuf = torch.full((B + 2, ld), 7.0, device="cuda", dtype=torch.bfloat16)
    dl = dbuf[1:-1]
    stats, db = torch.zeros(2, device="cuda"), torch.zeros(ld, device="cuda")
    C().softmax_xent_focal(logits, y, dl[:, :Cc], stats, dbias=db, num_classes=Cc, gamma=0.5, weight=w)
    torch.cuda.synchronize()
    assert bool((wbuf[:32] == 1e30).all()) and bool((wbuf[32 + Cc:] == 1e30).all())
    assert bool((dbuf[0].float() == 7.0).all()) and bool((dbuf[-1].float() == 7.0).all())
    yt = torch.where(bad, torch.full_like(y, -100), y)
    _check(dl, stats, db, focal_oracle(logits, yt, w, -100, 0.5), B, Cc, ign | bad)


@pytest.mark.parametrize("B,Cc,ld", SHAPES)
def test_two_launches_are_bit_identical(B, Cc, ld):
    logits, w = _logits(B, Cc, ld, seed=55), _weights(Cc, seed=56)
    y, _ = _labels(B, Cc, 2, seed=57)
    dl1, _, _ = _kernel(logits, y, ld, w, 2, 0.5)
    den1 = C().xent_wden_ws(logits).clone()
    dl2, _, _ = _kernel(logits, y, ld, w, 2, 0.5)
    den2 = C().xent_wden_ws(logits).clone()
    assert torch.equal(dl1.view(torch.int16), dl2.view(torch.int16))
    assert torch.equal(den1.view(torch.int32), den2.view(torch.int32))
    assert den1[0].item() > 0 and den1[1].item() == pytest.approx(1.0 / den1[0].item(), rel=1e-6)


@pytest.mark.parametrize("B,Cc,ld", SHAPES)
def test_all_ignored_batch_gives_zeros(B, Cc, ld):
    logits, w = _logits(B, Cc, ld, seed=58), _weights(Cc, seed=59)
    out = torch.full((2,), -5.0, device="cuda")
    for y in (torch.full((B,), 2, device="cuda"), torch.full((B,), 1, device="cuda")):   # all ignored / all weight 0
        dl, stats, db = _kernel(logits, y, ld, w, 2, 2.0, loss_out=out)
        assert out.tolist()[0] == 0.0 and stats[0].item() == 0.0
        assert dl.float().abs().max().item() == 0.0 and db.abs().max().item() == 0.0
        assert C().xent_wden_ws(logits)[:2].tolist() == [0.0, 0.0]
    assert out[1].item() == int((logits.float().argmax(1) == 1).sum())   # weight 0 rows are kept rows


@pytest.mark.parametrize("B,Cc,ld", [(300, 10, 16), (64, 1000, 1000)])
def test_focal_finalize(B, Cc, ld):
    """loss_out: the last block writes [focal loss, #correct], adds [B * loss, #correct] into stats once and
    leaves its accumulator zero for the next call."""
    logits, w = _logits(B, Cc, ld, seed=60), _weights(Cc, seed=61)
    y, _ = _labels(B, Cc, 2, seed=62)
    ref, _, correct = focal_oracle(logits, y, w, 2, 2.0)
    ref = ref.float()
    dl = torch.empty(B, ld, device="cuda", dtype=torch.bfloat16)
    stats = torch.tensor([1.0, 2.0], device="cuda")
    for _ in range(2):
        out = torch.full((2,), -5.0, device="cuda")
        C().softmax_xent_focal(logits, y, dl[:, :Cc], stats, None, Cc, gamma=2.0, weight=w, ignore_index=2,
                               loss_out=out)
        torch.testing.assert_close(out[0], ref, rtol=1e-4, atol=1e-4)   # (a dirty accumulator would double it)
        assert out[1].item() == correct
    torch.testing.assert_close(stats, torch.tensor([1.0 + 2 * ref.item() * B, 2.0 + 2 * correct], device="cuda"),
                               rtol=1e-4, atol=1e-3)


def test_binding_refusals():
    B, Cc, ld = 64, 10, 16
    logits = _logits(B, Cc, ld)
    y = torch.randint(0, Cc, (B,), device="cuda")
    w = _weights(Cc)
    for bad in (-1.0, float("nan"), float("inf"), 1e39):   # (1e39: not finite as the fp32 the kernel takes)
        with pytest.raises(RuntimeError, match="gamma"):
            _kernel(logits, y, ld, w, gamma=bad)
    with pytest.raises(RuntimeError, match="weight"):
        _kernel(logits, y, ld, w.double())
    with pytest.raises(RuntimeError, match="weight"):
        _kernel(logits, y, ld, torch.ones(Cc + 1, device="cuda"))
    with pytest.raises(RuntimeError, match="weight"):
        _kernel(logits, y, ld, w.cpu())
    with pytest.raises(RuntimeError, match="weight"):
        _kernel(logits, y, ld, torch.ones(2 * Cc, device="cuda")[::2])
    with pytest.raises(RuntimeError, match="labels"):   # xent_launch's own checks still apply
        _kernel(logits, y[:-1], ld, w)
    with pytest.raises(ValueError, match="label_smoothing"):   # and the Python entry's, on the GPU path too
        LF.cross_entropy(logits, y, None, 0.1, focal_gamma=2.0)
    with pytest.raises(ValueError, match="target"):
        LF.cross_entropy(logits, torch.softmax(logits.float(), 1), focal_gamma=2.0)


def test_autograd_path():
    from ldnn.models import FocalLoss

    B = 96
    buf = _logits(B, 10, 16, seed=63)
    w = _weights(10, seed=64)
    y, _ = _labels(B, 10, 2, seed=65)
    crit = FocalLoss(0.5, weight=w.cpu(), ignore_index=2)   # (the buffer follows the logits)
    logits = buf.detach().requires_grad_(True)
    stats = torch.zeros(2, device="cuda")
    loss = crit(logits, y, stats)
    (B * loss).backward()
    ref, grad, correct = focal_oracle(buf, y, w, 2, 0.5)
    assert bool(torch.isfinite(logits.grad.float()).all())
    torch.testing.assert_close(loss.detach(), ref.float(), rtol=1e-4, atol=1e-4)
    # (B * loss: the kernel's bf16 gradient is scaled by B in a second rounding, hence twice the atol)
    torch.testing.assert_close(logits.grad.float(), (B * grad).float(), rtol=2e-2, atol=2e-4)
    torch.testing.assert_close(stats, torch.tensor([ref.item() * B, float(correct)], device="cuda"),
                               rtol=1e-4, atol=1e-3)
    assert crit.weight.is_cuda
    # gamma = 0 takes the weighted launch: bit for bit the loss of the call without the keyword
    assert torch.equal(LF.cross_entropy(buf, y, None, 0.0, w, 2, focal_gamma=0.0),
                       LF.cross_entropy(buf, y, None, 0.0, w, 2))


def test_graphed_step_bakes_gamma_in():
    from ldnn.models import FocalLoss, xavier_init
    from ldnn.models.mlp import MLP
    from ldnn.optim import SGD
    from ldnn.train.graphed import GraphedStep

    torch.manual_seed(67)
    m = MLP(70, (33,), 10)
    xavier_init(m)
    ldnn.prepare(m, "cuda")
    opt = SGD(m.parameters(), lr=0.0, momentum=0.9)
    w1, w2 = _weights(10, seed=68), _weights(10, seed=69)
    crit = FocalLoss(2.0, weight=w1, ignore_index=2)
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
    refs = [focal_oracle(out, y, w, 2, 2.0)[0].item() for w in (w1, w2)]
    tols = [1e-4 + 1e-4 * abs(r) for r in refs]
    print(f"replayed {[got1, got2]}  ref {refs}")
    assert abs(got1 - refs[0]) <= tols[0] and abs(got2 - refs[1]) <= tols[1]
    assert abs(got1 - got2) > 10 * max(tols)
    # ... and equals an eager step with the new weights: the same kernels on the same inputs (one loss
    # workgroup: the same bits; the weight gradients may differ by the order of fp32 atomic sums)
    opt.zero_grad()
    loss = FocalLoss(2.0, weight=w2, ignore_index=2)(m(x), y)
    loss.backward()
    assert loss.item() == got2
    for a, p in zip(g2, m.parameters()):
        torch.testing.assert_close(a, p.grad, rtol=1e-4, atol=1e-6)
    # what the capture baked in must not change behind it
    crit.gamma = 0.5
    with pytest.raises(RuntimeError, match="gamma"):
        gs(x, y)
    crit.gamma = 2.0
    assert gs(x, y).item() == got2
    torch.cuda.synchronize()
