"""Class-probability targets in the fused softmax cross-entropy (xent.hip soft-target instances)
against ``F.cross_entropy(logits.float(), q, label_smoothing=eps)`` on the same bf16 logits and its
autograd gradient.

Direct kernel calls use grad_scale = 1, like test_label_smoothing_gpu.py.  Tolerances are the
project's (test_kernels_gpu.py::test_softmax_xent_matches_torch, test_label_smoothing_gpu.py): mean
loss rtol 1e-4 / atol 1e-4, #correct exact, gradient rtol 2e-2 / atol 1e-4, pad columns exactly 0,
bias sums within 1e-6 * sum |d| of the float64 column sums of the stored bf16 gradient.
"""
import pytest
import torch
import torch.nn.functional as F

import ldnn
from ldnn.ops import _ext
from ldnn.ops import functional as LF

pytestmark = pytest.mark.gpu

# (B, C, ld): the shapes test_label_smoothing_gpu.py uses to reach every branch of the two kernels
SHAPES = [(64, 10, 16), (300, 10, 16), (70, 3, 8), (65, 64, 64),          # one row per lane
          (257, 10, 10), (66, 65, 72), (64, 1000, 1000), (1100, 100, 104)]  # one wave per row
KINDS = ["normalised", "unnormalised", "twohot"]


def C():
    return _ext.C()


def _up4(n):
    return (n + 3) // 4 * 4


def _logits(B, Cc, ld, seed=21):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return (torch.randn(B, ld, device="cuda", generator=g) * 3).bfloat16()[:, :Cc]


def _targets(kind, B, Cc, seed=22):
    """Dense [B, C] fp32 targets whose top two entries never tie (the oracle's argmax is then
    unambiguous): random rows get 0.25 added to one entry, two-hot rows never use lam = 0.5."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    if kind == "twohot":
        a = torch.randint(0, Cc, (B,), device="cuda", generator=g)
        b = torch.randint(0, Cc, (B,), device="cuda", generator=g)
        b[::5] = a[::5]                                    # some a == b
        lam = torch.tensor([0.3, 0.8, 1.0], device="cuda")[torch.arange(B, device="cuda") % 3]
        q = torch.zeros(B, Cc, device="cuda")
        rows = torch.arange(B, device="cuda")
        q[rows, a] += lam
        q[rows, b] += 1.0 - lam
        return q
    q = torch.rand(B, Cc, device="cuda", generator=g)
    top = torch.randint(0, Cc, (B,), device="cuda", generator=g)
    q[torch.arange(B, device="cuda"), top] = 1.25
    q = q / q.sum(1, keepdim=True)
    if kind == "unnormalised":
        q = q * (0.3 + 1.4 * torch.rand(B, 1, device="cuda", generator=g))   # row sums in [0.3, 1.7]
    return q


def _strided(q, ldq):
    """q as the [:, :C] view of a [B, ldq] buffer (the pad holds junk the kernel must not read)."""
    buf = torch.full((q.shape[0], ldq), 9.0, device=q.device)
    buf[:, : q.shape[1]] = q
    return buf[:, : q.shape[1]]


def _oracle(logits, q, eps):
    """(mean loss, d(B * mean loss)/d logits, #correct) in fp32 from torch."""
    lf = logits.float().requires_grad_(True)
    loss = F.cross_entropy(lf, q, label_smoothing=eps)
    (loss * logits.shape[0]).backward()
    return loss.detach(), lf.grad, (lf.detach().argmax(1) == q.argmax(1)).sum().item()


def _kernel(logits, q, ld, **kw):
    B, Cc = logits.shape
    dl = torch.full((B, ld), 7.0, device="cuda", dtype=torch.bfloat16)
    stats = torch.zeros(2, device="cuda")
    db = torch.zeros(ld, device="cuda")
    C().softmax_xent_soft(logits, q, dl[:, :Cc], stats, dbias=db, num_classes=Cc, grad_scale=1.0, **kw)
    return dl, stats, db


def _check(dl, stats, db, logits, q, eps):
    B, Cc = logits.shape
    loss, grad, correct = _oracle(logits, q, eps)
    print(f"loss {stats[0].item() / B:.6f} ref {loss.item():.6f}  correct {stats[1].item():.0f} ref {correct}  "
          f"max |dgrad| {(dl[:, :Cc].float() - grad).abs().max().item():.3e}")
    torch.testing.assert_close(stats[0] / B, loss, rtol=1e-4, atol=1e-4)
    assert stats[1].item() == correct
    torch.testing.assert_close(dl[:, :Cc].float(), grad, rtol=2e-2, atol=1e-4)
    if dl.shape[1] > Cc:
        assert dl[:, Cc:].float().abs().max().item() == 0.0
    d64 = dl.double()
    err = (db.double() - d64.sum(0)).abs()
    bound = 1e-6 * d64.abs().sum(0)
    assert bool((err <= bound).all()), (err.max().item(), bound.min().item())


@pytest.mark.parametrize("pad_q", [False, True], ids=["ldq=C", "ldq=up4(C)"])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("eps", [0.0, 0.1])
@pytest.mark.parametrize("B,Cc,ld", SHAPES)
def test_soft_kernel_matches_torch(B, Cc, ld, eps, kind, pad_q):
    logits = _logits(B, Cc, ld)
    q = _targets(kind, B, Cc)
    qk = _strided(q, _up4(Cc)) if pad_q else q.contiguous()
    dl, stats, db = _kernel(logits, qk, ld, label_smoothing=eps)
    _check(dl, stats, db, logits, q, eps)


@pytest.mark.parametrize("eps", [0.0, 0.1])
@pytest.mark.parametrize("B,Cc,ld", SHAPES)
def test_onehot_soft_targets_reproduce_hard_labels(B, Cc, ld, eps):
    logits = _logits(B, Cc, ld, seed=23)
    labels = torch.randint(0, Cc, (B,), device="cuda", generator=torch.Generator(device="cuda").manual_seed(24))
    q = F.one_hot(labels, Cc).float()
    dl, stats, _ = _kernel(logits, q, ld, label_smoothing=eps)
    dh = torch.full((B, ld), 7.0, device="cuda", dtype=torch.bfloat16)
    sh = torch.zeros(2, device="cuda")
    C().softmax_xent(logits, labels, dh[:, :Cc], sh, dbias=None, num_classes=Cc, grad_scale=1.0,
                     label_smoothing=eps)
    torch.testing.assert_close(stats[0] / B, sh[0] / B, rtol=1e-4, atol=1e-4)
    assert stats[1].item() == sh[1].item()
    torch.testing.assert_close(dl.float(), dh.float(), rtol=2e-2, atol=1e-4)


@pytest.mark.parametrize("B,Cc,ld", [(300, 10, 16), (64, 1000, 1000)])
def test_soft_finalize(B, Cc, ld):
    """loss_out: the last block writes [mean loss, #correct], adds the sums into stats once and
    leaves its accumulator zero for the next call."""
    eps = 0.1
    logits = _logits(B, Cc, ld, seed=25)
    q = _targets("unnormalised", B, Cc, seed=26)
    ref, _, correct = _oracle(logits, q, eps)
    dl = torch.empty(B, ld, device="cuda", dtype=torch.bfloat16)
    stats = torch.tensor([1.0, 2.0], device="cuda")
    for _ in range(2):
        out = torch.full((2,), -5.0, device="cuda")
        C().softmax_xent_soft(logits, q, dl[:, :Cc], stats, None, Cc, 1.0 / B, loss_out=out, loss_scale=1.0 / B,
                              label_smoothing=eps)
        torch.testing.assert_close(out[0], ref, rtol=1e-4, atol=1e-4)   # (a dirty accumulator would double it)
        assert out[1].item() == correct
    torch.testing.assert_close(stats, torch.tensor([1.0 + 2 * ref.item() * B, 2.0 + 2 * correct], device="cuda"),
                               rtol=1e-4, atol=1e-3)


def test_binding_refusals():
    B, Cc, ld = 64, 10, 16
    logits = _logits(B, Cc, ld)
    q = _targets("normalised", B, Cc)
    with pytest.raises(RuntimeError, match="target"):
        _kernel(logits, torch.zeros(B, Cc, dtype=torch.int64, device="cuda"), ld)
    with pytest.raises(RuntimeError, match="target"):
        _kernel(logits, torch.zeros(B, Cc + 1, device="cuda"), ld)
    with pytest.raises(RuntimeError, match="target"):
        _kernel(logits, torch.zeros(Cc, B, device="cuda").t(), ld)
    with pytest.raises(RuntimeError, match="target"):
        _kernel(logits, q.cpu(), ld)
    for eps in (-0.1, 1.5):
        with pytest.raises(RuntimeError, match="label_smoothing"):
            _kernel(logits, q, ld, label_smoothing=eps)


def test_autograd_path():
    from ldnn.models import CrossEntropyLoss

    B = 96
    buf = _logits(B, 16, 16, seed=27)
    q = _targets("twohot", B, 10, seed=28)
    for eps, call in ((0.0, lambda lg, st: LF.cross_entropy(lg, q, st)),
                      (0.1, lambda lg, st: CrossEntropyLoss(label_smoothing=0.1)(lg, q, st))):
        logits = buf[:, :10].detach().requires_grad_(True)
        stats = torch.zeros(2, device="cuda")
        loss = call(logits, stats)
        (B * loss).backward()
        ref, grad, correct = _oracle(buf[:, :10], q, eps)
        torch.testing.assert_close(loss.detach(), ref, rtol=1e-4, atol=1e-4)
        torch.testing.assert_close(logits.grad.float(), grad, rtol=2e-2, atol=2e-4)
        torch.testing.assert_close(stats, torch.tensor([ref.item() * B, float(correct)], device="cuda"),
                                   rtol=1e-4, atol=1e-3)
    logits = buf[:, :10].detach().requires_grad_(True)
    ref, _, _ = _oracle(buf[:, :10], q.bfloat16().float(), 0.0)
    torch.testing.assert_close(LF.cross_entropy(logits, q.bfloat16()).detach(), ref, rtol=1e-4, atol=1e-4)
    with pytest.raises(ValueError, match="gradient"):
        LF.cross_entropy(logits, q.clone().requires_grad_(True))
    with pytest.raises(ValueError, match="96, 10"):
        LF.cross_entropy(logits, q[:, None, :])


def test_graphed_step_stages_the_targets():
    from ldnn.models import CrossEntropyLoss, xavier_init
    from ldnn.models.mlp import MLP
    from ldnn.optim import SGD
    from ldnn.train.graphed import GraphedStep

    torch.manual_seed(29)
    m = MLP(70, (33,), 10)
    xavier_init(m)
    ldnn.prepare(m, "cuda")
    opt = SGD(m.parameters(), lr=0.0, momentum=0.9)
    crit = CrossEntropyLoss()
    B = 64
    x = (torch.randn(B, 70, device="cuda") * 4).bfloat16()
    q1, q2 = _targets("twohot", B, 10, seed=30), _targets("normalised", B, 10, seed=31)
    gs = GraphedStep(m, crit, opt, x, q1)
    with torch.no_grad():
        out = m(x).float()   # lr = 0: the logits of every step
    got = [gs(x, q).item() for q in (q1, q2)]
    refs = [F.cross_entropy(out, q).item() for q in (q1, q2)]
    tols = [1e-4 + 1e-4 * abs(r) for r in refs]
    print(f"replayed {got}  ref {refs}")
    for g, r, t in zip(got, refs, tols):
        assert abs(g - r) <= t
    assert abs(got[0] - got[1]) > 10 * max(tols)
    # hard labels given to the step captured with [B, C] targets: the eager step, the hard-label loss
    y = torch.randint(0, 10, (B,), device="cuda")
    hard = gs(x, y).item()
    ref = F.cross_entropy(out, y).item()
    assert abs(hard - ref) <= 1e-4 + 1e-4 * abs(ref)
    # ... and a same-shape target of another dtype is not converted into the static buffer either
    assert abs(gs(x, q2.double()).item() - refs[1]) <= tols[1]
    torch.cuda.synchronize()
