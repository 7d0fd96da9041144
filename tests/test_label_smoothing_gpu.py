"""Label smoothing inside the fused softmax cross-entropy kernels (xent.hip SMOOTH instances)
against ``F.cross_entropy(logits.float(), labels, label_smoothing=eps)`` on the same bf16 logits
and its autograd gradient.

The direct kernel calls use grad_scale = 1 (not 1/B): with 1/B the smoothing term eps / (C * B) of
the gradient falls below the gradient atol and smoothing could not be told from none.  Tolerances
are those of test_kernels_gpu.py::test_softmax_xent_matches_torch: mean loss rtol 1e-4 / atol 1e-4,
#correct exact, gradient rtol 2e-2 (bf16 rounds at 2^-9 relative) / atol 1e-4, pad columns exactly 0.
"""
import pytest
import torch
import torch.nn.functional as F

import ldnn
from ldnn.ops import _ext
from ldnn.ops import functional as LF

pytestmark = pytest.mark.gpu

# (B, C, ld): the smallest shapes that reach every branch of the two kernels
ROWS = [(64, 10, 16),       # one block, padded columns
        (300, 10, 16),      # two blocks, ragged last block
        (70, 3, 8),         # LD = 8
        (65, 64, 64)]       # default case, no padding
WAVE = [(257, 10, 10),      # ld % 8 != 0: the unaligned fallback
        (66, 65, 72),       # two column tiles, the second partial
        (64, 1000, 1000),   # 16 tiles, 4 rows per block
        (1100, 100, 104)]   # B > 1024: 16 rows per block, ragged last block


def C():
    return _ext.C()


def _inputs(B, Cc, ld, seed=11):
    g = torch.Generator(device="cuda").manual_seed(seed)
    full = (torch.randn(B, ld, device="cuda", generator=g) * 3).bfloat16()
    labels = torch.randint(0, Cc, (B,), device="cuda", generator=g)
    return full[:, :Cc], labels


def _oracle(logits, labels, eps):
    """(mean loss, d(B * mean loss)/d logits, #correct) in fp32 from torch."""
    lf = logits.float().requires_grad_(True)
    loss = F.cross_entropy(lf, labels, label_smoothing=eps)
    (loss * logits.shape[0]).backward()
    return loss.detach(), lf.grad, (lf.detach().argmax(1) == labels).sum().item()


def _kernel(logits, labels, ld, **kw):
    B, Cc = logits.shape
    dl = torch.full((B, ld), 7.0, device="cuda", dtype=torch.bfloat16)
    stats = torch.zeros(2, device="cuda")
    db = torch.zeros(ld, device="cuda")
    C().softmax_xent(logits, labels, dl[:, :Cc], stats, dbias=db, num_classes=Cc, grad_scale=1.0, **kw)
    return dl, stats, db


@pytest.mark.parametrize("eps", [0.1, 1.0])
@pytest.mark.parametrize("B,Cc,ld", ROWS + WAVE)
def test_smoothed_kernel_matches_torch(B, Cc, ld, eps):
    logits, labels = _inputs(B, Cc, ld)
    dl, stats, db = _kernel(logits, labels, ld, label_smoothing=eps)
    loss, grad, correct = _oracle(logits, labels, eps)
    print(f"loss {stats[0].item() / B:.6f} ref {loss.item():.6f}  max |dgrad| "
          f"{(dl[:, :Cc].float() - grad).abs().max().item():.3e}")
    torch.testing.assert_close(stats[0] / B, loss, rtol=1e-4, atol=1e-4)
    assert stats[1].item() == correct
    torch.testing.assert_close(dl[:, :Cc].float(), grad, rtol=2e-2, atol=1e-4)
    if ld > Cc:
        assert dl[:, Cc:].float().abs().max().item() == 0.0
    # dbias = column sums of the kernel's own bf16 gradient: fp32 accumulation in any order errs by
    # about 2^-24 per term of sum |dlogits|; 1e-6 leaves a factor of about 16
    d64 = dl.double()
    err = (db.double() - d64.sum(0)).abs()
    bound = 1e-6 * d64.abs().sum(0)
    assert bool((err <= bound).all()), (err.max().item(), bound.min().item())


@pytest.mark.parametrize("B,Cc,ld", [(300, 10, 16), (64, 1000, 1000)])
def test_smoothed_finalize(B, Cc, ld):
    """loss_out with smoothing: the last block writes [smoothed mean loss, #correct], adds the sums
    into stats once, and leaves its workspace zero for the next call."""
    eps = 0.1
    logits, labels = _inputs(B, Cc, ld, seed=12)
    ref, _, correct = _oracle(logits, labels, eps)
    dl = torch.empty(B, ld, device="cuda", dtype=torch.bfloat16)
    stats = torch.tensor([1.0, 2.0], device="cuda")
    for rep in range(2):
        out = torch.full((2,), -5.0, device="cuda")
        C().softmax_xent(logits, labels, dl[:, :Cc], stats if rep == 0 else None, None, Cc, 1.0 / B,
                         loss_out=out, loss_scale=1.0 / B, label_smoothing=eps)
        torch.testing.assert_close(out[0], ref, rtol=1e-4, atol=1e-4)
        assert out[1].item() == correct
    torch.testing.assert_close(stats, torch.tensor([1.0 + ref.item() * B, 2.0 + correct], device="cuda"),
                               rtol=1e-4, atol=1e-3)


@pytest.mark.parametrize("B,Cc,ld", [(64, 10, 16), (64, 1000, 1000)])
def test_zero_smoothing_is_the_argument_omitted(B, Cc, ld):
    logits, labels = _inputs(B, Cc, ld, seed=13)
    dl0, st0, db0 = _kernel(logits, labels, ld)
    dl1, st1, db1 = _kernel(logits, labels, ld, label_smoothing=0.0)
    assert torch.equal(dl0.view(torch.int16), dl1.view(torch.int16))
    assert st0[1].item() == st1[1].item()
    if ld <= 64:                # the rows kernel, B <= 256: one block and therefore one atomic order
        assert torch.equal(st0, st1) and torch.equal(db0, db1)
    else:                       # several blocks add atomically
        torch.testing.assert_close(st0[0] / B, st1[0] / B, rtol=1e-4, atol=1e-4)


@pytest.mark.parametrize("eps", [-0.1, 1.5])
def test_binding_rejects_out_of_range(eps):
    logits, labels = _inputs(64, 10, 16)
    with pytest.raises(RuntimeError, match="label_smoothing"):
        _kernel(logits, labels, 16, label_smoothing=eps)


def test_autograd_path():
    """LF.cross_entropy(label_smoothing=) on padded bf16 logits; the multiplier B makes the effective
    gradient scale 1.  Tolerance of test_kernels_gpu.py::test_scale_bf16_and_loss_backward."""
    B = 96
    g = torch.Generator(device="cuda").manual_seed(14)
    buf = (torch.randn(B, 16, device="cuda", generator=g) * 3).bfloat16()
    labels = torch.randint(0, 10, (B,), device="cuda", generator=g)
    logits = buf[:, :10].requires_grad_(True)
    stats = torch.zeros(2, device="cuda")
    loss = LF.cross_entropy(logits, labels, stats, label_smoothing=0.1)
    (B * loss).backward()
    ref, grad, correct = _oracle(buf[:, :10], labels, 0.1)
    plain = F.cross_entropy(buf[:, :10].float(), labels)
    torch.testing.assert_close(loss.detach(), ref, rtol=1e-4, atol=1e-4)
    assert abs(ref.item() - plain.item()) > 1e-3
    torch.testing.assert_close(logits.grad.float(), grad, rtol=2e-2, atol=2e-4)
    torch.testing.assert_close(stats, torch.tensor([ref.item() * B, float(correct)], device="cuda"),
                               rtol=1e-4, atol=1e-3)
    with pytest.raises(ValueError):
        LF.cross_entropy(logits, labels, label_smoothing=1.5)


def test_graphed_step_bakes_the_smoothing_in():
    from ldnn.models import CrossEntropyLoss, xavier_init
    from ldnn.models.mlp import MLP
    from ldnn.optim import SGD
    from ldnn.train.graphed import GraphedStep

    torch.manual_seed(15)
    m = MLP(70, (33,), 10)
    xavier_init(m)
    ldnn.prepare(m, "cuda")
    opt = SGD(m.parameters(), lr=0.01, momentum=0.9)
    crit = CrossEntropyLoss(label_smoothing=0.1)
    x = (torch.randn(96, 70, device="cuda") * 4).bfloat16()
    y = torch.randint(0, 10, (96,), device="cuda")
    gs = GraphedStep(m, crit, opt, x, y)
    with torch.no_grad():
        out = m(x).float()   # the logits the next step's forward sees
    loss = gs(x, y).item()
    ref = F.cross_entropy(out, y, label_smoothing=0.1).item()
    plain = F.cross_entropy(out, y).item()
    tol = 1e-4 + 1e-4 * abs(ref)
    print(f"replayed loss {loss:.6f}  smoothed ref {ref:.6f}  unsmoothed {plain:.6f}")
    assert abs(loss - ref) <= tol
    assert abs(loss - plain) > 10 * tol
    crit.label_smoothing = 0.2
    with pytest.raises(RuntimeError, match="capture again"):
        gs(x, y)
    crit.label_smoothing = 0.1
    gs(x, y)
    torch.cuda.synchronize()
