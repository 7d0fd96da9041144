"""Class-probability targets through the public loss interface on the CPU path."""
import pytest
import torch
import torch.nn.functional as F

from ldnn.models import CrossEntropyLoss
from ldnn.ops import functional as LF


def _case(B=24, C=7, seed=0):
    g = torch.Generator().manual_seed(seed)
    logits = torch.randn(B, C, generator=g) * 3
    q = torch.rand(B, C, generator=g)
    q[torch.arange(B), torch.randint(0, C, (B,), generator=g)] = 1.25   # an unambiguous top entry
    return logits, q


@pytest.mark.parametrize("eps", [0.0, 0.1])
@pytest.mark.parametrize("normalise", [True, False])
def test_cpu_cross_entropy_matches_torch(eps, normalise):
    logits, q = _case()
    if normalise:
        q = q / q.sum(1, keepdim=True)
    lg = logits.clone().requires_grad_(True)
    stats = torch.zeros(2)
    loss = LF.cross_entropy(lg, q, stats, label_smoothing=eps)
    loss.backward()
    lr = logits.clone().requires_grad_(True)
    ref = F.cross_entropy(lr, q, label_smoothing=eps)
    ref.backward()
    torch.testing.assert_close(loss, ref)
    torch.testing.assert_close(lg.grad, lr.grad)
    # the argmax rule: agreement of the logits' argmax with the target row's
    correct = (logits.argmax(1) == q.argmax(1)).sum().item()
    torch.testing.assert_close(stats, torch.tensor([ref.item() * 24, float(correct)]))
    # the module dispatches likewise
    st2 = torch.zeros(2)
    torch.testing.assert_close(CrossEntropyLoss(label_smoothing=eps)(logits, q, st2), ref.detach())
    torch.testing.assert_close(st2, stats)


def test_onehot_targets_are_the_hard_labels():
    logits, _ = _case(seed=1)
    labels = torch.randint(0, 7, (24,), generator=torch.Generator().manual_seed(2))
    s_hard, s_soft = torch.zeros(2), torch.zeros(2)
    hard = LF.cross_entropy(logits, labels, s_hard, 0.1)
    soft = LF.cross_entropy(logits, F.one_hot(labels, 7).float(), s_soft, 0.1)
    torch.testing.assert_close(soft, hard)
    torch.testing.assert_close(s_soft, s_hard)
    # bf16 / fp16 targets are widened
    torch.testing.assert_close(LF.cross_entropy(logits, F.one_hot(labels, 7).bfloat16(), None, 0.1), hard)
    torch.testing.assert_close(LF.cross_entropy(logits, F.one_hot(labels, 7).half(), None, 0.1), hard)


def test_target_refusals_name_the_shapes():
    logits, q = _case()
    with pytest.raises(ValueError, match="gradient"):
        LF.cross_entropy(logits, q.clone().requires_grad_(True))
    for bad in (q[:, None, :], q[:, :6], q[:23], torch.zeros(24, 7, dtype=torch.long), q.double()[:, :, None]):
        with pytest.raises(ValueError, match=r"\(24, 7\).*" + str(tuple(bad.shape)).replace("(", r"\(").replace(")", r"\)")):
            LF.cross_entropy(logits, bad)


def test_module_still_refuses_what_it_does_not_implement():
    with pytest.raises(NotImplementedError, match="weights"):
        CrossEntropyLoss(weight=torch.ones(7))
    with pytest.raises(NotImplementedError, match="ignore_index"):
        CrossEntropyLoss(ignore_index=3)
    for red in ("sum", "none"):
        with pytest.raises(NotImplementedError, match="reduction"):
            CrossEntropyLoss(reduction=red)


def test_trainer_counts_samples_not_target_elements():
    import ldnn
    from ldnn.models.mlp import MLP
    from ldnn.optim import SGD
    from ldnn.train.trainer import train_local_epoch

    torch.manual_seed(3)
    m = MLP(12, (8,), 5)
    ldnn.prepare(m, "cpu")
    g = torch.Generator().manual_seed(4)
    batches = [(torch.randn(6, 12, generator=g), torch.softmax(torch.randn(6, 5, generator=g), 1)) for _ in range(3)]
    loss, acc, bl = train_local_epoch(m, batches, CrossEntropyLoss(), SGD(m.parameters(), lr=0.01), "cpu")
    assert train_local_epoch.last_samples == 18 and len(bl) == 3 and 0.0 <= acc <= 100.0
