"""Focal loss (Lin et al. 2017) of the cross-entropy on the CPU path: ``ops.functional.cross_entropy(focal_gamma=)``
and ``models.FocalLoss`` against a float64 autograd oracle, the refusals, the --focal_gamma flag and a short
trainer run.

The oracle forms q = 1 - p from the other classes, q = exp(logsumexp(x over c != y) - logsumexp(x)), so that it
stays finite on the planted saturated rows (where (1 - p) ** gamma gives NaN gradients even in float64):
loss = sum_kept a q^gamma (-log_softmax(x)[y]) / sum_kept a, a = w[y] (1 without weights).

The CPU path is the same formula in fp32 torch ops, on values of order 1 and sums of at most 300 rows:
rtol 1e-4 / atol 1e-5 for loss and gradient (a few hundred fp32 roundings; pow amplifies log's rounding by
gamma |log q| <= ~100).
"""
import json
import math

import pytest
import torch

import ldnn  # noqa: F401
from ldnn.models import CrossEntropyLoss, FocalLoss, WeightedCrossEntropyLoss
from ldnn.ops import functional as LF


def focal_oracle(logits, y, w, ignore_index, gamma):
    """(loss, d loss / d logits, #correct over kept rows) in float64 with autograd."""
    x = logits.detach().double().requires_grad_(True)
    ncls = x.shape[1]
    kept = (y != ignore_index) & (y >= 0) & (y < ncls)
    safe = torch.where(kept, y, torch.zeros_like(y))
    hot = torch.nn.functional.one_hot(safe, ncls).bool()
    lse = torch.logsumexp(x, 1)
    q = torch.exp(torch.logsumexp(x.masked_fill(hot, float("-inf")), 1) - lse)
    nlp = -torch.log_softmax(x, 1).gather(1, safe[:, None])[:, 0]
    a = kept.double() if w is None else w.double()[safe] * kept
    den = a.sum()
    loss = (a * q ** gamma * nlp).sum() / den
    loss.backward()
    hit = (x.detach().argmax(1) == y) & kept
    return loss.detach(), x.grad, int(hit.sum().item())


def _case(B, NC, ignore_index, seed=3):
    """Logits, labels with about a fifth of the rows ignored, weights with one exact 0; rows 0 and 1 are the
    planted ones (kept, class 0, weight > 0): p rounds to 1 in row 0, p ~ e^-60 in row 1."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, NC, generator=g) * 3
    y = torch.randint(0, NC, (B,), generator=g)
    y[torch.rand(B, generator=g) < 0.2] = ignore_index
    y[-1] = ignore_index
    w = torch.rand(NC, generator=g) * 3 + 0.1
    w[1] = 0.0
    y[0] = y[1] = 0
    x[0] = -60.0
    x[0, 0] = 60.0
    x[1] = 0.0
    x[1, 0] = -60.0
    return x, y, w


@pytest.mark.parametrize("weighted", [False, True], ids=["w=None", "w"])
@pytest.mark.parametrize("ignore_index", [-100, 2])
@pytest.mark.parametrize("gamma", [0.25, 0.5, 2.0])
@pytest.mark.parametrize("B,NC", [(300, 10), (5, 3)])
def test_matches_the_oracle(B, NC, gamma, ignore_index, weighted):
    x, y, w = _case(B, NC, ignore_index)
    w = w if weighted else None
    ref, grad, correct = focal_oracle(x, y, w, ignore_index, gamma)
    for call in (lambda lg, st: LF.cross_entropy(lg, y, st, weight=w, ignore_index=ignore_index, focal_gamma=gamma),
                 lambda lg, st: FocalLoss(gamma, weight=w, ignore_index=ignore_index)(lg, y, st)):
        a = x.clone().requires_grad_(True)
        stats = torch.tensor([1.0, 2.0])
        loss = call(a, stats)
        loss.backward()
        assert math.isfinite(loss.item()) and bool(torch.isfinite(a.grad).all()) and bool(torch.isfinite(stats).all())
        torch.testing.assert_close(loss.double(), ref, rtol=1e-4, atol=1e-5)
        torch.testing.assert_close(a.grad.double(), grad, rtol=1e-4, atol=1e-5)
        assert a.grad[0].abs().max().item() == 0.0            # the saturated row
        assert a.grad[y == ignore_index].abs().max().item() == 0.0
        torch.testing.assert_close(stats.double(), torch.tensor([1.0 + ref.item() * B, 2.0 + correct],
                                                                dtype=torch.float64), rtol=1e-4, atol=1e-4)


@pytest.mark.parametrize("weighted", [False, True], ids=["w=None", "w"])
@pytest.mark.parametrize("ignore_index", [-100, 2])
def test_gamma_zero_is_the_cross_entropy(weighted, ignore_index):
    x, y, w = _case(40, 7, ignore_index, seed=5)
    w = w if weighted else None
    if ignore_index == -100:
        y = y.clamp_min(0)   # (-100 rows: only the weighted entry takes them without the keyword)
    a = x.clone().requires_grad_(True)
    b = x.clone().requires_grad_(True)
    la = LF.cross_entropy(a, y, None, 0.0, w, ignore_index, focal_gamma=0.0)
    lb = LF.cross_entropy(b, y, None, 0.0, w, ignore_index)
    la.backward()
    lb.backward()
    assert torch.equal(la, lb) and torch.equal(a.grad, b.grad)
    crit = FocalLoss(0.0, weight=w, ignore_index=ignore_index)
    assert torch.equal(crit(x, y), WeightedCrossEntropyLoss(weight=w, ignore_index=ignore_index)(x, y))


def test_all_ignored_batch_is_zero_not_nan():
    x, _, w = _case(40, 7, 2)
    a = x.clone().requires_grad_(True)
    stats = torch.zeros(2)
    loss = FocalLoss(2.0, weight=w, ignore_index=2)(a, torch.full((40,), 2), stats)
    loss.backward()
    assert loss.item() == 0.0 and a.grad.abs().max().item() == 0.0 and stats.tolist() == [0.0, 0.0]


def test_refusals():
    x, y, w = _case(40, 7, -100)
    y = y.clamp_min(0)
    q = torch.softmax(x, 1)
    with pytest.raises(ValueError, match="label_smoothing"):
        LF.cross_entropy(x, y, None, 0.1, focal_gamma=2.0)
    with pytest.raises(ValueError, match="target"):
        LF.cross_entropy(x, q, focal_gamma=2.0)
    for bad in (-1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="focal_gamma"):
            LF.cross_entropy(x, y, focal_gamma=bad)
        with pytest.raises(ValueError, match="gamma"):
            FocalLoss(bad)
    LF.cross_entropy(x, q, None, 0.1, focal_gamma=0.0)   # gamma == 0 is today's call: nothing is refused
    with pytest.raises(ValueError, match="label_smoothing"):
        FocalLoss(2.0, label_smoothing=0.1)
    for red in ("sum", "none"):
        with pytest.raises(NotImplementedError, match="reduction"):
            FocalLoss(2.0, reduction=red)
    with pytest.raises(ValueError, match="class-probability"):
        FocalLoss(2.0)(x, q)


def test_module():
    c = FocalLoss(weight=[1, 2, 3], ignore_index=1)
    assert isinstance(c, WeightedCrossEntropyLoss) and isinstance(c, CrossEntropyLoss)
    assert c.gamma == 2.0 and c.label_smoothing == 0.0 and c.ignore_index == 1
    assert "weight" in dict(c.named_buffers()) and "gamma" not in c.state_dict()
    ptr = c.weight.data_ptr()
    c.set_class_weights([0.5, 0.0, 4.0])
    assert c.weight.data_ptr() == ptr and c.weight.tolist() == [0.5, 0.0, 4.0]
    c.gamma = 0.5   # a plain attribute: the next call uses it
    x = torch.tensor([[0.0, 1.0, 2.0], [2.0, 0.0, -1.0]])
    y = torch.tensor([2, 0])
    ref, _, _ = focal_oracle(x, y, c.weight, 1, 0.5)
    torch.testing.assert_close(c(x, y).double(), ref, rtol=1e-5, atol=1e-6)


def test_flag_parses_and_refuses(monkeypatch):
    import ldnn.cli as cli
    from ldnn.models.mlp import mlp2

    p = cli.build_parser()
    assert p.parse_args([]).focal_gamma == 0.0
    a = p.parse_args(["--focal_gamma", "2", "--class_weights", "balanced"])
    assert a.focal_gamma == 2.0 and a.class_weights == "balanced"
    assert "focal ones" in " ".join(p.format_help().split())   # (val / test losses: the help says so)
    base = ["--model", "mlp2", "--dataset", "mnist", "--device", "cpu", "--focal_gamma", "2"]
    for extra in (["--label_smoothing", "0.1"], ["--mixup", "0.2"], ["--cutmix", "1.0"]):
        with pytest.raises(SystemExit, match=f"--focal_gamma with {extra[0]}"):
            cli.main(base + extra)
    for bad in ("-1", "nan", "inf"):
        with pytest.raises(SystemExit, match="--focal_gamma must be finite"):
            cli.main(base[:-1] + [bad])
    cpu = torch.device("cpu")
    with monkeypatch.context() as mp:
        mp.setattr(cli, "native_gpu", lambda dev: True)   # (as on a GPU host with the extension)
        a = p.parse_args(["--model", "mlp2", "--engine", "static", "--focal_gamma", "2"])
        with pytest.raises(SystemExit, match="--focal_gamma runs on the autograd path"):
            cli.resolve_engine(a, mlp2(), cpu, 1)
        a.engine = "auto"
        assert cli.resolve_engine(a, mlp2(), cpu, 1) is False
        a.focal_gamma = 0.0
        assert cli.resolve_engine(a, mlp2(), cpu, 1) is True
    with pytest.raises(SystemExit):
        cli.main(base + ["--engine", "static"])


def test_trainer_runs_with_the_focal_criterion(tmp_path, monkeypatch):
    """One global epoch on a class-skewed synthetic shard with --class_weights balanced --focal_gamma 2: the
    criterion is a FocalLoss whose weights the trainer rewrites in place, and the epoch's loss is finite."""
    from ldnn.cli import main

    seen = []
    real = FocalLoss.forward

    def spy(self, logits, labels, stats=None):
        seen.append((self.gamma, self.weight.data_ptr()))
        return real(self, logits, labels, stats)

    monkeypatch.setattr(FocalLoss, "forward", spy)
    main(["--model", "mlp2", "--dataset", "mnist", "--n_train", "600", "--n_test", "80", "--epochs_global", "1",
          "--epochs_local", "1", "--device", "cpu", "--quiet", "--out_dir", str(tmp_path), "--plots", "", "--no_eval",
          "--partition", "skewed", "--fixed_ratio", "0.5", "--class_weights", "balanced", "--focal_gamma", "2",
          "--seed", "1"])
    assert seen and {g for g, _ in seen} == {2.0} and len({p for _, p in seen}) == 1
    ge = [r for r in map(json.loads, open(tmp_path / "metrics.rank0.jsonl")) if r.get("kind") == "global_epoch"]
    assert len(ge) == 1
    losses = [v for k, v in ge[0].items() if "loss" in k and isinstance(v, (int, float))]
    assert losses and all(math.isfinite(v) and v >= 0 for v in losses), ge[0]
    assert 0 <= ge[0]["class_weight_min"] <= 1 <= ge[0]["class_weight_max"]
