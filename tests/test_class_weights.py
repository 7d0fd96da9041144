"""Class weights and ignore_index of the cross-entropy on the CPU path: ``ops.functional.cross_entropy``
and ``models.WeightedCrossEntropyLoss`` against ``F.cross_entropy(weight=, ignore_index=, label_smoothing=)``,
the weight rules of ``data.class_weights``, the --class_weights flag and the trainer's per-epoch rewrite.

The CPU path is torch's own arithmetic (its weighted sum over the kept rows' weight sum), so loss and
gradient agree with torch's mean to a few fp32 roundings of values of order 1: rtol 1e-5 / atol 1e-6.
"""
import json

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import ldnn  # noqa: F401
from ldnn.data.class_weights import class_weights_from_labels, parse_class_weights
from ldnn.models import CrossEntropyLoss, WeightedCrossEntropyLoss
from ldnn.ops import functional as LF

B, NC = 40, 7


def _case(seed=3):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, NC, generator=g) * 2
    y = torch.randint(0, NC, (B,), generator=g)
    y[0] = y[-1] = 2
    y[5:9] = 2
    w = torch.rand(NC, generator=g) * 3
    w[1] = 0.0
    q = torch.rand(B, NC, generator=g)
    q = q / q.sum(1, keepdim=True)
    return x, y, w, q


@pytest.mark.parametrize("soft", [False, True], ids=["labels", "probabilities"])
@pytest.mark.parametrize("eps", [0.0, 0.1])
@pytest.mark.parametrize("ignore_index", [-100, 2])
@pytest.mark.parametrize("weighted", [False, True], ids=["w=None", "w"])
def test_matches_torch(weighted, ignore_index, eps, soft):
    x, y, w, q = _case()
    w = w if weighted else None
    t = q if soft else y
    for call in (lambda lg, st: LF.cross_entropy(lg, t, st, eps, weight=w, ignore_index=ignore_index),
                 lambda lg, st: WeightedCrossEntropyLoss(weight=w, ignore_index=ignore_index,
                                                         label_smoothing=eps)(lg, t, st)):
        a = x.clone().requires_grad_(True)
        b = x.clone().requires_grad_(True)
        stats = torch.tensor([1.0, 2.0])
        loss = call(a, stats)
        # (torch refuses an ignore_index beside probability targets: it does not apply to them)
        ref = F.cross_entropy(b, t, weight=w, label_smoothing=eps,
                              **({} if soft else dict(ignore_index=ignore_index)))
        loss.backward()
        ref.backward()
        torch.testing.assert_close(loss, ref, rtol=1e-5, atol=1e-6)
        torch.testing.assert_close(a.grad, b.grad, rtol=1e-5, atol=1e-6)
        # stats: [B * mean loss, #correct over the kept rows] on top of what was there
        kept = torch.ones(B, dtype=torch.bool) if soft else y != ignore_index
        hit = x.argmax(1) == (q.argmax(1) if soft else y)
        torch.testing.assert_close(stats, torch.tensor([1.0 + ref.item() * B, 2.0 + float((hit & kept).sum())]),
                                   rtol=1e-5, atol=1e-5)


@pytest.mark.parametrize("weighted", [False, True], ids=["w=None", "w"])
def test_all_ignored_batch_is_zero_not_nan(weighted):
    x, y, w, _ = _case()
    a = x.clone().requires_grad_(True)
    stats = torch.zeros(2)
    loss = WeightedCrossEntropyLoss(weight=w if weighted else None, ignore_index=2)(a, torch.full((B,), 2), stats)
    loss.backward()
    assert loss.item() == 0.0 and a.grad.abs().max().item() == 0.0
    assert stats.tolist() == [0.0, 0.0]
    # ... and so is a batch whose every kept class has weight 0
    a = x.clone().requires_grad_(True)
    loss = WeightedCrossEntropyLoss(weight=w)(a, torch.full((B,), 1))
    loss.backward()
    assert loss.item() == 0.0 and a.grad.abs().max().item() == 0.0


def test_module_buffer_and_refusals():
    c = WeightedCrossEntropyLoss(weight=[1, 2, 3], ignore_index=1)
    assert isinstance(c, CrossEntropyLoss)   # (the trainer's on-device statistics path takes it)
    assert c.weight.dtype == torch.float32 and "weight" in dict(c.named_buffers()) and c.ignore_index == 1
    ptr = c.weight.data_ptr()
    c.set_class_weights(np.array([0.5, 0.0, 4.0]))
    assert c.weight.data_ptr() == ptr and c.weight.tolist() == [0.5, 0.0, 4.0]
    with pytest.raises(ValueError, match="3"):
        c.set_class_weights([1.0, 2.0])
    with pytest.raises(ValueError, match="without class weights"):
        WeightedCrossEntropyLoss().set_class_weights([1.0, 2.0, 3.0])
    for red in ("sum", "none"):
        with pytest.raises(NotImplementedError, match="reduction"):
            WeightedCrossEntropyLoss(weight=torch.ones(3), reduction=red)
    x, y, _, _ = _case()
    with pytest.raises(ValueError, match="one value per class"):
        LF.cross_entropy(x, y, weight=torch.ones(NC + 1))


def test_rules_on_a_hand_made_histogram():
    # n = 12 over 5 classes: n_c = [6, 0, 4, 2, 0], three classes present
    y = np.array([0] * 6 + [2] * 4 + [3] * 2)
    w = class_weights_from_labels(y, 5, "balanced")
    assert w.dtype == np.float32
    np.testing.assert_allclose(w, [12 / (3 * 6), 0, 12 / (3 * 4), 12 / (3 * 2), 0], rtol=1e-6)
    s = class_weights_from_labels(y, 5, "sqrt")
    raw = np.array([6 ** -0.5, 0, 4 ** -0.5, 2 ** -0.5, 0])
    np.testing.assert_allclose(s, raw * 12 / (raw * [6, 0, 4, 2, 0]).sum(), rtol=1e-6)
    for v in (w, s):   # the mean per-sample weight is 1, absent classes get 0
        np.testing.assert_allclose(v[y].mean(), 1.0, rtol=1e-6)
        assert v[1] == 0 and v[4] == 0
    assert class_weights_from_labels([], 3, "balanced").tolist() == [0, 0, 0]
    assert class_weights_from_labels(torch.tensor([1, 1]), 3, "sqrt").tolist() == [0, 1, 0]
    with pytest.raises(ValueError, match="rule"):
        class_weights_from_labels(y, 5, "median")
    with pytest.raises(ValueError, match="labels"):
        class_weights_from_labels([0, 5], 5, "balanced")


def test_flag_parses_and_refuses(monkeypatch):
    import ldnn.cli as cli
    from ldnn.models.mlp import mlp2

    p = cli.build_parser()
    assert p.parse_args([]).class_weights == "none"
    assert "weighted" in p.format_help()   # (val / test losses are the weighted ones: the help says so)
    assert parse_class_weights("none") is None and parse_class_weights("balanced") == "balanced"
    assert parse_class_weights("1,0,2.5", 3).tolist() == [1.0, 0.0, 2.5]
    base = ["--model", "mlp2", "--dataset", "mnist", "--device", "cpu"]
    with pytest.raises(SystemExit, match="10 weights expected"):
        cli.main(base + ["--class_weights", "1,2,3"])
    with pytest.raises(SystemExit, match=">= 0"):
        cli.main(base + ["--class_weights", "1,1,1,1,-1,1,1,1,1,1"])
    with pytest.raises(SystemExit, match="comma-separated"):
        cli.main(base + ["--class_weights", "median"])
    cpu = torch.device("cpu")
    with monkeypatch.context() as mp:
        mp.setattr(cli, "native_gpu", lambda dev: True)   # (as on a GPU host with the extension)
        a = p.parse_args(["--model", "mlp2", "--engine", "static", "--class_weights", "balanced"])
        with pytest.raises(SystemExit, match="--class_weights runs on the autograd path"):
            cli.resolve_engine(a, mlp2(), cpu, 1)
        a.engine = "auto"
        assert cli.resolve_engine(a, mlp2(), cpu, 1) is False
        a.class_weights = "none"
        assert cli.resolve_engine(a, mlp2(), cpu, 1) is True
    with pytest.raises(SystemExit):
        cli.main(base + ["--engine", "static", "--class_weights", "sqrt"])


def test_trainer_rewrites_the_weights_per_shard(tmp_path, monkeypatch):
    """Two global epochs on a class-skewed synthetic shard: the criterion's buffer is rewritten in
    place from each shard's histogram (it changes with the re-partition), and the epoch records
    carry the weights' range."""
    from ldnn.cli import main

    written = []
    real = WeightedCrossEntropyLoss.set_class_weights

    def spy(self, values):
        real(self, values)
        written.append((self.weight.data_ptr(), self.weight.clone()))

    monkeypatch.setattr(WeightedCrossEntropyLoss, "set_class_weights", spy)
    main(["--model", "mlp2", "--dataset", "mnist", "--n_train", "600", "--n_test", "80", "--epochs_global", "2",
          "--epochs_local", "1", "--device", "cpu", "--quiet", "--out_dir", str(tmp_path), "--plots", "", "--no_eval",
          "--partition", "skewed", "--fixed_ratio", "0.5", "--class_weights", "balanced", "--seed", "1"])
    # epoch start, after its re-partition, next epoch start, after its re-partition
    assert len(written) == 4
    assert len({p for p, _ in written}) == 1                      # one persistent buffer
    assert not torch.equal(written[0][1], written[1][1])          # the new shard has another histogram
    assert torch.equal(written[1][1], written[2][1])              # the epoch starts from what the shard gave
    ge = [r for r in map(json.loads, open(tmp_path / "metrics.rank0.jsonl")) if r.get("kind") == "global_epoch"]
    assert len(ge) == 2
    for r, (_, w) in zip(ge, (written[0], written[2])):
        assert r["class_weight_min"] == pytest.approx(w.min().item()) and \
            r["class_weight_max"] == pytest.approx(w.max().item())
        assert 0 <= r["class_weight_min"] <= 1 <= r["class_weight_max"]
    # an explicit list is written once, at construction, and reported as it is
    written.clear()
    out2 = tmp_path / "list"
    main(["--model", "mlp2", "--dataset", "mnist", "--n_train", "200", "--n_test", "40", "--epochs_global", "1",
          "--epochs_local", "1", "--device", "cpu", "--quiet", "--out_dir", str(out2), "--plots", "", "--no_eval",
          "--class_weights", "1,2,3,4,5,6,7,8,9,0.5"])
    assert not written
    ge = [r for r in map(json.loads, open(out2 / "metrics.rank0.jsonl")) if r.get("kind") == "global_epoch"]
    assert ge[0]["class_weight_min"] == 0.5 and ge[0]["class_weight_max"] == 9.0
