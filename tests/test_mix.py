"""Batch mixing on the host: the plan's draws, the CPU twin of the mix pass, the CLI."""
import json

import numpy as np
import pytest
import torch

from ldnn.data.mix import MODE_CUTMIX, MODE_MIXUP, MODE_NONE, BatchMix, mix_reference


def _same(a, b):
    return a.mode == b.mode and a.lam == b.lam and np.array_equal(a.perm, b.perm) and a.box == b.box


def test_plan_is_a_function_of_the_seed():
    m = BatchMix(0.2, 1.0, num_classes=10)
    for seed in (0, 1, 2 ** 62 + 5):
        assert _same(m.plan(seed, 16, 32, 32), m.plan(seed, 16, 32, 32))
    plans = [m.plan(s, 16, 32, 32) for s in range(40)]
    assert any(not _same(plans[0], p) for p in plans[1:])
    assert {p.mode for p in plans} == {MODE_MIXUP, MODE_CUTMIX}
    for p in plans:
        assert sorted(p.perm.tolist()) == list(range(16)) and p.perm.dtype == np.int64
        assert 0.0 <= p.lam <= 1.0


def test_mixup_lam_is_uniform_at_alpha_one():
    # Beta(1, 1) is uniform: the mean of n = 2000 draws has standard error 0.0065, 0.03 is > 4 sigma
    m = BatchMix(mixup_alpha=1.0, num_classes=10)
    lams = [m.plan(s, 8, 4, 4).lam for s in range(2000)]
    assert abs(float(np.mean(lams)) - 0.5) <= 0.03


def test_prob_zero_is_the_identity_plan():
    m = BatchMix(0.2, 1.0, prob=0.0, num_classes=10)
    for s in range(50):
        p = m.plan(s, 12, 8, 8)
        assert p.mode == MODE_NONE and p.lam == 1.0 and p.box == (0, 0, 0, 0)
        assert np.array_equal(p.perm, np.arange(12))


@pytest.mark.parametrize("switch,mode", [(0.0, MODE_MIXUP), (1.0, MODE_CUTMIX)])
def test_switch_prob_pins_the_mode(switch, mode):
    m = BatchMix(0.2, 1.0, switch_prob=switch, num_classes=10)
    assert {m.plan(s, 8, 8, 8).mode for s in range(50)} == {mode}
    # one alpha on: that mode whatever switch_prob says
    assert {BatchMix(0.2, 0.0, switch_prob=1.0, num_classes=3).plan(s, 8, 8, 8).mode for s in range(20)} == {MODE_MIXUP}
    assert {BatchMix(0.0, 1.0, switch_prob=0.0, num_classes=3).plan(s, 8, 8, 8).mode for s in range(20)} == {MODE_CUTMIX}


def test_constructor_refusals():
    for kw in (dict(), dict(mixup_alpha=-1.0), dict(mixup_alpha=float("nan")), dict(mixup_alpha=1.0, prob=1.5),
               dict(cutmix_alpha=1.0, switch_prob=-0.1), dict(mixup_alpha=1.0, num_classes=0)):
        with pytest.raises(ValueError):
            BatchMix(**kw)


@pytest.mark.parametrize("H,W", [(32, 32), (7, 5), (1, 1)])
def test_cutmix_box_and_lam(H, W):
    """Images constant per sample, distinct values, a derangement as perm (with a fixed point an
    in-box pixel would not differ): the fraction of changed pixels is exactly 1 - lam."""
    B = 6
    m = BatchMix(cutmix_alpha=1.0, num_classes=10)
    x = torch.arange(1, B + 1, dtype=torch.float32).view(B, 1, 1, 1).expand(B, 3, H, W).contiguous()
    y = torch.arange(B) % 10
    perm = np.roll(np.arange(B, dtype=np.int64), 1)
    for s in range(200):
        p = m.plan(s, B, H, W)
        y0, y1, x0, x1 = p.box
        assert p.mode == MODE_CUTMIX and 0 <= y0 <= y1 <= H and 0 <= x0 <= x1 <= W
        plan = type(p)(p.mode, p.lam, perm, p.box)
        out, q = mix_reference(x, y, torch.as_tensor(perm), plan, 10)
        # exact: the same pixels change in each of the B * 3 planes, and lam is 1 - that fraction
        changed = int((out != x).sum().item())
        assert changed % (B * 3) == 0 and p.lam == 1.0 - (changed // (B * 3)) / float(H * W)
        assert torch.equal(out[:, :, y0:y1, x0:x1], x[torch.as_tensor(perm)][:, :, y0:y1, x0:x1])
        torch.testing.assert_close(q.sum(1), torch.ones(B), rtol=0, atol=1e-6)
        torch.testing.assert_close(q[torch.arange(B), y], torch.full((B,), p.lam, dtype=torch.float32), rtol=0, atol=1e-6)


def test_cpu_mixup_and_targets():
    g = torch.Generator().manual_seed(3)
    x = torch.randn(5, 3, 7, 5, generator=g)
    y = torch.tensor([1, 2, 2, 0, 9])
    perm = np.array([1, 2, 0, 3, 4], dtype=np.int64)   # pairs (2, 2): one class twice; fixed points 3, 4
    m = BatchMix(mixup_alpha=1.0, num_classes=10)
    plan = type(m.plan(0, 5, 7, 5))(MODE_MIXUP, 0.37, perm, (0, 0, 0, 0))
    out, q = m.apply(x, y, plan)
    ref = 0.37 * x.double() + 0.63 * x[torch.as_tensor(perm)].double()
    assert bool(((out.double() - ref).abs() <= 2.0 ** -22 * (0.37 * x.abs() + 0.63 * x[torch.as_tensor(perm)].abs())).all())
    assert q.shape == (5, 10) and q.stride() == (12, 1) and q.dtype == torch.float32
    exp = torch.zeros(5, 10)
    exp[0, 1], exp[0, 2] = 0.37, 0.63
    exp[1, 2] = 1.0
    exp[2, 2], exp[2, 1] = 0.37, 0.63
    exp[3, 0] = exp[4, 9] = 1.0
    torch.testing.assert_close(q, exp, rtol=0, atol=1e-6)
    xb = x.bfloat16()
    ob, _ = m.apply(xb, y, plan)
    assert ob.dtype == torch.bfloat16
    refb = 0.37 * xb.double() + 0.63 * xb[torch.as_tensor(perm)].double()
    assert bool(((ob.double() - refb).abs() <= 2.0 ** -8 * refb.abs() + 1e-6).all())


def test_loader_yields_soft_targets_on_every_batch():
    from ldnn.data.datasets import ArrayDataset
    from ldnn.data.loader import DeviceLoader

    g = torch.Generator().manual_seed(4)
    ds = ArrayDataset(torch.randint(0, 256, (40, 3, 8, 8), dtype=torch.uint8, generator=g),
                      torch.randint(0, 10, (40,), generator=g), 10, None, None, "t")
    mk = lambda **kw: DeviceLoader(ds, None, 16, "cpu", seed=5, **kw)   # noqa: E731
    plain = list(mk())
    # prob = 0.5: mixed and unmixed batches alike come as (x, q [B, 10] fp32); unmixed ones one-hot
    ld = mk(mix=BatchMix(1.0, 1.0, prob=0.5))          # (the loader fills in the class count)
    assert ld.mix.num_classes == 10
    seen = set()
    for epoch in range(4):
        for (x, q), (x0, y0) in zip(ld, plain):
            assert q.shape == (x.shape[0], 10) and q.dtype == torch.float32 and x.shape == x0.shape
            torch.testing.assert_close(q.sum(1), torch.ones(x.shape[0]), rtol=0, atol=1e-6)
            if torch.equal(x, x0):
                seen.add("unmixed")
            else:
                seen.add("mixed")
    assert seen == {"mixed", "unmixed"}
    assert 0.0 <= ld.pop_mix_lam_mean() <= 1.0 and ld.mix_lams == []
    assert mk().pop_mix_lam_mean() is None
    a, b = list(mk(mix=BatchMix(0.2, 1.0))), list(mk(mix=BatchMix(0.2, 1.0)))
    assert all(torch.equal(p[0], r[0]) and torch.equal(p[1], r[1]) for p, r in zip(a, b))


def test_get_loaders_mix_only_the_train_loader():
    from ldnn.data.loader import get_loaders, get_subset_loaders

    mix = BatchMix(0.2, 1.0)
    tr, va, te, trainset, valset, tri, vai = get_loaders(16, 1, 0, None, "cpu", dataset="mnist", n_train=200, n_test=40,
                                                         partition_rule="equal", mix=mix)
    assert tr.mix is not None and tr.mix.num_classes == 10 and va.mix is None and te.mix is None
    tr2, va2, _, _ = get_subset_loaders(trainset, valset, tri, vai, 16, 0.5, 0.5, 1.0, "cpu",
                                        np.random.default_rng(0), mix=tr.mix)
    assert tr2.mix is tr.mix and va2.mix is None
    assert next(iter(va))[1].dtype == torch.long and next(iter(tr))[1].dtype == torch.float32


def test_cli_engine_and_ranges(monkeypatch):
    import ldnn.cli as cli
    from ldnn.models.mlp import mlp2

    p = cli.build_parser()
    cpu = torch.device("cpu")
    with monkeypatch.context() as mp:
        mp.setattr(cli, "native_gpu", lambda dev: True)
        for flag in ("--mixup", "--cutmix"):
            a = p.parse_args(["--model", "mlp2", "--engine", "static", flag, "0.2"])
            with pytest.raises(SystemExit, match="runs on the autograd path"):
                cli.resolve_engine(a, mlp2(), cpu, 1)
            a = p.parse_args(["--model", "mlp2", "--engine", "auto", flag, "0.2"])
            assert cli.resolve_engine(a, mlp2(), cpu, 1) is False
        a = p.parse_args(["--model", "mlp2", "--engine", "static"])
        assert cli.resolve_engine(a, mlp2(), cpu, 1) is True
    for bad in (["--mixup", "-0.1"], ["--cutmix", "nan"], ["--mixup", "0.2", "--mix_prob", "1.5"],
                ["--cutmix", "1.0", "--mix_switch_prob", "-0.5"]):
        with pytest.raises(SystemExit, match=bad[-2].lstrip("-")):
            cli.main(bad)


def test_cli_cpu_run_with_mixing(tmp_path):
    from ldnn.cli import main

    main(["--model", "mlp2", "--dataset", "mnist", "--n_train", "400", "--n_test", "80", "--epochs_global", "1",
          "--epochs_local", "1", "--device", "cpu", "--quiet", "--out_dir", str(tmp_path), "--plots", "",
          "--no_repartition", "--mixup", "0.2", "--cutmix", "1.0", "--label_smoothing", "0.1"])
    recs = [json.loads(ln) for ln in open(tmp_path / "metrics.rank0.jsonl")]
    ep = [r for r in recs if r.get("kind") == "global_epoch"][0]
    assert 0.0 <= ep["mix_lam_mean"] <= 1.0
    assert ep["samples"] == ep["shard_size"] > 0
    assert np.isfinite(ep["train_loss"]) and np.isfinite(ep["val_loss"])
    test = [r for r in recs if r.get("kind") == "test"][0]
    assert np.isfinite(test["test_loss"])   # (validation and test run on hard labels)
