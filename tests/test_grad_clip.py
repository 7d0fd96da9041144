"""Global-norm gradient clipping in the flat optimizers (optim/optimizers.py), CPU paths:
the torch-op fallback against torch.nn.utils.clip_grad_norm_ + torch.optim, the non-finite
skip, sharded == unsharded under FakeWorld, the extra scalar all-reduce in the collective
schedule, and the CLI (--clip_grad_norm)."""
import json
import os
import socket
import subprocess
import sys

import pytest
import torch

import ldnn
from ldnn.models import CrossEntropyLoss, build_model, xavier_init
from ldnn.optim import SGD, Adam, AdamW, build_optimizer
from ldnn.parallel.comm import FakeWorld
from ldnn.parallel.ddp import DataParallel

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _init_state():
    torch.manual_seed(0)
    m = build_model("lenet5")
    xavier_init(m)
    return m.state_dict()


INIT = _init_state()


def _lenet(flat=True):
    m = build_model("lenet5")
    m.load_state_dict(INIT)
    if flat:
        ldnn.prepare(m, "cpu")
    return m


def _batch(g, n=8):
    return torch.randn(n, 1, 28, 28, generator=g), torch.randint(0, 10, (n,), generator=g)


def _flat_state(opt):
    return {k: v.clone() for k, v in opt._ls().items() if torch.is_tensor(v) and k in ("momentum", "exp_avg", "exp_avg_sq")}


# ---------------------------------------------------------------- against stock torch
@pytest.mark.parametrize("Opt,TOpt,kw", [
    (SGD, torch.optim.SGD, dict(lr=0.05, momentum=0.9)),
    (Adam, torch.optim.Adam, dict(lr=1e-3)),
])
@pytest.mark.parametrize("flat", [True, False])
def test_clipped_steps_match_torch(Opt, TOpt, kw, flat):
    """5 steps of LeNet-5 against clip_grad_norm_ + torch.optim on a plain copy.  The loss is
    scaled in turn so the reference's own norms straddle the threshold: some steps clip, some
    do not.  Tolerance: tests/test_optim_models.py's for the unclipped optimizers.

    SGD: the plain copy runs its own backward.  Adam: it is handed the model's gradients
    instead -- the flat model's padded layout sums a backward in another order, and one fc1
    weight whose first gradient is 7.8e-8 (7.7e-8 in the plain copy, near Adam's eps) then
    moves 1.5e-6 apart under Adam WITHOUT any clipping; the models' backward is compared
    elsewhere, this test is about the optimizer step."""
    max_norm = 8.0
    m, r = _lenet(flat), _lenet(False)
    o, ro = Opt(m.parameters(), max_grad_norm=max_norm, **kw), TOpt(r.parameters(), **kw)
    g = torch.Generator().manual_seed(1)
    scales = [1.0, 8.0, 1.0, 8.0, 1.0]   # loss scale: an ordinary and a large gradient in turn
    norms = []
    for s in scales:
        x, y = _batch(g)
        o.zero_grad()
        (torch.nn.functional.cross_entropy(m(x), y) * s).backward()
        if Opt is SGD:
            ro.zero_grad()
            (torch.nn.functional.cross_entropy(r(x), y) * s).backward()
        else:
            for p, q in zip(m.parameters(), r.parameters()):
                q.grad = p.grad.detach().clone()
        norms.append(float(torch.nn.utils.clip_grad_norm_(r.parameters(), max_norm)))
        ro.step()
        o.step()
        torch.testing.assert_close(float(o.grad_clip_stats()["last_norm"]), norms[-1], rtol=1e-5, atol=1e-7)
    assert any(n > max_norm for n in norms) and any(n < max_norm for n in norms), norms
    st = o.grad_clip_stats()
    assert int(st["steps"]) == 5 and int(st["clipped"]) == sum(n > max_norm for n in norms)
    assert int(st["skipped"]) == 0
    for a, b in zip(m.parameters(), r.parameters()):
        torch.testing.assert_close(a.detach(), b.detach(), rtol=1e-5, atol=1e-6)


@pytest.mark.parametrize("Opt,kw", [(SGD, dict(lr=0.05, momentum=0.9, weight_decay=1e-4)), (Adam, dict(lr=1e-2)),
                                    (AdamW, dict(lr=1e-2))])
def test_huge_threshold_is_bit_identical_to_unclipped(Opt, kw):
    a, b = _lenet(), _lenet()
    oa, ob = Opt(a.parameters(), max_grad_norm=1e30, **kw), Opt(b.parameters(), **kw)
    g = torch.Generator().manual_seed(2)
    for _ in range(3):
        x, y = _batch(g)
        for mod, opt in ((a, oa), (b, ob)):
            opt.zero_grad()
            torch.nn.functional.cross_entropy(mod(x), y).backward()
            opt.step()
    for p, q in zip(a.parameters(), b.parameters()):
        assert torch.equal(p, q)
    sa, sb = _flat_state(oa), _flat_state(ob)
    assert sa.keys() == sb.keys() and sa
    for k in sa:
        assert torch.equal(sa[k], sb[k]), k
    assert oa._ls()["step"] == ob._ls()["step"] == 3
    assert ob.grad_clip_stats() is None and int(oa.grad_clip_stats()["clipped"]) == 0


@pytest.mark.parametrize("Opt,kw", [(SGD, dict(lr=0.05, momentum=0.9)), (Adam, dict(lr=1e-2))])
@pytest.mark.parametrize("flat", [True, False])
def test_non_finite_gradient_skips_the_step(Opt, kw, flat):
    m = _lenet(flat)
    o = Opt(m.parameters(), max_grad_norm=1.0, **kw)
    g = torch.Generator().manual_seed(3)
    x, y = _batch(g)
    o.zero_grad()
    torch.nn.functional.cross_entropy(m(x), y).backward()
    o.step()                                   # one ordinary step: momentum / moments exist
    before = [p.detach().clone() for p in m.parameters()]
    st_before = _flat_state(o) if flat else {id(p): {k: (v.clone() if torch.is_tensor(v) else v)
                                                     for k, v in o.state[p].items()} for p in m.parameters()}
    step_before = o._ls().get("step") if flat else None
    x2, y2 = _batch(g)
    o.zero_grad()
    torch.nn.functional.cross_entropy(m(x2), y2).backward()
    good = [p.grad.detach().clone() for p in m.parameters()]
    next(iter(m.parameters())).grad.view(-1)[3] = float("inf")
    o.step()
    assert int(o.grad_clip_stats()["skipped"]) == 1
    for p, q in zip(m.parameters(), before):
        assert torch.equal(p.detach(), q)
    if flat:
        assert o._ls()["step"] == step_before
        for k, v in _flat_state(o).items():
            assert torch.equal(v, st_before[k]), k
    else:
        for p in m.parameters():
            for k, v in o.state[p].items():
                assert torch.equal(v, st_before[id(p)][k]) if torch.is_tensor(v) else v == st_before[id(p)][k], k
    # the next finite step == the same step of an optimizer that never saw the inf
    m2 = _lenet(flat)
    o2 = Opt(m2.parameters(), max_grad_norm=1.0, **kw)
    o2.zero_grad()
    torch.nn.functional.cross_entropy(m2(x), y).backward()
    o2.step()
    for mod, opt in ((m, o), (m2, o2)):
        opt.zero_grad()
        mod(x2).sum().backward()      # (allocates / fills every .grad)
        for p, gg in zip(mod.parameters(), good):
            p.grad.copy_(gg)
        opt.step()
    for p, q in zip(m.parameters(), m2.parameters()):
        assert torch.equal(p.detach(), q.detach())


def test_first_step_skipped_then_equals_a_fresh_first_step():
    """The issue's wording: after a skipped step, the next finite step equals, bitwise, the
    first step of a fresh optimizer on the same gradient (momentum / moments / step count
    were never touched)."""
    for Opt, kw in ((SGD, dict(lr=0.05, momentum=0.9)), (Adam, dict(lr=1e-2))):
        m, m2 = _lenet(), _lenet()
        o, o2 = Opt(m.parameters(), max_grad_norm=1.0, **kw), Opt(m2.parameters(), max_grad_norm=1.0, **kw)
        x, y = _batch(torch.Generator().manual_seed(4))
        o.zero_grad()
        torch.nn.functional.cross_entropy(m(x), y).backward()
        f = o._flat_for_group(o.param_groups[0])
        keep = f.grad.clone()
        f.grad[5] = float("nan")
        o.step()
        assert int(o.grad_clip_stats()["skipped"]) == 1 and o._ls().get("step", 0) == 0
        f.grad.copy_(keep)
        o.step()
        o2.zero_grad()
        torch.nn.functional.cross_entropy(m2(x), y).backward()
        o2.step()
        for p, q in zip(m.parameters(), m2.parameters()):
            assert torch.equal(p.detach(), q.detach())
        for k, v in _flat_state(o).items():
            assert torch.equal(v, _flat_state(o2)[k]), k


def test_different_thresholds_per_group_are_refused():
    m = _lenet(False)
    ps = list(m.parameters())
    o = SGD([{"params": ps[:2], "max_grad_norm": 1.0}, {"params": ps[2:], "max_grad_norm": 2.0}], lr=0.1)
    m(torch.randn(2, 1, 28, 28)).sum().backward()
    with pytest.raises(ValueError, match="same in every param group"):
        o.step()


def test_interface_and_old_checkpoints():
    m = _lenet()
    o = build_optimizer("adam", m.parameters(), 1e-3, max_grad_norm=0.5)
    assert o.param_groups[0]["max_grad_norm"] == 0.5 and not o.supports_ranges()
    assert build_optimizer("sgd", m.parameters(), 0.1).grad_clip_stats() is None
    assert build_optimizer("sgd", m.parameters(), 0.1, max_grad_norm=0.0)._clip_threshold() is None
    # a state_dict saved before the key existed still loads, and steps unclipped
    m(torch.randn(2, 1, 28, 28)).sum().backward()
    o.step()
    sd = o.state_dict()
    assert not any(k.startswith("clip") or k == "hp" for k in sd["ldnn_flat_state"])
    for g in sd["param_groups"]:
        g.pop("max_grad_norm")
    o2 = Adam(m.parameters(), lr=1e-3, max_grad_norm=0.5)
    o2.load_state_dict(sd)
    assert o2._clip_threshold() is None
    o2.step()


# ---------------------------------------------------------------- data parallel (FakeWorld)
def _dp_train(comm, shard, optname, clip, local_weight=None, gossip=0, steps=3, batch=6):
    m = build_model("lenet5")
    m.load_state_dict(INIT)
    ldnn.prepare(m, "cpu")
    dp = DataParallel(m, comm, bucket_cap_mb=0.05, shard_optimizer=shard, local_weight=local_weight, gossip=gossip)
    kw = dict(max_grad_norm=clip)
    opt = SGD(m.parameters(), lr=0.05, momentum=0.9, **kw) if optname == "sgd" else Adam(m.parameters(), lr=1e-3, **kw)
    g = torch.Generator().manual_seed(10 + comm.rank)
    crit = CrossEntropyLoss()
    norms, grads = [], []
    n0 = comm.schedule_digest()[0]
    for _ in range(steps):
        x = torch.randn(batch, 1, 28, 28, generator=g)
        y = torch.randint(0, 10, (batch,), generator=g)
        opt.zero_grad()
        (crit(dp(x), y) * 20.0).backward()
        dp.finish_gradient_sync()
        f = dp.flat
        grads.append({s.name: f.storage_view(s, f.grad).double() * f.grad_scale for s in f.segments})
        opt.step()
        if clip is not None:
            norms.append(float(opt.grad_clip_stats()["last_norm"]))
    nops = comm.schedule_digest()[0] - n0
    comm.check_schedule("end of test")
    dp.gather_master(opt)
    st = {k: v.clone() for k, v in m.state_dict().items()}
    return st, norms, grads, nops, (None if clip is None else {k: float(v) for k, v in opt.grad_clip_stats().items()})


@pytest.mark.parametrize("optname", ["sgd", "adam"])
def test_sharded_clipping_equals_unsharded(optname):
    N, clip = 3, 1.0
    sh = FakeWorld(N).run(_dp_train, True, optname, clip)
    ref = FakeWorld(N).run(_dp_train, False, optname, clip)
    for r in range(N):
        for k, v in ref[r][0].items():
            torch.testing.assert_close(sh[r][0][k].float(), v.float(), rtol=1e-5, atol=1e-6, msg=k)
    for step in range(3):
        # the norm of the averaged gradient, in fp64, from the unsharded run (whole on every rank)
        want = float(sum(g.square().sum() for g in ref[0][2][step].values()).sqrt())
        for r in range(N):
            assert sh[r][1][step] == sh[0][1][step]            # every rank reports the same norm
            torch.testing.assert_close(sh[r][1][step], want, rtol=1e-5, atol=0)
            torch.testing.assert_close(ref[r][1][step], want, rtol=1e-5, atol=0)
    assert sh[0][4]["clipped"] >= 1, sh[0][4]     # the threshold did bite


@pytest.mark.parametrize("kw", [dict(local_weight=0.7), dict(gossip=1)])
def test_weighted_mix_and_gossip_clip_their_own_gradient(kw):
    """Unsharded weighted all-reduce / ring gossip: every rank's optimizer sees its own complete
    post-mix gradient, so each steps with a finite norm of its own -- the norm of that gradient."""
    N = 3
    res = FakeWorld(N).run(_dp_train, False, "sgd", 1.0, **kw)
    for r in range(N):
        for step in range(3):
            want = float(sum(g.square().sum() for g in res[r][2][step].values()).sqrt())
            assert want > 0 and want == want
            torch.testing.assert_close(res[r][1][step], want, rtol=1e-5, atol=0)
        assert res[r][4]["steps"] == 3 and res[r][4]["skipped"] == 0
    assert len({res[r][1][0] for r in range(N)}) > 1    # per-rank norms


def _dp_inf(comm, shard):
    m = build_model("lenet5")
    m.load_state_dict(INIT)
    ldnn.prepare(m, "cpu")
    dp = DataParallel(m, comm, bucket_cap_mb=0.05, shard_optimizer=shard)
    opt = Adam(m.parameters(), lr=1e-3, max_grad_norm=1.0)
    g = torch.Generator().manual_seed(20 + comm.rank)
    crit = CrossEntropyLoss()
    for step in range(2):
        x, y = torch.randn(6, 1, 28, 28, generator=g), torch.randint(0, 10, (6,), generator=g)
        if step == 1 and comm.rank == 1:      # ONE rank overflows (its buckets go out NaN)
            x[0, 0, 0, 0] = float("inf")
        opt.zero_grad()
        crit(dp(x), y).backward()
        dp.finish_gradient_sync()
        if step == 1:
            dp.wait_gathers()
            before = (dp.flat.master.clone(), {k: v.clone() for k, v in _flat_state(opt).items()}, opt._ls()["step"])
        opt.step()
    dp.wait_gathers()
    same = torch.equal(dp.flat.master, before[0]) and all(torch.equal(v, before[1][k])
                                                          for k, v in _flat_state(opt).items())
    return same, opt._ls()["step"] == before[2], {k: float(v) for k, v in opt.grad_clip_stats().items()}


@pytest.mark.parametrize("shard", [True, False])
def test_one_ranks_overflow_skips_the_step_on_every_rank(shard):
    for same, step_same, st in FakeWorld(3).run(_dp_inf, shard):
        assert same and step_same and st["skipped"] == 1 and st["steps"] == 2, st


def test_sharded_clipping_adds_one_all_reduce_per_step():
    N, steps = 3, 3
    on = FakeWorld(N).run(_dp_train, True, "adam", 1.0)
    off = FakeWorld(N).run(_dp_train, True, "adam", None)
    unsh_on = FakeWorld(N).run(_dp_train, False, "adam", 1.0)
    unsh_off = FakeWorld(N).run(_dp_train, False, "adam", None)
    for r in range(N):
        assert on[r][3] - off[r][3] == steps       # exactly one more collective per step (check_schedule passed)
        assert unsh_on[r][3] == unsh_off[r][3]     # the unsharded path needs none


# ---------------------------------------------------------------- CLI
def test_cli_engine_resolution():
    from ldnn.cli import build_parser, resolve_engine
    from ldnn.models.mlp import mlp2

    a = build_parser().parse_args(["--engine", "static", "--clip_grad_norm", "1"])
    with pytest.raises(SystemExit, match="static"):
        resolve_engine(a, mlp2(), torch.device("cpu"), 1)
    a.engine = "auto"
    assert resolve_engine(a, mlp2(), torch.device("cpu"), 1) is False
    assert build_parser().parse_args([]).clip_grad_norm == 0.0


def test_cli_static_engine_message(monkeypatch):
    """With everything else in favour of the static engine, --clip_grad_norm is the stated reason."""
    from ldnn import cli
    from ldnn.models.mlp import mlp2

    model, dev = mlp2(), torch.device("cpu")
    monkeypatch.setattr(cli, "native_gpu", lambda d: True)   # (as on a GPU host with the extension)
    a = cli.build_parser().parse_args(["--engine", "static", "--clip_grad_norm", "1"])
    with pytest.raises(SystemExit, match="--clip_grad_norm runs on the autograd path"):
        cli.resolve_engine(a, model, dev, 1)
    a.engine = "auto"
    assert cli.resolve_engine(a, model, dev, 1) is False
    a.clip_grad_norm = 0.0
    assert cli.resolve_engine(a, model, dev, 1) is True


KEYS = {"grad_norm_last", "grad_clipped_steps", "grad_skipped_steps"}


@pytest.mark.parametrize("clip", ["0.5", "0"])
def test_cli_metrics_fields(tmp_path, clip):
    from ldnn.cli import main

    main(["--model", "mlp2", "--dataset", "mnist", "--n_train", "400", "--n_test", "80", "--epochs_global", "1",
          "--epochs_local", "1", "--device", "cpu", "--quiet", "--out_dir", str(tmp_path), "--plots", "", "--no_eval",
          "--clip_grad_norm", clip])
    recs = [json.loads(l) for l in open(tmp_path / "metrics.rank0.jsonl")]
    ge = [r for r in recs if r.get("kind") == "global_epoch"]
    assert ge
    for r in ge:
        if clip == "0":
            assert not (KEYS & set(r))
        else:
            assert KEYS <= set(r)
            assert r["grad_norm_last"] > 0 and r["grad_skipped_steps"] == 0 and r["grad_clipped_steps"] >= 0


def test_cli_batchnorm_model_with_clipping_and_digest(tmp_path):
    """A BatchNorm model through the CLI (its state_dict holds 0-dim int64 counters): trains
    clipped, logs the metrics fields and, on request only, the final_weights digest."""
    from ldnn.cli import main, weights_digest

    for name in ("enhanced_cnn_small", "resnet18"):
        assert len(weights_digest(build_model(name))) == 64
    for flag in ([], ["--log_weights_digest"]):
        out = tmp_path / ("d" if flag else "n")
        main(["--model", "enhanced_cnn_small", "--dataset", "cifar10", "--n_train", "96", "--n_test", "32",
              "--batch_size", "32", "--epochs_global", "1", "--epochs_local", "1", "--device", "cpu", "--quiet",
              "--out_dir", str(out), "--plots", "", "--no_eval", "--clip_grad_norm", "1.0"] + flag)
        recs = [json.loads(l) for l in open(out / "metrics.rank0.jsonl")]
        assert all(KEYS <= set(r) for r in recs if r.get("kind") == "global_epoch")
        fin = [r for r in recs if r.get("kind") == "final_weights"]
        assert len(fin) == (1 if flag else 0)
        assert all(len(r["sha256"]) == 64 for r in fin)


def _port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


@pytest.mark.slow
def test_cli_two_gloo_ranks_sharded_equals_unsharded(tmp_path):
    """train.py --sync_every step --clip_grad_norm 0.5 on 2 gloo ranks, mlp2: the final weights
    agree across the ranks (each rank's metrics file ends with the sha256 of its own replica,
    the one rank 0 checkpoints) and between the sharded and the replicated optimizer."""
    finals = {}
    for mode in ("on", "off"):
        out = tmp_path / mode
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
               "--master-port", str(_port()), os.path.join(ROOT, "train.py"), "--model", "mlp2", "--dataset", "mnist",
               "--n_train", "600", "--n_test", "100", "--epochs_global", "1", "--epochs_local", "1", "--device", "cpu",
               "--quiet", "--out_dir", str(out), "--plots", "", "--sync_every", "step", "--shard_optimizer", mode,
               "--optimizer", "sgd", "--lr", "0.05", "--checkpoint_every", "1", "--no_eval", "--bucket_mb", "0.05",
               "--clip_grad_norm", "0.5", "--no_repartition", "--partition_rule", "equal",
               "--log_weights_digest"]   # (equal: the shards do
        # not depend on the measured probe durations, so the two runs see the same data)
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-3000:]
        ck = sorted((out / "ckpt").glob("ckpt_ge*.pt"))
        assert ck, list(out.iterdir())
        finals[mode] = torch.load(ck[-1], weights_only=True)["model"]
        recs = [json.loads(l) for l in open(out / "metrics.rank0.jsonl")]
        assert all(KEYS <= set(r) for r in recs if r.get("kind") == "global_epoch")
        digests = []
        for rank in (0, 1):
            fin = [json.loads(l) for l in open(out / f"metrics.rank{rank}.jsonl")]
            fin = [r["sha256"] for r in fin if r.get("kind") == "final_weights"]
            assert len(fin) == 1, (mode, rank)
            digests.append(fin[0])
        assert digests[0] == digests[1], (mode, digests)      # bitwise equal replicas
        # ... and that digest is of the weights compared between the modes below
        from ldnn.cli import weights_digest
        from ldnn.models import build_model as _bm

        chk = _bm("mlp2")
        chk.load_state_dict(finals[mode])
        assert weights_digest(chk) == digests[0], mode
    for k, v in finals["off"].items():
        torch.testing.assert_close(finals["on"][k].float(), v.float(), rtol=1e-5, atol=1e-6, msg=k)
