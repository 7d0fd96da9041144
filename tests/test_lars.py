"""LARS in the flat SGD (optim/optimizers.py), CPU paths: the torch-op fallback against an
oracle written out here (per-tensor fp64 norms, the trust-ratio formula, torch.optim.SGD on a
plain copy), its edge cases, clipping + LARS, the state_dict round trip, sharded == unsharded
under FakeWorld with exactly one extra all-reduce, and the CLI (--optimizer lars)."""
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
TRUST, EPS, WD = 0.02, 1e-8, 1e-4


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


def _oracle_ratio(w, g, wd, trust=TRUST, eps=EPS, exclude_1d=True):
    """The issue's formula on one tensor, norms in fp64."""
    wn, gn = w.detach().double().norm().item(), g.double().norm().item()
    if wn > 0 and gn > 0 and not (exclude_1d and w.dim() < 2):
        return trust * wn / (gn + wd * wn + eps)
    return 1.0


def _oracle_step(r, ro, wd, max_norm=None, **kw):
    """One LARS step of the plain copy ``r`` (gradients already in .grad): clip first, ratios of
    the clipped gradient, u = ratio * (g + wd * w) handed to torch.optim.SGD(weight_decay=0)."""
    if max_norm is not None:
        torch.nn.utils.clip_grad_norm_(r.parameters(), max_norm)
    ratios = {}
    for n, p in r.named_parameters():
        ratios[n] = _oracle_ratio(p, p.grad, wd, **kw)
        p.grad = (ratios[n] * (p.grad + wd * p.detach())).float()
    ro.step()
    return ratios


def _stats_by_name(o, m):
    st = o.lars_stats()
    if st["names"] and st["names"][0].startswith("param"):   # per-tensor path: parameter order
        names = [n for n, _ in m.named_parameters()]
    else:
        names = st["names"]
    return {n: (float(st["ratio"][i]), float(st["w_norm"][i]), float(st["g_norm"][i])) for i, n in enumerate(names)}


# ---------------------------------------------------------------- 1. oracle
@pytest.mark.parametrize("nesterov", [False, True])
@pytest.mark.parametrize("flat", [True, False])
def test_lars_steps_match_the_oracle(flat, nesterov):
    """5 steps of LeNet-5 (1-D and 4-D tensors, the padded 10-row head), momentum 0.9, weight
    decay 1e-4.  Tolerance: tests/test_grad_clip.py::test_clipped_steps_match_torch's."""
    m, r = _lenet(flat), _lenet(False)
    kw = dict(lr=0.05, momentum=0.9, nesterov=nesterov)
    o = SGD(m.parameters(), weight_decay=WD, lars_trust=TRUST, lars_eps=EPS, **kw)
    ro = torch.optim.SGD(r.parameters(), weight_decay=0, **kw)
    g = torch.Generator().manual_seed(1)
    for _ in range(5):
        x, y = _batch(g)
        for mod, opt in ((m, o), (r, ro)):
            opt.zero_grad()
            torch.nn.functional.cross_entropy(mod(x), y).backward()
        want = _oracle_step(r, ro, WD)
        o.step()
        got = _stats_by_name(o, m)
        for n, v in want.items():
            assert got[n][0] == pytest.approx(v, rel=1e-5), n
    assert any(v != 1.0 for v in want.values()) and any(v == 1.0 for v in want.values())
    for a, b in zip(m.parameters(), r.parameters()):
        torch.testing.assert_close(a.detach(), b.detach(), rtol=1e-5, atol=1e-6)


# ---------------------------------------------------------------- 2. off == plain SGD
def test_lars_off_is_bit_identical_to_plain_sgd():
    a, b = _lenet(), _lenet()
    kw = dict(lr=0.05, momentum=0.9, weight_decay=WD)
    oa, ob = SGD(a.parameters(), lars_trust=None, **kw), SGD(b.parameters(), **kw)
    g = torch.Generator().manual_seed(2)
    for _ in range(3):
        x, y = _batch(g)
        for mod, opt in ((a, oa), (b, ob)):
            opt.zero_grad()
            torch.nn.functional.cross_entropy(mod(x), y).backward()
            opt.step()
    fa, fb = (o._flat_for_group(o.param_groups[0]) for o in (oa, ob))
    assert torch.equal(fa.master, fb.master)
    assert torch.equal(oa._ls()["momentum"], ob._ls()["momentum"])
    assert oa.lars_stats() is None and "lars" not in oa._ls()
    assert oa.supports_ranges() == ob.supports_ranges()


# ---------------------------------------------------------------- 3. edge cases
@pytest.mark.parametrize("flat", [True, False])
def test_zero_gradient_zero_tensor_and_1d_tensors(flat):
    m = _lenet(flat)
    ps = dict(m.named_parameters())
    zero_g = "fc2.weight"
    o = SGD(m.parameters(), lr=0.1, weight_decay=0.01, lars_trust=TRUST)
    x, y = _batch(torch.Generator().manual_seed(3))
    o.zero_grad()
    torch.nn.functional.cross_entropy(m(x), y).backward()
    ps[zero_g].grad.zero_()
    before = {n: p.detach().clone() for n, p in ps.items()}
    grads = {n: p.grad.detach().clone() for n, p in ps.items()}
    o.step()
    got = _stats_by_name(o, m)
    assert got[zero_g][0] == 1.0 and got[zero_g][2] == 0.0
    # the zero-gradient tensor moved by weight decay alone: w -= lr * wd * w
    torch.testing.assert_close(ps[zero_g].detach(), before[zero_g] * (1 - 0.1 * 0.01), rtol=1e-6, atol=1e-8)
    for n, p in ps.items():
        if p.dim() < 2:
            assert got[n][0] == 1.0, n
            torch.testing.assert_close(p.detach(), before[n] - 0.1 * (grads[n] + 0.01 * before[n]), rtol=1e-5,
                                       atol=1e-7)
        elif n != zero_g:
            assert got[n][0] == pytest.approx(_oracle_ratio(before[n], grads[n], 0.01), rel=1e-5) and got[n][0] != 1.0
    # lars_exclude_1d=False adapts them; a tensor of zeros (here a bias: zeroing a weight matrix
    # would take other tensors' gradients with it) keeps ratio 1
    m2 = _lenet(flat)
    with torch.no_grad():
        dict(m2.named_parameters())["fc3.bias"].zero_()
        dict(m2.named_parameters())["fc2.bias"].fill_(0.1)
    o2 = SGD(m2.parameters(), lr=0.1, weight_decay=0.01, lars_trust=TRUST, lars_exclude_1d=False)
    o2.zero_grad()
    torch.nn.functional.cross_entropy(m2(x), y).backward()
    want = {n: _oracle_ratio(p, p.grad, 0.01, exclude_1d=False) for n, p in m2.named_parameters()}
    o2.step()
    got2 = _stats_by_name(o2, m2)
    for n, p in m2.named_parameters():
        assert got2[n][0] == pytest.approx(want[n], rel=1e-5), n
    assert got2["fc3.bias"][0] == 1.0 and got2["fc3.bias"][1] == 0.0 and got2["fc3.bias"][2] > 0
    assert got2["fc2.bias"][0] != 1.0


# ---------------------------------------------------------------- 4. clipping + LARS
@pytest.mark.parametrize("flat", [True, False])
def test_clipping_and_lars_match_the_oracle(flat):
    """Clip first (global norm of the raw gradient), LARS norms of the clipped gradient; then a
    non-finite gradient skips the step and leaves lars_stats() untouched."""
    max_norm = 1.0
    m, r = _lenet(flat), _lenet(False)
    kw = dict(lr=0.05, momentum=0.9)
    o = SGD(m.parameters(), weight_decay=WD, lars_trust=TRUST, max_grad_norm=max_norm, **kw)
    ro = torch.optim.SGD(r.parameters(), weight_decay=0, **kw)
    g = torch.Generator().manual_seed(4)
    for s in (1.0, 20.0, 1.0, 20.0):
        x, y = _batch(g)
        for mod, opt in ((m, o), (r, ro)):
            opt.zero_grad()
            (torch.nn.functional.cross_entropy(mod(x), y) * s).backward()
        want = _oracle_step(r, ro, WD, max_norm=max_norm)
        o.step()
        got = _stats_by_name(o, m)
        for n, v in want.items():
            assert got[n][0] == pytest.approx(v, rel=1e-5), n
    assert int(o.grad_clip_stats()["clipped"]) >= 1 and int(o.grad_clip_stats()["steps"]) == 4
    for a, b in zip(m.parameters(), r.parameters()):
        torch.testing.assert_close(a.detach(), b.detach(), rtol=1e-5, atol=1e-6)
    # a non-finite gradient: skipped, nothing moves, the ratio statistics stay
    st = o.lars_stats()
    stats_before = {k: st[k].clone() for k in ("ratio", "w_norm", "g_norm")}
    before = [p.detach().clone() for p in m.parameters()]
    x, y = _batch(g)
    o.zero_grad()
    torch.nn.functional.cross_entropy(m(x), y).backward()
    next(iter(m.parameters())).grad.view(-1)[3] = float("inf")
    o.step()
    assert int(o.grad_clip_stats()["skipped"]) == 1
    for p, q in zip(m.parameters(), before):
        assert torch.equal(p.detach(), q)
    st = o.lars_stats()
    for k, v in stats_before.items():
        assert torch.equal(st[k], v), k


# ---------------------------------------------------------------- 5. state_dict
def test_state_dict_round_trip_and_old_checkpoints():
    m = _lenet()
    o = SGD(m.parameters(), lr=0.05, momentum=0.9, weight_decay=WD, lars_trust=TRUST, lars_eps=1e-6,
            lars_exclude_1d=False)
    m(torch.randn(2, 1, 28, 28)).sum().backward()
    o.step()
    sd = o.state_dict()
    assert not any(k.startswith("lars") or k == "hp" for k in sd["ldnn_flat_state"])
    o2 = SGD(m.parameters(), lr=0.1)
    o2.load_state_dict(sd)
    assert o2._lars_conf() == (TRUST, 1e-6, False)
    assert torch.equal(o2._ls()["momentum"], o._ls()["momentum"])
    o2.step()
    assert float(o2.lars_stats()["ratio"].min()) < 1.0
    # a state saved before the keys existed loads, and steps without LARS
    for g in sd["param_groups"]:
        for k in ("lars_trust", "lars_eps", "lars_exclude_1d"):
            g.pop(k)
    o3 = SGD(m.parameters(), lr=0.1, lars_trust=TRUST)
    o3.load_state_dict(sd)
    assert o3._lars_conf() is None and o3.lars_stats() is None
    o3.step()


# ---------------------------------------------------------------- 6. interface
def test_build_optimizer_and_adam():
    m = _lenet()
    o = build_optimizer("lars", m.parameters(), 0.1, weight_decay=WD)
    g0 = o.param_groups[0]
    assert isinstance(o, SGD) and g0["lars_trust"] == 0.001 and g0["lars_eps"] == 1e-8 and g0["lars_exclude_1d"] is True
    assert g0["momentum"] == 0.9 and not o.supports_ranges()
    assert build_optimizer("lars", m.parameters(), 0.1, lars_trust=0.01).param_groups[0]["lars_trust"] == 0.01
    assert build_optimizer("sgd", m.parameters(), 0.1).lars_stats() is None
    assert SGD(m.parameters(), lr=0.1).param_groups[0]["lars_trust"] is None
    for name, Opt in (("adam", Adam), ("adamw", AdamW)):
        with pytest.raises(TypeError):
            Opt(m.parameters(), lr=1e-3, lars_trust=0.001)
        with pytest.raises(TypeError):
            build_optimizer(name, m.parameters(), 1e-3, lars_trust=0.001)
    with pytest.raises(ValueError):
        SGD(m.parameters(), lr=0.1, lars_trust=0.0)


# ---------------------------------------------------------------- 7. data parallel (FakeWorld)
def _dp_train(comm, shard, lars, clip, local_weight=None, gossip=0, steps=3, batch=6):
    m = build_model("lenet5")
    m.load_state_dict(INIT)
    ldnn.prepare(m, "cpu")
    dp = DataParallel(m, comm, bucket_cap_mb=0.05, shard_optimizer=shard, local_weight=local_weight, gossip=gossip)
    opt = SGD(m.parameters(), lr=0.05, momentum=0.9, weight_decay=WD, max_grad_norm=clip, lars_trust=lars)
    g = torch.Generator().manual_seed(10 + comm.rank)
    crit = CrossEntropyLoss()
    ratios, want = [], []
    n0 = comm.schedule_digest()[0]
    for _ in range(steps):
        x = torch.randn(batch, 1, 28, 28, generator=g)
        y = torch.randint(0, 10, (batch,), generator=g)
        opt.zero_grad()
        (crit(dp(x), y) * 20.0).backward()
        dp.finish_gradient_sync()
        f = dp.flat
        if lars is not None and not shard:
            # the oracle's ratios from this rank's whole (mixed / averaged) gradient and master
            sq = sum((f.storage_view(s, f.grad).double() * f.grad_scale).square().sum() for s in f.segments)
            c = 1.0 if clip is None else min(1.0, clip / (float(sq.sqrt()) + 1e-6))
            want.append({s.name: _oracle_ratio(s.param, f.storage_view(s, f.grad).double() * f.grad_scale * c, WD)
                         for s in f.segments})
        opt.step()
        if lars is not None:
            st_ = opt.lars_stats()   # (by name: sharding lays the flat buffers out in another order)
            ratios.append(dict(zip(st_["names"], st_["ratio"].tolist())))
    nops = comm.schedule_digest()[0] - n0
    comm.check_schedule("end of test")
    dp.gather_master(opt)
    st = {k: v.clone() for k, v in m.state_dict().items()}
    return st, ratios, want, nops


@pytest.mark.parametrize("clip", [None, 1.0])
def test_sharded_lars_equals_unsharded(clip):
    """Tolerance: tests/test_grad_clip.py::test_sharded_clipping_equals_unsharded's."""
    N = 3
    sh = FakeWorld(N).run(_dp_train, True, TRUST, clip)
    ref = FakeWorld(N).run(_dp_train, False, TRUST, clip)
    for r in range(N):
        for k, v in ref[r][0].items():
            torch.testing.assert_close(sh[r][0][k].float(), v.float(), rtol=1e-5, atol=1e-6, msg=k)
        for step in range(3):
            assert sh[r][1][step] == sh[0][1][step]            # every rank finalizes the same ratios
            for n, v in ref[0][2][step].items():
                assert sh[r][1][step][n] == pytest.approx(v, rel=1e-5), (step, n)
                assert ref[r][1][step][n] == pytest.approx(v, rel=1e-5), (step, n)
    assert any(v != 1.0 for v in sh[0][1][0].values())


@pytest.mark.parametrize("kw", [dict(local_weight=0.7), dict(gossip=1)])
def test_weighted_mix_and_gossip_adapt_to_their_own_gradient(kw):
    N = 3
    res = FakeWorld(N).run(_dp_train, False, TRUST, None, **kw)
    for r in range(N):
        for step in range(3):
            for n, v in res[r][2][step].items():
                assert res[r][1][step][n] == pytest.approx(v, rel=1e-5), (step, n)
    assert res[0][1][0] != res[1][1][0]     # per-rank ratios


def test_sharded_lars_adds_one_all_reduce_per_step():
    N, steps = 3, 3
    off = FakeWorld(N).run(_dp_train, True, None, None)
    lars = FakeWorld(N).run(_dp_train, True, TRUST, None)
    both = FakeWorld(N).run(_dp_train, True, TRUST, 1.0)
    unsh_off = FakeWorld(N).run(_dp_train, False, None, None)
    unsh_on = FakeWorld(N).run(_dp_train, False, TRUST, 1.0)
    for r in range(N):
        assert lars[r][3] - off[r][3] == steps     # exactly one more collective per step (check_schedule passed)
        assert both[r][3] - off[r][3] == steps     # ... and clipping's sum rides in the same vector
        assert unsh_on[r][3] == unsh_off[r][3]     # the unsharded path needs none


# ---------------------------------------------------------------- 8. CLI
def test_cli_parser_and_engine_resolution(monkeypatch):
    from ldnn import cli
    from ldnn.models.mlp import mlp2

    d = cli.build_parser().parse_args([])
    assert d.lars_trust == 0.001 and d.lars_eps == 1e-8 and d.lars_adapt_1d is False
    model, dev = mlp2(), torch.device("cpu")
    monkeypatch.setattr(cli, "native_gpu", lambda d: True)   # (as on a GPU host with the extension)
    a = cli.build_parser().parse_args(["--engine", "static", "--optimizer", "lars"])
    with pytest.raises(SystemExit, match="--optimizer lars runs on the autograd path"):
        cli.resolve_engine(a, model, dev, 1)
    a.engine = "auto"
    assert cli.resolve_engine(a, model, dev, 1) is False
    a.optimizer = "sgd"
    assert cli.resolve_engine(a, model, dev, 1) is True


KEYS = {"lars_ratio_min", "lars_ratio_median", "lars_ratio_max"}


@pytest.mark.parametrize("optimizer", ["lars", "sgd"])
def test_cli_metrics_fields(tmp_path, optimizer):
    from ldnn.cli import main

    main(["--model", "mlp2", "--dataset", "mnist", "--n_train", "400", "--n_test", "80", "--epochs_global", "1",
          "--epochs_local", "1", "--device", "cpu", "--quiet", "--out_dir", str(tmp_path), "--plots", "", "--no_eval",
          "--optimizer", optimizer, "--lr", "0.05", "--lars_trust", "0.01", "--weight_decay", "1e-4"])
    recs = [json.loads(l) for l in open(tmp_path / "metrics.rank0.jsonl")]
    ge = [r for r in recs if r.get("kind") == "global_epoch"]
    assert ge
    for r in ge:
        if optimizer == "sgd":
            assert not (KEYS & set(r))
        else:
            assert KEYS <= set(r)
            assert 0 < r["lars_ratio_min"] <= r["lars_ratio_median"] <= r["lars_ratio_max"] and r["lars_ratio_min"] != 1


def _port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


@pytest.mark.slow
def test_cli_two_gloo_ranks_sharded_equals_unsharded(tmp_path):
    """train.py --sync_every step --optimizer lars on 2 gloo ranks, mlp2: replicas bitwise equal,
    and the sharded optimizer gives the replicated one's weights (tolerance of
    tests/test_grad_clip.py::test_cli_two_gloo_ranks_sharded_equals_unsharded)."""
    finals = {}
    for mode in ("on", "off"):
        out = tmp_path / mode
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
               "--master-port", str(_port()), os.path.join(ROOT, "train.py"), "--model", "mlp2", "--dataset", "mnist",
               "--n_train", "600", "--n_test", "100", "--epochs_global", "1", "--epochs_local", "1", "--device", "cpu",
               "--quiet", "--out_dir", str(out), "--plots", "", "--sync_every", "step", "--shard_optimizer", mode,
               "--optimizer", "lars", "--lars_trust", "0.01", "--weight_decay", "1e-4", "--lr", "0.05",
               "--checkpoint_every", "1", "--no_eval", "--bucket_mb", "0.05", "--no_repartition",
               "--partition_rule", "equal", "--log_weights_digest"]
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
    for k, v in finals["off"].items():
        torch.testing.assert_close(finals["on"][k].float(), v.float(), rtol=1e-5, atol=1e-6, msg=k)
