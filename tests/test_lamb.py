"""LAMB (optim/optimizers.py Lamb), CPU paths: the torch-op fallback against an oracle written out
here (per-tensor fp64 moments, direction and norms from the same fp32 gradients), its edge
cases, clipping + LAMB, the state_dict round trip, sharded == unsharded under FakeWorld with
exactly one (with clipping: two) extra all-reduce per step, and the CLI (--optimizer lamb)."""
import json
import os
import socket
import subprocess
import sys

import pytest
import torch

import ldnn
from ldnn.models import CrossEntropyLoss, build_model, xavier_init
from ldnn.optim import SGD, Adam, AdamW, Lamb, build_optimizer
from ldnn.optim.optimizers import lamb_chunk_table
from ldnn.parallel.comm import FakeWorld
from ldnn.parallel.ddp import DataParallel

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LR, B1, B2, EPS, WD = 1e-2, 0.9, 0.999, 1e-6, 1e-2


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


class _Oracle:
    """The issue's formulas per tensor in fp64 (weights, moments, direction, norms), fed the fp32
    gradients the model under test computed (Adam's normalised direction amplifies a last-bit
    difference between two models' gradients, so the oracle takes the very same ones)."""

    def __init__(self, model, lr=LR, wd=WD, eps=EPS, exclude_1d=True, max_norm=None):
        self.model, self.lr, self.wd, self.eps, self.excl, self.max_norm = model, lr, wd, eps, exclude_1d, max_norm
        self.w = {n: p.detach().double().clone() for n, p in model.named_parameters()}
        self.m = {n: torch.zeros_like(v) for n, v in self.w.items()}
        self.v = {n: torch.zeros_like(v) for n, v in self.w.items()}
        self.t = 0

    def step(self):
        """One step from the model's current .grad (call it before the optimizer's step)."""
        grads = {n: p.grad.detach().clone() for n, p in self.model.named_parameters()}
        if self.max_norm is not None:
            tmp = [torch.nn.Parameter(torch.zeros_like(g)) for g in grads.values()]
            for t, g in zip(tmp, grads.values()):
                t.grad = g
            torch.nn.utils.clip_grad_norm_(tmp, self.max_norm)      # (clips the clones in place)
        self.t += 1
        out = {}
        for n, p in self.model.named_parameters():
            g, w = grads[n].double(), self.w[n]
            self.m[n] = B1 * self.m[n] + (1 - B1) * g
            self.v[n] = B2 * self.v[n] + (1 - B2) * g * g
            u = (self.m[n] / (1 - B1 ** self.t)) / ((self.v[n] / (1 - B2 ** self.t)).sqrt() + self.eps) + self.wd * w
            wn, un = w.norm().item(), u.norm().item()
            r = wn / un if (wn > 0 and un > 0 and not (self.excl and p.dim() < 2)) else 1.0
            out[n] = (r, wn, un)
            self.w[n] = w - self.lr * r * u
        return out

    def check_weights(self):
        for n, p in self.model.named_parameters():
            torch.testing.assert_close(p.detach(), self.w[n].float(), rtol=1e-5, atol=1e-6, msg=n)


def _stats_by_name(o, m):
    st = o.lamb_stats()
    if st["names"] and st["names"][0].startswith("param"):   # per-tensor path: parameter order
        names = [n for n, _ in m.named_parameters()]
    else:
        names = st["names"]
    return {n: (float(st["ratio"][i]), float(st["w_norm"][i]), float(st["u_norm"][i])) for i, n in enumerate(names)}


def _backward(mod, opt, x, y, scale=1.0):
    opt.zero_grad()
    (torch.nn.functional.cross_entropy(mod(x), y) * scale).backward()


# ---------------------------------------------------------------- 1. oracle
@pytest.mark.parametrize("flat", [True, False])
def test_lamb_steps_match_the_oracle(flat):
    """5 steps of LeNet-5 (1-D and 4-D tensors, the padded 10-row head), batch 8, weight decay
    1e-2.  Ratios and norms within 1e-5 relative of the fp64 oracle (measured maximum on the
    flat path: 1.0e-7), weights within rtol 1e-5 / atol 1e-6."""
    m = _lenet(flat)
    o, ora = Lamb(m.parameters(), lr=LR, weight_decay=WD), _Oracle(m)
    g = torch.Generator().manual_seed(1)
    worst = 0.0
    for _ in range(5):
        x, y = _batch(g)
        _backward(m, o, x, y)
        want = ora.step()
        o.step()
        got = _stats_by_name(o, m)
        for n, v in want.items():
            for a, b in zip(got[n], v):
                assert a == pytest.approx(b, rel=1e-5), n
                worst = max(worst, abs(a - b) / abs(b) if b else abs(a))
    print(f"lamb ratios / norms worst relative error {worst:.3e}")
    assert any(v[0] != 1.0 for v in want.values())
    assert all(v[0] == 1.0 for n, v in want.items() if dict(m.named_parameters())[n].dim() < 2)
    ora.check_weights()
    if flat:
        assert sorted(k for k in o._ls() if k not in ("lamb", "hp")) == ["exp_avg", "exp_avg_sq", "step"]
        assert not o.supports_ranges() and o.range_updater() is None


# ---------------------------------------------------------------- 2. edge cases
@pytest.mark.parametrize("flat", [True, False])
def test_zero_gradient_zero_tensor_and_1d_tensors(flat):
    m = _lenet(flat)
    zero_g = "fc2.weight"
    o, ora = Lamb(m.parameters(), lr=LR, weight_decay=WD), _Oracle(m)
    g = torch.Generator().manual_seed(3)
    # step 1 builds moments; in step 2 one tensor's gradient is zero: it still moves (m, v != 0)
    for step in range(2):
        x, y = _batch(g)
        _backward(m, o, x, y)
        if step == 1:
            dict(m.named_parameters())[zero_g].grad.zero_()
        before = dict(m.named_parameters())[zero_g].detach().clone()
        want = ora.step()
        o.step()
    got = _stats_by_name(o, m)
    assert not torch.equal(dict(m.named_parameters())[zero_g].detach(), before)
    for n, v in want.items():
        assert got[n][0] == pytest.approx(v[0], rel=1e-5), n
    assert got[zero_g][0] != 1.0 and got[zero_g][2] > 0
    ora.check_weights()
    if flat:
        # the padded rows of the head ([10] -> padded storage) stay zero in master and moments
        f = o._flat_for_group(o.param_groups[0])
        padded = 0
        for buf in (f.master, o._ls()["exp_avg"], o._ls()["exp_avg_sq"]):
            for s in f.segments:
                sv = f.storage_view(s, buf)
                if sv.shape[0] > s.param.shape[0]:
                    padded += 1
                    assert bool((sv[s.param.shape[0]:] == 0).all()), s.name
                    assert bool((sv[:s.param.shape[0]] != 0).any()), s.name
        assert padded >= 3      # (the 10-row head is stored with padded rows)
    # lamb_exclude_1d=False adapts the 1-D tensors; an all-zero tensor keeps ratio 1
    m2 = _lenet(flat)
    with torch.no_grad():
        dict(m2.named_parameters())["fc3.bias"].zero_()
        dict(m2.named_parameters())["fc2.bias"].fill_(0.1)
    o2 = Lamb(m2.parameters(), lr=LR, weight_decay=WD, lamb_exclude_1d=False)
    ora2 = _Oracle(m2, exclude_1d=False)
    x, y = _batch(g)
    _backward(m2, o2, x, y)
    want = ora2.step()
    o2.step()
    got2 = _stats_by_name(o2, m2)
    for n, v in want.items():
        assert got2[n][0] == pytest.approx(v[0], rel=1e-5), n
    assert got2["fc3.bias"][0] == 1.0 and got2["fc3.bias"][1] == 0.0 and got2["fc3.bias"][2] > 0
    assert got2["fc2.bias"][0] != 1.0
    assert all(o2.lamb_stats()["adapted"])


# ---------------------------------------------------------------- 3. clipping + LAMB
@pytest.mark.parametrize("flat", [True, False])
def test_clipping_and_lamb_match_the_oracle(flat):
    """clip_grad_norm_ first, the moments from the clipped gradient; then a non-finite gradient
    skips the step: weights, moments, counters and lamb_stats() stay."""
    max_norm = 1.0
    m = _lenet(flat)
    o = Lamb(m.parameters(), lr=LR, weight_decay=WD, max_grad_norm=max_norm)
    ora = _Oracle(m, max_norm=max_norm)
    g = torch.Generator().manual_seed(4)
    for s in (1.0, 20.0, 1.0, 20.0):
        x, y = _batch(g)
        _backward(m, o, x, y, s)
        want = ora.step()
        o.step()
        got = _stats_by_name(o, m)
        for n, v in want.items():
            assert got[n][0] == pytest.approx(v[0], rel=1e-5), n
    assert int(o.grad_clip_stats()["clipped"]) >= 1 and int(o.grad_clip_stats()["steps"]) == 4
    ora.check_weights()
    st = o.lamb_stats()
    stats_before = {k: st[k].clone() for k in ("ratio", "w_norm", "u_norm")}
    before = [p.detach().clone() for p in m.parameters()]
    state_before = {k: v.clone() for k, v in o._ls().items() if torch.is_tensor(v) and k.startswith("exp")}
    per_tensor = {k: {a: (b.clone() if torch.is_tensor(b) else b) for a, b in v.items()} for k, v in o.state.items()}
    step_before = o.state_dict()["ldnn_flat_state"].get("step")
    x, y = _batch(g)
    _backward(m, o, x, y)
    next(iter(m.parameters())).grad.view(-1)[3] = float("inf")
    o.step()
    assert int(o.grad_clip_stats()["skipped"]) == 1
    for p, q in zip(m.parameters(), before):
        assert torch.equal(p.detach(), q)
    for k, v in state_before.items():
        assert torch.equal(o._ls()[k], v), k
    for k, v in per_tensor.items():
        for a, b in v.items():
            assert torch.equal(o.state[k][a], b) if torch.is_tensor(b) else o.state[k][a] == b, a
    assert o.state_dict()["ldnn_flat_state"].get("step") == step_before
    st = o.lamb_stats()
    for k, v in stats_before.items():
        assert torch.equal(st[k], v), k


# ---------------------------------------------------------------- 4. state_dict
@pytest.mark.parametrize("clip", [None, 1.0])
def test_state_dict_round_trip_continues_bit_for_bit(clip):
    ma, mb = _lenet(), _lenet()
    oa = Lamb(ma.parameters(), lr=LR, weight_decay=WD, max_grad_norm=clip)
    g = torch.Generator().manual_seed(5)
    batches = [_batch(g) for _ in range(5)]
    for x, y in batches[:2]:
        _backward(ma, oa, x, y, 20.0)
        oa.step()
    sd = oa.state_dict()
    assert sorted(sd["ldnn_flat_state"]) == ["exp_avg", "exp_avg_sq", "step"] and sd["ldnn_flat_state"]["step"] == 2
    mb.load_state_dict(ma.state_dict())
    ob = Lamb(mb.parameters(), lr=0.5)
    ob.load_state_dict(sd)
    assert ob.param_groups[0]["lr"] == LR and ob._lamb_conf() is True
    for x, y in batches[2:]:
        for mod, opt in ((ma, oa), (mb, ob)):
            _backward(mod, opt, x, y, 20.0)
            opt.step()
    fa, fb = (o._flat_for_group(o.param_groups[0]) for o in (oa, ob))
    assert torch.equal(fa.master, fb.master)
    for k in ("exp_avg", "exp_avg_sq"):
        assert torch.equal(oa._ls()[k], ob._ls()[k])
    assert oa.state_dict()["ldnn_flat_state"]["step"] == ob.state_dict()["ldnn_flat_state"]["step"] == 5


# ---------------------------------------------------------------- 5. interface
def test_build_optimizer_and_keyword_refusals():
    m = _lenet()
    o = build_optimizer("lamb", m.parameters(), 1e-3, weight_decay=WD, max_grad_norm=1.0)
    g0 = o.param_groups[0]
    assert isinstance(o, Lamb) and g0["lamb_exclude_1d"] is True and g0["eps"] == 1e-6 and g0["betas"] == (0.9, 0.999)
    assert g0["weight_decay"] == WD and g0["max_grad_norm"] == 1.0 and not o.supports_ranges()
    assert o.lars_stats() is None and o.lamb_stats() is not None
    assert build_optimizer("lamb", m.parameters(), 1e-3, lamb_exclude_1d=False).param_groups[0]["lamb_exclude_1d"] is False
    for name in ("sgd", "lars", "adam", "adamw"):
        with pytest.raises(TypeError):
            build_optimizer(name, m.parameters(), 1e-3, lamb_exclude_1d=False)
        assert build_optimizer(name, m.parameters(), 1e-3).lamb_stats() is None
    for kw in (dict(lars_trust=0.01), dict(lars_eps=1e-6), dict(lars_exclude_1d=False)):
        with pytest.raises(TypeError):
            build_optimizer("lamb", m.parameters(), 1e-3, **kw)
    for Opt in (SGD, Adam, AdamW):
        with pytest.raises(TypeError):
            Opt(m.parameters(), lr=1e-3, lamb_exclude_1d=True)


def test_chunk_table_counted_flags():
    bounds = [(0, 256), (256, 8192 + 256), (8512, 8576)]
    chunks, segs = lamb_chunk_table(bounds, [(0, 4096), (8512, 8576)], [(128, 1024)], 4096)
    assert segs[0] == (0, 2) and chunks[0] == (0, 2, 4, 1) and chunks[1] == (0, 0, 2, 0)
    s1 = chunks[segs[1][0]:segs[1][1]]
    assert s1 == [(1, 4, 16, 1), (1, 16, 64, 0)]
    assert chunks[segs[2][0]:segs[2][1]] == [(2, 133, 134, 0)]
    # every element of the ranges is covered exactly once, counted exactly inside the counted set
    cover = torch.zeros(8576 // 64, dtype=torch.int64)
    for _, b, e, c in chunks:
        cover[b:e] += 1
        assert c == int(128 <= b * 64 and e * 64 <= 1024)
    assert cover[:64].tolist() == [1] * 64 and int(cover[64:133].sum()) == 0 and int(cover[133]) == 1
    with pytest.raises(ValueError, match="64-element aligned"):
        lamb_chunk_table(bounds, [(0, 100)], [], 4096)
    with pytest.raises(ValueError, match="64-element aligned"):
        lamb_chunk_table(bounds, [(0, 128)], [(0, 32)], 4096)


# ---------------------------------------------------------------- 6. data parallel (FakeWorld)
def _dp_train(comm, shard, lamb, clip, local_weight=None, gossip=0, steps=3, batch=6):
    m = build_model("lenet5")
    m.load_state_dict(INIT)
    ldnn.prepare(m, "cpu")
    dp = DataParallel(m, comm, bucket_cap_mb=0.05, shard_optimizer=shard, local_weight=local_weight, gossip=gossip)
    opt = (Lamb(m.parameters(), lr=LR, weight_decay=WD, max_grad_norm=clip) if lamb else
           Adam(m.parameters(), lr=LR, weight_decay=WD, max_grad_norm=clip))
    g = torch.Generator().manual_seed(10 + comm.rank)
    crit = CrossEntropyLoss()
    ratios = []
    n0 = comm.schedule_digest()[0]
    for _ in range(steps):
        x = torch.randn(batch, 1, 28, 28, generator=g)
        y = torch.randint(0, 10, (batch,), generator=g)
        opt.zero_grad()
        (crit(dp(x), y) * 20.0).backward()
        dp.finish_gradient_sync()
        opt.step()
        if lamb:
            st_ = opt.lamb_stats()   # (by name: sharding lays the flat buffers out in another order)
            ratios.append(dict(zip(st_["names"], st_["ratio"].tolist())))
    nops = comm.schedule_digest()[0] - n0
    comm.check_schedule("end of test")
    dp.gather_master(opt)
    st = {k: v.clone() for k, v in m.state_dict().items()}
    return st, ratios, nops


@pytest.mark.parametrize("clip", [None, 1.0])
@pytest.mark.parametrize("world", [2, 3])
def test_sharded_lamb_equals_unsharded(world, clip):
    """Tolerance: tests/test_lars.py::test_sharded_lars_equals_unsharded's."""
    sh = FakeWorld(world).run(_dp_train, True, True, clip)
    ref = FakeWorld(world).run(_dp_train, False, True, clip)
    for r in range(world):
        for k, v in ref[r][0].items():
            torch.testing.assert_close(sh[r][0][k].float(), v.float(), rtol=1e-5, atol=1e-6, msg=k)
        for step in range(3):
            assert sh[r][1][step] == sh[0][1][step]            # every rank finalizes the same ratios
            for n, v in ref[0][1][step].items():
                assert sh[r][1][step][n] == pytest.approx(v, rel=1e-5), (step, n)
    assert any(v != 1.0 for v in sh[0][1][0].values())


def test_sharded_lamb_adds_one_all_reduce_per_step_and_two_with_clipping():
    N, steps = 3, 3
    off = FakeWorld(N).run(_dp_train, True, False, None)
    lamb = FakeWorld(N).run(_dp_train, True, True, None)
    both = FakeWorld(N).run(_dp_train, True, True, 1.0)
    unsh_off = FakeWorld(N).run(_dp_train, False, False, None)
    unsh_on = FakeWorld(N).run(_dp_train, False, True, 1.0)
    for r in range(N):
        assert lamb[r][2] - off[r][2] == steps         # exactly one more collective per step (check_schedule passed)
        assert both[r][2] - off[r][2] == 2 * steps     # clipping's scalar first, then LAMB's vector
        assert unsh_on[r][2] == unsh_off[r][2]         # the unsharded path needs none


@pytest.mark.parametrize("kw", [dict(local_weight=0.7), dict(gossip=1)])
def test_weighted_mix_and_gossip_adapt_to_their_own_gradient(kw):
    res = FakeWorld(3).run(_dp_train, False, True, None, **kw)
    assert res[0][1][0] != res[1][1][0]     # per-rank ratios


# ---------------------------------------------------------------- 7. CLI
def test_cli_parser_and_engine_resolution(monkeypatch):
    from ldnn import cli
    from ldnn.models.mlp import mlp2

    d = cli.build_parser().parse_args([])
    assert d.optimizer == "adam" and d.lamb_adapt_1d is False
    model, dev = mlp2(), torch.device("cpu")
    monkeypatch.setattr(cli, "native_gpu", lambda d: True)   # (as on a GPU host with the extension)
    a = cli.build_parser().parse_args(["--engine", "static", "--optimizer", "lamb", "--lamb_adapt_1d"])
    assert a.lamb_adapt_1d is True
    with pytest.raises(SystemExit, match="--optimizer lamb runs on the autograd path"):
        cli.resolve_engine(a, model, dev, 1)
    a.engine = "auto"
    assert cli.resolve_engine(a, model, dev, 1) is False
    a.optimizer = "adam"
    assert cli.resolve_engine(a, model, dev, 1) is True


KEYS = {"lamb_ratio_min", "lamb_ratio_median", "lamb_ratio_max"}


@pytest.mark.parametrize("optimizer", ["lamb", "adam"])
def test_cli_metrics_fields(tmp_path, optimizer):
    from ldnn.cli import main

    main(["--model", "mlp2", "--dataset", "mnist", "--n_train", "400", "--n_test", "80", "--epochs_global", "1",
          "--epochs_local", "1", "--device", "cpu", "--quiet", "--out_dir", str(tmp_path), "--plots", "", "--no_eval",
          "--optimizer", optimizer, "--lr", "0.001", "--weight_decay", "0.01", "--clip_grad_norm", "1.0"])
    recs = [json.loads(l) for l in open(tmp_path / "metrics.rank0.jsonl")]
    ge = [r for r in recs if r.get("kind") == "global_epoch"]
    assert ge
    for r in ge:
        if optimizer == "adam":
            assert not (KEYS & set(r))
        else:
            assert KEYS <= set(r) and "grad_norm_last" in r
            assert 0 < r["lamb_ratio_min"] <= r["lamb_ratio_median"] <= r["lamb_ratio_max"] and r["lamb_ratio_min"] != 1


def _port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


@pytest.mark.slow
def test_cli_two_gloo_ranks_sharded_equals_unsharded(tmp_path):
    """train.py --sync_every step --optimizer lamb on 2 gloo ranks, mlp2: replicas bitwise equal,
    and the sharded optimizer gives the replicated one's weights (tolerance of
    tests/test_lars.py::test_cli_two_gloo_ranks_sharded_equals_unsharded)."""
    finals = {}
    for mode in ("on", "off"):
        out = tmp_path / mode
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
               "--master-port", str(_port()), os.path.join(ROOT, "train.py"), "--model", "mlp2", "--dataset", "mnist",
               "--n_train", "600", "--n_test", "100", "--epochs_global", "1", "--epochs_local", "1", "--device", "cpu",
               "--quiet", "--out_dir", str(out), "--plots", "", "--sync_every", "step", "--shard_optimizer", mode,
               "--optimizer", "lamb", "--weight_decay", "0.01", "--lr", "0.001", "--clip_grad_norm", "1.0",
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
