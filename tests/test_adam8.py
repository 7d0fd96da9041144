"""Adam8bit (optim/optimizers.py; csrc/kernels/optim_q.hip), CPU paths: the torch twin ``_adam8_torch``
one step at a time against fp64, the stochastic rounding through the optimizer, a least-squares run beside
torch's Adam, and the sharded step under gloo.  ``one_step_case`` / ``drift_case`` / ``lsq_case`` are
also what tests/test_adam8_gpu.py runs on the kernel."""
import math
import os
import subprocess
import sys

import pytest
import torch

import ldnn
from ldnn.models.mlp import MLP
from ldnn.ops._ext import C
from ldnn.optim import Adam8bit, AdamW8bit, build_optimizer

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LR, B1, B2, EPS, GS, SEED = 1e-3, 0.9, 0.999, 1e-8, 0.5, 5
BIG = 4 * 256 * 3 + 5      # blocks: three sweeps of a 2-workgroup grid under set_opt_max_blocks(2) and a partial wave
INSTANCES = {"plain": {}, "clip": dict(coef=0.25), "prox": dict(mu=0.1), "coupled": dict(wd=0.1),
             "decoupled": dict(wd=0.1, decoupled=True)}


def _dec(codes, scale):
    return codes.cpu().view(torch.float8_e4m3fn).double().view(-1, 64) * scale.cpu().double().view(-1, 1)


def ref64(w, g, m0, s0, a, t, wd=0.0, decoupled=False, mu=0.0):
    """Steps 1-5 of one Adam8bit step in fp64 from the decoded state (m0, s0); returns (w, m, s)."""
    px = mu * (w - a)
    if wd != 0:
        if decoupled:
            w = w * (1 - LR * wd)
        else:
            g = g + wd * w
    g = g + px
    m = B1 * m0 + (1 - B1) * g
    v = torch.maximum(B2 * s0 * s0 + (1 - B2) * g * g, m * m * ((1 - B2) / (1 - B1)))
    s = v.sqrt()
    return w - (LR / (1 - B1 ** t)) * m / (s / math.sqrt(1 - B2 ** t) + EPS), m, s


def one_step_case(dev, nblk, coef=None, mu=0.0, wd=0.0, decoupled=False):
    """Three steps over ``nblk`` blocks, each against ``ref64`` from the state it started from (decoded on the
    host).  Block 1 is all zero, block 2's gradient spans eight decades.  cuda: ``adam8_step``; cpu: the twin."""
    n = nblk * 64
    gen = torch.Generator().manual_seed(nblk)
    w, a = torch.randn(n, generator=gen), torch.randn(n, generator=gen)
    grads = [torch.randn(n, generator=gen) for _ in range(3)]
    if nblk > 2:
        w[64:128], a[64:128] = 0, 0
        for g in grads:
            g[64:128] = 0
            g[128:192] *= 10.0 ** (-8 * torch.rand(64, generator=gen))
    w, a = w.to(dev), a.to(dev)
    mq, sq = (torch.zeros(n, dtype=torch.uint8, device=dev) for _ in range(2))
    ms, ss = (torch.zeros(nblk, device=dev) for _ in range(2))
    sh = torch.zeros(n, dtype=torch.bfloat16, device=dev) if dev == "cuda" else None
    c = 1.0 if coef is None else coef
    opt = (AdamW8bit if decoupled else Adam8bit)([torch.nn.Parameter(torch.zeros(1))])
    for t in (1, 2, 3):
        g = grads[t - 1].to(dev)
        ew, em, es = ref64(w.cpu().double(), g.cpu().double() * GS * c, _dec(mq, ms).view(-1), _dec(sq, ss).view(-1),
                           a.cpu().double(), t, wd, decoupled, mu)
        if dev == "cuda":
            hp = torch.tensor([LR, float(t)], device=dev)
            clip = None if coef is None else torch.tensor([1.0, coef, 0, 0, 0, 0, 0, 0], device=dev)
            prox = (a, torch.tensor([mu, 0, 0, 0], device=dev)) if mu else None
            C().adam8_step(w, g, mq, sq, ms, ss, sh, hp, GS, B1, B2, EPS, wd, decoupled, SEED, 0, clip=clip, prox=prox)
        else:
            opt._adam8_torch(w, g * GS * c, mq, sq, ms, ss, t, LR, B1, B2, EPS, wd, SEED, 0,
                             prox=mu * (w - a) if mu else None)
        torch.testing.assert_close(w.cpu(), ew.float(), rtol=1e-5, atol=1e-6)
        if sh is not None:
            assert torch.equal(sh.view(torch.int16), w.bfloat16().view(torch.int16))
        for name, x, codes, scale in (("m", em, mq, ms), ("s", es, sq, ss)):
            x = x.view(-1, 64)
            amax = x.abs().amax(1, keepdim=True)
            torch.testing.assert_close(scale.cpu(), (amax / 448).float().view(-1), rtol=2e-6, atol=0, msg=f"{name} scale")
            y = torch.where(amax > 0, x * (448 / amax), torch.zeros_like(x))
            got = codes.cpu().view(torch.float8_e4m3fn).double().view(-1, 64)
            assert bool(torch.isfinite(got).all()), name
            spacing = torch.exp2(torch.floor(torch.log2(y.abs().clamp(min=2.0 ** -6))) - 3)
            err = (got - y).abs() - (spacing + 16 * 2.0 ** -24 * y.abs())
            assert bool((err <= 0).all()), (name, t, err.max().item())
        assert bool((w[64:128] == 0).all()) or nblk <= 2


@pytest.mark.parametrize("inst", list(INSTANCES))
@pytest.mark.parametrize("nblk", [1, 5, BIG])
def test_twin_one_step_matches_fp64(nblk, inst):
    one_step_case("cpu", nblk, **INSTANCES[inst])


def _linear(dev, nin, nout, seed=0):
    torch.manual_seed(seed)
    m = MLP(nin, (), nout)
    ldnn.prepare(m, dev)
    return m


def drift_case(dev):
    """64 blocks, one eager step on a random gradient, then 200 on a zero one: round-to-nearest would leave
    the mean of s at exactly 1 x, stochastic rounding follows b2^100 = 0.905."""
    m = _linear(dev, 64, 64)
    o = Adam8bit(m.parameters(), lr=1e-4, betas=(0.9, 0.999), seed=3)
    f = o._flat_for_group(o.param_groups[0])
    f.grad.copy_(torch.randn(f.numel, generator=torch.Generator().manual_seed(1)))
    o.step()
    before = _dec(o._ls()["exp_avg_sq_q"], o._ls()["exp_avg_sq_scale"])
    for _ in range(200):
        f.grad.zero_()
        o.step()
    after = _dec(o._ls()["exp_avg_sq_q"], o._ls()["exp_avg_sq_scale"])
    ratio = (after.mean() / before.mean()).item()
    print(f"mean s after / before 200 zero-gradient steps: {ratio:.4f}")
    assert o._ls()["step"] == 201 and abs(ratio - 0.905) <= 0.02, ratio


def test_rounding_is_stochastic():
    drift_case("cpu")


def lsq_case(dev, seed):
    """Least squares, 2048 parameters (the first elements of a flat buffer), 300 steps: final loss of
    Adam8bit's flat step (cuda: the kernel) over torch.optim.Adam's in fp32, same data and start."""
    gen = torch.Generator().manual_seed(100 + seed)
    x, y = torch.randn(256, 64, generator=gen).to(dev), torch.randn(256, 32, generator=gen).to(dev)
    w0 = (0.1 * torch.randn(32, 64, generator=gen)).to(dev)

    def grad(w):
        r = w @ x.t() - y.t()
        return r.square().mean(), (2.0 / r.numel()) * (r @ x)

    o = Adam8bit(_linear(dev, 64, 32).parameters(), lr=LSQ_LR, seed=seed)
    f = o._flat_for_group(o.param_groups[0])
    f.master.zero_()
    f.master[:2048] = w0.reshape(-1)
    w = torch.nn.Parameter(w0.clone())
    ref = torch.optim.Adam([w], lr=LSQ_LR)
    for _ in range(300):
        f.grad.zero_()
        f.grad[:2048] = grad(f.master[:2048].view(32, 64))[1].reshape(-1)
        o.step()
        w.grad = grad(w.detach())[1]
        ref.step()
    return (grad(f.master[:2048].view(32, 64))[0] / grad(w.detach())[0]).item()


# (lr 1e-3: neither run has converged, the ratio sees the trajectory.)  The twin's ratios, seeds 0..4, CPU:
LSQ_LR = 1e-3
LSQ_MEASURED = (1.000322, 0.999963, 1.000097, 1.000035, 0.999958)


@pytest.mark.parametrize("seed", range(5))
def test_still_optimises_least_squares(seed):
    """Final-loss ratio against torch.optim.Adam.  Measured on the CPU twin for seeds 0..4: 1.000322,
    0.999963, 1.000097, 1.000035, 0.999958 (LSQ_MEASURED).  The bound is twice the worst of them; the margin
    covers the seed-to-seed spread of the rounding noise."""
    r = lsq_case("cpu", seed)
    print(f"seed {seed}: final loss ratio {r:.6f}")
    assert r <= 2 * max(LSQ_MEASURED)


def test_interface_and_state_dict():
    m = _linear("cpu", 64, 64)
    o = build_optimizer("adamw8bit", m.parameters(), 1e-3, weight_decay=0.1, max_grad_norm=1.0, seed=7)
    assert isinstance(o, AdamW8bit) and o.param_groups[0]["seed"] == 7 and o.param_groups[0]["weight_decay"] == 0.1
    assert type(build_optimizer("adam8bit", m.parameters(), 1e-3)) is Adam8bit
    with pytest.raises(ValueError, match="seed"):
        Adam8bit(m.parameters(), seed=-1)
    f = o._flat_for_group(o.param_groups[0])
    f.grad.copy_(torch.randn(f.numel, generator=torch.Generator().manual_seed(2)))
    o.step()
    ls, n = o._ls(), f.numel
    assert (ls["exp_avg_q"].dtype, ls["exp_avg_q"].shape, ls["exp_avg_scale"].shape) == (torch.uint8, (n,), (n // 64,))
    flat = o.state_dict()["ldnn_flat_state"]
    assert sorted(flat) == ["exp_avg_q", "exp_avg_scale", "exp_avg_sq_q", "exp_avg_sq_scale", "seed", "step"]
    assert flat["seed"] == 7 and flat["step"] == 1


@pytest.mark.parametrize("name", ["adam8bit", "adamw8bit"])
def test_cli_static_engine_refuses_and_auto_falls_back(monkeypatch, name):
    from ldnn import cli

    monkeypatch.setattr(cli, "native_gpu", lambda d: True)   # (as on a GPU host with the extension)
    a = cli.build_parser().parse_args(["--engine", "static", "--optimizer", name])
    with pytest.raises(SystemExit, match=f"--optimizer {name} runs on the autograd path"):
        cli.resolve_engine(a, MLP(70, (33,), 10), torch.device("cpu"), 1)
    a.engine = "auto"
    assert cli.resolve_engine(a, MLP(70, (33,), 10), torch.device("cpu"), 1) is False


# ---------------------------------------------------------------- sharded, 2 gloo ranks
CAP_MB = 0.005


def _sharded_run(comm):
    """Two steps; ``comm`` None: one process, no DataParallel, the flat buffer in the 2-rank sharded layout
    (the rounding bits follow the absolute flat index)."""
    from ldnn.models import CrossEntropyLoss
    from ldnn.parallel.ddp import DataParallel, _shard_layout, ensure_flat

    torch.manual_seed(0)
    m = MLP(64, (32,), 10)
    ldnn.prepare(m, "cpu")
    if comm is None:
        _shard_layout(m, ensure_flat(m), 2, int(CAP_MB * (1 << 20) / 4))
        fwd, kinds = m, None
    else:
        fwd = DataParallel(m, comm, bucket_cap_mb=CAP_MB, shard_optimizer=True)
        kinds = [b["sharded"] for b in fwd.bucketer.buckets]
    o = Adam8bit(m.parameters(), lr=1e-3, seed=9)
    gen = torch.Generator().manual_seed(4)
    crit = CrossEntropyLoss()
    for _ in range(2):
        x, y = torch.randn(8, 64, generator=gen), torch.randint(0, 10, (8,), generator=gen)
        o.zero_grad()
        crit(fwd(x), y).backward()    # (every rank the same batch: the average is the single-process gradient)
        if comm is not None:
            fwd.finish_gradient_sync()
        o.step()
    if comm is not None:
        fwd.gather_master(o)
    return {k: v.clone() for k, v in o._ls().items() if torch.is_tensor(v) and k.startswith("exp_avg")}, kinds


def _gloo_worker(rank, port, out):
    import torch.distributed as dist

    from ldnn.parallel.comm import default_comm

    dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", rank=rank, world_size=2)
    torch.save(_sharded_run(default_comm()), out)
    dist.destroy_process_group()


def test_sharded_two_ranks_gloo_equals_single_process(tmp_path):
    """Two sharded steps on 2 gloo ranks + ``gather_master(optimizer)``: codes and scales on both ranks are
    the single-process run's, bit for bit."""
    from test_sharded_dp import _port

    port = _port()
    procs = [subprocess.Popen([sys.executable, "-c",
                               f"import sys; sys.path[:0] = [{ROOT!r}, {os.path.join(ROOT, 'tests')!r}]; "
                               f"import test_adam8 as t; t._gloo_worker({r}, {port}, {str(tmp_path / f'r{r}.pt')!r})"])
             for r in range(2)]
    assert [p.wait(timeout=120) for p in procs] == [0, 0]
    ref, _ = _sharded_run(None)
    assert sorted(ref) == ["exp_avg_q", "exp_avg_scale", "exp_avg_sq_q", "exp_avg_sq_scale"]
    for r in range(2):
        got, gk = torch.load(tmp_path / f"r{r}.pt")
        assert gk[-1] is False and any(gk)
        for k, v in ref.items():
            assert torch.equal(got[k], v) and bool((v != 0).any()), (r, k)
