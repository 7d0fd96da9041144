"""Global-norm gradient clipping on the GPU: the grad_sumsq / clip_finalize kernels, the fused
SGD / Adam kernels' ``clip=`` form (csrc/kernels/optim.hip), and the clipped step replayed
from hipGraphs (GraphedStep, GraphedDPStep)."""
import hashlib
import os
import socket
import subprocess
import sys

import pytest
import torch

import ldnn
from ldnn.models import CrossEntropyLoss, build_model, xavier_init
from ldnn.ops._ext import C
from ldnn.optim import SGD, Adam
from ldnn.parallel.comm import LocalComm
from ldnn.parallel.ddp import DataParallel
from ldnn.train.graphed import GraphedDPStep, GraphedStep

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

MAXN, COEF, SKIP, NORM, STEPS, CLIPPED, SKIPPED = range(7)
# 4*256*2048 + 4*256 + 3: the first size whose grid-stride loop wraps under the 2048-block cap,
# with a scalar tail
N_WRAP = 2_098_179
SIZES = [1, 3, 4, 5, 255, 1024, 1025, N_WRAP]


def _state(max_norm):
    st = torch.zeros(8, device="cuda")
    st[MAXN] = max_norm
    return st


@pytest.fixture(scope="module")
def big():
    g = torch.Generator(device="cuda").manual_seed(11)
    buf = torch.randn(N_WRAP + 8, device="cuda", generator=g)
    return buf, buf.double().square()   # the reference squares, computed once


def _norm(x, scratch, gs=1.0, max_norm=1.0):
    st = _state(max_norm)
    n = C().grad_sumsq(x, scratch, 0)
    C().clip_finalize(scratch, n, st, gs)
    return st


def test_sumsq_norm_matches_fp64(big):
    """Every size at every element offset 0..3 against grad.double().square().sum(); bound 1e-5
    relative (expected ~1e-7: a thread adds a handful of fp32 squares, the partials meet in
    double).  Measured maximum on MI355X: 6.4e-8.  Two runs give the same bits; garbage in
    the unused scratch slots changes nothing."""
    buf, sq = big
    scratch = torch.zeros(4096, device="cuda")
    worst = 0.0
    for n in SIZES:
        for off in range(4):
            x = buf[off:off + n]
            assert C().grad_sumsq_parts(n) == min(2048, (n + 3) // 4 // 256 + ((n + 3) // 4 % 256 != 0))
            scratch.zero_()
            a = _norm(x, scratch, gs=0.5)
            scratch.fill_(float("nan"))      # garbage everywhere: only the written slots are read
            b = _norm(x, scratch, gs=0.5)
            want = 0.5 * sq[off:off + n].sum().sqrt().item()
            got = a[NORM].item()
            err = abs(got - want) / want
            worst = max(worst, err)
            assert err <= 1e-5, (n, off, got, want)
            assert torch.equal(a[NORM], b[NORM]), (n, off)
            assert a[SKIP].item() == 0 and a[STEPS].item() == 1
            assert a[COEF].item() == pytest.approx(min(1.0, 1.0 / (got + 1e-6)), rel=1e-6)
    print(f"grad_sumsq worst relative norm error {worst:.3e}")


def test_sumsq_ranges_in_consecutive_slots(big):
    """Three ranges (odd offsets and lengths) into consecutive slot runs == one launch over
    their concatenation within 1e-6; sumsq_total + clip_finalize(ext=) gives that norm too."""
    buf, sq = big
    scratch = torch.full((4096,), float("nan"), device="cuda")
    cuts = [(1, 1 + 70_001), (70_002, 70_002 + 5), (70_007, 70_007 + 300_003)]
    slot = 0
    for lo, hi in cuts:
        slot += C().grad_sumsq(buf[lo:hi], scratch, slot)
    st = _state(1.0)
    C().clip_finalize(scratch, slot, st, 1.0)
    one = _norm(buf[1:70_007 + 300_003], torch.zeros(4096, device="cuda"))
    assert abs(st[NORM].item() - one[NORM].item()) <= 1e-6 * one[NORM].item()
    local = torch.zeros(1, device="cuda")
    C().sumsq_total(scratch, slot, local)
    st2 = _state(1.0)
    C().clip_finalize(scratch, 0, st2, 1.0, ext=local)
    assert abs(st2[NORM].item() - one[NORM].item()) <= 1e-6 * one[NORM].item()
    with pytest.raises(RuntimeError, match="do not fit"):
        C().grad_sumsq(buf[:N_WRAP], scratch, 4096 - 2047)


def test_finalize_counters_and_skip():
    scratch = torch.zeros(64, device="cuda")
    st = _state(10.0)
    x = torch.ones(100, device="cuda")
    for x_, mx in ((x, 100.0), (x, 1.0), (x * float("inf"), 1.0), (x, 1.0)):
        st[MAXN] = mx                       # the host writes the threshold, the kernel reads it
        C().clip_finalize(scratch, C().grad_sumsq(x_, scratch, 0), st, 1.0)
    assert st[[STEPS, CLIPPED, SKIPPED]].tolist() == [4.0, 2.0, 1.0]
    assert st[SKIP].item() == 0 and st[NORM].item() == pytest.approx(10.0)
    assert st[COEF].item() == pytest.approx(1.0 / (10.0 + 1e-6))


# ---------------------------------------------------------------- fused optimizer kernels
N_OPT = 8192 + 7
T_BEGIN = 256     # one 64x64 tile inside the range


def _sgd_bufs(seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    p = torch.randn(N_OPT, device="cuda", generator=g)
    return dict(p=p, g=torch.randn(N_OPT, device="cuda", generator=g), m=torch.randn(N_OPT, device="cuda", generator=g),
                sh=p.bfloat16(), t=torch.zeros(64, 64, device="cuda", dtype=torch.bfloat16))


def _sgd(b, clip, tr, nesterov, zero=()):
    hp = torch.tensor([0.1, 0.0], device="cuda")
    kw = dict(t_begin=T_BEGIN, t_out=b["t"]) if tr else {}
    C().sgd_step(b["p"], b["g"], b["m"], b["sh"], hp, 0.5, 0.9, 0.0, 1e-4, nesterov, False, zero_ranges=list(zero),
                 clip=clip, **kw)


def _clone(b):
    return {k: v.clone() for k, v in b.items()}


@pytest.mark.parametrize("tr", [False, True])
@pytest.mark.parametrize("nesterov", [False, True])
def test_fused_sgd_clip(tr, nesterov):
    b0 = _sgd_bufs(21)
    scratch = torch.zeros(64, device="cuda")
    # a huge threshold: bit-identical to the call without clip
    a, b = _clone(b0), _clone(b0)
    _sgd(a, None, tr, nesterov)
    _sgd(b, _norm(b["g"], scratch, gs=0.5, max_norm=1e30), tr, nesterov)
    for k in a:
        assert torch.equal(a[k], b[k]), k
    # a threshold that clips: the torch fp32 formula on the CPU, tolerance of test_kernels_gpu's
    # fused-optimizer tests
    c = _clone(b0)
    st = _norm(c["g"], scratch, gs=0.5, max_norm=1.0)
    assert st[COEF].item() < 0.1
    _sgd(c, st, tr, nesterov)
    p, g, m = b0["p"].cpu(), b0["g"].cpu() * 0.5, b0["m"].cpu()
    g = g * (1.0 / (g.double().norm().float() + 1e-6)).clamp(max=1.0)
    g = g + 1e-4 * p
    m = 0.9 * m + g
    p = p - 0.1 * ((g + 0.9 * m) if nesterov else m)
    torch.testing.assert_close(c["p"].cpu(), p, rtol=1e-5, atol=1e-6)
    torch.testing.assert_close(c["m"].cpu(), m, rtol=1e-5, atol=1e-6)
    assert torch.equal(c["sh"], c["p"].bfloat16())
    if tr:
        assert torch.equal(c["t"], c["p"][T_BEGIN:T_BEGIN + 4096].view(64, 64).t().bfloat16())
    # an inf element: nothing changes but the requested zero range
    d = _clone(b0)
    d["g"][N_OPT - 2] = float("inf")
    st = _norm(d["g"], scratch, gs=0.5, max_norm=1.0)
    assert st[SKIP].item() == 1 and st[SKIPPED].item() == 1
    _sgd(d, st, tr, nesterov, zero=[(3, 5000), (8190, N_OPT)])
    for k in ("p", "m", "sh", "t"):
        assert torch.equal(d[k], b0[k]), k
    want = b0["g"].clone()
    want[N_OPT - 2] = float("inf")
    want[3:5000] = 0
    want[8190:] = 0
    assert torch.equal(d["g"], want)


@pytest.mark.parametrize("decoupled", [False, True])
def test_fused_adam_clip(decoupled):
    g_ = torch.Generator(device="cuda").manual_seed(22)
    n = N_OPT
    b0 = dict(p=torch.randn(n, device="cuda", generator=g_), g=torch.randn(n, device="cuda", generator=g_),
              m=torch.randn(n, device="cuda", generator=g_) * 0.1, v=torch.rand(n, device="cuda", generator=g_) * 0.01,
              hp=torch.tensor([1e-3, 3.0], device="cuda"))
    b0["sh"] = b0["p"].bfloat16()
    scratch = torch.zeros(64, device="cuda")
    wd = 1e-2

    def step(b, clip, zero=()):
        C().bump_step(b["hp"], clip=clip)
        C().adam_step(b["p"], b["g"], b["m"], b["v"], b["sh"], b["hp"], 0.5, 0.9, 0.999, 1e-8, wd, decoupled,
                      zero_ranges=list(zero), clip=clip)

    a, b = _clone(b0), _clone(b0)
    step(a, None)
    step(b, _norm(b["g"], scratch, gs=0.5, max_norm=1e30))
    for k in a:
        assert torch.equal(a[k], b[k]), k
    c = _clone(b0)
    st = _norm(c["g"], scratch, gs=0.5, max_norm=1.0)
    assert st[COEF].item() < 0.1
    step(c, st)
    p, g, m, v = b0["p"].cpu(), b0["g"].cpu() * 0.5, b0["m"].cpu(), b0["v"].cpu()
    g = g * (1.0 / (g.double().norm().float() + 1e-6)).clamp(max=1.0)
    if decoupled:
        p = p * (1 - 1e-3 * wd)
    else:
        g = g + wd * p
    m = 0.9 * m + 0.1 * g
    v = 0.999 * v + 0.001 * g * g
    t = 4
    p = p - (1e-3 / (1 - 0.9 ** t)) * m / (v.sqrt() / (1 - 0.999 ** t) ** 0.5 + 1e-8)
    assert c["hp"][1].item() == 4.0
    torch.testing.assert_close(c["p"].cpu(), p, rtol=1e-5, atol=1e-6)
    torch.testing.assert_close(c["m"].cpu(), m, rtol=1e-5, atol=1e-6)
    torch.testing.assert_close(c["v"].cpu(), v, rtol=1e-5, atol=1e-6)
    assert torch.equal(c["sh"], c["p"].bfloat16())
    d = _clone(b0)
    d["g"][17] = float("inf")
    st = _norm(d["g"], scratch, gs=0.5, max_norm=1.0)
    step(d, st, zero=[(0, 16), (20, n)])
    for k in ("p", "m", "v", "sh", "hp"):
        assert torch.equal(d[k], b0[k]), k       # hp[1]: Adam's step count did not advance
    want = torch.zeros_like(b0["g"])
    want[16:20] = b0["g"][16:20]
    want[17] = float("inf")
    assert torch.equal(d["g"], want)


# ---------------------------------------------------------------- graphed steps
def _models(name, n):
    torch.manual_seed(0)
    ms = [build_model(name) for _ in range(n)]
    xavier_init(ms[0])
    for m in ms[1:]:
        m.load_state_dict(ms[0].state_dict())
    for m in ms:
        ldnn.prepare(m, "cuda")
    return ms


def test_graphed_step_with_clipping_matches_eager():
    """LeNet-5, batch 8, Adam: 4 replays == 4 eager steps (two eager runs give the spread, as
    test_layers_gpu.py::test_graphed_step_matches_eager judges it), and a threshold changed
    between replays is the one the next replay clips with -- seen in what the captured Adam
    kernel wrote: exp_avg moves by 0.1 * coef * g per step, so |m_new - 0.9 m_old| must be
    0.1 * min(last_norm, max_norm), i.e. 0.05 before and 1e-4 after the 500x smaller threshold."""
    m1, m2, m3 = _models("lenet5", 3)
    o1, o2, o3 = (Adam(m.parameters(), lr=1e-3, max_grad_norm=0.5) for m in (m1, m2, m3))
    crit = CrossEntropyLoss()
    g = torch.Generator(device="cuda").manual_seed(1)
    xs = [torch.randn(8, 1, 28, 28, device="cuda", generator=g).bfloat16() for _ in range(5)]
    ys = [torch.randint(0, 10, (8,), device="cuda", generator=g) for _ in range(5)]
    for m, o in ((m1, o1), (m2, o2), (m3, o3)):
        o.zero_grad()
        crit(m(xs[0]), ys[0]).backward()
        o.step()
    p0 = [q.detach().clone() for q in m2.parameters()]
    gs = GraphedStep(m1, crit, o1, xs[1], ys[1], warmup=0)
    coefs, moved = [], []
    for i in range(1, 5):
        if i == 3:
            for o in (o1, o2, o3):
                o.param_groups[0]["max_grad_norm"] = 1e-3
        m_old = o1._ls()["exp_avg"].clone()
        gs(xs[i], ys[i])
        moved.append((o1._ls()["exp_avg"].double() - 0.9 * m_old.double()).norm().item())
        for m, o in ((m2, o2), (m3, o3)):
            o.zero_grad()
            crit(m(xs[i]), ys[i]).backward()
            o.step()
        st1, st2 = o1._ls()["clip"], o2._ls()["clip"]
        coefs.append((st1[COEF].item(), st1[NORM].item(), st1[MAXN].item()))
        assert st1[NORM].item() == pytest.approx(st2[NORM].item(), rel=2e-2)
        # the replay clipped with the CURRENT threshold
        assert st1[COEF].item() == pytest.approx(min(1.0, st1[MAXN].item() / (st1[NORM].item() + 1e-6)), rel=1e-5)
    assert coefs[1][2] == 0.5 and coefs[2][2] == pytest.approx(1e-3)
    assert coefs[2][0] < 0.01 * coefs[1][0]          # 500x smaller threshold, norms of the same order
    for (coef, norm, mx), mv in zip(coefs, moved):   # the update kernel applied THAT coefficient
        assert mv == pytest.approx(0.1 * coef * norm, rel=1e-3), (mv, coef, norm, mx)
    assert moved[1] == pytest.approx(0.1 * min(0.5, coefs[1][1]), rel=1e-3)
    assert moved[2] == pytest.approx(1e-4, rel=1e-3) and moved[3] == pytest.approx(1e-4, rel=1e-3)
    torch.cuda.synchronize()
    assert o1.grad_clip_stats()["steps"].item() == o2.grad_clip_stats()["steps"].item() == 5
    for (n, p), (_, q), (_, s), r in zip(m1.named_parameters(), m2.named_parameters(), m3.named_parameters(), p0):
        d1, d2, d3 = ((t.detach() - r).flatten().double() for t in (p, q, s))
        eg, ee = (d1 - d2).norm().item(), (d3 - d2).norm().item()
        assert eg <= 3.0 * ee + 2e-3 * d2.norm().item(), (n, eg, ee, d2.norm().item())


def test_graphed_dp_world1_sharded_clipping_equals_unsharded():
    """GraphedDPStep on a world-1 comm (a world of one has nothing to shard: shard_optimizer
    then keeps the replicated update; the 2-rank tests below run the sharded chain): both
    DataParallel forms, clipped, == the single-process clipped graphed step."""
    shape = (128, 1, 28, 28)
    m1, m2, m3 = _models("lenet5", 3)
    crit = CrossEntropyLoss()
    dps = [DataParallel(m1, LocalComm(), bucket_cap_mb=0.05, broadcast_init=False, shard_optimizer=True),
           DataParallel(m2, LocalComm(), bucket_cap_mb=0.05, broadcast_init=False)]
    opts = [Adam(m.parameters(), lr=1e-3, max_grad_norm=0.5) for m in (m1, m2, m3)]
    g = torch.Generator(device="cuda").manual_seed(2)
    xs = [torch.randn(*shape, device="cuda", generator=g).bfloat16() for _ in range(4)]
    ys = [torch.randint(0, 10, (shape[0],), device="cuda", generator=g) for _ in range(4)]
    p0 = [p.detach().clone() for p in m3.parameters()]
    for dp, o in zip(dps, opts):
        o.zero_grad()
        crit(dp(xs[0]), ys[0]).backward()
        dp.finish_gradient_sync()
        o.step()
        dp.wait_gathers()
    opts[2].zero_grad()
    crit(m3(xs[0]), ys[0]).backward()
    opts[2].step()
    gds = [GraphedDPStep(dp, crit, o, xs[0], ys[0]) for dp, o in zip(dps, opts)]
    gs = GraphedStep(m3, crit, opts[2], xs[0], ys[0], warmup=0)
    for i in range(1, 4):
        for s in (*gds, gs):
            s(xs[i], ys[i])
    for s in (*gds, gs):                 # the odd-shaped batch: the eager fallback
        s(xs[0][:50], ys[0][:50])
    dps[0].gather_master(opts[0])
    torch.cuda.synchronize()
    stats = [{k: v.item() for k, v in o.grad_clip_stats().items()} for o in opts]
    assert stats[0]["steps"] == stats[1]["steps"] == stats[2]["steps"] == 5
    assert stats[0]["clipped"] >= 1 and stats[0]["skipped"] == 0
    assert stats[0]["last_norm"] == pytest.approx(stats[2]["last_norm"], rel=2e-2)
    for ma in (m1, m2):
        for a, b, r in zip(ma.parameters(), m3.parameters(), p0):
            da, db = (a.detach() - r).double(), (b.detach() - r).double()
            assert (da - db).norm().item() <= 2e-2 * db.norm().item() + 1e-6


def test_clipped_replay_and_eager_fallback_record_the_same_schedule():
    """Sharded + clipping: a replay and the eager odd-batch fallback issue the same collectives
    -- the buckets', the scalar all-reduce, the weight all-gathers (a 2-rank stand-in comm
    keeps a real world's bookkeeping, as tests/test_graphed_dp_gpu.py does)."""

    from ldnn.parallel.comm import _Done

    class TwoRankEcho(LocalComm):
        world_size = 2

        def reduce_scatter(self, out, inp, async_op=False):
            self.record("reduce_scatter", inp)
            out.copy_(inp[: out.numel()])
            return _Done() if async_op else None

        def all_gather_into(self, out, inp, async_op=False):
            self.record("all_gather_into", out)
            return _Done() if async_op else None

    shape = (128, 1, 28, 28)
    m1, = _models("lenet5", 1)
    crit = CrossEntropyLoss()
    comms = [TwoRankEcho(), TwoRankEcho()]
    dp = DataParallel(m1, comms[0], bucket_cap_mb=0.05, broadcast_init=False, shard_optimizer=True)
    o1 = SGD(m1.parameters(), lr=0.01, momentum=0.9, max_grad_norm=0.5)
    x = torch.randn(*shape, device="cuda").bfloat16()
    y = torch.randint(0, 10, (shape[0],), device="cuda")
    o1.zero_grad()
    crit(dp(x), y).backward()
    dp.finish_gradient_sync()
    o1.step()
    dp.wait_gathers()
    gd = GraphedDPStep(dp, crit, o1, x, y)
    # the per-bucket optimizer graphs gave way to a norm graph and an update graph
    assert dp.sharded and [i for _, i in gd.g_opts] == [None, "clip"]
    digests = []
    for c, xb, yb in ((comms[0], x, y), (comms[1], x[:50], y[:50])):
        dp.comm = dp.bucketer.comm = gd.comm = c
        c._sched, c._nops = hashlib.sha1(), 0
        gd(xb, yb)    # full batch: graph chain; short batch: eager fallback
        dp.wait_gathers()
        digests.append(c.schedule_digest())
    torch.cuda.synchronize()
    nb = len(dp.bucketer.buckets)
    nsh = sum(b["sharded"] for b in dp.bucketer.buckets)
    assert digests[0] == digests[1] and digests[0][0] == nb + 1 + nsh, (digests, nb, nsh)


@pytest.mark.parametrize("extra", [["--shard", "--optimizer", "adam"], ["--shard"], []])
def test_graphed_dp_two_ranks_gloo_with_clipping(extra):
    """2 gloo ranks sharing the GPU (scripts/check_graphed_dp.py --clip): the clipped graphed DP
    step == ONE clipped graphed rank on the concatenated batches, sharded == unsharded, the
    schedule check passes, replicas identical."""
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.join(ROOT, "scripts", "check_graphed_dp.py"), "--clip", "0.5"] + extra
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    assert "GRAPHED_DP_OK" in r.stdout, r.stdout[-3000:]
