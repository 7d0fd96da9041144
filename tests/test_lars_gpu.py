"""LARS on the GPU: the seg_sumsq / lars_finalize kernels, the fused SGD kernel's ``lars=`` form
(csrc/kernels/optim.hip), and the LARS step replayed from hipGraphs (GraphedStep, GraphedDPStep)."""
import os
import socket
import subprocess
import sys

import pytest
import torch

import ldnn
from ldnn.models import CrossEntropyLoss, build_model, xavier_init
from ldnn.ops._ext import C
from ldnn.optim import SGD
from ldnn.optim.optimizers import lars_chunk_table
from ldnn.parallel.comm import LocalComm
from ldnn.parallel.ddp import DataParallel
from ldnn.train.graphed import GraphedDPStep, GraphedStep

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

COEF, SKIP = 1, 2
TRUST, EPS, WD, GS = 0.02, 1e-8, 1e-3, 0.5


def _layout(lens, gaps=()):
    """[(begin, end)] of segments ``lens`` long, a 64-element alignment gap after those in ``gaps``."""
    bounds, off = [], 0
    for i, n in enumerate(lens):
        bounds.append((off, off + n))
        off += n + (64 if i in gaps else 0)
    return bounds, off


def _bufs(bounds, n, seed):
    """master / grad: random inside the segments, NaN in the gaps (no chunk may touch them)."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    w = torch.full((n,), float("nan"), device="cuda")
    gr = torch.full((n,), float("nan"), device="cuda")
    for b, e in bounds:
        w[b:e] = torch.randn(e - b, device="cuda", generator=g)
        gr[b:e] = torch.randn(e - b, device="cuda", generator=g) * 3.0
    return w, gr


def _tables(bounds, ranges, adapt, slack=0):
    chunks, segs = lars_chunk_table(bounds, ranges, C().seg_sumsq_chunk())
    i32 = dict(dtype=torch.int32, device="cuda")
    segtab = torch.tensor([(a, b, int(ad), 0) for (a, b), ad in zip(segs, adapt)], **i32).reshape(-1, 4)
    partials = torch.full((2 * len(chunks) + slack,), float("nan"), device="cuda")
    return chunks, torch.tensor(chunks, **i32).reshape(-1, 4), segtab, partials


def _run(bounds, ranges, w, gr, adapt, ext=None, clip=None, sums=False, slack=0):
    S = len(bounds)
    _, chunks, segtab, partials = _tables(bounds, ranges, adapt, slack)
    hdr = torch.tensor([TRUST, EPS], device="cuda")
    ratio, wn, gn = torch.ones(65536, device="cuda"), torch.zeros(S, device="cuda"), torch.zeros(S, device="cuda")
    assert C().seg_sumsq(w, gr, chunks, partials, list(ranges), [b for b, _ in bounds]) == chunks.shape[0]
    if sums:
        out = torch.zeros(2 * S, device="cuda")
        C().lars_finalize(partials, segtab, hdr, ratio, wn, gn, 1.0, 0.0, sums_out=out)
        return out
    C().lars_finalize(partials, segtab, hdr, ratio, wn, gn, GS, WD, ext=ext, clip=clip)
    return ratio, wn, gn


def _want(bounds, ranges, w, gr, adapt, coef=1.0):
    """fp64: per-segment norms over the ranges, and the issue's formula."""
    out = []
    for (b, e), ad in zip(bounds, adapt):
        ws = gs = 0.0
        for lo, hi in ranges:
            x, y = max(b, lo), min(e, hi)
            if y > x:
                ws += w[x:y].double().square().sum().item()
                gs += gr[x:y].double().square().sum().item()
        wn, gn = ws ** 0.5, coef * GS * gs ** 0.5
        r = TRUST * wn / (gn + WD * wn + EPS) if (ad and wn > 0 and gn > 0) else 1.0
        out.append((r, wn, gn))
    return out


def _worst(got, want):
    ratio, wn, gn = (t.cpu().double() for t in got)
    worst = 0.0
    for i, (r, a, b) in enumerate(want):
        for g_, w_ in ((ratio[i].item(), r), (wn[i].item(), a), (gn[i].item(), b)):
            err = abs(g_ - w_) / w_ if w_ != 0 else abs(g_)
            assert err <= 1e-5, (i, g_, w_)
            worst = max(worst, err)
    assert bool((got[0][len(want):] == 1).all())     # the slots past the segments stay 1
    return worst


def test_seg_sumsq_and_finalize_match_fp64():
    """Made-up layouts against fp64 norms and the formula; bound 1e-5 relative on every w_norm,
    g_norm and ratio (the bound tests/test_grad_clip_gpu.py::test_sumsq_norm_matches_fp64 holds
    the same reduction structure to).  Measured maximum on MI355X: 1.2e-7.  Two runs give the same
    bits; NaN in the alignment gaps and in the unused partial slots changes nothing."""
    ch = C().seg_sumsq_chunk()
    assert ch % 64 == 0 and ch >= 1024
    layouts = [
        _layout([64, 128, ch - 64, ch, ch + 64, 3 * ch + 192], gaps=(1, 3)),
        _layout([192]),
        _layout([64] * 300),
    ]
    worst = 0.0
    for li, (bounds, n) in enumerate(layouts):
        S = len(bounds)
        adapt = [i % 4 != 1 for i in range(S)] if S > 1 else [True]
        w, gr = _bufs(bounds, n, 30 + li)
        last = bounds[-1]
        sets = [[(0, n)]]
        if li == 0:
            b2, b4 = bounds[2][0], bounds[4][0]
            sets.append([(b2 + 128, b4 + 64), (last[0] + 64, last[0] + 2 * ch + 128)])   # cut inside segments
            sets.append([(last[0] + ch + 64, last[0] + ch + 128)])                        # one 64-element piece
        for ranges in sets:
            chunks = lars_chunk_table(bounds, ranges, ch)[0]
            assert all(0 < (e - b) * 64 <= ch and bounds[s][0] <= b * 64 and e * 64 <= bounds[s][1]
                       for s, b, e, _ in chunks)
            assert [c[0] for c in chunks] == sorted(c[0] for c in chunks)      # a segment's chunks are consecutive
            a = _run(bounds, ranges, w, gr, adapt)
            b = _run(bounds, ranges, w, gr, adapt, slack=37)
            worst = max(worst, _worst(a, _want(bounds, ranges, w, gr, adapt)))
            for x, y in zip(a, b):
                assert torch.equal(x, y)
        if li == 0:
            # the sums of split ranges, added through ext, == the one-range result
            mid = bounds[4][0] + 128
            s1 = _run(bounds, [(0, mid)], w, gr, adapt, sums=True)
            s2 = _run(bounds, [(mid, n)], w, gr, adapt, sums=True)
            one = _run(bounds, [(0, n)], w, gr, adapt)
            S_ = len(bounds)
            hdr = torch.tensor([TRUST, EPS], device="cuda")
            segtab = _tables(bounds, [(0, n)], adapt)[2]
            ratio, wn, gn = torch.ones(65536, device="cuda"), torch.zeros(S_, device="cuda"), torch.zeros(S_, device="cuda")
            C().lars_finalize(None, segtab, hdr, ratio, wn, gn, GS, WD, ext=s1 + s2)
            for x, y in zip((ratio[:S_], wn, gn), (one[0][:S_], one[1], one[2])):
                assert bool(((x - y).abs() <= 1e-6 * y.abs()).all())
            # the clip state's coefficient scales the gradient norms; its skip flag writes nothing
            st = torch.zeros(8, device="cuda")
            st[COEF] = 0.25
            c = _run(bounds, [(0, n)], w, gr, adapt, clip=st)
            worst = max(worst, _worst(c, _want(bounds, [(0, n)], w, gr, adapt, coef=0.25)))
            st[SKIP] = 1.0
            d = _run(bounds, [(0, n)], w, gr, adapt, clip=st)
            assert bool((d[0] == 1).all()) and bool((d[1] == 0).all()) and bool((d[2] == 0).all())
    print(f"seg_sumsq + lars_finalize worst relative error {worst:.3e}")


def test_misaligned_ranges_are_refused():
    bounds, n = _layout([256, 256])
    w, gr = _bufs(bounds, n, 40)
    _, chunks, segtab, partials = _tables(bounds, [(0, n)], [True, True])
    with pytest.raises(RuntimeError, match="64-element aligned"):
        C().seg_sumsq(w, gr, chunks, partials, [(32, 256)], [0, 256])
    with pytest.raises(RuntimeError, match="multiple of 64"):
        C().seg_sumsq(w, gr, chunks, partials, [(0, n)], [0, 200])
    with pytest.raises(RuntimeError, match="64-element aligned"):
        C().seg_sumsq(w, gr, chunks, partials, [(0, n + 64)], [0, 256])      # past the buffers
    with pytest.raises(RuntimeError, match="2 slots per chunk"):
        C().seg_sumsq(w, gr, chunks, partials[:1], [(0, n)], [0, 256])
    with pytest.raises(ValueError, match="64-element aligned"):
        lars_chunk_table(bounds, [(0, 100)], C().seg_sumsq_chunk())


# ---------------------------------------------------------------- fused SGD kernel
N_OPT = 8192 + 64
# five segments and a gap; segment 2 spans element 4096, where a 4-workgroup grid's stride wraps
SEGS = [(0, 1024), (1024, 3072), (3072, 5120), (5184, 7232), (7232, N_OPT)]
RATIOS = [0.5, 1.0, 0.25, 1.0, 2.0]     # 1: an excluded tensor; 3: a zero gradient


def _sgd_bufs(seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    p = torch.randn(N_OPT, device="cuda", generator=g)
    gr = torch.randn(N_OPT, device="cuda", generator=g)
    gr[SEGS[3][0]:SEGS[3][1]] = 0
    ratio = torch.ones(65536, device="cuda")
    seg_of = torch.full((N_OPT // 64,), 65535, dtype=torch.int64)
    for i, (b, e) in enumerate(SEGS):
        seg_of[b // 64: e // 64] = i
        ratio[i] = RATIOS[i]
    return dict(p=p, g=gr, m=torch.randn(N_OPT, device="cuda", generator=g), sh=p.bfloat16(), ratio=ratio,
                map=seg_of.to(torch.uint16).cuda(), elem=ratio[seg_of.cuda()].repeat_interleave(64))


def _clone(b):
    return {k: v.clone() for k, v in b.items()}


def _sgd(b, nesterov, first, clip=None, zero=(), **kw):
    hp = torch.tensor([0.1, 0.0], device="cuda")
    C().sgd_step(b["p"], b["g"], b["m"], b["sh"], hp, GS, 0.9, 0.0, 1e-4, nesterov, first, zero_ranges=list(zero),
                 clip=clip, lars=(b["ratio"], b["map"]), **kw)


@pytest.mark.parametrize("first", [False, True])
@pytest.mark.parametrize("nesterov", [False, True])
def test_fused_sgd_lars(nesterov, first):
    """A hand-written ratio table against the fp32 torch formula, tolerance of
    tests/test_grad_clip_gpu.py::test_fused_sgd_clip; the gap (random values here) updates with ratio 1."""
    b0 = _sgd_bufs(41)
    C().set_opt_max_blocks(4)       # 4 workgroups x 256 threads x 4 elements: the stride wraps at 4096
    try:
        zero = [(3, 5000), (8190, N_OPT)]
        for coef in (None, 0.3):
            c = _clone(b0)
            st = None
            if coef is not None:
                st = torch.zeros(8, device="cuda")
                st[COEF] = coef
            _sgd(c, nesterov, first, clip=st, zero=zero)
            p, g, m, r = b0["p"].cpu(), b0["g"].cpu() * GS * (coef or 1.0), b0["m"].cpu(), b0["elem"].cpu()
            g = (g + 1e-4 * p) * r
            m = g.clone() if first else 0.9 * m + g
            p = p - 0.1 * ((g + 0.9 * m) if nesterov else m)
            torch.testing.assert_close(c["p"].cpu(), p, rtol=1e-5, atol=1e-6)
            torch.testing.assert_close(c["m"].cpu(), m, rtol=1e-5, atol=1e-6)
            assert torch.equal(c["sh"], c["p"].bfloat16())
            want = b0["g"].clone()
            want[3:5000] = 0
            want[8190:] = 0
            assert torch.equal(c["g"], want)
            # the zero-gradient segment moved by weight decay and momentum alone, the excluded one as plain SGD
            assert not torch.equal(c["p"][SEGS[0][0]:SEGS[0][1]], b0["p"][SEGS[0][0]:SEGS[0][1]])
        # the skip flag set: nothing but the zero ranges changes
        d = _clone(b0)
        st = torch.zeros(8, device="cuda")
        st[SKIP] = 1.0
        _sgd(d, nesterov, first, clip=st, zero=zero)
        for k in ("p", "m", "sh"):
            assert torch.equal(d[k], b0[k]), k
        assert torch.equal(d["g"], want)
        # a table of ones == the kernel without lars, bit for bit
        e, f = _clone(b0), _clone(b0)
        e["ratio"].fill_(1.0)
        _sgd(e, nesterov, first)
        hp = torch.tensor([0.1, 0.0], device="cuda")
        C().sgd_step(f["p"], f["g"], f["m"], f["sh"], hp, GS, 0.9, 0.0, 1e-4, nesterov, first)
        for k in ("p", "m", "sh", "g"):
            assert torch.equal(e[k], f[k]), k
    finally:
        C().set_opt_max_blocks(0)


def test_fused_sgd_lars_refusals():
    b = _sgd_bufs(42)
    t = torch.zeros(64, 64, device="cuda", dtype=torch.bfloat16)
    with pytest.raises(RuntimeError, match="t_out"):
        _sgd(b, False, False, t_begin=256, t_out=t)
    hp = torch.tensor([0.1, 0.0], device="cuda")
    args = (b["p"], b["g"], b["m"], b["sh"], hp, GS, 0.9, 0.0, 1e-4, False, False)
    with pytest.raises(RuntimeError, match="lars"):
        C().sgd_step(*args, lars=(b["ratio"][:100], b["map"]))          # a short ratio table
    with pytest.raises(RuntimeError, match="lars"):
        C().sgd_step(*args, lars=(b["ratio"], b["map"][:-1]))           # a short map
    with pytest.raises(RuntimeError):
        C().sgd_step(*args, lars=(b["ratio"], b["map"].to(torch.int32)))
    for k in ("p", "g", "m"):
        assert torch.equal(b[k], _sgd_bufs(42)[k])


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


def _implied_trust(o):
    """trust_coef as the stats of the last step imply it: ratio * (gn + wd * wn + eps) / wn over
    the adapted tensors."""
    st = o.lars_stats()
    ad = torch.tensor(st["adapted"], device="cuda")
    r, wn, gn = st["ratio"][ad].double(), st["w_norm"][ad].double(), st["g_norm"][ad].double()
    return (r * (gn + 1e-4 * wn + 1e-8) / wn).cpu()


def test_graphed_step_with_lars_matches_eager():
    """LeNet-5, batch 8, SGD-momentum + LARS: 4 replays == 4 eager steps (two eager runs give the
    spread, as tests/test_grad_clip_gpu.py::test_graphed_step_with_clipping_matches_eager judges
    it), and a trust coefficient made 10x smaller between replays 2 and 3 is the one the next
    replay's ratios carry (10x within 2 %)."""
    m1, m2, m3 = _models("lenet5", 3)
    o1, o2, o3 = (SGD(m.parameters(), lr=0.05, momentum=0.9, weight_decay=1e-4, lars_trust=TRUST)
                  for m in (m1, m2, m3))
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
    trusts = []
    for i in range(1, 5):
        if i == 3:
            for o in (o1, o2, o3):
                o.param_groups[0]["lars_trust"] = TRUST / 10
        gs(xs[i], ys[i])
        for m, o in ((m2, o2), (m3, o3)):
            o.zero_grad()
            crit(m(xs[i]), ys[i]).backward()
            o.step()
        trusts.append(_implied_trust(o1))
        r1, r2 = o1.lars_stats()["ratio"], o2.lars_stats()["ratio"]
        assert bool(((r1 - r2).abs() <= 2e-2 * r2.abs()).all()), (i, r1, r2)
    for t, want in zip(trusts, (TRUST, TRUST, TRUST / 10, TRUST / 10)):
        assert bool(((t - want).abs() <= 1e-3 * want).all()), (t, want)
    assert bool(((trusts[2] / trusts[1] - 0.1).abs() <= 0.02 * 0.1).all())
    ad = o1.lars_stats()["adapted"]
    assert any(ad) and not all(ad)
    assert bool((o1.lars_stats()["ratio"][~torch.tensor(ad, device="cuda")] == 1).all())
    torch.cuda.synchronize()
    for (n, p), (_, q), (_, s), r in zip(m1.named_parameters(), m2.named_parameters(), m3.named_parameters(), p0):
        d1, d2, d3 = ((t.detach() - r).flatten().double() for t in (p, q, s))
        eg, ee = (d1 - d2).norm().item(), (d3 - d2).norm().item()
        assert eg <= 3.0 * ee + 2e-3 * d2.norm().item(), (n, eg, ee, d2.norm().item())


@pytest.mark.parametrize("clip", [None, 0.5])
def test_graphed_dp_world1_lars_equals_single_process(clip):
    """GraphedDPStep on a world-1 comm, shard_optimizer on and off, == the single-process graphed
    step, with the odd-batch eager fallback; tolerance of
    tests/test_grad_clip_gpu.py::test_graphed_dp_world1_sharded_clipping_equals_unsharded."""
    shape = (128, 1, 28, 28)
    m1, m2, m3 = _models("lenet5", 3)
    crit = CrossEntropyLoss()
    dps = [DataParallel(m1, LocalComm(), bucket_cap_mb=0.05, broadcast_init=False, shard_optimizer=True),
           DataParallel(m2, LocalComm(), bucket_cap_mb=0.05, broadcast_init=False)]
    opts = [SGD(m.parameters(), lr=0.05, momentum=0.9, weight_decay=1e-4, lars_trust=TRUST, max_grad_norm=clip)
            for m in (m1, m2, m3)]
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
    stats = [dict(zip(o.lars_stats()["names"], o.lars_stats()["ratio"].tolist())) for o in opts]
    for st in stats[:2]:
        for n, v in stats[2].items():
            assert st[n] == pytest.approx(v, rel=2e-2), n
    assert any(v != 1.0 for v in stats[2].values())
    if clip is not None:
        cs = [{k: v.item() for k, v in o.grad_clip_stats().items()} for o in opts]
        assert cs[0]["steps"] == cs[1]["steps"] == cs[2]["steps"] == 5 and cs[0]["skipped"] == 0
    for ma in (m1, m2):
        for a, b, r in zip(ma.parameters(), m3.parameters(), p0):
            da, db = (a.detach() - r).double(), (b.detach() - r).double()
            assert (da - db).norm().item() <= 2e-2 * db.norm().item() + 1e-6


def test_graphed_dp_two_ranks_gloo_with_lars():
    """2 gloo ranks sharing the GPU (scripts/check_graphed_dp.py --lars --shard): the graphed
    sharded LARS step == ONE graphed rank on the concatenated batches == the unsharded run, the
    schedule check passes, replicas identical."""
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.join(ROOT, "scripts", "check_graphed_dp.py"), "--lars", "0.02", "--shard"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    assert "GRAPHED_DP_OK" in r.stdout, r.stdout[-3000:]
