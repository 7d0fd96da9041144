"""Adam8bit on the GPU: the adam8_step kernel (csrc/kernels/optim_q.hip) through the cases of
tests/test_adam8.py, and what only the kernel has: range launches, the skipped step, capture."""
import pytest
import torch

import ldnn
from ldnn.models import CrossEntropyLoss
from ldnn.models.mlp import MLP
from ldnn.ops._ext import C
from ldnn.optim import Adam8bit
from ldnn.train.graphed import GraphedStep
from test_adam8 import B1, B2, BIG, EPS, GS, INSTANCES, LR, LSQ_MEASURED, SEED, drift_case, lsq_case, one_step_case

pytestmark = pytest.mark.gpu
STATE = ("exp_avg_q", "exp_avg_sq_q", "exp_avg_scale", "exp_avg_sq_scale")


@pytest.mark.parametrize("inst", list(INSTANCES))
@pytest.mark.parametrize("nblk", [1, 5, BIG])
def test_kernel_one_step_matches_fp64(nblk, inst):
    C().set_opt_max_blocks(2 if nblk == BIG else 0)     # (BIG: the grid stride runs)
    try:
        one_step_case("cuda", nblk, **INSTANCES[inst])
    finally:
        C().set_opt_max_blocks(0)


def test_rounding_is_stochastic():
    drift_case("cuda")


def test_still_optimises_least_squares():
    r = lsq_case("cuda", 0)
    print(f"final loss ratio {r:.6f}")
    assert r <= 2 * max(LSQ_MEASURED)


def _bufs(nblk, seed, bad=None):
    """[w, g, mq, sq, ms, ss, shadow] after one warm step (so codes and scales are live), a fresh gradient."""
    n = nblk * 64
    gen = torch.Generator().manual_seed(seed)
    w, g0, g1 = (torch.randn(n, generator=gen).cuda() for _ in range(3))
    b = [w, g0, torch.zeros(n, dtype=torch.uint8, device="cuda"), torch.zeros(n, dtype=torch.uint8, device="cuda"),
         torch.zeros(nblk, device="cuda"), torch.zeros(nblk, device="cuda"),
         torch.zeros(n, dtype=torch.bfloat16, device="cuda")]
    C().adam8_step(*b, torch.tensor([LR, 1.0], device="cuda"), GS, B1, B2, EPS, 0.01, False, SEED, 0)
    b[1] = g1
    if bad is not None:
        g1[bad] = float("inf")
    return b


def _same(a, b):
    return all(torch.equal(x.view(torch.uint8), y.view(torch.uint8)) for x, y in zip(a, b))


@pytest.mark.parametrize("wide", [False, True])
def test_cuts_do_not_matter(wide):
    """One whole-buffer step == two range launches cut at block 3 of 7, bit for bit: master, shadow, codes,
    scales, cleared gradient ranges.  wide: the eight-lane form against the sixteen-lane whole-buffer step."""
    hp = torch.tensor([LR, 2.0], device="cuda")
    a, b = _bufs(7, 11), _bufs(7, 11)
    C().adam8_step(*a, hp, GS, B1, B2, EPS, 0.01, False, SEED, 0, zero_ranges=[(64, 300)])
    cut = 3 * 64
    for lo, hi, zr in ((0, cut, [(64, cut)]), (cut, 7 * 64, [(0, 300 - cut)])):
        C().adam8_step(b[0][lo:hi], b[1][lo:hi], b[2][lo:hi], b[3][lo:hi], b[4][lo // 64: hi // 64],
                       b[5][lo // 64: hi // 64], b[6][lo:hi], hp, GS, B1, B2, EPS, 0.01, False, SEED, lo, zero_ranges=zr,
                       wide=wide)
    assert _same(a, b) and bool((a[1][64:300] == 0).all()) and bool((a[1][300:] != 0).all())


def test_skipped_step_changes_nothing():
    """One inf in the gradient, clipping on: master, shadow, codes, scales and hp[1] keep their bits."""
    m = MLP(70, (33,), 10)
    ldnn.prepare(m, "cuda")
    o = Adam8bit(m.parameters(), lr=LR, max_grad_norm=1.0)
    f = o._flat_for_group(o.param_groups[0])
    f.grad.copy_(torch.randn(f.numel, generator=torch.Generator().manual_seed(3)))
    o.step()
    keep = [t.clone() for t in (f.master, f.shadow, o._ls()["hp"], *(o._ls()[k] for k in STATE))]
    f.grad.copy_(torch.randn(f.numel, generator=torch.Generator().manual_seed(4)))
    f.grad[77] = float("inf")
    o.step()
    torch.cuda.synchronize()
    assert _same(keep, (f.master, f.shadow, o._ls()["hp"], *(o._ls()[k] for k in STATE)))
    assert float(o._ls()["hp"][1]) == 1.0 and int(o.grad_clip_stats()["skipped"]) == 1


def test_graphed_step_equals_eager_bit_for_bit():
    """GraphedStep over a two-layer MLP, three replays == three eager steps from the same start: master
    and all four state tensors.  A capture before any eager step is refused."""
    torch.manual_seed(0)
    ms = [MLP(70, (33,), 10) for _ in range(2)]
    ms[1].load_state_dict(ms[0].state_dict())
    for m in ms:
        ldnn.prepare(m, "cuda")
    os_ = [Adam8bit(m.parameters(), lr=LR, seed=SEED) for m in ms]
    crit = CrossEntropyLoss()
    gen = torch.Generator(device="cuda").manual_seed(1)
    xs = [torch.randn(8, 70, device="cuda", generator=gen).bfloat16() for _ in range(4)]
    ys = [torch.randint(0, 10, (8,), device="cuda", generator=gen) for _ in range(4)]
    os_[0]._ldnn_capturing = True
    with pytest.raises(RuntimeError, match="run an eager optimizer step before capturing"):
        os_[0].step()
    os_[0]._ldnn_capturing = False
    for m, o in zip(ms, os_):
        o.zero_grad()
        crit(m(xs[0]), ys[0]).backward()
        o.step()
    gs = GraphedStep(ms[0], crit, os_[0], xs[1], ys[1], warmup=0)
    for i in (1, 2, 3):
        gs(xs[i], ys[i])
        os_[1].zero_grad()
        crit(ms[1](xs[i]), ys[i]).backward()
        os_[1].step()
    torch.cuda.synchronize()
    fa, fb = (o._flat_for_group(o.param_groups[0]) for o in os_)
    assert _same([fa.master, *(os_[0]._ls()[k] for k in STATE)], [fb.master, *(os_[1]._ls()[k] for k in STATE)])
    assert float(os_[0]._ls()["hp"][1]) == 4.0
