"""FedProx on the GPU: the PROX instances of sgd_kernel / adam_kernel / lion_kernel (csrc/kernels/optim.hip)
-- an exact contraction toward the anchor, fp64 references on seeded normals with and without the clip
state, mu = 0 and prox=None against the plain call, the skip flag, the range form -- and the term
replayed from a hipGraph (GraphedStep) with mu and the anchor changed between replays.

n = 16387 throughout (tests/test_lion_gpu.py's N_MAIN): a float4 body, a grid-stride wrap under
set_opt_max_blocks(4), and a 3-element scalar tail."""
import pytest
import torch

import ldnn
from ldnn.models import CrossEntropyLoss, build_model, xavier_init
from ldnn.models.mlp import MLP
from ldnn.ops._ext import C
from ldnn.optim import SGD, Adam, Lion
from ldnn.train.graphed import GraphedStep

pytestmark = pytest.mark.gpu

COEF, SKIP = 1, 2
N = 4 * 4096 + 3
LR, MU, GS, WD = 1e-3, 0.1, 0.5, 1e-2
SEED = 31       # (checked on the CPU: 0 of the 16387 elements of either Lion case are undecided)
ZERO = [(3, 5000), (N - 6, N)]


def _bits(t):
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def _inputs(seed=SEED, n=N):
    """w, g, m, v (>= 0), anchor: seeded normals drawn on the CPU (so the fp64 reference's undecided
    signs can be counted without a GPU), moved to the device."""
    g = torch.Generator().manual_seed(seed)
    w, gr, m = torch.randn(n, generator=g), torch.randn(n, generator=g) * 3.0, torch.randn(n, generator=g) * 0.5
    v = torch.randn(n, generator=g).square() * 0.1
    a = w + torch.randn(n, generator=g) * 0.3
    return tuple(t.cuda() for t in (w, gr, m, v, a))


def _clip(coef=None, skip=False):
    if coef is None and not skip:
        return None
    st = torch.zeros(8, device="cuda")
    st[COEF], st[SKIP] = (1.0 if coef is None else coef), float(skip)
    return st


def _hdr(mu):
    return torch.tensor([mu, 0.0, 0.0, 0.0], device="cuda")


# the four updates: (call(C, w, g, m, v, shadow, hp, prox, clip, zero), fp64 reference, moment count)
def _sgd(w, g, m, v, sh, hp, prox, clip, zero=()):
    C().sgd_step(w, g, m, sh, hp, GS, 0.9, 0.0, WD, False, False, zero_ranges=list(zero), clip=clip, prox=prox)


def _adam(decoupled):
    def call(w, g, m, v, sh, hp, prox, clip, zero=()):
        C().adam_step(w, g, m, v, sh, hp, GS, 0.9, 0.999, 1e-8, WD, decoupled, zero_ranges=list(zero), clip=clip,
                      prox=prox)
    return call


def _lion(w, g, m, v, sh, hp, prox, clip, zero=()):
    C().lion_step(w, g, m, sh, hp, GS, 0.9, 0.99, WD, zero_ranges=list(zero), clip=clip, prox=prox)


def _ref_sgd(w, g, m, v, a, gs, mu, t):
    g = g * gs + WD * w + mu * (w - a)
    m = 0.9 * m + g
    return w - LR * m, m, v, None


def _ref_adam(decoupled):
    def ref(w, g, m, v, a, gs, mu, t):
        g = g * gs
        p = w
        if decoupled:
            p = p * (1 - LR * WD)
        else:
            g = g + WD * w
        g = g + mu * (w - a)
        m = 0.9 * m + 0.1 * g
        v = 0.999 * v + 0.001 * g * g
        return p - (LR / (1 - 0.9 ** t)) * m / (v.sqrt() / (1 - 0.999 ** t) ** 0.5 + 1e-8), m, v, None
    return ref


def _ref_lion(w, g, m, v, a, gs, mu, t):
    g = g * gs + mu * (w - a)
    c = 0.9 * m + 0.1 * g
    und = c.abs() <= 4 * 2.0 ** -24 * ((0.9 * m).abs() + (0.1 * g).abs())
    return w * (1 - LR * WD) - LR * torch.sign(c), 0.99 * m + 0.01 * g, v, und


UPDATES = {"sgd": (_sgd, _ref_sgd, 1), "adam": (_adam(False), _ref_adam(False), 2),
           "adamw": (_adam(True), _ref_adam(True), 2), "lion": (_lion, _ref_lion, 1)}
T = 3.0      # Adam's step count in hp[1]


def _hp():
    return torch.tensor([LR, T], device="cuda")


# ---------------------------------------------------------------- 1. exact contraction
@pytest.mark.parametrize("cap", [0, 4])
def test_sgd_contracts_toward_the_anchor_bit_for_bit(cap):
    """Momentum 0, no weight decay, g = 0, mu = 1, lr = 0.5: w <- w - 0.5 (w - a), so after k steps
    w - a == (w0 - a) 2^-k.  Weights and anchor are small integers times 2^-4: every difference,
    product and sum is exact in fp32 for k = 1..4, whatever the evaluation order or contraction.  A
    wrong anchor index or a missed tail element shows as a differing bit."""
    g = torch.Generator().manual_seed(7)
    w0 = (torch.randint(-64, 65, (N,), generator=g).float() / 16).cuda()
    a = (torch.randint(-64, 65, (N,), generator=g).float() / 16).cuda()
    a0, d0 = a.clone(), w0 - a
    assert int((d0 != 0).sum()) > N // 2 and bool((d0[-3:] != 0).all())       # (the tail moves too)
    w, grad = w0.clone(), torch.zeros(N, device="cuda")
    sh = w.bfloat16()
    hp, hdr = torch.tensor([0.5, 0.0], device="cuda"), _hdr(1.0)
    C().set_opt_max_blocks(cap)
    try:
        for k in range(1, 5):
            C().sgd_step(w, grad, w, sh, hp, 1.0, 0.0, 0.0, 0.0, False, k == 1, prox=(a, hdr))
            assert torch.equal(_bits(w - a), _bits(d0 * 2.0 ** -k)), k
            assert torch.equal(_bits(sh), _bits(w.bfloat16())), k
    finally:
        C().set_opt_max_blocks(0)
    assert torch.equal(_bits(a), _bits(a0)) and bool((grad == 0).all())


# ---------------------------------------------------------------- 2. fp64 references
@pytest.mark.parametrize("coef", [None, 0.25], ids=["noclip", "clip"])
@pytest.mark.parametrize("name", list(UPDATES))
def test_prox_update_matches_fp64(name, coef):
    """sgd_step (momentum 0.9), adam_step (coupled and decoupled) and lion_step with prox=, mu = 0.1,
    weight decay 1e-2, grad_scale 0.5, with and without a clip state of coefficient 0.25, one step from
    seeded normals against the formulas in fp64: weights and moments within rtol 1e-5 / atol 1e-6, the
    bound tests/test_lion_gpu.py and tests/test_lamb_gpu.py hold these expressions to.  Lion: as in
    tests/test_lion_gpu.py::test_random_inputs_match_fp64, an element is undecided when |c| <= 4 * 2^-24
    * (|beta1 m| + |(1 - beta1) g|), its w must be one of the three possible outcomes, and at most
    0.01 % of the elements may be undecided (the seed gives 0).  The shadow is bf16(w) bitwise; the
    gradient and the anchor are only read."""
    call, ref, nmom = UPDATES[name]
    w0, g0, m0, v0, a0 = _inputs()
    w, g, m, v, a = (t.clone() for t in (w0, g0, m0, v0, a0))
    sh = w.bfloat16()
    call(w, g, m, v, sh, _hp(), (a, _hdr(MU)), _clip(coef))
    gs = GS * (coef if coef is not None else 1.0)
    rw, rm, rv, und = ref(w0.double(), g0.double(), m0.double(), v0.double(), a0.double(), gs, MU, T)
    tol = lambda r: 1e-6 + 1e-5 * r.abs()      # noqa: E731
    em = (m.double() - rm).abs()
    assert bool((em <= tol(rm)).all()), em.max().item()
    if nmom == 2:
        ev = (v.double() - rv).abs()
        assert bool((ev <= tol(rv)).all()), ev.max().item()
    else:
        assert torch.equal(_bits(v), _bits(v0))
    ew = (w.double() - rw).abs()
    if und is None:
        und = torch.zeros(N, dtype=torch.bool, device="cuda")
    n_und = int(und.sum())
    assert n_und <= 1e-4 * N, n_und
    assert bool((ew <= tol(rw))[~und].all()), ew[~und].max().item()
    if n_und:
        base = w0.double()[und] * (1 - LR * WD)
        ok = torch.zeros(n_und, dtype=torch.bool, device="cuda")
        for s in (-1.0, 0.0, 1.0):
            ok |= (w.double()[und] - (base - LR * s)).abs() <= tol(base - LR * s)
        assert bool(ok.all())
    assert not torch.equal(w, w0)
    assert torch.equal(_bits(sh), _bits(w.bfloat16()))
    assert torch.equal(_bits(g), _bits(g0)) and torch.equal(_bits(a), _bits(a0))
    # (the term is in the result: the same call without it lands elsewhere)
    w2, g2, m2, v2 = (t.clone() for t in (w0, g0, m0, v0))
    call(w2, g2, m2, v2, None, _hp(), None, _clip(coef))
    assert float((m2.double() - rm).abs().max()) > 1e-4
    print(f"{name} prox ({'clip' if coef else 'no clip'}): worst |dw| {ew[~und].max().item():.3e}, worst |dm| "
          f"{em.max().item():.3e}, undecided {n_und}")


# ---------------------------------------------------------------- 3. mu = 0 and prox=None
@pytest.mark.parametrize("coef", [None, 0.25], ids=["noclip", "clip"])
@pytest.mark.parametrize("name", list(UPDATES))
def test_mu_zero_and_no_prox_are_the_plain_update(name, coef):
    """prox= with mu = 0 in the header adds +-0 to every gradient element: the PROX instance gives the
    bits of the call without prox=; prox=None is that call (the parent's launch)."""
    call = UPDATES[name][0]
    w0, g0, m0, v0, a0 = _inputs()
    res = []
    for prox in ((a0.clone(), _hdr(0.0)), None, "absent"):
        w, g, m, v = (t.clone() for t in (w0, g0, m0, v0))
        sh = w.bfloat16()
        if prox == "absent":     # the parent-style call: no keyword at all
            {"sgd": lambda: C().sgd_step(w, g, m, sh, _hp(), GS, 0.9, 0.0, WD, False, False, clip=_clip(coef)),
             "adam": lambda: C().adam_step(w, g, m, v, sh, _hp(), GS, 0.9, 0.999, 1e-8, WD, False, clip=_clip(coef)),
             "adamw": lambda: C().adam_step(w, g, m, v, sh, _hp(), GS, 0.9, 0.999, 1e-8, WD, True, clip=_clip(coef)),
             "lion": lambda: C().lion_step(w, g, m, sh, _hp(), GS, 0.9, 0.99, WD, clip=_clip(coef))}[name]()
        else:
            call(w, g, m, v, sh, _hp(), prox, _clip(coef))
        res.append((w, g, m, v, sh))
    for other in res[1:]:
        for x, y in zip(res[0], other):
            assert torch.equal(_bits(x), _bits(y))
    assert not torch.equal(res[0][0], w0)


# ---------------------------------------------------------------- 4. the skip flag
@pytest.mark.parametrize("cap", [0, 4])
@pytest.mark.parametrize("name", list(UPDATES))
def test_skipped_step_changes_nothing_and_still_clears_the_zero_ranges(name, cap):
    call = UPDATES[name][0]
    w0, g0, m0, v0, a0 = _inputs()
    w, g, m, v, a = (t.clone() for t in (w0, g0, m0, v0, a0))
    sh = w.bfloat16()
    want_g = g0.clone()
    for lo, hi in ZERO:
        want_g[lo:hi] = 0
    C().set_opt_max_blocks(cap)
    try:
        call(w, g, m, v, sh, _hp(), (a, _hdr(MU)), _clip(skip=True), ZERO)
    finally:
        C().set_opt_max_blocks(0)
    for x, y in ((w, w0), (m, m0), (v, v0), (a, a0), (sh, w0.bfloat16()), (g, want_g)):
        assert torch.equal(_bits(x), _bits(y))
    # (not skipped: the same ranges are cleared and the step is the one without ranges)
    call(w, g0.clone(), m, v, sh, _hp(), (a, _hdr(MU)), _clip(1.0), ZERO)
    w2, g2, m2, v2 = (t.clone() for t in (w0, g0, m0, v0))
    call(w2, g2, m2, v2, None, _hp(), (a, _hdr(MU)), _clip(1.0))
    assert torch.equal(_bits(w), _bits(w2)) and torch.equal(_bits(m), _bits(m2)) and not torch.equal(w, w0)


# ---------------------------------------------------------------- 5. binding refusals
def test_binding_refusals_leave_the_buffers_alone():
    n = 4096
    w0, g0, m0, v0, a0 = _inputs(n=n)
    w, g, m, v, a = (t.clone() for t in (w0, g0, m0, v0, a0))
    hdr = _hdr(MU)
    ratio, segmap = torch.ones(65536, device="cuda"), torch.zeros(n // 64, dtype=torch.uint16, device="cuda")
    t_out = torch.zeros(64, 64, device="cuda").bfloat16()
    bad = [(a.double(), hdr), (a.cpu(), hdr), (a[:-4], hdr), (torch.zeros(n + 4, device="cuda")[1:n + 1], hdr),
           (a, hdr.double()), (a, hdr.cpu()), (a, hdr[:0]), (torch.zeros(2 * n, device="cuda")[::2], hdr)]
    for prox in bad:
        for call in (_sgd, _adam(False), _lion):
            with pytest.raises((RuntimeError, TypeError)):
                call(w, g, m, v, None, _hp(), prox, None)
    with pytest.raises(RuntimeError, match="prox"):
        C().sgd_step(w, g, m, None, _hp(), GS, 0.9, 0.0, WD, False, False, lars=(ratio, segmap), prox=(a, hdr))
    with pytest.raises(RuntimeError, match="prox"):
        C().sgd_step(w, g, m, None, _hp(), GS, 0.9, 0.0, WD, False, False, t_begin=0, t_out=t_out, prox=(a, hdr))
    torch.cuda.synchronize()
    for x, y in ((w, w0), (g, g0), (m, m0), (v, v0), (a, a0)):
        assert torch.equal(_bits(x), _bits(y))
    # (a range of the buffers: the anchor cut like the master is accepted)
    _sgd(w[64:], g[64:], m[64:], v, None, _hp(), (a[64:], hdr), None)
    assert torch.equal(_bits(w[:64]), _bits(w0[:64])) and not torch.equal(w[64:], w0[64:])


# ---------------------------------------------------------------- 6. the optimizers: ranges, graphs
def _model():
    torch.manual_seed(0)
    m = MLP(70, (33,), 10)
    ldnn.prepare(m, "cuda")
    return m


def _flat(opt):
    return opt._flat_for_group(opt.param_groups[0])


def _fill_grad(flat, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    flat.grad.copy_(torch.randn(flat.numel, device="cuda", generator=g))


@pytest.mark.parametrize("make", [lambda p: SGD(p, lr=0.05, momentum=0.9, weight_decay=1e-4, prox_mu=MU),
                                  lambda p: Adam(p, lr=1e-2, prox_mu=MU), lambda p: Lion(p, lr=1e-3, prox_mu=MU)],
                         ids=["sgd", "adam", "lion"])
def test_range_updates_equal_the_whole_buffer_step_bit_for_bit(make):
    """One eager step anchors both optimizers at the initial weights; the second step -- the term is now
    nonzero -- runs whole on one and as two range_updater() launches, cut at a multiple of 4, on the other."""
    o1, o2 = make(_model().parameters()), make(_model().parameters())
    f1, f2 = _flat(o1), _flat(o2)
    for f, o in ((f1, o1), (f2, o2)):
        _fill_grad(f, 1)
        o.step()
    a = o1._ls()["prox_anchor"]
    assert torch.equal(a, o2._ls()["prox_anchor"]) and not torch.equal(a, f1.master)
    _fill_grad(f1, 2)
    _fill_grad(f2, 2)
    o1.step()
    s = o2.range_updater()
    assert s is not None and s.prox is not None
    cut = (f2.numel // 2) // 4 * 4 + 4
    s.update(0, cut)
    s.update(cut, f2.numel)
    s.end()
    torch.cuda.synchronize()
    assert torch.equal(_bits(f1.master), _bits(f2.master)) and torch.equal(_bits(f1.shadow), _bits(f2.shadow))
    for k in ("momentum", "exp_avg", "exp_avg_sq", "prox_anchor"):
        if k in o1._ls():
            assert torch.equal(_bits(o1._ls()[k]), _bits(o2._ls()[k])), k
    # (and the term is in it: the anchor still holds the initial weights, the drift is that of two steps)
    assert o1.prox_stats()["drift_norm"] > 0 and sorted(o1.state_dict()["ldnn_flat_state"]) == \
        sorted(k for k in o1._ls() if k not in ("hp", "prox_anchor", "prox_hdr"))


def test_graphed_step_follows_mu_and_the_anchor():
    """GraphedStep on mlp3_small, SGD-momentum, captured with prox_mu = 0.1 after one eager step (which
    anchors).  Between the replays prox_mu changes (0.1, 0.5 with sync_hyperparams(), then back through the
    step's own refresh) and set_prox_anchor() re-anchors; an eager twin -- its own model, same inputs --
    is stepped with the same values.  Every replay's master within rtol 1e-5 / atol 1e-6 of the twin's
    (test 2's bound)."""
    torch.manual_seed(0)
    ms = [build_model("mlp3_small") for _ in range(2)]
    xavier_init(ms[0])
    ms[1].load_state_dict(ms[0].state_dict())
    for m in ms:
        ldnn.prepare(m, "cuda")
    o1, o2 = (SGD(m.parameters(), lr=0.05, momentum=0.9, prox_mu=MU) for m in ms)
    crit = CrossEntropyLoss()
    g = torch.Generator(device="cuda").manual_seed(1)
    xs = [torch.randn(64, 784, device="cuda", generator=g).bfloat16() for _ in range(6)]
    ys = [torch.randint(0, 10, (64,), device="cuda", generator=g) for _ in range(6)]

    def eager(m, o, i):
        o.zero_grad()
        crit(m(xs[i]), ys[i]).backward()
        o.step()

    # a capture before any anchor exists asks for an eager step first
    o1._ldnn_capturing = True
    try:
        o1.zero_grad()
        crit(ms[0](xs[0]), ys[0]).backward()
        with pytest.raises(RuntimeError, match="run an eager optimizer step before capturing"):
            o1.step()
    finally:
        o1._ldnn_capturing = False
    assert "prox_anchor" not in o1._ls()
    for m, o in zip(ms, (o1, o2)):
        eager(m, o, 0)
    gs = GraphedStep(ms[0], crit, o1, xs[1], ys[1], warmup=0)
    f1, f2 = _flat(o1), _flat(o2)
    anchor = o1._ls()["prox_anchor"]
    worst = 0.0
    for i in range(1, 6):
        if i == 2:
            for o in (o1, o2):
                o.param_groups[0]["prox_mu"] = 0.5
            o1.sync_hyperparams()
        if i == 3:
            for o in (o1, o2):
                o.set_prox_anchor()
            assert o1._ls()["prox_anchor"] is anchor and torch.equal(anchor, f1.master)
        if i == 4:
            for o in (o1, o2):
                o.param_groups[0]["prox_mu"] = MU      # (no explicit sync: the step refreshes a changed value)
        gs(xs[i], ys[i])
        eager(ms[1], o2, i)
        torch.cuda.synchronize()
        assert float(o1._ls()["prox_hdr"][0]) == pytest.approx(0.5 if i in (2, 3) else MU)
        d = (f1.master.double() - f2.master.double()).abs()
        worst = max(worst, d.max().item())
        assert bool((d <= 1e-6 + 1e-5 * f2.master.double().abs()).all()), (i, d.max().item())
        torch.testing.assert_close(o1._ls()["prox_anchor"], o2._ls()["prox_anchor"], rtol=1e-5, atol=1e-6)
    assert o1.prox_stats()["drift_norm"] > 0
    print(f"graphed SGD + prox vs eager twin: worst |dw| {worst:.3e}")
