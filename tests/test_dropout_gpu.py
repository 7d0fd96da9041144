"""The dropout kernels (dropout.hip) against the NumPy twin, bit for bit: y, dx and the counter read
back, over dense, padded, misaligned and 3-D layouts; the ticket; replay from a captured graph; a
graphed training step against eager ones; the placement in a CNN against the CPU twin path.

y = drop ? 0 : bf16_rne(float(x) * scale) has one correctly rounded fp32 product and one rounding
to bf16, and the mask is integer arithmetic: the comparison is exact (on the bit patterns, so a
dropped element is +0).  Not covered: element counts beyond 2^32 (the 64-bit indexing is by
inspection)."""
import numpy as np
import pytest
import torch

import ldnn
from ldnn.models import CrossEntropyLoss, build_model, xavier_init
from ldnn.models.layers import Dropout, reseed_dropout
from ldnn.models.mlp import MLP
from ldnn.ops import _ext
from ldnn.ops import functional as LF

pytestmark = pytest.mark.gpu

SEED, MODULE = 0x1234567890ABCDEF, 3


def _vals(n, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(n, generator=g) * 3).bfloat16()      # finite, bf16-exact


def _layout(kind, shape, seed):
    """(x on the GPU in the asked layout, the same values dense on the CPU)."""
    n = int(np.prod(shape))
    v = _vals(n, seed).view(shape)
    if kind == "dense":
        return v.cuda(), v
    if kind == "misaligned":      # the base sits 2 bytes into an aligned allocation: the scalar path
        buf = torch.zeros(n + 1, dtype=torch.bfloat16, device="cuda")
        buf[1:].copy_(v.view(-1))
        x = buf[1:].view(shape)
        assert x.data_ptr() % 16 == 2
        return x, v
    B, N = shape
    npad = int(kind)              # the [B, N] view of a [B, npad] buffer whose pad columns hold 1.0
    buf = torch.ones(B, npad, dtype=torch.bfloat16, device="cuda")
    buf[:, :N].copy_(v)
    return buf[:, :N], v


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int16)


def _expect(v, drop, thr):
    scale = float(LF.dropout_scale(thr))
    return torch.where(drop, torch.zeros(()), v.float() * scale).bfloat16()


def _mask(counter, thr, shape, seed=SEED, module=MODULE):
    N = shape[-1]
    return torch.from_numpy(LF.dropout_mask(seed, module, counter, thr, int(np.prod(shape)) // N, N)).view(shape)


def _pad_columns(t, npad):
    B, N = t.shape
    assert t.stride() == (npad, 1)
    return t.as_strided((B, npad), (npad, 1), t.storage_offset())[:, N:]


CASES = [("dense", (1, 1)), ("dense", (5, 10)), ("dense", (7, 8)), ("dense", (64, 120)), ("dense", (33, 1000)),
         ("16", (5, 10)), ("88", (64, 84)),
         ("24", (5, 13)),      # 5 columns in the row's last partial vector, then a vector that is all pad
         ("misaligned", (5, 16)), ("misaligned", (33, 1000)),
         ("dense", (2048, 4096)), ("dense", (4, 6, 20))]


@pytest.mark.parametrize("p", [0.25, 0.5])
@pytest.mark.parametrize("kind,shape", CASES, ids=lambda v: str(v).replace(" ", ""))
def test_kernels_match_the_twin_bit_for_bit(kind, shape, p):
    x, v = _layout(kind, shape, seed=7)
    g, gv = _layout(kind, shape, seed=8)
    x.requires_grad_()
    st = LF.DropoutState(x.device, SEED, MODULE)
    thr = LF.dropout_thr(p)
    y = LF.dropout(x, p, True, st)
    (ticket,) = y.grad_fn.saved_tensors
    (dx,) = torch.autograd.grad(y, x, g)
    torch.cuda.synchronize()
    assert st.read() == dict(seed=SEED, module_index=MODULE, counter=1, thr=thr)
    drop = _mask(0, thr, shape)
    assert y.shape == x.shape and y.dtype == torch.bfloat16 and dx.shape == x.shape
    assert torch.equal(_bits(y), _bits(_expect(v, drop, thr)))
    assert torch.equal(_bits(dx), _bits(_expect(gv, drop, thr)))
    if kind.isdigit():   # the result is again a zero-padded view of a padded buffer, whatever the input's pads held
        npad = int(kind)
        assert getattr(y, "_ldnn_zpad", False)
        assert not _pad_columns(y.detach(), npad).any()
        assert (_pad_columns(x.detach(), npad) == 1).all()
        # the backward launch on its own, into a buffer pre-filled with 1.0: pad columns come back 0 too
        full = torch.ones(shape[0], npad, dtype=torch.bfloat16, device="cuda")
        _ext.C().dropout_bwd(g, full[:, :shape[1]], ticket)
        assert torch.equal(_bits(full[:, :shape[1]]), _bits(dx)) and not full[:, shape[1]:].any()
    else:
        assert y.is_contiguous()
    # the second call draws the next mask
    y2 = LF.dropout(x.detach(), p, True, st)
    assert torch.equal(_bits(y2), _bits(_expect(v, _mask(1, thr, shape), thr))) and st.read()["counter"] == 2


def test_input_and_output_row_strides_may_differ():
    """The launches themselves on [5, 13] views of a [5, 16] input and a [5, 32] output (pre-filled with 1.0):
    16-byte accesses, a partial vector of 5 columns, two vectors of pad only, ld_in != ld_out."""
    shape, thr = (5, 13), 32768
    x, v = _layout("16", shape, seed=21)
    g, gv = _layout("16", shape, seed=22)
    st = LF.DropoutState(x.device, SEED, MODULE)
    st.set_rate(0.5)
    ticket = torch.zeros(8, dtype=torch.int32, device="cuda")
    ybuf, dbuf = (torch.ones(5, 32, dtype=torch.bfloat16, device="cuda") for _ in range(2))
    _ext.C().dropout_fwd(x, ybuf[:, :13], st.words, ticket)
    _ext.C().dropout_bwd(g, dbuf[:, :13], ticket)
    drop = _mask(0, thr, shape)
    assert torch.equal(_bits(ybuf[:, :13]), _bits(_expect(v, drop, thr))) and not ybuf[:, 13:].any()
    assert torch.equal(_bits(dbuf[:, :13]), _bits(_expect(gv, drop, thr))) and not dbuf[:, 13:].any()
    assert st.read()["counter"] == 1 and (ticket[4].item(), ticket[2].item()) == (0, thr)


def test_fresh_state_copies():
    """A state no rate was written into holds thr 0 and scale 1: a launch on it copies its input."""
    x, v = _layout("dense", (7, 8), seed=23)
    st = LF.DropoutState(x.device, SEED, MODULE)
    y = torch.empty_like(x)
    _ext.C().dropout_fwd(x, y, st.words, torch.zeros(8, dtype=torch.int32, device="cuda"))
    assert torch.equal(_bits(y), _bits(v)) and st.read() == dict(seed=SEED, module_index=MODULE, counter=1, thr=0)


def test_everything_dropped_at_rate_one():
    x, v = _layout("dense", (64, 120), seed=9)
    x.requires_grad_()
    st = LF.DropoutState(x.device, SEED, MODULE)
    y = LF.dropout(x, 1.0, True, st)
    (dx,) = torch.autograd.grad(y, x, torch.ones_like(y))
    assert not _bits(y).any() and not _bits(dx).any() and st.read()["counter"] == 1


def test_fp32_input_and_no_state_needed_when_off():
    x = torch.randn(9, 24, device="cuda", requires_grad=True)
    assert LF.dropout(x, 0.0, True, None) is x and LF.dropout(x, 0.5, False, None) is x
    st = LF.DropoutState(x.device, SEED, MODULE)
    y = LF.dropout(x, 0.5, True, st)
    y.sum().backward()
    drop = _mask(0, 32768, (9, 24))
    assert torch.equal(_bits(y), _bits(_expect(x.detach().cpu().bfloat16(), drop, 32768)))
    assert x.grad.dtype == torch.float32 and torch.equal(x.grad.cpu(), torch.where(drop, 0.0, 2.0))


def test_backward_uses_its_own_forwards_ticket():
    x, v = _layout("dense", (33, 1000), seed=10)
    x.requires_grad_()
    d = Dropout(0.5).train()
    reseed_dropout(d, 99)
    y1 = d(x)
    y2 = d(x)                      # the live counter has moved on
    reseed_dropout(d, 5)           # ... and so has the seed
    (dx,) = torch.autograd.grad(y1, x, torch.ones_like(y1))
    first = _mask(0, 32768, (33, 1000), seed=99, module=0)
    assert torch.equal(_bits(y2), _bits(_expect(v, _mask(1, 32768, (33, 1000), seed=99, module=0), 32768)))
    assert torch.equal(dx.cpu().float(), torch.where(first, 0.0, 2.0))


def test_graph_replay_draws_consecutive_masks():
    shape = (64, 120)
    x, v = _layout("dense", shape, seed=12)
    d = Dropout(0.5).train()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        d(x)                       # the state exists before the capture
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    assert reseed_dropout(d, 123) == 1
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        y = d(x)
    state = d.__dict__["_ldnn_drop"]
    assert state.read()["counter"] == 0          # (capturing launches nothing)
    for k in range(3):
        graph.replay()
        assert torch.equal(_bits(y), _bits(_expect(v, _mask(k, 32768, shape, seed=123, module=0), 32768))), k
    assert state.read()["counter"] == 3
    reseed_dropout(d, 123)                       # restarts the sequence without a recapture
    graph.replay()
    assert torch.equal(_bits(y), _bits(_expect(v, _mask(0, 32768, shape, seed=123, module=0), 32768)))
    reseed_dropout(d, 124)
    graph.replay()
    assert torch.equal(_bits(y), _bits(_expect(v, _mask(0, 32768, shape, seed=124, module=0), 32768)))
    d.p = 0.25                                   # the rate is state too: the host write is module.sync_rate
    d.sync_rate()
    graph.replay()
    assert torch.equal(_bits(y), _bits(_expect(v, _mask(1, 16384, shape, seed=124, module=0), 16384)))


def test_graphed_step_matches_eager_steps():
    """MLP 70-33-10 with dropout 0.5, SGD, batch 16: one eager step, then three replays against the
    same three eager steps of two more replicas, all reseeded alike.  Judged as
    tests/test_layers_gpu.py::test_graphed_step_matches_eager judges a graphed step: within the
    eager-vs-eager spread of the parameter updates plus its rounding-level floor, and pointing the same way
    (that test's SGD threshold, 0.9, or the eager runs' own agreement where that is lower)."""
    from ldnn.optim import SGD
    from ldnn.train.graphed import GraphedStep

    torch.manual_seed(0)
    ms = [MLP(70, (33,), 10, dropout=0.5) for _ in range(3)]
    xavier_init(ms[0])
    for m in ms[1:]:
        m.load_state_dict(ms[0].state_dict())
    for m in ms:
        ldnn.prepare(m, "cuda")
        assert reseed_dropout(m, 2025) == 1
    os_ = [SGD(m.parameters(), lr=0.05, momentum=0.9) for m in ms]
    crit = CrossEntropyLoss()
    g = torch.Generator(device="cuda").manual_seed(1)
    xs = [torch.randn(16, 70, device="cuda", generator=g).bfloat16() for _ in range(4)]
    ys = [torch.randint(0, 10, (16,), device="cuda", generator=g) for _ in range(4)]
    for m, o in zip(ms, os_):
        o.zero_grad()
        crit(m(xs[0]), ys[0]).backward()
        o.step()
    p0 = [q.detach().clone() for q in ms[1].parameters()]
    gs = GraphedStep(ms[0], crit, os_[0], xs[1], ys[1], warmup=0)
    for i in range(1, 4):
        gs(xs[i], ys[i])
        for m, o in zip(ms[1:], os_[1:]):
            o.zero_grad()
            crit(m(xs[i]), ys[i]).backward()
            o.step()
    torch.cuda.synchronize()
    # the captured step holds the dropout launch: only the kernel advances the counter on the GPU
    assert [m.drops[0].__dict__["_ldnn_drop"].read()["counter"] for m in ms] == [4, 4, 4]
    for (n, p), q, s, r in zip(ms[0].named_parameters(), ms[1].parameters(), ms[2].parameters(), p0):
        d1, d2, d3 = ((t.detach() - r).flatten().double() for t in (p, q, s))
        eg, ee = (d1 - d2).norm().item(), (d3 - d2).norm().item()
        print(f"{n}: graphed-eager {eg:.3e}  eager-eager {ee:.3e}  update {d2.norm().item():.3e}")
        assert d2.norm().item() > 0
        assert eg <= 3.0 * ee + 2e-3 * d2.norm().item(), (n, eg, ee, d2.norm().item())
        cos = torch.nn.functional.cosine_similarity(d1, d2, dim=0).item()
        cos_ee = torch.nn.functional.cosine_similarity(d3, d2, dim=0).item()
        assert cos > (0.9 if cos_ee >= 0.9 else cos_ee - 0.3), (n, cos, cos_ee)


def test_cnn_places_dropout_in_front_of_the_classifier():
    """enhanced_cnn_small with dropout 0.5, batch 8: one training step on the GPU against the same step
    on the CPU twin path (equal seeds: the same elements are dropped), with the tolerances of
    tests/test_layers_gpu.py::test_cnn_native_matches_cpu_fp32; the eval forward is the dropout-free
    model's."""
    torch.manual_seed(0)
    m = build_model("enhanced_cnn_small", dropout=0.5)
    xavier_init(m)
    ref, plain = build_model("enhanced_cnn_small", dropout=0.5), build_model("enhanced_cnn_small")
    ref.load_state_dict(m.state_dict())
    plain.load_state_dict(m.state_dict())
    with torch.no_grad():
        for q in ref.parameters():
            q.copy_(q.bfloat16().float())
    ldnn.prepare(m, "cuda")
    ldnn.prepare(plain, "cuda")
    ldnn.prepare(ref, "cpu")
    x = torch.randn(8, 3, 32, 32)
    y = torch.randint(0, 10, (8,))
    xg = x.cuda().bfloat16()
    with torch.no_grad():
        assert torch.equal(m.eval()(xg), plain.eval()(xg))
    m.train()
    ref.train()
    assert reseed_dropout(m, 31) == 1 and reseed_dropout(ref, 31) == 1
    out = m(xg)
    lo = CrossEntropyLoss()(out, y.cuda())
    lo.backward()
    ro = ref(x.bfloat16().float())
    lr_ = CrossEntropyLoss()(ro, y)
    lr_.backward()
    assert m.drop.__dict__["_ldnn_drop"].read()["counter"] == 1 == ref.drop.__dict__["_ldnn_drop"].read()["counter"]
    torch.testing.assert_close(out.float().cpu(), ro.detach(), rtol=5e-2, atol=5e-2 * ro.abs().max().item())
    assert abs(lo.item() - lr_.item()) < 0.05 * max(1.0, lr_.item())
    for (n, p), (_, q) in zip(m.named_parameters(), ref.named_parameters()):
        g, h = p.grad.float().cpu().flatten(), q.grad.flatten()
        cos = torch.nn.functional.cosine_similarity(g, h, dim=0).item()
        assert cos > 0.98, (n, cos)


def test_graphed_dp_chain_matches_the_single_graph():
    """LeNet-5 with dropout 0.5 (two modules) under GraphedDPStep on a world of one, segmented chain cut at
    three buckets, against GraphedStep on a replica reseeded alike: the tickets cross the chain's links,
    and both steps draw the same masks (the criterion of tests/test_graphed_dp_gpu.py::_close_updates)."""
    from ldnn.optim import SGD
    from ldnn.parallel.comm import LocalComm
    from ldnn.parallel.ddp import DataParallel
    from ldnn.train.graphed import GraphedDPStep, GraphedStep

    torch.manual_seed(0)
    m1, m2 = build_model("lenet5", dropout=0.5), build_model("lenet5", dropout=0.5)
    xavier_init(m1)
    m2.load_state_dict(m1.state_dict())
    for m in (m1, m2):
        ldnn.prepare(m, "cuda")
    crit = CrossEntropyLoss()
    dp = DataParallel(m1, LocalComm(), bucket_cap_mb=0.05, broadcast_init=False)
    assert len(dp.bucketer.buckets) >= 3
    assert reseed_dropout(dp, 77) == 2 and reseed_dropout(m2, 77) == 2       # (through the wrapper too)
    o1, o2 = SGD(m1.parameters(), lr=0.02, momentum=0.9), SGD(m2.parameters(), lr=0.02, momentum=0.9)
    g = torch.Generator(device="cuda").manual_seed(1)
    xs = [torch.randn(64, 1, 28, 28, device="cuda", generator=g).bfloat16() for _ in range(4)]
    ys = [torch.randint(0, 10, (64,), device="cuda", generator=g) for _ in range(4)]
    p0 = [p.detach().clone() for p in m2.parameters()]
    for m, o in ((m1, o1), (m2, o2)):
        o.zero_grad()
        crit(m(xs[0]), ys[0]).backward()
        o.step()
    gd = GraphedDPStep(dp, crit, o1, xs[0], ys[0], mode="segmented")
    gs = GraphedStep(m2, crit, o2, xs[0], ys[0], warmup=0)
    for i in range(1, 4):
        gd(xs[i], ys[i])
        gs(xs[i], ys[i])
    torch.cuda.synchronize()
    for m in (m1, m2):
        assert [d.__dict__["_ldnn_drop"].read()["counter"] for d in (m.drop1, m.drop2)] == [4, 4]
    for a, b, r in zip(m1.parameters(), m2.parameters(), p0):
        da, db = (a.detach() - r).double(), (b.detach() - r).double()
        assert (da - db).norm().item() <= 2e-2 * db.norm().item() + 1e-6, ((da - db).norm().item(), db.norm().item())
