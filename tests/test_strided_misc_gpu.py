"""The other bindings that read a row stride -- classifier heads, the pooled head, the fused
softmax cross-entropy, the bf16 transpose, the slab column sum -- on strided operands with
poisoned padding: tests/strided.py's three steps (dense run held to the fp64 / fp32 reference
with the neighbouring dense test's bound; the same on NaN / sentinel padded views, 16-B aligned
and no more, with every buffer's padding checked bit for bit; strided == dense where the path
has no atomics).

Pads that are zero BY CONTRACT (they are inside the operand's extent; everything beyond them is
poisoned), with the line that states each:
  * head W rows [ncls, rows): "[ldw_rows][ldw] bf16 weight (rows >= C zero-padded)",
    csrc/include/ldnn_kernels.h:574; the head bias likewise, "[ld] fp32 (zero-padded)", :575.
  * dlogits columns [ncls, 16) read by head_dgrad_stream / head_bwd: "padded classes hold 0",
    csrc/kernels/head.hip:467; the xent kernels write them so ("padded columns 0",
    csrc/include/ldnn_kernels.h:352).
  * softmax_xent writes ALL ld columns of each dlogits row, pad = 0 (csrc/bindings.cpp:530-531),
    so its dlogits buffer is padded with rows only and dlogits[:, C:ld] must come back 0.
head_wgrad's dz is a dense [B][ld] matrix (csrc/bindings.cpp:1136): its columns [rows, ld) are
operand data, not padding, and are zero here as in test_kernels_gpu.py::test_head_wgrad.
"""
import pytest
import torch
import torch.nn.functional as F

import ldnn  # noqa: F401
from ldnn.ops import _ext
from strided import T, three_steps

pytestmark = pytest.mark.gpu

PADS = [("min", 0), ("eng", 3)]     # (leading-dimension style, rows in front)


def C():
    return _ext.C()


def _gen(seed):
    return torch.Generator(device="cuda").manual_seed(seed)


def _head_ops(B, K, ncls, ld, act, seed):
    g = _gen(seed)
    h = torch.randn(B, K, device="cuda", generator=g)
    h = (h.relu() if act == "drelu" else h.sigmoid() if act == "dsigmoid" else h).bfloat16()
    W = torch.zeros(ld, K, device="cuda")
    W[:ncls] = torch.randn(ncls, K, device="cuda", generator=g) * K ** -0.5
    bias = torch.zeros(ld, device="cuda")
    bias[:ncls] = torch.randn(ncls, device="cuda", generator=g)
    y = torch.randint(0, ncls, (B,), device="cuda", generator=g)
    return h, W.bfloat16(), bias, y


def _dgrad_ref(dl, W, h, ncls, act):
    ref = dl.double()[:, :ncls] @ W.double()[:ncls]
    hd = h.double()
    return ref * (hd > 0) if act == "drelu" else ref * hd * (1 - hd) if act == "dsigmoid" else ref


@pytest.mark.parametrize("style,before", PADS)
@pytest.mark.parametrize("B", [70, 333])
@pytest.mark.parametrize("ncls,ld", [(10, 16), (40, 48)])
def test_head_fwd_xent(B, ncls, ld, style, before):
    K = 520
    h, W, bias, y = _head_ops(B, K, ncls, ld, "none", 1)
    spec = {"h": T("in", h), "W": T("in", W), "logits": T("dense", shape=(B, ld), dtype=torch.bfloat16),
            "dl": T("dense", shape=(B, ld), dtype=torch.bfloat16),
            "stats": T("dense", torch.zeros((B + 15) // 16, 2, device="cuda"))}
    ref = h.double() @ W.double().t() + bias.double()

    def check(t):
        logits, dl = t["logits"], t["dl"]
        assert ((logits.double() - ref).abs().max() / ref.abs().max()).item() < 1e-2
        assert logits[:, ncls:].float().abs().max().item() == 0.0
        lr = logits.float()[:, :ncls]
        loss = F.cross_entropy(lr, y, reduction="sum")
        s = t["stats"].sum(0)
        assert abs(s[0].item() - loss.item()) <= 1e-3 * loss.item() + 1e-2
        assert s[1].item() == (lr.argmax(1) == y).sum().item()
        gr = (torch.softmax(lr, 1) - F.one_hot(y, ncls).float()) / B
        assert (dl.float()[:, :ncls] - gr).abs().max().item() < 2e-2 / B + 1e-6
        assert dl[:, ncls:].float().abs().max().item() == 0.0

    three_steps(spec, lambda t: C().head_fwd_xent(t["h"], t["W"], bias, y, t["logits"], t["dl"], t["stats"], ncls,
                                                  1.0 / B), check, style, before)


@pytest.mark.parametrize("style,before", PADS)
@pytest.mark.parametrize("B", [70, 333])
@pytest.mark.parametrize("ncls,ld,mode,act", [(10, 16, 0, "drelu"), (10, 16, 1, "drelu"), (10, 16, 2, "drelu"),
                                              (40, 48, 1, "drelu"), (40, 48, 2, "dsigmoid"), (10, 16, 0, "none")])
def test_head_fwd_xent_fused_dgrad(B, ncls, ld, mode, act, style, before):
    """dgrad_mode 0 (forward, then the streaming dgrad), 1 (fused, h re-read), 2 (fused, h from
    LDS) with strided h, W and dh; dbias is longer than K."""
    c = C()
    K = 520
    h, W, bias, y = _head_ops(B, K, ncls, ld, act, 2)
    code = {"drelu": c.EPI_DRELU, "dsigmoid": c.EPI_DSIGMOID, "none": c.EPI_NONE}[act]
    spec = {"h": T("in", h), "W": T("in", W), "dl": T("dense", shape=(B, ld), dtype=torch.bfloat16),
            "stats": T("dense", torch.zeros((B + 15) // 16, 2, device="cuda")),
            "dh": T("out", shape=(B, K), dtype=torch.bfloat16),
            "dbias": T("out", torch.zeros(K, device="cuda"), exact=False),
            "ws": T("dense", shape=(c.head_dgrad_ws_floats(B, K),), dtype=torch.float32)}

    def check(t):
        ref = _dgrad_ref(t["dl"], W, h, ncls, act)
        assert (t["dh"].double() - ref).abs().max().item() <= 1e-2 * ref.abs().max().item()
        cs = t["dh"].float().sum(0)
        torch.testing.assert_close(t["dbias"], cs, rtol=1e-3, atol=1e-4 * cs.abs().max().item())

    dense, _ = three_steps(spec, lambda t: c.head_fwd_xent(t["h"], t["W"], bias, y, None, t["dl"], t["stats"], ncls,
                                                           1.0 / B, dh=t["dh"], dbias=t["dbias"], dgrad_epi=code,
                                                           dbias_ws=t["ws"], dgrad_mode=mode), check, style, before)
    dl2 = torch.empty(B, ld, device="cuda", dtype=torch.bfloat16)
    st2 = torch.zeros((B + 15) // 16, 2, device="cuda")
    c.head_fwd_xent(h, W, bias, y, None, dl2, st2, ncls, 1.0 / B)       # the loss path is unchanged by the dgrad
    assert torch.equal(dense["dl"], dl2) and torch.equal(dense["stats"], st2)


def _dlogits(B, ncls, seed):
    dl = torch.zeros(B, 16, device="cuda", dtype=torch.bfloat16)
    dl[:, :ncls] = (torch.randn(B, ncls, device="cuda", generator=_gen(seed)) / B).bfloat16()
    return dl


@pytest.mark.parametrize("style,before", PADS)
@pytest.mark.parametrize("B", [70, 333])
@pytest.mark.parametrize("act", ["drelu", "dsigmoid", "none"])
def test_head_dgrad_stream(B, act, style, before):
    c = C()
    K, ncls = 520, 10
    h, W, _, _ = _head_ops(B, K, ncls, 16, act, 3)
    dl = _dlogits(B, ncls, 4)
    code = {"drelu": c.EPI_DRELU, "dsigmoid": c.EPI_DSIGMOID, "none": c.EPI_NONE}[act]
    ref = _dgrad_ref(dl, W, h, ncls, act)
    spec = {"h": T("in", h), "W": T("in", W), "dh": T("out", shape=(B, K), dtype=torch.bfloat16),
            "dbias": T("out", torch.zeros(K, device="cuda"), exact=False)}

    def check(t):
        torch.testing.assert_close(t["dh"].double(), ref, rtol=1e-2, atol=1e-6)
        torch.testing.assert_close(t["dbias"], t["dh"].float().sum(0), rtol=1e-4, atol=1e-6)

    three_steps(spec, lambda t: c.head_dgrad_stream(t["h"], t["W"], dl, t["dh"], t["dbias"], code), check, style,
                before)


@pytest.mark.parametrize("style,before", PADS)
@pytest.mark.parametrize("B", [70, 333])
@pytest.mark.parametrize("relu", [True, False])
def test_head_bwd(B, relu, style, before):
    """Fused head dgrad + wgrad (K % 64 == 0): strided h, W, dh and dW; dW / dbias / db are
    accumulated with atomics (bound only), dh is a plain store (bit equality)."""
    c = C()
    K, ncls = 576, 10
    act = "drelu" if relu else "none"
    h, W, _, _ = _head_ops(B, K, ncls, 16, act, 5)
    dl = _dlogits(B, ncls, 6)
    ref = _dgrad_ref(dl, W, h, ncls, act)
    dW_ref = dl.double().t() @ h.double()
    spec = {"h": T("in", h), "W": T("in", W), "dh": T("out", shape=(B, K), dtype=torch.bfloat16),
            "dW": T("out", torch.zeros(16, K, device="cuda"), exact=False),
            "dbias": T("out", torch.zeros(K, device="cuda"), exact=False),
            "db": T("out", torch.zeros(16, device="cuda"), exact=False)}

    def check(t):
        torch.testing.assert_close(t["dh"].double(), ref, rtol=1e-2, atol=1e-2 * ref.abs().max().item())
        torch.testing.assert_close(t["dbias"], t["dh"].float().sum(0), rtol=1e-3,
                                   atol=1e-3 * t["dbias"].abs().max().item())
        torch.testing.assert_close(t["dW"].double(), dW_ref, rtol=1e-3, atol=1e-3 * dW_ref.abs().max().item())
        torch.testing.assert_close(t["db"].double(), dl.double().sum(0), rtol=1e-3, atol=1e-6)

    three_steps(spec, lambda t: c.head_bwd(t["h"], t["W"], dl, t["dh"], t["dW"], t["dbias"],
                                           c.EPI_DRELU if relu else c.EPI_NONE, t["db"]), check, style, before)


@pytest.mark.parametrize("style,before", PADS)
@pytest.mark.parametrize("splits", [1, 3])
@pytest.mark.parametrize("B,ld,rows", [(70, 16, 16), (333, 16, 10), (333, 48, 40)])
def test_head_wgrad(B, ld, rows, splits, style, before):
    """dW = dz^T h with strided h and dW (rows <= ld); one split stores (bit equality), several
    accumulate with atomics into the cleared gradient (bound only)."""
    K = 520
    g = _gen(7)
    dz = torch.randn(B, ld, device="cuda", generator=g)
    dz[:, rows:] = 0
    dz = dz.bfloat16()
    h = torch.randn(B, K, device="cuda", generator=g).bfloat16()
    ref = dz.double()[:, :rows].t() @ h.double()
    spec = {"h": T("in", h), "dW": T("out", torch.zeros(rows, K, device="cuda"), exact=splits == 1),
            "db": T("out", torch.zeros(rows, device="cuda"), exact=splits == 1)}

    def check(t):
        assert ((t["dW"].double() - ref).abs().max() / ref.abs().max()).item() < 1e-4
        assert (t["db"].double() - dz.double()[:, :rows].sum(0)).abs().max().item() < 1e-2

    three_steps(spec, lambda t: C().head_wgrad(dz, t["h"], t["dW"], t["db"], splits), check, style, before)


@pytest.mark.parametrize("style,before", PADS)
@pytest.mark.parametrize("N,Cc,HW,ncls", [(5, 64, 9, 1), (8, 512, 49, 16), (8, 512, 49, 10)])
def test_gap_linear_fwd_bwd(N, Cc, HW, ncls, style, before):
    """Pooled classifier head: w / logits (forward) and g / w / dw (backward) are [ncls][C] resp.
    [N][ncls] views of wider buffers; x, pooled and dx are dense by contract
    (csrc/bindings.cpp:2026-2028,2054-2056).  Bounds of test_gap_head_gpu.py; the pooled means are
    bf16 roundings of fp32 means of O(1) values (2^-8 relative)."""
    c = C()
    assert c.gap_linear_ok(N, HW, Cc, ncls)
    g = _gen(8)
    x = torch.randn(N, HW, Cc, device="cuda", generator=g).bfloat16()
    w = (torch.randn(ncls, Cc, device="cuda", generator=g) * Cc ** -0.5).bfloat16()
    b = torch.randn(ncls, device="cuda", generator=g)
    pooled_ref = x.double().mean(1)
    spec = {"w": T("in", w), "pooled": T("dense", shape=(N, Cc), dtype=torch.bfloat16),
            "logits": T("out", shape=(N, ncls), dtype=torch.bfloat16, ld=24 + 8 * (style == "eng"), col0=0)}

    def check(t):
        torch.testing.assert_close(t["pooled"].double(), pooled_ref, rtol=1e-2, atol=1e-2)
        ref = t["pooled"].double() @ w.double().t() + b.double()    # the Linear reads the stored bf16 means
        torch.testing.assert_close(t["logits"].double(), ref, rtol=2e-2, atol=2e-2 * ref.abs().max().item())

    dense, _ = three_steps(spec, lambda t: c.gap_linear_fwd(x, t["w"], b, t["pooled"], t["logits"], ncls), check,
                           style, before)
    pooled = dense["pooled"]
    gy = (torch.randn(N, ncls, device="cuda", generator=g) / N).bfloat16()
    dw_ref = gy.double().t() @ pooled.double()
    dx_ref = (gy.double() @ w.double() / HW)[:, None, :].expand(N, HW, Cc)
    spec2 = {"g": T("in", gy, ld=24 + 8 * (style == "eng"), col0=0), "w": T("in", w),
             "dw": T("out", shape=(ncls, Cc), dtype=torch.float32), "db": T("out", shape=(ncls,), dtype=torch.float32),
             "dx": T("dense", shape=(N, HW, Cc), dtype=torch.bfloat16)}

    def check2(t):
        torch.testing.assert_close(t["dw"].double(), dw_ref, rtol=2e-2, atol=1e-2 * dw_ref.abs().max().item())
        torch.testing.assert_close(t["db"].double(), gy.double().sum(0), rtol=2e-2, atol=2e-2)
        torch.testing.assert_close(t["dx"].double(), dx_ref, rtol=2e-2, atol=1e-2 * dx_ref.abs().max().item())

    three_steps(spec2, lambda t: c.gap_linear_bwd(t["g"], pooled, t["w"], t["dw"], t["db"], t["dx"], ncls), check2,
                style, before)


def _xent_check(B, Cc, lf_grad, loss_ref, correct):
    def check(t):
        dl = t["dl"]
        torch.testing.assert_close(t["stats"][0] / B, loss_ref, rtol=1e-4, atol=1e-4)
        assert t["stats"][1].item() == correct
        torch.testing.assert_close(dl[:, :Cc].float(), lf_grad, rtol=2e-2, atol=1e-4)
        assert dl[:, Cc:].float().abs().max().item() == 0.0       # pad columns come back 0
        torch.testing.assert_close(t["db"][:Cc], dl[:, :Cc].float().sum(0), rtol=1e-3, atol=1e-5)
    return check


@pytest.mark.parametrize("before", [0, 3])
@pytest.mark.parametrize("B", [70, 300])
@pytest.mark.parametrize("Cc,ld", [(10, 16), (100, 104)])
@pytest.mark.parametrize("soft", [False, True])
def test_softmax_xent(soft, Cc, ld, B, before):
    """The rows kernel (C = 10, ld = 16) and the wave kernel (C = 100, ld = 104): NaN in the pad
    columns of the logits and of the soft targets (ldq > C) and in the rows around both."""
    g = _gen(9)
    logits = torch.randn(B, Cc, device="cuda", generator=g).bfloat16()
    labels = torch.randint(0, Cc, (B,), device="cuda", generator=g)
    q = torch.softmax(torch.randn(B, Cc, device="cuda", generator=g), 1)
    lf = logits.float().requires_grad_(True)
    loss = F.cross_entropy(lf, q if soft else labels)
    loss.backward()
    correct = (logits.float().argmax(1) == (q.argmax(1) if soft else labels)).sum().item()
    spec = {"logits": T("in", logits, ld=ld, col0=0), "q": T("in", q, aligned=False),   # (the binding asks no alignment of the targets)
            "dl": T("out", shape=(B, ld), dtype=torch.bfloat16, full_rows=True),
            "stats": T("dense", torch.zeros(2, device="cuda"), exact=False),
            "db": T("out", torch.zeros(ld, device="cuda"), exact=False)}

    def call(t):
        lg = t["logits"]
        if lg.stride(0) != ld:      # the dense run: the [B][C] view of a zero-padded dense [B][ld] buffer,
            full = torch.zeros(B, ld, device="cuda", dtype=torch.bfloat16)   # as test_softmax_xent_matches_torch
            full[:, :Cc] = lg
            lg = full[:, :Cc]
        if soft:
            C().softmax_xent_soft(lg, t["q"], t["dl"][:, :Cc], t["stats"], dbias=t["db"], num_classes=Cc,
                                  grad_scale=1.0 / B)
        else:
            C().softmax_xent(lg, labels, t["dl"][:, :Cc], t["stats"], dbias=t["db"], num_classes=Cc,
                             grad_scale=1.0 / B)

    three_steps(spec, call, _xent_check(B, Cc, lf.grad, loss.detach(), correct), "min", before)


@pytest.mark.parametrize("style,before", PADS)
@pytest.mark.parametrize("r,cc", [(8, 1032), (1032, 8), (72, 136)])
def test_transpose_bf16(r, cc, style, before):
    x = torch.randn(r, cc, device="cuda", generator=_gen(10)).bfloat16()
    spec = {"x": T("in", x), "out": T("out", shape=(cc, r), dtype=torch.bfloat16)}

    def check(t):
        assert torch.equal(t["out"], x.t())

    three_steps(spec, lambda t: C().transpose_bf16(t["x"], t["out"]), check, style, before)


@pytest.mark.parametrize("style,before", PADS)
def test_slab_sum_cols(style, before):
    """ws [3][264][792] (dense by contract) summed into a [264][784] view of a wider buffer, column
    784 into `extra`."""
    ws = torch.randn(3, 264, 792, device="cuda", generator=_gen(11))
    tot = ws.double().sum(0)
    spec = {"out": T("out", shape=(264, 784), dtype=torch.float32), "extra": T("out", shape=(264,), dtype=torch.float32)}

    def check(t):
        torch.testing.assert_close(t["out"].double(), tot[:, :784], rtol=1e-6, atol=1e-5)
        torch.testing.assert_close(t["extra"].double(), tot[:, 784], rtol=1e-6, atol=1e-5)

    three_steps(spec, lambda t: C().slab_sum_cols(ws, t["out"], t["extra"]), check, style, before)
