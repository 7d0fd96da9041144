"""The fp8 Linear on the GPU: the cast kernels bit for bit against the recipe in torch on the CPU, gemm_f8
against fp64 on operands the kernel under test did not make, Linear(compute_dtype="fp8") against its CPU twin."""
import math

import pytest
import torch

import ldnn
from ldnn.models import CrossEntropyLoss, build_model, xavier_init
from ldnn.models.layers import Linear
from ldnn.ops import _ext
from ldnn.ops import functional as LF
from strided import assert_outside_untouched, poisoned, strided_like, write_inside

pytestmark = pytest.mark.gpu
FMT = {"e4m3": (448.0, torch.float8_e4m3fn, 0), "e5m2": (57344.0, torch.float8_e5m2, 1)}
EPS = 2.0 ** -23
# K_pad 2^-23 |A| @ |B|^T bounds a dot product added in fp32.  The MI355X's f8f6f4 MFMA does not add that way: it
# sums each group of 16 products with an aligned adder that truncates about 14 bits below the group's largest
# product (+1 -1 +2^-14 in one group gives 0, 2^-13 survives, a product in another group is added exactly).  On
# correct code the worst error against fp64 measured 25.2 times that bound (256 random fp32-out cases, K = 8 ..
# 2048, both formats; 3.8e-4 of |A| @ |B|^T, nearly independent of K: profiles/r25/README.md,
# accum_vs_fp64.jsonl).  The first term is widened to twice that ratio.
HW = 2 * 25.2
# The sigmoid epilogue's allowance for the device's fast exponential, beyond the propagated accumulation bound and the
# bf16 rounding of the result: test_gemm_f8_against_fp64's docstring.  Measured: no excess (the worst err - bound over
# the 32 sigmoid cases of the two files was -9.2e-6), so the figure is 0.
SIGMOID_EXCESS = 0.0
FAST_EXP = 2 * SIGMOID_EXCESS


def up128(v):
    return (v + 127) // 128 * 128


def quantize_ref(t, fmt):
    """The recipe on the CPU: (fp8 codes [R, C], the same as uint8 padded to 128 with code 0, amax, s)."""
    fmax, dt, _ = FMT[fmt]
    tf = t.detach().float().cpu()
    amax = tf.abs().max()
    if not torch.isfinite(amax):
        s = float("nan")
    elif amax == 0:
        s = 1.0
    else:
        m, ex = torch.frexp(amax)            # amax = m 2^ex, m in [0.5, 1); fmax = 0.875 2^q
        s = 2.0 ** min(math.frexp(fmax)[1] - int(ex) - int(m > 0.875), 126)
    codes = (tf * s).clamp(-fmax, fmax).to(dt)
    padded = torch.zeros(up128(t.shape[0]), up128(t.shape[1]), dtype=torch.uint8)
    padded[:t.shape[0], :t.shape[1]] = codes.view(torch.uint8)
    return codes, padded, amax.item(), s


CAST_CASES = [("randn", 1, 8), ("randn", 64, 64), ("randn", 65, 136), ("randn", 200, 72),
              ("zero", 65, 136), ("inf", 65, 136), ("boundary", 65, 136)]


@pytest.mark.parametrize("strided", [False, True])
@pytest.mark.parametrize("fmt", ["e4m3", "e5m2"])
@pytest.mark.parametrize("kind,R,C", CAST_CASES)
def test_casts_bit_for_bit(kind, R, C, fmt, strided):
    torch.manual_seed(R + C)
    t = (torch.randn(R, C) * 3).bfloat16()
    if kind == "zero":
        t.zero_()
    elif kind == "inf":
        t[R // 2, C // 2] = float("inf")
    elif kind == "boundary":   # amax exactly fmt_max * 2^-3: e = 3 must be taken
        t = t.clamp(-1, 1)
        t[R - 1, C - 1] = -FMT[fmt][0] / 8
    src = t.cuda()
    if strided:   # a [R, C] view of a wider buffer whose pad columns (and rows around) hold NaN
        src, _ = strided_like(src, ld=C + 24, before=1, col0=8)
    codes, codes_t, words = LF.fp8_quantize(src, fmt)
    torch.cuda.synchronize()
    _, ref, amax, s = quantize_ref(t, fmt)
    w = words.cpu()
    if kind == "inf":
        assert math.isinf(w[0].item()) and torch.isnan(w[1:3]).all()
        return
    assert torch.equal(w[:3].view(torch.int32), torch.tensor([amax, s, 1.0 / s]).view(torch.int32)), (w, amax, s)
    assert torch.equal(codes.cpu(), ref)          # logical codes and every pad byte (0)
    assert torch.equal(codes_t.cpu(), ref.t())
    if kind == "zero":
        assert w[1].item() == 1.0 and not codes.any()
    if kind == "boundary":
        assert s == 8.0


@pytest.mark.parametrize("out_kind", ["bf16_bias_relu", "bf16_bias", "bf16_bias_sigmoid", "bf16_none", "f32_beta0",
                                      "f32_beta1"])
@pytest.mark.parametrize("M,N,K", [(5, 8, 8), (128, 128, 128), (136, 264, 200), (300, 136, 784)])
@pytest.mark.parametrize("fmt", ["e4m3", "e5m2"])
def test_gemm_f8_against_fp64(fmt, M, N, K, out_kind):
    """|out - r| <= HW K_pad 2^-23 (|A| @ |B|^T) / (s_a s_b) + rnd (HW: above; 1 if the pipe added in fp32, products of
    two fp8 values being exact there); rnd = 2^-8 |r| (bf16 out) or 2^-23 (|r| + |beta C|) (fp32 out).  A wrong
    fragment or row mapping misses by |A| @ |B|^T itself.  bf16_bias_sigmoid: r = sigmoid(r + bias) in fp64 and the
    first term divided by 4 (sigmoid's Lipschitz constant), plus FAST_EXP for the device's fast exponential: twice
    the worst excess over the propagated bound measured on the kernels before the two files were merged, SIGMOID_EXCESS
    over these cases and test_mxfp8_gpu.py's.  No case exceeded it (worst err - bound -9.2e-6, worst err / bound
    0.991), so SIGMOID_EXCESS = 0 and FAST_EXP = 0 (profiles/r28/README.md)."""
    torch.manual_seed(M + N + K)
    C = _ext.C()
    ac, a8, _, sa = quantize_ref(torch.randn(M, K).bfloat16(), fmt)
    bc, b8, _, sb = quantize_ref(torch.randn(N, K).bfloat16(), "e4m3")
    wa = torch.tensor([0.0, sa, 1.0 / sa, 0.0], device="cuda")
    wb = torch.tensor([0.0, sb, 1.0 / sb, 0.0], device="cuda")
    A, B = ac.double(), bc.double()
    r = (A @ B.t()) / (sa * sb)
    bound = HW * up128(K) * EPS * (A.abs() @ B.abs().t()) / (sa * sb)
    f32 = out_kind.startswith("f32")
    out, h = poisoned(M, N, ld=N + 8, before=1, dtype=torch.float32 if f32 else torch.bfloat16, device="cuda",
                      fill="sentinel")
    if f32:
        beta = float(out_kind[-1])
        c0 = torch.randn(M, N)
        write_inside(out, c0.cuda())
        r = r + beta * c0.double()
        bound = bound + EPS * (r.abs() + (beta * c0).abs().double())
        C.gemm_f8(a8.cuda(), b8.cuda(), out, wa, wb, FMT[fmt][2], C.EPI_NONE, beta=beta)
    else:
        if out_kind != "bf16_none":
            bias = torch.randn(N)
            r = r + bias.double()
            epi = {"bf16_bias_relu": C.EPI_BIAS_RELU, "bf16_bias": C.EPI_BIAS, "bf16_bias_sigmoid": C.EPI_BIAS_SIGMOID}
            if out_kind == "bf16_bias_relu":
                r = r.clamp_min(0)
            elif out_kind == "bf16_bias_sigmoid":
                r, bound = torch.sigmoid(r), bound / 4 + FAST_EXP
            C.gemm_f8(a8.cuda(), b8.cuda(), out, wa, wb, FMT[fmt][2], epi[out_kind], bias=bias.cuda())
        else:
            C.gemm_f8(a8.cuda(), b8.cuda(), out, wa, wb, FMT[fmt][2], C.EPI_NONE)
        bound = bound + 2.0 ** -8 * r.abs()
    torch.cuda.synchronize()
    err = (out.cpu().double() - r).abs()
    print("worst err / bound", (err / bound.clamp_min(1e-300)).max().item())
    if out_kind == "bf16_bias_sigmoid":
        print("sigmoid excess over the propagated bound", (err - (bound - FAST_EXP)).max().item())
    assert (err <= bound).all(), ((err - bound).max().item(), (err / (A.abs() @ B.abs().t())).max().item())
    assert_outside_untouched(h, "gemm_f8 out")


@pytest.mark.parametrize("bias", [True, False])
@pytest.mark.parametrize("act", ["relu", "none"])
@pytest.mark.parametrize("B,K,N", [(8, 33, 40), (130, 784, 136)])
def test_linear_fp8_against_cpu_twin(B, K, N, act, bias):
    """Two forward + backward passes without a zero_grad in between (the second accumulates: grad_beta) on the GPU
    and in the CPU twin, same weights, input and bf16 upstream gradient, so both quantise to the same codes.  Each
    result may differ by gemm_f8's accumulation bound plus the twin's own fp32 matmul error (the same expression
    without HW: (HW + 1) K_pad 2^-23 |a| @ |b|, with |quantised| <= 1.2 |unquantised| for both formats) plus the
    output rounding."""
    torch.manual_seed(B + K + N)
    lg = Linear(K, N, bias=bias, activation=act, compute_dtype="fp8")
    lc = Linear(K, N, bias=bias, activation=act, compute_dtype="fp8")
    lc.load_state_dict(lg.state_dict())
    flat = ldnn.prepare(lg, "cuda")
    x, gy = torch.randn(B, K).bfloat16(), torch.randn(B, N).bfloat16()
    xg, xc = x.cuda().requires_grad_(), x.float().requires_grad_()
    for _ in range(2):
        yg, yc = lg(xg), lc(xc)
        yg.backward(gy.cuda())
        yc.backward(gy.float())
    torch.cuda.synchronize()
    w = lc.weight.detach().bfloat16().double().abs()
    xa, ga = x.double().abs(), gy.double().abs()

    def close(got, ref, absprod, kdim, rnd, passes):
        tol = passes * (HW + 1) * up128(kdim) * EPS * 1.2 * absprod + rnd * ref.abs().double() + 1e-30
        err = (got.detach().cpu().double() - ref.detach().double()).abs()
        assert (err <= tol).all(), (err / tol).max().item()

    close(yg, yc, xa @ w.t(), K, 2.0 ** -8, 1)
    close(xg.grad, xc.grad, ga @ w, N, 2.0 ** -8, 2)
    dw = flat.grad_storage(lg.weight)
    close(dw[:N, :K], lc.weight.grad, ga.t() @ xa, B, 2.0 ** -22, 2)
    assert dw[N:].abs().max().item() == 0.0 if dw.shape[0] > N else True
    assert dw[:, K:].abs().max().item() == 0.0 if dw.shape[1] > K else True
    assert lc.weight.grad.abs().max() > 0
    if bias:   # column sums of the bf16 gz in fp32 on both sides
        close(lg.bias.grad, lc.bias.grad, ga.sum(0), B, 2.0 ** -22, 2)


def test_mlp3_small_fp8_graphed_equals_eager(monkeypatch):
    """Three replays of a captured mlp3_small step with linear_dtype="fp8" against the same steps run eagerly, to
    the tolerance of test_layers_gpu's graphed-vs-eager test (within the eager-vs-eager spread of the updates plus
    a rounding-level floor).  One eager step issues 5 gemm_f8 launches (two hidden layers: forward and wgrad, the
    second also dgrad) and the output layer's 3 bf16 gemm launches, as in the bf16 model."""
    from ldnn.optim import SGD
    from ldnn.train.graphed import GraphedStep

    torch.manual_seed(0)
    ms = [build_model("mlp3_small", linear_dtype="fp8") for _ in range(3)]
    xavier_init(ms[0])
    for m in ms:
        m.load_state_dict(ms[0].state_dict())
        ldnn.prepare(m, "cuda")
    os_ = [SGD(m.parameters(), lr=0.05, momentum=0.9) for m in ms]
    crit = CrossEntropyLoss()
    gen = torch.Generator(device="cuda").manual_seed(1)
    xs = [torch.randn(64, 784, device="cuda", generator=gen).bfloat16() for _ in range(4)]
    ys = [torch.randint(0, 10, (64,), device="cuda", generator=gen) for _ in range(4)]
    calls = []
    C = _ext.C()
    for name in ("gemm", "gemm_f8"):
        monkeypatch.setattr(C, name, lambda *a, _f=getattr(C, name), _n=name, **k: (calls.append(_n), _f(*a, **k))[1])

    def eager(m, o, i):
        o.zero_grad()
        crit(m(xs[i]), ys[i]).backward()
        o.step()

    for m, o in zip(ms, os_):
        del calls[:]
        eager(m, o, 0)
    assert sorted(calls) == ["gemm"] * 3 + ["gemm_f8"] * 5
    p0 = [q.detach().clone() for q in ms[1].parameters()]
    gs = GraphedStep(ms[0], crit, os_[0], xs[1], ys[1], warmup=0)
    for i in (1, 2, 3):
        gs(xs[i], ys[i])
        eager(ms[1], os_[1], i)
        eager(ms[2], os_[2], i)
    torch.cuda.synchronize()
    for p, q, s, r in zip(*(m.parameters() for m in ms), p0):
        d1, d2, d3 = ((t.detach() - r).flatten().double() for t in (p, q, s))
        assert torch.isfinite(d1).all() and d2.norm() > 0
        assert (d1 - d2).norm().item() <= 3.0 * (d3 - d2).norm().item() + 2e-3 * d2.norm().item()
