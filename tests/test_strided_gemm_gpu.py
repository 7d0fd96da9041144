"""GEMM kernels on strided operands with poisoned padding (tests/strided.py).

Every case runs the kernel twice on the same data:
  1. on dense contiguous tensors, held to an fp64 reference with the bound of the
     neighbouring dense test (test_kernels_gpu.py / test_gemm_q_gpu.py / test_head_fused_gpu.py);
  2. on [rows][cols] views of wider buffers -- A, B, C, aux, masks, head_w, dbias and the
     optimizer state all strided at once, 16-B aligned and no more -- whose padding is NaN
     (inputs), 0xFF (input bit masks) or a sentinel bit pattern (outputs).  No NaN may reach
     an output, the same bound holds, and the padding of every buffer is bit-for-bit intact;
  3. a plain launch and the in-launch split-K combine are deterministic and the leading
     dimension does not change the arithmetic order: strided == dense, bit for bit.  Bias
     gradients (`dbias`) are finished with one atomic per column per wave and keep only
     their bound.

Shapes are the smallest with two tiles per side, a ragged second tile and a K tail behind
one full K tile.  Padding is at least a full tile of allocated rows behind every operand.

Zero-padding contracts (pads that must be zero, not ignored), as the bindings state them:
  * head_w rows [ncls, 16): "head_w must be [16][>= N] bf16 (classes zero-padded to 16)",
    csrc/bindings.cpp:130-132.  Those rows are zero here; the columns behind N are NaN.
"""
import pytest
import torch

import ldnn  # noqa: F401
from ldnn.ops import _ext
from strided import T, three_steps

pytestmark = pytest.mark.gpu

LAYOUTS = [(True, True), (True, False), (False, True), (False, False)]
PADS = [("min", 0), ("min", 3), ("eng", 0), ("eng", 3)]     # (leading-dimension style, rows in front)
PADS2 = [("min", 0), ("eng", 3)]
# (tile, variant): gemm.hip 128, gemm.hip k256 (1) and its ring experiments (2, 3), gemm_q.hip (32)
KERNELS = [(128, 0), (256, 1), (256, 2), (256, 3), (256, 32)]
SHAPES = {128: [(136, 136, 72), (136, 72, 8)], 256: [(264, 264, 72), (296, 264, 136)]}
KERNEL_SHAPES = [(t, v, s) for (t, v) in KERNELS for s in SHAPES[t]]


def C():
    return _ext.C()


def _ops(M, N, K, a_kc, b_kc, seed=0, scale_b=1.0):
    g = torch.Generator(device="cuda").manual_seed(seed)
    a = torch.randn((M, K) if a_kc else (K, M), device="cuda", generator=g).bfloat16()
    b = (torch.randn((N, K) if b_kc else (K, N), device="cuda", generator=g) * scale_b).bfloat16()
    A = a.double() if a_kc else a.double().t()
    B = b.double().t() if b_kc else b.double()
    return a, b, A @ B


def _check_plain(name, ref, K, f32):
    def check(t):
        if f32:
            err = (t[name].double() - ref).abs().max().item()
            assert err <= 1e-3 * K ** 0.5 + 1e-3, err
        else:
            err = ((t[name].double() - ref).abs().max() / ref.abs().max()).item()
            assert err < 1e-2, err
    return check


def _plain(tile, variant, M, N, K, a_kc, b_kc, style, before, f32):
    a, b, ref = _ops(M, N, K, a_kc, b_kc)
    spec = {"a": T("in", a), "b": T("in", b), "c": T("out", shape=(M, N), dtype=torch.float32 if f32 else torch.bfloat16)}
    # splitk=1: the fp32-out 128 tile otherwise picks a split count by itself (atomics)
    three_steps(spec, lambda t: C().gemm(t["a"], t["b"], t["c"], a_kc, b_kc, tile=tile, variant=variant, splitk=1),
                _check_plain("c", ref, K, f32), style, before)


@pytest.mark.parametrize("style,before", PADS)
@pytest.mark.parametrize("a_kc,b_kc", LAYOUTS)
@pytest.mark.parametrize("tile,variant,shape", KERNEL_SHAPES)
def test_layouts_fp32_and_bf16_out(tile, variant, shape, a_kc, b_kc, style, before):
    M, N, K = shape
    _plain(tile, variant, M, N, K, a_kc, b_kc, style, before, True)
    _plain(tile, variant, M, N, K, a_kc, b_kc, style, before, False)


@pytest.mark.parametrize("style,before", PADS2)
@pytest.mark.parametrize("K", [1, 7, 65, 333])
@pytest.mark.parametrize("tile,variant", KERNELS)
def test_kstrided_operands_any_k(tile, variant, K, style, before):
    """K % 8 != 0 is allowed when both operands are k-strided (csrc/bindings.cpp:78): the weight
    gradient of a partial batch."""
    M, N, _ = SHAPES[tile][0]
    _plain(tile, variant, M, N, K, False, False, style, before, True)
    _plain(tile, variant, M, N, K, False, False, style, before, False)


@pytest.mark.parametrize("style,before", PADS2)
@pytest.mark.parametrize("tile,variant", KERNELS)
def test_beta_accumulate(tile, variant, style, before):
    M, N, K = SHAPES[tile][0]
    a, b, ref = _ops(M, N, K, False, False, seed=1)
    c0 = torch.randn(M, N, device="cuda")
    spec = {"a": T("in", a), "b": T("in", b), "c": T("out", c0)}
    three_steps(spec, lambda t: C().gemm(t["a"], t["b"], t["c"], False, False, beta=1.0, tile=tile, variant=variant,
                                         splitk=1),
                _check_plain("c", c0.double() + ref, K, True), style, before)


def _act(ref, epi):
    return ref.relu() if epi == "relu" else ref.sigmoid() if epi == "sigmoid" else ref


@pytest.mark.parametrize("style,before", PADS2)
@pytest.mark.parametrize("epi", ["bias", "relu", "sigmoid"])
@pytest.mark.parametrize("tile,variant", KERNELS)
def test_forward_epilogues(tile, variant, epi, style, before):
    M, N, K = SHAPES[tile][0]
    a, b, ref = _ops(M, N, K, True, True, seed=2, scale_b=0.2)
    bias = torch.randn(N, device="cuda")
    ref = _act(ref + bias.double(), epi)
    code = {"bias": C().EPI_BIAS, "relu": C().EPI_BIAS_RELU, "sigmoid": C().EPI_BIAS_SIGMOID}[epi]
    spec = {"a": T("in", a), "b": T("in", b), "c": T("out", shape=(M, N), dtype=torch.bfloat16)}

    def check(t):
        torch.testing.assert_close(t["c"].double(), ref, rtol=2e-2, atol=2e-2)

    three_steps(spec, lambda t: C().gemm(t["a"], t["b"], t["c"], True, True, code, bias=bias, tile=tile,
                                         variant=variant), check, style, before)


def _dgrad_case(M, N, K, act, seed=3):
    """dX[M][N] = (dY[M][K] @ W[K][N]) * act'(y[M][N]); a k-contiguous A, a k-strided B."""
    a, b, gr = _ops(M, N, K, True, False, seed=seed, scale_b=0.2)
    g = torch.Generator(device="cuda").manual_seed(seed + 100)
    y = torch.randn(M, N, device="cuda", generator=g)
    y = (y.relu() if act == "relu" else y.sigmoid()).bfloat16()
    yd = y.double()
    ref = gr * (yd > 0) if act == "relu" else gr * yd * (1 - yd)
    return a, b, y, ref


def _check_dgrad(ref):
    def check(t):
        torch.testing.assert_close(t["c"].double(), ref, rtol=2e-2, atol=5e-2)
        torch.testing.assert_close(t["dbias"].double(), t["c"].double().sum(0), rtol=1e-3, atol=1e-2)
    return check


@pytest.mark.parametrize("style,before", PADS2)
@pytest.mark.parametrize("act", ["relu", "sigmoid"])
@pytest.mark.parametrize("tile,variant", KERNELS)
def test_dgrad_epilogues_strided_aux_and_dbias(tile, variant, act, style, before):
    """dbias is allocated longer than N (the binding asks for numel >= N) and accumulated into."""
    M, N, K = SHAPES[tile][0]
    a, b, y, ref = _dgrad_case(M, N, K, act)
    code = C().EPI_DRELU if act == "relu" else C().EPI_DSIGMOID
    spec = {"a": T("in", a), "b": T("in", b), "aux": T("in", y), "c": T("out", shape=(M, N), dtype=torch.bfloat16),
            "dbias": T("out", torch.zeros(N, device="cuda"), exact=False)}
    three_steps(spec, lambda t: C().gemm(t["a"], t["b"], t["c"], True, False, code, aux=t["aux"], dbias=t["dbias"],
                                         tile=tile, variant=variant), _check_dgrad(ref), style, before)


@pytest.mark.parametrize("style,before", PADS2)
@pytest.mark.parametrize("tile,variant", KERNELS)
@pytest.mark.parametrize("f32", [True, False])
def test_plain_dbias_of_kstrided_operands(tile, variant, f32, style, before):
    """Column sums of a plain product whose operands are both k-strided with ld > rows: the
    four-wave kernel's DMA fetches the pad columns of such operands (they are inside the buffer
    resource's range) into accumulator rows / columns that no store and no sum may use."""
    M, N, K = SHAPES[tile][1]
    a, b, ref = _ops(M, N, K, False, False, seed=4, scale_b=0.2)
    spec = {"a": T("in", a), "b": T("in", b), "c": T("out", shape=(M, N), dtype=torch.float32 if f32 else torch.bfloat16),
            "dbias": T("out", torch.zeros(N, device="cuda"), exact=False)}
    plain = _check_plain("c", ref, K, f32)

    def check(t):
        plain(t)
        torch.testing.assert_close(t["dbias"].double(), t["c"].double().sum(0), rtol=1e-3, atol=1e-2)

    three_steps(spec, lambda t: C().gemm(t["a"], t["b"], t["c"], False, False, dbias=t["dbias"], tile=tile,
                                         variant=variant, splitk=1), check, style, before)


def _bits(h):
    M, N = h.shape
    return ((h.float() > 0).view(M, N // 8, 8).to(torch.int32) << torch.arange(8, device=h.device)).sum(-1)


@pytest.mark.parametrize("style,before", PADS2)
@pytest.mark.parametrize("M,N,K", SHAPES[256])
def test_relu_mask_out_then_mask_in(M, N, K, style, before):
    """The four-wave kernel's ReLU bit masks with ldmask > ceil(N / 8): the forward writes N / 8
    bytes per row and nothing else; the dgrad reads them out of a 0xFF-poisoned buffer."""
    c = C()
    a, b, ref = _ops(M, N, K, True, True, seed=5, scale_b=0.2)
    bias = torch.randn(N, device="cuda")
    ref = (ref + bias.double()).relu()
    spec = {"a": T("in", a), "b": T("in", b), "c": T("out", shape=(M, N), dtype=torch.bfloat16),
            "mask": T("out", shape=(M, N // 8), dtype=torch.uint8)}

    def check(t):
        torch.testing.assert_close(t["c"].double(), ref, rtol=2e-2, atol=2e-2)
        assert torch.equal(t["mask"].to(torch.int32), _bits(t["c"]))

    dense, _ = three_steps(spec, lambda t: c.gemm(t["a"], t["b"], t["c"], True, True, c.EPI_BIAS_RELU, bias=bias,
                                                  mask_out=t["mask"]), check, style, before)
    # dgrad through the mask: dz_prev[M][N] = (dz[M][K2] @ w2[K2][N]) * (h > 0)
    K2 = 72
    dz, w2, gr = _ops(M, N, K2, True, False, seed=6, scale_b=0.2)
    ref2 = gr * (dense["c"].double() > 0)
    spec2 = {"a": T("in", dz), "b": T("in", w2), "mask": T("mask_in", dense["mask"]),
             "c": T("out", shape=(M, N), dtype=torch.bfloat16),
             "dbias": T("out", torch.zeros(N, device="cuda"), exact=False)}
    three_steps(spec2, lambda t: c.gemm(t["a"], t["b"], t["c"], True, False, c.EPI_DRELU, dbias=t["dbias"],
                                        mask_in=t["mask"]), _check_dgrad(ref2), style, before)


@pytest.mark.parametrize("style,before", PADS2)
@pytest.mark.parametrize("M,N,K", SHAPES[256])
def test_head_partials_strided_head_w(M, N, K, style, before):
    """EPI_BIAS_RELU_HEAD with head_w.stride(0) > N.  Zero by contract: head_w rows [ncls, 16)
    (csrc/bindings.cpp:130-132, "classes zero-padded to 16"); NaN: its columns behind N.
    head_part is dense by contract (csrc/bindings.cpp:133-135)."""
    c = C()
    a, b, ref = _ops(M, N, K, True, True, seed=7, scale_b=K ** -0.5)
    g = torch.Generator(device="cuda").manual_seed(8)
    bias = torch.randn(N, device="cuda", generator=g) * 0.1
    hw = torch.zeros(16, N, device="cuda", dtype=torch.bfloat16)
    hw[:10] = (torch.randn(10, N, device="cuda", generator=g) / N ** 0.5).bfloat16()
    ref = (ref + bias.double()).relu()
    spec = {"a": T("in", a), "b": T("in", b), "hw": T("in", hw), "c": T("out", shape=(M, N), dtype=torch.bfloat16),
            "part": T("dense", shape=((N + 255) // 256, M, 16), dtype=torch.float32)}

    def check(t):
        torch.testing.assert_close(t["c"].double(), ref, rtol=2e-2, atol=2e-2)
        for s in range(t["part"].shape[0]):   # the product of the STORED bf16 activation, per 256-column slab
            sl = slice(256 * s, min(N, 256 * (s + 1)))
            ref_s = t["c"][:, sl].double() @ hw[:, sl].double().t()
            torch.testing.assert_close(t["part"][s].double(), ref_s, rtol=1e-3,
                                       atol=1e-3 * max(1.0, ref_s.abs().max().item()))

    three_steps(spec, lambda t: c.gemm(t["a"], t["b"], t["c"], True, True, c.EPI_BIAS_RELU, bias=bias,
                                       head_w=t["hw"], head_part=t["part"]), check, style, before)


@pytest.mark.parametrize("style,before", PADS2)
@pytest.mark.parametrize("case", ["wgrad", "wgrad_beta", "fwd_relu", "dgrad_drelu"])
@pytest.mark.parametrize("tile", [128, 256])
def test_splitk_inlaunch_combine_uneven(tile, case, style, before):
    """K = 200 over 3 splits (4 K-tiles: 2 + 2 + 0 of them, the last one ragged): the in-launch
    combine is deterministic, so strided == dense bit for bit; the counters come back zero."""
    c = C()
    K, sk = 200, 3
    M, N, _ = SHAPES[tile][0]
    kw = dict(tile=tile, variant=32 if tile == 256 else 0, splitk=sk)
    ne, nc = c.gemm_q_ws(M, N, sk) if tile == 256 else c.gemm_splitk_ws(M, N, sk)
    ws = torch.empty(ne, device="cuda")
    cnt = torch.zeros(nc, device="cuda", dtype=torch.int32)
    if case in ("wgrad", "wgrad_beta"):
        a, b, ref = _ops(M, N, K, False, False, seed=9)
        c0 = torch.randn(M, N, device="cuda") if case == "wgrad_beta" else None
        spec = {"a": T("in", a), "b": T("in", b),
                "c": T("out", c0) if c0 is not None else T("out", shape=(M, N), dtype=torch.float32)}
        check = _check_plain("c", ref + (c0.double() if c0 is not None else 0), K, True)

        def call(t):
            c.gemm(t["a"], t["b"], t["c"], False, False, beta=1.0 if c0 is not None else 0.0, ws=ws, cnt=cnt, **kw)
    elif case == "fwd_relu":
        a, b, ref = _ops(M, N, K, True, True, seed=10, scale_b=0.2)
        bias = torch.randn(N, device="cuda")
        ref = (ref + bias.double()).relu()
        spec = {"a": T("in", a), "b": T("in", b), "c": T("out", shape=(M, N), dtype=torch.bfloat16)}

        def check(t):
            torch.testing.assert_close(t["c"].double(), ref, rtol=2e-2, atol=2e-2)

        def call(t):
            c.gemm(t["a"], t["b"], t["c"], True, True, c.EPI_BIAS_RELU, bias=bias, ws=ws, cnt=cnt, **kw)
    else:
        a, b, y, ref = _dgrad_case(M, N, K, "relu", seed=11)
        spec = {"a": T("in", a), "b": T("in", b), "aux": T("in", y), "c": T("out", shape=(M, N), dtype=torch.bfloat16),
                "dbias": T("out", torch.zeros(N, device="cuda"), exact=False)}
        check = _check_dgrad(ref)

        def call(t):
            c.gemm(t["a"], t["b"], t["c"], True, False, c.EPI_DRELU, aux=t["aux"], dbias=t["dbias"], ws=ws, cnt=cnt,
                   **kw)
    three_steps(spec, call, check, style, before)
    assert int(cnt.abs().sum().item()) == 0


@pytest.mark.parametrize("style,before", PADS2)
@pytest.mark.parametrize("a_kc,b_kc", [(False, False), (True, False)])
def test_slab_output_strided_operands(a_kc, b_kc, style, before):
    """Split-K partial products into dense [splitk][M][N] slabs (dense by contract,
    csrc/bindings.cpp:63-65): only A and B are strided."""
    c = C()
    M, N, K, sk = 264, 264, 200, 3
    a, b, ref = _ops(M, N, K, a_kc, b_kc, seed=12)
    spec = {"a": T("in", a), "b": T("in", b), "slabs": T("dense", shape=(sk, M, N), dtype=torch.float32)}

    def check(t):
        err = (t["slabs"].double().sum(0) - ref).abs().max().item()
        assert err <= 1e-3 * K ** 0.5 + 1e-3, err

    three_steps(spec, lambda t: c.gemm(t["a"], t["b"], t["slabs"], a_kc, b_kc, tile=256, splitk=sk), check, style, before)


@pytest.mark.parametrize("style,before", PADS2)
@pytest.mark.parametrize("N", [8, 40, 64])
@pytest.mark.parametrize("epi", ["none", "bias", "relu", "sigmoid"])
def test_skinny_n(N, epi, style, before):
    M, K = 70, 264
    a, b, ref = _ops(M, N, K, True, True, seed=13, scale_b=0.1)
    bias = torch.randn(N, device="cuda")
    code = {"none": C().EPI_NONE, "bias": C().EPI_BIAS, "relu": C().EPI_BIAS_RELU, "sigmoid": C().EPI_BIAS_SIGMOID}[epi]
    if epi != "none":
        ref = _act(ref + bias.double(), epi)
    spec = {"a": T("in", a), "b": T("in", b), "c": T("out", shape=(M, N), dtype=torch.bfloat16)}
    if epi == "none":
        check = _check_plain("c", ref, K, False)
    else:
        def check(t):
            torch.testing.assert_close(t["c"].double(), ref, rtol=2e-2, atol=2e-2)
    three_steps(spec, lambda t: C().gemm(t["a"], t["b"], t["c"], True, True, code,
                                         bias=bias if epi != "none" else None, tile=16), check, style, before)


@pytest.mark.parametrize("style,before", PADS2)
@pytest.mark.parametrize("kind", ["sgd", "adamw"])
@pytest.mark.parametrize("tile,M,N,K,splitk", [(128, 136, 136, 72, 0), (128, 136, 136, 200, 3), (256, 264, 264, 72, 0),
                                                (256, 264, 264, 1032, 0)])
def test_gemm_opt_strided_state(tile, M, N, K, splitk, kind, style, before):
    """gemm_opt with master / m / v / shadow as equally strided views (the engine's views into
    its flat buffers): gemm.hip's 128 tile (plain and in-launch split-K), its k256 kernel, and
    the four-wave kernel's row-staged update (tile 256, K >= 1024).  The dense run is held to
    the fp64 gradient and to the flat optimizer kernel applied to the separately computed
    gradient, with test_gemm_q_gpu.py's bounds; the strided run must equal the dense one."""
    c = C()
    dz, h, gref = _ops(M, N, K, False, False, seed=14, scale_b=0.1)
    g = torch.Generator(device="cuda").manual_seed(15)
    master0 = torch.randn(M, N, device="cuda", generator=g) * 0.05
    m0 = torch.randn(M, N, device="cuda", generator=g) * 1e-3
    v0 = torch.rand(M, N, device="cuda", generator=g) * 1e-5
    hp = torch.tensor([1e-2 if kind == "sgd" else 1e-3, 3.0], device="cuda")
    wd = 1e-2
    kw = {}
    if splitk > 1:
        ne, nc = c.gemm_splitk_ws(M, N, splitk)
        kw = dict(ws=torch.empty(ne, device="cuda"), cnt=torch.zeros(nc, device="cuda", dtype=torch.int32))
    grad = torch.empty(M, N, device="cuda")
    # (the tiling and the split gemm_opt takes: the same fp32 accumulation order)
    c.gemm(dz, h, grad, False, False, tile=tile, variant=32 if K >= 1024 else 1 if tile == 256 else 0,
           splitk=max(splitk, 1), **kw)
    assert (grad.double() - gref).abs().max().item() <= 1e-3 * K ** 0.5 + 1e-3
    mr, m1, v1 = master0.clone(), m0.clone(), v0.clone()
    sr = torch.empty(M, N, dtype=torch.bfloat16, device="cuda")
    if kind == "sgd":
        c.sgd_step(mr.view(-1), grad.view(-1), m1.view(-1), sr.view(-1), hp, 0.5, 0.9, 0.0, wd, False, False)
    else:
        c.adam_step(mr.view(-1), grad.view(-1), m1.view(-1), v1.view(-1), sr.view(-1), hp, 0.5, 0.9, 0.999, 1e-8, wd,
                    True)
    spec = {"a": T("in", dz), "b": T("in", h), "master": T("out", master0), "m": T("out", m0),
            "shadow": T("out", shape=(M, N), dtype=torch.bfloat16)}
    if kind != "sgd":
        spec["v"] = T("out", v0)

    def call(t):
        if kind == "sgd":
            c.gemm_opt(t["a"], t["b"], t["master"], False, False, "sgd", m=t["m"], shadow=t["shadow"], hp=hp,
                       grad_scale=0.5, momentum=0.9, weight_decay=wd, tile=tile, splitk=splitk, **kw)
        else:
            c.gemm_opt(t["a"], t["b"], t["master"], False, False, kind, m=t["m"], v=t["v"], shadow=t["shadow"], hp=hp,
                       grad_scale=0.5, weight_decay=wd, tile=tile, splitk=splitk, **kw)

    def check(t):
        torch.testing.assert_close(t["master"], mr, rtol=1e-5, atol=1e-7)
        torch.testing.assert_close(t["m"], m1, rtol=1e-4, atol=1e-9)
        if kind != "sgd":
            torch.testing.assert_close(t["v"], v1, rtol=1e-4, atol=1e-9)
        assert (t["shadow"].float() - sr.float()).abs().max().item() <= 2 ** -7 * mr.abs().max().item()

    three_steps(spec, call, check, style, before)
