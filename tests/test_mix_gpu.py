"""The batch-mix pass (mix.hip) against its definition, and the loader / trainer on top of it.

Mixup: out = lam x + (1 - lam) x[perm] against float64.  An fp32 output carries the rounding of
lam to fp32, of the two products and of the sum (fewer with contraction): at most 4 * 2^-24 =
2^-22 of |lam a| + |(1 - lam) b|.  A bf16 output adds one bf16 rounding, 2^-8 |ref| with slack
for a flipped tie.  CutMix copies: bit-exact.
"""
import numpy as np
import pytest
import torch

import ldnn
from ldnn.data.datasets import ArrayDataset
from ldnn.data.loader import DeviceLoader
from ldnn.data.mix import MODE_CUTMIX, MODE_MIXUP, BatchMix, MixPlan, mix_native, mix_reference

pytestmark = pytest.mark.gpu

SHAPES = [(5, 3, 32, 32),
          (3, 1, 28, 28),      # rows are no multiple of 8 elements
          (2, 3, 7, 5),        # 105 elements per image: the scalar path, unaligned image bases
          (4, 3, 224, 224)]
DTYPES = [torch.float32, torch.bfloat16]


def _batch(shape, dtype, seed=41, classes=10):
    g = torch.Generator(device="cuda").manual_seed(seed)
    n = int(np.prod(shape))
    # one element in: with 105-element images no bf16 image base is 16-byte aligned
    flat = torch.randn(n + 1, device="cuda", generator=g).to(dtype)
    x = flat[1:].view(shape) if shape[2:] == (7, 5) else flat[:n].view(shape)
    y = torch.randint(0, classes, (shape[0],), device="cuda", generator=g)
    return x, y


def _perm(kind, B):
    if kind == "identity":
        return np.arange(B, dtype=np.int64)
    if kind == "reversal":
        return np.arange(B, dtype=np.int64)[::-1].copy()
    p = np.random.default_rng(42).permutation(B).astype(np.int64)
    if B > 2:   # a random permutation with a fixed point
        j = int(np.where(p == 0)[0][0])
        p[j], p[0] = p[0], 0
    return p


def _run(x, y, plan, classes=10):
    perm = torch.as_tensor(plan.perm, device="cuda")
    out, q = mix_native(x, y, perm, plan, classes)
    torch.cuda.synchronize()
    return out, q


@pytest.mark.parametrize("perm", ["identity", "reversal", "random"])
@pytest.mark.parametrize("lam", [0.0, 0.37, 1.0])
@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_mixup_matches_float64(shape, dtype, lam, perm):
    x, y = _batch(shape, dtype)
    p = _perm(perm, shape[0])
    out, _ = _run(x, y, MixPlan(MODE_MIXUP, lam, p, (0, 0, 0, 0)))
    assert out.dtype == x.dtype and out.shape == x.shape
    a, b = x.double(), x[torch.as_tensor(p, device="cuda")].double()
    ref = lam * a + (1.0 - lam) * b
    bound = 2.0 ** -22 * ((lam * a).abs() + ((1.0 - lam) * b).abs())
    if dtype == torch.bfloat16:
        bound = bound + 2.0 ** -8 * ref.abs()
    err = (out.double() - ref).abs()
    print(f"max err {err.max().item():.3e}  max err / bound {(err / bound.clamp_min(1e-300)).max().item():.3f}")
    assert bool((err <= bound).all())


def _boxes(H, W):
    bs = [(0, 0, 0, 0),                                   # empty
          (0, H, 0, W),                                   # the whole image
          (H // 2, H // 2 + 1, W // 2, W // 2 + 1),       # one pixel
          (0, max(1, H // 3), 0, max(1, W // 3)),         # touching top and left
          (H - max(1, H // 3), H, W - max(1, W // 3), W),  # touching bottom and right
          (1 % H, H, min(3, W - 1), min(13, W))]          # column edges not divisible by 8
    return bs


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_cutmix_is_bit_exact(shape, dtype):
    x, y = _batch(shape, dtype, seed=43)
    B, _, H, W = shape
    for kind in ("reversal", "random"):
        p = _perm(kind, B)
        xp = x[torch.as_tensor(p, device="cuda")]
        for (y0, y1, x0, x1) in _boxes(H, W):
            lam = 1.0 - (y1 - y0) * (x1 - x0) / float(H * W)
            out, _ = _run(x, y, MixPlan(MODE_CUTMIX, lam, p, (y0, y1, x0, x1)))
            mask = torch.zeros(1, 1, H, W, dtype=torch.bool, device="cuda")
            mask[..., y0:y1, x0:x1] = True
            ref = torch.where(mask, xp, x)
            bits = torch.int32 if dtype == torch.float32 else torch.int16
            assert torch.equal(out.contiguous().view(bits), ref.contiguous().view(bits)), (kind, y0, y1, x0, x1)
            # ... and the CPU twin is the same function
            cpu, _ = mix_reference(x.cpu(), y.cpu(), torch.as_tensor(p), MixPlan(MODE_CUTMIX, lam, p, (y0, y1, x0, x1)), 10)
            assert torch.equal(cpu, ref.cpu())


@pytest.mark.parametrize("classes", [10, 1000])
@pytest.mark.parametrize("lam", [0.0, 0.37, 1.0])
def test_soft_targets(classes, lam):
    B = 37
    x, y = _batch((B, 1, 4, 4), torch.float32, seed=44, classes=classes)
    p = _perm("random", B)
    y[int(np.where(p == 3)[0][0])] = y[3]          # besides the fixed point: two samples of one class paired
    out, q = _run(x, y, MixPlan(MODE_MIXUP, lam, p, (0, 0, 0, 0)), classes)
    assert q.shape == (B, classes) and q.dtype == torch.float32 and q.stride() == ((classes + 3) // 4 * 4, 1)
    ref = torch.zeros(B, classes, device="cuda")
    rows = torch.arange(B, device="cuda")
    yp = y[torch.as_tensor(p, device="cuda")]
    ref[rows, y] += torch.tensor(lam, device="cuda")
    ref[rows, yp] += 1.0 - torch.tensor(lam, device="cuda")
    assert (q - ref).abs().max().item() <= 1e-6
    assert (q.sum(1) - 1.0).abs().max().item() <= 1e-6
    full = q.as_strided((B, q.stride(0)), (q.stride(0), 1))
    if full.shape[1] > classes:
        assert full[:, classes:].abs().max().item() == 0.0   # pad columns
    same = (y == yp)
    assert bool(same.any())
    assert bool((q[same].max(1).values == 1.0).all()) and bool(((q[same] != 0).sum(1) == 1).all())
    cpu_q = mix_reference(x.cpu(), y.cpu(), torch.as_tensor(p), MixPlan(MODE_MIXUP, lam, p, (0, 0, 0, 0)), classes)[1]
    assert (q.cpu() - cpu_q).abs().max().item() <= 1e-6


def test_binding_refusals():
    x, y = _batch((4, 3, 8, 8), torch.float32)
    p = _perm("reversal", 4)
    with pytest.raises(RuntimeError, match="box"):
        _run(x, y, MixPlan(MODE_CUTMIX, 0.5, p, (0, 9, 0, 8)))
    with pytest.raises(RuntimeError, match="lam"):
        _run(x, y, MixPlan(MODE_MIXUP, 1.5, p, (0, 0, 0, 0)))
    with pytest.raises(RuntimeError, match="perm"):
        _run(x, y, MixPlan(MODE_MIXUP, 0.5, p[:3], (0, 0, 0, 0)))


def _dataset(n=64, classes=10, seed=45):
    g = torch.Generator().manual_seed(seed)
    imgs = torch.randint(0, 256, (n, 3, 32, 32), dtype=torch.uint8, generator=g)
    labels = torch.randint(0, classes, (n,), generator=g)
    # mean 0 / std 1: the un-mixed batch is raw / 255 on both devices, bit for bit
    return ArrayDataset(imgs, labels, classes, (0.0, 0.0, 0.0), (1.0, 1.0, 1.0), "t")


def test_loader_parity_and_determinism():
    from ldnn.data import autoaugment as AA

    ds = _dataset()
    mix = BatchMix(0.2, 1.0, num_classes=10)
    mk = lambda dev, m=mix: DeviceLoader(ds, None, 16, dev, seed=7, dtype=torch.float32, mix=m)   # noqa: E731
    gpu, gpu2, cpu, plain = mk("cuda"), mk("cuda"), mk("cpu"), mk("cpu", None)
    epochs = []
    for epoch in range(2):
        got = []
        for k, ((xg, qg), (xg2, qg2), (xc, qc), (x0, y0)) in enumerate(zip(gpu, gpu2, cpu, plain)):
            plan = mix.plan(AA.batch_seed(7, epoch, k), 16, 32, 32)
            assert qg.shape == (16, 10) and qg.dtype == torch.float32 and xg.dtype == torch.float32
            assert torch.equal(xg, xg2) and torch.equal(qg, qg2)           # one seed, one stream of batches
            assert (qg.cpu() - qc).abs().max().item() <= 1e-6
            a, b = x0.double(), x0[torch.as_tensor(plan.perm)].double()
            if plan.cutmix:
                y0_, y1_, x0_, x1_ = plan.box
                ref = a.clone()
                ref[:, :, y0_:y1_, x0_:x1_] = b[:, :, y0_:y1_, x0_:x1_]
                bound = torch.zeros_like(ref)
            else:
                ref = plan.lam * a + (1.0 - plan.lam) * b
                bound = 2.0 ** -22 * ((plan.lam * a).abs() + ((1.0 - plan.lam) * b).abs())
            assert bool(((xg.cpu().double() - ref).abs() <= bound).all()), (epoch, k, plan.mode)
            assert bool(((xc.double() - ref).abs() <= bound).all()), (epoch, k, plan.mode)
            got.append((xg, qg))
        assert len(got) == 4
        epochs.append(got)
    assert any(not torch.equal(a[0], b[0]) for a, b in zip(*epochs))     # epoch 1 draws anew
    assert 0.0 <= gpu.pop_mix_lam_mean() <= 1.0


def test_train_local_epoch_with_graphs():
    from ldnn.models import CrossEntropyLoss, build_model, xavier_init
    from ldnn.optim import SGD
    from ldnn.train.trainer import train_local_epoch

    torch.manual_seed(46)
    m = build_model("enhanced_cnn_small")
    xavier_init(m)
    ldnn.prepare(m, "cuda")
    opt = SGD(m.parameters(), lr=0.01, momentum=0.9)
    loader = DeviceLoader(_dataset(), None, 16, "cuda", seed=8, dtype=torch.bfloat16,
                          mix=BatchMix(0.2, 1.0, num_classes=10))
    loss, acc, bl = train_local_epoch(m, loader, CrossEntropyLoss(label_smoothing=0.1), opt, "cuda", graphs=True)
    assert len(bl) == 4 and all(np.isfinite(v) for v in bl) and np.isfinite(loss)
    assert train_local_epoch.last_samples == 64            # samples, not samples x classes
    assert 0.0 <= acc <= 100.0
    assert getattr(m, "_ldnn_graphed", None) is not None   # batches 2-4 replayed the captured step
    assert 0.0 <= loader.pop_mix_lam_mean() <= 1.0
