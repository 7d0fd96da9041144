"""CNN training throughput (samples/s, 1 GPU): ldnn native path (implicit-GEMM conv,
fused BN+add+ReLU, fused optimizer) vs stock PyTorch-ROCm (MIOpen convs, autocast bf16,
channels_last, torch.optim), same model / batch / synthetic data.

    python scripts/bench_cnn.py --model enhanced_cnn --batch 256
"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import ldnn  # noqa: E402
from ldnn.models import CrossEntropyLoss, build_model, dataset_for, xavier_init  # noqa: E402
from ldnn.data.datasets import SHAPES  # noqa: E402
from ldnn.optim import SGD, Adam, Lamb, Lion  # noqa: E402


def run(step, steps, warmup):
    for _ in range(warmup):
        step()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        step()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="enhanced_cnn")
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--no-stock", action="store_true")
    ap.add_argument("--conv-impl", type=int, default=0, help="0 = LDS-DMA fast path, 1 = generic conv kernel only")
    ap.add_argument("--graph", action="store_true", help="replay the ldnn step from one hipGraph (train.graphed)")
    ap.add_argument("--optimizer", choices=["sgd", "adam", "lamb", "lion"], default="sgd",
                    help="sgd = momentum 0.9; adam = the reference config (BAR/main.py:53, lr 1e-3); lamb = Lamb "
                         "(lr 1e-3, weight decay 1e-2); lion = Lion (lr 1e-4, weight decay 0.1); the stock baseline "
                         "of lamb and lion is torch's Adam")
    ap.add_argument("--clip", type=float, default=0.0,
                    help="max_grad_norm of the ldnn optimizer (global-norm clipping; 0 = off, 1e30 = the clipped "
                         "kernels with unchanged math)")
    ap.add_argument("--lars", type=float, default=0.0,
                    help="lars_trust of the ldnn SGD (LARS trust ratios; 0 = off)")
    ap.add_argument("--label_smoothing", type=float, default=0.0,
                    help="label smoothing of the ldnn criterion (the fused loss kernel's SMOOTH instance; 0 = off); "
                         "the stock baseline gets the same value")
    ap.add_argument("--ema_decay", type=float, default=0.0,
                    help="ema_decay of the ldnn optimizer (the weight-EMA pass behind every update; 0 = off); the "
                         "stock baseline keeps no average")
    ap.add_argument("--lr_schedule", choices=["none", "constant", "linear", "poly", "cosine"], default="none",
                    help="lr_schedule of the ldnn optimizer (the one-thread lr_sched launch in front of the update; "
                         "10 warm-up steps, horizon 10000); the stock baseline keeps a constant rate")
    ap.add_argument("--dropout", type=float, default=0.0,
                    help="dropout rate of the ldnn model (build_model's keyword: the dropout.hip pass each way at the "
                         "model's dropout sites; 0 = off, no module is built); the stock baseline has none")
    ap.add_argument("--norm", choices=["batch", "group", "layer"], default="batch",
                    help="normalisation layer of the ldnn model and of the stock baseline (build_model's keyword; "
                         "group: GroupNorm, 32 groups, the group_norm.hip passes; layer: with --model mlp2 / mlp3 / "
                         "mlp3_small, a LayerNorm after every hidden Linear, the layer_norm.hip passes)")
    ap.add_argument("--targets", choices=["hard", "soft", "mix"], default="hard",
                    help="ldnn step: hard = class indices; soft = a pre-mixed batch's class-probability targets "
                         "[B, C] (the loss kernel's soft-target instance); mix = soft plus the batch-mix pass "
                         "(mix.hip, alternating Mixup / CutMix plans) in front of every step.  The stock baseline "
                         "keeps hard labels")
    a = ap.parse_args()
    from ldnn.ops import _ext as _e

    _e.C().set_conv_impl(a.conv_impl)
    shape = SHAPES[dataset_for(a.model)]
    nc = 1000 if a.model == "resnet18" else 10
    x = torch.randn(a.batch, *shape, device="cuda")
    y = torch.randint(0, nc, (a.batch,), device="cuda")

    torch.manual_seed(0)
    m = build_model(a.model, dropout=a.dropout, norm=a.norm)
    xavier_init(m)
    ldnn.prepare(m, "cuda")
    ldnn.reseed_dropout(m, 0)
    kw = dict(max_grad_norm=a.clip) if a.clip > 0 else {}
    if a.lars > 0:
        assert a.optimizer == "sgd", "--lars goes with --optimizer sgd"
        kw["lars_trust"] = a.lars
    if a.ema_decay > 0:
        kw["ema_decay"] = a.ema_decay
    if a.lr_schedule != "none":
        kw["lr_schedule"] = dict(kind=a.lr_schedule, total_steps=10000, warmup_steps=10)
    opt = (Adam(m.parameters(), lr=1e-3, **kw) if a.optimizer == "adam"
           else Lamb(m.parameters(), lr=1e-3, weight_decay=1e-2, **kw) if a.optimizer == "lamb"
           else Lion(m.parameters(), lr=1e-4, weight_decay=0.1, **kw) if a.optimizer == "lion"
           else SGD(m.parameters(), lr=0.01, momentum=0.9, **kw))
    crit = CrossEntropyLoss(label_smoothing=a.label_smoothing)
    xb = x.bfloat16()

    def step_ldnn():
        opt.zero_grad()
        crit(m(xb), y).backward()
        opt.step()

    feed = lambda: (xb, y)   # noqa: E731
    if a.targets != "hard":
        from ldnn.data.mix import BatchMix

        mix = BatchMix(0.2, 1.0, num_classes=nc)
        plans = [mix.plan(s, a.batch, shape[1], shape[2]) for s in range(16)]
        perms = [torch.as_tensor(p.perm, device="cuda") for p in plans]
        pre = mix.apply(xb, y, plans[0])
        k = [0]

        def feed():  # noqa: F811
            if a.targets == "soft":
                return pre
            k[0] = (k[0] + 1) % len(plans)
            from ldnn.data.mix import mix_native
            return mix_native(xb, y, perms[k[0]], plans[k[0]], nc)

        def step_ldnn():  # noqa: F811
            xm, q = feed()
            opt.zero_grad()
            crit(m(xm), q).backward()
            opt.step()

    if a.graph:
        from ldnn.train.graphed import GraphedStep

        gs = GraphedStep(m, crit, opt, *feed())

        def step_ldnn():  # noqa: F811
            gs(*feed())

    t = run(step_ldnn, a.steps, a.warmup)
    rec = {"model": a.model, "batch": a.batch, "optimizer": a.optimizer, "conv_impl": a.conv_impl, "graph": a.graph, "clip": a.clip, "lars": a.lars, "label_smoothing": a.label_smoothing, "ema_decay": a.ema_decay, "lr_schedule": a.lr_schedule, "dropout": a.dropout, "norm": a.norm, "targets": a.targets, "ldnn_ms": round(t * 1e3, 3), "ldnn_samples_per_s": round(a.batch / t, 1)}
    if a.lars > 0:   # (the ratios the timed steps ended on: near 1 keeps the math comparable with --lars 0)
        ls = opt.lars_stats()
        r = ls["ratio"].cpu()[torch.tensor(ls["adapted"])]
        rec["lars_ratio_median"] = round(float(r.median()), 4)
    if not a.no_stock:
        import torch.nn as nn

        torch.manual_seed(0)
        ref = build_model(a.model, norm=a.norm)
        # swap ldnn layers for stock torch behaviour: run the CPU/fp32 code path under autocast
        ref = ref.cuda().to(memory_format=torch.channels_last)
        os.environ["LDNN_DISABLE_NATIVE"] = "1"
        from ldnn.ops import _ext

        _ext._DISABLED = True
        ropt = (torch.optim.Adam(ref.parameters(), lr=1e-3) if a.optimizer in ("adam", "lamb", "lion") else
                torch.optim.SGD(ref.parameters(), lr=0.01, momentum=0.9))
        ce = nn.CrossEntropyLoss(label_smoothing=a.label_smoothing)
        xc = x.contiguous(memory_format=torch.channels_last)

        def step_stock():
            ropt.zero_grad(set_to_none=True)
            with torch.autocast("cuda", dtype=torch.bfloat16):
                loss = ce(ref(xc).float(), y)
            loss.backward()
            ropt.step()

        ts = run(step_stock, a.steps, a.warmup)
        _ext._DISABLED = False
        rec.update(stock_ms=round(ts * 1e3, 3), stock_samples_per_s=round(a.batch / ts, 1),
                   speedup=round(ts / t, 3))
    print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
