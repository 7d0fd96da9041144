#!/usr/bin/env python
"""Rates of the grouped 3x3 kernels (gconv.hip) at the separable EnhancedCNN's eight ``dw`` shapes, at group
widths 8, 16 and 32, beside two yardsticks alternated in the same process: the BatchNorm apply pass
(bn_fwd with stats_ready: one bf16 read, one bf16 write of the input's size: bytes per second) and the dense
3x3 C -> C forward / dgrad / wgrad of the same shape (the implicit-GEMM kernels).  Bytes are one read of each
input and one write of each output (fwd: x + y; dgrad: dy + dx; wgrad: x + dy); FLOP are 2 * 9 * gw per output
element.  HIP events around single launches, medians of --reps after a warm-up: the small stages sit on the
launch floor, where a time says nothing about the kernel.  Then the graphed step time of ``enhanced_cnn
--separable`` at group width 1 beside 16, alternated in the same run.  One JSON line each.

    python scripts/bench_gconv.py [--reps 30] [--steps 40] [--batch 64 256] [--step_batch 64]
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import ldnn  # noqa: E402
from ldnn.ops import _ext  # noqa: E402

# (C, H = W, stride) of conv1.dw / conv2.dw through layer1 .. layer4
SHAPES = [(64, 32, 2), (128, 16, 1), (128, 16, 2), (256, 8, 1), (256, 8, 2), (512, 4, 1), (512, 4, 2), (1024, 2, 1)]


def timed(fns, reps, warm=5):
    ts = {k: [] for k in fns}
    for i in range(warm + reps):
        for k, fn in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            if i >= warm:
                ts[k].append(a.elapsed_time(b) * 1e3)
    return {k: statistics.median(v) for k, v in ts.items()}


def kernels(N, reps):
    C_ = _ext.C()
    dev = "cuda"
    for C, H, st in SHAPES:
        P = (H - 1) // st + 1
        x = torch.randn(N, H, H, C, device=dev).bfloat16()
        y, dx = torch.empty(N, P, P, C, dtype=torch.bfloat16, device=dev), torch.empty_like(x)
        dy = torch.randn(N, P, P, C, device=dev).bfloat16()
        xb, yb = x.view(-1, C), torch.empty_like(x).view(-1, C)
        gamma, beta = torch.ones(C, device=dev), torch.zeros(C, device=dev)
        mean, inv = torch.empty(C, device=dev), torch.empty(C, device=dev)
        bws = torch.zeros(C_.bn_workspace_floats(C), device=dev)

        def bn(ready=True):
            C_.bn_fwd(xb, yb, None, gamma, beta, None, None, mean, inv, bws, 1e-5, 0.0, True, False, None,
                      stats_ready=ready)

        bn(False)   # (leaves the coefficients the apply-only calls read)
        wd = torch.randn(C, 3, 3, C, device=dev).bfloat16()
        dwd = torch.zeros(C, 3, 3, C, device=dev)
        fns = {"bn_apply": bn, "dense_fwd": lambda: C_.conv_fwd(x, wd, y, st, 1),
               "dense_dgrad": lambda: C_.conv_dgrad(dy, wd, dx, st, 1),
               "dense_wgrad": lambda: C_.conv_wgrad(dy, x, dwd, st, 1)}
        keep = []
        for gw in (8, 16, 32):
            if C // gw < 2:
                continue
            w = torch.randn(C, 3, 3, gw, device=dev).bfloat16()
            dw = torch.zeros(C, 3, 3, gw, device=dev)
            ws = torch.empty(C_.gconv_workspace_floats(N, H, H, C, gw, st), device=dev)
            keep.append((w, dw, ws))
            fns[f"gw{gw}_fwd"] = lambda w=w: C_.gconv_fwd(x, w, y, st)
            fns[f"gw{gw}_dgrad"] = lambda w=w: C_.gconv_dgrad(dy, w, dx, st)
            fns[f"gw{gw}_wgrad"] = lambda dw=dw, ws=ws: C_.gconv_wgrad(x, dy, ws, dw, False, st)
        t = timed(fns, reps)
        io = 2 * (x.numel() + y.numel())
        rec = {"shape_nhwc": [N, H, H, C], "stride": st, "reps": reps, "conv_bytes": io, "bn_apply_bytes": 4 * x.numel()}
        rec.update({k + "_us": round(v, 2) for k, v in t.items()})
        rec["bn_apply_TBps"] = round(4 * x.numel() / t["bn_apply"] / 1e6, 3)
        for k, v in t.items():
            if k.startswith("gw"):
                gw, ps = int(k[2:k.index("_")]), k[k.index("_") + 1:]
                rec[k + "_TBps"] = round(io / v / 1e6, 3)
                rec[k + "_TFLOPs"] = round(2 * 9 * gw * y.numel() / v / 1e6, 2)
                rec[k + "_over_dense"] = round(v / t["dense_" + ps], 3)
        print(json.dumps(rec), flush=True)


def steps(N, n_steps):
    from ldnn.models import CrossEntropyLoss, build_model, xavier_init
    from ldnn.optim import SGD
    from ldnn.train.graphed import GraphedStep

    torch.manual_seed(0)
    x = torch.randn(N, 3, 32, 32, device="cuda").bfloat16()
    y = torch.randint(0, 10, (N,), device="cuda")
    runs = {}
    for gw in (1, 16):
        m = build_model("enhanced_cnn", separable=True, group_width=gw)
        xavier_init(m)
        ldnn.prepare(m, "cuda")
        opt = SGD(m.parameters(), lr=0.01, momentum=0.9)
        gs = GraphedStep(m, CrossEntropyLoss(), opt, x, y)
        runs[f"gw{gw}"] = (lambda gs=gs: gs(x, y), sum(p.numel() for p in m.parameters()))
    t = timed({k: v[0] for k, v in runs.items()}, n_steps)
    print(json.dumps({"model": "enhanced_cnn --separable", "batch": N, "steps": n_steps,
                      **{k + "_params": v[1] for k, v in runs.items()},
                      **{k + "_graphed_step_us": round(v, 1) for k, v in t.items()}}), flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--batch", type=int, nargs="+", default=[64, 256])
    ap.add_argument("--step_batch", type=int, default=64)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_gconv.py measures on the GPU"
    for n in a.batch:
        kernels(n, a.reps)
    steps(a.step_batch, a.steps)
