#!/usr/bin/env python
"""Rates of the depthwise 3x3 kernels (dwconv.hip) at the separable EnhancedCNN's eight depthwise
shapes at batch 64, beside a project kernel that moves the same kind of bytes at the same shape: the
BatchNorm apply pass (bn_fwd with stats_ready: one bf16 read, one bf16 write of the input's size).
Bytes are one read of each input and one write of each output (fwd: x + y; dgrad: dy + dx; wgrad:
x + dy).  One process, alternated, HIP events, medians of --reps.  Then the graphed step time of
enhanced_cnn with --separable beside the dense model's, alternated in the same run.  One JSON line each.

    python scripts/bench_dwconv.py [--reps 50] [--steps 40] [--batch 64]
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
        w = torch.zeros(C, 3, 3, 8, dtype=torch.bfloat16, device=dev)
        w[..., 0] = torch.randn(C, 3, 3, device=dev)
        dw = torch.zeros(C, 3, 3, 8, device=dev)
        ws = torch.empty(C_.dwconv_workspace_floats(N, H, H, C, st), device=dev)
        xb, yb = x.view(-1, C), torch.empty_like(x).view(-1, C)
        gamma, beta = torch.ones(C, device=dev), torch.zeros(C, device=dev)
        mean, inv = torch.empty(C, device=dev), torch.empty(C, device=dev)
        bws = torch.zeros(C_.bn_workspace_floats(C), device=dev)

        def bn(ready=True):
            C_.bn_fwd(xb, yb, None, gamma, beta, None, None, mean, inv, bws, 1e-5, 0.0, True, False, None,
                      stats_ready=ready)

        bn(False)   # (leaves the coefficients the apply-only calls read)
        t = timed({"fwd": lambda: C_.dwconv_fwd(x, w, y, st), "dgrad": lambda: C_.dwconv_dgrad(dy, w, dx, st),
                   "wgrad": lambda: C_.dwconv_wgrad(x, dy, ws, dw, C, False, st), "bn_apply": bn}, reps)
        io = 2 * (x.numel() + y.numel())
        rec = {"shape_nhwc": [N, H, H, C], "stride": st, "reps": reps, "dw_bytes": io, "bn_apply_bytes": 4 * x.numel(),
               "wgrad_slices": ws.numel() // (9 * C)}
        rec.update({k + "_us": round(v, 2) for k, v in t.items()})
        rec.update({k + "_TBps": round((4 * x.numel() if k == "bn_apply" else io) / v / 1e6, 3) for k, v in t.items()})
        rec.update({k + "_over_bn_apply_rate": round(rec[k + "_TBps"] / rec["bn_apply_TBps"], 3)
                    for k in ("fwd", "dgrad", "wgrad")})
        print(json.dumps(rec), flush=True)


def steps(N, n_steps):
    from ldnn.models import CrossEntropyLoss, build_model, xavier_init
    from ldnn.optim import SGD
    from ldnn.train.graphed import GraphedStep

    torch.manual_seed(0)
    x = torch.randn(N, 3, 32, 32, device="cuda").bfloat16()
    y = torch.randint(0, 10, (N,), device="cuda")
    runs = {}
    for key, sep in (("dense", False), ("separable", True)):
        m = build_model("enhanced_cnn", separable=sep)
        xavier_init(m)
        ldnn.prepare(m, "cuda")
        opt = SGD(m.parameters(), lr=0.01, momentum=0.9)
        gs = GraphedStep(m, CrossEntropyLoss(), opt, x, y)
        runs[key] = (lambda gs=gs: gs(x, y), sum(p.numel() for p in m.parameters()))
    t = timed({k: v[0] for k, v in runs.items()}, n_steps)
    print(json.dumps({"model": "enhanced_cnn", "batch": N, "steps": n_steps,
                      **{k + "_params": v[1] for k, v in runs.items()},
                      **{k + "_graphed_step_us": round(v, 1) for k, v in t.items()}}), flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--batch", type=int, default=64)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_dwconv.py measures on the GPU"
    kernels(a.batch, a.reps)
    steps(a.batch, a.steps)
