#!/usr/bin/env python
"""Rates of the fp8 Linear's kernels (gemm_f8.hip, quant_f8.hip) at a 4096 x 4096 hidden layer and batch 4096.
The three gemm_f8 shapes (forward, dgrad, wgrad) beside C.gemm on bf16 operands of the same logical shape; the
two cast kernels on a 4096 x 4096 bf16 tensor beside the BatchNorm apply pass (bn_fwd with stats_ready: one bf16
read, one bf16 write), the yardstick of the other streaming kernels; then the graphed mlp3 step with
linear_dtype="fp8" beside bf16.  One process, alternated, HIP events, medians of --reps.  One JSON line each.

    python scripts/bench_fp8.py [--reps 50] [--steps 40] [--batch 4096]
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
from ldnn.ops import functional as LF  # noqa: E402


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


def gemms(B, H, reps):
    C = _ext.C()
    dev = "cuda"
    x = torch.randn(B, H, device=dev).bfloat16()
    w = (torch.randn(H, H, device=dev) * 0.02).bfloat16()
    gz = torch.randn(B, H, device=dev).bfloat16()
    bias = torch.zeros(H, device=dev)
    y, dx, dw = torch.empty_like(x), torch.empty_like(x), torch.empty(H, H, device=dev)
    x8, xt8, xw = LF.fp8_quantize(x, "e4m3")
    w8, wt8, ww = LF.fp8_quantize(w, "e4m3")
    g8, gt8, gw = LF.fp8_quantize(gz, "e5m2")
    t = timed({
        "fwd_fp8": lambda: C.gemm_f8(x8, w8, y, xw, ww, 0, C.EPI_BIAS_RELU, bias=bias),
        "fwd_bf16": lambda: C.gemm(x, w, y, True, True, C.EPI_BIAS_RELU, bias=bias),
        "dgrad_fp8": lambda: C.gemm_f8(g8, wt8, dx, gw, ww, 1, C.EPI_NONE),
        "dgrad_bf16": lambda: C.gemm(gz, w, dx, True, False),
        "wgrad_fp8": lambda: C.gemm_f8(gt8, xt8, dw, gw, xw, 1, C.EPI_NONE),
        "wgrad_bf16": lambda: C.gemm(gz, x, dw, False, False),
    }, reps)
    flop = 2.0 * B * H * H
    rec = {"kind": "gemm", "B": B, "K": H, "N": H, "reps": reps}
    rec.update({k + "_us": round(v, 1) for k, v in t.items()})
    rec.update({k + "_TFLOPs": round(flop / v / 1e6, 1) for k, v in t.items()})
    rec.update({g + "_fp8_over_bf16_time": round(t[g + "_fp8"] / t[g + "_bf16"], 3) for g in ("fwd", "dgrad", "wgrad")})
    print(json.dumps(rec), flush=True)


def casts(H, reps):
    C = _ext.C()
    dev = "cuda"
    x = torch.randn(H, H, device=dev).bfloat16()
    words = torch.empty(4, device=dev)
    out, out_t = torch.empty(H, H, dtype=torch.uint8, device=dev), torch.empty(H, H, dtype=torch.uint8, device=dev)
    none = torch.empty(0, dtype=torch.uint8, device=dev)
    yb = torch.empty_like(x)
    gamma, beta = torch.ones(H, device=dev), torch.zeros(H, device=dev)
    mean, inv = torch.empty(H, device=dev), torch.empty(H, device=dev)
    bws = torch.zeros(C.bn_workspace_floats(H), device=dev)

    def bn(ready=True):
        C.bn_fwd(x, yb, None, gamma, beta, None, None, mean, inv, bws, 1e-5, 0.0, True, False, None, stats_ready=ready)

    bn(False)   # (leaves the coefficients the apply-only calls read)
    C.f8_amax(x, words, 0)
    t = timed({"amax": lambda: C.f8_amax(x, words, 0),
               "cast_transpose": lambda: C.f8_cast_transpose(x, words, 0, out, out_t),
               "cast_only": lambda: C.f8_cast_transpose(x, words, 0, out, none),
               "bn_apply": bn}, reps)
    n = x.numel()
    byts = {"amax": 2 * n, "cast_transpose": 4 * n, "cast_only": 3 * n, "bn_apply": 4 * n}
    rec = {"kind": "cast", "shape": [H, H], "reps": reps}
    rec.update({k + "_us": round(v, 1) for k, v in t.items()})
    rec.update({k + "_TBps": round(byts[k] / v / 1e6, 3) for k, v in t.items()})
    rec.update({k + "_over_bn_apply_rate": round(rec[k + "_TBps"] / rec["bn_apply_TBps"], 3)
                for k in ("amax", "cast_transpose", "cast_only")})
    print(json.dumps(rec), flush=True)


def steps(B, n_steps):
    from ldnn.models import CrossEntropyLoss, build_model, xavier_init
    from ldnn.optim import SGD
    from ldnn.train.graphed import GraphedStep

    torch.manual_seed(0)
    x = torch.randn(B, 784, device="cuda").bfloat16()
    y = torch.randint(0, 10, (B,), device="cuda")
    runs = {}
    for dt in ("bf16", "fp8"):
        m = build_model("mlp3", linear_dtype=dt)
        xavier_init(m)
        ldnn.prepare(m, "cuda")
        opt = SGD(m.parameters(), lr=0.01, momentum=0.9)
        gs = GraphedStep(m, CrossEntropyLoss(), opt, x, y)
        runs[dt] = lambda gs=gs: gs(x, y)
    t = timed(runs, n_steps)
    print(json.dumps({"kind": "step", "model": "mlp3", "batch": B, "steps": n_steps,
                      **{k + "_graphed_step_us": round(v, 1) for k, v in t.items()},
                      "fp8_over_bf16_time": round(t["fp8"] / t["bf16"], 3)}), flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--batch", type=int, default=4096)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_fp8.py measures on the GPU"
    gemms(a.batch, 4096, a.reps)
    casts(4096, a.reps)
    steps(a.batch, a.steps)
