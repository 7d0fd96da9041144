#!/usr/bin/env python
"""Rates of the mxfp8 Linear's kernels (quant_mx8.hip, gemm_f8.hip) beside the per-tensor fp8 path and bf16, at a
4096 x 4096 hidden layer and batch 4096.  The variants alternate inside one process (HIP events around single
launches, medians of --reps); every record is one JSON line, printed and appended to <out>/bench_mxfp8.jsonl.

  quant : mx8_quantize (one launch, both orientations) on a 4096 x 4096 bf16 tensor beside the per-tensor trio
          (f8_amax = two launches, f8_cast_transpose) on the same input, and beside the BatchNorm apply pass
          (bn_fwd with stats_ready: one bf16 read, one bf16 write), the yardstick of the streaming kernels.
  gemm  : gemm_mx8 beside gemm_f8 and C.gemm for the forward, dgrad and wgrad shapes.
  step  : the graphed mlp3 step at --batch in bf16, fp8 and mxfp8.
  train : train.py --model mlp3 --dataset mnist-hard, two global epochs, same seed, the three dtypes (child
          processes, one after the other); the last epoch's line of each goes to <out>/train_mnist_hard.txt.

    python scripts/bench_mxfp8.py [--reps 50] [--steps 40] [--batch 4096] [--out profiles/r26] [--parts quant,gemm,step,train]
"""
import argparse
import json
import os
import subprocess
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import ldnn  # noqa: E402
from bench_fp8 import timed  # noqa: E402
from ldnn.ops import _ext  # noqa: E402
from ldnn.ops import functional as LF  # noqa: E402

OUT = None


def emit(rec):
    line = json.dumps(rec)
    print(line, flush=True)
    with open(os.path.join(OUT, "bench_mxfp8.jsonl"), "a") as f:
        f.write(line + "\n")


def quant(H, reps):
    C = _ext.C()
    dev = "cuda"
    x = torch.randn(H, H, device=dev).bfloat16()
    words = torch.empty(4, device=dev)
    u8 = lambda *s: torch.empty(*s, dtype=torch.uint8, device=dev)
    out, out_t, none = u8(H, H), u8(H, H), u8(0)
    mo, ms, mt, mts = u8(H, H), u8(H, H // 32), u8(H, H), u8(H, H // 32)
    yb = torch.empty_like(x)
    gamma, beta = torch.ones(H, device=dev), torch.zeros(H, device=dev)
    mean, inv = torch.empty(H, device=dev), torch.empty(H, device=dev)
    bws = torch.zeros(C.bn_workspace_floats(H), device=dev)

    def bn(ready=True):
        C.bn_fwd(x, yb, None, gamma, beta, None, None, mean, inv, bws, 1e-5, 0.0, True, False, None, stats_ready=ready)

    def trio():
        C.f8_amax(x, words, 0)
        C.f8_cast_transpose(x, words, 0, out, out_t)

    bn(False)   # (leaves the coefficients the apply-only calls read)
    t = timed({"mx8_quantize": lambda: C.mx8_quantize(x, 0, mo, ms, mt, mts),
               "mx8_quantize_rows_only": lambda: C.mx8_quantize(x, 0, mo, ms, none, none),
               "f8_trio": trio,
               "f8_amax": lambda: C.f8_amax(x, words, 0),
               "f8_cast_transpose": lambda: C.f8_cast_transpose(x, words, 0, out, out_t),
               "bn_apply": bn}, reps)
    n = x.numel()
    byts = {"mx8_quantize": (2 + 2 * (1 + 1 / 32)) * n, "mx8_quantize_rows_only": (2 + 1 + 1 / 32) * n, "f8_trio": 6 * n,
            "f8_amax": 2 * n, "f8_cast_transpose": 4 * n, "bn_apply": 4 * n}
    rec = {"kind": "quant", "shape": [H, H], "reps": reps}
    rec.update({k + "_us": round(v, 1) for k, v in t.items()})
    rec.update({k + "_TBps": round(byts[k] / v / 1e6, 3) for k, v in t.items()})
    rec["mx8_over_f8_trio_time"] = round(t["mx8_quantize"] / t["f8_trio"], 3)
    rec["mx8_over_bn_apply_rate"] = round(rec["mx8_quantize_TBps"] / rec["bn_apply_TBps"], 3)
    emit(rec)


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
    mx, mxs, mxt, mxts = LF.mx8_quantize(x, "e4m3")
    mw, mws, mwt, mwts = LF.mx8_quantize(w, "e4m3")
    mg, mgs, mgt, mgts = LF.mx8_quantize(gz, "e5m2")
    t = timed({
        "fwd_mxfp8": lambda: C.gemm_mx8(mx, mxs, mw, mws, y, 0, C.EPI_BIAS_RELU, bias=bias),
        "fwd_fp8": lambda: C.gemm_f8(x8, w8, y, xw, ww, 0, C.EPI_BIAS_RELU, bias=bias),
        "fwd_bf16": lambda: C.gemm(x, w, y, True, True, C.EPI_BIAS_RELU, bias=bias),
        "dgrad_mxfp8": lambda: C.gemm_mx8(mg, mgs, mwt, mwts, dx, 1, C.EPI_NONE),
        "dgrad_fp8": lambda: C.gemm_f8(g8, wt8, dx, gw, ww, 1, C.EPI_NONE),
        "dgrad_bf16": lambda: C.gemm(gz, w, dx, True, False),
        "wgrad_mxfp8": lambda: C.gemm_mx8(mgt, mgts, mxt, mxts, dw, 1, C.EPI_NONE),
        "wgrad_fp8": lambda: C.gemm_f8(gt8, xt8, dw, gw, xw, 1, C.EPI_NONE),
        "wgrad_bf16": lambda: C.gemm(gz, x, dw, False, False),
    }, reps)
    flop = 2.0 * B * H * H
    rec = {"kind": "gemm", "B": B, "K": H, "N": H, "reps": reps}
    rec.update({k + "_us": round(v, 1) for k, v in t.items()})
    rec.update({k + "_TFLOPs": round(flop / v / 1e6, 1) for k, v in t.items()})
    for g in ("fwd", "dgrad", "wgrad"):
        rec[g + "_mxfp8_over_bf16_time"] = round(t[g + "_mxfp8"] / t[g + "_bf16"], 3)
        rec[g + "_mxfp8_over_fp8_time"] = round(t[g + "_mxfp8"] / t[g + "_fp8"], 3)
    emit(rec)


def steps(B, n_steps):
    from ldnn.models import CrossEntropyLoss, build_model, xavier_init
    from ldnn.optim import SGD
    from ldnn.train.graphed import GraphedStep

    torch.manual_seed(0)
    x = torch.randn(B, 784, device="cuda").bfloat16()
    y = torch.randint(0, 10, (B,), device="cuda")
    runs = {}
    for dt in ("bf16", "fp8", "mxfp8"):
        m = build_model("mlp3", linear_dtype=dt)
        xavier_init(m)
        ldnn.prepare(m, "cuda")
        opt = SGD(m.parameters(), lr=0.01, momentum=0.9)
        gs = GraphedStep(m, CrossEntropyLoss(), opt, x, y)
        runs[dt] = lambda gs=gs: gs(x, y)
    t = timed(runs, n_steps)
    emit({"kind": "step", "model": "mlp3", "batch": B, "steps": n_steps,
          **{k + "_graphed_step_us": round(v, 1) for k, v in t.items()},
          "mxfp8_over_bf16_time": round(t["mxfp8"] / t["bf16"], 3),
          "mxfp8_over_fp8_time": round(t["mxfp8"] / t["fp8"], 3)})


def train():
    cmd = [sys.executable, os.path.join(ROOT, "train.py"), "--model", "mlp3", "--dataset", "mnist-hard", "--epochs_global",
           "2", "--epochs_local", "1", "--batch_size", "256", "--seed", "0", "--engine", "autograd"]
    with open(os.path.join(OUT, "train_mnist_hard.txt"), "a") as f:
        f.write("# " + " ".join(["train.py"] + cmd[2:]) + "\n")
        for dt in ("bf16", "fp8", "mxfp8"):
            r = subprocess.run(cmd + ["--linear_dtype", dt], capture_output=True, text=True, cwd=ROOT, timeout=900)
            lines = (r.stdout + r.stderr).splitlines()
            keep = [ln for ln in lines if "global epoch 2" in ln or "Test Accuracy" in ln] or lines[-5:]
            f.write(f"{dt} (rc {r.returncode}): " + " | ".join(ln.strip() for ln in keep) + "\n")
            f.flush()
            print(dt, r.returncode, keep, flush=True)
            if r.returncode != 0:   # (nothing more is started on the GPU after a failed child)
                raise SystemExit(f"train.py --linear_dtype {dt} failed: rc {r.returncode}")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r26"))
    ap.add_argument("--parts", default="quant,gemm,step", help="comma-separated: quant, gemm, step, train")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_mxfp8.py measures on the GPU"
    OUT = a.out
    os.makedirs(OUT, exist_ok=True)
    parts = a.parts.split(",")
    if "quant" in parts:
        quant(4096, a.reps)
    if "gemm" in parts:
        gemms(a.batch, 4096, a.reps)
    if "step" in parts:
        steps(a.batch, a.steps)
    if "train" in parts:
        train()
