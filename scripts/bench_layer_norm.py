#!/usr/bin/env python
"""Kernel rates of the LayerNorm row passes beside the activation passes that move the same bytes:
ln_fwd against act_fwd (4 B per element), ln_bwd plus its finalize against act_bwd (6 B per
element), in one process on the same buffers, alternated, HIP events, medians of `--reps`; warm
(the loop re-reads its buffers) and with 512 MiB streamed through the cache before every timed
iteration.  One JSON line per shape."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ldnn.ops import _ext  # noqa: E402

SHAPES = [(16384, 4096), (16384, 1024)]   # the flagship MLP's hidden activation at batch 16384, and a narrow one


def timed(fns, reps, before=None, warm=5):
    ts = {k: [] for k in fns}
    for i in range(warm + reps):
        for k, fn in fns.items():
            if before is not None:
                before()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            if i >= warm:
                ts[k].append(a.elapsed_time(b) * 1e3)
    return {k: statistics.median(v) for k, v in ts.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--act", choices=["relu", "sigmoid"], default="relu")
    a = ap.parse_args()
    C_ = _ext.C()
    dev = "cuda"
    act = {"relu": 0, "sigmoid": 1}[a.act]
    junk = torch.empty(128 << 20, device=dev)   # 512 MiB of fp32: more than the 256 MiB last-level cache
    for B, N in SHAPES:
        x = (1.5 * torch.randn(B, N, device=dev) + 0.5).bfloat16()
        dy, y, dx = torch.randn(B, N, device=dev).bfloat16(), torch.empty_like(x), torch.empty_like(x)
        gamma, beta = 1 + 0.3 * torch.randn(N, device=dev), 0.2 * torch.randn(N, device=dev)
        mean, rstd = torch.empty(B, device=dev), torch.empty(B, device=dev)
        ws = torch.empty(C_.ln_workspace_floats(B, N), device=dev)
        dg, db = torch.empty(N, device=dev), torch.empty(N, device=dev)
        xf, yf, dyf, dxf = x.view(-1), y.view(-1), dy.view(-1), dx.view(-1)
        fns_f = {"ln_fwd": lambda: C_.ln_fwd(x, y, gamma, beta, mean, rstd, 1e-5, act),
                 "act_fwd": lambda: C_.act_fwd(xf, yf, act)}
        fns_b = {"ln_bwd": lambda: C_.ln_bwd(x, dy, dx, gamma, beta, mean, rstd, ws, dg, db, act, grad_assign=True),
                 "ln_bwd_no_affine": lambda: C_.ln_bwd(x, dy, dx, None, None, mean, rstd, None, None, None, act),
                 "act_bwd": lambda: C_.act_bwd(dyf, yf, dxf, act)}
        fns_f["ln_fwd"]()
        n = x.numel()
        fb, bb = 4 * n, 6 * n
        rec = {"shape": [B, N], "act": a.act, "reps": a.reps, "fwd_bytes": fb, "bwd_bytes": bb,
               "ln_workspace_bytes": 4 * ws.numel()}
        for tag, before in (("warm", None), ("cold", lambda: junk.add_(1.0))):
            t = {**timed(fns_f, a.reps, before), **timed(fns_b, a.reps, before)}
            rec.update({f"{k}_{tag}_us": round(v, 2) for k, v in t.items()})
            rec.update({f"{k}_{tag}_TBps": round((fb if k.endswith("fwd") else bb) / v / 1e6, 3) for k, v in t.items()})
        print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
