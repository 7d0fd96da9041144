#!/usr/bin/env python
"""Kernel rates of the GroupNorm streaming passes beside the BatchNorm apply passes that move the
same bytes: gn_fwd(apply_only) against bn_fwd(stats_ready=True), gn_bwd(apply_only) against
bn_bwd(stats_ready=True), in one process on the same buffers, alternated, HIP events, medians of
`--reps`; the whole three-launch GroupNorm calls beside them.  One JSON line per shape."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ldnn.ops import _ext  # noqa: E402

SHAPES = [(64, 32, 32, 64), (64, 2, 2, 1024), (64, 56, 56, 64)]   # NHWC: EnhancedCNN b64 first / last, ResNet-18 b64


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--groups", type=int, default=32)
    a = ap.parse_args()
    C_ = _ext.C()
    dev = "cuda"
    for N, H, W, C in SHAPES:
        G, M = a.groups, N * H * W
        x = (1.5 * torch.randn(N, H, W, C, device=dev) + 0.5).bfloat16()
        dy, y, dx = torch.randn_like(x), torch.empty_like(x), torch.empty_like(x)
        mask = torch.empty(x.numel() // 8, dtype=torch.uint8, device=dev)
        gamma, beta = torch.ones(C, device=dev), torch.zeros(C, device=dev)
        mean, rstd = torch.empty(N * G, device=dev), torch.empty(N * G, device=dev)
        ws = torch.empty(C_.gn_workspace_floats(N, H * W, C, G), device=dev)
        dg, db = torch.empty(C, device=dev), torch.empty(C, device=dev)
        bws = torch.zeros(C_.bn_workspace_floats(C), device=dev)
        bmean, binv = torch.empty(C, device=dev), torch.empty(C, device=dev)
        bdg, bdb = torch.empty(C, device=dev), torch.empty(C, device=dev)
        x2, y2, dy2, dx2 = x.view(M, C), y.view(M, C), dy.view(M, C), dx.view(M, C)

        def gn_fwd(apply_only):
            C_.gn_fwd(x, y, None, gamma, beta, mean, rstd, ws, G, 1e-5, True, mask=mask, apply_only=apply_only)

        def gn_bwd(apply_only):
            C_.gn_bwd(x, dy, dx, None, gamma, mean, rstd, ws, dg, db, G, True, mask=mask, grad_assign=True,
                      apply_only=apply_only)

        def bn_fwd(ready):
            C_.bn_fwd(x2, y2, None, gamma, beta, None, None, bmean, binv, bws, 1e-5, 0.0, True, True, None,
                      stats_ready=ready, mask=mask)

        def bn_bwd(ready):
            C_.bn_bwd(x2, x2, dy2, dx2, None, gamma, bmean, binv, bws, bdg, bdb, True, mask=mask, grad_assign=True,
                      stats_ready=ready)

        # whole calls first: they leave the coefficients the apply-only calls read
        gn_fwd(False)
        bn_fwd(False)
        fwd = timed({"gn_apply": lambda: gn_fwd(True), "bn_apply": lambda: bn_fwd(True),
                     "gn_fwd_whole": lambda: gn_fwd(False), "bn_fwd_whole": lambda: bn_fwd(False)}, a.reps)
        gn_bwd(False)
        bn_bwd(False)
        bwd = timed({"gn_bwd_apply": lambda: gn_bwd(True), "bn_bwd_apply": lambda: bn_bwd(True),
                     "gn_bwd_whole": lambda: gn_bwd(False), "bn_bwd_whole": lambda: bn_bwd(False)}, a.reps)
        n = x.numel()
        fb, bb = n * (2 + 2 + 0.125), n * (2 + 2 + 2 + 0.125)   # x, y, mask / x, dy, dx, mask
        rec = {"shape_nhwc": [N, H, W, C], "groups": G, "slabs": C_.gn_slabs(N, H * W, C, G), "reps": a.reps,
               "fwd_apply_bytes": fb, "bwd_apply_bytes": bb}
        rec.update({k + "_us": round(v, 2) for k, v in {**fwd, **bwd}.items()})
        rec.update(gn_apply_TBps=round(fb / fwd["gn_apply"] / 1e6, 3), bn_apply_TBps=round(fb / fwd["bn_apply"] / 1e6, 3),
                   gn_bwd_apply_TBps=round(bb / bwd["gn_bwd_apply"] / 1e6, 3),
                   bn_bwd_apply_TBps=round(bb / bwd["bn_bwd_apply"] / 1e6, 3))
        print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
