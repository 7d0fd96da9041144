"""Achieved bytes/s of the clipping kernels beside the fused Adam's, same process, HIP events:
grad_sumsq (+ clip_finalize) measured alone and right before the fused Adam that re-reads the
same gradient (the order of a clipped step).

The stand-alone grad_sumsq loop re-reads ONE buffer: up to 256 MiB (EnhancedCNN's 178 MB) it
stays in the Infinity Cache between iterations, so that figure is a warm-cache rate, while the
Adam's 30 bytes per element do not fit.  ``clip_cost_us`` (norm + Adam minus Adam alone) is the
number that matches a training step, where the backward has just written the gradient.

    python scripts/bench_grad_clip.py [--n 44595786] [--iters 50]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ldnn.ops._ext import C  # noqa: E402


def timed(fn, iters, warmup=10):
    for _ in range(warmup):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e-3 / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=44_595_786, help="elements (default: EnhancedCNN's parameters)")
    ap.add_argument("--iters", type=int, default=50)
    a = ap.parse_args()
    n = a.n
    c = C()
    p, g, m, v = (torch.randn(n, device="cuda") * 0.01 for _ in range(4))
    v.abs_()
    sh = torch.empty(n, device="cuda", dtype=torch.bfloat16)
    hp = torch.tensor([1e-3, 1.0], device="cuda")
    st = torch.zeros(8, device="cuda")
    st[0] = 1e30
    scratch = torch.zeros(c.grad_sumsq_parts(n), device="cuda")

    def adam(clip=None):
        c.adam_step(p, g, m, v, sh, hp, 1.0, 0.9, 0.999, 1e-8, 0.0, False, clip=clip)

    def norm():
        c.clip_finalize(scratch, c.grad_sumsq(g, scratch, 0), st, 1.0)

    def clipped():
        norm()
        adam(st)

    t_adam = timed(adam, a.iters)
    rec = {"n": n, "adam_us": round(t_adam * 1e6, 2), "adam_bytes": 30 * n,
           "adam_TBps": round(30 * n / t_adam / 1e12, 3)}   # r+w master, m, v (24 B), r grad (4 B), w shadow (2 B)
    t_n = timed(norm, a.iters)
    t_c = timed(clipped, a.iters)
    rec.update({"sumsq_us": round(t_n * 1e6, 2), "sumsq_TBps": round(4 * n / t_n / 1e12, 3),
                "norm_plus_adam_us": round(t_c * 1e6, 2), "clip_cost_us": round((t_c - t_adam) * 1e6, 2)})
    print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
