"""Cost of the LARS kernels on a model's real flat buffers, same process, HIP events:
seg_sumsq + lars_finalize alone (beside grad_sumsq + clip_finalize, which reads half the bytes),
the fused SGD with and without the ratio lookup, and the triple of a LARS step.

The stand-alone loops re-read the same buffers: master + gradient of ResNet-18 (94 MB) and
EnhancedCNN (357 MB) -- the first stays in the 256 MiB Infinity Cache between iterations, the
second does not, and ``--flush`` streams a 512 MiB buffer before every iteration of the norm
loops to time them cold.  ``lars_cost_us`` (triple minus the plain SGD) is the number that
matches a training step, where the backward has just written the gradient.

    python scripts/bench_lars.py [--model resnet18] [--iters 50] [--flush]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import ldnn  # noqa: E402
from ldnn.models import build_model, xavier_init  # noqa: E402
from ldnn.ops._ext import C  # noqa: E402
from ldnn.optim.optimizers import _Lars  # noqa: E402


def timed(fn, iters, warmup=10, before=None):
    for _ in range(warmup):
        fn()
    evs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(iters)]
    torch.cuda.synchronize()
    for e0, e1 in evs:
        if before is not None:
            before()
        e0.record()
        fn()
        e1.record()
    torch.cuda.synchronize()
    ts = sorted(e0.elapsed_time(e1) for e0, e1 in evs)
    return ts[len(ts) // 2] * 1e-3      # median, seconds


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="resnet18")
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--flush", action="store_true", help="stream 512 MiB before every timed iteration (cold cache)")
    a = ap.parse_args()
    c = C()
    torch.manual_seed(0)
    m = build_model(a.model)
    xavier_init(m)
    f = ldnn.prepare(m, "cuda")
    n = f.numel
    for s in f.segments:      # a gradient of the weights' own scale, zero in the padding like a real one
        s.param.grad.copy_(torch.randn_like(s.param) * 0.01)
    mom = torch.zeros_like(f.master)
    hp = torch.tensor([0.0, 0.0], device="cuda")      # lr 0: the weights stay put over the iterations
    st = torch.zeros(8, device="cuda")
    st[0] = 1e30
    scratch = torch.zeros(c.grad_sumsq_parts(n), device="cuda")
    L = _Lars(f, None, True, f.master.device)
    L.hdr.copy_(torch.tensor([1.0, 1e-8]))
    t = L.table([(0, n)], False)
    offs = L.offsets
    junk = torch.empty(128 << 20, device="cuda") if a.flush else None
    flush = (lambda: junk.add_(1.0)) if a.flush else None

    def sgd(lars=None):
        c.sgd_step(f.master, f.grad, mom, f.shadow, hp, 1.0, 0.9, 0.0, 1e-4, False, False, lars=lars)

    def clip_norm():
        c.clip_finalize(scratch, c.grad_sumsq(f.grad, scratch, 0), st, 1.0)

    def lars_norm():
        c.seg_sumsq(f.master, f.grad, t["chunks"], t["partials"], t["ranges"], offs)
        c.lars_finalize(t["partials"], t["segtab"], L.hdr, L.ratio, L.w_norm, L.g_norm, 1.0, 1e-4)

    def triple():
        lars_norm()
        sgd((L.ratio, L.segmap))

    t_sgd = timed(sgd, a.iters, before=flush)
    t_sgdl = timed(lambda: sgd((L.ratio, L.segmap)), a.iters, before=flush)
    t_clip = timed(clip_norm, a.iters, before=flush)
    t_norm = timed(lars_norm, a.iters, before=flush)
    t_tri = timed(triple, a.iters, before=flush)
    us = lambda v: round(v * 1e6, 2)  # noqa: E731
    rec = {"model": a.model, "n": n, "segments": L.S, "chunks": int(t["chunks"].shape[0]), "flush": a.flush,
           "master_plus_grad_MB": round(8 * n / 1e6, 1),
           "sgd_us": us(t_sgd), "sgd_lars_us": us(t_sgdl), "sgd_bytes": 22 * n,   # r+w master, momentum; r grad; w shadow
           "sgd_TBps": round(22 * n / t_sgd / 1e12, 3),
           "grad_sumsq_clip_finalize_us": us(t_clip), "grad_sumsq_TBps": round(4 * n / t_clip / 1e12, 3),
           "seg_sumsq_lars_finalize_us": us(t_norm), "seg_sumsq_TBps": round(8 * n / t_norm / 1e12, 3),
           "triple_us": us(t_tri), "lars_cost_us": us(t_tri - t_sgd)}
    print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
