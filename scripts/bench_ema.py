"""Cost of the weight-EMA pass on a model's real flat buffers, same process, HIP events: the fused
Adam alone (30 B per element), ``ema_update`` alone (12 B: read w, e; write e), the pair "Adam then
ema_update" as a step issues them (``ema_begin`` included), and ``ema_swap`` (18 B: read w, e; write
w, e, shadow).  The yardstick is bytes: ``ema_update`` should cost about 12 / 30 = 0.4x the Adam's
time, the pair about 1.4x.

The loops re-read the same buffers (ResNet-18: 47 MB each, EnhancedCNN: 179 MB each); ``--flush``
streams a 512 MiB buffer before every timed iteration so that nothing is left in the 256 MiB
Infinity Cache.  lr is 0 and the gradient is rewritten by nobody, so the weights stay put.

    python scripts/bench_ema.py [--model resnet18] [--iters 50] [--flush]
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
    return ts[len(ts) // 2] * 1e-3, (ts[len(ts) // 4] * 1e-3, ts[3 * len(ts) // 4] * 1e-3)      # median, quartiles (s)


def setup(model):
    """The model's flat buffers with a gradient of the weights' own scale, Adam moments, an average
    that differs from the master, and the EMA header [d, warm-up, c, a_t]."""
    torch.manual_seed(0)
    m = build_model(model)
    xavier_init(m)
    f = ldnn.prepare(m, "cuda")
    for s in f.segments:
        s.param.grad.copy_(torch.randn_like(s.param) * 0.01)
    mm, vv = torch.zeros_like(f.master), torch.zeros_like(f.master)
    ema = f.master * 0.5
    hp = torch.tensor([0.0, 1.0], device="cuda")      # lr 0: the weights stay put over the iterations
    hdr = torch.tensor([0.999, 0.0, 0.0, 0.0], device="cuda")
    return f, mm, vv, ema, hp, hdr


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="resnet18")
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--flush", action="store_true", help="stream 512 MiB before every timed iteration (cold cache)")
    a = ap.parse_args()
    c = C()
    f, mm, vv, ema, hp, hdr = setup(a.model)
    n = f.numel
    junk = torch.empty(128 << 20, device="cuda") if a.flush else None
    flush = (lambda: junk.add_(1.0)) if a.flush else None

    def adam():
        c.adam_step(f.master, f.grad, mm, vv, f.shadow, hp, 1.0, 0.9, 0.999, 1e-8, 0.0, False)

    def update():
        c.ema_update(f.master, ema, hdr)

    def pair():
        c.ema_begin(hdr)
        adam()
        update()

    def swap():
        c.ema_swap(f.master, ema, f.shadow)

    c.ema_begin(hdr)      # (a_t = 0.001 for the rows that do not begin a step themselves)
    rows = {}
    for name, fn in (("adam", adam), ("ema_update", update), ("adam_then_ema", pair), ("ema_swap", swap),
                     ("adam_again", adam)):
        rows[name] = timed(fn, a.iters, before=flush)      # (iters is even: the swaps leave the buffers as they were)
    us = lambda v: round(v * 1e6, 2)  # noqa: E731
    rec = {"model": a.model, "n": n, "flush": a.flush, "buffer_MB": round(4 * n / 1e6, 1)}
    for name, (med, (q1, q3)) in rows.items():
        rec[name + "_us"] = us(med)
        rec[name + "_iqr_us"] = [us(q1), us(q3)]
    rec["adam_TBps"] = round(30 * n / rows["adam"][0] / 1e12, 3)
    rec["ema_update_TBps"] = round(12 * n / rows["ema_update"][0] / 1e12, 3)
    rec["ema_swap_TBps"] = round(18 * n / rows["ema_swap"][0] / 1e12, 3)
    rec["ema_over_adam"] = round(rows["ema_update"][0] / rows["adam"][0], 3)
    rec["pair_over_adam"] = round(rows["adam_then_ema"][0] / rows["adam"][0], 3)
    print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
