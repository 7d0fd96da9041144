"""Cost of the Lion kernel beside the fused Adam on a model's real flat buffers, same process, HIP
events: lion_step reads w, g, m and writes w, m and the bf16 shadow (3 * 4 + 2 * 4 + 2 = 22 B per
element), adam_step also reads and writes v (30 B).  The yardstick is bytes: Lion should cost about
22 / 30 = 0.73x the Adam's time.  The two are timed alternately (lion, adam, lion, adam) so a drift
of the box shows as a difference between the two rounds.

The loops re-read the same buffers (ResNet-18: 47 MB each, EnhancedCNN: 179 MB each); ``--flush``
streams a 512 MiB buffer before every timed iteration so that nothing is left in the 256 MiB
Infinity Cache.  lr is 0 and the gradient is rewritten by nobody, so the weights stay put.

    python scripts/bench_lion.py [--model resnet18] [--iters 50] [--flush]
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

LION_BYTES = 3 * 4 + 2 * 4 + 2      # read w, g, m; write w, m, bf16 shadow
ADAM_BYTES = 4 * 4 + 3 * 4 + 2      # read w, g, m, v; write w, m, v, bf16 shadow


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
    mm, vv = torch.zeros_like(f.master), torch.zeros_like(f.master)
    hp = torch.tensor([0.0, 1.0], device="cuda")      # lr 0: the weights stay put over the iterations
    junk = torch.empty(128 << 20, device="cuda") if a.flush else None
    flush = (lambda: junk.add_(1.0)) if a.flush else None

    def lion():
        c.lion_step(f.master, f.grad, mm, f.shadow, hp, 1.0, 0.9, 0.99, 0.0)

    def lion_wd():
        c.lion_step(f.master, f.grad, mm, f.shadow, hp, 1.0, 0.9, 0.99, 0.1)

    def adam():
        c.adam_step(f.master, f.grad, mm, vv, f.shadow, hp, 1.0, 0.9, 0.999, 1e-8, 0.0, False)

    rows = {}
    for name, fn in (("lion", lion), ("adam", adam), ("lion_again", lion), ("adam_again", adam), ("lion_wd", lion_wd)):
        rows[name] = timed(fn, a.iters, before=flush)
    us = lambda v: round(v * 1e6, 2)  # noqa: E731
    rec = {"model": a.model, "n": n, "flush": a.flush, "iters": a.iters, "buffer_MB": round(4 * n / 1e6, 1),
           "lion_B_per_elem": LION_BYTES, "adam_B_per_elem": ADAM_BYTES, "par": round(LION_BYTES / ADAM_BYTES, 3)}
    for name, (med, (q1, q3)) in rows.items():
        rec[name + "_us"] = us(med)
        rec[name + "_iqr_us"] = [us(q1), us(q3)]
    for k in ("lion", "lion_again"):
        rec[k + "_TBps"] = round(LION_BYTES * n / rows[k][0] / 1e12, 3)
    for k in ("adam", "adam_again"):
        rec[k + "_TBps"] = round(ADAM_BYTES * n / rows[k][0] / 1e12, 3)
    rec["lion_over_adam"] = round(rows["lion"][0] / rows["adam"][0], 3)
    rec["lion_over_adam_again"] = round(rows["lion_again"][0] / rows["adam_again"][0], 3)
    print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
