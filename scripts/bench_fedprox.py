"""Cost of the FedProx term in the fused updates on a model's real flat buffers, same process, HIP
events: sgd_step (momentum), adam_step and lion_step with and without prox=.  The term is one more
streamed operand, the fp32 anchor (4 B per element), so the yardstick is bytes: SGD-momentum 26 / 22
(w, g, momentum read; w, momentum, bf16 shadow written; + anchor), Adam 34 / 30, Lion 26 / 22.

Every pair is timed in alternating rounds (plain, prox, plain, prox): a drift of the box shows as a
difference between the two rounds of the same launch, and that spread of the plain launch is the margin
the measured ratio gets over the byte ratio.  The launch without prox= runs the instruction stream of
the tree before the term existed (scripts/optim_isa_diff.py), so it is the baseline.

The loops re-read the same buffers (ResNet-18: 47 MB each, EnhancedCNN: 179 MB each); ``--flush``
streams a 512 MiB buffer before every timed iteration so that nothing is left in the 256 MiB
Infinity Cache.  lr is 0 and the gradient is rewritten by nobody, so the weights stay put; mu is 0.1
and the anchor differs from the weights, so the term is computed in full.

    python scripts/bench_fedprox.py [--model resnet18] [--iters 50] [--flush]
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

BYTES = {"sgd": 3 * 4 + 2 * 4 + 2, "adam": 4 * 4 + 3 * 4 + 2, "lion": 3 * 4 + 2 * 4 + 2}     # without the anchor
ANCHOR_BYTES = 4


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
    anchor = f.master + 0.01
    hp = torch.tensor([0.0, 1.0], device="cuda")      # lr 0: the weights stay put over the iterations
    prox = (anchor, torch.tensor([0.1, 0.0, 0.0, 0.0], device="cuda"))
    junk = torch.empty(128 << 20, device="cuda") if a.flush else None
    flush = (lambda: junk.add_(1.0)) if a.flush else None

    def sgd(p):
        return lambda: c.sgd_step(f.master, f.grad, mm, f.shadow, hp, 1.0, 0.9, 0.0, 0.0, False, False, prox=p)

    def adam(p):
        return lambda: c.adam_step(f.master, f.grad, mm, vv, f.shadow, hp, 1.0, 0.9, 0.999, 1e-8, 0.0, False, prox=p)

    def lion(p):
        return lambda: c.lion_step(f.master, f.grad, mm, f.shadow, hp, 1.0, 0.9, 0.99, 0.0, prox=p)

    us = lambda v: round(v * 1e6, 2)  # noqa: E731
    rec = {"model": a.model, "n": n, "flush": a.flush, "iters": a.iters, "buffer_MB": round(4 * n / 1e6, 1)}
    for name, make in (("sgd", sgd), ("adam", adam), ("lion", lion)):
        rows = {}
        for tag, p in (("plain", None), ("prox", prox), ("plain_again", None), ("prox_again", prox)):
            rows[tag] = timed(make(p), a.iters, before=flush)
            mm.zero_()
            vv.zero_()
        b = BYTES[name]
        r = {"B_per_elem": [b + ANCHOR_BYTES, b], "byte_ratio": round((b + ANCHOR_BYTES) / b, 3)}
        for tag, (med, (q1, q3)) in rows.items():
            r[tag + "_us"] = us(med)
            r[tag + "_iqr_us"] = [us(q1), us(q3)]
            r[tag + "_TBps"] = round((b + (ANCHOR_BYTES if tag.startswith("prox") else 0)) * n / med / 1e12, 3)
        r["ratio"] = round(rows["prox"][0] / rows["plain"][0], 3)
        r["ratio_again"] = round(rows["prox_again"][0] / rows["plain_again"][0], 3)
        # the baseline's own spread between its two rounds: the margin over the byte ratio
        r["plain_round_spread"] = round(abs(rows["plain_again"][0] / rows["plain"][0] - 1.0), 3)
        r["within_byte_ratio_plus_spread"] = bool(max(r["ratio"], r["ratio_again"])
                                                  <= r["byte_ratio"] + r["plain_round_spread"])
        rec[name] = r
    print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
