"""Cost of the dropout pass, same process, HIP events, medians of --iters: ``dropout_fwd`` and
``dropout_bwd`` on [16384, 4096] and [64, 1024] bf16 beside ``act_fwd`` / ``act_bwd`` (ReLU) on the same
buffers.  The yardstick is bytes: dropout moves 4 B per element each way (read x, write y; read g,
write dx) like ``act_fwd``; ``act_bwd`` reads y as well (6 B per element).

Each shape runs warm (the loops re-read the same buffers: 134 MB a piece for the large shape, inside
the 256 MiB Infinity Cache) and with ``--flush``-style cold caches: 512 MiB streamed before every
timed iteration.

    python scripts/bench_dropout.py [--iters 50] [--p 0.5]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import ldnn  # noqa: E402,F401
from ldnn.ops import functional as LF  # noqa: E402
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--p", type=float, default=0.5)
    a = ap.parse_args()
    c = C()
    junk = torch.empty(128 << 20, device="cuda")
    us = lambda v: round(v * 1e6, 2)  # noqa: E731
    for R, N in ((16384, 4096), (64, 1024)):
        x = torch.randn(R, N, device="cuda").bfloat16()
        g = torch.randn(R, N, device="cuda").bfloat16()
        y, dx = torch.empty_like(x), torch.empty_like(x)
        st = LF.DropoutState(x.device, 1, 0)
        st.set_rate(a.p)
        ticket = torch.zeros(8, dtype=torch.int32, device="cuda")
        fns = {"dropout_fwd": lambda: c.dropout_fwd(x, y, st.words, ticket),
               "dropout_bwd": lambda: c.dropout_bwd(g, dx, ticket),
               "relu_fwd": lambda: c.act_fwd(x.view(-1), y.view(-1), 0),
               "relu_bwd": lambda: c.act_bwd(g.view(-1), y.view(-1), dx.view(-1), 0)}
        for flush in (False, True):
            before = (lambda: junk.add_(1.0)) if flush else None
            rec = {"shape": [R, N], "p": a.p, "flush": flush, "MB_per_pass": round(4 * R * N / 1e6, 2)}
            rows = {}
            for name in ("relu_fwd", "dropout_fwd", "relu_bwd", "dropout_bwd", "relu_fwd_again"):
                rows[name] = timed(fns[name.replace("_again", "")], a.iters, before=before)
                rec[name + "_us"] = us(rows[name][0])
                rec[name + "_iqr_us"] = [us(v) for v in rows[name][1]]
            rec["dropout_fwd_TBps"] = round(4 * R * N / rows["dropout_fwd"][0] / 1e12, 3)
            rec["dropout_bwd_TBps"] = round(4 * R * N / rows["dropout_bwd"][0] / 1e12, 3)
            rec["relu_fwd_TBps"] = round(4 * R * N / rows["relu_fwd"][0] / 1e12, 3)
            rec["fwd_over_relu_fwd"] = round(rows["dropout_fwd"][0] / rows["relu_fwd"][0], 3)
            rec["bwd_over_relu_bwd"] = round(rows["dropout_bwd"][0] / rows["relu_bwd"][0], 3)
            rec["bwd_over_relu_fwd"] = round(rows["dropout_bwd"][0] / rows["relu_fwd"][0], 3)
            print(json.dumps(rec), flush=True)
        assert st.read()["counter"] == 2 * (a.iters + 10)      # (every forward launch advanced the counter once)


if __name__ == "__main__":
    main()
