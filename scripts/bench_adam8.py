"""Cost of the Adam8bit kernel beside the fused Adam, same process, HIP events: adam8_step moves
18.25 B per element (w read and written, g read, bf16 shadow written, two code bytes read and written,
two fp32 scales per 64 elements read and written), adam_step 30 B.  The yardstick is bytes: 0.61x.
Sizes: EnhancedCNN's 44,595,786 parameters rounded up to 64, and the headline MLP
(784-4096-4096-10).  Timed alternately (adam8, adam, adam8 wide, adam again ...) so that a drift shows
up as a difference between the repeats; medians and quartiles over --iters launches each.  wide: the
eight-elements-per-lane form of the kernel (8 lanes per block) against four per lane (16 lanes per block).

    python scripts/bench_adam8.py [--iters 200] [--flush]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import ldnn  # noqa: E402,F401
from ldnn.ops._ext import C  # noqa: E402

ADAM8_BYTES = 2 * 4 + 4 + 2 + 4 + 4 * 4 / 64      # w, g, shadow, codes, scales
ADAM_BYTES = 4 * 4 + 3 * 4 + 2
SIZES = {"enhanced_cnn": (44595786 + 63) // 64 * 64,
         "mlp3": (784 * 4096 + 4096 + 4096 * 4096 + 4096 + 10 * 4096 + 10 + 63) // 64 * 64}


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
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--flush", action="store_true", help="stream 512 MiB before every timed iteration (cold cache)")
    a = ap.parse_args()
    c = C()
    junk = torch.empty(128 << 20, device="cuda") if a.flush else None
    flush = (lambda: junk.add_(1.0)) if a.flush else None
    for name, n in SIZES.items():
        gen = torch.Generator(device="cuda").manual_seed(0)
        w = torch.randn(n, device="cuda", generator=gen) * 0.05
        g = torch.randn(n, device="cuda", generator=gen) * 0.01
        sh = torch.zeros(n, dtype=torch.bfloat16, device="cuda")
        mm, vv = torch.zeros(n, device="cuda"), torch.zeros(n, device="cuda")
        mq, sq = (torch.zeros(n, dtype=torch.uint8, device="cuda") for _ in range(2))
        ms, ss = (torch.zeros(n // 64, device="cuda") for _ in range(2))
        hp = torch.tensor([0.0, 1.0], device="cuda")      # lr 0: the weights stay put over the iterations

        def adam8(wide=False):
            c.adam8_step(w, g, mq, sq, ms, ss, sh, hp, 1.0, 0.9, 0.999, 1e-8, 0.0, False, 0, 0, wide=wide)

        def adam():
            c.adam_step(w, g, mm, vv, sh, hp, 1.0, 0.9, 0.999, 1e-8, 0.0, False)

        rows = {}
        for key, fn in (("adam8", adam8), ("adam", adam), ("adam8_wide", lambda: adam8(True)), ("adam_again", adam),
                        ("adam8_again", adam8), ("adam8_wide_again", lambda: adam8(True))):
            rows[key] = timed(fn, a.iters, before=flush)
        us = lambda v: round(v * 1e6, 2)  # noqa: E731
        rec = {"buffer": name, "n": n, "flush": a.flush, "iters": a.iters, "adam8_B_per_elem": ADAM8_BYTES,
               "adam_B_per_elem": ADAM_BYTES, "par": round(ADAM8_BYTES / ADAM_BYTES, 3)}
        for key, (med, (q1, q3)) in rows.items():
            rec[key + "_us"] = us(med)
            rec[key + "_iqr_us"] = [us(q1), us(q3)]
            rec[key + "_TBps"] = round((ADAM_BYTES if key.startswith("adam_") or key == "adam" else ADAM8_BYTES)
                                       * n / med / 1e12, 3)
        rec["adam8_over_adam"] = round(rows["adam8"][0] / rows["adam"][0], 3)
        rec["adam8_again_over_adam_again"] = round(rows["adam8_again"][0] / rows["adam_again"][0], 3)
        rec["wide_over_adam8"] = round(rows["adam8_wide"][0] / rows["adam8"][0], 3)
        print(json.dumps(rec), flush=True)
        del w, g, sh, mm, vv, mq, sq, ms, ss


if __name__ == "__main__":
    main()
