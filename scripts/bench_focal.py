"""Cost of the focal loss in the fused softmax cross-entropy: the focal pair of launches (the
one-workgroup denominator pre-pass + the focal kernel instance) against the weighted pair of the
same build, in the same process, alternated sample by sample.  Both pairs move the same bytes; the
focal instance adds a few transcendental ops per row.

    python scripts/bench_focal.py [--gamma 2] [--out profiles/r21/focal_ab.jsonl]

One sample = `--inner` back-to-back calls between two HIP events, reported per call; medians of
`--samples`, with the 10th / 90th percentiles as the run-to-run spread.  The call is the one the
autograd loss makes: loss_out + stats, no dbias.  A tenth of the rows carry the ignored label.
`focal_minus_weighted_us` is to be read against `spread_us`, the wider of the two variants'
p10..p90 ranges.
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import ldnn  # noqa: E402,F401
from ldnn.ops import _ext  # noqa: E402

SHAPES = [(4096, 10, 16), (256, 1000, 1000)]   # (B, C, ld): rows kernel, wave kernel


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=50)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--gamma", type=float, default=2.0)
    ap.add_argument("--out", default=None, help="append the JSON lines to this file too")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_focal needs a GPU")
    if not a.gamma > 0:
        raise SystemExit("--gamma must be > 0 (0 is the weighted pair itself)")
    C = _ext.C()
    recs = []
    for B, Cc, ld in SHAPES:
        g = torch.Generator(device="cuda").manual_seed(0)
        logits = (torch.randn(B, ld, device="cuda", generator=g) * 3).bfloat16()[:, :Cc]
        labels = torch.randint(0, Cc, (B,), device="cuda", generator=g)
        labels[::10] = -100
        w = torch.rand(Cc, device="cuda", generator=g) * 3
        dl = torch.empty(B, ld, device="cuda", dtype=torch.bfloat16)
        stats = torch.zeros(2, device="cuda")
        out = torch.empty(2, device="cuda")

        def launch(focal):
            if focal:
                C.softmax_xent_focal(logits, labels, dl[:, :Cc], stats, None, Cc, gamma=a.gamma, weight=w,
                                     ignore_index=-100, loss_out=out)
            else:
                C.softmax_xent_w(logits, labels, dl[:, :Cc], stats, None, Cc, loss_out=out, weight=w,
                                 ignore_index=-100)

        def sample(focal):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.inner):
                launch(focal)
            e1.record()
            e1.synchronize()
            return e0.elapsed_time(e1) * 1e3 / a.inner   # us per call

        for focal in (False, True):   # warm both
            for _ in range(3):
                sample(focal)
        t = {False: [], True: []}
        for i in range(a.samples):
            for focal in ((False, True) if i % 2 == 0 else (True, False)):
                t[focal].append(sample(focal))

        def qt(v, f):
            return round(sorted(v)[min(len(v) - 1, int(f * len(v)))], 3)

        p, s = t[False], t[True]
        spread = max(qt(p, 0.9) - qt(p, 0.1), qt(s, 0.9) - qt(s, 0.1))
        recs.append({"bench": "focal_ab", "B": B, "C": Cc, "ld": ld, "kernel": "rows" if ld <= 64 else "wave",
                     "gamma": a.gamma, "samples": a.samples, "inner": a.inner,
                     "weighted_us": qt(p, 0.5), "weighted_p10_us": qt(p, 0.1), "weighted_p90_us": qt(p, 0.9),
                     "focal_us": qt(s, 0.5), "focal_p10_us": qt(s, 0.1), "focal_p90_us": qt(s, 0.9),
                     "launches": 2, "focal_minus_weighted_us": round(qt(s, 0.5) - qt(p, 0.5), 3),
                     "spread_us": round(spread, 3), "focal_over_weighted": round(qt(s, 0.5) / qt(p, 0.5), 4)})
        print(json.dumps(recs[-1]), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            for r in recs:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
