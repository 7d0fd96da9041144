"""Cost of label smoothing inside the fused softmax cross-entropy kernel: the SMOOTH instance
against the unsmoothed one in the same process, alternated sample by sample (both move the same
bytes; the smoothed one adds a row sum -- one wave reduction per row in the wave kernel).

    python scripts/bench_label_smoothing.py [--out profiles/r11/label_smoothing_ab.jsonl]

One sample = `--inner` back-to-back launches between two HIP events (a single launch of a few
microseconds is below what an event pair resolves), reported per launch; medians of `--samples`.
The call is the one the autograd loss makes: loss_out + stats, no dbias, grad_scale = 1/B.
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import ldnn  # noqa: E402,F401
from ldnn.ops import _ext  # noqa: E402

SHAPES = [(64, 10, 16), (256, 1000, 1000), (16384, 10, 16)]   # (B, C, ld): rows, wave, rows at many blocks


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=50)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--eps", type=float, default=0.1)
    ap.add_argument("--out", default=None, help="append the JSON lines to this file too")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_label_smoothing needs a GPU")
    C = _ext.C()
    recs = []
    for B, Cc, ld in SHAPES:
        g = torch.Generator(device="cuda").manual_seed(0)
        logits = (torch.randn(B, ld, device="cuda", generator=g) * 3).bfloat16()[:, :Cc]
        labels = torch.randint(0, Cc, (B,), device="cuda", generator=g)
        dl = torch.empty(B, ld, device="cuda", dtype=torch.bfloat16)
        stats = torch.zeros(2, device="cuda")
        out = torch.empty(2, device="cuda")

        def launch(eps):
            C.softmax_xent(logits, labels, dl[:, :Cc], stats, None, Cc, 1.0 / B, loss_out=out, loss_scale=1.0 / B,
                           label_smoothing=eps)

        def sample(eps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.inner):
                launch(eps)
            e1.record()
            e1.synchronize()
            return e0.elapsed_time(e1) * 1e3 / a.inner   # us per launch

        for eps in (0.0, a.eps):   # warm both instances
            for _ in range(3):
                sample(eps)
        t = {0.0: [], a.eps: []}
        for i in range(a.samples):
            for eps in ((0.0, a.eps) if i % 2 == 0 else (a.eps, 0.0)):
                t[eps].append(sample(eps))

        def q(v, f):
            return round(sorted(v)[min(len(v) - 1, int(f * len(v)))], 3)

        p, s = t[0.0], t[a.eps]
        recs.append({"bench": "label_smoothing_ab", "B": B, "C": Cc, "ld": ld, "kernel": "rows" if ld <= 64 else "wave",
                     "eps": a.eps, "samples": a.samples, "inner": a.inner,
                     "plain_us": q(p, 0.5), "plain_p10_us": q(p, 0.1), "plain_p90_us": q(p, 0.9),
                     "smooth_us": q(s, 0.5), "smooth_p10_us": q(s, 0.1), "smooth_p90_us": q(s, 0.9),
                     "smooth_over_plain": round(q(s, 0.5) / q(p, 0.5), 4)})
        print(json.dumps(recs[-1]), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            for r in recs:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
