"""Cost of class weights / ignore_index in the fused softmax cross-entropy: the weighted op (the
one-workgroup denominator pre-pass + the weighted kernel instance) against the unweighted launch in
the same process, alternated sample by sample.

    python scripts/bench_class_weights.py [--out profiles/r20/class_weights_ab.jsonl]

One sample = `--inner` back-to-back calls between two HIP events, reported per call; medians of
`--samples`.  The call is the one the autograd loss makes: loss_out + stats, no dbias.  A tenth of
the rows carry the ignored label.
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import ldnn  # noqa: E402,F401
from ldnn.ops import _ext  # noqa: E402

SHAPES = [(4096, 10, 16), (64, 1000, 1000)]   # (B, C, ld): rows kernel, wave kernel


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=50)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--eps", type=float, default=0.0)
    ap.add_argument("--out", default=None, help="append the JSON lines to this file too")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_class_weights needs a GPU")
    C = _ext.C()
    recs = []
    for B, Cc, ld in SHAPES:
        g = torch.Generator(device="cuda").manual_seed(0)
        logits = (torch.randn(B, ld, device="cuda", generator=g) * 3).bfloat16()[:, :Cc]
        labels = torch.randint(0, Cc, (B,), device="cuda", generator=g)
        ignored = labels.clone()
        ignored[::10] = -100
        w = torch.rand(Cc, device="cuda", generator=g) * 3
        dl = torch.empty(B, ld, device="cuda", dtype=torch.bfloat16)
        stats = torch.zeros(2, device="cuda")
        out = torch.empty(2, device="cuda")

        def launch(weighted):
            if weighted:
                C.softmax_xent_w(logits, ignored, dl[:, :Cc], stats, None, Cc, loss_out=out, label_smoothing=a.eps,
                                 weight=w, ignore_index=-100)
            else:
                C.softmax_xent(logits, labels, dl[:, :Cc], stats, None, Cc, 1.0 / B, loss_out=out,
                               loss_scale=1.0 / B, label_smoothing=a.eps)

        def sample(weighted):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.inner):
                launch(weighted)
            e1.record()
            e1.synchronize()
            return e0.elapsed_time(e1) * 1e3 / a.inner   # us per call

        for weighted in (False, True):   # warm both
            for _ in range(3):
                sample(weighted)
        t = {False: [], True: []}
        for i in range(a.samples):
            for weighted in ((False, True) if i % 2 == 0 else (True, False)):
                t[weighted].append(sample(weighted))

        def qt(v, f):
            return round(sorted(v)[min(len(v) - 1, int(f * len(v)))], 3)

        p, s = t[False], t[True]
        recs.append({"bench": "class_weights_ab", "B": B, "C": Cc, "ld": ld,
                     "kernel": "rows" if ld <= 64 else "wave", "eps": a.eps, "samples": a.samples, "inner": a.inner,
                     "plain_us": qt(p, 0.5), "plain_p10_us": qt(p, 0.1), "plain_p90_us": qt(p, 0.9),
                     "weighted_us": qt(s, 0.5), "weighted_p10_us": qt(s, 0.1), "weighted_p90_us": qt(s, 0.9),
                     "plain_launches": 1, "weighted_launches": 2,
                     "weighted_over_plain": round(qt(s, 0.5) / qt(p, 0.5), 4)})
        print(json.dumps(recs[-1]), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            for r in recs:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
