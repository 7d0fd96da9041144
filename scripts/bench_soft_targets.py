"""Cost of class-probability targets in the fused softmax cross-entropy kernel: the soft-target
instance against the plain (hard-label) one in the same process, alternated sample by sample.
The soft instance reads 4 * B * C more bytes (the fp32 targets); both are reported with their
bytes (logits read + gradient written [+ targets read]).

    python scripts/bench_soft_targets.py [--out profiles/r13/soft_targets_ab.jsonl]

One sample = `--inner` back-to-back launches between two HIP events, reported per launch; medians
of `--samples`.  The call is the one the autograd loss makes: loss_out + stats, no dbias,
grad_scale = 1/B.  The targets are two-hot rows in a [B, up4(C)] buffer, as the mix pass writes.
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
        raise SystemExit("bench_soft_targets needs a GPU")
    C = _ext.C()
    recs = []
    for B, Cc, ld in SHAPES:
        g = torch.Generator(device="cuda").manual_seed(0)
        logits = (torch.randn(B, ld, device="cuda", generator=g) * 3).bfloat16()[:, :Cc]
        labels = torch.randint(0, Cc, (B,), device="cuda", generator=g)
        ldq = (Cc + 3) // 4 * 4
        qbuf = torch.zeros(B, ldq, device="cuda")
        rows = torch.arange(B, device="cuda")
        qbuf[rows, labels] += 0.7
        qbuf[rows, labels.flip(0)] += 0.3
        q = qbuf[:, :Cc]
        dl = torch.empty(B, ld, device="cuda", dtype=torch.bfloat16)
        stats = torch.zeros(2, device="cuda")
        out = torch.empty(2, device="cuda")

        def launch(soft):
            if soft:
                C.softmax_xent_soft(logits, q, dl[:, :Cc], stats, None, Cc, 1.0 / B, loss_out=out,
                                    loss_scale=1.0 / B, label_smoothing=a.eps)
            else:
                C.softmax_xent(logits, labels, dl[:, :Cc], stats, None, Cc, 1.0 / B, loss_out=out,
                               loss_scale=1.0 / B)

        def sample(soft):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.inner):
                launch(soft)
            e1.record()
            e1.synchronize()
            return e0.elapsed_time(e1) * 1e3 / a.inner   # us per launch

        for soft in (False, True):   # warm both instances
            for _ in range(3):
                sample(soft)
        t = {False: [], True: []}
        for i in range(a.samples):
            for soft in ((False, True) if i % 2 == 0 else (True, False)):
                t[soft].append(sample(soft))

        def qt(v, f):
            return round(sorted(v)[min(len(v) - 1, int(f * len(v)))], 3)

        p, s = t[False], t[True]
        plain_bytes = B * Cc * 2 + B * ld * 2 + B * 8
        soft_bytes = B * Cc * 2 + B * ld * 2 + B * Cc * 4
        recs.append({"bench": "soft_targets_ab", "B": B, "C": Cc, "ld": ld, "ldq": ldq,
                     "kernel": "rows" if ld <= 64 else "wave", "eps": a.eps, "samples": a.samples, "inner": a.inner,
                     "plain_us": qt(p, 0.5), "plain_p10_us": qt(p, 0.1), "plain_p90_us": qt(p, 0.9),
                     "soft_us": qt(s, 0.5), "soft_p10_us": qt(s, 0.1), "soft_p90_us": qt(s, 0.9),
                     "plain_bytes": plain_bytes, "soft_bytes": soft_bytes,
                     "bytes_ratio": round(soft_bytes / plain_bytes, 3),
                     "soft_over_plain": round(qt(s, 0.5) / qt(p, 0.5), 4)})
        print(json.dumps(recs[-1]), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            for r in recs:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
