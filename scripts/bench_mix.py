"""The batch-mix pass (mix.hip: Mixup / CutMix + the soft targets, one launch) against the torch
composite that does the same in the same process -- index_select + mul + add for Mixup, index_select
+ torch.where for CutMix, each plus the two scatter writes of the targets -- alternated sample by
sample, and the pass's store policy (plain / nontemporal stores of the mixed batch) likewise.

    python scripts/bench_mix.py [--out profiles/r13/mix_ab.jsonl]

One sample = `--inner` back-to-back calls between two HIP events, reported per call; medians of
`--samples`.  Effective bandwidth counts the bytes the definition moves: Mixup reads the batch twice
and writes it once; CutMix reads it once and writes it once (a quarter-image box).
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import ldnn  # noqa: E402,F401
from ldnn.data.mix import MODE_CUTMIX, MODE_MIXUP, MixPlan, ldq_for, mix_native  # noqa: E402

CASES = [((64, 3, 32, 32), torch.bfloat16, 10), ((256, 3, 224, 224), torch.float32, 1000),
         ((256, 3, 224, 224), torch.bfloat16, 1000)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=50)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--out", default=None, help="append the JSON lines to this file too")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_mix needs a GPU")
    recs = []
    for shape, dtype, classes in CASES:
        B, _, H, W = shape
        g = torch.Generator(device="cuda").manual_seed(0)
        x = torch.randn(shape, device="cuda", generator=g).to(dtype)
        y = torch.randint(0, classes, (B,), device="cuda", generator=g)
        perm_np = np.random.default_rng(0).permutation(B).astype(np.int64)
        perm = torch.as_tensor(perm_np, device="cuda")
        rows = torch.arange(B, device="cuda")
        mask = torch.zeros(1, 1, H, W, dtype=torch.bool, device="cuda")
        box = (H // 4, H // 4 + H // 2, W // 4, W // 4 + W // 2)   # a quarter of the image
        mask[..., box[0]:box[1], box[2]:box[3]] = True
        for mode in (MODE_MIXUP, MODE_CUTMIX):
            lam = 0.37 if mode == MODE_MIXUP else 0.75
            plan = MixPlan(mode, lam, perm_np, box if mode == MODE_CUTMIX else (0, 0, 0, 0))

            def composite():
                xp = x.index_select(0, perm)
                out = torch.where(mask, xp, x) if mode == MODE_CUTMIX else x * lam + xp * (1.0 - lam)
                q = torch.zeros(B, ldq_for(classes), device="cuda")
                q[rows, y] += lam
                q[rows, y.index_select(0, perm)] += 1.0 - lam
                return out, q

            variants = {"composite": composite, "plain": lambda: mix_native(x, y, perm, plan, classes)}

            def sample(fn):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(a.inner):
                    fn()
                e1.record()
                e1.synchronize()
                return e0.elapsed_time(e1) * 1e3 / a.inner   # us per call

            names = list(variants)
            for n in names:
                for _ in range(3):
                    sample(variants[n])
            t = {n: [] for n in names}
            for i in range(a.samples):
                for n in (names if i % 2 == 0 else names[::-1]):   # alternate the order
                    t[n].append(sample(variants[n]))

            def qt(v, f):
                return round(sorted(v)[min(len(v) - 1, int(f * len(v)))], 3)

            nbytes = x.numel() * x.element_size() * (3 if mode == MODE_MIXUP else 2)
            rec = {"bench": "mix_ab", "shape": list(shape), "dtype": str(dtype).split(".")[-1], "classes": classes,
                   "mode": mode, "lam": lam, "samples": a.samples, "inner": a.inner, "bytes": nbytes}
            for n in names:
                rec.update({f"{n}_us": qt(t[n], 0.5), f"{n}_p10_us": qt(t[n], 0.1), f"{n}_p90_us": qt(t[n], 0.9),
                            f"{n}_TBps": round(nbytes / qt(t[n], 0.5) / 1e6, 3)})
            rec["plain_over_composite"] = round(rec["plain_us"] / rec["composite_us"], 4)
            recs.append(rec)
            print(json.dumps(rec), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            for r in recs:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
