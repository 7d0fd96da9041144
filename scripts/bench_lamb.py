"""Cost of the LAMB kernels on a model's real flat buffers, same process, HIP events: the fused
Adam alone (30 B per element), lamb_moments (24 B: read w, g, m, v; write m, v) under its three
access policies (gradient loads nontemporal = what the step uses, everything plain, everything
nontemporal), lamb_finalize, lamb_apply (18 B: read w, m, v; write w, shadow) and the whole LAMB
step (bump + moments + finalize + apply, 42 B).  The yardstick is bytes: the step should cost
about 42 / 30 = 1.4x the Adam's time.

The loops re-read the same buffers (ResNet-18: 47 MB each, EnhancedCNN: 179 MB each); ``--flush``
streams a 512 MiB buffer before every timed iteration so that nothing is left in the 256 MiB
Infinity Cache.  lr is 0 and the gradient is rewritten by nobody, so the weights stay put.

    python scripts/bench_lamb.py [--model resnet18] [--iters 50] [--flush]
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
from ldnn.optim.optimizers import _Lamb  # noqa: E402


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
    M = _Lamb(f, None, True, f.master.device)
    t = M.table([(0, n)], False, [(0, n)])
    offs = M.offsets
    junk = torch.empty(128 << 20, device="cuda") if a.flush else None
    flush = (lambda: junk.add_(1.0)) if a.flush else None
    B1, B2, EPS, WD = 0.9, 0.999, 1e-6, 1e-2

    def adam():
        c.adam_step(f.master, f.grad, mm, vv, f.shadow, hp, 1.0, B1, B2, 1e-8, 0.0, False)

    def moments(policy=1):
        c.lamb_moments(f.master, f.grad, mm, vv, t["chunks"], t["partials"], hp, 1.0, B1, B2, EPS, WD, t["ranges"], offs,
                       policy=policy)

    def finalize():
        c.lamb_finalize(t["partials"], t["segtab"], M.ratio, M.w_norm, M.g_norm)

    def apply():
        c.lamb_apply(f.master, f.grad, mm, vv, f.shadow, hp, B1, B2, EPS, WD, M.ratio, M.segmap)

    def step(policy=1):
        c.bump_step(hp)
        moments(policy)
        finalize()
        apply()

    rows = {}
    for name, fn in (("adam", adam), ("moments_nt_grad", moments), ("moments_all_plain", lambda: moments(0)),
                     ("moments_all_nt", lambda: moments(2)),
                     ("finalize", finalize), ("apply", apply), ("lamb_step", step), ("lamb_step_all_plain", lambda: step(0)),
                     ("lamb_step_all_nt", lambda: step(2)), ("adam_again", adam)):
        hp[1] = 1.0
        rows[name] = timed(fn, a.iters, before=flush)
    us = lambda v: round(v * 1e6, 2)  # noqa: E731
    rec = {"model": a.model, "n": n, "segments": M.S, "chunks": int(t["chunks"].shape[0]), "flush": a.flush,
           "buffer_MB": round(4 * n / 1e6, 1)}
    for name, (med, (q1, q3)) in rows.items():
        rec[name + "_us"] = us(med)
        rec[name + "_iqr_us"] = [us(q1), us(q3)]
    rec["adam_TBps"] = round(30 * n / rows["adam"][0] / 1e12, 3)
    rec["moments_TBps"] = round(24 * n / rows["moments_nt_grad"][0] / 1e12, 3)
    rec["apply_TBps"] = round(18 * n / rows["apply"][0] / 1e12, 3)
    rec["lamb_step_TBps"] = round(42 * n / rows["lamb_step"][0] / 1e12, 3)
    rec["lamb_over_adam"] = round(rows["lamb_step"][0] / rows["adam"][0], 3)
    print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
