#!/usr/bin/env python
"""How far gemm_mx8's block-scaled MFMA accumulation is from an fp32 one: gemm_mx8 (fp32 out, M = N = 128) against
fp64 on operands quantised on the CPU, over seeded cases: both A formats, K = 8 .. 2048, four operand
distributions (N(0,1), its cube, `spread` = N(0,1) with every 32-block times a random power of two in 2^-8 .. 2^8,
`one_block` = spread with each row of A non-zero in one block only).  Per (format, K, distribution) one JSON line
with the worst (err - 2^-23 |r|) over K_pad 2^-23 (|A| @ |B|^T), the bound of an fp32 accumulation, and over
|A| @ |B|^T itself; the last line is the overall worst.  tests/test_mxfp8_gpu.py takes its constant from it.

    python scripts/accum_mx8.py [--seeds 4] [--out profiles/r26]
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import ldnn  # noqa: E402,F401
from ldnn.ops import _ext  # noqa: E402
from ldnn.ops import functional as LF  # noqa: E402

M = N = 128


def operand(rows, K, dist):
    t = torch.randn(rows, K)
    if dist == "cube":
        t = t ** 3
    elif dist in ("spread", "one_block"):
        t = torch.ldexp(t, torch.randint(-8, 9, (rows, (K + 31) // 32)).repeat_interleave(32, 1)[:, :K])
    return t.bfloat16()


def case(fmt, K, dist, seed):
    torch.manual_seed(seed)
    a, b = operand(M, K, dist), operand(N, K, dist)
    if dist == "one_block":
        nb = (K + 127) // 128 * 4
        a = torch.where((torch.arange(K) // 32)[None, :] == (torch.arange(M) % nb)[:, None], a, torch.zeros_like(a))
    a8, as_ = LF._mx8_padded(a, fmt)
    b8, bs = LF._mx8_padded(b, "e4m3")
    A = LF._mx8_dequant(a8[:M], 127 - as_[:M].int(), fmt).double()
    B = LF._mx8_dequant(b8[:N], 127 - bs[:N].int(), "e4m3").double()
    out = torch.empty(M, N, device="cuda")
    C = _ext.C()
    C.gemm_mx8(a8.cuda(), as_.cuda(), b8.cuda(), bs.cuda(), out, LF.FP8_FORMATS[fmt][0], C.EPI_NONE)
    r, ab = A @ B.t(), A.abs() @ B.abs().t()
    err = ((out.cpu().double() - r).abs() - 2.0 ** -23 * r.abs()).clamp_min(0)
    ok = ab > 0
    return (err[ok] / (a8.shape[1] * 2.0 ** -23 * ab[ok])).max().item(), (err[ok] / ab[ok]).max().item()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--seeds", type=int, default=4)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r26"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "accum_mx8.py measures on the GPU"
    os.makedirs(a.out, exist_ok=True)
    worst, n = (0.0, None), 0
    with open(os.path.join(a.out, "accum_vs_fp64.jsonl"), "w") as f:
        for fmt in ("e4m3", "e5m2"):
            for K in (8, 16, 32, 64, 128, 256, 512, 1024, 2048):
                for dist in ("randn", "cube", "spread", "one_block"):
                    rs = [case(fmt, K, dist, s) for s in range(a.seeds)]
                    n += len(rs)
                    rec = {"fmt": fmt, "K": K, "dist": dist, "cases": len(rs),
                           "worst_over_fp32_bound": round(max(r[0] for r in rs), 3),
                           "worst_over_absprod": float(f"{max(r[1] for r in rs):.3g}")}
                    f.write(json.dumps(rec) + "\n")
                    if rec["worst_over_fp32_bound"] > worst[0]:
                        worst = (rec["worst_over_fp32_bound"], rec)
        last = {"cases": n, "worst_over_fp32_bound": worst[0], "at": worst[1]}
        f.write(json.dumps(last) + "\n")
    print(json.dumps(last))
