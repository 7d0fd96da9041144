"""Instruction mix of the four-wave GEMM's main loop, per gemm_kernel instantiation.

    python scripts/gemm_q_loop_mix.py                 (compiles csrc/kernels/gemm_q.hip to assembly)
    python scripts/gemm_q_loop_mix.py gemm_q.s        (an assembly file made earlier, e.g. of another tree)
    python scripts/gemm_q_loop_mix.py --check [--parent old.s]   (exit status 1 when a loop misses its budget)
    python scripts/gemm_q_loop_mix.py --scratch-map   (also: which blocks of each kernel spill)

The main loop of a gemm_kernel is the basic block that holds one K-tile: 128
v_mfma_f32_16x16x32_bf16 per wave.  One line per instantiation: the block's instruction count,
split into MFMA / LDS reads / buffer loads (the LDS-DMA) / K-tail masks (v_cndmask) / other
vector ALU / scalar, wait and branch / anything else, then the kernel's NumVgprs and ScratchSize
and whether the loop block touches scratch.  Instantiations with the same layouts, output type
and counts are folded into one line (the epilogue does not reach into the loop).

Budgets of --check (one wave per SIMD: nothing hides a non-MFMA instruction between two MFMAs):
the all-k-contiguous loop is the yardstick, N_kc instructions with 32 ds_read_b128; a loop that
reads a k-strided operand needs two ds_read_b64_tr_b16 per fragment instead of one read.
  <true,true>    within 3 instructions of the same instantiation in --parent (not judged without)
  <false,false>  <= 300 instructions, <= 16 vector-ALU ops besides the K-tail masks
  mixed          <= 290 instructions, <= 16 vector-ALU ops besides the K-tail masks
"""
import argparse
import os
import re
import shutil
import subprocess
import sys
import tempfile
from collections import OrderedDict

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "learning-deep-neural-network-in-distributed-computing-environment_amd", "csrc")
ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")


def compile_asm(out):
    cmd = [os.path.join(ROCM, "bin", "hipcc"), "-O3", "-std=c++17", f"-I{os.path.join(CSRC, 'include')}",
           f"--offload-arch={os.environ.get('LDNN_OFFLOAD_ARCH', 'gfx950')}", "-munsafe-fp-atomics",
           "--cuda-device-only", "-S", os.path.join(CSRC, "kernels", "gemm_q.hip"), "-o", out]
    subprocess.run(cmd, check=True)


def demangle(names):
    tool = shutil.which("llvm-cxxfilt") or os.path.join(ROCM, "llvm", "bin", "llvm-cxxfilt")
    if not os.path.exists(tool):
        tool = shutil.which("c++filt")
    if not tool:
        return {n: n for n in names}
    out = subprocess.run([tool] + list(names), capture_output=True, text=True).stdout.splitlines()
    return dict(zip(names, out)) if len(out) == len(names) else {n: n for n in names}


def functions(path):
    """{mangled name: (blocks, info)}: blocks = [[instruction, ...], ...] split at local labels,
    info = the resource comments that follow the function (NumVgprs, ScratchSize, ...)."""
    out, name, blocks, last = OrderedDict(), None, None, None
    for ln in open(path):
        m = re.match(r"^(_Z\w+):", ln)
        if m and name is None:
            name, blocks = m.group(1), [[]]
            continue
        if name is None:
            m = re.match(r"^;\s*(\w+):\s*(\d+)\s*$", ln)
            if m and last is not None:
                out[last][1].setdefault(m.group(1), int(m.group(2)))
            continue
        if ln.startswith(".Lfunc_end"):
            out[name] = (blocks, {})
            name, last = None, name
            continue
        if re.match(r"^\.LBB\d+_\d+:", ln):
            blocks.append([])
            continue
        ln = ln.split(";", 1)[0].strip()
        if not ln or ln.startswith(".") or ln.endswith(":"):
            continue
        blocks[-1].append(ln)
    return out


CLASSES = ("mfma", "lds_read", "buf_load", "ktail_mask", "valu", "scalar", "other")


def tally(block):
    t = dict.fromkeys(CLASSES, 0)
    for ins in block:
        op = ins.split()[0]
        if op.startswith("v_mfma"):
            t["mfma"] += 1
        elif op.startswith(("ds_read", "ds_load")):
            t["lds_read"] += 1
        elif op.startswith("buffer_load"):
            t["buf_load"] += 1
        elif op.startswith("v_cndmask"):
            t["ktail_mask"] += 1
        elif op.startswith("v_"):
            t["valu"] += 1
        elif op.startswith("s_"):
            t["scalar"] += 1
        else:
            t["other"] += 1
    return t


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("asm", nargs="?", help="assembly of gemm_q.hip (default: compile the tree's)")
    ap.add_argument("--check", action="store_true")
    ap.add_argument("--parent", help="assembly of the tree to compare the <true,true> loops with")
    ap.add_argument("--scratch-map", action="store_true", help="list the blocks that access scratch")
    args = ap.parse_args()
    if args.asm:
        fns = functions(args.asm)
    else:
        with tempfile.TemporaryDirectory() as d:
            compile_asm(os.path.join(d, "gemm_q.s"))
            fns = functions(os.path.join(d, "gemm_q.s"))
    fns = OrderedDict((n, v) for n, v in fns.items() if "gemm_kernel" in n)
    parent = {}
    if args.parent:
        pf = OrderedDict((n, v) for n, v in functions(args.parent).items() if "gemm_kernel" in n)
        for n, full in demangle(list(pf)).items():
            m = re.search(r"gemm_kernel<(\w+), (\w+), (\d+), (\w+), (\d+)>", full)
            loops = [b for b in pf[n][0] if sum(i.startswith("v_mfma") for i in b) == 128]
            if m and loops:
                parent[m.groups()] = len(loops[-1])
    pretty = demangle(list(fns))
    rows, smap = OrderedDict(), OrderedDict()
    for n, (blocks, info) in fns.items():
        m = re.search(r"gemm_kernel<(\w+), (\w+), (\d+), (\w+), (\d+)>", pretty[n])
        if not m:
            print(f"cannot read the template arguments of {pretty[n]}", file=sys.stderr)
            return 2
        a_kc, b_kc, epi, f32, xf = m.groups()
        loops = [b for b in blocks if sum(i.startswith("v_mfma") for i in b) == 128]
        if xf != "0" and loops:
            loops = loops[-1:]   # an experiment build may peel its first K-tile: the steady-state block
        if len(loops) != 1:
            print(f"{pretty[n]}: {len(loops)} blocks with 128 MFMAs", file=sys.stderr)
            return 2
        t = tally(loops[0])
        scr = sum(i.startswith(("scratch_", "buffer_store")) or (i.startswith("buffer_load") and " lds" not in i)
                  for i in loops[0])
        was = parent.get((a_kc, b_kc, epi, f32, xf))
        key = (a_kc, b_kc, f32, xf, was, len(loops[0]), tuple(t.values()), info.get("NumVgprs"), info.get("ScratchSize"),
               scr)
        rows.setdefault(key, []).append(epi)
        if args.scratch_map and xf == "0":
            # where the spills live: blocks in program order, the loop block marked
            li = next(i for i, b in enumerate(blocks) if b is loops[0])
            part = {"before loop": [0, 0, 0], "LOOP": [0, 0, 0], "after loop": [0, 0, 0]}
            for i, b in enumerate(blocks):
                st = sum(x.startswith("scratch_store") for x in b)
                ld = sum(x.startswith("scratch_load") for x in b)
                c = part["before loop" if i < li else ("LOOP" if i == li else "after loop")]
                c[0] += st
                c[1] += ld
                c[2] += bool(st or ld)
            smap.setdefault((a_kc, b_kc, f32, info.get("ScratchSize"), tuple(tuple(c) for c in part.values())),
                            []).append(epi)
    for (a_kc, b_kc, f32, ss, parts), epis in smap.items():
        print(f"{a_kc + ',' + b_kc:<12} {f32:<6} EPI {','.join(epis):<18} ScratchSize {ss!s:>3}: "
              + "; ".join(f"{w} {st} stores / {ld} loads in {nb} blocks"
                          for w, (st, ld, nb) in zip(("before loop", "LOOP", "after loop"), parts)))
    if smap:
        print()
    print(f"{'A_KC,B_KC':<12} {'f32':<6} {'XF':>3} {'EPI':<16} {'instr':>5} " + " ".join(f"{c:>10}" for c in CLASSES)
          + f" {'NumVgprs':>8} {'Scratch':>7} {'loop scratch ops':>16}")
    bad = 0
    for (a_kc, b_kc, f32, xf, was, n, t, vg, ss, scr), epis in rows.items():
        t = dict(zip(CLASSES, t))
        verdict = ""
        if args.check and xf == "0":
            if a_kc == b_kc == "true":
                ok = was is None or abs(n - was) <= 3
            else:
                ok = n <= (300 if a_kc == b_kc == "false" else 290) and t["valu"] <= 16
            verdict = ("  ok" if ok else "  OVER BUDGET") + (f" (parent {was})" if was is not None else "")
            bad += not ok
        print(f"{a_kc + ',' + b_kc:<12} {f32:<6} {xf:>3} {','.join(epis):<16} {n:>5} "
              + " ".join(f"{t[c]:>10}" for c in CLASSES) + f" {vg!s:>8} {ss!s:>7} {scr:>16}{verdict}")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
