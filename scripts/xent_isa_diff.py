"""Are the unsmoothed softmax-xent kernels still the instruction streams they were?

    hipcc -O3 -std=c++17 -I<pkg>/csrc/include --offload-arch=gfx950 -munsafe-fp-atomics \
          --cuda-device-only -S <pkg>/csrc/kernels/xent.hip -o new.s      (same on the older tree: old.s)
    python scripts/xent_isa_diff.py old.s new.s

Pairs every plain xent kernel of old.s with the plain instance of new.s that has the same leading
template arguments (the mode is a trailing `bool SMOOTH` in older trees, an `int MODE` -- 0 plain,
1 smoothed, 2 soft targets, 3 weighted labels, 4 weighted soft targets -- since the soft-target
instances; the instances of modes 1 to 4 are paired too where old.s has them, any other mode of
new.s, such as 5, focal, is ignored), and compares their instruction streams: comments dropped, the
function number of local labels (.LBB<fn>_<n>) and the kernels' own symbol names normalised.
Two scalar loads that differ only in their constant offset are counted apart: appended kernel
arguments move the hidden ones (block / grid size) behind them in the kernel-argument segment.
Prints one line per kernel; exit status 1 when a pair differs in anything else.
"""
import re
import sys


def kernels(path):
    """{mangled name: [instruction lines]} for every kernel function of an assembly file."""
    out, name, body = {}, None, None
    for ln in open(path):
        m = re.match(r"^(_Z\w+):", ln)
        if m and name is None:
            name, body = m.group(1), []
            continue
        if name is None:
            continue
        if ln.startswith(".Lfunc_end"):
            out[name] = body
            name = None
            continue
        ln = ln.split(";", 1)[0].strip()
        if not ln or (ln.startswith(".") and not ln.startswith(".LBB")):
            continue   # directives
        ln = re.sub(r"\.LBB\d+_", ".LBB_", ln)
        ln = re.sub(r"_Z\w+", "SYM", ln)
        body.append(ln)
    return out


def key(name):
    """('rows', LD) / ('wave',) / None, and the mode: 0 plain, 1 smoothed, 2 soft targets (None: a
    tree with plain kernels only)."""
    m = re.search(r"xent_rows_kernelILi(\d+)(?:ELb([01])|ELi(\d+))?EE", name)
    if m:
        return ("rows", int(m.group(1))), (None if m.group(2) is None and m.group(3) is None
                                           else int(m.group(2) or m.group(3)))
    m = re.search(r"\d+xent_kernel(?:ILb([01])EE|ILi(\d+)EE)?", name)
    if m:
        return ("wave",), (None if m.group(1) is None and m.group(2) is None else int(m.group(1) or m.group(2)))
    return None, None


_SLOAD = re.compile(r"^(s_load_dword\w* s\S+ s\[\d+:\d+\],) 0x[0-9a-f]+$")


def offset_only(x, y):
    a, b = _SLOAD.match(x), _SLOAD.match(y)
    return bool(a and b and a.group(1) == b.group(1))


def main():
    old, new = kernels(sys.argv[1]), kernels(sys.argv[2])
    def by_mode(ks, modes):
        return {key(n)[0]: b for n, b in ks.items() if key(n)[0] is not None and key(n)[1] in modes}

    plain, smooth, soft = by_mode(new, (None, 0)), by_mode(new, (1,)), by_mode(new, (2,))
    bad = 0
    bad += compare(by_mode(old, (None, 0)), plain, smooth, soft, "SMOOTH=false")
    if by_mode(old, (1,)):
        bad += compare(by_mode(old, (1,)), smooth, {}, {}, "SMOOTH=true")
    # the later modes, each against its own instance where old.s has it; a mode that is not in this
    # table (5, focal, has no counterpart in a tree before it) is left out of the comparison
    for mode, what in LATER_MODES.items():
        if by_mode(old, (mode,)):
            bad += compare(by_mode(old, (mode,)), by_mode(new, (mode,)), {}, {}, what)
    return 1 if bad else 0


LATER_MODES = {2: "soft", 3: "weighted", 4: "weighted_soft"}


def compare(olds, plain, smooth, soft, what):
    bad = 0
    for k in sorted(olds):
        a, b = olds[k], plain.get(k)
        tag = "_".join(str(v) for v in k) + {"SMOOTH=false": "", "SMOOTH=true": "_smooth"}.get(what, "_" + what)
        if b is None:
            print(f"{tag}: missing from {sys.argv[2]}")
            bad += 1
            continue
        pairs = [(x, y) for x, y in zip(a, b) if x != y]
        offs = sum(offset_only(x, y) for x, y in pairs)
        diff = len(pairs) - offs + abs(len(a) - len(b))
        bad += diff != 0
        s = smooth.get(k)
        t = soft.get(k)
        print(f"{tag}: old {len(a)} instructions, new {what} {len(b)}, kernel-argument offsets moved in "
              f"{offs}, otherwise differing {diff}: {'IDENTICAL' if diff == 0 else 'DIFFERENT'}"
              + (f"; SMOOTH=true {len(s)} instructions ({len(s) - len(b):+d})" if s is not None else "")
              + (f"; soft targets {len(t)} instructions ({len(t) - len(b):+d})" if t is not None else ""))
    return bad


if __name__ == "__main__":
    sys.exit(main())
