"""Are the optimizer kernels without the proximal term still the instruction streams they were?

    hipcc -O3 -fPIC -std=c++17 -I<pkg>/csrc/include --offload-arch=gfx950 -munsafe-fp-atomics \
          --cuda-device-only -S <pkg>/csrc/kernels/optim.hip -o new.s      (same on the older tree: old.s)
    python scripts/optim_isa_diff.py old.s new.s

Pairs every kernel of old.s with the kernel of new.s that has the same function name and the same
template arguments; sgd_kernel, adam_kernel and lion_kernel gained a trailing `bool PROX`, so their old
instances pair with the new PROX = false ones.  Compares the instruction streams: comments and
directives dropped, the function number of local labels (.LBB<fn>_<n>) and the kernels' own symbol
names normalised.  Scalar loads from the kernel-argument segment, and the s_add_u32 that forms the
address of the hidden arguments, that differ only in their constant offset are counted apart: an
appended (empty) argument behind a pointer moves the hidden ones (block / grid size) by 8 bytes.
Anything else is a difference.
Prints one line per pair, then the register and scratch figures of the kernels only new.s has; exit
status 1 when a pair differs or a kernel of old.s is missing.
"""
import re
import sys

GAINED_PROX = ("sgd_kernel", "adam_kernel", "lion_kernel")
_NAME = re.compile(r"^_ZN4ldnn12_GLOBAL__N_1\d+([a-z0-9_]+?_kernel)(?:I((?:L[bi]\d+E)+)E)?")
_SLOAD = re.compile(r"^(s_load_dword\w* s\S+ s\[\d+:\d+\],|s_add_u32 (s\d+), \2,) 0x[0-9a-f]+$")
_FIGURES = ("NumVgprs", "NumAgprs", "TotalNumSgprs", "ScratchSize", "LDSByteSize", "Occupancy")


def kernels(path):
    """{mangled name: ([instruction lines], {figure: value})} for every kernel of an assembly file."""
    out, name, body, figs = {}, None, None, None
    for ln in open(path):
        m = re.match(r"^(_Z\w+):", ln)
        if m and name is None:
            name, body, figs = m.group(1), [], None
            continue
        if name is None:
            continue
        if ln.startswith(".Lfunc_end"):
            figs = {}
            continue
        if figs is not None:     # the resource comments behind the function's end
            m = re.match(r"^; (\w+): (\d+)", ln)
            if m and m.group(1) in _FIGURES:
                figs[m.group(1)] = int(m.group(2))
            if "Occupancy" in figs or ln.startswith("\t.text") or re.match(r"^_Z\w+:", ln):
                out[name] = (body, figs)
                name = None
            continue
        ln = ln.split(";", 1)[0].strip()
        if not ln or (ln.startswith(".") and not ln.startswith(".LBB")):
            continue   # directives
        ln = re.sub(r"\.LBB\d+_", ".LBB_", ln)
        ln = re.sub(r"_Z\w+", "SYM", ln)
        body.append(ln)
    return out


def key(name, old):
    """(function, template arguments); the instances of old.s that gained PROX get its `false`."""
    m = _NAME.match(name)
    if m is None:
        return None
    args = tuple(int(a) for a in re.findall(r"L[bi](\d+)E", m.group(2) or ""))
    if old and m.group(1) in GAINED_PROX:
        args += (0,)
    return m.group(1), args


def label(k):
    return k[0] + ("<" + ", ".join(str(a) for a in k[1]) + ">" if k[1] else "")


def main():
    old = {key(n, True): v for n, v in kernels(sys.argv[1]).items() if key(n, True)}
    new = {key(n, False): v for n, v in kernels(sys.argv[2]).items() if key(n, False)}
    bad = 0
    for k in sorted(old):
        a, fa = old[k]
        if k not in new:
            print(f"{label(k)}: missing from {sys.argv[2]}")
            bad += 1
            continue
        b, fb = new[k]
        pairs = [(x, y) for x, y in zip(a, b) if x != y]
        offs = sum(bool(_SLOAD.match(x) and _SLOAD.match(y) and _SLOAD.match(x).group(1) == _SLOAD.match(y).group(1))
                   for x, y in pairs)
        diff = len(pairs) - offs + abs(len(a) - len(b))
        bad += diff != 0 or fa != fb
        print(f"{label(k)}: old {len(a)} instructions, new {len(b)}, kernel-argument offsets moved in {offs}, "
              f"otherwise differing {diff}, registers / scratch {'same' if fa == fb else f'{fa} -> {fb}'}: "
              f"{'IDENTICAL' if diff == 0 and fa == fb else 'DIFFERENT'}")
    for k in sorted(set(new) - set(old)):
        b, fb = new[k]
        print(f"{label(k)}: new, {len(b)} instructions, " + ", ".join(f"{f} {fb[f]}" for f in _FIGURES if f in fb))
    print(f"{len(old)} kernels of {sys.argv[1]} compared, {bad} differ or are missing; "
          f"{len(set(new) - set(old))} kernels only in {sys.argv[2]}")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
