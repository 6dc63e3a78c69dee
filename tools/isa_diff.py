#!/usr/bin/env python3
"""Per-kernel comparison of two assembly files from `make -C beatrice_amd/csrc asm`:

    python3 tools/isa_diff.py OLD.s NEW.s

For every kernel symbol: `identical` (the same text once comments are dropped and the
function numbers in .LBB<n>_ / .Lfunc_end<n> labels are normalised), `same instructions` (equal
instruction count and equal mnemonic histogram: a reordering or commuted operands), `different`
(with both counts), or `only in OLD` / `only in NEW`; next to it the kernel's SGPRs, VGPRs,
LDS bytes, scratch bytes and occupancy from its resource-usage block (old -> new where they
differ). Exit status 1 when a kernel present in both files is `different` or its resources changed.
"""
import collections
import re
import subprocess
import sys

RES = [("sgpr", "TotalNumSgprs"), ("vgpr", "NumVgprs"), ("lds", "LDSByteSize"), ("scratch", "ScratchSize"),
       ("occ", "Occupancy")]


def kernels(path):
    """{symbol: (normalised instruction lines, {resource: value})}"""
    text = open(path).read()
    out = {}
    for sym in re.findall(r"^\t\.amdhsa_kernel (\S+)$", text, re.M):
        body = text.split("\n%s:" % sym, 1)[1]
        code, info = body.split("\n\t.section\t.rodata", 1)[0], body.split("; Kernel info:", 1)[1]
        lines = []
        for ln in code.splitlines():
            ln = re.sub(r"\.(LBB|Lfunc_end)\d+", r".\1", ln.split(";", 1)[0]).strip()
            if ln:
                lines.append(" ".join(ln.split()))
        out[sym] = (lines, {k: int(re.search(r"^; %s: (\d+)" % key, info, re.M).group(1)) for k, key in RES})
    return out


def demangled(syms):
    try:
        names = subprocess.run(["c++filt"], input="\n".join(syms), capture_output=True, text=True, check=True)
        short = (re.sub(r"^void |\(anonymous namespace\)::|\([^()]*\)$", "", n) for n in names.stdout.splitlines())
        return dict(zip(syms, short))
    except (OSError, subprocess.CalledProcessError):
        return {s: s for s in syms}


def histogram(lines):
    return collections.Counter(ln.split()[0] for ln in lines if not ln.endswith(":") and not ln.startswith("."))


def main():
    old, new = kernels(sys.argv[1]), kernels(sys.argv[2])
    names = demangled(sorted(set(old) | set(new)))
    bad = 0
    for sym in sorted(names, key=names.get):
        if sym not in old or sym not in new:
            print("%-18s %s" % ("only in OLD" if sym in old else "only in NEW", names[sym]))
            continue
        (lo, ro), (ln, rn) = old[sym], new[sym]
        ho, hn = histogram(lo), histogram(ln)
        no, nn = sum(ho.values()), sum(hn.values())
        cls = "identical" if lo == ln else "same instructions" if ho == hn else "different %d -> %d" % (no, nn)
        res = " ".join("%s %s" % (k, ro[k] if ro[k] == rn[k] else "%d->%d" % (ro[k], rn[k])) for k, _ in RES)
        bad += cls.startswith("different") or ro != rn
        print("%-18s %5d  %s  %s" % (cls, nn, res, names[sym]))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
