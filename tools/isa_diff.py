"""Compare two gfx950 assembly listings kernel by kernel.

    hipcc <the library's flags> --cuda-device-only -S csrc/svm.hip -o new.s      (once per side)
    python tools/isa_diff.py parent.s new.s

Kernels are paired by demangled name.  Per kernel: the resources the code object declares on both sides, the instruction count
of both sides, the index of the first differing instruction and of the last v_mfma_* (comments, directives and label names
are ignored).  A kernel whose first difference comes after its last MFMA kept its main loop: only its epilogue moved ("tier 1");
one that differs earlier is "tier 2".  Kernels on one side only are listed and make the exit status non-zero.
"""
import re
import shutil
import subprocess
import sys

FIELDS = (".vgpr_count", ".sgpr_count", ".vgpr_spill_count", ".private_segment_fixed_size", ".group_segment_fixed_size")


def demangle(names):
    tool = shutil.which("llvm-cxxfilt") or shutil.which("c++filt") or "/opt/rocm/lib/llvm/bin/llvm-cxxfilt"
    out = subprocess.run([tool], input="\n".join(names), capture_output=True, text=True, check=True).stdout.split("\n")
    return dict(zip(names, (o.replace("(anonymous namespace)::", "") for o in out)))


def parse(path):
    """{mangled name: (instructions, {field: value})}"""
    body, meta, name, entry = {}, {}, None, None
    for line in open(path):
        s = line.split(";")[0].strip()
        m = re.match(r"^(\w+):$", s)
        if m and not s.startswith(".L") and name is None:
            name, body[m.group(1)] = m.group(1), []
            continue
        if name is not None:
            if s.startswith((".Lfunc_end", ".size")):                   # .size: the end of a data symbol
                name = None
            elif s and not s.startswith(".") and not s.endswith(":"):
                body[name].append(re.sub(r"\.LBB\w+", ".L", s))      # label names differ with the function's position in the file
            continue
        m = re.match(r"^(  - |    )(\.\w+):\s*(.*)$", line)              # a key of an entry of amdhsa.kernels
        if m:
            if m.group(1) == "  - ":
                entry = {}
            entry[m.group(2)] = m.group(3).strip()
            if m.group(2) == ".name":
                meta[m.group(3).strip()] = entry
    return {n: (ins, meta[n]) for n, ins in body.items() if n in meta}


def main():
    a, b = parse(sys.argv[1]), parse(sys.argv[2])
    names = demangle(sorted(set(a) | set(b)))
    tiers = {1: 0, 2: 0}
    worse = []
    for n in sorted(set(a) & set(b), key=names.get):
        (ia, ma), (ib, mb) = a[n], b[n]
        first = next((i for i, (x, y) in enumerate(zip(ia, ib)) if x != y), None if len(ia) == len(ib) else min(len(ia), len(ib)))
        last_mfma = max([i for i, x in enumerate(ia) if x.startswith("v_mfma_")], default=-1)
        tier = 1 if first is None or first > last_mfma else 2
        tiers[tier] += 1
        print("%s\n    %s | instructions %d -> %d | first difference %s | last v_mfma %d | %s" % (
            names[n], " ".join("%s %s -> %s" % (f[1:], ma.get(f), mb.get(f)) for f in FIELDS), len(ia), len(ib),
            "none" if first is None else first, last_mfma, "identical" if first is None else "tier %d" % tier))
        worse += ["%s: %s %s -> %s" % (names[n], f, ma.get(f), mb.get(f)) for f in FIELDS if int(mb.get(f, 0)) > int(ma.get(f, 0))]
    only = [(side, names[n]) for side, s in (("first", set(a) - set(b)), ("second", set(b) - set(a))) for n in sorted(s)]
    for side, n in only:
        print("only in the %s listing: %s" % (side, n))
    print("%d kernels paired: %d tier 1 (%d of them identical), %d tier 2; %d on one side only; %d resource figures went up" % (
        len(set(a) & set(b)), tiers[1], sum(a[n][0] == b[n][0] for n in set(a) & set(b)), tiers[2], len(only), len(worse)))
    for w in worse:
        print("went up: " + w)
    return 1 if only else 0


if __name__ == "__main__":
    sys.exit(main())
