#!/usr/bin/env python3
"""Per-kernel comparison of two device assemblies of the library's translation unit.

usage: hipcc --offload-arch=gfx950 -O3 -std=c++17 --cuda-device-only -S -o A.s sparsernns_amd/csrc/s5fxp_api.hip   (each tree)
       tools/disasm_compare.py [--strict] PARENT.s NEW.s
Per kernel the instruction text (labels renumbered, comments and directives dropped) is compared; prints the kernels whose
streams differ, with the number of differing instructions, and those only one side has.  --strict: exit status 1 when any
kernel's stream differs or exists on one side only (the gate of a refactor that must not change device code).  No GPU needed."""
import difflib
import re
import subprocess
import sys


def kernels(path):
    out, cur, name, funcs = {}, None, None, set()
    for line in open(path, errors="replace"):
        m = re.match(r"^\s*\.type\s+(_Z\w+),@function", line)
        if m:
            funcs.add(m.group(1))
        m = re.match(r"^(_Z\w+):\s*(;.*)?$", line)
        if m and m.group(1) in funcs:
            name, cur = m.group(1), []
            out[name] = cur
            continue
        if cur is None:
            continue
        s = line.split(";")[0].strip()
        if s.startswith(".Lfunc_end"):
            cur = None
            continue
        if not s or s.startswith("."):
            if re.match(r"^\.LBB\d+_\d+:", s):
                cur.append("L:")
            continue
        cur.append(re.sub(r"\.LBB\d+_\d+", "L", s))
    names = subprocess.run(["c++filt"], input="\n".join(out), capture_output=True, text=True).stdout.splitlines()
    return {short(n): v for n, v in zip(names, out.values())}


def short(n):
    n = n.replace("void s5::", "").replace("s5::", "")
    m = re.match(r"^(.*?)\((.*)\)$", n)
    if not m:
        return n
    tag = " [fold]" if "CGateFoldArgs" in m.group(2) else " [lazy]" if "ResidLazyArgs" in m.group(2) else ""
    return m.group(1) + tag


def main():
    args = [x for x in sys.argv[1:] if x != "--strict"]
    a, b = kernels(args[0]), kernels(args[1])
    both = [k for k in a if k in b]
    same = [k for k in both if a[k] == b[k]]
    print(f"kernels: parent {len(a)}, this commit {len(b)}; identical instruction streams: {len(same)}")
    print("\nchanged:")
    for k in both:
        if a[k] != b[k]:
            sm = difflib.SequenceMatcher(None, a[k], b[k], autojunk=False)
            nd = sum(max(i2 - i1, j2 - j1) for t, i1, i2, j1, j2 in sm.get_opcodes() if t != "equal")
            print(f"  {k}: {len(a[k])} -> {len(b[k])} instructions, {nd} differ")
    for title, x, y in (("only in the parent", a, b), ("only in this commit", b, a)):
        only = [k for k in x if k not in y]
        if only:
            print(f"\n{title}:")
            for k in only:
                print(f"  {k}: {len(x[k])} instructions")
    return 1 if "--strict" in sys.argv[1:] and not len(same) == len(a) == len(b) else 0


if __name__ == "__main__":
    sys.exit(main())
