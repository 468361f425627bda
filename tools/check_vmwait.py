#!/usr/bin/env python3
"""check_vmwait.py: the hidden-prefetch kernels (proj_p.hpp k_enc_p / k_dec_p: loads the compiler cannot see + s_waitcnt vmcnt(N)
by hand, scan_quad.hpp vm_wait) are only right while the compiler issues exactly the store instructions the counts were
taken from: N stores per wave on a full tile, the same number again on the guarded path of a partial tile.  If a later
compiler merged or split those stores, vm_wait<N> would return before the prefetch has landed.  This compiles the device
code to assembly (no GPU needed) and checks, per kernel, that the hand-written wait is there and that the kernel holds
2 x N tile stores (+ the few prologue stores).

The same loads break in a second way: the compiler does not know their destination registers are being written, so it may
copy, spill or reuse them before the data has landed.  The register audit follows every hidden load (a global_load inside
;;#ASMSTART / ;;#ASMEND) through the control-flow graph -- the loop's back edge included, since the prefetch at the end of a
tile is waited for at the top of the next -- to the wait that guards it (the hand-written s_waitcnt vmcnt(N), or a compiler wait
that leaves no more memory operations outstanding than were issued after the load), and fails if an instruction outside the inline-assembly blocks reads or writes one of its destination VGPRs on the
way.  It also reports .private_segment_fixed_size and .vgpr_spill_count of every kernel with hidden loads.  It audits
every kernel of the library that has hidden loads (today k_enc_p, k_dec_p, their float and int16 twins and the pair recurrence kernels).
  python tools/check_vmwait.py [--asm FILE.s]    (--asm: audit a given assembly file instead of compiling the library)
Exit code 0 = consistent."""
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "sparsernns_amd", "csrc", "s5fxp_api.hip")
# mangled prefix -> (stores per wave and full tile = the wait count, prologue stores allowed on top of 2 x that)
EXPECT = {
    "_ZN2s57k_dec_pILi3ELb0EE": (48, 0), "_ZN2s57k_dec_pILi6ELb0EE": (48, 0),
    "_ZN2s57k_dec_pILi3ELb1EE": (48, 2), "_ZN2s57k_dec_pILi6ELb1EE": (48, 2),
    "_ZN2s57k_enc_pILi3EE": (4, 0), "_ZN2s57k_enc_pILi6EE": (8, 0),
    # float in / float out (proj_p.hpp k_enc_pf / k_dec_pf: the same bodies, proj_enc_body.inc / proj_dec_body.inc): the same stores
    "_ZN2s58k_dec_pfILi3ELb0EE": (48, 0), "_ZN2s58k_dec_pfILi6ELb0EE": (48, 0),
    "_ZN2s58k_dec_pfILi3ELb1EE": (48, 2), "_ZN2s58k_dec_pfILi6ELb1EE": (48, 2),
    "_ZN2s58k_enc_pfILi3EE": (4, 0), "_ZN2s58k_enc_pfILi6EE": (8, 0),
    # the decoders of the ragged shapes (H = 48, 144): the same 48 stores.  (Their encoders, k_enc_p<2> / <5>, store
    # conditionally and wait for their prefetch with vmcnt(0); the register audit below covers them.)
    "_ZN2s57k_dec_pILi2ELb0EE": (48, 0), "_ZN2s57k_dec_pILi5ELb0EE": (48, 0),
    "_ZN2s57k_dec_pILi2ELb1EE": (48, 2), "_ZN2s57k_dec_pILi5ELb1EE": (48, 2),
    "_ZN2s58k_dec_pfILi2ELb0EE": (48, 0), "_ZN2s58k_dec_pfILi5ELb0EE": (48, 0),
    "_ZN2s58k_dec_pfILi2ELb1EE": (48, 2), "_ZN2s58k_dec_pfILi5ELb1EE": (48, 2),
    # int16 in / int16 out (k_enc_ps / k_dec_ps, the same bodies again): 8-byte hidden row loads, 2-byte output stores, the same counts
    "_ZN2s58k_dec_psILi3ELb0EE": (48, 0), "_ZN2s58k_dec_psILi6ELb0EE": (48, 0),
    "_ZN2s58k_dec_psILi3ELb1EE": (48, 2), "_ZN2s58k_dec_psILi6ELb1EE": (48, 2),
    "_ZN2s58k_dec_psILi2ELb0EE": (48, 0), "_ZN2s58k_dec_psILi5ELb0EE": (48, 0),
    "_ZN2s58k_dec_psILi2ELb1EE": (48, 2), "_ZN2s58k_dec_psILi5ELb1EE": (48, 2),
    "_ZN2s58k_enc_psILi3EE": (4, 0), "_ZN2s58k_enc_psILi6EE": (8, 0),
}


_VMEM = re.compile(r"^(global|buffer|flat|scratch)_(load|store|atomic)")
_WAIT = re.compile(r"s_waitcnt\b.*\bvmcnt\((\d+)\)")


def _vregs(operands: str) -> set:
    """VGPR numbers named in an operand string: v7, v[4:7]."""
    out = set()
    for a, b in re.findall(r"\bv\[(\d+):(\d+)\]", operands):
        out.update(range(int(a), int(b) + 1))
    out.update(int(v) for v in re.findall(r"(?<![\w\[:])v(\d+)\b", operands))
    return out


def _parse(body: str):
    """[(kind, text)] of a kernel body: kind 'asm' (inside ;;#ASMSTART/END), 'ins', 'label'; plus label -> index."""
    items, labels, in_asm = [], {}, False
    for line in body.split("\n"):
        t = line.split(";")[0].strip() if not line.strip().startswith(";;#ASM") else line.strip()
        if t == ";;#ASMSTART":
            in_asm = True
        elif t == ";;#ASMEND":
            in_asm = False
        elif re.match(r"^[.\w$]+:$", t):
            labels[t[:-1]] = len(items)
            items.append(("label", t[:-1]))
        elif t and not t.startswith("."):
            items.append(("asm" if in_asm else "ins", t))
    return items, labels


def audit_kernel(body: str):
    """Violations [(load, offending instruction)] of the hidden loads in one kernel body, and how many hidden loads it has."""
    items, labels = _parse(body)
    loads = [i for i, (k, t) in enumerate(items) if k == "asm" and re.match(r"^global_load_dword", t)]
    bad = []
    for i in loads:
        op, rest = (items[i][1].split(None, 1) + [""])[:2]
        dest = _vregs(rest.split(",")[0])
        seen, stack = set(), [(i + 1, 0)]
        while stack:
            j, n = stack.pop()
            while j < len(items):
                key = (j, min(n, 64))
                if key in seen:
                    break
                seen.add(key)
                kind, t = items[j]
                w = _WAIT.search(t)
                if w and (kind == "asm" or n >= int(w.group(1))):
                    break   # the hand-written wait (its count is checked above), or one that leaves <= n newer operations
                if kind != "label":
                    mn = t.split(None, 1)[0]
                    if kind == "ins" and not mn.startswith("s_") and _vregs(t.split(None, 1)[1] if " " in t else "") & dest:
                        bad.append((items[i][1], t))
                    if _VMEM.match(mn):
                        n += 1
                    if mn == "s_endpgm":
                        break
                    if mn.startswith("s_cbranch") or mn == "s_branch":
                        tgt = t.split()[-1]
                        if tgt in labels:
                            if mn == "s_branch":
                                j = labels[tgt]
                                continue
                            stack.append((labels[tgt], n))
                j += 1
    return bad, len(loads)


def kernel_meta(text: str) -> dict:
    """name -> {'.private_segment_fixed_size': .., '.vgpr_spill_count': ..} from the code object metadata."""
    meta = {}
    for entry in re.split(r"\n  - ", text[text.find("amdhsa.kernels:"):]):
        name = re.search(r"^\s*\.name:\s+(\S+)", entry, re.M)
        if name:
            meta[name.group(1)] = {k: int(v) for k, v in re.findall(r"^\s*(\.private_segment_fixed_size|\.vgpr_spill_count):\s+(\d+)",
                                                                   entry, re.M)}
    return meta


def audit(text: str) -> int:
    """Register audit of every kernel of an assembly file that issues hidden loads; returns the number of violations."""
    meta = kernel_meta(text)
    bad = 0
    for m in re.finditer(r"^(\w+):[^\n]*\n(.*?)^\.Lfunc_end", text, re.S | re.M):
        viol, n = audit_kernel(m.group(2))
        if not n:
            continue
        km = meta.get(m.group(1), {})
        print(f"{m.group(1)}: {n} hidden loads, private_segment_fixed_size {km.get('.private_segment_fixed_size', '?')}, "
              f"vgpr_spill_count {km.get('.vgpr_spill_count', '?')}: {'ok' if not viol else 'REGISTER TOUCHED BEFORE ITS WAIT'}")
        for load, ins in viol[:8]:
            print(f"    {load}  <-  {ins}")
        bad += len(viol)
    return bad


def main(argv) -> int:
    if len(argv) > 2 and argv[1] == "--asm":
        return 1 if audit(open(argv[2]).read()) else 0
    with tempfile.TemporaryDirectory() as d:
        out = os.path.join(d, "k.s")
        subprocess.check_call(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-Wno-unused-value", "-S",
                               "--cuda-device-only", "-o", out, SRC], stderr=subprocess.DEVNULL)
        text = open(out).read()
    bad = 0
    for key, (n, extra) in EXPECT.items():
        m = re.search(r"^" + re.escape(key) + r"[^\n]*\n(.*?)^\.Lfunc_end", text, re.S | re.M)
        if not m:
            print(f"{key}: kernel not found")
            bad += 1
            continue
        body = m.group(1)
        stores = len(re.findall(r"^\s*global_store", body, re.M))
        waits = len(re.findall(rf"s_waitcnt vmcnt\({n}\)\s*$", body, re.M))
        ok = waits >= 1 and stores == 2 * n + extra
        print(f"{key}: {stores} stores (expected {2 * n + extra}), {waits} x vmcnt({n}): {'ok' if ok else 'MISMATCH'}")
        bad += 0 if ok else 1
    bad += audit(text)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
