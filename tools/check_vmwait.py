#!/usr/bin/env python3
"""check_vmwait.py: the hidden-prefetch kernels (proj_p.hpp k_enc_p / k_dec_p: loads the compiler cannot see + s_waitcnt vmcnt(N)
by hand, scan_quad.hpp vm_wait) are only right while the compiler issues exactly the store instructions the counts were
taken from: N stores per wave on a full tile, the same number again on the guarded path of a partial tile.  If a later
compiler merged or split those stores, vm_wait<N> would return before the prefetch has landed.  This compiles the device
code to assembly (no GPU needed) and checks, per kernel, that the hand-written wait is there and that the kernel holds
2 x N tile stores (+ the few prologue stores).  The decoders copy their output tile out of LDS in rounds and wait by a run-time
count of rounds: there the check is one 16-byte store instruction per round (DEC_EXPECT).

The same loads break in a second way: the compiler does not know their destination registers are being written, so it may
copy, spill or reuse them before the data has landed.  The register audit follows every hidden load (a global_load inside
;;#ASMSTART / ;;#ASMEND) through the control-flow graph -- the loop's back edge included, since the prefetch at the end of a
tile is waited for at the top of the next -- to the wait that guards it (the hand-written s_waitcnt vmcnt(N), or a compiler wait
that leaves no more memory operations outstanding than were issued after the load), and fails if an instruction outside the inline-assembly blocks reads or writes one of its destination VGPRs on the
way.  It also reports .private_segment_fixed_size and .vgpr_spill_count of every kernel with hidden loads.  It audits
every kernel of the library that has hidden loads (today k_enc_p, k_dec_p, their float and int16 twins, the pair recurrence kernels
and the 32-frame UREC gate kernels).

The gate kernels (mfma_fused_body.inc EARLY: k_cgate_p<1, 3, .., 32, .., UREC>, both overloads, pair and quad16 streams) request a
tile's states in front of the staging and wait for them behind it, by count (vmcnt(NVC = 2)) where the previous tile was full and
drained (vmcnt(0)) elsewhere (scan_quad.hpp vm_wait_or_drain: both waits in one statement, the drained one first).  Their stores
keep their guards, which every thread passes behind a full tile, so what the count needs is that each copy of the staging (one
per BatchNorm arm, one of them runs) holds exactly NVC store instructions and that no other memory operation lies between the
last request and the waits: GATE_EXPECT.
  python tools/check_vmwait.py [--asm FILE.s | --gate]    (--asm: audit a given assembly file instead of compiling the library;
                                                          --gate: compile and check tools/gate_kernels.hip, the gate kernels alone)
Exit code 0 = consistent."""
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "sparsernns_amd", "csrc", "s5fxp_api.hip")
GATE_SRC = os.path.join(ROOT, "tools", "gate_kernels.hip")
# mangled prefix -> (stores per wave and full tile = the wait count, prologue stores allowed on top of 2 x that)
EXPECT = {
    "_ZN2s57k_enc_pILi3EE": (4, 0), "_ZN2s57k_enc_pILi6EE": (8, 0),
    # float in (proj_p.hpp k_enc_pf: the same body, proj_enc_body.inc): the same stores
    "_ZN2s58k_enc_pfILi3EE": (4, 0), "_ZN2s58k_enc_pfILi6EE": (8, 0),
    # (The encoders of the ragged shapes, k_enc_p<2> / <5>, store conditionally and wait for their prefetch with vmcnt(0); the
    # register audit below covers them.)
    # int16 in (k_enc_ps, the same body again): 8-byte hidden row loads, the same counts
    "_ZN2s58k_enc_psILi3EE": (4, 0), "_ZN2s58k_enc_psILi6EE": (8, 0),
}

# The decoders (proj_dec_body.inc) stage a tile of y in LDS and copy it out in rounds of one 16-byte store per lane; a wave waits for
# its prefetch by the number of rounds it took part in (scan_quad.hpp vm_wait_upto12: a ladder of waits, entered by a run-time
# count).  That count is right while a round is ONE store instruction: mangled prefix -> (rounds at the widest output = 16-byte
# stores of the tile loop, prologue stores on top: RESID publishes its AddCb, one of the two a 16-byte store).  The tile loop
# holds one more store, the element-wise remainder of a tensor's last tile.
DEC_EXPECT = {}
for _k, _name, _rounds in (("7k_dec_p", "int32", 12), ("8k_dec_pf", "float32", 12), ("8k_dec_ps", "int16", 6)):
    for _nt in (2, 3, 5, 6):
        DEC_EXPECT[f"_ZN2s5{_k}ILi{_nt}ELb0EE"] = (_rounds, 0)
        DEC_EXPECT[f"_ZN2s5{_k}ILi{_nt}ELb1EE"] = (_rounds, 2)

# the gate kernels that request their states early: mangled prefix (both overloads) -> stores of the staging per wave = the counted wait
GATE_EXPECT = {
    "_ZN2s59k_cgate_pILi1ELi3ELb0ELb1ELb1ELi32ELb0ELb1ELb1ELb0ELb1EE": 2,   # pair-native stream
    "_ZN2s59k_cgate_pILi1ELi3ELb0ELb1ELb1ELi32ELb0ELb0ELb1ELb0ELb1EE": 2,   # scan-native int16 stream
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
    items, labels, in_asm = [], {}, False   # (a numeric local label `1:` may repeat: labels["1"] lists its positions)
    for line in body.split("\n"):
        t = line.split(";")[0].strip() if not line.strip().startswith(";;#ASM") else line.strip()
        if t == ";;#ASMSTART":
            in_asm = True
        elif t == ";;#ASMEND":
            in_asm = False
        elif re.match(r"^\d+:$", t):
            labels.setdefault(t[:-1], []).append(len(items))
            items.append(("label", t[:-1]))
        elif re.match(r"^[.\w$]+:$", t):
            labels[t[:-1]] = len(items)
            items.append(("label", t[:-1]))
        elif t and not t.startswith("."):
            items.append(("asm" if in_asm else "ins", t))
    return items, labels


def _target(name: str, at: int, labels: dict):
    """Index of a branch target: a named label, or a numeric local one (`1f`: the next `1:`, `1b`: the previous)."""
    m = re.match(r"^(\d+)([fb])$", name)
    if m:
        pos = labels.get(m.group(1), [])
        pos = [p for p in pos if p > at] if m.group(2) == "f" else [p for p in reversed(pos) if p < at]
        return pos[0] if pos else None
    t = labels.get(name)
    return t if isinstance(t, int) else None


def audit_kernel(body: str, reached=None):
    """Violations [(load, offending instruction)] of the hidden loads in one kernel body, and how many hidden loads it has.
    reached (a list): receives (load number, N, n) for every hand-written s_waitcnt vmcnt(N) a path from a hidden load ends at,
    n = memory operations issued on that path since the load."""
    items, labels = _parse(body)
    loads = [i for i, (k, t) in enumerate(items) if k == "asm" and re.match(r"^global_load_dword", t)]
    bad = []
    for li, i in enumerate(loads):
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
                    if kind == "asm" and reached is not None:
                        reached.append((li, int(w.group(1)), n))
                    break   # the hand-written wait (its count is checked by the callers), or one that leaves <= n newer operations
                if kind != "label":
                    mn = t.split(None, 1)[0]
                    if kind == "ins" and not mn.startswith("s_") and _vregs(t.split(None, 1)[1] if " " in t else "") & dest:
                        bad.append((items[i][1], t))
                    if _VMEM.match(mn):
                        n += 1
                    if mn == "s_endpgm":
                        break
                    if mn.startswith("s_cbranch") or mn == "s_branch":
                        tgt = _target(t.split()[-1], j, labels)
                        if tgt is not None:
                            if mn == "s_branch":
                                j = tgt
                                continue
                            stack.append((tgt, n))
                j += 1
    return bad, len(loads)


GATE_ARMS = 3   # mfma_bn.hpp ROW_PACKED, ROW_SHIFTED, ROW_GENERIC


def _region_stores(body: str, load_no: int):
    """[16-byte global stores, other memory operations] among the instructions that lie on some path from hidden load number
    load_no to a hand-written wait: distinct instructions, however many paths cross them."""
    items, labels = _parse(body)
    loads = [i for i, (k, t) in enumerate(items) if k == "asm" and re.match(r"^global_load_dword", t)]
    seen, stack, ops = set(), [loads[load_no] + 1], set()
    while stack:
        j = stack.pop()
        while j < len(items) and j not in seen:
            seen.add(j)
            kind, t = items[j]
            if kind == "asm" and _WAIT.search(t):
                break
            if kind != "label":
                mn = t.split(None, 1)[0]
                if _VMEM.match(mn):
                    ops.add(j)
                if mn == "s_endpgm":
                    break
                if mn.startswith("s_cbranch") or mn == "s_branch":
                    tgt = _target(t.split()[-1], j, labels)
                    if tgt is not None:
                        if mn == "s_branch":
                            j = tgt
                            continue
                        stack.append(tgt)
            j += 1
    st = [j for j in ops if items[j][1].startswith("global_store_dwordx4")]
    return [len(st), len(ops) - len(st)]


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
        reached = []
        viol, n = audit_kernel(m.group(2), reached)
        if not n:
            continue
        km = meta.get(m.group(1), {})
        print(f"{m.group(1)}: {n} hidden loads, private_segment_fixed_size {km.get('.private_segment_fixed_size', '?')}, "
              f"vgpr_spill_count {km.get('.vgpr_spill_count', '?')}: {'ok' if not viol else 'REGISTER TOUCHED BEFORE ITS WAIT'}")
        for load, ins in viol[:8]:
            print(f"    {load}  <-  {ins}")
        bad += len(viol)
        gate = [nv for key, nv in GATE_EXPECT.items() if m.group(1).startswith(key)]
        if gate:
            # between the LAST request and the waits lie the staging's copies, one per BatchNorm arm (mfma_bn.hpp ROW_*: the arm
            # is chosen per call, the copies exclude each other): NVC 16-byte stores each and no other memory operation; both
            # waits are reached, and no other hand-written count
            waits = set(N for li, N, c in reached if N >= 0)
            stores = _region_stores(m.group(2), n - 1)
            ok = waits == {0, gate[0]} and stores == [GATE_ARMS * gate[0], 0]
            print(f"    between the last request and the waits: {stores[0]} global_store_dwordx4 (expected {GATE_ARMS} arms x {gate[0]}), "
                  f"{stores[1]} other memory operations, hand-written counts reached {sorted(waits)}: {'ok' if ok else 'MISMATCH'}")
            bad += 0 if ok else 1
    return bad


def main(argv) -> int:
    if len(argv) > 2 and argv[1] == "--asm":
        return 1 if audit(open(argv[2]).read()) else 0
    gate_only = argv[1:] == ["--gate"]
    with tempfile.TemporaryDirectory() as d:
        out = os.path.join(d, "k.s")
        subprocess.check_call(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-Wno-unused-value", "-S",
                               "--cuda-device-only", "-o", out, GATE_SRC if gate_only else SRC], stderr=subprocess.DEVNULL)
        text = open(out).read()
    bad = 0
    for key, (n, extra) in ({} if gate_only else EXPECT).items():
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
    for key, (rounds, extra) in ({} if gate_only else DEC_EXPECT).items():
        m = re.search(r"^" + re.escape(key) + r"[^\n]*\n(.*?)^\.Lfunc_end", text, re.S | re.M)
        if not m:
            print(f"{key}: kernel not found")
            bad += 1
            continue
        body = m.group(1)
        stores = len(re.findall(r"^\s*global_store", body, re.M))
        x4 = len(re.findall(r"^\s*global_store_dwordx4", body, re.M))
        rungs = [len(re.findall(rf"s_waitcnt vmcnt\({n}\)\s*$", body, re.M)) for n in range(13)]
        ok = min(rungs) >= 1 and x4 == rounds + (1 if extra else 0) and stores == rounds + 1 + extra
        print(f"{key}: {x4} 16-byte stores (expected {rounds + (1 if extra else 0)}), {stores} stores in all (expected {rounds + 1 + extra}), "
              f"wait ladder {'complete' if min(rungs) >= 1 else 'INCOMPLETE'}: {'ok' if ok else 'MISMATCH'}")
        bad += 0 if ok else 1
    for key in GATE_EXPECT:   # both overloads of each (CGateArgs, CGateFoldArgs)
        found = len(re.findall(r"^" + re.escape(key) + r"\w*:", text, re.M))
        if found != 2:
            print(f"{key}: {found} kernels (expected the two overloads)")
            bad += 1
    bad += audit(text)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
